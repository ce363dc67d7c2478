"""Adaptive sampling restated (rtggx_set_sample_map; include/rtggx.h, DESIGN.md "Adaptive sampling").

The frames.  FrameIndex enters a frame nowhere but getSampleParam, so the mapped frame of setting N at frame index F equals, on the blocks
whose count is c, the uniform frame of c samples at FrameIndex' = F N / c of the restatement (tests/restatement.py): that frame has exactly
the indices F N + k for k < c and packs with 1 / c.  mapped_frame() composes the expected images block by block from at most four such
frames, one per distinct count.  Each is traced with the visibility words of the other blocks cleared, so that the ray counts add up to
the mapped frame's exactly; RayTracingOut1 is put back before each, so that what a frame leaves untouched (metallic >= 1) is the previous
frame's word in every one of them.

The policy that was measured and left out of the library (tests/test_adaptive_host.py, DESIGN.md "Adaptive sampling").  policy() derives a
map from the sums of an accumulation (RTGGX_BUF_ACC_REFL / _DIFF) in numpy float32, one rounding per operation: per covered pixel, with n
the accumulated frames,
    inv = 1 / n;  for each image j: m = A_j.xyz * inv;  Y_j = (0.25 m.r + 0.5 m.g) + 0.25 m.b;  q = A_j.w * inv;  var_j = max(q - Y_j Y_j, 0)
    Y = Y0 + Y1;  var = var0 + var1;  d = Y + 0.5;  d2 = d d;  v = (0.25 var) / (d2 d2)
-- the luma variance behind the tone curve Y / (Y + 0.5), to first order; a NaN stays one --, per block the sum of v over its 64 lanes added
pairwise, adjacent lanes first, divided by the covered pixels and multiplied by the frames' sample count S, and the thresholds: 1 up to
the target, 2 up to twice, 4 up to four times it, else 8 (a NaN falls through to 8), then min(count, N); a block without a covered pixel
gets 1."""
import numpy as np

from gpu_support import FRAME_INDEX_OFFSET
from oracle import oracle as O

BLOCK = 8
COUNTS = (1, 2, 4, 8)
FRAME_BUFS = (O.BUF_RT_REFL, O.BUF_RT_DIFF, O.BUF_NORMAL, O.BUF_ROUGH_METAL, O.BUF_VELOCITY)      # what a ray trace writes


def blocks_of(W, H):
    """(blocks_y, blocks_x) of a frame of W x H pixels."""
    return (H + BLOCK - 1) // BLOCK, (W + BLOCK - 1) // BLOCK


def per_pixel(blocks, W, H):
    """The block map [blocks_y, blocks_x] spread over the pixels: [H, W]."""
    b = np.asarray(blocks)
    assert b.shape == blocks_of(W, H), (b.shape, W, H)
    return np.repeat(np.repeat(b, BLOCK, axis=0), BLOCK, axis=1)[:H, :W]


def _set_frame_index(o, index):
    fc = o.get_frame_constants()
    fc[FRAME_INDEX_OFFSET:FRAME_INDEX_OFFSET + 4] = np.array([index], np.uint32).view(np.uint8)
    o.set_frame_constants(fc.tobytes())


def _frame_index(o):
    return int(o.get_frame_constants()[FRAME_INDEX_OFFSET:FRAME_INDEX_OFFSET + 4].view(np.uint32)[0])


def mapped_frame(o, blocks):
    """The ray trace of a restatement Oracle `o` (its samples setting is N, its visibility pass done, its constants the frame's) under the
    map `blocks` (uint8 [blocks_y, blocks_x]; counts above N count as N).  Leaves the composed frame in the oracle's buffers, as o.ray_trace()
    would, and returns the number of rays."""
    N, F = o.samples, _frame_index(o)
    counts = per_pixel(np.minimum(np.asarray(blocks, np.uint32), N), o.W, o.H)
    vis = o.buffer(O.BUF_VISIBILITY)
    diff_before = o.buffer(O.BUF_RT_DIFF)
    composed = {b: None for b in FRAME_BUFS}
    rays = 0
    try:
        for c in COUNTS:
            here = counts == c
            if not here.any():
                continue
            o.buffer(O.BUF_VISIBILITY, copy=False)[...] = np.where(here, vis, 0)
            o.buffer(O.BUF_RT_DIFF, copy=False)[...] = diff_before
            o.set_samples_per_pixel(c)
            _set_frame_index(o, F * N // c)
            rays += o.ray_trace()
            for b in FRAME_BUFS:
                got = o.buffer(b)
                composed[b] = got if composed[b] is None else np.where(here, got, composed[b])
    finally:
        o.set_samples_per_pixel(N)
        _set_frame_index(o, F)
        o.buffer(O.BUF_VISIBILITY, copy=False)[...] = vis
    for b in FRAME_BUFS:
        o.buffer(b, copy=False)[...] = composed[b]
    return rays


def checkerboard(W, H, a=1, b=8):
    by, bx = blocks_of(W, H)
    y, x = np.mgrid[0:by, 0:bx]
    return np.where((x + y) & 1, b, a).astype(np.uint8)


def one_in_a_sea(W, H, sea=1, one=8, at=None):
    """`one` in one block (default: the middle one) of a map of `sea`."""
    by, bx = blocks_of(W, H)
    m = np.full((by, bx), sea, np.uint8)
    m[at if at is not None else (by // 2, bx // 2)] = one
    return m


def random_map(W, H, seed):
    return np.random.default_rng(seed).choice(np.array(COUNTS, np.uint8), size=blocks_of(W, H))


# ---- the policy ----------------------------------------------------------------------------------------------------------------------
def pairwise_sum(x):
    """The last axis (a power of two long) added pairwise, adjacent pairs first, level by level, in float32."""
    x = np.asarray(x, np.float32)
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def pixel_variance(acc_refl, acc_diff, frames):
    """v per pixel: float32 [H, W] from the two sums [H, W, 4] and the frame count."""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = f(1.0) / f(frames)

        def moments(A):
            A = np.asarray(A, np.float32)
            r, g, b = A[..., 0] * inv, A[..., 1] * inv, A[..., 2] * inv
            Y = (f(0.25) * r + f(0.5) * g) + f(0.25) * b
            q = A[..., 3] * inv
            t = q - Y * Y
            return Y, np.where(t < 0, f(0.0), t)      # (a NaN stays)
        Y0, var0 = moments(acc_refl)
        Y1, var1 = moments(acc_diff)
        Y, var = Y0 + Y1, var0 + var1
        d = Y + f(0.5)
        d2 = d * d
        return ((f(0.25) * var) / (d2 * d2)).astype(np.float32)


def block_lanes(image, fill):
    """[H, W] -> [blocks_y, blocks_x, 64], lane 8 (y & 7) + (x & 7), pixels beyond the frame holding `fill`."""
    H, W = image.shape
    by, bx = blocks_of(W, H)
    full = np.full((by * BLOCK, bx * BLOCK), fill, image.dtype)
    full[:H, :W] = image
    return full.reshape(by, BLOCK, bx, BLOCK).transpose(0, 2, 1, 3).reshape(by, bx, BLOCK * BLOCK)


def block_values(sums, covered, S):
    """x = (sum / covered) * S per block, float32 (a block without a covered pixel: the sum itself, which nobody reads)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return (np.asarray(sums, np.float32) / np.maximum(covered, 1).astype(np.float32)) * np.float32(S)


def counts(x, covered, target, N):
    """The thresholds: 1 if x <= target, else 2 if x <= 2 target, else 4 if x <= 4 target, else 8 -- a NaN compares false every time --,
    then min(count, N); a block without a covered pixel gets 1."""
    f = np.float32
    t = f(target)
    with np.errstate(invalid="ignore"):
        c = np.where(x <= t, 1, np.where(x <= f(2.0) * t, 2, np.where(x <= f(4.0) * t, 4, 8)))
    return np.where(np.asarray(covered) > 0, np.minimum(c, N), 1).astype(np.uint8)


def blocks_from_sums(acc_refl, acc_diff, visibility, frames, S):
    """(x, covered) per block from RTGGX_BUF_ACC_REFL / _DIFF [H, W, 4], the visibility words [H, W], n = frames and the frames' sample count S."""
    cov = np.asarray(visibility) != 0
    v = np.where(cov, pixel_variance(acc_refl, acc_diff, frames), np.float32(0.0)).astype(np.float32)
    covered = block_lanes(cov, False).sum(axis=-1)
    return block_values(pairwise_sum(block_lanes(v, np.float32(0.0))), covered, S), covered


def policy(acc_refl, acc_diff, visibility, frames, S, target, N):
    """The map uint8 [blocks_y, blocks_x]; N is the samples-per-pixel setting."""
    x, covered = blocks_from_sums(acc_refl, acc_diff, visibility, frames, S)
    return counts(x, covered, target, N)
