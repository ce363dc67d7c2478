"""Adaptive sampling without a GPU (rtggx_set_sample_map, rtggx_read_sample_map; include/rtggx.h, DESIGN.md "Adaptive sampling"): the ABI
surface, the composition rule of tests/adaptive_ref.py against the CPU restatement's uniform frames, and the policy that was measured and
NOT shipped -- a map from the accumulated variance, restated in tests/adaptive_ref.py: its known answers, and the measurement that decided
against it (at equal rays it leaves no less error than a uniform count; DESIGN.md has the figures).

`python tests/test_adaptive_host.py` writes that measurement to tests/golden/adaptive_convergence.json."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import accum_ref as AR  # noqa: E402
import adaptive_ref as A  # noqa: E402
import host_support as HS  # noqa: E402
from oracle import oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "adaptive_convergence.json")
W, H = 96, 54


def _ref():
    import restatement as RS
    return RS


# ---- 1. surface and bindings ---------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound_and_no_buffer_id_was_added(built):
    import ctypes as C
    from raytracedggx_amd import app
    HS.declared_exported_bound("rtggx_set_sample_map", r"\bint\s+rtggx_set_sample_map\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*const\s+uint8_t\s*\*\s*counts\s*,\s*uint32_t\s+blocks_x\s*,\s*uint32_t\s+blocks_y\s*\)")
    HS.declared_exported_bound("rtggx_read_sample_map", r"\bint\s+rtggx_read_sample_map\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*uint8_t\s*\*\s*counts\s*,\s*uint32_t\s+capacity\s*,\s*uint32_t\s*\*\s*blocks_x\s*,\s*uint32_t\s*\*\s*blocks_y\s*\)")
    header = open(os.path.join(ROOT, "include", "rtggx.h")).read()
    assert re.search(r"\bRTGGX_BUF_COUNT\s*=\s*28\b", header)      # the map has a read function of its own, no buffer id
    assert "rtggx_app_set_sample_map" in app.HOST_EXPORTS and hasattr(C.CDLL(app.HOST_LIB_PATH), "rtggx_app_set_sample_map")
    assert "rtggx_sample_map_from_accumulation" not in header      # the policy call was measured and left out (DESIGN.md "Adaptive sampling")
    assert callable(getattr(app.RayTracedGGX, "set_sample_map", None))


# ---- 2. the composition rule ---------------------------------------------------------------------------------------------------------
def _scene(o, metallic, vndf=False):
    HS.scene(o, "bunny.obj", metallic=metallic, vndf=vndf, frame=1)


def _frame_words(o):
    return {b: o.buffer(b) for b in A.FRAME_BUFS}


@pytest.mark.parametrize("metallic", [(1.0, 1.0), (0.25, 0.5)], ids=["metal", "diffuse"])
@pytest.mark.parametrize("N", [8, 4])
def test_composition_against_the_uniform_frames(built, metallic, N):
    """All N is the N-sample frame; all 1 is the one-sample frame at F N; under a checkerboard every block holds the words of the uniform
    frame of its count at F N / c, whose unpacked values are ray_trace_f32's images to the format's rounding; the rays add up."""
    RS = _ref()
    o, u = RS.Oracle(W, H, samples=N, entry="spp"), RS.Oracle(W, H, samples=N, entry="spp")
    try:
        _scene(o, metallic); _scene(u, metallic)
        F = 5
        for x in (o, u):
            HS.set_frame_index(x, F); HS.poison(x)
        by, bx = A.blocks_of(W, H)
        # all N
        rays = A.mapped_frame(o, np.full((by, bx), N, np.uint8))
        assert rays == u.ray_trace() > 0
        for b in A.FRAME_BUFS:
            np.testing.assert_array_equal(o.buffer(b), u.buffer(b), err_msg="all N: buffer %d" % b)
        rays_n = rays
        # all 1
        rays = A.mapped_frame(o, np.ones((by, bx), np.uint8))
        u.set_samples_per_pixel(1); HS.set_frame_index(u, F * N)
        assert rays == u.ray_trace() and 0 < rays < rays_n
        for b in A.FRAME_BUFS:
            np.testing.assert_array_equal(o.buffer(b), u.buffer(b), err_msg="all 1: buffer %d" % b)
        # the checkerboard (counts above N clamped)
        board = A.checkerboard(W, H)
        rays_b = A.mapped_frame(o, board)
        assert rays < rays_b < rays_n
        got = _frame_words(o)
        counts = A.per_pixel(np.minimum(board, N), W, H)
        covered = o.buffer(O.BUF_VISIBILITY) != 0
        for c in np.unique(counts):
            u.set_samples_per_pixel(int(c)); HS.set_frame_index(u, F * N // int(c))
            u.ray_trace()
            here = counts == c
            for b in A.FRAME_BUFS:
                np.testing.assert_array_equal(got[b][here], u.buffer(b)[here], err_msg="checkerboard, count %d: buffer %d" % (c, b))
            _, refl, _ = u.ray_trace_f32(int(c))
            at = here & covered & np.isfinite(refl).all(axis=-1)
            word, f32 = O.unpack_r11g11b10f(got[O.BUF_RT_REFL])[at].astype(np.float64), refl[at].astype(np.float64)
            small = f32 < 2.0 ** -13      # (below the format's normal range the spacing is absolute)
            assert (np.abs(word - f32)[~small] <= 2.0 ** -6 * f32[~small]).all() and (np.abs(word - f32)[small] <= 2.0 ** -19).all()
    finally:
        o.close(); u.close()


# ---- 3. the known answers of the policy that was left out (tests/adaptive_ref.py) --------------------------------------------------------
def _sums_of(values):
    """Sums [H, W, 4] of an accumulation of two frames whose reflection luma is Y -/+ s per pixel (grey: r = g = b), for `values` = (Y, s)
    [H, W, 2]: mean Y, variance s^2; the diffuse sums zero."""
    Y, s = values[..., 0].astype(np.float64), values[..., 1].astype(np.float64)
    a = np.zeros(values.shape[:2] + (4,), np.float32)
    a[..., 0] = a[..., 1] = a[..., 2] = (2.0 * Y).astype(np.float32)
    a[..., 3] = ((Y - s) ** 2 + (Y + s) ** 2).astype(np.float32)
    return a


def test_policy_known_answers():
    f = np.float32
    vis = np.ones((16, 24), np.uint32)
    zero = np.zeros((16, 24, 4), np.float32)
    # no variance: 1 everywhere; Y = 0.5, s = 0.5 exactly: var = 0.25, d = 1, v = 0.0625 per pixel, b = 0.0625, x = b S
    flat = _sums_of(np.dstack([np.full((16, 24), 0.5), np.zeros((16, 24))]))
    assert (A.policy(flat, zero, vis, 2, 8, 1e-4, 8) == 1).all()
    noisy = _sums_of(np.dstack([np.full((16, 24), 0.5), np.full((16, 24), 0.5)]))
    x, covered = A.blocks_from_sums(noisy, zero, vis, 2, 8)
    assert (x == f(0.5)).all() and (covered == 64).all()
    # exactly at target, 2 target and 4 target: the lower side; just above: the upper
    up = float(np.nextafter(f(0.5), f(1.0)))
    for target, want in ((0.5, 1), (0.25, 2), (0.125, 4), (0.1, 8), (0.3, 2), (0.2, 4)):
        assert (A.policy(noisy, zero, vis, 2, 8, target, 8) == want).all(), target
    for scale, want in ((1.0, 2), (2.0, 4), (4.0, 8)):
        assert (A.counts(np.full((2, 3), f(up * scale), f), np.full((2, 3), 64), 0.5, 8) == want).all()
    assert (A.policy(noisy, zero, vis, 2, 8, 0.1, 4) == 4).all() and (A.policy(noisy, zero, vis, 2, 8, 0.1, 2) == 2).all()      # min(count, N)
    # S scales x: the same sums from one-sample frames are an eighth of the per-sample variance
    assert (A.policy(noisy, zero, vis, 2, 1, 0.0625, 8) == 1).all() and (A.policy(noisy, zero, vis, 2, 8, 0.0625, 8) == 8).all()
    # a NaN falls through to N, whatever N; an infinite sum is one
    bad = noisy.copy(); bad[3, 5, 3] = np.nan
    inf = noisy.copy(); inf[9, 20] = np.inf
    for N in (8, 4, 2):
        got = A.policy(bad, zero, vis, 2, 8, 10.0, N)
        assert got[0, 0] == N and (np.delete(got.ravel(), 0) == 1).all()
        got = A.policy(inf, zero, vis, 2, 8, 10.0, N)
        assert got[1, 2] == N and (np.delete(got.ravel(), 1 * 3 + 2) == 1).all()
    # no covered pixel: 1, whatever the sums hold; uncovered lanes add +0.0 and do not count
    none = vis.copy(); none[8:, 8:16] = 0
    got = A.policy(bad * f(np.nan), zero, none, 2, 8, 1e-4, 8)
    assert got[1, 1] == 1 and got[0, 0] == 8
    half = vis.copy(); half[:8, :8:2] = 0
    x, covered = A.blocks_from_sums(noisy, zero, half, 2, 8)
    assert covered[0, 0] == 32 and x[0, 0] == f(0.5)
    # a frame that is no multiple of 8: lanes beyond it add +0.0
    x, covered = A.blocks_from_sums(noisy[:13, :21], zero[:13, :21], vis[:13, :21], 2, 8)
    assert covered.tolist() == [[64, 64, 40], [40, 40, 25]] and (x == f(0.5)).all()


def test_the_pairwise_order_matters():
    """64 values whose sequential float32 sum differs from the pairwise one: 1 followed by 63 times 2^-24 -- every sequential addition
    rounds back to 1 (a tie to even), pairwise the small ones add up exactly among themselves first."""
    f = np.float32
    v = np.full(64, f(2.0 ** -24), f); v[0] = f(1.0)
    seq = f(0.0)
    for t in v:
        seq = f(seq + t)
    pair = A.pairwise_sum(v)
    assert seq == f(1.0) and pair == f(1.0 + 31 * 2.0 ** -23) and pair != seq
    # ... and the policy's block sum is the pairwise one: lane 8 (y & 7) + (x & 7)
    img = v.reshape(8, 8)
    np.testing.assert_array_equal(A.pairwise_sum(A.block_lanes(img, f(0.0))), [[pair]])
    assert A.block_lanes(np.arange(64).reshape(8, 8), 0).ravel().tolist() == list(range(64))


# ---- 4. what it buys -----------------------------------------------------------------------------------------------------------------
FRAMES, N, SAMPLE_SET, METALLIC = 16, 8, 65536, (0.25, 0.5)


def _display_luma(o, frames, trace):
    """The tone-curved luma Y / (Y + 0.5) of the mean over `frames` of the frame value (RayTracingOut0 + RayTracingOut1 where a diffuse path
    wrote it), float64 [H, W], and the rays traced; trace(o) renders the frame whose index has been set."""
    vis = o.buffer(O.BUF_VISIBILITY)
    dm = AR.diffuse_mask(vis, METALLIC)
    total, rays = np.zeros((H, W, 3), np.float64), 0
    for F in frames:
        HS.set_frame_index(o, int(F))
        rays += trace(o)
        total += AR.unpack_r11g11b10f(o.buffer(O.BUF_RT_REFL)).astype(np.float64)
        with np.errstate(invalid="ignore"):
            total += np.where(dm[..., None], AR.unpack_r11g11b10f(o.buffer(O.BUF_RT_DIFF)).astype(np.float64), 0.0)
    mean = total / len(frames)
    Y = 0.25 * mean[..., 0] + 0.5 * mean[..., 1] + 0.25 * mean[..., 2]
    return Y / (Y + 0.5), rays


def measure(aim=3.0):
    """Bunny 96x54, metallic 0.25 / 0.5, still camera, sample set 65536, N = 8.  Frames 0..15 uniform, accumulated (accum_ref); the map from
    their variance; frames 16..31 under the map, and uniform at 1, 2, 4 and 8 samples.  The error: MSE over covered pixels of the display
    luma of the 16-frame mean against that of 256 frames of 8 samples at the frame indices 1024..1279 (sample indices 8192..10239: none of
    the runs').  The target is the one, of a geometric grid, whose map's mean count over covered pixels is nearest 3 -- between uniform 2
    and uniform 4 in rays; it is chosen from the counts alone, before any mapped frame is traced."""
    o = _ref().Oracle(W, H, samples=N, sample_set=SAMPLE_SET, entry="sampleset")
    try:
        _scene(o, METALLIC)
        vis = o.buffer(O.BUF_VISIBILITY)
        covered = vis != 0
        assert covered.sum() > 500
        acc = AR.Accumulator(H, W)
        for F in range(FRAMES):
            HS.set_frame_index(o, F)
            o.ray_trace()
            acc.add(o.buffer(O.BUF_RT_REFL), o.buffer(O.BUF_RT_DIFF), vis, METALLIC)
        x, cov = A.blocks_from_sums(acc.refl, acc.diff, vis, FRAMES, N)
        grid = [1e-6 * 2.0 ** (k / 4.0) for k in range(80)]
        mean_count = lambda t: float((A.counts(x, cov, t, N).astype(np.float64) * cov).sum() / cov.sum())
        target = min(grid, key=lambda t: abs(mean_count(t) - aim))
        blocks = A.policy(acc.refl, acc.diff, vis, FRAMES, N, target, N)
        later = range(FRAMES, 2 * FRAMES)
        ref, _ = _display_luma(o, range(1024, 1280), lambda oo: oo.ray_trace())
        out = {"target": target, "histogram": [int((blocks == c).sum()) for c in A.COUNTS], "mean_count": mean_count(target)}
        images, rays = {}, {}
        images["mapped"], rays["mapped"] = _display_luma(o, later, lambda oo: A.mapped_frame(oo, blocks))
        for n in A.COUNTS:
            o.set_samples_per_pixel(n)
            images["uniform_%d" % n], rays["uniform_%d" % n] = _display_luma(o, later, lambda oo: oo.ray_trace())
        # one set of pixels for every run: covered, and finite in the reference and in all of them (a sample may be 0 x inf at a grazing pixel)
        at = covered & np.isfinite(ref)
        for img in images.values():
            at &= np.isfinite(img)
        out["pixels"], out["covered"] = int(at.sum()), int(covered.sum())
        for k, img in images.items():
            out[k] = {"rays": rays[k], "mse": float(((img - ref)[at] ** 2).mean())}
        o.set_samples_per_pixel(N)
        lo, hi, m = out["uniform_2"], out["uniform_4"], out["mapped"]
        s = (math.log(m["rays"]) - math.log(lo["rays"])) / (math.log(hi["rays"]) - math.log(lo["rays"]))
        out["uniform_interpolated_mse"] = math.exp(math.log(lo["mse"]) + s * (math.log(hi["mse"]) - math.log(lo["mse"])))
        out["ratio"] = m["mse"] / out["uniform_interpolated_mse"]
        return out
    finally:
        o.close()


def test_the_measurement_that_left_the_policy_out(built):
    """The check the policy had to pass: the mapped run's rays between uniform 2's and uniform 4's, and its error BELOW the uniform error
    interpolated log-log to its ray count.  It does not pass: 121 645 rays against 88 527 and 177 014, MSE 2.62e-3 against an interpolated
    2.47e-3 -- a ratio of 1.06; 1.06, 1.05 and 1.00 at targets that give mean counts of 2.4, 3.4 and 3.7.  So the library ships the map and
    no policy (DESIGN.md "Adaptive sampling" says why counts in proportion to the variance lose).  What this test holds is the record: the
    rays bracket as required, the uniform errors fall with the count, and every figure equals tests/golden/adaptive_convergence.json
    within 5 % (same integers, same fp32 arithmetic; another libm may move a table entry by an ulp and a few packed words by a code).  A
    policy that is to be shipped has to bring this ratio below 1 first."""
    got = measure()
    recorded = json.load(open(GOLDEN))
    for k in ("mapped", "uniform_1", "uniform_2", "uniform_4", "uniform_8"):
        print("%s: %d rays, mse %.6g (recorded %d, %.6g)" % (k, got[k]["rays"], got[k]["mse"], recorded[k]["rays"], recorded[k]["mse"]))
    print("target %g, histogram %s, interpolated uniform mse %.6g, ratio %.4f (recorded %.4f)" % (
        got["target"], got["histogram"], got["uniform_interpolated_mse"], got["ratio"], recorded["ratio"]))
    assert got["uniform_2"]["rays"] < got["mapped"]["rays"] < got["uniform_4"]["rays"]
    assert got["pixels"] >= 0.99 * got["covered"]
    assert got["uniform_1"]["mse"] > got["uniform_2"]["mse"] > got["uniform_4"]["mse"] > got["uniform_8"]["mse"] > 0.0
    for k in ("mapped", "uniform_1", "uniform_2", "uniform_4", "uniform_8"):
        assert abs(got[k]["mse"] - recorded[k]["mse"]) <= 0.05 * recorded[k]["mse"], (k, got[k], recorded[k])
        assert abs(got[k]["rays"] - recorded[k]["rays"]) <= 0.01 * recorded[k]["rays"], (k, got[k], recorded[k])
    assert abs(got["ratio"] - recorded["ratio"]) <= 0.1 * recorded["ratio"]


if __name__ == "__main__":
    import __graft_entry__
    __graft_entry__.build()
    values = measure()
    values["what"] = ("bunny 96x54, metallic 0.25 / 0.5, sample set 65536, N = 8: the map from the variance of 16 accumulated uniform frames; MSE over "
                      "covered pixels of the display luma Y / (Y + 0.5) of the mean of the next 16 frames -- under the map, and uniform at 1, 2, 4, 8 "
                      "samples -- against 256 frames of 8 samples at other indices; ratio = mapped / uniform interpolated log-log to the mapped rays")
    with open(GOLDEN, "w") as fh:
        json.dump(values, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(values, indent=1, sort_keys=True))
