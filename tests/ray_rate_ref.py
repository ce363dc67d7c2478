"""numpy restatement of quarter-rate tracing (rtggx_set_ray_rate(ctx, 4); include/rtggx.h, DESIGN.md "Quarter-rate tracing"): which
pixel of each 2x2 quad a frame traces, and the reconstruction of the others (raytrace.hip reconstructKernel) from the G-buffer words and
the traced pixels' RayTracingOut0/1 words.  fp32 in the kernel's order of operations; the depth weight's exp and the divisions in fp64,
rounded once, as in the kernel -- bit for bit but for the rare fp64 exp whose rounding to fp32 the two libraries decide differently."""
import numpy as np

ORDER = ((0, 0), (1, 1), (1, 0), (0, 1))      # traced (x & 1, y & 1) by FrameIndex & 3

F32 = np.float32
_INV_NORMAL_SQ = F32(1.0) / F32(1046529.0)      # 1 / 1023^2
_INV_D24 = F32(1.0) / F32(16777215.0)
_INV_255 = F32(1.0) / F32(255.0)


def traced_mask(width, height, frame_index):
    ox, oy = ORDER[frame_index & 3]
    y, x = np.mgrid[0:height, 0:width]
    return ((x & 1) == ox) & ((y & 1) == oy)


def _ufloat_to_f32(v, mbits):
    v = v.astype(np.uint32)
    e, m = v >> mbits, v & ((1 << mbits) - 1)
    denorm = m.astype(np.float32) * np.array((127 - 14 - mbits) << 23, dtype=np.uint32).view(np.float32)
    bits = np.where(e == 31, 0x7F800000 | (m << (23 - mbits)), ((e + 112) << 23) | (m << (23 - mbits))).astype(np.uint32)
    return np.where(e == 0, denorm, bits.view(np.float32)).astype(np.float32)


def unpack_r11g11b10f(words):
    w = np.asarray(words, dtype=np.uint32)
    return np.stack([_ufloat_to_f32(w & 0x7FF, 6), _ufloat_to_f32((w >> 11) & 0x7FF, 6), _ufloat_to_f32(w >> 22, 5)], axis=-1)


def _f32_to_ufloat(f, mbits):
    """rtggx_device.h f32ToUfloat: 5-bit exponent, round to nearest even, negatives -> 0, finite overflow -> the largest finite value."""
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.int64)
    exp_max = 31 << mbits
    shift = 23 - mbits
    max_bits = 0x47000000 | (((1 << mbits) - 1) << shift)
    a = u - 0x38000000
    a = a + ((1 << (shift - 1)) - 1) + ((a >> shift) & 1)
    normal = a >> shift
    e = u >> 23
    mant = (u & 0x7FFFFF) | 0x800000
    sh = np.clip(shift + (113 - e), 1, 40)
    q = mant >> sh
    rem = mant & ((np.int64(1) << sh) - 1)
    half = np.int64(1) << (sh - 1)
    den = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    den = np.where((e < 127 - 15 - mbits - 1) | (shift + (113 - e) > 31), 0, den)
    out = np.select([(u & 0x7FFFFFFF) > 0x7F800000, (u & 0x80000000) != 0, u == 0x7F800000, u > max_bits, u < 0x38800000],
                    [exp_max | 1, 0, exp_max, exp_max - 1, den], normal)
    return out.astype(np.uint32)


def pack_r11g11b10f(rgb):
    rgb = np.asarray(rgb, dtype=np.float32)
    return _f32_to_ufloat(rgb[..., 0], 6) | (_f32_to_ufloat(rgb[..., 1], 6) << 11) | (_f32_to_ufloat(rgb[..., 2], 5) << 22)


def _texels(normal, depth, rough_metal):
    n = normal.astype(np.int64)
    nx = (2 * (n & 1023) - 1023).astype(np.float32)
    ny = (2 * ((n >> 10) & 1023) - 1023).astype(np.float32)
    nz = (2 * ((n >> 20) & 1023) - 1023).astype(np.float32)
    d = depth.astype(np.float32) * _INV_D24
    r = (rough_metal & 0xFF).astype(np.float32) * _INV_255
    return nx, ny, nz, d, r


def _shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx], `fill` outside."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    b[yd, xd] = a[ys, xs]
    return b


def reconstruct(vis, depth, normal, rough_metal, refl, diff, frame_index, diffuse_instances=(0, 1)):
    """Expected RayTracingOut0 / RayTracingOut1 after the reconstruction: the untraced covered pixels replaced, everything else as given
    (carry-over of RayTracingOut1 where metallic >= 1 is not modelled here).  vis: the visibility words (0 = background, else
    ((instance << 24) | primitive) + 1); depth: D24; normal: R10G10B10A2 words; rough_metal: R8G8 words; refl / diff: R11G11B10 words
    of the traced pixels (others are ignored); diffuse_instances: the instances whose metallic is below 1."""
    H, W = vis.shape
    vis = vis.astype(np.uint32)
    covered = vis != 0
    inst = np.where(covered, (vis.astype(np.int64) - 1) >> 24, -1)
    traced = traced_mask(W, H, frame_index)
    cand = traced & covered
    nx, ny, nz, d, r = _texels(normal, depth, rough_metal)
    Lr, Ld = unpack_r11g11b10f(refl), unpack_r11g11b10f(diff)
    zero3 = np.zeros((H, W, 3), np.float32)
    sumR, sumD, meanR, meanD = zero3.copy(), zero3.copy(), zero3.copy(), zero3.copy()
    wR, wD = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    n = np.zeros((H, W), np.int64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = _shift(cand, dx, dy, False) & (_shift(inst, dx, dy, -1) == inst) & covered
                I = (nx * _shift(nx, dx, dy) + ny * _shift(ny, dx, dy)) + nz * _shift(nz, dx, dy)
                x = np.maximum(I * _INV_NORMAL_SQ, F32(0.0))
                for _ in range(5):
                    x = x * x
                wnd = x * np.exp((-np.abs(d - _shift(d, dx, dy)) * d * F32(4.0)).astype(np.float64)).astype(np.float32)
                ts = np.clip(np.abs(_shift(r, dx, dy) - r) * F32(2.0), F32(0.0), F32(1.0))
                w = wnd * (F32(1.0) - ts * ts * (F32(3.0) - F32(2.0) * ts))
                qr, qd = _shift(Lr, dx, dy), _shift(Ld, dx, dy)
                ok3 = ok[..., None]
                sumR = np.where(ok3, sumR + qr * w[..., None], sumR); wR = np.where(ok, wR + w, wR); meanR = np.where(ok3, meanR + qr, meanR)
                sumD = np.where(ok3, sumD + qd * wnd[..., None], sumD); wD = np.where(ok, wD + wnd, wD); meanD = np.where(ok3, meanD + qd, meanD)
                n += ok
        far = n == 0
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                ok = far & _shift(cand, dx, dy, False) & (_shift(inst, dx, dy, -1) == inst) & covered
                ok3 = ok[..., None]
                meanR = np.where(ok3, meanR + _shift(Lr, dx, dy), meanR); meanD = np.where(ok3, meanD + _shift(Ld, dx, dy), meanD)
                n += ok
        cnt = np.maximum(n, 1).astype(np.float64)[..., None]
        div = lambda s, w: (s.astype(np.float64) / w).astype(np.float32)
        outR = np.where((wR > 0)[..., None], div(sumR, np.where(wR > 0, wR, F32(1.0)).astype(np.float64)[..., None]), np.where((n > 0)[..., None], div(meanR, cnt), meanR))
        outD = np.where((wD > 0)[..., None], div(sumD, np.where(wD > 0, wD, F32(1.0)).astype(np.float64)[..., None]), np.where((n > 0)[..., None], div(meanD, cnt), meanD))
    target = covered & ~traced
    dif = target & np.isin(inst, list(diffuse_instances))
    refl_out = np.where(target, pack_r11g11b10f(outR), refl.astype(np.uint32))
    diff_out = np.where(dif, pack_r11g11b10f(outD), diff.astype(np.uint32))
    return refl_out.astype(np.uint32), diff_out.astype(np.uint32), target, dif
