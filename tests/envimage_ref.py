"""Environments from images, restated with numpy from the contract in include/rtggx.h (rtggx_set_env_image, rtggx_generate_env_mips) and
not from the kernels: the RGBE decode and the clamp, the two cross tables, the fp32 mip chain operation by operation in np.float32, and a
float64 model of the panorama resampling.  Faces, texel order and directions are those of tests/env_ref.py (D3D's).  Also the writers the
tests need for Radiance .hdr (flat and new-style run-length scanlines) and .pfm files.

Images are arrays [H, W, ...] with row 0 at the top.  A cube level is float32 [6, s, s, 3]; a chain is the list of its levels."""
import numpy as np

import env_ref as R

EQUIRECT, VCROSS, HCROSS = 0, 1, 2
RGBE8, RGB32F = 0, 1
HALF_MAX = np.float32(65504.0)

# cell (row, col) -> (face, turned by 180 degrees); faces +X -X +Y -Y +Z -Z = 0 .. 5
CROSS = {VCROSS: {(0, 1): (2, False), (1, 0): (1, False), (1, 1): (4, False), (1, 2): (0, False), (2, 1): (3, False), (3, 1): (5, True)},
         HCROSS: {(0, 1): (2, False), (1, 0): (1, False), (1, 1): (4, False), (1, 2): (0, False), (1, 3): (5, False), (2, 1): (3, False)}}
CELLS = {VCROSS: (4, 3), HCROSS: (3, 4)}      # rows, columns of cells


def decode(pixels, image):
    """uint8 [H, W, 4] RGBE or float32 [H, W, 3] -> float32 [H, W, 3]: m 2^(e - 136) (e == 0: 0), then x > 0 ? min(x, 65504) : 0."""
    if pixels == RGBE8:
        image = np.asarray(image, np.uint8)
        e = image[..., 3].astype(np.int32)
        v = np.ldexp(image[..., :3].astype(np.float64), (e - 136)[..., None])      # exact in float64, and in float32 from e = 0 up (denormals included)
        x = np.where((e == 0)[..., None], 0.0, v).astype(np.float32)
        assert (x.astype(np.float64) == np.where((e == 0)[..., None], 0.0, v)).all()
    else:
        x = np.asarray(image, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.minimum(x, HALF_MAX), np.float32(0.0)).astype(np.float32)


def cross_level0(layout, rgb):
    """Decoded image float32 [H, W, 3] -> level 0 [6, c, c, 3]: a copy of six cells."""
    rows, cols = CELLS[layout]
    c = rgb.shape[0] // rows
    assert rgb.shape[0] == rows * c and rgb.shape[1] == cols * c
    cube = np.zeros((6, c, c, 3), np.float32)
    for (r, col), (face, turned) in CROSS[layout].items():
        cell = rgb[r * c:(r + 1) * c, col * c:(col + 1) * c]
        cube[face] = cell[::-1, ::-1] if turned else cell
    return cube


def paint_cross(layout, c, f):
    """The inverse: a cross image float64 [rows c, cols c, 3] whose cells hold f(direction through the texel's centre) [n, 3]; the cells no
    face uses are 0."""
    rows, cols = CELLS[layout]
    img = np.zeros((rows * c, cols * c, 3))
    y, x = np.meshgrid(np.arange(c), np.arange(c), indexing="ij")
    for (r, col), (face, turned) in CROSS[layout].items():
        fx, fy = (c - 1 - x, c - 1 - y) if turned else (x, y)      # the face texel shown at position (x, y) of the cell
        d = R.face_dir(np.full(c * c, face), ((fx + 0.5) / c * 2 - 1).reshape(-1), ((fy + 0.5) / c * 2 - 1).reshape(-1))
        img[r * c:(r + 1) * c, col * c:(col + 1) * c] = f(d).reshape(c, c, 3)
    return img


def chain_sides(size):
    """floor(log2(size)) + 1 levels of side max(size >> m, 1)."""
    return [size >> m for m in range(int(size).bit_length())]


def _halve(t, axis):
    """One axis of the box filter in float32, every operation rounded on its own in the contract's order.  t: float32, the axis of side p."""
    t = np.moveaxis(t, axis, 0)
    p = t.shape[0]
    q = p >> 1
    f = np.float32
    if p % 2 == 0:
        out = (t[0::2] + t[1::2]) / f(2)
    else:
        i = np.arange(q).reshape((q,) + (1,) * (t.ndim - 1))
        t0, t1, t2 = t[0:2 * q:2], t[1:2 * q:2], t[2:2 * q + 1:2]
        out = (((q - i).astype(f) * t0 + f(q) * t1) + (i + 1).astype(f) * t2) / f(p)
    assert out.dtype == np.float32
    return np.moveaxis(out, 0, axis)


def next_level(level):
    """float32 [6, p, p, 3] -> [6, p >> 1, p >> 1, 3]: each face alone, the horizontal pass (along x) first, then the vertical one."""
    return _halve(_halve(np.asarray(level, np.float32), 2), 1)


def chain(level0):
    levels = [np.asarray(level0, np.float32)]
    while levels[-1].shape[1] > 1:
        levels.append(next_level(levels[-1]))
    return levels


def pack(levels):
    """A chain -> uint16 [texels, 4], the layout of RTGGX_BUF_ENV: mip-major, six faces per mip, RGBA16F with alpha 1."""
    out = []
    for l in levels:
        t = np.ones(l.shape[:3] + (4,), np.float16)
        with np.errstate(over="ignore"):
            t[..., :3] = l.astype(np.float16)
        out.append(t.view(np.uint16).reshape(-1, 4))
    return np.concatenate(out)


def unpack(buf, size):
    """RTGGX_BUF_ENV uint16 [texels, 4] of a full chain -> the list of levels as float64 [6, s, s, 3]."""
    levels, at = [], 0
    for s in chain_sides(size):
        n = 6 * s * s
        levels.append(buf[at:at + n, :3].copy().view(np.float16).astype(np.float64).reshape(6, s, s, 3)); at += n
    assert at == buf.shape[0]
    return levels


def default_cube_size(width):
    s = 1
    while 2 * s <= width // 4:
        s *= 2
    return s


def equirect_level0(rgb, size):
    """The float64 model: decoded panorama [H, W, 3] -> level 0 float64 [6, size, size, 3].  Per texel the normalised direction through its
    centre, lon = atan2(d.x, d.z), lat = asin(d.y), s = (lon / 2 pi + 0.5) W - 0.5, t = (0.5 - lat / pi) H - 0.5, one bilinear tap, columns
    wrapping and rows clamping."""
    H, W = rgb.shape[:2]
    src = np.asarray(rgb, np.float64)
    d, _, _, _ = R.texel_centre_dirs(size)
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    lon, lat = np.arctan2(d[:, 0], d[:, 2]), np.arcsin(np.clip(d[:, 1], -1.0, 1.0))
    s, t = (lon / (2.0 * np.pi) + 0.5) * W - 0.5, (0.5 - lat / np.pi) * H - 0.5
    s0, t0 = np.floor(s), np.floor(t)
    fx, fy = (s - s0)[:, None], (t - t0)[:, None]
    x0, x1 = s0.astype(np.int64) % W, (s0.astype(np.int64) + 1) % W
    y0, y1 = np.clip(t0.astype(np.int64), 0, H - 1), np.clip(t0.astype(np.int64) + 1, 0, H - 1)
    out = (1.0 - fy) * ((1.0 - fx) * src[y0, x0] + fx * src[y0, x1]) + fy * ((1.0 - fx) * src[y1, x0] + fx * src[y1, x1])
    return out.reshape(6, size, size, 3)


def half_rounding(v):
    """What rounding |v| to binary16 may move it by: half the spacing of the halves around it (2^-25 below the smallest normal half)."""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 11.0)


# ---- file writers ------------------------------------------------------------------------------------------------------------------------
def _rle_channel(row):
    """New-style runs of one channel of one scanline (bytes): runs of 3 .. 127 equal bytes as (128 + n, value), the rest as literals of at
    most 128."""
    out, i, n = bytearray(), 0, len(row)
    lit = bytearray()

    def flush():
        nonlocal lit
        while lit:
            out.append(min(len(lit), 128)); out.extend(lit[:128]); lit = lit[128:]
    while i < n:
        j = i
        while j < n and j - i < 127 and row[j] == row[i]:
            j += 1
        if j - i >= 3:
            flush(); out.append(128 + (j - i)); out.append(row[i]); i = j
        else:
            lit.append(row[i]); i += 1
    flush()
    return bytes(out)


def hdr_bytes(rgbe, rle=False, magic=b"#?RADIANCE", fmt=b"FORMAT=32-bit_rle_rgbe", resolution=None):
    """uint8 [H, W, 4] -> the bytes of a Radiance file with flat or new-style run-length scanlines."""
    rgbe = np.asarray(rgbe, np.uint8)
    H, W = rgbe.shape[:2]
    head = magic + b"\n# written by tests/envimage_ref.py\n" + (fmt + b"\n" if fmt else b"") + b"EXPOSURE=1.0\n\n"
    head += (resolution if resolution is not None else b"-Y %d +X %d" % (H, W)) + b"\n"
    body = bytearray()
    for y in range(H):
        if rle:
            assert 8 <= W <= 32767
            body += bytes([2, 2, W >> 8, W & 255])
            for ch in range(4):
                body += _rle_channel(rgbe[y, :, ch].tobytes())
        else:
            body += rgbe[y].tobytes()
    return head + bytes(body)


def pfm_bytes(rgb, scale=b"-1.0"):
    """float32 [H, W, 3], row 0 at the top -> the bytes of a little-endian colour PFM file (rows bottom to top)."""
    rgb = np.asarray(rgb, np.float32)
    H, W = rgb.shape[:2]
    return b"PF\n%d %d\n" % (W, H) + scale + b"\n" + rgb[::-1].astype("<f4").tobytes()


def random_rgbe(rng, H, W, e_lo=20, e_hi=150):
    """Random RGBE pixels with exponents in [e_lo, e_hi], a tenth of them black (e == 0, any mantissa), a tenth with zero mantissas; never a
    pixel 1 1 1 n (an old-style run) and never 2 2 at the start of a row (the mark of a run-length scanline)."""
    p = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    p[..., 3] = rng.integers(e_lo, e_hi + 1, (H, W), dtype=np.uint8)
    kind = rng.integers(0, 10, (H, W))
    p[kind == 0, 3] = 0
    p[kind == 1, :3] = 0
    p[(p[..., 0] == 1) & (p[..., 1] == 1) & (p[..., 2] == 1), 0] = 7
    p[(p[:, 0, 0] == 2) & (p[:, 0, 1] == 2), 0, 0] = 3
    return p
