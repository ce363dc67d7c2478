"""Synthetic inputs of the denoise chain -- TEST INFRASTRUCTURE ONLY.  Deterministic (fixed seeds), small, packed as the render targets
hold them.  Used by tests/test_denoise_ref_host.py (model against oracle) and tests/test_gpu_denoise_synthetic.py (product against model).

What the kernels are entitled to assume (launchDenoise, denoise.hip; rtggx_upload, debug.hip) -- `check` asserts it on every case:
  1. the seven inputs and both TemporalSSOut images are whole W x H images of the context's size;
  2. the diffuse passes are launched iff a material of the frame constants has metallic < 1 (denoise.hip launchDenoise: metallic is a
     per-instance constant, Material.hlsli:20-30): a texel may carry a metal code below 255 only if a material says so.  (The converse is
     not assumed: materials with metallic < 1 over an all-255 image only cost two launches.)  Without diffuse passes FilteredOut is
     FilteredOut1 (one image; rtggx_readback returns it for both);
  3. depth words are 24-bit (D24_UNORM: at most 0xFFFFFF);
  4. velocity texels are finite half floats (the visibility pass writes a difference of two projected positions), of any size and sign:
     the history fetch clamps its addresses;
  5. the history image's alpha is the history weight a temporal pass wrote: finite, in [0, 1].  Its colour may be anything, and so may the
     other TemporalSSOut image (the H passes' scratch: pixels without a surface keep what it held);
  6. the raw ray-traced images are R11G11B10_FLOAT words of any value, inf and NaN codes included;
  7. normals (zero-length and non-unit codes included), their 2-bit alpha, roughness and depth are read per texel by every kernel and may
     vary freely;
  8. on a strip (rtggx_set_strip) a reprojection reads at most the history apron's rows beyond the strip.
After an upload the tiles' words read "unknown" (debug.hip rtggx_upload), so the tile-word and still-sky early-outs are NOT under test with
these inputs; they have their own bit-identity tests (tests/test_gpu_static_sky.py).
One more restriction is the suite's own, not the kernels': normals are either within 6 % of unit length, or the zero-length code, or long
enough to overflow the 512th power.  In between, a weight falls into fp32's denormal range, which D3D flushes, the oracle's host does not and
the product's v_exp_f32 may: no statement of the shader fixes the result there.
"""
import numpy as np

SIZES = [(1, 1), (9, 7), (17, 33), (64, 4), (65, 5), (97, 61), (333, 217)]
DEFAULT_BASE = (1.0, 1.0, 1.0, 1.0)


class Case:
    def __init__(self, name, W, H, seed, metallic=(1.0, 1.0), flat=False):
        self.name, self.W, self.H, self.flat = name, W, H, flat
        self.materials = [(0.16, float(metallic[0])), (0.5, float(metallic[1]))]      # (roughness, metallic) of the two instances
        self.expect = {}       # facts that make the case non-vacuous: asserted by the host test against the model
        self.strips = []       # row ranges the GPU test also renders as strips
        self.regions = {}      # named masks whose results must be finite (expect: finite_<name>_min)
        rng = self.rng = np.random.default_rng(seed)
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        self.xs, self.ys = xs, ys
        # normals: a smooth field plus noise, lengths within 2 % of 1
        n = np.stack([0.6 * np.sin(xs / 9.0 + 0.3) + 0.05 * rng.standard_normal((H, W)), 0.6 * np.cos(ys / 7.0) + 0.05 * rng.standard_normal((H, W)),
                      np.ones((H, W))], -1)
        n = n / np.linalg.norm(n, axis=-1, keepdims=True) * rng.uniform(0.98, 1.02, (H, W, 1))
        self.ncode = np.clip(np.rint((n * 0.5 + 0.5) * 1023.0), 0, 1023).astype(np.uint32)
        self.acode = rng.integers(1, 4, (H, W)).astype(np.uint32)                      # 1, 2, 3: a surface
        self.rough = rng.integers(0, 256, (H, W)).astype(np.uint16)
        self.metal = np.full((H, W), 255, np.uint16)
        if min(metallic) < 1.0:
            self.metal = np.where(rng.random((H, W)) < 0.5, 255, rng.integers(0, 255, (H, W))).astype(np.uint16)
        d = 0.55 + 0.3 * (xs / max(W - 1, 1)) - 0.2 * (ys / max(H - 1, 1)) + 0.002 * rng.standard_normal((H, W))
        self.depth = np.clip(np.rint(d * 16777215.0), 0, 0xFFFFFF).astype(np.uint32)
        self.refl, self.diff = self.lognormal_image(3.0, 12.0), self.lognormal_image(2.0, 10.0)
        self.vel = (rng.uniform(-0.4, 0.4, (H, W, 2)) / np.array([W, H])).astype(np.float16)      # sub-pixel
        self.hist = self.f16_image(); self.hist[..., 3] = (rng.integers(0, 16, (H, W)) / 15.0).astype(np.float16)
        self.scratch = self.f16_image()

    # ---- pieces
    def lognormal_image(self, spread, centre):
        """R11G11B10 words: exponents follow a smooth texture plus noise (2^-11 .. 2^3: four decades), mantissas random.  The diffuse image is
        the dimmer one: its passes have no Gaussian, they blur 33 taps wide, and a frame whose FilteredOut1 were mostly that blur would be flat
        to the temporal pass (ill-conditioned variance: see denoise_ref.py)."""
        rng, H, W = self.rng, self.H, self.W
        e = np.clip(np.rint(centre + spread * (np.sin(self.xs / 7.0) + np.cos(self.ys / 5.0))[..., None] + rng.standard_normal((H, W, 3))), 4, 18).astype(np.uint32)
        m6, m5 = rng.integers(0, 64, (H, W, 2)).astype(np.uint32), rng.integers(0, 32, (H, W)).astype(np.uint32)
        return ((e[..., 0] << 6) | m6[..., 0]) | (((e[..., 1] << 6) | m6[..., 1]) << 11) | (((e[..., 2] << 5) | m5) << 22)

    def f16_image(self):
        rng, H, W = self.rng, self.H, self.W
        c = np.exp2(1.5 * (np.sin(self.xs / 7.0) + np.cos(self.ys / 5.0))[..., None] + rng.uniform(-1.5, 1.5, (H, W, 4)))
        return c.astype(np.float16)

    def hole(self, mask):
        self.acode = np.where(mask, 0, self.acode).astype(np.uint32)

    def set_normal(self, mask, v):
        """The normal v (not normalised: its length is the caller's) at `mask`."""
        code = np.clip(np.rint((np.asarray(v, np.float64) * 0.5 + 0.5) * 1023.0), 0, 1023).astype(np.uint32)
        self.ncode = np.where(mask[..., None], code, self.ncode)

    # ---- packed
    def buffers(self):
        vel = np.ascontiguousarray(self.vel).view(np.uint16).astype(np.uint32)
        return {"normal": (self.ncode[..., 0] | (self.ncode[..., 1] << 10) | (self.ncode[..., 2] << 20) | (self.acode << 30)).astype(np.uint32),
                "rough_metal": (self.rough | (self.metal << 8)).astype(np.uint16), "depth": self.depth.astype(np.uint32),
                "velocity": (vel[..., 0] | (vel[..., 1] << 16)).astype(np.uint32), "rt_refl": self.refl.astype(np.uint32),
                "rt_diff": self.diff.astype(np.uint32),
                "history": np.ascontiguousarray(self.hist).view(np.uint64).reshape(self.H, self.W),
                "scratch": np.ascontiguousarray(self.scratch).view(np.uint64).reshape(self.H, self.W)}


def check(case):
    """The list of the module docstring, asserted."""
    b = case.buffers()
    for k, v in b.items():
        assert v.shape == (case.H, case.W), (case.name, k)
    any_diffuse = min(m for _, m in case.materials) < 1.0
    assert any_diffuse or (case.metal == 255).all(), "%s: metal codes below 255 need a material with metallic < 1" % case.name
    assert (b["depth"] <= 0xFFFFFF).all()
    assert np.isfinite(case.vel.astype(np.float64)).all(), "%s: velocities are finite" % case.name
    a = case.hist[..., 3].astype(np.float64)
    assert np.isfinite(a).all() and (a >= 0.0).all() and (a <= 1.0).all(), "%s: history alpha in [0, 1]" % case.name
    n = (2.0 * case.ncode.astype(np.float64) - 1023.0) / 1023.0
    l2 = (n * n).sum(-1)
    assert (((l2 > 0.88) & (l2 < 1.13)) | (l2 < 1e-5) | (l2 > 1.2)).all(), "%s: a normal in the denormal band of the 512th power" % case.name
    for lo, hi in case.strips:
        assert 0 <= lo < hi <= case.H
        assert (np.abs(case.vel[..., 1].astype(np.float64)) * case.H <= 2.0).all(), "%s: strips keep reprojections within the history apron" % case.name
    return b


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def _sizes():
    out = []
    for k, (W, H) in enumerate(SIZES[:6]):      # (333 x 217: the roughness cases below)
        c = Case("size_%dx%d" % (W, H), W, H, 100 + k, metallic=(1.0, 0.5))
        if W * H > 1:
            c.hole(c.rng.random((H, W)) < 0.15)
        c.expect = {"surface_min": 1}
        out.append(c)
    return out


def _rough_ramp_wide():
    c = Case("rough_ramp_wide_333x217", 333, 217, 1)
    c.rough = ((c.xs * 256.0) // 333.0).astype(np.uint16)       # every code; 0.1 rough W reaches 33, the clamp 0.05 H = 10.85 binds
    c.hole((c.xs > 300) & (c.ys % 50 < 3))
    c.expect = {"radii_min": 11, "radius_max": 10}
    c.strips = [(0, 64), (80, 144), (150, 217)]
    c.vel[..., 1] = np.clip(c.vel[..., 1], -1.0 / 217, 1.0 / 217)
    return c


def _rough_ramp_tall():
    c = Case("rough_ramp_tall_40x260", 40, 260, 2)
    c.rough = ((c.ys * 256.0) // 260.0).astype(np.uint16)       # every code; 0.1 rough W <= 4 (exactly 4 in fp32 at code 255) < 0.05 H = 13: the clamp never binds
    c.expect = {"radii_min": 5, "radius_max": 4}
    return c


def _rough_seam():
    c = Case("rough_seam_97x61", 97, 61, 3, metallic=(0.25, 1.0))
    c.rough = np.where(c.xs + 0.7 * c.ys < 60, 40, 200).astype(np.uint16)      # the seam crosses the 16- and 64-texel block borders obliquely
    c.hole(c.rng.random((61, 97)) < 0.03)
    c.expect = {"radii_min": 2}
    return c


def _rough_const():
    c = Case("rough_const_333x217", 333, 217, 4)
    c.rough[:] = 77
    W, H = 333, 217
    m = (c.xs == 20) & (c.ys == 30)                                            # one pixel
    m |= (c.xs >= 32) & (c.xs < 48) & (c.ys >= 64) & (c.ys < 80)               # a whole 16 x 16 tile
    m |= (c.xs >= 40) & (c.xs < 90) & (c.ys >= 120) & (c.ys < 170) & ((c.xs + c.ys) % 2 == 0)      # a checkerboard
    c.hole(m)                                                                  # x >= 140: tiles with a surface everywhere (and the frame's edge: the apron has none)
    c.expect = {"radii_min": 1, "holes_min": 16 * 16 + 1}
    c.strips = [(0, 33), (100, 117), (201, 217)]
    c.vel[..., 1] = np.clip(c.vel[..., 1], -1.0 / 217, 1.0 / 217)
    return c


def _normals():
    c = Case("normals_97x61", 97, 61, 5, metallic=(0.5, 0.5))
    W, H = 97, 61
    rng = c.rng
    c.metal = rng.integers(0, 255, (H, W)).astype(np.uint16)                   # every pixel takes part in the diffuse passes
    stripes = (c.xs >= 30) & (c.xs < 44) & (c.ys >= 20) & (c.ys < 40)
    c.set_normal(stripes & (c.xs % 2 == 0), (0.0, 0.0, 1.0)); c.set_normal(stripes & (c.xs % 2 == 1), (0.0, 0.0, -1.0))      # antiparallel neighbours: dot < 0
    c.ncode = np.where(((c.xs >= 50) & (c.xs < 56) & (c.ys >= 25) & (c.ys < 31))[..., None], 512, c.ncode).astype(np.uint32)      # the zero-length code, a block of it
    c.set_normal((c.xs >= 60) & (c.xs < 70) & (c.ys >= 20) & (c.ys < 30), (0.0, 0.6, 0.848))      # |n|^2 = 1.079 > 1: dot products above 1
    # centre normals with nx + ny + nz < -1.19 within 16 texels of each border: a tap outside the frame is 0 x inf
    far = np.array([-0.58, -0.58, -0.575])                                     # sum -1.735, |n|^2 = 1.0034
    for m in ((c.xs == 5) & (c.ys == 30), (c.xs == W - 7) & (c.ys == 33), (c.xs == 48) & (c.ys == 4), (c.xs == 52) & (c.ys == H - 9), (c.xs == 2) & (c.ys == 2)):
        c.set_normal(m, far)
    c.expect = {"nan_flt_rfl_min": 20, "wsum_diff_zero_min": 4}
    return c


def _alpha_holes():
    c = Case("alpha_codes_holes_97x61", 97, 61, 6)
    c.acode = ((c.xs // 3 + c.ys // 2) % 4).astype(np.uint32)                  # codes 0, 1, 2, 3 in small blocks: holes everywhere
    c.acode = np.where((c.xs >= 64) & (c.xs < 80) & (c.ys >= 16) & (c.ys < 32), 0, c.acode).astype(np.uint32)
    c.scratch[10:14, 20:30, :3] = np.float16(np.nan); c.scratch[40, 50:60, 0] = np.float16(np.inf)      # what the scratch held where there is no surface (and where there is: overwritten)
    c.expect = {"holes_min": 97 * 61 // 5, "plain_min": 100}
    return c


def _depth():
    c = Case("depth_97x61", 97, 61, 7, metallic=(1.0, 0.0))
    c.metal = np.where((c.xs // 5) % 2 == 0, 255, 100).astype(np.uint16)
    d = c.depth.copy()
    d[:, :16] = 0; d[:16, 80:] = 0xFFFFFF
    d[20:50, 16:48] = (np.linspace(0, 0xFFFFFF, 32)[None, :]).astype(np.uint32)              # a ramp over the whole range
    d[32:, 48:64] = 0x400000; d[32:, 64:80] = 0x400400                                        # steps at tile seams, small and
    d[48:, :] = np.where(c.xs[48:, :] < 64, d[48:, :], 0xC00000)                              # large
    c.depth = d
    c.expect = {"depth_zero": True}
    return c


def _metal_checker():
    c = Case("metal_checker_65x5", 65, 5, 8, metallic=(1.0, 0.3))
    c.metal = np.where((c.xs + c.ys) % 2 == 0, 255, 60).astype(np.uint16)
    c.ncode = np.where(((c.xs >= 20) & (c.xs < 30))[..., None], 512, c.ncode).astype(np.uint32)      # zero-length normals: every diffuse weight there is 0
    c.expect = {"wsum_diff_zero_min": 10}
    return c


def _metal_none():
    c = Case("metal_all_below_17x33", 17, 33, 9, metallic=(0.0, 0.9))
    c.metal = c.rng.integers(0, 255, (33, 17)).astype(np.uint16)
    return c


def _raw_extremes():
    """Zeros, denormal codes, the largest finite code, inf and NaN codes in the raw images.  A non-finite texel turns NaN in the H pass's tone
    map (inf / (1 + inf)) and takes its 33 x 33 footprint with it (one texel more in the temporal pass, another in the tone map), on a
    texel without a surface as well (its flag 0 times NaN).  So they are confined to the frame's top left corner, and the blocks whose VALUES
    are under test lie more than 34 texels away from it: Case.regions names them, and the host test asserts that the results there are finite."""
    c = Case("raw_extremes_97x61", 97, 61, 10, metallic=(0.5, 1.0))
    rng = c.rng
    box = lambda x0, x1, y0, y1: (c.xs >= x0) & (c.xs < x1) & (c.ys >= y0) & (c.ys < y1)
    corner, zeros, denormal, bright = box(0, 12, 0, 10), box(50, 80, 0, 10), box(50, 80, 34, 44), box(34, 80, 48, 61)
    c.hole(c.xs >= 80)
    c.hole(((c.xs == 2) & (c.ys == 3)) | ((c.xs == 7) & (c.ys == 8)))
    # the largest code: ten texels on a smooth, rough patch, so that the filters average each with its neighbours -- alone, its tone-mapped
    # luminance rounds to 1 in the half-float scratch and the inverse tone map 1 / (1 - luminance) is a pole, where no two evaluations agree
    c.set_normal(bright, (0.0, 0.0, 1.0)); c.rough = np.where(bright, 255, c.rough).astype(np.uint16); c.depth = np.where(bright, 0x900000, c.depth).astype(np.uint32)
    peaks = ((c.xs - 38) % 8 == 0) & (c.xs >= 38) & (c.xs <= 70) & ((c.ys == 51) | (c.ys == 57))
    assert int(peaks.sum()) == 10
    for img in ("refl", "diff"):
        w = getattr(c, img).copy()
        w[zeros] = 0
        den = rng.integers(1, 32, (3, 61, 97)).astype(np.uint32)
        w = np.where(denormal, den[0] | (den[1] << 11) | (den[2] << 22), w)     # denormal codes: exponent fields 0
        w = np.where(peaks, (0x7BF) | (0x7BF << 11) | (0x3DF << 22), w)         # the largest finite code in each channel (65024, 65024, 64512)
        pts = rng.choice(12 * 10, 30, replace=False); pts = (pts // 12) * 97 + pts % 12      # in the corner
        w.reshape(-1)[pts[:10]] = (0x7C0) | (0x123 << 11) | (0x155 << 22)       # +inf in red
        w.reshape(-1)[pts[10:20]] = (0x300) | (0x7C1 << 11) | (0x155 << 22)     # NaN in green
        w.reshape(-1)[pts[20:30]] = (0x300) | (0x300 << 11) | (0x3E0 << 22)     # +inf in blue
        w[3, 2] = 0x7C0; w[8, 7] = 0x7C1 << 11                                   # ... and on the two texels without a surface
        setattr(c, img, w.astype(np.uint32))
    near_peaks = np.zeros_like(peaks)
    for y, x in np.argwhere(peaks):
        near_peaks |= box(x - 2, x + 3, y - 2, y + 3)
    c.regions = {"zeros": zeros, "denormal": denormal, "largest": near_peaks}
    c.expect = {"nonfinite_flt_min": 20, "finite_zeros_min": 300, "finite_denormal_min": 300, "finite_largest_min": 250}
    return c


def _velocity():
    c = Case("velocity_97x61", 97, 61, 11, metallic=(1.0, 0.6))
    W, H = 97, 61
    rng = c.rng
    v = np.zeros((H, W, 2))
    r = lambda x0, x1, y0, y1: (c.xs >= x0) & (c.xs < x1) & (c.ys >= y0) & (c.ys < y1)
    v[r(16, 32, 0, 20)] = rng.uniform(-0.5, 0.5, (int(r(16, 32, 0, 20).sum()), 2)) / [W, H]                  # sub-pixel (0..16: zero)
    v[r(32, 48, 0, 20)] = rng.uniform(-6.0, 6.0, (int(r(32, 48, 0, 20).sum()), 2)) / [W, H]                  # several pixels
    v[r(0, 8, 20, 61)] = [1.5, 0.0]; v[r(89, 97, 20, 61)] = [-1.5, 0.0]                                       # beyond the frame: right / left
    v[r(20, 80, 53, 61)] = [0.0, -2.0]; v[r(20, 80, 20, 26)] = [0.0, 2.0]                                     # bottom / top
    v[r(48, 64, 0, 20)] = [3.0 / W, 0.0]; v[r(48, 64, 0, 20) & (c.xs % 2 == 0)] = [0.0, 3.0 / W]              # equal speeds side by side: ties of VelocityMax
    v[r(30, 70, 30, 50)] = [0.25 / W, 0.0]; v[r(30, 70, 30, 50) & (c.xs % 5 == 0) & (c.ys % 4 == 0)] = [4.0 / W, -3.0 / H]      # a fast neighbour
    c.vel = v.astype(np.float16)
    c.expect = {"over_each_border_min": 8, "vmax_moved_min": 50, "vmax_ties_min": 50, "gamma_at_clamp_min": 100}
    return c


def _history():
    c = Case("history_97x61", 97, 61, 12, metallic=(0.7, 1.0))
    c.hole((c.xs >= 70) & (c.ys < 30))
    # non-finite history texels make the bilinear fetch discontinuous where a weight is exactly 0 (0 x inf): reprojections here stay a tenth
    # of a texel away from the texel centres, where every faithful evaluation of the address agrees on the four taps
    c.vel = (c.rng.choice([-1.0, 1.0], (61, 97, 2)) * c.rng.uniform(0.1, 0.4, (61, 97, 2)) / np.array([97, 61])).astype(np.float16)
    c.vel[50:, :] = 0      # ... and a still band well away from them: with a history weight above 3/4 gamma reaches its upper clamp (8 / historyBlur > 32)
    c.hist[..., 3] = ((c.xs // 6) % 16 / 15.0).astype(np.float16)              # every k / 15
    from oracle import oracle as O
    raw = O.unpack_r11g11b10f(c.refl).astype(np.float64)
    # colour near the current image below row 40 (0.9 x the raw reflection), far from it above (another texture, 8 x brighter)
    c.hist[..., :3] = np.where((c.ys >= 40)[..., None], raw * 0.9, c.hist[..., :3].astype(np.float64) * 8.0).astype(np.float16)
    c.hist[5, 10:20, :3] = np.float16(np.nan); c.hist[8, 30:40, 1] = np.float16(np.inf); c.hist[45, 10:20, :3] = np.float16(np.nan)
    c.hist[20:30, 40:60, :3] = 0
    c.expect = {"plain_min": 100, "long_min": 2000, "gamma_at_clamp_min": 100}
    return c


def _flat():
    c = Case("temporal_flat_97x61", 97, 61, 13, flat=True)
    c.set_normal(np.ones((61, 97), bool), (0.0, 0.0, 1.0))
    c.acode[:] = 3; c.rough[:] = 128; c.depth[:] = 0x800000
    c.refl[:] = (0x3D0) | (0x3E8 << 11) | (0x1E4 << 22)                        # one colour, about (1.25, 1.6, 1.1)
    c.vel[:] = 0
    c.hist[..., :3] = np.float16(4.0); c.hist[..., 3] = np.float16(14.0 / 15.0)
    c.expect = {"ill_share_min": 0.5}
    return c


_CASES = None


def all_cases():
    """The cases, built once (nothing that uses them changes them)."""
    global _CASES
    if _CASES is None:
        _CASES = _sizes() + [_rough_ramp_wide(), _rough_ramp_tall(), _rough_seam(), _rough_const(), _normals(), _alpha_holes(), _depth(),
                             _metal_checker(), _metal_none(), _raw_extremes(), _velocity(), _history(), _flat()]
    return _CASES


def by_name(name):
    return {c.name: c for c in all_cases()}[name]


NAMES = [c.name for c in all_cases()]
