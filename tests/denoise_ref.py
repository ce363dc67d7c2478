"""A float64 model of the denoise chain, per pixel -- TEST INFRASTRUCTURE ONLY.

Written from the shaders' statement (oracle/orc_denoise.h cites the same lines), in vectorised numpy,
sharing no arithmetic with the oracle (only its numpy unpackers of the texel formats) and none with the product:

  CSSpatial_H_Refl.hlsl:15-50, CSSpatial_V_Refl.hlsl:16-59    reflection H / V   (SpatialFilter.hlsli:57-67)
  CSSpatial_H_Diff.hlsl:15-48, CSSpatial_V_Diff.hlsl:17-59    diffuse H / V      (SpatialFilter.hlsli:69-83)
  FilterCommon.hlsli:14-71                                    TM / ITM, the weights, the blur radius
  CSTemporalSS.hlsl:78-161, 166-236, 254-336                  temporal pass (_DENOISE_, _ALPHA_AS_ID_, _VARIANCE_AABB_, YCoCg)
  PSToneMap.hlsl:13-41                                        tone map + sharpening
  Denoiser.cpp:66-75, 361-478                                 pass order, ping-pong: scratch = TSS[parity], history = TSS[!parity]

What is float64 and what is not:
  * continuous arithmetic is float64.  A value is rounded only where the reference stores a typed texel: the H passes' RGBA16F scratch,
    FilteredOut, FilteredOut1, TemporalSSOut (float64 -> binary16, nearest even, once) and the RGBA8 back buffer;
  * decisions that are discontinuous are taken as the shader takes them, in fp32: the blur radius (int)clamp(0.1 rough W, 0, 0.05 H)
    (FilterCommon.hlsli:49-52) with rough = code / 255 in fp32; norm.w <= 0; metal >= 1; the sq > speedSq selection of VelocityMax
    (CSTemporalSS.hlsl:133-161); |alpha - filtered.w| < 1/255; filtered.w > 0; the floor and the address clamp of the bilinear history
    fetch; the isnan fallback at :331.  (The alpha values are multiples of 1/16 and the velocities half floats, so most of these are exact
    in either precision; the blur radius and the bilinear floor are the ones that need fp32.)
  * every factor of a tap's weight is rounded to fp32 before the product, and so is the product: fp32's RANGE is part of the result.  A
    tap outside the frame reads zeros, i.e. the normal (-1, -1, -1); for a centre normal with nx + ny + nz < -1.19 its 512th power exceeds
    fp32, the hit flag 0 times +inf is NaN (SpatialFilter.hlsli:60) and the pixel, then its column, turns NaN.  A power that is below
    fp32's range is 0, and a pixel all of whose weights are 0 is 0 / 0.  The pattern of non-finite pixels is part of the result.
D3D rules: an out-of-range texel load returns zeros; SampleLevel(LINEAR_CLAMP) is a bilinear fetch with clamped addresses; min / max /
clamp / saturate return the other operand for a NaN (np.fmin / np.fmax).

Temporal pass, conditioning.  The clamp window is mu +- gamma sigma with sigma^2 = m2 / 9 - mu^2 over the 3 x 3 neighbourhood, evaluated in
fp32 by subtraction.  Roundings on the way, in units of the unit roundoff u = eps32 / 2 and relative to m2 / 9 >= mu^2:
    mu   = (sum of 9) / 9          8 additions + 1 division = 9 u,   squared: 18 u, + 1 for the product  = 19 u
    m2/9 = (sum of 9 squares) / 9  1 square + 8 additions + 1 division                                   = 10 u
so |fl(var) - var| <= 29 u (m2 / 9) =: K eps32 (m2 / 9) with K = 15 (rounded up).  `cond` = eps32 (m2 / 9) / |var| is what one rounding is
worth relative to the variance; a pixel with cond > COND_MAX in any channel is ILL-CONDITIONED: its sigma is rounding noise, and the only
statement that can be made about a faithful fp32 result is that it lies in the interval obtained by moving sigma by
sqrt(K eps32 m2 / 9) (sqrt(|v +- d|) is within sqrt(d) of sqrt(v)) through the clamp window, the blend and the inverse tone map.  The
result is not monotone in sigma (the window clamps the history, sets the contrast and the distance to the clamp), so the interval is
the envelope over SIGMA_SAMPLES values of sigma between the two ends, per channel.
"""
import numpy as np

from oracle import oracle as O      # unpackers of the texel formats only

RADIUS = 16                          # SpatialFilter.hlsli:8
EPS32 = float(np.finfo(np.float32).eps)      # 2^-23
K_ROUNDINGS = 15                     # see the module docstring
COND_MAX = 1e-2                      # THE threshold between the ulp check and the interval check (temporal result only)
SIGMA_SAMPLES = 9

_ERR = dict(over="ignore", under="ignore", invalid="ignore", divide="ignore")


def f32(a):
    """Round to fp32 (overflow to inf, underflow to 0 / denormal), back in float64."""
    with np.errstate(**_ERR):
        return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def to_f16_words(rgba):
    """(H, W, 4) float64 -> RGBA16F words (uint64), each channel rounded once to nearest even."""
    with np.errstate(**_ERR):
        h = np.ascontiguousarray(np.asarray(rgba, np.float64).astype(np.float16))
    return h.view(np.uint64).reshape(h.shape[:2])


def from_f16_words(words):
    return O.unpack_rgba16f(words).astype(np.float64)


def ulp16(v):
    """The spacing of binary16 at |v| (2^-24 below 2^-14; that of 65504 at and above it)."""
    a = np.clip(np.abs(np.nan_to_num(np.asarray(v, np.float64), nan=1.0, posinf=65504.0, neginf=65504.0)), 2.0 ** -14, 65504.0)
    return np.exp2(np.floor(np.log2(a)) - 10.0)


def shifted(a, dx, dy, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` outside the frame."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    x0, x1, y0, y1 = max(0, -dx), min(W, W - dx), max(0, -dy), min(H, H - dy)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def unpack_gbuffer(normal, rough_metal, depth):
    n = np.asarray(normal, np.uint32)
    codes = np.stack([n & 1023, (n >> 10) & 1023, (n >> 20) & 1023], -1).astype(np.float64)
    rm = np.asarray(rough_metal, np.uint16).astype(np.uint32)
    g = {"n": (2.0 * codes - 1023.0) / 1023.0,                # code / 1023 * 2 - 1
         "surf": (n >> 30) > 0,                               # norm.w > 0
         "rough_code": (rm & 0xFF).astype(np.int64), "rough": (rm & 0xFF).astype(np.float64) / 255.0,
         "metal1": (rm >> 8) == 255,                          # metal >= 1
         "depth": np.asarray(depth, np.uint32).astype(np.float64) / 16777215.0}
    return g


def blur_radius(rough_code, W, H):
    """GaussianRadiusFromRoughness, FilterCommon.hlsli:49-52, in fp32 as stated: (int)clamp(0.1 * rough * W, 0, H * 0.05)."""
    rough = rough_code.astype(np.float32) / np.float32(255.0)
    v = (np.float32(0.1) * rough) * np.float32(W)
    return np.minimum(np.maximum(v, np.float32(0.0)), np.float32(H) * np.float32(0.05)).astype(np.int64)


def _lum(c):
    return c[..., 0] * 0.25 + c[..., 1] * 0.5 + c[..., 2] * 0.25


def tm3(c):      # FilterCommon.hlsli:14-19
    with np.errstate(**_ERR):
        return c / (1.0 + _lum(c))[..., None]


def itm3(c):     # :24-27
    with np.errstate(**_ERR):
        return c / (1.0 - _lum(c))[..., None]


def _common_weights(g, dx, dy, sigma_pow):
    """Normal and depth factors of the tap at (dx, dy), each rounded to fp32 (FilterCommon.hlsli:34-42)."""
    with np.errstate(**_ERR):
        nt = shifted(g["n"], dx, dy, -1.0)
        dot = nt[..., 0] * g["n"][..., 0] + nt[..., 1] * g["n"][..., 1] + nt[..., 2] * g["n"][..., 2]
        wn = f32(np.power(np.maximum(dot, 0.0), sigma_pow))
        dt = shifted(g["depth"], dx, dy, 0.0)
        wd = f32(np.exp(-np.abs(g["depth"] - dt) * g["depth"] * 4.0))
    return wn, wd


def reflection_pass(g, src, vertical, W, H):
    """One reflection pass over the whole frame: src (H, W, 3) -> the weighted mean (H, W, 3) (V: inverse tone-mapped), valid at surface
    pixels.  Also the sum of the weights."""
    br = blur_radius(g["rough_code"], W, H)
    sigma = (br + 1.0) / 3.0                                   # FilterCommon.hlsli:59-71
    mu = np.zeros((H, W, 3)); wsum = np.zeros((H, W))
    with np.errstate(**_ERR):
        for i in range(-RADIUS, RADIUS + 1):
            dx, dy = (0, i) if vertical else (i, 0)
            wn, wd = _common_weights(g, dx, dy, 512.0)
            flag = shifted(g["surf"], dx, dy, False).astype(np.float64)
            wg = f32(np.exp(-0.5 * (abs(i) / sigma) ** 2))
            t = np.clip(np.abs(shifted(g["rough"], dx, dy, 0.0) - g["rough"]) / 0.5, 0.0, 1.0)
            wr = f32(1.0 - t * t * (3.0 - 2.0 * t))
            w = f32((((flag * wg) * wn) * wd) * wr)             # SpatialFilter.hlsli:57-67, in its order: 0 x inf = NaN
            mu += shifted(src, dx, dy, 0.0) * w[..., None]
            wsum += w
        mu = mu / wsum[..., None]
        if vertical:
            mu = itm3(mu)
    return mu, wsum


def diffuse_pass(g, src, vertical, W, H):
    part = g["surf"] & ~g["metal1"]
    mu = np.zeros((H, W, 3)); wsum = np.zeros((H, W))
    with np.errstate(**_ERR):
        for i in range(-RADIUS, RADIUS + 1):
            dx, dy = (0, i) if vertical else (i, 0)
            pt = shifted(part, dx, dy, False)                  # CSSpatial_H_Diff.hlsl:35: such taps are SKIPPED, whatever they hold
            wn, wd = _common_weights(g, dx, dy, 32.0)
            w = np.where(pt, f32(wn * wd), 0.0)
            mu += np.where(pt[..., None], shifted(src, dx, dy, 0.0) * w[..., None], 0.0)
            wsum += w
        mu = mu / wsum[..., None]
        if vertical:
            mu = itm3(mu)
    return mu, wsum


def spatial_chain(inp):
    """The four spatial passes.  inp: dict of packed words (normal, rough_metal, depth, rt_refl, rt_diff, scratch = TSS[parity] as it
    stands before the frame).  Returns FilteredOut / FilteredOut1 as float64 before the store ("flt_rfl", "flt_dff": (H, W, 4)) and as
    words, the sums of weights and the blur radii."""
    H, W = inp["normal"].shape
    g = unpack_gbuffer(inp["normal"], inp["rough_metal"], inp["depth"])
    surf, part = g["surf"], g["surf"] & ~g["metal1"]
    refl = O.unpack_r11g11b10f(inp["rt_refl"]).astype(np.float64)
    diff = O.unpack_r11g11b10f(inp["rt_diff"]).astype(np.float64)
    scratch = from_f16_words(inp["scratch"])                  # the H pass leaves pixels without a surface as they were (H :19)
    # reflection H -> scratch (alpha 0), V -> FilteredOut (alpha 1); no surface: the raw texel, alpha 0 (V :22-26)
    muH, _ = reflection_pass(g, tm3(refl), False, W, H)
    scratch = np.where(surf[..., None], np.concatenate([muH, np.zeros((H, W, 1))], -1), scratch)
    scratch = from_f16_words(to_f16_words(scratch))
    muV, wsum_r = reflection_pass(g, scratch[..., :3], True, W, H)
    flt_rfl = np.where(surf[..., None], np.concatenate([muV, np.ones((H, W, 1))], -1), np.concatenate([refl, np.zeros((H, W, 1))], -1))
    flt_rfl_words = to_f16_words(flt_rfl)
    # diffuse H -> scratch, V -> FilteredOut1 = FilteredOut + diffuse; not taking part: FilteredOut passes through (V :24-28)
    dH, _ = diffuse_pass(g, tm3(diff), False, W, H)
    scratch = np.where(part[..., None], np.concatenate([dH, np.zeros((H, W, 1))], -1), scratch)
    scratch = from_f16_words(to_f16_words(scratch))
    dV, wsum_d = diffuse_pass(g, scratch[..., :3], True, W, H)
    dest = from_f16_words(flt_rfl_words)
    with np.errstate(**_ERR):
        flt_dff = np.where(part[..., None], np.concatenate([dest[..., :3] + dV, dest[..., 3:]], -1), dest)
    return {"flt_rfl": flt_rfl, "flt_rfl_words": flt_rfl_words, "flt_dff": flt_dff, "flt_dff_words": to_f16_words(flt_dff),
            "wsum_refl": wsum_r, "wsum_diff": wsum_d, "surf": surf, "diffuse": part, "blur_radius": blur_radius(g["rough_code"], W, H)}


# ---- CSTemporalSS.hlsl ---------------------------------------------------------------------------------------------------------------
_OFFSETS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (1, 1), (-1, 1)]      # g_texOffsets :48-52


def _to_ycocg(c):      # :78-85 -- a matrix product: the zero coefficient takes part (0 x inf = NaN in Co for an infinite green)
    return np.stack([c[..., 0] + 2.0 * c[..., 1] + c[..., 2], 2.0 * c[..., 0] + 0.0 * c[..., 1] - 2.0 * c[..., 2],
                     -c[..., 0] + 2.0 * c[..., 1] - c[..., 2]], -1)


def _tss_tm(c):        # :106-114
    with np.errstate(**_ERR):
        y = _to_ycocg(c)
        return y / (4.0 + y[..., :1])


def _tss_itm(c):       # :119-128, :90-101
    with np.errstate(**_ERR):
        k = 4.0 / (1.0 - c[..., 0])
        y, co, cg = c[..., 0] * k * 0.25, c[..., 1] * k * 0.25, c[..., 2] * k * 0.25
        return np.stack([y + co - cg, y + cg, y - co - cg], -1)


def _sat(x):
    return np.fmin(np.fmax(x, 0.0), 1.0)


def _lerp(a, b, t):
    return a + t * (b - a)


def temporal_pass(flt_dff_words, velocity, history_words):
    """CSTemporalSS.hlsl:254-336 on FilteredOut1 words.  Returns the result before the store ("value": (H, W, 4), alpha = the history
    weight), "words", per pixel "cond" (the worst channel's), "ill" (cond > COND_MAX), the interval "lo" / "hi" (H, W, 3) and the masks
    "long" (filtered.w > 0: the history takes part; elsewhere blend = 1 at :325 and the product takes its short "plain" path), "over" (a
    bilinear tap was clamped at a border: l, r, t, b), "vmax_moved" (VelocityMax took a neighbour's velocity) and "vmax_ties" (an equally
    fast neighbour with another velocity was passed over), "gamma_at_clamp" (8 / historyBlur was cut to 32 at :280-281)."""
    H, W = flt_dff_words.shape
    cur = from_f16_words(flt_dff_words)
    vw = np.asarray(velocity, np.uint32)
    vel = np.stack([(vw & 0xFFFF).astype(np.uint16).view(np.float16), (vw >> 16).astype(np.uint16).view(np.float16)], -1).astype(np.float64)
    with np.errstate(**_ERR):
        # VelocityMax :133-161 -- the comparison in fp32 (squares of half floats are exact, their sum is rounded once)
        vmax = vel.copy()
        v32 = vel.astype(np.float32)
        speed = v32[..., 0] * v32[..., 0] + v32[..., 1] * v32[..., 1]
        sq_all = speed.copy()
        ties = np.zeros((H, W), bool)
        for dx, dy in _OFFSETS[4:]:
            sq = shifted(sq_all, dx, dy, np.float32(0.0)); nb = shifted(vel, dx, dy, 0.0)
            take = sq > speed
            ties |= (sq == speed) & (speed > 0) & (nb != vmax).any(-1)      # an equally fast, different neighbour: the strict > keeps the earlier one
            vmax = np.where(take[..., None], nb, vmax); speed = np.where(take, sq, speed)
        moved = (vmax != vel).any(-1)
        # history = SampleLevel(linear clamp, uv - velocity) :259-260; floor and clamp in fp32, weights continuous
        xs, ys = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        sx = ((xs + 0.5) / W - vmax[..., 0]) * W - 0.5; sy = ((ys + 0.5) / H - vmax[..., 1]) * H - 0.5
        Wf, Hf = np.float32(W), np.float32(H)
        sx32 = ((xs.astype(np.float32) + np.float32(0.5)) / Wf - vmax[..., 0].astype(np.float32)) * Wf - np.float32(0.5)
        sy32 = ((ys.astype(np.float32) + np.float32(0.5)) / Hf - vmax[..., 1].astype(np.float32)) * Hf - np.float32(0.5)
        x0, y0 = np.floor(sx32).astype(np.float64), np.floor(sy32).astype(np.float64)
        fx, fy = sx - x0, sy - y0

        def cl(v, hi):
            return np.where(v < 0.0, 0, np.where(v > hi, hi, np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0))).astype(np.int64)
        ix0, ix1, iy0, iy1 = cl(x0, W - 1), cl(x0 + 1.0, W - 1), cl(y0, H - 1), cl(y0 + 1.0, H - 1)
        over = np.stack([x0 < 0.0, x0 + 1.0 > W - 1, y0 < 0.0, y0 + 1.0 > H - 1], -1)
        hist = from_f16_words(history_words)
        w00, w10, w01, w11 = (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy
        history = ((hist[iy0, ix0] * w00[..., None] + hist[iy0, ix1] * w10[..., None]) + hist[iy1, ix0] * w01[..., None]) + hist[iy1, ix1] * w11[..., None]
        # :262-281
        cur_blur = np.abs(vmax[..., 0]) * (4.0 * W) + np.abs(vmax[..., 1]) * (4.0 * H)
        hist_blur = np.fmax(1.0 - history[..., 3], cur_blur)
        hist_w = history[..., 3] * 15.0 + 1.0
        cur_tm = _tss_tm(cur[..., :3]); alpha = cur[..., 3]
        gamma = np.where(alpha <= 0.0, 1.0, np.fmin(np.fmax(8.0 / hist_blur, 1.0), 32.0))
        # NeighborMinMax :166-236
        filtered = np.concatenate([cur_tm, alpha[..., None]], -1)
        mu = cur_tm.copy(); m2 = cur_tm * cur_tm
        for k, (dx, dy) in enumerate(_OFFSETS):
            nraw = shifted(cur, dx, dy, 0.0)
            nb = np.concatenate([_tss_tm(nraw[..., :3]), nraw[..., 3:]], -1)
            filtered = filtered + nb * (0.5 if k < 4 else 0.25)
            mu = mu + nb[..., :3]; m2 = m2 + nb[..., :3] * nb[..., :3]
        filtered = filtered / 4.0
        gamma = np.where(np.abs(alpha - filtered[..., 3]) < 1.0 / 255.0, gamma, 1.0)
        gamma_at_clamp = (gamma == 32.0) & (alpha > 0.0) & (8.0 / hist_blur > 32.0)
        mu = mu / 9.0; m2 = m2 / 9.0
        var = m2 - mu * mu
        sigma = np.sqrt(np.abs(var))
        cond = np.max(np.where(np.abs(var) > 0.0, EPS32 * m2 / np.abs(var), np.where(m2 > 0.0, np.inf, 0.0)), -1)
        cond = np.where(np.isfinite(cond), cond, np.where(np.isnan(cond), 0.0, np.inf))      # a NaN neighbourhood is not "ill-conditioned": its pattern is checked
        dsig = np.sqrt(K_ROUNDINGS * EPS32 * np.abs(m2))
        cur_blur_s = _sat(cur_blur); hist_blur_s = _sat(hist_blur)      # :290-291
        hist_tm = _tss_tm(history[..., :3])

        def tail(sig):
            gs = gamma[..., None] * sig
            nmin = np.fmin(mu - gs, filtered[..., :3]); nmax = np.fmax(mu + gs, filtered[..., :3])
            nmin3, nmax3 = mu[..., 0] - sig[..., 0], mu[..., 0] + sig[..., 0]
            h = np.fmin(np.fmax(hist_tm, nmin), nmax)           # :294-299
            contrast = nmax3 - nmin3
            add_alias = _sat(hist_blur_s * 0.5 + 0.25 + 1.0 / (1.0 + contrast * (32.0 * 4.0)))      # :303-308
            fl = _lerp(filtered[..., :3], cur_tm, add_alias[..., None])      # :311
            dist = np.fmin(np.abs(nmin3 - h[..., 0]), np.abs(nmax3 - h[..., 0]))      # :314-325
            amt = np.fmin(1.0 / hist_w + hist_blur_s / 8.0, 1.0)
            blend = np.fmin(0.25 / _lerp(8.0, dist + contrast, amt), 0.25)
            blend = np.where(filtered[..., 3] > 0.0, blend, 1.0)
            res = _tss_itm(_lerp(h, fl, blend[..., None]))      # :327-329
            bad = np.isnan(res).any(-1)
            return np.where(bad[..., None], _tss_itm(fl), res)  # :331
        value = tail(sigma)
        lo, hi = value.copy(), value.copy()
        for s in np.linspace(-1.0, 1.0, SIGMA_SAMPLES):
            r = tail(np.maximum(sigma + s * dsig, 0.0))
            lo, hi = np.fmin(lo, r), np.fmax(hi, r)
        hw = np.fmin(hist_w / 15.0, 1.0 - cur_blur_s)           # :335
    value = np.concatenate([value, hw[..., None]], -1)
    long_path = filtered[..., 3] > 0.0
    return {"value": value, "words": to_f16_words(value), "cond": cond, "ill": (cond > COND_MAX) & long_path, "lo": lo, "hi": hi,
            "long": long_path, "over": over, "vmax_moved": moved, "vmax_ties": ties, "gamma_at_clamp": gamma_at_clamp}


# ---- PSToneMap.hlsl:13-41 --------------------------------------------------------------------------------------------------------------
# fp32 error of the value that is rounded to a code, in codes.  Each of the five terms t = c / (c + 0.5) in [0, 1) costs an addition, a
# division (or a 1-ulp reciprocal and a product) -- at most 3 eps32 absolute.  lap = -4 t0 + t1 + t2 + t3 + t4: |lap| <= 4, the terms bring
# 4 * 3 + 4 * 3 = 24 eps32, four additions of partial sums below 4 another 4 * 2 = 8 eps32: 32.  out = t0 - 0.2 lap: 3 + 0.2 * 32 + 2 (two
# roundings of values below 2) < 12 eps32; times 255, plus the two roundings of out * 255 + 0.5 below 256 (256 eps32): < 3400 eps32.
TONEMAP_TIE_CODES = 3400 * EPS32      # 4.1e-4 of a code


def tone_map(tss_words):
    """Returns (x, words, near_tie): x = (H, W, 4) the value whose floor is the code (clamp(out) * 255 + 0.5; NaN -> 0), the RGBA8 words,
    and where x lies within TONEMAP_TIE_CODES of an integer (a faithful fp32 evaluation may land on either side there)."""
    c = from_f16_words(tss_words)
    with np.errstate(**_ERR):
        t = np.concatenate([c[..., :3] / (c[..., :3] + 0.5), c[..., 3:]], -1)
        lap = -4.0 * t[..., :3]
        for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            lap = lap + shifted(t, dx, dy, 0.0)[..., :3]
        out = np.concatenate([t[..., :3] - 0.2 * lap, t[..., 3:]], -1)
        x = np.where(out > 0.0, np.fmin(out, 1.0), 0.0) * 255.0 + 0.5      # !(x > 0) -> 0: NaN and negatives
    code = np.floor(x).astype(np.uint32)
    words = code[..., 0] | (code[..., 1] << 8) | (code[..., 2] << 16) | (code[..., 3] << 24)
    near = np.abs(x - np.round(x)) < TONEMAP_TIE_CODES
    return x, words.astype(np.uint32), near


def chain(inp):
    """The whole frame: spatial_chain, temporal_pass on its FilteredOut1 words, tone_map on those."""
    out = spatial_chain(inp)
    out["temporal"] = temporal_pass(out["flt_dff_words"], inp["velocity"], inp["history"])
    out["bb_x"], out["bb_words"], out["bb_near"] = tone_map(out["temporal"]["words"])
    return out


# ---- comparison helpers shared by the host and the GPU tests --------------------------------------------------------------------------
def classes(v):
    """0 finite, 1 infinite (either sign: a quotient by a denominator that is 0 to rounding has no stable sign), 2 NaN."""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), 2, np.where(np.isinf(v), 1, 0))


def ulp_error(got_words, model_value, pixel_scale=False):
    """Per pixel, the largest colour-channel distance of the stored texel from the model's float64 value, in binary16 ulps of the model's
    value (-1 where nothing is finite on both sides: the pattern is compared separately).  pixel_scale: in ulps of the pixel's LARGEST
    channel -- for the temporal result, whose channels are Y +- Co +- Cg (CSTemporalSS.hlsl:90-101): a channel that cancels to a small
    value carries the absolute error of the large ones, and the ulp of its own value is not the scale of anything that was computed."""
    got = from_f16_words(got_words)[..., :3]
    ref = np.asarray(model_value, np.float64)[..., :3]
    with np.errstate(**_ERR):
        scale = ulp16(np.nanmax(np.where(np.isfinite(ref), np.abs(ref), 0.0), -1, keepdims=True)) if pixel_scale else ulp16(ref)
        e = np.abs(got - ref) / scale
    e = np.where(np.isfinite(got) & np.isfinite(ref), e, np.nan)
    return np.nanmax(np.where(np.isnan(e).all(-1, keepdims=True), -1.0, np.nan_to_num(e, nan=-1.0)), -1)      # -1: nothing to compare


def quantiles(e):
    """max / 99.9 % / 99 % / median of the entries >= 0."""
    e = np.asarray(e, np.float64).ravel(); e = e[e >= 0.0]
    if e.size == 0:
        return {"n": 0, "max": 0.0, "q999": 0.0, "q99": 0.0, "median": 0.0}
    return {"n": int(e.size), "max": float(e.max()), "q999": float(np.quantile(e, 0.999)), "q99": float(np.quantile(e, 0.99)),
            "median": float(np.median(e))}
