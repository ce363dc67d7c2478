"""Float64 model of one frame's shading paths per pixel, numpy only: the primary surface ray generation derives from the visibility
word, the GGX half vector (NDF map, and the VNDF map of rtggx_set_sampler), the ray's weight, the closest hit, the hit's shading and the
miss; paths of 1 to 4 levels (rtggx_set_max_recursion_depth) and 1 to 8 samples per pixel (rtggx_set_samples_per_pixel), written from the
rule texts of include/rtggx.h (follow_paths, frame).  It is the second witness of raytrace.hip next to the CPU oracle (oracle/orc_raytrace.h), which follows the kernel function by
function; this file shares no code with either and derives each step by another route wherever one exists:

  primary surface  the pixel centre's eye ray (ProjToWorld, ProjBias) meets the plane of the world-space triangle the visibility word names;
                   barycentrics are solved in world space (no screen-space gradients); N = n inverse-transpose(World), the inverse transpose
                   computed here from World, never read from the constants; velocity from WorldViewProjsPrev by definition
  sample           the integer hash in Python integers (exact); phi = 2 pi s / 256
  weight           BRDF NoL / pdf written from the definitions
  closest hit      Moeller-Trumbore over every triangle of both instances in world space, no tree, no object space
  hit shading      cube map and the nine SH coefficients from tests/env_ref.py; irradiance as sum A_l L_lm Y_lm(N)

A rounding is taken only where a typed texel is stored.  Every decision fp32 and float64 may take differently is FLAGGED per pixel, not
guessed (FLAG_* below); flagged pixels are compared with the oracle bit for bit like all others, but not with this model.

The sun's and the local lights' terms of the primary surface are sun_pass and lights_pass, from include/rtggx.h -- with the sun's disk
(rtggx_set_sun_angle) and the lights' radii: the hashes are integer and the draws exact, so the sampled target is computed, not guessed.
The light pick (rtggx_set_light_sampling) is pick_pass, its visibility records (rtggx_set_light_pick_visibility) records_pass one frame
at a time, the light list (rtggx_set_light_list) list_pass and cull_counts.
The sun's and the lights' terms at the surfaces the paths hit (rtggx_set_sun_reflections, rtggx_set_light_reflections; one sample) are
hits_pass, with the same sampled targets and mode 1's hit rule.
Out of scope: hit terms at N > 1, sample sets above 256, ray rate 4, the traversal's visiting order.

Conventions: row vectors (p' = p M); the frame constants are the 768 bytes of RtggxFrameConstants (include/rtggx.h), 4x4 matrices stored
transposed, 3x4 blocks as three rows of the transpose."""
import numpy as np

import env_ref as E

RAY_TMIN, RAY_TMAX = 1e-5, 10000.0      # the product's interval (rt_queue.h), both ends exclusive
REL_T, EDGE, NOL_EPS, UV_EPS, UP_EPS = 1e-5, 1e-5, 1e-5, 1e-4, 1e-5
UP_SWITCH = 0.999
FLAG_T_TIE, FLAG_EDGE, FLAG_NOL, FLAG_CHECKER, FLAG_UP, FLAG_TMIN, FLAG_CANCEL, FLAG_GRAZING, FLAG_RANGE, FLAG_CONE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
FLAG_NAMES = {FLAG_RANGE: "range", FLAG_CONE: "cone", FLAG_T_TIE: "t_tie", FLAG_EDGE: "edge", FLAG_NOL: "nol", FLAG_CHECKER: "checker", FLAG_UP: "up", FLAG_TMIN: "tmin", FLAG_CANCEL: "cancel",
              FLAG_GRAZING: "grazing"}
FLAG_GRAZING_DEEP = 1024      # NoL < GRAZING_NOL of a reflection at level >= 1 (no absolute side rule there: the pixel is just not compared)
FLAG_NAMES[FLAG_GRAZING_DEEP] = "grazing_deep"
# The reflection's weight is proportional to NoL (the other factors stay bounded: Vis's NoL + sqrt(...) is at least alpha), so the pixel's
# RELATIVE error is the absolute error of NoL over NoL.  That absolute error is a few 1e-6 in fp32 -- the primary surface's barycentrics come
# from screen-space gradients, P and V inherit their error, the reflection doubles it -- so below NoL = 2^-8 a faithful fp32 value is
# off by more than 1e-3 of itself, which is two codes of R11G11B10F.  Such pixels are ill-conditioned in the distance this test uses (ulps of
# the pixel's own largest channel) and are flagged, like a decision; nothing else about them is special.
GRAZING_NOL = 2.0 ** -8
# The one ill-conditioned step of the path: each sampler takes the root of a difference of two numbers near 1 -- 1 - cos^2 theta (NDF map, and
# the diffuse ray's sphere point), 1 - t1^2 - t2^2 (VNDF map) -- and fp32 rounds that difference with an ABSOLUTE error of a few 2^-24 however
# small it is: the direction is then off by up to sqrt(2^-22), far beyond every other threshold here.  The model cannot know which way fp32
# rounds, so it evaluates the pixel three times -- the difference as it is, and with CANCEL_SLACK taken from and added to it -- and returns
# the hull of the three as the pixel's interval; where the three take different decisions (another triangle, a miss, another checker
# cell, another side of NoL = 0) the pixel is flagged FLAG_CANCEL.  4 x 2^-24: the roundings of cos^2 theta (a quotient of two rounded
# numbers near 1, three half-ulps of 1) and one for the difference.
CANCEL_SLACK = 4.0 * 2.0 ** -24
SLACK_RUNS = (0.0, -1.0, 1.0)      # the three runs of a path by the sign of the slack; a segment's "run" is its index here


# ---- frame constants ---------------------------------------------------------------------------------------------------------------
def read_constants(fc_bytes):
    f = np.frombuffer(bytes(fc_bytes), np.float32)
    assert f.size == 192
    d = f.astype(np.float64)
    m4 = lambda a: d[a:a + 16].reshape(4, 4).T.copy()

    def m43(a):
        m = np.eye(4)
        m[:, :3] = d[a:a + 12].reshape(3, 4).T
        return m
    return {"wvp": [m4(0), m4(16)], "wvp_prev": [m4(32), m4(48)], "world": [m43(64), m43(76)],
            "frame_index": int(f[111:112].view(np.uint32)[0]), "proj_to_world": m4(112), "eye": d[128:131].copy(), "proj_bias": d[132:134].copy(),
            "colour": [d[176:179].copy(), d[180:183].copy()], "rough": [d[184], d[188]], "metal": [d[185], d[189]]}


def inverse_transpose(world):
    return np.linalg.inv(world[:3, :3]).T


# ---- stores --------------------------------------------------------------------------------------------------------------------------
def unorm_code(x, maxv):
    x = np.asarray(x, np.float64)
    return np.where(x > 0.0, np.floor(np.minimum(x, 1.0) * maxv + 0.5), 0.0).astype(np.int64)


def ufloat_values(mbits):
    """Every finite value of the unsigned small float with `mbits` mantissa bits, by code."""
    c = np.arange(31 << mbits)
    e, m = c >> mbits, (c & ((1 << mbits) - 1)).astype(np.float64)
    return np.where(e == 0, m * 2.0 ** (-14 - mbits), (1.0 + m / (1 << mbits)) * 2.0 ** (e - 15.0))


def ufloat_code(x, mbits):
    """float64 -> code of the unsigned small float: negatives to 0, round to nearest even, saturating at the largest finite value; NaN to
    the format's NaN, +inf to its inf."""
    x = np.asarray(x, np.float64)
    tab = ufloat_values(mbits)
    v = np.clip(np.where(np.isnan(x), 0.0, x), 0.0, tab[-1])
    hi = np.clip(np.searchsorted(tab, v, side="left"), 1, tab.size - 1)
    lo = hi - 1
    dl, dh = v - tab[lo], tab[hi] - v
    c = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    c = np.where(np.isposinf(x), 31 << mbits, c)
    return np.where(np.isnan(x), (31 << mbits) | 1, c).astype(np.int64)


def r11g11b10_codes(rgb):
    rgb = np.asarray(rgb, np.float64)
    return np.stack([ufloat_code(rgb[..., 0], 6), ufloat_code(rgb[..., 1], 6), ufloat_code(rgb[..., 2], 5)], axis=-1)


def r11g11b10_split(words):
    w = np.asarray(words).astype(np.int64)
    return np.stack([w & 0x7FF, (w >> 11) & 0x7FF, w >> 22], axis=-1)


def f16_ordered(x):
    """float64 -> binary16 (round to nearest even) as an integer that orders like the value; both zeros map to 0."""
    with np.errstate(over="ignore"):
        h = np.asarray(x, np.float64).astype(np.float16)
    c = h.view(np.uint16).astype(np.int64)
    return np.where(c & 0x8000, -(c & 0x7FFF), c)


def f16_words_ordered(words16):
    c = np.asarray(words16).astype(np.int64)
    return np.where(c & 0x8000, -(c & 0x7FFF), c)


def ulp32(x):
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 23.0)


# ---- the sample ----------------------------------------------------------------------------------------------------------------------
def _hash(seed):
    seed = (seed * 747796405 + 1) & 0xFFFFFFFF
    seed = (((seed >> ((seed >> 28) + 4)) ^ seed) * 277803737) & 0xFFFFFFFF
    return ((seed >> 22) ^ seed) & 0xFFFFFFFF


def sample_params(W, H, frame_index):
    """-> (s [H W] int, xi_y [H W]): the slot of the 256-member set and the second coordinate."""
    s = np.zeros(W * H, np.int64); y = np.zeros(W * H)
    for i in range(W * H):
        k = _hash((_hash(i) + frame_index) & 0xFFFFFFFF) % 256
        s[i] = k; y[i] = (_hash(k) & 0xFFFF) / 65536.0
    return s, y


# ---- vectors ---------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(axis=-1)


def _unit(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / np.sqrt(_dot(a, a))[..., None]


def _sat(x):
    return np.clip(x, 0.0, 1.0)


def tangent_frame(N):
    """The stated rule: up = y unless |n.y| >= 0.999, then x; T = unit(up x N), B = N x T.  -> (T, B, near the switch)."""
    up = np.where((np.abs(N[:, 1]) < UP_SWITCH)[:, None], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0])
    T = _unit(np.cross(up, N))
    return T, np.cross(N, T), np.abs(np.abs(N[:, 1]) - UP_SWITCH) <= UP_EPS


def ndf_half_vector(N, alpha, phi, xi, slack=0.0):
    """GGX NDF map: cos^2 theta = (1 - xi) / (1 + (alpha^2 - 1) xi).  slack: added to 1 - cos^2 theta before its root (CANCEL_SLACK)."""
    c2 = (1.0 - xi) / (1.0 + (alpha * alpha - 1.0) * xi)
    st, ct = np.sqrt(np.maximum(1.0 - c2 + slack, 0.0)), np.sqrt(c2)
    T, B, near = tangent_frame(N)
    return T * (st * np.cos(phi))[:, None] + B * (st * np.sin(phi))[:, None] + N * ct[:, None], near


def vndf_half_vector(N, V, alpha, phi, u, slack=0.0):
    """Heitz 2018, "Sampling the GGX Distribution of Visible Normals", listing 1 (isotropic): U1 = u, the angle phi = 2 pi U2.
    slack: added to 1 - t1^2 - t2^2 before its root (CANCEL_SLACK)."""
    T, B, near = tangent_frame(N)
    al = alpha[:, None] if np.ndim(alpha) else alpha
    ve = np.stack([_dot(V, T), _dot(V, B), _dot(V, N)], axis=1)
    vh = _unit(ve * np.concatenate([np.broadcast_to(al, (len(N), 1))] * 2 + [np.ones((len(N), 1))], axis=1))
    lensq = vh[:, 0] ** 2 + vh[:, 1] ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        t1v = np.where((lensq > 0)[:, None], np.stack([-vh[:, 1], vh[:, 0], np.zeros(len(N))], axis=1) / np.sqrt(lensq)[:, None], [1.0, 0.0, 0.0])
    t2v = np.cross(vh, t1v)
    r = np.sqrt(u)
    t1, t2 = r * np.cos(phi), r * np.sin(phi)
    s = 0.5 * (1.0 + vh[:, 2])
    t2 = (1.0 - s) * np.sqrt(1.0 - t1 * t1) + s * t2
    nh = t1[:, None] * t1v + t2[:, None] * t2v + np.sqrt(np.maximum(0.0, 1.0 - t1 * t1 - t2 * t2 + slack))[:, None] * vh
    ne = _unit(np.stack([alpha * nh[:, 0], alpha * nh[:, 1], np.maximum(0.0, nh[:, 2])], axis=1))
    return T * ne[:, :1] + B * ne[:, 1:2] + N * ne[:, 2:3], near


# ---- BRDF terms, from the definitions -----------------------------------------------------------------------------------------------
def ggx_d(alpha, NoH):
    a2 = alpha * alpha
    return a2 / (np.pi * (NoH * NoH * (a2 - 1.0) + 1.0) ** 2)


def smith_lambda_term(alpha, c):
    """c + sqrt(c (c - c a^2) + a^2): one factor of the separable Smith visibility's denominator."""
    a2 = alpha * alpha
    return c + np.sqrt(c * (c - c * a2) + a2)


def vis_smith(alpha, NoV, NoL):
    return 1.0 / (smith_lambda_term(alpha, NoV) * smith_lambda_term(alpha, NoL))


def g1(alpha, c):
    return 2.0 * c / smith_lambda_term(alpha, c)


def f0_of(colour, metal):
    return 0.04 + (colour - 0.04) * np.asarray(metal)[..., None]


def fresnel(f0, VoH):
    return f0 + (_sat(50.0 * f0[..., 1:2]) - f0) * ((1.0 - VoH) ** 5)[..., None]


def env_brdf_approx(f0, rough, NoV):
    """The mobile approximation of the pre-integrated environment BRDF, from its stated coefficients."""
    r = rough[:, None] * np.array([-1.0, -0.0275, -0.572, 0.022]) + np.array([1.0, 0.0425, 1.04, -0.04])
    a004 = np.minimum(r[:, 0] ** 2, 2.0 ** (-9.28 * NoV)) * r[:, 0] + r[:, 1]
    A, Bt = -1.04 * a004 + r[:, 2], (1.04 * a004 + r[:, 3]) * _sat(50.0 * f0[:, 1])
    return f0 * A[:, None] + Bt[:, None]


def ndf_weight(f0, alpha, NoV, NoL, VoH, NoH):
    """BRDF NoL / pdf_L with BRDF = D F Vis and pdf_L = D NoH / (4 VoH)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return fresnel(f0, VoH) * (vis_smith(alpha, NoV, NoL) * NoL * 4.0 * VoH / NoH)[..., None]


def vndf_weight(f0, alpha, NoL, VoH):
    return fresnel(f0, VoH) * g1(alpha, NoL)[..., None]


SH_BAND_FACTORS = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)      # the clamped cosine's zonal coefficients A_l


def sh_irradiance(coeffs, N):
    """E(N) = sum A_l L_lm Y_lm(N), not below zero; Y in env_ref's frame (x, y, z) = (-N.x, -N.y, N.z)."""
    return np.maximum((E.sh_basis(N) * SH_BAND_FACTORS) @ coeffs, 0.0)


# ---- the scene the model traces ------------------------------------------------------------------------------------------------------
class Scene:
    """Two meshes ((verts [nv 6], idx) in object space), the cube (env_cases.Cube) and what is derived once: the SH coefficients."""

    def __init__(self, meshes, cube):
        self.meshes = [(np.asarray(v, np.float64), np.asarray(i).reshape(-1, 3).astype(np.int64)) for v, i in meshes]
        self.cube = cube
        self.sh = E.sh_project(cube.levels[0], cube.size)[0]

    def environment(self, d, level):
        return E.environment(self.cube.levels, self.cube.size, d, level)


def _world_triangles(scene, fc):
    """-> (tris [m 3 3] world space, inst [m], prim [m]) in the order of the ids: the first of several minima is the lower id."""
    tris, inst, prim = [], [], []
    for k, (v, i) in enumerate(scene.meshes):
        p = np.concatenate([v[:, :3], np.ones((len(v), 1))], axis=1) @ fc["world"][k]
        tris.append(p[i][:, :, :3]); inst.append(np.full(len(i), k)); prim.append(np.arange(len(i)))
    return np.concatenate(tris), np.concatenate(inst), np.concatenate(prim)


def closest_hit(tris, org, d, skip, tmin=RAY_TMIN, tmax=RAY_TMAX, widen=None):
    """Brute force over every triangle.  org, d [n 3]; skip [n]: index into tris of the origin's primitive.  widen [n]: a factor on EDGE per
    ray (follow_paths: the error a deeper ray's origin carries).  -> dict: valid, tri, t, b [n 3] (weights of the three vertices), flags."""
    n, m = len(org), len(tris)
    out = {"valid": np.zeros(n, bool), "tri": np.zeros(n, np.int64), "t": np.full(n, np.inf), "b": np.zeros((n, 3)), "flags": np.zeros(n, np.int64)}
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    same = (tris[:, None] == tris[None]).all(axis=(2, 3))          # coincident triangles: their t is equal exactly, on every side
    step = max(1, 400000 // max(m, 1))
    for a in range(0, n, step):
        o, dd, sk = org[a:a + step], d[a:a + step], skip[a:a + step]
        band = EDGE if widen is None else (EDGE * widen[a:a + step])[:, None]
        k = len(o)
        p = np.cross(dd[:, None, :], e2[None])
        det = _dot(e1[None], p)
        with np.errstate(invalid="ignore", divide="ignore"):
            inv = 1.0 / det
            s = o[:, None, :] - tris[None, :, 0]
            u = _dot(s, p) * inv
            q = np.cross(s, e1[None])
            v = _dot(dd[:, None, :], q) * inv
            t = _dot(e2[None], q) * inv
        w = 1.0 - u - v
        lo = np.minimum(np.minimum(u, v), w)
        usable = (det != 0.0) & (np.arange(m)[None] != sk[:, None]) & np.isfinite(t)
        tm = np.asarray(tmax, np.float64)[a:a + step][:, None] if np.ndim(tmax) else tmax
        inside = usable & (lo >= 0.0) & (t > tmin) & (t < tm)
        tt = np.where(inside, t, np.inf)
        best = np.argmin(tt, axis=1)
        r = np.arange(k)
        tb = tt[r, best]
        valid = np.isfinite(tb)
        flags = np.zeros(k, np.int64)
        # a second candidate as close as rounding: a tie, unless it is the same triangle once more (equal t on every side, the lower id wins)
        reach = np.where(valid, tb * (1.0 + REL_T), np.inf)
        other = inside & (tt <= reach[:, None]) & (np.arange(m)[None] != best[:, None]) & ~(same[best] & (tt == tb[:, None]))
        flags |= np.where(other.any(axis=1), FLAG_T_TIE, 0)
        # a barycentric within EDGE of zero, on either side, on anything that is or could become the closest hit
        edge = usable & (np.abs(lo) <= band) & (t > 0.5 * tmin) & (t < tm) & (t <= reach[:, None])
        flags |= np.where(edge.any(axis=1), FLAG_EDGE, 0)
        ends = usable & (lo >= -band) & (((t > 0.5 * tmin) & (t < 2.0 * tmin)) | (np.abs(t - tm) < 1e-3 * tm))
        flags |= np.where(ends.any(axis=1), FLAG_TMIN, 0)
        sl = slice(a, a + k)
        out["valid"][sl], out["tri"][sl], out["t"][sl], out["flags"][sl] = valid, best, tb, flags
        out["b"][sl] = np.stack([w[r, best], u[r, best], v[r, best]], axis=1)
    return out


def _checker_roughness(inst, uv, rough, widen=1.0):
    """Instance 0's checkerboard: a quarter of the roughness where the two integer parts of 5 uv differ in parity (negative: 0).
    -> (roughness, within UV_EPS of a step)."""
    g = 5.0 * uv
    cell = np.floor(np.maximum(g, 0.0)).astype(np.int64)
    odd = ((cell[:, 0] ^ cell[:, 1]) & 1) == 1
    near = (np.abs(g - np.round(g)) <= np.reshape(UV_EPS * widen, (-1, 1))).any(axis=1) & (np.round(g) >= 0.0).any(axis=1)
    return np.where((inst == 0) & odd, 0.25 * rough, rough), near & (inst == 0)


def _uv(n, p):
    """Tri-planar coordinates from the object-space normal and position, scales (1, 0.2, 1)."""
    a = np.abs(n)
    s = p * np.array([1.0, 0.2, 1.0])
    uv = a[:, :1] * s[:, [1, 2]] + a[:, 1:2] * s[:, [2, 0]] + a[:, 2:3] * s[:, [0, 1]]
    return 0.5 * uv + 0.5


def _attributes(scene, fc, inst, prim, b, widen=1.0):
    """Object-space attributes at barycentric weights b [n 3] of (inst, prim) -> dict: pos_obj, N (world), rough, metal, colour, flags."""
    n = len(inst)
    pos, nrm = np.zeros((n, 3)), np.zeros((n, 3))
    for k, (v, i) in enumerate(scene.meshes):
        at = inst == k
        if at.any():
            vv = v[i[prim[at]]]                       # [k 3 6]
            pos[at] = (b[at][:, :, None] * vv[:, :, :3]).sum(axis=1)
            nrm[at] = (b[at][:, :, None] * vv[:, :, 3:]).sum(axis=1)
    it = np.stack([inverse_transpose(fc["world"][0]), inverse_transpose(fc["world"][1])])
    N = _unit(np.einsum("ni,nij->nj", nrm, it[inst]))
    rough0 = np.array(fc["rough"])[inst]
    rough, near = _checker_roughness(inst, _uv(nrm, pos), rough0, widen)
    return {"pos_obj": pos, "N": N, "rough": rough, "metal": np.array(fc["metal"])[inst], "colour": np.stack(fc["colour"])[inst],
            "flags": np.where(near, FLAG_CHECKER, 0)}


def _scale(lo, hi, f):
    a, b = lo * f, hi * f
    return np.minimum(a, b), np.maximum(a, b)


# ---- a path of D levels (include/rtggx.h: rtggx_set_max_recursion_depth) ---------------------------------------------------------------
TERM_NONE, TERM_MISS, TERM_PRESET, TERM_NOL, TERM_MIRROR, TERM_DIFFUSE = 0, 1, 2, 3, 4, 5      # how a path ended (TERM_NONE: no level-0 ray)
TERM_NAMES = {TERM_MISS: "miss", TERM_PRESET: "preset", TERM_NOL: "nol", TERM_MIRROR: "last_mirror", TERM_DIFFUSE: "last_diffuse"}
EVENTS = ("refl_to_diff", "diff_to_refl", "one_minus_m")


def _last_level(scene, a, d, diffuse_group):
    """The depth-1 shading of a hit with the attributes a, reached along d: metallic > 0.5 the cube along the dominant direction of the
    lobe times EnvBRDFApprox (0 where that direction lies under the surface), otherwise SH irradiance / pi x colour, the colour x (1 - m)
    for a diffuse-group ray.  diffuse_group [n] bool.  -> (lo, hi [n 3], flags [n])."""
    n = len(d)
    N, V = a["N"], -d
    mirror = a["metal"] > 0.5
    l, u, fl = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, np.int64)
    if mirror.any():
        j = mirror
        r, al = a["rough"][j], a["rough"][j] ** 2
        Nj, Vj = N[j], V[j]
        R = 2.0 * _dot(Nj, Vj)[:, None] * Nj - Vj
        with np.errstate(invalid="ignore"):
            w = (1.0 - al) * (np.sqrt(1.0 - al) + al)
        dr = Nj + w[:, None] * (R - Nj)
        NoL = _dot(Nj, dr)
        with np.errstate(divide="ignore"):
            level = (len(scene.cube.levels) - 1.0) - (3.0 - 1.15 * np.log2(r))
        el, eh = scene.environment(dr, np.where(np.isnan(level), 0.0, level))
        f = env_brdf_approx(f0_of(a["colour"][j], a["metal"][j]), r, _sat(_dot(Nj, Vj)))
        el, eh = _scale(el, eh, f)
        dark = NoL <= 0.0
        el[dark] = eh[dark] = 0.0
        l[j], u[j] = el, eh
        fl[j] = np.where(np.abs(NoL) <= NOL_EPS, FLAG_NOL, 0)
    if (~mirror).any():
        j = ~mirror
        c = a["colour"][j] * np.where(diffuse_group[j], 1.0 - a["metal"][j], 1.0)[:, None]
        l[j] = u[j] = sh_irradiance(scene.sh, N[j]) / np.pi * c
    return l, u, fl


def sphere_direction(N, phi, xi, slack=0.0):
    """The diffuse ray: unit(N + the point of the unit sphere at height 1 - 2 xi and azimuth phi).  slack: added to 1 - cos^2 before its root."""
    ct = 1.0 - 2.0 * xi
    st = np.sqrt(np.maximum(1.0 - ct * ct + slack, 0.0))
    return _unit(N + np.stack([np.cos(phi) * st, np.sin(phi) * st, ct], axis=1))


def follow_paths(scene, fc, geo, org, d, skip, T, diffuse_group, preset, phi, xi, depth=1, vndf=False, slack=0.0, segments=None, ident=None):
    """n paths of `depth` levels from their level-0 rays (org, d; skip: the index of the origin's triangle), as rtggx_set_max_recursion_depth
    states them.  T [n 3]: the level-0 weight w0; T_{d+1} = T_d w_{d+1}, and the value is c T with c what the path ends with:
      a miss                               environment(dir, level 0)
      a hit of a reflection-group ray whose preset (colour x metallic of the surface it left) is <= 0 everywhere: the preset
      a hit of the last level              its depth-1 shading (_last_level)
      a hit with metallic > 0.5            computeReflection with the path's (phi, xi) at every level: H by the sampler at the hit's N and
                                           V = -dir, R = reflect(-V, H); NoL <= 0 ends with 0; else a reflection-group ray from
                                           P = o + t dir along R, skipping the hit's triangle, of weight BRDF NoL / pdf (ndf_weight, vndf_weight)
      any other hit                        computeDiffuse: colour' = colour (1 - m) for a diffuse-group ray, colour for a reflection-group
                                           one; a diffuse-group ray along unit(N + sphere(xi)) of weight colour' (no 0.96)
    slack: CANCEL_SLACK's sign for every sampler root of the path, all levels together.  segments: a list that receives one dict per level
    of the rays that touch a surface (for the sun's and the lights' terms at the hits); ident [n]: what it names the paths by.
    -> dict: lo, hi [n 3]; flags [n]; sig [n, 3 depth] (per level: triangle or -1, roughness, how the path ended there) for the cancel rule;
       kind, level [n]: how and where each path ended; rays [depth]; events {name: count}."""
    tris, tri_inst, tri_prim = geo
    n = len(org)
    lo, hi = np.zeros((n, 3)), np.zeros((n, 3))
    flags, kind, level = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    sig = np.full((n, depth, 3), -3.0)
    rays = np.zeros(depth, np.int64)
    events = dict.fromkeys(EVENTS, 0)
    at = np.arange(n)                      # the paths that have a ray at this level
    grp = np.broadcast_to(np.asarray(diffuse_group, bool), (n,)).copy()
    T, preset = np.array(T, np.float64), np.array(preset, np.float64)
    # The error a ray's origin carries: a level-0 ray leaves the primary surface (EDGE and UV_EPS are sized for that); a deeper ray leaves the hit
    # point P = o + t dir, whose error along the surface is the ray's own over the cosine of incidence on the triangle's plane.  Every edge
    # band and checkerboard band of a level is widened by the product of those factors over the hits before it (1 at level 0).
    amp = np.ones(n)
    geo_n = _unit(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]))

    def end(which, lev, k, c_lo, c_hi):
        lo[at[which]], hi[at[which]] = _scale(c_lo, c_hi, T[which])
        kind[at[which]], level[at[which]] = k, lev

    for lev in range(depth):
        rays[lev] = at.size
        if not at.size:
            break
        h = closest_hit(tris, org, d, skip, widen=None if lev == 0 else amp)
        flags[at] |= h["flags"]
        sig[at, lev, 0], sig[at, lev, 1] = np.where(h["valid"], h["tri"], -1), 0.0
        miss = ~h["valid"]
        if miss.any():
            end(miss, lev, TERM_MISS, *scene.environment(d[miss], 0.0))
        hit = h["valid"]
        dark = hit & ~grp & (preset <= 0.0).all(axis=1)
        if dark.any():
            end(dark, lev, TERM_PRESET, preset[dark], preset[dark])
        hit = hit & ~dark
        k = np.nonzero(hit)[0]
        keep = np.zeros(at.size, bool)
        if k.size:
            a = _attributes(scene, fc, tri_inst[h["tri"][k]], tri_prim[h["tri"][k]], h["b"][k], 1.0 if lev == 0 else amp[k])
            # m = 0.5 decides between the two shadings; the constant is the same fp32 number on every side, so the decision is too -- but a case
            # that sits on the threshold tests nothing, and none may (m = 1 is a legitimate material: it only zeroes a factor)
            assert not (a["metal"] == 0.5).any(), "a hit's metallic is exactly 0.5"
            flags[at[k]] |= a["flags"]
            sig[at[k], lev, 1] = a["rough"]
            Pk = org[k] + h["t"][k][:, None] * d[k]
            mirror = a["metal"] > 0.5
            events["one_minus_m"] += int((~mirror & grp[k] & (a["metal"] > 0.0)).sum())
            if segments is not None:
                segments.append({"level": lev, "path": (at if ident is None else ident[at])[k], "P": Pk, "N": a["N"], "V": -d[k], "rough": a["rough"], "metal": a["metal"],
                                 "colour": a["colour"], "T": T[k].copy(), "diffuse_group": grp[k].copy(), "tri_of": h["tri"][k], "flags": a["flags"],
                                 "amp": amp[k] / np.maximum(np.abs(_dot(geo_n[h["tri"][k]], d[k])), 2.0 ** -20)})
            if lev + 1 == depth:
                l, u, fl = _last_level(scene, a, d[k], grp[k])
                flags[at[k]] |= fl
                lo[at[k]], hi[at[k]] = _scale(l, u, T[k])
                kind[at[k]], level[at[k]] = np.where(mirror, TERM_MIRROR, TERM_DIFFUSE), lev
            else:
                nd, w = np.zeros((k.size, 3)), np.zeros((k.size, 3))
                go = np.ones(k.size, bool)
                if mirror.any():
                    j = mirror
                    Nj, Vj, al = a["N"][j], -d[k][j], a["rough"][j] ** 2
                    Hh, near_up = vndf_half_vector(Nj, Vj, al, phi[k][j], xi[k][j], slack) if vndf else ndf_half_vector(Nj, al, phi[k][j], xi[k][j], slack)
                    R = 2.0 * _dot(Vj, Hh)[:, None] * Hh - Vj
                    NoL = _dot(Nj, R)
                    fl = np.where(near_up, FLAG_UP, 0) | np.where(np.abs(NoL) <= NOL_EPS, FLAG_NOL, 0) | np.where((NoL > 0.0) & (NoL < GRAZING_NOL), FLAG_GRAZING_DEEP, 0)
                    flags[at[k[j]]] |= fl
                    VoH, NoH, NoV = _sat(_dot(Vj, Hh)), _sat(_dot(Nj, Hh)), _sat(_dot(Nj, Vj))
                    f0 = f0_of(a["colour"][j], a["metal"][j])
                    w[j] = vndf_weight(f0, al, NoL, VoH) if vndf else ndf_weight(f0, al, NoV, NoL, VoH, NoH)
                    nd[j] = R
                    g = go[j]; g[NoL <= 0.0] = False; go[j] = g
                    events["diff_to_refl"] += int((grp[k][j] & (NoL > 0.0)).sum())
                if (~mirror).any():
                    j = ~mirror
                    w[j] = a["colour"][j] * np.where(grp[k][j], 1.0 - a["metal"][j], 1.0)[:, None]
                    nd[j] = sphere_direction(a["N"][j], phi[k][j], xi[k][j], slack)
                    events["refl_to_diff"] += int((~grp[k][j]).sum())
                stop = k[~go]
                lo[at[stop]] = hi[at[stop]] = 0.0
                kind[at[stop]], level[at[stop]] = TERM_NOL, lev
                keep[k[go]] = True
                nxt = {"org": Pk[go], "d": nd[go], "skip": h["tri"][k][go], "T": T[k][go] * w[go], "grp": ~mirror[go],
                       "preset": a["colour"][go] * a["metal"][go][:, None],
                       "amp": amp[k][go] / np.maximum(np.abs(_dot(geo_n[h["tri"][k]], d[k]))[go], 2.0 ** -20)}
        sig[at, lev, 2] = np.where(keep, -1.0, kind[at])
        if not keep.any():
            at = at[:0]
            continue
        at, phi, xi = at[keep], phi[keep], xi[keep]
        org, d, skip, T, grp, preset, amp = nxt["org"], nxt["d"], nxt["skip"], nxt["T"], nxt["grp"], nxt["preset"], nxt["amp"]
    return {"lo": lo, "hi": hi, "flags": flags, "sig": sig.reshape(n, 3 * depth), "kind": kind, "level": level, "rays": rays, "events": events}


def eye_ray_barycentrics(proj_to_world, T, ndc):
    """Weights of the three vertices of the world-space triangles T [n 3 3] where the eye rays through ndc [n 2] meet their planes: the ray
    joins the unprojected points at depth 0 and 1; the weights solve the 2 x 2 normal equations of P - v0 = b1 e1 + b2 e2."""
    n = len(ndc)

    def unproject(z):
        p = np.concatenate([ndc, np.full((n, 1), z), np.ones((n, 1))], axis=1) @ proj_to_world
        return p[:, :3] / p[:, 3:]
    p0, p1 = unproject(0.0), unproject(1.0)
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    nrm = np.cross(e1, e2)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = _dot(T[:, 0] - p0, nrm) / _dot(p1 - p0, nrm)
        r = p0 + s[:, None] * (p1 - p0) - T[:, 0]
        g11, g12, g22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
        den = g11 * g22 - g12 * g12
        b1 = (g22 * _dot(r, e1) - g12 * _dot(r, e2)) / den
        b2 = (g11 * _dot(r, e2) - g12 * _dot(r, e1)) / den
    return np.stack([1.0 - b1 - b2, b1, b2], axis=1)


def frame(scene, fc_bytes, vis, W, H, vndf=False, prev=None, depth=1, samples=1):
    """One frame.  vis [H W] uint32: the visibility words (the rasteriser's, taken as input).  prev: the previous frame's result, for the
    words a frame carries over (RayTracingOut1 where no diffuse ray is traced, the rough-metal word where nothing is drawn).
    depth: levels of rays per path (follow_paths).  samples: N; sample k draws sample_params(W, H, FrameIndex N + k), not wrapped, and
    carries it through every level of its two paths; the pixel's interval is (sum_k v_k) / N with v_k the hull of sample k's three runs
    (0 where it traces nothing).  At depth 1 and one sample this is the depth-1 model, bit for bit (tests/test_shading_paths_host.py).
    Flags: a pixel is flagged if any segment of either path of any sample is.  The cancel rule: each whole path is evaluated three times,
    with CANCEL_SLACK as it is, taken from and added to EVERY sampler root of the path, all levels together (fp32 rounds each root on its
    own, so the three runs are a sample of the 3^D combinations, not their hull: the measured floor is the judge of that choice); the
    pixel's interval is the hull, and it is flagged FLAG_CANCEL where the three runs differ at any level in the hit triangle, the hit's
    roughness or how the path ended there.  A level >= 1 reflection with NoL < GRAZING_NOL is flagged FLAG_GRAZING_DEEP; level 0's stays
    FLAG_GRAZING with its absolute side rule (refl_graze: sum over the grazing samples of |value| / NoL, over N).
    -> dict over [H W]: covered, flags, normal_value [.. 3], rm_value [.. 2], velocity_value [.. 2], refl_lo/hi, diff_lo/hi [.. 3],
       refl_traced (by any sample), diff_traced, diff_written, rm_written, rays (all samples and levels), and the bookkeeping at the end."""
    fc = read_constants(fc_bytes)
    n = W * H
    vis = np.asarray(vis).reshape(-1).astype(np.int64)
    covered = vis > 0
    word = np.where(covered, vis - 1, 0)
    inst, prim = word >> 24, word & 0xFFFFFF
    tris, tri_inst, tri_prim = _world_triangles(scene, fc)
    first = np.array([0, len(scene.meshes[0][1])])
    tri_of = first[np.minimum(inst, 1)] + prim
    py, px = np.divmod(np.arange(n), W)
    ndc = np.stack([(px + 0.5) / W * 2.0 - 1.0, -((py + 0.5) / H * 2.0 - 1.0)], axis=1)

    def unproject(xy, z):
        p = np.concatenate([xy, np.full((n, 1), z), np.ones((n, 1))], axis=1) @ fc["proj_to_world"]
        return p[:, :3] / p[:, 3:]

    # ---- primary surface: the eye ray through the pixel centre (less the jitter) meets the triangle's plane
    ndc_b = ndc - fc["proj_bias"]
    b = eye_ray_barycentrics(fc["proj_to_world"], tris[tri_of], ndc_b)
    b[~covered] = [1.0, 0.0, 0.0]
    a = _attributes(scene, fc, np.minimum(inst, 1), np.where(covered, prim, 0), b)
    flags = np.where(covered, a["flags"], 0)
    N, rough, metal, colour = a["N"], a["rough"], a["metal"], a["colour"]
    P = np.concatenate([a["pos_obj"], np.ones((n, 1))], axis=1)
    P = np.einsum("ni,nij->nj", P, np.stack(fc["world"])[np.minimum(inst, 1)])[:, :3]
    V = _unit(fc["eye"] - P)
    hp = np.einsum("ni,nij->nj", np.concatenate([a["pos_obj"], np.ones((n, 1))], axis=1), np.stack(fc["wvp_prev"])[np.minimum(inst, 1)])
    with np.errstate(invalid="ignore", divide="ignore"):
        velocity = (ndc_b - hp[:, :2] / hp[:, 3:]) * [0.5, -0.5]
    velocity[~covered] = 0.0
    N[~covered] = 0.0

    out = {"covered": covered.reshape(H, W), "normal_value": (N * 0.5 + 0.5).reshape(H, W, 3), "rm_value": np.stack([rough, metal], axis=1).reshape(H, W, 2),
           "velocity_value": velocity.reshape(H, W, 2), "rm_written": covered.reshape(H, W)}

    refl_lo, refl_hi = np.zeros((n, 3)), np.zeros((n, 3))
    diff_lo, diff_hi = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    # ---- nothing drawn: the environment along the pixel's eye ray (no jitter) into both images
    sky = ~covered
    if sky.any():
        Vs = _unit(fc["eye"] - unproject(ndc, 0.0))
        l, h = scene.environment(-Vs[sky], 0.0)
        refl_lo[sky], refl_hi[sky] = l, h
        diff_lo[sky], diff_hi[sky] = l, h

    c = np.nonzero(covered)[0]
    geo = (tris, tri_inst, tri_prim)
    refl_traced = np.zeros(n, bool); diff_traced = np.zeros(n, bool); refl_nol = np.zeros(n); refl_graze = np.zeros(n)
    term = {"refl": np.zeros((samples, n), np.int64), "diff": np.zeros((samples, n), np.int64)}
    term_level = {"refl": np.zeros((samples, n), np.int64), "diff": np.zeros((samples, n), np.int64)}
    rays_levels, events, segs = np.zeros(depth, np.int64), dict.fromkeys(EVENTS, 0), []
    n_rays = 0

    def three_runs(run):
        """A path three times, CANCEL_SLACK as it is, taken from and added to every sampler root of the path, all levels together ->
        (hull lo, hull hi, flags, the run without slack)."""
        res = [run(slack) for slack in (0.0, -CANCEL_SLACK, CANCEL_SLACK)]
        moved = (res[0]["sig"] != res[1]["sig"]).any(axis=1) | (res[0]["sig"] != res[2]["sig"]).any(axis=1)
        return (np.minimum.reduce([r["lo"] for r in res]), np.maximum.reduce([r["hi"] for r in res]),
                res[0]["flags"] | res[1]["flags"] | res[2]["flags"] | np.where(moved, FLAG_CANCEL, 0), res[0])

    def note(image, k, r, idx):
        term[image][k, idx], term_level[image][k, idx] = r["kind"], r["level"]
        rays_levels[:] += r["rays"]
        for e in EVENTS:
            events[e] += r["events"][e]

    dk = c[metal[c] < 1.0]
    tot = {}
    for k in range(samples if c.size else 0):
        s_slot, xi = sample_params(W, H, fc["frame_index"] * samples + k)
        phi = 2.0 * np.pi * s_slot / 256.0
        Nc, Vc, Pc, al = N[c], V[c], P[c], rough[c] ** 2
        f0 = f0_of(colour[c], metal[c])
        preset = colour[c] * metal[c][:, None]

        def reflection(slack):
            Hh, near_up = vndf_half_vector(Nc, Vc, al, phi[c], xi[c], slack) if vndf else ndf_half_vector(Nc, al, phi[c], xi[c], slack)
            R = 2.0 * _dot(Vc, Hh)[:, None] * Hh - Vc
            NoL = _dot(Nc, R)
            fl = np.where(near_up, FLAG_UP, 0) | np.where(np.abs(NoL) <= NOL_EPS, FLAG_NOL, 0) | np.where((NoL > 0.0) & (NoL < GRAZING_NOL), FLAG_GRAZING, 0)
            go = NoL > 0.0
            r = {"lo": np.zeros((c.size, 3)), "hi": np.zeros((c.size, 3)), "flags": fl, "sig": np.full((c.size, 3 * depth), -2.0), "go": go, "NoL": NoL,
                 "kind": np.zeros(c.size, np.int64), "level": np.zeros(c.size, np.int64), "rays": np.zeros(depth, np.int64), "events": dict.fromkeys(EVENTS, 0)}
            if go.any():
                VoH, NoH, NoV = _sat(_dot(Vc[go], Hh[go])), _sat(_dot(Nc[go], Hh[go])), _sat(_dot(Nc[go], Vc[go]))
                wgt = vndf_weight(f0[go], al[go], NoL[go], VoH) if vndf else ndf_weight(f0[go], al[go], NoV, NoL[go], VoH, NoH)
                at = len(segs)
                p = follow_paths(scene, fc, geo, Pc[go], R[go], tri_of[c[go]], wgt, False, preset[go], phi[c[go]], xi[c[go]], depth, vndf, slack,
                                 segs, c[go])
                for sg in segs[at:]:
                    sg.update(image=0, sample=k, run=SLACK_RUNS.index(np.sign(slack)))
                r["lo"][go], r["hi"][go] = p["lo"], p["hi"]
                r["flags"][go] |= p["flags"]; r["sig"][go] = p["sig"]
                r["kind"][go], r["level"][go], r["rays"], r["events"] = p["kind"], p["level"], p["rays"], p["events"]
            return r
        l, h, fl, r0 = three_runs(reflection)
        flags[c] |= fl
        note("refl", k, r0, c)
        n_rays += int(r0["go"].sum())
        gz = (r0["NoL"] > 0.0) & (r0["NoL"] < GRAZING_NOL)
        with np.errstate(invalid="ignore", divide="ignore"):
            refl_graze[c] += np.where(gz, np.maximum(np.abs(l), np.abs(h)).max(axis=-1) / r0["NoL"], 0.0) / samples
        if k == 0:
            tot["refl"] = [l, h]
            refl_nol[c] = r0["NoL"]
        else:
            tot["refl"] = [tot["refl"][0] + l, tot["refl"][1] + h]
        refl_traced[c] |= r0["go"]
        # ---- the diffuse ray
        if dk.size:
            def diffuse(slack):
                at = len(segs)
                p = follow_paths(scene, fc, geo, P[dk], sphere_direction(N[dk], phi[dk], xi[dk], slack), tri_of[dk], colour[dk] * 0.96, True,
                                 colour[dk] * metal[dk][:, None], phi[dk], xi[dk], depth, vndf, slack, segs, dk)
                for sg in segs[at:]:
                    sg.update(image=1, sample=k, run=SLACK_RUNS.index(np.sign(slack)))
                return p
            l, h, fl, r0 = three_runs(diffuse)
            flags[dk] |= fl
            note("diff", k, r0, dk)
            n_rays += dk.size
            diff_traced[dk] = True
            tot["diff"] = [l, h] if k == 0 else [tot["diff"][0] + l, tot["diff"][1] + h]
    if c.size:
        refl_lo[c], refl_hi[c] = tot["refl"][0] / samples, tot["refl"][1] / samples
        if dk.size:
            diff_lo[dk], diff_hi[dk] = tot["diff"][0] / samples, tot["diff"][1] / samples
    diff_written = sky | diff_traced
    if prev is not None:      # what this frame does not write stays
        keep = ~diff_written
        diff_lo[keep], diff_hi[keep] = prev["diff_lo"].reshape(n, 3)[keep], prev["diff_hi"].reshape(n, 3)[keep]
        rmv = out["rm_value"].reshape(n, 2)
        rmv[sky] = prev["rm_value"].reshape(n, 2)[sky]
    out["surface"] = {"P": P, "N": N, "V": V, "rough": rough, "metal": metal, "colour": colour, "tri_of": tri_of, "covered": covered, "flags": np.where(covered, a["flags"], 0)}
    t3 = tris[tri_of]      # the error P carries in fp32: the barycentrics' (BARY_EPS) times the longest edge of the pixel's triangle
    out["surface"]["p_eps"] = BARY_EPS * np.sqrt(np.maximum.reduce([_dot(t3[:, a] - t3[:, b], t3[:, a] - t3[:, b]) for a, b in ((0, 1), (1, 2), (2, 0))]))
    out.update(flags=flags.reshape(H, W), refl_lo=refl_lo.reshape(H, W, 3), refl_hi=refl_hi.reshape(H, W, 3), diff_lo=diff_lo.reshape(H, W, 3),
               diff_hi=diff_hi.reshape(H, W, 3), refl_traced=refl_traced.reshape(H, W), diff_traced=diff_traced.reshape(H, W),
               diff_written=diff_written.reshape(H, W), refl_nol=refl_nol.reshape(H, W), rays=int(rays_levels.sum()))
    # how every sample's path ended and at which level (TERM_*; [samples H W]), the rays per level, what happened on the way, and the rays that
    # touched a surface, level by level (of all three runs: "run" indexes SLACK_RUNS)
    out.update(depth=depth, samples=samples, rays_levels=rays_levels, events=events, segments=segs, refl_graze=refl_graze.reshape(H, W),
               refl_term=term["refl"].reshape(samples, H, W), refl_term_level=term_level["refl"].reshape(samples, H, W),
               diff_term=term["diff"].reshape(samples, H, W), diff_term_level=term_level["diff"].reshape(samples, H, W))
    assert int(rays_levels[0]) == n_rays
    return out


# ---- the sun and the local lights on the primary surface (include/rtggx.h: rtggx_set_sun at angle 0, rtggx_set_lights at radius 0) --------
MIN_LIGHT_ROUGHNESS = 1.0 / 32.0
D_SLACK = 4.0 * 2.0 ** -24      # the GGX denominator NoH^2 (a^2 - 1) + 1 is a difference of numbers near 1: fp32 leaves it an absolute error of this order


def _direct_term(s, k, L, NoL, d_slack=None):
    """Specular term per unit irradiance as an interval, and the diffuse one, at the pixels k with the unit direction L to the light:
    F D Vis NoL with r' = max(r, 1/32) and H = unit(V + L); colour 0.96 NoL / pi where m < 1 (0 elsewhere).  D is monotone in its
    denominator, which is taken D_SLACK lower (not below its least value a^2) and higher: a true interval of that rounding."""
    N, V = s["N"][k], s["V"][k]
    al = np.maximum(s["rough"][k], MIN_LIGHT_ROUGHNESS) ** 2
    Hh = _unit(V + L)
    NoH, VoH, NoV = _sat(_dot(N, Hh)), _sat(_dot(V, Hh)), _sat(_dot(N, V))
    a2 = al * al
    d = NoH * NoH * (a2 - 1.0) + 1.0
    base = fresnel(f0_of(s["colour"][k], s["metal"][k]), VoH) * (vis_smith(al, NoV, NoL) * NoL)[:, None]
    d_slack = D_SLACK if d_slack is None else d_slack      # (hits_pass: the hit's carried error on top)
    hi = base * (a2 / (np.pi * np.maximum(d - d_slack, a2) ** 2))[:, None]
    lo = base * (a2 / (np.pi * (d + d_slack) ** 2))[:, None]
    diff = s["colour"][k] * 0.96 * (NoL / np.pi)[:, None] * (s["metal"][k] < 1.0)[:, None]
    return lo, hi, diff


def _shadowed(tris, s, k, L, tmax):
    """Any triangle but the pixel's own on the ray from P along L over (RAY_TMIN, tmax) -> (occluded, flags)."""
    h = closest_hit(tris, s["P"][k], L, s["tri_of"][k], tmax=tmax)
    return h["valid"], h["flags"] & (FLAG_EDGE | FLAG_TMIN)


# ---- the sampled targets (include/rtggx.h: rtggx_set_sun_angle steps 1-5, rtggx_set_lights step 5, rtggx_set_light_sampling step 3) ----------
# All of it integer up to the two draws u = (w & 0xffff) / 65536 and x = (v >> 8) / 2^24, which are exact in fp32 and here.
SLOT_STRIDE = 0x9E3779B9
SLOT_SUN, SLOT_LIGHTS, SLOT_PICK = 0, 16, 96
OUTCOME_NONE, OUTCOME_NO_RAY, OUTCOME_OCCLUDED, OUTCOME_LIT = 0, 1, 2, 3      # of a pixel's one sampled ray: no candidate / not facing, no ray, occluded, lit
FLAG_PICK, FLAG_WEIGHT, FLAG_TARGET = 2048, 4096, 8192
FLAG_NAMES.update({FLAG_PICK: "pick_boundary", FLAG_WEIGHT: "tiny_weight", FLAG_TARGET: "target_in_surface"})
# The pick compares t = x W with the running sums c_j, i.e. x with c_j / W.  Each w_i is a product of about ten fp32 factors formed from P, N
# and V, whose own error is a few 1e-6 (NOL_EPS's reason), so c_j / W is known to a few 1e-6 relative, and it is at most 1: a draw within
# PICK_EPS of a boundary may fall on either side in fp32.  (The GGX denominator's D_SLACK interval is taken on top: the boundaries are
# formed from the terms' lower and upper ends, and x is held against their hull.)
PICK_EPS = 1e-5
# A weight fp32 may flush to zero on the way (its least normal number is 1.2e-38, and a weight is a product whose factors are formed one
# by one: a partial product may underflow where the whole does not): such a light's candidacy is uncertain.
TINY_WEIGHT = 1e-30
# ds2 against 1e-6: Ds = D + rho o carries the primary surface's few 1e-6 per component, so ds2 = |Ds|^2 is off by 2 |Ds| x that, 2e-9 x a
# few at |Ds| = 1e-3: within DS2_EPS of the threshold the step may go either way.
DS2_EPS = 1e-8
# The primary surface's P in fp32: the barycentrics come from screen-space gradients and are off by a few 1e-6 -- BARY_EPS,
# with room: the worst pixels of the list and record cases show 1e-6 and 4e-6 of their triangles' 4 and 8 units --, and P by that times the
# longest edge of the pixel's triangle: frame() hands it on per pixel as surface["p_eps"].
BARY_EPS = 5e-6


def sun_slot(level=None, image=0):
    """The sun's slot: 0 for the primary pass, 1 + 2 d + i at the hit of a level-d ray of the path that writes image i."""
    return SLOT_SUN if level is None else 1 + 2 * level + image


def light_slot(i):
    """The primary target slot of light i: 16 + i below 8, 4096 + i from 8 on (rtggx_set_light_list)."""
    return SLOT_LIGHTS + i if i < 8 else 4096 + i


def light_hit_slot(level, image, i):
    return 32 + 16 * level + 8 * image + i if i < 8 else 8192 + 1024 * (2 * level + image) + i


def pick_hit_slot(level, image):
    return 104 + 2 * level + image


VIS_FLOOR = 16      # RTGGX_LIGHT_VIS_FLOOR


def visibility_weights(w, v):
    """u_i = w_i max(v_i, RTGGX_LIGHT_VIS_FLOOR) (rtggx_set_light_pick_visibility, step 3); v: the carried bytes, shaped like w."""
    return np.asarray(w, np.float64) * np.maximum(np.asarray(v, np.int64), VIS_FLOOR)


def visibility_update(v, lit):
    """Step 6, in integers: unoccluded v + ((255 - v + 3) >> 2), occluded v - ((v + 3) >> 2)."""
    v = np.asarray(v, np.int64)
    return np.where(lit, v + ((255 - v + 3) >> 2), v - ((v + 3) >> 2))


def _hash_array(seed):
    """_hash over an array of 32-bit words held in uint64."""
    seed = (np.asarray(seed, np.uint64) * np.uint64(747796405) + np.uint64(1)) & np.uint64(0xFFFFFFFF)
    seed = (((seed >> ((seed >> np.uint64(28)) + np.uint64(4))) ^ seed) * np.uint64(277803737)) & np.uint64(0xFFFFFFFF)
    return ((seed >> np.uint64(22)) ^ seed) & np.uint64(0xFFFFFFFF)


def slot_words(pixels, frame_index, slot):
    """h = rng(rng(pixel) + FrameIndex), w = rng(h + slot 0x9E3779B9), with 32-bit wraparound at every step; pixels: full-frame indices
    y W + x; slot: a number or one per pixel.  -> int64."""
    h = _hash_array((_hash_array(pixels) + np.uint64(frame_index)) & np.uint64(0xFFFFFFFF))
    step = (np.asarray(slot, np.uint64) * np.uint64(SLOT_STRIDE)) & np.uint64(0xFFFFFFFF)
    return _hash_array((h + step) & np.uint64(0xFFFFFFFF)).astype(np.int64)


def target_draw(w):
    """(u, phi) of a target's word: u = (w & 0xffff) / 65536, s = w >> 24, phi = 2 pi s / 256 (entry s of the 256-entry table)."""
    w = np.asarray(w, np.int64)
    return (w & 0xFFFF) / 65536.0, 2.0 * np.pi * (w >> 24) / 256.0


def pick_draw(v):
    """x = (v >> 8) / 2^24."""
    return (np.asarray(v, np.int64) >> 8) / 16777216.0


def sun_disk_host(direction, degrees):
    """The host's (k, T, B): in double on the fp32 L, each result rounded once to fp32 (returned as float64).  a: the axis of the smallest
    |L_i|, ties to the lowest index; T = unit(a x L); B = L x T of the unrounded T."""
    L = np.asarray(direction, np.float32).astype(np.float64)
    k = 1.0 - np.cos(float(np.float32(degrees)) * np.pi / 180.0)
    a = np.zeros(3); a[int(np.argmin(np.abs(L)))] = 1.0
    T = np.cross(a, L); T = T / np.sqrt(T @ T)
    B = np.cross(L, T)
    r = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    return float(r(k)), r(T), r(B)


def sun_disk_direction(L, k, T, B, u, phi):
    """Steps 4 and 5: e = u k, cos(theta) = 1 - e, sin(theta) = sqrt(e (2 - e)); Ls = T cos(phi) sin(theta) + B sin(phi) sin(theta) + L cos(theta)."""
    e = np.asarray(u) * k
    ct, st = 1.0 - e, np.sqrt(e * (2.0 - e))
    return T * (np.cos(phi) * st)[..., None] + B * (np.sin(phi) * st)[..., None] + np.asarray(L, np.float64) * ct[..., None]


def sphere_point(u, phi):
    """z = 1 - 2 u; rho' = sqrt(1 - z z); o = (rho' cos(phi), rho' sin(phi), z)."""
    z = 1.0 - 2.0 * np.asarray(u)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=-1)


def _facing_flags(live, c):
    """A cosine against zero: within NOL_EPS either way is a decision fp32 may take differently."""
    return np.where(live & (np.abs(c) <= NOL_EPS), FLAG_NOL, 0)


def sun_pass(scene, fc_bytes, m, direction, irradiance, angle_degrees=0.0, slot=SLOT_SUN):
    """The sun's terms of one frame m (frame()'s result).  direction: L as the host hands it on (unit, fp32); irradiance E.
    angle_degrees > 0: rtggx_set_sun_angle -- the shadow ray points at Ls, a point of the disk drawn per pixel from `slot` with the
    frame's own index; a ray exists where dot(N, L) > 0 and dot(N, Ls) > 0; the term is the directional sun's (at L).
    -> dict over [H W]: spec_lo / spec_hi / diff [.. 3] (zero where there is no term), term (a term is added), flags, rays; with an angle
       also outcome (OUTCOME_*, by the sampled ray), centre_outcome (by the ray along L) and below (facing L, but Ls below the horizon)."""
    fc = read_constants(fc_bytes)
    s = m["surface"]
    n = len(s["P"])
    L, E = np.asarray(direction, np.float64), np.asarray(irradiance, np.float64)
    tris, _, _ = _world_triangles(scene, fc)
    lo, hi, df = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    flags, term = np.zeros(n, np.int64), np.zeros(n, bool)
    outcome, centre, below = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    NoL = _dot(s["N"], L)
    flags |= np.where(s["covered"] & (np.abs(NoL) <= NOL_EPS), FLAG_NOL, 0) | np.where(s["covered"] & (NoL > 0) & (NoL < GRAZING_NOL), FLAG_GRAZING, 0)
    k = np.nonzero(s["covered"] & (NoL > 0.0))[0]
    Ls = np.broadcast_to(L, (k.size, 3))
    if angle_degrees > 0.0 and k.size:
        kk, T, B = sun_disk_host(L, angle_degrees)
        u, phi = target_draw(slot_words(k, fc["frame_index"], slot))
        Ls = sun_disk_direction(L, kk, T, B, u, phi)
        # dot(N, Ls): N's few 1e-6 as at L; Ls itself adds three rounded products and two sums of magnitude <= 1, under 1e-6: NOL_EPS holds both
        up = _dot(s["N"][k], Ls)
        flags[k] |= _facing_flags(np.ones(k.size, bool), up)
        centre[k] = np.where(_shadowed(tris, s, k, np.broadcast_to(L, (k.size, 3)), RAY_TMAX)[0], OUTCOME_OCCLUDED, OUTCOME_LIT)
        below[k[up <= 0.0]] = True
        outcome[k[up <= 0.0]] = OUTCOME_NO_RAY
        k, Ls = k[up > 0.0], Ls[up > 0.0]
    rays = k.size
    if k.size:
        # (the ray's edge flags are the sampled ray's: EDGE is sized for the origin's error; Ls adds under 1e-6 of direction)
        occ, fl = _shadowed(tris, s, k, Ls, RAY_TMAX)
        flags[k] |= fl
        outcome[k] = np.where(occ, OUTCOME_OCCLUDED, OUTCOME_LIT)
        k = k[~occ]
        l, h, d = _direct_term(s, k, np.broadcast_to(L, (k.size, 3)), NoL[k])
        lo[k], hi[k], df[k], term[k] = l * E, h * E, d * E, True
    flags |= s["flags"]
    shape = m["covered"].shape
    return {"spec_lo": lo.reshape(shape + (3,)), "spec_hi": hi.reshape(shape + (3,)), "diff": df.reshape(shape + (3,)), "term": term.reshape(shape),
            "diffuse": (term & (s["metal"] < 1.0)).reshape(shape), "flags": flags.reshape(shape), "rays": int(rays),
            "outcome": outcome.reshape(shape), "centre_outcome": centre.reshape(shape), "below": below.reshape(shape)}


def light_window(d2, R):
    """sat(1 - (d / R)^4)^2."""
    return _sat(1.0 - (d2 / (R * R)) ** 2) ** 2


def light_spot(c, cos_outer, cos_inner):
    """The cone's factor s^2, s = sat((c - cos_outer) / (cos_inner - cos_outer))."""
    return _sat((c - cos_outer) / (cos_inner - cos_outer)) ** 2


def light_attenuation(d2, R, radius=0.0, spot=1.0):
    """window x spot / max(d^2, m2) with the floor m2 = max(radius^2, 1e-4)."""
    return light_window(d2, R) * spot / np.maximum(d2, max(radius * radius, 1e-4))


def _light_reach(s, lt):
    """Steps 1-4 of rtggx_set_lights for one light at every pixel -> (live [n]: in range, facing, inside the cone; D, d2, L, NoL, att, flags,
    (att_lo, att_hi)).  The interval of att: the window's 1 - q^2 cancels towards the range's end -- d2 carries 2 d p_eps of the primary
    surface, q^2 = (d2 / R^2)^2 so 4 q d p_eps / R^2 <= 4 d p_eps / R^2, an ABSOLUTE error of the difference however small it is -- and the
    cone's s = (c - cos_outer) / (...) does towards cos_outer, by the 1e-5 of FLAG_CONE's band; both factors are monotone, so att with each
    taken that much lower and higher is a true interval, as D_SLACK's is.  lights_pass, whose terms are added to a word that is seldom zero,
    uses the value; pick_pass, whose one term may be all a pixel has, the interval."""
    n = len(s["P"])
    R = float(np.float32(lt["range"]))
    D = np.asarray(lt["position"], np.float32).astype(np.float64) - s["P"]
    d2 = _dot(D, D)
    cov = s["covered"]
    flags = np.where(cov & ((np.abs(d2 - R * R) <= 1e-5 * R * R) | (np.abs(d2 - 1e-6) <= 1e-11)), FLAG_RANGE, 0)
    live = cov & (d2 >= 1e-6) & (d2 < R * R)
    L = _unit(D)
    NoL = _dot(s["N"], L)
    flags |= np.where(live & (np.abs(NoL) <= NOL_EPS), FLAG_NOL, 0) | np.where(live & (NoL > 0) & (NoL < GRAZING_NOL), FLAG_GRAZING, 0)
    live = live & (NoL > 0.0)
    spot = spot_lo = spot_hi = np.ones(n)
    co = float(np.float32(lt.get("cos_outer", -1.0)))
    if co > -1.0:
        ci = float(np.float32(lt["cos_inner"]))
        c = -_dot(L, np.asarray(lt["axis"], np.float32).astype(np.float64))
        flags |= np.where(live & (np.abs(c - co) <= 1e-5), FLAG_CONE, 0)
        live = live & (c > co)
        spot, spot_lo, spot_hi = light_spot(c, co, ci), light_spot(c - 1e-5, co, ci), light_spot(c + 1e-5, co, ci)
    rho = float(np.float32(lt.get("radius", 0.0)))
    with np.errstate(invalid="ignore", divide="ignore"):
        att = light_attenuation(d2, R, rho, spot)
        q2, slack = (d2 / (R * R)) ** 2, 4.0 * np.sqrt(d2) * s["p_eps"] / (R * R)
        floor = np.maximum(d2, max(rho * rho, 1e-4))
        att_lo, att_hi = _sat(1.0 - q2 - slack) ** 2 * spot_lo / floor, _sat(1.0 - q2 + slack) ** 2 * spot_hi / floor
    return live, D, d2, L, NoL, att, flags, (att_lo, att_hi)


def _light_target(s, lt, k, D, slot, frame_index):
    """Steps 5 and 6 at the pixels k: the target Ds = D + rho o with o drawn from `slot` (one per pixel or one for all), ds2, Ls, tmax and
    the test dot(N, Ls) > 0.  With rho = 0 there is no hash and Ds = D.  -> (ray exists [len k], Ls, tmax, below the horizon, flags)."""
    rho = float(np.float32(lt.get("radius", 0.0)))
    Ds = D[k]
    if rho > 0.0:
        u, phi = target_draw(slot_words(k, frame_index, slot))
        Ds = Ds + rho * sphere_point(u, phi)
    ds2 = _dot(Ds, Ds)
    flags = np.where(np.abs(ds2 - 1e-6) <= DS2_EPS, FLAG_TARGET, 0)
    some = ds2 >= 1e-6
    with np.errstate(invalid="ignore", divide="ignore"):
        Ls = _unit(Ds)
    up = np.where(some, _dot(s["N"][k], Ls), 0.0)
    # dot(N, Ls): N's error as at L, and Ls's: the few 1e-6 of Ds over |Ds| (no target of a case lies nearer than the range test's 1e-3
    # ... which NOL_EPS does not hold below |Ds| = 0.1: there the band widens in proportion)
    flags |= np.where(some & (np.abs(up) <= NOL_EPS * np.maximum(1.0, 0.1 / np.sqrt(np.maximum(ds2, 1e-12)))), FLAG_NOL, 0)
    below = some & (up <= 0.0)
    return some & ~below, Ls, np.sqrt(ds2), below, flags


def lights_pass(scene, fc_bytes, m, lights, first_slot=SLOT_LIGHTS):
    """The local lights' sums of one frame: lights as dicts (position, intensity, range, radius, axis, cos_outer, cos_inner; the axis a
    unit vector), summed in their order.  A light of radius rho > 0 aims its shadow ray at a point of its sphere, drawn per pixel from the
    slot first_slot + i (i: the light's index in the list, dark lights counted) with the frame's own index; the interval ends at the target;
    the term is the centre direction's.  The ray's t within 1e-3 of tmax is closest_hit's FLAG_TMIN, as at radius 0.
    -> like sun_pass; outcome, centre_outcome, below: [count H W] per light (centre: the ray at D over (RAY_TMIN, |D|))."""
    fc = read_constants(fc_bytes)
    s = m["surface"]
    n = len(s["P"])
    tris, _, _ = _world_triangles(scene, fc)
    lo, hi, df = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    flags, term, rays = np.zeros(n, np.int64), np.zeros(n, bool), 0
    outcome, centre, below = np.zeros((len(lights), n), np.int64), np.zeros((len(lights), n), np.int64), np.zeros((len(lights), n), bool)
    for i, lt in enumerate(lights):
        I = np.asarray(lt["intensity"], np.float64)
        if not (I > 0).any():
            continue
        live, D, d2, L, NoL, att, fl, _ = _light_reach(s, lt)
        flags |= fl
        k = np.nonzero(live)[0]
        if not k.size:
            continue
        go, Ls, tmax, bel, fl = _light_target(s, lt, k, D, first_slot + i, fc["frame_index"])
        flags[k] |= fl
        below[i, k] = bel
        outcome[i, k] = OUTCOME_NO_RAY
        if float(np.float32(lt.get("radius", 0.0))) > 0.0:
            centre[i, k] = np.where(_shadowed(tris, s, k, L[k], np.sqrt(d2[k]))[0], OUTCOME_OCCLUDED, OUTCOME_LIT)
        k, Ls, tmax = k[go], Ls[go], tmax[go]
        rays += k.size
        if not k.size:
            continue
        occ, fl = _shadowed(tris, s, k, Ls, tmax)
        flags[k] |= fl
        outcome[i, k] = np.where(occ, OUTCOME_OCCLUDED, OUTCOME_LIT)
        k = k[~occ]
        l, h, d = _direct_term(s, k, L[k], NoL[k])
        lo[k] += l * (I * att[k][:, None]); hi[k] += h * (I * att[k][:, None]); df[k] += d * (I * att[k][:, None]); term[k] = True
    flags |= s["flags"]
    shape = m["covered"].shape
    return {"spec_lo": lo.reshape(shape + (3,)), "spec_hi": hi.reshape(shape + (3,)), "diff": df.reshape(shape + (3,)), "term": term.reshape(shape),
            "diffuse": (term & (s["metal"] < 1.0)).reshape(shape), "flags": flags.reshape(shape), "rays": int(rays),
            "outcome": outcome.reshape((-1,) + shape), "centre_outcome": centre.reshape((-1,) + shape), "below": below.reshape((-1,) + shape)}


def luminance(c):
    """Y(c) = 0.25 r + 0.5 g + 0.25 b."""
    return 0.25 * c[..., 0] + 0.5 * c[..., 1] + 0.25 * c[..., 2]


def pick_choice(x, weights):
    """Steps 2-5 of mode 1 for weights [n_lights, n] (0: not a candidate) and draws x [n]: W summed ascending, t = x W, the first candidate
    with t < c, else the last candidate.  -> (chosen [n] or -1, W [n], c [n_lights n] the running sums)."""
    w = np.asarray(weights, np.float64)
    cand = w > 0.0
    c = np.cumsum(np.where(cand, w, 0.0), axis=0)
    W = c[-1]
    t = x * W
    hit = cand & (t[None] < c)
    first = np.argmax(hit, axis=0)
    last = w.shape[0] - 1 - np.argmax(cand[::-1], axis=0)
    chosen = np.where(hit.any(axis=0), first, last)
    return np.where(cand.any(axis=0), chosen, -1), W, c


def pick_pass(scene, fc_bytes, m, lights, weights=None, slots=None, draw_slot=SLOT_PICK):
    """Mode 1's primary pass (rtggx_set_light_sampling, steps 0-7): per pixel the candidates' spec_i and diff_i (lights_pass's terms, before
    any ray), w_i = Y(spec_i) + Y(diff_i) -- Y(spec_i) alone at metallic >= 1 --, a candidate iff w_i > 0; W ascending; x from draw_slot,
    t = x W; the first candidate with t < c, else the last; f = W / w_i; the chosen light's target from its own slot (slots[i], default
    16 + i), one ray; unoccluded: S0 = spec_i f, S1 = diff_i f.
    weights: a function (w [n_lights n], pixel info) -> u of the same shape, the pick weights in place of w (the visibility records' u_i).
    -> like sun_pass, and chosen [H W] (-1: no candidate), outcome [H W] (OUTCOME_*), centre_outcome, below, candidates [H W] (their number),
       later [H W] (the chosen light is not the first candidate), w [count H W]."""
    fc = read_constants(fc_bytes)
    s = m["surface"]
    n, nl = len(s["P"]), len(lights)
    tris, _, _ = _world_triangles(scene, fc)
    slots = [SLOT_LIGHTS + i for i in range(nl)] if slots is None else list(slots)
    flags = np.zeros(n, np.int64)
    sp_lo, sp_hi, sp_mid, dfs, df_lo, df_hi = [np.zeros((nl, n, 3)) for _ in range(6)]
    reach = []
    metal1 = s["metal"] >= 1.0
    for i, lt in enumerate(lights):
        I = np.asarray(lt["intensity"], np.float64)
        if not (I > 0).any():
            reach.append(None)
            continue
        live, D, d2, L, NoL, att, fl, (att_lo, att_hi) = _light_reach(s, lt)
        flags |= fl
        reach.append((D, d2, L))
        k = np.nonzero(live)[0]
        l, h, d = _direct_term(s, k, L[k], NoL[k])
        sp_lo[i, k], sp_hi[i, k], dfs[i, k] = l * (I * att_lo[k][:, None]), h * (I * att_hi[k][:, None]), d * (I * att[k][:, None])
        df_lo[i, k], df_hi[i, k] = d * (I * att_lo[k][:, None]), d * (I * att_hi[k][:, None])
        sp_mid[i, k] = 0.5 * (l + h) * (I * att[k][:, None])
    w_lo, w_hi = luminance(sp_lo) + np.where(metal1[None], 0.0, luminance(df_lo)), luminance(sp_hi) + np.where(metal1[None], 0.0, luminance(df_hi))
    w_mid = luminance(sp_mid) + np.where(metal1[None], 0.0, luminance(dfs))
    flags |= np.where(((w_hi > 0.0) & (w_lo < TINY_WEIGHT)).any(axis=0), FLAG_WEIGHT, 0)
    if weights is not None:
        w_lo, w_hi, w_mid = weights(w_lo), weights(w_hi), weights(w_mid)
    x = pick_draw(slot_words(np.arange(n), fc["frame_index"], draw_slot))
    chosen, W, c = pick_choice(x, w_mid)
    # the boundaries c_j / W from the terms' lower ends, upper ends and middles: x within PICK_EPS of their hull is a decision
    flags |= np.where(_pick_boundary_flags(x, w_lo, w_mid, w_hi), FLAG_PICK, 0)
    lo, hi, df, d_lo, d_hi = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    term, rays = np.zeros(n, bool), 0
    outcome, centre, below = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)
    cand = w_mid > 0.0
    first_cand = np.argmax(cand, axis=0)
    for i, lt in enumerate(lights):
        k = np.nonzero(chosen == i)[0]
        if not k.size:
            continue
        D, d2, L = reach[i]
        go, Ls, tmax, bel, fl = _light_target(s, lt, k, D, slots[i], fc["frame_index"])
        flags[k] |= fl
        below[k] = bel
        outcome[k] = OUTCOME_NO_RAY
        if float(np.float32(lt.get("radius", 0.0))) > 0.0:
            centre[k] = np.where(_shadowed(tris, s, k, L[k], np.sqrt(d2[k]))[0], OUTCOME_OCCLUDED, OUTCOME_LIT)
        k, Ls, tmax = k[go], Ls[go], tmax[go]
        rays += k.size
        if not k.size:
            continue
        occ, fl = _shadowed(tris, s, k, Ls, tmax)
        flags[k] |= fl
        outcome[k] = np.where(occ, OUTCOME_OCCLUDED, OUTCOME_LIT)
        k = k[~occ]
        # f = W / w_i = 1 + sum over the others of w_j / w_i: exactly 1 with a single candidate; its interval from the terms' ends
        others_lo, others_hi = w_lo[:, k].sum(axis=0) - w_lo[i, k], w_hi[:, k].sum(axis=0) - w_hi[i, k]
        f_lo, f_hi = 1.0 + others_lo / w_hi[i, k], 1.0 + others_hi / w_lo[i, k]
        f_mid = W[k] / w_mid[i, k]
        lo[k], hi[k], df[k], term[k] = sp_lo[i, k] * f_lo[:, None], sp_hi[i, k] * f_hi[:, None], dfs[i, k] * f_mid[:, None], True
        d_lo[k], d_hi[k] = df_lo[i, k] * f_lo[:, None], df_hi[i, k] * f_hi[:, None]
    flags |= s["flags"]
    shape = m["covered"].shape
    return {"spec_lo": lo.reshape(shape + (3,)), "spec_hi": hi.reshape(shape + (3,)), "diff": df.reshape(shape + (3,)), "term": term.reshape(shape),
            "diff_lo": d_lo.reshape(shape + (3,)), "diff_hi": d_hi.reshape(shape + (3,)),      # (f's interval on the diffuse term too)
            "diffuse": (term & (s["metal"] < 1.0)).reshape(shape), "flags": flags.reshape(shape), "rays": int(rays),
            "chosen": chosen.reshape(shape), "outcome": outcome.reshape(shape), "centre_outcome": centre.reshape(shape), "below": below.reshape(shape),
            "candidates": cand.sum(axis=0).reshape(shape), "later": ((chosen >= 0) & (chosen != first_cand)).reshape(shape),
            "w": w_mid.reshape((nl,) + shape), "W": W.reshape(shape), "x": x.reshape(shape)}


# ---- the visibility records (include/rtggx.h: rtggx_set_light_pick_visibility), one frame at a time ----------------------------------------
RECORD = np.dtype([("v", np.uint8, 8), ("normal", np.uint32), ("stamp", np.uint32)])      # RtggxLightVisRecord
HISTORY_VALID, HISTORY_SEQUENCE, HISTORY_OFF_FRAME, HISTORY_STAMP, HISTORY_INSTANCE, HISTORY_NORMAL = range(6)      # valid, or the first condition of step 2 that fails
HISTORY_NAMES = {HISTORY_SEQUENCE: "sequence", HISTORY_OFF_FRAME: "off_frame", HISTORY_STAMP: "stamp", HISTORY_INSTANCE: "instance", HISTORY_NORMAL: "normal"}
NORMAL_LIMIT = float(np.float32(0.9) * np.float32(1046529.0))      # 0.9f * 1046529.0f, the product rounded once
FLAG_HISTORY = 16384
FLAG_NAMES[FLAG_HISTORY] = "history_tap"
# ((float)x + 0.5f) - vx (float)W: the product is rounded once and the difference once more, 2 x 2^-24 x 96 at most -- 1.2e-5 --, and vx is the
# frame's own binary16 word, an input.  Within HISTORY_EPS of an integer floor() may land on either side.
HISTORY_EPS = 1e-4


class RecordSequence:
    """s and s0 from the call history: s counts the acting frames; s0 is s at the last reset -- the allocation (the first acting frame),
    every successful rtggx_set_lights and rtggx_set_light_sampling, every change of the setting."""

    def __init__(self):
        self.s = self.s0 = 0
        self.allocated = False

    def reset(self):
        self.s0 = self.s

    def acting_frame(self):
        """-> (s, s0) of the frame: it writes image s & 1 and reads image (s - 1) & 1."""
        if not self.allocated:
            self.allocated = True
            self.reset()
        self.s += 1
        return self.s, self.s0


def _half_words(w):
    return np.asarray(w).astype(np.uint16).view(np.float16).astype(np.float64)


def _normal_integers(words):
    w = np.asarray(words).astype(np.int64)
    return np.stack([2 * (w & 1023) - 1023, 2 * ((w >> 10) & 1023) - 1023, 2 * ((w >> 20) & 1023) - 1023], axis=-1)


def records_pass(scene, fc_bytes, m, lights, read, normal_words, velocity_words, s, s0):
    """One acting frame of rtggx_set_light_pick_visibility.  read: RECORD [H W], the image (s - 1) & 1 as the context holds it in front of
    the frame; normal_words, velocity_words: the frame's own G-buffer words; (s, s0): RecordSequence.acting_frame's.
    Steps 2-6: the tap (qx, qy) = floor((x + 0.5) - vx W, (y + 0.5) - vy H); valid iff s - 1 > s0, the tap inside the frame, the record's
    stamp >> 8 == (s - 1) & 0xFFFFFF, its stamp & 0xFF == inst + 1, and the integer dot of the two normal words' 2 q - 1023 >= NORMAL_LIMIT;
    v_i the record's bytes, or 255; u_i = w_i max(v_i, 16) in place of w_i in mode 1's pick (pick_pass); where a ray was traced the chosen
    light's byte is updated (visibility_update); the record written at every covered pixel: the bytes, the normal word, (s & 0xFFFFFF) << 8
    | (inst + 1).
    -> pick_pass's result, and records (RECORD [H W], what the frame writes at covered pixels), history [H W] (HISTORY_*), carried [H W 8]."""
    H, W = m["covered"].shape
    n = H * W
    vis = m["vis"].reshape(-1).astype(np.int64)
    cov = vis > 0
    inst = np.where(cov, (vis - 1) >> 24, 0)
    py, px = np.divmod(np.arange(n), W)
    vw = np.asarray(velocity_words).reshape(-1).astype(np.int64)
    fx, fy = (px + 0.5) - _half_words(vw & 0xFFFF) * W, (py + 0.5) - _half_words(vw >> 16) * H
    flags = np.where(cov & ((np.abs(fx - np.round(fx)) <= HISTORY_EPS) | (np.abs(fy - np.round(fy)) <= HISTORY_EPS)), FLAG_HISTORY, 0)
    qx, qy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
    tap = np.asarray(read).reshape(-1)[np.where(inside, qy * W + qx, 0)]
    stamp = tap["stamp"].astype(np.int64)
    dots = (_normal_integers(tap["normal"]) * _normal_integers(np.asarray(normal_words).reshape(-1))).sum(axis=-1)
    fails = [np.full(n, not (s - 1 > s0)), ~inside, (stamp >> 8) != ((s - 1) & 0xFFFFFF), (stamp & 0xFF) != inst + 1, dots < NORMAL_LIMIT]
    history = np.full(n, HISTORY_VALID)
    for cls, f in reversed(list(zip((HISTORY_SEQUENCE, HISTORY_OFF_FRAME, HISTORY_STAMP, HISTORY_INSTANCE, HISTORY_NORMAL), fails))):
        history[f] = cls
    carried = np.where((history == HISTORY_VALID)[:, None], tap["v"].astype(np.int64), 255)
    nl = len(lights)
    p = pick_pass(scene, fc_bytes, m, lights, weights=lambda w: visibility_weights(w, carried.T[:nl]))
    chosen, outcome = p["chosen"].reshape(-1), p["outcome"].reshape(-1)
    traced = (outcome == OUTCOME_OCCLUDED) | (outcome == OUTCOME_LIT)
    v = carried.copy()
    k = np.nonzero(traced)[0]
    v[k, chosen[k]] = visibility_update(carried[k, chosen[k]], outcome[k] == OUTCOME_LIT)
    rec = np.zeros(n, RECORD)
    rec["v"], rec["normal"], rec["stamp"] = v, np.asarray(normal_words).reshape(-1), ((s & 0xFFFFFF) << 8) | (inst + 1)
    p["flags"] = p["flags"] | flags.reshape(H, W)
    p.update(records=rec.reshape(H, W), history=np.where(cov, history, -1).reshape(H, W), carried=carried.reshape(H, W, 8))
    return p


def list_pass(scene, fc_bytes, m, lights):
    """rtggx_set_light_list's primary pass: mode 1's rule over all n lights, the target of light i from light_slot(i)."""
    return pick_pass(scene, fc_bytes, m, lights, slots=[light_slot(i) for i in range(len(lights))])


# The cull's box is made of the primary surface's P in fp32 (p_eps, the block's largest), so e_c is off by as much and dist2 = |e|^2 by 2 |e| sqrt(3) p_eps; the
# squares and sums add (1 + 2^-24)^8.  Within that of RRm the comparison dist2 < RRm may go either way.


def cull_counts(m, lights):
    """The cull of rtggx_set_light_list per 8 x 8 block, in float64: lo / hi of the covered pixels' P; per casting light
    e_c = max(max(lo_c - Pl_c, Pl_c - hi_c), 0), dist2 = |e|^2, RRm = R R (1 + 2^-12); kept iff dist2 < RRm.
    -> (certain [by bx]: lights kept whatever fp32 does, uncertain [by bx]: lights whose |dist2 - RRm| is within the slack of P's error,
        covered [by bx]: the block has a covered pixel).  A block without a covered pixel keeps nothing."""
    s = m["surface"]
    H, W = m["covered"].shape
    by, bx = -(-H // 8), -(-W // 8)
    P, cov = s["P"].reshape(H, W, 3), m["covered"]
    certain, uncertain, some = np.zeros((by, bx), np.int64), np.zeros((by, bx), np.int64), np.zeros((by, bx), bool)
    cast = [lt for lt in lights if (np.asarray(lt["intensity"], np.float64) > 0).any()]
    Pl = np.array([np.asarray(lt["position"], np.float32).astype(np.float64) for lt in cast]).reshape(-1, 3)
    RRm = np.array([float(np.float32(lt["range"])) ** 2 * (1.0 + 2.0 ** -12) for lt in cast])
    for j in range(by):
        for i in range(bx):
            c = cov[8 * j:8 * j + 8, 8 * i:8 * i + 8]
            if not c.any():
                continue
            some[j, i] = True
            p = P[8 * j:8 * j + 8, 8 * i:8 * i + 8][c]
            p_eps = float(s["p_eps"].reshape(H, W)[8 * j:8 * j + 8, 8 * i:8 * i + 8][c].max())
            lo, hi = p.min(axis=0), p.max(axis=0)
            e = np.maximum(np.maximum(lo - Pl, Pl - hi), 0.0)
            dist2 = (e * e).sum(axis=1)
            slack = 2.0 * np.sqrt(3.0 * dist2) * p_eps + 3.0 * p_eps * p_eps + 8.0 * 2.0 ** -24 * RRm
            unsure = np.abs(dist2 - RRm) <= slack
            certain[j, i], uncertain[j, i] = int(((dist2 < RRm) & ~unsure).sum()), int(unsure.sum())
    return certain, uncertain, some


# ---- the sun and the lights at the surfaces the paths hit (include/rtggx.h: rtggx_set_sun_reflections, rtggx_set_light_reflections) ----------
# A cosine formed at a hit -- NoL, NoH, the cone's c -- inherits the error of the hit point and of V = -dir: the primary surface's few 1e-6,
# doubled by a reflection (test_shading_ref_host.GRAZING_NOL_ERROR has the same figure for level 0's NoL), times the factor the hit point
# carries (follow_paths: 1 / cosine of incidence over the hits so far).  The terms are monotone in each of them, so the model takes each
# that much lower and higher: a true interval, like D_SLACK.  It matters where a factor is small: NoL just above the grazing flag, the
# cone's s^2 near cos_outer, the GGX denominator away from its peak at small roughness.
HIT_COSINE_ERROR = 1e-5
LOBES = ("mirror", "diffuse_on_reflection_ray", "diffuse_on_diffuse_ray")
HIT_CLASSES = ("facing_away", "occluded", "out_of_range", "outside_cone")


def _pick_boundary_flags(x, w_lo, w_mid, w_hi):
    """x within PICK_EPS of the hull of an inner boundary c_j / W formed from the weights' lower ends, middles and upper ends -> [n] bool."""
    with np.errstate(invalid="ignore", divide="ignore"):
        fr = np.stack([np.cumsum(w, axis=0) / w.sum(axis=0) for w in (w_lo, w_mid, w_hi)])
    inner = (w_mid > 0.0) & (np.cumsum(w_mid, axis=0) < w_mid.sum(axis=0)[None])      # (the last candidate's boundary is 1: x < 1 always, and "else the last" is the same light)
    return (inner & (x[None] >= fr.min(axis=0) - PICK_EPS) & (x[None] <= fr.max(axis=0) + PICK_EPS)).any(axis=0)


def hits_pass(scene, fc_bytes, m, sun=None, lights=(), sun_angle=0.0, mode=0):
    """The sum S of one one-sample frame m (frame()'s result at any depth): for every level-d ray that touches a surface (m["segments"]) the
    term of the lobe the path uses there -- metallic > 0.5: the specular term of _direct_term with the hit's N, V = -dir, (r, m) and colour,
    its D_SLACK interval kept; otherwise colour' NoL / pi with colour' = colour (1 - m) for a diffuse-group ray and colour for a
    reflection-group one, no 0.96 -- times E (the sun: sun = (L, E)) or I att (a light: window, cone and floor as in lights_pass), unless the
    hit faces away (NoL <= 0), lies out of range or outside the cone, or anything but the hit's own triangle lies on the shadow ray from the
    hit point over (RAY_TMIN, RAY_TMAX) for the sun and (RAY_TMIN, tmax) for a light; s_d = T_d term; S per (pixel, image) over d ascending,
    the sun first, then the lights in their order.
    The sampled targets: sun_angle > 0 aims the sun's ray at the point of the disk drawn from sun_slot(d, img); a light of radius > 0 aims
    at the point of its sphere drawn from light_hit_slot(d, img, i), tmax the target's distance; both with the path's pixel and the frame's
    index, both with the second test dot(N, Ls) > 0, the term the centre direction's.  mode 1 (rtggx_set_light_sampling, or a list): per hit
    the candidates' s_i = T_d term_i, w_i = Y(s_i), the draw from pick_hit_slot(d, img), the pick and f of pick_choice, one ray at the
    chosen light's target, the term s_i f.
    -> dict: lo, hi [2 H W 3] (image 0: RayTracingOut0), mid (the unslacked run's value with no error carried), term [2 H W], flags [H W] (the frame's and the pass's own), rays,
       counts {(level, lobe or class): terms or hits}."""
    assert m["samples"] == 1, "with several samples the terms go into the fp32 sample sums: no stage to observe"
    fc = read_constants(fc_bytes)
    F = fc["frame_index"]
    tris = _world_triangles(scene, fc)[0]
    shape = m["covered"].shape
    n = shape[0] * shape[1]
    flags, rays, counts = m["flags"].reshape(-1).copy(), 0, {}
    nol0 = m["refl_nol"].reshape(-1)
    runs = [(np.zeros((2, n, 3)), np.zeros((2, n, 3)), np.zeros((2, n), bool)) for _ in SLACK_RUNS]
    mid = np.zeros((2, n, 3))

    def count(lev, name, k):
        if sg["run"] == 0:
            counts[(lev, name)] = counts.get((lev, name), 0) + int(k)

    for sg in sorted(m["segments"], key=lambda g: g["level"]):
        img, px, lev = sg["image"], sg["path"], sg["level"]
        lo, hi, term = runs[sg["run"]]
        # the throughput: the reflection path's w0 is proportional to level 0's NoL and carries its error (the grazing rule of level 0)
        t_err = HIT_COSINE_ERROR / nol0[px] if img == 0 else np.zeros(len(px))
        mirror = sg["metal"] > 0.5
        cprime = sg["colour"] * np.where(sg["diffuse_group"], 1.0 - sg["metal"], 1.0)[:, None]
        lobe = np.where(mirror, 0, np.where(sg["diffuse_group"], 2, 1))

        def facing(L, live):
            NoL = _dot(sg["N"], L)
            fl = np.where(live & (np.abs(NoL) <= NOL_EPS), FLAG_NOL, 0) | np.where(live & (NoL > 0) & (NoL < GRAZING_NOL), FLAG_GRAZING_DEEP, 0)
            flags[px] |= fl
            count(lev, "facing_away", (live & (NoL <= 0.0)).sum())
            return NoL, live & (NoL > 0.0)

        def above(k, Ls):
            """The second test dot(N, Ls) > 0 at the hits k: the cosine carries the hit's error (HIT_COSINE_ERROR x amp) -> keep [len k]."""
            up = _dot(sg["N"][k], Ls)
            flags[px[k]] |= np.where(np.abs(up) <= np.maximum(NOL_EPS, HIT_COSINE_ERROR * sg["amp"][k]), FLAG_NOL, 0)
            count(lev, "below_horizon", (up <= 0.0).sum())
            return up > 0.0

        def terms(k, L, NoL, scale):
            """s_d = T_d term at the hits k, centre direction L, as an interval and a middle -> (lo, hi, mid [len k, 3])."""
            err = HIT_COSINE_ERROR * sg["amp"][k]
            sl, sh, _ = _direct_term(sg, k, L, NoL, D_SLACK + 2.0 * err / np.maximum(np.sqrt(_dot(sg["V"][k] + L, sg["V"][k] + L)), 2.0 ** -10))
            dt = cprime[k] * (NoL / np.pi)[:, None]
            nl, nh = (np.maximum(NoL - err, 0.0) / NoL)[:, None], ((NoL + err) / NoL)[:, None]
            tl = np.where(mirror[k][:, None], sl, dt) * nl * scale[0] * sg["T"][k] * np.maximum(1.0 - t_err[k], 0.0)[:, None]
            th = np.where(mirror[k][:, None], sh, dt) * nh * scale[1] * sg["T"][k] * (1.0 + t_err[k])[:, None]
            tm = np.where(mirror[k][:, None], 0.5 * (sl + sh), dt) * (0.5 * (scale[0] + scale[1])) * sg["T"][k]
            return np.minimum(tl, th), np.maximum(tl, th), tm

        def shadow(k, ray, tmax):
            """Shadow rays of the hits k along `ray` -> unoccluded [len k]."""
            nonlocal rays
            rays += k.size if sg["run"] == 0 else 0
            if not k.size:
                return np.zeros(0, bool)
            h = closest_hit(tris, sg["P"][k], ray, sg["tri_of"][k], tmax=tmax, widen=sg["amp"][k])
            flags[px[k]] |= h["flags"] & (FLAG_EDGE | FLAG_TMIN)
            count(lev, "occluded", h["valid"].sum())
            return ~h["valid"]

        def add(k, tl, th, tm):
            lo[img, px[k]] += tl; hi[img, px[k]] += th; term[img, px[k]] = True
            if sg["run"] == 0:      # the value itself, no error carried (the specular lobe: the middle of its D_SLACK interval)
                mid[img, px[k]] += tm
            for c, name in enumerate(LOBES):
                count(lev, name, (lobe[k] == c).sum())

        def lit(k, L, NoL, tmax, scale, ray=None):
            """Shadow rays of the hits k along `ray` (default: the centre direction L); the unoccluded ones' terms x scale x T into S."""
            keep = shadow(k, L if ray is None else ray, tmax)
            if k.size:
                k, L, NoL, scale = k[keep], L[keep], NoL[keep], (scale[0][keep], scale[1][keep])
                add(k, *terms(k, L, NoL, scale))

        def reach(lt):
            """Steps 1-4 of a light at the segment's hits -> (live, D, d2, L, NoL, (scale_lo, scale_hi) [n 3])."""
            I = np.asarray(lt["intensity"], np.float64)
            R = float(np.float32(lt["range"]))
            D = np.asarray(lt["position"], np.float32).astype(np.float64) - sg["P"]
            d2 = _dot(D, D)
            flags[px] |= np.where((np.abs(d2 - R * R) <= 1e-5 * R * R) | (np.abs(d2 - 1e-6) <= 1e-11), FLAG_RANGE, 0)
            live = (d2 >= 1e-6) & (d2 < R * R)
            count(lev, "out_of_range", (~live).sum())
            L = _unit(D)
            NoL, live = facing(L, live)
            spot = (np.ones(len(px)),) * 2
            co = float(np.float32(lt.get("cos_outer", -1.0)))
            if co > -1.0:
                c = -_dot(L, np.asarray(lt["axis"], np.float32).astype(np.float64))
                err = HIT_COSINE_ERROR * sg["amp"]
                flags[px] |= np.where(live & (np.abs(c - co) <= err), FLAG_CONE, 0)
                count(lev, "outside_cone", (live & (c <= co)).sum())
                live = live & (c > co)
                ci = float(np.float32(lt["cos_inner"]))
                spot = (light_spot(c - err, co, ci), light_spot(c + err, co, ci))
            rho = float(np.float32(lt.get("radius", 0.0)))
            with np.errstate(invalid="ignore", divide="ignore"):
                scale = tuple(I * light_attenuation(d2, R, rho, sp)[:, None] for sp in spot)
            return live, D, d2, L, NoL, scale

        def target(lt, i, k, D, d2):
            """Steps 5-6 at the hits k: the target from the light's own slot -> (ray exists [len k], Ls, tmax)."""
            rho = float(np.float32(lt.get("radius", 0.0)))
            Ds = D[k]
            if rho > 0.0:
                u, phi = target_draw(slot_words(px[k], F, light_hit_slot(lev, img, i)))
                Ds = Ds + rho * sphere_point(u, phi)
            ds2 = _dot(Ds, Ds)
            flags[px[k]] |= np.where(np.abs(ds2 - 1e-6) <= DS2_EPS, FLAG_TARGET, 0)
            some = ds2 >= 1e-6
            with np.errstate(invalid="ignore", divide="ignore"):
                Ls = _unit(Ds)
            go = some.copy()
            if rho > 0.0 and some.any():
                go[some] = above(k[some], Ls[some])
            return go, Ls, np.sqrt(ds2)

        every = np.ones(len(px), bool)
        if sun is not None:
            L, E = np.asarray(sun[0], np.float64), np.asarray(sun[1], np.float64)
            NoL, live = facing(np.broadcast_to(L, (len(px), 3)), every)
            k = np.nonzero(live)[0]
            ray = None
            if sun_angle > 0.0 and k.size:
                kk, T, B = sun_disk_host(L, sun_angle)
                u, phi = target_draw(slot_words(px[k], F, sun_slot(lev, img)))
                ray = sun_disk_direction(L, kk, T, B, u, phi)
                keep = above(k, ray)
                k, ray = k[keep], ray[keep]
            lit(k, np.broadcast_to(L, (k.size, 3)), NoL[k], RAY_TMAX, (np.broadcast_to(E, (k.size, 3)),) * 2, ray)
        cast = [(i, lt) for i, lt in enumerate(lights) if (np.asarray(lt["intensity"], np.float64) > 0).any()]
        if mode == 0:
            for i, lt in cast:
                live, D, d2, L, NoL, scale = reach(lt)
                k = np.nonzero(live)[0]
                go, Ls, tmax = target(lt, i, k, D, d2)
                k = k[go]
                lit(k, L[k], NoL[k], tmax[go], (scale[0][k], scale[1][k]), Ls[go])
        elif cast:
            ns = len(px)
            s_lo, s_hi, s_mid = [np.zeros((len(lights), ns, 3)) for _ in range(3)]
            held = {}
            for i, lt in cast:
                live, D, d2, L, NoL, scale = reach(lt)
                k = np.nonzero(live)[0]
                held[i] = (D, d2)
                if k.size:
                    s_lo[i, k], s_hi[i, k], s_mid[i, k] = terms(k, L[k], NoL[k], (scale[0][k], scale[1][k]))
            w_lo, w_hi, w_mid = luminance(s_lo), luminance(s_hi), luminance(s_mid)
            flags[px] |= np.where(((w_hi > 0.0) & (w_lo < TINY_WEIGHT)).any(axis=0), FLAG_WEIGHT, 0)
            x = pick_draw(slot_words(px, F, pick_hit_slot(lev, img)))
            chosen, W, _ = pick_choice(x, w_mid)
            flags[px] |= np.where(_pick_boundary_flags(x, w_lo, w_mid, w_hi), FLAG_PICK, 0)
            count(lev, "candidates", (chosen >= 0).sum())
            count(lev, "two_candidates", ((w_mid > 0).sum(axis=0) >= 2).sum())
            for i, lt in cast:
                k = np.nonzero(chosen == i)[0]
                if not k.size:
                    continue
                go, Ls, tmax = target(lt, i, k, *held[i])
                k, Ls, tmax = k[go], Ls[go], tmax[go]
                keep = shadow(k, Ls, tmax)
                if k.size:
                    k = k[keep]
                    others_lo, others_hi = w_lo[:, k].sum(axis=0) - w_lo[i, k], w_hi[:, k].sum(axis=0) - w_hi[i, k]
                    with np.errstate(invalid="ignore", divide="ignore"):      # (a lower end of 0: flagged FLAG_WEIGHT above)
                        f_lo, f_hi, f_mid = 1.0 + others_lo / w_hi[i, k], 1.0 + others_hi / w_lo[i, k], W[k] / w_mid[i, k]
                    add(k, s_lo[i, k] * f_lo[:, None], s_hi[i, k] * f_hi[:, None], s_mid[i, k] * f_mid[:, None])
                    count(lev, "chosen_from_8", (i >= 8) * k.size)
    # the hull of the three runs (frame(): the sampler roots' slack 0, -, +), flagged where they do not agree on which terms exist
    lo, hi, term = np.minimum.reduce([r[0] for r in runs]), np.maximum.reduce([r[1] for r in runs]), runs[0][2]
    flags |= np.where(((runs[1][2] != term) | (runs[2][2] != term)).any(axis=0), FLAG_CANCEL, 0)
    return {"lo": lo.reshape((2,) + shape + (3,)), "hi": hi.reshape((2,) + shape + (3,)), "term": term.reshape((2,) + shape), "flags": flags.reshape(shape),
            "mid": mid.reshape((2,) + shape + (3,)), "rays": int(rays), "counts": counts}


def sun_hits_pass(scene, fc_bytes, m, direction, irradiance):
    return hits_pass(scene, fc_bytes, m, sun=(direction, irradiance))


def light_hits_pass(scene, fc_bytes, m, lights):
    return hits_pass(scene, fc_bytes, m, lights=lights)


def unpack_r11g11b10(words):
    c = r11g11b10_split(words)
    return np.stack([ufloat_values(6)[np.minimum(c[..., 0], 1983)], ufloat_values(6)[np.minimum(c[..., 1], 1983)], ufloat_values(5)[np.minimum(c[..., 2], 991)]], axis=-1)


# ---- distances and the code rule ------------------------------------------------------------------------------------------------------
def ulp_distance(got, lo, hi):
    """Distance of fp32 values got [.. 3] from the interval [lo, hi], in fp32 ulps of the pixel's largest channel -> [..]."""
    got = np.asarray(got, np.float64)
    d = np.maximum(np.maximum(lo - got, got - hi), 0.0)
    scale = np.maximum(np.abs(lo), np.abs(hi)).max(axis=-1)
    return d.max(axis=-1) / ulp32(scale)


def quantiles(e):
    e = np.asarray(e, np.float64).reshape(-1)
    if e.size == 0:
        return {"n": 0, "max": 0.0, "q99": 0.0, "median": 0.0}
    return {"n": int(e.size), "max": float(e.max()), "q99": float(np.quantile(e, 0.99)), "median": float(np.median(e))}


def code_rule(code_of, stored, lo, hi, delta, one_code=True):
    """A stored code may differ from the code of the model's value by at most one, and only where that value lies within delta of a
    rounding boundary: stored in [code(lo - delta), code(hi + delta)] and within one of [code(lo), code(hi)].  code_of is monotone.
    one_code: where the limit of one code holds (binary16 near zero is finer than delta: there "within delta" is all that can be asked).
    -> (violations, uses of the allowance), boolean arrays."""
    stored = np.asarray(stored).astype(np.int64)
    c_lo, c_hi = code_of(lo), code_of(hi)
    ok = (stored >= np.minimum(code_of(lo - delta), c_lo)) & (stored <= np.maximum(code_of(hi + delta), c_hi))
    ok &= ((stored >= c_lo - 1) & (stored <= c_hi + 1)) | ~np.broadcast_to(one_code, ok.shape)
    return ~ok, ok & ((stored < c_lo) | (stored > c_hi))


def f16_spacing(x):
    """The distance between neighbouring binary16 values at |x| (2^-24 below the normal range)."""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(x)) - 10.0)
