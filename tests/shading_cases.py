"""Synthetic scenes for the per-pixel tests of the shading path (tests/shading_ref.py the model, tests/test_shading_ref_host.py on the CPU,
tests/test_gpu_shading_synthetic.py on the device).  Pure numpy: two small meshes, two World matrices, a camera, materials, a cube from
tests/env_cases.py.  Each case builds its own 768-byte frame constants by the layout of include/rtggx.h -- every matrix computed in float64
and rounded once -- and the model reads World, the view-projection and the materials from those bytes: the kernel's inputs are the
model's inputs.

Frames are at most 96 x 64 and ragged (75 x 53), meshes stay below 512 triangles, cubes have sides 5, 12 and 16.  Every case runs the
frame indices FRAMES; its camera (and, where said, its second instance) moves from frame to frame, so the velocity word is nowhere a
rounding residue around zero, where binary16's denormals are finer than fp32's error of a difference of two numbers near 1.

Families (the smallest set that reaches each branch):
  transforms   non-uniform scale x rotation about a skew axis x translation on both instances (the inverse transpose matters), the same
               mirrored (negative determinant) with a ProjBias, a moving instance, previous positions off screen
  normals      vertex normals that sweep |n.y| through 0.999 on both sides of it and on both signs, exactly +-y, shading normals at
               grazing angles to the eye and turned away from it
  materials    a closed room (instance 0: the checkerboard under all three dominant axes) around a ball: 13 roughness codes from 0 to 1,
               metallic 0, 0.25, 0.75 and 1 on both instances in the four combinations of "hit side above or below 0.5", colours with a
               zero channel, a zero green, all zero and above 1, cubes of 1, 3 and 5 mips
  hits         open sky; a cone whose apex lies on a pixel centre (a ray leaves a vertex shared by 16 triangles); two coincident sheets
  vndf         normals and materials once more under rtggx_set_sampler
  sun, lights  a slab under an occluder, lit by rtggx_set_sun (angle 0) and by rtggx_set_lights (radius 0); see all_cases
The sampled lights (the sun's disk, radii, the pick, the records, the list, their targets at the hits) have lists of their own:
sampled_cases, record_cases, sampled_hit_cases."""
import functools

import numpy as np

import bvh_cases
import env_cases
import env_ref

FRAMES = (0, 1, 255)


# ---- cubes ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def smooth_cube(size=16, mips=5):
    """A low-order polynomial radiance of the direction, every level sampled at its own texel centres: slopes of a few percent per texel,
    so the rounding of a direction is not what the measured floor shows."""
    codes = []
    for m in range(mips):
        s = env_cases.side(size, m)
        d, _, _, _ = env_ref.texel_centre_dirs(s)
        d = d / np.sqrt((d * d).sum(axis=1))[:, None]
        x, y, z = d[:, 0], d[:, 1], d[:, 2]
        rgb = np.stack([2.0 + 0.75 * y + 0.5 * x * z, 1.5 + 0.5 * x - 0.25 * y * y, 1.0 + 0.5 * z + 0.25 * x * y], axis=1)
        t = np.ones((6 * s * s, 4), np.float16)
        t[:, :3] = rgb.astype(np.float16)
        codes.append(t.reshape(6, s, s, 4).view(np.uint16).copy())
    return env_cases.Cube(size, mips, codes, "smooth_%d_%dmips" % (size, mips))


@functools.lru_cache(maxsize=None)
def signed_cube(size=12, mips=3):
    """Signed values, binary16 denormals of both signs and both zeros among ordinary texels (the recipe of env_cases.special_cube without
    its +-65504 texels)."""
    rng = np.random.default_rng(4242)
    codes = []
    for m in range(mips):
        s = env_cases.side(size, m)
        t = rng.uniform(-2.0, 8.0, (6, s, s, 4)).astype(np.float16).view(np.uint16).copy()
        kind = rng.integers(0, 10, (6, s, s, 3))
        den = rng.integers(1, 0x400, (6, s, s, 3)).astype(np.uint16) | (rng.integers(0, 2, (6, s, s, 3)).astype(np.uint16) << 15)
        rgb = t[..., :3]
        rgb[kind == 0] = den[kind == 0]
        rgb[kind == 1] = 0x0000
        rgb[kind == 2] = 0x8000
        t[..., 3] = 0x3C00
        codes.append(t)
    return env_cases.Cube(size, mips, codes, "signed_%d_%dmips" % (size, mips))


@functools.lru_cache(maxsize=None)
def constant_cube():
    return env_cases.constant_cube(5, 1.5)


# ---- matrices, float64, row vectors ---------------------------------------------------------------------------------------------------
def scale(x, y, z):
    return np.diag([x, y, z, 1.0])


def translate(x, y, z):
    m = np.eye(4); m[3, :3] = (x, y, z)
    return m


def rotate(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).T
    return m


def look_at(eye, focus, up=(0.0, 1.0, 0.0)):
    eye, focus = np.asarray(eye, np.float64), np.asarray(focus, np.float64)
    z = focus - eye; z /= np.linalg.norm(z)
    x = np.cross(up, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2] = x, y, z
    m[3, :3] = (-x @ eye, -y @ eye, -z @ eye)
    return m


def perspective(fov_y, aspect, zn, zf):
    h = 1.0 / np.tan(0.5 * fov_y)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1], m[2, 2], m[2, 3], m[3, 2] = h / aspect, h, zf / (zf - zn), 1.0, -zn * zf / (zf - zn)
    return m


# ---- meshes: (verts [nv 6] float32, idx [3 n] uint32) -----------------------------------------------------------------------------------
def _mesh(pos, nrm, idx):
    v = np.concatenate([np.asarray(pos, np.float64), np.asarray(nrm, np.float64)], axis=1).astype(np.float32)
    return v, np.asarray(idx, np.uint32).reshape(-1)


def join(*meshes):
    vs, is_, at = [], [], 0
    for v, i in meshes:
        vs.append(v); is_.append(i + np.uint32(at)); at += len(v)
    return np.concatenate(vs), np.concatenate(is_)


def grid(nx, nz, x0, x1, z0, z1, y=0.0, normal=None):
    """nx x nz quads in the plane y, two triangles each, shared vertices; normal: a function of the positions [n 3] -> normals [n 3]
    (default +y)."""
    gx, gz = np.meshgrid(np.linspace(x0, x1, nx + 1), np.linspace(z0, z1, nz + 1), indexing="ij")
    pos = np.stack([gx.reshape(-1), np.full(gx.size, y), gz.reshape(-1)], axis=1)
    nrm = np.tile([0.0, 1.0, 0.0], (len(pos), 1)) if normal is None else normal(pos)
    a = (np.arange(nx)[:, None] * (nz + 1) + np.arange(nz)[None, :]).reshape(-1)
    idx = np.stack([a, a + 1, a + nz + 1, a + 1, a + nz + 2, a + nz + 1], axis=1)
    return _mesh(pos, nrm, idx)


def sphere_cap(n_ring, n_seg, radius, half_angle, centre=(0.0, 0.0, 0.0)):
    """A cap of a sphere around +y with smooth normals: an apex fan and n_ring - 1 rings of quads."""
    pos, idx = [[0.0, 1.0, 0.0]], []
    for r in range(1, n_ring + 1):
        th = half_angle * r / n_ring
        for s in range(n_seg):
            ps = 2.0 * np.pi * s / n_seg
            pos.append([np.sin(th) * np.cos(ps), np.cos(th), np.sin(th) * np.sin(ps)])
    ring = lambda r, s: 1 + (r - 1) * n_seg + s % n_seg
    for s in range(n_seg):
        idx.append([0, ring(1, s), ring(1, s + 1)])
    for r in range(1, n_ring):
        for s in range(n_seg):
            idx.append([ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)]); idx.append([ring(r, s), ring(r + 1, s + 1), ring(r, s + 1)])
    nrm = np.array(pos)
    return _mesh(nrm * radius + np.asarray(centre), nrm, idx)


def closed_ball(n_ring=6, n_seg=10, radius=1.0):
    """A UV sphere with both poles as fans and smooth normals."""
    pos = [[0.0, 1.0, 0.0]]
    for r in range(1, n_ring):
        th = np.pi * r / n_ring
        for s in range(n_seg):
            ps = 2.0 * np.pi * s / n_seg
            pos.append([np.sin(th) * np.cos(ps), np.cos(th), np.sin(th) * np.sin(ps)])
    pos.append([0.0, -1.0, 0.0])
    last = len(pos) - 1
    ring = lambda r, s: 1 + (r - 1) * n_seg + s % n_seg
    idx = []
    for s in range(n_seg):
        idx.append([0, ring(1, s), ring(1, s + 1)]); idx.append([last, ring(n_ring - 1, s + 1), ring(n_ring - 1, s)])
    for r in range(1, n_ring - 1):
        for s in range(n_seg):
            idx.append([ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)]); idx.append([ring(r, s), ring(r + 1, s + 1), ring(r, s + 1)])
    nrm = np.array(pos)
    return _mesh(nrm * radius, nrm, idx)


def room():
    """The inside of the box [-1, 1]^3: 12 triangles, per face its own four vertices with the inward axis normal."""
    pos, nrm, idx = [], [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            u, w = (axis + 1) % 3, (axis + 2) % 3
            base = len(pos)
            for a, b in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3); p[axis], p[u], p[w] = sign, a, b
                n = np.zeros(3); n[axis] = -sign
                pos.append(p); nrm.append(n)
            idx += [[base, base + 1, base + 2], [base, base + 2, base + 3]]
    return _mesh(pos, nrm, idx)


def cone(apex, base_centre, base_radius, n=16):
    """n triangles around an apex they all share, smooth normals."""
    apex, c = np.asarray(apex, np.float64), np.asarray(base_centre, np.float64)
    ax = apex - c; h = np.linalg.norm(ax); ax /= h
    u = np.cross(ax, [0.3, 0.5, 0.8]); u /= np.linalg.norm(u); w = np.cross(ax, u)
    pos, nrm = [apex], [ax]
    for s in range(n):
        ps = 2.0 * np.pi * s / n
        r = np.cos(ps) * u + np.sin(ps) * w
        pos.append(c + base_radius * r)
        nn = h * r + base_radius * ax
        nrm.append(nn / np.linalg.norm(nn))
    idx = [[0, 1 + s, 1 + (s + 1) % n] for s in range(n)]
    return _mesh(pos, nrm, idx)


def oriented(mesh, world, eye):
    """The mesh with every triangle wound so that it faces `eye` under `world` (the rasteriser culls the others): clockwise on the
    screen, which is cross(v1 - v0, v2 - v0) towards the eye."""
    v, i = mesh
    i = i.reshape(-1, 3).copy()
    p = (np.concatenate([v[:, :3].astype(np.float64), np.ones((len(v), 1))], axis=1) @ world)[:, :3]
    t = p[i]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    away = ((np.asarray(eye) - t.mean(axis=1)) * n).sum(axis=1) < 0.0
    i[away] = i[away][:, [0, 2, 1]]
    return v, i.reshape(-1).astype(np.uint32)


# ---- a case --------------------------------------------------------------------------------------------------------------------------
class Case:
    """meshes, worlds (float64 4 x 4; world1_step: translation per frame of the second instance), camera (eye, focus, eye_step per frame; pan: the focus moves with the eye),
    materials per frame position: a function k -> ((colour, rough, metal), (colour, rough, metal)), the cube, the sampler."""

    def __init__(self, name, family, W, H, mesh0, mesh1, world0, world1, eye, focus, cube, materials, vndf=False, eye_step=(0.5, 0.5, 0.0),
                 world1_step=(0.0, 0.0, 0.0), proj_bias=(0.0, 0.0), fov=0.9, pan=True, sun=None, lights=None):
        self.name, self.family, self.W, self.H = name, family, W, H
        self.world0, self.world1 = np.asarray(world0, np.float64), np.asarray(world1, np.float64)
        self.eye, self.focus, self.eye_step, self.world1_step = np.asarray(eye, np.float64), np.asarray(focus, np.float64), np.asarray(eye_step), np.asarray(world1_step)
        self.meshes = [oriented(mesh0, self.world0, self.eye), oriented(mesh1, self.world1, self.eye)]
        assert all(i.size // 3 <= 512 for _, i in self.meshes) and W <= 96 and H <= 64 and cube.size <= 16
        self.cube, self.materials, self.vndf, self.proj_bias, self.fov, self.pan = cube, materials, vndf, proj_bias, fov, pan
        self.sun, self.lights = sun, lights      # functions of the frame position: (direction, irradiance) / a list of lights as dicts (capi.Light.of's arguments), or None

    def view_proj(self, k):
        return look_at(self.eye + k * self.eye_step, self.focus + (k * self.eye_step if self.pan else 0.0)) @ perspective(self.fov, self.W / self.H, 0.1, 100.0)

    def worlds(self, k):
        return self.world0, self.world1 @ translate(*(k * self.world1_step))

    def constants(self, k, frame_index=None):
        """The 768 bytes of frame position k (frame index FRAMES[k], or frame_index); the previous matrices are those of position k - 1."""
        f = np.zeros(192, np.float32)
        vp, vp_prev = self.view_proj(k), self.view_proj(k - 1)
        for i, (w, wp) in enumerate(zip(self.worlds(k), self.worlds(k - 1))):
            f[16 * i:16 * i + 16] = (w @ vp).T.reshape(-1)
            f[32 + 16 * i:48 + 16 * i] = (wp @ vp_prev).T.reshape(-1)
            it = np.zeros((3, 4)); it[:, :3] = np.linalg.inv(w[:3, :3])      # rows of the transpose of the inverse transpose
            f[88 + 12 * i:88 + 12 * i + (12 if i == 0 else 11)] = it.reshape(-1)[:12 if i == 0 else 11]
            f[136 + 20 * i:152 + 20 * i] = (w @ vp).T.reshape(-1)
            f[152 + 20 * i:154 + 20 * i] = self.proj_bias
        f[111:112] = np.array([FRAMES[k] if frame_index is None else frame_index], np.uint32).view(np.float32)
        f[112:128] = np.linalg.inv(vp).T.reshape(-1)
        f[128:131] = self.eye + k * self.eye_step
        f[132:134] = self.proj_bias
        for i, (colour, rough, metal) in enumerate(self.materials(k)):
            f[176 + 4 * i:179 + 4 * i] = colour; f[179 + 4 * i] = 1.0
            f[184 + 4 * i:186 + 4 * i] = (rough, metal)
        return bvh_cases.frame_constants(*self.worlds(k), base=f.tobytes())


def _fixed(m0, m1):
    return lambda k: (m0, m1)


SKEW0 = scale(2.0, 0.5, 1.25) @ rotate((1.0, 2.0, 0.5), 0.35) @ translate(0.2, -1.0, 0.3)
SKEW1 = scale(1.25, 2.0, 0.5) @ rotate((0.5, -1.0, 2.0), 0.6) @ translate(-0.3, 0.4, 0.1)
MIRROR = np.diag([-1.0, 1.0, 1.0, 1.0])
ROUGH_CODES = (1.0 / 255.0, 0.02, 0.05, 0.1, 0.16, 0.25, 0.35, 0.5, 0.62, 0.8, 0.9, 1.0)      # ... and 0 on instance 0
# (metallic of instance 0, of instance 1): a hit on either side of 0.5 from either side; every value on both instances
METALS = ((0.0, 0.25), (0.25, 1.0), (0.75, 0.0), (1.0, 0.75))
COLOURS = (((0.9, 0.0, 0.5), (1.5, 1.2, 0.7)), ((0.0, 0.8, 0.6), (0.0, 0.0, 0.0)), ((0.95, 0.93, 0.88), (0.3, 0.0, 0.9)), ((0.0, 0.0, 0.0), (1.0, 0.71, 0.29)))


def _sweep_normals(eye_obj):
    """Vertex normals of the `normals` family's grid (x in [-2, 2], z in [-2, 2]):
      z < -0.7      tilted from +y by theta with cos(theta) from 0.998 (x = -2) to 1 exactly (x = 2): |n.y| crosses 0.999 inside
      -0.7 .. 0.7   the same about -y: shading normals that face away from the eye
      z > 0.7       perpendicular to the direction to the eye but for sin(beta), beta from -0.06 to 0.06 along x: NoV crosses zero"""
    def f(p):
        n = np.zeros_like(p)
        c = 0.998 + 0.002 * (p[:, 0] + 2.0) / 4.0
        c[p[:, 0] >= 2.0] = 1.0
        s = np.sqrt(np.maximum(1.0 - c * c, 0.0))
        psi = 2.5 * p[:, 2] + 0.3
        tilt = np.stack([s * np.cos(psi), c, s * np.sin(psi)], axis=1)
        down = tilt * [1.0, -1.0, 1.0]
        v = eye_obj - p; v /= np.linalg.norm(v, axis=1)[:, None]
        t = np.cross(v, [1.0, 0.0, 0.0]); t /= np.linalg.norm(t, axis=1)[:, None]
        beta = 0.06 * p[:, 0] / 2.0
        graze = np.cos(beta)[:, None] * t + np.sin(beta)[:, None] * v
        n[:] = np.where((p[:, 2] < -0.7)[:, None], tilt, np.where((p[:, 2] <= 0.7)[:, None], down, graze))
        return n
    return f


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = []
    slab = grid(2, 2, -2.0, 2.0, -2.0, 2.0)
    cap = sphere_cap(5, 12, 1.0, 1.2)
    mats = _fixed(((0.95, 0.93, 0.88), 0.5, 0.25), ((1.0, 0.71, 0.29), 0.16, 0.75))
    # ---- transforms
    cases.append(Case("skew_75x53", "transforms", 75, 53, slab, cap, SKEW0, SKEW1, (1.5, 3.0, -6.0), (0.0, -0.3, 0.0), smooth_cube(), mats,
                      eye_step=(1.5, 0.4, 0.0), world1_step=(0.05, 0.02, -0.04), pan=True))
    # ... under open sky with F0's green below 0.2 on both instances (0.03 and 0.085): where sat(50 F0.g) is 1 and a smaller factor would not be
    dark_green = _fixed(((0.9, 0.0, 0.5), 0.5, 0.25), ((1.0, 0.1, 0.29), 0.16, 0.75))
    cases.append(Case("mirrored_bias_75x53", "transforms", 75, 53, slab, cap, SKEW0 @ MIRROR, MIRROR @ SKEW1, (1.5, 3.0, -6.0), (0.0, -0.3, 0.0), smooth_cube(), dark_green,
                      proj_bias=(0.3 / 75, -0.4 / 53)))
    # ---- normals
    eye = np.array([0.5, 4.0, -5.0])
    w1 = translate(0.0, 0.0, 0.0)
    # three strips with vertices of their own: an interpolated normal never runs from one rule to the next (through zero, between +y and -y)
    sweep = join(*(grid(16, 4, -2.0, 2.0, z0, z1, normal=_sweep_normals(eye)) for z0, z1 in ((-2.0, -0.75), (-0.65, 0.65), (0.75, 2.0))))
    under = grid(1, 1, -3.0, 3.0, -3.0, 3.0, y=-0.5)
    nmats = _fixed(((0.95, 0.93, 0.88), 0.5, 0.25), ((1.0, 0.71, 0.29), 0.3, 0.75))
    for vndf in (False, True):
        cases.append(Case("normals_75x53" + ("_vndf" if vndf else ""), "vndf" if vndf else "normals", 75, 53, under, sweep, translate(0, 0, 0), w1, eye, (0.0, 0.0, 0.0),
                          smooth_cube(), nmats, vndf=vndf))
    # ---- materials: a closed room around a ball
    room0 = scale(3.0, 1.5, 2.5) @ rotate((0.3, 1.0, 0.2), 0.2) @ translate(0.0, 0.5, 0.0)
    ball1 = scale(0.8, 0.6, 0.7) @ rotate((1.0, 0.2, 0.4), 0.5) @ translate(0.3, 0.0, 0.4)
    # (the last one, where both instances are metallic and the ball's roughness is 0.8 to 1: a cube whose levels differ, so that the level a
    # roughness selects shows in the value)
    cubes = (smooth_cube(), signed_cube(), constant_cube(), env_cases.random_cube(16, 5))
    for vndf in (False, True):
        for c in range(4):
            def m(k, c=c):
                r1 = ROUGH_CODES[3 * c + k]
                r0 = 0.0 if (c, k) == (2, 1) else ROUGH_CODES[(3 * c + k + 5) % 12]
                return (COLOURS[c][0], r0, METALS[c][0]), (COLOURS[c][1], r1, METALS[c][1])
            cases.append(Case("materials_%d_64x48" % c + ("_vndf" if vndf else ""), "vndf" if vndf else "materials", 64, 48, room(), closed_ball(), room0, ball1,
                              (-2.0, 1.2, -1.6), (0.3, 0.0, 0.4), cubes[c], m, vndf=vndf, eye_step=(0.3, 0.35, 0.1)))
    # ---- hits: open sky, a shared vertex on a pixel centre, coincident sheets
    hc = Case("sheets_vertex_96x64", "hits", 96, 64, slab, slab, scale(1.5, 1.0, 1.5) @ translate(0.0, -1.0, 0.0), np.eye(4), (0.0, 2.5, -6.0), (0.0, -0.2, 0.0), smooth_cube(),
              _fixed(((0.95, 0.93, 0.88), 0.3, 0.75), ((1.0, 0.71, 0.29), 0.2, 0.25)))
    # the apex: pixel (40, 22)'s centre of frame position 0, a third of the way into the depth range, unprojected
    ndc = np.array([(40 + 0.5) / 96 * 2 - 1, -((22 + 0.5) / 64 * 2 - 1), 0.975, 1.0])
    p = ndc @ np.linalg.inv(hc.view_proj(0)); apex = p[:3] / p[3]
    sheet = grid(1, 1, -1.2, 0.2, -0.5, 1.0, y=0.6)
    mesh1 = join(sheet, sheet, cone(apex, apex + np.array([0.1, -0.5, 0.9]), 0.6))
    cases.append(Case(hc.name, "hits", 96, 64, slab, mesh1, hc.world0, np.eye(4), hc.eye, hc.focus, smooth_cube(), hc.materials))
    # ---- sun: a slab with an occluder above it; the sun at the zenith, just above the slab's horizon (NoL 0.01) and slanted, so that the cap's
    # far side lies below its own horizon; metallic 1 below (RayTracingOut1 is a carry-over there) and 0.75 above, then 0.25 and 1;
    # roughness 0.1 x 0.25 on the checkerboard's odd cells and 0.02 on the cap: both below 1 / 32
    slab0 = scale(1.5, 1.0, 1.5) @ translate(0.0, -1.0, 0.0)
    over = join(grid(2, 2, -1.3, 0.3, -1.0, 0.6, y=-0.3), sphere_cap(3, 8, 0.5, 1.3, centre=(1.2, -0.9, 0.6)))
    suns = (((0.0, 1.0, 0.0), (3.0, 2.5, 2.0)), ((1.0, 0.01, 0.2), (3.0, 2.5, 2.0)), ((0.4, 0.8, -0.3), (0.0, 2.0, 4.0)))

    def sun_mats(k):
        return (((0.95, 0.93, 0.88), 0.1, (1.0, 1.0, 0.25)[k]), ((1.0, 0.71, 0.29), 0.02, (0.75, 0.75, 1.0)[k]))
    cases.append(Case("sun_75x53", "sun", 75, 53, slab, over, slab0, np.eye(4), (0.5, 2.0, -6.0), (0.0, -0.8, 0.0), smooth_cube(), sun_mats, sun=lambda k: suns[k]))
    # ---- lights: the same scene.  A and B: point lights 0.4 and 0.25 above the slab with ranges 2.5 and 5 (pixels from 0.05 R to beyond R);
    # a spot whose two cones cross the slab; a light 0.005 above the surface (the floor m2); one above the occluder and one between it and
    # the slab (the interval ends at the light); two lights, then eight with one of zero intensity in the middle, then three
    cone_cos = lambda deg: float(np.cos(np.radians(deg)))
    spot_axis = np.array([0.1, -1.0, 0.2]) / np.linalg.norm([0.1, -1.0, 0.2])
    A = dict(position=(0.5, -0.6, 0.3), intensity=(2.0, 1.5, 1.0), range=2.5)
    B = dict(position=(-1.0, -0.75, -0.5), intensity=(0.5, 1.0, 2.0), range=5.0)
    spot = dict(position=(0.3, 1.5, -0.2), intensity=(20.0, 20.0, 16.0), range=8.0, axis=tuple(spot_axis), cos_outer=cone_cos(35.0), cos_inner=cone_cos(15.0))
    dark = dict(position=(0.0, 0.0, 0.0), intensity=(0.0, 0.0, 0.0), range=10.0)
    low = dict(position=(0.7, -0.995, -0.8), intensity=(0.002, 0.002, 0.001), range=1.0)
    above = dict(position=(-0.4, 0.5, -0.1), intensity=(6.0, 6.0, 6.0), range=6.0)
    under = dict(position=(-0.4, -0.6, -0.1), intensity=(1.0, 0.5, 0.25), range=3.0)
    far = dict(position=(2.0, 0.5, 2.0), intensity=(4.0, 8.0, 4.0), range=4.0)
    light_sets = ([A, spot], [A, B, spot, dark, low, above, under, far], [above, dark, under])
    cases.append(Case("lights_75x53", "lights", 75, 53, slab, over, slab0, np.eye(4), (0.5, 2.0, -6.0), (0.0, -0.8, 0.0), smooth_cube(),
                      _fixed(((0.95, 0.93, 0.88), 0.5, 0.25), ((1.0, 0.71, 0.29), 0.3, 1.0)), lights=lambda k: light_sets[k]))
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


NAMES = tuple(c.name for c in all_cases())
FAMILIES = tuple(sorted({c.family for c in all_cases()}))


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


# ---- runs of D levels and N samples (tests/test_shading_paths_host.py, tests/test_gpu_shading_paths.py) --------------------------------
class PathRun:
    """A case at recursion depth D with N samples per pixel, at the frame positions `positions` (indices into FRAMES, in order: a frame's
    carry-over is of the one run before it)."""

    def __init__(self, case, depth, samples, positions=(0, 1, 2)):
        self.case, self.depth, self.samples, self.positions = case, depth, samples, tuple(positions)
        self.name = "%s_d%dn%d" % (case.name, depth, samples)


@functools.lru_cache(maxsize=None)
def room_2_path_case():
    """materials_2_64x48 for paths: at frame position 2 its room is a mirror (metallic 0.75) of roughness 0.02, 0.005 on the checkerboard's odd
    cells, and at depth 2 the second bounce off such a wall takes the cancelling root twice: 2.6 % of the covered pixels are flagged, above
    the cap.  Here the room's roughness at that position is 0.35; everything else is materials_2's (its position 1 keeps roughness 0)."""
    base = by_name("materials_2_64x48")

    def m(k):
        (c0, r0, m0), one = base.materials(k)
        return (c0, 0.35 if k == 2 else r0, m0), one
    case = Case("room_2_64x48", "materials", 64, 48, room(), closed_ball(), base.world0, base.world1, base.eye, base.focus, base.cube, m, eye_step=base.eye_step)
    return case


@functools.lru_cache(maxsize=None)
def path_cases():
    """The smallest set that reaches every branch of a path (a list of its own: NAMES, FAMILIES and the depth-1 floor file do not change):
      depth in a closed room, where every path runs to the last level          materials_0, 1, 3 and room_2 (for materials_2) at D = 2
      all levels, both samplers                                                materials_3 and its VNDF twin at D = 3 and 4; materials_0 and 1
                                                                               at D = 3 and 4 under either sampler; room_2 at D = 3
      open sky: misses at level >= 1, the coincident sheets hit by a deeper ray, the apex                sheets_vertex at D = 2
      hits on non-uniformly scaled, skewed and mirrored instances (the hit's own inverse transpose)      skew, mirrored_bias at D = 2
      samples: 8 (frame index 255 reaches FrameIndex N + k = 2047), 4 and 2; samples x depth             sheets_vertex, materials_3, skew; materials_3 at D = 2, N = 2
    A run of several samples uses the frame positions 0 and 2 (indices 0 and 255).  The last four are the scenes of hit_cases(): their floor
    at the hit runs' depth is the delta of the hit stages."""
    runs = [PathRun(by_name("materials_%d_64x48" % c), 2, 1) for c in (0, 1, 3)] + [PathRun(room_2_path_case(), 2, 1)]
    runs += [PathRun(by_name("materials_3_64x48" + v), d, 1) for d in (3, 4) for v in ("", "_vndf")]
    # materials_3's room is black and fully metallic: its paths end at level 1 with the preset or carry the throughput 0 -- the preset rule, and
    # nothing else.  The levels 2 and 3 of both samplers are reached in the rooms whose walls reflect:
    runs += [PathRun(by_name("materials_0_64x48"), 3, 1, (0, 2)), PathRun(by_name("materials_1_64x48"), 4, 1, (0, 2)),
             PathRun(by_name("materials_1_64x48_vndf"), 3, 1, (0, 2)), PathRun(by_name("materials_0_64x48_vndf"), 4, 1, (0, 2)),
             PathRun(by_name("materials_1_64x48"), 2, 2, (0, 2))]
    # ... and a reflection that ends under the surface (NoL <= 0) at a level >= 1 needs a metallic wall two bounces deep
    runs += [PathRun(room_2_path_case(), 3, 1, (0, 2))]
    # the scenes of the hit passes (hit_cases): their floor at depth 2 is the hit stages' delta
    runs += [PathRun(by_name("sun_75x53"), 2, 1), PathRun(by_name("lights_75x53"), 2, 1), PathRun(court_case(), 2, 1), PathRun(court_case(), 1, 1)]
    runs += [PathRun(by_name(n), 2, 1) for n in ("sheets_vertex_96x64", "skew_75x53", "mirrored_bias_75x53")]
    runs += [PathRun(by_name("sheets_vertex_96x64"), 1, 8, (0, 2)), PathRun(by_name("materials_3_64x48"), 1, 4, (0, 2)), PathRun(by_name("skew_75x53"), 1, 2, (0, 2)),
             PathRun(by_name("materials_3_64x48"), 2, 2, (0, 2))]
    assert len({r.name for r in runs}) == len(runs)
    return tuple(runs)


def courtyard():
    """room() without its ceiling (the face y = +1): walls that second rays meet, under open sky for a sun."""
    v, i = room()
    return v, np.delete(i.reshape(-1, 3), (6, 7), axis=0).reshape(-1)


@functools.lru_cache(maxsize=None)
def court_case():
    """The walled scene of the hit passes: the materials family's room without its ceiling around the ball, walls and floor with metallic 0.25
    (the diffuse lobe, on reflection-group and on diffuse-group rays), the ball with metallic 0.75 (the mirror lobe); suns a little off
    the zenith (no wall at NoL = 0 exactly), slanted and low (the walls' and the ball's shadows); a point light under the open top, a
    small-range one behind the ball, a spot whose cones cross the floor, one of zero intensity."""
    base = by_name("materials_0_64x48")
    suns = (((0.1, 1.0, 0.05), (3.0, 2.5, 2.0)), ((0.5, 0.8, -0.3), (2.0, 2.0, 1.5)), ((1.0, 0.45, 0.2), (0.0, 2.0, 4.0)))
    axis = np.array([0.15, -1.0, 0.1]) / np.linalg.norm([0.15, -1.0, 0.1])
    top = dict(position=(-0.5, 1.6, 0.3), intensity=(6.0, 5.0, 4.0), range=7.0)
    small = dict(position=(1.2, -0.2, 1.3), intensity=(1.0, 2.0, 3.0), range=1.6)
    spot = dict(position=(0.4, 1.8, 0.2), intensity=(20.0, 20.0, 16.0), range=8.0, axis=tuple(axis), cos_outer=float(np.cos(np.radians(40.0))), cos_inner=float(np.cos(np.radians(15.0))))
    dark = dict(position=(0.0, 0.0, 0.0), intensity=(0.0, 0.0, 0.0), range=10.0)
    sets = ([top, spot], [top, small, dark, spot], [small, spot])
    return Case("court_64x48", "materials", 64, 48, courtyard(), closed_ball(), base.world0, base.world1, base.eye, base.focus, smooth_cube(),
                _fixed(((0.9, 0.8, 0.6), 0.5, 0.25), ((1.0, 0.71, 0.29), 0.3, 0.75)), eye_step=base.eye_step, sun=lambda k: suns[k], lights=lambda k: sets[k])


class HitRun:
    """A case at depth D, one sample, with the sun (kind "sun": rtggx_set_sun_reflections), the lights ("lights":
    rtggx_set_light_reflections) or both at the surfaces its paths hit.  sun, lights: functions of the frame position."""

    def __init__(self, case, depth, kind, sun=None, lights=None):
        self.case, self.depth, self.samples, self.kind, self.positions = case, depth, 1, kind, (0, 1, 2)
        self.sun = sun if kind != "lights" else None
        self.lights = lights if kind != "sun" else None
        self.name = "%s_d%d_%s_hits" % (case.name, depth, kind)


@functools.lru_cache(maxsize=None)
def hit_cases():
    """sun_75x53 and lights_75x53 at D = 1 and 2, the sun scene with its sun and the list [A, spot] at D = 2 -- under open sky few second rays
    meet anything there and both instances are metallic -- and the walled court at D = 2 with each and with both, which supplies every
    class at both levels."""
    sun, lights, court = by_name("sun_75x53"), by_name("lights_75x53"), court_case()
    runs = [HitRun(sun, d, "sun", sun=sun.sun) for d in (1, 2)] + [HitRun(lights, d, "lights", lights=lights.lights) for d in (1, 2)]
    runs += [HitRun(sun, 2, "both", sun=sun.sun, lights=lambda k: lights.lights(0))]
    runs += [HitRun(court, 2, kind, sun=court.sun, lights=court.lights) for kind in ("sun", "lights", "both")]
    return tuple(runs)


HIT_NAMES = tuple(r.name for r in hit_cases())


def hit_by_name(name):
    return next(r for r in hit_cases() if r.name == name)


# ---- the sampled lights (tests/test_shading_sampled_host.py, tests/test_gpu_shading_sampled.py) ---------------------------------------------
class SampledRun:
    """A case whose one direct pass samples visibility, at the three frame positions.  kind "sun": the case's suns under
    rtggx_set_sun_angle, every frame position once per angle of `angles`; "lights": lights(k) with radii, every light its own ray; "pick":
    lights(k) under rtggx_set_light_sampling(ctx, 1); "list": lights(k) through rtggx_set_light_list."""

    def __init__(self, name, case, kind, angles=None, lights=None):
        self.name, self.case, self.kind, self.angles, self.lights, self.positions = name, case, kind, angles, lights, (0, 1, 2)
        self.family = {"sun": "sun_disk", "lights": "radii", "pick": "pick", "list": "list"}[kind]

    def passes(self, k):
        """The passes of frame position k, each on the frame as it stands in front of it: [(label, angle or None)]."""
        return [("sun at %g degrees" % a, a) for a in self.angles] if self.kind == "sun" else [(self.kind, None)]


def slats(n, x0, width, gap, z0, z1, y):
    """n strips along z, `width` wide and `gap` apart from x0 on: 2 n edges over the slab."""
    return join(*(grid(1, 1, x0 + i * (width + gap), x0 + i * (width + gap) + width, z0, z1, y=y) for i in range(n)))


@functools.lru_cache(maxsize=None)
def slat_cases():
    """sun_75x53's and lights_75x53's scene with the occluder's one square replaced by eight slats 0.2 wide and 0.2 apart, 1 above the slab: 16
    long edges.  A single square's penumbra is a few pixels at this size -- a 10 degree disk meets about twenty pixels whose sampled ray
    differs from the centre ray --; under the slats every gap is penumbra.  The slab, the cap, the camera, the materials, the suns and the
    lights are the two cases' own, so the terms are theirs and the floor their ray-traced path records is these passes' delta."""
    sun, lights = by_name("sun_75x53"), by_name("lights_75x53")
    slab = grid(2, 2, -2.0, 2.0, -2.0, 2.0)
    over = join(slats(8, -2.4, 0.2, 0.2, -2.0, 1.5, 0.0), sphere_cap(3, 8, 0.5, 1.3, centre=(1.2, -0.9, 0.6)))
    make = lambda name, fam, base: Case(name, fam, 75, 53, slab, over, base.world0, base.world1, base.eye, base.focus, smooth_cube(), base.materials,
                                        sun=base.sun, lights=base.lights)
    return make("slats_sun_75x53", "sun", sun), make("slats_lights_75x53", "lights", lights)


@functools.lru_cache(maxsize=None)
def many_lights(n, seed=7):
    """n small lights 0.2 to 0.9 above the slab (under the slats), ranges 0.7 to 1.5 -- a block of 8 x 8 pixels is reached by a few of them --;
    every seventh dark (it keeps its index), every third with a radius of 0.2 to 0.6 (8 and 11 among them, the first slots beyond 4096; many spheres dip into the slab: targets below the horizon), every eleventh a spot that points down."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        x, y, z, r, a, b, c, rho = [float(np.round(v, 3)) for v in rng.uniform((-2.8, -0.8, -2.8, 0.7, 0.2, 0.2, 0.2, 0.2), (2.8, -0.1, 2.8, 1.5, 2.0, 2.0, 2.0, 0.6))]
        lt = dict(position=(x, y, z), range=r, intensity=(0.0, 0.0, 0.0) if i % 7 == 3 else (a, b, c))
        if i % 3 == 2:
            lt["radius"] = rho
        if i % 11 == 6:
            lt.update(axis=(0.1, -1.0, 0.05), cos_outer=float(np.cos(np.radians(50.0))), cos_inner=float(np.cos(np.radians(20.0))))
        out.append(lt)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sampled_cases():
    """The slab under the slats (slat_cases: 75 x 53, ragged 8 x 8 blocks at the right and bottom edges), frames FRAMES.
      sun disk   the three suns of sun_75x53 -- zenith, NoL 0.01 above the slab's horizon (the below-horizon targets), slanted -- each at
                 0.27, 5 and 10 degrees
      radii      the three lists of lights_75x53 with radii: small (A, 0.05), near the light's height above the slab (B: 0.25 above it,
                 radius 0.3: the sphere dips into the slab, targets below the horizon), the spot with a radius, the lights above and under
                 the slats with wide ones (their penumbrae), the dark light still in the middle of its list (the slots keep their index)
      list       12, 65 and 200 small lights (many_lights) through rtggx_set_light_list: mode 1's rule with the list's slots, and the cull
      pick       two lights and eight, with the radii above and without any, over the slab (metallic 0.25: w_i = Y(spec_i) + Y(diff_i))
                 and the slats (metallic 1: Y(spec_i) alone).  The light 0.005 above the slab is lifted to 0.2 and made brighter: where
                 it stands in lights_75x53 it would be chosen at no pixel"""
    sun, lights = slat_cases()
    runs = [SampledRun("sun_disk_75x53", sun, "sun", angles=(0.27, 5.0, 10.0))]
    radius = {(0.5, -0.6, 0.3): 0.05, (-1.0, -0.75, -0.5): 0.3, (0.3, 1.5, -0.2): 0.2, (-0.4, 0.5, -0.1): 0.4, (-0.4, -0.6, -0.1): 0.2, (2.0, 0.5, 2.0): 0.5}

    def soft(k):
        return [dict(l, radius=radius.get(tuple(l["position"]), 0.0)) for l in lights.lights(k)]

    def lifted(of, a_radius=None):
        """The lists for the pick: the light 0.005 above the slab lifted and brighter, the one under the slats brighter (each is chosen 20
        times or more); a_radius: A's radius -- above its height of 0.4, so that the light the pick takes half of the time at position 0
        has targets below the horizon."""
        change = {(0.7, -0.995, -0.8): dict(position=(0.7, -0.8, -0.8), intensity=(0.5, 0.5, 0.25), range=1.5), (-0.4, -0.6, -0.1): dict(intensity=(2.0, 1.0, 0.5))}
        if a_radius is not None:
            change[(0.5, -0.6, 0.3)] = dict(radius=a_radius)
        return lambda k: [dict(l, **change.get(tuple(l["position"]), {})) for l in of(k)]
    runs.append(SampledRun("radii_75x53", lights, "lights", lights=soft))
    # the pick: position 0 two lights, position 1 eight (one dark), position 2 the three around the slats (one dark)
    runs.append(SampledRun("pick_75x53", lights, "pick", lights=lifted(lights.lights)))
    runs.append(SampledRun("pick_radii_75x53", lights, "pick", lights=lifted(soft, a_radius=0.6)))
    # the list: 12 lights cross the slot change at 8, 65 and 200 a 64-light chunk
    for n in (12, 65, 200):
        runs.append(SampledRun("list_%d_75x53" % n, lights, "list", lights=lambda k, n=n: list(many_lights(n))))
    assert len({r.name for r in runs}) == len(runs)
    return tuple(runs)


class RecordRun:
    """A sequence of acting frames of rtggx_set_light_pick_visibility, judged one frame at a time: frame j at camera position j with the
    frame index indices[j]; lights(j): the list rtggx_set_lights is called with in front of frame j (a reset), or None; scramble: the
    frames in front of which the test overwrites the image read (where the side under test has a way to write the records)."""

    def __init__(self, name, case, indices, lights, scramble=()):
        self.name, self.case, self.indices, self.lights, self.scramble, self.family = name, case, tuple(indices), lights, tuple(scramble), "records"


@functools.lru_cache(maxsize=None)
def record_cases():
    """The slab under four wide slats and a dome (both instance 1, at different depths: under a moving camera a point of the dome that a
    slat hid a frame ago finds the slat's record -- the same instance, another normal); the camera pans by (0.6, 0.3, 0) a frame and the
    second instance moves by (0.12, 0, 0.05), so pixels change their instance, previous positions leave the frame and land on sky.  Seven
    frames (indices 0, 1, 2, 3, 255, 256, 257); four lights with radii from the start, another four from frame 4 on (a reset in the middle);
    the image frame 3 reads is overwritten: every byte v random, the stamps and normals of the left quarter as well."""
    _, lights = slat_cases()
    slab = grid(2, 2, -2.0, 2.0, -2.0, 2.0)
    # (three more slats high up, seen against the sky: a covered pixel whose tap lands beside the silhouette finds a record nobody wrote a frame ago)
    over = join(slats(4, -2.2, 0.5, 0.4, -1.6, 1.2, 0.0), sphere_cap(5, 12, 1.0, 1.3, centre=(0.4, -1.1, 0.1)), slats(3, -1.8, 0.3, 0.9, 0.5, 3.0, 1.6))
    # (the slab twice as wide as in slat_cases: it leaves the frame on three sides, so panning brings in points whose previous position is outside)
    case = Case("records_75x53", "lights", 75, 53, slab, over, scale(3.0, 1.0, 3.0) @ translate(0.0, -1.0, 0.0), np.eye(4), lights.eye, lights.focus, smooth_cube(), lights.materials,
                eye_step=(0.6, 0.3, 0.0), world1_step=(0.12, 0.0, 0.05))
    A = dict(position=(0.5, -0.6, 0.3), intensity=(2.0, 1.5, 1.0), range=3.5, radius=0.2)
    B = dict(position=(-1.0, -0.75, -0.5), intensity=(0.5, 1.0, 2.0), range=5.0, radius=0.3)
    above = dict(position=(-0.4, 0.8, -0.1), intensity=(6.0, 6.0, 6.0), range=6.0, radius=0.4)
    far = dict(position=(2.0, 0.5, 2.0), intensity=(4.0, 8.0, 4.0), range=5.0, radius=0.5)
    dark = dict(position=(0.0, 0.0, 0.0), intensity=(0.0, 0.0, 0.0), range=10.0)
    under = dict(position=(-0.4, -0.6, -0.1), intensity=(2.0, 1.0, 0.5), range=3.0, radius=0.2)
    sets = {0: [A, B, dark, above, far], 4: [above, under, dark, A, far]}
    return (RecordRun("records_75x53", case, (0, 1, 2, 3, 255, 256, 257), lambda j: sets.get(j), scramble=(3,)),)


class SampledHitRun:
    """The court at depth D, one sample, with sampled targets at the surfaces its paths hit: the sun under an angle, lights with radii in
    mode 1 (rtggx_set_light_sampling), or a list (rtggx_set_light_list)."""

    def __init__(self, name, case, depth, sun=None, angle=0.0, lights=None, mode=0, as_list=False):
        self.name, self.case, self.depth, self.samples, self.positions = name, case, depth, 1, (0, 1, 2)
        self.sun, self.angle, self.lights, self.mode, self.as_list, self.family = sun, angle, lights, mode, as_list, "hits"


@functools.lru_cache(maxsize=None)
def court_lights(n, seed=11):
    """n lights inside the court's walls, ranges 2 to 5, every fourth with a radius, every seventh dark."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        x, y, z, r, a, b, c, rho = [float(np.round(v, 3)) for v in rng.uniform((-2.4, -0.6, -1.9, 2.0, 0.5, 0.5, 0.5, 0.1), (2.4, 1.6, 1.9, 5.0, 4.0, 4.0, 4.0, 0.4))]
        lt = dict(position=(x, y, z), range=r, intensity=(0.0, 0.0, 0.0) if i % 7 == 5 else (a, b, c))
        if i % 4 == 1:
            lt["radius"] = rho
        out.append(lt)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sampled_hit_cases():
    """The court at D = 2: its suns at 5 degrees (slots 1 + 2 d + i); its lights with radii in mode 1 (targets 32 + 16 d + 8 img + i, draws
    104 + 2 d + img); a list of 12 (targets 8192 + 1024 (2 d + img) + i from light 8 on)."""
    court = court_case()
    radius = {(-0.5, 1.6, 0.3): 0.3, (1.2, -0.2, 1.3): 0.15, (0.4, 1.8, 0.2): 0.25}

    def soft(k):
        return [dict(l, radius=radius.get(tuple(l["position"]), 0.0)) for l in court.lights(k)]
    return (SampledHitRun("court_d2_sun_5_degrees", court, 2, sun=court.sun, angle=5.0),
            SampledHitRun("court_d2_pick_radii", court, 2, lights=soft, mode=1),
            SampledHitRun("court_d2_list_12", court, 2, lights=lambda k: list(court_lights(12)), mode=1, as_list=True))


SAMPLED_NAMES = tuple(r.name for r in sampled_cases())


def sampled_by_name(name):
    return next(r for r in sampled_cases() if r.name == name)


PATH_NAMES = tuple(r.name for r in path_cases())


def path_by_name(name):
    return next(r for r in path_cases() if r.name == name)
