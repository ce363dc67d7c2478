"""Recursion depth without a GPU (rtggx_set_max_recursion_depth, -recursion N; include/rtggx.h, DESIGN.md "Recursion depth"): the ABI
surface, the command line's refusals before any GPU is touched, and the CPU restatement (tests/recursion_ref.cpp) at depth 1 against the
oracle's own depth-1 renderer, bit for bit, through the restatement's generalised path loop."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import assets
import recursion_ref as RR
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_set_max_recursion_depth_is_declared_exported_and_bound(built):
    from raytracedggx_amd import capi
    header = open(os.path.join(ROOT, "include", "rtggx.h")).read()
    assert re.search(r"\bint\s+rtggx_set_max_recursion_depth\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*uint32_t\s+depth\s*\)", header)
    assert re.search(r"#define\s+RTGGX_MAX_RECURSION_DEPTH\s+4u?\b", header)
    assert hasattr(C.CDLL(capi.LIB_PATH), "rtggx_set_max_recursion_depth")
    assert "rtggx_set_max_recursion_depth" in capi.EXPORTS
    assert callable(getattr(capi.Context, "set_max_recursion_depth", None))


def test_executable_refuses_bad_depths_before_touching_a_gpu(built):
    exe = os.path.join(ROOT, "raytracedggx_amd", "RayTracedGGX")
    scene = ["-mesh", assets.path("triangle.obj"), "-env", assets.path("rnl_cross.dds"), "-width", "64", "-height", "64"]
    for extra in (["-recursion", "0"], ["-recursion", "5"], ["-recursion"], ["/RECURSION", "-1"], ["-recursion", "9", "-gpus", "2"],
                  ["-Recursion", "x", "-strips", "2"]):
        r = subprocess.run([exe] + scene + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (extra, r.returncode, r.stderr)
        assert "-recursion" in r.stderr, (extra, r.stderr)
        assert "no HIP device" not in r.stderr and "rank" not in r.stderr.lower(), (extra, r.stderr)


def _scene(o, mesh, W, H, metallic, vndf, frame):
    v, i, _ = O.obj_import(assets.path(mesh))
    o.set_mesh(1, v, i)
    if mesh == "triangle.obj":
        o.set_env_rgba16f(1, 1, assets.constant_env_rgba16f(1.0))
    else:
        o.set_env_dds(assets.path("rnl_cross.dds"))
    o.set_metallic(0, metallic[0]); o.set_metallic(1, metallic[1])
    o.set_sampler(vndf)
    o.build_as()
    o.transform_sh()
    for _ in range(frame + 1):      # (FrameIndex and the model's turn advance with every frame)
        o.update_frame((10, 10, -24), O.camera_view_proj(W, H), 0.25)
    o.update_as()
    o.render_visibility()


@pytest.mark.parametrize("mesh,W,H", [("triangle.obj", 64, 48), ("bunny.obj", 96, 54), ("dragon.obj", 80, 60)], ids=["triangle", "bunny", "dragon"])
@pytest.mark.parametrize("metallic", [(1.0, 1.0), (0.25, 0.5)], ids=["metal", "diffuse"])
@pytest.mark.parametrize("vndf", [False, True], ids=["ndf", "vndf"])
def test_restatement_at_depth_1_equals_the_oracle(built, mesh, W, H, metallic, vndf):
    o = RR.Oracle(W, H, depth=1)
    try:
        _scene(o, mesh, W, H, metallic, vndf, frame=1)
        bufs = (O.BUF_RT_REFL, O.BUF_RT_DIFF, O.BUF_NORMAL, O.BUF_ROUGH_METAL, O.BUF_VELOCITY)

        def poison():      # (a word either renderer leaves alone stays poisoned in both)
            for b in bufs:
                o.buffer(b, copy=False)[...] = 0xBEEF if b == O.BUF_ROUGH_METAL else 0xDEADBEEF
        poison()
        ref_rays = o.ray_trace_depth1_oracle()
        ref = {b: o.buffer(b) for b in bufs}
        poison()
        rays = o.ray_trace()
        assert rays == ref_rays > 0
        for b, want in ref.items():
            np.testing.assert_array_equal(o.buffer(b), want, err_msg="buffer %d" % b)
        covered = o.buffer(O.BUF_VISIBILITY) != 0
        assert (ref[O.BUF_RT_DIFF][covered] != 0xDEADBEEF).any() == (min(metallic) < 1.0)      # (diffuse paths where there are some)
    finally:
        o.close()


def test_deeper_paths_trace_more_rays_and_change_the_image(built):
    """Depth 2 and 3 on the bunny with a diffuse model: the same G-buffer, more rays per level, and different raw images -- where a
    level-1 ray hits something.  Depth 1 returns to the oracle's image."""
    W, H = 96, 54
    o = RR.Oracle(W, H, depth=1)
    try:
        _scene(o, "bunny.obj", W, H, (1.0, 0.5), False, frame=0)
        r1 = o.ray_trace(); img1 = o.buffer(O.BUF_RT_REFL), o.buffer(O.BUF_RT_DIFF)
        o.set_max_recursion_depth(2); r2 = o.ray_trace(); img2 = o.buffer(O.BUF_RT_REFL), o.buffer(O.BUF_RT_DIFF)
        o.set_max_recursion_depth(3); r3 = o.ray_trace()
        assert r1 < r2 < r3 <= 3 * r1
        assert (img1[0] != img2[0]).any() and (img1[1] != img2[1]).any()
        o.set_max_recursion_depth(1)
        assert o.ray_trace() == r1
        np.testing.assert_array_equal(o.buffer(O.BUF_RT_REFL), img1[0])
        np.testing.assert_array_equal(o.buffer(O.BUF_RT_DIFF), img1[1])
    finally:
        o.close()
