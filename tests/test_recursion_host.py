"""Recursion depth without a GPU (rtggx_set_max_recursion_depth, -recursion N; include/rtggx.h, DESIGN.md "Recursion depth"): the ABI
surface, the command line's refusals before any GPU is touched, and the CPU restatement (tests/recursion_ref.cpp) at depth 1 against the
oracle's own depth-1 renderer, bit for bit, through the restatement's generalised path loop."""
import numpy as np
import pytest

import host_support as HS
import restatement as RS
from oracle import oracle as O


def test_set_max_recursion_depth_is_declared_exported_and_bound(built):
    HS.declared_exported_bound("rtggx_set_max_recursion_depth", r"\bint\s+rtggx_set_max_recursion_depth\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*uint32_t\s+depth\s*\)",
                               defines=[r"#define\s+RTGGX_MAX_RECURSION_DEPTH\s+4u?\b"])


def test_executable_refuses_bad_depths_before_touching_a_gpu(built):
    HS.executable_refuses((["-recursion", "0"], ["-recursion", "5"], ["-recursion"], ["/RECURSION", "-1"], ["-recursion", "9", "-gpus", "2"],
                           ["-Recursion", "x", "-strips", "2"]), "-recursion", no_device_message="no HIP device")


@pytest.mark.parametrize("mesh,W,H", [("triangle.obj", 64, 48), ("bunny.obj", 96, 54), ("dragon.obj", 80, 60)], ids=["triangle", "bunny", "dragon"])
@pytest.mark.parametrize("metallic", [(1.0, 1.0), (0.25, 0.5)], ids=["metal", "diffuse"])
@pytest.mark.parametrize("vndf", [False, True], ids=["ndf", "vndf"])
def test_restatement_at_depth_1_equals_the_oracle(built, mesh, W, H, metallic, vndf):
    o = RS.Oracle(W, H, depth=1, entry="depth")
    try:
        HS.scene(o, mesh, W, H, metallic, vndf, frame=1)
        HS.poison(o)
        ref_rays = o.ray_trace_depth1_oracle()
        ref = {b: o.buffer(b) for b in HS.RAW_BUFS}
        HS.poison(o)
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
    o = RS.Oracle(W, H, depth=1, entry="depth")
    try:
        HS.scene(o, "bunny.obj", W, H, (1.0, 0.5), False, frame=0)
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
