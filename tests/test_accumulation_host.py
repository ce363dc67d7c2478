"""Progressive accumulation without a GPU (rtggx_set_accumulation, -accumulate N; include/rtggx.h, DESIGN.md "Progressive accumulation"): the
ABI surface, the command line's refusals before any GPU is touched, and the numpy restatement (tests/accum_ref.py) on the CPU oracle's
frames -- a still camera, FrameIndex 0 .. 255 set by hand: its fp32 sums against float64 sums, the error of the n-frame mean, and the
background, which holds one word in every frame."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import accum_ref as AR
import host_support as HS
from oracle import oracle as O


def test_accumulation_is_declared_exported_and_bound(built):
    from raytracedggx_amd import app, capi
    for symbol, signature in (("rtggx_set_accumulation", r"\bint\s+rtggx_set_accumulation\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*int\s+enable\s*\)"),
                              ("rtggx_reset_accumulation", r"\bint\s+rtggx_reset_accumulation\s*\(\s*rtggx_context\s*\*\s*ctx\s*\)"),
                              ("rtggx_accumulated_frames", r"\bint\s+rtggx_accumulated_frames\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*uint32_t\s*\*\s*frames\s*\)"),
                              ("rtggx_present_accumulation", r"\bint\s+rtggx_present_accumulation\s*\(\s*rtggx_context\s*\*\s*ctx\s*\)")):
        HS.declared_exported_bound(symbol, signature)
    header = open(os.path.join(HS.ROOT, "include", "rtggx.h")).read()
    for name, value in (("RTGGX_BUF_ACC_REFL", 25), ("RTGGX_BUF_ACC_DIFF", 26), ("RTGGX_BUF_CONVERGED", 27), ("RTGGX_BUF_COUNT", 28)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), header), name
    assert (capi.BUF_ACC_REFL, capi.BUF_ACC_DIFF, capi.BUF_CONVERGED) == (25, 26, 27)
    assert "rtggx_app_save_converged" in app.HOST_EXPORTS and hasattr(C.CDLL(app.HOST_LIB_PATH), "rtggx_app_save_converged")
    assert callable(getattr(app.RayTracedGGX, "save_converged", None))


def test_executable_refuses_bad_accumulate_flags_before_touching_a_gpu(built):
    HS.executable_refuses((["-accumulate", "0"], ["-accumulate", "-3"], ["-accumulate"], ["/ACCUMULATE", "x"], ["-Accumulate", "-frames", "4"],
                           ["-accumulate", "8", "-rayrate", "4"], ["-rayrate", "4", "-accumulate", "8"], ["-accumulate", "8", "-gpus", "2"],
                           ["-gpus", "2", "-accumulate", "8"], ["-accumulate", "8", "-strips", "2"], ["-strips", "3", "-accumulate", "2", "-frames", "4"]),
                          "-accumulate")


# ---- the restatement on the oracle's frames ----------------------------------------------------------------------------------------
W, H, FRAMES = 96, 54, 256


def _frames(metallic):
    """The oracle's bunny at 96x54, still camera and model, one ray trace per FrameIndex 0 .. 255: (visibility, refl words [256, H, W],
    diff words [256, H, W])."""
    o = O.Oracle(W, H)
    try:
        HS.scene(o, "bunny.obj", metallic=metallic, frame=1)
        vis = o.buffer(O.BUF_VISIBILITY)
        refl, diff = np.zeros((FRAMES, H, W), np.uint32), np.zeros((FRAMES, H, W), np.uint32)
        for f in range(FRAMES):
            HS.set_frame_index(o, f)
            o.ray_trace()
            refl[f], diff[f] = o.buffer(O.BUF_RT_REFL), o.buffer(O.BUF_RT_DIFF)
        return vis, refl, diff
    finally:
        o.close()


@pytest.fixture(scope="module", params=[(1.0, 1.0), (0.25, 0.5)], ids=["metal", "diffuse"])
def run(built, request):
    """The frames once per material, the restatement's sums after 1, 16, 64 and 256 of them, and the float64 sums of the same addends."""
    metallic = request.param
    vis, refl, diff = _frames(metallic)
    acc = AR.Accumulator(H, W)
    exact = {"refl": np.zeros((H, W, 4)), "diff": np.zeros((H, W, 4))}
    absum = {"refl": np.zeros((H, W, 4)), "diff": np.zeros((H, W, 4))}
    dmask = AR.diffuse_mask(vis, metallic)
    at = {}
    for f in range(FRAMES):
        acc.add(refl[f], diff[f], vis, metallic)
        for name, words, mask in (("refl", refl[f], np.ones((H, W), bool)), ("diff", diff[f], dmask)):
            rgb = AR.unpack_r11g11b10f(words)
            y = AR.luma(rgb)
            v = np.concatenate([rgb, (y * y)[..., None]], axis=-1).astype(np.float64) * mask[..., None]      # the fp32 addends, summed in float64
            exact[name] += v; absum[name] += np.abs(v)
        if acc.frames in (1, 16, 64, 256):
            at[acc.frames] = (acc.refl.copy(), acc.diff.copy())
    return {"metallic": metallic, "vis": vis, "refl": refl, "diff": diff, "dmask": dmask, "acc": acc, "at": at, "exact": exact, "absum": absum}


def test_fp32_sums_stay_within_the_summation_bound_of_float64_sums(run):
    """A sequential fp32 sum of n non-negative addends differs from their exact sum by at most (n - 1) 2^-24 sum |v| to first order (each of
    the n - 1 additions rounds by at most 2^-24 of a partial sum, and no partial sum exceeds the total)."""
    assert run["acc"].frames == FRAMES
    for name, got in (("refl", run["acc"].refl), ("diff", run["acc"].diff)):
        want, bound = run["exact"][name], (FRAMES - 1) * 2.0 ** -24 * run["absum"][name]
        assert np.isfinite(want).all()
        err = np.abs(got.astype(np.float64) - want)
        print("%s %s: %.3f %% of the values differ from the float64 sum, worst error / bound %.3f" %
              (run["metallic"], name, 100.0 * (err > 0).mean(), (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
    assert not run["acc"].diff[~run["dmask"]].any(), "the diffuse sums are touched only where a diffuse path writes"
    assert run["dmask"].any() == (min(run["metallic"]) < 1.0)


def test_the_mean_converges_towards_the_256_frame_mean(run):
    """Covered pixels of each image: MSE of the n-frame mean against the 256-frame mean, below 1/4 of n = 1's at n = 16 and below 1/16 at
    n = 64 (independent draws would give 0.059 and 0.012).  Guards against "not averaged", not quality figures."""
    covered = run["vis"] != 0
    assert covered.sum() > 500
    images = [("refl", 0, covered)] + ([("diff", 1, run["dmask"])] if run["dmask"].any() else [])
    for name, k, mask in images:
        ref = AR.mean_variance(run["at"][256][k], 256)[0][mask]
        mse = {n: ((AR.mean_variance(run["at"][n][k], n)[0][mask] - ref) ** 2).mean() for n in (1, 16, 64)}
        print("%s %s: MSE %.4g at n = 1, ratio %.4f at 16, %.4f at 64" % (run["metallic"], name, mse[1], mse[16] / mse[1], mse[64] / mse[1]))
        assert mse[1] > 0.0
        assert mse[16] < mse[1] / 4.0 and mse[64] < mse[1] / 16.0, (name, mse)


def test_background_pixels_hold_one_word_and_have_no_variance(run):
    """The primary direction does not see the jitter: a background pixel holds the same environment word in every frame.  So the float64
    variance of its Y over the frames is exactly 0, and the variance derived from the fp32 sums is within the rounding of sum Y^2:
    n 2^-24 Y^2 (n - 1 additions and the square itself, each 2^-24 relative)."""
    sky = run["vis"] == 0
    assert sky.sum() > 500
    refl = run["refl"][:, sky]
    assert (refl == refl[0]).all()
    y = AR.luma(AR.unpack_r11g11b10f(refl)).astype(np.float64)
    assert np.isfinite(y).all()
    assert (y.var(axis=0) == 0.0).all()
    mean, var = AR.mean_variance(run["acc"].refl, FRAMES)
    np.testing.assert_array_equal(mean[sky], AR.unpack_r11g11b10f(refl[0]).astype(np.float64))      # 256 equal 7-bit addends: the sums are exact
    assert (np.abs(var[sky]) <= FRAMES * 2.0 ** -24 * y[0] ** 2).all()
    covered_var = AR.mean_variance(run["acc"].refl, FRAMES)[1][~sky]
    assert (covered_var > 0).mean() > 0.9, "the jittered pixels do vary"
