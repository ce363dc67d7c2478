"""Samples per pixel without a GPU (rtggx_set_samples_per_pixel, -spp N; include/rtggx.h, DESIGN.md "Samples per pixel"): the ABI surface,
the command line's refusals before any GPU is touched, and the CPU restatement (tests/spp_ref.cpp): at one sample it is the oracle's own
renderer bit for bit, its samples are those of N consecutive one-sample frames, averaging them reduces the error, and it traces N times
the rays."""
import numpy as np
import pytest

import host_support as HS
import restatement as RS
from oracle import oracle as O


def test_set_samples_per_pixel_is_declared_exported_and_bound(built):
    HS.declared_exported_bound("rtggx_set_samples_per_pixel", r"\bint\s+rtggx_set_samples_per_pixel\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*uint32_t\s+samples\s*\)",
                               defines=[r"#define\s+RTGGX_MAX_SAMPLES_PER_PIXEL\s+8u?\b"])


def test_executable_refuses_bad_sample_counts_before_touching_a_gpu(built):
    HS.executable_refuses((["-spp", "0"], ["-spp", "3"], ["-spp", "16"], ["-spp"], ["/SPP", "x"], ["-Spp", "-2"], ["-spp", "2", "-rayrate", "4"],
                           ["-rayrate", "4", "-spp", "8"], ["-spp", "3", "-gpus", "2"], ["-spp", "x", "-strips", "2"]), "-spp")


@pytest.mark.parametrize("mesh,W,H", [("triangle.obj", 64, 48), ("bunny.obj", 96, 54), ("dragon.obj", 80, 60)], ids=["triangle", "bunny", "dragon"])
@pytest.mark.parametrize("metallic", [(1.0, 1.0), (0.25, 0.5)], ids=["metal", "diffuse"])
@pytest.mark.parametrize("vndf", [False, True], ids=["ndf", "vndf"])
def test_restatement_at_one_sample_equals_the_oracle(built, mesh, W, H, metallic, vndf):
    """N = 1, depth 1: the oracle's own orc_ray_trace; N = 1, depth 2: tests/recursion_ref.cpp's orc_ray_trace_depth.  Both raw images,
    normal, rough/metal, velocity, bit for bit, and the ray count."""
    o = RS.Oracle(W, H, depth=1, samples=1, entry="spp")
    try:
        HS.scene(o, mesh, W, H, metallic, vndf, frame=1)
        for depth, reference in ((1, o.ray_trace_oracle), (2, o.ray_trace_depth_restatement)):
            o.set_max_recursion_depth(depth)
            HS.poison(o)
            ref_rays = reference()
            ref = {b: o.buffer(b) for b in HS.RAW_BUFS}
            HS.poison(o)
            rays = o.ray_trace()
            assert rays == ref_rays > 0
            for b, want in ref.items():
                np.testing.assert_array_equal(o.buffer(b), want, err_msg="depth %d buffer %d" % (depth, b))
            covered = o.buffer(O.BUF_VISIBILITY) != 0
            assert (ref[O.BUF_RT_DIFF][covered] != 0xDEADBEEF).any() == (min(metallic) < 1.0)      # (diffuse paths where there are some)
    finally:
        o.close()


# R11G11B10_FLOAT as the oracle packs it (oracle/orc_formats.h f32_to_ufloat): round to nearest even on a 6-bit (red, green) or 5-bit
# (blue) mantissa; below 2^-14 the format is denormal with the fixed step 2^(-14 - mbits); above MAX it saturates.  So for 0 <= x <= MAX
#     |Q(x) - x| <= EPS x + DELTA,     EPS = 2^-(mbits + 1) (half an ulp, relative to the binade's lower end),  DELTA = 2^(-15 - mbits).
_MBITS = np.array([6, 6, 5])
_EPS = 2.0 ** -(_MBITS + 1.0)
_DELTA = 2.0 ** (-15.0 - _MBITS)
_MAX = (2.0 - 2.0 ** -_MBITS) * 2.0 ** 15


@pytest.mark.parametrize("samples", [2, 4, 8])
@pytest.mark.parametrize("mesh,metallic,vndf,depth", [("bunny.obj", (1.0, 1.0), False, 1), ("bunny.obj", (0.25, 0.5), False, 1), ("bunny.obj", (0.25, 0.5), True, 1),
                                                      ("dragon.obj", (0.25, 0.5), False, 2)], ids=["bunny-metal", "bunny-diffuse", "bunny-vndf", "dragon-depth2"])
def test_the_samples_are_those_of_n_one_sample_frames(built, samples, mesh, metallic, vndf, depth):
    """The header's consequence: frame F at N takes the samples of the one-sample frames with the indices F N .. F N + N - 1.  The word at N,
    unpacked, against the mean of those N frames' unpacked words, at EVERY covered pixel, per channel.

    The bound, from the packing's rounding rule above.  With v_k >= 0 the samples' fp32 values and M their exact mean: the one-sample words
    give m = mean Q(v_k) with |m - M| <= EPS M + DELTA; the word at N is w = Q(M'), M' the fp32 sum in order scaled exactly by 1 / N,
    M' = M (1 + t), |t| <= (N - 1) 2^-24 (non-negative terms: every partial sum's rounding is at most 2^-24 of the final sum);
    |w - M'| <= EPS M' + DELTA.  Together |w - m| <= (2 EPS + (1 + EPS) t) M + 2 DELTA, and M <= (m + DELTA) / (1 - EPS) turns that into a
    bound on what the test can see: two roundings of the channel's mantissa plus the denormal floor.  It holds below saturation, which the
    test asserts of every word it compares."""
    N, W, H = samples, 160, 90
    o = RS.Oracle(W, H, depth=depth, samples=N, entry="spp")
    try:
        HS.scene(o, mesh, W, H, metallic, vndf, frame=2)
        F = HS.frame_index(o)
        assert 0 < F < 256
        covered = o.buffer(O.BUF_VISIBILITY) != 0
        assert covered.sum() > 1000
        HS.poison(o)
        rays_n = o.ray_trace()
        words = {b: o.buffer(b) for b in (O.BUF_RT_REFL, O.BUF_RT_DIFF)}
        diffuse = covered & (words[O.BUF_RT_DIFF] != 0xDEADBEEF)
        assert diffuse.any() == (min(metallic) < 1.0)
        total = {b: np.zeros((H, W, 3), np.float64) for b in words}
        rays_1 = 0
        o.set_samples_per_pixel(1)
        for k in range(N):
            HS.set_frame_index(o, F * N + k)
            HS.poison(o)
            rays_1 += o.ray_trace()
            for b in words:
                total[b] += O.unpack_r11g11b10f(o.buffer(b)).astype(np.float64)
        assert rays_n == rays_1 > 0
        t = (N - 1) * 2.0 ** -24
        worst = 0.0
        for b, mask in ((O.BUF_RT_REFL, covered), (O.BUF_RT_DIFF, diffuse)):
            w = O.unpack_r11g11b10f(words[b]).astype(np.float64)[mask]
            m = (total[b] / N)[mask]
            assert np.isfinite(w).all() and (w < _MAX).all() and (m < _MAX).all(), "a saturated word: the bound does not apply"
            M = (m + _DELTA) / (1.0 - _EPS)
            bound = (2.0 * _EPS + (1.0 + _EPS) * t) * M + 2.0 * _DELTA
            err = np.abs(w - m)
            rel = (err / np.maximum(m, 1e-30))[m > 1e-3]
            worst = max(worst, float(rel.max()) if rel.size else 0.0)
            bad = err > bound
            assert not bad.any(), "buffer %d: %d of %d values beyond the bound, worst %.3g against %.3g" % (b, bad.sum(), bad.size, (err - bound).max(), bound[np.unravel_index((err - bound).argmax(), err.shape)])
        print("N = %d %s: largest relative difference (values above 1e-3) %.4f" % (N, mesh, worst))
    finally:
        o.close()


@pytest.mark.parametrize("mesh,metallic,vndf,depth", [("bunny.obj", (1.0, 1.0), False, 1), ("bunny.obj", (0.25, 0.5), False, 1), ("bunny.obj", (0.25, 0.5), True, 1),
                                                      ("dragon.obj", (0.25, 0.5), False, 2)], ids=["bunny-metal", "bunny-diffuse", "bunny-vndf", "dragon-depth2"])
def test_averaging_reduces_the_error(built, mesh, metallic, vndf, depth):
    """Covered pixels of a 160x90 frame, the fp32 results before packing, against a 64-sample mean from the same routine: the mean squared
    error at N = 8 is below HALF that at N = 1, for the reflection and for the diffuse image.  Independent samples would give 1/9 (both the
    estimate and the reference carry variance: (1/8 + 1/64) / (1 + 1/64)); one half guards against "all samples equal" and "not averaged",
    it is not a quality figure."""
    W, H = 160, 90
    o = RS.Oracle(W, H, depth=depth, entry="spp")
    try:
        HS.scene(o, mesh, W, H, metallic, vndf, frame=1)
        covered = o.buffer(O.BUF_VISIBILITY) != 0
        _, ref_r, ref_d = o.ray_trace_f32(64)
        _, r1, d1 = o.ray_trace_f32(1)
        _, r8, d8 = o.ray_trace_f32(8)
        images = [("reflection", ref_r, r1, r8, covered)]
        diffuse = covered & np.isfinite(ref_d).all(axis=-1)
        if min(metallic) < 1.0:
            assert diffuse.sum() > 1000
            images.append(("diffuse", ref_d, d1, d8, diffuse))
        for name, ref, a1, a8, mask in images:
            ref64 = ref[mask].astype(np.float64)
            mse1 = ((a1[mask].astype(np.float64) - ref64) ** 2).mean()
            mse8 = ((a8[mask].astype(np.float64) - ref64) ** 2).mean()
            print("%s %s: MSE(8) / MSE(1) = %.3f" % (mesh, name, mse8 / mse1))
            assert mse1 > 0.0 and mse8 < 0.5 * mse1, "%s: MSE %.4g at N = 8, %.4g at N = 1" % (name, mse8, mse1)
    finally:
        o.close()


@pytest.mark.parametrize("metallic,depth", [((1.0, 1.0), 1), ((0.25, 0.5), 1), ((0.25, 0.5), 2)], ids=["metal", "diffuse", "diffuse-depth2"])
def test_ray_counts_scale_with_the_samples(built, metallic, depth):
    """N rays(1) 0.95 <= rays(N) <= N x covered pixels x rays per pixel and sample (one per image that is traced and level)."""
    W, H = 160, 90
    o = RS.Oracle(W, H, depth=depth, entry="spp")
    try:
        HS.scene(o, "bunny.obj", W, H, metallic, False, frame=1)
        covered = int((o.buffer(O.BUF_VISIBILITY) != 0).sum())
        per_pixel = (2 if min(metallic) < 1.0 else 1) * depth
        rays = {}
        for n in (1, 2, 4, 8):
            o.set_samples_per_pixel(n)
            rays[n] = o.ray_trace()
            print("N = %d: %d rays, x%.3f" % (n, rays[n], rays[n] / rays[1]))
            assert n * rays[1] * 0.95 <= rays[n] <= n * covered * per_pixel, (n, rays, covered)
    finally:
        o.close()
