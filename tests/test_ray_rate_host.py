"""Quarter-rate tracing without a GPU: the ABI surface of rtggx_set_ray_rate, the command line's refusals (before any GPU is touched),
and known answers of the reconstruction's numpy restatement (tests/ray_rate_ref.py) on synthetic G-buffers."""
import numpy as np

import host_support as HS
import ray_rate_ref as R


def test_set_ray_rate_is_declared_exported_and_bound(built):
    HS.declared_exported_bound("rtggx_set_ray_rate", r"\bint\s+rtggx_set_ray_rate\s*\(\s*rtggx_context\s*\*\s*ctx\s*,\s*uint32_t\s+pixels_per_ray\s*\)")


def test_executable_refuses_bad_ray_rates_before_touching_a_gpu(built):
    HS.executable_refuses((["-rayrate", "3"], ["-gpus", "2", "-rayrate", "4"], ["-strips", "2", "-rayrate", "4"], ["/RAYRATE", "4", "-Strips", "3"],
                           ["-rayrate", "4", "-gpus", "2"], ["-rayrate"]), "-rayrate", no_device_message="no HIP device")


def test_traced_pixels_cover_every_pixel_in_four_frames():
    seen = sum(R.traced_mask(7, 5, f).astype(int) for f in range(4))
    assert (seen == 1).all()
    assert R.traced_mask(4, 4, 0)[0, 0] and R.traced_mask(4, 4, 1)[1, 1] and R.traced_mask(4, 4, 2)[0, 1] and R.traced_mask(4, 4, 3)[1, 0]
    assert (R.traced_mask(6, 6, 256 + 1) == R.traced_mask(6, 6, 1)).all()


def test_r11g11b10_packer_round_trips_and_rounds_to_nearest_even():
    codes = np.arange(0, 1 << 11, dtype=np.uint32)
    words = codes | (codes << 11) | ((codes & 0x3FF) << 22)
    finite = (codes >> 6) < 31
    w = words[finite & ((codes & 0x3FF) >> 5 < 31)]
    np.testing.assert_array_equal(R.pack_r11g11b10f(R.unpack_r11g11b10f(w)), w)
    one = R.pack_r11g11b10f(np.array([[1.0, 1.0, 1.0]], np.float32))[0]
    tie = np.float32(1.0 + 1.0 / 128)      # halfway between 1 and 1 + 1/64: to the even code, 1
    assert R.pack_r11g11b10f(np.array([[tie, 0.0, -1.0]], np.float32))[0] == (one & 0x7FF)
    assert R.pack_r11g11b10f(np.array([[np.float32(1.0 + 3.0 / 128), 1e30, np.inf]], np.float32))[0] & 0x7FF == (one & 0x7FF) + 2


def _gbuffer(W, H, inst, normal_code=(512, 1023, 512), depth=0x800000, rough=128):
    vis = np.where(inst >= 0, (inst.astype(np.int64) << 24) + 1, 0).astype(np.uint32)
    n = normal_code[0] | (normal_code[1] << 10) | (normal_code[2] << 20) | (3 << 30)
    normal = np.full((H, W), n, np.uint32)
    return vis, np.full((H, W), depth, np.uint32), normal, np.full((H, W), rough | (0 << 8), np.uint16)


def test_flat_plane_with_constant_traced_values_reconstructs_the_constant():
    W, H = 9, 7
    vis, depth, normal, rm = _gbuffer(W, H, np.ones((H, W), np.int64))
    c_refl = R.pack_r11g11b10f(np.array([0.25, 0.5, 1.0], np.float32))
    c_diff = R.pack_r11g11b10f(np.array([3.0, 0.125, 0.75], np.float32))
    for f in range(4):
        refl, diff, target, dif = R.reconstruct(vis, depth, normal, rm, np.full((H, W), c_refl, np.uint32), np.full((H, W), c_diff, np.uint32), f)
        assert target.sum() == W * H - R.traced_mask(W, H, f).sum() and (dif == target).all()
        assert (refl == c_refl).all() and (diff == c_diff).all(), f


def test_two_instances_side_by_side_do_not_bleed():
    W, H = 12, 8
    inst = np.where(np.arange(W)[None, :] < 5, 0, 1).repeat(H, 0)
    vis, depth, normal, rm = _gbuffer(W, H, inst)
    a, b = R.pack_r11g11b10f(np.array([1.0, 0.0, 0.0], np.float32)), R.pack_r11g11b10f(np.array([0.0, 0.0, 2.0], np.float32))
    img = np.where(inst == 0, a, b).astype(np.uint32)
    for f in range(4):
        refl, diff, target, _ = R.reconstruct(vis, depth, normal, rm, img, img, f, diffuse_instances=(0,))
        np.testing.assert_array_equal(refl, img)
        np.testing.assert_array_equal(diff, img)      # instance 1 (metallic 1 here): RayTracingOut1 left as it was
        assert target[:, 4].any() and target[:, 5].any()


def test_zero_weights_take_the_fallbacks():
    W, H = 8, 8
    f = 0                                   # traced: even x, even y
    inst = np.ones((H, W), np.int64)
    inst[3:6, 3:8] = 2                      # (x 5, y 4) keeps instance 1: its distance-1 candidates (4, 4) (6, 4) are instance 2
    inst[5:8, 0:4] = -1; inst[7, 1] = 3     # (1, 7): no pixel of its instance anywhere near
    vis, depth, normal, rm = _gbuffer(W, H, inst)
    inst[4, 5] = 1; vis[4, 5] = (1 << 24) + 1
    normal[2, 3] = 512 | (0 << 10) | (512 << 20) | (3 << 30)      # (3, 2) faces away from its candidates (2, 2) (4, 2): every weight 0
    vals = np.zeros((H, W, 3), np.float32)
    vals[2, 2] = (1.0, 0.5, 0.25); vals[2, 4] = (0.5, 1.5, 0.75); vals[2, 6] = (2.0, 2.0, 2.0); vals[6, 4] = (4.0, 4.0, 4.0); vals[6, 6] = (2.0, 3.0, 4.0)
    img = R.pack_r11g11b10f(vals)
    refl, diff, target, dif = R.reconstruct(vis, depth, normal, rm, img, img, f)
    assert target[2, 3] and target[4, 5] and target[7, 1] and not dif[7, 1]
    # sum w = 0: the plain mean of the candidates
    assert refl[2, 3] == R.pack_r11g11b10f((vals[2, 2] + vals[2, 4]) / np.float64(2)) and diff[2, 3] == refl[2, 3]
    np.testing.assert_allclose(R.unpack_r11g11b10f(refl[2, 3]), [0.75, 1.0, 0.5], rtol=2 ** -6)
    # no candidate: the plain mean of the instance's traced pixels within distance 2, (4, 2) (6, 2) (4, 6) (6, 6)
    assert refl[4, 5] == R.pack_r11g11b10f((((vals[2, 4] + vals[2, 6]) + vals[6, 4]) + vals[6, 6]) / np.float64(4)) and diff[4, 5] == refl[4, 5]
    np.testing.assert_allclose(R.unpack_r11g11b10f(refl[4, 5]), [2.125, 2.625, 2.6875], rtol=2 ** -5)
    # none: 0
    assert refl[7, 1] == 0
