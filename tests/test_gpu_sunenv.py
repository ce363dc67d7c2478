"""The sun from the environment on the GPU (rtggx_sun_from_env; sunenv.hip sunPeakKernel, sunSumsKernel, sunRemoveKernel and their finishing
kernels): the record against the restatement (tests/sunenv_ref.py) on the synthetic cubes of tests/sunenv_cases.py -- peak, counts and flags
bit for bit, every fp64 sum equal to the model's (the summation bound, tightened: sunenv_ref.py), direction, irradiance and the whole cube
after the removal bit for bit once the model is given the reported background --, the context left alone where nothing is removed, the
refusals, the loop through rtggx_set_sun on the bunny against a twin that is handed the restated cube, and the -sunfromenv flag against
-sun."""
import numpy as np
import pytest

import env_cases as EC
import envimage_ref as E
import gpu_support as G
import sunenv_cases as SC
import sunenv_ref as SR

pytestmark = pytest.mark.gpu

CASES = SC.gpu_cases()
BY_NAME = {c.name: c for c in CASES}
W, H = 148, 84      # the sun-hit tests' frame: ragged right and bottom edges
METAL_ARGS = ["-metallic", "0.25", "0.75"]
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS
SCALARS = ("peak_luma", "peak_face", "peak_x", "peak_y", "texels_cone", "texels_ring", "texels_lit", "found", "removed")


@pytest.fixture(scope="module")
def ctx(built):
    from raytracedggx_amd import capi
    c = capi.Context(32, 32)
    yield c
    c.close()


def set_level0(ctx, case):
    from raytracedggx_amd import capi
    ctx.set_env(capi.FORMAT_RGBA16F, case.S, 1, case.codes.reshape(-1))


def ulps(a, b):
    return abs(a - b) / np.spacing(abs(b))


def check_record(rec, codes, args, label, remove=False):
    """A device record against the restatement; returns the model that was given the record's cos2 and background (what the cube and the
    float results are restated with)."""
    own = SR.estimate(codes, remove=remove, **args)
    for k in ("cos2_cone", "cos2_ring"):
        assert ulps(rec[k], own[k]) <= 4.0, "%s: %s %r, numpy %r" % (label, k, rec[k], own[k])
    cosines = SR.estimate(codes, remove=remove, given={"cos2_cone": rec["cos2_cone"], "cos2_ring": rec["cos2_ring"]}, **args)
    for k in SCALARS:
        assert rec[k] == cosines[k], "%s: %s is %r, restated %r" % (label, k, rec[k], cosines[k])
    half = np.spacing(np.maximum(cosines["background_half"], np.float32(2.0 ** -14)).astype(np.float16)).astype(np.float64)
    assert (np.abs(rec["background_half"].astype(np.float64) - cosines["background_half"].astype(np.float64)) <= half).all(), "%s: background_half %s, restated %s" % (
        label, rec["background_half"], cosines["background_half"])
    model = SR.estimate(codes, remove=remove, given=rec, **args)
    worst = 0.0
    for k in SR.SUMS:
        if k not in model["magnitude"]:      # (no pass C: the sums are 0 on both sides)
            assert not np.any(rec[k]) and not np.any(model[k]), "%s: %s" % (label, k)
            continue
        diff, room = np.abs(np.asarray(rec[k]) - np.asarray(model[k])), SR.DEVICE_BOUND * np.asarray(model["magnitude"][k])
        print("%s: %s differs by %s of a bound of %s" % (label, k, diff, room))
        assert np.all(diff <= room), "%s: %s is %r, restated %r, bound %r" % (label, k, rec[k], model[k], room)
        worst = max(worst, float(np.max(diff)))
    print("%s: largest difference of a sum %g" % (label, worst))
    assert rec["mean_luma"] == model["mean_luma"] and np.array_equal(rec["background"], model["background"]), label      # (quotients of equal sums)
    for k in ("direction", "irradiance"):
        same = (rec[k].view(np.uint32) == model[k].view(np.uint32)) | ((rec[k] == 0) & (model[k] == 0))      # (a moment component that sums to zero may carry either sign: the header says so)
        assert same.all(), "%s: %s is %s, restated %s" % (label, k, rec[k], model[k])
    return model


def non_degenerate(case):
    """The cases that are meant to have a cone and a ring worth the name: the placed suns at 20 / 40 degrees, and the corner at S = 64 with the
    default angles (69 and 416 texels; the centre there has 19 and 126 under the mask rule, one short of the bar, and is compared all the same)."""
    return case.faces is not None and case.S in (16, 37) or case.name == "S64_face5_corner"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_record_equals_the_restatement_and_the_context_stays_untouched(ctx, case):
    """remove = 0.  Peak, counts and flags bit for bit; cos2 within 4 ulp of numpy's and then taken over; every sum within the bound in
    force (sunenv_ref.DEVICE_BOUND: equal values, tightened from 64 x 2^-53 x sum |terms| after every measured difference was zero);
    background_half within one binary16 ulp, and with it given to the model direction and irradiance bit for bit.  The second call returns
    the same bytes, and RTGGX_BUF_ENV is what it was."""
    from raytracedggx_amd import capi
    set_level0(ctx, case)
    before = ctx.readback(capi.BUF_ENV)
    rec = ctx.sun_from_env(**case.args)
    model = check_record(rec, case.codes, case.args, case.name)
    if non_degenerate(case):
        faces = len(set((np.nonzero(model["cone_mask"])[0] // (case.S * case.S)).tolist()))
        assert rec["texels_cone"] >= 20 and rec["texels_ring"] >= 100 and faces == case.faces and rec["found"] == 1, (case.name, rec["texels_cone"], rec["texels_ring"], faces)
    again = ctx.sun_from_env(**case.args)
    assert again["bytes"] == rec["bytes"] and len(rec["bytes"]) == 224
    assert np.array_equal(ctx.readback(capi.BUF_ENV), before) and ctx.buffer_size(capi.BUF_ENV) == 8 * 6 * case.S * case.S


def garbage_levels(case, seed=3):
    """The case's level 0 with a chain of random levels below it: what the removal must throw away."""
    rng = np.random.default_rng(seed)
    codes = [case.codes]
    for s in E.chain_sides(case.S)[1:]:
        t = rng.uniform(0.0, 50.0, (6, s, s, 4)).astype(np.float16)
        t[..., 3] = 1.0
        codes.append(t.view(np.uint16).copy())
    return EC.Cube(case.S, len(codes), codes, case.name)


@pytest.mark.parametrize("case", [c for c in CASES if c.name not in ("constant", "black")], ids=lambda c: c.name)
def test_the_removal_leaves_the_restated_cube(ctx, case):
    """remove = 1 on a cube that came with other levels below level 0: the record is the remove = 0 record with removed = 1, and all of
    RTGGX_BUF_ENV -- the cut level 0 and every level of its box chain -- equals the restatement given the reported background."""
    from raytracedggx_amd import capi
    cube = garbage_levels(case)
    ctx.set_env(capi.FORMAT_RGBA16F, cube.size, cube.mips, cube.dds_order())
    rec = ctx.sun_from_env(remove=True, **case.args)
    model = check_record(rec, case.codes, case.args, case.name, remove=True)
    assert rec["removed"] == 1
    want = SR.cube_of(SR.removed_level0(case.codes, model))
    got = ctx.readback(capi.BUF_ENV)
    assert got.shape == want.shape
    n0 = 6 * case.S * case.S
    both_nan = ((got & 0x7FFF) > 0x7C00) & ((want & 0x7FFF) > 0x7C00)      # below level 0 a NaN is a NaN: IEEE leaves its payload open (the hostile cube's ring holds some)
    both_nan[:n0] = False
    bad = np.nonzero(((got != want) & ~both_nan).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d texels differ, first: texel %d = %s, restated %s" % (case.name, bad.size, got.shape[0], bad[0], got[bad[0]], want[bad[0]])
    assert (got[:n0][model["cone_mask"]] != case.codes.reshape(-1, 4)[model["cone_mask"]]).any() and np.array_equal(got[:n0][~model["cone_mask"]], case.codes.reshape(-1, 4)[~model["cone_mask"]])
    # what is left holds no sun above the background: a second call cuts nothing more out of the cone it finds
    after = ctx.sun_from_env(**case.args)
    assert after["peak_luma"] <= rec["peak_luma"]


@pytest.mark.parametrize("name", ["constant", "black"])
def test_nothing_found_leaves_the_cube_with_its_levels(ctx, name):
    from raytracedggx_amd import capi
    cube = garbage_levels(BY_NAME[name])
    ctx.set_env(capi.FORMAT_RGBA16F, cube.size, cube.mips, cube.dds_order())
    before = ctx.readback(capi.BUF_ENV)
    rec = ctx.sun_from_env(remove=True, **BY_NAME[name].args)
    check_record(rec, BY_NAME[name].codes, BY_NAME[name].args, name, remove=True)
    assert rec["found"] == 0 and rec["removed"] == 0 and not rec["direction"].any() and not rec["irradiance"].any()
    assert np.array_equal(ctx.readback(capi.BUF_ENV), before)


def test_refusals_leave_the_context_as_it_was(built):
    from raytracedggx_amd import capi
    c = capi.Context(32, 32)
    try:
        with pytest.raises(capi.RtggxError, match="no environment"):
            c.sun_from_env()
        set_level0(c, BY_NAME["S16_face0_edge"])
        before = c.readback(capi.BUF_ENV)
        for bad in (dict(cone=-1.0), dict(cone=45.5), dict(cone=float("nan")), dict(cone=20.0, ring=20.0), dict(cone=20.0, ring=10.0), dict(cone=20.0, ring=89.5),
                    dict(cone=40.0), dict(min_contrast=-1.0), dict(min_contrast=float("inf")), dict(min_contrast=float("nan"))):
            with pytest.raises(capi.RtggxError, match="rtggx_sun_from_env"):
                c.sun_from_env(remove=True, **bad)
        assert c.L.rtggx_sun_from_env(c.h, 20.0, 40.0, 0.0, 1, None) != 0 and b"null result" in c.L.rtggx_last_error()
        assert np.array_equal(c.readback(capi.BUF_ENV), before)
        check_record(c.sun_from_env(20.0, 40.0), BY_NAME["S16_face0_edge"].codes, dict(cone=20.0, ring=40.0), "after the refusals")
    finally:
        c.close()


def test_still_sky_runs_and_the_sh_state_go_on_across_a_call_that_removes_nothing(built):
    """A still camera under the stock environment: across calls with remove = 0, a refused call and a call that finds nothing to remove
    (a contrast no texel reaches) the runs of the tiles nothing is drawn in keep growing, and every image and the SH coefficients equal
    those of a twin that never calls."""
    from raytracedggx_amd import capi
    a, b = G.app(320, 180), G.app(320, 180)
    try:
        before = None
        env = a.context.readback(capi.BUF_ENV)
        for f in range(20):
            if f == 14:
                before = a.context.sky_runs()[0].copy()
                a.context.sun_from_env(20.0, 40.0, 1.0)
                assert a.context.sun_from_env(20.0, 40.0, 1e30, remove=True)["found"] == 0
                with pytest.raises(capi.RtggxError, match="rtggx_sun_from_env"):
                    a.context.sun_from_env(cone=50.0, remove=True)
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
        runs, threshold = a.context.sky_runs()
        assert (before >= threshold).any() and (runs[before >= threshold] > before[before >= threshold]).all()
        assert np.array_equal(a.context.readback(capi.BUF_ENV), env)
        assert np.array_equal(a.context.readback(capi.BUF_SH_COEFFS), b.context.readback(capi.BUF_SH_COEFFS))
    finally:
        a.OnDestroy(); b.OnDestroy()


def test_the_whole_loop_on_the_bunny_equals_a_twin_given_the_restated_cube(built):
    """set_env(cube), sun_from_env(remove), set_sun(direction, irradiance) against set_env(the restated cube, chain included) and the same
    set_sun: three frames, every buffer, the ray count, the environment and the SH coefficients."""
    from raytracedggx_amd import capi
    case = BY_NAME["S16_face2_corner"]      # (the sun stands above the scene: +Y, and lights the bunny and the ground)
    a, b = G.app(W, H, METAL_ARGS), G.app(W, H, METAL_ARGS)
    try:
        set_level0(a.context, case)
        rec = a.context.sun_from_env(remove=True, **case.args)
        model = check_record(rec, case.codes, case.args, case.name, remove=True)
        assert rec["removed"] == 1 and rec["direction"][1] > 0.5
        a.context.set_sun(rec["direction"], rec["irradiance"])
        levels = SR.chain_codes(SR.removed_level0(case.codes, model))
        cube = EC.Cube(case.S, len(levels), levels, "restated")
        b.context.set_env(capi.FORMAT_RGBA16F, cube.size, cube.mips, cube.dds_order())
        b.context.set_sun(rec["direction"], rec["irradiance"])
        dark = None
        for f in range(3):
            G.frame(a); G.frame(b)
            ia, ib = G.images(a, IMAGES), G.images(b, IMAGES)
            G.assert_same(ia, ib, "frame %d" % f)
            dark = ia
        assert np.array_equal(a.context.readback(capi.BUF_ENV), b.context.readback(capi.BUF_ENV))
        assert np.array_equal(a.context.readback(capi.BUF_SH_COEFFS).view(np.uint32), b.context.readback(capi.BUF_SH_COEFFS).view(np.uint32))
        assert dark["rays"][0] > 0 and (dark["vis"] != 0).any()
    finally:
        a.OnDestroy(); b.OnDestroy()


def cross_pfm(path, level0_codes):
    """A horizontal cross holding the cube's level 0 (exact: every half is a float), written as a .pfm file."""
    rgb = np.ascontiguousarray(level0_codes)[..., :3].copy().view(np.float16).astype(np.float32)
    S = rgb.shape[1]
    img = np.zeros((3 * S, 4 * S, 3), np.float32)
    for (r, col), (face, turned) in E.CROSS[E.HCROSS].items():
        img[r * S:(r + 1) * S, col * S:(col + 1) * S] = rgb[face]
    with open(path, "wb") as f:
        f.write(E.pfm_bytes(img))
    return str(path)


def test_the_flag_renders_what_the_sun_flag_renders_on_the_restated_cube(built, tmp_path):
    """-env <cross.pfm> -sunfromenv 20 against -env <the restated level 0 as a cross> -sun <the record's direction and irradiance>, the
    record taken through capi from the same cube and arguments (cone 20: ring 60, contrast 16): three frames, every buffer, the ray count,
    the environment and the SH coefficients.  (An image's chain is the box chain of its level 0, so the twin's cube is the removal's.)"""
    from raytracedggx_amd import capi
    case = BY_NAME["S16_face2_corner"]
    args = dict(cone=20.0)
    c = capi.Context(32, 32)
    try:
        set_level0(c, case)
        rec = c.sun_from_env(**args)
        model = check_record(rec, case.codes, args, "capi")
        assert rec["found"] == 1
    finally:
        c.close()
    sun = [repr(float(x)) for x in list(rec["direction"]) + list(rec["irradiance"])]
    a = G.app(W, H, METAL_ARGS + ["-env", cross_pfm(tmp_path / "sun.pfm", case.codes), "-sunfromenv", "20"])
    b = G.app(W, H, METAL_ARGS + ["-env", cross_pfm(tmp_path / "sunless.pfm", SR.removed_level0(case.codes, model)), "-sun"] + sun)
    try:
        want = SR.cube_of(SR.removed_level0(case.codes, model))
        assert np.array_equal(a.context.readback(capi.BUF_ENV), want) and np.array_equal(b.context.readback(capi.BUF_ENV), want)
        for f in range(3):
            G.frame(a); G.frame(b)
            G.assert_same(G.images(a, IMAGES), G.images(b, IMAGES), "frame %d" % f)
        assert np.array_equal(a.context.readback(capi.BUF_SH_COEFFS).view(np.uint32), b.context.readback(capi.BUF_SH_COEFFS).view(np.uint32))
    finally:
        a.OnDestroy(); b.OnDestroy()
