"""The float64 models of the environment path (tests/env_ref.py) against the CPU oracle (oracle/orc_raytrace.h environment, transform_sh)
on the synthetic cubes, directions and levels of tests/env_cases.py, and against answers known without either.  No GPU.

The oracle's sampler and the HIP kernel's are one text written twice; the model is written from the definitions (D3D face selection,
taps at texel centres, seamless edges).  Where the three agree, a face sign, a seam step or a mip weight copied wrong would have had to be
invented a third time, in another form.

Sampler: lo - B <= oracle <= hi + B in every channel of every direction, with B counted from the fp32 roundings of the evaluation
(env_cases.bound) and [lo, hi] the model's interval, which is a point except where a corner tap takes part (env_ref.py).  So that the
interval cannot hide a failure, the test asserts how often it IS a point: on every level of side 5 or more, for at least 80 % of the
random directions; and that the corner taps are exercised: at least 100 directions per case.

SH: |oracle - model| <= 2^-23 magnitude, magnitude being the same sum over absolute values.  Known answers: the constant cube gives
L00 = sqrt(4 pi) and nothing else; a cube holding basis function Y_k gives the k-th unit vector up to the discretisation error of the
64 x 64 midpoint rule, which the model reports by refinement (the rule's error falls with the square of the texel size, so the 64-cube's
error is 4/3 of its distance to the 128-cube's result to leading order; twice that is allowed)."""
import numpy as np
import pytest

import env_cases as EC
import env_ref as R
from oracle import oracle as O

CUBES = EC.all_cubes()


def oracle_with(cube):
    o = O.Oracle(8, 8, threads=1)
    o.set_env_rgba16f(cube.size, cube.mips, cube.mip_major())
    return o


def check_interval(got, lo, hi, B, label):
    got = got.astype(np.float64)
    B = np.broadcast_to(np.asarray(B, np.float64).reshape(-1, 1), got.shape)
    excess = np.maximum(lo - got, got - hi)
    i = np.unravel_index(np.argmax(excess / B), got.shape)
    print("%s: largest distance outside the interval %.3f B (direction %d); where the interval is a point, largest |value - model| %.3f B"
          % (label, max(excess[i] / B[i], 0.0), i[0], (np.abs(got - lo) / B)[(lo == hi)].max() if (lo == hi).any() else 0.0))
    assert (excess <= B).all(), "%s: direction %d channel %d: %.9g outside [%.9g, %.9g] by %.3g, B = %.3g" % (
        label, i[0], i[1], got[i], lo[i], hi[i], excess[i], B[i])
    return float(max(excess[i] / B[i], 0.0))


@pytest.mark.parametrize("cube", CUBES, ids=lambda c: c.name)
def test_sampler_model_against_the_oracle(cube):
    D, lv = EC.directions(cube.size), EC.levels_for(cube.mips)
    o = oracle_with(cube)
    try:
        got = EC.oracle_environment(o, D.d, lv)
        lo, hi, corner = R.environment(cube.levels, cube.size, D.d, lv, with_corner=True)
        assert ((lo == hi).all(axis=1) | corner).all()                    # a point wherever no corner tap takes part
        assert corner.sum() >= 100, "%s: only %d corner-tap directions" % (cube.name, corner.sum())
        check_interval(got, lo, hi, EC.bound(cube, lv), cube.name + " mixed levels")
        # every integer level by itself
        rnd = D.part("random")
        for m in range(cube.mips):
            got = EC.oracle_environment(o, D.d, float(m))
            lo, hi, corner = R.environment(cube.levels, cube.size, D.d, float(m), with_corner=True)
            check_interval(got, lo, hi, EC.bound(cube, float(m)), "%s level %d" % (cube.name, m))
            if EC.side(cube.size, m) >= 5:
                point = (lo == hi).all(axis=1)
                share = point[rnd].mean()
                print("%s level %d (side %d): the interval is a point for %.1f %% of the random directions, %.1f %% of all; %d corner-tap directions"
                      % (cube.name, m, EC.side(cube.size, m), 100 * share, 100 * point.mean(), corner.sum()))
                assert share >= 0.8
                assert corner.sum() >= 100
    finally:
        o.close()


def test_sampler_model_known_answers():
    """Independent of the oracle: a constant cube gives the constant in every direction and at every level; a texel-centre direction gives
    that texel (no neighbour has any weight); the midpoint of two texels' centres gives their mean -- across a cube edge too, where the
    neighbour is the texel the seam rule picks, named here by hand: on the edge between +x and +z (x = z > 0) the last column of +z meets the
    first column of +x, rows aligned."""
    const = [np.full((6, s, s, 3), 2.5) for s in (4, 2, 1)]
    D = EC.directions(4)
    lo, hi = R.environment(const, 4, D.d, EC.levels_for(3))
    assert np.allclose(lo, 2.5, rtol=1e-15) and np.allclose(hi, 2.5, rtol=1e-15)
    cube = EC.random_cube(5, 3)
    d, f, y, x = R.texel_centre_dirs(5)
    lo, hi = R.environment(cube.levels, 5, d, 0.0)
    assert np.allclose(lo, cube.levels[0][f, y, x], rtol=1e-13, atol=0.0) and np.array_equal(lo, hi)
    # +z face (4): u = d.x / d.z grows with x, v = -d.y / d.z; +x face (0): u = -d.z / d.x, so its column 0 is where z is largest
    L = cube.levels[0]
    for row in range(5):
        v = (row + 0.5) / 5 * 2.0 - 1.0
        on_edge = np.array([[1.0, -v, 1.0]])          # u = 1 on +z; ties go to x: sampled as u = -1 on +x.  Half a texel from both centres.
        lo, hi = R.environment(cube.levels, 5, on_edge, 0.0)
        want = 0.5 * (L[4, row, 4] + L[0, row, 0])
        assert np.allclose(lo, want, rtol=1e-13) and np.allclose(hi, want, rtol=1e-13), row
    # the axis convention of the faces: the centre of each face looks along its axis
    d, f, y, x = R.texel_centre_dirs(1)
    assert np.array_equal(d, np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float))
    assert np.array_equal(R.face_uv(d)[0], np.arange(6))


def oracle_sh(cube):
    o = oracle_with(cube)
    try:
        o.transform_sh()
        return o.buffer(O.BUF_SH_COEFFS).astype(np.float64).reshape(9, 3)
    finally:
        o.close()


@pytest.mark.parametrize("size", EC.SH_SIZES + (5, 12))
def test_sh_model_against_the_oracle(size):
    cube = EC.sh_cube(size)
    c, mag = R.sh_project(cube.levels[0], size)
    got = oracle_sh(cube)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("sh %d: largest |oracle - model| / (2^-23 magnitude) = %.3f" % (size, np.nanmax(np.where(mag > 0, np.abs(got - c) / (EC.SH_BOUND * mag), 0.0))))
    assert (np.abs(got - c) <= EC.SH_BOUND * mag).all()


def test_sh_known_answers():
    for size in (1, 2, 7, 64):
        c, mag = R.sh_project(np.ones((6, size, size, 3)), size)
        want = np.zeros((9, 3)); want[0] = np.sqrt(4.0 * np.pi)
        assert np.abs(c - want).max() <= 1e-13 * mag.max(), size
    for k in range(9):
        c, disc = EC.basis_answer(k)
        want = np.zeros((9, 3)); want[k] = 1.0
        assert disc.max() < 5e-3                       # (1 / 32)^2 texels: a wrong sign or a swapped axis is an error of 1 or 2
        assert (np.abs(c - want) <= disc).all(), "Y_%d: %s" % (k, np.abs(c - want).max(axis=1))
