"""The exact rasteriser model (tests/raster_ref.py) and its cases (tests/raster_cases.py), proven on the CPU: no GPU needed.

  * every case keeps its own conditions -- every vertex robust (the contract's fp32 chain, separate and fused, and the exact chain snap to the
    same integers and give the same fp32 z), the clipped polygons have the vertex counts they were built for, the overflow case's winners are
    spread over the index range, the watertight meshes cover every pixel exactly once, sloped triangles lie alone, the planned candidate count
    sits on every lane, the known answers hold;
  * the CPU oracle's render_visibility equals the model: visibility words on every pixel, depth codes on every pixel the model does not flag
    as ambiguous, within one code on the flagged ones, and the flagged share stays within its cap (1 % of a case's covered pixels) -- so the
    reference alone stays inside every condition tests/test_gpu_raster_synthetic.py imposes on the kernels;
  * a few answers of the model worked out by hand.

The whole file takes about 20 s on one core; the two cases with more than 65536 triangles take about half of it.
"""
from fractions import Fraction as Fr

import numpy as np
import pytest

import raster_cases as RC
import raster_ref as R

NAMES = RC.names()
case = RC.case


@pytest.mark.parametrize("name", NAMES)
def test_case_conditions(name):
    c = case(name)
    vertices, clipped = RC.check_robust(c)              # (raises where the fp32 chains and the exact one disagree, or the count of clipped triangles is not the case's)
    assert vertices + clipped > 0 and clipped == c.clipped and (clipped > 0 or not name.startswith("6-"))
    m = RC.check(c)
    assert m.covered.any() or name.startswith("1-"), "%s draws nothing" % name
    assert int(m.ambiguous.sum()) <= RC.AMBIGUOUS_CAP * int(m.covered.sum())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_model(built, name):
    c = case(name)
    vis, depth = RC.oracle_frame(c)
    RC.compare(name, vis, depth, c.model(), (0, c.H))


def test_a_vertex_that_is_not_robust_is_refused():
    c = RC.Case("tie", 97, 61)
    for k in range(64):                                                      # half units at a frame size that is no power of two: some of them snap either way
        c.tri(0, (1000.5 + 37 * k, 1000, 0.5), (3000, 1000.5 + 11 * k, 0.5), (1000, 3000, 0.5))
    c.filler()
    with pytest.raises(AssertionError, match="not robust"):
        RC.check_robust(c)
    # 32 x 16: x = 2^-13 - 2^-26 is 2^-14 of a sub-pixel unit below the tie 4096.5, but x + 1 rounds to 1 + 2^-13 in fp32, onto the tie
    x = np.float32(2.0 ** -13 - 2.0 ** -26)
    c = RC.Case("unclipped", 32, 16)
    c.raw(0, (x, 0.5, 0.5), (0.5, 0.0, 0.5), (x, -0.5, 0.5))
    c.filler()
    with pytest.raises(AssertionError, match="not robust"):
        RC.check_robust(c)
    # ... and the same vertex kept by the guard-band clipper: the clipped triangle is refused as a whole
    c = RC.Case("clipped", 32, 16)
    c.raw(0, (x, 0.5, 0.5), (512.0, 0.0, 0.5), (x, -0.5, 0.5))
    c.filler()
    c.clipped = 1
    assert c.model().polygons[0] == {0: 4}
    with pytest.raises(AssertionError, match="not robust"):
        RC.check_robust(c)
    # a case that states the wrong number of clipped triangles is refused too
    c = RC.Case("count", 32, 16)
    c.raw(0, (0.0, 0.5, 0.5), (512.0, 0.0, 0.5), (0.0, -0.5, 0.5))
    c.filler()
    with pytest.raises(AssertionError, match="clipped triangles"):
        RC.check_robust(c)


def _render(W, H, tris, inst=1):
    c = RC.Case("hand", W, H)
    for t in tris:
        c.raw(inst, *t)
    return c.filler().model()


def test_model_known_answers():
    # the quad of test_oracle_known_answers.py::test_rasteriser_fill_rules: [4, 12) x [4, 12) on 16 x 16, right and bottom edges excluded
    q = lambda x, y, z=0.5: ((x / 8.0) - 1.0, 1.0 - (y / 8.0), z)
    tris = [[q(4, 4), q(12, 4), q(12, 12)], [q(4, 4), q(12, 12), q(4, 12)]]
    m = _render(16, 16, tris)
    quad = np.zeros((16, 16), bool); quad[4:12, 4:12] = True
    cov = m.vis >= 0x01000001
    assert (cov == quad).all() and set(np.unique(m.vis[quad])) == {0x01000001, 0x01000002} and (m.count[quad] == 1).all()
    assert (m.vis[4:12, 4:12][np.triu_indices(8)] == 0x01000001).all()            # the diagonal's centres belong to the upper right triangle (its left edge)
    assert (m.depth[quad] == int(0.5 * 16777215.0 + 0.5)).all() and (m.depth[~quad & (m.vis == 0)] == 0xFFFFFF).all()
    # counter-clockwise: culled
    assert not (_render(16, 16, [[q(4, 4), q(12, 12), q(12, 4)]]).vis >= 0x01000001).any()
    # a tie keeps the lower word, a nearer fragment wins
    m = _render(16, 16, [tris[0], tris[0]])
    assert set(np.unique(m.vis[m.vis >= 0x01000001])) == {0x01000001}
    m = _render(16, 16, [tris[0], [q(4, 4, 0.25), q(12, 4, 0.25), q(12, 12, 0.25)], tris[0]])
    assert set(np.unique(m.vis[m.vis >= 0x01000001])) == {0x01000002}
    # z = 1 has the cleared code and a word above the cleared one: not drawn; the last code below it is
    m = _render(16, 16, [[q(4, 4, 1.0), q(12, 4, 1.0), q(12, 12, 1.0)]])
    assert not (m.vis >= 0x01000001).any() and (m.depth[4:12, 4:12] == 0xFFFFFF).all() and m.count[4, 11] == 1
    m = _render(16, 16, [[q(4, 4, 1.0 - 2.0 ** -24), q(12, 4, 1.0 - 2.0 ** -24), q(12, 12, 1.0 - 2.0 ** -24)]])
    assert m.vis[4, 11] == 0x01000001 and m.depth[4, 11] == 0xFFFFFE
    assert not _render(16, 16, [[q(4, 4, 1.5), q(12, 4, 1.5), q(12, 12, 1.5)]]).count[4:12, 4:12].any()
    # a sloped triangle whose z is 1/2 on a pixel centre: the code sits on a tie, and only there is it flagged
    m = _render(16, 16, [[q(4.5, 4, 0.25), q(12.5, 4, 0.75), q(4.5, 12, 0.25)]])
    assert m.ambiguous[4, 8] and m.depth[4, 8] == 0x800000 and m.ambiguous.sum() == m.covered[:, 8].sum() - (m.vis[:, 8] == 1).sum()
    assert R.round_f32(Fr(1, 3)) == Fr(11184811, 2 ** 25) and R.round_f32(Fr(3, 2) + Fr(1, 2 ** 24)) == Fr(3, 2)
