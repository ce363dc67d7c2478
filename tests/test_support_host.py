"""The tests' own support modules without a GPU (tests/gpu_support.py, tests/restatement.py): the comparison that every twin test rests on
fails when it should, the buffer groups are what the modules have always compared, and the one restatement Oracle reaches the three C
entry points."""
import numpy as np
import pytest

import gpu_support as G
import restatement as RS


def test_assert_same_fails_on_one_word_and_on_a_missing_key():
    a = {"refl": np.arange(12, dtype=np.uint32).reshape(3, 4), "rays": np.array([7])}
    b = {k: v.copy() for k, v in a.items()}
    G.assert_same(a, b, "equal")
    b["refl"][2, 3] ^= 1
    with pytest.raises(AssertionError, match="refl differs"):
        G.assert_same(a, b, "one word")
    b["refl"][2, 3] ^= 1
    del b["rays"]
    for x, y in ((a, b), (b, a)):
        with pytest.raises(AssertionError, match="rays"):
            G.assert_same(x, y, "a missing key")


def test_buffer_groups_are_the_ones_the_modules_compare():
    assert G.GBUFFER_MIN == ("vis", "normal", "rm")
    assert G.GBUFFER == ("vis", "depth", "normal", "rm", "velocity")
    assert G.RAW == ("refl", "diff")
    assert G.DENOISED == ("flt_rfl", "flt_dff", "tss0", "tss1", "back")
    assert G.RAYS == ("rays",)
    # each module's own selection (its constants, not helpers of it)
    import test_gpu_accumulation, test_gpu_ray_rate, test_gpu_recursion, test_gpu_sampleset, test_gpu_score, test_gpu_spp
    assert test_gpu_ray_rate.IMAGES == G.RAW + G.DENOISED
    for m in (test_gpu_recursion, test_gpu_spp):
        assert m.FRAME_WORDS == G.GBUFFER_MIN + G.RAW and m.IMAGES == G.GBUFFER_MIN + G.RAW + G.DENOISED
    assert test_gpu_sampleset.FRAME_WORDS == G.GBUFFER + G.RAW + G.RAYS and test_gpu_sampleset.IMAGES == G.GBUFFER + G.RAW + G.DENOISED + G.RAYS
    for m in (test_gpu_accumulation, test_gpu_score):
        assert m.IMAGES == G.GBUFFER + G.RAW + G.DENOISED + G.RAYS
    assert set(G.GBUFFER + G.RAW + G.DENOISED) == set(G._IMAGE_IDS)


@pytest.mark.parametrize("entry,symbol,arguments", [("depth", "orc_ray_trace_depth", [3]), ("spp", "orc_ray_trace_spp", [3, 4]),
                                                    ("sampleset", "orc_ray_trace_sampleset", [3, 4, 1024])], ids=["depth", "spp", "sampleset"])
def test_the_restatement_oracle_reaches_the_three_entry_points(entry, symbol, arguments):
    o = RS.Oracle(8, 8, depth=3, samples=4, sample_set=1024, entry=entry)
    try:
        fn, args = o.ray_trace_function()
        assert fn is getattr(RS.lib(), symbol) and fn.__name__ == symbol
        assert [a.value for a in args] == arguments
        assert o.L is RS.lib() and o.ray_trace_oracle.__func__ is RS.Oracle.ray_trace_depth1_oracle
    finally:
        o.close()
    with pytest.raises(KeyError):
        RS.Oracle(8, 8, entry="none")
