"""Scoring against a reference on the GPU (rtggx_set_reference, rtggx_set_scoring, rtggx_read_scores, -reference / -score; include/rtggx.h,
DESIGN.md "Scoring against a reference").  Its parity status: no counterpart in the reference; every record is pinned bit for bit -- nine
float64 sums and the counts -- to the numpy restatement (tests/score_ref.py) fed the device's own words of the same frame, which the rest
of the suite pins to the oracle.  The small frame is 100x54: P = 5400 is no power of two and no multiple of a chunk, a wave or a lane's run."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import assets
import gpu_support as G
import score_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = G.GBUFFER + G.RAW + G.DENOISED + G.RAYS


def _words(a):
    """The frame just rendered: (TemporalSSOut[parity], RayTracingOut0, RayTracingOut1, visibility); synchronises."""
    from raytracedggx_amd import capi
    c = a.context
    return c.readback(capi.BUF_TSS0 + c.frame_parity()), c.readback(capi.BUF_RT_REFL), c.readback(capi.BUF_RT_DIFF), c.readback(capi.BUF_VISIBILITY)


def _assert_record(got, words, metallic, reference, label, rows=(0, None)):
    want = SR.score(words[0], words[1], words[2], words[3], metallic, reference, rows[0], rows[1])
    bad = SR.same_record(got, want)
    assert not bad, "%s: %s differ: device %r, restatement %r" % (label, bad, {k: got[k] for k in bad}, {k: want[k] for k in bad})
    return want


_REFERENCES = {}


def _reference(W, H, metallic, mesh="bunny.obj", frames=32):
    """The reference of a scene, once per module: another context, -spp 8, `frames` frames accumulated and presented (RTGGX_BUF_CONVERGED)."""
    from raytracedggx_amd import capi
    key = (W, H, metallic, mesh, frames)
    if key not in _REFERENCES:
        x = G.app(W, H, ["-metallic", metallic[0], metallic[1], "-spp", 8], mesh=mesh)
        try:
            x.context.set_accumulation(True)
            for _ in range(frames):
                G.frame(x)
            x.context.present_accumulation()
            ref = x.context.readback(capi.BUF_CONVERGED)
        finally:
            x.OnDestroy()
        assert SR.unpack_rgba16f(ref).any() and np.isfinite(SR.unpack_rgba16f(ref)).all()
        ref.setflags(write=False)
        _REFERENCES[key] = ref
    return _REFERENCES[key]


# ---- 1. restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,metallic,extra", [
    ("bunny.obj", (1.0, 1.0), []), ("bunny.obj", (0.25, 0.5), []), ("bunny.obj", (1.0, 0.75), []),
    ("bunny.obj", (0.25, 0.5), ["-vndf"]), ("bunny.obj", (0.25, 0.5), ["-spp", 4, "-recursion", 2]), ("bunny.obj", (0.25, 0.5), ["-rayrate", 4]),
    ("bunny.obj", (0.25, 0.5), ["-sampleset", 4096]), ("dragon.obj", (0.25, 0.5), [])],
    ids=["metal", "diffuse", "metal-ground", "vndf", "spp4-depth2", "rayrate4", "sampleset4096", "dragon"])
def test_records_equal_the_restatement(built, mesh, metallic, extra):
    """100x54, 6 consecutive frames: every record against the restatement, bit for bit."""
    ref = _reference(100, 54, metallic, mesh)
    a = G.app(100, 54, ["-metallic", metallic[0], metallic[1]] + extra, mesh=mesh)
    try:
        c = a.context
        c.set_reference(ref)
        c.set_scoring(True)
        assert c.read_scores() == []
        for f in range(6):
            G.frame(a)
            words = _words(a)
            recs = c.read_scores()
            assert len(recs) == 1 and recs[0]["index"] == f and recs[0]["frame_index"] == G.frame_index(a), recs
            want = _assert_record(recs[0], words, metallic, ref, "%s %s frame %d" % (mesh, extra, f))
            assert want["pixels"] == 5400 and 0 < want["covered"] < 5400
            assert want["se_out_rgb"] > 0.0 and want["se_raw_rgb"] > 0.0 and want["ref_rgb2"] > want["ref_rgb2_cov"] > 0.0 and want["se_out_luma"] > 0.0
        assert c.read_scores() == []
    finally:
        a.OnDestroy()


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------------------
def test_one_pixel_and_a_strip_of_one_row(built):
    """P = 1: no addition at all in the contract's tree, ten levels of +0.0 padding on the device.  P = 100: one row of a 100x54 frame."""
    from raytracedggx_amd import capi
    a = G.app(1, 1)
    try:
        ref = np.array([[np.array([0.5, 0.25, 2.0, 1.0], np.float16).view(np.uint64)[0]]], np.uint64)
        a.context.set_reference(ref); a.context.set_scoring(True)
        for f in range(3):
            G.frame(a)
            words = _words(a)
            recs = a.context.read_scores()
            assert len(recs) == 1 and recs[0]["pixels"] == 1
            _assert_record(recs[0], words, (1.0, 1.0), ref, "1x1 frame %d" % f)
    finally:
        a.OnDestroy()
    metallic = (0.25, 0.5)
    ref = _reference(100, 54, metallic)
    a = G.app(100, 54, ["-metallic", metallic[0], metallic[1]])
    try:
        a.context.set_strip(30, 31)
        a.context.set_reference(ref); a.context.set_scoring(True)
        for f in range(3):
            G.frame(a)
            words = _words(a)
            recs = a.context.read_scores()
            assert len(recs) == 1 and recs[0]["pixels"] == 100
            want = _assert_record(recs[0], words, metallic, ref, "one row, frame %d" % f, rows=(30, 31))
            assert want["covered"] > 0 and want["se_out_rgb"] > 0.0
    finally:
        a.OnDestroy()


def test_a_frame_with_more_chunks_than_the_second_stage_has_lanes(built):
    """The launch shape built (score.hip): stage 1 reduces chunks of 1024 pixels, on at most two workgroups per CU -- 512 on an MI355X --
    which then loop over chunks; stage 2 is one workgroup of 1024 lanes.  1280 x 820 = 1 049 600 pixels are 1025 chunks: more than stage 1
    has workgroups (the grid loops), more than stage 2 has lanes (its loops over the partials and the counts go round more than once),
    and one more than a power of two: the partials are padded from 1025 to 2048, and the last chunk is a full one."""
    metallic = (0.25, 0.5)
    W, H = 1280, 820
    ref = _reference(W, H, metallic, frames=2)
    a = G.app(W, H, ["-metallic", metallic[0], metallic[1]])
    try:
        a.context.set_reference(ref); a.context.set_scoring(True)
        G.frame(a)
        words = _words(a)
        recs = a.context.read_scores()
        assert len(recs) == 1 and recs[0]["pixels"] == W * H == 1025 * 1024
        want = _assert_record(recs[0], words, metallic, ref, "1280x820")
        assert want["covered"] > 10000 and want["se_out_rgb"] > 0.0
    finally:
        a.OnDestroy()


def test_three_strips_score_their_own_rows(built):
    metallic = (0.25, 0.5)
    W, H = 320, 180
    ref = _reference(W, H, metallic, frames=8)
    strips = [(0, 60), (60, 120), (120, 180)]
    apps = [G.app(W, H, ["-metallic", metallic[0], metallic[1]]) for _ in strips]
    try:
        for a, (b, e) in zip(apps, strips):
            a.context.set_strip(b, e); a.context.set_reference(ref); a.context.set_scoring(True)
        for f in range(3):
            pixels = covered = 0
            for a, (b, e) in zip(apps, strips):
                G.frame(a)
                words = _words(a)
                recs = a.context.read_scores()
                assert len(recs) == 1 and recs[0]["index"] == f
                want = _assert_record(recs[0], words, metallic, ref, "rows [%d, %d) frame %d" % (b, e, f), rows=(b, e))
                pixels += want["pixels"]; covered += want["covered"]
            assert pixels == W * H and covered > 1000
    finally:
        for a in apps:
            a.OnDestroy()


# ---- 3. scoring changes nothing else --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["small-placement", "full-size-placement", "sync-flag", "caller-stream", "deforming"])
def test_a_scoring_context_renders_what_its_twin_renders(built, variant):
    """100x54, 6 frames: a scoring context against a twin that never called any of the four functions -- every buffer from the G-buffer and
    the raw images through the back buffer, and the ray count, after every frame.  The twin keeps the library's choice of fusing the tone
    map (small launches: fused); the scoring context never fuses."""
    import torch
    metallic = (0.25, 0.5)
    extra = ["-metallic", metallic[0], metallic[1]] + (["-sync"] if variant == "sync-flag" else []) + (["-deform", 0.05] if variant == "deforming" else [])
    ref = _reference(100, 54, metallic)
    a, twin = G.app(100, 54, extra), G.app(100, 54, extra)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()] if variant == "caller-stream" else None
    try:
        for k, x in enumerate((a, twin)):
            if variant == "small-placement":
                x.context.placement(1)
            if variant == "full-size-placement":
                x.context.placement(0)
            if streams is not None:
                x.context.set_stream(streams[k].cuda_stream)
        a.context.set_reference(ref); a.context.set_scoring(True)
        for f in range(6):
            G.frame(a); G.frame(twin)
            ia = G.images(a, IMAGES)
            G.assert_same(ia, G.images(twin, IMAGES), "%s, frame %d" % (variant, f))
            recs = a.context.read_scores()
            assert len(recs) == 1
            _assert_record(recs[0], _words(a), metallic, ref, "%s, frame %d" % (variant, f))
        if variant == "small-placement":
            assert a.context.placement(1)[1]["shade"] == "B", "small launches shade on the traversal's stream"
        if variant == "full-size-placement":
            assert a.context.placement(0)[1]["shade"] == "main"
        if variant == "deforming":
            assert a.context.placement()[0]["deforming"]
        if streams is not None:
            a.context.set_stream(0); twin.context.set_stream(0)
    finally:
        a.OnDestroy(); twin.OnDestroy()


# ---- 4. free-running ------------------------------------------------------------------------------------------------------------------
def test_free_running_frames_score_what_synchronised_ones_do(built):
    metallic = (1.0, 0.5)
    extra = ["-metallic", metallic[0], metallic[1]]
    ref = _reference(100, 54, metallic)
    a, twin = G.app(100, 54, extra), G.app(100, 54, extra)
    try:
        for x in (a, twin):
            x.context.set_reference(ref); x.context.set_scoring(True)
        want = []
        for f in range(16):
            G.frame(twin)
            words = _words(twin)
            recs = twin.context.read_scores()
            assert len(recs) == 1
            _assert_record(recs[0], words, metallic, ref, "synchronised twin, frame %d" % f)
            want += recs
        for f in range(16):
            G.frame(a)
        got = a.context.read_scores()
        assert [r["index"] for r in got] == list(range(16))
        for f, (g, w) in enumerate(zip(got, want)):
            assert g["frame_index"] == w["frame_index"] and not SR.same_record(g, w), "frame %d: %r vs %r" % (f, g, w)
    finally:
        a.OnDestroy(); twin.OnDestroy()


# ---- 5. the ring ------------------------------------------------------------------------------------------------------------------------
def test_the_ring_keeps_the_last_records_and_hands_them_out_in_order(built):
    from raytracedggx_amd import capi
    metallic = (1.0, 1.0)
    ref = _reference(100, 54, metallic)
    a = G.app(100, 54)
    try:
        c = a.context
        c.set_reference(ref); c.set_scoring(True)
        n = capi.SCORE_RING + 5
        frame_indices = []
        for f in range(n):
            G.frame(a)
            frame_indices.append(G.frame_index(a))
        words = _words(a)
        recs = c.read_scores()
        assert [r["index"] for r in recs] == list(range(5, n)), "the five oldest are gone, and the gap in index shows it"
        assert [r["frame_index"] for r in recs] == frame_indices[5:]
        _assert_record(recs[-1], words, metallic, ref, "the last of %d frames" % n)
        assert c.read_scores() == []
        for f in range(7):
            G.frame(a)
        words = _words(a)
        first = c.read_scores(capacity=3)
        assert [r["index"] for r in first] == [n, n + 1, n + 2], "the three oldest"
        rest = c.read_scores()
        assert [r["index"] for r in rest] == [n + 3, n + 4, n + 5, n + 6], "the next read continues"
        _assert_record(rest[-1], words, metallic, ref, "after the partial read")
    finally:
        a.OnDestroy()


# ---- 6. the reference -------------------------------------------------------------------------------------------------------------------
def test_a_frames_own_image_as_the_reference_scores_zero(built):
    """Two contexts render the same frames.  The twin's TemporalSSOut of frame 4 is the other's reference for ITS frame 4: se_out_* are +0.0."""
    metallic = (0.25, 0.5)
    extra = ["-metallic", metallic[0], metallic[1]]
    a, twin = G.app(100, 54, extra), G.app(100, 54, extra)
    try:
        for f in range(4):
            G.frame(a); G.frame(twin)
        G.frame(twin)
        own = _words(twin)[0]
        a.context.set_reference(own); a.context.set_scoring(True)
        G.frame(a)
        words = _words(a)
        np.testing.assert_array_equal(words[0], own)
        rec = a.context.read_scores()[0]
        _assert_record(rec, words, metallic, own, "own image")
        assert rec["se_out_rgb"] == 0.0 and rec["se_out_luma"] == 0.0 and rec["se_out_rgb_cov"] == 0.0 and rec["skipped_out"] == 0
        assert rec["se_raw_rgb"] > 0.0 and rec["ref_rgb2"] > 0.0
    finally:
        a.OnDestroy(); twin.OnDestroy()


def test_the_reference_can_be_replaced_in_mid_run(built):
    metallic = (0.25, 0.5)
    ref1 = _reference(100, 54, metallic)
    ref2 = _reference(100, 54, (1.0, 1.0))
    assert (ref1 != ref2).any()
    a = G.app(100, 54, ["-metallic", metallic[0], metallic[1]])
    try:
        c = a.context
        c.set_reference(ref1); c.set_scoring(True)
        for f in range(4):
            if f == 2:
                c.set_reference(ref2)      # no read in between: the two records before it were computed against ref1
            G.frame(a)
            if f >= 2:
                words = _words(a)
                recs = c.read_scores()
                assert [r["index"] for r in recs] == ([0, 1, 2] if f == 2 else [3])
                _assert_record(recs[-1], words, metallic, ref2, "second reference, frame %d" % f)
                if f == 2:
                    assert recs[0]["ref_rgb2"] == recs[1]["ref_rgb2"] == SR.tree_sum(SR.terms(*words, metallic, ref1)[0]["ref_rgb2"]) != recs[2]["ref_rgb2"]
    finally:
        a.OnDestroy()


def test_reference_from_accumulation_is_the_presented_mean_and_leaves_the_back_buffer(built):
    from raytracedggx_amd import capi
    metallic = (0.25, 0.5)
    extra = ["-metallic", metallic[0], metallic[1]]
    a, twin = G.app(100, 54, extra), G.app(100, 54, extra)
    try:
        for x in (a, twin):
            x.context.set_accumulation(True)
            for f in range(4):
                G.frame(x)
            x.context.set_accumulation(False)
        before = G.images(a, IMAGES)
        a.context.reference_from_accumulation()
        G.assert_same(G.images(a, IMAGES), before, "reference_from_accumulation")
        assert not a.context.readback(capi.BUF_CONVERGED).any(), "RTGGX_BUF_CONVERGED is the present's"
        twin.context.present_accumulation()
        conv = twin.context.readback(capi.BUF_CONVERGED)
        twin.context.set_reference(conv)
        for x in (a, twin):
            x.context.set_scoring(True)
        for f in range(2):
            G.frame(a); G.frame(twin)
            words = _words(a)
            ra, rt = a.context.read_scores(), twin.context.read_scores()
            assert len(ra) == len(rt) == 1 and not SR.same_record(ra[0], rt[0]), (ra, rt)
            _assert_record(ra[0], words, metallic, conv, "reference from the accumulation, frame %d" % f)
    finally:
        a.OnDestroy(); twin.OnDestroy()


# ---- 7. non-finite input ----------------------------------------------------------------------------------------------------------------
def test_non_finite_pixels_are_skipped_and_counted(built):
    """An environment of +infinity: the sky and every reflection that misses are infinite in the raw image and, after the denoiser, not
    finite in TemporalSSOut.  Two pixels of the reference are made non-finite as well.  Counts as the restatement's, every sum finite."""
    from raytracedggx_amd import capi
    ref = _reference(100, 54, (1.0, 1.0), mesh="triangle.obj", frames=8).copy()
    ref16 = ref.view(np.uint16).reshape(54, 100, 4)
    ref16[27, 50, 1] = 0x7C00; ref16[5, 5, 2] = 0x7E00      # +infinity under the model's row, a NaN in the sky
    a = G.app(100, 54, mesh="triangle.obj")
    try:
        a.context.set_env(capi.FORMAT_RGBA16F, 1, 1, assets.constant_env_rgba16f(np.inf))
        a.context.set_reference(ref); a.context.set_scoring(True)
        for f in range(3):
            G.frame(a)
            words = _words(a)
            rec = a.context.read_scores()[0]
            want = _assert_record(rec, words, (1.0, 1.0), ref, "infinite environment, frame %d" % f)
            assert rec["skipped_out"] >= 2 and rec["skipped_raw"] > 2 and rec["skipped_raw"] >= (words[3] == 0).sum()
            assert all(np.isfinite(rec[k]) for k in SR.SUMS)
            assert rec["pixels"] == 5400 and rec["covered"] == (words[3] != 0).sum() > 0
    finally:
        a.OnDestroy()


# ---- 8. control and refusals ------------------------------------------------------------------------------------------------------------
def test_off_and_on_refusals_and_release(built):
    from raytracedggx_amd import capi
    metallic = (0.25, 0.5)
    extra = ["-metallic", metallic[0], metallic[1]]
    ref = _reference(100, 54, metallic)
    a, twin = G.app(100, 54, extra), G.app(100, 54, extra)
    try:
        c = a.context
        L = c.L
        count = C.c_uint32(77)
        # before anything exists
        with pytest.raises(capi.RtggxError, match="rtggx_set_scoring"):
            c.set_scoring(True)
        with pytest.raises(capi.RtggxError, match="rtggx_set_scoring"):
            a.set_scoring(True)
        with pytest.raises(capi.RtggxError, match="rtggx_reference_from_accumulation"):
            c.reference_from_accumulation()
        for bad in (np.zeros((54, 99), np.uint64), np.zeros((54, 100, 2), np.uint64), np.zeros(1, np.uint64)):
            with pytest.raises(capi.RtggxError, match="rtggx_set_reference"):
                c.set_reference(bad)
        assert L.rtggx_set_reference(c.h, None, 43200) == -1 and b"rtggx_set_reference" in L.rtggx_last_error()
        assert c.read_scores() == []
        c.set_scoring(False)      # off without a reference: nothing to refuse
        G.frame(a); G.frame(twin)
        G.assert_same(G.images(a, IMAGES), G.images(twin, IMAGES), "after the refusals")
        # on, off for two frames, on again: index goes on counting, frame_index shows the frames in between
        c.set_reference(ref); c.set_scoring(True)
        shown = []
        for f in range(6):
            if f == 2:
                c.set_scoring(False)
            if f == 4:
                c.set_scoring(True)
            G.frame(a); G.frame(twin)
            shown.append(G.frame_index(a))
        words = _words(a)
        buf = (capi.Score * 8)()
        assert L.rtggx_read_scores(c.h, buf, 8, None) == -1 and b"rtggx_read_scores" in L.rtggx_last_error()
        assert L.rtggx_read_scores(c.h, None, 8, C.byref(count)) == -1 and count.value == 77
        recs = c.read_scores()      # the refused reads took nothing
        assert [r["index"] for r in recs] == [0, 1, 2, 3]
        assert [r["frame_index"] for r in recs] == [shown[0], shown[1], shown[4], shown[5]]
        _assert_record(recs[-1], words, metallic, ref, "on again")
        with pytest.raises(capi.RtggxError, match="rtggx_set_reference"):
            c.set_reference(np.zeros((10, 10), np.uint64))      # a refused replacement keeps the reference
        G.frame(a); G.frame(twin)
        words = _words(a)
        recs = c.read_scores()
        assert [r["index"] for r in recs] == [4]
        _assert_record(recs[0], words, metallic, ref, "after a refused replacement")
        # releasing the reference turns scoring off
        c.set_reference(None)
        for f in range(2):
            G.frame(a); G.frame(twin)
        assert c.read_scores() == []
        with pytest.raises(capi.RtggxError, match="rtggx_set_scoring"):
            c.set_scoring(True)
        G.assert_same(G.images(a, IMAGES), G.images(twin, IMAGES), "after the release")
        c.set_reference(ref); c.set_scoring(True)
        G.frame(a); G.frame(twin)
        assert [r["index"] for r in c.read_scores()] == [5]
    finally:
        a.OnDestroy(); twin.OnDestroy()


# ---- 9. the executable -------------------------------------------------------------------------------------------------------------------
def test_executable_saves_a_reference_and_scores_a_run_against_it(built, tmp_path):
    """RayTracedGGX -accumulate 8 -savereference ref.pfm, then -reference ref.pfm -score scores.jsonl: the PFM against RTGGX_BUF_CONVERGED of
    the same run driven from Python, the JSON lines against the restatement's figures of the same frames."""
    from raytracedggx_amd import app, capi
    exe = os.path.join(ROOT, "raytracedggx_amd", "RayTracedGGX")
    metallic = (0.25, 0.5)
    scene = ["-mesh", assets.path("bunny.obj"), "-env", assets.path("rnl_cross.dds"), "-width", "100", "-height", "54", "-metallic", "0.25", "0.5"]
    pfm, jsonl = str(tmp_path / "ref.pfm"), str(tmp_path / "scores.jsonl")
    r = subprocess.run([exe] + scene + ["-spp", "8", "-frames", "8", "-accumulate", "8", "-savereference", pfm, "-dump", str(tmp_path / "shot.png")],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0 and "wrote " + pfm in r.stdout, (r.stdout, r.stderr)
    x = G.app(100, 54, ["-metallic", 0.25, 0.5, "-spp", 8, "-accumulate", 8])
    try:
        for f in range(8):
            G.frame(x)
        x.context.present_accumulation()
        conv = x.context.readback(capi.BUF_CONVERGED)
        assert x.save_reference(str(tmp_path / "again.pfm"))
    finally:
        x.OnDestroy()
    ref16 = app.read_pfm(pfm, 100, 54)
    ref = np.ascontiguousarray(ref16).view(np.uint64)[..., 0]
    np.testing.assert_array_equal(ref, conv, err_msg="the PFM against RTGGX_BUF_CONVERGED")
    assert open(pfm, "rb").read() == open(str(tmp_path / "again.pfm"), "rb").read()
    r = subprocess.run([exe] + scene + ["-frames", "6", "-reference", pfm, "-score", jsonl], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = [json.loads(l) for l in open(jsonl)]
    assert [l["index"] for l in lines] == list(range(6))
    a = G.app(100, 54, ["-metallic", 0.25, 0.5, "-reference", pfm, "-score", str(tmp_path / "python.jsonl")])
    try:
        for f, line in enumerate(lines):
            G.frame(a)
            words = _words(a)
            want = SR.score(*words, metallic, ref)
            fig = SR.figures(want)
            assert line["frame_index"] == G.frame_index(a)
            for k in ("pixels", "covered", "skipped_out", "skipped_raw"):
                assert line[k] == want[k], (f, k)
            for k, v in fig.items():
                assert v is not None and line[k] == v, "frame %d %s: %r in the file, %r restated" % (f, k, line[k], v)
        assert a.flush_scores()
        recs = a.read_scores()
        assert recs == [], "the flush took them"
    finally:
        a.OnDestroy()
    assert [json.loads(l) for l in open(str(tmp_path / "python.jsonl"))] == lines
