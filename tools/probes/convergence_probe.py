"""What the estimators estimate: every ray budget of the renderer against a converged reference (rtggx_set_accumulation; DESIGN.md
"Progressive accumulation").  Bunny 640x360, still model and camera (-dt 0).  The reference: -spp 8 accumulated over 256 frames and
presented (RTGGX_BUF_CONVERGED), at recursion depth 1 and, for the depth-2 row, at depth 2.  Then 32 frames of each of rate 1 with the NDF
sampler, rate 1 with the VNDF sampler, rate 4, -spp 2 / 4 / 8 and rate 1 at depth 2: the relative L2 distance of TemporalSSOut's rgb (what
the denoiser shows) and of the last frame's raw image (RayTracingOut0 + RayTracingOut1 where a diffuse path wrote it) from the reference.
One JSON line per row.  --sampleset M (rtggx_set_sample_set; DESIGN.md "Sample-set size") gives the reference a sample set of M members:
at the default 256 its -spp 8 x 256 frames are 2048 draws from the same 256 points, with M = 65536 and --reference-frames 4096 it is the
ground truth the section asks for.  --rows-sampleset M gives the rows' contexts a set of their own (default: 256, the renderer as shipped).
--curve (rtggx_set_scoring; DESIGN.md "Scoring against a reference") hands the reference to every row's context (set_reference), turns scoring
on and prints, behind each row's line, one more: the figures of EVERY frame of the row, from one read_scores at its end -- no wait per frame.
    python tools/probes/convergence_probe.py [--frames 32] [--reference-frames 256] [--sampleset 256] [--rows-sampleset 256] [--metallic 0.25 0.5] [--curve] [--out rows.jsonl]"""
import argparse, json, math, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import accum_ref as AR
import assets
from raytracedggx_amd import app, capi

W, H = 640, 360
ROWS = [("rate1-ndf", 1, []), ("rate1-vndf", 1, ["-vndf"]), ("rate4", 1, ["-rayrate", 4]), ("spp2", 1, ["-spp", 2]), ("spp4", 1, ["-spp", 4]),
        ("spp8", 1, ["-spp", 8]), ("rate1-ndf-depth2", 2, ["-recursion", 2])]


def rgb16(words):
    return np.ascontiguousarray(words).view(np.float16).reshape(words.shape + (4,))[..., :3].astype(np.float64)


def rel_l2(x, ref):
    return float(np.sqrt(((x - ref) ** 2).sum() / max((ref ** 2).sum(), 1e-300)))


def make(extra, metallic):
    args = ["-mesh", assets.path("bunny.obj"), "-env", assets.path("rnl_cross.dds"), "-width", W, "-height", H, "-dt", 0] + list(extra)
    if metallic:
        args += ["-metallic", metallic[0], metallic[1]]
    return app.RayTracedGGX(args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reference-frames", type=int, default=256)
    ap.add_argument("--metallic", type=float, nargs=2, default=None)
    ap.add_argument("--sampleset", type=int, default=256, help="-sampleset M of the reference")
    ap.add_argument("--rows-sampleset", type=int, default=256, help="-sampleset M of the rows")
    ap.add_argument("--curve", action="store_true", help="score every frame on the device and print the rows' curves as well (at most %d frames)" % capi.SCORE_RING)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    met = tuple(a.metallic) if a.metallic else (1.0, 1.0)
    if a.curve and a.frames > capi.SCORE_RING:
        ap.error("--curve reads the ring once at the end: at most %d frames" % capi.SCORE_RING)
    reference, reference_words = {}, {}
    for depth in sorted({d for _, d, _ in ROWS}):
        x = make(["-spp", 8, "-recursion", depth] + (["-sampleset", a.sampleset] if a.sampleset != 256 else []), a.metallic)
        x.context.set_accumulation(True)
        for _ in range(a.reference_frames):
            x.OnUpdate(); x.OnRender()
        x.context.present_accumulation()
        reference_words[depth] = x.context.readback(capi.BUF_CONVERGED)
        reference[depth] = rgb16(reference_words[depth])
        assert x.context.accumulated_frames() == a.reference_frames
        x.OnDestroy()
    out = open(a.out, "w") if a.out else None
    for label, depth, extra in ROWS:
        x = make(extra + (["-sampleset", a.rows_sampleset] if a.rows_sampleset != 256 else []), a.metallic)
        c = x.context
        if a.curve:
            c.set_reference(reference_words[depth]); c.set_scoring(True)
        for _ in range(a.frames):
            x.OnUpdate(); x.OnRender()
        tss = rgb16(c.readback(capi.BUF_TSS0 + c.frame_parity()))
        raw = AR.unpack_r11g11b10f(c.readback(capi.BUF_RT_REFL)).astype(np.float64)
        mask = AR.diffuse_mask(c.readback(capi.BUF_VISIBILITY), met)
        raw += np.where(mask[..., None], AR.unpack_r11g11b10f(c.readback(capi.BUF_RT_DIFF)).astype(np.float64), 0.0)
        row = {"estimator": label, "depth": depth, "frames": a.frames, "reference": "spp8 x %d frames, depth %d, sample set %d" % (a.reference_frames, depth, a.sampleset), "sample_set": a.rows_sampleset,
               "metallic": list(met), "rel_l2_temporal_ss_out": round(rel_l2(tss, reference[depth]), 5), "rel_l2_raw_frame": round(rel_l2(raw, reference[depth]), 5)}
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
        if a.curve:
            recs = c.read_scores()
            rel = lambda r, se, ref2: round(math.sqrt(r[se] / r[ref2]), 5) if r[ref2] > 0.0 else None
            curve = {"estimator": label, "depth": depth, "curve_frames": [r["index"] for r in recs],
                     "rel_l2_temporal_ss_out": [rel(r, "se_out_rgb", "ref_rgb2") for r in recs], "rel_l2_raw_frame": [rel(r, "se_raw_rgb", "ref_rgb2") for r in recs],
                     "rel_l2_temporal_ss_out_covered": [rel(r, "se_out_rgb_cov", "ref_rgb2_cov") for r in recs],
                     "rel_l2_temporal_ss_out_luma": [rel(r, "se_out_luma", "ref_luma2") for r in recs], "skipped": [r["skipped_out"] + r["skipped_raw"] for r in recs]}
            line = json.dumps(curve)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
        x.OnDestroy()
    if out:
        out.close()


if __name__ == "__main__":
    main()
