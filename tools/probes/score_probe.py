"""Scoring on against off, and against scoring by readback (rtggx_set_scoring; DESIGN.md "Scoring against a reference"), on the bunny at
1920x1080 -- all metal and metallic 0.25 0.5 -- and at 3840x2160: free-running frames after a warm-up, the settings alive in the same process
and measured in alternation, `--rounds` times, as tools/probes/accum_probe.py does.
    off        a context that never heard of scoring
    on         scoring on; the ring is read once per round, behind the timed frames' synchronise
    readback   what tools/probes/convergence_probe.py did for its one frame, done for every frame: TemporalSSOut, both raw images and
               the visibility words read back (24 bytes per pixel, a synchronise per frame) and one relative L2 of each image in numpy
The reference is the mean of a few accumulated -spp 8 frames of the same scene: what it holds does not matter for the time.  Prints one
JSON line per (workload, setting, round): ms/frame and, for `on`, the records read and the last one's rel_l2_out.
    python tools/probes/score_probe.py [--frames 256] [--warmup 64] [--rounds 3] [--only bunny-1080] [--settings off on readback] [--readback-frames 32]
With --settings on and --rounds 1 it is the workload of a `rocprofv3 --kernel-trace --stats` run (the two scoring kernels' own time)."""
import argparse, json, math, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import accum_ref as AR
import assets
from raytracedggx_amd import app, capi

WORKLOADS = [("bunny", 1920, 1080, None), ("bunny", 1920, 1080, (0.25, 0.5)), ("bunny", 3840, 2160, None)]


def name(m, w, h, met):
    return "%s-%d%s" % (m, h, "" if met is None else "-m%g-%g" % met)


def rgb16(words):
    return np.ascontiguousarray(words).view(np.float16).reshape(words.shape + (4,))[..., :3].astype(np.float64)


def rel_l2(x, ref):
    return float(np.sqrt(((x - ref) ** 2).sum() / max((ref ** 2).sum(), 1e-300)))


def make(m, w, h, met, extra=()):
    args = ["-mesh", assets.path(m + ".obj"), "-env", assets.path("rnl_cross.dds"), "-width", w, "-height", h] + list(extra)
    if met is not None:
        args += ["-metallic", met[0], met[1]]
    return app.RayTracedGGX(args)


def score_by_readback(x, met, ref):
    c = x.context
    tss = rgb16(c.readback(capi.BUF_TSS0 + c.frame_parity()))
    raw = AR.unpack_r11g11b10f(c.readback(capi.BUF_RT_REFL)).astype(np.float64)
    mask = AR.diffuse_mask(c.readback(capi.BUF_VISIBILITY), met)
    raw += np.where(mask[..., None], AR.unpack_r11g11b10f(c.readback(capi.BUF_RT_DIFF)).astype(np.float64), 0.0)
    return rel_l2(tss, ref), rel_l2(raw, ref)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settings", nargs="+", default=["off", "on", "readback"], choices=["off", "on", "readback"])
    ap.add_argument("--readback-frames", type=int, default=32, help="timed frames of the readback leg per round (a frame of it takes a thousand times the others')")
    ap.add_argument("--only", nargs="*", default=None, help="workload names (bunny-1080, bunny-1080-m0.25-0.5, bunny-2160)")
    a = ap.parse_args()
    for m, w, h, met in WORKLOADS:
        label = name(m, w, h, met)
        if a.only and label not in a.only:
            continue
        r = make(m, w, h, met, ["-spp", 8])
        r.context.set_accumulation(True)
        for _ in range(8):
            r.OnUpdate(); r.OnRender()
        r.context.present_accumulation()
        reference = r.context.readback(capi.BUF_CONVERGED)
        r.OnDestroy()
        ref64 = rgb16(reference)
        metallic = met or (1.0, 1.0)
        apps = {s: make(m, w, h, met) for s in a.settings}
        if "on" in apps:
            apps["on"].context.set_reference(reference); apps["on"].context.set_scoring(True)
        for x in apps.values():
            for _ in range(a.warmup):
                x.OnUpdate(); x.OnRender()
            x.context.sync()
        if "on" in apps:
            apps["on"].context.read_scores()
        for rnd in range(a.rounds):
            for s, x in apps.items():
                c = x.context
                for _ in range(16):
                    x.OnUpdate(); x.OnRender()
                c.sync()
                if s == "on":
                    c.read_scores()
                frames = a.readback_frames if s == "readback" else a.frames
                row = {"workload": label, "setting": s, "round": rnd, "frames": frames}
                t0 = time.perf_counter()
                for _ in range(frames):
                    x.OnUpdate(); x.OnRender()
                    if s == "readback":
                        row["rel_l2_out"], row["rel_l2_raw"] = score_by_readback(x, metallic, ref64)
                c.sync()
                dt = time.perf_counter() - t0
                if s == "on":
                    t1 = time.perf_counter()
                    recs = c.read_scores()
                    row["read_scores_ms"] = round((time.perf_counter() - t1) * 1e3, 4)
                    row["records"] = len(recs)
                    row["rel_l2_out"] = math.sqrt(recs[-1]["se_out_rgb"] / recs[-1]["ref_rgb2"])
                    row["rel_l2_raw"] = math.sqrt(recs[-1]["se_raw_rgb"] / recs[-1]["ref_rgb2"])
                row["ms_per_frame"] = round(dt / frames * 1e3, 4)
                print(json.dumps(row), flush=True)
        for x in apps.values():
            x.OnDestroy()


if __name__ == "__main__":
    main()
