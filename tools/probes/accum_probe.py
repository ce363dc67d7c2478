"""Progressive accumulation on against off (rtggx_set_accumulation; DESIGN.md "Progressive accumulation") on the bunny at 1920x1080 and
3840x2160, the default metallic (1 1) and 0.25 0.5: free-running frames after a warm-up, both settings alive in the same process and
measured in alternation, `--rounds` times, as tools/probes/ray_rate_probe.py does.  Prints one JSON line per (workload, setting, round):
ms/frame and, for the accumulating context, the frames it has accumulated.
    python tools/probes/accum_probe.py [--frames 256] [--warmup 64] [--rounds 3] [--only bunny-1080] [--settings off on] [--sampleset 256]
With --settings on and --rounds 1 it is the workload of a `rocprofv3 --kernel-trace --stats` run (accumulateKernel's own time)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import assets
from raytracedggx_amd import app

WORKLOADS = [("bunny", w, h, met) for (w, h) in ((1920, 1080), (3840, 2160)) for met in (None, (0.25, 0.5))]


def name(m, w, h, met):
    return "%s-%d%s" % (m, h, "" if met is None else "-m%g-%g" % met)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settings", nargs="+", default=["off", "on"], choices=["off", "on"])
    ap.add_argument("--only", nargs="*", default=None, help="workload names (bunny-1080, bunny-2160-m0.25-0.5, ...)")
    ap.add_argument("--sampleset", type=int, default=256, help="-sampleset M of every context (rtggx_set_sample_set)")
    a = ap.parse_args()
    for m, w, h, met in WORKLOADS:
        label = name(m, w, h, met)
        if a.only and label not in a.only:
            continue
        apps = {}
        for s in a.settings:
            args = ["-mesh", assets.path(m + ".obj"), "-env", assets.path("rnl_cross.dds"), "-width", w, "-height", h]
            if met is not None:
                args += ["-metallic", met[0], met[1]]
            if a.sampleset != 256:
                args += ["-sampleset", a.sampleset]
            apps[s] = app.RayTracedGGX(args)
            apps[s].context.set_accumulation(s == "on")
        for x in apps.values():
            for _ in range(a.warmup):
                x.OnUpdate(); x.OnRender()
            x.context.sync()
        for rnd in range(a.rounds):
            for s, x in apps.items():
                c = x.context
                for _ in range(16):
                    x.OnUpdate(); x.OnRender()
                c.sync()
                t0 = time.perf_counter()
                for _ in range(a.frames):
                    x.OnUpdate(); x.OnRender()
                c.sync()
                dt = time.perf_counter() - t0
                print(json.dumps({"workload": label, "accumulate": s, "round": rnd, "frames": a.frames, "ms_per_frame": round(dt / a.frames * 1e3, 4),
                                  "sample_set": a.sampleset, "accumulated_frames": c.accumulated_frames()}), flush=True)
        for x in apps.values():
            x.OnDestroy()


if __name__ == "__main__":
    main()
