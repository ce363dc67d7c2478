"""The sample-set size M = 65536 against M = 256 (rtggx_set_sample_set; DESIGN.md "Sample-set size") on the bunny at 1920x1080 with the
default metallic (1 1) and 0.25 0.5 and at 3840x2160: free-running frames after a warm-up, every setting alive in the same process and
measured in alternation, `--rounds` times, as tools/probes/accum_probe.py does.  Prints one JSON line per (workload, M, round): ms/frame.
    python tools/probes/sampleset_probe.py [--frames 256] [--warmup 64] [--rounds 3] [--only bunny-1080] [--sets 256 65536]
With --sets M and --rounds 1 it is the workload of a `rocprofv3 --kernel-trace --stats` run of one setting."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import assets
from raytracedggx_amd import app

WORKLOADS = [("bunny", 1920, 1080, None), ("bunny", 1920, 1080, (0.25, 0.5)), ("bunny", 3840, 2160, None)]


def name(m, w, h, met):
    return "%s-%d%s" % (m, h, "" if met is None else "-m%g-%g" % met)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", type=int, nargs="+", default=[256, 65536])
    ap.add_argument("--only", nargs="*", default=None, help="workload names (bunny-1080, bunny-1080-m0.25-0.5, bunny-2160)")
    a = ap.parse_args()
    for m, w, h, met in WORKLOADS:
        label = name(m, w, h, met)
        if a.only and label not in a.only:
            continue
        apps = {}
        for s in a.sets:
            args = ["-mesh", assets.path(m + ".obj"), "-env", assets.path("rnl_cross.dds"), "-width", w, "-height", h]
            if met is not None:
                args += ["-metallic", met[0], met[1]]
            if s != 256:      # (the default context never calls the setter)
                args += ["-sampleset", s]
            apps[s] = app.RayTracedGGX(args)
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
                print(json.dumps({"workload": label, "sample_set": s, "round": rnd, "frames": a.frames, "ms_per_frame": round(dt / a.frames * 1e3, 4)}), flush=True)
        for x in apps.values():
            x.OnDestroy()


if __name__ == "__main__":
    main()
