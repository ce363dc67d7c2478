"""1, 2, 4 and 8 samples per pixel (rtggx_set_samples_per_pixel; DESIGN.md "Samples per pixel") on the eight workloads -- bunny and dragon,
1920x1080 and 3840x2160, the default metallic (1 1: reflection paths only) and 0.25 0.5 (a diffuse path per pixel as well): free-running
frames after a warm-up, every setting alive in the same process and measured in alternation, `--rounds` times.  Prints one JSON line per
(workload, N, round): ms/frame, rays per frame (all samples), rays per sample, Mrays/s, and the placement key of the last frame.
    python tools/probes/spp_probe.py [--frames 256] [--warmup 64] [--rounds 3] [--only bunny-1080] [--samples 1 2 4 8] [--force-small -1|0|1] [--sampleset 256]
With --samples N and --rounds 1 it is the workload of a `rocprofv3 --kernel-trace --stats` run of one setting."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import assets
from raytracedggx_amd import app

WORKLOADS = [(m, w, h, met) for m in ("bunny", "dragon") for (w, h) in ((1920, 1080), (3840, 2160)) for met in (None, (0.25, 0.5))]


def name(m, w, h, met):
    return "%s-%d%s" % (m, h, "" if met is None else "-m%g-%g" % met)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--only", nargs="*", default=None, help="workload names (bunny-1080, dragon-2160-m0.25-0.5, ...)")
    ap.add_argument("--force-small", type=int, default=-1, help="rtggx_debug_placement: -1 by the ray count, 0 / 1 the full-size / small-launch placement")
    ap.add_argument("--sampleset", type=int, default=256, help="-sampleset M of every context (rtggx_set_sample_set)")
    a = ap.parse_args()
    for m, w, h, met in WORKLOADS:
        label = name(m, w, h, met)
        if a.only and label not in a.only:
            continue
        apps = {}
        for n in a.samples:
            args = ["-mesh", assets.path(m + ".obj"), "-env", assets.path("rnl_cross.dds"), "-width", w, "-height", h, "-spp", n]
            if met is not None:
                args += ["-metallic", met[0], met[1]]
            if a.sampleset != 256:
                args += ["-sampleset", a.sampleset]
            apps[n] = app.RayTracedGGX(args)
            apps[n].context.placement(a.force_small)
        for x in apps.values():
            for _ in range(a.warmup):
                x.OnUpdate(); x.OnRender()
            x.context.sync()
        for rnd in range(a.rounds):
            for n, x in apps.items():
                c = x.context
                for _ in range(16):
                    x.OnUpdate(); x.OnRender()
                c.sync(); c.ray_total(reset=True)
                t0 = time.perf_counter()
                for _ in range(a.frames):
                    x.OnUpdate(); x.OnRender()
                c.sync()
                dt = time.perf_counter() - t0
                rays = c.ray_total()
                key, where = c.placement(a.force_small)
                print(json.dumps({"workload": label, "samples": n, "round": rnd, "frames": a.frames, "ms_per_frame": round(dt / a.frames * 1e3, 4),
                                  "rays_per_frame": rays // a.frames, "rays_per_sample": rays // a.frames // n, "mrays_per_s": round(rays / dt / 1e6, 1), "small": key["small"],
                                  "force_small": a.force_small, "sample_set": a.sampleset}), flush=True)
        for x in apps.values():
            x.OnDestroy()


if __name__ == "__main__":
    main()
