"""A mapped frame (rtggx_set_sample_map; DESIGN.md "Adaptive sampling") against the uniform frames of 8 samples and of 1 on the bunny at
1920x1080 and 3840x2160, all metal and at metallic 0.25 / 0.5: the three contexts alive in the same process and measured in alternation,
`--rounds` times `--frames` free-running frames after a warm-up, as tools/probes/sampleset_probe.py does.  The map is the one the policy of
tests/adaptive_ref.py derives from 16 accumulated frames of the mapped context itself (before its warm-up), at the target whose mean count
over covered pixels is nearest `--mean-count`.  Prints one JSON line per (workload, context, round): ms per frame and rays per frame, and
one per workload with the map's histogram.
    python tools/probes/adaptive_probe.py [--frames 256] [--warmup 64] [--rounds 3] [--mean-count 3] [--only bunny-1080]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import adaptive_ref as A
import assets
from raytracedggx_amd import app, capi

WORKLOADS = [("bunny", 1920, 1080, None), ("bunny", 1920, 1080, (0.25, 0.5)), ("bunny", 3840, 2160, None), ("bunny", 3840, 2160, (0.25, 0.5))]
N = 8


def name(m, w, h, met):
    return "%s-%d%s" % (m, h, "" if met is None else "-m%g-%g" % met)


def derive_map(x, mean_count):
    """16 uniform frames accumulated, the policy's map at the target that spends `mean_count` samples per covered pixel, accumulation off again."""
    c = x.context
    c.set_accumulation(True)
    for _ in range(16):
        x.OnUpdate(); x.OnRender()
    c.sync()
    refl, diff, vis = c.readback(capi.BUF_ACC_REFL), c.readback(capi.BUF_ACC_DIFF), c.readback(capi.BUF_VISIBILITY)
    c.set_accumulation(False); c.reset_accumulation()
    v, cov = A.blocks_from_sums(refl, diff, vis, 16, N)
    spent = lambda t: float((A.counts(v, cov, t, N).astype(np.float64) * cov).sum() / max(cov.sum(), 1))
    target = min((1e-7 * 2.0 ** (k / 4.0) for k in range(100)), key=lambda t: abs(spent(t) - mean_count))
    return A.counts(v, cov, target, N), target, spent(target)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mean-count", type=float, default=3.0)
    ap.add_argument("--only", nargs="*", default=None, help="workload names (bunny-1080, bunny-1080-m0.25-0.5, bunny-2160, bunny-2160-m0.25-0.5)")
    a = ap.parse_args()
    for m, w, h, met in WORKLOADS:
        label = name(m, w, h, met)
        if a.only and label not in a.only:
            continue
        apps = {}
        for which, spp in (("uniform-8", N), ("mapped", N), ("uniform-1", 1)):
            args = ["-mesh", assets.path(m + ".obj"), "-env", assets.path("rnl_cross.dds"), "-width", w, "-height", h]
            if met is not None:
                args += ["-metallic", met[0], met[1]]
            if spp != 1:
                args += ["-spp", spp]
            apps[which] = app.RayTracedGGX(args)
        blocks, target, spent = derive_map(apps["mapped"], a.mean_count)
        apps["mapped"].context.set_sample_map(blocks)
        print(json.dumps({"workload": label, "target": target, "mean_count": round(spent, 3),
                          "blocks_at_1_2_4_8": [int((blocks == c).sum()) for c in A.COUNTS]}), flush=True)
        for x in apps.values():
            for _ in range(a.warmup):
                x.OnUpdate(); x.OnRender()
            x.context.sync()
        for rnd in range(a.rounds):
            for which, x in apps.items():
                c = x.context
                for _ in range(16):
                    x.OnUpdate(); x.OnRender()
                c.sync()
                t0 = time.perf_counter()
                for _ in range(a.frames):
                    x.OnUpdate(); x.OnRender()
                c.sync()
                dt = time.perf_counter() - t0
                print(json.dumps({"workload": label, "context": which, "round": rnd, "frames": a.frames, "ms_per_frame": round(dt / a.frames * 1e3, 4),
                                  "rays_per_frame": c.ray_count()}), flush=True)
        for x in apps.values():
            x.OnDestroy()


if __name__ == "__main__":
    main()
