"""The lights at the surfaces the paths hit (rtggx_set_light_reflections; DESIGN.md "The lights in reflections"): what the toggle costs and
what it does to a converged image.  Bunny, rnl environment, -sharedmem, 1920x1080 unless told otherwise; the light sets are
tools/probes/lights_probe.py's (1: the spot B; 3: A, B, C of tests/golden/lights_classes.json; 8: those and five more).  One JSON line per record.
    python tools/probes/light_hits_probe.py cost [--counts 1 3 8] [--depths 1 2] [--pairs 4]
        per configuration (default and mixed materials, each depth, each light count) two contexts in one process, the lights alone and the
        lights with the toggle, 320 warm-up frames each, then windows of 256 frames alternating; host clock around frames that end in a
        synchronise.  ms per frame, and the shadow rays from hits (the difference of the ray counts of the last frame).
    python tools/probes/light_hits_probe.py frames [--lights N] [--depth D] [--frames 200] [--metallic a b]
        one context with the toggle, that many frames: what a `rocprofv3 --kernel-trace --stats` run of its own wraps.
    python tools/probes/light_hits_probe.py picture [--frames 1024] [--lights 3]
        mixed materials, still model, a sample set of 1024: two contexts accumulate the same frames with the lights alone (P) and with the
        toggle (T).  Relative L2 of T against P over covered pixels, and the covered pixels whose luminance the toggle raised."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import assets
from raytracedggx_amd import app, capi
from lights_probe import SETS, window


def make(w, h, metallic, depth, lights, toggle, extra=()):
    x = app.RayTracedGGX(["-mesh", assets.path("bunny.obj"), "-env", assets.path("rnl_cross.dds"), "-width", w, "-height", h, "-sharedmem"]
                         + (["-metallic", metallic[0], metallic[1]] if metallic else []) + (["-recursion", depth] if depth != 1 else []) + list(extra))
    x.set_lights(lights)
    if toggle:
        x.set_light_reflections(1)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["cost", "frames", "picture"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--metallic", type=float, nargs=2, default=None)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 3, 8])
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--lights", type=int, default=3)
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--frames", type=int, default=None)
    a = ap.parse_args()
    if a.mode == "cost":
        for met in (None, (0.25, 0.75)):
            for depth in a.depths:
                for n in a.counts:
                    apps = {"lights": make(a.width, a.height, met, depth, SETS[n], False), "toggle": make(a.width, a.height, met, depth, SETS[n], True)}
                    for x in apps.values():
                        window(x, 320)
                    ms = {k: [] for k in apps}
                    for _ in range(a.pairs):
                        for k, x in apps.items():
                            ms[k].append(round(window(x, 256), 4))
                    rays = {k: x.context.ray_count() for k, x in apps.items()}
                    print(json.dumps({"config": "%dx%d %s depth %d, %d lights" % (a.width, a.height, "default materials" if met is None else "-metallic %g %g" % met, depth, n),
                                      "ms": ms, "cost_ms": round(sum(ms["toggle"]) / a.pairs - sum(ms["lights"]) / a.pairs, 4), "rays": rays,
                                      "shadow_rays_from_hits": rays["toggle"] - rays["lights"]}), flush=True)
                    for x in apps.values():
                        x.OnDestroy()
    elif a.mode == "frames":
        frames = a.frames or 200
        x = make(a.width, a.height, a.metallic, a.depth, SETS[a.lights], True)
        window(x, frames)
        print(json.dumps({"lights": a.lights, "depth": a.depth, "metallic": a.metallic, "frames": frames, "rays": x.context.ray_count()}), flush=True)
        x.OnDestroy()
    else:
        frames = a.frames or 1024
        met = a.metallic or (0.25, 0.75)
        still = ["-dt", 0, "-sampleset", 1024]      # a still model, and a sample set that does not repeat within the frames
        mean, covered = {}, None
        for k, toggle in (("P", False), ("T", True)):
            x = make(a.width, a.height, met, a.depth, SETS[a.lights], toggle, still)
            c = x.context
            c.set_accumulation(True)
            for _ in range(frames):
                x.OnUpdate(); x.OnRender()
            c.sync()
            assert c.accumulated_frames() == frames
            mean[k] = (c.readback(capi.BUF_ACC_REFL)[..., :3].astype(np.float64) + c.readback(capi.BUF_ACC_DIFF)[..., :3].astype(np.float64)) / frames
            covered = c.readback(capi.BUF_VISIBILITY) != 0
            x.OnDestroy()
        y = {k: (0.25 * v[..., 0] + 0.5 * v[..., 1]) + 0.25 * v[..., 2] for k, v in mean.items()}
        d = mean["T"][covered] - mean["P"][covered]
        print(json.dumps({"frames": frames, "lights": a.lights, "depth": a.depth, "metallic": list(met), "covered_last_frame": int(covered.sum()),
                          "rel_l2_T_vs_P": float(np.sqrt((d * d).sum() / (mean["P"][covered] ** 2).sum())),
                          "T_strictly_above_P": int((y["T"] > y["P"])[covered].sum()), "T_below_P": int((y["T"] < y["P"])[covered].sum()),
                          "mean_luminance": {k: float(v[covered].mean()) for k, v in y.items()}}), flush=True)


if __name__ == "__main__":
    main()
