"""A sun with a size (rtggx_set_sun_angle; DESIGN.md "A sun with a size"): what the angle costs and what it does to a converged image.  Sun:
direction (-0.6, 0.5, -0.3), irradiance (3, 3, 3); bunny, rnl environment, 1920x1080 unless told otherwise.  One JSON line per record.
    python tools/probes/sun_soft_probe.py window [--reflections] [--angle A] [--metallic a b] [--depth D]
        one context, 320 warm-up frames, then 4 windows of 256 frames, host clock around frames that end in a synchronise.  Without --angle it
        calls nothing this feature added, so it runs on the parent commit as well: a process per measurement, parent and tree alternating.
    python tools/probes/sun_soft_probe.py angles [--angles 0 0.27 2 5] [--pairs 4]
        per configuration one context per angle in one process, windows of 256 frames alternating; ms per frame and the rays of the last frame.
    python tools/probes/sun_soft_probe.py picture [--frames 1024] [--angle 5]
        mixed materials, still model, a sample set of 1024: three contexts accumulate the same frames without a sun (U), with the directional sun (D) and at the angle (S).
        Relative L2 of S against D over covered pixels, and the pixels of S strictly between U and D -- the outer half of a penumbra, where
        the direction alone is lit -- and strictly above D, the inner half, where the direction alone is in shadow."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import assets
from raytracedggx_amd import app, capi

SUN = ["-sun", -0.6, 0.5, -0.3, 3.0, 3.0, 3.0]


def make(w, h, extra):
    return app.RayTracedGGX(["-mesh", assets.path("bunny.obj"), "-env", assets.path("rnl_cross.dds"), "-width", w, "-height", h, "-sharedmem"] + list(extra))


def window(x, frames):
    c = x.context
    c.sync()
    t0 = time.perf_counter()
    for _ in range(frames):
        x.OnUpdate(); x.OnRender()
    c.sync()
    return (time.perf_counter() - t0) / frames * 1e3


def flags(a, angle=None):
    extra = list(SUN)
    if a.reflections:
        extra += ["-sunreflections"]
    if a.metallic:
        extra += ["-metallic", a.metallic[0], a.metallic[1]]
    if a.depth != 1:
        extra += ["-recursion", a.depth]
    if angle is not None:
        extra += ["-sunangle", angle]
    return extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["window", "angles", "picture"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reflections", action="store_true")
    ap.add_argument("--metallic", type=float, nargs=2, default=None)
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--angle", type=float, default=None)
    ap.add_argument("--angles", type=float, nargs="+", default=[0.0, 0.27, 2.0, 5.0])
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.mode == "window":
        x = make(a.width, a.height, flags(a, a.angle))
        window(x, 320)
        ms = [round(window(x, 256), 4) for _ in range(4)]
        print(json.dumps({"label": a.label, "reflections": a.reflections, "angle": a.angle, "depth": a.depth, "metallic": a.metallic, "ms": ms, "mean_ms": round(sum(ms) / 4, 4),
                          "rays": x.context.ray_count()}), flush=True)
        x.OnDestroy()
    elif a.mode == "angles":
        for refl, met, depth in ((False, None, 1), (True, None, 1), (True, (0.25, 0.75), 2)):
            a.reflections, a.metallic, a.depth = refl, met, depth
            apps = {g: make(a.width, a.height, flags(a, g)) for g in a.angles}
            for x in apps.values():
                window(x, 320)
            ms = {g: [] for g in apps}
            for _ in range(a.pairs):
                for g, x in apps.items():
                    ms[g].append(round(window(x, 256), 4))
            print(json.dumps({"config": "%dx%d %s depth %d%s" % (a.width, a.height, "default materials" if met is None else "-metallic %g %g" % met, depth, " -sunreflections" if refl else ""),
                              "ms": {str(g): v for g, v in ms.items()}, "rays": {str(g): x.context.ray_count() for g, x in apps.items()}}), flush=True)
            for x in apps.values():
                x.OnDestroy()
    else:
        a.metallic = a.metallic or (0.25, 0.75)
        met = ["-metallic", a.metallic[0], a.metallic[1], "-dt", 0, "-sampleset", 1024]      # a still model, and a sample set that does not repeat within the frames
        angle = 5.0 if a.angle is None else a.angle
        apps = {"U": make(a.width, a.height, met), "D": make(a.width, a.height, met + SUN), "S": make(a.width, a.height, met + SUN + ["-sunangle", angle])}
        mean = {}
        for k, x in apps.items():
            c = x.context
            c.set_accumulation(True)
            for _ in range(a.frames):
                x.OnUpdate(); x.OnRender()
            c.sync()
            assert c.accumulated_frames() == a.frames
            mean[k] = (c.readback(capi.BUF_ACC_REFL)[..., :3].astype(np.float64) + c.readback(capi.BUF_ACC_DIFF)[..., :3].astype(np.float64)) / a.frames
            covered = c.readback(capi.BUF_VISIBILITY) != 0
            x.OnDestroy()
        y = {k: (0.25 * v[..., 0] + 0.5 * v[..., 1]) + 0.25 * v[..., 2] for k, v in mean.items()}
        d = mean["S"][covered] - mean["D"][covered]
        print(json.dumps({"frames": a.frames, "angle": angle, "metallic": list(a.metallic), "covered_last_frame": int(covered.sum()),
                          "rel_l2_S_vs_D": float(np.sqrt((d * d).sum() / (mean["D"][covered] ** 2).sum())),
                          "S_strictly_between_U_and_D": int(((y["S"] > y["U"]) & (y["S"] < y["D"]))[covered].sum()),
                          "S_strictly_above_D": int((y["S"] > y["D"])[covered].sum()),
                          "D_strictly_above_U": int((y["D"] > y["U"])[covered].sum())}), flush=True)


if __name__ == "__main__":
    main()
