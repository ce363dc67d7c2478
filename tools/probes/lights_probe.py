"""Local lights (rtggx_set_lights; DESIGN.md "Local lights"): what a light costs.  Bunny, rnl environment, -sharedmem, 1920x1080 unless told
otherwise.  The lights are those of tests/golden/lights_classes.json (world space: they are the same lights at every frame size) -- 1: the
spot B alone; 3: A, B, C; 8: the three and five more around the model, points and spots, with and without a radius.  One JSON line per record.
    python tools/probes/lights_probe.py cost [--counts 0 1 3 8] [--pairs 4] [--metallic a b]
        one context per count in one process, 320 warm-up frames each, then windows of 256 frames alternating; host clock around frames
        that end in a synchronise.  ms per frame, the rays of the last frame and, against the lightless context, the shadow rays.
    python tools/probes/lights_probe.py frames [--lights N] [--frames 200]
        one context, N lights, that many frames: what a `rocprofv3 --kernel-trace --stats` run of its own wraps."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import assets
from raytracedggx_amd import app

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "lights_classes.json")))
A, B, C = GOLDEN["lights"]
MORE = [dict(position=[6.0, 3.0, -9.0], intensity=[40.0, 40.0, 60.0], range=14.0),
        dict(position=[-3.0, 11.0, 2.0], intensity=[150.0, 120.0, 90.0], range=30.0, radius=0.3, axis=[0.2, -1.0, -0.1], cos_outer=B["cos_outer"], cos_inner=B["cos_inner"]),
        dict(position=[0.0, 1.0, -9.0], intensity=[20.0, 25.0, 20.0], range=12.0, radius=0.25),
        dict(position=[9.0, 5.0, 4.0], intensity=[50.0, 30.0, 30.0], range=18.0),
        dict(position=[-9.0, 8.0, 6.0], intensity=[90.0, 90.0, 90.0], range=35.0, radius=0.0, axis=[1.0, -0.8, -0.6], cos_outer=B["cos_outer"], cos_inner=B["cos_inner"])]
SETS = {0: [], 1: [B], 3: [A, B, C], 8: [A, B, C] + MORE}


def make(w, h, metallic, lights):
    x = app.RayTracedGGX(["-mesh", assets.path("bunny.obj"), "-env", assets.path("rnl_cross.dds"), "-width", w, "-height", h, "-sharedmem"]
                         + (["-metallic", metallic[0], metallic[1]] if metallic else []))
    if lights:
        x.set_lights(lights)
    return x


def window(x, frames):
    c = x.context
    c.sync()
    t0 = time.perf_counter()
    for _ in range(frames):
        x.OnUpdate(); x.OnRender()
    c.sync()
    return (time.perf_counter() - t0) / frames * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["cost", "frames"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--metallic", type=float, nargs=2, default=None)
    ap.add_argument("--counts", type=int, nargs="+", default=[0, 1, 3, 8])
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--lights", type=int, default=3)
    ap.add_argument("--frames", type=int, default=200)
    a = ap.parse_args()
    if a.mode == "cost":
        apps = {n: make(a.width, a.height, a.metallic, SETS[n]) for n in a.counts}
        for x in apps.values():
            window(x, 320)
        ms = {n: [] for n in apps}
        for _ in range(a.pairs):
            for n, x in apps.items():
                ms[n].append(round(window(x, 256), 4))
        rays = {n: x.context.ray_count() for n, x in apps.items()}
        print(json.dumps({"config": "%dx%d %s" % (a.width, a.height, "default materials" if a.metallic is None else "-metallic %g %g" % tuple(a.metallic)),
                          "ms": {str(n): v for n, v in ms.items()}, "rays": {str(n): r for n, r in rays.items()},
                          "shadow_rays": {str(n): r - rays[0] for n, r in rays.items()} if 0 in rays else None}), flush=True)
        for x in apps.values():
            x.OnDestroy()
    else:
        x = make(a.width, a.height, a.metallic, SETS[a.lights])
        window(x, a.frames)
        print(json.dumps({"lights": a.lights, "frames": a.frames, "rays": x.context.ray_count()}), flush=True)
        x.OnDestroy()


if __name__ == "__main__":
    main()
