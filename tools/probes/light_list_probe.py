"""A culled light list (rtggx_set_light_list; DESIGN.md "A culled light list"): what the generality costs at eight lights against mode 1 of
rtggx_set_lights, and how a frame scales with the length of the list, with the cull and without it.  Bunny, rnl environment, -sharedmem,
1920x1080 unless told otherwise.  One JSON line per record.
    python tools/probes/light_list_probe.py eight [--pairs 4]
        the eight lights of tools/probes/lights_probe.py (SETS[8]) through rtggx_set_lights in mode 1 and as a list, per material (default,
        -metallic 0.25 0.75) at depth 1, and with -lightreflections at depth 2: contexts in one process, 320 warm-up frames each, then
        windows of 256 frames alternating; host clock around frames that end in a synchronise.  ms per frame and the rays of the last frame.
    python tools/probes/light_list_probe.py scaling [--counts 64 256 1024] [--pairs 3] [--frames 64] [--reflections]
        lattices of n small-range point lights over the ground, a point of it within range of a handful: per n
        one context with the cull and one with rtggx_debug_light_list_cull(ctx, 0), --frames warm-up frames each, then windows of --frames
        frames alternating; the kept lights per block with a covered pixel (mean, max) of the last frame.  --reflections: depth 2 with
        -lightreflections."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import assets
from raytracedggx_amd import app, capi
from lights_probe import SETS, window

MATERIALS = (None, (0.25, 0.75))


def make(w, h, metallic, depth, extra=()):
    return app.RayTracedGGX(["-mesh", assets.path("bunny.obj"), "-env", assets.path("rnl_cross.dds"), "-width", w, "-height", h, "-sharedmem"]
                            + (["-metallic", metallic[0], metallic[1]] if metallic else []) + (["-recursion", depth] if depth != 1 else []) + list(extra))


def lattice(n):
    """n point lights (a square number): a square lattice over the ground, x, z in [-9.5, 9.5], half a spacing above it, the range 1.3
    spacings, so that a point of the ground lies within range of about five; the intensity grows with the range squared."""
    side = int(round(n ** 0.5))
    assert side * side == n, n
    spacing = 19.0 / (side - 1)
    reach = 1.3 * spacing
    return [dict(position=[-9.5 + spacing * ix, 0.5 * spacing, -9.5 + spacing * iz], intensity=[2.0 * reach * reach, 1.8 * reach * reach, 1.5 * reach * reach], range=reach)
            for iz in range(side) for ix in range(side)]


def measure(apps, pairs, warm, frames, record):
    for x in apps.values():
        window(x, warm)
    ms = {k: [] for k in apps}
    for _ in range(pairs):
        for k, x in apps.items():
            ms[k].append(round(window(x, frames), 4))
    record.update(ms=ms, mean_ms={k: round(sum(v) / len(v), 4) for k, v in ms.items()}, rays={k: x.context.ray_count() for k, x in apps.items()})
    return record


def kept(x):
    c = x.context
    c.sync()
    counts, vis = c.read_light_list_counts(), c.readback(capi.BUF_VISIBILITY) != 0
    H, W = vis.shape
    pad = np.zeros((counts.shape[0] * 8, counts.shape[1] * 8), bool)
    pad[:H, :W] = vis
    covered = pad.reshape(counts.shape[0], 8, counts.shape[1], 8).any((1, 3))
    return {"blocks": int(covered.sum()), "mean": round(float(counts[covered].mean()), 2), "max": int(counts.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["eight", "scaling"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--counts", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--pairs", type=int, default=None)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reflections", action="store_true")
    a = ap.parse_args()
    if a.what == "eight":
        for met in MATERIALS:
            for depth, toggle in ((1, False), (2, True)):
                apps = {"8 lights, mode 1": make(a.width, a.height, met, depth), "8 lights, a list": make(a.width, a.height, met, depth)}
                apps["8 lights, mode 1"].set_lights(SETS[8]); apps["8 lights, mode 1"].set_light_sampling(1)
                apps["8 lights, a list"].set_light_list(SETS[8])
                for x in apps.values():
                    x.set_light_reflections(1 if toggle else 0)
                rec = measure(apps, a.pairs or 4, 320, 256, {"config": "%dx%d %s depth %d%s" % (
                    a.width, a.height, "default materials" if met is None else "-metallic %g %g" % met, depth, ", -lightreflections" if toggle else "")})
                rec["kept"] = kept(apps["8 lights, a list"])
                print(json.dumps(rec), flush=True)
                for x in apps.values():
                    x.OnDestroy()
    else:
        depth = 2 if a.reflections else 1
        for n in a.counts:
            apps = {"%d lights, cull" % n: make(a.width, a.height, (0.25, 0.75), depth), "%d lights, no cull" % n: make(a.width, a.height, (0.25, 0.75), depth)}
            for k, x in apps.items():
                x.set_light_list(lattice(n)); x.set_light_reflections(1 if a.reflections else 0)
            apps["%d lights, no cull" % n].context.debug_light_list_cull(0)
            rec = measure(apps, a.pairs or 3, a.frames, a.frames, {"config": "%dx%d -metallic 0.25 0.75 depth %d%s, lattice of %d" % (
                a.width, a.height, depth, ", -lightreflections" if a.reflections else "", n)})
            rec["kept"] = {k: kept(x) for k, x in apps.items()}
            print(json.dumps(rec), flush=True)
            for x in apps.values():
                x.OnDestroy()


if __name__ == "__main__":
    main()
