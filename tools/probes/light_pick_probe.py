"""One shadow ray per surface point for all lights (rtggx_set_light_sampling; DESIGN.md "One ray for all lights"): what mode 1 costs against
mode 0, and what it costs in quality.  Bunny, rnl environment, -sharedmem, 1920x1080 unless told otherwise; the light sets are
tools/probes/lights_probe.py's (1: the spot B; 3: A, B, C of tests/golden/lights_classes.json; 8: those and five more).  One JSON line per record.
    python tools/probes/light_pick_probe.py cost [--counts 1 3 8] [--pairs 4]
        per material (default, -metallic 0.25 0.75) one context without lights and one per (count, mode) in one process, 320 warm-up frames
        each, then windows of 256 frames alternating; host clock around frames that end in a synchronise.  ms per frame and the rays of the
        last frame.
    python tools/probes/light_pick_probe.py hits [--counts 3 8] [--depths 1 2] [--pairs 4]
        the same with -lightreflections, per material and depth: one context per (count, mode) beside one with the lights alone in mode 0.
    python tools/probes/light_pick_probe.py frames [--lights N] [--depth D] [--frames 200] [--metallic a b] [--mode 1]
        one context with -lightreflections, that many frames: what a `rocprofv3 --kernel-trace --stats` run of its own wraps.
    python tools/probes/light_pick_probe.py noise [--frames 64] [--reference-frames 256]
        mixed materials, the still model, the golden three lights: a mode-0 context accumulates --reference-frames frames with a sample set
        of 65536; its mean is the reference two fresh contexts, mode 0 and mode 1, score every frame against on the device.  Per mode the
        curve of se_out_rgb_cov (TemporalSSOut against the reference over covered pixels) and of its raw counterpart, as sums and as relative L2."""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assets
from raytracedggx_amd import app, capi
from lights_probe import SETS, window

MATERIALS = (None, (0.25, 0.75))


def make(w, h, metallic, depth, lights, toggle, mode, extra=()):
    x = app.RayTracedGGX(["-mesh", assets.path("bunny.obj"), "-env", assets.path("rnl_cross.dds"), "-width", w, "-height", h, "-sharedmem"]
                         + (["-metallic", metallic[0], metallic[1]] if metallic else []) + (["-recursion", depth] if depth != 1 else []) + list(extra))
    if lights:
        x.set_lights(lights)
    if toggle:
        x.set_light_reflections(1)
    if mode:
        x.set_light_sampling(mode)
    return x


def measure(apps, pairs, config):
    for x in apps.values():
        window(x, 320)
    ms = {k: [] for k in apps}
    for _ in range(pairs):
        for k, x in apps.items():
            ms[k].append(round(window(x, 256), 4))
    rays = {k: x.context.ray_count() for k, x in apps.items()}
    print(json.dumps({"config": config, "ms": ms, "mean_ms": {k: round(sum(v) / len(v), 4) for k, v in ms.items()}, "rays": rays}), flush=True)
    for x in apps.values():
        x.OnDestroy()


def material_name(met):
    return "default materials" if met is None else "-metallic %g %g" % met


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cost", "hits", "frames", "noise"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--metallic", type=float, nargs=2, default=None)
    ap.add_argument("--counts", type=int, nargs="+", default=None)
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--lights", type=int, default=3)
    ap.add_argument("--depth", type=int, default=1)
    ap.add_argument("--mode", type=int, default=1)
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--reference-frames", type=int, default=256)
    a = ap.parse_args()
    if a.what == "cost":
        for met in MATERIALS:
            apps = {"no lights": make(a.width, a.height, met, 1, [], False, 0)}
            for n in a.counts or [1, 3, 8]:
                for mode in (0, 1):
                    apps["%d lights, mode %d" % (n, mode)] = make(a.width, a.height, met, 1, SETS[n], False, mode)
            measure(apps, a.pairs, "%dx%d %s" % (a.width, a.height, material_name(met)))
    elif a.what == "hits":
        for met in MATERIALS:
            for depth in a.depths:
                apps = {}
                for n in a.counts or [3, 8]:
                    apps["%d lights alone, mode 0" % n] = make(a.width, a.height, met, depth, SETS[n], False, 0)
                    for mode in (0, 1):
                        apps["%d lights at the hits, mode %d" % (n, mode)] = make(a.width, a.height, met, depth, SETS[n], True, mode)
                measure(apps, a.pairs, "%dx%d %s depth %d, -lightreflections" % (a.width, a.height, material_name(met), depth))
    elif a.what == "frames":
        frames = a.frames or 200
        x = make(a.width, a.height, a.metallic, a.depth, SETS[a.lights], True, a.mode)
        window(x, frames)
        print(json.dumps({"lights": a.lights, "depth": a.depth, "mode": a.mode, "metallic": a.metallic, "frames": frames, "rays": x.context.ray_count()}), flush=True)
        x.OnDestroy()
    else:
        frames = a.frames or 64
        if frames > capi.SCORE_RING:
            ap.error("the ring is read once at the end: at most %d frames" % capi.SCORE_RING)
        met = tuple(a.metallic) if a.metallic else (0.25, 0.75)
        still = ["-dt", 0]
        r = make(a.width, a.height, met, 1, SETS[3], False, 0, still + ["-sampleset", 65536])
        r.context.set_accumulation(True)
        for _ in range(a.reference_frames):
            r.OnUpdate(); r.OnRender()
        r.context.present_accumulation()
        assert r.context.accumulated_frames() == a.reference_frames
        reference = r.context.readback(capi.BUF_CONVERGED)
        r.OnDestroy()
        for mode in (0, 1):
            x = make(a.width, a.height, met, 1, SETS[3], False, mode, still)
            c = x.context
            c.set_reference(reference); c.set_scoring(True)
            for _ in range(frames):
                x.OnUpdate(); x.OnRender()
            recs = c.read_scores()
            rel = lambda rec, se: round(math.sqrt(rec[se] / rec["ref_rgb2_cov"]), 5) if rec["ref_rgb2_cov"] > 0.0 else None
            print(json.dumps({"mode": mode, "frames": frames, "metallic": list(met), "reference": "mode 0, %d accumulated frames, sample set 65536" % a.reference_frames,
                              "rays_last_frame": c.ray_count(), "ref_rgb2_cov": recs[-1]["ref_rgb2_cov"],
                              "se_out_rgb_cov": [round(rec["se_out_rgb_cov"], 3) for rec in recs], "se_raw_rgb_cov": [round(rec["se_raw_rgb_cov"], 3) for rec in recs],
                              "rel_l2_out_cov": [rel(rec, "se_out_rgb_cov") for rec in recs], "rel_l2_raw_cov": [rel(rec, "se_raw_rgb_cov") for rec in recs]}), flush=True)
            x.OnDestroy()


if __name__ == "__main__":
    main()
