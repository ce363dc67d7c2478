"""The pick weighted by what the pixel remembers (rtggx_set_light_pick_visibility; DESIGN.md "The pick and what the pixel remembers"): what
the records cost on top of mode 1, and what they buy.  Bunny, rnl environment, -sharedmem, 1920x1080 unless told otherwise.  One JSON line
per record.
    python tools/probes/light_vis_probe.py cost [--counts 3 8] [--pairs 4]
        per material (default, -metallic 0.25 0.75) one context per (count, setting) in mode 1 in one process (tools/probes/lights_probe.py's
        light sets), 320 warm-up frames each, then windows of 256 frames alternating; ms per frame and the rays of the last frame.
    python tools/probes/light_vis_probe.py noise [--frames 64] [--reference-frames 256]
        mixed materials, the still model, the lights of tests/golden/light_vis_classes.json (a bright lamp behind the model, a dim one in
        front, a spot): a mode-0 context accumulates --reference-frames frames with a sample set of 65536; its mean is the reference three
        fresh contexts -- mode 0, mode 1, mode 1 with the records -- score every frame against on the device.  Per context the curves of
        se_out_rgb_cov and of its raw counterpart, as sums and as relative L2, and the rays of the last frame."""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from raytracedggx_amd import capi
from light_pick_probe import MATERIALS, make, material_name, measure
from lights_probe import SETS

OCCLUDED = json.load(open(os.path.join(ROOT, "tests", "golden", "light_vis_classes.json")))["lights"]


def make_vis(w, h, metallic, lights, mode, vis, extra=()):
    x = make(w, h, metallic, 1, lights, False, mode, extra)
    if vis:
        x.set_light_pick_visibility(1)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cost", "noise"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--counts", type=int, nargs="+", default=[3, 8])
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reference-frames", type=int, default=256)
    a = ap.parse_args()
    if a.what == "cost":
        for met in MATERIALS:
            apps = {}
            for n in a.counts:
                for vis in (0, 1):
                    apps["%d lights, mode 1%s" % (n, ", the records" if vis else "")] = make_vis(a.width, a.height, met, SETS[n], 1, vis)
            measure(apps, a.pairs, "%dx%d %s" % (a.width, a.height, material_name(met)))
        return
    if a.frames > capi.SCORE_RING:
        ap.error("the ring is read once at the end: at most %d frames" % capi.SCORE_RING)
    met, still = (0.25, 0.75), ["-dt", 0]
    r = make_vis(a.width, a.height, met, OCCLUDED, 0, 0, still + ["-sampleset", 65536])
    r.context.set_accumulation(True)
    for _ in range(a.reference_frames):
        r.OnUpdate(); r.OnRender()
    r.context.present_accumulation()
    assert r.context.accumulated_frames() == a.reference_frames
    reference = r.context.readback(capi.BUF_CONVERGED)
    r.OnDestroy()
    for name, mode, vis in (("mode 0", 0, 0), ("mode 1", 1, 0), ("mode 1, the records", 1, 1)):
        x = make_vis(a.width, a.height, met, OCCLUDED, mode, vis, still)
        c = x.context
        c.set_reference(reference); c.set_scoring(True)
        for _ in range(a.frames):
            x.OnUpdate(); x.OnRender()
        recs = c.read_scores()
        rel = lambda rec, se: round(math.sqrt(rec[se] / rec["ref_rgb2_cov"]), 5) if rec["ref_rgb2_cov"] > 0.0 else None
        print(json.dumps({"context": name, "frames": a.frames, "metallic": list(met), "reference": "mode 0, %d accumulated frames, sample set 65536" % a.reference_frames,
                          "rays_last_frame": c.ray_count(), "ref_rgb2_cov": recs[-1]["ref_rgb2_cov"],
                          "se_out_rgb_cov": [round(rec["se_out_rgb_cov"], 3) for rec in recs], "se_raw_rgb_cov": [round(rec["se_raw_rgb_cov"], 3) for rec in recs],
                          "rel_l2_out_cov": [rel(rec, "se_out_rgb_cov") for rec in recs], "rel_l2_raw_cov": [rel(rec, "se_raw_rgb_cov") for rec in recs]}), flush=True)
        x.OnDestroy()


if __name__ == "__main__":
    main()
