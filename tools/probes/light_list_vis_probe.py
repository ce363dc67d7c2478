"""A list's pick weighted by what the pixel remembers (rtggx_set_light_list_visibility; DESIGN.md "What a pixel remembers of a list"): what
the records cost on top of a list, and what they buy.  Bunny, rnl environment, -sharedmem, 1920x1080 unless told otherwise.  One JSON line
per record.
    python tools/probes/light_list_vis_probe.py cost [--counts 64 256 1024] [--pairs 3] [--frames 64]
        the lattices of tools/probes/light_list_probe.py: per n one context with the list alone and one with the records in one process,
        --frames warm-up frames each, then windows of --frames frames alternating; ms per frame, the rays of the last frame, and how many
        records of the last frame hold an entry.
    python tools/probes/light_list_vis_probe.py noise [--frames 64] [--reference-frames 512]
        mixed materials, the still model, 65 lights of tests/golden/light_list_vis_classes.json (56 of the lattice and the nine bright lamps
        behind the model): a context with the list alone accumulates --reference-frames frames with a sample set of 65536; its mean is the
        reference two fresh contexts -- the list, the list with the records -- score every frame against on the device.  Per context the
        curves of se_out_rgb_cov and of its raw counterpart, as sums and as relative L2, and the rays of the last frame."""
import argparse, json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from raytracedggx_amd import capi
from light_list_probe import lattice, make, measure

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "light_list_vis_classes.json")))["lights"]
OCCLUDED = GOLDEN[:56] + GOLDEN[64:]      # 65 lights: two chunks, the lamps behind the model last


def held(x):
    c = x.context
    seq = c.read_light_list_visibility(0)[1]
    records = c.read_light_list_visibility(seq & 1)[0]      # the image the last frame wrote
    written = (records["stamp"] >> 8) == (seq & 0xFFFFFF)
    entries = records["entry"][written]
    return {"records_written": int(written.sum()), "records_with_an_entry": int((entries != 0xFFFF).any(-1).sum()), "full_records": int((entries != 0xFFFF).all(-1).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cost", "noise"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--counts", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reference-frames", type=int, default=512)
    a = ap.parse_args()
    met = (0.25, 0.75)
    if a.what == "cost":
        for n in a.counts:
            apps = {"%d lights, the list" % n: make(a.width, a.height, met, 1), "%d lights, the records" % n: make(a.width, a.height, met, 1)}
            for x in apps.values():
                x.set_light_list(lattice(n))
            apps["%d lights, the records" % n].set_light_list_visibility(1)
            rec = measure(apps, a.pairs, a.frames, a.frames, {"config": "%dx%d -metallic 0.25 0.75 depth 1, lattice of %d" % (a.width, a.height, n)})
            rec["records"] = held(apps["%d lights, the records" % n])
            print(json.dumps(rec), flush=True)
            for x in apps.values():
                x.OnDestroy()
        return
    if a.frames > capi.SCORE_RING:
        ap.error("the ring is read once at the end: at most %d frames" % capi.SCORE_RING)
    still = ["-dt", 0]
    r = make(a.width, a.height, met, 1, still + ["-sampleset", 65536])
    r.set_light_list(OCCLUDED)
    r.context.set_accumulation(True)
    for _ in range(a.reference_frames):
        r.OnUpdate(); r.OnRender()
    r.context.present_accumulation()
    assert r.context.accumulated_frames() == a.reference_frames
    reference = r.context.readback(capi.BUF_CONVERGED)
    r.OnDestroy()
    for name, vis in (("the list", 0), ("the list, the records", 1)):
        x = make(a.width, a.height, met, 1, still)
        x.set_light_list(OCCLUDED)
        if vis:
            x.set_light_list_visibility(1)
        c = x.context
        c.set_reference(reference); c.set_scoring(True)
        for _ in range(a.frames):
            x.OnUpdate(); x.OnRender()
        recs = c.read_scores()
        rel = lambda rec, se: round(math.sqrt(rec[se] / rec["ref_rgb2_cov"]), 5) if rec["ref_rgb2_cov"] > 0.0 else None
        out = {"context": name, "frames": a.frames, "metallic": list(met), "lights": len(OCCLUDED),
               "reference": "the list, %d accumulated frames, sample set 65536" % a.reference_frames, "rays_last_frame": c.ray_count(),
               "ref_rgb2_cov": recs[-1]["ref_rgb2_cov"], "se_out_rgb_cov": [round(rec["se_out_rgb_cov"], 3) for rec in recs],
               "se_raw_rgb_cov": [round(rec["se_raw_rgb_cov"], 3) for rec in recs],
               "rel_l2_out_cov": [rel(rec, "se_out_rgb_cov") for rec in recs], "rel_l2_raw_cov": [rel(rec, "se_raw_rgb_cov") for rec in recs]}
        if vis:
            out["records"] = held(x)
        print(json.dumps(out), flush=True)
        x.OnDestroy()


if __name__ == "__main__":
    main()
