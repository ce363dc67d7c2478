"""Moving light lists (rtggx_update_light_list, rtggx_update_light_list_device; DESIGN.md section 9 "Moving light lists"): what a frame costs
when the list changes before every frame, by each of the ways to change it, and what the records buy on a list that moves.  Bunny, rnl
environment, -sharedmem, -metallic 0.25 0.75, 1920x1080 unless told otherwise; lattices of n lights orbiting the world y axis by --degrees a
frame, every list computed before the clock starts.  It reads nothing outside the repository.  One JSON line per record.
    python tools/moving_lights.py time --mode static|set|host|device [--count 256] [--frames 256] [--warmup 64]
        ONE mode in this process: ms per frame over --frames un-synchronised frames that end in one synchronise, and the drains
        (rtggx_debug_visibility_drains) and fence waits of the window.  static: the list never changes; set: rtggx_set_light_list before
        every frame (the only way before; this mode runs on the parent commit as well); host / device: the update calls.
    python tools/moving_lights.py pairs [--counts 64 256 1024] [--pairs 8]
        the protocol of the timing runs: per count and pair the four modes one after the other, each in a fresh child process.
    python tools/moving_lights.py records [--frames 64] [--reference-frames 512]
        65 lights of tests/golden/light_list_vis_classes.json (56 of its lattice, then the nine bright lamps), the lamps moving along
        tests/light_list_moving_ref.py's line over --frames frames, the model still.  Reference: the mean of --reference-frames
        accumulated frames over the same motion, sample set 65536.  Two fresh contexts -- the list, the list with the records -- run the
        motion once with rtggx_update_light_list before every frame and score every frame on the device (rtggx_set_scoring): the last
        frame's se_out_rgb_cov and se_raw_rgb_cov, and its ray count."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools", "probes"))
import numpy as np


def rows_of(lights):
    from raytracedggx_amd import capi
    return np.frombuffer(b"".join(bytes(capi.Light.of(**l)) for l in lights), np.float32).reshape(-1, 16).copy()


def rotate_y(rows, degrees):
    out = rows.copy()
    a = np.radians(float(degrees)); ca, sa = np.cos(a), np.sin(a)
    x, z = rows[:, 0].astype(np.float64), rows[:, 2].astype(np.float64)
    out[:, 0], out[:, 2] = (x * ca + z * sa).astype(np.float32), (z * ca - x * sa).astype(np.float32)
    return out


def run_mode(a):
    if a.mode == "device":      # (torch finds its device before the application's library is loaded, as in the tests)
        import torch
        torch.cuda.init()
    from raytracedggx_amd import capi
    from light_list_probe import lattice, make
    base = lattice(a.count)
    rows = rows_of(base)
    period = 64
    lists = [rotate_y(rows, a.degrees * f) for f in range(period)]
    x = make(a.width, a.height, (0.25, 0.75), 1)
    c = x.context
    x.set_light_list(base)
    updates = hasattr(c, "update_light_list")      # (the parent commit has none: static and set only)
    if a.mode in ("host", "device") and not updates:
        raise SystemExit("this build has no rtggx_update_light_list")
    if a.mode == "set":
        arrays = [(capi.Light * a.count).from_buffer_copy(l.tobytes()) for l in lists]
    if a.mode == "device":
        stream = torch.cuda.Stream()
        dev = [torch.from_numpy(l).cuda() for l in lists]
        torch.cuda.synchronize()

    def frame(f):
        k = f % period
        if a.mode == "set":
            c._check(c.L.rtggx_set_light_list(c.h, arrays[k], a.count))
        elif a.mode == "host":
            c.update_light_list(lists[k])
        elif a.mode == "device":
            c.update_light_list_device(dev[k].data_ptr(), 0, a.count, 0, stream.cuda_stream)
        x.OnUpdate(); x.OnRender()
    for f in range(a.warmup):
        frame(f)
    c.sync()
    if updates:
        c.debug_visibility_drains(reset=True)
    c.fence_wait(True)
    t0 = time.perf_counter()
    for f in range(a.warmup, a.warmup + a.frames):
        frame(f)
    c.sync()
    ms = (time.perf_counter() - t0) * 1e3 / a.frames
    us, waits = c.fence_wait(True)
    print(json.dumps({"mode": a.mode, "lights": a.count, "size": [a.width, a.height], "frames": a.frames, "ms_per_frame": round(ms, 4),
                      "drains": c.debug_visibility_drains() if updates else None, "fence_waits": waits, "rays_last_frame": c.ray_count()}), flush=True)
    x.OnDestroy()


def run_pairs(a):
    for n in a.counts:
        out = {m: [] for m in ("static", "set", "host", "device")}
        for _ in range(a.pairs):
            for m in out:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "time", "--mode", m, "--count", str(n), "--frames", str(a.frames), "--warmup", str(a.warmup),
                                    "--width", str(a.width), "--height", str(a.height)], capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise SystemExit("mode %s, %d lights: %s" % (m, n, r.stderr[-400:]))
                out[m].append(json.loads(r.stdout.strip().splitlines()[-1])["ms_per_frame"])
        print(json.dumps({"lights": n, "size": [a.width, a.height], "ms_per_frame": out, "mean": {m: round(sum(v) / len(v), 4) for m, v in out.items()},
                          "update_below_set_in_pairs": {m: sum(1 for u, s in zip(out[m], out["set"]) if u < s) for m in ("host", "device")}}), flush=True)


def run_records(a):
    import json as J
    import light_list_moving_ref as LM
    from raytracedggx_amd import capi
    from light_list_probe import make
    golden = J.load(open(os.path.join(ROOT, "tests", "golden", "light_list_vis_classes.json")))["lights"]
    occluded = golden[:56] + golden[64:]      # 65 lights, the nine lamps last
    rows = rows_of(occluded)
    lamps = slice(56, 65)

    def moved(f):
        out = rows.copy()
        t = (f % (2 * a.frames)) / float(a.frames)
        t = t if t <= 1.0 else 2.0 - t      # there and back
        for k in range(3):
            out[lamps, k] = (rows[lamps, k].astype(np.float64) + t * LM.TRAVEL[k]).astype(np.float32)
        return out
    still = ["-dt", 0]
    r = make(a.width, a.height, (0.25, 0.75), 1, still + ["-sampleset", 65536])
    r.set_light_list(occluded); r.context.set_accumulation(True)
    for f in range(a.reference_frames):
        r.context.update_light_list(moved(f % a.frames)); r.OnUpdate(); r.OnRender()
    r.context.present_accumulation()
    reference = r.context.readback(capi.BUF_CONVERGED)
    r.OnDestroy()
    for name, vis in (("the moving list", 0), ("the moving list, the records", 1)):
        x = make(a.width, a.height, (0.25, 0.75), 1, still)
        x.set_light_list(occluded)
        if vis:
            x.set_light_list_visibility(1)
        c = x.context
        c.set_reference(reference); c.set_scoring(True)
        for f in range(a.frames):
            c.update_light_list(moved(f)); x.OnUpdate(); x.OnRender()
        recs = c.read_scores()
        print(json.dumps({"context": name, "frames": a.frames, "reference": "the mean of %d frames over the same motion" % a.reference_frames,
                          "se_out_rgb_cov_last": round(recs[-1]["se_out_rgb_cov"], 3), "se_raw_rgb_cov_last": round(recs[-1]["se_raw_rgb_cov"], 3),
                          "rays_last_frame": c.ray_count(), "drains": c.debug_visibility_drains()}), flush=True)
        x.OnDestroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["time", "pairs", "records"])
    ap.add_argument("--mode", choices=["static", "set", "host", "device"], default="static")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--counts", type=int, nargs="+", default=[64, 256, 1024])
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--degrees", type=float, default=2.0)
    ap.add_argument("--reference-frames", type=int, default=512)
    a = ap.parse_args()
    {"time": run_mode, "pairs": run_pairs, "records": run_records}[a.what](a)


if __name__ == "__main__":
    main()
