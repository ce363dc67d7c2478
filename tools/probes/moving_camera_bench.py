"""The bench frame (1080p bunny, all-metal, free-running) with a camera that moves EVERY frame: a -track script holds the left button down and
drags the mouse along a slow Lissajous figure, so rg.ProjToWorld / rg.EyePt differ from frame to frame and no tile is ever left alone as
still sky (DESIGN.md section 5 "Still sky"): what the run words cost where they cannot help.  Same window as bench.py (256 priming frames,
64 warm-up, 256 timed, bracketed by synchronisation); prints one JSON line.
    python tools/probes/moving_camera_bench.py [--steps K] [--warmup W] [--mesh dragon.obj] [--metallic 0.25 0.5]"""
import argparse, json, math, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # as bench.py
import assets
from raytracedggx_amd.strips import StripRenderer

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=256); ap.add_argument("--warmup", type=int, default=64); ap.add_argument("--prime-frames", type=int, default=256)
ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--mesh", default="bunny.obj"); ap.add_argument("--metallic", type=float, nargs=2, default=None)
args = ap.parse_args()
total = args.prime_frames + args.warmup + args.steps
with tempfile.TemporaryDirectory() as tmp:
    track = os.path.join(tmp, "held_drag.track")
    with open(track, "w") as f:
        f.write("0 down %d %d\n" % (args.width // 2, args.height // 2))
        for k in range(1, total + 2):
            f.write("%d move %.3f %.3f\n" % (k, args.width / 2 + 300.0 * math.sin(0.05 * k), args.height / 2 + 60.0 * math.sin(0.031 * k)))
    r = StripRenderer(args.width, args.height, assets.path(args.mesh), assets.path("rnl_cross.dds"),
                      extra_args=("-sharedmem", "-track", track) + (("-metallic", args.metallic[0], args.metallic[1]) if args.metallic else ()))
    ctx = r.context
    eyes = set()
    for k in range(args.prime_frames + args.warmup):
        r.frame()
        if k < 8:
            eyes.add(r.app.frame_constants().tobytes()[448:528])
    assert len(eyes) >= 7, "the camera is not moving: %d views in 8 frames" % len(eyes)
    ctx.sync(); t0 = time.perf_counter()
    for _ in range(args.steps):
        r.frame()
    ctx.sync(); dt = time.perf_counter() - t0
    runs, threshold = ctx.sky_runs() if hasattr(ctx, "sky_runs") else (None, None)
    print(json.dumps({"probe": "moving_camera_bench", "mesh": args.mesh, "metallic": args.metallic, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_step": round(dt * 1e3 / args.steps, 4), "tiles_left_alone": None if runs is None else int((runs >= threshold).sum())}), flush=True)
    r.close()
