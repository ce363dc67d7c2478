"""The sun from the environment (rtggx_sun_from_env; DESIGN.md "The sun from the environment"): what the call costs and what it does to the image.
    cost    host time of the whole call (allocations, three reductions with a wait each, the frees; with removal the rewrite of level 0,
            the box chain and the swap) beside rtggx_generate_env_mips on the same cube, in one process and one context: synthetic cubes of
            side 256 and 1024 (a smooth sky and a sun two degrees across, tests/sunenv_cases.py's recipe about a free direction), default
            angles.  The cube is set again -- unmeasured -- before every timed call (a removal leaves no sun for the next one); `--calls`
            timed calls after one unmeasured, the sequence run `--rounds` times.
    image   the bunny at 1920 x 1080, still model and camera (-dt 0), -metallic 0.25 0.75, under the synthetic 256 probe, the mean of
            `--frames` accumulated frames: (probe) the probe alone, its sun in the cube; (hand) the probe as it is plus the measured sun
            through rtggx_set_sun -- what a user who types -sun beside such a probe gets: the sun twice --; (fromenv) the sun taken out of
            the cube and set as the light.  Printed: the mean luminance and the relative L2 distance between each pair, over the covered pixels
            and over the ground alone (instance 0: mostly diffuse at metallic 0.25, and no mirror image of this sun toward the camera).
One JSON line per row.
    python tools/probes/sunenv_probe.py [cost] [image] [--calls 7] [--rounds 2] [--frames 256]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import assets
import sunenv_cases as SC
import sunenv_ref as SR
from raytracedggx_amd import app, capi

TOWARD = np.array([0.35, 0.7, -0.62])      # above and in front of the default camera's view of the model


def probe_cube(S, patch_degrees=2.0, level=20000.0):
    """Level 0 codes uint16 [6, S, S, 4]: sunenv_cases' smooth background plus level (1 - angle / patch)^2 about TOWARD."""
    D = SR.directions(S).astype(np.float64)
    u = D / np.sqrt((D * D).sum(axis=1))[:, None]
    ang = np.degrees(np.arccos(np.clip(u @ (TOWARD / np.linalg.norm(TOWARD)), -1.0, 1.0)))
    sun = np.where(ang < patch_degrees, level * (1.0 - ang / patch_degrees) ** 2, 0.0)
    return SC.codes_of(S, SC.background(S, True, 21) + sun[:, None] * np.array([1.0, 0.9, 0.7]))


def cost(a):
    c = capi.Context(64, 64)
    for S in (256, 1024):
        codes = probe_cube(S).reshape(-1)

        def timed(fn):
            ms = []
            for k in range(a.calls + 1):
                c.set_env(capi.FORMAT_RGBA16F, S, 1, codes); c.sync()
                t0 = time.perf_counter(); r = fn(); t = (time.perf_counter() - t0) * 1e3
                if k:
                    ms.append(t)
            return r, {"min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3), "max_ms": round(max(ms), 3)}
        for rnd in range(a.rounds):
            for label, fn in (("rtggx_generate_env_mips", c.generate_env_mips), ("rtggx_sun_from_env remove 0", lambda: c.sun_from_env()),
                              ("rtggx_sun_from_env remove 1", lambda: c.sun_from_env(remove=True))):
                r, t = timed(fn)
                row = {"part": "cost", "round": rnd, "cube": "%d^2, %d texels" % (S, 6 * S * S), "call": label, "calls": a.calls}
                if r is not None:
                    row.update(found=r["found"], removed=r["removed"], texels_cone=r["texels_cone"], texels_ring=r["texels_ring"], texels_lit=r["texels_lit"])
                print(json.dumps(dict(row, **t)), flush=True)
    c.close()


def rgb16(words):
    return np.ascontiguousarray(words).view(np.float16).reshape(words.shape + (4,))[..., :3].astype(np.float64)


def rel_l2(x, ref, mask):
    x, ref = x[mask], ref[mask]
    return round(float(np.sqrt(((x - ref) ** 2).sum() / max((ref ** 2).sum(), 1e-300))), 5)


def image(a):
    W, H, S = 1920, 1080, 256
    codes = probe_cube(S)
    means, covered, ground, rec = {}, None, None, None
    for mode in ("probe", "hand", "fromenv"):
        x = app.RayTracedGGX(["-mesh", assets.path("bunny.obj"), "-env", assets.path("rnl_cross.dds"), "-width", W, "-height", H, "-dt", 0, "-metallic", 0.25, 0.75])
        c = x.context
        c.set_env(capi.FORMAT_RGBA16F, S, 1, codes.reshape(-1))
        c.generate_env_mips()
        if mode != "probe":
            rec = c.sun_from_env(remove=(mode == "fromenv"))
            c.set_sun(rec["direction"], rec["irradiance"])
        c.set_accumulation(True)
        for _ in range(a.frames):
            x.OnUpdate(); x.OnRender()
        vis = c.readback(capi.BUF_VISIBILITY)
        covered = vis != 0
        ground = covered & (((vis.astype(np.int64) - 1) >> 24) == 0)
        c.present_accumulation()
        means[mode] = rgb16(c.readback(capi.BUF_CONVERGED))
        x.OnDestroy()
    print(json.dumps({"part": "image", "probe": "synthetic %d^2, sun 2 degrees across toward %s" % (S, TOWARD.tolist()), "frames": a.frames, "covered_pixels": int(covered.sum()),
                      "direction": [float(v) for v in rec["direction"]], "irradiance": [float(v) for v in rec["irradiance"]], "texels_lit": rec["texels_lit"],
                      "ground_pixels": int(ground.sum()),
                      "mean_luma_covered": {m: round(float(SR.luma(means[m][covered]).mean()), 4) for m in means},
                      "mean_luma_ground": {m: round(float(SR.luma(means[m][ground]).mean()), 4) for m in means},
                      "median_luma_covered": {m: round(float(np.median(SR.luma(means[m][covered]))), 4) for m in means}}), flush=True)
    for x, ref in (("hand", "fromenv"), ("probe", "fromenv"), ("probe", "hand")):
        print(json.dumps({"part": "image", "what": "%s against %s" % (x, ref), "rel_l2_covered": rel_l2(means[x], means[ref], covered),
                          "rel_l2_ground": rel_l2(means[x], means[ref], ground)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["cost", "image"])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--frames", type=int, default=256)
    a = ap.parse_args()
    if "cost" in a.parts:
        cost(a)
    if "image" in a.parts:
        image(a)


if __name__ == "__main__":
    main()
