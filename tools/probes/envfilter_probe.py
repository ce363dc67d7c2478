"""GGX-prefiltered environments (rtggx_prefilter_env; DESIGN.md "Prefiltered environments"): what the call costs and what it does to the image.
    cost    host time of the whole call (tables, uploads, kernels, the wait, the frees) beside rtggx_generate_env_mips on the same cube, in
            one process and one context: rnl_cross.dds (256^2, 9 levels) at N = 256, 1024 and 4096, and the 512 cube of a 2048 x 1024
            panorama of random pixels at N = 1024; `--calls` timed calls after one unmeasured, the sequence run `--rounds` times.
    image   the bunny at 1920 x 1080, still model and camera (-dt 0), with the environment's levels below level 0 being (dds) the file's
            own, (box) rtggx_generate_env_mips', (ggx) rtggx_prefilter_env's at N = 1024.  Per chain: a reference -- recursion depth 3, -spp 8,
            sample set 4096, accumulated over `--reference-frames` frames and presented -- and the renderer as shipped at depth 1: the
            converged mean of `--frames` frames (accumulation: the bias alone) and the denoised image of the last of them.  Printed: the relative
            L2 distance, over the covered pixels (the sky is the same everywhere) and over all, of each depth-1 image from each reference.
One JSON line per row.  --lib: another build of librtggx.so for the cost part (a comparison of kernel variants; the image part goes through
the application library, which binds the build beside it).
    python tools/probes/envfilter_probe.py [cost] [image] [--calls 7] [--rounds 2] [--frames 256] [--reference-frames 512] [--lib path]"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import assets
from oracle import oracle as O
from raytracedggx_amd import app, capi


def timed(fn, calls):
    fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter(); fn(); ms.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(ms), 3), "median_ms": round(float(np.median(ms)), 3), "max_ms": round(max(ms), 3)}


def cost(a):
    o = O.Oracle(1, 1)      # (the file's BC6H blocks decoded on the CPU: with --lib no second build of the library enters the process)
    o.set_env_dds(assets.path("rnl_cross.dds"))
    size, mips, dds = o.env_texels()      # mip-major, uint16 [texels, 4]
    o.close()
    assert (size, mips) == (256, 9)
    level0 = dds[:6 * 256 * 256].reshape(6, 256 * 256 * 4)
    rng = np.random.default_rng(1)
    pano = rng.uniform(0.0, 8.0, (1024, 2048, 3)).astype(np.float32)
    c = capi.Context(64, 64)
    for rnd in range(a.rounds):
        for cube, setup in (("rnl_cross.dds level 0, 256^2, 9 levels", lambda: c.set_env(capi.FORMAT_RGBA16F, 256, 1, level0.reshape(-1))),
                            ("panorama 2048x1024 -> 512^2, 10 levels", lambda: c.set_env_image(capi.ENV_EQUIRECT, capi.PIXELS_RGB32F, 2048, 1024, pano, cube_size=512))):
            setup()
            rows = [("rtggx_generate_env_mips", c.generate_env_mips)]
            rows += [("rtggx_prefilter_env(%d)" % n, (lambda n=n: c.prefilter_env(n))) for n in ((256, 1024, 4096) if cube.startswith("rnl") else (1024,))]
            for label, fn in rows:
                print(json.dumps(dict({"part": "cost", "round": rnd, "cube": cube, "call": label, "calls": a.calls, "lib": capi.LIB_PATH}, **timed(fn, a.calls))), flush=True)
    c.close()


def rgb16(words):
    return np.ascontiguousarray(words).view(np.float16).reshape(words.shape + (4,))[..., :3].astype(np.float64)


def rel_l2(x, ref, mask=None):
    if mask is not None:
        x, ref = x[mask], ref[mask]
    ok = np.isfinite(x).all(axis=-1) & np.isfinite(ref).all(axis=-1)      # (pixels with a non-finite component in either image are left out)
    x, ref = x[ok], ref[ok]
    return round(float(np.sqrt(((x - ref) ** 2).sum() / max((ref ** 2).sum(), 1e-300))), 5)


def image(a):
    W, H = 1920, 1080

    def make(chain, extra):
        x = app.RayTracedGGX(["-mesh", assets.path("bunny.obj"), "-env", assets.path("rnl_cross.dds"), "-width", W, "-height", H, "-dt", 0] + extra)
        if chain == "box":
            x.context.generate_env_mips()
        elif chain == "ggx":
            x.context.prefilter_env(1024)
        return x

    chains = ("dds", "box", "ggx")
    reference, mean1, last1, covered = {}, {}, {}, None
    for chain in chains:
        x = make(chain, ["-recursion", 3, "-spp", 8, "-sampleset", 4096])
        x.context.set_accumulation(True)
        for _ in range(a.reference_frames):
            x.OnUpdate(); x.OnRender()
        x.context.present_accumulation()
        reference[chain] = rgb16(x.context.readback(capi.BUF_CONVERGED))
        x.OnDestroy()
        x = make(chain, [])
        x.context.set_accumulation(True)
        for _ in range(a.frames):
            x.OnUpdate(); x.OnRender()
        c = x.context
        last1[chain] = rgb16(c.readback(capi.BUF_TSS0 + c.frame_parity()))
        covered = c.readback(capi.BUF_VISIBILITY) != 0
        c.present_accumulation()
        mean1[chain] = rgb16(c.readback(capi.BUF_CONVERGED))
        x.OnDestroy()
    for ref in chains:
        for chain in chains:
            print(json.dumps({"part": "image", "reference": "depth 3, spp 8, sample set 4096, %d frames, chain %s" % (a.reference_frames, ref), "depth1_chain": chain, "frames": a.frames,
                              "covered_pixels": int(covered.sum()),
                              "rel_l2_mean_covered": rel_l2(mean1[chain], reference[ref], covered), "rel_l2_mean_all": rel_l2(mean1[chain], reference[ref]),
                              "rel_l2_denoised_covered": rel_l2(last1[chain], reference[ref], covered), "rel_l2_denoised_all": rel_l2(last1[chain], reference[ref])}), flush=True)
    for chain in ("box", "ggx"):
        print(json.dumps({"part": "image", "what": "depth-1 mean, chain %s against chain dds, covered" % chain, "rel_l2": rel_l2(mean1[chain], mean1["dds"], covered)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parts", nargs="*", default=["cost", "image"])
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reference-frames", type=int, default=512)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    if "cost" in a.parts:
        cost(a)
    if "image" in a.parts:
        image(a)


if __name__ == "__main__":
    main()
