"""What the host tests of the settings (tests/test_*_host.py) share: the oracle's scene with FrameIndex set by hand, and the two tests every
setting brings along -- its C function declared, exported and bound; its command-line flag refused before a GPU is touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import assets
from gpu_support import FRAME_INDEX_OFFSET
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAW_BUFS = (O.BUF_RT_REFL, O.BUF_RT_DIFF, O.BUF_NORMAL, O.BUF_ROUGH_METAL, O.BUF_VELOCITY)      # what a ray trace of the oracle writes


def scene(o, mesh="bunny.obj", W=None, H=None, metallic=(1.0, 1.0), vndf=False, frame=1):
    """The oracle `o` with `mesh` under the still camera, `frame` + 1 frames in (FrameIndex and the model's turn advance with every frame),
    the visibility pass done.  W, H: the camera's aspect (default: the oracle's own size)."""
    v, i, _ = O.obj_import(assets.path(mesh))
    o.set_mesh(1, v, i)
    if mesh == "triangle.obj":
        o.set_env_rgba16f(1, 1, assets.constant_env_rgba16f(1.0))
    else:
        o.set_env_dds(assets.path("rnl_cross.dds"))
    o.set_metallic(0, metallic[0]); o.set_metallic(1, metallic[1])
    o.set_sampler(vndf)
    o.build_as()
    o.transform_sh()
    for _ in range(frame + 1):
        o.update_frame((10, 10, -24), O.camera_view_proj(W or o.W, H or o.H), 0.25)
    o.update_as()
    o.render_visibility()


def frame_index(o):
    return int(o.get_frame_constants()[FRAME_INDEX_OFFSET:FRAME_INDEX_OFFSET + 4].view(np.uint32)[0])


def set_frame_index(o, index):
    fc = o.get_frame_constants()
    fc[FRAME_INDEX_OFFSET:FRAME_INDEX_OFFSET + 4] = np.array([index], np.uint32).view(np.uint8)
    o.set_frame_constants(fc.tobytes())


def poison(o):      # (a word either renderer leaves alone stays poisoned in both)
    for b in RAW_BUFS:
        o.buffer(b, copy=False)[...] = 0xBEEF if b == O.BUF_ROUGH_METAL else 0xDEADBEEF


def declared_exported_bound(symbol, signature_regex, defines=(), method=None):
    """include/rtggx.h declares `symbol` with `signature_regex` and holds every regex of `defines`; the library exports it, capi lists it and
    capi.Context has `method`."""
    from raytracedggx_amd import capi
    header = open(os.path.join(ROOT, "include", "rtggx.h")).read()
    assert re.search(signature_regex, header), symbol
    for d in defines:
        assert re.search(d, header), d
    assert hasattr(C.CDLL(capi.LIB_PATH), symbol) and symbol in capi.EXPORTS, symbol
    assert callable(getattr(capi.Context, method or symbol[len("rtggx_"):], None)), symbol


SCENE = ("-mesh", assets.path("triangle.obj"), "-env", assets.path("rnl_cross.dds"), "-width", "64", "-height", "64")


def executable_refuses(cases, must_mention=None, scene=SCENE, no_device_message="HIP device", nor_on_stdout=False):
    """The executable ends every command line of `cases` with status 1 and `must_mention` on stderr (None: each case is a pair of the
    arguments and its own word), without a word of a device (`no_device_message`; nor_on_stdout: on neither stream) or of a rank."""
    exe = os.path.join(ROOT, "raytracedggx_amd", "RayTracedGGX")
    for case in cases:
        extra, word = (case, must_mention) if must_mention is not None else case
        r = subprocess.run([exe] + list(scene) + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (extra, r.returncode, r.stderr)
        assert word in r.stderr, (extra, r.stderr)
        assert no_device_message not in r.stderr and "rank" not in r.stderr.lower(), (extra, r.stderr)
        assert not nor_on_stdout or no_device_message not in r.stdout, (extra, r.stdout)
