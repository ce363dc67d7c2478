"""Python driver over the C++ host layer (libRayTracedGGX.so): the frame entry is the reference's
RayTracedGGX::OnUpdate / OnRender, the constructor takes the reference's command line
(`-mesh <obj> x y z s`, `-env <dds>`; RayTracedGGX.cpp:462-511) plus the headless extensions.
"""
import ctypes as C
import os

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "libRayTracedGGX.so")
HOST_EXPORTS = ["rtggx_app_last_error", "rtggx_app_create", "rtggx_app_destroy", "rtggx_app_on_update", "rtggx_app_on_render",
                "rtggx_app_on_key_up", "rtggx_app_set_time_step", "rtggx_app_context", "rtggx_app_size",
                "rtggx_app_frame_constants", "rtggx_app_save_image", "rtggx_host_obj_import", "rtggx_host_obj_copy",
                "rtggx_host_halton", "rtggx_host_frame_constants", "rtggx_host_write_png", "rtggx_host_camera",
                "rtggx_app_on_lbutton_down", "rtggx_app_on_lbutton_up", "rtggx_app_on_mouse_move", "rtggx_app_on_mouse_wheel", "rtggx_app_load_track",
                "rtggx_host_exchange_plan", "rtggx_host_balanced_bounds", "rtggx_app_set_dump_prefix", "rtggx_app_last_screen_shot", "rtggx_app_save_converged",
                "rtggx_host_frame_indices", "rtggx_host_accumulation_note",
                "rtggx_app_save_reference", "rtggx_app_flush_scores", "rtggx_app_set_reference", "rtggx_app_set_scoring", "rtggx_app_read_scores",
                "rtggx_host_write_pfm", "rtggx_host_read_pfm", "rtggx_host_load_env_image",
                "rtggx_app_set_sample_map", "rtggx_app_set_lights", "rtggx_app_set_light_reflections", "rtggx_app_set_light_sampling",
                "rtggx_app_set_light_pick_visibility", "rtggx_app_set_light_list",
                "rtggx_app_set_light_list_visibility", "rtggx_app_update_light_list", "rtggx_app_update_light_list_device",
                "rtggx_app_read_light_list"]

_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise ImportError("libRayTracedGGX.so is not built: run __graft_entry__.build() or `make -C raytracedggx_amd`")
        capi.load()  # librtggx.so first (same directory, also found through rpath)
        L = C.CDLL(HOST_LIB_PATH)
        L.rtggx_app_last_error.restype = C.c_char_p
        L.rtggx_app_create.restype = C.c_void_p
        L.rtggx_app_create.argtypes = [C.c_int, C.POINTER(C.c_char_p)]
        L.rtggx_app_context.restype = C.c_void_p
        for n in ("rtggx_app_destroy", "rtggx_app_on_update", "rtggx_app_on_render"):
            getattr(L, n).argtypes = [C.c_void_p]
            getattr(L, n).restype = None
        L.rtggx_app_context.argtypes = [C.c_void_p]
        L.rtggx_app_on_key_up.argtypes = [C.c_void_p, C.c_int]
        L.rtggx_app_set_time_step.argtypes = [C.c_void_p, C.c_float]
        L.rtggx_app_size.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.rtggx_app_frame_constants.argtypes = [C.c_void_p, C.c_void_p]
        L.rtggx_app_save_image.argtypes = [C.c_void_p, C.c_char_p]
        L.rtggx_app_save_converged.argtypes = [C.c_void_p, C.c_char_p]
        L.rtggx_app_set_dump_prefix.argtypes = [C.c_void_p, C.c_char_p]
        L.rtggx_app_save_reference.argtypes = [C.c_void_p, C.c_char_p]
        L.rtggx_app_flush_scores.argtypes = [C.c_void_p]
        L.rtggx_app_set_reference.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rtggx_app_set_scoring.argtypes = [C.c_void_p, C.c_int]
        L.rtggx_app_read_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.rtggx_host_write_pfm.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rtggx_host_read_pfm.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rtggx_host_load_env_image.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_int),
                                                C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.rtggx_app_set_sample_map.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.rtggx_app_set_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.rtggx_app_set_light_reflections.argtypes = [C.c_void_p, C.c_int]
        L.rtggx_app_set_light_sampling.argtypes = [C.c_void_p, C.c_int]
        L.rtggx_app_set_light_pick_visibility.argtypes = [C.c_void_p, C.c_int]
        L.rtggx_app_set_light_list.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.rtggx_app_set_light_list_visibility.argtypes = [C.c_void_p, C.c_int]
        L.rtggx_app_update_light_list.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        L.rtggx_app_update_light_list_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.rtggx_app_read_light_list.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.rtggx_app_last_screen_shot.argtypes = [C.c_void_p]
        L.rtggx_app_last_screen_shot.restype = C.c_char_p
        L.rtggx_host_obj_import.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p]
        L.rtggx_host_obj_copy.argtypes = [C.c_void_p, C.c_void_p]
        L.rtggx_host_halton.argtypes = [C.c_uint32, C.c_void_p]
        L.rtggx_host_frame_constants.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p]
        for n in ("rtggx_app_on_lbutton_down", "rtggx_app_on_lbutton_up", "rtggx_app_on_mouse_move"):
            getattr(L, n).argtypes = [C.c_void_p, C.c_float, C.c_float]
            getattr(L, n).restype = None
        L.rtggx_app_on_mouse_wheel.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
        L.rtggx_app_on_mouse_wheel.restype = None
        L.rtggx_app_load_track.argtypes = [C.c_void_p, C.c_char_p]
        L.rtggx_host_camera.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.rtggx_host_camera.restype = None
        L.rtggx_host_frame_indices.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        L.rtggx_host_frame_indices.restype = C.c_uint32
        L.rtggx_host_write_png.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        _lib = L
    return _lib


def obj_import(path):
    """ObjLoader::Import of the product's host layer -> (verts[nv,6], indices[ni], aabb[6])."""
    L = load()
    nv, ni = C.c_uint32(), C.c_uint32()
    aabb = np.zeros(6, np.float32)
    if L.rtggx_host_obj_import(path.encode(), C.byref(nv), C.byref(ni), aabb.ctypes.data_as(C.c_void_p)) != 0:
        raise IOError(L.rtggx_app_last_error().decode())
    v = np.zeros((nv.value, 6), np.float32)
    i = np.zeros(ni.value, np.uint32)
    L.rtggx_host_obj_copy(v.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p))
    return v, i, aabb


def camera(width, height, events):
    """The camera handlers on their own: events = [(type, a, b)], type 1 down, 2 up, 3 move, 4 wheel -> (eye[3], view[4, 4])."""
    ev = np.ascontiguousarray(np.asarray(events, np.float32).reshape(-1, 3))
    eye, view = np.zeros(3, np.float32), np.zeros((4, 4), np.float32)
    load().rtggx_host_camera(C.c_uint32(width), C.c_uint32(height), ev.ctypes.data_as(C.c_void_p), C.c_uint32(len(ev)),
                             eye.ctypes.data_as(C.c_void_p), view.ctypes.data_as(C.c_void_p))
    return eye, view


def halton(n):
    xy = np.zeros((n, 2), np.float32)
    load().rtggx_host_halton(n, xy.ctypes.data_as(C.c_void_p))
    return xy


def frame_constants(width, height, frames, dt=1.0 / 60.0, pos_scale=(0, 0, 0, 1), eye=(10.0, 10.0, -24.0), focus=(0.0, 3.0, 0.0)):
    """RayTracer::UpdateFrame of the host layer for `frames` consecutive frames -> uint8[frames, 768]."""
    out = np.zeros((frames, 768), np.uint8)
    ps, e, f = (np.asarray(a, np.float32) for a in (pos_scale, eye, focus))
    load().rtggx_host_frame_constants(width, height, ps.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p),
                                      f.ctypes.data_as(C.c_void_p), dt, frames, out.ctypes.data_as(C.c_void_p))
    return out


def frame_indices(sample_set, frames):
    """RayTracer::SetSampleSetSize(sample_set) and `frames` consecutive UpdateFrame calls of the host layer -> (the size the RayTracer holds
    -- 256 where the setter refused --, FrameIndex[frames])."""
    out = np.zeros(frames, np.uint32)
    held = load().rtggx_host_frame_indices(int(sample_set), frames, out.ctypes.data_as(C.c_void_p))
    return held, out


def write_pfm(path, rgba16f):
    """The host layer's PFM writer (no device): rgba16f = uint16[H, W, 4] (or uint64[H, W]) RGBA16F words -> "PF", fp32 rgb, rows bottom to top."""
    a = np.ascontiguousarray(rgba16f)
    if a.dtype == np.uint64:
        a = a.view(np.uint16).reshape(a.shape[0], a.shape[1], 4)
    a = np.ascontiguousarray(a, np.uint16)
    if load().rtggx_host_write_pfm(str(path).encode(), a.shape[1], a.shape[0], a.ctypes.data_as(C.c_void_p)) != 0:
        raise IOError("cannot write " + str(path))


def read_pfm(path, width, height):
    """The host layer's PFM reader (no device) -> uint16[height, width, 4] RGBA16F words, every fp32 value rounded to nearest even, alpha 1.
    Raises IOError for what the reader refuses: a missing, malformed or truncated file, another size, a non-negative scale."""
    L = load()
    out = np.zeros((height, width, 4), np.uint16)
    if L.rtggx_host_read_pfm(str(path).encode(), int(width), int(height), out.ctypes.data_as(C.c_void_p)) != 0:
        raise IOError(L.rtggx_app_last_error().decode())
    return out


def load_env_image(path):
    """The host layer's Radiance .hdr / .pfm readers (no device; told apart by the file's first bytes) -> (pixels, layout, image): pixels
    capi.PIXELS_RGBE8 with image uint8[H, W, 4] or capi.PIXELS_RGB32F with image float32[H, W, 3], rows top to bottom; layout what the aspect
    ratio tells (capi.ENV_EQUIRECT / ENV_VCROSS / ENV_HCROSS) or -1.  Raises IOError with the reader's reason for what it refuses."""
    L = load()
    px, lay, w, h, n = C.c_int(), C.c_int(), C.c_uint32(), C.c_uint32(), C.c_size_t()
    if L.rtggx_host_load_env_image(str(path).encode(), C.byref(px), C.byref(w), C.byref(h), C.byref(lay), None, 0, C.byref(n)) != 0:
        raise IOError(L.rtggx_app_last_error().decode())
    raw = np.zeros(n.value, np.uint8)
    if L.rtggx_host_load_env_image(str(path).encode(), None, None, None, None, raw.ctypes.data_as(C.c_void_p), raw.size, None) != 0:
        raise IOError(L.rtggx_app_last_error().decode())
    image = raw.reshape(h.value, w.value, 4) if px.value == capi.PIXELS_RGBE8 else raw.view(np.float32).reshape(h.value, w.value, 3)
    return px.value, lay.value, image


def accumulation_note(frames, samples, sample_set):
    """What the line -accumulate prints says about the sample set after `frames` frames of `samples` samples (no device)."""
    L = load()
    buf = C.create_string_buffer(512)
    L.rtggx_host_accumulation_note.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_int]
    if L.rtggx_host_accumulation_note(int(frames), int(samples), int(sample_set), buf, 512) < 0:
        raise ValueError("rtggx_host_accumulation_note: capacity")
    return buf.value.decode()


class BorrowedContext(capi.Context):
    """capi.Context view of the rtggx_context owned by a RayTracedGGX application object."""

    def __init__(self, handle, width, height):  # pylint: disable=super-init-not-called
        self.L = capi.load()
        self.W, self.H = width, height
        self.h = C.c_void_p(handle)

    def close(self):
        self.h = None


class RayTracedGGX:
    """The reference's application object, headless: RayTracedGGX(args).OnUpdate()/OnRender()."""

    def __init__(self, args):
        self.L = load()
        argv = [b"RayTracedGGX"] + [str(a).encode() for a in args]
        arr = (C.c_char_p * len(argv))(*argv)
        self.h = self.L.rtggx_app_create(len(argv), arr)
        if not self.h:
            raise capi.RtggxError("RayTracedGGX::OnInit failed: " + self.L.rtggx_app_last_error().decode())
        w, h = C.c_uint32(), C.c_uint32()
        self.L.rtggx_app_size(self.h, C.byref(w), C.byref(h))
        self.width, self.height = w.value, h.value
        self.context = BorrowedContext(self.L.rtggx_app_context(self.h), self.width, self.height)

    def OnUpdate(self):
        self.L.rtggx_app_on_update(self.h)

    def OnRender(self):
        self.L.rtggx_app_on_render(self.h)

    def OnKeyUp(self, key):
        self.L.rtggx_app_on_key_up(self.h, int(key))

    # the sample's camera interactions (RayTracedGGX.cpp:400-455), positions in pixels
    def OnLButtonDown(self, x, y):
        self.L.rtggx_app_on_lbutton_down(self.h, x, y)

    def OnLButtonUp(self, x, y):
        self.L.rtggx_app_on_lbutton_up(self.h, x, y)

    def OnMouseMove(self, x, y):
        self.L.rtggx_app_on_mouse_move(self.h, x, y)

    def OnMouseWheel(self, dz, x=0.0, y=0.0):
        self.L.rtggx_app_on_mouse_wheel(self.h, dz, x, y)

    def load_track(self, path):
        return self.L.rtggx_app_load_track(self.h, path.encode()) == 0

    def set_time_step(self, dt):
        self.L.rtggx_app_set_time_step(self.h, dt)

    def frame_constants(self):
        b = np.zeros(768, np.uint8)
        self.L.rtggx_app_frame_constants(self.h, b.ctypes.data_as(C.c_void_p))
        return b

    def save_image(self, path):
        return self.L.rtggx_app_save_image(self.h, path.encode()) == 0

    def save_converged(self, path):
        """The mean of the accumulated frames (-accumulate N, or context.set_accumulation) presented and its tone map written to `path`;
        prints the frame count and the mean relative standard error of Y.  False when nothing was accumulated."""
        return self.L.rtggx_app_save_converged(self.h, path.encode()) == 0

    def save_reference(self, path):
        """BUF_CONVERGED as the last save_converged / present_accumulation left it, written as a PFM file (-savereference)."""
        return self.L.rtggx_app_save_reference(self.h, path.encode()) == 0

    def set_reference(self, rgba16f):
        """RayTracer::SetReference: H x W RGBA16F words (uint64[H, W] as readback(BUF_CONVERGED) gives them); None releases the image."""
        if rgba16f is None:
            rc = self.L.rtggx_app_set_reference(self.h, None, 0)
        else:
            a = np.ascontiguousarray(rgba16f)
            rc = self.L.rtggx_app_set_reference(self.h, a.ctypes.data_as(C.c_void_p), a.nbytes)
        if rc != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def reference_from_accumulation(self):
        self.context.reference_from_accumulation()

    def set_sample_map(self, counts):
        """RayTracer::SetSampleMap: uint8[ceil(H / 8), ceil(W / 8)] counts (1, 2, 4 or 8) of the -spp N samples each 8x8 block traces, from the
        next frame on; None clears the map."""
        if counts is None:
            rc = self.L.rtggx_app_set_sample_map(self.h, None, 0, 0)
        else:
            a = np.ascontiguousarray(counts, np.uint8)
            rc = self.L.rtggx_app_set_sample_map(self.h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0])
        if rc != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def set_lights(self, lights):
        """RayTracer::SetLights: a sequence of capi.Light (or dicts of capi.Light.of's arguments) from the next frame on; None or empty: off."""
        lights = [l if isinstance(l, capi.Light) else capi.Light.of(**l) for l in (lights or ())]
        a = (capi.Light * len(lights))(*lights) if lights else None
        if self.L.rtggx_app_set_lights(self.h, a, len(lights)) != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def set_light_reflections(self, on):
        """RayTracer::SetLightReflections: the lights at the surfaces the paths hit as well, from the next frame on (0 or 1)."""
        if self.L.rtggx_app_set_light_reflections(self.h, int(on)) != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def set_light_sampling(self, mode):
        """RayTracer::SetLightSampling: 0 a shadow ray per light, 1 one per surface point for all lights, from the next frame on."""
        if self.L.rtggx_app_set_light_sampling(self.h, int(mode)) != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def set_light_list(self, lights):
        """RayTracer::SetLightList: a list of up to capi.MAX_LIGHT_LIST lights (capi.Light, or dicts with its arguments) under mode 1's
        rule from the next frame on; None or an empty sequence clears it."""
        lights = [l if isinstance(l, capi.Light) else capi.Light.of(**l) for l in (lights or ())]
        a = (capi.Light * len(lights))(*lights) if lights else None
        if self.L.rtggx_app_set_light_list(self.h, a, len(lights)) != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def update_light_list(self, lights, first=0):
        """RayTracer::UpdateLightList: lights first .. of the list replaced from the next frame on; no wait, the records' history kept."""
        lights = [l if isinstance(l, capi.Light) else capi.Light.of(**l) for l in lights]
        a = (capi.Light * len(lights))(*lights) if lights else None
        if self.L.rtggx_app_update_light_list(self.h, a, int(first), len(lights)) != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def update_light_list_device(self, ptr, first, count, kinds, stream=0):
        """RayTracer::UpdateLightListDevice: the same from device memory, read in the order of `stream` and checked on the device."""
        if self.L.rtggx_app_update_light_list_device(self.h, C.c_void_p(int(ptr)), int(first), int(count), int(kinds), C.c_void_p(int(stream) or None)) != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def read_light_list(self, count):
        """RayTracer::ReadLightList: the `count` lights the last frame read as the kernels see them, float32 [count, 16].  Synchronises."""
        a = np.zeros((int(count), 16), np.float32)
        if self.L.rtggx_app_read_light_list(self.h, a.ctypes.data_as(C.c_void_p), a.nbytes) != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())
        return a

    def set_light_pick_visibility(self, enable):
        """RayTracer::SetLightPickVisibility: the pick of mode 1 weighted by the visibility each pixel remembers (0 / 1), from the next frame on."""
        if self.L.rtggx_app_set_light_pick_visibility(self.h, int(enable)) != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def set_light_list_visibility(self, enable):
        """RayTracer::SetLightListVisibility: the list's pick weighted by the sparse record each pixel keeps (0 / 1), from the next frame on."""
        if self.L.rtggx_app_set_light_list_visibility(self.h, int(enable)) != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def set_scoring(self, enable):
        """RayTracer::SetScoring: every frame from the next one on is scored against the reference; refused without one."""
        if self.L.rtggx_app_set_scoring(self.h, 1 if enable else 0) != 0:
            raise capi.RtggxError(self.L.rtggx_app_last_error().decode())

    def read_scores(self, capacity=None):
        """RayTracer::ReadScores: the unread records, oldest first, as a list of dicts."""
        out = []
        while capacity is None or len(out) < capacity:
            room = capi.SCORE_RING if capacity is None else min(capi.SCORE_RING, capacity - len(out))
            buf, n = (capi.Score * room)(), C.c_uint32()
            if self.L.rtggx_app_read_scores(self.h, buf, room, C.byref(n)) != 0:
                raise capi.RtggxError(self.L.rtggx_app_last_error().decode())
            out += [buf[i].as_dict() for i in range(n.value)]
            if n.value < room:
                break
        return out

    def flush_scores(self):
        """Appends the unread records to the -score file as JSON lines (the executable does so every capi.SCORE_RING frames and at the end)."""
        return self.L.rtggx_app_flush_scores(self.h) == 0

    def set_dump_prefix(self, prefix):
        """Where [F11] screen shots go: <prefix>_f<frame>.png (the -dump flag)."""
        self.L.rtggx_app_set_dump_prefix(self.h, prefix.encode())

    def last_screen_shot(self):
        """The file the most recent [F11] (key code 0x7A, `key F11` in a -track script) wrote; '' if none."""
        return self.L.rtggx_app_last_screen_shot(self.h).decode()

    def OnDestroy(self):
        if self.h:
            self.context.close()
            self.L.rtggx_app_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.OnDestroy()
        except Exception:
            pass
