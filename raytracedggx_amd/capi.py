"""ctypes binding of librtggx.so -- the C ABI declared in include/rtggx.h.

The library is the product: hand-written HIP for gfx950 behind `extern "C"` entry points.  There is
no CPU fallback; loading fails loudly when the shared object is missing, and rtggx_create fails
when no HIP device is present.
"""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librtggx.so")

# buffer ids (rtggx.h)
BUF_VISIBILITY, BUF_DEPTH, BUF_NORMAL, BUF_ROUGH_METAL, BUF_VELOCITY, BUF_RT_REFL, BUF_RT_DIFF, BUF_TSS0, BUF_TSS1, \
    BUF_FLT_RFL, BUF_FLT_DFF, BUF_BACKBUFFER, BUF_SH_COEFFS, BUF_BVH_NODES0, BUF_BVH_TRIS0, BUF_BVH_NODES1, BUF_BVH_TRIS1, \
    BUF_TLAS, BUF_ENV, BUF_BVH4_NODES0, BUF_BVH4_NODES1, BUF_BIN_WORK, BUF_BVH4_TOP0, BUF_BVH4_TOP1, BUF_EXCHANGE_TOKENS, \
    BUF_ACC_REFL, BUF_ACC_DIFF, BUF_CONVERGED = range(28)
MAX_PEERS, IPC_HANDLE_BYTES = 16, 64
FORMAT_RGBA32F, FORMAT_RGBA16F, FORMAT_BC6H_UF16, FORMAT_BC6H_SF16 = 2, 10, 95, 96
ENV_EQUIRECT, ENV_VCROSS, ENV_HCROSS = 0, 1, 2      # layouts and pixel formats of rtggx_set_env_image
PIXELS_RGBE8, PIXELS_RGB32F = 0, 1
ENV_FILTER_MIN_SAMPLES, ENV_FILTER_MAX_SAMPLES = 64, 4096      # rtggx_prefilter_env
MAX_SUN_ANGLE_DEGREES = 10.0                                    # rtggx_set_sun_angle
MAX_LIGHTS = 8                                                  # rtggx_set_lights
MAX_LIGHT_LIST = 1024                                           # rtggx_set_light_list
LIGHT_KIND_RADIUS, LIGHT_KIND_CONE = 1, 2                       # rtggx_update_light_list_device's kinds

_BUF_DTYPE = {BUF_VISIBILITY: np.uint32, BUF_DEPTH: np.uint32, BUF_NORMAL: np.uint32, BUF_ROUGH_METAL: np.uint16,
              BUF_VELOCITY: np.uint32, BUF_RT_REFL: np.uint32, BUF_RT_DIFF: np.uint32, BUF_TSS0: np.uint64, BUF_TSS1: np.uint64,
              BUF_FLT_RFL: np.uint64, BUF_FLT_DFF: np.uint64, BUF_BACKBUFFER: np.uint32, BUF_SH_COEFFS: np.float32,
              BUF_BVH_NODES0: np.uint32, BUF_BVH_TRIS0: np.uint32, BUF_BVH_NODES1: np.uint32, BUF_BVH_TRIS1: np.uint32,
              BUF_TLAS: np.float32, BUF_ENV: np.uint16, BUF_BVH4_NODES0: np.uint32, BUF_BVH4_NODES1: np.uint32, BUF_BIN_WORK: np.uint32,
              BUF_BVH4_TOP0: np.uint32, BUF_BVH4_TOP1: np.uint32, BUF_EXCHANGE_TOKENS: np.uint32,
              BUF_ACC_REFL: np.float32, BUF_ACC_DIFF: np.float32, BUF_CONVERGED: np.uint64}

EXPORTS = ["rtggx_last_error", "rtggx_create", "rtggx_destroy", "rtggx_set_strip", "rtggx_set_stream", "rtggx_set_mesh",
           "rtggx_set_env", "rtggx_set_material", "rtggx_set_metallic", "rtggx_build_as", "rtggx_update_frame", "rtggx_update_as",
           "rtggx_transform_sh", "rtggx_render_visibility", "rtggx_ray_trace", "rtggx_denoise", "rtggx_tone_map", "rtggx_sync",
           "rtggx_ray_count", "rtggx_get_timings", "rtggx_enable_timing", "rtggx_buffer_size", "rtggx_readback", "rtggx_buffer_ptr",
           "rtggx_upload", "rtggx_frame_parity", "rtggx_bvh_root", "rtggx_trace_rays", "rtggx_ray_total", "rtggx_kernel_times", "rtggx_debug_counters", "rtggx_debug_trace_split", "rtggx_debug_trace_residency", "rtggx_get_stream", "rtggx_set_history_peers", "rtggx_history_ipc_export", "rtggx_history_ipc_open",
           "rtggx_set_async_compute", "rtggx_set_history_apron", "rtggx_history_overreach", "rtggx_copy_bandwidth", "rtggx_refit_as", "rtggx_refit_as_device", "rtggx_refit_stats", "rtggx_set_refit_policy", "rtggx_set_sampler", "rtggx_set_ray_rate", "rtggx_set_max_recursion_depth", "rtggx_set_samples_per_pixel", "rtggx_debug_fuse_tone_map", "rtggx_debug_placement", "rtggx_debug_tile_words", "rtggx_debug_static_sky", "rtggx_debug_settled_sky", "rtggx_debug_settled_words", "rtggx_debug_sky_runs", "rtggx_debug_collapse_weights", "rtggx_debug_fence_wait", "rtggx_debug_shader_clock", "rtggx_debug_environment",
           "rtggx_set_accumulation", "rtggx_reset_accumulation", "rtggx_accumulated_frames", "rtggx_present_accumulation", "rtggx_set_sample_set",
           "rtggx_set_reference", "rtggx_reference_from_accumulation", "rtggx_set_scoring", "rtggx_read_scores",
           "rtggx_set_env_image", "rtggx_generate_env_mips", "rtggx_prefilter_env",
           "rtggx_set_sample_map", "rtggx_read_sample_map", "rtggx_trace_occlusion", "rtggx_set_sun", "rtggx_set_sun_reflections",
           "rtggx_sun_from_env", "rtggx_set_sun_angle", "rtggx_set_lights", "rtggx_set_light_reflections", "rtggx_set_light_sampling",
           "rtggx_set_light_pick_visibility", "rtggx_read_light_visibility",
           "rtggx_set_light_list", "rtggx_read_light_list_counts", "rtggx_debug_light_list_cull",
           "rtggx_set_light_list_visibility", "rtggx_read_light_list_visibility",
           "rtggx_update_light_list", "rtggx_update_light_list_device", "rtggx_read_light_list", "rtggx_read_light_list_rejects",
           "rtggx_debug_visibility_drains"]
SCORE_RING = 256


class Timings(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("update_as", "visibility", "ray_trace", "spatial_refl_h", "spatial_refl_v",
                                         "spatial_diff_h", "spatial_diff_v", "temporal", "tone_map", "frame", "ray_trace_kernel")]


class Score(C.Structure):
    """RtggxScore (rtggx.h): one scored frame -- counts, then nine fp64 sums in the contract's pairwise order."""
    _fields_ = [("index", C.c_uint64), ("frame_index", C.c_uint32), ("pad", C.c_uint32), ("pixels", C.c_uint64), ("covered", C.c_uint64),
                ("skipped_out", C.c_uint64), ("skipped_raw", C.c_uint64)] + \
               [(n, C.c_double) for n in ("se_out_rgb", "se_out_luma", "se_raw_rgb", "se_raw_luma", "ref_rgb2", "ref_luma2",
                                          "se_out_rgb_cov", "se_raw_rgb_cov", "ref_rgb2_cov")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "pad"}


class SunEstimate(C.Structure):
    """RtggxSunEstimate (rtggx.h): what rtggx_sun_from_env found -- the masks' squared cosines, the peak, the fp64 sums in the contract's
    pairwise order, the background and its binary16 rounding, direction and irradiance for set_sun, the counts."""
    _fields_ = [(n, C.c_double) for n in ("cos2_cone", "cos2_ring", "peak_luma", "mean_luma", "weight_all", "weight_cone", "weight_ring")] + \
               [(n, C.c_double * 3) for n in ("ring_rgb", "background", "excess", "moment")] + \
               [(n, C.c_float * 3) for n in ("background_half", "direction", "irradiance")] + \
               [(n, C.c_uint32) for n in ("found", "removed", "peak_face", "peak_x", "peak_y", "texels_cone", "texels_ring", "texels_lit", "pad")]

    def as_dict(self):
        """Scalars as Python numbers, the triples as numpy arrays of their own type; "bytes": the record as it lies in memory."""
        out = {"bytes": bytes(self)}
        for n, t in self._fields_:
            if n != "pad":
                v = getattr(self, n)
                out[n] = v if t in (C.c_double, C.c_uint32) else np.array(list(v), np.float64 if t == C.c_double * 3 else np.float32)
        return out


class Light(C.Structure):
    """RtggxLight (rtggx.h), 64 bytes: a point light, or with cos_outer > -1 a spot along `axis`; radius > 0: an emitting sphere."""
    _fields_ = [("position", C.c_float * 3), ("range", C.c_float), ("intensity", C.c_float * 3), ("radius", C.c_float),
                ("axis", C.c_float * 3), ("cos_outer", C.c_float), ("cos_inner", C.c_float), ("pad", C.c_float * 3)]

    @classmethod
    def of(cls, position, intensity, range, radius=0.0, axis=(0.0, 0.0, 0.0), cos_outer=-1.0, cos_inner=1.0):
        return cls((C.c_float * 3)(*position), range, (C.c_float * 3)(*intensity), radius, (C.c_float * 3)(*axis), cos_outer, cos_inner)


LIGHT_VIS_FLOOR = 16      # RTGGX_LIGHT_VIS_FLOOR
# RtggxLightVisRecord (rtggx.h), 16 bytes: eight visibility bytes, the pixel's normal word, the stamp
LIGHT_VIS_RECORD = np.dtype([("v", np.uint8, 8), ("normal", np.uint32), ("stamp", np.uint32)])
LIGHT_LIST_VIS_ENTRIES, LIGHT_LIST_VIS_FLOOR = 4, 4      # RTGGX_LIGHT_LIST_VIS_ENTRIES, RTGGX_LIGHT_LIST_VIS_FLOOR
# RtggxLightListVisRecord (rtggx.h), 16 bytes: four entries (v << 10) | light (0xFFFF: free), the pixel's normal word, the stamp
LIGHT_LIST_VIS_RECORD = np.dtype([("entry", np.uint16, 4), ("normal", np.uint32), ("stamp", np.uint32)])

_lib = None


def load():
    """Load librtggx.so; raises if the HIP library has not been built (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("librtggx.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C raytracedggx_amd` (hipcc, gfx950). There is no CPU path.")
    L = C.CDLL(LIB_PATH)
    L.rtggx_last_error.restype = C.c_char_p
    vp = C.c_void_p
    L.rtggx_create.argtypes = [C.POINTER(vp), C.c_uint32, C.c_uint32, C.c_int]
    L.rtggx_destroy.argtypes = [vp]
    L.rtggx_destroy.restype = None
    L.rtggx_set_strip.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.rtggx_set_stream.argtypes = [vp, vp]
    L.rtggx_set_async_compute.argtypes = [vp, C.c_int]
    L.rtggx_set_ray_rate.argtypes = [vp, C.c_uint32]
    L.rtggx_set_max_recursion_depth.argtypes = [vp, C.c_uint32]
    L.rtggx_set_samples_per_pixel.argtypes = [vp, C.c_uint32]
    L.rtggx_set_sample_set.argtypes = [vp, C.c_uint32]
    L.rtggx_set_accumulation.argtypes = [vp, C.c_int]
    L.rtggx_reset_accumulation.argtypes = [vp]
    L.rtggx_accumulated_frames.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.rtggx_present_accumulation.argtypes = [vp]
    L.rtggx_set_reference.argtypes = [vp, vp, C.c_size_t]
    L.rtggx_reference_from_accumulation.argtypes = [vp]
    L.rtggx_set_scoring.argtypes = [vp, C.c_int]
    L.rtggx_read_scores.argtypes = [vp, C.POINTER(Score), C.c_uint32, C.POINTER(C.c_uint32)]
    L.rtggx_set_sample_map.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.rtggx_read_sample_map.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.rtggx_set_history_apron.argtypes = [vp, C.c_uint32]
    L.rtggx_debug_shader_clock.argtypes = [vp, C.POINTER(C.c_double)]
    L.rtggx_refit_as.argtypes = [vp, C.c_uint32, vp, C.c_uint32]
    L.rtggx_set_refit_policy.argtypes = [vp, C.c_float, C.c_uint32]
    L.rtggx_refit_stats.argtypes = [vp, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.rtggx_copy_bandwidth.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    L.rtggx_history_overreach.argtypes = [vp, C.POINTER(C.c_uint32), C.c_int]
    L.rtggx_set_mesh.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32]
    L.rtggx_set_env.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, vp, C.c_size_t]
    L.rtggx_set_env_image.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, vp, C.c_size_t, C.c_uint32]
    L.rtggx_generate_env_mips.argtypes = [vp]
    L.rtggx_prefilter_env.argtypes = [vp, C.c_uint32]
    L.rtggx_set_material.argtypes = [vp, C.c_uint32, vp, C.c_float, C.c_float]
    L.rtggx_set_metallic.argtypes = [vp, C.c_uint32, C.c_float]
    for n in ("rtggx_build_as", "rtggx_update_as", "rtggx_transform_sh", "rtggx_render_visibility", "rtggx_ray_trace",
              "rtggx_tone_map", "rtggx_sync"):
        getattr(L, n).argtypes = [vp]
    L.rtggx_update_frame.argtypes = [vp, vp]
    L.rtggx_denoise.argtypes = [vp, C.c_int]
    L.rtggx_ray_count.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.rtggx_get_timings.argtypes = [vp, C.POINTER(Timings)]
    L.rtggx_enable_timing.argtypes = [vp, C.c_int]
    L.rtggx_buffer_size.argtypes = [vp, C.c_int, C.POINTER(C.c_size_t)]
    L.rtggx_readback.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.rtggx_buffer_ptr.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.rtggx_upload.argtypes = [vp, C.c_int, vp, C.c_size_t]
    L.rtggx_frame_parity.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.rtggx_bvh_root.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int32)]
    L.rtggx_trace_rays.argtypes = [vp, vp, C.c_uint32, vp]
    L.rtggx_trace_occlusion.argtypes = [vp, vp, C.c_uint32, vp]
    L.rtggx_set_sun.argtypes = [vp, vp, vp]
    L.rtggx_set_sun_reflections.argtypes = [vp, C.c_int]
    L.rtggx_set_sun_angle.argtypes = [vp, C.c_float]
    L.rtggx_set_lights.argtypes = [vp, C.POINTER(Light), C.c_uint32]
    L.rtggx_set_light_reflections.argtypes = [vp, C.c_int]
    L.rtggx_set_light_sampling.argtypes = [vp, C.c_int]
    L.rtggx_set_light_pick_visibility.argtypes = [vp, C.c_int]
    L.rtggx_read_light_visibility.argtypes = [vp, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_uint32)]
    L.rtggx_set_light_list.argtypes = [vp, C.POINTER(Light), C.c_uint32]
    L.rtggx_read_light_list_counts.argtypes = [vp, vp, C.c_size_t]
    L.rtggx_debug_light_list_cull.argtypes = [vp, C.c_int]
    L.rtggx_set_light_list_visibility.argtypes = [vp, C.c_int]
    L.rtggx_read_light_list_visibility.argtypes = [vp, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_uint32)]
    L.rtggx_update_light_list.argtypes = [vp, C.POINTER(Light), C.c_uint32, C.c_uint32]
    L.rtggx_update_light_list_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.rtggx_read_light_list.argtypes = [vp, vp, C.c_size_t]
    L.rtggx_read_light_list_rejects.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.rtggx_debug_visibility_drains.argtypes = [vp, C.POINTER(C.c_uint32), C.c_int]
    L.rtggx_sun_from_env.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_int, C.POINTER(SunEstimate)]
    L.rtggx_ray_total.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
    L.rtggx_kernel_times.argtypes = [vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]
    _lib = L
    return L


class RtggxError(RuntimeError):
    pass


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One rtggx_context: scene + render targets on one GPU.  Method names follow rtggx.h."""

    def __init__(self, width, height, device=0):
        self.L = load()
        self.W, self.H = int(width), int(height)
        h = C.c_void_p()
        self._check(self.L.rtggx_create(C.byref(h), self.W, self.H, int(device)))
        self.h = h

    def _check(self, rc):
        if rc != 0:
            raise RtggxError("librtggx: %s (code %d)" % (self.L.rtggx_last_error().decode(), rc))

    def close(self):
        if getattr(self, "h", None):
            self.L.rtggx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_strip(self, row_begin, row_end):
        self._check(self.L.rtggx_set_strip(self.h, row_begin, row_end))

    def set_stream(self, stream_handle):
        self._check(self.L.rtggx_set_stream(self.h, C.c_void_p(stream_handle)))

    def shader_clock_mhz(self):
        m = C.c_double()
        self._check(self.L.rtggx_debug_shader_clock(self.h, C.byref(m)))
        return m.value

    def copy_bandwidth(self, nbytes=1 << 30, iterations=8):
        """GB/s (read + written) of a float4 copy kernel over two buffers of nbytes each: the attainable HBM peak on this box."""
        g = C.c_double()
        self._check(self.L.rtggx_copy_bandwidth(self.h, int(nbytes), int(iterations), C.byref(g)))
        return g.value

    def set_history_apron(self, rows):
        self._check(self.L.rtggx_set_history_apron(self.h, int(rows)))

    def history_overreach(self, reset=True):
        """Rows by which a history tap read beyond the delivered apron since the last reset (strips; 0 = exact)."""
        n = C.c_uint32()
        self._check(self.L.rtggx_history_overreach(self.h, C.byref(n), int(reset)))
        return n.value

    def set_async_compute(self, enable):
        self._check(self.L.rtggx_set_async_compute(self.h, int(bool(enable))))

    def set_mesh(self, slot, verts, indices):
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 6)
        i = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        self._check(self.L.rtggx_set_mesh(self.h, slot, _p(v), v.shape[0], _p(i), i.size))

    def refit_as(self, slot, verts):
        """New vertex positions / normals for an unchanged topology: staged now, uploaded and refitted on stream B by the next frame."""
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 6)
        self._check(self.L.rtggx_refit_as(self.h, slot, _p(v), v.shape[0]))

    def refit_as_device(self, slot, device_ptr, num_verts, stream=0):
        """New vertices from DEVICE memory (a mesh animated on the GPU): ordered on `stream` like a hipMemcpyAsync out of the buffer."""
        self.L.rtggx_refit_as_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        self._check(self.L.rtggx_refit_as_device(self.h, slot, C.c_void_p(int(device_ptr)), int(num_verts), C.c_void_p(int(stream) or None)))

    def fence_wait(self, reset=True):
        """(us the host has waited at the frames-in-flight fence, frames that waited) since the last reset (diagnostic)."""
        us, n = C.c_double(0.0), C.c_uint32(0)
        self.L.rtggx_debug_fence_wait.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_int]
        self._check(self.L.rtggx_debug_fence_wait(self.h, C.byref(us), C.byref(n), 1 if reset else 0))
        return us.value, n.value

    def fuse_tone_map(self, mode):
        """True / False: the temporal pass always / never tone-maps its result as well; None: the library's choice (small launches) (diagnostic)."""
        self._check(self.L.rtggx_debug_fuse_tone_map(self.h, -1 if mode is None else 1 if mode else 0))

    def tile_words(self, enable):
        """False: every 16x16 tile of the visibility target counts as drawn (rounds 1-3); True: the tiles' words decide (diagnostic)."""
        self._check(self.L.rtggx_debug_tile_words(self.h, 1 if enable else 0))

    def static_sky(self, enable):
        """False: ray generation and the reflection V pass leave no tile alone for having been sky in the frames before (diagnostic)."""
        self._check(self.L.rtggx_debug_static_sky(self.h, 1 if enable else 0))

    def sky_runs(self):
        """(runs[tiles_y, tiles_x], threshold): per 16x16 tile of the most recent ray generation the consecutive frames it has had no surface
        under the current epoch, and the run from which that ray generation left a tile alone (diagnostic; synchronises)."""
        tiles = ((self.W + 15) // 16) * ((self.H + 15) // 16 + 1)
        runs = np.zeros(tiles, np.uint32)
        tx, ty, th = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self.L.rtggx_debug_sky_runs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.L.rtggx_debug_sky_runs(self.h, _p(runs), tiles, C.byref(tx), C.byref(ty), C.byref(th)))
        return runs[:tx.value * ty.value].reshape(ty.value, tx.value), int(th.value)

    def settled_sky(self, enable):
        """False: the temporal pass keeps no settled words, and neither it nor the tone map leaves a block over settled sky alone (diagnostic)."""
        self.L.rtggx_debug_settled_sky.argtypes = [C.c_void_p, C.c_int]
        self._check(self.L.rtggx_debug_settled_sky(self.h, 1 if enable else 0))

    def settled_words(self):
        """(words[2, blocks_y, blocks_x], epoch): per history parity and 64x4 block of the temporal pass `epoch << 8 | bit 0 settled | bit 1
        left alone`, and the epoch words count under now (diagnostic; synchronises)."""
        n = ((self.W + 63) // 64) * ((self.H + 3) // 4)
        w = np.zeros((2, n), np.uint32)
        bx, by, ep = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self.L.rtggx_debug_settled_words.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        self._check(self.L.rtggx_debug_settled_words(self.h, _p(w[0]), _p(w[1]), n, C.byref(bx), C.byref(by), C.byref(ep)))
        return np.ascontiguousarray(w.reshape(2, bx.value, by.value).transpose(0, 2, 1)), int(ep.value)

    def placement(self, force_small=-1):
        """Pins the `small launch` fact of the stream placement (0 / 1; -1: by the ray count) and returns the key and placement of the most
        recent ray_trace: ({small, strip, deforming, diffuse, caller_stream}, {gen, trace, shade: "main" | "B" | "C" | "R", frames_in_flight})."""
        k, w = C.c_uint32(), C.c_uint32()
        self.L.rtggx_debug_placement.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self._check(self.L.rtggx_debug_placement(self.h, int(force_small), C.byref(k), C.byref(w)))
        names = ("main", "B", "C", "R", "?")
        key = {n: bool((k.value >> i) & 1) for i, n in enumerate(("small", "strip", "deforming", "diffuse", "caller_stream"))}
        where = {"raster": names[(w.value >> 16) & 15], "gen": names[w.value & 15], "trace": names[(w.value >> 4) & 15], "shade": names[(w.value >> 8) & 15], "frames_in_flight": (w.value >> 12) & 15}
        return key, where

    def collapse_weights(self, area=None, tris=None):
        """(area weight, triangle-count weight) of the 4-wide collapse's objective; given both, sets them for builds from now on (diagnostic)."""
        self.L.rtggx_debug_collapse_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        get = (C.c_float * 2)()
        if area is not None:
            st = (C.c_float * 2)(float(area), float(tris))
            self._check(self.L.rtggx_debug_collapse_weights(self.h, st, get))
        else:
            self._check(self.L.rtggx_debug_collapse_weights(self.h, None, get))
        return float(get[0]), float(get[1])

    def set_history_peers(self, bounds, tss0, tss1):
        """Multi-GPU strips: every rank's TemporalSSOut[0] / [1] as device pointers valid in this process (0: this rank's own), and the
        strip boundaries (world + 1 rows) -- history taps beyond the exchanged apron then read the owner's image.  bounds=None: forget them."""
        self.L.rtggx_set_history_peers.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        if bounds is None:
            self._check(self.L.rtggx_set_history_peers(self.h, 0, None, None, None))
            return
        world = len(bounds) - 1
        b = (C.c_uint32 * (world + 1))(*[int(x) for x in bounds])
        p0 = (C.c_void_p * world)(*[C.c_void_p(int(x) or None) for x in tss0])
        p1 = (C.c_void_p * world)(*[C.c_void_p(int(x) or None) for x in tss1])
        self._check(self.L.rtggx_set_history_peers(self.h, world, b, p0, p1))

    def history_ipc_export(self):
        """This context's two history images as inter-process handles (2 x 64 bytes) for another process's history_ipc_open."""
        self.L.rtggx_history_ipc_export.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        buf = C.create_string_buffer(2 * IPC_HANDLE_BYTES)
        self._check(self.L.rtggx_history_ipc_export(self.h, buf, len(buf.raw)))
        return bytes(buf.raw)

    def history_ipc_open(self, handles):
        """Another process's history_ipc_export opened here: (TemporalSSOut[0], TemporalSSOut[1]) device pointers for set_history_peers."""
        self.L.rtggx_history_ipc_open.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
        p0, p1 = C.c_void_p(), C.c_void_p()
        self._check(self.L.rtggx_history_ipc_open(self.h, bytes(handles), len(handles), C.byref(p0), C.byref(p1)))
        return int(p0.value), int(p1.value)

    def set_sampler(self, vndf):
        self._check(self.L.rtggx_set_sampler(self.h, 1 if vndf else 0))

    def set_ray_rate(self, pixels_per_ray):
        """1 (default) or 4: one pixel of each 2x2 quad traced per frame, the others reconstructed (include/rtggx.h); synchronises."""
        self._check(self.L.rtggx_set_ray_rate(self.h, int(pixels_per_ray)))

    def set_max_recursion_depth(self, depth):
        """1 (default) to 4 levels of rays per path (include/rtggx.h); taken over by the next frame."""
        self._check(self.L.rtggx_set_max_recursion_depth(self.h, int(depth)))

    def set_samples_per_pixel(self, samples):
        """1 (default), 2, 4 or 8 samples per covered pixel (include/rtggx.h); taken over by the next frame; not together with ray rate 4."""
        self._check(self.L.rtggx_set_samples_per_pixel(self.h, int(samples)))

    def set_sample_set(self, size):
        """The size of the sample set: 256 (default) or a power of two up to 65536 (include/rtggx.h); taken over by the next frame;
        synchronises.  The caller's FrameIndex should count modulo it."""
        self._check(self.L.rtggx_set_sample_set(self.h, int(size)))

    def set_accumulation(self, enable):
        """Progressive accumulation of the raw traced images (include/rtggx.h): on from the next frame; the first enable allocates 40 bytes
        per pixel; not together with ray rate 4.  Enabling does not reset, disabling keeps the sums and the count."""
        self._check(self.L.rtggx_set_accumulation(self.h, 1 if enable else 0))

    def reset_accumulation(self):
        """Sums and frame count back to zero, enqueued on the main stream (no wait)."""
        self._check(self.L.rtggx_reset_accumulation(self.h))

    def accumulated_frames(self):
        n = C.c_uint32()
        self._check(self.L.rtggx_accumulated_frames(self.h, C.byref(n)))
        return int(n.value)

    def present_accumulation(self):
        """BUF_CONVERGED = the mean of the accumulated frames, and its tone map in BUF_BACKBUFFER (whole frames, at least one frame)."""
        self._check(self.L.rtggx_present_accumulation(self.h))

    def set_reference(self, rgba16f):
        """The image every frame is scored against: H x W RGBA16F words as readback(BUF_CONVERGED) gives them (uint64[H, W], or any array of
        W * H * 8 bytes); None releases it and turns scoring off.  Synchronises; may replace a reference in mid-run (include/rtggx.h)."""
        if rgba16f is None:
            self._check(self.L.rtggx_set_reference(self.h, None, 0))
            return
        a = np.ascontiguousarray(rgba16f)
        self._check(self.L.rtggx_set_reference(self.h, _p(a), a.nbytes))

    def reference_from_accumulation(self):
        """The reference becomes the mean of the accumulated frames (present_accumulation's image) without touching the back buffer."""
        self._check(self.L.rtggx_reference_from_accumulation(self.h))

    def set_scoring(self, enable):
        """Every frame from the next one on is scored against the reference inside the frame; refused without a reference."""
        self._check(self.L.rtggx_set_scoring(self.h, 1 if enable else 0))

    def read_scores(self, capacity=None):
        """The unread records, oldest first, as a list of dicts (at most `capacity`; default: all of them).  Waits for the main stream only."""
        out = []
        while capacity is None or len(out) < capacity:
            room = SCORE_RING if capacity is None else min(SCORE_RING, capacity - len(out))
            buf, n = (Score * room)(), C.c_uint32()
            self._check(self.L.rtggx_read_scores(self.h, buf, room, C.byref(n)))
            out += [buf[i].as_dict() for i in range(n.value)]
            if n.value < room:
                break
        return out

    def set_sample_map(self, counts):
        """Adaptive sampling (include/rtggx.h): uint8[ceil(H / 8), ceil(W / 8)] counts -- 1, 2, 4 or 8 -- of the N samples each 8x8 block
        traces, from the next frame on; None clears the map.  Whole frames only; synchronises."""
        if counts is None:
            self._check(self.L.rtggx_set_sample_map(self.h, None, 0, 0))
            return
        a = np.ascontiguousarray(counts, np.uint8)
        if a.ndim != 2:
            raise ValueError("a sample map is a 2-d array of blocks")
        self._check(self.L.rtggx_set_sample_map(self.h, _p(a), a.shape[1], a.shape[0]))

    def read_sample_map(self):
        """The map most recently set, uint8[blocks_y, blocks_x], read back from the device; None when there is none."""
        a = np.zeros(((self.H + 7) // 8, (self.W + 7) // 8), np.uint8)
        bx, by = C.c_uint32(), C.c_uint32()
        self._check(self.L.rtggx_read_sample_map(self.h, _p(a), a.size, C.byref(bx), C.byref(by)))
        if bx.value == 0 and by.value == 0:
            return None
        assert (by.value, bx.value) == a.shape
        return a

    def set_refit_policy(self, rebuild_ratio=1.2, steps_per_frame=16):
        self._check(self.L.rtggx_set_refit_policy(self.h, rebuild_ratio, steps_per_frame))

    def refit_stats(self, slot=1):
        ratio, refits, rebuilds = C.c_float(), C.c_uint32(), C.c_uint32()
        self._check(self.L.rtggx_refit_stats(self.h, slot, C.byref(ratio), C.byref(refits), C.byref(rebuilds)))
        return {"cost_ratio": ratio.value, "refits": refits.value, "rebuilds": rebuilds.value}

    def set_env(self, fmt, size, mips, data):
        b = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self._check(self.L.rtggx_set_env(self.h, fmt, size, mips, _p(b), b.size))

    def set_env_image(self, layout, pixels, width, height, data, cube_size=0):
        """The cube and its full mip chain built on the device from an image (include/rtggx.h): layout ENV_EQUIRECT / ENV_VCROSS / ENV_HCROSS,
        pixels PIXELS_RGBE8 (uint8[H, W, 4]) or PIXELS_RGB32F (float32[H, W, 3]), rows top to bottom; cube_size for a panorama only (0: the
        largest power of two <= width / 4).  data=None passes a null pointer (refused, like everything the header lists)."""
        if data is None:
            self._check(self.L.rtggx_set_env_image(self.h, int(layout), int(pixels), int(width), int(height), None, 0, int(cube_size)))
            return
        b = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self._check(self.L.rtggx_set_env_image(self.h, int(layout), int(pixels), int(width), int(height), _p(b), b.size, int(cube_size)))

    def generate_env_mips(self):
        """The full mip chain below the current level 0 of the environment, rebuilt on the device (include/rtggx.h)."""
        self._check(self.L.rtggx_generate_env_mips(self.h))

    def prefilter_env(self, samples=0):
        """Every level below level 0 of the environment rebuilt on the device as the GGX-prefiltered radiance of the roughness that selects
        it (include/rtggx.h): `samples` per texel, a power of two from ENV_FILTER_MIN_SAMPLES to ENV_FILTER_MAX_SAMPLES, 0 = 1024."""
        self._check(self.L.rtggx_prefilter_env(self.h, int(samples)))

    def set_material(self, mesh, base_color, roughness, metallic):
        bc = np.asarray(base_color, np.float32)
        self._check(self.L.rtggx_set_material(self.h, mesh, _p(bc), roughness, metallic))

    def set_metallic(self, mesh, metallic):
        self._check(self.L.rtggx_set_metallic(self.h, mesh, metallic))

    def build_as(self):
        self._check(self.L.rtggx_build_as(self.h))

    def update_frame(self, constants768):
        b = np.frombuffer(bytes(constants768), np.uint8).copy()
        if b.size != 768:
            raise ValueError("RtggxFrameConstants is 768 bytes")
        self._check(self.L.rtggx_update_frame(self.h, _p(b)))

    def update_as(self):
        self._check(self.L.rtggx_update_as(self.h))

    def transform_sh(self):
        self._check(self.L.rtggx_transform_sh(self.h))

    def render_visibility(self):
        self._check(self.L.rtggx_render_visibility(self.h))

    def ray_trace(self):
        self._check(self.L.rtggx_ray_trace(self.h))

    def denoise(self, use_shared_mem=False):
        self._check(self.L.rtggx_denoise(self.h, 1 if use_shared_mem else 0))

    def tone_map(self):
        self._check(self.L.rtggx_tone_map(self.h))

    def sync(self):
        self._check(self.L.rtggx_sync(self.h))

    def ray_count(self):
        n = C.c_uint64()
        self._check(self.L.rtggx_ray_count(self.h, C.byref(n)))
        return int(n.value)

    def ray_total(self, reset=False):
        n = C.c_uint64()
        self._check(self.L.rtggx_ray_total(self.h, C.byref(n), 1 if reset else 0))
        return int(n.value)

    def debug_trace_split(self, work_per_wave, max_shift, capacity=-1):
        """Sets the adaptive-split parameters of the trace kernel; returns the split-list entries the last frame asked for."""
        d = C.c_uint32()
        self.L.rtggx_debug_trace_split.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        self._check(self.L.rtggx_debug_trace_split(self.h, work_per_wave, max_shift, capacity, C.byref(d)))
        return int(d.value)

    def stream(self):
        """The context's main stream as an integer handle (rtggx_get_stream)."""
        h = C.c_void_p()
        self.L.rtggx_get_stream.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self.L.rtggx_get_stream(self.h, C.byref(h)))
        return int(h.value or 0)

    def trace_residency(self, force_waves=0):
        """(waves of the traversal's resident workgroup, share of the frame period the traversal took when last sampled)."""
        w, sh = C.c_uint32(), C.c_float()
        self.L.rtggx_debug_trace_residency.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        self._check(self.L.rtggx_debug_trace_residency(self.h, force_waves, C.byref(w), C.byref(sh)))
        return int(w.value), float(sh.value)

    def debug_counters(self, n=8, reset=True):
        out = np.zeros(n, np.uint32)
        self.L.rtggx_debug_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
        self._check(self.L.rtggx_debug_counters(self.h, _p(out), n, 1 if reset else 0))
        return out

    def debug_environment(self, dirs, levels, level0=False):
        """The filtered environment in each of dirs[n, 3] at mip level levels[n] (a scalar serves all), through the device functions the frame
        kernels call; level0: through their folded level-0 path, which ignores the level (include/rtggx.h).  Returns float32 [n, 3]."""
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        lv = np.ascontiguousarray(np.broadcast_to(np.asarray(levels, np.float32), (d.shape[0],)))
        out = np.zeros((d.shape[0], 3), np.float32)
        self.L.rtggx_debug_environment.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        self._check(self.L.rtggx_debug_environment(self.h, _p(d), _p(lv), d.shape[0], 1 if level0 else 0, _p(out)))
        return out

    def enable_timing(self, mode=1):
        """0 off, 1 every pass (timings()), 2 ray-trace kernel ring (kernel_times()), 3 the same for every 8th frame."""
        self._check(self.L.rtggx_enable_timing(self.h, int(mode)))

    def kernel_times(self):
        ms = np.zeros(4096, np.float32)
        n = C.c_uint32()
        self._check(self.L.rtggx_kernel_times(self.h, _p(ms), ms.size, C.byref(n)))
        return ms[:n.value].copy()

    def timings(self):
        t = Timings()
        self._check(self.L.rtggx_get_timings(self.h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in Timings._fields_}

    def buffer_size(self, bid):
        n = C.c_size_t()
        self._check(self.L.rtggx_buffer_size(self.h, bid, C.byref(n)))
        return int(n.value)

    def buffer_ptr(self, bid):
        p = C.c_void_p()
        self._check(self.L.rtggx_buffer_ptr(self.h, bid, C.byref(p)))
        return int(p.value)

    def readback(self, bid):
        n = self.buffer_size(bid)
        dt = np.dtype(_BUF_DTYPE[bid])
        out = np.zeros(max(n // dt.itemsize, 0), dt)
        if n:
            self._check(self.L.rtggx_readback(self.h, bid, _p(out), n))
        if bid <= BUF_BACKBUFFER or bid == BUF_CONVERGED:
            return out.reshape(self.H, self.W)
        if bid in (BUF_ACC_REFL, BUF_ACC_DIFF):
            return out.reshape(self.H, self.W, 4)
        if bid == BUF_SH_COEFFS:
            return out.reshape(9, 3)
        if bid in (BUF_BVH_NODES0, BUF_BVH_NODES1):
            return out.reshape(-1, 16)
        if bid in (BUF_BVH_TRIS0, BUF_BVH_TRIS1):
            return out.reshape(-1, 16)
        if bid == BUF_TLAS:
            return out.reshape(2, 4, 4)
        if bid == BUF_ENV:
            return out.reshape(-1, 4)
        if bid in (BUF_BVH4_NODES0, BUF_BVH4_NODES1, BUF_BVH4_TOP0, BUF_BVH4_TOP1):
            return out.reshape(-1, 32)
        return out

    def upload(self, bid, array):
        a = np.ascontiguousarray(array)
        self._check(self.L.rtggx_upload(self.h, bid, _p(a), a.nbytes))

    def frame_parity(self):
        p = C.c_uint32()
        self._check(self.L.rtggx_frame_parity(self.h, C.byref(p)))
        return int(p.value)

    def bvh_root(self, slot):
        r = C.c_int32()
        self._check(self.L.rtggx_bvh_root(self.h, slot, C.byref(r)))
        return int(r.value)

    def trace_rays(self, rays):
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros((r.shape[0], 6), np.float32)
        self._check(self.L.rtggx_trace_rays(self.h, _p(r), r.shape[0], _p(out)))
        return {"t": out[:, 0].copy(), "inst": out[:, 1].copy().view(np.uint32), "prim": out[:, 2].copy().view(np.uint32),
                "b1": out[:, 3].copy(), "b2": out[:, 4].copy(), "valid": out[:, 5] > 0.5}

    def set_sun(self, direction, irradiance):
        """A directional light with ray-traced shadows from the next frame on; (None, None) or a zero irradiance turns it off."""
        if direction is None and irradiance is None:
            return self._check(self.L.rtggx_set_sun(self.h, None, None))
        d, e = np.ascontiguousarray(direction, np.float32).reshape(3), np.ascontiguousarray(irradiance, np.float32).reshape(3)
        self._check(self.L.rtggx_set_sun(self.h, _p(d), _p(e)))

    def set_sun_reflections(self, on):
        """The sun term and the shadow at the surfaces the paths hit as well (0 / 1), from the next frame on; it acts only while a sun is set."""
        self._check(self.L.rtggx_set_sun_reflections(self.h, int(on)))

    def set_sun_angle(self, degrees):
        """The angular radius of the sun's disk in degrees, 0 to MAX_SUN_ANGLE_DEGREES, from the next frame on: shadow rays toward a point
        of the disk (include/rtggx.h has the rule).  0: the directional sun.  It acts only while a sun is set."""
        self._check(self.L.rtggx_set_sun_angle(self.h, float(degrees)))

    def set_lights(self, lights):
        """Point and spot lights with ray-traced shadows from the next frame on (include/rtggx.h has the rule): a sequence of Light, or of
        dicts with Light.of's arguments; None or an empty sequence turns them off."""
        lights = [l if isinstance(l, Light) else Light.of(**l) for l in (lights or ())]
        if not lights:
            return self._check(self.L.rtggx_set_lights(self.h, None, 0))
        self._check(self.L.rtggx_set_lights(self.h, (Light * len(lights))(*lights), len(lights)))

    def set_light_reflections(self, on):
        """The lights' terms and shadows at the surfaces the paths hit as well (0 / 1), from the next frame on; it acts only while lights are set."""
        self._check(self.L.rtggx_set_light_reflections(self.h, int(on)))

    def set_light_sampling(self, mode):
        """0: every light traces its own shadow ray; 1: one shadow ray per surface point for all lights, the light picked by the luminance it
        would contribute unshadowed (include/rtggx.h has the rule).  From the next frame on; it acts only while lights are set."""
        self._check(self.L.rtggx_set_light_sampling(self.h, int(mode)))

    def set_light_pick_visibility(self, enable):
        """Mode 1's pick weighted by the visibility each pixel remembers per light (0 / 1; include/rtggx.h has the rule).  From the next
        frame on; it acts only in mode-1 frames with a casting light; whole frames only."""
        self._check(self.L.rtggx_set_light_pick_visibility(self.h, int(enable)))

    def read_light_visibility(self, image):
        """(records, sequence): image 0 or 1 of the records as a LIGHT_VIS_RECORD array [H, W], and the context's s.  Raises before the
        first acting frame."""
        a = np.zeros((self.H, self.W), LIGHT_VIS_RECORD)
        seq = C.c_uint32()
        self._check(self.L.rtggx_read_light_visibility(self.h, int(image), _p(a), a.nbytes, C.byref(seq)))
        return a, seq.value

    def set_light_list(self, lights):
        """A list of up to MAX_LIGHT_LIST lights under mode 1's rule, culled per 8x8 block, from the next frame on (include/rtggx.h has the
        rule): a sequence of Light, or of dicts with Light.of's arguments; None or an empty sequence clears the list.  In place of
        set_lights, not beside it."""
        lights = [l if isinstance(l, Light) else Light.of(**l) for l in (lights or ())]
        if not lights:
            return self._check(self.L.rtggx_set_light_list(self.h, None, 0))
        self._check(self.L.rtggx_set_light_list(self.h, (Light * len(lights))(*lights), len(lights)))

    def read_light_list_counts(self):
        """The kept lights per 8x8 block of the last frame's primary pass with a list, uint32 [ceil(H/8), ceil(W/8)].  Synchronises.  Raises
        before the first frame with a list, and on a strip."""
        a = np.zeros(((self.H + 7) // 8, (self.W + 7) // 8), np.uint32)
        self._check(self.L.rtggx_read_light_list_counts(self.h, _p(a), a.nbytes))
        return a

    def debug_light_list_cull(self, enable):
        """1 (default): the list's cull; 0: every casting light is kept in every block that has a point -- the same images, the walk's time."""
        self._check(self.L.rtggx_debug_light_list_cull(self.h, int(enable)))

    def set_light_list_visibility(self, enable):
        """A list's pick weighted by the sparse record each pixel keeps of the lights it found hidden (0 / 1; include/rtggx.h has the rule).
        From the next frame on; it acts only in frames with a list that has a casting light; whole frames only."""
        self._check(self.L.rtggx_set_light_list_visibility(self.h, int(enable)))

    def read_light_list_visibility(self, image):
        """(records, sequence): image 0 or 1 of the list's records as a LIGHT_LIST_VIS_RECORD array [H, W], and the setting's s.  Raises
        before the first acting frame."""
        a = np.zeros((self.H, self.W), LIGHT_LIST_VIS_RECORD)
        seq = C.c_uint32()
        self._check(self.L.rtggx_read_light_list_visibility(self.h, int(image), _p(a), a.nbytes, C.byref(seq)))
        return a, seq.value

    def update_light_list(self, lights, first=0):
        """Lights first .. first + len(lights) - 1 of the list the context holds, replaced from the next frame on (include/rtggx.h has
        the rule): a sequence of Light, or of dicts with Light.of's arguments, or a float32 array [n, 16] in RtggxLight's layout.  No wait,
        no reset of the records' history."""
        if isinstance(lights, np.ndarray):
            a = np.ascontiguousarray(lights, np.float32).reshape(-1, 16)
            return self._check(self.L.rtggx_update_light_list(self.h, C.cast(_p(a), C.POINTER(Light)) if len(a) else None, int(first), len(a)))
        lights = [l if isinstance(l, Light) else Light.of(**l) for l in lights]
        self._check(self.L.rtggx_update_light_list(self.h, (Light * len(lights))(*lights) if lights else None, int(first), len(lights)))

    def update_light_list_device(self, ptr, first, count, kinds, stream=0):
        """The same from `count` RtggxLight in device memory at `ptr` (16-byte aligned), read on `stream` (0: the null stream) in stream
        order; kinds: LIGHT_KIND_RADIUS | LIGHT_KIND_CONE, what the lights may have.  An invalid light becomes one that casts nothing
        and is counted (read_light_list_rejects)."""
        self._check(self.L.rtggx_update_light_list_device(self.h, C.c_void_p(int(ptr)), int(first), int(count), int(kinds), C.c_void_p(int(stream) or None)))

    def read_light_list(self):
        """The list the last frame read as the kernels see it: float32 [count, 16] in RtggxLight's layout.  Synchronises.  Raises before
        the first frame with a list."""
        a = np.zeros((self._light_list_count(), 16), np.float32)
        self._check(self.L.rtggx_read_light_list(self.h, _p(a), a.nbytes))
        return a

    def _light_list_count(self):
        """The count rtggx_read_light_list wants: its message names it (the ABI has no getter of its own)."""
        if self.L.rtggx_read_light_list(self.h, None, 0) == 0:
            return 0
        m = re.search(r"(\d+) lights of 64 bytes", self.L.rtggx_last_error().decode())
        if not m:
            self._check(-1)
        return int(m.group(1))

    def read_light_list_rejects(self, reset=False):
        """The lights the device path has refused since the last reset.  Synchronises."""
        n = C.c_uint64()
        self._check(self.L.rtggx_read_light_list_rejects(self.h, C.byref(n), 1 if reset else 0))
        return n.value

    def debug_visibility_drains(self, reset=False):
        """How often rtggx_render_visibility has waited for every stream of the context since the last reset."""
        n = C.c_uint32()
        self._check(self.L.rtggx_debug_visibility_drains(self.h, C.byref(n), 1 if reset else 0))
        return n.value

    def sun_from_env(self, cone=0, ring=0, min_contrast=0, remove=False):
        """The sun of the current environment (include/rtggx.h): the record as a dict (SunEstimate.as_dict) -- "direction" and "irradiance" are
        what set_sun takes, "found" says whether there is a sun at all.  cone, ring: half-angles in degrees (0: 4 and three times the cone);
        min_contrast: how far the peak must stand above the mean luminance (0: 16); remove: cut the sun out of the cube and rebuild its box
        chain.  Synchronises."""
        e = SunEstimate()
        self._check(self.L.rtggx_sun_from_env(self.h, float(cone), float(ring), float(min_contrast), 1 if remove else 0, C.byref(e)))
        return e.as_dict()

    def trace_occlusion(self, rays):
        """One bool per ray {o.xyz, d.xyz, tmin, tmax}: is there a triangle with tmin < t < tmax (the any-hit traversal)."""
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
        out = np.zeros(r.shape[0], np.uint32)
        self._check(self.L.rtggx_trace_occlusion(self.h, _p(r), r.shape[0], _p(out)))
        return out != 0
