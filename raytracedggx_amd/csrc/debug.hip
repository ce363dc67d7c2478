// C ABI of librtggx (include/rtggx.h), part 4 of 4: what tests, tools and the benchmark ask a context -- counters, timing, buffer access,
// the diagnostic switches and probes, rays traced on their own.
#include <cstring>
#include "capi_internal.h"
#include "rt_queue.h"
namespace rt {
__global__ void __launch_bounds__(256) copyKernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) dst[i] = src[i];
}
typedef float __attribute__((ext_vector_type(4))) CopyVec4;
__global__ void __launch_bounds__(256) copyKernelNT(const CopyVec4* __restrict__ src, CopyVec4* __restrict__ dst, size_t n) {      // the data is used once: non-temporal loads and stores
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) __builtin_nontemporal_store(__builtin_nontemporal_load(&src[i]), &dst[i]);
}
}  // namespace rt
using namespace rt;

extern "C" {
int rtggx_ray_count(rtggx_context* c, uint64_t* rays) {
  RT_CHECK_CTX(c);
  uint32_t h[256];
  RT_HIP(syncStreams(c));
  RT_HIP(hipMemcpy(h, c->lastRayCounter32, sizeof h, hipMemcpyDeviceToHost));
  uint64_t s = 0; for (auto v : h) s += v;
  *rays = s;
  return 0;
}

// Diagnostic counters of builds compiled with -DRT_TRACE_STATS (zero otherwise): lane node steps, lane leaf
// steps, wave iterations, refills -- accumulated since the last reset.
int rtggx_debug_counters(rtggx_context* c, uint32_t* out, uint32_t n, int reset) {
  RT_CHECK_CTX(c);
  if (n > 768) { setError("rtggx_debug_counters: at most 768 words"); return -1; }
  RT_HIP(syncStreams(c));
  RT_HIP(hipMemcpy(out, c->rayCounterBuf + 1024, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (reset) { RT_HIP(hipMemset(c->rayCounterBuf + 1024, 0, 768 * 4)); RT_HIP(hipStreamSynchronize(nullptr)); }
  return 0;
}

int rtggx_debug_fence_wait(rtggx_context* c, double* usTotal, uint32_t* waits, int reset) {
  RT_CHECK_CTX(c);
  if (usTotal) *usTotal = c->fenceWaitUs;
  if (waits) *waits = c->fenceWaits;
  if (reset) { c->fenceWaitUs = 0.0; c->fenceWaits = 0u; }
  return 0;
}
int rtggx_debug_fuse_tone_map(rtggx_context* c, int mode) {
  RT_CHECK_CTX(c);
  c->fuseToneMap = mode < 0 ? -1 : mode != 0;      // from the next rtggx_denoise on
  return 0;
}
// force_small: -1 by the ray count, 0 / 1 the placement of a full-size / small launch whatever the count (from the next frame on).
// key / where (either may be null): the most recent rtggx_ray_trace's key (bit 0 small, 1 strip, 2 deforming, 3 diffuse, 4 caller-owned
// stream) and placement (bits 0-3 / 4-7 / 8-11: the streams of ray generation / traversal / hit shading -- 0 main, 1 B, 2 C, 3 R --,
// bits 12-15 frames in flight).
int rtggx_debug_tile_words(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  c->useTileWords = enable != 0;
  c->sky.breakRuns(SkyBreak::TileWordsSwitch);
  return 0;
}
// Still sky (rtggx_context.h InputSet::skyRun): enable = 0 -- the runs are still counted, but no tile is left alone for them.
int rtggx_debug_static_sky(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  c->sky.enableStaticSky(enable != 0);
  return 0;
}
// The current set's runs (0 where a word was written under another epoch than the current one), tile by tile of the most recent ray
// generation's grid; *threshold: the run from which that ray generation left a tile alone.
int rtggx_debug_sky_runs(rtggx_context* c, uint32_t* runs, uint32_t capacity, uint32_t* tilesX, uint32_t* tilesY, uint32_t* threshold) {
  RT_CHECK_CTX(c);
  const uint32_t n = c->sky.genTilesX() * c->sky.genTilesY();
  if (!runs || capacity < n || n > c->skyTiles) { setError("rtggx_debug_sky_runs: room for %u words", n); return -1; }
  RT_HIP(syncStreams(c));
  if (n) RT_HIP(hipMemcpy(runs, c->cur().skyRun, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; ++i) runs[i] = (runs[i] >> 8) == c->sky.epoch() ? runs[i] & 0xFFu : 0u;
  if (tilesX) *tilesX = c->sky.genTilesX();
  if (tilesY) *tilesY = c->sky.genTilesY();
  if (threshold) *threshold = RT_SKY_PREV_RUN + 1u;
  return 0;
}
// Settled sky (denoise.hip temporalKernel): enable = 0 -- no words are kept and no block of the temporal pass or the tone map is left alone.
int rtggx_debug_settled_sky(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  c->sky.enableSettledSky(enable != 0);
  return 0;
}
// Both word arrays as they are (epoch << 8 | flags) without their border, blocksX columns of blocksY words each; *epoch: the epoch words count under now.
int rtggx_debug_settled_words(rtggx_context* c, uint32_t* words0, uint32_t* words1, uint32_t capacity, uint32_t* blocksX, uint32_t* blocksY, uint32_t* epoch) {
  RT_CHECK_CTX(c);
  const uint32_t n = c->settledX * c->settledY;
  if (!words0 || !words1 || capacity < n) { setError("rtggx_debug_settled_words: room for %u words each", n); return -1; }
  RT_HIP(syncStreams(c));
  uint32_t* const out[2] = {words0, words1};
  for (int p = 0; p < 2 && n; ++p)
    RT_HIP(hipMemcpy2D(out[p], (size_t)c->settledY * 4, c->settled[p] + c->settledPitch + 1u, (size_t)c->settledPitch * 4, (size_t)c->settledY * 4, c->settledX, hipMemcpyDeviceToHost));
  if (blocksX) *blocksX = c->settledX;
  if (blocksY) *blocksY = c->settledY;
  if (epoch) *epoch = c->sky.epoch();
  return 0;
}
int rtggx_debug_placement(rtggx_context* c, int forceSmall, uint32_t* key, uint32_t* where) {
  RT_CHECK_CTX(c);
  if (forceSmall < -1 || forceSmall > 1) { setError("rtggx_debug_placement: force_small is -1, 0 or 1"); return -1; }
  c->forcePlacement = forceSmall;
  if (forceSmall >= 0) c->lastTraceSmall = forceSmall == 1;
  if (key) *key = c->lastPlacement[0];
  if (where) *where = c->lastPlacement[1];
  return 0;
}
int rtggx_debug_collapse_weights(rtggx_context* c, const float* set, float* get) {
  RT_CHECK_CTX(c);
  if (set) { if (!(set[0] >= 0.0f) || !(set[1] >= 0.0f) || !(set[0] + set[1] > 0.0f)) { setError("rtggx_debug_collapse_weights: two non-negative weights, not both zero"); return -1; }
             c->collapseWeights[0] = set[0]; c->collapseWeights[1] = set[1]; }
  if (get) { get[0] = c->collapseWeights[0]; get[1] = c->collapseWeights[1]; }
  return 0;
}
int rtggx_debug_trace_residency(rtggx_context* c, uint32_t forceWaves, uint32_t* waves, float* share) {
  RT_CHECK_CTX(c);
  if (forceWaves != 0u && forceWaves != 10u && forceWaves != 12u && forceWaves != 14u && forceWaves != 16u) { setError("rtggx_debug_trace_residency: %u waves: 0, 10, 12, 14 or 16", forceWaves); return -1; }
  c->traceWavesForced = forceWaves;
  if (forceWaves) c->traceWaves = forceWaves;
  if (waves) *waves = c->traceWaves;
  if (share) *share = c->traceShare;
  return 0;
}

// The environment sampler by itself: n directions (and levels) through the device functions the frame kernels call.  Reads the decoded
// cube and its offset table, nothing else: no frame state, no sky runs, no input set.
int rtggx_debug_environment(rtggx_context* c, const float* dirs3, const float* levels, uint32_t n, int level0Path, float* rgb3) {
  RT_CHECK_CTX(c);
  if (!c->env.texels) { setError("rtggx_debug_environment: no environment map"); return -1; }
  if (n == 0 || !dirs3 || !rgb3 || (!levels && !level0Path)) { setError("rtggx_debug_environment: no directions, levels or result (n %u)", n); return -1; }
  DevBuf<float> dD, dL, dO;
  hipError_t e = alloc(dD, (size_t)n * 3);
  if (e == hipSuccess) e = alloc(dO, (size_t)n * 3);
  if (e == hipSuccess && levels) e = alloc(dL, (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(dD, dirs3, (size_t)n * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess && levels) e = hipMemcpy(dL, levels, (size_t)n * 4, hipMemcpyHostToDevice);
  int r = 0;
  if (e == hipSuccess) r = launchDebugEnvironment(c, dD, dL, n, level0Path, dO, c->streamMain);
  if (e == hipSuccess && !r) e = hipStreamSynchronize(c->streamMain);
  if (e == hipSuccess && !r) e = hipMemcpy(rgb3, dO, (size_t)n * 12, hipMemcpyDeviceToHost);
  if (e != hipSuccess) { setError("rtggx_debug_environment: %s", hipGetErrorString(e)); return -2; }
  return r;
}

int rtggx_debug_trace_split(rtggx_context* c, uint32_t workPerWave, uint32_t maxShift, int capacity, uint32_t* lastDemand) {
  RT_CHECK_CTX(c);
  if (maxShift > 3u) { setError("rtggx_debug_trace_split: max_shift %u > 3", maxShift); return -1; }
  if (capacity > (int)RT_SPLIT_CAP) { setError("rtggx_debug_trace_split: capacity %d > %u", capacity, RT_SPLIT_CAP); return -1; }
  RT_HIP(syncStreams(c));
  if (lastDemand) RT_HIP(hipMemcpy(lastDemand, c->cur().splitCount, 4, hipMemcpyDeviceToHost));
  c->splitWork = workPerWave; c->splitMaxShift = maxShift;
  c->splitCapForced = capacity < 0 ? 0xFFFFFFFFu : ((uint32_t)capacity / 32u) * 32u;
  return 0;
}

int rtggx_ray_total(rtggx_context* c, uint64_t* rays, int reset) {
  RT_CHECK_CTX(c);
  unsigned long long h[256];
  RT_HIP(syncStreams(c));
  RT_HIP(hipMemcpy(h, c->rayCounter + 256, sizeof h, hipMemcpyDeviceToHost));
  uint64_t s = 0; for (auto v : h) s += v;
  *rays = s;
  if (reset) { RT_HIP(hipMemset(c->rayCounter + 256, 0, sizeof h)); RT_HIP(hipStreamSynchronize(nullptr)); }
  return 0;
}

// mode 0: off; 1: every pass (rtggx_get_timings); 2: only the ray-trace kernel, one event pair per frame
// kept in a ring of `RTGGX_KERNEL_RING` frames (rtggx_kernel_times) -- no host synchronisation per frame.
int rtggx_enable_timing(rtggx_context* c, int mode) {
  RT_CHECK_CTX(c);
  c->timing = mode == 1; c->timingsPending = false;
  c->kernelRing = mode == 2 || mode == 3; c->kevCount = 0; c->ringStride = mode == 3 ? 8u : 1u; c->ringTick = 0;
  if (c->kernelRing && c->kevBegin.empty()) {
    c->kevBegin.resize(RTGGX_KERNEL_RING); c->kevEnd.resize(RTGGX_KERNEL_RING);
    for (uint32_t i = 0; i < RTGGX_KERNEL_RING; ++i) { RT_HIP(create(c->kevBegin[i])); RT_HIP(create(c->kevEnd[i])); }
  }
  return 0;
}
int rtggx_kernel_times(rtggx_context* c, float* ms, uint32_t capacity, uint32_t* count) {
  RT_CHECK_CTX(c);
  RT_HIP(syncStreams(c));
  const uint32_t n = c->kevCount < capacity ? c->kevCount : capacity;
  for (uint32_t i = 0; i < n; ++i) RT_HIP(hipEventElapsedTime(&ms[i], c->kevBegin[i], c->kevEnd[i]));
  *count = n;
  c->kevCount = 0;
  return 0;
}
int rtggx_get_timings(rtggx_context* c, RtggxTimings* out) {
  RT_CHECK_CTX(c);
  if (!c->timing || !c->timingsPending) { setError("rtggx_get_timings: timing not enabled or no complete frame"); return -1; }
  RT_HIP(syncStreams(c));
  auto ms = [&](int a, int b) { float t = 0.0f; hipEventElapsedTime(&t, c->tev[a], c->tev[b]); return t; };
  RtggxTimings t;
  t.update_as = ms(0, 1); t.visibility = ms(2, 13); t.ray_trace = ms(3, 14); t.spatial_refl_h = ms(9, 4); t.spatial_refl_v = ms(4, 5);
  t.spatial_diff_h = ms(5, 6); t.spatial_diff_v = ms(6, 7); t.temporal = ms(7, 8); t.tone_map = ms(8, 10); t.frame = ms(2, 10);
  t.ray_trace_kernel = ms(11, 12);
  *out = t;
  return 0;
}

static int bufferInfo(rtggx_context* c, int id, void** ptr, size_t* bytes) {
  const size_t n = (size_t)c->W * c->H;
  switch (id) {
    case RTGGX_BUF_VISIBILITY: case RTGGX_BUF_DEPTH: *ptr = nullptr; *bytes = n * 4; return 0;   // halves of visDepth: staged
    case RTGGX_BUF_NORMAL: *ptr = c->cur().normal; *bytes = n * 4; return 0;
    case RTGGX_BUF_ROUGH_METAL: *ptr = c->cur().roughMetal; *bytes = n * 2; return 0;
    case RTGGX_BUF_VELOCITY: *ptr = c->cur().velocity; *bytes = n * 4; return 0;
    case RTGGX_BUF_RT_REFL: *ptr = c->cur().rtRefl; *bytes = n * 4; return 0;
    case RTGGX_BUF_RT_DIFF: *ptr = c->cur().rtDiff; *bytes = n * 4; return 0;
    case RTGGX_BUF_TSS0: *ptr = c->tss[0]; *bytes = n * 8; return 0;
    case RTGGX_BUF_TSS1: *ptr = c->tss[1]; *bytes = n * 8; return 0;
    case RTGGX_BUF_FLT_RFL: *ptr = c->fltRflIsFltDff ? c->fltDff.get() : c->fltRfl.get(); *bytes = n * 8; return 0;      // identical images when no diffuse pass ran: only one was written (denoise.hip launchDenoise)
    case RTGGX_BUF_FLT_DFF: *ptr = c->fltDff; *bytes = n * 8; return 0;
    case RTGGX_BUF_BACKBUFFER: *ptr = c->backbuffer; *bytes = n * 4; return 0;
    case RTGGX_BUF_SH_COEFFS: *ptr = c->sh; *bytes = 108; return 0;
    case RTGGX_BUF_BVH_NODES0: case RTGGX_BUF_BVH_NODES1: { const MeshDev& m = c->mesh[id == RTGGX_BUF_BVH_NODES1]; *ptr = m.nodes; *bytes = m.numTris > 1 && m.nodes ? (size_t)(m.numTris - 1) * 64 : 0; return 0; }
    case RTGGX_BUF_BVH_TRIS0: case RTGGX_BUF_BVH_TRIS1: { const MeshDev& m = c->mesh[id == RTGGX_BUF_BVH_TRIS1]; *ptr = m.tris; *bytes = m.tris ? (size_t)m.numTris * 64 : 0; return 0; }
    case RTGGX_BUF_TLAS: *ptr = nullptr; *bytes = 128; return 0;
    case RTGGX_BUF_BVH4_NODES0: case RTGGX_BUF_BVH4_NODES1: { const MeshDev& m = c->mesh[id == RTGGX_BUF_BVH4_NODES1]; *ptr = m.nodes4; *bytes = m.numTris > 1 && m.nodes4 ? (size_t)(m.numTris - 1) * sizeof(Bvh4Node) : 0; return 0; }
    case RTGGX_BUF_BVH4_TOP0: case RTGGX_BUF_BVH4_TOP1: { const MeshDev& m = c->mesh[id == RTGGX_BUF_BVH4_TOP1]; *ptr = m.top; *bytes = m.top ? (size_t)m.topCount * sizeof(Bvh4Node) : 0; return 0; }
    case RTGGX_BUF_BIN_WORK: *ptr = c->binWork; *bytes = (size_t)(((c->W + 15) / 16) * ((c->H + 15) / 16)) * 4u * 4u; return 0;
    case RTGGX_BUF_ENV: *ptr = c->env.texels; *bytes = (size_t)c->env.totalTexels * 8; return 0;
    case RTGGX_BUF_EXCHANGE_TOKENS: *ptr = c->exchangeTokens; *bytes = 4 * 2 * RT_MAX_PEERS; return 0;
    case RTGGX_BUF_ACC_REFL: case RTGGX_BUF_ACC_DIFF: case RTGGX_BUF_CONVERGED:
      if (!c->accRefl) { setError("buffer %d exists once accumulation has been enabled (rtggx_set_accumulation)", id); return -1; }
      *ptr = id == RTGGX_BUF_ACC_REFL ? (void*)c->accRefl : id == RTGGX_BUF_ACC_DIFF ? (void*)c->accDiff : (void*)c->converged;
      *bytes = n * (id == RTGGX_BUF_CONVERGED ? 8u : 16u); return 0;
    default: setError("unknown buffer id %d", id); return -1;
  }
}

int rtggx_buffer_size(rtggx_context* c, int id, size_t* bytes) { RT_CHECK_CTX(c); void* p; return bufferInfo(c, id, &p, bytes); }

int rtggx_buffer_ptr(rtggx_context* c, int id, void** dptr) {
  RT_CHECK_CTX(c);
  size_t bytes;
  const int r = bufferInfo(c, id, dptr, &bytes);
  if (r) return r;
  if (id == RTGGX_BUF_VISIBILITY || id == RTGGX_BUF_DEPTH) *dptr = c->curVis().depth;   // packed u64: (depth << 32) | visibility
  if (!*dptr) { setError("buffer %d has no device storage", id); return -1; }
  return 0;
}

int rtggx_readback(rtggx_context* c, int id, void* dst, size_t bytes) {
  RT_CHECK_CTX(c);
  void* p; size_t need;
  int r = bufferInfo(c, id, &p, &need);
  if (r) return r;
  if (bytes < need) { setError("rtggx_readback: buffer %d needs %zu bytes, %zu given", id, need, bytes); return -1; }
  RT_HIP(syncStreams(c));
  if (id == RTGGX_BUF_TLAS) { memcpy(dst, c->invWorld, 128); return 0; }
  if (id == RTGGX_BUF_VISIBILITY || id == RTGGX_BUF_DEPTH) {
    DevBuf<uint32_t> dVis, dDepth;
    RT_HIP(alloc(dVis, need / 4)); RT_HIP(alloc(dDepth, need / 4));
    r = unpackVisDepth(c, dVis, dDepth, c->streamMain);
    if (!r && hipStreamSynchronize(c->streamMain) != hipSuccess) { setError("readback: stream sync failed"); r = -2; }   // the copy below runs on the null stream
    if (!r) { hipError_t e = hipMemcpy(dst, id == RTGGX_BUF_VISIBILITY ? dVis.get() : dDepth.get(), need, hipMemcpyDeviceToHost); if (e != hipSuccess) { setError("hipMemcpy: %s", hipGetErrorString(e)); r = -2; } }
    return r;
  }
  if (need == 0) return 0;
  RT_HIP(hipMemcpy(dst, p, need, hipMemcpyDeviceToHost));
  return 0;
}

int rtggx_upload(rtggx_context* c, int id, const void* src, size_t bytes) {
  RT_CHECK_CTX(c);
  void* p; size_t need;
  int r = bufferInfo(c, id, &p, &need);
  if (r) return r;
  if (bytes != need) { setError("rtggx_upload: buffer %d is %zu bytes, %zu given", id, need, bytes); return -1; }
  RT_HIP(syncStreams(c));
  c->toneMapDone = false;      // (a tone map after an upload reads what was uploaded)
  c->curVis().flags.rasterFrame = 0u;      // ... and the tiles' words of this frame's visibility pass do not describe it (rtggx_context.h VisTarget::dirty)
  c->sky.breakRuns(SkyBreak::Upload);      // ... and what a still-sky tile relies on being in place may just have been replaced
  if (id == RTGGX_BUF_VISIBILITY || id == RTGGX_BUF_DEPTH) {
    // replace one half of the packed buffer
    DevBuf<uint32_t> dVis, dDepth;
    RT_HIP(alloc(dVis, need / 4)); RT_HIP(alloc(dDepth, need / 4));
    r = unpackVisDepth(c, dVis, dDepth, c->streamMain);
    if (!r && hipStreamSynchronize(c->streamMain) != hipSuccess) { setError("upload: stream sync failed"); r = -2; }
    if (!r) { hipError_t e = hipMemcpy(id == RTGGX_BUF_VISIBILITY ? dVis.get() : dDepth.get(), src, need, hipMemcpyHostToDevice); if (e != hipSuccess) { setError("hipMemcpy: %s", hipGetErrorString(e)); r = -2; } }
    if (!r) r = packVisDepth(c, dVis, dDepth, c->streamMain);
    if (!r && id == RTGGX_BUF_DEPTH && hipMemcpy(c->cur().depth32, src, need, hipMemcpyHostToDevice) != hipSuccess) { setError("upload: depth copy failed"); r = -2; }      // the filters' copy (ray generation writes it otherwise)
    hipStreamSynchronize(c->streamMain);
    return r;
  }
  if (id == RTGGX_BUF_SH_COEFFS) c->shDone = true;
  if (!p || id >= RTGGX_BUF_BVH_NODES0) { setError("rtggx_upload: buffer %d is not writable", id); return -1; }
  RT_HIP(hipMemcpy(p, src, need, hipMemcpyHostToDevice));
  return 0;
}

// Attainable HBM bandwidth of the device, for the roofline's "peak measured beside the vendor figure" (SURVEY 8d): a float4
// copy kernel over two buffers of `bytes` each (far larger than the 256 MiB Infinity Cache when bytes >= 1 GiB: at 2 x 128 MiB the same
// loop reads 7.2 TB/s), timed with events on the main stream; gbytes_per_s = (bytes read + bytes written) / time.  The launch shape
// matters by 20 % on this part and non-temporal accesses by another 8 % (tools/microbench/copy_bw.hip, profiles/r03_h_copy_peak.txt,
// r04_b_copy_peak.txt: a grid-stride loop at 4 workgroups per CU 5.7 TB/s, at 16 per CU 4.6, hipMemcpyAsync 4.8; the same loop at 4 per CU
// with non-temporal loads and stores 6.17 TB/s -- 98 % of the 6.29 MI355X_MICROARCH.md quotes; rounds 2-3 reported 5.5-5.7 without them):
// the shapes of kCopyShapes each get `iterations` launches, plain and non-temporal, and the best one is reported.
static const uint32_t kCopyShapes[] = {2u, 4u, 8u, 16u};   // workgroups per CU
int rtggx_copy_bandwidth(rtggx_context* c, size_t bytes, int iterations, double* gbytesPerS) {
  RT_CHECK_CTX(c);
  if (!gbytesPerS || bytes < 1024 || iterations < 1) { setError("rtggx_copy_bandwidth: bad arguments"); return -1; }
  RT_HIP(syncStreams(c));
  const size_t n = bytes / 16;
  DevBuf<float4> src, dst;
  RT_HIP(alloc(src, n));
  if (alloc(dst, n) != hipSuccess) { setError("rtggx_copy_bandwidth: out of device memory"); return -2; }
  hipMemsetAsync(src, 0x3C, n * 16, c->streamMain);
  Event e0, e1; RT_HIP(create(e0)); RT_HIP(create(e1));
  hipError_t e = hipSuccess;
  double best = 0.0;
  for (uint32_t shape : kCopyShapes) {
    const uint32_t blocks = c->numCUs * shape;
    for (int nt = 0; nt < 2 && e == hipSuccess; ++nt) {
      const auto launch = [&]() { if (nt) hipLaunchKernelGGL(copyKernelNT, dim3(blocks), dim3(256), 0, c->streamMain, (const CopyVec4*)src.get(), (CopyVec4*)dst.get(), n);
                                  else hipLaunchKernelGGL(copyKernel, dim3(blocks), dim3(256), 0, c->streamMain, (const float4*)src, dst.get(), n); };
      for (int i = 0; i < 2; ++i) launch();
      hipEventRecord(e0, c->streamMain);
      for (int i = 0; i < iterations; ++i) launch();
      hipEventRecord(e1, c->streamMain);
      e = hipEventSynchronize(e1);
      float ms = 0.0f;
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
      if (e != hipSuccess || !(ms > 0.0f)) { if (e == hipSuccess) e = hipErrorUnknown; break; }
      const double rate = 2.0 * (double)(n * 16) * iterations / ((double)ms * 1e-3) / 1e9;
      if (rate > best) best = rate;
    }
    if (e != hipSuccess) break;
  }
  if (e != hipSuccess) { setError("rtggx_copy_bandwidth: %s", hipGetErrorString(e)); return -2; }
  *gbytesPerS = best;
  return 0;
}

// Diagnostic: the shader clock the chip is running at right now -- one wave on stream R idles for ~20 us between two readings of
// s_memtime (shader cycles) and s_memrealtime (100 MHz), while whatever the other streams hold keeps running (profiles/r02_*).
__global__ void clockProbeKernel(unsigned long long* out) {
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long r1 = r0;
  while (r1 - r0 < 2000ull) { __builtin_amdgcn_s_sleep(32); r1 = __builtin_amdgcn_s_memrealtime(); }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; }
}
int rtggx_debug_shader_clock(rtggx_context* c, double* mhz) {
  RT_CHECK_CTX(c);
  if (!mhz) { setError("rtggx_debug_shader_clock: null result"); return -1; }
  DevBuf<unsigned long long> d; unsigned long long h[2] = {0, 1};
  RT_HIP(alloc(d, 2));
  hipLaunchKernelGGL(clockProbeKernel, dim3(1), dim3(64), 0, c->streamRefit, d.get());
  RT_HIP(hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, c->streamRefit));
  RT_HIP(hipStreamSynchronize(c->streamRefit));
  *mhz = (double)h[0] / (double)h[1] * 100.0;
  return 0;
}

int rtggx_frame_parity(rtggx_context* c, uint32_t* parity) { RT_CHECK_CTX(c); *parity = c->frameParity; return 0; }
int rtggx_bvh_root(rtggx_context* c, uint32_t slot, int32_t* root) { RT_CHECK_CTX(c); if (slot > 1) { setError("bad slot"); return -1; } *root = c->mesh[slot].root; return 0; }

int rtggx_trace_rays(rtggx_context* c, const float* rays, uint32_t n, float* out) {
  RT_CHECK_CTX(c);
  if (!c->asBuilt || !c->haveConstants) { setError("rtggx_trace_rays: build_as / update_frame / update_as first"); return -1; }
  RT_HIP(syncStreams(c));   // the ray bins are shared with the frame path on stream B
  c->sky.breakRuns(SkyBreak::TraceRays);        // (... and a still-sky tile relies on its bins' counts being 0)
  { const int r = ensureParams(c); if (r) return r; }
  DevBuf<float> dR, dO;
  RT_HIP(alloc(dR, (size_t)n * 8)); RT_HIP(alloc(dO, (size_t)n * 6));
  RT_HIP(hipMemcpy(dR, rays, (size_t)n * 32, hipMemcpyHostToDevice));
  int r = 0;
  const uint32_t perLaunch = c->numBinsMax * c->binSlots;
  for (uint32_t done = 0; done < n && !r; done += perLaunch) {   // the ray bins' capacity per launch
    const uint32_t m = n - done < perLaunch ? n - done : perLaunch;
    r = launchTraceRays(c, c->slots[c->slot], dR + (size_t)done * 8, m, dO + (size_t)done * 6, c->streamMain);
  }
  const hipError_t queued = hipStreamSynchronize(c->streamMain);      // also after a failed chunk: the chunks before it still read dR and write dO, which leave with this scope
  if (!r) { hipError_t e = queued; if (e == hipSuccess) e = hipMemcpy(out, dO, (size_t)n * 24, hipMemcpyDeviceToHost); if (e != hipSuccess) { setError("trace_rays: %s", hipGetErrorString(e)); r = -2; } }
  return r;
}

// The list path of rtggx_trace_rays through the any-hit variant of the trace kernel: one word per ray, 1 = occluded.
int rtggx_trace_occlusion(rtggx_context* c, const float* rays, uint32_t n, uint32_t* occluded) {
  RT_CHECK_CTX(c);
  if (!rays || !occluded) { setError("rtggx_trace_occlusion: null rays or result"); return -1; }
  if (n == 0u) { setError("rtggx_trace_occlusion: no rays"); return -1; }
  if (!c->asBuilt || !c->haveConstants) { setError("rtggx_trace_occlusion: build_as / update_frame / update_as first"); return -1; }
  RT_HIP(syncStreams(c));   // the ray bins are shared with the frame path on stream B
  c->sky.breakRuns(SkyBreak::TraceRays);        // (it refills a set's bins, as rtggx_trace_rays does)
  { const int r = ensureParams(c); if (r) return r; }
  DevBuf<float> dR; DevBuf<uint32_t> dO;
  RT_HIP(alloc(dR, (size_t)n * 8)); RT_HIP(alloc(dO, (size_t)n));
  RT_HIP(hipMemcpy(dR, rays, (size_t)n * 32, hipMemcpyHostToDevice));
  int r = 0;
  const uint32_t perLaunch = c->numBinsMax * c->binSlots;
  for (uint32_t done = 0; done < n && !r; done += perLaunch) {   // the ray bins' capacity per launch
    const uint32_t m = n - done < perLaunch ? n - done : perLaunch;
    r = launchTraceOcclusion(c, c->slots[c->slot], dR + (size_t)done * 8, m, dO + (size_t)done, c->streamMain);
  }
  const hipError_t queued = hipStreamSynchronize(c->streamMain);      // also after a failed chunk (see rtggx_trace_rays)
  if (!r) { hipError_t e = queued; if (e == hipSuccess) e = hipMemcpy(occluded, dO, (size_t)n * 4, hipMemcpyDeviceToHost); if (e != hipSuccess) { setError("trace_occlusion: %s", hipGetErrorString(e)); r = -2; } }
  return r;
}

}  // extern "C"
