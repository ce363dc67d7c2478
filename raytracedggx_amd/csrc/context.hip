// C ABI of librtggx (include/rtggx.h), part 1 of 4: the context's lifetime -- what it allocates at creation and on the first use of a
// feature --, the error text, and the entry points that only record state or allocate.  (mesh.hip: scene geometry and refits; frame.hip:
// the per-frame passes and where their kernels go; debug.hip: counters, timing, readback, probes.)
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cmath>
#include <vector>
#include <algorithm>
#include "capi_internal.h"
#include "rt_queue.h"
#include "rt_env_filter.h"
#include "rt_sun_env.h"
#include "rt_light_check.h"

#ifndef RT_REFIT_REBUILD_RATIO
#define RT_REFIT_REBUILD_RATIO 1.2f      // a refitted tree whose cost has grown by this factor since its build is rebuilt (rtggx_refit_as)
#endif
#ifndef RT_REBUILD_STEPS
#define RT_REBUILD_STEPS 16u             // launches of such a rebuild issued per frame (the bunny's build is ~75: five frames)
#endif
namespace rt {
static thread_local char g_err[512] = "";
void setError(const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
}

__global__ void uploadParamsKernel(FrameParams src, FrameParams* dst) {
  // 912 bytes: one wave copies the by-value argument into the device-resident slot
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&src);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  for (uint32_t i = threadIdx.x; i < sizeof(FrameParams) / 4; i += blockDim.x) d[i] = s[i];
}
int uploadParams(rtggx_context* c, uint32_t slot, hipStream_t s) {
  hipLaunchKernelGGL(uploadParamsKernel, dim3(1), dim3(64), 0, s, c->slots[slot], c->dParams + slot);
  RT_HIP(hipGetLastError());
  return 0;
}
int resetSettled(rtggx_context* c) {
  for (auto& w : c->settled) {
    RT_HIP(hipMemset(w, 0xFF, c->settledWords() * 4));
    RT_HIP(hipMemset2D(w + c->settledPitch + 1u, (size_t)c->settledPitch * 4, 0, (size_t)c->settledY * 4, c->settledX));
  }
  RT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}
// The buffers of input set i (rtggx_context.h InputSet) that it does not have yet: all of them at creation, the ray bins again after
// growBins has released them.  The G-buffer words and the traced images start cleared.
int allocSet(rtggx_context* c, uint32_t i) {
  InputSet& s = c->sets[i];
  const size_t n = (size_t)c->W * c->H, slots = (size_t)c->numBinsMax * c->binSlots;
  for (DevBuf<uint32_t>* p : {&s.normal, &s.depth32, &s.velocity, &s.rtRefl, &s.rtDiff}) if (!*p) RT_HIP(allocFilled(*p, n));
  if (!s.roughMetal) RT_HIP(allocFilled(s.roughMetal, n));
  if (!s.rayQueue) RT_HIP(alloc(s.rayQueue, slots * sizeof(rt::RayRec)));
  if (!s.hitQueue) RT_HIP(alloc(s.hitQueue, slots * 8));
  if (!s.binCount) RT_HIP(allocFilled(s.binCount, (size_t)c->numBinsMax));
  if (!s.splitList) RT_HIP(alloc(s.splitList, (size_t)RT_SPLIT_CAP));
  if (!s.skyRun) RT_HIP(allocFilled(s.skyRun, c->skyTiles));
  c->sky.breakRuns(SkyBreak::SetBuffers);
  s.splitCount = c->largeCountBase + 2 + i;
  if (!s.evRead) RT_HIP(create(s.evRead, RT_EVENT_FLAGS));
  return 0;
}

// rtggx_create's work.  On failure it returns at once: what it created goes with the context.
static int initContext(rtggx_context* c, uint32_t width, uint32_t height, int device) {
  c->device = device; c->W = width; c->H = height; c->rowBegin = 0; c->rowEnd = height;
  const size_t n = (size_t)width * height;
  // Streams and priorities (measured in rounds 1-3, profiles/r02_c_ab_pipeline.txt; the switches that chose between them are gone):
  //   main  high   hit shading, spatial filters, temporal pass + tone map: the longest chain of the three, and the one the others slow down most
  //   B     low    the traversal (one resident workgroup per CU)
  //   C     low    visibility pass + ray generation of the next frame
  //   R     middle vertex upload + tree refit of a deforming mesh; the traversals of odd frames where launches are small
  int prioLeast = 0, prioGreatest = 0;
  RT_HIP(hipDeviceGetStreamPriorityRange(&prioLeast, &prioGreatest));
  const int prioMid = (prioLeast + prioGreatest) / 2;
  RT_HIP(create(c->ownMain, hipStreamNonBlocking, prioGreatest));
  RT_HIP(create(c->ownAS, hipStreamNonBlocking, prioLeast));
  c->streamMain = c->ownMain; c->streamAS = c->ownAS;
  RT_HIP(create(c->ownVis, hipStreamNonBlocking, prioLeast)); c->streamVis = c->ownVis;
  RT_HIP(create(c->streamRefit, hipStreamNonBlocking, prioMid));
  for (Event* e : {&c->evVis, &c->evRefit, &c->evAS, &c->evRT}) RT_HIP(create(*e, RT_EVENT_FLAGS));
  for (auto& f : c->frames) { RT_HIP(create(f.gen, RT_EVENT_FLAGS)); RT_HIP(create(f.trace, RT_EVENT_FLAGS)); }
  for (auto& e : c->tev) RT_HIP(create(e));
  c->rebuildRatio = RT_REFIT_REBUILD_RATIO; c->rebuildSteps = RT_REBUILD_STEPS;      // rtggx_set_refit_policy
  {
    hipDeviceProp_t prop;
    RT_HIP(hipGetDeviceProperties(&prop, device));
    c->numCUs = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
  }
  // one bin of 128 ray slots per 8x8 pixel sub-tile (4 per 16x16 tile): at most 2 rays per pixel
  c->numBinsMax = ((width + 15) / 16) * ((height + 15) / 16) * 4u;
  if (c->numBinsMax < 64u) c->numBinsMax = 64u;            // room for rtggx_trace_rays batches on tiny frames
  c->binSlots = RT_BIN_MIN;      // (all-metal default materials: one ray per pixel; rtggx_update_frame grows the bins with the first metallic below 1)
  c->largeCapacity = 1u << 16;
  // one word per 16x16 tile and a row more (a strip's tiles start at its first row): a VisTarget's dirty words, a set's skyRun
  c->skyTiles = (size_t)((width + 15) / 16) * ((height + 15) / 16 + 1);
  for (auto& b : c->largeTrisBuf) RT_HIP(alloc(b, (size_t)c->largeCapacity * 56));
  RT_HIP(allocFilled(c->largeCountBase, 2 + RT_SETS));
  for (uint32_t i = 0; i < RT_SETS; ++i) { const int r = allocSet(c, i); if (r) return r; }
  for (auto& v : c->vis) { RT_HIP(allocFilled(v.depth, n)); RT_HIP(allocFilled(v.dirty, c->skyTiles, 0xFF)); }
  RT_HIP(allocFilled(c->visDirtyOnes, c->skyTiles, 0xFF));
  c->settledX = (width + 63) / 64; c->settledY = (height + 3) / 4;      // one word per block of the temporal pass and a border (rtggx_context::settled)
  c->settledPitch = (c->settledY + 3u) / 4u * 4u + 2u;                    // (a tone-map block reads the words of four blocks and one either side)
  for (auto& w : c->settled) RT_HIP(alloc(w, c->settledWords()));
  { const int r = resetSettled(c); if (r) return r; }
  RT_HIP(allocFilled(c->backbuffer, n));
  RT_HIP(allocFilled(c->tss[0], n)); RT_HIP(allocFilled(c->tss[1], n)); RT_HIP(allocFilled(c->fltRfl, n)); RT_HIP(allocFilled(c->fltDff, n));
  RT_HIP(allocFilled(c->rayCounter, 512));
  RT_HIP(allocFilled(c->rayCounterBuf, 1792));      // [4][256] per-frame counters + 768 statistics words
  c->lastRayCounter32 = c->rayCounterBuf;
  RT_HIP(allocFilled(c->traceStamps, 8));
  RT_HIP(alloc(c->hostRayCounters, 264)); memset(c->hostRayCounters, 0, 264 * 4); RT_HIP(create(c->evRayCounters, hipEventDisableTiming));   // [0..255] rays; [256] split demand; [258..261] duration and period of a trace launch (two 64-bit words)
  for (auto& b : c->binWorkBuf) RT_HIP(allocFilled(b, (size_t)c->numBinsMax));
  c->selectSet(0);
  c->splitWork = RT_SPLIT_WORK; c->splitMaxShift = RT_SPLIT_MAX_SHIFT;      // rtggx_debug_trace_split
  RT_HIP(allocFilled(c->dEnvMipOffset, 16));
  RT_HIP(allocFilled(c->dummyRecord, 128));
  RT_HIP(allocFilled(c->histReach, 1));
  RT_HIP(allocFilled(c->exchangeTokens, 2 * RT_MAX_PEERS));
  RT_HIP(allocFilled(c->dPeerTable, sizeof(void*) * 2 * RT_MAX_PEERS + 4 * (RT_MAX_PEERS + 1)));
  RT_HIP(allocFilled(c->sh, 27));
  RT_HIP(alloc(c->cosSinTab, 512));
  RT_HIP(alloc(c->dParams, RT_SLOTS));
  {  // cos/sin(2*pi*s/256): double libm, rounded once (RayTracing.hlsl:94,100 with xi.x = s/256, :391)
    float tab[512];
    for (int s = 0; s < 256; ++s) { const double phi = 2.0 * 3.14159265358979323846 * (double)s / 256.0; tab[s] = (float)cos(phi); tab[256 + s] = (float)sin(phi); }
    RT_HIP(hipMemcpy(c->cosSinTab, tab, sizeof tab, hipMemcpyHostToDevice));
  }
  // default materials, RayTracer.cpp:134-139
  const float bc0[4] = {0.95f, 0.93f, 0.88f, 1.0f}, bc1[4] = {1.0f, 0.71f, 0.29f, 1.0f};
  const float rm0[4] = {0.5f, 1.0f, 0.0f, 0.0f}, rm1[4] = {0.16f, 1.0f, 0.0f, 0.0f};
  memcpy(c->material.BaseColors[0], bc0, 16); memcpy(c->material.BaseColors[1], bc1, 16);
  memcpy(c->material.RoughMetals[0], rm0, 16); memcpy(c->material.RoughMetals[1], rm1, 16);
  memset(c->invWorld, 0, sizeof c->invWorld);
  for (int i = 0; i < 2; ++i) for (int k = 0; k < 4; ++k) c->invWorld[i][k * 5] = 1.0f;
  memset(c->slots, 0, sizeof c->slots);
  { const int r = setMeshImpl(c, RTGGX_GROUND, &kGroundVerts[0][0], 24, kGroundIdx, 36); if (r) return r; }
  // hipMemset of device memory does not wait on the host, and the null stream it runs on is not ordered against this context's
  // (non-blocking) streams: nothing of the first frame may overtake a clear
  RT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}
// What N > 1 samples per pixel need (rtggx_set_samples_per_pixel): allocated with the first N > 1.
int allocSamples(rtggx_context* c) {
  if (c->sppAcc && c->sppParams) return 0;
  const size_t n = (size_t)c->W * c->H;
  if (!c->evSpp) RT_HIP(create(c->evSpp, hipEventDisableTiming));
  if (!c->sppParams) RT_HIP(alloc(c->sppParams, RT_SLOTS * RTGGX_MAX_SAMPLES_PER_PIXEL));
  if (!c->sppAcc) {
    RT_HIP(allocFilled(c->sppAcc, n * 2u * 3u));
    RT_HIP(hipStreamSynchronize(nullptr));      // (the clear runs on the null stream, which this context's streams are not ordered against)
  }
  return 0;
}
// The table of a sample set of M > 256 members (rtggx_set_sample_set): M pairs {cos, sin}(2 pi s / M), double libm rounded once -- the rule of
// the 256-entry table, whose entry k is this one's entry k M / 256 bit for bit (the quotient s / M is the same double).  Made once per size.
int allocSampleTable(rtggx_context* c, uint32_t m) {
  DevBuf<float>& tab = c->cosSinWide[rtggx_context::sampleSetSlot(m)];
  if (tab) return 0;
  std::vector<float> host(2u * (size_t)m);
  for (uint32_t s = 0; s < m; ++s) { const double phi = 2.0 * 3.14159265358979323846 * (double)s / (double)m; host[2u * s] = (float)cos(phi); host[2u * s + 1u] = (float)sin(phi); }
  DevBuf<float> d;
  hipError_t e = alloc(d, host.size());
  if (e == hipSuccess) e = hipMemcpy(d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { setError("rtggx_set_sample_set: %s (%zu bytes for the table of %u samples)", hipGetErrorString(e), host.size() * sizeof(float), m); return -2; }
  tab = std::move(d);
  return 0;
}
// What accumulation needs (rtggx_set_accumulation): the two sums and the mean image, 2 x 16 + 8 bytes per pixel of the full frame, zeroed;
// allocated with the first enable -- all three or none.
int allocAccumulation(rtggx_context* c) {
  if (c->accRefl) return 0;
  const size_t n = (size_t)c->W * c->H;
  DevBuf<float4> a0, a1; DevBuf<uint2> cv;
  hipError_t e = alloc(a0, n);
  if (e == hipSuccess) e = alloc(a1, n);
  if (e == hipSuccess) e = alloc(cv, n);
  if (e == hipSuccess) e = hipMemset(a0, 0, n * 16);
  if (e == hipSuccess) e = hipMemset(a1, 0, n * 16);
  if (e == hipSuccess) e = hipMemset(cv, 0, n * 8);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // (the clears run on the null stream, which this context's streams are not ordered against)
  if (e != hipSuccess) { setError("rtggx_set_accumulation: %s (%zu bytes for the sums and the mean image)", hipGetErrorString(e), n * 40); return -2; }
  c->accRefl = std::move(a0); c->accDiff = std::move(a1); c->converged = std::move(cv);
  return 0;
}
// What scoring needs (rtggx_set_reference, rtggx_set_scoring; score.hip): the reference image, 8 bytes per pixel of the full frame, with the
// first reference; the ring of records and the tree's partial sums -- sized for the full frame, whatever strip is scored -- with the first
// enable, all of them or none.
static int allocReference(rtggx_context* c, const char* who) {
  if (c->reference) return 0;
  const size_t n = (size_t)c->W * c->H;
  const hipError_t e = alloc(c->reference, n);
  if (e != hipSuccess) { setError("%s: %s (%zu bytes for the reference image)", who, hipGetErrorString(e), n * 8); return -2; }
  return 0;
}
static int allocScoring(rtggx_context* c) {
  if (c->scoreRing) return 0;
  const size_t chunks = ((size_t)c->W * c->H + RT_SCORE_CHUNK - 1u) / RT_SCORE_CHUNK;
  uint32_t stride = 1u; while (stride < chunks) stride <<= 1;
  const size_t half = stride > 1u ? stride / 2u : 1u;
  DevBuf<double> p0, p1; DevBuf<uint32_t> counts; DevBuf<RtggxScore> ring;
  hipError_t e = alloc(p0, (size_t)RT_SCORE_SUMS * stride);
  if (e == hipSuccess) e = alloc(p1, (size_t)RT_SCORE_SUMS * half);
  if (e == hipSuccess) e = alloc(counts, 3u * (size_t)stride);
  if (e == hipSuccess) e = allocFilled(ring, RTGGX_SCORE_RING);
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // (the clear runs on the null stream, which this context's streams are not ordered against)
  if (e != hipSuccess) { setError("rtggx_set_scoring: %s (the ring of records and the partial sums)", hipGetErrorString(e)); return -2; }
  c->scorePartial[0] = std::move(p0); c->scorePartial[1] = std::move(p1); c->scoreCounts = std::move(counts); c->scoreRing = std::move(ring); c->scoreStride = stride;
  return 0;
}
}  // namespace rt
using namespace rt;

extern "C" {
const char* rtggx_last_error(void) { return rt::g_err; }

int rtggx_create(rtggx_context** out, uint32_t width, uint32_t height, int device) {
  if (!out || width == 0 || height == 0 || width > 16384 || height > 16384) { setError("rtggx_create: bad arguments"); return -1; }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { setError("rtggx_create: no HIP device available (this library has no CPU path)"); return -2; }
  if (device < 0 || device >= count) { setError("rtggx_create: device %d out of range (%d devices)", device, count); return -1; }
  RT_HIP(hipSetDevice(device));
  rtggx_context* c = new rtggx_context();
  const int r = initContext(c, width, height, device);
  if (r) { rtggx_destroy(c); return r; }      // (what was created goes with it)
  *out = c;
  return 0;
}

// Also the end of a partly created context (rtggx_create).  Nothing may still run when the members release what they own.
void rtggx_destroy(rtggx_context* c) {
  if (!c) return;
  hipSetDevice(c->device);
  hipDeviceSynchronize();
  delete c;
}

int rtggx_set_strip(rtggx_context* c, uint32_t rowBegin, uint32_t rowEnd) {
  RT_CHECK_CTX(c);
  if (rowBegin > rowEnd || rowEnd > c->H) { setError("rtggx_set_strip: bad rows [%u,%u) for height %u", rowBegin, rowEnd, c->H); return -1; }
  if (c->rayRate != 1u && (rowBegin > 0u || rowEnd < c->H)) { setError("rtggx_set_strip: rows [%u,%u) of %u: a context tracing one pixel in %u renders whole frames", rowBegin, rowEnd, c->H, c->rayRate); return -1; }
  if ((c->sampleMap >= 0 || c->sampleMapRequested >= 0) && (rowBegin > 0u || rowEnd < c->H)) { setError("rtggx_set_strip: rows [%u,%u) of %u on a context with a sample map (rtggx_set_sample_map): a strip's tiles count from its first row, a block would no longer be a bin -- whole frames only", rowBegin, rowEnd, c->H); return -1; }
  if ((c->lightVis || c->lightVisRequested) && (rowBegin > 0u || rowEnd < c->H)) { setError("rtggx_set_strip: rows [%u,%u) of %u on a context with the pick's visibility records (rtggx_set_light_pick_visibility): a reprojected tap may lie in another rank's rows -- whole frames only", rowBegin, rowEnd, c->H); return -1; }
  if ((c->lightListVis || c->lightListVisRequested) && (rowBegin > 0u || rowEnd < c->H)) { setError("rtggx_set_strip: rows [%u,%u) of %u on a context with a list's visibility records (rtggx_set_light_list_visibility): a reprojected tap may lie in another rank's rows -- whole frames only", rowBegin, rowEnd, c->H); return -1; }
  c->rowBegin = rowBegin; c->rowEnd = rowEnd; c->toneMapDone = false;
  c->sky.breakRuns(SkyBreak::Strip);
  return 0;
}

// Multi-GPU strips: the caller exchanges `rows` rows of TemporalSSOut beyond each strip edge between frames.  The
// temporal pass reports reprojections that read further than that (rtggx_history_overreach): such frames differ from the
// single-GPU frame, and the caller widens the apron or reports it.
int rtggx_set_history_apron(rtggx_context* c, uint32_t rows) {
  RT_CHECK_CTX(c);
  c->historyApron = rows;
  return 0;
}
int rtggx_history_overreach(rtggx_context* c, uint32_t* rows, int reset) {
  RT_CHECK_CTX(c);
  if (!rows) { setError("rtggx_history_overreach: null result"); return -1; }
  RT_HIP(syncStreams(c));
  RT_HIP(hipMemcpy(rows, c->histReach, 4, hipMemcpyDeviceToHost));
  if (reset) { RT_HIP(hipMemset(c->histReach, 0, 4)); RT_HIP(hipStreamSynchronize(nullptr)); }
  return 0;
}

int rtggx_set_stream(rtggx_context* c, void* stream) {
  RT_CHECK_CTX(c);
  RT_HIP(syncStreams(c));
  if (stream) { c->streamMain = (hipStream_t)stream; c->externalStream = true; }
  else { c->streamMain = c->ownMain; c->externalStream = false; }
  c->sppStream = nullptr; c->sunHitStream = nullptr;      // (everything has ended; the stream given up may not outlive this call)
  if (!c->asyncCompute) c->streamAS = c->streamMain;
  return 0;
}

// Multi-GPU strips: the history images of ALL ranks, mapped into this process, for the temporal pass's taps beyond the exchanged apron
// ("N-strip output == 1-strip output on every buffer"; the reference samples its one history texture anywhere,
// CSTemporalSS.hlsl:259-265).  Every rank allocates full-size targets, so rank r's TemporalSSOut[p] holds the rows r owns at the same
// offsets as this rank's own image does; a tap at row y outside [b - apron, e + apron) is read from the image of the rank whose strip
// holds y.  `bounds`: world + 1 ascending rows (rank r owns [bounds[r], bounds[r + 1])); tss0 / tss1: world device pointers each, valid in
// THIS process -- another context's rtggx_buffer_ptr in the same process, or what rtggx_history_ipc_open returned for another process's
// rtggx_history_ipc_export.  The entries of this rank itself may be its own pointers or null.
// ORDERING is the caller's, and the per-frame exchange already provides it where it has a message in each direction between two ranks
// (include/rtggx.h): rank A's temporal pass of frame f + 1 may read rank B's image once B's temporal pass of frame f has ended (A's
// receive from B in the exchange of frame f), and B's H filter of frame f + 2, which reuses that image as scratch, waits for A's temporal
// pass of frame f + 1 (B's receive from A in the exchange of frame f + 1) -- both on the main streams the exchange is issued on.
int rtggx_set_history_peers(rtggx_context* c, uint32_t world, const uint32_t* bounds, void* const* tss0, void* const* tss1) {
  RT_CHECK_CTX(c);
  if (world == 0u) { RT_HIP(syncStreams(c)); c->peerWorld = 0u; return 0; }
  if (world > RT_MAX_PEERS || !bounds || !tss0 || !tss1) { setError("rtggx_set_history_peers: 1 .. %d ranks, boundaries and two pointer lists", RT_MAX_PEERS); return -1; }
  if (bounds[0] != 0u || bounds[world] != c->H) { setError("rtggx_set_history_peers: boundaries must run from 0 to the frame height %u", c->H); return -1; }
  for (uint32_t r = 0; r < world; ++r) if (bounds[r] > bounds[r + 1]) { setError("rtggx_set_history_peers: boundaries must ascend"); return -1; }
  RT_HIP(syncStreams(c));
  struct { const void* tss[2][RT_MAX_PEERS]; uint32_t bounds[RT_MAX_PEERS + 1]; } table;
  memset(&table, 0, sizeof table);
  for (uint32_t r = 0; r < world; ++r) {
    const bool own = bounds[r] <= c->rowBegin && c->rowEnd <= bounds[r + 1] && c->rowEnd > c->rowBegin;
    table.tss[0][r] = tss0[r] ? tss0[r] : own ? (void*)c->tss[0] : nullptr; table.tss[1][r] = tss1[r] ? tss1[r] : own ? (void*)c->tss[1] : nullptr;
    if (bounds[r + 1] > bounds[r] && (!table.tss[0][r] || !table.tss[1][r])) { setError("rtggx_set_history_peers: no history images for rank %u", r); return -1; }
  }
  for (uint32_t r = 0; r <= world; ++r) table.bounds[r] = bounds[r];
  for (uint32_t r = world + 1; r <= RT_MAX_PEERS; ++r) table.bounds[r] = c->H;
  static_assert(sizeof table == sizeof(void*) * 2 * RT_MAX_PEERS + 4 * (RT_MAX_PEERS + 1) + 4 || sizeof table == sizeof(void*) * 2 * RT_MAX_PEERS + 4 * (RT_MAX_PEERS + 1), "peer table layout");
  RT_HIP(hipMemcpy(c->dPeerTable, &table, sizeof(void*) * 2 * RT_MAX_PEERS + 4 * (RT_MAX_PEERS + 1), hipMemcpyHostToDevice));
  c->peerWorld = world;
  return 0;
}
// One process per GPU: the two history images as inter-process handles (2 x 64 bytes: hipIpcMemHandle_t of TemporalSSOut[0], [1]) ...
int rtggx_history_ipc_export(rtggx_context* c, void* handles, size_t bytes) {
  RT_CHECK_CTX(c);
  static_assert(sizeof(hipIpcMemHandle_t) == RTGGX_IPC_HANDLE_BYTES, "hipIpcMemHandle_t size");
  if (!handles || bytes < 2 * sizeof(hipIpcMemHandle_t)) { setError("rtggx_history_ipc_export: room for two %zu-byte handles", sizeof(hipIpcMemHandle_t)); return -1; }
  hipIpcMemHandle_t h[2];
  for (int p = 0; p < 2; ++p) RT_HIP(hipIpcGetMemHandle(&h[p], c->tss[p]));
  memcpy(handles, h, sizeof h);
  return 0;
}
// ... and another rank's handles opened in this process: two device pointers for rtggx_set_history_peers (unmapped with the context).
int rtggx_history_ipc_open(rtggx_context* c, const void* handles, size_t bytes, void** tss0, void** tss1) {
  RT_CHECK_CTX(c);
  if (!handles || bytes < 2 * sizeof(hipIpcMemHandle_t) || !tss0 || !tss1) { setError("rtggx_history_ipc_open: bad arguments"); return -1; }
  hipIpcMemHandle_t h[2]; memcpy(h, handles, sizeof h);
  void* p[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k) {
    IpcMapping mapped;
    RT_HIP(hipIpcOpenMemHandle(mapped.put(), h[k], hipIpcMemLazyEnablePeerAccess));
    p[k] = mapped;
    c->ipcMapped.push_back(std::move(mapped));
  }
  *tss0 = p[0]; *tss1 = p[1];
  return 0;
}

int rtggx_get_stream(rtggx_context* c, void** stream) {
  RT_CHECK_CTX(c);
  if (!stream) { setError("rtggx_get_stream: null"); return -1; }
  *stream = (void*)c->streamMain;
  return 0;
}

// The sample's [A] toggle / m_asyncCompute (RayTracedGGX.cpp:304-353 vs the single command list of :513-556).  Off: every
// pass of a frame is issued to ONE stream in submission order -- no stream B, no stream C, no overlap between the
// ray-tracing half of one frame and the denoising half of the previous one.  Results are identical either way.
int rtggx_set_async_compute(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  if ((enable != 0) == c->asyncCompute) return 0;
  RT_HIP(syncStreams(c));
  c->asyncCompute = enable != 0; c->sppStream = nullptr; c->sunHitStream = nullptr;
  c->streamAS = c->asyncCompute ? c->ownAS : c->streamMain;
  c->streamVis = c->asyncCompute ? c->ownVis : nullptr;
  c->evVisStream = nullptr; for (auto& f : c->frames) f.genFrame = 0u;
  return 0;
}

// Quarter-rate tracing (raytrace.hip rayGenKernel, reconstructKernel; DESIGN.md "Quarter-rate tracing").  Whole frames only: a strip's
// apron rows and the exchanged history are not defined for it (yet).  A bin covers other pixels at the other rate, so what the adaptive
// split knows about its bins -- the cost record, the demand that sizes the split list, the ray count behind the placement -- starts afresh.
int rtggx_set_ray_rate(rtggx_context* c, uint32_t pixelsPerRay) {
  RT_CHECK_CTX(c);
  if (pixelsPerRay != 1u && pixelsPerRay != 4u) { setError("rtggx_set_ray_rate: %u pixels per ray: 1 or 4", pixelsPerRay); return -1; }
  if (pixelsPerRay != 1u && c->samplesRequested > 1u) { setError("rtggx_set_ray_rate: rate %u on a context tracing %u samples per pixel (rtggx_set_samples_per_pixel): one asks for fewer rays, the other for more", pixelsPerRay, c->samplesRequested); return -1; }
  if (pixelsPerRay != 1u && c->accumulateRequested) { setError("rtggx_set_ray_rate: rate %u on an accumulating context (rtggx_set_accumulation): three quarters of such a frame are interpolations", pixelsPerRay); return -1; }
  if (pixelsPerRay != 1u && c->sunRequested.on) { setError("rtggx_set_ray_rate: rate %u on a context with a sun (rtggx_set_sun): three quarters of such a frame are interpolations", pixelsPerRay); return -1; }
  if (pixelsPerRay != 1u && c->lightsRequested.count) { setError("rtggx_set_ray_rate: rate %u on a context with lights (rtggx_set_lights): three quarters of such a frame are interpolations", pixelsPerRay); return -1; }
  if (pixelsPerRay != 1u && c->lightListRequested.count) { setError("rtggx_set_ray_rate: rate %u on a context with a light list (rtggx_set_light_list): three quarters of such a frame are interpolations", pixelsPerRay); return -1; }
  if (pixelsPerRay != 1u && (c->rowBegin > 0u || c->rowEnd < c->H)) { setError("rtggx_set_ray_rate: rate %u on a strip (rows [%u,%u) of %u): whole frames only", pixelsPerRay, c->rowBegin, c->rowEnd, c->H); return -1; }
  if (pixelsPerRay == c->rayRate) return 0;
  RT_HIP(syncStreams(c));
  c->rayRate = pixelsPerRay;
  for (auto& b : c->binWorkBuf) RT_HIP(hipMemset(b, 0, (size_t)c->numBinsMax * 4));
  RT_HIP(hipDeviceSynchronize());
  c->splitDemand = 0u; c->rayCountersInFlight = false; c->lastFrameRays = 0xFFFFFFFFu; c->traceLaunches = 0u;
  return 0;
}

// Recursion depth (raytrace.hip launchShade; DESIGN.md "Recursion depth"): 1..4 levels of rays per path.  The levels after the first reuse
// the frame's bins in place and its trace kernel; nothing is allocated.  Taken over by the next rtggx_render_visibility.
int rtggx_set_max_recursion_depth(rtggx_context* c, uint32_t depth) {
  RT_CHECK_CTX(c);
  if (depth < 1u || depth > RTGGX_MAX_RECURSION_DEPTH) { setError("rtggx_set_max_recursion_depth: depth %u: 1 to %u", depth, RTGGX_MAX_RECURSION_DEPTH); return -1; }
  c->depthRequested = depth;
  return 0;
}

// Samples per pixel (raytrace.hip launchShadeSamples; DESIGN.md "Samples per pixel"): 1, 2, 4 or 8.  Taken over by the next
// rtggx_render_visibility.  The first N > 1 allocates the sums and the samples' constants (allocSamples); N = 1 never does.
// No synchronisation and no end of the still-sky runs (rtggx_context.h RT_SKY_PREV_RUN): nothing a run vouches for changes with N.  A tile
// without a surface has no covered pixel, so no sample pass stores anything in it -- its G-buffer and image words are ray generation's at
// every N (background: the environment, no ray, no averaging); its bins are never written by a sample pass (the sample generation, the
// shading passes and the resolve leave at the tile's word like every kernel behind the visibility pass; where the words read "all ones"
// a bin without a covered pixel gets the count 0 without a mark -- the value the run vouches for); and the cost records and split lists
// are ray generation's and the level-0 traversal's alone, which N does not touch.
int rtggx_set_samples_per_pixel(rtggx_context* c, uint32_t samples) {
  RT_CHECK_CTX(c);
  if (samples != 1u && samples != 2u && samples != 4u && samples != 8u) { setError("rtggx_set_samples_per_pixel: %u samples per pixel: 1, 2, 4 or %u", samples, RTGGX_MAX_SAMPLES_PER_PIXEL); return -1; }
  if (samples > 1u && c->rayRate != 1u) { setError("rtggx_set_samples_per_pixel: %u samples per pixel on a context tracing one pixel in %u (rtggx_set_ray_rate): one asks for more rays, the other for fewer", samples, c->rayRate); return -1; }
  if (samples > 1u) { const int r = allocSamples(c); if (r) return r; }
  c->samplesRequested = samples;
  return 0;
}

// Sample-set size (raytrace.hip sampleParamWide; DESIGN.md "Sample-set size"): M = 256 (the reference's set: the kernels and the table of a
// context that never calls this) or a power of two up to 65536, which selects the set-size-aware variants of the three kernels that take a
// sample and a table of M {cos, sin} pairs (allocSampleTable).  Taken over by the next rtggx_render_visibility; synchronises like
// rtggx_set_ray_rate.  No end of the still-sky runs -- a pixel without a surface takes no sample, and bins, cost records and split lists
// do not depend on M -- and no reset of an accumulation.
int rtggx_set_sample_set(rtggx_context* c, uint32_t size) {
  RT_CHECK_CTX(c);
  if (size < RTGGX_MIN_SAMPLE_SET || size > RTGGX_MAX_SAMPLE_SET || (size & (size - 1u)) != 0u) { setError("rtggx_set_sample_set: %u samples: a power of two from %u to %u", size, RTGGX_MIN_SAMPLE_SET, RTGGX_MAX_SAMPLE_SET); return -1; }
  if (size == c->sampleSetRequested) return 0;
  RT_HIP(syncStreams(c));
  if (size > RTGGX_MIN_SAMPLE_SET) { const int r = allocSampleTable(c, size); if (r) return r; }
  c->sampleSetRequested = size;
  return 0;
}

// Progressive accumulation (raytrace.hip accumulateKernel; DESIGN.md "Progressive accumulation").  Taken over by the next
// rtggx_render_visibility; the first enable allocates (allocAccumulation), off never does.  No synchronisation and no end of the still-sky
// runs: the kernel only reads the current set's traced images and the frame's visibility words, behind everything that writes them.
int rtggx_set_accumulation(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  if (enable && c->rayRate != 1u) { setError("rtggx_set_accumulation: on a context tracing one pixel in %u (rtggx_set_ray_rate): three quarters of such a frame are interpolations", c->rayRate); return -1; }
  if (enable) { const int r = allocAccumulation(c); if (r) return r; }
  c->accumulateRequested = enable != 0;
  return 0;
}
// The sun (include/rtggx.h).  The direction is normalised in double and rounded once; (NULL, NULL) or E = 0 turns the sun off.  A refused call
// leaves what the context had.  The first call that turns it on allocates the queue: local owners first, members when all exist.  No
// synchronisation, no end of a still-sky run, no reset of an accumulation: no sky texel depends on the sun, and the request takes effect with
// the next rtggx_render_visibility.
int rtggx_set_sun(rtggx_context* c, const float direction[3], const float irradiance[3]) {
  RT_CHECK_CTX(c);
  if (!direction && !irradiance) { c->sunRequested.on = false; return 0; }
  if (!direction || !irradiance) { setError("rtggx_set_sun: a direction without an irradiance, or the reverse"); return -1; }
  const double x = direction[0], y = direction[1], z = direction[2], len = std::sqrt(x * x + y * y + z * z);
  if (!std::isfinite(len) || !(len > 0.0)) { setError("rtggx_set_sun: the direction (%g, %g, %g) has no finite, non-zero length", x, y, z); return -1; }
  for (int k = 0; k < 3; ++k) if (!std::isfinite(irradiance[k]) || irradiance[k] < 0.0f) { setError("rtggx_set_sun: irradiance component %d is %g: finite and not negative", k, (double)irradiance[k]); return -1; }
  const bool on = irradiance[0] > 0.0f || irradiance[1] > 0.0f || irradiance[2] > 0.0f;
  if (on && c->rayRate != 1u) { setError("rtggx_set_sun: on a context tracing one pixel in %u (rtggx_set_ray_rate): three quarters of such a frame are interpolations", c->rayRate); return -1; }
  if (on) { bool filled = false; const int r = c->sunQueue.ensure(c->numBinsMax, RT_BIN_MIN, false, filled); if (r) return r; }      // (the call does not synchronise: see above)
  rtggx_context::Sun sun;
  sun.on = on;
  sun.L[0] = (float)(x / len); sun.L[1] = (float)(y / len); sun.L[2] = (float)(z / len);
  for (int k = 0; k < 3; ++k) sun.E[k] = irradiance[k];
  {  // the disk's frame (rtggx_set_sun_angle): double arithmetic on the stored fp32 L, T and B each rounded once
    const double l[3] = {sun.L[0], sun.L[1], sun.L[2]};
    int a = 0;
    for (int k = 1; k < 3; ++k) if (std::fabs(l[k]) < std::fabs(l[a])) a = k;      // the axis of the smallest |L_i|, ties to the lowest index
    const int a1 = (a + 1) % 3, a2 = (a + 2) % 3;
    double t[3]; t[a] = 0.0; t[a1] = -l[a2]; t[a2] = l[a1];                         // cross(e_a, L)
    const double tl = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int k = 0; k < 3; ++k) t[k] /= tl;
    const double b[3] = {l[1] * t[2] - l[2] * t[1], l[2] * t[0] - l[0] * t[2], l[0] * t[1] - l[1] * t[0]};      // cross(L, T)
    for (int k = 0; k < 3; ++k) { sun.T[k] = (float)t[k]; sun.B[k] = (float)b[k]; }
  }
  c->sunRequested = sun;
  return 0;
}
// The sun's angular radius (include/rtggx.h).  Only the value and k = 1 - cos of it are kept, whether or not a sun is set; nothing is
// allocated, and it takes effect with the next rtggx_render_visibility.  No synchronisation, no end of a still-sky run, no reset of an
// accumulation, as for the sun itself.
int rtggx_set_sun_angle(rtggx_context* c, float degrees) {
  RT_CHECK_CTX(c);
  if (!(degrees >= 0.0f && degrees <= RTGGX_MAX_SUN_ANGLE_DEGREES)) { setError("rtggx_set_sun_angle: %g degrees: the radius of the disk, 0 to %g", (double)degrees, (double)RTGGX_MAX_SUN_ANGLE_DEGREES); return -1; }
  c->sunAngleRequested.degrees = degrees;
  c->sunAngleRequested.k = (float)(1.0 - std::cos((double)degrees * 3.14159265358979323846 / 180.0));
  return 0;
}
// The sun at the surfaces the paths hit (include/rtggx.h).  Only the value is kept: it is stored whether or not a sun is set, allocates nothing
// here (the first frame that has both on does: lighting.hip beginSunHits) and takes effect with the next rtggx_render_visibility.  No
// synchronisation, no end of a still-sky run, no reset of an accumulation, as for the sun itself.
int rtggx_set_sun_reflections(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  if (enable != 0 && enable != 1) { setError("rtggx_set_sun_reflections: %d: 0 or 1", enable); return -1; }
  c->sunReflectionsRequested = enable == 1;
  return 0;
}
// One light of a list as both setters check it (rtggx_set_lights, rtggx_set_light_list: fn names the caller in the message): l is the copy the
// context keeps, its axis normalised in double and rounded once, its pad zero
static int checkLight(const char* fn, uint32_t i, RtggxLight& l) {
  static_assert(sizeof(RtggxLight) == sizeof(LightWords), "RtggxLight is sixteen floats");
  LightWords w; memcpy(&w, &l, sizeof w);
  const uint32_t reason = lightCheck(w, LIGHT_KINDS_ALL);      // rt_light_check.h: the one statement of the rule, the device's as well
  const int k = (int)(reason >> 8);
  switch (reason & 0xFFu) {
    case LIGHT_OK: break;
    case LIGHT_BAD_POSITION: setError("%s: light %u: position component %d is %g: finite", fn, i, k, (double)l.position[k]); return -1;
    case LIGHT_BAD_RANGE: setError("%s: light %u: a range of %g: finite and above 0", fn, i, (double)l.range); return -1;
    case LIGHT_BAD_INTENSITY: setError("%s: light %u: intensity component %d is %g: finite and not negative", fn, i, k, (double)l.intensity[k]); return -1;
    case LIGHT_BAD_RADIUS: setError("%s: light %u: a radius of %g: finite, not negative and below the range %g", fn, i, (double)l.radius, (double)l.range); return -1;
    case LIGHT_BAD_AXIS: setError("%s: light %u: the axis (%g, %g, %g) has no finite, non-zero length", fn, i, (double)l.axis[0], (double)l.axis[1], (double)l.axis[2]); return -1;
    case LIGHT_BAD_COSINES: setError("%s: light %u: cosines %g (outer) and %g (inner): -1 < outer < inner <= 1", fn, i, (double)l.cos_outer, (double)l.cos_inner); return -1;
    default: setError("%s: light %u: cos_outer is %g: at most -1 (no cone), or -1 < outer < inner <= 1", fn, i, (double)l.cos_outer); return -1;
  }
  lightNormaliseAxis(w);
  memcpy(&l, &w, sizeof w);
  l.pad[0] = l.pad[1] = l.pad[2] = 0.0f;
  return 0;
}
// Local lights (include/rtggx.h).  The list is checked as a whole and copied; a cone's axis is normalised in double and rounded once, the sun's
// rule.  (NULL, 0) turns the lights off.  A refused call leaves what the context had.  Nothing is allocated here (the first frame with lights
// does: lighting.hip launchLights).  No synchronisation, no end of a still-sky run, no reset of an accumulation, as for the sun.
int rtggx_set_lights(rtggx_context* c, const RtggxLight* lights, uint32_t count) {
  RT_CHECK_CTX(c);
  if (count > RTGGX_MAX_LIGHTS) { setError("rtggx_set_lights: %u lights: at most %u", count, RTGGX_MAX_LIGHTS); return -1; }
  if (count && !lights) { setError("rtggx_set_lights: %u lights at a null pointer", count); return -1; }
  if (count && c->lightListRequested.count) { setError("rtggx_set_lights: %u lights on a context that holds a light list of %u (rtggx_set_light_list): the context holds one or the other", count, c->lightListRequested.count); return -1; }
  if (count && c->rayRate != 1u) { setError("rtggx_set_lights: on a context tracing one pixel in %u (rtggx_set_ray_rate): three quarters of such a frame are interpolations", c->rayRate); return -1; }
  rtggx_context::Lights next;
  for (uint32_t i = 0; i < count; ++i) {
    RtggxLight l = lights[i];
    if (checkLight("rtggx_set_lights", i, l)) return -1;
    next.l[i] = l;
  }
  next.count = count;
  c->lightsRequested = next;
  c->lightVisSeq0 = c->lightVisSeq;      // rtggx_set_light_pick_visibility: a reset -- the next acting frame has no valid history
  return 0;
}
// A light list beyond eight (include/rtggx.h): rtggx_set_lights' checks over up to RTGGX_MAX_LIGHT_LIST lights, copied; (NULL, 0) clears the
// list.  A refused call leaves what the context had.  Nothing is allocated here: the next rtggx_render_visibility uploads the list
// (lighting.hip uploadLightList).  No end of a still-sky run, no reset of an accumulation, as for the lights.
int rtggx_set_light_list(rtggx_context* c, const RtggxLight* lights, uint32_t count) {
  RT_CHECK_CTX(c);
  if (count > RTGGX_MAX_LIGHT_LIST) { setError("rtggx_set_light_list: %u lights: at most %u", count, RTGGX_MAX_LIGHT_LIST); return -1; }
  if (count && !lights) { setError("rtggx_set_light_list: %u lights at a null pointer", count); return -1; }
  if (count && c->lightsRequested.count) { setError("rtggx_set_light_list: a list of %u on a context that holds %u lights (rtggx_set_lights): the context holds one or the other", count, c->lightsRequested.count); return -1; }
  if (count && c->rayRate != 1u) { setError("rtggx_set_light_list: on a context tracing one pixel in %u (rtggx_set_ray_rate): three quarters of such a frame are interpolations", c->rayRate); return -1; }
  rtggx_context::LightList next;
  next.l.resize(count);
  for (uint32_t i = 0; i < count; ++i) {
    RtggxLight l = lights[i];
    if (checkLight("rtggx_set_light_list", i, l)) return -1;
    next.l[i] = l;
  }
  c->lightListVisSeq0 = c->lightListVisSeq;      // rtggx_set_light_list_visibility: a reset -- the next acting frame has no valid history
  if (!count && !c->lightListRequested.count) return 0;      // nothing held, nothing asked for: the context stays as it is
  next.count = count;
  next.version = ++c->lightListVersions;
  c->lightListRequested = std::move(next);
  return 0;
}
// Lights that move, the host path (include/rtggx.h): the range is checked as rtggx_set_light_list checks it and copied into the list the
// context holds; nothing reaches the device here -- the next rtggx_render_visibility (or an rtggx_update_light_list_device in front of
// it) stages what has changed and copies it asynchronously into a version no frame in flight reads (lighting.hip "Moving light
// lists").  No wait, no end of a still-sky run, no reset of an accumulation, and s0 stays: the records' history is kept.
int rtggx_update_light_list(rtggx_context* c, const RtggxLight* lights, uint32_t first, uint32_t count) {
  RT_CHECK_CTX(c);
  rtggx_context::LightList& L = c->lightListRequested;
  if (!L.count) { setError("rtggx_update_light_list: the context holds no light list (rtggx_set_light_list)"); return -1; }
  if (first > L.count || count > L.count - first) { setError("rtggx_update_light_list: lights %u .. %u of a list of %u: the count of a list never changes", first, first + count, L.count); return -1; }
  if (!count) return 0;
  if (!lights) { setError("rtggx_update_light_list: %u lights at a null pointer", count); return -1; }
  std::vector<RtggxLight> next(lights, lights + count);
  for (uint32_t i = 0; i < count; ++i) if (checkLight("rtggx_update_light_list", first + i, next[i])) return -1;
  std::copy(next.begin(), next.end(), L.l.begin() + first);
  if (L.version == c->lightListStored) {      // (a list set and not yet uploaded carries them in its own upload)
    const bool none = c->lightListDirtyLo >= c->lightListDirtyHi;
    c->lightListDirtyLo = none ? first : std::min(c->lightListDirtyLo, first);
    c->lightListDirtyHi = none ? first + count : std::max(c->lightListDirtyHi, first + count);
  }
  return 0;
}
// How often rtggx_render_visibility has waited for every stream of the context since the last reset: what makes "no drain" testable
int rtggx_debug_visibility_drains(rtggx_context* c, uint32_t* drains, int reset) {
  RT_CHECK_CTX(c);
  if (!drains) { setError("rtggx_debug_visibility_drains: a null pointer"); return -1; }
  if (reset != 0 && reset != 1) { setError("rtggx_debug_visibility_drains: reset %d: 0 or 1", reset); return -1; }
  *drains = c->visibilityDrains;
  if (reset) c->visibilityDrains = 0u;
  return 0;
}
// The kept lights per 8x8 block of the last frame's primary pass with a list, behind everything the context has enqueued
int rtggx_read_light_list_counts(rtggx_context* c, uint32_t* out, size_t bytes) {
  RT_CHECK_CTX(c);
  if (c->rowBegin > 0u || c->rowEnd < c->H) { setError("rtggx_read_light_list_counts: on a strip (rows [%u,%u) of %u): whole frames only", c->rowBegin, c->rowEnd, c->H); return -1; }
  if (!c->lightListKept || !c->lightListFrame) { setError("rtggx_read_light_list_counts: no counts yet: they exist from the first frame with a list (rtggx_set_light_list)"); return -1; }
  const size_t want = (size_t)((c->H + 7u) / 8u) * ((c->W + 7u) / 8u) * 4u;
  if (!out || bytes != want) { setError("rtggx_read_light_list_counts: %zu bytes at %p: %u x %u blocks of 4 bytes are %zu", bytes, (void*)out, (c->W + 7u) / 8u, (c->H + 7u) / 8u, want); return -1; }
  RT_HIP(syncStreams(c));
  RT_HIP(hipMemcpy(out, c->lightListKept, want, hipMemcpyDeviceToHost));
  return 0;
}
// 1 (default): the cull; 0: every casting light is kept wherever a block has a point -- the same images, the time of the walk over all lights
int rtggx_debug_light_list_cull(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  if (enable != 0 && enable != 1) { setError("rtggx_debug_light_list_cull: %d: 0 or 1", enable); return -1; }
  c->lightListCullOn = enable == 1;
  return 0;
}
// The lights at the surfaces the paths hit (include/rtggx.h).  Only the value is kept: it is stored whether or not lights are set, allocates
// nothing here (the first frame that has both does: lighting.hip beginSunHits) and takes effect with the next rtggx_render_visibility.  No
// synchronisation, no end of a still-sky run, no reset of an accumulation, as for the lights themselves.
int rtggx_set_light_reflections(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  if (enable != 0 && enable != 1) { setError("rtggx_set_light_reflections: %d: 0 or 1", enable); return -1; }
  c->lightReflectionsRequested = enable == 1;
  return 0;
}
// One shadow ray per surface point for all lights (include/rtggx.h).  Only the value is kept: it is stored whether or not lights are set,
// allocates nothing here (the first mode-1 frame with lights does: lighting.hip launchLights) and takes effect with the next
// rtggx_render_visibility.  No synchronisation, no end of a still-sky run, no reset of an accumulation, as for the lights themselves.
int rtggx_set_light_sampling(rtggx_context* c, int mode) {
  RT_CHECK_CTX(c);
  if (mode != 0 && mode != 1) { setError("rtggx_set_light_sampling: mode %d: 0 (a shadow ray per light) or 1 (one for all lights)", mode); return -1; }
  c->lightSamplingRequested = (uint32_t)mode;
  c->lightVisSeq0 = c->lightVisSeq;      // rtggx_set_light_pick_visibility: a reset
  return 0;
}
// The pick weighted by the pixel's remembered visibility (include/rtggx.h).  Only the value is kept: it allocates nothing here (the first
// acting frame does: lighting.hip launchLights) and takes effect with the next rtggx_render_visibility.  A change of the setting is a reset
// of the sequence.  No synchronisation, no end of a still-sky run, no reset of an accumulation, as for the mode.
int rtggx_set_light_pick_visibility(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  if (enable != 0 && enable != 1) { setError("rtggx_set_light_pick_visibility: %d: 0 or 1", enable); return -1; }
  if (enable == 1 && (c->rowBegin > 0u || c->rowEnd < c->H)) { setError("rtggx_set_light_pick_visibility: on a strip (rows [%u,%u) of %u): a reprojected tap may lie in another rank's rows -- whole frames only", c->rowBegin, c->rowEnd, c->H); return -1; }
  if ((enable == 1) != c->lightVisRequested) c->lightVisSeq0 = c->lightVisSeq;
  c->lightVisRequested = enable == 1;
  return 0;
}
// One of the two images of records, behind everything the context has enqueued
int rtggx_read_light_visibility(rtggx_context* c, uint32_t image, RtggxLightVisRecord* out, size_t bytes, uint32_t* sequence) {
  RT_CHECK_CTX(c);
  if (image > 1u) { setError("rtggx_read_light_visibility: image %u: 0 or 1", image); return -1; }
  if (!c->lightVisImg[image]) { setError("rtggx_read_light_visibility: no records yet: they exist from the first frame of mode 1 with a casting light and rtggx_set_light_pick_visibility(ctx, 1)"); return -1; }
  const size_t want = (size_t)c->W * c->H * sizeof(RtggxLightVisRecord);
  if (!out || bytes != want) { setError("rtggx_read_light_visibility: %zu bytes at %p: %u x %u records of 16 bytes are %zu", bytes, (void*)out, c->W, c->H, want); return -1; }
  RT_HIP(syncStreams(c));
  RT_HIP(hipMemcpy(out, c->lightVisImg[image], want, hipMemcpyDeviceToHost));
  if (sequence) *sequence = c->lightVisSeq;
  return 0;
}
// A list's pick weighted by the pixel's sparse record (include/rtggx.h): rtggx_set_light_pick_visibility's setter and reader for the list's
// own setting, sequence and images (the first acting frame allocates them: lighting.hip launchLights)
int rtggx_set_light_list_visibility(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  if (enable != 0 && enable != 1) { setError("rtggx_set_light_list_visibility: %d: 0 or 1", enable); return -1; }
  if (enable == 1 && (c->rowBegin > 0u || c->rowEnd < c->H)) { setError("rtggx_set_light_list_visibility: on a strip (rows [%u,%u) of %u): a reprojected tap may lie in another rank's rows -- whole frames only", c->rowBegin, c->rowEnd, c->H); return -1; }
  if ((enable == 1) != c->lightListVisRequested) c->lightListVisSeq0 = c->lightListVisSeq;
  c->lightListVisRequested = enable == 1;
  return 0;
}
int rtggx_read_light_list_visibility(rtggx_context* c, uint32_t image, RtggxLightListVisRecord* out, size_t bytes, uint32_t* sequence) {
  RT_CHECK_CTX(c);
  if (image > 1u) { setError("rtggx_read_light_list_visibility: image %u: 0 or 1", image); return -1; }
  if (!c->lightListVisImg[image]) { setError("rtggx_read_light_list_visibility: no records yet: they exist from the first frame of a list with a casting light and rtggx_set_light_list_visibility(ctx, 1)"); return -1; }
  const size_t want = (size_t)c->W * c->H * sizeof(RtggxLightListVisRecord);
  if (!out || bytes != want) { setError("rtggx_read_light_list_visibility: %zu bytes at %p: %u x %u records of 16 bytes are %zu", bytes, (void*)out, c->W, c->H, want); return -1; }
  RT_HIP(syncStreams(c));
  RT_HIP(hipMemcpy(out, c->lightListVisImg[image], want, hipMemcpyDeviceToHost));
  if (sequence) *sequence = c->lightListVisSeq;
  return 0;
}
// Sums and count back to zero: two clears on the main stream, behind the frames it holds and in front of the next one; nothing waits.
int rtggx_reset_accumulation(rtggx_context* c) {
  RT_CHECK_CTX(c);
  if (c->accRefl) {
    const size_t n = (size_t)c->W * c->H;
    RT_HIP(hipMemsetAsync(c->accRefl, 0, n * 16, c->streamMain));
    RT_HIP(hipMemsetAsync(c->accDiff, 0, n * 16, c->streamMain));
  }
  c->accumFrames = 0u;
  return 0;
}
int rtggx_accumulated_frames(rtggx_context* c, uint32_t* frames) {
  RT_CHECK_CTX(c);
  if (!frames) { setError("rtggx_accumulated_frames: null result"); return -1; }
  *frames = c->accumFrames;      // (counted as the frames are enqueued: no wait)
  return 0;
}
// The mean image, then the tone map of it (the frame's own kernel, reading RTGGX_BUF_CONVERGED instead of TemporalSSOut), both on the main
// stream.  Between a frame's rtggx_denoise and its rtggx_tone_map it takes the back buffer from a fused temporal pass: that tone map then
// runs as a kernel of its own again.
int rtggx_present_accumulation(rtggx_context* c) {
  RT_CHECK_CTX(c);
  if (!c->accRefl) { setError("rtggx_present_accumulation: accumulation was never enabled (rtggx_set_accumulation)"); return -1; }
  if (c->rowBegin > 0u || c->rowEnd < c->H) { setError("rtggx_present_accumulation: on a strip (rows [%u,%u) of %u): whole frames only", c->rowBegin, c->rowEnd, c->H); return -1; }
  if (c->accumFrames == 0u) { setError("rtggx_present_accumulation: no frame has been accumulated"); return -1; }
  FrameParams fp = c->slots[c->slot];      // (only the size and the rows enter the tone map)
  fp.W = c->W; fp.H = c->H; fp.rowBegin = 0u; fp.rowEnd = c->H;
  int r = launchPresentAccumulation(c, c->streamMain);
  if (!r) r = launchToneMap(c, fp, c->streamMain, nullptr, c->converged);
  c->toneMapDone = false;
  return r;
}

// Adaptive sampling (raytrace.hip launchShadeSamples; DESIGN.md "Adaptive sampling").  The map lives on the device in
// bin order, a byte per bin (rtggx_context::sampleMapBuf); the host keeps no copy.  Both entry points wait for every stream first: the
// copy they then write is the one no frame reads -- not the one in force, which a frame whose visibility pass has run will still be
// traced under --, and the next rtggx_render_visibility takes it over.  No end of the still-sky runs: a tile without a surface has no
// covered pixel, and a mapped sample pass stores into its bins the count the run vouches for, 0 without a mark.
namespace rt {
static uint32_t mapBlocksX(const rtggx_context* c) { return (c->W + 7u) / 8u; }
static uint32_t mapBlocksY(const rtggx_context* c) { return (c->H + 7u) / 8u; }
static size_t mapWords(const rtggx_context* c) { return (size_t)((c->W + 15u) / 16u) * ((c->H + 15u) / 16u); }      // one word per tile: its four bins' counts
static uint32_t mapBinOf(const rtggx_context* c, uint32_t bx, uint32_t by) { return ((by >> 1) * ((c->W + 15u) / 16u) + (bx >> 1)) * 4u + (by & 1u) * 2u + (bx & 1u); }
// both copies or none; returns the index of the copy a set may write
static int sampleMapTarget(rtggx_context* c, const char* who) {
  if (!c->sampleMapBuf[0]) {
    DevBuf<uint32_t> a, b;
    hipError_t e = alloc(a, mapWords(c));
    if (e == hipSuccess) e = alloc(b, mapWords(c));
    if (e != hipSuccess) { setError("%s: %s (2 x %zu bytes for the map)", who, hipGetErrorString(e), mapWords(c) * 4u); return -2; }
    c->sampleMapBuf[0] = std::move(a); c->sampleMapBuf[1] = std::move(b);
  }
  return c->sampleMap == 0 ? 1 : 0;
}
}  // namespace rt
int rtggx_set_sample_map(rtggx_context* c, const uint8_t* counts, uint32_t blocksX, uint32_t blocksY) {
  RT_CHECK_CTX(c);
  if (!counts && blocksX == 0u && blocksY == 0u) { RT_HIP(syncStreams(c)); c->sampleMapRequested = -1; return 0; }
  if (!counts) { setError("rtggx_set_sample_map: null counts"); return -1; }
  if (blocksX != mapBlocksX(c) || blocksY != mapBlocksY(c)) { setError("rtggx_set_sample_map: a map of %u x %u blocks for a frame of %u x %u pixels, which has %u x %u blocks of 8 x 8", blocksX, blocksY, c->W, c->H, mapBlocksX(c), mapBlocksY(c)); return -1; }
  if (c->rowBegin > 0u || c->rowEnd < c->H) { setError("rtggx_set_sample_map: on a strip (rows [%u,%u) of %u): a strip's tiles count from its first row, a block would no longer be a bin -- whole frames only", c->rowBegin, c->rowEnd, c->H); return -1; }
  std::vector<uint32_t> words(mapWords(c), 0x01010101u);
  uint8_t* const bins = reinterpret_cast<uint8_t*>(words.data());
  for (uint32_t by = 0; by < blocksY; ++by)
    for (uint32_t bx = 0; bx < blocksX; ++bx) {
      const uint8_t n = counts[(size_t)by * blocksX + bx];
      if (n != 1u && n != 2u && n != 4u && n != 8u) { setError("rtggx_set_sample_map: a count of %u at block (%u, %u): 1, 2, 4 or 8", (unsigned)n, bx, by); return -1; }
      bins[mapBinOf(c, bx, by)] = n;
    }
  RT_HIP(syncStreams(c));
  const int t = sampleMapTarget(c, "rtggx_set_sample_map");
  if (t < 0) return t;
  RT_HIP(hipMemcpy(c->sampleMapBuf[t], words.data(), words.size() * 4u, hipMemcpyHostToDevice));
  c->sampleMapRequested = t;
  return 0;
}
int rtggx_read_sample_map(rtggx_context* c, uint8_t* counts, uint32_t capacity, uint32_t* blocksX, uint32_t* blocksY) {
  RT_CHECK_CTX(c);
  if (!blocksX || !blocksY) { setError("rtggx_read_sample_map: null result"); return -1; }
  RT_HIP(syncStreams(c));
  if (c->sampleMapRequested < 0) { *blocksX = 0u; *blocksY = 0u; return 0; }
  const uint32_t bX = mapBlocksX(c), bY = mapBlocksY(c);
  *blocksX = bX; *blocksY = bY;
  if (!counts || capacity < bX * bY) { setError("rtggx_read_sample_map: room for %u counts, the map has %u x %u", counts ? capacity : 0u, bX, bY); return -1; }
  std::vector<uint32_t> words(mapWords(c));
  RT_HIP(hipMemcpy(words.data(), c->sampleMapBuf[c->sampleMapRequested], words.size() * 4u, hipMemcpyDeviceToHost));
  const uint8_t* const bins = reinterpret_cast<const uint8_t*>(words.data());
  for (uint32_t by = 0; by < bY; ++by)
    for (uint32_t bx = 0; bx < bX; ++bx) counts[(size_t)by * bX + bx] = bins[mapBinOf(c, bx, by)];
  return 0;
}
// Scoring against a reference (score.hip; DESIGN.md "Scoring against a reference").  The reference is read by the scoring kernels on the
// main stream alone.  rtggx_set_reference copies from the host: it waits for every stream first (frames in flight still read the image it
// replaces or frees) and copies before it returns; rtggx_reference_from_accumulation writes it by a kernel on the main stream, behind the
// scores already enqueued there and in front of the later ones -- no wait.
int rtggx_set_reference(rtggx_context* c, const void* rgba16f, size_t bytes) {
  RT_CHECK_CTX(c);
  const size_t want = (size_t)c->W * c->H * 8u;
  if (!rgba16f && bytes == 0u) {      // release: scoring ends with it
    RT_HIP(syncStreams(c));
    c->reference.reset();
    c->scoring = c->scoringRequested = false;
    return 0;
  }
  if (!rgba16f || bytes != want) { setError("rtggx_set_reference: %zu bytes for a %u x %u RGBA16F image of %zu", bytes, c->W, c->H, want); return -1; }
  RT_HIP(syncStreams(c));
  { const int r = allocReference(c, "rtggx_set_reference"); if (r) return r; }
  RT_HIP(hipMemcpy(c->reference, rgba16f, want, hipMemcpyHostToDevice));
  return 0;
}
int rtggx_reference_from_accumulation(rtggx_context* c) {
  RT_CHECK_CTX(c);
  if (!c->accRefl) { setError("rtggx_reference_from_accumulation: accumulation was never enabled (rtggx_set_accumulation)"); return -1; }
  if (c->rowBegin > 0u || c->rowEnd < c->H) { setError("rtggx_reference_from_accumulation: on a strip (rows [%u,%u) of %u): whole frames only", c->rowBegin, c->rowEnd, c->H); return -1; }
  if (c->accumFrames == 0u) { setError("rtggx_reference_from_accumulation: no frame has been accumulated"); return -1; }
  { const int r = allocReference(c, "rtggx_reference_from_accumulation"); if (r) return r; }
  return launchReferenceFromAccumulation(c, c->streamMain);
}
// Taken over by the next rtggx_render_visibility, like accumulation; off allocates nothing.  `index` goes on counting over off and on.
int rtggx_set_scoring(rtggx_context* c, int enable) {
  RT_CHECK_CTX(c);
  if (enable && !c->reference) { setError("rtggx_set_scoring: no reference image (rtggx_set_reference, rtggx_reference_from_accumulation)"); return -1; }
  if (enable) { const int r = allocScoring(c); if (r) return r; }
  c->scoringRequested = enable != 0;
  return 0;
}
// The unread records, oldest first.  Waits for the main stream alone: every record is written by the last kernel rtggx_denoise put there.
int rtggx_read_scores(rtggx_context* c, RtggxScore* out, uint32_t capacity, uint32_t* count) {
  RT_CHECK_CTX(c);
  if (!count || (!out && capacity > 0u)) { setError("rtggx_read_scores: null result"); return -1; }
  *count = 0u;
  if (!c->scoreRing || c->scoreIndex == c->scoreRead) return 0;
  RT_HIP(hipStreamSynchronize(c->streamMain));
  if (c->scoreIndex - c->scoreRead > (uint64_t)RTGGX_SCORE_RING) c->scoreRead = c->scoreIndex - (uint64_t)RTGGX_SCORE_RING;      // the older ones have been overwritten
  const uint64_t unread = c->scoreIndex - c->scoreRead;
  const uint32_t n = unread < capacity ? (uint32_t)unread : capacity;
  for (uint32_t done = 0; done < n;) {      // at most two runs of slots: the ring wraps once
    const uint32_t slot = (uint32_t)((c->scoreRead + done) % (uint64_t)RTGGX_SCORE_RING);
    const uint32_t run = n - done < (uint32_t)RTGGX_SCORE_RING - slot ? n - done : (uint32_t)RTGGX_SCORE_RING - slot;
    RT_HIP(hipMemcpy(out + done, c->scoreRing + slot, sizeof(RtggxScore) * run, hipMemcpyDeviceToHost));
    done += run;
  }
  c->scoreRead += n; *count = n;
  return 0;
}

int rtggx_set_env(rtggx_context* c, int format, uint32_t size, uint32_t mips, const void* data, size_t bytes) {
  RT_CHECK_CTX(c);
  if (!data) { setError("rtggx_set_env: null data"); return -1; }
  RT_HIP(syncStreams(c));
  c->sky.breakRuns(SkyBreak::Environment);
  return decodeEnv(c, format, size, mips, data, bytes, c->streamMain);
}

// Everything is checked before anything is touched: a refused image leaves the environment, the still-sky runs and the frame as they were.
int rtggx_set_env_image(rtggx_context* c, int layout, int pixels, uint32_t width, uint32_t height, const void* data, size_t bytes, uint32_t cubeSize) {
  RT_CHECK_CTX(c);
  if (!data) { setError("rtggx_set_env_image: null data"); return -1; }
  if (layout != RTGGX_ENV_EQUIRECT && layout != RTGGX_ENV_VCROSS && layout != RTGGX_ENV_HCROSS) { setError("rtggx_set_env_image: unknown layout %d", layout); return -1; }
  if (pixels != RTGGX_PIXELS_RGBE8 && pixels != RTGGX_PIXELS_RGB32F) { setError("rtggx_set_env_image: unknown pixel format %d", pixels); return -1; }
  if (width == 0u || height == 0u) { setError("rtggx_set_env_image: an image of %u x %u pixels", width, height); return -1; }
  uint32_t size;
  if (layout == RTGGX_ENV_EQUIRECT) {
    if (width > 16384u || height > 8192u) { setError("rtggx_set_env_image: a panorama of %u x %u pixels, more than 16384 x 8192", width, height); return -1; }
    if (cubeSize > 4096u) { setError("rtggx_set_env_image: cube size %u, more than 4096", cubeSize); return -1; }
    size = cubeSize;
    if (!size) for (size = 1u; 2u * size <= width / 4u; size *= 2u) {}      // the largest power of two <= width / 4 (1 below 8 columns)
  } else {
    const uint32_t across = layout == RTGGX_ENV_VCROSS ? 3u : 4u, down = layout == RTGGX_ENV_VCROSS ? 4u : 3u;
    if (width % across != 0u || height % down != 0u || width / across != height / down) {
      setError("rtggx_set_env_image: %u x %u pixels are no %s cross (%u x %u square cells)", width, height, layout == RTGGX_ENV_VCROSS ? "vertical" : "horizontal", across, down); return -1;
    }
    size = width / across;
    if (size > 4096u) { setError("rtggx_set_env_image: a cross of cell %u, more than 4096", size); return -1; }
    if (cubeSize != 0u) { setError("rtggx_set_env_image: cube size %u given with a cross: its cells are the faces, a cross is never resampled", cubeSize); return -1; }
  }
  const size_t need = (size_t)width * height * (pixels == RTGGX_PIXELS_RGBE8 ? 4u : 12u);
  if (bytes < need) { setError("rtggx_set_env_image: %zu bytes given, %zu needed", bytes, need); return -1; }
  RT_HIP(syncStreams(c));
  const int r = buildEnvFromImage(c, layout, pixels, width, height, data, size, c->streamMain);
  if (r == 0) c->sky.breakRuns(SkyBreak::Environment);      // (a failed build has left the old one)
  return r;
}

int rtggx_generate_env_mips(rtggx_context* c) {
  RT_CHECK_CTX(c);
  if (!c->env.texels) { setError("rtggx_generate_env_mips: no environment map"); return -1; }
  RT_HIP(syncStreams(c));
  const int r = generateEnvMips(c, c->streamMain);
  if (r == 0) c->sky.breakRuns(SkyBreak::Environment);
  return r;
}

// Checked before anything is touched, like rtggx_set_env_image: a refusal leaves the environment, the still-sky runs and the frame as they were.
int rtggx_prefilter_env(rtggx_context* c, uint32_t samples) {
  RT_CHECK_CTX(c);
  if (!c->env.texels) { setError("rtggx_prefilter_env: no environment map"); return -1; }
  uint32_t n = 0;
  if (!envFilterSamples(samples, n)) { setError("rtggx_prefilter_env: %u samples: a power of two from %u to %u, or 0 for %u", samples, RTGGX_ENV_FILTER_MIN_SAMPLES, RTGGX_ENV_FILTER_MAX_SAMPLES, kEnvFilterDefaultSamples); return -1; }
  RT_HIP(syncStreams(c));
  const int r = prefilterEnv(c, n, c->streamMain);
  if (r == 0) c->sky.breakRuns(SkyBreak::Environment);
  return r;
}

// Checked before anything is touched; and a call that takes nothing out -- remove == 0, or no sun found -- leaves the environment, the
// still-sky runs and the SH state as they were: it has only read level 0.
int rtggx_sun_from_env(rtggx_context* c, float coneDegrees, float ringDegrees, float minContrast, int remove, RtggxSunEstimate* out) {
  RT_CHECK_CTX(c);
  if (!out) { setError("rtggx_sun_from_env: null result"); return -1; }
  if (!c->env.texels) { setError("rtggx_sun_from_env: no environment map"); return -1; }
  if (c->env.size > kSunEnvMaxSide) { setError("rtggx_sun_from_env: a cube of side %u, more than %u", c->env.size, kSunEnvMaxSide); return -1; }
  SunEnvAngles angles;
  if (const char* why = sunEnvAngles(coneDegrees, ringDegrees, minContrast, angles)) { setError("rtggx_sun_from_env: %s (cone %g, ring %g, contrast %g)", why, coneDegrees, ringDegrees, minContrast); return -1; }
  RT_HIP(syncStreams(c));
  const int r = sunFromEnv(c, angles, remove, out, c->streamMain);
  if (r == 0 && out->removed) c->sky.breakRuns(SkyBreak::Environment);
  return r;
}

int rtggx_set_material(rtggx_context* c, uint32_t mesh, const float baseColor[4], float roughness, float metallic) {
  RT_CHECK_CTX(c);
  if (mesh >= RTGGX_NUM_MESH) { setError("rtggx_set_material: bad mesh"); return -1; }
  memcpy(c->material.BaseColors[mesh], baseColor, 16);
  c->material.RoughMetals[mesh][0] = roughness; c->material.RoughMetals[mesh][1] = metallic;
  return 0;
}
int rtggx_set_sampler(rtggx_context* c, int vndf) {
  RT_CHECK_CTX(c);
  c->vndf = vndf != 0;      // takes effect with the next rtggx_update_frame
  return 0;
}
int rtggx_set_metallic(rtggx_context* c, uint32_t mesh, float metallic) {   // RayTracer.cpp:244-248
  RT_CHECK_CTX(c);
  if (mesh >= RTGGX_NUM_MESH) { setError("rtggx_set_metallic: bad mesh"); return -1; }
  c->material.RoughMetals[mesh][1] = metallic;
  return 0;
}

}  // extern "C"
