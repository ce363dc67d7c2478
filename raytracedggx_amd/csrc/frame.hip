// C ABI of librtggx (include/rtggx.h), part 3 of 4: the per-frame entry points and the placement of their kernels on the context's streams.
// Frame order issued by the host (RayTracedGGX::OnRender, RayTracedGGX.cpp:302-353):
//   update_as (stream B)  ||  render_visibility (stream A)  -> event ->  ray_trace -> denoise -> tone_map
#include <cstring>
#include <chrono>
#include "capi_internal.h"
#include "rt_queue.h"
namespace rt {
// world -> object matrices of the two instances: general 4x4 inverse by cofactors in double,
// rounded once (the software TLAS; DESIGN.md "TLAS").
static void invert4x4(const float* a /*row-major*/, float* out) {
  double m[16], inv[16];
  for (int i = 0; i < 16; ++i) m[i] = (double)a[i];
  inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
  inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
  inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
  inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
  inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
  inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
  inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
  inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
  inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
  inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
  inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
  inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
  inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
  inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
  inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
  inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
  const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
  const double rdet = 1.0 / det;
  for (int i = 0; i < 16; ++i) out[i] = (float)(inv[i] * rdet);
}

// The frames-in-flight fence (InputSet::evRead: the last reader of an input set has ended) rides on a kernel's completion signal, and a
// kernel that carries an event leaves its queue idle for ~5 us behind it (profiles/r03_c_strip_chain.txt).  So it rides on the LAST
// kernel the main stream gets for the frame: the fused temporal + tone-map kernel, or the tone map where that is a kernel of its own.
// A frame that ends earlier -- the caller traces without denoising -- gets the event recorded explicitly by the next frame (settleSetRead).
static void settleSetRead(rtggx_context* c) {
  if (c->setReadDeferred < 0) return;
  InputSet& set = c->sets[c->setReadDeferred];
  hipEventRecord(set.evRead, c->streamMain);
  set.readRecorded = true; c->setReadDeferred = -1;
}
hipError_t syncStreams(rtggx_context* c) {
  hipError_t e = c->ownVis ? hipStreamSynchronize(c->ownVis) : hipSuccess;
  if (e == hipSuccess && c->streamRefit) e = hipStreamSynchronize(c->streamRefit);
  if (e == hipSuccess) e = hipStreamSynchronize(c->ownAS);
  if (e == hipSuccess) e = hipStreamSynchronize(c->streamMain);
  return e;
}
// Constants reach the device in rtggx_update_as; a caller that skips it still gets them, on the main stream.
// The constants go up on stream B (which also runs the visibility pass); everything on the main stream that
// consumes them is ordered behind the event.
static int uploadParamsStreamB(rtggx_context* c) {
  // (a visibility pass that has carried this slot to the device already -- rtggx_update_as came after it -- writes the same words from
  // its first workgroup, on another stream: this upload, the newer TLAS, must land second)
  if (c->evVisStream && c->evVisStream != c->streamAS) RT_HIP(hipStreamWaitEvent(c->streamAS, c->evVis, 0));
  const int r = uploadParams(c, c->slot, c->streamAS);
  if (r) return r;
  c->slotUploaded = true;
  RT_HIP(hipEventRecord(c->evAS, c->streamAS));
  RT_HIP(hipStreamWaitEvent(c->streamMain, c->evAS, 0));
  return 0;
}
int ensureParams(rtggx_context* c) { return c->slotUploaded ? 0 : uploadParamsStreamB(c); }
}  // namespace rt
using namespace rt;

extern "C" {
// A material with metallic below 1 traces a diffuse ray per covered pixel as well: two ray slots per pixel.  The bins grow once, before
// the first such frame (the frames in flight are waited for: the old bins are theirs).
static int growBins(rtggx_context* c) {
  RT_HIP(syncStreams(c));
  for (auto& set : c->sets) { set.rayQueue.reset(); set.hitQueue.reset(); }
  c->binSlots = RT_BIN;
  for (uint32_t i = 0; i < RT_SETS; ++i) { const int r = allocSet(c, i); if (r) return r; }      // (the bins, at the new size)
  c->testRayRange.reset();
  c->sunHitQueue.release(); c->lightHitQueue.release();      // (rtggx_set_sun_reflections, rtggx_set_light_reflections: their bins follow the frame's, at the next lit frame)
  return 0;
}
int rtggx_update_frame(rtggx_context* c, const RtggxFrameConstants* k) {
  RT_CHECK_CTX(c);
  if (!k) { setError("rtggx_update_frame: null constants"); return -1; }
  if (c->binSlots < RT_BIN && (c->material.RoughMetals[0][1] < 1.0f || c->material.RoughMetals[1][1] < 1.0f)) { const int r = growBins(c); if (r) return r; }
  c->slot = (c->slot + 1) % RT_SLOTS;   // RayTracer::FrameCount + 1 (rtggx_context.h)
  FrameParams& fp = c->slots[c->slot];
  fp.g = k->global; fp.rg = k->rayGen; fp.po[0] = k->perObject[0]; fp.po[1] = k->perObject[1];
  fp.mat = c->material;
  fp.W = c->W; fp.H = c->H; fp.rowBegin = c->rowBegin; fp.rowEnd = c->rowEnd;
  fp.flags = c->vndf ? RT_FLAG_VNDF : 0u; fp.sampleMask = c->sampleSet - 1u; fp.pad[0] = fp.pad[1] = 0u;      // (the mask: once more in rtggx_render_visibility, where a new set size takes over)
  memcpy(fp.invWorld, c->invWorld, sizeof fp.invWorld);
  c->haveConstants = true; c->slotUploaded = false; c->slotRendered = false;
  return 0;
}

// RayTracer::UpdateAccelerationStructure: refresh the two TLAS instance transforms from CBGlobal::Worlds
// (= m_worlds, RayTracer.cpp:288-290, 329-336).  Runs on the AS stream, overlapping the visibility pass.
int rtggx_update_as(rtggx_context* c) {
  RT_CHECK_CTX(c);
  if (!c->haveConstants) { setError("rtggx_update_as: rtggx_update_frame has not been called"); return -1; }
  FrameParams& fp = c->slots[c->slot];
  for (int i = 0; i < 2; ++i) {
    const M4 w = cbLoad4x3(fp.g.Worlds[i]);
    invert4x4(&w.m[0][0], c->invWorld[i]);
  }
  memcpy(fp.invWorld, c->invWorld, sizeof fp.invWorld);
  // Legal call order "render_visibility before update_as" (the sample's two queues overlap them, RayTracedGGX.cpp:304-339):
  // the visibility pass has then carried this slot to the device with the PREVIOUS frame's TLAS.  Mark it stale, so that
  // rtggx_ray_trace (ensureParams) sends it again, behind the visibility pass, before anything reads invWorld.
  c->slotUploaded = false;
  // The constants (with the refreshed TLAS) ride to the device with the first kernel of the visibility pass, which
  // follows on stream B (rtggx_render_visibility); a caller that traces without a visibility pass gets them through
  // ensureParams.  In timing mode they are uploaded here, so that the pass has a duration of its own.
  if (c->timing) {
    hipEventRecord(c->tev[0], c->streamAS);
    const int r = uploadParamsStreamB(c);
    if (r) return r;
    hipEventRecord(c->tev[1], c->streamAS);
  }
  return 0;
}

int rtggx_transform_sh(rtggx_context* c) {
  RT_CHECK_CTX(c);
  return projectSH(c, c->streamAS);      // consumed by the shading kernel, which runs on stream B
}

// The frame on the device (RayTracedGGX::OnRender, RayTracedGGX.cpp:302-353, re-cut for this machine).  Three stages on three
// streams, each stage one frame behind the one before it:
//     stream C   visibility pass (its first kernel carries the frame constants) -> ray generation        of frame f + 1
//     stream B   traversal                                                                                of frame f
//     main       hit / miss shading -> spatial filters -> temporal pass + tone map                        of frame f - 1
// plus stream R for the vertex upload and tree refit of a deforming mesh.  No stage fills the machine by itself (the traversal
// is a latency-bound chain of dependent gathers: profiles/r02_*_limiter.txt), so the three overlap; what each stage hands to the next
// exists four times (the input sets), and the events are
//     evVis                  visibility f        -> ray generation f           (R -> C; stream order where both are on C)
//     frameEvents(f).gen     ray generation f    -> traversal f                (C -> B)
//                            ray generation f    -> visibility f + 2           (C -> R: the target and the list it cleared)
//     frameEvents(f).trace   traversal f         -> shading f                  (B -> main)
//                            traversal f - 2     -> ray generation f           (B -> C: the bins' cost record and the ray counters
//                                                                               exist twice, by frame parity)
//     evRefit                refit f             -> visibility f, traversal f  (R -> C, B)
//     sets[set].evRead       last reader of a set -> the HOST, four frames later (the sample's frames-in-flight fence)
// rtggx_set_async_compute(0) (the sample's [A] toggle) puts everything on the main stream.
//
// WHERE a frame's kernels go is decided in ONE place, placeFrame, from a key of five facts (round 4: rounds 2-3 had grown nine
// interacting switches for it).  The table, each line measured in the round that introduced it (DESIGN.md sections 5, 7, 9):
//     key                              visibility pass   ray generation   traversal            hit shading       frames in flight
//     full-size launch                 C                 C                B                    main              4
//       + a mesh deforms / diffuse rays                                                                          3   (the front stages otherwise run ahead into one of two states)
//     small launch (< 200 000 rays)    C                 C                B, odd frames on R   the traversal's   4   (two traversals in flight; the main stream's chain is a strip's longest)
//       + a mesh deforms               C                 C                B                    main              4   (R is the refit's)
//     strip / caller-owned stream      no line of their own: rows and the main stream's identity do not move a kernel
//     async compute off                main              main             main                 main              4
struct Placement {
  bool small, strip, deforming, diffuse, callerStream;      // the key
  hipStream_t raster, gen, trace, shade;
  uint32_t framesInFlight;
  bool alternate, shadeWithTrace;
};
static Placement placeFrame(const rtggx_context* c, const FrameParams& fp, uint32_t frame) {
  Placement P;
  P.small = c->lastTraceSmall;      // by the ray count of the most recent frame whose count has arrived (raytrace.hip launchRayTrace; rtggx_debug_placement)
  P.strip = fp.rowBegin > 0u || fp.rowEnd < fp.H;
  P.deforming = c->mesh[0].deforming || c->mesh[1].deforming;
  P.diffuse = fp.mat.RoughMetals[0][1] < 1.0f || fp.mat.RoughMetals[1][1] < 1.0f;
  P.callerStream = c->externalStream;
  const bool async = c->asyncCompute && c->streamVis != nullptr;
  P.gen = async ? c->streamVis : c->streamMain;
  // (the visibility pass on the geometry stream R, beside the previous frame's ray generation instead of behind it -- built and measured in
  // round 4: 1080p 0.186 -> 0.202-0.216 ms, the traversal stretched from 0.146 to 0.226 ms by the busier mid-priority stream; profiles/r04_c_pipeline_ab.txt.
  // What it needed stays: ray generation clears the target of frame f + 2, and the pass waits for that ray generation by event.)
  P.raster = P.gen;
  P.alternate = async && c->streamRefit != nullptr && P.small && !P.deforming && (frame & 1u) != 0u;
  P.trace = !async ? c->streamMain : P.alternate ? c->streamRefit : c->streamAS;
  P.shadeWithTrace = async && !c->timing && P.small && !P.deforming;
  P.shade = P.shadeWithTrace ? P.trace : c->streamMain;
  P.framesInFlight = async && !P.small && (P.deforming || P.diffuse) ? RT_SETS - 1u : RT_SETS;
  return P;
}

static int waitForSet(rtggx_context* c, const InputSet& set) {
  if (set.readRecorded && hipEventQuery(set.evRead) != hipSuccess) {
    const auto t0 = std::chrono::steady_clock::now();
    RT_HIP(hipEventSynchronize(set.evRead));
    c->fenceWaitUs += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); ++c->fenceWaits;      // rtggx_debug_fence_wait
  }
  return 0;
}

int rtggx_render_visibility(rtggx_context* c) {
  RT_CHECK_CTX(c);
  if (!c->haveConstants) { setError("rtggx_render_visibility: no frame constants"); return -1; }
  if (!c->shDone && c->env.texels) { const int r = projectSH(c, c->streamAS); if (r) return r; }   // first frame only, RayTracer.cpp:345-350
  settleSetRead(c);      // (the previous frame ended without the kernel that would have carried its set's event)
  ++c->frameCounter;
  c->maxDepth = c->depthRequested; c->samples = c->samplesRequested; c->accumulate = c->accumulateRequested; c->sun = c->sunRequested; c->sunAngle = c->sunAngleRequested; c->sunReflections = c->sunReflectionsRequested; c->lights = c->lightsRequested; c->lightReflections = c->lightReflectionsRequested; c->lightSampling = c->lightSamplingRequested; c->lightVis = c->lightVisRequested; c->lightListVis = c->lightListVisRequested;
  bool takeLightList = false;      // rtggx_update_light_list[_device]: what the calls left is taken further down, on the frame's first stream
  if (c->lightList.version != c->lightListRequested.version && !(c->lightListPend >= 0 && c->lightListStored == c->lightListRequested.version)) {      // rtggx_set_light_list: the new list, and its copy on the device
    dropLightListUpdates(c);      // (updates of the list this one replaces)
    RT_HIP(syncStreams(c)); ++c->visibilityDrains;      // (a frame in flight may read the list the upload replaces)
    c->lightList = c->lightListRequested;
    const int r = uploadLightList(c); if (r) return r;
  } else {
    if (c->lightList.version != c->lightListRequested.version) c->lightListFrame = false;      // (a new list that a device update has uploaded already)
    takeLightList = true;
  }
  c->scoring = c->scoringRequested && c->reference != nullptr;
  c->sampleMap = c->sampleMapRequested;      // rtggx_set_sample_map: the setter has waited for every stream and written the copy no frame reads
  bool resendConstants = false;
  if (c->sampleSet != c->sampleSetRequested) {      // rtggx_set_sample_set: the kernels' variant, the table and the constants' mask change together
    // several frames from one rtggx_update_frame share the slot's device copy: the frame before may still read the mask that goes with ITS
    // table (a larger mask on a smaller table would read beyond it) -- wait for it.  One update per frame, the normal order, never waits.
    if (c->slotRendered) { RT_HIP(syncStreams(c)); ++c->visibilityDrains; }
    c->sampleSet = c->sampleSetRequested;
    c->slots[c->slot].sampleMask = c->sampleSet - 1u;
    resendConstants = c->slotUploaded;      // constants already on their way (timing mode) go again behind this pass, as after a late rtggx_update_as
  }
  c->denoiseIssued = false; c->toneMapDone = false;
  c->selectSet(c->setAhead(1u));
  // the set was last read four frames ago: normally long done; a host that has run further ahead than that waits here (also what makes
  // it safe for this frame's ray generation to clear the NEXT frame's visibility target: rtggx_context.h RT_VIS_RING)
  { const int r = waitForSet(c, c->cur()); if (r) return r; }
  const Placement P = placeFrame(c, c->slots[c->slot], c->frameCounter);
  // THREE frames in flight where the table says so: the host also waits for the end of frame f - 3 (profiles/r03_i_deform_states.txt:
  // with four, the deforming bunny at 1080p ran at 0.212-0.219 or 0.26-0.30 ms per frame, a run fell into one state; with three 0.220-0.238)
  if (P.framesInFlight < RT_SETS) { const int r = waitForSet(c, c->sets[c->setAhead(RT_SETS - P.framesInFlight)]); if (r) return r; }
  c->refitIssued = false;
  { const int r = issuePendingRefits(c, &c->refitIssued); if (r) return r; }
  const hipStream_t s = P.raster;
  if (takeLightList) { const int r = takeLightListUpdates(c, s); if (r) return r; }      // (nothing where no update call came: no launch, no copy)
  if (c->evVisStream && c->evVisStream != s) RT_HIP(hipStreamWaitEvent(s, c->evVis, 0));      // the previous pass ran on another stream
  // this frame's target and list of large triangles were cleared by the ray generation two frames back: on another stream, mostly
  { const FrameEvents& g = c->frameEvents(c->frameCounter + 2u);
    if (c->frameCounter >= 2u && g.genFrame == c->frameCounter - 2u && g.genStream != s) RT_HIP(hipStreamWaitEvent(s, g.gen, 0)); }
  // constants already on their way on stream B (timing mode uploads them in rtggx_update_as): the pass reads dParams[slot] and has to be
  // ordered behind that upload (evAS); on stream B it follows it anyway
  if (c->slotUploaded && s != c->streamAS) RT_HIP(hipStreamWaitEvent(s, c->evAS, 0));
  if (c->refitIssued && c->asyncCompute && s != c->streamRefit) RT_HIP(hipStreamWaitEvent(s, c->evRefit, 0));       // the rasteriser reads this set's vertices (on R it follows the refit anyway)
  if (c->timing) hipEventRecord(c->tev[2], s);
  int r = launchVisibility(c, c->slots[c->slot], s, c->streamVis ? c->evVis : nullptr);
  c->slotRendered = true;
  if (resendConstants) c->slotUploaded = false;      // (rtggx_ray_trace's ensureParams; nothing in front of it reads the mask)
  if (c->streamVis) c->evVisStream = s;
  if (c->timing) hipEventRecord(c->tev[13], s);
  if (!r) r = issueRebuildSteps(c);
  return r;
}

int rtggx_ray_trace(rtggx_context* c) {
  RT_CHECK_CTX(c);
  if (!c->haveConstants || !c->asBuilt) { setError("rtggx_ray_trace: %s", c->asBuilt ? "no frame constants" : "rtggx_build_as has not been called"); return -1; }
  if (!c->env.texels) { setError("rtggx_ray_trace: no environment map"); return -1; }
  { const int r = ensureParams(c); if (r) return r; }
  const uint32_t f = c->frameCounter;
  const FrameParams& fp = c->slots[c->slot];
  const Placement P = placeFrame(c, fp, f);
  c->lastPlacement[0] = P.small | (P.strip << 1) | (P.deforming << 2) | (P.diffuse << 3) | (P.callerStream << 4);
  const auto streamId = [&](hipStream_t st) { return st == c->streamMain ? 0u : st == c->streamAS ? 1u : st == c->streamVis ? 2u : st == c->streamRefit ? 3u : 4u; };
  c->lastPlacement[1] = streamId(P.gen) | (streamId(P.trace) << 4) | (streamId(P.shade) << 8) | (P.framesInFlight << 12) | (streamId(P.raster) << 16);
  const hipStream_t sGen = P.gen;
  if (c->evVisStream && c->evVisStream != sGen) RT_HIP(hipStreamWaitEvent(sGen, c->evVis, 0));      // this frame's visibility pass (on the geometry stream)
  // Small launches last as long as their longest chain of dependent traversal steps and leave most of the chip idle meanwhile: the
  // traversals of odd frames go to a second stream (R, idle unless a mesh deforms), so that two are in flight.  Everything a traversal
  // shares with its neighbours in time is per input set, per frame parity or per frame & 3, and everybody who needs its results waits
  // for its event, not for its stream; the stack spill area exists twice (launchTrace).  (A third traversal stream loses everywhere:
  // beyond four streams with work on them the queues take turns; profiles/r03_c_strip_chain.txt.)
  const hipStream_t sTrace = P.trace;
  c->traceSpillHalf = P.alternate ? 1u : 0u;
  if (sGen != sTrace) {
    // ray generation reads the cost record of the traversal two frames back and resets that frame's ray counters (frame parity)
    if (c->frameEvents(f + 2u).traceRecorded) RT_HIP(hipStreamWaitEvent(sGen, c->frameEvents(f + 2u).trace, 0));
    // a caller that skipped the visibility pass (or uploaded constants on stream B): order ray generation behind the upload
    if (c->slotUploaded) RT_HIP(hipStreamWaitEvent(sGen, c->evAS, 0));
  }
  if (c->refitIssued && c->asyncCompute) RT_HIP(hipStreamWaitEvent(sTrace, c->evRefit, 0));      // this set's tree
  // rtggx_update_light_list[_device]: the frame's version of the list was written on another stream (the visibility pass's, the
  // caller's) -- the two streams whose kernels read it wait for that write, until it is seen to have ended
  if (c->lightListAwaitWritten && c->lightListCur >= 0 && c->lightList.count) {
    rtggx_context::LightListVersion& v = c->lightListRing[c->lightListCur];
    if (hipEventQuery(v.evWritten) == hipSuccess) c->lightListAwaitWritten = false;
    else { RT_HIP(hipStreamWaitEvent(c->streamMain, v.evWritten, 0)); if (sTrace != c->streamMain) RT_HIP(hipStreamWaitEvent(sTrace, v.evWritten, 0)); }
  }
  if (c->timing) hipEventRecord(c->tev[3], sGen);
  FrameEvents& ev = c->frameEvents(f);
  const bool shadeWithTrace = P.shadeWithTrace && sGen != sTrace && sTrace != c->streamMain;
  // who carries RayTracingOut1 over from the previous set where this frame traces no diffuse ray (raytrace.hip launchShade): ray
  // generation, unless the previous frame's shading kernel wrote into that set's image -- then, once, ray generation waits for it
  // (one bubble in the pipeline), so that the previous set's image is final when it reads it
  if (c->shadeWroteDiff && !P.diffuse && !c->lastFrameDiffuse && c->diffStream) {
    if (c->diffStream != sGen) { RT_HIP(hipEventRecord(c->evRT, c->diffStream)); RT_HIP(hipStreamWaitEvent(sGen, c->evRT, 0)); }
    c->shadeWroteDiff = false;
  }
  c->lastFrameDiffuse = P.diffuse;
  c->genCarriesDiff = !c->shadeWroteDiff;
  int r = launchRayTrace(c, fp, sGen, sTrace, shadeWithTrace ? nullptr : ev.trace);
  ev.traceRecorded = true;
  c->lastRayCounter32 = c->rayCounter32;
  c->shadeWroteDiff = !c->genCarriesDiff || P.diffuse;
  if (shadeWithTrace) {
    // Small launches: the hit shading follows the traversal on ITS stream (the main stream's chain -- shading, two filters, temporal pass +
    // tone map -- is the longest stage of a thin strip's frame, and the two traversal streams alternate, so theirs may be twice as long:
    // 1920 x 171 0.060 -> 0.052 ms per frame, profiles/r03_c_strip_chain.txt); the event the main stream -- and ray generation two frames
    // on -- waits for then rides on the shading kernel.  The shading of frame f copies what it does not trace from the image of frame
    // f - 1, which the other traversal stream's shading kernel wrote, or the main stream's if this is the first frame shaded here.
    if (!c->genCarriesDiff && c->shadeStream && c->shadeStream != sTrace) {
      if (c->shadeStream == c->streamMain) { RT_HIP(hipEventRecord(c->evRT, c->streamMain)); RT_HIP(hipStreamWaitEvent(sTrace, c->evRT, 0)); }
      else if (c->frameEvents(f + 3u).traceRecorded) RT_HIP(hipStreamWaitEvent(sTrace, c->frameEvents(f + 3u).trace, 0));
    }
    if (!r) r = launchShade(c, fp, sTrace, ev.trace);
    c->shadeStream = sTrace;
    RT_HIP(hipStreamWaitEvent(c->streamMain, ev.trace, 0));
  } else {
    // stream B runs ahead with the traversal; shading and the denoiser consume the bins, the G-buffer and the traced images on the main
    // stream (the event completes with the trace kernel; a shading kernel of the frame before on a traversal stream has been waited for
    // by the main stream in its own frame)
    RT_HIP(hipStreamWaitEvent(c->streamMain, ev.trace, 0));
    if (!r) r = launchShade(c, fp, c->streamMain);
    c->shadeStream = c->streamMain;
  }
  // rate 4: the untraced pixels, on the main stream behind the hit shading (raytrace.hip reconstructKernel)
  c->diffStream = c->shadeStream;
  if (c->rayRate == 4u) {
    if (!r) r = launchReconstruct(c, fp, c->streamMain);
    c->diffStream = c->streamMain;
  }
  // the sun (rtggx_set_sun): three kernels on the main stream, where both traced images are complete (see the accumulation below) -- behind the
  // hit shading and the resolve of N samples, in front of the accumulation, the scoring and the denoiser.  The next frame's carry-over of
  // RayTracingOut1 and its shading kernels wait for whoever wrote the images last: from here on that is the main stream.  With a deforming
  // mesh the shadow launch reads this set's tree: the main stream follows the traversal's event, which followed the refit's.
  if (c->sun.on) {
    if (!r) r = launchSun(c, fp, c->streamMain);
    c->shadeStream = c->diffStream = c->streamMain;
  }
  // local lights (rtggx_set_lights): per light three kernels and one resolve behind the last, on the main stream behind the sun's pass, for
  // the sun's reasons -- both traced images are complete here, and from here on the main stream is who wrote them last
  if (c->lights.count || c->lightList.count) {      // (rtggx_set_light_list: the same pass over the list)
    if (!r) r = launchLights(c, fp, c->streamMain);
    c->shadeStream = c->diffStream = c->streamMain;
  }
  // rtggx_update_light_list[_device]: the frame's version of the list has been read for the last time where the main stream stands --
  // launchLights ran on it, and it has passed ev.trace, which rides behind the hit passes (launchShade's `done`)
  if (c->lightListCur >= 0 && c->lightList.count) {
    rtggx_context::LightListVersion& v = c->lightListRing[c->lightListCur];
    RT_HIP(hipEventRecord(v.evRead, c->streamMain)); v.readRecorded = true;
  }
  // accumulation (rtggx_set_accumulation): the frame's two traced images into the running sums, on the main stream.  Both images are
  // complete where the main stream stands: it has passed ev.trace, which rides on the traversal with the shading (and the resolve of N
  // samples) following on the main stream itself, or -- small launches -- on the LAST kernel of the shading on the traversal's stream
  // (launchShade's `done`: the final pass, or the resolve); ray generation, which writes the background words, precedes the traversal.
  // The sums exist once: consecutive frames' kernels follow each other on the main stream, whichever stream shaded them.  The kernel
  // reads the current set in front of the denoiser, so the set's evRead -- recorded behind it on this stream -- covers it.
  if (c->accumulate) {
    if (!r) r = launchAccumulate(c, fp, c->streamMain);
    if (!r) ++c->accumFrames;
  }
  // the main stream has now been given work that reads the current input set: that set may not be overwritten (four frames from now)
  // before its evRead, which rides on the LAST kernel the main stream gets for this frame (settleSetRead)
  c->setReadDeferred = (int)c->setIndex;
  if (c->timing) hipEventRecord(c->tev[14], c->streamMain);
  return r;
}

int rtggx_denoise(rtggx_context* c, int useSharedMem) {
  RT_CHECK_CTX(c);
  if (!c->haveConstants) { setError("rtggx_denoise: no frame constants"); return -1; }
  if (c->timing) hipEventRecord(c->tev[9], c->streamMain);   // start of denoise
  // Denoiser::Denoise and Denoiser::ToneMap follow each other in every frame of the sample (RayTracedGGX.cpp:341-350), and the temporal pass can
  // tone-map its result as well (denoise.hip temporalToneKernel; rtggx_tone_map then finds its work done): one launch, one event-carrying
  // gap and 8 bytes per pixel less.  WHERE that pays was measured (profiles/r04_c_pipeline_ab.txt): on small launches -- thin strips, small
  // frames, bound by the host's launches and the main stream's chain of short kernels -- and NOT on full-size frames, where the fused
  // kernel's workgroups of 1024 threads and 45 KB of LDS find room on a CU shared with the traversal's resident workgroup and ray
  // generation later than four small ones do (1080p 0.186 -> 0.204 ms; 512 threads: 0.199).  So it follows the placement's `small`; not in
  // the per-pass timing mode (the tone map keeps a duration of its own); rtggx_debug_fuse_tone_map pins it either way.
  // While scoring is on (rtggx_set_scoring) the tone map is never fused either: the scoring kernels go behind the temporal pass and in FRONT
  // of the kernel that carries the set's evRead -- they read the set's traced images and the frame's visibility target.
  const bool fuse = !c->timing && !c->scoring && (c->fuseToneMap > 0 || (c->fuseToneMap < 0 && c->lastTraceSmall));
  // the fused kernel is the frame's last on this stream and carries the set's event; else the tone map will
  const int r = launchDenoise(c, c->slots[c->slot], useSharedMem, c->streamMain, fuse ? c->cur().evRead : nullptr, fuse);
  if (fuse) { c->cur().readRecorded = true; c->setReadDeferred = -1; } else c->setReadDeferred = (int)c->setIndex;
  // the frame's score (score.hip): TemporalSSOut[parity] is complete where the main stream stands, the set's evRead still to come -- on the
  // tone map, or recorded by settleSetRead -- behind these two kernels
  if (!r && c->scoring && c->reference) { const int rs = launchScore(c, c->slots[c->slot], c->streamMain); if (rs) return rs; }
  c->denoiseIssued = true; c->toneMapDone = fuse && c->slots[c->slot].rowEnd > c->slots[c->slot].rowBegin;
  return r;
}

int rtggx_tone_map(rtggx_context* c) {
  RT_CHECK_CTX(c);
  if (!c->haveConstants) { setError("rtggx_tone_map: no frame constants"); return -1; }
  int r = 0;
  if (c->toneMapDone) c->toneMapDone = false;      // this frame's rtggx_denoise wrote the back buffer as well
  else {
    const bool carry = c->setReadDeferred >= 0;
    r = launchToneMap(c, c->slots[c->slot], c->streamMain, carry ? c->sets[c->setReadDeferred].evRead : nullptr);
    if (carry && c->slots[c->slot].rowEnd > c->slots[c->slot].rowBegin) { c->sets[c->setReadDeferred].readRecorded = true; c->setReadDeferred = -1; }
  }
  settleSetRead(c);
  if (c->timing) { hipEventRecord(c->tev[10], c->streamMain); c->timingsPending = true; }
  return r;
}

int rtggx_sync(rtggx_context* c) {
  RT_CHECK_CTX(c);
  RT_HIP(syncStreams(c));
  return 0;
}

}  // extern "C"
