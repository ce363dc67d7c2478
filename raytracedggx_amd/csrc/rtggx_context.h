// Context of librtggx: device memory, streams and per-frame state behind the C ABI of rtggx.h.
//
// HBM layout (all buffers are linear, row-major, one element per pixel, W*H elements):
//   visDepth   u64   (D24 << 32) | visibility word -- the visibility pass resolves depth order
//                    with one 64-bit atomicMin per fragment; consumers read the halves
//   normal     u32   R10G10B10A2_UNORM      roughMetal u16 R8G8_UNORM     velocity u32 R16G16_FLOAT
//   rtRefl/rtDiff u32 R11G11B10_FLOAT       tss[2], fltRfl, fltDff u64 R16G16B16A16_FLOAT
//   backbuffer u32   R8G8B8A8_UNORM
// normal, roughMetal, velocity, rtRefl, rtDiff and the ray bins exist RT_SETS times (rt::InputSet, "input sets"): streams C and B
// (visibility, ray generation, traversal) fill one set while the main stream (shading, denoise, tone map) still reads an earlier
// one.  visDepth exists RT_VIS_RING times (rt::VisTarget).
// Scene: per mesh 24-byte vertices, u32 indices, 64-byte binary BVH nodes, their 128-byte 4-wide collapse,
// 64-byte leaf triangles; environment as RGBA16F mip-major (6 faces per mip); 9 float3 SH coefficients.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdlib.h>
#include <string>
#include <utility>
#include <vector>
#include <memory>
#include "rtggx_device.h"
#include "rt_owned_hip.h"
#include "rt_sky_chain.h"

// Input sets (G-buffer, traced images, ray bins): RT_SETS of them, used round-robin.  Stream B fills set i while the main stream
// still consumes the set of the frame before; before stream B is given the work that overwrites a set, the HOST waits
// for the event of that set's last reader, three frames back -- the frames-in-flight fence of the sample
// (RayTracedGGX.cpp: FrameCount = 3), and cheaper than a cross-queue wait on the GPU (10 us per frame on stream B's
// chain).  The frame constants live in a ring of RT_SLOTS device slots: one more than sets, because the tone map of
// frame f still reads its slot after the event of set f has completed.
// Round 2: FOUR sets (the sample's FrameCount is 3).  A frame's latency through the three stages (+ the refit of a deforming mesh) is
// 0.45-0.6 ms; with three sets in flight a thin strip or a deforming mesh ran out of frames to overlap: 1920x171 strip 0.0726 -> 0.0579 ms,
// deforming bunny 0.2432 -> 0.2347, 4K 0.758 -> 0.743, the 1080p frame unchanged; five and six give nothing more (profiles/r02_c_ab_pipeline.txt).
#ifndef RT_SETS
#define RT_SETS 4
#endif
#define RT_SLOTS (RT_SETS + 1)
// The visibility target (visDepth) exists twice more than the other members of an input set: ray generation of frame f clears the
// target of frame f + 2 on its way (raytrace.hip) -- one kernel launch and one pass over 8 bytes per pixel less per frame --, and the
// target it clears must be one nobody reads any more: frame f + 2 - RT_VIS_RING's, whose last reader the host has waited for (InputSet::evRead).
#define RT_VIS_RING (RT_SETS + 2)
#define RT_VIS_CLEAR 0x00FFFFFF00000000ull      // (D24 = 1.0) << 32 | nothing drawn
// Still sky (InputSet::skyRun): ray generation of frame f leaves a tile alone when the tile's word was 0, under one epoch, in frame f and
// in the RT_SKY_PREV_RUN frames before it.  Derived, not tuned -- everything the kernel would store there must be in place already:
//   * this set's G-buffer and traced texels were written in frame f - RT_SETS: that frame found the tile without a surface under this
//     epoch (same camera, same environment) -- frames f - 1 .. f - RT_SETS in the run;
//   * RoughMetal is carried from set to set where nothing is hit: all RT_SETS sets hold one value once the tile has had no surface
//     in RT_SETS consecutive frames -- the same frames;
//   * this set's bin counts are 0 WITHOUT a split mark: frame f - RT_SETS wrote them from the cost record (binWork, two of them by frame
//     parity) that the traversal of frame f - RT_SETS - 2 left: that frame had no rays here either -- f - RT_SETS - 1, f - RT_SETS - 2 in
//     the run as well; both cost records then read 0 (zeroed by the ray generations of frames f - 1 and f - 2 or found 0 by them, and
//     the traversal does not touch the bins of a tile whose word is 0).
// The reflection V pass (denoise.hip) leaves a block alone when all its tiles have a run of RT_SKY_V_RUN: FilteredOut1 exists once, and the
// previous frame's V pass stored the same conversion of the same sky texels there.
// The temporal pass and the tone map (denoise.hip "settled sky") ask for a run of RT_SKY_WINDOW_RUN in every tile their window touches, and
// for no more: they keep no copy of anything from an earlier frame that a run would have to vouch for -- what is already in place they
// compare bit by bit (the settled words).  The run only has to say what this frame's INPUTS are over the window:
//   * a run of 1 under the current epoch: this frame's ray generation found the tile without a surface at rate 1.  It then stored velocity 0
//     and the environment texel behind the pixel into this set, or validly left them in place (RT_SKY_PREV_RUN); both are functions of the
//     pixel and the epoch alone (rt_sky_chain.h rayGeneration: the camera and the environment are in the epoch, jitter and frame index do
//     not enter a sky pixel);
//   * the reflection V pass of this frame stored that texel's conversion, alpha 0, into FilteredOut1 -- every pixel without a surface takes
//     storeSkipped, in a tile without a surface or beside one -- or validly left it in place (RT_SKY_V_RUN).
// A longer run would add nothing: the frame before is covered by the settled word, which is set only by a block whose window had these
// runs in ITS frame, under the same epoch.
#define RT_SKY_PREV_RUN (RT_SETS + 2)
#define RT_SKY_V_RUN 2u
#define RT_SKY_WINDOW_RUN 1u
// Settled words (rtggx_context::settled): epoch << 8 | flags of one 64 x 4 block of the temporal pass
#define RT_SETTLED 1u          // the block's texels of this frame are, bit for bit, the ones the other history image holds
#define RT_SETTLED_SKIPPED 2u  // ... and the block was left alone for it (a mark for tests: readers mask it)
#define RT_SETTLED_BORDER 0xFFFFFFFFu      // a word outside the grid (no block's word: flags are two bits)
#define RT_SKY_RUN_CAP 255u
namespace rt {

// A queue of shadow rays with its owners: what one pass of direct lighting (lighting.hip) fills, traces through the any-hit traversal and adds
// from.  The format of an input set's bins (rt_queue.h, where the methods are): numBins bins of `slots` ray records and hit keys, a count
// per bin, and -- the local lights -- the rays' own (tmin, tmax) per slot.  view(): what launchTrace takes, the queue's own shape in it.
struct TraceQueue;
struct ShadowQueue {
  DevBuf<void> rays, hits, range; DevBuf<uint32_t> count; uint32_t slots = 0;
  int ensure(uint32_t numBins, uint32_t binSlots, bool withRange, bool& filled);
  void release();
  TraceQueue view() const;
};

// What a build tells the host: written by the build's kernels, copied to pinned memory behind its last one.
#define RT_TREELET_LEVELS 3
struct BuildResult {
  uint32_t numRounds;                        // PLOC rounds (= entries of roundBase - 1)
  uint32_t treelets[RT_TREELET_LEVELS];      // refit treelets per level (lbvh.hip "treelets")
  uint32_t topCount;                         // entries of the LDS table of the tree's top
  uint32_t depth;                            // deepest leaf (number of ancestors)
  uint32_t stack4, depth4, nodes4;           // the 4-wide collapse (lbvh.hip roots4Kernel): the most entries a traversal's stack can hold, its levels, its nodes
  uint32_t error;                            // bit 0: more than RT_MAX_ROUNDS rounds; bit 1: a treelet level beyond RT_TREELET_LEVELS would be needed
  uint32_t itemCursor, roundCursor;
  uint32_t finalEntry, finalLds;             // statistics of plocFinal: clusters handed to it, clusters when its LDS rounds began
  float cost, pad2;                          // sum of the node-box half-areas (SAH cost up to constants)
};
// Everything a build derives from ONE vertex shape that refits of later shapes keep using (lbvh.hip): the binary topology (PLOC creates
// nodes in rounds; a node's children are leaves or nodes of EARLIER rounds, and node indices are handed out round by round), the
// per-primitive and per-node boxes of the latest refit, the refit schedule (treelets of <= 1024 nodes, one workgroup each, level by
// level), the list of nodes at the tree's top.  All of it is produced on the device without a host round trip; the host learns a
// handful of counts (BuildResult) when the build has ended.
struct BvhTopo {
  DevBuf<uint32_t> order;        // leaf slot -> primitive (Morton order)
  DevBuf<int32_t> left, right, nodeParent, leafParent;
  DevBuf<float> nodeBox, triBox;
  DevBuf<uint32_t> cnt[RT_TREELET_LEVELS];   // per node: nodes of its subtree that treelet level l still has to place
  DevBuf<uint32_t> roundBase;                // device: first node of PLOC round k
  DevBuf<void> dTreelets, dRefitItems; DevBuf<uint32_t> dRefitRounds; DevBuf<int32_t> treeletRoots;
  DevBuf<int32_t> topList, topRank;
  DevBuf<float4> cost4;          // the collapse's dynamic programme per binary node: F(n, 1..3) and the choices (lbvh.hip collapseCostTreelets)
  DevBuf<int4> ent4; DevBuf<uint32_t> lvl4;            // the 4-wide collapse: per binary node the entries it has as a 4-wide node, and its level there (~0: it is not one)
  DevBuf<BuildResult> dResult; PinnedBuf<BuildResult> hResult;         // device record, pinned copy
  BuildResult result{};                      // the host's copy, valid once the build has ended
  uint32_t numTris = 0; int32_t root = -1;
  bool refittable = false;                   // a PLOC build of more than one triangle (the refit needs its rounds)
};

struct MeshDev {
  MeshDev(); ~MeshDev();         // (lbvh.hip, where BuildJob is complete)
  // Owner and view: every array that exists once per input set when the mesh deforms and once while it is static is an array of owners
  // (xOwn: a static mesh fills entry 0 alone) and an array of views (xBuf: what the kernels are given, all entries valid, all equal to entry
  // 0 while the mesh is static).  verts, fat, nodes, nodes4, tris, top: views of the CURRENT input set's entry (selectSet).
  float* verts = nullptr;        // view; 6 floats per vertex
  // A mesh whose vertices change per frame (rtggx_refit_as) keeps one vertex buffer per input set: the shading of frame f on the
  // main stream still reads the vertices of frame f while stream B already moves them for frame f + 1.  A static mesh has one
  // allocation, and the three pointers alias it.
  DevBuf<float> vertsOwn[RT_SETS]; float* vertsBuf[RT_SETS] = {};
  // "Fat triangles": per primitive its three 24-byte vertices side by side (80 bytes = 5 x 16: p0 n0 p1 n1 p2 n2 + 8 pad), indexed by
  // primitive id.  Ray generation and hit shading fetch a triangle's vertices with five 16-byte loads in ONE dependent step instead of
  // three index loads followed by eighteen 4-byte loads (two steps): these kernels are latency-bound (profiles/r02_d_limiter.txt).
  // Per input set like the vertices; rebuilt from them by a refit.
  float4* fat = nullptr; DevBuf<float4> fatOwn[RT_SETS]; float4* fatBuf[RT_SETS] = {};
  uint32_t vertsVersion[RT_SETS] = {}, version = 0, latestSet = 0;
  bool deforming = false;
  PinnedBuf<float> stage[RT_SLOTS];   // pinned host staging ring for the vertices handed to rtggx_refit_as
  uint32_t stageNext = 0; int pendingStage = -1;
  DevBuf<float> deviceStage[RT_SLOTS];   // device-side staging ring of rtggx_refit_as_device; the events that order it against the caller's stream
  uint32_t deviceStageNext = 0; int pendingDeviceStage = -1; Event evProduced, evStaged;
  // what a build derives from one vertex shape and a refit keeps: `topo` (BvhTopo above); `job`: a build in progress (lbvh.hip BuildJob)
  BvhTopo topo;
  std::unique_ptr<struct BuildJob> job;
  bool wantRebuild = false;      // the refitted tree's cost has drifted: the next frame starts a rebuild
  uint32_t topoVersion = 0, topoVersionOfSet[RT_SETS] = {};      // a set whose tree arrays were emitted for an older topology is emitted in full by its next refit
  DevBuf<float> dCost;           // device: sum of the node-box half-areas of the current tree (SAH cost up to constants)
  PinnedBuf<float> hCost;        // pinned: its copy, refreshed asynchronously after every refit
  Event evCost; bool costInFlight = false;
  float builtCost = 0.0f, lastCost = 0.0f;
  uint32_t refits = 0, rebuilds = 0;
  DevBuf<uint32_t> indices;
  uint32_t numVerts = 0, numIndices = 0, numTris = 0;
  BvhNode* nodes = nullptr;      // view; numTris - 1 (0 when numTris == 1): the binary LBVH as built
  Bvh4Node* nodes4 = nullptr;    // view; same count, sparse: the 4-wide collapse the trace kernel walks
  BvhTri* tris = nullptr;        // view; numTris, leaf (Morton) order
  // the three above are those of the CURRENT input set: like the vertices, the boxes and leaf triangles of a deforming mesh exist
  // once per input set (frame f + 1's refit on stream R writes its set while frame f's traversal still walks the other)
  DevBuf<BvhNode> nodesOwn[RT_SETS]; DevBuf<Bvh4Node> nodes4Own[RT_SETS]; DevBuf<BvhTri> trisOwn[RT_SETS];
  BvhNode* nodesBuf[RT_SETS] = {}; Bvh4Node* nodes4Buf[RT_SETS] = {}; BvhTri* trisBuf[RT_SETS] = {};
  // the top of the tree once more, breadth-first, for the trace kernel's LDS (rtggx_device.h RT_TOP_*; lbvh.hip planTopKernel / emitTop):
  // topo.topList[k] = node of rank k, topo.topRank[node] = its rank or -1; the table itself per input set like the nodes
  uint32_t topCount = 0; uint32_t topCountBuf[RT_SETS] = {};
  Bvh4Node* top = nullptr; DevBuf<Bvh4Node> topOwn[RT_SETS]; Bvh4Node* topBuf[RT_SETS] = {};
  int32_t root = -1;             // 0, or ~0 for a single-triangle mesh
  uint32_t depth = 0;            // deepest leaf (number of ancestors)
  uint32_t stack4 = 0;           // the most entries a traversal of the 4-wide tree can have on its stack (BuildResult::stack4 of the latest topology)
  float bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};   // vertex bounds (Morton normalisation box)
};

struct EnvDev {
  DevBuf<uint2> texels;          // RGBA16F, mip-major, 6 faces per mip
  uint32_t size = 0, mips = 0;
  uint32_t mipOffset[16] = {};   // texel offset of mip m (face 0)
  uint64_t totalTexels = 0;
};

// Everything the per-frame kernels need, passed by value as one kernel argument.
struct FrameParams {
  RtggxCBGlobal g;
  RtggxRayGenConstants rg;
  RtggxCBPerObject po[2];
  RtggxCBMaterial mat;
  float invWorld[2][16];         // TLAS: world -> object, row-vector row-major
  uint32_t W, H;
  uint32_t rowBegin, rowEnd;     // strip of the frame this context renders
  uint32_t flags;                // RT_FLAG_*
  uint32_t sampleMask;           // rtggx_set_sample_set: M - 1 of the frame's sample set (raytrace.hip sampleParamWide; the 256-member code does not read it)
  uint32_t pad[2];
};
#define RT_FLAG_VNDF 1u          // rtggx_set_sampler: visible-normal sampling of the reflection lobe instead of the reference's NDF sampling

// One input set: everything stream B's stages write for a frame and the main stream reads (allocated by context.hip allocSet).
struct InputSet {
  DevBuf<uint32_t> normal, velocity, rtRefl, rtDiff;
  DevBuf<uint16_t> roughMetal;
  DevBuf<uint32_t> depth32;          // the D24 word of visDepth once more, 4 bytes per pixel, for the spatial filters (written by ray generation)
  // ray bins of the trace pass (rt_queue.h): numBinsMax bins of binSlots ray records and hit keys, and the rays in each bin
  DevBuf<void> rayQueue, hitQueue;
  DevBuf<uint32_t> binCount;
  // Bins whose traversal was expensive in the previous frame are traced by 2, 4 or 8 waves (trace.hip "adaptive split"): [RT_SPLIT_CAP]
  // (shift << 28) | (slice << 24) | bin, one entry per wave of a listed bin.  Per set: the visibility pass of the next frame, which empties
  // its set's list, may run beside this frame's traversal.  The count is a word of largeCountBase (zeroed by the previous frame's ray generation).
  DevBuf<uint32_t> splitList; uint32_t* splitCount = nullptr;      // (splitCount: a view)
  // "Still sky" (raytrace.hip rayGenKernel): one word per 16x16 tile of ray generation's grid, epoch << 8 | run.  run: the consecutive frames,
  // this set's included and saturating at RT_SKY_RUN_CAP, in which ray generation found the tile's word 0 under one epoch (rt_sky_chain.h
  // SkyChain).  Written by the set's ray generation, read by the next frame's (earlier on the same stream, like roughMetalPrev) and by the
  // set's own reflection V pass behind the traversal's event; protected by evRead like the set's other members.
  DevBuf<uint32_t> skyRun;
  Event evRead;                     // the set's last reader done: the HOST waits for it before stream B is given work that overwrites the set
  bool readRecorded = false;
};

// One visibility target (RT_VIS_RING above), by frame number.
struct VisTarget {
  DevBuf<unsigned long long> depth;         // visDepth
  // One word per 16x16 tile, set by the rasterisers where they draw: a tile whose word is 0 holds nothing but the clear value, and ray
  // generation neither reads nor re-clears it (three quarters of the bunny frame: 16 bytes per pixel and the first of its dependent
  // fetches).  Tiles are ray generation's, counted from the pass's first row: the words mean something only for the rows they were kept
  // under (flags.rows; another strip: everything is read and cleared, which also resets the words).
  DevBuf<uint32_t> dirty;
  struct { uint32_t frame = 0, rows[2] = {0, 0}; } cleared;      // a ray generation has cleared the target, over these rows, FOR this frame (0: not)
  struct { uint32_t rows[2] = {0, 0}; uint32_t rasterFrame = 0; } flags;      // word 0 => tile clear, for tiles counted from rows[0]; rasterFrame: the frame whose visibility pass drew into the target last
};

// What the stages of frame f tell the streams of later frames, by f & 3 (frame.hip rtggx_render_visibility).
struct FrameEvents {
  Event gen;                         // ray generation of frame f done (C -> B: traversal f; C -> R: the visibility pass of frame f + 2, whose target and lists it cleared)
  uint32_t genFrame = 0;             // the frame it belongs to (0: none)
  hipStream_t genStream = nullptr;   // and its stream (a view)
  Event trace;                       // traversal of frame f done (B -> main; B -> C two frames later: binWork)
  bool traceRecorded = false;
};

}  // namespace rt

// The 4-wide collapse's objective (lbvh.hip): cost of a 4-wide node = AREA x half-area / the root's + TRIS x triangles / all triangles.
#ifndef RT_COLLAPSE_AREA_WEIGHT
#define RT_COLLAPSE_AREA_WEIGHT 1.0f
#define RT_COLLAPSE_TRIS_WEIGHT 0.0f
#endif
#define RT_MAX_PEERS 16      // ranks whose history images a context can map (rtggx_set_history_peers): one node has eight GPUs

struct rtggx_context {
  int device = 0;
  uint32_t W = 0, H = 0;
  uint32_t rowBegin = 0, rowEnd = 0;
  uint32_t historyApron = 18;           // rows of TemporalSSOut beyond the strip the caller delivers between frames (rtggx_set_history_apron)
  rt::DevBuf<uint32_t> histReach;       // device word: the furthest a history tap reached beyond them, in rows (temporalKernel)
  // Streams: the four the context creates are owners; streamMain, streamAS, streamVis (and sppStream, shadeStream, diffStream, evVisStream
  // below) are views -- of one of them, or of the caller's stream (rtggx_set_stream).
  rt::Stream ownMain; hipStream_t streamMain = nullptr, streamAS = nullptr;
  rt::Stream streamRefit;                          // stream R: vertex uploads and tree refits of deforming meshes (rtggx_refit_as)
  // Frame pipeline (frame.hip): three stages on three streams -- C: visibility + ray generation, B: traversal, main: shading + denoiser +
  // tone map -- so that ray generation of frame f + 1 runs beside the traversal of frame f.
  bool refitIssued = false;                        // per-frame issue state (frame.hip)
  uint32_t frameCounter = 0;                       // frames started (rtggx_render_visibility); parity selects binWork / ray counters
  rt::FrameEvents frames[4];                       // by frame & 3
  rt::FrameEvents& frameEvents(uint32_t f) { return frames[f & 3u]; }
  rt::Stream ownAS, ownVis;                        // the context's own stream B / stream C; streamAS / streamVis alias streamMain / null while
  bool asyncCompute = true;                        // rtggx_set_async_compute(0) is in force (the sample's [A] toggle: one queue, submission order)
  // Launches with few rays (thin strips, small frames) leave most of the machine idle and last as long as stream B's chain
  // of dependent kernels: there the visibility pass of frame f+1 runs on a stream of its own (C), beside the traversal
  // of frame f, instead of behind it.  (On full frames the machine is saturated and this gains nothing.)
  hipStream_t streamVis = nullptr;
  rt::Event evVis;                      // completes with the last kernel of the most recent visibility pass, on either stream
  hipStream_t evVisStream = nullptr;    // the stream the most recent visibility pass ran on (null: none yet)
  rt::Event evAS;                 // constants uploaded (stream B -> main)
  rt::Event evRefit;              // vertices of the current set uploaded and the tree refitted (stream B -> stream C)
  rt::Event evRT;                 // ray trace done (stream B -> main)
  int setReadDeferred = -1;       // the set whose evRead is still to ride on a later kernel of this frame (frame.hip settleSetRead)
  double fenceWaitUs = 0.0; uint32_t fenceWaits = 0;      // host time spent waiting at the frames-in-flight fence (rtggx_render_visibility; rtggx_debug_fence_wait)
  // The temporal pass and the tone map as one kernel (denoise.hip temporalToneKernel): rtggx_denoise then writes the back buffer as well and
  // the rtggx_tone_map that follows it in the same frame has nothing left to launch.  -1: where it pays -- small launches (frame.hip
  // rtggx_denoise); rtggx_debug_fuse_tone_map(ctx, 0 / 1): never / always.
  int fuseToneMap = -1; bool toneMapDone = false, denoiseIssued = false;
  // Multi-GPU strips: every rank's two history images as mapped into THIS process (rtggx_set_history_peers) -- device table
  // [2][RT_MAX_PEERS] pointers + [RT_MAX_PEERS + 1] row boundaries; a history tap beyond the exchanged apron reads the owner's image.
  rt::DevBuf<uint32_t> exchangeTokens;     // RTGGX_BUF_EXCHANGE_TOKENS
  float collapseWeights[2] = {RT_COLLAPSE_AREA_WEIGHT, RT_COLLAPSE_TRIS_WEIGHT};      // rtggx_debug_collapse_weights
  uint32_t peerWorld = 0; rt::DevBuf<void> dPeerTable; std::vector<rt::IpcMapping> ipcMapped;      // (what rtggx_history_ipc_open mapped: unmapped with the context)
  uint32_t lastPlacement[2] = {0, 0};      // key and placement of the most recent rtggx_ray_trace (rtggx_debug_placement)
  int forcePlacement = -1;       // rtggx_debug_placement: -1 by the ray count; 0 / 1: the placement of a full-size / a small launch whatever the count
  bool fltRflIsFltDff = false;          // the last denoise ran without diffuse passes: FilteredOut == FilteredOut1 and only the latter was written
  bool externalStream = false;

  bool vndf = false;             // rtggx_set_sampler
  // rtggx_set_sun: a directional light with ray-traced shadows (lighting.hip launchSun).  Requested values take effect with the next
  // rtggx_render_visibility, like the other per-frame settings.  The queue is the sun's own -- the frame's bins are still read by the shading of the
  // frame in flight, and still sky relies on their counts --: one ray slot per pixel of a bin's 8x8 sub-tile, 48 + 8 bytes per pixel and 4 per bin,
  // allocated by the first call that turns the sun on.
  struct Sun { bool on = false; float L[3] = {}, E[3] = {}, T[3] = {}, B[3] = {}; } sun, sunRequested;      // T, B: the disk's frame about L (rtggx_set_sun_angle), made with L
  rt::ShadowQueue sunQueue;
  // rtggx_set_sun_angle: the angular radius of the sun's disk in degrees and k = 1 - cos of it.  Stored whether or not a sun is set; the
  // frame's, the next frame's.  0: the directional sun, and the SOFT = false kernels (lighting.hip launchSun, launchSunHits).  No buffer.
  struct SunAngle { float degrees = 0.0f, k = 0.0f; } sunAngle, sunAngleRequested;
  // rtggx_set_sun_reflections: the sun term and the shadow at the surfaces the paths hit (lighting.hip launchSunHits).  Stored whether or not a
  // sun is set; the frame's, the next frame's.  Everything below exists from the first frame that has both on (lighting.hip beginSunHits):
  //   sunHitQueue  a queue of the feature's own, bins of binSlots slots (released when the bins grow)
  //   sunHitSums   S of the one-sample frame: [2][W * H] float4 -- the sum of the terms r, g, b and the number of terms --, all zero between
  //                frames (sunHitResolveKernel leaves them so)
  // ONE of each for all input sets, like sppAcc: consecutive frames' passes follow each other in stream order, or by evSunHit where the
  // stream changes (sunHitStream: a view, the stream of the most recent frame that used them).
  bool sunReflections = false, sunReflectionsRequested = false;
  rt::ShadowQueue sunHitQueue; rt::DevBuf<float> sunHitSums;
  hipStream_t sunHitStream = nullptr; rt::Event evSunHit;
  // rtggx_set_lights: point and spot lights with ray-traced shadows (lighting.hip launchLights).  The requested list takes effect with the next
  // rtggx_render_visibility, like the sun.  Everything below exists from the first frame with count > 0 (lighting.hip launchLights):
  //   lightQueue   ONE queue in the sun's format for all lights -- bins of RT_BIN_MIN slots --, refilled light by light, with the rays' own
  //                (tmin, tmax) beside it
  //   lightSums    S0 and S1: [2][W * H] float4 -- the sum of the terms r, g, b and the number of terms --, all zero between frames (the
  //                resolve leaves them so)
  // The pass runs on the main stream only: consecutive frames' kernels follow each other there.
  struct Lights { uint32_t count = 0; RtggxLight l[RTGGX_MAX_LIGHTS] = {}; } lights, lightsRequested;
  rt::ShadowQueue lightQueue; rt::DevBuf<float> lightSums;
  // rtggx_set_light_reflections: the lights' terms and shadows at the surfaces the paths hit (lighting.hip launchLightHits).  Stored whether or
  // not lights are set; the frame's, the next frame's.  From the first frame that has lights and the toggle on (lighting.hip beginSunHits):
  //   lightHitQueue  a queue of the feature's own with the rays' intervals beside it, bins of binSlots slots (released when the bins grow),
  //                refilled light by light and level by level
  // S of the one-sample frame, the event and the stream view are the sun's hit pass's (sunHitSums, evSunHit, sunHitStream): the two features
  // add into one sum per (pixel, image) and one resolve packs it.
  bool lightReflections = false, lightReflectionsRequested = false;
  rt::ShadowQueue lightHitQueue;
  // rtggx_set_light_sampling: 0 a shadow ray per light, 1 one per surface point for all lights (lighting.hip launchLights, launchLightHits:
  // the picking kernels in place of the per-light loops).  Stored whether or not lights are set; the frame's, the next frame's.  From the
  // first mode-1 frame with lights:
  //   lightPickDiff  the chosen light's finished diffuse term beside lightQueue, one float4 per ray slot
  uint32_t lightSampling = 0, lightSamplingRequested = 0;
  rt::DevBuf<float> lightPickDiff;
  // rtggx_set_light_pick_visibility: the pick weighted by the pixel's remembered visibility (lighting.hip launchLights: the Vis kernels in
  // place of the picking pair of the primary pass).  Stored always; the frame's, the next frame's.  From the first acting frame (mode 1, a
  // casting light, the setting on):
  //   lightVisImg    two images of W x H RtggxLightVisRecord (four words each); frame s writes [s & 1] and reads [(s - 1) & 1]
  //   lightVisSeq    s, the number of acting frames; lightVisSeq0: s at the last reset (the setters, the allocation)
  // The records are not per input set: consecutive frames' passes follow each other on the main stream.
  bool lightVis = false, lightVisRequested = false;
  uint32_t lightVisSeq = 0, lightVisSeq0 = 0;
  rt::DevBuf<uint32_t> lightVisImg[2];
  // rtggx_set_light_list_visibility: the same for a list (lighting.hip launchLights: lightListVisGenKernel, lightListVisAddKernel in the
  // list's branch), with a sequence and two images of W x H RtggxLightListVisRecord of its own, from the first acting frame (a list with a
  // casting light, the setting on).  Resets: the allocation, every successful rtggx_set_light_list, every change of the setting.
  bool lightListVis = false, lightListVisRequested = false;
  uint32_t lightListVisSeq = 0, lightListVisSeq0 = 0;
  rt::DevBuf<uint32_t> lightListVisImg[2];
  // rtggx_set_light_list: up to RTGGX_MAX_LIGHT_LIST lights in device memory under mode 1's rule, culled per 8x8 block (lighting.hip
  // lightListGenKernel, lightListHitGenKernel).  The context holds this list or rtggx_set_lights' (the setters refuse the other); the
  // requested list takes effect with the next rtggx_render_visibility, which uploads it where its version differs (lighting.hip
  // uploadLightList).  From that upload:
  //   lightListRecs  the 64-byte records (LightArgs, the neutral cone where a light has none), lightListCapacity of them
  //   lightListCull  (Pl, R) per light, R = 0 where it casts nothing
  //   lightListCasting, lightListVariant  how many lights cast rays, and the instance [2 cone + soft] the list runs
  // and from the first frame with a list:
  //   lightListKept  the kept lights per 8x8 block of the last such frame's primary pass (rtggx_read_light_list_counts); lightListFrame:
  //                  such a frame has run since the last upload
  // lightQueue, lightSums, lightPickDiff and lightHitQueue are used as in mode 1.
  struct LightList { uint32_t count = 0; uint64_t version = 0; std::vector<RtggxLight> l; uint32_t kinds = 0; bool presumed = false; } lightList, lightListRequested;
  rt::DevBuf<float> lightListRecs, lightListCull; uint32_t lightListCapacity = 0, lightListCasting = 0, lightListVariant = 0;
  rt::DevBuf<uint32_t> lightListKept; bool lightListFrame = false;
  bool lightListCullOn = true;      // rtggx_debug_light_list_cull
  uint64_t lightListVersions = 0;      // successful rtggx_set_light_list calls that changed what is held: the next list's version
  // rtggx_update_light_list, rtggx_update_light_list_device: lights that move (lighting.hip "Moving light lists").
  // Nothing below exists before the first update.  The list's device storage becomes a ring of VERSIONS: a version is written once --
  // by the host path's staged copy, by lightListPrepareKernel, by both in call order --, read by every frame from the
  // rtggx_render_visibility that takes it until the next that takes another, and written again only when the last frame that read it
  // has ended (evRead, recorded on the main stream behind the frame's last pass over the list).  A LightList's kinds / presumed: what
  // the device path's callers declared, and that its values are no longer the host's to know (the list is presumed casting).
  //   buf        count records of 64 bytes, then count cull entries of 16 (capacity RTGGX_MAX_LIGHT_LIST: any list fits any version)
  //   stage      the same, pinned: the host path's staging; staged: a copy out of it has been enqueued since the version was opened
  //   evWritten  behind the last write, on writeStream; evCopied: behind the last copy out of it into a newer version
  //   lightListRecsCur / CullCur  what the frame's kernels read: a version's, or lightListRecs / lightListCull (lightListCur = -1)
  //   lightListNewest  where the newest complete list lies (-1: lightListRecs / lightListCull); lightListPend: the version the updates
  //                    since the last rtggx_render_visibility have opened (-1: none); lightListStored: the LightList::version it holds
  //   lightListDirtyLo / Hi  the host path's lights not yet on the device
  struct LightListVersion {
    rt::DevBuf<float> buf; rt::PinnedBuf<float> stage; rt::Event evWritten, evRead, evCopied;
    hipStream_t writeStream = nullptr; bool written = false, readRecorded = false, copied = false, staged = false;
  };
  static constexpr uint32_t kLightListVersions = 8u;      // more than the frames in flight (RT_SETS) plus the one being written
  LightListVersion lightListRing[kLightListVersions]; bool lightListRingReady = false;
  const float* lightListRecsCur = nullptr; const float* lightListCullCur = nullptr;
  int lightListCur = -1, lightListNewest = -1, lightListPend = -1; uint32_t lightListRingNext = 0;
  bool lightListAwaitWritten = false;      // the frame's version may still be on its way: the streams that read it wait for evWritten
  uint64_t lightListStored = 0;
  uint32_t lightListDirtyLo = 0, lightListDirtyHi = 0;
  rt::DevBuf<unsigned long long> lightListRejects;      // rtggx_read_light_list_rejects: the device path's refused lights, one word
  uint32_t visibilityDrains = 0;      // rtggx_debug_visibility_drains: rtggx_render_visibility's waits for every stream
  uint32_t rayRate = 1;         // rtggx_set_ray_rate: pixels per traced ray, 1 or 4 (raytrace.hip rayGenKernel, reconstructKernel)
  uint32_t maxDepth = 1, depthRequested = 1;      // rtggx_set_max_recursion_depth: 1..4 levels of rays per path (raytrace.hip launchShade); the frame's, the next frame's
  // rtggx_set_samples_per_pixel: 1, 2, 4 or 8 samples per covered pixel (raytrace.hip launchShade; DESIGN.md "Samples per pixel"); the
  // frame's, the next frame's.  Everything below exists from the first N > 1 on (context.hip allocSamples):
  //   sppAcc     the fp32 sums of RayTracingOut0 / RayTracingOut1, [2][W * H][3] floats, all zero between frames (the resolve leaves them so).
  //              ONE pair for all input sets: the frames' shading passes follow each other in stream order, or by evSpp where the stream changes
  //   sppParams  [RT_SLOTS][RTGGX_MAX_SAMPLES_PER_PIXEL] copies of the slot's frame constants, sample k's with FrameIndex * N + k
  uint32_t samples = 1, samplesRequested = 1;
  rt::DevBuf<float> sppAcc; rt::DevBuf<rt::FrameParams> sppParams;
  hipStream_t sppStream = nullptr; rt::Event evSpp;      // (a view:) the stream of the most recent frame that used sppAcc
  // rtggx_set_accumulation (raytrace.hip accumulateKernel; DESIGN.md "Progressive accumulation"): the frame's, the next frame's.  The sums
  // exist ONCE, from the first enable on (context.hip allocAccumulation), [W * H] float4 each -- sum r, g, b, Y^2 of RayTracingOut0 / 1 --, and
  // are touched by the main stream alone (the kernel behind the hit shading, the reset's clears, the present): stream order is the order of
  // the frames.  accumFrames: frames added since the last reset, counted by the host as it enqueues them.
  bool accumulate = false, accumulateRequested = false;
  uint32_t accumFrames = 0;
  // rtggx_set_sample_map (raytrace.hip launchShadeSamples; DESIGN.md "Adaptive sampling"): one count per ray bin of the full frame, a byte
  // each in bin order -- a tile's four counts are one word, read by a wave with one scalar load like the tile word; bins beyond the
  // frame's blocks hold 1.  Two copies, allocated with the first set: a set writes the one
  // no frame reads (it has waited for every stream; a frame whose visibility pass has run keeps the one it was launched under), and
  // rtggx_render_visibility takes the requested one over.  -1: no map.
  rt::DevBuf<uint32_t> sampleMapBuf[2];
  int sampleMap = -1, sampleMapRequested = -1;
  const uint32_t* sampleMapWords() const { return sampleMap < 0 ? nullptr : sampleMapBuf[sampleMap].get(); }
  rt::DevBuf<float4> accRefl, accDiff; rt::DevBuf<uint2> converged;      // converged: RTGGX_BUF_CONVERGED (rtggx_present_accumulation)
  // rtggx_set_reference / rtggx_set_scoring (score.hip; DESIGN.md "Scoring against a reference"): the frame's, the next frame's.  Nothing
  // below exists on a context that never calls them (context.hip allocReference, allocScoring).
  //   reference      W * H RGBA16F words, written by rtggx_set_reference (host copy) or rtggx_reference_from_accumulation (main stream)
  //   scorePartial   the tree's levels, ping-pong: [0] RT_SCORE_SUMS x scoreStride doubles -- one per sum and chunk of RT_SCORE_CHUNK pixels,
  //                  sum-major --, [1] half of that; scoreCounts: 3 words per chunk (covered, skipped_out, skipped_raw)
  //   scoreRing      RTGGX_SCORE_RING records, slot = index % RTGGX_SCORE_RING
  // ONE set of partials for all frames: both stages of every frame run on the main stream, in its order.  scoreIndex: frames scored so
  // far, counted by the host as it enqueues them; scoreRead: the first record rtggx_read_scores has not handed out yet.
  bool scoring = false, scoringRequested = false;
  rt::DevBuf<uint2> reference;
  rt::DevBuf<double> scorePartial[2]; rt::DevBuf<uint32_t> scoreCounts; uint32_t scoreStride = 0;
  rt::DevBuf<RtggxScore> scoreRing;
  uint64_t scoreIndex = 0, scoreRead = 0;
  uint32_t traceGrid[4] = {};    // the frame's level-0 trace launch -- bins, tile grid x / y, slice shift --, which the later levels repeat
  float rebuildRatio = 1.2f; uint32_t rebuildSteps = 16;      // rtggx_set_refit_policy
  rt::MeshDev mesh[2];
  rt::EnvDev env;
  rt::DevBuf<float> sh;          // 27 floats
  rt::DevBuf<float> cosSinTab;   // 512 floats: cos[256], sin[256]
  // rtggx_set_sample_set (raytrace.hip sampleParamWide; DESIGN.md "Sample-set size"): M of the frame, of the next frame; 256 = the reference's.
  // One table per size M = 512 << k ever asked for, M {cos, sin} pairs, made by the setter and kept as long as the context: a frame in flight
  // and a frame whose visibility pass has run keep the table they were launched with whatever the caller sets next.
  uint32_t sampleSet = RTGGX_MIN_SAMPLE_SET, sampleSetRequested = RTGGX_MIN_SAMPLE_SET;
  rt::DevBuf<float> cosSinWide[8];
  static uint32_t sampleSetSlot(uint32_t m) { uint32_t k = 0; while ((512u << k) < m) ++k; return k; }
  const float* sampleTable() const { return sampleSet > RTGGX_MIN_SAMPLE_SET ? cosSinWide[sampleSetSlot(sampleSet)] : cosSinTab; }

  // render targets
  // Everything the visibility and ray-tracing passes write and the denoiser (main stream) reads exists RT_SETS times (the input sets), so
  // that frame N+1's visibility + ray trace overlap frame N's denoise + tone map; the visibility target RT_VIS_RING times.  cur() is the
  // set of the frame being rendered (advanced by rtggx_render_visibility), prev() / next() the sets of the frames before and after it;
  // curVis() the frame's target.
  rt::InputSet sets[RT_SETS];
  uint32_t setIndex = 0;
  uint32_t setAhead(uint32_t k) const { return (setIndex + k) % RT_SETS; }      // the set of the frame k after this one (of RT_SETS - k before it)
  rt::InputSet& cur() { return sets[setIndex]; }
  rt::InputSet& prev() { return sets[setAhead(RT_SETS - 1u)]; }
  rt::InputSet& next() { return sets[setAhead(1u)]; }
  rt::VisTarget vis[RT_VIS_RING];
  rt::VisTarget& visOf(uint32_t frame) { return vis[frame % RT_VIS_RING]; }
  rt::VisTarget& curVis() { return visOf(frameCounter); }
  void selectSet(uint32_t i) {
    setIndex = i;
    largeTris = largeTrisBuf[frameCounter & 1u]; largeCount = largeCountBase ? largeCountBase + (frameCounter & 1u) : nullptr;
    for (auto& m : mesh) { m.verts = m.vertsBuf[i]; m.fat = m.fatBuf[i]; m.nodes = m.nodesBuf[i]; m.nodes4 = m.nodes4Buf[i]; m.top = m.topBuf[i]; m.topCount = m.topCountBuf[i]; m.tris = m.trisBuf[i]; }
    binWork = binWorkBuf[frameCounter & 1u]; rayCounter32 = rayCounterBuf + (frameCounter & 3u) * 256u;
  }
  rt::DevBuf<uint32_t> backbuffer;
  rt::DevBuf<uint2> tss[2], fltRfl, fltDff;
  uint32_t frameParity = 0;

  // visibility scratch
  // LargeTri records queued by rasterSmall, merged by rasterLarge; twice, by frame parity (ray generation of frame f empties the
  // list of frame f + 1: the count it zeroes must not be the one a consumer of frame f could still read)
  void* largeTris = nullptr; rt::DevBuf<void> largeTrisBuf[2];      // (largeTris: a view of the current frame's, selectSet)
  uint32_t* largeCount = nullptr;       // view: the current frame's count (selectSet)
  rt::DevBuf<uint32_t> largeCountBase;  // [0], [1] entries of largeTrisBuf[parity]; [2 + i] sets[i].splitCount
  // The adaptive split's record of what each bin cost (InputSet::splitList):
  uint32_t* binWork = nullptr;          // view (selectSet): [numBinsMax] lane-steps the trace kernel spent on the bin (read and zeroed by rayGenKernel)
  rt::DevBuf<uint32_t> binWorkBuf[2];   // by frame parity: ray generation of frame f reads what the traversal of frame f - 2 recorded
                                        // (frame f - 1's may still be running beside it) and the traversal of frame f records anew
  // the words of the current frame's target, for the kernels that follow its visibility pass: the target's own where they describe rows [rb, re), else all ones
  const uint32_t* tileWords(uint32_t rb, uint32_t re) {
    const rt::VisTarget& v = curVis();
    return useTileWords && !traversalBound && v.flags.rasterFrame == frameCounter && v.flags.rows[0] == rb && v.flags.rows[1] == re ? v.dirty.get() : visDirtyOnes.get();
  }
  // Still sky and settled sky (InputSet::skyRun; `settled` below): the epoch, the facts of the most recent ray
  // generation, reflection V pass, temporal pass and tone map, and every decision taken from them (rt_sky_chain.h).
  rt::SkyChain sky;
  size_t skyTiles = 0;           // words of a set's skyRun, as many as a VisTarget's
  // Settled sky (denoise.hip temporalKernel, toneMapKernel): one word per 64 x 4 block of the temporal pass, twice by
  // history parity -- array p is written by the temporal pass that writes TSS[p].  Column-major with a border: block (bx, by) of settledX x
  // settledY at (bx + 1) * settledPitch + by + 1, so that the three words of a block's column of neighbours and the six under a tone-map
  // block are consecutive and no reader clamps.  The border (a column either side, a word above, the rest of the pitch below) holds
  // RT_SETTLED_BORDER, which no kernel writes and every reader takes as settled: clamped addressing never reads outside the frame.  Words
  // count under the epoch of the run words (sky.epoch()).
  rt::DevBuf<uint32_t> settled[2]; uint32_t settledX = 0, settledY = 0, settledPitch = 0;
  size_t settledWords() const { return (size_t)(settledX + 2u) * settledPitch + 8u; }      // (+ 8: a reader's four-word load of three words may end beyond the last column)
  bool useTileWords = true;      // rtggx_debug_tile_words
  // Where the TRAVERSAL is the frame's period (two rays per pixel into a large mesh: it runs 96 % of the time) nobody asks the words:
  // workgroups over empty tiles that leave at once make the other stages' kernels run denser beside the traversal and stretch it -- dragon,
  // metallic 0.25 / 0.5: 0.354 ms without the words, 0.360 with them everywhere but in the filters, 0.378 with them in the filters as well
  // (profiles/r04_j_tile_words.txt).  Decided once per frame (launchRayTrace) from the share of the period the traversal's own time stamps
  // measure (trace.hip steerTraceWaves), with hysteresis; the words themselves are kept either way.
  bool traversalBound = false;
  const uint32_t* traceTileWords = nullptr;      // view; launchRayTrace -> launchTrace: tileWords() of the frame's G-buffer rows
  rt::DevBuf<uint32_t> visDirtyOnes;     // as many words as a VisTarget's, all ones: "every tile may hold something" (raytrace.hip GenArgs)
  uint32_t splitDemand = 0;             // entries the most recent frame whose count has arrived wanted (hostRayCounters[256])
  uint32_t splitCapForced = 0xFFFFFFFFu;   // rtggx_debug_trace_split: fixed capacity instead of the demand-driven one
  uint32_t splitWork = 0, splitMaxShift = 0;   // set at creation (RT_SPLIT_WORK, or RTGGX_SPLIT_WORK / RTGGX_SPLIT_MAX_SHIFT)
  uint32_t largeCapacity = 0;

  uint32_t numBinsMax = 0, binSlots = 64;      // bins per set; ray slots per bin (rt_queue.h RT_BIN_MIN / RT_BIN)
  rt::DevBuf<void> testRayRange;      // rtggx_trace_rays: the rays' own (TMin, TMax), one float2 per slot of an input set's bins
  rt::DevBuf<int32_t> stackOverflow;    // traversal-stack spill area (entries beyond the LDS stack), sized from
  uint32_t spillEntries = 0;            // the depth of the built trees: [spillEntries][numBinsMax * 128] words
  rt::DevBuf<void> dummyRecord;         // 128 zero bytes: record base for meshes without nodes / absent meshes
  rt::DevBuf<uint32_t> dEnvMipOffset;   // device copy of env.mipOffset
  bool lastTraceSmall = false; uint32_t traceSpillHalf = 0;
  hipStream_t shadeStream = nullptr;     // view: the stream the most recent hit shading ran on (frame.hip rtggx_ray_trace: the main stream, or the traversal's for small launches)
  // RayTracingOut1 keeps what it held where no diffuse ray is traced: with several input sets, carried over from the previous set -- by ray
  // generation when the previous frame's shading kernel wrote nothing into that set (genCarriesDiff), else by the shading kernel (raytrace.hip)
  bool genCarriesDiff = false, shadeWroteDiff = false, lastFrameDiffuse = false;
  hipStream_t diffStream = nullptr;      // the stream of the most recent frame's last writer of RayTracingOut1: the hit shading's, or at rate 4 the main stream (reconstruction)
  uint32_t numCUs = 256;
  // the trace kernel's workgroup size (full-size launches) and the time stamps it takes of itself (trace.hip): stamps = 3 x (start, end) + (sum of durations, latest start)
  uint32_t traceWaves = 12, traceWavesForced = 0; float traceShare = 0.0f; rt::DevBuf<unsigned long long> traceStamps; uint32_t traceStampLaunch = 0;
  unsigned long long traceStampSum = 0, traceStampStart = 0; uint32_t traceStampAt = 0, traceSampleLaunch = 0;      // the previous sample; the launch the sample in flight was taken at
  uint32_t traceTrial = 0, traceCooldown = 0, traceWavesSince = 0; float traceTrialBase = 0.0f;      // a trial of two more waves: samples seen, the period to beat

  // counters
  rt::PinnedBuf<uint32_t> hostRayCounters;  // pinned copy of rayCounter32[0..255], refreshed asynchronously after every trace launch
  rt::Event evRayCounters; bool rayCountersInFlight = false; uint32_t traceLaunches = 0;
  uint32_t lastFrameRays = 0xFFFFFFFFu; // rays of the most recent frame whose counters have arrived (unknown: assume a full machine)
  uint32_t* rayCounter32 = nullptr;     // view: 256 per-frame partial counts written by the trace kernel (the current frame's half of ...)
  rt::DevBuf<uint32_t> rayCounterBuf;   // ... [4][256] by frame number & 3, then 768 words of RT_TRACE_STATS counters.  (Four, not two like binWork:
                                        // ray generation of frame f zeroes its quarter, and the asynchronous copy of frame f - 2's counters to the
                                        // host, queued behind that frame's traversal, may not have run yet; frame f - 4's has.)
  uint32_t* lastRayCounter32 = nullptr; // view: the half of the most recent rtggx_ray_trace (rtggx_ray_count)
  rt::DevBuf<unsigned long long> rayCounter;  // [0..255] last frame, [256..511] running total

  // per-frame constants: ring of RayTracer::FrameCount slots (host side; kernels take them by value)
  rt::FrameParams slots[RT_SLOTS];
  uint32_t slot = 0;
  rt::DevBuf<rt::FrameParams> dParams;  // device ring, 3 slots; kernels read their constants from here
  bool slotUploaded = false;
  bool slotRendered = false;     // a frame has been rendered from this slot since rtggx_update_frame filled it: its kernels may still read the device copy
  RtggxCBMaterial material;
  float invWorld[2][16];
  bool haveConstants = false, asBuilt = false, shDone = false;

  // timing
  bool timing = false;        // all per-pass events (rtggx_get_timings)
  bool kernelRing = false;    // only the ray-trace kernel, one event pair per sampled frame in a ring (rtggx_kernel_times)
  uint32_t ringStride = 1, ringTick = 0;   // every ringStride-th frame is sampled
  std::vector<rt::Event> kevBegin, kevEnd;
  uint32_t kevCount = 0;
  rt::Event tev[16];
  bool timingsPending = false;
};

namespace rt {
// Rows each pass must cover so that the strip [rowBegin,rowEnd) of the final image is exact
// (SURVEY.md 8e): the tone map reads TSS at +-1 row, the temporal pass FilteredOut1 at +-1, the
// vertical filters the horizontal scratch at +-16.  Pure per-pixel passes recompute the apron
// instead of exchanging it.
enum RowPass { ROWS_GBUFFER /* visibility, ray trace, H filters: +-18 */, ROWS_VFILTER /* +-2 */, ROWS_TEMPORAL /* +-1 */, ROWS_FINAL };
inline void passRows(const FrameParams& fp, RowPass pass, uint32_t& b, uint32_t& e) {
  const uint32_t apron = pass == ROWS_GBUFFER ? 18u : pass == ROWS_VFILTER ? 2u : pass == ROWS_TEMPORAL ? 1u : 0u;
  b = fp.rowBegin > apron ? fp.rowBegin - apron : 0u;
  e = fp.rowEnd + apron < fp.H ? fp.rowEnd + apron : fp.H;
  if (fp.rowEnd <= fp.rowBegin) { b = e = 0; }
}
void setError(const char* fmt, ...);
#define RT_HIP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { rt::setError("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); return -2; } } while (0)
// Launches kernel k on stream s.  An event given as start or stop rides on the kernel's dispatch (hipExtLaunchKernelGGL; see `done`
// below).  hipExtLaunchKernelGGL packs the arguments by the types of the expressions it is given, so they are converted to the kernel's
// parameter types first.
template <class... P, class... A>
inline void launch(void (*k)(P...), dim3 grid, dim3 block, hipStream_t s, hipEvent_t start, hipEvent_t stop, A&&... a) {
  if (start || stop) hipExtLaunchKernelGGL(k, grid, block, 0, s, start, stop, 0, static_cast<P>(a)...);
  else hipLaunchKernelGGL(k, grid, block, 0, s, static_cast<P>(a)...);
}

// kernels / launchers implemented in the .hip files
int uploadParams(rtggx_context* c, uint32_t slot, hipStream_t s);
int launchVisibility(rtggx_context* c, const FrameParams& fp, hipStream_t s, hipEvent_t done = nullptr);
// Acceleration-structure builds (lbvh.hip).  A build is a fixed sequence of kernel launches on one stream, no host round trip in it:
//   buildLbvh          all of it at once, then ONE wait (rtggx_build_as; the sample: BuildAccelerationStructures + one WaitForGpu)
//   startRebuild       the same sequence for a mesh that deforms, from the vertices of input set `set`, into a topology of its own ...
//   continueRebuild    ... issued a few launches per frame behind the frame's refit; when the last one has ended (an event the host
//                      polls) the new topology replaces the old one between two frames.  Nothing waits.
int buildLbvh(rtggx_context* c, uint32_t slot, hipStream_t s);
int startRebuild(rtggx_context* c, uint32_t slot, uint32_t set);      // 1: started, 0: not (one is in progress, or the mesh cannot be refitted), < 0: error
int continueRebuild(rtggx_context* c, uint32_t slot, hipStream_t s, uint32_t maxSteps, bool* swapped);      // maxSteps 0: only ask whether a build whose launches are all out has ended (then the swap); > 0: only issue launches
int prepareRebuild(rtggx_context* c, uint32_t slot);      // the second topology and the build's scratch memory, once, when a mesh begins to deform
void abandonRebuild(rtggx_context* c, uint32_t slot);      // (synchronises; before the mesh's buffers are freed)
int refitLbvh(rtggx_context* c, uint32_t slot, uint32_t set, hipStream_t s);      // boxes of the existing tree from the vertices of input set `set`, into that set's BVH arrays: no host round trip
void freeBuildProducts(MeshDev& m);      // (the caller has synchronised)
int buildFatTris(rtggx_context* c, uint32_t slot, uint32_t set, hipStream_t s);      // mesh.fatBuf[set] from mesh.vertsBuf[set] and the indices
int launchRayTrace(rtggx_context* c, const FrameParams& fp, hipStream_t sGen, hipStream_t sTrace, hipEvent_t done = nullptr);   // ray generation on sGen, traversal on sTrace (joined by evGen when they differ)
// `done` (may be null) on the launch functions below: an event that completes with the pass's last kernel.  It rides on that
// kernel's own completion signal (hipExtLaunchKernelGGL) instead of a marker packet behind it: a marker costs its queue
// 5-7 us, and the frame's two chains had four of them (rocprofv3 kernel trace, profiles/).
int launchShade(rtggx_context* c, const FrameParams& fp, hipStream_t s, hipEvent_t done = nullptr);      // hit / miss shading of the traced bins
int launchSun(rtggx_context* c, const FrameParams& fp, hipStream_t s);      // rtggx_set_sun: shadow rays from the primary surface, the any-hit traversal, the add into RayTracingOut0/1
int uploadLightList(rtggx_context* c);      // rtggx_set_light_list: c->lightList to the device, behind a wait for every stream
int takeLightListUpdates(rtggx_context* c, hipStream_t s);      // rtggx_update_light_list[_device]: what the calls since the last frame left, taken by this frame (uploads on s)
void dropLightListUpdates(rtggx_context* c);      // a new list replaces them
int launchLights(rtggx_context* c, const FrameParams& fp, hipStream_t s);   // rtggx_set_lights: per light generate -> any-hit -> add into the sums, one resolve into RayTracingOut0/1
// rtggx_set_sun_reflections, rtggx_set_light_reflections (lighting.hip; called by launchShade in front of every level's shading pass): the frame's
// first use of their queues and sums on stream s, then per level the sun's pass and the lights' (HitPass: rt_queue.h), then for a
// one-sample frame the resolve
struct HitPass;
int beginSunHits(rtggx_context* c, hipStream_t s, bool wantSums, bool sunQueue, bool lightQueue);
int launchSunHits(rtggx_context* c, const FrameParams& fp, const HitPass& p);
int launchLightHits(rtggx_context* c, const FrameParams& fp, const HitPass& p);
int launchSunHitResolve(rtggx_context* c, hipStream_t s, float* sums, const uint32_t* tileWords, uint32_t tilesX, uint32_t rowBegin, uint32_t rowEnd, hipEvent_t done);      // behind the last shading pass: S into the packed words
int launchReconstruct(rtggx_context* c, const FrameParams& fp, hipStream_t s);      // rate 4: the untraced pixels of RayTracingOut0/1, after the hit shading
int allocSamples(rtggx_context* c);      // what N > 1 samples per pixel need (rtggx_context::sppAcc, sppParams), once
int allocAccumulation(rtggx_context* c);      // what rtggx_set_accumulation needs (rtggx_context::accRefl, accDiff, converged), once
int launchAccumulate(rtggx_context* c, const FrameParams& fp, hipStream_t s);      // the frame's traced images added to the sums, the strip's own rows
int launchPresentAccumulation(rtggx_context* c, hipStream_t s);      // RTGGX_BUF_CONVERGED from the sums and accumFrames
// Scoring against a reference (score.hip): a chunk is the run of pixels one workgroup reduces to one partial per sum.
#define RT_SCORE_CHUNK 1024u
#define RT_SCORE_SUMS 9u
int launchScore(rtggx_context* c, const FrameParams& fp, hipStream_t s);      // the frame's record into slot scoreIndex % RTGGX_SCORE_RING: two kernels
int launchReferenceFromAccumulation(rtggx_context* c, hipStream_t s);      // rtggx_context::reference = the mean image of the sums and accumFrames
int launchTraceRays(rtggx_context* c, const FrameParams& fp, const float* dRays, uint32_t n, float* dOut, hipStream_t s);
int launchTraceOcclusion(rtggx_context* c, const FrameParams& fp, const float* dRays, uint32_t n, uint32_t* dOut, hipStream_t s);      // the same list through the any-hit traversal (rt_queue.h)
int launchDebugEnvironment(rtggx_context* c, const float* dDirs, const float* dLevels, uint32_t n, int level0, float* dOut, hipStream_t s);      // rtggx_debug_environment: reads the environment only
int resetSettled(rtggx_context* c);      // both arrays of settled words: blocks 0, border RT_SETTLED_BORDER (context.hip; null stream, the caller has synchronised)
int launchDenoise(rtggx_context* c, const FrameParams& fp, int useLds, hipStream_t s, hipEvent_t done = nullptr, bool fuseToneMap = false);      // fuseToneMap: the last kernel also writes the back buffer
int launchToneMap(rtggx_context* c, const FrameParams& fp, hipStream_t s, hipEvent_t done = nullptr, const uint2* source = nullptr);      // source: an RGBA16F image to tone-map instead of TemporalSSOut[parity]
int decodeEnv(rtggx_context* c, int format, uint32_t size, uint32_t mips, const void* hostData, size_t bytes, hipStream_t s);
int buildEnvFromImage(rtggx_context* c, int layout, int pixels, uint32_t width, uint32_t height, const void* hostData, uint32_t size, hipStream_t s);   // rtggx_set_env_image, arguments checked
int generateEnvMips(rtggx_context* c, hipStream_t s);                                                                                                  // rtggx_generate_env_mips
int prefilterEnv(rtggx_context* c, uint32_t samples, hipStream_t s);                                                                                   // rtggx_prefilter_env, arguments checked: samples is the count itself
// one level of the prefiltered cube (raytrace.hip, beside the sampler it calls): 6 side^2 texels at dst from the box-chain cube and a table of K entries
int launchEnvPrefilter(const uint2* srcTexels, uint32_t size, uint32_t mips, const uint32_t* dSrcMipOffset, const float4* dTable, uint32_t K, float invW,
                       uint32_t side, uint2* dst, hipStream_t s);
// The sun from the environment (sunenv.hip; rt_sun_env.h: the host's arithmetic).  SunCone: what tells the cone's texels and what they are cut
// down to -- the peak texel's integer direction P, P . P, the squared cosine, the background as binary16 codes.
struct SunEnvAngles;
struct SunCone { double P[3], nP, cos2Cone; uint32_t b16[3]; };
int sunFromEnv(rtggx_context* c, const SunEnvAngles& angles, int remove, RtggxSunEstimate* out, hipStream_t s);      // rtggx_sun_from_env, arguments checked, streams waited for
void launchSunRemove(const uint2* src, uint2* dst, uint32_t size, const SunCone& cone, hipStream_t s);               // level 0 of `size` with the cone's texels cut down
int removeSunFromEnv(rtggx_context* c, const SunCone& cone, hipStream_t s);                                          // env.hip: the cut level 0, its box chain, installed
int projectSH(rtggx_context* c, hipStream_t s);
int unpackVisDepth(rtggx_context* c, uint32_t* dVis, uint32_t* dDepth, hipStream_t s);
int packVisDepth(rtggx_context* c, const uint32_t* dVis, const uint32_t* dDepth, hipStream_t s);
}  // namespace rt
