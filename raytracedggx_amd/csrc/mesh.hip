// C ABI of librtggx (include/rtggx.h), part 2 of 4: scene geometry -- mesh upload, the build of the acceleration structures, and the
// refits and rebuilds of meshes that deform (lbvh.hip has the kernels).
#include <cstring>
#include "capi_internal.h"
namespace rt {
// Vertex storage of a mesh: one allocation aliased by all input sets, or one per set once the mesh deforms; the staging ring.
static void resetMeshVerts(MeshDev& m) {
  for (int i = 0; i < RT_SETS; ++i) { m.vertsOwn[i].reset(); m.fatOwn[i].reset(); m.vertsBuf[i] = nullptr; m.fatBuf[i] = nullptr; }
  m.fat = nullptr;
  for (auto& st : m.stage) st.reset();
  for (auto& st : m.deviceStage) st.reset();
  m.evProduced.reset(); m.evStaged.reset();
  m.pendingDeviceStage = -1; m.deviceStageNext = 0;
  m.verts = nullptr; m.deforming = false; m.pendingStage = -1; m.version = 0; m.latestSet = 0;
  for (auto& v : m.vertsVersion) v = 0;
}
// Hit keys and visibility words carry the primitive in their low 24 bits, the instance above it (trace.hip, raytrace.hip,
// visibility.hip): a mesh of more triangles would alias primitive ids without a trace of it.
#define RT_MAX_TRIANGLES (1u << 24)
int setMeshImpl(rtggx_context* c, uint32_t slot, const float* verts, uint32_t nv, const uint32_t* idx, uint32_t ni) {
  if (ni / 3u > RT_MAX_TRIANGLES) { setError("rtggx_set_mesh: %u triangles, more than the %u a 24-bit primitive id can tell apart", ni / 3u, RT_MAX_TRIANGLES); return -1; }
  MeshDev& m = c->mesh[slot];
  RT_HIP(syncStreams(c));       // frames in flight on any of the streams still read the buffers freed below
  abandonRebuild(c, slot); m.wantRebuild = false;
  resetMeshVerts(m);
  freeBuildProducts(m);
  m.indices.reset();
  m.root = -1; m.numVerts = nv; m.numIndices = ni; m.numTris = ni / 3;
  for (uint32_t i = 0; i < ni; ++i) if (idx[i] >= nv) { setError("rtggx_set_mesh: index %u out of range (%u vertices)", idx[i], nv); m.numVerts = m.numIndices = m.numTris = 0; return -1; }
  if (nv && ni) {
    RT_HIP(alloc(m.vertsOwn[0], 6 * (size_t)nv));
    m.verts = m.vertsOwn[0]; for (auto& b : m.vertsBuf) b = m.verts;      // static until rtggx_refit_as: one allocation for all input sets
    RT_HIP(alloc(m.indices, (size_t)ni));
    RT_HIP(hipMemcpy(m.verts, verts, sizeof(float) * 6 * (size_t)nv, hipMemcpyHostToDevice));
    RT_HIP(hipMemcpy(m.indices, idx, sizeof(uint32_t) * (size_t)ni, hipMemcpyHostToDevice));
    for (int k = 0; k < 3; ++k) { m.bmin[k] = 3.4e38f; m.bmax[k] = -3.4e38f; }
    for (uint32_t v = 0; v < nv; ++v) for (int k = 0; k < 3; ++k) { const float x = verts[6 * (size_t)v + k]; if (x < m.bmin[k]) m.bmin[k] = x; if (x > m.bmax[k]) m.bmax[k] = x; }
    RT_HIP(alloc(m.fatOwn[0], 5 * (size_t)m.numTris));
    m.fat = m.fatOwn[0]; for (auto& b : m.fatBuf) b = m.fat;
    { const int r = buildFatTris(c, slot, 0, c->streamMain); if (r) return r; }
    RT_HIP(hipStreamSynchronize(c->streamMain));
  }
  c->asBuilt = false;
  return 0;
}

const float kGroundVerts[24][6] = {   // RayTracer::createGroundMesh, RayTracer.cpp:430-461
  {-1, 1, -1, 0, 1, 0}, {1, 1, -1, 0, 1, 0}, {1, 1, 1, 0, 1, 0}, {-1, 1, 1, 0, 1, 0},
  {-1, -1, -1, 0, -1, 0}, {1, -1, -1, 0, -1, 0}, {1, -1, 1, 0, -1, 0}, {-1, -1, 1, 0, -1, 0},
  {-1, -1, 1, -1, 0, 0}, {-1, -1, -1, -1, 0, 0}, {-1, 1, -1, -1, 0, 0}, {-1, 1, 1, -1, 0, 0},
  {1, -1, 1, 1, 0, 0}, {1, -1, -1, 1, 0, 0}, {1, 1, -1, 1, 0, 0}, {1, 1, 1, 1, 0, 0},
  {-1, -1, -1, 0, 0, -1}, {1, -1, -1, 0, 0, -1}, {1, 1, -1, 0, 0, -1}, {-1, 1, -1, 0, 0, -1},
  {-1, -1, 1, 0, 0, 1}, {1, -1, 1, 0, 0, 1}, {1, 1, 1, 0, 0, 1}, {-1, 1, 1, 0, 0, 1}};
const uint32_t kGroundIdx[36] = {3, 1, 0, 2, 1, 3, 6, 4, 5, 7, 4, 6, 11, 9, 8, 10, 9, 11,   // :477-496
                                        14, 12, 13, 15, 12, 14, 19, 17, 16, 18, 17, 19, 22, 20, 21, 23, 20, 22};

// Issued by rtggx_render_visibility once the new input set is selected and fenced: bring the set's vertex buffer up to date and
// refit -- everything on stream R; *touched: stream R was given work the visibility pass and the traversal must follow (evRefit, recorded
// HERE, right behind the refit).  A rebuild beside the frames gets its next launches only after that and after the visibility pass
// (issueRebuildSteps): they read the snapshot and write the job's own topology, nobody waits for them, and they must not sit between a
// frame's refit and what waits for it (round 3 issued them in front: while a rebuild was in progress every frame stalled behind 16
// build launches, the single-workgroup plocFinal among them).
int issuePendingRefits(rtggx_context* c, bool* touched) {
  *touched = false;
  const hipStream_t s = c->asyncCompute ? c->streamRefit : c->streamMain;
  bool swapped[RTGGX_NUM_MESH] = {};
  for (uint32_t slot = 0; slot < RTGGX_NUM_MESH; ++slot) {
    MeshDev& m = c->mesh[slot];
    if (!m.deforming) continue;
    // has a rebuild whose launches are all out ended?  then this frame's refit is the first on the new topology
    { const int r = continueRebuild(c, slot, s, 0u, &swapped[slot]); if (r) return r; }
    const size_t bytes = sizeof(float) * 6 * (size_t)m.numVerts;
    const uint32_t set = c->setIndex;
    bool refit = true;
    if (m.pendingStage >= 0) {
      RT_HIP(hipMemcpyAsync(m.vertsBuf[set], m.stage[m.pendingStage], bytes, hipMemcpyHostToDevice, s));
      m.pendingStage = -1; ++m.version;
    } else if (m.pendingDeviceStage >= 0) {      // rtggx_refit_as_device: staged on this stream already
      RT_HIP(hipMemcpyAsync(m.vertsBuf[set], m.deviceStage[m.pendingDeviceStage], bytes, hipMemcpyDeviceToDevice, s));
      m.pendingDeviceStage = -1; ++m.version;
    } else if (m.vertsVersion[set] != m.version) {      // no new shape this frame: this set still holds an older one
      RT_HIP(hipMemcpyAsync(m.vertsBuf[set], m.vertsBuf[m.latestSet], bytes, hipMemcpyDeviceToDevice, s));
    } else refit = false;
    if (refit) {
      m.vertsVersion[set] = m.version; m.latestSet = set;
      const int r = refitLbvh(c, slot, set, s);           // this set's leaf triangles and nodes from this set's vertices
      if (r) return r;
      *touched = true;
    }
  }
  if (*touched && c->asyncCompute) RT_HIP(hipEventRecord(c->evRefit, s));
  for (uint32_t slot = 0; slot < RTGGX_NUM_MESH; ++slot) {
    MeshDev& m = c->mesh[slot];
    if (!m.deforming) continue;
    if (m.wantRebuild && !swapped[slot]) {      // (the cost that asked for it was the old topology's)
      const int r = startRebuild(c, slot, m.latestSet);
      if (r < 0) return r;
      if (r == 1) m.wantRebuild = false;
    } else if (swapped[slot]) m.wantRebuild = false;
  }
  return 0;
}
// ... and, once the frame's visibility pass (which follows the refit on the same stream where launches are full-size) is out as well:
// the next launches of a rebuild in progress (the first ones of one just started: the copy of the vertices it starts from).
int issueRebuildSteps(rtggx_context* c) {
  const hipStream_t s = c->asyncCompute ? c->streamRefit : c->streamMain;
  for (uint32_t slot = 0; slot < RTGGX_NUM_MESH; ++slot) {
    if (!c->mesh[slot].deforming) continue;
    bool sw = false;
    const int r = continueRebuild(c, slot, s, c->rebuildSteps, &sw);
    if (r) return r;
  }
  return 0;
}
}  // namespace rt
using namespace rt;

extern "C" {
int rtggx_set_mesh(rtggx_context* c, uint32_t slot, const float* verts, uint32_t nv, const uint32_t* idx, uint32_t ni) {
  RT_CHECK_CTX(c);
  if (slot >= RTGGX_NUM_MESH || !verts || !idx || ni % 3 != 0) { setError("rtggx_set_mesh: bad arguments"); return -1; }
  return setMeshImpl(c, slot, verts, nv, idx, ni);
}

int rtggx_build_as(rtggx_context* c) {
  RT_CHECK_CTX(c);
  RT_HIP(syncStreams(c));
  // (a mesh that deforms keeps its per-set vertex buffers: it is built from its newest shape, and every input set gets the tree of
  // that set's own vertices -- lbvh.hip buildLbvh; a rebuild in progress beside the frames is dropped)
  for (uint32_t i = 0; i < 2; ++i) { abandonRebuild(c, i); c->mesh[i].wantRebuild = false; const int r = buildLbvh(c, i, c->streamAS); if (r) return r; }
  c->selectSet(c->setIndex);
  c->asBuilt = true;
  return 0;
}

// Deforming meshes (the sample itself only turns a rigid instance, RayTracer.cpp:326-341): new vertices for an
// unchanged topology.  The call only STAGES them (one copy into pinned memory); the upload and the refit of the acceleration
// structure are issued by the next rtggx_render_visibility on stream R -- behind the previous frame's traversal, beside that
// frame's shading and denoising on the main stream -- without a synchronisation.  The topology stays the one the last build
// chose; when the tree's cost has grown by RT_REFIT_REBUILD_RATIO since that build, the mesh is REBUILT beside the frames (round 3;
// lbvh.hip startRebuild: a few launches per frame behind the frame's refit, the new topology swapped in between two frames).  This call
// never waits for the GPU -- except the first one for a mesh, which allocates the per-set buffers.
struct PerSetTree { DevBuf<BvhTri> tris[RT_SETS]; DevBuf<BvhNode> nodes[RT_SETS]; DevBuf<Bvh4Node> nodes4[RT_SETS], top[RT_SETS]; };
static int splitBvhPerSet(rtggx_context* c, uint32_t slot, PerSetTree& out);
// The first new shape of a mesh: one vertex buffer per input set (rtggx_context.h), the staging ring, the tree arrays per set, the second
// topology and scratch memory of a rebuild beside the frames -- the one place where a refit call waits for the GPU.
static int beginDeforming(rtggx_context* c, uint32_t slot) {
  MeshDev& m = c->mesh[slot];
  if (m.deforming) return 0;
  const size_t bytes = sizeof(float) * 6 * (size_t)m.numVerts;
  RT_HIP(syncStreams(c));
  // Everything into locals first -- the copies of the vertices and of the tree, the staging ring --, then all of it into the mesh at once:
  // a failure on the way leaves the mesh static, with one allocation per array as before.
  DevBuf<float> nv2[RT_SETS]; DevBuf<float4> nf[RT_SETS]; PinnedBuf<float> st[RT_SLOTS];
  const size_t fb = sizeof(float4) * 5 * (size_t)m.numTris;
  bool ok = true;
  for (int i = 1; i < RT_SETS && ok; ++i) ok = alloc(nv2[i], 6 * (size_t)m.numVerts) == hipSuccess && alloc(nf[i], 5 * (size_t)m.numTris) == hipSuccess;
  for (int i = 0; i < RT_SLOTS && ok; ++i) ok = alloc(st[i], 6 * (size_t)m.numVerts) == hipSuccess;
  if (!ok) { setError("rtggx_refit_as: out of memory for the per-set vertex buffers of mesh %u", slot); return -2; }
  for (int i = 1; i < RT_SETS; ++i) { RT_HIP(hipMemcpy(nv2[i], m.vertsBuf[0], bytes, hipMemcpyDeviceToDevice)); RT_HIP(hipMemcpy(nf[i], m.fatBuf[0], fb, hipMemcpyDeviceToDevice)); }
  PerSetTree tree;
  { const int r = splitBvhPerSet(c, slot, tree); if (r) return r; }
  { const int r = prepareRebuild(c, slot); if (r) return r; }      // the second topology and the build's scratch memory: not in the frame loop (complete or absent; a later attempt finds it)
  // A device-to-device hipMemcpy does NOT wait on the host (only its issue is synchronous) and runs on the null stream, which the
  // non-blocking streams of this context are not ordered against: the next frame's refit on stream R wrote a set's nodes while the copy
  // of the OLD nodes into the same array was still on its way, and the copy landed last (found once GPU_MAX_HW_QUEUES=8 gave the null
  // stream a hardware queue of its own: test_deforming_mesh_async_refit_against_the_oracle, "child box must contain the child").
  RT_HIP(hipStreamSynchronize(nullptr));
  for (int i = 1; i < RT_SETS; ++i) {
    m.vertsOwn[i] = std::move(nv2[i]); m.vertsBuf[i] = m.vertsOwn[i]; m.fatOwn[i] = std::move(nf[i]); m.fatBuf[i] = m.fatOwn[i];
    if (!tree.tris[i]) continue;      // (no tree yet, or one per set already)
    m.trisOwn[i] = std::move(tree.tris[i]); m.trisBuf[i] = m.trisOwn[i]; m.nodesOwn[i] = std::move(tree.nodes[i]); m.nodesBuf[i] = m.nodesOwn[i];
    m.nodes4Own[i] = std::move(tree.nodes4[i]); m.nodes4Buf[i] = m.nodes4Own[i]; m.topOwn[i] = std::move(tree.top[i]); m.topBuf[i] = m.topOwn[i];
    m.topCountBuf[i] = m.topCountBuf[0];
  }
  for (int i = 0; i < RT_SLOTS; ++i) m.stage[i] = std::move(st[i]);
  m.deforming = true; m.latestSet = c->setIndex;
  c->selectSet(c->setIndex);
  return 0;
}
static int checkRefit(rtggx_context* c, uint32_t slot, const void* verts, uint32_t nv, const char* who) {
  if (slot >= RTGGX_NUM_MESH || !verts) { setError("%s: bad arguments", who); return -1; }
  const MeshDev& m = c->mesh[slot];
  if (!c->asBuilt || !m.tris) { setError("%s: rtggx_build_as has not been called", who); return -1; }
  if (nv != m.numVerts) { setError("%s: %u vertices given, the mesh has %u (a new topology needs rtggx_set_mesh + rtggx_build_as)", who, nv, m.numVerts); return -1; }
  return 0;
}
// the cost of the tree after an earlier refit has arrived: has the shape drifted too far from the one the topology was built for?
static void pollTreeCost(rtggx_context* c, MeshDev& m) {
  if (m.costInFlight && hipEventQuery(m.evCost) == hipSuccess) { m.lastCost = *m.hCost; m.costInFlight = false; }
  // (a build of cost 0 -- every box without area: a mesh that starts collapsed onto an axis-aligned line or into a point -- is outgrown by any cost above 0)
  if (m.lastCost > c->rebuildRatio * m.builtCost) m.wantRebuild = true;      // started by the next frame (issuePendingRefits)
}
int rtggx_refit_as(rtggx_context* c, uint32_t slot, const float* verts, uint32_t nv) {
  RT_CHECK_CTX(c);
  { const int r = checkRefit(c, slot, verts, nv, "rtggx_refit_as"); if (r) return r; }
  { const int r = beginDeforming(c, slot); if (r) return r; }
  MeshDev& m = c->mesh[slot];
  pollTreeCost(c, m);
  // A shape that no frame has picked up yet (two calls between frames, calls without frames) is simply replaced: its staging buffer has
  // no copy in flight.  Otherwise the next buffer of the ring: it was last consumed RT_SLOTS frames ago, and the copy that read it was
  // ordered before a traversal whose frame the host has since waited for (the set fence of rtggx_render_visibility).
  uint32_t st;
  if (m.pendingStage >= 0) st = (uint32_t)m.pendingStage;
  else { st = m.stageNext; m.stageNext = (m.stageNext + 1u) % RT_SLOTS; }
  memcpy(m.stage[st], verts, sizeof(float) * 6 * (size_t)nv);
  m.pendingStage = (int)st; m.pendingDeviceStage = -1;      // (the newest shape wins)
  return 0;
}
// The same for a mesh that is animated ON the GPU (round 4): `dverts` is a device pointer, `stream` the stream that
// produces it (null: the null stream).  Like a hipMemcpyAsync on that stream: the copy out of `dverts` is ordered behind everything the
// stream holds at the time of the call, and what the caller gives the stream afterwards -- the next animation step, overwriting `dverts` --
// behind the copy.  It runs on the context's geometry stream, into a device-side staging ring the next frame's refit reads: no host copy
// (836 KB and 17 us per frame for the bunny through rtggx_refit_as), no wait.
int rtggx_refit_as_device(rtggx_context* c, uint32_t slot, const float* dverts, uint32_t nv, void* stream) {
  RT_CHECK_CTX(c);
  { const int r = checkRefit(c, slot, dverts, nv, "rtggx_refit_as_device"); if (r) return r; }
  { const int r = beginDeforming(c, slot); if (r) return r; }
  MeshDev& m = c->mesh[slot];
  const size_t bytes = sizeof(float) * 6 * (size_t)nv;
  if (!m.deviceStage[0]) {      // the staging ring and its two events: all of them, or nothing half-done is left behind
    DevBuf<float> st[RT_SLOTS]; Event produced, staged;
    bool ok = true;
    for (int i = 0; i < RT_SLOTS && ok; ++i) ok = alloc(st[i], 6 * (size_t)nv) == hipSuccess;
    ok = ok && create(produced, hipEventDisableTiming) == hipSuccess && create(staged, hipEventDisableTiming) == hipSuccess;
    if (!ok) { setError("rtggx_refit_as_device: out of memory for the staging ring of mesh %u", slot); return -2; }
    for (int i = 0; i < RT_SLOTS; ++i) m.deviceStage[i] = std::move(st[i]);
    m.evProduced = std::move(produced); m.evStaged = std::move(staged);
  }
  pollTreeCost(c, m);
  const hipStream_t s = c->asyncCompute ? c->streamRefit : c->streamMain, producer = (hipStream_t)stream;
  const uint32_t k = m.deviceStageNext; m.deviceStageNext = (m.deviceStageNext + 1u) % RT_SLOTS;      // (copies into the ring follow each other and their readers on one stream)
  if (producer != s) { RT_HIP(hipEventRecord(m.evProduced, producer)); RT_HIP(hipStreamWaitEvent(s, m.evProduced, 0)); }
  RT_HIP(hipMemcpyAsync(m.deviceStage[k], dverts, bytes, hipMemcpyDeviceToDevice, s));
  if (producer != s) { RT_HIP(hipEventRecord(m.evStaged, s)); RT_HIP(hipStreamWaitEvent(producer, m.evStaged, 0)); }
  m.pendingDeviceStage = (int)k; m.pendingStage = -1;
  return 0;
}
int rtggx_set_refit_policy(rtggx_context* c, float rebuildRatio, uint32_t stepsPerFrame) {
  RT_CHECK_CTX(c);
  if (!(rebuildRatio > 1.0f) || stepsPerFrame == 0u) { setError("rtggx_set_refit_policy: a ratio above 1 and at least one step per frame"); return -1; }
  c->rebuildRatio = rebuildRatio; c->rebuildSteps = stepsPerFrame;
  return 0;
}
int rtggx_refit_stats(rtggx_context* c, uint32_t slot, float* costRatio, uint32_t* refits, uint32_t* rebuilds) {
  RT_CHECK_CTX(c);
  if (slot >= RTGGX_NUM_MESH) { setError("rtggx_refit_stats: bad mesh"); return -1; }
  MeshDev& m = c->mesh[slot];
  RT_HIP(syncStreams(c));
  if (m.costInFlight) { m.lastCost = *m.hCost; m.costInFlight = false; }
  if (costRatio) *costRatio = m.builtCost > 0.0f ? m.lastCost / m.builtCost : m.lastCost > 0.0f ? __builtin_inff() : 1.0f;      // (0 / 0: one triangle, or still collapsed)
  if (refits) *refits = m.refits;
  if (rebuilds) *rebuilds = m.rebuilds;
  return 0;
}

// The boxes and leaf triangles of a deforming mesh once per input set (rtggx_context.h): copies of the tree just built, into `out`
// (beginDeforming installs them with everything else).
static int splitBvhPerSet(rtggx_context* c, uint32_t slot, PerSetTree& out) {
  MeshDev& m = c->mesh[slot];
  const size_t n = m.numTris, nn = n > 1 ? n - 1 : 1, topCap = slot == 0 ? RT_TOP_SLOT0 : RT_TOP_SLOT1;
  for (int i = 1; i < RT_SETS; ++i) {
    if (m.trisBuf[i] != m.trisBuf[0]) continue;
    RT_HIP(alloc(out.tris[i], n)); RT_HIP(hipMemcpy(out.tris[i], m.trisBuf[0], sizeof(BvhTri) * n, hipMemcpyDeviceToDevice));
    RT_HIP(alloc(out.nodes[i], nn)); RT_HIP(hipMemcpy(out.nodes[i], m.nodesBuf[0], sizeof(BvhNode) * nn, hipMemcpyDeviceToDevice));
    RT_HIP(alloc(out.nodes4[i], nn)); RT_HIP(hipMemcpy(out.nodes4[i], m.nodes4Buf[0], sizeof(Bvh4Node) * nn, hipMemcpyDeviceToDevice));
    RT_HIP(alloc(out.top[i], topCap)); RT_HIP(hipMemcpy(out.top[i], m.topBuf[0], sizeof(Bvh4Node) * topCap, hipMemcpyDeviceToDevice));
  }
  return 0;
}

}  // extern "C"
