// Ray-tracing pass: the gfx950 replacement of DispatchRays(W,H,1) over RayTracing.cso
// (RayTracer::rayTrace, RayTracedGGX/Content/RayTracer.cpp:793-810).  The four DXR shaders of
// RayTracedGGX/Content/Shaders/RayTracing.hlsl become three kernels around a ray queue (and, since, the variants and passes listed below):
//
//   rayGenKernel   raygenMain :541-565 up to the TraceRay calls: G-buffer reconstruction from the
//                  visibility buffer (getPrimarySurface :277-333), GGX / uniform-sphere sampling
//                  (:92-162, :394-406), BRDF weight (:459-480).  Pixels whose ray is degenerate
//                  (background, NoL <= 0) are finished here (missMain :620-625 / zero); every real
//                  ray is compacted, by wave ballot, into the bin of the wave's own 8x8-pixel sub-tile
//                  (rt_queue.h: no atomics).
//   traceKernel    TraceRay :183-198 (trace.hip): one wave per bin over a two-level software BVH -- the ray
//                  is carried into each instance's object space (TLAS = two world->object matrices) and
//                  walks the 4-wide collapse of the Morton-ordered PLOC tree with a per-lane stack in LDS,
//                  nearer child first, lanes sharing work inside the wave.  Ray/triangle: watertight test
//                  (Woop, Benthin, Wald 2013), no culling, TMin < t < TMax, ties to the lower
//                  (instance, primitive).
//   shadeKernel    closestHitReflection :571-590, closestHitDiffuse :593-614, missMain :620-625 and
//                  the tail of computeReflection / computeDiffuse, with Material.hlsli,
//                  BRDFModels.hlsli, SHIrradianceTypeless.hlsli:16-37; writes RayTracingOut0/1.
//
// Beside them here: sampleParamsKernel / sampleGenKernel / resolveSamplesKernel (N samples per pixel), reconstructKernel (quarter rate),
// accumulateKernel / presentAccumulationKernel, envPrefilterKernel, and the test entries (fillTestQueue, exportTestHits, exportOcclusion,
// debugEnvironmentKernel).  Direct lighting -- the sun, the local lights, both at the surfaces the paths hit -- is lighting.hip; launchShade
// calls its hit passes in front of every level's shading pass.  What both files' kernels call (Material.hlsli, BRDF terms, rng, triangle and
// attribute helpers) is rt_surface.h.
//
// rayGenKernel and traceKernel run on stream B, shadeKernel on the main stream one frame behind (frame.hip).
// Roofline: HBM by decree of the metric (no MFMA work exists here).  Algorithmic bytes:
// rayGen 18 B/pixel (+64 B per queued ray); trace 64 B ray + 16 B hit per ray + the scene arrays
// once; shade 64+16 B in, 4 B out per ray.  The BVH (<= 14 MB) is L2/MALL resident, so traversal is
// bound by L1 request rate, issue and latency, not by HBM (DESIGN.md "Roofline").
#include <cstring>
#include <type_traits>
#include "rt_queue.h"
#include "rt_traverse.h"
#include "rt_surface.h"

namespace rt {


// ---- environment (RayTracing.hlsl:167-180; D3D cube sampling restated) --------------
struct EnvRef { const uint2* __restrict__ texels; uint32_t size, mips; const uint32_t* __restrict__ mipOffset; };

RT_DEV void cubeFaceUV(f3 d, int& face, float& u, float& v) {
  const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
  if (ax >= ay && ax >= az) { face = d.x >= 0.0f ? 0 : 1; u = (d.x >= 0.0f ? -d.z : d.z) / ax; v = -d.y / ax; }
  else if (ay >= az) { face = d.y >= 0.0f ? 2 : 3; u = d.x / ay; v = (d.y >= 0.0f ? d.z : -d.z) / ay; }
  else { face = d.z >= 0.0f ? 4 : 5; u = (d.z >= 0.0f ? d.x : -d.x) / az; v = -d.y / az; }
}
RT_DEV f3 cubeFaceDir(int face, float u, float v) {
  switch (face) {
    case 0: return mk3(1.0f, -v, -u);
    case 1: return mk3(-1.0f, -v, u);
    case 2: return mk3(u, 1.0f, v);
    case 3: return mk3(u, -1.0f, -v);
    case 4: return mk3(u, -v, 1.0f);
    default: return mk3(-u, -v, -1.0f);
  }
}
// MIP0: the level is known to be 0 where it is called (the sky behind a pixel, a ray that misses): its texels start at offset 0, and
// the offset table -- one more dependent fetch in front of every texel -- is not read.
template <bool MIP0 = false>
RT_DEV f3 cubeTexel(const EnvRef& e, uint32_t mip, int face, int x, int y) {
  const int s = (int)((e.size >> mip) ? (e.size >> mip) : 1u);
  if (x < 0 || y < 0 || x >= s || y >= s) {
    const float u = ((float)x + 0.5f) / (float)s * 2.0f - 1.0f, v = ((float)y + 0.5f) / (float)s * 2.0f - 1.0f;
    float uu, vv; cubeFaceUV(cubeFaceDir(face, u, v), face, uu, vv);
    x = (int)floorf((uu * 0.5f + 0.5f) * (float)s); y = (int)floorf((vv * 0.5f + 0.5f) * (float)s);
    x = min(max(x, 0), s - 1); y = min(max(y, 0), s - 1);
  }
  const uint2 t = e.texels[(MIP0 ? 0u : e.mipOffset[mip]) + (uint32_t)face * (uint32_t)(s * s) + (uint32_t)(y * s + x)];
  return mk3(f16ToF32(t.x & 0xFFFFu), f16ToF32(t.x >> 16), f16ToF32(t.y & 0xFFFFu));
}
template <bool MIP0 = false>
RT_DEV f3 cubeBilinear(const EnvRef& e, uint32_t mip, int face, float u, float v) {
  const int s = (int)((e.size >> mip) ? (e.size >> mip) : 1u);
  const float x = (u * 0.5f + 0.5f) * (float)s - 0.5f, y = (v * 0.5f + 0.5f) * (float)s - 0.5f;
  const float x0 = floorf(x), y0 = floorf(y);
  const float fx = x - x0, fy = y - y0;
  const int ix = (int)x0, iy = (int)y0;
  const float w00 = (1.0f - fx) * (1.0f - fy), w10 = fx * (1.0f - fy), w01 = (1.0f - fx) * fy, w11 = fx * fy;
  const f3 c00 = cubeTexel<MIP0>(e, mip, face, ix, iy), c10 = cubeTexel<MIP0>(e, mip, face, ix + 1, iy);
  const f3 c01 = cubeTexel<MIP0>(e, mip, face, ix, iy + 1), c11 = cubeTexel<MIP0>(e, mip, face, ix + 1, iy + 1);
  return ((c00 * w00 + c10 * w10) + c01 * w01) + c11 * w11;
}
// environment(e, dir, 0): RayTracing.hlsl:620-625 (missMain) and the sky behind a pixel -- the same arithmetic with the level's constants folded
RT_DEV f3 environmentLevel0(const EnvRef& e, f3 dir) {
  int face; float u, v; cubeFaceUV(dir, face, u, v);
  return cubeBilinear<true>(e, 0u, face, u, v);
}
__device__ __noinline__ f3 environment(EnvRef e, f3 dir, float level) {
  int face; float u, v; cubeFaceUV(dir, face, u, v);
  const float maxLevel = (float)(e.mips - 1);
  const float l = fminf(fmaxf(level, 0.0f), maxLevel);
  const float l0 = floorf(l), fl = l - l0;
  const uint32_t m0 = (uint32_t)l0, m1 = min(m0 + 1, e.mips - 1);
  const f3 a = cubeBilinear(e, m0, face, u, v);
  if (fl == 0.0f) return a;
  const f3 b = cubeBilinear(e, m1, face, u, v);
  return a * (1.0f - fl) + b * fl;
}

// ---- SHIrradianceTypeless.hlsli:16-37 ------------------------------------------------------------------
RT_DEV f3 evaluateSHIrradiance(const float* __restrict__ sh, f3 norm) {
  const float c1 = 0.42904276540489171563379376569857f, c2 = 0.51166335397324424423977581244463f;
  const float c3 = 0.24770795610037568833406429782001f, c4 = 0.88622692545275801364908374167057f;
  const float x = -norm.x, y = -norm.y, z = norm.z;
#define SHL(i) mk3(sh[3 * (i)], sh[3 * (i) + 1], sh[3 * (i) + 2])
  f3 irr = (c1 * (x * x - y * y)) * SHL(8);
  irr = irr + (c3 * (3.0f * z * z - 1.0f)) * SHL(6);
  irr = irr + c4 * SHL(0);
  irr = irr + (2.0f * c1) * ((SHL(4) * x * y + SHL(7) * x * z) + SHL(5) * y * z);
  irr = irr + (2.0f * c2) * ((SHL(3) * x + SHL(1) * y) + SHL(2) * z);
#undef SHL
  return mk3(fmaxf(0.0f, irr.x), fmaxf(0.0f, irr.y), fmaxf(0.0f, irr.z));
}

// ---- RayTracing.hlsl helpers ---------------------------------------------------------------------------
RT_DEV float calcMipFromRoughness(float rgh, float mipCount) {   // :416-422
  const float level = 3.0f - 1.15f * log2Contract(rgh);
  return mipCount - 1.0f - level;
}
RT_DEV f3 localToWorld(f3 n, f3 l) {   // :129-147
  const f3 up = fabsf(n.y) < 0.999f ? mk3(0.0f, 1.0f, 0.0f) : mk3(1.0f, 0.0f, 0.0f);
  const f3 xAxis = normalize3(cross3(up, n));
  const f3 yAxis = cross3(n, xAxis);
  return (xAxis * l.x + yAxis * l.y) + n * l.z;
}
// Opt-in sampler (rtggx_set_sampler; north_star: "GGX-VNDF importance sampling in the hit path"): the half vector from the distribution of
// VISIBLE normals (Heitz 2018, "Sampling the GGX Distribution of Visible Normals", listing 1; isotropic, alpha = roughness^2 as in
// computeLocalDirectionGGX), in the tangent frame of localToWorld.  The reference samples the plain GGX NDF (RayTracing.hlsl:92-101,
// 424-484): that stays the default and the parity path; this one has its own oracle counterpart (orc_raytrace.h vndf_half_vector).
RT_DEV f3 vndfHalfVector(f3 n, f3 v, float alpha, float cosPhi, float sinPhi, float u) {
  const f3 up = fabsf(n.y) < 0.999f ? mk3(0.0f, 1.0f, 0.0f) : mk3(1.0f, 0.0f, 0.0f);
  const f3 xAxis = normalize3(cross3(up, n));
  const f3 yAxis = cross3(n, xAxis);
  const f3 ve = mk3(dot3(v, xAxis), dot3(v, yAxis), dot3(v, n));
  const f3 vh = normalize3(mk3(alpha * ve.x, alpha * ve.y, ve.z));
  const float lensq = vh.x * vh.x + vh.y * vh.y;
  const f3 t1v = lensq > 0.0f ? mk3(-vh.y, vh.x, 0.0f) * (1.0f / sqrtf(lensq)) : mk3(1.0f, 0.0f, 0.0f);
  const f3 t2v = cross3(vh, t1v);
  const float r = sqrtf(u);
  const float t1 = r * cosPhi;
  float t2 = r * sinPhi;
  const float sw = 0.5f * (1.0f + vh.z);
  t2 = (1.0f - sw) * sqrtf(1.0f - t1 * t1) + sw * t2;
  const f3 nh = (t1 * t1v + t2 * t2v) + sqrtf(fmaxf(0.0f, (1.0f - t1 * t1) - t2 * t2)) * vh;
  const f3 hl = normalize3(mk3(alpha * nh.x, alpha * nh.y, fmaxf(0.0f, nh.z)));
  return (xAxis * hl.x + yAxis * hl.y) + n * hl.z;
}
// computeReflection (:424-484) at a depth that traces (the shading pass that spawns rays, shadeKernel): the same arithmetic as ray
// generation's depth-0 code -- which stays written out, so that its ISA is the one it was before recursion existed --: the half vector -- the reference's GGX NDF sample (computeDirectionGGX :92-101),
// or VNDF with rtggx_set_sampler --, and, where NoL = dot(N, reflect(-V, H)) > 0, the ray's weight (:477)
RT_DEV f3 reflectionHalfVector(bool vndf, f3 N, f3 V, float a, float cosPhi, float sinPhi, float xiY) {
  if (vndf) return vndfHalfVector(N, V, a, cosPhi, sinPhi, xiY);
  const float cosTheta = sqrtf((1.0f - xiY) / (1.0f + (a * a - 1.0f) * xiY));
  const float sinTheta = sqrtf(1.0f - cosTheta * cosTheta);
  return localToWorld(N, mk3(cosPhi * sinTheta, sinPhi * sinTheta, cosTheta));
}
RT_DEV f3 reflectionWeight(bool vndf, f3 N, f3 V, f3 Hh, float NoL, f2 rghMtl, f3 color) {
  const float a = rghMtl.x * rghMtl.x;
  const f3 f0 = mk3(lerpf(0.04f, color.x, rghMtl.y), lerpf(0.04f, color.y, rghMtl.y), lerpf(0.04f, color.z, rghMtl.y));
  const float NoV = saturatef(dot3(N, V));
  const float VoH = saturatef(dot3(V, Hh));
  const f3 F = fSchlick(f0, VoH);
  const float vis = visSmith(rghMtl.x, NoV, NoL);
  const float NoH = saturatef(dot3(N, Hh));
  const float k = 4.0f * VoH / NoH;
  f3 w = mk3(((NoL * F.x) * vis) * k, ((NoL * F.y) * vis) * k, ((NoL * F.z) * vis) * k);
  if (vndf) {      // BRDF x NoL / pdf of the visible-normal sampler = F x G2 / G1(V) = F x G1(L), with the separable Smith terms of Vis_Smith
    const float a2 = a * a;
    const float g1l = (2.0f * NoL) / (NoL + sqrtf(NoL * (NoL - NoL * a2) + a2));
    w = mk3(F.x * g1l, F.y * g1l, F.z * g1l);
  }
  return w;
}
// computeDiffuse's ray (computeDirectionCos :150-162, the uniform-sphere branch), as in ray generation
RT_DEV f3 diffuseDirection(f3 N, float cosPhi, float sinPhi, float xiY) {
  const float cosTheta = 1.0f - 2.0f * xiY;
  const float sinTheta = sqrtf(1.0f - cosTheta * cosTheta);
  return normalize3(N + mk3(cosPhi * sinTheta, sinPhi * sinTheta, cosTheta));
}

// =========================================================================================================
// Kernel 1: ray generation
// =========================================================================================================
struct GenArgs {
  const unsigned long long* visDepth; uint32_t* depthOut;
  // the head of the NEXT frame's visibility pass (visibility.hip): its target is cleared and its lists are emptied here, on the way
  // (visNext == null: not).  One kernel launch per frame less, and the clear's 8 bytes per pixel ride on a kernel that is there anyway.
  // (Tried with it and not kept: merging the queued large triangles -- rasterLarge's work -- here as well.  Same arithmetic, but in
  // front of every wave's first dependent fetch: rayGenKernel 85 -> 169 us per launch, the 1080p frame 0.190 -> 0.243 ms, 4K 0.715 ->
  // 0.980; with the records in LDS no different.  profiles/r03_b_visibility_merge.txt)
  unsigned long long* visNext; uint32_t* zeroNext0; uint32_t* zeroNext1;
  // one word per tile of this kernel (rtggx_context.h VisTarget::dirty): 0 = the tile of the target holds the clear value only.  visDirty: of the
  // target read here; visDirtyNext: of visNext; where the words are not known both point at words that are all ones (read / clear every
  // tile).  The words of visNext's tiles end as 0 (visDirtyNextOut: the target's own words)
  const uint32_t* visDirty; const uint32_t* visDirtyNext; uint32_t* visDirtyNextOut;
  // still sky (rtggx_context.h InputSet::skyRun, RT_SKY_PREV_RUN): the previous set's run words, this set's, the epoch (24 bits) they count
  // under, and the previous run from which a tile without a surface is left alone (above RT_SKY_RUN_CAP: never)
  const uint32_t* skyPrev; uint32_t* skyOut; uint32_t skyEpoch, skyPrevRun;
  uint32_t* normalOut; uint16_t* roughMetalOut; uint32_t* velocityOut; uint32_t* reflOut; uint32_t* diffOut;
  const uint16_t* roughMetalPrev;   // the previous frame's input set = what this target held before this frame
  const uint32_t* diffPrev;         // likewise RayTracingOut1, or null: the hit shading carries it over (launchShade)
  const float4* fat0; const float4* fat1;
  const uint2* env; const uint32_t* envMipOffset; uint32_t envSize, envMips;
  const float* cosSin;
  RayRec* rays; HitKey* hits; uint32_t* binCount; uint32_t binSlots;      // slots per bin (rt_queue.h)
  uint32_t* frameRays;      // 256 per-frame ray counters, zeroed here, added to by the trace kernel
  uint32_t tilesX, numTiles, rowBegin, rowEnd;
  // adaptive split (trace.hip): null / 0 when off
  uint32_t* binWork; uint32_t* splitList; uint32_t* splitCount; uint32_t splitWork, frontWork, splitMaxShift, splitCap;
};

// Sample-set size M > 256 (rtggx_set_sample_set; DESIGN.md "Sample-set size"): getSampleParam with numSamples = M.  The slot is the low bits
// of the same word (M is a power of two: % M), xi.y the same hash of the slot, and the table -- handed over in the kernels' cosSin pointer --
// holds M interleaved {cos, sin} pairs: one 8-byte load per lane (two 4-byte loads half a table apart would each take a cache line of
// their own per lane at 65536 entries).  The mask is the frame constants' (uniform): every sample's copy carries it (sampleParamsKernel).
// WIDE = false is the code of the 256-member set as it was, the kernels' bodies unchanged (profiles/r10_a_sampleset_isa.txt).
RT_DEV void sampleParamWide(const FrameParams& fp, const float* table, uint32_t pixel, float& xiY, float& cosPhi, float& sinPhi) {
  uint32_t s = rng(pixel); s += fp.g.FrameIndex; s = rng(s); s &= fp.sampleMask;
  xiY = (float)(rng(s) & 0xffffu) / 65536.0f;
  const float2 cs = reinterpret_cast<const float2*>(table)[s];
  cosPhi = cs.x; sinPhi = cs.y;
}
#ifndef RT_GEN_MIN_BLOCKS
#define RT_GEN_MIN_BLOCKS 1
#endif
// Quarter-rate tracing (rtggx_set_ray_rate(ctx, 4); DESIGN.md "Quarter-rate tracing"): with F = FrameIndex & 3 a frame traces the pixel
// o = {(0,0), (1,1), (1,0), (0,1)}[F] of every 2x2 quad, so that four consecutive frames trace every pixel once.
RT_DEV bool quadTraced(uint32_t px, uint32_t py, uint32_t frameIndex) {
  const uint32_t f = frameIndex & 3u;
  return (px & 1u) == ((0x6u >> f) & 1u) && (py & 1u) == ((0xAu >> f) & 1u);
}
// Rate 4: the workgroup's rays into its one bin, reflection rays first, then diffuse rays, each in wave order; the adaptive split's
// decision (rayGenKernel) once per bin.  At most 64 reflection rays (one per quad) and 64 diffuse rays: the bin's slots as at rate 1.
RT_DEV void rayGenQuadBin(const GenArgs& A, bool wantRefl, bool wantDiff, const RayRec& rr, const RayRec& rd) {
  __shared__ uint32_t waveRays[2][4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u, bin = blockIdx.x;
  const unsigned long long maskR = __ballot(wantRefl), maskD = __ballot(wantDiff), below = (1ull << lane) - 1ull;
  if (lane == 0) { waveRays[0][wave] = (uint32_t)__popcll(maskR); waveRays[1][wave] = (uint32_t)__popcll(maskD); }
  __syncthreads();
  uint32_t baseR = 0u, baseD = 0u, nR = 0u, nD = 0u;
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint32_t r = waveRays[0][k], d = waveRays[1][k];
    if (k < wave) { baseR += r; baseD += d; }
    nR += r; nD += d;
  }
  RayRec* dst = A.rays + (size_t)bin * A.binSlots;
  HitKey* keys = A.hits + (size_t)bin * A.binSlots;
  if (wantRefl) { const uint32_t k = baseR + (uint32_t)__popcll(maskR & below); dst[k] = rr; keys[k] = hitKey(RT_RAY_TMAX, 0xFFFFFFFFu); }
  const uint32_t kD = nR + baseD + (uint32_t)__popcll(maskD & below);
  if (wantDiff && kD < A.binSlots) { dst[kD] = rd; keys[kD] = hitKey(RT_RAY_TMAX, 0xFFFFFFFFu); }
  if (threadIdx.x != 0) return;
  const uint32_t nRaysInBin = min(nR + nD, A.binSlots);
  uint32_t mark = 0u;
  if (A.binWork != nullptr) {      // the adaptive split as in rayGenKernel<1>, for one bin
    const uint32_t w = A.binWork[bin];
    A.binWork[bin] = 0u;
    uint32_t shift = 0u;
    while (shift < A.splitMaxShift && (w >> shift) > A.splitWork) ++shift;
    const uint32_t n = (shift || w > A.frontWork) ? 1u << shift : 0u;
    if (n) {
      const uint32_t base = atomicAdd(A.splitCount, n);
      const bool fits = base + n <= A.splitCap;
      for (uint32_t k = 0; k < n && base + k < A.splitCap; ++k) A.splitList[base + k] = fits ? ((shift << 28) | (k << 24) | bin) : 0xFFFFFFFFu;
      mark = fits ? (shift << 1) | 1u : 0u;
    }
  }
  A.binCount[bin] = nRaysInBin | (mark << 8);
}
// RATE 1: every covered pixel traces (the reference's DispatchRays(W,H,1)); workgroup b <-> 16x16 tile b, its wave w <-> bin 4b + w.
// RATE 4: one pixel per quad traces, and the workgroup's (at most 64 + 64) rays go to ONE bin, compacted over its four waves through LDS,
// so that the traversal's waves stay as full as at rate 1.  Workgroup b <-> bin b; four consecutive bins are the four 16x16 tiles of a
// 32x32 tile (launchTrace gets the 32x32 grid).  A bin whose 16x16 tile lies outside the frame is written empty.
template <int RATE, bool WIDE = false>
__global__ void __launch_bounds__(256, RT_GEN_MIN_BLOCKS) rayGenKernel(const FrameParams* __restrict__ fpp, GenArgs A) {
  const FrameParams& fp = *fpp;
  if (blockIdx.x == 0) A.frameRays[threadIdx.x] = 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0 && A.visNext != nullptr) { *A.zeroNext0 = 0u; *A.zeroNext1 = 0u; }      // the next frame's large-triangle list, the next set's split list
  // 16x16 pixel tile per workgroup, 8x8 per wave: the 64 rays a wave appends are neighbours on screen
  uint32_t tile = blockIdx.x;
  if constexpr (RATE == 4) {
    const uint32_t superX = (A.tilesX + 1u) >> 1, sup = blockIdx.x >> 2;
    const uint32_t tx = (sup % superX) * 2u + (blockIdx.x & 1u), ty = (sup / superX) * 2u + ((blockIdx.x >> 1) & 1u);
    tile = ty * A.tilesX + tx;
    if (tx >= A.tilesX || tile >= A.numTiles) {      // (uniform)
      if (threadIdx.x == 0) { A.binCount[blockIdx.x] = 0u; if (A.binWork != nullptr) A.binWork[blockIdx.x] = 0u; }
      return;
    }
  }
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t px = (tile % A.tilesX) * 16 + (wave & 1u) * 8 + (lane & 7u);
  const uint32_t py = A.rowBegin + (tile / A.tilesX) * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool inside = px < fp.W && py < A.rowEnd;
  const bool traced = RATE == 1 || quadTraced(px, py, fp.g.FrameIndex);
  // (three scalar loads, one wait: as vector loads in front of the kernel's first fetch two of them cost ray generation 10 us in the frame)
  uint32_t wordHere, wordNext, skyWord;
  asm volatile("s_load_dword %0, %3, %6\n\ts_load_dword %1, %4, %6\n\ts_load_dword %2, %5, %6\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(wordHere), "=&s"(wordNext), "=&s"(skyWord) : "s"(A.visDirty), "s"(A.visDirtyNext), "s"(A.skyPrev), "s"(tile * 4u) : "memory");
  const bool drawn = wordHere != 0u;                                    // uniform over the workgroup
  const bool clearNext = A.visNext != nullptr && wordNext != 0u;
  // Still sky: the tile's run of frames without a surface under this epoch goes on or ends (a plain store from one lane; at rate 4 it
  // always ends: this path is rate 1's).  A tile whose run is long enough holds, in this set, everything the rest of this kernel would
  // store there (RT_SKY_PREV_RUN).  Not where the target two frames on wants clearing: its word is 0 wherever this tile's run can be long
  // enough (that target was drawn into RT_VIS_RING - 2 = RT_SETS frames ago), unless the words are not known -- such a tile takes the long
  // path, whose registers a second copy of that clear in here would raise by two (a wave per SIMD less).  Uniform over the workgroup.
  const uint32_t skyPrevRun = (skyWord >> 8) == A.skyEpoch ? skyWord & 0xFFu : 0u;
  const uint32_t skyWordOut = (A.skyEpoch << 8) | (drawn || RATE != 1 ? 0u : min(skyPrevRun + 1u, RT_SKY_RUN_CAP));      // (stored below, beside the other word)
  if (RATE == 1 && !drawn && !clearNext && skyPrevRun >= A.skyPrevRun) {
    if (threadIdx.x == 0) A.skyOut[tile] = skyWordOut;
    return;
  }
  const EnvRef env{A.env, A.envSize, A.envMips, A.envMipOffset};
  bool wantRefl = false, wantDiff = false;
  RayRec rr, rd;
  if (inside) {
    const uint32_t W = fp.W, H = fp.H;
    const size_t pix = (size_t)py * W + px;
    // getPrimarySurface :277-333
    const unsigned long long visWord = drawn ? A.visDepth[pix] : RT_VIS_CLEAR;
    if (clearNext) A.visNext[pix] = RT_VIS_CLEAR;
    // getSampleParam :394-406 -- of every pixel of a tile with something in it, before the visibility word is back: the table fetch then
    // travels beside that word instead of behind the triangle's
    float xiY = 0.0f, cosPhi = 0.0f, sinPhi = 0.0f;
    if constexpr (WIDE) { if (drawn) sampleParamWide(fp, A.cosSin, py * W + px, xiY, cosPhi, sinPhi); }
    else if (drawn) {
      uint32_t s = py * W + px;
      s = rng(s); s += fp.g.FrameIndex; s = rng(s); s %= 256u;
      xiY = (float)(rng(s) & 0xffffu) / 65536.0f;
      cosPhi = A.cosSin[s]; sinPhi = A.cosSin[256 + s];
    }
    uint32_t visibility = (uint32_t)visWord;
    A.depthOut[pix] = (uint32_t)(visWord >> 32);      // the filters read depth four bytes at a time instead of every other word of an 8-byte array
    f2 screenPos; screenPos.x = ((float)px + 0.5f) / (float)W * 2.0f - 1.0f; screenPos.y = ((float)py + 0.5f) / (float)H * 2.0f - 1.0f;
    screenPos.y = -screenPos.y;
    const f3 eye = mk3(fp.rg.EyePt[0], fp.rg.EyePt[1], fp.rg.EyePt[2]);
    bool hit; f3 N, V, P, color; f2 rghMtl, velocity; uint32_t inst = 0, prim = 0;
    if (visibility > 0) {
      --visibility;
      hit = true; inst = visibility >> 24; prim = visibility & 0xFFFFFFu;
      asm volatile("" : "+v"(prim));      // see shadeKernel: the mask must survive the array indexing by inst below
      const Tri3 v = getVertices(inst ? A.fat1 : A.fat0, prim);
      const M4 wvp = cbLoad4x4(fp.g.WorldViewProjs[inst]);
      f4 p[3];
      for (int k = 0; k < 3; ++k) p[k] = mulPoint(v.pos[k], wvp);
      screenPos.x -= fp.rg.ProjBias[0]; screenPos.y -= fp.rg.ProjBias[1];
      const f2 bary = calcBarycentrics(p, screenPos);
      const Attrib a = interpAttrib(v, bary.x, bary.y);
      color = mk3(fp.mat.BaseColors[inst][0], fp.mat.BaseColors[inst][1], fp.mat.BaseColors[inst][2]);
      rghMtl = getRoughMetal(fp.mat, inst, a.UV);
      const f4 hPrev = mulPoint(a.Pos, cbLoad4x4(fp.g.WorldViewProjsPrev[inst]));
      velocity.x = (screenPos.x - hPrev.x / hPrev.w) * 0.5f; velocity.y = (screenPos.y - hPrev.y / hPrev.w) * -0.5f;
      const f4 P4 = mulPoint(a.Pos, cbLoad4x3(fp.g.Worlds[inst]));
      P = mk3(P4.x, P4.y, P4.z);
      N = normalize3(mulDir(a.Nrm, cbLoad3x3(inst ? fp.g.WorldIT1 : fp.g.WorldITs0)));
      V = normalize3(eye - P);
    } else {
      f4 sp4; sp4.x = screenPos.x; sp4.y = screenPos.y; sp4.z = 0.0f; sp4.w = 1.0f;
      const f4 world = mulVec4(sp4, cbLoad4x4(fp.rg.ProjToWorld));
      hit = false; velocity.x = 0.0f; velocity.y = 0.0f;
      P = mk3(world.x / world.w, world.y / world.w, world.z / world.w);
      N = mk3(0.0f, 0.0f, 0.0f);
      V = normalize3(eye - P);
      rghMtl.x = 0.0f; rghMtl.y = 0.0f;
      color = mk3(0.0f, 0.0f, 0.0f);
    }
    // G-buffer stores :552-554
    A.normalOut[pix] = packR10G10B10A2(N.x * 0.5f + 0.5f, N.y * 0.5f + 0.5f, N.z * 0.5f + 0.5f, hit ? 1.0f : 0.0f);
    // the reference leaves RoughMetal untouched where nothing is hit, and RayTracingOut1 where no diffuse ray is traced:
    // with several input sets "untouched" means carrying the word of the previous frame's set over.  RoughMetal is carried here
    // (the previous set's was written by the previous ray generation, earlier on this stream); RayTracingOut1 below or by shadeKernel
    A.roughMetalOut[pix] = hit ? (uint16_t)packR8G8(rghMtl.x, rghMtl.y) : A.roughMetalPrev[pix];
    A.velocityOut[pix] = packR16G16F(velocity.x, velocity.y);

    if (!hit) {
      // degenerate ray [0,0] along -V always misses: missMain, environment mip 0; metallic 0 < 1 -> same for the diffuse target
      const uint32_t c = packR11G11B10F(environmentLevel0(env, -V));
      A.reflOut[pix] = c;
      A.diffOut[pix] = c;
    } else {
      const uint32_t skip = (inst << 24) | prim;
      if (traced) {  // computeReflection depth 0 :424-484 (an untraced pixel's RayTracingOut0 is reconstructed: reconstructKernel)
        const float a = rghMtl.x * rghMtl.x;
        const bool vndf = (fp.flags & RT_FLAG_VNDF) != 0u;      // uniform
        f3 Hh;
        if (vndf) Hh = vndfHalfVector(N, V, a, cosPhi, sinPhi, xiY);
        else {
          const float cosTheta = sqrtf((1.0f - xiY) / (1.0f + (a * a - 1.0f) * xiY));
          const float sinTheta = sqrtf(1.0f - cosTheta * cosTheta);
          Hh = localToWorld(N, mk3(cosPhi * sinTheta, sinPhi * sinTheta, cosTheta));
        }
        const f3 R = reflect3(-V, Hh);
        const float NoL = dot3(N, R);
        if (NoL <= 0.0f) A.reflOut[pix] = 0u;   // :459
        else {
          const f3 f0 = mk3(lerpf(0.04f, color.x, rghMtl.y), lerpf(0.04f, color.y, rghMtl.y), lerpf(0.04f, color.z, rghMtl.y));
          const float NoV = saturatef(dot3(N, V));
          const float VoH = saturatef(dot3(V, Hh));
          const f3 F = fSchlick(f0, VoH);
          const float vis = visSmith(rghMtl.x, NoV, NoL);
          const float NoH = saturatef(dot3(N, Hh));
          const float k = 4.0f * VoH / NoH;
          wantRefl = true;
          rr.ox = P.x; rr.oy = P.y; rr.oz = P.z;
          rr.dx = R.x; rr.dy = R.y; rr.dz = R.z;
          rr.pixel = (uint32_t)pix; rr.skip = skip; rr.flags = 0u;
          rr.wx = ((NoL * F.x) * vis) * k; rr.wy = ((NoL * F.y) * vis) * k; rr.wz = ((NoL * F.z) * vis) * k;   // :477
          if (vndf) {      // BRDF x NoL / pdf of the visible-normal sampler = F x G2 / G1(V) = F x G1(L), with the separable Smith terms of Vis_Smith
            const float a2 = a * a;
            const float g1l = (2.0f * NoL) / (NoL + sqrtf(NoL * (NoL - NoL * a2) + a2));
            rr.wx = F.x * g1l; rr.wy = F.y * g1l; rr.wz = F.z * g1l;
          }
        }
      }
      if (rghMtl.y < 1.0f) {   // :559-564, computeDiffuse depth 0 :486-535
        if (traced) {
          const float cosTheta = 1.0f - 2.0f * xiY;
          const float sinTheta = sqrtf(1.0f - cosTheta * cosTheta);
          const f3 dir = normalize3(N + mk3(cosPhi * sinTheta, sinPhi * sinTheta, cosTheta));
          wantDiff = true;
          rd.ox = P.x; rd.oy = P.y; rd.oz = P.z;
          rd.dx = dir.x; rd.dy = dir.y; rd.dz = dir.z;
          rd.pixel = (uint32_t)pix; rd.skip = skip; rd.flags = 1u;
          rd.wx = color.x * (1.0f - 0.04f); rd.wy = color.y * (1.0f - 0.04f); rd.wz = color.z * (1.0f - 0.04f);   // :532
        }
      } else if (A.diffPrev != nullptr) A.diffOut[pix] = A.diffPrev[pix];      // RayTracingOut1 keeps what it held: carried over from the previous frame's set, here or by shadeKernel (launchShade)
    }
  }
  if (threadIdx.x == 0) { A.skyOut[tile] = skyWordOut; if (clearNext) A.visDirtyNextOut[tile] = 0u; }      // (visDirtyNext: read above by this workgroup only)
  if constexpr (RATE == 4) { rayGenQuadBin(A, wantRefl, wantDiff, rr, rd); return; }

  // wave-level compaction into this wave's own bin (rt_queue.h): reflection rays first, then diffuse rays
  const uint32_t bin = blockIdx.x * 4u + wave;
  const unsigned long long maskR = __ballot(wantRefl), maskD = __ballot(wantDiff), below = (1ull << lane) - 1ull;
  const uint32_t nR = (uint32_t)__popcll(maskR);
  RayRec* dst = A.rays + (size_t)bin * A.binSlots;
  HitKey* keys = A.hits + (size_t)bin * A.binSlots;      // every ray starts as a miss at TMax
  if (wantRefl) { const uint32_t k = (uint32_t)__popcll(maskR & below); dst[k] = rr; keys[k] = hitKey(RT_RAY_TMAX, 0xFFFFFFFFu); }
  // (a diffuse ray needs bins of two rays per pixel: rtggx_update_frame grows them with the first metallic below 1, and launchRayTrace
  // refuses a frame whose materials and bins disagree.  The bound here is the last line: a record is never written beyond its bin.)
  const uint32_t kD = nR + (uint32_t)__popcll(maskD & below);
  if (wantDiff && kD < A.binSlots) { dst[kD] = rd; keys[kD] = hitKey(RT_RAY_TMAX, 0xFFFFFFFFu); }
  const uint32_t nRaysInBin = min(nR + (uint32_t)__popcll(maskD), A.binSlots);
  if (A.binWork == nullptr) {
    if (lane == 0) A.binCount[bin] = nRaysInBin;
    return;
  }
  // Adaptive split (trace.hip).  What this bin's rays cost in the previous frame decides whether it goes on the split
  // list -- whose bins the trace kernel starts first -- and how many waves trace it: one per `splitWork` lane-steps, up
  // to 2^splitMaxShift.  One atomic per workgroup allocates the entries of its four bins; the count keeps running past
  // the list's capacity (the host sizes the next launches from it).
  __shared__ uint32_t want[4], listBase;
  uint32_t shift = 0u, n = 0u;
  if (lane == 0) {
    const uint32_t w = A.binWork[bin];
    A.binWork[bin] = 0u;
    while (shift < A.splitMaxShift && (w >> shift) > A.splitWork) ++shift;
    n = (shift || w > A.frontWork) ? 1u << shift : 0u;
    want[wave] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) { const uint32_t total = want[0] + want[1] + want[2] + want[3]; listBase = total ? atomicAdd(A.splitCount, total) : 0u; }
  __syncthreads();
  if (lane == 0) {
    uint32_t base = listBase, mark = 0u;
    for (uint32_t k = 0; k < wave; ++k) base += want[k];
    if (n) {
      const bool fits = base + n <= A.splitCap;
      for (uint32_t k = 0; k < n && base + k < A.splitCap; ++k) A.splitList[base + k] = fits ? ((shift << 28) | (k << 24) | bin) : 0xFFFFFFFFu;
      mark = fits ? (shift << 1) | 1u : 0u;
    }
    A.binCount[bin] = nRaysInBin | (mark << 8);     // rays in the bin | bit 8: on the split list | bits 9..: log2(its waves)
  }
}

// =========================================================================================================
// Kernel 3: hit / miss shading
// =========================================================================================================
struct ShadeArgs {
  const RayRec* rays; const HitKey* hits; const uint32_t* binCount; uint32_t binSlots;
  const float4* fat0; const float4* fat1;
  const uint2* env; const uint32_t* envMipOffset; uint32_t envSize, envMips;
  const float* sh;
  uint32_t* reflOut; uint32_t* diffOut;
  // carry-over of RayTracingOut1 (see the kernel)
  const uint32_t* diffPrev; const unsigned long long* visDepth; uint32_t tilesX, rowBegin, rowEnd, carryMask;
  const uint32_t* tileWords;      // one word per tile of this kernel, 0 = nothing was drawn there (rtggx_context.h VisTarget::dirty): no rays, nothing to carry
  // the spawning pass (SHADE_SPAWN): each ray's child goes back into the ray's own bin, in place (the same arrays as rays / hits / binCount)
  RayRec* spawnRays; HitKey* spawnHits; uint32_t* spawnCount; const float* cosSin;
  // the accumulating passes (SHADE_ACCUM, SHADE_SPAWN_ACCUM): the fp32 sums of the two images, three floats per pixel
  float* accRefl; float* accDiff;
};

// The shading passes of a path of recursion depth D (rtggx_set_max_recursion_depth; DESIGN.md "Recursion depth"): level d < D - 1 shades
// its hits by spawning the next level's rays (SHADE_SPAWN), level D - 1 finishes every path (SHADE_FINAL at D = 1 -- the code of the depth-1
// renderer, unchanged --, SHADE_FINAL_DEEP after it).  A path ends in the spawning pass where its ray misses, where a reflection-group
// ray's preset is <= 0, and where NoL <= 0.  Ray flags: bit 0 the hit group (1: diffuse); bit 1 set where the image the path writes --
// that of its level-0 ray's group -- differs from the group of the ray in hand (never at level 0).
// With N > 1 samples per pixel (rtggx_set_samples_per_pixel; DESIGN.md "Samples per pixel") a path's value c * T is ADDED to the pixel's fp32
// sum instead of being packed into the image: SHADE_ACCUM ends every path (the image from the ray's flags, as SHADE_FINAL_DEEP -- at level 0
// bit 1 is clear), SHADE_SPAWN_ACCUM is SHADE_SPAWN for the paths that end in it.  One lane per (pixel, image) and pass, the passes in
// stream order, sample after sample: the sum's order is k = 0, 1, ..., N - 1 whatever the scheduling (no atomics).  A sample that traces
// nothing adds nothing: acc + 0 = acc.  resolveSamplesKernel packs the sums.
enum ShadePass { SHADE_FINAL = 0, SHADE_SPAWN = 1, SHADE_FINAL_DEEP = 2, SHADE_ACCUM = 3, SHADE_SPAWN_ACCUM = 4 };
constexpr bool shadeSpawns(int pass) { return pass == SHADE_SPAWN || pass == SHADE_SPAWN_ACCUM; }
constexpr bool shadeAccumulates(int pass) { return pass == SHADE_ACCUM || pass == SHADE_SPAWN_ACCUM; }

// computeReflection at recursion depth 1 (:424-484)
RT_DEV f3 reflectionDepth1(const EnvRef& env, f2 rghMtl, f3 N, f3 V, f3 color) {
  const float level = calcMipFromRoughness(rghMtl.x, (float)env.mips);
  const float a = rghMtl.x * rghMtl.x;
  const f3 R = reflect3(-V, N);
  const f3 dir = lerp3(N, R, (1.0f - a) * (sqrtf(1.0f - a) + a));
  const float NoL = dot3(N, dir);
  if (NoL <= 0.0f) return mk3(0.0f, 0.0f, 0.0f);
  const f3 e = environment(env, dir, level);
  const f3 f0 = mk3(lerpf(0.04f, color.x, rghMtl.y), lerpf(0.04f, color.y, rghMtl.y), lerpf(0.04f, color.z, rghMtl.y));
  const float NoV = saturatef(dot3(N, V));
  return e * envBRDFApprox(f0, rghMtl.x, NoV);
}

// Rate 4: workgroup b shades the four bins of 32x32 tile b (rayGenKernel), one per wave as at rate 1; its tile word is the OR of the words of
// the 16x16 tiles in it.  RayTracingOut1 is carried over by reconstructKernel instead, which visits every covered pixel anyway.
RT_DEV uint32_t quadTileWord(const uint32_t* words, uint32_t tile32, uint32_t tilesX, uint32_t tilesY) {
  const uint32_t superX = (tilesX + 1u) >> 1, tx = (tile32 % superX) * 2u, ty = (tile32 / superX) * 2u;
  const uint32_t i0 = ty * tilesX + tx;
  const bool right = tx + 1u < tilesX, down = ty + 1u < tilesY;
  const uint32_t i1 = right ? i0 + 1u : i0, i2 = down ? i0 + tilesX : i0, i3 = right && down ? i0 + tilesX + 1u : i0;
  uint32_t a, b, c, d;
  asm volatile("s_load_dword %0, %4, %5\n\ts_load_dword %1, %4, %6\n\ts_load_dword %2, %4, %7\n\ts_load_dword %3, %4, %8\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d)
               : "s"(words), "s"(RT_SGPR(i0 * 4u)), "s"(RT_SGPR(i1 * 4u)), "s"(RT_SGPR(i2 * 4u)), "s"(RT_SGPR(i3 * 4u)) : "memory");
  return a | b | c | d;
}
template <int RATE, int PASS, bool WIDE = false>
__global__ void __launch_bounds__(256, RT_GEN_MIN_BLOCKS) shadeKernel(const FrameParams* __restrict__ fpp, ShadeArgs A) {
  const FrameParams& fp = *fpp;
  const EnvRef env{A.env, A.envSize, A.envMips, A.envMipOffset};
  // workgroup b shades the four bins its rayGen namesake filled: wave w <-> bin 4b + w
  // (Round 4, measured and dropped: a LIST of the bins -- or tiles -- with a surface, appended by ray generation, walked here by a grid of
  // eight workgroups per CU, instead of three quarters of this kernel's waves reading a zero and leaving.  One atomic per wave with a
  // surface, ~8 000 per frame on one word, runs at the memory side of eight L2s: ray generation 80 -> 155 us in the frame, the frame
  // 0.185 -> 0.266 ms; one per tile behind a workgroup barrier: ray generation 80 -> 91 us, the frame +1.3 %.  profiles/r04_j_tile_words.txt)
  const uint32_t tile = blockIdx.x;
  { uint32_t word;      // three quarters of the bunny frame's workgroups leave here, after one scalar load (before: a vector load of the bin's count each)
    if constexpr (RATE == 1) asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(word) : "s"(A.tileWords), "s"(tile * 4u) : "memory");
    else word = quadTileWord(A.tileWords, tile, A.tilesX, (A.rowEnd - A.rowBegin + 15u) / 16u);
    if (word == 0u) return; }
  const uint32_t bin = tile * 4u + (threadIdx.x >> 6);
  // Carry-over of RayTracingOut1.  The reference has ONE such texture and leaves it untouched where no diffuse ray is traced
  // (covered pixels of a fully metallic instance, RayTracing.hlsl:559): it keeps the last value ever written there.  With three
  // input sets that is the word of the previous frame's set -- final only once that frame's shading has run, which is earlier
  // on THIS stream; ray generation (stream C, a frame ahead of this stream) must not read it.  The wave's bin is its 8x8 pixel
  // sub-tile, so it walks those pixels: covered by an instance with metallic >= 1 (carryMask bit per instance) -> copy.
  if (RATE == 1 && A.carryMask != 0u) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t px = (tile % A.tilesX) * 16u + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t py = A.rowBegin + (tile / A.tilesX) * 16u + (wave >> 1) * 8u + (lane >> 3);
    if (px < fp.W && py < A.rowEnd) {
      const size_t pix = (size_t)py * fp.W + px;
      const uint32_t vis = (uint32_t)A.visDepth[pix];
      if (vis != 0u && ((A.carryMask >> ((vis - 1u) >> 24)) & 1u)) A.diffOut[pix] = A.diffPrev[pix];
    }
  }
  const uint32_t count = min(A.binCount[bin] & 0xFFu, A.binSlots);
  uint32_t spawned = 0u;      // SHADE_SPAWN: children written to the front of the bin so far (a child's slot is never above its parent's)
  for (uint32_t i = threadIdx.x & 63u; i < count; i += 64u) {
    const size_t slot = (size_t)bin * A.binSlots + i;
    const float4* rp = reinterpret_cast<const float4*>(A.rays + slot);
    const float4 q0 = rp[0], q1 = rp[1], q2 = rp[2];
    // the round-1 names: ra = origin, rb = direction, rc = (pixel, skip, flags), rw = weight
    const float4 ra = make_float4(q0.x, q0.y, q0.z, RT_RAY_TMIN), rb = make_float4(q0.w, q1.x, q1.y, RT_RAY_TMAX), rw = make_float4(q2.x, q2.y, q2.z, 0.0f);
    const uint4 rc = make_uint4(__float_as_uint(q1.z), __float_as_uint(q1.w), __float_as_uint(q2.w), 0u);
    const uint32_t hitId = hitKeyId(A.hits[slot]);
    const f3 dir = mk3(rb.x, rb.y, rb.z);
    const bool diffuseGroup = (rc.z & 1u) != 0u;
    const uint32_t srcInst = rc.y >> 24;
    f3 col;
    bool child = false; RayRec cr;      // SHADE_SPAWN: the path goes on with this ray
    if (hitId == 0xFFFFFFFFu) col = environmentLevel0(env, dir);   // missMain :620-625
    else {
      // payload preset = color * metallic of the surface the ray left (:456); closestHitReflection returns it untouched when <= 0 (:573)
      const float m = fp.mat.RoughMetals[srcInst][1];
      const f3 preset = mk3(fp.mat.BaseColors[srcInst][0] * m, fp.mat.BaseColors[srcInst][1] * m, fp.mat.BaseColors[srcInst][2] * m);
      if (!diffuseGroup && preset.x <= 0.0f && preset.y <= 0.0f && preset.z <= 0.0f) col = preset;
      else {
        const uint32_t hInst = hitId >> 24;
        uint32_t hPrim = hitId & 0xFFFFFFu;
        // hipcc 7.2 drops this mask when the same id also indexes a two-element array (it then addresses the triangle
        // with the whole id: a fault for every hit on instance 1): keep it behind a barrier, and select instead of index
        asm volatile("" : "+v"(hPrim));
        const Tri3 v = getVertices(hInst ? A.fat1 : A.fat0, hPrim);
        // the hit attributes (barycentrics) of the recorded triangle: the traversal's own test, repeated
        float ht, hb1 = 0.0f, hb2 = 0.0f;
        woopTestVerts(toObject(ra.x, ra.y, ra.z, rb.x, rb.y, rb.z, hInst ? fp.invWorld[1] : fp.invWorld[0]), v.pos[0], v.pos[1], v.pos[2], ht, hb1, hb2);
        const Attrib a = interpAttrib(v, hb1, hb2);
        const f3 N = normalize3(mulDir(a.Nrm, cbLoad3x3(hInst ? fp.g.WorldIT1 : fp.g.WorldITs0)));
        const f2 rm = getRoughMetal(fp.mat, hInst, a.UV);
        f3 color = mk3(fp.mat.BaseColors[hInst][0], fp.mat.BaseColors[hInst][1], fp.mat.BaseColors[hInst][2]);
        const f3 V = -dir;
        if constexpr (!shadeSpawns(PASS)) {
          if (rm.y > 0.5f) col = reflectionDepth1(env, rm, N, V, color);
          else {
            if (diffuseGroup) color = color * (1.0f - rm.y);                 // :607
            const f3 irr = evaluateSHIrradiance(A.sh, N);                    // computeDiffuse depth 1 :513,532
            col = mk3(irr.x / RT_PI, irr.y / RT_PI, irr.z / RT_PI) * color;
          }
        } else {
          // the closest-hit shaders at depth d + 1 < D (:571-614): hitWorldPosition (:338-341), getSampleParam(DispatchRaysIndex()) -- the
          // pixel's xi at every level --, then computeReflection / computeDiffuse up to their TraceRay
          const f3 P = mk3(ra.x + ht * rb.x, ra.y + ht * rb.y, ra.z + ht * rb.z);
          float xiY, cosPhi, sinPhi;
          if constexpr (WIDE) sampleParamWide(fp, A.cosSin, rc.x, xiY, cosPhi, sinPhi);
          else {
            uint32_t s = rng(rc.x); s += fp.g.FrameIndex; s = rng(s); s %= 256u;
            xiY = (float)(rng(s) & 0xffffu) / 65536.0f; cosPhi = A.cosSin[s]; sinPhi = A.cosSin[256 + s];
          }
          const uint32_t toDiffImage = (rc.z ^ (rc.z >> 1)) & 1u;
          f3 w, L;
          if (rm.y > 0.5f) {
            const bool vndf = (fp.flags & RT_FLAG_VNDF) != 0u;
            const f3 Hh = reflectionHalfVector(vndf, N, V, rm.x * rm.x, cosPhi, sinPhi, xiY);
            L = reflect3(-V, Hh);
            const float NoL = dot3(N, L);
            if (NoL <= 0.0f) col = mk3(0.0f, 0.0f, 0.0f);                // :459
            else { w = reflectionWeight(vndf, N, V, Hh, NoL, rm, color); child = true; cr.flags = toDiffImage << 1; }
          } else {
            if (diffuseGroup) color = color * (1.0f - rm.y);                 // :607
            L = diffuseDirection(N, cosPhi, sinPhi, xiY);
            w = color; child = true; cr.flags = 1u | ((toDiffImage ^ 1u) << 1);      // no x (1 - 0.04) at depth >= 1 (:532)
          }
          if (child) {
            cr.ox = P.x; cr.oy = P.y; cr.oz = P.z; cr.dx = L.x; cr.dy = L.y; cr.dz = L.z;
            cr.pixel = rc.x; cr.skip = hitId;
            cr.wx = rw.x * w.x; cr.wy = rw.y * w.y; cr.wz = rw.z * w.z;      // the path's throughput
          }
        }
      }
    }
    if constexpr (shadeSpawns(PASS)) {
      // compaction into the bin, in place: this round's records have been read (and waited for) before any lane writes
      const unsigned long long mask = __ballot(child);
      if (child) {
        const size_t k = (size_t)bin * A.binSlots + spawned + (uint32_t)__popcll(mask & ((1ull << (threadIdx.x & 63u)) - 1ull));
        A.spawnRays[k] = cr; A.spawnHits[k] = hitKey(RT_RAY_TMAX, 0xFFFFFFFFu);
      }
      spawned += (uint32_t)__popcll(mask);
      if (child) continue;
    }
    if constexpr (shadeAccumulates(PASS)) {
      float* acc = (((rc.z ^ (rc.z >> 1)) & 1u) != 0u ? A.accDiff : A.accRefl) + 3u * (size_t)rc.x;
      acc[0] = acc[0] + col.x * rw.x; acc[1] = acc[1] + col.y * rw.y; acc[2] = acc[2] + col.z * rw.z;
      continue;
    }
    const uint32_t packed = packR11G11B10F(mk3(col.x * rw.x, col.y * rw.y, col.z * rw.z));
    const bool toDiff = PASS == SHADE_FINAL ? diffuseGroup : ((rc.z ^ (rc.z >> 1)) & 1u) != 0u;
    if (toDiff) A.diffOut[rc.x] = packed; else A.reflOut[rc.x] = packed;
  }
  if constexpr (shadeSpawns(PASS)) { if ((threadIdx.x & 63u) == 0u) A.spawnCount[bin] = spawned; }
}

// =========================================================================================================
// Kernel 4 (rate 4 only): reconstruction of the untraced pixels, in place (DESIGN.md "Quarter-rate tracing")
// =========================================================================================================
// It reads only traced pixels and writes only untraced covered ones, so RayTracingOut0/1 serve as input and output.  For an untraced covered
// pixel c the candidates are the traced pixels q at Chebyshev distance 1, inside the frame, covered by c's instance (2 or 4 of them):
//   RayTracingOut0 = sum w L(q) / sum w,  w = NormalWeight(nc, nq, 32) DepthWeight(zc, zq, 4) RoughnessWeight(rc, rq, 0, 0.5)
//   RayTracingOut1 = the same with w = NormalWeight(nc, nq, 32) DepthWeight(zc, zq, 4) (DiffuseWeight), where c's metallic < 1
// (FilterCommon.hlsli:34-47, SpatialFilter.hlsli:69-75) on the G-buffer words the filters read: normals 10-bit UNORM x 2 - 1, not
// renormalised; D24 depth / (2^24 - 1); R8 roughness.  sum w = 0: the plain mean of the candidates; no candidate: the plain mean of c's
// instance's traced pixels within Chebyshev distance 2; none: 0.  The normal weight's 32nd power is five squarings of the fp32 dot product
// (its integer numerator is exact); the depth weight's exp and the final divisions are evaluated in fp64 and rounded once to fp32, i.e.
// correctly rounded; everything else is fp32 without contraction (Makefile).  So tests/ray_rate_ref.py restates it bit for bit in numpy:
// reconstructed values often lie next to a rounding tie of R11G11B10 (the mean of two codes), and an ulp of a weight would decide the side.
// Where c's metallic >= 1 RayTracingOut1 is carried over from the previous set (carryMask), at traced pixels as well (the rate-1 rule).
struct ReconArgs {
  const unsigned long long* visDepth; const uint32_t* normal; const uint16_t* roughMetal; const uint32_t* depth32;
  uint32_t* reflOut; uint32_t* diffOut;       // read at traced pixels, written at the others
  const uint32_t* diffPrev; uint32_t carryMask, diffMask;      // bit per instance: metallic >= 1 (carry RayTracingOut1 over) / < 1 (reconstruct it)
  const uint32_t* tileWords; uint32_t tilesX, rowBegin, rowEnd;
};
struct ReconTexel { float nx, ny, nz, depth, rough; };
RT_DEV ReconTexel reconTexel(const ReconArgs& A, size_t i) {
  const uint32_t n = A.normal[i];
  ReconTexel t;
  t.nx = (float)(2 * (int)(n & 1023u) - 1023); t.ny = (float)(2 * (int)((n >> 10) & 1023u) - 1023); t.nz = (float)(2 * (int)((n >> 20) & 1023u) - 1023);
  t.depth = (float)A.depth32[i] * (1.0f / 16777215.0f);
  t.rough = (float)(A.roughMetal[i] & 0xFFu) * (1.0f / 255.0f);
  return t;
}
RT_DEV float reconNormalDepthWeight(const ReconTexel& c, const ReconTexel& q) {
  const float I = (c.nx * q.nx + c.ny * q.ny) + c.nz * q.nz;            // integers below 2^24: exact
  float x = fmaxf(I * (1.0f / 1046529.0f), 0.0f);                       // dot(nc, nq) = I / 1023^2, one rounding
  x = x * x; x = x * x; x = x * x; x = x * x; x = x * x;                 // ^32
  return x * (float)exp((double)(-fabsf(c.depth - q.depth) * c.depth * 4.0f));      // SIGMA_Z = 4; fp64: correctly rounded
}
RT_DEV f3 reconDivide(f3 s, float w) {      // correctly rounded (fp64 quotient, one rounding to fp32), whatever the fp32 division lowers to
  const double d = (double)w;
  return mk3((float)((double)s.x / d), (float)((double)s.y / d), (float)((double)s.z / d));
}
__global__ void __launch_bounds__(256) reconstructKernel(const FrameParams* __restrict__ fpp, ReconArgs A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  { uint32_t word;      // a 16x16 tile of ray generation's grid: nothing drawn there, nothing to do
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(word) : "s"(A.tileWords), "s"(tile * 4u) : "memory");
    if (word == 0u) return; }
  const uint32_t W = fp.W;
  const uint32_t px = (tile % A.tilesX) * 16u + (threadIdx.x & 15u), py = A.rowBegin + (tile / A.tilesX) * 16u + (threadIdx.x >> 4);
  if (px >= W || py >= A.rowEnd) return;
  const size_t pix = (size_t)py * W + px;
  const uint32_t vis = (uint32_t)A.visDepth[pix];
  if (vis == 0u) return;      // background: both images were written by ray generation
  const uint32_t inst = (vis - 1u) >> 24;
  if ((A.carryMask >> inst) & 1u) A.diffOut[pix] = A.diffPrev[pix];
  const uint32_t f = fp.g.FrameIndex & 3u, ox = (0x6u >> f) & 1u, oy = (0xAu >> f) & 1u;
  if ((px & 1u) == ox && (py & 1u) == oy) return;      // traced
  const bool diffuse = ((A.diffMask >> inst) & 1u) != 0u;
  const ReconTexel c = reconTexel(A, pix);
  f3 sumR = mk3(0.0f, 0.0f, 0.0f), sumD = sumR, meanR = sumR, meanD = sumR;
  float wR = 0.0f, wD = 0.0f;
  uint32_t n = 0u;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = (int)px + dx, qy = (int)py + dy;
      if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)fp.H || ((uint32_t)qx & 1u) != ox || ((uint32_t)qy & 1u) != oy) continue;
      const size_t q = (size_t)qy * W + (uint32_t)qx;
      const uint32_t vq = (uint32_t)A.visDepth[q];
      if (vq == 0u || ((vq - 1u) >> 24) != inst) continue;
      const ReconTexel t = reconTexel(A, q);
      const float wnd = reconNormalDepthWeight(c, t);
      const float ts = saturatef(fabsf(t.rough - c.rough) * 2.0f);
      const float w = wnd * (1.0f - ts * ts * (3.0f - 2.0f * ts));
      const f3 L = unpackR11G11B10F(A.reflOut[q]);
      sumR = sumR + L * w; wR += w; meanR = meanR + L;
      if (diffuse) { const f3 Ld = unpackR11G11B10F(A.diffOut[q]); sumD = sumD + Ld * wnd; wD += wnd; meanD = meanD + Ld; }
      ++n;
    }
  if (n == 0u) {      // no candidate at distance 1: the traced pixels of c's instance within distance 2
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll 1
      for (int dx = -2; dx <= 2; ++dx) {
        const int qx = (int)px + dx, qy = (int)py + dy;
        if (qx < 0 || qy < 0 || qx >= (int)W || qy >= (int)fp.H || ((uint32_t)qx & 1u) != ox || ((uint32_t)qy & 1u) != oy) continue;
        const size_t q = (size_t)qy * W + (uint32_t)qx;
        const uint32_t vq = (uint32_t)A.visDepth[q];
        if (vq == 0u || ((vq - 1u) >> 24) != inst) continue;
        meanR = meanR + unpackR11G11B10F(A.reflOut[q]);
        if (diffuse) meanD = meanD + unpackR11G11B10F(A.diffOut[q]);
        ++n;
      }
  }
  A.reflOut[pix] = packR11G11B10F(wR > 0.0f ? reconDivide(sumR, wR) : n ? reconDivide(meanR, (float)n) : meanR);
  if (diffuse) A.diffOut[pix] = packR11G11B10F(wD > 0.0f ? reconDivide(sumD, wD) : n ? reconDivide(meanD, (float)n) : meanD);
}

// =========================================================================================================
// Kernels 5-7 (N > 1 samples per pixel only; rtggx_set_samples_per_pixel, DESIGN.md "Samples per pixel")
// =========================================================================================================
// Sample k of frame F is the sample of a one-sample frame with FrameIndex F * N + k (include/rtggx.h), and the frame index enters a frame
// nowhere but getSampleParam -- in ray generation, in the spawning shading pass and below.  So sample k's kernels are given a COPY of the
// frame's constants with that index, and ray generation (sample 0) and the spawning pass serve every sample as they are.
__global__ void sampleParamsKernel(const FrameParams* __restrict__ src, FrameParams* __restrict__ dst, uint32_t samples) {
  constexpr uint32_t words = sizeof(FrameParams) / 4u, indexWord = (offsetof(FrameParams, g) + offsetof(RtggxCBGlobal, FrameIndex)) / 4u;
  for (uint32_t i = threadIdx.x; i < words * samples; i += blockDim.x) {
    const uint32_t k = i / words, w = i % words, v = reinterpret_cast<const uint32_t*>(src)[w];
    reinterpret_cast<uint32_t*>(dst + k)[w] = w == indexWord ? v * samples + k : v;
  }
}

// Sample k > 0: the rays ray generation would queue for a frame with sample k's index, into the same bins -- whose rays of the sample
// before have been shaded.  The primary surface comes from the visibility word again (rayGenKernel's arithmetic); nothing of the G-buffer,
// the images, the sky runs, the next frame's target or the adaptive split is touched: a bin's count is written without a mark, and the
// traversal of these rays (launchTrace with a spill part) neither splits nor records costs.  A tile whose word is 0 has no bin with a ray
// in it, now as before.
struct SampleGenArgs {
  const unsigned long long* visDepth; const float4* fat0; const float4* fat1; const float* cosSin;
  RayRec* rays; HitKey* hits; uint32_t* binCount; uint32_t binSlots;
  const uint32_t* tileWords; uint32_t tilesX, rowBegin, rowEnd;
};
// MAPPED (rtggx_set_sample_map; DESIGN.md "Adaptive sampling"): the wave's block traces the samples k < its count.  The map holds a byte per
// bin in bin order, so a tile's word holds its four waves' counts: one scalar load, like the tile word.  A wave whose block has had its
// samples stores the count 0 for its bin and leaves: the bin still holds the previous sample's rays and count (or, at depth D > 1, its last
// level's), and the traversal and the shading passes of this sample read that one array -- a bin that kept its count would be traced and
// added again.  (k < N always, so k >= count is k >= min(count, N).)
struct SampleGenArgsMapped : SampleGenArgs { const uint32_t* sampleMap; uint32_t sample; };
template <bool WIDE, bool MAPPED = false>
__global__ void __launch_bounds__(256, RT_GEN_MIN_BLOCKS) sampleGenKernel(const FrameParams* __restrict__ fpp, std::conditional_t<MAPPED, SampleGenArgsMapped, SampleGenArgs> A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  { uint32_t word;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(word) : "s"(A.tileWords), "s"(tile * 4u) : "memory");
    if (word == 0u) return; }
  if constexpr (MAPPED) {
    uint32_t counts;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(counts) : "s"(A.sampleMap), "s"(tile * 4u) : "memory");
    const uint32_t w = RT_SGPR(threadIdx.x >> 6);
    if (A.sample >= ((counts >> (8u * w)) & 0xFFu)) {
      if ((threadIdx.x & 63u) == 0u) A.binCount[tile * 4u + w] = 0u;
      return;
    }
  }
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t px = (tile % A.tilesX) * 16 + (wave & 1u) * 8 + (lane & 7u);
  const uint32_t py = A.rowBegin + (tile / A.tilesX) * 16 + (wave >> 1) * 8 + (lane >> 3);
  bool wantRefl = false, wantDiff = false;
  RayRec rr, rd;
  if (px < fp.W && py < A.rowEnd) {
    const uint32_t W = fp.W, H = fp.H;
    const size_t pix = (size_t)py * W + px;
    uint32_t visibility = (uint32_t)A.visDepth[pix];
    float xiY, cosPhi, sinPhi;      // getSampleParam :394-406
    if constexpr (WIDE) sampleParamWide(fp, A.cosSin, py * W + px, xiY, cosPhi, sinPhi);
    else {
      uint32_t s = py * W + px;
      s = rng(s); s += fp.g.FrameIndex; s = rng(s); s %= 256u;
      xiY = (float)(rng(s) & 0xffffu) / 65536.0f; cosPhi = A.cosSin[s]; sinPhi = A.cosSin[256 + s];
    }
    if (visibility > 0) {      // getPrimarySurface :277-333, the covered branch
      --visibility;
      const uint32_t inst = visibility >> 24;
      uint32_t prim = visibility & 0xFFFFFFu;
      asm volatile("" : "+v"(prim));      // see shadeKernel
      f2 screenPos; screenPos.x = ((float)px + 0.5f) / (float)W * 2.0f - 1.0f; screenPos.y = ((float)py + 0.5f) / (float)H * 2.0f - 1.0f;
      screenPos.y = -screenPos.y;
      const f3 eye = mk3(fp.rg.EyePt[0], fp.rg.EyePt[1], fp.rg.EyePt[2]);
      const Tri3 v = getVertices(inst ? A.fat1 : A.fat0, prim);
      const M4 wvp = cbLoad4x4(fp.g.WorldViewProjs[inst]);
      f4 p[3];
      for (int k = 0; k < 3; ++k) p[k] = mulPoint(v.pos[k], wvp);
      screenPos.x -= fp.rg.ProjBias[0]; screenPos.y -= fp.rg.ProjBias[1];
      const f2 bary = calcBarycentrics(p, screenPos);
      const Attrib a = interpAttrib(v, bary.x, bary.y);
      const f3 color = mk3(fp.mat.BaseColors[inst][0], fp.mat.BaseColors[inst][1], fp.mat.BaseColors[inst][2]);
      const f2 rghMtl = getRoughMetal(fp.mat, inst, a.UV);
      const f4 P4 = mulPoint(a.Pos, cbLoad4x3(fp.g.Worlds[inst]));
      const f3 P = mk3(P4.x, P4.y, P4.z);
      const f3 N = normalize3(mulDir(a.Nrm, cbLoad3x3(inst ? fp.g.WorldIT1 : fp.g.WorldITs0)));
      const f3 V = normalize3(eye - P);
      const uint32_t skip = (inst << 24) | prim;
      {  // computeReflection depth 0 :424-484
        const bool vndf = (fp.flags & RT_FLAG_VNDF) != 0u;      // uniform
        const f3 Hh = reflectionHalfVector(vndf, N, V, rghMtl.x * rghMtl.x, cosPhi, sinPhi, xiY);
        const f3 R = reflect3(-V, Hh);
        const float NoL = dot3(N, R);
        if (NoL > 0.0f) {   // :459
          const f3 w = reflectionWeight(vndf, N, V, Hh, NoL, rghMtl, color);
          wantRefl = true;
          rr.ox = P.x; rr.oy = P.y; rr.oz = P.z; rr.dx = R.x; rr.dy = R.y; rr.dz = R.z;
          rr.pixel = (uint32_t)pix; rr.skip = skip; rr.flags = 0u;
          rr.wx = w.x; rr.wy = w.y; rr.wz = w.z;
        }
      }
      if (rghMtl.y < 1.0f) {   // :559-564, computeDiffuse depth 0 :486-535
        const f3 dir = diffuseDirection(N, cosPhi, sinPhi, xiY);
        wantDiff = true;
        rd.ox = P.x; rd.oy = P.y; rd.oz = P.z; rd.dx = dir.x; rd.dy = dir.y; rd.dz = dir.z;
        rd.pixel = (uint32_t)pix; rd.skip = skip; rd.flags = 1u;
        rd.wx = color.x * (1.0f - 0.04f); rd.wy = color.y * (1.0f - 0.04f); rd.wz = color.z * (1.0f - 0.04f);   // :532
      }
    }
  }
  // wave-level compaction into this wave's own bin, as in rayGenKernel<1>: reflection rays first, then diffuse rays
  const uint32_t bin = blockIdx.x * 4u + wave;
  const unsigned long long maskR = __ballot(wantRefl), maskD = __ballot(wantDiff), below = (1ull << lane) - 1ull;
  const uint32_t nR = (uint32_t)__popcll(maskR);
  RayRec* dst = A.rays + (size_t)bin * A.binSlots;
  HitKey* keys = A.hits + (size_t)bin * A.binSlots;
  if (wantRefl) { const uint32_t k = (uint32_t)__popcll(maskR & below); dst[k] = rr; keys[k] = hitKey(RT_RAY_TMAX, 0xFFFFFFFFu); }
  const uint32_t kD = nR + (uint32_t)__popcll(maskD & below);
  if (wantDiff && kD < A.binSlots) { dst[kD] = rd; keys[kD] = hitKey(RT_RAY_TMAX, 0xFFFFFFFFu); }      // (never beyond the bin: rayGenKernel)
  if (lane == 0) A.binCount[bin] = min(nR + (uint32_t)__popcll(maskD), A.binSlots);
}

// After the last sample: the word of every covered pixel from its sums, pack_r11g11b10(acc * (1 / N)) -- N is a power of two, the scaling
// exact --, RayTracingOut1 where the pixel's metallic < 1 (diffMask, bit per instance; elsewhere it keeps what was carried over).  The sums
// are left zero for the next frame.  Background pixels hold the environment from ray generation: no ray, no averaging.
// MAPPED (rtggx_set_sample_map): the scale is 1 / c of the pixel's block, c = min(its count, N) -- 1, 2, 4 or 8, as exact.  The 16 x 16
// lanes span two blocks per wave, so every lane loads the byte of its own bin.
struct ResolveArgs {
  const unsigned long long* visDepth; float* accRefl; float* accDiff; uint32_t* reflOut; uint32_t* diffOut;
  const uint32_t* tileWords; uint32_t tilesX, rowBegin, rowEnd, diffMask; float scale;
};
struct ResolveArgsMapped : ResolveArgs { const uint8_t* sampleMap; uint32_t samples; };
template <bool MAPPED = false>
__global__ void __launch_bounds__(256) resolveSamplesKernel(const FrameParams* __restrict__ fpp, std::conditional_t<MAPPED, ResolveArgsMapped, ResolveArgs> A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  { uint32_t word;
    asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(word) : "s"(A.tileWords), "s"(tile * 4u) : "memory");
    if (word == 0u) return; }
  const uint32_t px = (tile % A.tilesX) * 16u + (threadIdx.x & 15u), py = A.rowBegin + (tile / A.tilesX) * 16u + (threadIdx.x >> 4);
  if (px >= fp.W || py >= A.rowEnd) return;
  const size_t pix = (size_t)py * fp.W + px;
  const uint32_t vis = (uint32_t)A.visDepth[pix];
  if (vis == 0u) return;
  float scale = A.scale;
  if constexpr (MAPPED) scale = 1.0f / (float)min((uint32_t)A.sampleMap[tile * 4u + ((threadIdx.x >> 7) & 1u) * 2u + ((threadIdx.x >> 3) & 1u)], A.samples);
  float* r = A.accRefl + 3u * pix;
  A.reflOut[pix] = packR11G11B10F(mk3(r[0] * scale, r[1] * scale, r[2] * scale));
  r[0] = 0.0f; r[1] = 0.0f; r[2] = 0.0f;
  if ((A.diffMask >> ((vis - 1u) >> 24)) & 1u) {
    float* d = A.accDiff + 3u * pix;
    A.diffOut[pix] = packR11G11B10F(mk3(d[0] * scale, d[1] * scale, d[2] * scale));
    d[0] = 0.0f; d[1] = 0.0f; d[2] = 0.0f;
  }
}

// =========================================================================================================
// host side
// =========================================================================================================
// Still sky, once in 2^24 bumps of the epoch (rt_sky_chain.h takeWrapped): no word of an earlier time round may meet its epoch again.
// Every run word and every settled word is cleared, with the device idle before and after.
static int clearSkyWordsAfterWrap(rtggx_context* c) {
  RT_HIP(hipDeviceSynchronize());
  for (auto& st : c->sets) RT_HIP(hipMemset(st.skyRun, 0, c->skyTiles * 4));
  { const int r = resetSettled(c); if (r) return r; }
  RT_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

int launchRayTrace(rtggx_context* c, const FrameParams& fp, hipStream_t sGen, hipStream_t s, hipEvent_t done) {
  uint32_t rb, re;
  passRows(fp, ROWS_GBUFFER, rb, re);
  if (re <= rb) return 0;
  const uint32_t tilesX = (fp.W + 15) / 16, tilesY = (re - rb + 15) / 16;
  // rate 4 (rayGenKernel): one bin per 16x16 tile, numbered by 32x32 tile, and the traversal's grid of 32x32 tiles
  const bool quad = c->rayRate == 4u;
  const uint32_t quadX = (tilesX + 1u) / 2u, quadY = (tilesY + 1u) / 2u;
  if ((fp.mat.RoughMetals[0][1] < 1.0f || fp.mat.RoughMetals[1][1] < 1.0f) && c->binSlots < RT_BIN) {
    setError("rtggx_ray_trace: a material with metallic below 1 (a diffuse ray per pixel as well) but ray bins of %u slots: rtggx_update_frame sizes them", c->binSlots); return -1;
  }
  GenArgs G;
  const InputSet& set = c->cur();
  // ray generation starts the visibility pass of the frame after next (GenArgs): its target cleared, its list of large triangles emptied
  // (the list by frame parity: the one this frame's visibility pass has just used up), and the next set's split list
  { const uint32_t thenFrame = c->frameCounter + 2u;
    VisTarget& vn = c->visOf(thenFrame);
    G.visNext = vn.depth; G.zeroNext0 = c->largeCountBase + (thenFrame & 1u); G.zeroNext1 = c->next().splitCount;
    vn.cleared.frame = thenFrame; vn.cleared.rows[0] = rb; vn.cleared.rows[1] = re;
    // the tiles' words (VisTarget::dirty): usable where they were kept for these very rows
    if (c->traceShare > 0.93f) c->traversalBound = true; else if (c->traceShare < 0.89f) c->traversalBound = false;
    // (rate 4: the trace kernel's grid is of 32x32 tiles, which these words do not describe -- it is given words that are all ones)
    G.visDirty = c->tileWords(rb, re); c->traceTileWords = quad ? c->visDirtyOnes : G.visDirty;
    G.visDirtyNextOut = vn.dirty;
    G.visDirtyNext = c->useTileWords && !c->traversalBound && vn.flags.rows[0] == rb && vn.flags.rows[1] == re ? vn.dirty : c->visDirtyOnes;
    vn.flags.rows[0] = rb; vn.flags.rows[1] = re;
  }
  G.visDepth = c->curVis().depth; G.depthOut = set.depth32; G.normalOut = set.normal; G.roughMetalOut = set.roughMetal; G.velocityOut = set.velocity; G.reflOut = set.rtRefl; G.diffOut = set.rtDiff;
  G.roughMetalPrev = c->prev().roughMetal;
  G.diffPrev = c->genCarriesDiff ? c->prev().rtDiff : nullptr;
  G.fat0 = c->mesh[0].fat; G.fat1 = c->mesh[1].fat;
  G.env = c->env.texels; G.envMipOffset = c->dEnvMipOffset; G.envSize = c->env.size; G.envMips = c->env.mips; G.cosSin = c->sampleTable();
  G.rays = (RayRec*)set.rayQueue.get(); G.hits = (HitKey*)set.hitQueue.get(); G.binCount = set.binCount; G.binSlots = c->binSlots; G.frameRays = c->rayCounter32;
  G.tilesX = tilesX; G.numTiles = tilesX * tilesY; G.rowBegin = rb; G.rowEnd = re;
  const uint32_t splitWork = c->splitWork, splitMaxShift = c->splitMaxShift;
  const uint32_t numBins = quad ? quadX * quadY * 4u : G.numTiles * 4u;
  const uint32_t sliceShift = chooseSliceShift(c, true, numBins);
  // "wide" launches: few enough rays that the traversal does not fill the chip for long (trace.hip launchTrace, frame.hip rtggx_ray_trace)
  c->lastTraceSmall = c->forcePlacement >= 0 ? c->forcePlacement == 1 : (sliceShift > 0u || c->lastFrameRays < RT_WIDE_RAYS);
  const bool adaptive = splitWork != 0u && sliceShift == 0u;
  // the split list is sized from the demand of an earlier frame (copied back asynchronously, like the ray counters)
  const uint32_t splitCap = !adaptive ? 0u : c->splitCapForced != 0xFFFFFFFFu ? c->splitCapForced
                          : c->splitDemand == 0u ? 0u : ((c->splitDemand + c->splitDemand / 8u + 64u + 31u) / 32u) * 32u;
  G.binWork = adaptive ? c->binWork : nullptr; G.splitList = set.splitList; G.splitCount = set.splitCount;
  G.frontWork = RT_SPLIT_FRONT < splitWork ? RT_SPLIT_FRONT : splitWork;
  G.splitWork = splitWork; G.splitMaxShift = splitMaxShift < 3u ? splitMaxShift : 3u; G.splitCap = splitCap < RT_SPLIT_CAP ? splitCap : RT_SPLIT_CAP;
  // still sky (rt_sky_chain.h rayGeneration; what else ends the runs: SkyBreak): the decision selects skyEpoch and skyPrevRun.  The runs are
  // kept either way; with rtggx_debug_static_sky(ctx, 0) no run is ever long enough
  { SkyChain::GenFacts now;
    now.frame = c->frameCounter; now.rows[0] = rb; now.rows[1] = re; now.rate = c->rayRate; now.sliceShift = sliceShift; now.tilesX = tilesX; now.tilesY = tilesY;
    now.adaptive = adaptive; now.stream = sGen;
    memcpy(now.camera, fp.rg.ProjToWorld, 64); memcpy(now.camera + 16, fp.rg.EyePt, 16);
    G.skyEpoch = c->sky.rayGeneration(now); }
  if (c->sky.takeWrapped()) { const int r = clearSkyWordsAfterWrap(c); if (r) return r; }
  G.skyPrev = c->prev().skyRun; G.skyOut = set.skyRun; G.skyPrevRun = c->sky.prevRunThreshold(RT_SKY_PREV_RUN, RT_SKY_RUN_CAP);
  // ray generation on stream C, the traversal on stream B behind it: the event rides on ray generation
  FrameEvents& ev = c->frameEvents(c->frameCounter);
  // N > 1 samples per pixel: the samples' copies of the frame constants (sampleParamsKernel), and ray generation traces sample 0
  const FrameParams* genParams = c->dParams + c->slot;
  if (c->samples > 1u) {
    FrameParams* const sp = c->sppParams + (size_t)c->slot * RTGGX_MAX_SAMPLES_PER_PIXEL;
    hipLaunchKernelGGL(sampleParamsKernel, dim3(1), dim3(256), 0, sGen, genParams, sp, c->samples);
    genParams = sp;
  }
  const bool wide = c->sampleSet > RTGGX_MIN_SAMPLE_SET;      // rtggx_set_sample_set: the kernels that take a sample in their set-size-aware variant
  launch(wide ? (quad ? rayGenKernel<4, true> : rayGenKernel<1, true>) : quad ? rayGenKernel<4> : rayGenKernel<1>, dim3(quad ? numBins : G.numTiles), dim3(256), sGen, nullptr, sGen != s ? ev.gen : nullptr, genParams, G);
  ev.genFrame = 0u; ev.genStream = sGen;
  if (sGen != s) {
    RT_HIP(hipStreamWaitEvent(s, ev.gen, 0));
    ev.genFrame = c->frameCounter;      // (the event exists: a visibility pass on another stream two frames on waits for it)
  }
  if (c->timing) hipEventRecord(c->tev[11], s);
  const bool ring = c->kernelRing && c->kevCount < c->kevBegin.size() && (c->ringTick++ % c->ringStride) == 0u;
  // a sampled frame: the event pair of the kernel ring rides on the dispatch (and `done` is recorded behind it)
  const TraceQueue q{G.rays, G.hits, G.binCount, G.binSlots, nullptr};
  c->traceGrid[0] = numBins; c->traceGrid[1] = quad ? quadX : tilesX; c->traceGrid[2] = quad ? quadY : tilesY; c->traceGrid[3] = sliceShift;      // (the later levels' launches: launchShade)
  { const int r = launchTrace(c, fp, s, q, numBins, true, quad ? quadX : tilesX, quad ? quadY : tilesY, sliceShift, adaptive ? (int)G.splitCap : -1,
                              ring ? c->kevBegin[c->kevCount] : nullptr, ring ? c->kevEnd[c->kevCount] : done); if (r) return r; }
  if (c->timing) hipEventRecord(c->tev[12], s);
  if (ring) ++c->kevCount;
  if (done && ring) hipEventRecord(done, s);
  RT_HIP(hipGetLastError());
  return 0;
}

// The shading of the frame's traced bins: at recursion depth D (rtggx_set_max_recursion_depth) D passes, each but the last spawning the next
// level's rays into the bins they shade and tracing them with the trace kernel on this stream (ShadePass).  `done` rides on the last pass.
static void (*const kShade[3][2])(const FrameParams*, ShadeArgs) = {      // [ShadePass][rate 4]
    {shadeKernel<1, SHADE_FINAL>, shadeKernel<4, SHADE_FINAL>}, {shadeKernel<1, SHADE_SPAWN>, shadeKernel<4, SHADE_SPAWN>},
    {shadeKernel<1, SHADE_FINAL_DEEP>, shadeKernel<4, SHADE_FINAL_DEEP>}};
static void (*const kShadeSpawnWide[2])(const FrameParams*, ShadeArgs) = {shadeKernel<1, SHADE_SPAWN, true>, shadeKernel<4, SHADE_SPAWN, true>};      // sample-set size > 256
// N > 1 samples per pixel (rate 1 only), depth D: per sample D shading passes that add to the sums, in front of every sample but the first
// its rays' generation and their traversal, behind the last one the resolve -- N * D shading passes, N * D - 1 traversals, N - 1 sample
// generations and the resolve on this stream, the frame's bins reused in place throughout.  Every traversal here is a later level's in launchTrace's terms: a spill part of its
// own, no stamps, no cost record, no split list, no counter read-back -- nothing the next frame's level-0 traversal (stream B) also uses.
// `done` rides on the resolve, the last kernel of the frame that reads the bins.
static int launchShadeSamples(rtggx_context* c, const FrameParams& fp, hipStream_t s, hipEvent_t done, ShadeArgs S, uint32_t numTiles, int spillPart) {
  const uint32_t N = c->samples, depth = c->maxDepth;
  const bool wide = c->sampleSet > RTGGX_MIN_SAMPLE_SET;
  if (!c->sppAcc || !c->sppParams) { setError("rtggx_ray_trace: %u samples per pixel without their buffers", N); return -1; }
  // the sums exist once: the previous frame's passes may have run on another stream (small launches alternate two; frame.hip rtggx_ray_trace)
  if (c->sppStream && c->sppStream != s) { RT_HIP(hipEventRecord(c->evSpp, c->sppStream)); RT_HIP(hipStreamWaitEvent(s, c->evSpp, 0)); }
  c->sppStream = s;
  const InputSet& set = c->cur();
  const FrameParams* const sp = c->sppParams + (size_t)c->slot * RTGGX_MAX_SAMPLES_PER_PIXEL;
  S.accRefl = c->sppAcc; S.accDiff = c->sppAcc + 3u * (size_t)c->W * c->H;
  SampleGenArgs G;
  G.visDepth = S.visDepth; G.fat0 = S.fat0; G.fat1 = S.fat1; G.cosSin = S.cosSin;
  G.rays = S.spawnRays; G.hits = S.spawnHits; G.binCount = S.spawnCount; G.binSlots = S.binSlots;
  G.tileWords = S.tileWords; G.tilesX = S.tilesX; G.rowBegin = S.rowBegin; G.rowEnd = S.rowEnd;
  // rtggx_set_sample_map: the frame's map (whole frames only: this pass's tiles are the frame's) selects the MAPPED variants of the sample
  // generation and of the resolve; the launches stay the N-sample frame's, the traversals and shading passes simply find fewer rays
  const uint32_t* const map = c->sampleMapWords();
  if (map && (S.rowBegin != 0u || S.rowEnd != c->H)) { setError("rtggx_ray_trace: a sample map on rows [%u,%u) of %u", S.rowBegin, S.rowEnd, c->H); return -1; }
  SampleGenArgsMapped GM;
  static_cast<SampleGenArgs&>(GM) = G; GM.sampleMap = map; GM.sample = 0u;
  const TraceQueue q{S.rays, S.spawnHits, S.binCount, S.binSlots, nullptr};
  // rtggx_set_sun_reflections: at every level acc = acc + s_d comes first, then the pass's own add of the paths that end there
  // rtggx_set_light_reflections: then the lights' terms, i ascending, still in front of the pass's own add
  const bool sunHits = c->sun.on && c->sunReflections, lightHits = (c->lights.count > 0u || c->lightList.count > 0u) && c->lightReflections;
  if (sunHits || lightHits) { const int r = beginSunHits(c, s, false, sunHits, lightHits); if (r) return r; }
  for (uint32_t k = 0; k < N; ++k) {
    for (uint32_t level = 0; level < depth; ++level) {
      if (k > 0 && level == 0) {
        if (map) { GM.sample = k; launch(wide ? sampleGenKernel<true, true> : sampleGenKernel<false, true>, dim3(numTiles), dim3(256), s, nullptr, nullptr, sp + k, GM); }
        else launch(wide ? sampleGenKernel<true> : sampleGenKernel<false>, dim3(numTiles), dim3(256), s, nullptr, nullptr, sp + k, G);
      }
      if (k > 0 || level > 0) {
        const int r = launchTrace(c, fp, s, q, c->traceGrid[0], true, c->traceGrid[1], c->traceGrid[2], c->traceGrid[3], -1, nullptr, nullptr, spillPart);
        if (r) return r;
      }
      const HitPass hp{s, q, S.fat0, S.fat1, S.tileWords, numTiles, spillPart, true, S.accRefl, S.accDiff, fp.g.FrameIndex * N + k, level};
      if (sunHits) { const int r = launchSunHits(c, fp, hp); if (r) return r; }
      if (lightHits) { const int r = launchLightHits(c, fp, hp); if (r) return r; }
      launch(level + 1u < depth ? (wide ? shadeKernel<1, SHADE_SPAWN_ACCUM, true> : shadeKernel<1, SHADE_SPAWN_ACCUM>) : shadeKernel<1, SHADE_ACCUM>, dim3(numTiles), dim3(256), s, nullptr, nullptr, sp + k, S);
      S.carryMask = 0u;      // (carried over once, by the first pass)
      RT_HIP(hipGetLastError());
    }
  }
  ResolveArgs R;
  R.visDepth = S.visDepth; R.accRefl = S.accRefl; R.accDiff = S.accDiff; R.reflOut = set.rtRefl; R.diffOut = set.rtDiff;
  R.tileWords = S.tileWords; R.tilesX = S.tilesX; R.rowBegin = S.rowBegin; R.rowEnd = S.rowEnd;
  R.diffMask = (fp.mat.RoughMetals[0][1] < 1.0f ? 1u : 0u) | (fp.mat.RoughMetals[1][1] < 1.0f ? 2u : 0u);      // rghMtl.y < 1 (:559) is the instance's constant
  R.scale = 1.0f / (float)N;
  if (map) {
    ResolveArgsMapped RM;
    static_cast<ResolveArgs&>(RM) = R; RM.sampleMap = reinterpret_cast<const uint8_t*>(map); RM.samples = N;
    launch(resolveSamplesKernel<true>, dim3(numTiles), dim3(256), s, nullptr, done, c->dParams + c->slot, RM);
  } else launch(resolveSamplesKernel<false>, dim3(numTiles), dim3(256), s, nullptr, done, c->dParams + c->slot, R);
  RT_HIP(hipGetLastError());
  return 0;
}
int launchShade(rtggx_context* c, const FrameParams& fp, hipStream_t s, hipEvent_t done) {
  uint32_t rb, re;
  passRows(fp, ROWS_GBUFFER, rb, re);
  if (re <= rb) return 0;
  const uint32_t tilesX = (fp.W + 15) / 16, numTiles = tilesX * ((re - rb + 15) / 16);
  const InputSet& set = c->cur();
  ShadeArgs S;
  S.diffPrev = c->prev().rtDiff; S.visDepth = c->curVis().depth; S.tilesX = tilesX; S.rowBegin = rb; S.rowEnd = re;
  S.carryMask = (fp.mat.RoughMetals[0][1] >= 1.0f ? 1u : 0u) | (fp.mat.RoughMetals[1][1] >= 1.0f ? 2u : 0u);      // rghMtl.y < 1 is the test of :559; it is the instance's constant
  // ... unless ray generation has carried those pixels over already.  It can when the previous frame's shading kernel wrote nothing
  // into the previous set's image (no diffuse rays, no carrying): that image was final when the previous ray generation ended, earlier
  // on the same stream.  The steady state of an all-metal scene: 8 bytes per covered pixel less (this loop reads the visibility word
  // again), and no dependency between the shading kernels of consecutive frames (frame.hip rtggx_ray_trace).
  if (c->genCarriesDiff) S.carryMask = 0u;
  S.tileWords = c->tileWords(rb, re);
  const bool quad = c->rayRate == 4u;      // (rate 4: 32x32 tiles, and RayTracingOut1 is carried over by launchReconstruct)
  const uint32_t grid = quad ? ((tilesX + 1u) / 2u) * ((re - rb + 31u) / 32u) : numTiles;
  if (quad) S.carryMask = 0u;
  S.rays = (const RayRec*)set.rayQueue.get(); S.hits = (const HitKey*)set.hitQueue.get(); S.binCount = set.binCount; S.binSlots = c->binSlots;
  S.fat0 = c->mesh[0].fat; S.fat1 = c->mesh[1].fat;
  S.env = c->env.texels; S.envMipOffset = c->dEnvMipOffset; S.envSize = c->env.size; S.envMips = c->env.mips; S.sh = c->sh;
  S.reflOut = set.rtRefl; S.diffOut = set.rtDiff;
  S.spawnRays = (RayRec*)set.rayQueue.get(); S.spawnHits = (HitKey*)set.hitQueue.get(); S.spawnCount = set.binCount; S.cosSin = c->sampleTable();
  S.accRefl = nullptr; S.accDiff = nullptr;
  const FrameParams* const dfp = c->dParams + c->slot;
  const uint32_t depth = c->maxDepth;
  // Levels 1.. run behind this stream's shading of the level before, beside the next frame's level-0 traversal (stream B): a part of the
  // spill area of their own on the main stream; on a traversal stream (small launches, frame.hip) that stream's own, in stream order
  const int spillPart = s == c->streamMain ? 2 : (int)c->traceSpillHalf;
  if (c->samples > 1u && !quad) return launchShadeSamples(c, fp, s, done, S, numTiles, spillPart);
  // rtggx_set_sun_reflections (the sun excludes rate 4): every level's hits add their terms to S in front of the level's shading pass, and
  // behind the last pass -- which then no longer carries `done` -- sunHitResolveKernel adds S to the packed words
  // rtggx_set_light_reflections (the lights exclude rate 4 as well): the lights' terms follow the sun's into the same S, i ascending, and
  // the one resolve packs what either feature left there
  const bool sunHits = c->sun.on && c->sunReflections && !quad, lightHits = (c->lights.count > 0u || c->lightList.count > 0u) && c->lightReflections && !quad, anyHits = sunHits || lightHits;
  float* sums[2] = {nullptr, nullptr};
  if (anyHits) {
    const int r = beginSunHits(c, s, true, sunHits, lightHits); if (r) return r;
    sums[0] = c->sunHitSums; sums[1] = c->sunHitSums + 4u * (size_t)c->W * c->H;
  }
  for (uint32_t level = 0; level < depth; ++level) {
    const TraceQueue q{S.rays, S.spawnHits, S.binCount, S.binSlots, nullptr};
    if (level > 0) {
      const int r = launchTrace(c, fp, s, q, c->traceGrid[0], true, c->traceGrid[1], c->traceGrid[2], c->traceGrid[3], -1, nullptr, nullptr, spillPart);
      if (r) return r;
      S.carryMask = 0u;      // (carried over once, by the first pass)
    }
    const HitPass hp{s, q, S.fat0, S.fat1, S.tileWords, numTiles, spillPart, false, sums[0], sums[1], fp.g.FrameIndex, level};
    if (sunHits) { const int r = launchSunHits(c, fp, hp); if (r) return r; }
    if (lightHits) { const int r = launchLightHits(c, fp, hp); if (r) return r; }
    const int pass = level + 1u < depth ? SHADE_SPAWN : level == 0 ? SHADE_FINAL : SHADE_FINAL_DEEP;
    launch(pass == SHADE_SPAWN && c->sampleSet > RTGGX_MIN_SAMPLE_SET ? kShadeSpawnWide[quad] : kShade[pass][quad], dim3(grid), dim3(256), s, nullptr, pass == SHADE_SPAWN || anyHits ? nullptr : done, dfp, S);
    RT_HIP(hipGetLastError());
  }
  if (anyHits) return launchSunHitResolve(c, s, c->sunHitSums, S.tileWords, tilesX, rb, re, done);
  return 0;
}

int launchReconstruct(rtggx_context* c, const FrameParams& fp, hipStream_t s) {
  uint32_t rb, re;
  passRows(fp, ROWS_GBUFFER, rb, re);
  if (re <= rb) return 0;
  const uint32_t tilesX = (fp.W + 15) / 16, numTiles = tilesX * ((re - rb + 15) / 16);
  const InputSet& set = c->cur();
  ReconArgs R;
  R.visDepth = c->curVis().depth; R.normal = set.normal; R.roughMetal = set.roughMetal; R.depth32 = set.depth32;
  R.reflOut = set.rtRefl; R.diffOut = set.rtDiff;
  R.diffPrev = c->prev().rtDiff;
  const uint32_t metal = (fp.mat.RoughMetals[0][1] >= 1.0f ? 1u : 0u) | (fp.mat.RoughMetals[1][1] >= 1.0f ? 2u : 0u);      // as launchShade's carryMask
  R.carryMask = c->genCarriesDiff ? 0u : metal; R.diffMask = ~metal & 3u;
  R.tileWords = c->tileWords(rb, re); R.tilesX = tilesX; R.rowBegin = rb; R.rowEnd = re;
  hipLaunchKernelGGL(reconstructKernel, dim3(numTiles), dim3(256), 0, s, c->dParams + c->slot, R);
  RT_HIP(hipGetLastError());
  return 0;
}

// ---- test entry: closest-hit queries for an explicit ray list (through the same trace kernel) ---------------
__global__ void fillTestQueue(const float* __restrict__ rays, uint32_t n, uint32_t binSlots, RayRec* q0, HitKey* keys, uint32_t* binCount, float2* tRange) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i % binSlots == 0 && i < n) binCount[i / binSlots] = n - i < binSlots ? n - i : binSlots;   // bins are filled densely, in order
  if (i >= n) return;
  const float* r = rays + 8 * (size_t)i;
  RayRec rr;
  rr.ox = r[0]; rr.oy = r[1]; rr.oz = r[2]; rr.dx = r[3]; rr.dy = r[4]; rr.dz = r[5];
  rr.pixel = 0u; rr.skip = 0xFFFFFFFFu; rr.flags = 0u; rr.wx = rr.wy = rr.wz = 0.0f;
  q0[i] = rr;
  tRange[i] = make_float2(r[6], r[7]);      // these rays bring their own interval
  keys[i] = hitKey(r[7], 0xFFFFFFFFu);
}
__global__ void exportTestHits(const FrameParams* __restrict__ fpp, const RayRec* __restrict__ rays, const HitKey* __restrict__ hits, uint32_t n,
                               const float4* __restrict__ fat0, const float4* __restrict__ fat1, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const HitKey k = hits[i];
  const uint32_t id = hitKeyId(k);
  float* o = out + 6 * (size_t)i;
  const bool valid = id != 0xFFFFFFFFu;
  float t = hitKeyT(k), b1 = 0.0f, b2 = 0.0f;
  if (valid) {
    const RayRec rr = rays[i];
    const uint32_t inst = id >> 24;
    uint32_t prim = id & 0xFFFFFFu;
    // (same compiler hazard as in shadeKernel: keep the mask behind a barrier)
    asm volatile("" : "+v"(prim));
    const Tri3 v = getVertices(inst ? fat1 : fat0, prim);
    woopTestVerts(toObject(rr.ox, rr.oy, rr.oz, rr.dx, rr.dy, rr.dz, inst ? fpp->invWorld[1] : fpp->invWorld[0]), v.pos[0], v.pos[1], v.pos[2], t, b1, b2);
  }
  o[0] = t; o[1] = u2f(valid ? id >> 24 : 0u); o[2] = u2f(valid ? id & 0xFFFFFFu : 0u); o[3] = b1; o[4] = b2; o[5] = valid ? 1.0f : 0.0f;
}
int launchTraceRays(rtggx_context* c, const FrameParams& fp, const float* dRays, uint32_t n, float* dOut, hipStream_t s) {
  if (!n) return 0;
  if (n > c->numBinsMax * c->binSlots) { setError("rtggx_trace_rays: at most %u rays per launch", c->numBinsMax * c->binSlots); return -1; }
  const uint32_t numBins = (((n + c->binSlots - 1u) / c->binSlots) + 3u) & ~3u;   // whole tiles of four bins
  const InputSet& set = c->cur();
  RT_HIP(hipMemsetAsync(set.binCount, 0, (size_t)numBins * 4, s));
  // the rays' own (TMin, TMax): one float2 per slot, kept for the context's lifetime once a caller has used this entry point
  if (!c->testRayRange) RT_HIP(alloc(c->testRayRange, (size_t)c->numBinsMax * RT_BIN * sizeof(float2)));
  hipLaunchKernelGGL(fillTestQueue, dim3((n + 255) / 256), dim3(256), 0, s, dRays, n, c->binSlots, (RayRec*)set.rayQueue.get(), (HitKey*)set.hitQueue.get(), set.binCount, (float2*)c->testRayRange.get());
  const TraceQueue q{(const RayRec*)set.rayQueue.get(), (HitKey*)set.hitQueue.get(), set.binCount, c->binSlots, (const float2*)c->testRayRange.get()};
  { const int r = launchTrace(c, fp, s, q, numBins, false, 0u, 0u, chooseSliceShift(c, false, numBins), -1); if (r) return r; }
  hipLaunchKernelGGL(exportTestHits, dim3((n + 255) / 256), dim3(256), 0, s, c->dParams + c->slot, (const RayRec*)set.rayQueue.get(), (const HitKey*)set.hitQueue.get(), n,
                     (const float4*)c->mesh[0].fat, (const float4*)c->mesh[1].fat, dOut);
  RT_HIP(hipGetLastError());
  return 0;
}

// ---- occlusion queries for an explicit ray list (rtggx_trace_occlusion): the same list path, through the any-hit variant of the trace kernel ----
__global__ void exportOcclusion(const HitKey* __restrict__ hits, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = hitKeyId(hits[i]) != 0xFFFFFFFFu ? 1u : 0u;      // which triangle an occluded ray's key names is unspecified (rt_queue.h): only this bit leaves
}
int launchTraceOcclusion(rtggx_context* c, const FrameParams& fp, const float* dRays, uint32_t n, uint32_t* dOut, hipStream_t s) {
  if (!n) return 0;
  if (n > c->numBinsMax * c->binSlots) { setError("rtggx_trace_occlusion: at most %u rays per launch", c->numBinsMax * c->binSlots); return -1; }
  const uint32_t numBins = (((n + c->binSlots - 1u) / c->binSlots) + 3u) & ~3u;   // whole tiles of four bins
  const InputSet& set = c->cur();
  RT_HIP(hipMemsetAsync(set.binCount, 0, (size_t)numBins * 4, s));
  if (!c->testRayRange) RT_HIP(alloc(c->testRayRange, (size_t)c->numBinsMax * RT_BIN * sizeof(float2)));
  hipLaunchKernelGGL(fillTestQueue, dim3((n + 255) / 256), dim3(256), 0, s, dRays, n, c->binSlots, (RayRec*)set.rayQueue.get(), (HitKey*)set.hitQueue.get(), set.binCount, (float2*)c->testRayRange.get());
  const TraceQueue q{(const RayRec*)set.rayQueue.get(), (HitKey*)set.hitQueue.get(), set.binCount, c->binSlots, (const float2*)c->testRayRange.get()};
  { const int r = launchTrace(c, fp, s, q, numBins, false, 0u, 0u, chooseSliceShift(c, false, numBins), -1, nullptr, nullptr, -1, true); if (r) return r; }
  hipLaunchKernelGGL(exportOcclusion, dim3((n + 255) / 256), dim3(256), 0, s, (const HitKey*)set.hitQueue.get(), n, dOut);
  RT_HIP(hipGetLastError());
  return 0;
}

// ---- test entry: the environment sampler alone (the frame kernels' own device functions, one lane per direction) ------
__global__ void debugEnvironmentKernel(EnvRef env, const float* __restrict__ dirs, const float* __restrict__ levels, uint32_t n, int level0, float* __restrict__ rgb) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f3 d = mk3(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]);
  const f3 c = level0 ? environmentLevel0(env, d) : environment(env, d, levels[i]);
  rgb[3 * (size_t)i] = c.x; rgb[3 * (size_t)i + 1] = c.y; rgb[3 * (size_t)i + 2] = c.z;
}
int launchDebugEnvironment(rtggx_context* c, const float* dDirs, const float* dLevels, uint32_t n, int level0, float* dOut, hipStream_t s) {
  const EnvRef env{c->env.texels, c->env.size, c->env.mips, c->dEnvMipOffset};
  hipLaunchKernelGGL(debugEnvironmentKernel, dim3((n + 255) / 256), dim3(256), 0, s, env, dDirs, dLevels, n, level0, dOut);
  RT_HIP(hipGetLastError());
  return 0;
}

// ---- GGX-prefiltered environments (rtggx_prefilter_env; include/rtggx.h, DESIGN.md "Prefiltered environments") --------------------
// One level of the new cube from the box-chain cube `src`: one wave per destination texel, four waves per workgroup.  Lane j owns the
// table entries j, j + 64, ... -- one 16-byte load per lane and step, 1 KB contiguous per wave -- and adds its terms in that order;
// the 64 partial sums meet in a butterfly over lane ^ 1, ^ 2, ... ^ 32, which is the contract's adjacent-first pairwise tree (a + b is
// commutative) and needs no LDS.  The taps are the frame's own sampler, called as the frame calls it: eight 8-byte gathers and the offset
// word each, four of them in flight at a time, from a cube whose coarse levels sit in L2 -- latency, not bandwidth, so the kernel stays
// below 64 VGPRs (57 with the callee) and eight waves per SIMD hide it.  (Two entries per lane in flight through an inlined copy of the
// sampler: 1-3 % off the call at N = 4096, nothing below, seven times the code; not kept -- DESIGN.md.)  A lane without an entry holds
// +0.  No atomics: the texel is a pure function of the cube and the table.
struct EnvFilterArgs {
  EnvRef src;                            // level 0 and the full box chain (its own offset table)
  const float4* __restrict__ table;      // K x (x, y, z, lod): rt_env_filter.h
  uint2* __restrict__ dst;               // the level's texels in the new cube
  uint32_t K, side;
  float invW;
};
__global__ void __launch_bounds__(256, 8) envPrefilterKernel(EnvFilterArgs A) {
  const size_t texel = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6), perFace = (size_t)A.side * A.side;
  if (texel >= 6u * perFace) return;      // (whole waves: the guard is wave-uniform)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t face = (uint32_t)(texel / perFace), rem = (uint32_t)(texel % perFace), y = rem / A.side, x = rem % A.side;
  const float u = ((float)x + 0.5f) / (float)A.side * 2.0f - 1.0f, v = ((float)y + 0.5f) / (float)A.side * 2.0f - 1.0f;
  const f3 R = normalize3(cubeFaceDir((int)face, u, v));
  f3 sum = mk3(0.0f, 0.0f, 0.0f);
  for (uint32_t k = lane; k < A.K; k += 64u) {
    const float4 e = A.table[k];
    const f3 c = environment(A.src, localToWorld(R, mk3(e.x, e.y, e.z)), e.w);
    sum = sum + c * e.z;
  }
  for (int d = 1; d < 64; d <<= 1) sum = sum + mk3(__shfl_xor(sum.x, d), __shfl_xor(sum.y, d), __shfl_xor(sum.z, d));
  if (lane == 0u) A.dst[texel] = packRGBA16F(fminf(sum.x * A.invW, 65504.0f), fminf(sum.y * A.invW, 65504.0f), fminf(sum.z * A.invW, 65504.0f), 1.0f);
}
int launchEnvPrefilter(const uint2* srcTexels, uint32_t size, uint32_t mips, const uint32_t* dSrcMipOffset, const float4* dTable, uint32_t K, float invW,
                       uint32_t side, uint2* dst, hipStream_t s) {
  EnvFilterArgs A;
  A.src = EnvRef{srcTexels, size, mips, dSrcMipOffset};
  A.table = dTable; A.dst = dst; A.K = K; A.side = side; A.invW = invW;
  const size_t waves = 6u * (size_t)side * side;
  hipLaunchKernelGGL(envPrefilterKernel, dim3((uint32_t)((waves + 3u) / 4u)), dim3(256), 0, s, A);
  RT_HIP(hipGetLastError());
  return 0;
}

// ---- progressive accumulation (rtggx_set_accumulation; include/rtggx.h, DESIGN.md "Progressive accumulation") ---------------------
// The frame's two traced images added to the running sums: one lane per pixel of the strip's own rows -- whole rows, so the pixels are
// one contiguous range [first, first + count) of every image --, a streaming pass of 8 + 4 (+ 4) bytes read and 16 (+ 16) read and
// written per pixel.  It visits every pixel and asks no tile word: a sky tile holds its environment words in every input set, whoever
// wrote them (ray generation this frame, or an earlier one where a still sky was left alone).  The diffuse image is added where a diffuse
// path wrote it this frame: a covered pixel whose instance's metallic is below 1 (diffMask, bit per instance: resolveSamplesKernel's rule).
// fp32, every operation rounded on its own (no contraction), the order of the sum is the order of the launches on the stream.
struct AccumArgs {
  const unsigned long long* visDepth; const uint32_t* refl; const uint32_t* diff; float4* accRefl; float4* accDiff;
  uint32_t first, count, diffMask;
};
RT_DEV float4 accumulateWord(float4 a, uint32_t word) {
#pragma clang fp contract(off)
  const f3 c = unpackR11G11B10F(word);
  const float y = (0.25f * c.x + 0.5f * c.y) + 0.25f * c.z;      // the luma of the temporal pass's YCoCg
  return make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + y * y);
}
__global__ void __launch_bounds__(256) accumulateKernel(AccumArgs A) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= A.count) return;
  const size_t pix = (size_t)A.first + i;
  const uint32_t vis = (uint32_t)A.visDepth[pix];
  A.accRefl[pix] = accumulateWord(A.accRefl[pix], A.refl[pix]);
  const uint32_t inst = (vis - 1u) >> 24;      // (two instances: an uploaded word that names another has no material)
  if (vis != 0u && inst < 2u && ((A.diffMask >> inst) & 1u)) A.accDiff[pix] = accumulateWord(A.accDiff[pix], A.diff[pix]);
}
int launchAccumulate(rtggx_context* c, const FrameParams& fp, hipStream_t s) {
  if (!c->accRefl || !c->accDiff) { setError("rtggx_ray_trace: accumulation without its buffers"); return -1; }
  if (fp.rowEnd <= fp.rowBegin) return 0;
  const InputSet& set = c->cur();
  AccumArgs A;
  A.visDepth = c->curVis().depth; A.refl = set.rtRefl; A.diff = set.rtDiff; A.accRefl = c->accRefl; A.accDiff = c->accDiff;
  A.first = fp.rowBegin * fp.W; A.count = (fp.rowEnd - fp.rowBegin) * fp.W;
  A.diffMask = (fp.mat.RoughMetals[0][1] < 1.0f ? 1u : 0u) | (fp.mat.RoughMetals[1][1] < 1.0f ? 2u : 0u);
  hipLaunchKernelGGL(accumulateKernel, dim3((A.count + 255u) / 256u), dim3(256), 0, s, A);
  RT_HIP(hipGetLastError());
  return 0;
}

// The mean image of rtggx_present_accumulation: per component (float)((double)sum / (double)n) of each image, the two means added in
// fp32 -- the denoiser's composition dest + diffuse (denoise.hip spatialTiledKernel<3>); A1 is zero where no diffuse path contributed.
__global__ void __launch_bounds__(256) presentAccumulationKernel(const float4* __restrict__ accRefl, const float4* __restrict__ accDiff, uint2* __restrict__ out, uint32_t count, uint32_t frames) {
#pragma clang fp contract(off)
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  const double n = (double)frames;
  const float4 a = accRefl[i], d = accDiff[i];
  const float r = (float)((double)a.x / n) + (float)((double)d.x / n);
  const float g = (float)((double)a.y / n) + (float)((double)d.y / n);
  const float b = (float)((double)a.z / n) + (float)((double)d.z / n);
  out[i] = packRGBA16F(r, g, b, 1.0f);
}
int launchPresentAccumulation(rtggx_context* c, hipStream_t s) {
  const uint32_t count = c->W * c->H;
  hipLaunchKernelGGL(presentAccumulationKernel, dim3((count + 255u) / 256u), dim3(256), 0, s, (const float4*)c->accRefl, (const float4*)c->accDiff, c->converged, count, c->accumFrames);
  RT_HIP(hipGetLastError());
  return 0;
}

}  // namespace rt
