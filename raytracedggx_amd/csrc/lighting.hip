// Direct lighting: the sun (rtggx_set_sun, rtggx_set_sun_angle), the local lights (rtggx_set_lights) and both at the surfaces the paths hit
// (rtggx_set_sun_reflections, rtggx_set_light_reflections); one shadow ray for all lights (rtggx_set_light_sampling: the two picking kernels
// further down, with a table of their own; rtggx_set_light_pick_visibility: the primary pair of them once more, with a record per pixel);
// a list of up to 1024 lights in device memory, culled per block (rtggx_set_light_list: the last pair of generating kernels; its primary
// kernel once more with a sparse record per pixel: rtggx_set_light_list_visibility).
// include/rtggx.h has the per-pixel rules, DESIGN.md section 9 the structure.
//
// Every pass is the same three launches around a queue of its own (rt::ShadowQueue, rt_queue.h): a generating kernel derives a surface --
// the primary one from the visibility word, or the hit of a traced ray -- and, where a light reaches it, compacts ONE shadow ray into the
// wave's bin, with the finished term in the record; the any-hit traversal (trace.hip) leaves an unoccluded ray's key a miss; an adding
// kernel, one lane per slot, adds the unoccluded terms.  No two lanes meet at a pixel and nothing is atomic: the order of a sum is the order
// of the launches on the stream.
//
//   the step, written once below           who runs it
//   tileIsEmpty                            every kernel here
//   atPrimarySurface                       sunGenKernel, lightGenKernel
//   atTracedHit, hitLobeTerm               sunHitGenKernel, lightHitGenKernel
//   deltaLightSpecular                     all four
//   shadowSample + the slot numbering      the SOFT variants of all four
//   evalLight                              lightGenKernel, lightHitGenKernel
//   compactShadowRay                       all four
//
// SOFT and CONE are compile-time: a directional sun, and a context with point lights of radius 0, pay for neither the hash nor the cone.
#include <type_traits>
#include <cstring>
#include "capi_internal.h"
#include "rt_queue.h"
#include "rt_traverse.h"
#include "rt_surface.h"
#include "rt_light_check.h"

namespace rt {

// The guard of every kernel here: one word per 16x16 tile (rtggx_context::tileWords), 0 = nothing drawn there; a scalar load and its own
// wait, so that an empty workgroup leaves before it has touched a vector register.
RT_DEV bool tileIsEmpty(const uint32_t* tileWords, uint32_t tile) {
  uint32_t word;
  asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(word) : "s"(tileWords), "s"(tile * 4u) : "memory");
  return word == 0u;
}

struct Surface { f3 P, N, V, color; f2 rm; };      // rm: (roughness, metallic)

// Step 1 of rtggx_set_sun, step 0 of rtggx_set_lights: the primary surface from the visibility word -- getPrimarySurface :277-333, the covered
// branch, ray generation's arithmetic.  Where a surface covers the pixel, lit(surface) runs -- inside the branch that found it, so that a
// kernel's control flow is the one of the steps written out.  pixel: the full-frame index y W + x.
struct PrimarySurface : Surface { uint32_t pixel, inst, prim; };
template <class Lit>
RT_DEV void atPrimarySurface(const FrameParams& fp, const unsigned long long* visDepth, const float4* fat0, const float4* fat1, uint32_t px, uint32_t py, Lit lit) {
  const uint32_t W = fp.W, H = fp.H;
  const size_t pix = (size_t)py * W + px;
  uint32_t visibility = (uint32_t)visDepth[pix];
  if (visibility == 0) return;
  --visibility;
  const uint32_t inst = visibility >> 24;
  uint32_t prim = visibility & 0xFFFFFFu;
  asm volatile("" : "+v"(prim));      // see shadeKernel
  f2 screenPos; screenPos.x = ((float)px + 0.5f) / (float)W * 2.0f - 1.0f; screenPos.y = ((float)py + 0.5f) / (float)H * 2.0f - 1.0f;
  screenPos.y = -screenPos.y;
  const f3 eye = mk3(fp.rg.EyePt[0], fp.rg.EyePt[1], fp.rg.EyePt[2]);
  const Tri3 v = getVertices(inst ? fat1 : fat0, prim);
  const M4 wvp = cbLoad4x4(fp.g.WorldViewProjs[inst]);
  f4 p[3];
  for (int k = 0; k < 3; ++k) p[k] = mulPoint(v.pos[k], wvp);
  screenPos.x -= fp.rg.ProjBias[0]; screenPos.y -= fp.rg.ProjBias[1];
  const f2 bary = calcBarycentrics(p, screenPos);
  const Attrib a = interpAttrib(v, bary.x, bary.y);
  PrimarySurface s;
  s.color = mk3(fp.mat.BaseColors[inst][0], fp.mat.BaseColors[inst][1], fp.mat.BaseColors[inst][2]);
  s.rm = getRoughMetal(fp.mat, inst, a.UV);
  const f4 P4 = mulPoint(a.Pos, cbLoad4x3(fp.g.Worlds[inst]));
  s.P = mk3(P4.x, P4.y, P4.z);
  s.N = normalize3(mulDir(a.Nrm, cbLoad3x3(inst ? fp.g.WorldIT1 : fp.g.WorldITs0)));
  s.V = normalize3(eye - s.P);
  s.pixel = (uint32_t)pix; s.inst = inst; s.prim = prim;
  lit(s);
}

// A traced ray of the frame's bins that TOUCHES A SURFACE (rtggx_set_sun_reflections): it hits, and it is not a reflection-group ray whose
// preset is <= 0 in every component (shadeKernel: :573 returns the preset).  The hit as shadeKernel derives it: triangle from the hit id,
// barycentrics from the repeated watertight test, P = o + t dir (hitWorldPosition :338-341), V = -dir.  image: the image the path writes
// (1: RayTracingOut1); q2.xyz: the throughput T the record carries.  What only a lit hit needs is computed where it is asked for.
// Where the ray touches, lit(hit) runs, inside the branch that found it (atPrimarySurface).
struct TracedHit {
  float4 q0, q1, q2;      // the record's three words
  uint32_t pixel, hitId, image; bool diffuseGroup;
  float t; f3 N; f2 UV;
  RT_DEV f3 P() const { return mk3(q0.x + t * q0.w, q0.y + t * q1.x, q0.z + t * q1.y); }
  RT_DEV f3 V() const { return mk3(-q0.w, -q1.x, -q1.y); }
  RT_DEV f2 rm(const FrameParams& fp) const { return getRoughMetal(fp.mat, hitId >> 24, UV); }
  RT_DEV f3 color(const FrameParams& fp) const { return mk3(fp.mat.BaseColors[hitId >> 24][0], fp.mat.BaseColors[hitId >> 24][1], fp.mat.BaseColors[hitId >> 24][2]); }
};
template <class Lit>
RT_DEV void atTracedHit(const FrameParams& fp, const RayRec* rays, const HitKey* hits, const float4* fat0, const float4* fat1, size_t slot, Lit lit) {
  TracedHit h;
  const float4* rp = reinterpret_cast<const float4*>(rays + slot);
  h.q0 = rp[0]; h.q1 = rp[1]; h.q2 = rp[2];
  const uint32_t skip = __float_as_uint(h.q1.w), flags = __float_as_uint(h.q2.w);
  h.pixel = __float_as_uint(h.q1.z); h.hitId = hitKeyId(hits[slot]);
  h.diffuseGroup = (flags & 1u) != 0u;
  h.image = (flags ^ (flags >> 1)) & 1u;
  const uint32_t srcInst = skip >> 24;
  const float m = fp.mat.RoughMetals[srcInst][1];
  const bool presetReturn = !h.diffuseGroup && fp.mat.BaseColors[srcInst][0] * m <= 0.0f && fp.mat.BaseColors[srcInst][1] * m <= 0.0f && fp.mat.BaseColors[srcInst][2] * m <= 0.0f;
  if (h.hitId == 0xFFFFFFFFu || presetReturn) return;
  const uint32_t hInst = h.hitId >> 24;
  uint32_t hPrim = h.hitId & 0xFFFFFFu;
  asm volatile("" : "+v"(hPrim));      // see shadeKernel
  const Tri3 v = getVertices(hInst ? fat1 : fat0, hPrim);
  float hb1 = 0.0f, hb2 = 0.0f;
  woopTestVerts(toObject(h.q0.x, h.q0.y, h.q0.z, h.q0.w, h.q1.x, h.q1.y, hInst ? fp.invWorld[1] : fp.invWorld[0]), v.pos[0], v.pos[1], v.pos[2], h.t, hb1, hb2);
  const Attrib a = interpAttrib(v, hb1, hb2);
  h.N = normalize3(mulDir(a.Nrm, cbLoad3x3(hInst ? fp.g.WorldIT1 : fp.g.WorldITs0)));
  h.UV = a.UV;
  lit(h);
}

// The specular term under a delta light (step 4 of rtggx_set_sun, step 8 of rtggx_set_lights, the m > 0.5 lobe of the two hit rules):
// F D Vis NoL with the roughness floored at 1/32 -- a mirror under a delta light has no finite answer.  Returns F k, k = (D vis) NoL; the
// caller multiplies by the light's E.
RT_DEV f3 deltaLightSpecular(f3 N, f3 V, f3 L, float NoL, f3 color, f2 rm) {
  const float r = fmaxf(rm.x, 1.0f / 32.0f);
  const f3 Hh = normalize3(V + L);
  const float NoH = saturatef(dot3(N, Hh)), VoH = saturatef(dot3(V, Hh)), NoV = saturatef(dot3(N, V));
  const float al = r * r, a2 = al * al;
  const float d = (NoH * a2 - NoH) * NoH + 1.0f;
  const float D = a2 / ((RT_PI * d) * d);
  const f3 f0 = mk3(lerpf(0.04f, color.x, rm.y), lerpf(0.04f, color.y, rm.y), lerpf(0.04f, color.z, rm.y));
  const f3 F = fSchlick(f0, VoH);
  const float vis = visSmith(r, NoV, NoL);
  const float k = (D * vis) * NoL;
  return mk3(F.x * k, F.y * k, F.z * k);
}
// The diffuse colour of a hit: color (1 - m) for a diffuse-group ray (:607), color for a reflection-group ray
RT_DEV f3 hitDiffuseColor(f3 color, f2 rm, bool diffuseGroup) { return diffuseGroup ? color * (1.0f - rm.y) : color; }
// The term of the lobe the path uses at a hit (step 3 of rtggx_set_sun_reflections, step 4 of rtggx_set_light_reflections) at the centre
// direction L, under the irradiance E att (the sun: att = 1, which multiplies away).  m > 0.5: (F k) (E att); else (color' g) E with
// g = (NoL / pi) att -- no x (1 - 0.04) at depth >= 1 (:532).
RT_DEV f3 hitLobeTerm(const FrameParams& fp, const TracedHit& h, f3 L, float NoL, f3 E, float att) {
  const f2 rm = h.rm(fp);
  const f3 color = h.color(fp);
  if (rm.y > 0.5f) {
    const f3 Fk = deltaLightSpecular(h.N, h.V(), L, NoL, color, rm);
    return mk3(Fk.x * (E.x * att), Fk.y * (E.y * att), Fk.z * (E.z * att));
  }
  const f3 diffuse = hitDiffuseColor(color, rm, h.diffuseGroup);
  const float g = (NoL / RT_PI) * att;
  return mk3((diffuse.x * g) * E.x, (diffuse.y * g) * E.y, (diffuse.z * g) * E.z);
}

// The slots of the soft shadows' hash, all of them (include/rtggx.h): 0 the sun at the primary surface; 1 + 2 d + img the sun at a level-d
// hit of a path that writes image img; 16 + i light i at the primary surface; 32 + 16 d + 8 img + i light i at a level-d hit.  The host
// hands a kernel the slot at img = 0, the kernel adds the image's stride.
#define RT_SLOT_SUN 0u
#define RT_SLOT_SUN_HIT(d) (1u + 2u * (d))
#define RT_SLOT_SUN_HIT_IMAGE 1u
#define RT_SLOT_LIGHT(i) (16u + (i))
#define RT_SLOT_LIGHT_HIT(d, i) (32u + 16u * (d) + (i))
#define RT_SLOT_LIGHT_HIT_IMAGE 8u
// What a soft shadow draws its target from (step 2 of rtggx_set_sun_angle, step 5 of rtggx_set_lights): w = rng(h + j 0x9E3779B9) with
// h = rng(rng(pixel) + frameIndex), getSampleParam's word before its mask; u = the low 16 bits in [0, 1), s = the top 8, an entry of the
// 256-entry cos/sin table whatever the sample set is.  frameIndex: of the sample the pass belongs to.
struct ShadowSample { float u; uint32_t s; };
RT_DEV ShadowSample shadowSample(uint32_t pixel, uint32_t frameIndex, uint32_t j) {
  uint32_t h = rng(pixel); h += frameIndex; h = rng(h);
  const uint32_t w = rng(h + j * 0x9E3779B9u);
  ShadowSample o; o.u = (float)(w & 0xffffu) / 65536.0f; o.s = w >> 24;
  return o;
}

// A shadow ray's record: from P along dir, skipping the triangle it starts on; weight and flags are what the pass's adding kernel reads
RT_DEV RayRec shadowRay(f3 P, f3 dir, uint32_t pixel, uint32_t skip, f3 weight, uint32_t flags) {
  RayRec r;
  r.ox = P.x; r.oy = P.y; r.oz = P.z; r.dx = dir.x; r.dy = dir.y; r.dz = dir.z;
  r.pixel = pixel; r.skip = skip;
  r.wx = weight.x; r.wy = weight.y; r.wz = weight.z;
  r.flags = flags;
  return r;
}
// One shadow ray per wanting lane into the front of the wave's bin, in lane order behind the `written` records of the wave's earlier
// rounds (a single-round kernel: 0, and RT_BIN_MIN slots): the record, the key the traversal starts from -- (tmax, miss) -- and, where
// the queue has them (RANGE), the ray's interval (1e-5, tmax).  Returns how many the wave wrote.
template <bool RANGE>
RT_DEV uint32_t compactShadowRay(bool want, const RayRec& r, float tmax, RayRec* rays, HitKey* hits, float2* range, uint32_t bin, uint32_t binSlots, uint32_t written, uint32_t lane) {
  const unsigned long long mask = __ballot(want);
  if (want) {
    const size_t k = (size_t)bin * binSlots + written + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    rays[k] = r; hits[k] = hitKey(tmax, 0xFFFFFFFFu);
    if constexpr (RANGE) range[k] = make_float2(RT_RAY_TMIN, tmax);
  }
  return (uint32_t)__popcll(mask);
}

// ---- the sun (rtggx_set_sun; DESIGN.md section 9 "Sun and shadow rays") ----------------------------------------------------------------------
// Three kernels on the stream that has this frame's two traced images complete (frame.hip rtggx_ray_trace): sunGenKernel puts the specular
// term in the record's weight and NoL in its flags word; sunAddKernel adds an unoccluded slot's terms to its pixel's packed words (a pixel
// has at most one slot).
#ifndef RT_SUN_CLOSEST
#define RT_SUN_CLOSEST 0      // measurement: 1 traces the shadow queue with the closest-hit kernel (the same images; profiles/r14_d_sun_cost.txt)
#endif
// A sun with a size (rtggx_set_sun_angle): what the SOFT variants of the two generating kernels are given on top of their arguments -- the
// disk's frame, k = 1 - cos(radius), the 256-entry cos/sin table, and (the hits) the frame index of the sample the pass belongs to with the
// level's slot.  SOFT = false is the kernel without any of it, body and arguments.
struct SunDiskArgs { float Tx, Ty, Tz, Bx, By, Bz, k; const float* cosSin; uint32_t frameIndex, slotBase; };
// Steps 1-5 of rtggx_set_sun_angle: the direction toward a point of the disk, uniform in solid angle over the cap; not renormalised.
RT_DEV f3 sunDiskDirection(const SunDiskArgs& K, f3 L, uint32_t pixel, uint32_t frameIndex, uint32_t j) {
  const ShadowSample x = shadowSample(pixel, frameIndex, j);
  const float cosPhi = K.cosSin[x.s], sinPhi = K.cosSin[256u + x.s];
  const float e = x.u * K.k;
  const float cosTheta = 1.0f - e, sinTheta = sqrtf(e * (2.0f - e));      // (not 1 - cos^2: it cancels at small angles)
  const float ct = cosPhi * sinTheta, st = sinPhi * sinTheta;
  return mk3((K.Tx * ct + K.Bx * st) + L.x * cosTheta, (K.Ty * ct + K.By * st) + L.y * cosTheta, (K.Tz * ct + K.Bz * st) + L.z * cosTheta);
}
struct SunGenArgs {
  const unsigned long long* visDepth; const float4* fat0; const float4* fat1;
  RayRec* rays; HitKey* hits; uint32_t* binCount;
  const uint32_t* tileWords; uint32_t tilesX, rowBegin, rowEnd;
  float Lx, Ly, Lz, Ex, Ey, Ez;
};
struct SunGenArgsSoft : SunGenArgs { SunDiskArgs disk; };      // slot RT_SLOT_SUN, the frame's own index (the constants')
template <bool SOFT>
__global__ void __launch_bounds__(256) sunGenKernel(const FrameParams* __restrict__ fpp, std::conditional_t<SOFT, SunGenArgsSoft, SunGenArgs> A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t px = (tile % A.tilesX) * 16 + (wave & 1u) * 8 + (lane & 7u);
  const uint32_t py = A.rowBegin + (tile / A.tilesX) * 16 + (wave >> 1) * 8 + (lane >> 3);
  bool want = false;
  RayRec rr;
  if (px < fp.W && py < A.rowEnd) atPrimarySurface(fp, A.visDepth, A.fat0, A.fat1, px, py, [&](const PrimarySurface& s) {
    const f3 L = mk3(A.Lx, A.Ly, A.Lz);
    const float NoL = dot3(s.N, L);
    f3 Ls = L;      // SOFT: toward the point of the disk the pixel draws this frame; below the horizon there is no ray and no term
    bool facing = NoL > 0.0f;
    if constexpr (SOFT) { if (facing) { Ls = sunDiskDirection(A.disk, L, s.pixel, fp.g.FrameIndex, RT_SLOT_SUN); facing = dot3(s.N, Ls) > 0.0f; } }
    if (facing) {
      const f3 Fk = deltaLightSpecular(s.N, s.V, L, NoL, s.color, s.rm);
      want = true;
      rr = shadowRay(s.P, Ls, s.pixel, (s.inst << 24) | s.prim, mk3(Fk.x * A.Ex, Fk.y * A.Ey, Fk.z * A.Ez), __float_as_uint(NoL));
    }
  });
  const uint32_t bin = blockIdx.x * 4u + wave;
  const uint32_t n = compactShadowRay<false>(want, rr, RT_RAY_TMAX, A.rays, A.hits, nullptr, bin, RT_BIN_MIN, 0u, lane);
  if (lane == 0) A.binCount[bin] = n;
}
struct SunAddArgs {
  const RayRec* rays; const HitKey* hits; const uint32_t* binCount; const uint32_t* tileWords;
  uint32_t* reflOut; uint32_t* diffOut; float Ex, Ey, Ez;
};
__global__ void __launch_bounds__(256) sunAddKernel(const FrameParams* __restrict__ fpp, SunAddArgs A) {
  const FrameParams& fp = *fpp;
  if (tileIsEmpty(A.tileWords, blockIdx.x)) return;
  const uint32_t bin = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (lane >= A.binCount[bin]) return;
  const size_t k = (size_t)bin * RT_BIN_MIN + lane;
  if (hitKeyId(A.hits[k]) != 0xFFFFFFFFu) return;      // occluded: both words stay
  const RayRec rr = A.rays[k];
  const uint32_t inst = rr.skip >> 24;
  const f3 spec = mk3(rr.wx, rr.wy, rr.wz);
  A.reflOut[rr.pixel] = packR11G11B10F(unpackR11G11B10F(A.reflOut[rr.pixel]) + spec);
  if (fp.mat.RoughMetals[inst][1] < 1.0f) {      // rghMtl.y < 1 is the instance's constant (launchShade); elsewhere RayTracingOut1 is a carry-over and stays
    const float w = __uint_as_float(rr.flags) / RT_PI;
    const f3 diff = mk3(((fp.mat.BaseColors[inst][0] * (1.0f - 0.04f)) * w) * A.Ex, ((fp.mat.BaseColors[inst][1] * (1.0f - 0.04f)) * w) * A.Ey,
                        ((fp.mat.BaseColors[inst][2] * (1.0f - 0.04f)) * w) * A.Ez);
    A.diffOut[rr.pixel] = packR11G11B10F(unpackR11G11B10F(A.diffOut[rr.pixel]) + diff);
  }
}
static SunDiskArgs sunDisk(const rtggx_context* c, uint32_t frameIndex, uint32_t slotBase) {
  const rtggx_context::Sun& sun = c->sun;
  return SunDiskArgs{sun.T[0], sun.T[1], sun.T[2], sun.B[0], sun.B[1], sun.B[2], c->sunAngle.k, c->cosSinTab, frameIndex, slotBase};
}
int launchSun(rtggx_context* c, const FrameParams& fp, hipStream_t s) {
  uint32_t rb, re;
  passRows(fp, ROWS_GBUFFER, rb, re);
  if (re <= rb) return 0;
  const uint32_t tilesX = (fp.W + 15) / 16, tilesY = (re - rb + 15) / 16, numTiles = tilesX * tilesY;
  if (numTiles * 4u > c->numBinsMax || !c->sunQueue.rays) { setError("rtggx_ray_trace: the sun's queue does not hold %u bins", numTiles * 4u); return -1; }
  const InputSet& set = c->cur();
  const rtggx_context::Sun& sun = c->sun;
  const TraceQueue q = c->sunQueue.view();      // bins of RT_BIN_MIN slots whatever the frame's have
  SunGenArgs G;
  G.visDepth = c->curVis().depth; G.fat0 = c->mesh[0].fat; G.fat1 = c->mesh[1].fat;
  G.rays = (RayRec*)q.rays; G.hits = q.hits; G.binCount = c->sunQueue.count;
  G.tileWords = c->tileWords(rb, re); G.tilesX = tilesX; G.rowBegin = rb; G.rowEnd = re;
  G.Lx = sun.L[0]; G.Ly = sun.L[1]; G.Lz = sun.L[2]; G.Ex = sun.E[0]; G.Ey = sun.E[1]; G.Ez = sun.E[2];
  const FrameParams* const dfp = c->dParams + c->slot;
  if (c->sunAngle.degrees > 0.0f) {      // rtggx_set_sun_angle
    SunGenArgsSoft GS;
    static_cast<SunGenArgs&>(GS) = G;
    GS.disk = sunDisk(c, 0u, 0u);
    launch(sunGenKernel<true>, dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, GS);
  } else launch(sunGenKernel<false>, dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, G);
  // Spill part 2 is the main stream's (launchShade): the launches that use it are in this stream's order, and nothing beside the stream touches it
  { const int r = launchTrace(c, fp, s, q, numTiles * 4u, true, tilesX, tilesY, c->traceGrid[3], -1, nullptr, nullptr, 2, !RT_SUN_CLOSEST); if (r) return r; }
  SunAddArgs S;
  S.rays = q.rays; S.hits = q.hits; S.binCount = q.binCount; S.tileWords = G.tileWords;
  S.reflOut = set.rtRefl; S.diffOut = set.rtDiff; S.Ex = G.Ex; S.Ey = G.Ey; S.Ez = G.Ez;
  launch(sunAddKernel, dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, S);
  RT_HIP(hipGetLastError());
  return 0;
}

// ---- local lights (rtggx_set_lights; DESIGN.md section 9 "Local lights") -----------------------------------------------------------------------
// The sun's pass with a light inside the scene: per light, in index order on the main stream, into ONE queue all lights share, the ray's own
// interval (1e-5, tmax) in a float2 array beside it, which the any-hit traversal reads (TraceQueue::tRange).  lightGenKernel puts the specular
// term in the record's weight and g = (NoL / pi) att in its flags word; lightAddKernel adds an unoccluded slot's terms to the pixel's fp32 sums
// (a pixel has at most one slot per light: the order of a sum is the order of the lights).  Behind the last light sunHitResolveKernel packs
// the sums into the words and leaves them zero.
struct LightArgs { float Px, Py, Pz, range, Ix, Iy, Iz, radius, Ax, Ay, Az, cosOuter, cosInner; };
struct LightSample { f3 L, Ls; float NoL, tmax, att; };      // L: toward the centre (the term's direction); Ls, tmax: the shadow ray's
// Steps 1-6 of rtggx_set_lights at the surface point P with normal N: where none of them says 'no ray, no term', onLit(sample) runs
// (atPrimarySurface).  j: the hash slot (SOFT only).
template <bool CONE, bool SOFT, class Lit>
RT_DEV void evalLight(const LightArgs& K, const float* cosSin, f3 P, f3 N, uint32_t pixel, uint32_t frameIndex, uint32_t j, Lit onLit) {
  // steps 1 and 2: in range, facing
  const f3 D = mk3(K.Px - P.x, K.Py - P.y, K.Pz - P.z);
  const float d2 = dot3(D, D), RR = K.range * K.range;
  const f3 L = normalize3(D);
  const float NoL = dot3(N, L);
  bool lit = d2 >= 1e-6f && d2 < RR && NoL > 0.0f;
  float spot = 1.0f;
  if constexpr (CONE) {      // step 3
    const float c = -dot3(L, mk3(K.Ax, K.Ay, K.Az));
    const float t = saturatef((c - K.cosOuter) / (K.cosInner - K.cosOuter));
    spot = t * t;
    lit = lit && c > K.cosOuter;
  }
  f3 Ds = D;
  if constexpr (SOFT) {      // step 5: a point of the emitting sphere, uniform over its surface
    if (lit) {
      const ShadowSample x = shadowSample(pixel, frameIndex, j);
      const float z = 1.0f - 2.0f * x.u, rho = sqrtf(1.0f - z * z);
      Ds = mk3(D.x + K.radius * (rho * cosSin[x.s]), D.y + K.radius * (rho * cosSin[256u + x.s]), D.z + K.radius * z);
    }
  }
  const float ds2 = dot3(Ds, Ds);
  const f3 Ls = normalize3(Ds);
  lit = lit && ds2 >= 1e-6f && dot3(N, Ls) > 0.0f;      // step 6
  if (!lit) return;
  // step 4: the window, the floor; E = I att
  const float q = d2 / RR;
  float win = saturatef(1.0f - q * q); win = win * win;
  const float m2 = fmaxf(K.radius * K.radius, 1e-4f);
  LightSample o;
  o.att = (win * spot) / fmaxf(d2, m2);
  o.L = L; o.Ls = Ls; o.NoL = NoL; o.tmax = sqrtf(ds2);
  onLit(o);
}
struct LightGenArgs {
  const unsigned long long* visDepth; const float4* fat0; const float4* fat1;
  RayRec* rays; HitKey* hits; uint32_t* binCount; float2* tRange;
  const uint32_t* tileWords; uint32_t tilesX, rowBegin, rowEnd;
  LightArgs light;
  const float* cosSin; uint32_t slot;      // SOFT: the 256-entry table, and RT_SLOT_LIGHT(i)
};
template <bool CONE, bool SOFT>
__global__ void __launch_bounds__(256) lightGenKernel(const FrameParams* __restrict__ fpp, LightGenArgs A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t px = (tile % A.tilesX) * 16 + (wave & 1u) * 8 + (lane & 7u);
  const uint32_t py = A.rowBegin + (tile / A.tilesX) * 16 + (wave >> 1) * 8 + (lane >> 3);
  bool want = false;
  RayRec rr;
  float tmax = 0.0f;
  if (px < fp.W && py < A.rowEnd) atPrimarySurface(fp, A.visDepth, A.fat0, A.fat1, px, py, [&](const PrimarySurface& s) {
    evalLight<CONE, SOFT>(A.light, A.cosSin, s.P, s.N, s.pixel, fp.g.FrameIndex, A.slot, [&](const LightSample& l) {      // step 8: the sun's term at the centre direction L
    const f3 Fk = deltaLightSpecular(s.N, s.V, l.L, l.NoL, s.color, s.rm);
    want = true;
    tmax = l.tmax;
    rr = shadowRay(s.P, l.Ls, s.pixel, (s.inst << 24) | s.prim, mk3(Fk.x * (A.light.Ix * l.att), Fk.y * (A.light.Iy * l.att), Fk.z * (A.light.Iz * l.att)),
                   __float_as_uint((l.NoL / RT_PI) * l.att));
  }); });
  const uint32_t bin = blockIdx.x * 4u + wave;
  const uint32_t n = compactShadowRay<true>(want, rr, tmax, A.rays, A.hits, A.tRange, bin, RT_BIN_MIN, 0u, lane);
  if (lane == 0) A.binCount[bin] = n;
}
struct LightAddArgs {
  const RayRec* rays; const HitKey* hits; const uint32_t* binCount; const uint32_t* tileWords;
  float4* sumRefl; float4* sumDiff; float Ix, Iy, Iz;
};
__global__ void __launch_bounds__(256) lightAddKernel(const FrameParams* __restrict__ fpp, LightAddArgs A) {
  const FrameParams& fp = *fpp;
  if (tileIsEmpty(A.tileWords, blockIdx.x)) return;
  const uint32_t bin = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (lane >= A.binCount[bin]) return;
  const size_t k = (size_t)bin * RT_BIN_MIN + lane;
  if (hitKeyId(A.hits[k]) != 0xFFFFFFFFu) return;      // occluded: no term
  const RayRec rr = A.rays[k];
  const uint32_t inst = rr.skip >> 24;
  const float4 s0 = A.sumRefl[rr.pixel];
  A.sumRefl[rr.pixel] = make_float4(s0.x + rr.wx, s0.y + rr.wy, s0.z + rr.wz, s0.w + 1.0f);
  if (fp.mat.RoughMetals[inst][1] < 1.0f) {      // rghMtl.y < 1 is the instance's constant (launchShade); elsewhere RayTracingOut1 is a carry-over and stays
    const float g = __uint_as_float(rr.flags);
    const float4 s1 = A.sumDiff[rr.pixel];
    A.sumDiff[rr.pixel] = make_float4(s1.x + ((fp.mat.BaseColors[inst][0] * (1.0f - 0.04f)) * g) * A.Ix, s1.y + ((fp.mat.BaseColors[inst][1] * (1.0f - 0.04f)) * g) * A.Iy,
                                      s1.z + ((fp.mat.BaseColors[inst][2] * (1.0f - 0.04f)) * g) * A.Iz, s1.w + 1.0f);
  }
}
// A light of the context's list as the kernels take it; whether it casts rays at all (intensity 0 in every component: it keeps its index and
// casts none); which <CONE, SOFT> instance it runs, as an index [2 cone + soft] into a table of the four
static LightArgs lightArgs(const RtggxLight& l) {
  return LightArgs{l.position[0], l.position[1], l.position[2], l.range, l.intensity[0], l.intensity[1], l.intensity[2], l.radius,
                   l.axis[0], l.axis[1], l.axis[2], l.cos_outer, l.cos_inner};
}
static bool lightCastsRays(const RtggxLight& l) { return l.intensity[0] > 0.0f || l.intensity[1] > 0.0f || l.intensity[2] > 0.0f; }
static uint32_t lightVariant(const RtggxLight& l) { return (l.cos_outer > -1.0f ? 2u : 0u) | (l.radius > 0.0f ? 1u : 0u); }
static void (*const kLightGen[4])(const FrameParams*, LightGenArgs) = {lightGenKernel<false, false>, lightGenKernel<false, true>, lightGenKernel<true, false>, lightGenKernel<true, true>};

// One level's unoccluded terms into the sums of the two hit passes.  One lane per slot.  SAMPLES: the sums are the sample sums (three floats
// per pixel and image); else S, four: the terms and their number.
struct SunHitAddArgs {
  const RayRec* rays; const HitKey* hits; const uint32_t* binCount; uint32_t binSlots; const uint32_t* tileWords;
  float* sumRefl; float* sumDiff;
};
template <bool SAMPLES>
__global__ void __launch_bounds__(256) sunHitAddKernel(SunHitAddArgs A) {
  if (tileIsEmpty(A.tileWords, blockIdx.x)) return;
  const uint32_t bin = blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t count = min(A.binCount[bin], A.binSlots);
  for (uint32_t i = threadIdx.x & 63u; i < count; i += 64u) {
    const size_t k = (size_t)bin * A.binSlots + i;
    if (hitKeyId(A.hits[k]) != 0xFFFFFFFFu) continue;      // occluded: no term
    const RayRec rr = A.rays[k];
    float* const sum = (rr.flags & 1u) != 0u ? A.sumDiff : A.sumRefl;
    if constexpr (SAMPLES) {
      float* acc = sum + 3u * (size_t)rr.pixel;
      acc[0] = acc[0] + rr.wx; acc[1] = acc[1] + rr.wy; acc[2] = acc[2] + rr.wz;
    } else {
      float4* acc = reinterpret_cast<float4*>(sum) + rr.pixel;
      const float4 s = *acc;
      *acc = make_float4(s.x + rr.wx, s.y + rr.wy, s.z + rr.wz, s.w + 1.0f);
    }
  }
}
// One sample per pixel, behind the last shading pass or the last light: word = pack(unpack(word) + S) where a term exists (S.w: their
// number), the word untouched where none does; S is left zero for the next frame by the lanes that found it set.
struct SunHitResolveArgs { float4* sumRefl; float4* sumDiff; uint32_t* reflOut; uint32_t* diffOut; const uint32_t* tileWords; uint32_t tilesX, rowBegin, rowEnd; };
__global__ void __launch_bounds__(256) sunHitResolveKernel(const FrameParams* __restrict__ fpp, SunHitResolveArgs A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t px = (tile % A.tilesX) * 16u + (threadIdx.x & 15u), py = A.rowBegin + (tile / A.tilesX) * 16u + (threadIdx.x >> 4);
  if (px >= fp.W || py >= A.rowEnd) return;
  const size_t pix = (size_t)py * fp.W + px;
  const float4 r = A.sumRefl[pix], d = A.sumDiff[pix];
  if (r.w != 0.0f) { A.reflOut[pix] = packR11G11B10F(unpackR11G11B10F(A.reflOut[pix]) + mk3(r.x, r.y, r.z)); A.sumRefl[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
  if (d.w != 0.0f) { A.diffOut[pix] = packR11G11B10F(unpackR11G11B10F(A.diffOut[pix]) + mk3(d.x, d.y, d.z)); A.sumDiff[pix] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
}
// S = sums: [2][W * H] float4, RayTracingOut0's then RayTracingOut1's; `done` (may be null) rides on the kernel
int launchSunHitResolve(rtggx_context* c, hipStream_t s, float* sums, const uint32_t* tileWords, uint32_t tilesX, uint32_t rowBegin, uint32_t rowEnd, hipEvent_t done) {
  const InputSet& set = c->cur();
  const SunHitResolveArgs R{(float4*)sums, (float4*)sums + (size_t)c->W * c->H, set.rtRefl, set.rtDiff, tileWords, tilesX, rowBegin, rowEnd};
  launch(sunHitResolveKernel, dim3(tilesX * ((rowEnd - rowBegin + 15u) / 16u)), dim3(256), s, nullptr, done, c->dParams + c->slot, R);
  RT_HIP(hipGetLastError());
  return 0;
}
// (a fill runs on the null stream, which this context's streams are not ordered against: one synchronise behind all of a call's fills)
static int syncFills(bool filled) { if (filled) RT_HIP(hipStreamSynchronize(nullptr)); return 0; }

// ---- one shadow ray for all lights (rtggx_set_light_sampling(ctx, 1); DESIGN.md section 9 "One ray for all lights") -----------------------------
// In place of the per-light loops of launchLights and launchLightHits: ONE generating kernel takes the whole list as a kernel argument -- the
// walk over the lights is wave-uniform and fed by scalar loads --, weighs every light by the luminance w_i its unshadowed term would have at
// the surface (a first loop, unrolled to the constant bound 8, so that the w_i stay in registers), picks one light per surface point with
// one draw of the pixel's hash, evaluates that light once more -- now with its target -- and compacts its ONE shadow ray with the finished
// term times f = W / w_i.  One any-hit traversal and one add follow, whatever the number of lights.
//   the step, written once below           who runs it
//   pickLuminance, pickDraw, pickLight     lightPickGenKernel, lightHitPickGenKernel
//   chosenLight                            both: the chosen light's record out of the kernel argument, by selects
// CONE and SOFT are compile-time here as well, but per LIST: does any casting light have a cone, a radius.  In a CONE instance a light
// without a cone runs the cone's arithmetic on A = 0, cos_outer = -2, cos_inner = -1 (pickList), which gives spot = 1 exactly and refuses
// nothing; in a SOFT instance a chosen light without a radius takes the branch without the hash, so that Ds is D bit for bit.
#define RT_SLOT_LIGHT_PICK 96u
#define RT_SLOT_LIGHT_PICK_HIT(d) (104u + 2u * (d))
#define RT_SLOT_LIGHT_PICK_HIT_IMAGE 1u
struct LightListArgs { LightArgs light[RTGGX_MAX_LIGHTS]; uint32_t castMask; const float* cosSin; };      // castMask: bit i, light i has an intensity
RT_DEV float pickLuminance(f3 c) { return (0.25f * c.x + 0.5f * c.y) + 0.25f * c.z; }
// Step 3: x in [0, 1) from the top 24 bits of the slot's word
RT_DEV float pickDraw(uint32_t pixel, uint32_t frameIndex, uint32_t j) {
  uint32_t h = rng(pixel); h += frameIndex; h = rng(h);
  const uint32_t v = rng(h + j * 0x9E3779B9u);
  return (float)(v >> 8) / 16777216.0f;
}
// Step 4 over the eight weights (0: not a candidate): the first candidate with t < c, else the last one; wOut: its weight
RT_DEV uint32_t pickLight(const float (&w)[RTGGX_MAX_LIGHTS], float t, float& wOut) {
  float c = 0.0f;
  uint32_t chosen = 0u;
  bool found = false;
#pragma unroll
  for (uint32_t i = 0; i < RTGGX_MAX_LIGHTS; ++i) {
    if (w[i] > 0.0f) {
      c = c + w[i];
      if (!found) { chosen = i; wOut = w[i]; found = t < c; }
    }
  }
  return chosen;
}
RT_DEV LightArgs chosenLight(const LightListArgs& list, uint32_t chosen) {
  LightArgs K = list.light[0];
#pragma unroll
  for (uint32_t i = 1; i < RTGGX_MAX_LIGHTS; ++i) {
    const LightArgs& o = list.light[i];
    const bool is = chosen == i;
    K.Px = is ? o.Px : K.Px; K.Py = is ? o.Py : K.Py; K.Pz = is ? o.Pz : K.Pz; K.range = is ? o.range : K.range;
    K.Ix = is ? o.Ix : K.Ix; K.Iy = is ? o.Iy : K.Iy; K.Iz = is ? o.Iz : K.Iz; K.radius = is ? o.radius : K.radius;
    K.Ax = is ? o.Ax : K.Ax; K.Ay = is ? o.Ay : K.Ay; K.Az = is ? o.Az : K.Az; K.cosOuter = is ? o.cosOuter : K.cosOuter; K.cosInner = is ? o.cosInner : K.cosInner;
  }
  return K;
}
// Steps 1-4 and 8 of rtggx_set_lights for one light at the primary surface, without the target: spec and (diffuse: m < 1) diff
struct PickTerms { f3 spec, diff; float w; };
template <bool CONE>
RT_DEV PickTerms primaryPickTerms(const LightArgs& K, const PrimarySurface& s, bool diffuse) {
  PickTerms o;
  o.spec = o.diff = mk3(0.0f, 0.0f, 0.0f); o.w = 0.0f;
  evalLight<CONE, false>(K, nullptr, s.P, s.N, 0u, 0u, 0u, [&](const LightSample& l) {
    const f3 Fk = deltaLightSpecular(s.N, s.V, l.L, l.NoL, s.color, s.rm);
    o.spec = mk3(Fk.x * (K.Ix * l.att), Fk.y * (K.Iy * l.att), Fk.z * (K.Iz * l.att));
    o.w = pickLuminance(o.spec);
    if (diffuse) {
      const float g = (l.NoL / RT_PI) * l.att;
      o.diff = mk3(((s.color.x * (1.0f - 0.04f)) * g) * K.Ix, ((s.color.y * (1.0f - 0.04f)) * g) * K.Iy, ((s.color.z * (1.0f - 0.04f)) * g) * K.Iz);
      o.w = o.w + pickLuminance(o.diff);
    }
  });
  if (!(o.w > 0.0f)) o.w = 0.0f;      // not a candidate (a NaN is none)
  return o;
}
// Step 6: the chosen light's target.  A light without a radius in a SOFT instance: the branch without the hash
template <bool CONE, bool SOFT>
RT_DEV bool chosenLightSample(const LightArgs& K, const float* cosSin, f3 P, f3 N, uint32_t pixel, uint32_t frameIndex, uint32_t j, LightSample& out) {
  bool lit = false;
  const auto onLit = [&](const LightSample& l) { out = l; lit = true; };
  if constexpr (SOFT) {
    if (K.radius > 0.0f) evalLight<CONE, true>(K, cosSin, P, N, pixel, frameIndex, j, onLit);
    else evalLight<CONE, false>(K, cosSin, P, N, pixel, frameIndex, j, onLit);
  } else evalLight<CONE, false>(K, cosSin, P, N, pixel, frameIndex, j, onLit);
  return lit;
}
struct LightPickGenArgs {
  const unsigned long long* visDepth; const float4* fat0; const float4* fat1;
  RayRec* rays; HitKey* hits; uint32_t* binCount; float2* tRange; float4* diffTerm;      // diffTerm: S1 of the slot's ray, where m < 1
  const uint32_t* tileWords; uint32_t tilesX, rowBegin, rowEnd;
  LightListArgs list;
};
template <bool CONE, bool SOFT>
__global__ void __launch_bounds__(256) lightPickGenKernel(const FrameParams* __restrict__ fpp, LightPickGenArgs A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t px = (tile % A.tilesX) * 16 + (wave & 1u) * 8 + (lane & 7u);
  const uint32_t py = A.rowBegin + (tile / A.tilesX) * 16 + (wave >> 1) * 8 + (lane >> 3);
  bool want = false, wantDiff = false;
  RayRec rr;
  float tmax = 0.0f;
  f3 S1 = mk3(0.0f, 0.0f, 0.0f);
  if (px < fp.W && py < A.rowEnd) atPrimarySurface(fp, A.visDepth, A.fat0, A.fat1, px, py, [&](const PrimarySurface& s) {
    const bool diffuse = s.rm.y < 1.0f;
    // steps 1 and 2: the eight weights, W
    float w[RTGGX_MAX_LIGHTS];
    float W = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < RTGGX_MAX_LIGHTS; ++i) {
      w[i] = 0.0f;
      if ((A.list.castMask >> i) & 1u) w[i] = primaryPickTerms<CONE>(A.list.light[i], s, diffuse).w;
      W = W + w[i];      // (a weight of +0 leaves W as it is)
    }
    if (!(W > 0.0f)) return;      // no candidate
    // steps 3-5
    const float t = pickDraw(s.pixel, fp.g.FrameIndex, RT_SLOT_LIGHT_PICK) * W;
    float wc = 0.0f;
    const uint32_t chosen = pickLight(w, t, wc);
    const float f = W / wc;
    // steps 6 and 7: the chosen light once more, with its target
    const LightArgs K = chosenLight(A.list, chosen);
    LightSample l;
    if (!chosenLightSample<CONE, SOFT>(K, A.list.cosSin, s.P, s.N, s.pixel, fp.g.FrameIndex, RT_SLOT_LIGHT(chosen), l)) return;
    const PickTerms x = primaryPickTerms<CONE>(K, s, diffuse);
    want = true; wantDiff = diffuse;
    tmax = l.tmax;
    rr = shadowRay(s.P, l.Ls, s.pixel, (s.inst << 24) | s.prim, mk3(x.spec.x * f, x.spec.y * f, x.spec.z * f), 0u);
    S1 = mk3(x.diff.x * f, x.diff.y * f, x.diff.z * f);
  });
  const uint32_t bin = blockIdx.x * 4u + wave;
  const unsigned long long wanting = __ballot(want);      // (the slot compactShadowRay gives the lane)
  if (wantDiff) A.diffTerm[(size_t)bin * RT_BIN_MIN + (uint32_t)__popcll(wanting & ((1ull << lane) - 1ull))] = make_float4(S1.x, S1.y, S1.z, 0.0f);
  const uint32_t n = compactShadowRay<true>(want, rr, tmax, A.rays, A.hits, A.tRange, bin, RT_BIN_MIN, 0u, lane);
  if (lane == 0) A.binCount[bin] = n;
}
// lightAddKernel for a queue whose rays belong to different lights: the slot's own S1 beside the record
struct LightPickAddArgs {
  const RayRec* rays; const HitKey* hits; const uint32_t* binCount; const uint32_t* tileWords; const float4* diffTerm;
  float4* sumRefl; float4* sumDiff;
};
__global__ void __launch_bounds__(256) lightPickAddKernel(const FrameParams* __restrict__ fpp, LightPickAddArgs A) {
  const FrameParams& fp = *fpp;
  if (tileIsEmpty(A.tileWords, blockIdx.x)) return;
  const uint32_t bin = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (lane >= A.binCount[bin]) return;
  const size_t k = (size_t)bin * RT_BIN_MIN + lane;
  if (hitKeyId(A.hits[k]) != 0xFFFFFFFFu) return;      // occluded: no term
  const RayRec rr = A.rays[k];
  const uint32_t inst = rr.skip >> 24;
  const float4 s0 = A.sumRefl[rr.pixel];
  A.sumRefl[rr.pixel] = make_float4(s0.x + rr.wx, s0.y + rr.wy, s0.z + rr.wz, s0.w + 1.0f);
  if (fp.mat.RoughMetals[inst][1] < 1.0f) {      // (lightAddKernel)
    const float4 d = A.diffTerm[k], s1 = A.sumDiff[rr.pixel];
    A.sumDiff[rr.pixel] = make_float4(s1.x + d.x, s1.y + d.y, s1.z + d.z, s1.w + 1.0f);
  }
}
// ---- the pick and what the pixel remembers (rtggx_set_light_pick_visibility; DESIGN.md section 9 under that title) -----------------------------
// The picking pair of the primary pass once more, with a record per pixel (RtggxLightVisRecord: eight visibility bytes, the normal word, a
// stamp) in two images that alternate by the sequence number s: lightPickVisGenKernel follows the frame's velocity word to the record the
// previous acting frame wrote, takes its eight bytes where the record is that frame's, that instance's and of a like normal (255 each
// otherwise), writes the pixel's own record with them and multiplies every candidate's weight by max(v_i, RTGGX_LIGHT_VIS_FLOOR) before the
// draw; the chosen index travels in the shadow ray's flags word.  lightPickVisAddKernel moves the chosen light's byte a quarter of the way
// to 255 or to 0 by what the ray met -- a read-modify-write of one word of the pixel's own record -- and adds as lightPickAddKernel does.
// The eight bytes stay two registers: the unrolled loop shifts them out by constants.
struct LightVisArgs {
  const uint32_t* normal; const uint32_t* velocity;      // the frame's own G-buffer words (the current input set)
  const uint4* prev; uint4* next;                        // the image read ((s - 1) & 1) and the image written (s & 1)
  uint32_t prevSeq, stampHigh, history;                  // (s - 1) & 0xFFFFFF; (s & 0xFFFFFF) << 8; s - 1 > s0
};
RT_DEV float visByteWeight(uint32_t lo, uint32_t hi, uint32_t i) {      // (float)max(v_i, floor); i is a constant where this is inlined
  const uint32_t v = ((i < 4u ? lo : hi) >> (8u * (i & 3u))) & 0xFFu;
  return (float)max(v, RTGGX_LIGHT_VIS_FLOOR);
}
RT_DEV int visNormalDot(uint32_t a, uint32_t b) {      // the dot of the spatial filters' decode (denoise.hip loadG): integers, 1023^2 is one
  const int ax = 2 * (int)(a & 1023u) - 1023, ay = 2 * (int)((a >> 10) & 1023u) - 1023, az = 2 * (int)((a >> 20) & 1023u) - 1023;
  const int bx = 2 * (int)(b & 1023u) - 1023, by = 2 * (int)((b >> 10) & 1023u) - 1023, bz = 2 * (int)((b >> 20) & 1023u) - 1023;
  return ax * bx + ay * by + az * bz;
}
template <bool CONE, bool SOFT>
__global__ void __launch_bounds__(256) lightPickVisGenKernel(const FrameParams* __restrict__ fpp, LightPickGenArgs A, LightVisArgs R) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t px = (tile % A.tilesX) * 16 + (wave & 1u) * 8 + (lane & 7u);
  const uint32_t py = A.rowBegin + (tile / A.tilesX) * 16 + (wave >> 1) * 8 + (lane >> 3);
  bool want = false, wantDiff = false;
  RayRec rr;
  float tmax = 0.0f;
  f3 S1 = mk3(0.0f, 0.0f, 0.0f);
  if (px < fp.W && py < A.rowEnd && py < fp.H) atPrimarySurface(fp, A.visDepth, A.fat0, A.fat1, px, py, [&](const PrimarySurface& s) {
    const bool diffuse = s.rm.y < 1.0f;
    // step 2: the history, along the frame's own velocity
    const uint32_t nrm = R.normal[s.pixel], vel = R.velocity[s.pixel];
    const float qx = floorf(((float)px + 0.5f) - f16ToF32(vel & 0xFFFFu) * (float)fp.W), qy = floorf(((float)py + 0.5f) - f16ToF32(vel >> 16) * (float)fp.H);
    uint32_t lo = 0xFFFFFFFFu, hi = 0xFFFFFFFFu;
    if (R.history != 0u && qx >= 0.0f && qx < (float)fp.W && qy >= 0.0f && qy < (float)fp.H) {
      const uint4 rec = R.prev[(size_t)(uint32_t)qy * fp.W + (uint32_t)qx];
      if ((rec.w >> 8) == R.prevSeq && (rec.w & 0xFFu) == s.inst + 1u && (float)visNormalDot(rec.z, nrm) >= 0.9f * 1046529.0f) { lo = rec.x; hi = rec.y; }
    }
    R.next[s.pixel] = make_uint4(lo, hi, nrm, R.stampHigh | (s.inst + 1u));
    // steps 1 and 3: the eight weights times what the pixel remembers, U
    float u[RTGGX_MAX_LIGHTS];
    float U = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < RTGGX_MAX_LIGHTS; ++i) {
      u[i] = 0.0f;
      if ((A.list.castMask >> i) & 1u) {
        const float w = primaryPickTerms<CONE>(A.list.light[i], s, diffuse).w;
        if (w > 0.0f) u[i] = w * visByteWeight(lo, hi, i);
      }
      U = U + u[i];      // (a weight of +0 leaves U as it is)
    }
    if (!(U > 0.0f)) return;      // no candidate
    // step 4: mode 1's draw, pick and f on u
    const float t = pickDraw(s.pixel, fp.g.FrameIndex, RT_SLOT_LIGHT_PICK) * U;
    float uc = 0.0f;
    const uint32_t chosen = pickLight(u, t, uc);
    const float f = U / uc;
    // step 5: mode 1's steps 6 and 7; the chosen index in the record's flags word, for the update
    const LightArgs K = chosenLight(A.list, chosen);
    LightSample l;
    if (!chosenLightSample<CONE, SOFT>(K, A.list.cosSin, s.P, s.N, s.pixel, fp.g.FrameIndex, RT_SLOT_LIGHT(chosen), l)) return;
    const PickTerms x = primaryPickTerms<CONE>(K, s, diffuse);
    want = true; wantDiff = diffuse;
    tmax = l.tmax;
    rr = shadowRay(s.P, l.Ls, s.pixel, (s.inst << 24) | s.prim, mk3(x.spec.x * f, x.spec.y * f, x.spec.z * f), chosen);
    S1 = mk3(x.diff.x * f, x.diff.y * f, x.diff.z * f);
  });
  const uint32_t bin = blockIdx.x * 4u + wave;
  const unsigned long long wanting = __ballot(want);      // (the slot compactShadowRay gives the lane)
  if (wantDiff) A.diffTerm[(size_t)bin * RT_BIN_MIN + (uint32_t)__popcll(wanting & ((1ull << lane) - 1ull))] = make_float4(S1.x, S1.y, S1.z, 0.0f);
  const uint32_t n = compactShadowRay<true>(want, rr, tmax, A.rays, A.hits, A.tRange, bin, RT_BIN_MIN, 0u, lane);
  if (lane == 0) A.binCount[bin] = n;
}
// lightPickAddKernel with step 6: every slot below the bin's count updates its pixel's record, occluded or not
__global__ void __launch_bounds__(256) lightPickVisAddKernel(const FrameParams* __restrict__ fpp, LightPickAddArgs A, uint32_t* records) {
  const FrameParams& fp = *fpp;
  if (tileIsEmpty(A.tileWords, blockIdx.x)) return;
  const uint32_t bin = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (lane >= A.binCount[bin]) return;
  const size_t k = (size_t)bin * RT_BIN_MIN + lane;
  const bool occluded = hitKeyId(A.hits[k]) != 0xFFFFFFFFu;
  const RayRec rr = A.rays[k];
  const uint32_t chosen = rr.flags & 7u, shift = 8u * (chosen & 3u);
  uint32_t* const word = records + 4u * (size_t)rr.pixel + (chosen >> 2);      // the pixel's own record: no other lane has this pixel
  const uint32_t old = *word, v = (old >> shift) & 0xFFu;
  const uint32_t next = occluded ? v - ((v + 3u) >> 2) : v + ((255u - v + 3u) >> 2);
  *word = (old & ~(0xFFu << shift)) | (next << shift);
  if (occluded) return;      // no term
  const uint32_t inst = rr.skip >> 24;
  const float4 s0 = A.sumRefl[rr.pixel];
  A.sumRefl[rr.pixel] = make_float4(s0.x + rr.wx, s0.y + rr.wy, s0.z + rr.wz, s0.w + 1.0f);
  if (fp.mat.RoughMetals[inst][1] < 1.0f) {      // (lightAddKernel)
    const float4 d = A.diffTerm[k], s1 = A.sumDiff[rr.pixel];
    A.sumDiff[rr.pixel] = make_float4(s1.x + d.x, s1.y + d.y, s1.z + d.z, s1.w + 1.0f);
  }
}
// The context's list as the picking kernels take it, and the instance [2 cone + soft] the list runs (see above)
static uint32_t pickVariant(const rtggx_context* c) {
  uint32_t v = 0u;
  for (uint32_t i = 0; i < c->lights.count; ++i) if (lightCastsRays(c->lights.l[i])) v |= lightVariant(c->lights.l[i]);
  return v;
}
static LightListArgs pickList(const rtggx_context* c) {
  LightListArgs L = {};
  for (uint32_t i = 0; i < c->lights.count; ++i) {
    const RtggxLight& l = c->lights.l[i];
    if (!lightCastsRays(l)) continue;
    L.castMask |= 1u << i;
    L.light[i] = lightArgs(l);
    if (!(l.cos_outer > -1.0f)) { L.light[i].Ax = L.light[i].Ay = L.light[i].Az = 0.0f; L.light[i].cosOuter = -2.0f; L.light[i].cosInner = -1.0f; }
  }
  L.cosSin = c->cosSinTab;
  return L;
}
static void (*const kLightPickGen[4])(const FrameParams*, LightPickGenArgs) = {lightPickGenKernel<false, false>, lightPickGenKernel<false, true>, lightPickGenKernel<true, false>, lightPickGenKernel<true, true>};
static void (*const kLightPickVisGen[4])(const FrameParams*, LightPickGenArgs, LightVisArgs) = {lightPickVisGenKernel<false, false>, lightPickVisGenKernel<false, true>, lightPickVisGenKernel<true, false>, lightPickVisGenKernel<true, true>};
static int clearLightListCounts(rtggx_context* c, hipStream_t s);      // rtggx_set_light_list, further down
static int launchLightListGen(rtggx_context* c, hipStream_t s, const LightPickGenArgs& P, uint32_t numTiles, const LightVisArgs* records);
__global__ void __launch_bounds__(256) lightListVisAddKernel(const FrameParams* __restrict__ fpp, LightPickAddArgs A, uint32_t* records);      // rtggx_set_light_list_visibility, further down

int launchLights(rtggx_context* c, const FrameParams& fp, hipStream_t s) {
  uint32_t rb, re;
  passRows(fp, ROWS_GBUFFER, rb, re);
  if (re <= rb) return 0;
  const uint32_t tilesX = (fp.W + 15) / 16, tilesY = (re - rb + 15) / 16, numTiles = tilesX * tilesY;
  if (numTiles * 4u > c->numBinsMax) { setError("rtggx_ray_trace: the lights' queue does not hold %u bins", numTiles * 4u); return -1; }
  const bool list = c->lightList.count > 0u;      // rtggx_set_light_list: mode 1's launches, the generating kernel the list's (further down)
  const bool pick = c->lightSampling == 1u || list;      // rtggx_set_light_sampling
  { // what the lights need, from the first frame that has some: the queue with its intervals, the sums -- and in mode 1 the diffuse terms
    bool filled = false;
    { const int r = c->lightQueue.ensure(c->numBinsMax, RT_BIN_MIN, true, filled); if (r) return r; }
    if (!c->lightSums) { RT_HIP(allocFilled(c->lightSums, (size_t)c->W * c->H * 8u)); filled = true; }
    if (pick && !c->lightPickDiff) RT_HIP(alloc(c->lightPickDiff, (size_t)c->numBinsMax * RT_BIN_MIN * 4u));
    { const int r = syncFills(filled); if (r) return r; } }
  const InputSet& set = c->cur();
  const FrameParams* const dfp = c->dParams + c->slot;
  const TraceQueue q = c->lightQueue.view();      // bins of RT_BIN_MIN slots, as the sun's, and the rays' own intervals
  LightGenArgs G;
  G.visDepth = c->curVis().depth; G.fat0 = c->mesh[0].fat; G.fat1 = c->mesh[1].fat;
  G.rays = (RayRec*)q.rays; G.hits = q.hits; G.binCount = c->lightQueue.count; G.tRange = (float2*)q.tRange;
  G.tileWords = c->tileWords(rb, re); G.tilesX = tilesX; G.rowBegin = rb; G.rowEnd = re;
  G.cosSin = c->cosSinTab;
  LightAddArgs D;
  D.rays = q.rays; D.hits = q.hits; D.binCount = q.binCount; D.tileWords = G.tileWords;
  D.sumRefl = (float4*)c->lightSums.get(); D.sumDiff = D.sumRefl + (size_t)c->W * c->H;
  if (pick) {      // one generating launch, one traversal, one add for the whole list (none where no light has an intensity)
    LightPickGenArgs P;
    P.visDepth = G.visDepth; P.fat0 = G.fat0; P.fat1 = G.fat1;
    P.rays = G.rays; P.hits = G.hits; P.binCount = G.binCount; P.tRange = G.tRange; P.diffTerm = (float4*)c->lightPickDiff.get();
    P.tileWords = G.tileWords; P.tilesX = tilesX; P.rowBegin = rb; P.rowEnd = re;
    if (list) {      // rtggx_set_light_list: the same three launches (none where no light of the list has an intensity) and the resolve
      { const int r = clearLightListCounts(c, s); if (r) return r; }
      if (c->lightListCasting && c->lightListVis) {      // rtggx_set_light_list_visibility: an acting frame -- the same three launches with the records
        if (rb > 0u || re < fp.H) { setError("rtggx_ray_trace: the list's visibility records on rows [%u,%u) of %u: whole frames only", rb, re, fp.H); return -1; }
        if (!c->lightListVisImg[0] || !c->lightListVisImg[1]) {      // the allocation is a reset
          for (auto& img : c->lightListVisImg) if (!img) RT_HIP(allocFilled(img, (size_t)c->W * c->H * 4u));
          { const int r = syncFills(true); if (r) return r; }
          c->lightListVisSeq0 = c->lightListVisSeq;
        }
        const uint32_t seq = ++c->lightListVisSeq;
        LightVisArgs R;
        R.normal = set.normal; R.velocity = set.velocity;
        R.prev = (const uint4*)c->lightListVisImg[(seq - 1u) & 1u].get(); R.next = (uint4*)c->lightListVisImg[seq & 1u].get();
        R.prevSeq = (seq - 1u) & 0xFFFFFFu; R.stampHigh = (seq & 0xFFFFFFu) << 8; R.history = seq - 1u > c->lightListVisSeq0 ? 1u : 0u;
        { const int r = launchLightListGen(c, s, P, numTiles, &R); if (r) return r; }
        { const int r = launchTrace(c, fp, s, q, numTiles * 4u, true, tilesX, tilesY, c->traceGrid[3], -1, nullptr, nullptr, 2, true); if (r) return r; }
        const LightPickAddArgs PD{q.rays, q.hits, q.binCount, G.tileWords, P.diffTerm, D.sumRefl, D.sumDiff};
        launch(lightListVisAddKernel, dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, PD, (uint32_t*)R.next);
        RT_HIP(hipGetLastError());
      } else if (c->lightListCasting) {
        { const int r = launchLightListGen(c, s, P, numTiles, nullptr); if (r) return r; }
        { const int r = launchTrace(c, fp, s, q, numTiles * 4u, true, tilesX, tilesY, c->traceGrid[3], -1, nullptr, nullptr, 2, true); if (r) return r; }
        const LightPickAddArgs PD{q.rays, q.hits, q.binCount, G.tileWords, P.diffTerm, D.sumRefl, D.sumDiff};
        launch(lightPickAddKernel, dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, PD);
        RT_HIP(hipGetLastError());
      }
      return launchSunHitResolve(c, s, c->lightSums, G.tileWords, tilesX, rb, re, nullptr);
    }
    P.list = pickList(c);
    if (P.list.castMask && c->lightVis) {      // rtggx_set_light_pick_visibility: an acting frame -- the same three launches with the records
      if (rb > 0u || re < fp.H) { setError("rtggx_ray_trace: the pick's visibility records on rows [%u,%u) of %u: whole frames only", rb, re, fp.H); return -1; }
      if (!c->lightVisImg[0] || !c->lightVisImg[1]) {      // the allocation is a reset
        for (auto& img : c->lightVisImg) if (!img) RT_HIP(allocFilled(img, (size_t)c->W * c->H * 4u));
        { const int r = syncFills(true); if (r) return r; }
        c->lightVisSeq0 = c->lightVisSeq;
      }
      const uint32_t seq = ++c->lightVisSeq;
      LightVisArgs R;
      R.normal = set.normal; R.velocity = set.velocity;
      R.prev = (const uint4*)c->lightVisImg[(seq - 1u) & 1u].get(); R.next = (uint4*)c->lightVisImg[seq & 1u].get();
      R.prevSeq = (seq - 1u) & 0xFFFFFFu; R.stampHigh = (seq & 0xFFFFFFu) << 8; R.history = seq - 1u > c->lightVisSeq0 ? 1u : 0u;
      launch(kLightPickVisGen[pickVariant(c)], dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, P, R);
      { const int r = launchTrace(c, fp, s, q, numTiles * 4u, true, tilesX, tilesY, c->traceGrid[3], -1, nullptr, nullptr, 2, true); if (r) return r; }
      const LightPickAddArgs PD{q.rays, q.hits, q.binCount, G.tileWords, P.diffTerm, D.sumRefl, D.sumDiff};
      launch(lightPickVisAddKernel, dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, PD, (uint32_t*)R.next);
      RT_HIP(hipGetLastError());
    } else if (P.list.castMask) {
      launch(kLightPickGen[pickVariant(c)], dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, P);
      { const int r = launchTrace(c, fp, s, q, numTiles * 4u, true, tilesX, tilesY, c->traceGrid[3], -1, nullptr, nullptr, 2, true); if (r) return r; }
      const LightPickAddArgs PD{q.rays, q.hits, q.binCount, G.tileWords, P.diffTerm, D.sumRefl, D.sumDiff};
      launch(lightPickAddKernel, dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, PD);
      RT_HIP(hipGetLastError());
    }
    return launchSunHitResolve(c, s, c->lightSums, G.tileWords, tilesX, rb, re, nullptr);
  }
  for (uint32_t i = 0; i < c->lights.count; ++i) {
    const RtggxLight& l = c->lights.l[i];
    if (!lightCastsRays(l)) continue;
    G.light = lightArgs(l); G.slot = RT_SLOT_LIGHT(i);
    launch(kLightGen[lightVariant(l)], dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, G);
    // the sun's launch (launchSun): spill part 2
    { const int r = launchTrace(c, fp, s, q, numTiles * 4u, true, tilesX, tilesY, c->traceGrid[3], -1, nullptr, nullptr, 2, true); if (r) return r; }
    D.Ix = G.light.Ix; D.Iy = G.light.Iy; D.Iz = G.light.Iz;
    launch(lightAddKernel, dim3(numTiles), dim3(256), s, nullptr, nullptr, dfp, D);
    RT_HIP(hipGetLastError());
  }
  return launchSunHitResolve(c, s, c->lightSums, G.tileWords, tilesX, rb, re, nullptr);
}

// ---- the sun and the lights at the surfaces the paths hit (rtggx_set_sun_reflections, rtggx_set_light_reflections) -----------------------------
// In front of EVERY level's shading pass, on the stream that shades: a spawning pass compacts the next level's rays into the bin in place, so
// the hits are read first -- the sun's pass, then per light, in index order, the lights'.  A generating kernel walks the wave's bin as
// shadeKernel does (a bin of 128 takes two rounds) and compacts one shadow ray per lit hit into the same bin of a queue of the feature's own:
// origin the hit point, skip the hit triangle, weight the finished s = T_d term, flags the image the path writes.  sunHitAddKernel (a record
// carries all it reads) adds an unoccluded ray's weight to the pixel's sum -- S (one sample: sunHitSums, resolved into the packed words
// behind the last shading pass by sunHitResolveKernel) or the sample sums resolveSamplesKernel packs (N > 1).  A pass holds at most one
// live path per (pixel, image): the order of a sum is sun, then the lights ascending, level by level.
struct HitBinArgs {
  const RayRec* rays; const HitKey* hits; const uint32_t* binCount; uint32_t binSlots;      // the frame's bins, this level's rays and their hits
  const float4* fat0; const float4* fat1;
};
struct SunHitGenArgs : HitBinArgs {
  RayRec* outRays; HitKey* outHits; uint32_t* outCount;                                     // the feature's queue: the same bins, binSlots slots each
  const uint32_t* tileWords;
  float Lx, Ly, Lz, Ex, Ey, Ez;
};
struct SunHitGenArgsSoft : SunHitGenArgs { SunDiskArgs disk; };      // the frame index of the sample the pass belongs to, RT_SLOT_SUN_HIT(d)
template <bool SOFT>
__global__ void __launch_bounds__(256) sunHitGenKernel(const FrameParams* __restrict__ fpp, std::conditional_t<SOFT, SunHitGenArgsSoft, SunHitGenArgs> A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t bin = tile * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint32_t count = RT_SGPR(min(A.binCount[bin] & 0xFFu, A.binSlots));
  const f3 L = mk3(A.Lx, A.Ly, A.Lz);
  uint32_t written = 0u;      // shadow rays in the front of the bin so far: never more than the records read
  for (uint32_t base = 0u; base < count; base += 64u) {
    const uint32_t i = base + lane;
    bool want = false;
    RayRec sr;
    if (i < count) atTracedHit(fp, A.rays, A.hits, A.fat0, A.fat1, (size_t)bin * A.binSlots + i, [&](const TracedHit& h) {
      const float NoL = dot3(h.N, L);
      f3 Ls = L;      // SOFT: toward the point of the disk this hit's slot draws
      bool facing = NoL > 0.0f;
      if constexpr (SOFT) { if (facing) { Ls = sunDiskDirection(A.disk, L, h.pixel, A.disk.frameIndex, A.disk.slotBase + RT_SLOT_SUN_HIT_IMAGE * h.image); facing = dot3(h.N, Ls) > 0.0f; } }
      if (facing) {
        const f3 term = hitLobeTerm(fp, h, L, NoL, mk3(A.Ex, A.Ey, A.Ez), 1.0f);
        want = true;
        sr = shadowRay(h.P(), Ls, h.pixel, h.hitId, mk3(h.q2.x * term.x, h.q2.y * term.y, h.q2.z * term.z), h.image);      // s_d = T_d * term
      }
    });
    written += compactShadowRay<false>(want, sr, RT_RAY_TMAX, A.outRays, A.outHits, nullptr, bin, A.binSlots, written, lane);
  }
  if (lane == 0u) A.outCount[bin] = written;
}
struct LightHitGenArgs : HitBinArgs {
  RayRec* outRays; HitKey* outHits; uint32_t* outCount; float2* outRange;                   // the feature's queue: the same bins, binSlots slots each
  const uint32_t* tileWords;
  LightArgs light;
  const float* cosSin; uint32_t frameIndex, slotBase;      // SOFT: the 256-entry table, the frame index of the sample the pass belongs to, RT_SLOT_LIGHT_HIT(d, i)
};
template <bool CONE, bool SOFT>
__global__ void __launch_bounds__(256) lightHitGenKernel(const FrameParams* __restrict__ fpp, LightHitGenArgs A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t bin = tile * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint32_t count = RT_SGPR(min(A.binCount[bin] & 0xFFu, A.binSlots));
  uint32_t written = 0u;      // shadow rays in the front of the bin so far: never more than the records read
  for (uint32_t base = 0u; base < count; base += 64u) {
    const uint32_t i = base + lane;
    bool want = false;
    RayRec sr;
    float tmax = 0.0f;
    if (i < count) atTracedHit(fp, A.rays, A.hits, A.fat0, A.fat1, (size_t)bin * A.binSlots + i, [&](const TracedHit& h) {
      evalLight<CONE, SOFT>(A.light, A.cosSin, h.P(), h.N, h.pixel, A.frameIndex, A.slotBase + RT_SLOT_LIGHT_HIT_IMAGE * h.image, [&](const LightSample& l) {
      const f3 term = hitLobeTerm(fp, h, l.L, l.NoL, mk3(A.light.Ix, A.light.Iy, A.light.Iz), l.att);
      want = true;
      tmax = l.tmax;
      sr = shadowRay(h.P(), l.Ls, h.pixel, h.hitId, mk3(h.q2.x * term.x, h.q2.y * term.y, h.q2.z * term.z), h.image);      // s = T_d * term
    }); });
    written += compactShadowRay<true>(want, sr, tmax, A.outRays, A.outHits, A.outRange, bin, A.binSlots, written, lane);
  }
  if (lane == 0u) A.outCount[bin] = written;
}
static void (*const kLightHitGen[4])(const FrameParams*, LightHitGenArgs) = {lightHitGenKernel<false, false>, lightHitGenKernel<false, true>, lightHitGenKernel<true, false>, lightHitGenKernel<true, true>};
// rtggx_set_light_sampling(ctx, 1) at the hits: lightHitGenKernel's walk of the bin with lightPickGenKernel's pick -- the weight of light i is
// the luminance of the finished s_i = T_d term_i, the draw's slot RT_SLOT_LIGHT_PICK_HIT(level) + img, the record's weight s_i f
struct LightHitPickGenArgs : HitBinArgs {
  RayRec* outRays; HitKey* outHits; uint32_t* outCount; float2* outRange;                   // the feature's queue: the same bins, binSlots slots each
  const uint32_t* tileWords;
  uint32_t frameIndex, level;      // the frame index of the sample the pass belongs to
  LightListArgs list;
};
// Steps 1 and 4-5 of rtggx_set_light_reflections for one light at a hit, without the target: s = T_d term (0 where the light does not reach)
template <bool CONE>
RT_DEV f3 hitPickTerm(const FrameParams& fp, const LightArgs& K, const TracedHit& h, f3 P) {
  f3 s = mk3(0.0f, 0.0f, 0.0f);
  evalLight<CONE, false>(K, nullptr, P, h.N, 0u, 0u, 0u, [&](const LightSample& l) {
    const f3 term = hitLobeTerm(fp, h, l.L, l.NoL, mk3(K.Ix, K.Iy, K.Iz), l.att);
    s = mk3(h.q2.x * term.x, h.q2.y * term.y, h.q2.z * term.z);
  });
  return s;
}
template <bool CONE, bool SOFT>
__global__ void __launch_bounds__(256) lightHitPickGenKernel(const FrameParams* __restrict__ fpp, LightHitPickGenArgs A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t bin = tile * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint32_t count = RT_SGPR(min(A.binCount[bin] & 0xFFu, A.binSlots));
  uint32_t written = 0u;      // shadow rays in the front of the bin so far: never more than the records read
  for (uint32_t base = 0u; base < count; base += 64u) {
    const uint32_t i = base + lane;
    bool want = false;
    RayRec sr;
    float tmax = 0.0f;
    if (i < count) atTracedHit(fp, A.rays, A.hits, A.fat0, A.fat1, (size_t)bin * A.binSlots + i, [&](const TracedHit& h) {
      const f3 P = h.P();
      float w[RTGGX_MAX_LIGHTS];
      float W = 0.0f;
#pragma unroll
      for (uint32_t k = 0; k < RTGGX_MAX_LIGHTS; ++k) {
        w[k] = 0.0f;
        if ((A.list.castMask >> k) & 1u) {
          const float y = pickLuminance(hitPickTerm<CONE>(fp, A.list.light[k], h, P));
          w[k] = y > 0.0f ? y : 0.0f;      // (a NaN is no candidate)
        }
        W = W + w[k];
      }
      if (!(W > 0.0f)) return;
      const float t = pickDraw(h.pixel, A.frameIndex, RT_SLOT_LIGHT_PICK_HIT(A.level) + RT_SLOT_LIGHT_PICK_HIT_IMAGE * h.image) * W;
      float wc = 0.0f;
      const uint32_t chosen = pickLight(w, t, wc);
      const float f = W / wc;
      const LightArgs K = chosenLight(A.list, chosen);
      LightSample l;
      if (!chosenLightSample<CONE, SOFT>(K, A.list.cosSin, P, h.N, h.pixel, A.frameIndex, RT_SLOT_LIGHT_HIT(A.level, chosen) + RT_SLOT_LIGHT_HIT_IMAGE * h.image, l)) return;
      const f3 s = hitPickTerm<CONE>(fp, K, h, P);
      want = true;
      tmax = l.tmax;
      sr = shadowRay(P, l.Ls, h.pixel, h.hitId, mk3(s.x * f, s.y * f, s.z * f), h.image);
    });
    written += compactShadowRay<true>(want, sr, tmax, A.outRays, A.outHits, A.outRange, bin, A.binSlots, written, lane);
  }
  if (lane == 0u) A.outCount[bin] = written;
}
static void (*const kLightHitPickGen[4])(const FrameParams*, LightHitPickGenArgs) = {lightHitPickGenKernel<false, false>, lightHitPickGenKernel<false, true>, lightHitPickGenKernel<true, false>, lightHitPickGenKernel<true, true>};

// ---- a light list beyond eight (rtggx_set_light_list; DESIGN.md section 9 "A culled light list") ---------------------------------------------
// Mode 1's rule over up to RTGGX_MAX_LIGHT_LIST lights that live in device memory: 64-byte records (LightArgs, pickList's neutral cone where a
// light has none) and a packed (Pl, R) per light for the cull, R = 0 where the light casts nothing.  A wave owns an 8x8 block (the hits: one
// 64-slot round of its bin), reduces the box of its points' P across the wave and tests 64 lights per step against it, a light per lane;
// the ballot is a wave-uniform mask of the lights that are KEPT, and the wave walks its set bits -- the index is uniform, the record arrives
// by scalar loads -- while every lane adds its w_i to W.  A second walk recomputes the weights until every lane has found its light: no
// array of weights, in registers or LDS, indexed by a lane's value.  A light out of range of the whole box has w_i = +0 at each of its
// points, which leaves W and c as they are: the images are those of the walk over all lights, bit for bit (include/rtggx.h has the argument).
//   the step, written once below           who runs it
//   waveBox, keptLights                    lightListGenKernel, lightListHitGenKernel
// and from above: evalLight, primaryPickTerms, hitPickTerm, chosenLightSample, pickDraw, compactShadowRay; the adds and the resolve are mode 1's.
struct LightRecord { LightArgs k; float pad[3]; };
static_assert(sizeof(LightRecord) == 64 && sizeof(LightRecord) == sizeof(RtggxLight), "a light's record is 64 bytes");
#define RT_SLOT_LIST_FIRST 8u      // below it a light's target draws from the slots of rtggx_set_lights
#define RT_SLOT_LIST_LIGHT(i) ((i) < RT_SLOT_LIST_FIRST ? RT_SLOT_LIGHT(i) : 4096u + (i))
#define RT_SLOT_LIST_LIGHT_HIT(d, img, i) ((i) < RT_SLOT_LIST_FIRST ? RT_SLOT_LIGHT_HIT(d, i) + RT_SLOT_LIGHT_HIT_IMAGE * (img) : 8192u + 1024u * (2u * (d) + (img)) + (i))
RT_DEV float waveUniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
RT_DEV float waveMin(float v) { for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o)); return waveUniform(v); }
RT_DEV float waveMax(float v) { for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o)); return waveUniform(v); }
// The box of the points P of the wave's lanes that have one; none: (+inf, -inf), which keeps nothing
struct WaveBox { float lox, loy, loz, hix, hiy, hiz; };
RT_DEV WaveBox waveBox(bool has, f3 P) {
  const float inf = __int_as_float(0x7F800000);
  WaveBox b;
  b.lox = waveMin(has ? P.x : inf); b.loy = waveMin(has ? P.y : inf); b.loz = waveMin(has ? P.z : inf);
  b.hix = waveMax(has ? P.x : -inf); b.hiy = waveMax(has ? P.y : -inf); b.hiz = waveMax(has ? P.z : -inf);
  return b;
}
// The cull's test of lights 64 chunk .. 64 chunk + 63, a light per lane: bit l is set iff light 64 chunk + l is kept.  any: the wave has a
// point at all; cullOn = 0 (rtggx_debug_light_list_cull): every casting light is kept where it has.
RT_DEV unsigned long long keptLights(const float4* __restrict__ cull, uint32_t count, uint32_t chunk, uint32_t lane, const WaveBox& b, bool any, uint32_t cullOn) {
  const uint32_t i = chunk * 64u + lane;
  bool keep = false;
  if (i < count) {
    const float4 c = cull[i];
    const float ex = fmaxf(fmaxf(b.lox - c.x, c.x - b.hix), 0.0f), ey = fmaxf(fmaxf(b.loy - c.y, c.y - b.hiy), 0.0f), ez = fmaxf(fmaxf(b.loz - c.z, c.z - b.hiz), 0.0f);
    const float dist2 = (ex * ex + ey * ey) + ez * ez;
    const float RRm = (c.w * c.w) * 1.000244140625f;
    keep = cullOn != 0u ? dist2 < RRm : any && c.w > 0.0f;
  }
  return __ballot(keep);
}
struct LightListGenArgs {
  const unsigned long long* visDepth; const float4* fat0; const float4* fat1;
  RayRec* rays; HitKey* hits; uint32_t* binCount; float2* tRange; float4* diffTerm;      // (LightPickGenArgs)
  const uint32_t* tileWords; uint32_t tilesX, rowBegin, rowEnd;
  const float* cosSin; uint32_t* kept; uint32_t blocksX, count, cullOn;      // kept: per 8x8 block of the frame, row-major, blocksX a row
};
template <bool CONE, bool SOFT>
__global__ void __launch_bounds__(256) lightListGenKernel(const FrameParams* __restrict__ fpp, const LightRecord* __restrict__ recs, const float4* __restrict__ cull, LightListGenArgs A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t px = (tile % A.tilesX) * 16 + (wave & 1u) * 8 + (lane & 7u);
  const uint32_t py = A.rowBegin + (tile / A.tilesX) * 16 + (wave >> 1) * 8 + (lane >> 3);
  PrimarySurface S = {};
  bool covered = false;
  if (px < fp.W && py < A.rowEnd) atPrimarySurface(fp, A.visDepth, A.fat0, A.fat1, px, py, [&](const PrimarySurface& s) { S = s; covered = true; });
  const bool diffuse = S.rm.y < 1.0f;
  const WaveBox box = waveBox(covered, S.P);
  const bool any = __ballot(covered) != 0ull;
  const uint32_t chunks = (A.count + 63u) >> 6;
  // steps 1 and 2 over the kept lights, ascending: W
  float W = 0.0f;
  uint32_t kept = 0u;
  for (uint32_t chunk = 0u; chunk < chunks; ++chunk) {
    unsigned long long m = keptLights(cull, A.count, chunk, lane, box, any, A.cullOn);
    kept += (uint32_t)__popcll(m);
    while (m != 0ull) {
      const uint32_t i = RT_SGPR(chunk * 64u + (uint32_t)__builtin_ctzll(m));
      m &= m - 1ull;
      const LightArgs K = recs[i].k;
      if (covered) W = W + primaryPickTerms<CONE>(K, S, diffuse).w;      // (a weight of +0 leaves W as it is)
    }
  }
  if (lane == 0u && px < fp.W && py < A.rowEnd) A.kept[(size_t)(py >> 3) * A.blocksX + (px >> 3)] = kept;
  const bool active = covered && W > 0.0f;      // a candidate
  bool want = false, wantDiff = false;
  RayRec rr;
  float tmax = 0.0f;
  f3 S1 = mk3(0.0f, 0.0f, 0.0f);
  if (__ballot(active) != 0ull) {
    // steps 3-5: the same walk once more, until every lane has its light
    const float t = pickDraw(S.pixel, fp.g.FrameIndex, RT_SLOT_LIGHT_PICK) * W;
    float c = 0.0f, wc = 0.0f;
    uint32_t chosen = 0u;
    bool found = !active;
    for (uint32_t chunk = 0u; chunk < chunks && __ballot(!found) != 0ull; ++chunk) {
      unsigned long long m = keptLights(cull, A.count, chunk, lane, box, any, A.cullOn);
      while (m != 0ull && __ballot(!found) != 0ull) {
        const uint32_t i = RT_SGPR(chunk * 64u + (uint32_t)__builtin_ctzll(m));
        m &= m - 1ull;
        const LightArgs K = recs[i].k;
        if (!found) {
          const float w = primaryPickTerms<CONE>(K, S, diffuse).w;
          if (w > 0.0f) { c = c + w; chosen = i; wc = w; found = t < c; }
        }
      }
    }
    if (active) {      // steps 6 and 7: the chosen light once more, with its target; its record is the lane's own load
      const float f = W / wc;
      const LightArgs K = recs[chosen].k;
      LightSample l;
      if (chosenLightSample<CONE, SOFT>(K, A.cosSin, S.P, S.N, S.pixel, fp.g.FrameIndex, RT_SLOT_LIST_LIGHT(chosen), l)) {
        const PickTerms x = primaryPickTerms<CONE>(K, S, diffuse);
        want = true; wantDiff = diffuse;
        tmax = l.tmax;
        rr = shadowRay(S.P, l.Ls, S.pixel, (S.inst << 24) | S.prim, mk3(x.spec.x * f, x.spec.y * f, x.spec.z * f), 0u);
        S1 = mk3(x.diff.x * f, x.diff.y * f, x.diff.z * f);
      }
    }
  }
  const uint32_t bin = blockIdx.x * 4u + wave;
  const unsigned long long wanting = __ballot(want);      // (the slot compactShadowRay gives the lane)
  if (wantDiff) A.diffTerm[(size_t)bin * RT_BIN_MIN + (uint32_t)__popcll(wanting & ((1ull << lane) - 1ull))] = make_float4(S1.x, S1.y, S1.z, 0.0f);
  const uint32_t n = compactShadowRay<true>(want, rr, tmax, A.rays, A.hits, A.tRange, bin, RT_BIN_MIN, 0u, lane);
  if (lane == 0) A.binCount[bin] = n;
}
// The hits (rtggx_set_light_reflections with a list): lightHitPickGenKernel's walk of the bin, the box over the touched hits of one round
struct LightListHitGenArgs : HitBinArgs {
  RayRec* outRays; HitKey* outHits; uint32_t* outCount; float2* outRange;                   // the feature's queue: the same bins, binSlots slots each
  const uint32_t* tileWords;
  const float* cosSin; uint32_t frameIndex, level, count, cullOn;      // the frame index of the sample the pass belongs to
};
template <bool CONE, bool SOFT>
__global__ void __launch_bounds__(256) lightListHitGenKernel(const FrameParams* __restrict__ fpp, const LightRecord* __restrict__ recs, const float4* __restrict__ cull, LightListHitGenArgs A) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t bin = tile * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const uint32_t count = RT_SGPR(min(A.binCount[bin] & 0xFFu, A.binSlots));
  const uint32_t chunks = (A.count + 63u) >> 6;
  uint32_t written = 0u;      // shadow rays in the front of the bin so far: never more than the records read
  for (uint32_t base = 0u; base < count; base += 64u) {
    const uint32_t slot = base + lane;
    TracedHit H = {};
    bool touched = false;
    if (slot < count) atTracedHit(fp, A.rays, A.hits, A.fat0, A.fat1, (size_t)bin * A.binSlots + slot, [&](const TracedHit& h) { H = h; touched = true; });
    const f3 P = H.P();
    const WaveBox box = waveBox(touched, P);
    const bool any = __ballot(touched) != 0ull;
    float W = 0.0f;
    for (uint32_t chunk = 0u; chunk < chunks; ++chunk) {
      unsigned long long m = keptLights(cull, A.count, chunk, lane, box, any, A.cullOn);
      while (m != 0ull) {
        const uint32_t i = RT_SGPR(chunk * 64u + (uint32_t)__builtin_ctzll(m));
        m &= m - 1ull;
        const LightArgs K = recs[i].k;
        if (touched) {
          const float y = pickLuminance(hitPickTerm<CONE>(fp, K, H, P));
          W = W + (y > 0.0f ? y : 0.0f);      // (a NaN is no candidate)
        }
      }
    }
    const bool active = touched && W > 0.0f;
    bool want = false;
    RayRec sr;
    float tmax = 0.0f;
    if (__ballot(active) != 0ull) {
      const float t = pickDraw(H.pixel, A.frameIndex, RT_SLOT_LIGHT_PICK_HIT(A.level) + RT_SLOT_LIGHT_PICK_HIT_IMAGE * H.image) * W;
      float c = 0.0f, wc = 0.0f;
      uint32_t chosen = 0u;
      bool found = !active;
      for (uint32_t chunk = 0u; chunk < chunks && __ballot(!found) != 0ull; ++chunk) {
        unsigned long long m = keptLights(cull, A.count, chunk, lane, box, any, A.cullOn);
        while (m != 0ull && __ballot(!found) != 0ull) {
          const uint32_t i = RT_SGPR(chunk * 64u + (uint32_t)__builtin_ctzll(m));
          m &= m - 1ull;
          const LightArgs K = recs[i].k;
          if (!found) {
            const float w = pickLuminance(hitPickTerm<CONE>(fp, K, H, P));
            if (w > 0.0f) { c = c + w; chosen = i; wc = w; found = t < c; }
          }
        }
      }
      if (active) {
        const float f = W / wc;
        const LightArgs K = recs[chosen].k;
        LightSample l;
        if (chosenLightSample<CONE, SOFT>(K, A.cosSin, P, H.N, H.pixel, A.frameIndex, RT_SLOT_LIST_LIGHT_HIT(A.level, H.image, chosen), l)) {
          const f3 s = hitPickTerm<CONE>(fp, K, H, P);
          want = true;
          tmax = l.tmax;
          sr = shadowRay(P, l.Ls, H.pixel, H.hitId, mk3(s.x * f, s.y * f, s.z * f), H.image);
        }
      }
    }
    written += compactShadowRay<true>(want, sr, tmax, A.outRays, A.outHits, A.outRange, bin, A.binSlots, written, lane);
  }
  if (lane == 0u) A.outCount[bin] = written;
}
static void (*const kLightListGen[4])(const FrameParams*, const LightRecord*, const float4*, LightListGenArgs) = {lightListGenKernel<false, false>, lightListGenKernel<false, true>, lightListGenKernel<true, false>, lightListGenKernel<true, true>};
static void (*const kLightListHitGen[4])(const FrameParams*, const LightRecord*, const float4*, LightListHitGenArgs) = {lightListHitGenKernel<false, false>, lightListHitGenKernel<false, true>, lightListHitGenKernel<true, false>, lightListHitGenKernel<true, true>};
// ---- a list's pick and what the pixel remembers (rtggx_set_light_list_visibility; DESIGN.md section 9 "What a pixel remembers of a list") ------
// lightListGenKernel and lightPickAddKernel once more, with a sparse record per pixel (RtggxLightListVisRecord: four 16-bit entries
// (v << 10) | light, 0xFFFF free, the normal word, a stamp) in two images that alternate by the feature's own sequence number:
// lightListVisGenKernel follows the frame's velocity word as lightPickVisGenKernel does, carries the four entries where the record is the
// previous acting frame's, that instance's and of a like normal (all free otherwise), writes the pixel's own record and multiplies every
// candidate's weight by max(v_i, RTGGX_LIGHT_LIST_VIS_FLOOR), v_i = 63 where no entry names light i.  The walk's index is the wave's scalar:
// a lane finds v_i with four compares of it against the fields of its own two entry words -- nothing is indexed by a lane's value.  The
// chosen index (10 bits) travels in the shadow ray's flags word; lightListVisAddKernel moves the chosen light's v a quarter of the way to 63
// or to 0, frees the entry at 63, inserts one at 47 on the first occlusion (the lowest free slot, else in place of the greatest v), and
// adds as lightPickAddKernel does.
#define RT_LIST_VIS_FREE 0xFFFFu
// v of the entry that names light i (the lowest slot, should two name it), 63 where none does; e0: entries 0 and 1, e1: entries 2 and 3
RT_DEV uint32_t listVisOf(uint32_t e0, uint32_t e1, uint32_t i) {
  const uint32_t a = e0 & 0xFFFFu, b = e0 >> 16, c = e1 & 0xFFFFu, d = e1 >> 16;
  uint32_t v = 63u;
  v = (d != RT_LIST_VIS_FREE && (d & 1023u) == i) ? d >> 10 : v;
  v = (c != RT_LIST_VIS_FREE && (c & 1023u) == i) ? c >> 10 : v;
  v = (b != RT_LIST_VIS_FREE && (b & 1023u) == i) ? b >> 10 : v;
  v = (a != RT_LIST_VIS_FREE && (a & 1023u) == i) ? a >> 10 : v;
  return v;
}
RT_DEV float listVisWeight(uint32_t e0, uint32_t e1, uint32_t i) { return (float)max(listVisOf(e0, e1, i), RTGGX_LIGHT_LIST_VIS_FLOOR); }
// Step 6 on the two entry words for the chosen light; the four entries stay registers: every loop below has constant bounds
RT_DEV void listVisUpdate(uint32_t& e0, uint32_t& e1, uint32_t chosen, bool occluded) {
  uint32_t ent[4] = {e0 & 0xFFFFu, e0 >> 16, e1 & 0xFFFFu, e1 >> 16};
  uint32_t k = 4u, v = 63u;
#pragma unroll
  for (uint32_t j = 4u; j-- > 0u;) if (ent[j] != RT_LIST_VIS_FREE && (ent[j] & 1023u) == chosen) { k = j; v = ent[j] >> 10; }
  const uint32_t next = occluded ? v - ((v + 3u) >> 2) : v + ((63u - v + 3u) >> 2);
  uint32_t put = next == 63u ? RT_LIST_VIS_FREE : (next << 10) | chosen;
  if (k == 4u) {
    if (!occluded) return;      // believed visible and seen: nothing to record
    put = (47u << 10) | chosen;
    uint32_t most = 0u;
    bool free = false;
#pragma unroll
    for (uint32_t j = 0u; j < 4u; ++j) {
      if (free) continue;
      if (ent[j] == RT_LIST_VIS_FREE) { k = j; free = true; }
      else if (k == 4u || (ent[j] >> 10) > most) { k = j; most = ent[j] >> 10; }
    }
  }
#pragma unroll
  for (uint32_t j = 0u; j < 4u; ++j) ent[j] = j == k ? put : ent[j];
  e0 = ent[0] | (ent[1] << 16); e1 = ent[2] | (ent[3] << 16);
}
template <bool CONE, bool SOFT>
__global__ void __launch_bounds__(256) lightListVisGenKernel(const FrameParams* __restrict__ fpp, const LightRecord* __restrict__ recs, const float4* __restrict__ cull, LightListGenArgs A, LightVisArgs R) {
  const FrameParams& fp = *fpp;
  const uint32_t tile = blockIdx.x;
  if (tileIsEmpty(A.tileWords, tile)) return;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t px = (tile % A.tilesX) * 16 + (wave & 1u) * 8 + (lane & 7u);
  const uint32_t py = A.rowBegin + (tile / A.tilesX) * 16 + (wave >> 1) * 8 + (lane >> 3);
  PrimarySurface S = {};
  bool covered = false;
  if (px < fp.W && py < A.rowEnd && py < fp.H) atPrimarySurface(fp, A.visDepth, A.fat0, A.fat1, px, py, [&](const PrimarySurface& s) { S = s; covered = true; });
  const bool diffuse = S.rm.y < 1.0f;
  // step 2: the history, along the frame's own velocity; the record is written whether or not a light reaches the pixel
  uint32_t e0 = 0xFFFFFFFFu, e1 = 0xFFFFFFFFu;
  if (covered) {
    const uint32_t nrm = R.normal[S.pixel], vel = R.velocity[S.pixel];
    const float qx = floorf(((float)px + 0.5f) - f16ToF32(vel & 0xFFFFu) * (float)fp.W), qy = floorf(((float)py + 0.5f) - f16ToF32(vel >> 16) * (float)fp.H);
    if (R.history != 0u && qx >= 0.0f && qx < (float)fp.W && qy >= 0.0f && qy < (float)fp.H) {
      const uint4 rec = R.prev[(size_t)(uint32_t)qy * fp.W + (uint32_t)qx];
      if ((rec.w >> 8) == R.prevSeq && (rec.w & 0xFFu) == S.inst + 1u && (float)visNormalDot(rec.z, nrm) >= 0.9f * 1046529.0f) { e0 = rec.x; e1 = rec.y; }
    }
    R.next[S.pixel] = make_uint4(e0, e1, nrm, R.stampHigh | (S.inst + 1u));
  }
  const WaveBox box = waveBox(covered, S.P);
  const bool any = __ballot(covered) != 0ull;
  const uint32_t chunks = (A.count + 63u) >> 6;
  // steps 1 and 3 over the kept lights, ascending: U
  float U = 0.0f;
  uint32_t kept = 0u;
  for (uint32_t chunk = 0u; chunk < chunks; ++chunk) {
    unsigned long long m = keptLights(cull, A.count, chunk, lane, box, any, A.cullOn);
    kept += (uint32_t)__popcll(m);
    while (m != 0ull) {
      const uint32_t i = RT_SGPR(chunk * 64u + (uint32_t)__builtin_ctzll(m));
      m &= m - 1ull;
      const LightArgs K = recs[i].k;
      if (covered) U = U + primaryPickTerms<CONE>(K, S, diffuse).w * listVisWeight(e0, e1, i);      // (a weight of +0 leaves U as it is)
    }
  }
  if (lane == 0u && px < fp.W && py < A.rowEnd) A.kept[(size_t)(py >> 3) * A.blocksX + (px >> 3)] = kept;
  const bool active = covered && U > 0.0f;      // a candidate
  bool want = false, wantDiff = false;
  RayRec rr;
  float tmax = 0.0f;
  f3 S1 = mk3(0.0f, 0.0f, 0.0f);
  if (__ballot(active) != 0ull) {
    // step 4: the same walk once more on u, until every lane has its light
    const float t = pickDraw(S.pixel, fp.g.FrameIndex, RT_SLOT_LIGHT_PICK) * U;
    float c = 0.0f, uc = 0.0f;
    uint32_t chosen = 0u;
    bool found = !active;
    for (uint32_t chunk = 0u; chunk < chunks && __ballot(!found) != 0ull; ++chunk) {
      unsigned long long m = keptLights(cull, A.count, chunk, lane, box, any, A.cullOn);
      while (m != 0ull && __ballot(!found) != 0ull) {
        const uint32_t i = RT_SGPR(chunk * 64u + (uint32_t)__builtin_ctzll(m));
        m &= m - 1ull;
        const LightArgs K = recs[i].k;
        if (!found) {
          const float w = primaryPickTerms<CONE>(K, S, diffuse).w;
          if (w > 0.0f) { const float u = w * listVisWeight(e0, e1, i); c = c + u; chosen = i; uc = u; found = t < c; }
        }
      }
    }
    if (active) {      // step 5: the list's steps 6 and 7; the chosen index in the record's flags word, for the update
      const float f = U / uc;
      const LightArgs K = recs[chosen].k;
      LightSample l;
      if (chosenLightSample<CONE, SOFT>(K, A.cosSin, S.P, S.N, S.pixel, fp.g.FrameIndex, RT_SLOT_LIST_LIGHT(chosen), l)) {
        const PickTerms x = primaryPickTerms<CONE>(K, S, diffuse);
        want = true; wantDiff = diffuse;
        tmax = l.tmax;
        rr = shadowRay(S.P, l.Ls, S.pixel, (S.inst << 24) | S.prim, mk3(x.spec.x * f, x.spec.y * f, x.spec.z * f), chosen);
        S1 = mk3(x.diff.x * f, x.diff.y * f, x.diff.z * f);
      }
    }
  }
  const uint32_t bin = blockIdx.x * 4u + wave;
  const unsigned long long wanting = __ballot(want);      // (the slot compactShadowRay gives the lane)
  if (wantDiff) A.diffTerm[(size_t)bin * RT_BIN_MIN + (uint32_t)__popcll(wanting & ((1ull << lane) - 1ull))] = make_float4(S1.x, S1.y, S1.z, 0.0f);
  const uint32_t n = compactShadowRay<true>(want, rr, tmax, A.rays, A.hits, A.tRange, bin, RT_BIN_MIN, 0u, lane);
  if (lane == 0) A.binCount[bin] = n;
}
// lightPickAddKernel with step 6: every slot below the bin's count updates the two entry words of its pixel's own record, occluded or not
__global__ void __launch_bounds__(256) lightListVisAddKernel(const FrameParams* __restrict__ fpp, LightPickAddArgs A, uint32_t* records) {
  const FrameParams& fp = *fpp;
  if (tileIsEmpty(A.tileWords, blockIdx.x)) return;
  const uint32_t bin = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (lane >= A.binCount[bin]) return;
  const size_t k = (size_t)bin * RT_BIN_MIN + lane;
  const bool occluded = hitKeyId(A.hits[k]) != 0xFFFFFFFFu;
  const RayRec rr = A.rays[k];
  uint2* const entries = reinterpret_cast<uint2*>(records + 4u * (size_t)rr.pixel);      // the pixel's own record: no other lane has this pixel
  uint2 e = *entries;
  listVisUpdate(e.x, e.y, rr.flags & 1023u, occluded);
  *entries = e;
  if (occluded) return;      // no term
  const uint32_t inst = rr.skip >> 24;
  const float4 s0 = A.sumRefl[rr.pixel];
  A.sumRefl[rr.pixel] = make_float4(s0.x + rr.wx, s0.y + rr.wy, s0.z + rr.wz, s0.w + 1.0f);
  if (fp.mat.RoughMetals[inst][1] < 1.0f) {      // (lightAddKernel)
    const float4 d = A.diffTerm[k], s1 = A.sumDiff[rr.pixel];
    A.sumDiff[rr.pixel] = make_float4(s1.x + d.x, s1.y + d.y, s1.z + d.z, s1.w + 1.0f);
  }
}
static void (*const kLightListVisGen[4])(const FrameParams*, const LightRecord*, const float4*, LightListGenArgs, LightVisArgs) = {lightListVisGenKernel<false, false>, lightListVisGenKernel<false, true>, lightListVisGenKernel<true, false>, lightListVisGenKernel<true, true>};
// The list to the device when the setting takes effect (frame.hip rtggx_render_visibility): the records with pickList's neutral cone, the
// cull's (Pl, R) with R = 0 where a light casts nothing; how many cast, and the instance [2 cone + soft] the list runs.  A frame that still
// reads the previous list may be in flight: the caller has waited for the streams (a NEW list is a setup step; lights that move are updated in place: "moving light lists" below).
int uploadLightList(rtggx_context* c) {
  const std::vector<RtggxLight>& list = c->lightList.l;
  c->lightListCasting = 0u; c->lightListVariant = 0u;
  c->lightListFrame = false;
  c->lightListCur = c->lightListNewest = -1; c->lightListStored = c->lightList.version; c->lightListAwaitWritten = false;      // (rtggx_update_light_list: the frames read this copy again)
  c->lightListRecsCur = c->lightListCullCur = nullptr;
  if (list.empty()) return 0;
  static_assert(sizeof(LightRecord) == sizeof(LightWords) && sizeof(LightCull) == sizeof(float4), "rt_light_check.h converts into the kernels' records");
  std::vector<LightRecord> recs(list.size());
  std::vector<float4> cull(list.size());
  for (size_t i = 0; i < list.size(); ++i) {
    const RtggxLight& l = list[i];
    LightWords w, r; LightCull q;
    memcpy(&w, &l, sizeof w);
    lightConvert(w, r, q);      // (the list was checked when it was set: context.hip checkLight)
    memcpy(&recs[i], &r, sizeof r); memcpy(&cull[i], &q, sizeof q);
    if (lightCastsRays(l)) { ++c->lightListCasting; c->lightListVariant |= lightVariant(l); }
  }
  if (c->lightListCapacity < list.size()) {
    c->lightListRecs.reset(); c->lightListCull.reset();
    RT_HIP(alloc(c->lightListRecs, list.size() * 16u)); RT_HIP(alloc(c->lightListCull, list.size() * 4u));
    c->lightListCapacity = (uint32_t)list.size();
  }
  RT_HIP(hipMemcpy(c->lightListRecs, recs.data(), recs.size() * sizeof(LightRecord), hipMemcpyHostToDevice));
  RT_HIP(hipMemcpy(c->lightListCull, cull.data(), cull.size() * sizeof(float4), hipMemcpyHostToDevice));
  c->lightListRecsCur = c->lightListRecs; c->lightListCullCur = c->lightListCull;
  return 0;
}
// The blocks' kept counts (rtggx_read_light_list_counts) exist from the first frame with a list and are cleared in front of every such
// frame's primary pass: a wave that leaves on a zero tile word writes none, and a list without a casting light launches nothing.
static int clearLightListCounts(rtggx_context* c, hipStream_t s) {
  const uint32_t blocks = ((c->W + 7u) / 8u) * ((c->H + 7u) / 8u);
  if (!c->lightListKept) { RT_HIP(allocFilled(c->lightListKept, (size_t)blocks)); const int r = syncFills(true); if (r) return r; }
  RT_HIP(hipMemsetAsync(c->lightListKept, 0, (size_t)blocks * 4u, s));
  c->lightListFrame = true;
  return 0;
}
// The generating launch of the primary pass with a list, in lightPickGenKernel's place (launchLights): P's queue, rows and tiles; records:
// rtggx_set_light_list_visibility's images and sequence in an acting frame, null otherwise
static int launchLightListGen(rtggx_context* c, hipStream_t s, const LightPickGenArgs& P, uint32_t numTiles, const LightVisArgs* records) {
  const uint32_t blocksX = (c->W + 7u) / 8u;
  LightListGenArgs A;
  A.visDepth = P.visDepth; A.fat0 = P.fat0; A.fat1 = P.fat1;
  A.rays = P.rays; A.hits = P.hits; A.binCount = P.binCount; A.tRange = P.tRange; A.diffTerm = P.diffTerm;
  A.tileWords = P.tileWords; A.tilesX = P.tilesX; A.rowBegin = P.rowBegin; A.rowEnd = P.rowEnd;
  A.cosSin = c->cosSinTab; A.kept = c->lightListKept; A.blocksX = blocksX; A.count = c->lightList.count; A.cullOn = c->lightListCullOn ? 1u : 0u;
  if (records) launch(kLightListVisGen[c->lightListVariant], dim3(numTiles), dim3(256), s, nullptr, nullptr, c->dParams + c->slot,
                      (const LightRecord*)c->lightListRecsCur, (const float4*)c->lightListCullCur, A, *records);
  else launch(kLightListGen[c->lightListVariant], dim3(numTiles), dim3(256), s, nullptr, nullptr, c->dParams + c->slot,
              (const LightRecord*)c->lightListRecsCur, (const float4*)c->lightListCullCur, A);
  return 0;
}

// The frame's first use of the hit passes' queues and sums on stream s.  They exist from the first frame that has the sun or lights and the
// respective toggle on: per feature its queue at the frame's slots per bin (the bins' growth releases it: frame.hip growBins, behind a wait
// for every stream) -- the lights' with the rays' intervals --, and for one-sample frames S, which the two share.  The use is ordered behind
// the previous frame's, which may have run on another stream (small launches alternate two), as launchShadeSamples orders sppAcc.
int beginSunHits(rtggx_context* c, hipStream_t s, bool wantSums, bool sunQueue, bool lightQueue) {
  bool filled = false;
  if (!c->evSunHit) RT_HIP(create(c->evSunHit, hipEventDisableTiming));
  if (sunQueue) { const int r = c->sunHitQueue.ensure(c->numBinsMax, c->binSlots, false, filled); if (r) return r; }
  if (lightQueue) { const int r = c->lightHitQueue.ensure(c->numBinsMax, c->binSlots, true, filled); if (r) return r; }
  if (wantSums && !c->sunHitSums) { RT_HIP(allocFilled(c->sunHitSums, (size_t)c->W * c->H * 8u)); filled = true; }
  { const int r = syncFills(filled); if (r) return r; }
  if (c->sunHitStream && c->sunHitStream != s) { RT_HIP(hipEventRecord(c->evSunHit, c->sunHitStream)); RT_HIP(hipStreamWaitEvent(s, c->evSunHit, 0)); }
  c->sunHitStream = s;
  return 0;
}
// One level's hits (HitPass, rt_queue.h: the bins, their rays traced and not yet shaded) under the sun, and under the lights: the generation,
// the any-hit traversal of the feature's queue on the frame's trace grid with this stream's spill part (launchShade) -- the lights' reading
// the rays' own intervals --, the add into sumRefl / sumDiff
static int traceAndAddHits(rtggx_context* c, const FrameParams& fp, const HitPass& p, const TraceQueue& q) {
  { const int r = launchTrace(c, fp, p.s, q, c->traceGrid[0], true, c->traceGrid[1], c->traceGrid[2], c->traceGrid[3], -1, nullptr, nullptr, p.spillPart, true); if (r) return r; }
  const SunHitAddArgs D{q.rays, q.hits, q.binCount, q.binSlots, p.tileWords, p.sumRefl, p.sumDiff};
  launch(p.samples ? sunHitAddKernel<true> : sunHitAddKernel<false>, dim3(p.numTiles), dim3(256), p.s, nullptr, nullptr, D);
  RT_HIP(hipGetLastError());
  return 0;
}
int launchSunHits(rtggx_context* c, const FrameParams& fp, const HitPass& p) {
  const TraceQueue q = c->sunHitQueue.view();
  if (p.numTiles * 4u > c->numBinsMax || q.binSlots != p.bins.binSlots) { setError("rtggx_ray_trace: the queue of rtggx_set_sun_reflections does not hold %u bins of %u slots", p.numTiles * 4u, p.bins.binSlots); return -1; }
  SunHitGenArgs G;
  static_cast<HitBinArgs&>(G) = HitBinArgs{p.bins.rays, p.bins.hits, p.bins.binCount, p.bins.binSlots, p.fat0, p.fat1};
  G.outRays = (RayRec*)q.rays; G.outHits = q.hits; G.outCount = c->sunHitQueue.count;
  G.tileWords = p.tileWords;
  G.Lx = c->sun.L[0]; G.Ly = c->sun.L[1]; G.Lz = c->sun.L[2]; G.Ex = c->sun.E[0]; G.Ey = c->sun.E[1]; G.Ez = c->sun.E[2];
  if (c->sunAngle.degrees > 0.0f) {      // rtggx_set_sun_angle
    SunHitGenArgsSoft GS;
    static_cast<SunHitGenArgs&>(GS) = G;
    GS.disk = sunDisk(c, p.frameIndex, RT_SLOT_SUN_HIT(p.level));
    launch(sunHitGenKernel<true>, dim3(p.numTiles), dim3(256), p.s, nullptr, nullptr, c->dParams + c->slot, GS);
  } else launch(sunHitGenKernel<false>, dim3(p.numTiles), dim3(256), p.s, nullptr, nullptr, c->dParams + c->slot, G);
  return traceAndAddHits(c, fp, p, q);
}
int launchLightHits(rtggx_context* c, const FrameParams& fp, const HitPass& p) {
  const TraceQueue q = c->lightHitQueue.view();
  if (p.numTiles * 4u > c->numBinsMax || q.binSlots != p.bins.binSlots) { setError("rtggx_ray_trace: the queue of rtggx_set_light_reflections does not hold %u bins of %u slots", p.numTiles * 4u, p.bins.binSlots); return -1; }
  LightHitGenArgs G;
  static_cast<HitBinArgs&>(G) = HitBinArgs{p.bins.rays, p.bins.hits, p.bins.binCount, p.bins.binSlots, p.fat0, p.fat1};
  G.outRays = (RayRec*)q.rays; G.outHits = q.hits; G.outCount = c->lightHitQueue.count; G.outRange = (float2*)q.tRange;
  G.tileWords = p.tileWords;
  G.cosSin = c->cosSinTab; G.frameIndex = p.frameIndex;
  if (c->lightList.count) {      // rtggx_set_light_list: mode 1's launches, the generating kernel the list's
    if (!c->lightListCasting) return 0;
    LightListHitGenArgs P;
    static_cast<HitBinArgs&>(P) = G;
    P.outRays = G.outRays; P.outHits = G.outHits; P.outCount = G.outCount; P.outRange = G.outRange;
    P.tileWords = G.tileWords;
    P.cosSin = G.cosSin; P.frameIndex = p.frameIndex; P.level = p.level; P.count = c->lightList.count; P.cullOn = c->lightListCullOn ? 1u : 0u;
    launch(kLightListHitGen[c->lightListVariant], dim3(p.numTiles), dim3(256), p.s, nullptr, nullptr, c->dParams + c->slot,
           (const LightRecord*)c->lightListRecsCur, (const float4*)c->lightListCullCur, P);
    return traceAndAddHits(c, fp, p, q);
  }
  if (c->lightSampling == 1u) {      // rtggx_set_light_sampling: one generating launch, one traversal, one add for the whole list
    LightHitPickGenArgs P;
    static_cast<HitBinArgs&>(P) = G;
    P.outRays = G.outRays; P.outHits = G.outHits; P.outCount = G.outCount; P.outRange = G.outRange;
    P.tileWords = G.tileWords;
    P.frameIndex = p.frameIndex; P.level = p.level;
    P.list = pickList(c);
    if (!P.list.castMask) return 0;
    launch(kLightHitPickGen[pickVariant(c)], dim3(p.numTiles), dim3(256), p.s, nullptr, nullptr, c->dParams + c->slot, P);
    return traceAndAddHits(c, fp, p, q);
  }
  for (uint32_t i = 0; i < c->lights.count; ++i) {
    const RtggxLight& l = c->lights.l[i];
    if (!lightCastsRays(l)) continue;
    G.light = lightArgs(l); G.slotBase = RT_SLOT_LIGHT_HIT(p.level, i);
    launch(kLightHitGen[lightVariant(l)], dim3(p.numTiles), dim3(256), p.s, nullptr, nullptr, c->dParams + c->slot, G);
    { const int r = traceAndAddHits(c, fp, p, q); if (r) return r; }
  }
  return 0;
}


// ---- moving light lists (rtggx_update_light_list, rtggx_update_light_list_device; DESIGN.md section 9 "Moving light lists") -----------------
// Only WHICH list a frame reads is new: the cull, the pick, the slots and the records' update above are untouched, and take their recs /
// cull pointers from the frame's version (rtggx_context::lightListRecsCur / CullCur).  A version is written once, in call order, on
// whatever streams the calls name; every write waits for the version's previous write where that ran on another stream and records
// evWritten behind itself.  The frame that takes a version lets the streams that read it wait for evWritten (frame.hip
// rtggx_ray_trace) and records evRead behind its last pass over the list; the ring's next write into the version waits for that on the
// host -- with eight versions and at most four frames in flight it has long happened.
//
// lightListPrepareKernel: the device path.  One lane per light: the 64 bytes as four 16-byte loads, rt_light_check.h's check and
// conversion, the record as four 16-byte stores and the cull entry as one.  A refused light is written in its sanitised form and counted:
// one ballot and one atomic add per wave (a workgroup is one wave).  No LDS, at most 16 workgroups.
struct LightPrepareArgs { const float4* in; float4* recs; float4* cull; unsigned long long* rejects; uint32_t count, kinds; };
__global__ void __launch_bounds__(64) lightListPrepareKernel(LightPrepareArgs A) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  bool reject = false;
  if (i < A.count) {
    const float4 a = A.in[4u * i], b = A.in[4u * i + 1u], c = A.in[4u * i + 2u], d = A.in[4u * i + 3u];
    const LightWords l = {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w}};
    LightWords r; LightCull q;
    reject = lightCheck(l, A.kinds) != LIGHT_OK;
    if (reject) lightSanitise(r, q); else lightConvert(l, r, q);
    A.recs[4u * i] = make_float4(r.w[0], r.w[1], r.w[2], r.w[3]); A.recs[4u * i + 1u] = make_float4(r.w[4], r.w[5], r.w[6], r.w[7]);
    A.recs[4u * i + 2u] = make_float4(r.w[8], r.w[9], r.w[10], r.w[11]); A.recs[4u * i + 3u] = make_float4(r.w[12], r.w[13], r.w[14], r.w[15]);
    A.cull[i] = make_float4(q.x, q.y, q.z, q.R);
  }
  const unsigned long long m = __ballot(reject);
  if (m != 0ull && threadIdx.x == 0u) atomicAdd(A.rejects, (unsigned long long)__popcll(m));
}
// casting count and variant of the frame's list: what the host knows of it, and what the device path's callers declared
static void lightListState(rtggx_context* c) {
  c->lightListCasting = 0u; c->lightListVariant = c->lightList.kinds;
  for (const RtggxLight& l : c->lightList.l) if (lightCastsRays(l)) { ++c->lightListCasting; c->lightListVariant |= lightVariant(l); }
  if (c->lightList.presumed && !c->lightListCasting) c->lightListCasting = 1u;      // presumed casting: the frame launches the list's kernels
}
static float* versionRecs(rtggx_context::LightListVersion& v) { return v.buf.get(); }
static float* versionCull(rtggx_context::LightListVersion& v, uint32_t count) { return v.buf.get() + (size_t)count * 16u; }
// The ring, at the first update of a context's life (a setup step: eight allocations of 80 KB, as many pinned, the events)
static int ensureLightListRing(rtggx_context* c) {
  if (c->lightListRingReady) return 0;
  for (auto& v : c->lightListRing) {
    RT_HIP(alloc(v.buf, (size_t)RTGGX_MAX_LIGHT_LIST * 20u)); RT_HIP(alloc(v.stage, (size_t)RTGGX_MAX_LIGHT_LIST * 20u));
    RT_HIP(create(v.evWritten, hipEventDisableTiming)); RT_HIP(create(v.evRead, hipEventDisableTiming)); RT_HIP(create(v.evCopied, hipEventDisableTiming));
  }
  c->lightListRingReady = true;
  return 0;
}
// every write into a version: behind its previous write
static int beginVersionWrite(rtggx_context::LightListVersion& v, hipStream_t s) {
  if (v.written && v.writeStream != s) RT_HIP(hipStreamWaitEvent(s, v.evWritten, 0));
  return 0;
}
static int endVersionWrite(rtggx_context::LightListVersion& v, hipStream_t s) {
  RT_HIP(hipEventRecord(v.evWritten, s));
  v.written = true; v.writeStream = s;
  return 0;
}
// The version the updates since the last rtggx_render_visibility write into, opened by the first of them on its stream s: the next of
// the ring that neither the current frame reads nor holds the newest list.  merge: it begins as a copy of the newest list (a partial
// range on a list whose values the host does not know).
static int openLightListVersion(rtggx_context* c, hipStream_t s, bool merge) {
  { const int r = ensureLightListRing(c); if (r) return r; }
  uint32_t k = c->lightListRingNext;
  while ((int)k == c->lightListCur || (int)k == c->lightListNewest) k = (k + 1u) % rtggx_context::kLightListVersions;
  c->lightListRingNext = (k + 1u) % rtggx_context::kLightListVersions;
  rtggx_context::LightListVersion& v = c->lightListRing[k];
  // its last reader, or -- a version no frame took -- its last write, has ended: in the steady state long ago
  if (v.readRecorded) RT_HIP(hipEventSynchronize(v.evRead));
  if (v.written) RT_HIP(hipEventSynchronize(v.evWritten));
  if (v.copied) RT_HIP(hipEventSynchronize(v.evCopied));
  v.written = v.readRecorded = v.copied = v.staged = false; v.writeStream = nullptr;
  const uint32_t n = c->lightListRequested.count;
  if (merge) {
    if (c->lightListNewest >= 0) {
      rtggx_context::LightListVersion& src = c->lightListRing[c->lightListNewest];
      if (src.written && src.writeStream != s) RT_HIP(hipStreamWaitEvent(s, src.evWritten, 0));
      RT_HIP(hipMemcpyAsync(v.buf.get(), src.buf.get(), (size_t)n * 80u, hipMemcpyDeviceToDevice, s));
      RT_HIP(hipEventRecord(src.evCopied, s)); src.copied = true;
    } else {      // rtggx_set_light_list's copy, written behind a wait for every stream
      RT_HIP(hipMemcpyAsync(versionRecs(v), c->lightListRecs.get(), (size_t)n * 64u, hipMemcpyDeviceToDevice, s));
      RT_HIP(hipMemcpyAsync(versionCull(v, n), c->lightListCull.get(), (size_t)n * 16u, hipMemcpyDeviceToDevice, s));
    }
    { const int r = endVersionWrite(v, s); if (r) return r; }
  }
  c->lightListPend = (int)k;
  return 0;
}
// The host path's lights that are not yet on the device (rtggx_context::lightListDirtyLo / Hi of lightListRequested), into the open
// version through its pinned staging, on s.  Where none is open one is opened: with the whole list from the host where the host knows
// it, as a copy of the newest with the range on top where it does not.
static int flushLightListUpdates(rtggx_context* c, hipStream_t s) {
  const rtggx_context::LightList& L = c->lightListRequested;
  uint32_t lo = c->lightListDirtyLo, hi = c->lightListDirtyHi;
  if (lo >= hi) return 0;
  if (c->lightListPend < 0) {
    if (!L.presumed) { lo = 0u; hi = L.count; }
    const int r = openLightListVersion(c, s, !(lo == 0u && hi == L.count)); if (r) return r;
  }
  rtggx_context::LightListVersion& v = c->lightListRing[c->lightListPend];
  if (v.staged) RT_HIP(hipEventSynchronize(v.evWritten));      // (host, device and host again between two frames: the staging is still the first copy's)
  LightWords* recs = (LightWords*)v.stage.get(); LightCull* cull = (LightCull*)(v.stage.get() + (size_t)L.count * 16u);
  for (uint32_t i = lo; i < hi; ++i) { LightWords w; memcpy(&w, &L.l[i], sizeof w); lightConvert(w, recs[i], cull[i]); }
  { const int r = beginVersionWrite(v, s); if (r) return r; }
  if (lo == 0u && hi == L.count) RT_HIP(hipMemcpyAsync(v.buf.get(), v.stage.get(), (size_t)L.count * 80u, hipMemcpyHostToDevice, s));
  else {
    RT_HIP(hipMemcpyAsync(versionRecs(v) + (size_t)lo * 16u, recs + lo, (size_t)(hi - lo) * 64u, hipMemcpyHostToDevice, s));
    RT_HIP(hipMemcpyAsync(versionCull(v, L.count) + (size_t)lo * 4u, cull + lo, (size_t)(hi - lo) * 16u, hipMemcpyHostToDevice, s));
  }
  v.staged = true;
  c->lightListDirtyLo = c->lightListDirtyHi = 0u;
  c->lightListStored = L.version;
  return endVersionWrite(v, s);
}
void dropLightListUpdates(rtggx_context* c) {      // (a version that was opened and is not taken: its writes are waited for when the ring comes round)
  c->lightListPend = -1; c->lightListDirtyLo = c->lightListDirtyHi = 0u;
}
// rtggx_render_visibility: the frame takes what the update calls since the last frame left -- the host's copy of the list, the version
// they opened (the host path's upload goes on s, the frame's first stream) --, or nothing: then it launches and copies nothing.
int takeLightListUpdates(rtggx_context* c, hipStream_t s) {
  if (c->lightListPend < 0 && c->lightListDirtyLo >= c->lightListDirtyHi) return 0;
  { const int r = flushLightListUpdates(c, s); if (r) return r; }
  c->lightList = c->lightListRequested;
  lightListState(c);
  rtggx_context::LightListVersion& v = c->lightListRing[c->lightListPend];
  c->lightListCur = c->lightListNewest = c->lightListPend; c->lightListPend = -1;
  c->lightListRecsCur = versionRecs(v); c->lightListCullCur = versionCull(v, c->lightList.count);
  c->lightListAwaitWritten = true;
  return 0;
}
}  // namespace rt
using namespace rt;

extern "C" {
// The device path (include/rtggx.h): ordered like hipMemcpyAsync on the caller's stream -- the merge copy, where the range is partial,
// and lightListPrepareKernel run ON that stream, so what it holds precedes the read and what follows is behind it.  No host copy, no
// wait in the steady state.  A rtggx_set_light_list that has not taken effect yet is uploaded here (its whole list through the staging).
int rtggx_update_light_list_device(rtggx_context* c, const RtggxLight* device_lights, uint32_t first, uint32_t count, uint32_t kinds, void* hip_stream) {
  RT_CHECK_CTX(c);
  rtggx_context::LightList& L = c->lightListRequested;
  if (!L.count) { setError("rtggx_update_light_list_device: the context holds no light list (rtggx_set_light_list)"); return -1; }
  if (first > L.count || count > L.count - first) { setError("rtggx_update_light_list_device: lights %u .. %u of a list of %u: the count of a list never changes", first, first + count, L.count); return -1; }
  if (kinds > (RTGGX_LIGHT_KIND_RADIUS | RTGGX_LIGHT_KIND_CONE)) { setError("rtggx_update_light_list_device: kinds %u: RTGGX_LIGHT_KIND_RADIUS | RTGGX_LIGHT_KIND_CONE at the most", kinds); return -1; }
  if (!count) return 0;
  if (!device_lights) { setError("rtggx_update_light_list_device: %u lights at a null pointer", count); return -1; }
  if (((uintptr_t)device_lights & 15u) != 0u) { setError("rtggx_update_light_list_device: the lights at %p: aligned to 16 bytes", (const void*)device_lights); return -1; }
  const hipStream_t s = (hipStream_t)hip_stream;
  if (!c->lightListRejects) { RT_HIP(allocFilled(c->lightListRejects, 1)); const int r = syncFills(true); if (r) return r; }
  if (L.version != c->lightListStored) { dropLightListUpdates(c); c->lightListDirtyLo = 0u; c->lightListDirtyHi = L.count; }      // a list set and not yet taken: its upload, now
  { const int r = flushLightListUpdates(c, s); if (r) return r; }      // (the host path's earlier calls: call order)
  if (c->lightListPend < 0) { const int r = openLightListVersion(c, s, !(first == 0u && count == L.count)); if (r) return r; }
  rtggx_context::LightListVersion& v = c->lightListRing[c->lightListPend];
  { const int r = beginVersionWrite(v, s); if (r) return r; }
  LightPrepareArgs A;
  A.in = (const float4*)device_lights; A.recs = (float4*)versionRecs(v) + (size_t)first * 4u; A.cull = (float4*)versionCull(v, L.count) + first;
  A.rejects = c->lightListRejects.get(); A.count = count; A.kinds = kinds;
  launch(lightListPrepareKernel, dim3((count + 63u) / 64u), dim3(64), s, nullptr, nullptr, A);
  RT_HIP(hipGetLastError());
  { const int r = endVersionWrite(v, s); if (r) return r; }
  L.kinds |= kinds; L.presumed = true;
  c->lightListStored = L.version;
  return 0;
}
// The list the last frame read, as the kernels see it, behind everything the context has enqueued and behind the version's last write
int rtggx_read_light_list(rtggx_context* c, RtggxLight* out, size_t bytes) {
  RT_CHECK_CTX(c);
  if (!c->lightList.count || !c->lightListRecsCur) { setError("rtggx_read_light_list: no list yet: it exists from the first frame with a list (rtggx_set_light_list)"); return -1; }
  const size_t want = (size_t)c->lightList.count * sizeof(RtggxLight);
  if (!out || bytes != want) { setError("rtggx_read_light_list: %zu bytes at %p: %u lights of 64 bytes are %zu", bytes, (void*)out, c->lightList.count, want); return -1; }
  RT_HIP(syncStreams(c));
  if (c->lightListCur >= 0 && c->lightListRing[c->lightListCur].written) RT_HIP(hipEventSynchronize(c->lightListRing[c->lightListCur].evWritten));
  RT_HIP(hipMemcpy(out, c->lightListRecsCur, want, hipMemcpyDeviceToHost));
  return 0;
}
// The device path's refused lights since the last reset, behind every lightListPrepareKernel enqueued so far
int rtggx_read_light_list_rejects(rtggx_context* c, uint64_t* rejects, int reset) {
  RT_CHECK_CTX(c);
  if (!rejects) { setError("rtggx_read_light_list_rejects: a null pointer"); return -1; }
  if (reset != 0 && reset != 1) { setError("rtggx_read_light_list_rejects: reset %d: 0 or 1", reset); return -1; }
  RT_HIP(syncStreams(c));
  unsigned long long n = 0ull;
  if (c->lightListRejects) {
    for (auto& v : c->lightListRing) if (v.written) RT_HIP(hipEventSynchronize(v.evWritten));      // (the callers' streams are not the context's)
    RT_HIP(hipMemcpy(&n, c->lightListRejects.get(), sizeof n, hipMemcpyDeviceToHost));
    if (reset && n) { const unsigned long long zero = 0ull; RT_HIP(hipMemcpy(c->lightListRejects.get(), &zero, sizeof zero, hipMemcpyHostToDevice)); }
  }
  *rejects = (uint64_t)n;
  return 0;
}
}  // extern "C"
