// What a surface is made of, for the kernels that derive one: the device functions raytrace.hip (ray generation, hit shading) and lighting.hip
// (the sun, the local lights) both call -- Material.hlsli, the BRDF terms of BRDFModels.hlsli, the hash and the triangle / attribute
// helpers of RayTracing.hlsl.  The objects are compiled separately, without relocatable device code: everything here is an inline device
// function, and each file's kernels get their own copy.
#pragma once
#include "rtggx_device.h"

namespace rt {

#define RT_PI 3.1415926535897f   // BRDFModels.hlsli:5
#define RT_SGPR(v) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(v)))      // a workgroup-uniform value the compiler may have computed in vector registers

// ---- Material.hlsli -----------------------------------------------------------------------------------
RT_DEV f2 getUV(f3 n, f3 p, f3 scl) {   // :16-23
  f2 uv; uv.x = fabsf(n.x) * p.y * scl.y; uv.y = fabsf(n.x) * p.z * scl.z;
  uv.x += fabsf(n.y) * p.z * scl.z; uv.y += fabsf(n.y) * p.x * scl.x;
  uv.x += fabsf(n.z) * p.x * scl.x; uv.y += fabsf(n.z) * p.y * scl.y;
  uv.x = uv.x * 0.5f + 0.5f; uv.y = uv.y * 0.5f + 0.5f;
  return uv;
}
RT_DEV f2 getRoughMetal(const RtggxCBMaterial& mat, uint32_t inst, f2 uv) {   // :30-48
  float rough = mat.RoughMetals[inst][0];
  if (inst == 0) {
    const uint32_t px = ftou(uv.x * 5.0f) & 1u, py = ftou(uv.y * 5.0f) & 1u;
    rough = (px ^ py) ? rough * 0.25f : rough;
  }
  f2 r; r.x = rough; r.y = mat.RoughMetals[inst][1];
  return r;
}

// ---- BRDFModels.hlsli ---------------------------------------------------------------------------------
RT_DEV float visSmith(float roughness, float NoV, float NoL) {   // :30-39
  const float a = roughness * roughness, a2 = a * a;
  const float v = NoV + sqrtf(NoV * (NoV - NoV * a2) + a2);
  const float l = NoL + sqrtf(NoL * (NoL - NoL * a2) + a2);
  return 1.0f / (v * l);
}
RT_DEV f3 fSchlick(f3 spec, float VoH) {   // :54-62, pow(x,5) by multiplication
  const float x = 1.0f - VoH, x2 = x * x;
  const float fc = (x2 * x2) * x;
  const float s = saturatef(50.0f * spec.y) * fc;
  return mk3(s + (1.0f - fc) * spec.x, s + (1.0f - fc) * spec.y, s + (1.0f - fc) * spec.z);
}
RT_DEV f3 envBRDFApprox(f3 spec, float roughness, float NoV) {   // :64-77
  const float rx = roughness * -1.0f + 1.0f, ry = roughness * -0.0275f + 0.0425f;
  const float rz = roughness * -0.572f + 1.04f, rw = roughness * 0.022f + -0.04f;
  const float a004 = fminf(rx * rx, exp2Contract(-9.28f * NoV)) * rx + ry;
  const float ABx = -1.04f * a004 + rz;
  float ABy = 1.04f * a004 + rw;
  ABy *= saturatef(50.0f * spec.y);
  return mk3(spec.x * ABx + ABy, spec.y * ABx + ABy, spec.z * ABx + ABy);
}

// ---- RayTracing.hlsl helpers ---------------------------------------------------------------------------
RT_DEV uint32_t rng(uint32_t seed) {   // :379-387
  seed = seed * 747796405u + 1u;
  seed = ((seed >> ((seed >> 28) + 4u)) ^ seed) * 277803737u;
  seed = (seed >> 22) ^ seed;
  return seed;
}
struct Tri3 { f3 pos[3], nrm[3]; };
RT_DEV Tri3 getVertices(const float4* __restrict__ fat, uint32_t prim) {   // :230-244, from the primitive's fat triangle (rtggx_context.h): five 16-byte loads, one dependent step
  const float4* p = fat + 5 * (size_t)prim;
  const float4 a = p[0], b = p[1], c = p[2], d = p[3], e = p[4];
  Tri3 v;
  v.pos[0] = mk3(a.x, a.y, a.z); v.nrm[0] = mk3(a.w, b.x, b.y);
  v.pos[1] = mk3(b.z, b.w, c.x); v.nrm[1] = mk3(c.y, c.z, c.w);
  v.pos[2] = mk3(d.x, d.y, d.z); v.nrm[2] = mk3(d.w, e.x, e.y);
  return v;
}
struct Attrib { f3 Pos, Nrm; f2 UV; };
RT_DEV Attrib interpAttrib(const Tri3& v, float b1, float b2) {   // :249-271
  const float w0 = 1.0f - (b1 + b2);
  Attrib a;
  a.Pos = (w0 * v.pos[0] + b1 * v.pos[1]) + b2 * v.pos[2];
  a.Nrm = (w0 * v.nrm[0] + b1 * v.nrm[1]) + b2 * v.nrm[2];
  a.UV = getUV(a.Nrm, a.Pos, mk3(1.0f, 0.2f, 1.0f));
  return a;
}
RT_DEV f2 calcBarycentrics(const f4 p[3], f2 ndc) {   // :204-225
  const f3 invW = mk3(1.0f / p[0].w, 1.0f / p[1].w, 1.0f / p[2].w);
  f2 ndc0, ndc1, ndc2;
  ndc0.x = p[0].x * invW.x; ndc0.y = p[0].y * invW.x; ndc1.x = p[1].x * invW.y; ndc1.y = p[1].y * invW.y; ndc2.x = p[2].x * invW.z; ndc2.y = p[2].y * invW.z;
  const float det = (ndc2.x - ndc1.x) * (ndc0.y - ndc1.y) - (ndc2.y - ndc1.y) * (ndc0.x - ndc1.x);
  const float invDet = 1.0f / det;
  const f3 dPdx = mk3(ndc1.y - ndc2.y, ndc2.y - ndc0.y, ndc0.y - ndc1.y) * invDet;
  const f3 dPdy = mk3(ndc2.x - ndc1.x, ndc0.x - ndc2.x, ndc1.x - ndc0.x) * invDet;
  f2 dv; dv.x = ndc.x - ndc0.x; dv.y = ndc.y - ndc0.y;
  const float interpInvW = (invW.x + dv.x * dot3(invW, dPdx)) + dv.y * dot3(invW, dPdy);
  const float interpW = 1.0f / interpInvW;
  f2 b;
  b.x = interpW * (dv.x * dPdx.y * invW.y + dv.y * dPdy.y * invW.y);
  b.y = interpW * (dv.x * dPdx.z * invW.z + dv.y * dPdy.z * invW.z);
  return b;
}

}  // namespace rt
