// One light of a list, checked and converted, for the host and for the device (rtggx_set_lights, rtggx_set_light_list,
// rtggx_update_light_list: context.hip checkLight; rtggx_update_light_list_device: lighting.hip lightListPrepareKernel).  The header
// includes nothing of HIP: tests/light_prepare_main.cpp compiles it with a host compiler.
//   lightCheck    the refusal reason of include/rtggx.h's rule, in the order checkLight has always reported them, and 0 where the light
//                 is accepted.  Bits 8.. hold the component for LIGHT_BAD_POSITION and LIGHT_BAD_INTENSITY.  `kinds`
//                 (RTGGX_LIGHT_KIND_RADIUS | RTGGX_LIGHT_KIND_CONE) is what the caller of the device path declared: an accepted
//                 light with a radius or a cone that is not declared is a reason too.  The host passes LIGHT_KINDS_ALL.
//   lightConvert  an ACCEPTED light as the list's kernels read it: the 64-byte record (RtggxLight's layout; a cone's axis normalised in
//                 double and rounded once, the neutral cone (-2, -1) with a zero axis where there is none, the pad zero) and the cull's
//                 (Pl, R) with R = 0 where the light casts nothing.
//   lightSanitise what a refused light of the device path becomes: a light at the origin without intensity, R = 0 -- never kept, never
//                 evaluated, its index kept.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define RT_LIGHT_HD __host__ __device__
#else
#define RT_LIGHT_HD
#endif
namespace rt {
enum LightReason : uint32_t {
  LIGHT_OK = 0u, LIGHT_BAD_POSITION = 1u, LIGHT_BAD_RANGE = 2u, LIGHT_BAD_INTENSITY = 3u, LIGHT_BAD_RADIUS = 4u, LIGHT_BAD_AXIS = 5u,
  LIGHT_BAD_COSINES = 6u, LIGHT_BAD_COS_OUTER = 7u, LIGHT_UNDECLARED_RADIUS = 8u, LIGHT_UNDECLARED_CONE = 9u
};
constexpr uint32_t LIGHT_KIND_RADIUS = 1u, LIGHT_KIND_CONE = 2u, LIGHT_KINDS_ALL = 3u;      // RTGGX_LIGHT_KIND_*: the bits of the list's variant [2 cone + soft]
// the 64 bytes of RtggxLight / LightRecord as sixteen floats: 0-2 position, 3 range, 4-6 intensity, 7 radius, 8-10 axis, 11 cos_outer,
// 12 cos_inner, 13-15 pad
struct LightWords { float w[16]; };
struct LightCull { float x, y, z, R; };

RT_LIGHT_HD inline bool lightFinite(float x) { return __builtin_isfinite(x); }
RT_LIGHT_HD inline uint32_t lightCheck(const LightWords& l, uint32_t kinds) {
  for (uint32_t k = 0; k < 3u; ++k) if (!lightFinite(l.w[k])) return LIGHT_BAD_POSITION | (k << 8);
  const float range = l.w[3], radius = l.w[7], cosOuter = l.w[11], cosInner = l.w[12];
  if (!lightFinite(range) || !(range > 0.0f)) return LIGHT_BAD_RANGE;
  for (uint32_t k = 0; k < 3u; ++k) if (!lightFinite(l.w[4 + k]) || l.w[4 + k] < 0.0f) return LIGHT_BAD_INTENSITY | (k << 8);
  if (!lightFinite(radius) || radius < 0.0f || !(radius < range)) return LIGHT_BAD_RADIUS;
  if (cosOuter > -1.0f) {      // a cone; (a NaN here is no cone by this test and is refused with the last reason)
    const double x = l.w[8], y = l.w[9], z = l.w[10], len = __builtin_sqrt(x * x + y * y + z * z);
    if (!__builtin_isfinite(len) || !(len > 0.0)) return LIGHT_BAD_AXIS;
    if (!(cosOuter < cosInner && cosInner <= 1.0f)) return LIGHT_BAD_COSINES;
  } else if (!(cosOuter <= -1.0f)) return LIGHT_BAD_COS_OUTER;
  if (radius > 0.0f && !(kinds & LIGHT_KIND_RADIUS)) return LIGHT_UNDECLARED_RADIUS;
  if (cosOuter > -1.0f && !(kinds & LIGHT_KIND_CONE)) return LIGHT_UNDECLARED_CONE;
  return LIGHT_OK;
}
RT_LIGHT_HD inline bool lightCasts(const LightWords& l) { return l.w[4] > 0.0f || l.w[5] > 0.0f || l.w[6] > 0.0f; }
// the axis of an accepted cone, normalised in double and rounded once (what the context keeps of a light: checkLight)
RT_LIGHT_HD inline void lightNormaliseAxis(LightWords& l) {
  if (!(l.w[11] > -1.0f)) return;
  const double x = l.w[8], y = l.w[9], z = l.w[10], len = __builtin_sqrt(x * x + y * y + z * z);
  l.w[8] = (float)(x / len); l.w[9] = (float)(y / len); l.w[10] = (float)(z / len);
}
RT_LIGHT_HD inline void lightConvert(const LightWords& l, LightWords& rec, LightCull& cull) {
  rec = l;
  lightNormaliseAxis(rec);
  if (!(l.w[11] > -1.0f)) { rec.w[8] = rec.w[9] = rec.w[10] = 0.0f; rec.w[11] = -2.0f; rec.w[12] = -1.0f; }
  rec.w[13] = rec.w[14] = rec.w[15] = 0.0f;
  cull.x = l.w[0]; cull.y = l.w[1]; cull.z = l.w[2]; cull.R = lightCasts(l) ? l.w[3] : 0.0f;
}
RT_LIGHT_HD inline void lightSanitise(LightWords& rec, LightCull& cull) {
  for (int k = 0; k < 16; ++k) rec.w[k] = 0.0f;
  rec.w[3] = 1.0f; rec.w[11] = -2.0f; rec.w[12] = -1.0f;
  cull.x = cull.y = cull.z = cull.R = 0.0f;
}
}  // namespace rt
