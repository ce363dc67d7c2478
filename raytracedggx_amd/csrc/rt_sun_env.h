// The sun from the environment (rtggx_sun_from_env; include/rtggx.h): the host side of the rule, without HIP (plain C++17), so that
// tests/sun_env_main.cpp can drive it on a CPU -- the arguments and their defaults, the two squared cosines, the background and its one
// rounding to binary16, the found decision, the direction and the irradiance.  The one function the kernels share with the host, a
// texel's integer direction, carries the device qualifiers only where a HIP compiler reads this file.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RT_SUN_HD __host__ __device__ inline
#else
#define RT_SUN_HD inline
#endif

namespace rt {

// Policy defaults, not measured values: a cone wide enough for a sun smeared by a probe's optics and its resampling to a cube, a ring three
// times as wide to take the sky around it from, and a peak sixteen times the mean before anything is called a sun.
constexpr float kSunEnvDefaultCone = 4.0f, kSunEnvDefaultRingFactor = 3.0f, kSunEnvDefaultContrast = 16.0f;
constexpr uint32_t kSunEnvMaxSide = 8192u;

// D = S cubeFaceDir(f, a / S, b / S) with a = 2 x + 1 - S, b = 2 y + 1 - S (raytrace.hip cubeFaceDir's signs): three integers of
// magnitude <= S, exact in a double; D . D <= 3 S^2 as well.
RT_SUN_HD void sunEnvDirection(uint32_t S, uint32_t face, uint32_t x, uint32_t y, double D[3]) {
  const double s = (double)S, a = (double)(2 * (int)x + 1 - (int)S), b = (double)(2 * (int)y + 1 - (int)S);
  switch (face) {
    case 0: D[0] = s; D[1] = -b; D[2] = -a; break;
    case 1: D[0] = -s; D[1] = -b; D[2] = a; break;
    case 2: D[0] = a; D[1] = s; D[2] = b; break;
    case 3: D[0] = a; D[1] = -s; D[2] = -b; break;
    case 4: D[0] = a; D[1] = -b; D[2] = s; break;
    default: D[0] = -a; D[1] = -b; D[2] = -s; break;
  }
}

struct SunEnvAngles { float cone, ring, minContrast; double cos2Cone, cos2Ring; };

// cos^2 of an angle given in degrees as a float: libm's cosine of the double angle, squared -- two roundings after the library's own.
inline double sunEnvCos2(float degrees) {
  const double c = std::cos((double)degrees * (3.14159265358979323846 / 180.0));
  return c * c;
}

// The arguments with 0 replaced by the defaults, or the reason they are refused (nullptr: accepted).
inline const char* sunEnvAngles(float coneDegrees, float ringDegrees, float minContrast, SunEnvAngles& out) {
  if (!(coneDegrees == coneDegrees) || !(ringDegrees == ringDegrees)) return "an angle that is not a number";
  out.cone = coneDegrees == 0.0f ? kSunEnvDefaultCone : coneDegrees;
  if (!(out.cone > 0.0f && out.cone <= 45.0f)) return "a cone outside (0, 45] degrees";
  out.ring = ringDegrees == 0.0f ? kSunEnvDefaultRingFactor * out.cone : ringDegrees;
  if (!(out.ring > out.cone && out.ring <= 89.0f)) return "a ring outside (cone, 89] degrees";
  if (!std::isfinite(minContrast) || minContrast < 0.0f) return "a contrast that is negative or not finite";
  out.minContrast = minContrast == 0.0f ? kSunEnvDefaultContrast : minContrast;
  out.cos2Cone = sunEnvCos2(out.cone); out.cos2Ring = sunEnvCos2(out.ring);
  return nullptr;
}

// fp32 -> binary16, round to nearest even, as the device's conversion (v_cvt_f16_f32) does it.  The callers here hand over values in [0, 65504].
inline uint16_t sunEnvHalf(float f) {
  uint32_t u; std::memcpy(&u, &f, 4);
  const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
  const uint32_t a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);
  if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);      // 65520 and beyond round to infinity
  if (a < 0x38800000u) {                                       // below the smallest normal half: multiples of 2^-24
    if (a < 0x33000000u) return sign;                          // below 2^-25 (2^-25 itself ties to even: zero)
    const uint32_t e = a >> 23, mant = (a & 0x7FFFFFu) | 0x800000u, sh = 126u - e;
    const uint32_t q = mant >> sh, rem = mant & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
  }
  uint32_t r = a - 0x38000000u;
  r += 0xFFFu + ((r >> 13) & 1u);
  return (uint16_t)(sign | (r >> 13));
}
inline float sunEnvHalfToFloat(uint16_t h) {      // exact; finite, non-negative halves are all the callers have
  const uint32_t e = (h >> 10) & 31u, m = h & 0x3FFu;
  if (e == 0u) return std::ldexp((float)m, -24);
  return std::ldexp((float)(m | 0x400u), (int)e - 25);
}

// background = ring_rgb / weight_ring per channel (0 with an empty ring), and b16: (float)background capped at 65504, rounded once to
// binary16 -- the level the cone's texels are cut down to, and what `excess` is measured above.
struct SunEnvBackground { double background[3]; uint16_t half[3]; float halfAsFloat[3]; };
inline SunEnvBackground sunEnvBackground(const double ringRgb[3], double weightRing) {
  SunEnvBackground b;
  for (int c = 0; c < 3; ++c) {
    b.background[c] = weightRing > 0.0 ? ringRgb[c] / weightRing : 0.0;
    float f = (float)b.background[c];
    f = f > 0.0f ? (f < 65504.0f ? f : 65504.0f) : 0.0f;
    b.half[c] = sunEnvHalf(f);
    b.halfAsFloat[c] = sunEnvHalfToFloat(b.half[c]);
  }
  return b;
}

// mean_luma = sum(w Y) / weight_all; a sun is there when the peak is not black and stands min_contrast times above that mean.
inline bool sunEnvFound(double peakLuma, double sumWY, double weightAll, float minContrast, double& meanLuma) {
  meanLuma = weightAll > 0.0 ? sumWY / weightAll : 0.0;
  return !(peakLuma == 0.0 || peakLuma < (double)minContrast * meanLuma);
}

// direction = moment / |moment|, irradiance = excess (4 pi / weight_all) -- shFinalizeKernel's normalisation; no cosine factor inside the
// cone: over a few degrees about the direction it is 1 to a part in a few hundred --, in double, each quantity rounded to fp32 once.
// False (and zeros) when |moment| is zero or not finite.
inline bool sunEnvResult(const double moment[3], const double excess[3], double weightAll, float direction[3], float irradiance[3]) {
  const double len = std::sqrt((moment[0] * moment[0] + moment[1] * moment[1]) + moment[2] * moment[2]);
  for (int c = 0; c < 3; ++c) direction[c] = irradiance[c] = 0.0f;
  if (!std::isfinite(len) || !(len > 0.0)) return false;
  const double scale = 4.0 * 3.14159265358979323846 / weightAll;
  for (int c = 0; c < 3; ++c) { direction[c] = (float)(moment[c] / len); irradiance[c] = (float)(excess[c] * scale); }
  return true;
}

}  // namespace rt
