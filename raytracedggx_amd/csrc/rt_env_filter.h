// GGX-prefiltered environments (rtggx_prefilter_env): the host side of the filter, without HIP (plain C++17), so that
// tests/env_filter_main.cpp can print it on a CPU.  The contract is in include/rtggx.h; DESIGN.md "Prefiltered environments".
//
// Level m of a cube with M levels is the one calcCubemapMipFromRoughness picks for the roughness r(m); its texels are the radiance
// averaged over the GGX lobe of that roughness around the texel's direction, with N = V = R (the split-sum assumption).  The lobe is
// sampled by a table built here once per level: N half vectors -- the radical inverse of i for the polar angle, i / N for the azimuth --
// reflected about, kept where N.L > 0, each with the mip level of the SOURCE cube whose texel covers the solid angle the sample stands for.
// Every expression is a double operation in the order written, rounded to fp32 once: the table is a pure function of (S, M, m, N).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../include/rtggx.h"

namespace rt {

constexpr uint32_t kEnvFilterDefaultSamples = 1024u;

// rtggx_prefilter_env's argument: 0 stands for the default, anything else must be a power of two in [MIN, MAX].  False: refused.
inline bool envFilterSamples(uint32_t samples, uint32_t& n) {
  if (samples == 0u) { n = kEnvFilterDefaultSamples; return true; }
  if (samples < RTGGX_ENV_FILTER_MIN_SAMPLES || samples > RTGGX_ENV_FILTER_MAX_SAMPLES || (samples & (samples - 1u)) != 0u) return false;
  n = samples;
  return true;
}

// floor(log2(size)) + 1: the levels of a full chain (size >= 1)
inline uint32_t envFilterLevels(uint32_t size) { uint32_t mips = 1; while ((size >> mips) != 0u) ++mips; return mips; }

// The roughness whose reflection reads level m of M: the inverse of level = M - 4 + 1.15 log2(r), clamped at 1 -- every level from
// M - 4 on is the widest lobe.
inline double envFilterRoughness(uint32_t m, uint32_t M) {
  const double r = std::exp2(((double)m - ((double)M - 4.0)) / 1.15);
  return r < 1.0 ? r : 1.0;
}
// Levels with the same roughness have the same table: every m >= M - 4 (r = 1 exactly; exp2 of a non-negative number is >= 1).
inline bool envFilterWidest(uint32_t m, uint32_t M) { return m + 4u >= M; }

struct EnvFilterEntry { float x, y, z, lod; };      // L in the frame of localToWorld (z = N.L, the weight), the source level: 16 bytes
struct EnvFilterTable {
  std::vector<EnvFilterEntry> entries;      // the K kept ones, in order of i
  float invW = 0.0f;                        // 1 / sum of z
};

inline uint32_t envFilterBitReverse(uint32_t v) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0F0F0F0Fu) | ((v & 0x0F0F0F0Fu) << 4);
  v = ((v >> 8) & 0x00FF00FFu) | ((v & 0x00FF00FFu) << 8);
  return (v >> 16) | (v << 16);
}

// The table of level m (1 .. M - 1) of a cube of side S with M levels, N samples.
inline EnvFilterTable envFilterTable(uint32_t S, uint32_t M, uint32_t m, uint32_t N) {
  const double pi = 3.14159265358979323846;
  const double r = envFilterRoughness(m, M), a = r * r, a2 = a * a;
  EnvFilterTable t;
  t.entries.reserve(N);
  double sum = 0.0;
  for (uint32_t i = 0; i < N; ++i) {
    const double u = (double)envFilterBitReverse(i) / 4294967296.0;
    const double c2 = (1.0 - u) / (1.0 + (a2 - 1.0) * u);      // cos^2 of the half vector's polar angle (computeLocalDirectionGGX)
    const double z = 2.0 * c2 - 1.0;                            // N.L of L = reflect(-V, H) with V = N
    if (!(z > 0.0)) continue;
    const double ct = std::sqrt(c2), st = std::sqrt(1.0 - c2);
    const double phi = 2.0 * pi * (double)i / (double)N;
    const double x = 2.0 * ct * st * std::cos(phi), y = 2.0 * ct * st * std::sin(phi);
    const double d = (a2 - 1.0) * c2 + 1.0;
    const double pdf = a2 / (pi * d * d) / 4.0;                 // D(H) N.H / (4 V.H), N.H = V.H
    double lod = 0.5 * std::log2((6.0 * S * S) / (4.0 * pi * N * pdf)) + 1.0;      // the sample's solid angle over a level-0 texel's, one level up
    lod = std::fmin(std::fmax(lod, 0.0), (double)(M - 1u));
    const EnvFilterEntry e = {(float)x, (float)y, (float)z, (float)lod};
    t.entries.push_back(e);
    sum += (double)e.z;
  }
  t.invW = (float)(1.0 / sum);
  return t;
}

}  // namespace rt
