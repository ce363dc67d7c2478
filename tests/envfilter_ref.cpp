// TEST INFRASTRUCTURE ONLY.  The CPU restatement of rtggx_prefilter_env, written from the contract in include/rtggx.h and not from
// raytracedggx_amd/csrc/rt_env_filter.h or the kernel: the whole CPU oracle (oracle/orc_capi.cpp, unchanged) and beside it
//   orc_prefilter_table(S, M, m, N, ...)   the sample table of level m, its K and invW
//   orc_prefilter_env(h, N, out)           every level of the prefiltered cube from the cube the oracle holds (which the caller has made the
//                                          source C: level 0 and the full box chain, tests/envimage_ref.py)
// The taps are the oracle's environment(), the frame its local_to_world(), the texel's direction its normalize(cube_face_dir()).  Built
// by tests/envfilter_ref.py with the flags of tests/restatement.py (-ffp-contract=off -fno-fast-math: every operation rounded on its own).
#include "../oracle/orc_capi.cpp"

namespace orc {

struct FilterEntry { float x, y, z, lod; };

static uint32_t bit_reverse32(uint32_t v) { uint32_t r = 0; for (int b = 0; b < 32; ++b) { r = (r << 1) | (v & 1u); v >>= 1; } return r; }

static uint32_t full_levels(uint32_t S) { uint32_t M = 0; while (S) { ++M; S >>= 1; } return M; }      // floor(log2 S) + 1

// Sample table of level m: the contract's expressions, double, in the order written.
static void filter_table(uint32_t S, uint32_t M, uint32_t m, uint32_t N, std::vector<FilterEntry>& kept, float& invW) {
  const double PI = 3.14159265358979323846;
  double r = std::exp2(((double)m - ((double)M - 4.0)) / 1.15);
  if (r > 1.0) r = 1.0;
  const double a = r * r;
  const double a2 = a * a;
  kept.clear();
  double W = 0.0;
  for (uint32_t i = 0; i < N; ++i) {
    const double u = (double)bit_reverse32(i) / 4294967296.0;
    const double c2 = (1.0 - u) / (1.0 + (a2 - 1.0) * u);
    const double z = 2.0 * c2 - 1.0;
    if (z > 0.0) {
      const double ct = std::sqrt(c2);
      const double st = std::sqrt(1.0 - c2);
      const double phi = 2.0 * PI * (double)i / (double)N;
      const double x = 2.0 * ct * st * std::cos(phi);
      const double y = 2.0 * ct * st * std::sin(phi);
      const double d = (a2 - 1.0) * c2 + 1.0;
      const double pdf = a2 / (PI * d * d) / 4.0;
      double lod = 0.5 * std::log2((6.0 * (double)S * (double)S) / (4.0 * PI * (double)N * pdf)) + 1.0;
      lod = std::fmin(std::fmax(lod, 0.0), (double)(M - 1));
      FilterEntry e; e.x = (float)x; e.y = (float)y; e.z = (float)z; e.lod = (float)lod;
      kept.push_back(e);
      W += (double)e.z;
    }
  }
  invW = (float)(1.0 / W);
}

// One texel: 64 partials over k = j (mod 64) ascending, then the pairwise tree, adjacent pairs first.
static uint64_t filter_texel(const Ctx& c, const std::vector<FilterEntry>& t, float invW, int face, uint32_t x, uint32_t y, uint32_t s) {
  const float u = ((float)x + 0.5f) / (float)s * 2.0f - 1.0f, v = ((float)y + 0.5f) / (float)s * 2.0f - 1.0f;
  const float3 R = normalize(cube_face_dir(face, u, v));
  float3 p[64];
  for (size_t j = 0; j < 64; ++j) {
    float3 acc = f3(0.0f, 0.0f, 0.0f);
    for (size_t k = j; k < t.size(); k += 64) {
      const float3 dir = local_to_world(R, f3(t[k].x, t[k].y, t[k].z));
      const float3 e = environment(c, dir, t[k].lod);
      acc = f3(acc.x + e.x * t[k].z, acc.y + e.y * t[k].z, acc.z + e.z * t[k].z);
    }
    p[j] = acc;
  }
  for (size_t n = 64; n > 1; n /= 2)
    for (size_t i = 0; i < n / 2; ++i) p[i] = f3(p[2 * i].x + p[2 * i + 1].x, p[2 * i].y + p[2 * i + 1].y, p[2 * i].z + p[2 * i + 1].z);
  return pack_rgba16f(std::fmin(p[0].x * invW, 65504.0f), std::fmin(p[0].y * invW, 65504.0f), std::fmin(p[0].z * invW, 65504.0f), 1.0f);
}

}  // namespace orc

// entries4: room for N x 4 floats; returns K
extern "C" uint32_t orc_prefilter_table(uint32_t S, uint32_t M, uint32_t m, uint32_t N, float* entries4, float* invW) {
  std::vector<FilterEntry> t;
  filter_table(S, M, m, N, t, *invW);
  for (size_t k = 0; k < t.size(); ++k) { entries4[4 * k] = t[k].x; entries4[4 * k + 1] = t[k].y; entries4[4 * k + 2] = t[k].z; entries4[4 * k + 3] = t[k].lod; }
  return (uint32_t)t.size();
}

// out: mip-major, six faces per mip, RGBA16F words -- the layout of RTGGX_BUF_ENV; level 0 is the oracle's own.  The oracle's cube must
// hold the full chain.  Returns 0, or -1 when it does not.
extern "C" int orc_prefilter_env(void* h, uint32_t N, uint64_t* out) {
  Ctx* c = (Ctx*)h;
  const uint32_t S = c->env.size, M = full_levels(S);
  if (S == 0 || c->env.mips != M) return -1;
  size_t at = 0;
  for (int f = 0; f < 6; ++f) { const auto& l = c->env.level[(size_t)f]; std::memcpy(out + at, l.data(), l.size() * 2); at += l.size() / 4; }
  std::vector<FilterEntry> table; float invW = 0.0f;
  for (uint32_t m = 1; m < M; ++m) {
    const uint32_t s = S >> m ? S >> m : 1u;
    filter_table(S, M, m, N, table, invW);
    uint64_t* dst = out + at;
    parallel_rows(c->threads, 6u * s, [&](uint32_t row) {
      const int face = (int)(row / s); const uint32_t y = row % s;
      for (uint32_t x = 0; x < s; ++x) dst[(size_t)row * s + x] = filter_texel(*c, table, invW, face, x, y, s);
    });
    at += 6u * (size_t)s * s;
  }
  return 0;
}
