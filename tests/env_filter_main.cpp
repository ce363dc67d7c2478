// TEST INFRASTRUCTURE ONLY.  A program of its own around raytracedggx_amd/csrc/rt_env_filter.h (the host side of rtggx_prefilter_env: no HIP
// in it), built by tests/test_envfilter_host.py with a host compiler -- once plainly, once under AddressSanitizer and UBSan -- and run as a
// child process.
//   env_filter_main tables S N [S N ...]   for every pair and every level m = 1 .. M - 1, on stdout in binary: six uint32
//                                          (S, M, m, N, K, the bits of invW), then K x 4 uint32 (the bits of x, y, z, lod)
//   env_filter_main samples v [v ...]      per value one text line "v ok n": envFilterSamples' answer
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../raytracedggx_amd/csrc/rt_env_filter.h"

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "samples") == 0) {
    for (int i = 2; i < argc; ++i) {
      const uint32_t v = (uint32_t)std::strtoul(argv[i], nullptr, 0);
      uint32_t n = 0;
      const bool ok = rt::envFilterSamples(v, n);
      std::printf("%u %d %u\n", v, ok ? 1 : 0, n);
    }
    return 0;
  }
  if (argc >= 4 && std::strcmp(argv[1], "tables") == 0 && argc % 2 == 0) {
    for (int i = 2; i + 1 < argc; i += 2) {
      const uint32_t S = (uint32_t)std::strtoul(argv[i], nullptr, 0), N = (uint32_t)std::strtoul(argv[i + 1], nullptr, 0);
      const uint32_t M = rt::envFilterLevels(S);
      for (uint32_t m = 1; m < M; ++m) {
        const rt::EnvFilterTable t = rt::envFilterTable(S, M, m, N);
        const uint32_t head[6] = {S, M, m, N, (uint32_t)t.entries.size(), bits(t.invW)};
        if (std::fwrite(head, 4, 6, stdout) != 6) return 2;
        static_assert(sizeof(rt::EnvFilterEntry) == 16, "four floats");
        if (!t.entries.empty() && std::fwrite(t.entries.data(), 16, t.entries.size(), stdout) != t.entries.size()) return 2;
        // what the launcher relies on: the levels from M - 4 on have roughness exactly 1 and therefore one table
        if (rt::envFilterWidest(m, M) != (rt::envFilterRoughness(m, M) == 1.0)) return 3;
      }
    }
    return 0;
  }
  std::fprintf(stderr, "usage: env_filter_main tables S N [S N ...] | samples v [v ...]\n");
  return 1;
}
