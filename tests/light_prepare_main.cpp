// A program of its own around raytracedggx_amd/csrc/rt_light_check.h, the one statement of "is this light valid, and what do the list's
// kernels read of it" that the host (context.hip checkLight, lighting.hip uploadLightList) and the device (lightListPrepareKernel) share.
// The header includes nothing of HIP, so a host compiler builds this, plain and under AddressSanitizer and UBSan
// (tests/test_light_list_moving_host.py).
//   light_prepare <in> <out>
// in:  uint32 n, then n times { uint32 kinds, 16 floats: an RtggxLight }
// out: n times { uint32 reason, 16 floats: the record, 4 floats: the cull entry, 16 floats: the light as checkLight keeps it (axis
//      normalised) where it is accepted, zeros otherwise } -- a refused light in its sanitised form, as lightListPrepareKernel writes it
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../raytracedggx_amd/csrc/rt_light_check.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: light_prepare <in> <out>\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n > 65536u) { std::fprintf(stderr, "bad count\n"); return 2; }
  std::vector<uint32_t> kinds(n);
  std::vector<rt::LightWords> in(n);
  for (uint32_t i = 0; i < n; ++i)
    if (std::fread(&kinds[i], 4, 1, f) != 1 || std::fread(&in[i], sizeof(rt::LightWords), 1, f) != 1) { std::fprintf(stderr, "short input\n"); return 2; }
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  uint32_t rejects = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t reason = rt::lightCheck(in[i], kinds[i]);
    rt::LightWords rec, kept;
    rt::LightCull cull;
    std::memset(&kept, 0, sizeof kept);
    if (reason != rt::LIGHT_OK) { rt::lightSanitise(rec, cull); ++rejects; }
    else { rt::lightConvert(in[i], rec, cull); kept = in[i]; rt::lightNormaliseAxis(kept); }
    std::fwrite(&reason, 4, 1, o); std::fwrite(&rec, sizeof rec, 1, o); std::fwrite(&cull, sizeof cull, 1, o); std::fwrite(&kept, sizeof kept, 1, o);
  }
  std::fclose(o);
  std::printf("light prepare: %u lights, %u rejects\n", n, rejects);
  return 0;
}
