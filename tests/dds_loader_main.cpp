// Stand-alone driver of host/DDSLoader.h for tests/test_bc6h_host.py, which builds it plain and with -fsanitize=address,undefined and runs
// it as a child process over files it wrote: well-formed cube maps of every accepted kind and malformed ones.  One line per file: what the
// loader returned -- format, size, mips, payload bytes and the payload's FNV-1a checksum -- or the reason it gave for refusing the file.  A
// file that is refused without a reason, or accepted with a payload of another length than the header implies, ends the run with status 1.
#include <cstdio>
#include <string>
#include "../raytracedggx_amd/host/DDSLoader.h"

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <file.dds> ...\n", argv[0]); return 2; }
  for (int a = 1; a < argc; ++a) {
    const char* slash = std::strrchr(argv[a], '/');
    const char* name = slash ? slash + 1 : argv[a];
    DDS::Loader loader; DDS::CubeImage cube; std::string error;
    if (!loader.LoadCubeFromFile(argv[a], cube, error)) {
      if (error.empty()) { std::fprintf(stderr, "%s: refused without a reason\n", name); return 1; }
      if (!cube.payload.empty()) { std::fprintf(stderr, "%s: refused, but a payload was left behind\n", name); return 1; }
      std::printf("%s: error: %s\n", name, error.c_str());
      continue;
    }
    size_t want = 0;
    for (uint32_t m = 0; m < cube.mips; ++m) {
      const size_t s = (cube.size >> m) ? (cube.size >> m) : 1;
      want += (cube.format == 95 || cube.format == 96) ? ((s + 3) / 4) * ((s + 3) / 4) * 16 : s * s * (cube.format == 10 ? 8 : 16);
    }
    if (cube.payload.size() != want * 6) { std::fprintf(stderr, "%s: %zu payload bytes, the header implies %zu\n", name, cube.payload.size(), want * 6); return 1; }
    uint32_t h = 0x811C9DC5u;
    for (uint8_t b : cube.payload) h = (h ^ b) * 0x01000193u;
    std::printf("%s: format %d size %u mips %u bytes %zu fnv %08x\n", name, cube.format, cube.size, cube.mips, cube.payload.size(), h);
  }
  return 0;
}
