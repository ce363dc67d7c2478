// Stand-alone driver of host/EnvImageLoader.h for tests/test_envimage_host.py, which builds it with -fsanitize=address,undefined and runs
// it as a child process: the readers over one valid file, over every truncation of it and over the file with each byte in turn replaced by
// values that matter to a run length.  Every buffer handed to the reader is a heap block of exactly the file's size, so a read past its end
// is caught.  Exit status 0: the whole file parsed, every truncation was refused with a reason, and every corrupted file either parsed or was
// refused with a reason.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../raytracedggx_amd/host/EnvImageLoader.h"

static bool parseExact(const std::vector<uint8_t>& file, size_t n, EnvImage::Image& image, std::string& error) {
  std::unique_ptr<uint8_t[]> block(new uint8_t[n ? n : 1]);
  std::memcpy(block.get(), file.data(), n);
  return EnvImage::Parse(block.get(), n, image, error);
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <file.hdr | file.pfm>\n", argv[0]); return 2; }
  std::vector<uint8_t> file; std::string error;
  if (!EnvImage::ReadFile(argv[1], file, error)) { std::fprintf(stderr, "%s\n", error.c_str()); return 2; }
  EnvImage::Image image;
  if (!parseExact(file, file.size(), image, error)) { std::fprintf(stderr, "the whole file is refused: %s\n", error.c_str()); return 1; }
  std::printf("whole %u x %u format %d bytes %zu\n", image.width, image.height, image.pixels, image.data.size());
  size_t refused = 0;
  for (size_t n = 0; n < file.size(); ++n) {
    EnvImage::Image part; error.clear();
    if (parseExact(file, n, part, error)) { std::fprintf(stderr, "the first %zu of %zu bytes parse\n", n, file.size()); return 1; }
    if (error.empty()) { std::fprintf(stderr, "the first %zu bytes are refused without a reason\n", n); return 1; }
    ++refused;
  }
  std::printf("truncations refused %zu\n", refused);
  static const uint8_t kValues[] = {0, 1, 2, 127, 128, 129, 130, 200, 255};
  size_t parsed = 0, bad = 0;
  std::vector<uint8_t> mutated = file;
  for (size_t at = 0; at < file.size(); ++at) {
    for (uint8_t v : kValues) {
      if (file[at] == v) continue;
      mutated[at] = v;
      EnvImage::Image part; error.clear();
      if (parseExact(mutated, mutated.size(), part, error)) {
        if (part.data.size() != (size_t)part.width * part.height * (part.pixels == EnvImage::RGBE8 ? 4u : 12u)) { std::fprintf(stderr, "byte %zu = %u: the image's size and its data disagree\n", at, v); return 1; }
        ++parsed;
      } else {
        if (error.empty()) { std::fprintf(stderr, "byte %zu = %u: refused without a reason\n", at, v); return 1; }
        ++bad;
      }
    }
    mutated[at] = file[at];
  }
  std::printf("corruptions parsed %zu refused %zu\n", parsed, bad);
  return 0;
}
