// Environment images as people have them: Radiance .hdr (RGBE) and .pfm files holding a vertical or horizontal cross or a
// latitude-longitude panorama.  Only the container is read here -- the pixels go to rtggx_set_env_image untouched (RGBE8 or RGB32F, rows top
// to bottom), which builds the cube and its mip chain on the device.  No device code; every malformed or truncated file is an error string,
// never a read past the buffer.
//   Radiance: magic "#?RADIANCE" or "#?RGBE", header lines up to an empty one with FORMAT=32-bit_rle_rgbe among them, the resolution line
//             "-Y H +X W" (rows top to bottom, the orientation every writer uses), then per row a flat scanline (4 W bytes) or a new-style
//             run-length one (2 2 W_hi W_lo, then the four channels each as runs: a count above 128 repeats the next byte count - 128 times,
//             a count of 1 .. 128 copies that many bytes).  Old-style runs (a pixel 1 1 1 n repeating the one before) are refused -- and
//             with them a flat scanline that holds a real pixel with the mantissas 1 1 1, which the format cannot tell from one.
//   PFM:      "PF", width and height, a NEGATIVE scale (little-endian; its magnitude is not applied), one white-space byte, then rows bottom
//             to top of fp32 rgb: flipped here.
#pragma once
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace EnvImage {

enum Layout { EQUIRECT = 0, VCROSS = 1, HCROSS = 2 };      // RTGGX_ENV_* of rtggx.h
enum Pixels { RGBE8 = 0, RGB32F = 1 };                     // RTGGX_PIXELS_*
const uint32_t MaxSide = 16384;                            // of a source image: a vertical cross of 4096-texel cells

struct Image {
  int pixels = RGBE8;
  uint32_t width = 0, height = 0;
  std::vector<uint8_t> data;      // width x height pixels of 4 (RGBE8) or 12 (RGB32F) bytes, rows top to bottom
};

// 3:4 a vertical cross, 4:3 a horizontal one, 2:1 a panorama; anything else: -1 (the caller has to name the layout)
inline int LayoutFromAspect(uint32_t w, uint32_t h) {
  if (w == 0 || h == 0) return -1;
  if ((uint64_t)w * 4 == (uint64_t)h * 3) return VCROSS;
  if ((uint64_t)w * 3 == (uint64_t)h * 4) return HCROSS;
  if (w == 2 * (uint64_t)h) return EQUIRECT;
  return -1;
}
inline bool ParseLayoutName(const std::string& name, int& layout) {
  if (name == "equirect") layout = EQUIRECT; else if (name == "vcross") layout = VCROSS; else if (name == "hcross") layout = HCROSS; else return false;
  return true;
}

inline bool IsRadiance(const uint8_t* d, size_t n) { return n >= 2 && d[0] == '#' && d[1] == '?'; }
inline bool IsPfm(const uint8_t* d, size_t n) { return n >= 2 && d[0] == 'P' && d[1] == 'F'; }

// One header line starting at `pos` (up to, not including, '\n'; a '\r' in front of it is dropped); false at the end of the buffer.
inline bool NextLine(const uint8_t* d, size_t n, size_t& pos, std::string& line) {
  if (pos >= n) return false;
  size_t end = pos;
  while (end < n && d[end] != '\n') ++end;
  if (end == n) return false;      // a header line without its end: truncated
  line.assign(reinterpret_cast<const char*>(d) + pos, end - pos);
  if (!line.empty() && line.back() == '\r') line.pop_back();
  pos = end + 1;
  return true;
}

inline bool ParseRadiance(const uint8_t* d, size_t n, Image& out, std::string& error) {
  size_t pos = 0;
  std::string line;
  if (!NextLine(d, n, pos, line) || (line != "#?RADIANCE" && line != "#?RGBE")) { error = "not a Radiance file (no \"#?RADIANCE\" or \"#?RGBE\")"; return false; }
  bool format = false;
  for (;;) {
    if (!NextLine(d, n, pos, line)) { error = "truncated Radiance header"; return false; }
    if (line.empty()) break;
    if (line.compare(0, 7, "FORMAT=") == 0) {
      if (line != "FORMAT=32-bit_rle_rgbe") { error = "unsupported Radiance format \"" + line.substr(7, 40) + "\" (32-bit_rle_rgbe is read)"; return false; }
      format = true;
    }
  }
  if (!format) { error = "Radiance header without FORMAT=32-bit_rle_rgbe"; return false; }
  if (!NextLine(d, n, pos, line)) { error = "truncated Radiance header (no resolution line)"; return false; }
  unsigned long h = 0, w = 0; char tail = 0;
  if (line.size() > 64 || std::sscanf(line.c_str(), "-Y %lu +X %lu%c", &h, &w, &tail) != 2) { error = "Radiance resolution line \"" + line.substr(0, 40) + "\": only \"-Y H +X W\" is read"; return false; }
  if (w == 0 || h == 0 || w > MaxSide || h > MaxSide) { error = "Radiance image of " + std::to_string(w) + " x " + std::to_string(h) + " pixels: 1 .. 16384 each way"; return false; }
  const size_t W = w, H = h;
  out.pixels = RGBE8; out.width = (uint32_t)w; out.height = (uint32_t)h;
  out.data.clear();
  std::vector<uint8_t> row(4 * W);
  for (size_t y = 0; y < H; ++y) {
    const bool rle = W >= 8 && W <= 32767 && n - pos >= 4 && d[pos] == 2 && d[pos + 1] == 2 && (d[pos + 2] & 0x80u) == 0;
    if (rle) {
      if ((((size_t)d[pos + 2]) << 8 | d[pos + 3]) != W) { error = "run-length scanline " + std::to_string(y) + " has another width than the image"; return false; }
      pos += 4;
      for (int ch = 0; ch < 4; ++ch) {
        size_t x = 0;
        while (x < W) {
          if (pos >= n) { error = "truncated Radiance file (scanline " + std::to_string(y) + ")"; return false; }
          size_t count = d[pos++];
          if (count > 128) {      // a run
            count -= 128;
            if (count > W - x) { error = "run of scanline " + std::to_string(y) + " passes its end"; return false; }
            if (pos >= n) { error = "truncated Radiance file (scanline " + std::to_string(y) + ")"; return false; }
            const uint8_t v = d[pos++];
            for (size_t k = 0; k < count; ++k) row[4 * (x + k) + ch] = v;
          } else {                // literal bytes
            if (count == 0) { error = "run of length 0 in scanline " + std::to_string(y); return false; }
            if (count > W - x) { error = "run of scanline " + std::to_string(y) + " passes its end"; return false; }
            if (count > n - pos) { error = "truncated Radiance file (scanline " + std::to_string(y) + ")"; return false; }
            for (size_t k = 0; k < count; ++k) row[4 * (x + k) + ch] = d[pos + k];
            pos += count;
          }
          x += count;
        }
      }
    } else {
      if (n - pos < 4 * W) { error = "truncated Radiance file (scanline " + std::to_string(y) + ")"; return false; }
      std::memcpy(row.data(), d + pos, 4 * W);
      pos += 4 * W;
      for (size_t x = 0; x < W; ++x)
        if (row[4 * x] == 1 && row[4 * x + 1] == 1 && row[4 * x + 2] == 1) { error = "old-style run-length scanlines (scanline " + std::to_string(y) + ") are not read (a flat pixel with the mantissas 1 1 1 reads as one: Radiance's own ambiguity): rewrite the file with new-style runs"; return false; }
    }
    out.data.insert(out.data.end(), row.begin(), row.end());      // grows with what the file really holds
  }
  return true;
}

inline bool ParsePfm(const uint8_t* d, size_t n, Image& out, std::string& error) {
  // three white-space separated tokens behind "PF", then ONE white-space byte
  size_t pos = 2;
  const auto token = [&](std::string& t) {
    while (pos < n && std::isspace(d[pos])) ++pos;
    t.clear();
    while (pos < n && !std::isspace(d[pos]) && t.size() < 40) t.push_back((char)d[pos++]);
    return !t.empty() && pos < n && std::isspace(d[pos]);      // the token has ended inside the buffer
  };
  if (!IsPfm(d, n) || n < 3 || !std::isspace(d[2])) { error = "not a colour PFM file (no \"PF\")"; return false; }
  std::string tw, th, ts;
  if (!token(tw) || !token(th)) { error = "malformed PFM header (width and height)"; return false; }
  char* end = nullptr;
  const unsigned long w = std::strtoul(tw.c_str(), &end, 10); const bool wOk = *end == 0 && tw[0] != '-';
  const unsigned long h = std::strtoul(th.c_str(), &end, 10); const bool hOk = *end == 0 && th[0] != '-';
  if (!wOk || !hOk) { error = "malformed PFM header (width and height)"; return false; }
  if (!token(ts)) { error = "malformed PFM header (scale)"; return false; }
  const double scale = std::strtod(ts.c_str(), &end);
  if (*end != 0) { error = "malformed PFM header (scale)"; return false; }
  if (!(scale < 0.0)) { error = "a non-negative scale: big-endian PFM files are not read"; return false; }
  ++pos;      // the one white-space byte behind the scale
  if (w == 0 || h == 0 || w > MaxSide || h > MaxSide) { error = "PFM image of " + std::to_string(w) + " x " + std::to_string(h) + " pixels: 1 .. 16384 each way"; return false; }
  const size_t rowBytes = 12 * (size_t)w;
  if (n - pos < rowBytes * h) { error = "truncated PFM file"; return false; }
  out.pixels = RGB32F; out.width = (uint32_t)w; out.height = (uint32_t)h;
  out.data.resize(rowBytes * h);
  for (size_t y = 0; y < h; ++y) std::memcpy(out.data.data() + y * rowBytes, d + pos + (h - 1 - y) * rowBytes, rowBytes);      // bottom row first in the file
  return true;
}

// By the file's first bytes, not by its name.
inline bool Parse(const uint8_t* d, size_t n, Image& out, std::string& error) {
  if (IsRadiance(d, n)) return ParseRadiance(d, n, out, error);
  if (IsPfm(d, n)) return ParsePfm(d, n, out, error);
  error = "neither a Radiance (\"#?\") nor a PFM (\"PF\") file";
  return false;
}

inline bool ReadFile(const char* fileName, std::vector<uint8_t>& d, std::string& error) {
  FILE* f = std::fopen(fileName ? fileName : "", "rb");
  if (!f) { error = std::string("cannot open ") + (fileName ? fileName : ""); return false; }
  d.clear();
  uint8_t buf[1 << 16]; size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
  std::fclose(f);
  return true;
}

inline bool LoadFromFile(const char* fileName, Image& out, std::string& error) {
  std::vector<uint8_t> d;
  if (!ReadFile(fileName, d, error)) return false;
  if (!Parse(d.data(), d.size(), out, error)) { error = std::string(fileName) + ": " + error; return false; }
  return true;
}

}  // namespace EnvImage
