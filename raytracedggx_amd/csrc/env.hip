// Environment map upload: the gfx950 side of DDS::Loader::CreateTextureFromFile
// (RayTracedGGX/Content/RayTracer.cpp:143-150) and of SphericalHarmonics::Transform
// (RayTracer.cpp:307-310, 345-350; XUSG/Advanced/XUSGAdvanced.h:623-648).
//
// D3D samples BC6H in texture hardware; CDNA4 has no BC6H unit, so the blocks are decoded once
// into an RGBA16F mip pyramid (mip-major, six faces per mip) that the trace kernel filters by
// hand.  BC6H_UF16 / BC6H_SF16 decode follows the published format (Direct3D 11 "BC6H format" / Khronos Data
// Format Specification, BPTC float): one lane per 4x4 block.
// SH projection: one lane per mip-0 texel, solid-angle weighted, real orthonormal basis in the
// consumer's axis convention (SHIrradianceTypeless.hlsli:23-25: x=-n.x, y=-n.y, z=n.z),
// workgroup reduction in LDS, fp64 atomics; weights normalised to 4*pi.
#include <vector>
#include <cstring>
#include "rtggx_context.h"
#include "rt_env_filter.h"

namespace rt {

// ---- BC6H mode descriptors -----------------------------------------------------------------------------
// Fields: 0 m, 1 d, then r/g/b x w/x/y/z = 2 + 4*channel + endpoint.
struct Bc6Mode { uint8_t id, transformed, regions, wbits, delta[3]; uint8_t nbits; uint8_t field[82], bit[82]; };

// Header bit streams, least significant bit first.  "f[a:b]" with a>=b is bits b..a ascending,
// with a<b it is bits b..a descending (the reversed high bits of modes 13 and 14).
static const struct { uint8_t id, transformed, regions, wbits, dr, dg, db; const char* bits; } kModeSrc[14] = {
  {0x00, 1, 2, 10, 5, 5, 5, "m1:0 gy4 by4 bz4 rw9:0 gw9:0 bw9:0 rx4:0 gz4 gy3:0 gx4:0 bz0 gz3:0 bx4:0 bz1 by3:0 ry4:0 bz2 rz4:0 bz3 d4:0"},
  {0x01, 1, 2, 7, 6, 6, 6, "m1:0 gy5 gz4 gz5 rw6:0 bz0 bz1 by4 gw6:0 by5 bz2 gy4 bw6:0 bz3 bz5 bz4 rx5:0 gy3:0 gx5:0 gz3:0 bx5:0 by3:0 ry5:0 rz5:0 d4:0"},
  {0x02, 1, 2, 11, 5, 4, 4, "m4:0 rw9:0 gw9:0 bw9:0 rx4:0 rw10 gy3:0 gx3:0 gw10 bz0 gz3:0 bx3:0 bw10 bz1 by3:0 ry4:0 bz2 rz4:0 bz3 d4:0"},
  {0x06, 1, 2, 11, 4, 5, 4, "m4:0 rw9:0 gw9:0 bw9:0 rx3:0 rw10 gz4 gy3:0 gx4:0 gw10 gz3:0 bx3:0 bw10 bz1 by3:0 ry3:0 bz0 bz2 rz3:0 gy4 bz3 d4:0"},
  {0x0a, 1, 2, 11, 4, 4, 5, "m4:0 rw9:0 gw9:0 bw9:0 rx3:0 rw10 by4 gy3:0 gx3:0 gw10 bz0 gz3:0 bx4:0 bw10 by3:0 ry3:0 bz1 bz2 rz3:0 bz4 bz3 d4:0"},
  {0x0e, 1, 2, 9, 5, 5, 5, "m4:0 rw8:0 by4 gw8:0 gy4 bw8:0 bz4 rx4:0 gz4 gy3:0 gx4:0 bz0 gz3:0 bx4:0 bz1 by3:0 ry4:0 bz2 rz4:0 bz3 d4:0"},
  {0x12, 1, 2, 8, 6, 5, 5, "m4:0 rw7:0 gz4 by4 gw7:0 bz2 gy4 bw7:0 bz3 bz4 rx5:0 gy3:0 gx4:0 bz0 gz3:0 bx4:0 bz1 by3:0 ry5:0 rz5:0 d4:0"},
  {0x16, 1, 2, 8, 5, 6, 5, "m4:0 rw7:0 bz0 by4 gw7:0 gy5 gy4 bw7:0 gz5 bz4 rx4:0 gz4 gy3:0 gx5:0 gz3:0 bx4:0 bz1 by3:0 ry4:0 bz2 rz4:0 bz3 d4:0"},
  {0x1a, 1, 2, 8, 5, 5, 6, "m4:0 rw7:0 bz1 by4 gw7:0 by5 gy4 bw7:0 bz5 bz4 rx4:0 gz4 gy3:0 gx4:0 bz0 gz3:0 bx5:0 by3:0 ry4:0 bz2 rz4:0 bz3 d4:0"},
  {0x1e, 0, 2, 6, 6, 6, 6, "m4:0 rw5:0 gz4 bz0 bz1 by4 gw5:0 gy5 by5 bz2 gy4 bw5:0 gz5 bz3 bz5 bz4 rx5:0 gy3:0 gx5:0 gz3:0 bx5:0 by3:0 ry5:0 rz5:0 d4:0"},
  {0x03, 0, 1, 10, 10, 10, 10, "m4:0 rw9:0 gw9:0 bw9:0 rx9:0 gx9:0 bx9:0"},
  {0x07, 1, 1, 11, 9, 9, 9, "m4:0 rw9:0 gw9:0 bw9:0 rx8:0 rw10 gx8:0 gw10 bx8:0 bw10"},
  {0x0b, 1, 1, 12, 8, 8, 8, "m4:0 rw9:0 gw9:0 bw9:0 rx7:0 rw10:11 gx7:0 gw10:11 bx7:0 bw10:11"},
  {0x0f, 1, 1, 16, 4, 4, 4, "m4:0 rw9:0 gw9:0 bw9:0 rx3:0 rw10:15 gx3:0 gw10:15 bx3:0 bw10:15"},
};

static void buildModeTable(std::vector<Bc6Mode>& out) {
  out.resize(14);
  for (int mi = 0; mi < 14; ++mi) {
    Bc6Mode& m = out[mi];
    std::memset(&m, 0, sizeof m);
    m.id = kModeSrc[mi].id; m.transformed = kModeSrc[mi].transformed; m.regions = kModeSrc[mi].regions; m.wbits = kModeSrc[mi].wbits;
    m.delta[0] = kModeSrc[mi].dr; m.delta[1] = kModeSrc[mi].dg; m.delta[2] = kModeSrc[mi].db;
    const char* s = kModeSrc[mi].bits;
    int n = 0;
    while (*s) {
      while (*s == ' ') ++s;
      if (!*s) break;
      int field;
      if (*s == 'm') { field = 0; ++s; } else if (*s == 'd') { field = 1; ++s; }
      else { const int ch = *s == 'r' ? 0 : (*s == 'g' ? 1 : 2); const int ep = s[1] - 'w'; field = 2 + 4 * ch + ep; s += 2; }
      int a = 0; while (*s >= '0' && *s <= '9') a = a * 10 + (*s++ - '0');
      int b = a;
      if (*s == ':') { ++s; b = 0; while (*s >= '0' && *s <= '9') b = b * 10 + (*s++ - '0'); }
      if (a >= b) for (int k = b; k <= a; ++k) { m.field[n] = (uint8_t)field; m.bit[n] = (uint8_t)k; ++n; }
      else for (int k = b; k >= a; --k) { m.field[n] = (uint8_t)field; m.bit[n] = (uint8_t)k; ++n; }
    }
    m.nbits = (uint8_t)n;
  }
}

__constant__ uint8_t kPartition2[32][16] = {
  {0,0,1,1,0,0,1,1,0,0,1,1,0,0,1,1}, {0,0,0,1,0,0,0,1,0,0,0,1,0,0,0,1}, {0,1,1,1,0,1,1,1,0,1,1,1,0,1,1,1}, {0,0,0,1,0,0,1,1,0,0,1,1,0,1,1,1},
  {0,0,0,0,0,0,0,1,0,0,0,1,0,0,1,1}, {0,0,1,1,0,1,1,1,0,1,1,1,1,1,1,1}, {0,0,0,1,0,0,1,1,0,1,1,1,1,1,1,1}, {0,0,0,0,0,0,0,1,0,0,1,1,0,1,1,1},
  {0,0,0,0,0,0,0,0,0,0,0,1,0,0,1,1}, {0,0,1,1,0,1,1,1,1,1,1,1,1,1,1,1}, {0,0,0,0,0,0,0,1,0,1,1,1,1,1,1,1}, {0,0,0,0,0,0,0,0,0,0,0,1,0,1,1,1},
  {0,0,0,1,0,1,1,1,1,1,1,1,1,1,1,1}, {0,0,0,0,0,0,0,0,1,1,1,1,1,1,1,1}, {0,0,0,0,1,1,1,1,1,1,1,1,1,1,1,1}, {0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1},
  {0,0,0,0,1,0,0,0,1,1,1,0,1,1,1,1}, {0,1,1,1,0,0,0,1,0,0,0,0,0,0,0,0}, {0,0,0,0,0,0,0,0,1,0,0,0,1,1,1,0}, {0,1,1,1,0,0,1,1,0,0,0,1,0,0,0,0},
  {0,0,1,1,0,0,0,1,0,0,0,0,0,0,0,0}, {0,0,0,0,1,0,0,0,1,1,0,0,1,1,1,0}, {0,0,0,0,0,0,0,0,1,0,0,0,1,1,0,0}, {0,1,1,1,0,0,1,1,0,0,1,1,0,0,0,1},
  {0,0,1,1,0,0,0,1,0,0,0,1,0,0,0,0}, {0,0,0,0,1,0,0,0,1,0,0,0,1,1,0,0}, {0,1,1,0,0,1,1,0,0,1,1,0,0,1,1,0}, {0,0,1,1,0,1,1,0,0,1,1,0,1,1,0,0},
  {0,0,0,1,0,1,1,1,1,1,1,0,1,0,0,0}, {0,0,0,0,1,1,1,1,1,1,1,1,0,0,0,0}, {0,1,1,1,0,0,0,1,1,0,0,0,1,1,1,0}, {0,0,1,1,1,0,0,1,1,0,0,1,1,1,0,0}};
__constant__ uint8_t kAnchor2[32] = {15,15,15,15,15,15,15,15, 15,15,15,15,15,15,15,15, 15,2,8,2,2,8,8,15, 2,8,2,2,8,8,2,2};
__constant__ int kWeight3[8] = {0, 9, 18, 27, 37, 46, 55, 64};
__constant__ int kWeight4[16] = {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64};

RT_DEV int blockBit(const uint32_t blk[4], int pos) { return (blk[pos >> 5] >> (pos & 31)) & 1; }
RT_DEV int unquantizeU(int c, int bits) {
  if (bits >= 15) return c;
  if (c == 0) return 0;
  if (c == (1 << bits) - 1) return 0xFFFF;
  return ((c << 16) + 0x8000) >> bits;
}

// BC6H_SF16: endpoints are two's-complement numbers of wbits bits; magnitudes unquantise to 15 bits, the sign is carried
RT_DEV int signExtendBits(int v, int bits) { const int m = 1 << (bits - 1); return ((v & ((1 << bits) - 1)) ^ m) - m; }
RT_DEV int unquantizeS(int c, int bits) {
  if (bits >= 16) return c;
  const bool neg = c < 0;
  if (neg) c = -c;
  int u;
  if (c == 0) u = 0;
  else if (c >= (1 << (bits - 1)) - 1) u = 0x7FFF;
  else u = ((c << 15) + 0x4000) >> (bits - 1);
  return neg ? -u : u;
}

// One lane decodes one block of one mip of one face and writes up to 16 RGBA16F texels.
__global__ void bc6hDecodeKernel(const uint32_t* __restrict__ blocks, const Bc6Mode* __restrict__ modes, uint2* __restrict__ dst,
                                 uint32_t size, uint32_t blocksPerRow, uint32_t numBlocks, int isSigned) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= numBlocks) return;
  uint32_t blk[4];
  for (int k = 0; k < 4; ++k) blk[k] = blocks[4 * (size_t)b + k];
  int modeBits = blk[0] & 3;
  if (modeBits >= 2) modeBits = blk[0] & 31;
  int mi = -1;
  for (int k = 0; k < 14; ++k) if (modes[k].id == modeBits) mi = k;
  const uint32_t bx = b % blocksPerRow, by = b / blocksPerRow;
  uint16_t px[16][3];
  if (mi < 0) { for (int i = 0; i < 16; ++i) px[i][0] = px[i][1] = px[i][2] = 0; }
  else {
    const Bc6Mode& md = modes[mi];
    int fld[14];
    for (int k = 0; k < 14; ++k) fld[k] = 0;
    for (int i = 0; i < md.nbits; ++i) fld[md.field[i]] |= blockBit(blk, i) << md.bit[i];
    int e[2][2][3];
    for (int c = 0; c < 3; ++c) {
      const int w = fld[2 + 4 * c], x = fld[3 + 4 * c], y = fld[4 + 4 * c], z = fld[5 + 4 * c];
      e[0][0][c] = w;
      if (md.transformed) {
        const int mask = (1 << md.wbits) - 1, sb = 1 << (md.delta[c] - 1);
        e[0][1][c] = (w + ((x ^ sb) - sb)) & mask;
        e[1][0][c] = (w + ((y ^ sb) - sb)) & mask;
        e[1][1][c] = (w + ((z ^ sb) - sb)) & mask;
      } else { e[0][1][c] = x; e[1][0][c] = y; e[1][1][c] = z; }
      if (isSigned) for (int r = 0; r < 2; ++r) for (int k = 0; k < 2; ++k) e[r][k][c] = signExtendBits(e[r][k][c], md.wbits);
    }
    for (int r = 0; r < 2; ++r) for (int k = 0; k < 2; ++k) for (int c = 0; c < 3; ++c)
      e[r][k][c] = isSigned ? unquantizeS(e[r][k][c], md.wbits) : unquantizeU(e[r][k][c], md.wbits);
    const int part = md.regions == 2 ? fld[1] : 0;
    const int ibits = md.regions == 2 ? 3 : 4;
    int pos = md.regions == 2 ? 82 : 65;
    for (int i = 0; i < 16; ++i) {
      const int region = md.regions == 2 ? kPartition2[part][i] : 0;
      const bool anchor = (i == 0) || (md.regions == 2 && i == kAnchor2[part]);
      const int n = anchor ? ibits - 1 : ibits;
      int idx = 0;
      for (int k = 0; k < n; ++k) idx |= blockBit(blk, pos + k) << k;
      pos += n;
      const int wgt = ibits == 3 ? kWeight3[idx] : kWeight4[idx];
      for (int c = 0; c < 3; ++c) {
        const int v = (e[region][0][c] * (64 - wgt) + e[region][1][c] * wgt + 32) >> 6;
        if (!isSigned) px[i][c] = (uint16_t)((v * 31) >> 6);
        else { const int m = v < 0 ? ((-v) * 31) >> 5 : (v * 31) >> 5; px[i][c] = (uint16_t)(v < 0 ? (0x8000 | m) : m); }
      }
    }
  }
  for (uint32_t y = 0; y < 4; ++y) for (uint32_t x = 0; x < 4; ++x) {
    const uint32_t X = bx * 4 + x, Y = by * 4 + y;
    if (X >= size || Y >= size) continue;
    const uint16_t* p = px[y * 4 + x];
    dst[(size_t)Y * size + X] = make_uint2((uint32_t)p[0] | ((uint32_t)p[1] << 16), (uint32_t)p[2] | (0x3C00u << 16));
  }
}
__global__ void f32ToF16Kernel(const float* __restrict__ src, uint2* __restrict__ dst, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = packRGBA16F(src[4 * (size_t)i], src[4 * (size_t)i + 1], src[4 * (size_t)i + 2], src[4 * (size_t)i + 3]);
}

int decodeEnv(rtggx_context* c, int format, uint32_t size, uint32_t mips, const void* hostData, size_t bytes, hipStream_t s) {
  // cubes up to 8192^2 (the reference's maxsize, RayTracer.cpp:146) with at most a full mip chain: log2(size) + 1 <= 14 levels
  if (size == 0 || size > 8192 || mips == 0 || mips > 14 || (size >> (mips - 1)) == 0) { setError("rtggx_set_env: bad size/mips (size %u, %u mips)", size, mips); return -1; }
  size_t perFace = 0; uint64_t texels = 0;
  for (uint32_t m = 0; m < mips; ++m) {
    const uint32_t sz = size >> m;
    perFace += (format == RTGGX_FORMAT_BC6H_UF16 || format == RTGGX_FORMAT_BC6H_SF16) ? (size_t)((sz + 3) / 4) * ((sz + 3) / 4) * 16 : (size_t)sz * sz * (format == RTGGX_FORMAT_RGBA16F ? 8 : 16);
    c->env.mipOffset[m] = (uint32_t)texels;
    texels += 6ull * sz * sz;
  }
  if (format != RTGGX_FORMAT_BC6H_UF16 && format != RTGGX_FORMAT_BC6H_SF16 && format != RTGGX_FORMAT_RGBA16F && format != RTGGX_FORMAT_RGBA32F) { setError("rtggx_set_env: unsupported format %d", format); return -1; }
  if (bytes < perFace * 6) { setError("rtggx_set_env: %zu bytes given, %zu needed", bytes, perFace * 6); return -1; }
  c->env.texels.reset();
  RT_HIP(alloc(c->env.texels, texels));
  c->env.size = size; c->env.mips = mips; c->env.totalTexels = texels;
  DevBuf<char> dSrc;
  RT_HIP(alloc(dSrc, perFace * 6));
  RT_HIP(hipMemcpyAsync(dSrc, hostData, perFace * 6, hipMemcpyHostToDevice, s));
  DevBuf<Bc6Mode> dModes;
  const bool bc6h = format == RTGGX_FORMAT_BC6H_UF16 || format == RTGGX_FORMAT_BC6H_SF16;
  if (bc6h) {
    std::vector<Bc6Mode> modes; buildModeTable(modes);
    RT_HIP(alloc(dModes, 14));
    RT_HIP(hipMemcpyAsync(dModes, modes.data(), sizeof(Bc6Mode) * 14, hipMemcpyHostToDevice, s));
    RT_HIP(hipStreamSynchronize(s));   // `modes` is about to go out of scope
  }
  for (uint32_t face = 0; face < 6; ++face) {
    size_t off = perFace * face;
    for (uint32_t m = 0; m < mips; ++m) {
      const uint32_t sz = size >> m;
      uint2* dst = c->env.texels + c->env.mipOffset[m] + (size_t)face * sz * sz;
      if (bc6h) {
        const uint32_t bpr = (sz + 3) / 4, nb = bpr * bpr;
        hipLaunchKernelGGL(bc6hDecodeKernel, dim3((nb + 63) / 64), dim3(64), 0, s, (const uint32_t*)((const char*)dSrc + off), dModes, dst, sz, bpr, nb, format == RTGGX_FORMAT_BC6H_SF16 ? 1 : 0);
        off += (size_t)nb * 16;
      } else if (format == RTGGX_FORMAT_RGBA16F) {
        RT_HIP(hipMemcpyAsync(dst, (const char*)dSrc + off, (size_t)sz * sz * 8, hipMemcpyDeviceToDevice, s));
        off += (size_t)sz * sz * 8;
      } else {
        hipLaunchKernelGGL(f32ToF16Kernel, dim3((sz * sz + 255) / 256), dim3(256), 0, s, (const float*)((const char*)dSrc + off), dst, sz * sz);
        off += (size_t)sz * sz * 16;
      }
    }
  }
  RT_HIP(hipGetLastError());
  RT_HIP(hipStreamSynchronize(s));
  RT_HIP(hipMemcpy(c->dEnvMipOffset, c->env.mipOffset, 16 * sizeof(uint32_t), hipMemcpyHostToDevice));
  c->shDone = false;
  return 0;
}

// ---- environments from images (rtggx_set_env_image, rtggx_generate_env_mips; DESIGN.md "Environments from images") -----------------------
// Level 0 is built on the device from a cross (a copy of six cells) or a latitude-longitude panorama (one fp64 bilinear tap per cube texel),
// the chain below it by an exact-coverage box filter, every level in fp32 from the fp32 level above and packed to RGBA16F once.  All of it
// runs at initialisation only: plain streaming kernels, one lane per texel, 64-bit indices (6 x 4096^2 texels x 16 bytes pass 2^31).

// One source pixel as fp32 rgb: RGBE8 is m 2^(e - 136) per channel (exact; e == 0: black), RGB32F the value as it is; then NaN, negatives and
// zeros become +0 and everything above the largest finite half becomes it, so that whatever follows is finite and fits a half.
RT_DEV f3 envPixel(const void* __restrict__ src, int pixels, size_t i) {
  float r, g, b;
  if (pixels == RTGGX_PIXELS_RGBE8) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(src)[i];
    const int e = (int)(w >> 24);      // bytes r, g, b, e
    r = e ? ldexpf((float)(w & 255u), e - 136) : 0.0f; g = e ? ldexpf((float)((w >> 8) & 255u), e - 136) : 0.0f; b = e ? ldexpf((float)((w >> 16) & 255u), e - 136) : 0.0f;
  } else {
    const float* p = reinterpret_cast<const float*>(src) + 3 * i;
    r = p[0]; g = p[1]; b = p[2];
  }
  return mk3(r > 0.0f ? fminf(r, 65504.0f) : 0.0f, g > 0.0f ? fminf(g, 65504.0f) : 0.0f, b > 0.0f ? fminf(b, 65504.0f) : 0.0f);
}

// Level 0 from a cross: cube texel (face, y, x) is the pixel at (row c + y, col c + x) of the face's cell; the vertical cross stores -Z
// turned by 180 degrees (it continues the column +Y, +Z, -Y downwards).
__constant__ uint8_t kCrossCell[2][6][2] = {{{1, 2}, {1, 0}, {0, 1}, {2, 1}, {1, 1}, {3, 1}},      // vertical: (row, col) of +X -X +Y -Y +Z -Z
                                            {{1, 2}, {1, 0}, {0, 1}, {2, 1}, {1, 1}, {1, 3}}};     // horizontal
__global__ void __launch_bounds__(256) envCrossKernel(const void* __restrict__ src, int pixels, uint32_t width, uint32_t cell, int horizontal,
                                                      float4* __restrict__ level0, uint2* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x, perFace = (size_t)cell * cell;
  if (i >= 6u * perFace) return;
  const uint32_t face = (uint32_t)(i / perFace), rem = (uint32_t)(i % perFace);
  uint32_t y = rem / cell, x = rem % cell;
  if (!horizontal && face == 5u) { y = cell - 1u - y; x = cell - 1u - x; }
  const size_t row = (size_t)kCrossCell[horizontal][face][0] * cell + y, col = (size_t)kCrossCell[horizontal][face][1] * cell + x;
  const f3 v = envPixel(src, pixels, row * width + col);
  level0[i] = make_float4(v.x, v.y, v.z, 1.0f);
  dst[i] = packRGBA16F(v.x, v.y, v.z, 1.0f);
}

// Level 0 from a panorama of width x height pixels, rows top to bottom: the direction through the texel's centre, its longitude and latitude
// (+Z in the middle of the image, +X to its right, +Y in the top row), one bilinear tap -- columns wrap, rows clamp.  Coordinates and
// weights in fp64, rounded once: the kernel runs once, and what it may differ from a float64 model by is a rounding of the result.
__global__ void __launch_bounds__(256) envEquirectKernel(const void* __restrict__ src, int pixels, uint32_t width, uint32_t height, uint32_t size,
                                                         float4* __restrict__ level0, uint2* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x, perFace = (size_t)size * size;
  if (i >= 6u * perFace) return;
  const uint32_t face = (uint32_t)(i / perFace), rem = (uint32_t)(i % perFace), y = rem / size, x = rem % size;
  const double u = ((double)x + 0.5) / (double)size * 2.0 - 1.0, w = ((double)y + 0.5) / (double)size * 2.0 - 1.0;
  double dx, dy, dz;
  switch (face) {
    case 0: dx = 1.0; dy = -w; dz = -u; break;
    case 1: dx = -1.0; dy = -w; dz = u; break;
    case 2: dx = u; dy = 1.0; dz = w; break;
    case 3: dx = u; dy = -1.0; dz = -w; break;
    case 4: dx = u; dy = -w; dz = 1.0; break;
    default: dx = -u; dy = -w; dz = -1.0; break;
  }
  const double len = sqrt(dx * dx + dy * dy + dz * dz);
  const double pi = 3.14159265358979323846;
  const double lon = atan2(dx / len, dz / len), lat = asin(fmin(fmax(dy / len, -1.0), 1.0));
  const double s = (lon / (2.0 * pi) + 0.5) * (double)width - 0.5, t = (0.5 - lat / pi) * (double)height - 0.5;
  const double s0 = floor(s), t0 = floor(t), fx = s - s0, fy = t - t0;
  const long long W = (long long)width, H = (long long)height;
  const long long x0 = (((long long)s0 % W) + W) % W, x1 = (x0 + 1) % W;
  const long long ty = (long long)t0;
  const long long y0 = ty < 0 ? 0 : (ty > H - 1 ? H - 1 : ty), y1 = ty + 1 < 0 ? 0 : (ty + 1 > H - 1 ? H - 1 : ty + 1);
  const f3 a = envPixel(src, pixels, (size_t)(y0 * W + x0)), b = envPixel(src, pixels, (size_t)(y0 * W + x1));
  const f3 c = envPixel(src, pixels, (size_t)(y1 * W + x0)), d = envPixel(src, pixels, (size_t)(y1 * W + x1));
  // (no term is negative: nothing cancels, and the sum is as accurate relative to itself as its terms)
  const float r = (float)((1.0 - fy) * ((1.0 - fx) * (double)a.x + fx * (double)b.x) + fy * ((1.0 - fx) * (double)c.x + fx * (double)d.x));
  const float g = (float)((1.0 - fy) * ((1.0 - fx) * (double)a.y + fx * (double)b.y) + fy * ((1.0 - fx) * (double)c.y + fx * (double)d.y));
  const float bl = (float)((1.0 - fy) * ((1.0 - fx) * (double)a.z + fx * (double)b.z) + fy * ((1.0 - fx) * (double)c.z + fx * (double)d.z));
  level0[i] = make_float4(r, g, bl, 1.0f);
  dst[i] = packRGBA16F(r, g, bl, 1.0f);
}

// rtggx_generate_env_mips: the decoded level 0 back in fp32 (every half is one)
__global__ void __launch_bounds__(256) envWidenKernel(const uint2* __restrict__ texels, float4* __restrict__ level0, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const f4 v = unpackRGBA16F(texels[i]);
  level0[i] = make_float4(v.x, v.y, v.z, 1.0f);
}

// One axis of the box filter that halves a side p to q = p >> 1: child i covers parents 2 i, 2 i + 1 of an even side; of an odd one
// (p = 2 q + 1) the span [i p / q, (i + 1) p / q), which is (q - i) / q of parent 2 i, all of 2 i + 1 and (i + 1) / q of 2 i + 2 -- integer
// weights that sum to p.  Every operation is an fp32 operation of its own, in this order (tests/envimage_ref.py restates it bit for bit).
RT_DEV float envBox(float t0, float t1, float t2, uint32_t i, uint32_t q, bool odd) {
  if (!odd) return (t0 + t1) / 2.0f;
  return (((float)(q - i) * t0 + (float)q * t1) + (float)(i + 1u) * t2) / (float)(2u * q + 1u);
}
// Level m + 1 from the fp32 level m, each face alone: the horizontal pass of the (up to three) parent rows, then the vertical one -- the
// separable filter, the rows of its first pass recomputed by the lanes that share them instead of stored.
__global__ void __launch_bounds__(256) envMipKernel(const float4* __restrict__ parent, uint32_t p, float4* __restrict__ child, uint2* __restrict__ dst) {
  const uint32_t q = p >> 1;
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x, perFace = (size_t)q * q;
  if (i >= 6u * perFace) return;
  const uint32_t face = (uint32_t)(i / perFace), rem = (uint32_t)(i % perFace), y = rem / q, x = rem % q;
  const bool odd = (p & 1u) != 0u;
  const float4* f = parent + (size_t)face * p * p;
  float h[3][3];
  for (uint32_t k = 0; k < (odd ? 3u : 2u); ++k) {
    const float4* row = f + (size_t)(2u * y + k) * p + 2u * x;
    const float4 a = row[0], b = row[1], c = odd ? row[2] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    h[k][0] = envBox(a.x, b.x, c.x, x, q, odd); h[k][1] = envBox(a.y, b.y, c.y, x, q, odd); h[k][2] = envBox(a.z, b.z, c.z, x, q, odd);
  }
  if (!odd) h[2][0] = h[2][1] = h[2][2] = 0.0f;
  const float r = envBox(h[0][0], h[1][0], h[2][0], y, q, odd), g = envBox(h[0][1], h[1][1], h[2][1], y, q, odd), b = envBox(h[0][2], h[1][2], h[2][2], y, q, odd);
  child[i] = make_float4(r, g, b, 1.0f);
  dst[i] = packRGBA16F(r, g, b, 1.0f);
}

static uint32_t fullChain(uint32_t size) { uint32_t mips = 1; while ((size >> mips) != 0u) ++mips; return mips; }
static uint32_t envBlocks(size_t n) { return (uint32_t)((n + 255u) / 256u); }

// Levels 1 .. of `texels` from the fp32 level 0 in `ping` (`pong`: room for level 1), alternating between the two.
static void launchEnvChain(uint2* texels, const uint32_t* mipOffset, uint32_t size, uint32_t mips, float4* ping, float4* pong, hipStream_t s) {
  for (uint32_t m = 1; m < mips; ++m) {
    const uint32_t p = size >> (m - 1u), q = p >> 1;
    hipLaunchKernelGGL(envMipKernel, dim3(envBlocks(6u * (size_t)q * q)), dim3(256), 0, s, (const float4*)ping, p, pong, texels + mipOffset[m]);
    float4* t = ping; ping = pong; pong = t;
  }
}

// The new cube takes the context's place only when everything has been built and its mip offsets are on the device: a failure on the way
// leaves the environment as it was (nothing runs between the copy of the offsets and the swap: the caller has waited for every stream).
static int installEnv(rtggx_context* c, DevBuf<uint2>& texels, uint32_t size, uint32_t mips, const uint32_t* mipOffset, uint64_t total) {
  uint32_t offsets[16];
  for (uint32_t m = 0; m < 16u; ++m) offsets[m] = m < mips ? mipOffset[m] : 0u;
  const hipError_t e = hipMemcpy(c->dEnvMipOffset, offsets, sizeof offsets, hipMemcpyHostToDevice);
  if (e != hipSuccess) { setError("environment: mip offsets: %s", hipGetErrorString(e)); return -2; }
  c->env.texels = std::move(texels); c->env.size = size; c->env.mips = mips; c->env.totalTexels = total;
  std::memcpy(c->env.mipOffset, offsets, sizeof offsets);
  c->shDone = false;
  return 0;
}
static uint64_t chainOffsets(uint32_t size, uint32_t mips, uint32_t* mipOffset) {
  uint64_t texels = 0;
  for (uint32_t m = 0; m < mips; ++m) { const uint32_t sz = size >> m; mipOffset[m] = (uint32_t)texels; texels += 6ull * sz * sz; }
  return texels;
}

// The arguments have been checked by rtggx_set_env_image: the layout and pixel format are known ones, `size` is the cube's side (the cell of
// a cross), the source holds width x height pixels.
int buildEnvFromImage(rtggx_context* c, int layout, int pixels, uint32_t width, uint32_t height, const void* hostData, uint32_t size, hipStream_t s) {
  const uint32_t mips = fullChain(size);
  uint32_t mipOffset[16];
  const uint64_t total = chainOffsets(size, mips, mipOffset);
  const size_t srcBytes = (size_t)width * height * (pixels == RTGGX_PIXELS_RGBE8 ? 4u : 12u), n0 = 6u * (size_t)size * size, h = size >> 1, n1 = 6u * h * h;
  DevBuf<void> dSrc; DevBuf<uint2> texels; DevBuf<float4> ping, pong;
  hipError_t e = alloc(dSrc, srcBytes);
  if (e == hipSuccess) e = alloc(texels, total);
  if (e == hipSuccess) e = alloc(ping, n0);
  if (e == hipSuccess && n1) e = alloc(pong, n1);
  if (e == hipSuccess) e = hipMemcpyAsync(dSrc, hostData, srcBytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    if (layout == RTGGX_ENV_EQUIRECT) hipLaunchKernelGGL(envEquirectKernel, dim3(envBlocks(n0)), dim3(256), 0, s, (const void*)dSrc, pixels, width, height, size, ping, texels);
    else hipLaunchKernelGGL(envCrossKernel, dim3(envBlocks(n0)), dim3(256), 0, s, (const void*)dSrc, pixels, width, size, layout == RTGGX_ENV_HCROSS ? 1 : 0, ping, texels);
    launchEnvChain(texels, mipOffset, size, mips, ping, pong, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { setError("rtggx_set_env_image: %s", hipGetErrorString(e)); return -2; }
  return installEnv(c, texels, size, mips, mipOffset, total);
}

// The cube rtggx_generate_env_mips leaves, enqueued on `s`: the context's level 0 as it is and the full box chain below it.  The buffers are
// allocated here; the two fp32 scratch levels must outlive the launches (the caller synchronises `s` before it lets go of them).
// `cone` (rtggx_sun_from_env's removal): level 0 is the context's with the sun cut out of the cone's texels (sunenv.hip), and the chain is that one's.
struct BoxChain { DevBuf<uint2> texels; DevBuf<float4> ping, pong; };
static hipError_t launchBoxChain(rtggx_context* c, BoxChain& b, uint32_t size, uint32_t mips, const uint32_t* mipOffset, uint64_t total, hipStream_t s, const SunCone* cone = nullptr) {
  const size_t n0 = 6u * (size_t)size * size, h = size >> 1, n1 = 6u * h * h;
  hipError_t e = alloc(b.texels, total);
  if (e == hipSuccess) e = alloc(b.ping, n0);
  if (e == hipSuccess && n1) e = alloc(b.pong, n1);
  if (e == hipSuccess && !cone) e = hipMemcpyAsync(b.texels, c->env.texels, n0 * sizeof(uint2), hipMemcpyDeviceToDevice, s);      // level 0 stays what it is
  if (e != hipSuccess) return e;
  if (cone) launchSunRemove(c->env.texels, b.texels, size, *cone, s);
  hipLaunchKernelGGL(envWidenKernel, dim3(envBlocks(n0)), dim3(256), 0, s, cone ? (const uint2*)b.texels : (const uint2*)c->env.texels, b.ping.get(), n0);
  launchEnvChain(b.texels, mipOffset, size, mips, b.ping, b.pong, s);
  return hipGetLastError();
}

int generateEnvMips(rtggx_context* c, hipStream_t s) {
  const uint32_t size = c->env.size, mips = fullChain(size);
  uint32_t mipOffset[16];
  const uint64_t total = chainOffsets(size, mips, mipOffset);
  BoxChain b;
  hipError_t e = launchBoxChain(c, b, size, mips, mipOffset, total, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { setError("rtggx_generate_env_mips: %s", hipGetErrorString(e)); return -2; }
  return installEnv(c, b.texels, size, mips, mipOffset, total);
}

// rtggx_sun_from_env's removal (sunenv.hip measures, this replaces): generateEnvMips over the cut level 0.  The caller has waited for every stream.
int removeSunFromEnv(rtggx_context* c, const SunCone& cone, hipStream_t s) {
  const uint32_t size = c->env.size, mips = fullChain(size);
  uint32_t mipOffset[16];
  const uint64_t total = chainOffsets(size, mips, mipOffset);
  BoxChain b;
  hipError_t e = launchBoxChain(c, b, size, mips, mipOffset, total, s, &cone);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { setError("rtggx_sun_from_env: %s", hipGetErrorString(e)); return -2; }
  return installEnv(c, b.texels, size, mips, mipOffset, total);
}

// rtggx_prefilter_env (include/rtggx.h; rt_env_filter.h builds the tables): the box-chain cube C beside the context's, then every level
// below level 0 of a third cube from C -- one launch per level, the levels from M - 4 on sharing the table of roughness 1 --, all on `s`
// with one wait at the end.  C, the tables and the offsets of C are scratch and gone on return; the context's cube is replaced last.
int prefilterEnv(rtggx_context* c, uint32_t samples, hipStream_t s) {
  const uint32_t size = c->env.size, mips = fullChain(size);
  uint32_t mipOffset[16] = {};
  const uint64_t total = chainOffsets(size, mips, mipOffset);
  // the tables, one behind the other: level m's starts at first[m] and holds count[m] entries
  std::vector<EnvFilterEntry> entries;
  uint32_t first[16] = {}, count[16] = {}; float invW[16] = {};
  for (uint32_t m = 1; m < mips; ++m) {
    if (m > 1u && envFilterWidest(m - 1u, mips)) { first[m] = first[m - 1u]; count[m] = count[m - 1u]; invW[m] = invW[m - 1u]; continue; }
    const EnvFilterTable t = envFilterTable(size, mips, m, samples);
    first[m] = (uint32_t)entries.size(); count[m] = (uint32_t)t.entries.size(); invW[m] = t.invW;
    entries.insert(entries.end(), t.entries.begin(), t.entries.end());
  }
  BoxChain b; DevBuf<uint2> texels; DevBuf<uint32_t> dOffsets; DevBuf<float4> dTable;
  static_assert(sizeof(EnvFilterEntry) == sizeof(float4), "a table entry is one 16-byte load");
  hipError_t e = launchBoxChain(c, b, size, mips, mipOffset, total, s);
  if (e == hipSuccess) e = alloc(texels, total);
  if (e == hipSuccess) e = alloc(dOffsets, 16);
  if (e == hipSuccess && !entries.empty()) e = alloc(dTable, entries.size());
  if (e == hipSuccess) e = hipMemcpyAsync(texels, c->env.texels, 6u * (size_t)size * size * sizeof(uint2), hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) e = hipMemcpyAsync(dOffsets, mipOffset, sizeof mipOffset, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && !entries.empty()) e = hipMemcpyAsync(dTable, entries.data(), entries.size() * sizeof(EnvFilterEntry), hipMemcpyHostToDevice, s);
  int launched = 0;
  for (uint32_t m = 1; m < mips && e == hipSuccess && launched == 0; ++m)
    launched = launchEnvPrefilter(b.texels, size, mips, dOffsets, dTable.get() + first[m], count[m], invW[m], size >> m, texels.get() + mipOffset[m], s);
  const hipError_t waited = hipStreamSynchronize(s);      // (whatever happened: the host arrays above and the scratch are in use until here)
  if (launched) return launched;                          // (the launcher has said why)
  if (e == hipSuccess) e = waited;
  if (e != hipSuccess) { setError("rtggx_prefilter_env: %s", hipGetErrorString(e)); return -2; }
  return installEnv(c, texels, size, mips, mipOffset, total);
}

// ---- SH projection ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) shProjectKernel(const uint2* __restrict__ texels, uint32_t size, double* __restrict__ acc) {
  __shared__ double red[256];
  const uint32_t n = 6u * size * size;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  double v[28];
  for (int k = 0; k < 28; ++k) v[k] = 0.0;
  if (i < n) {
    const uint32_t face = i / (size * size), rem = i % (size * size), y = rem / size, x = rem % size;
    const double u = ((double)x + 0.5) / (double)size * 2.0 - 1.0, w = ((double)y + 0.5) / (double)size * 2.0 - 1.0;
    double dx, dy, dz;
    switch (face) {
      case 0: dx = 1.0; dy = -w; dz = -u; break;
      case 1: dx = -1.0; dy = -w; dz = u; break;
      case 2: dx = u; dy = 1.0; dz = w; break;
      case 3: dx = u; dy = -1.0; dz = -w; break;
      case 4: dx = u; dy = -w; dz = 1.0; break;
      default: dx = -u; dy = -w; dz = -1.0; break;
    }
    const double len = sqrt(dx * dx + dy * dy + dz * dz);
    const double sx = -dx / len, sy = -dy / len, sz = dz / len;
    const double wt = 1.0 / (len * len * len);
    const double Y[9] = {0.28209479177387814, 0.4886025119029199 * sy, 0.4886025119029199 * sz, 0.4886025119029199 * sx,
                         1.0925484305920792 * sx * sy, 1.0925484305920792 * sy * sz, 0.31539156525252005 * (3.0 * sz * sz - 1.0),
                         1.0925484305920792 * sx * sz, 0.5462742152960396 * (sx * sx - sy * sy)};
    const uint2 t = texels[i];
    const double L[3] = {(double)f16ToF32(t.x & 0xFFFFu), (double)f16ToF32(t.x >> 16), (double)f16ToF32(t.y & 0xFFFFu)};
    for (int k = 0; k < 9; ++k) for (int ch = 0; ch < 3; ++ch) v[3 * k + ch] = Y[k] * wt * L[ch];
    v[27] = wt;
  }
  for (int k = 0; k < 28; ++k) {
    red[threadIdx.x] = v[k];
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) { if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st]; __syncthreads(); }
    if (threadIdx.x == 0) atomicAdd(&acc[k], red[0]);
    __syncthreads();
  }
}
__global__ void shFinalizeKernel(const double* __restrict__ acc, float* __restrict__ sh) {
  const int k = threadIdx.x;
  if (k < 27) sh[k] = (float)(acc[k] * (4.0 * 3.14159265358979323846 / acc[27]));
}

int projectSH(rtggx_context* c, hipStream_t s) {
  if (!c->env.texels) { setError("rtggx_transform_sh: no environment map"); return -1; }
  DevBuf<double> acc;
  RT_HIP(alloc(acc, 28));
  RT_HIP(hipMemsetAsync(acc, 0, 28 * sizeof(double), s));
  const uint32_t n = 6u * c->env.size * c->env.size;
  hipLaunchKernelGGL(shProjectKernel, dim3((n + 255) / 256), dim3(256), 0, s, c->env.texels, c->env.size, acc);
  hipLaunchKernelGGL(shFinalizeKernel, dim3(1), dim3(64), 0, s, acc, c->sh);
  RT_HIP(hipGetLastError());
  RT_HIP(hipStreamSynchronize(s));
  c->shDone = true;
  return 0;
}

}  // namespace rt
