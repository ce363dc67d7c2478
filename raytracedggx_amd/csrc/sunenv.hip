// The sun from the environment (rtggx_sun_from_env; include/rtggx.h, DESIGN.md "The sun from the environment"; rt_sun_env.h holds the
// host's arithmetic): three reductions over the 6 S^2 texels of level 0 and, where the sun is taken out, the rewrite of level 0.
//   pass A  sunPeakKernel / sunPeakFinishKernel: the texel of greatest Y, ties to the lowest index -- a maximum, so any order gives it.
//   pass B  sunSumsKernel<0>: weight_all, sum(w Y), weight_ring, ring_rgb, and the texels in the cone and in the ring;
//   pass C  sunSumsKernel<1>: weight_cone, excess, moment over the cone, and its lit texels; both finished by sunSumsFinishKernel.
// THE TREE is score.hip's: every sum runs over ALL texels i = 0 .. 6 S^2 - 1 -- a texel outside the sum's mask contributes +0.0 --, padded
// with +0.0 to a power of two and added pairwise, adjacent pairs first.  Stage 1: a workgroup of 256 lanes takes an aligned chunk of
// RT_SUN_CHUNK = 1024 texels, a lane the aligned run of 4, the wave six levels by xor shuffles, the four waves two more through LDS;
// stage 2: one workgroup, the levels above a chunk over the chunks' partials.  Padding further than the next power of two adds +0.0 to
// finished subtrees: no bit changes but the sign of a sum that is zero (the moment's terms are signed; a zero sum reads +0.0 or -0.0).
// No atomics, no contraction, no inline assembly.  Setup work, not per frame: 8 bytes read per texel and pass, nothing written but the
// partials; the host waits after each pass for the few numbers the next one needs.
#include "rtggx_context.h"
#include "rt_sun_env.h"

namespace rt {

#define RT_SUN_CHUNK 1024u
#define RT_SUN_SUMS 7u
#define RT_SUN_FINISH_THREADS 1024u

// One channel of a texel: x > 0 ? min(x, 65504) : 0 -- NaN, negatives and both zeros become +0, infinity the largest finite half.
RT_DEV double sunValue(uint32_t half) { const float x = f16ToF32(half); return x > 0.0f ? (double)fminf(x, 65504.0f) : 0.0; }
RT_DEV double sunLuma(double r, double g, double b) {
#pragma clang fp contract(off)
  return (0.25 * r + 0.5 * g) + 0.25 * b;
}
RT_DEV void sunTexel(const uint2* __restrict__ texels, uint32_t i, double v[3]) {
  const uint2 t = texels[i];
  v[0] = sunValue(t.x & 0xFFFFu); v[1] = sunValue(t.x >> 16); v[2] = sunValue(t.y & 0xFFFFu);
}
RT_DEV void sunTexelDirection(uint32_t S, uint32_t i, double D[3]) {
  const uint32_t perFace = S * S, face = i / perFace, rem = i - face * perFace, y = rem / S, x = rem - y * S;
  sunEnvDirection(S, face, x, y, D);
}
// In the cone of half-angle acos(sqrt(cos2)) about P: dot > 0 and dot^2 >= (cos2 n) nP.  dot, n and nP are integers and exact; the three
// products are double products, each rounded on its own.
RT_DEV bool sunInside(double dot, double n, double nP, double cos2) {
#pragma clang fp contract(off)
  return dot > 0.0 && dot * dot >= (cos2 * n) * nP;
}

// ---- pass A: the peak --------------------------------------------------------------------------------------------------------------------
RT_DEV void sunBetter(double& y, uint32_t& i, double y2, uint32_t i2) { if (y2 > y || (y2 == y && i2 < i)) { y = y2; i = i2; } }

struct SunPeak { double luma; uint32_t index, pad; };

__global__ void __launch_bounds__(256) sunPeakKernel(const uint2* __restrict__ texels, uint32_t count, uint32_t numChunks, double* __restrict__ chunkLuma, uint32_t* __restrict__ chunkIndex) {
  __shared__ double waveLuma[4];
  __shared__ uint32_t waveIndex[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t chunk = blockIdx.x; chunk < numChunks; chunk += gridDim.x) {
    const uint32_t p0 = chunk * RT_SUN_CHUNK + threadIdx.x * 4u;      // (count <= 6 x 8192^2 < 2^29)
    double best = -1.0; uint32_t at = 0xFFFFFFFFu;                    // (every Y is >= 0: the first texel replaces this)
    for (uint32_t k = 0; k < 4u; ++k) {
      if (p0 + k < count) { double v[3]; sunTexel(texels, p0 + k, v); sunBetter(best, at, sunLuma(v[0], v[1], v[2]), p0 + k); }
    }
    for (uint32_t m = 1u; m < 64u; m <<= 1) {
      const double y2 = __shfl_xor(best, (int)m, 64); const uint32_t i2 = (uint32_t)__shfl_xor((int)at, (int)m, 64);
      sunBetter(best, at, y2, i2);
    }
    if (lane == 0u) { waveLuma[wave] = best; waveIndex[wave] = at; }
    __syncthreads();
    if (threadIdx.x == 0u) {
      for (uint32_t w = 1; w < 4u; ++w) sunBetter(best, at, waveLuma[w], waveIndex[w]);
      chunkLuma[chunk] = best; chunkIndex[chunk] = at;
    }
    __syncthreads();      // (the next chunk's waves write the same LDS words)
  }
}
__global__ void __launch_bounds__(RT_SUN_FINISH_THREADS) sunPeakFinishKernel(const double* __restrict__ chunkLuma, const uint32_t* __restrict__ chunkIndex, uint32_t numChunks, SunPeak* __restrict__ out) {
  __shared__ double luma[RT_SUN_FINISH_THREADS];
  __shared__ uint32_t index[RT_SUN_FINISH_THREADS];
  const uint32_t tid = threadIdx.x;
  double best = -1.0; uint32_t at = 0xFFFFFFFFu;
  for (uint32_t i = tid; i < numChunks; i += RT_SUN_FINISH_THREADS) sunBetter(best, at, chunkLuma[i], chunkIndex[i]);
  luma[tid] = best; index[tid] = at;
  __syncthreads();
  for (uint32_t w = RT_SUN_FINISH_THREADS / 2u; w > 0u; w >>= 1) {
    if (tid < w) { sunBetter(best, at, luma[tid + w], index[tid + w]); luma[tid] = best; index[tid] = at; }
    __syncthreads();
  }
  if (tid == 0u) { SunPeak p; p.luma = best; p.index = at; p.pad = 0u; *out = p; }
}

// ---- passes B and C: the sums --------------------------------------------------------------------------------------------------------------
struct SunSumsArgs {
  const uint2* texels; double* partial; uint32_t* counts;      // partial[sum * stride + chunk], counts[chunk * 2 + which]
  uint32_t S, count, numChunks, stride;
  double P[3], nP, cos2Cone, cos2Ring, b16[3];                 // the peak's integer direction and its square; pass C: the background's half
};

// The terms of one texel.  Pass 0 (B): w, w Y, then over the ring w, w r, w g, w b (and one sum that stays +0.0); counts: in the cone, in
// the ring.  Pass 1 (C), over the cone: w, w e_r, w e_g, w e_b, (w Y(e)) d_x, d_y, d_z; counts: lit, nothing.
template <int PASS>
RT_DEV void sunTerms(const SunSumsArgs& A, uint32_t i, double t[RT_SUN_SUMS], uint32_t& c0, uint32_t& c1) {
#pragma clang fp contract(off)
  double D[3], v[3];
  sunTexelDirection(A.S, i, D);
  sunTexel(A.texels, i, v);
  const double n = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2], dot = (D[0] * A.P[0] + D[1] * A.P[1]) + D[2] * A.P[2];      // (integers: exact in any order)
  const double q = sqrt(n), w = (4.0 * (double)A.S) / (n * q);
  const bool cone = sunInside(dot, n, A.nP, A.cos2Cone);
#pragma unroll
  for (uint32_t s = 0; s < RT_SUN_SUMS; ++s) t[s] = 0.0;
  if (PASS == 0) {
    const bool ring = !cone && sunInside(dot, n, A.nP, A.cos2Ring);
    t[0] = w; t[1] = w * sunLuma(v[0], v[1], v[2]);
    if (ring) { t[2] = w; t[3] = w * v[0]; t[4] = w * v[1]; t[5] = w * v[2]; }
    c0 = cone ? 1u : 0u; c1 = ring ? 1u : 0u;
  } else {
    c0 = 0u; c1 = 0u;
    if (cone) {
      const double e0 = fmax(v[0] - A.b16[0], 0.0), e1 = fmax(v[1] - A.b16[1], 0.0), e2 = fmax(v[2] - A.b16[2], 0.0);
      const double wy = w * sunLuma(e0, e1, e2);
      t[0] = w; t[1] = w * e0; t[2] = w * e1; t[3] = w * e2;
      t[4] = wy * (D[0] / q); t[5] = wy * (D[1] / q); t[6] = wy * (D[2] / q);
      c0 = (e0 > 0.0 || e1 > 0.0 || e2 > 0.0) ? 1u : 0u;
    }
  }
}

template <int PASS>
__global__ void __launch_bounds__(256) sunSumsKernel(SunSumsArgs A) {
#pragma clang fp contract(off)
  __shared__ double waveSum[RT_SUN_SUMS][4];
  __shared__ uint32_t waveCount[2][4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t chunk = blockIdx.x; chunk < A.numChunks; chunk += gridDim.x) {
    const uint32_t p0 = chunk * RT_SUN_CHUNK + threadIdx.x * 4u;
    double t[4][RT_SUN_SUMS];
    uint32_t cnt[2] = {0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      if (p0 + k < A.count) {
        uint32_t c0, c1;
        sunTerms<PASS>(A, p0 + k, t[k], c0, c1);
        cnt[0] += c0; cnt[1] += c1;
      } else {
#pragma unroll
        for (uint32_t s = 0; s < RT_SUN_SUMS; ++s) t[k][s] = 0.0;
      }
    }
    double v[RT_SUN_SUMS];
#pragma unroll
    for (uint32_t s = 0; s < RT_SUN_SUMS; ++s) v[s] = (t[0][s] + t[1][s]) + (t[2][s] + t[3][s]);
#pragma unroll
    for (uint32_t m = 1u; m < 64u; m <<= 1) {
#pragma unroll
      for (uint32_t s = 0; s < RT_SUN_SUMS; ++s) v[s] = v[s] + __shfl_xor(v[s], (int)m, 64);
#pragma unroll
      for (uint32_t q = 0; q < 2u; ++q) cnt[q] += (uint32_t)__shfl_xor((int)cnt[q], (int)m, 64);
    }
    if (lane == 0u) {
#pragma unroll
      for (uint32_t s = 0; s < RT_SUN_SUMS; ++s) waveSum[s][wave] = v[s];
      waveCount[0][wave] = cnt[0]; waveCount[1][wave] = cnt[1];
    }
    __syncthreads();
    if (threadIdx.x < RT_SUN_SUMS) {
      const uint32_t s = threadIdx.x;
      A.partial[(size_t)s * A.stride + chunk] = (waveSum[s][0] + waveSum[s][1]) + (waveSum[s][2] + waveSum[s][3]);
    } else if (threadIdx.x >= 64u && threadIdx.x < 66u) {
      const uint32_t q = threadIdx.x - 64u;
      A.counts[(size_t)chunk * 2u + q] = (waveCount[q][0] + waveCount[q][1]) + (waveCount[q][2] + waveCount[q][3]);
    }
    __syncthreads();      // (the next chunk's waves write the same LDS words)
  }
}

struct SunSums { double sum[RT_SUN_SUMS]; unsigned long long count[2]; };
struct SunFinishArgs {
  double* level[2];      // [0]: stage 1's partials, RT_SUN_SUMS x stride; [1]: room for half of that
  const uint32_t* counts;
  SunSums* out;
  uint32_t numChunks, stride;      // stride: a power of two >= numChunks >= 1
};
__global__ void __launch_bounds__(RT_SUN_FINISH_THREADS) sunSumsFinishKernel(SunFinishArgs A) {
#pragma clang fp contract(off)
  __shared__ unsigned long long countSum[2][RT_SUN_FINISH_THREADS];
  const uint32_t tid = threadIdx.x;
  uint32_t src = 0u;
  for (uint32_t n = A.stride; n > 1u; n >>= 1) {
    const uint32_t half = n >> 1;
    const double* x = A.level[src]; double* y = A.level[src ^ 1u];
    const uint32_t valid = src == 0u && n == A.stride ? A.numChunks : n;      // beyond the last chunk: the padding, +0.0 (stage 1 wrote nothing there)
    for (uint32_t i = tid; i < RT_SUN_SUMS * half; i += RT_SUN_FINISH_THREADS) {
      const uint32_t s = i / half, j = i - s * half;
      const double a = 2u * j < valid ? x[(size_t)s * n + 2u * j] : 0.0;
      const double b = 2u * j + 1u < valid ? x[(size_t)s * n + 2u * j + 1u] : 0.0;
      y[(size_t)s * half + j] = a + b;
    }
    __syncthreads();      // (one workgroup: the barrier orders its global stores and loads)
    src ^= 1u;
  }
  unsigned long long c[2] = {0ull, 0ull};
  for (uint32_t i = tid; i < A.numChunks; i += RT_SUN_FINISH_THREADS) { c[0] += A.counts[(size_t)i * 2u]; c[1] += A.counts[(size_t)i * 2u + 1u]; }
  countSum[0][tid] = c[0]; countSum[1][tid] = c[1];
  __syncthreads();
  for (uint32_t w = RT_SUN_FINISH_THREADS / 2u; w > 0u; w >>= 1) {
    if (tid < w) { countSum[0][tid] += countSum[0][tid + w]; countSum[1][tid] += countSum[1][tid + w]; }
    __syncthreads();
  }
  if (tid == 0u) {
    const double* r = A.level[src];
    SunSums R;
    for (uint32_t s = 0; s < RT_SUN_SUMS; ++s) R.sum[s] = r[s];
    R.count[0] = countSum[0][0]; R.count[1] = countSum[1][0];
    *A.out = R;
  }
}

// ---- the removal: level 0 of the new cube ---------------------------------------------------------------------------------------------------
// A copy, but in the cone each of r, g, b becomes min(v, b16) -- both are binary16 values, nothing is rounded --; alpha is kept.
RT_DEV uint32_t sunCut(uint32_t half, uint32_t b16) {
  const float x = f16ToF32(half);
  const uint32_t v = x > 0.0f ? ((half & 0x7FFFu) == 0x7C00u ? 0x7BFFu : half) : 0u;      // the texel's value as a half: +inf is 65504, what is not > 0 is +0
  return v < b16 ? v : b16;                                                               // (non-negative halves order as their codes do)
}
__global__ void __launch_bounds__(256) sunRemoveKernel(const uint2* __restrict__ src, uint2* __restrict__ dst, uint32_t S, uint32_t count, SunCone C) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  uint2 t = src[i];
  double D[3];
  sunTexelDirection(S, i, D);
  const double n = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2], dot = (D[0] * C.P[0] + D[1] * C.P[1]) + D[2] * C.P[2];
  if (sunInside(dot, n, C.nP, C.cos2Cone))
    t = make_uint2(sunCut(t.x & 0xFFFFu, C.b16[0]) | (sunCut(t.x >> 16, C.b16[1]) << 16), sunCut(t.y & 0xFFFFu, C.b16[2]) | (t.y & 0xFFFF0000u));
  dst[i] = t;
}
void launchSunRemove(const uint2* src, uint2* dst, uint32_t size, const SunCone& cone, hipStream_t s) {
  const uint32_t count = 6u * size * size;
  hipLaunchKernelGGL(sunRemoveKernel, dim3((count + 255u) / 256u), dim3(256), 0, s, src, dst, size, count, cone);
}

// ---- the call -----------------------------------------------------------------------------------------------------------------------------
// The arguments have been checked and every stream waited for (rtggx_sun_from_env, context.hip).  Everything allocated here is scratch and
// gone on return; the context is touched by removeSunFromEnv (env.hip) alone, and only when a sun was found and is to be taken out.
int sunFromEnv(rtggx_context* c, const SunEnvAngles& angles, int remove, RtggxSunEstimate* out, hipStream_t s) {
  const uint32_t S = c->env.size, count = 6u * S * S, numChunks = (count + RT_SUN_CHUNK - 1u) / RT_SUN_CHUNK;
  uint32_t stride = 1u; while (stride < numChunks) stride <<= 1;
  DevBuf<double> partial0, partial1, chunkLuma; DevBuf<uint32_t> counts, chunkIndex; DevBuf<SunPeak> dPeak; DevBuf<SunSums> dSums;
  RT_HIP(alloc(partial0, (size_t)RT_SUN_SUMS * stride));
  RT_HIP(alloc(partial1, (size_t)RT_SUN_SUMS * (stride > 1u ? stride / 2u : 1u)));
  RT_HIP(alloc(counts, (size_t)numChunks * 2u));
  RT_HIP(alloc(chunkLuma, numChunks));
  RT_HIP(alloc(chunkIndex, numChunks));
  RT_HIP(alloc(dPeak, 1));
  RT_HIP(alloc(dSums, 1));
  // few waves that stream, as the scoring does: at most two workgroups per CU, each looping over chunks
  const uint32_t grid = numChunks < 2u * c->numCUs ? numChunks : 2u * c->numCUs;

  RtggxSunEstimate E;
  memset(&E, 0, sizeof E);
  E.cos2_cone = angles.cos2Cone; E.cos2_ring = angles.cos2Ring;

  // pass A
  SunPeak peak;
  hipLaunchKernelGGL(sunPeakKernel, dim3(grid), dim3(256), 0, s, (const uint2*)c->env.texels, count, numChunks, chunkLuma.get(), chunkIndex.get());
  hipLaunchKernelGGL(sunPeakFinishKernel, dim3(1), dim3(RT_SUN_FINISH_THREADS), 0, s, (const double*)chunkLuma, (const uint32_t*)chunkIndex, numChunks, dPeak.get());
  RT_HIP(hipGetLastError());
  RT_HIP(hipMemcpyAsync(&peak, dPeak, sizeof peak, hipMemcpyDeviceToHost, s));
  RT_HIP(hipStreamSynchronize(s));
  if (peak.index >= count) { setError("rtggx_sun_from_env: the peak search returned texel %u of %u", peak.index, count); return -2; }
  E.peak_luma = peak.luma;
  E.peak_face = peak.index / (S * S); E.peak_y = (peak.index % (S * S)) / S; E.peak_x = peak.index % S;

  SunSumsArgs A;
  A.texels = c->env.texels; A.partial = partial0; A.counts = counts;
  A.S = S; A.count = count; A.numChunks = numChunks; A.stride = stride;
  sunEnvDirection(S, E.peak_face, E.peak_x, E.peak_y, A.P);
  A.nP = (A.P[0] * A.P[0] + A.P[1] * A.P[1]) + A.P[2] * A.P[2];
  A.cos2Cone = angles.cos2Cone; A.cos2Ring = angles.cos2Ring;
  A.b16[0] = A.b16[1] = A.b16[2] = 0.0;
  SunFinishArgs F;
  F.level[0] = partial0; F.level[1] = partial1; F.counts = counts; F.out = dSums; F.numChunks = numChunks; F.stride = stride;
  SunSums sums;

  // pass B
  hipLaunchKernelGGL(sunSumsKernel<0>, dim3(grid), dim3(256), 0, s, A);
  hipLaunchKernelGGL(sunSumsFinishKernel, dim3(1), dim3(RT_SUN_FINISH_THREADS), 0, s, F);
  RT_HIP(hipGetLastError());
  RT_HIP(hipMemcpyAsync(&sums, dSums, sizeof sums, hipMemcpyDeviceToHost, s));
  RT_HIP(hipStreamSynchronize(s));
  E.weight_all = sums.sum[0]; E.weight_ring = sums.sum[2];
  for (int k = 0; k < 3; ++k) E.ring_rgb[k] = sums.sum[3 + k];
  E.texels_cone = (uint32_t)sums.count[0]; E.texels_ring = (uint32_t)sums.count[1];
  const SunEnvBackground bg = sunEnvBackground(E.ring_rgb, E.weight_ring);
  for (int k = 0; k < 3; ++k) { E.background[k] = bg.background[k]; E.background_half[k] = bg.halfAsFloat[k]; }
  E.found = sunEnvFound(E.peak_luma, sums.sum[1], E.weight_all, angles.minContrast, E.mean_luma) ? 1u : 0u;

  if (E.found) {
    // pass C
    for (int k = 0; k < 3; ++k) A.b16[k] = (double)bg.halfAsFloat[k];
    hipLaunchKernelGGL(sunSumsKernel<1>, dim3(grid), dim3(256), 0, s, A);
    hipLaunchKernelGGL(sunSumsFinishKernel, dim3(1), dim3(RT_SUN_FINISH_THREADS), 0, s, F);
    RT_HIP(hipGetLastError());
    RT_HIP(hipMemcpyAsync(&sums, dSums, sizeof sums, hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    E.weight_cone = sums.sum[0];
    for (int k = 0; k < 3; ++k) { E.excess[k] = sums.sum[1 + k]; E.moment[k] = sums.sum[4 + k]; }
    E.texels_lit = (uint32_t)sums.count[0];
    E.found = sunEnvResult(E.moment, E.excess, E.weight_all, E.direction, E.irradiance) ? 1u : 0u;
  }
  *out = E;      // (the measurement is complete: a removal that fails leaves the old cube and this record, removed = 0)
  if (E.found && remove) {
    SunCone cone;
    for (int k = 0; k < 3; ++k) { cone.P[k] = A.P[k]; cone.b16[k] = bg.half[k]; }
    cone.nP = A.nP; cone.cos2Cone = angles.cos2Cone;
    const int r = removeSunFromEnv(c, cone, s);
    if (r) return r;
    out->removed = 1u;
  }
  return 0;
}

}  // namespace rt
