// Scoring against a reference image (rtggx_set_reference, rtggx_set_scoring; include/rtggx.h, DESIGN.md "Scoring against a reference"):
// nine fp64 sums and three counts over the pixels of the context's own rows, one record per frame, inside the frame on the main stream.
//
// THE TREE.  The contract fixes the order of every sum: the terms of pixels p = 0 .. P - 1, padded with +0.0 to a power of two, added
// pairwise -- adjacent pairs first, level by level.  Every term is a square or a sum of squares, so it is never -0.0, and x + (+0.0) = x
// for such x: padding FURTHER than the next power of two changes no bit, and a subtree that holds padding alone is +0.0.  That is what
// lets the two stages cut the tree at fixed places:
//   stage 1  scorePixelsKernel: a workgroup of 256 lanes takes an aligned chunk of RT_SCORE_CHUNK = 1024 pixels (aligned in p, not in
//            memory), a lane the aligned run of 4 -- levels 1 and 2 in its registers, (t0 + t1) + (t2 + t3) --, the wave levels 3 to 8 by xor
//            shuffles over 1, 2, 4 .. 32 lanes -- both partners of a pair compute a + b and b + a, the same bits --, the four waves levels
//            9 and 10 through LDS.  One partial per sum and chunk, plain stores; the grid loops over chunks, and since a chunk's partial
//            depends on its pixels alone, which workgroup takes it changes nothing.
//   stage 2  scoreFinishKernel: one workgroup, the levels above a chunk one at a time over the chunks' partials (padded to a power of two
//            by reading +0.0 beyond the last chunk), ping-pong between two buffers with a barrier per level; then the counts, and the
//            record into its slot of the ring.
// No atomics, no contraction (#pragma below; the build's -ffp-contract=off says the same), no inline assembly.
// Traffic per pixel: 8 (TemporalSSOut) + 8 (reference) + 4 + 4 (the raw words) + 8 (visibility and depth) = 32 bytes read, nothing written
// but 9 doubles and 3 words per 1024 pixels.
#include "rtggx_context.h"

namespace rt {

struct ScoreArgs {
  const uint2* out; const uint2* ref; const uint32_t* refl; const uint32_t* diff; const unsigned long long* visDepth;
  double* partial; uint32_t* counts;
  uint32_t first, count, diffMask, numChunks, stride;      // pixels [first, first + count) of every image; partial[sum * stride + chunk]
};

struct ScoreTerms { double s[RT_SCORE_SUMS]; uint32_t covered, skippedOut, skippedRaw; };

RT_DEV bool finite3(double r, double g, double b) { return isfinite(r) && isfinite(g) && isfinite(b); }
RT_DEV double luma(double r, double g, double b) {
#pragma clang fp contract(off)
  return (0.25 * r + 0.5 * g) + 0.25 * b;
}
RT_DEV double energy(double r, double g, double b) {
#pragma clang fp contract(off)
  return (r * r + g * g) + b * b;
}

// The terms of one pixel, in the order of RtggxScore's sums: se_out_rgb, se_out_luma, se_raw_rgb, se_raw_luma, ref_rgb2, ref_luma2,
// se_out_rgb_cov, se_raw_rgb_cov, ref_rgb2_cov.
RT_DEV void pixelTerms(const ScoreArgs& A, size_t pix, double t[RT_SCORE_SUMS], uint32_t& covered, uint32_t& skippedOut, uint32_t& skippedRaw) {
#pragma clang fp contract(off)
  const f4 o = unpackRGBA16F(A.out[pix]), r = unpackRGBA16F(A.ref[pix]);
  const uint32_t vis = (uint32_t)A.visDepth[pix];
  const f3 w0 = unpackR11G11B10F(A.refl[pix]);
  const uint32_t inst = (vis - 1u) >> 24;      // (two instances: an uploaded word that names another has no material -- accumulateKernel's rule)
  const bool cov = vis != 0u, diff = cov && inst < 2u && ((A.diffMask >> inst) & 1u);
  double wr = (double)w0.x, wg = (double)w0.y, wb = (double)w0.z;
  if (diff) { const f3 w1 = unpackR11G11B10F(A.diff[pix]); wr = wr + (double)w1.x; wg = wg + (double)w1.y; wb = wb + (double)w1.z; }
  const double rr = (double)r.x, rg = (double)r.y, rb = (double)r.z;
  const double orr = (double)o.x, og = (double)o.y, ob = (double)o.z;
  const bool refOk = finite3(rr, rg, rb);
  const bool outOk = refOk && finite3(orr, og, ob), rawOk = refOk && finite3(wr, wg, wb);
  const double yRef = luma(rr, rg, rb);
  double seOut = 0.0, seOutY = 0.0, seRaw = 0.0, seRawY = 0.0, ref2 = 0.0, refY2 = 0.0;
  if (outOk) {
    const double dy = luma(orr, og, ob) - yRef;
    seOut = energy(orr - rr, og - rg, ob - rb); seOutY = dy * dy;
    ref2 = energy(rr, rg, rb); refY2 = yRef * yRef;
  }
  if (rawOk) {
    const double dy = luma(wr, wg, wb) - yRef;
    seRaw = energy(wr - rr, wg - rg, wb - rb); seRawY = dy * dy;
  }
  t[0] = seOut; t[1] = seOutY; t[2] = seRaw; t[3] = seRawY; t[4] = ref2; t[5] = refY2;
  t[6] = cov ? seOut : 0.0; t[7] = cov ? seRaw : 0.0; t[8] = cov ? ref2 : 0.0;
  covered = cov ? 1u : 0u; skippedOut = outOk ? 0u : 1u; skippedRaw = rawOk ? 0u : 1u;
}

__global__ void __launch_bounds__(256) scorePixelsKernel(ScoreArgs A) {
#pragma clang fp contract(off)
  __shared__ double waveSum[RT_SCORE_SUMS][4];
  __shared__ uint32_t waveCount[3][4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t chunk = blockIdx.x; chunk < A.numChunks; chunk += gridDim.x) {
    const uint32_t p0 = chunk * RT_SCORE_CHUNK + threadIdx.x * 4u;      // (a frame has at most 2^28 pixels)
    double t[4][RT_SCORE_SUMS];
    uint32_t cnt[3] = {0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      if (p0 + k < A.count) {
        uint32_t c, so, sr;
        pixelTerms(A, (size_t)A.first + p0 + k, t[k], c, so, sr);
        cnt[0] += c; cnt[1] += so; cnt[2] += sr;
      } else {
#pragma unroll
        for (uint32_t s = 0; s < RT_SCORE_SUMS; ++s) t[k][s] = 0.0;
      }
    }
    double v[RT_SCORE_SUMS];
#pragma unroll
    for (uint32_t s = 0; s < RT_SCORE_SUMS; ++s) v[s] = (t[0][s] + t[1][s]) + (t[2][s] + t[3][s]);
#pragma unroll
    for (uint32_t m = 1u; m < 64u; m <<= 1) {
#pragma unroll
      for (uint32_t s = 0; s < RT_SCORE_SUMS; ++s) v[s] = v[s] + __shfl_xor(v[s], (int)m, 64);
#pragma unroll
      for (uint32_t q = 0; q < 3u; ++q) cnt[q] += (uint32_t)__shfl_xor((int)cnt[q], (int)m, 64);
    }
    if (lane == 0u) {
#pragma unroll
      for (uint32_t s = 0; s < RT_SCORE_SUMS; ++s) waveSum[s][wave] = v[s];
#pragma unroll
      for (uint32_t q = 0; q < 3u; ++q) waveCount[q][wave] = cnt[q];
    }
    __syncthreads();
    if (threadIdx.x < RT_SCORE_SUMS) {
      const uint32_t s = threadIdx.x;
      A.partial[(size_t)s * A.stride + chunk] = (waveSum[s][0] + waveSum[s][1]) + (waveSum[s][2] + waveSum[s][3]);
    } else if (threadIdx.x >= 64u && threadIdx.x < 67u) {
      const uint32_t q = threadIdx.x - 64u;
      A.counts[(size_t)chunk * 3u + q] = (waveCount[q][0] + waveCount[q][1]) + (waveCount[q][2] + waveCount[q][3]);
    }
    __syncthreads();      // (the next chunk's waves write the same LDS words)
  }
}

struct ScoreFinishArgs {
  double* level[2];      // [0]: stage 1's partials, RT_SCORE_SUMS x stride; [1]: room for half of that
  const uint32_t* counts;
  RtggxScore* record;
  uint64_t index, pixels;
  uint32_t frameIndex, numChunks, stride;      // stride: a power of two >= max(numChunks, 1)
};

#define RT_SCORE_FINISH_THREADS 1024u
__global__ void __launch_bounds__(RT_SCORE_FINISH_THREADS) scoreFinishKernel(ScoreFinishArgs A) {
#pragma clang fp contract(off)
  __shared__ unsigned long long countSum[3][RT_SCORE_FINISH_THREADS];
  const uint32_t tid = threadIdx.x;
  // the levels above a chunk: n values per sum at [sum * n + i] become n / 2 at [sum * (n / 2) + i]
  uint32_t src = 0u;
  for (uint32_t n = A.stride; n > 1u; n >>= 1) {
    const uint32_t half = n >> 1;
    const double* x = A.level[src]; double* y = A.level[src ^ 1u];
    const uint32_t valid = src == 0u && n == A.stride ? A.numChunks : n;      // beyond the last chunk: the padding, +0.0 (stage 1 wrote nothing there)
    for (uint32_t i = tid; i < RT_SCORE_SUMS * half; i += RT_SCORE_FINISH_THREADS) {
      const uint32_t s = i / half, j = i - s * half;
      const double a = 2u * j < valid ? x[(size_t)s * n + 2u * j] : 0.0;
      const double b = 2u * j + 1u < valid ? x[(size_t)s * n + 2u * j + 1u] : 0.0;
      y[(size_t)s * half + j] = a + b;
    }
    __syncthreads();      // (one workgroup: the barrier orders its global stores and loads)
    src ^= 1u;
  }
  // the counts: integers, any order
  unsigned long long c[3] = {0ull, 0ull, 0ull};
  for (uint32_t i = tid; i < A.numChunks; i += RT_SCORE_FINISH_THREADS) { c[0] += A.counts[(size_t)i * 3u]; c[1] += A.counts[(size_t)i * 3u + 1u]; c[2] += A.counts[(size_t)i * 3u + 2u]; }
  for (uint32_t q = 0; q < 3u; ++q) countSum[q][tid] = c[q];
  __syncthreads();
  for (uint32_t w = RT_SCORE_FINISH_THREADS / 2u; w > 0u; w >>= 1) {
    if (tid < w) for (uint32_t q = 0; q < 3u; ++q) countSum[q][tid] += countSum[q][tid + w];
    __syncthreads();
  }
  if (tid == 0u) {
    const double* r = A.level[src];
    const bool any = A.numChunks > 0u;
    RtggxScore S;
    S.index = A.index; S.frame_index = A.frameIndex; S.pad = 0u;
    S.pixels = A.pixels; S.covered = countSum[0][0]; S.skipped_out = countSum[1][0]; S.skipped_raw = countSum[2][0];
    S.se_out_rgb = any ? r[0] : 0.0; S.se_out_luma = any ? r[1] : 0.0; S.se_raw_rgb = any ? r[2] : 0.0; S.se_raw_luma = any ? r[3] : 0.0;
    S.ref_rgb2 = any ? r[4] : 0.0; S.ref_luma2 = any ? r[5] : 0.0;
    S.se_out_rgb_cov = any ? r[6] : 0.0; S.se_raw_rgb_cov = any ? r[7] : 0.0; S.ref_rgb2_cov = any ? r[8] : 0.0;
    *A.record = S;
  }
}

int launchScore(rtggx_context* c, const FrameParams& fp, hipStream_t s) {
  if (!c->reference || !c->scoreRing || !c->scorePartial[0] || !c->scorePartial[1] || !c->scoreCounts) { setError("rtggx_denoise: scoring without its buffers"); return -1; }
  const uint32_t rows = fp.rowEnd > fp.rowBegin ? fp.rowEnd - fp.rowBegin : 0u;
  const uint32_t count = rows * fp.W, numChunks = (count + RT_SCORE_CHUNK - 1u) / RT_SCORE_CHUNK;
  uint32_t stride = 1u; while (stride < numChunks) stride <<= 1;
  if (stride > c->scoreStride) { setError("rtggx_denoise: %u chunks of scored pixels, room for %u", numChunks, c->scoreStride); return -1; }
  if (numChunks) {
    ScoreArgs A;
    A.out = c->tss[c->frameParity]; A.ref = c->reference; A.refl = c->cur().rtRefl; A.diff = c->cur().rtDiff; A.visDepth = c->curVis().depth;
    A.partial = c->scorePartial[0]; A.counts = c->scoreCounts;
    A.first = fp.rowBegin * fp.W; A.count = count; A.numChunks = numChunks; A.stride = stride;
    A.diffMask = (fp.mat.RoughMetals[0][1] < 1.0f ? 1u : 0u) | (fp.mat.RoughMetals[1][1] < 1.0f ? 2u : 0u);
    // few waves that stream (the frame is bound by wave slots): at most two workgroups per CU, each looping over chunks
    const uint32_t grid = numChunks < 2u * c->numCUs ? numChunks : 2u * c->numCUs;
    hipLaunchKernelGGL(scorePixelsKernel, dim3(grid), dim3(256), 0, s, A);
  }
  ScoreFinishArgs F;
  F.level[0] = c->scorePartial[0]; F.level[1] = c->scorePartial[1]; F.counts = c->scoreCounts;
  F.record = c->scoreRing + (c->scoreIndex % (uint64_t)RTGGX_SCORE_RING);
  F.index = c->scoreIndex; F.pixels = count; F.frameIndex = fp.g.FrameIndex; F.numChunks = numChunks; F.stride = stride;
  hipLaunchKernelGGL(scoreFinishKernel, dim3(1), dim3(RT_SCORE_FINISH_THREADS), 0, s, F);
  RT_HIP(hipGetLastError());
  ++c->scoreIndex;
  return 0;
}

// rtggx_reference_from_accumulation: presentAccumulationKernel's arithmetic (raytrace.hip) into the reference image -- per component
// (float)((double)sum / (double)n) of each image, the two means added in fp32, alpha 1.
__global__ void __launch_bounds__(256) referenceFromAccumulationKernel(const float4* __restrict__ accRefl, const float4* __restrict__ accDiff, uint2* __restrict__ out, uint32_t count, uint32_t frames) {
#pragma clang fp contract(off)
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  const double n = (double)frames;
  const float4 a = accRefl[i], d = accDiff[i];
  const float r = (float)((double)a.x / n) + (float)((double)d.x / n);
  const float g = (float)((double)a.y / n) + (float)((double)d.y / n);
  const float b = (float)((double)a.z / n) + (float)((double)d.z / n);
  out[i] = packRGBA16F(r, g, b, 1.0f);
}
int launchReferenceFromAccumulation(rtggx_context* c, hipStream_t s) {
  const uint32_t count = c->W * c->H;
  hipLaunchKernelGGL(referenceFromAccumulationKernel, dim3((count + 255u) / 256u), dim3(256), 0, s, (const float4*)c->accRefl, (const float4*)c->accDiff, c->reference, count, c->accumFrames);
  RT_HIP(hipGetLastError());
  return 0;
}

}  // namespace rt
