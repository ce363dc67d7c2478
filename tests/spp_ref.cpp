// TEST INFRASTRUCTURE ONLY.  tests/recursion_ref.cpp (the whole CPU oracle plus follow_path) plus orc_ray_trace_spp(h, D, N): raygenMain at
// recursion depth D with N samples per covered pixel -- the semantics of rtggx_set_samples_per_pixel (include/rtggx.h, DESIGN.md "Samples
// per pixel").  It is raygen_pixel_depth with the sample loop: sample k takes xi = get_sample_param(pixel, FrameIndex * N + k), its value
// v_k = c_k * T_k is what the one-sample frame packs (0 where NoL <= 0), and the pixel's word is pack_r11g11b10((0 + v_0 + ... + v_{N-1}) *
// (1 / N)), summed in that order in fp32.  Built by tests/restatement.py with the oracle Makefile's flags.  At N = 1 it reproduces
// orc_ray_trace / orc_ray_trace_depth bit for bit (tests/test_spp_host.py); N = 2, 4, 8 pin the product's multi-sample frames.
#include "recursion_ref.cpp"

namespace orc {

// Returns the rays traced.  sumRefl / sumDiff (may be null): the pixel's fp32 results before packing, 3 floats per pixel (tests of the
// averaging itself; there N may be any count, and 1 / N is then rounded once).
static inline uint32_t raygen_pixel_spp(Ctx& c, uint32_t px, uint32_t py, uint32_t D, uint32_t N, float* sumRefl, float* sumDiff, float* primary = nullptr) {
  const uint32_t W = c.W, H = c.H; const size_t pix = (size_t)py * W + px;
  const FrameConstants& fc = c.fc;
  uint32_t rays = 0;
  Surface s{};
  uint32_t visibility = c.vis[pix];
  float2 screenPos = {((float)px + 0.5f) / (float)W * 2.0f - 1.0f, ((float)py + 0.5f) / (float)H * 2.0f - 1.0f};
  screenPos.y = -screenPos.y;
  const float3 eye = f3(fc.rg.EyePt[0], fc.rg.EyePt[1], fc.rg.EyePt[2]);
  if (visibility > 0) {
    --visibility;
    s.hit = true; s.inst = visibility >> 24; s.prim = visibility & 0xFFFFFFu;
    const Vertex3 v = get_vertices(c, s.inst, s.prim);
    const M4 wvp = cb_load4x4(fc.g.WorldViewProjs[s.inst]);
    float4 p[3];
    for (int k = 0; k < 3; ++k) p[k] = mul_point(v.pos[k], wvp);
    screenPos.x -= fc.rg.ProjBias[0]; screenPos.y -= fc.rg.ProjBias[1];
    const float2 bary = calc_barycentrics(p, screenPos);
    const Attrib a = interp_attrib(v, bary.x, bary.y);
    s.color = f3(fc.mat.BaseColors[s.inst][0], fc.mat.BaseColors[s.inst][1], fc.mat.BaseColors[s.inst][2]);
    s.rghMtl = get_rough_metal(c, s.inst, a.UV);
    const float4 hPrev = mul_point(a.Pos, cb_load4x4(fc.g.WorldViewProjsPrev[s.inst]));
    s.velocity = {(screenPos.x - hPrev.x / hPrev.w) * 0.5f, (screenPos.y - hPrev.y / hPrev.w) * -0.5f};
    const float4 P4 = mul_point(a.Pos, cb_load4x3(fc.g.Worlds[s.inst]));
    s.P = f3(P4.x, P4.y, P4.z);
    s.N = normalize(mul_dir(a.Nrm, cb_load3x3(s.inst ? fc.g.WorldIT1 : fc.g.WorldITs0)));
    s.V = normalize(eye - s.P);
  } else {
    const float4 world = mul_vec4(float4{screenPos.x, screenPos.y, 0.0f, 1.0f}, cb_load4x4(fc.rg.ProjToWorld));
    s.hit = false; s.velocity = {0.0f, 0.0f};
    s.P = f3(world.x / world.w, world.y / world.w, world.z / world.w);
    s.N = f3(0, 0, 0);
    s.V = normalize(eye - s.P);
    s.rghMtl = {0.0f, 0.0f};
    s.color = f3(0, 0, 0);
  }
  c.normal[pix] = pack_r10g10b10a2(s.N.x * 0.5f + 0.5f, s.N.y * 0.5f + 0.5f, s.N.z * 0.5f + 0.5f, s.hit ? 1.0f : 0.0f);
  if (s.hit) c.roughMetal[pix] = pack_r8g8(s.rghMtl.x, s.rghMtl.y);
  c.velocity[pix] = pack_r16g16f(s.velocity.x, s.velocity.y);
  if (primary) {      // the primary surface in front of the G-buffer's packs: N * 0.5 + 0.5, the velocity, the roughness
    float* g = primary + 6 * pix;
    g[0] = s.N.x * 0.5f + 0.5f; g[1] = s.N.y * 0.5f + 0.5f; g[2] = s.N.z * 0.5f + 0.5f; g[3] = s.velocity.x; g[4] = s.velocity.y; g[5] = s.rghMtl.x;
  }

  if (!s.hit) {      // background: the environment along -V into both images, no ray and no averaging
    const float3 e = environment(c, -s.V, 0.0f);
    c.refl[pix] = pack_r11g11b10f(e.x, e.y, e.z);
    c.diff[pix] = c.refl[pix];
    if (sumRefl) { sumRefl[3 * pix] = e.x; sumRefl[3 * pix + 1] = e.y; sumRefl[3 * pix + 2] = e.z; }
    if (sumDiff) { sumDiff[3 * pix] = e.x; sumDiff[3 * pix + 1] = e.y; sumDiff[3 * pix + 2] = e.z; }
    return 0;
  }
  const bool diffuse = s.rghMtl.y < 1.0f;
  float3 accR = f3(0, 0, 0), accD = f3(0, 0, 0);
  for (uint32_t k = 0; k < N; ++k) {
    const SampleParam xi = get_sample_param(px, py, W, fc.g.FrameIndex * N + k);
    {  // the reflection path: level 0 is computeReflection at depth 0 (:424-484)
      const float a = s.rghMtl.x * s.rghMtl.x;
      float3 Hh;
      if (c.vndf) Hh = vndf_half_vector(s.N, s.V, a, c.cosTab[xi.s], c.sinTab[xi.s], xi.y);
      else {
        const float cosTheta = std::sqrt((1.0f - xi.y) / (1.0f + (a * a - 1.0f) * xi.y));
        const float sinTheta = std::sqrt(1.0f - cosTheta * cosTheta);
        Hh = local_to_world(s.N, f3(c.cosTab[xi.s] * sinTheta, c.sinTab[xi.s] * sinTheta, cosTheta));
      }
      const float3 R = reflect(-s.V, Hh);
      const float NoL = dot(s.N, R);
      float3 v = f3(0, 0, 0);
      if (NoL > 0.0f) {
        const float3 f0 = f3(lerp(0.04f, s.color.x, s.rghMtl.y), lerp(0.04f, s.color.y, s.rghMtl.y), lerp(0.04f, s.color.z, s.rghMtl.y));
        const float NoV = saturate(dot(s.N, s.V));
        const float VoH = saturate(dot(s.V, Hh));
        const float3 F = f_schlick(f0, VoH);
        const float vis = vis_smith(s.rghMtl.x, NoV, NoL);
        const float NoH = saturate(dot(s.N, Hh));
        const float kk = 4.0f * VoH / NoH;
        float3 T = f3(((NoL * F.x) * vis) * kk, ((NoL * F.y) * vis) * kk, ((NoL * F.z) * vis) * kk);   // w0
        if (c.vndf) {
          const float a2 = a * a;
          const float g1l = (2.0f * NoL) / (NoL + std::sqrt(NoL * (NoL - NoL * a2) + a2));
          T = f3(F.x * g1l, F.y * g1l, F.z * g1l);
        }
        const float3 col = follow_path(c, s.P, R, s.inst, s.prim, false, s.color * s.rghMtl.y, xi, D, T, rays);
        v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      }
      accR = f3(accR.x + v.x, accR.y + v.y, accR.z + v.z);
    }
    if (diffuse) {   // the diffuse path: level 0 is computeDiffuse at depth 0 (:486-535)
      const float cosTheta = 1.0f - 2.0f * xi.y;
      const float sinTheta = std::sqrt(1.0f - cosTheta * cosTheta);
      const float3 dir = normalize(s.N + f3(c.cosTab[xi.s] * sinTheta, c.sinTab[xi.s] * sinTheta, cosTheta));
      float3 T = s.color * (1.0f - 0.04f);                                                     // w0 (:532)
      const float3 col = follow_path(c, s.P, dir, s.inst, s.prim, true, s.color * s.rghMtl.y, xi, D, T, rays);
      const float3 v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      accD = f3(accD.x + v.x, accD.y + v.y, accD.z + v.z);
    }
  }
  const float scale = 1.0f / (float)N;
  accR = f3(accR.x * scale, accR.y * scale, accR.z * scale);
  c.refl[pix] = pack_r11g11b10f(accR.x, accR.y, accR.z);
  if (sumRefl) { sumRefl[3 * pix] = accR.x; sumRefl[3 * pix + 1] = accR.y; sumRefl[3 * pix + 2] = accR.z; }
  if (diffuse) {
    accD = f3(accD.x * scale, accD.y * scale, accD.z * scale);
    c.diff[pix] = pack_r11g11b10f(accD.x, accD.y, accD.z);
    if (sumDiff) { sumDiff[3 * pix] = accD.x; sumDiff[3 * pix + 1] = accD.y; sumDiff[3 * pix + 2] = accD.z; }
  }
  return rays;
}

}  // namespace orc

extern "C" uint64_t orc_ray_trace_spp_f32(void* h, uint32_t depth, uint32_t samples, float* sumRefl, float* sumDiff) {
  Ctx* c = (Ctx*)h;
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) { uint64_t r = 0; for (uint32_t x = 0; x < c->W; ++x) r += raygen_pixel_spp(*c, x, y, depth, samples, sumRefl, sumDiff); rays += r; });
  c->rayCount = rays.load();
  return c->rayCount;
}
// ... and the primary surface's values in front of the G-buffer's packs (tests/test_shading_ref_host.py measures the model's distance from them)
extern "C" uint64_t orc_ray_trace_spp_primary_f32(void* h, uint32_t depth, uint32_t samples, float* sumRefl, float* sumDiff, float* primary) {
  Ctx* c = (Ctx*)h;
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) { uint64_t r = 0; for (uint32_t x = 0; x < c->W; ++x) r += raygen_pixel_spp(*c, x, y, depth, samples, sumRefl, sumDiff, primary); rays += r; });
  c->rayCount = rays.load();
  return c->rayCount;
}
extern "C" uint64_t orc_ray_trace_spp(void* h, uint32_t depth, uint32_t samples) { return orc_ray_trace_spp_f32(h, depth, samples, nullptr, nullptr); }
