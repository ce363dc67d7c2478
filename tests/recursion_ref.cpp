// TEST INFRASTRUCTURE ONLY.  The CPU oracle (oracle/orc_capi.cpp, included whole) plus orc_ray_trace_depth(h, D): raygenMain
// (RayTracing.hlsl:541-565) at recursion depth D, i.e. the reference's shaders with the closest hits (:571-614) passing
// payload.RecursionDepth + 1 -- the semantics of rtggx_set_max_recursion_depth (include/rtggx.h, DESIGN.md "Recursion depth").  Built by
// tests/restatement.py with the oracle Makefile's flags.  At D = 1 it reproduces orc_ray_trace bit for bit through the same path loop
// (tests/test_recursion_host.py); D = 2..4 pin the product's multi-bounce frames.
#include "../oracle/orc_capi.cpp"

namespace orc {

// A path from its level-0 ray on: the value c at its end.  T: the path's throughput, T_{d+1} = T_d * w_{d+1} (multiplied forward, one
// fp32 product per component); rays: incremented per traced ray.  preset: colour x metallic of the surface the ray left (:456).
static inline float3 follow_path(const Ctx& c, float3 o, float3 dir, uint32_t skipInst, uint32_t skipPrim, bool diffuseGroup, float3 preset,
                                 const SampleParam& xi, uint32_t D, float3& T, uint32_t& rays) {
  for (uint32_t d = 0;; ++d) {
    ++rays;
    const Hit h = trace_closest(c, o, dir, 1e-5f, 10000.0f, skipInst, skipPrim);
    if (!h.valid) return environment(c, dir, 0.0f);                                          // missMain :620-625
    if (!diffuseGroup && preset.x <= 0.0f && preset.y <= 0.0f && preset.z <= 0.0f) return preset;   // closestHitReflection :573
    float3 N, color; float2 rm; hit_surface(c, h, N, rm, color);
    const float3 V = -dir;
    if (d + 1 == D) {                                                                        // depth D reached: the depth-1 shading
      if (rm.y > 0.5f) return reflection_depth1(c, rm, N, V, color);
      return diffuse_depth1(c, N, diffuseGroup ? color * (1.0f - rm.y) : color);
    }
    const float3 P = f3(o.x + h.t * dir.x, o.y + h.t * dir.y, o.z + h.t * dir.z);           // hitWorldPosition :338-341
    float3 L, w;
    if (rm.y > 0.5f) {                                                                       // computeReflection at depth d + 1
      const float a = rm.x * rm.x;
      float3 Hh;
      if (c.vndf) Hh = vndf_half_vector(N, V, a, c.cosTab[xi.s], c.sinTab[xi.s], xi.y);
      else {
        const float cosTheta = std::sqrt((1.0f - xi.y) / (1.0f + (a * a - 1.0f) * xi.y));
        const float sinTheta = std::sqrt(1.0f - cosTheta * cosTheta);
        Hh = local_to_world(N, f3(c.cosTab[xi.s] * sinTheta, c.sinTab[xi.s] * sinTheta, cosTheta));
      }
      L = reflect(-V, Hh);
      const float NoL = dot(N, L);
      if (NoL <= 0.0f) return f3(0, 0, 0);                                                  // :459
      const float3 f0 = f3(lerp(0.04f, color.x, rm.y), lerp(0.04f, color.y, rm.y), lerp(0.04f, color.z, rm.y));
      const float NoV = saturate(dot(N, V));
      const float VoH = saturate(dot(V, Hh));
      const float3 F = f_schlick(f0, VoH);
      const float vis = vis_smith(rm.x, NoV, NoL);
      const float NoH = saturate(dot(N, Hh));
      const float k = 4.0f * VoH / NoH;
      w = f3(((NoL * F.x) * vis) * k, ((NoL * F.y) * vis) * k, ((NoL * F.z) * vis) * k);   // :477
      if (c.vndf) {
        const float a2 = a * a;
        const float g1l = (2.0f * NoL) / (NoL + std::sqrt(NoL * (NoL - NoL * a2) + a2));
        w = f3(F.x * g1l, F.y * g1l, F.z * g1l);
      }
      diffuseGroup = false;
    } else {                                                                                 // computeDiffuse at depth d + 1
      if (diffuseGroup) color = color * (1.0f - rm.y);                                      // :607
      const float cosTheta = 1.0f - 2.0f * xi.y;
      const float sinTheta = std::sqrt(1.0f - cosTheta * cosTheta);
      L = normalize(N + f3(c.cosTab[xi.s] * sinTheta, c.sinTab[xi.s] * sinTheta, cosTheta));
      w = color;                                                                             // no x (1 - 0.04) at depth >= 1 (:532)
      diffuseGroup = true;
    }
    preset = color * rm.y;
    T = f3(T.x * w.x, T.y * w.y, T.z * w.z);
    o = P; dir = L; skipInst = h.inst; skipPrim = h.prim;
  }
}

// raygen_pixel (orc_raytrace.h) with the closest-hit shading of its two rays replaced by follow_path.  Returns the rays traced.
static inline uint32_t raygen_pixel_depth(Ctx& c, uint32_t px, uint32_t py, uint32_t D) {
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

  const SampleParam xi = get_sample_param(px, py, W, fc.g.FrameIndex);

  // the reflection path: level 0 is computeReflection at depth 0 (:424-484)
  float3 refl;
  if (!s.hit) refl = environment(c, -s.V, 0.0f);
  else {
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
    if (NoL <= 0.0f) refl = f3(0, 0, 0);
    else {
      const float3 f0 = f3(lerp(0.04f, s.color.x, s.rghMtl.y), lerp(0.04f, s.color.y, s.rghMtl.y), lerp(0.04f, s.color.z, s.rghMtl.y));
      const float NoV = saturate(dot(s.N, s.V));
      const float VoH = saturate(dot(s.V, Hh));
      const float3 F = f_schlick(f0, VoH);
      const float vis = vis_smith(s.rghMtl.x, NoV, NoL);
      const float NoH = saturate(dot(s.N, Hh));
      const float k = 4.0f * VoH / NoH;
      float3 T = f3(((NoL * F.x) * vis) * k, ((NoL * F.y) * vis) * k, ((NoL * F.z) * vis) * k);   // w0
      if (c.vndf) {
        const float a2 = a * a;
        const float g1l = (2.0f * NoL) / (NoL + std::sqrt(NoL * (NoL - NoL * a2) + a2));
        T = f3(F.x * g1l, F.y * g1l, F.z * g1l);
      }
      const float3 col = follow_path(c, s.P, R, s.inst, s.prim, false, s.color * s.rghMtl.y, xi, D, T, rays);
      refl = f3(col.x * T.x, col.y * T.y, col.z * T.z);
    }
  }
  c.refl[pix] = pack_r11g11b10f(refl.x, refl.y, refl.z);

  if (s.rghMtl.y < 1.0f) {   // the diffuse path: level 0 is computeDiffuse at depth 0 (:486-535)
    float3 diff;
    if (!s.hit) diff = environment(c, -s.V, 0.0f);
    else {
      const float cosTheta = 1.0f - 2.0f * xi.y;
      const float sinTheta = std::sqrt(1.0f - cosTheta * cosTheta);
      const float3 dir = normalize(s.N + f3(c.cosTab[xi.s] * sinTheta, c.sinTab[xi.s] * sinTheta, cosTheta));
      float3 T = s.color * (1.0f - 0.04f);                                                     // w0 (:532)
      const float3 col = follow_path(c, s.P, dir, s.inst, s.prim, true, s.color * s.rghMtl.y, xi, D, T, rays);
      diff = f3(col.x * T.x, col.y * T.y, col.z * T.z);
    }
    c.diff[pix] = pack_r11g11b10f(diff.x, diff.y, diff.z);
  }
  return rays;
}

}  // namespace orc

extern "C" uint64_t orc_ray_trace_depth(void* h, uint32_t depth) {
  Ctx* c = (Ctx*)h;
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) { uint64_t r = 0; for (uint32_t x = 0; x < c->W; ++x) r += raygen_pixel_depth(*c, x, y, depth); rays += r; });
  c->rayCount = rays.load();
  return c->rayCount;
}
