// TEST INFRASTRUCTURE ONLY.  CPU restatement of the sun at the surfaces the paths hit (rtggx_set_sun_reflections; include/rtggx.h has the
// rule): tests/sun_ref.cpp -- the whole oracle, the depth, spp and sample-set restatements and orc_sun_apply -- plus
// orc_ray_trace_sun_hits(h, D, N, M, L, E, flags, counts, lit): tests/sampleset_ref.cpp's path walker once more, with the rule inside it.
// flags bit 0: the toggle (clear: the walker is raygen_pixel_m's, line by line); bit 1: the terms go into the fp32 sums even at N = 1 (a
// block of a sample map that gets one sample of an N-sample frame).  counts (may be null): [4 levels][SH_COLUMNS] -- per level the rays that
// miss, that return their preset, and the touched hits facing away, occluded and lit, then among the sun-facing ones the two lobes -- ADDED
// to what the array holds.  lit (may be null): per pixel bit 0 / 1, a term exists in RayTracingOut0 / RayTracingOut1.  Occlusion is the
// `valid` of the oracle's closest hit on the shadow ray, as in sun_ref.cpp.  The primary pass (orc_sun_apply) is the caller's to run
// afterwards.  Every operation is fp32, rounded on its own (-ffp-contract=off).
#include "sun_ref.cpp"

namespace orc {
enum { SH_MISS = 0, SH_PRESET, SH_AWAY, SH_OCCLUDED, SH_LIT, SH_SPECULAR, SH_DIFFUSE, SH_COLUMNS };
struct SunHits { bool on, sums; float3 L, E; };
struct SunHitCounts { uint64_t n[4][SH_COLUMNS] = {}; };

// step 3 of the rule: the lobe the path uses at the surface
static inline float3 sun_hit_term(const SunHits& sun, float3 N, float3 V, float2 rm, float3 color, bool diffuseGroup, float NoL) {
  const float3 L = sun.L, E = sun.E;
  if (rm.y > 0.5f) {
    const float r = std::fmax(rm.x, 1.0f / 32.0f);
    const float3 Hh = normalize(V + L);
    const float NoH = saturate(dot(N, Hh)), VoH = saturate(dot(V, Hh)), NoV = saturate(dot(N, V));
    const float al = r * r, a2 = al * al;
    const float d = (NoH * a2 - NoH) * NoH + 1.0f;
    const float D = a2 / ((kPI * d) * d);
    const float3 f0 = f3(lerp(0.04f, color.x, rm.y), lerp(0.04f, color.y, rm.y), lerp(0.04f, color.z, rm.y));
    const float3 F = f_schlick(f0, VoH);
    const float vis = vis_smith(r, NoV, NoL);
    const float k = (D * vis) * NoL;
    return f3((F.x * k) * E.x, (F.y * k) * E.y, (F.z * k) * E.z);
  }
  if (diffuseGroup) color = color * (1.0f - rm.y);
  const float w = NoL / kPI;
  return f3((color.x * w) * E.x, (color.y * w) * E.y, (color.z * w) * E.z);
}

// follow_path_m with the rule: S takes s_d = T_d * term at every touched, sun-facing, unoccluded hit, levels ascending (with the sums
// rule S is the pixel's sum itself, which then gets the path's value behind the terms: the caller's add)
static inline float3 follow_path_h(const Ctx& c, float3 o, float3 dir, uint32_t skipInst, uint32_t skipPrim, bool diffuseGroup, float3 preset,
                                   const SampleM& xi, uint32_t D, float3& T, uint32_t& rays, const SunHits& sun, float3& S, bool& any, SunHitCounts& n) {
  for (uint32_t d = 0;; ++d) {
    ++rays;
    const Hit h = trace_closest(c, o, dir, 1e-5f, 10000.0f, skipInst, skipPrim);
    if (!h.valid) { ++n.n[d][SH_MISS]; return environment(c, dir, 0.0f); }
    if (!diffuseGroup && preset.x <= 0.0f && preset.y <= 0.0f && preset.z <= 0.0f) { ++n.n[d][SH_PRESET]; return preset; }
    float3 N, color; float2 rm; hit_surface(c, h, N, rm, color);
    const float3 V = -dir;
    const float3 P = f3(o.x + h.t * dir.x, o.y + h.t * dir.y, o.z + h.t * dir.z);
    if (sun.on) {
      const float NoL = dot(N, sun.L);
      if (NoL <= 0.0f) ++n.n[d][SH_AWAY];
      else {
        ++n.n[d][rm.y > 0.5f ? SH_SPECULAR : SH_DIFFUSE];
        ++rays;
        if (trace_closest(c, P, sun.L, 1e-5f, 10000.0f, h.inst, h.prim).valid) ++n.n[d][SH_OCCLUDED];
        else {
          ++n.n[d][SH_LIT];
          const float3 term = sun_hit_term(sun, N, V, rm, color, diffuseGroup, NoL);
          S = f3(S.x + T.x * term.x, S.y + T.y * term.y, S.z + T.z * term.z);
          any = true;
        }
      }
    }
    if (d + 1 == D) {
      if (rm.y > 0.5f) return reflection_depth1(c, rm, N, V, color);
      return diffuse_depth1(c, N, diffuseGroup ? color * (1.0f - rm.y) : color);
    }
    float3 L, w;
    if (rm.y > 0.5f) {
      const float3 Hh = half_vector_m(c, N, V, rm.x * rm.x, xi);
      L = reflect(-V, Hh);
      const float NoL = dot(N, L);
      if (NoL <= 0.0f) return f3(0, 0, 0);
      w = reflection_weight_m(c, N, V, Hh, NoL, rm, color);
      diffuseGroup = false;
    } else {
      if (diffuseGroup) color = color * (1.0f - rm.y);
      L = diffuse_direction_m(N, xi);
      w = color;
      diffuseGroup = true;
    }
    preset = color * rm.y;
    T = f3(T.x * w.x, T.y * w.y, T.z * w.z);
    o = P; dir = L; skipInst = h.inst; skipPrim = h.prim;
  }
}

static inline uint32_t raygen_pixel_h(Ctx& c, const TableM& t, uint32_t px, uint32_t py, uint32_t D, uint32_t N, uint32_t M, const SunHits& sun, SunHitCounts& n, uint8_t* lit) {
  const uint32_t W = c.W, H = c.H; const size_t pix = (size_t)py * W + px;
  const FrameConstants& fc = c.fc;
  uint32_t rays = 0;
  Surface s{};
  uint32_t visibility = c.vis[pix];
  float2 screenPos = {((float)px + 0.5f) / (float)W * 2.0f - 1.0f, ((float)py + 0.5f) / (float)H * 2.0f - 1.0f};
  screenPos.y = -screenPos.y;
  const float3 eye = f3(fc.rg.EyePt[0], fc.rg.EyePt[1], fc.rg.EyePt[2]);
  if (lit) lit[pix] = 0;
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

  if (!s.hit) {      // background: no path, no term
    const float3 e = environment(c, -s.V, 0.0f);
    c.refl[pix] = pack_r11g11b10f(e.x, e.y, e.z);
    c.diff[pix] = c.refl[pix];
    return 0;
  }
  const bool diffuse = s.rghMtl.y < 1.0f;
  float3 accR = f3(0, 0, 0), accD = f3(0, 0, 0), SR = f3(0, 0, 0), SD = f3(0, 0, 0);
  bool anyR = false, anyD = false;
  for (uint32_t k = 0; k < N; ++k) {
    const SampleM xi = get_sample_param_m(t, px, py, W, fc.g.FrameIndex * N + k, M);
    {
      const float3 Hh = half_vector_m(c, s.N, s.V, s.rghMtl.x * s.rghMtl.x, xi);
      const float3 R = reflect(-s.V, Hh);
      const float NoL = dot(s.N, R);
      float3 v = f3(0, 0, 0);
      if (NoL > 0.0f) {
        float3 T = reflection_weight_m(c, s.N, s.V, Hh, NoL, s.rghMtl, s.color);
        const float3 col = follow_path_h(c, s.P, R, s.inst, s.prim, false, s.color * s.rghMtl.y, xi, D, T, rays, sun, sun.sums ? accR : SR, anyR, n);
        v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      }
      accR = f3(accR.x + v.x, accR.y + v.y, accR.z + v.z);
    }
    if (diffuse) {
      const float3 dir = diffuse_direction_m(s.N, xi);
      float3 T = s.color * (1.0f - 0.04f);
      const float3 col = follow_path_h(c, s.P, dir, s.inst, s.prim, true, s.color * s.rghMtl.y, xi, D, T, rays, sun, sun.sums ? accD : SD, anyD, n);
      const float3 v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      accD = f3(accD.x + v.x, accD.y + v.y, accD.z + v.z);
    }
  }
  const float scale = 1.0f / (float)N;
  c.refl[pix] = pack_r11g11b10f(accR.x * scale, accR.y * scale, accR.z * scale);
  if (diffuse) c.diff[pix] = pack_r11g11b10f(accD.x * scale, accD.y * scale, accD.z * scale);
  if (!sun.sums) {      // one sample: the packed add, where a term exists
    float rgb[3];
    if (anyR) { unpack_r11g11b10f(c.refl[pix], rgb); c.refl[pix] = pack_r11g11b10f(rgb[0] + SR.x, rgb[1] + SR.y, rgb[2] + SR.z); }
    if (anyD) { unpack_r11g11b10f(c.diff[pix], rgb); c.diff[pix] = pack_r11g11b10f(rgb[0] + SD.x, rgb[1] + SD.y, rgb[2] + SD.z); }
  }
  if (lit) lit[pix] = (uint8_t)((anyR ? 1 : 0) | (anyD ? 2 : 0));
  return rays;
}
}  // namespace orc

extern "C" uint32_t orc_sun_hit_columns() { return orc::SH_COLUMNS; }
extern "C" uint64_t orc_ray_trace_sun_hits(void* h, uint32_t depth, uint32_t samples, uint32_t M, const float* L, const float* E, uint32_t flags, uint64_t* counts, uint8_t* lit) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  const TableM& t = table_m(M);
  SunHits sun;
  sun.on = (flags & 1u) != 0u; sun.sums = (flags & 2u) != 0u || samples > 1u;
  sun.L = L ? f3(L[0], L[1], L[2]) : f3(0, 0, 0); sun.E = E ? f3(E[0], E[1], E[2]) : f3(0, 0, 0);
  std::atomic<uint64_t> rays{0};
  std::mutex lock;
  parallel_rows(c->threads, c->H, [&](uint32_t y) {
    uint64_t r = 0; SunHitCounts n;
    for (uint32_t x = 0; x < c->W; ++x) r += raygen_pixel_h(*c, t, x, y, depth, samples, M, sun, n, lit);
    rays += r;
    if (counts) { std::lock_guard<std::mutex> g(lock); for (int d = 0; d < 4; ++d) for (int k = 0; k < SH_COLUMNS; ++k) counts[d * SH_COLUMNS + k] += n.n[d][k]; }
  });
  c->rayCount = rays.load();
  return c->rayCount;
}
