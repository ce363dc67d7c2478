// TEST INFRASTRUCTURE ONLY.  CPU restatement of a sun with a size (rtggx_set_sun_angle; include/rtggx.h has the rule): tests/sun_hit_ref.cpp
// -- the whole oracle, every restatement, orc_sun_apply and orc_ray_trace_sun_hits -- plus the rule's direction (sun_disk_direction), the
// primary pass with it (orc_sun_soft_apply) and sun_hit_ref.cpp's path walker once more with it (orc_ray_trace_sun_soft_hits).  The disk is
// the caller's: T, B and k as the host makes them (tests/sun_soft_ref.py mirrors that).
// The primary pass.  classes (may be null): sun_ref.cpp's 0-3 by the SAMPLED ray, and 4 "below the horizon" (NoL > 0, dot(N, Ls) <= 0: no
// ray, no term).  centre (may be null): per pixel the class the directional sun gives, 0-3, from one more ray that is counted nowhere.
// unoccluded: every ray that exists counts as unoccluded -- with k = 0 the directional sun's LIT word at every sun-facing pixel, which the
// tests compare a pixel that the disk lights against.
// The walker.  counts: sun_hit_ref.cpp's, by the sampled ray (a hit below the horizon is in none of facing-away / occluded / lit, but in
// its lobe's column).  soft (may be null): [4 levels][2] -- hits below the horizon, and (statistics on) hits whose sampled ray's outcome
// differs from the centre ray's -- ADDED to what the array holds.  changed (may be null): per pixel bit 0 / 1, a hit of the path that
// writes RayTracingOut0 / 1 is of one of those two kinds.  Every operation is fp32, rounded on its own (-ffp-contract=off).
#include "sun_hit_ref.cpp"

namespace orc {
struct SunDisk { float3 T, B; float k; };
struct SunSoftCounts { uint64_t n[4][2] = {}; };
enum { SS_BELOW = 0, SS_DIFFERS = 1 };

// steps 1-5 of the rule; u and s (may be null): the disk coordinates drawn
static inline float3 sun_disk_direction(const SunDisk& K, float3 L, uint32_t pixel, uint32_t frameIndex, uint32_t j, float* uOut = nullptr, uint32_t* sOut = nullptr) {
  const TableM& t = table_m(256);      // always the 256-entry table, whatever the sample set
  uint32_t h = rng(pixel); h += frameIndex; h = rng(h);
  const uint32_t w = rng(h + j * 0x9E3779B9u);
  const float u = (float)(w & 0xffffu) / 65536.0f;
  const uint32_t s = w >> 24;
  const float cosPhi = t.cosTab[s], sinPhi = t.sinTab[s];
  const float e = u * K.k;
  const float cosTheta = 1.0f - e, sinTheta = std::sqrt(e * (2.0f - e));
  const float ct = cosPhi * sinTheta, st = sinPhi * sinTheta;
  if (uOut) *uOut = u;
  if (sOut) *sOut = s;
  return f3((K.T.x * ct + K.B.x * st) + L.x * cosTheta, (K.T.y * ct + K.B.y * st) + L.y * cosTheta, (K.T.z * ct + K.B.z * st) + L.z * cosTheta);
}

// sun_ref.cpp's sun_pixel with step 6 and 7 of the rule: the ray along Ls, the term at L
static inline uint32_t sun_soft_pixel(Ctx& c, uint32_t px, uint32_t py, float3 L, float3 E, const SunDisk& K, uint32_t frameIndex, uint8_t* classes, uint8_t* centre, bool unoccluded) {
  const uint32_t W = c.W, H = c.H; const size_t pix = (size_t)py * W + px;
  const FrameConstants& fc = c.fc;
  uint32_t visibility = c.vis[pix];
  if (classes) classes[pix] = 0;
  if (centre) centre[pix] = 0;
  if (visibility == 0) return 0;
  float2 screenPos = {((float)px + 0.5f) / (float)W * 2.0f - 1.0f, ((float)py + 0.5f) / (float)H * 2.0f - 1.0f};
  screenPos.y = -screenPos.y;
  const float3 eye = f3(fc.rg.EyePt[0], fc.rg.EyePt[1], fc.rg.EyePt[2]);
  --visibility;
  const uint32_t inst = visibility >> 24, prim = visibility & 0xFFFFFFu;
  const Vertex3 v = get_vertices(c, inst, prim);
  const M4 wvp = cb_load4x4(fc.g.WorldViewProjs[inst]);
  float4 p[3];
  for (int k = 0; k < 3; ++k) p[k] = mul_point(v.pos[k], wvp);
  screenPos.x -= fc.rg.ProjBias[0]; screenPos.y -= fc.rg.ProjBias[1];
  const float2 bary = calc_barycentrics(p, screenPos);
  const Attrib a = interp_attrib(v, bary.x, bary.y);
  const float3 color = f3(fc.mat.BaseColors[inst][0], fc.mat.BaseColors[inst][1], fc.mat.BaseColors[inst][2]);
  const float2 rghMtl = get_rough_metal(c, inst, a.UV);
  const float4 P4 = mul_point(a.Pos, cb_load4x3(fc.g.Worlds[inst]));
  const float3 P = f3(P4.x, P4.y, P4.z);
  const float3 N = normalize(mul_dir(a.Nrm, cb_load3x3(inst ? fc.g.WorldIT1 : fc.g.WorldITs0)));
  const float3 V = normalize(eye - P);
  const float NoL = dot(N, L);
  if (NoL <= 0.0f) { if (classes) classes[pix] = 1; if (centre) centre[pix] = 1; return 0; }
  if (centre) centre[pix] = trace_closest(c, P, L, 1e-5f, 10000.0f, inst, prim).valid ? 2 : 3;
  const float3 Ls = sun_disk_direction(K, L, (uint32_t)pix, frameIndex, 0u);
  if (!(dot(N, Ls) > 0.0f)) { if (classes) classes[pix] = 4; return 0; }
  if (!unoccluded && trace_closest(c, P, Ls, 1e-5f, 10000.0f, inst, prim).valid) { if (classes) classes[pix] = 2; return 1; }
  if (classes) classes[pix] = 3;
  const float r = std::fmax(rghMtl.x, 1.0f / 32.0f);
  const float3 Hh = normalize(V + L);
  const float NoH = saturate(dot(N, Hh)), VoH = saturate(dot(V, Hh)), NoV = saturate(dot(N, V));
  const float al = r * r, a2 = al * al;
  const float d = (NoH * a2 - NoH) * NoH + 1.0f;
  const float D = a2 / ((kPI * d) * d);
  const float3 f0 = f3(lerp(0.04f, color.x, rghMtl.y), lerp(0.04f, color.y, rghMtl.y), lerp(0.04f, color.z, rghMtl.y));
  const float3 F = f_schlick(f0, VoH);
  const float vis = vis_smith(r, NoV, NoL);
  const float k = (D * vis) * NoL;
  float rgb[3];
  unpack_r11g11b10f(c.refl[pix], rgb);
  c.refl[pix] = pack_r11g11b10f(rgb[0] + (F.x * k) * E.x, rgb[1] + (F.y * k) * E.y, rgb[2] + (F.z * k) * E.z);
  if (rghMtl.y < 1.0f) {
    const float w = NoL / kPI;
    unpack_r11g11b10f(c.diff[pix], rgb);
    c.diff[pix] = pack_r11g11b10f(rgb[0] + ((color.x * (1.0f - 0.04f)) * w) * E.x, rgb[1] + ((color.y * (1.0f - 0.04f)) * w) * E.y,
                                  rgb[2] + ((color.z * (1.0f - 0.04f)) * w) * E.z);
  }
  return 1;
}

// follow_path_h with the rule: the hit of the level-d ray of the path that writes `image` draws slot 1 + 2 d + image with the frame index
// of its sample; stats: the centre ray is traced as well (counted nowhere) for SS_DIFFERS
static inline float3 follow_path_s(const Ctx& c, float3 o, float3 dir, uint32_t skipInst, uint32_t skipPrim, bool diffuseGroup, float3 preset,
                                   const SampleM& xi, uint32_t D, float3& T, uint32_t& rays, const SunHits& sun, float3& S, bool& any, SunHitCounts& n,
                                   const SunDisk& K, uint32_t pixel, uint32_t frameIndex, uint32_t image, bool stats, SunSoftCounts& sn, bool& changed) {
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
        const float3 Ls = sun_disk_direction(K, sun.L, pixel, frameIndex, 1u + 2u * d + image);
        const bool centreLit = stats && !trace_closest(c, P, sun.L, 1e-5f, 10000.0f, h.inst, h.prim).valid;
        if (!(dot(N, Ls) > 0.0f)) { ++sn.n[d][SS_BELOW]; changed = true; }
        else {
          ++rays;
          const bool lit = !trace_closest(c, P, Ls, 1e-5f, 10000.0f, h.inst, h.prim).valid;
          if (stats && lit != centreLit) { ++sn.n[d][SS_DIFFERS]; changed = true; }
          if (!lit) ++n.n[d][SH_OCCLUDED];
          else {
            ++n.n[d][SH_LIT];
            const float3 term = sun_hit_term(sun, N, V, rm, color, diffuseGroup, NoL);
            S = f3(S.x + T.x * term.x, S.y + T.y * term.y, S.z + T.z * term.z);
            any = true;
          }
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

// raygen_pixel_h, its two walks through follow_path_s
static inline uint32_t raygen_pixel_s(Ctx& c, const TableM& t, uint32_t px, uint32_t py, uint32_t D, uint32_t N, uint32_t M, const SunHits& sun, SunHitCounts& n, uint8_t* lit,
                                      const SunDisk& K, bool stats, SunSoftCounts& sn, uint8_t* changed) {
  const uint32_t W = c.W, H = c.H; const size_t pix = (size_t)py * W + px;
  const FrameConstants& fc = c.fc;
  uint32_t rays = 0;
  Surface s{};
  uint32_t visibility = c.vis[pix];
  float2 screenPos = {((float)px + 0.5f) / (float)W * 2.0f - 1.0f, ((float)py + 0.5f) / (float)H * 2.0f - 1.0f};
  screenPos.y = -screenPos.y;
  const float3 eye = f3(fc.rg.EyePt[0], fc.rg.EyePt[1], fc.rg.EyePt[2]);
  if (lit) lit[pix] = 0;
  if (changed) changed[pix] = 0;
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
  bool anyR = false, anyD = false, chR = false, chD = false;
  for (uint32_t k = 0; k < N; ++k) {
    const uint32_t index = fc.g.FrameIndex * N + k;      // sample k's frame index: the path's, and the one its hits draw the disk with
    const SampleM xi = get_sample_param_m(t, px, py, W, index, M);
    {
      const float3 Hh = half_vector_m(c, s.N, s.V, s.rghMtl.x * s.rghMtl.x, xi);
      const float3 R = reflect(-s.V, Hh);
      const float NoL = dot(s.N, R);
      float3 v = f3(0, 0, 0);
      if (NoL > 0.0f) {
        float3 T = reflection_weight_m(c, s.N, s.V, Hh, NoL, s.rghMtl, s.color);
        const float3 col = follow_path_s(c, s.P, R, s.inst, s.prim, false, s.color * s.rghMtl.y, xi, D, T, rays, sun, sun.sums ? accR : SR, anyR, n, K, (uint32_t)pix, index, 0u, stats, sn, chR);
        v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      }
      accR = f3(accR.x + v.x, accR.y + v.y, accR.z + v.z);
    }
    if (diffuse) {
      const float3 dir = diffuse_direction_m(s.N, xi);
      float3 T = s.color * (1.0f - 0.04f);
      const float3 col = follow_path_s(c, s.P, dir, s.inst, s.prim, true, s.color * s.rghMtl.y, xi, D, T, rays, sun, sun.sums ? accD : SD, anyD, n, K, (uint32_t)pix, index, 1u, stats, sn, chD);
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
  if (changed) changed[pix] = (uint8_t)((chR ? 1 : 0) | (chD ? 2 : 0));
  return rays;
}
static inline SunDisk sun_disk(const float* T, const float* B, float k) { return SunDisk{f3(T[0], T[1], T[2]), f3(B[0], B[1], B[2]), k}; }
}  // namespace orc

// out: Ls (3 floats), u, and s as a float
extern "C" void orc_sun_disk_sample(uint32_t pixel, uint32_t frameIndex, uint32_t j, const float* L, const float* T, const float* B, float k, float* out) {
  using namespace orc;
  float u; uint32_t s;
  const float3 d = sun_disk_direction(sun_disk(T, B, k), f3(L[0], L[1], L[2]), pixel, frameIndex, j, &u, &s);
  out[0] = d.x; out[1] = d.y; out[2] = d.z; out[3] = u; out[4] = (float)s;
}
extern "C" uint64_t orc_sun_soft_apply(void* h, const float* L, const float* E, const float* T, const float* B, float k, uint32_t frameIndex, uint8_t* classes, uint8_t* centre, uint32_t unoccluded) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  const float3 l = f3(L[0], L[1], L[2]), e = f3(E[0], E[1], E[2]);
  const SunDisk K = sun_disk(T, B, k);
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) { uint64_t r = 0; for (uint32_t x = 0; x < c->W; ++x) r += sun_soft_pixel(*c, x, y, l, e, K, frameIndex, classes, centre, unoccluded != 0u); rays += r; });
  c->rayCount += rays.load();
  return rays.load();
}
// flags: bits 0 and 1 as orc_ray_trace_sun_hits has them; bit 2: the statistics (soft's second column, changed), at the price of the centre rays
extern "C" uint64_t orc_ray_trace_sun_soft_hits(void* h, uint32_t depth, uint32_t samples, uint32_t M, const float* L, const float* E, const float* T, const float* B, float k,
                                                uint32_t flags, uint64_t* counts, uint8_t* lit, uint64_t* soft, uint8_t* changed) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  const TableM& t = table_m(M);
  SunHits sun;
  sun.on = (flags & 1u) != 0u; sun.sums = (flags & 2u) != 0u || samples > 1u;
  sun.L = f3(L[0], L[1], L[2]); sun.E = f3(E[0], E[1], E[2]);
  const SunDisk K = sun_disk(T, B, k);
  const bool stats = (flags & 4u) != 0u;
  std::atomic<uint64_t> rays{0};
  std::mutex lock;
  parallel_rows(c->threads, c->H, [&](uint32_t y) {
    uint64_t r = 0; SunHitCounts n; SunSoftCounts sn;
    for (uint32_t x = 0; x < c->W; ++x) r += raygen_pixel_s(*c, t, x, y, depth, samples, M, sun, n, lit, K, stats, sn, changed);
    rays += r;
    std::lock_guard<std::mutex> g(lock);
    if (counts) for (int d = 0; d < 4; ++d) for (int k2 = 0; k2 < SH_COLUMNS; ++k2) counts[d * SH_COLUMNS + k2] += n.n[d][k2];
    if (soft) for (int d = 0; d < 4; ++d) for (int k2 = 0; k2 < 2; ++k2) soft[d * 2 + k2] += sn.n[d][k2];
  });
  c->rayCount = rays.load();
  return c->rayCount;
}
