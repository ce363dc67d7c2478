// TEST INFRASTRUCTURE ONLY.  CPU restatement of the local lights at the surfaces the paths hit (rtggx_set_light_reflections; include/rtggx.h
// has the rule): tests/lights_ref.cpp -- the whole oracle, every restatement, the three sun passes and the lights' primary pass -- plus
// orc_ray_trace_light_hits: sun_soft_ref.cpp's path walker (the one that carries the sun's hit terms and the disk) once more, with the
// lights' rule behind the sun's at every touched hit.  A sun without a size is the disk with k = 0, where Ls = L exactly.
// flags bit 0: the sun's toggle (rtggx_set_sun_reflections under a sun); bit 1: the terms go into the fp32 sums even at N = 1 (a block of a
// sample map that gets one sample of an N-sample frame); bit 3: this feature's toggle.  With bits 0 and 3 clear the walker is
// raygen_pixel_m's, line by line.
// counts, lit: sun_hit_ref.cpp's (lit: a term of EITHER feature exists in RayTracingOut0 / 1).  lcounts (may be null): [4 levels][8 lights]
// [LH_COLUMNS] -- per level and light the touched hits out of range, facing away, outside the cone, below the horizon, occluded and lit,
// then the lit ones by lobe -- ADDED to what the array holds.  llit (may be null): per pixel bit 0 / 1, a LIGHT's term exists in
// RayTracingOut0 / 1.  lcls0 (may be null): [8 lights][2 images][H][W], the class (LC_* of lights_ref.cpp, 0: no touched hit) of the level-0
// hit of the pixel's last sample under each light.  The return value counts every ray; *hitRays (may be null) gets the shadow rays from hits
// under the lights.  The primary passes are the caller's to run afterwards.  Every operation is fp32, rounded on its own (-ffp-contract=off).
#include "lights_ref.cpp"

namespace orc {
enum { LH_RANGE = 0, LH_AWAY, LH_CONE, LH_BELOW, LH_OCCLUDED, LH_LIT, LH_LIT_SPECULAR, LH_LIT_DIFFUSE, LH_COLUMNS };
struct LightHits { bool on; const Light* l; uint32_t count; };
struct LightHitCounts { uint64_t n[4][8][LH_COLUMNS] = {}; uint64_t rays = 0; };

// step 2 of the rule: the point of the unit sphere the hit of slot j draws
static inline float3 light_hit_sphere_point(uint32_t pixel, uint32_t frameIndex, uint32_t j, uint32_t* wOut = nullptr, float* uOut = nullptr, uint32_t* sOut = nullptr) {
  const TableM& t = table_m(256);      // always the 256-entry table, whatever the sample set
  uint32_t h = rng(pixel); h += frameIndex; h = rng(h);
  const uint32_t w = rng(h + j * 0x9E3779B9u);
  const float u = (float)(w & 0xffffu) / 65536.0f;
  const uint32_t s = w >> 24;
  const float z = 1.0f - 2.0f * u;
  const float rho = std::sqrt(1.0f - z * z);
  if (wOut) *wOut = w;
  if (uOut) *uOut = u;
  if (sOut) *sOut = s;
  return f3(rho * t.cosTab[s], rho * t.sinTab[s], z);
}

// steps 1-5 of the rule for one light at one touched hit: the class, and where lit the term added to S
static inline uint8_t light_hit(const Ctx& c, const Light& l, uint32_t i, float3 P, float3 N, float3 V, float2 rm, float3 color, bool diffuseGroup, uint32_t hInst, uint32_t hPrim,
                                float3 T, uint32_t pixel, uint32_t frameIndex, uint32_t d, uint32_t image, float3& S, uint32_t& rays, uint64_t& hitRays) {
  // 1
  const float3 D = f3(l.P.x - P.x, l.P.y - P.y, l.P.z - P.z);
  const float d2 = dot(D, D), RR = l.R * l.R;
  if (d2 < 1e-6f || d2 >= RR) return LC_RANGE;
  const float3 L = normalize(D);
  const float NoL = dot(N, L);
  if (NoL <= 0.0f) return LC_AWAY;
  float spot = 1.0f;
  if (l.cosOuter > -1.0f) {
    const float cc = -dot(L, l.A);
    if (cc <= l.cosOuter) return LC_CONE;
    const float s = saturate((cc - l.cosOuter) / (l.cosInner - l.cosOuter));
    spot = s * s;
  }
  const float q = d2 / RR;
  float win = saturate(1.0f - q * q); win = win * win;
  const float m2 = std::fmax(l.rho * l.rho, 1e-4f);
  const float att = (win * spot) / std::fmax(d2, m2);
  // 2
  float3 Ds = D;
  if (l.rho > 0.0f) {
    const float3 o = light_hit_sphere_point(pixel, frameIndex, 32u + 16u * d + 8u * image + i);
    Ds = f3(D.x + l.rho * o.x, D.y + l.rho * o.y, D.z + l.rho * o.z);
  }
  const float ds2 = dot(Ds, Ds);
  if (ds2 < 1e-6f) return LC_RANGE;      // (the target in the surface: counted with "out of range", as in lights_ref.cpp)
  const float3 Ls = normalize(Ds);
  const float tmax = std::sqrt(ds2);
  // 3
  if (!(dot(N, Ls) > 0.0f)) return LC_BELOW;
  ++rays; ++hitRays;
  if (trace_closest(c, P, Ls, 1e-5f, tmax, hInst, hPrim).valid) return LC_OCCLUDED;
  // 4
  float3 term;
  if (rm.y > 0.5f) {
    const float r = std::fmax(rm.x, 1.0f / 32.0f);
    const float3 Hh = normalize(V + L);
    const float NoH = saturate(dot(N, Hh)), VoH = saturate(dot(V, Hh)), NoV = saturate(dot(N, V));
    const float al = r * r, a2 = al * al;
    const float dd = (NoH * a2 - NoH) * NoH + 1.0f;
    const float Dg = a2 / ((kPI * dd) * dd);
    const float3 f0 = f3(lerp(0.04f, color.x, rm.y), lerp(0.04f, color.y, rm.y), lerp(0.04f, color.z, rm.y));
    const float3 F = f_schlick(f0, VoH);
    const float vis = vis_smith(r, NoV, NoL);
    const float k = (Dg * vis) * NoL;
    term = f3((F.x * k) * (l.I.x * att), (F.y * k) * (l.I.y * att), (F.z * k) * (l.I.z * att));
  } else {
    if (diffuseGroup) color = color * (1.0f - rm.y);
    const float g = (NoL / kPI) * att;
    term = f3((color.x * g) * l.I.x, (color.y * g) * l.I.y, (color.z * g) * l.I.z);
  }
  // 5
  S = f3(S.x + T.x * term.x, S.y + T.y * term.y, S.z + T.z * term.z);
  return LC_LIT;
}

// follow_path_s with the rule: at every touched hit the sun's term first, then the lights' for i ascending
static inline float3 follow_path_l(const Ctx& c, float3 o, float3 dir, uint32_t skipInst, uint32_t skipPrim, bool diffuseGroup, float3 preset,
                                   const SampleM& xi, uint32_t D, float3& T, uint32_t& rays, const SunHits& sun, float3& S, bool& any, SunHitCounts& n,
                                   const SunDisk& K, uint32_t pixel, uint32_t frameIndex, uint32_t image, bool stats, SunSoftCounts& sn, bool& changed,
                                   const LightHits& lh, LightHitCounts& ln, bool& anyLight, uint8_t* cls0) {
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
    if (lh.on) {
      for (uint32_t i = 0; i < lh.count; ++i) {
        const Light& l = lh.l[i];
        if (!(l.I.x > 0.0f || l.I.y > 0.0f || l.I.z > 0.0f)) continue;
        const uint8_t cls = light_hit(c, l, i, P, N, V, rm, color, diffuseGroup, h.inst, h.prim, T, pixel, frameIndex, d, image, S, rays, ln.rays);
        ++ln.n[d][i][cls - LC_RANGE];
        if (cls == LC_LIT) { ++ln.n[d][i][rm.y > 0.5f ? LH_LIT_SPECULAR : LH_LIT_DIFFUSE]; any = true; anyLight = true; }
        if (d == 0 && cls0) cls0[i] = cls;
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

// raygen_pixel_s, its two walks through follow_path_l
static inline uint32_t raygen_pixel_l(Ctx& c, const TableM& t, uint32_t px, uint32_t py, uint32_t D, uint32_t N, uint32_t M, const SunHits& sun, SunHitCounts& n, uint8_t* lit,
                                      const SunDisk& K, bool stats, SunSoftCounts& sn, uint8_t* changed, const LightHits& lh, LightHitCounts& ln, uint8_t* llit, uint8_t* lcls0) {
  const uint32_t W = c.W, H = c.H; const size_t pix = (size_t)py * W + px, frame = (size_t)W * H;
  const FrameConstants& fc = c.fc;
  uint32_t rays = 0;
  Surface s{};
  uint32_t visibility = c.vis[pix];
  float2 screenPos = {((float)px + 0.5f) / (float)W * 2.0f - 1.0f, ((float)py + 0.5f) / (float)H * 2.0f - 1.0f};
  screenPos.y = -screenPos.y;
  const float3 eye = f3(fc.rg.EyePt[0], fc.rg.EyePt[1], fc.rg.EyePt[2]);
  if (lit) lit[pix] = 0;
  if (changed) changed[pix] = 0;
  if (llit) llit[pix] = 0;
  if (lcls0) for (uint32_t i = 0; i < 16u; ++i) lcls0[i * frame + pix] = 0;
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
  bool anyR = false, anyD = false, chR = false, chD = false, lightR = false, lightD = false;
  uint8_t cls[2][8];
  for (uint32_t k = 0; k < N; ++k) {
    const uint32_t index = fc.g.FrameIndex * N + k;      // sample k's frame index: the path's, and the one its hits draw the disk and the spheres with
    const SampleM xi = get_sample_param_m(t, px, py, W, index, M);
    for (int i = 0; i < 8; ++i) cls[0][i] = cls[1][i] = 0;
    {
      const float3 Hh = half_vector_m(c, s.N, s.V, s.rghMtl.x * s.rghMtl.x, xi);
      const float3 R = reflect(-s.V, Hh);
      const float NoL = dot(s.N, R);
      float3 v = f3(0, 0, 0);
      if (NoL > 0.0f) {
        float3 T = reflection_weight_m(c, s.N, s.V, Hh, NoL, s.rghMtl, s.color);
        const float3 col = follow_path_l(c, s.P, R, s.inst, s.prim, false, s.color * s.rghMtl.y, xi, D, T, rays, sun, sun.sums ? accR : SR, anyR, n, K, (uint32_t)pix, index, 0u, stats, sn, chR,
                                         lh, ln, lightR, cls[0]);
        v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      }
      accR = f3(accR.x + v.x, accR.y + v.y, accR.z + v.z);
    }
    if (diffuse) {
      const float3 dir = diffuse_direction_m(s.N, xi);
      float3 T = s.color * (1.0f - 0.04f);
      const float3 col = follow_path_l(c, s.P, dir, s.inst, s.prim, true, s.color * s.rghMtl.y, xi, D, T, rays, sun, sun.sums ? accD : SD, anyD, n, K, (uint32_t)pix, index, 1u, stats, sn, chD,
                                       lh, ln, lightD, cls[1]);
      const float3 v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      accD = f3(accD.x + v.x, accD.y + v.y, accD.z + v.z);
    }
  }
  const float scale = 1.0f / (float)N;
  c.refl[pix] = pack_r11g11b10f(accR.x * scale, accR.y * scale, accR.z * scale);
  if (diffuse) c.diff[pix] = pack_r11g11b10f(accD.x * scale, accD.y * scale, accD.z * scale);
  if (!sun.sums) {      // one sample: the packed add, where a term of either feature exists -- one rounding
    float rgb[3];
    if (anyR) { unpack_r11g11b10f(c.refl[pix], rgb); c.refl[pix] = pack_r11g11b10f(rgb[0] + SR.x, rgb[1] + SR.y, rgb[2] + SR.z); }
    if (anyD) { unpack_r11g11b10f(c.diff[pix], rgb); c.diff[pix] = pack_r11g11b10f(rgb[0] + SD.x, rgb[1] + SD.y, rgb[2] + SD.z); }
  }
  if (lit) lit[pix] = (uint8_t)((anyR ? 1 : 0) | (anyD ? 2 : 0));
  if (changed) changed[pix] = (uint8_t)((chR ? 1 : 0) | (chD ? 2 : 0));
  if (llit) llit[pix] = (uint8_t)((lightR ? 1 : 0) | (lightD ? 2 : 0));
  if (lcls0) for (uint32_t i = 0; i < 8u; ++i) { lcls0[(i * 2u) * frame + pix] = cls[0][i]; lcls0[(i * 2u + 1u) * frame + pix] = cls[1][i]; }
  return rays;
}
}  // namespace orc

extern "C" uint32_t orc_light_hit_columns() { return orc::LH_COLUMNS; }
// out: w, u's bits as k = u 65536, s -- of the slot j = 32 + 16 d + 8 img + i
extern "C" void orc_light_hit_sample(uint32_t pixel, uint32_t frameIndex, uint32_t d, uint32_t image, uint32_t i, uint32_t* out) {
  uint32_t w, s; float u;
  orc::light_hit_sphere_point(pixel, frameIndex, 32u + 16u * d + 8u * image + i, &w, &u, &s);
  out[0] = w; out[1] = (uint32_t)(u * 65536.0f); out[2] = s;
}
extern "C" uint64_t orc_ray_trace_light_hits(void* h, uint32_t depth, uint32_t samples, uint32_t M, const float* L, const float* E, const float* T, const float* B, float k,
                                             uint32_t flags, uint64_t* counts, uint8_t* lit, uint64_t* soft, uint8_t* changed,
                                             const float* lights, uint32_t count, uint64_t* lcounts, uint8_t* llit, uint8_t* lcls0, uint64_t* hitRays) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  if (count > 8u) return ~0ull;
  const TableM& t = table_m(M);
  SunHits sun;
  sun.on = (flags & 1u) != 0u; sun.sums = (flags & 2u) != 0u || samples > 1u;
  sun.L = f3(L[0], L[1], L[2]); sun.E = f3(E[0], E[1], E[2]);
  const SunDisk K = sun_disk(T, B, k);
  const bool stats = (flags & 4u) != 0u;
  Light ls[8];
  for (uint32_t i = 0; i < count; ++i) {
    const float* f = lights + 16u * i;
    ls[i] = Light{f3(f[0], f[1], f[2]), f[3], f3(f[4], f[5], f[6]), f[7], f3(f[8], f[9], f[10]), f[11], f[12]};
  }
  const LightHits lh{(flags & 8u) != 0u && count > 0u, ls, count};
  std::atomic<uint64_t> rays{0};
  std::mutex lock;
  uint64_t shadow = 0;
  parallel_rows(c->threads, c->H, [&](uint32_t y) {
    uint64_t r = 0; SunHitCounts n; SunSoftCounts sn; LightHitCounts ln;
    for (uint32_t x = 0; x < c->W; ++x) r += raygen_pixel_l(*c, t, x, y, depth, samples, M, sun, n, lit, K, stats, sn, changed, lh, ln, llit, lcls0);
    rays += r;
    std::lock_guard<std::mutex> g(lock);
    shadow += ln.rays;
    if (counts) for (int d = 0; d < 4; ++d) for (int k2 = 0; k2 < SH_COLUMNS; ++k2) counts[d * SH_COLUMNS + k2] += n.n[d][k2];
    if (soft) for (int d = 0; d < 4; ++d) for (int k2 = 0; k2 < 2; ++k2) soft[d * 2 + k2] += sn.n[d][k2];
    if (lcounts) for (int d = 0; d < 4; ++d) for (int i = 0; i < 8; ++i) for (int k2 = 0; k2 < LH_COLUMNS; ++k2) lcounts[(d * 8 + i) * LH_COLUMNS + k2] += ln.n[d][i][k2];
  });
  if (hitRays) *hitRays = shadow;
  c->rayCount = rays.load();
  return c->rayCount;
}
