// TEST INFRASTRUCTURE ONLY.  CPU restatement of a light list beyond eight (rtggx_set_light_list; include/rtggx.h has the rule):
// tests/light_pick_ref.cpp -- the whole oracle and every restatement below it, mode 1's steps among them -- plus the same rule over ALL n
// lights of a list, WITHOUT a cull, in scalar C++ with the list's hash slots:
//   orc_light_list_apply        the primary pass on the oracle's RayTracingOut0/1 as they are (orc_light_pick_apply's place); with flags
//                               bit 1 instead the sum of every candidate's term behind a ray of its own (radius 0: no hash), images untouched
//   orc_ray_trace_light_list    light_pick_ref.cpp's path walker once more, the pick over the list at every touched hit
//   orc_light_list_cull         the cull restated apart from the rule: per 8x8 block the box of the covered pixels' P, the kept lights, the
//                               lights that are a candidate at some pixel of the block -- and how often "in range at a pixel => kept" fails
//   orc_light_list_slot, orc_light_list_hit_slot      the hash slot of a light's target
// Per pixel the primary pass records (all may be null) info [H][W][4] uint16: the number of candidates, the chosen index (0xFFFF: none),
// the class of the chosen ray (LC_* of lights_ref.cpp; LC_RANGE: the target in the surface; 0: no candidate), flags (bit 0: the "none, so
// the last candidate" branch was needed, bit 1: the chosen light is not the first candidate); wf [H][W][2] floats: W and f; terms [H][W][6]
// floats: S0 and S1 as added (0 where no term); P [H][W][3] floats: the surface point (covered pixels); reach and cand [H][W][ceil(n / 8)]
// bytes: bit k of a pixel, light k casts rays and has d2 < R R there / is a candidate there.  flags bit 0 of the call: every ray that exists
// counts as unoccluded.  The hit pass records pcounts [4 levels][LL_COLUMNS], ADDED to what the array holds, and pchosen0 [2 images][H][W]
// int16: the light chosen at the level-0 hit of the pixel's last sample (-1: none).
// Every operation is fp32, rounded on its own (-ffp-contract=off).
#include "light_pick_ref.cpp"

#include <vector>

namespace orc {
enum { LL_CAND1 = 0, LL_CAND2, LL_RANGE, LL_BELOW, LL_OCCLUDED, LL_LIT, LL_CHOSEN8, LL_CHOSEN64, LL_COLUMNS };
struct LightListCounts { uint64_t n[4][LL_COLUMNS] = {}; };
struct LightListHits { bool on; const Light* l; uint32_t count; };

static inline uint32_t list_slot(uint32_t i) { return i < 8u ? 16u + i : 4096u + i; }
static inline uint32_t list_hit_slot(uint32_t d, uint32_t image, uint32_t i) { return i < 8u ? 32u + 16u * d + 8u * image + i : 8192u + 1024u * (2u * d + image) + i; }
static inline bool casts(const Light& l) { return l.I.x > 0.0f || l.I.y > 0.0f || l.I.z > 0.0f; }

// one candidate of a point: its index, weight, and what the term needs
struct ListCand { uint32_t i; float w; float3 a, b, D; };      // a: spec (primary) or s (hits); b: diff (primary)
// steps 2-5 over the candidates, in the order they were found (ascending): W, the chosen candidate's position, f
static inline size_t list_choose(const std::vector<ListCand>& cs, uint32_t word, float& Wsum, float& f, bool& fallback) {
  Wsum = 0.0f;
  for (const ListCand& c : cs) Wsum = Wsum + c.w;
  const float t = pick_x(word) * Wsum;
  float c = 0.0f;
  size_t chosen = cs.size();
  for (size_t k = 0; k < cs.size(); ++k) {
    c = c + cs[k].w;
    if (t < c) { chosen = k; break; }
  }
  fallback = chosen == cs.size();
  if (fallback) chosen = cs.size() - 1;
  f = Wsum / cs[chosen].w;
  return chosen;
}

struct ListRecord { uint16_t* info; float* wf; float* terms; float* P; uint8_t* reach; uint8_t* cand; };

static inline uint32_t list_pixel(Ctx& c, uint32_t px, uint32_t py, const std::vector<Light>& lights, uint32_t frameIndex, bool unoccluded, bool sumAll, const ListRecord& rec,
                                  std::vector<ListCand>& cs) {
  const uint32_t W_ = c.W; const size_t pix = (size_t)py * W_ + px;
  const size_t bytes = (lights.size() + 7u) / 8u;
  const FrameConstants& fc = c.fc;
  uint32_t visibility = c.vis[pix];
  if (rec.info) { rec.info[pix * 4] = 0; rec.info[pix * 4 + 1] = 0xFFFF; rec.info[pix * 4 + 2] = 0; rec.info[pix * 4 + 3] = 0; }
  if (rec.wf) rec.wf[pix * 2] = rec.wf[pix * 2 + 1] = 0.0f;
  if (rec.terms) for (int k = 0; k < 6; ++k) rec.terms[pix * 6 + k] = 0.0f;
  if (rec.P) for (int k = 0; k < 3; ++k) rec.P[pix * 3 + k] = 0.0f;
  if (rec.reach) for (size_t k = 0; k < bytes; ++k) rec.reach[pix * bytes + k] = 0;
  if (rec.cand) for (size_t k = 0; k < bytes; ++k) rec.cand[pix * bytes + k] = 0;
  if (visibility == 0) return 0;
  // step 0: lights_pixel's surface
  float2 screenPos = {((float)px + 0.5f) / (float)W_ * 2.0f - 1.0f, ((float)py + 0.5f) / (float)c.H * 2.0f - 1.0f};
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
  const bool diffuse = rghMtl.y < 1.0f;
  if (rec.P) { rec.P[pix * 3] = P.x; rec.P[pix * 3 + 1] = P.y; rec.P[pix * 3 + 2] = P.z; }
  // step 1: the candidates, over ALL lights
  cs.clear();
  for (uint32_t i = 0; i < lights.size(); ++i) {
    const Light& l = lights[i];
    if (!casts(l)) continue;
    if (rec.reach) {
      const float3 D = f3(l.P.x - P.x, l.P.y - P.y, l.P.z - P.z);
      if (dot(D, D) < l.R * l.R) rec.reach[pix * bytes + (i >> 3)] |= (uint8_t)(1u << (i & 7u));
    }
    const LightReach r = light_reach(l, P, N);
    if (!r.reach) continue;
    const float3 Fk = light_Fk(N, V, r.L, r.NoL, color, rghMtl);
    ListCand k{};
    k.i = i; k.D = r.D;
    k.a = f3(Fk.x * (l.I.x * r.att), Fk.y * (l.I.y * r.att), Fk.z * (l.I.z * r.att));
    float wi = pick_luminance(k.a);
    k.b = f3(0, 0, 0);
    if (diffuse) {
      const float g = (r.NoL / kPI) * r.att;
      k.b = f3(((color.x * (1.0f - 0.04f)) * g) * l.I.x, ((color.y * (1.0f - 0.04f)) * g) * l.I.y, ((color.z * (1.0f - 0.04f)) * g) * l.I.z);
      wi = wi + pick_luminance(k.b);
    }
    if (!(wi > 0.0f)) continue;      // (a NaN is not a candidate)
    k.w = wi;
    cs.push_back(k);
    if (rec.cand) rec.cand[pix * bytes + (i >> 3)] |= (uint8_t)(1u << (i & 7u));
  }
  if (rec.info) rec.info[pix * 4] = (uint16_t)cs.size();
  if (cs.empty()) return 0;
  if (sumAll) {      // every candidate behind a ray of its own, the terms added in index order: what the pick estimates (radius 0 only)
    uint32_t rays = 0;
    float3 S0 = f3(0, 0, 0), S1 = f3(0, 0, 0);
    for (const ListCand& k : cs) {
      float3 Ls; float tmax = 0.0f;
      if (light_target(lights[k.i], k.D, N, (uint32_t)pix, frameIndex, list_slot(k.i), Ls, tmax)) continue;
      ++rays;
      if (trace_closest(c, P, Ls, 1e-5f, tmax, inst, prim).valid) continue;
      S0 = f3(S0.x + k.a.x, S0.y + k.a.y, S0.z + k.a.z);
      if (diffuse) S1 = f3(S1.x + k.b.x, S1.y + k.b.y, S1.z + k.b.z);
    }
    if (rec.terms) { rec.terms[pix * 6] = S0.x; rec.terms[pix * 6 + 1] = S0.y; rec.terms[pix * 6 + 2] = S0.z; rec.terms[pix * 6 + 3] = S1.x; rec.terms[pix * 6 + 4] = S1.y; rec.terms[pix * 6 + 5] = S1.z; }
    return rays;
  }
  // steps 2-5
  float Wsum, f; bool fallback;
  const size_t at = list_choose(cs, pick_word((uint32_t)pix, frameIndex, 96u), Wsum, f, fallback);
  const ListCand& ch = cs[at];
  if (rec.info) { rec.info[pix * 4 + 1] = (uint16_t)ch.i; rec.info[pix * 4 + 3] = (uint16_t)((fallback ? 1 : 0) | (at != 0 ? 2 : 0)); }
  if (rec.wf) { rec.wf[pix * 2] = Wsum; rec.wf[pix * 2 + 1] = f; }
  // step 6
  float3 Ls; float tmax = 0.0f;
  uint8_t cls = light_target(lights[ch.i], ch.D, N, (uint32_t)pix, frameIndex, list_slot(ch.i), Ls, tmax);
  if (cls) { if (rec.info) rec.info[pix * 4 + 2] = cls; return 0; }
  cls = !unoccluded && trace_closest(c, P, Ls, 1e-5f, tmax, inst, prim).valid ? LC_OCCLUDED : LC_LIT;
  if (rec.info) rec.info[pix * 4 + 2] = cls;
  if (cls == LC_OCCLUDED) return 1;
  // step 7
  const float3 S0 = f3(0.0f + ch.a.x * f, 0.0f + ch.a.y * f, 0.0f + ch.a.z * f);
  float rgb[3];
  unpack_r11g11b10f(c.refl[pix], rgb);
  c.refl[pix] = pack_r11g11b10f(rgb[0] + S0.x, rgb[1] + S0.y, rgb[2] + S0.z);
  if (rec.terms) { rec.terms[pix * 6] = S0.x; rec.terms[pix * 6 + 1] = S0.y; rec.terms[pix * 6 + 2] = S0.z; }
  if (diffuse) {
    const float3 S1 = f3(0.0f + ch.b.x * f, 0.0f + ch.b.y * f, 0.0f + ch.b.z * f);
    unpack_r11g11b10f(c.diff[pix], rgb);
    c.diff[pix] = pack_r11g11b10f(rgb[0] + S1.x, rgb[1] + S1.y, rgb[2] + S1.z);
    if (rec.terms) { rec.terms[pix * 6 + 3] = S1.x; rec.terms[pix * 6 + 4] = S1.y; rec.terms[pix * 6 + 5] = S1.z; }
  }
  return 1;
}

// the hits' rule at one touched hit: the chosen light (-1: no candidate) and, where lit, s_i f added to S
static inline int list_hit(const Ctx& c, const LightListHits& lh, float3 P, float3 N, float3 V, float2 rm, float3 color, bool diffuseGroup, uint32_t hInst, uint32_t hPrim,
                           float3 T, uint32_t pixel, uint32_t frameIndex, uint32_t d, uint32_t image, float3& S, uint32_t& rays, uint64_t& hitRays, uint64_t* pc, bool& lit,
                           std::vector<ListCand>& cs) {
  cs.clear();
  lit = false;
  for (uint32_t i = 0; i < lh.count; ++i) {
    const Light& l = lh.l[i];
    if (!casts(l)) continue;
    const LightReach r = light_reach(l, P, N);
    if (!r.reach) continue;
    const float3 term = light_hit_term(l, r, N, V, rm, color, diffuseGroup);
    ListCand k{};
    k.i = i; k.D = r.D;
    k.a = f3(T.x * term.x, T.y * term.y, T.z * term.z);
    k.w = pick_luminance(k.a);
    if (!(k.w > 0.0f)) continue;
    cs.push_back(k);
  }
  if (cs.empty()) return -1;
  ++pc[LL_CAND1];
  if (cs.size() >= 2) ++pc[LL_CAND2];
  float Wsum, f; bool fallback;
  const size_t at = list_choose(cs, pick_word(pixel, frameIndex, 104u + 2u * d + image), Wsum, f, fallback);
  const ListCand& ch = cs[at];
  if (cs.size() >= 2 && ch.i >= 8u) ++pc[LL_CHOSEN8];
  if (ch.i >= 64u) ++pc[LL_CHOSEN64];
  float3 Ls; float tmax = 0.0f;
  const uint8_t cls = light_target(lh.l[ch.i], ch.D, N, pixel, frameIndex, list_hit_slot(d, image, ch.i), Ls, tmax);
  if (cls) { ++pc[cls == LC_RANGE ? LL_RANGE : LL_BELOW]; return (int)ch.i; }
  ++rays; ++hitRays;
  if (trace_closest(c, P, Ls, 1e-5f, tmax, hInst, hPrim).valid) { ++pc[LL_OCCLUDED]; return (int)ch.i; }
  ++pc[LL_LIT];
  S = f3(S.x + ch.a.x * f, S.y + ch.a.y * f, S.z + ch.a.z * f);
  lit = true;
  return (int)ch.i;
}

// follow_path_p with the list's pick in place of its lights
static inline float3 follow_path_ll(const Ctx& c, float3 o, float3 dir, uint32_t skipInst, uint32_t skipPrim, bool diffuseGroup, float3 preset,
                                    const SampleM& xi, uint32_t D, float3& T, uint32_t& rays, const SunHits& sun, float3& S, bool& any, SunHitCounts& n,
                                    const SunDisk& K, uint32_t pixel, uint32_t frameIndex, uint32_t image, SunSoftCounts& sn,
                                    const LightListHits& lh, uint64_t& hitRays, LightListCounts& pn, int16_t& chosen0, std::vector<ListCand>& cs) {
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
        if (!(dot(N, Ls) > 0.0f)) ++sn.n[d][SS_BELOW];
        else {
          ++rays;
          const bool lit = !trace_closest(c, P, Ls, 1e-5f, 10000.0f, h.inst, h.prim).valid;
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
      bool lit;
      const int ch = list_hit(c, lh, P, N, V, rm, color, diffuseGroup, h.inst, h.prim, T, pixel, frameIndex, d, image, S, rays, hitRays, pn.n[d], lit, cs);
      if (lit) any = true;
      if (d == 0) chosen0 = (int16_t)ch;
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

// raygen_pixel_p, its two walks through follow_path_ll
static inline uint32_t raygen_pixel_ll(Ctx& c, const TableM& t, uint32_t px, uint32_t py, uint32_t D, uint32_t N, uint32_t M, const SunHits& sun, SunHitCounts& n,
                                       const SunDisk& K, SunSoftCounts& sn, const LightListHits& lh, uint64_t& hitRays, LightListCounts& pn, int16_t* pchosen0,
                                       std::vector<ListCand>& cs) {
  const uint32_t W = c.W, H = c.H; const size_t pix = (size_t)py * W + px, frame = (size_t)W * H;
  const FrameConstants& fc = c.fc;
  uint32_t rays = 0;
  Surface s{};
  uint32_t visibility = c.vis[pix];
  float2 screenPos = {((float)px + 0.5f) / (float)W * 2.0f - 1.0f, ((float)py + 0.5f) / (float)H * 2.0f - 1.0f};
  screenPos.y = -screenPos.y;
  const float3 eye = f3(fc.rg.EyePt[0], fc.rg.EyePt[1], fc.rg.EyePt[2]);
  if (pchosen0) pchosen0[pix] = pchosen0[frame + pix] = -1;
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
  int16_t chosen[2] = {-1, -1};
  for (uint32_t k = 0; k < N; ++k) {
    const uint32_t index = fc.g.FrameIndex * N + k;      // sample k's frame index: the path's, and the one its hits draw with
    const SampleM xi = get_sample_param_m(t, px, py, W, index, M);
    chosen[0] = chosen[1] = -1;
    {
      const float3 Hh = half_vector_m(c, s.N, s.V, s.rghMtl.x * s.rghMtl.x, xi);
      const float3 R = reflect(-s.V, Hh);
      const float NoL = dot(s.N, R);
      float3 v = f3(0, 0, 0);
      if (NoL > 0.0f) {
        float3 T = reflection_weight_m(c, s.N, s.V, Hh, NoL, s.rghMtl, s.color);
        const float3 col = follow_path_ll(c, s.P, R, s.inst, s.prim, false, s.color * s.rghMtl.y, xi, D, T, rays, sun, sun.sums ? accR : SR, anyR, n, K, (uint32_t)pix, index, 0u, sn,
                                          lh, hitRays, pn, chosen[0], cs);
        v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      }
      accR = f3(accR.x + v.x, accR.y + v.y, accR.z + v.z);
    }
    if (diffuse) {
      const float3 dir = diffuse_direction_m(s.N, xi);
      float3 T = s.color * (1.0f - 0.04f);
      const float3 col = follow_path_ll(c, s.P, dir, s.inst, s.prim, true, s.color * s.rghMtl.y, xi, D, T, rays, sun, sun.sums ? accD : SD, anyD, n, K, (uint32_t)pix, index, 1u, sn,
                                        lh, hitRays, pn, chosen[1], cs);
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
  if (pchosen0) { pchosen0[pix] = chosen[0]; pchosen0[frame + pix] = chosen[1]; }
  return rays;
}

static inline std::vector<Light> read_light_list(const float* lights, uint32_t count) {
  std::vector<Light> ls(count);
  if (count) read_lights(lights, count, ls.data());
  return ls;
}
}  // namespace orc

extern "C" uint32_t orc_light_list_columns() { return orc::LL_COLUMNS; }
extern "C" uint32_t orc_light_list_slot(uint32_t i) { return orc::list_slot(i); }
extern "C" uint32_t orc_light_list_hit_slot(uint32_t d, uint32_t image, uint32_t i) { return orc::list_hit_slot(d, image, i); }
extern "C" uint64_t orc_light_list_apply(void* h, const float* lights, uint32_t count, uint32_t frameIndex, uint32_t flags, uint16_t* info, float* wf, float* terms,
                                         float* P, uint8_t* reach, uint8_t* cand) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  if (count > 1024u) return ~0ull;
  const std::vector<Light> ls = read_light_list(lights, count);
  const ListRecord rec{info, wf, terms, P, reach, cand};
  const bool sumAll = (flags & 2u) != 0u;
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) {
    uint64_t r = 0; std::vector<ListCand> cs;
    for (uint32_t x = 0; x < c->W; ++x) r += list_pixel(*c, x, y, ls, frameIndex, (flags & 1u) != 0u, sumAll, rec, cs);
    rays += r;
  });
  if (!sumAll) c->rayCount += rays.load();
  return rays.load();
}
// The cull, from what the rule's pass recorded: P [H][W][3], reach and cand [H][W][ceil(n / 8)].  Per 8x8 block, row-major, over its covered
// pixels: kept = the lights with dist2 < RRm (0 without a covered pixel), cands = the lights that are a candidate at some pixel of the
// block.  Returns the number of (block, light) pairs with the light in range at a pixel of the block and NOT kept: the implication the
// cull's invisibility rests on says 0.
extern "C" uint64_t orc_light_list_cull(void* h, const float* lights, uint32_t count, const float* P, const uint8_t* reach, const uint8_t* cand, uint32_t* kept, uint32_t* cands) {
  using namespace orc;
  const Ctx* c = (const Ctx*)h;
  if (count > 1024u) return ~0ull;
  const std::vector<Light> ls = read_light_list(lights, count);
  const uint32_t W = c->W, H = c->H, bx = (W + 7u) / 8u, by = (H + 7u) / 8u;
  const size_t bytes = (count + 7u) / 8u;
  uint64_t violations = 0;
  std::vector<uint8_t> anyReach(bytes), anyCand(bytes);
  for (uint32_t b = 0; b < bx * by; ++b) {
    const uint32_t x0 = (b % bx) * 8u, y0 = (b / bx) * 8u;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::fill(anyReach.begin(), anyReach.end(), 0); std::fill(anyCand.begin(), anyCand.end(), 0);
    bool covered = false;
    for (uint32_t y = y0; y < y0 + 8u && y < H; ++y) for (uint32_t x = x0; x < x0 + 8u && x < W; ++x) {
      const size_t pix = (size_t)y * W + x;
      if (c->vis[pix] == 0) continue;
      covered = true;
      for (int k = 0; k < 3; ++k) { lo[k] = std::fmin(lo[k], P[pix * 3 + k]); hi[k] = std::fmax(hi[k], P[pix * 3 + k]); }
      for (size_t k = 0; k < bytes; ++k) { anyReach[k] |= reach[pix * bytes + k]; anyCand[k] |= cand[pix * bytes + k]; }
    }
    uint32_t nKept = 0, nCand = 0;
    for (uint32_t i = 0; i < count; ++i) {
      const Light& l = ls[i];
      bool keep = false;
      if (covered && casts(l)) {
        const float Pl[3] = {l.P.x, l.P.y, l.P.z};
        float e[3];
        for (int k = 0; k < 3; ++k) e[k] = std::fmax(std::fmax(lo[k] - Pl[k], Pl[k] - hi[k]), 0.0f);
        const float dist2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
        const float RRm = (l.R * l.R) * 1.000244140625f;
        keep = dist2 < RRm;
      }
      if (keep) ++nKept;
      if ((anyCand[i >> 3] >> (i & 7u)) & 1u) ++nCand;
      if (((anyReach[i >> 3] >> (i & 7u)) & 1u) && !keep) ++violations;
    }
    kept[b] = nKept; cands[b] = nCand;
  }
  return violations;
}
extern "C" uint64_t orc_ray_trace_light_list(void* h, uint32_t depth, uint32_t samples, uint32_t M, const float* L, const float* E, const float* T, const float* B, float k,
                                             uint32_t flags, const float* lights, uint32_t count, uint64_t* hitRays, uint64_t* pcounts, int16_t* pchosen0) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  if (count > 1024u) return ~0ull;
  const TableM& t = table_m(M);
  SunHits sun;
  sun.on = (flags & 1u) != 0u; sun.sums = (flags & 2u) != 0u || samples > 1u;
  sun.L = f3(L[0], L[1], L[2]); sun.E = f3(E[0], E[1], E[2]);
  const SunDisk K = sun_disk(T, B, k);
  const std::vector<Light> ls = read_light_list(lights, count);
  const LightListHits lh{(flags & 8u) != 0u && count > 0u, ls.data(), count};
  std::atomic<uint64_t> rays{0};
  std::mutex lock;
  uint64_t shadow = 0;
  parallel_rows(c->threads, c->H, [&](uint32_t y) {
    uint64_t r = 0, hr = 0; SunHitCounts n; SunSoftCounts sn; LightListCounts pn; std::vector<ListCand> cs;
    for (uint32_t x = 0; x < c->W; ++x) r += raygen_pixel_ll(*c, t, x, y, depth, samples, M, sun, n, K, sn, lh, hr, pn, pchosen0, cs);
    rays += r;
    std::lock_guard<std::mutex> g(lock);
    shadow += hr;
    if (pcounts) for (int d = 0; d < 4; ++d) for (int k2 = 0; k2 < LL_COLUMNS; ++k2) pcounts[d * LL_COLUMNS + k2] += pn.n[d][k2];
  });
  if (hitRays) *hitRays = shadow;
  c->rayCount = rays.load();
  return c->rayCount;
}
