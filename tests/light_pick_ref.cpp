// TEST INFRASTRUCTURE ONLY.  CPU restatement of one shadow ray per surface point for all local lights (rtggx_set_light_sampling; include/rtggx.h
// has the rule): tests/light_hit_ref.cpp -- the whole oracle, every restatement, the sun's passes, the lights' primary pass and the lights at
// the hits -- plus both passes of the new rule in scalar C++:
//   orc_light_pick_apply        the primary pass in mode 1 on the oracle's RayTracingOut0/1 as they are (orc_lights_apply's place)
//   orc_ray_trace_light_pick    light_hit_ref.cpp's path walker once more, with `mode`: 0 the lights' loop at every touched hit (line by line
//                               orc_ray_trace_light_hits), 1 the pick
//   orc_light_pick_intervals    all 2^24 values of the draw against eight weights
//   orc_light_pick_draw         the draw's word of a (pixel, frame index, slot)
// Per pixel the primary pass records (all may be null) info [H][W][4] bytes: the number of candidates, the chosen index (255: none), the
// class of the chosen ray (LC_* of lights_ref.cpp; LC_RANGE: the target in the surface; 0: no candidate), flags (bit 0: the "none, so the
// last candidate" branch was needed, bit 1: the chosen light is not the first candidate); wf [H][W][2] floats: W and f; terms [H][W][6]
// floats: S0 and S1 as added (0 where no term); weights [H][W][8] floats: w_i (0: no candidate).  flags bit 0 of the call: every ray that
// exists counts as unoccluded.  The hit pass records pcounts [4 levels][PC_COLUMNS], ADDED to what the array holds, and pchosen0 [2 images]
// [H][W] signed bytes: the light chosen at the level-0 hit of the pixel's last sample (-1: none).
// Every operation is fp32, rounded on its own (-ffp-contract=off).
#include "light_hit_ref.cpp"

namespace orc {
enum { PC_CAND1 = 0, PC_CAND2, PC_RANGE, PC_BELOW, PC_OCCLUDED, PC_LIT, PC_LATER, PC_FALLBACK, PC_CHOSEN0, PC_COLUMNS = PC_CHOSEN0 + 8 };
struct LightPickCounts { uint64_t n[4][PC_COLUMNS] = {}; };

static inline float pick_luminance(float3 c) { return (0.25f * c.x + 0.5f * c.y) + 0.25f * c.z; }
// step 3: the word v of the slot, and x
static inline uint32_t pick_word(uint32_t pixel, uint32_t frameIndex, uint32_t slot) {
  uint32_t h = rng(pixel); h += frameIndex; h = rng(h);
  return rng(h + slot * 0x9E3779B9u);
}
static inline float pick_x(uint32_t v) { return (float)(v >> 8) / 16777216.0f; }
// step 2
static inline float pick_sum(const float* w, const bool* cand) {
  float W = 0.0f;
  for (uint32_t i = 0; i < 8u; ++i) if (cand[i]) W = W + w[i];
  return W;
}
// step 4: the first candidate with t < c, else the last one
static inline int pick_choose(const float* w, const bool* cand, float t, bool& fallback, bool& later) {
  float c = 0.0f;
  int last = -1, first = -1, chosen = -1;
  for (int i = 0; i < 8; ++i) {
    if (!cand[i]) continue;
    if (first < 0) first = i;
    last = i;
    c = c + w[i];
    if (chosen < 0 && t < c) chosen = i;
  }
  fallback = chosen < 0;
  if (fallback) chosen = last;
  later = chosen != first;
  return chosen;
}

// steps 1-4 of rtggx_set_lights at (P, N): does the light reach, and then D, L, NoL, att
struct LightReach { bool reach; float3 D, L; float NoL, att; };
static inline LightReach light_reach(const Light& l, float3 P, float3 N) {
  LightReach o{};
  o.D = f3(l.P.x - P.x, l.P.y - P.y, l.P.z - P.z);
  const float d2 = dot(o.D, o.D), RR = l.R * l.R;
  if (d2 < 1e-6f || d2 >= RR) return o;
  o.L = normalize(o.D);
  o.NoL = dot(N, o.L);
  if (o.NoL <= 0.0f) return o;
  float spot = 1.0f;
  if (l.cosOuter > -1.0f) {
    const float cc = -dot(o.L, l.A);
    if (cc <= l.cosOuter) return o;
    const float s = saturate((cc - l.cosOuter) / (l.cosInner - l.cosOuter));
    spot = s * s;
  }
  const float q = d2 / RR;
  float win = saturate(1.0f - q * q); win = win * win;
  const float m2 = std::fmax(l.rho * l.rho, 1e-4f);
  o.att = (win * spot) / std::fmax(d2, m2);
  o.reach = true;
  return o;
}
// F k of step 8
static inline float3 light_Fk(float3 N, float3 V, float3 L, float NoL, float3 color, float2 rm) {
  const float r = std::fmax(rm.x, 1.0f / 32.0f);
  const float3 Hh = normalize(V + L);
  const float NoH = saturate(dot(N, Hh)), VoH = saturate(dot(V, Hh)), NoV = saturate(dot(N, V));
  const float al = r * r, a2 = al * al;
  const float d = (NoH * a2 - NoH) * NoH + 1.0f;
  const float Dg = a2 / ((kPI * d) * d);
  const float3 f0 = f3(lerp(0.04f, color.x, rm.y), lerp(0.04f, color.y, rm.y), lerp(0.04f, color.z, rm.y));
  const float3 F = f_schlick(f0, VoH);
  const float vis = vis_smith(r, NoV, NoL);
  const float k = (Dg * vis) * NoL;
  return f3(F.x * k, F.y * k, F.z * k);
}
// steps 5-6 for one light with hash slot j: the class where there is no ray (LC_RANGE: the target in the surface), else 0 with Ls and tmax
static inline uint8_t light_target(const Light& l, float3 D, float3 N, uint32_t pixel, uint32_t frameIndex, uint32_t j, float3& Ls, float& tmax) {
  float3 Ds = D;
  if (l.rho > 0.0f) {
    const float3 o = light_hit_sphere_point(pixel, frameIndex, j);
    Ds = f3(D.x + l.rho * o.x, D.y + l.rho * o.y, D.z + l.rho * o.z);
  }
  const float ds2 = dot(Ds, Ds);
  if (ds2 < 1e-6f) return LC_RANGE;
  Ls = normalize(Ds);
  tmax = std::sqrt(ds2);
  if (!(dot(N, Ls) > 0.0f)) return LC_BELOW;
  return 0;
}

struct PickRecord { uint8_t* info; float* wf; float* terms; float* weights; };

static inline uint32_t pick_pixel(Ctx& c, uint32_t px, uint32_t py, const Light* lights, uint32_t count, uint32_t frameIndex, bool unoccluded, const PickRecord& rec) {
  const uint32_t W_ = c.W, H = c.H; const size_t pix = (size_t)py * W_ + px;
  const FrameConstants& fc = c.fc;
  uint32_t visibility = c.vis[pix];
  if (rec.info) { rec.info[pix * 4] = 0; rec.info[pix * 4 + 1] = 255; rec.info[pix * 4 + 2] = 0; rec.info[pix * 4 + 3] = 0; }
  if (rec.wf) rec.wf[pix * 2] = rec.wf[pix * 2 + 1] = 0.0f;
  if (rec.terms) for (int k = 0; k < 6; ++k) rec.terms[pix * 6 + k] = 0.0f;
  if (rec.weights) for (int k = 0; k < 8; ++k) rec.weights[pix * 8 + k] = 0.0f;
  if (visibility == 0) return 0;
  (void)H;
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
  // step 1: the candidates
  float w[8] = {}; bool cand[8] = {}; float3 spec[8], diff[8], D[8];
  uint32_t n = 0;
  for (uint32_t i = 0; i < count; ++i) {
    const Light& l = lights[i];
    if (!(l.I.x > 0.0f || l.I.y > 0.0f || l.I.z > 0.0f)) continue;
    const LightReach r = light_reach(l, P, N);
    if (!r.reach) continue;
    const float3 Fk = light_Fk(N, V, r.L, r.NoL, color, rghMtl);
    spec[i] = f3(Fk.x * (l.I.x * r.att), Fk.y * (l.I.y * r.att), Fk.z * (l.I.z * r.att));
    float wi = pick_luminance(spec[i]);
    diff[i] = f3(0, 0, 0);
    if (diffuse) {
      const float g = (r.NoL / kPI) * r.att;
      diff[i] = f3(((color.x * (1.0f - 0.04f)) * g) * l.I.x, ((color.y * (1.0f - 0.04f)) * g) * l.I.y, ((color.z * (1.0f - 0.04f)) * g) * l.I.z);
      wi = wi + pick_luminance(diff[i]);
    }
    if (!(wi > 0.0f)) continue;      // (a NaN is not a candidate)
    w[i] = wi; cand[i] = true; D[i] = r.D; ++n;
  }
  if (rec.info) rec.info[pix * 4] = (uint8_t)n;
  if (rec.weights) for (int k = 0; k < 8; ++k) rec.weights[pix * 8 + k] = w[k];
  if (n == 0) return 0;
  // steps 2-5
  const float Wsum = pick_sum(w, cand);
  const float t = pick_x(pick_word((uint32_t)pix, frameIndex, 96u)) * Wsum;
  bool fallback, later;
  const int ch = pick_choose(w, cand, t, fallback, later);
  const float f = Wsum / w[ch];
  if (rec.info) { rec.info[pix * 4 + 1] = (uint8_t)ch; rec.info[pix * 4 + 3] = (uint8_t)((fallback ? 1 : 0) | (later ? 2 : 0)); }
  if (rec.wf) { rec.wf[pix * 2] = Wsum; rec.wf[pix * 2 + 1] = f; }
  // step 6
  float3 Ls; float tmax = 0.0f;
  uint8_t cls = light_target(lights[ch], D[ch], N, (uint32_t)pix, frameIndex, 16u + (uint32_t)ch, Ls, tmax);
  if (cls) { if (rec.info) rec.info[pix * 4 + 2] = cls; return 0; }
  cls = !unoccluded && trace_closest(c, P, Ls, 1e-5f, tmax, inst, prim).valid ? LC_OCCLUDED : LC_LIT;
  if (rec.info) rec.info[pix * 4 + 2] = cls;
  if (cls == LC_OCCLUDED) return 1;
  // step 7
  const float3 S0 = f3(0.0f + spec[ch].x * f, 0.0f + spec[ch].y * f, 0.0f + spec[ch].z * f);
  float rgb[3];
  unpack_r11g11b10f(c.refl[pix], rgb);
  c.refl[pix] = pack_r11g11b10f(rgb[0] + S0.x, rgb[1] + S0.y, rgb[2] + S0.z);
  if (rec.terms) { rec.terms[pix * 6] = S0.x; rec.terms[pix * 6 + 1] = S0.y; rec.terms[pix * 6 + 2] = S0.z; }
  if (diffuse) {
    const float3 S1 = f3(0.0f + diff[ch].x * f, 0.0f + diff[ch].y * f, 0.0f + diff[ch].z * f);
    unpack_r11g11b10f(c.diff[pix], rgb);
    c.diff[pix] = pack_r11g11b10f(rgb[0] + S1.x, rgb[1] + S1.y, rgb[2] + S1.z);
    if (rec.terms) { rec.terms[pix * 6 + 3] = S1.x; rec.terms[pix * 6 + 4] = S1.y; rec.terms[pix * 6 + 5] = S1.z; }
  }
  return 1;
}

// step 4 of rtggx_set_light_reflections: the term of the lobe the path uses at the hit
static inline float3 light_hit_term(const Light& l, const LightReach& r, float3 N, float3 V, float2 rm, float3 color, bool diffuseGroup) {
  if (rm.y > 0.5f) {
    const float3 Fk = light_Fk(N, V, r.L, r.NoL, color, rm);
    return f3(Fk.x * (l.I.x * r.att), Fk.y * (l.I.y * r.att), Fk.z * (l.I.z * r.att));
  }
  if (diffuseGroup) color = color * (1.0f - rm.y);
  const float g = (r.NoL / kPI) * r.att;
  return f3((color.x * g) * l.I.x, (color.y * g) * l.I.y, (color.z * g) * l.I.z);
}
// the hits' rule in mode 1 at one touched hit: the chosen light (-1: no candidate) and, where lit, s_i f added to S
static inline int pick_hit(const Ctx& c, const LightHits& lh, float3 P, float3 N, float3 V, float2 rm, float3 color, bool diffuseGroup, uint32_t hInst, uint32_t hPrim,
                           float3 T, uint32_t pixel, uint32_t frameIndex, uint32_t d, uint32_t image, float3& S, uint32_t& rays, uint64_t& hitRays, uint64_t* pc, bool& lit) {
  float w[8] = {}; bool cand[8] = {}; float3 s[8], D[8];
  uint32_t n = 0;
  lit = false;
  for (uint32_t i = 0; i < lh.count; ++i) {
    const Light& l = lh.l[i];
    if (!(l.I.x > 0.0f || l.I.y > 0.0f || l.I.z > 0.0f)) continue;
    const LightReach r = light_reach(l, P, N);
    if (!r.reach) continue;
    const float3 term = light_hit_term(l, r, N, V, rm, color, diffuseGroup);
    s[i] = f3(T.x * term.x, T.y * term.y, T.z * term.z);
    const float wi = pick_luminance(s[i]);
    if (!(wi > 0.0f)) continue;
    w[i] = wi; cand[i] = true; D[i] = r.D; ++n;
  }
  if (n == 0) return -1;
  ++pc[PC_CAND1];
  if (n >= 2) ++pc[PC_CAND2];
  const float Wsum = pick_sum(w, cand);
  const float t = pick_x(pick_word(pixel, frameIndex, 104u + 2u * d + image)) * Wsum;
  bool fallback, later;
  const int ch = pick_choose(w, cand, t, fallback, later);
  const float f = Wsum / w[ch];
  if (n >= 2) ++pc[PC_CHOSEN0 + ch];
  if (fallback) ++pc[PC_FALLBACK];
  if (later && !fallback) ++pc[PC_LATER];
  float3 Ls; float tmax = 0.0f;
  const uint8_t cls = light_target(lh.l[ch], D[ch], N, pixel, frameIndex, 32u + 16u * d + 8u * image + (uint32_t)ch, Ls, tmax);
  if (cls) { ++pc[cls == LC_RANGE ? PC_RANGE : PC_BELOW]; return ch; }
  ++rays; ++hitRays;
  if (trace_closest(c, P, Ls, 1e-5f, tmax, hInst, hPrim).valid) { ++pc[PC_OCCLUDED]; return ch; }
  ++pc[PC_LIT];
  S = f3(S.x + s[ch].x * f, S.y + s[ch].y * f, S.z + s[ch].z * f);
  lit = true;
  return ch;
}

// follow_path_l with the mode: 0 its lights' loop, 1 the pick
static inline float3 follow_path_p(const Ctx& c, float3 o, float3 dir, uint32_t skipInst, uint32_t skipPrim, bool diffuseGroup, float3 preset,
                                   const SampleM& xi, uint32_t D, float3& T, uint32_t& rays, const SunHits& sun, float3& S, bool& any, SunHitCounts& n,
                                   const SunDisk& K, uint32_t pixel, uint32_t frameIndex, uint32_t image, bool stats, SunSoftCounts& sn, bool& changed,
                                   const LightHits& lh, LightHitCounts& ln, bool& anyLight, uint8_t* cls0, bool pick, LightPickCounts& pn, int8_t& chosen0) {
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
    if (lh.on && pick) {
      bool lit;
      const int ch = pick_hit(c, lh, P, N, V, rm, color, diffuseGroup, h.inst, h.prim, T, pixel, frameIndex, d, image, S, rays, ln.rays, pn.n[d], lit);
      if (lit) { any = true; anyLight = true; }
      if (d == 0) chosen0 = (int8_t)ch;
    } else if (lh.on) {
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

// raygen_pixel_l, its two walks through follow_path_p
static inline uint32_t raygen_pixel_p(Ctx& c, const TableM& t, uint32_t px, uint32_t py, uint32_t D, uint32_t N, uint32_t M, const SunHits& sun, SunHitCounts& n, uint8_t* lit,
                                      const SunDisk& K, bool stats, SunSoftCounts& sn, uint8_t* changed, const LightHits& lh, LightHitCounts& ln, uint8_t* llit, uint8_t* lcls0,
                                      bool pick, LightPickCounts& pn, int8_t* pchosen0) {
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
  bool anyR = false, anyD = false, chR = false, chD = false, lightR = false, lightD = false;
  uint8_t cls[2][8];
  int8_t chosen[2] = {-1, -1};
  for (uint32_t k = 0; k < N; ++k) {
    const uint32_t index = fc.g.FrameIndex * N + k;      // sample k's frame index: the path's, and the one its hits draw with
    const SampleM xi = get_sample_param_m(t, px, py, W, index, M);
    for (int i = 0; i < 8; ++i) cls[0][i] = cls[1][i] = 0;
    chosen[0] = chosen[1] = -1;
    {
      const float3 Hh = half_vector_m(c, s.N, s.V, s.rghMtl.x * s.rghMtl.x, xi);
      const float3 R = reflect(-s.V, Hh);
      const float NoL = dot(s.N, R);
      float3 v = f3(0, 0, 0);
      if (NoL > 0.0f) {
        float3 T = reflection_weight_m(c, s.N, s.V, Hh, NoL, s.rghMtl, s.color);
        const float3 col = follow_path_p(c, s.P, R, s.inst, s.prim, false, s.color * s.rghMtl.y, xi, D, T, rays, sun, sun.sums ? accR : SR, anyR, n, K, (uint32_t)pix, index, 0u, stats, sn, chR,
                                         lh, ln, lightR, cls[0], pick, pn, chosen[0]);
        v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      }
      accR = f3(accR.x + v.x, accR.y + v.y, accR.z + v.z);
    }
    if (diffuse) {
      const float3 dir = diffuse_direction_m(s.N, xi);
      float3 T = s.color * (1.0f - 0.04f);
      const float3 col = follow_path_p(c, s.P, dir, s.inst, s.prim, true, s.color * s.rghMtl.y, xi, D, T, rays, sun, sun.sums ? accD : SD, anyD, n, K, (uint32_t)pix, index, 1u, stats, sn, chD,
                                       lh, ln, lightD, cls[1], pick, pn, chosen[1]);
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
  if (pchosen0) { pchosen0[pix] = chosen[0]; pchosen0[frame + pix] = chosen[1]; }
  return rays;
}

static inline void read_lights(const float* lights, uint32_t count, Light* ls) {
  for (uint32_t i = 0; i < count; ++i) {
    const float* f = lights + 16u * i;
    ls[i] = Light{f3(f[0], f[1], f[2]), f[3], f3(f[4], f[5], f[6]), f[7], f3(f[8], f[9], f[10]), f[11], f[12]};
  }
}
}  // namespace orc

extern "C" uint32_t orc_light_pick_columns() { return orc::PC_COLUMNS; }
extern "C" uint32_t orc_light_pick_draw(uint32_t pixel, uint32_t frameIndex, uint32_t slot) { return orc::pick_word(pixel, frameIndex, slot); }
extern "C" uint64_t orc_light_pick_apply(void* h, const float* lights, uint32_t count, uint32_t frameIndex, uint32_t flags, uint8_t* info, float* wf, float* terms, float* weights) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  Light ls[8];
  if (count > 8u) return ~0ull;
  read_lights(lights, count, ls);
  const PickRecord rec{info, wf, terms, weights};
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) { uint64_t r = 0; for (uint32_t x = 0; x < c->W; ++x) r += pick_pixel(*c, x, y, ls, count, frameIndex, (flags & 1u) != 0u, rec); rays += r; });
  c->rayCount += rays.load();
  return rays.load();
}
// w: eight weights (0: no candidate).  out: per light the number of values k = v >> 8 of all 2^24 that choose it, the first and the last such k
extern "C" void orc_light_pick_intervals(const float* w, uint64_t* out) {
  using namespace orc;
  bool cand[8];
  for (int i = 0; i < 8; ++i) { cand[i] = w[i] > 0.0f; out[3 * i] = 0; out[3 * i + 1] = ~0ull; out[3 * i + 2] = 0; }
  const float W = pick_sum(w, cand);
  for (uint32_t k = 0; k < (1u << 24); ++k) {
    const float t = pick_x(k << 8) * W;
    bool fallback, later;
    const int ch = pick_choose(w, cand, t, fallback, later);
    if (ch < 0) continue;
    if (!out[3 * ch]++) out[3 * ch + 1] = k;
    out[3 * ch + 2] = k;
  }
}
extern "C" uint64_t orc_ray_trace_light_pick(void* h, uint32_t depth, uint32_t samples, uint32_t M, const float* L, const float* E, const float* T, const float* B, float k,
                                             uint32_t flags, uint64_t* counts, uint8_t* lit, uint64_t* soft, uint8_t* changed,
                                             const float* lights, uint32_t count, uint64_t* lcounts, uint8_t* llit, uint8_t* lcls0, uint64_t* hitRays,
                                             uint32_t mode, uint64_t* pcounts, int8_t* pchosen0) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  if (count > 8u || mode > 1u) return ~0ull;
  const TableM& t = table_m(M);
  SunHits sun;
  sun.on = (flags & 1u) != 0u; sun.sums = (flags & 2u) != 0u || samples > 1u;
  sun.L = f3(L[0], L[1], L[2]); sun.E = f3(E[0], E[1], E[2]);
  const SunDisk K = sun_disk(T, B, k);
  const bool stats = (flags & 4u) != 0u;
  Light ls[8];
  read_lights(lights, count, ls);
  const LightHits lh{(flags & 8u) != 0u && count > 0u, ls, count};
  std::atomic<uint64_t> rays{0};
  std::mutex lock;
  uint64_t shadow = 0;
  parallel_rows(c->threads, c->H, [&](uint32_t y) {
    uint64_t r = 0; SunHitCounts n; SunSoftCounts sn; LightHitCounts ln; LightPickCounts pn;
    for (uint32_t x = 0; x < c->W; ++x) r += raygen_pixel_p(*c, t, x, y, depth, samples, M, sun, n, lit, K, stats, sn, changed, lh, ln, llit, lcls0, mode == 1u, pn, pchosen0);
    rays += r;
    std::lock_guard<std::mutex> g(lock);
    shadow += ln.rays;
    if (counts) for (int d = 0; d < 4; ++d) for (int k2 = 0; k2 < SH_COLUMNS; ++k2) counts[d * SH_COLUMNS + k2] += n.n[d][k2];
    if (soft) for (int d = 0; d < 4; ++d) for (int k2 = 0; k2 < 2; ++k2) soft[d * 2 + k2] += sn.n[d][k2];
    if (lcounts) for (int d = 0; d < 4; ++d) for (int i = 0; i < 8; ++i) for (int k2 = 0; k2 < LH_COLUMNS; ++k2) lcounts[(d * 8 + i) * LH_COLUMNS + k2] += ln.n[d][i][k2];
    if (pcounts) for (int d = 0; d < 4; ++d) for (int k2 = 0; k2 < PC_COLUMNS; ++k2) pcounts[d * PC_COLUMNS + k2] += pn.n[d][k2];
  });
  if (hitRays) *hitRays = shadow;
  c->rayCount = rays.load();
  return c->rayCount;
}
