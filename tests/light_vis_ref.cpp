// TEST INFRASTRUCTURE ONLY.  CPU restatement of the pick weighted by what the pixel remembers (rtggx_set_light_pick_visibility; include/rtggx.h
// has the rule): tests/light_pick_ref.cpp -- the whole oracle and every restatement below it -- plus the primary pass with the records in
// scalar C++:
//   orc_light_vis_apply     the primary pass of an acting frame on the oracle's RayTracingOut0/1, normal and velocity words as they are
//                           (orc_light_pick_apply's place): reads one image of records, writes the other
//   orc_light_vis_update    step 6 for one byte
//   orc_light_vis_runs      how many occlusions in a row take 255 to 0, and how many lit outcomes take 0 to 255
// A record is four words (RtggxLightVisRecord): v[0..3], v[4..7], the normal word, the stamp.  Per pixel the pass records what
// orc_light_pick_apply records (weights: the w_i, before the records weigh them; wf: U and f) and vinfo [H][W][4] bytes: the history's class
// (VC_*; 0: not covered), flags (VF_*), the chosen light's byte before and after the update (both 0 where nothing was chosen).
// Every operation is fp32, rounded on its own (-ffp-contract=off).
#include "light_pick_ref.cpp"

namespace orc {
enum { VC_NONE = 0, VC_VALID, VC_SEQUENCE, VC_OFF_FRAME, VC_STAMP, VC_INSTANCE, VC_NORMAL };
enum { VF_FLOOR = 1, VF_DIFFERS = 2, VF_ZERO = 4, VF_FULL = 8, VF_UPDATED = 16 };      // a candidate below the floor; the pick is not mode 1's on the same draw; a candidate at 0; at 255; a ray was traced
static const uint32_t kVisFloor = 16u;

static inline uint32_t vis_update(uint32_t v, bool occluded) { return occluded ? v - ((v + 3u) >> 2) : v + ((255u - v + 3u) >> 2); }
static inline int vis_normal_dot(uint32_t a, uint32_t b) {
  const int ax = 2 * (int)(a & 1023u) - 1023, ay = 2 * (int)((a >> 10) & 1023u) - 1023, az = 2 * (int)((a >> 20) & 1023u) - 1023;
  const int bx = 2 * (int)(b & 1023u) - 1023, by = 2 * (int)((b >> 10) & 1023u) - 1023, bz = 2 * (int)((b >> 20) & 1023u) - 1023;
  return ax * bx + ay * by + az * bz;
}
static inline uint32_t vis_byte(const uint32_t* rec, uint32_t i) { return (rec[i >> 2] >> (8u * (i & 3u))) & 0xFFu; }

static inline uint32_t vis_pixel(Ctx& c, uint32_t px, uint32_t py, const Light* lights, uint32_t count, uint32_t frameIndex, bool unoccluded, const PickRecord& rec,
                                 const uint32_t* prev, uint32_t* next, uint32_t s, uint32_t s0, uint8_t* vinfo) {
  const uint32_t W_ = c.W, H = c.H; const size_t pix = (size_t)py * W_ + px;
  const FrameConstants& fc = c.fc;
  uint32_t visibility = c.vis[pix];
  if (rec.info) { rec.info[pix * 4] = 0; rec.info[pix * 4 + 1] = 255; rec.info[pix * 4 + 2] = 0; rec.info[pix * 4 + 3] = 0; }
  if (rec.wf) rec.wf[pix * 2] = rec.wf[pix * 2 + 1] = 0.0f;
  if (rec.terms) for (int k = 0; k < 6; ++k) rec.terms[pix * 6 + k] = 0.0f;
  if (rec.weights) for (int k = 0; k < 8; ++k) rec.weights[pix * 8 + k] = 0.0f;
  if (vinfo) for (int k = 0; k < 4; ++k) vinfo[pix * 4 + k] = 0;
  if (visibility == 0) return 0;      // not covered: nothing is written
  // step 0: pick_pixel's surface
  float2 screenPos = {((float)px + 0.5f) / (float)W_ * 2.0f - 1.0f, ((float)py + 0.5f) / (float)H * 2.0f - 1.0f};
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
  // step 1: the candidates, pick_pixel's
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
    if (!(wi > 0.0f)) continue;
    w[i] = wi; cand[i] = true; D[i] = r.D; ++n;
  }
  if (rec.info) rec.info[pix * 4] = (uint8_t)n;
  if (rec.weights) for (int k = 0; k < 8; ++k) rec.weights[pix * 8 + k] = w[k];
  // step 2: the history
  const uint32_t nrm = c.normal[pix], vel = c.velocity[pix];
  const float vx = f16_to_f32((uint16_t)(vel & 0xFFFFu)), vy = f16_to_f32((uint16_t)(vel >> 16));
  const float qx = std::floor(((float)px + 0.5f) - vx * (float)W_), qy = std::floor(((float)py + 0.5f) - vy * (float)H);
  uint8_t cls = VC_VALID;
  const uint32_t* R = nullptr;
  if (!(s - 1u > s0)) cls = VC_SEQUENCE;
  else if (!(qx >= 0.0f && qx < (float)W_ && qy >= 0.0f && qy < (float)H)) cls = VC_OFF_FRAME;
  else {
    R = prev + 4u * ((size_t)(uint32_t)qy * W_ + (uint32_t)qx);
    if ((R[3] >> 8) != ((s - 1u) & 0xFFFFFFu)) cls = VC_STAMP;
    else if ((R[3] & 0xFFu) != inst + 1u) cls = VC_INSTANCE;
    else if (!((float)vis_normal_dot(R[2], nrm) >= 0.9f * 1046529.0f)) cls = VC_NORMAL;
  }
  uint32_t* mine = next + 4u * pix;
  mine[0] = cls == VC_VALID ? R[0] : 0xFFFFFFFFu; mine[1] = cls == VC_VALID ? R[1] : 0xFFFFFFFFu;
  mine[2] = nrm; mine[3] = ((s & 0xFFFFFFu) << 8) | (inst + 1u);
  if (vinfo) vinfo[pix * 4] = cls;
  if (n == 0) return 0;
  // step 3: the weights
  float u[8] = {};
  uint8_t flags = 0;
  for (uint32_t i = 0; i < 8u; ++i) {
    if (!cand[i]) continue;
    const uint32_t vi = vis_byte(mine, i);
    if (vi < kVisFloor) flags |= VF_FLOOR;
    if (vi == 0u) flags |= VF_ZERO;
    if (vi == 255u) flags |= VF_FULL;
    u[i] = w[i] * (float)(vi > kVisFloor ? vi : kVisFloor);
  }
  // step 4: mode 1's draw, pick and f on u
  const float U = pick_sum(u, cand);
  const float x = pick_x(pick_word((uint32_t)pix, frameIndex, 96u));
  bool fallback, later;
  const int ch = pick_choose(u, cand, x * U, fallback, later);
  const float f = U / u[ch];
  { bool fb1, lt1; if (pick_choose(w, cand, x * pick_sum(w, cand), fb1, lt1) != ch) flags |= VF_DIFFERS; }
  if (rec.info) { rec.info[pix * 4 + 1] = (uint8_t)ch; rec.info[pix * 4 + 3] = (uint8_t)((fallback ? 1 : 0) | (later ? 2 : 0)); }
  if (rec.wf) { rec.wf[pix * 2] = U; rec.wf[pix * 2 + 1] = f; }
  const uint32_t before = vis_byte(mine, (uint32_t)ch);
  if (vinfo) { vinfo[pix * 4 + 1] = flags; vinfo[pix * 4 + 2] = vinfo[pix * 4 + 3] = (uint8_t)before; }
  // step 5: mode 1's steps 6 and 7
  float3 Ls; float tmax = 0.0f;
  uint8_t rc = light_target(lights[ch], D[ch], N, (uint32_t)pix, frameIndex, 16u + (uint32_t)ch, Ls, tmax);
  if (rc) { if (rec.info) rec.info[pix * 4 + 2] = rc; return 0; }      // no ray: v as carried
  rc = !unoccluded && trace_closest(c, P, Ls, 1e-5f, tmax, inst, prim).valid ? LC_OCCLUDED : LC_LIT;
  if (rec.info) rec.info[pix * 4 + 2] = rc;
  // step 6: the update
  const uint32_t after = vis_update(before, rc == LC_OCCLUDED), shift = 8u * ((uint32_t)ch & 3u);
  mine[ch >> 2] = (mine[ch >> 2] & ~(0xFFu << shift)) | (after << shift);
  if (vinfo) { vinfo[pix * 4 + 1] = (uint8_t)(flags | VF_UPDATED); vinfo[pix * 4 + 3] = (uint8_t)after; }
  if (rc == LC_OCCLUDED) return 1;
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
}  // namespace orc

extern "C" uint32_t orc_light_vis_floor() { return orc::kVisFloor; }
extern "C" uint32_t orc_light_vis_update(uint32_t v, uint32_t occluded) { return orc::vis_update(v & 0xFFu, occluded != 0u); }
// out[0]: occlusions in a row from 255 until 0; out[1]: lit outcomes in a row from 0 until 255 (at most 1000 each)
extern "C" void orc_light_vis_runs(uint32_t* out) {
  uint32_t v = 255u, n = 0;
  while (v != 0u && n < 1000u) { v = orc::vis_update(v, true); ++n; }
  out[0] = n;
  v = 0u; n = 0;
  while (v != 255u && n < 1000u) { v = orc::vis_update(v, false); ++n; }
  out[1] = n;
}
extern "C" uint64_t orc_light_vis_apply(void* h, const float* lights, uint32_t count, uint32_t frameIndex, uint32_t flags, uint8_t* info, float* wf, float* terms, float* weights,
                                        const uint32_t* prev, uint32_t* next, uint32_t s, uint32_t s0, uint8_t* vinfo) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  Light ls[8];
  if (count > 8u || !prev || !next || prev == next) return ~0ull;
  read_lights(lights, count, ls);
  const PickRecord rec{info, wf, terms, weights};
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) { uint64_t r = 0; for (uint32_t x = 0; x < c->W; ++x) r += vis_pixel(*c, x, y, ls, count, frameIndex, (flags & 1u) != 0u, rec, prev, next, s, s0, vinfo); rays += r; });
  c->rayCount += rays.load();
  return rays.load();
}
