// TEST INFRASTRUCTURE ONLY.  CPU restatement of a list's pick weighted by what the pixel remembers (rtggx_set_light_list_visibility;
// include/rtggx.h has the rule): tests/light_list_ref.cpp -- the whole oracle and every restatement below it, the list's rule among them --
// plus the primary pass with the sparse records over ALL n lights of the list, WITHOUT a cull, in scalar C++:
//   orc_light_list_vis_apply     the primary pass of an acting frame on the oracle's RayTracingOut0/1, normal and velocity words as they
//                                are (orc_light_list_apply's place): reads one image of records, writes the other
//   orc_light_list_vis_update    step 6 on one record's four entries
//   orc_light_list_vis_floor     RTGGX_LIGHT_LIST_VIS_FLOOR as restated
// A record is four words (RtggxLightListVisRecord): entries 0 and 1, entries 2 and 3 (the lower index in the low half), the normal word,
// the stamp.  Per pixel the pass records what orc_light_list_apply records (info, wf: U and f, terms, P, reach, cand) and vinfo [H][W][4]
// bytes: the history's class (LVC_*; 0: not covered); the event of the update (LVE_*) with flags in the high bits (LVF_*); the chosen
// light's v before and after the update (both 0 where nothing was chosen).
// Every operation is fp32, rounded on its own (-ffp-contract=off).
#include "light_list_ref.cpp"

namespace orc {
enum { LVC_NONE = 0, LVC_VALID, LVC_SEQUENCE, LVC_OFF_FRAME, LVC_STAMP, LVC_INSTANCE, LVC_NORMAL };
enum { LVE_NONE = 0, LVE_KEPT, LVE_MOVED, LVE_INSERTED, LVE_EVICTED, LVE_DROPPED };      // no ray; unrecorded and seen; an entry's v moved; a free slot taken; an entry replaced; an entry freed at 63
enum { LVF_RAY = 16, LVF_CARRIED = 32, LVF_FLOOR = 64, LVF_DIFFERS = 128 };              // a ray was traced; the carried record holds an entry; a candidate's v is below the floor; the pick is not the list's on the same draw
static const uint32_t kListVisFloor = 4u, kListVisFree = 0xFFFFu;

static inline int list_vis_normal_dot(uint32_t a, uint32_t b) {
  const int ax = 2 * (int)(a & 1023u) - 1023, ay = 2 * (int)((a >> 10) & 1023u) - 1023, az = 2 * (int)((a >> 20) & 1023u) - 1023;
  const int bx = 2 * (int)(b & 1023u) - 1023, by = 2 * (int)((b >> 10) & 1023u) - 1023, bz = 2 * (int)((b >> 20) & 1023u) - 1023;
  return ax * bx + ay * by + az * bz;
}
static inline uint32_t list_vis_entry(const uint32_t* rec, uint32_t k) { return (rec[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu; }
static inline void list_vis_set_entry(uint32_t* rec, uint32_t k, uint32_t e) { const uint32_t sh = 16u * (k & 1u); rec[k >> 1] = (rec[k >> 1] & ~(0xFFFFu << sh)) | (e << sh); }
// the slot, not free, that holds light i: the lowest; 4: none
static inline uint32_t list_vis_slot(const uint32_t* rec, uint32_t i) {
  for (uint32_t k = 0; k < 4u; ++k) { const uint32_t e = list_vis_entry(rec, k); if (e != kListVisFree && (e & 1023u) == i) return k; }
  return 4u;
}
static inline uint32_t list_vis_v(const uint32_t* rec, uint32_t i) { const uint32_t k = list_vis_slot(rec, i); return k < 4u ? list_vis_entry(rec, k) >> 10 : 63u; }
// step 6; returns the event
static inline uint8_t list_vis_update(uint32_t* rec, uint32_t i, bool occluded, uint32_t& before, uint32_t& after) {
  const uint32_t k = list_vis_slot(rec, i);
  before = k < 4u ? list_vis_entry(rec, k) >> 10 : 63u;
  after = occluded ? before - ((before + 3u) >> 2) : before + ((63u - before + 3u) >> 2);
  if (k < 4u) {
    list_vis_set_entry(rec, k, after == 63u ? kListVisFree : (after << 10) | i);
    return after == 63u ? LVE_DROPPED : LVE_MOVED;
  }
  if (!occluded) return LVE_KEPT;
  for (uint32_t j = 0; j < 4u; ++j) if (list_vis_entry(rec, j) == kListVisFree) { list_vis_set_entry(rec, j, (47u << 10) | i); return LVE_INSERTED; }
  uint32_t at = 0u;
  for (uint32_t j = 1; j < 4u; ++j) if ((list_vis_entry(rec, j) >> 10) > (list_vis_entry(rec, at) >> 10)) at = j;
  list_vis_set_entry(rec, at, (47u << 10) | i);
  return LVE_EVICTED;
}

static inline uint32_t list_vis_pixel(Ctx& c, uint32_t px, uint32_t py, const std::vector<Light>& lights, uint32_t frameIndex, bool unoccluded, const ListRecord& rec,
                                      std::vector<ListCand>& cs, const uint32_t* prev, uint32_t* next, uint32_t s, uint32_t s0, uint8_t* vinfo) {
  const uint32_t W_ = c.W, H = c.H; const size_t pix = (size_t)py * W_ + px;
  const size_t bytes = (lights.size() + 7u) / 8u;
  const FrameConstants& fc = c.fc;
  uint32_t visibility = c.vis[pix];
  if (rec.info) { rec.info[pix * 4] = 0; rec.info[pix * 4 + 1] = 0xFFFF; rec.info[pix * 4 + 2] = 0; rec.info[pix * 4 + 3] = 0; }
  if (rec.wf) rec.wf[pix * 2] = rec.wf[pix * 2 + 1] = 0.0f;
  if (rec.terms) for (int k = 0; k < 6; ++k) rec.terms[pix * 6 + k] = 0.0f;
  if (rec.P) for (int k = 0; k < 3; ++k) rec.P[pix * 3 + k] = 0.0f;
  if (rec.reach) for (size_t k = 0; k < bytes; ++k) rec.reach[pix * bytes + k] = 0;
  if (rec.cand) for (size_t k = 0; k < bytes; ++k) rec.cand[pix * bytes + k] = 0;
  if (vinfo) for (int k = 0; k < 4; ++k) vinfo[pix * 4 + k] = 0;
  if (visibility == 0) return 0;      // not covered: nothing is written
  // step 0: list_pixel's surface
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
  if (rec.P) { rec.P[pix * 3] = P.x; rec.P[pix * 3 + 1] = P.y; rec.P[pix * 3 + 2] = P.z; }
  // step 2: the history
  const uint32_t nrm = c.normal[pix], vel = c.velocity[pix];
  const float vx = f16_to_f32((uint16_t)(vel & 0xFFFFu)), vy = f16_to_f32((uint16_t)(vel >> 16));
  const float qx = std::floor(((float)px + 0.5f) - vx * (float)W_), qy = std::floor(((float)py + 0.5f) - vy * (float)H);
  uint8_t cls = LVC_VALID;
  const uint32_t* R = nullptr;
  if (!(s - 1u > s0)) cls = LVC_SEQUENCE;
  else if (!(qx >= 0.0f && qx < (float)W_ && qy >= 0.0f && qy < (float)H)) cls = LVC_OFF_FRAME;
  else {
    R = prev + 4u * ((size_t)(uint32_t)qy * W_ + (uint32_t)qx);
    if ((R[3] >> 8) != ((s - 1u) & 0xFFFFFFu)) cls = LVC_STAMP;
    else if ((R[3] & 0xFFu) != inst + 1u) cls = LVC_INSTANCE;
    else if (!((float)list_vis_normal_dot(R[2], nrm) >= 0.9f * 1046529.0f)) cls = LVC_NORMAL;
  }
  uint32_t* mine = next + 4u * pix;
  mine[0] = cls == LVC_VALID ? R[0] : 0xFFFFFFFFu; mine[1] = cls == LVC_VALID ? R[1] : 0xFFFFFFFFu;
  mine[2] = nrm; mine[3] = ((s & 0xFFFFFFu) << 8) | (inst + 1u);
  uint8_t flags = (mine[0] != 0xFFFFFFFFu || mine[1] != 0xFFFFFFFFu) ? LVF_CARRIED : 0;
  if (vinfo) { vinfo[pix * 4] = cls; vinfo[pix * 4 + 1] = flags; }
  // steps 1 and 3: the candidates over ALL lights, their weights times what the pixel remembers
  cs.clear();
  std::vector<ListCand> plain;      // the same candidates with the list's own weights: what the list would have picked on this draw
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
    plain.push_back(k);
    const uint32_t vi = list_vis_v(mine, i);
    if (vi < kListVisFloor) flags |= LVF_FLOOR;
    k.w = wi * (float)(vi > kListVisFloor ? vi : kListVisFloor);
    cs.push_back(k);
    if (rec.cand) rec.cand[pix * bytes + (i >> 3)] |= (uint8_t)(1u << (i & 7u));
  }
  if (rec.info) rec.info[pix * 4] = (uint16_t)cs.size();
  if (vinfo) vinfo[pix * 4 + 1] = flags;
  if (cs.empty()) return 0;
  // step 4: the list's draw, pick and f on u
  float U, f; bool fallback;
  const uint32_t word = pick_word((uint32_t)pix, frameIndex, 96u);
  const size_t at = list_choose(cs, word, U, f, fallback);
  const ListCand& ch = cs[at];
  { float W0, f0; bool fb0; if (plain[list_choose(plain, word, W0, f0, fb0)].i != ch.i) flags |= LVF_DIFFERS; }
  if (rec.info) { rec.info[pix * 4 + 1] = (uint16_t)ch.i; rec.info[pix * 4 + 3] = (uint16_t)((fallback ? 1 : 0) | (at != 0 ? 2 : 0)); }
  if (rec.wf) { rec.wf[pix * 2] = U; rec.wf[pix * 2 + 1] = f; }
  const uint32_t carried = list_vis_v(mine, ch.i);
  if (vinfo) { vinfo[pix * 4 + 1] = flags; vinfo[pix * 4 + 2] = vinfo[pix * 4 + 3] = (uint8_t)carried; }
  // step 5: the list's steps 6 and 7
  float3 Ls; float tmax = 0.0f;
  uint8_t rc = light_target(lights[ch.i], ch.D, N, (uint32_t)pix, frameIndex, list_slot(ch.i), Ls, tmax);
  if (rc) { if (rec.info) rec.info[pix * 4 + 2] = rc; return 0; }      // no ray: the entries as carried
  rc = !unoccluded && trace_closest(c, P, Ls, 1e-5f, tmax, inst, prim).valid ? LC_OCCLUDED : LC_LIT;
  if (rec.info) rec.info[pix * 4 + 2] = rc;
  // step 6: the update
  uint32_t before, after;
  const uint8_t event = list_vis_update(mine, ch.i, rc == LC_OCCLUDED, before, after);
  if (vinfo) { vinfo[pix * 4 + 1] = (uint8_t)(flags | LVF_RAY | event); vinfo[pix * 4 + 2] = (uint8_t)before; vinfo[pix * 4 + 3] = (uint8_t)after; }
  if (rc == LC_OCCLUDED) return 1;
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
}  // namespace orc

extern "C" uint32_t orc_light_list_vis_floor() { return orc::kListVisFloor; }
// entries: the record's four 16-bit entries, updated in place; out[0]: the event, out[1], out[2]: v before and after
extern "C" void orc_light_list_vis_update(uint16_t* entries, uint32_t light, uint32_t occluded, uint32_t* out) {
  uint32_t rec[2] = {(uint32_t)entries[0] | ((uint32_t)entries[1] << 16), (uint32_t)entries[2] | ((uint32_t)entries[3] << 16)};
  uint32_t before, after;
  out[0] = orc::list_vis_update(rec, light & 1023u, occluded != 0u, before, after);
  out[1] = before; out[2] = after;
  for (uint32_t k = 0; k < 4u; ++k) entries[k] = (uint16_t)orc::list_vis_entry(rec, k);
}
extern "C" uint64_t orc_light_list_vis_apply(void* h, const float* lights, uint32_t count, uint32_t frameIndex, uint32_t flags, uint16_t* info, float* wf, float* terms,
                                             float* P, uint8_t* reach, uint8_t* cand, const uint32_t* prev, uint32_t* next, uint32_t s, uint32_t s0, uint8_t* vinfo) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  if (count > 1024u || !prev || !next || prev == next) return ~0ull;
  const std::vector<Light> ls = read_light_list(lights, count);
  const ListRecord rec{info, wf, terms, P, reach, cand};
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) {
    uint64_t r = 0; std::vector<ListCand> cs;
    for (uint32_t x = 0; x < c->W; ++x) r += list_vis_pixel(*c, x, y, ls, frameIndex, (flags & 1u) != 0u, rec, cs, prev, next, s, s0, vinfo);
    rays += r;
  });
  c->rayCount += rays.load();
  return rays.load();
}
