// TEST INFRASTRUCTURE ONLY.  CPU restatement of the local lights (rtggx_set_lights; include/rtggx.h has the rule): tests/sun_soft_ref.cpp -- the
// whole oracle, every restatement and the three sun passes -- plus the lights' pass, steps 0-8 of the rule on the oracle's RayTracingOut0/1 as
// they are, behind whatever ray_trace() and sun pass ran.  lights: count records in RtggxLight's layout (16 floats), the axis already
// normalised as the host normalises it (tests/lights_ref.py mirrors that).  classes (may be null): [count][H][W], per light and pixel
// 0 not covered (or a light without intensity), 1 out of range, 2 facing away, 3 outside the cone, 4 below the horizon, 5 occluded, 6 lit.
// aux (may be null): [count][H][W][2] floats, at pixels of class 5 and 6 the cone's s of step 3 (1 without a cone) and the final win of step
// 4.  flags bit 0: every ray that exists counts as unoccluded.  Every operation is fp32, rounded on its own (-ffp-contract=off).
#include "sun_soft_ref.cpp"

namespace orc {
struct Light { float3 P; float R; float3 I; float rho; float3 A; float cosOuter, cosInner; };
enum { LC_NONE = 0, LC_RANGE = 1, LC_AWAY = 2, LC_CONE = 3, LC_BELOW = 4, LC_OCCLUDED = 5, LC_LIT = 6 };

// step 5 with rho > 0: the point of the unit sphere light i draws at this pixel and frame
static inline float3 light_sphere_point(uint32_t pixel, uint32_t frameIndex, uint32_t i, float* uOut = nullptr, uint32_t* sOut = nullptr) {
  const TableM& t = table_m(256);      // always the 256-entry table, whatever the sample set
  uint32_t h = rng(pixel); h += frameIndex; h = rng(h);
  const uint32_t w = rng(h + (16u + i) * 0x9E3779B9u);
  const float u = (float)(w & 0xffffu) / 65536.0f;
  const uint32_t s = w >> 24;
  const float z = 1.0f - 2.0f * u;
  const float rho = std::sqrt(1.0f - z * z);
  if (uOut) *uOut = u;
  if (sOut) *sOut = s;
  return f3(rho * t.cosTab[s], rho * t.sinTab[s], z);
}
static inline float3 light_sphere_point_us(float u, uint32_t s) {      // the same from (u, s), for the test of |o|
  const TableM& t = table_m(256);
  const float z = 1.0f - 2.0f * u;
  const float rho = std::sqrt(1.0f - z * z);
  return f3(rho * t.cosTab[s], rho * t.sinTab[s], z);
}

static inline uint32_t lights_pixel(Ctx& c, uint32_t px, uint32_t py, const Light* lights, uint32_t count, uint32_t frameIndex, uint8_t* classes, float* aux, bool unoccluded) {
  const uint32_t W = c.W, H = c.H; const size_t pix = (size_t)py * W + px, frame = (size_t)W * H;
  const FrameConstants& fc = c.fc;
  uint32_t visibility = c.vis[pix];
  if (classes) for (uint32_t i = 0; i < count; ++i) classes[i * frame + pix] = LC_NONE;
  if (aux) for (uint32_t i = 0; i < count; ++i) aux[(i * frame + pix) * 2] = aux[(i * frame + pix) * 2 + 1] = 0.0f;
  if (visibility == 0) return 0;
  // step 0: sun_soft_pixel's surface
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
  float3 S0 = f3(0, 0, 0), S1 = f3(0, 0, 0);
  uint32_t n = 0, rays = 0;
  for (uint32_t i = 0; i < count; ++i) {
    const Light& l = lights[i];
    if (!(l.I.x > 0.0f || l.I.y > 0.0f || l.I.z > 0.0f)) continue;
    uint8_t* const cls = classes ? classes + i * frame + pix : nullptr;
    // 1
    const float3 D = f3(l.P.x - P.x, l.P.y - P.y, l.P.z - P.z);
    const float d2 = dot(D, D), RR = l.R * l.R;
    if (d2 < 1e-6f || d2 >= RR) { if (cls) *cls = LC_RANGE; continue; }
    // 2
    const float3 L = normalize(D);
    const float NoL = dot(N, L);
    if (NoL <= 0.0f) { if (cls) *cls = LC_AWAY; continue; }
    // 3
    float spot = 1.0f, s = 1.0f;
    if (l.cosOuter > -1.0f) {
      const float cc = -dot(L, l.A);
      if (cc <= l.cosOuter) { if (cls) *cls = LC_CONE; continue; }
      s = saturate((cc - l.cosOuter) / (l.cosInner - l.cosOuter));
      spot = s * s;
    }
    // 4
    const float q = d2 / RR;
    float win = saturate(1.0f - q * q); win = win * win;
    const float m2 = std::fmax(l.rho * l.rho, 1e-4f);
    const float att = (win * spot) / std::fmax(d2, m2);
    const float3 E = f3(l.I.x * att, l.I.y * att, l.I.z * att);
    // 5
    float3 Ds = D;
    if (l.rho > 0.0f) {
      const float3 o = light_sphere_point((uint32_t)pix, frameIndex, i);
      Ds = f3(D.x + l.rho * o.x, D.y + l.rho * o.y, D.z + l.rho * o.z);
    }
    const float ds2 = dot(Ds, Ds);
    if (ds2 < 1e-6f) { if (cls) *cls = LC_RANGE; continue; }      // (the target in the surface: counted with "out of range")
    const float3 Ls = normalize(Ds);
    const float tmax = std::sqrt(ds2);
    // 6
    if (!(dot(N, Ls) > 0.0f)) { if (cls) *cls = LC_BELOW; continue; }
    // 7
    ++rays;
    if (aux) { aux[(i * frame + pix) * 2] = s; aux[(i * frame + pix) * 2 + 1] = win; }
    if (!unoccluded && trace_closest(c, P, Ls, 1e-5f, tmax, inst, prim).valid) { if (cls) *cls = LC_OCCLUDED; continue; }
    if (cls) *cls = LC_LIT;
    // 8
    const float r = std::fmax(rghMtl.x, 1.0f / 32.0f);
    const float3 Hh = normalize(V + L);
    const float NoH = saturate(dot(N, Hh)), VoH = saturate(dot(V, Hh)), NoV = saturate(dot(N, V));
    const float al = r * r, a2 = al * al;
    const float d = (NoH * a2 - NoH) * NoH + 1.0f;
    const float Dg = a2 / ((kPI * d) * d);
    const float3 f0 = f3(lerp(0.04f, color.x, rghMtl.y), lerp(0.04f, color.y, rghMtl.y), lerp(0.04f, color.z, rghMtl.y));
    const float3 F = f_schlick(f0, VoH);
    const float vis = vis_smith(r, NoV, NoL);
    const float k = (Dg * vis) * NoL;
    S0 = f3(S0.x + (F.x * k) * E.x, S0.y + (F.y * k) * E.y, S0.z + (F.z * k) * E.z);
    if (rghMtl.y < 1.0f) {
      const float g = (NoL / kPI) * att;
      S1 = f3(S1.x + ((color.x * (1.0f - 0.04f)) * g) * l.I.x, S1.y + ((color.y * (1.0f - 0.04f)) * g) * l.I.y, S1.z + ((color.z * (1.0f - 0.04f)) * g) * l.I.z);
    }
    ++n;
  }
  if (n > 0) {
    float rgb[3];
    unpack_r11g11b10f(c.refl[pix], rgb);
    c.refl[pix] = pack_r11g11b10f(rgb[0] + S0.x, rgb[1] + S0.y, rgb[2] + S0.z);
    if (rghMtl.y < 1.0f) {
      unpack_r11g11b10f(c.diff[pix], rgb);
      c.diff[pix] = pack_r11g11b10f(rgb[0] + S1.x, rgb[1] + S1.y, rgb[2] + S1.z);
    }
  }
  return rays;
}
}  // namespace orc

extern "C" uint64_t orc_lights_apply_aux(void* h, const float* lights, uint32_t count, uint32_t frameIndex, uint8_t* classes, uint32_t flags, float* aux) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  Light ls[8];
  if (count > 8u) return ~0ull;
  for (uint32_t i = 0; i < count; ++i) {
    const float* f = lights + 16u * i;
    ls[i] = Light{f3(f[0], f[1], f[2]), f[3], f3(f[4], f[5], f[6]), f[7], f3(f[8], f[9], f[10]), f[11], f[12]};
  }
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) { uint64_t r = 0; for (uint32_t x = 0; x < c->W; ++x) r += lights_pixel(*c, x, y, ls, count, frameIndex, classes, aux, (flags & 1u) != 0u); rays += r; });
  c->rayCount += rays.load();
  return rays.load();
}
extern "C" uint64_t orc_lights_apply(void* h, const float* lights, uint32_t count, uint32_t frameIndex, uint8_t* classes, uint32_t flags) {
  return orc_lights_apply_aux(h, lights, count, frameIndex, classes, flags, nullptr);
}
// out: o (3 floats) for the pair (u = k / 65536, s); and the pair a (pixel, FrameIndex, i) draws: out = o, u, s as a float
extern "C" void orc_light_sphere_point(uint32_t k, uint32_t s, float* out) {
  const orc::float3 o = orc::light_sphere_point_us((float)k / 65536.0f, s);
  out[0] = o.x; out[1] = o.y; out[2] = o.z;
}
extern "C" void orc_light_sphere_points(float* out) {      // all 65536 x 256: |o|^2 - 1 in double, its extremes into out[0], out[1]
  double lo = 0.0, hi = 0.0;
  for (uint32_t k = 0; k < 65536u; ++k) for (uint32_t s = 0; s < 256u; ++s) {
    const orc::float3 o = orc::light_sphere_point_us((float)k / 65536.0f, s);
    const double e = std::sqrt((double)o.x * o.x + (double)o.y * o.y + (double)o.z * o.z) - 1.0;
    if (e < lo) lo = e;
    if (e > hi) hi = e;
  }
  out[0] = (float)lo; out[1] = (float)hi;
}
extern "C" void orc_light_sphere_sample(uint32_t pixel, uint32_t frameIndex, uint32_t i, float* out) {
  float u; uint32_t s;
  const orc::float3 o = orc::light_sphere_point(pixel, frameIndex, i, &u, &s);
  out[0] = o.x; out[1] = o.y; out[2] = o.z; out[3] = u; out[4] = (float)s;
}
