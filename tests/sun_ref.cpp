// CPU restatement of the sun (rtggx_set_sun; include/rtggx.h has the rule): orc_sun_apply(h, L, E, classes) applies steps 1-5 to the oracle's
// RayTracingOut0/1 after any ray_trace() -- the oracle's own or one of the restatements this file includes -- and returns the number of shadow
// rays.  Occlusion is the `valid` of the oracle's closest hit on the shadow ray, which is what the any-hit traversal computes by construction.
// classes (may be null): per pixel 0 not covered, 1 NoL <= 0, 2 occluded, 3 lit.  Every operation is fp32, rounded on its own (-ffp-contract=off).
#include "restatements.cpp"

namespace orc {
static inline uint32_t sun_pixel(Ctx& c, uint32_t px, uint32_t py, float3 L, float3 E, uint8_t* classes) {
  const uint32_t W = c.W, H = c.H; const size_t pix = (size_t)py * W + px;
  const FrameConstants& fc = c.fc;
  uint32_t visibility = c.vis[pix];
  if (classes) classes[pix] = 0;
  if (visibility == 0) return 0;
  // getPrimarySurface :277-333, the covered branch, as raygen_pixel has it
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
  if (NoL <= 0.0f) { if (classes) classes[pix] = 1; return 0; }
  if (trace_closest(c, P, L, 1e-5f, 10000.0f, inst, prim).valid) { if (classes) classes[pix] = 2; return 1; }
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
}  // namespace orc

extern "C" uint64_t orc_sun_apply(void* h, const float* L, const float* E, uint8_t* classes) {
  using namespace orc;
  Ctx* c = (Ctx*)h;
  const float3 l = f3(L[0], L[1], L[2]), e = f3(E[0], E[1], E[2]);
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) { uint64_t r = 0; for (uint32_t x = 0; x < c->W; ++x) r += sun_pixel(*c, x, y, l, e, classes); rays += r; });
  c->rayCount += rays.load();
  return rays.load();
}
