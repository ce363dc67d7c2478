// TEST INFRASTRUCTURE ONLY.  Part of tests/restatements.cpp, which has brought in the CPU oracle before this file (oracle/orc_capi.cpp, whole
// and unchanged: Ctx::cosTab keeps its 256 entries).  orc_ray_trace_sampleset(h, D, N, M): raygenMain at recursion depth D with N samples
// per covered pixel drawn from a sample set of M members -- the semantics of rtggx_set_sample_set (include/rtggx.h, DESIGN.md "Sample-set size").  getSampleParam(index, dim, numSamples = M):
//     s = rng(rng(y W + x) + i) & (M - 1),  xi.x = s / M,  xi.y = (rng(s) & 0xffff) / 65536,
//     (cosPhi, sinPhi) = ((float)cos(phi), (float)sin(phi)),  phi = 2.0 * 3.14159265358979323846 * (double)s / (double)M
// with i = FrameIndex * N + k for sample k.  The path functions are those of tests/recursion_ref.cpp / tests/spp_ref.cpp once more, taking
// their angle from this file's own M-entry table instead of the oracle's.  Built by tests/restatement.py with the oracle Makefile's flags.
// At M = 256 it reproduces tests/spp_ref.cpp bit for bit (tests/test_sampleset_host.py); larger M pin the product's frames.
#include <mutex>

namespace orc {

struct SampleM { uint32_t s; float x, y, cosPhi, sinPhi; };
struct TableM { std::vector<float> cosTab, sinTab; };

// the M-entry table: the rule of the oracle's own (orc_capi.cpp orc_create) with M in place of 256; made once per size
static const TableM& table_m(uint32_t M) {
  static std::mutex lock; static TableM tables[17];
  uint32_t k = 0; while ((1u << k) < M) ++k;
  std::lock_guard<std::mutex> g(lock);
  TableM& t = tables[k];
  if (t.cosTab.size() != M) {
    t.cosTab.resize(M); t.sinTab.resize(M);
    for (uint32_t s = 0; s < M; ++s) { const double phi = 2.0 * 3.14159265358979323846 * (double)s / (double)M; t.cosTab[s] = (float)std::cos(phi); t.sinTab[s] = (float)std::sin(phi); }
  }
  return t;
}
static inline SampleM get_sample_param_m(const TableM& t, uint32_t px, uint32_t py, uint32_t W, uint32_t index, uint32_t M) {
  uint32_t s = py * W + px;
  s = rng(s); s += index; s = rng(s); s &= M - 1u;
  return {s, (float)s / (float)M, (float)(rng(s) & 0xffffu) / 65536.0f, t.cosTab[s], t.sinTab[s]};
}

// computeReflection's half vector and weight at any depth, computeDiffuse's direction: shared by level 0 and the path loop
static inline float3 half_vector_m(const Ctx& c, float3 N, float3 V, float a, const SampleM& xi) {
  if (c.vndf) return vndf_half_vector(N, V, a, xi.cosPhi, xi.sinPhi, xi.y);
  const float cosTheta = std::sqrt((1.0f - xi.y) / (1.0f + (a * a - 1.0f) * xi.y));
  const float sinTheta = std::sqrt(1.0f - cosTheta * cosTheta);
  return local_to_world(N, f3(xi.cosPhi * sinTheta, xi.sinPhi * sinTheta, cosTheta));
}
static inline float3 reflection_weight_m(const Ctx& c, float3 N, float3 V, float3 Hh, float NoL, float2 rm, float3 color) {
  const float a = rm.x * rm.x;
  const float3 f0 = f3(lerp(0.04f, color.x, rm.y), lerp(0.04f, color.y, rm.y), lerp(0.04f, color.z, rm.y));
  const float NoV = saturate(dot(N, V));
  const float VoH = saturate(dot(V, Hh));
  const float3 F = f_schlick(f0, VoH);
  const float vis = vis_smith(rm.x, NoV, NoL);
  const float NoH = saturate(dot(N, Hh));
  const float k = 4.0f * VoH / NoH;
  if (c.vndf) {
    const float a2 = a * a;
    const float g1l = (2.0f * NoL) / (NoL + std::sqrt(NoL * (NoL - NoL * a2) + a2));
    return f3(F.x * g1l, F.y * g1l, F.z * g1l);
  }
  return f3(((NoL * F.x) * vis) * k, ((NoL * F.y) * vis) * k, ((NoL * F.z) * vis) * k);   // :477
}
static inline float3 diffuse_direction_m(float3 N, const SampleM& xi) {
  const float cosTheta = 1.0f - 2.0f * xi.y;
  const float sinTheta = std::sqrt(1.0f - cosTheta * cosTheta);
  return normalize(N + f3(xi.cosPhi * sinTheta, xi.sinPhi * sinTheta, cosTheta));
}

// A path from its level-0 ray on (tests/recursion_ref.cpp follow_path): the value c at its end; T the throughput, multiplied forward.
static inline float3 follow_path_m(const Ctx& c, float3 o, float3 dir, uint32_t skipInst, uint32_t skipPrim, bool diffuseGroup, float3 preset,
                                   const SampleM& xi, uint32_t D, float3& T, uint32_t& rays) {
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
      const float3 Hh = half_vector_m(c, N, V, rm.x * rm.x, xi);
      L = reflect(-V, Hh);
      const float NoL = dot(N, L);
      if (NoL <= 0.0f) return f3(0, 0, 0);                                                  // :459
      w = reflection_weight_m(c, N, V, Hh, NoL, rm, color);
      diffuseGroup = false;
    } else {                                                                                 // computeDiffuse at depth d + 1
      if (diffuseGroup) color = color * (1.0f - rm.y);                                      // :607
      L = diffuse_direction_m(N, xi);
      w = color;                                                                             // no x (1 - 0.04) at depth >= 1 (:532)
      diffuseGroup = true;
    }
    preset = color * rm.y;
    T = f3(T.x * w.x, T.y * w.y, T.z * w.z);
    o = P; dir = L; skipInst = h.inst; skipPrim = h.prim;
  }
}

// tests/spp_ref.cpp raygen_pixel_spp with the sample taken from the set of M.  Returns the rays traced.
static inline uint32_t raygen_pixel_m(Ctx& c, const TableM& t, uint32_t px, uint32_t py, uint32_t D, uint32_t N, uint32_t M) {
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

  if (!s.hit) {      // background: the environment along -V into both images; no sample is taken
    const float3 e = environment(c, -s.V, 0.0f);
    c.refl[pix] = pack_r11g11b10f(e.x, e.y, e.z);
    c.diff[pix] = c.refl[pix];
    return 0;
  }
  const bool diffuse = s.rghMtl.y < 1.0f;
  float3 accR = f3(0, 0, 0), accD = f3(0, 0, 0);
  for (uint32_t k = 0; k < N; ++k) {
    const SampleM xi = get_sample_param_m(t, px, py, W, fc.g.FrameIndex * N + k, M);
    {  // the reflection path: level 0 is computeReflection at depth 0 (:424-484)
      const float3 Hh = half_vector_m(c, s.N, s.V, s.rghMtl.x * s.rghMtl.x, xi);
      const float3 R = reflect(-s.V, Hh);
      const float NoL = dot(s.N, R);
      float3 v = f3(0, 0, 0);
      if (NoL > 0.0f) {
        float3 T = reflection_weight_m(c, s.N, s.V, Hh, NoL, s.rghMtl, s.color);   // w0
        const float3 col = follow_path_m(c, s.P, R, s.inst, s.prim, false, s.color * s.rghMtl.y, xi, D, T, rays);
        v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      }
      accR = f3(accR.x + v.x, accR.y + v.y, accR.z + v.z);
    }
    if (diffuse) {   // the diffuse path: level 0 is computeDiffuse at depth 0 (:486-535)
      const float3 dir = diffuse_direction_m(s.N, xi);
      float3 T = s.color * (1.0f - 0.04f);                                                     // w0 (:532)
      const float3 col = follow_path_m(c, s.P, dir, s.inst, s.prim, true, s.color * s.rghMtl.y, xi, D, T, rays);
      const float3 v = f3(col.x * T.x, col.y * T.y, col.z * T.z);
      accD = f3(accD.x + v.x, accD.y + v.y, accD.z + v.z);
    }
  }
  const float scale = 1.0f / (float)N;
  c.refl[pix] = pack_r11g11b10f(accR.x * scale, accR.y * scale, accR.z * scale);
  if (diffuse) c.diff[pix] = pack_r11g11b10f(accD.x * scale, accD.y * scale, accD.z * scale);
  return rays;
}

}  // namespace orc

extern "C" uint64_t orc_ray_trace_sampleset(void* h, uint32_t depth, uint32_t samples, uint32_t M) {
  Ctx* c = (Ctx*)h;
  const TableM& t = table_m(M);
  std::atomic<uint64_t> rays{0};
  parallel_rows(c->threads, c->H, [&](uint32_t y) { uint64_t r = 0; for (uint32_t x = 0; x < c->W; ++x) r += raygen_pixel_m(*c, t, x, y, depth, samples, M); rays += r; });
  c->rayCount = rays.load();
  return c->rayCount;
}
// known answers: the sample of index `index` at pixel (x, y) of a frame W wide, from a set of M: its slot and (xi.x, xi.y)
extern "C" void orc_sample_param_m(uint32_t x, uint32_t y, uint32_t W, uint32_t index, uint32_t M, uint32_t* s, float* xi2) {
  const SampleM p = get_sample_param_m(table_m(M), x, y, W, index, M); *s = p.s; xi2[0] = p.x; xi2[1] = p.y;
}
// the M-entry table, interleaved {cos, sin}: 2 M floats
extern "C" void orc_sample_table_m(uint32_t M, float* cosSin) {
  const TableM& t = table_m(M);
  for (uint32_t s = 0; s < M; ++s) { cosSin[2 * s] = t.cosTab[s]; cosSin[2 * s + 1] = t.sinTab[s]; }
}
// distinct slots s a pixel visits over the indices [begin, end): W * H counts (the integer test of "& (M - 1) on the right word")
extern "C" void orc_distinct_slots_m(uint32_t W, uint32_t H, uint32_t begin, uint32_t end, uint32_t M, uint32_t* counts) {
  const TableM& t = table_m(M);
  std::vector<uint8_t> seen(M);
  for (uint32_t y = 0; y < H; ++y) for (uint32_t x = 0; x < W; ++x) {
    std::fill(seen.begin(), seen.end(), 0);
    uint32_t n = 0;
    for (uint32_t i = begin; i < end; ++i) { const uint32_t s = get_sample_param_m(t, x, y, W, i, M).s; n += !seen[s]; seen[s] = 1; }
    counts[(size_t)y * W + x] = n;
  }
}
