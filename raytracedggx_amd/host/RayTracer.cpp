#include "RayTracer.h"

#include <cstdio>
#include <cstring>

#include "DDSLoader.h"
#include "EnvImageLoader.h"
#include "ObjLoader.h"

void HaltonSequence::Next(float& x, float& y) {
  // base 2: the bits that change between n and n+1 are flipped from the least significant one
  uint32_t before = m_base2;
  uint32_t changed = before ^ (m_base2 + 1);
  ++m_base2;
  for (float step = 0.5f; changed; step *= 0.5f, changed >>= 1, before >>= 1) m_x += (before & 1u) ? -step : step;
  // base 3: two bits per ternary digit; a digit that reaches 3 wraps to 0 and carries
  ++m_base3;
  uint32_t digitMask = 0x3u, digitOne = 0x1u;
  float step = 1.0f / 3.0f;
  while ((m_base3 & digitMask) == digitMask) {
    m_base3 += digitOne;
    m_y += -2.0f * step;
    digitMask <<= 2; digitOne <<= 2; step *= 1.0f / 3.0f;
  }
  m_y += step;
  x = m_x; y = m_y;
}

RayTracer::RayTracer() { std::memset(m_worldViewProjs, 0, sizeof m_worldViewProjs); }

RayTracer::~RayTracer() { if (m_ctx) rtggx_destroy(m_ctx); }

bool RayTracer::check(int rc, const char* what) {
  if (rc == 0) return true;
  m_error = std::string(what) + ": " + rtggx_last_error();
  std::fprintf(stderr, "RayTracer: %s\n", m_error.c_str());
  return false;
}

bool RayTracer::Init(uint32_t width, uint32_t height, const char* fileName, const char* envFileName,
                     const float posScale[4], int device) {
  m_width = width; m_height = height;
  std::memcpy(m_posScale, posScale, sizeof m_posScale);
  const auto fail = [&](const std::string& why) { m_error = why; std::fprintf(stderr, "RayTracer: %s\n", why.c_str()); return false; };

  // The environment file, by its first bytes: read and checked on the host before a device is asked for
  DDS::CubeImage cube;
  EnvImage::Image image;
  int layout = m_envLayout;
  bool isImage = false;
  {
    uint8_t magic[4] = {0, 0, 0, 0};
    FILE* f = std::fopen(envFileName, "rb");
    if (!f) return fail(std::string("cannot open ") + envFileName);
    const size_t got = std::fread(magic, 1, 4, f);
    std::fclose(f);
    isImage = EnvImage::IsRadiance(magic, got) || EnvImage::IsPfm(magic, got);
  }
  std::string err;
  if (isImage) {
    if (!EnvImage::LoadFromFile(envFileName, image, err)) return fail(err);
    if (layout < 0) layout = EnvImage::LayoutFromAspect(image.width, image.height);
    if (layout < 0) return fail(std::string(envFileName) + ": " + std::to_string(image.width) + " x " + std::to_string(image.height) + " pixels are neither 3:4 (vertical cross), 4:3 (horizontal cross) nor 2:1 (panorama): name the layout with -envlayout equirect|vcross|hcross");
    if (layout != EnvImage::EQUIRECT && m_envCubeSize != 0u) return fail("-envsize: a cross is never resampled, its cells are the cube's faces (" + std::string(envFileName) + " is a " + (layout == EnvImage::VCROSS ? "vertical" : "horizontal") + " cross)");
    if (m_envGenerateMips && m_envPrefilterSamples == 0u) std::fprintf(stderr, "RayTracer: -envmips has no effect on %s: an image always gets its full mip chain\n", envFileName);
  } else {
    if (!DDS::Loader().LoadCubeFromFile(envFileName, cube, err)) return fail(err);      // (RayTracer.cpp:143-150)
    if (m_envLayout >= 0 || m_envCubeSize != 0u) std::fprintf(stderr, "RayTracer: -envlayout / -envsize have no effect on %s: a DDS cube is taken as it is\n", envFileName);
  }

  if (!check(rtggx_create(&m_ctx, width, height, device), "rtggx_create")) return false;   // render targets + ground mesh + materials

  // Load inputs (RayTracer.cpp:83-86)
  ObjLoader objLoader;
  if (!objLoader.Import(fileName, true, true)) return fail(std::string("cannot import ") + fileName);
  m_numVerts = objLoader.GetNumVertices(); m_numIndices = objLoader.GetNumIndices();
  m_modelVerts.assign(reinterpret_cast<const float*>(objLoader.GetVertices()), reinterpret_cast<const float*>(objLoader.GetVertices()) + 6 * (size_t)m_numVerts);
  if (!check(rtggx_set_mesh(m_ctx, MODEL_OBJ, reinterpret_cast<const float*>(objLoader.GetVertices()), m_numVerts,
                            objLoader.GetIndices(), m_numIndices), "rtggx_set_mesh")) return false;

  if (isImage) {
    if (!check(rtggx_set_env_image(m_ctx, layout, image.pixels, image.width, image.height, image.data.data(), image.data.size(), m_envCubeSize), "rtggx_set_env_image")) return false;
  } else {
    if (!check(rtggx_set_env(m_ctx, cube.format, cube.size, cube.mips, cube.payload.data(), cube.payload.size()), "rtggx_set_env")) return false;
    uint32_t full = 1; while ((cube.size >> full) != 0u) ++full;
    // (the prefilter starts from the full box chain below the current level 0 whatever levels the cube came with: it implies -envmips)
    if (m_envGenerateMips && m_envPrefilterSamples == 0u && cube.mips < full && !check(rtggx_generate_env_mips(m_ctx), "rtggx_generate_env_mips")) return false;
  }
  // -sunfromenv: the sun leaves the cube before the prefilter smears it over the rough levels, and comes back as a light with shadows
  RtggxSunEstimate sun{};
  if (m_sunFromEnv && !SunFromEnvironment(m_sunFromEnvCone, 0.0f, 0.0f, true, sun)) return false;
  if (m_envPrefilterSamples != 0u && !PrefilterEnvironment(m_envPrefilterSamples)) return false;
  if (m_sunFromEnv) {
    if (!sun.found) std::printf("-sunfromenv: no sun in %s (peak luminance %g against a mean of %g): rendering without one\n", envFileName, sun.peak_luma, sun.mean_luma);
    else {
      std::printf("-sunfromenv: sun toward (%.9g %.9g %.9g), irradiance (%.9g %.9g %.9g), %u texels cut down in %s\n", sun.direction[0], sun.direction[1], sun.direction[2],
                  sun.irradiance[0], sun.irradiance[1], sun.irradiance[2], sun.texels_lit, envFileName);
      if (!SetSun(sun.direction, sun.irradiance)) return false;
    }
  }
  return true;
}

bool RayTracer::PrefilterEnvironment(uint32_t samples) { return check(rtggx_prefilter_env(m_ctx, samples), "rtggx_prefilter_env"); }
bool RayTracer::SunFromEnvironment(float cone, float ring, float minContrast, bool remove, RtggxSunEstimate& estimate) {
  return check(rtggx_sun_from_env(m_ctx, cone, ring, minContrast, remove ? 1 : 0, &estimate), "rtggx_sun_from_env");
}

bool RayTracer::BuildAccelerationStructures() { return check(rtggx_build_as(m_ctx), "rtggx_build_as"); }

bool RayTracer::Postinit() { return check(rtggx_sync(m_ctx), "rtggx_sync"); }

void RayTracer::SetMetallic(uint32_t meshIdx, float metallic) { check(rtggx_set_metallic(m_ctx, meshIdx, metallic), "rtggx_set_metallic"); }

void RayTracer::SetSampler(bool vndf) { check(rtggx_set_sampler(m_ctx, vndf ? 1 : 0), "rtggx_set_sampler"); }

bool RayTracer::SetRayRate(uint32_t pixelsPerRay) { return check(rtggx_set_ray_rate(m_ctx, pixelsPerRay), "rtggx_set_ray_rate"); }
bool RayTracer::SetSun(const float dir[3], const float e[3]) { return check(rtggx_set_sun(m_ctx, dir, e), "rtggx_set_sun"); }
bool RayTracer::SetSunAngle(float degrees) { return check(rtggx_set_sun_angle(m_ctx, degrees), "rtggx_set_sun_angle"); }
bool RayTracer::SetLights(const RtggxLight* lights, uint32_t count) { return check(rtggx_set_lights(m_ctx, lights, count), "rtggx_set_lights"); }
bool RayTracer::SetLightReflections(bool enable) { return check(rtggx_set_light_reflections(m_ctx, enable ? 1 : 0), "rtggx_set_light_reflections"); }
bool RayTracer::SetLightList(const RtggxLight* lights, uint32_t count) { return check(rtggx_set_light_list(m_ctx, lights, count), "rtggx_set_light_list"); }
bool RayTracer::SetLightSampling(int mode) { return check(rtggx_set_light_sampling(m_ctx, mode), "rtggx_set_light_sampling"); }
bool RayTracer::SetLightListVisibility(bool enable) { return check(rtggx_set_light_list_visibility(m_ctx, enable ? 1 : 0), "rtggx_set_light_list_visibility"); }
bool RayTracer::UpdateLightList(const RtggxLight* lights, uint32_t first, uint32_t count) { return check(rtggx_update_light_list(m_ctx, lights, first, count), "rtggx_update_light_list"); }
bool RayTracer::UpdateLightListDevice(const RtggxLight* deviceLights, uint32_t first, uint32_t count, uint32_t kinds, void* stream) { return check(rtggx_update_light_list_device(m_ctx, deviceLights, first, count, kinds, stream), "rtggx_update_light_list_device"); }
bool RayTracer::ReadLightList(RtggxLight* out, size_t bytes) { return check(rtggx_read_light_list(m_ctx, out, bytes), "rtggx_read_light_list"); }
bool RayTracer::SetLightPickVisibility(bool enable) { return check(rtggx_set_light_pick_visibility(m_ctx, enable ? 1 : 0), "rtggx_set_light_pick_visibility"); }
bool RayTracer::SetSunReflections(bool enable) { return check(rtggx_set_sun_reflections(m_ctx, enable ? 1 : 0), "rtggx_set_sun_reflections"); }

bool RayTracer::SetSamplesPerPixel(uint32_t samples) { return check(rtggx_set_samples_per_pixel(m_ctx, samples), "rtggx_set_samples_per_pixel"); }
bool RayTracer::SetMaxRecursionDepth(uint32_t depth) { return check(rtggx_set_max_recursion_depth(m_ctx, depth), "rtggx_set_max_recursion_depth"); }

bool RayTracer::SetSampleSetSize(uint32_t size) {
  // (without a context -- constants only -- the rule is rtggx_set_sample_set's own)
  if (!m_ctx && (size < RTGGX_MIN_SAMPLE_SET || size > RTGGX_MAX_SAMPLE_SET || (size & (size - 1u)) != 0u)) { m_error = "SetSampleSetSize: a power of two from 256 to 65536"; return false; }
  if (m_ctx && !check(rtggx_set_sample_set(m_ctx, size), "rtggx_set_sample_set")) return false;
  m_sampleSet = size;      // UpdateFrame counts modulo it from here on
  m_frameCounter %= m_sampleSet;
  return true;
}

bool RayTracer::SetAccumulation(bool enable) { return check(rtggx_set_accumulation(m_ctx, enable ? 1 : 0), "rtggx_set_accumulation"); }
bool RayTracer::ResetAccumulation() { return check(rtggx_reset_accumulation(m_ctx), "rtggx_reset_accumulation"); }

bool RayTracer::SetSampleMap(const uint8_t* counts, uint32_t blocksX, uint32_t blocksY) { return check(rtggx_set_sample_map(m_ctx, counts, blocksX, blocksY), "rtggx_set_sample_map"); }
bool RayTracer::ReadSampleMap(std::vector<uint8_t>& counts, uint32_t& blocksX, uint32_t& blocksY) {
  counts.assign((size_t)((m_width + 7u) / 8u) * ((m_height + 7u) / 8u), 0);
  if (!check(rtggx_read_sample_map(m_ctx, counts.data(), (uint32_t)counts.size(), &blocksX, &blocksY), "rtggx_read_sample_map")) return false;
  counts.resize((size_t)blocksX * blocksY);
  return true;
}

bool RayTracer::SetReference(const void* rgba16f, size_t bytes) { return check(rtggx_set_reference(m_ctx, rgba16f, bytes), "rtggx_set_reference"); }
bool RayTracer::SetScoring(bool enable) { return check(rtggx_set_scoring(m_ctx, enable ? 1 : 0), "rtggx_set_scoring"); }
bool RayTracer::ReadScores(std::vector<RtggxScore>& out) {
  for (;;) {      // a ring's worth at a time until nothing is left unread
    const size_t have = out.size();
    out.resize(have + RTGGX_SCORE_RING);
    uint32_t n = 0;
    const bool ok = check(rtggx_read_scores(m_ctx, out.data() + have, RTGGX_SCORE_RING, &n), "rtggx_read_scores");
    out.resize(have + (ok ? n : 0u));
    if (!ok) return false;
    if (n < (uint32_t)RTGGX_SCORE_RING) return true;
  }
}

void RayTracer::SetAsyncCompute(bool asyncCompute) { check(rtggx_set_async_compute(m_ctx, asyncCompute ? 1 : 0), "rtggx_set_async_compute"); }

void RayTracer::UpdateFrame(uint8_t frameIndex, const xm::Float3& eyePt, const xm::Matrix& viewProj, float timeStep) {
  (void)frameIndex;   // the constant-buffer slot ring lives inside librtggx
  using namespace xm;
  float hx, hy;
  m_halton.Next(hx, hy);
  const float projBias[2] = {(hx * 2.0f - 1.0f) / (float)m_width, (hy * 2.0f - 1.0f) / (float)m_height};

  RtggxFrameConstants& cb = m_constants;
  {
    const Matrix projToWorld = Inverse(viewProj);
    StoreFloat4x4(cb.rayGen.ProjToWorld, Transpose(projToWorld));
    cb.rayGen.EyePt[0] = eyePt.x; cb.rayGen.EyePt[1] = eyePt.y; cb.rayGen.EyePt[2] = eyePt.z; cb.rayGen.EyePt[3] = 0.0f;
    cb.rayGen.ProjBias[0] = projBias[0]; cb.rayGen.ProjBias[1] = projBias[1];
    cb.rayGen.pad[0] = cb.rayGen.pad[1] = 0.0f;
  }
  {
    m_angle += 16.0f * timeStep * 3.141592654f / 180.0f;
    const Matrix rot = RotationY(m_angle);
    const Matrix worlds[NUM_MESH] = {
      Scaling(10.0f, 0.5f, 10.0f) * Translation(0.0f, -0.5f, 0.0f),
      Scaling(m_posScale[3], m_posScale[3], m_posScale[3]) * rot * Translation(m_posScale[0], m_posScale[1], m_posScale[2])};
    for (uint32_t i = 0; i < NUM_MESH; ++i) {
      float wvp[16];
      StoreFloat4x4(wvp, Transpose(worlds[i] * viewProj));
      // m_worldViewProjs is never initialised by the reference's constructor; first frame: prev = current
      std::memcpy(cb.global.WorldViewProjsPrev[i], m_hasPrev ? m_worldViewProjs[i] : wvp, 64);
      std::memcpy(cb.global.WorldViewProjs[i], wvp, 64);
      StoreFloat3x4(cb.global.Worlds[i], worlds[i]);
      std::memcpy(m_worldViewProjs[i], wvp, 64);
      std::memcpy(cb.perObject[i].WorldViewProj, wvp, 64);
      cb.perObject[i].ProjBias[0] = projBias[0]; cb.perObject[i].ProjBias[1] = projBias[1];
      cb.perObject[i].pad[0] = cb.perObject[i].pad[1] = 0.0f;
    }
    StoreFloat3x4(cb.global.WorldITs0, Identity());
    StoreFloat3x4(cb.global.WorldIT1, rot, 11);
    m_hasPrev = true;
    cb.global.FrameIndex = m_frameCounter++;
    m_frameCounter %= m_sampleSet;      // n = 256 beside s_frameIndex (RayTracer.cpp:282), a setting here: the size of the sample set
  }
  std::memset(&cb.material, 0, sizeof cb.material);   // CBMaterial is persistent on the device (rtggx_set_material)
  if (m_ctx) check(rtggx_update_frame(m_ctx, &cb), "rtggx_update_frame");
}

void RayTracer::TransformSH() { check(rtggx_transform_sh(m_ctx), "rtggx_transform_sh"); }

void RayTracer::Render(uint8_t frameIndex) {
  RenderVisibility(frameIndex);
  check(rtggx_ray_trace(m_ctx), "rtggx_ray_trace");
}

bool RayTracer::UpdateMesh(const float* vertices, uint32_t numVertices) { return check(rtggx_refit_as(m_ctx, MODEL_OBJ, vertices, numVertices), "rtggx_refit_as"); }

void RayTracer::UpdateAccelerationStructure(uint8_t) { check(rtggx_update_as(m_ctx), "rtggx_update_as"); }

void RayTracer::RenderVisibility(uint8_t, bool) { check(rtggx_render_visibility(m_ctx), "rtggx_render_visibility"); }

void RayTracer::RayTrace(uint8_t) { check(rtggx_ray_trace(m_ctx), "rtggx_ray_trace"); }
