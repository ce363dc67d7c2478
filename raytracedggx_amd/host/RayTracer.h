// Host-side mirror of the reference's RayTracer (RayTracedGGX/Content/RayTracer.h:24-45): same
// public method names and argument meaning, minus the D3D12 handles.  Every method forwards to one
// entry point of librtggx (include/rtggx.h); the only arithmetic kept on the host is what the
// reference keeps there: the per-frame constants of UpdateFrame (RayTracer.cpp:250-305).
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "../../include/rtggx.h"
#include "XMath.h"

// XUSG::IncrementalHalton (declared RayTracedGGX/XUSG/Advanced/XUSGAdvanced.h:834; body in the
// closed XUSG.dll).  n-th call = (radical_inverse_2(n), radical_inverse_3(n)), accumulated
// incrementally in fp32 -- algorithm and known answers: SURVEY.md row H4 / Appendix F.
class HaltonSequence {
 public:
  void Next(float& x, float& y);
 private:
  uint32_t m_base2 = 0, m_base3 = 0;
  float m_x = 0.0f, m_y = 0.0f;
};

class RayTracer {
 public:
  enum MeshIndex : uint32_t { GROUND, MODEL_OBJ, NUM_MESH };
  static const uint8_t FrameCount = 3;

  RayTracer();
  virtual ~RayTracer();

  // Loads the mesh (OBJ) and the environment, creates the render targets and uploads everything.  posScale = (x, y, z, scale) of the
  // model instance.  The environment is told by the file's first bytes: "DDS " a cube with its mip chain (rtggx_set_env), "#?" a Radiance
  // .hdr and "PF" a .pfm image (EnvImageLoader.h, rtggx_set_env_image) -- read, and a bad one refused, before anything touches a GPU.
  bool Init(uint32_t width, uint32_t height, const char* fileName, const char* envFileName,
            const float posScale[4], int device = 0);
  // What Init does with the environment file (-envlayout, -envsize, -envmips); to be called before it.  layout: RTGGX_ENV_* or -1 = by the
  // image's aspect ratio (3:4 vertical cross, 4:3 horizontal cross, 2:1 panorama; anything else is refused).  cubeSize: the cube's side for a
  // panorama (0: the largest power of two <= width / 4); refused with a cross, whose cells are the faces.  generateMips: a DDS cube with
  // fewer levels than a full chain gets the chain built on the device (rtggx_generate_env_mips).  prefilterSamples: 0 = off, else the sample
  // count (a power of two from 64 to 4096) with which Init, once the environment is installed -- DDS cube or image --, rebuilds the levels
  // below level 0 as the GGX-prefiltered radiance (-envprefilter, rtggx_prefilter_env); it builds the full chain itself, generateMips or not.
  void SetEnvOptions(int layout, uint32_t cubeSize, bool generateMips, uint32_t prefilterSamples = 0) { m_envLayout = layout; m_envCubeSize = cubeSize; m_envGenerateMips = generateMips; m_envPrefilterSamples = prefilterSamples; }
  // rtggx_prefilter_env on the current environment: samples 0 = 1024, else a power of two from 64 to 4096; a refusal leaves it as it was
  bool PrefilterEnvironment(uint32_t samples);
  // rtggx_sun_from_env on the current environment: the sun's direction and irradiance measured from the cube (cone, ring in degrees and
  // minContrast: 0 = the library's defaults) and, with remove, the sun cut out of the cube and its box chain rebuilt.  estimate.found says
  // whether there is one; a refusal leaves everything as it was.
  bool SunFromEnvironment(float cone, float ring, float minContrast, bool remove, RtggxSunEstimate& estimate);
  // -sunfromenv [degrees]: Init, once the -env file is loaded and -envmips has had its turn, takes the sun out of the cube
  // (SunFromEnvironment with remove), THEN prefilters (-envprefilter sees the sunless cube) and sets the measured sun (SetSun); where no sun
  // is found it says so in one line and goes on without one.  To be called before Init; coneDegrees 0 = the library's default.
  void SetSunFromEnvironment(bool enable, float coneDegrees = 0.0f) { m_sunFromEnv = enable; m_sunFromEnvCone = coneDegrees; }
  bool BuildAccelerationStructures();
  bool Postinit();

  void SetMetallic(uint32_t meshIdx, float metallic);
  // m_asyncCompute of the sample (RayTracedGGX.h:118): true = the multi-stream frame (its two queues), false = one stream in
  // submission order (its single command list, RayTracedGGX.cpp:513-556)
  void SetAsyncCompute(bool asyncCompute);
  void SetSampler(bool vndf);            // rtggx_set_sampler: visible-normal (Heitz 2018) sampling of the reflection lobe, opt-in (-vndf)
  bool SetRayRate(uint32_t pixelsPerRay);
  // A directional light with ray-traced shadows from the next frame on (rtggx_set_sun): dir toward the sun, e its irradiance; (nullptr, nullptr): off.
  bool SetSun(const float dir[3], const float e[3]);
  // The sun term and the shadow at the surfaces seen in reflections as well (rtggx_set_sun_reflections); it acts only while a sun is set.
  bool SetSunReflections(bool enable);
  // The angular radius of the sun's disk in degrees, 0 to RTGGX_MAX_SUN_ANGLE_DEGREES (rtggx_set_sun_angle): shadow rays toward a point of
  // the disk, a penumbra.  0: the directional sun.  It acts only while a sun is set.
  bool SetSunAngle(float degrees);
  // Point and spot lights inside the scene with ray-traced shadows from the next frame on (rtggx_set_lights): up to RTGGX_MAX_LIGHTS, copied;
  // (nullptr, 0): off.
  bool SetLights(const RtggxLight* lights, uint32_t count);
  // The lights' terms and shadows at the surfaces seen in reflections as well (rtggx_set_light_reflections); it acts only while lights are set.
  bool SetLightReflections(bool enable);
  // One shadow ray per surface point for all lights (rtggx_set_light_sampling): 0 a ray per light (default), 1 one light picked per point; it
  // acts only while lights are set.
  bool SetLightSampling(int mode);
  // The pick of mode 1 weighted by the visibility each pixel remembers per light (rtggx_set_light_pick_visibility); it acts only in mode 1
  // while a light casts rays; whole frames only.
  bool SetLightPickVisibility(bool enable);
  // A list of up to RTGGX_MAX_LIGHT_LIST lights under mode 1's rule, culled per 8x8 block, from the next frame on (rtggx_set_light_list):
  // copied; (nullptr, 0) clears it.  In place of SetLights, not beside it.
  bool SetLightList(const RtggxLight* lights, uint32_t count);
  // The list's pick weighted by the sparse record each pixel keeps of the lights it found hidden (rtggx_set_light_list_visibility); it acts
  // only on a list while a light casts rays; whole frames only.
  bool SetLightListVisibility(bool enable);
  // Lights first .. first + count - 1 of the list replaced from the next frame on, without a wait and without a reset of the records'
  // history: from a host array, checked and copied (rtggx_update_light_list), or from device memory in the order of `stream`, checked on
  // the device (rtggx_update_light_list_device; kinds: RTGGX_LIGHT_KIND_*).  ReadLightList: the list the last frame read, as the kernels
  // see it (rtggx_read_light_list; synchronises).
  bool UpdateLightList(const RtggxLight* lights, uint32_t first, uint32_t count);
  bool UpdateLightListDevice(const RtggxLight* deviceLights, uint32_t first, uint32_t count, uint32_t kinds, void* stream);
  bool ReadLightList(RtggxLight* out, size_t bytes);
  bool SetSamplesPerPixel(uint32_t samples);   // rtggx_set_samples_per_pixel: 1 (default), 2, 4 or 8 samples per covered pixel (-spp); not together with ray rate 4
  bool SetMaxRecursionDepth(uint32_t depth);   // rtggx_set_max_recursion_depth: 1 (default; RayTracer.cpp:605 SetMaxRecursionDepth(1)) to 4 levels of rays per path (-recursion)   // rtggx_set_ray_rate: 1 (default) or 4 -- one pixel of each 2x2 quad traced per frame, the rest reconstructed (-rayrate)
  // rtggx_set_sample_set: the size of the sample set getSampleParam draws from, 256 (default, the reference's) or a power of two up to
  // 65536 (-sampleset); UpdateFrame's frame index counts modulo it.  A refused size leaves both as they were.
  bool SetSampleSetSize(uint32_t size);
  uint32_t GetSampleSetSize() const { return m_sampleSet; }
  // rtggx_set_accumulation / rtggx_reset_accumulation: the running sums of the raw traced images, on from the next frame (-accumulate);
  // not together with ray rate 4.  A moving camera or a changed material is the caller's to reset.
  bool SetAccumulation(bool enable);
  bool ResetAccumulation();
  // rtggx_set_sample_map / rtggx_read_sample_map: how many of the N samples each 8 x 8 block of the full frame traces -- ceil(W / 8) x
  // ceil(H / 8) counts of 1, 2, 4 or 8, row-major; nullptr, 0, 0 clears the map --, and the map most recently set read back (empty: none).
  // Whole frames only; each call synchronises.
  bool SetSampleMap(const uint8_t* counts, uint32_t blocksX, uint32_t blocksY);
  bool ReadSampleMap(std::vector<uint8_t>& counts, uint32_t& blocksX, uint32_t& blocksY);
  // rtggx_set_reference / rtggx_set_scoring / rtggx_read_scores: the image every frame is scored against on the device (W * H RGBA16F
  // words; nullptr, 0 releases it), scoring on from the next frame (refused without a reference), and the records not yet read, oldest
  // first, appended to `out` -- it waits for the main stream alone (-reference, -score)
  bool SetReference(const void* rgba16f, size_t bytes);
  bool SetScoring(bool enable);
  bool ReadScores(std::vector<RtggxScore>& out);
  void UpdateFrame(uint8_t frameIndex, const xm::Float3& eyePt, const xm::Matrix& viewProj, float timeStep);
  void TransformSH();
  void Render(uint8_t frameIndex);
  void UpdateAccelerationStructure(uint8_t frameIndex);
  // Deforming model: new vertices {Pos, Nrm} for the unchanged topology of the loaded mesh.  The acceleration
  // structure is refitted on the device at the start of the next frame, asynchronously (rtggx_refit_as).
  bool UpdateMesh(const float* vertices, uint32_t numVertices);
  const std::vector<float>& GetModelVertices() const { return m_modelVerts; }       // as imported: 6 floats per vertex
  void RenderVisibility(uint8_t frameIndex, bool asyncCompute = false);
  void RayTrace(uint8_t frameIndex);

  rtggx_context* GetContext() const { return m_ctx; }
  const RtggxFrameConstants& GetFrameConstants() const { return m_constants; }
  uint32_t GetNumModelVertices() const { return m_numVerts; }
  uint32_t GetNumModelIndices() const { return m_numIndices; }
  const std::string& GetLastError() const { return m_error; }

 protected:
  bool check(int rc, const char* what);

  rtggx_context* m_ctx = nullptr;
  uint32_t m_width = 0, m_height = 0;
  float m_posScale[4] = {0.0f, 0.0f, 0.0f, 1.0f};
  uint32_t m_numVerts = 0, m_numIndices = 0;
  std::vector<float> m_modelVerts;
  int m_envLayout = -1; uint32_t m_envCubeSize = 0; bool m_envGenerateMips = false; uint32_t m_envPrefilterSamples = 0;      // SetEnvOptions
  bool m_sunFromEnv = false; float m_sunFromEnvCone = 0.0f;      // SetSunFromEnvironment

  // state UpdateFrame keeps between frames (statics / members in the reference)
  HaltonSequence m_halton;
  float m_angle = 0.0f;            // RayTracer.cpp:270
  uint32_t m_frameCounter = 0;     // s_frameIndex, RayTracer.cpp:282
  uint32_t m_sampleSet = RTGGX_MIN_SAMPLE_SET;      // const auto n = 256u beside it
  bool m_hasPrev = false;
  float m_worldViewProjs[NUM_MESH][16];   // RayTracer.h:131
  RtggxFrameConstants m_constants{};
  std::string m_error;
};
