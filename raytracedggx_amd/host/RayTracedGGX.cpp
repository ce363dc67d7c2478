#include <cmath>
#include <cstring>
#include "RayTracedGGX.h"
#include "EnvImageLoader.h"

#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#define PIDIV4 0.785398163f

static const float g_FOVAngleY = PIDIV4;   // RayTracedGGX.cpp:19-23
static const float g_zNear = 1.0f;
static const float g_zFar = 1000.0f;

RayTracedGGX::RayTracedGGX(uint32_t width, uint32_t height, std::string name) : m_width(width), m_height(height), m_title(std::move(name)) {
  for (auto& metallic : m_metallics) metallic = 1.0f;   // RayTracedGGX.cpp:51
}

RayTracedGGX::~RayTracedGGX() {}

// LoadPipeline + LoadAssets (RayTracedGGX.cpp:61-279)
void RayTracedGGX::OnInit() {
  m_rayTracer = std::make_unique<RayTracer>();
  m_rayTracer->SetEnvOptions(m_envLayout, m_envSize, m_envMips, m_envPrefilter);      // -envlayout, -envsize, -envmips, -envprefilter: what Init does with the -env file
  m_rayTracer->SetSunFromEnvironment(m_sunFromEnv, m_sunFromEnvCone);                  // -sunfromenv: ... and the sun it finds there (opt-in)
  if (!m_rayTracer->Init(m_width, m_height, m_meshFileName.c_str(), m_envFileName.c_str(), m_meshPosScale, m_device))
    throw std::runtime_error("RayTracer::Init failed: " + m_rayTracer->GetLastError());
  m_denoiser = std::make_unique<Denoiser>();
  if (!m_denoiser->Init(m_rayTracer->GetContext(), m_width, m_height)) throw std::runtime_error("Denoiser::Init failed");
  if (!m_rayTracer->BuildAccelerationStructures()) throw std::runtime_error("BuildAccelerationStructures failed: " + m_rayTracer->GetLastError());
  if (!m_rayTracer->Postinit()) throw std::runtime_error("Postinit failed");
  if (m_hasMetallicOverride) for (uint32_t i = 0; i < RayTracer::NUM_MESH; ++i) m_rayTracer->SetMetallic(i, m_metallics[i]);
  if (m_vndf) m_rayTracer->SetSampler(true);            // -vndf: visible-normal sampling of the reflection lobe (opt-in; the reference samples the NDF)
  if (m_rayRate != 1u && !m_rayTracer->SetRayRate(m_rayRate)) throw std::runtime_error("-rayrate: " + m_rayTracer->GetLastError());      // -rayrate 4: one ray per 2x2 quad (opt-in)
  if (m_hasSun && !m_rayTracer->SetSun(m_sun, m_sun + 3)) throw std::runtime_error("-sun: " + m_rayTracer->GetLastError());      // -sun: a directional light with ray-traced shadows (opt-in)
  if (m_sunReflections && !m_rayTracer->SetSunReflections(true)) throw std::runtime_error("-sunreflections: " + m_rayTracer->GetLastError());      // -sunreflections: ... at the surfaces the paths hit as well (opt-in)
  if (!m_lights.empty() && !m_rayTracer->SetLights(m_lights.data(), (uint32_t)m_lights.size())) throw std::runtime_error("-light / -spot: " + m_rayTracer->GetLastError());      // -light, -spot: local lights with ray-traced shadows (opt-in)
  if (!m_lightList.empty() && !m_rayTracer->SetLightList(m_lightList.data(), (uint32_t)m_lightList.size())) throw std::runtime_error("-lightlist: " + m_rayTracer->GetLastError());      // -lightlist: a light list beyond eight, one shadow ray per point (opt-in)
  if (m_lightReflections && !m_rayTracer->SetLightReflections(true)) throw std::runtime_error("-lightreflections: " + m_rayTracer->GetLastError());      // -lightreflections: ... at the surfaces the paths hit as well (opt-in)
  if (m_lightPick && !m_rayTracer->SetLightSampling(1)) throw std::runtime_error("-lightpick: " + m_rayTracer->GetLastError());      // -lightpick: one shadow ray per surface point for all lights (opt-in)
  if (m_lightListVisibility && !m_rayTracer->SetLightListVisibility(true)) throw std::runtime_error("-lightlistvisibility: " + m_rayTracer->GetLastError());      // -lightlistvisibility: the list's pick weighted by what the pixel remembers (opt-in)
  if (m_lightVisibility && !m_rayTracer->SetLightPickVisibility(true)) throw std::runtime_error("-lightvisibility: " + m_rayTracer->GetLastError());      // -lightvisibility: the pick weighted by what the pixel remembers (opt-in)
  if (m_sunAngle != 0.0f && !m_rayTracer->SetSunAngle(m_sunAngle)) throw std::runtime_error("-sunangle: " + m_rayTracer->GetLastError());      // -sunangle: a sun with a size, soft shadows (opt-in)
  if (m_recursionDepth != 1u && !m_rayTracer->SetMaxRecursionDepth(m_recursionDepth)) throw std::runtime_error("-recursion: " + m_rayTracer->GetLastError());      // -recursion N: multi-bounce paths (opt-in)
  if (m_samplesPerPixel != 1u && !m_rayTracer->SetSamplesPerPixel(m_samplesPerPixel)) throw std::runtime_error("-spp: " + m_rayTracer->GetLastError());      // -spp N: multi-sample tracing (opt-in)
  if (m_sampleSet != RTGGX_MIN_SAMPLE_SET && !m_rayTracer->SetSampleSetSize(m_sampleSet)) throw std::runtime_error("-sampleset: " + m_rayTracer->GetLastError());      // -sampleset M: a larger sample set (opt-in)
  m_rayTracer->SetAsyncCompute(m_asyncCompute != 0);   // -sync: one stream, submission order (the sample's single command list)
  // -reference: the image read while the command line was parsed goes to the device; -score: every frame from the first one is scored
  if (!m_referenceImage.empty() && !m_rayTracer->SetReference(m_referenceImage.data(), m_referenceImage.size() * 2)) throw std::runtime_error("-reference: " + m_rayTracer->GetLastError());
  if (!m_scoreFile.empty() && !m_rayTracer->SetScoring(true)) throw std::runtime_error("-score: " + m_rayTracer->GetLastError());

  if (m_deformAmplitude != 0.0f) {       // key shapes of the breathing model: x and z displaced by a wave travelling up the y axis
    const std::vector<float>& base = m_rayTracer->GetModelVertices();
    m_deformShapes.assign(DeformPeriod, base);
    for (uint32_t k = 0; k < DeformPeriod; ++k) {
      const float phase = 6.283185307f * (float)k / (float)DeformPeriod;
      for (size_t v = 0; v + 5 < base.size(); v += 6) {
        const float y = base[v + 1];
        m_deformShapes[k][v] = base[v] + m_deformAmplitude * std::sin(1.3f * y + phase);
        m_deformShapes[k][v + 2] = base[v + 2] + 0.7f * m_deformAmplitude * std::cos(0.8f * y - phase);
      }
    }
  }
  InitCamera();
  if (!m_trackFileName.empty() && !LoadTrack(m_trackFileName)) throw std::runtime_error("cannot read track " + m_trackFileName);
  m_initialized = true;
}

// Projection and view (RayTracedGGX.cpp:262-277)
void RayTracedGGX::InitCamera() {
  const float aspectRatio = (float)m_width / (float)m_height;
  m_proj = xm::PerspectiveFovLH(g_FOVAngleY, aspectRatio, g_zNear, g_zFar);
  m_focusPt = {0.0f, 3.0f, 0.0f};
  m_eyePt = {10.0f, 10.0f, -24.0f};
  m_view = xm::LookAtLH(m_eyePt, m_focusPt, xm::Float3{0.0f, 1.0f, 0.0f});
}

// RayTracedGGX.cpp:282-299
void RayTracedGGX::OnUpdate() {
  for (; m_trackNext < m_track.size() && m_track[m_trackNext].frame <= m_frameNumber; ++m_trackNext) {
    const TrackEvent& e = m_track[m_trackNext];
    switch (e.type) {
      case 0: OnKeyUp((uint8_t)e.a); break;
      case 1: OnLButtonDown(e.a, e.b); break;
      case 2: OnLButtonUp(e.a, e.b); break;
      case 3: OnMouseMove(e.a, e.b); break;
      case 4: OnMouseWheel(e.a, 0.0f, 0.0f); break;
      default: OnMouseLeave(); break;
    }
  }
  // -accumulate N: on from the frame that leaves N frames of the run (from the first one when the run is no longer than N)
  if (m_accumulate != 0u && m_frameNumber == (m_numFrames > m_accumulate ? m_numFrames - m_accumulate : 0u) && !m_rayTracer->SetAccumulation(true))
    throw std::runtime_error("-accumulate: " + m_rayTracer->GetLastError());
  if (!m_deformShapes.empty() && !m_isPaused) {
    const std::vector<float>& shape = m_deformShapes[m_frameNumber % DeformPeriod];
    m_rayTracer->UpdateMesh(shape.data(), (uint32_t)(shape.size() / 6));
  }
  // -lightlistorbit d: before frame n every position and spot axis of the FILE's list turned about the world y axis by n d degrees --
  // x' = x cos a + z sin a, z' = z cos a - x sin a, from the originals in double and rounded once, so nothing drifts --, handed over
  // without a wait and without a reset of the records (RayTracer::UpdateLightList)
  if (m_lightListOrbit != 0.0 && !m_lightList.empty()) {
    const double a = (double)m_frameNumber * m_lightListOrbit * 3.14159265358979323846 / 180.0, ca = std::cos(a), sa = std::sin(a);
    m_lightListMoved = m_lightList;
    for (RtggxLight& l : m_lightListMoved) {
      const double px = l.position[0], pz = l.position[2], ax = l.axis[0], az = l.axis[2];
      l.position[0] = (float)(px * ca + pz * sa); l.position[2] = (float)(pz * ca - px * sa);
      l.axis[0] = (float)(ax * ca + az * sa); l.axis[2] = (float)(az * ca - ax * sa);
    }
    if (!m_rayTracer->UpdateLightList(m_lightListMoved.data(), 0u, (uint32_t)m_lightListMoved.size())) throw std::runtime_error("-lightlistorbit: " + m_rayTracer->GetLastError());
  }
  ++m_frameNumber;
  const float timeStep = m_isPaused ? 0.0f : m_fixedTimeStep;
  m_rayTracer->UpdateFrame(m_frameIndex, m_eyePt, m_view * m_proj, timeStep);
}

// RayTracedGGX.cpp:302-353.  asyncCompute: TLAS update on its own stream beside the visibility pass,
// the ray trace waits for it; otherwise everything in submission order (PopulateCommandList :513-556).
void RayTracedGGX::OnRender() {
  m_rayTracer->UpdateAccelerationStructure(m_frameIndex);
  m_rayTracer->RenderVisibility(m_frameIndex, m_asyncCompute != 0);
  m_rayTracer->RayTrace(m_frameIndex);
  m_denoiser->Denoise(m_useSharedMem, m_asyncCompute != 0);
  m_denoiser->ToneMap();
  m_frameIndex = (uint8_t)((m_frameIndex + 1) % FrameCount);   // MoveToNextFrame :684-701
  // -score: the ring holds RTGGX_SCORE_RING records; it is read that often (one wait for the main stream) and once more at the end
  if (!m_scoreFile.empty() && m_frameNumber % (uint32_t)RTGGX_SCORE_RING == 0u && !FlushScores()) throw std::runtime_error("-score: cannot write " + m_scoreFile);
  // Screen-shot helper (MoveToNextFrame :703-717: the sample copies the back buffer of the frame rendered after [F11] and writes
  // "RayTracedGGX_<time stamp>.png" FrameCount frames later).  Headless runs want reproducible names: <-dump prefix or RayTracedGGX>
  // _f<frame number, 6 digits>.png, written at once (the read-back waits for the frame).
  if (m_screenShot) {
    m_screenShot = 0;
    std::string stem = m_dumpPrefix.empty() ? std::string("RayTracedGGX") : m_dumpPrefix;
    if (stem.size() >= 4 && (stem.compare(stem.size() - 4, 4, ".png") == 0 || stem.compare(stem.size() - 4, 4, ".ppm") == 0)) stem.resize(stem.size() - 4);
    char tail[32]; std::snprintf(tail, sizeof tail, "_f%06u.png", m_frameNumber - 1u);      // OnUpdate has counted this frame already
    m_lastScreenShot = stem + tail;
    if (SaveImage(m_lastScreenShot.c_str())) std::printf("wrote %s\n", m_lastScreenShot.c_str()); else m_lastScreenShot.clear();
  }
}

void RayTracedGGX::OnDestroy() {
  if (!m_scoreFile.empty() && m_rayTracer && m_rayTracer->GetContext()) FlushScores();
  if (m_rayTracer && m_rayTracer->GetContext()) rtggx_sync(m_rayTracer->GetContext());   // WaitForGpu
  m_denoiser.reset();
  m_rayTracer.reset();
  m_initialized = false;
}

// RayTracedGGX.cpp:365-398 (key codes: ' ' pause, 0x25/0x27 mesh select, 0x26/0x28 metallic, 'V', 'A')
void RayTracedGGX::OnKeyUp(uint8_t key) {
  float& metallic = m_metallics[m_currentMesh];
  switch (key) {
    case ' ': m_isPaused = !m_isPaused; break;
    case 0x25: m_currentMesh = (m_currentMesh + RayTracer::NUM_MESH - 1) % RayTracer::NUM_MESH; break;
    case 0x27: m_currentMesh = (m_currentMesh + 1) % RayTracer::NUM_MESH; break;
    case 0x26: metallic = std::min(metallic + 0.25f, 1.0f); m_rayTracer->SetMetallic(m_currentMesh, metallic); break;
    case 0x28: metallic = std::max(metallic - 0.25f, 0.0f); m_rayTracer->SetMetallic(m_currentMesh, metallic); break;
    case 0x7A: m_screenShot = 1; break;                       // VK_F11, RayTracedGGX.cpp:388-390: the frame rendered next is saved
    case 'V': m_useSharedMem = !m_useSharedMem; break;
    case 'A': m_asyncCompute = !m_asyncCompute; m_rayTracer->SetAsyncCompute(m_asyncCompute != 0); break;   // RayTracedGGX.cpp:394-396
    default: break;
  }
}

// RayTracedGGX.cpp:400-455: orbit about the focus point while the left button is held, dolly with the wheel
void RayTracedGGX::OnLButtonDown(float posX, float posY) { m_tracking = true; m_mousePt[0] = posX; m_mousePt[1] = posY; }
void RayTracedGGX::OnLButtonUp(float, float) { m_tracking = false; }
void RayTracedGGX::OnMouseLeave() { m_tracking = false; }
static float distance(const xm::Float3& a, const xm::Float3& b) { const xm::Float3 d = xm::Sub(a, b); return std::sqrt(xm::Dot(d, d)); }
void RayTracedGGX::OnMouseMove(float posX, float posY) {
  if (!m_tracking) return;
  const float dx = m_mousePt[0] - posX, dy = m_mousePt[1] - posY;
  const float twoPi = 6.283185307f;                                     // XM_2PI
  const float pitch = twoPi * dy / (float)m_height, yaw = twoPi * dx / (float)m_width;
  const float len = distance(m_focusPt, m_eyePt);
  xm::Matrix transform = xm::Translation(0.0f, 0.0f, -len);
  transform = transform * xm::RotationRollPitchYaw(pitch, yaw, 0.0f);
  transform = transform * xm::Translation(0.0f, 0.0f, len);
  m_view = m_view * transform;
  const xm::Matrix viewInv = xm::Inverse(m_view);
  m_eyePt = {viewInv.r[3][0], viewInv.r[3][1], viewInv.r[3][2]};
  m_mousePt[0] = posX; m_mousePt[1] = posY;
}
void RayTracedGGX::OnMouseWheel(float deltaZ, float, float) {
  const float len = distance(m_focusPt, m_eyePt);
  m_view = m_view * xm::Translation(0.0f, 0.0f, -len * deltaZ / 16.0f);
  const xm::Matrix viewInv = xm::Inverse(m_view);
  m_eyePt = {viewInv.r[3][0], viewInv.r[3][1], viewInv.r[3][2]};
}

bool RayTracedGGX::LoadTrack(const std::string& fileName) {
  FILE* f = std::fopen(fileName.c_str(), "r");
  if (!f) return false;
  m_track.clear(); m_trackNext = 0;
  char line[256];
  while (std::fgets(line, sizeof line, f)) {
    unsigned frame; char cmd[32], arg[32]; float a = 0.0f, b = 0.0f;
    if (line[0] == '#' || std::sscanf(line, "%u %31s", &frame, cmd) != 2) continue;
    const std::string c = cmd;
    TrackEvent e{frame, 5, 0.0f, 0.0f};
    if (c == "key") {
      if (std::sscanf(line, "%u %*s %31s", &frame, arg) != 2) continue;
      const std::string k = arg;
      const int code = k == "SPACE" ? ' ' : k == "LEFT" ? 0x25 : k == "UP" ? 0x26 : k == "RIGHT" ? 0x27 : k == "DOWN" ? 0x28 : k == "F11" ? 0x7A : k.size() == 1 ? std::toupper((unsigned char)k[0]) : std::atoi(arg);
      e.type = 0; e.a = (float)code;
    } else if (c == "down" || c == "up" || c == "move") {
      if (std::sscanf(line, "%u %*s %f %f", &frame, &a, &b) != 3) continue;
      e.type = c == "down" ? 1 : c == "up" ? 2 : 3; e.a = a; e.b = b;
    } else if (c == "wheel") {
      if (std::sscanf(line, "%u %*s %f", &frame, &a) != 2) continue;
      e.type = 4; e.a = a;
    } else if (c != "leave") continue;
    m_track.push_back(e);
  }
  std::fclose(f);
  std::stable_sort(m_track.begin(), m_track.end(), [](const TrackEvent& x, const TrackEvent& y) { return x.frame < y.frame; });
  return true;
}

// RayTracedGGX.cpp:462-511: '-' or '/' prefix, case-insensitive names; a following token is a value
// unless it starts with '/' or with '-' not followed by a digit or '.'.
// A light from the numbers of -light / -spot or of a line of -lightlist: v = position, intensity, range, radius and (spot) axis, outer and
// inner half-angle in degrees.  Everything the library would refuse is refused here; what / whatSpot lead the message.  The cosines:
// cos(degrees pi / 180) in double, rounded once.
static RtggxLight lightFromNumbers(const std::string& what, const std::string& whatSpot, bool spot, const float v[13]) {
  RtggxLight l{};
  for (int k = 0; k < 3; ++k) { l.position[k] = v[k]; l.intensity[k] = v[3 + k]; }
  l.range = v[6]; l.radius = v[7]; l.cos_outer = -1.0f; l.cos_inner = 1.0f;
  for (int k = 0; k < 3; ++k) if (!std::isfinite(l.position[k])) throw std::runtime_error(what + ": a finite position");
  for (int k = 0; k < 3; ++k) if (!std::isfinite(l.intensity[k]) || l.intensity[k] < 0.0f) throw std::runtime_error(what + ": an intensity that is finite and not negative");
  if (!std::isfinite(l.range) || !(l.range > 0.0f)) throw std::runtime_error(what + ": a range that is finite and above 0");
  if (!std::isfinite(l.radius) || l.radius < 0.0f || !(l.radius < l.range)) throw std::runtime_error(what + ": a radius that is finite, not negative and below the range");
  if (spot) {
    for (int k = 0; k < 3; ++k) l.axis[k] = v[8 + k];
    const double len = std::sqrt((double)v[8] * v[8] + (double)v[9] * v[9] + (double)v[10] * v[10]);
    if (!std::isfinite(len) || !(len > 0.0)) throw std::runtime_error(whatSpot + ": an axis of finite, non-zero length");
    if (!(v[12] > 0.0f && v[12] < v[11] && v[11] < 180.0f)) throw std::runtime_error(whatSpot + ": half-angles in degrees with 0 < inner < outer < 180");
    l.cos_outer = (float)std::cos((double)v[11] * 3.14159265358979323846 / 180.0); l.cos_inner = (float)std::cos((double)v[12] * 3.14159265358979323846 / 180.0);
    if (!(l.cos_outer > -1.0f && l.cos_outer < l.cos_inner && l.cos_inner <= 1.0f)) throw std::runtime_error(whatSpot + ": half-angles in degrees with 0 < inner < outer < 180, apart by more than fp32 tells");
  }
  return l;
}

void RayTracedGGX::ParseCommandLineArgs(char* argv[], int argc) {
  const auto lower = [](std::string s) { std::transform(s.begin(), s.end(), s.begin(), [](unsigned char ch) { return (char)std::tolower(ch); }); return s; };
  const auto isArgMatched = [&](int i, const char* name) {
    const char* arg = argv[i];
    return (arg[0] == '-' || arg[0] == '/') && lower(arg + 1) == lower(name);
  };
  // On POSIX an absolute path also starts with '/': such a token is a flag only when it names one.
  static const char* const kFlags[] = {"warp", "uma", "mesh", "env", "width", "height", "frames", "dt", "metallic", "sharedmem", "sync", "vndf", "device", "dump", "gpus", "track", "deform", "rank", "idfile", "strips", "balance", "rayrate", "sun", "sunreflections", "sunfromenv", "sunangle", "light", "spot", "lightreflections", "lightpick", "lightvisibility", "lightlistvisibility", "lightlistorbit", "lightlist", "recursion", "spp", "accumulate", "sampleset", "savereference", "reference", "score", "envlayout", "envsize", "envmips", "envprefilter"};
  const auto isFlagName = [&](const char* name) { for (const char* f : kFlags) if (lower(name) == f) return true; return false; };
  const auto hasNextArgValue = [&](int i) {
    if (i + 1 >= argc) return false;
    const char* arg = argv[i + 1];
    if (arg[0] == '/') return !isFlagName(arg + 1);
    return arg[0] != '-' || (arg[1] >= '0' && arg[1] <= '9') || arg[1] == '.';
  };
  const auto nextFloat = [&](int& i, float& dst) { if (hasNextArgValue(i)) { float v; if (std::sscanf(argv[i + 1], "%f", &v) == 1) { dst = v; ++i; } } };
  for (int i = 1; i < argc; ++i) {
    if (isArgMatched(i, "warp") || isArgMatched(i, "uma")) continue;   // device selection of the D3D sample: ignored
    else if (isArgMatched(i, "mesh")) {
      if (hasNextArgValue(i)) m_meshFileName = argv[++i];
      nextFloat(i, m_meshPosScale[0]); nextFloat(i, m_meshPosScale[1]); nextFloat(i, m_meshPosScale[2]); nextFloat(i, m_meshPosScale[3]);
    } else if (isArgMatched(i, "env")) { if (hasNextArgValue(i)) m_envFileName = argv[++i]; }
    // environments from images (RayTracer::SetEnvOptions): the layout of a .hdr / .pfm image whose aspect ratio does not tell, the side of
    // the cube a panorama is resampled to, and the mip chain of a DDS cube that came without one built on the device
    else if (isArgMatched(i, "envlayout")) {
      if (!hasNextArgValue(i) || !EnvImage::ParseLayoutName(lower(argv[++i]), m_envLayout)) throw std::runtime_error("-envlayout: equirect, vcross or hcross");
    }
    else if (isArgMatched(i, "envsize")) {
      const long size = hasNextArgValue(i) ? std::atol(argv[++i]) : 0;
      if (size < 1 || size > 4096) throw std::runtime_error("-envsize: the side of the cube, 1 to 4096");
      m_envSize = (uint32_t)size;
    }
    else if (isArgMatched(i, "envmips")) m_envMips = true;
    // -envprefilter [N]: GGX-prefiltered levels below level 0 (rtggx_prefilter_env); the count is checked here, before a device is asked for
    else if (isArgMatched(i, "envprefilter")) {
      long samples = 1024;
      if (hasNextArgValue(i)) { char* end = nullptr; samples = std::strtol(argv[++i], &end, 10); if (end == argv[i] || *end != '\0') samples = -1; }
      if (samples < (long)RTGGX_ENV_FILTER_MIN_SAMPLES || samples > (long)RTGGX_ENV_FILTER_MAX_SAMPLES || (samples & (samples - 1)) != 0) throw std::runtime_error("-envprefilter: a number of samples that is a power of two from 64 to 4096 (1024 without a number)");
      m_envPrefilter = (uint32_t)samples;
    }
    // extensions replacing the window / message loop
    else if (isArgMatched(i, "width")) { if (hasNextArgValue(i)) m_width = (uint32_t)std::atoi(argv[++i]); }
    else if (isArgMatched(i, "height")) { if (hasNextArgValue(i)) m_height = (uint32_t)std::atoi(argv[++i]); }
    else if (isArgMatched(i, "frames")) { if (hasNextArgValue(i)) m_numFrames = (uint32_t)std::atoi(argv[++i]); }
    else if (isArgMatched(i, "dt")) { nextFloat(i, m_fixedTimeStep); }
    else if (isArgMatched(i, "metallic")) { nextFloat(i, m_metallics[0]); nextFloat(i, m_metallics[1]); m_hasMetallicOverride = true; }
    else if (isArgMatched(i, "sharedmem")) m_useSharedMem = true;
    else if (isArgMatched(i, "sync")) m_asyncCompute = 0;
    else if (isArgMatched(i, "vndf")) m_vndf = true;
    // -sun <x> <y> <z> <r> <g> <b>: a directional light toward (x, y, z) with irradiance (r, g, b) and ray-traced shadows (rtggx_set_sun); the
    // six numbers are checked here, before a device is asked for
    else if (isArgMatched(i, "sun")) {
      int got = 0;
      for (; got < 6 && hasNextArgValue(i); ++got) { char* end = nullptr; m_sun[got] = std::strtof(argv[++i], &end); if (end == argv[i] || *end != '\0') throw std::runtime_error("-sun: six numbers, a direction toward the sun and an irradiance"); }
      if (got != 6) throw std::runtime_error("-sun: six numbers, a direction toward the sun and an irradiance");
      const double len = std::sqrt((double)m_sun[0] * m_sun[0] + (double)m_sun[1] * m_sun[1] + (double)m_sun[2] * m_sun[2]);
      if (!std::isfinite(len) || !(len > 0.0)) throw std::runtime_error("-sun: a direction of finite, non-zero length");
      for (int k = 3; k < 6; ++k) if (!std::isfinite(m_sun[k]) || m_sun[k] < 0.0f) throw std::runtime_error("-sun: an irradiance that is finite and not negative");
      m_hasSun = true;
    }
    else if (isArgMatched(i, "sunreflections")) m_sunReflections = true;      // (without -sun: refused below, once the whole line is read)
    else if (isArgMatched(i, "lightreflections")) m_lightReflections = true;      // (without -light / -spot: refused below, once the whole line is read)
    else if (isArgMatched(i, "lightpick")) m_lightPick = true;      // (without -light / -spot: refused below, once the whole line is read)
    else if (isArgMatched(i, "lightlistorbit")) {      // (without -lightlist: refused below, once the whole line is read)
      if (i + 1 >= argc) throw std::runtime_error("-lightlistorbit: degrees per frame");
      char* end = nullptr; m_lightListOrbit = std::strtod(argv[++i], &end);
      if (end == argv[i] || *end || !std::isfinite(m_lightListOrbit)) throw std::runtime_error(std::string("-lightlistorbit: ") + argv[i] + ": degrees per frame, a finite number");
      m_lightListOrbitGiven = true;
    }
    else if (isArgMatched(i, "lightlistvisibility")) m_lightListVisibility = true;      // (without -lightlist, or with strips: refused below, once the whole line is read)
    else if (isArgMatched(i, "lightvisibility")) m_lightVisibility = true;      // (without -lightpick, or with strips: refused below, once the whole line is read)
    // -sunfromenv [degrees]: the sun measured from the -env cube and taken out of it (rtggx_sun_from_env, RayTracer::Init); the half-angle
    // of the cone is checked here, before a device is asked for; without a number it is the library's default
    else if (isArgMatched(i, "sunfromenv")) {
      float cone = 0.0f;
      if (hasNextArgValue(i)) {
        char* end = nullptr; cone = std::strtof(argv[++i], &end);
        if (end == argv[i] || *end != '\0' || !(cone > 0.0f && cone <= 45.0f)) throw std::runtime_error("-sunfromenv: the half-angle of the sun's cone in degrees, above 0 and at most 45 (4 without a number)");
      }
      m_sunFromEnv = true; m_sunFromEnvCone = cone;
    }
    // -sunangle <degrees>: the angular radius of the sun's disk (rtggx_set_sun_angle); checked here, before a device is asked for
    else if (isArgMatched(i, "sunangle")) {
      float angle = -1.0f;
      if (hasNextArgValue(i)) { char* end = nullptr; angle = std::strtof(argv[++i], &end); if (end == argv[i] || *end != '\0') angle = -1.0f; }
      if (!(angle >= 0.0f && angle <= RTGGX_MAX_SUN_ANGLE_DEGREES)) throw std::runtime_error("-sunangle: the angular radius of the sun's disk in degrees, 0 to 10");
      m_sunAngle = angle; m_hasSunAngle = true;
    }
    // -light <x> <y> <z> <r> <g> <b> <range> [<radius>] and -spot <x> <y> <z> <r> <g> <b> <range> <radius> <ax> <ay> <az> <outer degrees>
    // <inner degrees>: a point or a spot light (rtggx_set_lights), repeatable, in the order typed; everything the library would refuse is
    // refused here, before a device is asked for.  The cosines: cos(degrees pi / 180) in double, rounded once.
    else if (isArgMatched(i, "light") || isArgMatched(i, "spot")) {
      const bool spot = isArgMatched(i, "spot");
      const std::string what = spot ? "-spot" : "-light";
      const std::string usage = spot ? "-spot: thirteen numbers -- position, intensity, range, radius, axis, outer and inner half-angle in degrees"
                                     : "-light: seven or eight numbers -- position, intensity, range and, optionally, radius";
      float v[13] = {};
      int got = 0;
      for (; got < (spot ? 13 : 8) && hasNextArgValue(i); ++got) { char* end = nullptr; v[got] = std::strtof(argv[++i], &end); if (end == argv[i] || *end != '\0') throw std::runtime_error(usage); }
      if (spot ? got != 13 : got < 7) throw std::runtime_error(usage);
      if (m_lights.size() >= RTGGX_MAX_LIGHTS) throw std::runtime_error(what + ": at most 8 lights (-light and -spot together)");
      m_lights.push_back(lightFromNumbers(what, spot ? "-spot" : what, spot, v));
    }
    // -lightlist <file>: a light list beyond eight (rtggx_set_light_list).  Plain text, a light per line, blank lines and # comments allowed:
    //   light x y z r g b range [radius]
    //   spot x y z r g b range radius ax ay az outer inner      (the angles in degrees, as for -spot)
    // read and checked here, with the line number in the message, before a device is asked for
    else if (isArgMatched(i, "lightlist")) {
      if (!hasNextArgValue(i)) throw std::runtime_error("-lightlist: a file name");
      m_lightListFile = argv[++i];
      FILE* f = std::fopen(m_lightListFile.c_str(), "r");
      if (!f) throw std::runtime_error("-lightlist: cannot open " + m_lightListFile);
      std::vector<std::string> lines;
      { std::string line; int ch; while ((ch = std::fgetc(f)) != EOF) { if (ch == '\n') { lines.push_back(line); line.clear(); } else line.push_back((char)ch); } if (!line.empty()) lines.push_back(line); }
      std::fclose(f);
      m_lightList.clear();
      for (size_t n = 0; n < lines.size(); ++n) {
        std::string text = lines[n].substr(0, lines[n].find('#'));
        std::vector<std::string> words;
        { size_t at = 0; while (at < text.size()) { while (at < text.size() && std::isspace((unsigned char)text[at])) ++at; size_t end = at; while (end < text.size() && !std::isspace((unsigned char)text[end])) ++end; if (end > at) words.push_back(text.substr(at, end - at)); at = end; } }
        if (words.empty()) continue;
        const std::string where = "-lightlist: " + m_lightListFile + ", line " + std::to_string(n + 1);
        const bool spot = words[0] == "spot";
        if (!spot && words[0] != "light") throw std::runtime_error(where + ": '" + words[0] + "': a line begins with light or spot");
        const std::string usage = where + (spot ? ": spot and thirteen numbers -- position, intensity, range, radius, axis, outer and inner half-angle in degrees"
                                                : ": light and seven or eight numbers -- position, intensity, range and, optionally, radius");
        float v[13] = {};
        const size_t got = words.size() - 1;
        if (spot ? got != 13 : (got != 7 && got != 8)) throw std::runtime_error(usage);
        for (size_t k = 0; k < got; ++k) { char* end = nullptr; v[k] = std::strtof(words[k + 1].c_str(), &end); if (end == words[k + 1].c_str() || *end != '\0') throw std::runtime_error(usage); }
        if (m_lightList.size() >= RTGGX_MAX_LIGHT_LIST) throw std::runtime_error(where + ": at most 1024 lights");
        m_lightList.push_back(lightFromNumbers(where, where, spot, v));
      }
    }
    else if (isArgMatched(i, "rayrate")) {
      const int rate = hasNextArgValue(i) ? std::atoi(argv[++i]) : 0;
      if (rate != 1 && rate != 4) throw std::runtime_error("-rayrate: 1 or 4 pixels per traced ray");
      m_rayRate = (uint32_t)rate;
    }
    else if (isArgMatched(i, "recursion")) {
      const int depth = hasNextArgValue(i) ? std::atoi(argv[++i]) : 0;
      if (depth < 1 || depth > (int)RTGGX_MAX_RECURSION_DEPTH) throw std::runtime_error("-recursion: 1 to 4 levels of rays per path");
      m_recursionDepth = (uint32_t)depth;
    }
    else if (isArgMatched(i, "spp")) {
      const int samples = hasNextArgValue(i) ? std::atoi(argv[++i]) : 0;
      if (samples != 1 && samples != 2 && samples != 4 && samples != 8) throw std::runtime_error("-spp: 1, 2, 4 or 8 samples per pixel");
      m_samplesPerPixel = (uint32_t)samples;
    }
    else if (isArgMatched(i, "sampleset")) {
      const long size = hasNextArgValue(i) ? std::atol(argv[++i]) : 0;
      if (size < (long)RTGGX_MIN_SAMPLE_SET || size > (long)RTGGX_MAX_SAMPLE_SET || (size & (size - 1)) != 0) throw std::runtime_error("-sampleset: a power of two from 256 to 65536");
      m_sampleSet = (uint32_t)size;
    }
    else if (isArgMatched(i, "accumulate")) {
      const int frames = hasNextArgValue(i) ? std::atoi(argv[++i]) : 0;
      if (frames < 1) throw std::runtime_error("-accumulate: a number of frames, 1 or more");
      m_accumulate = (uint32_t)frames;
    }
    else if (isArgMatched(i, "savereference")) { if (hasNextArgValue(i)) m_saveReferenceFile = argv[++i]; else throw std::runtime_error("-savereference: a file name"); }
    else if (isArgMatched(i, "reference")) { if (hasNextArgValue(i)) m_referenceFile = argv[++i]; else throw std::runtime_error("-reference: a file name"); }
    else if (isArgMatched(i, "score")) { if (hasNextArgValue(i)) m_scoreFile = argv[++i]; else throw std::runtime_error("-score: a file name"); }
    else if (isArgMatched(i, "device")) { if (hasNextArgValue(i)) m_device = std::atoi(argv[++i]); }
    else if (isArgMatched(i, "dump")) { if (hasNextArgValue(i)) m_dumpPrefix = argv[++i]; }
    else if (isArgMatched(i, "deform")) { nextFloat(i, m_deformAmplitude); }
    else if (isArgMatched(i, "track")) { if (hasNextArgValue(i)) m_trackFileName = argv[++i]; }
    // Several GPUs = one process per GPU, each rendering a strip of rows and exchanging the temporal history over RCCL
    // (host/Strips.cpp; Main.cpp restarts the executable once per rank).  -rank / -idfile are what the launcher passes on;
    // -strips N renders N strips in THIS process on one GPU (the exchange code without N GPUs); -balance 0: equal strips.
    else if (isArgMatched(i, "gpus")) { if (hasNextArgValue(i)) m_gpus = std::atoi(argv[++i]); if (m_gpus < 1 || m_gpus > 64) throw std::runtime_error("-gpus: 1 .. 64"); }
    else if (isArgMatched(i, "rank")) { if (hasNextArgValue(i)) m_rank = std::atoi(argv[++i]); }
    else if (isArgMatched(i, "idfile")) { if (hasNextArgValue(i)) m_idFile = argv[++i]; }
    else if (isArgMatched(i, "strips")) { if (hasNextArgValue(i)) m_strips = std::atoi(argv[++i]); if (m_strips < 1 || m_strips > 64) throw std::runtime_error("-strips: 1 .. 64"); }
    else if (isArgMatched(i, "balance")) { if (hasNextArgValue(i)) m_balance = std::atoi(argv[++i]) != 0; }
  }
  // a cross is never resampled (rtggx_set_env_image); where the layout comes from the image's aspect ratio RayTracer::Init refuses it
  if (m_envSize != 0u && (m_envLayout == EnvImage::VCROSS || m_envLayout == EnvImage::HCROSS)) throw std::runtime_error("-envsize together with -envlayout vcross / hcross: a cross is never resampled, its cells are the cube's faces");
  // three quarters of a rate-4 frame are interpolations (rtggx_set_accumulation); the sums of several strips are not gathered
  if (m_accumulate != 0u && m_rayRate != 1u) throw std::runtime_error("-accumulate together with -rayrate 4: refused");
  if (m_accumulate != 0u && (m_gpus > 1 || m_strips > 1)) throw std::runtime_error("-accumulate: whole frames on one GPU only, not with -gpus N > 1 or -strips N > 1");
  // scoring against a reference (rtggx_set_scoring): a strip scores its own rows and nobody adds the records of several; the file is read
  // -- and a bad one refused -- here, before anything has touched a GPU
  if (!m_saveReferenceFile.empty() && m_accumulate == 0u) throw std::runtime_error("-savereference: needs -accumulate N (the converged image is what it writes)");
  if (!m_scoreFile.empty() && m_referenceFile.empty()) throw std::runtime_error("-score: needs -reference <file.pfm>");
  if ((!m_scoreFile.empty() || !m_referenceFile.empty()) && (m_gpus > 1 || m_strips > 1)) throw std::runtime_error("-reference / -score: whole frames on one GPU only, not with -gpus N > 1 or -strips N > 1");
  if (!m_referenceFile.empty()) { std::string why; if (!ReadPfm(m_referenceFile.c_str(), m_width, m_height, m_referenceImage, why)) throw std::runtime_error("-reference: " + why); }
  // the sun in reflections (rtggx_set_sun_reflections) acts only under a sun: asking for it without one is a mistake, refused here
  // one sun: the one typed in or the one the environment holds; and a sun excludes rate 4 wherever it comes from (rtggx_set_sun)
  if (m_sunFromEnv && m_hasSun) throw std::runtime_error("-sunfromenv together with -sun: one sun, measured or given");
  if (m_sunFromEnv && m_rayRate != 1u) throw std::runtime_error("-sunfromenv together with -rayrate 4: refused");
  if (m_sunReflections && !m_hasSun && !m_sunFromEnv) throw std::runtime_error("-sunreflections without -sun: there is no light to reflect");
  if (m_hasSunAngle && !m_hasSun && !m_sunFromEnv) throw std::runtime_error("-sunangle without -sun or -sunfromenv: there is no sun to give a size");
  // quarter-rate tracing renders whole frames only (rtggx_set_ray_rate): refused here, before anything has touched a GPU
  // one knob asks for fewer rays, the other for more (rtggx_set_samples_per_pixel)
  if (m_rayRate != 1u && m_hasSun) throw std::runtime_error("-sun together with -rayrate 4: refused");
  // the lights in reflections (rtggx_set_light_reflections) act only under lights: the rule of -sunreflections without -sun
  if (m_lightReflections && m_lights.empty() && m_lightList.empty()) throw std::runtime_error("-lightreflections without -light or -spot: there is no light to reflect");
  // one ray for all lights (rtggx_set_light_sampling) acts only under lights: the same rule
  if (m_lightPick && m_lights.empty()) throw std::runtime_error("-lightpick without -light or -spot: there is no light to pick");
  // the pick's visibility records (rtggx_set_light_pick_visibility) act only in mode 1, and on whole frames
  if (m_lightVisibility && !m_lightPick) throw std::runtime_error("-lightvisibility without -lightpick: there is no pick to weight");
  if (m_lightVisibility && (m_gpus > 1 || m_strips > 1)) throw std::runtime_error("-lightvisibility: whole frames only, not with -gpus N > 1 or -strips N > 1");
  if (m_rayRate != 1u && !m_lights.empty()) throw std::runtime_error("-light / -spot together with -rayrate 4: refused");
  // a light list (rtggx_set_light_list) is held in place of the lights, not beside them, and excludes rate 4 as they do
  // the list's visibility records (rtggx_set_light_list_visibility) act only on a list, and on whole frames
  if (m_lightListOrbitGiven && m_lightListFile.empty()) throw std::runtime_error("-lightlistorbit without -lightlist: there is no list to turn");
  if (m_lightListVisibility && m_lightListFile.empty()) throw std::runtime_error("-lightlistvisibility without -lightlist: there is no list whose pick to weight");
  if (m_lightListVisibility && (m_gpus > 1 || m_strips > 1)) throw std::runtime_error("-lightlistvisibility: whole frames only, not with -gpus N > 1 or -strips N > 1");
  if (!m_lightListFile.empty() && !m_lights.empty()) throw std::runtime_error("-lightlist together with -light / -spot: the context holds one or the other");
  if (!m_lightListFile.empty() && m_rayRate != 1u) throw std::runtime_error("-lightlist together with -rayrate 4: refused");
  if (m_rayRate != 1u && m_samplesPerPixel != 1u) throw std::runtime_error("-spp N > 1 together with -rayrate 4: refused");
  if (m_rayRate != 1u && (m_gpus > 1 || m_strips > 1)) throw std::runtime_error("-rayrate 4: whole frames only, not with -gpus N > 1 or -strips N > 1");
}

// PNG, the container the sample's screenshot uses (stbi_write_png, RayTracedGGX.cpp:736): 8-bit RGB or RGBA, one IDAT of
// stored (uncompressed) deflate blocks -- every PNG reader accepts it, and no compression library is needed.
bool WritePng(const char* fileName, uint32_t w, uint32_t h, uint32_t comp, const uint8_t* pixels) {
  if ((comp != 3 && comp != 4) || w == 0 || h == 0) return false;
  static uint32_t crcTable[256];
  if (!crcTable[1]) for (uint32_t n = 0; n < 256; ++n) { uint32_t c = n; for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1; crcTable[n] = c; }
  const auto be32 = [](std::vector<uint8_t>& v, uint32_t x) { v.push_back((uint8_t)(x >> 24)); v.push_back((uint8_t)(x >> 16)); v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x); };
  std::vector<uint8_t> file = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
  const auto chunk = [&](const char* type, const std::vector<uint8_t>& data) {
    be32(file, (uint32_t)data.size());
    const size_t start = file.size();
    file.insert(file.end(), type, type + 4); file.insert(file.end(), data.begin(), data.end());
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = start; i < file.size(); ++i) c = crcTable[(c ^ file[i]) & 0xFFu] ^ (c >> 8);
    be32(file, c ^ 0xFFFFFFFFu);
  };
  std::vector<uint8_t> ihdr; be32(ihdr, w); be32(ihdr, h);
  ihdr.push_back(8); ihdr.push_back(comp == 3 ? 2 : 6); ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);
  chunk("IHDR", ihdr);
  // raw image: per scanline a filter byte (0 = none) + the pixels
  const size_t stride = (size_t)w * comp + 1;
  std::vector<uint8_t> raw(stride * h);
  for (uint32_t y = 0; y < h; ++y) { raw[y * stride] = 0; std::memcpy(&raw[y * stride + 1], pixels + (size_t)y * w * comp, (size_t)w * comp); }
  std::vector<uint8_t> z = {0x78, 0x01};      // zlib header, then stored blocks of at most 65535 bytes
  uint32_t a = 1, b = 0;                       // Adler-32 of the raw data
  for (size_t pos = 0; pos < raw.size();) {
    const size_t n = std::min<size_t>(65535, raw.size() - pos);
    z.push_back(pos + n == raw.size() ? 1 : 0);
    z.push_back((uint8_t)n); z.push_back((uint8_t)(n >> 8)); z.push_back((uint8_t)~n); z.push_back((uint8_t)(~n >> 8));
    z.insert(z.end(), raw.begin() + pos, raw.begin() + pos + n);
    for (size_t i = pos; i < pos + n; ++i) { a = (a + raw[i]) % 65521u; b = (b + a) % 65521u; }
    pos += n;
  }
  be32(z, (b << 16) | a);
  chunk("IDAT", z);
  chunk("IEND", {});
  FILE* f = std::fopen(fileName, "wb");
  if (!f) return false;
  const bool ok = std::fwrite(file.data(), 1, file.size(), f) == file.size();
  std::fclose(f);
  return ok;
}

// fp16 <-> fp32 on the host, bit by bit: every half is exact in fp32; fp32 to half rounds to nearest even, overflows to infinity, keeps NaN.
static float halfToFloat(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3FFu;
  uint32_t u;
  if (e == 0u) {
    if (m == 0u) u = sign;
    else { int shift = 0; uint32_t mm = m; while (!(mm & 0x400u)) { mm <<= 1; ++shift; } u = sign | ((uint32_t)(113 - shift) << 23) | ((mm & 0x3FFu) << 13); }
  } else if (e == 31u) u = sign | 0x7F800000u | (m << 13);
  else u = sign | ((e + 112u) << 23) | (m << 13);
  float f; std::memcpy(&f, &u, 4); return f;
}
static uint16_t floatToHalf(float f) {
  uint32_t u; std::memcpy(&u, &f, 4);
  const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
  const uint32_t a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return (uint16_t)(sign | 0x7E00u | ((a >> 13) & 0x3FFu));      // NaN
  if (a >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);                              // 65536 and beyond, infinity
  if (a < 0x38800000u) {                                                               // below the smallest normal half: a multiple of 2^-24
    if (a < 0x33000000u) return sign;                                                  // below 2^-25: zero (2^-25 itself is a tie, to even: zero)
    const uint32_t e = a >> 23, mant = (a & 0x7FFFFFu) | 0x800000u, sh = 126u - e;     // value = mant * 2^(e - 150); in units of 2^-24: mant >> (126 - e)
    const uint32_t q = mant >> sh, rem = mant & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    return (uint16_t)(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
  }
  uint32_t r = a - 0x38000000u;                                                        // rebias, then round the 13 dropped bits to even; a carry walks into the exponent
  r += 0xFFFu + ((r >> 13) & 1u);
  return (uint16_t)(sign | (r >> 13));
}

bool WritePfm(const char* fileName, uint32_t w, uint32_t h, const uint16_t* rgba16f) {
  if (!fileName || !rgba16f || w == 0u || h == 0u) return false;
  FILE* f = std::fopen(fileName, "wb");
  if (!f) return false;
  std::fprintf(f, "PF\n%u %u\n-1.0\n", w, h);
  std::vector<float> row((size_t)w * 3);
  bool ok = true;
  for (uint32_t y = h; y-- > 0u && ok;) {      // bottom row first
    for (uint32_t x = 0; x < w; ++x) for (int k = 0; k < 3; ++k) row[3 * (size_t)x + k] = halfToFloat(rgba16f[4 * ((size_t)y * w + x) + k]);
    ok = std::fwrite(row.data(), 4, row.size(), f) == row.size();
  }
  return std::fclose(f) == 0 && ok;
}

bool ReadPfm(const char* fileName, uint32_t w, uint32_t h, std::vector<uint16_t>& rgba16f, std::string& error) {
  const std::string name = fileName ? fileName : "";
  FILE* f = std::fopen(name.c_str(), "rb");
  if (!f) { error = "cannot open " + name; return false; }
  const auto fail = [&](const std::string& why) { std::fclose(f); error = name + ": " + why; return false; };
  // the header: three tokens lines "PF", "<w> <h>", "<scale>", separated by white space, ONE white-space byte behind the scale
  char magic[3] = {0, 0, 0}; unsigned fw = 0, fh = 0; double scale = 0.0; char sep = 0;
  if (std::fscanf(f, "%2s", magic) != 1 || std::strcmp(magic, "PF") != 0) return fail("not a colour PFM file (no \"PF\")");
  if (std::fscanf(f, "%u %u", &fw, &fh) != 2) return fail("malformed PFM header (width and height)");
  if (std::fscanf(f, "%lf", &scale) != 1 || std::fread(&sep, 1, 1, f) != 1 || !std::isspace((unsigned char)sep)) return fail("malformed PFM header (scale)");
  if (!(scale < 0.0)) return fail("a non-negative scale: big-endian PFM files are not read");
  if (fw != w || fh != h) { char t[96]; std::snprintf(t, sizeof t, "%u x %u pixels, the frame has %u x %u", fw, fh, w, h); return fail(t); }
  std::vector<float> row((size_t)w * 3);
  rgba16f.assign((size_t)w * h * 4, 0x3C00u);      // alpha 1
  for (uint32_t y = h; y-- > 0u;) {
    if (std::fread(row.data(), 4, row.size(), f) != row.size()) { rgba16f.clear(); return fail("truncated PFM file"); }
    for (uint32_t x = 0; x < w; ++x) for (int k = 0; k < 3; ++k) rgba16f[4 * ((size_t)y * w + x) + k] = floatToHalf(row[3 * (size_t)x + k]);
  }
  std::fclose(f);
  return true;
}

bool RayTracedGGX::SaveReference(const char* fileName) {
  rtggx_context* ctx = GetContext();
  if (!ctx) return false;
  std::vector<uint16_t> image((size_t)m_width * m_height * 4);
  if (rtggx_readback(ctx, RTGGX_BUF_CONVERGED, image.data(), image.size() * 2) != 0) { std::fprintf(stderr, "SaveReference: %s\n", rtggx_last_error()); return false; }
  if (!WritePfm(fileName, m_width, m_height, image.data())) { std::fprintf(stderr, "SaveReference: cannot write %s\n", fileName); return false; }
  std::printf("wrote %s\n", fileName);
  return true;
}

// One JSON line per record: the relative L2 distances sqrt(se / ref2) -- null where the reference's energy is 0 --, %.17g: the double itself.
bool RayTracedGGX::FlushScores() {
  if (m_scoreFile.empty() || !m_rayTracer) return false;
  std::vector<RtggxScore> scores;
  if (!m_rayTracer->ReadScores(scores)) { std::fprintf(stderr, "FlushScores: %s\n", m_rayTracer->GetLastError().c_str()); return false; }
  FILE* f = std::fopen(m_scoreFile.c_str(), m_scoreFileStarted ? "ab" : "wb");
  if (!f) return false;
  m_scoreFileStarted = true;
  const auto rel = [&](const char* key, double se, double ref2) {
    if (ref2 > 0.0 && std::isfinite(se)) std::fprintf(f, ", \"%s\": %.17g", key, std::sqrt(se / ref2)); else std::fprintf(f, ", \"%s\": null", key);
  };
  for (const RtggxScore& s : scores) {
    std::fprintf(f, "{\"index\": %llu, \"frame_index\": %u", (unsigned long long)s.index, s.frame_index);
    rel("rel_l2_out", s.se_out_rgb, s.ref_rgb2); rel("rel_l2_raw", s.se_raw_rgb, s.ref_rgb2);
    rel("rel_l2_out_cov", s.se_out_rgb_cov, s.ref_rgb2_cov); rel("rel_l2_raw_cov", s.se_raw_rgb_cov, s.ref_rgb2_cov);
    rel("rel_l2_out_luma", s.se_out_luma, s.ref_luma2); rel("rel_l2_raw_luma", s.se_raw_luma, s.ref_luma2);
    std::fprintf(f, ", \"pixels\": %llu, \"covered\": %llu, \"skipped_out\": %llu, \"skipped_raw\": %llu}\n", (unsigned long long)s.pixels,
                 (unsigned long long)s.covered, (unsigned long long)s.skipped_out, (unsigned long long)s.skipped_raw);
  }
  return std::fclose(f) == 0;
}

// The mean relative standard error of Y over covered pixels of one accumulated image, from its sums (4 floats per pixel: sum r, g, b, Y^2):
// per pixel mean = (0.25 sum r + 0.5 sum g + 0.25 sum b) / n, variance = (sum Y^2 / n - mean^2) n / (n - 1), error = sqrt(variance / n) / mean;
// pixels the image never received anything at (all four sums zero) and pixels of mean 0 are left out.  Negative: no pixel counted.
// n is the count of ALL accumulated frames: the figure assumes what -accumulate provides, materials and coverage that stay as they are over
// those frames.  Where fewer than n frames contributed to a pixel of the diffuse image (metallic changed in mid-run, the model turned under
// it), mean and variance are those of a sum diluted by the missing frames, not the diffuse image's own: reset after such a change.
static double meanRelativeStdError(const std::vector<float>& sums, const std::vector<uint32_t>& visibility, uint32_t n) {
  double total = 0.0; size_t counted = 0;
  for (size_t i = 0; i < visibility.size(); ++i) {
    if (!visibility[i]) continue;
    const double r = sums[4 * i], g = sums[4 * i + 1], b = sums[4 * i + 2], yy = sums[4 * i + 3];
    const double mean = (0.25 * r + 0.5 * g + 0.25 * b) / n;
    if (!(mean > 0.0) || !std::isfinite(mean) || !std::isfinite(yy)) continue;
    const double var = std::max(yy / n - mean * mean, 0.0) * (n > 1u ? (double)n / (n - 1u) : 1.0);
    total += std::sqrt(var / n) / mean; ++counted;
  }
  return counted ? total / (double)counted : -1.0;
}

// What the -accumulate line says about the sample set.  FrameIndex counts modulo M (RayTracer::UpdateFrame), and frame F at N samples takes
// the indices F N .. F N + N - 1: the still camera's frames repeat after M FRAMES whatever N is -- M N samples --, so the warning is for
// n > M frames.
std::string AccumulationSampleSetNote(uint32_t frames, uint32_t samplesPerPixel, uint32_t sampleSet) {
  char text[256];
  int len = std::snprintf(text, sizeof text, "; sample set of %u", sampleSet);
  if (frames > sampleSet)
    std::snprintf(text + len, sizeof text - (size_t)len, "\nwarning: %u frames of %u samples from a set of %u: the frames repeat after %u (%llu samples), -sampleset M up to %u extends it",
                  frames, samplesPerPixel, sampleSet, sampleSet, (unsigned long long)sampleSet * samplesPerPixel, RTGGX_MAX_SAMPLE_SET);
  return text;
}

bool RayTracedGGX::SaveConverged(const char* fileName) {
  rtggx_context* ctx = GetContext();
  if (!ctx) return false;
  uint32_t n = 0;
  if (rtggx_present_accumulation(ctx) != 0 || rtggx_accumulated_frames(ctx, &n) != 0) { std::fprintf(stderr, "SaveConverged: %s\n", rtggx_last_error()); return false; }
  if (!SaveImage(fileName)) return false;
  const size_t pixels = (size_t)m_width * m_height;
  std::vector<uint32_t> vis(pixels); std::vector<float> refl(4 * pixels), diff(4 * pixels);
  if (rtggx_readback(ctx, RTGGX_BUF_VISIBILITY, vis.data(), pixels * 4) != 0 || rtggx_readback(ctx, RTGGX_BUF_ACC_REFL, refl.data(), pixels * 16) != 0 ||
      rtggx_readback(ctx, RTGGX_BUF_ACC_DIFF, diff.data(), pixels * 16) != 0) { std::fprintf(stderr, "SaveConverged: %s\n", rtggx_last_error()); return false; }
  const double eR = meanRelativeStdError(refl, vis, n), eD = meanRelativeStdError(diff, vis, n);
  std::printf("accumulated %u frames: mean relative standard error of Y over covered pixels, reflection %.5f", n, eR);
  if (eD >= 0.0) std::printf(", diffuse %.5f", eD);
  std::printf("%s", AccumulationSampleSetNote(n, m_samplesPerPixel, m_rayTracer->GetSampleSetSize()).c_str());
  std::printf("\nwrote %s\n", fileName);
  std::fflush(stdout);
  return true;
}

bool RayTracedGGX::SaveImage(const char* fileName) {
  rtggx_context* ctx = GetContext();
  if (!ctx) return false;
  std::vector<uint32_t> px((size_t)m_width * m_height);
  if (rtggx_readback(ctx, RTGGX_BUF_BACKBUFFER, px.data(), px.size() * 4) != 0) { std::fprintf(stderr, "SaveImage: %s\n", rtggx_last_error()); return false; }
  const std::string name = fileName;
  if (name.size() >= 4 && name.compare(name.size() - 4, 4, ".png") == 0) {      // RGB, as the sample's screenshot (comp = 3)
    std::vector<uint8_t> rgb((size_t)m_width * m_height * 3);
    for (size_t i = 0; i < px.size(); ++i) { rgb[3 * i] = (uint8_t)px[i]; rgb[3 * i + 1] = (uint8_t)(px[i] >> 8); rgb[3 * i + 2] = (uint8_t)(px[i] >> 16); }
    return WritePng(fileName, m_width, m_height, 3, rgb.data());
  }
  FILE* f = std::fopen(fileName, "wb");
  if (!f) return false;
  std::fprintf(f, "P6\n%u %u\n255\n", m_width, m_height);
  std::vector<uint8_t> row((size_t)m_width * 3);
  for (uint32_t y = 0; y < m_height; ++y) {
    for (uint32_t x = 0; x < m_width; ++x) { const uint32_t p = px[(size_t)y * m_width + x]; row[3 * x] = (uint8_t)p; row[3 * x + 1] = (uint8_t)(p >> 8); row[3 * x + 2] = (uint8_t)(p >> 16); }
    std::fwrite(row.data(), 1, row.size(), f);
  }
  std::fclose(f);
  return true;
}
