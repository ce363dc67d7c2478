// Headless frame driver with the reference's entry points (RayTracedGGX/RayTracedGGX.h:27-146,
// DXFramework virtuals RayTracedGGX/Common/DXFramework.h:23-26): OnInit / OnUpdate / OnRender /
// OnDestroy, the same command line (RayTracedGGX.cpp:462-511) and the same defaults
// (RayTracedGGX.cpp:37-39, camera :19-23, 267-277).  What the window supplied interactively is
// supplied by extra flags: -width -height -frames -dt -metallic -sharedmem -sync -vndf -rayrate -sun -sunreflections -sunfromenv -sunangle -light -spot -lightreflections -lightpick -lightvisibility -lightlist -lightlistvisibility -lightlistorbit -recursion -spp -sampleset -accumulate -savereference -reference -score -envlayout -envsize -envmips -envprefilter -device -dump -track -deform -gpus -strips -balance.
#pragma once
#include <vector>
#include <cstdint>
#include <memory>
#include <string>
#include "Denoiser.h"
#include "RayTracer.h"
#include "XMath.h"

bool WritePng(const char* fileName, uint32_t w, uint32_t h, uint32_t comp, const uint8_t* pixels);   // comp 3 (RGB) or 4 (RGBA), 8 bits

// PFM, the float container of a reference image (-savereference / -reference): "PF", width and height, scale -1.0 (little-endian), then rows
// bottom to top of fp32 rgb.  The images here are RGBA16F words (the layout of RTGGX_BUF_CONVERGED): every half is exact in fp32, so writing
// and reading gives the halves back; on load any fp32 value is rounded to nearest even into a half and alpha is 1.  ReadPfm refuses a missing,
// malformed or truncated file, a size other than w x h and a non-negative (big-endian) scale, and says why in `error`.
bool WritePfm(const char* fileName, uint32_t w, uint32_t h, const uint16_t* rgba16f);
bool ReadPfm(const char* fileName, uint32_t w, uint32_t h, std::vector<uint16_t>& rgba16f, std::string& error);

// the tail of the line -accumulate prints: "; sample set of M", and a warning once more than M frames were accumulated (they repeat)
std::string AccumulationSampleSetNote(uint32_t frames, uint32_t samplesPerPixel, uint32_t sampleSet);

class RayTracedGGX {
 public:
  RayTracedGGX(uint32_t width, uint32_t height, std::string name);
  virtual ~RayTracedGGX();

  virtual void OnInit();
  virtual void OnUpdate();
  virtual void OnRender();
  virtual void OnDestroy();
  virtual void OnKeyUp(uint8_t key);
  // camera interactions of the sample's window (RayTracedGGX.h:58-63, .cpp:400-455): positions in pixels
  virtual void OnLButtonDown(float posX, float posY);
  virtual void OnLButtonUp(float posX, float posY);
  virtual void OnMouseMove(float posX, float posY);
  virtual void OnMouseWheel(float deltaZ, float posX, float posY);
  virtual void OnMouseLeave();
  void InitCamera();                                 // projection and view of LoadAssets (RayTracedGGX.cpp:262-277)
  const xm::Float3& GetEyePt() const { return m_eyePt; }
  const xm::Matrix& GetView() const { return m_view; }
  // Scripted input (replaces the message loop): a text file, one event per line, applied by OnUpdate before the frame
  // with that number:  <frame> key <code | SPACE LEFT RIGHT UP DOWN V A> | down x y | up x y | move x y | wheel dz | leave
  bool LoadTrack(const std::string& fileName);

  void ParseCommandLineArgs(char* argv[], int argc);

  bool IsInitialized() const { return m_initialized; }
  uint32_t GetWidth() const { return m_width; }
  uint32_t GetHeight() const { return m_height; }
  uint32_t GetNumFrames() const { return m_numFrames; }
  const std::string& GetDumpPrefix() const { return m_dumpPrefix; }
  void SetDumpPrefix(const std::string& prefix) { m_dumpPrefix = prefix; }
  const std::string& GetLastScreenShot() const { return m_lastScreenShot; }
  // multi-GPU (host/Strips.h): -gpus N (one process per GPU), what the launcher hands a rank, the single-process mode
  int GetNumGpus() const { return m_gpus; }
  int GetRank() const { return m_rank; }
  const std::string& GetIdFile() const { return m_idFile; }
  int GetNumStrips() const { return m_strips; }
  bool GetBalance() const { return m_balance; }
  RayTracer* GetRayTracer() const { return m_rayTracer.get(); }
  rtggx_context* GetContext() const { return m_rayTracer ? m_rayTracer->GetContext() : nullptr; }
  void SetFixedTimeStep(float dt) { m_fixedTimeStep = dt; }
  // -accumulate N: the mean of the accumulated frames presented (rtggx_present_accumulation) and its tone map written like SaveImage's; one
  // line on stdout: the frame count and the mean relative standard error of Y over covered pixels, from the sums, in double (per image;
  // it divides by the count of all accumulated frames, so it assumes materials that did not change since the last reset)
  uint32_t GetAccumulate() const { return m_accumulate; }
  bool SaveConverged(const char* fileName);
  // -savereference <file.pfm>: RTGGX_BUF_CONVERGED as SaveConverged left it, as a PFM file
  const std::string& GetSaveReference() const { return m_saveReferenceFile; }
  bool SaveReference(const char* fileName);
  // -score <file.jsonl>: the records rtggx_read_scores hands out, one JSON line per frame appended to the file; OnRender calls it every
  // RTGGX_SCORE_RING frames, the caller once more at the end of the run (OnDestroy does)
  bool FlushScores();
  bool SaveImage(const char* fileName);   // tone-mapped back buffer as PNG (name ends in .png) or binary PPM (screenshot, RayTracedGGX.cpp:719-739)

 protected:
  static const uint8_t FrameCount = RayTracer::FrameCount;

  uint32_t m_width, m_height;
  std::string m_title;
  std::unique_ptr<RayTracer> m_rayTracer;
  std::unique_ptr<Denoiser> m_denoiser;
  uint8_t m_frameIndex = 0;
  bool m_initialized = false;

  // toggles of the reference (RayTracedGGX.h:118-124)
  int m_asyncCompute = 1;
  uint32_t m_currentMesh = 0;
  bool m_useSharedMem = false;
  bool m_isPaused = false;
  uint32_t m_screenShot = 0;           // RayTracedGGX.h:123; set by [F11]
  std::string m_lastScreenShot;        // the file the last [F11] wrote
  float m_metallics[RayTracer::NUM_MESH];

  // camera (RayTracedGGX.h:100-104)
  xm::Matrix m_proj, m_view;
  xm::Float3 m_focusPt, m_eyePt;
  bool m_tracking = false;
  float m_mousePt[2] = {0.0f, 0.0f};
  struct TrackEvent { uint32_t frame; int type; float a, b; };   // type: 0 key, 1 down, 2 up, 3 move, 4 wheel, 5 leave
  std::vector<TrackEvent> m_track;
  size_t m_trackNext = 0;
  uint32_t m_frameNumber = 0;
  std::string m_trackFileName;

  // command line
  std::string m_meshFileName = "Assets/dragon.obj";
  std::string m_envFileName = "Assets/rnl_cross.dds";
  // -env takes a DDS cube, a Radiance .hdr or a .pfm image (told by the file's first bytes).  -envlayout <equirect|vcross|hcross>: the layout
  // of an image whose aspect ratio is none of 2:1, 3:4, 4:3; -envsize <1..4096>: the side of the cube a panorama is resampled to (refused
  // with a cross); -envmips: a DDS cube with fewer levels than a full chain gets it built on the device (RayTracer::SetEnvOptions);
  // -envprefilter [N]: the levels below level 0 rebuilt as the GGX-prefiltered radiance, N samples per texel (a power of two from 64 to 4096,
  // 1024 without a number; 0 here: off), DDS cube or image, every rank of -gpus / -strips; it implies -envmips
  int m_envLayout = -1; uint32_t m_envSize = 0; bool m_envMips = false; uint32_t m_envPrefilter = 0;
  float m_meshPosScale[4] = {0.0f, 0.0f, 0.0f, 1.0f};
  uint32_t m_numFrames = 1;
  float m_fixedTimeStep = 1.0f / 60.0f;   // the reference steps by the wall clock (StepTimer); fixed here for reproducible runs
  int m_device = 0;
  std::string m_dumpPrefix;
  int m_gpus = 1, m_rank = -1, m_strips = 1; bool m_balance = true; std::string m_idFile;
  bool m_hasMetallicOverride = false;
  bool m_vndf = false;                 // -vndf
  uint32_t m_recursionDepth = 1;       // -recursion <1..4>: levels of rays per path (RayTracer::SetMaxRecursionDepth)
  uint32_t m_samplesPerPixel = 1;      // -spp <1|2|4|8>: samples per covered pixel (RayTracer::SetSamplesPerPixel); not together with -rayrate 4
  uint32_t m_sampleSet = RTGGX_MIN_SAMPLE_SET;      // -sampleset <256..65536, a power of two>: the size of the sample set (RayTracer::SetSampleSetSize); every rank of -gpus / -strips gets it
  uint32_t m_accumulate = 0;           // -accumulate <N>: accumulation on for the last N frames of the run (all of them when N >= -frames); not with -rayrate 4, -gpus, -strips
  // -reference <file.pfm>: the image every frame is scored against (RayTracer::SetReference), read -- and refused -- while the command line is
  // parsed; -score <file.jsonl>: scoring on from frame 0 (needs -reference); -savereference <file.pfm>: needs -accumulate.  -reference and
  // -score: whole frames on one GPU only, not with -gpus / -strips
  std::string m_referenceFile, m_scoreFile, m_saveReferenceFile;
  std::vector<uint16_t> m_referenceImage;
  bool m_scoreFileStarted = false;
  bool m_sunReflections = false;      // -sunreflections: the sun at the surfaces seen in reflections as well (RayTracer::SetSunReflections); needs -sun
  float m_sun[6] = {}; bool m_hasSun = false;      // -sun <x> <y> <z> <r> <g> <b>: direction toward the sun and irradiance (RayTracer::SetSun); not together with -rayrate 4
  // -sunfromenv [degrees]: the sun's direction and irradiance measured from the -env cube, the sun taken out of the cube (before
  // -envprefilter filters it) and set as the light (RayTracer::SetSunFromEnvironment); degrees: the half-angle of the cone about the brightest
  // texel, in (0, 45], 0 here = the library's default of 4; not together with -sun or -rayrate 4; -sunreflections is accepted with it
  bool m_sunFromEnv = false; float m_sunFromEnvCone = 0.0f;
  // -sunangle <degrees>: the angular radius of the sun's disk, 0 to 10 -- soft shadows (RayTracer::SetSunAngle); needs -sun or -sunfromenv,
  // and -sunfromenv sets none by itself: its cone is a policy default, not a measurement of the disk
  float m_sunAngle = 0.0f; bool m_hasSunAngle = false;
  // -light <x> <y> <z> <r> <g> <b> <range> [<radius>] and -spot <x> <y> <z> <r> <g> <b> <range> <radius> <ax> <ay> <az> <outer degrees>
  // <inner degrees>: point and spot lights inside the scene with ray-traced shadows (RayTracer::SetLights); both repeatable, up to
  // RTGGX_MAX_LIGHTS lights in the order typed; not together with -rayrate 4
  std::vector<RtggxLight> m_lights;
  bool m_lightReflections = false;    // -lightreflections: the lights at the surfaces seen in reflections as well (RayTracer::SetLightReflections); needs -light or -spot
  bool m_lightPick = false;           // -lightpick: one shadow ray per surface point for all lights (RayTracer::SetLightSampling(1)); needs -light or -spot
  bool m_lightVisibility = false;     // -lightvisibility: the pick weighted by the visibility each pixel remembers (RayTracer::SetLightPickVisibility); needs -lightpick; whole frames only
  // -lightlist <file>: a light list beyond eight -- up to RTGGX_MAX_LIGHT_LIST lines "light x y z r g b range [radius]" or "spot x y z r g b
  // range radius ax ay az outer inner" (RayTracer::SetLightList); not together with -light / -spot or -rayrate 4; -lightreflections is
  // accepted with it
  std::string m_lightListFile; std::vector<RtggxLight> m_lightList;
  // -lightlistorbit <degrees per frame>: before frame n the file's list turned about the world y axis by n x degrees, positions and spot
  // axes, computed from the originals in double (RayTracer::UpdateLightList: no wait, the records' history kept); needs -lightlist
  double m_lightListOrbit = 0.0; bool m_lightListOrbitGiven = false; std::vector<RtggxLight> m_lightListMoved;
  bool m_lightListVisibility = false; // -lightlistvisibility: the list's pick weighted by the sparse record each pixel keeps (RayTracer::SetLightListVisibility); needs -lightlist; whole frames only
  uint32_t m_rayRate = 1;              // -rayrate <1|4>: pixels per traced ray (RayTracer::SetRayRate); 4 renders whole frames only: not with -gpus / -strips
  // -deform <amplitude>: the model breathes -- a travelling sine wave through its vertices, DeformPeriod key shapes computed once
  // at start-up and handed to RayTracer::UpdateMesh one per frame (per-frame host cost: one copy of the vertex array)
  float m_deformAmplitude = 0.0f;
  static const uint32_t DeformPeriod = 32;
  std::vector<std::vector<float>> m_deformShapes;
};
