// C entry points over the C++ host classes, for drivers that are not C++ (bench.py, tests):
// the frame entry stays RayTracedGGX::OnUpdate / OnRender.
#include <cstring>
#include <exception>
#include <string>
#include <vector>
#include "EnvImageLoader.h"
#include "ObjLoader.h"
#include "RayTracedGGX.h"
#include "Strips.h"

static thread_local std::string g_appError;

extern "C" {

const char* rtggx_app_last_error(void) { return g_appError.c_str(); }

// argv-style construction: the same flags as the RayTracedGGX executable.
void* rtggx_app_create(int argc, char** argv) {
  try {
    RayTracedGGX* app = new RayTracedGGX(1280, 720, "DXR Ray-Traced GGX");
    app->ParseCommandLineArgs(argv, argc);
    app->OnInit();
    return app;
  } catch (const std::exception& e) { g_appError = e.what(); return nullptr; }
}
void rtggx_app_destroy(void* h) { RayTracedGGX* app = (RayTracedGGX*)h; if (app) { app->OnDestroy(); delete app; } }
void rtggx_app_on_update(void* h) { ((RayTracedGGX*)h)->OnUpdate(); }
void rtggx_app_on_render(void* h) { ((RayTracedGGX*)h)->OnRender(); }
void rtggx_app_on_key_up(void* h, int key) { ((RayTracedGGX*)h)->OnKeyUp((uint8_t)key); }
void rtggx_app_on_lbutton_down(void* h, float x, float y) { ((RayTracedGGX*)h)->OnLButtonDown(x, y); }
void rtggx_app_on_lbutton_up(void* h, float x, float y) { ((RayTracedGGX*)h)->OnLButtonUp(x, y); }
void rtggx_app_on_mouse_move(void* h, float x, float y) { ((RayTracedGGX*)h)->OnMouseMove(x, y); }
void rtggx_app_on_mouse_wheel(void* h, float dz, float x, float y) { ((RayTracedGGX*)h)->OnMouseWheel(dz, x, y); }
int rtggx_app_load_track(void* h, const char* path) { return ((RayTracedGGX*)h)->LoadTrack(path) ? 0 : -1; }
// The camera handlers on their own (no device): events = n x (type, a, b) with type 1 down, 2 up, 3 move, 4 wheel;
// returns the eye point and the view matrix (row-major) they lead to from the sample's initial camera.
void rtggx_host_camera(uint32_t width, uint32_t height, const float* events, uint32_t n, float* eye3, float* view16) {
  RayTracedGGX app(width, height, "");
  app.InitCamera();
  for (uint32_t i = 0; i < n; ++i) {
    const float* e = events + 3 * i;
    switch ((int)e[0]) { case 1: app.OnLButtonDown(e[1], e[2]); break; case 2: app.OnLButtonUp(e[1], e[2]); break;
                         case 3: app.OnMouseMove(e[1], e[2]); break; case 4: app.OnMouseWheel(e[1], 0.0f, 0.0f); break; default: app.OnMouseLeave(); }
  }
  eye3[0] = app.GetEyePt().x; eye3[1] = app.GetEyePt().y; eye3[2] = app.GetEyePt().z;
  std::memcpy(view16, app.GetView().r, 64);
}
void rtggx_app_set_time_step(void* h, float dt) { ((RayTracedGGX*)h)->SetFixedTimeStep(dt); }
void* rtggx_app_context(void* h) { return ((RayTracedGGX*)h)->GetContext(); }
void rtggx_app_size(void* h, uint32_t* w, uint32_t* ht) { *w = ((RayTracedGGX*)h)->GetWidth(); *ht = ((RayTracedGGX*)h)->GetHeight(); }
void rtggx_app_frame_constants(void* h, void* out768) { std::memcpy(out768, &((RayTracedGGX*)h)->GetRayTracer()->GetFrameConstants(), sizeof(RtggxFrameConstants)); }
int rtggx_app_set_dump_prefix(void* h, const char* prefix) { ((RayTracedGGX*)h)->SetDumpPrefix(prefix ? prefix : ""); return 0; }
const char* rtggx_app_last_screen_shot(void* h) { return ((RayTracedGGX*)h)->GetLastScreenShot().c_str(); }
int rtggx_app_save_converged(void* h, const char* path) { return ((RayTracedGGX*)h)->SaveConverged(path) ? 0 : -1; }
int rtggx_app_save_image(void* h, const char* path) { return ((RayTracedGGX*)h)->SaveImage(path) ? 0 : -1; }

int rtggx_app_save_reference(void* h, const char* path) { return ((RayTracedGGX*)h)->SaveReference(path) ? 0 : -1; }
int rtggx_app_flush_scores(void* h) { return ((RayTracedGGX*)h)->FlushScores() ? 0 : -1; }
// RayTracer::SetReference / SetScoring / ReadScores of the application's ray tracer (capacity records of 120 bytes at `out`)
int rtggx_app_set_reference(void* h, const void* rgba16f, size_t bytes) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (rt->SetReference(rgba16f, bytes)) return 0;
  g_appError = rt->GetLastError(); return -1;
}
int rtggx_app_set_scoring(void* h, int enable) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (rt->SetScoring(enable != 0)) return 0;
  g_appError = rt->GetLastError(); return -1;
}
int rtggx_app_read_scores(void* h, void* out, uint32_t capacity, uint32_t* count) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (!count || (!out && capacity)) { g_appError = "rtggx_app_read_scores: null result"; return -1; }
  if (rtggx_read_scores(rt->GetContext(), (RtggxScore*)out, capacity, count) == 0) return 0;
  g_appError = rtggx_last_error(); return -1;
}
// The PFM writer and reader on their own (no device): w x h RGBA16F words out of / into `rgba16f`.
int rtggx_host_write_pfm(const char* path, uint32_t w, uint32_t h, const uint16_t* rgba16f) { return WritePfm(path, w, h, rgba16f) ? 0 : -1; }
int rtggx_host_read_pfm(const char* path, uint32_t w, uint32_t h, uint16_t* rgba16f) {
  std::vector<uint16_t> image; std::string error;
  if (!ReadPfm(path, w, h, image, error)) { g_appError = error; return -1; }
  std::memcpy(rgba16f, image.data(), image.size() * 2);
  return 0;
}

// The Radiance / PFM readers on their own (no device): the image's pixel format (0 RGBE8, 1 RGB32F), size, the layout its aspect ratio
// tells (0 panorama, 1 vertical cross, 2 horizontal cross, -1 none) and the bytes it takes; the pixels, rows top to bottom, are copied
// where `capacity` holds them (call once with 0 for the size).
int rtggx_host_load_env_image(const char* path, int* pixels, uint32_t* width, uint32_t* height, int* layout, void* data, size_t capacity, size_t* bytes) {
  EnvImage::Image image; std::string error;
  if (!EnvImage::LoadFromFile(path, image, error)) { g_appError = error; return -1; }
  if (pixels) *pixels = image.pixels;
  if (width) *width = image.width;
  if (height) *height = image.height;
  if (layout) *layout = EnvImage::LayoutFromAspect(image.width, image.height);
  if (bytes) *bytes = image.data.size();
  if (data && capacity >= image.data.size()) std::memcpy(data, image.data.data(), image.data.size());
  return 0;
}

int rtggx_host_write_png(const char* path, uint32_t w, uint32_t h, uint32_t comp, const uint8_t* pixels) { return WritePng(path, w, h, comp, pixels) ? 0 : -1; }

// Host-only pieces, usable without a GPU: the OBJ importer and the Halton sequence.
static ObjLoader g_obj;
int rtggx_host_obj_import(const char* path, uint32_t* numVerts, uint32_t* numIndices, float* aabb6) {
  g_obj = ObjLoader();
  if (!g_obj.Import(path, true, true)) { g_appError = std::string("cannot import ") + path; return -1; }
  *numVerts = g_obj.GetNumVertices(); *numIndices = g_obj.GetNumIndices();
  if (aabb6) { const ObjLoader::AABB& a = g_obj.GetAABB(); aabb6[0] = a.Min.x; aabb6[1] = a.Min.y; aabb6[2] = a.Min.z; aabb6[3] = a.Max.x; aabb6[4] = a.Max.y; aabb6[5] = a.Max.z; }
  return 0;
}
void rtggx_host_obj_copy(float* verts, uint32_t* indices) {
  std::memcpy(verts, g_obj.GetVertices(), (size_t)g_obj.GetNumVertices() * 24);
  std::memcpy(indices, g_obj.GetIndices(), (size_t)g_obj.GetNumIndices() * 4);
}
void rtggx_host_halton(uint32_t n, float* xy) { HaltonSequence h; for (uint32_t i = 0; i < n; ++i) h.Next(xy[2 * i], xy[2 * i + 1]); }

// RayTracer::UpdateFrame on its own (constants only, no device): `frames` consecutive frames with a
// fixed time step and the default camera; writes frames x 768 bytes.
class ConstantsOnlyRayTracer : public RayTracer {
 public:
  void Setup(uint32_t w, uint32_t h, const float* ps) { m_width = w; m_height = h; std::memcpy(m_posScale, ps, 16); }
};
}  // extern "C"

// UpdateFrame calls rtggx_update_frame; with a null context that call only reports an error, the constants are still produced.
extern "C" void rtggx_host_frame_constants(uint32_t width, uint32_t height, const float* posScale4, const float* eye3, const float* focus3,
                                           float dt, uint32_t frames, void* out) {
  ConstantsOnlyRayTracer rt; rt.Setup(width, height, posScale4);
  const xm::Float3 eye{eye3[0], eye3[1], eye3[2]}, focus{focus3[0], focus3[1], focus3[2]};
  const xm::Matrix proj = xm::PerspectiveFovLH(0.785398163f, (float)width / (float)height, 1.0f, 1000.0f);
  const xm::Matrix view = xm::LookAtLH(eye, focus, xm::Float3{0.0f, 1.0f, 0.0f});
  for (uint32_t f = 0; f < frames; ++f) {
    rt.UpdateFrame((uint8_t)(f % 3), eye, view * proj, dt);
    std::memcpy((char*)out + 768 * (size_t)f, &rt.GetFrameConstants(), 768);
  }
}

// RayTracer::SetSampleSetSize and the frame counter behind it (no device): the FrameIndex of `frames` consecutive UpdateFrame calls after
// SetSampleSetSize(size); returns the size the RayTracer then holds (a refused size leaves 256).
extern "C" uint32_t rtggx_host_frame_indices(uint32_t size, uint32_t frames, uint32_t* out) {
  ConstantsOnlyRayTracer rt; const float ps[4] = {0.0f, 0.0f, 0.0f, 1.0f}; rt.Setup(64, 36, ps);
  rt.SetSampleSetSize(size);
  const xm::Float3 eye{10.0f, 10.0f, -24.0f};
  const xm::Matrix viewProj = xm::LookAtLH(eye, xm::Float3{0.0f, 3.0f, 0.0f}, xm::Float3{0.0f, 1.0f, 0.0f}) * xm::PerspectiveFovLH(0.785398163f, 64.0f / 36.0f, 1.0f, 1000.0f);
  for (uint32_t f = 0; f < frames; ++f) { rt.UpdateFrame((uint8_t)(f % 3), eye, viewProj, 0.0f); out[f] = rt.GetFrameConstants().global.FrameIndex; }
  return rt.GetSampleSetSize();
}

// The tail of the -accumulate line (AccumulationSampleSetNote) for `frames` accumulated frames of `samples` samples from a set of `sampleSet`.
extern "C" int rtggx_host_accumulation_note(uint32_t frames, uint32_t samples, uint32_t sampleSet, char* out, int capacity) {
  const std::string s = AccumulationSampleSetNote(frames, samples, sampleSet);
  if ((int)s.size() + 1 > capacity) return -1;
  std::memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

// RayTracer::SetSampleMap of the application's ray tracer (counts = NULL, 0, 0 clears)
extern "C" int rtggx_app_set_sample_map(void* h, const uint8_t* counts, uint32_t blocksX, uint32_t blocksY) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (rt->SetSampleMap(counts, blocksX, blocksY)) return 0;
  g_appError = rt->GetLastError();
  return -1;
}

// RayTracer::SetLights of the application's ray tracer (lights = NULL, 0 turns them off)
extern "C" int rtggx_app_set_lights(void* h, const RtggxLight* lights, uint32_t count) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (rt->SetLights(lights, count)) return 0;
  g_appError = rt->GetLastError();
  return -1;
}

// RayTracer::SetLightList of the application's ray tracer (lights = NULL, 0 clears the list)
extern "C" int rtggx_app_set_light_list(void* h, const RtggxLight* lights, uint32_t count) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (rt->SetLightList(lights, count)) return 0;
  g_appError = rt->GetLastError();
  return -1;
}

// RayTracer::SetLightReflections of the application's ray tracer
extern "C" int rtggx_app_set_light_reflections(void* h, int enable) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (enable != 0 && enable != 1) { g_appError = "rtggx_app_set_light_reflections: 0 or 1"; return -1; }
  if (rt->SetLightReflections(enable == 1)) return 0;
  g_appError = rt->GetLastError();
  return -1;
}

// RayTracer::SetLightSampling of the application's ray tracer
extern "C" int rtggx_app_set_light_sampling(void* h, int mode) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (mode != 0 && mode != 1) { g_appError = "rtggx_app_set_light_sampling: 0 or 1"; return -1; }
  if (rt->SetLightSampling(mode)) return 0;
  g_appError = rt->GetLastError();
  return -1;
}

// RayTracer::SetLightPickVisibility of the application's ray tracer
extern "C" int rtggx_app_set_light_pick_visibility(void* h, int enable) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (enable != 0 && enable != 1) { g_appError = "rtggx_app_set_light_pick_visibility: 0 or 1"; return -1; }
  if (rt->SetLightPickVisibility(enable == 1)) return 0;
  g_appError = rt->GetLastError();
  return -1;
}

// RayTracer::SetLightListVisibility of the application's ray tracer
extern "C" int rtggx_app_set_light_list_visibility(void* h, int enable) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (enable != 0 && enable != 1) { g_appError = "rtggx_app_set_light_list_visibility: 0 or 1"; return -1; }
  if (rt->SetLightListVisibility(enable == 1)) return 0;
  g_appError = rt->GetLastError();
  return -1;
}

// RayTracer::UpdateLightList, UpdateLightListDevice and ReadLightList of the application's ray tracer
extern "C" int rtggx_app_update_light_list(void* h, const RtggxLight* lights, uint32_t first, uint32_t count) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (rt->UpdateLightList(lights, first, count)) return 0;
  g_appError = rt->GetLastError();
  return -1;
}
extern "C" int rtggx_app_update_light_list_device(void* h, const RtggxLight* deviceLights, uint32_t first, uint32_t count, uint32_t kinds, void* stream) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (rt->UpdateLightListDevice(deviceLights, first, count, kinds, stream)) return 0;
  g_appError = rt->GetLastError();
  return -1;
}
extern "C" int rtggx_app_read_light_list(void* h, RtggxLight* out, size_t bytes) {
  RayTracer* rt = ((RayTracedGGX*)h)->GetRayTracer();
  if (rt->ReadLightList(out, bytes)) return 0;
  g_appError = rt->GetLastError();
  return -1;
}

// The multi-GPU host's plan functions (host/Strips.cpp), for the tests that compare them with raytracedggx_amd/strips.py.
// bounds: nullptr / 0 for equal strips, else world + 1 row numbers.  ops: 5 int32 per transfer (send, buffer: 1 history / 0 back buffer / 2 token, rowBegin, rowEnd, peer);
// returns the number of transfers, or -1 with rtggx_app_last_error set.
extern "C" int rtggx_host_exchange_plan(uint32_t height, int rank, int world, uint32_t apron, const uint32_t* bounds, int32_t* ops, int capacity) {
  try {
    const std::vector<uint32_t> b(bounds, bounds + (bounds ? world + 1 : 0));
    const std::vector<strips::Op> plan = strips::ExchangePlan(height, rank, world, apron, &b);
    if ((int)plan.size() > capacity) { g_appError = "rtggx_host_exchange_plan: capacity"; return -1; }
    for (size_t i = 0; i < plan.size(); ++i) { int32_t* o = ops + 5 * i; o[0] = plan[i].send; o[1] = plan[i].buffer == strips::Buffer::History ? 1 : plan[i].buffer == strips::Buffer::BackBuffer ? 0 : 2; o[2] = (int32_t)plan[i].rowBegin; o[3] = (int32_t)plan[i].rowEnd; o[4] = plan[i].peer; }
    return (int)plan.size();
  } catch (const std::exception& e) { g_appError = e.what(); return -1; }
}
extern "C" int rtggx_host_balanced_bounds(const double* rowCost, uint32_t height, int world, uint32_t minRows, double firstExtra, uint32_t* boundsOut) {
  try {
    const std::vector<uint32_t> b = strips::BalancedBounds(std::vector<double>(rowCost, rowCost + height), world, minRows, firstExtra);
    for (size_t i = 0; i < b.size(); ++i) boundsOut[i] = b[i];
    return 0;
  } catch (const std::exception& e) { g_appError = e.what(); return -1; }
}
