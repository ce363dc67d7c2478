// What the four translation units behind the C ABI (context.hip, mesh.hip, frame.hip, debug.hip) share among each other and with nobody else.
#pragma once
#include "rtggx_context.h"

// The events that order the streams of one context among each other, and the frames-in-flight fence.  (Measured in round 4: with
// hipEventReleaseToDevice the 1080p frame gets SLOWER, 0.184 -> 0.191-0.197 ms; hipEventDisableSystemFence changes nothing.)
#define RT_EVENT_FLAGS (hipEventDisableTiming)
#define RT_CHECK_CTX(c) do { if (!(c)) { rt::setError("null context"); return -1; } hipError_t _e = hipSetDevice((c)->device); if (_e != hipSuccess) { rt::setError("hipSetDevice: %s", hipGetErrorString(_e)); return -2; } } while (0)

namespace rt {
int allocSet(rtggx_context* c, uint32_t i);                                 // context.hip
extern const float kGroundVerts[24][6]; extern const uint32_t kGroundIdx[36];      // mesh.hip
int setMeshImpl(rtggx_context* c, uint32_t slot, const float* verts, uint32_t nv, const uint32_t* idx, uint32_t ni);
int issuePendingRefits(rtggx_context* c, bool* touched);
int issueRebuildSteps(rtggx_context* c);
hipError_t syncStreams(rtggx_context* c);                                   // frame.hip
int ensureParams(rtggx_context* c);
}  // namespace rt
