// The owners of everything librtggx gets from the HIP runtime (rt_owned.h), and the only place that calls the runtime's allocation and
// release functions.  The helpers return the runtime's code for RT_HIP (rtggx_context.h) or for a caller's own message; an owner that
// fails to fill stays empty.  Rule for several resources that belong together: allocate into locals, move them into the members when
// all have succeeded -- a failure on the way releases the locals and leaves the members as they were (DESIGN.md "Ownership").
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "rt_owned.h"
namespace rt {
struct FreeDevice { void operator()(void* p) const { hipFree(p); } };
struct FreePinned { void operator()(void* p) const { hipHostFree(p); } };
struct DestroyEvent { void operator()(hipEvent_t e) const { hipEventDestroy(e); } };
struct DestroyStream { void operator()(hipStream_t s) const { hipStreamDestroy(s); } };
struct CloseIpc { void operator()(void* p) const { hipIpcCloseMemHandle(p); } };
template <class T> using DevBuf = Owned<T*, FreeDevice>;
template <class T> using PinnedBuf = Owned<T*, FreePinned>;
using Event = Owned<hipEvent_t, DestroyEvent>;
using Stream = Owned<hipStream_t, DestroyStream>;
using IpcMapping = Owned<void*, CloseIpc>;

template <class T> struct ElementSize { static constexpr size_t value = sizeof(T); };
template <> struct ElementSize<void> { static constexpr size_t value = 1; };      // untyped buffers count bytes
// `count` elements; what the owner held is released first.
template <class T> inline hipError_t alloc(DevBuf<T>& b, size_t count) { return hipMalloc(b.put(), count * ElementSize<T>::value); }
template <class T> inline hipError_t alloc(PinnedBuf<T>& b, size_t count) { return hipHostMalloc(b.put(), count * ElementSize<T>::value); }
// ... and every byte set to `byte`.  The clear runs on the null stream, which a context's non-blocking streams are not ordered against, and
// does not wait on the host: whoever needs it done synchronises the null stream himself, once behind all his clears.
template <class T> inline hipError_t allocFilled(DevBuf<T>& b, size_t count, int byte = 0) {
  const hipError_t e = alloc(b, count);
  return e != hipSuccess ? e : hipMemset(b, byte, count * ElementSize<T>::value);
}
inline hipError_t create(Event& e, unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(e.put(), flags); }
inline hipError_t create(Stream& s, unsigned flags, int priority) { return hipStreamCreateWithPriority(s.put(), flags, priority); }
}  // namespace rt
