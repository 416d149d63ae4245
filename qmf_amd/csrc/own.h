// Move-only owners of HIP resources: device memory, pinned host memory, events and streams.
// An owner converts to the raw handle, which is what the runtime calls and the kernel
// argument structs take; the resource is released when the owner goes out of scope.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <type_traits>

namespace qmfx {

template <typename T, typename Release>
struct Owned : std::unique_ptr<T, Release> {
  using std::unique_ptr<T, Release>::unique_ptr;
  operator T*() const { return this->get(); }
  // an untyped buffer (DevPtr<void>) seen in the context precision
  template <typename U>
  U* as() const {
    return static_cast<U*>(this->get());
  }
};

struct DevFree {
  void operator()(void* p) const { (void)hipFree(p); }
};
struct PinnedFree {
  void operator()(void* p) const { (void)hipHostFree(p); }
};
struct EventDestroy {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};
struct StreamDestroy {
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
template <typename T>
using DevPtr = Owned<T, DevFree>;
template <typename T>
using PinnedPtr = Owned<T, PinnedFree>;
using Event = Owned<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using Stream = Owned<std::remove_pointer_t<hipStream_t>, StreamDestroy>;

// Each of these releases what the owner held, then takes the new resource on success.
template <typename T>
hipError_t dev_alloc(DevPtr<T>& p, size_t bytes) {
  p.reset();
  void* raw = nullptr;
  const hipError_t e = hipMalloc(&raw, bytes);
  if (e == hipSuccess) p.reset(static_cast<T*>(raw));
  return e;
}
// Device scratch that knows its size: the buffer and the bytes it holds (ctx.h's reserve()
// grows it on demand).  Converts like the owner it is, so argument code reads the same.
template <typename T>
struct Scratch : DevPtr<T> {
  size_t bytes = 0;
};
template <typename T>
hipError_t pinned_alloc(PinnedPtr<T>& p, size_t bytes) {
  p.reset();
  void* raw = nullptr;
  const hipError_t e = hipHostMalloc(&raw, bytes);
  if (e == hipSuccess) p.reset(static_cast<T*>(raw));
  return e;
}
inline hipError_t make_event(Event& ev, unsigned flags = hipEventDefault) {
  ev.reset();
  hipEvent_t raw = nullptr;
  const hipError_t e = hipEventCreateWithFlags(&raw, flags);
  if (e == hipSuccess) ev.reset(raw);
  return e;
}
inline hipError_t make_stream(Stream& st) {
  st.reset();
  hipStream_t raw = nullptr;
  const hipError_t e = hipStreamCreateWithFlags(&raw, hipStreamNonBlocking);
  if (e == hipSuccess) st.reset(raw);
  return e;
}

}  // namespace qmfx
