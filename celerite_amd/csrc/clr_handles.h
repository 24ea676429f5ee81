// celerite_amd/csrc/clr_handles.h -- owning handles of the HIP resources the host code keeps: device arrays, pinned host
// arrays, streams and events.  Each frees its resource when its owner goes away (a plan, a solver, a function's scope),
// so that no list of members has to be kept in step with a struct.  Nothing else in csrc/ calls hipFree, hipHostFree,
// hipStreamDestroy or hipEventDestroy: tests/test_host_api.py checks it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <algorithm>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>

#include "../../include/celerite_hip.h"

// the calling thread's last error message (api_misc.hip)
extern thread_local std::string clr_api_last_error;

namespace clr {

struct DeviceMemory {
  static constexpr const char* name = "hipMalloc";
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void* p) { (void)hipFree(p); }
};
struct PinnedMemory {
  static constexpr const char* name = "hipHostMalloc";
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
};

// Grow-only array of T: reserve(n) reallocates (contents not kept) only when n exceeds the capacity, release() frees it
// early, the destructor at the latest.  Returns a clr_status; a failed allocation leaves the array empty.
template <class T, class Memory = DeviceMemory>
struct Buffer {
  T* p = nullptr;
  size_t cap = 0;  // elements
  Buffer() = default;
  Buffer(Buffer&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  Buffer& operator=(Buffer&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~Buffer() { release(); }
  int reserve(size_t n) {
    if (n <= cap && p) return CLR_OK;
    release();
    const size_t want = std::max<size_t>(n, 1);
    const hipError_t e = Memory::alloc(reinterpret_cast<void**>(&p), want * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      clr_api_last_error = std::string(Memory::name) + "(" + std::to_string(want * sizeof(T)) + " bytes): " + hipGetErrorString(e);
      return CLR_HIP_ERROR;
    }
    cap = want;
    return CLR_OK;
  }
  void release() {
    if (p) Memory::free(p);
    p = nullptr;
    cap = 0;
  }
};
template <class T>
using PinnedBuffer = Buffer<T, PinnedMemory>;

struct StreamDeleter { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct EventDeleter { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDeleter>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDeleter>;

// create into an owner, which releases what it held before
inline hipError_t create_stream(Stream& s) {
  hipStream_t r = nullptr;
  const hipError_t e = hipStreamCreateWithFlags(&r, hipStreamNonBlocking);
  if (e == hipSuccess) s.reset(r);
  return e;
}
inline hipError_t create_event(Event& ev, unsigned flags = hipEventDefault) {
  hipEvent_t r = nullptr;
  const hipError_t e = hipEventCreateWithFlags(&r, flags);
  if (e == hipSuccess) ev.reset(r);
  return e;
}

static_assert(!std::is_copy_constructible<Buffer<double>>::value && !std::is_copy_assignable<Buffer<double>>::value,
              "a device array has one owner");
static_assert(!std::is_copy_constructible<PinnedBuffer<double>>::value && !std::is_copy_assignable<PinnedBuffer<double>>::value,
              "a pinned array has one owner");
static_assert(!std::is_copy_constructible<Stream>::value && !std::is_copy_assignable<Stream>::value, "a stream has one owner");
static_assert(!std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value, "an event has one owner");

}  // namespace clr
