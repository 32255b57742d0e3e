// capi_buffers.h -- the one owning type of the C boundary: a block of device (hipMalloc) or page-locked (hipHostMalloc) memory that is
// freed when its owner dies.  Every such block of bahip_context, of bahip_frame_planes and of the test hooks is a member or a local of
// this type, so none of them needs a line in a destructor, and growing one is one call of reserve().
#pragma once

#include <hip/hip_runtime.h>
#include <stdio.h>

#include <atomic>
#include <string>

namespace bahip_capi {

extern thread_local std::string g_last_error;   // bahip_last_error() (capi.hip)

// what the owning buffers of this process hold at the moment (bahip_debug_live_allocations): a buffer that is not freed shows here
inline std::atomic<long long> g_live_allocations{0}, g_live_bytes{0};

template <typename T> inline constexpr size_t kBufferElementBytes = sizeof(T);
template <> inline constexpr size_t kBufferElementBytes<void> = 1;   // untyped scratch: sized in bytes

template <typename T, bool kPinned>
class Buffer {
 public:
  Buffer() = default;
  explicit Buffer(unsigned host_malloc_flags) : flags_(host_malloc_flags) { static_assert(kPinned, "flags belong to page-locked memory"); }
  Buffer(Buffer&& other) noexcept : p_(other.p_), n_(other.n_), flags_(other.flags_) { other.p_ = nullptr; other.n_ = 0; }
  Buffer& operator=(Buffer&& other) noexcept {   // (the flags stay: they say what this buffer allocates next time)
    if (this != &other) { release(); p_ = other.p_; n_ = other.n_; other.p_ = nullptr; other.n_ = 0; }
    return *this;
  }
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { release(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t size() const { return n_; }   // elements allocated (bytes for T = void)

  void release() {
    if (p_) {
      if (kPinned) hipHostFree(p_); else hipFree(p_);
      g_live_allocations -= 1;
      g_live_bytes -= (long long)(kBufferElementBytes<T> * n_);
    }
    p_ = nullptr; n_ = 0;
  }
  // Gives the block up without freeing it, for the one caller that must leave memory to an operation it could not wait for.
  T* detach() {
    T* p = p_;
    if (p_) { g_live_allocations -= 1; g_live_bytes -= (long long)(kBufferElementBytes<T> * n_); }
    p_ = nullptr; n_ = 0;
    return p;
  }

  // Room for `need` elements: nothing happens while the block has them, otherwise a block of need + slack elements replaces it (the
  // contents are NOT carried over).  The new block is allocated FIRST and the old one freed on success, so a failed grow leaves the
  // buffer as it was; release_first frees before it allocates (for blocks so large that old and new must not exist together) and
  // leaves an empty buffer on failure.  Returns 1 with the error text set on failure; *reallocated says whether the memory is new.
  int reserve(size_t need, size_t slack, const char* what, bool release_first = false, bool* reallocated = nullptr) {
    if (reallocated) *reallocated = false;
    if (need <= n_ && p_) return 0;
    if (release_first) release();
    const size_t count = need + slack, bytes = kBufferElementBytes<T> * count;
    void* grown = nullptr;
    const hipError_t e = kPinned ? hipHostMalloc(&grown, bytes, flags_) : hipMalloc(&grown, bytes);
    if (e != hipSuccess) {
      char buf[160];
      snprintf(buf, sizeof(buf), "%s of %zu bytes for %s failed", kPinned ? "hipHostMalloc" : "hipMalloc", bytes, what);
      g_last_error = buf;
      return 1;
    }
    release();
    p_ = static_cast<T*>(grown); n_ = count;
    if (p_) { g_live_allocations += 1; g_live_bytes += (long long)bytes; }
    if (reallocated) *reallocated = true;
    return 0;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
  unsigned flags_ = hipHostMallocDefault;
};

template <typename T> using DeviceBuffer = Buffer<T, false>;
template <typename T> using PinnedBuffer = Buffer<T, true>;
constexpr unsigned kHostVisible = hipHostMallocMapped | hipHostMallocCoherent;   // page-locked memory the kernels write and the host polls

}  // namespace bahip_capi
