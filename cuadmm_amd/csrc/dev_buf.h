// Owning wrappers of device memory, pinned memory and events, and the small host helpers every engine unit uses.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <vector>

#include "device_util.h"

namespace cuadmm {

inline double wall_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  int alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return CUADMM_OK;
    CUADMM_HIP_TRY(hipMalloc(&p, sizeof(T) * count));
    return CUADMM_OK;
  }
  int grow(size_t count) { return n < count ? alloc(count) : CUADMM_OK; }      // at least count elements; a larger buffer loses its contents
  int upload(const T* h, size_t count) {
    if (count == 0) return CUADMM_OK;
    return staged_h2d(p, h, sizeof(T) * count);   // never hipMemcpy on caller / vector memory (staging.hip)
  }
  int from(const std::vector<T>& h, size_t pad = 0) {   // pad: extra (zeroed) elements behind the data
    int rc = alloc(h.size() + pad);
    if (rc) return rc;
    n = h.size();
    if (pad) CUADMM_HIP_TRY(hipMemset(p + h.size(), 0, sizeof(T) * pad));
    return upload(h.data(), h.size());
  }
  void release() {
    if (p) { hipError_t e = hipFree(p); (void)e; }
    p = nullptr; n = 0;
  }
  ~DevBuf() { release(); }
};

template <class T>
struct PinnedBuf {
  T* p = nullptr;
  size_t n = 0;
  int alloc(size_t count) {
    release();
    n = count;
    if (count == 0) return CUADMM_OK;
    CUADMM_HIP_TRY(hipHostMalloc(&p, sizeof(T) * count, hipHostMallocDefault));
    return CUADMM_OK;
  }
  void release() {
    if (p) { hipError_t e = hipHostFree(p); (void)e; }
    p = nullptr; n = 0;
  }
  ~PinnedBuf() { release(); }
};

// Host loops over the m constraints: serial below kHostParMin, else kHostChunks fixed index ranges on the host pool
// (aat_ldlt.cpp).  Sums are formed per range and combined in range order: reproducible for any thread count.
constexpr int kHostParMin = 20000, kHostChunks = 32;
constexpr size_t kSvecPad = 64 * 40;       // >= 64 * U * batches of every tile geometry (psd_sign_closed.h)
template <class F>
void host_ranges(int m, F&& body) {   // body(chunk, lo, hi)
  if (m < kHostParMin) { body(0, 0, m); return; }
  struct Ctx { F* f; int m; } ctx{&body, m};
  cuadmm_host_parallel_for(kHostChunks, [](int c, void* p) {
    Ctx* x = static_cast<Ctx*>(p);
    const long long lo = (long long)x->m * c / kHostChunks, hi = (long long)x->m * (c + 1) / kHostChunks;
    (*x->f)(c, (int)lo, (int)hi);
  }, &ctx);
}

// milliseconds between two recorded events; 0, with the runtime's error cleared, where it cannot tell
inline float event_ms(hipEvent_t a, hipEvent_t b) {
  float t = 0;
  if (hipEventElapsedTime(&t, a, b) != hipSuccess) { t = 0; (void)hipGetLastError(); }
  return t;
}

enum KClass { K_ATY = 0, K_PSD = 1, K_POST = 2, K_SPMV = 3, K_COPY = 4, K_HOST = 5, K_COMM = 6, K_TAIL = 7, K_NUM = CUADMM_NUM_KCLASS };

// keeps the calling thread's current device across an entry point that visits several devices (the in-process group's leader):
// a caller that shares the thread with another HIP user (torch) finds its device as it left it
struct DeviceGuard {
  int dev = -1;
  DeviceGuard() { if (hipGetDevice(&dev) != hipSuccess) { dev = -1; (void)hipGetLastError(); } }
  ~DeviceGuard() { if (dev >= 0) (void)hipSetDevice(dev); }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// An event that is created where its user first needs it and destroyed with its owner.  Not yet created: converts to a null hipEvent_t.
struct DevEvent {
  hipEvent_t e = nullptr;
  int create(unsigned flags = 0) { CUADMM_HIP_TRY(flags ? hipEventCreateWithFlags(&e, flags) : hipEventCreate(&e)); return CUADMM_OK; }
  operator hipEvent_t() const { return e; }
  DevEvent() = default;
  ~DevEvent() { if (e) { hipError_t r = hipEventDestroy(e); (void)r; } }
  DevEvent(const DevEvent&) = delete;
  DevEvent& operator=(const DevEvent&) = delete;
};

// makes `device` the calling thread's current one, or says why not (engine.hip)
int check_device(int device);

}  // namespace cuadmm
