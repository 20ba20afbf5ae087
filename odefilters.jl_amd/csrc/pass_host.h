// Host-side scaffold of the post-processing passes over the records (summary.hip, errors.hip, datalik.hip, datalik_times.hip,
// events.hip): scratch buffers that grow, the event pair that times a pass, and the release of device pointers.  Host code only;
// like summary.h, errors.h, datalik.h and events.h this header includes none of the step headers, so that no filter / smoother
// kernel depends on it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <string>

namespace odef {

// the refusal of a pass: `err` becomes the formatted message, the result is -1
inline int pass_fail(std::string& err, const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  err = buf;
  return -1;
}

// makes the scratch buffer *p hold at least `bytes` (contents are not kept); false: out of device memory
inline bool grow(void** p, size_t* cap, size_t bytes) {
  if (*cap >= bytes) return true;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *cap = 0;
  if (hipMalloc(p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  *cap = bytes;
  return true;
}

// frees the device pointers that are set and nulls them
template <class... T>
inline void free_device(T*&... p) {
  ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...);
}

// Times one pass on its stream.  begin() creates the two events on first use and fails only there; end() is the tail of a pass:
// the launches' last error, the closing record, the wait, the elapsed time (ms may be null).
struct PassTimer {
  hipEvent_t ev[2] = {nullptr, nullptr};

  hipError_t begin(hipStream_t stream) {
    for (hipEvent_t& e : ev)
      if (!e) {
        const hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) return rc;
      }
    (void)hipEventRecord(ev[0], stream);
    return hipSuccess;
  }
  hipError_t end(hipStream_t stream, float* ms) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ev[1], stream);
    if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
    if (e == hipSuccess && ms) e = hipEventElapsedTime(ms, ev[0], ev[1]);
    return e;
  }
  void destroy() {
    for (hipEvent_t& e : ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
};

}  // namespace odef
