// HIPCHK and DevBuf, the owning device buffer of the library's host code: wh_host.h and wh_calibrate.hip include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include "../../include/witch_hip.h"

namespace wh {
void set_error(const char *fmt, ...);
}

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess) {                                                           \
      wh::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return WH_EHIP;                                                                 \
    }                                                                                 \
  } while (0)

// Device memory that frees itself.  ensure() only grows (with slack, so that a slowly growing caller does not reallocate
// every call) and does not keep the contents.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  int ensure(size_t bytes) {
    if (bytes <= cap) return WH_OK;
    release();
    size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&p, want) != hipSuccess) {
      p = nullptr;
      wh::set_error("hipMalloc of %zu bytes failed", want);
      return WH_ENOMEM;
    }
    cap = want;
    return WH_OK;
  }
  void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a DevBuf owns its memory");
