// host_common.h -- what the host side of both translation units (narde.hip,
// dqn_learner.hip) shares: the error text behind narde_last_error(), the
// device guard and the launch check of every C entry point.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/narde.h"

namespace narde_host {

// narde_last_error()'s text, one per thread; defined in narde.hip
extern thread_local char g_err[512];

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) return fail(NARDE_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// the handle's device for the call; the caller's restored after it (no
// runtime call on the way out when they are the same -- the usual case, and
// the timed launch's host path)
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int d) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != d) switched = hipSetDevice(d) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched && prev >= 0) (void)hipSetDevice(prev);
  }
};

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NARDE_EHIP, "%s launch: %s", what, hipGetErrorString(e));
  return NARDE_OK;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; }

}  // namespace narde_host
