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

// A 198 -> hidden -> 1 value net's description, as every call that takes one
// checks it (narde_value_mlp and narde_value_mlp_train share these fields):
// ld_max is the kernels' bound on a weight row's stride.
inline int check_mlp_fields(const void* w1t, int64_t ld_w1t, const void* b1, const void* w2, const void* b2, int hidden,
                            int hidden_act, int out_act, int64_t ld_max) {
  if (!w1t || !b1 || !w2 || !b2) return fail(NARDE_EINVAL, "the net has a NULL weight array");
  if (hidden < 1 || hidden > NARDE_VALUE_HIDDEN_MAX)
    return fail(NARDE_EINVAL, "hidden %d outside 1..%d", hidden, NARDE_VALUE_HIDDEN_MAX);
  if (ld_w1t < hidden || ld_w1t > ld_max)
    return fail(NARDE_EINVAL, "ld_w1t %lld outside hidden %d .. %lld", (long long)ld_w1t, hidden, (long long)ld_max);
  if (hidden_act < 0 || hidden_act > 2 || out_act < 0 || out_act > 2)
    return fail(NARDE_EINVAL, "activations: hidden 0 sigmoid, 1 tanh, 2 relu; out 0 none, 1 sigmoid, 2 tanh");
  return NARDE_OK;
}

// The scoring calls' checks of a narde_value_mlp and the kernels' view of it
// (Net: kernels_rows.h ValNet): the values are the mover's (perspective 0) or
// white's (1), written to `value` where the call writes values at all.
template <class Net>
inline int check_value_mlp(const narde_value_mlp* net, int perspective, float* value, int64_t ld_max, Net& vn) {
  if (!net) return fail(NARDE_EINVAL, "NULL argument");
  if (const int rc = check_mlp_fields(net->w1t, net->ld_w1t, net->b1, net->w2, net->b2, net->hidden, net->hidden_act,
                                      net->out_act, ld_max))
    return rc;
  if (perspective != 0 && perspective != 1)
    return fail(NARDE_EINVAL, "perspective must be 0 (the mover's values) or 1 (white's)");
  vn = Net{net->w1t, net->ld_w1t, net->b1, net->w2, net->b2, net->hidden, net->hidden_act, net->out_act, perspective,
           value};
  return NARDE_OK;
}

// The calls over n given public records (u32[n][8]; narde_records_lookahead,
// narde_turn_records_lookahead): a record a workgroup, so n is a grid's x.
inline int check_given_records(int64_t n, const void* records) {
  if (!records) return fail(NARDE_EINVAL, "NULL argument");
  if (n < 1 || n >= (int64_t(1) << 31)) return fail(NARDE_EINVAL, "n %lld outside 1 .. 2^31 - 1", (long long)n);
  if (!aligned16(records)) return fail(NARDE_EINVAL, "records must be 16-B aligned");
  return NARDE_OK;
}

}  // namespace narde_host
