// How an entry point refuses its arguments: the status code it returns and the one thread-local message behind al_last_error()
// (inline, so one buffer per library, with external linkage: the library is built without hidden visibility), plus the range
// overlap test that several of those refusals share.  Included by al_kernels.hip (the C ABI) and by the kernel headers whose
// host side checks arguments (the *_prepare and *_check functions); al_transforms.hip does not see it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/audiblelight_hip.h"

namespace al {

inline thread_local char g_err[256] = "";

inline int fail(int code, const char *msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

// "<entry>: <why>", AL_E_BADARG
inline int fail_arg(const char *entry, const char *why) {
  snprintf(g_err, sizeof(g_err), "%s: %s", entry, why);
  return AL_E_BADARG;
}

inline int check_error(hipError_t e, const char *what) {
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return AL_E_HIP;
  }
  return AL_OK;
}

inline int check_launch(const char *what) { return check_error(hipGetLastError(), what); }

// do a[0, na) and b[0, nb) share a sample?
inline bool fx_ranges_overlap(const float *a, int64_t na, const float *b, int64_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb * sizeof(float) && pb < pa + (uintptr_t)na * sizeof(float);
}

}  // namespace al
