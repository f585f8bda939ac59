// Error plumbing of the C ABI, shared by its translation units (hs_api*.cpp): the
// calling thread's last error message and the helpers that set it.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace hs {

extern thread_local std::string g_err;   // one object, defined in hs_api.cpp; hs_last_error reads it

inline int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}
inline bool hip_ok(hipError_t e, const char* what) {
  if (e == hipSuccess) return true;
  g_err = std::string(what) + ": " + hipGetErrorString(e);
  return false;
}
// a launch's or runtime call's result as the ABI's 0 / -1
inline int hip_rc(hipError_t e, const char* what) { return hip_ok(e, what) ? 0 : -1; }

}  // namespace hs
