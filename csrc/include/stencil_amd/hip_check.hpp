#pragma once

#include <hip/hip_runtime.h>

#include <sstream>
#include <stdexcept>
#include <string>

namespace stencil_amd {

inline void hip_check(hipError_t err, const char *file, int line) {
  if (err != hipSuccess) {
    std::ostringstream ss;
    ss << "HIP error at " << file << ":" << line << ": " << hipGetErrorString(err);
    throw std::runtime_error(ss.str());
  }
}

#define STENCIL_HIP(expr) ::stencil_amd::hip_check((expr), __FILE__, __LINE__)

// end the capture running on `stream` and instantiate what it recorded into
// `exec`; the intermediate hipGraph_t is not kept
inline void end_capture_instantiate(hipStream_t stream, hipGraphExec_t &exec) {
  hipGraph_t g = nullptr;
  STENCIL_HIP(hipStreamEndCapture(stream, &g));
  STENCIL_HIP(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
  STENCIL_HIP(hipGraphDestroy(g));
}

} // namespace stencil_amd
