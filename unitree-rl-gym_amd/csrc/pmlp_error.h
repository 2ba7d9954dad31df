// pmlp_error.h — the host side's error report, shared by ppo_mlp.hip and ppo_loss.hip: the
// text behind pmlp_last_error (one definition, in ppo_mlp.hip) and the status after a launch.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace pmlp_host {
// records m as the calling thread's pmlp_last_error text and returns code
__attribute__((visibility("hidden"))) int fail(int code, const std::string& m);
}  // namespace pmlp_host

#define PMLP_CHECK_LAUNCH(what)                                                                          \
    do {                                                                                                 \
        hipError_t _e = hipGetLastError();                                                               \
        if (_e != hipSuccess) return pmlp_host::fail(-2, std::string(what) + ": " + hipGetErrorString(_e)); \
    } while (0)
