// Host-side policy shared by every file that exports part of include/waveverify_hip.h: how an entry point reports failure, and how a
// workspace is carved.
// Host only: no kernel includes this for device code.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "../../include/waveverify_hip.h"

namespace wv {

// Every non-zero return of an exported function goes through here: stores `msg` in the one thread-local string behind
// wv_last_error() and returns `code`.  Like errno, the message is defined only after a non-zero return: success neither clears nor
// touches it.  Defined in wv_model.hip.
int fail(int code, std::string msg);

// workspace carve-outs: every sub-buffer starts on a 256-byte boundary
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// One description of a workspace for both of its readers: take(bytes) hands out the next sub-buffer and advances by al256(bytes).  Over
// a null base it only counts (take returns null), and `used` is then the size the same sequence of takes needs.
struct Carver {
    char* base;
    size_t used = 0;
    explicit Carver(void* b) : base((char*)b) {}
    float* take(size_t bytes) {
        float* p = base ? (float*)(base + used) : nullptr;
        used += al256(bytes);
        return p;
    }
};

}  // namespace wv

// a #define'd limit of the public header as text, so that a message cannot drift from the limit it names
#define WV_STR_(x) #x
#define WV_STR(x) WV_STR_(x)

// A HIP runtime call, a launcher's hipError_t or hipGetLastError() after a launch: WV_EHIP with the expression and HIP's text.
#define WV_HIP_TRY(expr)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return wv::fail(WV_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)
