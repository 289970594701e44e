// The resampler arithmetic of the native-rate route, shared by every kernel that forms the up-sampled residual
// (csrc/wv_native.hip, csrc/wv_channel_floor.hip, csrc/wv_live_floor.hip): ONE device function makes the fmaf chain, so the bits of u[m] cannot differ between them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace wv {

constexpr int NATIVE_TILE = 256;
constexpr size_t NATIVE_LDS_BYTES = 64 * 1024;        // what a workgroup may ask for without opting in to more

// Outputs [m0, m0 + 256) of one clip read phase groups n_lo = m0 / nw .. (m0 + 255) / nw, at most (nw + 254) / nw groups past n_lo:
// inputs n_lo * orig - width + [0, span * orig + L).
__host__ __device__ inline long long native_window(int orig, int nw, int L) { return (long long)((nw + NATIVE_TILE - 2) / nw) * orig + L; }

// The fmaf chain of output m over the staged window (win[0] is input sample n_lo * orig - width).
__device__ inline float native_chain(const float* __restrict__ Kt, const float* win, int m, int n_lo, int orig, int nw, int L) {
    const int n = m / nw, f = m - n * nw;
    const float* w = win + (size_t)(n - n_lo) * orig;
    const float* kf = Kt + f;
    float acc = 0.f;
#pragma unroll 4
    for (int j = 0; j < L; ++j) acc = fmaf(kf[(size_t)j * nw], w[j], acc);
    return acc;
}

}  // namespace wv
