// The arithmetic of the SNR floors (DESIGN sections 7d-11 to 7d-13), shared by csrc/wv_snr_floor.hip, csrc/wv_channel_floor.hip and
// csrc/wv_live_floor.hip: the fixed-order frame energy, the gain rule, the weight rule and the output rule exist once.  Device only; compile
// with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace wv {

// The 16 lanes of a group: sum of squares of p[0 .. len) in THE order (sample k to partial (k >> 2) & 15, ascending k from +0.0, then the
// folds ^8, ^4, ^2, ^1); every lane returns the folded sum.  All 16 lanes of the group must call it.
__device__ __forceinline__ double frame_energy(const float* __restrict__ p, int len, int lane) {
    double e = 0.0;
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    for (int k = lane * 4; k < len; k += 64) {
        if (vec && k + 4 <= len) {
            const float4 v = *reinterpret_cast<const float4*>(p + k);
            e += (double)v.x * (double)v.x;
            e += (double)v.y * (double)v.y;
            e += (double)v.z * (double)v.z;
            e += (double)v.w * (double)v.w;
        } else {
            for (int i = k; i < k + 4 && i < len; ++i) e += (double)p[i] * (double)p[i];
        }
    }
    e += __shfl_xor(e, 8, 16);
    e += __shfl_xor(e, 4, 16);
    e += __shfl_xor(e, 2, 16);
    e += __shfl_xor(e, 1, 16);
    return e;
}

// frame_energy for a frame that is not one array (the live delay line followed by the new samples): get(k) is sample k.  The same partials, the
// same order within each and the same folds, so the sum has frame_energy's bits.  All 16 lanes of the group must call it.
template <class Get>
__device__ __forceinline__ double frame_energy_by(const Get& get, int len, int lane) {
    double e = 0.0;
    for (int k = lane * 4; k < len; k += 64)
        for (int i = k; i < k + 4 && i < len; ++i) {
            const double v = (double)get(i);
            e += v * v;
        }
    e += __shfl_xor(e, 8, 16);
    e += __shfl_xor(e, 4, 16);
    e += __shfl_xor(e, 2, 16);
    e += __shfl_xor(e, 1, 16);
    return e;
}

__device__ __forceinline__ float floor_gain(double Ex, double Er, float s, double rho) {
    if (Er == 0.0) return s;
    const double q = __dsqrt_rn(__ddiv_rn(rho * Ex, Er));
    return q < (double)s ? (float)q : s;
}

__device__ __forceinline__ float floor_weight(float gp, float g, float ramp) {
    if (gp < g) {
        const float w = gp + (g - gp) * ramp;
        return w < g ? w : g;
    }
    return g;
}

__device__ __forceinline__ float floor_out(float x, float v, int add) { return add ? (v == 0.f ? x : x + v) : v; }

}  // namespace wv
