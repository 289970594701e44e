// ITU-R BS.1770-4 gated loudness of N windows of one f32 arena, and the loudness-gated batch draw of data.ClipPool.  The constants, the
// K-weighting table and the float64 statement of the algorithm are in waveverify_amd/loudness.py; this file is the device route of
// metrics.Loudness and ClipPool.sample.
//
// loudness   a lane per window, 64 windows per workgroup of one wave.  The two K-weighting biquads are one linear recurrence with 4 states
//            (transposed direct form II), and it is run as what it is: sample by sample in f64, in scipy.signal.sosfilt's own order of
//            operations (this file is built with -ffp-contract=off: plain multiplies and adds), so the K-weighted signal is the float64
//            oracle's bit for bit before its one rounding to f32.  The high-pass poles are a nearly double pair (0.98514 +- 0.00053i at
//            16 kHz): such a recurrence amplifies every rounding by three digits, and where only the filter rings the float64 result
//            is itself 1e-11 .. 3e-10 from exact arithmetic.  Any other order -- chunks run from a zero state and linked by powers of the
//            transition matrix were built and measured, with exact powers and compensated sums: 1.8e-11 .. 4.0e-10 from the oracle
//            in those sub-blocks -- lands that far from the sequential result, past the 1e-11 the sub-block energies are held to.
//            So the parallelism is across windows only (a training batch offers 64 x 8 of them), and the wave's lanes share the loads:
//              stage   chunk by chunk (64 samples), the wave loads every window's chunk with one coalesced load each, zeros past the
//                      window's own length, one chunk ahead of the filter so that the 64 loads are in flight while the lanes compute;
//                      then into LDS, row stride 65 floats, so that the lanes, each reading its own row, hit different banks
//              run     every lane filters its row, adds y^2 in sample order and closes a 100 ms sub-block where it ends (T and fs are
//                      the same for all windows: the control flow is uniform)
//              store   with `filtered` given, the rows go back through LDS and out coalesced
//            then every lane gates its own window on the finished sub-block energies, blocks in ascending order.
//            No atomics, every order fixed by T and fs alone: two runs are bit-equal and a window's numbers depend neither on N nor on
//            its row.
// sample     choice[b] = the first try whose loudness is above the cutoff, else the last; that window copied out, zero-filled.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wv_host.h"
#include "wv_kernels.h"

namespace {

constexpr int LD_CHUNK = 64;                         // samples of every window staged in LDS at a time (wv_loudness_chunk)
constexpr int LD_LANES = 64;                         // windows of a workgroup: one wave, a lane each
constexpr int LD_STRIDE = LD_CHUNK + 1;              // LDS row stride in floats: odd, so lane r's row starts in bank r mod 32
constexpr int LD_MAX_T = 1 << 30;
constexpr double LD_OFFSET = -0.691, LD_ABS_GATE = -70.0, LD_REL_GATE = -10.0, LD_MIN_LOUDNESS = -70.0;
constexpr int PS_SPAN = 1024;                        // samples a workgroup of the copy moves

struct Sos {
    double b0, b1, b2, a1, a2, c0, c1, c2, d1, d2;
};

// one sample through both sections; s = {z1, z2 of the shelf, z1, z2 of the high-pass}
__device__ __forceinline__ double ld_step(const Sos& k, double x, double (&s)[4]) {
    const double y1 = k.b0 * x + s[0];
    s[0] = k.b1 * x - k.a1 * y1 + s[1];
    s[1] = k.b2 * x - k.a2 * y1;
    const double y2 = k.c0 * y1 + s[2];
    s[2] = k.c1 * y1 - k.d1 * y2 + s[3];
    s[3] = k.c2 * y1 - k.d2 * y2;
    return y2;
}

// mean square of gating block j = sub-blocks j..j+3
__device__ __forceinline__ double ld_block_ms(const double* __restrict__ s, int j, int h) {
    return (((s[j] + s[j + 1]) + s[j + 2]) + s[j + 3]) / (4.0 * (double)h);
}

// grid ceil(N / 64), 64 threads.  T >= 4 h (the launcher checks).
__global__ __launch_bounds__(LD_LANES) void loudness_kernel(const float* __restrict__ pool, const long long* __restrict__ starts,
                                                            const int* __restrict__ lens, int N, int T, int h, const double* __restrict__ tab,
                                                            double* __restrict__ lufs, double* __restrict__ sub, float* __restrict__ filtered) {
    __shared__ float xs[LD_LANES * LD_STRIDE];                   // [window][sample of the chunk], 16.6 KB
    __shared__ long long sh_start[LD_LANES];
    __shared__ int sh_len[LD_LANES];
    const int lane = threadIdx.x, w0 = blockIdx.x * LD_LANES, n = w0 + lane;
    const int rows = min(LD_LANES, N - w0);                      // windows of this workgroup
    const bool live = lane < rows;
    sh_start[lane] = live ? starts[n] : 0;
    sh_len[lane] = live ? min(max(lens[n], 0), T) : 0;
    __syncthreads();
    const int nsub = T / h, tend = nsub * h;                     // samples behind tend belong to no sub-block
    double* subn = sub + (size_t)(live ? n : w0) * nsub;
    const Sos k = {tab[0], tab[1], tab[2], tab[4], tab[5], tab[6], tab[7], tab[8], tab[10], tab[11]};
    float* xr = xs + lane * LD_STRIDE;
    double s[4] = {0.0, 0.0, 0.0, 0.0};                          // zero at the window's first sample
    double acc = 0.0;
    int j = 0, left = h;                                         // the open sub-block and the samples it still takes

    // stage, one chunk ahead: the wave's 64 loads of the NEXT chunk (a row each, coalesced) stay in flight in registers while the lanes
    // filter this one; nothing at or past a window's start + len is read (a row past the workgroup's windows has length 0)
    float nx[LD_LANES];
    auto fetch = [&](int at) {
#pragma unroll
        for (int r = 0; r < LD_LANES; ++r) nx[r] = at < sh_len[r] ? pool[sh_start[r] + at] : 0.f;
    };
    fetch(lane);
    for (int t0 = 0; t0 < T; t0 += LD_CHUNK) {
        const int t = t0 + lane;
#pragma unroll
        for (int r = 0; r < LD_LANES; ++r) xs[r * LD_STRIDE + lane] = nx[r];
        __syncthreads();
        if (t0 + LD_CHUNK < T) fetch(t + LD_CHUNK);
        const int m = min(LD_CHUNK, T - t0);
        for (int i0 = 0; i0 < m; i0 += 8) {                      // run: 8 samples read ahead of the recurrence that waits on nothing else
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = xr[i0 + u];       // inside the row also where i0 + u >= m
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u;
                if (i < m) {
                    const double y = ld_step(k, (double)v[u], s);
                    if (filtered) xr[i] = (float)y;
                    if (t0 + i < tend) {
                        acc += y * y;
                        if (--left == 0) {
                            if (live) subn[j] = acc;
                            ++j;
                            acc = 0.0;
                            left = h;
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (filtered && t < T)                                   // store
            for (int r = 0; r < rows; ++r) filtered[(size_t)(w0 + r) * T + t] = xs[r * LD_STRIDE + lane];
        __syncthreads();
    }
    if (!live) return;

    // gating, blocks in ascending order
    const int nb = nsub - 3;
    double sum = 0.0;
    int cnt = 0;
    for (int b = 0; b < nb; ++b) {
        const double z = ld_block_ms(subn, b, h);
        if (LD_OFFSET + 10.0 * log10(z) > LD_ABS_GATE) {
            sum += z;
            ++cnt;
        }
    }
    if (cnt == 0) {
        lufs[n] = LD_MIN_LOUDNESS;
        return;
    }
    const double gate = (LD_OFFSET + 10.0 * log10(sum / (double)cnt)) + LD_REL_GATE;
    sum = 0.0;
    cnt = 0;
    for (int b = 0; b < nb; ++b) {
        const double z = ld_block_ms(subn, b, h);
        const double l = LD_OFFSET + 10.0 * log10(z);
        if (l > LD_ABS_GATE && l > gate) {
            sum += z;
            ++cnt;
        }
    }
    lufs[n] = LD_OFFSET + 10.0 * log10(sum / (double)cnt);      // the loudest block passes its own relative gate: cnt >= 1
}

// grid (ceil(T / PS_SPAN), B), 256 threads; every workgroup of a row takes the same decision from the same numbers
__global__ __launch_bounds__(256) void pool_sample_kernel(const float* __restrict__ pool, const long long* __restrict__ starts,
                                                          const int* __restrict__ lens, const double* __restrict__ lufs, int tries, int T,
                                                          double cutoff, float* __restrict__ out, int* __restrict__ choice) {
    const int b = blockIdx.y;
    int k = 0;
    if (lufs) {
        k = tries - 1;
        for (int q = 0; q < tries; ++q)
            if (lufs[(size_t)b * tries + q] > cutoff) {
                k = q;
                break;
            }
    }
    const size_t w = (size_t)b * tries + k;
    const float* src = pool + starts[w];
    const int len = min(max(lens[w], 0), T);
    float* o = out + (size_t)b * T;
    const int t1 = min((int)blockIdx.x * PS_SPAN + PS_SPAN, T);
    for (int t = blockIdx.x * PS_SPAN + threadIdx.x; t < t1; t += 256) o[t] = t < len ? src[t] : 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) choice[b] = k;
}

using wv::fail;

// 0 = fine, else what is wrong with the shape
const char* ld_shape_error(int N, int T, int fs) {
    if (N < 1) return "N < 1";
    if (fs < 1 || fs % 10 != 0) return "fs must be a positive multiple of 10 (sub-blocks are fs / 10 samples)";
    if (T > LD_MAX_T) return "T above 2^30";
    if ((long long)T < 4LL * (fs / 10)) return "T shorter than one gating block of 4 sub-blocks (0.4 s)";
    return nullptr;
}

}  // namespace

extern "C" {

int wv_loudness_chunk(void) { return LD_CHUNK; }

size_t wv_loudness_workspace_bytes(int N, int T, int fs) { return ld_shape_error(N, T, fs) ? 0 : 256; }

int wv_loudness(const float* pool, const int64_t* starts, const int32_t* lens, int N, int T, int fs, const double* table, double* lufs,
                double* sub, float* filtered, void* ws, size_t ws_bytes, void* stream) {
    if (!pool || !starts || !lens || !table || !lufs || !sub) return fail(WV_EINVAL, "wv_loudness: null pointer (pool, starts, lens, table, lufs, sub)");
    if (const char* why = ld_shape_error(N, T, fs)) return fail(WV_EINVAL, std::string("wv_loudness: ") + why);
    if (((uintptr_t)starts | (uintptr_t)table | (uintptr_t)lufs | (uintptr_t)sub) & 7u) return fail(WV_EINVAL, "wv_loudness: starts, table, lufs and sub must be 8-byte aligned");
    if (!ws || ws_bytes < wv_loudness_workspace_bytes(N, T, fs)) return fail(WV_EINVAL, "wv_loudness: workspace missing or smaller than wv_loudness_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    const double samples = (double)N * T;
    wv::prof::Scope ps(st, "loudness", 20.0 * samples, 4.0 * samples * (filtered ? 2.0 : 1.0) + 8.0 * N * (T / (fs / 10) + 1));
    hipLaunchKernelGGL(loudness_kernel, dim3((N + LD_LANES - 1) / LD_LANES), dim3(LD_LANES), 0, st, pool, (const long long*)starts, lens, N, T, fs / 10, table, lufs, sub, filtered);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}

int wv_pool_sample(const float* pool, const int64_t* starts, const int32_t* lens, const double* lufs, int B, int tries, int T, double cutoff,
                   float* out, int32_t* choice, void* stream) {
    if (!pool || !starts || !lens || !out || !choice) return fail(WV_EINVAL, "wv_pool_sample: null pointer (pool, starts, lens, out, choice)");
    if (B < 1 || B > 65535 || tries < 1 || T < 1) return fail(WV_EINVAL, "wv_pool_sample: B outside [1, 65535], tries < 1 or T < 1");
    if (((uintptr_t)starts | (uintptr_t)lufs) & 7u) return fail(WV_EINVAL, "wv_pool_sample: starts and lufs must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    wv::prof::Scope ps(st, "pool_sample", 0.0, 8.0 * B * T);
    hipLaunchKernelGGL(pool_sample_kernel, dim3((T + PS_SPAN - 1) / PS_SPAN, B), dim3(256), 0, st, pool, (const long long*)starts, lens, lufs, tries, T,
                       cutoff, out, choice);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}

}  // extern "C"
