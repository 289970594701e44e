// The two ends of the native-rate embed route: a C-channel file at its own sample rate goes to the model's 16 kHz
// mono in ONE kernel, and the model's 16 kHz residual comes back onto every channel at the file's rate in ONE kernel.
//     front end:  mono[s] = (x[b][0][s] + x[b][1][s] + ...) / C          (f32, left to right, a true divide)
//                 y[b][m] = sum_j K[f][j] * mono_z[n * orig - width + j]   m = n * nw + f
//     back end:   u[b][m] = sum_j K[f][j] * delta_z[n * orig - width + j]
//                 out[b][c][m] = x[b][c][m] + gain * u[b][m]               every channel c
// with resample_kernel's arithmetic (csrc/wv_fx.hip): one fmaf chain per output in ascending j from +0.f, the signal zero outside its
// length.  What differs is how the operands arrive.  The tap table comes TRANSPOSED, kernels_t [L][nw]: consecutive lanes are
// consecutive output phases f, so one tap load of a wave is one run of addresses instead of 64 lines L floats apart.  And the input
// window of a workgroup's 256 outputs is staged in LDS once, zero-filled outside the signal; the front end forms the channel mean while
// it stages, so no mono copy and no up-sampled residual ever reaches memory.
// One workgroup = one clip x 256 outputs.  Compiled with -ffp-contract=off: x + gain * u keeps its two roundings.
#include <hip/hip_runtime.h>

#include "wv_host.h"

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

__global__ __launch_bounds__(256) void native_downmix_resample_kernel(const float* __restrict__ x, const float* __restrict__ Kt, float* __restrict__ y,
                                                                       int C, int Tn, int Tout, int orig, int nw, int L, int width) {
    extern __shared__ float win[];
    const int b = blockIdx.y, m0 = blockIdx.x * NATIVE_TILE, tid = threadIdx.x;
    const int n_lo = m0 / nw, n_out = min(NATIVE_TILE, Tout - m0), n_hi = (m0 + n_out - 1) / nw;
    const long long s_base = (long long)n_lo * orig - width;
    const int wlen = (n_hi - n_lo) * orig + L;
    const float* xb = x + (size_t)b * C * Tn;
    const float fc = (float)C;
    for (int i = tid; i < wlen; i += 256) {
        const long long s = s_base + i;
        float v = 0.f;
        if (s >= 0 && s < Tn) {
            v = xb[(size_t)s];
            for (int c = 1; c < C; ++c) v += xb[(size_t)c * Tn + (size_t)s];
            v = v / fc;
        }
        win[i] = v;
    }
    __syncthreads();
    const int m = m0 + tid;
    if (tid < n_out) y[(size_t)b * Tout + m] = native_chain(Kt, win, m, n_lo, orig, nw, L);
}

// x and out may be the same buffer: element [b][c][m] is read and written by the one thread that owns m, the read first.
__global__ __launch_bounds__(256) void native_upsample_add_kernel(const float* x, const float* __restrict__ delta, const float* __restrict__ Kt, float* out,
                                                                   int C, int T16, int Tn, int orig, int nw, int L, int width, float gain) {
    extern __shared__ float win[];
    const int b = blockIdx.y, m0 = blockIdx.x * NATIVE_TILE, tid = threadIdx.x;
    const int n_lo = m0 / nw, n_out = min(NATIVE_TILE, Tn - m0), n_hi = (m0 + n_out - 1) / nw;
    const long long s_base = (long long)n_lo * orig - width;
    const int wlen = (n_hi - n_lo) * orig + L;
    const float* db = delta + (size_t)b * T16;
    for (int i = tid; i < wlen; i += 256) {
        const long long s = s_base + i;
        win[i] = (s >= 0 && s < T16) ? db[(size_t)s] : 0.f;
    }
    __syncthreads();
    const int m = m0 + tid;
    if (tid >= n_out) return;
    const float gu = gain * native_chain(Kt, win, m, n_lo, orig, nw, L);
    const size_t base = (size_t)b * C * Tn + (size_t)m;
    for (int c = 0; c < C; ++c) out[base + (size_t)c * Tn] = x[base + (size_t)c * Tn] + gu;
}

}  // namespace wv

using wv::fail;

// The refusals both calls share; T_in / T_len are the resampler's input and output lengths.  -> WV_OK, or the code already reported.
static int native_check(const char* who, int B, int C, int T_in, int T_len, int orig, int nw, int L, int width, size_t* smem) {
    const std::string w(who);
    if (B < 1 || B > 65535) return fail(WV_EINVAL, w + ": B outside [1, 65535]");
    if (C < 1 || C > 64) return fail(WV_EINVAL, w + ": C outside [1, 64]");
    if (T_in < 1 || T_len < 1 || orig < 1 || nw < 1 || L < 1 || width < 0) return fail(WV_EINVAL, w + ": Tn, T16, Tout, orig, nw or L < 1, or width < 0");
    if ((long long)T_len > ((long long)T_in + orig - 1) / orig * nw + nw) return fail(WV_EINVAL, w + ": output longer than (ceil(T_in / orig) + 1) * nw");
    const long long bytes = wv::native_window(orig, nw, L) * (long long)sizeof(float);
    if (bytes > (long long)wv::NATIVE_LDS_BYTES) return fail(WV_EINVAL, w + ": the input window of a 256-output tile (" + std::to_string(bytes) + " bytes) exceeds 64 KB of LDS");
    *smem = (size_t)bytes;
    return WV_OK;
}

extern "C" int wv_native_downmix_resample(const float* x, const float* kernels_t, float* y, int B, int C, int Tn, int orig, int nw, int L, int width, int Tout,
                                          void* stream) {
    if (!x || !kernels_t || !y) return fail(WV_EINVAL, "wv_native_downmix_resample: null pointer (x, kernels_t, y)");
    size_t smem = 0;
    if (int rc = native_check("wv_native_downmix_resample", B, C, Tn, Tout, orig, nw, L, width, &smem)) return rc;
    hipLaunchKernelGGL(wv::native_downmix_resample_kernel, dim3((Tout - 1) / wv::NATIVE_TILE + 1, B), dim3(256), smem, (hipStream_t)stream, x,
                       kernels_t, y, C, Tn, Tout, orig, nw, L, width);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}

extern "C" int wv_native_upsample_add(const float* x, const float* delta, const float* kernels_t, float* out, int B, int C, int T16, int Tn, int orig, int nw,
                                      int L, int width, float gain, void* stream) {
    if (!x || !delta || !kernels_t || !out) return fail(WV_EINVAL, "wv_native_upsample_add: null pointer (x, delta, kernels_t, out)");
    size_t smem = 0;
    if (int rc = native_check("wv_native_upsample_add", B, C, T16, Tn, orig, nw, L, width, &smem)) return rc;
    hipLaunchKernelGGL(wv::native_upsample_add_kernel, dim3((Tn - 1) / wv::NATIVE_TILE + 1, B), dim3(256), smem, (hipStream_t)stream, x, delta,
                       kernels_t, out, C, T16, Tn, orig, nw, L, width, gain);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}
