// Decision and quality metrics of a validation pass, per clip, each from ONE read of its inputs (waveverify_amd/metrics.py holds the
// semantics; scripts/evaluate.py of the reference: BER.forward :442-516, MIOU.forward :591-665, SISNR.forward :167-229).
//
//   decode   per (clip, bit): S = sum_t sigmoid(l[t]) m[t], N = sum_t m[t]; then in f32, as the reference writes it:
//            avg = S / (N + eps) (masked) or S / T (no mask), decoded = avg >= thr, valid = N > 0; per clip: wrong valid bits, valid bits
//   iou      per clip: |p&g|, |p|g| for the foreground (p = raw > 0.5, g = mask == 1) and |!p & g0|, |!p | g0| for the background (g0 = mask == 0)
//   sisnr    per clip: sum x, sum y, sum xx, sum xy, sum yy (x = estimate, y = reference); SI-SNR in dB is algebra on the five moments
//
// Every row is cut into chunks of MT_CHUNK samples, whatever the grid: one workgroup sums one chunk in f64 (or int32) in a fixed order
// (thread t takes samples t, t + 256, ...; wave shuffle tree; the four waves in order) and a second, small launch adds the chunks of a
// row in ascending order and finishes.  No atomics: the results are bit-identical from run to run and do not depend on the batch the
// row arrived in.  Loads are single floats, so inputs need 4-byte alignment only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wv_host.h"

namespace {

constexpr int MT_NT = 256;                     // threads per workgroup (4 waves of 64)
constexpr int MT_PER = 16;                     // samples per thread
constexpr int MT_CHUNK = MT_NT * MT_PER;       // 4096 samples per workgroup
constexpr int MT_MAX_ROWS = 65535;             // gridDim.y

__host__ __device__ inline int mt_chunks(int T) { return (T + MT_CHUNK - 1) / MT_CHUNK; }

template <typename V>
__device__ __forceinline__ V mt_wave_sum(V v) {                  // lane 0 gets the sum, fixed tree
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// sums of N values per thread over the workgroup; thread 0 returns with the totals in v[]
template <typename V, int N>
__device__ __forceinline__ void mt_block_sum(V (&v)[N], V* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const V w = mt_wave_sum(v[i]);
        if (lane == 0) sh[wave * N + i] = w;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = ((sh[i] + sh[N + i]) + sh[2 * N + i]) + sh[3 * N + i];
    }
}

__global__ __launch_bounds__(MT_NT) void metrics_decode_kernel(const float* __restrict__ logits, const float* __restrict__ mask,
                                                               double* __restrict__ part, int W, int T) {
    __shared__ double sh[4 * 2];
    const int row = blockIdx.y, b = row / W;
    const float* z = logits + (size_t)row * T;
    const float* m = mask ? mask + (size_t)b * T : nullptr;
    const long long t0 = (long long)blockIdx.x * MT_CHUNK + threadIdx.x;
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < MT_PER; ++j) {
        const long long t = t0 + (long long)j * MT_NT;
        if (t < T) {
            const double p = 1.0 / (1.0 + exp(-(double)z[t]));
            if (m) {
                const double mv = (double)m[t];
                acc[0] += p * mv;
                acc[1] += mv;
            } else {
                acc[0] += p;
            }
        }
    }
    mt_block_sum<double, 2>(acc, sh);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)row * gridDim.x + blockIdx.x) * 2;
        o[0] = acc[0];
        o[1] = acc[1];
    }
}

// one wave per clip: thread w finishes bit w, w + 64, ...; the per-clip counts are integer sums
__global__ __launch_bounds__(64) void metrics_decode_finish_kernel(const double* __restrict__ part, const float* __restrict__ bits, int has_mask,
                                                                   float thr, float eps, int W, int T, int nchunks, float* __restrict__ avg,
                                                                   int* __restrict__ errors, int* __restrict__ valid) {
    const int b = blockIdx.x;
    int n_err = 0, n_valid = 0;
    for (int w = threadIdx.x; w < W; w += 64) {
        const size_t row = (size_t)b * W + w;
        const double* p = part + row * nchunks * 2;
        double s = 0.0, n = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            s += p[2 * c];
            n += p[2 * c + 1];
        }
        const float sf = (float)s;
        float a;
        bool ok = true;
        if (has_mask) {
            const float nf = (float)n;
            a = sf / (nf + eps);                                  // the eps add in f32, as (mask.sum + eps) is
            ok = nf > 0.f;
        } else {
            a = sf / (float)T;
        }
        avg[row] = a;
        const float dec = a >= thr ? 1.f : 0.f;
        n_valid += ok ? 1 : 0;
        n_err += (ok && dec != bits[row]) ? 1 : 0;
    }
    n_err = mt_wave_sum(n_err);
    n_valid = mt_wave_sum(n_valid);
    if (threadIdx.x == 0) {
        errors[b] = n_err;
        valid[b] = n_valid;
    }
}

__global__ __launch_bounds__(MT_NT) void metrics_iou_kernel(const float* __restrict__ pred, const float* __restrict__ mask, int* __restrict__ part,
                                                            int T) {
    __shared__ int sh[4 * 4];
    const int b = blockIdx.y;
    const float* p = pred + (size_t)b * T;
    const float* g = mask + (size_t)b * T;
    const long long t0 = (long long)blockIdx.x * MT_CHUNK + threadIdx.x;
    int acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < MT_PER; ++j) {
        const long long t = t0 + (long long)j * MT_NT;
        if (t < T) {
            const bool fg = p[t] > 0.5f;                           // the RAW locator output at 0.5; NaN is background
            const float gv = g[t];
            const bool g1 = gv == 1.f, g0 = gv == 0.f;
            acc[0] += (fg && g1) ? 1 : 0;
            acc[1] += (fg || g1) ? 1 : 0;
            acc[2] += (!fg && g0) ? 1 : 0;
            acc[3] += (!fg || g0) ? 1 : 0;
        }
    }
    mt_block_sum<int, 4>(acc, sh);
    if (threadIdx.x == 0) {
        int* o = part + ((size_t)b * gridDim.x + blockIdx.x) * 4;
        for (int i = 0; i < 4; ++i) o[i] = acc[i];
    }
}

__global__ __launch_bounds__(64) void metrics_iou_finish_kernel(const int* __restrict__ part, int B, int nchunks, int* __restrict__ counts) {
    const int i = blockIdx.x * 64 + threadIdx.x;                   // (clip, count)
    if (i >= 4 * B) return;
    const int b = i >> 2, k = i & 3;
    int s = 0;
    for (int c = 0; c < nchunks; ++c) s += part[((size_t)b * nchunks + c) * 4 + k];
    counts[i] = s;
}

__global__ __launch_bounds__(MT_NT) void metrics_sisnr_kernel(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ part,
                                                              int T) {
    __shared__ double sh[4 * 5];
    const int b = blockIdx.y;
    const float* xe = est + (size_t)b * T;
    const float* yr = ref + (size_t)b * T;
    const long long t0 = (long long)blockIdx.x * MT_CHUNK + threadIdx.x;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < MT_PER; ++j) {
        const long long t = t0 + (long long)j * MT_NT;
        if (t < T) {
            const double x = (double)xe[t], y = (double)yr[t];     // products of two f32 are exact in f64
            acc[0] += x;
            acc[1] += y;
            acc[2] += x * x;
            acc[3] += x * y;
            acc[4] += y * y;
        }
    }
    mt_block_sum<double, 5>(acc, sh);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)b * gridDim.x + blockIdx.x) * 5;
        for (int i = 0; i < 5; ++i) o[i] = acc[i];
    }
}

// SISNR.forward on the moments.  With x, y zero-meaned: E = <y,y>, d = <x,y>, a = d / (E + eps):
//   proj = a y,  |proj|^2 = a^2 E,  |x - proj|^2 = <x,x> - 2 a d + a^2 E = (<x,x> - (d / E) d) + E (a - d / E)^2
// The second form has no cancellation between its two non-negative parts: the first is what of x is orthogonal to y (exactly 0 for
// x == y, where the three centred moments are the same number), the second what the eps in a leaves, E (a - d/E)^2 = d^2 eps^2 / (E (E + eps)^2).
__global__ __launch_bounds__(64) void metrics_sisnr_finish_kernel(const double* __restrict__ part, int B, int T, int nchunks, double eps,
                                                                  double* __restrict__ sisnr, double* __restrict__ moments) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nchunks; ++c)
        for (int i = 0; i < 5; ++i) m[i] += part[((size_t)b * nchunks + c) * 5 + i];
    for (int i = 0; i < 5; ++i) moments[(size_t)b * 5 + i] = m[i];
    const double n = (double)T;
    const double xx = fmax(m[2] - (m[0] * m[0]) / n, 0.0);
    const double xy = m[3] - (m[0] * m[1]) / n;
    const double yy = fmax(m[4] - (m[1] * m[1]) / n, 0.0);
    const double e = yy + eps;                                     // ref_energy
    const double a = xy / e;
    const double proj_power = a * a * yy;
    double noise = xx;
    if (yy > 0.0) {
        const double r = xy / yy;
        const double k = xy * eps / (yy * e);                     // |a - r|
        noise = fmax(xx - r * xy, 0.0) + yy * k * k;
    }
    const double ratio = proj_power / (noise + eps);
    sisnr[b] = 10.0 * log10(ratio + eps);
}

using wv::fail;
inline bool mt_shape_ok(long long rows, int T) { return rows >= 1 && rows <= MT_MAX_ROWS && T >= 1; }
inline int mt_launched() {
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}

}  // namespace

extern "C" {

size_t wv_metrics_decode_workspace_bytes(int B, int W, int T) {
    if (B < 1 || W < 1 || !mt_shape_ok((long long)B * W, T)) return 0;
    return wv::al256((size_t)B * W * mt_chunks(T) * 2 * sizeof(double));
}

int wv_metrics_decode(const float* logits, const float* bits, const float* mask, float threshold, float eps, int B, int W, int T, float* avg,
                      int* errors, int* valid, void* ws, size_t ws_bytes, void* stream) {
    if (!logits || !bits || !avg || !errors || !valid || B < 1 || W < 1 || !mt_shape_ok((long long)B * W, T)) return fail(WV_EINVAL, "null pointer (logits, bits, avg, errors, valid), B or W < 1, T < 1 or B * W > " + std::to_string(MT_MAX_ROWS));
    if (!ws || ((uintptr_t)ws & 7u) || ws_bytes < wv_metrics_decode_workspace_bytes(B, W, T)) return fail(WV_ENOMEM, "workspace missing, not 8-byte aligned, or too small");
    hipStream_t st = (hipStream_t)stream;
    const int nc = mt_chunks(T);
    hipLaunchKernelGGL(metrics_decode_kernel, dim3(nc, B * W), dim3(MT_NT), 0, st, logits, mask, (double*)ws, W, T);
    hipLaunchKernelGGL(metrics_decode_finish_kernel, dim3(B), dim3(64), 0, st, (const double*)ws, bits, mask ? 1 : 0, threshold, eps, W, T, nc, avg,
                       errors, valid);
    return mt_launched();
}

size_t wv_metrics_iou_workspace_bytes(int B, int T) {
    if (!mt_shape_ok(B, T)) return 0;
    return wv::al256((size_t)B * mt_chunks(T) * 4 * sizeof(int));
}

int wv_metrics_iou(const float* pred, const float* mask, int B, int T, int* counts, void* ws, size_t ws_bytes, void* stream) {
    if (!pred || !mask || !counts || !mt_shape_ok(B, T)) return fail(WV_EINVAL, "null pointer (pred, mask, counts), T < 1 or B outside [1, " + std::to_string(MT_MAX_ROWS) + "]");
    if (!ws || ((uintptr_t)ws & 3u) || ws_bytes < wv_metrics_iou_workspace_bytes(B, T)) return fail(WV_ENOMEM, "workspace missing, not 4-byte aligned, or too small");
    hipStream_t st = (hipStream_t)stream;
    const int nc = mt_chunks(T);
    hipLaunchKernelGGL(metrics_iou_kernel, dim3(nc, B), dim3(MT_NT), 0, st, pred, mask, (int*)ws, T);
    hipLaunchKernelGGL(metrics_iou_finish_kernel, dim3((4 * B + 63) / 64), dim3(64), 0, st, (const int*)ws, B, nc, counts);
    return mt_launched();
}

size_t wv_metrics_sisnr_workspace_bytes(int B, int T) {
    if (!mt_shape_ok(B, T)) return 0;
    return wv::al256((size_t)B * mt_chunks(T) * 5 * sizeof(double));
}

int wv_metrics_sisnr(const float* estimate, const float* reference, int B, int T, double eps, double* sisnr, double* moments, void* ws,
                     size_t ws_bytes, void* stream) {
    if (!estimate || !reference || !sisnr || !moments || !mt_shape_ok(B, T)) return fail(WV_EINVAL, "null pointer (estimate, reference, sisnr, moments), T < 1 or B outside [1, " + std::to_string(MT_MAX_ROWS) + "]");
    if (((uintptr_t)sisnr & 7u) || ((uintptr_t)moments & 7u)) return fail(WV_EINVAL, "sisnr / moments not 8-byte aligned");
    if (!ws || ((uintptr_t)ws & 7u) || ws_bytes < wv_metrics_sisnr_workspace_bytes(B, T)) return fail(WV_ENOMEM, "workspace missing, not 8-byte aligned, or too small");
    hipStream_t st = (hipStream_t)stream;
    const int nc = mt_chunks(T);
    hipLaunchKernelGGL(metrics_sisnr_kernel, dim3(nc, B), dim3(MT_NT), 0, st, estimate, reference, (double*)ws, T);
    hipLaunchKernelGGL(metrics_sisnr_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, st, (const double*)ws, B, T, nc, eps, sisnr, moments);
    return mt_launched();
}

}  // extern "C"
