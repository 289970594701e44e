// The reference's plain-arithmetic time-domain effects on the device (utils/effect_augmentation.py:1081-1332 the straight-through
// Functions, :1504-1681 echo / pink_noise, :1873-2132 median_filter .. random_noise, :2338-2404 white_noise / shush, :190-209 the
// linear stretch).  Unlike the sinc filters of wv_fx.hip these are pinned to the reference itself (tests/golden/effects_time.npz):
// the pointwise ops, the median, shush and scatter-zero bit for bit, echo / smooth / stretch to the filter bar (float sums whose
// order is not the CPU's), and case by case to a float64 oracle of each operation (oracle/wv_oracle_fx_time.py, tests/test_gpu_fx_time_fuzz.py).
// This file is compiled with -ffp-contract=off: a mul followed by an add stays two roundings, as in torch; the one fused multiply-add,
// the stretch's source coordinate, is written out as fmaf because torch's CPU kernel fuses it.
// All kernels are bandwidth-class: [rows][T] contiguous f32 in, the same out, 16-byte accesses where the placement allows them
// (the pointwise pass; the windowed kernels read a tile through LDS, whose fill is coalesced dwords because tiles start at any
// sample), one launch each except echo (whole-tensor maxima first, then the apply).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wv_host.h"

namespace wv {

constexpr int FXT_TILE = 256;

__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

// ---- pointwise pass ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pointwise_op(int op, float x, float nz, float a) {
    if (op == WV_FX_SCALE) return x * a;                               // tensor * scale
    if (op == WV_FX_ADD_NOISE) {                                       // tensor + noise * std
        const float s = nz * a;
        return x + s;
    }
    if (op == WV_FX_MUL) return x * nz;                                // gradient * keep mask
    const float q = rintf(x * a);                                      // (tensor * max_val).round() / max_val: half to even, IEEE divide
    return q / a;
}

__global__ __launch_bounds__(256) void pointwise_kernel(const float* __restrict__ x, const float* __restrict__ noise, float* __restrict__ y, size_t n, int op,
                                                         float a, int vec) {
    const size_t stride = (size_t)gridDim.x * 256, i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n4 = vec ? n / 4 : 0;
    const bool two = op == WV_FX_ADD_NOISE || op == WV_FX_MUL;
    for (size_t i = i0; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (two) z = reinterpret_cast<const float4*>(noise)[i];
        float4 o;
        o.x = pointwise_op(op, v.x, z.x, a);
        o.y = pointwise_op(op, v.y, z.y, a);
        o.z = pointwise_op(op, v.z, z.z, a);
        o.w = pointwise_op(op, v.w, z.w, a);
        reinterpret_cast<float4*>(y)[i] = o;
    }
    for (size_t i = n4 * 4 + i0; i < n; i += stride) y[i] = pointwise_op(op, x[i], two ? noise[i] : 0.f, a);
}

// ---- sliding median (scipy.signal.medfilt: window centred, ZERO padding) ------------------------------------------------------------
// One workgroup = one row x 256 outputs; the 256 + k - 1 window samples come from an LDS tile.  K > 0: the window goes to registers and
// an odd-even transposition network of K rounds sorts it (compare-exchange by `<`, so the multiset is kept whatever the values).  K = 0:
// rank counting over the tile for any odd k: the sample with exactly k / 2 samples before it in the order (value, position) is the median.
__device__ __forceinline__ void cswap(float& a, float& b) {
    const bool s = b < a;
    const float lo = s ? b : a, hi = s ? a : b;
    a = lo;
    b = hi;
}

template <int K>
__global__ __launch_bounds__(256) void median_kernel(const float* __restrict__ x, float* __restrict__ y, int T, int k) {
    extern __shared__ float tile[];
    const int row = blockIdx.y, n0 = blockIdx.x * FXT_TILE, tid = threadIdx.x;
    const int kk = K > 0 ? K : k, h = kk / 2;
    const float* xr = x + (size_t)row * T;
    for (int i = tid; i < FXT_TILE + kk - 1; i += 256) {
        const int s = n0 + i - h;
        tile[i] = (s >= 0 && s < T) ? xr[s] : 0.f;
    }
    __syncthreads();
    const int n = n0 + tid;
    if (n >= T) return;
    float res;
    if constexpr (K > 0) {
        float v[K];
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = tile[tid + j];
#pragma unroll
        for (int r = 0; r < K; ++r) {
#pragma unroll
            for (int j = r & 1; j + 1 < K; j += 2) cswap(v[j], v[j + 1]);
        }
        res = v[K / 2];
    } else {
        const float* w = tile + tid;
        res = __uint_as_float(0x7FC00000u);                            // a NaN in the window has no rank: outside the contract
        for (int i = 0; i < kk; ++i) {
            const float vi = w[i];
            int rank = 0;
            for (int j = 0; j < kk; ++j) {
                const float vj = w[j];
                rank += (vj < vi || (vj == vi && j < i)) ? 1 : 0;
            }
            if (rank == h) res = vi;
        }
    }
    y[(size_t)row * T + n] = res;
}

// ---- shush: zero the k quietest samples of each row ---------------------------------------------------------------------------------
// One workgroup per row.  The k-th smallest |x| is found by a radix select over the 31 magnitude bits, 8 bits a pass from the top: an
// LDS histogram of the samples that still match the prefix, a scan for the bin that holds rank k.  Then every sample below the
// threshold goes, and of the samples equal to it the earliest ones until k are gone (an ordered count across the workgroup; skipped
// when all of them go).  y = x * keep, so a zeroed negative sample is -0 as in the reference; mask_out = mask_in * (y != 0).
constexpr int SHUSH_THREADS = 1024;

__global__ __launch_bounds__(SHUSH_THREADS) void shush_kernel(const float* __restrict__ x, const float* __restrict__ mask_in, float* __restrict__ y,
                                                              float* __restrict__ keep, float* __restrict__ mask_out, int T, int k) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_kk, s_eq;
    __shared__ uint32_t wsum[SHUSH_THREADS / 64];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* xr = x + (size_t)row * T;
    uint32_t prefix = 0, kk = (uint32_t)k, cnt_eq = 0;
    if (k > 0) {
        for (int pass = 3; pass >= 0; --pass) {
            const int shift = pass * 8;
            const uint32_t himask = pass == 3 ? 0u : (0xFFFFFFFFu << (shift + 8));
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int t = tid; t < T; t += SHUSH_THREADS) {
                const uint32_t b = abs_bits(xr[t]);
                if ((b & himask) == prefix) atomicAdd(&hist[(b >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t cum = 0;
                for (int bin = 0; bin < 256; ++bin) {
                    const uint32_t c = hist[bin];
                    if (cum + c >= kk) {
                        s_prefix = prefix | ((uint32_t)bin << shift);
                        s_kk = kk - cum;
                        s_eq = c;
                        break;
                    }
                    cum += c;
                }
            }
            __syncthreads();
            prefix = s_prefix;
            kk = s_kk;
            cnt_eq = s_eq;
        }
    }
    const uint32_t thr = prefix;                                       // kk of the cnt_eq samples with |x| == thr go, and all below
    const bool ordered = k > 0 && kk != cnt_eq;
    uint32_t base = 0;
    for (int c0 = 0; c0 < T; c0 += SHUSH_THREADS) {
        const int t = c0 + tid;
        const bool valid = t < T;
        const float v = valid ? xr[t] : 0.f;
        const uint32_t b = abs_bits(v);
        bool kp = k == 0 || b > thr;
        if (ordered) {
            const bool eq = valid && b == thr;
            const unsigned long long bal = __ballot(eq);
            const int lane = tid & 63, wave = tid >> 6;
            if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
            __syncthreads();
            uint32_t before = base, total = 0;
            for (int w = 0; w < SHUSH_THREADS / 64; ++w) {
                const uint32_t c = wsum[w];
                before += w < wave ? c : 0u;
                total += c;
            }
            before += (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            if (eq && before >= kk) kp = true;
            base += total;
            __syncthreads();
        }
        if (valid) {
            const float kf = kp ? 1.f : 0.f;
            const float o = v * kf;
            const size_t i = (size_t)row * T + t;
            y[i] = o;
            keep[i] = kf;
            if (mask_in) mask_out[i] = mask_in[i] * (o == 0.f ? 0.f : 1.f);
        }
    }
}

// ---- echo ---------------------------------------------------------------------------------------------------------------------------
// c[row][t] = x[row][t] + volume * x[row][t + n - 1] for t < T - n + 1 (the reference's cross-correlation with [1, 0, .., 0, volume]),
// y = c / max|c| * max|x| when both maxima (over the WHOLE tensor) are > 0, the last n - 1 samples of every row 0.
// The record: rec[0] = (bits of max|x|) << 32 | ~position, rec[1] the same for c (positions are flat indices into [rows][T]); the
// maximum of these 64-bit keys is the largest magnitude at its earliest position, so an integer atomic max gives the same record in
// whatever order the workgroups arrive.
__device__ __forceinline__ unsigned long long peak_key(float v, size_t i) {
    return ((unsigned long long)abs_bits(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
}
__device__ __forceinline__ float peak_value(unsigned long long key) { return __uint_as_float((uint32_t)(key >> 32)); }
__device__ __forceinline__ size_t peak_index(unsigned long long key) { return (size_t)(0xFFFFFFFFu - (uint32_t)key); }

__global__ __launch_bounds__(256) void echo_peaks_kernel(const float* __restrict__ x, unsigned long long* __restrict__ rec, size_t N, int T, int n, float volume) {
    __shared__ unsigned long long red[2][256];
    const int tid = threadIdx.x;
    unsigned long long kx = 0, kc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < N; i += (size_t)gridDim.x * 256) {
        const int t = (int)(i % (size_t)T);
        const float v = x[i];
        const unsigned long long a = peak_key(v, i);
        kx = a > kx ? a : kx;
        if (t < T - n + 1) {
            const float d = volume * x[i + n - 1];
            const unsigned long long b = peak_key(v + d, i);
            kc = b > kc ? b : kc;
        }
    }
    red[0][tid] = kx;
    red[1][tid] = kc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            red[0][tid] = red[0][tid + off] > red[0][tid] ? red[0][tid + off] : red[0][tid];
            red[1][tid] = red[1][tid + off] > red[1][tid] ? red[1][tid + off] : red[1][tid];
        }
        __syncthreads();
    }
    if (tid == 0) {
        atomicMax(&rec[0], red[0][0]);
        atomicMax(&rec[1], red[1][0]);
    }
}

__global__ __launch_bounds__(256) void echo_apply_kernel(const float* __restrict__ x, const unsigned long long* __restrict__ rec, float* __restrict__ y, size_t N,
                                                          int T, int n, float volume) {
    const float mo = peak_value(rec[0]), mr = peak_value(rec[1]);
    const bool norm = mr > 0.f && mo > 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        const int t = (int)(i % (size_t)T);
        float o = 0.f;
        if (t < T - n + 1) {
            const float d = volume * x[i + n - 1];
            o = x[i] + d;
            if (norm) {
                o = o / mr;
                o = o * mo;
            }
        }
        y[i] = o;
    }
}

// Echo backward (the reference's autograd crosses the correlation and both maxima).  With s = mo / mr, S = sum(g * c) / mr over the
// valid samples, I the positions with |x| == mo and J the valid positions with |c| == mr (torch's full-reduction max shares its
// gradient evenly among tied positions):
//     dx[u] = s * (g[u] + volume * g[u - n + 1])  -  S * s / |J| * sum_{j in J} sign(c[j]) * (e_j + volume * e_(j + n - 1))  +  S / |I| * sum_{i in I} sign(x[i]) * e_i.
// Pass 1: ECHO_PARTS partial sums of g * c, each summed in a fixed order, and beside them the partial counts of I and J (c is formed
// as the forward formed it, so `==` against the record's magnitudes finds exactly the samples the forward's maxima saw); pass 2 adds
// them in index order (every workgroup, the same way) and writes dx, testing each sample against the two magnitudes.  With one peak
// each the divisions are by 1 and the result is what the recorded positions alone would give.  Without the normalisation (a maximum
// of 0) only the first term is left, with s = 1.  Workspace: float parts[ECHO_PARTS], then uint32 |I| and |J| partials of the same length.
constexpr int ECHO_PARTS = 256;

__global__ __launch_bounds__(256) void echo_dot_kernel(const float* __restrict__ x, const float* __restrict__ g, const unsigned long long* __restrict__ rec,
                                                        float* __restrict__ parts, size_t N, int T, int n, float volume) {
    __shared__ float red[256];
    __shared__ uint32_t redx[256], redc[256];
    const int tid = threadIdx.x;
    const uint32_t bo = (uint32_t)(rec[0] >> 32), br = (uint32_t)(rec[1] >> 32);
    float acc = 0.f;
    uint32_t nx = 0, nc = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < N; i += (size_t)gridDim.x * 256) {
        const int t = (int)(i % (size_t)T);
        const float v = x[i];
        nx += abs_bits(v) == bo ? 1u : 0u;
        if (t < T - n + 1) {
            const float d = volume * x[i + n - 1];
            const float c = v + d;
            acc += g[i] * c;
            nc += abs_bits(c) == br ? 1u : 0u;
        }
    }
    red[tid] = acc;
    redx[tid] = nx;
    redc[tid] = nc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            red[tid] += red[tid + off];
            redx[tid] += redx[tid + off];
            redc[tid] += redc[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t* counts = reinterpret_cast<uint32_t*>(parts + ECHO_PARTS);
        parts[blockIdx.x] = red[0];
        counts[blockIdx.x] = redx[0];
        counts[ECHO_PARTS + blockIdx.x] = redc[0];
    }
}

__global__ __launch_bounds__(256) void echo_backward_kernel(const float* __restrict__ x, const float* __restrict__ g, const unsigned long long* __restrict__ rec,
                                                             const float* __restrict__ parts, int nparts, float* __restrict__ dx, size_t N, int T, int n,
                                                             float volume) {
    __shared__ float s_S, s_nx, s_nc;
    const float mo = peak_value(rec[0]), mr = peak_value(rec[1]);
    const uint32_t bo = (uint32_t)(rec[0] >> 32), br = (uint32_t)(rec[1] >> 32);
    const bool norm = mr > 0.f && mo > 0.f;
    if (threadIdx.x == 0) {
        const uint32_t* counts = reinterpret_cast<const uint32_t*>(parts + ECHO_PARTS);
        double sum = 0.0;
        uint32_t nx = 0, nc = 0;
        for (int p = 0; p < nparts; ++p) {
            sum += (double)parts[p];
            nx += counts[p];
            nc += counts[ECHO_PARTS + p];
        }
        s_S = norm ? (float)(sum / (double)mr) : 0.f;
        s_nx = (float)(nx > 0 ? nx : 1u);
        s_nc = (float)(nc > 0 ? nc : 1u);
    }
    __syncthreads();
    const float S = s_S, s = norm ? mo / mr : 1.f, fnx = s_nx, fnc = s_nc;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (size_t)gridDim.x * 256) {
        const int t = (int)(i % (size_t)T);
        const float v = x[i];
        float dc0 = 0.f, dc1 = 0.f;                                    // dL/dc at t and at t - n + 1
        if (t < T - n + 1) {
            dc0 = s * g[i];
            if (norm) {
                const float d = volume * x[i + n - 1];
                const float c = v + d;
                if (abs_bits(c) == br) dc0 -= S * s * (c < 0.f ? -1.f : 1.f) / fnc;
            }
        }
        if (t - n + 1 >= 0) {
            const size_t j = i - (size_t)(n - 1);
            dc1 = s * g[j];
            if (norm) {
                const float d = volume * v;
                const float c = x[j] + d;
                if (abs_bits(c) == br) dc1 -= S * s * (c < 0.f ? -1.f : 1.f) / fnc;
            }
        }
        float o = dc0 + volume * dc1;
        if (norm && abs_bits(v) == bo) o += S * (v < 0.f ? -1.f : 1.f) / fnx;
        dx[i] = o;
    }
}

// ---- smooth: box filter of w taps over the REFLECT-padded signal, mask from the ZERO-padded mask ------------------------------------
__device__ __forceinline__ int reflect(int s, int T) { return s < 0 ? -s : (s >= T ? 2 * (T - 1) - s : s); }

__global__ __launch_bounds__(256) void smooth_kernel(const float* __restrict__ x, const float* __restrict__ mask_in, float* __restrict__ y,
                                                      float* __restrict__ mask_out, int T, int w, float thr) {
    extern __shared__ float tile[];                    // x tile [256 + w - 1], then the mask tile of the same length
    const int row = blockIdx.y, n0 = blockIdx.x * FXT_TILE, tid = threadIdx.x;
    const int len = FXT_TILE + w - 1, pad_l = (w - 1) / 2;
    const float* xr = x + (size_t)row * T;
    const float* mr = mask_in ? mask_in + (size_t)row * T : nullptr;
    float* mt = tile + len;
    for (int i = tid; i < len; i += 256) {
        const int s = n0 + i - pad_l;
        tile[i] = xr[min(max(reflect(s, T), 0), T - 1)];               // the clamp only guards tile entries no output of this row reads
        if (mr) mt[i] = (s >= 0 && s < T) ? mr[s] : 0.f;
    }
    __syncthreads();
    const int n = n0 + tid;
    if (n >= T) return;
    const float wf = (float)w, inv = 1.0f / wf;
    float acc = 0.f, cnt = 0.f;
    for (int j = 0; j < w; ++j) acc += tile[tid + j] * inv;
    y[(size_t)row * T + n] = acc;
    if (mr) {
        for (int j = 0; j < w; ++j) cnt += mt[tid + j];
        mask_out[(size_t)row * T + n] = (cnt / wf >= thr) ? 1.f : 0.f;
    }
}

// Transpose of smooth's audio path, fused: the transposed box filter gives the gradient towards the padded signal,
//     dxp[p] = sum_{t = max(0, p - w + 1)}^{min(T - 1, p)} g[t] / w,   p < T + w - 1,
// and the transpose of the reflect padding folds the pad samples back onto the interior samples they mirror:
//     dx[u] = dxp[u + pad_l]  +  dxp[pad_l - u] (1 <= u <= pad_l)  +  dxp[pad_l + 2 (T - 1) - u] (T - 1 - pad_r <= u <= T - 2).
__device__ __forceinline__ float box_transposed(const float* __restrict__ g, int p, int T, int w, float inv) {
    float acc = 0.f;
    for (int t = max(0, p - w + 1); t <= min(T - 1, p); ++t) acc += g[t] * inv;
    return acc;
}

__global__ __launch_bounds__(256) void smooth_backward_kernel(const float* __restrict__ g, float* __restrict__ dx, int T, int w) {
    const int row = blockIdx.y, u = blockIdx.x * 256 + threadIdx.x;
    if (u >= T) return;
    const int pad_l = (w - 1) / 2, pad_r = w - 1 - pad_l;
    const float inv = 1.0f / (float)w;
    const float* gr = g + (size_t)row * T;
    float o = box_transposed(gr, u + pad_l, T, w, inv);
    if (u >= 1 && u <= pad_l) o += box_transposed(gr, pad_l - u, T, w, inv);
    if (u >= T - 1 - pad_r && u <= T - 2) o += box_transposed(gr, pad_l + 2 * (T - 1) - u, T, w, inv);
    dx[(size_t)row * T + u] = o;
}

// ---- scatter-zero and linear stretch ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scatter_zero_kernel(float* __restrict__ y, float* __restrict__ mask, const int* __restrict__ idx, int T, int num) {
    const int row = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= num) return;
    const int t = idx[(size_t)row * num + j];
    if (t < 0 || t >= T) return;                                       // never a store outside the row
    y[(size_t)row * T + t] = 0.f;
    if (mask) mask[(size_t)row * T + t] = 0.f;
}

// torch.nn.functional.interpolate(mode='linear', align_corners=False): scale = Tin / Tout in f32, source coordinate
// max(0, scale * (m + 0.5) - 0.5) rounded ONCE (a fused multiply-add: rounding the product first moves the coordinate by up to an ulp
// of m, 1e-4 of the peak on a one-second clip), the two neighbours weighted 1 - l and l.
__global__ __launch_bounds__(256) void stretch_kernel(const float* __restrict__ x, float* __restrict__ y, int Tin, int Tout) {
    const int row = blockIdx.y, m = blockIdx.x * 256 + threadIdx.x;
    if (m >= Tout) return;
    const float scale = (float)Tin / (float)Tout;
    float src = fmaf(scale, (float)m + 0.5f, -0.5f);                   // ONE rounding, as torch's CPU kernel is compiled; the file's other products stay unfused
    src = src < 0.f ? 0.f : src;
    const int i0 = min((int)src, Tin - 1), i1 = i0 + (i0 < Tin - 1 ? 1 : 0);
    const float l1 = src - (float)i0, l0 = 1.f - l1;
    const float* xr = x + (size_t)row * Tin;
    y[(size_t)row * Tout + m] = l0 * xr[i0] + l1 * xr[i1];
}

static inline int flat_grid(size_t n, int per_block, int cap) {
    const size_t b = (n + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > (size_t)cap ? (size_t)cap : b));
}

static inline bool rows_ok(int rows, int T) { return rows >= 1 && rows <= 65535 && T >= 1 && (unsigned long long)rows * (unsigned long long)T < 0xFFFFFFFFull; }

}  // namespace wv

using wv::fail;

static int launched() {
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}

extern "C" int wv_fx_pointwise(const float* x, const float* noise, float* y, int rows, int T, int op, float a, void* stream) {
    if (!x || !y || !wv::rows_ok(rows, T) || op < WV_FX_SCALE || op > WV_FX_MUL) return fail(WV_EINVAL, "null pointer (x, y), rows outside [1, 65535], T < 1 or rows * T >= 2^32, or an unknown op");
    const bool two = op == WV_FX_ADD_NOISE || op == WV_FX_MUL;
    if (two && !noise) return fail(WV_EINVAL, "this op reads noise, which is null");
    const size_t n = (size_t)rows * T;
    const int vec = (((uintptr_t)x | (uintptr_t)y | (uintptr_t)(two ? noise : x)) & 15u) == 0;
    hipLaunchKernelGGL(wv::pointwise_kernel, dim3(wv::flat_grid(vec ? n / 4 + 3 : n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, x, noise, y, n, op, a, vec);
    return launched();
}

extern "C" int wv_fx_median(const float* x, float* y, int rows, int T, int k, void* stream) {
    if (!x || !y || !wv::rows_ok(rows, T) || k < 1 || k > WV_FX_MEDIAN_MAX_K || (k & 1) == 0) return fail(WV_EINVAL, "null pointer (x, y), rows outside [1, 65535], T < 1 or rows * T >= 2^32, or k not odd in [1, " WV_STR(WV_FX_MEDIAN_MAX_K) "]");
    const dim3 grid((T + wv::FXT_TILE - 1) / wv::FXT_TILE, rows), block(256);
    const size_t smem = (size_t)(wv::FXT_TILE + k - 1) * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
#define WV_MEDIAN_NET(K) \
    case K: hipLaunchKernelGGL(wv::median_kernel<K>, grid, block, smem, s, x, y, T, k); break;
    switch (k) {
        WV_MEDIAN_NET(1) WV_MEDIAN_NET(3) WV_MEDIAN_NET(5) WV_MEDIAN_NET(7) WV_MEDIAN_NET(9) WV_MEDIAN_NET(11) WV_MEDIAN_NET(13) WV_MEDIAN_NET(15)
        WV_MEDIAN_NET(17) WV_MEDIAN_NET(19) WV_MEDIAN_NET(21) WV_MEDIAN_NET(23) WV_MEDIAN_NET(25) WV_MEDIAN_NET(27) WV_MEDIAN_NET(29) WV_MEDIAN_NET(31)
        default: hipLaunchKernelGGL(wv::median_kernel<0>, grid, block, smem, s, x, y, T, k); break;
    }
#undef WV_MEDIAN_NET
    static_assert(WV_FX_MEDIAN_NET_K == 31, "the switch above lists the network sizes");
    return launched();
}

extern "C" int wv_fx_shush(const float* x, const float* mask_in, float* y, float* keep, float* mask_out, int rows, int T, int k, void* stream) {
    if (!x || !y || !keep || !wv::rows_ok(rows, T) || k < 0 || k > T - 1 || (mask_in && !mask_out)) return fail(WV_EINVAL, "null pointer (x, y, keep), rows outside [1, 65535], T < 1 or rows * T >= 2^32, k outside [0, T - 1], or mask_in without mask_out");
    hipLaunchKernelGGL(wv::shush_kernel, dim3(rows), dim3(wv::SHUSH_THREADS), 0, (hipStream_t)stream, x, mask_in, y, keep, mask_out, T, k);
    return launched();
}

extern "C" int wv_fx_echo_peaks(const float* x, void* rec, int rows, int T, int n, float volume, void* stream) {
    if (!x || !rec || !wv::rows_ok(rows, T) || n < 2 || n > T || ((uintptr_t)rec & 7u)) return fail(WV_EINVAL, "null pointer (x, rec), rows outside [1, 65535], T < 1 or rows * T >= 2^32, n outside [2, T], or rec not 8-byte aligned");
    WV_HIP_TRY(hipMemsetAsync(rec, 0, WV_FX_ECHO_RECORD_BYTES, (hipStream_t)stream));
    const size_t N = (size_t)rows * T;
    hipLaunchKernelGGL(wv::echo_peaks_kernel, dim3(wv::flat_grid(N, 1024, 1024)), dim3(256), 0, (hipStream_t)stream, x, (unsigned long long*)rec, N, T, n, volume);
    return launched();
}

extern "C" int wv_fx_echo_apply(const float* x, const void* rec, float* y, int rows, int T, int n, float volume, void* stream) {
    if (!x || !rec || !y || !wv::rows_ok(rows, T) || n < 2 || n > T || ((uintptr_t)rec & 7u)) return fail(WV_EINVAL, "null pointer (x, rec, y), rows outside [1, 65535], T < 1 or rows * T >= 2^32, n outside [2, T], or rec not 8-byte aligned");
    const size_t N = (size_t)rows * T;
    hipLaunchKernelGGL(wv::echo_apply_kernel, dim3(wv::flat_grid(N, 1024, 2048)), dim3(256), 0, (hipStream_t)stream, x, (const unsigned long long*)rec, y, N, T, n,
                       volume);
    return launched();
}

extern "C" size_t wv_fx_echo_backward_workspace_bytes(void) { return (size_t)wv::ECHO_PARTS * (sizeof(float) + 2 * sizeof(uint32_t)); }

extern "C" int wv_fx_echo_backward(const float* x, const float* g, const void* rec, float* dx, int rows, int T, int n, float volume, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (!x || !g || !rec || !dx || !workspace || !wv::rows_ok(rows, T) || n < 2 || n > T || ((uintptr_t)rec & 7u) || ((uintptr_t)workspace & 3u) ||
        workspace_bytes < wv_fx_echo_backward_workspace_bytes())
        return fail(WV_EINVAL, "null pointer (x, g, rec, dx, workspace), rows outside [1, 65535], T < 1 or rows * T >= 2^32, n outside [2, T], rec not 8-byte or workspace not 4-byte aligned, or workspace too small");
    const size_t N = (size_t)rows * T;
    const int parts = wv::flat_grid(N, 1024, wv::ECHO_PARTS);
    hipLaunchKernelGGL(wv::echo_dot_kernel, dim3(parts), dim3(256), 0, (hipStream_t)stream, x, g, (const unsigned long long*)rec, (float*)workspace, N, T, n,
                       volume);
    hipLaunchKernelGGL(wv::echo_backward_kernel, dim3(wv::flat_grid(N, 1024, 2048)), dim3(256), 0, (hipStream_t)stream, x, g, (const unsigned long long*)rec,
                       (const float*)workspace, parts, dx, N, T, n, volume);
    return launched();
}

extern "C" int wv_fx_smooth(const float* x, const float* mask_in, float* y, float* mask_out, int rows, int T, int w, float valid_threshold, void* stream) {
    if (!x || !y || !wv::rows_ok(rows, T) || w < 1 || w > WV_FX_SMOOTH_MAX_W || w - 1 - (w - 1) / 2 >= T || (mask_in && !mask_out)) return fail(WV_EINVAL, "null pointer (x, y), rows outside [1, 65535], T < 1 or rows * T >= 2^32, w outside [1, " WV_STR(WV_FX_SMOOTH_MAX_W) "], right pad w - 1 - (w - 1) / 2 >= T, or mask_in without mask_out");
    const size_t smem = 2 * (size_t)(wv::FXT_TILE + w - 1) * sizeof(float);
    hipLaunchKernelGGL(wv::smooth_kernel, dim3((T + wv::FXT_TILE - 1) / wv::FXT_TILE, rows), dim3(256), smem, (hipStream_t)stream, x, mask_in, y, mask_out, T, w,
                       valid_threshold);
    return launched();
}

extern "C" int wv_fx_smooth_backward(const float* g, float* dx, int rows, int T, int w, void* stream) {
    if (!g || !dx || !wv::rows_ok(rows, T) || w < 1 || w > WV_FX_SMOOTH_MAX_W || w - 1 - (w - 1) / 2 >= T) return fail(WV_EINVAL, "null pointer (g, dx), rows outside [1, 65535], T < 1 or rows * T >= 2^32, w outside [1, " WV_STR(WV_FX_SMOOTH_MAX_W) "] or right pad w - 1 - (w - 1) / 2 >= T");
    hipLaunchKernelGGL(wv::smooth_backward_kernel, dim3((T + 255) / 256, rows), dim3(256), 0, (hipStream_t)stream, g, dx, T, w);
    return launched();
}

extern "C" int wv_fx_scatter_zero(float* y, float* mask, const int* idx, int rows, int T, int num, void* stream) {
    if (!y || !wv::rows_ok(rows, T) || num < 0 || num > T || (num > 0 && !idx)) return fail(WV_EINVAL, "null y, rows outside [1, 65535], T < 1 or rows * T >= 2^32, num outside [0, T], or indices wanted without idx");
    if (num == 0) return WV_OK;
    hipLaunchKernelGGL(wv::scatter_zero_kernel, dim3((num + 255) / 256, rows), dim3(256), 0, (hipStream_t)stream, y, mask, idx, T, num);
    return launched();
}

extern "C" int wv_fx_stretch_linear(const float* x, float* y, int rows, int Tin, int Tout, void* stream) {
    if (!x || !y || !wv::rows_ok(rows, Tin) || !wv::rows_ok(rows, Tout)) return fail(WV_EINVAL, "null pointer (x, y), or rows outside [1, 65535], Tin or Tout < 1, or rows * Tin or rows * Tout >= 2^32");
    hipLaunchKernelGGL(wv::stretch_kernel, dim3((Tout + 255) / 256, rows), dim3(256), 0, (hipStream_t)stream, x, y, Tin, Tout);
    return launched();
}
