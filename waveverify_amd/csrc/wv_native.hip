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

// ---- live sessions ---------------------------------------------------------------------------------------------------
// The same two ends for a stream that arrives in pushes.  A stage's sequence is cat(history[0 .. hv), new[0 .. n)), never materialised: sample
// p is read from the history when p < hv, else from the new buffer.  Output 0 of a call is phase 0 of the first phase group not yet emitted;
// its first tap is sequence sample -pad (pad > 0 only while the stream's own start is still inside the filter), so output m = g * nw + f reads
// sequence samples g * orig - pad + j, zero outside [0, hv + n): the chain of the file kernels over the same values.  One workgroup is one
// stream x 256 outputs as above; the workgroups past the last tile write the next state into second buffers.
namespace wv {

// The front stage's sequence: the history holds channel MEANS, the new samples are C planar channels whose mean is formed as the file kernel
// forms it.
struct SessionMono {
    const float* h;
    const float* xs;
    int hv, C;
    long long n;
    __device__ float operator()(long long p) const {
        if (p < 0 || p >= hv + n) return 0.f;
        if (p < hv) return h[(size_t)p];
        const size_t q = (size_t)(p - hv);
        float v = xs[q];
        for (int c = 1; c < C; ++c) v += xs[(size_t)c * (size_t)n + q];
        return v / (float)C;
    }
};

__global__ __launch_bounds__(256) void native_session_down_kernel(const float* __restrict__ hist, int hcap, int hv, const float* __restrict__ x, int n,
                                                                   const float* __restrict__ Kt, float* __restrict__ y, int n_out, int pad,
                                                                   float* __restrict__ hist_out, int drop, int hv2, int tiles, int C, int orig, int nw,
                                                                   int L) {
    extern __shared__ float win[];
    const int s = blockIdx.y, tid = threadIdx.x;
    const SessionMono seq{hist + (size_t)s * hcap, x + (size_t)s * C * (size_t)n, hv, C, (long long)n};
    if ((int)blockIdx.x >= tiles) {                                    // the next history: sequence samples [drop, drop + hv2)
        const int j = ((int)blockIdx.x - tiles) * NATIVE_TILE + tid;
        if (j < hv2) hist_out[(size_t)s * hcap + j] = seq((long long)drop + j);
        return;
    }
    const int m0 = blockIdx.x * NATIVE_TILE;
    const int n_lo = m0 / nw, cnt = min(NATIVE_TILE, n_out - m0), n_hi = (m0 + cnt - 1) / nw;
    const long long p_base = (long long)n_lo * orig - pad;
    const int wlen = (n_hi - n_lo) * orig + L;
    for (int i = tid; i < wlen; i += 256) win[i] = seq(p_base + i);
    __syncthreads();
    if (tid < cnt) y[(size_t)s * n_out + m0 + tid] = native_chain(Kt, win, m0 + tid, n_lo, orig, nw, L);
}

__global__ __launch_bounds__(256) void native_session_up_add_kernel(const float* __restrict__ rhist, int rcap, int rv, const float* __restrict__ r, int nr,
                                                                     const float* __restrict__ Kt, const float* __restrict__ pend, int pcap, int pv,
                                                                     const float* __restrict__ x, int n, float* __restrict__ out, int k, int pad, float gain,
                                                                     float* __restrict__ pend_out, int pv2, float* __restrict__ rhist_out, int rdrop, int rv2,
                                                                     int tiles, int rblocks, int C, int orig, int nw, int L) {
    extern __shared__ float win[];
    const int s = blockIdx.y, tid = threadIdx.x, bx = blockIdx.x;
    const float* rh = rhist + (size_t)s * rcap;
    const float* rs = r + (size_t)s * (size_t)nr;
    const long long r_end = (long long)rv + nr;
    auto resid = [&](long long p) -> float { return (p < 0 || p >= r_end) ? 0.f : p < rv ? rh[(size_t)p] : rs[(size_t)(p - rv)]; };
    // sample i of channel c of cat(pending[0 .. pv), x[0 .. n))
    auto orig_ch = [&](int c, long long i) -> float {
        const size_t row = (size_t)s * C + c;
        return i < pv ? pend[row * pcap + (size_t)i] : x[row * (size_t)n + (size_t)(i - pv)];
    };
    if (bx >= tiles + rblocks) {                                       // the next delay line: the originals not yet emitted, [k, k + pv2)
        const int j = (bx - tiles - rblocks) * NATIVE_TILE + tid;
        if (j < pv2)
            for (int c = 0; c < C; ++c) pend_out[((size_t)s * C + c) * pcap + j] = orig_ch(c, (long long)k + j);
        return;
    }
    if (bx >= tiles) {                                                 // the next residual history
        const int j = (bx - tiles) * NATIVE_TILE + tid;
        if (j < rv2) rhist_out[(size_t)s * rcap + j] = resid((long long)rdrop + j);
        return;
    }
    const int m0 = bx * NATIVE_TILE;
    const int n_lo = m0 / nw, cnt = min(NATIVE_TILE, k - m0), n_hi = (m0 + cnt - 1) / nw;
    const long long p_base = (long long)n_lo * orig - pad;
    const int wlen = (n_hi - n_lo) * orig + L;
    for (int i = tid; i < wlen; i += 256) win[i] = resid(p_base + i);
    __syncthreads();
    if (tid >= cnt) return;
    const int m = m0 + tid;
    const float gu = gain * native_chain(Kt, win, m, n_lo, orig, nw, L);
    for (int c = 0; c < C; ++c) out[((size_t)s * C + c) * (size_t)k + m] = orig_ch(c, m) + gu;
}

}  // namespace wv

// The refusals both session calls share.  seq = the resampler's sequence length (history + new), n_out what it is asked for.
static int native_session_check(const char* who, int S, int C, int orig, int nw, int L, int width, int pad, long long seq, int n_out, size_t* smem) {
    const std::string w(who);
    if (S < 1 || S > 65535) return fail(WV_EINVAL, w + ": S outside [1, 65535]");
    if (C < 1 || C > 64) return fail(WV_EINVAL, w + ": C outside [1, 64]");
    if (orig < 1 || nw < 1 || L < 1 || width < 0) return fail(WV_EINVAL, w + ": orig, nw or L < 1, or width < 0");
    if (pad < 0 || pad > width) return fail(WV_EINVAL, w + ": pad outside [0, width]");
    if (n_out < 0 || (long long)n_out > ((seq + pad + orig - 1) / orig + 1) * nw) return fail(WV_EINVAL, w + ": outputs < 0 or more than (ceil((pad + history + new) / orig) + 1) * nw");
    const long long bytes = wv::native_window(orig, nw, L) * (long long)sizeof(float);
    if (bytes > (long long)wv::NATIVE_LDS_BYTES) return fail(WV_EINVAL, w + ": the input window of a 256-output tile (" + std::to_string(bytes) + " bytes) exceeds 64 KB of LDS");
    *smem = (size_t)bytes;
    return WV_OK;
}

// ceil(v / 256) for any int v >= 0, without the overflow of v + 255.
static int tiles_of(int v) { return v / wv::NATIVE_TILE + (v % wv::NATIVE_TILE != 0); }

// 0 <= valid <= cap, and the next state a suffix of the sequence that fits: drop + next == valid + fresh.
static bool session_roll_ok(int cap, int valid, int fresh, int drop, int next) {
    return cap >= 1 && valid >= 0 && valid <= cap && fresh >= 0 && drop >= 0 && next >= 0 && next <= cap && (long long)drop + next == (long long)valid + fresh;
}

extern "C" int wv_native_session_down(const float* hist, int hcap, int hv, const float* x, int n, const float* kernels_t, float* y, int n_out, int pad,
                                      float* hist_out, int drop, int hv2, int S, int C, int orig, int nw, int L, int width, void* stream) {
    const char* who = "wv_native_session_down";
    if (!hist || !hist_out || hist == hist_out || !kernels_t || (n > 0 && !x) || (n_out > 0 && !y)) return fail(WV_EINVAL, std::string(who) + ": null pointer (hist, hist_out, kernels_t; x with n > 0; y with n_out > 0), or hist_out == hist");
    if (!session_roll_ok(hcap, hv, n, drop, hv2)) return fail(WV_EINVAL, std::string(who) + ": hcap < 1, hv or hv2 outside [0, hcap], n or drop < 0, or drop + hv2 != hv + n");
    size_t smem = 0;
    if (int rc = native_session_check(who, S, C, orig, nw, L, width, pad, (long long)hv + n, n_out, &smem)) return rc;
    const int tiles = tiles_of(n_out), blocks = tiles + tiles_of(hv2);
    if (blocks == 0) return WV_OK;
    hipLaunchKernelGGL(wv::native_session_down_kernel, dim3(blocks, S), dim3(256), smem, (hipStream_t)stream, hist, hcap, hv, x, n, kernels_t, y, n_out, pad,
                       hist_out, drop, hv2, tiles, C, orig, nw, L);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}

extern "C" int wv_native_session_up_add(const float* rhist, int rcap, int rv, const float* r, int nr, const float* kernels_t, const float* pend, int pcap, int pv,
                                        const float* x, int n, float* out, int k, int pad, float gain, float* pend_out, float* rhist_out, int rdrop, int rv2,
                                        int S, int C, int orig, int nw, int L, int width, void* stream) {
    const char* who = "wv_native_session_up_add";
    if (!rhist || !rhist_out || rhist == rhist_out || !pend || !pend_out || pend == pend_out || !kernels_t || (nr > 0 && !r) || (n > 0 && !x) || (k > 0 && !out))
        return fail(WV_EINVAL, std::string(who) + ": null pointer (rhist, rhist_out, pend, pend_out, kernels_t; r with nr > 0; x with n > 0; out with k > 0), or a next-state buffer that is its source");
    if (!session_roll_ok(rcap, rv, nr, rdrop, rv2)) return fail(WV_EINVAL, std::string(who) + ": rcap < 1, rv or rv2 outside [0, rcap], nr or rdrop < 0, or rdrop + rv2 != rv + nr");
    const long long pv2 = (long long)pv + n - k;
    if (pcap < 1 || pv < 0 || pv > pcap || n < 0 || k < 0 || pv2 < 0 || pv2 > pcap) return fail(WV_EINVAL, std::string(who) + ": pcap < 1, pv outside [0, pcap], n or k < 0, or pv + n - k outside [0, pcap]");
    size_t smem = 0;
    if (int rc = native_session_check(who, S, C, orig, nw, L, width, pad, (long long)rv + nr, k, &smem)) return rc;
    const int tiles = tiles_of(k), rblocks = tiles_of(rv2);
    const int blocks = tiles + rblocks + tiles_of((int)pv2);
    if (blocks == 0) return WV_OK;
    hipLaunchKernelGGL(wv::native_session_up_add_kernel, dim3(blocks, S), dim3(256), smem, (hipStream_t)stream, rhist, rcap, rv, r, nr, kernels_t, pend, pcap,
                       pv, x, n, out, k, pad, gain, pend_out, (int)pv2, rhist_out, rdrop, rv2, tiles, rblocks, C, orig, nw, L);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}
