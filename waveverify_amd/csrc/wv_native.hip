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
#include "wv_native_bank.h"                             // the bank rows and SessionBack: shared with csrc/wv_live_floor.hip
#include "wv_native_chain.h"                            // NATIVE_TILE, native_window, native_chain: shared with csrc/wv_channel_floor.hip

namespace wv {

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

// One workgroup of the front stage for ONE stream, shared by the lockstep kernel and the bank kernel (which differ only in where a stream's
// operands lie): block bx < tiles is the 256-output tile bx, the blocks from `tiles` on write the next history, sequence samples
// [drop, drop + hv2).  y and hist_out are the stream's own rows.  Every thread of the workgroup must call it (it holds a barrier).
__device__ __forceinline__ void native_down_stream(float* win, int bx, int tid, const SessionMono& seq, const float* __restrict__ Kt, float* __restrict__ y,
                                                   int n_out, int pad, float* __restrict__ hist_out, int drop, int hv2, int tiles, int orig, int nw, int L) {
    if (bx >= tiles) {                                                 // the next history: sequence samples [drop, drop + hv2)
        const int j = (bx - tiles) * NATIVE_TILE + tid;
        if (j < hv2) hist_out[j] = seq((long long)drop + j);
        return;
    }
    const int m0 = bx * NATIVE_TILE;
    const int n_lo = m0 / nw, cnt = min(NATIVE_TILE, n_out - m0), n_hi = (m0 + cnt - 1) / nw;
    const long long p_base = (long long)n_lo * orig - pad;
    const int wlen = (n_hi - n_lo) * orig + L;
    for (int i = tid; i < wlen; i += 256) win[i] = seq(p_base + i);
    __syncthreads();
    if (tid < cnt) y[m0 + tid] = native_chain(Kt, win, m0 + tid, n_lo, orig, nw, L);
}

__global__ __launch_bounds__(256) void native_session_down_kernel(const float* __restrict__ hist, int hcap, int hv, const float* __restrict__ x, int n,
                                                                   const float* __restrict__ Kt, float* __restrict__ y, int n_out, int pad,
                                                                   float* __restrict__ hist_out, int drop, int hv2, int tiles, int C, int orig, int nw,
                                                                   int L) {
    extern __shared__ float win[];
    const int s = blockIdx.y;
    const SessionMono seq{hist + (size_t)s * hcap, x + (size_t)s * C * (size_t)n, hv, C, (long long)n};
    native_down_stream(win, blockIdx.x, threadIdx.x, seq, Kt, y + (size_t)s * n_out, n_out, pad, hist_out + (size_t)s * hcap, drop, hv2, tiles, orig, nw, L);
}

// One workgroup of the back stage for ONE stream, shared like native_down_stream: blocks [0, tiles) are output tiles (out: the stream's C rows of
// k floats), [tiles, tiles + rblocks) write the next residual history, the rest the next delay line (pend_out: the stream's C rows of pcap floats).
__device__ __forceinline__ void native_up_add_stream(float* win, int bx, int tid, const SessionBack& b, const float* __restrict__ Kt, float* __restrict__ out,
                                                     int k, int pad, float gain, float* __restrict__ pend_out, int pv2, float* __restrict__ rhist_out, int rdrop,
                                                     int rv2, int tiles, int rblocks, int C, int orig, int nw, int L) {
    if (bx >= tiles + rblocks) {                                       // the next delay line: the originals not yet emitted, [k, k + pv2)
        const int j = (bx - tiles - rblocks) * NATIVE_TILE + tid;
        if (j < pv2)
            for (int c = 0; c < C; ++c) pend_out[(size_t)c * b.pcap + j] = b.orig_ch(c, (long long)k + j);
        return;
    }
    if (bx >= tiles) {                                                 // the next residual history
        const int j = (bx - tiles) * NATIVE_TILE + tid;
        if (j < rv2) rhist_out[j] = b.resid((long long)rdrop + j);
        return;
    }
    const int m0 = bx * NATIVE_TILE;
    const int n_lo = m0 / nw, cnt = min(NATIVE_TILE, k - m0), n_hi = (m0 + cnt - 1) / nw;
    const long long p_base = (long long)n_lo * orig - pad;
    const int wlen = (n_hi - n_lo) * orig + L;
    for (int i = tid; i < wlen; i += 256) win[i] = b.resid(p_base + i);
    __syncthreads();
    if (tid >= cnt) return;
    const int m = m0 + tid;
    const float gu = gain * native_chain(Kt, win, m, n_lo, orig, nw, L);
    for (int c = 0; c < C; ++c) out[(size_t)c * (size_t)k + m] = b.orig_ch(c, m) + gu;
}

__global__ __launch_bounds__(256) void native_session_up_add_kernel(const float* __restrict__ rhist, int rcap, int rv, const float* __restrict__ r, int nr,
                                                                     const float* __restrict__ Kt, const float* __restrict__ pend, int pcap, int pv,
                                                                     const float* __restrict__ x, int n, float* __restrict__ out, int k, int pad, float gain,
                                                                     float* __restrict__ pend_out, int pv2, float* __restrict__ rhist_out, int rdrop, int rv2,
                                                                     int tiles, int rblocks, int C, int orig, int nw, int L) {
    extern __shared__ float win[];
    const size_t s = blockIdx.y;
    const SessionBack b{rhist + s * rcap, r + s * (size_t)nr, pend + s * C * pcap, x + s * C * (size_t)n, rv, nr, pcap, pv, n};
    native_up_add_stream(win, blockIdx.x, threadIdx.x, b, Kt, out + s * C * (size_t)k, k, pad, gain, pend_out + s * C * pcap, pv2, rhist_out + s * rcap, rdrop,
                         rv2, tiles, rblocks, C, orig, nw, L);
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

// ---- native-rate session banks ---------------------------------------------------------------------------------------
// The same two stages for the slots of a bank, each slot with its own rate, channel count, packet length and resampler state: one workgroup row
// (blockIdx.y) per descriptor, the per-stream bodies above.  A slot's state is ping-pong: the descriptor's `half` names the half a launch reads,
// the launch writes the other, so no byte is read and written by one launch and the blocks of a row need no order among themselves.  The rate
// table travels in the kernel's arguments; a descriptor names a rate by index.
namespace wv {

// One descriptor row of wv_native_bank_down, checked the same way by every workgroup that serves it: a row that breaks the contract is skipped
// whole (native_bank.native_bank_down_row_ok states the same rule).
struct NativeDownRow {
    int64_t slot, rate, C, hv, x_off, n, y_off, n_out, pad, drop, hv2, half;
    bool ok;
};

__device__ __forceinline__ NativeDownRow native_bank_down_row(const int64_t* __restrict__ desc, int p, const NativeRates& rates, int n_rates, int capacity,
                                                              int hcap, int64_t n_x, int64_t n_y) {
    const int64_t* d = desc + 12 * (size_t)p;
    NativeDownRow r = {d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11], false};
    if (r.slot < 0 || r.slot >= capacity || r.rate < 0 || r.rate >= n_rates || r.C < 1 || r.C > 64 || (r.half != 0 && r.half != 1)) return r;
    if (!native_roll_ok(hcap, r.hv, r.n, r.drop, r.hv2)) return r;
    const wv_native_rate& t = rates.r[r.rate];
    r.ok = r.pad >= 0 && r.pad <= t.width && native_count_ok(r.n_out, r.hv + r.n, r.pad, t.orig, t.nw) && native_range_ok(r.x_off, r.C, r.n, n_x) &&
           native_range_ok(r.y_off, 1, r.n_out, n_y);
    return r;
}

__global__ __launch_bounds__(256) void native_bank_down_kernel(float* hist, int capacity, int hcap, const float* __restrict__ x, int64_t n_x, NativeRates rates,
                                                                int n_rates, const int64_t* __restrict__ desc, float* __restrict__ y, int64_t n_y) {
    extern __shared__ float win[];
    const NativeDownRow r = native_bank_down_row(desc, blockIdx.y, rates, n_rates, capacity, hcap, n_x, n_y);
    if (!r.ok) return;
    const int n_out = (int)r.n_out, hv2 = (int)r.hv2, tiles = native_tiles(n_out);
    if ((int64_t)blockIdx.x >= (int64_t)tiles + native_tiles(hv2)) return;        // the grid is as wide as the tick's longest row
    const wv_native_rate& t = rates.r[r.rate];
    float* h = hist + (size_t)r.slot * 2 * hcap;
    const SessionMono seq{h + (size_t)r.half * hcap, x + r.x_off, (int)r.hv, (int)r.C, r.n};
    native_down_stream(win, blockIdx.x, threadIdx.x, seq, t.kernels_t, y + r.y_off, n_out, (int)r.pad, h + (size_t)(1 - r.half) * hcap, (int)r.drop, hv2,
                       tiles, t.orig, t.nw, t.L);
}

__global__ __launch_bounds__(256) void native_bank_up_add_kernel(float* rhist, int rcap, float* pend, int pcap, int Cmax, int capacity,
                                                                  const float* __restrict__ res, int64_t n_r, const float* __restrict__ x, int64_t n_x,
                                                                  NativeRates rates, int n_rates, const int64_t* __restrict__ desc,
                                                                  const float* __restrict__ gain, float* __restrict__ out, int64_t n_out) {
    extern __shared__ float win[];
    const NativeUpRow r = native_bank_up_row(desc, blockIdx.y, rates, n_rates, capacity, rcap, pcap, Cmax, n_r, n_x, n_out);
    if (!r.ok) return;
    const int k = (int)r.k, rv2 = (int)r.rv2, pv2 = (int)r.pv2, tiles = native_tiles(k), rblocks = native_tiles(rv2);
    if ((int64_t)blockIdx.x >= (int64_t)tiles + rblocks + native_tiles(pv2)) return;
    const wv_native_rate& t = rates.r[r.rate];
    float* rh = rhist + (size_t)r.slot * 2 * rcap;
    float* pd = pend + (size_t)r.slot * 2 * Cmax * pcap;
    const size_t cur = (size_t)r.half, nxt = (size_t)(1 - r.half);
    const SessionBack b{rh + cur * rcap, res + r.r_off, pd + cur * Cmax * pcap, x + r.x_off, (int)r.rv, (int)r.nr, pcap, (int)r.pv, (int)r.n};
    native_up_add_stream(win, blockIdx.x, threadIdx.x, b, t.kernels_t, out + r.out_off, k, (int)r.pad, gain[blockIdx.y], pd + nxt * Cmax * pcap, pv2,
                         rh + nxt * rcap, (int)r.rdrop, rv2, tiles, rblocks, (int)r.C, t.orig, t.nw, t.L);
}

}  // namespace wv

extern "C" int wv_native_bank_down(float* hist, int capacity, int hcap, const float* x, int64_t n_x, const wv_native_rate* rates, int n_rates,
                                   const int64_t* desc, int P, int blocks, float* y, int64_t n_y, void* stream) {
    const char* who = "wv_native_bank_down";
    wv::NativeRates tab;
    size_t smem = 0;
    if (int rc = native_bank_check(who, capacity, P, blocks, rates, n_rates, &tab, &smem)) return rc;
    if (hcap < 1 || n_x < 0 || n_y < 0) return fail(WV_EINVAL, std::string(who) + ": hcap < 1, n_x < 0 or n_y < 0");
    if (!hist || (P > 0 && !desc) || (n_x > 0 && !x) || (n_y > 0 && !y)) return fail(WV_EINVAL, std::string(who) + ": null hist, descriptors without desc, samples without x, or outputs without y");
    const size_t hb = (size_t)capacity * 2 * hcap * 4, xb = (size_t)n_x * 4, yb = (size_t)n_y * 4;
    if (native_overlap(hist, hb, x, xb) || native_overlap(hist, hb, y, yb) || native_overlap(x, xb, y, yb)) return fail(WV_EINVAL, std::string(who) + ": hist, x and y must not overlap");
    if (P == 0 || blocks == 0) return WV_OK;
    hipLaunchKernelGGL(wv::native_bank_down_kernel, dim3(blocks, P), dim3(256), smem, (hipStream_t)stream, hist, capacity, hcap, x, n_x, tab, n_rates, desc, y,
                       n_y);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}

extern "C" int wv_native_bank_up_add(float* rhist, int rcap, float* pend, int pcap, int Cmax, int capacity, const float* r, int64_t n_r, const float* x,
                                     int64_t n_x, const wv_native_rate* rates, int n_rates, const int64_t* desc, const float* gain, int P, int blocks,
                                     float* out, int64_t n_out, void* stream) {
    const char* who = "wv_native_bank_up_add";
    wv::NativeRates tab;
    size_t smem = 0;
    if (int rc = native_bank_check(who, capacity, P, blocks, rates, n_rates, &tab, &smem)) return rc;
    if (rcap < 1 || pcap < 1 || Cmax < 1 || Cmax > 64 || n_r < 0 || n_x < 0 || n_out < 0) return fail(WV_EINVAL, std::string(who) + ": rcap or pcap < 1, Cmax outside [1, 64], or n_r, n_x or n_out < 0");
    if (!rhist || !pend || (P > 0 && (!desc || !gain)) || (n_r > 0 && !r) || (n_x > 0 && !x) || (n_out > 0 && !out))
        return fail(WV_EINVAL, std::string(who) + ": null rhist or pend, descriptors without desc or gain, or a positive count without its arena (r, x, out)");
    const size_t hb = (size_t)capacity * 2 * rcap * 4, pb = (size_t)capacity * 2 * Cmax * pcap * 4, rb = (size_t)n_r * 4, xb = (size_t)n_x * 4, ob = (size_t)n_out * 4;
    if (native_overlap(rhist, hb, pend, pb) || native_overlap(rhist, hb, r, rb) || native_overlap(rhist, hb, x, xb) || native_overlap(rhist, hb, out, ob) ||
        native_overlap(pend, pb, r, rb) || native_overlap(pend, pb, x, xb) || native_overlap(pend, pb, out, ob) || native_overlap(r, rb, out, ob) ||
        native_overlap(x, xb, out, ob))
        return fail(WV_EINVAL, std::string(who) + ": rhist, pend, r, x and out must not overlap (r and x are only read and may)");
    if (P == 0 || blocks == 0) return WV_OK;
    hipLaunchKernelGGL(wv::native_bank_up_add_kernel, dim3(blocks, P), dim3(256), smem, (hipStream_t)stream, rhist, rcap, pend, pcap, Cmax, capacity, r, n_r, x,
                       n_x, tab, n_rates, desc, gain, out, n_out);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}
