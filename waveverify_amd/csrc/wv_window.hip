// Windowed long-form and live-session execution.  A clip, or a stream, runs as a batch of WINDOWS: a run of
// frames plus a left halo at least as long as the nets' receptive field; the window batch goes through the unchanged net forwards and
// only each window's kept columns come back.  This file holds the data movement around those forwards:
//   window_gather_kernel   packed multi-clip source -> [W, 1, L] window batch (16-byte loads / stores where aligned)
//   window_scatter_kernel  kept columns of [W, C, L] window outputs -> each clip's [C, T] output
//   window_mean_kernel     per-window sigmoid sums psum[W, nb] (head_kernel / head16_kernel in their windowed mode) -> mean_prob[B, nb],
//                          windows of a clip added in a fixed order in f64: deterministic, no drift with length
//   frames_reduce_kernel   the localized heads' per-frame sums fsum[B, nb + 1, Fr] -> per SEGMENT {clip, f_lo, f_hi} the masked mean probability
//                          of every bit and the gated sample count, frames added in order in f64
//   session_advance_kernel a live session's tick: [S, H] history + [S, n] new samples -> the tick's window and the next history
//   segment_track_kernel   a live segment session's tick: the new frames' sums -> the per-stream open run, gap ring and ring of closed segments
// Every kernel checks its indices against the buffer sizes it is given, so a bad table skips work instead of writing out of bounds.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "wv_host.h"

namespace wv {

constexpr int WIN_NT = 256, WIN_PER_THREAD = 4, WIN_TILE = WIN_NT * WIN_PER_THREAD;

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// grid (ceil(L / WIN_TILE), W): window w = src[offs[w] .. offs[w] + L)
__global__ __launch_bounds__(WIN_NT) void window_gather_kernel(const float* __restrict__ src, int64_t n_src, const int64_t* __restrict__ offs,
                                                               float* __restrict__ dst, int L) {
    const int w = blockIdx.y;
    const int64_t off = offs[w];
    if (off < 0 || off + L > n_src) return;
    const float* s = src + off;
    float* d = dst + (size_t)w * L;
    const int j = blockIdx.x * WIN_TILE + threadIdx.x * WIN_PER_THREAD;
    if (aligned16(s) && aligned16(d) && j + WIN_PER_THREAD <= L) {
        *reinterpret_cast<float4*>(d + j) = *reinterpret_cast<const float4*>(s + j);
        return;
    }
#pragma unroll
    for (int i = 0; i < WIN_PER_THREAD; ++i)
        if (j + i < L) d[j + i] = s[j + i];
}

// grid (ceil(L / WIN_TILE), C, W).  desc[w] = {dst offset of the window's column 0 (row 0), dst row stride, keep lo, keep hi}, the keep
// range relative to the window: out[desc0 + c * desc1 + j] = y[w][c][j] for j in [lo, hi).
__global__ __launch_bounds__(WIN_NT) void window_scatter_kernel(const float* __restrict__ y, const int64_t* __restrict__ desc, float* __restrict__ out,
                                                                int64_t n_out, int C, int L) {
    const int c = blockIdx.y, w = blockIdx.z;
    const int64_t base = desc[4 * w], stride = desc[4 * w + 1], lo = desc[4 * w + 2], hi = desc[4 * w + 3];
    if (lo < 0 || hi > L || lo >= hi || base + lo < 0 || base + (int64_t)(C - 1) * stride + hi > n_out) return;
    const float* s = y + ((size_t)w * C + c) * L;
    float* d = out + base + (int64_t)c * stride;
    const int j = blockIdx.x * WIN_TILE + threadIdx.x * WIN_PER_THREAD;
    if (aligned16(s) && aligned16(d) && j >= lo && j + WIN_PER_THREAD <= hi) {
        *reinterpret_cast<float4*>(d + j) = *reinterpret_cast<const float4*>(s + j);
        return;
    }
#pragma unroll
    for (int i = 0; i < WIN_PER_THREAD; ++i)
        if (j + i >= lo && j + i < hi) d[j + i] = s[j + i];
}

// one thread per (clip, bit): mean[b][k] = (sum over rows[ptr[b] .. ptr[b+1]) of psum[row][k], in that order, in f64) / len[b]
__global__ __launch_bounds__(WIN_NT) void window_mean_kernel(const float* __restrict__ psum, int n_rows, const int* __restrict__ ptr,
                                                             const int* __restrict__ rows, const int64_t* __restrict__ len, float* __restrict__ mean,
                                                             int B, int nb) {
    const int i = blockIdx.x * WIN_NT + threadIdx.x;
    if (i >= B * nb) return;
    const int b = i / nb, k = i % nb;
    double acc = 0.0;
    for (int r = ptr[b]; r < ptr[b + 1]; ++r) {
        const int row = rows[r];
        if (row >= 0 && row < n_rows) acc += (double)psum[(size_t)row * nb + k];
    }
    mean[i] = len[b] > 0 ? (float)(acc / (double)len[b]) : 0.f;
}

// one thread per (segment, bit): S = sum over f in [f_lo, f_hi) of fsum[clip][bit][f] and N = the same sum of the count row, both in that
// order in f64; prob = S / (float(N) + eps), the eps add in f32 as metrics_decode_finish_kernel makes it, the quotient rounded once;
// N == 0 (an empty or wholly ungated segment) gives prob = 0.  A segment outside the tensor is treated as empty.
__global__ __launch_bounds__(WIN_NT) void frames_reduce_kernel(const float* __restrict__ fsum, int B, int nb, int Fr, const int* __restrict__ seg, int n_seg,
                                                               float eps, float* __restrict__ prob, double* __restrict__ count) {
    const int i = blockIdx.x * WIN_NT + threadIdx.x;
    if (i >= n_seg * nb) return;
    const int sg = i / nb, k = i % nb;
    const int clip = seg[3 * sg], lo = seg[3 * sg + 1], hi = seg[3 * sg + 2];
    double acc = 0.0, cnt = 0.0;
    if (clip >= 0 && clip < B && lo >= 0 && hi <= Fr) {
        const float* row = fsum + ((size_t)clip * (nb + 1) + k) * Fr;
        const float* crow = fsum + ((size_t)clip * (nb + 1) + nb) * Fr;
        for (int f = lo; f < hi; ++f) {
            acc += (double)row[f];
            cnt += (double)crow[f];
        }
    }
    const float d = (float)cnt + eps;
    prob[i] = cnt > 0.0 ? (float)(acc / (double)d) : 0.f;
    if (k == 0) count[sg] = cnt;
}

// grid (ceil(max(wlen, hv2) / WIN_NT), S).  Stream s's samples are cat(hist[s][0 .. hv), x[s][0 .. n)); the window is that sequence's
// first wlen samples, the next history its samples [drop, drop + hv2).
__global__ __launch_bounds__(WIN_NT) void session_advance_kernel(const float* __restrict__ hist, int hcap, int hv, const float* __restrict__ x, int n,
                                                                 float* __restrict__ win, int wlen, float* __restrict__ hist_out, int drop, int hv2) {
    const int s = blockIdx.y, j = blockIdx.x * WIN_NT + threadIdx.x;
    const float* h = hist + (size_t)s * hcap;
    const float* xs = x + (size_t)s * n;
    if (j < wlen) win[(size_t)s * wlen + j] = j < hv ? h[j] : xs[j - hv];
    if (j < hv2) {
        const int q = drop + j;
        hist_out[(size_t)s * hcap + j] = q < hv ? h[q] : xs[q - hv];
    }
}

// ---- the streaming form of segments_from_counts + frames_reduce_kernel ----------------------------------------
// Byte layout of the two caller-owned buffers (the header states it for callers): per stream `state` holds int64 {open, lo, hi, frames seen},
// f64 sums [nb + 1] of the open run and the gap ring [G - 1][nb + 1] f32; `events` holds an int64 event counter and `capacity` records
// {int64 lo, int64 hi, f64 count, f32 prob[nb]}.  Every section starts on an 8-byte boundary.
struct SegLayout {
    size_t state_stride, event_stride, rec;
};

static inline size_t up8(size_t x) { return (x + 7) & ~(size_t)7; }

static inline SegLayout seg_layout(int nb, int G, int capacity) {
    SegLayout l;
    l.state_stride = 32 + 8 * (size_t)(nb + 1) + up8(4 * (size_t)(G - 1) * (nb + 1));
    l.rec = 24 + up8(4 * (size_t)nb);
    l.event_stride = 8 + (size_t)capacity * l.rec;
    return l;
}

// grid (S), block = nb + 1 rounded up to a wave.  Thread k <= nb owns row k of the sums (row nb is the count row); EVERY thread reads the count
// row of every frame and keeps the run's count sum itself, so all threads of a stream take the same decisions without exchanging anything.
// Frames of this tick are read from fsum wherever they are needed; the ring only carries the off frames after `hi` over to the next tick
// (frame j in slot j % (G - 1); at most G - 1 consecutive frames are ever held, so slots never collide).  A run is closed as soon as G off
// frames have passed, hence an on frame that meets an open run always has a gap < G and merges.  Reads of the state come before the barrier,
// writes after it; event records are write-only.
__global__ __launch_bounds__(256) void segment_track_kernel(const float* __restrict__ fsum, int nb, int Fr, int f_lo, int n, long long frame0, int hop,
                                                            int last_valid, int final_, double min_on, int G, int min_len, float eps, char* state,
                                                            size_t state_stride, char* events, size_t event_stride, size_t rec, int capacity) {
    const int s = blockIdx.x, k = threadIdx.x;
    const bool owns = k <= nb;
    const int r = owns ? k : nb;
    const float* fs = fsum + (size_t)s * (nb + 1) * Fr + f_lo;
    const float* crow = fs + (size_t)nb * Fr;
    const float* krow = fs + (size_t)r * Fr;
    long long* hdr = reinterpret_cast<long long*>(state + (size_t)s * state_stride);
    double* accp = reinterpret_cast<double*>(hdr + 4);
    float* ring = reinterpret_cast<float*>(accp + nb + 1);
    long long* nevp = reinterpret_cast<long long*>(events + (size_t)s * event_stride);
    char* recs = reinterpret_cast<char*>(nevp + 1);
    const int R = G - 1;

    bool open = hdr[0] != 0;
    long long lo = hdr[1], hi = hdr[2], nev = *nevp;
    double acc = accp[r], cnt = accp[nb];
    // a state that cannot follow from zeros and gapless ticks (another frame0, a buffer never cleared) is taken as closed, so that no ring
    // slot or event record is ever addressed outside its buffer
    if (open && !(lo >= 0 && lo < hi && hi <= frame0 && frame0 - hi < G)) open = false;
    if (nev < 0 || nev > (1LL << 62)) nev = 0;

    auto close = [&]() {
        if (hi - lo >= min_len) {
            char* e = recs + (size_t)(nev % capacity) * rec;
            if (k == 0) {
                reinterpret_cast<long long*>(e)[0] = lo;
                reinterpret_cast<long long*>(e)[1] = hi;
                reinterpret_cast<double*>(e)[2] = cnt;
            }
            if (k < nb) {
                const float d = (float)cnt + eps;
                reinterpret_cast<float*>(e + 24)[k] = cnt > 0.0 ? (float)(acc / (double)d) : 0.f;
            }
            ++nev;
        }
        open = false;
    };

    for (int i = 0; i < n; ++i) {
        const long long g = frame0 + i;
        const float c = crow[i];
        const int valid = (final_ && i == n - 1) ? last_valid : hop;
        const bool on = valid > 0 && (double)c >= min_on * (double)valid;
        if (on) {
            if (open) {
                for (long long j = hi; j < g; ++j) {                 // the gap's off frames first, one by one, then the frame itself
                    float v, vc;
                    if (j >= frame0) {
                        v = krow[j - frame0];
                        vc = crow[j - frame0];
                    } else {
                        const float* slot = ring + (size_t)(j % R) * (nb + 1);
                        v = slot[r];
                        vc = slot[nb];
                    }
                    acc += (double)v;
                    cnt += (double)vc;
                }
            } else {
                open = true;
                lo = g;
                acc = cnt = 0.0;
            }
            acc += (double)krow[i];
            cnt += (double)c;
            hi = g + 1;
        } else if (open && g + 1 - hi >= G) {
            close();
        }
    }
    if (final_ && open) close();
    __syncthreads();

    const long long fend = frame0 + n;
    if (owns) {
        if (open)
            for (long long j = hi > frame0 ? hi : frame0; j < fend; ++j) ring[(size_t)(j % R) * (nb + 1) + k] = krow[j - frame0];
        accp[k] = acc;
    }
    if (k == 0) {
        hdr[0] = open ? 1 : 0;
        hdr[1] = lo;
        hdr[2] = hi;
        hdr[3] = fend;
        *nevp = nev;
    }
}

}  // namespace wv

using wv::fail;

static int launched() {
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}

extern "C" int wv_window_gather(const float* src, int64_t n_src, const int64_t* offs, float* dst, int W, int L, void* stream) {
    if (!src || !offs || !dst || W < 1 || W > 65535 || L < 1 || n_src < L) return fail(WV_EINVAL, "null pointer (src, offs, dst), W outside [1, 65535], L < 1 or n_src < L");
    hipLaunchKernelGGL(wv::window_gather_kernel, dim3((L + wv::WIN_TILE - 1) / wv::WIN_TILE, W), dim3(wv::WIN_NT), 0, (hipStream_t)stream, src, n_src,
                       offs, dst, L);
    return launched();
}

extern "C" int wv_window_scatter(const float* y, const int64_t* desc, float* out, int64_t n_out, int W, int C, int L, void* stream) {
    if (!y || !desc || !out || W < 1 || W > 65535 || C < 1 || C > 65535 || L < 1 || n_out < 1) return fail(WV_EINVAL, "null pointer (y, desc, out), W or C outside [1, 65535], L or n_out < 1");
    hipLaunchKernelGGL(wv::window_scatter_kernel, dim3((L + wv::WIN_TILE - 1) / wv::WIN_TILE, C, W), dim3(wv::WIN_NT), 0, (hipStream_t)stream, y, desc,
                       out, n_out, C, L);
    return launched();
}

extern "C" int wv_window_reduce_mean(const float* psum, int n_rows, const int* ptr, const int* rows, const int64_t* lengths, float* mean_prob, int B,
                                     int nb, void* stream) {
    if (!psum || !ptr || !rows || !lengths || !mean_prob || n_rows < 1 || B < 1 || nb < 1) return fail(WV_EINVAL, "null pointer (psum, ptr, rows, lengths, mean_prob) or n_rows, B, nb < 1");
    hipLaunchKernelGGL(wv::window_mean_kernel, dim3((B * nb + wv::WIN_NT - 1) / wv::WIN_NT), dim3(wv::WIN_NT), 0, (hipStream_t)stream, psum, n_rows, ptr,
                       rows, lengths, mean_prob, B, nb);
    return launched();
}

extern "C" int wv_frames_reduce(const float* fsum, int B, int nb, int Fr_stride, const int* seg, int n_seg, float eps, float* prob, double* count,
                                void* stream) {
    if (!fsum || !seg || !prob || !count || B < 1 || nb < 1 || Fr_stride < 1 || n_seg < 1 || (long long)n_seg * nb > 0x7fffffffLL) return fail(WV_EINVAL, "null pointer (fsum, seg, prob, count), B, nb, Fr_stride or n_seg < 1, or n_seg * nb beyond 2^31");
    hipLaunchKernelGGL(wv::frames_reduce_kernel, dim3((n_seg * nb + wv::WIN_NT - 1) / wv::WIN_NT), dim3(wv::WIN_NT), 0, (hipStream_t)stream, fsum, B, nb,
                       Fr_stride, seg, n_seg, eps, prob, count);
    return launched();
}

extern "C" int wv_session_advance(const float* hist, int hcap, int hv, const float* x, int n, float* win, int wlen, float* hist_out, int drop, int hv2,
                                  int S, void* stream) {
    if (!hist || !hist_out || hist == hist_out || S < 1 || S > 65535 || hcap < 1 || hv < 0 || hv > hcap || n < 0 || (n > 0 && !x)) return fail(WV_EINVAL, "null hist / hist_out (or the same buffer), S outside [1, 65535], hcap < 1, hv outside [0, hcap], n < 0, or samples without x");
    if (wlen < 0 || wlen > hv + n || (wlen > 0 && !win) || drop < 0 || hv2 < 0 || hv2 > hcap || drop + hv2 != hv + n) return fail(WV_EINVAL, "wlen outside [0, hv + n] (or a window without win), drop < 0, hv2 outside [0, hcap], or drop + hv2 != hv + n");
    const int m = wlen > hv2 ? wlen : hv2;
    if (m == 0) return WV_OK;
    hipLaunchKernelGGL(wv::session_advance_kernel, dim3((m + wv::WIN_NT - 1) / wv::WIN_NT, S), dim3(wv::WIN_NT), 0, (hipStream_t)stream, hist, hcap, hv,
                       x, n, win, wlen, hist_out, drop, hv2);
    return launched();
}

extern "C" int wv_segment_track_bytes(int S, int nb, int min_gap_frames, int capacity, size_t* state_bytes, size_t* event_bytes) {
    if (!state_bytes || !event_bytes || S < 1 || S > 65535 || nb < 1 || nb > WV_SEGMENT_MAX_BITS || min_gap_frames < 1 ||
        min_gap_frames > WV_SEGMENT_MAX_GAP || capacity < 1)
        return fail(WV_EINVAL, "wv_segment_track_bytes: null output, S outside [1, 65535], nb outside [1, " WV_STR(WV_SEGMENT_MAX_BITS)
                               "], min_gap_frames outside [1, " WV_STR(WV_SEGMENT_MAX_GAP) "] or capacity < 1");
    const wv::SegLayout l = wv::seg_layout(nb, min_gap_frames, capacity);
    *state_bytes = (size_t)S * l.state_stride;
    *event_bytes = (size_t)S * l.event_stride;
    return WV_OK;
}

extern "C" int wv_segment_track(const float* fsum, int S, int nb, int Fr_stride, int f_lo, int f_hi, int64_t frame0, int hop, int last_valid,
                                int final, double min_on, int min_gap_frames, int min_len_frames, float eps, void* state, size_t state_bytes,
                                void* events, size_t event_bytes, int capacity, void* stream) {
    if (!state || !events || S < 1 || S > 65535 || nb < 1 || nb > WV_SEGMENT_MAX_BITS)
        return fail(WV_EINVAL, "wv_segment_track: null state / events, S outside [1, 65535] or nb outside [1, " WV_STR(WV_SEGMENT_MAX_BITS) "]");
    if (min_gap_frames < 1 || min_gap_frames > WV_SEGMENT_MAX_GAP || min_len_frames < 0 || capacity < 1 || !(min_on == min_on))
        return fail(WV_EINVAL, "wv_segment_track: min_gap_frames outside [1, " WV_STR(WV_SEGMENT_MAX_GAP) "], min_len_frames < 0, capacity < 1 or "
                               "min_on not a number");
    if (f_lo < 0 || f_hi < f_lo || f_hi > Fr_stride || (f_hi > f_lo && !fsum) || frame0 < 0 || hop < 1 || last_valid < 0 || last_valid > hop)
        return fail(WV_EINVAL, "wv_segment_track: frames [f_lo, f_hi) outside [0, Fr_stride] (or frames without fsum), frame0 < 0, hop < 1 or "
                               "last_valid outside [0, hop]");
    const wv::SegLayout l = wv::seg_layout(nb, min_gap_frames, capacity);
    if (state_bytes < (size_t)S * l.state_stride || event_bytes < (size_t)S * l.event_stride || ((uintptr_t)state & 7) || ((uintptr_t)events & 7))
        return fail(WV_EINVAL, "wv_segment_track: state or events shorter than wv_segment_track_bytes gives, or not 8-byte aligned");
    if (f_hi == f_lo && !final) return WV_OK;
    const int nt = (nb + 1 + 63) / 64 * 64;
    hipLaunchKernelGGL(wv::segment_track_kernel, dim3(S), dim3(nt), 0, (hipStream_t)stream, fsum, nb, Fr_stride, f_lo, f_hi - f_lo, (long long)frame0,
                       hop, last_valid, final, min_on, min_gap_frames, min_len_frames, eps, (char*)state, l.state_stride, (char*)events,
                       l.event_stride, l.rec, capacity);
    return launched();
}
