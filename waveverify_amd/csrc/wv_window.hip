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
//   bank_advance_kernel    a session bank's tick: a descriptor per stream that pushed, its history shifted in place, its window row filled
//   bank_detect_update_kernel  a detect bank's tick: the windows' sigmoid sums into the per-slot f64 accumulators, mean probabilities and bits out
//   segment_track_kernel   a live segment session's tick: the new frames' sums -> the per-stream open run, gap ring and ring of closed segments
//   bank_segment_track_kernel  a segment bank's tick: the same per-stream body, a descriptor per slot with its own frame range and row block
//   segment_split_kernel / bank_segment_split_kernel  the two trackers under a split rule: a run is also cut where the decoded id changes
//   span_gather_kernel     span embedding: packed clips -> a left-aligned, right-zero-padded window batch, a {offset, length} descriptor per row
//   span_scatter_add_kernel  span embedding: out = x + w * residual over each row's keep range, w the span's gain and edge ramp
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

// ---- session banks: every stream its own tick --------------------------------------------------------------------
// One descriptor row of wv_bank_advance, checked the same way by every workgroup that serves it: a row that breaks the contract is skipped whole.
struct BankRow {
    int64_t slot, hv, x_off, n, row, wlen, drop, hv2;
    bool ok;
};

__device__ __forceinline__ BankRow bank_row(const int64_t* __restrict__ desc, int p, int capacity, int hcap, int64_t n_x, int A, int Lmax) {
    const int64_t* d = desc + 8 * (size_t)p;
    BankRow r = {d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], false};
    if (r.slot < 0 || r.slot >= capacity || r.hv < 0 || r.hv > hcap || r.hv2 < 0 || r.hv2 > hcap || r.n < 0 || r.n > n_x || r.x_off < 0 ||
        r.x_off > n_x - r.n)
        return r;
    const int64_t len = r.hv + r.n;                             // both within their ranges: no overflow
    r.ok = r.drop >= 0 && r.drop <= len && r.drop + r.hv2 == len && r.wlen >= 0 && r.wlen <= len && r.wlen <= Lmax &&
           (r.wlen == 0 || (r.row >= 0 && r.row < A));
    return r;
}

// four samples q .. q + 3 (the first `count` of them) of cat(h[0 .. hv), xs[0 .. n)): one 16-byte load where all four lie in one source and
// that address is aligned
__device__ __forceinline__ float4 bank_load4(const float* h, int hv, const float* xs, int q, int count) {
    if (count == 4 && q + 4 <= hv && aligned16(h + q)) return *reinterpret_cast<const float4*>(h + q);
    if (count == 4 && q >= hv && aligned16(xs + (q - hv))) return *reinterpret_cast<const float4*>(xs + (q - hv));
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (count > 0) v.x = q < hv ? h[q] : xs[q - hv];
    if (count > 1) v.y = q + 1 < hv ? h[q + 1] : xs[q + 1 - hv];
    if (count > 2) v.z = q + 2 < hv ? h[q + 2] : xs[q + 2 - hv];
    if (count > 3) v.w = q + 3 < hv ? h[q + 3] : xs[q + 3 - hv];
    return v;
}

__device__ __forceinline__ void bank_store4(float* d, int count, float4 v) {
    if (count == 4 && aligned16(d)) {
        *reinterpret_cast<float4*>(d) = v;
        return;
    }
    if (count > 0) d[0] = v.x;
    if (count > 1) d[1] = v.y;
    if (count > 2) d[2] = v.z;
    if (count > 3) d[3] = v.w;
}

// grid (1 + ceil(Lmax / WIN_TILE), P).  Row p's stream is cat(hist[slot][0 .. hv), x[x_off .. x_off + n)).
//   blockIdx.x == 0  owns the slot's history, the only memory of this launch that is read and written: it first copies the window's
//                    history-sourced columns [0, min(hv, wlen)), then shifts the history IN PLACE to the stream's samples [drop, drop + hv2) in
//                    ascending chunks of WIN_TILE.  A chunk at offset c reads hist[c + drop ..) (or x) and writes hist[c .. c + WIN_TILE): every
//                    load of a chunk comes before the barrier, every store after it, so a store never meets a load of its own chunk, and the
//                    loads of the next chunk start at or beyond where this one's stores end.  No other workgroup touches this history row.
//   blockIdx.x >= 1  tile blockIdx.x - 1 of the window row: the x-sourced columns [hv, wlen) and the zeros [wlen, Lmax).  x and win alias
//                    nothing, so these tiles need no order among themselves or with the owner, whose columns they leave out.
__global__ __launch_bounds__(WIN_NT) void bank_advance_kernel(float* hist, int capacity, int hcap, const float* __restrict__ x, int64_t n_x,
                                                              const int64_t* __restrict__ desc, float* __restrict__ win, int A, int Lmax) {
    const BankRow r = bank_row(desc, blockIdx.y, capacity, hcap, n_x, A, Lmax);
    if (!r.ok) return;
    const int hv = (int)r.hv, wlen = (int)r.wlen, drop = (int)r.drop, hv2 = (int)r.hv2;
    const int hw = hv < wlen ? hv : wlen;                       // window columns that come from the history
    const float* xs = x + r.x_off;                              // never dereferenced where n == 0
    float* w = wlen ? win + (size_t)r.row * Lmax : win;         // never dereferenced where wlen == 0 (then hw == 0 and no tile has work)
    if (blockIdx.x > 0) {
        if (wlen == 0) return;
        const int j = (blockIdx.x - 1) * WIN_TILE + threadIdx.x * WIN_PER_THREAD;
        if (j >= Lmax) return;
        const int count = Lmax - j < 4 ? Lmax - j : 4;
        if (j >= wlen) {
            bank_store4(w + j, count, make_float4(0.f, 0.f, 0.f, 0.f));
        } else if (j >= hw && j + count <= wlen) {              // j >= hw and j < wlen: hw == hv, so every sample is x's
            bank_store4(w + j, count, bank_load4(xs, 0, xs, j - hv, count));
        } else {
            for (int i = 0; i < count; ++i)                     // a group that straddles hw or wlen
                if (j + i >= hw) w[j + i] = j + i < wlen ? xs[j + i - hv] : 0.f;
        }
        return;
    }
    float* h = hist + (size_t)r.slot * hcap;
    for (int c = 0; c < hw; c += WIN_TILE) {
        const int j = c + threadIdx.x * WIN_PER_THREAD;
        if (j < hw) {
            const int count = hw - j < 4 ? hw - j : 4;
            bank_store4(w + j, count, bank_load4(h, hv, xs, j, count));
        }
    }
    if (drop == 0 && r.n == 0) return;                          // nothing moves
    // with drop == 0 the first hv samples stay where they are: the copy starts at the chunk that holds hv
    for (int c = drop == 0 ? hv / WIN_TILE * WIN_TILE : 0; c < hv2; c += WIN_TILE) {
        const int j = c + threadIdx.x * WIN_PER_THREAD;
        const int count = j >= hv2 ? 0 : (hv2 - j < 4 ? hv2 - j : 4);
        const float4 v = bank_load4(h, hv, xs, j + drop, count);
        __syncthreads();
        bank_store4(h + j, count, v);
    }
}

// grid (A), one thread per (row, bit), bits beyond the block in a stride loop.  desc[r] = {slot, samples}.  Every thread reads the slot's
// counter before the barrier, thread 0 writes it after.
__global__ __launch_bounds__(WIN_NT) void bank_detect_update_kernel(double* acc, int64_t* seen, int capacity, int nb, const float* __restrict__ psum,
                                                                    const int64_t* __restrict__ desc, float* __restrict__ mean_prob,
                                                                    int* __restrict__ bits) {
    const int r = blockIdx.x;
    const int64_t slot = desc[2 * r], samples = desc[2 * r + 1];
    if (slot < 0 || slot >= capacity || samples < 0) return;
    const int64_t total = seen[slot] + samples;
    __syncthreads();
    if (threadIdx.x == 0) seen[slot] = total;
    const double den = (double)(total > 1 ? total : 1);
    for (int k = threadIdx.x; k < nb; k += blockDim.x) {
        const double a = acc[(size_t)slot * nb + k] + (double)psum[(size_t)r * nb + k];
        acc[(size_t)slot * nb + k] = a;
        const float mp = (float)(a / den);
        mean_prob[(size_t)r * nb + k] = mp;
        bits[(size_t)r * nb + k] = mp >= 0.5f ? 1 : 0;
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

// One stream's tick, run by one workgroup of nb + 1 threads rounded up to a wave (segment_track_kernel and bank_segment_track_kernel both call
// it, every thread of the workgroup together).  fs: the stream's rows at this tick's first column, row k at fs + k * Fr; n frames, the first
// being the stream's frame frame0; st / ev: the stream's own state and event sections.  Thread k <= nb owns row k of the sums (row nb is the
// count row); EVERY thread reads the count row of every frame and keeps the run's count sum itself, so all threads of a stream take the same
// decisions without exchanging anything.  Frames of this tick are read from fsum wherever they are needed; the ring only carries the off
// frames after `hi` over to the next tick (frame j in slot j % (G - 1); at most G - 1 consecutive frames are ever held, so slots never
// collide).  A run is closed as soon as G off frames have passed, hence an on frame that meets an open run always has a gap < G and merges.
// Reads of the state come before the barrier, writes after it; event records are write-only.
__device__ __forceinline__ void segment_track_stream(const float* __restrict__ fs, size_t Fr, int nb, int n, long long frame0, int hop, int last_valid,
                                                     int final_, double min_on, int G, int min_len, float eps, char* st, char* ev, size_t rec,
                                                     int capacity) {
    const int k = threadIdx.x;
    const bool owns = k <= nb;
    const int r = owns ? k : nb;
    const float* crow = fs + (size_t)nb * Fr;
    const float* krow = fs + (size_t)r * Fr;
    long long* hdr = reinterpret_cast<long long*>(st);
    double* accp = reinterpret_cast<double*>(hdr + 4);
    float* ring = reinterpret_cast<float*>(accp + nb + 1);
    long long* nevp = reinterpret_cast<long long*>(ev);
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

// grid (S), block = nb + 1 rounded up to a wave: stream s = blockIdx.x of S lockstep streams, all on the same frame range.
__global__ __launch_bounds__(256) void segment_track_kernel(const float* __restrict__ fsum, int nb, int Fr, int f_lo, int n, long long frame0, int hop,
                                                            int last_valid, int final_, double min_on, int G, int min_len, float eps, char* state,
                                                            size_t state_stride, char* events, size_t event_stride, size_t rec, int capacity) {
    const int s = blockIdx.x;
    segment_track_stream(fsum + (size_t)s * (nb + 1) * Fr + f_lo, (size_t)Fr, nb, n, frame0, hop, last_valid, final_, min_on, G, min_len, eps,
                         state + (size_t)s * state_stride, events + (size_t)s * event_stride, rec, capacity);
}

// ---- segment banks: every slot its own frame range ------------------------------------------------------------
// One descriptor row of wv_bank_segment_track = {slot, fsum_off, Fr_stride, f_lo, f_hi, frame0, last_valid, final}; a row that breaks the
// contract is skipped whole (session.bank_track_row_ok restates the predicate).  The divisions keep every product inside int64.
struct TrackRow {
    int64_t slot, off, Fr, f_lo, f_hi, frame0, last_valid, final_;
    bool ok;
};

__device__ __forceinline__ TrackRow track_row(const int64_t* __restrict__ desc, int p, int capacity, int nb, int hop, int64_t n_fsum) {
    const int64_t* d = desc + 8 * (size_t)p;
    TrackRow r = {d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], false};
    r.ok = r.slot >= 0 && r.slot < capacity && r.Fr >= 0 && r.Fr <= 0x7fffffffLL && r.f_lo >= 0 && r.f_lo <= r.f_hi && r.f_hi <= r.Fr && r.off >= 0 &&
           r.off <= n_fsum && r.Fr <= (n_fsum - r.off) / (nb + 1) && r.frame0 >= 0 && r.last_valid >= 0 && r.last_valid <= hop;
    return r;
}

// grid (P), block = nb + 1 rounded up to a wave.  Workgroup p serves descriptor p: the body is segment_track_stream on the slot's own state and
// event sections, its rows at fsum + fsum_off.  A row without frames that is not final changes nothing and returns at once, as wv_segment_track
// launches nothing for such a tick.  The row is read alike by every thread, so a workgroup leaves whole or runs whole.
__global__ __launch_bounds__(256) void bank_segment_track_kernel(const float* __restrict__ fsum, int64_t n_fsum, const int64_t* __restrict__ desc,
                                                                 int capacity, int nb, int hop, double min_on, int G, int min_len, float eps,
                                                                 char* state, size_t state_stride, char* events, size_t event_stride, size_t rec,
                                                                 int ring) {
    const TrackRow r = track_row(desc, blockIdx.x, capacity, nb, hop, n_fsum);
    if (!r.ok || (r.f_hi == r.f_lo && !r.final_)) return;
    segment_track_stream(fsum + r.off + r.f_lo, (size_t)r.Fr, nb, (int)(r.f_hi - r.f_lo), (long long)r.frame0, hop, (int)r.last_valid,
                         r.final_ != 0, min_on, G, min_len, eps, state + (size_t)r.slot * state_stride, events + (size_t)r.slot * event_stride,
                         rec, ring);
}

// ---- splitting a run where the decoded id changes (localize.SplitRule is the definition) -------------------------
// Byte layout (the header states it for callers): per stream `state` holds int64 {open, lo, hi, frames seen, plo, pending 0/1, cg}, f64 cS,
// f64 sums [nb + 1] of the current piece over [plo, sb) and the ring [2 W + G][nb + 1] f32 of raw frame columns, frame j in slot
// j % (2 W + G); `events` holds an int64 event counter and `capacity` records {int64 lo, int64 hi, f64 count, int64 flags, f32 prob[nb]}.
// The next boundary to evaluate, gn = max(plo + W, hi - W + 1), and the first frame still in the ring, sb = max(plo, gn - W), follow from
// the header: every boundary with W frames of the run on its right is evaluated as soon as `hi` allows it.
static inline SegLayout split_layout(int nb, int G, int W, int capacity) {
    SegLayout l;
    l.state_stride = 64 + 8 * (size_t)(nb + 1) + up8(4 * (size_t)(2 * W + G) * (nb + 1));
    l.rec = 32 + up8(4 * (size_t)nb);
    l.event_stride = 8 + (size_t)capacity * l.rec;
    return l;
}

struct SplitShared {
    double L[256], R[256], D[256], cnt;
    int V[256];
};

// One stream's tick under a split rule, run by one workgroup of nb + 1 threads rounded up to a wave, every thread together (the barriers
// inside are reached by all: every decision below is taken alike by every thread, from the count row of fsum, which all read, and from values
// that went through LDS).  Thread k <= nb owns row k: its window sums, its row of the ring and its piece sum.  A frame column stays in the
// ring while a cut may still fall before it (from sb on); it joins the piece's f64 sum, in ascending order, when sb passes it or when its
// piece is emitted, so the sum is one ascending pass over the piece whatever the ticks.  Frames of this tick are read from fsum, older ones
// from the ring; at the end of the tick the columns from max(sb, frame0) on go into the ring (fewer than 2 W + G, so slots never collide).
// Reads of the state come before the last barrier, writes after it; event records are write-only.
__device__ __forceinline__ void segment_split_stream(const float* __restrict__ fs, size_t Fr, int nb, int n, long long frame0, int hop, int last_valid,
                                                     int final_, double min_on, int G, int min_len, float eps, int W, double thr, int min_bits,
                                                     char* st, char* ev, size_t rec, int capacity, SplitShared& sh) {
    const int k = threadIdx.x;
    const bool owns = k <= nb;
    const int r = owns ? k : nb;
    const float* crow = fs + (size_t)nb * Fr;
    const float* krow = fs + (size_t)r * Fr;
    long long* hdr = reinterpret_cast<long long*>(st);
    double* cSp = reinterpret_cast<double*>(hdr + 7);
    double* accp = cSp + 1;
    float* ring = reinterpret_cast<float*>(accp + nb + 1);
    long long* nevp = reinterpret_cast<long long*>(ev);
    char* recs = reinterpret_cast<char*>(nevp + 1);
    const int RC = 2 * W + G;

    bool open = hdr[0] != 0, pend = hdr[5] != 0;
    long long lo = hdr[1], hi = hdr[2], plo = hdr[4], cg = hdr[6], nev = *nevp;
    double cS = *cSp, acc = accp[r];
    // a state that cannot follow from zeros and gapless ticks is taken as closed; ring slots are addressed by j % RC with j >= 0 only
    if (open && !(frame0 <= (1LL << 62) && lo >= 0 && lo <= plo && plo < hi && hi <= frame0 && frame0 - hi < G && (hdr[5] == 0 || hdr[5] == 1)))
        open = false;
    if (open && pend) {
        const long long gn0 = plo + W > hi - W + 1 ? plo + W : hi - W + 1;
        if (!(cg >= plo + W && cg <= hi - W && gn0 - cg <= W)) open = false;
    }
    if (!open) pend = false;
    if (nev < 0 || nev > (1LL << 62)) nev = 0;
    long long gn = 0, sb = 0;
    if (open) {
        gn = plo + W > hi - W + 1 ? plo + W : hi - W + 1;
        sb = plo > gn - W ? plo : gn - W;
    }

    auto col = [&](long long j) -> double {
        return (double)(j >= frame0 ? krow[j - frame0] : ring[(size_t)(j % RC) * (nb + 1) + r]);
    };
    auto add_to = [&](long long e) {
        for (; sb < e; ++sb) acc += col(sb);
    };
    // the piece [plo, e) becomes the next event; flags bit 0: its start is a cut, bit 1: its end is one
    auto emit = [&](long long e, long long flags) {
        add_to(e);
        if (k == nb) sh.cnt = acc;
        __syncthreads();
        const double cnt = sh.cnt;
        char* rp = recs + (size_t)(nev % capacity) * rec;
        if (k == 0) {
            reinterpret_cast<long long*>(rp)[0] = plo;
            reinterpret_cast<long long*>(rp)[1] = e;
            reinterpret_cast<double*>(rp)[2] = cnt;
            reinterpret_cast<long long*>(rp)[3] = flags | (plo > lo ? 1 : 0);
        }
        if (k < nb) {
            const float d = (float)cnt + eps;
            reinterpret_cast<float*>(rp + 32)[k] = cnt > 0.0 ? (float)(acc / (double)d) : 0.f;
        }
        ++nev;
        __syncthreads();
    };
    auto commit = [&]() {
        emit(cg, 2);
        plo = cg;
        pend = false;
        acc = 0.0;
    };
    auto evaluate = [&](long long g) {
        if (pend && g - cg >= W) commit();
        double L = 0.0, Rs = 0.0;
        for (long long j = g - W; j < g; ++j) L += col(j);
        for (long long j = g; j < g + W; ++j) Rs += col(j);
        if (owns) {
            sh.L[k] = L;
            sh.R[k] = Rs;
        }
        __syncthreads();
        const double Ln = sh.L[nb], Rn = sh.R[nb];
        const bool ok = Ln > 0.0 && Rn > 0.0;
        if (ok && k < nb) {
            const double pL = L / Ln, pR = Rs / Rn;
            sh.D[k] = fabs(pL - pR);
            sh.V[k] = (pL >= 0.5) != (pR >= 0.5) ? 1 : 0;
        }
        __syncthreads();
        if (ok) {
            double S = 0.0;
            int d = 0;
            for (int q = 0; q < nb; ++q) {
                S += sh.D[q];
                d += sh.V[q];
            }
            if (S >= thr && d >= min_bits && (!pend || S > cS)) {
                pend = true;
                cg = g;
                cS = S;
            }
        }
        __syncthreads();
    };
    auto close = [&]() {
        if (hi - lo >= min_len) {
            if (pend) commit();
            emit(hi, 0);
        }
        open = pend = false;
    };

    for (int i = 0; i < n; ++i) {
        const long long g = frame0 + i;
        const float c = crow[i];
        const int valid = (final_ && i == n - 1) ? last_valid : hop;
        const bool on = valid > 0 && (double)c >= min_on * (double)valid;
        if (on) {
            if (!open) {
                open = true;
                pend = false;
                lo = plo = sb = g;
                gn = g + W;
                acc = 0.0;
            }
            hi = g + 1;
            while (gn + W <= hi) {
                evaluate(gn);
                ++gn;
                add_to(plo > gn - W ? plo : gn - W);
            }
        } else if (open && g + 1 - hi >= G) {
            close();
        }
    }
    if (final_ && open) close();
    __syncthreads();

    const long long fend = frame0 + n;
    if (owns) {
        if (open)
            for (long long j = sb > frame0 ? sb : frame0; j < fend; ++j) ring[(size_t)(j % RC) * (nb + 1) + k] = krow[j - frame0];
        accp[k] = acc;
    }
    if (k == 0) {
        hdr[0] = open ? 1 : 0;
        hdr[1] = lo;
        hdr[2] = hi;
        hdr[3] = fend;
        hdr[4] = plo;
        hdr[5] = pend ? 1 : 0;
        hdr[6] = cg;
        *cSp = cS;
        *nevp = nev;
    }
}

// grid (S), block = nb + 1 rounded up to a wave: wv_segment_track's launch shape with the split body.
__global__ __launch_bounds__(256) void segment_split_kernel(const float* __restrict__ fsum, int nb, int Fr, int f_lo, int n, long long frame0, int hop,
                                                            int last_valid, int final_, double min_on, int G, int min_len, float eps, int W,
                                                            double thr, int min_bits, char* state, size_t state_stride, char* events,
                                                            size_t event_stride, size_t rec, int capacity) {
    __shared__ SplitShared sh;
    const int s = blockIdx.x;
    segment_split_stream(fsum + (size_t)s * (nb + 1) * Fr + f_lo, (size_t)Fr, nb, n, frame0, hop, last_valid, final_, min_on, G, min_len, eps, W, thr,
                         min_bits, state + (size_t)s * state_stride, events + (size_t)s * event_stride, rec, capacity, sh);
}

// grid (P), block = nb + 1 rounded up to a wave: wv_bank_segment_track's descriptors and row predicate with the split body.
__global__ __launch_bounds__(256) void bank_segment_split_kernel(const float* __restrict__ fsum, int64_t n_fsum, const int64_t* __restrict__ desc,
                                                                 int capacity, int nb, int hop, double min_on, int G, int min_len, float eps, int W,
                                                                 double thr, int min_bits, char* state, size_t state_stride, char* events,
                                                                 size_t event_stride, size_t rec, int ring) {
    __shared__ SplitShared sh;
    const TrackRow r = track_row(desc, blockIdx.x, capacity, nb, hop, n_fsum);
    if (!r.ok || (r.f_hi == r.f_lo && !r.final_)) return;
    segment_split_stream(fsum + r.off + r.f_lo, (size_t)r.Fr, nb, (int)(r.f_hi - r.f_lo), (long long)r.frame0, hop, (int)r.last_valid,
                         r.final_ != 0, min_on, G, min_len, eps, W, thr, min_bits, state + (size_t)r.slot * state_stride,
                         events + (size_t)r.slot * event_stride, rec, ring, sh);
}

// ---- span embedding: windows of chosen stretches, the residual added inside the stretch only -------------------
// grid (ceil(Lmax / WIN_TILE), A).  desc[r] = {src offset, wlen}: row r = src[off .. off + wlen), then zeros in [wlen, Lmax).  A row that
// reaches outside src or beyond Lmax is skipped whole (not even zero-filled).
__global__ __launch_bounds__(WIN_NT) void span_gather_kernel(const float* __restrict__ src, int64_t n_src, const int64_t* __restrict__ desc,
                                                             float* __restrict__ dst, int Lmax) {
    const int r = blockIdx.y;
    const int64_t off = desc[2 * r], wl = desc[2 * r + 1];
    if (off < 0 || wl < 0 || wl > Lmax || off > n_src - wl) return;
    const int wlen = (int)wl;
    const float* s = src + off;                                 // never dereferenced where wlen == 0
    float* d = dst + (size_t)r * Lmax;
    const int j = blockIdx.x * WIN_TILE + threadIdx.x * WIN_PER_THREAD;
    if (j >= Lmax) return;
    const int count = Lmax - j < 4 ? Lmax - j : 4;
    if (j >= wlen) {
        bank_store4(d + j, count, make_float4(0.f, 0.f, 0.f, 0.f));
    } else if (j + 4 <= wlen) {
        bank_store4(d + j, 4, bank_load4(s, 0, s, j, 4));       // hv = 0: every sample is the second source's
    } else {
        for (int i = 0; i < count; ++i) d[j + i] = j + i < wlen ? s[j + i] : 0.f;   // a group that straddles wlen
    }
}

// One descriptor row of wv_span_scatter_add = {offset in out of the window's column 0, keep lo, keep hi, span start, span end}, the last four
// relative to the window's column 0; a row that breaks the contract is skipped whole (window.span_row_ok restates the predicate).
struct SpanRow {
    int64_t o, lo, hi, ss, se;
    bool ok;
};

__device__ __forceinline__ SpanRow span_row(const int64_t* __restrict__ desc, int r, int64_t n_out, int Lmax) {
    const int64_t* d = desc + 5 * (size_t)r;
    SpanRow s = {d[0], d[1], d[2], d[3], d[4], false};
    s.ok = s.lo >= 0 && s.lo < s.hi && s.hi <= Lmax && s.ss <= s.lo && s.hi <= s.se && s.o >= -s.lo && s.o <= n_out - s.hi;
    return s;
}

// w(j) = gain * ramp[m] for m = min(j - span start, span end - 1 - j) < F, else gain.  An edge farther than F from j counts as F, so a span
// edge anywhere in int64 never overflows the difference.
__device__ __forceinline__ float span_weight(const SpanRow& s, int64_t j, const float* __restrict__ ramp, int F, float gain) {
    const int64_t a = s.ss < j - F ? F : j - s.ss, b = s.se > j + F ? F : s.se - 1 - j;
    const int64_t m = a < b ? a : b;
    return m < F ? gain * ramp[m] : gain;
}

// grid (ceil(Lmax / WIN_TILE), A): for j in [lo, hi) out[o + j] = x[o + j] + w(j) * y[r][j] (w * y alone where x is null), three roundings.
// x may be out: a thread reads x[o + j] before it writes out[o + j], and nobody else touches that element.  x and out carry no __restrict__.
__global__ __launch_bounds__(WIN_NT) void span_scatter_add_kernel(const float* __restrict__ y, const float* x, const int64_t* __restrict__ desc,
                                                                  const float* __restrict__ ramp, int F, float gain, float* out, int64_t n_out,
                                                                  int Lmax) {
    const int r = blockIdx.y;
    const SpanRow s = span_row(desc, r, n_out, Lmax);
    if (!s.ok) return;
    const int lo = (int)s.lo, hi = (int)s.hi;
    const int j = blockIdx.x * WIN_TILE + threadIdx.x * WIN_PER_THREAD;
    if (j + WIN_PER_THREAD <= lo || j >= hi) return;
    const float* yr = y + (size_t)r * Lmax;
    const float* xr = x ? x + s.o : nullptr;
    float* d = out + s.o;
    if (j >= lo && j + WIN_PER_THREAD <= hi && aligned16(yr + j) && aligned16(d + j) && (!xr || aligned16(xr + j))) {
        const float4 v = *reinterpret_cast<const float4*>(yr + j);
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
        if (xr) u = *reinterpret_cast<const float4*>(xr + j);
        const float p0 = span_weight(s, j, ramp, F, gain) * v.x, p1 = span_weight(s, j + 1, ramp, F, gain) * v.y;
        const float p2 = span_weight(s, j + 2, ramp, F, gain) * v.z, p3 = span_weight(s, j + 3, ramp, F, gain) * v.w;
        *reinterpret_cast<float4*>(d + j) = xr ? make_float4(u.x + p0, u.y + p1, u.z + p2, u.w + p3) : make_float4(p0, p1, p2, p3);
        return;
    }
#pragma unroll
    for (int i = 0; i < WIN_PER_THREAD; ++i) {
        const int q = j + i;
        if (q >= lo && q < hi) {
            const float p = span_weight(s, q, ramp, F, gain) * yr[q];
            d[q] = xr ? xr[q] + p : p;
        }
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

static bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && p < q + b_bytes && q < p + a_bytes;
}

extern "C" int wv_bank_advance(float* hist, int capacity, int hcap, const float* x, int64_t n_x, const int64_t* desc, int P, float* win, int A,
                               int Lmax, void* stream) {
    if (!hist || !desc || (n_x > 0 && !x) || (A > 0 && !win))
        return fail(WV_EINVAL, "wv_bank_advance: null hist or desc, samples without x, or window rows without win");
    if (capacity < 1 || capacity > WV_BANK_MAX_SLOTS || hcap < 1 || n_x < 0 || P < 0 || P > 65535 || A < 0 || A > 65535 || Lmax < 0 || (A > 0 && Lmax < 1))
        return fail(WV_EINVAL, "wv_bank_advance: capacity outside [1, " WV_STR(WV_BANK_MAX_SLOTS) "], hcap < 1, n_x < 0, P or A outside [0, 65535], "
                               "Lmax < 0, or window rows of no length");
    const size_t hb = (size_t)capacity * hcap * 4, xb = (size_t)n_x * 4, wb = (size_t)A * Lmax * 4;
    if (overlap(hist, hb, x, xb) || overlap(hist, hb, win, wb) || overlap(x, xb, win, wb))
        return fail(WV_EINVAL, "wv_bank_advance: hist, x and win must not overlap");
    if (P == 0) return WV_OK;
    const int tiles = A > 0 ? (Lmax + wv::WIN_TILE - 1) / wv::WIN_TILE : 0;
    hipLaunchKernelGGL(wv::bank_advance_kernel, dim3(1 + tiles, P), dim3(wv::WIN_NT), 0, (hipStream_t)stream, hist, capacity, hcap, x, n_x, desc, win,
                       A, Lmax);
    return launched();
}

extern "C" int wv_bank_detect_update(double* acc, int64_t* seen, int capacity, int nb, const float* psum, const int64_t* desc, int A,
                                     float* mean_prob, int* bits, void* stream) {
    if (!acc || !seen || !psum || !desc || !mean_prob || !bits)
        return fail(WV_EINVAL, "wv_bank_detect_update: null pointer (acc, seen, psum, desc, mean_prob, bits)");
    if (capacity < 1 || capacity > WV_BANK_MAX_SLOTS || nb < 1 || A < 0 || A > 65535)
        return fail(WV_EINVAL, "wv_bank_detect_update: capacity outside [1, " WV_STR(WV_BANK_MAX_SLOTS) "], nb < 1 or A outside [0, 65535]");
    if (A == 0) return WV_OK;
    hipLaunchKernelGGL(wv::bank_detect_update_kernel, dim3(A), dim3(nb <= 64 ? 64 : wv::WIN_NT), 0, (hipStream_t)stream, acc, seen, capacity, nb, psum,
                       desc, mean_prob, bits);
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

extern "C" int wv_bank_segment_track(const float* fsum, int64_t n_fsum, const int64_t* desc, int P, int capacity, int nb, int hop, double min_on,
                                     int min_gap_frames, int min_len_frames, float eps, void* state, size_t state_bytes, void* events,
                                     size_t event_bytes, int ring, void* stream) {
    if (!desc || !state || !events || n_fsum < 0 || (n_fsum > 0 && !fsum))
        return fail(WV_EINVAL, "wv_bank_segment_track: null desc, state or events, n_fsum < 0, or frame sums without fsum");
    if (capacity < 1 || capacity > WV_BANK_MAX_SLOTS || P < 0 || P > 65535 || nb < 1 || nb > WV_SEGMENT_MAX_BITS || hop < 1)
        return fail(WV_EINVAL, "wv_bank_segment_track: capacity outside [1, " WV_STR(WV_BANK_MAX_SLOTS) "], P outside [0, 65535], nb outside [1, "
                               WV_STR(WV_SEGMENT_MAX_BITS) "] or hop < 1");
    if (min_gap_frames < 1 || min_gap_frames > WV_SEGMENT_MAX_GAP || min_len_frames < 0 || ring < 1 || !(min_on == min_on))
        return fail(WV_EINVAL, "wv_bank_segment_track: min_gap_frames outside [1, " WV_STR(WV_SEGMENT_MAX_GAP) "], min_len_frames < 0, ring < 1 or "
                               "min_on not a number");
    const wv::SegLayout l = wv::seg_layout(nb, min_gap_frames, ring);
    if (state_bytes / l.state_stride < (size_t)capacity || event_bytes / l.event_stride < (size_t)capacity || ((uintptr_t)state & 7) ||
        ((uintptr_t)events & 7))
        return fail(WV_EINVAL, "wv_bank_segment_track: state or events shorter than wv_segment_track_bytes gives for `capacity` streams, or not "
                               "8-byte aligned");
    if (P == 0) return WV_OK;
    const int nt = (nb + 1 + 63) / 64 * 64;
    hipLaunchKernelGGL(wv::bank_segment_track_kernel, dim3(P), dim3(nt), 0, (hipStream_t)stream, fsum, n_fsum, desc, capacity, nb, hop, min_on,
                       min_gap_frames, min_len_frames, eps, (char*)state, l.state_stride, (char*)events, l.event_stride, l.rec, ring);
    return launched();
}

static const char* split_rule_bad(int nb, int G, int min_len, int W, double thr, int min_bits) {
    const int need = G > min_len ? (G > 2 ? G : 2) : (min_len > 2 ? min_len : 2);
    if (W < need || W > WV_SPLIT_MAX_WINDOW) return "window_frames outside [max(2, min_gap_frames, min_len_frames), " WV_STR(WV_SPLIT_MAX_WINDOW) "]";
    if (!(thr > 0.0)) return "threshold not above 0";
    if (min_bits < 1 || min_bits > nb) return "min_bits outside [1, nb]";
    return nullptr;
}

extern "C" int wv_segment_split_bytes(int S, int nb, int min_gap_frames, int window_frames, int capacity, size_t* state_bytes,
                                      size_t* event_bytes) {
    if (!state_bytes || !event_bytes || S < 1 || S > 65535 || nb < 1 || nb > WV_SEGMENT_MAX_BITS || min_gap_frames < 1 ||
        min_gap_frames > WV_SEGMENT_MAX_GAP || window_frames < 2 || window_frames > WV_SPLIT_MAX_WINDOW || capacity < 1)
        return fail(WV_EINVAL, "wv_segment_split_bytes: null output, S outside [1, 65535], nb outside [1, "
                               WV_STR(WV_SEGMENT_MAX_BITS) "], min_gap_frames outside [1, " WV_STR(WV_SEGMENT_MAX_GAP)
                               "], window_frames outside [2, " WV_STR(WV_SPLIT_MAX_WINDOW) "] or capacity < 1");
    const wv::SegLayout l = wv::split_layout(nb, min_gap_frames, window_frames, capacity);
    *state_bytes = (size_t)S * l.state_stride;
    *event_bytes = (size_t)S * l.event_stride;
    return WV_OK;
}

extern "C" int wv_segment_track_split(const float* fsum, int S, int nb, int Fr_stride, int f_lo, int f_hi, int64_t frame0, int hop, int last_valid,
                                      int final, double min_on, int min_gap_frames, int min_len_frames, float eps, int window_frames,
                                      double threshold, int min_bits, void* state, size_t state_bytes, void* events, size_t event_bytes,
                                      int capacity, void* stream) {
    if (!state || !events || S < 1 || S > 65535 || nb < 1 || nb > WV_SEGMENT_MAX_BITS)
        return fail(WV_EINVAL, "wv_segment_track_split: null state / events, S outside [1, 65535] or nb outside [1, " WV_STR(WV_SEGMENT_MAX_BITS) "]");
    if (min_gap_frames < 1 || min_gap_frames > WV_SEGMENT_MAX_GAP || min_len_frames < 0 || capacity < 1 || !(min_on == min_on))
        return fail(WV_EINVAL, "wv_segment_track_split: min_gap_frames outside [1, " WV_STR(WV_SEGMENT_MAX_GAP) "], min_len_frames < 0, capacity < 1 "
                               "or min_on not a number");
    if (const char* bad = split_rule_bad(nb, min_gap_frames, min_len_frames, window_frames, threshold, min_bits))
        return fail(WV_EINVAL, std::string("wv_segment_track_split: ") + bad);
    if (f_lo < 0 || f_hi < f_lo || f_hi > Fr_stride || (f_hi > f_lo && !fsum) || frame0 < 0 || hop < 1 || last_valid < 0 || last_valid > hop)
        return fail(WV_EINVAL, "wv_segment_track_split: frames [f_lo, f_hi) outside [0, Fr_stride] (or frames without fsum), frame0 < 0, hop < 1 or "
                               "last_valid outside [0, hop]");
    const wv::SegLayout l = wv::split_layout(nb, min_gap_frames, window_frames, capacity);
    if (state_bytes < (size_t)S * l.state_stride || event_bytes < (size_t)S * l.event_stride || ((uintptr_t)state & 7) || ((uintptr_t)events & 7))
        return fail(WV_EINVAL, "wv_segment_track_split: state or events shorter than wv_segment_split_bytes gives, or not 8-byte aligned");
    if (f_hi == f_lo && !final) return WV_OK;
    const int nt = (nb + 1 + 63) / 64 * 64;
    hipLaunchKernelGGL(wv::segment_split_kernel, dim3(S), dim3(nt), 0, (hipStream_t)stream, fsum, nb, Fr_stride, f_lo, f_hi - f_lo, (long long)frame0,
                       hop, last_valid, final, min_on, min_gap_frames, min_len_frames, eps, window_frames, threshold, min_bits, (char*)state,
                       l.state_stride, (char*)events, l.event_stride, l.rec, capacity);
    return launched();
}

extern "C" int wv_bank_segment_track_split(const float* fsum, int64_t n_fsum, const int64_t* desc, int P, int capacity, int nb, int hop, double min_on,
                                           int min_gap_frames, int min_len_frames, float eps, int window_frames, double threshold, int min_bits,
                                           void* state, size_t state_bytes, void* events, size_t event_bytes, int ring, void* stream) {
    if (!desc || !state || !events || n_fsum < 0 || (n_fsum > 0 && !fsum))
        return fail(WV_EINVAL, "wv_bank_segment_track_split: null desc, state or events, n_fsum < 0, or frame sums without fsum");
    if (capacity < 1 || capacity > WV_BANK_MAX_SLOTS || P < 0 || P > 65535 || nb < 1 || nb > WV_SEGMENT_MAX_BITS || hop < 1)
        return fail(WV_EINVAL, "wv_bank_segment_track_split: capacity outside [1, " WV_STR(WV_BANK_MAX_SLOTS) "], P outside [0, 65535], nb outside [1, "
                               WV_STR(WV_SEGMENT_MAX_BITS) "] or hop < 1");
    if (min_gap_frames < 1 || min_gap_frames > WV_SEGMENT_MAX_GAP || min_len_frames < 0 || ring < 1 || !(min_on == min_on))
        return fail(WV_EINVAL, "wv_bank_segment_track_split: min_gap_frames outside [1, " WV_STR(WV_SEGMENT_MAX_GAP) "], min_len_frames < 0, ring < 1 "
                               "or min_on not a number");
    if (const char* bad = split_rule_bad(nb, min_gap_frames, min_len_frames, window_frames, threshold, min_bits))
        return fail(WV_EINVAL, std::string("wv_bank_segment_track_split: ") + bad);
    const wv::SegLayout l = wv::split_layout(nb, min_gap_frames, window_frames, ring);
    if (state_bytes / l.state_stride < (size_t)capacity || event_bytes / l.event_stride < (size_t)capacity || ((uintptr_t)state & 7) ||
        ((uintptr_t)events & 7))
        return fail(WV_EINVAL, "wv_bank_segment_track_split: state or events shorter than wv_segment_split_bytes gives for `capacity` streams, or "
                               "not 8-byte aligned");
    if (P == 0) return WV_OK;
    const int nt = (nb + 1 + 63) / 64 * 64;
    hipLaunchKernelGGL(wv::bank_segment_split_kernel, dim3(P), dim3(nt), 0, (hipStream_t)stream, fsum, n_fsum, desc, capacity, nb, hop, min_on,
                       min_gap_frames, min_len_frames, eps, window_frames, threshold, min_bits, (char*)state, l.state_stride, (char*)events,
                       l.event_stride, l.rec, ring);
    return launched();
}

extern "C" int wv_span_gather(const float* src, int64_t n_src, const int64_t* desc, float* dst, int A, int Lmax, void* stream) {
    if (!desc || !dst || n_src < 0 || (n_src > 0 && !src))
        return fail(WV_EINVAL, "wv_span_gather: null desc or dst, n_src < 0, or samples without src");
    if (A < 0 || A > 65535 || Lmax < 1) return fail(WV_EINVAL, "wv_span_gather: A outside [0, 65535] or Lmax < 1");
    if (A == 0) return WV_OK;
    hipLaunchKernelGGL(wv::span_gather_kernel, dim3((Lmax + wv::WIN_TILE - 1) / wv::WIN_TILE, A), dim3(wv::WIN_NT), 0, (hipStream_t)stream, src, n_src,
                       desc, dst, Lmax);
    return launched();
}

extern "C" int wv_span_scatter_add(const float* y, const float* x, const int64_t* desc, const float* ramp, int F, float gain, float* out,
                                   int64_t n_out, int A, int Lmax, void* stream) {
    if (!y || !desc || !out || n_out < 1) return fail(WV_EINVAL, "wv_span_scatter_add: null y, desc or out, or n_out < 1");
    if (F < 0 || (F > 0 && !ramp) || !(gain == gain) || A < 0 || A > 65535 || Lmax < 1)
        return fail(WV_EINVAL, "wv_span_scatter_add: F < 0, a fade without ramp, gain not a number, A outside [0, 65535] or Lmax < 1");
    if (A == 0) return WV_OK;
    hipLaunchKernelGGL(wv::span_scatter_add_kernel, dim3((Lmax + wv::WIN_TILE - 1) / wv::WIN_TILE, A), dim3(wv::WIN_NT), 0, (hipStream_t)stream, y, x,
                       desc, ramp, F, gain, out, n_out, Lmax);
    return launched();
}
