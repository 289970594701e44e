// The per-channel SNR floor for LIVE native-rate banks: wv_native_bank_up_add's back stage with the floor of section 7d-12
// on it, for P descriptor rows of any mix of rates in ONE launch.  Per row, with seq_u = cat(uhold[0 .. uv), new u) and seq_x[c] =
// cat(pend[c][0 .. pv), x[c][0 .. n)), both starting at the stream's first sample not yet emitted, start(f0):
//     new u[m]     = native_up_add_stream's chain over cat(rhist, r) (native_chain, the same device function), nu = k + uv2 - uv of them
//     frames       f0 .. f0 + nf - 1, frame f = [start(f), start(f + 1)) - start(f0), start(f) = ceil(f * nw * hop / orig); at `final` the last is cut at k
//     Eu[f], Ex[c][f]   frame_energy's fixed order over seq_u and seq_x[c], k counted inside the frame
//     g[c][f]      = floor_gain(Ex, Eu, cap, rho); the gain before frame f0 is the slot's gprev; stream frame 0 takes its own and reads no state
//     out[c][i]    = floor_out(seq_x[c][i], floor_weight(g[c][f - 1], g[c][f], float32((i - start + 1) / L_f)) * seq_u[i], 1),  i < k
// and the four states roll into the slot's other half: rhist, pend (seq_x from k on), uhold (seq_u from k on), gprev (g[.][f0 + nf - 1]).
// Grid (blocks, P), 256 threads.  A row's blocks are: ceil(nf / NF) TILES of NF frames, then the blocks that roll rhist, pend and uhold, then (nf == 0
// only) one that carries gprev over.  A tile forms its u ONCE into LDS (and, when it is not the row's first, also u of the one frame before it, whose
// energies it needs for that frame's gain: gains have no recursion), then the energies, 16 lanes a sum, then the gains in LDS, then out.  out is never
// x, pend or uhold (refused), the states are ping-pong, so no byte is read and written by one launch and a row's blocks need no order.
// Compiled with -ffp-contract=off.  Plain loads and vector stores only; no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wv_floor_math.h"
#include "wv_host.h"
#include "wv_native_bank.h"
#include "wv_native_chain.h"

namespace wv {

constexpr int LF_NT = 256;             // threads of a workgroup: 16 groups of 16 lanes
constexpr int LF_MAX_NF = 16;          // frames of a tile at the most (plus the one before it)
constexpr int LF_U_FLOATS = 8192;      // u of a tile and the frame before it, in LDS, at the most
constexpr int LF_G_FLOATS = (LF_MAX_NF + 1) * 64;      // the tile's gains [frame][channel]
constexpr int LF_DESC = 21;

// The frames of one rate under the call's hop, and how a workgroup's LDS is laid out for it: the input window, then u, then the gains.
struct LfGeom {
    int64_t M;                         // nw * hop: frame f starts at ceil(f * M / orig)
    int maxlen;                        // ceil(M / orig): a frame holds this many samples or one fewer
    int win_floats;                    // native_window(orig, nw, L)
    int nf;                            // frames of a tile, 0 where the rate does not fit
};

__host__ __device__ inline LfGeom lf_geom(int orig, int nw, int L, int hop) {
    LfGeom q;
    q.M = (int64_t)nw * hop;
    const int64_t maxlen = (q.M + orig - 1) / orig;
    const long long win = native_window(orig, nw, L);
    long long room = (long long)WV_CHANNEL_FLOOR_LDS_FLOATS - LF_G_FLOATS - win;
    room = room < LF_U_FLOATS ? room : LF_U_FLOATS;
    const bool fits = maxlen <= WV_CHANNEL_FLOOR_MAX_FRAME && room >= 2 * maxlen;      // the frame before a tile, and one frame of it
    long long nf = fits ? room / maxlen - 1 : 0;
    q.maxlen = (int)(maxlen <= WV_CHANNEL_FLOOR_MAX_FRAME ? maxlen : 0);
    q.win_floats = (int)win;
    q.nf = (int)(nf < LF_MAX_NF ? nf : LF_MAX_NF);
    return q;
}

__device__ __forceinline__ int64_t lf_start(int64_t f, int64_t M, int orig) { return (f * M + orig - 1) / orig; }

__device__ __forceinline__ bool lf_cap_ok(float s) { return s >= 0.f && s <= 3.402823466e38f; }      // not negative, NaN or infinite

// One descriptor row (native_bank.native_bank_floor_up_row_ok states the same rule): wv_native_bank_up_add's fifteen fields, k now the samples that
// LEAVE, then f0, nf, uv, uv2, the gains offset (-1: none) and final.
struct LiveFloorRow {
    int64_t slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half, f0, nf, uv, uv2, g_off, fin, pv2, nu;
    bool ok;
};

__device__ __forceinline__ LiveFloorRow live_floor_row(const int64_t* __restrict__ desc, int p, const NativeRates& rates, int n_rates, int capacity, int rcap,
                                                       int pcap, int ucap, int Cmax, int64_t n_r, int64_t n_x, int64_t n_out, int64_t n_gains, int hop) {
    const int64_t* d = desc + LF_DESC * (size_t)p;
    LiveFloorRow r = {d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11], d[12], d[13], d[14], d[15], d[16], d[17], d[18], d[19], d[20],
                      0, 0, false};
    if (r.slot < 0 || r.slot >= capacity || r.rate < 0 || r.rate >= n_rates || r.C < 1 || r.C > 64 || r.C > Cmax || (r.half != 0 && r.half != 1)) return r;
    if (!native_roll_ok(rcap, r.rv, r.nr, r.rdrop, r.rv2)) return r;
    if (r.pv < 0 || r.pv > pcap || r.n < 0 || r.n > NATIVE_BANK_MAX_COUNT || r.k < 0 || r.k > r.pv + r.n) return r;
    r.pv2 = r.pv + r.n - r.k;
    if (r.pv2 > pcap || r.uv < 0 || r.uv > ucap || r.uv2 < 0 || r.uv2 > ucap || (r.fin != 0 && r.fin != 1) || (r.fin && r.uv2 != 0)) return r;
    r.nu = r.k + r.uv2 - r.uv;                                         // uv + (new u) == k + uv2
    const wv_native_rate& t = rates.r[r.rate];
    if (r.pad < 0 || r.pad > t.width || !native_count_ok(r.nu, r.rv + r.nr, r.pad, t.orig, t.nw)) return r;
    const int64_t M = (int64_t)t.nw * hop;
    if (r.f0 < 0 || r.nf < 0 || r.nf > NATIVE_BANK_MAX_COUNT || r.f0 > ((int64_t)1 << 62) / M - r.nf) return r;      // f * M stays inside int64
    const int64_t a = lf_start(r.f0, M, t.orig), whole = lf_start(r.f0 + r.nf, M, t.orig) - a;
    if (!r.fin ? r.k != whole : r.nf == 0 ? r.k != 0 : (r.k > whole || r.k <= lf_start(r.f0 + r.nf - 1, M, t.orig) - a)) return r;
    r.ok = native_range_ok(r.r_off, 1, r.nr, n_r) && native_range_ok(r.x_off, r.C, r.n, n_x) && native_range_ok(r.out_off, r.C, r.k, n_out) &&
           (r.g_off == -1 || native_range_ok(r.g_off, r.C, r.nf, n_gains));
    return r;
}

__global__ __launch_bounds__(LF_NT) void native_bank_floor_up_add_kernel(float* rhist, int rcap, float* pend, int pcap, float* uhold, int ucap, float* gprev,
                                                                         int Cmax, int capacity, const float* __restrict__ res, int64_t n_r,
                                                                         const float* __restrict__ x, int64_t n_x, NativeRates rates, int n_rates,
                                                                         const int64_t* __restrict__ desc, const float* __restrict__ cap, int hop, double rho,
                                                                         float* __restrict__ out, int64_t n_out, float* __restrict__ gains, int64_t n_gains) {
    extern __shared__ float lds[];
    __shared__ int fs[LF_MAX_NF + 2];                                   // the starts of the tile's frames in the tile's u, the last cut at k
    __shared__ int fl[LF_MAX_NF + 1];                                   // their nominal lengths
    __shared__ double sEu[LF_MAX_NF + 1];
    const LiveFloorRow r = live_floor_row(desc, blockIdx.y, rates, n_rates, capacity, rcap, pcap, ucap, Cmax, n_r, n_x, n_out, n_gains, hop);
    if (!r.ok) return;
    const float s = cap[blockIdx.y];
    if (!lf_cap_ok(s)) return;                                          // the row is skipped whole, by every workgroup
    const wv_native_rate& t = rates.r[r.rate];
    const LfGeom q = lf_geom(t.orig, t.nw, t.L, hop);
    const int tid = threadIdx.x, C = (int)r.C, k = (int)r.k, uv = (int)r.uv, uv2 = (int)r.uv2, rv2 = (int)r.rv2, pv2 = (int)r.pv2, nf = (int)r.nf, pad = (int)r.pad;
    const int64_t tiles = ((int64_t)nf + q.nf - 1) / q.nf;
    const int rblocks = native_tiles(rv2), pblocks = native_tiles(pv2), ublocks = native_tiles(uv2);
    int64_t bx = blockIdx.x;
    if (bx >= tiles + rblocks + pblocks + ublocks + (nf == 0)) return;  // the grid is as wide as the tick's longest row
    const size_t cur = (size_t)r.half, nxt = (size_t)(1 - r.half);
    float* rh = rhist + (size_t)r.slot * 2 * rcap;
    float* pd = pend + (size_t)r.slot * 2 * Cmax * pcap;
    float* uh = uhold + (size_t)r.slot * 2 * ucap;
    float* gp = gprev + (size_t)r.slot * 2 * Cmax;
    const SessionBack b{rh + cur * rcap, res + r.r_off, pd + cur * Cmax * pcap, x + r.x_off, (int)r.rv, (int)r.nr, pcap, (int)r.pv, (int)r.n};
    const float* uh_cur = uh + cur * ucap;
    const float* Kt = t.kernels_t;
    float* win = lds;

    if (bx >= tiles) {                                                  // ---- the next states
        bx -= tiles;
        if (bx < rblocks) {                                             // the next residual history
            const int j = (int)bx * NATIVE_TILE + tid;
            if (j < rv2) rh[nxt * rcap + j] = b.resid(r.rdrop + j);
            return;
        }
        bx -= rblocks;
        if (bx < pblocks) {                                             // the next delay line: the originals not yet emitted, [k, k + pv2)
            const int j = (int)bx * NATIVE_TILE + tid;
            if (j < pv2)
                for (int c = 0; c < C; ++c) pd[(nxt * Cmax + c) * pcap + j] = b.orig_ch(c, (long long)k + j);
            return;
        }
        bx -= pblocks;
        if (bx < ublocks) {                                             // the next held u: seq_u [k, k + uv2), from the old hold or formed here
            const int j0 = (int)bx * NATIVE_TILE, cnt = min(NATIVE_TILE, uv2 - j0);
            const int m_lo = max(k + j0 - uv, 0), m_hi = k + j0 + cnt - uv;      // the new u among them (none where m_hi <= m_lo)
            if (m_hi > m_lo) {
                const int n_lo = m_lo / t.nw, n_hi = (m_hi - 1) / t.nw;
                const long long p_base = (long long)n_lo * t.orig - pad;
                const int wlen = (n_hi - n_lo) * t.orig + t.L;
                for (int i = tid; i < wlen; i += LF_NT) win[i] = b.resid(p_base + i);
                __syncthreads();
                if (tid < cnt) {
                    const int m = k + j0 + tid - uv;
                    uh[nxt * ucap + j0 + tid] = m < 0 ? uh_cur[k + j0 + tid] : native_chain(Kt, win, m, n_lo, t.orig, t.nw, t.L);
                }
            } else if (tid < cnt) {
                uh[nxt * ucap + j0 + tid] = uh_cur[k + j0 + tid];
            }
            return;
        }
        if (tid < C) gp[nxt * Cmax + tid] = gp[cur * Cmax + tid];       // no frame completed: the gain before the next one is still the old one
        return;
    }

    // ---- a tile: frames i0 .. i0 + nft - 1 of the row, and (not the row's first tile) the frame before them
    float* ub = lds + q.win_floats;
    float* sG = ub + (size_t)(q.nf + 1) * q.maxlen;                     // [frame of the tile][64]
    const int grp = tid >> 4, lane = tid & 15;
    const int64_t i0 = bx * q.nf;
    const int nft = nf - i0 < q.nf ? (int)(nf - i0) : q.nf, lead = bx > 0 ? 1 : 0, nfr = nft + lead;
    const int64_t a0 = lf_start(r.f0, q.M, t.orig);
    const int base = (int)(lf_start(r.f0 + i0 - lead, q.M, t.orig) - a0);      // seq index of the tile's first sample
    if (tid <= nfr) {
        const int64_t a = lf_start(r.f0 + i0 - lead + tid, q.M, t.orig) - a0;
        fs[tid] = (int)(a < k ? a : (int64_t)k) - base;
        if (tid < nfr) fl[tid] = (int)(lf_start(r.f0 + i0 - lead + tid + 1, q.M, t.orig) - a0 - a);
    }
    __syncthreads();
    const int tile_len = fs[nfr];                                       // <= (nf + 1) * maxlen

    // u of the tile: what was held, then the chain in 256-output steps through the staged window, as the file kernel forms it
    for (int i = tid; i < tile_len; i += LF_NT)
        if (base + i < uv) ub[i] = uh_cur[base + i];
    const int m_lo = max(base - uv, 0), m_hi = base + tile_len - uv;
    for (int o = m_lo; o < m_hi; o += NATIVE_TILE) {
        const int cnt = min(NATIVE_TILE, m_hi - o);
        const int n_lo = o / t.nw, n_hi = (o + cnt - 1) / t.nw;
        const long long p_base = (long long)n_lo * t.orig - pad;
        const int wlen = (n_hi - n_lo) * t.orig + t.L;
        for (int i = tid; i < wlen; i += LF_NT) win[i] = b.resid(p_base + i);
        __syncthreads();
        if (tid < cnt) ub[o + uv - base + tid] = native_chain(Kt, win, o + tid, n_lo, t.orig, t.nw, t.L);
        __syncthreads();                                                // the window is staged again; after the last step: u is complete
    }
    __syncthreads();

    // Eu per frame: one 16-lane group a frame; the same trip count for every thread
    for (int j0 = 0; j0 < nfr; j0 += 16) {
        const int j = j0 + grp;
        const bool live = j < nfr;
        const double Eu = frame_energy(ub + (live ? fs[j] : 0), live ? fs[j + 1] - fs[j] : 0, lane);
        if (live && lane == 0) sEu[j] = Eu;
    }
    __syncthreads();

    // Ex per (frame, channel) over cat(pend, x), and the gain
    const int tasks = nfr * C;
    for (int t0 = 0; t0 < tasks; t0 += 16) {
        const int tk = t0 + grp;
        const bool live = tk < tasks;
        const int j = live ? tk / C : 0, c = live ? tk - j * C : 0;
        const long long at = (long long)base + fs[j];
        const double Ex = frame_energy_by([&](int i) { return b.orig_ch(c, at + i); }, live ? fs[j + 1] - fs[j] : 0, lane);
        if (live && lane == 0) sG[j * 64 + c] = floor_gain(Ex, sEu[j], s, rho);
    }
    __syncthreads();

    // the trace and the slot's next gain
    float* gout = r.g_off >= 0 ? gains + r.g_off : nullptr;
    for (int e = tid; e < nft * C; e += LF_NT) {
        const int j = e / C, c = e - j * C;
        const float g = sG[(j + lead) * 64 + c];
        if (gout) gout[(size_t)c * nf + (size_t)(i0 + j)] = g;
        if (i0 + j == nf - 1) gp[nxt * Cmax + c] = g;
    }

    // out
    float* ob = out + r.out_off;
    for (int j = lead; j < nfr; ++j) {
        const int len = fs[j + 1] - fs[j], Lf = fl[j];
        const bool first = r.f0 + i0 + (j - lead) == 0;                 // the stream's frame 0 ramps from its own gain
        for (int kk = tid; kk < len; kk += LF_NT) {
            const int i = base + fs[j] + kk;
            const float u = ub[fs[j] + kk];
            float ramp = -1.f;
            for (int c = 0; c < C; ++c) {
                const float G = sG[j * 64 + c];
                const float Pg = first ? G : j == 0 ? gp[cur * Cmax + c] : sG[(j - 1) * 64 + c];
                if (Pg < G && ramp < 0.f) ramp = (float)__ddiv_rn((double)(kk + 1), (double)Lf);
                ob[(size_t)c * k + i] = floor_out(b.orig_ch(c, i), floor_weight(Pg, G, ramp) * u, 1);
            }
        }
    }
}

}  // namespace wv

using wv::fail;

extern "C" int wv_native_bank_floor_up_add(float* rhist, int rcap, float* pend, int pcap, float* uhold, int ucap, float* gprev, int Cmax, int capacity,
                                           const float* r, int64_t n_r, const float* x, int64_t n_x, const wv_native_rate* rates, int n_rates,
                                           const int64_t* desc, const float* cap, int P, int blocks, int hop, double rho, float* out, int64_t n_out,
                                           float* gains, int64_t n_gains, void* stream) {
    const char* who = "wv_native_bank_floor_up_add";
    const std::string w(who);
    wv::NativeRates tab;
    size_t smem = 0;
    if (int rc = native_bank_check(who, capacity, P, blocks, rates, n_rates, &tab, &smem)) return rc;
    if (rcap < 1 || pcap < 1 || ucap < 1 || Cmax < 1 || Cmax > 64 || n_r < 0 || n_x < 0 || n_out < 0 || n_gains < 0)
        return fail(WV_EINVAL, w + ": rcap, pcap or ucap < 1, Cmax outside [1, 64], or n_r, n_x, n_out or n_gains < 0");
    if (!rhist || !pend || !uhold || !gprev || (P > 0 && (!desc || !cap)) || (n_r > 0 && !r) || (n_x > 0 && !x) || (n_out > 0 && !out) || (n_gains > 0 && !gains))
        return fail(WV_EINVAL, w + ": null rhist, pend, uhold or gprev, descriptors without desc or cap, or a positive count without its arena (r, x, out, gains)");
    if (hop < 1) return fail(WV_EINVAL, w + ": hop < 1");
    if (!(rho > 0.0) || !std::isfinite(rho)) return fail(WV_EINVAL, w + ": rho not finite or <= 0");
    smem = 0;
    for (int i = 0; i < n_rates; ++i) {
        const wv_native_rate& t = rates[i];
        if ((long long)t.nw * hop > 0x7fffffffLL) return fail(WV_EINVAL, w + ": rate " + std::to_string(i) + ": nw * hop beyond 2^31 - 1");
        const wv::LfGeom q = wv::lf_geom(t.orig, t.nw, t.L, hop);
        if (q.nf < 1)
            return fail(WV_EINVAL, w + ": rate " + std::to_string(i) + ": a frame of ceil(nw * hop / orig) native samples exceeds WV_CHANNEL_FLOOR_MAX_FRAME = " WV_STR(WV_CHANNEL_FLOOR_MAX_FRAME) ", or two of them with the input window (" + std::to_string(q.win_floats) + " floats) and the gains the LDS budget of " WV_STR(WV_CHANNEL_FLOOR_LDS_FLOATS) " floats");
        const size_t need = ((size_t)q.win_floats + (size_t)(q.nf + 1) * q.maxlen + wv::LF_G_FLOATS) * sizeof(float);
        smem = need > smem ? need : smem;
    }
    const struct { const void* p; size_t bytes; bool written; } a[] = {
        {rhist, (size_t)capacity * 2 * rcap * 4, true}, {pend, (size_t)capacity * 2 * Cmax * pcap * 4, true}, {uhold, (size_t)capacity * 2 * ucap * 4, true},
        {gprev, (size_t)capacity * 2 * Cmax * 4, true}, {out, (size_t)n_out * 4, true}, {gains, (size_t)n_gains * 4, true},
        {r, (size_t)n_r * 4, false}, {x, (size_t)n_x * 4, false}};
    for (size_t i = 0; i < sizeof(a) / sizeof(a[0]); ++i)
        for (size_t j = i + 1; j < sizeof(a) / sizeof(a[0]); ++j)
            if ((a[i].written || a[j].written) && native_overlap(a[i].p, a[i].bytes, a[j].p, a[j].bytes))
                return fail(WV_EINVAL, w + ": rhist, pend, uhold, gprev, r, x, out and gains must not overlap (r and x are only read and may)");
    if (P == 0 || blocks == 0) return WV_OK;
    hipLaunchKernelGGL(wv::native_bank_floor_up_add_kernel, dim3(blocks, P), dim3(wv::LF_NT), smem, (hipStream_t)stream, rhist, rcap, pend, pcap, uhold, ucap,
                       gprev, Cmax, capacity, r, n_r, x, n_x, tab, n_rates, desc, cap, hop, rho, out, n_out, gains, n_gains);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}
