// The per-channel SNR floor at a file's own rate (waveverify_amd/channel_floor.py is the definition): the back end of
// the native-rate route with the floor of section 7d-11 applied per ORIGINAL channel, on the native time line.
//     u[b][m]      = wv_native_upsample_add's fmaf chain over delta (native_chain, the same device function)
//     frame of m   = (m * orig) / (nw * hop)                       the 16 kHz floor's frames seen from the native time line
//     start(f)     = ceil(f * nw * hop / orig), nominal length L_f = start(f + 1) - start(f); the last frame is cut at Tn
//     Ex[c][f], Eu[f]  float64 sums of squares in THE fixed order of frame_energy, k counted inside the native frame
//     g[c][f]      = floor_gain(Ex, Eu, s[b], rho)
//     w            = floor_weight(g[c][f - 1] (f = 0: g[c][0]), g[c][f], float32((k + 1) / L_f))
//     v = w * u;   out[b][c][m] = add ? (v == 0 ? x : x + v) : v
// TWO launches and a workspace (form three of the issue's list; DESIGN section 7d-12 has the figures):
//   gains  grid (tile of NF frames, row): u of the tile's frames is formed ONCE, in 256-output steps through the staged input window, into
//          LDS and into the workspace's u [B][Tn]; Eu per frame from LDS, then Ex per (frame, channel) from x, 16 lanes a sum; g to the
//          workspace's g [B][C][F] (and to the caller's trace).  It reads x and writes neither x nor out.
//   apply  grid (tile of NF frames, row): u and the two gains back from the workspace, each out element read (x) and written by ONE thread,
//          so out may be x.
// A weight needs the gain of the frame before, hence the launch boundary: with out == x a fused kernel would read frame f - 1 of x for its
// energy while the workgroup that owns f - 1 overwrites it.
// Compiled with -ffp-contract=off.  Plain loads and vector stores only; no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wv_floor_math.h"
#include "wv_host.h"
#include "wv_native_chain.h"

namespace wv {

constexpr int CF_NT = 256;             // threads of a workgroup: 16 groups of 16 lanes
constexpr int CF_MAX_NF = 16;          // frames of a tile at the most
constexpr int CF_U_FLOATS = 8192;      // u of a tile held in LDS at the most (32 KB)

struct CfGeom {
    int orig, nw, L, width, hop;
    int nf;                            // frames of a tile
    int win_floats;                    // native_window(orig, nw, L)
    int64_t M;                         // nw * hop: frame f starts at ceil(f * M / orig)
    int64_t F;                         // frames of a row: frame(Tn - 1) + 1
};

__device__ __forceinline__ int64_t cf_start(int64_t f, const CfGeom& q) { return (f * q.M + q.orig - 1) / q.orig; }

__device__ __forceinline__ bool cf_strength_ok(float s) { return s >= 0.f && s <= 3.402823466e38f; }      // not negative, NaN or infinite

__global__ __launch_bounds__(CF_NT) void channel_floor_gains_kernel(const float* __restrict__ x, const float* __restrict__ delta,
                                                                    const float* __restrict__ Kt, const float* __restrict__ strengths,
                                                                    float* __restrict__ u_ws, float* __restrict__ g_ws, float* __restrict__ gains,
                                                                    int C, int T16, int Tn, CfGeom q, double rho) {
    extern __shared__ float lds[];
    __shared__ int fs[CF_MAX_NF + 1];                               // starts of the tile's frames, relative to the tile's first sample
    __shared__ double sEu[CF_MAX_NF];
    float* win = lds;
    float* ub = lds + q.win_floats;
    const int b = blockIdx.y, tid = threadIdx.x, grp = tid >> 4, lane = tid & 15;
    const float s = strengths[b];
    if (!cf_strength_ok(s)) return;                                 // the row is skipped whole, by every workgroup of both launches
    const int64_t f0 = (int64_t)blockIdx.x * q.nf;
    const int nf = q.F - f0 < q.nf ? (int)(q.F - f0) : q.nf;
    const int64_t ms = cf_start(f0, q);                             // < Tn: frame f0 <= F - 1 holds a sample
    if (tid <= nf) {
        const int64_t a = cf_start(f0 + tid, q);
        fs[tid] = (int)((a < Tn ? a : (int64_t)Tn) - ms);
    }
    __syncthreads();
    const int tile_len = fs[nf];                                    // <= nf * ceil(M / orig) <= CF_U_FLOATS

    // u of the tile, 256 outputs a step: the file kernel's staging and chain, from any m0
    const float* db = delta + (size_t)b * T16;
    for (int o = 0; o < tile_len; o += NATIVE_TILE) {
        const int m0 = (int)ms + o;
        const int cnt = min(NATIVE_TILE, tile_len - o);
        const int n_lo = m0 / q.nw, n_hi = (m0 + cnt - 1) / q.nw;
        const long long s_base = (long long)n_lo * q.orig - q.width;
        const int wlen = (n_hi - n_lo) * q.orig + q.L;
        for (int i = tid; i < wlen; i += CF_NT) {
            const long long sidx = s_base + i;
            win[i] = (sidx >= 0 && sidx < T16) ? db[(size_t)sidx] : 0.f;
        }
        __syncthreads();
        if (tid < cnt) {
            const float u = native_chain(Kt, win, m0 + tid, n_lo, q.orig, q.nw, q.L);
            ub[o + tid] = u;
            u_ws[(size_t)b * Tn + (size_t)(m0 + tid)] = u;
        }
        __syncthreads();                                            // the window is staged again
    }

    // Eu per frame: one 16-lane group a frame (nf <= 16 groups); the same trip count for every thread
    {
        const int len = grp < nf ? fs[grp + 1] - fs[grp] : 0;
        const double Eu = frame_energy(ub + (grp < nf ? fs[grp] : 0), len, lane);
        if (grp < nf && lane == 0) sEu[grp] = Eu;
    }
    __syncthreads();

    // Ex per (frame, channel) and the gain
    const float* xb = x + (size_t)b * C * Tn;
    const int tasks = nf * C;
    for (int t0 = 0; t0 < tasks; t0 += 16) {
        const int t = t0 + grp;
        const bool live = t < tasks;
        const int i = live ? t / C : 0, c = live ? t - i * C : 0;
        const int len = live ? fs[i + 1] - fs[i] : 0;
        const double Ex = frame_energy(xb + (size_t)c * Tn + (size_t)(ms + fs[i]), len, lane);
        if (live && lane == 0) {
            const float g = floor_gain(Ex, sEu[i], s, rho);
            const size_t at = ((size_t)b * C + c) * (size_t)q.F + (size_t)(f0 + i);
            g_ws[at] = g;
            if (gains) gains[at] = g;
        }
    }
}

// x and out may be the same buffer: element [b][c][m] is read and written by the one thread that owns m, the read first.
__global__ __launch_bounds__(CF_NT) void channel_floor_apply_kernel(const float* x, const float* __restrict__ strengths, const float* __restrict__ u_ws,
                                                                    const float* __restrict__ g_ws, float* out, int C, int Tn, CfGeom q, int add) {
    const int b = blockIdx.y, tid = threadIdx.x;
    if (!cf_strength_ok(strengths[b])) return;
    const int64_t f0 = (int64_t)blockIdx.x * q.nf;
    const int nf = q.F - f0 < q.nf ? (int)(q.F - f0) : q.nf;
    const float* ur = u_ws + (size_t)b * Tn;
    const float* gb = g_ws + (size_t)b * C * (size_t)q.F;
    const size_t row = (size_t)b * C * Tn;
    int64_t a = cf_start(f0, q);
    for (int i = 0; i < nf; ++i) {
        const int64_t f = f0 + i;
        const int64_t nxt = cf_start(f + 1, q);
        const int Lf = (int)(nxt - a);                              // the nominal length, also of a cut last frame
        const int len = (int)((nxt < Tn ? nxt : (int64_t)Tn) - a);
        const int64_t fp = f > 0 ? f - 1 : 0;
        for (int k = tid; k < len; k += CF_NT) {
            const size_t m = (size_t)(a + k);
            const float u = ur[m];
            float ramp = -1.f;
            for (int c = 0; c < C; ++c) {
                const float P = gb[(size_t)c * (size_t)q.F + (size_t)fp], G = gb[(size_t)c * (size_t)q.F + (size_t)f];
                if (P < G && ramp < 0.f) ramp = (float)__ddiv_rn((double)(k + 1), (double)Lf);
                const size_t at = row + (size_t)c * Tn + m;
                out[at] = floor_out(add ? x[at] : 0.f, floor_weight(P, G, ramp) * u, add);
            }
        }
        a = nxt;
    }
}

}  // namespace wv

using wv::fail;

// Everything both entry points refuse, and the geometry.  -> WV_OK, or the code already reported.
static int channel_floor_check(const char* who, int B, int C, int T16, int Tn, int orig, int nw, int L, int width, int hop, wv::CfGeom* q) {
    const std::string w(who);
    if (B < 1 || B > 65535) return fail(WV_EINVAL, w + ": B outside [1, 65535]");
    if (C < 1 || C > 64) return fail(WV_EINVAL, w + ": C outside [1, 64]");
    if (T16 < 1 || Tn < 1 || orig < 1 || nw < 1 || L < 1 || width < 0) return fail(WV_EINVAL, w + ": Tn, T16, orig, nw or L < 1, or width < 0");
    if ((long long)Tn > ((long long)T16 + orig - 1) / orig * nw + nw) return fail(WV_EINVAL, w + ": output longer than (ceil(T16 / orig) + 1) * nw");
    const long long win = wv::native_window(orig, nw, L);
    if (win * (long long)sizeof(float) > (long long)wv::NATIVE_LDS_BYTES) return fail(WV_EINVAL, w + ": the input window of a 256-output tile (" + std::to_string(win * 4) + " bytes) exceeds 64 KB of LDS");
    if (hop < 1) return fail(WV_EINVAL, w + ": hop < 1");
    const long long M = (long long)nw * hop;
    if (M > 0x7fffffffLL) return fail(WV_EINVAL, w + ": nw * hop beyond 2^31 - 1");
    const long long maxlen = (M + orig - 1) / orig;                 // a frame holds floor or ceil of nw * hop / orig samples
    if (maxlen > WV_CHANNEL_FLOOR_MAX_FRAME || win + maxlen > WV_CHANNEL_FLOOR_LDS_FLOATS)
        return fail(WV_EINVAL, w + ": a frame of " + std::to_string(maxlen) + " native samples exceeds WV_CHANNEL_FLOOR_MAX_FRAME = " WV_STR(WV_CHANNEL_FLOOR_MAX_FRAME) ", or with the input window (" + std::to_string(win) + " floats) the LDS budget of " WV_STR(WV_CHANNEL_FLOOR_LDS_FLOATS) " floats");
    const long long F = ((long long)(Tn - 1) * orig) / M + 1;
    if (F > 0x7fffffffLL) return fail(WV_EINVAL, w + ": more than 2^31 - 1 frames");
    long long room = WV_CHANNEL_FLOOR_LDS_FLOATS - win;
    room = room < wv::CF_U_FLOATS ? room : wv::CF_U_FLOATS;
    long long nf = room / maxlen;
    nf = nf < wv::CF_MAX_NF ? nf : wv::CF_MAX_NF;
    *q = wv::CfGeom{orig, nw, L, width, hop, (int)nf, (int)win, (int64_t)M, (int64_t)F};
    return WV_OK;
}

extern "C" int wv_native_floor_up_add_bytes(int B, int C, int T16, int Tn, int orig, int nw, int L, int width, int hop, size_t* workspace_bytes) {
    const char* who = "wv_native_floor_up_add_bytes";
    if (!workspace_bytes) return fail(WV_EINVAL, std::string(who) + ": null workspace_bytes");
    wv::CfGeom q;
    if (int rc = channel_floor_check(who, B, C, T16, Tn, orig, nw, L, width, hop, &q)) return rc;
    wv::Carver cv(nullptr);
    cv.take((size_t)B * Tn * sizeof(float));
    cv.take((size_t)B * C * (size_t)q.F * sizeof(float));
    *workspace_bytes = cv.used;
    return WV_OK;
}

extern "C" int wv_native_floor_up_add(const float* x, const float* delta, const float* kernels_t, float* out, int B, int C, int T16, int Tn, int orig, int nw,
                                      int L, int width, int hop, double rho, const float* strengths, int add, float* gains, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    const char* who = "wv_native_floor_up_add";
    if (!x || !delta || !kernels_t || !out || !strengths || !workspace)
        return fail(WV_EINVAL, std::string(who) + ": null pointer (x, delta, kernels_t, out, strengths, workspace)");
    wv::CfGeom q;
    if (int rc = channel_floor_check(who, B, C, T16, Tn, orig, nw, L, width, hop, &q)) return rc;
    if (!(rho > 0.0) || !std::isfinite(rho)) return fail(WV_EINVAL, std::string(who) + ": rho not finite or <= 0");
    if (add != 0 && add != 1) return fail(WV_EINVAL, std::string(who) + ": add not 0 / 1");
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(WV_EINVAL, std::string(who) + ": workspace not on a 256-byte boundary");
    wv::Carver cv(workspace);
    float* u_ws = cv.take((size_t)B * Tn * sizeof(float));
    float* g_ws = cv.take((size_t)B * C * (size_t)q.F * sizeof(float));
    if (cv.used > workspace_bytes) return fail(WV_EINVAL, std::string(who) + ": workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(cv.used) + " needed (wv_native_floor_up_add_bytes)");
    const int tiles = (int)((q.F + q.nf - 1) / q.nf);
    const size_t smem = ((size_t)q.win_floats + (size_t)q.nf * (size_t)((q.M + orig - 1) / orig)) * sizeof(float);
    hipLaunchKernelGGL(wv::channel_floor_gains_kernel, dim3(tiles, B), dim3(wv::CF_NT), smem, (hipStream_t)stream, x, delta, kernels_t, strengths, u_ws, g_ws,
                       gains, C, T16, Tn, q, rho);
    WV_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(wv::channel_floor_apply_kernel, dim3(tiles, B), dim3(wv::CF_NT), 0, (hipStream_t)stream, x, strengths, u_ws, g_ws, out, C, Tn, q, add);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}
