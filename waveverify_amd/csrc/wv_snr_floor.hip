// The SNR floor of embedding: the residual r the generator made for the 16 kHz input x is scaled frame by frame so
// that in no frame of L samples it is louder than min_snr_db below x, and silence stays silent.  Per row, frames counted from its sample 0,
// frame f = [fL, min((f+1)L, n)):
//     Ex = sum x^2, Er = sum r^2                 float64; the f32 x f32 products are exact there
//     g[f] = s                                   where Er == 0
//          = q < (double)s ? (float)q : s        q = sqrt((rho * Ex) / Er), correctly rounded divide and square root
//     w[k] = g_prev < g[f] ? min(g[f], g_prev + (g[f] - g_prev) * ramp[k]) : g[f]        f32, every rounding kept; g_prev = g[f-1], for
//                                                                                        frame 0 the stored state or, without one, g[0]
//     v = w * r;   out = v   or, with add,   out = (v == 0 ? x : x + v)                  +-0 keeps x's own bits, -0.0 included
// THE SUMMATION ORDER (snr_floor.frame_energy restates it).  A frame's samples k = 0 .. len-1 go to 16 partial sums, sample k to partial
// (k >> 2) & 15; each partial adds its squares in ascending k from +0.0; the 16 partials are then folded p[j] += p[j ^ 8], ^ 4, ^ 2, ^ 1.
// Nothing in it depends on the tile size, the launch geometry or the row's place in the call: 16 lanes own one frame, lane j owns partial j
// and reads samples 4j .. 4j+3 of every 64 (a 16-byte move where the address allows), and the fold is four lane exchanges.
// One launch per call, grid (tile of SF_TF frames, row).  g[f] has no recursion, so a tile needs of its predecessor only the energies of
// the one frame before it, which it recomputes; the tile 0 of a row also computes the row's LAST frame's gain, because the block that
// reads the row's state must be the one that writes it.  x and r are read once plus two frames per tile at the most, out is written once.
// Because of the re-read out may overlap neither x nor r.  No atomics.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wv_floor_math.h"
#include "wv_host.h"

namespace wv {

constexpr int SF_NT = 256;             // threads of a workgroup: 16 groups of 16 lanes
constexpr int SF_TF = 32;              // frames of a tile
constexpr int SF_SLOTS = SF_TF + 2;    // gains a tile holds: frame f0 - 1, its own SF_TF, the row's last frame (tile 0 only)
constexpr int SF_DESC = 8;             // int64 per descriptor row

// One descriptor row = {offset of the row in x, in r, in out, n, the strength's f32 bits, state index or -1, fresh flag, offset in gains or
// -1}; a row that breaks the contract is skipped whole (snr_floor.row_ok restates the predicate).
struct FloorRow {
    int64_t xo, ro, oo, n, si, fresh, go;
    float s;
    bool ok;
};

__device__ __forceinline__ FloorRow floor_row(const int64_t* __restrict__ desc, int r, int64_t n_x, int64_t n_r, int64_t n_out, int64_t n_max,
                                              int n_state, int64_t n_gains, int L) {
    const int64_t* d = desc + SF_DESC * (size_t)r;
    FloorRow w = {d[0], d[1], d[2], d[3], d[5], d[6], d[7], 0.f, false};
    const int64_t sb = d[4];
    if (sb < 0 || sb > 0xffffffffLL || w.n < 0 || w.n > n_max) return w;
    w.s = __uint_as_float((unsigned)sb);
    if (!(w.s >= 0.f) || !(w.s <= 3.402823466e38f)) return w;                       // negative, NaN or infinite
    if (w.xo < 0 || w.xo > n_x - w.n || w.ro < 0 || w.ro > n_r - w.n || w.oo < 0 || w.oo > n_out - w.n) return w;
    if (w.si < -1 || w.si >= n_state) return w;
    const int64_t F = (w.n + L - 1) / L;
    if (w.go < -1 || (w.go >= 0 && w.go > n_gains - F)) return w;
    w.ok = true;
    return w;
}

// frame_energy (the 16 lanes of a group, the order above), floor_gain, floor_weight and floor_out: wv_floor_math.h, shared with the
// per-channel floor (csrc/wv_channel_floor.hip).

// out, x and r carry no __restrict__ towards each other beyond what the entry point has checked (no overlap).
__global__ __launch_bounds__(SF_NT) void snr_floor_kernel(const float* __restrict__ x, int64_t n_x, const float* __restrict__ r, int64_t n_r,
                                                          float* __restrict__ out, int64_t n_out, const int64_t* __restrict__ desc, int64_t n_max,
                                                          float* gstate, int n_state, float* __restrict__ gains, int64_t n_gains,
                                                          const float* __restrict__ ramp, int L, double rho, int add) {
    __shared__ float sg[SF_SLOTS];
    const FloorRow w = floor_row(desc, blockIdx.y, n_x, n_r, n_out, n_max, n_state, n_gains, L);
    if (!w.ok) return;
    const int64_t F = (w.n + L - 1) / L;
    const int64_t f0 = (int64_t)blockIdx.x * SF_TF;
    if (f0 >= F) return;                                            // also every tile of a row with n == 0
    const int nf = F - f0 < SF_TF ? (int)(F - f0) : SF_TF;
    const float* xr = x + w.xo;
    const float* rr = r + w.ro;
    float* outr = out + w.oo;
    const int tid = threadIdx.x, grp = tid >> 4, lane = tid & 15;
    const bool first = blockIdx.x == 0;
    const bool stored = first && w.si >= 0 && !w.fresh;
    float g_in = 0.f;
    if (tid == 0 && stored) g_in = gstate[w.si];                    // a fresh or absent state is never read

    // gains: slot 0 = frame f0 - 1, slots 1 .. nf = the tile's frames, slot SF_TF + 1 = the row's last frame where tile 0 does not hold it
    for (int it = 0; it < (SF_SLOTS + 15) / 16; ++it) {             // the same trip count for every thread: the fold exchanges lanes
        const int slot = it * 16 + grp;
        int64_t f = -1;
        if (slot == 0) f = f0 - 1;                                  // -1 for tile 0
        else if (slot <= nf) f = f0 + slot - 1;
        else if (slot == SF_TF + 1 && first && F > SF_TF) f = F - 1;
        const int64_t at = f * L;
        const int len = f < 0 ? 0 : (w.n - at < L ? (int)(w.n - at) : L);
        const double Ex = frame_energy(xr + (f < 0 ? 0 : at), len, lane);
        const double Er = frame_energy(rr + (f < 0 ? 0 : at), len, lane);
        if (f >= 0 && lane == 0) {
            const float g = floor_gain(Ex, Er, w.s, rho);
            sg[slot] = g;
            if (slot >= 1 && slot <= nf && w.go >= 0) gains[w.go + f] = g;
        }
    }
    __syncthreads();
    if (tid == 0 && first) {
        sg[0] = stored ? g_in : sg[1];
        if (w.si >= 0) gstate[w.si] = F > SF_TF ? sg[SF_TF + 1] : sg[(int)F];
    }
    __syncthreads();

    const int64_t base = f0 * L;
    const int64_t rest = w.n - base;
    const int tile_len = rest < (int64_t)nf * L ? (int)rest : nf * L;          // L <= WV_SNR_FLOOR_MAX_FRAME: nf * L stays an int
    const bool vec = ((reinterpret_cast<uintptr_t>(xr + base) | reinterpret_cast<uintptr_t>(rr + base) | reinterpret_cast<uintptr_t>(outr + base)) & 15) == 0;
    const float* xt = xr + base;
    const float* rt = rr + base;
    float* ot = outr + base;
    for (int i = tid * 4; i < tile_len; i += SF_NT * 4) {
        int fr = i / L, k = i - fr * L;
        if (vec && i + 4 <= tile_len) {
            const float4 xv = *reinterpret_cast<const float4*>(xt + i);
            const float4 rv = *reinterpret_cast<const float4*>(rt + i);
            const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, rs[4] = {rv.x, rv.y, rv.z, rv.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = floor_out(xs[e], floor_weight(sg[fr], sg[fr + 1], ramp[k]) * rs[e], add);
                if (++k == L) {
                    k = 0;
                    ++fr;
                }
            }
            *reinterpret_cast<float4*>(ot + i) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            for (int e = 0; e < 4 && i + e < tile_len; ++e) {
                ot[i + e] = floor_out(xt[i + e], floor_weight(sg[fr], sg[fr + 1], ramp[k]) * rt[i + e], add);
                if (++k == L) {
                    k = 0;
                    ++fr;
                }
            }
        }
    }
}

}  // namespace wv

using wv::fail;

static bool overlap(const void* a, int64_t a_n, const void* b, int64_t b_n) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    const size_t pa = (size_t)a_n * 4, qb = (size_t)b_n * 4;
    return pa && qb && p < q + qb && q < p + pa;
}

extern "C" int wv_snr_floor(const float* x, int64_t n_x, const float* r, int64_t n_r, float* out, int64_t n_out, const int64_t* desc, int A,
                            int64_t n_max, float* gstate, int n_state, float* gains, int64_t n_gains, const float* ramp, int L, double rho,
                            int add, void* stream) {
    if (!x || !r || !out || !desc || !ramp) return fail(WV_EINVAL, "wv_snr_floor: null x, r, out, desc or ramp");
    if (n_x < 0 || n_r < 0 || n_out < 0 || n_state < 0 || n_gains < 0 || (n_state > 0 && !gstate) || (n_gains > 0 && !gains))
        return fail(WV_EINVAL, "wv_snr_floor: n_x, n_r, n_out, n_state or n_gains < 0, or states without gstate, or gains without their array");
    if (L < 1 || L > WV_SNR_FLOOR_MAX_FRAME || !(rho > 0.0) || !std::isfinite(rho) || A < 0 || A > 65535 || n_max < 0 || n_max > 0x7fffffffLL || (add != 0 && add != 1))
        return fail(WV_EINVAL, "wv_snr_floor: L outside [1, " WV_STR(WV_SNR_FLOOR_MAX_FRAME) "], rho not finite or <= 0, A outside [0, 65535], n_max outside [0, 2^31 - 1] or add not 0 / 1");
    if (overlap(out, n_out, x, n_x) || overlap(out, n_out, r, n_r)) return fail(WV_EINVAL, "wv_snr_floor: out must overlap neither x nor r");
    if (A == 0 || n_max == 0) return WV_OK;
    const int64_t frames = (n_max + L - 1) / L;
    const int tiles = (int)((frames + wv::SF_TF - 1) / wv::SF_TF);
    hipLaunchKernelGGL(wv::snr_floor_kernel, dim3(tiles, A), dim3(wv::SF_NT), 0, (hipStream_t)stream, x, n_x, r, n_r, out, n_out, desc, n_max, gstate,
                       n_state, gains, n_gains, ramp, L, rho, add);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}
