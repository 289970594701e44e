// What the native-rate bank kernels share (DESIGN sections 7d-8 and 7d-13; csrc/wv_native.hip, csrc/wv_live_floor.hip): the back stage's operands of
// one stream, the rate table as a kernel argument, the clauses of the row rule and the back stage's row, and the refusals every bank entry point makes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "wv_host.h"
#include "wv_native_chain.h"

namespace wv {

// The back stage's operands for ONE stream: the residual sequence cat(rh[0 .. rv), rs[0 .. nr)) and the originals cat(pend[c][0 .. pv), x[c][0 .. n)),
// channel c of the delay line pcap floats after channel c - 1, channel c of the new samples n floats after it.
struct SessionBack {
    const float* rh;
    const float* rs;
    const float* pend;
    const float* x;
    int rv, nr, pcap, pv, n;
    __device__ float resid(long long p) const { return (p < 0 || p >= (long long)rv + nr) ? 0.f : p < rv ? rh[(size_t)p] : rs[(size_t)(p - rv)]; }
    __device__ float orig_ch(int c, long long i) const {
        return i < pv ? pend[(size_t)c * pcap + (size_t)i] : x[(size_t)c * (size_t)n + (size_t)(i - pv)];
    }
};

struct NativeRates {
    wv_native_rate r[WV_NATIVE_BANK_MAX_RATES];
};

constexpr int64_t NATIVE_BANK_MAX_COUNT = 2147483647 - NATIVE_TILE;    // per-row sample counts stay ints, tile arithmetic included

__device__ __forceinline__ int native_tiles(int v) { return v / NATIVE_TILE + (v % NATIVE_TILE != 0); }

// 0 <= valid <= cap, and the next state a suffix of the sequence that fits: session_roll_ok on a descriptor's 64-bit fields.
__device__ __forceinline__ bool native_roll_ok(int64_t cap, int64_t valid, int64_t fresh, int64_t drop, int64_t next) {
    return valid >= 0 && valid <= cap && fresh >= 0 && fresh <= NATIVE_BANK_MAX_COUNT && drop >= 0 && next >= 0 && next <= cap && drop <= valid + fresh &&
           drop + next == valid + fresh;
}

// off >= 0 and off + rows * len <= total, with rows <= 64 and len <= NATIVE_BANK_MAX_COUNT (no overflow)
__device__ __forceinline__ bool native_range_ok(int64_t off, int64_t rows, int64_t len, int64_t total) {
    return off >= 0 && off <= total && rows * len <= total - off;
}

// native_session_check's output count bound: no more than (ceil((pad + sequence) / orig) + 1) * nw
__device__ __forceinline__ bool native_count_ok(int64_t cnt, int64_t seq, int64_t pad, int orig, int nw) {
    return cnt >= 0 && cnt <= NATIVE_BANK_MAX_COUNT && cnt <= ((seq + pad + orig - 1) / orig + 1) * (int64_t)nw;
}

// One descriptor row of wv_native_bank_up_add (native_bank.native_bank_up_row_ok states the same rule).
struct NativeUpRow {
    int64_t slot, rate, C, rv, r_off, nr, x_off, n, out_off, k, pad, rdrop, rv2, pv, half, pv2;
    bool ok;
};

__device__ __forceinline__ NativeUpRow native_bank_up_row(const int64_t* __restrict__ desc, int p, const NativeRates& rates, int n_rates, int capacity, int rcap,
                                                          int pcap, int Cmax, int64_t n_r, int64_t n_x, int64_t n_out) {
    const int64_t* d = desc + 15 * (size_t)p;
    NativeUpRow r = {d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11], d[12], d[13], d[14], 0, false};
    if (r.slot < 0 || r.slot >= capacity || r.rate < 0 || r.rate >= n_rates || r.C < 1 || r.C > 64 || r.C > Cmax || (r.half != 0 && r.half != 1)) return r;
    if (!native_roll_ok(rcap, r.rv, r.nr, r.rdrop, r.rv2)) return r;
    if (r.pv < 0 || r.pv > pcap || r.n < 0 || r.n > NATIVE_BANK_MAX_COUNT || r.k < 0 || r.k > r.pv + r.n) return r;
    r.pv2 = r.pv + r.n - r.k;
    const wv_native_rate& t = rates.r[r.rate];
    r.ok = r.pv2 <= pcap && r.pad >= 0 && r.pad <= t.width && native_count_ok(r.k, r.rv + r.nr, r.pad, t.orig, t.nw) &&
           native_range_ok(r.r_off, 1, r.nr, n_r) && native_range_ok(r.x_off, r.C, r.n, n_x) && native_range_ok(r.out_off, r.C, r.k, n_out);
    return r;
}

}  // namespace wv

static inline bool native_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && p < q + b_bytes && q < p + a_bytes;
}

// The refusals the bank calls share: the counts, and the rate table, which is copied into `out`.  -> WV_OK, or the code already reported.
static inline int native_bank_check(const char* who, int capacity, int P, int blocks, const wv_native_rate* rates, int n_rates, wv::NativeRates* out,
                                    size_t* smem) {
    using wv::fail;
    const std::string w(who);
    if (capacity < 1 || capacity > WV_BANK_MAX_SLOTS) return fail(WV_EINVAL, w + ": capacity outside [1, " WV_STR(WV_BANK_MAX_SLOTS) "]");
    if (P < 0 || P > 65535) return fail(WV_EINVAL, w + ": P outside [0, 65535]");
    if (blocks < 0 || blocks > WV_NATIVE_BANK_MAX_BLOCKS) return fail(WV_EINVAL, w + ": blocks outside [0, " WV_STR(WV_NATIVE_BANK_MAX_BLOCKS) "]");
    if (!rates || n_rates < 1 || n_rates > WV_NATIVE_BANK_MAX_RATES) return fail(WV_EINVAL, w + ": null rates, or n_rates outside [1, " WV_STR(WV_NATIVE_BANK_MAX_RATES) "]");
    long long bytes = 0;
    *out = wv::NativeRates{};
    for (int i = 0; i < n_rates; ++i) {
        const wv_native_rate& t = rates[i];
        if (!t.kernels_t || t.orig < 1 || t.nw < 1 || t.L < 1 || t.width < 0) return fail(WV_EINVAL, w + ": rate " + std::to_string(i) + ": null table, orig, nw or L < 1, or width < 0");
        const long long b = wv::native_window(t.orig, t.nw, t.L) * (long long)sizeof(float);
        if (b > (long long)wv::NATIVE_LDS_BYTES) return fail(WV_EINVAL, w + ": rate " + std::to_string(i) + ": the input window of a 256-output tile (" + std::to_string(b) + " bytes) exceeds 64 KB of LDS");
        bytes = b > bytes ? b : bytes;
        out->r[i] = t;
    }
    *smem = (size_t)bytes;
    return WV_OK;
}
