// Host-side sanitizer pass over wv_native_bank_floor_up_add's argument checks (csrc/wv_live_floor.hip): a stand-alone program, no GPU, no launch.
//
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           waveverify_amd/csrc/wv_live_floor.hip tools/livefloor_argcheck.cpp -o livefloor_argcheck && ./livefloor_argcheck
//
// Every call below is refused with WV_EINVAL, or succeeds without a launch (P == 0, blocks == 0), so nothing here needs a device: the addresses
// are host arrays that a refusal never follows.  The program exits non-zero on the first call that returns something else, and the sanitizers
// report whatever the checks themselves do wrong (an overflow in the overlap or LDS arithmetic, a bad read of the rate table).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../include/waveverify_hip.h"

namespace wv {
static thread_local std::string last_error;
int fail(int code, std::string msg) {            // wv_model.hip's, restated: the one error channel
    last_error = std::move(msg);
    return code;
}
}  // namespace wv

struct Args {
    float* rhist;
    int rcap;
    float* pend;
    int pcap;
    float* uhold;
    int ucap;
    float* gprev;
    int Cmax, capacity;
    const float* r;
    int64_t n_r;
    const float* x;
    int64_t n_x;
    const wv_native_rate* rates;
    int n_rates;
    const int64_t* desc;
    const float* cap;
    int P, blocks, hop;
    double rho;
    float* out;
    int64_t n_out;
    float* gains;
    int64_t n_gains;
};

static int call(const Args& a) {
    return wv_native_bank_floor_up_add(a.rhist, a.rcap, a.pend, a.pcap, a.uhold, a.ucap, a.gprev, a.Cmax, a.capacity, a.r, a.n_r, a.x, a.n_x, a.rates,
                                       a.n_rates, a.desc, a.cap, a.P, a.blocks, a.hop, a.rho, a.out, a.n_out, a.gains, a.n_gains, nullptr);
}

static int failures = 0;
static const char* const WHO = "wv_native_bank_floor_up_add";

static void expect(const char* why, const Args& a, int want) {
    const int rc = call(a);
    const bool named = want == WV_OK || std::strncmp(wv::last_error.c_str(), WHO, std::strlen(WHO)) == 0;
    if (rc != want || !named) {
        std::printf("FAIL %s: returned %d, expected %d (%s)\n", why, rc, want, wv::last_error.c_str());
        ++failures;
    }
}

int main() {
    // capacity 2: rhist [2][2][8], pend [2][2][2][8], uhold [2][2][4], gprev [2][2][2]; arenas r 16, x 16, out 16, gains 8
    static float rhist[32], pend[64], uhold[16], gprev[8], r[16], x[16], out[16], gains[8], table[64], cap[2];
    static int64_t desc[2 * 21];
    static wv_native_rate rates[2] = {{table, 1, 3, 7, 3}, {table, 2, 1, 8, 3}};
    const Args ok = {rhist, 8, pend, 8, uhold, 4, gprev, 2, 2, r, 16, x, 16, rates, 2, desc, cap, 2, 4, 16, 0.01, out, 16, gains, 8};
    const double inf = std::numeric_limits<double>::infinity();
    static wv_native_rate broken[2];
    Args a;
#define REFUSED(why, stmt) \
    a = ok;                \
    stmt;                  \
    expect(why, a, WV_EINVAL)
#define BROKEN(why, stmt)                        \
    std::memcpy(broken, rates, sizeof(rates));   \
    stmt;                                        \
    a = ok;                                      \
    a.rates = broken;                            \
    expect(why, a, WV_EINVAL)
    REFUSED("null rhist", a.rhist = nullptr);
    REFUSED("null pend", a.pend = nullptr);
    REFUSED("null uhold", a.uhold = nullptr);
    REFUSED("null gprev", a.gprev = nullptr);
    REFUSED("null r with n_r > 0", a.r = nullptr);
    REFUSED("null x with n_x > 0", a.x = nullptr);
    REFUSED("null out with n_out > 0", a.out = nullptr);
    REFUSED("null gains with n_gains > 0", a.gains = nullptr);
    REFUSED("null desc with P > 0", a.desc = nullptr);
    REFUSED("null cap with P > 0", a.cap = nullptr);
    REFUSED("null rates", a.rates = nullptr);
    REFUSED("rcap < 1", a.rcap = 0);
    REFUSED("pcap < 1", a.pcap = 0);
    REFUSED("ucap < 1", a.ucap = 0);
    REFUSED("ucap < 0", a.ucap = std::numeric_limits<int>::min());
    REFUSED("Cmax < 1", a.Cmax = 0);
    REFUSED("Cmax > 64", a.Cmax = 65);
    REFUSED("capacity < 1", a.capacity = 0);
    REFUSED("capacity past the limit", a.capacity = WV_BANK_MAX_SLOTS + 1);
    REFUSED("n_r < 0", a.n_r = -1);
    REFUSED("n_x < 0", a.n_x = -1);
    REFUSED("n_out < 0", a.n_out = -1);
    REFUSED("n_gains < 0", a.n_gains = -1);
    REFUSED("n_rates < 1", a.n_rates = 0);
    REFUSED("n_rates past the limit", a.n_rates = WV_NATIVE_BANK_MAX_RATES + 1);
    REFUSED("P < 0", a.P = -1);
    REFUSED("P > 65535", a.P = 65536);
    REFUSED("blocks < 0", a.blocks = -1);
    REFUSED("blocks past the limit", a.blocks = WV_NATIVE_BANK_MAX_BLOCKS + 1);
    REFUSED("hop < 1", a.hop = 0);
    REFUSED("hop < 0", a.hop = std::numeric_limits<int>::min());
    REFUSED("nw * hop beyond 2^31 - 1", a.hop = std::numeric_limits<int>::max());
    REFUSED("a frame beyond WV_CHANNEL_FLOOR_MAX_FRAME", a.hop = WV_CHANNEL_FLOOR_MAX_FRAME * 2 + 2);      // rate 1: ceil(hop / 2) = 4097
    REFUSED("rho = 0", a.rho = 0.0);
    REFUSED("rho < 0", a.rho = -1.0);
    REFUSED("rho = nan", a.rho = std::nan(""));
    REFUSED("rho = inf", a.rho = inf);
    BROKEN("null table", broken[1].kernels_t = nullptr);
    BROKEN("orig < 1", broken[1].orig = 0);
    BROKEN("nw < 1", broken[0].nw = 0);
    BROKEN("L < 1", broken[1].L = 0);
    BROKEN("width < 0", broken[0].width = -1);
    BROKEN("an input window past 64 KB of LDS", (broken[1].orig = 64, broken[1].L = 2 * 8200 + 64, broken[1].width = 8200));
    BROKEN("two frames that fit alone but not beside the input window", (broken[0].orig = 16, broken[0].nw = 2040, broken[0].L = 11000));      // 2 * 2040 + 11016 + 1088
    REFUSED("out is x", a.out = x);
    REFUSED("out is r", a.out = r);
    REFUSED("out overlaps pend", a.out = pend + 60);
    REFUSED("out overlaps rhist", a.out = rhist + 20);
    REFUSED("out overlaps uhold", a.out = uhold + 8);
    REFUSED("out overlaps gprev", a.out = gprev + 4);
    REFUSED("gains is out", a.gains = out);
    REFUSED("gains overlaps the end of x", a.gains = const_cast<float*>(x) + 12);
    REFUSED("gains overlaps gprev", a.gains = gprev);
    REFUSED("x overlaps pend", a.x = pend);
    REFUSED("r overlaps rhist", a.r = rhist + 30);
    REFUSED("r overlaps uhold", a.r = uhold);
    REFUSED("uhold is rhist", a.uhold = rhist);
    REFUSED("gprev inside pend", a.gprev = pend + 10);
    REFUSED("pend overlaps rhist", a.pend = rhist);
    REFUSED("sizes near int64 max still overlap", (a.n_x = std::numeric_limits<int64_t>::max() / 8, a.n_out = a.n_x));
#undef REFUSED
#undef BROKEN
    a = ok;
    a.r = x;                                     // r and x are only read and may overlap
    a.P = 0;
    expect("r == x, P == 0", a, WV_OK);
    a = ok;
    a.P = 0;
    a.desc = nullptr;
    a.cap = nullptr;
    expect("P == 0 is success without a launch", a, WV_OK);
    a = ok;
    a.blocks = 0;
    expect("blocks == 0 is success without a launch", a, WV_OK);
    a = ok;
    a.P = 0;
    a.r = a.x = nullptr;
    a.out = a.gains = nullptr;
    a.n_r = a.n_x = a.n_out = a.n_gains = 0;
    expect("no arenas", a, WV_OK);
    for (float v : out) failures += v != 0.f;
    for (float v : gains) failures += v != 0.f;
    for (float v : rhist) failures += v != 0.f;
    for (float v : pend) failures += v != 0.f;
    for (float v : uhold) failures += v != 0.f;
    for (float v : gprev) failures += v != 0.f;
    std::printf("%s\n", failures ? "argument checks: FAILED" : "argument checks: ok");
    return failures ? 1 : 0;
}
