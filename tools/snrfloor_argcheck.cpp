// Host-side sanitizer pass over wv_snr_floor's argument checks (csrc/wv_snr_floor.hip): a stand-alone program, no GPU, no launch.
//
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//           waveverify_amd/csrc/wv_snr_floor.hip tools/snrfloor_argcheck.cpp -o snrfloor_argcheck && ./snrfloor_argcheck
//
// Every call below is refused with WV_EINVAL, or succeeds without a launch (A == 0, n_max == 0), so nothing here needs a device: the
// addresses are host arrays that a refusal never follows.  The program exits non-zero on the first call that returns something else, and
// the sanitizers report whatever the checks themselves do wrong (an overflow in the overlap arithmetic, a bad read of an argument).
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
    const float* x;
    int64_t n_x;
    const float* r;
    int64_t n_r;
    float* out;
    int64_t n_out;
    const int64_t* desc;
    int A;
    int64_t n_max;
    float* gstate;
    int n_state;
    float* gains;
    int64_t n_gains;
    const float* ramp;
    int L;
    double rho;
    int add;
};

static int call(const Args& a) {
    return wv_snr_floor(a.x, a.n_x, a.r, a.n_r, a.out, a.n_out, a.desc, a.A, a.n_max, a.gstate, a.n_state, a.gains, a.n_gains, a.ramp, a.L, a.rho,
                        a.add, nullptr);
}

static int failures = 0;

static void expect(const char* why, const Args& a, int want) {
    const int rc = call(a);
    const bool named = want == WV_OK || std::strncmp(wv::last_error.c_str(), "wv_snr_floor", 12) == 0;
    if (rc != want || !named) {
        std::printf("FAIL %s: returned %d, expected %d (%s)\n", why, rc, want, wv::last_error.c_str());
        ++failures;
    }
}

int main() {
    static float buf[64];
    static int64_t desc[8];
    static float state[2], gains[16], ramp[4] = {0.25f, 0.5f, 0.75f, 1.f};
    const Args ok = {buf, 16, buf + 16, 16, buf + 32, 16, desc, 1, 16, state, 2, gains, 16, ramp, 4, 0.01, 1};
    const double inf = std::numeric_limits<double>::infinity();
    Args a;
#define REFUSED(why, stmt) \
    a = ok;                \
    stmt;                  \
    expect(why, a, WV_EINVAL)
    REFUSED("null x", a.x = nullptr);
    REFUSED("null r", a.r = nullptr);
    REFUSED("null out", a.out = nullptr);
    REFUSED("null desc", a.desc = nullptr);
    REFUSED("null ramp", a.ramp = nullptr);
    REFUSED("n_x < 0", a.n_x = -1);
    REFUSED("n_r < 0", a.n_r = -1);
    REFUSED("n_out < 0", a.n_out = -1);
    REFUSED("n_state < 0", a.n_state = -1);
    REFUSED("states without gstate", a.gstate = nullptr);
    REFUSED("n_gains < 0", a.n_gains = -1);
    REFUSED("gains without their array", a.gains = nullptr);
    REFUSED("L < 1", a.L = 0);
    REFUSED("L < 0", a.L = std::numeric_limits<int>::min());
    REFUSED("L beyond the limit", a.L = WV_SNR_FLOOR_MAX_FRAME + 1);
    REFUSED("rho = 0", a.rho = 0.0);
    REFUSED("rho < 0", a.rho = -1.0);
    REFUSED("rho = nan", a.rho = std::nan(""));
    REFUSED("rho = inf", a.rho = inf);
    REFUSED("A < 0", a.A = -1);
    REFUSED("A > 65535", a.A = 65536);
    REFUSED("n_max < 0", a.n_max = -1);
    REFUSED("n_max beyond 2^31 - 1", a.n_max = (int64_t)1 << 31);
    REFUSED("n_max = int64 max", a.n_max = std::numeric_limits<int64_t>::max());
    REFUSED("add = 2", a.add = 2);
    REFUSED("add < 0", a.add = -1);
    REFUSED("out is x", a.out = buf);
    REFUSED("out is r", a.out = buf + 16);
    REFUSED("out overlaps the end of x", a.out = buf + 8);
    REFUSED("out overlaps the start of r", (a.out = buf + 8, a.n_out = 12, a.n_x = 4));
    REFUSED("x inside out", (a.out = buf, a.n_out = 64, a.x = buf + 40, a.r = buf + 20));
    REFUSED("sizes near int64 max still overlap", (a.n_x = std::numeric_limits<int64_t>::max() / 8, a.n_out = a.n_x));
#undef REFUSED
    a = ok;
    a.A = 0;
    expect("A == 0 is success without a launch", a, WV_OK);
    a = ok;
    a.n_max = 0;
    expect("n_max == 0 is success without a launch", a, WV_OK);
    a = ok;
    a.A = 0;
    a.gstate = nullptr;
    a.n_state = 0;
    a.gains = nullptr;
    a.n_gains = 0;
    expect("no states, no gains", a, WV_OK);
    for (float v : buf) failures += v != 0.f;
    std::printf("%s\n", failures ? "argument checks: FAILED" : "argument checks: ok");
    return failures ? 1 : 0;
}
