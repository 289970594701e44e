// STOI (short-time objective intelligibility, Taal et al. 2011, non-extended) of a batch of clip pairs, the way the pystoi package
// states it and the reference reports it on every validation batch (scripts/evaluate.py:65-144).  waveverify_amd/stoi.py holds the
// constants and the float64 statement of the algorithm; this file is the device route of metrics.STOI.  Four stages on one stream:
//
//   resample   wv_fx_resample (csrc/wv_fx.hip) with the host's table of Octave's `resample` filter, both signals to 10 kHz
//   keep       one workgroup per clip: energies of the Hann-windowed 256-sample frames of the CLEAN clip in f64, the clip's maximum, the
//              frames within 40 dB of it, and their indices in ascending order (ballot + popcount prefix, one wave)
//   bands      the clip with its dropped frames cut out is the overlap-add of the kept windowed frames; frame j of THAT signal is
//                  w * (F[kept[j]] + [j > 0] F[kept[j-1]][128:] onto the first half + F[kept[j+1]][:128] onto the last half),  F[i] = w * x10[128 i :]
//              so it is gathered straight into LDS, 32 frames a workgroup, and multiplied by the [512][256] DFT basis (bins 7..218,
//              re / im interleaved, the second window folded in) on v_mfma_f32_32x32x2_f32; re^2 + im^2 per bin, the bins of a band
//              added in ascending order in f64, sqrt -> tob [B][2][15][Jmax]
//   correlate  one workgroup per clip: every (segment of 30 frames, band) row in f64 -- scale, clip, remove the means, normalise,
//              dot -- a thread adds its rows in ascending order, then a fixed tree; d = sum / (segments * 15), 1e-5 under 30 frames
//
// No atomics, every order fixed, nothing of one clip depends on another: two runs are bit-equal and a clip's result is the same in any
// batch.  All loads are single floats, so inputs need 4-byte alignment only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wv_host.h"

namespace {

constexpr int ST_FRAME = 256, ST_HOP = 128, ST_BANDS = 15, ST_NSEG = 30;
constexpr int ST_ROWS = 512;                    // basis rows: 2 * 212 (re, im of bins 7..218) padded to 16 tiles of 32
constexpr int ST_BIN0 = 7, ST_NBINS = 212;
constexpr int ST_COLS = 32;                     // frames per workgroup of the band launch
constexpr int ST_LD = ST_COLS + 1;              // LDS row stride of the frame tile (odd: the column-wise build is conflict-free)
// Taal's MATLAB frames with 1:K/2:(length(x)-K): the end is EXCLUSIVE.  The same switch, under the same name, is in waveverify_amd/stoi.py.
constexpr bool ST_FRAME_END_EXCLUSIVE = true;
constexpr double ST_EPS = 2.220446049250313e-16;                 // float64 machine epsilon
constexpr double ST_DYN_RANGE = 40.0;
constexpr double ST_CLIP = 1.0 + 5.623413251903491;              // 1 + 10^(15 / 20)
constexpr double ST_SHORT = 1e-5;
constexpr int ST_MAX_B = 65535;

// first DFT bin of every third-octave band (150 Hz * 2^((2 i - 1) / 6) on the 512-point grid at 10 kHz); band i ends where i + 1 begins
__constant__ int st_band_lo[ST_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

using f32x16 = __attribute__((ext_vector_type(16))) float;

__host__ __device__ inline int st_frames(int n) {
    const int end = n - ST_FRAME + (ST_FRAME_END_EXCLUSIVE ? 0 : 1);
    return end <= 0 ? 0 : (end + ST_HOP - 1) / ST_HOP;
}

__device__ __forceinline__ double st_wave_sum(double v) {        // lane 0 gets the sum, fixed tree
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// ---- keep: energies, maximum, ordered compaction.  grid B, 256 threads.
__global__ __launch_bounds__(256) void stoi_keep_kernel(const float* __restrict__ xs, int T10, int nf, const float* __restrict__ win,
                                                        double* __restrict__ energy, int* __restrict__ kept, int* __restrict__ frames,
                                                        int* __restrict__ kept_idx) {
    __shared__ double shmax[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* xr = xs + (size_t)b * T10;
    double* e = energy + (size_t)b * nf;
    double w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = (double)win[lane + 64 * q];
    for (int i = wave; i < nf; i += 4) {                         // a wave per frame; the last sample read is 128 (nf - 1) + 255 < T10
        const float* f = xr + (size_t)ST_HOP * i;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double v = w[q] * (double)f[lane + 64 * q];
            s += v * v;
        }
        s = st_wave_sum(s);
        if (lane == 0) e[i] = 20.0 * log10(sqrt(s) + ST_EPS);
    }
    __threadfence_block();
    __syncthreads();
    double mx = -HUGE_VAL;
    for (int i = tid; i < nf; i += 256) mx = fmax(mx, e[i]);
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) shmax[wave] = mx;
    __syncthreads();
    if (wave != 0) return;
    mx = fmax(fmax(shmax[0], shmax[1]), fmax(shmax[2], shmax[3]));
    int* kp = kept + (size_t)b * nf;
    int* ko = kept_idx ? kept_idx + (size_t)b * nf : nullptr;
    int base = 0;
    for (int i0 = 0; i0 < nf; i0 += 64) {
        const int i = i0 + lane;
        const bool keep = i < nf && (mx - ST_DYN_RANGE - e[i]) < 0.0;
        const unsigned long long m = __ballot(keep);
        if (keep) {
            const int at = base + __popcll(m & ((1ull << lane) - 1ull));
            kp[at] = i;
            if (ko) ko[at] = i;
        }
        base += __popcll(m);
    }
    if (ko)
        for (int i = base + lane; i < nf; i += 64) ko[i] = -1;
    if (lane == 0) {
        frames[2 * b] = base;
        frames[2 * b + 1] = nf;
    }
}

// ---- bands: gather 32 frames, [512][256] x [256][32] on the matrix pipe, band magnitudes.  grid (ceil(Jmax / 32), 2, B), 256 threads.
__global__ __launch_bounds__(256) void stoi_bands_kernel(const float* __restrict__ xs, const float* __restrict__ ys, int T10, int nf, int Jmax,
                                                         const int* __restrict__ kept, const int* __restrict__ frames,
                                                         const float* __restrict__ basis, const float* __restrict__ win, float* __restrict__ tob) {
    __shared__ float tile[ST_FRAME * ST_LD];                     // [sample][frame], 33 KB
    __shared__ float pw[ST_NBINS * ST_COLS];                     // [bin][frame] re^2 + im^2, 26.5 KB
    const int b = blockIdx.z, sig = blockIdx.y, j0 = blockIdx.x * ST_COLS, tid = threadIdx.x;
    const int J = frames[2 * b] - 1;
    float* out = tob + ((size_t)b * 2 + sig) * ST_BANDS * Jmax;
    if (j0 >= J) {                                               // nothing of this clip here: its columns are zeros
        for (int idx = tid; idx < ST_BANDS * ST_COLS; idx += 256) {
            const int j = j0 + (idx & 31);
            if (j < Jmax) out[(size_t)(idx >> 5) * Jmax + j] = 0.f;
        }
        return;
    }
    const float* src = (sig ? ys : xs) + (size_t)b * T10;
    const int* kp = kept + (size_t)b * nf;
    {
        const int n = tid;                                       // a thread per sample of the frame, the 32 frames in turn
        const float wn = win[n], wo = win[n ^ ST_HOP];
        for (int c = 0; c < ST_COLS; ++c) {
            const int j = j0 + c;
            float v = 0.f;
            if (j < J) {                                         // kept[j + 1] exists: j + 1 <= J = kept - 1
                v = wn * src[(size_t)ST_HOP * kp[j] + n];
                if (n >= ST_HOP) v += wo * src[(size_t)ST_HOP * kp[j + 1] + n - ST_HOP];
                else if (j > 0) v += wo * src[(size_t)ST_HOP * kp[j - 1] + n + ST_HOP];
            }
            tile[n * ST_LD + c] = v;
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
    // A = basis rows (wave w takes row tiles w, w + 4, w + 8, w + 12), B = the frames; lane l feeds A[row r][k = 2 s + h], B[k][frame r]
    const float* bp = basis + (size_t)h * ST_ROWS + wave * 32 + r;
    for (int s = 0; s < ST_FRAME / 2; ++s) {
        const float bv = tile[(2 * s + h) * ST_LD + r];
        const float* a = bp + (size_t)s * 2 * ST_ROWS;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q * 128], bv, acc[q], 0, 0, 0);
    }
    // D: lane holds frame r, rows (reg & 3) + 8 (reg >> 2) + 4 h of its tile; rows 2 i, 2 i + 1 are re, im of bin i
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int bin = (wave + 4 * q) * 16 + 4 * g + 2 * h + p;
                const float re = acc[q][4 * g + 2 * p], im = acc[q][4 * g + 2 * p + 1];
                if (bin < ST_NBINS) pw[bin * ST_COLS + r] = re * re + im * im;
            }
    __syncthreads();
    for (int idx = tid; idx < ST_BANDS * ST_COLS; idx += 256) {
        const int band = idx >> 5, c = idx & 31, j = j0 + c;
        double s = 0.0;
        for (int bin = st_band_lo[band] - ST_BIN0; bin < st_band_lo[band + 1] - ST_BIN0; ++bin) s += (double)pw[bin * ST_COLS + c];
        if (j < Jmax) out[(size_t)band * Jmax + j] = j < J ? (float)sqrt(s) : 0.f;
    }
}

// ---- correlate: grid B, 256 threads.  Row r = (band, segment), segment fastest: neighbouring lanes read neighbouring frames.
__global__ __launch_bounds__(256) void stoi_corr_kernel(const float* __restrict__ tob, int Jmax, const int* __restrict__ frames,
                                                        double* __restrict__ stoi) {
    __shared__ double sh[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int J = frames[2 * b] - 1;
    if (J < ST_NSEG) {
        if (tid == 0) stoi[b] = ST_SHORT;
        return;
    }
    const int M = J - ST_NSEG + 1, rows = M * ST_BANDS;
    const float* xt = tob + (size_t)b * 2 * ST_BANDS * Jmax;
    const float* yt = xt + (size_t)ST_BANDS * Jmax;
    double acc = 0.0;
    for (int row = tid; row < rows; row += 256) {
        const int band = row / M, seg = row - band * M;
        const float* xp = xt + (size_t)band * Jmax + seg;
        const float* yp = yt + (size_t)band * Jmax + seg;
        double sxx = 0.0, syy = 0.0;
        for (int i = 0; i < ST_NSEG; ++i) {
            const double x = (double)xp[i], y = (double)yp[i];
            sxx += x * x;
            syy += y * y;
        }
        const double alpha = sqrt(sxx) / (sqrt(syy) + ST_EPS);
        double sx = 0.0, sy = 0.0;
        for (int i = 0; i < ST_NSEG; ++i) {
            const double x = (double)xp[i];
            sx += x;
            sy += fmin((double)yp[i] * alpha, x * ST_CLIP);
        }
        const double mx = sx / ST_NSEG, my = sy / ST_NSEG;
        double cxx = 0.0, cyy = 0.0, cxy = 0.0;
        for (int i = 0; i < ST_NSEG; ++i) {
            const double x = (double)xp[i];
            const double xc = x - mx, yc = fmin((double)yp[i] * alpha, x * ST_CLIP) - my;
            cxx += xc * xc;
            cyy += yc * yc;
            cxy += xc * yc;
        }
        acc += cxy / ((sqrt(cxx) + ST_EPS) * (sqrt(cyy) + ST_EPS));
    }
    acc = st_wave_sum(acc);
    if ((tid & 63) == 0) sh[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) stoi[b] = (((sh[0] + sh[1]) + sh[2]) + sh[3]) / ((double)M * ST_BANDS);
}

using wv::al256;
using wv::fail;

struct StPlan {
    bool ok = false, resample = false;
    int T10 = 0, nf = 0, Jmax = 0;
    size_t off_x10 = 0, off_energy = 0, off_kept = 0, off_tob = 0, bytes = 0;
};

StPlan st_plan(int B, int T, int up, int down, int L, int width) {
    StPlan p;
    if (B < 1 || B > ST_MAX_B || T < 1 || up < 1 || down < 1) return p;
    p.resample = up != down;
    if (p.resample && (L < 1 || width < 0)) return p;
    const long long t10 = p.resample ? ((long long)T * up + down - 1) / down : T;
    if (t10 > 0x7fffffffLL - ST_FRAME) return p;
    p.T10 = (int)t10;
    p.nf = st_frames(p.T10);
    p.Jmax = p.nf > 1 ? p.nf - 1 : 0;
    size_t o = 0;
    p.off_x10 = o;
    if (p.resample) o += al256((size_t)2 * B * p.T10 * sizeof(float));
    p.off_energy = o;
    o += al256((size_t)B * p.nf * sizeof(double));
    p.off_kept = o;
    o += al256((size_t)B * p.nf * sizeof(int));
    p.off_tob = o;
    o += al256((size_t)B * 2 * ST_BANDS * p.Jmax * sizeof(float));
    p.bytes = o ? o : 256;
    p.ok = true;
    return p;
}

}  // namespace

extern "C" {

size_t wv_metrics_stoi_workspace_bytes(int B, int T, int up, int down, int L, int width) {
    const StPlan p = st_plan(B, T, up, down, L, width);
    return p.ok ? p.bytes : 0;
}

int wv_metrics_stoi(const float* reference, const float* estimate, int B, int T, const float* kernels, int up, int down, int L, int width,
                    const float* basis, double* stoi, int* frames, int* kept_idx, float* tob, void* ws, size_t ws_bytes, void* stream) {
    const StPlan p = st_plan(B, T, up, down, L, width);
    if (!reference || !estimate || !basis || !stoi || !frames || !p.ok) return fail(WV_EINVAL, "null pointer (reference, estimate, basis, stoi, frames), T, up, down < 1, L < 1 or width < 0 with up != down, or B outside [1, " + std::to_string(ST_MAX_B) + "]");
    if ((kernels != nullptr) != p.resample) return fail(WV_EINVAL, "kernels must be given exactly when up != down (NULL = the clips are at 10 kHz already)");
    if ((uintptr_t)stoi & 7u) return fail(WV_EINVAL, "stoi not 8-byte aligned");
    if (!ws || ((uintptr_t)ws & 7u) || ws_bytes < p.bytes) return fail(WV_ENOMEM, "workspace missing, not 8-byte aligned, or too small");
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    const float *xs = reference, *ys = estimate;
    if (p.resample) {
        float* x10 = (float*)(w + p.off_x10);
        float* y10 = x10 + (size_t)B * p.T10;
        int rc = wv_fx_resample(reference, kernels, x10, B, T, down, up, L, width, p.T10, stream);
        if (rc != WV_OK) return rc;
        rc = wv_fx_resample(estimate, kernels, y10, B, T, down, up, L, width, p.T10, stream);
        if (rc != WV_OK) return rc;
        xs = x10;
        ys = y10;
    }
    const float* win = basis + (size_t)ST_FRAME * ST_ROWS;
    int* kept = (int*)(w + p.off_kept);
    float* tb = tob ? tob : (float*)(w + p.off_tob);
    hipLaunchKernelGGL(stoi_keep_kernel, dim3(B), dim3(256), 0, st, xs, p.T10, p.nf, win, (double*)(w + p.off_energy), kept, frames, kept_idx);
    if (p.Jmax > 0)
        hipLaunchKernelGGL(stoi_bands_kernel, dim3((p.Jmax + ST_COLS - 1) / ST_COLS, 2, B), dim3(256), 0, st, xs, ys, p.T10, p.nf, p.Jmax, kept, frames,
                           basis, win, tb);
    hipLaunchKernelGGL(stoi_corr_kernel, dim3(B), dim3(256), 0, st, tb, p.Jmax, frames, stoi);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}

}  // extern "C"
