// Multi-scale STFT and mel-spectrogram reconstruction losses (scripts/loss.py:449-731 of the reference) with their gradient towards
// the watermarked audio.  Semantics and the primitive choices are written down in waveverify_amd/spectral_loss.py; this unit runs them.
//
// Per scale (window w, hop w/4, F = w/2 + 1, Tf = T/hop + 1 frames per clip, ncols = B*Tf rounded up to 4 frame columns):
//   frames    Fr[sig][k][col] = s[reflect(t*hop + k - w/2)]   sig 0 = wm, sig 1 = x (one launch, both signals)
//   GEMM      C[sig][2F][ncols] = Basis[2F][w] @ Fr[sig]       rows f < F: cos_f * hann, rows F + f: -sin_f * hann (f32 matrix pipe,
//                                                              the generic 1x1 core; wm and x in one launch over the same basis)
//   mel       one thread per (mel band, frame): both signals' band energies from |X| over the band's non-zero bins, the clamp / log10 /
//             L1 terms, per-workgroup partial sums; dL/dmel of wm when a gradient is wanted
//   bins      one thread per (bin, frame): |X| of both signals, the STFT loss's terms; dL/d|X| = the STFT part + the mel filters^T of
//             dL/dmel; dC = dL/d|X| * X / |X| (0 where |X| = 0) written as G[2F][ncols]
//   GEMM      Q[w][ncols] = Basis^T @ G                        (into the frames buffer, free by then)
//   OLA       dwm[b][s] += sum over frames of Q at every padded position that reads sample s (the reflect padding's adjoint folds the
//             mirrored samples back), in a fixed order
// and one reduction launch at the end sums every scale's partials in double, in a fixed order: the loss is deterministic (no atomics).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "wv_host.h"
#include "wv_kernels.h"

namespace {

constexpr int SL_NT = 256;
constexpr int SL_MAX_SCALES = 16;
constexpr float SL_LN10 = 2.302585092994046f;

__device__ __forceinline__ int sl_reflect(int i, int T) {        // torch's reflect padding (pad < T)
    if (i < 0) i = -i;
    if (i >= T) i = 2 * (T - 1) - i;
    return i;
}

// fixed-order tree sum of one value per thread over the workgroup; thread 0 gets the total
__device__ __forceinline__ float sl_block_sum(float v, float* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = SL_NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float sl_sign(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(SL_NT) void specloss_frames_kernel(const float* __restrict__ wm, const float* __restrict__ x, float* __restrict__ Fr,
                                                                int B, int T, int Tf, int ncols, int w, int hop) {
    const int col = blockIdx.x * SL_NT + threadIdx.x, k = blockIdx.y, sig = blockIdx.z;
    if (col >= ncols) return;
    float v = 0.f;                                                // padding columns: zero frames (zero spectra, no loss, no gradient)
    if (col < B * Tf) {
        const int b = col / Tf, t = col - b * Tf;
        v = (sig ? x : wm)[(size_t)b * T + sl_reflect(t * hop + k - w / 2, T)];
    }
    Fr[((size_t)sig * w + k) * ncols + col] = v;
}

struct SlMel {                 // band m covers bins [lo[m], hi[m]) with weights wt[off[m] + f - lo[m]]; bin f lies in bands [mlo[f], mhi[f])
    const int *lo, *hi, *off, *mlo, *mhi;
    const float* wt;
    int n_mels;
};

struct SlTerm {                // one loss term: log_w * mean|pow*log10(clamp(a)) - pow*log10(clamp(b))| + mag_w * mean|a - b|
    float pow, eps;
    float g_log, g_mag;        // grad_scale * weight / element count: the gradient factors of the two parts
};

__device__ __forceinline__ float sl_term(float a, float b, const SlTerm& q, float& lsum, float& msum) {
    const float la = q.pow * log10f(fmaxf(a, q.eps)), lb = q.pow * log10f(fmaxf(b, q.eps));
    const float d = la - lb;
    lsum += fabsf(d);
    msum += fabsf(a - b);
    float g = 0.f;
    if (a >= q.eps) g = q.g_log * sl_sign(d) * q.pow / (a * SL_LN10);   // clamp passes no gradient below eps
    return fmaf(q.g_mag, sl_sign(a - b), g);
}

__global__ __launch_bounds__(SL_NT) void specloss_mel_kernel(const float* __restrict__ C, int F, int ncols, int nvalid, SlMel mel, SlTerm q,
                                                             float* __restrict__ dmel, float* __restrict__ part) {
    __shared__ float red[SL_NT];
    const int col = blockIdx.x * SL_NT + threadIdx.x, m = blockIdx.y;
    float lsum = 0.f, msum = 0.f;
    if (col < ncols) {
        const int lo = mel.lo[m], hi = mel.hi[m];
        const float* wt = mel.wt + mel.off[m];
        const float* Ca = C + col;
        const float* Cb = C + (size_t)2 * F * ncols + col;
        float a = 0.f, b = 0.f;
        for (int f = lo; f < hi; ++f) {
            const float ra = Ca[(size_t)f * ncols], ia = Ca[(size_t)(F + f) * ncols];
            const float rb = Cb[(size_t)f * ncols], ib = Cb[(size_t)(F + f) * ncols];
            a = fmaf(wt[f - lo], sqrtf(fmaf(ra, ra, ia * ia)), a);
            b = fmaf(wt[f - lo], sqrtf(fmaf(rb, rb, ib * ib)), b);
        }
        float l = 0.f, mg = 0.f;
        const float g = sl_term(a, b, q, l, mg);
        if (col < nvalid) { lsum = l; msum = mg; }
        if (dmel) dmel[(size_t)m * ncols + col] = col < nvalid ? g : 0.f;
    }
    lsum = sl_block_sum(lsum, red);
    msum = sl_block_sum(msum, red);
    if (threadIdx.x == 0) {
        const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x, nb = (size_t)gridDim.x * gridDim.y;
        part[blk] = lsum;
        part[nb + blk] = msum;
    }
}

__global__ __launch_bounds__(SL_NT) void specloss_bins_kernel(const float* __restrict__ C, int F, int ncols, int nvalid, int has_stft, SlTerm q,
                                                              SlMel mel, const float* __restrict__ dmel, float* __restrict__ G,
                                                              float* __restrict__ part) {
    __shared__ float red[SL_NT];
    const int col = blockIdx.x * SL_NT + threadIdx.x, f = blockIdx.y;
    float lsum = 0.f, msum = 0.f;
    if (col < ncols) {
        const float ra = C[(size_t)f * ncols + col], ia = C[(size_t)(F + f) * ncols + col];
        const float* Cb = C + (size_t)2 * F * ncols;
        const float rb = Cb[(size_t)f * ncols + col], ib = Cb[(size_t)(F + f) * ncols + col];
        const float a = sqrtf(fmaf(ra, ra, ia * ia)), b = sqrtf(fmaf(rb, rb, ib * ib));
        float g = 0.f;
        if (has_stft) {
            float l = 0.f, mg = 0.f;
            g = sl_term(a, b, q, l, mg);
            if (col < nvalid) { lsum = l; msum = mg; }
        }
        if (G) {
            if (dmel) {
                for (int m = mel.mlo[f]; m < mel.mhi[f]; ++m) {
                    const int lo = mel.lo[m];
                    if (f >= lo && f < mel.hi[m]) g = fmaf(mel.wt[mel.off[m] + f - lo], dmel[(size_t)m * ncols + col], g);
                }
            }
            const bool live = a > 0.f && col < nvalid;
            const float s = live ? g / a : 0.f;
            G[(size_t)f * ncols + col] = s * ra;
            G[(size_t)(F + f) * ncols + col] = s * ia;
        }
    }
    if (part) {
        lsum = sl_block_sum(lsum, red);
        msum = sl_block_sum(msum, red);
        if (threadIdx.x == 0) {
            const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x, nb = (size_t)gridDim.x * gridDim.y;
            part[blk] = lsum;
            part[nb + blk] = msum;
        }
    }
}

// dwm[b][s] += sum over every padded position p that reads sample s (p = s + w/2, and the mirrored p of the reflect padding) of
// sum over frames t with 0 <= p - t*hop < w of Q[p - t*hop][b*Tf + t]   (fixed order: direct, left mirror, right mirror; t ascending)
__global__ __launch_bounds__(SL_NT) void specloss_ola_kernel(const float* __restrict__ Q, float* __restrict__ dwm, int T, int Tf, int ncols, int w,
                                                             int hop) {
    const int s = blockIdx.x * SL_NT + threadIdx.x, b = blockIdx.y;
    if (s >= T) return;
    const int half = w / 2;
    const float* q = Q + (size_t)b * Tf;
    float acc = 0.f;
    auto gather = [&](int p) {
        const int t_lo = p >= w ? (p - w) / hop + 1 : 0;
        const int t_hi = min(Tf - 1, p / hop);
        for (int t = t_lo; t <= t_hi; ++t) acc += q[(size_t)(p - t * hop) * ncols + t];
    };
    gather(s + half);
    if (s >= 1 && s <= half) gather(half - s);
    if (s <= T - 2 && s >= T - 1 - half) gather(2 * (T - 1) - s + half);
    dwm[(size_t)b * T + s] += acc;
}

struct SlReduce {
    int n;
    int flags[SL_MAX_SCALES];
    long long off[SL_MAX_SCALES], nb_bins[SL_MAX_SCALES], nb_mel[SL_MAX_SCALES];   // partials: [bins log][bins mag][mel log][mel mag]
    double inv_stft[SL_MAX_SCALES], inv_mel[SL_MAX_SCALES];
    float stft_lw[SL_MAX_SCALES], stft_mw[SL_MAX_SCALES], mel_lw[SL_MAX_SCALES], mel_mw[SL_MAX_SCALES];
};

__device__ double sl_sum(const float* p, long long n, double* red) {
    double v = 0.0;
    for (long long i = threadIdx.x; i < n; i += SL_NT) v += (double)p[i];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = SL_NT / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(SL_NT) void specloss_reduce_kernel(const float* __restrict__ part, SlReduce r, float* __restrict__ terms,
                                                                float* __restrict__ totals) {
    __shared__ double red[SL_NT];
    double tot_stft = 0.0, tot_mel = 0.0;
    for (int s = 0; s < r.n; ++s) {
        const float* p = part + r.off[s];
        double ts = 0.0, tm = 0.0;
        if (r.flags[s] & 1) {
            const double l = sl_sum(p, r.nb_bins[s], red), m = sl_sum(p + r.nb_bins[s], r.nb_bins[s], red);
            ts = (r.stft_lw[s] * l + r.stft_mw[s] * m) * r.inv_stft[s];
        }
        if (r.flags[s] & 2) {
            const float* pm = p + 2 * r.nb_bins[s];
            const double l = sl_sum(pm, r.nb_mel[s], red), m = sl_sum(pm + r.nb_mel[s], r.nb_mel[s], red);
            tm = (r.mel_lw[s] * l + r.mel_mw[s] * m) * r.inv_mel[s];
        }
        if (threadIdx.x == 0) {
            terms[2 * s] = (float)ts;
            terms[2 * s + 1] = (float)tm;
        }
        tot_stft += ts;
        tot_mel += tm;
    }
    if (threadIdx.x == 0) {
        totals[0] = (float)tot_stft;
        totals[1] = (float)tot_mel;
    }
}

using wv::al256;
using wv::fail;

}  // namespace

struct wv_specloss_scale {
    int w = 0, flags = 0, n_mels = 0;
    float stft[4] = {0, 0, 0, 0}, mel[4] = {0, 0, 0, 0};          // log_weight, mag_weight, pow, clamp_eps
    float *wt_fwd = nullptr, *wt_bwd = nullptr, *mel_wt = nullptr;
    int* mel_idx = nullptr;                                      // lo[n_mels], hi[n_mels], off[n_mels], mlo[F], mhi[F]
};

struct wv_specloss_plan {
    std::vector<wv_specloss_scale> sc;
    ~wv_specloss_plan() {
        for (auto& s : sc) { (void)hipFree(s.wt_fwd); (void)hipFree(s.wt_bwd); (void)hipFree(s.mel_wt); (void)hipFree(s.mel_idx); }
    }
};

namespace {

struct SlGeom {
    int w, F, hop, Tf, ncols;
};
SlGeom sl_geom(const wv_specloss_scale& s, int B, int T) {
    SlGeom g;
    g.w = s.w; g.F = s.w / 2 + 1; g.hop = s.w / 4; g.Tf = T / g.hop + 1; g.ncols = wv::round_up(B * g.Tf, 4);
    return g;
}
size_t sl_nb(size_t ncols) { return (ncols + SL_NT - 1) / SL_NT; }

struct SlLayout {
    size_t fr = 0, c = 0, g = 0, dm = 0, part = 0;               // byte offsets
    size_t total = 0;
    std::vector<long long> poff, nb_bins, nb_mel;               // partials, in floats
};
SlLayout sl_layout(const wv_specloss_plan* p, int B, int T) {
    SlLayout L;
    size_t fr = 0, c = 0, g = 0, dm = 0;
    long long np = 0;
    for (const auto& s : p->sc) {
        const SlGeom q = sl_geom(s, B, T);
        fr = std::max(fr, (size_t)2 * q.w * q.ncols);
        c = std::max(c, (size_t)2 * 2 * q.F * q.ncols);
        g = std::max(g, (size_t)2 * q.F * q.ncols);
        if (s.flags & 2) dm = std::max(dm, (size_t)s.n_mels * q.ncols);
        const long long nbb = (s.flags & 1) ? (long long)sl_nb(q.ncols) * q.F : 0, nbm = (s.flags & 2) ? (long long)sl_nb(q.ncols) * s.n_mels : 0;
        L.poff.push_back(np); L.nb_bins.push_back(nbb); L.nb_mel.push_back(nbm);
        np += 2 * nbb + 2 * nbm;
    }
    L.fr = 0;
    L.c = L.fr + al256(fr * 4);
    L.g = L.c + al256(c * 4);
    L.dm = L.g + al256(g * 4);
    L.part = L.dm + al256(std::max<size_t>(dm, 1) * 4);
    L.total = L.part + al256((size_t)std::max<long long>(np, 1) * 4);
    return L;
}

hipError_t sl_gemm(const float* X, int M, int K, const float* wt, float* Y, int Bg, int ncols, hipStream_t s) {
    wv::DwPwArgs a{};
    a.X = X; a.pw.M = M; a.pw.K = K; a.pw.Mp = wv::round_up(M, wv::M_ALIGN); a.pw.Kp = wv::round_up(K, wv::BK); a.pw.wt = wt; a.pw.wq = nullptr;
    a.bias = nullptr; a.Y = Y; a.B = Bg; a.Tin = ncols; a.Tout = ncols; a.mode = 0; a.ks = 1; a.pre_scale = 1.f; a.pre_elu = 0; a.l2norm = 0;
    a.out_scale = 1.f;
    return wv::launch_dw_pw(a, s);
}

}  // namespace

extern "C" {

int wv_specloss_plan_create(int n_scales, const int* window_lengths, const int* flags, const int* n_mels, const float* params,
                            const float* windows, const float* mel_filters, wv_specloss_plan** out) {
    if (!out || n_scales < 1 || n_scales > SL_MAX_SCALES || !window_lengths || !flags || !params || !windows) return fail(WV_EINVAL, "null pointer (out, window_lengths, flags, params, windows) or n_scales outside [1, " + std::to_string(SL_MAX_SCALES) + "]");
    for (int i = 0; i < n_scales; ++i) {
        const int w = window_lengths[i];
        if (w < 8 || (w & 3) || w > 65536 || flags[i] < 1 || flags[i] > 3) return fail(WV_EINVAL, "a window length that is not a multiple of 4 in [8, 65536], or flags outside [1, 3]");
        if ((flags[i] & 2) && (!n_mels || n_mels[i] < 1 || !mel_filters)) return fail(WV_EINVAL, "a mel term without n_mels >= 1 or without mel_filters");
    }
    auto* p = new wv_specloss_plan();
    auto up = [](auto** d, const auto& v) {
        using E = typename std::decay_t<decltype(v)>::value_type;
        return hipMalloc((void**)d, std::max<size_t>(v.size(), 1) * sizeof(E)) == hipSuccess &&
               hipMemcpy(*d, v.data(), v.size() * sizeof(E), hipMemcpyHostToDevice) == hipSuccess;
    };
    const float* win = windows;
    const float* melp = mel_filters;
    for (int i = 0; i < n_scales; ++i) {
        wv_specloss_scale s;
        s.w = window_lengths[i]; s.flags = flags[i]; s.n_mels = (flags[i] & 2) ? n_mels[i] : 0;
        std::memcpy(s.stft, params + 8 * i, 4 * sizeof(float));
        std::memcpy(s.mel, params + 8 * i + 4, 4 * sizeof(float));
        const int w = s.w, F = w / 2 + 1, M2 = 2 * F;
        // windowed DFT basis, rows f: cos(2 pi f n / w) * win[n], rows F + f: -sin(2 pi f n / w) * win[n]  (angles reduced exactly mod w)
        std::vector<float> basis((size_t)M2 * w);
        for (int f = 0; f < F; ++f)
            for (int n = 0; n < w; ++n) {
                const double ang = 2.0 * M_PI * (double)(((long long)f * n) % w) / w;
                basis[(size_t)f * w + n] = (float)(std::cos(ang) * (double)win[n]);
                basis[(size_t)(F + f) * w + n] = (float)(-std::sin(ang) * (double)win[n]);
            }
        win += w;
        const int Mp_f = wv::round_up(M2, wv::M_ALIGN), Kp_f = wv::round_up(w, wv::BK);
        const int Mp_b = wv::round_up(w, wv::M_ALIGN), Kp_b = wv::round_up(M2, wv::BK);
        std::vector<float> wf((size_t)Kp_f * Mp_f, 0.f), wb((size_t)Kp_b * Mp_b, 0.f);
        for (int m = 0; m < M2; ++m)
            for (int n = 0; n < w; ++n) {
                wf[(size_t)n * Mp_f + m] = basis[(size_t)m * w + n];
                wb[(size_t)m * Mp_b + n] = basis[(size_t)m * w + n];
            }
        bool ok = up(&s.wt_fwd, wf) && up(&s.wt_bwd, wb);
        if (ok && (s.flags & 2)) {
            // the dense [n_mels][F] filters as bands of their non-zero bins
            const int nm = s.n_mels;
            std::vector<int> idx((size_t)3 * nm + 2 * F);
            int *lo = idx.data(), *hi = lo + nm, *off = hi + nm, *mlo = off + nm, *mhi = mlo + F;
            std::vector<float> wt;
            for (int f = 0; f < F; ++f) { mlo[f] = nm; mhi[f] = 0; }
            for (int m = 0; m < nm; ++m) {
                const float* row = melp + (size_t)m * F;
                int a = 0, b = F;
                while (a < F && row[a] == 0.f) ++a;
                while (b > a && row[b - 1] == 0.f) --b;
                lo[m] = a; hi[m] = b; off[m] = (int)wt.size();
                for (int f = a; f < b; ++f) {
                    wt.push_back(row[f]);
                    mlo[f] = std::min(mlo[f], m); mhi[f] = std::max(mhi[f], m + 1);
                }
            }
            for (int f = 0; f < F; ++f)
                if (mhi[f] == 0) mlo[f] = 0;
            melp += (size_t)nm * F;
            ok = up(&s.mel_wt, wt) && up(&s.mel_idx, idx);
        }
        p->sc.push_back(s);
        if (!ok) { delete p; return fail(WV_EHIP, "device allocation or upload of a scale's packs failed"); }
    }
    *out = p;
    return WV_OK;
}

void wv_specloss_plan_destroy(wv_specloss_plan* p) { delete p; }

size_t wv_specloss_workspace_bytes(const wv_specloss_plan* p, int B, int T) {
    if (!p || B < 1 || T < 1) return 0;
    return sl_layout(p, B, T).total;
}

int wv_specloss(const wv_specloss_plan* p, const float* wm, const float* x, int B, int T, float* terms, float* totals, float* dwm,
                float stft_grad_scale, float mel_grad_scale, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !wm || !x || !terms || !totals || B < 1 || T < 1 || B > 65535) return fail(WV_EINVAL, "null pointer (plan, wm, x, terms, totals), B outside [1, 65535] or T < 1");
    for (const auto& s : p->sc) {
        if (T <= s.w / 2) return fail(WV_EINVAL, "T <= w / 2 for some scale: the reflect padding needs more samples");                       // reflect padding needs w/2 < T
        if ((long long)B * (T / (s.w / 4) + 1) * (s.w + 2) > (1LL << 31) - 1) return fail(WV_EINVAL, "B * frames * (w + 2) exceeds 2^31 - 1 for some scale");
    }
    const SlLayout L = sl_layout(p, B, T);
    if (!ws || ws_bytes < L.total) return fail(WV_ENOMEM, "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    float* Fr = (float*)(base + L.fr);
    float* C = (float*)(base + L.c);
    float* G = (float*)(base + L.g);
    float* dm = (float*)(base + L.dm);
    float* part = (float*)(base + L.part);
    SlReduce r{};
    r.n = (int)p->sc.size();
    for (int i = 0; i < r.n; ++i) {
        const wv_specloss_scale& s = p->sc[i];
        const SlGeom q = sl_geom(s, B, T);
        const int nvalid = B * q.Tf, F = q.F;
        const double n_stft = (double)B * F * q.Tf, n_mel = (double)B * s.n_mels * q.Tf;
        hipLaunchKernelGGL(specloss_frames_kernel, dim3(sl_nb(q.ncols), q.w, 2), dim3(SL_NT), 0, st, wm, x, Fr, B, T, q.Tf, q.ncols, q.w, q.hop);
        WV_HIP_TRY(sl_gemm(Fr, 2 * F, q.w, s.wt_fwd, C, 2, q.ncols, st));
        SlMel mel{};
        if (s.flags & 2) {
            mel.lo = s.mel_idx; mel.hi = mel.lo + s.n_mels; mel.off = mel.hi + s.n_mels; mel.mlo = mel.off + s.n_mels; mel.mhi = mel.mlo + F;
            mel.wt = s.mel_wt; mel.n_mels = s.n_mels;
            SlTerm qm{s.mel[2], s.mel[3], (float)(mel_grad_scale * s.mel[0] / n_mel), (float)(mel_grad_scale * s.mel[1] / n_mel)};
            float* pm = part + L.poff[i] + 2 * L.nb_bins[i];
            hipLaunchKernelGGL(specloss_mel_kernel, dim3(sl_nb(q.ncols), s.n_mels), dim3(SL_NT), 0, st, C, F, q.ncols, nvalid, mel, qm,
                               dwm ? dm : nullptr, pm);
        }
        if ((s.flags & 1) || dwm) {
            SlTerm qs{s.stft[2], s.stft[3], (float)(stft_grad_scale * s.stft[0] / n_stft), (float)(stft_grad_scale * s.stft[1] / n_stft)};
            hipLaunchKernelGGL(specloss_bins_kernel, dim3(sl_nb(q.ncols), F), dim3(SL_NT), 0, st, C, F, q.ncols, nvalid, s.flags & 1, qs, mel,
                               (dwm && (s.flags & 2)) ? dm : nullptr, dwm ? G : nullptr, (s.flags & 1) ? part + L.poff[i] : nullptr);
        }
        if (dwm) {
            WV_HIP_TRY(sl_gemm(G, q.w, 2 * F, s.wt_bwd, Fr, 1, q.ncols, st));
            hipLaunchKernelGGL(specloss_ola_kernel, dim3((T + SL_NT - 1) / SL_NT, B), dim3(SL_NT), 0, st, Fr, dwm, T, q.Tf, q.ncols, q.w, q.hop);
        }
        r.flags[i] = s.flags; r.off[i] = L.poff[i]; r.nb_bins[i] = L.nb_bins[i]; r.nb_mel[i] = L.nb_mel[i];
        r.inv_stft[i] = 1.0 / n_stft; r.inv_mel[i] = s.n_mels ? 1.0 / n_mel : 0.0;
        r.stft_lw[i] = s.stft[0]; r.stft_mw[i] = s.stft[1]; r.mel_lw[i] = s.mel[0]; r.mel_mw[i] = s.mel[1];
    }
    hipLaunchKernelGGL(specloss_reduce_kernel, dim3(1), dim3(SL_NT), 0, st, part, r, terms, totals);
    WV_HIP_TRY(hipGetLastError());
    return WV_OK;
}

}  // extern "C"
