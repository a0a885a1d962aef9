// Psychoacoustic constraint projections for gfx950: LDS-staged Stockham FFT (STFT / iSTFT),
// fused spectral projections, wave-level reductions for the time-domain norms.
//
// Reference behaviour reproduced (paths into the reference's src/):
//   core/fourier_transforms.py:4-41      compute_stft / compute_istft
//   core/projections.py:11-159           project_{snr,linf,l2,tv,min_max_freqs,fm_norm,phon_level}
//   training_utils/train.py:27-99        _align_to, _project_frequency_domain, perturbation_constraint
//
// Data layout: waveforms (rows, L) f32 row-major.  Spectra are frame-major (rows, T, F) complex64
// so that one workgroup = one frame writes F contiguous bins.  The frequency-domain projections
// never materialise the spectrum: one kernel does window -> FFT -> per-bin op -> inverse FFT ->
// window and leaves windowed frames (rows, T, n_fft) for the overlap-add kernel.  All data-dependent
// branches of the reference ("scale only if over epsilon") become a predicated scale factor computed
// on the device, so a projection has no host synchronisation.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "paa_common.h"
#include "mask_kernels.h"
#include "spec_kernels.h"

namespace paa {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

constexpr int FFT_NT = 256;   // threads per frame workgroup
constexpr int RED_NT = 256;
constexpr int MAX_PART = 4096;

enum FrameOp { OP_STFT = 0, OP_MINMAX = 1, OP_PHON = 2, OP_FM = 3, OP_ISTFT = 4 };

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// In-LDS Stockham autosort FFT, radix 4 with one radix-2 pass when log2(N) is odd.
// INV=false: X[k] = sum x[n] e^{-2 pi i nk/N};  INV=true: unnormalised inverse.
// tw[m] = e^{-2 pi i m / N}.  Returns the buffer that holds the result (natural order).
template <bool INV>
__device__ float2* fft_lds(float2* src, float2* dst, const float2* __restrict__ tw, int N, int log2n) {
    const int tid = threadIdx.x;
    int Ns = 1;
    int rem = log2n;
    while (rem >= 2) {
        const int q = N >> 2;
        const int tstep = N / (Ns * 4);
        for (int j = tid; j < q; j += FFT_NT) {
            const int k = j & (Ns - 1);
            const int m = k * tstep;
            float2 v0 = src[j], v1 = src[j + q], v2 = src[j + 2 * q], v3 = src[j + 3 * q];
            if (k) {
                float2 w1 = tw[m], w2 = tw[2 * m], w3 = tw[3 * m];
                if (INV) { w1.y = -w1.y; w2.y = -w2.y; w3.y = -w3.y; }
                v1 = cmul(v1, w1); v2 = cmul(v2, w2); v3 = cmul(v3, w3);
            }
            const float2 a = make_float2(v0.x + v2.x, v0.y + v2.y);
            const float2 b = make_float2(v0.x - v2.x, v0.y - v2.y);
            const float2 c = make_float2(v1.x + v3.x, v1.y + v3.y);
            float2 d = make_float2(v1.x - v3.x, v1.y - v3.y);
            // forward: y1 = b - i d, y3 = b + i d ; inverse: swapped
            float2 id = INV ? make_float2(-d.y, d.x) : make_float2(d.y, -d.x);   // (-i d) fwd, (+i d) inv
            const int o = ((j - k) << 2) + k;
            dst[o] = make_float2(a.x + c.x, a.y + c.y);
            dst[o + Ns] = make_float2(b.x + id.x, b.y + id.y);
            dst[o + 2 * Ns] = make_float2(a.x - c.x, a.y - c.y);
            dst[o + 3 * Ns] = make_float2(b.x - id.x, b.y - id.y);
        }
        __syncthreads();
        float2* t = src; src = dst; dst = t;
        Ns <<= 2;
        rem -= 2;
    }
    if (rem == 1) {
        const int h = N >> 1;
        const int tstep = N / (Ns * 2);
        for (int j = tid; j < h; j += FFT_NT) {
            const int k = j & (Ns - 1);
            float2 v0 = src[j], v1 = src[j + h];
            if (k) {
                float2 w1 = tw[k * tstep];
                if (INV) w1.y = -w1.y;
                v1 = cmul(v1, w1);
            }
            const int o = ((j - k) << 1) + k;
            dst[o] = make_float2(v0.x + v1.x, v0.y + v1.y);
            dst[o + Ns] = make_float2(v0.x - v1.x, v0.y - v1.y);
        }
        __syncthreads();
        float2* t = src; src = dst; dst = t;
    }
    return src;
}

struct FrameArgs {
    const float* x;      // (rows, L) waveform            [all ops but ISTFT]
    const float* S_in;   // (rows, T, F) complex64        [ISTFT]
    float* S_out;        // (rows, T, F) complex64        [STFT]
    float* frames;       // (rows, T, N) windowed inverse frames
    double* part;        // (rows*T) per-frame partial sums [FM]
    const float2* tw;
    const float* win;
    const float* fm;     // [10][F], negative => out of the interpolator's frequency range
    const float* thr;    // [F] spl_thresh
    const float* thr_max;  // [1]
    int L, T, N, log2n, hop, F;
    float bin_hz, min_f, max_f, phon_ref;
    const float* rscale; // (rows) per-row bound scale, nullable [PHON: the threshold moves by 20 log10(s) dB]
};

// One workgroup = one STFT frame: window -> FFT -> OP on the F one-sided bins -> inverse FFT -> window.
template <int OP>
__global__ __launch_bounds__(FFT_NT) void k_frame(FrameArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2* buf0 = reinterpret_cast<float2*>(smem_raw);
    float2* buf1 = buf0 + a.N;
    __shared__ double red[FFT_NT / 64];
    const int t = blockIdx.x, row = blockIdx.y, tid = threadIdx.x;
    const int N = a.N, F = a.F, half = N >> 1;
    float2* X;
    if (OP != OP_ISTFT) {
        const float* x = a.x + (size_t)row * a.L;
        for (int n = tid; n < N; n += FFT_NT) {
            int s = t * a.hop + n - half;                  // center=True: reflect pad n_fft/2
            if (s < 0) s = -s;
            if (s >= a.L) s = 2 * (a.L - 1) - s;
            buf0[n] = make_float2(x[s] * a.win[n], 0.f);
        }
        __syncthreads();
        X = fft_lds<false>(buf0, buf1, a.tw, N, a.log2n);
    } else {
        const float2* S = reinterpret_cast<const float2*>(a.S_in) + ((size_t)row * a.T + t) * F;
        for (int k = tid; k < F; k += FFT_NT) buf0[k] = S[k];
        __syncthreads();
        X = buf0;
    }
    float2* Y = (X == buf0) ? buf1 : buf0;

    if (OP == OP_STFT) {
        float2* S = reinterpret_cast<float2*>(a.S_out) + ((size_t)row * a.T + t) * F;
        for (int k = tid; k < F; k += FFT_NT) S[k] = X[k];
        return;
    }
    double acc = 0.0;
    const float thr_row = (OP == OP_PHON && a.rscale) ? 20.f * log10f(row_scale(a.rscale, row)) : 0.f;
    for (int k = tid; k < F; k += FFT_NT) {
        float2 v = X[k];
        if (OP == OP_MINMAX) {
            // projections.py:68-80: keep bins OUTSIDE [min, max]
            const float f = (float)k * a.bin_hz;
            const float m = ((f < a.min_f) || (f > a.max_f)) ? 1.f : 0.f;
            v.x *= m; v.y *= m;
        } else if (OP == OP_PHON) {
            // projections.py:138-159
            const float mag = hypotf(v.x, v.y);
            const float mag_db = 20.f * log10f(mag + 1e-8f);
            float thr = (a.thr[k] - a.thr_max[0]) + a.phon_ref;
            if (a.rscale) thr += thr_row;
            const float db = (mag_db > thr) ? thr : mag_db;
            const float mc = exp10f(db / 20.f);
            const float ang = atan2f(v.y, v.x);
            float sn, cs;
            sincosf(ang, &sn, &cs);
            v = make_float2(mc * cs, mc * sn);
        } else if (OP == OP_FM) {
            // projections.py:83-113: weight = bilinear(iso grid)(10 log10(|S|^2 + 1e-10), f_bin); OOB -> 1
            const float mag = hypotf(v.x, v.y);
            const float pw = mag * mag;
            const float s = 10.f * log10f(pw + 1e-10f);
            float w = 1.f;
            const float w0 = a.fm[k];
            if (w0 >= 0.f && s >= 0.f && s <= 90.f) {
                int i = (int)floorf(s * 0.1f);
                i = i > 8 ? 8 : i;
                if (s <= 10.f * (float)i && i > 0) i -= 1;       // searchsorted(side='left') - 1
                const float ys = (s - 10.f * (float)i) * 0.1f;
                w = a.fm[i * F + k] * (1.f - ys) + a.fm[(i + 1) * F + k] * ys;
            }
            acc += (double)(pw * w);
        }
        if (k == 0 || k == half) v.y = 0.f;               // irfft ignores Im(DC), Im(Nyquist)
        Y[k] = v;
        if (k > 0 && k < half) Y[N - k] = make_float2(v.x, -v.y);
    }
    if (OP == OP_FM) {
        const double tot = block_sum<double, FFT_NT>(acc, red);
        if (tid == 0) a.part[(size_t)row * a.T + t] = tot;
    }
    __syncthreads();
    float2* y = fft_lds<true>(Y, X, a.tw, N, a.log2n);
    float* fr = a.frames + ((size_t)row * a.T + t) * N;
    const float inv = 1.f / (float)N;
    for (int n = tid; n < N; n += FFT_NT) fr[n] = y[n].x * inv * a.win[n];
}

// Overlap-add + envelope division + trim + _align_to (train.py:27-35): out (rows, out_len).
// Samples >= hop*(T-1) are zero (right zero-pad).  scal (nullable): row `row` is scaled by scal[row * scal_rs], scal_rs = 0 for
// one factor over all rows, 1 for a factor per row (per-row projections, paa_project_rows).
__global__ void k_ola(const float* __restrict__ frames, const float* __restrict__ win, const float* __restrict__ scal, int scal_rs,
                      float* __restrict__ out, int T, int N, int hop, int out_len) {
    const int row = blockIdx.y;
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= out_len) return;
    float v = 0.f;
    if (m < hop * (T - 1)) {
        const int s = m + (N >> 1);
        int t1 = s / hop;
        if (t1 > T - 1) t1 = T - 1;
        int t0 = (s - N + hop) / hop;                      // ceil((s - N + 1) / hop) for s-N+1 >= 0
        if (s - N + 1 <= 0) t0 = 0;
        float sum = 0.f, env = 0.f;
        const float* fr = frames + (size_t)row * T * N;
        for (int t = t0; t <= t1; ++t) {
            const int n = s - t * hop;
            sum += fr[(size_t)t * N + n];
            const float w = win[n];
            env += w * w;
        }
        v = sum / env;
        if (scal) v *= scal[row * scal_rs];
    }
    out[(size_t)row * out_len + m] = v;
}

// Statistic groups.  The kernels below take blockIdx.y as the group: a span of the rows projected under one statistic of its own,
// either all the rows (one group: the universal perturbation) or one row each (paa_project_rows).  Element and partial counts are
// per group, group g's partials start at g * (partials per group), rscale (nullable) holds one bound scale per group, and group
// 0 alone writes the diagnostic slots scal[0..2].  One group is the many-group kernel at blockIdx.y = 0: every offset is zero,
// row_scale(nullptr, .) is 1.0f and x * 1.0f is exact.

// projections.py:116-133 project_fm_norm: scale = eps / max(norm, 1e-8) if norm > eps else 1, eps = eps * rscale[g].
// One workgroup per group: it sums part[g * n, (g + 1) * n) and keeps the group's scale in gscale[g] (k_ola reads it there).
// gscale may be scal itself (one group, the spectrum-level entries): no __restrict__ on the two.
__global__ __launch_bounds__(RED_NT) void k_fm_finalize(const double* __restrict__ part, int n, float eps, float* gscale, float* scal,
                                                      const float* __restrict__ rscale) {
    __shared__ double red[RED_NT / 64];
    const int g = blockIdx.y;
    part += (size_t)g * n;
    eps = eps * row_scale(rscale, g);
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += RED_NT) s += part[i];
    s = block_sum<double, RED_NT>(s, red);
    if (threadIdx.x == 0) {
        const float norm = sqrtf((float)s);
        const float scale = (norm <= eps) ? 1.f : eps / fmaxf(norm, 1e-8f);
        gscale[g] = scale;
        if (g == 0) { scal[0] = scale; scal[1] = norm; }
    }
}

// Second launch of a fused spectral projection: dst = src * scale, the scale being the predicated FM factor computed from
// the per-workgroup partial sums of the first launch (every block re-sums the few hundred partials of its group: no third
// launch); npart = 0: plain copy (min_max_freqs / max_phon / masking, in-place form only).
__global__ __launch_bounds__(RED_NT) void k_spec_finish(const float* __restrict__ src, float* __restrict__ dst, int64_t n,
                                                      const double* __restrict__ part, int npart, float eps, float* __restrict__ scal,
                                                      const float* __restrict__ rscale) {
    __shared__ double red[RED_NT / 64];
    const int g = blockIdx.y;
    eps = eps * row_scale(rscale, g);
    src += (size_t)g * n;
    dst += (size_t)g * n;
    float scale = 1.f;
    if (npart > 0) {
        part += (size_t)g * npart;
        double s = 0.0;
        for (int i = threadIdx.x; i < npart; i += RED_NT) s += part[i];
        s = block_sum<double, RED_NT>(s, red);
        const float norm = sqrtf((float)s);
        scale = (norm <= eps) ? 1.f : eps / fmaxf(norm, 1e-8f);
        if (g == 0 && blockIdx.x == 0 && threadIdx.x == 0) { scal[0] = scale; scal[1] = norm; }
    }
    const int64_t n4 = n >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {
        for (int64_t i = (int64_t)blockIdx.x * RED_NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * RED_NT) {
            float4 v = s4[i];
            v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
            d4[i] = v;
        }
        for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * RED_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RED_NT) dst[i] = src[i] * scale;
    } else {
        for (int64_t i = (int64_t)blockIdx.x * RED_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RED_NT) dst[i] = src[i] * scale;
    }
}

// ---- time-domain reductions --------------------------------------------------------------------
enum RedMode { RED_SQ = 0, RED_TV = 1 };

// Blocks [0, g1) reduce x1 (n1 elements, rows of length L1), blocks [g1, g1+g2) reduce x2; n1 / n2 are per group, group
// blockIdx.y reads x1 + g n1 and x2 + g n2 and writes its g1 + g2 partials to part[g (g1 + g2) + ...]: each row of a per-row call is
// reduced exactly as a one-row call reduces it.
template <int MODE>
__global__ __launch_bounds__(RED_NT) void k_reduce2(const float* __restrict__ x1, int64_t n1, int L1, int g1,
                                                  const float* __restrict__ x2, int64_t n2, int L2, int g2,
                                                  double* __restrict__ part) {
    __shared__ double red[RED_NT / 64];
    x1 += (size_t)blockIdx.y * n1;
    x2 += (size_t)blockIdx.y * n2;
    part += (size_t)blockIdx.y * (g1 + g2);
    const bool first = (int)blockIdx.x < g1;
    const float* x = first ? x1 : x2;
    const int64_t n = first ? n1 : n2;
    const int L = first ? L1 : L2;
    const int g = first ? g1 : g2;
    const int b = first ? blockIdx.x : blockIdx.x - g1;
    float acc = 0.f;
    double dacc = 0.0;
    int cnt = 0;
    for (int64_t i = (int64_t)b * RED_NT + threadIdx.x; i < n; i += (int64_t)g * RED_NT) {
        if (MODE == RED_SQ) {
            const float v = x[i];
            acc += v * v;
        } else {
            if ((int)(i % L) != L - 1) acc += fabsf(x[i + 1] - x[i]);
        }
        if (++cnt == 64) { dacc += (double)acc; acc = 0.f; cnt = 0; }
    }
    dacc += (double)acc;
    dacc = block_sum<double, RED_NT>(dacc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = dacc;
}

struct ApplyArgs {
    const double* part;
    int g1, g2;
    float eps;          // l2_size | tv_epsilon
    float snr_db, snr_linear;
    double numel_clean, numel_p;
    float* scal;        // [0] scale applied, [1..] diagnostics
    const float* ext;   // optional device [sum clean^2, TV(clean)] supplied by the caller (data-parallel runs)
    const float* ext_clips;   // optional device [1]: number of clean clips over ALL ranks (an exact small integer in f32);
    double clip_len;          //   numel_clean = ext_clips[0] * clip_len then replaces the host value above
    const float* rscale;      // optional device (groups) bound scale s of each group (paa_project_rows_scaled): l2 / tv eps * s, snr_db - 20 log10(s)
};

// p = src * scale (src == p: in place; otherwise the out-of-place form reads the caller's source directly — no copy in front)
// n is the element count of a group; group blockIdx.y's scale comes from its own g1 + g2 partials (k_reduce2).
template <int NORM>
__global__ __launch_bounds__(RED_NT) void k_apply_scale(const float* src, float* p, int64_t n, ApplyArgs a) {
    __shared__ double red[RED_NT / 64];
    const int g = blockIdx.y;
    src += (size_t)g * n;
    p += (size_t)g * n;
    a.part += (size_t)g * (a.g1 + a.g2);
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < a.g1; i += RED_NT) s1 += a.part[i];
    for (int i = threadIdx.x; i < a.g2; i += RED_NT) s2 += a.part[a.g1 + i];
    s1 = block_sum<double, RED_NT>(s1, red);
    s2 = block_sum<double, RED_NT>(s2, red);
    if (a.ext) s1 = (double)a.ext[NORM == PAA_NORM_TV ? 1 : 0];
    const double numel_clean = a.ext_clips ? (double)a.ext_clips[0] * a.clip_len : a.numel_clean;
    float scale = 1.f;
    // the group's bound scale: x * 1.0f and x - 20 log10f(1.0f) are exact, so s = 1 gives the bits of the unscaled projection
    const float rs = row_scale(a.rscale, g);
    if (NORM == PAA_NORM_L2) {                     // projections.py:41-46 (s2 = sum p^2)
        const float norm = sqrtf((float)s2);
        const float eps = a.eps * rs;
        if (norm > eps) scale = eps / norm;
    } else if (NORM == PAA_NORM_SNR) {             // projections.py:11-35 (s1 = sum clean^2, s2 = sum p^2)
        const float sp = (float)(s1 / numel_clean);
        const float np_ = (float)(s2 / a.numel_p);
        const float cur = 10.f * log10f(sp / (np_ + 1e-12f));
        float want = a.snr_db;
        if (a.rscale) want = a.snr_db - 20.f * log10f(rs);
        if (!(cur >= want)) {
            const float target = sqrtf(sp / a.snr_linear * (float)numel_clean) * rs;
            const float cn = sqrtf((float)s2);
            if (!(cn < 1e-8f)) scale = target / cn;
        }
    } else if (NORM == PAA_NORM_TV) {              // projections.py:56-66 (s1 = TV(clean), s2 = TV(p))
        const float eps = (a.eps * rs) * (float)s1;
        const float tv = (float)s2;
        if (tv > eps) scale = eps / tv;
    }
    if (g == 0 && blockIdx.x == 0 && threadIdx.x == 0) { a.scal[0] = scale; a.scal[1] = (float)s1; a.scal[2] = (float)s2; }
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(p)) & 15) == 0) {
        const int64_t n4 = n >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* p4 = reinterpret_cast<float4*>(p);
        for (int64_t i = (int64_t)blockIdx.x * RED_NT + threadIdx.x; i < n4; i += (int64_t)gridDim.x * RED_NT) {
            float4 v = s4[i];
            v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
            p4[i] = v;
        }
        for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * RED_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RED_NT) p[i] = src[i] * scale;
    } else {
        for (int64_t i = (int64_t)blockIdx.x * RED_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RED_NT) p[i] = src[i] * scale;
    }
}

__global__ void k_clamp(const float* src, float* p, int64_t n, float lo, float hi) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = fminf(fmaxf(src[i], lo), hi);       // torch.clamp propagates NaN; fminf/fmaxf do not: see DESIGN.md
}

// linf with a per-row bound scale: row blockIdx.y is clamped to +-(lim * s_row)
__global__ void k_clamp_rows(const float* src, float* p, int L, float lim, const float* __restrict__ rscale) {
    const float hi = lim * row_scale(rscale, blockIdx.y);
    src += (size_t)blockIdx.y * L;
    p += (size_t)blockIdx.y * L;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L; i += gridDim.x * blockDim.x)
        p[i] = fminf(fmaxf(src[i], -hi), hi);
}

__global__ void k_sign_step(float* __restrict__ p, const float* __restrict__ g, float lr, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = g[i];
    const float s = (v > 0.f) ? 1.f : ((v < 0.f) ? -1.f : v);   // sign(0) = 0, sign(NaN) = NaN
    p[i] = p[i] + lr * s;
}

// train.py:165-175 with torch.optim.Adam(lr) as build.py:352-359 builds it: one element of torch's foreach Adam step
// (torch/optim/adam.py _multi_tensor_adam, non-capturable; see paa_adam_step in include/paa_hip.h).  Every rounding is
// spelled out: contraction is off, and the three FMAs are the ones torch's gfx950 foreach kernels execute (lerp, addcmul,
// addcdiv each compile to one v_fma_f32 / v_pk_fma_f32 there); the sqrt and the two divisions are IEEE-rounded, as there.
struct AdamScal {
    float step_size, bc2_sqrt, w1, beta2, omb2, eps, grad_sign;
};

__device__ __forceinline__ void adam_elem(float& p, float gin, float& m, float& v, float& gout, const AdamScal& s) {
#pragma clang fp contract(off)
    const float g = s.grad_sign * gin;
    const float diff = g - m;                                            // ATen/native/Lerp.h
    m = (fabsf(s.w1) < 0.5f) ? __builtin_fmaf(s.w1, diff, m) : __builtin_fmaf(-diff, 1.f - s.w1, g);
    v = v * s.beta2;                                                     // _foreach_mul_
    v = __builtin_fmaf(s.omb2, g * g, v);                                // _foreach_addcmul_
    float d = sqrtf(v) / s.bc2_sqrt;                                     // _foreach_sqrt, _foreach_div_
    d = d + s.eps;                                                       // _foreach_add_
    p = __builtin_fmaf(s.step_size, m / d, p);                           // _foreach_addcdiv_
    gout = g;
}

// Streaming: one float4 of each operand per thread, the L % 4 tail by the first threads of block 0.  The vector path
// needs every pointer 16-byte aligned; otherwise the whole vector is done element by element.
__global__ void k_adam_step(float* __restrict__ p, const float* __restrict__ grad, float grad_sign, float* __restrict__ m,
                            float* __restrict__ v, const float* __restrict__ scal, float w1, float beta2, float omb2, float eps,
                            float* __restrict__ gout, int n, int vec) {
    const AdamScal s{scal[0], scal[1], w1, beta2, omb2, eps, grad_sign};
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n4 = vec ? (n >> 2) : 0;
    if (i < n4) {
        float4 pp = reinterpret_cast<const float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(grad)[i];
        float4 mm = reinterpret_cast<const float4*>(m)[i];
        float4 vv = reinterpret_cast<const float4*>(v)[i];
        float4 go;
        adam_elem(pp.x, gg.x, mm.x, vv.x, go.x, s);
        adam_elem(pp.y, gg.y, mm.y, vv.y, go.y, s);
        adam_elem(pp.z, gg.z, mm.z, vv.z, go.z, s);
        adam_elem(pp.w, gg.w, mm.w, vv.w, go.w, s);
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (gout) reinterpret_cast<float4*>(gout)[i] = go;
    }
    const int j = (n4 << 2) + i;                 // the elements the vector path leaves: at most 3, or all of them
    if (j < n && (!vec || i < 4)) {
        float pp = p[j], mm = m[j], vv = v[j], go;
        adam_elem(pp, grad[j], mm, vv, go, s);
        p[j] = pp;
        m[j] = mm;
        v[j] = vv;
        if (gout) gout[j] = go;
    }
}

__global__ void k_compose_clamp(const float* __restrict__ x, const float* __restrict__ p, float* __restrict__ out,
                                int B, int L) {
    const int64_t n = (int64_t)B * L;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = fminf(fmaxf(x[i] + p[i % L], -1.f), 1.f);
}

// out[b][i] = clamp(x[b][i] + p[b][i], -1, 1): one perturbation row per clip
__global__ void k_compose_clamp_rows(const float* __restrict__ x, const float* __restrict__ p, float* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = fminf(fmaxf(x[i] + p[i], -1.f), 1.f);
}

}  // namespace paa

using namespace paa;

struct paa_proj {
    int n_fft, hop, win, sr, F, log2n, max_batch, max_len;
    float2* d_tw = nullptr;
    float* d_win = nullptr;
    float* d_fm = nullptr;
    float* d_thr = nullptr;
    float* d_thr_max = nullptr;
    float* d_frames = nullptr;
    double* d_part = nullptr;
    float* d_scal = nullptr;
    size_t frames_floats = 0;
    // masking norm (default geometry only): bound / threshold workspace (max_batch, Tmax, F), pass 1's per-workgroup maxima,
    // and the per-bin tables [z | quiet | ath] (3 F floats) + packed windows (F ints)
    float* d_mask = nullptr;
    float* d_mpart = nullptr;
    float* d_mtab = nullptr;
    int* d_mwin = nullptr;
    int mask_kA = 0;
    // temporal masking (paa_proj_set_masking_spread): off while both tables are empty.  d_mask2: the second
    // (max_batch, Tmax, F) plane pass 2 writes theta into, allocated on first use; d_mpmax: Pmax per row for a caller that asks for none
    int n_post = 0, n_pre = 0;
    float post_db[MASK_LAGS] = {}, pre_db[MASK_LAGS] = {};
    float* d_mask2 = nullptr;
    float* d_mpmax = nullptr;
};

extern "C" const char* paa_last_error(void) { return paa::g_err.c_str(); }
// 350 + 1 if the library was built with -DPAA_EXPERIMENTS (diagnostic configurations and environment switches present)
extern "C" int paa_version(void) {
#ifdef PAA_EXPERIMENTS
    return 351;
#else
    return 350;
#endif
}

extern "C" paa_status paa_proj_set_spl_thresh(paa_proj* h, const float* spl) {
    if (!h || !spl) PAA_FAIL(PAA_ERR_ARG, "paa_proj_set_spl_thresh: null argument");
    float mx = spl[0];
    for (int i = 1; i < h->F; ++i) mx = spl[i] > mx ? spl[i] : mx;
    PAA_HIP(hipMemcpy(h->d_thr, spl, sizeof(float) * h->F, hipMemcpyHostToDevice));
    PAA_HIP(hipMemcpy(h->d_thr_max, &mx, sizeof(float), hipMemcpyHostToDevice));
    return PAA_OK;
}

extern "C" paa_status paa_proj_create(paa_proj** out, int n_fft, int hop, int win, int sr, const double* fm_table,
                                      const float* spl_thresh, int max_batch, int max_len) {
    if (!out) PAA_FAIL(PAA_ERR_ARG, "paa_proj_create: out is null");
    int log2n = 0;
    while ((1 << log2n) < n_fft) ++log2n;
    if ((1 << log2n) != n_fft || n_fft < 64 || n_fft > 4096)
        PAA_FAIL(PAA_ERR_ARG, "n_fft=%d unsupported: must be a power of two in [64, 4096]", n_fft);
    if (win != n_fft) PAA_FAIL(PAA_ERR_ARG, "win_length=%d != n_fft=%d is not supported", win, n_fft);
    if (hop <= 0 || hop > n_fft) PAA_FAIL(PAA_ERR_ARG, "hop_length=%d out of range", hop);
    if (max_batch < 1 || max_len <= n_fft / 2) PAA_FAIL(PAA_ERR_SIZE, "max_batch/max_len too small");
    paa_proj* h = new paa_proj();
    h->n_fft = n_fft; h->hop = hop; h->win = win; h->sr = sr; h->F = n_fft / 2 + 1; h->log2n = log2n;
    h->max_batch = max_batch; h->max_len = max_len;
    const int F = h->F;
    std::vector<float2> tw(n_fft);
    std::vector<float> w(n_fft);
    for (int m = 0; m < n_fft; ++m) {
        const double ang = -2.0 * M_PI * (double)m / (double)n_fft;
        tw[m] = make_float2((float)cos(ang), (float)sin(ang));
        w[m] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)m / (double)n_fft));   // torch.hann_window (periodic)
    }
    // torch.istft refuses windows whose overlap-added squared envelope touches zero (NOLA); so does this library
    // (hop == n_fft with a Hann window would divide by zero in the overlap-add)
    for (int r = 0; r < hop; ++r) {
        double env = 0.0;
        for (int n = r; n < n_fft; n += hop) env += (double)w[n] * (double)w[n];
        if (env < 1e-11) { delete h; PAA_FAIL(PAA_ERR_ARG, "window overlap-add envelope is zero at offset %d (hop_length=%d, n_fft=%d): iSTFT undefined", r, hop, n_fft); }
    }
    std::vector<float> fm(10 * F, 1.f), thr(F, 0.f);
    if (fm_table) for (int i = 0; i < 10 * F; ++i) fm[i] = (float)fm_table[i];
    const int Tmax = 1 + max_len / hop;
    h->frames_floats = (size_t)max_batch * Tmax * n_fft;
#define PC(e) do { hipError_t _e = (e); if (_e != hipSuccess) { paa::set_error(std::string(#e) + ": " + hipGetErrorString(_e)); paa_proj_destroy(h); return PAA_ERR_HIP; } } while (0)
    PC(hipMalloc(&h->d_tw, sizeof(float2) * n_fft));
    PC(hipMalloc(&h->d_win, sizeof(float) * n_fft));
    PC(hipMalloc(&h->d_fm, sizeof(float) * 10 * F));
    PC(hipMalloc(&h->d_thr, sizeof(float) * F));
    PC(hipMalloc(&h->d_thr_max, sizeof(float)));
    PC(hipMalloc(&h->d_frames, sizeof(float) * h->frames_floats));
    PC(hipMalloc(&h->d_part, sizeof(double) * (MAX_PART + (size_t)max_batch * Tmax)));
    PC(hipMalloc(&h->d_scal, sizeof(float) * 8));
    PC(hipMemcpy(h->d_tw, tw.data(), sizeof(float2) * n_fft, hipMemcpyHostToDevice));
    PC(hipMemcpy(h->d_win, w.data(), sizeof(float) * n_fft, hipMemcpyHostToDevice));
    PC(hipMemcpy(h->d_fm, fm.data(), sizeof(float) * 10 * F, hipMemcpyHostToDevice));
    PC(hipMemset(h->d_scal, 0, sizeof(float) * 8));
    if (n_fft == 1024 && hop == 256 && win == 1024) {
        std::vector<float> mt(3 * F);
        std::vector<int> mw(F);
        mask_tables(sr, mt.data(), mt.data() + F, mt.data() + 2 * F, mw.data(), &h->mask_kA);
        PC(hipMalloc(&h->d_mask, sizeof(float) * (size_t)max_batch * Tmax * F));
        PC(hipMalloc(&h->d_mpart, sizeof(float) * (size_t)max_batch * spec_psd_groups(Tmax)));
        PC(hipMalloc(&h->d_mtab, sizeof(float) * 3 * F));
        PC(hipMalloc(&h->d_mwin, sizeof(int) * F));
        PC(hipMemcpy(h->d_mtab, mt.data(), sizeof(float) * 3 * F, hipMemcpyHostToDevice));
        PC(hipMemcpy(h->d_mwin, mw.data(), sizeof(int) * F, hipMemcpyHostToDevice));
    }
#undef PC
    if (spl_thresh) {
        paa_status s = paa_proj_set_spl_thresh(h, spl_thresh);
        if (s != PAA_OK) { paa_proj_destroy(h); return s; }
    } else {
        thr.assign(F, 0.f);
        paa_proj_set_spl_thresh(h, thr.data());
    }
    *out = h;
    return PAA_OK;
}

#ifdef PAA_SPEC_STAMP
// diagnostic builds only (tools/fft_stamps.py): the per-iteration s_memtime stamps k_spec_run left in the FM partial array
extern "C" paa_status paa_debug_spec_stamps(paa_proj* h, long long* host, int n) {
    PAA_HIP(hipDeviceSynchronize());
    PAA_HIP(hipMemcpy(host, h->d_part + MAX_PART, sizeof(long long) * n, hipMemcpyDeviceToHost));
    return PAA_OK;
}
#endif

extern "C" void paa_proj_destroy(paa_proj* h) {
    if (!h) return;
    void* ptrs[] = {h->d_tw, h->d_win, h->d_fm, h->d_thr, h->d_thr_max, h->d_frames, h->d_part, h->d_scal,
                    h->d_mask, h->d_mpart, h->d_mtab, h->d_mwin, h->d_mask2, h->d_mpmax};
    for (void* q : ptrs) if (q) (void)hipFree(q);
    delete h;
}

static paa_status check_rows(const paa_proj* h, int rows, int L, const char* who) {
    if (rows < 1 || rows > h->max_batch) PAA_FAIL(PAA_ERR_SIZE, "%s: rows=%d exceeds max_batch=%d", who, rows, h->max_batch);
    if (L > h->max_len) PAA_FAIL(PAA_ERR_SIZE, "%s: L=%d exceeds max_len=%d", who, L, h->max_len);
    if (L <= h->n_fft / 2) PAA_FAIL(PAA_ERR_SIZE, "%s: L=%d must exceed n_fft/2=%d (reflect padding)", who, L, h->n_fft / 2);
    return PAA_OK;
}

static FrameArgs frame_args(const paa_proj* h, int L, int T) {
    FrameArgs a{};
    a.tw = h->d_tw; a.win = h->d_win; a.fm = h->d_fm; a.thr = h->d_thr; a.thr_max = h->d_thr_max;
    a.frames = h->d_frames; a.part = h->d_part + MAX_PART;
    a.L = L; a.T = T; a.N = h->n_fft; a.log2n = h->log2n; a.hop = h->hop; a.F = h->F;
    a.bin_hz = (float)((double)h->sr / (double)h->n_fft);
    return a;
}

static bool fused_geometry(const paa_proj* h) { return h->n_fft == 1024 && h->hop == 256 && h->win == 1024; }
static SpecArgs spec_args(const paa_proj* h, int L, int T, int out_len) {
    SpecArgs a{};
    a.tw = h->d_tw; a.win = h->d_win; a.fm = h->d_fm; a.thr = h->d_thr; a.thr_max = h->d_thr_max;
    a.part = h->d_part + MAX_PART;
    a.L = L; a.T = T; a.out_len = out_len;
    a.bin_hz = (float)((double)h->sr / (double)h->n_fft);
    return a;
}
static int spec_op_of(int norm) {
    return norm == PAA_NORM_MIN_MAX_FREQS ? SOP_MINMAX : norm == PAA_NORM_MAX_PHON ? SOP_PHON : norm == PAA_NORM_FLETCHER_MUNSON ? SOP_FM
         : norm == PAA_NORM_MASKING ? SOP_MASK : SOP_NONE;
}

// Temporal masking: the decrement tables of the post- and pre-masking spread, post_db[j - 1] = w_post[j] dB at lag j
// frames.  Both empty: the mode is off and masking_pass launches what it launched before this entry existed.
extern "C" paa_status paa_proj_set_masking_spread(paa_proj* h, int n_post, const float* post_db, int n_pre, const float* pre_db) {
    if (!h) PAA_FAIL(PAA_ERR_ARG, "paa_proj_set_masking_spread: null handle");
    if (!fused_geometry(h) || !h->d_mask)
        PAA_FAIL(PAA_ERR_ARG, "masking needs n_fft = win_length = 1024, hop_length = 256 (got %d / %d / %d)", h->n_fft, h->win, h->hop);
    const int n[2] = {n_post, n_pre};
    const float* tab[2] = {post_db, pre_db};
    for (int s = 0; s < 2; ++s) {
        const char* side = s ? "pre" : "post";
        if (n[s] < 0 || n[s] > MASK_LAGS)
            PAA_FAIL(PAA_ERR_ARG, "paa_proj_set_masking_spread: n_%s=%d must lie in [0, %d]", side, n[s], MASK_LAGS);
        if (n[s] > 0 && !tab[s]) PAA_FAIL(PAA_ERR_ARG, "paa_proj_set_masking_spread: %s_db is null with n_%s=%d", side, side, n[s]);
        for (int j = 0; j < n[s]; ++j)
            if (!(std::isfinite(tab[s][j]) && tab[s][j] > 0.f && (j == 0 || tab[s][j] >= tab[s][j - 1])))
                PAA_FAIL(PAA_ERR_ARG, "paa_proj_set_masking_spread: %s_db[%d]=%g must be finite, positive and not below %s_db[%d]", side, j,
                         (double)tab[s][j], side, j > 0 ? j - 1 : 0);
    }
    if ((n_post || n_pre) && !h->d_mask2) {
        const size_t Tmax = 1 + h->max_len / h->hop;
        PAA_HIP(hipMalloc(&h->d_mask2, sizeof(float) * (size_t)h->max_batch * Tmax * h->F));
        PAA_HIP(hipMalloc(&h->d_mpmax, sizeof(float) * (size_t)h->max_batch));
    }
    h->n_post = n_post; h->n_pre = n_pre;
    for (int j = 0; j < MASK_LAGS; ++j) {
        h->post_db[j] = j < n_post ? post_db[j] : 0.f;
        h->pre_db[j] = j < n_pre ? pre_db[j] : 0.f;
    }
    return PAA_OK;
}

// Masking threshold of the clean clips (B, L) into h->d_mask (passes 1 and 2 of mask_kernels.hip): theta (dB) into d_theta when
// given, else the magnitude bound A in place in h->d_mask; with min_rows, pass 3 leaves min_b A_b in row 0.  With temporal masking on,
// pass 2 writes theta into h->d_mask2 and k_mask_spread writes theta' into d_theta, or the bound A' into h->d_mask.
static paa_status masking_pass(paa_proj* h, const float* d_clean, int B, int L, float margin, float* d_psd, float* d_theta,
                               float* d_pmax, bool min_rows, hipStream_t st) {
    if (!d_clean || B < 1) PAA_FAIL(PAA_ERR_NEED_CLEAN, "masking projection requires clean_audio");
    if (!fused_geometry(h) || !h->d_mask)
        PAA_FAIL(PAA_ERR_ARG, "masking needs n_fft = win_length = 1024, hop_length = 256 (got %d / %d / %d)", h->n_fft, h->win, h->hop);
    PAA_TRY(check_rows(h, B, L, "masking"));
    const int T = 1 + L / h->hop;
    SpecArgs sa = spec_args(h, L, T, 0);
    sa.x = d_clean; sa.psd = h->d_mask; sa.pmax_part = h->d_mpart;
    PAA_TRY(spec_psd(sa, B, st));
    MaskArgs ma{};
    ma.P = h->d_mask; ma.part = h->d_mpart; ma.nparts = spec_psd_groups(T);
    ma.out = d_theta ? d_theta : h->d_mask; ma.psd = d_psd; ma.pmax = d_pmax;
    ma.tab = MaskTables{h->d_mtab, h->d_mtab + h->F, h->d_mtab + 2 * h->F, h->d_mwin, h->mask_kA};
    ma.T = T; ma.bound = d_theta ? 0 : 1; ma.margin = margin;
    if (h->n_post || h->n_pre) {
        MaskSpreadArgs sp{};
        sp.theta = h->d_mask2; sp.out = ma.out; sp.T = T; sp.bound = ma.bound; sp.margin = margin;
        sp.n_post = h->n_post; sp.n_pre = h->n_pre;
        std::copy(h->post_db, h->post_db + MASK_LAGS, sp.post);
        std::copy(h->pre_db, h->pre_db + MASK_LAGS, sp.pre);
        if (!ma.pmax) ma.pmax = h->d_mpmax;
        sp.pmax = ma.pmax;
        ma.out = h->d_mask2; ma.bound = 0;
        PAA_TRY(mask_threshold(ma, B, st));
        PAA_TRY(mask_spread(sp, B, st));
    } else {
        PAA_TRY(mask_threshold(ma, B, st));
    }
    if (min_rows && !d_theta) PAA_TRY(mask_min_rows(h->d_mask, B, (int64_t)T * h->F, st));
    return PAA_OK;
}

template <int OP>
static paa_status launch_frames(const paa_proj* h, const FrameArgs& a, int rows, hipStream_t st) {
    const size_t lds = 2 * sizeof(float2) * h->n_fft;
    hipLaunchKernelGGL(k_frame<OP>, dim3(a.T, rows), dim3(FFT_NT), lds, st, a);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_stft(paa_proj* h, const float* d_x, int B, int L, float* d_out, void* stream) {
    if (!h || !d_x || !d_out) PAA_FAIL(PAA_ERR_ARG, "paa_stft: null argument");
    PAA_TRY(check_rows(h, B, L, "paa_stft"));
    if (fused_geometry(h)) {
        SpecArgs sa = spec_args(h, L, 1 + L / h->hop, 0);
        sa.x = d_x; sa.S_out = d_out;
        return spec_stft(sa, B, (hipStream_t)stream);
    }
    FrameArgs a = frame_args(h, L, 1 + L / h->hop);
    a.x = d_x; a.S_out = d_out;
    return launch_frames<OP_STFT>(h, a, B, (hipStream_t)stream);
}

extern "C" paa_status paa_istft(paa_proj* h, const float* d_S, int B, int T, float* d_out, void* stream) {
    if (!h || !d_S || !d_out) PAA_FAIL(PAA_ERR_ARG, "paa_istft: null argument");
    if (T < 2) PAA_FAIL(PAA_ERR_SIZE, "paa_istft: T=%d", T);
    if (B < 1 || B > h->max_batch || (size_t)B * T * h->n_fft > h->frames_floats)
        PAA_FAIL(PAA_ERR_SIZE, "paa_istft: B=%d T=%d exceeds the workspace", B, T);
    hipStream_t st = (hipStream_t)stream;
    if (fused_geometry(h)) {
        SpecArgs sa = spec_args(h, 0, T, h->hop * (T - 1));
        sa.S_in = d_S; sa.out = d_out;
        return spec_istft(sa, B, st);
    }
    FrameArgs a = frame_args(h, 0, T);
    a.S_in = d_S;
    PAA_TRY(launch_frames<OP_ISTFT>(h, a, B, st));
    const int out_len = h->hop * (T - 1);
    hipLaunchKernelGGL(k_ola, dim3(cdiv(out_len, 256), B), dim3(256), 0, st, h->d_frames, h->d_win, (const float*)nullptr, 0,
                       d_out, T, h->n_fft, h->hop, out_len);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

// One projection call, as every entry below describes its own.  The rows are projected in `groups` statistic groups: 1 = one
// statistic over all the rows (the universal perturbation: perturbation_constraint(p, clean, args), train.py:69-99), rows = every
// row under its own (per-clip perturbations: row r exactly as perturbation_constraint(src[r][None], clean[r][None], args) projects
// it — l2 / fletcher_munson from the row's own norm, snr from clean row r's own mean power, tv from TV(clean[r])).
struct ProjCall {
    const char* who;           // the entry's name, for messages
    const float* src;          // (rows, L); src == dst: in place, otherwise the two must not overlap
    float* dst;
    int rows, L;
    int groups;                // 1 or rows
    const float* clean;        // (B, L) clean clips, nullable; groups == rows: B == rows, clip r belongs to row r
    int B;
    const float* ext;          // device [sum clean^2, TV(clean)] in place of the clean clips (paa_project_ext), nullable
    const float* ext_clips;    // with ext: device [1] clip count over all ranks, nullable (then ext_numel holds clean.numel())
    double ext_numel;
    const float* rscale;       // device (groups) bound scale of each group (paa_project_rows_scaled), nullable
};

static bool overlap(const float* a, const float* b, int64_t n) { return (a < b ? a : b) + n > (a < b ? b : a); }

// The refusals every entry shares.  up_front: the sizes are held against the handle's for every norm (the per-row entries);
// otherwise only the norms that need the frame workspace check them (check_rows in project_call).
static paa_status check_call(const paa_proj* h, const paa_params* prm, const ProjCall& c, bool up_front) {
    if (!h || !prm || !c.src || !c.dst) PAA_FAIL(PAA_ERR_ARG, "%s: null argument", c.who);
    if (c.rows < 1 || c.L < 2) PAA_FAIL(PAA_ERR_SIZE, "%s: rows=%d L=%d", c.who, c.rows, c.L);
    if (up_front && (c.rows > h->max_batch || c.L > h->max_len))
        PAA_FAIL(PAA_ERR_SIZE, "%s: rows=%d L=%d exceeds max_batch=%d / max_len=%d", c.who, c.rows, c.L, h->max_batch, h->max_len);
    if (prm->norm_type < PAA_NORM_L2 || prm->norm_type > PAA_NORM_MASKING) PAA_FAIL(PAA_ERR_BAD_NORM, "Unknown norm_type: %d", prm->norm_type);
    return PAA_OK;
}

// Grid of a scaling launch (k_apply_scale, k_spec_finish) over `groups` groups of n elements: one group spreads over up to 1024
// workgroups of per_wg elements each, several groups take up to 128 workgroups of 1024 elements per group.
static dim3 scale_grid(int groups, int64_t n, int per_wg) {
    return groups == 1 ? dim3(std::min(cdiv(n, per_wg), 1024)) : dim3(std::min(cdiv(n, (int64_t)RED_NT * 4), 128), groups);
}

template <class Args>
static void set_bin_params(Args& a, const paa_params* prm) {
    a.min_f = prm->min_freq_attack; a.max_f = prm->max_freq_attack; a.phon_ref = prm->phon_reference_db;
}

// The projection of a checked call (P0-P7 of DESIGN.md §1).  A group spans rows / groups rows: n elements of the perturbation, nc of
// the clean clips; its partial sums are laid out and summed as a call on that group alone lays them out and sums them.
static paa_status project_call(paa_proj* h, const paa_params* prm, const ProjCall& c, hipStream_t st) {
    const int nt = prm->norm_type, L = c.L, rows = c.rows, groups = c.groups;
    const bool in_place = c.src == c.dst;
    const int64_t all = (int64_t)rows * L, n = all / groups;
    if (nt == PAA_NORM_LINF) {
        if (c.rscale)
            hipLaunchKernelGGL(k_clamp_rows, dim3(std::min(cdiv((int64_t)L, 256), 256), rows), dim3(256), 0, st, c.src, c.dst, L,
                               prm->linf_size, c.rscale);
        else
            hipLaunchKernelGGL(k_clamp, dim3(std::min(cdiv(all, 256), 2048)), dim3(256), 0, st, c.src, c.dst, all, -prm->linf_size,
                               prm->linf_size);
        PAA_LAUNCH_CHECK();
        return PAA_OK;
    }
    if (nt == PAA_NORM_L2 || nt == PAA_NORM_SNR || nt == PAA_NORM_TV) {
        // the reduction and the scaling pass read the source directly
        if (nt != PAA_NORM_L2 && !c.ext && (!c.clean || c.B < 1)) {
            if (nt == PAA_NORM_SNR) PAA_FAIL(PAA_ERR_NEED_CLEAN, "SNR projection requires clean_audio ro compare to");
            PAA_FAIL(PAA_ERR_NEED_CLEAN, "TV projection can benefit from clean_audio for bounds");
        }
        const int64_t nc = (nt == PAA_NORM_L2 || c.ext) ? 0 : (int64_t)(c.B / groups) * L;
        const int g1 = nc ? std::min(cdiv(nc, (int64_t)RED_NT * 16), 2048) : 0;
        const int g2 = std::min(cdiv(n, (int64_t)RED_NT * 8), 1024);
        // one group's partials (at most 3072) fit below the frame partials of d_part; several groups' go to the frame workspace, idle for these norms
        double* part = groups == 1 ? h->d_part : reinterpret_cast<double*>(h->d_frames);
        if (groups > 1 && (size_t)groups * (g1 + g2) * 2 > h->frames_floats)
            PAA_FAIL(PAA_ERR_SIZE, "%s: rows=%d L=%d exceeds the workspace", c.who, rows, L);
        if (nt == PAA_NORM_TV)
            hipLaunchKernelGGL(k_reduce2<RED_TV>, dim3(g1 + g2, groups), dim3(RED_NT), 0, st, c.clean, nc, L, g1, c.src, n, L, g2, part);
        else
            hipLaunchKernelGGL(k_reduce2<RED_SQ>, dim3(g1 + g2, groups), dim3(RED_NT), 0, st, c.clean, nc, L, g1, c.src, n, L, g2, part);
        PAA_LAUNCH_CHECK();
        ApplyArgs a{};
        a.part = part; a.g1 = g1; a.g2 = g2; a.scal = h->d_scal;
        a.numel_clean = c.ext ? c.ext_numel : (double)nc; a.numel_p = (double)n; a.ext = c.ext;
        a.ext_clips = c.ext ? c.ext_clips : nullptr; a.clip_len = (double)L; a.rscale = c.rscale;
        a.snr_db = prm->snr_db; a.snr_linear = (float)pow(10.0, (double)prm->snr_db / 10.0);
        a.eps = (nt == PAA_NORM_L2) ? prm->l2_size : prm->tv_epsilon;
        const dim3 grid = scale_grid(groups, n, 256);
        if (nt == PAA_NORM_L2) hipLaunchKernelGGL(k_apply_scale<PAA_NORM_L2>, grid, dim3(RED_NT), 0, st, c.src, c.dst, n, a);
        else if (nt == PAA_NORM_SNR) hipLaunchKernelGGL(k_apply_scale<PAA_NORM_SNR>, grid, dim3(RED_NT), 0, st, c.src, c.dst, n, a);
        else hipLaunchKernelGGL(k_apply_scale<PAA_NORM_TV>, grid, dim3(RED_NT), 0, st, c.src, c.dst, n, a);
        PAA_LAUNCH_CHECK();
        return PAA_OK;
    }
    // the spectral norms: fletcher_munson, min_max_freqs, max_phon, masking
    PAA_TRY(check_rows(h, rows, L, c.who));
    const bool fm = nt == PAA_NORM_FLETCHER_MUNSON;
    const int T = 1 + L / h->hop;
    // masking: every clip's bound; one group hides under all of them (their minimum, left in row 0), a row of its own under its own clip's
    if (nt == PAA_NORM_MASKING) PAA_TRY(masking_pass(h, c.clean, c.B, L, prm->masking_margin_db, nullptr, nullptr, nullptr, groups == 1, st));
    if (fused_geometry(h)) {
        // one fused launch STFT -> per-bin op -> iSTFT + overlap-add (spec_kernels.hip), then the scale / copy-back launch
        SpecArgs a = spec_args(h, L, T, L);
        a.mask = h->d_mask; a.mask_rs = groups == 1 ? 0 : (int64_t)T * h->F;
        set_bin_params(a, prm);
        a.x = c.src; a.rscale = c.rscale;
        a.out = in_place ? h->d_frames : c.dst;                // in place: through the workspace (neighbouring workgroups re-read the halo)
        int npart = 0;
        PAA_TRY(spec_project(a, spec_op_of(nt), rows, &npart, st));
        if (fm || in_place) {
            const int fg = fm ? groups : 1;                    // a plain copy back has no statistic: one span over all the rows
            const int64_t fn = all / fg;
            hipLaunchKernelGGL(k_spec_finish, scale_grid(fg, fn, RED_NT * 4), dim3(RED_NT), 0, st, (const float*)a.out, c.dst, fn,
                               (const double*)a.part, fm ? npart / fg : 0, prm->fm_epsilon, h->d_scal, c.rscale);
            PAA_LAUNCH_CHECK();
        }
        return PAA_OK;
    }
    // the generic frame kernels work in place: copy first.  FM keeps the groups' scales as floats at the front of d_part, below the
    // frame partials
    if (fm && groups > 2 * MAX_PART) PAA_FAIL(PAA_ERR_SIZE, "%s: rows=%d exceeds %d", c.who, rows, 2 * MAX_PART);
    if (!in_place) PAA_HIP(hipMemcpyAsync(c.dst, c.src, sizeof(float) * all, hipMemcpyDeviceToDevice, st));
    FrameArgs a = frame_args(h, L, T);
    a.x = c.dst; a.rscale = c.rscale;
    set_bin_params(a, prm);
    float* gscale = nullptr;
    if (nt == PAA_NORM_MIN_MAX_FREQS) PAA_TRY(launch_frames<OP_MINMAX>(h, a, rows, st));
    else if (nt == PAA_NORM_MAX_PHON) PAA_TRY(launch_frames<OP_PHON>(h, a, rows, st));
    else {
        PAA_TRY(launch_frames<OP_FM>(h, a, rows, st));
        gscale = reinterpret_cast<float*>(h->d_part);
        hipLaunchKernelGGL(k_fm_finalize, dim3(1, groups), dim3(RED_NT), 0, st, (const double*)a.part, rows / groups * T,
                           prm->fm_epsilon, gscale, h->d_scal, c.rscale);
        PAA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_ola, dim3(cdiv(L, 256), rows), dim3(256), 0, st, h->d_frames, h->d_win, (const float*)gscale,
                       groups == 1 ? 0 : 1, c.dst, T, h->n_fft, h->hop, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_project(paa_proj* h, const paa_params* prm, float* d_p, int rows_p, const float* d_clean,
                                  int B, int L, void* stream) {
    const ProjCall c{"paa_project", d_p, d_p, rows_p, L, 1, d_clean, B};
    PAA_TRY(check_call(h, prm, c, false));
    return project_call(h, prm, c, (hipStream_t)stream);
}

extern "C" paa_status paa_project_to(paa_proj* h, const paa_params* prm, const float* d_src, float* d_dst, int rows_p,
                                     const float* d_clean, int B, int L, void* stream) {
    const ProjCall c{"paa_project_to", d_src, d_dst, rows_p, L, 1, d_clean, B};
    if (!d_src || !d_dst) PAA_FAIL(PAA_ERR_ARG, "paa_project_to: null argument");
    if (rows_p > 0 && L > 0 && overlap(d_src, d_dst, (int64_t)rows_p * L)) PAA_FAIL(PAA_ERR_ARG, "paa_project_to: source and destination overlap");
    PAA_TRY(check_call(h, prm, c, false));
    return project_call(h, prm, c, (hipStream_t)stream);
}

// Statistics of the clean clips from the device in place of the clips themselves (data-parallel runs): l2 / snr / tv
extern "C" paa_status paa_project_ext(paa_proj* h, const paa_params* prm, float* d_p, int rows_p, const float* d_clean_stats,
                                      const float* d_clip_count, double clean_numel, int L, void* stream) {
    if (prm && prm->norm_type == PAA_NORM_MASKING) PAA_FAIL(PAA_ERR_BAD_NORM, "paa_project_ext: the masking norm needs the clean clips (paa_project)");
    if (!d_clean_stats) PAA_FAIL(PAA_ERR_NEED_CLEAN, "paa_project_ext: clean statistics are required");
    if (!d_clip_count && !(clean_numel > 0.0)) PAA_FAIL(PAA_ERR_ARG, "paa_project_ext: neither a device clip count nor a positive clean_numel");
    const ProjCall c{"paa_project_ext", d_p, d_p, rows_p, L, 1, nullptr, 0, d_clean_stats, d_clip_count, clean_numel};
    PAA_TRY(check_call(h, prm, c, false));
    return project_call(h, prm, c, (hipStream_t)stream);
}

// Per-row form: every row is a group, clean clip r belongs to row r; no launch per row.  d_scale (nullable, device (rows)): the
// per-row bound scale of paa_project_rows_scaled; null is paa_project_rows.
static paa_status project_rows(paa_proj* h, const paa_params* prm, const float* d_src, float* d_dst, int rows, const float* d_clean,
                               int L, const float* d_scale, void* stream, const char* who) {
    const ProjCall c{who, d_src, d_dst, rows, L, rows, d_clean, rows, nullptr, nullptr, 0.0, d_scale};
    PAA_TRY(check_call(h, prm, c, true));
    if (d_src != d_dst && overlap(d_src, d_dst, (int64_t)rows * L)) PAA_FAIL(PAA_ERR_ARG, "%s: source and destination overlap", who);
    if (d_scale && prm->norm_type == PAA_NORM_MASKING)
        PAA_FAIL(PAA_ERR_BAD_NORM, "%s: the masking norm takes no bound scale (norm_type %d)", who, prm->norm_type);
    return project_call(h, prm, c, (hipStream_t)stream);
}

extern "C" paa_status paa_project_rows(paa_proj* h, const paa_params* prm, const float* d_src, float* d_dst, int rows,
                                       const float* d_clean, int L, void* stream) {
    return project_rows(h, prm, d_src, d_dst, rows, d_clean, L, nullptr, stream, "paa_project_rows");
}

extern "C" paa_status paa_project_rows_scaled(paa_proj* h, const paa_params* prm, const float* d_src, float* d_dst, int rows,
                                              const float* d_clean, int L, const float* d_scale, void* stream) {
    return project_rows(h, prm, d_src, d_dst, rows, d_clean, L, d_scale, stream, "paa_project_rows_scaled");
}

// core/projections.py:68-159 called directly on a spectrum (the reference's project_min_max_freqs / project_fm_norm /
// project_phon_level take the complex (B, F, T) STFT tensor): d_S_in, d_S_out (B, T, F) complex64 frame-major
// (in place allowed); prm->norm_type selects the op.  Works for any frame geometry (pure per-bin arithmetic).
extern "C" paa_status paa_spectrum_project(paa_proj* h, const paa_params* prm, const float* d_S_in, float* d_S_out, int B, int T,
                                           void* stream) {
    if (!h || !prm || !d_S_in || !d_S_out) PAA_FAIL(PAA_ERR_ARG, "paa_spectrum_project: null argument");
    if (B < 1 || T < 1) PAA_FAIL(PAA_ERR_SIZE, "paa_spectrum_project: B=%d T=%d", B, T);
    if (h->F != 513) PAA_FAIL(PAA_ERR_ARG, "paa_spectrum_project: n_fft=%d (only 1024 is built)", h->n_fft);
    const int nt = prm->norm_type;
    const int op = spec_op_of(nt);
    if (op == SOP_NONE || op == SOP_MASK) PAA_FAIL(PAA_ERR_BAD_NORM, "paa_spectrum_project: norm_type %d is not a frequency-domain projection", nt);
    hipStream_t st = (hipStream_t)stream;
    SpecArgs a = spec_args(h, 0, T, 0);
    a.part = h->d_part;
    set_bin_params(a, prm);
    a.S_in = d_S_in;
    if (op != SOP_FM) {
        a.S_out = d_S_out;
        return spec_apply(a, op, B, nullptr, nullptr, st);
    }
    int npart = 0;
    a.S_out = nullptr;                                       // pass 1: weighted power only
    PAA_TRY(spec_apply(a, SOP_FM, B, nullptr, &npart, st));
    hipLaunchKernelGGL(k_fm_finalize, dim3(1), dim3(RED_NT), 0, st, (const double*)a.part, npart, prm->fm_epsilon, h->d_scal, h->d_scal,
                       (const float*)nullptr);
    PAA_LAUNCH_CHECK();
    a.S_out = d_S_out; a.part = nullptr;                     // pass 2: S * predicated scale
    return spec_apply(a, SOP_NONE, B, h->d_scal, nullptr, st);
}

// The masking threshold of the clean clips d_clean (B, L): theta (B, T, F) dB, optionally P - Pmax + 96 (B, T, F) and Pmax (B).
// Masking-threshold loss: passes 1 and 2 leave every clip's bound A_b in h->d_mask and Pmax_b in the idle frame
// workspace, then ONE fused launch (k_spec_mloss) and the loss partials' finishing launch.  Frame workspace: [B x parts doubles:
// loss partials | B doubles: finishing scratch | B floats: Pmax].
// alpha_rows = 1: one weight (d_alpha [1], NULL = 1.0), paa_masking_loss itself; alpha_rows = p_rows = B: row b's own weight.
static paa_status masking_loss_entry(paa_proj* h, const paa_params* prm, const float* d_p, int p_rows, const float* d_clean, int B, int L,
                                     const float* d_alpha, int alpha_rows, float* d_grad, float* d_loss_rows, float* d_loss_sum,
                                     float* d_weight, void* stream, const char* who) {
    if (!h || !prm || !d_p) PAA_FAIL(PAA_ERR_ARG, "%s: null argument", who);
    if (!d_clean || B < 1) PAA_FAIL(PAA_ERR_NEED_CLEAN, "the masking loss requires clean_audio");
    if (p_rows != 1 && p_rows != B) PAA_FAIL(PAA_ERR_ARG, "%s: p_rows=%d must be 1 or B=%d", who, p_rows, B);
    if (alpha_rows != 1 && !(alpha_rows == B && p_rows == B))
        PAA_FAIL(PAA_ERR_ARG, "%s: alpha_rows=%d must be 1, or B=%d with p_rows=B (p_rows=%d)", who, alpha_rows, B, p_rows);
    if (alpha_rows != 1 && !d_alpha) PAA_FAIL(PAA_ERR_ARG, "%s: alpha_rows=%d needs d_alpha", who, alpha_rows);
    hipStream_t st = (hipStream_t)stream;
    const int T = 1 + L / h->hop;
    const int parts = spec_mloss_parts(T);
    double* lpart = reinterpret_cast<double*>(h->d_frames);
    double* scratch = lpart + (size_t)B * parts;
    float* pmax = reinterpret_cast<float*>(scratch + B);
    if (B <= h->max_batch && ((size_t)B * (parts + 1)) * 2 + B > h->frames_floats)
        PAA_FAIL(PAA_ERR_SIZE, "%s: workspace too small", who);
    PAA_TRY(masking_pass(h, d_clean, B, L, prm->masking_margin_db, nullptr, nullptr, pmax, false, st));
    SpecArgs a = spec_args(h, L, T, L);
    a.x = d_p; a.mask = h->d_mask; a.mask_rs = (int64_t)T * h->F;
    a.pmax = pmax; a.alpha = d_alpha; a.alpha_rs = alpha_rows == 1 ? 0 : 1; a.grad = d_grad; a.wout = d_weight; a.lpart = lpart;
    a.nclip = p_rows == 1 ? B : 1; a.per_clip = p_rows == 1 ? 0 : 1; a.lstride = parts;
    PAA_TRY(spec_mloss(a, p_rows, st));
    if (d_loss_rows || d_loss_sum) PAA_TRY(spec_mloss_finish(lpart, parts, B, scratch, d_loss_rows, d_loss_sum, st));
    return PAA_OK;
}

extern "C" paa_status paa_masking_loss_rows(paa_proj* h, const paa_params* prm, const float* d_p, int p_rows, const float* d_clean,
                                            int B, int L, const float* d_alpha, int alpha_rows, float* d_grad, float* d_loss_rows,
                                            float* d_loss_sum, float* d_weight, void* stream) {
    return masking_loss_entry(h, prm, d_p, p_rows, d_clean, B, L, d_alpha, alpha_rows, d_grad, d_loss_rows, d_loss_sum, d_weight, stream,
                              "paa_masking_loss_rows");
}

extern "C" paa_status paa_masking_loss(paa_proj* h, const paa_params* prm, const float* d_p, int p_rows, const float* d_clean, int B,
                                       int L, const float* d_alpha, float* d_grad, float* d_loss_rows, float* d_loss_sum,
                                       float* d_weight, void* stream) {
    return masking_loss_entry(h, prm, d_p, p_rows, d_clean, B, L, d_alpha, 1, d_grad, d_loss_rows, d_loss_sum, d_weight, stream,
                              "paa_masking_loss");
}

extern "C" paa_status paa_masking_threshold(paa_proj* h, const float* d_clean, int B, int L, float* d_psd, float* d_theta,
                                            float* d_pmax, void* stream) {
    if (!h || !d_theta) PAA_FAIL(PAA_ERR_ARG, "paa_masking_threshold: null argument");
    return masking_pass(h, d_clean, B, L, 0.f, d_psd, d_theta, d_pmax, false, (hipStream_t)stream);
}

// core/projections.py:83-113 compute_fm_weighted_norm_interp: sqrt(sum |S|^2 w(10 log10(|S|^2 + 1e-10), f)) -> d_out[0]
extern "C" paa_status paa_fm_weighted_norm(paa_proj* h, const float* d_S, int B, int T, float* d_out, void* stream) {
    if (!h || !d_S || !d_out) PAA_FAIL(PAA_ERR_ARG, "paa_fm_weighted_norm: null argument");
    if (B < 1 || T < 1) PAA_FAIL(PAA_ERR_SIZE, "paa_fm_weighted_norm: B=%d T=%d", B, T);
    if (h->F != 513) PAA_FAIL(PAA_ERR_ARG, "paa_fm_weighted_norm: n_fft=%d (only 1024 is built)", h->n_fft);
    hipStream_t st = (hipStream_t)stream;
    SpecArgs a = spec_args(h, 0, T, 0);
    a.part = h->d_part;
    a.S_in = d_S; a.S_out = nullptr;
    int npart = 0;
    PAA_TRY(spec_apply(a, SOP_FM, B, nullptr, &npart, st));
    hipLaunchKernelGGL(k_fm_finalize, dim3(1), dim3(RED_NT), 0, st, (const double*)a.part, npart, 0.f, h->d_scal, h->d_scal,
                       (const float*)nullptr);
    PAA_LAUNCH_CHECK();
    PAA_HIP(hipMemcpyAsync(d_out, h->d_scal + 1, sizeof(float), hipMemcpyDeviceToDevice, st));
    return PAA_OK;
}

namespace paa {
__global__ __launch_bounds__(RED_NT) void k_sum_parts(const double* __restrict__ part, int g1, int g2, float* __restrict__ out,
                                                      float* __restrict__ count_out, float count) {
    __shared__ double red[RED_NT / 64];
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < g1; i += RED_NT) s1 += part[i];
    for (int i = threadIdx.x; i < g2; i += RED_NT) s2 += part[g1 + i];
    s1 = block_sum<double, RED_NT>(s1, red);
    s2 = block_sum<double, RED_NT>(s2, red);
    if (threadIdx.x == 0) { out[0] = (float)s1; out[1] = (float)s2; if (count_out) count_out[0] = count; }
}
}  // namespace paa

extern "C" paa_status paa_batch_stats(paa_proj* h, const float* d_clean, int B, int L, float* d_out2, float* d_clip_count,
                                      void* stream) {
    if (!h || !d_clean || !d_out2) PAA_FAIL(PAA_ERR_ARG, "paa_batch_stats: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nc = (int64_t)B * L;
    const int g = std::min(cdiv(nc, (int64_t)RED_NT * 16), 2048);
    hipLaunchKernelGGL(k_reduce2<RED_SQ>, dim3(g), dim3(RED_NT), 0, st, d_clean, nc, L, g, (const float*)nullptr, (int64_t)0, L, 0,
                       h->d_part);
    PAA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_reduce2<RED_TV>, dim3(g), dim3(RED_NT), 0, st, d_clean, nc, L, g, (const float*)nullptr, (int64_t)0, L, 0,
                       h->d_part + g);
    PAA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sum_parts, dim3(1), dim3(RED_NT), 0, st, (const double*)h->d_part, g, g, d_out2, d_clip_count, (float)B);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_sign_step(float* d_p, const float* d_grad, float lr, int L, void* stream) {
    if (!d_p || !d_grad) PAA_FAIL(PAA_ERR_ARG, "paa_sign_step: null argument");
    hipLaunchKernelGGL(k_sign_step, dim3(cdiv(L, 256)), dim3(256), 0, (hipStream_t)stream, d_p, d_grad, lr, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_adam_step(float* d_p, const float* d_grad, float grad_sign, float* d_exp_avg, float* d_exp_avg_sq,
                                    const float* d_scal, float w1, float beta2, float omb2, float eps, float* d_grad_out, int L,
                                    void* stream) {
    if (!d_p || !d_grad || !d_exp_avg || !d_exp_avg_sq || !d_scal) PAA_FAIL(PAA_ERR_ARG, "paa_adam_step: null argument");
    if (L < 1) PAA_FAIL(PAA_ERR_SIZE, "paa_adam_step: L=%d", L);
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_p) | reinterpret_cast<uintptr_t>(d_grad) |
                        reinterpret_cast<uintptr_t>(d_exp_avg) | reinterpret_cast<uintptr_t>(d_exp_avg_sq) |
                        reinterpret_cast<uintptr_t>(d_grad_out);
    const int vec = (a & 15) == 0;
    const int threads = vec ? std::max(L >> 2, 1) : L;
    hipLaunchKernelGGL(k_adam_step, dim3(cdiv(threads, 256)), dim3(256), 0, (hipStream_t)stream, d_p, d_grad, grad_sign,
                       d_exp_avg, d_exp_avg_sq, d_scal, w1, beta2, omb2, eps, d_grad_out, L, vec);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

// core/projections.py:37-39 project_linf(p, min_val, max_val) with an arbitrary box (the dispatcher passes +-linf_size).
extern "C" paa_status paa_clamp(float* d_p, int64_t n, float lo, float hi, void* stream) {
    if (!d_p) PAA_FAIL(PAA_ERR_ARG, "paa_clamp: null argument");
    if (n < 1) PAA_FAIL(PAA_ERR_SIZE, "paa_clamp: n=%lld", (long long)n);
    // lo > hi: every element becomes hi, as torch.clamp documents (min(max(x, lo), hi))
    hipLaunchKernelGGL(k_clamp, dim3(std::min(cdiv(n, 256), 2048)), dim3(256), 0, (hipStream_t)stream, (const float*)d_p, d_p, n, lo, hi);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_compose_clamp(const float* d_clean, const float* d_p, float* d_out, int B, int L, void* stream) {
    if (!d_clean || !d_p || !d_out) PAA_FAIL(PAA_ERR_ARG, "paa_compose_clamp: null argument");
    hipLaunchKernelGGL(k_compose_clamp, dim3(std::min(cdiv((int64_t)B * L, 256), 4096)), dim3(256), 0, (hipStream_t)stream,
                       d_clean, d_p, d_out, B, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

// train.py:136 with one perturbation row per clip: out[b] = clamp(clean[b] + p[b], -1, 1).  p_rows = 1 is paa_compose_clamp.
extern "C" paa_status paa_compose_clamp_rows(const float* d_clean, const float* d_p, int p_rows, float* d_out, int B, int L,
                                             void* stream) {
    if (!d_clean || !d_p || !d_out) PAA_FAIL(PAA_ERR_ARG, "paa_compose_clamp_rows: null argument");
    if (B < 1 || L < 1) PAA_FAIL(PAA_ERR_SIZE, "paa_compose_clamp_rows: B=%d L=%d", B, L);
    if (p_rows != 1 && p_rows != B) PAA_FAIL(PAA_ERR_SIZE, "paa_compose_clamp_rows: p_rows=%d must be 1 or B=%d", p_rows, B);
    if (p_rows == 1) return paa_compose_clamp(d_clean, d_p, d_out, B, L, stream);
    const int64_t n = (int64_t)B * L;
    hipLaunchKernelGGL(k_compose_clamp_rows, dim3(std::min(cdiv(n, 256), 4096)), dim3(256), 0, (hipStream_t)stream, d_clean, d_p,
                       d_out, n);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}
