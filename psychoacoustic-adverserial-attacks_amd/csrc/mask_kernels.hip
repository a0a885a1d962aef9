// Clean-signal masking threshold for gfx950 (the masking norm).  Default frame geometry only (n_fft = 1024,
// hop = 256, F = 513 bins).  Three passes over a (rows, T, F) f32 workspace:
//
//  1. k_spec_psd (spec_kernels.hip): the wave-per-frame STFT with a level epilogue, P = 10 log10(|X|^2 + 1e-20), plus one
//     maximum per workgroup.
//  2. k_mask_threshold (here): ONE WAVE PER FRAME.  The row maximum Pmax is the maximum of pass 1's partials (order-free).  The
//     frame's normalised levels P - Pmax + 96 go to LDS; a lane owns bins lane + 64 j (j < 8) and lane 0 also bin 512.
//     Candidates are strict local maxima; their tonal level P_TM sums the three neighbours' powers.  Candidates under the
//     threshold in quiet are dropped, and a candidate survives unless a louder one (or an equal one at a lower bin) lies within
//     0.5 Bark ([lo_k, hi_k], host table): an order-free non-maximum suppression.  Survivors are at least 0.5 Bark apart, so at
//     most 53 at any sample rate; __ballot + mbcnt compact them into an LDS list in ascending bin order.  Each lane then sums
//     10^(T_j(i) / 10) over that list in that order (hardware exp2 / log2), plus the ATH term, relative to a per-bin offset so
//     that neither the loud end nor the 27 dB / Bark tails leave the f32 range.  Writes theta (dB) or the magnitude bound
//     A = 10^((theta + margin - 96 + Pmax) / 20); in place over P when called from a projection.
//  2b. k_mask_spread (temporal masking; only when paa_proj_set_masking_spread gave tables): pass 2 then writes
//     theta into a second plane, and this pass spreads it along time (post- and pre-masking) into theta' or the bound A'.
//  3. k_mask_min (universal perturbation only): A[0] = min over the clips.
//
// Deterministic: no atomics, every sum in a fixed order; results are written with vector stores.
#include <math.h>

#include <algorithm>

#include "mask_kernels.h"

namespace paa {

namespace {

constexpr int F = 513, MW = 4, MAXM = 64;
constexpr float C10 = 0.332192809488736235f;     // log2(10) / 10:  10^(x / 10) = exp2(x C10)
constexpr float DB = 3.01029995663981195f;       // 10 log10(2):    10 log10(s) = DB log2(s)
constexpr float NOATH = 88.f;                    // bins below kA: the sum is taken as s 2^-88 (no overflow below 2^127)

__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float lg2(float x) { return __builtin_amdgcn_logf(x); }

// grid: (ceil(T / MW), rows), MW waves, one frame each; no workgroup barrier (the waves share nothing)
__global__ __launch_bounds__(MW * 64) void k_mask_threshold(MaskArgs a) {
    __shared__ float pl[MW][F + 3];                  // P - Pmax + 96 of the wave's frame
    __shared__ float tl[MW][F + 3];                  // P_TM of the remaining candidates, -inf elsewhere
    __shared__ float4 ml[MW][MAXM];                  // survivors: z_j, (P_TM - 6.025 - 0.275 z_j) C10, 27 C10, upper slope C10
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = blockIdx.y, t = blockIdx.x * MW + wave;
    float pm = -INFINITY;
    for (int i = lane; i < a.nparts; i += 64) pm = fmaxf(pm, a.part[(size_t)row * a.nparts + i]);
    pm = wave_max(pm);
    if (t >= a.T) return;
    if (a.pmax && t == 0 && lane == 0) a.pmax[row] = pm;
    const size_t off = ((size_t)row * a.T + t) * F;
    float* P = pl[wave];
    float* M = tl[wave];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int k = lane + 64 * j;
        if (k < F) {
            const float v = (a.P[off + k] - pm) + 96.f;
            P[k] = v;
            if (a.psd) a.psd[off + k] = v;
        }
    }
    wave_fence();
    // candidates (1 <= k <= F - 2: j < 8) and their tonal level; below the threshold in quiet they are dropped
    float tm[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = lane + 64 * j;
        float v = -INFINITY;
        if (k >= 1) {
            const float l = P[k - 1], c = P[k], r = P[k + 1];
            if (c > l && c > r) {
                const float ptm = DB * lg2(ex2(l * C10) + ex2(c * C10) + ex2(r * C10));
                if (!(ptm < a.tab.quiet[k])) v = ptm;
            }
        }
        tm[j] = v;
        M[k] = v;
    }
    if (lane == 0) M[F - 1] = -INFINITY;
    wave_fence();
    // order-free suppression: k survives unless a remaining candidate within 0.5 Bark is louder, or as loud at a lower bin
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = lane + 64 * j;
        if (tm[j] > -INFINITY) {
            const int w = a.tab.win[k];
            const int lo = w & 0xffff, hi = w >> 16;
            bool s = true;
            for (int i = lo; i <= hi; ++i) {
                const float v = M[i];
                if (v > tm[j] || (v == tm[j] && i < k)) { s = false; break; }
            }
            keep |= (s ? 1u : 0u) << j;
        }
    }
    // compaction in ascending bin order (bin = lane + 64 j: j major, lane minor)
    int n = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool s = (keep >> j) & 1u;
        const unsigned long long b = __ballot(s);
        if (s) {
            const int pos = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
            if (pos < MAXM) {
                const float zj = a.tab.z[lane + 64 * j];
                ml[wave][pos] = make_float4(zj, (tm[j] - 6.025f - 0.275f * zj) * C10, 27.f * C10,
                                            (-27.f + 0.37f * fmaxf(tm[j] - 40.f, 0.f)) * C10);
            }
        }
        n += __popcll(b);
    }
    n = n < MAXM ? n : MAXM;
    wave_fence();
    // global threshold of the lane's bins: survivors in list order, then the ATH term
    const float c = a.margin - 96.f + pm;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int k = lane + 64 * j;
        if (k < F) {
            const float zi = a.tab.z[k];
            const bool ath = k >= a.tab.kA;
            const float o = ath ? a.tab.ath[k] * C10 : -NOATH;       // per-bin offset, in log2 units
            float s = 0.f;
            for (int m = 0; m < n; ++m) {
                const float4 q = ml[wave][m];
                const float dz = zi - q.x;
                s += ex2(fmaf(dz <= 0.f ? q.z : q.w, dz, q.y) - o);
            }
            if (ath) s += 1.f;
            const float theta = (lg2(s) + o) * DB;                   // -inf when s = 0
            a.out[off + k] = a.bound ? ex2((theta + c) * (0.5f * C10)) : theta;
        }
    }
}

// Temporal masking between passes 2 and 3.  grid: (ceil(T / ST), rows); a workgroup owns ST frames of one row and reads
// its halo of n_post frames before and n_pre after from the theta plane, which is why the result goes to another plane.  A wave takes
// units of 64 bins x SR frames: lanes along bins (dword accesses, coalesced), the SR running maxima in registers; every theta frame
// of the unit's window is loaded once and meets all SR output frames.  The decrements sit in LDS indexed by the signed lag d = t - s,
// 0 at d = 0 and +inf outside the two tables, so a term out of the window is -inf and the inner loop has no branch; the index is
// uniform over the wave (a broadcast read).  Frames outside [0, T) are never loaded (T < J included), frames >= T never stored.
constexpr int ST = 32, SR = 8, SOFF = SR - 1 + MASK_LAGS, SWN = 2 * SOFF + 1, SCH = (F + 63) / 64;
__global__ __launch_bounds__(256) void k_mask_spread(MaskSpreadArgs a) {
    __shared__ float wl[SWN];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < SWN) {
        const int d = (int)threadIdx.x - SOFF;                        // frames from the masker to the masked frame
        float w = INFINITY;
        if (d == 0) w = 0.f;
        else if (d > 0 && d <= a.n_post) w = a.post[d - 1];
        else if (d < 0 && -d <= a.n_pre) w = a.pre[-d - 1];
        wl[threadIdx.x] = w;
    }
    __syncthreads();
    const int row = blockIdx.y, tile0 = blockIdx.x * ST;
    const float* __restrict__ in = a.theta + (size_t)row * a.T * F;
    float* __restrict__ out = a.out + (size_t)row * a.T * F;
    const float c = a.bound ? a.margin - 96.f + a.pmax[row] : 0.f;
    for (int u = wave; u < SCH * (ST / SR); u += 4) {
        const int t0 = tile0 + (u / SCH) * SR, k = (u % SCH) * 64 + lane;
        if (t0 >= a.T) break;
        const bool live = k < F;                                      // the last chunk holds bin 512 only
        float acc[SR];
#pragma unroll
        for (int r = 0; r < SR; ++r) acc[r] = -INFINITY;
        const int s0 = max(t0 - a.n_post, 0), s1 = min(t0 + SR - 1 + a.n_pre, a.T - 1);
#pragma unroll 4
        for (int s = s0; s <= s1; ++s) {
            const float v = live ? in[(size_t)s * F + k] : -INFINITY;
            const float* w = wl + (t0 - s + SOFF);                    // w[r]: the decrement at lag (t0 + r) - s
#pragma unroll
            for (int r = 0; r < SR; ++r) acc[r] = fmaxf(acc[r], v - w[r]);
        }
#pragma unroll
        for (int r = 0; r < SR; ++r)
            if (live && t0 + r < a.T) out[(size_t)(t0 + r) * F + k] = a.bound ? ex2((acc[r] + c) * (0.5f * C10)) : acc[r];
    }
}

__global__ __launch_bounds__(256) void k_mask_min(float* __restrict__ A, int rows, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float v = A[i];
        for (int r = 1; r < rows; ++r) v = fminf(v, A[(size_t)r * n + i]);
        A[i] = v;
    }
}

}  // namespace

void mask_tables(int sr, float* z, float* quiet, float* ath, int* win, int* kA) {
    double zd[F];
    int ka = F;
    for (int k = 0; k < F; ++k) {
        const double f = (double)k * (double)sr / 1024.0;
        zd[k] = 13.0 * atan(0.00076 * f) + 3.5 * atan((f / 7500.0) * (f / 7500.0));
        const double fk = f / 1000.0;
        const double q = 3.64 * pow(fk, -0.8) - 6.5 * exp(-0.6 * (fk - 3.3) * (fk - 3.3)) + 1e-3 * fk * fk * fk * fk - 12.0;
        z[k] = (float)zd[k];
        quiet[k] = (float)q;                                         // +inf at k = 0 (never a candidate)
        if (ka == F && zd[k] > 1.0) ka = k;
        ath[k] = k >= ka ? (float)q : 0.f;
    }
    for (int k = 0; k < F; ++k) {
        int lo = k, hi = k;
        while (lo > 0 && fabs(zd[lo - 1] - zd[k]) < 0.5) --lo;
        while (hi < F - 1 && fabs(zd[hi + 1] - zd[k]) < 0.5) ++hi;
        win[k] = lo | (hi << 16);
    }
    *kA = ka;
}

paa_status mask_threshold(const MaskArgs& a, int rows, hipStream_t st) {
    hipLaunchKernelGGL(k_mask_threshold, dim3(cdiv(a.T, MW), rows), dim3(MW * 64), 0, st, a);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

paa_status mask_spread(const MaskSpreadArgs& a, int rows, hipStream_t st) {
    hipLaunchKernelGGL(k_mask_spread, dim3(cdiv(a.T, ST), rows), dim3(256), 0, st, a);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

paa_status mask_min_rows(float* A, int rows, int64_t n, hipStream_t st) {
    if (rows < 2) return PAA_OK;
    hipLaunchKernelGGL(k_mask_min, dim3(std::min(cdiv(n, 256), 2048)), dim3(256), 0, st, A, rows, n);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

}  // namespace paa
