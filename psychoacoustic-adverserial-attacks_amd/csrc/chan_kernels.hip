// The playback channel on the placement layer: sample-clock drift of the emitter and ambient noise at the
// microphone.
//
// Drift (paa_drift_apply).  Clip b is resampled by the ratio r_b = rq_b / 2^32 (unsigned Q32, clamped to [2^31, 2^33]) with a
// 16-tap Hann-windowed sinc, T = 8; the output keeps the length L and samples outside [0, L) are zeros:
//     pos_q = i * rq_b (64-bit, exact),  n = pos_q >> 32,  f = (pos_q & 0xffffffff) * 2^-32
//     y[b][i]  = sum_{t = -T+1 .. T} w(t - f) * x[b][n + t]                                  (adjoint = 0)
//     gx[b][j] = sum_{i : n_i in [j - T, j + T - 1]} w(j - n_i - f_i) * g[b][i]              (adjoint = 1: the exact transpose)
//     w(u) = sinc(u) * (1 + cos(pi u / T)) / 2 for |u| < T, else 0;  sinc(0) = 1
// Both directions take their weights from ONE device function (drift_w) whose roundings are spelled out, so the adjoint is the
// transpose of the very matrix the forward applies.  sin(pi (t - f)) = -(-1)^t sin(pi f): one sinpif per output, and an exact
// zero at f = 0, where the weights are {1, 0, ...} and y = x bit for bit (rq = 2^32).  No band-limiting for r > 1.
// The forward is one f32 fmaf chain, t ascending; the adjoint one f64 sum, i ascending, rounded once: every output is owned by
// one thread, no atomics, two calls give the same bits.  Both are single passes over B * L floats: a thread writes DRIFT_PER_THREAD
// outputs a block-width apart (as k_place_rows), and the 16-tap windows of neighbouring outputs, which overlap almost
// completely, are served by the cache.
//
// Noise (paa_noise_add).  rows[b][i] += sigma_b * z_{b,i}, sigma_b = sqrt(mean_i clean[b][i]^2) * 10^(-snr_b / 20) (f64 sum in a
// fixed order), z a standard normal by Box-Muller on the noise stream of philox.h (its stream table; normal_pair).  Word pair
// (c[2p], c[2p+1]), p = (i & 3) >> 1, of the block of group i >> 2 gives
//     u1 = ((c[2p] >> 8) + 1) * 2^-24 in (0, 1],  u2 = (c[2p+1] >> 8) * 2^-24 in [0, 1),  rad = sqrt(-2 ln u1)
//     z = rad * cos(2 pi u2) for even i, rad * sin(2 pi u2) for odd i.
//
// Draw (paa_chan_draw).  The channel stream of philox.h:  rq_b = 2^32 + ((((int64) c0 - 2^31) * D) >> 31)  (pure integers, draw_rq),
// snr_b = fmaf((c1 >> 8) * 2^-24, hi - lo, lo)  (draw_snr).
#include "paa_common.h"
#include "philox.h"

using namespace paa;

namespace {

constexpr int CHAN_NT = 256;            // threads per block of the drift and the noise kernels
constexpr int DRIFT_PER_THREAD = 4;     // outputs per thread of both drift directions: a block covers 1024 consecutive samples
constexpr int DRIFT_T = 8;              // half width of the window: taps t = -T+1 .. T
constexpr uint64_t RQ_MIN = 1ull << 31, RQ_MAX = 1ull << 33;

__device__ __forceinline__ uint64_t clamp_rq(uint64_t rq) { return rq < RQ_MIN ? RQ_MIN : (rq > RQ_MAX ? RQ_MAX : rq); }

// f of the operator as a float: the 32 fraction bits rounded to 24 (it may round up to 1.0f, which drift_w takes like any other)
__device__ __forceinline__ float frac_of(uint64_t pos_q) { return (float)(uint32_t)pos_q * 0x1p-32f; }

// w(t - f) as a float32, s = sinpif(f):  u = fl32(t - f);  1 at u = 0, 0 at |u| >= T;  else the two float32 transcendentals s and
// cospif(u / 8) combined in float64 (every product there is exact or rounds far below float32) and rounded ONCE,
//     w = fl32( +-s * (0.5 + 0.5 cospi(u / 8)) / (pi u) ).
// Three roundings in all: |w - exact| <= 2.25 * 2^-24 with correctly rounded sinpif / cospif (1.64 * 2^-24 measured on the
// host); a float32 combine has five and was measured at 3.6.  One function, so the forward and the adjoint hold the same bits.
__device__ __forceinline__ float drift_w(int t, float f, float s) {
    const float u = __fsub_rn((float)t, f);
    if (u == 0.0f) return 1.0f;
    if (!(fabsf(u) < (float)DRIFT_T)) return 0.0f;
    const double c = 0.5 + 0.5 * (double)cospif(u * 0.125f);
    const double num = (double)((t & 1) ? s : -s);                       // sin(pi (t - f)) = -(-1)^t sin(pi f)
    return (float)((num * c) / (3.14159265358979323846 * (double)u));
}

// grid (tiles of CHAN_NT * DRIFT_PER_THREAD outputs, clips); thread t of a tile writes outputs tile0 + t + k * CHAN_NT
__global__ void __launch_bounds__(CHAN_NT) k_drift_apply(const uint64_t* __restrict__ rq, const float* __restrict__ in,
                                                         float* __restrict__ out, int B, int L) {
    const int64_t tile0 = (int64_t)blockIdx.x * (CHAN_NT * DRIFT_PER_THREAD);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const uint64_t r = clamp_rq(rq[b]);
        const float* __restrict__ x = in + (int64_t)b * L;
        float* __restrict__ y = out + (int64_t)b * L;
#pragma unroll
        for (int k = 0; k < DRIFT_PER_THREAD; ++k) {
            const int64_t i = tile0 + threadIdx.x + k * CHAN_NT;
            if (i >= L) break;
            const uint64_t pos = (uint64_t)i * r;                        // i < 2^31, r <= 2^33: no overflow
            const int64_t n = (int64_t)(pos >> 32);
            float acc = 0.0f;
            if ((uint32_t)pos == 0u) {                                   // f = 0: the weights are exactly {1, 0, ...}
                if (n < L) acc = x[n];
            } else if (n - (DRIFT_T - 1) < L) {                          // else every tap reads a zero
                const float f = frac_of(pos);
                const float s = sinpif(f);
#pragma unroll
                for (int t = -DRIFT_T + 1; t <= DRIFT_T; ++t) {
                    const int64_t j = n + t;
                    const float v = x[min(max(j, (int64_t)0), (int64_t)L - 1)];      // a clamped (valid) address, then the zero
                    acc = fmaf(drift_w(t, f, s), (j >= 0 && j < L) ? v : 0.0f, acc);
                }
            }
            y[i] = acc;
        }
    }
}

// the transpose as a gather: output j collects the inputs i whose window [n_i - T + 1, n_i + T] holds j, i ascending
__global__ void __launch_bounds__(CHAN_NT) k_drift_adjoint(const uint64_t* __restrict__ rq, const float* __restrict__ g,
                                                           float* __restrict__ out, int B, int L) {
    const int64_t tile0 = (int64_t)blockIdx.x * (CHAN_NT * DRIFT_PER_THREAD);
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const uint64_t r = clamp_rq(rq[b]);
        const float* __restrict__ gb = g + (int64_t)b * L;
        float* __restrict__ y = out + (int64_t)b * L;
#pragma unroll
        for (int k = 0; k < DRIFT_PER_THREAD; ++k) {
            const int64_t j = tile0 + threadIdx.x + k * CHAN_NT;
            if (j >= L) break;
            // the first i with n_i >= j - T:  i * r >= (j - T) 2^32  (one 64-bit division; (j - T) 2^32 + r < 2^64)
            const int64_t lo = j - DRIFT_T;
            int64_t i = lo <= 0 ? 0 : (int64_t)((((uint64_t)lo << 32) + r - 1) / r);
            double acc = 0.0;
            for (; i < L; ++i) {                                         // at most 2 T 2^32 / r + 1 <= 33 candidates
                const uint64_t pos = (uint64_t)i * r;
                const int64_t n = (int64_t)(pos >> 32);
                if (n > j + DRIFT_T - 1) break;
                const float gv = gb[i];
                float w;
                if ((uint32_t)pos == 0u) {
                    w = n == j ? 1.0f : 0.0f;
                } else {
                    const float f = frac_of(pos);
                    w = drift_w((int)(j - n), f, sinpif(f));
                }
                acc += (double)w * (double)gv;                           // exact products, f64 sum, one rounding at the end
            }
            y[j] = (float)acc;
        }
    }
}

__global__ void __launch_bounds__(DRAW_NT) k_chan_draw(uint32_t k0, uint32_t k1, int32_t* __restrict__ counter, int stream_id,
                                                       int clip_base, int B, uint32_t drift_q32, float snr_lo, float snr_hi,
                                                       uint64_t* __restrict__ rq, float* __restrict__ snr) {
    draw_clips(k0, k1, counter, stream_id, clip_base, B, TAG_CHAN, [=](int b, const uint32_t (&c)[4]) {
        rq[b] = draw_rq(c[0], drift_q32);
        snr[b] = draw_snr(c[1], snr_lo, snr_hi);
    });
}

// one block per clip: sigma_b.  The per-thread partial sums (i = tid, tid + 256, ...) and their reduction have a fixed order.
// Block 0 alone touches the counter, after reading it: the add that follows reads step = *counter - 1 and writes nothing to it.
__global__ void __launch_bounds__(CHAN_NT) k_noise_sigma(int32_t* __restrict__ counter, const float* __restrict__ clean,
                                                         const float* __restrict__ snr, float* __restrict__ sigma, int B, int L) {
    __shared__ double sm[CHAN_NT / 64];
    const int b = blockIdx.x;
    const float* __restrict__ x = clean + (int64_t)b * L;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < L; i += CHAN_NT) {
        const double v = (double)x[i];
        acc = fma(v, v, acc);
    }
    const double sum = block_sum<double, CHAN_NT>(acc, sm);
    if (threadIdx.x == 0) {
        sigma[b] = (float)(sqrt(sum / (double)L) * pow(10.0, (double)snr[b] * -0.05));
        if (b == 0) {
            const uint32_t step = (uint32_t)*counter;
            *counter = (int32_t)(step + 1u);
        }
    }
}

// grid (blocks of CHAN_NT groups of four samples, clips): a thread draws one Philox block and adds its four normals
__global__ void __launch_bounds__(CHAN_NT) k_noise_add(uint32_t k0, uint32_t k1, const int32_t* __restrict__ counter, int stream_id,
                                                       int clip_base, const float* __restrict__ sigma, float* __restrict__ rows,
                                                       int B, int L) {
    const uint32_t step = (uint32_t)*counter - 1u;                       // k_noise_sigma has advanced it
    const int64_t grp = (int64_t)blockIdx.x * CHAN_NT + threadIdx.x;
    const int64_t i0 = grp * 4;
    if (i0 >= L) return;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float sg = sigma[b];
        if (sg == 0.0f) continue;                                        // a silent clip: its rows keep their bits
        uint32_t c[4];
        noise_counter(c, step, (uint32_t)(clip_base + b), (uint32_t)grp, (uint32_t)stream_id);
        philox4x32_10(c, k0, noise_k1(k1));
        float* __restrict__ y = rows + (int64_t)b * L + i0;
        const int m = (int)min((int64_t)4, (int64_t)L - i0);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float z_even, z_odd;
            normal_pair(c[2 * p], c[2 * p + 1], z_even, z_odd);
            if (2 * p < m) y[2 * p] = fmaf(sg, z_even, y[2 * p]);
            if (2 * p + 1 < m) y[2 * p + 1] = fmaf(sg, z_odd, y[2 * p + 1]);
        }
    }
}

}  // namespace

extern "C" paa_status paa_chan_draw(uint64_t seed, int32_t* d_counter, int stream_id, int clip_base, int B, uint32_t drift_q32,
                                    float snr_lo_db, float snr_hi_db, uint64_t* d_rq, float* d_snr_db, void* stream) {
    if (!d_counter || !d_rq || !d_snr_db) PAA_FAIL(PAA_ERR_ARG, "paa_chan_draw: null argument");
    if (B < 1) PAA_FAIL(PAA_ERR_ARG, "paa_chan_draw: B=%d (>= 1)", B);
    if (drift_q32 > (1u << 31)) PAA_FAIL(PAA_ERR_ARG, "paa_chan_draw: drift_q32=%u above 2^31", drift_q32);
    if (!(snr_lo_db <= snr_hi_db) || !(fabsf(snr_lo_db) <= 1000.0f) || !(fabsf(snr_hi_db) <= 1000.0f))
        PAA_FAIL(PAA_ERR_ARG, "paa_chan_draw: snr range [%g, %g] dB", (double)snr_lo_db, (double)snr_hi_db);
    const PhiloxKey k = key_of(seed);
    hipLaunchKernelGGL(k_chan_draw, dim3(1), dim3(DRAW_NT), 0, (hipStream_t)stream, k.k0, k.k1, d_counter, stream_id, clip_base, B,
                       drift_q32, snr_lo_db, snr_hi_db, d_rq, d_snr_db);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_drift_apply(const uint64_t* d_rq, const float* d_in, float* d_out, int B, int L, int adjoint,
                                      void* stream) {
    if (!d_rq || !d_in || !d_out) PAA_FAIL(PAA_ERR_ARG, "paa_drift_apply: null argument");
    if (B < 1 || L < 1) PAA_FAIL(PAA_ERR_ARG, "paa_drift_apply: B=%d L=%d (>= 1 each)", B, L);
    const uintptr_t i0 = (uintptr_t)d_in, o0 = (uintptr_t)d_out, bytes = (uintptr_t)B * (uintptr_t)L * sizeof(float);
    if (i0 < o0 + bytes && o0 < i0 + bytes) PAA_FAIL(PAA_ERR_ARG, "paa_drift_apply: d_in and d_out overlap");
    const dim3 grid = clips_grid(cdiv(L, CHAN_NT * DRIFT_PER_THREAD), B);
    if (adjoint)
        hipLaunchKernelGGL(k_drift_adjoint, grid, dim3(CHAN_NT), 0, (hipStream_t)stream, d_rq, d_in, d_out, B, L);
    else
        hipLaunchKernelGGL(k_drift_apply, grid, dim3(CHAN_NT), 0, (hipStream_t)stream, d_rq, d_in, d_out, B, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_noise_add(uint64_t seed, int32_t* d_counter, int stream_id, int clip_base, const float* d_clean,
                                    const float* d_snr_db, float* d_sigma, float* d_rows, int B, int L, void* stream) {
    if (!d_counter || !d_clean || !d_snr_db || !d_sigma || !d_rows) PAA_FAIL(PAA_ERR_ARG, "paa_noise_add: null argument");
    if (B < 1 || L < 1) PAA_FAIL(PAA_ERR_ARG, "paa_noise_add: B=%d L=%d (>= 1 each)", B, L);
    hipLaunchKernelGGL(k_noise_sigma, dim3(B), dim3(CHAN_NT), 0, (hipStream_t)stream, d_counter, d_clean, d_snr_db, d_sigma, B, L);
    PAA_LAUNCH_CHECK();
    const PhiloxKey k = key_of(seed);
    hipLaunchKernelGGL(k_noise_add, clips_grid(cdiv(cdiv(L, 4), CHAN_NT), B), dim3(CHAN_NT), 0, (hipStream_t)stream, k.k0, k.k1,
                       d_counter, stream_id, clip_base, d_sigma, d_rows, B, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}
