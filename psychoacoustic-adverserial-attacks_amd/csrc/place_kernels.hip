// Random placement of the universal perturbation: a per-clip circular shift s_b, tiling to the clip length
// and a gain a_b,
//     rows[b][i] = a_b * delta[(i + s_b) mod Lp]                                   (paa_place_rows, gather only)
//     grad[j]    = sum_b a_b * sum_{i < L, (i + s_b) mod Lp = j} G[b][i]           (paa_place_reduce, its adjoint)
// and the draw of (s_b, a_b) from the placement stream of philox.h with the step counter in device memory (paa_place_draw), so that
// a captured graph draws anew on every replay.  All three are memory-bound: the gather reads delta (Lp floats, cache-resident) and writes
// B * L floats once; the reduce reads B * L floats once, every output owned by one thread (no atomics, f64 sums in a fixed
// order: two calls give the same bits).  No integer division per element: a thread resolves its start once and wraps by
// compare-and-subtract.
#include "paa_common.h"
#include "philox.h"

using namespace paa;

namespace {

constexpr int PLACE_NT = 256;          // threads per block of the gather and the reduce
constexpr int ROWS_PER_THREAD = 8;     // outputs per thread of the gather: a block covers 2048 consecutive samples of one row
constexpr int REDUCE_CLIPS = 256;      // clips whose (shift, gain) a block of the reduce stages in LDS at a time

// s mod Lp in [0, Lp) for any int32 s (a shift from a caller's buffer may be negative or >= Lp)
__device__ __forceinline__ int wrap_shift(int s, int Lp) {
    int r = s % Lp;
    return r < 0 ? r + Lp : r;
}

__global__ void __launch_bounds__(DRAW_NT) k_place_draw(uint32_t k0, uint32_t k1, int32_t* __restrict__ counter, int stream_id,
                                                        int clip_base, int B, int Lp, int shift_on, float gain_db,
                                                        int32_t* __restrict__ shift, float* __restrict__ gain) {
    draw_clips(k0, k1, counter, stream_id, clip_base, B, TAG_PLACE, [=](int b, const uint32_t (&c)[4]) {
        shift[b] = shift_on ? draw_below(c[0], Lp) : 0;
        gain[b] = draw_gain(c[1], gain_db);
    });
}

// grid (tiles of PLACE_NT * ROWS_PER_THREAD samples, clips); thread t of a tile writes samples tile0 + t + k * PLACE_NT
__global__ void __launch_bounds__(PLACE_NT) k_place_rows(const float* __restrict__ p, int Lp, const int32_t* __restrict__ shift,
                                                         const float* __restrict__ gain, float* __restrict__ rows, int B, int L) {
    const int64_t tile0 = (int64_t)blockIdx.x * (PLACE_NT * ROWS_PER_THREAD);
    const unsigned uLp = (unsigned)Lp;
    const unsigned step = (unsigned)PLACE_NT % uLp;
    // start of the tile and of this thread modulo Lp, once; both addends are < Lp, so one compare-and-subtract each
    const unsigned tile_m = (unsigned)(tile0 % Lp);
    unsigned t_m = (unsigned)threadIdx.x % uLp + tile_m;
    if (t_m >= uLp) t_m -= uLp;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float a = gain ? gain[b] : 1.0f;
        unsigned j = t_m + (unsigned)wrap_shift(shift[b], Lp);
        if (j >= uLp) j -= uLp;
        float* __restrict__ out = rows + (int64_t)b * L;
        int64_t i = tile0 + threadIdx.x;
#pragma unroll
        for (int k = 0; k < ROWS_PER_THREAD; ++k) {
            if (i < L) out[i] = a * p[j];
            i += PLACE_NT;
            j += step;
            if (j >= uLp) j -= uLp;
        }
    }
}

// one thread per output j: clips ascending, then i ascending; every term (double) a_b * (double) G[b][i] is exact in f64
__global__ void __launch_bounds__(PLACE_NT) k_place_reduce(const float* __restrict__ G, const int32_t* __restrict__ shift,
                                                           const float* __restrict__ gain, float* __restrict__ grad, int B, int L,
                                                           int Lp) {
    __shared__ int s_shift[REDUCE_CLIPS];
    __shared__ float s_gain[REDUCE_CLIPS];
    const int64_t j = (int64_t)blockIdx.x * PLACE_NT + threadIdx.x;
    double acc = 0.0;
    for (int b0 = 0; b0 < B; b0 += REDUCE_CLIPS) {
        const int nb = min(REDUCE_CLIPS, B - b0);
        __syncthreads();
        for (int k = threadIdx.x; k < nb; k += PLACE_NT) {
            s_shift[k] = wrap_shift(shift[b0 + k], Lp);
            s_gain[k] = gain[b0 + k];
        }
        __syncthreads();
        if (j < Lp) {
            for (int k = 0; k < nb; ++k) {
                const double a = (double)s_gain[k];
                const float* __restrict__ g = G + (int64_t)(b0 + k) * L;
                int64_t i = j - s_shift[k];              // the first i >= 0 with (i + s) mod Lp = j
                if (i < 0) i += Lp;
#pragma unroll 4
                for (; i < L; i += Lp) acc += a * (double)g[i];
            }
        }
    }
    if (j < Lp) grad[j] = (float)acc;                    // no term: +0.0f
}

}  // namespace

extern "C" paa_status paa_place_draw(uint64_t seed, int32_t* d_counter, int stream_id, int clip_base, int B, int Lp, int shift_on,
                                     float gain_db, int32_t* d_shift, float* d_gain, void* stream) {
    if (!d_counter || !d_shift || !d_gain) PAA_FAIL(PAA_ERR_ARG, "paa_place_draw: null argument");
    if (B < 1 || Lp < 1) PAA_FAIL(PAA_ERR_ARG, "paa_place_draw: B=%d Lp=%d (>= 1 each)", B, Lp);
    if (!(gain_db >= 0.0f && gain_db <= 20.0f)) PAA_FAIL(PAA_ERR_ARG, "paa_place_draw: gain_db=%g outside [0, 20]", (double)gain_db);
    const PhiloxKey k = key_of(seed);
    hipLaunchKernelGGL(k_place_draw, dim3(1), dim3(DRAW_NT), 0, (hipStream_t)stream, k.k0, k.k1, d_counter, stream_id, clip_base, B,
                       Lp, shift_on, gain_db, d_shift, d_gain);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_place_rows(const float* d_p, int Lp, const int32_t* d_shift, const float* d_gain, float* d_rows, int B,
                                     int L, void* stream) {
    if (!d_p || !d_shift || !d_rows) PAA_FAIL(PAA_ERR_ARG, "paa_place_rows: null argument");
    if (B < 1 || L < 1 || Lp < 1) PAA_FAIL(PAA_ERR_ARG, "paa_place_rows: B=%d L=%d Lp=%d (>= 1 each)", B, L, Lp);
    const dim3 grid = clips_grid(cdiv(L, PLACE_NT * ROWS_PER_THREAD), B);
    hipLaunchKernelGGL(k_place_rows, grid, dim3(PLACE_NT), 0, (hipStream_t)stream, d_p, Lp, d_shift, d_gain, d_rows, B, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_place_reduce(const float* d_grad_rows, const int32_t* d_shift, const float* d_gain, float* d_grad, int B,
                                       int L, int Lp, void* stream) {
    if (!d_grad_rows || !d_shift || !d_gain || !d_grad) PAA_FAIL(PAA_ERR_ARG, "paa_place_reduce: null argument");
    if (B < 1 || L < 1 || Lp < 1) PAA_FAIL(PAA_ERR_ARG, "paa_place_reduce: B=%d L=%d Lp=%d (>= 1 each)", B, L, Lp);
    hipLaunchKernelGGL(k_place_reduce, dim3(cdiv(Lp, PLACE_NT)), dim3(PLACE_NT), 0, (hipStream_t)stream, d_grad_rows, d_shift,
                       d_gain, d_grad, B, L, Lp);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}
