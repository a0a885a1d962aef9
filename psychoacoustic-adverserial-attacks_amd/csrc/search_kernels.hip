// Per-clip bound search on the device: after the step's word-error counters are known and BEFORE the
// update, decide per clip whether the attack succeeded, keep the perturbation row that produced the success together with the
// bound scale it was projected under, and tighten that clip's scale:
//     success_b  (targeted)    errors_b == 0 and ref_words_b > 0
//                (untargeted)  ref_words_b > 0 and errors_b * 1000 >= wer_milli * ref_words_b
//     on success               best[b] <- delta[b];  best_scale[b] <- scale[b];  best_step[b] <- step;
//                              scale[b] <- fmaxf(scale[b] * shrink, floor_scale)
//     on failure               nothing of clip b is written
//     afterwards               *step += 1 (on the device: a captured graph counts on)
// Two launches, so that no block reads what another block of its launch writes: k_search_decide (ONE workgroup) reads the counter,
// the counts and the scales, writes the scalars and one flag per row; k_search_keep (chunks, B) copies the flagged rows.  The flags
// live in a fixed device array (one per row, B <= SEARCH_MAX_B = the grid's y limit), so the entry allocates nothing; calls on
// different streams of one device must not overlap (as with a projection context's workspace).  No atomics.
#include <algorithm>

#include "paa_common.h"

using namespace paa;

namespace {

constexpr int SEARCH_NT = 256;
constexpr int SEARCH_MAX_B = 65535;
constexpr int KEEP_CHUNK = 4096;       // floats one block of the copy covers per grid stride
constexpr int KEEP_MAX_CHUNKS = 64;

__device__ int32_t g_search_flag[SEARCH_MAX_B];

__global__ void __launch_bounds__(SEARCH_NT) k_search_decide(const int32_t* __restrict__ counts, int B, int targeted, int wer_milli,
                                                             float shrink, float floor_scale, float* __restrict__ scale,
                                                             float* __restrict__ best_scale, int32_t* __restrict__ best_step,
                                                             int32_t* __restrict__ step_ctr) {
    const int32_t step = *step_ctr;
    for (int b = threadIdx.x; b < B; b += SEARCH_NT) {
        const int32_t e = counts[3 * b], w = counts[3 * b + 1];
        // exact integer compares (64-bit products: no caller's wer_milli can overflow them)
        const bool ok = targeted ? (e == 0 && w > 0) : (w > 0 && (int64_t)e * 1000 >= (int64_t)wer_milli * w);
        g_search_flag[b] = ok ? 1 : 0;
        if (ok) {
            const float s = scale[b];
            best_scale[b] = s;
            best_step[b] = step;
            scale[b] = fmaxf(s * shrink, floor_scale);
        }
    }
    __syncthreads();                          // every thread has read the counter
    if (threadIdx.x == 0) *step_ctr = step + 1;
}

// Per-clip adaptive masking-loss weight: the decide kernel of paa_clip_anneal.  Same success test, same shape
// (ONE workgroup, one flag per row for k_search_keep), but the row is kept only where its masking loss improves on the best so far
// (strict f32 compare: a NaN loss never keeps, an equal loss keeps the earlier delta), and alpha moves on the periods of n = step + 1:
//     keep   success && l < best_loss[b]      best_loss[b] <- l;  best_alpha[b] <- alpha[b];  best_step[b] <- step;  flag (row copy)
//     raise  success && n % up_every == 0     alpha[b] <- fminf(fmaxf(alpha[b] * up, alpha_min), alpha_max)
//     lower  !success && n % down_every == 0  alpha[b] <- fminf(fmaxf(alpha[b] * down, alpha_min), alpha_max)
// best_alpha is the alpha the kept delta was optimised under: it is read before alpha moves.
__global__ void __launch_bounds__(SEARCH_NT) k_anneal_decide(const int32_t* __restrict__ counts, const float* __restrict__ loss_rows,
                                                             int B, int targeted, int wer_milli, int up_every, int down_every, float up,
                                                             float down, float alpha_min, float alpha_max, float* __restrict__ alpha,
                                                             float* __restrict__ best_loss, float* __restrict__ best_alpha,
                                                             int32_t* __restrict__ best_step, int32_t* __restrict__ step_ctr) {
    const int32_t step = *step_ctr;
    const int64_t n = (int64_t)step + 1;
    const bool up_now = n % up_every == 0, down_now = n % down_every == 0;
    for (int b = threadIdx.x; b < B; b += SEARCH_NT) {
        const int32_t e = counts[3 * b], w = counts[3 * b + 1];
        const bool ok = targeted ? (e == 0 && w > 0) : (w > 0 && (int64_t)e * 1000 >= (int64_t)wer_milli * w);
        const float l = loss_rows[b], a = alpha[b];
        const bool keep = ok && l < best_loss[b];
        g_search_flag[b] = keep ? 1 : 0;
        if (keep) {
            best_loss[b] = l;
            best_alpha[b] = a;
            best_step[b] = step;
        }
        if (ok ? up_now : down_now) alpha[b] = fminf(fmaxf(a * (ok ? up : down), alpha_min), alpha_max);
    }
    __syncthreads();                          // every thread has read the counter
    if (threadIdx.x == 0) *step_ctr = step + 1;
}

// grid (chunks, B): row blockIdx.y, flag uniform over the block. 16-byte accesses where both row bases are aligned (L odd
// misaligns every second row), element by element otherwise.
__global__ void __launch_bounds__(SEARCH_NT) k_search_keep(const float* __restrict__ delta, float* __restrict__ best, int L) {
    const int b = blockIdx.y;
    if (!g_search_flag[b]) return;
    const float* __restrict__ src = delta + (size_t)b * L;
    float* __restrict__ dst = best + (size_t)b * L;
    const int t0 = blockIdx.x * SEARCH_NT + threadIdx.x, stride = gridDim.x * SEARCH_NT;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const int n4 = L >> 2;
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
        float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
        for (int i = t0; i < n4; i += stride) d4[i] = s4[i];
        for (int i = (n4 << 2) + t0; i < L; i += stride) dst[i] = src[i];
    } else {
        for (int i = t0; i < L; i += stride) dst[i] = src[i];
    }
}

}  // namespace

extern "C" paa_status paa_clip_search(const float* d_delta, int B, int L, const int32_t* d_counts, int targeted, int wer_milli,
                                      float shrink, float floor_scale, float* d_scale, float* d_best, float* d_best_scale,
                                      int32_t* d_best_step, int32_t* d_step, void* stream) {
    if (!d_delta || !d_counts || !d_scale || !d_best || !d_best_scale || !d_best_step || !d_step)
        PAA_FAIL(PAA_ERR_ARG, "paa_clip_search: null argument");
    if (B < 1 || L < 1) PAA_FAIL(PAA_ERR_ARG, "paa_clip_search: B=%d L=%d (>= 1 each)", B, L);
    if (B > SEARCH_MAX_B) PAA_FAIL(PAA_ERR_ARG, "paa_clip_search: B=%d exceeds %d", B, SEARCH_MAX_B);
    if (!(shrink > 0.0f && shrink < 1.0f)) PAA_FAIL(PAA_ERR_ARG, "paa_clip_search: shrink=%g outside (0, 1)", (double)shrink);
    if (!(floor_scale > 0.0f && floor_scale <= 1.0f))
        PAA_FAIL(PAA_ERR_ARG, "paa_clip_search: floor_scale=%g outside (0, 1]", (double)floor_scale);
    if (wer_milli < 1) PAA_FAIL(PAA_ERR_ARG, "paa_clip_search: wer_milli=%d (>= 1)", wer_milli);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_search_decide, dim3(1), dim3(SEARCH_NT), 0, st, d_counts, B, targeted ? 1 : 0, wer_milli, shrink,
                       floor_scale, d_scale, d_best_scale, d_best_step, d_step);
    PAA_LAUNCH_CHECK();
    const int chunks = std::min(cdiv(L, KEEP_CHUNK), KEEP_MAX_CHUNKS);
    hipLaunchKernelGGL(k_search_keep, dim3(chunks, B), dim3(SEARCH_NT), 0, st, d_delta, d_best, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_clip_anneal(const float* d_delta, int B, int L, const int32_t* d_counts, const float* d_loss_rows, int targeted,
                                      int wer_milli, int up_every, int down_every, float up, float down, float alpha_min,
                                      float alpha_max, float* d_alpha, float* d_best, float* d_best_loss, float* d_best_alpha,
                                      int32_t* d_best_step, int32_t* d_step, void* stream) {
    if (!d_delta || !d_counts || !d_loss_rows || !d_alpha || !d_best || !d_best_loss || !d_best_alpha || !d_best_step || !d_step)
        PAA_FAIL(PAA_ERR_ARG, "paa_clip_anneal: null argument");
    if (B < 1 || L < 1) PAA_FAIL(PAA_ERR_ARG, "paa_clip_anneal: B=%d L=%d (>= 1 each)", B, L);
    if (B > SEARCH_MAX_B) PAA_FAIL(PAA_ERR_ARG, "paa_clip_anneal: B=%d exceeds %d", B, SEARCH_MAX_B);
    if (wer_milli < 1) PAA_FAIL(PAA_ERR_ARG, "paa_clip_anneal: wer_milli=%d (>= 1)", wer_milli);
    if (up_every < 1 || down_every < 1)
        PAA_FAIL(PAA_ERR_ARG, "paa_clip_anneal: up_every=%d down_every=%d (>= 1 each)", up_every, down_every);
    if (!(up > 1.0f && up < INFINITY)) PAA_FAIL(PAA_ERR_ARG, "paa_clip_anneal: up=%g must be finite and > 1", (double)up);
    if (!(down > 0.0f && down < 1.0f)) PAA_FAIL(PAA_ERR_ARG, "paa_clip_anneal: down=%g outside (0, 1)", (double)down);
    if (!(alpha_min > 0.0f && alpha_min <= alpha_max && alpha_max < INFINITY))
        PAA_FAIL(PAA_ERR_ARG, "paa_clip_anneal: need 0 < alpha_min=%g <= alpha_max=%g < inf", (double)alpha_min, (double)alpha_max);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_anneal_decide, dim3(1), dim3(SEARCH_NT), 0, st, d_counts, d_loss_rows, B, targeted ? 1 : 0, wer_milli, up_every,
                       down_every, up, down, alpha_min, alpha_max, d_alpha, d_best_loss, d_best_alpha, d_best_step, d_step);
    PAA_LAUNCH_CHECK();
    const int chunks = std::min(cdiv(L, KEEP_CHUNK), KEEP_MAX_CHUNKS);
    hipLaunchKernelGGL(k_search_keep, dim3(chunks, B), dim3(SEARCH_NT), 0, st, d_delta, d_best, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}
