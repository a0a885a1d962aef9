// Per-clip perturbations through the playback chain: B clips, G draws of the chain per clip, R = B * G rows,
// r = b * G + g.  The two ends of the chain and the vote over the draws:
//     rows[r][i]       = a_r * (clean[b][i] + delta[b][i])        (paa_eot_rows: the mixture is what the loudspeaker plays)
//     clean_rows[r][i] = clean[b][i]                              (the level reference of paa_noise_add, per row)
//     grad[b][i]       = f32(sum_g (double) a_r * (double) G[r][i])   (paa_eot_reduce: the adjoint of paa_eot_rows in delta)
//     counts[b]        = counts_rows[b * G + g*],  g* the draw worst for the attacker   (paa_eot_vote)
// All memory-bound and elementwise along a row: a block of paa_eot_rows reads its stretch of clean_b / delta_b for every draw (the
// re-reads hit the cache) and writes G rows; a thread of paa_eot_reduce owns its outputs and adds the G terms in ascending g in f64
// (every product of two floats is exact there, so a fused multiply-add changes no bit: the bits of paa_place_reduce at shift 0).
// No atomics; nothing depends on the grid.  A row is walked in 16-byte accesses when all of its pointers have the same offset
// within 16 bytes — after a scalar head of up to three elements and before a scalar tail — and element by element otherwise.
#include <algorithm>

#include "paa_common.h"

using namespace paa;

namespace {

constexpr int EOT_NT = 256;
constexpr int EOT_CHUNK = 4096;        // floats one block covers per grid stride
constexpr int EOT_MAX_CHUNKS = 64;

// floats from p up to the next 16-byte boundary (0 .. 3); p is a float pointer, so its address is a multiple of 4
__device__ __forceinline__ int head_of(const void* p) { return (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2); }

// The walk of one row of L elements by the blocks of grid x: f1(i) for the scalar head [0, h) and tail, f4(i) for the aligned
// groups [i, i + 4).  h < 0: no common offset, every element through f1.
template <typename F1, typename F4>
__device__ __forceinline__ void walk_row(int L, int h, F1 f1, F4 f4) {
    const int64_t t0 = (int64_t)blockIdx.x * EOT_NT + threadIdx.x, stride = (int64_t)gridDim.x * EOT_NT;
    if (h < 0 || L < h + 4) {
        for (int64_t i = t0; i < L; i += stride) f1(i);
        return;
    }
    const int64_t n4 = (L - h) >> 2, tail0 = h + (n4 << 2);
    for (int64_t v = t0; v < n4; v += stride) f4(h + (v << 2));
    if (t0 < h) f1(t0);                                           // t0 < 3: threads of block 0
    for (int64_t i = tail0 + t0; i < L; i += stride) f1(i);
}

// grid (chunks, clips): the block strides b over the clips by gridDim.y and runs the draws of each
__global__ void __launch_bounds__(EOT_NT) k_eot_rows(const float* __restrict__ clean, const float* __restrict__ delta,
                                                     const float* __restrict__ gain, float* __restrict__ rows,
                                                     float* __restrict__ clean_rows, int B, int G, int L) {
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* __restrict__ c = clean ? clean + (int64_t)b * L : nullptr;
        const float* __restrict__ d = delta + (int64_t)b * L;
        for (int g = 0; g < G; ++g) {
            const int64_t r = (int64_t)b * G + g;
            const float a = gain ? gain[r] : 1.0f;
            float* __restrict__ out = rows + r * L;
            float* __restrict__ cout = clean_rows ? clean_rows + r * L : nullptr;
            int h = head_of(d);
            if (head_of(out) != h || (c && head_of(c) != h) || (cout && head_of(cout) != h)) h = -1;
            // one add, then one multiply: the intrinsics keep the compiler from contracting or reassociating them
            auto val = [&](float cv, float dv) {
                const float s = c ? __fadd_rn(cv, dv) : dv;
                return gain ? __fmul_rn(a, s) : s;
            };
            walk_row(L, h,
                     [&](int64_t i) {
                         const float cv = c ? c[i] : 0.0f;
                         out[i] = val(cv, d[i]);
                         if (cout) cout[i] = cv;
                     },
                     [&](int64_t i) {
                         const float4 dv = *reinterpret_cast<const float4*>(d + i);
                         const float4 cv = c ? *reinterpret_cast<const float4*>(c + i) : make_float4(0.f, 0.f, 0.f, 0.f);
                         *reinterpret_cast<float4*>(out + i) = make_float4(val(cv.x, dv.x), val(cv.y, dv.y), val(cv.z, dv.z), val(cv.w, dv.w));
                         if (cout) *reinterpret_cast<float4*>(cout + i) = cv;
                     });
        }
    }
}

// grid (chunks, clips); every output element is written by exactly one thread, its G terms added in ascending g
__global__ void __launch_bounds__(EOT_NT) k_eot_reduce(const float* __restrict__ Gr, const float* __restrict__ gain,
                                                       float* __restrict__ grad, int B, int G, int L) {
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* __restrict__ src = Gr + (int64_t)b * G * L;         // row b * G; row g of the clip lies g * L further
        const float* __restrict__ a = gain ? gain + (int64_t)b * G : nullptr;
        float* __restrict__ out = grad + (int64_t)b * L;
        // the G source rows share their offset when a row is a whole number of 16-byte groups (or there is one row)
        const int h = ((L & 3) == 0 || G == 1) && head_of(src) == head_of(out) ? head_of(out) : -1;
        walk_row(L, h,
                 [&](int64_t i) {
                     double acc = 0.0;
                     for (int g = 0; g < G; ++g) acc += (a ? (double)a[g] : 1.0) * (double)src[(int64_t)g * L + i];
                     out[i] = (float)acc;
                 },
                 [&](int64_t i) {
                     double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                     for (int g = 0; g < G; ++g) {
                         const double ag = a ? (double)a[g] : 1.0;
                         const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)g * L + i);
                         a0 += ag * (double)v.x;
                         a1 += ag * (double)v.y;
                         a2 += ag * (double)v.z;
                         a3 += ag * (double)v.w;
                     }
                     *reinterpret_cast<float4*>(out + i) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
                 });
    }
}

// one thread per clip: the first draw with strictly fewer (untargeted) / strictly more (targeted) errors than every draw before it
__global__ void __launch_bounds__(EOT_NT) k_eot_vote(const int32_t* __restrict__ rows, int B, int G, int targeted,
                                                     int32_t* __restrict__ counts) {
    for (int64_t b = (int64_t)blockIdx.x * EOT_NT + threadIdx.x; b < B; b += (int64_t)gridDim.x * EOT_NT) {
        const int32_t* __restrict__ c = rows + b * G * 3;
        int best = 0;
        int32_t e = c[0];
        for (int g = 1; g < G; ++g) {
            const int32_t eg = c[3 * (int64_t)g];
            if (targeted ? eg > e : eg < e) {
                best = g;
                e = eg;
            }
        }
        counts[3 * b] = e;
        counts[3 * b + 1] = c[3 * (int64_t)best + 1];
        counts[3 * b + 2] = c[3 * (int64_t)best + 2];
    }
}

paa_status check_shape(const char* who, int B, int G, int L) {
    if (B < 1 || G < 1 || L < 1) PAA_FAIL(PAA_ERR_ARG, "%s: B=%d G=%d L=%d (>= 1 each)", who, B, G, L);
    if ((int64_t)B * G > INT32_MAX) PAA_FAIL(PAA_ERR_ARG, "%s: B * G = %lld rows exceed INT32_MAX", who, (long long)B * G);
    return PAA_OK;
}

dim3 row_grid(int B, int L) { return clips_grid(std::min(cdiv(L, EOT_CHUNK), EOT_MAX_CHUNKS), B); }

}  // namespace

extern "C" paa_status paa_eot_rows(const float* d_clean, const float* d_delta, const float* d_gain, float* d_rows,
                                   float* d_clean_rows, int B, int G, int L, void* stream) {
    if (!d_delta || !d_rows) PAA_FAIL(PAA_ERR_ARG, "paa_eot_rows: null argument");
    if (d_clean_rows && !d_clean) PAA_FAIL(PAA_ERR_ARG, "paa_eot_rows: d_clean_rows needs d_clean");
    PAA_TRY(check_shape("paa_eot_rows", B, G, L));
    hipLaunchKernelGGL(k_eot_rows, row_grid(B, L), dim3(EOT_NT), 0, (hipStream_t)stream, d_clean, d_delta, d_gain, d_rows,
                       d_clean_rows, B, G, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_eot_reduce(const float* d_grad_rows, const float* d_gain, float* d_grad, int B, int G, int L,
                                     void* stream) {
    if (!d_grad_rows || !d_grad) PAA_FAIL(PAA_ERR_ARG, "paa_eot_reduce: null argument");
    PAA_TRY(check_shape("paa_eot_reduce", B, G, L));
    hipLaunchKernelGGL(k_eot_reduce, row_grid(B, L), dim3(EOT_NT), 0, (hipStream_t)stream, d_grad_rows, d_gain, d_grad, B, G, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_eot_vote(const int32_t* d_counts_rows, int B, int G, int targeted, int32_t* d_counts, void* stream) {
    if (!d_counts_rows || !d_counts) PAA_FAIL(PAA_ERR_ARG, "paa_eot_vote: null argument");
    PAA_TRY(check_shape("paa_eot_vote", B, G, 1));
    hipLaunchKernelGGL(k_eot_vote, dim3(std::min(cdiv(B, EOT_NT), 1024)), dim3(EOT_NT), 0, (hipStream_t)stream, d_counts_rows, B, G,
                       targeted ? 1 : 0, d_counts);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}
