// Room responses on the placement layer: clip b hears its row through the response h_c, c = index[b],
//     out[b][i] = sum_{k=0}^{min(K-1, i)}     h_c[k] * in[b][i - k]          (paa_rir_apply, adjoint = 0: causal FIR, zero history)
//     out[b][j] = sum_{k=0}^{min(K-1, L-1-j)} h_c[k] * in[b][j + k]          (adjoint = 1: its exact adjoint)
// and the draw of c_b from the room stream of philox.h with a step counter of its own in device memory (paa_rir_draw).
//
// The apply is a Toeplitz product on the f32-input MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain at the f32
// vector peak).  A wave owns 32 x 32 output tiles Y[m][n] = y[base + 32 n + m] and sums over j = 0 .. K + 30 (zero-extended to K + 37 at most),
//     forward:  Y[m][n] += hz[j + m - 31] * x[base + 32 n + 31 - j]          hz = h, zero outside [0, K)
//     adjoint:  Y[m][n] += hz[j - m]      * x[base + 32 n + j]               x = 0 outside [0, L)
// so one band of hz serves every tile of every clip, only 31 of the K + 31 steps are padding, and edges need no branch: samples
// and taps out of range are staged as zeros.  The signal is the A operand (row = n) and the band the B operand (column = m): an
// accumulator register then holds 32 consecutive outputs across 32 lanes, and the stores are 128-byte lines.  The j loop runs
// in chunks of RIR_JC steps staged in LDS (the band: RIR_JC + 31 floats; the signal window of the block's span: RIR_SPAN + RIR_JC
// - 32 floats, one pad dword per 32 so that the 32-dword lane stride of the signal read hits 32 different banks).  Every output
// has ONE accumulator chain, j ascending, whatever the grid: two calls give the same bits.  No atomics, no allocation.
#include "paa_common.h"
#include "philox.h"

using namespace paa;

namespace {

constexpr int RIR_NT = 256;                               // 4 waves
constexpr int RIR_TILES = 1;                              // 32 x 32 tiles per wave (more would share the band operand)
constexpr int RIR_WAVE_SPAN = RIR_TILES * 1024;           // outputs per wave
constexpr int RIR_SPAN = (RIR_NT / 64) * RIR_WAVE_SPAN;   // outputs per block: 4096 consecutive samples of one clip
constexpr int RIR_UNROLL = 4;                             // MFMA steps (of two j each) per group of the inner loop
constexpr int RIR_JC = 2080;                              // j steps per staged chunk (a multiple of 2 RIR_UNROLL): K = 4096 in two
constexpr int RIR_XS = RIR_SPAN + RIR_JC - 32;            // signal samples a chunk needs
constexpr int RIR_XS_PHYS = RIR_XS + RIR_XS / 32 + 1;     // with one pad dword per 32

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int wrap_index(int c, int N) {
    int r = c % N;
    return r < 0 ? r + N : r;
}

__global__ void __launch_bounds__(DRAW_NT) k_rir_draw(uint32_t k0, uint32_t k1, int32_t* __restrict__ counter, int stream_id,
                                                      int clip_base, int B, int N, int32_t* __restrict__ index) {
    draw_clips(k0, k1, counter, stream_id, clip_base, B, TAG_ROOM,
               [=](int b, const uint32_t (&c)[4]) { index[b] = draw_below(c[0], N); });
}

// grid (spans of RIR_SPAN outputs, clips); wave w of a block owns the tiles at span0 + w * RIR_WAVE_SPAN + t * 1024
template <int ADJ>
__global__ void __launch_bounds__(RIR_NT) k_rir_apply(const float* __restrict__ bank, int N, int K, const int32_t* __restrict__ index,
                                                      const float* __restrict__ in, float* __restrict__ out, int B, int L) {
    __shared__ float hs[RIR_JC + 32];
    __shared__ float xs[RIR_XS_PHYS];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, half = lane >> 5;           // r: n of the signal operand, m of the band operand; half: k of the step
    const int64_t span0 = (int64_t)blockIdx.x * RIR_SPAN;
    const int toff = wave * RIR_WAVE_SPAN;
    const bool active = span0 + toff < L;                // wave-uniform: a wave past the end only helps to stage
    const int jtot = (K + 31 + 2 * RIR_UNROLL - 1) & ~(2 * RIR_UNROLL - 1);      // K + 31 steps, zero-extended to whole unrolled groups
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const float* __restrict__ h = bank + (int64_t)wrap_index(index[b], N) * K;
        const float* __restrict__ x = in + (int64_t)b * L;
        f32x16 acc[RIR_TILES];
#pragma unroll
        for (int t = 0; t < RIR_TILES; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[t][v] = 0.0f;
        for (int jc = 0; jc < jtot; jc += RIR_JC) {
            const int jn = min(RIR_JC, jtot - jc);       // a multiple of 2 RIR_UNROLL
            __syncthreads();                             // the chunk before has been read
            // Staging loads a clamped (always valid) address and selects the zero afterwards, so that the unrolled loops issue
            // their global loads together instead of one latency after the other.
#pragma unroll 4
            for (int t = tid; t < jn + 31; t += RIR_NT) {                       // hz[jc - 31 .. jc + jn - 1]
                const int a = jc - 31 + t;
                const float v = h[min(max(a, 0), K - 1)];
                hs[t] = (a >= 0 && a < K) ? v : 0.0f;
            }
            const int64_t xlo = ADJ ? span0 + jc : span0 + 32 - jc - jn;        // first sample of the window
#pragma unroll 4
            for (int t = tid; t < RIR_SPAN + jn - 32; t += RIR_NT) {
                const int64_t xi = xlo + t;
                const float v = x[min(max(xi, (int64_t)0), (int64_t)L - 1)];
                xs[t + (t >> 5)] = (xi >= 0 && xi < L) ? v : 0.0f;
            }
            __syncthreads();
            if (active) {
                // step s of the chunk is j = jc + 2 s + half.  Band: hs[(j - jc) + m] forward, hs[(j - jc) - m + 31] adjoint;
                // signal: window sample toff + 32 n + (jn - 1 - (j - jc)) forward, toff + 32 n + (j - jc) adjoint.
                int la = ADJ ? half - r + 31 : half + r;
                int lx = ADJ ? toff + 32 * r + half : toff + 32 * r + jn - 1 - half;
                for (int s = 0; s < jn; s += 2 * RIR_UNROLL) {                  // RIR_UNROLL steps: every LDS read first, then the MFMAs
                    float hv[RIR_UNROLL], xv[RIR_UNROLL][RIR_TILES];
#pragma unroll
                    for (int u = 0; u < RIR_UNROLL; ++u) {
                        hv[u] = hs[la + 2 * u];
                        const int q = ADJ ? lx + 2 * u : lx - 2 * u;
                        const int px = q + (q >> 5);
#pragma unroll
                        for (int t = 0; t < RIR_TILES; ++t) xv[u][t] = xs[px + t * 1056];   // tile t: 1024 samples = 1056 padded dwords on
                    }
#pragma unroll
                    for (int u = 0; u < RIR_UNROLL; ++u)
#pragma unroll
                        for (int t = 0; t < RIR_TILES; ++t)
                            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv[u][t], hv[u], acc[t], 0, 0, 0);
                    la += 2 * RIR_UNROLL;
                    lx += ADJ ? 2 * RIR_UNROLL : -2 * RIR_UNROLL;
                }
            }
        }
        if (active) {
            float* __restrict__ y = out + (int64_t)b * L;
#pragma unroll
            for (int t = 0; t < RIR_TILES; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) {           // D: column = lane & 31 (m), row = (v & 3) + 8 (v >> 2) + 4 half (n)
                    const int n = (v & 3) + 8 * (v >> 2) + 4 * half;
                    const int64_t i = span0 + toff + t * 1024 + 32 * n + r;
                    if (i < L) y[i] = acc[t][v];
                }
        }
    }
}

}  // namespace

extern "C" paa_status paa_rir_draw(uint64_t seed, int32_t* d_counter, int stream_id, int clip_base, int B, int N, int32_t* d_index,
                                   void* stream) {
    if (!d_counter || !d_index) PAA_FAIL(PAA_ERR_ARG, "paa_rir_draw: null argument");
    if (B < 1 || N < 1) PAA_FAIL(PAA_ERR_ARG, "paa_rir_draw: B=%d N=%d (>= 1 each)", B, N);
    const PhiloxKey k = key_of(seed);
    hipLaunchKernelGGL(k_rir_draw, dim3(1), dim3(DRAW_NT), 0, (hipStream_t)stream, k.k0, k.k1, d_counter, stream_id, clip_base, B, N,
                       d_index);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}

extern "C" paa_status paa_rir_apply(const float* d_bank, int N, int K, const int32_t* d_index, const float* d_in, float* d_out, int B,
                                    int L, int adjoint, void* stream) {
    if (!d_bank || !d_index || !d_in || !d_out) PAA_FAIL(PAA_ERR_ARG, "paa_rir_apply: null argument");
    if (B < 1 || L < 1 || N < 1) PAA_FAIL(PAA_ERR_ARG, "paa_rir_apply: B=%d L=%d N=%d (>= 1 each)", B, L, N);
    if (K < 1 || K > PAA_RIR_MAX_TAPS) PAA_FAIL(PAA_ERR_ARG, "paa_rir_apply: K=%d outside [1, %d]", K, PAA_RIR_MAX_TAPS);
    const uintptr_t i0 = (uintptr_t)d_in, o0 = (uintptr_t)d_out, bytes = (uintptr_t)B * (uintptr_t)L * sizeof(float);
    if (i0 < o0 + bytes && o0 < i0 + bytes) PAA_FAIL(PAA_ERR_ARG, "paa_rir_apply: d_in and d_out overlap");
    const dim3 grid = clips_grid(cdiv(L, RIR_SPAN), B);
    if (adjoint)
        hipLaunchKernelGGL(k_rir_apply<1>, grid, dim3(RIR_NT), 0, (hipStream_t)stream, d_bank, N, K, d_index, d_in, d_out, B, L);
    else
        hipLaunchKernelGGL(k_rir_apply<0>, grid, dim3(RIR_NT), 0, (hipStream_t)stream, d_bank, N, K, d_index, d_in, d_out, B, L);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}
