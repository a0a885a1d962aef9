// Clean-signal masking threshold (MPEG-1 psychoacoustic model 1 as Qin et al. 2019 §4.1 use it) for the default frame geometry
// (n_fft = win = 1024, hop = 256): see mask_kernels.hip and DESIGN.md §6c.
#pragma once
#include "paa_common.h"

namespace paa {

// Per-bin constants, computed on the host in double at paa_proj_create (mask_tables) and uploaded once.
struct MaskTables {
    const float* z;        // [F] Bark of bin k
    const float* quiet;    // [F] threshold in quiet at f_k, dB (masker candidates below it are dropped)
    const float* ath;      // [F] ATH_k, dB (read for k >= kA only)
    const int* win;        // [F] lo_k | hi_k << 16: the bins j with |z_j - z_k| < 0.5
    int kA;                // first bin with z > 1
};

struct MaskArgs {
    const float* P;        // (rows, T, F) level in dB (k_spec_psd)
    const float* part;     // (rows, nparts) per-workgroup maxima of P (k_spec_psd)
    float* out;            // (rows, T, F): theta in dB, or the magnitude bound A when `bound` (may alias P)
    float* psd;            // nullable (rows, T, F): P - Pmax + 96
    float* pmax;           // nullable (rows): Pmax
    MaskTables tab;
    int T, nparts, bound;
    float margin;          // masking_margin_db
};

// Temporal masking: theta'(t, k) = max(theta(t, k), theta(t - j, k) - post[j - 1] (1 <= j <= n_post, t - j >= 0),
// theta(t + j, k) - pre[j - 1] (1 <= j <= n_pre, t + j < T)), every term one f32 subtraction, max exact.
constexpr int MASK_LAGS = 32;
struct MaskSpreadArgs {
    const float* theta;    // (rows, T, F) theta in dB (pass 2); never the plane `out` points into
    float* out;            // (rows, T, F): theta' in dB, or the magnitude bound A' when `bound`
    const float* pmax;     // (rows) Pmax (pass 2; read when `bound`)
    int T, bound, n_post, n_pre;
    float margin;
    float post[MASK_LAGS]; // decrement in dB at lag j = index + 1 frames after the masker
    float pre[MASK_LAGS];  // ... before the masker
};

// host: the tables of one sample rate; z, quiet, ath as float, win packed
void mask_tables(int sr, float* z, float* quiet, float* ath, int* win, int* kA);
// pass 2: theta (or A) of every frame of `rows` rows
paa_status mask_threshold(const MaskArgs& a, int rows, hipStream_t st);
// between passes 2 and 3, temporal masking on: theta' (or A') of every frame of `rows` rows
paa_status mask_spread(const MaskSpreadArgs& a, int rows, hipStream_t st);
// pass 3 (universal perturbation): A[0] = min over rows of A[r], elementwise over n = T * F floats
paa_status mask_min_rows(float* A, int rows, int64_t n, hipStream_t st);

}  // namespace paa
