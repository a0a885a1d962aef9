// Fused STFT -> per-bin projection -> iSTFT path for the default frame geometry (n_fft = win = 1024, hop = 256):
// see spec_kernels.hip.  Other geometries stay on the generic one-frame-per-workgroup kernels of proj_kernels.hip.
#pragma once
#include "paa_common.h"

namespace paa {

// SOP_MASK: clip each bin to a per-(row, frame, bin) magnitude bound (masking norm); SOP_PSD: the forward half only, writing
// 10 log10(|X|^2 + 1e-20) per bin (the masking threshold's first pass); SOP_MLOSS: the masking-threshold loss term (k_spec_mloss:
// hinge weight per bin against the clips' bounds, then the ADJOINT of the STFT instead of its inverse)
enum SpecOp { SOP_NONE = 0, SOP_MINMAX = 1, SOP_PHON = 2, SOP_FM = 3, SOP_MASK = 4, SOP_PSD = 5, SOP_MLOSS = 6 };

struct SpecArgs {
    const float* x;        // (rows, L) waveform in                       [waveform source]
    const float* S_in;     // (rows, T, F) complex64 in                   [spectrum source]
    float* out;            // (rows, out_len) waveform out                [waveform destination]
    float* S_out;          // (rows, T, F) complex64 out                  [spectrum destination]
    double* part;          // FM: one partial sum of |S|^2 w per (row, workgroup)
    const float2* tw;      // e^{-2 pi i m / 1024}, m < 1024
    const float* win;      // periodic Hann window, 1024
    const float* fm;       // [10][513] Fletcher-Munson weights lerped to the bins (< 0: outside the interpolator)
    const float* thr;      // [513] max_phon contour
    const float* thr_max;  // [1]
    int L, T, out_len;     // samples per row in, frames, samples per row out (>= 256 (T - 1); the tail is zero-filled)
    float bin_hz, min_f, max_f, phon_ref;
    const float* mask;     // MASK: magnitude bound, frame t of row r at mask + r * mask_rs + t * F (mask_rs = 0: one bound for all rows)
    int64_t mask_rs;
    float* psd;            // PSD: (rows, T, F) f32 level in dB
    float* pmax_part;      // PSD: the maximum level of each (row, workgroup), (rows, gridDim.x)
    // MLOSS (spec_mloss): x = the perturbation rows, mask / mask_rs = every clip's bound A_b; a row is held against `nclip` clips
    // starting at clip (per_clip ? row : 0)
    const float* pmax;     // (clips) Pmax_b of the clean clips
    const float* alpha;    // device [1] (alpha_rs = 0) or (rows) (alpha_rs = 1: row r reads alpha[r]), nullable (1.0)
    float* grad;           // (rows, L): grad -= alpha * dloss; nullable (losses only)
    float* wout;           // (rows, T, F) hinge weight W; nullable
    double* lpart;         // loss partials, (clips, lstride): one double per (clip, workgroup, wave)
    int nclip, per_clip, lstride;
    int alpha_rs;          // stride of alpha over the rows: 0 or 1 (paa_masking_loss_rows)
    const float* rscale;   // PHON, row projections: (rows) per-row bound scale s, nullable; the threshold moves by 20 log10(s) dB
};

// rows x (L) waveform -> per-bin op -> waveform (train.py:38-66 _project_frequency_domain with _align_to), in place allowed
// when out == x is NOT used by a later workgroup — callers pass a separate output buffer.
paa_status spec_project(const SpecArgs& a, int op, int rows, int* n_part, hipStream_t st);
paa_status spec_stft(const SpecArgs& a, int rows, hipStream_t st);     // fourier_transforms.py:20-29
paa_status spec_istft(const SpecArgs& a, int rows, hipStream_t st);    // fourier_transforms.py:31-41
// per-bin op on a caller-supplied spectrum (projections.py:68-159 called on a (B, F, T) tensor), frame-major storage
paa_status spec_apply(const SpecArgs& a, int op, int rows, const float* scale, int* n_part, hipStream_t st);
// masking threshold pass 1 (k_spec_psd): a.x (rows, L) -> a.psd (rows, T, F) and a.pmax_part (rows, spec_psd_groups(T))
paa_status spec_psd(const SpecArgs& a, int rows, hipStream_t st);
inline int spec_psd_groups(int T) { return cdiv(T, 4); }
// masking-threshold loss of `rows` perturbation rows (SpecArgs: MLOSS fields): grad -= alpha * d(sum_b l_b), W and the loss
// partials a.lpart[clip * a.lstride + i], i < spec_mloss_parts(T) (a.lstride must be that number); then spec_mloss_finish sums
// them in a fixed order: loss_rows[b] (nullable), loss_sum[0] = sum_b (double)loss_rows[b] (nullable); scratch: `clips` doubles
constexpr int MLOSS_NW = 8;                                       // waves = frames per workgroup of k_spec_mloss
inline int spec_mloss_groups(int T) { return T <= MLOSS_NW ? 1 : cdiv(T, MLOSS_NW - 3); }
inline int spec_mloss_parts(int T) { return spec_mloss_groups(T) * MLOSS_NW; }
paa_status spec_mloss(const SpecArgs& a, int rows, hipStream_t st);
paa_status spec_mloss_finish(const double* lpart, int lstride, int clips, double* scratch, float* loss_rows, float* loss_sum,
                             hipStream_t st);
int spec_groups(int T, int rows, int op, bool src_spec);        // workgroups per row spec_project / spec_istft launch (size of the FM partial array / rows)

}  // namespace paa
