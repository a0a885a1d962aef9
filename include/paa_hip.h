/* paa_hip.h — C ABI of libpaa_hip.so, the MI355X (gfx950) implementation of the PGD inner step of
 * tomer-erez/Psychoacoustic-adverserial-attacks (hot path only).
 *
 * The reference has no FFI: its boundary is a set of Python call signatures.  Each entry point
 * below names the reference function it replaces (paths are into the reference's src/).  All
 * pointers named d_* are DEVICE pointers owned by the caller (torch tensors on the host side);
 * every call is asynchronous on `stream` (a hipStream_t passed as void*), performs no allocation,
 * no host synchronisation and is hipGraph-capturable, unless stated otherwise.  Every function
 * returns a paa_status; nothing throws or aborts across this boundary.  paa_last_error() returns
 * a thread-local message for the most recent non-zero status.
 */
#ifndef PAA_HIP_H
#define PAA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PAA_OK = 0,
    PAA_ERR_BAD_NORM = 1,    /* train.py:98   ValueError("Unknown norm_type") */
    PAA_ERR_NEED_CLEAN = 2,  /* train.py:90-95 ValueError: snr / tv without clean audio */
    PAA_ERR_SIZE = 3,        /* shape / capacity mismatch (build.py:315 ValueError on length) */
    PAA_ERR_HIP = 4,         /* a HIP runtime call failed; message carries hipGetErrorString */
    PAA_ERR_ARG = 5,         /* null pointer / invalid enum / unsupported parameter */
    PAA_ERR_MISSING = 6      /* a required weight tensor was not supplied */
} paa_status;

/* args.norm_type (training_utils/parser.py:38-40), in the parser's order of choices.  PAA_NORM_MASKING (extension): clip every
 * bin of the perturbation's STFT to the clean clip's frequency-masking threshold (paa_masking_threshold), default geometry only */
typedef enum {
    PAA_NORM_L2 = 0, PAA_NORM_LINF = 1, PAA_NORM_SNR = 2, PAA_NORM_TV = 3,
    PAA_NORM_FLETCHER_MUNSON = 4, PAA_NORM_MIN_MAX_FREQS = 5, PAA_NORM_MAX_PHON = 6, PAA_NORM_MASKING = 7
} paa_norm;

/* The fields of the reference's argparse namespace that the hot path reads (parser.py:10-66). */
typedef struct {
    int32_t norm_type;        /* paa_norm */
    float l2_size, linf_size, snr_db, tv_epsilon, fm_epsilon;
    float min_freq_attack, max_freq_attack, phon_reference_db;
    float lr;                 /* args.lr, PGD step size (train.py:161) */
    int32_t direction;        /* +1 untargeted, -1 targeted (train.py:124) */
    float masking_margin_db;  /* masking norm: dB added to the threshold (args.masking_margin_db, extension) */
} paa_params;

const char* paa_last_error(void);
/* 350 = this header (340 + the placement entries paa_place_draw, paa_place_rows and paa_place_reduce; the room-response entries
 * paa_rir_draw and paa_rir_apply, and the playback-channel entries paa_chan_draw, paa_drift_apply and paa_noise_add, are later
 * additions that changed nothing else and took no new number); 351 = the same ABI built
 * with -DPAA_EXPERIMENTS (diagnostic kernels and environment switches compiled in,
 * tools/ only).  Bindings refuse other values. */
int paa_version(void);
/* sizeof(paa_params), sizeof(paa_arch), sizeof(paa_tensor), sizeof(paa_gemm_desc): layout check for bindings */
void paa_abi_sizes(int32_t* out4);

/* ------------------------------------------------------------------ projection context ----- */
/* Holds FFT twiddles, the periodic Hann window, the Fletcher-Munson weight table, the max_phon
 * contour and the frame / partial-sum workspace.  Replaces the per-call setup in
 * core/fourier_transforms.py:20,32 and the scipy interpolator object of core/iso.py:238-266.
 *   fm_table:   host, [10][n_fft/2+1] float64 — iso weight grid already lerped along frequency to
 *               the rfft bins (value < 0 marks a bin outside [20 Hz, 20 kHz] => weight 1.0)
 *   spl_thresh: host, [n_fft/2+1] float32 — build.py:325-348 init_phon_threshold_tensor
 * Allocates device memory (not capturable). max_batch*max_len bounds later calls. */
typedef struct paa_proj paa_proj;
paa_status paa_proj_create(paa_proj** out, int n_fft, int hop_length, int win_length, int sr,
                           const double* fm_table, const float* spl_thresh, int max_batch, int max_len);
void paa_proj_destroy(paa_proj* h);
paa_status paa_proj_set_spl_thresh(paa_proj* h, const float* spl_thresh /* host, F */);

/* training_utils/train.py:69-99 perturbation_constraint (dispatch) over
 * core/projections.py:11-159.  In place on d_p (rows_p, L); rows_p is 1 for the universal
 * perturbation (build.py:301).  d_clean (B, L) may be NULL except for snr / tv; when NULL the
 * frequency-domain result keeps iSTFT length semantics by zeroing samples >= hop*(T-1)
 * exactly as _align_to (train.py:27-35) does with a length-L clean batch. */
paa_status paa_project(paa_proj* h, const paa_params* prm, float* d_p, int rows_p,
                       const float* d_clean, int B, int L, void* stream);

/* Out-of-place form of paa_project: reads d_src (rows_p, L), writes d_dst (rows_p, L); the two must not overlap.  This is
 * how the reference's functions behave (they return a new tensor, projections.py:24,33,46) and it is the fast path of the
 * frequency-domain norms: ONE fused launch (STFT -> per-bin op -> iSTFT + overlap-add; plus the scale launch for
 * fletcher_munson), whereas the in-place form goes through the workspace and a copy-back launch. */
paa_status paa_project_to(paa_proj* h, const paa_params* prm, const float* d_src, float* d_dst, int rows_p,
                          const float* d_clean, int B, int L, void* stream);

/* core/projections.py:68-80 project_min_max_freqs, :116-133 project_fm_norm, :138-159 project_phon_level applied to a
 * spectrum the caller already holds (these reference functions take the complex (B, F, T) STFT tensor, train.py:52-59):
 * d_S_in / d_S_out (B, T, F) complex64 interleaved, frame-major (the transposed view of the reference's layout);
 * in place allowed.  prm->norm_type must be one of the three frequency-domain norms (else PAA_ERR_BAD_NORM). */
paa_status paa_spectrum_project(paa_proj* h, const paa_params* prm, const float* d_S_in, float* d_S_out, int B, int T,
                                void* stream);
/* core/projections.py:83-113 compute_fm_weighted_norm_interp: d_out[0] = sqrt(sum |S|^2 * w(10 log10(|S|^2 + 1e-10), f_bin)) */
paa_status paa_fm_weighted_norm(paa_proj* h, const float* d_S, int B, int T, float* d_out, void* stream);

/* Data-parallel form: project_snr / project_tv use whole-batch statistics of the clean
 * audio (projections.py:11-35, 56-66), so every rank reduces its shard with paa_batch_stats —
 * d_out2 = [sum clean^2, TV(clean)], d_clip_count[0] = (float)B (nullable) — the caller all-reduces
 * these three numbers with the gradient, and paa_project_ext projects from the GLOBAL values:
 * d_clean_stats = device [sum clean^2, TV(clean)] over all ranks; the SNR target norm's clean.numel()
 * (projections.py:27) is d_clip_count[0] * L when d_clip_count (device, the all-reduced clip count — a
 * small integer, exact in f32) is given, else the host value clean_numel.  Nothing here depends on the
 * local batch size being equal across ranks or steps. */
paa_status paa_batch_stats(paa_proj* h, const float* d_clean, int B, int L, float* d_out2, float* d_clip_count,
                           void* stream);
paa_status paa_project_ext(paa_proj* h, const paa_params* prm, float* d_p, int rows_p,
                           const float* d_clean_stats /* device [2] */, const float* d_clip_count /* device [1] or NULL */,
                           double clean_numel /* used when d_clip_count is NULL */, int L, void* stream);

/* ---- masking norm (PAA_NORM_MASKING, extension) -------------------------------------------------------
 * MPEG-1 psychoacoustic model 1 threshold of each clean clip on the default frame geometry (n_fft = win = 1024, hop = 256;
 * any other geometry: PAA_ERR_ARG).  P = 10 log10(|STFT(clean_b)|^2 + 1e-20), Pmax_b its maximum over the clip, and
 * P' = P - Pmax_b + 96; tonal maskers are the strict local maxima of P' at or above the threshold in quiet that no louder masker
 * within 0.5 Bark suppresses; theta(t, k) = 10 log10(sum_j 10^(T_j(k) / 10) + [z_k > 1] 10^(ATH_k / 10)) (dB, -inf where the
 * sum is 0).  The projection clips S = STFT(delta) to A = 10^((theta + masking_margin_db - 96 + Pmax_b) / 20) per bin, phase
 * kept, then iSTFT with the _align_to tail rule.  paa_project / paa_project_to: rows of d_p under min_b A_b (the universal
 * perturbation hides under every clip of the batch); paa_project_rows: row b under A_b.  d_clean is required
 * (PAA_ERR_NEED_CLEAN); paa_project_ext and paa_spectrum_project refuse the norm (PAA_ERR_BAD_NORM).  The threshold is
 * recomputed from d_clean inside every projection call (a captured step follows the clean buffer); the workspace is
 * allocated by paa_proj_create (B <= max_batch).
 * paa_masking_threshold: d_theta (B, T, F) theta in dB, frame-major like paa_stft; d_psd (B, T, F) P' (nullable);
 * d_pmax (B) Pmax_b (nullable). */
paa_status paa_masking_threshold(paa_proj* h, const float* d_clean, int B, int L, float* d_psd, float* d_theta, float* d_pmax,
                                 void* stream);

/* ---- masking-threshold loss term (Qin et al. 2019 stage 2, extension) ----------------------------------
 * With theta_b, Pmax_b and A_b of clean clip b as above (margin = prm->masking_margin_db, the only field read), S = STFT(delta),
 * c_b = 10^((96 - Pmax_b) / 10), T = 1 + L / 256, F = 513:
 *   l_b(delta) = 1 / (T F) sum_{t,k} max(c_b |S(t,k)|^2 - 10^((theta_b(t,k) + margin) / 10), 0) = c_b / (T F) sum max(|S|^2 - A_b^2, 0)
 * (strict hinge: a bin is active iff |S|^2 > A_b^2).  d_p (p_rows, L): p_rows = 1 holds the one row against all B clips,
 * p_rows = B holds row b against clip b; any other p_rows is PAA_ERR_ARG.  With W(t,k) = 1 / (T F) sum_b c_b [active_b(t,k)] and
 * H = W S, DC and Nyquist doubled, the gradient of sum_b l_b is the adjoint of the STFT applied to H: the windowed frames
 * w 1024 irfft(H(t,:)) overlap-added with no envelope division, the reflect padding folded back onto the samples it mirrors.
 *   d_alpha     device [1], read on the stream (a captured graph follows it); NULL = 1.0
 *   d_grad      (p_rows, L): d_grad -= alpha * grad(sum_b l_b) (the step's convention: grad = d(direction * CTC), the term is
 *               subtracted from the objective); NULL = losses only
 *   d_loss_rows (B) l_b, not weighted by alpha; nullable
 *   d_loss_sum  [1] = (float) sum_b (double) d_loss_rows[b] in clip order, WRITTEN, not accumulated; nullable
 *   d_weight    (p_rows, T, F) W, a diagnostic for tests; nullable
 * No atomics: two calls give the same bits.  d_clean is required (PAA_ERR_NEED_CLEAN); default frame geometry only
 * (PAA_ERR_ARG); B <= max_batch of the context (PAA_ERR_SIZE).  The threshold is recomputed from d_clean in every call. */
paa_status paa_masking_loss(paa_proj* h, const paa_params* prm, const float* d_p, int p_rows, const float* d_clean, int B, int L,
                            const float* d_alpha, float* d_grad, float* d_loss_rows, float* d_loss_sum, float* d_weight,
                            void* stream);

/* core/fourier_transforms.py:4-29 compute_stft: (B, L) -> d_out (B, T, F) complex64 interleaved,
 * T = 1 + L / hop; the (B, F, T) tensor the reference returns is the transpose-view of this. */
paa_status paa_stft(paa_proj* h, const float* d_x, int B, int L, float* d_out, void* stream);
/* core/fourier_transforms.py:31-41 compute_istft: d_S (B, T, F) complex64 -> d_out (B, hop*(T-1)). */
paa_status paa_istft(paa_proj* h, const float* d_S, int B, int T, float* d_out, void* stream);

/* train.py:160-161  p += lr * sign(grad). */
paa_status paa_sign_step(float* d_p, const float* d_grad, float lr, int L, void* stream);
/* train.py:165-175 with torch.optim.Adam(lr) as build.py:352-359 builds it (foreach, capturable=False,
 * weight_decay 0, amsgrad / maximize off), in the order of torch/optim/adam.py _multi_tensor_adam, per element i < L:
 *   g = grad_sign * d_grad[i]
 *   m = lerp(m, g, w1)                  w1 = (float)(1 - beta1); ATen/native/Lerp.h: |w1| < 0.5 ? fma(w1, g - m, m)
 *                                                                 : fma(-(g - m), 1 - w1, g)
 *   v = v * beta2;  v = fma(omb2, g * g, v)                       omb2 = (float)(1 - beta2)   (_foreach_addcmul_)
 *   d = sqrt(v) / d_scal[1];  d = d + eps
 *   p = fma(d_scal[0], m / d, p)                                  (_foreach_addcdiv_)
 *   d_grad_out[i] = g                   (d_grad_out may be NULL)
 * The three FMAs are the contractions torch's own gfx950 foreach kernels execute; sqrt and division are IEEE-rounded,
 * so the result equals torch.optim.Adam fed the same gradient, bit for bit.
 * d_scal: device [2] = { -lr / (1 - beta1^t), sqrt(1 - beta2^t) }, computed on the host in double as
 * _multi_tensor_adam does and rounded to f32.  Read from device memory so that a captured graph picks up the new
 * step count and a StepLR-changed lr on every replay.  Stream-ordered, allocates nothing, capturable. */
paa_status paa_adam_step(float* d_p, const float* d_grad, float grad_sign, float* d_exp_avg, float* d_exp_avg_sq,
                         const float* d_scal, float w1, float beta2, float omb2, float eps, float* d_grad_out, int L,
                         void* stream);
/* core/projections.py:37-39 project_linf(p, min_val, max_val): in-place clamp of n floats to [lo, hi]. */
paa_status paa_clamp(float* d_p, int64_t n, float lo, float hi, void* stream);
/* train.py:136  out = clamp(clean + p, -1, 1), p broadcast over the batch. */
paa_status paa_compose_clamp(const float* d_clean, const float* d_p, float* d_out, int B, int L, void* stream);

/* ---- per-clip perturbations: one row delta_b per clip b (the per-utterance attack next to the universal one) ----- */
/* training_utils/train.py:69-99 perturbation_constraint applied to every row on its own: row r of d_src (rows, L) is
 * projected as perturbation_constraint(src[r][None], clean[r][None], args) projects it — l2 and fletcher_munson from the
 * row's own norm, snr from clean row r's own mean power (clean.numel() = L), tv from TV(clean[r]); linf, min_max_freqs and
 * max_phon are row-local already.  d_clean (rows, L) is required for snr / tv (PAA_ERR_NEED_CLEAN as paa_project).  In place
 * when d_src == d_dst, out of place otherwise (the two must not overlap).  rows = 1 is paa_project_to / paa_project on that
 * row.  One launch sequence for all rows; the workspace is the one paa_proj_create sized (rows <= max_batch, L <= max_len). */
paa_status paa_project_rows(paa_proj* h, const paa_params* prm, const float* d_src, float* d_dst, int rows,
                            const float* d_clean, int L, void* stream);
/* ---- per-clip bound search (extension; additions to ABI 350) ------------------------------------------------
 * paa_project_rows_scaled: paa_project_rows with row r's bound tightened by s = d_scale[r], a device (rows) f32 array read on the
 * stream (a captured graph follows the buffer).  f32 arithmetic, part of the contract:
 *   linf             clamp to +-(linf_size * s)
 *   l2               eps = l2_size * s
 *   tv               eps = (tv_epsilon * s) * TV(clean_r)
 *   fletcher_munson  eps = fm_epsilon * s (fused and generic frame geometry alike)
 *   snr              the row is left alone iff cur >= snr_db - 20 log10f(s); else its target norm is sqrtf(sp / snr_linear * numel) * s
 *   max_phon         the per-bin threshold is thr + 20 log10f(s) dB
 *   min_max_freqs    has no size: s is ignored
 *   masking          PAA_ERR_BAD_NORM (a per-clip threshold with a moving margin is a change of its own)
 * d_scale == NULL is paa_project_rows: the same launches, the same bits.  s = 1.0f gives the bits of the unscaled call for every
 * norm (x * 1.0f, log10f(1.0f) = 0 and thr + 0.0f are exact).  A value that is not a finite positive number is treated as 1.0f on
 * the device, so it cannot produce NaN rows.  In place and out of place, workspace, PAA_ERR_SIZE / PAA_ERR_NEED_CLEAN /
 * PAA_ERR_ARG as paa_project_rows; with a scale, rows = 1 runs the row launches (the same bits as the one-row call at s = 1).
 * No atomics. */
paa_status paa_project_rows_scaled(paa_proj* h, const paa_params* prm, const float* d_src, float* d_dst, int rows,
                                   const float* d_clean, int L, const float* d_scale /* device (rows) */, void* stream);
/* Decide / keep / shrink, per clip b, with step = *d_step and (e, w, _) = d_counts[b] (what paa_wer_counts wrote for the step):
 *   success   targeted: e == 0 && w > 0;  untargeted: w > 0 && e * 1000 >= wer_milli * w   (exact integer compares)
 *   on success  d_best[b] <- d_delta[b] (the whole row: 16-byte accesses where both row bases are 16-byte aligned, element by
 *               element otherwise), d_best_scale[b] <- d_scale[b], d_best_step[b] <- step,
 *               d_scale[b] <- fmaxf(d_scale[b] * shrink, floor_scale)
 *   on failure  nothing of clip b is written: not its d_best row, not its scalars
 *   afterwards  *d_step = step + 1 ON THE DEVICE, so a captured graph counts on.
 * The step's counters belong to the delta that ENTERED the step, so the call sits after paa_wer_counts and BEFORE the update: it
 * records the delta that produced the success with the scale that delta was projected under (d_best[b] satisfies the bound at
 * d_best_scale[b]).  Two launches (a one-workgroup decide kernel writing per-row flags, then a (chunks, B) copy grid): no block
 * reads what another block of its launch writes.  Capturable, allocates nothing, no atomics; the flags are a fixed per-device
 * array, so calls on different streams of one device must not overlap.  PAA_ERR_ARG before any launch: a null pointer, B < 1
 * (or B > 65535), L < 1, shrink outside (0, 1), floor_scale outside (0, 1], wer_milli < 1. */
paa_status paa_clip_search(const float* d_delta /* (B, L) */, int B, int L, const int32_t* d_counts /* (B, 3) paa_wer_counts */,
                           int targeted, int wer_milli, float shrink, float floor_scale,
                           float* d_scale /* (B) in/out */, float* d_best /* (B, L) */, float* d_best_scale /* (B) */,
                           int32_t* d_best_step /* (B) */, int32_t* d_step /* [1] */, void* stream);
/* ---- per-clip adaptive masking-loss weight (Qin et al. 2019 stage 2 schedule, extension; additions to ABI 350) ----
 * paa_masking_loss_rows: paa_masking_loss with one weight per row.  alpha_rows is 1 or p_rows:
 *   alpha_rows = 1   paa_masking_loss itself: d_alpha device [1] or NULL = 1.0, the same launches, the same bits (paa_masking_loss
 *                    IS this call with alpha_rows = 1)
 *   alpha_rows = B   needs p_rows = B and a non-null d_alpha (B): row b of d_grad gets -= d_alpha[b] * grad l_b.  The row is the
 *                    workgroup's blockIdx.y, so the weight stays one scalar load per workgroup.
 * Any other combination is PAA_ERR_ARG before any launch.  Nothing else differs: d_loss_rows / d_loss_sum are the unweighted l_b and
 * their sum, d_weight the hinge weight W.  No atomics. */
paa_status paa_masking_loss_rows(paa_proj* h, const paa_params* prm, const float* d_p, int p_rows, const float* d_clean, int B, int L,
                                 const float* d_alpha, int alpha_rows, float* d_grad, float* d_loss_rows, float* d_loss_sum,
                                 float* d_weight, void* stream);
/* Decide / keep / move alpha, per clip b, with step = *d_step, n = step + 1, (e, w, _) = d_counts[b] (paa_wer_counts of the step),
 * l = d_loss_rows[b] (l_b of the step, paa_masking_loss_rows) and a = d_alpha[b].  All float arithmetic in f32, part of the contract:
 *   success   exactly paa_clip_search's test, the same integer compares
 *   keep      success && l < d_best_loss[b] (strict f32 compare: a NaN l never keeps, an equal l keeps the earlier delta):
 *             d_best[b] <- d_delta[b] (the whole row, as paa_clip_search copies it), d_best_loss[b] <- l,
 *             d_best_alpha[b] <- a (the alpha this delta was optimised under), d_best_step[b] <- step
 *   raise     success && n % up_every == 0:     d_alpha[b] <- fminf(fmaxf(a * up, alpha_min), alpha_max)
 *   lower     !success && n % down_every == 0:  d_alpha[b] <- fminf(fmaxf(a * down, alpha_min), alpha_max)
 *   otherwise nothing of clip b is written
 *   afterwards  *d_step = step + 1 ON THE DEVICE, so a captured graph counts on.
 * (Qin's constants: up 1.2 every 20 steps, down 0.8 every 50, alpha_min = alpha0 / 100.)  The counters and l_b both belong to the
 * delta that ENTERED the step, so the call sits after paa_wer_counts and BEFORE the update: the delta kept is the delta judged.  Two
 * launches, as paa_clip_search and for its reason (a one-workgroup decide kernel writing the scalars and one flag per row, then the
 * same (chunks, B) copy grid over the same flag array): the two entries never run in one step, and calls on different streams of one
 * device must not overlap.  Capturable, allocates nothing, no atomics.  PAA_ERR_ARG before any launch: a null pointer, B < 1,
 * B > 65535, L < 1, wer_milli < 1, up_every < 1, down_every < 1, up not finite or <= 1, down outside (0, 1), not
 * 0 < alpha_min <= alpha_max < inf. */
paa_status paa_clip_anneal(const float* d_delta /* (B, L) */, int B, int L, const int32_t* d_counts /* (B, 3) paa_wer_counts */,
                           const float* d_loss_rows /* (B) l_b of this step */, int targeted, int wer_milli,
                           int up_every, int down_every, float up, float down, float alpha_min, float alpha_max,
                           float* d_alpha /* (B) in/out */, float* d_best /* (B, L) */, float* d_best_loss /* (B) in/out */,
                           float* d_best_alpha /* (B) */, int32_t* d_best_step /* (B) */, int32_t* d_step /* [1] */, void* stream);
/* ---- temporal masking: post- and pre-masking of the threshold (extension; addition to ABI 350) ----------------------
 * post_db / pre_db are HOST arrays of decrements in dB: post_db[j - 1] = w_post[j] applies j frames after a masker, pre_db[j - 1] =
 * w_pre[j] j frames before it.  With tables set, every masking entry (paa_masking_threshold, the masking projections,
 * paa_masking_loss*) uses
 *   theta'(t, k) = max(theta(t, k), max_{1<=j<=n_post, t-j>=0} theta(t - j, k) - w_post[j], max_{1<=j<=n_pre, t+j<T} theta(t + j, k) - w_pre[j])
 * in place of theta: each term one f32 subtraction, the maximum exact, so the result is independent of order and tiling; the bound is
 * A' = 10^((theta' + margin - 96 + Pmax_b) / 20), the universal bound the minimum over clips of A'_b.  One more launch
 * (k_mask_spread) between the threshold pass and the minimum pass; pass 2 then writes theta into a second (max_batch, Tmax, F) plane
 * that this call allocates on first use (so it is NOT capturable: call it before capture; paa_proj_destroy frees the plane).
 * n_post = n_pre = 0 turns the mode off: the launches, arguments and bits of a handle that never saw this call.
 * PAA_ERR_ARG: a null handle, a non-default frame geometry, n outside [0, 32], a null table with n > 0, a value that is not finite,
 * not positive, or below its predecessor. */
paa_status paa_proj_set_masking_spread(paa_proj* h, int n_post, const float* post_db, int n_pre, const float* pre_db);
/* train.py:136 with one perturbation row per clip: out[b] = clamp(clean[b] + p[b], -1, 1); d_p (p_rows, L), p_rows in
 * {1, B}; p_rows = 1 is paa_compose_clamp. */
paa_status paa_compose_clamp_rows(const float* d_clean, const float* d_p, int p_rows, float* d_out, int B, int L,
                                  void* stream);

/* ---- random placement of the universal perturbation (extension) ----------------------------------------------
 * The perturbation delta has Lp >= 1 samples, the clips L; clip b gets a shift s_b in [0, Lp) and a gain a_b > 0:
 *   rows[b][i] = a_b * delta[(i + s_b) mod Lp]                          i = 0 .. L-1          (paa_place_rows)
 *   grad[j]    = sum_b a_b * sum_{i < L, (i + s_b) mod Lp = j} G[b][i]                         (paa_place_reduce, the adjoint)
 * Lp = L, s = 0, a = 1 is the plain universal step; Lp < L tiles delta (the seam is not smoothed); Lp > L uses a window of it.
 * G (B, L) is what paa_model_fwd_bwd_rows writes for d_p = rows.  No entry uses atomics: two calls give the same bits.  Null
 * pointers (except where stated), B < 1, L < 1 or Lp < 1: PAA_ERR_ARG, before any launch.
 *
 * THE STREAM TABLE of the playback chain (placement, room responses §6g, the channel §6k; csrc/philox.h).  Every
 * random number is a word of Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85) under
 * (k0, k1) = (seed & 0xffffffff, seed >> 32), with clip = clip_base + b:
 *     stream                            key                        counter (word 0, 1, 2, 3)
 *     placement draw  (paa_place_draw)  (k0, k1)                   (step, clip, stream_id, 0)
 *     room draw       (paa_rir_draw)    (k0, k1)                   (step, clip, stream_id, 1)
 *     channel draw    (paa_chan_draw)   (k0, k1)                   (step, clip, stream_id, 2)
 *     noise samples   (paa_noise_add)   (k0, k1 ^ 0x6E6F6973)      (step, clip, i >> 2,    stream_id)
 * The draws differ in word 3, the noise from all of them in the key: no (counter, key) pair of one stream is another's.  A draw is
 * ONE block: step = *d_counter read on the device, then *d_counter = step + 1 ON THE DEVICE (one thread, after every clip has
 * read step), so a captured graph draws anew on every replay.
 *
 * paa_place_draw: the placement stream.  With outputs r0..r3: d_shift[b] = (r0 * Lp) >> 32 (64-bit product; 0 when shift_on = 0);
 * u = (r1 >> 8) * 2^-24, d_gain[b] = exp2f(fmaf(u, 2 gain_db, -gain_db) * (log2(10) / 20)), exactly 1.0f for gain_db = 0.
 * gain_db outside [0, 20]: PAA_ERR_ARG.  stream_id: 0 = training, 1 = evaluation (by convention of the callers). */
paa_status paa_place_draw(uint64_t seed, int32_t* d_counter, int stream_id, int clip_base, int B, int Lp, int shift_on,
                          float gain_db, int32_t* d_shift, float* d_gain, void* stream);
/* d_p (Lp) -> d_rows (B, L); the product is one f32 multiply; d_gain NULL = 1.  A shift outside [0, Lp) is reduced modulo Lp on
 * the device (never an out-of-bounds index).  64-bit element offsets; rows need no alignment. */
paa_status paa_place_rows(const float* d_p, int Lp, const int32_t* d_shift, const float* d_gain /* nullable */, float* d_rows,
                          int B, int L, void* stream);
/* d_grad_rows (B, L) -> d_grad (Lp), WRITTEN, not accumulated.  Every output is owned by one thread; the terms
 * (double) a_b * (double) G[b][i] (exact in f64) are added in f64, clips ascending and then i ascending, and rounded once to
 * f32.  An output with no term (Lp > L) is +0.0f. */
paa_status paa_place_reduce(const float* d_grad_rows, const int32_t* d_shift, const float* d_gain, float* d_grad, int B, int L,
                            int Lp, void* stream);

/* ---- room responses on the placement layer (extension) ---------------------------------------------------------
 * A bank d_bank (N, K) of float32 room responses; clip b hears its row through response c_b = d_index[b]:
 *   out[b][i] = sum_{k=0}^{min(K-1, i)}     h_c[k] * in[b][i - k]      i = 0 .. L-1   (adjoint = 0: causal FIR, zero history, the
 *                                                                                      tail beyond L dropped; linear, not circular)
 *   out[b][j] = sum_{k=0}^{min(K-1, L-1-j)} h_c[k] * in[b][j + k]      j = 0 .. L-1   (adjoint = 1: the exact adjoint)
 * Both entries are asynchronous on the stream, allocate nothing, are capturable and use no atomics: two calls give the same bits.
 * They are additions to ABI 350: a binding that does not know them loses nothing.
 *
 * paa_rir_draw: the room stream of the stream table (above, at paa_place_draw).  d_index[b] = (r0 * N) >> 32.  d_counter is a
 * counter of the room draw's own (placement's is not advanced under explicit placements).  Null pointers, B < 1 or N < 1:
 * PAA_ERR_ARG. */
#define PAA_RIR_MAX_TAPS 16384
paa_status paa_rir_draw(uint64_t seed, int32_t* d_counter, int stream_id, int clip_base, int B, int N, int32_t* d_index,
                        void* stream);
/* d_in (B, L) -> d_out (B, L), WRITTEN; they must not overlap (PAA_ERR_ARG).  An index outside [0, N) is reduced modulo N on the
 * device (never an out-of-bounds row).  1 <= K <= PAA_RIR_MAX_TAPS, N >= 1, B >= 1, L >= 1, else PAA_ERR_ARG before any launch.
 * 64-bit element offsets; rows need no alignment.  Every output is one f32 fmaf chain over j = 0 .. K + 30 in ascending order
 * (v_mfma_f32_32x32x2_f32; terms outside the response or the row are exact zeros), independent of the grid:
 * |out - exact| <= (K + 64) 2^-24 sum_k |h_k in| + 2^-149. */
paa_status paa_rir_apply(const float* d_bank, int N, int K, const int32_t* d_index, const float* d_in, float* d_out, int B, int L,
                         int adjoint, void* stream);

/* ---- the playback channel on the placement layer: clock drift and ambient noise (extension) --------------------
 * Drift: clip b is resampled by r_b = rq_b / 2^32 (unsigned Q32; values outside [2^31, 2^33] are clamped on the device) with a
 * 16-tap Hann-windowed sinc, T = 8.  The output keeps the length L; samples outside [0, L) are zeros:
 *   pos_q = i * rq_b (64-bit, exact),  n = pos_q >> 32,  f = (pos_q & 0xffffffff) * 2^-32
 *   out[b][i] = sum_{t=-T+1..T} w(t - f) * in[b][n + t]                               (adjoint = 0)
 *   out[b][j] = sum_{i : n_i in [j-T, j+T-1]} w(j - n_i - f_i) * in[b][i]             (adjoint = 1: the exact transpose)
 *   w(u) = sinc(u) * (1 + cos(pi u / T)) / 2 for |u| < T, else 0 (sinc(0) = 1), in float32 with f rounded to float32
 * rq = 2^32 is the identity bit for bit.  No band-limiting is done for r > 1: meant for |r - 1| <= 0.1.
 * Noise: rows[b][i] += sigma_b * z_{b,i},  sigma_b = sqrt(mean_i clean[b][i]^2) * 10^(-snr_b / 20),  z standard normal.
 * All three entries are asynchronous on the stream, allocate nothing, are capturable and use no atomics: two calls on the same
 * inputs (and, for the noise, the same counter value) give the same bits.  They are additions to ABI 350.
 *
 * paa_chan_draw: the channel stream of the stream table (at paa_place_draw).  With outputs r0, r1:
 *   d_rq[b]     = 2^32 + ((((int64) r0 - 2^31) * drift_q32) >> 31)     (integers only, arithmetic shift; within 2^32 +- drift_q32)
 *   d_snr_db[b] = fmaf((r1 >> 8) * 2^-24, snr_hi_db - snr_lo_db, snr_lo_db)
 * d_counter is a counter of the channel draw's own.  drift_q32 = round(drift_ppm * 1e-6 * 2^32), computed by the caller.  Null
 * pointers, B < 1, drift_q32 > 2^31, snr_lo_db > snr_hi_db or either beyond +-1000: PAA_ERR_ARG. */
paa_status paa_chan_draw(uint64_t seed, int32_t* d_counter, int stream_id, int clip_base, int B, uint32_t drift_q32,
                         float snr_lo_db, float snr_hi_db, uint64_t* d_rq /* (B) */, float* d_snr_db /* (B) */, void* stream);
/* d_in (B, L) -> d_out (B, L), WRITTEN; they must not overlap.  Null pointers, B < 1, L < 1 or overlapping buffers: PAA_ERR_ARG
 * before any launch.  64-bit element offsets; rows need no alignment.  adjoint = 0: one f32 fmaf chain per output, t ascending,
 *   |out - exact| <= 2^-24 (16 sum_t |w_t in_t| + 8 sum_t |in_t|) + 2^-149
 * (the chain, and the rounding of the float32 weights).  adjoint = 1: the same float32 weights, exact products summed in f64 in
 * ascending i and rounded once; every output is owned by one thread. */
paa_status paa_drift_apply(const uint64_t* d_rq, const float* d_in, float* d_out, int B, int L, int adjoint, void* stream);
/* In place on d_rows (B, L).  Two launches: d_sigma[b] (a workspace of B floats, and an output) from d_clean (B, L) and
 * d_snr_db (B), then the add.  The samples: the noise stream of the stream table (at paa_place_draw); the word pair
 * (r[2p], r[2p+1]), p = (i & 3) >> 1, of the block of group i >> 2 gives
 *   u1 = ((r[2p] >> 8) + 1) * 2^-24,  u2 = (r[2p+1] >> 8) * 2^-24,  z = sqrt(-2 ln u1) * (cos(2 pi u2) for even i, sin for odd i).
 * step = *d_counter, a counter of the noise's own: the first launch advances it (one block, after reading it) and the second
 * reads it back as *d_counter - 1.  A clip with sigma = 0 keeps its rows' bits.  Null pointers, B < 1 or L < 1: PAA_ERR_ARG. */
paa_status paa_noise_add(uint64_t seed, int32_t* d_counter, int stream_id, int clip_base, const float* d_clean,
                         const float* d_snr_db, float* d_sigma /* (B) */, float* d_rows, int B, int L, void* stream);

/* ---- per-clip perturbations through the playback chain: the two ends and the vote (extension) -------------------
 * A batch of B clips, each with a perturbation of its own, is heard through G draws of the chain above: R = B * G rows,
 * r = b * G + g.  What is played is the mixture: one loudspeaker emits x_b + delta_b at the gain a_r of draw r,
 *   rows[r][i] = a_r * (clean[b][i] + delta[b][i])                                       (paa_eot_rows)
 *   grad[b][i] = sum_g a_r * G[r][i]                                                     (paa_eot_reduce, its adjoint in delta)
 * and paa_eot_vote picks, per clip, the word-error counters of the draw that is worst for the attacker.  The links between the
 * two ends are the entries above, on R rows.  All three are asynchronous on the stream, allocate nothing, are capturable, use no
 * atomics, and their results do not depend on the grid: two calls give the same bits.  64-bit element offsets; rows need no
 * alignment (16-byte accesses where a row's pointers share their offset within 16 bytes, after a scalar head and before a scalar
 * tail; element by element otherwise).  Null pointers (except where stated), B < 1, G < 1, L < 1 or B * G > INT32_MAX: PAA_ERR_ARG
 * before any launch, outputs untouched.  They are additions to ABI 350.
 *
 * paa_eot_rows: ONE f32 add, then ONE f32 multiply, never contracted.  d_clean NULL: the add is skipped (rows = a * delta);
 * d_gain NULL: the multiply is skipped.  d_clean_rows (nullable; needs d_clean): clean_rows[r][i] = clean[b][i], the level
 * reference paa_noise_add reads per row.  The outputs must not overlap the inputs. */
paa_status paa_eot_rows(const float* d_clean /* (B, L) nullable */, const float* d_delta /* (B, L) */,
                        const float* d_gain /* (B * G) nullable */, float* d_rows /* (B * G, L) */,
                        float* d_clean_rows /* (B * G, L) nullable */, int B, int G, int L, void* stream);
/* d_grad_rows (B * G, L) -> d_grad (B, L), WRITTEN, not accumulated.  Every output is owned by one thread; the terms
 * (double) a_r * (double) G[r][i] (exact in f64) are added in f64, g ascending, and rounded once to f32.  d_gain NULL = 1.  B = 1
 * gives the bits of paa_place_reduce(B = G, shifts 0, Lp = L). */
paa_status paa_eot_reduce(const float* d_grad_rows, const float* d_gain /* (B * G) nullable */, float* d_grad, int B, int G, int L,
                          void* stream);
/* d_counts_rows (B * G, 3): the (errors, reference words, hypothesis words) of paa_wer_counts per row -> d_counts (B, 3): the
 * triple of the draw with the fewest errors (targeted = 0) or the most errors (targeted != 0); ties go to the lowest g.  A clip
 * that "succeeds" on the voted counters succeeds in every draw. */
paa_status paa_eot_vote(const int32_t* d_counts_rows, int B, int G, int targeted, int32_t* d_counts, void* stream);

/* ------------------------------------------------------------------ model context ---------- */
/* Wav2Vec2ForCTC forward + CTC loss + backward to the waveform (core/loss_helpers.py:12-23 ->
 * transformers modeling_wav2vec2.py:1667-1736; training_utils/train.py:136-158). */
typedef struct {
    int32_t n_conv;               /* 7 */
    int32_t conv_dim[8], conv_kernel[8], conv_stride[8];
    int32_t conv_bias;            /* 0/1 */
    int32_t feat_norm_layer;      /* 0 = "group" (GroupNorm after conv0), 1 = "layer" (LN after every conv) */
    int32_t hidden, layers, heads, ffn;
    int32_t pos_k, pos_groups;
    int32_t stable_ln;            /* do_stable_layer_norm */
    int32_t vocab, blank;
    float ln_eps;
} paa_arch;

typedef struct {
    const char* name;             /* packed-tensor name, see paa_amd/model.py */
    const float* d_ptr;           /* device pointer, stays owned by the caller and must outlive the model */
    int64_t numel;
} paa_tensor;

/* precision: 0 = bf16 MFMA operands / f32 accumulate; 1 = split-bf16 (hi+lo, 3 MFMA passes),
 * fp32-parity mode.  Activations are stored in f32 in both modes.
 * GEMM weights arrive as bf16 bit patterns: "<name>" (hi plane) and, for precision 1, "<name>.lo" (lo plane, bf16(w - hi));
 * optionally "<name>.il" (precision 1, 2 * numel elements): the same two planes interleaved per 32-element K group of each
 * row, [32 hi | 32 lo | 32 hi | ...] — used by the large products where present (csrc/gemm.h, B_il), never required. */
typedef struct paa_model paa_model;
paa_status paa_model_create(paa_model** out, const paa_arch* arch, const paa_tensor* tensors, int n_tensors,
                            int max_batch, int length, int precision);
void paa_model_destroy(paa_model* m);
int64_t paa_model_workspace_bytes(const paa_model* m);
int paa_model_frames(const paa_model* m);     /* T_e for the configured length */

/* One forward + backward.  d_clean (B, L), d_p (1, L) [may be NULL: no perturbation, no clamp —
 * evaluation.py:16 semantics], d_labels (B, S_max) int32 with negatives as padding.
 *   d_grad  (L)  out: sum_b mask_b * dLoss/dperturbed_b, times `direction`   (train.py:158) — NULL => forward only
 *   d_logits (B, T_e, V) out (may be NULL)
 *   d_stats  (8) out: [0] loss (sum over the batch, HF ctc_loss_reduction='sum').  Slots [1..7] are NOT written by
 *            this call: they belong to the caller's data-parallel bookkeeping (paa_amd/training_utils/pgd.py packs
 *            [1] sum clean^2 and [2] TV(clean) from paa_batch_stats, [3] WER word errors, [4] WER reference words — the host's
 *            counters of the PREVIOUS step by default, THIS step's own counters written by paa_wer_counts (d_sums) with
 *            device_wer=True —,
 *            [5] the local clip count B (paa_batch_stats), [6] sum_b l_b of paa_masking_loss (masking_loss_alpha > 0, else 0),
 *            behind the gradient, so that ONE all-reduce carries everything
 *            and the global clean.numel() = L * sum_r B_r needs no collective of its own).
 */
paa_status paa_model_fwd_bwd(paa_model* m, const float* d_clean, const float* d_p, const int32_t* d_labels,
                             int B, int S_max, int direction, float* d_grad, float* d_logits, float* d_stats,
                             void* stream);

/* train.py:136-158 with one perturbation row per clip: d_p is (p_rows, L), p_rows in {1, B}.  p_rows = 1 is exactly
 * paa_model_fwd_bwd.  p_rows = B: clip b is composed as clamp(clean[b] + d_p[b], -1, 1) and d_grad (B, L) receives
 * direction * mask_b * dLoss/dperturbed_b in row b — the clip's own gradient (in eval mode clip b's loss depends on
 * delta_b alone), with no sum over the clips.  d_logits / d_stats as paa_model_fwd_bwd. */
paa_status paa_model_fwd_bwd_rows(paa_model* m, const float* d_clean, const float* d_p, int p_rows, const int32_t* d_labels,
                                  int B, int S_max, int direction, float* d_grad, float* d_logits, float* d_stats,
                                  void* stream);

/* Forward + CTC loss only (core/loss_helpers.py:46-57 get_loss, training_utils/evaluation.py:5-31): clamp = 0 adds p
 * without clamping as the reference's evaluation does (evaluation.py:16); d_p may be NULL (clean evaluation). */
paa_status paa_model_forward(paa_model* m, const float* d_clean, const float* d_p, int clamp, const int32_t* d_labels,
                             int B, int S_max, float* d_logits, float* d_stats, void* stream);
/* The same with d_p (p_rows, L), p_rows in {1, B}, one perturbation row per clip when p_rows = B
 * (training_utils/evaluation.py:5-31 on per-clip perturbations). */
paa_status paa_model_forward_rows(paa_model* m, const float* d_clean, const float* d_p, int p_rows, int clamp,
                                  const int32_t* d_labels, int B, int S_max, float* d_logits, float* d_stats, void* stream);

/* ---- true clip lengths (extension) ----------------------------------------------------------------------------
 * Every clip is cropped or right-zero-padded to the model's length L.  With lengths set, the model computes what HuggingFace's
 * Wav2Vec2ForCTC(input_values, attention_mask, labels) computes for clips of len_b in [400, L] samples, T_b = feat_len(len_b):
 *   compose   perturbed[b][i] = clamp(clean[b][i] + p[..][i], -1, 1) for i < len_b and exactly 0 beyond (clamp = 0: the plain sum
 *             under the same mask); the input gradient gets no term from i >= len_b (row b, or the sum over b)
 *   frames    rows t >= T_b of the feature projection's output are zeroed before the positional conv, and their gradient dropped
 *   attention keys >= T_b of clip b get probability 0 in every layer; ctx and dqkv rows >= T_b are zeros
 *   CTC       input_length = T_b; dlogits rows >= T_b are zero; an infeasible label row gives +inf as without lengths
 *   outputs   rows >= T_b of d_logits are zeros
 * d_lengths: device pointer to max_batch int32 entries, or NULL to switch the mode off (then every result is bit-identical to a
 * model that never had lengths).  The pointer is KEPT; its contents are read on the stream by every later
 * paa_model_fwd_bwd{,_rows} / paa_model_forward{,_rows} call, so a replayed graph follows the buffer.  The caller validates the
 * values; the device additionally clamps len_b to [0, L] and T_b to [1, T_e], so no value can index out of bounds.  Only the
 * fused attention path (head dim 64) supports lengths: PAA_ERR_ARG elsewhere.  Not itself capturable (it changes what later
 * calls launch); an addition to ABI 350. */
paa_status paa_model_set_lengths(paa_model* m, const int32_t* d_lengths);
/* d_out (B) int32 = T_b of the current length buffer, on the stream; PAA_ERR_ARG when no lengths are set. */
paa_status paa_model_frame_counts(paa_model* m, int B, int32_t* d_out, void* stream);
/* paa_argmax_ids on (B, T, V) logits with per-clip frame counts d_frames (B, clamped to [1, T] on the device): frames
 * t >= d_frames[b] get the id `blank`, so the greedy decode and paa_wer_counts see T_b frames of clip b. */
paa_status paa_argmax_ids_len(const float* d_logits, int B, int T, int V, const int32_t* d_frames, int blank, int16_t* d_ids,
                              void* stream);
/* d_p[r][i] = 0 for i >= d_lengths[r] (clamped to [0, L]), r < rows: the tail of a per-clip perturbation row beyond its clip. */
paa_status paa_mask_tail_rows(float* d_p, int rows, int L, const int32_t* d_lengths, void* stream);

/* core/loss_helpers.py:26,61  pred_ids = torch.argmax(logits, dim=-1): d_logits (rows, V) f32 -> d_ids (rows) int16
 * (first maximum wins; a NaN counts as the maximum, as in torch).  Feeds the host-side greedy CTC decode / WER. */
paa_status paa_argmax_ids(const float* d_logits, int64_t rows, int V, int16_t* d_ids, void* stream);

/* ---- on-device greedy CTC decode + word error counters (extension) -----------------------------------------
 * core/loss_helpers.py greedy_decode_ids + wer_texts + wer_counts on integers, one clip per workgroup, no host round trip.
 *   d_ids    (B, T) int16, what paa_argmax_ids writes
 *   d_canon  (V) int32: -1 = drop (special token), 0 = word delimiter, > 0 = code point of the token's lower-cased character;
 *            an id outside [0, V) is dropped
 *   d_refs   (B, R_cap) int32 code points: the words of the cleaned, lower-cased reference one after another, each terminated
 *            by 0, the row padded with -1 (a row ends at its first negative entry; entries behind an unterminated last word
 *            are not a word)
 * Frames whose id maps to -1 are dropped FIRST; a surviving frame is kept iff its id differs from the id of the previous
 * surviving frame ("A <pad> A" is one A: transformers 5.15 batch_decode, tests/golden/labels.json).  Hypothesis words are the
 * maximal runs of kept non-delimiter tokens; two words are equal iff length and every code point agree (compared in full);
 * errors = unit-cost Levenshtein distance between the two word sequences (either may be empty).
 *   d_counts (B, 3) int32 out: errors, reference words, hypothesis words of every clip
 *   d_sums   [2] float out, nullable: sum_b errors, sum_b reference words — integer sums converted once: exact, and the same
 *            bits in every run (no atomics)
 * Caps: 1 <= T <= 4096, 1 <= R_cap <= 8192 and the clip's LDS image (10 R_cap + 6 T bytes) within 64 KiB, else
 * PAA_ERR_SIZE; null pointers, B <= 0 or V outside [1, 32767]: PAA_ERR_ARG.  Nothing is truncated. */
paa_status paa_wer_counts(const int16_t* d_ids, int B, int T, const int32_t* d_canon, int V, const int32_t* d_refs, int R_cap,
                          int32_t* d_counts, float* d_sums, void* stream);
/* Per-step stats log: copies d_stats[0..n) to row (*d_cursor mod cap) of d_log (cap, n) and increments *d_cursor ON THE DEVICE,
 * so a captured graph appends a new row on every replay.  1 <= n <= 64, cap >= 1, else PAA_ERR_ARG. */
paa_status paa_stats_push(const float* d_stats, int n, float* d_log, int32_t* d_cursor, int cap, void* stream);

/* Diagnostics for tests: synchronous copy of a named internal activation to the host (see csrc/model.hip);
 * returns the number of floats the buffer holds for batch B (0 = unknown name, <0 = HIP error). */
int64_t paa_model_debug_read(paa_model* m, const char* name, float* host, int64_t max_floats, int B);
int paa_model_layout(const paa_model* m, int i);  /* padded rows of conv layer i; -1: frame rows P; -2: score ld */

/* ------------------------------------------------------------------ kernel-level test entries */
/* C[M,N] = epilogue(A[M,K] * B) — the MFMA GEMM all conv / linear / attention products go through.
 * See csrc/gemm.h for the descriptor; exported so tests can check each variant against the oracle. */
struct paa_gemm_desc;
paa_status paa_gemm(const struct paa_gemm_desc* d, void* stream);
/* Test / measurement aid: kernel selection of paa_gemm for the large regular products.  0 = automatic (default),
 * 1 = register-staged kernels only, else force ONE LDS-DMA ring configuration wherever its shape constraints hold: 7 / 8 =
 * 192 x 128 split / bf16 (csrc/gemm_ring.hip), 20 / 21 = 256 x 256 split / bf16, 22 / 23 = 192 x 256 split / bf16
 * (csrc/gemm_ring2.hip).  Results are bit-identical across all of them (same K order); tests assert that.  Any other value
 * selects a configuration only a -DPAA_EXPERIMENTS build holds (measured and rejected variants, timing probes); the shipped
 * library falls back to the register-staged kernels for it. */
void paa_gemm_config(int ring_mode);
/* Test / measurement aid: path of the fused attention backward.  0 = automatic (default: one pass in split-bf16 mode up to two
 * 256-key blocks, T <= 512; the kernel pair beyond that and, at every T, in bf16 mode, where one pass measured slower),
 * 1 = always the dQ and dK/dV kernel pair, 2 = one pass wherever a workspace is given, in either precision.  Any other value
 * leaves the mode as it is.  Returns the number of one-pass dispatches since the previous call (and resets that count). */
int paa_attn_bwd_config(int mode);
/* Measurement aid: the attention backward with a caller-owned one-pass workspace of paa_attn_dq_part_floats() floats (null: the
 * kernel pair); lo planes all null = bf16 mode, d_klen nullable.  The other backward entries allocate a workspace per call. */
int64_t paa_attn_dq_part_floats(int B, int nh, int T, int Tp);
paa_status paa_attn_bwd_ws(const void* qkv_hi, const void* qkv_lo, const void* ctx_hi, const void* ctx_lo, const float* lse,
                           const void* dctx_hi, const void* dctx_lo, float* delta, void* dqkv_hi, void* dqkv_lo,
                           const int32_t* d_klen, float* dq_part, int B, int T, int P, int Tp, int H, int nh, void* stream);
/* Test aid.  option 0: value != 0 makes the GroupNorm backward of conv0 take its statistics-pass + GEMM-pass path (the fallback of
 * the shapes the fused single-pass kernel does not cover) on every shape, so that tests can compare the two on the same operands. */
paa_status paa_test_option(int option, int value);
/* Measurement aid (bench.py roofline leg): HIP-event timing of every GEMM launch on its own stream.
 * paa_prof_enable(n>0) starts recording up to n launches (0 stops); paa_prof_read fills out[64][4] =
 * {launches, total ms, total algorithmic FLOP (2*M*N*K*batch), total algorithmic HBM bytes (every operand and result
 * byte of the descriptor once)} per kernel variant
 * (tall*32 + bf16_operands*16 + (narrow | 192-row tall tile)*8 + split*4 + a_kcontig*2 + b_kcontig; 40 / 44 = slab kernel
 * of the grouped positional convolution; 60 / 61 = LDS-DMA ring kernels, bf16 / split) and resets. */
paa_status paa_prof_enable(int max_launches);
paa_status paa_prof_read(double* out256);
/* paa_prof_pause(1) stops recording without releasing the events, paa_prof_pause(0) resumes: bench.py creates the
 * events before its timed region and records on the LAST timed step only (the first timing event recorded on a HIP
 * stream switches its queue to profiled dispatch for good, which costs ~4 % on every later launch). */
paa_status paa_prof_pause(int paused);
/* Fused attention (head_dim 64, bf16 planes as uint16): qkv (B*P, 3H) = Q|K|V, ctx/dctx (B*P, H), lse/delta (B*nh, Tp) */
paa_status paa_attn_fwd(const void* qkv, void* ctx, float* lse, int B, int T, int P, int Tp, int H, int nh, void* stream);
paa_status paa_attn_bwd(const void* qkv, const void* ctx, const float* lse, const void* dctx, float* delta, void* dqkv,
                        int B, int T, int P, int Tp, int H, int nh, void* stream);
/* the same with every operand as a hi + lo pair of bf16 planes (split-bf16, the fp32-parity mode) */
paa_status paa_attn_fwd_split(const void* qkv_hi, const void* qkv_lo, void* ctx_hi, void* ctx_lo, float* lse, int B, int T, int P,
                              int Tp, int H, int nh, void* stream);
paa_status paa_attn_bwd_split(const void* qkv_hi, const void* qkv_lo, const void* ctx_hi, const void* ctx_lo, const float* lse,
                              const void* dctx_hi, const void* dctx_lo, float* delta, void* dqkv_hi, void* dqkv_lo,
                              int B, int T, int P, int Tp, int H, int nh, void* stream);
/* The four entries above with a per-clip key count d_klen (device, B int32, clamped to [1, T] on the device; NULL = the entries
 * above, bit for bit).  Rows < d_klen[b] of clip b's ctx / lse / delta / dqkv are what the entries above write for that clip alone
 * at T = d_klen[b], bit for bit; rows [d_klen[b], T) of ctx and dqkv are zero bits; lse / delta there are not written. */
paa_status paa_attn_fwd_len(const void* qkv, void* ctx, float* lse, const int32_t* d_klen, int B, int T, int P, int Tp, int H,
                            int nh, void* stream);
paa_status paa_attn_bwd_len(const void* qkv, const void* ctx, const float* lse, const void* dctx, float* delta, void* dqkv,
                            const int32_t* d_klen, int B, int T, int P, int Tp, int H, int nh, void* stream);
paa_status paa_attn_fwd_split_len(const void* qkv_hi, const void* qkv_lo, void* ctx_hi, void* ctx_lo, float* lse,
                                  const int32_t* d_klen, int B, int T, int P, int Tp, int H, int nh, void* stream);
paa_status paa_attn_bwd_split_len(const void* qkv_hi, const void* qkv_lo, const void* ctx_hi, const void* ctx_lo, const float* lse,
                                  const void* dctx_hi, const void* dctx_lo, float* delta, void* dqkv_hi, void* dqkv_lo,
                                  const int32_t* d_klen, int B, int T, int P, int Tp, int H, int nh, void* stream);
paa_status paa_layernorm_fwd(const float* x, const float* g, const float* b, float* y, float* stats,
                             int rows, int cols, float eps, void* stream);
paa_status paa_layernorm_bwd(const float* dy, const float* x, const float* g, const float* stats, float* dx,
                             int rows, int cols, void* stream);
paa_status paa_softmax_fwd(float* s, int rows, int cols, int ld, float scale, void* stream);
paa_status paa_softmax_bwd(float* dp, const float* p, int rows, int cols, int ld, float scale, void* stream);
paa_status paa_ctc(const float* logits, const int32_t* labels, int B, int T, int V, int S_max, int blank,
                   float grad_scale, float* nll /* B */, float* dlogits /* may be NULL */, float* work, void* stream);
int64_t paa_ctc_work_floats(int B, int T, int V, int S_max);
/* paa_ctc with a per-clip frame count d_frames (device, B int32, clamped to [1, T] on the device; NULL = paa_ctc): clip b aligns
 * over its first d_frames[b] frames — nll[b] and dlogits rows < d_frames[b] are what paa_ctc gives for that clip alone at
 * T = d_frames[b], bit for bit — and dlogits rows beyond are zero.  The work buffer is sized for T (paa_ctc_work_floats). */
paa_status paa_ctc_len(const float* logits, const int32_t* labels, const int32_t* d_frames, int B, int T, int V, int S_max,
                       int blank, float grad_scale, float* nll /* B */, float* dlogits /* may be NULL */, float* work, void* stream);
/* rows [d_frames[b], T) of clip b of x (B, P, cols) f32 (nullable) and of its bf16 planes (hi, lo, il as below; nullable) become
 * zero; cols % 4 == 0 (il: % 32), P >= T. */
paa_status paa_zero_frames(float* x, void* hi, void* lo, int il, const int32_t* d_frames, int B, int T, int P, int cols,
                           void* stream);
/* The row kernels above with every option the model passes them.  A set of bf16 planes of an f32 result v is given as
 * (hi, lo, il): hi = bf16(v) round-to-nearest-even, lo = bf16(v - hi) (nullable: hi plane only), both uint16 arrays of the
 * result's shape; il != 0: ONE array of twice the elements at hi holds both planes interleaved per 32-element group,
 * [32 hi | 32 lo | 32 hi | ...] (element i at (i / 32) * 64 + i % 32, its lo part 32 further), lo is ignored; rows must then be
 * multiples of 32 elements (cols % 32 != 0, for paa_mul_gelu_grad_planes n % 32 != 0: PAA_ERR_ARG).  hi null = no planes.
 * paa_layernorm_fwd_planes: y nullable; yb planes of y; actb planes of gelu(y) and yact its f32 form (nullable each).
 * paa_layernorm_bwd_planes: dx = LN'(dy) + add (add nullable); dx nullable, and it may alias dy; dxb planes of dx.
 * cols % 4 != 0: PAA_ERR_ARG (as the entries above). */
paa_status paa_layernorm_fwd_planes(const float* x, const float* g, const float* b, float* y, float* stats,
                                    void* yb_hi, void* yb_lo, int yb_il, void* actb_hi, void* actb_lo, int actb_il,
                                    float* yact, int rows, int cols, float eps, void* stream);
paa_status paa_layernorm_bwd_planes(const float* dy, const float* x, const float* g, const float* stats, const float* add,
                                    float* dx, void* dxb_hi, void* dxb_lo, int dxb_il, int rows, int cols, void* stream);
/* n_mat matrices of rows_per_mat valid rows each, matrix i starting at row i * mat_rows_ld (mat_rows_ld >= rows_per_mat), row
 * stride ld >= cols.  Columns [cols, ld) of the valid rows are zeroed; the rows between two matrices are not touched. */
paa_status paa_softmax_fwd_mats(float* s, int n_mat, int rows_per_mat, int mat_rows_ld, int cols, int ld, float scale,
                                void* stream);
paa_status paa_softmax_bwd_mats(float* dp, const float* p, int n_mat, int rows_per_mat, int mat_rows_ld, int cols, int ld,
                                float scale, void* stream);
/* paa_ctc on logits / dlogits of (B, Tpad, V), Tpad >= T: frames [T, Tpad) of the logits are not read, those of dlogits and of
 * its planes dlb_hi / dlb_lo (planar, nullable; they need dlogits) are zeroed.  Two calls give the same bits. */
paa_status paa_ctc_padded(const float* logits, const int32_t* labels, int B, int T, int Tpad, int V, int S_max, int blank,
                          float grad_scale, float* nll /* B */, float* dlogits, void* dlb_hi, void* dlb_lo, float* work,
                          void* stream);
/* out = dy * gelu'(pre) over n elements, gelu'(x) = Phi(x) + x phi(x): f32 out (nullable) and / or planes of it. */
paa_status paa_mul_gelu_grad_planes(const float* dy, const float* pre, float* out, void* out_hi, void* out_lo, int out_il,
                                    int64_t n, void* stream);

/* ------------------------------------------------------ alignment-margin loss ----- */
/* Forced alignment of every clip's label row to its frames, and the Carlini-Wagner hinge on that alignment.  For clip b with
 * T_b = d_frames[b] frames (clamped to [1, T]; d_frames NULL: T), valid labels l_1..l_S (the non-negative entries of its row, in
 * order) and extended states e_0..e_2S = blank, l_1, blank, ..., blank:
 *   v_0(0) = z[0][blank], v_0(1) = z[0][l_1];   v_t(s) = z[t][e_s] + max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2))
 * on the RAW logits z in float64 (s-2 only where e_s != blank and e_s != e_{s-2}); among equal maxima the predecessor with the
 * largest state index wins (stay, then s-1, then s-2), and at the end state 2S wins over 2S-1.  pi_t = e_s of the path's state.
 *   m_t = (double)kappa + z[t][c*_t] - z[t][pi_t],   c*_t = the first maximum of z[t][c] over c != pi_t
 *   loss[b] = sum_{t < T_b} max(m_t, 0)                                (float64 sum in a fixed order, rounded once to f32)
 *   dlogits[t][c*_t] = +grad_scale, dlogits[t][pi_t] = -grad_scale on the frames with m_t > 0, every other entry 0
 * logits / dlogits are (B, Tpad, V) with Tpad >= T: frames [T, Tpad) of the logits are not read; rows t >= T_b and the pad rows of
 * dlogits and of its planar bf16 planes dlb_hi / dlb_lo (nullable; they need dlogits and a hi plane) are zeros.  A label row
 * that no path of T_b frames spells gives loss[b] = +inf, NaN in the clip's dlogits rows and the all-blank alignment; the other
 * clips are not affected.  align (B, T) int16 (nullable) receives pi, `blank` for t >= T_b.  dlogits NULL: forced aligner and
 * loss only.  labels (B, S_max) int32, values < V, negatives = padding anywhere in the row; 2 S_max + 1 <= 1024, 2 <= V <= 256,
 * T <= 8192.  work: paa_align_margin_work_floats(B, T, V, S_max) floats, 16-byte aligned.  Two calls give the same bits.
 * PAA_ERR_ARG: a null logits / labels / loss / work, planes without dlogits, kappa negative or not finite, a misaligned work
 * buffer; PAA_ERR_SIZE: a shape outside the ranges above.  Additions to ABI 350. */
int64_t paa_align_margin_work_floats(int B, int T, int V, int S_max);
paa_status paa_align_margin(const float* logits, const int32_t* labels, const int32_t* d_frames /* nullable */, int B, int T,
                            int Tpad, int V, int S_max, int blank, float kappa, float grad_scale, float* loss /* B */,
                            int16_t* align /* (B, T), nullable */, float* dlogits /* nullable */, void* dlb_hi, void* dlb_lo,
                            float* work, void* stream);
/* The loss of every later paa_model_fwd_bwd{,_rows} call, with or without a gradient: kind 0 = CTC (the default), 1 = the alignment
 * margin above with `kappa` (direction as grad_scale, the model's true clip lengths as d_frames).  The per-clip values land where
 * the CTC values do, so d_stats[0] = sum_b loss_b.  paa_model_forward{,_rows} keep reporting CTC.  Kind 0 restores bits identical
 * to a model that never had a loss set.  Kind 1 needs 2 S_max + 1 <= 1024 at the call (PAA_ERR_SIZE there).  Not itself
 * capturable (it changes what later calls launch).  PAA_ERR_ARG: a null model, another kind, kappa negative or not finite. */
paa_status paa_model_set_loss(paa_model* m, int kind, float kappa);

/* ------------------------------------------------------ feature-distance loss ----- */
/* Cosine distance between the rows of two hidden states, with its cotangent.  For clip b with T_b = d_frames[b] frames (clamped to
 * [1, T]; d_frames NULL: T) and the rows h = h[b][t], r = ref[b][t] of H floats:
 *   d[b][t]  = 1 - <h, r> / (|h| |r|)                           loss[b] = sum_{t < T_b} d[b][t]
 *   dh[b][t] = -grad_scale (r / |r| - cos h / |h|) / |h|        = grad_scale * d d[b][t] / d h
 * A row with |h| <= 1e-8 or |r| <= 1e-8 has d = 1 and a zero cotangent row (the definition, not an approximation).  The three dot
 * products are accumulated in float64 from the f32 inputs, d is rounded to f32 once, loss[b] is the float64 sum of those f32
 * values in a fixed order, rounded once; no atomics, so two calls give the same bits.  h and dh are (B, h_rows, H) with
 * h_rows >= T (the model's padded layout), ref is (B, ref_rows, H) with ref_rows >= T: rows [T, ..) of h and ref are not read, and
 * rows t >= T_b and the pad rows of dh are zeros.  dist (B, T), nullable, receives d (zeros for t >= T_b); dh nullable: loss only.
 * work: paa_feature_cos_work_floats(B, T) floats, 16-byte aligned.  PAA_ERR_ARG: a null h / ref / loss / work or a misaligned
 * work buffer; PAA_ERR_SIZE: B or T < 1, a row count below T, H not a multiple of 4 in [4, 4096].  Additions to ABI 350. */
int64_t paa_feature_cos_work_floats(int B, int T);
paa_status paa_feature_cos(const float* h, int h_rows, const float* ref, int ref_rows, const int32_t* d_frames /* nullable */,
                           int B, int T, int H, float grad_scale, float* loss /* B */, float* dist /* (B, T), nullable */,
                           float* dh /* (B, h_rows, H), nullable */, float* work, void* stream);
/* The last hidden state of the encoder (the output of its final LayerNorm, the operand of lm_head; HF
 * Wav2Vec2Model(...).last_hidden_state in eval mode) of B clips -> d_out (B, T_e, H) f32, dense.  d_clean / d_p / p_rows / clamp
 * as paa_model_forward_rows; under paa_model_set_lengths the rows t >= T_b are zeros.  The f32 copy of the hidden state lives in a
 * buffer that is allocated at the first call of this entry or of paa_model_set_feature_loss, so a model that never uses either is
 * launch for launch what it was; once the buffer exists the call is capturable.  The debug-read name "hfinal" reads that buffer
 * in the model's padded layout. */
paa_status paa_model_features(paa_model* m, const float* d_clean, const float* d_p /* nullable */, int p_rows, int clamp, int B,
                              float* d_out /* (B, T_e, H) */, void* stream);
/* d_ref (max_batch, T_e, H) f32 on the device switches the loss of every later paa_model_fwd_bwd{,_rows} call to the feature
 * distance above between the call's last hidden state and d_ref (direction as grad_scale, the model's true clip lengths as
 * d_frames); NULL switches it off and restores bits identical to a model that never had it set.  The pointer is KEPT and read on
 * the stream, so a replayed graph follows the buffer.  While it is set: d_stats[0] = sum_b loss[b] (the per-clip values land where
 * the CTC values do); d_labels may be NULL even with a gradient and is not read; the backward pass starts from dh at the hidden
 * state, without the lm_head input-gradient product; the logits are produced as ever.  paa_model_forward{,_rows} keep reporting
 * CTC.  Mutually exclusive with loss kind 1: each of the two setters returns PAA_ERR_ARG while the other loss is active.  Not
 * itself capturable. */
paa_status paa_model_set_feature_loss(paa_model* m, const float* d_ref);

#ifdef __cplusplus
}
#endif
#endif
