// On-device greedy CTC decode + word error counters and the per-step stats log.
//
// paa_wer_counts restates core/loss_helpers.py greedy_decode_ids + wer_texts + wer_counts on integers: token ids go through a
// canon[V] table (-1 drop, 0 word delimiter, > 0 the code point of the lower-cased character), the references arrive as code
// points with every word terminated by 0.  One clip per workgroup, one wave per workgroup: every cross-lane step is a wave
// operation (ballot / popcount compaction, readlane of the last surviving id, a DPP prefix-min for the Levenshtein row) and the
// carries between 64-lane chunks stay in wave-uniform registers, so no step needs more than the LDS hand-off barrier.
#include "paa_common.h"

using namespace paa;

namespace {

constexpr int WER_T_MAX = 4096;        // frames per clip (a 30 s clip has 1499)
constexpr int WER_R_MAX = 8192;        // reference entries per clip (code points + terminators)
constexpr size_t WER_LDS_MAX = 64 * 1024;

__host__ __device__ inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

// LDS image of one clip: [ref R int32 | kept T int32 | d0, d1 (R + 1) u16 | rend R u16 | hstart, hend ceil(T / 2) u16]
struct WerLds {
    size_t ref, kept, d0, d1, rend, hstart, hend, total;
};
__host__ __device__ inline WerLds wer_lds(int T, int R) {
    WerLds o;
    size_t p = 0;
    o.ref = p;    p += al16(sizeof(int32_t) * (size_t)R);
    o.kept = p;   p += al16(sizeof(int32_t) * (size_t)T);
    o.d0 = p;     p += al16(sizeof(uint16_t) * (size_t)(R + 1));
    o.d1 = p;     p += al16(sizeof(uint16_t) * (size_t)(R + 1));
    o.rend = p;   p += al16(sizeof(uint16_t) * (size_t)R);
    o.hstart = p; p += al16(sizeof(uint16_t) * (size_t)((T + 1) / 2));
    o.hend = p;   p += al16(sizeof(uint16_t) * (size_t)((T + 1) / 2));
    o.total = p;
    return o;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// inclusive prefix-min over the 64 lanes: row_shr 1 / 2 / 4 / 8 scan each row of 16, row_bcast15 / row_bcast31 carry the row
// totals on.  A lane without a source (and a row the row mask excludes) reads `big`, the identity.
__device__ __forceinline__ int wave_prefix_min(int x) {
    constexpr int big = 0x3fffffff;
    x = min(x, __builtin_amdgcn_update_dpp(big, x, 0x111, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(big, x, 0x112, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(big, x, 0x114, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(big, x, 0x118, 0xf, 0xf, false));
    x = min(x, __builtin_amdgcn_update_dpp(big, x, 0x142, 0xa, 0xf, false));     // lane 15 -> row 1, lane 47 -> row 3
    x = min(x, __builtin_amdgcn_update_dpp(big, x, 0x143, 0xc, 0xf, false));     // lane 31 -> rows 2 and 3
    return x;
}

__global__ void __launch_bounds__(64) k_wer_counts(const int16_t* __restrict__ ids, int T, const int32_t* __restrict__ canon, int V,
                                                   const int32_t* __restrict__ refs, int R, int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const WerLds o = wer_lds(T, R);
    int32_t* s_ref = reinterpret_cast<int32_t*>(smem + o.ref);
    int32_t* s_kept = reinterpret_cast<int32_t*>(smem + o.kept);
    uint16_t* s_d0 = reinterpret_cast<uint16_t*>(smem + o.d0);
    uint16_t* s_d1 = reinterpret_cast<uint16_t*>(smem + o.d1);
    uint16_t* s_rend = reinterpret_cast<uint16_t*>(smem + o.rend);
    uint16_t* s_hstart = reinterpret_cast<uint16_t*>(smem + o.hstart);
    uint16_t* s_hend = reinterpret_cast<uint16_t*>(smem + o.hend);
    const int b = blockIdx.x, lane = threadIdx.x;
    const int16_t* idr = ids + (size_t)b * T;
    const int32_t* rr = refs + (size_t)b * R;

    // ---- hypothesis: drop the specials first, then keep a frame iff its id differs from the previous SURVIVING frame's id
    int n_kept = 0;
    int last_id = -1;                          // id of the last surviving frame of the chunks behind (wave-uniform)
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        int id = -1, c = -1;
        if (t < T) {
            id = idr[t];
            if (id >= 0 && id < V) c = canon[id];
        }
        const bool alive = c >= 0;
        const unsigned long long am = __ballot(alive);
        const unsigned long long before = am & lanes_below(lane);
        const int src = before ? 63 - __clzll(before) : lane;
        const int got = __shfl(id, src, 64);
        const int prev = before ? got : last_id;
        const bool keep = alive && id != prev;
        const unsigned long long km = __ballot(keep);
        if (keep) s_kept[n_kept + __popcll(km & lanes_below(lane))] = c;
        n_kept += __popcll(km);
        if (am) last_id = __shfl(id, 63 - __clzll(am), 64);
    }
    // ---- reference row: the row ends at its first negative entry; every 0 before that terminates one word
    int n_rw = 0;
    bool open = true;
    for (int k0 = 0; k0 < R && open; k0 += 64) {
        const int k = k0 + lane;
        const int v = k < R ? rr[k] : -1;
        const unsigned long long neg = __ballot(v < 0);
        const bool live = !(neg & (lanes_below(lane) | (1ull << lane)));      // no negative entry at or before this lane
        if (k < R) s_ref[k] = v;
        const bool term = live && v == 0;
        const unsigned long long tm = __ballot(term);
        if (term) s_rend[n_rw + __popcll(tm & lanes_below(lane))] = (uint16_t)k;
        n_rw += __popcll(tm);
        open = neg == 0;
    }
    __syncthreads();
    // ---- hypothesis words: maximal runs of non-delimiter kept tokens; starts and ends are numbered by their own running counts
    int n_hw = 0, n_he = 0;
    for (int k0 = 0; k0 < n_kept; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < n_kept;
        const bool tok = in && s_kept[k] != 0;
        const bool starts = tok && (k == 0 || s_kept[k - 1] == 0);
        const bool ends = tok && (k == n_kept - 1 || s_kept[k + 1] == 0);
        const unsigned long long sm = __ballot(starts), em = __ballot(ends);
        if (starts) s_hstart[n_hw + __popcll(sm & lanes_below(lane))] = (uint16_t)k;
        if (ends) s_hend[n_he + __popcll(em & lanes_below(lane))] = (uint16_t)(k + 1);
        n_hw += __popcll(sm);
        n_he += __popcll(em);
    }
    // ---- Levenshtein over words, one row per hypothesis word, lanes over the reference words
    for (int j = lane; j <= n_rw; j += 64) s_d0[j] = (uint16_t)j;
    __syncthreads();
    uint16_t* dp = s_d0;
    uint16_t* dn = s_d1;
    for (int i = 1; i <= n_hw; ++i) {
        const int hs = s_hstart[i - 1], hl = s_hend[i - 1] - hs;
        int carry = i;                                        // d[i][0] - 0
        for (int j0 = 1; j0 <= n_rw; j0 += 64) {
            const int j = j0 + lane;
            const bool in = j <= n_rw;
            int x = 0x3fffffff;
            if (in) {
                const int rs = j == 1 ? 0 : s_rend[j - 2] + 1;
                const int rl = s_rend[j - 1] - rs;
                bool same = rl == hl;
                for (int k = 0; same && k < hl; ++k) same = s_kept[hs + k] == s_ref[rs + k];
                x = min((int)dp[j] + 1, (int)dp[j - 1] + (same ? 0 : 1)) - j;
            }
            // d[j] = min(t[j], d[j - 1] + 1)  <=>  d[j] - j = min over k <= j of (t[k] - k), the carry being d[j0 - 1] - (j0 - 1)
            x = min(wave_prefix_min(x), carry);
            if (in) dn[j] = (uint16_t)(x + j);
            carry = __shfl(x, 63, 64);
        }
        if (lane == 0) dn[0] = (uint16_t)i;
        __syncthreads();
        uint16_t* t = dp; dp = dn; dn = t;
    }
    if (lane == 0) {
        counts[b * 3 + 0] = dp[n_rw];
        counts[b * 3 + 1] = n_rw;
        counts[b * 3 + 2] = n_hw;
    }
}

// sums[0] = sum_b errors, sums[1] = sum_b reference words: integer sums converted once, so the floats are exact and the same in
// every run (no atomics)
__global__ void __launch_bounds__(64) k_wer_sums(const int32_t* __restrict__ counts, int B, float* __restrict__ sums) {
    int e = 0, w = 0;
    for (int b = threadIdx.x; b < B; b += 64) {
        e += counts[b * 3 + 0];
        w += counts[b * 3 + 1];
    }
    e = wave_sum(e);
    w = wave_sum(w);
    if (threadIdx.x == 0) {
        sums[0] = (float)e;
        sums[1] = (float)w;
    }
}

__global__ void __launch_bounds__(64) k_stats_push(const float* __restrict__ stats, int n, float* __restrict__ log,
                                                   int32_t* __restrict__ cursor, int cap) {
    const unsigned cur = (unsigned)*cursor;
    const size_t row = cur % (unsigned)cap;
    for (int i = threadIdx.x; i < n; i += 64) log[row * n + i] = stats[i];
    __syncthreads();                          // every lane has read the cursor
    if (threadIdx.x == 0) *cursor = (int32_t)(cur + 1u);
}

}  // namespace

extern "C" paa_status paa_wer_counts(const int16_t* d_ids, int B, int T, const int32_t* d_canon, int V, const int32_t* d_refs,
                                     int R_cap, int32_t* d_counts, float* d_sums, void* stream) {
    if (!d_ids || !d_canon || !d_refs || !d_counts) PAA_FAIL(PAA_ERR_ARG, "paa_wer_counts: null argument");
    if (B <= 0) PAA_FAIL(PAA_ERR_ARG, "paa_wer_counts: B=%d", B);
    if (V < 1 || V > 32767) PAA_FAIL(PAA_ERR_ARG, "paa_wer_counts: V=%d outside [1, 32767]", V);
    if (T < 1 || T > WER_T_MAX) PAA_FAIL(PAA_ERR_SIZE, "paa_wer_counts: T=%d frames outside [1, %d]", T, WER_T_MAX);
    if (R_cap < 1 || R_cap > WER_R_MAX)
        PAA_FAIL(PAA_ERR_SIZE, "paa_wer_counts: R_cap=%d reference entries outside [1, %d]", R_cap, WER_R_MAX);
    const WerLds o = wer_lds(T, R_cap);
    if (o.total > WER_LDS_MAX)
        PAA_FAIL(PAA_ERR_SIZE, "paa_wer_counts: T=%d with R_cap=%d needs %zu bytes of LDS, the limit is %zu", T, R_cap, o.total,
                 WER_LDS_MAX);
    hipLaunchKernelGGL(k_wer_counts, dim3(B), dim3(64), o.total, (hipStream_t)stream, d_ids, T, d_canon, V, d_refs, R_cap, d_counts);
    PAA_LAUNCH_CHECK();
    if (d_sums) {
        hipLaunchKernelGGL(k_wer_sums, dim3(1), dim3(64), 0, (hipStream_t)stream, d_counts, B, d_sums);
        PAA_LAUNCH_CHECK();
    }
    return PAA_OK;
}

extern "C" paa_status paa_stats_push(const float* d_stats, int n, float* d_log, int32_t* d_cursor, int cap, void* stream) {
    if (!d_stats || !d_log || !d_cursor) PAA_FAIL(PAA_ERR_ARG, "paa_stats_push: null argument");
    if (n < 1 || n > 64 || cap < 1) PAA_FAIL(PAA_ERR_ARG, "paa_stats_push: n=%d (1..64) cap=%d (>= 1)", n, cap);
    hipLaunchKernelGGL(k_stats_push, dim3(1), dim3(64), 0, (hipStream_t)stream, d_stats, n, d_log, d_cursor, cap);
    PAA_LAUNCH_CHECK();
    return PAA_OK;
}
