// The random draws of the playback chain ("The playback chain"): Philox4x32-10, the table that keeps the chain's four
// random streams apart, the arithmetic that turns Philox words into a clip's draw, and the one-block draw kernel's counter
// protocol.  Everything but that protocol compiles with a plain C++ compiler too, so the generator, the table and the draws of
// the three links are checked on the host (tests/hip/philox_host.cpp).  The noise samples are not: normal_pair takes other
// trigonometric functions on the host, and the formula the device runs is covered by the GPU tests alone.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PAA_HD __host__ __device__ __forceinline__
#else
#define PAA_HD inline
#endif

namespace paa {

PAA_HD void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// Philox4x32-10 (Salmon et al. 2011): ten rounds, the key bumped by the Weyl constants between them
PAA_HD void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// ---- the stream table --------------------------------------------------------------------------------------------------------
//     stream            key                    counter (word 0, 1, 2, 3)
//     placement draw    (k0, k1)               (step, clip, stream_id, TAG_PLACE)
//     room draw         (k0, k1)               (step, clip, stream_id, TAG_ROOM)
//     channel draw      (k0, k1)               (step, clip, stream_id, TAG_CHAN)
//     noise samples     (k0, k1 ^ NOISE_KEY)   (step, clip, i >> 2,    stream_id)
// with (k0, k1) the halves of the run's seed, clip the global clip id and stream_id 0 for training, 1 for evaluation.  No
// (counter, key) pair of one stream equals a pair of another: the three draws share the key and differ in counter word 3, and
// the noise, whose word 3 is free, differs from all three in the key, since NOISE_KEY != 0 flips bits of k1 for every seed.
enum DrawTag : uint32_t { TAG_PLACE = 0, TAG_ROOM = 1, TAG_CHAN = 2 };
constexpr uint32_t NOISE_KEY = 0x6E6F6973u;      // "nois"

struct PhiloxKey {
    uint32_t k0, k1;
};

inline PhiloxKey key_of(uint64_t seed) { return {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)}; }

PAA_HD uint32_t noise_k1(uint32_t k1) { return k1 ^ NOISE_KEY; }

PAA_HD void draw_counter(uint32_t (&c)[4], uint32_t step, uint32_t clip, uint32_t stream_id, DrawTag tag) {
    c[0] = step; c[1] = clip; c[2] = stream_id; c[3] = tag;
}

// group = i >> 2: one Philox block gives the four normals of samples 4 group .. 4 group + 3
PAA_HD void noise_counter(uint32_t (&c)[4], uint32_t step, uint32_t clip, uint32_t group, uint32_t stream_id) {
    c[0] = step; c[1] = clip; c[2] = group; c[3] = stream_id;
}

// ---- a clip's draw from its Philox words -------------------------------------------------------------------------------------
// 24 bits of a word: exact in f32, u in [0, 1)
PAA_HD float unit24(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

// uniform in [0, n): the shift of a placement (n = Lp) and the room of a bank (n = N)
PAA_HD int32_t draw_below(uint32_t w, int n) { return (int32_t)(((uint64_t)w * (uint64_t)(uint32_t)n) >> 32); }

// uniform in [-G, +G] dB as a factor; log2(10) / 20; gain_db = 0 -> exactly 1.0f
PAA_HD float draw_gain(uint32_t w, float gain_db) {
    const float db = fmaf(unit24(w), 2.0f * gain_db, -gain_db);
    return exp2f(db * 0.16609640474436813f);
}

// the clock ratio in Q32, uniform in 2^32 +- D, pure integers (arithmetic shift: floor)
PAA_HD uint64_t draw_rq(uint32_t w, uint32_t drift_q32) {
    const int64_t d = (((int64_t)w - ((int64_t)1 << 31)) * (int64_t)drift_q32) >> 31;
    return (uint64_t)(((int64_t)1 << 32) + d);
}

PAA_HD float draw_snr(uint32_t w, float snr_lo, float snr_hi) { return fmaf(unit24(w), snr_hi - snr_lo, snr_lo); }

// Box-Muller on a word pair: u1 in (0, 1], u2 in [0, 1) -> two standard normals (the even and the odd sample of the pair).  The
// host build has no cospif / sinpif and takes libm's cosf / sinf of 2 pi u2: the same pair to a few units of float32.
PAA_HD void normal_pair(uint32_t wa, uint32_t wb, float& z_even, float& z_odd) {
    const float u1 = (float)((wa >> 8) + 1u) * 0x1p-24f;
    const float u2 = unit24(wb);
    const float rad = sqrtf(-2.0f * logf(u1));
#ifdef __HIP_DEVICE_COMPILE__
    z_even = rad * cospif(2.0f * u2);
    z_odd = rad * sinpif(2.0f * u2);
#else
    z_even = rad * cosf(6.283185307179586f * u2);
    z_odd = rad * sinf(6.283185307179586f * u2);
#endif
}

#ifdef __HIPCC__
// ---- the draw kernels' counter protocol --------------------------------------------------------------------------------------
// A draw is ONE block of DRAW_NT threads: it reads the step from ``counter`` in device memory, hands body(b, words) the Philox
// words of every clip b < B of the stream ``tag``, and advances the counter once every thread has read it, so that a captured
// graph draws anew on every replay.
constexpr int DRAW_NT = 256;

template <class Body>
__device__ __forceinline__ void draw_clips(uint32_t k0, uint32_t k1, int32_t* __restrict__ counter, int stream_id, int clip_base,
                                           int B, DrawTag tag, Body body) {
    const uint32_t step = (uint32_t)*counter;
    for (int b = threadIdx.x; b < B; b += DRAW_NT) {
        uint32_t c[4];
        draw_counter(c, step, (uint32_t)(clip_base + b), (uint32_t)stream_id, tag);
        philox4x32_10(c, k0, k1);
        body(b, c);
    }
    __syncthreads();                          // every thread has read the counter
    if (threadIdx.x == 0) *counter = (int32_t)(step + 1u);
}
#endif

}  // namespace paa
