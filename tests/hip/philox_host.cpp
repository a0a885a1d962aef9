// Stand-alone host program over csrc/philox.h for tests/test_philox_host.py (no GPU, no HIP): one query per line of stdin, one
// line of results per query.  Integers are decimal, floats are printed with nine digits (a float32 round-trips).
//     philox c0 c1 c2 c3 k0 k1                  -> the four words, hexadecimal
//     input  NAME seed step clip stream group   -> counter words and key of one Philox call of the stream NAME (place / room / chan /
//                                                  noise), before the rounds: the stream table
//     place  seed step base B stream Lp on G    -> shift gain, per clip
//     room   seed step base B stream N          -> index, per clip
//     chan   seed step base B stream D lo hi    -> rq snr_db, per clip
//     normal seed step clip stream L            -> the L noise samples of one clip
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../psychoacoustic-adverserial-attacks_amd/csrc/philox.h"

using namespace paa;

static uint64_t u64() {
    uint64_t v = 0;
    if (scanf("%" SCNu64, &v) != 1) v = 0;
    return v;
}

static float f32() {
    double v = 0.0;
    if (scanf("%lf", &v) != 1) v = 0.0;
    return (float)v;
}

static void draw_words(uint32_t (&c)[4], uint64_t seed, uint32_t step, uint32_t clip, uint32_t stream, DrawTag tag) {
    const PhiloxKey k = key_of(seed);
    draw_counter(c, step, clip, stream, tag);
    philox4x32_10(c, k.k0, k.k1);
}

int main() {
    char cmd[16], name[16];
    uint32_t c[4];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "philox")) {
            for (uint32_t& w : c) w = (uint32_t)u64();
            const uint32_t k0 = (uint32_t)u64(), k1 = (uint32_t)u64();
            philox4x32_10(c, k0, k1);
            printf("%08x %08x %08x %08x", c[0], c[1], c[2], c[3]);
        } else if (!strcmp(cmd, "input")) {
            if (scanf("%15s", name) != 1) return 2;
            const PhiloxKey k = key_of(u64());
            const uint32_t step = (uint32_t)u64(), clip = (uint32_t)u64(), stream = (uint32_t)u64(), group = (uint32_t)u64();
            uint32_t k1 = k.k1;
            if (!strcmp(name, "noise")) {
                noise_counter(c, step, clip, group, stream);
                k1 = noise_k1(k1);
            } else {
                draw_counter(c, step, clip, stream, !strcmp(name, "place") ? TAG_PLACE : !strcmp(name, "room") ? TAG_ROOM : TAG_CHAN);
            }
            printf("%u %u %u %u %u %u", c[0], c[1], c[2], c[3], k.k0, k1);
        } else if (!strcmp(cmd, "place") || !strcmp(cmd, "room") || !strcmp(cmd, "chan")) {
            const uint64_t seed = u64();
            const uint32_t step = (uint32_t)u64(), base = (uint32_t)u64(), B = (uint32_t)u64(), stream = (uint32_t)u64();
            if (cmd[0] == 'p') {
                const int Lp = (int)u64(), on = (int)u64();
                const float G = f32();
                for (uint32_t b = 0; b < B; ++b) {
                    draw_words(c, seed, step, base + b, stream, TAG_PLACE);
                    printf("%d %.9g ", on ? draw_below(c[0], Lp) : 0, (double)draw_gain(c[1], G));
                }
            } else if (cmd[0] == 'r') {
                const int N = (int)u64();
                for (uint32_t b = 0; b < B; ++b) {
                    draw_words(c, seed, step, base + b, stream, TAG_ROOM);
                    printf("%d ", draw_below(c[0], N));
                }
            } else {
                const uint32_t D = (uint32_t)u64();
                const float lo = f32(), hi = f32();
                for (uint32_t b = 0; b < B; ++b) {
                    draw_words(c, seed, step, base + b, stream, TAG_CHAN);
                    printf("%" PRIu64 " %.9g ", draw_rq(c[0], D), (double)draw_snr(c[1], lo, hi));
                }
            }
        } else if (!strcmp(cmd, "normal")) {
            const PhiloxKey k = key_of(u64());
            const uint32_t step = (uint32_t)u64(), clip = (uint32_t)u64(), stream = (uint32_t)u64();
            const uint64_t L = u64();
            for (uint64_t g = 0; 4 * g < L; ++g) {
                noise_counter(c, step, clip, (uint32_t)g, stream);
                philox4x32_10(c, k.k0, noise_k1(k.k1));
                for (int p = 0; p < 2; ++p) {
                    float z[2];
                    normal_pair(c[2 * p], c[2 * p + 1], z[0], z[1]);
                    for (int q = 0; q < 2; ++q)
                        if (4 * g + 2 * p + q < L) printf("%.9g ", (double)z[q]);
                }
            }
        } else {
            fprintf(stderr, "philox_host: unknown query %s\n", cmd);
            return 2;
        }
        printf("\n");
    }
    return 0;
}
