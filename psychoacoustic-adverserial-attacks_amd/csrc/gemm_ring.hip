// LDS-DMA ring GEMM kernels for gfx950 (see gemm.h for the contract, gemm_dev.h for the shared epilogues).
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "gemm_dev.h"

namespace paa {

// ---- LDS-DMA ring kernel: 256 x (256|128) tiles, one 8-wave workgroup per CU ------------------------------------------
// The large products of the step (conv stack, FFN, QKV) at the operand cost per FLOP of a 256 x 256 bf16 tile (or a
// 256 x 128 split-bf16 tile: three MFMAs per operand pair make it equally dense).  Operand K slabs go global -> LDS by
// global_load_lds_dwordx4 (no staging registers, no ds_write) into a ring of NST stages; the load cursor runs NST - 1
// stages ahead of the MFMAs over the flat (output tile, K slab) sequence of this persistent workgroup, so tile
// boundaries do not drain it; ONE workgroup barrier per stage, and a COUNTED s_waitcnt vmcnt in front of it keeps the
// younger stages in flight across the barrier (a stage has NST - 2 whole compute stages to land; the 2-stage form of
// round 1 waited vmcnt(0) every K tile and exposed the DMA's issue-to-landed time).  The DMA writes LDS lane-linearly, so
// the bank-conflict swizzle lives on the SOURCE side: slot p of LDS row r receives global chunk p ^ f(r), and the
// fragment reads apply the same XOR (f = (r >> 1) & 7 for 128-byte rows, (r >> 2) & 3 for 64-byte rows: every
// ds_read_b128 lane group then covers all 64 banks).  B rows are permuted inside each 64-row group exactly as
// store_bf<PERM> does, for the vector epilogue.  Stage layout: A_hi rows | B_hi rows [| A_lo rows | B_lo rows].
// Everything diagnostic in this file — the clock stamps, the ablation bits, the MFMA-shape probe and every ring configuration the
// automatic selection of gemm.hip cannot reach — is compiled only with -DPAA_EXPERIMENTS (tools/*.sh pass it through
// PAA_EXTRA_HIPCC_FLAGS).  The shipped library holds configurations 7 and 8 (192 x 128, two workgroups per CU) from this file.
#if (defined(PAA_CLOCK_STAMP) || defined(PAA_ABL)) && !defined(PAA_EXPERIMENTS)
#error "PAA_CLOCK_STAMP / PAA_ABL are diagnostic builds: add -DPAA_EXPERIMENTS"
#endif
#ifdef PAA_CLOCK_STAMP
// Diagnostic build only (tools/clock_probe.py): shader-clock ticks and 100 MHz real-time ticks around each workgroup's
// whole tile loop, written to a buffer of their own that nothing else reads (MI355X_MICROARCH.md, DVFS give-back item 6).
__device__ unsigned long long g_clock_stamp[2 * 1024];
#endif
// Diagnostic builds only (tools/gemm_ablate.sh, never the shipped library): -DPAA_ABL=<bits> removes parts of the kernel to price
// them — 1: no epilogue (the accumulators are only summed), 2: no operand DMA, 4: no workgroup barrier, 8: no fragment reads
// inside the K loop.  Results are WRONG under any bit.
#ifndef PAA_ABL
#define PAA_ABL 0
#endif
typedef __attribute__((address_space(1))) const void* gas_ptr;
typedef __attribute__((address_space(3))) void* las_ptr;
template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// AHEAD: the barrier of iteration `it` certifies stage it + 1 (not just `it`), so the first fragments of the NEXT stage can
// be read from LDS under the last MFMAs of the current one and the MFMAs after a barrier start at once instead of
// waiting out an LDS round trip that all eight lock-stepped waves would sit through together; costs one stage of
// prefetch distance (NST - 2 stages in flight instead of NST - 1).
// MF16 (probe, WRONG RESULTS): every 32x32x16 MFMA replaced by two 16x16x32 MFMAs of the same flops on the same fragments,
// to time the MFMA shape inside this loop before investing in a 16x16 fragment layout and epilogue.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <bool MF16>
__device__ __forceinline__ void mfma_step(const bf16x8& a, const bf16x8& b, f32x16& c) {
    if constexpr (!MF16) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    } else {
        f32x4 lo = {c[0], c[1], c[2], c[3]}, hi = {c[4], c[5], c[6], c[7]};
        lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, lo, 0, 0, 0);
        hi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, hi, 0, 0, 0);
        c[0] = lo[0]; c[1] = lo[1]; c[2] = lo[2]; c[3] = lo[3]; c[4] = hi[0]; c[5] = hi[1]; c[6] = hi[2]; c[7] = hi[3];
    }
}

template <int BM, int BN, int BK, int PREC, int NST, int WR, int WC, bool AHEAD, int WPS = 2, bool MF16 = false>
__global__ __launch_bounds__(WR * WC * 64, WPS) void k_gemm_ring(GemmArgs g) {
    constexpr int NW = WR * WC;
    constexpr int NPL = PREC ? 2 : 1;
    constexpr int RB = BK * 2;                 // bytes per LDS row (one plane)
    constexpr int CPR = RB / 16;               // 16-byte chunks per row
    constexpr int RPI = 1024 / RB;             // rows per DMA wave-instruction
    constexpr int RBR = 256 / RB;              // rows per 256-byte bank row
    constexpr int PROWS = BM + BN;             // rows of one plane
    constexpr int ROWS = PROWS * NPL;
    constexpr int STAGE = ROWS * RB;
    constexpr int GPW = ROWS / RPI / NW;       // DMA wave-instructions per wave per stage
    constexpr int MI = BM / WR / 32, NJ = BN / WC / 32, KS = BK / 16;
    constexpr int D = NST - 1;                 // stages in flight ahead of the MFMAs
    static_assert(NJ == 2 || NJ == 4, "vector epilogue: 64-column groups per wave");
    static_assert(ROWS % (RPI * NW) == 0 && PROWS % RPI == 0 && BM % RPI == 0, "a DMA wave-instruction must not straddle operands or planes");
    static_assert(NST * STAGE <= 160 * 1024 && D >= 1 && D <= 3 && D * GPW < 64, "ring does not fit");
    static_assert(!AHEAD || D >= 2, "certifying one stage ahead needs two stages of lookahead");
    __shared__ __attribute__((aligned(1024))) unsigned char smem[NST * STAGE];

    const paa_gemm_desc& d = g.d;
    const int nwg = g.tiles_m * g.tiles_n;
    const int total = nwg * d.batch;
    const int nk = d.K / BK;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WC, wc = wave % WC;
    const int lr = lane & 31, lh = lane >> 5;

    struct Tile { int m0, n0, z1, z2; };
    auto decode = [&](int t) {
        Tile c;
        const int z = t / nwg, orig = t - z * nwg;
        const int q = nwg >> 3, r8 = nwg & 7, xcd = orig & 7;
        const int id = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (orig >> 3);
        const int tm = id / g.tiles_n, tn = id - tm * g.tiles_n;
        c.m0 = tm * BM; c.n0 = tn * BN;
        c.z1 = z / d.batch2; c.z2 = z - c.z1 * d.batch2;
        return c;
    };

    // ---- load cursor: (tile lt, K slab lk) is the next stage to request --------------------------------------------
    int lt = blockIdx.x, lk = 0;
    if (lt >= total) return;
    // k_group order of the K slabs (gemm.h): kg_spt slabs per tap, kg_taps taps; 0 = plain K order
    const int kg_spt = (d.k_group > 0 && d.k_group % BK == 0 && d.K % d.k_group == 0 && d.K > d.k_group) ? d.k_group / BK : 0;
    const int kg_taps = kg_spt ? d.K / d.k_group : 1;
    int ltap = 0, lc = 0, lslab = 0;           // (tap, channel slab) and K slab index of the next stage to request
    const unsigned short* src[GPW];
    auto set_src = [&](int t) {
        const Tile c = decode(t);
        const int64_t aoff = c.z1 * d.a_s1 + c.z2 * d.a_s2, boff = c.z1 * d.b_s1 + c.z2 * d.b_s2;
#pragma unroll
        for (int i = 0; i < GPW; ++i) {
            const int r = (i * NW + wave) * RPI + lane / CPR;             // ring row of this lane's chunk
            const int pl = r / PROWS;                                      // plane (0 = hi, 1 = lo)
            const int rr = r - pl * PROWS;                                 // row inside the plane: A rows, then B rows
            const int ch = (lane % CPR) ^ ((r / RBR) & (CPR - 1));        // global chunk that lands in slot lane % CPR
            if (rr < BM) {
                const unsigned short* A = reinterpret_cast<const unsigned short*>(pl ? d.A_lo : (const void*)d.A) + aoff;
                src[i] = A + (int64_t)min(c.m0 + rr, d.M - 1) * d.lda + ch * 8;
            } else {
                const unsigned short* B = reinterpret_cast<const unsigned short*>(pl ? d.B_lo : (const void*)d.B) + boff;
                const int p = rr - BM;
                const int nl = (p & ~63) + 8 * ((p & 31) >> 2) + 4 * ((p >> 5) & 1) + (p & 3);
                src[i] = B + (int64_t)min(c.n0 + nl, d.N - 1) * d.ldb + ch * 8;
            }
        }
    };
    auto issue = [&](int slot) {
        unsigned char* st = smem + slot * STAGE;
        if (!(PAA_ABL & 2)) {
#pragma unroll
            for (int i = 0; i < GPW; ++i)
                __builtin_amdgcn_global_load_lds((gas_ptr)(src[i] + (int64_t)lslab * BK), (las_ptr)(st + (i * NW + wave) * 1024), 16, 0, 0);
        }
        if (kg_spt) {
            if (++ltap == kg_taps) { ltap = 0; ++lc; }
            lslab = ltap * kg_spt + lc;
        } else {
            ++lslab;
        }
        if (++lk == nk) {
            lk = 0; ltap = 0; lc = 0; lslab = 0;
            lt += gridDim.x;
            if (lt < total) set_src(lt);
        }
    };
    set_src(lt);
    int pend = 0, islot = 0;                   // stages requested and not yet consumed; next slot to fill
#pragma unroll
    for (int s = 0; s < D; ++s)
        if (lt < total) { issue(islot); islot = islot + 1 == NST ? 0 : islot + 1; ++pend; }

    // fragment addressing: row base + swizzled 16-byte chunk of the k slice
    const int sw = (lr / RBR) & (CPR - 1);
    int offk[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) offk[ks] = ((2 * ks + lh) ^ sw) << 4;
    const int arow = (wr * (BM / WR) + lr) * RB, brow = (BM + wc * (BN / WC) + lr) * RB;
    constexpr int LO = PROWS * RB;             // hi -> lo plane distance inside a stage

#ifdef PAA_CLOCK_STAMP
    const unsigned long long stamp_t0 = __builtin_amdgcn_s_memtime(), stamp_r0 = __builtin_amdgcn_s_memrealtime();
#endif
    int cslot = 0;                             // slot of the stage the MFMAs consume next
    constexpr int NM = NJ * (PREC ? 3 : 1);
    bf16x8 bh[NJ], bl[NJ], bhn[NJ], bln[NJ], ah, al, ahn, aln;
    auto first_frags = [&](int slot) {         // the fragments the first MFMA group of a stage needs -> the "next" registers
        const unsigned char* sa = smem + slot * STAGE + arow;
        const unsigned char* sb = smem + slot * STAGE + brow;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            bhn[j] = *reinterpret_cast<const bf16x8*>(sb + j * 32 * RB + offk[0]);
            if (PREC) bln[j] = *reinterpret_cast<const bf16x8*>(sb + LO + j * 32 * RB + offk[0]);
        }
        ahn = *reinterpret_cast<const bf16x8*>(sa + offk[0]);
        if (PREC) aln = *reinterpret_cast<const bf16x8*>(sa + LO + offk[0]);
    };
    if constexpr (AHEAD) {                     // stages 0 and 1 landed everywhere; stage 0's first fragments in registers
        if (pend >= 3) wait_vmcnt<(D >= 3 ? 1 : 0) * GPW>(); else wait_vmcnt<0>();
        __builtin_amdgcn_sched_barrier(0);
        if (!(PAA_ABL & 4)) __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        first_frags(0);
    }
    bool first_it = true;
    bool first_abl = true;
    (void)first_abl;
    for (int t = blockIdx.x; t < total; t += gridDim.x) {
        const Tile cur = decode(t);
        f32x16 acc[NJ / 2][MI][2];             // [64-column group][row block][column block]: one epilogue_vec per group
#pragma unroll
        for (int h = 0; h < NJ / 2; ++h)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[h][i][j][e] = 0.f;

        for (int kt = 0; kt < nk; ++kt) {
            if constexpr (AHEAD) {
                // stage `cslot` was certified by the previous barrier; this one certifies the stage after it
                if (!first_it) {
                    if (pend >= 3) wait_vmcnt<(D >= 3 ? 1 : 0) * GPW>(); else wait_vmcnt<0>();
                    __builtin_amdgcn_sched_barrier(0);
                    if (!(PAA_ABL & 4)) __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                }
                first_it = false;
            } else {
                // my pieces of the oldest pending stage have landed; the younger ones stay in flight across the barrier
                if (pend >= 3) wait_vmcnt<(D >= 3 ? 2 : 0) * GPW>();
                else if (pend == 2) wait_vmcnt<(D >= 2 ? 1 : 0) * GPW>();
                else wait_vmcnt<0>();
                __builtin_amdgcn_sched_barrier(0);
                if (!(PAA_ABL & 4)) __builtin_amdgcn_s_barrier();      // everyone's have; everyone is done reading the slot refilled next
                __builtin_amdgcn_sched_barrier(0);
            }
            if (lt < total) { issue(islot); islot = islot + 1 == NST ? 0 : islot + 1; } else --pend;
            const unsigned char* sa = smem + cslot * STAGE + arow;
            const unsigned char* sb = smem + cslot * STAGE + brow;
            cslot = cslot + 1 == NST ? 0 : cslot + 1;
            if constexpr (AHEAD) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) { bh[j] = bhn[j]; bl[j] = bln[j]; }
                ah = ahn; al = aln;
            } else if ((PAA_ABL & 8) && !first_abl) {
                // fragments stay what they were
            } else {
                first_abl = false;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    bh[j] = *reinterpret_cast<const bf16x8*>(sb + j * 32 * RB + offk[0]);
                    if (PREC) bl[j] = *reinterpret_cast<const bf16x8*>(sb + LO + j * 32 * RB + offk[0]);
                    bhn[j] = bh[j]; bln[j] = bl[j];
                }
                ah = *reinterpret_cast<const bf16x8*>(sa + offk[0]);
                if (PREC) al = *reinterpret_cast<const bf16x8*>(sa + LO + offk[0]);
                ahn = ah; aln = al;
                __builtin_amdgcn_sched_group_barrier(0x100, (NJ + 1) * NPL, 0);
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int i = 0; i < MI; ++i) {
                    const int ni = (i + 1 < MI) ? i + 1 : 0, nks = (i + 1 < MI) ? ks : ks + 1;
                    if ((PAA_ABL & 8)) {
                    } else if (nks < KS) {
                        ahn = *reinterpret_cast<const bf16x8*>(sa + ni * 32 * RB + offk[nks < KS ? nks : 0]);
                        if (PREC) aln = *reinterpret_cast<const bf16x8*>(sa + LO + ni * 32 * RB + offk[nks < KS ? nks : 0]);
                        if (ni == 0) {
#pragma unroll
                            for (int j = 0; j < NJ; ++j) {
                                bhn[j] = *reinterpret_cast<const bf16x8*>(sb + j * 32 * RB + offk[nks < KS ? nks : 0]);
                                if (PREC) bln[j] = *reinterpret_cast<const bf16x8*>(sb + LO + j * 32 * RB + offk[nks < KS ? nks : 0]);
                            }
                        }
                    } else if constexpr (AHEAD) {
                        first_frags(cslot);            // next stage (certified by this iteration's barrier); garbage after the last one
                    }
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        if (PREC) {
                            mfma_step<MF16>(al, bh[j], acc[j >> 1][i][j & 1]);
                            mfma_step<MF16>(ah, bl[j], acc[j >> 1][i][j & 1]);
                        }
                        mfma_step<MF16>(ah, bh[j], acc[j >> 1][i][j & 1]);
                    }
                    __builtin_amdgcn_s_setprio(0);
                    if (nks < KS) {
                        if (ni == 0) __builtin_amdgcn_sched_group_barrier(0x100, (NJ + 1) * NPL, 0);
                        else __builtin_amdgcn_sched_group_barrier(0x100, NPL, 0);
                    } else if constexpr (AHEAD) {
                        __builtin_amdgcn_sched_group_barrier(0x100, (NJ + 1) * NPL, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
                    if (nks < KS) {
                        ah = ahn; al = aln;
                        if (ni == 0) {
#pragma unroll
                            for (int j = 0; j < NJ; ++j) { bh[j] = bhn[j]; bl[j] = bln[j]; }
                        }
                    }
                }
        }
        if (PAA_ABL & 1) {
            float sum = 0.f;
#pragma unroll
            for (int h = 0; h < NJ / 2; ++h)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) sum += acc[h][i][j][e];
            if (sum == 12345.678f && d.Cb) reinterpret_cast<unsigned short*>(d.Cb)[lane] = 1;
            continue;
        }
        epilogue_vec<MI, true>(d, acc[0], cur.m0 + wr * (BM / WR), cur.n0 + wc * (BN / WC), cur.z1, cur.z2, lane);
        if constexpr (NJ == 4)      // (written out: a loop over the groups is not unrolled and sends the accumulators through scratch)
            epilogue_vec<MI, true>(d, acc[1], cur.m0 + wr * (BM / WR), cur.n0 + wc * (BN / WC) + 64, cur.z1, cur.z2, lane);
    }
#ifdef PAA_CLOCK_STAMP
    if (tid == 0 && blockIdx.x < 1024) {
        g_clock_stamp[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - stamp_t0;
        g_clock_stamp[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - stamp_r0;
    }
#endif
}

template <int BM, int BN, int BK, int PREC, int NST, int WR, int WC, bool AHEAD, int WPS = 2, bool MF16 = false>
static void launch_ring(const GemmArgs& g, hipStream_t st) {
    static const int per_cu = blocks_per_cu(k_gemm_ring<BM, BN, BK, PREC, NST, WR, WC, AHEAD, WPS, MF16>, WR * WC * 64);
    const int resident = per_cu * device_cus();
    const int total = g.tiles_m * g.tiles_n * g.d.batch;
    const int blocks = resident > 0 ? std::min(total, resident) : total;
    hipLaunchKernelGGL((k_gemm_ring<BM, BN, BK, PREC, NST, WR, WC, AHEAD, WPS, MF16>), dim3(blocks), dim3(WR * WC * 64), 0, st, g);
}

void launch_ring_cfg(int cfg, const GemmArgs& g, hipStream_t st) {
    switch (cfg) {
        case 7: launch_ring<192, 128, 32, 1, 2, 2, 2, false, 2>(g, st); break;  // split, 192-row tiles, 2 x 40 KB, two workgroups per CU
        case 8: launch_ring<192, 128, 64, 0, 2, 2, 2, false, 2>(g, st); break;  // bf16, 192-row tiles, 2 x 40 KB, two workgroups per CU
#ifdef PAA_EXPERIMENTS      // measured and not selected; results equal to the shipped kernels except 9 / 10
        case 2: launch_ring<256, 256, 64, 0, 2, 2, 4, false>(g, st); break;     // bf16, 2 stages of 64 KB (the round-1 structure)
        case 3: launch_ring<256, 256, 32, 0, 4, 2, 4, false>(g, st); break;     // bf16, 4 stages of 32 KB, 3 in flight
        case 4: launch_ring<256, 128, 32, 1, 3, 4, 2, false>(g, st); break;     // split, 3 stages of 48 KB, 2 in flight
        case 5: launch_ring<256, 256, 32, 0, 4, 2, 4, true>(g, st); break;      // bf16, 4 stages, certified one ahead
        case 6: launch_ring<256, 128, 32, 1, 3, 4, 2, true>(g, st); break;      // split, 3 stages, certified one ahead
        case 11: launch_ring<192, 128, 16, 1, 4, 2, 2, false, 2>(g, st); break; // split, 192-row tiles, 4 x 20 KB (K slabs of 16), three in flight, two per CU
        case 12: launch_ring<192, 128, 32, 0, 4, 2, 2, false, 2>(g, st); break; // bf16, 192-row tiles, 4 x 20 KB (K slabs of 32), three in flight, two per CU
        case 14: launch_ring<256, 256, 64, 0, 2, 2, 2, false, 1>(g, st); break; // bf16, FOUR waves of 128 x 128 (one per SIMD, 512-register budget), 2 x 64 KB
        case 15: launch_ring<256, 256, 32, 0, 4, 2, 2, true, 1>(g, st); break;  // bf16, four waves of 128 x 128, 4 x 32 KB, certified one ahead
        case 16: launch_ring<256, 256, 32, 1, 2, 2, 2, false, 1>(g, st); break; // split, four waves of 128 x 128, 2 x 64 KB
        case 17: launch_ring<256, 256, 32, 1, 2, 2, 4, false>(g, st); break;    // split, 256 x 256, eight waves, 2 x 64 KB (two-stage form of ring2's 20)
        case 18: launch_ring<192, 256, 32, 1, 2, 2, 4, false>(g, st); break;    // split, 192 x 256, eight waves, 2 x 56 KB (two-stage form of 22)
        case 19: launch_ring<192, 256, 64, 0, 2, 2, 4, false>(g, st); break;    // bf16, 192 x 256, eight waves, 2 x 56 KB (two-stage form of 23)
        case 9: launch_ring<192, 128, 32, 1, 2, 2, 2, false, 2, true>(g, st); break;    // PROBE (wrong results): cfg 7 with 16x16x32 MFMAs
        case 10: launch_ring<192, 128, 64, 0, 2, 2, 2, false, 2, true>(g, st); break;   // PROBE (wrong results): cfg 8 with 16x16x32 MFMAs
#endif
        default: break;
    }
}

#ifdef PAA_CLOCK_STAMP
}  // namespace paa
// median over workgroups of (shader ticks / 100 MHz ticks) * 0.1 = GHz held during the last ring-kernel launch
extern "C" double paa_debug_ring_clock_ghz(int n_blocks) {
    static unsigned long long host[2 * 1024];
    if (n_blocks > 1024) n_blocks = 1024;
    if (hipDeviceSynchronize() != hipSuccess) return -1.0;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(paa::g_clock_stamp), sizeof(unsigned long long) * 2 * n_blocks) != hipSuccess) return -2.0;
    std::vector<double> r;
    for (int i = 0; i < n_blocks; ++i) if (host[2 * i + 1] > 0) r.push_back(0.1 * (double)host[2 * i] / (double)host[2 * i + 1]);
    if (r.empty()) return 0.0;
    std::sort(r.begin(), r.end());
    return r[r.size() / 2];
}
namespace paa {
#endif

int ring_tile_rows(int cfg) { return ((cfg >= 7 && cfg <= 13) || cfg == 18 || cfg == 19 || cfg == 22 || cfg == 23) ? 192 : 256; }
int ring_tile_cols(int cfg) { return (cfg == 4 || (cfg >= 6 && cfg <= 13)) ? 128 : 256; }
// forced (gemm.hip: a configuration asked for through paa_gemm_config): the separate-ring kernels from three K slabs (one per slot of
// the A ring) upwards; the automatic selection keeps its floor of four
bool ring_cfg_ok(int cfg, const paa_gemm_desc& d, bool forced) {
    if (cfg < 2 || cfg > 23 || cfg == 13) return false;       // 20..23: gemm_ring2.hip (separate operand rings)
#ifdef PAA_EXPERIMENTS
    // 9 / 10 are timing probes with WRONG results (MF16): only reachable when the measurement script asks for them
    static const bool probes = getenv("PAA_MF16_PROBE") != nullptr;
    if ((cfg == 9 || cfg == 10) && !probes) return false;
#else
    if (cfg != 7 && cfg != 8 && cfg < 20) return false;        // the configurations the shipped library holds
#endif
    const bool split = cfg == 4 || cfg == 6 || cfg == 7 || cfg == 9 || cfg == 11 || cfg == 16 || cfg == 17 || cfg == 18 || cfg == 20 || cfg == 22;
    if (split != (d.precision != 0)) return false;
    const int bk = (cfg == 2 || cfg == 8 || cfg == 10 || cfg == 14 || cfg == 19 || cfg == 21 || cfg == 23) ? 64 : cfg == 11 ? 16 : 32;
    return d.K % bk == 0 && d.K >= ((forced && cfg >= 20) ? 3 : 4) * bk;
}

}  // namespace paa
