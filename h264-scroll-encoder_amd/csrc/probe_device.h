/*
 * probe_device.h -- device functions of the dynamic rect's QP probe
 * (scroll_batch_dyn_probe): how many bits the coder would
 * spend on a block and on an MB, without writing one.
 *
 * The coder's CAVLC (dyn_device.h: cavlc_block, cavlc_body) takes levels
 * from memory and puts bits into a sink.  The probe needs the lengths alone,
 * at several QPs per block, from levels that live in registers: block_len
 * takes a block's levels by value in raster order and returns TotalCoeff,
 * TrailingOnes and the bits of everything after the coeff_token; token_len
 * is the coeff_token's length at an nC; mb_len sums an MB.  Lengths come
 * from PLens, the length columns of dyn_device.h's Tabs (684 bytes: LDS).
 *
 * Pure integer functions like dyn_device.h: k_dyn_probe (probe_kernels.hip)
 * uses them per lane, tests/hostsim/probe_sim.cpp compiles them for the CPU
 * and tests/test_probe_hostsim.py checks them against the oracle's coder.
 */
#ifndef SCROLL_PROBE_DEVICE_H
#define SCROLL_PROBE_DEVICE_H

#include "dyn_device.h"

namespace scroll {
namespace probe {

/* code lengths: coeff_token ([0..2] the nC columns, [3] chroma DC),
 * total_zeros, chroma DC total_zeros, run_before, and me(v) of a
 * coded_block_pattern (Table 9-4, inter) */
struct alignas(4) PLens {
    uint8_t ct[4][68];
    uint8_t tz[15][16];
    uint8_t tzdc[3][4];
    uint8_t rb[7][16];
    uint8_t cbp[48];
};
static_assert(sizeof(PLens) % 4 == 0, "PLens copies as 32-bit words");

constexpr PLens make_plens(const dyn::Tabs &T)
{
    PLens P{};
    for (int i = 0; i < 3 * 68; ++i) P.ct[i / 68][i % 68] = T.ct_len[i / 68][i % 68];
    for (int i = 0; i < 20; ++i) P.ct[3][i] = T.ctdc_len[i];
    for (int i = 0; i < 15 * 16; ++i) P.tz[i / 16][i % 16] = T.tz_len[i / 16][i % 16];
    for (int i = 0; i < 12; ++i) P.tzdc[i / 4][i % 4] = T.tzdc_len[i / 4][i % 4];
    for (int i = 0; i < 7 * 15; ++i) P.rb[i / 15][i % 15] = T.rb_len[i / 15][i % 15];
    for (int i = 0; i < 48; ++i) P.cbp[i] = (uint8_t)(2 * (31 - __builtin_clz((uint32_t)T.cbp_code[i] + 1u)) + 1);
    return P;
}

/* bits of coeff_token (9.2.1) for (TotalCoeff, TrailingOnes) at nC; nC = -1:
 * the chroma DC block */
__device__ __host__ inline int token_len(const PLens &P, int tc, int t1, int nC)
{
    if (nC >= 8) return 6;
    const int tb = nC < 0 ? 3 : nC < 2 ? 0 : nC < 4 ? 1 : 2;
    return P.ct[tb][4 * tc + t1];
}

/* bits of level_prefix + level_suffix (9.2.2.1) of levelCode at suffixLength
 * sl: the length of dyn_device.h's level_field */
__device__ __host__ inline int level_len(int code, int sl)
{
    if (sl == 0) return code < 14 ? code + 1 : code < 30 ? 19 : 28;
    return code < (15 << sl) ? (code >> sl) + 1 + sl : 28;
}

/* coefficient i (scan order) of a block of MAXC coefficients whose levels lv
 * are in raster order: 16 a luma block, 15 a chroma AC block (scan positions
 * 1..15), 4 the chroma DC block (lv[0..3] as they are) */
template <int MAXC>
__device__ __host__ constexpr int scan_pos(int i)
{
    return MAXC == 4 ? i : dyn::ZZ[MAXC == 15 ? i + 1 : i];
}

/* the block's non-zero mask in scan order (bit i: coefficient i) */
template <int MAXC>
__device__ __host__ inline uint32_t scan_mask(const int lv[16])
{
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) nz |= lv[scan_pos<MAXC>(i)] != 0 ? 1u << i : 0u;
    return nz;
}

/* total_zeros + run_before bits of a block with non-zero mask nz (scan
 * order), as cavlc_block lays them */
template <int MAXC>
__device__ __host__ inline int zeros_len(const PLens &P, uint32_t nz, int tc)
{
    if (tc == 0) return 0;
    const int hi = dyn::top_bit(nz);
    int zl = hi + 1 - tc, bits = 0;
    if (tc < MAXC) bits = MAXC == 4 ? P.tzdc[tc - 1][zl] : P.tz[tc - 1][zl];
    uint32_t m = nz;
    int p = hi;
    for (int k = 0; k < tc - 1 && zl > 0; ++k) {
        m &= ~(1u << p);
        const int q = dyn::top_bit(m);
        const int run = p - q - 1;
        bits += P.rb[(zl < 7 ? zl : 7) - 1][run];
        zl -= run;
        p = q;
    }
    return bits;
}

/* One block: levels by value (raster order, static indices only: nothing is
 * addressed at run time, so nothing goes to scratch).  Returns the bits
 * after the coeff_token -- trailing-ones signs, levels with the prefix-14 /
 * 15 escapes, total_zeros, run_before -- and TotalCoeff / TrailingOnes. */
template <int MAXC>
__device__ __host__ inline int block_len(const PLens &P, const int lv[16], int &tc, int &t1)
{
    const uint32_t nz = scan_mask<MAXC>(lv);
    tc = __builtin_popcount(nz);
    /* one walk down the scan: the +-1 run at its high end (TrailingOnes, at
     * most 3: one sign bit each), then the levels with their suffixLength.
     * (Two walks, and an early return for an empty block, both measured
     * slower in k_dyn_probe: DESIGN.md §6) */
    int n1 = 0, bits = 0, sl = 0;
    bool trail = true, first = true;
#pragma unroll
    for (int i = MAXC - 1; i >= 0; --i) {
        const int v = lv[scan_pos<MAXC>(i)];
        if (v != 0) {
            const int a = v < 0 ? -v : v;
            if (trail && a == 1 && n1 < 3) {
                n1++;
                bits++;
            } else {
                if (first) sl = (tc > 10 && n1 < 3) ? 1 : 0;
                trail = false;
                int code = 2 * a - 2 + (v < 0 ? 1 : 0);
                if (first && n1 < 3) code -= 2;
                first = false;
                bits += level_len(code, sl);
                if (sl == 0) sl = 1;
                if (a > (3 << (sl - 1)) && sl < 6) sl++;
            }
        }
    }
    t1 = n1;
    return bits + zeros_len<MAXC>(P, nz, tc);
}

/* coded_block_pattern of an MB from its blocks' TotalCoeffs (16 luma in
 * raster order) and chroma flags */
__device__ __host__ inline int cbp_of(const uint8_t tcl[16], bool any_dc, bool any_ac)
{
    int cbp = any_ac ? 32 : any_dc ? 16 : 0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (tcl[r]) cbp |= 1 << ((r >> 3) * 2 + ((r & 3) >> 1));
    return cbp;
}

/* The MB-level sum (or_mb_residual's syntax).  tt: per block TotalCoeff << 2
 * | TrailingOnes, 16 luma in raster order then Cb AC 4, Cr AC 4; body: the
 * sum of the 24 blocks' block_len (blocks of uncoded 8x8s / an uncoded AC
 * class have none); dc_bits: coeff_token + body of the two chroma DC blocks;
 * left / top: the neighbours' TotalCoeffs as or_mb_residual indexes them
 * (24 each; NULL: unavailable).  Returns me(v) + mb_qp_delta + residual. */
__device__ __host__ inline int mb_len(const PLens &P, const uint8_t tt[24], int body, int dc_bits, bool any_dc,
                                      const uint8_t *left, const uint8_t *top)
{
    uint8_t tcl[16];
    bool any_ac = false;
    for (int r = 0; r < 16; ++r) tcl[r] = tt[r] >> 2;
    for (int i = 16; i < 24; ++i) any_ac |= (tt[i] >> 2) != 0;
    const int cbp = cbp_of(tcl, any_dc, any_ac);
    int bits = P.cbp[cbp];
    if (cbp == 0) return bits;
    bits += 1 + body;                                       /* mb_qp_delta se(0) */
    for (int r = 0; r < 16; ++r) {
        const int x = r & 3, y = r >> 2;
        if (!(cbp >> ((y >> 1) * 2 + (x >> 1)) & 1)) continue;
        const int nA = x > 0 ? tt[r - 1] >> 2 : left ? left[r + 3] : -1;
        const int nB = y > 0 ? tt[r - 4] >> 2 : top ? top[r + 12] : -1;
        bits += token_len(P, tt[r] >> 2, tt[r] & 3, dyn::nc_of(nA, nB));
    }
    if (cbp >> 4) bits += dc_bits;
    if ((cbp >> 4) == 2)
        for (int i = 16; i < 24; ++i) {
            const int k = (i - 16) & 3, x = k & 1, y = k >> 1;
            const int nA = x > 0 ? tt[i - 1] >> 2 : left ? left[i + 1] : -1;
            const int nB = y > 0 ? tt[i - 2] >> 2 : top ? top[i + 2] : -1;
            bits += token_len(P, tt[i] >> 2, tt[i] & 3, dyn::nc_of(nA, nB));
        }
    return bits;
}

}  // namespace probe
}  // namespace scroll

#endif
