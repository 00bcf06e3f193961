/*
 * recon_block.h -- what the reconstruction kernels (k_dyn_recon,
 * recon_kernels.hip; k_hdyn_recon, hrecon_kernels.hip) share.  Per lane: a
 * 4x4 block's source and prediction as four packed rows each, from them the
 * coder's coefficients, and prediction + residual clipped, stored and
 * compared with the source.  Per workgroup: recon_row, the loop over a rect
 * MB row's blocks and the squared-error reduction, which takes the
 * prediction from the kernel.  Device only.
 */
#ifndef SCROLL_RECON_BLOCK_H
#define SCROLL_RECON_BLOCK_H

#include <hip/hip_runtime.h>

#include "engine.h"
#include "recon_device.h"

namespace scroll {
namespace recon {

__device__ inline uint32_t ld32(const uint8_t *p) { return *reinterpret_cast<const uint32_t *>(p); }
__device__ inline void st32(uint8_t *p, uint32_t v) { *reinterpret_cast<uint32_t *>(p) = v; }

__device__ inline void unpack4(uint32_t v, int *o)
{
    o[0] = (int)(v & 255u);
    o[1] = (int)((v >> 8) & 255u);
    o[2] = (int)((v >> 16) & 255u);
    o[3] = (int)(v >> 24);
}
__device__ inline uint32_t pack4(const int *o)
{
    return (uint32_t)o[0] | (uint32_t)o[1] << 8 | (uint32_t)o[2] << 16 | (uint32_t)o[3] << 24;
}

/* A block's source and prediction stay packed (4 + 4 registers) while its
 * coefficients go through quant / dequant / inverse: they are unpacked for
 * the residual, and again for add + clip + squared error.  (Kept as 32
 * unpacked registers across the transforms the kernel took 116 VGPRs.) */
__device__ inline void block_fwd(const uint32_t sv[4], const uint32_t pv[4], int W[16])
{
    int sp[16], pr[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unpack4(sv[i], sp + 4 * i);
        unpack4(pv[i], pr + 4 * i);
    }
    residual_fwd(sp, pr, W);
}

/* prediction + res, clipped -> 4 rows at dst (stride bytes apart); returns
 * the squared error against the source */
__device__ inline uint32_t block_store(uint32_t sv[4], uint32_t pv[4], int res[16], uint8_t *dst, int stride)
{
    /* the packed words as new values once the residual exists, so that the
     * bytes unpacked for block_fwd are not kept live until here */
    asm volatile("" : "+v"(sv[0]), "+v"(sv[1]), "+v"(sv[2]), "+v"(sv[3]), "+v"(pv[0]), "+v"(pv[1]), "+v"(pv[2]),
                 "+v"(pv[3]), "+v"(res[0]));
    /* sum (s - o)^2 = sum s^2 + sum o^2 - 2 sum s o on the packed bytes: three
     * 4-byte dot products per row, the source never unpacked again */
    uint32_t sq = 0, cross = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int pr[4], out[4];
        unpack4(pv[i], pr);
#pragma unroll
        for (int x = 0; x < 4; ++x) out[x] = add_clip(pr[x], res[4 * i + x]);
        const uint32_t ov = pack4(out);
        sq = __builtin_amdgcn_udot4(sv[i], sv[i], sq, false);
        sq = __builtin_amdgcn_udot4(ov, ov, sq, false);
        cross = __builtin_amdgcn_udot4(sv[i], ov, cross, false);
        st32(dst + (size_t)i * stride, ov);
    }
    return sq - 2u * cross;
}

__device__ inline uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

/* One rect MB row (row r of the g.w x g.h rect) of one frame, by a workgroup
 * of NT threads, one 4x4 block per thread and pass: levels at QP qpy / its
 * QPc, the decoded blocks to rec + fo, their squared error against src + fo
 * (the frame's rect as I420; source and reconstruction share the layout)
 * added to sse3[0..2] (Y, Cb, Cr).  red: NT / 64 x 3 words of LDS.
 *
 * Task slots of a row (w = rect MBs per row):
 *   [0, 16 w)            luma blocks in raster order (4 block rows of 4 w);
 *                        padded to a multiple of 64
 *   then per plane       ceil(2 w / 32) waves of chroma blocks: lanes 0..31
 *                        32 consecutive blocks of the plane's upper block
 *                        row, lanes 32..63 the same blocks of the lower one
 * so adjacent lanes touch adjacent 4 bytes of one picture row (a wave's row
 * loads and stores are runs of 128 or 256 bytes), and the four blocks of an
 * MB's chroma plane sit in one wave at lanes l, l ^ 1, l ^ 32, l ^ 33: they
 * exchange their DC coefficients by __shfl_xor.  Rows of more than NT slots
 * loop (config 3: 704 slots, 3 passes of 256).
 *
 * Where a block's prediction comes from is the kernel's, as a Pred P:
 *   P.coded(m)             is MB m of the row coded at all?  (a lane of an MB
 *                          that is not still takes part in the DC exchange)
 *   P.luma(by, bx, pv)     luma block (by, bx) of the row -> its four packed
 *   P.chroma(p, by, bx, pv)   rows; the same of plane p (0 Cb, 1 Cr)
 * all three inlined: the loop is instantiated per kernel and GEN.  A block's
 * source rows are loaded before its prediction: the other way round
 * k_hdyn_recon took 4 % longer (profiles/rowloop_recon_bench_order_p720dyn.txt). */
template <int NT, class Pred>
__device__ inline void recon_row(const Pred &P, int qpy, const DynGeom &g, int r, size_t fo,
                                 const uint8_t *__restrict__ src, uint8_t *__restrict__ rec, uint32_t (*red)[3],
                                 unsigned long long *sse3)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int qpc = dyn::qp_chroma(qpy);
    const QParams ql = dyn::qparams_rt(qpy), qc = dyn::qparams_rt(qpc);
    const DQParams dl = dqparams_rt(qpy), dc = dqparams_rt(qpc);
    const int ndt = g.w * g.h;
    const int lstride = 16 * g.w, cstride = 8 * g.w;
    const int nl = 16 * g.w, nl64 = (nl + 63) & ~63;
    const int gc = (2 * g.w + 31) >> 5;                  /* chroma waves per plane */
    const int total = nl64 + 128 * gc;
    const uint32_t m_4w = dyn::magic32((uint32_t)(4 * g.w));

    uint32_t e0 = 0, e1 = 0, e2 = 0;                     /* this thread's squared error: Y, Cb, Cr */
    for (int base = 0; base < total; base += NT) {
        const int wb = __builtin_amdgcn_readfirstlane(base + (t & ~63));   /* the wave's first slot */
        if (wb >= total) continue;
        if (wb < nl64) {                                 /* luma, raster */
            const int slot = wb + lane;
            if (slot >= nl) continue;
            const int by = (int)dyn::div_m((uint32_t)slot, m_4w), bx = slot - by * 4 * g.w;
            if (!P.coded(bx >> 2)) continue;
            const size_t po = fo + (size_t)(16 * r + 4 * by) * lstride + 4 * bx;
            uint32_t sv[4], pv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) sv[i] = ld32(src + po + (size_t)i * lstride);
            P.luma(by, bx, pv);
            int W[16], res[16];
            block_fwd(sv, pv, W);
            recon_residual<false>(W, 0, res, ql, dl);
            e0 += block_store(sv, pv, res, rec + po, lstride);
        } else {                                         /* chroma: plane p, wave grp of it */
            const int cw = (wb - nl64) >> 6;
            const int p = cw >= gc ? 1 : 0, grp = cw - p * gc;
            const int by = lane >> 5, bx = 32 * grp + (lane & 31);
            const bool act = bx < 2 * g.w && P.coded(bx >> 1);   /* the same for an MB's four lanes */
            const size_t po = fo + (size_t)256 * ndt + (size_t)p * 64 * ndt + (size_t)(8 * r + 4 * by) * cstride + 4 * bx;
            uint32_t sv[4] = {0, 0, 0, 0}, pv[4] = {0, 0, 0, 0};
            int W[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) W[k] = 0;
            if (act) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sv[i] = ld32(src + po + (size_t)i * cstride);
                P.chroma(p, by, bx, pv);
                block_fwd(sv, pv, W);
            }
            /* the plane's four DC coefficients of this MB, in raster order */
            const int k = 2 * by + (bx & 1);
            const int x0 = W[0], x1 = __shfl_xor(x0, 1, 64), x2 = __shfl_xor(x0, 32, 64), x3 = __shfl_xor(x0, 33, 64);
            int w0[4], dcs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = j ^ k;
                w0[j] = d == 0 ? x0 : d == 1 ? x1 : d == 2 ? x2 : x3;
            }
            chroma_dc_coded(w0, dcs, qc, dc);
            if (act) {
                const int mydc = k == 0 ? dcs[0] : k == 1 ? dcs[1] : k == 2 ? dcs[2] : dcs[3];
                int res[16];
                recon_residual<true>(W, mydc, res, qc, dc);
                const uint32_t e = block_store(sv, pv, res, rec + po, cstride);
                if (p) e2 += e;
                else e1 += e;
            }
        }
    }
    /* squared error: wave, workgroup, then one 64-bit atomic per plane (a
     * thread's sum stays below 2^22, a workgroup's below 2^30) */
    e0 = wave_sum(e0);
    e1 = wave_sum(e1);
    e2 = wave_sum(e2);
    if (lane == 0) {
        red[wave][0] = e0;
        red[wave][1] = e1;
        red[wave][2] = e2;
    }
    __syncthreads();
    if (t < 3) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) v += red[k][t];
        if (v) atomicAdd(&sse3[t], (unsigned long long)v);
    }
}

}  // namespace recon
}  // namespace scroll

#endif
