/*
 * probe_kernels.hip -- MI355X (gfx950) kernel of the dynamic rect's QP probe
 * (scroll_batch_dyn_probe): per frame and candidate QP, the
 * squared error a decoder would see in the rect, the bits its MBs would
 * cost (coded_block_pattern + mb_qp_delta + residual) and their non-zero
 * levels -- what a rate controller asks before it picks the QP.
 *
 * k_dyn_probe is built like k_dyn_recon, not like k_dyn_row: a workgroup is
 * one rect MB row of one frame, reads k_dyn_rows' prediction rows, and
 * neither waits for nor hands anything to another workgroup.  A block's
 * source and prediction are loaded and transformed once; a run-time loop
 * over the candidates then quantises the coefficients W[16] with the coder's
 * own functions (dyn_device.h), measures the CAVLC body (probe_device.h),
 * runs the decoder's half (recon_device.h) for the squared error, and leaves
 * TotalCoeff << 2 | TrailingOnes of the block in LDS at [candidate][block].
 * The TotalCoeffs of the row above that nC needs are recomputed here (its
 * bottom luma block row and lower chroma block rows: forward half only).
 * After a barrier the coeff_token lengths at the composed nC and the MB
 * level fields are added, and one integer atomicAdd per (candidate, field)
 * goes to the frame's result.  Nothing is written but the results.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <algorithm>

#include "recon_device.h"
#include "recon_block.h"
#include "recon_pred.h"
#include "probe_device.h"
#include "dyn_engine.h"
#include "dyn_pos.h"
#include "probe_engine.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::recon;
using namespace scroll::probe;

namespace {

constexpr int PB_T = 256, PB_NW = PB_T / 64, PB_Q = SCROLL_DYN_PROBE_MAX_QPS;

constexpr Tabs k_ptabs = SCROLL_DYN_TABS;
__constant__ PLens g_plens = make_plens(k_ptabs);

struct ProbeLds {
    ReconLds cur, abv;                  /* prediction rows of this rect row and of the one above */
    PLens pl;
    uint32_t red[PB_NW][PB_Q][5];       /* per wave and candidate: bits, nonzero, Y, Cb, Cr */
};

/* dynamic LDS per candidate and rect MB of the row: 32 TotalCoeff bytes (16
 * luma, 8 chroma AC, 8 of the row above), the two chroma DC blocks (u16:
 * bits << 3 | TotalCoeff) and the MB's coded_block_pattern */
constexpr int PB_MB_BYTES = 32 + 4 + 1;

/* a[k] += v for a wave-uniform k, with static indices only (the sums stay in
 * registers) */
__device__ inline void acc_add(uint32_t a[PB_Q], int k, uint32_t v)
{
#pragma unroll
    for (int kk = 0; kk < PB_Q; ++kk) a[kk] += kk == k ? v : 0u;
}

/* block_store (recon_block.h) without the store: prediction + res, clipped,
 * and its squared error against the source on the packed bytes */
__device__ inline uint32_t block_sse(const uint32_t sv[4], const uint32_t pv[4], const int res[16])
{
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
    }
    return sq - 2u * cross;
}

/* candidate k of the packed list */
__device__ inline int qp_at(uint64_t qps, int k) { return __builtin_amdgcn_readfirstlane((int)(qps >> (8 * k)) & 255); }

/* GEN = false: grid (rect MB rows, frames, streams), every row whose chroma
 * prediction rows (its own 16 and the 8 of the block row above it) are
 * plain; GEN = true: grid (list slots, rect MB rows) -- the list holds every
 * frame of the batch, more than a grid's y may count -- the frames k_dyn_rows
 * listed (ctr[1] of them from ctr[DYN_CTR_LIST]), the rows that read a
 * half-pel waypoint chain: chroma_px_any is a tree of calls, kept out of the
 * common instantiation as in k_dyn_recon.  Each instantiation returns for
 * the other's rows. */
template <bool GEN>
__global__ __launch_bounds__(PB_T) void k_dyn_probe(const DevStream *__restrict__ st,
                                                    const NalDesc *__restrict__ nal, int ld_nal,
                                                    const PlanPending *__restrict__ pend,
                                                    const DynFrame *__restrict__ dfr, int ld_fr, DynGeom g,
                                                    const uint32_t *__restrict__ rows,
                                                    const uint8_t *__restrict__ src,
                                                    const uint8_t *__restrict__ refs, uint64_t qps, int nq,
                                                    ScrollDynProbe *__restrict__ res, uint32_t *__restrict__ done,
                                                    const uint32_t *__restrict__ ctr)
{
    extern __shared__ __align__(16) uint8_t dl[];
    __shared__ ProbeLds L;
    const int r = GEN ? blockIdx.y : blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    size_t nb;
    if (GEN) {
        if ((uint32_t)blockIdx.x >= min(ctr[1], g.gen_cap)) return;
        nb = ctr[DYN_CTR_LIST + blockIdx.x];
    } else {
        nb = (size_t)blockIdx.z * ld_fr + blockIdx.y;
    }
    const int s = (int)(nb / (size_t)ld_fr), f = (int)(nb - (size_t)s * ld_fr);
    const DynFrame df = dfr[nb];
    if (df.nal < 0) return;                              /* no dynamic NAL in this frame */
    dyn_frame_geom(g, nb);                               /* RowPred's origin, avl / avt: the frame's own */
    if (r >= g.h) {
        /* past the rows of a frame sized on its own: nothing to count, but
         * done[] stays the batch's h for every frame (once: GEN walks only the listed frames) */
        if (!GEN && t == 0) atomicAdd(&done[nb], 1u);
        return;
    }
    const bool above = r > 0;                            /* the row above is a rect row */
    if (t < 64) {
        const int i = t & 31, rr = t < 32 ? r : (above ? r - 1 : r);
        const uint32_t e = rows[nb * (size_t)(32 * g.ld_h) +
                                (i < 16 ? 16 * rr + i : 16 * g.h + (i < 24 ? 8 * rr + i - 16 : 8 * g.h + 8 * rr + i - 24))];
        if (t < 32) L.cur.rt[i] = e;
        else L.abv.rt[i] = e;
    } else if (t < 72) {
        L.cur.wo[t - 64] = L.abv.wo[t - 64] = pend[s].wo[t - 64];
        L.cur.wv[t - 64] = L.abv.wv[t - 64] = pend[s].wv[t - 64];
    }
    for (int i = t; i < (int)(sizeof(PLens) / 4); i += PB_T)
        reinterpret_cast<uint32_t *>(&L.pl)[i] = reinterpret_cast<const uint32_t *>(&g_plens)[i];
    __syncthreads();
    {
        bool gen = false;                               /* some chroma row read here needs the tree */
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t ea = L.cur.rt[16 + i], eb = L.cur.rt[24 + i];
            gen |= (ea & ROW_GEN) || (((ea >> 28) & 7u) && (eb & ROW_GEN));
        }
        if (above) {
#pragma unroll
            for (int i = 4; i < 8; ++i) {
                const uint32_t ea = L.abv.rt[16 + i], eb = L.abv.rt[24 + i];
                gen |= (ea & ROW_GEN) || (((ea >> 28) & 7u) && (eb & ROW_GEN));
            }
        }
        if (gen != GEN) return;
    }

    const int w = g.w, ndt = g.w * g.h;
    const int lstride = 16 * w, cstride = 8 * w;
    const int nl = 16 * w, nl64 = (nl + 63) & ~63;
    const int gc = (2 * w + 31) >> 5;                    /* chroma waves per plane */
    const int na64 = (4 * w + 63) & ~63;                 /* the row above: 4 w luma, 2 x 2 w chroma blocks */
    const int sB = nl64, sC = sB + 128 * gc, sD = sC + (above ? na64 : 0), total = sD + (above ? na64 : 0);
    const uint32_t m_4w = magic32((uint32_t)(4 * w));
    const size_t fo = (size_t)s * g.src_ld + (size_t)f * g.src_fr;
    /* per candidate k: tcb[k 32 w + ...]: 16 w luma (raster), 8 w chroma AC
     * (plane, block row, block), 4 w + 2 x 2 w of the row above */
    uint8_t *tcb = dl;
    uint16_t *dcw = reinterpret_cast<uint16_t *>(dl + (size_t)nq * 32 * w);   /* [k][plane][MB] */
    uint8_t *cbpb = dl + (size_t)nq * 36 * w;                                  /* [k][MB] */
    const int kst = 32 * w;

    const uint8_t *rb = refs + (size_t)s * g.ref_ld;
    const uint32_t csz = (uint32_t)g.pw * (uint32_t)g.ph / 4;
    const NalDesc *nd = nal + (size_t)s * ld_nal + df.nal;
    const RowPred<GEN> P{L.cur, rb, csz, g.x0, g.y0 + r, st + s, nd};
    const RowPred<GEN> Pa{L.abv, rb, csz, g.x0, g.y0 + r - 1, st + s, nd};

    if (!above)                                          /* rect row 0: TotalCoeff 0 above (or unavailable) */
        for (int k = 0; k < nq; ++k)
            for (int j = t; j < 8 * w; j += PB_T) tcb[k * kst + 24 * w + j] = 0;

    /* this thread's sums per candidate: bits | nonzero << 20, and the errors */
    uint32_t bn[PB_Q], ey[PB_Q], eu[PB_Q], ev[PB_Q];
#pragma unroll
    for (int k = 0; k < PB_Q; ++k) bn[k] = ey[k] = eu[k] = ev[k] = 0;

    for (int base = 0; base < total; base += PB_T) {
        const int wb = __builtin_amdgcn_readfirstlane(base + (t & ~63));   /* the wave's first slot */
        if (wb >= total) continue;
        if (wb < sB) {                                   /* luma, raster */
            const int slot = wb + lane;
            if (slot >= nl) continue;
            const int by = (int)div_m((uint32_t)slot, m_4w), bx = slot - by * 4 * w;
            const size_t po = fo + (size_t)(16 * r + 4 * by) * lstride + 4 * bx;
            uint32_t sv[4], pv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) sv[i] = ld32(src + po + (size_t)i * lstride);
            P.luma(by, bx, pv);
            int W[16];
            block_fwd(sv, pv, W);
#pragma nounroll
            for (int k = 0; k < nq; ++k) {
                const int qpy = qp_at(qps, k);
                const QParams ql = qparams_rt(qpy);
                const DQParams dq = dqparams_rt(qpy);
                int lv[16], c[16], rs[16], tc, t1;
                quant4x4<false>(W, lv, ql);
                const int bl = block_len<16>(L.pl, lv, tc, t1);
                dequant4x4(lv, c, dq);
                inv4x4(c, rs);
                tcb[k * kst + slot] = (uint8_t)(tc << 2 | t1);
                acc_add(bn, k, (uint32_t)bl | (uint32_t)tc << 20);
                acc_add(ey, k, block_sse(sv, pv, rs));
            }
        } else if (wb < sC) {                            /* chroma: plane p, wave grp of it */
            const int cw = (wb - sB) >> 6;
            const int p = cw >= gc ? 1 : 0, grp = cw - p * gc;
            const int by = lane >> 5, bx = 32 * grp + (lane & 31);
            const bool act = bx < 2 * w;                 /* the same for an MB's four lanes */
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
            const int kb = 2 * by + (bx & 1);
            const int x0 = W[0], x1 = __shfl_xor(x0, 1, 64), x2 = __shfl_xor(x0, 32, 64), x3 = __shfl_xor(x0, 33, 64);
            int w0[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = j ^ kb;
                w0[j] = d == 0 ? x0 : d == 1 ? x1 : d == 2 ? x2 : x3;
            }
            if (!act) continue;
            const int h0 = w0[0] + w0[1] + w0[2] + w0[3], h1 = w0[0] - w0[1] + w0[2] - w0[3];
            const int h2 = w0[0] + w0[1] - w0[2] - w0[3], h3 = w0[0] - w0[1] - w0[2] + w0[3];
            const int slot = 16 * w + p * 4 * w + by * 2 * w + bx;
#pragma nounroll
            for (int k = 0; k < nq; ++k) {
                const int qpc = qp_chroma(qp_at(qps, k));
                const QParams qc = qparams_rt(qpc);
                const DQParams dq = dqparams_rt(qpc);
                int ld[16], dcs[4];
                ld[0] = quant_dc(h0, qc);
                ld[1] = quant_dc(h1, qc);
                ld[2] = quant_dc(h2, qc);
                ld[3] = quant_dc(h3, qc);
                chroma_dc(ld, dcs, dq);
                int lv[16], c[16], rs[16], tc, t1;
                quant4x4<true>(W, lv, qc);
                const int bl = block_len<15>(L.pl, lv, tc, t1);
                dequant4x4(lv, c, dq);
                c[0] = kb == 0 ? dcs[0] : kb == 1 ? dcs[1] : kb == 2 ? dcs[2] : dcs[3];
                inv4x4(c, rs);
                tcb[k * kst + slot] = (uint8_t)(tc << 2 | t1);
                uint32_t add = (uint32_t)bl | (uint32_t)tc << 20;
                if (kb == 0) {                           /* one lane per MB and plane: the DC block, nC = -1 */
                    int tcd, t1d;
                    const int bd = block_len<4>(L.pl, ld, tcd, t1d) + token_len(L.pl, tcd, t1d, -1);
                    dcw[(k * 2 + p) * w + (bx >> 1)] = (uint16_t)(bd << 3 | tcd);
                    add += (uint32_t)tcd << 20;
                }
                acc_add(bn, k, add);
                const uint32_t e = block_sse(sv, pv, rs);
                if (p) acc_add(ev, k, e);
                else acc_add(eu, k, e);
            }
        } else {                                         /* the row above: TotalCoeffs only */
            const bool lum = wb < sD;
            const int slot = wb - (lum ? sC : sD) + lane;
            if (slot >= 4 * w) continue;
            uint32_t sv[4], pv[4];
            int W[16];
            if (lum) {                                   /* its bottom luma block row */
                const size_t po = fo + (size_t)(16 * (r - 1) + 12) * lstride + 4 * slot;
#pragma unroll
                for (int i = 0; i < 4; ++i) sv[i] = ld32(src + po + (size_t)i * lstride);
                Pa.luma(3, slot, pv);
                block_fwd(sv, pv, W);
#pragma nounroll
                for (int k = 0; k < nq; ++k) {
                    int lv[16];
                    quant4x4<false>(W, lv, qparams_rt(qp_at(qps, k)));
                    tcb[k * kst + 24 * w + slot] = (uint8_t)(__builtin_popcount(scan_mask<16>(lv)) << 2);
                }
            } else {                                     /* each plane's lower chroma block row */
                const int p = slot >= 2 * w ? 1 : 0, bx = slot - p * 2 * w;
                const size_t po = fo + (size_t)256 * ndt + (size_t)p * 64 * ndt + (size_t)(8 * (r - 1) + 4) * cstride + 4 * bx;
#pragma unroll
                for (int i = 0; i < 4; ++i) sv[i] = ld32(src + po + (size_t)i * cstride);
                Pa.chroma(p, 1, bx, pv);
                block_fwd(sv, pv, W);
#pragma nounroll
                for (int k = 0; k < nq; ++k) {
                    int lv[16];
                    quant4x4<true>(W, lv, qparams_rt(qp_chroma(qp_at(qps, k))));
                    tcb[k * kst + 28 * w + slot] = (uint8_t)(__builtin_popcount(scan_mask<15>(lv)) << 2);
                }
            }
        }
    }
    __syncthreads();

    /* MB level: coded_block_pattern, mb_qp_delta, the DC blocks */
#pragma nounroll
    for (int k = 0; k < nq; ++k) {
        const uint8_t *tk = tcb + k * kst;
        for (int m = t; m < w; m += PB_T) {
            int cbp = 0;
#pragma unroll
            for (int by = 0; by < 4; ++by) {
                const uint32_t v = *reinterpret_cast<const uint32_t *>(tk + by * 4 * w + 4 * m);
                if (v & 0xffffu) cbp |= 1 << ((by >> 1) * 2);
                if (v >> 16) cbp |= 1 << ((by >> 1) * 2 + 1);
            }
            uint32_t ac = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)                   /* (plane, block row): 2 blocks each */
                ac |= *reinterpret_cast<const uint16_t *>(tk + 16 * w + i * 2 * w + 2 * m);
            const uint32_t d0 = dcw[(k * 2 + 0) * w + m], d1 = dcw[(k * 2 + 1) * w + m];
            cbp |= ac ? 32 : ((d0 | d1) & 7u) ? 16 : 0;
            cbpb[k * w + m] = (uint8_t)cbp;
            acc_add(bn, k, (uint32_t)L.pl.cbp[cbp] + (cbp ? 1u : 0u) + ((cbp >> 4) ? (d0 >> 3) + (d1 >> 3) : 0u));
        }
    }
    __syncthreads();

    /* coeff_token of every block of a coded 8x8 / the coded AC class, at the
     * nC composed from the left and top TotalCoeffs: MBs outside the rect
     * count as available with 0, picture edges as unavailable */
    const bool avl = g.x0 > 0, avt = g.y0 + r > 0;
#pragma nounroll
    for (int k = 0; k < nq; ++k) {
        const uint8_t *tk = tcb + k * kst;
        for (int j = t; j < 24 * w; j += PB_T) {
            int nA, nB, cbp;
            bool coded;
            if (j < 16 * w) {
                const int by = (int)div_m((uint32_t)j, m_4w), bx = j - by * 4 * w;
                cbp = cbpb[k * w + (bx >> 2)];
                coded = cbp >> ((by >> 1) * 2 + ((bx & 3) >> 1)) & 1;
                nA = bx > 0 ? tk[j - 1] >> 2 : avl ? 0 : -1;
                nB = by > 0 ? tk[j - 4 * w] >> 2 : avt ? tk[24 * w + bx] >> 2 : -1;
            } else {
                const int jj = j - 16 * w, p = jj >= 4 * w ? 1 : 0, rem = jj - p * 4 * w;
                const int by = rem >= 2 * w ? 1 : 0, bx = rem - by * 2 * w;
                cbp = cbpb[k * w + (bx >> 1)];
                coded = (cbp >> 4) == 2;
                nA = bx > 0 ? tk[j - 1] >> 2 : avl ? 0 : -1;
                nB = by > 0 ? tk[j - 2 * w] >> 2 : avt ? tk[28 * w + p * 2 * w + bx] >> 2 : -1;
            }
            if (coded) acc_add(bn, k, (uint32_t)token_len(L.pl, tk[j] >> 2, tk[j] & 3, nc_of(nA, nB)));
        }
    }

    /* wave, workgroup, then one integer atomic per candidate and field */
#pragma unroll
    for (int k = 0; k < PB_Q; ++k) {
        if (k >= nq) break;
        const uint32_t b = wave_sum(bn[k] & 0xfffffu), n = wave_sum(bn[k] >> 20);
        const uint32_t y = wave_sum(ey[k]), u = wave_sum(eu[k]), v = wave_sum(ev[k]);
        if (lane == 0) {
            L.red[wave][k][0] = b;
            L.red[wave][k][1] = n;
            L.red[wave][k][2] = y;
            L.red[wave][k][3] = u;
            L.red[wave][k][4] = v;
        }
    }
    __syncthreads();
    if (t < 5 * nq) {
        const int k = t / 5, fld = t - 5 * k;
        unsigned long long v = 0;
#pragma unroll
        for (int i = 0; i < PB_NW; ++i) v += L.red[i][k][fld];
        ScrollDynProbe *o = res + nb * PB_Q + k;
        if (fld == 0) atomicAdd(&o->bits, (uint32_t)v);
        else if (fld == 1) atomicAdd(&o->nonzero, (uint32_t)v);
        else if (v) atomicAdd(reinterpret_cast<unsigned long long *>(&o->sse[fld - 2]), v);
    }
    if (t == 0) atomicAdd(&done[nb], 1u);                /* rect rows counted into this frame */
}

size_t probe_lds_bytes(int w, int nq) { return (size_t)PB_MB_BYTES * (size_t)w * (size_t)nq; }

}  // namespace

int probe_launch(hipStream_t hs, int nframes, int S, const DevStream *st, const NalDesc *nal, int ld_nal,
                 const PlanPending *pend, const DynFrame *dfr, int ld_fr, const DynGeom *g,
                 const uint32_t *rows, const uint8_t *src, const uint8_t *refs, const ProbeQps *q,
                 ScrollDynProbe *res, uint32_t *done, const uint32_t *ctr, hipEvent_t ev0, hipEvent_t ev1)
{
    if (nframes <= 0 || S <= 0) return 0;
    uint64_t qps = 0;
    for (int k = 0; k < q->n; ++k) qps |= (uint64_t)q->qp[k] << (8 * k);
    const size_t lds = probe_lds_bytes(g->w, q->n);
    if (lds + sizeof(ProbeLds) > 65536) {
        /* wide rects at many candidates: dynamic LDS past the 64 KB default
         * (a 256-MB row at 8 candidates: 74 KB of the CU's 160 KB) */
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dyn_probe<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dyn_probe<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return -1;
    }
    if (hipMemsetAsync(res, 0, (size_t)S * ld_fr * PB_Q * sizeof(ScrollDynProbe), hs) != hipSuccess ||
        hipMemsetAsync(done, 0, (size_t)S * ld_fr * sizeof(uint32_t), hs) != hipSuccess)
        return -1;
    if (ev0 && hipEventRecord(ev0, hs) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dyn_probe<false>, dim3(g->h, nframes, S), dim3(PB_T), lds, hs, st, nal, ld_nal, pend, dfr,
                       ld_fr, *g, rows, src, refs, qps, q->n, res, done, ctr);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dyn_probe<true>, dim3(std::min<uint32_t>(g->gen_cap, (uint32_t)(nframes * S)), g->h),
                       dim3(PB_T), lds, hs, st, nal, ld_nal, pend, dfr, ld_fr, *g, rows, src, refs, qps, q->n, res,
                       done, ctr);
    if (hipGetLastError() != hipSuccess) return -1;
    if (ev1 && hipEventRecord(ev1, hs) != hipSuccess) return -1;
    return 0;
}
