/*
 * recon_kernels.hip -- MI355X (gfx950) kernel of the dynamic rect's
 * reconstruction (scroll_batch_set_dyn_recon): the picture a
 * decoder displays for the rect of every dynamic NAL, and its sum of squared
 * errors against the source, per frame and plane.
 *
 * k_dyn_recon repeats the coder's forward half per 4x4 block with the
 * coder's own functions (dyn_device.h: fwd4x4, quant, quant_dc at the
 * stream's QP / QPc), so its levels are the coded ones, and runs the
 * decoder's half on them (recon_device.h).  It reads k_dyn_rows' prediction
 * rows and is independent of k_dyn_row: levels stay in 32-bit registers, so
 * the same code serves the int8 path and the general path (QP < 22); rows
 * with a half-pel waypoint chain run in the template's second instantiation.
 *
 * Workgroup = one rect MB row of one dynamic NAL, 256 threads, one 4x4
 * block per thread and pass.  Task slots of a row (w = rect MBs per row):
 *   [0, 16 w)            luma blocks in raster order (4 block rows of 4 w);
 *                        padded to a multiple of 64
 *   then per plane       ceil(2 w / 32) waves of chroma blocks: lanes 0..31
 *                        32 consecutive blocks of the plane's upper block
 *                        row, lanes 32..63 the same blocks of the lower one
 * so adjacent lanes touch adjacent 4 bytes of one picture row (a wave's row
 * loads and stores are runs of 128 or 256 bytes), and the four blocks of an
 * MB's chroma plane sit in one wave at lanes l, l ^ 1, l ^ 32, l ^ 33: they
 * exchange their DC coefficients by __shfl_xor.  Rows of more than 256 slots
 * loop (config 3: 704 slots, 3 passes).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <algorithm>

#include "recon_device.h"
#include "recon_block.h"
#include "dyn_engine.h"
#include "recon_engine.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::recon;

namespace {

constexpr int RC_T = 256, RC_NW = RC_T / 64;/* rows[] entries (k_dyn_rows, dyn_kernels.hip): the chroma fraction in bits
 * 28..30, ROW_GEN a half-pel waypoint chain, the byte offset below */
constexpr uint32_t ROW_GEN = 1u << 31, ROW_OFF = 0x0fffffffu;

struct ReconLds {
    uint32_t rt[32];                    /* the row's prediction rows: 16 luma, 8 upper, 8 lower chroma */
    int32_t wo[8], wv[8];               /* the frame's waypoint table (half-pel chains only) */
    uint32_t red[RC_NW][3];
};

/* four chroma prediction samples through a half-pel waypoint chain (the
 * general path's sampler, k_dyn_code_general): row ya of the NAL's region,
 * plane p, columns X .. X + 3 */
__device__ inline void chroma_pred_any(const DevStream *S, const NalDesc &d, const int32_t *wo, const int32_t *wv,
                                       const uint8_t *rb, int mbrow, int p, int X, int yrow, int *pred)
{
    const int w = S->w, h = S->h;
    NalCtx c;
    c.w = w;
    c.h = h;
    c.log2_mfn = S->log2_mfn;
    c.poc_type = S->poc_type;
    c.log2_poc = S->log2_poc;
    c.deblock = S->deblock;
    c.kind = d.kind;
    c.off = d.off;
    c.frame_num = d.frame_num;
    c.nwp = d.nwp;
    c.wp_off = wo;
    c.wp_lt = wo;                       /* regions() does not read the long-term indices */
    c.wp_valid = wv;
    const Regions rg = regions(c);
    const bool cA = mbrow < (h - d.off) / 16;
    const int ref = cA ? rg.ra : rg.rb, q = 4 * (cA ? rg.mva : rg.mvb);
    const int o = q >> 3, fr = q & 7;
    const WpTab T{wo, wv, h};
    const uint32_t ysz = (uint32_t)w * (uint32_t)h, csz = ysz / 4;
    RefPics P;
    P.w = w;
    P.h = h;
    for (int i = 0; i < 2; ++i) {
        P.pl[i][0] = rb + (size_t)i * (ysz + 2 * csz);
        P.pl[i][1] = P.pl[i][0] + ysz;
        P.pl[i][2] = P.pl[i][1] + csz;
    }
    for (int x = 0; x < 4; ++x) {
        const int a = chroma_px_any<9>(T, P, ref, 1 + p, X + x, yrow + o);
        const int b = fr ? chroma_px_any<9>(T, P, ref, 1 + p, X + x, yrow + o + 1) : 0;
        pred[x] = ((8 - fr) * a + fr * b + 4) >> 3;
    }
}

/* GEN = false: grid (rect MB rows, frames, streams), every row whose chroma
 * prediction rows are plain; GEN = true: grid (rect MB rows, record slots),
 * the frames k_dyn_rows listed for the general path (ctr[1] of them from
 * ctr[DYN_CTR_LIST], as k_dyn_row<true> takes them), the rows with a
 * half-pel waypoint chain.  The bilinear tree behind that branch is a chain
 * of calls (218 VGPRs and 248 bytes of scratch with it in the kernel), so it
 * has its own instantiation and the common one stays free of calls. */
template <bool GEN>
__global__ __launch_bounds__(RC_T) void k_dyn_recon(const DevStream *__restrict__ st,
                                                    const NalDesc *__restrict__ nal, int ld_nal,
                                                    const PlanPending *__restrict__ pend,
                                                    const DynFrame *__restrict__ dfr, int ld_fr, DynGeom g,
                                                    const uint32_t *__restrict__ rows,
                                                    const uint8_t *__restrict__ src,
                                                    const uint8_t *__restrict__ refs, uint8_t *__restrict__ rec,
                                                    unsigned long long *__restrict__ sse,
                                                    const uint32_t *__restrict__ ctr)
{
    __shared__ ReconLds L;
    const int r = blockIdx.x, t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    size_t nb;
    if (GEN) {
        if ((uint32_t)blockIdx.y >= min(ctr[1], g.gen_cap)) return;
        nb = ctr[DYN_CTR_LIST + blockIdx.y];
    } else {
        nb = (size_t)blockIdx.z * ld_fr + blockIdx.y;
    }
    const int s = (int)(nb / (size_t)ld_fr), f = (int)(nb - (size_t)s * ld_fr);
    const DynFrame df = dfr[nb];
    if (df.nal < 0) return;                              /* no dynamic NAL in this frame */
    if (t < 32)
        L.rt[t] = rows[nb * (size_t)(32 * g.h) +
                       (t < 16 ? 16 * r + t : 16 * g.h + (t < 24 ? 8 * r + t - 16 : 8 * g.h + 8 * r + t - 24))];
    else if (t >= 64 && t < 72) {
        L.wo[t - 64] = pend[s].wo[t - 64];
        L.wv[t - 64] = pend[s].wv[t - 64];
    }
    __syncthreads();
    {
        bool gen = false;                               /* some chroma row of this MB row needs the tree */
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t ea = L.rt[16 + i], eb = L.rt[24 + i];
            gen |= (ea & ROW_GEN) || (((ea >> 28) & 7u) && (eb & ROW_GEN));
        }
        if (gen != GEN) return;
    }

    const int qpy = __builtin_amdgcn_readfirstlane(st[s].dyn_qp);
    const int qpc = qp_chroma(qpy);
    const QParams ql = qparams_rt(qpy), qc = qparams_rt(qpc);
    const DQParams dl = dqparams_rt(qpy), dc = dqparams_rt(qpc);
    const uint32_t ysz = (uint32_t)g.pw * (uint32_t)g.ph, csz = ysz / 4;
    const uint8_t *rb = refs + (size_t)s * g.ref_ld;
    const size_t fo = (size_t)s * g.src_ld + (size_t)f * g.src_fr;     /* source and recon share the layout */
    const int ndt = g.w * g.h;
    const int lstride = 16 * g.w, cstride = 8 * g.w;
    const int nl = 16 * g.w, nl64 = (nl + 63) & ~63;
    const int gc = (2 * g.w + 31) >> 5;                  /* chroma waves per plane */
    const int total = nl64 + 128 * gc;
    const uint32_t m_4w = magic32((uint32_t)(4 * g.w));

    uint32_t e0 = 0, e1 = 0, e2 = 0;                     /* this thread's squared error: Y, Cb, Cr */
    for (int base = 0; base < total; base += RC_T) {
        const int wb = __builtin_amdgcn_readfirstlane(base + (t & ~63));   /* the wave's first slot */
        if (wb >= total) continue;
        if (wb < nl64) {                                 /* luma, raster */
            const int slot = wb + lane;
            if (slot >= nl) continue;
            const int by = (int)div_m((uint32_t)slot, m_4w), bx = slot - by * 4 * g.w;
            const size_t po = fo + (size_t)(16 * r + 4 * by) * lstride + 4 * bx;
            const uint8_t *pp = rb + 16 * g.x0 + 4 * bx;
            uint32_t sv[4], pv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sv[i] = ld32(src + po + (size_t)i * lstride);
                pv[i] = ld32(pp + L.rt[4 * by + i]);
            }
            int W[16], res[16];
            block_fwd(sv, pv, W);
            recon_residual<false>(W, 0, res, ql, dl);
            e0 += block_store(sv, pv, res, rec + po, lstride);
        } else {                                         /* chroma: plane p, wave grp of it */
            const int cw = (wb - nl64) >> 6;
            const int p = cw >= gc ? 1 : 0, grp = cw - p * gc;
            const int by = lane >> 5, bx = 32 * grp + (lane & 31);
            const bool act = bx < 2 * g.w;
            const size_t po = fo + (size_t)256 * ndt + (size_t)p * 64 * ndt + (size_t)(8 * r + 4 * by) * cstride + 4 * bx;
            uint32_t sv[4] = {0, 0, 0, 0}, pv[4] = {0, 0, 0, 0};
            int W[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) W[k] = 0;
            if (act) {
                const int X = 8 * g.x0 + 4 * bx;
                const uint8_t *cp = rb + (size_t)p * csz + X;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sv[i] = ld32(src + po + (size_t)i * cstride);
                    const uint32_t ea = L.rt[16 + 4 * by + i], eb = L.rt[24 + 4 * by + i];
                    const uint32_t fr = (ea >> 28) & 7u;
                    int pr[4];
                    if (!GEN || (!(ea & ROW_GEN) && !(fr && (eb & ROW_GEN)))) {
                        int a[4], b[4];
                        unpack4(ld32(cp + (ea & ROW_OFF)), a);
                        unpack4(fr ? ld32(cp + (eb & ROW_OFF)) : 0u, b);
#pragma unroll
                        for (int x = 0; x < 4; ++x) pr[x] = ((8 - (int)fr) * a[x] + (int)fr * b[x] + 4) >> 3;
                    } else if constexpr (GEN) {          /* a half-pel waypoint step: any depth */
                        chroma_pred_any(st + s, nal[(size_t)s * ld_nal + df.nal], L.wo, L.wv, rb, g.y0 + r, p, X,
                                        8 * (g.y0 + r) + 4 * by + i, pr);
                    }
                    pv[i] = pack4(pr);
                }
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
        L.red[wave][0] = e0;
        L.red[wave][1] = e1;
        L.red[wave][2] = e2;
    }
    __syncthreads();
    if (t < 3) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < RC_NW; ++k) v += L.red[k][t];
        if (v) atomicAdd(&sse[nb * 3 + t], (unsigned long long)v);
    }
}

}  // namespace

int recon_launch(hipStream_t hs, int nframes, int S, const DevStream *st, const NalDesc *nal, int ld_nal,
                 const PlanPending *pend, const DynFrame *dfr, int ld_fr, const DynGeom *g,
                 const uint32_t *rows, const uint8_t *src, const uint8_t *refs, uint8_t *rec,
                 unsigned long long *sse, const uint32_t *ctr, hipEvent_t ev0, hipEvent_t ev1)
{
    if (nframes <= 0 || S <= 0) return 0;
    if (hipMemsetAsync(sse, 0, (size_t)S * ld_fr * 3 * sizeof(unsigned long long), hs) != hipSuccess) return -1;
    if (ev0 && hipEventRecord(ev0, hs) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dyn_recon<false>, dim3(g->h, nframes, S), dim3(RC_T), 0, hs, st, nal, ld_nal, pend, dfr,
                       ld_fr, *g, rows, src, refs, rec, sse, ctr);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dyn_recon<true>, dim3(g->h, std::min<uint32_t>(g->gen_cap, (uint32_t)(nframes * S))),
                       dim3(RC_T), 0, hs, st, nal, ld_nal, pend, dfr, ld_fr, *g, rows, src, refs, rec, sse, ctr);
    if (hipGetLastError() != hipSuccess) return -1;
    if (ev1 && hipEventRecord(ev1, hs) != hipSuccess) return -1;
    return 0;
}
