/*
 * hrecon_kernels.hip -- MI355X (gfx950) kernel of the dynamic rect's
 * reconstruction under UI hints (scroll_batch_set_dyn_recon_hinted,
 * DESIGN.md §3i): the picture a decoder displays for the rect of every
 * frame k_hdyn_code codes (hints, per-frame rect position and QP, the
 * whole-picture fallback), and its squared error against the source.
 *
 * k_hdyn_recon takes each rect MB's (ref, mv) from hint_device.h field() over
 * the frame's hint rects (none in a frame that fell back) exactly as
 * k_hdyn_code resolves it, fetches the prediction at that motion
 * (hrecon_device.h), makes the levels with the coder's own fwd4x4 / quant /
 * quant_dc at the frame's QP (SpliceFrame.hd_qp) and runs the decoder's half
 * on them (recon_device.h).  It is independent of k_hdyn_code and
 * k_splice_stage: no workgroup waits on another one.
 *
 * Workgroup = one rect MB row of one frame, 256 threads, grid (h, frames,
 * streams); the slot layout is k_dyn_recon's (recon_kernels.hip): luma blocks
 * in raster order, then per plane waves whose lanes l, l ^ 1, l ^ 32, l ^ 33
 * hold one MB's four chroma blocks (DCs by __shfl_xor).  The row's MBs
 * resolve their motion once into LDS, one thread per MB; a bad MB (its hint
 * names no valid reference: k_splice_stage fails the stream) writes nothing.
 * Rows with an MB whose chroma goes through a half-pel waypoint step run in
 * the template's second instantiation, which alone holds the bilinear call
 * tree.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrecon_device.h"
#include "recon_block.h"
#include "hint_device.h"
#include "hrecon_engine.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::hint;
using namespace scroll::recon;
using namespace scroll::hrecon;

namespace {

constexpr int HR_T = 256, HR_NW = HR_T / 64;
constexpr int HR_BAD = 1, HR_GEN = 2;

struct HrMb {
    int16_t ref, fl, mvx, mvy;          /* motion in pixels (|mv| <= SCROLL_HINT_MAX_MV, the picture's height) */
};

struct HreconLds {
    ScrollHintRect rc[SCROLL_HINT_MAX_RECTS];
    int32_t wo[8], wv[8];
    HrMb mb[DYN_MAX_W];
    uint32_t red[HR_NW][3];
};

template <bool GEN>
__global__ __launch_bounds__(HR_T) void k_hdyn_recon(const DevStream *__restrict__ st,
                                                     const NalDesc *__restrict__ nal, int ld_nal,
                                                     const PlanPending *__restrict__ pend,
                                                     const DynFrame *__restrict__ dfr, int ld_fr,
                                                     const HintFrame *__restrict__ hf,
                                                     const ScrollHintRect *__restrict__ pool,
                                                     const SpliceFrame *__restrict__ spf, DynGeom g,
                                                     const uint8_t *__restrict__ src,
                                                     const uint8_t *__restrict__ refs, uint8_t *__restrict__ rec,
                                                     unsigned long long *__restrict__ sse)
{
    __shared__ HreconLds L;
    const int r = blockIdx.x, f = blockIdx.y, s = blockIdx.z, t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    if (GEN) {
        /* a half-pel step needs a valid waypoint at an odd offset (a step is
         * wo, wo - wo' or wo - h, h even): without one this instantiation
         * has nothing to do, and ends before it loads anything else */
        bool odd = false;
        for (int i = 0; i < 8; ++i) odd |= pend[s].wv[i] && (pend[s].wo[i] & 1);
        if (!odd) return;
    }
    const size_t fi = (size_t)s * ld_fr + f;
    const DynFrame df = dfr[fi];
    if (df.nal < 0) return;                                 /* experiment mode: no scroll NAL */
    const SpliceFrame SF = spf[fi];
    if (SF.w <= 0) return;                                  /* no rect in this frame */
    const HintFrame H = hf[fi];
    const bool fb = (H.mode & HINT_MODE_FB) != 0;
    if ((SF.pad & 1) && !fb) return;                        /* a dormant fallback region */
    const int nr = fb ? 0 : min((int)H.n, SCROLL_HINT_MAX_RECTS);
    if (t < 8) {
        L.wo[t] = pend[s].wo[t];
        L.wv[t] = pend[s].wv[t];
    }
    for (int i = t; i < nr; i += HR_T) L.rc[i] = pool[H.first + i];
    __syncthreads();
    const DevStream *S = st + s;
    const WpTab T{L.wo, L.wv, S->h};
    bool gen = false;
    if (t < g.w) {                                          /* one thread per MB of the row */
        const NalDesc d = nal[(size_t)s * ld_nal + df.nal];
        NalCtx c;
        c.w = S->w;
        c.h = S->h;
        c.log2_mfn = S->log2_mfn;
        c.poc_type = S->poc_type;
        c.log2_poc = S->log2_poc;
        c.deblock = S->deblock;
        c.kind = d.kind;
        c.off = d.off;
        c.frame_num = d.frame_num;
        c.nwp = d.nwp;
        c.wp_off = L.wo;
        c.wp_lt = L.wo;                                     /* regions() does not read the long-term indices */
        c.wp_valid = L.wv;
        const Regions rg = regions(c);
        const Layout lay{(c.h - c.off) / 16, rg.ra, 4 * rg.mva, rg.rb, 4 * rg.mvb};
        bool bad;
        const Mv me = field(L.rc, L.wv, nr, SF.x0 + t, SF.y0 + r, lay, c.nwp, bad);
        const int mvy = me.my / 4;
        gen = !bad && chroma_needs_gen(T, me.ref, mvy, SF.y0 + r);
        L.mb[t] = HrMb{(int16_t)me.ref, (int16_t)((bad ? HR_BAD : 0) | (gen ? HR_GEN : 0)), (int16_t)(me.mx / 4),
                       (int16_t)mvy};
    }
    if ((__syncthreads_or(gen) != 0) != GEN) return;

    const int qpy = __builtin_amdgcn_readfirstlane(SF.hd_qp);
    const int qpc = qp_chroma(qpy);
    const QParams ql = qparams_rt(qpy), qc = qparams_rt(qpc);
    const DQParams dl = dqparams_rt(qpy), dc = dqparams_rt(qpc);
    const Pics P{refs + (size_t)s * g.ref_ld, g.pw, g.ph};
    const size_t fo = (size_t)s * g.src_ld + (size_t)f * g.src_fr;     /* source and recon share the layout */
    const int ndt = g.w * g.h;
    const int lstride = 16 * g.w, cstride = 8 * g.w;
    const int nl = 16 * g.w, nl64 = (nl + 63) & ~63;
    const int gc = (2 * g.w + 31) >> 5;                  /* chroma waves per plane */
    const int total = nl64 + 128 * gc;
    const uint32_t m_4w = magic32((uint32_t)(4 * g.w));

    uint32_t e0 = 0, e1 = 0, e2 = 0;                     /* this thread's squared error: Y, Cb, Cr */
    for (int base = 0; base < total; base += HR_T) {
        const int wb = __builtin_amdgcn_readfirstlane(base + (t & ~63));   /* the wave's first slot */
        if (wb >= total) continue;
        if (wb < nl64) {                                 /* luma, raster */
            const int slot = wb + lane;
            if (slot >= nl) continue;
            const int by = (int)div_m((uint32_t)slot, m_4w), bx = slot - by * 4 * g.w;
            const HrMb m = L.mb[bx >> 2];
            if (m.fl & HR_BAD) continue;
            const size_t po = fo + (size_t)(16 * r + 4 * by) * lstride + 4 * bx;
            uint32_t sv[4], pv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) sv[i] = ld32(src + po + (size_t)i * lstride);
            pred_luma4x4(T, P, m.ref, m.mvx, m.mvy, 16 * SF.x0 + 4 * bx, 16 * (SF.y0 + r) + 4 * by, pv);
            int W[16], res[16];
            block_fwd(sv, pv, W);
            recon_residual<false>(W, 0, res, ql, dl);
            e0 += block_store(sv, pv, res, rec + po, lstride);
        } else {                                         /* chroma: plane p, wave grp of it */
            const int cw = (wb - nl64) >> 6;
            const int p = cw >= gc ? 1 : 0, grp = cw - p * gc;
            const int by = lane >> 5, bx = 32 * grp + (lane & 31);
            const HrMb m = L.mb[min(bx >> 1, g.w - 1)];
            const bool act = bx < 2 * g.w && !(m.fl & HR_BAD);   /* the same for an MB's four lanes */
            const size_t po = fo + (size_t)256 * ndt + (size_t)p * 64 * ndt + (size_t)(8 * r + 4 * by) * cstride + 4 * bx;
            uint32_t sv[4] = {0, 0, 0, 0}, pv[4] = {0, 0, 0, 0};
            int W[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) W[k] = 0;
            if (act) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sv[i] = ld32(src + po + (size_t)i * cstride);
                const int X = 8 * SF.x0 + 4 * bx, Y = 8 * (SF.y0 + r) + 4 * by;
                if (!GEN || !(m.fl & HR_GEN)) pred_chroma4x4<false>(T, P, m.ref, p, m.mvx, m.mvy, X, Y, pv);
                else if constexpr (GEN) pred_chroma4x4<true>(T, P, m.ref, p, m.mvx, m.mvy, X, Y, pv);
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
        for (int k = 0; k < HR_NW; ++k) v += L.red[k][t];
        if (v) atomicAdd(&sse[fi * 3 + t], (unsigned long long)v);
    }
}

}  // namespace

int hrecon_launch(hipStream_t hs, int nframes, int S, const DevStream *st, const NalDesc *nal, int ld_nal,
                  const PlanPending *pend, const DynFrame *dfr, int ld_fr, const HintFrame *hf,
                  const ScrollHintRect *pool, const SpliceFrame *spf, const DynGeom *g, const uint8_t *src,
                  const uint8_t *refs, uint8_t *rec, unsigned long long *sse, hipEvent_t ev0, hipEvent_t ev1)
{
    if (nframes <= 0 || S <= 0) return 0;
    if (g->w > DYN_MAX_W) return -1;
    if (hipMemsetAsync(sse, 0, (size_t)S * ld_fr * 3 * sizeof(unsigned long long), hs) != hipSuccess) return -1;
    if (ev0 && hipEventRecord(ev0, hs) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_hdyn_recon<false>, dim3(g->h, nframes, S), dim3(HR_T), 0, hs, st, nal, ld_nal, pend, dfr,
                       ld_fr, hf, pool, spf, *g, src, refs, rec, sse);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_hdyn_recon<true>, dim3(g->h, nframes, S), dim3(HR_T), 0, hs, st, nal, ld_nal, pend, dfr,
                       ld_fr, hf, pool, spf, *g, src, refs, rec, sse);
    if (hipGetLastError() != hipSuccess) return -1;
    if (ev1 && hipEventRecord(ev1, hs) != hipSuccess) return -1;
    return 0;
}
