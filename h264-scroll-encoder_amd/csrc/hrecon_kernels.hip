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
 * streams): the row loop, its task slots and the squared-error reduction are
 * recon_block.h's recon_row, shared with k_dyn_recon; this kernel's part is
 * the prediction (HintPred).  The row's MBs resolve their motion once into
 * LDS, one thread per MB; a bad MB (its hint names no valid reference:
 * k_splice_stage fails the stream) writes nothing.  Rows with an MB whose
 * chroma goes through a half-pel waypoint step run in the template's second
 * instantiation, which alone holds the bilinear call tree.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrecon_device.h"
#include "recon_block.h"
#include "hint_device.h"
#include "hrecon_engine.h"
#include "nal_ctx.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::hint;
using namespace scroll::recon;
using namespace scroll::hrecon;

namespace {

constexpr int HR_T = 256, HR_NW = HR_T / 64;
struct HreconLds {
    ScrollHintRect rc[SCROLL_HINT_MAX_RECTS];
    int32_t wo[8], wv[8];
    HrMb mb[DYN_MAX_W];
    uint32_t red[HR_NW][3];
};

/* recon_row's predictor: a block's prediction at its MB's resolved motion
 * (L.mb[]); the row's first MB is (mbx, mby) of the picture */
template <bool GEN>
struct HintPred {
    const HreconLds &L;
    const WpTab &T;
    const Pics &R;
    int mbx, mby;

    __device__ inline bool coded(int m) const { return !(L.mb[m].fl & HR_BAD); }
    __device__ inline void luma(int by, int bx, uint32_t pv[4]) const
    {
        const HrMb m = L.mb[bx >> 2];
        pred_luma4x4(T, R, m.ref, m.mvx, m.mvy, 16 * mbx + 4 * bx, 16 * mby + 4 * by, pv);
    }
    __device__ inline void chroma(int p, int by, int bx, uint32_t pv[4]) const
    {
        const HrMb m = L.mb[bx >> 1];
        const int X = 8 * mbx + 4 * bx, Y = 8 * mby + 4 * by;
        if (!GEN || !(m.fl & HR_GEN)) pred_chroma4x4<false>(T, R, m.ref, p, m.mvx, m.mvy, X, Y, pv);
        else if constexpr (GEN) pred_chroma4x4<true>(T, R, m.ref, p, m.mvx, m.mvy, X, Y, pv);
    }
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
        const NalCtx c = nal_ctx(S, d, L.wo, L.wo, L.wv);    /* regions() does not read the long-term indices */
        const Layout lay = layout(c);
        bool bad;
        const Mv me = field(L.rc, L.wv, nr, SF.x0 + t, SF.y0 + r, lay, c.nwp, bad);
        const int mvy = me.my / 4;
        gen = !bad && chroma_needs_gen(T, me.ref, mvy, SF.y0 + r);
        L.mb[t] = HrMb{(int16_t)me.ref, (int16_t)((bad ? HR_BAD : 0) | (gen ? HR_GEN : 0)), (int16_t)(me.mx / 4),
                       (int16_t)mvy};
    }
    if ((__syncthreads_or(gen) != 0) != GEN) return;

    const Pics R{refs + (size_t)s * g.ref_ld, g.pw, g.ph};
    const HintPred<GEN> P{L, T, R, SF.x0, SF.y0 + r};
    recon_row<HR_T>(P, __builtin_amdgcn_readfirstlane(SF.hd_qp), g, r, (size_t)s * g.src_ld + (size_t)f * g.src_fr,
                    src, rec, L.red, sse + fi * 3);
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
