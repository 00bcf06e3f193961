/*
 * hprobe_kernels.hip -- MI355X (gfx950) kernels of the QP probe of the
 * dynamic rect under UI hints (scroll_batch_dyn_probe_hinted, DESIGN.md §3j,
 * "Under UI hints"): per frame and candidate QP, the squared error a decoder
 * would see in the rect, the bits its MBs would cost and their non-zero
 * levels, for the rect k_hdyn_code would code -- under the frame's hint
 * rects at the frame's own position, or the whole picture of a frame that
 * falls back.
 *
 * k_hprobe_class decides per frame what the next compose would make of it
 * (nothing to probe, hinted, falls back, fails) into a buffer of the probe's
 * own; the test for a rect on a missing reference is k_hint_fb's
 * (hint_device.h bad_ref_share), and HintFrame.mode is not written.
 *
 * k_hdyn_probe is k_hdyn_recon's prologue and predictor around
 * probe_block.h's probe_row, k_dyn_probe's row loop with the predictor as a
 * parameter: a workgroup is one rect MB row of one frame, grid (h, frames,
 * streams), 256 threads.  The row's MBs, and those of the rect row above whose TotalCoeffs
 * nC needs, resolve their (ref, mv) from hint_device.h field() once into
 * LDS; rows with an MB whose chroma goes through a half-pel waypoint step
 * run in the second instantiation, which alone holds the bilinear call
 * tree.  No workgroup waits on, polls or hands anything to another: the only
 * cross-workgroup operations are probe_row's final integer atomicAdds and
 * the row counter, into buffers a hipMemsetAsync zeroed.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "hrecon_device.h"
#include "probe_block.h"
#include "hint_device.h"
#include "hprobe_engine.h"
#include "nal_ctx.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::hint;
using namespace scroll::recon;
using namespace scroll::hrecon;
using namespace scroll::probe;

namespace {

constexpr int HC_T = 256;

__global__ __launch_bounds__(HC_T) void k_hprobe_class(const DevStream *__restrict__ st,
                                                       const NalDesc *__restrict__ nal, int ld_nal,
                                                       const PlanPending *__restrict__ pend,
                                                       const DynFrame *__restrict__ dfr, int ld_fr,
                                                       const HintFrame *__restrict__ hf,
                                                       const ScrollHintRect *__restrict__ pool,
                                                       const SpliceFrame *__restrict__ spf, int fallback,
                                                       uint8_t *__restrict__ cls)
{
    __shared__ ScrollHintRect rc[SCROLL_HINT_MAX_RECTS];
    __shared__ int32_t wv[8];
    const int s = blockIdx.y, f = blockIdx.x, t = threadIdx.x;
    const size_t fi = (size_t)s * ld_fr + f;
    const HintFrame H = hf[fi];
    const int j = dfr[fi].nal;
    const int nr = min((int)H.n, SCROLL_HINT_MAX_RECTS);
    bool bad = false;
    if (j >= 0 && nr > 0) {                                /* uniform */
        if (t < nr) rc[t] = pool[H.first + t];
        if (t < 8) wv[t] = pend[s].wv[t];
        __syncthreads();
        const DevStream *S = st + s;
        const int nwp = nal[(size_t)s * ld_nal + j].nwp;
        const int mbw = S->w / 16, nmb = mbw * (S->h / 16);
        bad = __syncthreads_or(bad_ref_share(rc, wv, nr, mbw, nmb, nwp, t, HC_T)) != 0;
    }
    if (t == 0) {
        const SpliceFrame SF = spf[fi];
        int c;
        if (j < 0) c = HPROBE_NONE;                        /* experiment mode: no scroll NAL */
        else if (bad) c = fallback ? HPROBE_FB : HPROBE_FAIL;
        else if (SF.w <= 0 || (SF.pad & 1)) c = HPROBE_NONE;   /* no rect / a dormant fallback region */
        else c = HPROBE_HINT;
        cls[fi] = (uint8_t)c;
    }
}

struct HprobeLds {
    ScrollHintRect rc[SCROLL_HINT_MAX_RECTS];
    int32_t wo[8], wv[8];
    HrMb mb[DYN_MAX_W], mba[DYN_MAX_W];     /* the row's MBs, those of the rect row above */
    ProbeRowLds row;
};

/* probe_row's predictor: a block's prediction at its MB's resolved motion
 * (mb[]); the row's first MB is (mbx, mby) of the picture */
template <bool GEN>
struct HintRowPred {
    const HrMb *mb;
    const WpTab &T;
    const Pics &R;
    int mbx, mby;

    __device__ inline void luma(int by, int bx, uint32_t pv[4]) const
    {
        const HrMb m = mb[bx >> 2];
        pred_luma4x4(T, R, m.ref, m.mvx, m.mvy, 16 * mbx + 4 * bx, 16 * mby + 4 * by, pv);
    }
    __device__ inline void chroma(int p, int by, int bx, uint32_t pv[4]) const
    {
        const HrMb m = mb[bx >> 1];
        const int X = 8 * mbx + 4 * bx, Y = 8 * mby + 4 * by;
        if (!GEN || !(m.fl & HR_GEN)) pred_chroma4x4<false>(T, R, m.ref, p, m.mvx, m.mvy, X, Y, pv);
        else if constexpr (GEN) pred_chroma4x4<true>(T, R, m.ref, p, m.mvx, m.mvy, X, Y, pv);
    }
};

template <bool GEN>
__global__ __launch_bounds__(PB_T) void k_hdyn_probe(const DevStream *__restrict__ st,
                                                     const NalDesc *__restrict__ nal, int ld_nal,
                                                     const PlanPending *__restrict__ pend,
                                                     const DynFrame *__restrict__ dfr, int ld_fr,
                                                     const HintFrame *__restrict__ hf,
                                                     const ScrollHintRect *__restrict__ pool,
                                                     const SpliceFrame *__restrict__ spf,
                                                     const uint8_t *__restrict__ cls, DynGeom g,
                                                     const uint8_t *__restrict__ src,
                                                     const uint8_t *__restrict__ refs, uint64_t qps, int nq,
                                                     ScrollDynProbe *__restrict__ res, uint32_t *__restrict__ done)
{
    extern __shared__ __align__(16) uint8_t dl[];
    __shared__ HprobeLds L;
    const int r = blockIdx.x, f = blockIdx.y, s = blockIdx.z, t = threadIdx.x;
    if (GEN) {
        /* a half-pel step needs a valid waypoint at an odd offset: without
         * one this instantiation has nothing to do (as k_hdyn_recon<true>) */
        bool odd = false;
        for (int i = 0; i < 8; ++i) odd |= pend[s].wv[i] && (pend[s].wo[i] & 1);
        if (!odd) return;
    }
    const size_t fi = (size_t)s * ld_fr + f;
    const int c = cls[fi];
    if (c != HPROBE_HINT && c != HPROBE_FB) return;         /* nothing to probe, or the compose would fail */
    const DynFrame df = dfr[fi];
    const SpliceFrame SF = spf[fi];
    if (df.nal < 0 || SF.w <= 0) return;
    const bool fb = c == HPROBE_FB;
    if ((SF.pad & 1) && !fb) return;                        /* a dormant fallback region */
    const HintFrame H = hf[fi];
    const int nr = fb ? 0 : min((int)H.n, SCROLL_HINT_MAX_RECTS);
    const bool above = r > 0;                               /* the row above is a rect row */
    if (t < 8) {
        L.wo[t] = pend[s].wo[t];
        L.wv[t] = pend[s].wv[t];
    }
    for (int i = t; i < nr; i += PB_T) L.rc[i] = pool[H.first + i];
    load_plens(L.row.pl);
    __syncthreads();
    const DevStream *S = st + s;
    const WpTab T{L.wo, L.wv, S->h};
    bool gen = false;
    const int w = g.w;
    /* one MB per thread and pass: the row's, then those of the row above (2 w
     * may pass the workgroup) */
    for (int i = t; i < (above ? 2 * w : w); i += PB_T) {
        const bool up = i >= w;
        const int m = up ? i - w : i, mby = SF.y0 + (up ? r - 1 : r);
        const NalDesc d = nal[(size_t)s * ld_nal + df.nal];
        const NalCtx cx = nal_ctx(S, d, L.wo, L.wo, L.wv);   /* regions() does not read the long-term indices */
        const Layout lay = layout(cx);
        bool bad;
        const Mv me = field(L.rc, L.wv, nr, SF.x0 + m, mby, lay, cx.nwp, bad);
        const int mvy = me.my / 4;
        const bool gm = !bad && chroma_needs_gen(T, me.ref, mvy, mby);
        gen |= gm;
        const HrMb e{(int16_t)me.ref, (int16_t)((bad ? HR_BAD : 0) | (gm ? HR_GEN : 0)), (int16_t)(me.mx / 4),
                     (int16_t)mvy};
        if (up) L.mba[m] = e;
        else L.mb[m] = e;
    }
    if ((__syncthreads_or(gen) != 0) != GEN) return;

    const Pics R{refs + (size_t)s * g.ref_ld, g.pw, g.ph};
    const HintRowPred<GEN> P{L.mb, T, R, SF.x0, SF.y0 + r};
    const HintRowPred<GEN> Pa{L.mba, T, R, SF.x0, SF.y0 + r - 1};
    probe_row<PB_T>(P, Pa, L.row, dl, w, g.h, SF.x0, SF.y0, r, above, (size_t)s * g.src_ld + (size_t)f * g.src_fr,
                    src, qps, nq, res + fi * PB_Q, done + fi);
}

}  // namespace

int hprobe_launch(hipStream_t hs, int nframes, int S, const DevStream *st, const NalDesc *nal, int ld_nal,
                  const PlanPending *pend, const DynFrame *dfr, int ld_fr, const HintFrame *hf,
                  const ScrollHintRect *pool, const SpliceFrame *spf, int fallback, const DynGeom *g,
                  const uint8_t *src, const uint8_t *refs, const ProbeQps *q, uint8_t *cls, ScrollDynProbe *res,
                  uint32_t *done, hipEvent_t ev1)
{
    if (nframes <= 0 || S <= 0) return 0;
    if (g->w > DYN_MAX_W || q->n < 1 || q->n > PB_Q) return -1;
    uint64_t qps = 0;
    for (int k = 0; k < q->n; ++k) qps |= (uint64_t)q->qp[k] << (8 * k);
    const size_t lds = probe_lds_bytes(g->w, q->n);
    if (lds + sizeof(HprobeLds) > 65536) {
        /* wide rects at many candidates: dynamic LDS past the 64 KB default */
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hdyn_probe<false>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hdyn_probe<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return -1;
    }
    if (hipMemsetAsync(res, 0, (size_t)S * ld_fr * PB_Q * sizeof(ScrollDynProbe), hs) != hipSuccess ||
        hipMemsetAsync(done, 0, (size_t)S * ld_fr * sizeof(uint32_t), hs) != hipSuccess ||
        hipMemsetAsync(cls, 0, (size_t)S * ld_fr, hs) != hipSuccess)
        return -1;
    hipLaunchKernelGGL(k_hprobe_class, dim3(nframes, S), dim3(HC_T), 0, hs, st, nal, ld_nal, pend, dfr, ld_fr, hf,
                       pool, spf, fallback, cls);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_hdyn_probe<false>, dim3(g->h, nframes, S), dim3(PB_T), lds, hs, st, nal, ld_nal, pend, dfr,
                       ld_fr, hf, pool, spf, cls, *g, src, refs, qps, q->n, res, done);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_hdyn_probe<true>, dim3(g->h, nframes, S), dim3(PB_T), lds, hs, st, nal, ld_nal, pend, dfr,
                       ld_fr, hf, pool, spf, cls, *g, src, refs, qps, q->n, res, done);
    if (hipGetLastError() != hipSuccess) return -1;
    if (ev1 && hipEventRecord(ev1, hs) != hipSuccess) return -1;
    return 0;
}
