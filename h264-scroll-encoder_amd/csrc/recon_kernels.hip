/*
 * recon_kernels.hip -- MI355X (gfx950) kernel of the dynamic rect's
 * reconstruction (scroll_batch_set_dyn_recon): the picture a
 * decoder displays for the rect of every dynamic NAL, and its sum of squared
 * errors against the source, per frame and plane.
 *
 * k_dyn_recon repeats the coder's forward half per 4x4 block with the
 * coder's own functions (dyn_device.h: fwd4x4, quant, quant_dc at the
 * frame's QP / QPc), so its levels are the coded ones, and runs the
 * decoder's half on them (recon_device.h).  It reads k_dyn_rows' prediction
 * rows and is independent of k_dyn_row: levels stay in 32-bit registers, so
 * the same code serves the int8 path and the general path (QP < 22); rows
 * with a half-pel waypoint chain run in the template's second instantiation.
 *
 * Workgroup = one rect MB row of one dynamic NAL, 256 threads: the row loop,
 * its task slots and the squared-error reduction are recon_block.h's
 * recon_row, shared with k_hdyn_recon; this kernel's part is the prediction
 * (RowPred of recon_pred.h: the row's prediction rows, in LDS).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <algorithm>

#include "recon_device.h"
#include "recon_block.h"
#include "dyn_engine.h"
#include "dyn_pos.h"
#include "nal_ctx.h"
#include "recon_engine.h"
#include "recon_pred.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::recon;

namespace {

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
    dyn_frame_geom(g, nb);                               /* RowPred's origin: the frame's own */
    if (r >= g.h) return;                                /* past the rows of a frame sized on its own */
    if (t < 32)
        L.rt[t] = rows[nb * (size_t)(32 * g.ld_h) +
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

    const uint8_t *rb = refs + (size_t)s * g.ref_ld;
    const RowPred<GEN> P{L, rb, (uint32_t)g.pw * (uint32_t)g.ph / 4, g.x0, g.y0 + r, st + s,
                         nal + (size_t)s * ld_nal + df.nal};
    /* the frame's rect QP: k_dyn_rows left it in DynFrame.ep (k_dyn_epfix runs after this kernel) */
    recon_row<RC_T>(P, __builtin_amdgcn_readfirstlane((int)df.ep), g, r,
                    (size_t)s * g.src_ld + (size_t)f * g.src_fr, src, rec, L.red, sse + nb * 3);
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
