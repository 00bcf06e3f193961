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
 * Workgroup = one rect MB row of one dynamic NAL, 256 threads: the row loop,
 * its task slots and the squared-error reduction are recon_block.h's
 * recon_row, shared with k_hdyn_recon; this kernel's part is the prediction
 * (RowPred: the row's prediction rows, in LDS).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <algorithm>

#include "recon_device.h"
#include "recon_block.h"
#include "dyn_engine.h"
#include "nal_ctx.h"
#include "recon_engine.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::recon;

namespace {

constexpr int RC_T = 256, RC_NW = RC_T / 64;

/* rows[] entries (k_dyn_rows, dyn_kernels.hip): the chroma fraction in bits
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
    const Regions rg = regions(nal_ctx(S, d, wo, wo, wv));   /* regions() does not read the long-term indices */
    const bool cA = mbrow < (h - d.off) / 16;
    const int ref = cA ? rg.ra : rg.rb, q = 4 * (cA ? rg.mva : rg.mvb);
    const int o = q >> 3, fr = q & 7;
    const WpTab T{wo, wv, h};
    const RefPics P = Pics{rb, w, h}.refpics();
    for (int x = 0; x < 4; ++x) {
        const int a = chroma_px_any<9>(T, P, ref, 1 + p, X + x, yrow + o);
        const int b = fr ? chroma_px_any<9>(T, P, ref, 1 + p, X + x, yrow + o + 1) : 0;
        pred[x] = ((8 - fr) * a + fr * b + 4) >> 3;
    }
}

/* recon_row's predictor: every MB of the row is coded, and block row i of a
 * block predicts from the picture row at L.rt[]'s byte offset (chroma: two
 * rows and their eighth-pel fraction), at the rect's own columns */
template <bool GEN>
struct RowPred {
    const ReconLds &L;
    const uint8_t *rb;                  /* the stream's reference pair */
    uint32_t csz;                       /* bytes of a chroma plane */
    int x0, mbrow;                      /* the rect's first MB column, the row's MB row in the picture */
    const DevStream *S;                 /* GEN: chroma_pred_any's stream and NAL */
    const NalDesc *d;

    __device__ inline bool coded(int) const { return true; }
    __device__ inline void luma(int by, int bx, uint32_t pv[4]) const
    {
        const uint8_t *pp = rb + 16 * x0 + 4 * bx;
#pragma unroll
        for (int i = 0; i < 4; ++i) pv[i] = ld32(pp + L.rt[4 * by + i]);
    }
    __device__ inline void chroma(int p, int by, int bx, uint32_t pv[4]) const
    {
        const int X = 8 * x0 + 4 * bx;
        const uint8_t *cp = rb + (size_t)p * csz + X;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
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
                chroma_pred_any(S, *d, L.wo, L.wv, rb, mbrow, p, X, 8 * mbrow + 4 * by + i, pr);
            }
            pv[i] = pack4(pr);
        }
    }
};

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

    const uint8_t *rb = refs + (size_t)s * g.ref_ld;
    const RowPred<GEN> P{L, rb, (uint32_t)g.pw * (uint32_t)g.ph / 4, g.x0, g.y0 + r, st + s,
                         nal + (size_t)s * ld_nal + df.nal};
    recon_row<RC_T>(P, __builtin_amdgcn_readfirstlane(st[s].dyn_qp), g, r,
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
