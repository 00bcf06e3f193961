/*
 * recon_pred.h -- the prediction of a rect MB row from k_dyn_rows' prediction
 * rows (dyn_kernels.hip), for the kernels that read them: k_dyn_recon
 * (recon_kernels.hip) and k_dyn_probe (probe_kernels.hip).  ReconLds holds
 * the row's 32 entries, RowPred is recon_row's predictor over them, and
 * chroma_pred_any the sampler behind a half-pel waypoint chain.  Device only.
 */
#ifndef SCROLL_RECON_PRED_H
#define SCROLL_RECON_PRED_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "recon_device.h"
#include "recon_block.h"
#include "nal_ctx.h"

namespace scroll {
namespace recon {

using namespace scroll::dyn;

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

}  // namespace recon
}  // namespace scroll

#endif
