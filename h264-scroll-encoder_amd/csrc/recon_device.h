/*
 * recon_device.h -- device functions of the dynamic rect's reconstruction:
 * what a decoder displays for a rect MB coded by the dynamic-rect coder
 * (dyn_device.h), and its squared error against the source.
 *
 * The levels are the coder's by construction: the same fwd4x4, quant /
 * quant_dc, QParams, +-LEVEL_MAX clamp and QPc (dyn_device.h).  This header
 * adds the decoder's half: dequantisation with flat scaling lists
 * (H.264 8.5.12.1), the chroma DC path (8.5.11.1 / 8.5.11.2), the inverse
 * 4x4 transform (8.5.12.2), prediction + clip; and where the prediction is
 * read from: the addresses of a stream's reference planes (Pics).
 *
 * Pure integer functions like dyn_device.h: k_dyn_recon (recon_kernels.hip)
 * uses them per lane, tests/hostsim/recon_sim.cpp compiles them for the CPU
 * and tests/test_recon_hostsim.py checks them against the test decoder.
 */
#ifndef SCROLL_RECON_DEVICE_H
#define SCROLL_RECON_DEVICE_H

#include "dyn_device.h"

namespace scroll {
namespace recon {

using dyn::clampi;

/* the stream's two reference pictures, I420 one after the other (plane
 * addresses by arithmetic: a pointer table indexed by the picture a row
 * resolves to would live in scratch) */
struct Pics {
    const uint8_t *base;
    int w, h;
    __device__ __host__ inline uint32_t ysz() const { return (uint32_t)w * (uint32_t)h; }
    /* plane p (0 Y, 1 Cb, 2 Cr) of picture b */
    __device__ __host__ inline const uint8_t *plane(int b, int p) const
    {
        const uint32_t y = ysz();
        return base + (size_t)b * (y + y / 2) + (p == 0 ? 0u : p == 1 ? y : y + y / 4);
    }
    __device__ __host__ inline dyn::RefPics refpics() const
    {
        dyn::RefPics R;
        for (int b = 0; b < 2; ++b)
            for (int p = 0; p < 3; ++p) R.pl[b][p] = plane(b, p);
        R.w = w;
        R.h = h;
        return R;
    }
};

/* LevelScale / 16 of the (even, even) / (odd, odd) / mixed 4x4 positions at
 * QP % 6 (Table of 8.5.9, v), shift = QP / 6: the position classes of
 * QParams (mf0 / mf1 / mf2) */
struct DQParams {
    int32_t s0, s1, s2;             /* v << sh of the three classes (<= 29 << 8)  */
    int32_t v0, sh;                 /* the chroma DC path's: v of class 0, QP / 6 */
};
/* for a QP known only at run time (wave-uniform: the selects stay scalar) */
__device__ __host__ inline DQParams dqparams_rt(int qp)
{
    const int r = qp % 6, sh = qp / 6;
    const int v0 = r == 0 ? 10 : r == 1 ? 11 : r == 2 ? 13 : r == 3 ? 14 : r == 4 ? 16 : 18;
    const int v1 = r == 0 ? 16 : r == 1 ? 18 : r == 2 ? 20 : r == 3 ? 23 : r == 4 ? 25 : 29;
    const int v2 = r == 0 ? 13 : r == 1 ? 14 : r == 2 ? 16 : r == 3 ? 18 : r == 4 ? 20 : 23;
    return DQParams{v0 << sh, v1 << sh, v2 << sh, v0, sh};
}

/* one level at raster position pos (8.5.12.1, flat lists): LevelScale =
 * 16 v, so below QP 24 ((c 16 v) + 2^(3 - sh)) >> (4 - sh) is exactly
 * (c v) << sh as it is above: one 24-bit multiply by v << sh.  |level| <=
 * LEVEL_MAX: the product stays below 2^24 (2063 x 29 x 2^8) */
__device__ __host__ inline int dequant(int level, int pos, const DQParams &d)
{
    const int i = pos >> 2, j = pos & 3;
    return __mul24(level, ((i | j) & 1) == 0 ? d.s0 : (((i & j) & 1) ? d.s1 : d.s2));
}

/* a 4x4 block of levels in raster order -> scaled coefficients */
__device__ __host__ inline void dequant4x4(const int lv[16], int c[16], const DQParams &d)
{
#pragma unroll
    for (int p = 0; p < 16; ++p) c[p] = dequant(lv[p], p, d);
}

/* chroma DC (8.5.11.1 / 8.5.11.2): the plane's four quantised DCs (blocks in
 * raster order) -> coefficient 0 of each of its four blocks; d: QPc's */
__device__ __host__ inline void chroma_dc(const int c[4], int dc[4], const DQParams &d)
{
    const int f[4] = {c[0] + c[1] + c[2] + c[3], c[0] - c[1] + c[2] - c[3], c[0] + c[1] - c[2] - c[3],
                      c[0] - c[1] - c[2] + c[3]};
#pragma unroll
    for (int k = 0; k < 4; ++k) dc[k] = (int)((uint32_t)__mul24(f[k], 16 * d.v0) << d.sh) >> 5;   /* |f| <= 8252 */
}

/* inverse 4x4 integer transform (8.5.12.2), (x + 32) >> 6.  Coefficient 0
 * reaches every output with weight 1 and through no halving, so the
 * rounding 32 is added to it once */
__device__ __host__ inline void inv4x4(const int c[16], int r[16])
{
    int t[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c0 = i == 0 ? c[0] + 32 : c[4 * i];
        const int e0 = c0 + c[4 * i + 2], e1 = c0 - c[4 * i + 2];
        const int e2 = (c[4 * i + 1] >> 1) - c[4 * i + 3], e3 = c[4 * i + 1] + (c[4 * i + 3] >> 1);
        t[4 * i + 0] = e0 + e3;
        t[4 * i + 1] = e1 + e2;
        t[4 * i + 2] = e1 - e2;
        t[4 * i + 3] = e0 - e3;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e0 = t[j] + t[8 + j], e1 = t[j] - t[8 + j];
        const int e2 = (t[4 + j] >> 1) - t[12 + j], e3 = t[4 + j] + (t[12 + j] >> 1);
        r[j] = (e0 + e3) >> 6;
        r[4 + j] = (e1 + e2) >> 6;
        r[8 + j] = (e1 - e2) >> 6;
        r[12 + j] = (e0 - e3) >> 6;
    }
}

/* prediction + residual, clipped to 8 bits */
__device__ __host__ inline int add_clip(int pred, int res) { return clampi(pred + res, 0, 255); }

/* levels in raster order (coefficient 0 replaced by dc when DC is set: the
 * chroma AC blocks) -> reconstructed samples */
template <bool DC>
__device__ __host__ inline void recon_levels(const int lv[16], int dc, const int pred[16], int out[16],
                                             const DQParams &d)
{
    int c[16], r[16];
    dequant4x4(lv, c, d);
    if (DC) c[0] = dc;
    inv4x4(c, r);
#pragma unroll
    for (int p = 0; p < 16; ++p) out[p] = add_clip(pred[p], r[p]);
}

/* source - prediction -> the coder's transform coefficients */
__device__ __host__ inline void residual_fwd(const int src[16], const int pred[16], int W[16])
{
    int x[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) x[p] = src[p] - pred[p];
    dyn::fwd4x4(x, W);
}

/* coefficients -> the coded levels (raster; a chroma AC block's position 0
 * is coded in the plane's DC block: left 0 here) */
template <bool DC>
__device__ __host__ inline void quant4x4(const int W[16], int lv[16], const QParams &q)
{
#pragma unroll
    for (int p = 0; p < 16; ++p) lv[p] = (DC && p == 0) ? 0 : dyn::quant(W[p], p, q);
}

/* the plane's four DC coefficients (W[0] of its blocks, raster) -> what the
 * decoder puts at coefficient 0 of each: forward 2x2 Hadamard, quant_dc,
 * then chroma_dc; q / d: QPc's */
__device__ __host__ inline void chroma_dc_coded(const int w0[4], int dc[4], const QParams &q, const DQParams &d)
{
    const int lv[4] = {dyn::quant_dc(w0[0] + w0[1] + w0[2] + w0[3], q), dyn::quant_dc(w0[0] - w0[1] + w0[2] - w0[3], q),
                       dyn::quant_dc(w0[0] + w0[1] - w0[2] - w0[3], q), dyn::quant_dc(w0[0] - w0[1] - w0[2] + w0[3], q)};
    chroma_dc(lv, dc, d);
}

/* squared error of a reconstructed block (<= 16 x 255^2) */
__device__ __host__ inline uint32_t sse16(const int src[16], const int out[16])
{
    uint32_t e = 0;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        const int dd = src[p] - out[p];
        e += (uint32_t)(dd * dd);
    }
    return e;
}

/* coefficients -> the residual a decoder adds to the prediction: quant,
 * dequant, inverse.  DC: a chroma AC block, whose coefficient 0 is dc
 * (chroma_dc_coded of its plane) */
template <bool DC>
__device__ __host__ inline void recon_residual(const int W[16], int dc, int r[16], const QParams &q,
                                               const DQParams &d)
{
    int lv[16], c[16];
    quant4x4<DC>(W, lv, q);
    dequant4x4(lv, c, d);
    if (DC) c[0] = dc;
    inv4x4(c, r);
}

/* that residual + prediction, clipped; returns the squared error */
__device__ __host__ inline uint32_t add_clip_sse(const int r[16], const int src[16], const int pred[16], int out[16])
{
#pragma unroll
    for (int p = 0; p < 16; ++p) out[p] = add_clip(pred[p], r[p]);
    return sse16(src, out);
}

/* coefficients -> reconstruction and its squared error */
template <bool DC>
__device__ __host__ inline uint32_t recon_coefs(const int W[16], int dc, const int src[16], const int pred[16],
                                                int out[16], const QParams &q, const DQParams &d)
{
    int r[16];
    recon_residual<DC>(W, dc, r, q, d);
    return add_clip_sse(r, src, pred, out);
}

/* one luma 4x4 block from pixels to reconstruction: residual -> fwd4x4 ->
 * quant -> dequant -> inverse -> add -> clip; returns the squared error */
__device__ __host__ inline uint32_t recon_luma4x4(const int src[16], const int pred[16], int out[16],
                                                  const QParams &q, const DQParams &d)
{
    int W[16];
    residual_fwd(src, pred, W);
    return recon_coefs<false>(W, 0, src, pred, out, q, d);
}

/* one chroma plane of an MB (its four 4x4 blocks in raster order, which
 * share the DC block) from pixels to reconstruction; q / d: QPc's */
__device__ __host__ inline uint32_t recon_chroma8x8(const int src[4][16], const int pred[4][16], int out[4][16],
                                                    const QParams &q, const DQParams &d)
{
    int W[4][16], w0[4], dc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        residual_fwd(src[k], pred[k], W[k]);
        w0[k] = W[k][0];
    }
    chroma_dc_coded(w0, dc, q, d);
    uint32_t e = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) e += recon_coefs<true>(W[k], dc[k], src[k], pred[k], out[k], q, d);
    return e;
}

}  // namespace recon
}  // namespace scroll

#endif
