/*
 * hrecon_device.h -- prediction fetch of the dynamic rect's reconstruction
 * under UI hints (k_hdyn_recon, hrecon_kernels.hip): the 16 prediction
 * samples of a 4x4 block at an MB's hinted motion (ref, mvx, mvy in pixels),
 * as k_hdyn_code (hdyn_kernels.hip) and oracle/splice_oracle.c hd_pred take
 * them:
 *   luma    full-pel, row y through luma_row (waypoints through their own
 *           rows), columns clamped to the picture;
 *   chroma  2-D 1/8-pel bilinear at mv / 2 (8.4.2.2.2), rows through
 *           chroma_row while the waypoint chain is full-pel, per sample
 *           through chroma_px_any<9> at a half-pel step (GEN), columns
 *           clamped to the picture.
 * A block row is 4 (luma) or 5 (chroma) bytes at any byte alignment: inside
 * the picture two aligned dword loads and a byte shift, else a clamp per
 * sample.  Rows come back packed, byte j = column j.
 *
 * Pure functions of (reference planes, waypoint table): the kernel calls them
 * per lane, tests/hostsim/hrecon_sim.cpp compiles them for the CPU.
 */
#ifndef SCROLL_HRECON_DEVICE_H
#define SCROLL_HRECON_DEVICE_H

#include "recon_device.h"

namespace scroll {
namespace hrecon {

using dyn::chroma_px_any;
using dyn::chroma_row;
using dyn::clampi;
using dyn::luma_row;
using dyn::RefPics;
using dyn::WpTab;
using recon::Pics;

/* a rect MB's resolved motion, as the kernels keep it in LDS (k_hdyn_recon,
 * k_hdyn_probe): pixels (|mv| <= SCROLL_HINT_MAX_MV, the picture's height) */
constexpr int HR_BAD = 1, HR_GEN = 2;
struct HrMb {
    int16_t ref, fl, mvx, mvy;          /* fl: HR_BAD its hint names no valid reference, HR_GEN chroma_needs_gen */
};

/* bytes X .. X + n - 1 (n <= 5) of a row from the aligned dwords that hold
 * them: needs 0 <= X and X + n <= the row's length.  The second dword is
 * loaded only when one of the n bytes lies in it, so no load leaves the
 * dwords the row's own bytes occupy */
__device__ __host__ inline uint64_t row_bytes(const uint8_t *row, int X, int n)
{
    const uintptr_t a = (uintptr_t)(row + X);
    const uint32_t sh = (uint32_t)(a & 3);
    const uint32_t *q = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    const uint32_t lo = q[0], hi = sh + (uint32_t)n > 4u ? q[1] : 0u;
    return (((uint64_t)hi << 32) | lo) >> (8 * sh);
}

/* columns X .. X + 3 of a picture row of W samples, clamped to the picture */
__device__ __host__ inline uint32_t row4(const uint8_t *row, int X, int W)
{
    if (X >= 0 && X + 4 <= W) return (uint32_t)row_bytes(row, X, 4);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) v |= (uint32_t)row[clampi(X + j, 0, W - 1)] << (8 * j);
    return v;
}

/* columns X .. X + 3 (a) and X + 1 .. X + 4 (b), clamped to the picture */
__device__ __host__ inline void row5(const uint8_t *row, int X, int W, uint32_t &a, uint32_t &b)
{
    if (X >= 0 && X + 5 <= W) {
        const uint64_t v = row_bytes(row, X, 5);
        a = (uint32_t)v;
        b = (uint32_t)(v >> 8);
        return;
    }
    a = b = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a |= (uint32_t)row[clampi(X + j, 0, W - 1)] << (8 * j);
        b |= (uint32_t)row[clampi(X + j + 1, 0, W - 1)] << (8 * j);
    }
}

__device__ __host__ inline uint32_t byte_of(uint32_t v, int j) { return (v >> (8 * j)) & 255u; }

/* luma block at (X, Y) of the picture, motion (mvx, mvy) pixels */
__device__ __host__ inline void pred_luma4x4(const WpTab &T, const Pics &R, int ref, int mvx, int mvy, int X,
                                             int Y, uint32_t pv[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int yo;
        const int b = luma_row(T, ref, Y + i + mvy, yo);
        pv[i] = row4(R.plane(b, 0) + (size_t)yo * R.w, X + mvx, R.w);
    }
}

/* (8 - fx) A + fx B of columns x .. x + 3 of chroma row y of reference ref:
 * the bilinear numerator's horizontal half (no rounding before the vertical
 * one) */
template <bool GEN>
__device__ __host__ inline void chroma_hrow(const WpTab &T, const Pics &R, int ref, int p, int x, int y, int fx,
                                            int h[4])
{
    const int wc = R.w / 2;
    int yo = 0;
    const int b = chroma_row(T, ref, y, yo);
    if (!GEN || b >= 0) {
        uint32_t A, B;
        const uint8_t *row = R.plane(b < 0 ? 0 : b, 1 + p) + (size_t)yo * wc;
        if (fx) {
            row5(row, x, wc, A, B);
        } else {
            A = row4(row, x, wc);
            B = 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = (8 - fx) * (int)byte_of(A, j) + fx * (int)byte_of(B, j);
    } else {
        const RefPics P = R.refpics();
        for (int j = 0; j < 4; ++j) {                       /* a half-pel waypoint step: any depth */
            const int A = chroma_px_any<9>(T, P, ref, 1 + p, clampi(x + j, 0, wc - 1), y);
            const int B = fx ? chroma_px_any<9>(T, P, ref, 1 + p, clampi(x + j + 1, 0, wc - 1), y) : 0;
            h[j] = (8 - fx) * A + fx * B;
        }
    }
}

/* chroma block at (X, Y) of plane p (0 Cb, 1 Cr), the MB's luma motion
 * (mvx, mvy) pixels.  GEN = false needs a full-pel waypoint chain on every
 * row it reads (chroma_needs_gen false) */
template <bool GEN>
__device__ __host__ inline void pred_chroma4x4(const WpTab &T, const Pics &R, int ref, int p, int mvx, int mvy,
                                               int X, int Y, uint32_t pv[4])
{
    const int qx = 4 * mvx, qy = 4 * mvy, fx = qx & 7, fy = qy & 7;
    const int x = X + (qx >> 3), y = Y + (qy >> 3);
    int h0[4], h1[4];
    chroma_hrow<GEN>(T, R, ref, p, x, y, fx, h0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t v = 0;
        if (fy) {
            chroma_hrow<GEN>(T, R, ref, p, x, y + i + 1, fx, h1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v |= (uint32_t)(((8 - fy) * h0[j] + fy * h1[j] + 32) >> 6) << (8 * j);
                h0[j] = h1[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v |= (uint32_t)((8 * h0[j] + 32) >> 6) << (8 * j);
            if (i < 3) chroma_hrow<GEN>(T, R, ref, p, x, y + i + 1, fx, h0);
        }
        pv[i] = v;
    }
}

/* does a chroma row the MB at MB row mby reads (8 mby + (4 mvy >> 3) .. + 8)
 * go through a half-pel waypoint step? */
__device__ __host__ inline bool chroma_needs_gen(const WpTab &T, int ref, int mvy, int mby)
{
    if (ref < 2) return false;
    const int y = 8 * mby + ((4 * mvy) >> 3);
    for (int i = 0; i <= 8; ++i) {
        int yo;
        if (chroma_row(T, ref, y + i, yo) < 0) return true;
    }
    return false;
}

}  // namespace hrecon
}  // namespace scroll

#endif
