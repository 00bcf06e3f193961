/*
 * csc_device.h -- the rule by which 8-bit RGBA / BGRA surface pixels become
 * the I420 samples the dynamic rect codes (scroll_batch_dyn_source_from_surfaces,
 * scroll_batch_surfaces_to_i420).
 *
 * Pure integer functions: k_csc (csc_kernels.hip) runs them per pixel and per
 * 2x2 quad, tests/hostsim/csc_sim.cpp compiles them for the CPU and
 * tests/test_csc_hostsim.py checks them against a numpy restatement of the
 * table below and against the real-valued matrices.
 *
 * Luma, per pixel:
 *     Y = (yr R + yg G + yb B + yoff) >> 16
 * Chroma, per 2x2 quad (box siting: the sample sits at the quad's centre),
 * Sr, Sg, Sb the sums of the four pixels' channels (0..1020):
 *     C = clamp((cr Sr + cg Sg + cb Sb + (128 << 18) + (1 << 17)) >> 18, 0, 255)
 * with an arithmetic (floor) shift; the clamp matters: full-range pure blue
 * gives 256 before it.  Alpha is ignored.
 *
 * Coefficients, Q16.  Luma rows sum to round(65536 219 / 255) = 56284
 * (limited range) or 65536 (full), green taking the remainder; every chroma
 * row sums to 0, green taking the remainder, so grey is exactly 128; yoff =
 * (16 << 16 limited, 0 full) + 32768.  Every output is within 0.5 (rounding)
 * + 3 * 0.5 / 65536 * 255 ~ 0.006 (coefficient rounding) of the real-valued
 * formula.
 */
#ifndef SCROLL_CSC_DEVICE_H
#define SCROLL_CSC_DEVICE_H

#include <stdint.h>

#include "composer_batch.h"     /* SCROLL_SURF_* */

#if !defined(__HIPCC__) && !defined(__device__)
#define __device__
#define __host__
#endif

namespace scroll {
namespace csc {

/* the rule's coefficients by byte position in the pixel (byte 3 is alpha):
 * RGBA has R in byte 0, BGRA has B there */
struct Coef {
    int32_t y[3], yoff;
    int32_t cb[3], cr[3];
};

/* matrix / range -> yr, yg, yb, yoff, Cb r g b, Cr r g b */
__host__ __device__ inline void coef_rgb(uint32_t matrix, uint32_t full_range, int32_t k[10])
{
    const int32_t t[4][10] = {
        {16829, 33039, 6416, 1081344, -9714, -19070, 28784, 28784, -24103, -4681},      /* BT.601 limited */
        {19595, 38470, 7471, 32768, -11058, -21710, 32768, 32768, -27439, -5329},       /* BT.601 full    */
        {11966, 40254, 4064, 1081344, -6596, -22188, 28784, 28784, -26145, -2639},      /* BT.709 limited */
        {13933, 46871, 4732, 32768, -7509, -25259, 32768, 32768, -29763, -3005},        /* BT.709 full    */
    };
    const int row = (matrix == SCROLL_SURF_BT709 ? 2 : 0) + (full_range ? 1 : 0);
    for (int i = 0; i < 10; ++i) k[i] = t[row][i];
}

__host__ __device__ inline Coef coef(uint32_t format, uint32_t matrix, uint32_t full_range)
{
    int32_t k[10];
    coef_rgb(matrix, full_range, k);
    const int r = format == SCROLL_SURF_BGRA ? 2 : 0, b = 2 - r;
    Coef c;
    c.y[r] = k[0];
    c.y[1] = k[1];
    c.y[b] = k[2];
    c.yoff = k[3];
    c.cb[r] = k[4];
    c.cb[1] = k[5];
    c.cb[b] = k[6];
    c.cr[r] = k[7];
    c.cr[1] = k[8];
    c.cr[b] = k[9];
    return c;
}

/* one pixel's luma from its bytes 0..2 */
__host__ __device__ inline uint32_t luma(const Coef &c, uint32_t p0, uint32_t p1, uint32_t p2)
{
    return (uint32_t)(c.y[0] * (int32_t)p0 + c.y[1] * (int32_t)p1 + c.y[2] * (int32_t)p2 + c.yoff) >> 16;
}

/* one chroma sample from a 2x2 quad's sums of bytes 0..2; k = Coef.cb or .cr */
__host__ __device__ inline uint32_t chroma(const int32_t k[3], uint32_t s0, uint32_t s1, uint32_t s2)
{
    /* clamp, then shift: the same value as clamp(v >> 18, 0, 255), the floor
     * shift being monotone.  (In the other order hipcc pairs two results with
     * v_ashr_pk_u8_i32 and ORs the next ones onto its destination as if its
     * upper half were zero; on gfx950 it came back with stale bits in it.) */
    int32_t v = k[0] * (int32_t)s0 + k[1] * (int32_t)s1 + k[2] * (int32_t)s2 + (128 << 18) + (1 << 17);
    v = v < 0 ? 0 : v > (256 << 18) - 1 ? (256 << 18) - 1 : v;
    return (uint32_t)v >> 18;
}

/* a pixel as the surface holds it: a little-endian 32-bit word, byte 0 lowest */
__host__ __device__ inline uint32_t luma_px(const Coef &c, uint32_t px)
{
    return luma(c, px & 255u, (px >> 8) & 255u, (px >> 16) & 255u);
}

/* the quad's sums of bytes 0 and 2 (low / high half) and of byte 1 (low half):
 * four values of at most 255 never carry out of 16 bits */
__host__ __device__ inline void quad_sums(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t *s02, uint32_t *s1)
{
    *s02 = (a & 0x00FF00FFu) + (b & 0x00FF00FFu) + (c & 0x00FF00FFu) + (d & 0x00FF00FFu);
    *s1 = ((a >> 8) & 255u) + ((b >> 8) & 255u) + ((c >> 8) & 255u) + ((d >> 8) & 255u);
}

__host__ __device__ inline uint32_t chroma_quad(const int32_t k[3], uint32_t s02, uint32_t s1)
{
    return chroma(k, s02 & 0xFFFFu, s1, s02 >> 16);
}

/* n / d and the remainder for the flat task index, d >= 1, by a multiply
 * with m = magic(d) and one correction (the estimate is q or q - 1) */
__host__ __device__ inline uint32_t magic(uint32_t d)
{
    return d <= 1u ? 0xFFFFFFFFu : (uint32_t)(((uint64_t)1 << 32) / d);
}

__host__ __device__ inline uint32_t divmod(uint32_t n, uint32_t d, uint32_t m, uint32_t *rem)
{
    uint32_t q = (uint32_t)(((uint64_t)n * m) >> 32);
    uint32_t r = n - q * d;
    if (r >= d) {
        ++q;
        r -= d;
    }
    *rem = r;
    return q;
}

}  // namespace csc
}  // namespace scroll

#endif
