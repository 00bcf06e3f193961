/*
 * csc_kernels.hip -- MI355X (gfx950) kernel of the surface entry (DESIGN.md
 * §3l): windows of pitched 8-bit RGBA / BGRA surfaces to planar I420, by the
 * rule of csc_device.h.
 *
 * The kernel moves bytes: 4 per pixel in, 1.5 out, a few integer operations
 * each.  A lane converts a patch of 8 x 2 pixels: four 16-byte loads issued
 * together (the window is MB-aligned in a 16-byte-aligned surface, so every
 * one is a full vector load), two 8-byte luma stores and one 4-byte store
 * each of Cb and Cr.  (stream, frame, row pair, column group) flatten into
 * one task index, so consecutive lanes take consecutive patches along a row
 * and on into the next row pair and item: waves stay full at any rect width,
 * and a wave's loads cover runs of 32 bytes per lane.  Coefficients and
 * geometry are kernel arguments (SGPRs); every offset is 64-bit.  No LDS.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "csc_device.h"
#include "csc_engine.h"

using namespace scroll::csc;

namespace {

constexpr uint32_t CSC_T = 256;
constexpr uint32_t CSC_MAX_BLOCKS = 256u * 8u;      /* 8 workgroups of 4 waves per CU; the rest by grid stride */

struct CscArgs {
    CscJob j;
    uint32_t cw;            /* column groups per row: w / 8 */
    uint32_t tpi;           /* tasks per item: (h / 2) cw */
    uint32_t total;         /* S nframes tpi */
    uint32_t m_cw, m_tpi, m_nf;     /* magic() of the three divisors */
};

__device__ inline uint32_t luma4(const Coef &k, const uint4 &p)
{
    return luma_px(k, p.x) | (luma_px(k, p.y) << 8) | (luma_px(k, p.z) << 16) | (luma_px(k, p.w) << 24);
}

/* the two chroma samples of four pixel columns: top row t, bottom row b */
__device__ inline void chroma2(const Coef &k, const uint4 &t, const uint4 &b, int sh, uint32_t *cb, uint32_t *cr)
{
    uint32_t s02, s1;
    quad_sums(t.x, t.y, b.x, b.y, &s02, &s1);
    *cb |= chroma_quad(k.cb, s02, s1) << sh;
    *cr |= chroma_quad(k.cr, s02, s1) << sh;
    quad_sums(t.z, t.w, b.z, b.w, &s02, &s1);
    *cb |= chroma_quad(k.cb, s02, s1) << (sh + 8);
    *cr |= chroma_quad(k.cr, s02, s1) << (sh + 8);
}

__global__ __launch_bounds__(CSC_T) void k_csc(CscArgs a)
{
    const CscJob &j = a.j;
    const uint32_t stride = gridDim.x * CSC_T;
    for (uint32_t t = blockIdx.x * CSC_T + threadIdx.x; t < a.total; t += stride) {
        uint32_t r, cg, f;
        const uint32_t item = divmod(t, a.tpi, a.m_tpi, &r);
        const uint32_t rp = divmod(r, a.cw, a.m_cw, &cg);
        const uint32_t s = divmod(item, j.nframes, a.m_nf, &f);
        int32_t x0 = j.x0, y0 = j.y0;
        uint32_t w = j.w, h = j.h;      /* the item's own window */
        if (j.dpos) {
            const uint32_t e = j.dpos[(uint64_t)s * j.dpos_ld + f];
            const uint32_t pm = j.pos_mask ? j.pos_mask : 0xFFFFu, lo = e & 0xFFFFu, hi = e >> 16;
            x0 = e == 0xFFFFFFFFu ? -1 : (int32_t)(lo & pm);
            y0 = (int32_t)(hi & pm);
            w -= 16u * ((lo & ~pm) >> 8);
            h -= 16u * ((hi & ~pm) >> 8);
        } else if (j.pos) {
            /* (x, y) in one 8-byte load */
            const uint64_t p = reinterpret_cast<const uint64_t *>(j.pos)[(uint64_t)s * j.nframes + f];
            x0 = (int32_t)(uint32_t)p;
            y0 = (int32_t)(uint32_t)(p >> 32);
        }
        if (x0 < 0) continue;           /* no rect in this frame: its block stays */
        if (2u * rp >= h || 8u * cg >= w) continue;     /* past a sized frame's own window */
        const uint64_t plane = (uint64_t)w * h;
        if (j.cropped) x0 = y0 = 0;
        const uint8_t *sp = j.src + (uint64_t)s * j.src_ld + (uint64_t)f * j.src_fr +
                            ((uint64_t)(16u * (uint32_t)y0) + 2u * rp) * j.pitch +
                            ((uint64_t)(16u * (uint32_t)x0) + 8u * cg) * 4u;
        const uint4 t0 = *reinterpret_cast<const uint4 *>(sp);
        const uint4 t1 = *reinterpret_cast<const uint4 *>(sp + 16);
        const uint4 b0 = *reinterpret_cast<const uint4 *>(sp + j.pitch);
        const uint4 b1 = *reinterpret_cast<const uint4 *>(sp + j.pitch + 16);

        uint8_t *dp = j.dst + (uint64_t)s * j.dst_ld + (uint64_t)f * j.dst_fr;
        uint8_t *yp = dp + (uint64_t)(2u * rp) * w + 8u * cg;
        *reinterpret_cast<uint2 *>(yp) = make_uint2(luma4(j.k, t0), luma4(j.k, t1));
        *reinterpret_cast<uint2 *>(yp + w) = make_uint2(luma4(j.k, b0), luma4(j.k, b1));

        uint32_t cb = 0, cr = 0;
        chroma2(j.k, t0, b0, 0, &cb, &cr);
        chroma2(j.k, t1, b1, 16, &cb, &cr);
        uint8_t *cp = dp + plane + (uint64_t)rp * (w >> 1) + 4u * cg;
        *reinterpret_cast<uint32_t *>(cp) = cb;
        *reinterpret_cast<uint32_t *>(cp + (plane >> 2)) = cr;
    }
}

}  // namespace

int csc_launch(hipStream_t hs, const CscJob *job)
{
    if (job->S == 0 || job->nframes == 0 || job->w == 0 || job->h == 0) return 0;
    if (csc_tasks(job) > CSC_MAX_TASKS) return -1;
    CscArgs a{};
    a.j = *job;
    a.cw = job->w / 8u;
    a.tpi = (job->h / 2u) * a.cw;
    a.total = job->S * job->nframes * a.tpi;
    a.m_cw = magic(a.cw);
    a.m_tpi = magic(a.tpi);
    a.m_nf = magic(job->nframes);
    const uint32_t blocks = std::min<uint32_t>((a.total + CSC_T - 1u) / CSC_T, CSC_MAX_BLOCKS);
    hipLaunchKernelGGL(k_csc, dim3(blocks), dim3(CSC_T), 0, hs, a);
    return hipGetLastError() != hipSuccess ? -1 : 0;
}
