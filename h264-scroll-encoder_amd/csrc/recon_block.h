/*
 * recon_block.h -- per-lane block helpers of the reconstruction kernels
 * (k_dyn_recon, recon_kernels.hip; k_hdyn_recon, hrecon_kernels.hip): a 4x4
 * block's source and prediction as four packed rows each, from them the
 * coder's coefficients, and prediction + residual clipped, stored and
 * compared with the source.  Device only.
 */
#ifndef SCROLL_RECON_BLOCK_H
#define SCROLL_RECON_BLOCK_H

#include <hip/hip_runtime.h>

#include "recon_device.h"

namespace scroll {
namespace recon {

__device__ inline uint32_t ld32(const uint8_t *p) { return *reinterpret_cast<const uint32_t *>(p); }
__device__ inline void st32(uint8_t *p, uint32_t v) { *reinterpret_cast<uint32_t *>(p) = v; }

__device__ inline void unpack4(uint32_t v, int *o)
{
    o[0] = (int)(v & 255u);
    o[1] = (int)((v >> 8) & 255u);
    o[2] = (int)((v >> 16) & 255u);
    o[3] = (int)(v >> 24);
}
__device__ inline uint32_t pack4(const int *o)
{
    return (uint32_t)o[0] | (uint32_t)o[1] << 8 | (uint32_t)o[2] << 16 | (uint32_t)o[3] << 24;
}

/* A block's source and prediction stay packed (4 + 4 registers) while its
 * coefficients go through quant / dequant / inverse: they are unpacked for
 * the residual, and again for add + clip + squared error.  (Kept as 32
 * unpacked registers across the transforms the kernel took 116 VGPRs.) */
__device__ inline void block_fwd(const uint32_t sv[4], const uint32_t pv[4], int W[16])
{
    int sp[16], pr[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unpack4(sv[i], sp + 4 * i);
        unpack4(pv[i], pr + 4 * i);
    }
    residual_fwd(sp, pr, W);
}

/* prediction + res, clipped -> 4 rows at dst (stride bytes apart); returns
 * the squared error against the source */
__device__ inline uint32_t block_store(uint32_t sv[4], uint32_t pv[4], int res[16], uint8_t *dst, int stride)
{
    /* the packed words as new values once the residual exists, so that the
     * bytes unpacked for block_fwd are not kept live until here */
    asm volatile("" : "+v"(sv[0]), "+v"(sv[1]), "+v"(sv[2]), "+v"(sv[3]), "+v"(pv[0]), "+v"(pv[1]), "+v"(pv[2]),
                 "+v"(pv[3]), "+v"(res[0]));
    /* sum (s - o)^2 = sum s^2 + sum o^2 - 2 sum s o on the packed bytes: three
     * 4-byte dot products per row, the source never unpacked again */
    uint32_t sq = 0, cross = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int pr[4], out[4];
        unpack4(pv[i], pr);
#pragma unroll
        for (int x = 0; x < 4; ++x) out[x] = add_clip(pr[x], res[4 * i + x]);
        const uint32_t ov = pack4(out);
        sq = __builtin_amdgcn_udot4(sv[i], sv[i], sq, false);
        sq = __builtin_amdgcn_udot4(ov, ov, sq, false);
        cross = __builtin_amdgcn_udot4(sv[i], ov, cross, false);
        st32(dst + (size_t)i * stride, ov);
    }
    return sq - 2u * cross;
}

__device__ inline uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

}  // namespace recon
}  // namespace scroll

#endif
