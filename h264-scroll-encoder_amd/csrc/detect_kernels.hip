/*
 * detect_kernels.hip -- MI355X (gfx950) kernels of scroll_batch_detect_offsets
 * (DESIGN.md §3q): each frame's scroll offset found from the renderer's
 * surfaces and the stacked reference pictures, by the rule of detect_device.h.
 *
 *   k_det_surf   the hot kernel, bandwidth-bound by construction: it reads
 *                every byte of the used segments once.  k_dyn_damage's shape:
 *                a wave takes a span of four used segments x 16 pixel rows; a
 *                lane takes 4 pixels of each row, one 16-byte load, all 16
 *                rows' loads issued before the first use, so a segment's 16
 *                lanes read one contiguous 256-byte run per row and with
 *                seg_step > 1 nothing between the used runs is touched.  The
 *                16 lanes of a segment are one DPP row: two quad permutes, a
 *                half-row mirror and a row mirror leave the segment's sum in
 *                every lane, no LDS; two rows' sums (at most 16,320 each)
 *                ride in one register, so 16 rows cost 32 cross-lane adds.
 *                Lane q of a segment then stores row q's signature: per row
 *                the wave's four uint16 are contiguous.  (stream, frame, row
 *                block, span) flatten into one wave-uniform task index walked
 *                by grid stride; a partial last segment and a partial last
 *                span mask their lanes.  Every surface and signature offset is
 *                64-bit.  No atomics.
 *   k_det_refs   the same reduction over the luma bytes of A and B: 2 ph rows
 *                per stream (once with a shared pair), a dword per lane and
 *                row, stored segment-major ([segment][row]) for k_det_score.
 *   k_det_score  a workgroup takes 256 consecutive candidates of one frame's
 *                window, a lane per candidate, and walks the picture in tiles
 *                of 128 rows x 16 used segments: the tile's sigS goes to LDS
 *                row-major (read at a wave-uniform address: a broadcast), the
 *                384 rows of sigR that the 256 candidates reach to LDS
 *                segment-major, so consecutive lanes read consecutive uint16
 *                of one segment's column -- two lanes a dword, 32 consecutive
 *                banks per wave, conflict-free by the bank rule.  16 KB of LDS
 *                whatever the picture: nothing assumes a frame's signatures
 *                fit.  The count stays in a register; one plain store per
 *                candidate.
 *   k_det_pick   one workgroup per frame: the window's scores to the two
 *                largest keys (a uint64 maximum and runner-up, merged by a
 *                tree in LDS), the record, 0xFFFFFFFF over the scores outside
 *                the window and, on request, the frame's offset: plain
 *                stores, no hand-off between workgroups.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "detect_device.h"
#include "detect_engine.h"

using namespace scroll;
using namespace scroll::csc;
using namespace scroll::detect;

namespace {

constexpr uint32_t SIG_T = 256;
constexpr uint32_t SIG_WAVES = SIG_T / 64u;
constexpr uint32_t SIG_MAX_BLOCKS = 256u * 8u;      /* 8 workgroups of 4 waves per CU; the rest by grid stride */
constexpr uint32_t SCORE_T = 256;                   /* candidates per workgroup */
constexpr uint32_t TILE_Y = 128;                    /* picture rows per tile */
constexpr uint32_t TILE_C = 16;                     /* used segments per tile */
constexpr uint32_t TILE_R = TILE_Y + SCORE_T;       /* rows of sigR a tile's candidates reach (TILE_Y + SCORE_T - 1), even */
constexpr uint32_t PICK_T = 256;

struct SigArgs {
    DetJob j;
    uint32_t nsp;           /* spans per row block: ceil(nuse / 4) */
    uint32_t nrb;           /* row blocks of 16 per item: ph / 16 (surfaces), 2 ph / 16 (references) */
    uint32_t nit;           /* items per stream: nframes (surfaces), 1 (references) */
    uint32_t total;
    uint32_t m_nsp, m_nrb, m_nit;   /* magic() of the three divisors */
};

template <int CTRL>
__device__ inline uint32_t dpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}

/* the sums of the 16 lanes of each DPP row, in every lane of it: quad_perm
 * [1,0,3,2] and [2,3,0,1], row_half_mirror, row_mirror */
__device__ inline uint32_t row_sum(uint32_t v)
{
    v += dpp<0xB1>(v);
    v += dpp<0x4E>(v);
    v += dpp<0x141>(v);
    v += dpp<0x140>(v);
    return v;
}

/* acc[r]: the lane's share of row r.  Two rows per register through the
 * reduction; the signature of row q comes back */
__device__ inline uint32_t rows_reduce(const uint32_t acc[16], uint32_t q)
{
    uint32_t v = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t two = row_sum(acc[2 * i] | acc[2 * i + 1] << 16);
        v = (q >> 1) == (uint32_t)i ? two : v;
    }
    return (q & 1u) ? v >> 16 : v & 0xFFFFu;
}

__global__ __launch_bounds__(SIG_T) void k_det_surf(SigArgs a)
{
    const DetJob &j = a.j;
    const uint32_t lane = threadIdx.x & 63u, g = lane >> 4, q = lane & 15u;
    const uint32_t nwaves = gridDim.x * SIG_WAVES;
    /* the task is the wave's: uniform, so its state lives in SGPRs */
    for (uint32_t t = __builtin_amdgcn_readfirstlane(blockIdx.x * SIG_WAVES + (threadIdx.x >> 6)); t < a.total;
         t += nwaves) {
        uint32_t sp, rb, f;
        const uint32_t row = divmod(t, a.nsp, a.m_nsp, &sp);
        const uint32_t item = divmod(row, a.nrb, a.m_nrb, &rb);
        const uint32_t s = divmod(item, a.nit, a.m_nit, &f);
        const uint64_t nb = (uint64_t)s * j.ld_fr + f;
        const uint32_t cu = 4u * sp + g;                /* the used segment, segment cu seg_step of the picture */
        const uint32_t x = cu * j.rule.seg_step * SEG + 4u * q;
        const bool seg = cu < j.nuse;                   /* a partial last span */
        const bool on = seg && x < j.pw;                /* a partial last segment */
        uint32_t acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0u;
        if (on) {
            const uint8_t *sp0 = j.src + (uint64_t)s * j.src_ld + (uint64_t)f * j.src_fr +
                                 (uint64_t)(16u * rb) * j.pitch + (uint64_t)x * 4u;
            uint4 px[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) px[r] = *reinterpret_cast<const uint4 *>(sp0 + (uint64_t)r * j.pitch);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = sig4(j.k, px[r].x, px[r].y, px[r].z, px[r].w);
        }
        const uint32_t v = rows_reduce(acc, q);
        if (seg) j.sig_s[(nb * j.ph + 16u * rb + q) * j.nuse + cu] = (uint16_t)v;
    }
}

__global__ __launch_bounds__(SIG_T) void k_det_refs(SigArgs a)
{
    const DetJob &j = a.j;
    const uint32_t lane = threadIdx.x & 63u, g = lane >> 4, q = lane & 15u;
    const uint32_t nwaves = gridDim.x * SIG_WAVES;
    for (uint32_t t = __builtin_amdgcn_readfirstlane(blockIdx.x * SIG_WAVES + (threadIdx.x >> 6)); t < a.total;
         t += nwaves) {
        uint32_t sp, rb;
        const uint32_t s = divmod(divmod(t, a.nsp, a.m_nsp, &sp), a.nrb, a.m_nrb, &rb);
        const uint32_t cu = 4u * sp + g;
        const uint32_t x = cu * j.rule.seg_step * SEG + 4u * q;
        const bool seg = cu < j.nuse;
        const bool on = seg && x < j.pw;
        /* 16 rows of the stack never straddle A and B: ph is a multiple of 16 */
        const uint32_t r0 = 16u * rb;
        uint32_t acc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0u;
        if (on) {
            const uint8_t *rp0 = j.refs + (uint64_t)s * j.ref_ld +
                                 (r0 < j.ph ? (uint64_t)r0 * j.pw : j.pic + (uint64_t)(r0 - j.ph) * j.pw) + x;
            uint32_t rf[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) rf[r] = *reinterpret_cast<const uint32_t *>(rp0 + (uint64_t)r * j.pw);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = ref4(rf[r]);
        }
        const uint32_t v = rows_reduce(acc, q);
        if (seg) j.sig_r[((uint64_t)s * j.nuse + cu) * (2u * j.ph) + r0 + q] = (uint16_t)v;
    }
}

__device__ inline uint32_t eq16(uint32_t a, uint32_t b) { return a == b ? 1u : 0u; }

__global__ __launch_bounds__(SCORE_T) void k_det_score(DetJob j)
{
    __shared__ __attribute__((aligned(16))) uint16_t sR[TILE_C][TILE_R];
    __shared__ __attribute__((aligned(16))) uint16_t sS[TILE_Y][TILE_C];
    const uint32_t s = blockIdx.z, f = blockIdx.y, t = threadIdx.x;
    const uint64_t nb = (uint64_t)s * j.ld_fr + f;
    const Window w = window(j.off[nb], j.rule.radius, j.ph);
    const uint32_t o0 = (uint32_t)w.lo + SCORE_T * blockIdx.x;
    if (o0 > (uint32_t)w.hi) return;                    /* the workgroup's: a window clipped at 0 or ph is shorter */
    const uint32_t o = o0 + t;
    const bool active = o <= (uint32_t)w.hi;
    const uint32_t nu = j.nuse, ph2 = 2u * j.ph;
    const uint16_t *gr = j.sig_r + (j.ref_ld ? (uint64_t)s * nu * ph2 : 0u);
    const uint16_t *gs = j.sig_s + nb * j.ph * nu;
    uint32_t cnt = 0u;
    for (uint32_t y0 = 0; y0 < j.ph; y0 += TILE_Y) {
        const uint32_t ty = min(TILE_Y, j.ph - y0);
        for (uint32_t c0 = 0; c0 < nu; c0 += TILE_C) {
            const uint32_t ncc = min(TILE_C, nu - c0), ncc4 = (ncc + 3u) & ~3u;
            __syncthreads();                            /* the last tile has been read */
            /* rows y0 + o0 .. + ty + 254 of the stack; what no active candidate reads gets a value no signature has */
            for (uint32_t i = t; i < ncc4 * TILE_R; i += SCORE_T) {
                const uint32_t cc = i / TILE_R, k = i % TILE_R, r = y0 + o0 + k;
                sR[cc][k] = cc < ncc && r < ph2 ? gr[(uint64_t)(c0 + cc) * ph2 + r] : (uint16_t)0xFFFFu;
            }
            for (uint32_t i = t; i < ty * TILE_C; i += SCORE_T) {
                const uint32_t y = i / TILE_C, cc = i % TILE_C;
                sS[y][cc] = cc < ncc ? gs[(uint64_t)(y0 + y) * nu + c0 + cc] : (uint16_t)0xFFFEu;
            }
            __syncthreads();
            if (active) {
                for (uint32_t y = 0; y < ty; ++y) {
                    for (uint32_t cc = 0; cc < ncc4; cc += 4u) {
                        const uint2 v = *reinterpret_cast<const uint2 *>(&sS[y][cc]);
                        cnt += eq16(v.x & 0xFFFFu, sR[cc][y + t]) + eq16(v.x >> 16, sR[cc + 1u][y + t]) +
                               eq16(v.y & 0xFFFFu, sR[cc + 2u][y + t]) + eq16(v.y >> 16, sR[cc + 3u][y + t]);
                    }
                }
            }
        }
    }
    if (active) j.scores[nb * (j.ph + 1u) + o] = cnt;
}

__global__ __launch_bounds__(PICK_T) void k_det_pick(DetJob j)
{
    __shared__ Top2 part[PICK_T];
    const uint32_t s = blockIdx.y, f = blockIdx.x, t = threadIdx.x;
    const uint64_t nb = (uint64_t)s * j.ld_fr + f;
    const Window w = window(j.off[nb], j.rule.radius, j.ph);
    uint32_t *sc = j.scores + nb * (j.ph + 1u);
    Top2 a = top2_init();
    for (uint32_t o = t; o <= j.ph; o += PICK_T) {
        if ((int32_t)o < w.lo || (int32_t)o > w.hi)
            sc[o] = NO_SCORE;
        else
            top2_add(a, key(sc[o], (int32_t)o, w.c0));
    }
    part[t] = a;
    for (uint32_t n = PICK_T / 2; n > 0; n >>= 1) {
        __syncthreads();
        if (t < n) top2_merge(part[t], part[t + n]);
    }
    if (t == 0) {
        const ScrollOffsetFound r = found(part[0], w, j.ph * j.nuse, j.rule.min_match);
        j.res[nb] = r;
        if (j.rule.apply && r.status == SCROLL_DET_FOUND) j.off[nb] = r.off;
    }
}

int sig_launch(void (*kern)(SigArgs), hipStream_t hs, const DetJob *job, uint32_t nstreams, uint32_t nit, uint32_t nrb)
{
    SigArgs a{};
    a.j = *job;
    a.nsp = (job->nuse + 3u) / 4u;
    a.nrb = nrb;
    a.nit = nit;
    const uint64_t total = (uint64_t)nstreams * nit * nrb * a.nsp;
    if (total == 0) return 0;
    if (total >= ((uint64_t)1 << 31)) return -1;
    a.total = (uint32_t)total;
    a.m_nsp = magic(a.nsp);
    a.m_nrb = magic(a.nrb);
    a.m_nit = magic(a.nit);
    const uint32_t blocks = std::min<uint32_t>((a.total + SIG_WAVES - 1u) / SIG_WAVES, SIG_MAX_BLOCKS);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(SIG_T), 0, hs, a);
    return hipGetLastError() != hipSuccess ? -1 : 0;
}

}  // namespace

int det_launch_refs(hipStream_t hs, const DetJob *job)
{
    return sig_launch(k_det_refs, hs, job, job->ref_ld ? job->S : 1u, 1u, 2u * job->ph / 16u);
}

int det_launch_surf(hipStream_t hs, const DetJob *job)
{
    return sig_launch(k_det_surf, hs, job, job->S, job->nframes, job->ph / 16u);
}

int det_launch_score(hipStream_t hs, const DetJob *job)
{
    if (job->S == 0 || job->nframes == 0) return 0;
    /* the longest window: 2 radius + 1 candidates, at most ph + 1 */
    const uint32_t r = std::min(job->rule.radius, job->ph);
    const uint32_t ncand = std::min(2u * r + 1u, job->ph + 1u);
    hipLaunchKernelGGL(k_det_score, dim3((ncand + SCORE_T - 1u) / SCORE_T, job->nframes, job->S), dim3(SCORE_T), 0, hs,
                       *job);
    return hipGetLastError() != hipSuccess ? -1 : 0;
}

int det_launch_pick(hipStream_t hs, const DetJob *job)
{
    if (job->S == 0 || job->nframes == 0) return 0;
    hipLaunchKernelGGL(k_det_pick, dim3(job->nframes, job->S), dim3(PICK_T), 0, hs, *job);
    return hipGetLastError() != hipSuccess ? -1 : 0;
}
