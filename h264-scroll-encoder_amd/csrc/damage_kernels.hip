/*
 * damage_kernels.hip -- MI355X (gfx950) kernels of scroll_batch_dyn_locate
 * (DESIGN.md §3n): the per-MB damage map between the renderer's surfaces and
 * the luma a decoder shows for a scroll MB without residual, and the rect's
 * placement over the damaged MBs, by the rule of damage_device.h.
 *
 *   k_dmg_rows    per (stream, frame): the byte offset, in the stream's
 *                 reference pair, of the prediction row of every luma row of
 *                 the picture (the luma branch of k_dyn_rows over the whole
 *                 picture).  A kernel of its own and not the head of
 *                 k_dyn_damage: a frame's rows are shared by all its spans,
 *                 and resolving them is a chain of dependent loads (plan,
 *                 waypoint table, regions) that would sit in front of every
 *                 wave's surface loads; the table is 4 bytes per picture row
 *                 against 4 x width bytes of surface.
 *   k_dyn_damage  the hot kernel, bandwidth-bound by construction: it reads
 *                 every surface byte once.  A wave takes a span of 16 MBs x
 *                 16 pixel rows; a lane takes 4 pixels of each row: one
 *                 16-byte surface load and one dword of the reference row,
 *                 all 16 rows' loads issued before the first use, so a wave's
 *                 load of a row covers 1,024 contiguous surface bytes and
 *                 256 of the reference.  The four lanes of an MB are one DPP
 *                 quad: two cross-lane adds, then one lane per MB stores the
 *                 uint32 -- 16 lanes a 64-byte run.  (stream, frame, MB row,
 *                 span) flatten into one wave-uniform task index walked by
 *                 grid stride; a partial last span masks its lanes.  Geometry
 *                 and coefficients are kernel arguments (SGPRs), every
 *                 surface and map offset is 64-bit.  No LDS, no atomics.
 *   k_dyn_place   one workgroup per frame reduces its map to the
 *                 ScrollDynDamage record and, on request, the position
 *                 table's entry: plain stores, no hand-off between workgroups.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "damage_device.h"
#include "damage_engine.h"
#include "nal_ctx.h"

using namespace scroll;
using namespace scroll::csc;
using namespace scroll::damage;

namespace {

constexpr uint32_t DMG_T = 256;
constexpr uint32_t DMG_WAVES = DMG_T / 64u;
constexpr uint32_t DMG_MAX_BLOCKS = 256u * 8u;      /* 8 workgroups of 4 waves per CU; the rest by grid stride */
constexpr uint32_t PLACE_T = 256;

__global__ __launch_bounds__(256) void k_dmg_rows(const DevStream *__restrict__ st, const NalDesc *__restrict__ nal,
                                                  int ld_nal, const PlanPending *__restrict__ pend,
                                                  const DynFrame *__restrict__ dfr, int ld_fr, int ph,
                                                  uint32_t *__restrict__ rows)
{
    __shared__ int32_t wo[8], wl[8], wv[8];
    const int s = blockIdx.y, f = blockIdx.x, t = threadIdx.x;
    const size_t nb = (size_t)s * ld_fr + f;
    const int j = dfr[nb].nal;
    if (j < 0) return;                                  /* no scroll NAL: k_dyn_damage reads no row of it */
    if (t < 8) {
        wo[t] = pend[s].wo[t];
        wl[t] = pend[s].wl[t];
        wv[t] = pend[s].wv[t];
    }
    __syncthreads();
    const DevStream *S = st + s;
    const NalDesc d = nal[(size_t)s * ld_nal + j];
    const NalCtx c = nal_ctx(S, d, wo, wl, wv);
    const Regions rg = regions(c);
    const int w = c.w, h = c.h, a_end = (h - c.off) / 16;
    const uint32_t ysz = (uint32_t)w * (uint32_t)h, pic = ysz + ysz / 2;
    const dyn::WpTab T{wo, wv, h};
    uint32_t *rw = rows + nb * (size_t)ph;
    for (int Y = t; Y < ph; Y += 256) {
        int yo;
        const int b = pred_row(T, rg, a_end, Y, yo);
        rw[Y] = (uint32_t)b * pic + (uint32_t)yo * (uint32_t)w;
    }
}

struct DmgArgs {
    DmgJob j;
    uint32_t nsp;           /* spans per MB row: ceil(mbw / 16) */
    uint32_t total;         /* S nframes mbh nsp */
    uint32_t m_nsp, m_mbh, m_nf;    /* magic() of the three divisors */
};

template <int CTRL>
__device__ inline uint32_t quad(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}

__global__ __launch_bounds__(DMG_T) void k_dyn_damage(DmgArgs a)
{
    const DmgJob &j = a.j;
    const uint32_t lane = threadIdx.x & 63u, mbl = lane >> 2, q = lane & 3u;
    const uint32_t nwaves = gridDim.x * DMG_WAVES;
    /* the task is the wave's: uniform, so its state lives in SGPRs */
    for (uint32_t t = __builtin_amdgcn_readfirstlane(blockIdx.x * DMG_WAVES + (threadIdx.x >> 6)); t < a.total;
         t += nwaves) {
        uint32_t sp, my, f;
        const uint32_t row = divmod(t, a.nsp, a.m_nsp, &sp);
        const uint32_t item = divmod(row, j.mbh, a.m_mbh, &my);
        const uint32_t s = divmod(item, j.nframes, a.m_nf, &f);
        const uint64_t nb = (uint64_t)s * j.ld_fr + f;
        const uint32_t mx = 16u * sp + mbl;
        const bool on = mx < j.mbw;                     /* a partial last span */
        uint32_t *mp = j.map + (nb * j.mbh + my) * j.mbw + mx;
        if (j.dfr[nb].nal < 0) {                        /* no scroll NAL: zero entries */
            if (on && q == 0u) *mp = 0u;
            continue;
        }
        uint32_t acc = 0u;
        if (on) {
            const uint32_t *rw = j.rows + (nb * j.mbh + my) * 16u;
            const uint8_t *sp0 = j.src + (uint64_t)s * j.src_ld + (uint64_t)f * j.src_fr +
                                 (uint64_t)(16u * my) * j.pitch + (uint64_t)(16u * mx + 4u * q) * 4u;
            const uint8_t *rp0 = j.refs + (uint64_t)s * j.ref_ld + (16u * mx + 4u * q);
            uint4 px[16];
            uint32_t rf[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                px[r] = *reinterpret_cast<const uint4 *>(sp0 + (uint64_t)r * j.pitch);
                rf[r] = *reinterpret_cast<const uint32_t *>(rp0 + rw[r]);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc = sq4(j.k, px[r].x, px[r].y, px[r].z, px[r].w, rf[r], acc);
        }
        /* the MB's four lanes: quad_perm [1,0,3,2], then [2,3,0,1] */
        acc += quad<0xB1>(acc);
        acc += quad<0x4E>(acc);
        if (on && q == 0u) *mp = acc;
    }
}

/* 256 values in LDS -> v[0], by op */
template <class V, class Op>
__device__ inline void reduce256(V *v, int t, Op op)
{
    for (int n = PLACE_T / 2; n > 0; n >>= 1) {
        __syncthreads();
        if (t < n) op(v[t], v[t + n]);
    }
    __syncthreads();
}

__global__ __launch_bounds__(PLACE_T) void k_dyn_place(const DynFrame *__restrict__ dfr, int ld_fr,
                                                       const uint32_t *__restrict__ map, uint32_t mbw, uint32_t mbh,
                                                       uint32_t w, uint32_t h, ScrollDynLocate rule,
                                                       ScrollDynDamage *__restrict__ res, uint32_t *__restrict__ dpos)
{
    __shared__ Acc part[PLACE_T];
    __shared__ uint64_t in[PLACE_T];
    __shared__ ScrollDynDamage rec;
    const int s = blockIdx.y, f = blockIdx.x, t = threadIdx.x;
    const size_t nb = (size_t)s * ld_fr + f;
    if (dfr[nb].nal < 0) {
        if (t == 0) {
            res[nb] = noframe();
            if (dpos) dpos[nb] = DYN_POS_NONE;
        }
        return;
    }
    const uint32_t nmb = mbw * mbh;
    const uint32_t *m = map + nb * nmb;
    Acc a = acc_init();
    for (uint32_t i = t; i < nmb; i += PLACE_T) acc_add(a, m[i], i % mbw, i / mbw, rule.mb_sse);
    part[t] = a;
    reduce256(part, t, [](Acc &x, const Acc &y) { acc_merge(x, y); });
    if (t == 0) rec = place(part[0], w, h, mbw, mbh, rule.margin, rule.size);
    __syncthreads();
    ScrollDynDamage r = rec;
    uint64_t sum = 0;
    const uint32_t wf = placed_w(r, w, rule.size), hf = placed_h(r, h, rule.size);   /* the rect as placed (and sized) */
    if (r.x0 >= 0)
        for (uint32_t i = t; i < wf * hf; i += PLACE_T)
            sum += m[((uint32_t)r.y0 + i / wf) * mbw + (uint32_t)r.x0 + i % wf];
    in[t] = sum;
    reduce256(in, t, [](uint64_t &x, const uint64_t &y) { x += y; });
    if (t == 0) {
        finish(r, in[0]);
        res[nb] = r;
        if (dpos) dpos[nb] = rule.size ? pos_entry_sized(r, w, h) : pos_entry(r);
    }
}

}  // namespace

int dmg_launch_rows(hipStream_t hs, int nframes, int S, const DevStream *st, const NalDesc *nal, int ld_nal,
                    const PlanPending *pend, const DynFrame *dfr, int ld_fr, int ph, uint32_t *rows)
{
    if (nframes <= 0 || S <= 0) return 0;
    hipLaunchKernelGGL(k_dmg_rows, dim3(nframes, S), dim3(256), 0, hs, st, nal, ld_nal, pend, dfr, ld_fr, ph, rows);
    return hipGetLastError() != hipSuccess ? -1 : 0;
}

int dmg_launch_damage(hipStream_t hs, const DmgJob *job)
{
    if (job->S == 0 || job->nframes == 0 || job->mbw == 0 || job->mbh == 0) return 0;
    if (dmg_tasks(job) >= DMG_MAX_TASKS) return -1;
    DmgArgs a{};
    a.j = *job;
    a.nsp = (job->mbw + 15u) / 16u;
    a.total = (uint32_t)dmg_tasks(job);
    a.m_nsp = magic(a.nsp);
    a.m_mbh = magic(job->mbh);
    a.m_nf = magic(job->nframes);
    const uint32_t blocks = std::min<uint32_t>((a.total + DMG_WAVES - 1u) / DMG_WAVES, DMG_MAX_BLOCKS);
    hipLaunchKernelGGL(k_dyn_damage, dim3(blocks), dim3(DMG_T), 0, hs, a);
    return hipGetLastError() != hipSuccess ? -1 : 0;
}

int dmg_launch_place(hipStream_t hs, int nframes, int S, const DynFrame *dfr, int ld_fr, const uint32_t *map,
                     uint32_t mbw, uint32_t mbh, uint32_t w, uint32_t h, const ScrollDynLocate *rule,
                     ScrollDynDamage *res, uint32_t *dpos)
{
    if (nframes <= 0 || S <= 0) return 0;
    hipLaunchKernelGGL(k_dyn_place, dim3(nframes, S), dim3(PLACE_T), 0, hs, dfr, ld_fr, map, mbw, mbh, w, h, *rule, res,
                       dpos);
    return hipGetLastError() != hipSuccess ? -1 : 0;
}
