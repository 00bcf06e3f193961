/*
 * mask_kernels.hip -- MI355X (gfx950) kernels of scroll_batch_dyn_mask
 * (DESIGN.md §3o): the per-MB difference between the dynamic rect's source and
 * the prediction k_dyn_row subtracts from it, the keep decision by the rule of
 * mask_device.h, and the source of the MBs not kept overwritten by that
 * prediction.  The prediction is the coder's own: k_dyn_rows' prediction rows
 * read through RowPred<GEN> (recon_pred.h), as k_dyn_recon and k_dyn_probe
 * read them; rows behind a half-pel waypoint chain (chroma_pred_any, a chain
 * of calls with scratch) run in the kernels' second instantiation over the
 * frames k_dyn_rows listed, so that the common one stays free of calls.
 *
 *   k_dyn_mask_diff  the hot kernel, bandwidth-bound by construction: it reads
 *                    every source byte of the rect and as many reference
 *                    bytes once.  A wave takes a span of 16 MBs of one rect MB
 *                    row; the four lanes of an MB are one DPP quad.  Luma:
 *                    lane q takes the MB's block column q, 16 rows of 4 bytes,
 *                    so a wave's load of a row covers 256 contiguous bytes of
 *                    the source and of the reference.  Chroma: lane q takes
 *                    block column q & 1 of plane q >> 1, 8 rows: two runs of
 *                    128 bytes per load.  The source loads depend on nothing
 *                    but the lane's address and stand before the prediction's
 *                    in program order.  The row's 32 prediction-row entries are
 *                    the wave's (uniform loads, no LDS).  Two cross-lane adds,
 *                    then one lane per MB stores { Dy, Dc }: 16 lanes a
 *                    128-byte run.  One task per wave, no loop: every load
 *                    precedes the wave's only store.  Every source and map
 *                    offset is 64-bit.  No LDS, no atomics.
 *   k_dyn_mask_fill  one workgroup per rect MB row of a frame, its waves over
 *                    the row's spans in the same lane mapping: the keep
 *                    decision by dilation over the stored map (an MB's
 *                    neighbours split over its quad), then, for the MBs not
 *                    kept, the chroma planes' squared error apart (the map
 *                    holds their sum) and, with apply, the prediction stored
 *                    over the source: plain vector stores.  The row's Cb / Cr
 *                    sums go to a partial of its own.
 *   k_dyn_mask_rec   one workgroup per frame: the KEPT bits into the map, the
 *                    counts and the Y sum from it, the rows' partials summed:
 *                    the record, by plain stores.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "csc_device.h"         /* scroll::csc::magic, divmod */
#include "dyn_engine.h"
#include "dyn_pos.h"
#include "mask_device.h"
#include "mask_engine.h"
#include "nal_ctx.h"
#include "recon_pred.h"

using namespace scroll;
using namespace scroll::dyn;
using namespace scroll::recon;
using namespace scroll::mask;

namespace {

constexpr uint32_t MK_T = 256, MK_WAVES = MK_T / 64u;

struct MaskArgs {
    MaskJob j;
    uint32_t nsp;           /* spans per rect row: ceil(w / 16) */
    uint32_t total;         /* S nframes h nsp */
    uint32_t m_nsp, m_h, m_nf;      /* magic() of the three divisors */
};

template <int CTRL>
__device__ inline uint32_t quad(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}

/* the sum over an MB's four lanes: quad_perm [1,0,3,2], then [2,3,0,1] */
__device__ inline uint32_t quad_sum(uint32_t v)
{
    v += quad<0xB1>(v);
    v += quad<0x4E>(v);
    return v;
}

/* rect row r of frame nb: its 32 prediction-row entries (and, GEN, the
 * stream's waypoint table) into L, as k_dyn_recon fills its ReconLds; returns
 * whether some chroma row of it runs through a half-pel chain.  Everything
 * here is uniform over the wave. */
template <bool GEN>
__device__ inline bool row_table(const MaskJob &j, const DynGeom &g, size_t nb, int s, int r, ReconLds &L)
{
    const int h = g.h;                                  /* the frame's own; frames stride by the batch's */
    const uint32_t *rw = j.rows + nb * (size_t)(32 * g.ld_h);
#pragma unroll
    for (int i = 0; i < 16; ++i) L.rt[i] = rw[16 * r + i];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        L.rt[16 + i] = rw[16 * h + 8 * r + i];
        L.rt[24 + i] = rw[24 * h + 8 * r + i];
    }
    if (GEN) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            L.wo[i] = j.pend[s].wo[i];
            L.wv[i] = j.pend[s].wv[i];
        }
    }
    bool gen = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t ea = L.rt[16 + i], eb = L.rt[24 + i];
        gen |= (ea & ROW_GEN) || (((ea >> 28) & 7u) && (eb & ROW_GEN));
    }
    return gen;
}

/* a lane's share of MB mx of rect row r: packed source and prediction rows */
struct MbPix {
    uint32_t sy[16], py[16];        /* luma block column q: 16 rows */
    uint32_t sc[8], pc[8];          /* block column q & 1 of chroma plane q >> 1: 8 rows */
};

struct MbAt {
    uint8_t *ly, *lc;               /* the lane's first luma / chroma word in the frame's source */
    size_t lstride, cstride;
    int bxl, bxc, p;
};

__device__ inline MbAt mb_at(uint8_t *fs, const DynGeom &g, int r, uint32_t mx, uint32_t q)
{
    MbAt a;
    const size_t ndt = (size_t)g.w * (size_t)g.h;
    a.lstride = (size_t)16 * g.w;
    a.cstride = (size_t)8 * g.w;
    a.bxl = (int)(4u * mx + q);
    a.p = (int)(q >> 1);
    a.bxc = (int)(2u * mx + (q & 1u));
    a.ly = fs + (size_t)(16 * r) * a.lstride + (size_t)4 * a.bxl;
    a.lc = fs + (size_t)256 * ndt + (size_t)a.p * 64 * ndt + (size_t)(8 * r) * a.cstride + (size_t)4 * a.bxc;
    return a;
}

template <bool GEN, bool LUMA_SRC>
__device__ inline void mb_load(const RowPred<GEN> &P, const MbAt &a, MbPix &x)
{
    if (LUMA_SRC) {
#pragma unroll
        for (int i = 0; i < 16; ++i) x.sy[i] = ld32(a.ly + (size_t)i * a.lstride);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) x.sc[i] = ld32(a.lc + (size_t)i * a.cstride);
#pragma unroll
    for (int by = 0; by < 4; ++by) P.luma(by, a.bxl, x.py + 4 * by);
#pragma unroll
    for (int by = 0; by < 2; ++by) P.chroma(a.p, by, a.bxc, x.pc + 4 * by);
}

/* GEN = false: one wave per task (s, f, rect row, span) in a flat grid;
 * GEN = true: grid (tasks of a frame, record slots), the frames k_dyn_rows
 * listed (ctr[1] of them from ctr[DYN_CTR_LIST], as k_dyn_recon<true> takes
 * them).  A row belongs to the instantiation its chroma rows ask for. */
template <bool GEN>
__global__ __launch_bounds__(MK_T) void k_dyn_mask_diff(MaskArgs a)
{
    const MaskJob &j = a.j;
    const uint32_t lane = threadIdx.x & 63u, mbl = lane >> 2, q = lane & 3u;
    const uint32_t t = __builtin_amdgcn_readfirstlane(blockIdx.x * MK_WAVES + (threadIdx.x >> 6));
    uint32_t sp, r, s, f;
    if (GEN) {
        if ((uint32_t)blockIdx.y >= min(j.ctr[1], j.g.gen_cap)) return;
        if (t >= (uint32_t)j.g.h * a.nsp) return;
        const uint32_t fr = j.ctr[DYN_CTR_LIST + blockIdx.y];
        s = fr / (uint32_t)j.ld_fr;
        f = fr - s * (uint32_t)j.ld_fr;
        r = csc::divmod(t, a.nsp, a.m_nsp, &sp);
        if (s >= j.S || f >= j.nframes) return;
    } else {
        if (t >= a.total) return;
        const uint32_t row = csc::divmod(t, a.nsp, a.m_nsp, &sp);
        const uint32_t item = csc::divmod(row, (uint32_t)j.g.h, a.m_h, &r);
        s = csc::divmod(item, j.nframes, a.m_nf, &f);
    }
    const size_t nb = (size_t)s * j.ld_fr + f;
    const uint32_t mx = 16u * sp + mbl;
    DynGeom g = j.g;
    dyn_frame_geom(g, nb);                              /* RowPred's origin and the rect's size: the frame's own */
    if (r >= (uint32_t)g.h) return;                     /* past the rows of a frame sized on its own */
    const bool on = mx < (uint32_t)g.w;                 /* a partial last span, or past the frame's own columns */
    /* the frame's block of the map keeps the batch's stride; inside it the map is the frame's own w_f x h_f */
    uint2 *mp = reinterpret_cast<uint2 *>(j.map) + nb * (size_t)g.ld_h * (size_t)g.ld_w + (size_t)r * (size_t)g.w + mx;
    const DynFrame df = j.dfr[nb];
    if (df.nal < 0) {                                   /* no dynamic NAL: zero entries */
        if (!GEN && on && q == 0u) *mp = make_uint2(0u, 0u);
        return;
    }
    ReconLds L;
    if (row_table<GEN>(j, g, nb, (int)s, (int)r, L) != GEN) return;
    const uint8_t *rb = j.refs + (size_t)s * g.ref_ld;
    const RowPred<GEN> P{L, rb, (uint32_t)g.pw * (uint32_t)g.ph / 4, g.x0, g.y0 + (int)r, j.st + s,
                         j.nal + (size_t)s * j.ld_nal + df.nal};
    uint32_t dy = 0u, dc = 0u;
    if (on) {
        MbPix x;
        mb_load<GEN, true>(P, mb_at(j.src + (size_t)s * g.src_ld + (size_t)f * g.src_fr, g, (int)r, mx, q), x);
#pragma unroll
        for (int i = 0; i < 16; ++i) dy = sq4b(x.sy[i], x.py[i], dy);
#pragma unroll
        for (int i = 0; i < 8; ++i) dc = sq4b(x.sc[i], x.pc[i], dc);
    }
    dy = quad_sum(dy);
    dc = quad_sum(dc);
    if (on && q == 0u) *mp = make_uint2(dy, dc);
}

/* GEN = false: grid (rect rows, frames, streams); GEN = true: (rect rows, record slots) */
template <bool GEN>
__global__ __launch_bounds__(MK_T) void k_dyn_mask_fill(MaskArgs a)
{
    __shared__ uint32_t red[MK_WAVES][2];
    const MaskJob &j = a.j;
    const uint32_t lane = threadIdx.x & 63u, mbl = lane >> 2, q = lane & 3u, wave = threadIdx.x >> 6;
    const uint32_t r = blockIdx.x;
    uint32_t s, f;
    if (GEN) {
        if ((uint32_t)blockIdx.y >= min(j.ctr[1], j.g.gen_cap)) return;
        const uint32_t fr = j.ctr[DYN_CTR_LIST + blockIdx.y];
        s = fr / (uint32_t)j.ld_fr;
        f = fr - s * (uint32_t)j.ld_fr;
        if (s >= j.S || f >= j.nframes) return;
    } else {
        s = blockIdx.z;
        f = blockIdx.y;
    }
    const size_t nb = (size_t)s * j.ld_fr + f;
    const DynFrame df = j.dfr[nb];
    if (df.nal < 0) return;                             /* no dynamic NAL: the source stays */
    DynGeom g = j.g;
    dyn_frame_geom(g, nb);
    if (r >= (uint32_t)g.h) return;                     /* past the rows of a frame sized on its own */
    ReconLds L;
    if (row_table<GEN>(j, g, nb, (int)s, (int)r, L) != GEN) return;
    const uint8_t *rb = j.refs + (size_t)s * g.ref_ld;
    const RowPred<GEN> P{L, rb, (uint32_t)g.pw * (uint32_t)g.ph / 4, g.x0, g.y0 + (int)r, j.st + s,
                         j.nal + (size_t)s * j.ld_nal + df.nal};
    uint8_t *fs = j.src + (size_t)s * g.src_ld + (size_t)f * g.src_fr;
    const uint32_t *fm = j.map + nb * (size_t)g.ld_h * (size_t)g.ld_w * 2u;
    const uint32_t w = (uint32_t)g.w, h = (uint32_t)g.h;
    uint32_t e = 0u;                                    /* this lane's plane (q >> 1): squared error dropped */
    for (uint32_t sp = wave; sp < a.nsp; sp += MK_WAVES) {
        const uint32_t mx = 16u * sp + mbl;
        const bool on = mx < w;
        /* the MB's neighbours, a quarter per lane of its quad */
        uint32_t kp = on && kept_part(fm, w, h, mx, r, j.rule, q, 4u) ? 1u : 0u;
        kp = quad_sum(kp);
        if (!on || kp) continue;
        const MbAt at = mb_at(fs, g, (int)r, mx, q);
        MbPix x;
        mb_load<GEN, false>(P, at, x);
#pragma unroll
        for (int i = 0; i < 8; ++i) e = sq4b(x.sc[i], x.pc[i], e);
        if (j.rule.apply) {
#pragma unroll
            for (int i = 0; i < 16; ++i) st32(at.ly + (size_t)i * at.lstride, x.py[i]);
#pragma unroll
            for (int i = 0; i < 8; ++i) st32(at.lc + (size_t)i * at.cstride, x.pc[i]);
        }
    }
    /* a lane's sum stays below 2^26 (16 spans / 4 waves, 32 samples each), a row's below 2^31 */
    const uint32_t ecb = wave_sum(q < 2u ? e : 0u), ecr = wave_sum(q < 2u ? 0u : e);
    if (lane == 0u) {
        red[wave][0] = ecb;
        red[wave][1] = ecr;
    }
    __syncthreads();
    if (threadIdx.x < 2u) {
        unsigned long long v = 0;
#pragma unroll
        for (uint32_t k = 0; k < MK_WAVES; ++k) v += red[k][threadIdx.x];
        j.part[(nb * (size_t)g.ld_h + r) * 2u + threadIdx.x] = v;
    }
}

/* grid (frames, streams) */
__global__ __launch_bounds__(MK_T) void k_dyn_mask_rec(MaskArgs a)
{
    __shared__ Acc part[MK_T];
    const MaskJob &j = a.j;
    const uint32_t s = blockIdx.y, f = blockIdx.x, t = threadIdx.x;
    const size_t nb = (size_t)s * j.ld_fr + f;
    if (j.dfr[nb].nal < 0) {
        if (t == 0u) j.res[nb] = noframe();
        return;
    }
    DynGeom g = j.g;
    dyn_frame_geom(g, nb);                              /* the frame's own w_f x h_f MBs */
    const uint32_t w = (uint32_t)g.w, h = (uint32_t)g.h, nmb = w * h;
    uint32_t *fm = j.map + nb * (size_t)g.ld_h * (size_t)g.ld_w * 2u;
    Acc acc = acc_init();
    /* the KEPT bit goes into words whose other 31 bits never change, and a
     * neighbour's read masks it off: what another thread sees of this
     * thread's store does not matter */
    for (uint32_t i = t; i < nmb; i += MK_T) fm[2u * i + 1u] = acc_mb(acc, fm, w, h, i % w, i / w, j.rule);
    const unsigned long long *pr = j.part + nb * (size_t)g.ld_h * 2u;
    for (uint32_t r = t; r < h; r += MK_T) {
        acc.drop[1] += pr[2u * r];
        acc.drop[2] += pr[2u * r + 1u];
    }
    part[t] = acc;
    for (uint32_t n = MK_T / 2u; n > 0u; n >>= 1) {
        __syncthreads();
        if (t < n) acc_merge(part[t], part[t + n]);
    }
    if (t == 0u) j.res[nb] = record(part[0]);
}

}  // namespace

int mask_launch(hipStream_t hs, const MaskJob *job, hipEvent_t ev0, hipEvent_t ev1)
{
    if (job->S == 0 || job->nframes == 0 || job->g.w <= 0 || job->g.h <= 0) return 0;
    if (mask_tasks(job) >= MASK_MAX_TASKS) return -1;
    MaskArgs a{};
    a.j = *job;
    a.nsp = ((uint32_t)job->g.w + 15u) / 16u;
    a.total = (uint32_t)mask_tasks(job);
    a.m_nsp = scroll::csc::magic(a.nsp);
    a.m_h = scroll::csc::magic((uint32_t)job->g.h);
    a.m_nf = scroll::csc::magic(job->nframes);
    const uint32_t h = (uint32_t)job->g.h, nf = job->nframes, S = job->S;
    const uint32_t slots = std::min<uint32_t>(job->g.gen_cap, nf * S);
    const uint32_t fblocks = (h * a.nsp + MK_WAVES - 1u) / MK_WAVES;
    if (ev0 && hipEventRecord(ev0, hs) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dyn_mask_diff<false>, dim3((a.total + MK_WAVES - 1u) / MK_WAVES), dim3(MK_T), 0, hs, a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dyn_mask_diff<true>, dim3(fblocks, slots), dim3(MK_T), 0, hs, a);
    if (hipGetLastError() != hipSuccess) return -1;
    if (ev1 && hipEventRecord(ev1, hs) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dyn_mask_fill<false>, dim3(h, nf, S), dim3(MK_T), 0, hs, a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dyn_mask_fill<true>, dim3(h, slots), dim3(MK_T), 0, hs, a);
    if (hipGetLastError() != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dyn_mask_rec, dim3(nf, S), dim3(MK_T), 0, hs, a);
    return hipGetLastError() != hipSuccess ? -1 : 0;
}
