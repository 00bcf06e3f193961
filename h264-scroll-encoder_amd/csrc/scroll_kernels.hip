/*
 * scroll_kernels.hip -- MI355X (gfx950) engine of the many-stream scroll
 * composer: plan kernel (per-stream state machine + exact NAL sizes + output
 * offsets), emit kernel (random-access bit generation, 16 B per lane) and
 * the host-delivery kernels, with their launchers (scroll_engine.h).
 *
 * Reference hot path: src/composer.c:255-264 -> src/h264_writer.c:541-782 ->
 * src/bitwriter.c -> src/nal.c:52-84.  See DESIGN.md for the data layout and
 * the roofline of each kernel.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "scroll_engine.h"
#include "dyn_engine.h"         /* DYN_CTR_LIST: the counters k_plan zeroes */
#include "scroll_device.h"

using namespace scroll;

static_assert(sizeof(DevStream) == 256, "DevStream must stay 256 B");
static_assert(sizeof(NalDesc) == 32, "NalDesc must stay 32 B");

namespace {

#ifndef SCROLL_TILE
#define SCROLL_TILE 16
#endif
#ifndef SCROLL_EMIT_WAVES
#define SCROLL_EMIT_WAVES 1
#endif
constexpr int TILE = SCROLL_TILE;              /* NAL units per wave tile in k_emit */
constexpr int EMIT_WAVES = SCROLL_EMIT_WAVES;  /* waves per k_emit workgroup        */
#ifndef SCROLL_PLAN_THREADS
#define SCROLL_PLAN_THREADS 1024   /* 16 waves: the NAL sizing pass is latency-bound */
#endif
constexpr int PLAN_THREADS = SCROLL_PLAN_THREADS;

/* ---------------------------------------------------------------------- */
/* helpers                                                                 */
/* ---------------------------------------------------------------------- */
__device__ inline uint64_t lanemask_lt()
{
    uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

__device__ inline uint64_t wave_incl_scan(uint64_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint64_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ inline void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline NalCtx make_ctx(const int32_t *cfg, const int32_t *wo, const int32_t *wl,
                                  const int32_t *wv, const NalDesc &d)
{
    NalCtx c;
    c.w = cfg[0];
    c.h = cfg[1];
    c.log2_mfn = cfg[2];
    c.poc_type = cfg[3];
    c.log2_poc = cfg[4];
    c.deblock = cfg[5];
    c.kind = d.kind;
    c.off = d.off;
    c.frame_num = d.frame_num;
    c.nwp = d.nwp;
    c.wp_off = wo;
    c.wp_lt = wl;
    c.wp_valid = wv;
    return c;
}

/* ---------------------------------------------------------------------- */
/* k_plan: one workgroup per stream.                                       */
/*  phase 1 (wave 0): composer_write_scroll_frame state machine over the   */
/*          stream's offsets (src/composer.c:255-264, h264_writer.c:666-676,*/
/*          :772-777) -> one NalDesc per NAL unit, frame_num per NAL.       */
/*  phase 2 (all waves): exact size of every NAL (run layout, or the serial */
/*          path when emulation prevention / long codes are possible), and  */
/*          a block scan -> byte offset of every NAL in the stream arena.   */
/* With the dynamic rect the kernel runs twice around the dynamic coder: a  */
/* pass (PLAN_STATE: phase 1, totals + final table to PlanPending, frame -> */
/* scroll NAL map to DynFrame) and a size pass (PLAN_SIZE: phase 2, sizes   */
/* of dynamic NALs from DynFrame).                                          */
/* ---------------------------------------------------------------------- */
__global__ __launch_bounds__(PLAN_THREADS) void k_plan(DevStream *__restrict__ st,
                                                       const int32_t *__restrict__ offs,
                                                       int ld_off, NalDesc *__restrict__ nal,
                                                       int ld_nal, int nframes, int mode,
                                                       int flags, PlanPending *__restrict__ pend,
                                                       DynFrame *__restrict__ dfr, int ld_fr,
                                                       const uint32_t *__restrict__ pool_ctr = nullptr,
                                                       uint32_t spill_cap = 0, uint32_t gen_cap = 0,
                                                       uint32_t *__restrict__ ctr_zero = nullptr,
                                                       const uint32_t *__restrict__ dpos = nullptr)
{
    const int s = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int32_t s_cfg[8];
    __shared__ int32_t s_wo[8], s_wl[8], s_wv[8];
    __shared__ int32_t s_nnal, s_nwp_end, s_fn_end, s_nalwp;
    __shared__ uint64_t s_wsum[PLAN_THREADS / 64];
    __shared__ uint64_t s_carry;
    __shared__ int32_t s_nslow;

    DevStream *S = st + s;
    if (tid < 8) {
        s_wo[tid] = S->wp_off[tid];
        s_wl[tid] = S->wp_lt[tid];
        s_wv[tid] = S->wp_valid[tid];
    }
    /* the dynamic rect's per-compose counters (spill / record slots),
     * zeroed here rather than by a fill launch of their own */
    if (ctr_zero && s == 0 && tid < DYN_CTR_LIST) ctr_zero[tid] = 0u;
    if (tid == 0) {
        s_cfg[0] = S->w; s_cfg[1] = S->h; s_cfg[2] = S->log2_mfn; s_cfg[3] = S->poc_type;
        s_cfg[4] = S->log2_poc; s_cfg[5] = S->deblock; s_cfg[6] = S->frame_num; s_cfg[7] = S->nwp;
        s_carry = 0;
        s_nslow = 0;
        if ((flags & PLAN_REWIND) && !(flags & PLAN_STATE)) {
            S->out_pos = 0;
            S->undelivered = 0;
        }
        /* the dynamic rect ran out of a scratch pool somewhere in this
         * compose: no stream commits, so the same compose can be retried
         * once the batch has grown its pools */
        if ((flags & PLAN_SIZE) && pool_ctr && (pool_ctr[0] > spill_cap || pool_ctr[1] > gen_cap))
            S->err |= SCROLL_DEVERR_DYN;
    }
    const int F = nframes >= 0 ? nframes : S->frames;
    NalDesc *N = nal + (size_t)s * ld_nal;
    __syncthreads();
    const uint64_t out0 = S->out_pos;

    if (flags & PLAN_SIZE) {
        if (tid < 8) {
            s_wo[tid] = pend[s].wo[tid];
            s_wl[tid] = pend[s].wl[tid];
            s_wv[tid] = pend[s].wv[tid];
        }
        if (tid == 0) {
            s_nnal = pend[s].nnal;
            s_nwp_end = pend[s].nwp_end;
            s_fn_end = pend[s].fn_end;
            s_nalwp = pend[s].nalwp;
        }
    } else if (mode == SCROLL_PLAN_EXPLICIT) {
        if (tid == 0) {
            s_nnal = S->nnal;
            s_nwp_end = s_cfg[7];
            s_fn_end = s_cfg[6];
            s_nalwp = 0;
        }
    } else if (wave == 0) {
        /* waypoint table held in registers with static indices (no scratch) */
        int wo[8], wl[8], wv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            wo[k] = s_wo[k];
            wl[k] = s_wl[k];
            wv[k] = s_wv[k];
        }
        int n = s_cfg[7];
        const int fn0 = s_cfg[6];
        int nalc = 0, nalwp = 0;
        const int32_t *O = offs + (size_t)s * ld_off;
        for (int base = 0; base < F; base += 64) {
            int i = base + lane;
            bool valid = i < F;
            int off = valid ? O[i] : 0;
            bool cand = valid && off != 0 && (off % MVL) == 0;   /* h264_writer.c:667-668 */
            uint64_t mask = __ballot(cand);
            int my_n = n, has_wp = 0, wp_nb = 0;
            while (mask) {
                int jl = __ffsll((unsigned long long)mask) - 1;
                mask &= mask - 1;
                int offj = __shfl(off, jl, 64);
                bool need = true;
#pragma unroll
                for (int k = 0; k < 8; ++k)                       /* :670-674 */
                    if (k < n && wv[k] && wo[k] == offj) need = false;
                if (need) {
                    if (lane == jl) {
                        has_wp = 1;
                        wp_nb = n;
                    }
                    if (n < 8) {                                  /* :772-777 */
#pragma unroll
                        for (int k = 0; k < 8; ++k)
                            if (k == n) {
                                wo[k] = offj;
                                wl[k] = 2 + n;
                                wv[k] = 1;
                            }
                        n++;
                    }
                    if (lane >= jl) my_n = n;
                }
            }
            uint64_t vmask = __ballot(valid), wmask = __ballot(has_wp != 0);
            uint64_t lt = lanemask_lt();
            if (mode == SCROLL_PLAN_COMPOSER) {
                int first = nalc + __popcll(vmask & lt) + __popcll(wmask & lt);
                if (valid) {
                    if (has_wp) {
                        NalDesc d{};
                        d.kind = 1; d.off = off; d.frame_num = fn0 + first; d.nwp = (uint8_t)wp_nb;
                        d.frame = (uint32_t)i;
                        N[first] = d;
                    }
                    NalDesc d{};
                    d.kind = 0; d.off = off; d.frame_num = fn0 + first + has_wp;
                    d.nwp = (uint8_t)my_n; d.frame = (uint32_t)i;
                    N[first + has_wp] = d;
                    /* dpos (the plain rect's per-frame origins): a frame without a rect has no dynamic NAL */
                    if (flags & PLAN_DYN)
                        dfr[(size_t)s * ld_fr + i].nal =
                            dpos && dpos[(size_t)s * ld_fr + i] == DYN_POS_NONE ? -1 : first + has_wp;
                }
                nalc += __popcll(vmask) + __popcll(wmask);
            } else {   /* experiment: waypoint NAL replaces the scroll NAL */
                int idx = nalc + __popcll(vmask & lt);
                if (valid) {
                    NalDesc d{};
                    d.kind = has_wp ? 1 : 0; d.off = off; d.frame_num = fn0 + idx;
                    d.nwp = (uint8_t)(has_wp ? wp_nb : my_n); d.frame = (uint32_t)i;
                    N[idx] = d;
                    if (flags & PLAN_DYN)
                        dfr[(size_t)s * ld_fr + i].nal =
                            has_wp || (dpos && dpos[(size_t)s * ld_fr + i] == DYN_POS_NONE) ? -1 : idx;
                }
                nalc += __popcll(vmask);
            }
            nalwp += __popcll(wmask);
        }
        if (lane < 8) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k == lane) {
                    s_wo[k] = wo[k];
                    s_wl[k] = wl[k];
                    s_wv[k] = wv[k];
                }
        }
        if (lane == 0) {
            s_nnal = nalc;
            s_nwp_end = n;
            s_fn_end = fn0 + nalc;
            s_nalwp = nalwp;
        }
    }
    __syncthreads();
    if (flags & PLAN_STATE) {
        if (tid < 8) {
            pend[s].wo[tid] = s_wo[tid];
            pend[s].wl[tid] = s_wl[tid];
            pend[s].wv[tid] = s_wv[tid];
        }
        if (tid == 0) {
            pend[s].nnal = s_nnal;
            pend[s].nwp_end = s_nwp_end;
            pend[s].fn_end = s_fn_end;
            pend[s].nalwp = s_nalwp;
        }
        return;
    }

    /* phase 2: sizes + offsets.  Every NAL reads the FINAL table: entries are
     * only appended, and a NAL only looks at its first nwp entries. */
    const int nnal = s_nnal;
    for (int t = 0; t < nnal; t += PLAN_THREADS) {
        int j = t + tid;
        uint64_t sz = 0;
        int slow = 0;
        if (j < nnal) {
            NalDesc d = N[j];
            NalCtx c = make_ctx(s_cfg, s_wo, s_wl, s_wv, d);
            uint32_t fsz = 0;
            /* (DynFrame.nal < 0 on a scroll NAL: only with dpos, a frame without a rect -- k_emit's) */
            const bool dyn = (flags & PLAN_DYN) && d.kind == 0 && (!dpos || dfr[(size_t)s * ld_fr + d.frame].nal >= 0);
            bool fast = !dyn && !(flags & SCROLL_DEBUG_FORCE_SERIAL) && build_nal<false>(c, nullptr, &fsz);
            if (dyn) {
                const DynFrame df = dfr[(size_t)s * ld_fr + d.frame];
                sz = 5u + (uint64_t)df.rbsp_bytes + df.ep;     /* start code + header + EBSP */
                slow = 2;
            } else if (fast) {
                sz = fsz;
            } else {
                sz = serial_size(c);
                slow = 1;
            }
        }
        uint64_t inc = wave_incl_scan(sz, lane);
        if (lane == 63) s_wsum[wave] = inc;
        int ns = __popcll(__ballot(slow == 1));
        if (lane == 0 && ns) atomicAdd(&s_nslow, ns);
        __syncthreads();
        uint64_t before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_wsum[w];
        if (j < nnal) {
            N[j].out_off = out0 + before + inc - sz;
            N[j].size = (uint32_t)sz;
            N[j].slow = (uint8_t)slow;
        }
        __syncthreads();
        if (tid == 0) {
            uint64_t tot = 0;
            for (int w = 0; w < PLAN_THREADS / 64; ++w) tot += s_wsum[w];
            s_carry += tot;
        }
        __syncthreads();
    }

    if (tid == 0) {
        uint64_t total = s_carry;
        S->n_slow = s_nslow;
        if (out0 + total > S->out_cap || (S->err & SCROLL_DEVERR_STAGED)) {
            if (!(S->err & SCROLL_DEVERR_STAGED))
                S->err |= SCROLL_DEVERR_OVERFLOW;   /* nothing committed, nothing emitted */
            S->nnal = 0;
            S->batch_bytes = 0;
        } else {
            S->out_pos = out0 + total;
            S->batch_bytes = total;
            S->undelivered += total;
            S->nnal = nnal;
            S->nal_wp = s_nalwp;
            S->frame_num = s_fn_end;
            S->nwp = s_nwp_end;
            if (mode != SCROLL_PLAN_EXPLICIT) S->frames_written += F;
        }
    }
    if (tid < 8 && mode != SCROLL_PLAN_EXPLICIT && out0 + s_carry <= S->out_cap &&
        !(S->err & SCROLL_DEVERR_STAGED)) {
        S->wp_off[tid] = s_wo[tid];
        S->wp_lt[tid] = s_wl[tid];
        S->wp_valid[tid] = s_wv[tid];
    }
}

/* ---------------------------------------------------------------------- */
/* k_emit: one wave per tile of TILE consecutive NAL units of one stream.   */
/*                                                                          */
/* Rule: every 128-byte line of an arena is written whole, by one wave, in  */
/* one pass.  A line written in pieces at different times (16- to 64-byte   */
/* holes filled later) costs the memory system up to 2x (DESIGN.md §6,      */
/* tools/store_floor.hip).  So:                                             */
/*  1. lanes build the run layouts of the tile's NALs plus up to XB / XA    */
/*     neighbour NALs, which supply the bytes of the two seam lines the     */
/*     tile shares with the adjacent tiles;                                 */
/*  2. the wave's chunk range covers whole lines [line(B0), line(B1)).      */
/*     Chunks are classified into PURE entries (runs of chunks inside one   */
/*     periodic run) and MIXED entries (runs of chunks holding NAL headers, */
/*     run boundaries, NAL boundaries, seam bytes);                         */
/*  3. mixed chunks are computed, one lane each, into LDS;                  */
/*  4. one pass streams every chunk of the range in order, 4 groups of 64   */
/*     chunks per iteration: each lane finds its entry (entry-start flag    */
/*     map + mbcnt), pulls the entry data by ds_bpermute and either expands */
/*     the run pattern at its phase or copies its mixed words from LDS.     */
/* Seam lines: both neighbours compute the identical full line and write    */
/* it (benign duplicate); a side whose neighbour bytes cannot be computed   */
/* here (serial-path or too many tiny neighbour NALs) writes only its own   */
/* bytes of that line.  A stream's first tile in a launch merges the line   */
/* head from memory (the previous compose's bytes); its last tile zero-     */
/* fills its line tail (arena slack).  Tiles holding a serial-path NAL use  */
/* the generic byte path and the owning lane writes that NAL serially;     */
/* dynamic-rect NALs (slow = 2) are written by k_dyn_gather.                */
/* ---------------------------------------------------------------------- */
constexpr int PURE_U = 4;         /* 64-chunk groups per stream iteration      */
constexpr int XB = SEAM_XB, XA = SEAM_XA;   /* neighbour layouts before / after the tile */
constexpr int NL = XB + TILE + XA;
constexpr int MAXPE = 8 * TILE;   /* pure + mixed entries per wave             */
constexpr int MAXMX = 6 * TILE;   /* mixed chunks per wave (~3-4 per NAL)      */
constexpr uint32_t PE_VS_MASK = (1u << 22) - 1;   /* chunks of a tile < 2^22   */
constexpr uint32_t PE_MIXED = 15u;                /* run field of a mixed entry */
static_assert(NL <= 64, "layout index is 6 bits and one lane builds each layout");
static_assert(PURE_U == 4, "the flag map packs 4 groups per lane dword");

struct EmitWaveLds {
    Lay lay[NL];
    int32_t noff[NL + 1];         /* layout i's first byte - B0 (signed)       */
    uint32_t pe_cb[MAXPE];        /* mixed entry: index of its first chunk in mw */
    uint32_t pe_vj[MAXPE];        /* first chunk (rel cs) | layout << 22 | run << 28 */
    uint32_t mx[MAXMX];           /* mixed chunk: (chunk rel cs) << 6 | first layout */
    alignas(16) uint32_t mw[MAXMX][4];   /* mixed chunk words, MSB first (ds_read_b128) */
    uint32_t flg[64];             /* stream loop: entry-start flags, byte 4 p + u
                                     = an entry starts at chunk v0 + 64 u + p   */
};

/* 16-B global store to an integer address (address space 1: a
 * global_store, not flat) */
__device__ inline void store_raw(uint64_t addr, const uint32_t o[4])
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) u32x4 gu32x4;
    u32x4 v;
    v.x = o[0];
    v.y = o[1];
    v.z = o[2];
    v.w = o[3];
    *reinterpret_cast<gu32x4 *>(addr) = v;
}

/* MSB-first words of a chunk whose bytes < first are outside this wave */
__device__ inline void store_bytes(uint8_t *A, uint64_t p, uint64_t lo, uint64_t hi,
                                   const uint32_t w[4])
{
    for (int k = 0; k < 16; ++k) {
        const uint64_t x = p + (uint64_t)k;
        if (x < lo || x >= hi) continue;
        A[x] = (uint8_t)(w[k >> 2] >> (24 - 8 * (k & 3)));
    }
}

__global__ __launch_bounds__(EMIT_WAVES * 64) void k_emit(const DevStream *__restrict__ st,
                                                          const NalDesc *__restrict__ nal,
                                                          int ld_nal, uint8_t *__restrict__ arena,
                                                          uint64_t ld_arena, int flags,
                                                          uint64_t *__restrict__ dbg)
{
    __shared__ EmitWaveLds s_w[EMIT_WAVES];
    __shared__ int32_t s_cfg[8], s_wo[8], s_wl[8], s_wv[8];
    __shared__ LenLut s_lut;

    const int s = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = (int)uni((uint32_t)(tid >> 6));      /* wave-uniform -> SGPR */
    const DevStream *S = st + s;
    const int t0 = (blockIdx.x * EMIT_WAVES + wave) * TILE;
    /* lane i <-> layout i <-> NAL t0 - XB + i.  Every start-up load in one
     * memory round trip: the descriptors (bounded by the descriptor
     * capacity; lanes past nnal are ignored below), the stream config and
     * its waypoint table. */
    const int ti = t0 - XB + lane;
    NalDesc d{};
    if (lane < NL && ti >= 0 && ti < ld_nal) d = nal[(size_t)s * ld_nal + ti];
    if (tid < 8) {
        s_wo[tid] = S->wp_off[tid];
        s_wl[tid] = S->wp_lt[tid];
        s_wv[tid] = S->wp_valid[tid];
    }
    if (tid == 0) {
        s_cfg[0] = S->w; s_cfg[1] = S->h; s_cfg[2] = S->log2_mfn; s_cfg[3] = S->poc_type;
        s_cfg[4] = S->log2_poc; s_cfg[5] = S->deblock;
    }
    if (tid < 64) lut_entry((uint32_t)tid + 1u, s_lut.magic[tid], s_lut.mods[tid]);
    const int nnal = S->nnal;
    __syncthreads();
    if (t0 >= nnal) return;
    const int cnt = min(TILE, nnal - t0);
    const int lo = max(0, XB - t0);                       /* first valid layout   */
    const int hi = XB + cnt + min(XA, nnal - t0 - cnt);   /* one past the last    */
    const LenLut &T = s_lut;
    EmitWaveLds &W = s_w[wave];
    const bool stamps = (flags & SCROLL_DEBUG_EMIT_STAMPS) && dbg;
    uint64_t *stamp = dbg + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * EMIT_WAVES + wave) * 8;
    auto mark = [&](int k) {
        if (stamps) {
            uint64_t t = __builtin_amdgcn_s_memtime();
            if (lane == 0) stamp[k] = t;
        }
    };
    mark(0);
    if (stamps && lane == 0) stamp[5] = __builtin_amdgcn_s_memrealtime();
    Lay *L = W.lay;
    int32_t *noff = W.noff;
    uint8_t *A = arena + (size_t)s * ld_arena;

    /* 1. layouts (own NALs + neighbours) */
    const uint64_t B0 = ((uint64_t)__builtin_amdgcn_readlane((int)(uint32_t)(d.out_off >> 32), XB) << 32) |
                        (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)d.out_off, XB);
    const bool valid = lane >= lo && lane < hi;
    const bool own = lane >= XB && lane < XB + cnt;
    bool my_slow = false;
    NalCtx my_ctx;
    if (valid) {
        my_ctx = make_ctx(s_cfg, s_wo, s_wl, s_wv, d);
        my_slow = d.slow != 0;
        if (!my_slow) {
            uint32_t sz;
            build_nal<true, false>(my_ctx, &L[lane], &sz);   /* plan proved it fast */
        } else {
            L[lane].nal_bits = d.size * 8u;
            L[lane].used_bits = 0;
            L[lane].hdr_bits = 0;
            L[lane].nruns = 0;
        }
        noff[lane] = (int32_t)(int64_t)(d.out_off - B0);
        if (lane == hi - 1) noff[hi] = (int32_t)(int64_t)(d.out_off + d.size - B0);
    }
    const uint64_t slow_mask = __ballot(valid && my_slow);
    const bool any_slow = (slow_mask >> XB) & ((cnt == 64 ? 0ull : (1ull << cnt)) - 1ull) ? true : false;
    wave_lds_sync();
    mark(1);
    if (flags & SCROLL_DEBUG_EMIT_BUILD) return;

    const uint64_t B1 = B0 + (uint64_t)(int64_t)noff[XB + cnt];

    /* seam lines (scroll_device.h seam_plan): head bytes [line(B0), B0)
     * from memory (a stream's first tile) or from previous layouts; tail
     * bytes [B1, line end) zero (last tile) or from next layouts */
    const Seams z = seam_plan(B0, B1, t0, cnt, nnal, lo, hi, noff, slow_mask);
    const bool head_full = z.head_full, tail_full = z.tail_full;
    const uint64_t cs = z.cs, ce = z.ce;
    const uint64_t nch = ce - cs;

    /* 2. classify the owned chunks of every own NAL into entries */
    uint32_t npe = 0, nmx = 0;
    uint64_t own0 = 0, own1 = 0, Aj = 0;
    if (own && !my_slow) {
        owned_chunks(z, B0, noff, lane, cnt, own0, own1);
        Aj = 8 * (B0 + (uint64_t)(int64_t)noff[lane]);
        entry_walk(L[lane], Aj, own0, own1, [&](int r, uint64_t c0e, uint64_t c1e) {
            npe++;
            if (r < 0) nmx += (uint32_t)(c1e - c0e);
        });
    }
    const uint32_t pe_inc = (uint32_t)wave_incl_scan(npe, lane);
    const uint32_t mx_inc = (uint32_t)wave_incl_scan(nmx, lane);
    const uint32_t tot_pe = uni((uint32_t)__shfl(pe_inc, 63, 64));
    const uint32_t tot_mx = uni((uint32_t)__shfl(mx_inc, 63, 64));
    const bool generic = any_slow || (B1 - B0) >= (1ull << 26) || nch >= (1ull << 22) ||
                         tot_pe > (uint32_t)MAXPE || tot_mx > (uint32_t)MAXMX;

    if (!generic) {
        if (own) {
            uint32_t e = pe_inc - npe, m = mx_inc - nmx;
            entry_walk(L[lane], Aj, own0, own1, [&](int r, uint64_t c0e, uint64_t c1e) {
                W.pe_vj[e] = (uint32_t)(c0e - cs) | ((uint32_t)lane << 22) |
                             ((r < 0 ? PE_MIXED : (uint32_t)r) << 28);
                W.pe_cb[e] = m;
                e++;
                if (r < 0)
                    for (uint64_t c = c0e; c < c1e; ++c)
                        W.mx[m++] = ((uint32_t)(c - cs) << 6) | mixed_first(z, c << 4, B0, lane);
            });
        }
        wave_lds_sync();
        mark(2);

        /* 3. mixed chunks -> LDS (head chunks merge the bytes before B0 from
         * memory on the launch's first tile) */
        const int mix_hi = tail_full ? z.t_hi : XB + cnt;
        const uint32_t mx_end = (flags & SCROLL_DEBUG_EMIT_NOMIXED) ? 0u : tot_mx;
        for (uint32_t k = (uint32_t)lane; k < mx_end; k += 64) {
            const uint32_t mm = W.mx[k];
            const uint64_t p = (cs + (mm >> 6)) << 4;
            uint32_t w[4];
            mixed_chunk(L, noff, mix_hi, (int)(mm & 63u), ((int64_t)p - (int64_t)B0) * 8, T, w);
            if (z.head_rmw && p < B0) {
                const uint4 old = *reinterpret_cast<const uint4 *>(A + p);
                const uint32_t ow[4] = {__builtin_bswap32(old.x), __builtin_bswap32(old.y),
                                        __builtin_bswap32(old.z), __builtin_bswap32(old.w)};
                const int32_t nb = (int32_t)(B0 - p);          /* bytes kept, 1..15 */
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    w[q] |= ow[q] & range_mask(0, 8 * nb - 32 * q);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) W.mw[k][q] = w[q];
        }
        wave_lds_sync();
        mark(3);
        if (stamps && lane == 0) stamp[6] = ((uint64_t)nch << 32) | tot_mx;

        /* 4. stream.  Lane k of a window holds entry ebase + k: first chunk
         * vs (relative to cs), and for a pure entry K = run bit of chunk cs
         * (mod 2^32; chunk cs + v starts at run bit K + 128 v), code len,
         * magic, pattern192; for a mixed entry len = 0 and K + v = the mw
         * index of chunk cs + v. */
        uint32_t ebase = 0;
        uint32_t e_vs = 0xffffffffu, e_K = 0, e_len = 0, e_mag = 0, e_q[6] = {0, 0, 0, 0, 0, 0};
        auto load_window = [&](uint32_t base) {
            const uint32_t idx = base + (uint32_t)lane;
            e_vs = 0xffffffffu;
            if (idx < tot_pe) {
                const uint32_t vj = W.pe_vj[idx];
                const uint32_t vs = vj & PE_VS_MASK;
                const int j = (int)((vj >> 22) & 63u);
                const uint32_t r = vj >> 28;
                e_vs = vs;
                if (r == PE_MIXED) {
                    e_len = 0;
                    e_mag = 0;
                    e_K = W.pe_cb[idx] - vs;
#pragma unroll
                    for (int z = 0; z < 6; ++z) e_q[z] = 0;
                } else {
                    const Lay &Lj = L[j];
                    const uint32_t rs0 = r ? Lj.run_end[r - 1] : Lj.hdr_bits;
                    const uint64_t Arun = 8 * (B0 + (uint64_t)(int64_t)noff[j]) + rs0;
                    e_K = (uint32_t)((cs << 7) - Arun);        /* chunk cs + v: bit K + 128 v */
                    e_len = Lj.len[r];
                    e_mag = T.magic[e_len - 1];
                    pattern192(Lj.pat[r][0], Lj.pat[r][1], T.mods[e_len - 1], e_q);
                }
            }
        };
        /* the 4 words of chunk v from entry data (len 0 = mixed) */
        auto words = [&](uint32_t v, uint32_t K, uint32_t len, uint32_t mag, const uint32_t q[6],
                         uint32_t w[4]) {
            pure_words(K + (v << 7), len ? len : 1u, mag, q, w);
            if (__ballot(len == 0u)) {                  /* some lane in a mixed entry */
                const uint32_t mi = len ? 0u : min(K + v, (uint32_t)MAXMX - 1u);
                const uint4 mv = *reinterpret_cast<const uint4 *>(W.mw[mi]);
                w[0] = len ? w[0] : mv.x;
                w[1] = len ? w[1] : mv.y;
                w[2] = len ? w[2] : mv.z;
                w[3] = len ? w[3] : mv.w;
            }
        };
        const uint32_t nv = (flags & SCROLL_DEBUG_EMIT_NOPURE) ? 0u : (uint32_t)nch;
        const bool do_store = !(flags & SCROLL_DEBUG_EMIT_NOSTORE);
        if (nv) load_window(0);
        auto store4 = [&](uint32_t (&w)[PURE_U][4], const uint32_t (&vv)[PURE_U]) {
            if (do_store) {
                /* byte-swap all groups first and keep them live together, so
                 * the stores read distinct registers (no WAR stall behind a
                 * queued store) */
                uint32_t o[PURE_U][4];
#pragma unroll
                for (int u = 0; u < PURE_U; ++u)
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[u][k] = __builtin_bswap32(w[u][k]);
                uint64_t ptr[PURE_U];
#pragma unroll
                for (int u = 0; u < PURE_U; ++u) {
                    ptr[u] = (uint64_t)(uintptr_t)A + ((cs + vv[u]) << 4);
                    asm volatile("" : "+v"(o[u][0]), "+v"(o[u][1]), "+v"(o[u][2]), "+v"(o[u][3]),
                                 "+v"(ptr[u]));
                }
#pragma unroll
                for (int u = 0; u < PURE_U; ++u) store_raw(ptr[u], o[u]);
                asm volatile("" ::"v"(o[PURE_U - 1][0]), "v"(ptr[0]));
            } else {
#pragma unroll
                for (int u = 0; u < PURE_U; ++u)
                    asm volatile("" ::"v"(w[u][0]), "v"(w[u][1]), "v"(w[u][2]), "v"(w[u][3]));
            }
        };

        for (uint32_t v0 = 0; v0 < nv; v0 += 64u * PURE_U) {
            const uint32_t vlast = min(v0 + 64u * PURE_U, nv) - 1u;
            uint64_t m = __ballot(e_vs <= vlast);
            if ((m >> 63) && ebase + 64 < tot_pe) {
                /* the window must hold every entry of the iteration */
                const uint32_t ks = ebase + (uint32_t)__popcll(__ballot(e_vs <= v0)) - 1u;
                if (ks != ebase) {
                    ebase = ks;
                    load_window(ebase);
                    m = __ballot(e_vs <= vlast);
                }
            }
            uint32_t w[PURE_U][4], vv[PURE_U];
            if ((m >> 63) && ebase + 64 < tot_pe) {
                /* > 64 entries in 256 chunks (tiny NALs): group by group,
                 * entry by entry, reloading the window as needed */
#pragma unroll
                for (int u = 0; u < PURE_U; ++u) {
                    const uint32_t v = min(v0 + 64u * (uint32_t)u + (uint32_t)lane, vlast);
                    vv[u] = v;
                    const uint32_t g = min(v0 + 64u * (uint32_t)u, vlast);
                    /* move the window to start at the entry holding g, so it
                     * holds all (<= 64) entries of the group */
                    for (;;) {
                        const uint64_t b = __ballot(e_vs <= g);
                        if (!(b >> 63) || ebase + 64 >= tot_pe) break;
                        ebase += 63;                      /* every entry starts <= g */
                        load_window(ebase);
                    }
                    const uint32_t ks = ebase + (uint32_t)__popcll(__ballot(e_vs <= g)) - 1u;
                    if (ks != ebase) {
                        ebase = ks;
                        load_window(ebase);
                    }
                    const uint32_t k0 = 0u;
                    const uint32_t k1 = (uint32_t)__popcll(__ballot(e_vs <= min(g + 63u, vlast))) - 1u;
                    uint32_t kk = k0;
                    for (uint32_t jb = k0 + 1; jb <= k1; ++jb)
                        kk += v >= (uint32_t)__builtin_amdgcn_readlane((int)e_vs, (int)jb) ? 1u : 0u;
                    const int src = (int)(kk << 2);
                    uint32_t q[6];
#pragma unroll
                    for (int z = 0; z < 6; ++z) q[z] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)e_q[z]);
                    words(v, (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)e_K),
                          (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)e_len),
                          (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)e_mag), q, w[u]);
                }
                store4(w, vv);
                continue;
            }
            const uint32_t ks0 = (uint32_t)__popcll(__ballot(e_vs <= v0)) - 1u;  /* window index */
            const bool starts = e_vs > v0 && e_vs <= vlast;
            if (__ballot(starts) == 0) {
                /* one entry covers the whole iteration: SGPR operands */
                const uint32_t K = (uint32_t)__builtin_amdgcn_readlane((int)e_K, (int)ks0);
                const uint32_t len = (uint32_t)__builtin_amdgcn_readlane((int)e_len, (int)ks0);
                const uint32_t mag = (uint32_t)__builtin_amdgcn_readlane((int)e_mag, (int)ks0);
                uint32_t q[6];
#pragma unroll
                for (int z = 0; z < 6; ++z) q[z] = (uint32_t)__builtin_amdgcn_readlane((int)e_q[z], (int)ks0);
#pragma unroll
                for (int u = 0; u < PURE_U; ++u) {
                    vv[u] = min(v0 + 64u * (uint32_t)u + (uint32_t)lane, vlast);
                    words(vv[u], K, len, mag, q, w[u]);
                }
            } else {
                /* entry-start flags of the 4 groups -> per-lane entry index
                 * (window lane) by one ballot + mbcnt per group */
                W.flg[lane] = 0u;
                if (starts) {
                    const uint32_t rel = e_vs - v0;
                    reinterpret_cast<uint8_t *>(W.flg)[(rel & 63u) * 4u + (rel >> 6)] = 1;
                }
                wave_lds_sync();
                const uint32_t f4 = W.flg[lane];
                uint32_t base = ks0;
#pragma unroll
                for (int u = 0; u < PURE_U; ++u) {
                    const uint32_t fu = (f4 >> (8 * u)) & 255u;
                    const uint64_t B = __ballot(fu != 0u);
                    const uint32_t below = __builtin_amdgcn_mbcnt_hi(
                        (uint32_t)(B >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)B, 0u));
                    const uint32_t kk = base + below + fu;
                    base += (uint32_t)__popcll(B);
                    vv[u] = min(v0 + 64u * (uint32_t)u + (uint32_t)lane, vlast);
                    const int src = (int)(kk << 2);
                    uint32_t q[6];
#pragma unroll
                    for (int z = 0; z < 6; ++z) q[z] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)e_q[z]);
                    words(vv[u], (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)e_K),
                          (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)e_len),
                          (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)e_mag), q, w[u]);
                }
            }
            store4(w, vv);
        }

        /* partial chunks of a seam line whose neighbour bytes are not
         * available here: own bytes only */
        if (!(flags & SCROLL_DEBUG_EMIT_NOBYTES)) {
            const bool ph = !head_full && (B0 & 15);
            const bool pt = !tail_full && (B1 & 15) && (B1 >> 4) >= cs;
            const uint64_t pc = lane == 0 ? (B0 >> 4) : (B1 >> 4);
            if ((lane == 0 && ph) || (lane == 1 && pt && !(ph && (B1 >> 4) == (B0 >> 4)))) {
                uint32_t w[4];
                mixed_chunk(L, noff, XB + cnt, XB, ((int64_t)(pc << 4) - (int64_t)B0) * 8, T, w);
                store_bytes(A, pc << 4, B0, B1, w);
            }
        }
    } else {
        /* generic byte path: the bytes of every own run-layout NAL, one
         * byte per lane; serial-path and dynamic-rect NALs are written by
         * their own writers (below / k_dyn_gather) */
        const Lay *Lo = L + XB;
        const int32_t *no = noff + XB;
        for (int jn = 0; jn < cnt; ++jn) {
            if ((slow_mask >> (XB + jn)) & 1ull) continue;
            const uint32_t r0 = (uint32_t)no[jn], r1 = (uint32_t)no[jn + 1];
            for (uint32_t rel = r0 + (uint32_t)lane; rel < r1; rel += 64) {
                int jj = jn;
                A[B0 + rel] = (uint8_t)tile_byte(Lo, no, cnt, jj, rel);
            }
        }
    }
    mark(4);
    if (stamps && lane == 0) {
        uint64_t hw = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);      /* HW_ID */
        uint64_t xcc = (uint32_t)__builtin_amdgcn_s_getreg((15 << 11) | 20);    /* XCC_ID */
        stamp[7] = (__builtin_amdgcn_s_memrealtime() & 0xffffffffull) | (hw << 32);
        stamp[6] = (stamp[6] & 0x00ffffffffffffffull) | ((xcc & 0xff) << 56);
    }
    if (own && d.slow == 1) serial_write(my_ctx, A + d.out_off);
}

}  // namespace

/* ------------------------ host delivery (PCIe) ----------------------------- */
/* The reference hands its bytes over in host memory (composer.c:255-291).
 * scroll_batch_output_to_host_async packs the bytes appended to every stream
 * since its previous delivery (DevStream.undelivered) into pinned host memory, device-side and asynchronously: one
 * workgroup scans the streams' byte counts (16-byte aligned offsets) into the
 * host table, then every stream's bytes are read from its arena and stored
 * straight into the pinned buffer by (8, S) workgroups of 16-byte chunks --
 * no host sync between the compose and the copy, and the host never needs
 * the sizes before the bytes land.  (extern "C": the library exports the two
 * kernels under their plain names) */
extern "C" {
namespace {
constexpr int OUT_Z = 8;
__global__ __launch_bounds__(1024) void k_out_table(DevStream *__restrict__ st, int S, uint64_t cap,
                                                    uint64_t *__restrict__ dtab, uint64_t *__restrict__ htab)
{
    __shared__ uint64_t s_w[16], s_carry;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (int s0 = 0; s0 < S; s0 += 1024) {
        const int s = s0 + t;
        const uint64_t n = s < S ? st[s].undelivered : 0, a = (n + 15) & ~(uint64_t)15;
        const uint64_t inc = wave_incl_scan(a, lane);
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint64_t before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_w[w];
        if (s < S) {
            dtab[1 + 2 * (size_t)s] = htab[1 + 2 * (size_t)s] = before + inc - a;
            dtab[2 + 2 * (size_t)s] = htab[2 + 2 * (size_t)s] = n;
        }
        __syncthreads();
        if (t == 0)
            for (int w = 0; w < 16; ++w) s_carry += s_w[w];
        __syncthreads();
    }
    if (t == 0) {
        /* total: its aligned size, or ~0 when it does not fit (nothing copied,
         * the bytes stay undelivered) */
        const uint64_t tot = s_carry <= cap ? s_carry : ~(uint64_t)0;
        dtab[0] = htab[0] = tot;
    }
    if (s_carry <= cap)
        for (int s = t; s < S; s += 1024) st[s].undelivered = 0;
}

/* grid (OUT_Z, S): stream s's last-compose bytes -> dst + its offset, one
 * 16-byte chunk per thread and iteration: two aligned arena loads and a
 * byte funnel shift (bytes past n are don't-care: the table has n) */
__global__ __launch_bounds__(256) void k_out_copy(const DevStream *__restrict__ st, const uint8_t *__restrict__ arena,
                                                  uint64_t ld_arena, uint64_t arena_end,
                                                  const uint64_t *__restrict__ dtab, uint8_t *__restrict__ dst)
{
    const int s = blockIdx.y;
    if (dtab[0] == ~(uint64_t)0) return;
    const uint64_t n = dtab[2 + 2 * (size_t)s], o = dtab[1 + 2 * (size_t)s];
    const uint64_t from = (uint64_t)s * ld_arena + st[s].out_pos - n;   /* arena byte of the first new byte */
    uint4 *d = reinterpret_cast<uint4 *>(dst + o);
    const uint32_t q = (uint32_t)(from & 15u) >> 2, rb = (uint32_t)from & 3u;
    const uint64_t base = from & ~(uint64_t)15;
    const uint4 *a = reinterpret_cast<const uint4 *>(arena + base);
    const uint64_t nch = (n + 15) / 16;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < nch; j += (uint64_t)OUT_Z * 256) {
        const uint4 x = a[j];
        const uint4 y = (q | rb) && base + 16 * (j + 2) <= arena_end ? a[j + 1] : x;
        const uint32_t w0 = x.x, w1 = x.y, w2 = x.z, w3 = x.w, w4 = y.x, w5 = y.y, w6 = y.z, w7 = y.w;
        /* word k of the output = bytes 4 (q + k) + rb .. of w[] */
        auto pick = [&](uint32_t i) -> uint32_t {        /* w[i], i <= 7, by selects */
            const uint32_t lo = i & 1u ? (i & 2u ? w3 : w1) : (i & 2u ? w2 : w0);
            const uint32_t hi = i & 1u ? (i & 2u ? w7 : w5) : (i & 2u ? w6 : w4);
            return i & 4u ? hi : lo;
        };
        uint32_t o4[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t lo = pick(q + k), hi = pick(q + k + 1u);
            o4[k] = rb ? __builtin_amdgcn_alignbyte(hi, lo, rb) : lo;
        }
        d[j] = make_uint4(o4[0], o4[1], o4[2], o4[3]);
    }
}
}  // namespace
}  // extern "C"

/* ---------------------------------------------------------------------- */
/* launchers (scroll_engine.h)                                             */
/* ---------------------------------------------------------------------- */
void scroll_launch_plan(hipStream_t hs, int S, DevStream *st, const int32_t *offs, int ld_off, NalDesc *nal,
                        int ld_nal, int nframes, int mode, int flags, PlanPending *pend, DynFrame *dfr, int ld_fr,
                        const uint32_t *pool_ctr, uint32_t spill_cap, uint32_t gen_cap, uint32_t *ctr_zero,
                        const uint32_t *dpos)
{
    hipLaunchKernelGGL(k_plan, dim3(S), dim3(PLAN_THREADS), 0, hs, st, offs, ld_off, nal, ld_nal, nframes, mode,
                       flags, pend, dfr, ld_fr, pool_ctr, spill_cap, gen_cap, ctr_zero, dpos);
}

static int emit_gx(int nal_max)
{
    const int per_wg = EMIT_WAVES * TILE;
    return (nal_max + per_wg - 1) / per_wg;
}

size_t scroll_emit_stamp_slots(int nal_max, int S)
{
    const int gx = emit_gx(nal_max);
    return gx > 0 ? (size_t)gx * S * EMIT_WAVES : 0;
}

void scroll_launch_emit(hipStream_t hs, int S, int nal_max, const DevStream *st, const NalDesc *nal, int ld_nal,
                        uint8_t *arena, uint64_t ld_arena, int flags, uint64_t *dbg)
{
    const int gx = emit_gx(nal_max);
    if (gx > 0)
        hipLaunchKernelGGL(k_emit, dim3(gx, S), dim3(EMIT_WAVES * 64), 0, hs, st, nal, ld_nal, arena, ld_arena,
                           flags, dbg);
}

void scroll_launch_out_table(hipStream_t hs, DevStream *st, int S, uint64_t cap, uint64_t *dtab, uint64_t *htab)
{
    hipLaunchKernelGGL(k_out_table, dim3(1), dim3(1024), 0, hs, st, S, cap, dtab, htab);
}

void scroll_launch_out_copy(hipStream_t hs, const DevStream *st, int S, const uint8_t *arena, uint64_t ld_arena,
                            uint64_t arena_end, const uint64_t *dtab, uint8_t *dst)
{
    hipLaunchKernelGGL(k_out_copy, dim3(OUT_Z, (unsigned)S), dim3(256), 0, hs, st, arena, ld_arena, arena_end, dtab,
                       dst);
}
