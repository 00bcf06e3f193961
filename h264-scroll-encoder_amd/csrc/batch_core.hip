/*
 * batch_core.hip -- the batch engine behind include/composer_batch.h: create
 * and destroy, streams and offsets, the per-step path (launch, compose,
 * sync), output and host delivery, NAL info and timing.  The features a
 * compose drives live beside it (batch.h has the map).
 */
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "batch.h"
#include "scroll_engine.h"
#include "dyn_engine.h"
#include "recon_engine.h"
#include "hrecon_engine.h"
#include "hint_engine.h"
#include "splice_engine.h"
#include "hdyn_engine.h"

using namespace scroll::batch;

/* event pairs of one compose.  Dynamic rect: plan = [0,1) + [2,3), dyn
 * stage [1,2), emit [3,4), dyn emit [4,5).  Otherwise only events 0, 1, 4
 * are recorded (fewer markers between the kernels): plan [0,1), emit [1,4).
 * lite (scroll_batch_enable_timing(b, 2)): only the dominant kernel's pair,
 * dyn code [1,6) (reported as dyn stage too) or emit [1,4) -- each event
 * record is a marker packet that holds the queue for microseconds, so the
 * full set costs a timed step ~ 40 us of gaps between its kernels */
static void event_ms(const hipEvent_t *e, bool dyn, bool lite, float out[6])
{
    auto el = [&](int a, int b) {
        float v = 0.0f;
        return hipEventElapsedTime(&v, e[a], e[b]) == hipSuccess ? v : 0.0f;
    };
    if (lite) {
        for (int k = 0; k < 6; ++k) out[k] = 0.0f;
        if (dyn) out[2] = out[4] = el(1, 6);
        else out[1] = el(1, 4);
        return;
    }
    if (dyn) {
        out[0] = el(0, 1) + el(2, 3);
        out[1] = el(3, 4);
        out[2] = el(1, 2);
        out[3] = el(4, 5);
        out[4] = el(1, 6);
        out[5] = el(6, 2);
    } else {
        out[0] = el(0, 1);
        out[1] = el(1, 4);
        out[2] = out[3] = out[4] = out[5] = 0.0f;
    }
}

static void fold_ring(ScrollBatch *b)
{
    for (int i = 0; i + NEV <= b->ring_used; i += NEV) {
        float m[6];
        event_ms(&b->ring[i], (b->ring_dyn[i / NEV] & 1) != 0, (b->ring_dyn[i / NEV] & 2) != 0, m);
        for (int k = 0; k < 6; ++k) b->acc_ms[k] += m[k];
        b->acc_n++;
    }
    b->ring_used = 0;
}

static int ring_events(ScrollBatch *b, hipEvent_t **evs)
{
    if ((size_t)b->ring_used + NEV > b->ring.size()) {
        if (b->ring.size() >= (size_t)NEV * 256) {   /* bound: fold pending timings first */
            HIPCHK(hipStreamSynchronize(b->last));
            fold_ring(b);
        } else {
            for (int i = 0; i < NEV; ++i) {
                hipEvent_t e;
                HIPCHK(timing_event(&e));
                b->ring.push_back(e);
            }
            b->ring_dyn.push_back(0);
        }
    }
    *evs = &b->ring[b->ring_used];
    b->ring_used += NEV;
    return SCROLL_OK;
}

/* b->d_dbg with room for `slots` 8-word debug stamps, zeroed on hs */
static int dbg_stamps(ScrollBatch *b, size_t slots, hipStream_t hs)
{
    if (slots > b->dbg_slots) {
        if (b->d_dbg) (void)hipFree(b->d_dbg);
        HIPCHK(hipMalloc(&b->d_dbg, slots * 8 * sizeof(uint64_t)));
        b->dbg_slots = slots;
    }
    HIPCHK(hipMemsetAsync(b->d_dbg, 0, slots * 8 * sizeof(uint64_t), hs));
    return SCROLL_OK;
}

/* the reconstruction's timing pair (created on first use) */
static int rc_events(ScrollBatch *b)
{
    if (!b->rc_ev[0]) {
        HIPCHK(hipEventCreate(&b->rc_ev[0]));
        HIPCHK(hipEventCreate(&b->rc_ev[1]));
    }
    return SCROLL_OK;
}

namespace scroll {
namespace batch {

static thread_local char g_err[512];

void set_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int usable_devices(std::vector<int> *ids)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_err("no HIP device visible (libh264scroll needs an MI355X / gfx950)");
        return 0;
    }
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) != hipSuccess) continue;
        if (strncmp(p.gcnArchName, "gfx950", 6) == 0) {
            ok++;
            if (ids) ids->push_back(i);
        }
    }
    if (!ok) set_err("no gfx950 device among %d HIP devices", n);
    return ok;
}

int check_cfg(const ComposerConfig *c)
{
    if (c->log2_max_frame_num < 1 || c->log2_max_frame_num > 16 ||
        (c->pic_order_cnt_type == 0 &&
         (c->log2_max_pic_order_cnt_lsb < 1 || c->log2_max_pic_order_cnt_lsb > 16)) ||
        c->num_waypoints < 0 || c->num_waypoints > MAX_WAYPOINTS || c->width < 0 ||
        c->height < 0) {
        set_err("unsupported ComposerConfig (log2 fields must be 1..16, num_waypoints 0..8)");
        return SCROLL_ERR_CONFIG;
    }
    return SCROLL_OK;
}

void cfg_to_dev(const ComposerConfig *c, DevStream *d)
{
    d->w = c->width;
    d->h = c->height;
    d->log2_mfn = c->log2_max_frame_num;
    d->poc_type = c->pic_order_cnt_type;
    d->log2_poc = c->log2_max_pic_order_cnt_lsb;
    d->deblock = c->deblocking_filter_control_present_flag;
    d->frame_num = c->frame_num;
    d->nwp = c->num_waypoints;
    for (int i = 0; i < 8; ++i) {
        d->wp_off[i] = c->waypoints[i].offset_px;
        d->wp_lt[i] = c->waypoints[i].long_term_idx;
        d->wp_valid[i] = c->waypoints[i].valid;
    }
}

void dev_to_cfg(const DevStream *d, ComposerConfig *c)
{
    c->frame_num = d->frame_num;
    c->num_waypoints = d->nwp;
    for (int i = 0; i < 8; ++i) {
        c->waypoints[i].offset_px = d->wp_off[i];
        c->waypoints[i].long_term_idx = d->wp_lt[i];
        c->waypoints[i].valid = d->wp_valid[i];
    }
}

/* timing-only events: no system-scope fence on record (no cache writeback /
 * invalidate between the kernels being timed) */
hipError_t timing_event(hipEvent_t *e)
{
    return hipEventCreateWithFlags(e, hipEventDisableSystemFence);
}

int hip_fail(const char *who, hipError_t e, bool clear)
{
    set_err("%s: %s", who, hipGetErrorString(e));
    if (clear) (void)hipGetLastError();
    return e == hipErrorOutOfMemory ? SCROLL_ERR_OOM : SCROLL_ERR_HIP;
}

/* grow a device buffer to n elements of `size` bytes (contents dropped) */
int dev_grow(void **p, size_t *cap, size_t n, size_t size, const char *who)
{
    if (n <= *cap) return SCROLL_OK;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc(p, std::max<size_t>(n, 1) * size);
    if (e != hipSuccess) return hip_fail(who, e);
    *cap = n;
    return SCROLL_OK;
}

int batch_host_sync(ScrollBatch *b)
{
    if (b->host_valid) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->last));
    HIPCHK(hipMemcpy(b->h_st, b->d_st, (size_t)b->nstreams * sizeof(DevStream),
                     hipMemcpyDeviceToHost));
    b->host_valid = 1;
    return SCROLL_OK;
}

int launch(ScrollBatch *b, int nframes, int plan_mode, int nal_max, hipStream_t hs, int plan_flags)
{
    int S = b->nstreams;
    if (S == 0) return SCROLL_OK;
    hipEvent_t *rev = nullptr;
    if (b->timing) {
        int rc = ring_events(b, &rev);
        if (rc) return rc;
    }
    const bool hint = b->hint_on && plan_mode != SCROLL_PLAN_EXPLICIT;
    const bool dyn = (b->dyn_on || hint) && plan_mode != SCROLL_PLAN_EXPLICIT;   /* staged NALs */
    const bool lite = b->timing == 2;
    /* lite with the row coder: its pair goes right around k_dyn_row
     * (dyn_launch_code), not around the whole code step */
    const bool lite_row = lite && dyn && !hint;
    auto mark = [&](int k) -> int {
        if (!b->timing || (!dyn && k != 0 && k != 1 && k != 4)) return SCROLL_OK;
        if (lite) {                     /* the dominant kernel's pair, ring only */
            if ((k == 1 || k == (dyn ? 6 : 4)) && !lite_row) HIPCHK(hipEventRecord(rev[k], hs));
            return SCROLL_OK;
        }
        HIPCHK(hipEventRecord(b->ev[k], hs));
        HIPCHK(hipEventRecord(rev[k], hs));
        return SCROLL_OK;
    };
    if (b->timing) {
        b->ring_dyn[(b->ring_used - NEV) / NEV] = (uint8_t)((dyn ? 1 : 0) | (lite ? 2 : 0));
        if (!lite) b->ev_dyn = dyn ? 1 : 0;
    }
    const int ld_fr = b->max_frames;
    /* k_plan's own flags start at PLAN_REWIND: the debug bits from there up
     * (SCROLL_DEBUG_DYN_STAMPS is the same bit) are not for it */
    const int plan_debug = b->debug & (PLAN_REWIND - 1);
    int rc = mark(0);
    if (rc) return rc;
    if (!dyn) {
        scroll_launch_plan(hs, S, b->d_st, b->d_off, b->max_frames, b->d_nal, b->ld_nal, nframes, plan_mode,
                           plan_debug | plan_flags, b->d_pend, b->d_dfr, ld_fr);
        HIPCHK(hipGetLastError());
        if ((rc = mark(1)) || (rc = mark(2)) || (rc = mark(3))) return rc;
    } else {
        const bool dyn_rect = b->dyn_on && !hint;
        /* moving rects: the position table for this compose's kernels (NULL: none set, or hints) */
        b->geo.dpos = nullptr;
        if (dyn_rect && b->dyn_moving && (rc = dyn_pos_table(b, hs, &b->geo.dpos))) return rc;
        scroll_launch_plan(hs, S, b->d_st, b->d_off, b->max_frames, b->d_nal, b->ld_nal, nframes, plan_mode,
                           plan_debug | plan_flags | PLAN_STATE | PLAN_DYN, b->d_pend, b->d_dfr,
                           ld_fr, nullptr, 0u, 0u, dyn_rect ? b->dx.ctr : nullptr, b->geo.dpos);
        HIPCHK(hipGetLastError());
        if ((rc = mark(1))) return rc;
        uint64_t *stamps = nullptr;
        if (b->debug & SCROLL_DEBUG_DYN_STAMPS) {   /* k_dyn_emit_gather's, then k_dyn_group's */
            const size_t slots = (2 + (size_t)b->geo.ld_groups) * (size_t)nframes * S;
            if ((rc = dbg_stamps(b, slots, hs))) return rc;
            stamps = b->d_dbg + 2 * (size_t)nframes * S * 8;
        }
        b->geo.debug = b->debug;
        if (hint) {
            if (b->sp_parse) {
                if (splice_launch_parse(hs, b->sp_n, b->sp_ymax, b->d_sp_list, b->d_spf, b->d_sp_units,
                                        b->d_sp_lanes, b->sp_nslots, b->d_st, ld_fr, b->d_sp_rbsp, b->d_sp_rec)) {
                    set_err("k_splice_parse launch: %s", hipGetErrorString(hipGetLastError()));
                    return SCROLL_ERR_HIP;
                }
                b->sp_parse = 0;
            }
            if (b->fallback && b->dyn_on &&
                hint_launch_fb(hs, nframes, S, b->d_st, b->d_nal, b->ld_nal, b->d_pend, b->d_dfr, ld_fr,
                               b->d_hf, b->d_pool)) {
                set_err("k_hint_fb launch: %s", hipGetErrorString(hipGetLastError()));
                return SCROLL_ERR_HIP;
            }
            if (hint_launch_stage(hs, nframes, S, b->d_st, b->d_nal, b->ld_nal, b->d_pend,
                                  b->d_dfr, ld_fr, b->d_hf, b->d_pool, b->d_stage,
                                  b->geo.slot_bytes)) {
                set_err("k_hint_stage launch: %s", hipGetErrorString(hipGetLastError()));
                return SCROLL_ERR_HIP;
            }
            const bool combined = b->dyn_on;
            if (combined &&
                hdyn_launch_code(hs, nframes, S, b->d_st, b->d_nal, b->ld_nal, b->d_pend, b->d_dfr, ld_fr,
                                 b->d_hf, b->d_pool, b->d_spf, &b->geo, b->d_src, b->d_refs,
                                 b->d_sp_rec, b->d_sp_rbsp, b->hd_mb_words)) {
                set_err("k_hdyn_code launch: %s", hipGetErrorString(hipGetLastError()));
                return SCROLL_ERR_HIP;
            }
            if (combined && b->recon_on && b->recon_hinted) {
                /* the decoded rects + their squared error at the hinted
                 * motion, beside k_hdyn_code (after k_hint_fb: it reads the
                 * frames' fallback bits) */
                const bool timed = b->timing != 0;
                if (timed && (rc = rc_events(b))) return rc;
                if (hrecon_launch(hs, nframes, S, b->d_st, b->d_nal, b->ld_nal, b->d_pend, b->d_dfr, ld_fr,
                                  b->d_hf, b->d_pool, b->d_spf, &b->geo, b->d_src, b->d_refs, b->d_rec, b->d_sse,
                                  timed ? b->rc_ev[0] : nullptr, timed ? b->rc_ev[1] : nullptr)) {
                    set_err("k_hdyn_recon launch: %s", hipGetErrorString(hipGetLastError()));
                    return SCROLL_ERR_HIP;
                }
                b->rc_timed = timed ? 1 : 0;
                b->rc_last_hint = 1;
                std::fill(b->rc_fail.begin(), b->rc_fail.end(), 0);
            }
            if ((b->sp_n > 0 || combined) &&
                splice_launch_stage(hs, nframes, S, b->d_st, b->d_nal, b->ld_nal, b->d_pend,
                                    b->d_dfr, ld_fr, b->d_hf, b->d_pool, b->d_spf, b->d_sp_rec,
                                    b->d_sp_rbsp, b->d_stage, b->geo.slot_bytes)) {
                set_err("k_splice_stage launch: %s", hipGetErrorString(hipGetLastError()));
                return SCROLL_ERR_HIP;
            }
            if ((rc = mark(6))) return rc;
        } else {
            b->dx.epoch = b->dx.epoch % 0xffffffu + 1u;    /* look-back epoch, never 0 */
            /* (a pipeline over stream chunks, the coder of one chunk beside the
             * packing of the one before on a second HIP stream, measured slower
             * at 2 / 4 / 8 chunks: DESIGN.md §6; the device-side frame lists
             * are batch-wide, so the launches below cover the whole batch) */
            const DynGeom &G = b->geo;
            /* SCROLL_DYN_FORK=1: the general path and the static groups on a
             * second stream beside k_dyn_row (created on first use) */
            const DynFork *fk = nullptr;
            static const bool fork_on = [] {
                const char *e = getenv("SCROLL_DYN_FORK");
                return e && e[0] == '1';
            }();
            if (fork_on) {
                if (!b->fork.side) {
                    HIPCHK(hipStreamCreateWithFlags(&b->fork.side, hipStreamNonBlocking));
                    HIPCHK(hipEventCreateWithFlags(&b->fork.e0, hipEventDisableTiming));
                    HIPCHK(hipEventCreateWithFlags(&b->fork.e1, hipEventDisableTiming));
                }
                fk = &b->fork;
            }
            if (dyn_launch_code(hs, nframes, S, b->d_st, b->d_nal, b->ld_nal, b->d_pend, b->d_dfr, ld_fr, &G,
                                b->d_src, b->d_refs, &b->dx, b->dx.epoch, b->dyn_pw / 16, stamps, fk,
                                lite_row ? rev[1] : nullptr, lite_row ? rev[6] : nullptr)) {
                set_err("k_dyn_code launch: %s", hipGetErrorString(hipGetLastError()));
                return SCROLL_ERR_HIP;
            }
            if ((rc = mark(6))) return rc;
            if (b->recon_on) {
                /* the decoded rects + their squared error, from k_dyn_rows'
                 * rows on the launch stream (independent of k_dyn_row) */
                const bool timed = b->timing != 0;
                if (timed && (rc = rc_events(b))) return rc;
                if (recon_launch(hs, nframes, S, b->d_st, b->d_nal, b->ld_nal, b->d_pend, b->d_dfr, ld_fr, &G,
                                 b->dx.rows, b->d_src, b->d_refs, b->d_rec, b->d_sse, b->dx.ctr,
                                 timed ? b->rc_ev[0] : nullptr, timed ? b->rc_ev[1] : nullptr)) {
                    set_err("k_dyn_recon launch: %s", hipGetErrorString(hipGetLastError()));
                    return SCROLL_ERR_HIP;
                }
                b->rc_timed = timed ? 1 : 0;
                b->rc_last_hint = 0;
            }
            if (dyn_launch_pack(hs, nframes, S, b->d_st, b->d_nal, b->ld_nal, b->d_pend, b->d_dfr, ld_fr, &G,
                                &b->dx, b->d_stage, stamps ? b->d_dbg : nullptr, fk)) {
                set_err("k_dyn_static / k_dyn_epfix launch: %s", hipGetErrorString(hipGetLastError()));
                return SCROLL_ERR_HIP;
            }
        }
        if ((rc = mark(2))) return rc;
        scroll_launch_plan(hs, S, b->d_st, b->d_off, b->max_frames, b->d_nal, b->ld_nal, nframes, plan_mode,
                           plan_debug | plan_flags | PLAN_SIZE | PLAN_DYN, b->d_pend, b->d_dfr,
                           ld_fr, (b->dyn_on && !b->hint_on) ? (const uint32_t *)b->dx.ctr : nullptr,
                           b->geo.rs_spill_cap, b->geo.gen_cap, nullptr, b->geo.dpos);
        HIPCHK(hipGetLastError());
        if ((rc = mark(3))) return rc;
    }
    const size_t slots = scroll_emit_stamp_slots(nal_max, S);   /* 0: no NAL, no launch */
    if (slots && (b->debug & SCROLL_DEBUG_EMIT_STAMPS) && (rc = dbg_stamps(b, slots, hs))) return rc;
    scroll_launch_emit(hs, S, nal_max, b->d_st, b->d_nal, b->ld_nal, b->d_arena, (uint64_t)b->ld_arena, b->debug,
                       b->d_dbg);
    HIPCHK(hipGetLastError());
    if ((rc = mark(4))) return rc;
    if (dyn && dyn_launch_emit(hs, nframes, S, b->d_st, b->d_nal, b->ld_nal, b->d_dfr, ld_fr,
                               &b->geo, b->d_stage, hint ? nullptr : &b->dx, b->d_arena,
                               (uint64_t)b->ld_arena,
                               (b->debug & SCROLL_DEBUG_DYN_STAMPS) && b->d_dbg
                                   ? b->d_dbg + (size_t)nframes * S * 8 : nullptr)) {
        set_err("k_dyn_gather launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    if ((rc = mark(5))) return rc;
    if (b->timing == 1) b->timed_pending = 1;
    b->host_valid = 0;
    b->nal_cache_valid = 0;
    b->last = hs;
    return SCROLL_OK;
}

/* the status scroll_batch_sync gives for stream s's pending error bits */
int stream_fail_code(ScrollBatch *b, int s)
{
    const int32_t e = b->h_st[s].err;
    if (!e) return SCROLL_OK;
    if (e & SCROLL_DEVERR_HANDOFF) return SCROLL_ERR_DEVICE;
    if (e & SCROLL_DEVERR_SPLICE) {
        int st = 0;
        for (int ff = 0; ff < b->max_frames && !st; ++ff)
            if (splice_frame_status(b, (size_t)s * b->max_frames + ff, &st)) break;
        return st == HDYN_STATUS_OVERFLOW ? SCROLL_ERR_OVERFLOW : SCROLL_ERR_CONFIG;
    }
    if (e & SCROLL_DEVERR_HINT) return SCROLL_ERR_CONFIG;
    return SCROLL_ERR_OVERFLOW;
}

int load_nals(ScrollBatch *b)
{
    if (b->nal_cache_valid) return SCROLL_OK;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    b->nal_cache.resize((size_t)b->nstreams * b->ld_nal);
    HIPCHK(hipMemcpy(b->nal_cache.data(), b->d_nal, b->nal_cache.size() * sizeof(NalDesc),
                     hipMemcpyDeviceToHost));
    b->nal_cache_valid = 1;
    return SCROLL_OK;
}

}  // namespace batch
}  // namespace scroll

extern "C" {

const char *scroll_last_error(void) { return g_err; }

const char *scroll_version(void) { return "h264scroll-amd 0.1 (gfx950)"; }

int scroll_device_count(void) { return usable_devices(nullptr); }

int scroll_batch_create(ScrollBatch **out, const ScrollBatchDesc *desc)
{
    if (!out || !desc || desc->max_streams <= 0 || desc->max_frames <= 0 ||
        desc->arena_bytes == 0 ||
        (desc->mode != SCROLL_MODE_COMPOSER && desc->mode != SCROLL_MODE_EXPERIMENT)) {
        set_err("scroll_batch_create: bad descriptor");
        return SCROLL_ERR_ARG;
    }
    *out = nullptr;
    std::vector<int> ids;
    if (!usable_devices(&ids)) return SCROLL_ERR_NO_DEVICE;
    int n = 0;
    (void)hipGetDeviceCount(&n);
    if (desc->device < 0 || desc->device >= n) {
        set_err("scroll_batch_create: device %d out of range (%d visible)", desc->device, n);
        return SCROLL_ERR_ARG;
    }
    bool ok = false;
    for (int i : ids) ok |= (i == desc->device);
    if (!ok) {
        set_err("scroll_batch_create: device %d is not gfx950", desc->device);
        return SCROLL_ERR_NO_DEVICE;
    }
    HIPCHK(hipSetDevice(desc->device));
    ScrollBatch *b = new ScrollBatch();
    b->device = desc->device;
    b->mode = desc->mode;
    b->max_streams = desc->max_streams;
    b->max_frames = desc->max_frames;
    b->arena_bytes = desc->arena_bytes;
    /* >= 128 B slack past out_cap: k_emit writes whole 128-byte lines and
     * zero-fills the tail of a stream's last line */
    b->ld_arena = (desc->arena_bytes + 128 + 255) & ~(size_t)255;
    b->ld_nal = 2 * desc->max_frames;
    size_t S = (size_t)desc->max_streams;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMalloc(&b->d_st, S * sizeof(DevStream));
    if (e == hipSuccess) e = hipHostMalloc(&b->h_st, S * sizeof(DevStream), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&b->d_off, S * (size_t)desc->max_frames * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&b->d_nal, S * (size_t)b->ld_nal * sizeof(NalDesc));
    if (e == hipSuccess) e = hipMalloc(&b->d_arena, S * b->ld_arena);
    if (e == hipSuccess) e = hipMalloc(&b->d_pend, S * sizeof(PlanPending));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->own, hipStreamNonBlocking);
    for (int i = 0; i < NEV && e == hipSuccess; ++i) e = timing_event(&b->ev[i]);
    if (e == hipSuccess) e = hipMemset(b->d_st, 0, S * sizeof(DevStream));
    if (e == hipSuccess) e = hipMemset(b->d_off, 0, S * (size_t)desc->max_frames * sizeof(int32_t));
    if (e != hipSuccess) {
        scroll_batch_destroy(b);
        return hip_fail("scroll_batch_create", e);
    }
    memset(b->h_st, 0, S * sizeof(DevStream));
    b->last = b->own;
    *out = b;
    return SCROLL_OK;
}

void scroll_batch_destroy(ScrollBatch *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->own) (void)hipStreamSynchronize(b->own);
    for (int i = 0; i < NEV; ++i)
        if (b->ev[i]) (void)hipEventDestroy(b->ev[i]);
    for (hipEvent_t e : b->ring) (void)hipEventDestroy(e);
    if (b->fork.side) {
        (void)hipStreamSynchronize(b->fork.side);
        (void)hipStreamDestroy(b->fork.side);
        (void)hipEventDestroy(b->fork.e0);
        (void)hipEventDestroy(b->fork.e1);
    }
    if (b->own) (void)hipStreamDestroy(b->own);
    (void)hipFree(b->d_st);
    (void)hipHostFree(b->h_st);
    (void)hipFree(b->d_off);
    (void)hipFree(b->d_nal);
    (void)hipFree(b->d_arena);
    (void)hipFree(b->d_out_tab);
    (void)hipFree(b->d_upd);
    if (b->out_ev) (void)hipEventDestroy(b->out_ev);
    (void)hipFree(b->d_pend);
    (void)hipFree(b->d_dfr);
    (void)hipFree(b->d_src);
    (void)hipFree(b->d_refs);
    (void)hipFree(b->d_stage);
    (void)hipFree(b->d_rec);
    (void)hipFree(b->d_sse);
    for (hipEvent_t e : b->rc_ev)
        if (e) (void)hipEventDestroy(e);
    probe_release(b);
    locate_release(b);
    mask_release(b);
    detect_release(b);
    (void)hipFree(b->dx.qpf);
    rate_release(b);
    surface_release(b, true);
    (void)hipFree(b->d_hf);
    (void)hipFree(b->d_pool);
    (void)hipFree(b->d_spf);
    (void)hipFree(b->d_sp_nal);
    (void)hipFree(b->d_sp_rbsp);
    (void)hipFree(b->d_sp_rec);
    (void)hipFree(b->d_sp_list);
    (void)hipFree(b->d_sp_units);
    (void)hipFree(b->d_sp_lanes);
    (void)hipFree(b->d_ing_in);
    (void)hipFree(b->d_ipcm_cnt);
    (void)hipFree(b->d_ipcm_stg);
    (void)hipFree(b->d_ipcm_hw);
    (void)hipFree(b->d_ing_files);
    (void)hipFree(b->d_ing_scan);
    (void)hipFree(b->d_ing_out);
    (void)hipFree(b->d_ing_work);
    for (hipEvent_t e : b->ing_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : b->ipcm_ev)
        if (e) (void)hipEventDestroy(e);
    (void)hipFree(b->d_ipcm_sticky);
    if (b->d_dbg) (void)hipFree(b->d_dbg);
    delete b;
}

int scroll_batch_num_streams(const ScrollBatch *b) { return b ? b->nstreams : 0; }

int scroll_batch_set_debug(ScrollBatch *b, int flags)
{
    if (!b) return SCROLL_ERR_ARG;
    b->debug = flags;
    return SCROLL_OK;
}

int scroll_batch_add_stream(ScrollBatch *b, const ComposerConfig *cfg)
{
    if (!b || !cfg) return SCROLL_ERR_ARG;
    if (b->nstreams >= b->max_streams) {
        set_err("scroll_batch_add_stream: batch full (%d streams)", b->max_streams);
        return SCROLL_ERR_ARG;
    }
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (b->dyn_on && (cfg->width != b->dyn_pw || cfg->height != b->dyn_ph)) {
        set_err("scroll_batch_add_stream: the dynamic rect needs %dx%d streams", b->dyn_pw,
                b->dyn_ph);
        return SCROLL_ERR_CONFIG;
    }
    if (b->hint_on && ((cfg->width / 16) * (cfg->height / 16) > b->hint_max_mb ||
                       cfg->width / 16 > HINT_MAX_MBW)) {
        set_err("scroll_batch_add_stream: hint staging slots hold %d MBs per picture, %d per row",
                b->hint_max_mb, HINT_MAX_MBW);
        return SCROLL_ERR_CONFIG;
    }
    rc = batch_host_sync(b);
    if (rc) return rc;
    int s = b->nstreams;
    DevStream *d = &b->h_st[s];
    if (b->dyn_qp != 26 && !cfg->deblocking_filter_control_present_flag) {
        set_err("scroll_batch_add_stream: a stream with the deblocking filter on (no "
                "deblocking_filter_control_present_flag) needs the rect at QP 26, the batch's is %d",
                b->dyn_qp);
        return SCROLL_ERR_CONFIG;
    }
    memset(d, 0, sizeof(*d));
    cfg_to_dev(cfg, d);
    d->dyn_qp = b->dyn_qp;
    d->out_pos = 0;
    d->out_cap = b->arena_bytes;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpy(b->d_st + s, d, sizeof(DevStream), hipMemcpyHostToDevice));
    b->nstreams++;
    return s;
}

int scroll_batch_get_config(ScrollBatch *b, int s, ComposerConfig *cfg)
{
    if (!b || !cfg || s < 0 || s >= b->nstreams) return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    const DevStream *d = &b->h_st[s];
    composer_config_init(cfg, d->w, d->h);
    cfg->log2_max_frame_num = d->log2_mfn;
    cfg->pic_order_cnt_type = d->poc_type;
    cfg->log2_max_pic_order_cnt_lsb = d->log2_poc;
    cfg->deblocking_filter_control_present_flag = d->deblock;
    dev_to_cfg(d, cfg);
    return SCROLL_OK;
}

int scroll_batch_set_config(ScrollBatch *b, int s, const ComposerConfig *cfg)
{
    if (!b || !cfg || s < 0 || s >= b->nstreams) return SCROLL_ERR_ARG;
    int rc = check_cfg(cfg);
    if (rc) return rc;
    rc = batch_host_sync(b);
    if (rc) return rc;
    DevStream *d = &b->h_st[s];
    if (!cfg->deblocking_filter_control_present_flag) {
        /* the guard of add_stream / set_dyn_qp*: the loop filter on keeps the
         * stream's rect, and every per-frame rect QP of it, at 26 */
        bool bad = d->dyn_qp != 26;
        const size_t F = (size_t)b->max_frames, i0 = (size_t)s * F;
        for (size_t f = 0; !bad && f < F && i0 + f < b->h_dyn_qp.size(); ++f) {
            const int q = b->h_dyn_qp[i0 + f];
            bad = q >= 0 && q != 26;
        }
        bool any = false;                /* the plain rect's per-frame table too */
        if (!bad && b->dx.qpf && !qp_frames_any(b, &any))
            for (size_t f = 0; !bad && f < F; ++f) bad = b->h_qpf[i0 + f] != 0xFFu && b->h_qpf[i0 + f] != 26u;
        if (bad) {
            set_err("scroll_batch_set_config: stream %d's rect QP is not 26: it cannot turn the deblocking "
                    "filter on (no deblocking_filter_control_present_flag)", s);
            return SCROLL_ERR_CONFIG;
        }
    }
    cfg_to_dev(cfg, d);
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpy(b->d_st + s, d, sizeof(DevStream), hipMemcpyHostToDevice));
    return SCROLL_OK;
}

int scroll_batch_set_offsets(ScrollBatch *b, const int32_t *offsets, int nframes)
{
    if (!b || !offsets || nframes < 0 || nframes > b->max_frames) return SCROLL_ERR_ARG;
    if (nframes == 0 || b->nstreams == 0) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpy2D(b->d_off, (size_t)b->max_frames * sizeof(int32_t), offsets,
                       (size_t)nframes * sizeof(int32_t), (size_t)nframes * sizeof(int32_t),
                       (size_t)b->nstreams, hipMemcpyHostToDevice));
    return SCROLL_OK;
}

int32_t *scroll_batch_offsets_device(ScrollBatch *b) { return b ? b->d_off : nullptr; }

int scroll_batch_compose(ScrollBatch *b, int nframes, void *hip_stream)
{
    return scroll_batch_compose_ex(b, nframes, hip_stream, 0);
}

int scroll_batch_compose_ex(ScrollBatch *b, int nframes, void *hip_stream, int flags)
{
    if (!b || nframes < 0 || nframes > b->max_frames) {
        set_err("scroll_batch_compose: nframes %d out of range", nframes);
        return SCROLL_ERR_ARG;
    }
    if (b->dyn_on && !b->dyn_refs) {
        set_err("scroll_batch_compose: dynamic rect without reference pictures");
        return SCROLL_ERR_CONFIG;
    }
    HIPCHK(hipSetDevice(b->device));
    const bool combined = b->hint_on && b->dyn_on;
    /* located positions (scroll_batch_dyn_locate) that anything but the plain
     * moving rect's kernels is about to read: the host's copy first */
    if (b->dpos_dev && (b->hint_on || !b->dyn_moving)) {
        int rc = dyn_pos_refresh(b);
        if (rc) return rc;
    }
    if (combined && b->dsz_any) {
        /* (the host's copy is current: the refresh above) */
        set_err("scroll_batch_compose: a frame has a size of its own (scroll_batch_set_dyn_rect_size_at), which "
                "the rect under UI hints does not follow: clear the hints or the sizes");
        return SCROLL_ERR_CONFIG;
    }
    if (b->dyn_pos_custom && !b->hint_on && !b->dyn_moving) {
        set_err("scroll_batch_compose: per-frame dynamic rect positions need UI hints "
                "(scroll_batch_set_hints)");
        return SCROLL_ERR_CONFIG;
    }
    if (b->recon_on && b->hint_on) {
        /* hints and the fallback code the rect in k_hdyn_code /
         * k_splice_stage, which k_dyn_recon does not follow: k_hdyn_recon
         * does, once opted in; a spliced slice carries MB types neither decodes */
        bool spliced = b->sp_n > 0;
        for (const ScrollBatch::SpliceHost &sp : b->h_sp) spliced |= sp.w > 0;
        if (!b->recon_hinted || spliced) {
            set_err("scroll_batch_compose: the dynamic rect's reconstruction (scroll_batch_set_dyn_recon) "
                    "covers the plain dynamic rect, and the rect under UI hints with "
                    "scroll_batch_set_dyn_recon_hinted, never spliced slices: clear the hints / splices, opt "
                    "in or turn it off");
            return SCROLL_ERR_CONFIG;
        }
    }
    if (b->hint_on && b->dx.qpf) {
        /* the per-frame QP table is the plain rect's; under hints the frames' QPs are set_dyn_qp_at's */
        bool any = false;
        int rc = qp_frames_any(b, &any);
        if (rc) return rc;
        if (any) {
            set_err("scroll_batch_compose: per-frame rect QPs are set (scroll_batch_set_dyn_qp_frames / "
                    "scroll_batch_dyn_pick) and so are UI hints: clear one of them "
                    "(scroll_batch_clear_dyn_qp_frames; under hints: scroll_batch_set_dyn_qp_at)");
            return SCROLL_ERR_CONFIG;
        }
    }
    if (b->hint_on && b->sp_dirty) {
        int rc = splice_upload(b);
        if (rc) return rc;
        if (combined) b->hd_dirty = 1;
    }
    if (combined && b->hd_dirty) {
        int rc = hd_upload(b);
        if (rc) return rc;
    }
    if (b->hint_on && b->hint_dirty) {
        int rc = hint_upload(b);
        if (rc) return rc;
    }
    hipStream_t hs = hip_stream ? (hipStream_t)hip_stream : b->own;
    int plan = b->mode == SCROLL_MODE_EXPERIMENT ? SCROLL_PLAN_EXPERIMENT : SCROLL_PLAN_COMPOSER;
    int nal_max = plan == SCROLL_PLAN_COMPOSER ? 2 * nframes : nframes;
    b->last_plan_mode = plan;
    b->last_nframes = nframes;
    return launch(b, nframes, plan, nal_max, hs,
                  (flags & SCROLL_COMPOSE_REWIND) ? PLAN_REWIND : 0);
}

int scroll_batch_sync(ScrollBatch *b)
{
    if (!b) return SCROLL_ERR_ARG;
    {
        int rc0 = batch_host_sync(b);
        if (rc0) return rc0;
        if ((rc0 = ipcm_async_check(b))) return rc0;
    }
    if (b->timed_pending) {
        event_ms(b->ev, b->ev_dyn != 0, false, b->ms);
        b->timed_pending = 0;
    }
    int rc = SCROLL_OK;
    for (int s = 0; s < b->nstreams; ++s) {
        if (!b->h_st[s].err) continue;
        if (b->rc_last_hint && (size_t)s < b->rc_fail.size())
            b->rc_fail[s] = stream_fail_code(b, s);
        if (rc == SCROLL_OK && (b->h_st[s].err & SCROLL_DEVERR_HANDOFF)) {
            set_err("stream %d: a dynamic-rect row waited past its bound for the row above's "
                    "TotalCoeffs (k_dyn_row hand-off); the stream committed nothing", s);
            rc = SCROLL_ERR_DEVICE;
        } else if (rc == SCROLL_OK && (b->h_st[s].err & SCROLL_DEVERR_SPLICE)) {
            int st = 0, ff = 0;
            for (; ff < b->max_frames && !st; ++ff)
                if (splice_frame_status(b, (size_t)s * b->max_frames + ff, &st)) break;
            if (st == HDYN_STATUS_OVERFLOW) {
                set_err("stream %d frame %d: a dynamic-rect MB under hints outgrew its %u-byte "
                        "region (raise slot_bytes of scroll_batch_set_dyn_rect)", s, ff - 1,
                        4u * b->hd_mb_words);
                rc = SCROLL_ERR_OVERFLOW;
            } else {
                set_err("stream %d frame %d: %s: %s", s, ff - 1,
                        b->dyn_on ? "dynamic rect under hints" : "spliced slice", splice_msg(st));
                rc = SCROLL_ERR_CONFIG;
            }
        } else if (rc == SCROLL_OK && (b->h_st[s].err & SCROLL_DEVERR_HINT)) {
            set_err("stream %d: a hint rect names a reference that is not valid in its frame "
                    "(ref 2 + i needs waypoint i)", s);
            rc = SCROLL_ERR_CONFIG;
        } else if (rc == SCROLL_OK && (b->h_st[s].err & SCROLL_DEVERR_DYN)) {
            uint32_t used[2] = {0, 0};
            if (b->dyn_on && !b->hint_on && b->dx.ctr)
                HIPCHK(hipMemcpy(used, b->dx.ctr, sizeof(used), hipMemcpyDeviceToHost));
            if (used[0] > b->geo.rs_spill_cap || used[1] > b->geo.gen_cap) {
                /* content past the typical-size pools: grow them to their
                 * bound for the next compose (this one committed nothing for
                 * the stream) */
                const int grc = dyn_grow_pools(b);
                set_err("stream %d: the dynamic rect's %s pool ran out (%u of %u); %s", s,
                        used[0] > b->geo.rs_spill_cap ? "row-stage spill" : "general-path record",
                        used[0] > b->geo.rs_spill_cap ? used[0] : used[1],
                        used[0] > b->geo.rs_spill_cap ? b->geo.rs_spill_cap : b->geo.gen_cap,
                        grc ? "growing it failed" : "grown: compose again");
            } else {
                set_err("stream %d: a staged NAL outgrew its staging slot (%llu bytes)", s,
                        (unsigned long long)b->geo.slot_bytes);
            }
            rc = SCROLL_ERR_OVERFLOW;
        } else if (rc == SCROLL_OK) {
            set_err("stream %d: output arena overflow (%llu bytes used, capacity %llu)", s,
                    (unsigned long long)b->h_st[s].out_pos,
                    (unsigned long long)b->h_st[s].out_cap);
            rc = SCROLL_ERR_OVERFLOW;
        }
        b->h_st[s].err = 0;                      /* reported once, then cleared */
        HIPCHK(hipMemcpy(&b->d_st[s].err, &b->h_st[s].err, sizeof(int32_t),
                         hipMemcpyHostToDevice));
    }
    if (rc) return rc;
    return SCROLL_OK;
}

size_t scroll_batch_output_size(ScrollBatch *b, int s)
{
    if (!b || s < 0 || s >= b->nstreams || batch_host_sync(b)) return 0;
    return (size_t)b->h_st[s].out_pos;
}

int scroll_batch_copy_output(ScrollBatch *b, int s, size_t from, uint8_t *dst, size_t n)
{
    if (!b || s < 0 || s >= b->nstreams || (!dst && n)) return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    if (from + n > b->h_st[s].out_pos) {
        set_err("scroll_batch_copy_output: range beyond stream output");
        return SCROLL_ERR_ARG;
    }
    if (n == 0) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpy(dst, b->d_arena + (size_t)s * b->ld_arena + from, n, hipMemcpyDeviceToHost));
    return SCROLL_OK;
}

int scroll_host_alloc(void **p, size_t n)
{
    if (!p) return SCROLL_ERR_ARG;
    *p = nullptr;
    hipError_t e = hipHostMalloc(p, n ? n : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_err("scroll_host_alloc(%zu): %s", n, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SCROLL_ERR_OOM : SCROLL_ERR_HIP;
    }
    return SCROLL_OK;
}

void scroll_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

int scroll_batch_output_to_host_async(ScrollBatch *b, uint8_t *dst, size_t cap, uint64_t *table, void *hip_stream)
{
    if (!b || !dst || !table || (cap & 15) || (reinterpret_cast<uintptr_t>(dst) & 15)) {
        set_err("scroll_batch_output_to_host_async: bad arguments (dst / cap must be 16-byte aligned)");
        return SCROLL_ERR_ARG;
    }
    HIPCHK(hipSetDevice(b->device));
    hipStream_t hs = hip_stream ? (hipStream_t)hip_stream : (b->last ? b->last : b->own);
    if (b->last && hs != b->last) {                 /* after the last compose */
        if (!b->out_ev) HIPCHK(hipEventCreateWithFlags(&b->out_ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(b->out_ev, b->last));
        HIPCHK(hipStreamWaitEvent(hs, b->out_ev, 0));
    }
    const size_t S = (size_t)b->nstreams;
    if (b->out_tab_cap < 1 + 2 * S) {
        (void)hipFree(b->d_out_tab);
        b->d_out_tab = nullptr;
        b->out_tab_cap = 0;
        HIPCHK(hipMalloc(&b->d_out_tab, (1 + 2 * S) * sizeof(uint64_t)));
        b->out_tab_cap = 1 + 2 * S;
    }
    scroll_launch_out_table(hs, b->d_st, (int)S, (uint64_t)cap, b->d_out_tab, table);
    HIPCHK(hipGetLastError());
    if (S) {
        scroll_launch_out_copy(hs, b->d_st, (int)S, b->d_arena, (uint64_t)b->ld_arena,
                               (uint64_t)b->max_streams * b->ld_arena, b->d_out_tab, dst);
        HIPCHK(hipGetLastError());
    }
    b->last = hs;
    b->host_valid = 0;      /* k_out_table zeroes DevStream.undelivered: the next sync waits for
                               the copy and refreshes the host mirror before anything uploads it */
    return SCROLL_OK;
}

const uint8_t *scroll_batch_output_device(ScrollBatch *b, int s)
{
    if (!b || s < 0 || s >= b->nstreams) return nullptr;
    return b->d_arena + (size_t)s * b->ld_arena;
}

int scroll_batch_reset_output(ScrollBatch *b)
{
    if (!b) return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    for (int s = 0; s < b->nstreams; ++s) b->h_st[s].out_pos = b->h_st[s].undelivered = 0;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpy(b->d_st, b->h_st, (size_t)b->nstreams * sizeof(DevStream),
                     hipMemcpyHostToDevice));
    return SCROLL_OK;
}

int scroll_batch_nal_count(ScrollBatch *b, int s)
{
    if (!b || s < 0 || s >= b->nstreams) return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    return b->h_st[s].nnal;
}

int scroll_batch_nal_info(ScrollBatch *b, int s, int i, int *kind, int *offset_px,
                          uint32_t *size, int *slow)
{
    if (!b || s < 0 || s >= b->nstreams) return SCROLL_ERR_ARG;
    int rc = load_nals(b);
    if (rc) return rc;
    if (i < 0 || i >= b->h_st[s].nnal) return SCROLL_ERR_ARG;
    const NalDesc &d = b->nal_cache[(size_t)s * b->ld_nal + i];
    if (kind) *kind = d.kind;
    if (offset_px) *offset_px = d.off;
    if (size) *size = d.size;
    if (slow) *slow = d.slow;
    return SCROLL_OK;
}

int scroll_batch_kernel_stats(ScrollBatch *b, double *plan_ms, double *emit_ms, int *count)
{
    if (!b) return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(b->last));
    fold_ring(b);
    if (plan_ms) *plan_ms = b->acc_ms[0];
    if (emit_ms) *emit_ms = b->acc_ms[1];
    if (count) *count = b->acc_n;
    for (int k = 0; k < 6; ++k) b->acc_ms[k] = 0;
    b->acc_n = 0;
    return SCROLL_OK;
}

int scroll_batch_kernel_stats_ex(ScrollBatch *b, double ms[6], int *count)
{
    if (!b || !ms) return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(b->last));
    fold_ring(b);
    for (int k = 0; k < 6; ++k) {
        ms[k] = b->acc_ms[k];
        b->acc_ms[k] = 0;
    }
    if (count) *count = b->acc_n;
    b->acc_n = 0;
    return SCROLL_OK;
}

long long scroll_batch_debug_stamps(ScrollBatch *b, uint64_t *dst, long long max_slots)
{
    if (!b || batch_host_sync(b) || !b->d_dbg) return 0;
    long long n = (long long)b->dbg_slots < max_slots ? (long long)b->dbg_slots : max_slots;
    if (hipMemcpy(dst, b->d_dbg, (size_t)n * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost) !=
        hipSuccess)
        return 0;
    return n;
}

unsigned long long scroll_batch_last_bytes(ScrollBatch *b)
{
    if (!b || batch_host_sync(b)) return 0;
    unsigned long long t = 0;
    for (int s = 0; s < b->nstreams; ++s) t += b->h_st[s].batch_bytes;
    return t;
}

long long scroll_batch_last_nals(ScrollBatch *b)
{
    if (!b || batch_host_sync(b)) return -1;
    long long t = 0;
    for (int s = 0; s < b->nstreams; ++s) t += b->h_st[s].nnal;
    return t;
}

int scroll_batch_enable_timing(ScrollBatch *b, int on)
{
    if (!b) return SCROLL_ERR_ARG;
    b->timing = on;
    return SCROLL_OK;
}

float scroll_batch_kernel_ms(ScrollBatch *b, int which)
{
    if (!b || which < 0 || which > 5) return -1.0f;
    if (b->timing == 2) return -1.0f;           /* lite: no per-kernel pairs (kernel_stats_ex has the dominant one) */
    if (batch_host_sync(b)) return -1.0f;
    if (b->timed_pending) {
        event_ms(b->ev, b->ev_dyn != 0, false, b->ms);
        b->timed_pending = 0;
    }
    return b->ms[which];
}

}  // extern "C"
