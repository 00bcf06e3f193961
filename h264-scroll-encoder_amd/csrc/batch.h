/*
 * batch.h -- internal to the host-side batch engine behind
 * include/composer_batch.h: the batch's state and what its files share.
 *   batch_core.hip    create / destroy, streams, compose, sync, output, timing
 *   batch_pass.hip    what the side passes share: the last-run record, the dry plan, the prediction rows
 *   batch_dyn.hip     the dynamic rect, its reconstruction and its QP probe
 *   batch_rate.hip    the plain rect's per-frame QP table and the pick on the device
 *   batch_hint.hip    UI hints, the rect under hints, the splice
 *   batch_ingest.hip  ingest, I_PCM files, reference updates
 *   batch_surface.hip pixels from RGBA / BGRA surfaces: the rect's source, I420 pictures, device references
 *   batch_damage.hip  the rect located from the surfaces: damage map, placement, the positions' device ownership
 *   batch_mask.hip    the rect's per-MB source mask: difference map, keep decision, fill
 *   batch_detect.hip  each frame's scroll offset detected from the surfaces: signatures, scores, the choice
 *   batch_dropin.hip  the synchronous drop-in helpers of engine.h
 * A side pass (the QP probe, the pick, the locate, the mask, the detect) is
 * an asynchronous call beside the compose with device buffers of its own: it
 * keeps its last run in a PassRun and, where it needs the compose's state
 * pass, runs it dry into a DryPlan (and k_dyn_rows into a PredRows) through
 * batch_pass.hip's helpers.  A new pass does the same.
 * Nothing here enters the library's dynamic symbol table.
 */
#ifndef SCROLL_BATCH_H
#define SCROLL_BATCH_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "engine.h"
#include "dyn_engine.h"         /* DynScratch, DynFork */
#include "splice_engine.h"      /* SpliceFrame, SpliceMbRec, SpliceUnit */
#include "ingest_engine.h"      /* IngestFile, IngestScan, IngestOut */
#include "pick_engine.h"        /* PickOut */

/* (set_err: scroll::batch's, below) */
#define HIPCHK(x)                                                                  \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            set_err("%s failed: %s", #x, hipGetErrorString(e_));                   \
            return SCROLL_ERR_HIP;                                                 \
        }                                                                          \
    } while (0)

/* ======================================================================== */
/* ScrollBatch                                                              */
/* ======================================================================== */
/* (the public headers' opaque type: global, and outside the hidden region
 * below, which would take its implicit members' symbols out of the library;
 * so are the three records it holds by value) */
/* a side pass's last run (batch_pass.hip) */
struct PassRun {
    int nframes = -1, nstreams = 0;    /* the last run; nframes -1: none */
    int timed = 0;                     /* the last run recorded its timing events */
    int nev = 0;                       /* the pass's timing events, ev[0 .. nev - 1] (pass_begin); 0: never timed */
    hipEvent_t fin = nullptr;          /* recorded after the last run's launches */
    hipEvent_t ev[5] = {};             /* timing: created on first use; those past nev stay null */
};
/* the compose's state pass into buffers of a side pass's own, nothing committed */
struct DryPlan {
    NalDesc *nal = nullptr;
    DynFrame *dfr = nullptr;
    PlanPending *pend = nullptr;
};
/* k_dyn_rows' prediction rows after a dry plan, as the compose keeps them in dx */
struct PredRows {
    uint32_t *rows = nullptr, *ctr = nullptr;
    uint4 *heads = nullptr;
};
constexpr int NEV = 7;
struct ScrollBatch {
    int device = 0;
    int mode = SCROLL_MODE_COMPOSER;
    int max_streams = 0, max_frames = 0, nstreams = 0;
    int debug = 0;
    size_t arena_bytes = 0, ld_arena = 0;
    int ld_nal = 0;
    DevStream *d_st = nullptr;
    DevStream *h_st = nullptr;
    int32_t *d_off = nullptr;
    NalDesc *d_nal = nullptr;
    uint8_t *d_arena = nullptr;
    hipStream_t own = nullptr;
    hipStream_t last = nullptr;
    hipEvent_t ev[NEV] = {};
    int timing = 0;
    int timed_pending = 0;
    float ms[6] = {0, 0, 0, 0, 0, 0};  /* plan, emit, dyn stage, dyn emit, dyn code, dyn pack */
    std::vector<hipEvent_t> ring;      /* NEV events per timed compose, pending */
    std::vector<uint8_t> ring_dyn;     /* per pending compose: 1 the dynamic-rect pipeline ran, 2 lite timing */
    int ev_dyn = 0;                    /* the same for b->ev */
    int ring_used = 0;
    double acc_ms[6] = {0, 0, 0, 0, 0, 0};
    int acc_n = 0;
    int host_valid = 1;
    int last_plan_mode = SCROLL_PLAN_COMPOSER;
    int last_nframes = 0;
    std::vector<NalDesc> nal_cache;
    int nal_cache_valid = 0;
    uint64_t *d_dbg = nullptr;
    size_t dbg_slots = 0;
    /* dynamic rect (configs 3-5) */
    PlanPending *d_pend = nullptr;
    int dyn_on = 0;
    int dyn_pw = 0, dyn_ph = 0;        /* picture size every stream must have      */
    int dyn_refs = 0;                  /* 0 unset, 1 shared pair, 2 per stream     */
    DynGeom geo{};
    DynFrame *d_dfr = nullptr;
    uint8_t *d_src = nullptr, *d_refs = nullptr, *d_stage = nullptr;
    DynScratch dx{};                   /* rows, block records, look-back words of the dynamic coder */
    /* the rect's reconstruction (scroll_batch_set_dyn_recon, recon_kernels.hip) */
    int recon_on = 0;
    uint8_t *d_rec = nullptr;          /* decoded rects, d_src's layout and strides          */
    unsigned long long *d_sse = nullptr;   /* [max_streams * max_frames][3]: Y, Cb, Cr       */
    hipEvent_t rc_ev[2] = {};          /* timing: around k_dyn_recon (created on first use)  */
    int rc_timed = 0;                  /* the last compose recorded them                     */
    /* ... under UI hints (scroll_batch_set_dyn_recon_hinted, hrecon_kernels.hip) */
    int recon_hinted = 0;
    int rc_last_hint = 0;              /* the last compose ran k_hdyn_recon                  */
    std::vector<int> rc_fail;          /* [stream]: the status scroll_batch_sync reported for that compose */
    /* the QP probe (scroll_batch_dyn_probe, probe_kernels.hip): a trial plan
     * and its prediction rows in buffers of its own, so that nothing of the
     * batch's state is touched; allocated by the first probe */
    struct Probe {
        DryPlan plan;
        PredRows pr;
        uint32_t *done = nullptr;
        ScrollDynProbe *res = nullptr;  /* [max_streams * max_frames][SCROLL_DYN_PROBE_MAX_QPS] */
        uint8_t *cls = nullptr;         /* [max_streams * max_frames]: k_hprobe_class (scroll_batch_dyn_probe_hinted) */
        int hinted = 0;                 /* the last probe was the hinted one */
        int nq = 0;
        uint8_t qps[SCROLL_DYN_PROBE_MAX_QPS] = {};   /* the last probe's candidates (scroll_batch_dyn_pick) */
        PassRun run;                    /* ev[0..1]: around the probe's launches */
    } pb;
    /* the plain rect's per-frame QP table (dx.qpf, batch_rate.hip) and the
     * pick that fills it from the probe on the device (pick_kernels.hip);
     * everything allocated on first use, freed with the rect */
    std::vector<uint8_t> h_qpf;         /* the table as the host last knew it, [max_streams * max_frames] */
    int qpf_dev = 0;                    /* the device may have written it since (a pick, a caller's kernel) */
    struct Rate {
        long long *level = nullptr;     /* [max_streams]: the buckets' levels */
        uint32_t *fb = nullptr;         /* [max_streams]: frame_bits per stream of the last pick that gave them */
        PickOut *out = nullptr;         /* [max_streams * max_frames]: the last pick's choices */
        PassRun run;                    /* the last pick (no timing events) */
    } rt;
    /* pixels from renderer surfaces (batch_surface.hip, csc_kernels.hip):
     * nothing here exists before the first conversion */
    struct Surf {
        int32_t *pos = nullptr;         /* [nstreams * nframes][2]: the last call's per-frame rect origins (custom positions only) */
        std::vector<int32_t> h_pos;     /* what was uploaded there */
        /* recorded after the last kernel that reads pos: it guards pos and goes
         * with the rect (surface_release).  Not the end of a run: run.fin below
         * stays null, and nothing may wait on it or record it */
        hipEvent_t fin = nullptr;
        PassRun run;                    /* ev[0..1] and timed only: around the last conversion; kept with the batch */
    } sf;
    /* the rect located from the surfaces (scroll_batch_dyn_locate,
     * batch_damage.hip, damage_kernels.hip): a dry plan, the prediction rows
     * of whole pictures, the map and the records; nothing here exists before
     * the first locate, everything goes with the rect */
    struct Locate {
        DryPlan plan;
        uint32_t *rows = nullptr;       /* [max_streams * max_frames][ph] */
        uint32_t *map = nullptr;        /* [max_streams * max_frames][mbh][mbw] */
        ScrollDynDamage *res = nullptr; /* [max_streams * max_frames] */
        PassRun run;                    /* ev[0..3]: the call's start, around k_dyn_damage, its end */
    } lc;
    /* the rect's per-MB source mask (scroll_batch_dyn_mask, batch_mask.hip,
     * mask_kernels.hip): a dry plan and its prediction rows as the probe keeps
     * them, the map, the rows' chroma partials and the records; nothing here
     * exists before the first mask, everything goes with the rect */
    struct Mask {
        DryPlan plan;
        PredRows pr;
        uint32_t *map = nullptr;        /* [max_streams * max_frames][h][w][2] */
        unsigned long long *part = nullptr;   /* [max_streams * max_frames][h][2]: Cb, Cr dropped per rect row */
        ScrollDynMask *res = nullptr;   /* [max_streams * max_frames] */
        PassRun run;                    /* ev[0..3]: the call's start, around k_dyn_mask_diff, its end */
    } mk;
    /* each frame's scroll offset detected from the surfaces
     * (scroll_batch_detect_offsets, batch_detect.hip, detect_kernels.hip):
     * both signature arrays, the scores and the records; nothing here exists
     * before the first detect, everything goes with the rect */
    struct Detect {
        uint16_t *sig_s = nullptr;      /* [max_streams * max_frames][ph][nseg] (the call's nuse of them) */
        uint16_t *sig_r = nullptr;      /* [max_streams][nseg][2 ph] */
        uint32_t *scores = nullptr;     /* [max_streams * max_frames][ph + 1] */
        ScrollOffsetFound *res = nullptr;   /* [max_streams * max_frames] */
        PassRun run;                    /* ev[0..4]: the call's start, around k_det_surf, after k_det_score, its end */
    } dt;
    /* UI hints: staged like the dynamic rect (shares
     * d_dfr, d_stage and geo.slot_bytes; the two are exclusive) */
    int hint_on = 0;
    int hint_dirty = 0;
    int hint_max_mb = 0;               /* MBs per picture the slots are sized for */
    std::vector<std::vector<ScrollHintRect>> h_hint;   /* [s * max_frames + f] */
    std::vector<int16_t> h_hint_mode;
    HintFrame *d_hf = nullptr;
    ScrollHintRect *d_pool = nullptr;
    size_t pool_cap = 0;
    /* pre-encoded MB splice: frames of the hint path
     * whose rect comes from an external slice */
    struct SpliceHost {
        int x0 = 0, y0 = 0, w = 0, h = 0;
        std::vector<uint8_t> nal;      /* host bytes (scroll_batch_set_splice)          */
        const uint8_t *dnal = nullptr; /* or device bytes (scroll_batch_set_splices_device) */
        size_t n = 0;
    };
    std::vector<SpliceHost> h_sp;      /* [s * max_frames + f]; w = 0: none */
    /* the dynamic rect under UI hints (hdyn_kernels.hip): with both on,
     * every frame's rect MBs are coded by k_hdyn_code into splice records
     * (d_sp_rec, word pool d_sp_rbsp) and composed by k_splice_stage */
    std::vector<int32_t> h_dyn_pos;    /* [2 (s * max_frames + f)]: rect origin, x0 < 0: none */
    int fallback = 0;                  /* scroll_batch_set_fallback: k_hint_fb before the stage kernels */
    DynFork fork{};                    /* SCROLL_DYN_FORK=1: the general path + static groups beside k_dyn_row */
    std::vector<int32_t> h_dyn_qp;     /* [s * max_frames + f]: the frame's rect QP under hints, -1: the stream's */
    int dyn_pos_custom = 0;            /* some frame's origin differs from the batch rect */
    /* scroll_batch_set_dyn_rect_moving: h_dyn_pos honoured without hints, on
     * the k_dyn_row path.  The device table (DynGeom.dpos's form) exists
     * while the flag is on and is uploaded, on the stream of the compose or
     * probe that finds it stale, only while some entry differs from the
     * batch's position; otherwise the kernels get no table */
    int dyn_moving = 0;
    uint32_t *d_dpos = nullptr;        /* [max_streams * max_frames] */
    std::vector<uint32_t> h_dpos;      /* what was uploaded there (the copy's source until the stream has run it) */
    int dpos_stale = 1;                /* h_dyn_pos changed since the upload */
    int dpos_any = 0;                  /* as of the upload: some entry differs */
    /* a locate with apply wrote entries of d_dpos (batch_damage.hip): the
     * device's table is the truth and h_dyn_pos / dyn_pos_custom are behind
     * until dyn_pos_refresh reads it back; never set together with dpos_stale */
    int dpos_dev = 0;
    /* scroll_batch_set_dyn_rect_size_at: the columns and rows
     * frame (s, f)'s rect is short of the batch's, [2 (s * max_frames + f)],
     * empty until the first size is set -- apart from h_dyn_pos, which the
     * hinted uploads read.  dsz_any: some entry is not 0 (as of the last
     * change, or of the read-back of a located table); dsz_on: the row stage
     * is sized for every h_f (done once, by the first call) */
    std::vector<uint8_t> h_dyn_dsz;
    size_t dsz_nz = 0;                 /* frames whose entry is not (0, 0): dsz_any without a scan */
    int dsz_any = 0;
    int dsz_on = 0;
    hipStream_t dpos_hs = nullptr;     /* the stream that upload ran on ... */
    hipEvent_t dpos_ev = nullptr;      /* ... and its end: other streams wait for it, the next packing too */
    int dyn_qp = 26;                   /* the rect's QP (scroll_batch_set_dyn_qp)          */
    int hd_dirty = 0;                  /* d_spf / HintFrame of the combined frames out of date */
    uint32_t hd_mb_words = 0;          /* pool words per rect MB */
    size_t dyn_cap = 0;                /* the dynamic rect's own staging cap (geo.slot_bytes without hints) */
    int sp_n = 0;                      /* spliced frames                           */
    int sp_dirty = 0;                  /* upload + parse before the next compose   */
    int sp_parse = 0;                  /* k_splice_parse pending                   */
    SpliceFrame *d_spf = nullptr;      /* [max_streams * max_frames]               */
    uint8_t *d_sp_nal = nullptr;
    uint32_t *d_sp_rbsp = nullptr;
    SpliceMbRec *d_sp_rec = nullptr;
    int32_t *d_sp_list = nullptr;
    SpliceUnit *d_sp_units = nullptr;  /* NAL unit slots (splice_unit_cap per frame) */
    int32_t *d_sp_lanes = nullptr;     /* lane list: count (zero between parses), (list index, unit) pairs */
    size_t sp_lanes_cap = 0, sp_nslots = 0;
    int sp_ymax = 1;                   /* most unit slots of a frame (parse grid y)  */
    size_t sp_nal_cap = 0, sp_rbsp_cap = 0, sp_rec_cap = 0, sp_list_cap = 0, sp_units_cap = 0;
    /* stream ingest: scratch, grown on demand */
    uint8_t *d_ing_in = nullptr;
    size_t ing_in_cap = 0;
    IngestFile *d_ing_files = nullptr;
    IngestScan *d_ing_scan = nullptr;
    IngestOut *d_ing_out = nullptr;
    int ing_cap = 0;
    void *d_ing_work = nullptr;                 /* segmented ingest scratch */
    size_t ing_work_bytes = 0;
    hipEvent_t ing_ev[2] = {};         /* timing: around the ingest kernels */
    /* reference files from pictures: EP count per chunk */
    uint32_t *d_ipcm_cnt = nullptr;
    size_t ipcm_cap = 0;
    uint8_t *d_ipcm_stg = nullptr;              /* count pass RBSP for the write pass */
    size_t ipcm_stg_cap = 0;
    /* the one pass: the chunks' hand-off words */
    unsigned long long *d_ipcm_hw = nullptr;
    size_t ipcm_hw_cap = 0;
    uint32_t ipcm_epoch = 0;
    double ipcm_ms = 0.0;
    int ipcm_n = 0;
    /* the asynchronous I_PCM calls since the last sync: their overflow flag
     * (checked at the sync) and, with timing, their event pairs */
    uint32_t *ipcm_over = nullptr;      /* = d_ipcm_sticky while calls are pending */
    uint32_t *d_ipcm_sticky = nullptr;
    size_t ipcm_over_stride = 0;
    std::vector<hipEvent_t> ipcm_ev;    /* pairs, reused */
    size_t ipcm_ev_used = 0;
    double ing_ms = 0.0;
    int ing_n = 0;
    /* host delivery: per-stream (offset, bytes) table of the last packing */
    int dyn_grow = 0;                  /* the dynamic rect's pools at their bounds (after running out) */
    int32_t *d_upd = nullptr;          /* reference updates: (stream, which) per entry */
    size_t upd_cap = 0;
    uint64_t *d_out_tab = nullptr;
    size_t out_tab_cap = 0;
    hipEvent_t out_ev = nullptr;
};

#pragma GCC visibility push(hidden)
namespace scroll {
namespace batch {

/* ---- batch_core.hip ---- */
void set_err(const char *fmt, ...);
int usable_devices(std::vector<int> *ids);
int check_cfg(const ComposerConfig *c);
void cfg_to_dev(const ComposerConfig *c, DevStream *d);
void dev_to_cfg(const DevStream *d, ComposerConfig *c);
hipError_t timing_event(hipEvent_t *e);
/* `who` could not allocate (or otherwise failed with e): the message
 * "who: error", the sticky error cleared on request, SCROLL_ERR_OOM or
 * SCROLL_ERR_HIP */
int hip_fail(const char *who, hipError_t e, bool clear = false);
int dev_grow(void **p, size_t *cap, size_t n, size_t size, const char *who);
int batch_host_sync(ScrollBatch *b);
int launch(ScrollBatch *b, int nframes, int plan_mode, int nal_max, hipStream_t hs, int plan_flags = 0);
int stream_fail_code(ScrollBatch *b, int s);
int load_nals(ScrollBatch *b);

/* ---- batch_pass.hip ---- */
/* waits for the last run, destroys the record's events and resets it */
void pass_release(PassRun *r);
/* a run begins on hs: not timed yet; with the batch's timing on, the pass's n
 * events (those not there yet are created) and ev[0] recorded */
int pass_begin(ScrollBatch *b, PassRun *r, int n, hipStream_t hs);
/* ev[i] recorded, when the batch's timing is on */
int pass_mark(ScrollBatch *b, PassRun *r, int i, hipStream_t hs);
/* the timing's end: the pass's last event recorded, the run timed */
int pass_stop(ScrollBatch *b, PassRun *r, hipStream_t hs);
/* the run's end: pass_stop, fin recorded, the run of nframes x nstreams the last one */
int pass_end(ScrollBatch *b, PassRun *r, hipStream_t hs, int nframes, int nstreams);
/* a result call of `who` without a run to read (none yet, or released with
 * the pass's buffers): SCROLL_ERR_CONFIG, "no <noun> to read (<entry>; ...)" */
int pass_have(const PassRun *r, const char *who, const char *noun, const char *entry);
/* the frame of the last run that a result call names: pass_have, stream and
 * frame inside it (SCROLL_ERR_ARG); the run has finished on return */
int pass_frame_arg(ScrollBatch *b, PassRun *r, int s, int f, const char *who, const char *noun, const char *entry);
/* ms from ev[from] to ev[to] of the last run, once its last event has
 * passed; -1 when it was not timed or the time cannot be read */
float pass_span_ms(ScrollBatch *b, const PassRun *r, int from, int to);
hipError_t dry_plan_alloc(const ScrollBatch *b, DryPlan *d);
void dry_plan_free(DryPlan *d);
/* k_plan's state pass for nframes of the batch's streams into d; ctr: the
 * counters it zeroes, dpos: the moving rect's position table, or none */
int dry_plan_launch(ScrollBatch *b, hipStream_t hs, int nframes, const DryPlan &d, int flags_extra = 0,
                    uint32_t *ctr = nullptr, const uint32_t *dpos = nullptr);
hipError_t pred_rows_alloc(const ScrollBatch *b, PredRows *p);
void pred_rows_free(PredRows *p);
/* k_dyn_rows after dry_plan_launch into p, G->gen_cap a slot for every frame; no per-frame QP table */
int pred_rows_launch(ScrollBatch *b, hipStream_t hs, int nframes, const DryPlan &d, const PredRows &p, DynGeom *G);

/* ---- batch_dyn.hip ---- */
void probe_release(ScrollBatch *b);
void dyn_release(ScrollBatch *b);
int dyn_grow_pools(ScrollBatch *b);
int dyn_reserve_gen(ScrollBatch *b, size_t need);
int dyn_set_refs(ScrollBatch *b, int s, const uint8_t *ref_a, const uint8_t *ref_b, hipMemcpyKind kind);
/* *dpos: the position table for a launch of the plain rect's kernels on hs
 * (uploaded there first when stale), or NULL: the flag is off, or every
 * frame sits at the batch's position */
int dyn_pos_table(ScrollBatch *b, hipStream_t hs, const uint32_t **dpos);
/* entry i of the table as the host has it: origin and size packed (dyn_pos.h) */
uint32_t dyn_pos_word(const ScrollBatch *b, size_t i);
/* some frame has a size of its own (bringing the host's copy up to date
 * first where a locate wrote the table): what the hinted paths refuse */
int dyn_sizes_any(ScrollBatch *b, bool *any);
/* before the first frame gets a size of its own (scroll_batch_set_dyn_rect_size_at,
 * a locate with size = 1): the row stage, the groups' bit counts and the
 * static grid for every legal (y0, h_f), allocated once; later calls do
 * nothing.  SCROLL_ERR_CONFIG without scroll_batch_set_dyn_rect_moving or in
 * a picture of more than 256 MBs either way */
int dyn_sizes_enable(ScrollBatch *b, const char *who);

/* ---- batch_rate.hip ---- */
void rate_release(ScrollBatch *b);
/* *any: some entry of the per-frame QP table differs from 0xFF (reads the
 * table back when the device may have written it) */
int qp_frames_any(ScrollBatch *b, bool *any);

/* ---- batch_hint.hip ---- */
int hint_upload(ScrollBatch *b);
int hd_setup(ScrollBatch *b);
int hd_upload(ScrollBatch *b);
int splice_upload(ScrollBatch *b);
int splice_frame_status(ScrollBatch *b, size_t i, int *status);
const char *splice_msg(int e);

/* ---- batch_ingest.hip ---- */
int ipcm_async_check(ScrollBatch *b);

/* ---- batch_surface.hip ---- */
/* the per-frame position table goes with the rect (all = false); the timing
 * events with the batch (all = true) */
void surface_release(ScrollBatch *b, bool all);
/* what every surface call asks of the surfaces: w pixels of every row lie inside the pitch */
int surf_args(const char *who, const ScrollSurfaces *surf, uint64_t w, bool streams);

/* ---- batch_damage.hip ---- */
void locate_release(ScrollBatch *b);
/* before host code reads or merges into h_dyn_pos / dyn_pos_custom: when a
 * locate has placed frames on the device, wait for it and read the table
 * back (synchronising); otherwise nothing */
int dyn_pos_refresh(ScrollBatch *b);

/* ---- batch_mask.hip ---- */
void mask_release(ScrollBatch *b);

/* ---- batch_detect.hip ---- */
void detect_release(ScrollBatch *b);

}  // namespace batch
}  // namespace scroll
#pragma GCC visibility pop

#endif
