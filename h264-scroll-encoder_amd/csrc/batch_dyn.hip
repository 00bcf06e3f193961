/*
 * batch_dyn.hip -- the batch engine's dynamic rect (batch.h): the rect, its
 * pools, references and source, its QP, the fallback switch, the
 * reconstruction and the QP probe (plain and under UI hints).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "batch.h"
#include "scroll_engine.h"
#include "dyn_engine.h"
#include "probe_engine.h"
#include "hprobe_engine.h"
#include "hdyn_engine.h"        /* HDYN_MB_WORDS_*: pool words per rect MB under hints */
#include "dyn_pos.h"            /* dyn_pos_pack: the position table's word */
#include "dyn_device.h"         /* scroll::dyn::qparams, qp_chroma: DynGeom's quantisers */

using namespace scroll::batch;

namespace scroll {
namespace batch {

/* the probe's buffers go with the rect they were sized for */
void probe_release(ScrollBatch *b)
{
    ScrollBatch::Probe &p = b->pb;
    pass_release(&p.run);
    dry_plan_free(&p.plan);
    pred_rows_free(&p.pr);
    (void)hipFree(p.done);
    (void)hipFree(p.res);
    (void)hipFree(p.cls);
    p = ScrollBatch::Probe{};
}

void dyn_release(ScrollBatch *b)
{
    probe_release(b);
    locate_release(b);                 /* the locate's buffers, and the device's ownership of the positions */
    mask_release(b);
    detect_release(b);
    if (!b->hint_on) {                 /* else they are the hint path's */
        (void)hipFree(b->d_dfr);
        (void)hipFree(b->d_stage);
        b->d_dfr = nullptr;
        b->d_stage = nullptr;
    }
    (void)hipFree(b->d_src);
    (void)hipFree(b->d_refs);
    (void)hipFree(b->dx.rows);
    (void)hipFree(b->dx.meta);
    (void)hipFree(b->dx.body_lo);
    (void)hipFree(b->dx.body_hi);
    (void)hipFree(b->dx.body_w);
    (void)hipFree(b->dx.heads);
    (void)hipFree(b->dx.tcx);
    (void)hipFree(b->dx.rowstage);
    (void)hipFree(b->dx.ctr);
    (void)hipFree(b->dx.gbits);
    (void)hipFree(b->dx.qpf);          /* the per-frame QP table, its pick and the buckets' levels */
    (void)hipFree(b->d_dpos);          /* the moving rect's position table goes with the rect */
    if (b->dpos_ev) (void)hipEventDestroy(b->dpos_ev);
    b->d_dpos = nullptr;
    b->dpos_ev = nullptr;
    b->dpos_hs = nullptr;
    b->h_dpos.clear();
    b->dyn_moving = 0;
    b->dpos_stale = 1;
    b->dpos_any = 0;
    b->h_dyn_dsz.clear();              /* sizes go with the rect */
    b->dsz_nz = 0;
    b->dsz_any = 0;
    b->dsz_on = 0;
    rate_release(b);
    surface_release(b, false);
    (void)hipFree(b->d_rec);           /* the reconstruction goes with the rect it was sized for */
    (void)hipFree(b->d_sse);
    b->d_rec = nullptr;
    b->d_sse = nullptr;
    b->recon_on = 0;
    b->recon_hinted = 0;
    b->d_src = b->d_refs = nullptr;
    b->dx = DynScratch{};
    b->dyn_on = 0;
    b->dyn_refs = 0;
    b->h_dyn_pos.clear();
    b->h_dyn_qp.clear();
    b->dyn_pos_custom = 0;
    if (b->hint_on) {                  /* the combined frames become plain hint frames */
        b->geo.x0 = b->geo.y0 = b->geo.w = b->geo.h = 0;
        b->sp_dirty = 1;                   /* d_spf back to the (no) splices */
        b->hint_dirty = 1;
    }
}

/* the general-path record pool and the row-stage spill pool at their
 * bounds (a slot for every NAL / rect row), keeping source and references */
int dyn_grow_pools(ScrollBatch *b)
{
    if (!b->dyn_on || b->dyn_grow) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    DynGeom g = b->geo;
    const size_t S = (size_t)b->max_streams, F = (size_t)b->max_frames, nmb = (size_t)g.w * g.h;
    g.gen_cap = (uint32_t)(S * F);
    if (g.rs_spill_cap) g.rs_spill_cap = (uint32_t)(S * F * (size_t)g.h);
    const size_t nrec = (size_t)g.gen_cap * DYN_PIECES * nmb;
    const size_t rs_words = S * F * g.rs_frame_words + (size_t)g.rs_spill_cap * g.rs_spill_words;
    uint16_t *meta = nullptr;
    uint2 *lo = nullptr, *hi = nullptr;
    uint4 *wd = nullptr;
    uint32_t *rs = nullptr;
    hipError_t e = hipMalloc(&meta, nrec * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc(&lo, nrec * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(&hi, nrec * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(&wd, nrec * sizeof(uint4));
    if (e == hipSuccess) e = hipMalloc(&rs, rs_words * sizeof(uint32_t));
    if (e != hipSuccess) {
        (void)hipFree(meta);
        (void)hipFree(lo);
        (void)hipFree(hi);
        (void)hipFree(wd);
        (void)hipFree(rs);
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? SCROLL_ERR_OOM : SCROLL_ERR_HIP;
    }
    (void)hipFree(b->dx.meta);
    (void)hipFree(b->dx.body_lo);
    (void)hipFree(b->dx.body_hi);
    (void)hipFree(b->dx.body_w);
    (void)hipFree(b->dx.rowstage);
    b->dx.meta = meta;
    b->dx.body_lo = lo;
    b->dx.body_hi = hi;
    b->dx.body_w = wd;
    b->dx.rowstage = rs;
    b->dx.spill = rs + S * F * g.rs_frame_words;
    b->geo.gen_cap = g.gen_cap;
    b->geo.rs_spill_cap = g.rs_spill_cap;
    b->dyn_grow = 1;
    return SCROLL_OK;
}

/* general-path record slots for `need` NALs (at most one per frame), keeping
 * everything else: for per-frame QPs below QP_MIN that the engine knows of
 * before the launch (batch_rate.hip).  The batch is idle when this runs. */
int dyn_reserve_gen(ScrollBatch *b, size_t need)
{
    if (!b->dyn_on) return SCROLL_OK;
    need = std::min(need, (size_t)b->max_streams * (size_t)b->max_frames);
    if (need <= b->geo.gen_cap) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    const size_t nrec = need * DYN_PIECES * (size_t)b->geo.w * b->geo.h;
    uint16_t *meta = nullptr;
    uint2 *lo = nullptr, *hi = nullptr;
    uint4 *wd = nullptr;
    hipError_t e = hipMalloc(&meta, nrec * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc(&lo, nrec * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(&hi, nrec * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(&wd, nrec * sizeof(uint4));
    if (e != hipSuccess) {
        (void)hipFree(meta);
        (void)hipFree(lo);
        (void)hipFree(hi);
        (void)hipFree(wd);
        return hip_fail("the dynamic rect's general-path record pool", e, true);
    }
    (void)hipFree(b->dx.meta);
    (void)hipFree(b->dx.body_lo);
    (void)hipFree(b->dx.body_hi);
    (void)hipFree(b->dx.body_w);
    b->dx.meta = meta;
    b->dx.body_lo = lo;
    b->dx.body_hi = hi;
    b->dx.body_w = wd;
    b->geo.gen_cap = (uint32_t)need;
    return SCROLL_OK;
}

}  // namespace batch
}  // namespace scroll

static size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

static size_t dyn_pair_bytes(const ScrollBatch *b)
{
    return round256((size_t)3 * b->dyn_pw * b->dyn_ph);   /* A and B, I420 each */
}

static int probe_alloc(ScrollBatch *b)
{
    ScrollBatch::Probe &p = b->pb;
    if (p.res) return SCROLL_OK;
    const size_t NF = (size_t)b->max_streams * (size_t)b->max_frames;
    hipError_t e = dry_plan_alloc(b, &p.plan);
    if (e == hipSuccess) e = pred_rows_alloc(b, &p.pr);
    if (e == hipSuccess) e = hipMalloc(&p.done, NF * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&p.res, NF * SCROLL_DYN_PROBE_MAX_QPS * sizeof(ScrollDynProbe));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p.run.fin, hipEventDisableTiming);
    if (e != hipSuccess) {
        probe_release(b);
        return hip_fail("scroll_batch_dyn_probe", e, true);
    }
    return SCROLL_OK;
}

/* what both probes ask of their arguments and of the batch; the candidates -> Q */
static int probe_args(ScrollBatch *b, const char *who, int nframes, const uint8_t *qps, int nq, ProbeQps *Q)
{
    if (!b || !qps || nq < 1 || nq > SCROLL_DYN_PROBE_MAX_QPS) {
        set_err("%s: 1..%d candidate QPs", who, SCROLL_DYN_PROBE_MAX_QPS);
        return SCROLL_ERR_ARG;
    }
    if (nframes < 0 || nframes > b->max_frames) {
        set_err("%s: nframes %d out of range", who, nframes);
        return SCROLL_ERR_ARG;
    }
    Q->n = nq;
    for (int k = 0; k < nq; ++k) {
        if (qps[k] > 51) {
            set_err("%s: candidate %d: QP %d outside 0..51", who, k, qps[k]);
            return SCROLL_ERR_ARG;
        }
        Q->qp[k] = qps[k];
    }
    if (!b->dyn_on || !b->dyn_refs) {
        set_err("%s: needs a dynamic rect with reference pictures "
                "(scroll_batch_set_dyn_rect, scroll_batch_set_dyn_refs)", who);
        return SCROLL_ERR_CONFIG;
    }
    return SCROLL_OK;
}

/* a probe of nframes frames at nq candidates, once its buffers are there:
 * the compose's state pass into the probe's own DryPlan (k_plan with
 * PLAN_STATE reads the streams and commits nothing; ctr: the counters it
 * zeroes, or none), then the probe's own launches: own(hs, S, G, ev1), ev1 to
 * record after them when timed.  The run is stored before the launches, and
 * fin recorded, for a probe of no frames too: it is a valid last probe, which
 * a pick of 0 frames may follow */
template <class Own>
static int probe_run(ScrollBatch *b, int nframes, const ProbeQps &Q, void *hip_stream, int hinted, uint32_t *ctr,
                     Own own)
{
    ScrollBatch::Probe &p = b->pb;
    hipStream_t hs = hip_stream ? (hipStream_t)hip_stream : b->own;
    const int S = b->nstreams, nq = Q.n;
    p.run.nframes = nframes;
    p.run.nstreams = S;
    p.nq = nq;
    for (int k = 0; k < nq; ++k) p.qps[k] = Q.qp[k];
    p.run.timed = 0;
    p.hinted = hinted;
    if (S > 0 && nframes > 0) {
        const bool timed = b->timing != 0;
        int rc = pass_begin(b, &p.run, 2, hs);
        if (rc) return rc;
        DynGeom G = b->geo;
        G.debug = b->debug;
        /* moving rects (never under hints): the frames' own origins, and no dynamic NAL where there is no rect */
        if ((rc = dyn_pos_table(b, hs, &G.dpos))) return rc;
        if ((rc = dry_plan_launch(b, hs, nframes, p.plan, 0, ctr, G.dpos))) return rc;
        if ((rc = own(hs, S, G, timed ? p.run.ev[1] : nullptr))) return rc;
        p.run.timed = timed ? 1 : 0;
    }
    HIPCHK(hipEventRecord(p.run.fin, hs));
    return SCROLL_OK;
}

namespace scroll {
namespace batch {

/* reference pictures A and B of stream s (-1: of every stream) from host or
 * device memory: scroll_batch_set_dyn_refs and _device */
int dyn_set_refs(ScrollBatch *b, int s, const uint8_t *ref_a, const uint8_t *ref_b, hipMemcpyKind kind)
{
    if (!b || !b->dyn_on || !ref_a || !ref_b || s < -1 || s >= b->nstreams) return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    const bool dev = kind == hipMemcpyDeviceToDevice;
    /* device pictures may come from work queued on any stream, and the copy
     * from them must have landed before the next compose on any stream */
    if (dev) HIPCHK(hipDeviceSynchronize());
    const size_t pic = (size_t)3 * b->dyn_pw * b->dyn_ph / 2, pair = dyn_pair_bytes(b);
    if (s >= 0 && b->dyn_refs == 1)                      /* shared -> per stream */
        for (int k = 1; k < b->nstreams; ++k)
            HIPCHK(hipMemcpy(b->d_refs + k * pair, b->d_refs, pair, hipMemcpyDeviceToDevice));
    uint8_t *dst = b->d_refs + (s < 0 ? 0 : (size_t)s * pair);
    HIPCHK(hipMemcpy(dst, ref_a, pic, kind));
    HIPCHK(hipMemcpy(dst + pic, ref_b, pic, kind));
    if (dev) HIPCHK(hipDeviceSynchronize());
    if (s < 0) {
        b->dyn_refs = 1;
        b->geo.ref_ld = 0;
    } else {
        b->dyn_refs = 2;
        b->geo.ref_ld = pair;
    }
    return SCROLL_OK;
}

uint32_t dyn_pos_word(const ScrollBatch *b, size_t i)
{
    const int32_t x = b->h_dyn_pos[2 * i], y = b->h_dyn_pos[2 * i + 1];
    if (x < 0) return DYN_POS_NONE;
    const bool sz = !b->h_dyn_dsz.empty();
    return dyn_pos_pack((uint32_t)x, (uint32_t)y, sz ? b->h_dyn_dsz[2 * i] : 0u, sz ? b->h_dyn_dsz[2 * i + 1] : 0u);
}

int dyn_sizes_any(ScrollBatch *b, bool *any)
{
    *any = false;
    if (!b->dyn_on || !b->dsz_on) return SCROLL_OK;
    const int rc = dyn_pos_refresh(b);
    if (rc) return rc;
    *any = b->dsz_any != 0;
    return SCROLL_OK;
}

int dyn_sizes_enable(ScrollBatch *b, const char *who)
{
    if (!b->dyn_moving) {
        set_err("%s: a frame's own size needs scroll_batch_set_dyn_rect_moving", who);
        return SCROLL_ERR_CONFIG;
    }
    if (b->geo.pos_mask != 0xffu) {
        set_err("%s: a frame's own size needs a picture of at most 256 x 256 MBs (the table word's origin bytes)", who);
        return SCROLL_ERR_CONFIG;
    }
    if (b->dsz_on) return SCROLL_OK;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    if (b->pb.run.fin) HIPCHK(hipEventSynchronize(b->pb.run.fin));     /* a probe on another stream */
    if (b->dpos_ev) HIPCHK(hipEventSynchronize(b->dpos_ev));   /* an upload or a locate */
    DynGeom g = b->geo;
    dyn_rowstage_geom(&g, b->dyn_pw / 16, b->dyn_ph / 16, 2);
    const size_t S = (size_t)b->max_streams, F = (size_t)b->max_frames;
    const size_t rs_words = S * F * g.rs_frame_words + (size_t)g.rs_spill_cap * g.rs_spill_words;
    uint32_t *rs = nullptr, *gbits = nullptr;
    hipError_t e = hipMalloc(&rs, rs_words * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&gbits, S * F * (size_t)g.ld_groups * sizeof(uint32_t));
    if (e != hipSuccess) {
        (void)hipFree(rs);
        (void)hipFree(gbits);
        return hip_fail(who, e, true);
    }
    (void)hipFree(b->dx.rowstage);
    (void)hipFree(b->dx.gbits);
    b->dx.rowstage = rs;
    b->dx.spill = rs + S * F * g.rs_frame_words;
    b->dx.gbits = gbits;
    g.dpos = nullptr;
    b->geo = g;
    b->h_dyn_dsz.assign(2 * S * F, 0);
    b->dsz_nz = 0;
    b->dsz_any = 0;
    b->dsz_on = 1;
    return SCROLL_OK;
}

int dyn_pos_table(ScrollBatch *b, hipStream_t hs, const uint32_t **dpos)
{
    *dpos = nullptr;
    if (!b->dyn_on || !b->dyn_moving || b->hint_on) return SCROLL_OK;
    /* (a table a locate has written, dpos_dev, is never stale: it is handed
     * out below as the device left it, nothing uploaded over it) */
    if (b->dpos_stale) {
        /* the last upload has read its source */
        if (b->dpos_hs) HIPCHK(hipEventSynchronize(b->dpos_ev));
        const size_t n = (size_t)b->max_streams * b->max_frames;
        b->h_dpos.resize(n);
        bool any = false;
        for (size_t i = 0; i < n; ++i) {
            const int32_t x = b->h_dyn_pos[2 * i], y = b->h_dyn_pos[2 * i + 1];
            any |= x != b->geo.x0 || (x >= 0 && y != b->geo.y0);
            b->h_dpos[i] = dyn_pos_word(b, i);
        }
        any |= b->dsz_any != 0;                         /* a frame sized on its own */
        b->dpos_hs = nullptr;
        if (any) {
            HIPCHK(hipMemcpyAsync(b->d_dpos, b->h_dpos.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, hs));
            HIPCHK(hipEventRecord(b->dpos_ev, hs));
            b->dpos_hs = hs;
        }
        b->dpos_any = any ? 1 : 0;
        b->dpos_stale = 0;
    }
    if (!b->dpos_any) return SCROLL_OK;
    if (hs != b->dpos_hs) HIPCHK(hipStreamWaitEvent(hs, b->dpos_ev, 0));   /* uploaded on another stream */
    *dpos = b->d_dpos;
    return SCROLL_OK;
}

}  // namespace batch
}  // namespace scroll

extern "C" {

/* ------------------------------ dynamic rect ----------------------------- */
int scroll_batch_set_dyn_rect(ScrollBatch *b, int x0, int y0, int w, int h, size_t slot_bytes)
{
    if (!b || x0 < 0 || y0 < 0 || w < 0 || h < 0) return SCROLL_ERR_ARG;
    if (b->hint_on && b->sp_n > 0 && w > 0 && h > 0) {
        set_err("scroll_batch_set_dyn_rect: not combinable with spliced slices (clear them first)");
        return SCROLL_ERR_CONFIG;
    }
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    dyn_release(b);
    if (w == 0 || h == 0) return SCROLL_OK;
    if (b->nstreams == 0) {
        set_err("scroll_batch_set_dyn_rect: add the streams first");
        return SCROLL_ERR_ARG;
    }
    const int pw = b->h_st[0].w, ph = b->h_st[0].h;
    for (int s = 1; s < b->nstreams; ++s)
        if (b->h_st[s].w != pw || b->h_st[s].h != ph) {
            set_err("scroll_batch_set_dyn_rect: streams of one batch must share the picture size");
            return SCROLL_ERR_CONFIG;
        }
    const int mbw = pw / 16, mbh = ph / 16;
    /* prediction rows are byte offsets into a reference pair below 2^28 */
    if ((pw & 15) || (ph & 15) || x0 + w > mbw || y0 + h > mbh || w > DYN_MAX_W || h > DYN_MAX_H ||
        mbw > DYN_MAX_MBW || mbh > DYN_MAX_MBH ||
        (size_t)3 * pw * ph >= ((size_t)1 << 28)) {
        set_err("scroll_batch_set_dyn_rect: rect (%d,%d %dx%d MBs) not supported in %dx%d", x0, y0,
                w, h, pw, ph);
        return SCROLL_ERR_CONFIG;
    }
    DynGeom g{};
    g.x0 = x0;
    g.y0 = y0;
    g.pw = pw;
    g.ph = ph;
    g.w = g.ld_w = w;
    g.h = g.ld_h = h;
    /* origins below 256 leave a table word's high bytes to the frames' sizes */
    g.pos_mask = mbw <= 256 && mbh <= 256 ? 0xffu : 0xffffu;
    g.qp = b->dyn_qp;
    g.ql = scroll::dyn::qparams(g.qp);
    g.qc = scroll::dyn::qparams(scroll::dyn::qp_chroma(g.qp));
    g.src_fr = (uint64_t)384 * w * h;
    g.src_ld = round256((size_t)b->max_frames * g.src_fr);
    g.ref_ld = 0;
    g.slot_bytes = slot_bytes ? round256(slot_bytes + DYN_OVF_BYTES) : dyn_slot_bound(mbw, mbh, w, h);
    g.ep_cap = dyn_ep_cap(w, h, b->debug);
    dyn_rowstage_geom(&g, mbw, mbh, 0);                /* ngroups = ld_groups: this placement's */
    b->dyn_pw = pw;
    b->dyn_ph = ph;
    const size_t S = (size_t)b->max_streams, F = (size_t)b->max_frames;
    hipError_t e = hipSuccess;
    if (!b->hint_on) {                 /* with hints: the hint path's DynFrames and slots */
        e = hipMalloc(&b->d_dfr, S * F * sizeof(DynFrame));
        /* the RBSP is never staged (k_dyn_epfix / k_dyn_emit_gather read the
         * row groups): per frame only its EP list; slot_bytes stays the cap */
        if (e == hipSuccess) e = hipMalloc(&b->d_stage, S * F * (size_t)4 * g.ep_cap);
        if (e == hipSuccess) e = hipMemset(b->d_dfr, 0, S * F * sizeof(DynFrame));
    }
    if (e == hipSuccess) e = hipMalloc(&b->d_src, S * g.src_ld);
    if (e == hipSuccess) e = hipMalloc(&b->d_refs, S * dyn_pair_bytes(b));
    if (e == hipSuccess) e = hipMalloc(&b->dx.rows, S * F * 32 * h * sizeof(uint32_t));
    /* scratch sized for typical content: general-path record
     * slots for 1/64 of the frames (those NALs need half-pel chroma steps the
     * composer's own waypoints never make), spill slots for 1/32 of the rect
     * rows; a compose that runs out fails the frames concerned with
     * SCROLL_ERR_OVERFLOW and the next compose has pools at their bound */
    g.gen_cap = (uint32_t)std::min(S * F, std::max<size_t>(32, S * F / 64));
    g.rs_spill_cap = g.rs_row_words < g.rs_spill_words
                         ? (uint32_t)std::min(S * F * (size_t)h, std::max<size_t>(2048, S * F * (size_t)h / 32))
                         : 0u;
    g.rs_frames = (uint32_t)(S * F);
    if (b->dyn_grow) {                 /* pools at their bounds (ran out before) */
        g.gen_cap = (uint32_t)(S * F);
        if (g.rs_spill_cap) g.rs_spill_cap = (uint32_t)(S * F * (size_t)h);
    }
    const size_t nrec = (size_t)g.gen_cap * DYN_PIECES * w * h;
    if (e == hipSuccess) e = hipMalloc(&b->dx.meta, nrec * sizeof(uint16_t));
    if (e == hipSuccess) e = hipMalloc(&b->dx.body_lo, nrec * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(&b->dx.body_hi, nrec * sizeof(uint2));
    if (e == hipSuccess) e = hipMalloc(&b->dx.body_w, nrec * sizeof(uint4));
    const size_t ng = (size_t)g.ld_groups;
    if (e == hipSuccess) e = hipMalloc(&b->dx.heads, S * F * DYN_HEAD_VECS * sizeof(uint4));
    if (e == hipSuccess) e = hipMalloc(&b->dx.tcx, S * F * w * h * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(b->dx.tcx, 0, S * F * w * h * sizeof(unsigned long long));
    const size_t rs_words = S * F * g.rs_frame_words + (size_t)g.rs_spill_cap * g.rs_spill_words;
    if (e == hipSuccess) e = hipMalloc(&b->dx.rowstage, rs_words * sizeof(uint32_t));
    if (e == hipSuccess) b->dx.spill = b->dx.rowstage + S * F * g.rs_frame_words;
    /* counters and the general-record list (dyn_engine.h) */
    if (e == hipSuccess) e = hipMalloc(&b->dx.ctr, (DYN_CTR_LIST + S * F) * sizeof(uint32_t));
    b->dx.ctr_frames = (uint32_t)(S * F);
    if (e == hipSuccess) e = hipMalloc(&b->dx.gbits, S * F * ng * sizeof(uint32_t));
    b->dx.epoch = 0;
    if (e == hipSuccess) e = hipMemset(b->d_src, 0, S * g.src_ld);
    if (e == hipSuccess) e = hipMemset(b->d_refs, 0, S * dyn_pair_bytes(b));
    if (e != hipSuccess) {
        dyn_release(b);
        return hip_fail("scroll_batch_set_dyn_rect", e);
    }
    b->dyn_cap = g.slot_bytes;
    if (b->hint_on) g.slot_bytes = b->geo.slot_bytes;   /* the hint path's slots (grown by hd_setup) */
    b->geo = g;
    b->dyn_on = 1;
    b->h_dyn_pos.assign(2 * S * F, 0);
    b->h_dyn_qp.assign(S * F, -1);
    for (size_t i = 0; i < S * F; ++i) {
        b->h_dyn_pos[2 * i] = x0;
        b->h_dyn_pos[2 * i + 1] = y0;
    }
    b->dyn_pos_custom = 0;
    b->hd_mb_words = slot_bytes == 0 ? HDYN_MB_WORDS_DEFAULT
                                     : (uint32_t)std::min<size_t>(HDYN_MB_WORDS_MAX,
                                                                  std::max<size_t>(HDYN_MB_WORDS_MIN,
                                                                                   slot_bytes / (4 * (size_t)w * h)));
    if (b->hint_on) return hd_setup(b);
    return SCROLL_OK;
}

int scroll_batch_set_dyn_rect_at(ScrollBatch *b, int s, int f, int x0, int y0)
{
    if (!b || !b->dyn_on || s < 0 || s >= b->nstreams || f < 0 || f >= b->max_frames) {
        set_err("scroll_batch_set_dyn_rect_at: no dynamic rect, or stream / frame out of range");
        return SCROLL_ERR_ARG;
    }
    const int mbw = b->dyn_pw / 16, mbh = b->dyn_ph / 16;
    if (x0 >= 0 && (y0 < 0 || x0 + b->geo.w > mbw || y0 + b->geo.h > mbh)) {
        set_err("scroll_batch_set_dyn_rect_at: rect at (%d, %d) leaves the picture", x0, y0);
        return SCROLL_ERR_ARG;
    }
    int rc = batch_host_sync(b);
    if (rc) return rc;
    /* with moving rects a probe on a stream of its own may still read the device table */
    if (b->dyn_moving && b->pb.run.fin) HIPCHK(hipEventSynchronize(b->pb.run.fin));
    /* positions a locate placed on the device stay, all but this one */
    if ((rc = dyn_pos_refresh(b))) return rc;
    const size_t i = (size_t)s * b->max_frames + f;
    b->h_dyn_pos[2 * i] = x0 < 0 ? -1 : x0;
    b->h_dyn_pos[2 * i + 1] = x0 < 0 ? -1 : y0;
    if (x0 != b->geo.x0 || (x0 >= 0 && y0 != b->geo.y0)) b->dyn_pos_custom = 1;
    b->dpos_stale = 1;
    b->hd_dirty = 1;
    b->hint_dirty = 1;
    return SCROLL_OK;
}

/* The plain rect placed per stream and per frame: on, a
 * compose without hints honours scroll_batch_set_dyn_rect_at's positions on
 * the k_dyn_row path.  A frame's row groups change in number with y0, so the
 * row stage (every frame's region, the static groups' slots) and the groups'
 * bit counts are sized here, once, for every legal y0: no later position
 * allocates.  Off: back to the batch position's sizes.  The flag goes with
 * the rect (scroll_batch_set_dyn_rect drops it). */
int scroll_batch_set_dyn_rect_moving(ScrollBatch *b, int on)
{
    if (!b) return SCROLL_ERR_ARG;
    if (!b->dyn_on) {
        if (!on) return SCROLL_OK;
        set_err("scroll_batch_set_dyn_rect_moving: needs a dynamic rect (scroll_batch_set_dyn_rect)");
        return SCROLL_ERR_CONFIG;
    }
    if ((on != 0) == (b->dyn_moving != 0)) return SCROLL_OK;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    if (b->pb.run.fin) HIPCHK(hipEventSynchronize(b->pb.run.fin));     /* a probe on another stream */
    if (b->dpos_ev) HIPCHK(hipEventSynchronize(b->dpos_ev));
    if ((rc = dyn_pos_refresh(b))) return rc;                   /* located positions outlive the table */
    if (!on && b->dsz_on) {                                     /* sizes need the flag: they go with it */
        b->h_dyn_dsz.clear();
        b->dsz_nz = 0;
        b->dsz_any = 0;
        b->dsz_on = 0;
    }
    DynGeom g = b->geo;
    dyn_rowstage_geom(&g, b->dyn_pw / 16, b->dyn_ph / 16, on ? 1 : 0);
    const size_t S = (size_t)b->max_streams, F = (size_t)b->max_frames;
    const size_t rs_words = S * F * g.rs_frame_words + (size_t)g.rs_spill_cap * g.rs_spill_words;
    uint32_t *rs = nullptr, *gbits = nullptr, *dpos = nullptr;
    hipEvent_t ev = nullptr;
    hipError_t e = hipMalloc(&rs, rs_words * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&gbits, S * F * (size_t)g.ld_groups * sizeof(uint32_t));
    if (e == hipSuccess && on) e = hipMalloc(&dpos, S * F * sizeof(uint32_t));
    if (e == hipSuccess && on) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipFree(rs);
        (void)hipFree(gbits);
        (void)hipFree(dpos);
        return hip_fail("scroll_batch_set_dyn_rect_moving", e, true);
    }
    (void)hipFree(b->dx.rowstage);
    (void)hipFree(b->dx.gbits);
    (void)hipFree(b->d_dpos);
    if (b->dpos_ev) (void)hipEventDestroy(b->dpos_ev);
    b->dx.rowstage = rs;
    b->dx.spill = rs + S * F * g.rs_frame_words;
    b->dx.gbits = gbits;
    b->d_dpos = dpos;
    b->dpos_ev = ev;
    b->dpos_hs = nullptr;
    b->dpos_stale = 1;
    b->dpos_any = 0;
    g.dpos = nullptr;
    b->geo = g;
    b->dyn_moving = on ? 1 : 0;
    return SCROLL_OK;
}

/* The plain rect sized per stream and per frame: frame f of
 * stream s codes w x h MBs at its own origin.  The table's word carries the
 * difference to the batch's size, so a batch that never calls this uploads
 * the words it always did. */
int scroll_batch_set_dyn_rect_size_at(ScrollBatch *b, int s, int f, int w, int h)
{
    const char *who = "scroll_batch_set_dyn_rect_size_at";
    if (!b || !b->dyn_on || s < 0 || s >= b->nstreams || f < 0 || f >= b->max_frames) {
        set_err("%s: no dynamic rect, or stream / frame out of range", who);
        return SCROLL_ERR_ARG;
    }
    if (w < 1 || w > b->geo.w || h < 1 || h > b->geo.h) {
        set_err("%s: size %d x %d outside 1..%d x 1..%d (scroll_batch_set_dyn_rect's size)", who, w, h, b->geo.w,
                b->geo.h);
        return SCROLL_ERR_ARG;
    }
    int rc = dyn_sizes_enable(b, who);
    if (rc) return rc;
    if ((rc = batch_host_sync(b))) return rc;
    /* a probe on a stream of its own may still read the device table */
    if (b->pb.run.fin) HIPCHK(hipEventSynchronize(b->pb.run.fin));
    /* what a locate placed on the device stays, all but this frame's size */
    if ((rc = dyn_pos_refresh(b))) return rc;
    const size_t i = (size_t)s * b->max_frames + f;
    const bool was = (b->h_dyn_dsz[2 * i] | b->h_dyn_dsz[2 * i + 1]) != 0, is = w != b->geo.w || h != b->geo.h;
    b->h_dyn_dsz[2 * i] = (uint8_t)(b->geo.w - w);
    b->h_dyn_dsz[2 * i + 1] = (uint8_t)(b->geo.h - h);
    b->dsz_nz = b->dsz_nz - (was ? 1 : 0) + (is ? 1 : 0);      /* no scan of the other frames' entries */
    b->dsz_any = b->dsz_nz ? 1 : 0;
    b->dpos_stale = 1;
    return SCROLL_OK;
}

/* the conventional-encode fallback (docs/MASTER_DESIGN.md:220): needs the
 * dynamic rect to be the whole picture, so that every frame's source is a
 * whole picture a conventional encoder would have */
int scroll_batch_set_fallback(ScrollBatch *b, int on)
{
    if (!b) return SCROLL_ERR_ARG;
    if (on && (!b->dyn_on || b->geo.x0 != 0 || b->geo.y0 != 0 || b->geo.w != b->dyn_pw / 16 ||
               b->geo.h != b->dyn_ph / 16)) {
        set_err("scroll_batch_set_fallback: needs the dynamic rect to be the whole picture "
                "(scroll_batch_set_dyn_rect(b, 0, 0, width / 16, height / 16, ...))");
        return SCROLL_ERR_CONFIG;
    }
    int rc = batch_host_sync(b);
    if (rc) return rc;
    b->fallback = on ? 1 : 0;
    b->hd_dirty = 1;
    return SCROLL_OK;
}

int scroll_batch_fallback_frame(ScrollBatch *b, int s, int f, int *fell_back)
{
    if (!b || !fell_back || s < 0 || s >= b->nstreams || f < 0 || f >= b->max_frames) return SCROLL_ERR_ARG;
    *fell_back = 0;
    if (!b->hint_on || !b->d_hf) return SCROLL_OK;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HintFrame H;
    HIPCHK(hipMemcpy(&H, b->d_hf + (size_t)s * b->max_frames + f, sizeof(H), hipMemcpyDeviceToHost));
    *fell_back = (H.mode & HINT_MODE_FB) ? 1 : 0;
    return SCROLL_OK;
}

int scroll_batch_set_dyn_refs(ScrollBatch *b, int s, const uint8_t *ref_a, const uint8_t *ref_b)
{
    return dyn_set_refs(b, s, ref_a, ref_b, hipMemcpyHostToDevice);
}

int scroll_batch_set_dyn_source(ScrollBatch *b, const uint8_t *src, int nframes)
{
    if (!b || !b->dyn_on || !src || nframes < 0 || nframes > b->max_frames) return SCROLL_ERR_ARG;
    if (nframes == 0) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    const size_t row = (size_t)nframes * b->geo.src_fr;
    HIPCHK(hipMemcpy2D(b->d_src, b->geo.src_ld, src, row, row, (size_t)b->nstreams,
                       hipMemcpyHostToDevice));
    return SCROLL_OK;
}

uint8_t *scroll_batch_dyn_source_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride)
{
    if (!b || !b->dyn_on) return nullptr;
    if (stream_stride) *stream_stride = b->geo.src_ld;
    if (frame_stride) *frame_stride = b->geo.src_fr;
    return b->d_src;
}

int scroll_batch_dyn_source_synth(ScrollBatch *b, int nframes, int stream_base, int t0)
{
    if (!b || !b->dyn_on || nframes < 0 || nframes > b->max_frames) return SCROLL_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    /* with moving rects every frame's pattern is the one of its own position (a frame without a rect: the origin's) */
    DynGeom G = b->geo;
    int rc = dyn_pos_table(b, b->own, &G.dpos);
    if (rc) return rc;
    if (dyn_launch_synth(b->own, nframes, b->nstreams, b->d_src, &G, b->max_frames, stream_base, t0)) {
        set_err("k_dyn_synth launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    HIPCHK(hipStreamSynchronize(b->own));
    return SCROLL_OK;
}

int scroll_batch_dyn_frame_info(ScrollBatch *b, int s, int f, uint32_t *rbsp_bytes,
                                uint32_t *ep_bytes)
{
    if (!b || !(b->dyn_on || b->hint_on) || s < 0 || s >= b->nstreams || f < 0 ||
        f >= b->max_frames)
        return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    DynFrame d;
    HIPCHK(hipMemcpy(&d, b->d_dfr + (size_t)s * b->max_frames + f, sizeof(d),
                     hipMemcpyDeviceToHost));
    if (rbsp_bytes) *rbsp_bytes = d.rbsp_bytes;
    if (ep_bytes) *ep_bytes = d.ep;
    return d.nal < 0 ? 1 : SCROLL_OK;
}

int scroll_batch_dyn_totals(ScrollBatch *b, unsigned long long *rbsp_bytes,
                            unsigned long long *ep_bytes, long long *dyn_nals)
{
    if (!b || !(b->dyn_on || b->hint_on)) return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    const size_t S = (size_t)b->nstreams, F = (size_t)b->max_frames;
    std::vector<DynFrame> v(S * F);
    HIPCHK(hipMemcpy(v.data(), b->d_dfr, v.size() * sizeof(DynFrame), hipMemcpyDeviceToHost));
    unsigned long long r = 0, e = 0;
    long long n = 0;
    for (size_t s = 0; s < S; ++s)
        for (int f = 0; f < b->last_nframes; ++f) {
            const DynFrame &d = v[s * F + (size_t)f];
            if (d.nal < 0) continue;
            r += d.rbsp_bytes;
            e += d.ep;
            n++;
        }
    if (rbsp_bytes) *rbsp_bytes = r;
    if (ep_bytes) *ep_bytes = e;
    if (dyn_nals) *dyn_nals = n;
    return SCROLL_OK;
}

/* the rect's QP of stream s (every stream: s < 0); with the deblocking
 * filter on (no deblocking_filter_control_present_flag: ingested streams may
 * have it) a QP other than 26 would change the filtering of the scroll
 * region's MBs (their QP follows the slice / the coded MBs before them), so
 * it is refused for such streams */
static int set_stream_qp(ScrollBatch *b, int s, int qp, const char *who)
{
    if (!b || qp < SCROLL_DYN_QP_MIN || qp > SCROLL_DYN_QP_MAX || s >= b->nstreams) {
        set_err("%s: QP %d outside %d..%d or stream %d out of range", who, qp, SCROLL_DYN_QP_MIN,
                SCROLL_DYN_QP_MAX, s);
        return SCROLL_ERR_ARG;
    }
    const int s0 = s < 0 ? 0 : s, s1 = s < 0 ? b->nstreams : s + 1;
    for (int k = s0; k < s1; ++k)
        if (qp != 26 && !b->h_st[k].deblock) {
            set_err("%s: stream %d has the deblocking filter on (no "
                    "deblocking_filter_control_present_flag): its rect codes at QP 26", who, k);
            return SCROLL_ERR_CONFIG;
        }
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    for (int k = s0; k < s1; ++k) {
        b->h_st[k].dyn_qp = qp;
        HIPCHK(hipMemcpy(&b->d_st[k].dyn_qp, &qp, sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (s < 0) b->dyn_qp = qp;         /* streams added later */
    b->hd_dirty = 1;                   /* under hints: frames without their own QP follow the stream */
    return SCROLL_OK;
}

int scroll_batch_set_dyn_qp(ScrollBatch *b, int qp)
{
    return set_stream_qp(b, -1, qp, "scroll_batch_set_dyn_qp");
}

int scroll_batch_set_dyn_qp_stream(ScrollBatch *b, int s, int qp)
{
    if (!b || s < 0) {
        set_err("scroll_batch_set_dyn_qp_stream: bad stream");
        return SCROLL_ERR_ARG;
    }
    return set_stream_qp(b, s, qp, "scroll_batch_set_dyn_qp_stream");
}

int scroll_batch_set_dyn_qp_at(ScrollBatch *b, int s, int f, int qp)
{
    if (!b || !b->hint_on || !b->dyn_on || s < 0 || s >= b->nstreams || f < 0 || f >= b->max_frames ||
        qp < -1 || qp > SCROLL_DYN_QP_MAX) {
        set_err("scroll_batch_set_dyn_qp_at: needs UI hints and the dynamic rect (without hints: "
                "scroll_batch_set_dyn_qp_frames); stream / frame / QP (-1, 0..%d) out of range", SCROLL_DYN_QP_MAX);
        return SCROLL_ERR_ARG;
    }
    if (qp >= 0 && qp != 26 && !b->h_st[s].deblock) {
        set_err("scroll_batch_set_dyn_qp_at: stream %d has the deblocking filter on: its rect codes at QP 26",
                s);
        return SCROLL_ERR_CONFIG;
    }
    int rc = batch_host_sync(b);
    if (rc) return rc;
    const size_t i = (size_t)s * b->max_frames + f;
    if (b->h_dyn_qp.size() < (size_t)b->max_streams * b->max_frames)
        b->h_dyn_qp.assign((size_t)b->max_streams * b->max_frames, -1);
    b->h_dyn_qp[i] = qp;
    b->hd_dirty = 1;
    return SCROLL_OK;
}

/* ------------------- the dynamic rect's reconstruction -------------------- */
int scroll_batch_set_dyn_recon(ScrollBatch *b, int on)
{
    if (!b) return SCROLL_ERR_ARG;
    if (on && !b->dyn_on) {
        set_err("scroll_batch_set_dyn_recon: needs a dynamic rect (scroll_batch_set_dyn_rect)");
        return SCROLL_ERR_CONFIG;
    }
    if ((on != 0) == (b->recon_on != 0)) return SCROLL_OK;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    if (!on) {
        (void)hipFree(b->d_rec);
        (void)hipFree(b->d_sse);
        b->d_rec = nullptr;
        b->d_sse = nullptr;
        b->recon_on = 0;
        b->recon_hinted = 0;
        return SCROLL_OK;
    }
    const size_t S = (size_t)b->max_streams, F = (size_t)b->max_frames;
    hipError_t e = hipMalloc(&b->d_rec, S * b->geo.src_ld);
    if (e == hipSuccess) e = hipMalloc(&b->d_sse, S * F * 3 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(b->d_rec, 0, S * b->geo.src_ld);
    if (e == hipSuccess) e = hipMemset(b->d_sse, 0, S * F * 3 * sizeof(unsigned long long));
    if (e != hipSuccess) {
        (void)hipFree(b->d_rec);
        (void)hipFree(b->d_sse);
        b->d_rec = nullptr;
        b->d_sse = nullptr;
        return hip_fail("scroll_batch_set_dyn_recon", e, true);
    }
    b->recon_on = 1;
    b->rc_timed = 0;
    b->rc_last_hint = 0;
    return SCROLL_OK;
}

int scroll_batch_set_dyn_recon_hinted(ScrollBatch *b, int on)
{
    if (!b) return SCROLL_ERR_ARG;
    if (on && !b->recon_on) {
        set_err("scroll_batch_set_dyn_recon_hinted: needs the reconstruction on (scroll_batch_set_dyn_recon)");
        return SCROLL_ERR_CONFIG;
    }
    int rc = batch_host_sync(b);
    if (rc) return rc;
    if (on) b->rc_fail.resize((size_t)b->max_streams, 0);   /* sized here, not on the compose path */
    b->recon_hinted = on ? 1 : 0;
    return SCROLL_OK;
}

uint8_t *scroll_batch_dyn_recon_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride)
{
    if (!b || !b->recon_on) return nullptr;
    if (stream_stride) *stream_stride = b->geo.src_ld;
    if (frame_stride) *frame_stride = b->geo.src_fr;
    return b->d_rec;
}

/* frame f of the last compose: 0 it has a reconstruction, 1 no dynamic NAL,
 * < 0 not available */
static int recon_frame(ScrollBatch *b, int s, int f, const char *who)
{
    if (!b) return SCROLL_ERR_ARG;
    if (!b->recon_on) {
        set_err("%s: the reconstruction is off (scroll_batch_set_dyn_recon)", who);
        return SCROLL_ERR_CONFIG;
    }
    if (s < 0 || s >= b->nstreams || f < 0 || f >= b->last_nframes) {
        set_err("%s: stream %d / frame %d outside the last compose", who, s, f);
        return SCROLL_ERR_ARG;
    }
    int rc = batch_host_sync(b);
    if (rc) return rc;
    const size_t fi = (size_t)s * b->max_frames + f;
    DynFrame d;
    if (b->rc_last_hint) {
        /* a hinted compose: a stream that failed has no reconstruction to
         * show (its error bits, or what scroll_batch_sync made of them) */
        const int e = b->h_st[s].err ? stream_fail_code(b, s) : ((size_t)s < b->rc_fail.size() ? b->rc_fail[s] : 0);
        if (e) {
            set_err("%s: stream %d failed in the last compose (status %d): no reconstruction", who, s, e);
            return e;
        }
        HIPCHK(hipMemcpy(&d, b->d_dfr + fi, sizeof(d), hipMemcpyDeviceToHost));
        if (d.nal < 0 || !b->d_spf || !b->d_hf) return 1;
        SpliceFrame sf;
        HintFrame hfr;
        HIPCHK(hipMemcpy(&sf, b->d_spf + fi, sizeof(sf), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&hfr, b->d_hf + fi, sizeof(hfr), hipMemcpyDeviceToHost));
        /* no rect in the frame, or a dormant fallback region in a frame that did not fall back */
        if (sf.w <= 0 || ((sf.pad & 1) && !(hfr.mode & HINT_MODE_FB))) return 1;
        return SCROLL_OK;
    }
    HIPCHK(hipMemcpy(&d, b->d_dfr + fi, sizeof(d), hipMemcpyDeviceToHost));
    if (d.nal < 0) return 1;
    /* DynFrame.err bits DF_OVER | DF_HANDOFF (dyn_kernels.hip): the frame was not coded */
    if (d.err & 5u) {
        set_err("%s: stream %d frame %d failed in the dynamic-rect coder: nothing was coded", who, s, f);
        return SCROLL_ERR_OVERFLOW;
    }
    return SCROLL_OK;
}

int scroll_batch_dyn_recon(ScrollBatch *b, int s, int f, uint8_t *dst)
{
    if (!dst) return SCROLL_ERR_ARG;
    int rc = recon_frame(b, s, f, "scroll_batch_dyn_recon");
    if (rc) return rc;
    HIPCHK(hipMemcpy(dst, b->d_rec + (size_t)s * b->geo.src_ld + (size_t)f * b->geo.src_fr, b->geo.src_fr,
                     hipMemcpyDeviceToHost));
    return SCROLL_OK;
}

int scroll_batch_dyn_sse(ScrollBatch *b, int s, int f, uint64_t sse[3])
{
    if (!sse) return SCROLL_ERR_ARG;
    int rc = recon_frame(b, s, f, "scroll_batch_dyn_sse");
    if (rc) return rc;
    unsigned long long v[3];
    HIPCHK(hipMemcpy(v, b->d_sse + ((size_t)s * b->max_frames + f) * 3, sizeof(v), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; ++k) sse[k] = v[k];
    return SCROLL_OK;
}

float scroll_batch_dyn_recon_ms(ScrollBatch *b)
{
    if (!b || !b->recon_on || !b->rc_timed) return -1.0f;
    if (batch_host_sync(b)) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, b->rc_ev[0], b->rc_ev[1]) != hipSuccess) {
        (void)hipGetLastError();
        return -1.0f;
    }
    return ms;
}

/* ------------------- probing the rect at candidate QPs -------------------- */
int scroll_batch_dyn_probe(ScrollBatch *b, int nframes, const uint8_t *qps, int nq, void *hip_stream)
{
    ProbeQps Q{};
    int rc = probe_args(b, "scroll_batch_dyn_probe", nframes, qps, nq, &Q);
    if (rc) return rc;
    if (b->hint_on) {
        set_err("scroll_batch_dyn_probe: covers the plain dynamic rect, not the rect under UI hints: "
                "clear the hints");
        return SCROLL_ERR_CONFIG;
    }
    HIPCHK(hipSetDevice(b->device));
    if ((rc = probe_alloc(b))) return rc;
    ScrollBatch::Probe &p = b->pb;
    const int ld_fr = b->max_frames;
    /* k_dyn_rows after the state pass, into the probe's own rows / heads / ctr */
    return probe_run(b, nframes, Q, hip_stream, 0, p.pr.ctr, [&](hipStream_t hs, int S, DynGeom &G, hipEvent_t ev1) {
        /* (no per-frame QP table: the probe's QPs are its arguments) */
        const int rr = pred_rows_launch(b, hs, nframes, p.plan, p.pr, &G);
        if (rr) return rr;
        if (probe_launch(hs, nframes, S, b->d_st, p.plan.nal, b->ld_nal, p.plan.pend, p.plan.dfr, ld_fr, &G,
                         p.pr.rows, b->d_src, b->d_refs, &Q, p.res, p.done, p.pr.ctr, nullptr, ev1)) {
            set_err("k_dyn_probe launch: %s", hipGetErrorString(hipGetLastError()));
            return SCROLL_ERR_HIP;
        }
        return SCROLL_OK;
    });
}

/* The same question for the rect under UI hints: what the next compose's
 * k_hdyn_code would make of every frame (its hint rects, its own rect
 * position, the fallback), at candidate QPs instead of the frames' own.  The
 * uploads are the ones that compose would do anyway; the plan goes into the
 * probe's own NalDesc / DynFrame / PlanPending and the frames' classes into
 * a buffer of the probe's own, so that nothing of the batch's state, of the
 * last compose's results or of its fallback flags changes. */
int scroll_batch_dyn_probe_hinted(ScrollBatch *b, int nframes, const uint8_t *qps, int nq, void *hip_stream)
{
    ProbeQps Q{};
    int rc = probe_args(b, "scroll_batch_dyn_probe_hinted", nframes, qps, nq, &Q);
    if (rc) return rc;
    if (!b->hint_on) {
        set_err("scroll_batch_dyn_probe_hinted: covers the rect under UI hints (scroll_batch_set_hints); "
                "the plain dynamic rect is scroll_batch_dyn_probe's");
        return SCROLL_ERR_CONFIG;
    }
    bool spliced = b->sp_n > 0;
    for (const ScrollBatch::SpliceHost &sp : b->h_sp) spliced |= sp.w > 0;
    if (spliced) {
        set_err("scroll_batch_dyn_probe_hinted: a spliced slice carries MB types the probe does not follow: "
                "clear the splices");
        return SCROLL_ERR_CONFIG;
    }
    HIPCHK(hipSetDevice(b->device));
    bool sized = false;
    if ((rc = dyn_sizes_any(b, &sized))) return rc;
    if (sized) {
        set_err("scroll_batch_dyn_probe_hinted: a frame has a size of its own (scroll_batch_set_dyn_rect_size_at), "
                "which the rect under UI hints does not follow: clear the hints or the sizes");
        return SCROLL_ERR_CONFIG;
    }
    if (b->hd_dirty && (rc = hd_upload(b))) return rc;
    if (b->hint_dirty && (rc = hint_upload(b))) return rc;
    if ((rc = probe_alloc(b))) return rc;
    ScrollBatch::Probe &p = b->pb;
    if (!p.cls) {
        hipError_t e = hipMalloc(&p.cls, (size_t)b->max_streams * (size_t)b->max_frames);
        if (e != hipSuccess) return hip_fail("scroll_batch_dyn_probe_hinted", e, true);
    }
    const int ld_fr = b->max_frames;
    /* no k_dyn_rows after the state pass (the motion is the hints'), and no counters for it to zero */
    return probe_run(b, nframes, Q, hip_stream, 1, nullptr, [&](hipStream_t hs, int S, DynGeom &G, hipEvent_t ev1) {
        if (hprobe_launch(hs, nframes, S, b->d_st, p.plan.nal, b->ld_nal, p.plan.pend, p.plan.dfr, ld_fr, b->d_hf,
                          b->d_pool, b->d_spf, b->fallback, &G, b->d_src, b->d_refs, &Q, p.cls, p.res, p.done, ev1)) {
            set_err("k_hdyn_probe launch: %s", hipGetErrorString(hipGetLastError()));
            return SCROLL_ERR_HIP;
        }
        return SCROLL_OK;
    });
}

int scroll_batch_dyn_probe_result(ScrollBatch *b, int s, int f, int k, ScrollDynProbe *out)
{
    if (!b || !out) return SCROLL_ERR_ARG;
    ScrollBatch::Probe &p = b->pb;
    /* (the range message names the candidate too: pass_frame_arg's first half only) */
    const int rc = pass_have(&p.run, "scroll_batch_dyn_probe_result", "probe", "scroll_batch_dyn_probe");
    if (rc) return rc;
    if (s < 0 || s >= p.run.nstreams || f < 0 || f >= p.run.nframes || k < 0 || k >= p.nq) {
        set_err("scroll_batch_dyn_probe_result: stream %d / frame %d / candidate %d outside the last probe", s, f, k);
        return SCROLL_ERR_ARG;
    }
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipEventSynchronize(p.run.fin));
    const size_t fi = (size_t)s * b->max_frames + f;
    DynFrame d;
    HIPCHK(hipMemcpy(&d, p.plan.dfr + fi, sizeof(d), hipMemcpyDeviceToHost));
    if (d.nal < 0) return 1;
    if (p.hinted) {
        uint8_t c = 0;
        HIPCHK(hipMemcpy(&c, p.cls + fi, 1, hipMemcpyDeviceToHost));
        if (c == HPROBE_NONE) return 1;
        if (c == HPROBE_FAIL) {
            set_err("scroll_batch_dyn_probe_result: stream %d frame %d: a hint rect names a reference the frame "
                    "lacks and the fallback is off (the compose would fail the stream)", s, f);
            return SCROLL_ERR_CONFIG;
        }
    }
    uint32_t rows_in = 0;
    HIPCHK(hipMemcpy(&rows_in, p.done + fi, sizeof(rows_in), hipMemcpyDeviceToHost));
    if (rows_in != (uint32_t)b->geo.h) {
        set_err("scroll_batch_dyn_probe_result: stream %d frame %d: %u of %d rect rows counted", s, f, rows_in,
                b->geo.h);
        return SCROLL_ERR_DEVICE;
    }
    HIPCHK(hipMemcpy(out, p.res + fi * SCROLL_DYN_PROBE_MAX_QPS + k, sizeof(*out), hipMemcpyDeviceToHost));
    return SCROLL_OK;
}

const ScrollDynProbe *scroll_batch_dyn_probe_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride)
{
    if (!b || !b->pb.res) return nullptr;
    if (frame_stride) *frame_stride = SCROLL_DYN_PROBE_MAX_QPS * sizeof(ScrollDynProbe);
    if (stream_stride) *stream_stride = (size_t)b->max_frames * SCROLL_DYN_PROBE_MAX_QPS * sizeof(ScrollDynProbe);
    return b->pb.res;
}

float scroll_batch_dyn_probe_ms(ScrollBatch *b) { return b ? pass_span_ms(b, &b->pb.run, 0, 1) : -1.0f; }

}  // extern "C"
