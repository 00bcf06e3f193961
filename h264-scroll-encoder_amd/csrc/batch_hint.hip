/*
 * batch_hint.hip -- the batch engine's hint path (batch.h): UI hints, the
 * dynamic rect under hints (record pools and per-frame positions) and the
 * pre-encoded MB splice that rides on it.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "batch.h"
#include "hint_engine.h"
#include "splice_engine.h"

using namespace scroll::batch;

/* --------------------------------- UI hints -------------------------------- */
static void hint_release(ScrollBatch *b)
{
    (void)hipFree(b->d_dfr);
    (void)hipFree(b->d_stage);
    (void)hipFree(b->d_hf);
    (void)hipFree(b->d_pool);
    b->d_dfr = nullptr;
    b->d_stage = nullptr;
    b->d_hf = nullptr;
    b->d_pool = nullptr;
    b->pool_cap = 0;
    b->hint_on = 0;
    b->hint_dirty = 0;
    b->h_hint.clear();
    b->h_hint_mode.clear();
    (void)hipFree(b->d_spf);
    (void)hipFree(b->d_sp_nal);
    (void)hipFree(b->d_sp_rbsp);
    (void)hipFree(b->d_sp_rec);
    (void)hipFree(b->d_sp_list);
    (void)hipFree(b->d_sp_units);
    (void)hipFree(b->d_sp_lanes);
    b->d_spf = nullptr;
    b->d_sp_nal = nullptr;
    b->d_sp_rbsp = nullptr;
    b->d_sp_rec = nullptr;
    b->d_sp_list = nullptr;
    b->d_sp_units = nullptr;
    b->d_sp_lanes = nullptr;
    b->sp_nal_cap = b->sp_rbsp_cap = b->sp_rec_cap = b->sp_list_cap = b->sp_units_cap = b->sp_lanes_cap = 0;
    b->sp_nslots = 0;
    b->h_sp.clear();
    b->sp_n = 0;
    b->sp_dirty = 0;
    b->sp_parse = 0;
}

namespace scroll {
namespace batch {

/* host hint tables -> d_hf (per frame) + d_pool (all rects) */
int hint_upload(ScrollBatch *b)
{
    int prc = dyn_pos_refresh(b);      /* positions a locate placed before the hints came */
    if (prc) return prc;
    const size_t n = b->h_hint.size();
    std::vector<HintFrame> hf(n);
    std::vector<ScrollHintRect> pool;
    for (size_t i = 0; i < n; ++i) {
        hf[i].first = (int32_t)pool.size();
        hf[i].n = (int16_t)b->h_hint[i].size();
        hf[i].mode = b->h_hint_mode[i];
        if (i < b->h_sp.size() && b->h_sp[i].w > 0) hf[i].mode |= HINT_MODE_SPLICED;
        if (b->dyn_on && 2 * i < b->h_dyn_pos.size() && b->h_dyn_pos[2 * i] >= 0)
            hf[i].mode |= HINT_MODE_SPLICED;   /* the rect's MBs: k_hdyn_code's records */
        pool.insert(pool.end(), b->h_hint[i].begin(), b->h_hint[i].end());
    }
    int rc = dev_grow((void **)&b->d_pool, &b->pool_cap, pool.size(), sizeof(ScrollHintRect),
                      "scroll_batch_compose: hint rects");
    if (rc) return rc;
    HIPCHK(hipMemcpy(b->d_hf, hf.data(), n * sizeof(HintFrame), hipMemcpyHostToDevice));
    if (!pool.empty())
        HIPCHK(hipMemcpy(b->d_pool, pool.data(), pool.size() * sizeof(ScrollHintRect),
                         hipMemcpyHostToDevice));
    b->hint_dirty = 0;
    return SCROLL_OK;
}

/* the dynamic rect under hints: record / word pools for every frame's rect
 * MBs, staging slots grown to the largest NAL such a frame composes */
int hd_setup(ScrollBatch *b)
{
    const size_t S = (size_t)b->max_streams, F = (size_t)b->max_frames;
    const size_t nmb = (size_t)b->geo.w * b->geo.h;
    const size_t words = S * F * nmb * b->hd_mb_words + 2 + RBSP_SLACK_WORDS;   /* + the stage's look-ahead */
    int rc;
    if (!b->d_spf) {
        HIPCHK(hipMalloc(&b->d_spf, S * F * sizeof(SpliceFrame)));
        HIPCHK(hipMemset(b->d_spf, 0, S * F * sizeof(SpliceFrame)));
    }
    if ((rc = dev_grow((void **)&b->d_sp_rbsp, &b->sp_rbsp_cap, words, sizeof(uint32_t), "splice")) ||
        (rc = dev_grow((void **)&b->d_sp_rec, &b->sp_rec_cap, S * F * nmb, sizeof(SpliceMbRec), "splice")))
        return rc;
    const size_t slot = splice_slot_bound(b->dyn_pw / 16, b->dyn_ph / 16, b->geo.w, b->geo.h,
                                          nmb * 4 * b->hd_mb_words);
    if (slot > b->geo.slot_bytes) {
        void *ns = nullptr;
        hipError_t e = hipMalloc(&ns, S * F * slot);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_err("dynamic rect under hints: staging (%zu bytes per frame): %s", slot,
                    hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? SCROLL_ERR_OOM : SCROLL_ERR_HIP;
        }
        (void)hipFree(b->d_stage);
        b->d_stage = (uint8_t *)ns;
        b->geo.slot_bytes = slot;
    }
    b->hd_dirty = 1;
    b->hint_dirty = 1;
    return SCROLL_OK;
}

/* every frame's rect position -> d_spf (records and words at fixed places) */
int hd_upload(ScrollBatch *b)
{
    const size_t S = (size_t)b->max_streams, F = (size_t)b->max_frames;
    const size_t nmb = (size_t)b->geo.w * b->geo.h;
    int prc = dyn_pos_refresh(b);      /* positions a locate placed before the hints came */
    if (prc) return prc;
    std::vector<SpliceFrame> spf(S * F);
    for (size_t i = 0; i < S * F; ++i) {
        SpliceFrame &o = spf[i];
        o = SpliceFrame{};
        const bool dormant = b->h_dyn_pos[2 * i] < 0;
        if (dormant && !b->fallback) continue;
        /* the fallback: a frame without the rect keeps a dormant whole-picture
         * region (pad 1) that k_hdyn_code codes only if k_hint_fb marks it */
        o.x0 = dormant ? 0 : b->h_dyn_pos[2 * i];
        o.y0 = dormant ? 0 : b->h_dyn_pos[2 * i + 1];
        o.pad = dormant ? 1 : 0;
        o.w = b->geo.w;
        o.h = b->geo.h;
        o.rbsp_word = i * nmb * b->hd_mb_words;
        o.rec_first = (uint32_t)(i * nmb);
        const int fq = i < b->h_dyn_qp.size() ? b->h_dyn_qp[i] : -1;
        const size_t st = i / F;
        o.hd_qp = fq >= 0 ? fq : (st < (size_t)b->nstreams ? b->h_st[st].dyn_qp : b->dyn_qp);
    }
    HIPCHK(hipMemcpy(b->d_spf, spf.data(), S * F * sizeof(SpliceFrame), hipMemcpyHostToDevice));
    b->hd_dirty = 0;
    return SCROLL_OK;
}

/* host splices -> device (table, NAL pool, pools sized for the parse) and
 * staging slots grown to the largest spliced NAL's bound; k_splice_parse
 * runs on the next compose's stream */
int splice_upload(ScrollBatch *b)
{
    const size_t S = (size_t)b->max_streams, F = (size_t)b->max_frames;
    std::vector<SpliceFrame> spf(S * F);
    for (SpliceFrame &o : spf) o.hd_qp = -1;             /* spliced slices keep their own QP chain */
    std::vector<int32_t> list;
    std::vector<uint8_t> pool;
    size_t words = 0, recs = 0, nunits = 0, slot = b->geo.slot_bytes;
    int ymax = 1;
    std::vector<size_t> pool_off(b->h_sp.size(), 0);
    for (size_t i = 0; i < b->h_sp.size(); ++i) {
        const ScrollBatch::SpliceHost &h = b->h_sp[i];
        SpliceFrame &o = spf[i];
        o = SpliceFrame{};
        o.hd_qp = -1;
        if (h.w <= 0) continue;
        o.x0 = h.x0;
        o.y0 = h.y0;
        o.w = h.w;
        o.h = h.h;
        o.nal_len = (uint32_t)h.n;
        o.rbsp_word = words;
        o.rec_first = (uint32_t)recs;
        if (!h.dnal) {                 /* host bytes -> the NAL pool */
            pool_off[i] = pool.size();
            pool.insert(pool.end(), h.nal.begin(), h.nal.end());
            pool.resize((pool.size() + 3) & ~(size_t)3);
        }
        words += (h.n + 3) / 4 + 2;    /* k_splice_parse's units stay below (len + 2) / 4 + 1 words */
        recs += (size_t)h.w * h.h;
        o.unit_first = (uint32_t)nunits;
        nunits += splice_unit_cap(h.w * h.h);
        ymax = std::max(ymax, (int)splice_unit_cap(h.w * h.h));
        list.push_back((int32_t)i);
        const DevStream &d = b->h_st[i / F];
        slot = std::max(slot, splice_slot_bound(d.w / 16, d.h / 16, h.w, h.h, h.n));
    }
    int rc;
    if (!b->d_spf) {
        HIPCHK(hipMalloc(&b->d_spf, S * F * sizeof(SpliceFrame)));
    }
    const char *who = "splice";
    if ((rc = dev_grow((void **)&b->d_sp_nal, &b->sp_nal_cap, pool.size(), 1, who)) ||
        (rc = dev_grow((void **)&b->d_sp_rbsp, &b->sp_rbsp_cap, words + RBSP_SLACK_WORDS, sizeof(uint32_t), who)) ||
        (rc = dev_grow((void **)&b->d_sp_rec, &b->sp_rec_cap, recs, sizeof(SpliceMbRec), who)) ||
        (rc = dev_grow((void **)&b->d_sp_list, &b->sp_list_cap, list.size(), sizeof(int32_t), who)) ||
        (rc = dev_grow((void **)&b->d_sp_units, &b->sp_units_cap, nunits, sizeof(SpliceUnit), who)))
        return rc;
    if (1 + 2 * nunits > b->sp_lanes_cap) {
        if ((rc = dev_grow((void **)&b->d_sp_lanes, &b->sp_lanes_cap, 1 + 2 * nunits, sizeof(int32_t), who))) return rc;
        HIPCHK(hipMemset(b->d_sp_lanes, 0, sizeof(int32_t)));     /* k_splice_fix keeps it zero after */
    }
    b->sp_nslots = nunits;
    if (slot > b->geo.slot_bytes) {
        /* the new slots first: on failure the old ones, the hints and the
         * splices stay as they were (sp_dirty stays set: the next compose
         * tries again, or the caller clears / shrinks the splices) */
        void *ns = nullptr;
        hipError_t e = hipMalloc(&ns, S * F * slot);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_err("scroll_batch_compose: splice staging (%zu bytes per frame): %s", slot,
                    hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? SCROLL_ERR_OOM : SCROLL_ERR_HIP;
        }
        (void)hipFree(b->d_stage);
        b->d_stage = (uint8_t *)ns;
        b->geo.slot_bytes = slot;
    }
    for (size_t i = 0; i < b->h_sp.size(); ++i)
        if (b->h_sp[i].w > 0) spf[i].nal = b->h_sp[i].dnal ? b->h_sp[i].dnal : b->d_sp_nal + pool_off[i];
    HIPCHK(hipMemcpy(b->d_spf, spf.data(), S * F * sizeof(SpliceFrame), hipMemcpyHostToDevice));
    if (!pool.empty())
        HIPCHK(hipMemcpy(b->d_sp_nal, pool.data(), pool.size(), hipMemcpyHostToDevice));
    if (!list.empty())
        HIPCHK(hipMemcpy(b->d_sp_list, list.data(), list.size() * sizeof(int32_t),
                         hipMemcpyHostToDevice));
    b->sp_n = (int)list.size();
    b->sp_ymax = ymax;
    b->sp_parse = b->sp_n > 0;
    b->sp_dirty = 0;
    return SCROLL_OK;
}

int splice_frame_status(ScrollBatch *b, size_t i, int *status)
{
    *status = SCROLL_SPLICE_OK;
    const bool on = (i < b->h_sp.size() && b->h_sp[i].w > 0) ||
                    (b->hint_on && b->dyn_on && 2 * i < b->h_dyn_pos.size() && b->h_dyn_pos[2 * i] >= 0);
    if (!b->d_spf || !on) return SCROLL_OK;
    SpliceFrame sf;
    HIPCHK(hipMemcpy(&sf, b->d_spf + i, sizeof(sf), hipMemcpyDeviceToHost));
    *status = sf.status ? sf.status : sf.stage_status;
    return SCROLL_OK;
}

const char *splice_msg(int e)
{
    switch (e) {
    case SCROLL_SPLICE_ERR_NAL: return "not a coded slice of an IDR or non-IDR picture (or more than 1,024 slices)";
    case SCROLL_SPLICE_ERR_HEADER: return "slice header outside the supported syntax, or slices out of order";
    case SCROLL_SPLICE_ERR_MBTYPE: return "an intra MB whose prediction reads other samples in the composed picture";
    case SCROLL_SPLICE_ERR_SYNTAX: return "malformed or truncated slice data, or slices not covering the rect's MBs";
    case SCROLL_SPLICE_ERR_REF: return "a ref_idx that is not a valid reference of the frame";
    default: return "unknown";
    }
}

}  // namespace batch
}  // namespace scroll

extern "C" {

int scroll_batch_set_hints(ScrollBatch *b, int s, int f, const ScrollHintRect *rects, int n,
                           int mode)
{
    if (!b || s < 0 || s >= b->nstreams || f < 0 || f >= b->max_frames || n < 0 ||
        n > SCROLL_HINT_MAX_RECTS || (n > 0 && !rects) ||
        (mode != SCROLL_HINT_EXACT && mode != SCROLL_HINT_PSKIP && mode != SCROLL_HINT_SPEC)) {
        set_err("scroll_batch_set_hints: bad arguments");
        return SCROLL_ERR_ARG;
    }
    for (int i = 0; i < n; ++i) {
        const ScrollHintRect &r = rects[i];
        if (r.ref < 0 || r.ref >= 2 + 8 || r.mv_x < -SCROLL_HINT_MAX_MV ||
            r.mv_x > SCROLL_HINT_MAX_MV || r.mv_y < -SCROLL_HINT_MAX_MV ||
            r.mv_y > SCROLL_HINT_MAX_MV) {
            set_err("scroll_batch_set_hints: rect %d: ref %d / mv (%d, %d) out of range", i,
                    r.ref, r.mv_x, r.mv_y);
            return SCROLL_ERR_ARG;
        }
    }
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    if (!b->hint_on) {
        int mb = 0;
        for (int k = 0; k < b->nstreams; ++k) {
            mb = std::max(mb, (b->h_st[k].w / 16) * (b->h_st[k].h / 16));
            if (b->h_st[k].w / 16 > HINT_MAX_MBW) {
                set_err("scroll_batch_set_hints: stream %d is wider than %d MBs", k, HINT_MAX_MBW);
                return SCROLL_ERR_CONFIG;
            }
        }
        const size_t slot = hint_slot_bound(1, mb);     /* slots from the MB count only */
        const size_t S = (size_t)b->max_streams, F = (size_t)b->max_frames;
        hipError_t e = hipSuccess;
        if (b->dyn_on) {
            /* the dynamic rect's DynFrames stay; its EP-list buffer becomes
             * the hint path's staging slots (hd_setup grows them for the rect) */
            void *ns = nullptr;
            e = hipMalloc(&ns, S * F * slot);
            if (e == hipSuccess) e = hipMalloc(&b->d_hf, S * F * sizeof(HintFrame));
            if (e != hipSuccess) {
                (void)hipFree(ns);
                (void)hipFree(b->d_hf);
                b->d_hf = nullptr;
                return hip_fail("scroll_batch_set_hints", e, true);
            }
            (void)hipFree(b->d_stage);
            b->d_stage = (uint8_t *)ns;
        } else {
            e = hipMalloc(&b->d_dfr, S * F * sizeof(DynFrame));
            if (e == hipSuccess) e = hipMalloc(&b->d_stage, S * F * slot);
            if (e == hipSuccess) e = hipMalloc(&b->d_hf, S * F * sizeof(HintFrame));
            if (e == hipSuccess) e = hipMemset(b->d_dfr, 0, S * F * sizeof(DynFrame));
            if (e != hipSuccess) {
                hint_release(b);
                return hip_fail("scroll_batch_set_hints", e);
            }
            b->geo = DynGeom{};
        }
        b->geo.slot_bytes = slot;
        b->hint_max_mb = mb;
        b->h_hint.assign(S * F, {});
        b->h_hint_mode.assign(S * F, (int16_t)SCROLL_HINT_EXACT);
        b->hint_on = 1;
        if (b->dyn_on && (rc = hd_setup(b))) return rc;
    }
    const size_t i = (size_t)s * b->max_frames + f;
    b->h_hint[i].assign(rects, rects + n);
    b->h_hint_mode[i] = (int16_t)mode;
    b->hint_dirty = 1;
    return SCROLL_OK;
}

int scroll_batch_clear_hints(ScrollBatch *b)
{
    if (!b) return SCROLL_ERR_ARG;
    if (!b->hint_on) return SCROLL_OK;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    hint_release(b);
    if (b->dyn_on) {                   /* the dynamic rect alone again: its DynFrames + EP lists */
        const size_t S = (size_t)b->max_streams, F = (size_t)b->max_frames;
        hipError_t e = hipMalloc(&b->d_dfr, S * F * sizeof(DynFrame));
        if (e == hipSuccess) e = hipMalloc(&b->d_stage, S * F * (size_t)4 * b->geo.ep_cap);
        if (e == hipSuccess) e = hipMemset(b->d_dfr, 0, S * F * sizeof(DynFrame));
        if (e != hipSuccess) {
            dyn_release(b);
            return hip_fail("scroll_batch_clear_hints", e);
        }
        b->geo.slot_bytes = b->dyn_cap;
        if (b->dyn_pos_custom || b->dpos_dev || b->dsz_any) {   /* (located positions and sizes go too, unread) */
            if (b->dpos_dev) HIPCHK(hipEventSynchronize(b->dpos_ev));
            b->dpos_dev = 0;
            for (size_t i = 0; i < S * F; ++i) {
                b->h_dyn_pos[2 * i] = b->geo.x0;
                b->h_dyn_pos[2 * i + 1] = b->geo.y0;
            }
            std::fill(b->h_dyn_dsz.begin(), b->h_dyn_dsz.end(), (uint8_t)0);   /* sizes go with the positions */
            b->dsz_nz = 0;
            b->dsz_any = 0;
            b->dyn_pos_custom = 0;
            b->dpos_stale = 1;
        }
    }
    return SCROLL_OK;
}

/* ------------------------- pre-encoded MB splice --------------------------- */
int scroll_batch_set_splice(ScrollBatch *b, int s, int f, int x0, int y0, int w, int h,
                            const uint8_t *nal, size_t n)
{
    if (!b || s < 0 || s >= b->nstreams || f < 0 || f >= b->max_frames ||
        (n > 0 && (!nal || w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || n >= SCROLL_SPLICE_MAX_BYTES))) {
        set_err("scroll_batch_set_splice: bad arguments");
        return SCROLL_ERR_ARG;
    }
    if (n > 0 && (x0 + w > b->h_st[s].w / 16 || y0 + h > b->h_st[s].h / 16)) {
        set_err("scroll_batch_set_splice: rect (%d, %d) %dx%d MBs outside the %dx%d picture", x0,
                y0, w, h, b->h_st[s].w, b->h_st[s].h);
        return SCROLL_ERR_ARG;
    }
    if (b->dyn_on) {
        set_err("scroll_batch_set_splice: not combinable with a dynamic rect (one spliced rect per frame)");
        return SCROLL_ERR_CONFIG;
    }
    if (n == 0 && !b->hint_on) return SCROLL_OK;
    if (!b->hint_on) {                 /* the splice rides on the hint path, SPEC by default */
        int rc = scroll_batch_set_hints(b, s, f, nullptr, 0, SCROLL_HINT_SPEC);
        if (rc) return rc;
        std::fill(b->h_hint_mode.begin(), b->h_hint_mode.end(), (int16_t)SCROLL_HINT_SPEC);
    } else {
        int rc = batch_host_sync(b);
        if (rc) return rc;
    }
    const size_t i = (size_t)s * b->max_frames + f;
    if (b->h_sp.size() < (size_t)b->max_streams * b->max_frames)
        b->h_sp.resize((size_t)b->max_streams * b->max_frames);
    ScrollBatch::SpliceHost &sp = b->h_sp[i];
    if (n == 0) {
        sp = ScrollBatch::SpliceHost{};
    } else {
        sp.x0 = x0;
        sp.y0 = y0;
        sp.w = w;
        sp.h = h;
        sp.nal.assign(nal, nal + n);
        sp.dnal = nullptr;
        sp.n = n;
    }
    b->sp_dirty = 1;
    b->hint_dirty = 1;
    return SCROLL_OK;
}

int scroll_batch_set_splices_device(ScrollBatch *b, int n, const ScrollSpliceDesc *d)
{
    if (!b || n < 0 || (n > 0 && !d)) {
        set_err("scroll_batch_set_splices_device: bad arguments");
        return SCROLL_ERR_ARG;
    }
    for (int k = 0; k < n; ++k) {
        const ScrollSpliceDesc &e = d[k];
        const bool on = e.n > 0;
        if (e.s < 0 || e.s >= b->nstreams || e.f < 0 || e.f >= b->max_frames ||
            (on && (!e.nal || e.w <= 0 || e.h <= 0 || e.x0 < 0 || e.y0 < 0 ||
                    e.n >= SCROLL_SPLICE_MAX_BYTES || e.x0 + e.w > b->h_st[e.s].w / 16 ||
                    e.y0 + e.h > b->h_st[e.s].h / 16))) {
            set_err("scroll_batch_set_splices_device: entry %d: bad stream / frame / rect / size", k);
            return SCROLL_ERR_ARG;
        }
    }
    if (n == 0) return SCROLL_OK;
    if (b->dyn_on) {
        set_err("scroll_batch_set_splices_device: not combinable with a dynamic rect (one spliced rect per frame)");
        return SCROLL_ERR_CONFIG;
    }
    if (!b->hint_on) {
        int rc = scroll_batch_set_hints(b, d[0].s, d[0].f, nullptr, 0, SCROLL_HINT_SPEC);
        if (rc) return rc;
        std::fill(b->h_hint_mode.begin(), b->h_hint_mode.end(), (int16_t)SCROLL_HINT_SPEC);
    } else {
        int rc = batch_host_sync(b);
        if (rc) return rc;
    }
    if (b->h_sp.size() < (size_t)b->max_streams * b->max_frames)
        b->h_sp.resize((size_t)b->max_streams * b->max_frames);
    for (int k = 0; k < n; ++k) {
        const ScrollSpliceDesc &e = d[k];
        ScrollBatch::SpliceHost &sp = b->h_sp[(size_t)e.s * b->max_frames + e.f];
        sp = ScrollBatch::SpliceHost{};
        if (e.n == 0) continue;
        sp.x0 = e.x0;
        sp.y0 = e.y0;
        sp.w = e.w;
        sp.h = e.h;
        sp.dnal = e.nal;
        sp.n = (size_t)e.n;
    }
    b->sp_dirty = 1;
    b->hint_dirty = 1;
    return SCROLL_OK;
}

int scroll_batch_clear_splices(ScrollBatch *b)
{
    if (!b) return SCROLL_ERR_ARG;
    if (b->h_sp.empty()) return SCROLL_OK;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    b->h_sp.clear();
    b->sp_dirty = 1;
    b->hint_dirty = 1;
    return SCROLL_OK;
}

int scroll_batch_splice_status(ScrollBatch *b, int s, int f, int *status)
{
    if (!b || !status || s < 0 || s >= b->nstreams || f < 0 || f >= b->max_frames)
        return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    return splice_frame_status(b, (size_t)s * b->max_frames + f, status);
}

int scroll_batch_splice_refusal(ScrollBatch *b, int s, int f, int *status, int *mb_x, int *mb_y, int *mb_type)
{
    if (!b || !status || s < 0 || s >= b->nstreams || f < 0 || f >= b->max_frames)
        return SCROLL_ERR_ARG;
    int rc = batch_host_sync(b);
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    const size_t i = (size_t)s * b->max_frames + f;
    rc = splice_frame_status(b, i, status);
    if (rc) return rc;
    int x = -1, y = -1, t = -1;
    if (*status == SCROLL_SPLICE_ERR_MBTYPE && b->d_spf) {
        SpliceFrame sf;
        HIPCHK(hipMemcpy(&sf, b->d_spf + i, sizeof(sf), hipMemcpyDeviceToHost));
        if (sf.bad_mb >= 0 && sf.w > 0) {
            const int m = sf.bad_mb & 0xffff;
            x = m % sf.w;
            y = m / sf.w;
            t = sf.bad_mb >> 16;
        }
    }
    if (mb_x) *mb_x = x;
    if (mb_y) *mb_y = y;
    if (mb_type) *mb_type = t;
    return SCROLL_OK;
}

}  // extern "C"
