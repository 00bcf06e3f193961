/*
 * batch_dropin.hip -- synchronous helpers for the drop-in entry points
 * (engine.h): one process-wide batch, composed and read back under a lock.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "batch.h"

using namespace scroll::batch;

static std::mutex g_mu;

struct TempBatch {
    ScrollBatch *b = nullptr;
    int streams = 0, frames = 0;
    size_t arena = 0;
    int mode = -1;
};
static TempBatch g_tmp;

static int temp_batch(int streams, int frames, size_t arena, int mode, ScrollBatch **out)
{
    TempBatch &t = g_tmp;
    if (!t.b || t.streams < streams || t.frames < frames || t.arena < arena || t.mode != mode) {
        if (t.b) scroll_batch_destroy(t.b);
        t.b = nullptr;
        ScrollBatchDesc d;
        d.device = 0;
        std::vector<int> ids;
        if (!usable_devices(&ids)) return SCROLL_ERR_NO_DEVICE;
        d.device = ids[0];
        d.max_streams = streams > t.streams ? streams : t.streams;
        d.max_frames = frames > t.frames ? frames : t.frames;
        d.arena_bytes = arena > t.arena ? arena : t.arena;
        d.mode = mode;
        int rc = scroll_batch_create(&t.b, &d);
        if (rc) return rc;
        t.streams = d.max_streams;
        t.frames = d.max_frames;
        t.arena = d.arena_bytes;
        t.mode = mode;
    }
    t.b->nstreams = 0;
    t.b->host_valid = 1;
    *out = t.b;
    return SCROLL_OK;
}

static size_t round_arena(size_t n)
{
    size_t a = 1u << 20;
    while (a < n) a <<= 1;
    return a;
}

extern "C" {

int scroll_engine_write_nals(const ComposerConfig *cfg, const NalDesc *nals, int n,
                             uint8_t *dst, size_t cap, size_t *written)
{
    std::lock_guard<std::mutex> lk(g_mu);
    *written = 0;
    int rc = check_cfg(cfg);
    if (rc) return rc;
    ScrollBatch *b;
    rc = temp_batch(1, n, round_arena(cap), SCROLL_MODE_COMPOSER, &b);
    if (rc) return rc;
    DevStream *d = &b->h_st[0];
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
    d->out_cap = cap;
    d->nnal = n;
    b->nstreams = 1;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpyAsync(b->d_st, d, sizeof(DevStream), hipMemcpyHostToDevice, b->own));
    HIPCHK(hipMemcpyAsync(b->d_nal, nals, (size_t)n * sizeof(NalDesc), hipMemcpyHostToDevice,
                          b->own));
    rc = launch(b, 0, SCROLL_PLAN_EXPLICIT, n, b->own);
    if (rc) return rc;
    rc = scroll_batch_sync(b);
    if (rc) return rc;
    size_t tot = (size_t)b->h_st[0].out_pos;
    HIPCHK(hipMemcpy(dst, b->d_arena, tot, hipMemcpyDeviceToHost));
    *written = tot;
    return SCROLL_OK;
}

int scroll_engine_compose(ComposerConfig *const *cfgs, const int *const *offs, const int *frames,
                          int nstreams, int mode, uint8_t *const *dsts, const size_t *caps,
                          size_t *written, int **wp_offsets_out)
{
    std::lock_guard<std::mutex> lk(g_mu);
    int fmax = 0;
    size_t cmax = 0;
    for (int i = 0; i < nstreams; ++i) {
        written[i] = 0;
        int rc = check_cfg(cfgs[i]);
        if (rc) return rc;
        if (frames[i] > fmax) fmax = frames[i];
        if (caps[i] > cmax) cmax = caps[i];
    }
    if (nstreams == 0 || fmax == 0) return SCROLL_OK;
    ScrollBatch *b;
    int rc = temp_batch(nstreams, fmax, round_arena(cmax), mode, &b);
    if (rc) return rc;
    std::vector<int32_t> off((size_t)nstreams * fmax, 0);
    for (int i = 0; i < nstreams; ++i) {
        DevStream *d = &b->h_st[i];
        memset(d, 0, sizeof(*d));
        cfg_to_dev(cfgs[i], d);
        d->out_pos = 0;
        d->out_cap = caps[i];
        d->frames = frames[i];
        memcpy(&off[(size_t)i * fmax], offs[i], (size_t)frames[i] * sizeof(int32_t));
    }
    b->nstreams = nstreams;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpyAsync(b->d_st, b->h_st, (size_t)nstreams * sizeof(DevStream),
                          hipMemcpyHostToDevice, b->own));
    HIPCHK(hipMemcpy2DAsync(b->d_off, (size_t)b->max_frames * sizeof(int32_t), off.data(),
                            (size_t)fmax * sizeof(int32_t), (size_t)fmax * sizeof(int32_t),
                            (size_t)nstreams, hipMemcpyHostToDevice, b->own));
    int plan = mode == SCROLL_MODE_EXPERIMENT ? SCROLL_PLAN_EXPERIMENT : SCROLL_PLAN_COMPOSER;
    rc = launch(b, -1, plan, plan == SCROLL_PLAN_COMPOSER ? 2 * fmax : fmax, b->own);
    if (rc) return rc;
    rc = scroll_batch_sync(b);
    if (rc) return rc;
    if (wp_offsets_out) {
        rc = load_nals(b);
        if (rc) return rc;
    }
    for (int i = 0; i < nstreams; ++i) {
        size_t tot = (size_t)b->h_st[i].out_pos;
        if (tot) {
            HIPCHK(hipMemcpy(dsts[i], b->d_arena + (size_t)i * b->ld_arena, tot,
                             hipMemcpyDeviceToHost));
        }
        written[i] = tot;
        dev_to_cfg(&b->h_st[i], cfgs[i]);
        if (wp_offsets_out && wp_offsets_out[i]) {
            int k = 0;
            for (int j = 0; j < b->h_st[i].nnal; ++j) {
                const NalDesc &nd = b->nal_cache[(size_t)i * b->ld_nal + j];
                if (nd.kind == 1) wp_offsets_out[i][k++] = nd.off;
            }
            wp_offsets_out[i][k] = -1;
        }
    }
    return SCROLL_OK;
}

}  // extern "C"
