/*
 * batch_ingest.hip -- the batch engine's way in for pre-encoded references
 * (batch.h): stream ingest, I_PCM reference files from pictures, and
 * mid-stream reference updates.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "batch.h"
#include "hint_engine.h"        /* HINT_MAX_MBW: the hint slots an ingested stream must fit */
#include "ingest_engine.h"
#include "ipcm_engine.h"

using namespace scroll::batch;

/* ------------------------------ stream ingest ------------------------------ */
static const char *ing_msg(int e)
{
    switch (e) {
    case ING_ERR_MISSING: return "reference file missing SPS/PPS/IDR";
    case ING_ERR_PARSE: return "unsupported SPS/PPS (scaling matrices, POC type 1 or slice groups)";
    case ING_ERR_DIMS: return "reference frame dimensions don't match";
    case ING_ERR_NALS: return "too many NAL units in a reference file";
    case ING_ERR_OVERFLOW: return "header larger than the stream arena";
    case ING_ERR_WAIT: return "a segment of the header waited too long for the one before it";
    default: return "ingest failed";
    }
}

/* the per-file scratch of n streams' ingest or n reference updates
 * (d_ing_files, d_ing_scan, d_ing_out) */
static int ing_reserve(ScrollBatch *b, int n, const char *who)
{
    if (n <= b->ing_cap) return SCROLL_OK;
    (void)hipFree(b->d_ing_files);
    (void)hipFree(b->d_ing_scan);
    (void)hipFree(b->d_ing_out);
    b->d_ing_files = nullptr;
    b->d_ing_scan = nullptr;
    b->d_ing_out = nullptr;
    b->ing_cap = 0;
    hipError_t e = hipMalloc(&b->d_ing_files, 2 * (size_t)n * sizeof(IngestFile));
    if (e == hipSuccess) e = hipMalloc(&b->d_ing_scan, 2 * (size_t)n * sizeof(IngestScan));
    if (e == hipSuccess) e = hipMalloc(&b->d_ing_out, (size_t)n * sizeof(IngestOut));
    if (e != hipSuccess) return hip_fail(who, e);
    b->ing_cap = n;
    return SCROLL_OK;
}

/* d_ing_in, where the host entry points put their files, at tot bytes */
static int ing_in_reserve(ScrollBatch *b, size_t tot, const char *who)
{
    return dev_grow((void **)&b->d_ing_in, &b->ing_in_cap, tot, 1, who);
}

namespace scroll {
namespace batch {

/* the asynchronous I_PCM calls' outcome (scroll_batch_sync): their overflow
 * flag, after the stream is idle */
int ipcm_async_check(ScrollBatch *b)
{
    if (!b->ipcm_over) return SCROLL_OK;
    uint32_t over = 0;
    HIPCHK(hipStreamSynchronize(b->own));
    HIPCHK(hipMemcpy(&over, b->ipcm_over, sizeof(over), hipMemcpyDeviceToHost));
    b->ipcm_over = nullptr;
    if (over) {
        set_err("scroll_batch_ipcm_files_device_async: a file exceeded out_stride (%zu bytes): "
                "its call wrote no file", b->ipcm_over_stride);
        return SCROLL_ERR_OVERFLOW;
    }
    return SCROLL_OK;
}

}  // namespace batch
}  // namespace scroll

extern "C" {

int scroll_batch_ingest_device(ScrollBatch *b, int n, const uint8_t *d_files, const uint64_t *desc,
                               int *first)
{
    if (!b || n < 0 || (n > 0 && (!d_files || !desc))) return SCROLL_ERR_ARG;
    if (b->nstreams + n > b->max_streams) {
        set_err("scroll_batch_ingest: %d + %d streams exceed the batch (%d)", b->nstreams, n,
                b->max_streams);
        return SCROLL_ERR_ARG;
    }
    int rc = batch_host_sync(b);
    if (rc) return rc;
    if (first) *first = b->nstreams;
    if (n == 0) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    if ((rc = ing_reserve(b, n, "scroll_batch_ingest"))) return rc;
    std::vector<IngestFile> files(2 * (size_t)n);
    uint64_t maxf = 0, totf = 0;
    for (int k = 0; k < 2 * n; ++k) {
        files[k].off = desc[2 * k];
        files[k].size = desc[2 * k + 1];
        maxf = std::max(maxf, files[k].size);
        totf += files[k].size;
    }
    const bool serial = getenv("SCROLL_INGEST_SERIAL") != nullptr;
    /* the one-pass segments (default); round 4's three passes for
     * comparison (tests): SCROLL_INGEST_THREEPASS=1 stages the output bytes
     * while that scratch (every file sized like the largest, ~1.25x per
     * segment) stays within 4x the input plus 256 MB and under 8 GB, and
     * otherwise -- or with SCROLL_INGEST_RECOMPUTE=1 -- decodes again */
    int mode = ING_ONEPASS;
    if (getenv("SCROLL_INGEST_THREEPASS") || getenv("SCROLL_INGEST_RECOMPUTE")) {
        const size_t stg_bytes = ingest_work_bytes(n, maxf, ING_STAGED);
        mode = getenv("SCROLL_INGEST_RECOMPUTE") == nullptr && stg_bytes <= ((size_t)8 << 30) &&
                       stg_bytes <= 4 * (size_t)totf + ((size_t)256 << 20)
                   ? ING_STAGED
                   : ING_RECOMPUTE;
    }
    const size_t wb = serial ? 0 : ingest_work_bytes(n, maxf, mode);
    if ((rc = dev_grow(&b->d_ing_work, &b->ing_work_bytes, wb, 1, "scroll_batch_ingest"))) return rc;
    hipStream_t hs = b->own;
    HIPCHK(hipMemcpyAsync(b->d_ing_files, files.data(), files.size() * sizeof(IngestFile),
                          hipMemcpyHostToDevice, hs));
    if (b->timing) {
        for (hipEvent_t &e : b->ing_ev)
            if (!e) HIPCHK(timing_event(&e));
        HIPCHK(hipEventRecord(b->ing_ev[0], hs));
    }
    if (ingest_launch(hs, d_files, b->d_ing_files, n, maxf, b->d_ing_scan, b->d_ing_out,
                      b->d_arena, (uint64_t)b->ld_arena, (uint64_t)b->arena_bytes, b->nstreams,
                      serial ? nullptr : b->d_ing_work, wb, mode)) {
        set_err("ingest launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    if (b->timing) HIPCHK(hipEventRecord(b->ing_ev[1], hs));
    std::vector<IngestOut> outs((size_t)n);
    HIPCHK(hipMemcpyAsync(outs.data(), b->d_ing_out, outs.size() * sizeof(IngestOut),
                          hipMemcpyDeviceToHost, hs));
    HIPCHK(hipStreamSynchronize(hs));
    if (b->timing) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, b->ing_ev[0], b->ing_ev[1]) == hipSuccess) {
            b->ing_ms += ms;
            b->ing_n++;
        }
    }
    for (int k = 0; k < n; ++k) {
        if (outs[k].err != ING_OK) {
            set_err("scroll_batch_ingest: new stream %d: %s", k, ing_msg(outs[k].err));
            /* a segment's bounded look-back wait is a device hand-off failure,
             * not a bad file (as k_dyn_row's DF_HANDOFF) */
            return outs[k].err == ING_ERR_OVERFLOW ? SCROLL_ERR_OVERFLOW
                   : outs[k].err == ING_ERR_WAIT   ? SCROLL_ERR_DEVICE
                                                   : SCROLL_ERR_CONFIG;
        }
        if ((b->dyn_on && (outs[k].w != b->dyn_pw || outs[k].h != b->dyn_ph)) ||
            (b->hint_on && ((outs[k].w / 16) * (outs[k].h / 16) > b->hint_max_mb ||
                            outs[k].w / 16 > HINT_MAX_MBW))) {
            set_err("scroll_batch_ingest: new stream %d (%dx%d) does not fit the batch's "
                    "dynamic rect / hint slots", k, outs[k].w, outs[k].h);
            return SCROLL_ERR_CONFIG;
        }
    }
    /* the config composer_init derives (src/composer.c:193-203), frame_num 2
     * after composer_write_header */
    const int s0 = b->nstreams;
    for (int k = 0; k < n; ++k) {
        /* the rule add_stream enforces: the loop filter on (no
         * deblocking_filter_control_present_flag) keeps the rect at QP 26 */
        if (b->dyn_qp != 26 && !outs[k].deblock) {
            set_err("scroll_batch_ingest: new stream %d has the deblocking filter on (no "
                    "deblocking_filter_control_present_flag); the batch's rect QP is %d, not 26", k, b->dyn_qp);
            return SCROLL_ERR_CONFIG;
        }
    }
    for (int k = 0; k < n; ++k) {
        ComposerConfig cfg;
        composer_config_init(&cfg, outs[k].w, outs[k].h);
        composer_config_set_sps_params(&cfg, 4, 2, 4);
        composer_config_set_pps_params(&cfg, 1, outs[k].deblock);
        cfg.frame_num = 2;
        if ((rc = check_cfg(&cfg))) return rc;
        DevStream *d = &b->h_st[s0 + k];
        memset(d, 0, sizeof(*d));
        cfg_to_dev(&cfg, d);
        d->dyn_qp = b->dyn_qp;              /* the batch's rect QP, as add_stream sets it */
        d->out_pos = outs[k].bytes;
        d->undelivered = outs[k].bytes;     /* SPS + PPS + A + B go out with the first delivery */
        d->out_cap = b->arena_bytes;
    }
    HIPCHK(hipMemcpy(b->d_st + s0, b->h_st + s0, (size_t)n * sizeof(DevStream),
                     hipMemcpyHostToDevice));
    b->nstreams += n;
    return SCROLL_OK;
}

int scroll_batch_ingest_stats(ScrollBatch *b, double *ms, int *count)
{
    if (!b) return SCROLL_ERR_ARG;
    if (ms) *ms = b->ing_ms;
    if (count) *count = b->ing_n;
    b->ing_ms = 0.0;
    b->ing_n = 0;
    return SCROLL_OK;
}

/* ------------------- reference files from pictures (I_PCM) ------------------ */
/* the I_PCM files of n pictures; sizes: host (synchronous call) or device
 * (d_sizes, asynchronous: the overflow check waits for the next sync) */
static int ipcm_files(ScrollBatch *b, int n, int w, int h, const uint8_t *d_pics, size_t pic_stride, uint8_t *d_out,
                      size_t out_stride, uint64_t *sizes, uint64_t *d_sizes_out)
{
    const bool async = d_sizes_out != nullptr;
    if (!b || n < 0 || (n > 0 && (!d_pics || !d_out || !(sizes || d_sizes_out)))) return SCROLL_ERR_ARG;
    if (n == 0) return SCROLL_OK;
    const size_t nmb = (size_t)(w / 16) * (size_t)(h / 16);
    if (w <= 0 || h <= 0 || (w & 15) || (h & 15) || nmb >= 65536 ||
        pic_stride < (size_t)w * h * 3 / 2) {
        set_err("scroll_batch_ipcm_files: %dx%d pictures (stride %zu) not supported", w, h, pic_stride);
        return SCROLL_ERR_ARG;
    }
    if (!async) {
        int rc = batch_host_sync(b);
        if (rc) return rc;
    }
    HIPCHK(hipSetDevice(b->device));
    if (async && !b->ipcm_over) {                   /* the sticky overflow flag (read at the next sync) */
        if (!b->d_ipcm_sticky) HIPCHK(hipMalloc(&b->d_ipcm_sticky, sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(b->d_ipcm_sticky, 0, sizeof(uint32_t), b->own));
    }
    IpcmGeom g{};
    g.w = w;
    g.h = h;
    g.mbw = (uint32_t)(w / 16);
    g.nmb = (uint32_t)nmb;
    g.m_mbw = g.mbw <= 1 ? 0u : 0xffffffffu / g.mbw + 1u;
    g.m_386 = 0;
    g.pic_stride = pic_stride;
    g.out_stride = out_stride;
    /* prefix: SPS, PPS (h264_generate_sps / _pps, identical in the composer
     * and the experiment) as NAL units, then the IDR's start code + header */
    {
        uint8_t rbsp[64];
        NALWriter nw;
        uint8_t tmp[64];
        nal_writer_init(&nw, g.pre, IPCM_PRE_MAX, tmp, sizeof(tmp));
        size_t k = h264_generate_sps(rbsp, sizeof(rbsp), w, h);
        nal_write_unit(&nw, 3, 7, rbsp, k, 1);
        k = h264_generate_pps(rbsp, sizeof(rbsp));
        nal_write_unit(&nw, 3, 8, rbsp, k, 1);
        size_t o = nal_writer_get_size(&nw);
        const uint8_t idr[5] = {0, 0, 0, 1, (uint8_t)(3 << 5 | 5)};
        memcpy(g.pre + o, idr, 5);
        g.npre = (uint32_t)(o + 5);
    }
    /* IDR slice header with the experiment's defaults (h264_encoder.c:12-29,
     * :622-662) + MB 0's mb_type ue(25) and alignment (:730-736) */
    {
        BitWriter bw;
        bitwriter_init(&bw, g.hdr, sizeof(g.hdr));
        bitwriter_write_ue(&bw, 0);          /* first_mb_in_slice */
        bitwriter_write_ue(&bw, 7);          /* slice_type I (all) */
        bitwriter_write_ue(&bw, 0);          /* pic_parameter_set_id */
        bitwriter_write_bits(&bw, 0, 4);     /* frame_num, log2_max_frame_num 4 */
        bitwriter_write_ue(&bw, 0);          /* idr_pic_id */
        bitwriter_write_bit(&bw, 0);         /* no_output_of_prior_pics_flag */
        bitwriter_write_bit(&bw, 1);         /* long_term_reference_flag */
        bitwriter_write_se(&bw, 0);          /* slice_qp_delta */
        bitwriter_write_ue(&bw, 1);          /* disable_deblocking_filter_idc */
        bitwriter_write_ue(&bw, 25);         /* mb_type I_PCM */
        while (!bitwriter_is_byte_aligned(&bw)) bitwriter_write_bit(&bw, 0);
        g.nh = (uint32_t)bitwriter_get_size(&bw);
    }
    g.rbsp_len = (uint32_t)(g.nh - 2 + 386 * nmb + 1);
    g.nchunk = (g.rbsp_len + IPCM_CHUNK - 1) / IPCM_CHUNK;
    /* counts [n][nchunk] u32, then sizes [n] u64, then the over flag */
    const size_t cnt_bytes = ((size_t)n * g.nchunk * sizeof(uint32_t) + 7) & ~(size_t)7;
    const size_t need = cnt_bytes + (size_t)n * sizeof(uint64_t) + sizeof(uint64_t);
    if (need > b->ipcm_cap && async && b->ipcm_over) {
        /* an earlier asynchronous call may still use the scratch */
        HIPCHK(hipStreamSynchronize(b->own));
    }
    int rc = dev_grow((void **)&b->d_ipcm_cnt, &b->ipcm_cap, need, 1, "scroll_batch_ipcm_files");
    if (rc) return rc;
    /* SCROLL_IPCM_ONEPASS=1: the one pass when no file can overflow
     * out_stride -- 1.54x the algorithmic bytes instead of 2.50x, but 0.67
     * against 0.57 ms per ipcm720 call (its look-back holds each workgroup
     * for a round trip; profiles/r06o_ipcm_onepass.txt), so not the default */
    const bool one = getenv("SCROLL_IPCM_ONEPASS") != nullptr && out_stride >= ipcm_worst(&g);
    if (one && (size_t)n * g.nchunk > b->ipcm_hw_cap) {
        if (async && b->ipcm_over) HIPCHK(hipStreamSynchronize(b->own));
        (void)hipFree(b->d_ipcm_hw);
        b->d_ipcm_hw = nullptr;
        b->ipcm_hw_cap = 0;
        const size_t words = (size_t)n * g.nchunk;
        hipError_t e = hipMalloc(&b->d_ipcm_hw, words * sizeof(unsigned long long));
        if (e != hipSuccess) return hip_fail("scroll_batch_ipcm_files", e);
        HIPCHK(hipMemsetAsync(b->d_ipcm_hw, 0, words * sizeof(unsigned long long), b->own));
        b->ipcm_hw_cap = words;
    }
    /* the write pass reads the count pass's RBSP while that scratch stays
     * under 4 GB, else it generates the bytes again */
    const uint64_t stg_stride = (uint64_t)g.nchunk * IPCM_CHUNK;
    const size_t stg_need = (size_t)n * stg_stride;
    uint8_t *stg = nullptr;
    if (!one && getenv("SCROLL_IPCM_RECOMPUTE") == nullptr && stg_need <= ((size_t)4 << 30)) {
        if (stg_need > b->ipcm_stg_cap) {
            (void)hipFree(b->d_ipcm_stg);
            b->d_ipcm_stg = nullptr;
            b->ipcm_stg_cap = 0;
            if (hipMalloc(&b->d_ipcm_stg, stg_need) == hipSuccess) b->ipcm_stg_cap = stg_need;
            else (void)hipGetLastError();               /* no scratch: the generating write pass */
        }
        if (b->d_ipcm_stg) stg = b->d_ipcm_stg;
    }
    hipStream_t hs = b->own;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (b->timing && !async) {
        for (hipEvent_t &e : b->ing_ev)                  /* created lazily, shared with ingest */
            if (!e) HIPCHK(timing_event(&e));
        e0 = b->ing_ev[0];
        e1 = b->ing_ev[1];
    } else if (b->timing) {                             /* a pair per call, read at the stats */
        if (b->ipcm_ev.size() < b->ipcm_ev_used + 2) {
            for (int k = 0; k < 2; ++k) {
                hipEvent_t e;
                HIPCHK(timing_event(&e));
                b->ipcm_ev.push_back(e);
            }
        }
        e0 = b->ipcm_ev[b->ipcm_ev_used];
        e1 = b->ipcm_ev[b->ipcm_ev_used + 1];
        b->ipcm_ev_used += 2;
    }
    if (async && b->last && b->last != hs) {
        /* a compose queued on a caller's stream: own waits for it, so that
         * b->last = own below still covers it (the next sync must not copy
         * d_st back while that compose runs) */
        if (!b->out_ev) HIPCHK(hipEventCreateWithFlags(&b->out_ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(b->out_ev, b->last));
        HIPCHK(hipStreamWaitEvent(hs, b->out_ev, 0));
    }
    if (e0) HIPCHK(hipEventRecord(e0, hs));
    uint64_t *d_sizes = async ? d_sizes_out
                              : reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(b->d_ipcm_cnt) + cnt_bytes);
    uint32_t *d_over = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(b->d_ipcm_cnt) + cnt_bytes +
                                                    (size_t)n * sizeof(uint64_t));
    /* count pass, sizes and the overflow check, write pass: no host step in
     * between (the write pass writes nothing when a file is over) */
    uint32_t *sticky = async ? b->d_ipcm_sticky : nullptr;
    if (one) {
        b->ipcm_epoch = b->ipcm_epoch % 0xffffffu + 1u;          /* 24 bits, never 0 */
        const IpcmOnePass op{b->d_ipcm_hw, b->ipcm_epoch, d_sizes, sticky};
        if (ipcm_launch_onepass(hs, n, &g, d_pics, d_out, d_over, &op)) {
            set_err("ipcm launch: %s", hipGetErrorString(hipGetLastError()));
            return SCROLL_ERR_HIP;
        }
    } else if (ipcm_launch(hs, 0, n, &g, d_pics, b->d_ipcm_cnt, d_out, stg, stg_stride, d_sizes, d_over, sticky) ||
               ipcm_launch(hs, 1, n, &g, d_pics, b->d_ipcm_cnt, d_out, stg, stg_stride, d_sizes, d_over, sticky)) {
        set_err("ipcm launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    if (e1) HIPCHK(hipEventRecord(e1, hs));
    if (async) {
        /* nothing comes back now: the overflow flag is read at the next sync */
        b->ipcm_over = b->d_ipcm_sticky;
        b->ipcm_over_stride = out_stride;
        b->last = hs;
        b->host_valid = 0;
        return SCROLL_OK;
    }
    uint32_t over_flag = 0;
    HIPCHK(hipMemcpyAsync(sizes, d_sizes, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, hs));
    HIPCHK(hipMemcpyAsync(&over_flag, d_over, sizeof(uint32_t), hipMemcpyDeviceToHost, hs));
    HIPCHK(hipStreamSynchronize(hs));
    if (e0) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        b->ipcm_ms += ms;
        b->ipcm_n++;
    }
    if (over_flag) {
        int over = 0;
        while (over < n && sizes[over] <= out_stride) ++over;
        set_err("scroll_batch_ipcm_files: file %d needs %llu bytes, out_stride is %zu", over,
                (unsigned long long)sizes[over < n ? over : 0], out_stride);
        return SCROLL_ERR_OVERFLOW;
    }
    return SCROLL_OK;
}

int scroll_batch_ipcm_files_device(ScrollBatch *b, int n, int w, int h, const uint8_t *d_pics,
                                   size_t pic_stride, uint8_t *d_out, size_t out_stride,
                                   uint64_t *sizes)
{
    return ipcm_files(b, n, w, h, d_pics, pic_stride, d_out, out_stride, sizes, nullptr);
}

int scroll_batch_ipcm_files_device_async(ScrollBatch *b, int n, int w, int h, const uint8_t *d_pics,
                                         size_t pic_stride, uint8_t *d_out, size_t out_stride,
                                         uint64_t *d_sizes)
{
    if (!b || (n > 0 && !d_sizes)) return SCROLL_ERR_ARG;
    return ipcm_files(b, n, w, h, d_pics, pic_stride, d_out, out_stride, nullptr, d_sizes);
}

int scroll_batch_ipcm_stats(ScrollBatch *b, double *ms, int *count)
{
    if (!b) return SCROLL_ERR_ARG;
    if (b->ipcm_ev_used) {                              /* the asynchronous calls' pairs */
        HIPCHK(hipStreamSynchronize(b->own));
        for (size_t k = 0; k + 1 < b->ipcm_ev_used; k += 2) {
            float v = 0.0f;
            HIPCHK(hipEventElapsedTime(&v, b->ipcm_ev[k], b->ipcm_ev[k + 1]));
            b->ipcm_ms += v;
            b->ipcm_n++;
        }
        b->ipcm_ev_used = 0;
    }
    if (ms) *ms = b->ipcm_ms;
    if (count) *count = b->ipcm_n;
    b->ipcm_ms = 0.0;
    b->ipcm_n = 0;
    return SCROLL_OK;
}

int scroll_batch_ingest(ScrollBatch *b, int n, const uint8_t *const *ref_a, const size_t *na,
                        const uint8_t *const *ref_b, const size_t *nb, int *first)
{
    if (!b || n < 0 || (n > 0 && (!ref_a || !na || !ref_b || !nb))) return SCROLL_ERR_ARG;
    if (n == 0) return scroll_batch_ingest_device(b, 0, nullptr, nullptr, first);
    std::vector<uint64_t> desc(4 * (size_t)n);
    size_t tot = 0;
    for (int k = 0; k < n; ++k) {
        if ((na[k] && !ref_a[k]) || (nb[k] && !ref_b[k])) return SCROLL_ERR_ARG;
        desc[4 * k] = tot;
        desc[4 * k + 1] = na[k];
        tot += (na[k] + 255) & ~(size_t)255;
        desc[4 * k + 2] = tot;
        desc[4 * k + 3] = nb[k];
        tot += (nb[k] + 255) & ~(size_t)255;
    }
    HIPCHK(hipSetDevice(b->device));
    int rc = ing_in_reserve(b, tot, "scroll_batch_ingest");
    if (rc) return rc;
    for (int k = 0; k < n; ++k) {
        if (na[k]) HIPCHK(hipMemcpy(b->d_ing_in + desc[4 * k], ref_a[k], na[k], hipMemcpyHostToDevice));
        if (nb[k]) HIPCHK(hipMemcpy(b->d_ing_in + desc[4 * k + 2], ref_b[k], nb[k], hipMemcpyHostToDevice));
    }
    return scroll_batch_ingest_device(b, n, b->d_ing_in, desc.data(), first);
}

/* mid-stream long-term reference updates (k_ing_update, ingest_kernels.hip) */
int scroll_batch_update_refs_device(ScrollBatch *b, int n, const int *streams, const int *which,
                                    const uint8_t *d_files, const uint64_t *desc, int *status)
{
    if (!b || n < 0 || (n > 0 && (!streams || !which || !d_files || !desc))) return SCROLL_ERR_ARG;
    std::vector<uint8_t> seen((size_t)b->nstreams, 0);
    for (int k = 0; k < n; ++k) {
        if (streams[k] < 0 || streams[k] >= b->nstreams || which[k] < 0 || which[k] > 1 || seen[streams[k]]) {
            set_err("scroll_batch_update_refs: entry %d: bad or repeated stream / which", k);
            return SCROLL_ERR_ARG;
        }
        seen[streams[k]] = 1;
    }
    if (n == 0) return SCROLL_OK;
    HIPCHK(hipSetDevice(b->device));
    if (int rc = ing_reserve(b, n, "scroll_batch_update_refs")) return rc;
    if ((size_t)n > b->upd_cap) {
        (void)hipFree(b->d_upd);
        b->d_upd = nullptr;
        b->upd_cap = 0;
        HIPCHK(hipMalloc(&b->d_upd, 2 * (size_t)n * sizeof(int32_t)));
        b->upd_cap = (size_t)n;
    }
    std::vector<IngestFile> files((size_t)n);
    std::vector<int32_t> ups(2 * (size_t)n);
    uint64_t maxf = 0;
    for (int k = 0; k < n; ++k) {
        files[k].off = desc[2 * k];
        files[k].size = desc[2 * k + 1];
        maxf = std::max(maxf, files[k].size);
        ups[2 * k] = streams[k];
        ups[2 * k + 1] = which[k];
    }
    hipStream_t hs = b->last ? b->last : b->own;   /* after the pending composes */
    HIPCHK(hipMemcpyAsync(b->d_ing_files, files.data(), files.size() * sizeof(IngestFile),
                          hipMemcpyHostToDevice, hs));
    HIPCHK(hipMemcpyAsync(b->d_upd, ups.data(), ups.size() * sizeof(int32_t), hipMemcpyHostToDevice, hs));
    if (update_launch(hs, d_files, b->d_ing_files, n, maxf, b->d_ing_scan, b->d_upd, b->d_ing_out, b->d_st,
                      b->d_arena, (uint64_t)b->ld_arena)) {
        set_err("reference update launch: %s", hipGetErrorString(hipGetLastError()));
        return SCROLL_ERR_HIP;
    }
    std::vector<IngestOut> outs((size_t)n);
    HIPCHK(hipMemcpyAsync(outs.data(), b->d_ing_out, outs.size() * sizeof(IngestOut), hipMemcpyDeviceToHost, hs));
    HIPCHK(hipStreamSynchronize(hs));
    b->host_valid = 0;
    b->nal_cache_valid = 0;
    int rc = SCROLL_OK;
    for (int k = 0; k < n; ++k) {
        if (status) status[k] = outs[k].err;
        if (outs[k].err != ING_OK && rc == SCROLL_OK) {
            set_err("scroll_batch_update_refs: stream %d: %s", streams[k],
                    outs[k].err == ING_ERR_DIMS ? "picture size differs from the stream's" : ing_msg(outs[k].err));
            rc = outs[k].err == ING_ERR_OVERFLOW ? SCROLL_ERR_OVERFLOW : SCROLL_ERR_CONFIG;
        }
    }
    return rc;
}

int scroll_batch_update_refs(ScrollBatch *b, int n, const int *streams, const int *which,
                             const uint8_t *const *files, const size_t *sizes, int *status)
{
    if (!b || n < 0 || (n > 0 && (!files || !sizes))) return SCROLL_ERR_ARG;
    std::vector<uint64_t> desc(2 * (size_t)n);
    size_t tot = 0;
    for (int k = 0; k < n; ++k) {
        if (sizes[k] && !files[k]) return SCROLL_ERR_ARG;
        desc[2 * k] = tot;
        desc[2 * k + 1] = sizes[k];
        tot += (sizes[k] + 255) & ~(size_t)255;
    }
    if (n == 0) return SCROLL_OK;
    int rc = batch_host_sync(b);                  /* the input buffer may be in use */
    if (rc) return rc;
    HIPCHK(hipSetDevice(b->device));
    if ((rc = ing_in_reserve(b, tot, "scroll_batch_update_refs"))) return rc;
    for (int k = 0; k < n; ++k)
        if (sizes[k]) HIPCHK(hipMemcpy(b->d_ing_in + desc[2 * k], files[k], sizes[k], hipMemcpyHostToDevice));
    return scroll_batch_update_refs_device(b, n, streams, which, b->d_ing_in, desc.data(), status);
}

}  // extern "C"
