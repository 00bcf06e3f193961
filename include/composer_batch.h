/*
 * composer_batch.h -- ADDITIVE many-stream API (no reference counterpart).
 *
 * The reference API is synchronous, single-stream and single-frame
 * (include/composer.h:79, include/h264_writer.h:124).  Throughput on an
 * MI355X needs many (stream, frame) items per launch, so this header adds a
 * batch object that keeps every stream's ComposerConfig state, its scroll
 * offsets ("UI hints") and its Annex-B output arena resident in HBM:
 *
 *   scroll_batch_create()            one batch per GPU (device ordinal)
 *   scroll_batch_add_stream(cfg)     a stream = one ComposerConfig
 *   scroll_batch_set_offsets()       [streams][frames] offsets -> HBM
 *   scroll_batch_compose(n, stream)  async: GPU state machine (waypoints,
 *                                    frame_num) + P-slice kernels; appends
 *                                    n composed frames to every stream arena
 *   scroll_batch_sync()              wait + surface device error words
 *   scroll_batch_copy_output()       arena -> host
 *
 * Semantics per stream are exactly n calls of composer_write_scroll_frame
 * (src/composer.c:255-264), or of the experiment's loop body
 * (experiments/scroll-encoder/src/main.c:418-424) in SCROLL_MODE_EXPERIMENT.
 * Streams are independent; multi-GPU = one batch per device with a static
 * contiguous shard of the streams (no collective).
 *
 * All functions return SCROLL_OK (0) or a negative SCROLL_ERR_* code;
 * scroll_last_error() has the message.  No CPU fallback exists: without a
 * usable gfx950 device every compose call fails with SCROLL_ERR_NO_DEVICE.
 */
#ifndef COMPOSER_BATCH_H
#define COMPOSER_BATCH_H

#include <stddef.h>
#include <stdint.h>
#include "composer.h"
#include "h264_writer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCROLL_OK             0
#define SCROLL_ERR_NO_DEVICE (-1)
#define SCROLL_ERR_ARG       (-2)
#define SCROLL_ERR_OOM       (-3)
#define SCROLL_ERR_OVERFLOW  (-4)   /* output arena full (reference: assert abort) */
#define SCROLL_ERR_HIP       (-5)
#define SCROLL_ERR_CONFIG    (-6)   /* config outside the supported syntax range  */
#define SCROLL_ERR_DEVICE    (-7)   /* a device-side wait timed out (the dynamic rect's
                                       row hand-off): that stream committed nothing */

#define SCROLL_MODE_COMPOSER   0    /* waypoint NAL in addition to the scroll NAL */
#define SCROLL_MODE_EXPERIMENT 1    /* waypoint NAL instead of the scroll NAL     */

/* debug flags (tests / profiling ablations; outputs are wrong for 2, 4, 8) */
#define SCROLL_DEBUG_FORCE_SERIAL 1 /* every NAL through the serial device path   */
#define SCROLL_DEBUG_EMIT_NOSTORE 2 /* k_emit computes every chunk, stores none   */
#define SCROLL_DEBUG_EMIT_ZEROS   4 /* k_emit stores zero chunks, computes none   */
#define SCROLL_DEBUG_EMIT_BUILD   8 /* k_emit builds the layouts and stops        */
#define SCROLL_DEBUG_EMIT_NOPURE 16 /* k_emit skips the pure-chunk phase          */
#define SCROLL_DEBUG_EMIT_NOMIXED 32 /* k_emit skips the mixed-chunk phase        */
#define SCROLL_DEBUG_EMIT_STAMPS 64 /* k_emit records s_memtime per phase per wave */
#define SCROLL_DEBUG_EMIT_NOBYTES 128 /* k_emit skips the tile-end partial chunks  */
#define SCROLL_DEBUG_DYN_STAMPS 256 /* k_dyn_row / gather: realtime per phase    */
/* retired: runtime ablations of the earlier one-kernel dynamic coder (no
 * kernel reads them now; k_dyn_row's per-phase times come from
 * SCROLL_DEBUG_DYN_STAMPS).  Values kept so the flag numbering stays
 * stable. */
#define SCROLL_DEBUG_DYN_NOLOAD  512
#define SCROLL_DEBUG_DYN_NOCAVLC 1024
#define SCROLL_DEBUG_DYN_NOHEAD  2048
#define SCROLL_DEBUG_DYN_NOWRITE 4096
/* tests: the dynamic emit keeps at most 4 EP positions per NAL, so every NAL
 * with more emulation-prevention bytes takes the large-NAL path (k_dyn_emit,
 * otherwise only reached past 2,048 EP bytes); output unchanged */
#define SCROLL_DEBUG_DYN_EPCAP4 8192
/* tests: k_dyn_row of stream 0, frame 0, rect row 0 does not publish its
 * bottom TotalCoeffs, so row 1's bounded wait expires: stream 0 fails with
 * SCROLL_ERR_DEVICE, every other stream composes normally */
#define SCROLL_DEBUG_DYN_NOPUBLISH 16384
/* tests: the dynamic rect's NALs go to the arena through the round-3 gather
 * (k_dyn_emit_gather) instead of k_dyn_gather; output unchanged */
#define SCROLL_DEBUG_DYN_GATHER1 32768
/* tests: the dynamic rect's EP-position machinery of the whole-picture rects
 * on any rect -- the 8,192-entry epfix set and list, and k_dyn_gather's LDS
 * windows at 7 positions each (every NAL with more EP bytes is gathered
 * window by window); output unchanged.  Set before scroll_batch_set_dyn_rect */
#define SCROLL_DEBUG_DYN_EPWIN 65536

typedef struct ScrollBatch ScrollBatch;

typedef struct {
    int device;            /* HIP device ordinal                               */
    int max_streams;
    int max_frames;        /* max composed frames per scroll_batch_compose    */
    size_t arena_bytes;    /* device output arena per stream                   */
    int mode;              /* SCROLL_MODE_*                                    */
} ScrollBatchDesc;

const char *scroll_last_error(void);
int scroll_device_count(void);                 /* usable gfx950 devices (0 if none) */
const char *scroll_version(void);

int scroll_batch_create(ScrollBatch **out, const ScrollBatchDesc *desc);
void scroll_batch_destroy(ScrollBatch *b);
int scroll_batch_add_stream(ScrollBatch *b, const ComposerConfig *cfg); /* -> stream id */
int scroll_batch_num_streams(const ScrollBatch *b);
int scroll_batch_set_debug(ScrollBatch *b, int flags);

/* offsets: host array [num_streams][nframes] (row stride nframes) */
int scroll_batch_set_offsets(ScrollBatch *b, const int32_t *offsets, int nframes);
/* device array [num_streams][max_frames]; fill it from device code to skip H2D */
int32_t *scroll_batch_offsets_device(ScrollBatch *b);

/* async on hip_stream (hipStream_t; NULL = the batch's own stream) */
int scroll_batch_compose(ScrollBatch *b, int nframes, void *hip_stream);
/* flags: SCROLL_COMPOSE_REWIND = start every arena at 0 (the caller has
 * consumed the previous batch's bytes) -- device-side, no host sync. */
#define SCROLL_COMPOSE_REWIND 1
int scroll_batch_compose_ex(ScrollBatch *b, int nframes, void *hip_stream, int flags);
int scroll_batch_sync(ScrollBatch *b);

/* state after sync: ComposerConfig as the reference would hold it */
int scroll_batch_get_config(ScrollBatch *b, int s, ComposerConfig *cfg);
int scroll_batch_set_config(ScrollBatch *b, int s, const ComposerConfig *cfg);
size_t scroll_batch_output_size(ScrollBatch *b, int s);
int scroll_batch_copy_output(ScrollBatch *b, int s, size_t from, uint8_t *dst, size_t n);
const uint8_t *scroll_batch_output_device(ScrollBatch *b, int s);
/* Host delivery (the reference returns its bytes in host memory,
 * composer.c:255-291): pinned host buffers the device writes into, and the
 * bytes appended to every stream since its previous delivery (composes,
 * reference updates; a rewound arena starts over) packed into dst back to
 * back in stream order, asynchronously on hip_stream (NULL = the stream of
 * the last compose; another stream waits for it).  table (pinned, 1 + 2 S
 * u64) gets [0] = the packed size (~0: larger than cap, nothing written),
 * then per stream its offset in dst (16-byte aligned) and its byte count.
 * dst and cap 16-byte aligned.  Valid after scroll_batch_sync / a stream
 * sync; the arenas must not be rewritten before the copy has run. */
int scroll_host_alloc(void **p, size_t n);
void scroll_host_free(void *p);
int scroll_batch_output_to_host_async(ScrollBatch *b, uint8_t *dst, size_t cap, uint64_t *table,
                                      void *hip_stream);
int scroll_batch_reset_output(ScrollBatch *b);   /* rewind all arenas, keep state */

/* last compose: planned NAL units of stream s (kind/size/offset per NAL) */
int scroll_batch_nal_count(ScrollBatch *b, int s);
int scroll_batch_nal_info(ScrollBatch *b, int s, int i, int *kind, int *offset_px,
                          uint32_t *size, int *slow);

/* HIP-event timing of the last compose's kernels, on the launch stream:
 * which 0 = plan kernel(s), 1 = emit kernel, 2 = dyn stage, 3 = dyn emit,
 * 4 = dyn code (k_dyn_rows + k_dyn_code), 5 = dyn pack (k_dyn_group + k_dyn_ep).
 * Enable before compose: on = 1 every pair (kernel_ms and kernel_stats_ex
 * complete); on = 2 ("lite") only the dominant kernel's pair -- dyn code
 * (also reported as dyn stage) or emit -- into kernel_stats_ex, the others
 * 0: each event record is a marker packet that holds the queue between the
 * kernels, so a timed step with every pair runs ~ 40 us longer; 0 off.
 * kernel_ms returns -1 while lite timing is on (no per-kernel pairs exist). */
int scroll_batch_enable_timing(ScrollBatch *b, int on);
float scroll_batch_kernel_ms(ScrollBatch *b, int which);
/* all timed composes since the last call: summed plan / emit kernel ms and
 * the number of composes; the accumulators are reset afterwards */
int scroll_batch_kernel_stats(ScrollBatch *b, double *plan_ms, double *emit_ms, int *count);
/* SCROLL_DEBUG_EMIT_STAMPS: copy the per-wave phase stamps of the last
 * compose (8 x u64 per wave slot); returns the number of wave slots */
long long scroll_batch_debug_stamps(ScrollBatch *b, uint64_t *dst, long long max_slots);
/* bytes appended to every arena by the last compose (sum over streams) */
unsigned long long scroll_batch_last_bytes(ScrollBatch *b);
/* NAL units planned by the last compose (sum over streams) */
long long scroll_batch_last_nals(ScrollBatch *b);

/* ---- dynamic rect (BASELINE configs 3-5; no reference counterpart) ----
 * Every scroll NAL of the batch carries a rectangle of dynamic MBs: they keep
 * their row's (ref_idx, mv) and add coded_block_pattern, mb_qp_delta and a
 * CAVLC residual of (source - prediction) at QP 26 or the rect's QP
 * (scroll_batch_set_dyn_qp; bit-exact definition:
 * oracle/dyn_oracle.h).  Waypoint NALs stay residual-free.  All streams of
 * the batch must share one picture size; call after adding the streams.
 *
 *   scroll_batch_set_dyn_rect(b, x0, y0, w, h, slot)   MB units; w or h = 0
 *       turns the rect off.  slot = staging bytes per frame, 0 = a bound no
 *       NAL can exceed (larger ones fail with SCROLL_ERR_OVERFLOW).
 *   scroll_batch_set_dyn_refs(b, s, a, b)   decoded reference pictures A and
 *       B (I420, w*h*3/2 bytes each) of stream s, or of every stream (s = -1)
 *   source pixels: [stream][frame] blocks of 384*w*h bytes (the rect's luma
 *       16w x 16h, then Cb, Cr 8w x 8h), frame f = the f-th composed frame of
 *       the next compose: scroll_batch_set_dyn_source (host copy),
 *       scroll_batch_dyn_source_device (fill in place), or
 *       scroll_batch_dyn_source_synth (the synthetic source of SURVEY §8d for
 *       global stream ids stream_base + s and frame numbers t0 + f). */
int scroll_batch_set_dyn_rect(ScrollBatch *b, int x0, int y0, int w, int h, size_t slot_bytes);
int scroll_batch_set_dyn_refs(ScrollBatch *b, int s, const uint8_t *ref_a, const uint8_t *ref_b);
/*   scroll_batch_set_dyn_qp(b, qp)   the rect's QP, 0..51 (default 26), of
 *       every stream (and of streams added later), for the following
 *       composes: a stream's dynamic scroll NALs then carry slice_qp_delta =
 *       qp - 26 (chroma at QPc, Table 8-15) and their MBs mb_qp_delta 0;
 *       waypoint NALs and the P-only path are unchanged.  Below 22 a NAL's
 *       levels need 16 bits and it is coded on the general path (records in
 *       HBM); levels are clamped to +-2063, the largest every CAVLC context
 *       codes with level_prefix <= 15 (reached only by chroma DC below QPc 6).
 *   scroll_batch_set_dyn_qp_stream(b, s, qp)   the same for stream s.
 *   scroll_batch_set_dyn_qp_at(b, s, f, qp)    under UI hints (the rect in the
 *       frame's hint record): frame f of stream s at QP qp, -1 = the
 *       stream's.  There the slice QP stays 26 and the rect's first MB with a
 *       residual carries mb_qp_delta qp - 26, the others 0.  (Without hints a
 *       frame's own QP is scroll_batch_set_dyn_qp_frames', further down.)
 *   A stream with the deblocking filter on (no
 *   deblocking_filter_control_present_flag, e.g. an ingested one) keeps QP 26:
 *   another QP would change the filtering of its scroll MBs (SCROLL_ERR_CONFIG). */
#define SCROLL_DYN_QP_MIN 0
#define SCROLL_DYN_QP_MAX 51
int scroll_batch_set_dyn_qp(ScrollBatch *b, int qp);
int scroll_batch_set_dyn_qp_stream(ScrollBatch *b, int s, int qp);
int scroll_batch_set_dyn_qp_at(ScrollBatch *b, int s, int f, int qp);
int scroll_batch_set_dyn_source(ScrollBatch *b, const uint8_t *src, int nframes);
/* Under UI hints (scroll_batch_set_hints) the rect's MBs keep the hint
 * field's (ref, mv) -- full-pel luma, 2-D 1/8-pel chroma prediction at that
 * motion -- and the rect may sit anywhere in each frame:
 *   scroll_batch_set_dyn_rect_at(b, s, f, x0, y0)   frame f of stream s puts
 *       the rect's w x h MBs at (x0, y0); x0 = -1: no rect in that frame.
 *       Positions other than set_dyn_rect's need hints at compose time, or
 *       scroll_batch_set_dyn_rect_moving below (SCROLL_ERR_CONFIG otherwise);
 *       set_dyn_rect and clear_hints reset them.
 * Each rect MB's residual bits get a region of slot_bytes / (w h) bytes
 * (64 to 2048; slot_bytes 0: 512, which saturated +-255 residuals stay well
 * inside); an MB that outgrows it fails the compose with SCROLL_ERR_OVERFLOW.
 * Bit-exact definition: oracle/splice_oracle.h or_hint_dyn_scroll_nal.
 * Not combinable with spliced slices (one rect per frame). */
int scroll_batch_set_dyn_rect_at(ScrollBatch *b, int s, int f, int x0, int y0);
/* The plain rect (no hints) placed per stream and per frame, on the fast
 * path (k_dyn_rows / k_dyn_row / k_dyn_static / k_dyn_epfix / k_dyn_gather):
 *   scroll_batch_set_dyn_rect_moving(b, 1)   a compose without hints honours
 *       set_dyn_rect_at's positions: entry [s max_frames + f] applies to
 *       frame f of every following compose.  Frame f with its rect at (x, y)
 *       is, byte for byte, NAL f of the same compose with the batch rect at
 *       (x, y) -- prediction is from the static pictures only; a frame
 *       without a rect (x0 = -1) carries the plain scroll NAL the batch
 *       writes with the rect off, has no dynamic NAL (scroll_batch_dyn_frame_info,
 *       _dyn_recon, _dyn_sse, the probe's results and the pick return 1 /
 *       leave it alone, as for a frame the experiment mode replaced) and keeps
 *       its source bytes.  The per-frame QP table, the reconstruction, the
 *       probe, the pick, dyn_source_synth and dyn_source_from_surfaces follow
 *       the positions.  Needs a dynamic rect (SCROLL_ERR_CONFIG without one);
 *       sizes the row stage once for every legal position, so no later
 *       set_dyn_rect_at allocates; scroll_batch_set_dyn_rect drops the flag
 *       with the rect.  With hints set the hinted path runs as it always has
 *       and the flag changes nothing there; scroll_batch_set_fallback stays
 *       hints-only.  Off (the default): nothing changes -- a moved position
 *       without hints is refused at compose time. */
int scroll_batch_set_dyn_rect_moving(ScrollBatch *b, int on);
/* The plain rect sized per stream and per frame, on the same path:
 *   scroll_batch_set_dyn_rect_size_at(b, s, f, w_f, h_f)   frame f of stream s
 *       codes a rect of w_f x h_f MBs at the frame's own origin (the
 *       batch's, set_dyn_rect_at's or a locate's), 1 <= w_f <= w, 1 <= h_f <=
 *       h of set_dyn_rect (SCROLL_ERR_ARG otherwise); (w, h) restores the
 *       batch size.  Frame f is then, byte for byte, the NAL of a batch whose
 *       rect is w_f x h_f at that origin.  Needs set_dyn_rect_moving
 *       (SCROLL_ERR_CONFIG without it) and a picture of at most 256 x 256
 *       MBs (SCROLL_ERR_CONFIG).  Entry f holds for frame f of every
 *       following compose; set_dyn_rect and clear_hints reset sizes together
 *       with positions.  Origins stay legal by the batch size (x0 + w <= mbw,
 *       y0 + h <= mbh), so a sized rect never leaves the picture; a frame
 *       without a rect stays x0 = -1 (there is no size 0).  The first call
 *       sizes the row stage for every (y0, h_f), once; no later one allocates.
 *   Layout: a sized frame is, inside its own slots, a batch whose rect is
 *       w_f x h_f.  Its source block (set_dyn_source, _dyn_source_device,
 *       _from_surfaces, _synth) is luma 16 h_f rows of 16 w_f bytes, then Cb
 *       and Cr at 8 w_f x 8 h_f, at the start of the frame's slot; the same
 *       holds for its scroll_batch_dyn_recon block and its mask-map block
 *       (w_f x h_f pairs).  Slots keep the batch's strides (384 w h bytes a
 *       frame); the rest of a slot is neither read nor written.
 *   The per-frame QP table, the reconstruction and dyn_sse, the probe, the
 *       pick, the mask, dyn_source_synth and dyn_source_from_surfaces follow
 *       the sizes; scroll_batch_dyn_locate places them with size = 1.  With
 *       UI hints set, a compose (its reconstruction included) or a hinted
 *       probe returns SCROLL_ERR_CONFIG while any frame has a size of its
 *       own.  Never called: nothing changes -- no launch, no allocation, no
 *       byte. */
int scroll_batch_set_dyn_rect_size_at(ScrollBatch *b, int s, int f, int w, int h);
/* The conventional-encode fallback (docs/MASTER_DESIGN.md:220: "if hints
 * missing/inconsistent -> full conventional encode"), opt-in:
 *   scroll_batch_set_fallback(b, 1)   with UI hints and a dynamic rect that
 *       is the whole picture (set_dyn_rect(b, 0, 0, width / 16, height / 16,
 *       ...): every frame's source is then a whole picture, as a conventional
 *       encoder's).  A frame whose hints put an MB on a rect naming a
 *       reference the frame lacks -- a frame that fails its stream with
 *       SCROLL_ERR_CONFIG without the flag -- is coded instead as a full
 *       P frame: its hint rects dropped, every MB on the scroll frame's own
 *       motion with the residual of the frame's source (the rect at (0, 0),
 *       whether or not set_dyn_rect_at placed it), in the frame's hint mode
 *       and rect QP.  Other frames are unchanged.  SCROLL_ERR_CONFIG when the
 *       rect is not the whole picture.
 *   scroll_batch_fallback_frame(b, s, f, &on)   after a compose: 1 when
 *       frame f of stream s fell back.
 * Bit-exact definition: oracle/splice_oracle.h or_compose_hint_dyn with no
 * hint rects and the whole-picture rect. */
int scroll_batch_set_fallback(ScrollBatch *b, int on);
int scroll_batch_fallback_frame(ScrollBatch *b, int s, int f, int *fell_back);
uint8_t *scroll_batch_dyn_source_device(ScrollBatch *b, size_t *stream_stride,
                                        size_t *frame_stride);
int scroll_batch_dyn_source_synth(ScrollBatch *b, int nframes, int stream_base, int t0);
/* last compose, frame f of stream s: staged RBSP bytes and EP bytes */
int scroll_batch_dyn_frame_info(ScrollBatch *b, int s, int f, uint32_t *rbsp_bytes,
                                uint32_t *ep_bytes);
/* last compose, all streams: staged RBSP bytes, EP bytes, dynamic NALs */
int scroll_batch_dyn_totals(ScrollBatch *b, unsigned long long *rbsp_bytes,
                            unsigned long long *ep_bytes, long long *dyn_nals);
/* The dynamic rect's reconstruction (opt-in; off: no launch, allocation or
 * output byte of any compose changes).  With it on, every compose also
 * produces, for each frame with a dynamic NAL, the rect a decoder displays
 * -- the coded levels dequantised (H.264 8.5.12.1, chroma DC 8.5.11), inverse
 * transformed (8.5.12.2), added to the prediction and clipped -- and its sum
 * of squared errors against the source, per plane.  The emitted bytes are
 * the same as with it off.
 *
 *   scroll_batch_set_dyn_recon(b, on)   needs a dynamic rect
 *       (SCROLL_ERR_CONFIG without one); allocates the reconstruction
 *       (sized and laid out like the source buffer) and the error sums;
 *       on = 0 frees them.  scroll_batch_set_dyn_rect -- a new rect or none
 *       -- turns it off: call it again for the new rect.
 *   By itself it covers the plain dynamic rect: a compose with the
 *       reconstruction on and UI hints set fails with SCROLL_ERR_CONFIG.
 *   scroll_batch_set_dyn_recon_hinted(b, on)   opt-in on top of it (needs the
 *       reconstruction on, SCROLL_ERR_CONFIG otherwise; off by default;
 *       set_dyn_recon(b, 0) and set_dyn_rect turn it off too): composes with
 *       UI hints -- the rect in the hint record, per-frame positions
 *       (set_dyn_rect_at) and QPs (set_dyn_qp_at), the whole-picture fallback
 *       -- then fill the same two outputs for every frame whose rect was
 *       coded, each MB predicted at its hinted motion (full-pel luma, 2-D
 *       1/8-pel chroma, samples clamped to the picture) and quantised at the
 *       frame's QP.  Composes without hints on such a batch are unchanged.
 *       Spliced slices stay refused (SCROLL_ERR_CONFIG): they carry MB types
 *       the reconstruction does not decode.  Under hints the accessors below
 *       return 1 for a frame without a dynamic NAL, without the rect
 *       (set_dyn_rect_at with x0 = -1) or with a fallback region that did not
 *       fall back, and the stream's negative compose status (what
 *       scroll_batch_sync reports for it: SCROLL_ERR_CONFIG for a hint on a
 *       missing reference, SCROLL_ERR_OVERFLOW for an MB past its region)
 *       for every frame of a stream whose last compose failed.
 *   scroll_batch_dyn_recon_device(b, &ls, &lf)   the device buffer,
 *       [stream][frame] blocks of 384*w*h bytes at the source's strides
 *       (luma 16w x 16h, then Cb, Cr 8w x 8h); NULL while off.  Valid on the
 *       compose's stream after the compose; frames without a dynamic NAL
 *       keep their earlier bytes.
 *   scroll_batch_dyn_recon(b, s, f, dst)   frame f of stream s of the last
 *       compose -> 384*w*h host bytes; scroll_batch_dyn_sse(b, s, f, sse) its
 *       squared error, Y / Cb / Cr.  Both synchronise the compose's stream.
 *       0; 1 when the frame has no dynamic NAL (nothing written), as
 *       scroll_batch_dyn_frame_info; SCROLL_ERR_CONFIG while off,
 *       SCROLL_ERR_ARG outside the last compose's frames,
 *       SCROLL_ERR_OVERFLOW for a frame the coder failed.
 *   scroll_batch_dyn_recon_ms(b)   with scroll_batch_enable_timing: HIP-event
 *       ms of the reconstruction kernels of the last compose; -1 without. */
int scroll_batch_set_dyn_recon(ScrollBatch *b, int on);
int scroll_batch_set_dyn_recon_hinted(ScrollBatch *b, int on);
uint8_t *scroll_batch_dyn_recon_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride);
int scroll_batch_dyn_recon(ScrollBatch *b, int s, int f, uint8_t *dst);      /* 384*w*h host bytes */
int scroll_batch_dyn_sse(ScrollBatch *b, int s, int f, uint64_t sse[3]);     /* Y, Cb, Cr */
float scroll_batch_dyn_recon_ms(ScrollBatch *b);

/* ---- probing the rect at candidate QPs, before the frame is spent ----
 * Everything above answers after the compose, when the stream has moved on
 * (frame_num, the waypoint table).  The probe answers before: for the
 * offsets of scroll_batch_set_offsets and the source of set_dyn_source /
 * _device / _synth, what the next scroll_batch_compose(b, nframes) of the
 * plain dynamic rect would produce per frame at each of nq candidate QPs
 * (every stream gets the same list), whatever QP the streams are set to.
 * It commits nothing: stream state, arenas, NAL lists, dyn_frame_info, the
 * reconstruction and the SSE sums of the last compose stay as they are, and
 * a compose after it emits the bytes it would have emitted without it (the
 * probe plans and resolves its prediction rows in buffers of its own,
 * allocated on the first probe, freed by set_dyn_rect and destroy).
 *
 * Per frame and candidate QP q (ScrollDynProbe, exact integers):
 *   sse[3]    what scroll_batch_dyn_sse reports after a compose at q;
 *   bits      the rect MBs' coded_block_pattern + mb_qp_delta + residual
 *             bits at q (oracle/dyn_oracle.c or_mb_residual's syntax; nC
 *             from the left / top TotalCoeffs, MBs outside the rect
 *             available with 0, picture edges unavailable);
 *   nonzero   the sum of TotalCoeff over the rect's blocks (luma, chroma DC,
 *             chroma AC).
 * From bits to a size: nothing else in the dynamic NAL depends on the QP but
 * slice_qp_delta, so its RBSP bits before the stop bit are
 *     bits(q) + len(se(q - 26)) + C(frame),
 * C one constant per frame (slice header, MB heads, static rows): known from
 * any one compose or probe-and-compose of that frame, and it cancels when
 * candidates are compared.  Emulation-prevention bytes come on top.
 *
 *   scroll_batch_dyn_probe(b, nframes, qps, nq, hip_stream)   asynchronous on
 *       hip_stream (0 = the batch's own).  SCROLL_ERR_CONFIG without a
 *       dynamic rect or references, and with UI hints set (the rect under
 *       hints is not probed: clear the hints); SCROLL_ERR_ARG for nq outside
 *       1..SCROLL_DYN_PROBE_MAX_QPS, a QP outside 0..51 or nframes outside
 *       0..max_frames.  A stream that must keep QP 26 (its config has the
 *       deblocking filter on) is probed like any other: its numbers at other
 *       QPs are informational.
 *   scroll_batch_dyn_probe_result(b, s, f, k, out)   candidate k of frame f of
 *       stream s of the last probe; synchronises the probe's stream.  0; 1
 *       when the frame has no dynamic NAL (a waypoint frame in experiment
 *       mode; nothing written), as scroll_batch_dyn_frame_info;
 *       SCROLL_ERR_ARG for s, f or k outside the last probe;
 *       SCROLL_ERR_CONFIG before any probe or after set_dyn_rect dropped it;
 *       SCROLL_ERR_DEVICE if not every rect row of the frame was counted
 *       (never 0 over partial sums).
 *   scroll_batch_dyn_probe_device(b, &ls, &lf)   the device results,
 *       [stream][frame][SCROLL_DYN_PROBE_MAX_QPS] at byte strides ls / lf;
 *       NULL before the first probe.  Valid on the probe's stream after it.
 *   scroll_batch_dyn_probe_ms(b)   with scroll_batch_enable_timing: HIP-event
 *       ms of the last probe's launches; -1 without. */
#define SCROLL_DYN_PROBE_MAX_QPS 8
typedef struct {
    uint64_t sse[3];    /* Y, Cb, Cr: what scroll_batch_dyn_sse would report at this QP */
    uint32_t bits;      /* the rect MBs' coded_block_pattern + mb_qp_delta + residual bits */
    uint32_t nonzero;   /* sum of TotalCoeff over the rect's blocks (luma, chroma DC, chroma AC) */
} ScrollDynProbe;       /* 32 bytes */
int scroll_batch_dyn_probe(ScrollBatch *b, int nframes, const uint8_t *qps, int nq, void *hip_stream);
int scroll_batch_dyn_probe_result(ScrollBatch *b, int s, int f, int k, ScrollDynProbe *out);
const ScrollDynProbe *scroll_batch_dyn_probe_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride);
float scroll_batch_dyn_probe_ms(ScrollBatch *b);   /* with enable_timing; -1 without */

/* ---- the same probe for the rect under UI hints ----
 * scroll_batch_dyn_probe_hinted(b, nframes, qps, nq, hip_stream) answers for
 * the rect the next scroll_batch_compose(b, nframes) would code with UI hints
 * set: the offsets, source, hint records, per-frame rect positions
 * (scroll_batch_set_dyn_rect_at) and fallback setting as they stand; the
 * frames' own QPs (scroll_batch_set_dyn_qp_at) are ignored.  Every rect MB
 * takes the (ref, mv) of its topmost hint rect, else of its scroll row; a
 * frame that falls back (scroll_batch_set_fallback) is probed as the whole
 * picture without hint rects.  Arguments, candidate limit, argument errors
 * and asynchrony are scroll_batch_dyn_probe's, results come through the
 * accessors above, ScrollDynProbe means the same (sse: scroll_batch_dyn_sse
 * after a hinted compose of that frame at q; an MB with
 * coded_block_pattern 0 counts its one-bit code whether or not the composer
 * then writes it as P_Skip), and nothing is committed: HintFrame flags,
 * scroll_batch_fallback_frame and everything of the last compose stay.  It
 * does the hint / position uploads the next compose would do anyway.
 *
 * From bits to a size: under hints slice_qp_delta is 0, the first rect MB
 * with coded_block_pattern != 0 in raster order carries mb_qp_delta = q - 26
 * and the others 0.  With
 *     D(q) = len(se(q - 26)) - 1  if nonzero(q) > 0, else 0
 * the scroll NAL's RBSP bits before the stop bit are
 *     bits(q) + D(q) + C(frame)
 * exactly in SCROLL_HINT_EXACT and SCROLL_HINT_SPEC; in SCROLL_HINT_PSKIP
 * exactly while no rect MB is written as P_Skip and strictly more than the
 * NAL otherwise (a skipped MB drops at least five header bits and lengthens
 * a skip run by at most one): an upper bound that is safe for a budget.
 * bits says nothing about an MB outgrowing its slot_bytes / (w h) region
 * (SCROLL_ERR_OVERFLOW at the compose).
 *
 * SCROLL_ERR_CONFIG without a dynamic rect or references, without UI hints
 * (that is scroll_batch_dyn_probe's case) and with any spliced slice in the
 * batch.  scroll_batch_dyn_probe_result after it: 0; 1 (nothing written) for
 * a frame without a dynamic NAL, without the rect (set_dyn_rect_at x0 = -1)
 * or with a dormant fallback region that does not fall back;
 * SCROLL_ERR_CONFIG for a frame -- that frame only -- whose hint rects name a
 * reference it lacks while the fallback is off (the compose would fail the
 * stream); SCROLL_ERR_DEVICE as above. */
int scroll_batch_dyn_probe_hinted(ScrollBatch *b, int nframes, const uint8_t *qps, int nq, void *hip_stream);

/* ---- the plain rect at a QP of its own per frame ----
 * A table of one byte per (stream, frame of the compose) on the device,
 * [s * stream_stride + f]: 0xFF the stream's QP (scroll_batch_set_dyn_qp /
 * _stream), any other value that frame's QP, 0..51 (a byte above 51 that a
 * caller's own kernel writes counts as 0xFF).  Entry f applies to frame f of
 * every following scroll_batch_compose of the plain dynamic rect until it is
 * changed or cleared, whatever nframes that compose has.  Frame f's dynamic
 * scroll NAL then carries slice_qp_delta = its QP - 26 and is coded, decoded
 * (scroll_batch_set_dyn_recon) and measured at that QP; a frame below 22 goes
 * the general path on its own, beside int8 frames of the same stream.  An
 * entry of a frame without a dynamic NAL (a waypoint frame in experiment
 * mode) is ignored.  Prediction is from the static pictures only, so frame
 * f's NAL is the NAL of a compose with every frame at that QP.  Bit-exact
 * definition: oracle/dyn_oracle.h or_compose_dyn, called per frame with the
 * frame's QP in its or_dyn_rect.
 * The table is allocated by the first call below that needs it and freed by
 * scroll_batch_set_dyn_rect and scroll_batch_destroy; without it no compose
 * gains a launch, an allocation or a changed byte.
 *
 *   scroll_batch_set_dyn_qp_frames(b, s, f0, n, qps)   entries f0 .. f0 + n - 1
 *       of stream s (s = -1: of every stream) from qps[0..n), -1 = the
 *       stream's QP.  SCROLL_ERR_CONFIG without the dynamic rect or with UI
 *       hints set (under hints the per-frame QP is scroll_batch_set_dyn_qp_at's),
 *       and for a QP other than 26 or -1 on a stream with the deblocking
 *       filter on; SCROLL_ERR_ARG for a range outside 0..max_frames or a QP
 *       outside -1..51.  Synchronises the batch.  Frames below 22 get their
 *       general-path record slots here, not at a failing compose.
 *   scroll_batch_clear_dyn_qp_frames(b)   every entry back to 0xFF.
 *   scroll_batch_dyn_qp_frames(b, s, f0, n, out)   the entries as they stand on
 *       the device (-1 for 0xFF), after everything queued on the batch's last
 *       stream and the last pick's: how a caller learns what
 *       scroll_batch_dyn_pick chose.  All -1 before the table exists.
 *   scroll_batch_dyn_qp_frames_device(b, &stream_stride)   the table itself, for
 *       a caller's own kernel on the compose's stream (allocated, all 0xFF,
 *       if it was not; NULL without the dynamic rect or when that fails).
 *       The general-path pool is then sized for whatever QPs it may hold by
 *       the existing overflow status: a compose that runs out fails the
 *       frames concerned with SCROLL_ERR_OVERFLOW, grows the pool, and the
 *       caller composes again.
 * A scroll_batch_compose with UI hints set while any entry differs from 0xFF
 * returns SCROLL_ERR_CONFIG and commits nothing. */
int scroll_batch_set_dyn_qp_frames(ScrollBatch *b, int s, int f0, int n, const int8_t *qps);
int scroll_batch_clear_dyn_qp_frames(ScrollBatch *b);
int scroll_batch_dyn_qp_frames(ScrollBatch *b, int s, int f0, int n, int8_t *out);
uint8_t *scroll_batch_dyn_qp_frames_device(ScrollBatch *b, size_t *stream_stride);

/* ---- picking those QPs on the device, from the probe ----
 * scroll_batch_dyn_pick(b, nframes, &rate, frame_bits_per_stream, hip_stream)
 * reads the last scroll_batch_dyn_probe's device results and row counters and
 * writes entries 0 .. nframes - 1 of every stream of the table above: no
 * result crosses to the host.  Asynchronous on hip_stream (0 = the batch's
 * own), which must be the stream of the probe before it and of the compose
 * after it.
 *
 * The cost of candidate k of a frame is the QP-dependent part of its NAL's
 * RBSP bits, cost(k) = bits[k] + len(se(qp[k] - 26)) (C(frame) above cancels).
 * pick(allow): among the candidates with cost <= allow the smallest
 * sse[0] + sse[1] + sse[2]; ties go to the smaller cost, then to the earlier
 * candidate.  If none fits, the candidate with the smallest cost (ties to the
 * smaller error, then to the earlier one), reported as over.
 *   SCROLL_DYN_RATE_FRAME    allow = frame_bits for every frame; stateless.
 *   SCROLL_DYN_RATE_BUCKET   a leaky bucket per stream, its signed 64-bit level
 *       kept on the device across calls.  Every frame of the pick in order --
 *       a frame that gets no choice included, at cost 0 --
 *           allow = min(bucket_bits, level + frame_bits)
 *           pick(max(allow, 0))
 *           level = max(allow - cost(chosen), -bucket_bits).
 *       The level moves at the pick, not at the compose: a pick that is not
 *       followed by its compose, or is made twice, has still spent.
 *       scroll_batch_set_dyn_rect resets every level to 0.
 * frame_bits_per_stream: num_streams host values replacing rate.frame_bits,
 * or NULL.
 * A frame gets its chosen QP; it gets 0xFF and no choice when the probe found
 * no dynamic NAL in it, when its stream has the deblocking filter on (it
 * keeps QP 26), or when the probe did not count every rect row of it.
 * With a candidate below 22 the general-path record pool is sized here for
 * every frame taking one (this call then synchronises the batch once).
 * SCROLL_ERR_CONFIG before any plain probe, when the last probe was the
 * hinted one, for nframes beyond the last probe's, and with UI hints set;
 * SCROLL_ERR_ARG for a NULL rate or an unknown mode.
 *
 *   scroll_batch_dyn_pick_result(b, s, f, &k, &qp)   frame f of stream s of the
 *       last pick; synchronises its stream.  0: candidate k at QP qp within
 *       the allowance; 1: the cheapest candidate, over it; 2: nothing chosen,
 *       the frame keeps the stream's QP (k and qp are -1); SCROLL_ERR_DEVICE
 *       for a frame whose rows were not all counted; SCROLL_ERR_CONFIG before
 *       any pick; SCROLL_ERR_ARG outside the last pick.
 *   scroll_batch_dyn_rate_level(b, s, &level, set)   stream s's bucket level:
 *       set = 0 reads it (after the last pick), set != 0 writes *level. */
#define SCROLL_DYN_RATE_FRAME  0
#define SCROLL_DYN_RATE_BUCKET 1
typedef struct {
    uint32_t mode;          /* SCROLL_DYN_RATE_* */
    uint32_t frame_bits;    /* FRAME: the allowance; BUCKET: what every frame adds to the level */
    uint32_t bucket_bits;   /* BUCKET: the level's cap, and the cap of its debt */
    uint32_t pad;
} ScrollDynRate;
int scroll_batch_dyn_pick(ScrollBatch *b, int nframes, const ScrollDynRate *rate,
                          const uint32_t *frame_bits_per_stream, void *hip_stream);
int scroll_batch_dyn_pick_result(ScrollBatch *b, int s, int f, int *k, int *qp);
int scroll_batch_dyn_rate_level(ScrollBatch *b, int s, int64_t *level, int set);
/* HIP-event ms of the timed composes since the last call: plan (both
 * passes), emit, dyn stage (= dyn code + dyn pack), dyn emit, dyn code
 * (k_dyn_rows + k_dyn_code), dyn pack (k_dyn_group + k_dyn_ep); accumulators reset
 * afterwards */
int scroll_batch_kernel_stats_ex(ScrollBatch *b, double ms[6], int *count);

/* ---- UI hints (reference design docs/MASTER_DESIGN.md:
 * 58-64,103-146, no reference implementation) ----
 * Rectangles of MBs with their own reference and displacement, laid over
 * the scroll layout of the frame's offset: static chrome, a horizontally
 * scrolling row, a second pane.  MBs no rect covers keep the scroll frame's
 * (ref, mv).  Later rects lie on top.  Bit-exact definition:
 * oracle/hint_oracle.h.  Once hints are set, every scroll NAL of the batch
 * is coded per MB (waypoint NALs are unchanged); a frame without hints then
 * equals the reference's scroll frame byte for byte in SCROLL_HINT_EXACT.
 *
 *   modes: SCROLL_HINT_EXACT  the reference's MB syntax (mb_skip_run 0,
 *              get_mv_prediction of h264_writer.c:369-432) for any MV field;
 *          SCROLL_HINT_PSKIP  standard median prediction (H.264 8.4.1.3) and
 *              P_Skip runs for ref-0 MBs on their skip motion (8.4.1.1);
 *          SCROLL_HINT_SPEC   the reference's MB syntax (no skipped MBs) with
 *              the standard's median prediction: a standard decoder gets the
 *              intended motion for any MV field, and the plain scroll layout
 *              is still the reference's frame byte for byte (a row-uniform
 *              field never reaches the cases where get_mv_prediction departs
 *              from 8.4.1.3).
 *   scroll_batch_set_hints(b, s, f, rects, n, mode)   hints of frame f (the
 *       f-th frame of each following compose) of stream s; n <=
 *       SCROLL_HINT_MAX_RECTS; n = 0 gives the plain layout in `mode`.  A
 *       rect whose ref is not a valid reference of its frame (2 + i needs
 *       waypoint i) fails that stream's compose with SCROLL_ERR_CONFIG.
 *   scroll_batch_clear_hints(b)   back to plain scroll frames (k_emit path).
 * Pictures up to 240 MBs (3840 px) wide.
 * With a dynamic rect: see scroll_batch_set_dyn_rect_at. */
#define SCROLL_HINT_EXACT 0
#define SCROLL_HINT_PSKIP 1
#define SCROLL_HINT_SPEC 2
#define SCROLL_HINT_MAX_RECTS 64
#define SCROLL_HINT_MAX_MV 8192     /* |mv_x|, |mv_y| in pixels */
typedef struct ScrollHintRect {
    int16_t x0, y0, x1, y1;         /* MBs [x0, x1) x [y0, y1), clipped to the picture */
    int16_t ref;                    /* 0 = A, 1 = B, 2 + i = waypoint i               */
    int16_t reserved;               /* 0                                              */
    int32_t mv_x, mv_y;             /* pixels: MB (x, y) predicts from (16x + mv_x, 16y + mv_y) */
} ScrollHintRect;
int scroll_batch_set_hints(ScrollBatch *b, int s, int f, const ScrollHintRect *rects, int n,
                           int mode);
int scroll_batch_clear_hints(ScrollBatch *b);

/* ---- pre-encoded MB splice (reference design
 * docs/MASTER_DESIGN.md:39-40,87-90,142-146,166-171, no reference
 * implementation) ----
 * The MBs of an external P slice -- a conventional encoder's output for the
 * dynamic rect, coded as its own w x h MB picture -- are transplanted into
 * the rect [x0, x0 + w) x [y0, y0 + h) of frame f's scroll NAL: P_Skip MBs
 * become P_L0_16x16 with their skip motion, partitioned MBs keep their
 * partitioning (P_8x8ref0 written as P_8x8 with ref_idx 0), mb_skip_run /
 * ref_idx / every (sub-)partition's mvd are re-coded for the composed
 * picture (4x4-block neighbours, 8.4.1.3), mb_qp_delta rebased to the composed
 * slice QP, each residual block keeps its bits after coeff_token and gets
 * the coeff_token of its composed nC.  MBs outside the rect follow the frame's
 * UI hints (a splice turns the hint path on in SCROLL_HINT_SPEC, so a standard
 * decoder gets the spliced motion, and frames without a splice and without
 * hints still equal the reference's scroll frames; set_hints(.., NULL, 0,
 * SCROLL_HINT_PSKIP) adds P_Skip runs, SCROLL_HINT_EXACT the reference's own
 * predictor).
 * Bit-exact definition: oracle/splice_oracle.h.
 *
 * The external picture: one NAL (Annex-B start code optional), or several
 * Annex-B NAL units -- its slices, in MB order, each starting at the MB after
 * the previous one's last (first_mb_in_slice), together covering the w*h MBs
 * (at most 1,024 slices; each is parsed by its own wave); P slices or I
 * slices (nal_unit_type 1, or 5 for an IDR picture: a conventional encoder's
 * first frame and scene cuts; an I slice's MBs are the P slice's intra types,
 * without mb_skip_run), CAVLC, parsed with the composed stream's SPS/PPS (log2_max_frame_num, POC
 * type, 2 default references, disable_deblocking_filter_idc 1 when the
 * stream signals deblocking control); no ref_pic_list_modification, or one
 * that restates the composed list (op k: long_term_pic_num k, as the
 * composer's own slices write it); MBs of any inter type (P_L0_16x16,
 * P_L0_L0_16x8 / 8x16, P_8x8 with any sub_mb_types, P_8x8ref0), P_Skip, and
 * the intra types of a P slice (I_4x4, I_16x16, I_PCM) where the neighbour
 * MBs their sample prediction reads have the same availability in the
 * external and the composed picture (so not on the rect's left / top edge
 * unless that is the picture's, no above-right I_4x4 modes on its right
 * edge; I_PCM anywhere; splice_oracle.h has the rule);
 * ref_idx 0 = A, 1 = B, 2 + i = waypoint i of the composed stream; motion
 * vectors are displacements in the composed picture, |mv| <= 16383 quarter
 * pels; CAVLC level_prefix <= 15 (Baseline / Main).
 *
 *   scroll_batch_set_splice(b, s, f, x0, y0, w, h, nal, n)   frame f of
 *       stream s, for every following compose; n = 0 removes it.  The slice
 *       is parsed on the GPU by the next compose; a slice outside the
 *       supported syntax, or a reference the frame does not have, fails that
 *       stream's compose with SCROLL_ERR_CONFIG (nothing of the batch is
 *       written for the stream) and scroll_batch_splice_status gives the
 *       reason (SCROLL_SPLICE_ERR_*).
 *   scroll_batch_clear_splices(b)   remove every splice (hints stay).
 * The staging slots grow to the largest spliced NAL's bound (about the
 * external slice plus 16 bytes per picture MB) for every (stream, frame). */
#define SCROLL_SPLICE_MAX_BYTES   ((uint64_t)1 << 29)   /* n < 512 MiB: 32-bit bit offsets */
#define SCROLL_SPLICE_OK          0
#define SCROLL_SPLICE_ERR_NAL     1   /* not a coded slice (nal_unit_type 1 / 5), or
                                       * more than 1,024 slices                      */
#define SCROLL_SPLICE_ERR_HEADER  2   /* slice header outside the supported syntax  */
#define SCROLL_SPLICE_ERR_MBTYPE  3   /* an intra MB whose prediction would change   */
#define SCROLL_SPLICE_ERR_SYNTAX  4   /* malformed, truncated or MB count mismatch   */
#define SCROLL_SPLICE_ERR_REF     5   /* ref_idx not a valid reference of the frame  */
int scroll_batch_set_splice(ScrollBatch *b, int s, int f, int x0, int y0, int w, int h,
                            const uint8_t *nal, size_t n);
/* the same for many frames at once, the NALs already in device memory (e.g.
 * a dynamic encoder's output arena on the same GPU): nal = device pointer,
 * read by the next compose (keep it valid and unchanged until that compose
 * has been synced); n = 0 removes the entry's splice.  Each call marks the
 * slices changed, so the next compose parses them again (new content in
 * place needs only another call). */
typedef struct ScrollSpliceDesc {
    int32_t s, f;                   /* stream, frame                              */
    int32_t x0, y0, w, h;           /* MB rect                                    */
    const uint8_t *nal;             /* device pointer to the external NAL         */
    uint64_t n;                     /* its bytes                                  */
} ScrollSpliceDesc;
int scroll_batch_set_splices_device(ScrollBatch *b, int n, const ScrollSpliceDesc *d);
int scroll_batch_clear_splices(ScrollBatch *b);
/* after sync: SCROLL_SPLICE_* of frame f of stream s in the last compose
 * (SCROLL_SPLICE_OK also when the frame has no splice) */
int scroll_batch_splice_status(ScrollBatch *b, int s, int f, int *status);
/* the same, and for SCROLL_SPLICE_ERR_MBTYPE the refused MB: its position in
 * the external picture (MB units) and its mb_type in P-slice numbering (5
 * I_4x4, 6..29 I_16x16; an I slice's k is 5 + k) -- the MB a caller can
 * re-code as I_PCM or with a mode that reads no neighbour across the rect's
 * edge (the margin ring, docs/MASTER_DESIGN.md:54-56); -1 otherwise */
int scroll_batch_splice_refusal(ScrollBatch *b, int s, int f, int *status, int *mb_x, int *mb_y, int *mb_type);

/* ---- stream ingest on the GPU ----
 * Batched composer_init + composer_write_header (reference src/composer.c:
 * 127-253): n new streams from their reference files (Annex-B with SPS, PPS
 * and an IDR slice: A and B), parsed and rewritten on the GPU.  Each new
 * stream's arena starts with SPS + PPS + IDR A (long-term 0) + non-IDR I B
 * (long-term 1), byte-identical to the reference; its config is the one
 * composer_init derives (log2_max_frame_num 4, POC type 2, A's deblocking
 * flag; frame_num 2 after the header).  Synchronous.  On an error no stream
 * is added and the message names the first failing one (missing NAL unit,
 * unsupported SPS/PPS, A/B size mismatch, header larger than the arena).
 *   scroll_batch_ingest(b, n, a, na, b_, nb, &first)   host files
 *   scroll_batch_ingest_device(b, n, d_files, desc, &first)   files already in
 *       device memory: desc[4k..4k+3] = offset, size of A, offset, size of B
 * The new streams get ids first .. first + n - 1.
 * Device scratch, kept by the batch for later calls: 2 n x 1.25 x the LARGEST
 * file's bytes (each slice body's 16 KB segments keep their output bytes
 * between the summary and the write pass, every file sized like the largest)
 * while that stays under 8 GB and under 4 x the input's bytes + 256 MB, else a
 * few hundred bytes per segment of the largest file (the write pass decodes
 * again).  Slices over 16 MB go one workgroup per stream, without scratch. */
int scroll_batch_ingest(ScrollBatch *b, int n, const uint8_t *const *ref_a, const size_t *na,
                        const uint8_t *const *ref_b, const size_t *nb, int *first);
int scroll_batch_ingest_device(ScrollBatch *b, int n, const uint8_t *d_files,
                               const uint64_t *desc, int *first);

/* Mid-stream long-term reference ("atlas") update -- SURVEY 8f row 3; the
 * reference only installs A / B at composer_write_header.  Entry k: the IDR
 * picture of Annex-B file k (parse_reference_file's rules, parsed with the
 * file's own SPS / PPS) becomes a non-IDR I frame of stream streams[k]
 * marked long_term_frame_idx which[k] (0 = A, 1 = B): the reference's
 * h264_rewrite_as_non_idr_i_frame (h264_writer.c:296-350) with the index as
 * a parameter, at the stream's frame_num, written with the stream's config,
 * appended after everything composed so far.  Its MMCO 4
 * (max_long_term_frame_idx_plus1 = 2) drops the stream's waypoints, so the
 * stream continues with an empty waypoint table and frame_num + 1; later
 * scroll frames predict from the new picture.  Streams distinct per call;
 * the picture must have the stream's size.  Synchronous; status[k] (may be
 * NULL) = 0 or the ingest error class (1 missing NAL, 2 refused SPS / PPS,
 * 3 size, 4 too many NALs, 5 arena full: nothing appended).  For a batch
 * with a dynamic rect also give the stream its new pictures
 * (scroll_batch_set_dyn_refs): prediction reads those. */
int scroll_batch_update_refs(ScrollBatch *b, int n, const int *streams, const int *which,
                             const uint8_t *const *files, const size_t *sizes, int *status);
/* the same from files already on the device (desc: offset, size per entry) */
int scroll_batch_update_refs_device(ScrollBatch *b, int n, const int *streams, const int *which,
                                    const uint8_t *d_files, const uint64_t *desc, int *status);
/* with timing enabled: summed ms of the ingest kernels (HIP events on the
 * batch's stream) and the number of ingest calls since the last call */
int scroll_batch_ingest_stats(ScrollBatch *b, double *ms, int *count);

/* ---- reference files from pictures on the GPU ----
 * The experiment's I_PCM reference writer (experiments/scroll-encoder/src/
 * h264_encoder.c:730-918: SPS + PPS + an IDR slice of I_PCM MBs, as the
 * SURVEY Appendix B harness frames it) generalised from one stripe colour per
 * MB to any I420 picture: n pictures at d_pics + i * pic_stride (Y w*h, then
 * Cb, Cr w*h/4 each, device memory) become n Annex-B files at d_out + i *
 * out_stride (device memory); sizes[i] (host) receives each file's bytes.
 * The files are what scroll_batch_ingest_device reads, so new streams (or a
 * new long-term reference picture) go from pixels to a composing stream
 * without leaving the GPU.  Synchronous; SCROLL_ERR_OVERFLOW (the sizes are
 * filled, nothing written) when a file exceeds out_stride -- at most
 * 1.5 x (w*h*193/128) + 128 bytes.  w, h multiples of 16, < 65536 MBs.
 * Device scratch, kept by the batch: the files' RBSP bytes (n x about 1.5 x
 * w*h, 4 KB aligned) while under 4 GB, which the write pass reads instead of
 * generating them again. */
int scroll_batch_ipcm_files_device(ScrollBatch *b, int n, int w, int h, const uint8_t *d_pics,
                                   size_t pic_stride, uint8_t *d_out, size_t out_stride,
                                   uint64_t *sizes);
/* the same without the host step: the sizes go to d_sizes (device, n u64)
 * and the call returns once its launches are queued on the batch's stream;
 * a file past out_stride (that call then writes no file) is reported by the
 * next scroll_batch_sync as SCROLL_ERR_OVERFLOW.  For pipelines that feed
 * the files straight to scroll_batch_ingest_device; the scratch is the
 * batch's, so calls of one batch run in stream order. */
int scroll_batch_ipcm_files_device_async(ScrollBatch *b, int n, int w, int h, const uint8_t *d_pics,
                                         size_t pic_stride, uint8_t *d_out, size_t out_stride,
                                         uint64_t *d_sizes);
/* with timing enabled: summed kernel ms of the calls above since the last
 * call (both passes) and the number of calls */
int scroll_batch_ipcm_stats(ScrollBatch *b, double *ms, int *count);

/* ---- pixels from renderer surfaces (docs/MASTER_DESIGN.md §5: "dynamic-region
 * pixels for frame N (cropped from renderer)") ----
 * A renderer hands out 8-bit RGBA or BGRA framebuffers; the rect's source,
 * the references and the I_PCM writer above take planar I420.  These calls
 * crop, convert and subsample on the device, by one exact integer rule
 * (csrc/csc_device.h; alpha ignored):
 *     Y = (yr R + yg G + yb B + yoff) >> 16                         per pixel
 *     C = clamp((cr Sr + cg Sg + cb Sb + (128 << 18) + (1 << 17)) >> 18, 0, 255)
 * per 2x2 quad, Sr Sg Sb the quad's channel sums (box siting: the chroma
 * sample sits at the quad's centre), Q16 coefficients of BT.601 or BT.709 in
 * limited (16..235 / 16..240) or full range.  Every output is within 0.506
 * of the real-valued matrix.
 *
 * ScrollSurfaces: frame f of stream s is the surface at base + s
 * stream_stride + f frame_stride, rows pitch bytes apart, 4 bytes per pixel.
 * base, pitch and both strides are multiples of 16 (every load is then a full
 * 16-byte vector load); pitch covers the surface's width.
 *
 *   scroll_batch_dyn_source_from_surfaces(b, nframes, &surf, hip_stream)
 *       fills frames 0 .. nframes - 1 of every stream of the source buffer
 *       (scroll_batch_set_dyn_source's, scroll_batch_dyn_source_device's
 *       layout).  cropped = 0: the surfaces are whole pictures and frame f of
 *       stream s is cut out where its rect sits -- scroll_batch_set_dyn_rect's
 *       position, or scroll_batch_set_dyn_rect_at's; cropped = 1: they are the
 *       rect itself, 16w x 16h pixels.  A frame without a rect (set_dyn_rect_at
 *       with x0 = -1) and frames from nframes on keep their bytes -- except
 *       with the fallback on (scroll_batch_set_fallback): there a frame
 *       without the rect is coded as the whole picture from its source block
 *       if it falls back, which only the compose decides, so it is converted
 *       like a frame with the rect at (0, 0) (the rect is the whole picture).
 *       Asynchronous on hip_stream (0 = the batch's own), which must be the
 *       stream of the probe or compose that reads the source.  The batch's
 *       host-side calls do not wait for it: synchronise hip_stream before a
 *       scroll_batch_set_dyn_source / _synth into the same buffer and
 *       before the surfaces are rewritten or freed.  With per-frame
 *       positions the call first waits for the
 *       previous such call's kernel (it uploads a table of them).
 *       SCROLL_ERR_CONFIG without a dynamic rect; SCROLL_ERR_ARG, and nothing
 *       written, for a misaligned base, pitch or stride, an unknown format or
 *       matrix, nframes outside 0..max_frames, a pitch smaller than the
 *       surface's row, or more than 2^35 pixels in one call.
 *   scroll_batch_surfaces_to_i420(b, n, w, h, &surf, d_pics, pic_stride, hip_stream)
 *       n whole w x h surfaces (multiples of 16) at base + i frame_stride
 *       become I420 pictures at d_pics + i pic_stride (Y w*h, then Cb, Cr
 *       w*h/4 each; d_pics and pic_stride multiples of 16): what
 *       scroll_batch_ipcm_files_device and scroll_batch_set_dyn_refs_device
 *       read.  stream_stride and cropped are ignored.  Needs no dynamic rect.
 *       Asynchronous on hip_stream: scroll_batch_ipcm_files_device runs on the
 *       batch's own stream, so synchronise hip_stream first unless it is that
 *       one (0).  At most 2^35 pixels per call (SCROLL_ERR_ARG).
 *   scroll_batch_set_dyn_refs_device(b, s, d_ref_a, d_ref_b)
 *       scroll_batch_set_dyn_refs with the pictures in device memory (a
 *       device-to-device copy, the same shared / per-stream semantics;
 *       synchronous), so pictures go from renderer surfaces to the coder's
 *       references without a host step.
 *   scroll_batch_surface_ms(b)   with scroll_batch_enable_timing: HIP-event ms
 *       of the last conversion's launches; -1 without.
 * A compose that uses none of these gains no launch, allocation or changed
 * byte. */
#define SCROLL_SURF_RGBA  0         /* bytes in memory: R, G, B, A */
#define SCROLL_SURF_BGRA  1         /* bytes in memory: B, G, R, A */
#define SCROLL_SURF_BT601 0
#define SCROLL_SURF_BT709 1
typedef struct {
    const uint8_t *base;        /* device memory */
    uint64_t pitch;             /* bytes per pixel row */
    uint64_t frame_stride;      /* bytes between a stream's consecutive frames */
    uint64_t stream_stride;     /* bytes between streams; 0: every stream reads the same surfaces */
    uint32_t format;            /* SCROLL_SURF_RGBA / SCROLL_SURF_BGRA */
    uint32_t matrix;            /* SCROLL_SURF_BT601 / SCROLL_SURF_BT709 */
    uint32_t full_range;        /* 0 limited (16..235 / 16..240), 1 full */
    uint32_t cropped;           /* 0: surfaces are whole pictures, the rect is cut out at each frame's rect
                                   position; 1: surfaces are the rect itself, 16w x 16h pixels */
} ScrollSurfaces;
int scroll_batch_dyn_source_from_surfaces(ScrollBatch *b, int nframes, const ScrollSurfaces *surf, void *hip_stream);
int scroll_batch_surfaces_to_i420(ScrollBatch *b, int n, int w, int h, const ScrollSurfaces *surf,
                                  uint8_t *d_pics, size_t pic_stride, void *hip_stream);
int scroll_batch_set_dyn_refs_device(ScrollBatch *b, int s, const uint8_t *d_ref_a, const uint8_t *d_ref_b);
float scroll_batch_surface_ms(ScrollBatch *b);   /* with enable_timing; -1 without */

/* ---- the dynamic rect located from the surfaces (docs/MASTER_DESIGN.md §7.1) ----
 * Where the rect sits need not come from the renderer: the device holds the
 * surfaces and the exact luma a decoder shows for a scroll MB without
 * residual, and compares the two per MB (csrc/damage_device.h):
 *     D(mx, my) = sum over the MB's 256 pixels of (Ysrc - Ypred)^2
 * Ysrc: the luma rule above on the surface pixel; Ypred: the luma prediction
 * of the scroll NAL a compose at scroll_batch_set_offsets' offsets would
 * write for the frame (full-pel rows of reference picture A / B, waypoints
 * resolved).  Luma only: a change of colour with unchanged luma is not seen.
 * Against the prediction: with the loop filter on (an ingested stream) the
 * decoded picture can differ from it at the seam of the two regions.
 * An MB is damaged iff D > mb_sse; the damaged MBs' bounding box, grown by
 * margin MBs (0..4) on each side and clipped to the picture, is where the
 * w x h rect goes: x0 = min(bx0, mbw - w), y0 = min(by0, mbh - h).
 *   SCROLL_DYN_LOC_NONE     nothing damaged: no rect (x0 = y0 = -1), box 0
 *   SCROLL_DYN_LOC_FIT      the box is at most w x h: the rect covers it
 *   SCROLL_DYN_LOC_OVER     it is larger: the rect covers its top-left part
 *   SCROLL_DYN_LOC_NOFRAME  the frame has no scroll NAL (experiment mode's
 *                           waypoint frame): no rect, zero map entries
 * sse_all: the sum of D over the picture, sse_out: over the MBs outside the
 * placed rect (sse_all without one) -- the luma squared error of the
 * displayed frame that the rect cannot mend, in scroll_batch_dyn_sse's units;
 * max_sse: the largest D.
 *
 *   scroll_batch_dyn_locate(b, nframes, &surf, &rule, hip_stream)
 *       frames 0 .. nframes - 1 of every stream: the map, the records and,
 *       with rule.apply = 1, the frames' positions (what
 *       scroll_batch_set_dyn_rect_at would have been called with; entries
 *       from nframes on keep their values).  A dry state pass (nothing of the
 *       batch's state changes), then k_dmg_rows, k_dyn_damage, k_dyn_place.
 *       Asynchronous on hip_stream (0 = the batch's own), which must be the
 *       stream of the surface conversion, probe and compose that follow: a
 *       tick is set_offsets -> locate -> dyn_source_from_surfaces (which cuts
 *       at the located positions) -> [probe -> pick] -> compose, without a
 *       host synchronisation.  Reading the positions on the host
 *       (scroll_batch_set_dyn_rect_at merging one entry, hints turned on,
 *       scroll_batch_set_dyn_rect_moving off) synchronises and reads them back.
 *       The surfaces are whole pictures: cropped = 1 is SCROLL_ERR_ARG, as
 *       are the surface checks above, nframes outside 0..max_frames, margin
 *       > 4 and apply > 1.  SCROLL_ERR_CONFIG without a dynamic rect with
 *       reference pictures, with UI hints set, and for apply = 1 without
 *       scroll_batch_set_dyn_rect_moving.  A refused call writes nothing.
 *       Buffers (records, map, a row table of 4 bytes per picture row and
 *       frame, the dry pass's plan) are allocated by the first call and go
 *       with the rect; a batch that never calls it gains no launch,
 *       allocation or changed byte.
 *       rule.size (the rule's fourth word, which was reserved and 0): 0 as
 *       above, byte for byte, the records included.  1, with apply = 1: the
 *       rect keeps the placed origin and is also sized per frame
 *       (scroll_batch_set_dyn_rect_size_at's contract), w_f = min(bx1, x0 +
 *       w) - x0, h_f = min(by1, y0 + h) - y0: a FIT rect covers exactly
 *       origin-to-box-end, an OVER rect is the batch size where it is over.
 *       sse_out is then summed outside the sized rect and the record's
 *       reserved holds (w_f - 1) | (h_f - 1) << 8 on FIT / OVER, else 0.
 *       size > 1, or size = 1 without apply, is SCROLL_ERR_ARG; size = 1
 *       needs what set_dyn_rect_size_at needs (SCROLL_ERR_CONFIG).
 *   scroll_batch_dyn_locate_result / _damage_map  one frame's record / its
 *       mbw * mbh map entries, row by row (synchronising; SCROLL_ERR_CONFIG
 *       before the first locate, SCROLL_ERR_ARG outside the last one)
 *   scroll_batch_dyn_locate_device / _damage_map_device   the device arrays,
 *       [stream][frame] records (stream_stride in bytes) and [stream][frame]
 *       [mbh][mbw] uint32 (strides in bytes); NULL before the first locate
 *   scroll_batch_dyn_locate_ms   with scroll_batch_enable_timing: HIP-event
 *       ms of the last locate's launches; -1 without. */
#define SCROLL_DYN_LOC_NONE    0
#define SCROLL_DYN_LOC_FIT     1
#define SCROLL_DYN_LOC_OVER    2
#define SCROLL_DYN_LOC_NOFRAME 3
typedef struct {
    int16_t  x0, y0;               /* placed origin in MBs; x0 = -1: none */
    uint16_t bx0, by0, bx1, by1;   /* the box after the margin, [bx0,bx1) x [by0,by1); 0 when none */
    uint16_t status, reserved;     /* SCROLL_DYN_LOC_* */
    uint32_t n_mb, max_sse;
    uint64_t sse_all, sse_out;
} ScrollDynDamage;                 /* 40 bytes */
typedef struct { uint32_t mb_sse, margin, apply, size; } ScrollDynLocate;
int scroll_batch_dyn_locate(ScrollBatch *b, int nframes, const ScrollSurfaces *surf,
                            const ScrollDynLocate *rule, void *hip_stream);
int scroll_batch_dyn_locate_result(ScrollBatch *b, int s, int f, ScrollDynDamage *out);   /* synchronising */
const ScrollDynDamage *scroll_batch_dyn_locate_device(ScrollBatch *b, size_t *stream_stride);
int scroll_batch_dyn_damage_map(ScrollBatch *b, int s, int f, uint32_t *dst);             /* mbw*mbh, synchronising */
const uint32_t *scroll_batch_dyn_damage_map_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride);
float scroll_batch_dyn_locate_ms(ScrollBatch *b);   /* with enable_timing; -1 without */
float scroll_batch_dyn_locate_kernel_ms(ScrollBatch *b);   /* the same for k_dyn_damage alone */

/* ---- only the changed MBs of the rect are coded: the per-MB source mask ----
 * (docs/MASTER_DESIGN.md §6).  The rect is a box, and every MB
 * of it is coded from whatever the source holds: where the renderer drew
 * nothing new the coder still spends levels on the difference between a
 * pristine surface and the lossy references.  The mask compares every rect MB
 * of the source with the exact prediction a decoder forms for it
 * (csrc/mask_device.h):
 *     Dy = sum over the MB's 256 luma samples of (src - pred)^2
 *     Dc = the same sum over its 64 + 64 chroma samples (Cb + Cr together)
 * pred: what k_dyn_row subtracts -- full-pel luma, 1/8-pel bilinear chroma,
 * waypoints resolved through their chains (half-pel chains included), at the
 * frame's own rect position (the batch's, scroll_batch_set_dyn_rect_at's or the
 * located one) and scroll_batch_set_offsets' offsets.
 * An MB is changed iff Dy > mb_sse_y || Dc > mb_sse_c; it is kept iff a
 * changed MB of the same rect lies within `grow` MBs of it in both directions
 * (Chebyshev distance, 0..2; grow = 0: the changed MBs themselves).  With
 * apply = 1 every sample of an MB that is not kept is replaced in the source
 * by its prediction: the MB then quantises to all-zero levels, is coded with
 * coded_block_pattern 0, and a decoder shows for it exactly what it shows for
 * a scroll MB.  Kept MBs are not written.  Everything after it (the probe,
 * the pick, the compose, the reconstruction) reads the source and follows.
 *
 *   scroll_batch_dyn_mask(b, nframes, &rule, hip_stream)
 *       frames 0 .. nframes - 1 of every stream.  A dry state pass (nothing of
 *       the batch's state changes), k_dyn_rows into buffers of the mask's own,
 *       then k_dyn_mask_diff, k_dyn_mask_fill, k_dyn_mask_rec.  Asynchronous
 *       on hip_stream (0 = the batch's own), which must be the stream of the
 *       source step before it and of the probe / compose after it.
 *       SCROLL_ERR_CONFIG without a dynamic rect with reference pictures and
 *       with UI hints set; SCROLL_ERR_ARG for nframes outside 0..max_frames,
 *       grow > 2, apply > 1 or a NULL rule.  A refused call writes nothing.
 *       A frame without a dynamic NAL (no rect in it, experiment mode's
 *       waypoint frame) gets SCROLL_DYN_MASK_NOFRAME, zero map entries and an
 *       untouched source.  A second call with the same rule leaves the source
 *       as it is (the MBs it dropped now have D = 0).  Buffers are allocated by
 *       the first call and go with the rect; a batch that never calls it gains
 *       no launch, allocation or changed byte.
 *   the map: per frame w * h entries of two uint32, row by row over the rect's
 *       MBs: { Dy, Dc | kept << 31 } (SCROLL_DYN_MASK_KEPT; Dc < 2^24).
 *   the record: n_changed, n_kept, and sse_drop[Y, Cb, Cr] = the squared
 *       error between the source as it was and the prediction, summed over
 *       the MBs not kept: what the mask gives up, in scroll_batch_dyn_sse's
 *       units (with the reconstruction on, dyn_sse after the mask + sse_drop is
 *       the squared error of the decoded rect against the original source).
 *       Every value is a sum or a count over the stored map: no atomics,
 *       independent of order.
 *   scroll_batch_dyn_mask_result / _mask_map   one frame's record / its map
 *       (2 w h uint32; synchronising; SCROLL_ERR_CONFIG before the first mask,
 *       SCROLL_ERR_ARG outside the last one)
 *   scroll_batch_dyn_mask_device / _mask_map_device   the device arrays,
 *       [stream][frame] records and [stream][frame][h][w][2] uint32 (strides
 *       in bytes); NULL before the first mask
 *   scroll_batch_dyn_mask_ms   with scroll_batch_enable_timing: HIP-event ms of
 *       the last mask's launches; -1 without. */
#define SCROLL_DYN_MASK_OK      0
#define SCROLL_DYN_MASK_NOFRAME 1
#define SCROLL_DYN_MASK_KEPT    0x80000000u   /* bit 31 of a map entry's second word */
typedef struct {
    uint32_t mb_sse_y;             /* an MB changed iff Dy > mb_sse_y ...                     */
    uint32_t mb_sse_c;             /* ... or Dc > mb_sse_c (Cb + Cr together)                */
    uint8_t  grow;                 /* 0..2: keep MBs within this Chebyshev distance of a changed MB */
    uint8_t  apply;                /* 1: overwrite the source of MBs not kept; 0: report only */
    uint8_t  reserved[2];
} ScrollDynMaskRule;               /* 12 bytes */
typedef struct {
    int32_t  status;               /* SCROLL_DYN_MASK_* */
    uint32_t n_changed, n_kept;
    uint32_t reserved;
    uint64_t sse_drop[3];          /* Y, Cb, Cr */
} ScrollDynMask;                   /* 40 bytes */
int scroll_batch_dyn_mask(ScrollBatch *b, int nframes, const ScrollDynMaskRule *rule, void *hip_stream);
int scroll_batch_dyn_mask_result(ScrollBatch *b, int s, int f, ScrollDynMask *out);       /* synchronising */
const ScrollDynMask *scroll_batch_dyn_mask_device(ScrollBatch *b, size_t *stream_stride);
int scroll_batch_dyn_mask_map(ScrollBatch *b, int s, int f, uint32_t *dst);               /* 2*w*h, synchronising */
const uint32_t *scroll_batch_dyn_mask_map_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride);
float scroll_batch_dyn_mask_ms(ScrollBatch *b);     /* with enable_timing; -1 without */
float scroll_batch_dyn_mask_kernel_ms(ScrollBatch *b);     /* the same for k_dyn_mask_diff alone */

/* ---- each frame's scroll offset detected from the surfaces ----
 * The one per-frame input that still comes from the renderer as a hint is the
 * scroll offset.  The device holds both sides of the question -- the surfaces
 * and reference pictures A and B, whose stacked rows R[r] (row r of A for r <
 * ph, row r - ph of B otherwise) are what a scroll at offset o shows: picture
 * row Y displays R[Y + o] -- so the offset is a search over at most ph + 1
 * vertical displacements (csrc/detect_device.h).  Pure integer:
 *   segments   64 columns wide, nseg = ceil(pw / 64) (the last one 16, 32 or
 *              48 wide); used: 0, seg_step, 2 seg_step, ... < nseg (nuse).
 *   signatures sigR[r][c] = the sum of R[r][x] over segment c; sigS[Y][c] =
 *              the sum of the luma rule above over segment c of surface row Y.
 *   window     c0 = clamp(offsets[s][f], 0, ph) is the caller's estimate (the
 *              last known offset, say); lo = max(c0 - radius, 0), hi =
 *              min(c0 + radius, ph); radius >= ph searches every offset.
 *   score(o)   = #{ (Y, used c) : sigS[Y][c] == sigR[Y + o][c] }, Y < ph, out
 *              of n_sig = ph nuse.  Exact agreements are counted, differences
 *              are not summed: the rows the dynamic rect covers do not vote.
 *   choice     off = the candidate largest under (score descending, |o - c0|
 *              ascending, o ascending); second / second_off = the score and
 *              offset of the largest other candidate under the same key (0
 *              and -1 without one).
 *   SCROLL_DET_LOW    score < min_match
 *   SCROLL_DET_FOUND  score >= min_match and score > second
 *   SCROLL_DET_TIED   score >= min_match and score == second: a flat or
 *                     periodic page, the offsets cannot be told apart
 * The tearing of the MB row that straddles A and B and the waypoint chain are
 * not modelled: the locate that follows at the detected offset counts them as
 * damage.  Luma only, vertical full-pel motion only.
 *
 *   scroll_batch_detect_offsets(b, nframes, &surf, &rule, hip_stream)
 *       frames 0 .. nframes - 1 of every stream: the records, the scores and,
 *       with rule.apply = 1, offsets[s][f] = off for FOUND frames only (LOW
 *       and TIED frames and entries from nframes on keep their values), in the
 *       device array scroll_batch_offsets_device, which the locate, the probe
 *       and the compose that follow read.  k_det_refs, k_det_surf,
 *       k_det_score, k_det_pick; it reads no stream state, so it works with
 *       UI hints set and in experiment mode.  Asynchronous on hip_stream (0 =
 *       the batch's own), which must be the stream of the locate, the
 *       conversion and the compose that follow: a tick becomes detect ->
 *       locate -> ..., the estimate left in the offsets by
 *       scroll_batch_set_offsets or by device code.  scroll_batch_set_offsets
 *       copies synchronously on another stream: after a detect with apply,
 *       synchronise hip_stream before calling it.
 *       SCROLL_ERR_CONFIG without a dynamic rect with reference pictures;
 *       SCROLL_ERR_ARG for a NULL rule, nframes outside 0..max_frames,
 *       seg_step 0 or above nseg, apply > 1, cropped = 1, the surface checks
 *       above and more than 2^35 pixels in one call.  A refused call writes
 *       nothing.  Records, scores and both signature arrays (recomputed by
 *       every call) are allocated by the first call and go with the rect; a
 *       batch that never calls it gains no launch, allocation or changed byte.
 *   scroll_batch_detect_result / _scores   one frame's record / its ph + 1
 *       scores: score(o) at index o for lo <= o <= hi, 0xFFFFFFFF elsewhere
 *       (synchronising; SCROLL_ERR_CONFIG before the first detect,
 *       SCROLL_ERR_ARG outside the last one)
 *   scroll_batch_detect_device / _scores_device   the device arrays,
 *       [stream][frame] records and [stream][frame][ph + 1] uint32 (strides in
 *       bytes); NULL before the first detect
 *   scroll_batch_detect_ms / _kernel_ms   with scroll_batch_enable_timing:
 *       HIP-event ms of the last detect's launches / of k_det_surf alone; -1
 *       without. */
#define SCROLL_DET_LOW   0
#define SCROLL_DET_FOUND 1
#define SCROLL_DET_TIED  2
typedef struct {
    int32_t  off, centre;          /* the chosen offset; c0, the clamped estimate */
    uint32_t score, second;
    int32_t  second_off;           /* -1: no other candidate */
    uint32_t n_sig;                /* ph nuse: what score is out of */
    uint16_t lo, hi;               /* the window searched */
    uint16_t status, reserved;     /* SCROLL_DET_* */
} ScrollOffsetFound;               /* 32 bytes */
typedef struct { uint32_t radius, seg_step, min_match, apply; } ScrollDetect;
int scroll_batch_detect_offsets(ScrollBatch *b, int nframes, const ScrollSurfaces *surf,
                                const ScrollDetect *rule, void *hip_stream);
int scroll_batch_detect_result(ScrollBatch *b, int s, int f, ScrollOffsetFound *out);     /* synchronising */
const ScrollOffsetFound *scroll_batch_detect_device(ScrollBatch *b, size_t *stream_stride);
int scroll_batch_detect_scores(ScrollBatch *b, int s, int f, uint32_t *dst);              /* ph + 1, synchronising */
const uint32_t *scroll_batch_detect_scores_device(ScrollBatch *b, size_t *stream_stride, size_t *frame_stride);
float scroll_batch_detect_ms(ScrollBatch *b);          /* with enable_timing; -1 without */
float scroll_batch_detect_kernel_ms(ScrollBatch *b);   /* the same for k_det_surf alone */
float scroll_batch_detect_score_ms(ScrollBatch *b);    /* the same for k_det_score + k_det_pick */

/* Composer-level batch: offsets[i] composed on cs[i], i < n, in
 * order; Composers may repeat.  Output lands in each Composer's buffer before
 * return (equivalent to n composer_write_scroll_frame calls + a flush). */
int composer_batch_write_scroll_frames(Composer *const *cs, const int *offsets, int n,
                                       int flags);
/* Force queued frames of c onto the GPU now (0 or SCROLL_ERR_*). */
int composer_flush(Composer *c);

#ifdef __cplusplus
}
#endif
#endif /* COMPOSER_BATCH_H */
