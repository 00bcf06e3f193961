/*
 * nal_ctx.h -- the NalCtx (scroll_device.h) of a planned NAL: the stream's
 * syntax fields (DevStream), the NAL's own (NalDesc, k_plan's state pass) and
 * a waypoint table.  A header of its own because scroll_device.h is also
 * compiled for the CPU (tests/hostsim) without the host interface engine.h.
 */
#ifndef SCROLL_NAL_CTX_H
#define SCROLL_NAL_CTX_H

#include "engine.h"
#include "scroll_device.h"

namespace scroll {

/* NalCtx of scroll NAL d of stream S with the waypoint table (wo, wl, wv) */
__device__ inline NalCtx nal_ctx(const DevStream *S, const NalDesc &d, const int32_t *wo, const int32_t *wl,
                                 const int32_t *wv)
{
    NalCtx c;
    c.w = S->w;
    c.h = S->h;
    c.log2_mfn = S->log2_mfn;
    c.poc_type = S->poc_type;
    c.log2_poc = S->log2_poc;
    c.deblock = S->deblock;
    c.kind = d.kind;
    c.off = d.off;
    c.frame_num = d.frame_num;
    c.nwp = d.nwp;
    c.wp_off = wo;
    c.wp_lt = wl;
    c.wp_valid = wv;
    return c;
}

}  // namespace scroll

#endif
