/* mdlaunch.h - what md_picture.hip:svt_amd_md_encode_picture_launch calls in mdlaunch_kernels.hip and mdctl_kernels.hip (not part of the C-ABI).  Each of them
 * queues on the context's stream and returns: no copy from or to host memory, no wait. */
#ifndef SVT_AMD_MDLAUNCH_H
#define SVT_AMD_MDLAUNCH_H
#include "svt_amd_internal.h"

/* k_md_source: three DEVICE planes of a width x height picture (chroma half of both) at the caller's pitches into the object's planes; pitches in samples.
 * view: the 8-MSB views of 16-bit planes, at dst_pitch BYTES a row (bps == 1: unused) */
struct MdSourcePlanes {
    const void *src[3];
    void *dst[3];
    uint8_t *view[3];
    uint32_t src_pitch[2], dst_pitch[2];
    uint32_t width, height;
};
int svt_amd_mdlaunch_source(SvtAmdContext *ctx, const MdSourcePlanes *planes, int bps);

/* k_md_stage: HOST records, read before the call returns, into DEVICE records (4-byte aligned, sizes multiples of 4): they travel in the kernel-argument block */
#define MDL_STAGE_PARTS 4
#define MDL_STAGE_WORDS 960
struct MdStagePart {
    void *d_dst;
    const void *src;
    size_t bytes;
};
int svt_amd_mdlaunch_stage(SvtAmdContext *ctx, const MdStagePart *parts, int n);

/* mdctl_kernels.hip: svt_amd_mdctl_check_async without the copy - the record stays in the context's device scratch, *d_out points at it.  Valid until the next check
 * queued on the context, in stream order */
int svt_amd_mdctl_check_device(SvtAmdContext *ctx, const SvtAmdMdLcu *d_lcus, int n, int depth_mode, int inter, const SvtAmdMdCtlCheck **d_out);

/* k_md_gate: behind that check - both ticket counters 0 (first_bad == 0xFFFFFFFF) or `closed`, and the status record (or NULL) */
int svt_amd_mdlaunch_gate(SvtAmdContext *ctx, const SvtAmdMdCtlCheck *d_check, unsigned *d_ticket_md, unsigned *d_ticket_ep, unsigned closed, SvtAmdMdLaunchStatus *d_status);

#endif
