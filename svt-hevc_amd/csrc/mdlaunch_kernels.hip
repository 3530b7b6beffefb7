/*
 * mdlaunch_kernels.hip - what svt_amd_md_encode_picture_launch (md_picture.hip; include/svt_hevc_amd.h "Device-resident mode decision") queues in
 * front of the mode-decision kernel in place of the blocking call's host copies: every input reaches the picture object's device state by a LAUNCH, so the entry
 * neither copies from host memory nor waits, and a second launch queued on the same object before the first has run finds the first one's inputs untouched.
 *   k_md_source<T>  grid (rows / 4 capped, 3 planes), a wave per row: the caller's DEVICE source planes into the object's own planes at the object's pitch - 16 bytes
 *                   a lane where a row allows it, dwords otherwise and in a row's tail (md_source_logic.h) - and for T = uint16_t the 8-MSB view the mode decision
 *                   reads, in the same pass (the blocking call: hipMemcpy2DAsync + k_msb_view).  A copy and no read in place: the object's planes have 64 bytes of
 *                   slack behind them, a caller's allocation promises none.
 *   k_md_stage      grid (1): the picture controls, the inter controls, the rate tables and the kernel's descriptor arrive BY VALUE in the kernel-argument block
 *                   - captured when the launch is queued - and are stored into the object's device records, a dword a lane.
 *   k_md_gate       grid (1), a wave: reads the check record k_mdctl_check left on the device and writes BOTH ticket counters - 0 for a controls array the
 *                   blocking call's host loop accepts, the LCU count otherwise: k_md_picture and k_encode_picture return on their first ticket and no LCU of a
 *                   malformed leaf list is read - and the caller's status record.
 * Bound: k_md_source by HBM (each byte read once, written once; 10 bit: + half a byte of view a byte); the other two by launch latency.
 */
#include "svt_amd_internal.h"
#include "mdlaunch.h"
#include <string.h>
#define MDSRC_FN __host__ __device__ __forceinline__
#include "md_source_logic.h"

#define MDL_SOURCE_MAX_GROUPS 1024

template <typename T>
__global__ __launch_bounds__(256) void k_md_source(MdSourcePlanes S)
{
    const int p = (int)blockIdx.y, c = p ? 1 : 0;
    const uint32_t row_bytes = (S.width >> c) * (uint32_t)sizeof(T), rows = S.height >> c;
    const uint8_t *src = (const uint8_t *)(p == 0 ? S.src[0] : p == 1 ? S.src[1] : S.src[2]);
    uint8_t *dst = (uint8_t *)(p == 0 ? S.dst[0] : p == 1 ? S.dst[1] : S.dst[2]);
    uint8_t *view = p == 0 ? S.view[0] : p == 1 ? S.view[1] : S.view[2];
    const size_t sp = (size_t)S.src_pitch[c] * sizeof(T), dp = (size_t)S.dst_pitch[c] * sizeof(T), vp = S.dst_pitch[c];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (uint32_t y = blockIdx.x * 4 + wave; y < rows; y += gridDim.x * 4) {
        const uint8_t *s = src + y * sp;
        uint8_t *d = dst + y * dp, *v = sizeof(T) == 2 ? view + y * vp : nullptr;
        const MdSrcRow r = mdsrc_row((uintptr_t)s, (uintptr_t)d, (uintptr_t)v, row_bytes);
        for (uint32_t i = lane; i < r.items; i += 64)
            mdsrc_item(s, d, v, r, i, (int)sizeof(T));
    }
}

/* the kernel-argument block of k_md_stage: up to four records, back to back as dwords */
struct MdStagePack {
    uint32_t *dst[MDL_STAGE_PARTS];
    uint32_t words[MDL_STAGE_PARTS];
    uint32_t payload[MDL_STAGE_WORDS];
};
static_assert(sizeof(MdStagePack) <= 4096, "one launch's argument block");

/* The pack is read through the kernel-argument segment's own address (the pack is the kernel's only argument: it starts at offset 0): indexed by the lane as a
 * by-value parameter it would be copied to the private segment first. */
__global__ __launch_bounds__(256) void k_md_stage(MdStagePack pack_by_value)
{
    typedef const __attribute__((address_space(4))) MdStagePack *PackPtr;
    const PackPtr K = (PackPtr)__builtin_amdgcn_kernarg_segment_ptr();
    uint32_t first = 0;
#pragma unroll
    for (int k = 0; k < MDL_STAGE_PARTS; k++) {
        const uint32_t n = K->words[k];
        uint32_t *dst = K->dst[k];
        for (uint32_t i = threadIdx.x; i < n; i += 256)
            dst[i] = K->payload[first + i];
        first += n;
    }
}

__global__ __launch_bounds__(64) void k_md_gate(const SvtAmdMdCtlCheck *__restrict__ check, unsigned *ticket_md, unsigned *ticket_ep, unsigned closed,
                                                SvtAmdMdLaunchStatus *status)
{
    const uint32_t t = threadIdx.x;
    const bool refused = check->first_bad != 0xFFFFFFFFu;
    if (t == 0)
        *ticket_md = refused ? closed : 0u;
    if (t == 1)
        *ticket_ep = refused ? closed : 0u;
    if (status) {
        static_assert(sizeof(SvtAmdMdCtlCheck) == 88 && sizeof(SvtAmdMdLaunchStatus) == 96, "status record");
        if (t < sizeof(SvtAmdMdCtlCheck) / 4)
            ((uint32_t *)&status->check)[t] = ((const uint32_t *)check)[t];
        if (t == 32)
            status->refused = refused ? 1u : 0u;
        if (t == 33)
            status->pad = 0u;
    }
}

/* ---------------------------------------------------------------- host side ---------------------------------------------------------------- */

int svt_amd_mdlaunch_source(SvtAmdContext *ctx, const MdSourcePlanes *S, int bps)
{
    const unsigned groups = (S->height + 3) / 4 < MDL_SOURCE_MAX_GROUPS ? (S->height + 3) / 4 : MDL_SOURCE_MAX_GROUPS;
    if (bps == 2)
        hipLaunchKernelGGL(k_md_source<uint16_t>, dim3(groups, 3), dim3(256), 0, svt_amd_ctx_stream(ctx), *S);
    else
        hipLaunchKernelGGL(k_md_source<uint8_t>, dim3(groups, 3), dim3(256), 0, svt_amd_ctx_stream(ctx), *S);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}

int svt_amd_mdlaunch_stage(SvtAmdContext *ctx, const MdStagePart *parts, int n)
{
    hipStream_t st = svt_amd_ctx_stream(ctx);
    static thread_local MdStagePack pack;
    int k = 0;
    while (k < n) { /* as many records as fit one argument block a launch */
        memset(&pack, 0, sizeof(pack));
        uint32_t used = 0;
        int slot = 0;
        for (; k < n && slot < MDL_STAGE_PARTS; k++, slot++) {
            const uint32_t words = (uint32_t)(parts[k].bytes / 4);
            if (parts[k].bytes % 4 || words > MDL_STAGE_WORDS || ((uintptr_t)parts[k].d_dst & 3)) {
                svt_amd_set_error("svt_amd_md_encode_picture_launch: a staged record of %zu bytes", parts[k].bytes);
                return SVT_AMD_ERR_BAD_PARAM;
            }
            if (used + words > MDL_STAGE_WORDS)
                break;
            pack.dst[slot] = (uint32_t *)parts[k].d_dst, pack.words[slot] = words;
            memcpy(pack.payload + used, parts[k].src, parts[k].bytes);
            used += words;
        }
        hipLaunchKernelGGL(k_md_stage, dim3(1), dim3(256), 0, st, pack);
        HIP_TRY(hipGetLastError());
    }
    return SVT_AMD_OK;
}

int svt_amd_mdlaunch_gate(SvtAmdContext *ctx, const SvtAmdMdCtlCheck *d_check, unsigned *d_ticket_md, unsigned *d_ticket_ep, unsigned closed, SvtAmdMdLaunchStatus *d_status)
{
    hipLaunchKernelGGL(k_md_gate, dim3(1), dim3(64), 0, svt_amd_ctx_stream(ctx), d_check, d_ticket_md, d_ticket_ep, closed, d_status);
    HIP_TRY(hipGetLastError());
    return SVT_AMD_OK;
}
