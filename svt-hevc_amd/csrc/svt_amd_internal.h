/*
 * Internal declarations of the HIP library (not part of the C-ABI).
 * Device memory layout of one picture slot (all planes 8-bit, row pitch a
 * multiple of 256 B, sample (0,0) 128-B aligned so LCU rows are fetched as
 * aligned 64-B segments):
 *
 *   full      (W   x H  ) valid x in [-68 , W+68),  y in [-68, H+68)   PA "inputPaddedPicture"
 *   quarter   (W/2 x H/2) valid pad 32                                  "quarterDecimatedPicture"
 *   sixteenth (W/4 x H/4) valid pad 16                                  "sixteenthDecimatedPicture"
 *   hp_b / hp_h / hp_j    geometry of `full`; AVC-style half-pel planes
 */
#ifndef SVT_AMD_INTERNAL_H
#define SVT_AMD_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/svt_hevc_amd.h"
#include "slot_records.h"

static inline int svt_amd_lcu_count(int w, int h) { return ((w + 63) / 64) * ((h + 63) / 64); }

struct DevPlane {
    uint8_t *origin;   /* device pointer to sample (0,0) */
    int32_t  pitch;    /* bytes per row */
    int32_t  width, height, pad;
    uint8_t *alloc;    /* base of the allocation */
    size_t   alloc_bytes;
    int32_t  lead_rows; /* rows above y = -pad kept as guard */
    int32_t  lead_cols; /* bytes left of x = 0 in each row   */
};

struct DevPicture {
    DevPlane full, quarter, sixteenth, hp_b, hp_h, hp_j;
    SvtAmdMeLcuResult *d_me_out;   /* device buffer, one record per LCU */
    SvtAmdOisLcuResult *d_ois_out; /* device buffer, one record per LCU */
    void *d_me_carry;              /* MeCarry per LCU (me_kernels.hip), 192 B reserved each */
    uint8_t *d_staging;            /* device copy of the raw luma (upload path) */
    size_t   staging_bytes;
    uint8_t *h_staging;            /* pinned host copy of the raw luma (asynchronous upload path), allocated on first use */
    uint8_t *d_pack;               /* compact wire form of this slot's ME + OIS records (svt_amd_*_fetch_compact_async) */
    size_t pack_bytes;
    hipEvent_t ev_ready;           /* recorded after the planes of this slot were built: lanes on other streams wait on it */
    SlotRecords rec;               /* which picture's ME / OIS records the buffers hold and who is ordered behind whom: slot_records.h, through context.hip only */
    uint16_t width, height;
    int      valid;
};

/* kernel-side view */
struct PicView {
    const uint8_t *full, *quarter, *sixteenth, *hp_b, *hp_h, *hp_j;
    int32_t pitch_full, pitch_quarter, pitch_sixteenth;
};

enum { KC_PREP = 0, KC_ME_SEARCH = 1, KC_OIS = 2, KC_COUNT = 3 };

#define SVT_AMD_MAX_BATCH 256

/* one motion-estimation job = one picture (or an LCU range of it) against its references */
struct MeJobDev {
    SvtAmdMeParams P;
    PicView cur, ref0, ref1;
    SvtAmdMeLcuResult *out;
    struct MeCarry *carry;         /* per-LCU hand-over between the HME and the search kernel */
    int32_t lcu_begin, lcu_count;
    unsigned long long *dbg_clock; /* optional: 16 clock stamps per workgroup (phase profile) */
};

/* one open-loop intra search job = one picture */
struct OisJobDev {
    SvtAmdOisParams P;
    const uint8_t *full;           /* padded source luma, sample (0,0) */
    int32_t pitch, lcus_w, nlcu;
    const SvtAmdMeLcuResult *me;   /* ME results of the picture (P/B) */
    SvtAmdOisLcuResult *out;
};

/* where the pack kernels find picture i of a batch (svt_amd_records_pack_batch_async) */
struct PackSrc {
    const uint32_t *me, *ois;      /* the slot's d_me_out / d_ois_out */
};

/* the batched, stream-ordered entries of pa_batch.h: each owns one device allocation of the context (SvtAmdContext.d_batch), what follows the descriptor table
 * in it is the entry's own.  side / chroma: per-region sums; detect / noise: a per-picture reduction; sbo: per-workgroup partials and per-LCU flags; mdc: per-LCU
 * scores and flags; irc: per-workgroup vote totals, per-LCU votes and flags; mdctl: the check record of a bound controls array; scd: nothing */
enum SvtAmdBatchEntry { BATCH_SIDE, BATCH_CHROMA, BATCH_DETECT, BATCH_NOISE, BATCH_SBO, BATCH_MDC, BATCH_IRC, BATCH_MDCTL, BATCH_SCD, BATCH_ENTRIES };

struct SvtAmdContext {
    int device;
    SvtAmdContext *parent;         /* lane (svt_amd_context_fork): shares the parent's picture slots, owns everything else */
    hipStream_t stream;            /* made at the first stream-ordered use: read it through svt_amd_ctx_stream() only */
    int stream_failed;             /* the stream could not be made: svt_amd_synchronize reports it */
    uint16_t max_w, max_h;
    int num_slots;
    DevPicture *slots;
    hipEvent_t ev_begin, ev_end;
    /* per-kernel-class event pairs recorded while the timer is armed */
    int timer_armed;
    struct Stamp { hipEvent_t a, b; int cls; } *stamps;
    int num_stamps, cap_stamps;
    SvtAmdMeLcuResult *d_me_scratch; /* host-supplied ME results for svt_amd_ois_picture */
    void *d_prep_jobs;             /* device array of SVT_AMD_MAX_BATCH prep descriptors (128 B each reserved) */
    OisJobDev *d_ois_jobs;         /* device array of SVT_AMD_MAX_BATCH OIS job descriptors */
    MeJobDev *d_jobs;              /* device array of SVT_AMD_MAX_BATCH job descriptors */
    unsigned long long *d_dbg;     /* phase-profile buffer (svt_amd_debug_me_phase_profile) */
    size_t dbg_slots;
    void *d_cabac_cost;            /* this context's copy of the caller's CabacCost_t (rate_device.h) */
    uint8_t *d_leaf_scratch;       /* staging of the one-unit host-pointer forms (svt_amd_ctx_scratch) */
    size_t leaf_scratch_bytes;
    /* front-end pipeline (svt_amd_frontend_submit / _wait): pinned result buffers + completion event of this lane */
    SvtAmdMeLcuResult *h_me;
    SvtAmdOisLcuResult *h_ois;
    hipEvent_t ev_done;
    int frontend_busy;
    hipEvent_t ev_user[8];         /* svt_amd_lane_event_record / _wait */
    uint8_t *h_desc_ring;          /* pinned ring of launch descriptors (svt_amd_upload_descriptors) */
    hipEvent_t ev_desc[8];
    int desc_next;
    /* Completion markers of this lane's ME / OIS launches and of its kernels that read a slot's records in place (slot_mark_lend): one record per launch, lent to
     * every slot the launch wrote.
     * INVARIANT: an entry is only ever re-recorded by this lane, later in this lane's stream order.  A waiter holding a reference from before the ring came
     * round (16 launches ago) therefore waits for a LATER point of the stream that wrote its records: longer than needed, never too little.  The ring lives
     * as long as the lane: svt_amd_context_destroy clears every slot reference to it, of all three kinds, behind the lane's synchronisation, before it destroys the events. */
    hipEvent_t ev_launch[16];
    int launch_next;
    unsigned long long mark_records, mark_waits; /* svt_amd_debug_launch_markers */
    void *d_pack_src;              /* device table of the pack kernels' per-picture sources (svt_amd_records_pack_batch_async) */
    void *d_batch[BATCH_ENTRIES];  /* per batched entry: its descriptor table + the scratch its kernels accumulate into, allocated at its first call (svt_amd_batch_begin) */
    void *d_tmvp;                 /* per-LCU intra-area sums of svt_amd_motion_field_launch (tmvp_kernels.hip), allocated at its first call */
    /* multi-GPU exchange (comm.hip): RCCL communicator + the all-gather buffer (one slot per rank) */
    void *comm;
    int comm_world, comm_rank;
    uint8_t *d_xchg;
    size_t xchg_bytes;
};

/* device scratch of at least `bytes` owned by the context (grown on demand, freed by svt_amd_context_destroy);
 * callers serialise per context, as for every other call on one context */
/* launch descriptors (job arrays) reach the device without the copy engines: see context.hip */
int svt_amd_upload_descriptors(SvtAmdContext *ctx, void *d_dst, const void *src, size_t bytes);
int svt_amd_ctx_scratch(SvtAmdContext *ctx, size_t bytes, uint8_t **out);
/* context.hip: the device's view of a range inside a svt_amd_host_register'ed buffer, or nullptr */
const void *svt_amd_registered_device_ptr(const void *h_ptr, size_t bytes);

/* context.hip: what a consumer of the records resident in a slot goes through, in this order.  The mode-decision call (md_picture.hip) calls all three itself;
 * the batched readers (source-based operations, mode-decision configuration, initial rate control) go through the first two by way of
 * svt_amd_batch_slot_records and svt_amd_batch_bind_records (pa_batch.h) and leave no read mark.
 * svt_amd_slot_records: the device pointer of the slot's ME (which == 0) / OIS (which == 1) records, or nullptr unless the slot is in range, holds a picture of
 * w x h and complete records of it.  It sets no error text: the caller refuses in its own words.
 * svt_amd_records_wait: the stream of `ctx` orders itself behind the launch that wrote them (no wait where that ran on this very lane, or where there is nothing
 * to wait for).  A batched consumer passes `seen` (room for `cap` events) / `nseen`, zeroed once per call: one wait per distinct producing launch.
 * svt_amd_records_read_mark: behind the kernel that read them in place - the next ME / OIS launch INTO the slot from another lane orders itself behind it. */
const void *svt_amd_slot_records(SvtAmdContext *root, int slot, int which, int w, int h);
int svt_amd_records_wait(SvtAmdContext *ctx, DevPicture *s, int which, hipEvent_t *seen, int *nseen, int cap);
int svt_amd_records_read_mark(SvtAmdContext *ctx, SvtAmdContext *root, int slot);

void svt_amd_set_error(const char *fmt, ...);

/* mdctl_kernels.hip: queues the check kernel over a DEVICE array of n SvtAmdMdLcu records on the context's stream and the copy of its record to `h_out`
 * (page-locked); the caller synchronises.  depth_mode: SvtAmdMdPicture.depth_mode; inter: a P / B call (md_lcu_supported is applied) */
int svt_amd_mdctl_check_async(SvtAmdContext *ctx, const SvtAmdMdLcu *d_lcus, int n, int depth_mode, int inter, SvtAmdMdCtlCheck *h_out);

/* The context's stream.  A context holds none until its first stream-ordered use (a launch, an asynchronous copy, an event
 * record or wait, a timer): one that only allocates, pins host memory, copies blocking and forks lanes - the root of a host that
 * does all its work on lanes - never takes a hardware queue from them (context.hip, above svt_amd_runtime_env_defaults). */
hipStream_t svt_amd_ctx_stream(SvtAmdContext *ctx);
static inline bool svt_amd_ctx_has_stream(const SvtAmdContext *ctx) { return ctx->stream != nullptr; }
/* waits for whatever the context has queued; a context without a stream has queued nothing (one whose stream could not be made has
 * queued on the null stream) */
static inline hipError_t svt_amd_ctx_sync(SvtAmdContext *ctx)
{
    return ctx->stream || ctx->stream_failed ? hipStreamSynchronize(ctx->stream) : hipSuccess;
}
#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            svt_amd_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),       \
                              __FILE__, __LINE__);                                         \
            return SVT_AMD_ERR_DEVICE;                                                     \
        }                                                                                  \
    } while (0)

/* stamps a kernel class duration when the timer is armed */
int svt_amd_stamp_begin(SvtAmdContext *ctx, int cls);
int svt_amd_stamp_end(SvtAmdContext *ctx);

/* kernel launchers (prep_kernels.hip / me_kernels.hip) */
int svt_amd_launch_prep(SvtAmdContext *ctx, DevPicture *pic, const uint8_t *d_luma, uint32_t stride);
int svt_amd_launch_prep_batch(SvtAmdContext *ctx, DevPicture *const *pics, const uint8_t *const *d_luma, uint32_t stride,
                              int n);
int svt_amd_launch_me_batch(SvtAmdContext *ctx, const MeJobDev *host_jobs, int njobs, int max_lcus);
int svt_amd_me_kernel_occupancy(const SvtAmdMeParams *p, int phase, int *workgroups_per_cu, int *private_bytes);
int svt_amd_launch_zz_sad(SvtAmdContext *ctx, const DevPicture *cur, const DevPicture *prev, SvtAmdZzLcu *d_out);
int svt_amd_launch_ois_batch(SvtAmdContext *ctx, const struct OisJobDev *host_jobs, int njobs, int max_lcus);

static inline PicView make_view(const DevPicture *p)
{
    PicView v;
    v.full = p->full.origin;
    v.quarter = p->quarter.origin;
    v.sixteenth = p->sixteenth.origin;
    v.hp_b = p->hp_b.origin;
    v.hp_h = p->hp_h.origin;
    v.hp_j = p->hp_j.origin;
    v.pitch_full = p->full.pitch;
    v.pitch_quarter = p->quarter.pitch;
    v.pitch_sixteenth = p->sixteenth.pitch;
    return v;
}

#endif
