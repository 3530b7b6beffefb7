/*
 * pa_batch.h - the host half the batched, stream-ordered entries share (side_kernels.hip, where the functions live, detect_kernels.hip, noise_kernels.hip,
 * sbo_kernels.hip, mdc_kernels.hip, irc_kernels.hip, mdctl_kernels.hip).  A launcher reads top to bottom: check (svt_amd_batch_header; the
 * batch's size from svt_amd_batch_slot per job where the jobs name picture slots, from svt_amd_batch_geometry where it is an argument; svt_amd_batch_slot_records
 * for a job that reads the ME / OIS records resident in a slot; its own checks - all before the device is touched), svt_amd_batch_begin with the entry's
 * SvtAmdBatchEntry, fill its *JobDev records and wait on what they point into (svt_amd_batch_wait_slot for planes, svt_amd_batch_bind_records for records),
 * svt_amd_upload_descriptors, zero what its kernels accumulate into (svt_amd_batch_run), launch, hipGetLastError.  `entry` is the caller's __func__.
 */
#ifndef SVT_AMD_PA_BATCH_H
#define SVT_AMD_PA_BATCH_H
#include "svt_amd_internal.h"

/* refuses a call: sets the error text and returns; SVT_AMD_TRY passes on what a callee returned */
#define SVT_AMD_BAD(...) do { svt_amd_set_error(__VA_ARGS__); return SVT_AMD_ERR_BAD_PARAM; } while (0)
#define SVT_AMD_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

static inline bool svt_amd_regions_ok(int regions_w, int regions_h) { return regions_w >= 1 && regions_h >= 1 && regions_w * regions_h <= 64; }
int svt_amd_batch_header(const char *entry, const SvtAmdContext *ctx, const void *jobs, const void *out, int num_jobs);
int svt_amd_batch_slot(const char *entry, const SvtAmdContext *ctx, int job, int slot, int *w, int *h);
int svt_amd_batch_begin(SvtAmdContext *ctx, SvtAmdBatchEntry which, size_t record_bytes, size_t scratch_bytes, void **d_tab, void **d_scratch);
int svt_amd_batch_wait_slot(SvtAmdContext *ctx, int slot);
bool svt_amd_batch_run(const uint8_t *want, size_t stride, int num_jobs, int *begin, int *end);

/* the size of a batch that takes it as arguments, in samples, LCUs and workgroups of four LCUs; cap_*: of the largest picture the context was made for, which
 * per-LCU scratch is sized by once.  must_fit: a picture of more LCUs than that is refused */
struct SvtAmdBatchGeometry { int w, h, wl, hl, lcus, groups, cap_lcus, cap_groups; };
int svt_amd_batch_geometry(const char *entry, const SvtAmdContext *ctx, int luma_width, int luma_height, int max_lcus, bool must_fit, SvtAmdBatchGeometry *g);

/* the ME / OIS records resident in a slot, read in place by a job of a batch: the check names the kinds the job reads there, the binder is one per call */
enum { BATCH_REC_ME = 1 << SLOT_ME, BATCH_REC_OIS = 1 << SLOT_OIS };
struct SvtAmdRecordsBinder {
    hipEvent_t waited[32]; /* the producing launches this call has ordered itself behind: one wait each, however many slots they wrote */
    int nwaited = 0;
};
int svt_amd_batch_slot_records(const char *entry, SvtAmdContext *ctx, int job, int slot, int kinds, int w, int h);
int svt_amd_batch_bind_records(SvtAmdContext *ctx, SvtAmdRecordsBinder *b, int slot, int kind, const void **records);

/* lcuParams->potentialLogoLcu (Codec/EbSequenceControlSet.c:253-272), shared by detect_kernels.hip and irc_kernels.hip: the map of the resolution class in LCUs,
 * and the rule - the comparisons are the reference's signed ones (lumaWidth - 3 * 64 may be negative) */
__host__ __device__ static inline int svt_amd_logo_cols(int resolution_class) { return resolution_class == 0 ? 3 : resolution_class < 3 ? 7 : 14; }
__host__ __device__ static inline int svt_amd_logo_rows(int resolution_class) { return resolution_class == 0 ? 2 : resolution_class < 3 ? 4 : 8; }
__device__ __forceinline__ bool detect_logo_lcu(int ox, int oy, int width, int height, int cols, int rows)
{
    return ((ox >= width - cols * 64 || ox < cols * 64) && oy < rows * 64) || oy >= height - rows * 64;
}

#endif
