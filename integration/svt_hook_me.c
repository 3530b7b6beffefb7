/*
 * integration/svt_hook_me.c - the reference-side binding of the batched front-half boundary
 * (motion estimation + open-loop intra search).
 *
 * This is the code a maintainer adds to the reference: it is
 * compiled against the reference headers and linked, with the reference's own
 * objects and -Wl,--wrap=MotionEstimateLcu, into oracle/_ref/hooked/libSvtHevcEnc.so.1 /
 * SvtHevcEncApp_hip.  Every call the reference's MotionEstimationKernel makes to
 * MotionEstimateLcu (Codec/EbMotionEstimationProcess.c:780) is answered from the
 * result of ONE svt_amd_me_picture() call per picture on the MI355X; the
 * reference's CPU motion search is never executed.  OpenLoopIntraSearchLcu (:793) is
 * answered the same way from ONE svt_amd_ois_picture() per picture (--wrap=OpenLoopIntraSearchLcu).
 * There is no fallback: any error from the HIP library aborts the encoder.
 *
 * Contains no reference source.
 */
#include <pthread.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>
#include "EbErrorCodes.h"
#include "EbEncodeContext.h"

#include "EbDefinitions.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbMotionEstimation.h"
#include "EbMotionEstimationContext.h"
#include "EbReferenceObject.h"
#include "EbMotionEstimationProcess.h"
#include "EbModeDecisionProcess.h"
#include "EbModeDecision.h"
#include "EbFullLoop.h"
#include "EbTransforms.h"
#include "EbInterPrediction.h"
#include "EbNeighborArrays.h"
#include "EbIntraPrediction.h"
#include "EbAvailability.h"
#include "EbEncDecProcess.h"
#include "EbCodingUnit.h"
#include "EbTransformUnit.h"
#include "EbCabacContextModel.h"
#include "EbSystemResourceManager.h"
#include "EbUnPackProcess.h"
#include "EbPackUnPack_C.h"

#include "../include/svt_hevc_amd.h"
#include "svt_hook_internal.h"

#define NSLOTS 48   /* device picture slots, keyed by pictureNumber % NSLOTS */
#define NLANES_MAX 8
static int g_nlanes = NLANES_MAX; /* front-end lanes = pictures whose ME / OIS results are in flight or being served (SVT_HOOK_FRONT_LANES=<1..8>).  A lane is a stream is a hardware queue,
                          * and the device schedules only so many at once (svt_hook_encdec.c: ep_lanes): 4 serve > 1000 pictures/s (a picture holds its lane 4 ms) - what the closed-loop
                          * configuration of bench.py sets; 8 without the switch */
#define NLANES g_nlanes

/*
 * Front half, pipelined: a picture's first MotionEstimateLcu / OpenLoopIntraSearchLcu call claims a LANE (its own HIP stream
 * and pinned result buffers, include/svt_hevc_amd.h "Front-end pipeline"), queues upload -> planes -> ME -> OIS -> result copies
 * on it and only then waits for that lane's completion event; threads of other pictures run their own lanes meanwhile, so copies
 * and kernels of neighbouring pictures overlap and nobody waits under the table lock.  A lane is released when every LCU of its
 * picture has been served (both loops of EbMotionEstimationProcess.c:706-820), which is what sizes the table safely.
 */
typedef struct {
    SvtAmdContext *lane;
    uint64_t pic;
    int state;                       /* 0 free, 1 submitted */
    unsigned gen;                    /* claims so far: tells a thread's cached entry from a re-used lane */
    const SvtAmdMeCuResult *me;      /* pinned, COMPACT records (include/svt_hevc_amd.h), valid while state == 1 */
    const uint8_t *ois;
    int ois_nc;                      /* candidates per CU in the compact OIS records */
    unsigned me_left, ois_left;      /* LCUs still to serve (atomics) */
    SvtAmdOisParams oisp;
    double t_submit;                 /* timeline of the lane (report only) */
    int timed;
} FrontEntry;

/* front-half timeline, printed by the report: where a picture's time on a lane goes */
static double g_t_submit_call, g_t_device, g_t_lane_held, g_t_lane_wait;
#define TL_N 24
static double g_tl0, g_tl_submit[TL_N], g_tl_ready[TL_N], g_tl_released[TL_N]; /* first pictures, seconds since the first call */
static unsigned long g_n_lane_wait, g_n_timed;
static double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;
static pthread_mutex_t g_front_lock = PTHREAD_MUTEX_INITIALIZER; /* entry table + slot table */
static pthread_cond_t g_front_cv = PTHREAD_COND_INITIALIZER;
static SvtAmdContext *g_ctx;
static FrontEntry g_front[NLANES_MAX];
static uint64_t g_slot_pic[NSLOTS];
static unsigned long g_ois_pictures, g_ois_lcus;
static uint32_t g_nlcu;
static unsigned long g_pictures, g_lcus;
static int g_verbose; /* SVT_HOOK_VERBOSE=1: one stderr line per picture handled on the device */
/* calls a binding handed back to the reference function (switch off, or outside what the binding covers) */
/* The counters sit on the mode decision's hottest calls (millions per second over all EncDec threads): one block per thread,
 * summed by the report - a shared counter would bounce its cache line between the sockets on every call. */
enum { CPU_EncodePassInterPrediction, CPU_EncodePassInterPrediction16bit, CPU_Inter2Nx2NPuPredictionHevc, CPU_Intra4x4IntraPredictionCl, CPU_IntraPredictionCl, CPU_IntraPredictionOl, CPU_SaoGenerationDecision, CPU_SaoGenerationDecision16bit, CPU_COUNTERS };
typedef struct HookCounters {
    unsigned long v[CPU_COUNTERS];
    struct HookCounters *next;
    char pad[64];
} HookCounters;
static __thread HookCounters *t_counters;
static HookCounters *g_counters;
static pthread_mutex_t g_counters_lock = PTHREAD_MUTEX_INITIALIZER;
static HookCounters *counters_of_thread(void)
{
    HookCounters *c = (HookCounters *)calloc(1, sizeof(*c)); /* lives until exit: the report reads it after the thread is gone */
    if (!c)
        abort();
    svt_hook_lock(&g_counters_lock);
    c->next = g_counters, g_counters = c;
    svt_hook_unlock(&g_counters_lock);
    return t_counters = c;
}
#define COUNT_CPU(name) (++(t_counters ? t_counters : counters_of_thread())->v[CPU_##name])
static unsigned long counter_sum(int i)
{
    unsigned long n = 0;
    svt_hook_lock(&g_counters_lock);
    for (const HookCounters *c = g_counters; c; c = c->next)
        n += c->v[i];
    svt_hook_unlock(&g_counters_lock);
    return n;
}
static void hook_report(void);
static int ensure_context(uint16_t lumaWidth, uint16_t lumaHeight);
static void pin_deferred(void);

/* SVT_HOOK_TIMELINE (svt_hook_internal.h) */
#define TL_MAX 65536
static struct TlEvent { char kind[12]; unsigned long long picture; int a, b; double t0, t1; } *g_tl;
static int g_tl_n, g_tl_state;
double svt_hook_now(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
void svt_hook_timeline(const char *kind, unsigned long long picture, int a, int b, double t_begin, double t_end)
{
    if (g_tl_state == 0) {
        int on = getenv("SVT_HOOK_TIMELINE") != NULL, expect = 0;
        struct TlEvent *buf = on ? (struct TlEvent *)calloc(TL_MAX, sizeof(*buf)) : NULL;
        if (buf && __atomic_compare_exchange_n(&g_tl, &(struct TlEvent *){NULL}, buf, 0, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE))
            __atomic_store_n(&g_tl_state, 1, __ATOMIC_RELEASE);
        else {
            free(buf);
            __atomic_compare_exchange_n(&g_tl_state, &expect, on ? 1 : -1, 0, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE);
        }
    }
    if (g_tl_state < 0 || !g_tl)
        return;
    const int i = __atomic_fetch_add(&g_tl_n, 1, __ATOMIC_RELAXED);
    if (i >= TL_MAX)
        return;
    struct TlEvent *e = &g_tl[i];
    strncpy(e->kind, kind, sizeof(e->kind) - 1);
    e->picture = picture, e->a = a, e->b = b, e->t0 = t_begin, e->t1 = t_end;
}
int svt_hook_timeline_enabled(void)
{
    static int on = -1;
    if (on < 0)
        on = getenv("SVT_HOOK_TIMELINE") != NULL;
    return on;
}
static void timeline_write(void)
{
    const char *path = getenv("SVT_HOOK_TIMELINE");
    if (!path || !g_tl)
        return;
    FILE *f = fopen(path, "w");
    if (!f)
        return;
    const int n = g_tl_n < TL_MAX ? g_tl_n : TL_MAX;
    double t0 = 1e300;
    for (int i = 0; i < n; i++)
        t0 = g_tl[i].t0 < t0 ? g_tl[i].t0 : t0;
    for (int i = 0; i < n; i++)
        fprintf(f, "%s %llu %d %d %.3f %.3f\n", g_tl[i].kind, g_tl[i].picture, g_tl[i].a, g_tl[i].b, 1e3 * (g_tl[i].t0 - t0), 1e3 * (g_tl[i].t1 - t0));
    fclose(f);
}

/* The reference's error model (SURVEY 8b "Errors"): failures at EbInitEncoder time come back as EB_ERRORTYPE
 * (EB_ErrorInsufficientResources from the object constructors, Codec/EbEncHandle.c:689 ff.); failures inside the running pipeline go
 * to the application through appCallbackPtr->ErrorHandler (Codec/EbErrorHandling.h:15 CHECK_REPORT_ERROR: the handler posts an output
 * packet whose nFlags is the error code, EbH265GetPacket hands it over as EB_ErrorMax, and the reporting thread stops for good).  A HIP
 * failure follows the same two routes: never abort() in a host that loaded the library (ffmpeg, gstreamer). */
static EbCallback_t *g_app_cb; /* encodeContextPtr->appCallbackPtr, noted by the first bound call of the running pipeline */
void svt_hook_note_callback(const SequenceControlSet_t *scs)
{
    if (!__atomic_load_n(&g_app_cb, __ATOMIC_RELAXED) && scs && scs->encodeContextPtr)
        __atomic_store_n(&g_app_cb, scs->encodeContextPtr->appCallbackPtr, __ATOMIC_RELEASE);
}
/* what the calling thread holds (see svt_hook_internal.h) */
#define HELD_MAX 8
static __thread pthread_mutex_t *t_held[HELD_MAX];
static __thread int t_nheld;
static __thread int t_kernel_thread; /* the thread runs inside kernel_thread() below: counted in g_live_threads */
void svt_hook_lock(pthread_mutex_t *m)
{
    pthread_mutex_lock(m);
    if (t_nheld < HELD_MAX)
        t_held[t_nheld++] = m;
}
void svt_hook_unlock(pthread_mutex_t *m)
{
    for (int i = t_nheld - 1; i >= 0; i--)
        if (t_held[i] == m) {
            for (int k = i; k + 1 < t_nheld; k++)
                t_held[k] = t_held[k + 1];
            t_nheld--;
            break;
        }
    pthread_mutex_unlock(m);
}
static int g_failed, g_reported, g_context_failed; /* reset when the last kernel thread has gone (hook_teardown): the next encoder of the process starts clean */
int svt_hook_failed(void) { return __atomic_load_n(&g_failed, __ATOMIC_ACQUIRE); }
static void hook_teardown(void);
static int g_live_threads;
static void die(const char *what)
{
    fprintf(stderr, "svt_hook_me: %s: %s\n", what, svt_amd_last_error());
    EbCallback_t *cb = __atomic_load_n(&g_app_cb, __ATOMIC_ACQUIRE);
    if (cb && cb->ErrorHandler && !getenv("SVT_HOOK_ABORT_ON_ERROR")) {
        __atomic_store_n(&g_failed, 1, __ATOMIC_RELEASE); /* from here on every binding hands its call to the reference code */
        while (t_nheld > 0) /* nothing this thread holds may outlive it: locks (innermost first) ... */
            pthread_mutex_unlock(t_held[--t_nheld]);
        svt_hook_encdec_thread_exit(); /* ... and its device lane */
        if (!__atomic_exchange_n(&g_reported, 1, __ATOMIC_ACQ_REL)) /* one error packet; every failing thread stops */
            cb->ErrorHandler(cb->handle, EB_ENC_ME_ERROR1 + 0x80); /* no message of the application's table: it prints "Error: Others!" */
        if (t_kernel_thread) { /* the thread leaves without returning through kernel_thread(): its count goes here */
            t_kernel_thread = 0;
            if (__atomic_sub_fetch(&g_live_threads, 1, __ATOMIC_ACQ_REL) == 0)
                hook_teardown();
        }
        pthread_exit(NULL); /* the reference spins in `while(1);` after the handler (and EbDeinitEncoder then never joins that thread); leaving
                             * the thread instead lets the application shut the encoder down after it has seen the error packet */
    }
    abort(); /* no pipeline to report to (stand-alone harness use) */
}
void svt_hook_die(const char *what) { die(what); }
const char *svt_hook_cfg(const char *name)
{
    static const struct { const char *name, *value; } defaults[] = {{"SVT_HOOK_MD", "pb"}, {"SVT_HOOK_PCS_POOL", "16"}, {"SVT_HOOK_EP_LANES", "12"}, {"SVT_HOOK_FRONT_LANES", "4"}};
    const char *v = getenv(name);
    if (v)
        return (!v[0] || !strcmp(v, "0") || !strcmp(v, "off")) ? NULL : v;
    for (size_t i = 0; i < sizeof(defaults) / sizeof(defaults[0]); i++)
        if (!strcmp(name, defaults[i].name))
            return defaults[i].value;
    return NULL;
}

SvtAmdContext *svt_hook_device(uint16_t lumaWidth, uint16_t lumaHeight)
{
    SvtAmdContext *have = __atomic_load_n(&g_ctx, __ATOMIC_ACQUIRE); /* (created once per encoder instance; the per-LCU callers must not queue on a global lock) */
    if (have)
        return have;
    svt_hook_lock(&g_front_lock);
    const int rc = ensure_context(lumaWidth, lumaHeight);
    svt_hook_unlock(&g_front_lock);
    if (rc)
        die("device start-up");
    return g_ctx;
}

/* The rate tables handed to the device are the reference's CabacCost_t, field for field */
_Static_assert(sizeof(CabacCost_t) == sizeof(SvtAmdCabacCost), "CabacCost_t layout");
_Static_assert(offsetof(CabacCost_t, CabacBitsLast) == offsetof(SvtAmdCabacCost, CabacBitsLast), "CabacBitsLast");
_Static_assert(offsetof(CabacCost_t, CabacBitsSig) == offsetof(SvtAmdCabacCost, CabacBitsSig), "CabacBitsSig");
_Static_assert(offsetof(CabacCost_t, CabacBitsG1) == offsetof(SvtAmdCabacCost, CabacBitsG1), "CabacBitsG1");
_Static_assert(offsetof(CabacCost_t, CabacBitsG2) == offsetof(SvtAmdCabacCost, CabacBitsG2), "CabacBitsG2");
_Static_assert(offsetof(CabacCost_t, CabacBitsSigMl) == offsetof(SvtAmdCabacCost, CabacBitsSigMl), "CabacBitsSigMl");
_Static_assert(offsetof(CabacCost_t, CabacBitsG1x) == offsetof(SvtAmdCabacCost, CabacBitsG1x), "CabacBitsG1x");
_Static_assert(offsetof(CabacCost_t, CabacBitsSigV) == offsetof(SvtAmdCabacCost, CabacBitsSigV), "CabacBitsSigV");

/* `padded`: any picture buffer whose luma is the source picture (PA padded copy or the enhanced input).  Called under
 * g_front_lock; queues the upload on `lane` unless the slot already holds (or is already being filled with) the picture. */
static int ensure_uploaded(SvtAmdContext *lane, uint64_t pic, const EbPictureBufferDesc_t *padded)
{
    const int slot = (int)(pic % NSLOTS);
    if (g_slot_pic[slot] != pic + 1) {
        const uint8_t *luma = padded->bufferY + (size_t)padded->originY * padded->strideY + padded->originX;
        if (svt_amd_picture_upload_async(lane, slot, luma, padded->strideY, padded->width, padded->height))
            die("svt_amd_picture_upload_async");
        g_slot_pic[slot] = pic + 1;
    }
    return slot;
}

static void fill_params(SvtAmdMeParams *p, const PictureParentControlSet_t *pcs, const SequenceControlSet_t *scs,
                        const MeContext_t *ctx)
{
    const int nlists = (pcs->sliceType == EB_P_PICTURE) ? 1 : 2;
    memset(p, 0, sizeof(*p));
    p->luma_width = scs->lumaWidth;
    p->luma_height = scs->lumaHeight;
    p->num_lists = (uint8_t)nlists;
    p->temporal_layer_index = pcs->temporalLayerIndex;
    p->ref_pocs_equal = (nlists == 2 && pcs->refPicPocArray[0] == pcs->refPicPocArray[1]);
    p->enable_hme_flag = pcs->enableHmeFlag;
    p->enable_hme_level0 = pcs->enableHmeLevel0Flag;
    p->enable_hme_level1 = pcs->enableHmeLevel1Flag;
    p->enable_hme_level2 = pcs->enableHmeLevel2Flag;
    p->one_quadrant_hme = ctx->oneQuadrantHME;
    p->update_hme_search_center = ctx->updateHmeSearchCenter;
    p->num_hme_regions_w = (uint8_t)ctx->numberHmeSearchRegionInWidth;
    p->num_hme_regions_h = (uint8_t)ctx->numberHmeSearchRegionInHeight;
    p->search_area_width = (uint8_t)ctx->searchAreaWidth;
    p->search_area_height = (uint8_t)ctx->searchAreaHeight;
    p->fractional_search_method = ctx->fractionalSearchMethod;
    p->fractional_search_model = ctx->fractionalSearchModel;
    p->fractional_search_64x64 = ctx->fractionalSearch64x64;
    p->cu8x8_mode = pcs->cu8x8Mode;
    p->cu16x16_mode = pcs->cu16x16Mode;
    p->hme_l0_total_w = ctx->hmeLevel0TotalSearchAreaWidth;
    p->hme_l0_total_h = ctx->hmeLevel0TotalSearchAreaHeight;
    for (int k = 0; k < 2; k++) {
        p->hme_l0_w[k] = ctx->hmeLevel0SearchAreaInWidthArray[k];
        p->hme_l0_h[k] = ctx->hmeLevel0SearchAreaInHeightArray[k];
        p->hme_l1_w[k] = ctx->hmeLevel1SearchAreaInWidthArray[k];
        p->hme_l1_h[k] = ctx->hmeLevel1SearchAreaInHeightArray[k];
        p->hme_l2_w[k] = ctx->hmeLevel2SearchAreaInWidthArray[k];
        p->hme_l2_h[k] = ctx->hmeLevel2SearchAreaInHeightArray[k];
    }
    p->hme_l0_mult_x = (uint16_t)HME_LEVEL_0_SEARCH_AREA_MULTIPLIER_X[pcs->hierarchicalLevels][pcs->temporalLayerIndex];
    p->hme_l0_mult_y = (uint16_t)HME_LEVEL_0_SEARCH_AREA_MULTIPLIER_Y[pcs->hierarchicalLevels][pcs->temporalLayerIndex];
    p->lambda = (uint32_t)ctx->lambda;
    for (int k = 0; k < 12; k++)
        p->mvd_bits[k] = ctx->mvdBitsArray[k];
}

/* The open-loop intra search controls of a picture.  At the picture's first MotionEstimateLcu call only MeContext_t is at hand,
 * so the three MotionEstimationContext_t values are derived as SignalDerivationMeKernelOq does
 * (Codec/EbMotionEstimationProcess.c:356-396); every OpenLoopIntraSearchLcu call checks them against the context it is given. */
static void fill_ois_params(SvtAmdOisParams *p, const PictureParentControlSet_t *pcs, const SequenceControlSet_t *scs)
{
    memset(p, 0, sizeof(*p));
    p->luma_width = scs->lumaWidth;
    p->luma_height = scs->lumaHeight;
    p->slice_is_intra = pcs->sliceType == EB_I_PICTURE;
    p->temporal_layer_index = pcs->temporalLayerIndex;
    p->limit_ois_to_dc_mode = pcs->limitOisToDcModeFlag;
    p->skip_ois_8x8 = pcs->skipOis8x8;
    p->cu8x8_mode = pcs->cu8x8Mode;
    p->ois_kernel_level = pcs->encMode <= ENC_MODE_4 && scs->inputResolution < INPUT_SIZE_4K_RANGE && pcs->temporalLayerIndex == 0;
    if (scs->inputResolution == INPUT_SIZE_4K_RANGE)
        p->ois_th_set = (pcs->encMode <= ENC_MODE_5 && pcs->isUsedAsReferenceFlag == EB_TRUE) ? 2 : 1;
    else
        p->ois_th_set = pcs->encMode <= ENC_MODE_6 ? 2 : 1;
    p->set_best_ois_distortion_to_valid = 0;
}

/* The picture's lane entry: claims a lane and queues the whole front half on first touch; returns with the results complete.
 * `me_ctx` is NULL when the first touch is an OIS call (I pictures never reach MotionEstimateLcu). */
/*
 * SURVEY 8f-3, the source-based-operations input of the mode-decision configuration: CalculateAcEnergy (EbSourceBasedOperationsProcess.c:302) asks
 * ComputeNxMSatdSadLCU (EbPictureOperators.c:232) for the AC energy of the 64x64 and of the four 32x32 of every complete LCU of an I picture (outside
 * low-delay P).  With SVT_HOOK_SBO=1 the device computes all of them in one launch from the luma the front half has just uploaded for the picture's open-loop
 * intra search (svt_amd_picture_ac_energy), while the picture still holds its lane; the reference's calls - which arrive two processes later - are answered
 * from that table.  A table entry is keyed by the address of the picture's first luma sample in the encoder's enhanced-picture buffer: the buffer is handed to
 * a later picture only after this one has left the encoder, and a later I picture in the same buffer replaces the entry before its own calls arrive.
 */
#define SBO_PICTURES 128
typedef struct { const uint8_t *base; uint32_t stride, width, height, lcus_w; uint64_t *energy; size_t capacity; } SboEntry;
static SboEntry g_sbo[SBO_PICTURES];
static pthread_mutex_t g_sbo_lock = PTHREAD_MUTEX_INITIALIZER;
static unsigned long g_sbo_pictures, g_sbo_answers, g_sbo_cpu;
static int sbo_on(void)
{
    static int on = -1;
    if (on < 0)
        on = getenv("SVT_HOOK_SBO") && atoi(getenv("SVT_HOOK_SBO")) > 0;
    return on;
}
static void sbo_note_picture(FrontEntry *e, const PictureParentControlSet_t *pcs, const SequenceControlSet_t *scs)
{
    if (!sbo_on() || pcs->sliceType != EB_I_PICTURE || pcs->predStructure == EB_PRED_LOW_DELAY_P)
        return;
    const EbPictureBufferDesc_t *in = pcs->enhancedPicturePtr;
    const uint8_t *base = in->bufferY + (size_t)in->originY * in->strideY + in->originX;
    const uint32_t n = ((scs->lumaWidth + 63u) / 64u) * ((scs->lumaHeight + 63u) / 64u);
    uint64_t *energy = (uint64_t *)malloc((size_t)n * 5 * sizeof(uint64_t));
    if (!energy || svt_amd_picture_ac_energy(e->lane, (int)(pcs->pictureNumber % NSLOTS), energy))
        die("svt_amd_picture_ac_energy");
    pthread_mutex_lock(&g_sbo_lock);
    SboEntry *t = NULL;
    for (int i = 0; i < SBO_PICTURES && !t; i++)
        if (g_sbo[i].base == base || !g_sbo[i].base)
            t = &g_sbo[i];
    if (!t) { /* more enhanced-picture buffers than entries: the calls of this picture go to the reference code */
        pthread_mutex_unlock(&g_sbo_lock);
        free(energy);
        return;
    }
    free(t->energy);
    t->base = base, t->stride = in->strideY, t->width = scs->lumaWidth, t->height = scs->lumaHeight, t->lcus_w = (scs->lumaWidth + 63u) / 64u, t->energy = energy;
    g_sbo_pictures++;
    pthread_mutex_unlock(&g_sbo_lock);
}
EB_U64 __real_ComputeNxMSatdSadLCU(EB_U8 *src, EB_U32 srcStride, EB_U32 width, EB_U32 height);
EB_U64 __wrap_ComputeNxMSatdSadLCU(EB_U8 *src, EB_U32 srcStride, EB_U32 width, EB_U32 height)
{
    if (sbo_on() && !svt_hook_failed() && width == height && (width == 64 || width == 32)) {
        pthread_mutex_lock(&g_sbo_lock);
        for (int i = 0; i < SBO_PICTURES && g_sbo[i].base; i++) {
            const SboEntry *t = &g_sbo[i];
            if (t->stride != srcStride || src < t->base || (size_t)(src - t->base) >= (size_t)t->stride * t->height)
                continue;
            const uint32_t y = (uint32_t)((size_t)(src - t->base) / t->stride), x = (uint32_t)((size_t)(src - t->base) % t->stride);
            if (x + width > t->width || y + height > t->height || (x & 31) || (y & 31) || (width == 64 && ((x | y) & 63)))
                break;
            const uint64_t *en = t->energy + (size_t)((y >> 6) * t->lcus_w + (x >> 6)) * 5;
            const uint64_t v = width == 64 ? en[0] : en[1 + (((y >> 5) & 1) << 1) + ((x >> 5) & 1)];
            if (v == 100000000ull)
                break; /* an LCU the picture does not cover: never asked for by CalculateAcEnergy */
            g_sbo_answers++;
            pthread_mutex_unlock(&g_sbo_lock);
            return v;
        }
        g_sbo_cpu++;
        pthread_mutex_unlock(&g_sbo_lock);
    }
    return __real_ComputeNxMSatdSadLCU(src, srcStride, width, height);
}

static FrontEntry *front_entry(PictureParentControlSet_t *pcs, const MeContext_t *me_ctx, const EbPictureBufferDesc_t *inputPtr)
{
    static __thread FrontEntry *cached;
    static __thread unsigned cached_gen;
    const uint64_t pic = pcs->pictureNumber;
    FrontEntry *e = cached;
    if (e && __atomic_load_n(&e->state, __ATOMIC_ACQUIRE) == 1 && e->pic == pic && e->gen == cached_gen)
        return e; /* this thread already waited for it */
    SequenceControlSet_t *scs = (SequenceControlSet_t *)pcs->sequenceControlSetWrapperPtr->objectPtr;
    svt_hook_note_callback(scs);
    svt_hook_lock(&g_front_lock);
    if (ensure_context(scs->lumaWidth, scs->lumaHeight)) {
        svt_hook_unlock(&g_front_lock);
        die("device start-up");
    }
    g_nlcu = ((scs->lumaWidth + 63u) / 64u) * ((scs->lumaHeight + 63u) / 64u);
    for (;;) {
        e = NULL;
        FrontEntry *fr = NULL;
        for (int i = 0; i < NLANES; i++) {
            if (g_front[i].state == 1 && g_front[i].pic == pic)
                e = &g_front[i];
            else if (g_front[i].state == 0 && !fr)
                fr = &g_front[i];
        }
        if (e)
            break;
        if (fr) {
            e = fr;
            const double t0 = now_s();
            const int intra = pcs->sliceType == EB_I_PICTURE;
            if (!intra && !me_ctx)
                die("front_entry: OIS before ME on a non-intra picture (unexpected call order)");
            SvtAmdFrontendJob job;
            memset(&job, 0, sizeof(job));
            if (intra) {
                job.cur_slot = ensure_uploaded(e->lane, pic, inputPtr);
            } else {
                const int nlists = (pcs->sliceType == EB_P_PICTURE) ? 1 : 2;
                EbPaReferenceObject_t *cur = (EbPaReferenceObject_t *)pcs->paReferencePictureWrapperPtr->objectPtr;
                job.cur_slot = ensure_uploaded(e->lane, pic, cur->inputPaddedPicturePtr);
                for (int l = 0; l < nlists; l++) {
                    EbPaReferenceObject_t *ro = (EbPaReferenceObject_t *)pcs->refPaPicPtrArray[l]->objectPtr;
                    job.ref_slot[l] = ensure_uploaded(e->lane, pcs->refPicPocArray[l], ro->inputPaddedPicturePtr);
                }
                job.has_me = 1;
                fill_params(&job.me, pcs, scs, me_ctx);
            }
            job.has_ois = 1;
            job.compact = 1; /* the D2H copy is the longest stage of a lane: fetch only what is read below */
            fill_ois_params(&job.ois, pcs, scs);
            if (svt_amd_frontend_submit(e->lane, &job))
                die("svt_amd_frontend_submit");
            e->oisp = job.ois;
            e->ois_nc = svt_amd_ois_compact_candidates(&job.ois);
            e->pic = pic;
            e->me_left = intra ? 0 : g_nlcu;
            e->ois_left = g_nlcu;
            e->me = NULL, e->ois = NULL;
            e->gen++;
            e->t_submit = now_s(), e->timed = 0;
            if (g_tl0 == 0)
                g_tl0 = t0;
            if (pic < TL_N)
                g_tl_submit[pic] = e->t_submit - g_tl0;
            g_t_submit_call += e->t_submit - t0;
            if (!intra)
                g_pictures++;
            g_ois_pictures++;
            if (g_verbose) {
                if (!intra)
                    fprintf(stderr, "svt_hook_me: ME picture %llu on the GPU (%u LCUs)\n", (unsigned long long)pic, g_nlcu);
                fprintf(stderr, "svt_hook_me: OIS picture %llu on the GPU (%u LCUs)\n", (unsigned long long)pic, g_nlcu);
            }
            __atomic_store_n(&e->state, 1, __ATOMIC_RELEASE);
            break;
        }
        {
            const double tw = now_s();
            pthread_cond_wait(&g_front_cv, &g_front_lock); /* every lane is serving an earlier picture */
            g_t_lane_wait += now_s() - tw, g_n_lane_wait++;
        }
    }
    svt_hook_unlock(&g_front_lock);
    /* outside the lock: wait for this lane's completion event (idempotent; any number of threads may wait) */
    const SvtAmdMeLcuResult *me;
    const SvtAmdOisLcuResult *ois;
    if (svt_amd_frontend_wait(e->lane, &me, &ois))
        die("svt_amd_frontend_wait");
    e->me = (const SvtAmdMeCuResult *)me, e->ois = (const uint8_t *)ois;
    const int first_back = !__atomic_exchange_n(&e->timed, 1, __ATOMIC_ACQ_REL);
    if (first_back) { /* first thread back: submit -> results on the host */
        svt_hook_lock(&g_front_lock);
        g_t_device += now_s() - e->t_submit, g_n_timed++;
        if (e->pic < TL_N)
            g_tl_ready[e->pic] = now_s() - g_tl0;
        svt_hook_unlock(&g_front_lock);
    }
    if (first_back)
        sbo_note_picture(e, pcs, scs);
    cached = e;
    cached_gen = e->gen;
    return e;
}

static void front_served(FrontEntry *e, unsigned *counter)
{
    if (__atomic_sub_fetch(counter, 1, __ATOMIC_ACQ_REL) != 0)
        return;
    if (__atomic_load_n(&e->me_left, __ATOMIC_ACQUIRE) || __atomic_load_n(&e->ois_left, __ATOMIC_ACQUIRE))
        return;
    svt_hook_lock(&g_front_lock);
    g_t_lane_held += now_s() - e->t_submit;
    if (e->pic < TL_N)
        g_tl_released[e->pic] = now_s() - g_tl0;
    svt_amd_frontend_release(e->lane);
    __atomic_store_n(&e->state, 0, __ATOMIC_RELEASE);
    pthread_cond_broadcast(&g_front_cv);
    svt_hook_unlock(&g_front_lock);
}

/* SVT_HOOK_FRONT_VERIFY=1: every MotionEstimateLcu / OpenLoopIntraSearchLcu call is answered by the device AND by the reference code, the two answers are compared and
 * counted (the reference's stays).  A proof that does not depend on WHEN anything arrives - what a rate-controlled encode needs, whose bitstream does
 * (tests/test_gpu_e2e_bitstream.py). */
static unsigned long g_me_verified, g_me_mismatch, g_ois_verified, g_ois_mismatch;
static int front_verify(void)
{
    static int on = -1;
    if (on < 0)
        on = getenv("SVT_HOOK_FRONT_VERIFY") != NULL;
    return on;
}
EB_ERRORTYPE __real_MotionEstimateLcu(PictureParentControlSet_t *pcs, EB_U32 lcuIndex, EB_U32 lcuOriginX, EB_U32 lcuOriginY, MeContext_t *ctx,
                                      EbPictureBufferDesc_t *inputPtr);
EB_ERRORTYPE __real_OpenLoopIntraSearchLcu(PictureParentControlSet_t *pcs, EB_U32 lcuIndex, MotionEstimationContext_t *ctx, EbPictureBufferDesc_t *inputPtr);
EB_ERRORTYPE __wrap_MotionEstimateLcu(PictureParentControlSet_t *pcs, EB_U32 lcuIndex, EB_U32 lcuOriginX,
                                      EB_U32 lcuOriginY, MeContext_t *ctx, EbPictureBufferDesc_t *inputPtr)
{
    if (svt_hook_failed()) /* a binding has reported a device failure: the pipeline drains on the reference's own code */
        return __real_MotionEstimateLcu(pcs, lcuIndex, lcuOriginX, lcuOriginY, ctx, inputPtr);
    SequenceControlSet_t *scs = (SequenceControlSet_t *)pcs->sequenceControlSetWrapperPtr->objectPtr;
    FrontEntry *e = front_entry(pcs, ctx, inputPtr);
    const SvtAmdMeCuResult *r = &e->me[(size_t)lcuIndex * SVT_AMD_ME_PU_COUNT];
    for (int pu = 0; pu < SVT_AMD_ME_PU_COUNT; pu++) {
        MeCuResults_t *m = &pcs->meResults[lcuIndex][pu];
        const SvtAmdMeCuResult *s = &r[pu];
        m->xMvL0 = s->x_mv_l0;
        m->yMvL0 = s->y_mv_l0;
        m->xMvL1 = s->x_mv_l1;
        m->yMvL1 = s->y_mv_l1;
        m->totalMeCandidateIndex = s->total_me_candidate_index;
        for (int k = 0; k < s->total_me_candidate_index; k++) {
            m->distortionDirection[k].distortion = s->distortion[k];
            m->distortionDirection[k].direction = s->direction[k];
        }
    }
    if (scs->staticConfig.rateControlMode) { /* EbMotionEstimation.c:4442-4448 */
        pcs->rcMEdistortion[lcuIndex] = 0;
        for (int i = 0; i < 16; i++)
            pcs->rcMEdistortion[lcuIndex] += pcs->meResults[lcuIndex][5 + i].distortionDirection[0].distortion;
    }
    if (front_verify()) { /* SVT_HOOK_FRONT_VERIFY: the reference code answers the same call; its answer stays in the picture, the two are compared */
        MeCuResults_t dev[SVT_AMD_ME_PU_COUNT];
        memcpy(dev, pcs->meResults[lcuIndex], sizeof(dev));
        const EB_U32 rc_dev = scs->staticConfig.rateControlMode ? pcs->rcMEdistortion[lcuIndex] : 0;
        (void)__real_MotionEstimateLcu(pcs, lcuIndex, lcuOriginX, lcuOriginY, ctx, inputPtr);
        int bad = scs->staticConfig.rateControlMode && rc_dev != pcs->rcMEdistortion[lcuIndex];
        for (int pu = 0; pu < SVT_AMD_ME_PU_COUNT && !bad; pu++) {
            const MeCuResults_t *a = &dev[pu], *b = &pcs->meResults[lcuIndex][pu];
            bad = a->xMvL0 != b->xMvL0 || a->yMvL0 != b->yMvL0 || a->totalMeCandidateIndex != b->totalMeCandidateIndex;
            if (pcs->sliceType == EB_B_PICTURE)
                bad = bad || a->xMvL1 != b->xMvL1 || a->yMvL1 != b->yMvL1;
            for (int k = 0; k < b->totalMeCandidateIndex && !bad; k++)
                bad = a->distortionDirection[k].distortion != b->distortionDirection[k].distortion || a->distortionDirection[k].direction != b->distortionDirection[k].direction;
            if (bad && __atomic_load_n(&g_me_mismatch, __ATOMIC_RELAXED) < 4)
                fprintf(stderr, "svt_hook_me: FRONT VERIFY picture %llu lcu %u unit %d: device (%d,%d)/(%d,%d) n %u d0 %u, reference (%d,%d)/(%d,%d) n %u d0 %u\n",
                        (unsigned long long)pcs->pictureNumber, lcuIndex, pu, a->xMvL0, a->yMvL0, a->xMvL1, a->yMvL1, a->totalMeCandidateIndex, a->distortionDirection[0].distortion,
                        b->xMvL0, b->yMvL0, b->xMvL1, b->yMvL1, b->totalMeCandidateIndex, b->distortionDirection[0].distortion);
        }
        __atomic_add_fetch(&g_me_verified, 1, __ATOMIC_RELAXED);
        if (bad)
            __atomic_add_fetch(&g_me_mismatch, 1, __ATOMIC_RELAXED);
    }
    __atomic_add_fetch(&g_lcus, 1, __ATOMIC_RELAXED);
    front_served(e, &e->me_left);
    return EB_ErrorNone;
}

/* Under g_front_lock.  Returns non-zero (with the library's message on stderr) when the device cannot be brought up; the caller maps it
 * to the reference's error model (see die()). */
static int ensure_context(uint16_t lumaWidth, uint16_t lumaHeight)
{
    if (g_ctx)
        return 0;
    if (g_context_failed)
        return 1;
    const char *dev = getenv("SVT_AMD_DEVICE");
    const uint16_t mh = (uint16_t)((lumaHeight + 7) & ~7);
    SvtAmdContext *ctx = NULL;
    const char *step = "svt_amd_context_create";
    /* the encoder keeps up to NLANES + EP_LANES streams busy: a hardware queue each (the library's opt-in).  The setting changes the process
     * environment, so it belongs to EbInitEncoder time only - before the encoder's threads exist (setenv racing another thread's getenv is undefined) and before the
     * process's first HIP call (it has no effect afterwards).  Under SVT_HOOK_LAZY_INIT this function runs on a kernel thread: the environment is left alone and the
     * consequence is said out loud. */
    if (getenv("SVT_HOOK_LAZY_INIT")) {
        if (!getenv("GPU_MAX_HW_QUEUES"))
            fprintf(stderr, "svt_hook_me: SVT_HOOK_LAZY_INIT: GPU_MAX_HW_QUEUES is not set and cannot be set from a worker thread - the lanes' streams share the runtime's "
                            "default of 4 hardware queues (pictures in flight on the device will serialise; set GPU_MAX_HW_QUEUES=24 in the environment)\n");
    } else if (!getenv("SVT_HOOK_KEEP_RUNTIME_ENV")) {
        (void)svt_amd_runtime_env_defaults();
    }
    /* EncDec threads wait 60 - 100 ms for their picture's device call and motion-estimation threads 10 - 20 ms for their picture's lane while the base-layer pictures
     * are decided by host threads on the same logical processors: waiting threads sleep (the library's opt-in; SVT_HOOK_WAIT=spin keeps the runtime's default) */
    if (!(getenv("SVT_HOOK_WAIT") && !strcmp(getenv("SVT_HOOK_WAIT"), "spin")) && svt_amd_host_wait_mode(dev ? atoi(dev) : 0, 1))
        fprintf(stderr, "svt_hook_me: svt_amd_host_wait_mode: %s (host threads will spin in their waits)\n", svt_amd_last_error());
    {
        const char *fl = svt_hook_cfg("SVT_HOOK_FRONT_LANES");
        const int n = fl ? atoi(fl) : 0;
        if (n >= 1 && n <= NLANES_MAX)
            g_nlanes = n;
    }
    int rc = svt_amd_context_create(dev ? atoi(dev) : 0, lumaWidth, mh, NSLOTS, &ctx);
    for (int i = 0; i < NLANES && !rc; i++)
        step = "svt_amd_context_fork", rc = svt_amd_context_fork(ctx, &g_front[i].lane);
    /* pinned buffers and kernel code objects now, not inside the first pictures (EbInitEncoder is outside the encode clock) */
    if (!rc && !getenv("SVT_HOOK_NO_WARMUP")) {
        step = "svt_amd_frontend_warmup", rc = svt_amd_frontend_warmup(ctx);
        for (int i = 0; i < NLANES && !rc; i++)
            rc = svt_amd_frontend_warmup(g_front[i].lane);
    }
    if (rc) {
        fprintf(stderr, "svt_hook_me: %s (device %s): %s\n", step, dev ? dev : "0", svt_amd_last_error());
        for (int i = 0; i < NLANES; i++)
            if (g_front[i].lane)
                svt_amd_context_destroy(g_front[i].lane), g_front[i].lane = NULL;
        if (ctx)
            svt_amd_context_destroy(ctx);
        g_context_failed = 1;
        return 1;
    }
    g_ctx = ctx;
    pin_deferred(); /* picture pools built before the device came up (the reference-picture pool, EbEncHandle.c:889) */
    if (!getenv("SVT_HOOK_LAZY_INIT"))
        svt_hook_encdec_warmup();
    g_nlcu = ((lumaWidth + 63u) / 64u) * ((lumaHeight + 63u) / 64u);
    g_verbose = getenv("SVT_HOOK_VERBOSE") != NULL;
    fprintf(stderr, "svt_hook_me: motion estimation on %s\n", svt_amd_version());
    atexit(hook_report);
    return 0;
}

/* Device start-up belongs to EbInitEncoder, not to the first picture: the picture-analysis reference objects are built there
 * (EbEncHandle.c, EbSystemResourceCtor with this creator), and their descriptor carries the luma size. */
/* (the creator, not EbPaReferenceObjectCtor: the reference calls the constructor from the same translation unit, Codec/EbReferenceObject.c:270,
 * where --wrap cannot reach; the creator is taken by address in EbEncHandle.c:944) */
EB_ERRORTYPE __real_EbPaReferenceObjectCreator(EB_PTR *objectDblPtr, EB_PTR objectInitDataPtr);
EB_ERRORTYPE __wrap_EbPaReferenceObjectCreator(EB_PTR *objectDblPtr, EB_PTR objectInitDataPtr)
{
    const EbPaReferenceObjectDescInitData_t *d = (const EbPaReferenceObjectDescInitData_t *)objectInitDataPtr;
    if (d && !getenv("SVT_HOOK_LAZY_INIT")) {
        svt_hook_lock(&g_front_lock);
        const int rc = ensure_context(d->referencePictureDescInitData.maxWidth, d->referencePictureDescInitData.maxHeight);
        svt_hook_unlock(&g_front_lock);
        if (rc) /* no usable MI355X: EbInitEncoder fails like any other resource the encoder cannot get (EbEncHandle.c EB_NEW chain) */
            return EB_ErrorInsufficientResources;
    }
    return __real_EbPaReferenceObjectCreator(objectDblPtr, objectInitDataPtr);
}

/*
 * Open-loop intra search: every call of OpenLoopIntraSearchLcu (EbMotionEstimationProcess.c:793) is answered from the
 * picture's lane.  For P/B pictures the ME results the search consults are the ones the device produced for this picture
 * (queued on the same stream right before it).
 */
EB_ERRORTYPE __wrap_OpenLoopIntraSearchLcu(PictureParentControlSet_t *pcs, EB_U32 lcuIndex,
                                           MotionEstimationContext_t *ctx, EbPictureBufferDesc_t *inputPtr)
{
    if (svt_hook_failed())
        return __real_OpenLoopIntraSearchLcu(pcs, lcuIndex, ctx, inputPtr);
    FrontEntry *e = front_entry(pcs, NULL, inputPtr);
    if (e->oisp.ois_kernel_level != ctx->oisKernelLevel || e->oisp.ois_th_set != ctx->oisThSet ||
        e->oisp.set_best_ois_distortion_to_valid != ctx->setBestOisDistortionToValid) {
        die("open-loop intra search controls differ from SignalDerivationMeKernelOq's");
    }
    const int nc = e->ois_nc;
    const uint32_t *cand = (const uint32_t *)(e->ois + (size_t)lcuIndex * SVT_AMD_OIS_COMPACT_BYTES(nc));
    const uint8_t *total = (const uint8_t *)(cand + SVT_AMD_ME_PU_COUNT * nc);
    OisCu32Cu16Results_t *a = pcs->oisCu32Cu16Results[lcuIndex];
    OisCu8Results_t *b = pcs->oisCu8Results[lcuIndex];
    for (int cu = 1; cu < SVT_AMD_ME_PU_COUNT; cu++) {
        OisCandidate_t *c = cu < 21 ? a->sortedOisCandidate[cu] : b->sortedOisCandidate[cu - 21];
        for (int k = 0; k < nc; k++) {
            const uint32_t w = cand[cu * nc + k];
            if (w & SVT_AMD_OIS_W_DIST)
                c[k].distortion = w & 0xFFFFFu;
            if (w & SVT_AMD_OIS_W_VALID)
                c[k].validDistortion = (w >> 20) & 1u;
            if (w & SVT_AMD_OIS_W_MODE)
                c[k].intraMode = w >> 24;
        }
        if (total[cu] != 0xFF) {
            if (cu < 21)
                a->totalIntraLumaMode[cu] = total[cu];
            else
                b->totalIntraLumaMode[cu - 21] = total[cu];
        }
    }
    if (front_verify()) {
        OisCu32Cu16Results_t da = *a;
        OisCu8Results_t db = *b;
        (void)__real_OpenLoopIntraSearchLcu(pcs, lcuIndex, ctx, inputPtr);
        int bad = 0;
        for (int cu = 1; cu < SVT_AMD_ME_PU_COUNT && !bad; cu++) { /* the fields the device's records carry for this unit are the fields the reference writes */
            const OisCandidate_t *x = cu < 21 ? da.sortedOisCandidate[cu] : db.sortedOisCandidate[cu - 21], *y = cu < 21 ? a->sortedOisCandidate[cu] : b->sortedOisCandidate[cu - 21];
            for (int k = 0; k < nc && !bad; k++) {
                const uint32_t w = cand[cu * nc + k];
                bad = ((w & SVT_AMD_OIS_W_DIST) && x[k].distortion != y[k].distortion) || ((w & SVT_AMD_OIS_W_VALID) && x[k].validDistortion != y[k].validDistortion) ||
                      ((w & SVT_AMD_OIS_W_MODE) && x[k].intraMode != y[k].intraMode);
            }
            if (total[cu] != 0xFF)
                bad = bad || (cu < 21 ? da.totalIntraLumaMode[cu] != a->totalIntraLumaMode[cu] : db.totalIntraLumaMode[cu - 21] != b->totalIntraLumaMode[cu - 21]);
            if (bad && __atomic_load_n(&g_ois_mismatch, __ATOMIC_RELAXED) < 4)
                fprintf(stderr, "svt_hook_me: FRONT VERIFY picture %llu lcu %u: open-loop intra search of unit %d differs\n", (unsigned long long)pcs->pictureNumber, lcuIndex, cu);
        }
        __atomic_add_fetch(&g_ois_verified, 1, __ATOMIC_RELAXED);
        if (bad)
            __atomic_add_fetch(&g_ois_mismatch, 1, __ATOMIC_RELAXED);
    }
    __atomic_add_fetch(&g_ois_lcus, 1, __ATOMIC_RELAXED);
    front_served(e, &e->ois_left);
    return EB_ErrorNone;
}

/*
 * Mode-decision luma full loop: ProductFullLoop (EbFullLoop.c:185, called from PerformFullLoop,
 * EbProductCodingLoop.c:4445) is answered per call by svt_amd_full_loop_luma() whenever the candidate uses the
 * configuration the fused kernel implements (no RDOQ / PM-core, coefficient-domain distortion, no CABAC-context
 * update: every preset >= encMode 5 except the lowest-delay corner cases); other calls go to the reference code.
 * This binding moves each candidate over PCIe on its own, so it proves parity, not speed - the batched form
 * svt_amd_full_loop_luma_batch is the product path.  Off unless SVT_HOOK_FULLLOOP=1.
 */
void __real_ProductFullLoop(EbPictureBufferDesc_t *inputPicturePtr, EB_U32 inputOriginIndex,
                            ModeDecisionCandidateBuffer_t *candidateBuffer, ModeDecisionContext_t *contextPtr,
                            const CodedUnitStats_t *cuStatsPtr, PictureControlSet_t *pcs, EB_U32 qp,
                            EB_U32 *yCountNonZeroCoeffs, EB_U64 *yCoeffBits, EB_U64 *yFullDistortion);
static unsigned long g_fl_gpu, g_fl_cpu, g_fl_cabac_gpu, g_cl_cabac_gpu;
_Static_assert(sizeof(CoeffCtxtMdl_t) == SVT_AMD_COEFF_CTX_WORDS * 4, "CoeffCtxtMdl_t layout");
static int g_fl_state; /* 0 unknown, 1 on, -1 off */

void __wrap_ProductFullLoop(EbPictureBufferDesc_t *inputPicturePtr, EB_U32 inputOriginIndex,
                            ModeDecisionCandidateBuffer_t *candidateBuffer, ModeDecisionContext_t *contextPtr,
                            const CodedUnitStats_t *cuStatsPtr, PictureControlSet_t *pcs, EB_U32 qp,
                            EB_U32 *yCountNonZeroCoeffs, EB_U64 *yCoeffBits, EB_U64 *yFullDistortion)
{
    if (g_fl_state == 0)
        g_fl_state = getenv("SVT_HOOK_FULLLOOP") ? 1 : -1;
    if (g_fl_state < 0 || !g_ctx || (contextPtr->rdoqPmCoreMethod && contextPtr->rdoqPmCoreMethod != EB_PMCORE) ||
        contextPtr->spatialSseFullLoop || contextPtr->pfMdMode > 1) {
        if (g_fl_state > 0) {
            svt_hook_lock(&g_lock);
            g_fl_cpu++;
            svt_hook_unlock(&g_lock);
        }
        __real_ProductFullLoop(inputPicturePtr, inputOriginIndex, candidateBuffer, contextPtr, cuStatsPtr, pcs, qp,
                               yCountNonZeroCoeffs, yCoeffBits, yFullDistortion);
        return;
    }
    ModeDecisionCandidate_t *c = candidateBuffer->candidatePtr;
    const uint32_t size = cuStatsPtr->size;
    const uint32_t origin = size == 64 ? 0 : cuStatsPtr->originX + (cuStatsPtr->originY << 6);
    SvtAmdFullLoopIn in;
    SvtAmdFullLoopOut out;
    memset(&in, 0, sizeof(in));
    in.size = size, in.qp = qp, in.slice_type = pcs->sliceType, in.pf_mode = contextPtr->pfMdMode;
    in.pm_core = (uint16_t)contextPtr->rdoqPmCoreMethod;
    in.cand_type = c->type, in.intra_luma_mode = c->intraLumaMode, in.full_lambda = contextPtr->fullLambda;
    in.cbf_bits[0] = c->mdRateEstimationPtr->lumaCbfBits[0], in.cbf_bits[1] = c->mdRateEstimationPtr->lumaCbfBits[1];
    in.cbf_bits[2] = c->mdRateEstimationPtr->lumaCbfBits[5], in.cbf_bits[3] = c->mdRateEstimationPtr->lumaCbfBits[6];
    in.ycbf = c->yCbf, in.coeff_bits = *yCoeffBits, in.dist[0] = yFullDistortion[0], in.dist[1] = yFullDistortion[1];
    int16_t *q = (int16_t *)candidateBuffer->residualQuantCoeffPtr->bufferY + origin; /* residual in, quantised out */
    int16_t *r = (int16_t *)candidateBuffer->reconCoeffPtr->bufferY + origin;
    svt_hook_lock(&g_lock);
    /* coeffCabacUpdate (full-depth pictures, EbEncDecProcess.c:2115): the candidate's context model goes with the call and comes
     * back updated (EbFullLoop.c:265-280; the mode decision copies it from / to latestValidCoeffCtxModel around the loop) */
    if (contextPtr->coeffCabacUpdate
            ? svt_amd_full_loop_luma_cabac(g_ctx, (const SvtAmdCabacCost *)contextPtr->CabacCost, &in, q, q, r, 64,
                                           (uint32_t *)&candidateBuffer->candBuffCoeffCtxModel, &out)
            : svt_amd_full_loop_luma(g_ctx, (const SvtAmdCabacCost *)contextPtr->CabacCost, &in, q, q, r, 64, &out))
        die("svt_amd_full_loop_luma");
    if (contextPtr->coeffCabacUpdate)
        g_fl_cabac_gpu++;
    if (g_fl_gpu++ == 0 && g_verbose)
        fprintf(stderr, "svt_hook_me: luma full loop (ProductFullLoop) on the GPU\n");
    if (g_verbose && (g_fl_gpu % 2000) == 0)
        fprintf(stderr, "svt_hook_me: %lu full-loop candidates on the GPU, %lu on the CPU\n", g_fl_gpu, g_fl_cpu);
    svt_hook_unlock(&g_lock);
    if (size == 64)
        for (int k = 1; k < 5; k++)
            yCountNonZeroCoeffs[k] = out.nz[k];
    else
        yCountNonZeroCoeffs[0] = out.nz[0];
    *yCoeffBits = out.coeff_bits;
    yFullDistortion[0] = out.dist[0], yFullDistortion[1] = out.dist[1];
    c->yCbf = out.ycbf;
    for (int k = 0; k < 4; k++) {
        candidateBuffer->yDc[k] = out.ydc[k];
        candidateBuffer->yCountNonZeroCoeffs[k] = out.cand_nz[k];
    }
}

/*
 * Mode-decision chroma full loop: the pair FullLoop_R (EbFullLoop.c:579) + CuFullDistortionFastTuMode_R (:873), called
 * back to back with the chroma mask (EbProductCodingLoop.c:4291-4319, :4518-4547), is answered by one
 * svt_amd_full_loop_chroma() call made from the first of the two; the second hands out the stashed results.  Same
 * conditions and the same SVT_HOOK_FULLLOOP=1 switch as the luma binding above.
 */
void __real_FullLoop_R(LargestCodingUnit_t *lcuPtr, ModeDecisionCandidateBuffer_t *candidateBuffer,
                       ModeDecisionContext_t *contextPtr, const CodedUnitStats_t *cuStatsPtr,
                       EbPictureBufferDesc_t *inputPicturePtr, PictureControlSet_t *pcs, EB_U32 componentMask, EB_U32 cbQp,
                       EB_U32 crQp, EB_U32 *cbCountNonZeroCoeffs, EB_U32 *crCountNonZeroCoeffs);
void __real_CuFullDistortionFastTuMode_R(EbPictureBufferDesc_t *inputPicturePtr, EB_U32 inputCbOriginIndex,
                                         LargestCodingUnit_t *lcuPtr, ModeDecisionCandidateBuffer_t *candidateBuffer,
                                         ModeDecisionContext_t *contextPtr, ModeDecisionCandidate_t *candidatePtr,
                                         const CodedUnitStats_t *cuStatsPtr, EB_U64 cbFullDistortion[DIST_CALC_TOTAL],
                                         EB_U64 crFullDistortion[DIST_CALC_TOTAL],
                                         EB_U32 countNonZeroCoeffs[3][MAX_NUM_OF_TU_PER_CU], EB_U32 componentMask,
                                         EB_U64 *cbCoeffBits, EB_U64 *crCoeffBits);
static unsigned long g_cl_gpu, g_cl_cpu;
static __thread SvtAmdChromaLoopOut t_chroma_out;
static __thread const ModeDecisionCandidateBuffer_t *t_chroma_for; /* candidate buffer the stash belongs to */

void __wrap_FullLoop_R(LargestCodingUnit_t *lcuPtr, ModeDecisionCandidateBuffer_t *candidateBuffer,
                       ModeDecisionContext_t *contextPtr, const CodedUnitStats_t *cuStatsPtr,
                       EbPictureBufferDesc_t *inputPicturePtr, PictureControlSet_t *pcs, EB_U32 componentMask, EB_U32 cbQp,
                       EB_U32 crQp, EB_U32 *cbCountNonZeroCoeffs, EB_U32 *crCountNonZeroCoeffs)
{
    if (g_fl_state == 0)
        g_fl_state = getenv("SVT_HOOK_FULLLOOP") ? 1 : -1;
    t_chroma_for = NULL;
    /* PM-core leaves chroma alone (EbTransforms.c:2808): its Decoupled... call is the plain quantiser there */
    if (g_fl_state < 0 || !g_ctx || (contextPtr->rdoqPmCoreMethod && contextPtr->rdoqPmCoreMethod != EB_PMCORE) || contextPtr->spatialSseFullLoop ||
        componentMask != PICTURE_BUFFER_DESC_CHROMA_MASK ||
        candidateBuffer->residualQuantCoeffPtr->strideCb != 32 || candidateBuffer->reconCoeffPtr->strideCb != 32) {
        if (g_fl_state > 0) {
            svt_hook_lock(&g_lock);
            g_cl_cpu++;
            svt_hook_unlock(&g_lock);
        }
        __real_FullLoop_R(lcuPtr, candidateBuffer, contextPtr, cuStatsPtr, inputPicturePtr, pcs, componentMask, cbQp, crQp,
                          cbCountNonZeroCoeffs, crCountNonZeroCoeffs);
        return;
    }
    const ModeDecisionCandidate_t *c = candidateBuffer->candidatePtr;
    const uint32_t size = cuStatsPtr->size;
    const uint32_t origin = size == 64 ? 0 : (cuStatsPtr->originX + cuStatsPtr->originY * 32) >> 1;
    SvtAmdChromaLoopIn in;
    memset(&in, 0, sizeof(in));
    in.size = size, in.cb_qp = cbQp, in.cr_qp = crQp, in.slice_type = pcs->sliceType, in.pf_mode = contextPtr->pfMdMode;
    in.cand_type = c->type, in.intra_luma_mode = c->intraLumaMode;
    int16_t *q[2] = {(int16_t *)candidateBuffer->residualQuantCoeffPtr->bufferCb + origin,
                     (int16_t *)candidateBuffer->residualQuantCoeffPtr->bufferCr + origin}; /* residual in, quantised out */
    int16_t *r[2] = {(int16_t *)candidateBuffer->reconCoeffPtr->bufferCb + origin,
                     (int16_t *)candidateBuffer->reconCoeffPtr->bufferCr + origin};
    svt_hook_lock(&g_lock);
    /* coeffCabacUpdate: the model is moved by the rate estimation of the SECOND reference call (TuEstimateCoeffBits_R inside
     * CuFullDistortionFastTuMode_R); nothing touches it between the two, so updating it here is equivalent */
    if (contextPtr->coeffCabacUpdate
            ? svt_amd_full_loop_chroma_cabac(g_ctx, (const SvtAmdCabacCost *)contextPtr->CabacCost, &in, (const int16_t *const *)q, q, r, 32,
                                             (uint32_t *)&candidateBuffer->candBuffCoeffCtxModel, &t_chroma_out)
            : svt_amd_full_loop_chroma(g_ctx, (const SvtAmdCabacCost *)contextPtr->CabacCost, &in, (const int16_t *const *)q, q, r, 32,
                                       &t_chroma_out))
        die("svt_amd_full_loop_chroma");
    if (contextPtr->coeffCabacUpdate)
        g_cl_cabac_gpu++;
    if (g_cl_gpu++ == 0 && g_verbose)
        fprintf(stderr, "svt_hook_me: chroma full loop (FullLoop_R + CuFullDistortionFastTuMode_R) on the GPU\n");
    if (g_verbose && (g_cl_gpu % 2000) == 0)
        fprintf(stderr, "svt_hook_me: %lu chroma full-loop candidates on the GPU, %lu on the CPU\n", g_cl_gpu, g_cl_cpu);
    svt_hook_unlock(&g_lock);
    for (int k = (size == 64 ? 1 : 0); k < (size == 64 ? 5 : 1); k++)
        cbCountNonZeroCoeffs[k] = t_chroma_out.nz[0][k], crCountNonZeroCoeffs[k] = t_chroma_out.nz[1][k];
    t_chroma_for = candidateBuffer;
}

void __wrap_CuFullDistortionFastTuMode_R(EbPictureBufferDesc_t *inputPicturePtr, EB_U32 inputCbOriginIndex,
                                         LargestCodingUnit_t *lcuPtr, ModeDecisionCandidateBuffer_t *candidateBuffer,
                                         ModeDecisionContext_t *contextPtr, ModeDecisionCandidate_t *candidatePtr,
                                         const CodedUnitStats_t *cuStatsPtr, EB_U64 cbFullDistortion[DIST_CALC_TOTAL],
                                         EB_U64 crFullDistortion[DIST_CALC_TOTAL],
                                         EB_U32 countNonZeroCoeffs[3][MAX_NUM_OF_TU_PER_CU], EB_U32 componentMask,
                                         EB_U64 *cbCoeffBits, EB_U64 *crCoeffBits)
{
    if (t_chroma_for != candidateBuffer || componentMask != PICTURE_BUFFER_DESC_CHROMA_MASK) {
        t_chroma_for = NULL;
        __real_CuFullDistortionFastTuMode_R(inputPicturePtr, inputCbOriginIndex, lcuPtr, candidateBuffer, contextPtr,
                                            candidatePtr, cuStatsPtr, cbFullDistortion, crFullDistortion, countNonZeroCoeffs,
                                            componentMask, cbCoeffBits, crCoeffBits);
        return;
    }
    t_chroma_for = NULL;
    const SvtAmdChromaLoopOut *o = &t_chroma_out;
    candidatePtr->cbCbf |= o->cbf[0], candidatePtr->crCbf |= o->cbf[1];
    *cbCoeffBits += o->coeff_bits[0], *crCoeffBits += o->coeff_bits[1];
    cbFullDistortion[0] += o->dist[0][0], cbFullDistortion[1] += o->dist[0][1];
    crFullDistortion[0] += o->dist[1][0], crFullDistortion[1] += o->dist[1][1];
}

/*
 * Final encode pass, reconstruction of a transform unit: EncodeGenerateRecon / EncodeGenerateRecon16bit
 * (EbCodingLoop.c:1084, :1660) are static, but the encode pass only reaches them through the global table
 * EncodeGenerateReconFunctionPtr[2] (:1807).  With SVT_HOOK_RECON=1 its slots are replaced: every plane the call
 * reconstructs (cbf set, CU not skipped) is answered by svt_amd_recon_tu() (inverse transform / DC shortcut / DST +
 * prediction add on the device); 4:2:0 only, anything else goes to the saved reference function.
 */
typedef void (*ReconFn)(EncDecContext_t *, EB_U32, EB_U32, EB_U32, EB_COLOR_FORMAT, EB_BOOL, EB_U32, EbPictureBufferDesc_t *,
                        EbPictureBufferDesc_t *, EB_S16 *);
extern ReconFn EncodeGenerateReconFunctionPtr[2];
static ReconFn g_recon_real[2];
static unsigned long g_recon_gpu;
static int g_recon_on;

static void recon_on_device(int is16, EncDecContext_t *ctx, EB_U32 originX, EB_U32 originY, EB_U32 componentMask,
                            EB_COLOR_FORMAT colorFormat, EB_BOOL secondChroma, EB_U32 tuSize, EbPictureBufferDesc_t *predSamples,
                            EbPictureBufferDesc_t *residual16bit, EB_S16 *scratch)
{
    if (svt_hook_ep_active) { /* the device encoded this LCU: its reconstruction is already here */
        svt_hook_ep_recon(ctx, originX, originY, tuSize, predSamples);
        return;
    }
    if (!g_recon_on || !g_ctx || colorFormat != EB_YUV420 || secondChroma) {
        g_recon_real[is16](ctx, originX, originY, componentMask, colorFormat, secondChroma, tuSize, predSamples, residual16bit, scratch);
        return;
    }
    const CodingUnit_t *cu = ctx->cuPtr;
    const TransformUnit_t *tu = &cu->transformUnitArray[ctx->tuItr];
    const int bps = is16 ? 2 : 1;
    for (int p = 0; p < 3; p++) {
        const int wanted = p == 0 ? (componentMask & PICTURE_BUFFER_DESC_LUMA_MASK) != 0 : (componentMask & PICTURE_BUFFER_DESC_CHROMA_MASK) != 0;
        const int cbf = p == 0 ? tu->lumaCbf : p == 1 ? tu->cbCbf : tu->crCbf;
        if (!wanted || !cbf || cu->skipFlag)
            continue;
        const uint32_t n = p == 0 ? tuSize : (tuSize == 4 ? 4 : tuSize >> 1);
        const int dst = p == 0 && tuSize == 4;
        const int only_dc = tuSize == 4 ? 0 : (p == 0 ? (tu->transCoeffShapeLuma == ONLY_DC_SHAPE || tu->isOnlyDc[0])
                                                      : (tu->transCoeffShapeChroma == ONLY_DC_SHAPE || tu->isOnlyDc[p]));
        uint32_t off, scratchOff, cstride, stride;
        uint8_t *plane;
        int16_t *cplane;
        if (p == 0) {
            stride = predSamples->strideY, plane = predSamples->bufferY, cplane = (int16_t *)residual16bit->bufferY;
            off = (predSamples->originY + originY) * stride + (predSamples->originX + originX);
            scratchOff = ((originY & 63) * 64) + (originX & 63), cstride = 64;
        } else {
            stride = p == 1 ? predSamples->strideCb : predSamples->strideCr;
            plane = p == 1 ? predSamples->bufferCb : predSamples->bufferCr;
            cplane = (int16_t *)(p == 1 ? residual16bit->bufferCb : residual16bit->bufferCr);
            off = ((predSamples->originX + originX) >> 1) + (((predSamples->originY + originY) >> 1) * stride);
            scratchOff = ((originX & 63) >> 1) + (((originY & 63) >> 1) * 32), cstride = 32;
        }
        svt_hook_lock(&g_lock);
        if (svt_amd_recon_tu(g_ctx, bps, (int)n, only_dc, dst, cplane + scratchOff, cstride, plane + (size_t)off * bps, stride,
                             plane + (size_t)off * bps, stride))
            die("svt_amd_recon_tu");
        if (g_recon_gpu++ == 0 && g_verbose)
            fprintf(stderr, "svt_hook_me: transform-unit reconstruction (EncodeGenerateRecon) on the GPU\n");
        svt_hook_unlock(&g_lock);
    }
}
static void recon8(EncDecContext_t *a, EB_U32 b, EB_U32 c, EB_U32 d, EB_COLOR_FORMAT e, EB_BOOL f, EB_U32 g, EbPictureBufferDesc_t *h,
                   EbPictureBufferDesc_t *i, EB_S16 *j)
{
    recon_on_device(0, a, b, c, d, e, f, g, h, i, j);
}
static void recon16(EncDecContext_t *a, EB_U32 b, EB_U32 c, EB_U32 d, EB_COLOR_FORMAT e, EB_BOOL f, EB_U32 g, EbPictureBufferDesc_t *h,
                    EbPictureBufferDesc_t *i, EB_S16 *j)
{
    recon_on_device(1, a, b, c, d, e, f, g, h, i, j);
}
__attribute__((constructor)) static void recon_install(void)
{
    g_recon_on = getenv("SVT_HOOK_RECON") != NULL;
    if (!g_recon_on && !getenv("SVT_HOOK_ENCODEPASS") && !svt_hook_cfg("SVT_HOOK_MD"))
        return;
    g_recon_real[0] = EncodeGenerateReconFunctionPtr[0], g_recon_real[1] = EncodeGenerateReconFunctionPtr[1];
    EncodeGenerateReconFunctionPtr[0] = recon8, EncodeGenerateReconFunctionPtr[1] = recon16;
}

/*
 * Encode-pass intra prediction of a prediction unit: GenerateIntraReferenceSamplesEncodePass (+16bit) and
 * EncodePassIntraPrediction (+16bit) are reached through the global tables GenerateIntraReferenceSamplesFuncTable[2] /
 * EncodePassIntraPredictionFuncTable[2] (EbCodingLoop.c:1814, :1832).  With SVT_HOOK_INTRA=1 both slots are replaced: the
 * first cuts the slices of the neighbour arrays the unit can see into an SvtAmdIntraPuJob (and still lets the reference
 * build its arrays, which nothing reads afterwards), the second answers with svt_amd_intra_pu() - availability,
 * substitution, smoothing, mode dispatch and the three predicted blocks all come from the device.  4:2:0, units of 8..32.
 */
typedef EB_ERRORTYPE (*IntraGenFn)(EB_BOOL, EB_BOOL, EB_U32, EB_U32, EB_U32, EB_U32, EB_U32, NeighborArrayUnit_t *, NeighborArrayUnit_t *,
                                   NeighborArrayUnit_t *, NeighborArrayUnit_t *, void *, EB_COLOR_FORMAT, EB_BOOL, EB_BOOL, EB_BOOL);
typedef EB_ERRORTYPE (*IntraPredFn)(void *, EB_U32, EB_U32, EB_U32, EB_U32, EbPictureBufferDesc_t *, EB_COLOR_FORMAT, EB_BOOL, EB_U32,
                                    EB_U32, EB_U32);
extern IntraGenFn GenerateIntraReferenceSamplesFuncTable[2];
extern IntraPredFn EncodePassIntraPredictionFuncTable[2];
static IntraGenFn g_intra_gen[2];
static IntraPredFn g_intra_pred[2];
static unsigned long g_intra_gpu;
static int g_intra_on;
static __thread SvtAmdIntraPuJob t_intra_job;
static __thread void *t_intra_for; /* reference-sample object the stashed job belongs to */

static uint16_t na_rd(const uint8_t *a, uint32_t i, int bps) { return bps == 1 ? a[i] : ((const uint16_t *)a)[i]; }

static EB_ERRORTYPE intra_gen(int is16, EB_BOOL constrained, EB_BOOL strong, EB_U32 originX, EB_U32 originY, EB_U32 size, EB_U32 lcuSize,
                              EB_U32 cuDepth, NeighborArrayUnit_t *mode, NeighborArrayUnit_t *y, NeighborArrayUnit_t *cb,
                              NeighborArrayUnit_t *cr, void *ref, EB_COLOR_FORMAT cf, EB_BOOL pl, EB_BOOL pt, EB_BOOL pr)
{
    t_intra_for = NULL;
    if (svt_hook_ep_active)
        return EB_ErrorNone; /* the device encoded this LCU: nothing reads the reference-sample arrays */
    if (g_intra_on && g_ctx && cf == EB_YUV420 && size >= 8 && size <= 32) {
        SvtAmdIntraPuJob *j = &t_intra_job;
        const int bps = is16 ? 2 : 1;
        memset(j, 0, sizeof(*j));
        j->size = size, j->constrained_intra = constrained, j->strong_smoothing = strong;
        j->pic_left = pl, j->pic_top = pt, j->pic_right = pr;
        uint32_t lg = 0;
        while ((1u << lg) < size)
            lg++;
        const uint32_t cuIndex = ((originY & (lcuSize - 1)) >> lg) * (1u << cuDepth) + ((originX & (lcuSize - 1)) >> lg);
        j->bottom_left_ok = isBottomLeftAvailable(cuDepth, cuIndex), j->top_right_ok = isUpperRightAvailable(cuDepth, cuIndex);
        for (uint32_t k = 0; k < 2 * size / 4; k++) {
            const uint32_t li = GetNeighborArrayUnitLeftIndex(mode, originY + 4 * k), ti = GetNeighborArrayUnitTopIndex(mode, originX + 4 * k);
            j->mode_left[k] = li >= mode->leftArraySize ? 0xFE : mode->leftArray[li];
            j->mode_top[k] = ti >= mode->topArraySize ? 0xFE : mode->topArray[ti];
        }
        j->mode_tl = mode->topLeftArray[GetNeighborArrayUnitTopLeftIndex(mode, (EB_S32)originX, (EB_S32)originY)];
        NeighborArrayUnit_t *na[3] = {y, cb, cr};
        for (int p = 0; p < 3; p++) {
            const uint32_t sh = p ? 1 : 0, n2 = (2 * size) >> sh, ox = originX >> sh, oy = originY >> sh;
            for (uint32_t i = 0; i < n2; i++) {
                const uint32_t k = (i << sh) >> 2;
                j->left[p][i] = j->mode_left[k] == 0xFE ? 0 : na_rd(na[p]->leftArray, oy + i, bps);
                j->top[p][i] = j->mode_top[k] == 0xFE ? 0 : na_rd(na[p]->topArray, ox + i, bps);
            }
            j->tl[p] = p == 0 ? na_rd(y->topLeftArray, MAX_PICTURE_HEIGHT_SIZE + originX - originY, bps)
                              : na_rd(na[p]->topLeftArray, ((MAX_PICTURE_HEIGHT_SIZE - originY) >> 1) + (originX >> 1), bps);
        }
        t_intra_for = ref;
    }
    return g_intra_gen[is16](constrained, strong, originX, originY, size, lcuSize, cuDepth, mode, y, cb, cr, ref, cf, pl, pt, pr);
}

/* intra 4x4 coding units (EbCodingLoop.c:3594-3690): the luma generator per 4x4 partition and the chroma generator once per 8x8
 * coding unit are reached through two more global tables; their slots stash a size-4 luma job / a size-8 chroma job, and the
 * prediction slot answers the luma-mask and the chroma-mask calls from them. */
typedef EB_ERRORTYPE (*LumaGenFn)(EB_BOOL, EB_BOOL, EB_U32, EB_U32, EB_U32, EB_U32, EB_U32, NeighborArrayUnit_t *, NeighborArrayUnit_t *,
                                  NeighborArrayUnit_t *, NeighborArrayUnit_t *, void *, EB_BOOL, EB_BOOL, EB_BOOL);
typedef EB_ERRORTYPE (*ChromaGenFn)(EB_BOOL, EB_BOOL, EB_U32, EB_U32, EB_U32, EB_U32, EB_U32, NeighborArrayUnit_t *, NeighborArrayUnit_t *,
                                    NeighborArrayUnit_t *, NeighborArrayUnit_t *, void *, EB_COLOR_FORMAT, EB_BOOL, EB_BOOL, EB_BOOL, EB_BOOL);
extern LumaGenFn GenerateLumaIntraReferenceSamplesFuncTable[2];
extern ChromaGenFn GenerateChromaIntraReferenceSamplesFuncTable[2];
static LumaGenFn g_intra_lgen[2];
static ChromaGenFn g_intra_cgen[2];
static __thread SvtAmdIntraPuJob t_intra4_job[2]; /* [0] luma partition, [1] chroma pair */
static __thread void *t_intra4_for[2];
static unsigned long g_intra4_gpu;

static void intra_slices(SvtAmdIntraPuJob *j, int bps, EB_BOOL constrained, EB_BOOL strong, EB_U32 originX, EB_U32 originY, EB_U32 size,
                         EB_U32 lcuSize, EB_U32 partitionDepth, NeighborArrayUnit_t *mode, NeighborArrayUnit_t *na[3], int p0, int p1, EB_BOOL pl,
                         EB_BOOL pt, EB_BOOL pr)
{
    memset(j, 0, sizeof(*j));
    j->size = size, j->constrained_intra = constrained, j->strong_smoothing = strong;
    j->pic_left = pl, j->pic_top = pt, j->pic_right = pr;
    uint32_t lg = 0;
    while ((1u << lg) < size)
        lg++;
    const uint32_t cuIndex = ((originY & (lcuSize - 1)) >> lg) * (1u << partitionDepth) + ((originX & (lcuSize - 1)) >> lg);
    j->bottom_left_ok = isBottomLeftAvailable(partitionDepth, cuIndex), j->top_right_ok = isUpperRightAvailable(partitionDepth, cuIndex);
    for (uint32_t k = 0; k < 2 * size / 4; k++) {
        const uint32_t li = GetNeighborArrayUnitLeftIndex(mode, originY + 4 * k), ti = GetNeighborArrayUnitTopIndex(mode, originX + 4 * k);
        j->mode_left[k] = li >= mode->leftArraySize ? 0xFE : mode->leftArray[li];
        j->mode_top[k] = ti >= mode->topArraySize ? 0xFE : mode->topArray[ti];
    }
    j->mode_tl = mode->topLeftArray[GetNeighborArrayUnitTopLeftIndex(mode, (EB_S32)originX, (EB_S32)originY)];
    for (int p = p0; p < p1; p++) {
        const uint32_t sh = p ? 1 : 0, n2 = (2 * size) >> sh, ox = originX >> sh, oy = originY >> sh;
        for (uint32_t i = 0; i < n2; i++) {
            const uint32_t k = (i << sh) >> 2;
            j->left[p][i] = j->mode_left[k] == 0xFE ? 0 : na_rd(na[p]->leftArray, oy + i, bps);
            j->top[p][i] = j->mode_top[k] == 0xFE ? 0 : na_rd(na[p]->topArray, ox + i, bps);
        }
        j->tl[p] = p == 0 ? na_rd(na[0]->topLeftArray, MAX_PICTURE_HEIGHT_SIZE + originX - originY, bps)
                          : na_rd(na[p]->topLeftArray, ((MAX_PICTURE_HEIGHT_SIZE - originY) >> 1) + (originX >> 1), bps);
    }
}

static EB_ERRORTYPE intra_lgen(int is16, EB_BOOL constrained, EB_BOOL strong, EB_U32 originX, EB_U32 originY, EB_U32 size, EB_U32 lcuSize,
                               EB_U32 cuDepth, NeighborArrayUnit_t *mode, NeighborArrayUnit_t *y, NeighborArrayUnit_t *cb, NeighborArrayUnit_t *cr,
                               void *ref, EB_BOOL pl, EB_BOOL pt, EB_BOOL pr)
{
    t_intra4_for[0] = NULL;
    if (g_intra_on && g_ctx && size == 4) {
        NeighborArrayUnit_t *na[3] = {y, cb, cr};
        intra_slices(&t_intra4_job[0], is16 ? 2 : 1, constrained, strong, originX, originY, 4, lcuSize, cuDepth + 1, mode, na, 0, 1, pl, pt, pr);
        t_intra4_for[0] = ref;
    }
    return g_intra_lgen[is16](constrained, strong, originX, originY, size, lcuSize, cuDepth, mode, y, cb, cr, ref, pl, pt, pr);
}

static EB_ERRORTYPE intra_cgen(int is16, EB_BOOL constrained, EB_BOOL strong, EB_U32 originX, EB_U32 originY, EB_U32 size, EB_U32 lcuSize,
                               EB_U32 cuDepth, NeighborArrayUnit_t *mode, NeighborArrayUnit_t *y, NeighborArrayUnit_t *cb, NeighborArrayUnit_t *cr,
                               void *ref, EB_COLOR_FORMAT cf, EB_BOOL second, EB_BOOL pl, EB_BOOL pt, EB_BOOL pr)
{
    t_intra4_for[1] = NULL;
    if (g_intra_on && g_ctx && size == 8 && cf == EB_YUV420 && !second) {
        NeighborArrayUnit_t *na[3] = {y, cb, cr};
        intra_slices(&t_intra4_job[1], is16 ? 2 : 1, constrained, strong, originX, originY, 8, lcuSize, cuDepth, mode, na, 1, 3, pl, pt, pr);
        t_intra4_for[1] = ref;
    }
    return g_intra_cgen[is16](constrained, strong, originX, originY, size, lcuSize, cuDepth, mode, y, cb, cr, ref, cf, second, pl, pt, pr);
}

static EB_ERRORTYPE intra_pred(int is16, void *ref, EB_U32 originX, EB_U32 originY, EB_U32 puSize, EB_U32 puChromaSize,
                               EbPictureBufferDesc_t *pic, EB_COLOR_FORMAT cf, EB_BOOL second, EB_U32 lumaMode, EB_U32 chromaMode,
                               EB_U32 mask)
{
    if (svt_hook_ep_active)
        return EB_ErrorNone;
    if (puSize == 4 && cf == EB_YUV420 && !second && lumaMode <= 34 &&
        (mask == PICTURE_BUFFER_DESC_LUMA_MASK || mask == PICTURE_BUFFER_DESC_CHROMA_MASK)) { /* intra 4x4 coding unit */
        const int c = mask == PICTURE_BUFFER_DESC_CHROMA_MASK;
        void *stash4 = t_intra4_for[c];
        t_intra4_for[c] = NULL;
        if (stash4 && stash4 == ref) {
            const size_t bps4 = is16 ? 2 : 1;
            SvtAmdIntraPuJob *j4 = &t_intra4_job[c];
            j4->luma_mode = (uint8_t)lumaMode, j4->chroma_mode = (uint8_t)chromaMode;
            svt_hook_lock(&g_lock);
            int rc4;
            if (!c)
                rc4 = svt_amd_intra_pu(g_ctx, (int)bps4, j4, pic->bufferY + ((size_t)originY * pic->strideY + originX) * bps4, pic->strideY, NULL,
                                       NULL, 0);
            else
                rc4 = svt_amd_intra_pu(g_ctx, (int)bps4, j4, NULL, 0,
                                       pic->bufferCb + ((size_t)(originY >> 1) * pic->strideCb + (originX >> 1)) * bps4,
                                       pic->bufferCr + ((size_t)(originY >> 1) * pic->strideCr + (originX >> 1)) * bps4, pic->strideCb);
            if (rc4)
                die("svt_amd_intra_pu (intra 4x4)");
            if (g_intra4_gpu++ == 0 && g_verbose)
                fprintf(stderr, "svt_hook_me: encode-pass intra 4x4 prediction on the GPU\n");
            svt_hook_unlock(&g_lock);
            return EB_ErrorNone;
        }
    }
    void *stash = t_intra_for;
    t_intra_for = NULL;
    if (!stash || stash != ref || puSize != t_intra_job.size || second || mask != PICTURE_BUFFER_DESC_FULL_MASK || lumaMode > 34)
        return g_intra_pred[is16](ref, originX, originY, puSize, puChromaSize, pic, cf, second, lumaMode, chromaMode, mask);
    const size_t bps = is16 ? 2 : 1;
    t_intra_job.luma_mode = (uint8_t)lumaMode, t_intra_job.chroma_mode = (uint8_t)chromaMode;
    svt_hook_lock(&g_lock);
    if (svt_amd_intra_pu(g_ctx, (int)bps, &t_intra_job, pic->bufferY + ((size_t)originY * pic->strideY + originX) * bps, pic->strideY,
                         pic->bufferCb + ((size_t)(originY >> 1) * pic->strideCb + (originX >> 1)) * bps,
                         pic->bufferCr + ((size_t)(originY >> 1) * pic->strideCr + (originX >> 1)) * bps, pic->strideCb))
        die("svt_amd_intra_pu");
    if (g_intra_gpu++ == 0 && g_verbose)
        fprintf(stderr, "svt_hook_me: encode-pass intra prediction (reference samples + prediction) on the GPU\n");
    svt_hook_unlock(&g_lock);
    return EB_ErrorNone;
}

#define IGEN_ARGS EB_BOOL a, EB_BOOL b, EB_U32 c, EB_U32 d, EB_U32 e, EB_U32 f, EB_U32 g, NeighborArrayUnit_t *h, NeighborArrayUnit_t *i, \
                  NeighborArrayUnit_t *j, NeighborArrayUnit_t *k, void *l, EB_COLOR_FORMAT m, EB_BOOL n, EB_BOOL o, EB_BOOL p
static EB_ERRORTYPE intra_gen8(IGEN_ARGS) { return intra_gen(0, a, b, c, d, e, f, g, h, i, j, k, l, m, n, o, p); }
static EB_ERRORTYPE intra_gen16(IGEN_ARGS) { return intra_gen(1, a, b, c, d, e, f, g, h, i, j, k, l, m, n, o, p); }
#define IPRED_ARGS void *a, EB_U32 b, EB_U32 c, EB_U32 d, EB_U32 e, EbPictureBufferDesc_t *f, EB_COLOR_FORMAT g, EB_BOOL h, EB_U32 i, EB_U32 j, EB_U32 k
static EB_ERRORTYPE intra_pred8(IPRED_ARGS) { return intra_pred(0, a, b, c, d, e, f, g, h, i, j, k); }
static EB_ERRORTYPE intra_pred16(IPRED_ARGS) { return intra_pred(1, a, b, c, d, e, f, g, h, i, j, k); }
#define ILGEN_ARGS EB_BOOL a, EB_BOOL b, EB_U32 c, EB_U32 d, EB_U32 e, EB_U32 f, EB_U32 g, NeighborArrayUnit_t *h, NeighborArrayUnit_t *i, \
                   NeighborArrayUnit_t *j, NeighborArrayUnit_t *k, void *l, EB_BOOL n, EB_BOOL o, EB_BOOL p
static EB_ERRORTYPE intra_lgen8(ILGEN_ARGS) { return intra_lgen(0, a, b, c, d, e, f, g, h, i, j, k, l, n, o, p); }
static EB_ERRORTYPE intra_lgen16(ILGEN_ARGS) { return intra_lgen(1, a, b, c, d, e, f, g, h, i, j, k, l, n, o, p); }
#define ICGEN_ARGS EB_BOOL a, EB_BOOL b, EB_U32 c, EB_U32 d, EB_U32 e, EB_U32 f, EB_U32 g, NeighborArrayUnit_t *h, NeighborArrayUnit_t *i, \
                   NeighborArrayUnit_t *j, NeighborArrayUnit_t *k, void *l, EB_COLOR_FORMAT m, EB_BOOL q, EB_BOOL n, EB_BOOL o, EB_BOOL p
static EB_ERRORTYPE intra_cgen8(ICGEN_ARGS) { return intra_cgen(0, a, b, c, d, e, f, g, h, i, j, k, l, m, q, n, o, p); }
static EB_ERRORTYPE intra_cgen16(ICGEN_ARGS) { return intra_cgen(1, a, b, c, d, e, f, g, h, i, j, k, l, m, q, n, o, p); }
__attribute__((constructor)) static void intra_install(void)
{
    g_intra_on = getenv("SVT_HOOK_INTRA") != NULL;
    if (!g_intra_on && !getenv("SVT_HOOK_ENCODEPASS") && !svt_hook_cfg("SVT_HOOK_MD"))
        return;
    g_intra_gen[0] = GenerateIntraReferenceSamplesFuncTable[0], g_intra_gen[1] = GenerateIntraReferenceSamplesFuncTable[1];
    g_intra_pred[0] = EncodePassIntraPredictionFuncTable[0], g_intra_pred[1] = EncodePassIntraPredictionFuncTable[1];
    GenerateIntraReferenceSamplesFuncTable[0] = intra_gen8, GenerateIntraReferenceSamplesFuncTable[1] = intra_gen16;
    EncodePassIntraPredictionFuncTable[0] = intra_pred8, EncodePassIntraPredictionFuncTable[1] = intra_pred16;
    g_intra_lgen[0] = GenerateLumaIntraReferenceSamplesFuncTable[0], g_intra_lgen[1] = GenerateLumaIntraReferenceSamplesFuncTable[1];
    g_intra_cgen[0] = GenerateChromaIntraReferenceSamplesFuncTable[0], g_intra_cgen[1] = GenerateChromaIntraReferenceSamplesFuncTable[1];
    GenerateLumaIntraReferenceSamplesFuncTable[0] = intra_lgen8, GenerateLumaIntraReferenceSamplesFuncTable[1] = intra_lgen16;
    GenerateChromaIntraReferenceSamplesFuncTable[0] = intra_cgen8, GenerateChromaIntraReferenceSamplesFuncTable[1] = intra_cgen16;
}

/* Mode-decision side: IntraPredictionCl (EbIntraPrediction.c:3682, reached through ProductPredictionFunTableCl) predicts the
 * luma block and / or the chroma pair of a candidate from the mode decision's own neighbour arrays into the candidate's
 * LCU-local prediction buffer.  Same switch; the reference's generators still run (their flags and arrays are host state
 * other paths read), the predicted samples come from the device. */
EB_ERRORTYPE __real_IntraPredictionCl(ModeDecisionContext_t *md, EB_U32 componentMask, PictureControlSet_t *pcs,
                                      ModeDecisionCandidateBuffer_t *cand);
static unsigned long g_md_intra_gpu;
static int g_md_intra_state;

static void md_intra_job(SvtAmdIntraPuJob *j, ModeDecisionContext_t *md, int chroma)
{
    const uint32_t size = md->cuStats->size, originX = md->cuOriginX, originY = md->cuOriginY, cuDepth = md->cuStats->depth;
    NeighborArrayUnit_t *mode = md->modeTypeNeighborArray;
    memset(j, 0, sizeof(*j));
    j->size = size, j->constrained_intra = 0, j->strong_smoothing = 1;
    if (!chroma) { /* EbProductCodingLoop.c:274-276; the chroma generator is called without edge flags (:2203-2219) */
        const uint32_t m = md->lcuPtr->size - 1;
        j->pic_left = md->lcuPtr->lcuEdgeInfoPtr->tileLeftEdgeFlag == EB_TRUE && (originX & m) == 0;
        j->pic_top = md->lcuPtr->lcuEdgeInfoPtr->tileTopEdgeFlag == EB_TRUE && (originY & m) == 0;
        j->pic_right = md->lcuPtr->lcuEdgeInfoPtr->tileRightEdgeFlag == EB_TRUE && ((originX + size) & m) == 0;
    }
    uint32_t lg = 0;
    while ((1u << lg) < size)
        lg++;
    const uint32_t cuIndex = ((originY & 63) >> lg) * (1u << cuDepth) + ((originX & 63) >> lg);
    j->bottom_left_ok = isBottomLeftAvailable(cuDepth, cuIndex), j->top_right_ok = isUpperRightAvailable(cuDepth, cuIndex);
    for (uint32_t k = 0; k < 2 * size / 4; k++) {
        const uint32_t li = GetNeighborArrayUnitLeftIndex(mode, originY + 4 * k), ti = GetNeighborArrayUnitTopIndex(mode, originX + 4 * k);
        j->mode_left[k] = li >= mode->leftArraySize ? 0xFE : mode->leftArray[li];
        j->mode_top[k] = ti >= mode->topArraySize ? 0xFE : mode->topArray[ti];
    }
    j->mode_tl = mode->topLeftArray[GetNeighborArrayUnitTopLeftIndex(mode, (EB_S32)originX, (EB_S32)originY)];
    NeighborArrayUnit_t *na[3] = {md->lumaReconNeighborArray, md->cbReconNeighborArray, md->crReconNeighborArray};
    for (int p = chroma ? 1 : 0; p < (chroma ? 3 : 1); p++) {
        const uint32_t sh = p ? 1 : 0, n2 = (2 * size) >> sh, ox = originX >> sh, oy = originY >> sh;
        for (uint32_t i = 0; i < n2; i++) {
            const uint32_t k = (i << sh) >> 2;
            j->left[p][i] = j->mode_left[k] == 0xFE ? 0 : na[p]->leftArray[oy + i];
            j->top[p][i] = j->mode_top[k] == 0xFE ? 0 : na[p]->topArray[ox + i];
        }
        j->tl[p] = p == 0 ? na[0]->topLeftArray[MAX_PICTURE_HEIGHT_SIZE + originX - originY]
                          : na[p]->topLeftArray[((MAX_PICTURE_HEIGHT_SIZE - originY) >> 1) + (originX >> 1)];
    }
}

EB_ERRORTYPE __wrap_IntraPredictionCl(ModeDecisionContext_t *md, EB_U32 componentMask, PictureControlSet_t *pcs,
                                      ModeDecisionCandidateBuffer_t *cand)
{
    if (g_md_intra_state == 0)
        g_md_intra_state = getenv("SVT_HOOK_INTRA") ? 1 : -1;
    const uint32_t size = md->cuStats->size, lumaMode = cand->candidatePtr->intraLumaMode;
    const int chromaAsked = (componentMask & PICTURE_BUFFER_DESC_CHROMA_MASK) != 0;
    if (g_md_intra_state < 0 || !g_ctx || md->intraMdOpenLoopFlag || size < 8 || size > 32 || lumaMode > 34 ||
        (chromaAsked && ((componentMask & PICTURE_BUFFER_DESC_CHROMA_MASK) != PICTURE_BUFFER_DESC_CHROMA_MASK ||
                         !md->useChromaInformationInFullLoop))) {
        COUNT_CPU(IntraPredictionCl);
        return __real_IntraPredictionCl(md, componentMask, pcs, cand);
    }
    EbPictureBufferDesc_t *in = pcs->ParentPcsPtr->enhancedPicturePtr, *pred = cand->predictionPtr;
    SvtAmdIntraPuJob j;
    if (componentMask & PICTURE_BUFFER_DESC_LUMA_MASK) {
        if (md->lumaIntraRefSamplesGenDone == EB_FALSE)
            GenerateIntraLumaReferenceSamplesMd(md, in);
        md_intra_job(&j, md, 0);
        j.luma_mode = (uint8_t)lumaMode, j.chroma_mode = 4;
        svt_hook_lock(&g_lock);
        if (svt_amd_intra_pu(g_ctx, 1, &j, pred->bufferY + (md->cuOriginY & 63) * 64 + (md->cuOriginX & 63), pred->strideY, NULL, NULL, 0))
            die("svt_amd_intra_pu (mode decision, luma)");
        if (g_md_intra_gpu++ == 0 && g_verbose)
            fprintf(stderr, "svt_hook_me: mode-decision intra prediction (IntraPredictionCl) on the GPU\n");
        svt_hook_unlock(&g_lock);
    }
    if (chromaAsked) {
        if (md->chromaIntraRefSamplesGenDone == EB_FALSE)
            GenerateIntraChromaReferenceSamplesMd(md, in);
        md_intra_job(&j, md, 1);
        j.luma_mode = (uint8_t)lumaMode, j.chroma_mode = 4;
        const uint32_t o = (((md->cuOriginY & 63) * 32) + (md->cuOriginX & 63)) >> 1;
        svt_hook_lock(&g_lock);
        if (svt_amd_intra_pu(g_ctx, 1, &j, NULL, 0, pred->bufferCb + o, pred->bufferCr + o, pred->strideCb))
            die("svt_amd_intra_pu (mode decision, chroma)");
        g_md_intra_gpu++;
        svt_hook_unlock(&g_lock);
    }
    return EB_ErrorNone;
}

/* The open-loop twin: IntraPredictionOl (EbIntraPrediction.c:5427, slot of ProductPredictionFunTableOl) predicts from SOURCE
 * neighbours (UpdateNeighborSamplesArrayOL / UpdateChromaNeighborSamplesArrayOL, :4952, :5065: mid-grey where the picture ends,
 * no substitution, no smoothing).  Same switch, same device call: every neighbour group marked available, the literal
 * samples in the job, no_smoothing = 1. */
EB_ERRORTYPE __real_IntraPredictionOl(ModeDecisionContext_t *md, EB_U32 componentMask, PictureControlSet_t *pcs,
                                      ModeDecisionCandidateBuffer_t *cand);
static unsigned long g_md_intra_ol_gpu;

static void ol_slices(uint16_t *left, uint16_t *top, uint16_t *tl, const uint8_t *plane, uint32_t stride, uint32_t x, uint32_t y, uint32_t n,
                      uint32_t width, uint32_t height, int picLeft, int picTop)
{
    const uint8_t *src = plane + (size_t)y * stride + x;
    for (uint32_t i = 0; i < 2 * n; i++)
        left[i] = top[i] = 128;
    *tl = 128;
    if (!picLeft)
        for (uint32_t i = 0; i < 2 * n && y + i < height; i++)
            left[i] = src[(size_t)i * stride - 1];
    if (!picLeft && !picTop)
        *tl = src[-(ptrdiff_t)stride - 1];
    if (!picTop)
        for (uint32_t i = 0; i < 2 * n && x + i < width; i++)
            top[i] = src[i - (ptrdiff_t)stride];
}

EB_ERRORTYPE __wrap_IntraPredictionOl(ModeDecisionContext_t *md, EB_U32 componentMask, PictureControlSet_t *pcs,
                                      ModeDecisionCandidateBuffer_t *cand)
{
    if (g_md_intra_state == 0)
        g_md_intra_state = getenv("SVT_HOOK_INTRA") ? 1 : -1;
    const uint32_t size = md->cuStats->size, lumaMode = cand->candidatePtr->intraLumaMode, ox = md->cuOriginX, oy = md->cuOriginY;
    const int chromaAsked = (componentMask & PICTURE_BUFFER_DESC_CHROMA_MASK) != 0;
    if (g_md_intra_state < 0 || !g_ctx || !md->intraMdOpenLoopFlag || size < 8 || size > 32 || lumaMode > 34 ||
        (chromaAsked && (componentMask & PICTURE_BUFFER_DESC_CHROMA_MASK) != PICTURE_BUFFER_DESC_CHROMA_MASK)) {
        COUNT_CPU(IntraPredictionOl);
        return __real_IntraPredictionOl(md, componentMask, pcs, cand);
    }
    EbPictureBufferDesc_t *in = pcs->ParentPcsPtr->enhancedPicturePtr, *pred = cand->predictionPtr;
    const uint32_t m = md->lcuPtr->size - 1;
    const int picLeft = md->lcuPtr->lcuEdgeInfoPtr->pictureLeftEdgeFlag == EB_TRUE && (ox & m) == 0;
    const int picTop = md->lcuPtr->lcuEdgeInfoPtr->pictureTopEdgeFlag == EB_TRUE && (oy & m) == 0;
    SvtAmdIntraPuJob j;
    memset(&j, 0, sizeof(j));
    j.size = size, j.bottom_left_ok = j.top_right_ok = 1, j.no_smoothing = 1, j.mode_tl = 2;
    memset(j.mode_left, 2, sizeof(j.mode_left)), memset(j.mode_top, 2, sizeof(j.mode_top));
    j.luma_mode = (uint8_t)lumaMode, j.chroma_mode = 4;
    if (componentMask & PICTURE_BUFFER_DESC_LUMA_MASK) {
        if (md->lumaIntraRefSamplesGenDone == EB_FALSE)
            GenerateIntraLumaReferenceSamplesMd(md, in);
        ol_slices(j.left[0], j.top[0], &j.tl[0], in->bufferY + (size_t)in->originY * in->strideY + in->originX, in->strideY, ox, oy, size,
                  in->width, in->height, picLeft, picTop);
        svt_hook_lock(&g_lock);
        if (svt_amd_intra_pu(g_ctx, 1, &j, pred->bufferY + (oy & 63) * 64 + (ox & 63), pred->strideY, NULL, NULL, 0))
            die("svt_amd_intra_pu (mode decision, open loop, luma)");
        if (g_md_intra_ol_gpu++ == 0 && g_verbose)
            fprintf(stderr, "svt_hook_me: open-loop mode-decision intra prediction (IntraPredictionOl) on the GPU\n");
        svt_hook_unlock(&g_lock);
    }
    if (chromaAsked) {
        if (md->chromaIntraRefSamplesGenDone == EB_FALSE)
            GenerateIntraChromaReferenceSamplesMd(md, in);
        ol_slices(j.left[1], j.top[1], &j.tl[1], in->bufferCb + (size_t)(in->originY >> 1) * in->strideCb + (in->originX >> 1), in->strideCb,
                  ox >> 1, oy >> 1, size >> 1, in->width >> 1, in->height >> 1, picLeft, picTop);
        ol_slices(j.left[2], j.top[2], &j.tl[2], in->bufferCr + (size_t)(in->originY >> 1) * in->strideCr + (in->originX >> 1), in->strideCr,
                  ox >> 1, oy >> 1, size >> 1, in->width >> 1, in->height >> 1, picLeft, picTop);
        const uint32_t o = (((oy & 63) * 32) + (ox & 63)) >> 1;
        svt_hook_lock(&g_lock);
        if (svt_amd_intra_pu(g_ctx, 1, &j, NULL, 0, pred->bufferCb + o, pred->bufferCr + o, pred->strideCb))
            die("svt_amd_intra_pu (mode decision, open loop, chroma)");
        g_md_intra_ol_gpu++;
        svt_hook_unlock(&g_lock);
    }
    return EB_ErrorNone;
}

/* The mode decision's intra 4x4 search: Intra4x4IntraPredictionCl (EbIntraPrediction.c:3993, called per candidate from
 * PerformIntra4x4Search, EbProductCodingLoop.c:2836) predicts a 4x4 luma partition and, with chroma in the loop, the coding unit's
 * chroma pair from the references Intra4x4InitFastLoop (:2543) built: luma size 4 at depth 3, no edge flags; chroma at the coding
 * unit.  Same switch, same jobs as the encode-pass 4x4 path. */
EB_ERRORTYPE __real_Intra4x4IntraPredictionCl(EB_U32 puIndex, EB_U32 puOriginX, EB_U32 puOriginY, EB_U32 puWidth, EB_U32 puHeight, EB_U32 lcuSize,
                                              EB_U32 componentMask, PictureControlSet_t *pcs, ModeDecisionCandidateBuffer_t *cand, EB_PTR ctx);
static unsigned long g_md_intra4_gpu;

EB_ERRORTYPE __wrap_Intra4x4IntraPredictionCl(EB_U32 puIndex, EB_U32 puOriginX, EB_U32 puOriginY, EB_U32 puWidth, EB_U32 puHeight, EB_U32 lcuSize,
                                              EB_U32 componentMask, PictureControlSet_t *pcs, ModeDecisionCandidateBuffer_t *cand, EB_PTR ctx)
{
    ModeDecisionContext_t *md = (ModeDecisionContext_t *)ctx;
    if (g_md_intra_state == 0)
        g_md_intra_state = getenv("SVT_HOOK_INTRA") ? 1 : -1;
    const uint32_t lumaMode = cand->candidatePtr->intraLumaMode;
    const int chromaAsked = (componentMask & PICTURE_BUFFER_DESC_CHROMA_MASK) != 0;
    if (g_md_intra_state < 0 || !g_ctx || puWidth != 4 || puHeight != 4 || lcuSize != 64 || md->intraMdOpenLoopFlag || lumaMode > 34 ||
        !(componentMask & PICTURE_BUFFER_DESC_LUMA_MASK) ||
        (chromaAsked && (componentMask & PICTURE_BUFFER_DESC_CHROMA_MASK) != PICTURE_BUFFER_DESC_CHROMA_MASK)) {
        COUNT_CPU(Intra4x4IntraPredictionCl);
        return __real_Intra4x4IntraPredictionCl(puIndex, puOriginX, puOriginY, puWidth, puHeight, lcuSize, componentMask, pcs, cand, ctx);
    }
    NeighborArrayUnit_t *na[3] = {md->lumaReconNeighborArray, md->cbReconNeighborArray, md->crReconNeighborArray};
    EbPictureBufferDesc_t *pred = cand->predictionPtr;
    SvtAmdIntraPuJob j;
    intra_slices(&j, 1, EB_FALSE, EB_TRUE, puOriginX, puOriginY, 4, 64, 3 + 1, md->modeTypeNeighborArray, na, 0, 1, EB_FALSE, EB_FALSE, EB_FALSE);
    j.luma_mode = (uint8_t)lumaMode, j.chroma_mode = 4;
    svt_hook_lock(&g_lock);
    if (svt_amd_intra_pu(g_ctx, 1, &j, pred->bufferY + ((puOriginY & 63) * pred->strideY) + (puOriginX & 63), pred->strideY, NULL, NULL, 0))
        die("svt_amd_intra_pu (mode decision, 4x4 luma)");
    if (chromaAsked) {
        intra_slices(&j, 1, EB_FALSE, EB_TRUE, md->cuOriginX, md->cuOriginY, 8, 64, md->cuDepth, md->modeTypeNeighborArray, na, 1, 3, EB_FALSE,
                     EB_FALSE, EB_FALSE);
        j.luma_mode = (uint8_t)lumaMode, j.chroma_mode = 4;
        const uint32_t oc = (((puOriginY & 63) * pred->strideCb) + (puOriginX & 63)) >> 1;
        if (svt_amd_intra_pu(g_ctx, 1, &j, NULL, 0, pred->bufferCb + oc, pred->bufferCr + oc, pred->strideCb))
            die("svt_amd_intra_pu (mode decision, 4x4 chroma)");
    }
    if (g_md_intra4_gpu++ == 0 && g_verbose)
        fprintf(stderr, "svt_hook_me: mode-decision intra 4x4 search prediction (Intra4x4IntraPredictionCl) on the GPU\n");
    svt_hook_unlock(&g_lock);
    return EB_ErrorNone;
}

/*
 * Encode-pass inter prediction: EncodePassInterPrediction (EbInterPrediction.c:761, called per prediction unit from
 * EbCodingLoop.c:3932) is answered by svt_amd_inter_pu_batch() with SVT_HOOK_INTER=1 (8-bit 4:2:0).  Reference pictures
 * stay resident in HBM: each (buffer, POC) pair is uploaded once, whole and padded, into a small cache of device copies.
 */
EB_ERRORTYPE __real_EncodePassInterPrediction(MvUnit_t *mvUnit, EB_U16 puOriginX, EB_U16 puOriginY, EB_U8 puWidth, EB_U8 puHeight,
                                              PictureControlSet_t *pcs, EbPictureBufferDesc_t *predictionPtr,
                                              MotionCompensationPredictionContext_t *mcpContext);
/* The cache grows instead of recycling a slot somebody still reads: a slot is PINNED from the lookup that hands it out until its user lets go (a per-unit binding: until
 * its device call has returned; a picture object of the device-resident encode pass: until the object moves on to another picture), and only unpinned slots are
 * candidates for eviction (least recently used first).  ADVICE r2 / VERDICT r3: with a fixed table of 16 the live reference set of deep hierarchies + several
 * pictures in flight could outgrow it, and the victim's device memory was freed or overwritten under kernels still reading it. */
#define REF_CACHE_STEP 16
struct RefSlot { const void *buf; uint64_t poc, used; void *d[3]; size_t bytes[3]; SvtAmdRefPicture pic; int from_device, pins; };
static struct RefSlot *g_refs;
static int REF_CACHE; /* slots allocated */
static struct RefSlot *ref_victim(void) /* under g_lock: the least recently used unpinned slot; a new one when every slot is in use */
{
    struct RefSlot *victim = NULL;
    for (int i = 0; i < REF_CACHE; i++)
        if (!g_refs[i].pins && (!victim || g_refs[i].used < victim->used))
            victim = &g_refs[i];
    if (victim)
        return victim;
    struct RefSlot *n = (struct RefSlot *)realloc(g_refs, sizeof(*g_refs) * (size_t)(REF_CACHE + REF_CACHE_STEP));
    if (!n)
        die("out of memory (reference cache)");
    memset(n + REF_CACHE, 0, sizeof(*n) * REF_CACHE_STEP);
    g_refs = n, REF_CACHE += REF_CACHE_STEP;
    return &g_refs[REF_CACHE - REF_CACHE_STEP];
}
/* under g_lock */
static void ref_unpin(int slot)
{
    if (slot >= 0 && slot < REF_CACHE && g_refs[slot].pins > 0)
        g_refs[slot].pins--;
}
void svt_hook_release_references(const int slot[2])
{
    svt_hook_lock(&g_lock);
    ref_unpin(slot[0]), ref_unpin(slot[1]);
    svt_hook_unlock(&g_lock);
}
static unsigned long g_ref_from_device, g_ref_dev_checked, g_ref_dev_mismatch;
static int g_ref_dev_verify = -1;
static uint64_t g_ref_clock;
static void *g_inter_scratch[3]; /* device prediction planes: 64x64, 32x32, 32x32 */
static unsigned long g_inter_gpu, g_inter_uploads;
static int g_inter_state;

/* Page-locks the planes of one of the encoder's pooled picture buffers (EbPictureBufferDescCtor / EbReconPictureBufferDescCtor allocate lumaSize / chromaSize
 * samples per plane, Codec/EbPictureBufferDesc.c:59-94, :149-166) for the life of the encoder: svt_amd_host_register remembers the range, a second call is a
 * lookup; hook_teardown releases them before EbDeinitEncoder frees the buffers.  SVT_HOOK_PIN_HOST=0 leaves the buffers pageable. */
/* Page-locking a buffer is a call into the driver that updates the device's address space: made while mode-decision kernels of other pictures are running it can
 * take hundreds of milliseconds, and the runtime's other calls queue behind it (profiles/r05_v: a picture's plane copies issued 720 ms apart).  The encoder's
 * picture pools are therefore pinned where they are BUILT (EbInitEncoder: svt_hook_pin_pool from the EbSystemResourceCtor binding), not where a picture first uses
 * one of their buffers; buffers built before the device context exists wait in a list that device start-up empties. */
static struct { const EbPictureBufferDesc_t *p; size_t bps; } g_pin_later[1024];
static int g_pin_later_n;
static pthread_mutex_t g_pin_lock = PTHREAD_MUTEX_INITIALIZER;
static unsigned long g_pinned_at_init;
static int pin_enabled(void)
{
    static int state; /* 0 unknown, 1 on, -1 off */
    if (!state) {
        const char *v = getenv("SVT_HOOK_PIN_HOST");
        state = (v && !strcmp(v, "0")) ? -1 : 1;
    }
    return state > 0;
}
static void pin_now(const EbPictureBufferDesc_t *p, size_t bps)
{
    if (p->bufferY)
        (void)svt_amd_host_register(g_ctx, p->bufferY, (size_t)p->lumaSize * bps);
    if (p->bufferCb)
        (void)svt_amd_host_register(g_ctx, p->bufferCb, (size_t)p->chromaSize * bps);
    if (p->bufferCr)
        (void)svt_amd_host_register(g_ctx, p->bufferCr, (size_t)p->chromaSize * bps);
}
void svt_hook_pin_picture(const EbPictureBufferDesc_t *p, size_t bps)
{
    if (!pin_enabled() || !g_ctx || !p)
        return;
    pin_now(p, bps);
}
/* at pool-construction time: now if the device is up, when it comes up otherwise */
void svt_hook_pin_picture_at_init(const EbPictureBufferDesc_t *p, size_t bps)
{
    if (!pin_enabled() || !p)
        return;
    pthread_mutex_lock(&g_pin_lock);
    if (g_ctx) {
        pin_now(p, bps);
        g_pinned_at_init++;
    } else if (g_pin_later_n < (int)(sizeof(g_pin_later) / sizeof(g_pin_later[0]))) {
        g_pin_later[g_pin_later_n].p = p, g_pin_later[g_pin_later_n].bps = bps;
        g_pin_later_n++;
    }
    pthread_mutex_unlock(&g_pin_lock);
}
static void pin_deferred(void) /* device start-up, g_ctx set */
{
    pthread_mutex_lock(&g_pin_lock);
    for (int i = 0; i < g_pin_later_n; i++)
        pin_now(g_pin_later[i].p, g_pin_later[i].bps), g_pinned_at_init++;
    g_pin_later_n = 0;
    pthread_mutex_unlock(&g_pin_lock);
}

/* must hold g_lock.  *slot = the cache slot, PINNED: the caller unpins it (ref_unpin / svt_hook_release_references) when it no longer reads the device copy */
static const SvtAmdRefPicture *resident_reference_via(SvtAmdContext *via, const EbPictureBufferDesc_t *p, uint64_t poc, size_t bps, int *slot);
static const SvtAmdRefPicture *resident_reference_bps(const EbPictureBufferDesc_t *p, uint64_t poc, size_t bps, int *slot) { return resident_reference_via(g_ctx, p, poc, bps, slot); }
static const SvtAmdRefPicture *resident_reference(const EbPictureBufferDesc_t *p, uint64_t poc, int *slot) { return resident_reference_bps(p, poc, 1, slot); }
/* via: the context whose stream carries an upload.  The root context's stream shares its hardware queue with whatever lane the runtime mapped there - an upload
 * behind another picture's 60 - 100 ms persistent kernel waits that long (profiles/r04_g_timeline_*.txt: 25 - 45 ms per device picture on average); a picture's own lane
 * is idle at this point. */
static const SvtAmdRefPicture *resident_reference_via(SvtAmdContext *via, const EbPictureBufferDesc_t *p, uint64_t poc, size_t bps, int *slot)
{
    for (int i = 0; i < REF_CACHE; i++) {
        if (g_refs[i].buf == p->bufferY && g_refs[i].poc == poc && g_refs[i].d[0]) {
            g_refs[i].used = ++g_ref_clock;
            g_refs[i].pins++, *slot = i;
            if (g_refs[i].from_device == 1) { /* produced on the device (svt_hook_register_device_reference): never uploaded.  The encoder has
                                               * finished its own copy by now; SVT_HOOK_ENCODEPASS_REFS=verify compares the two once */
                if (g_ref_dev_verify < 0) {
                    const char *v = getenv("SVT_HOOK_ENCODEPASS_REFS");
                    g_ref_dev_verify = v && !strcmp(v, "verify");
                }
                if (g_ref_dev_verify) {
                    const uint32_t rowsY = p->height + 2 * p->originY, rowsC = rowsY >> 1;
                    const size_t need[3] = {(size_t)rowsY * p->strideY * bps, (size_t)rowsC * p->strideCb * bps, (size_t)rowsC * p->strideCr * bps};
                    const uint8_t *src[3] = {p->bufferY, p->bufferCb, p->bufferCr};
                    int bad = 0;
                    for (int k = 0; k < 3; k++) {
                        uint8_t *tmp = (uint8_t *)malloc(need[k]);
                        if (!tmp || svt_amd_device_download(g_ctx, tmp, g_refs[i].d[k], need[k]))
                            die("svt_amd_device_download (reference verification)");
                        if (memcmp(tmp, src[k], need[k])) {
                            const uint32_t stride = k ? p->strideCb : p->strideY;
                            size_t first = 0, count = 0;
                            uint32_t x0 = ~0u, x1 = 0, y0 = ~0u, y1 = 0;
                            for (size_t o = 0; o < need[k] / bps; o++)
                                if (memcmp(tmp + o * bps, src[k] + o * bps, bps)) {
                                    const uint32_t x = (uint32_t)(o % stride), y = (uint32_t)(o / stride);
                                    if (!count++)
                                        first = o;
                                    x0 = x < x0 ? x : x0, x1 = x > x1 ? x : x1, y0 = y < y0 ? y : y0, y1 = y > y1 ? y : y1;
                                }
                            fprintf(stderr, "svt_hook_me: REFVERIFY poc %llu plane %d: %zu samples differ, first at (%zu,%zu), box x %u..%u y %u..%u (padded "
                                            "coordinates, origin %u,%u)\n", (unsigned long long)poc, k, count, first % stride, first / stride, x0, x1, y0, y1,
                                    k ? p->originX >> 1 : p->originX, k ? p->originY >> 1 : p->originY);
                            bad = 1;
                        }
                        free(tmp);
                    }
                    g_ref_dev_checked++, g_ref_dev_mismatch += bad;
                }
                g_refs[i].from_device = 2;
            }
            return &g_refs[i].pic;
        }
    }
    struct RefSlot *victim = ref_victim();
    const uint32_t rowsY = p->height + 2 * p->originY, rowsC = rowsY >> 1;
    const size_t need[3] = {(size_t)rowsY * p->strideY * bps, (size_t)rowsC * p->strideCb * bps, (size_t)rowsC * p->strideCr * bps};
    const uint8_t *src[3] = {p->bufferY, p->bufferCb, p->bufferCr};
    svt_hook_pin_picture(p, bps); /* the encoder's reference-picture pool is page-locked once: the upload is a DMA transfer, not a copy kernel */
    const double t_up = svt_hook_now();
    for (int k = 0; k < 3; k++) {
        if (victim->bytes[k] < need[k]) {
            if (victim->d[k] && svt_amd_device_free(g_ctx, victim->d[k]))
                die("svt_amd_device_free");
            if (svt_amd_device_alloc(g_ctx, need[k], &victim->d[k]))
                die("svt_amd_device_alloc");
            victim->bytes[k] = need[k];
        }
        if (svt_amd_device_upload(via, victim->d[k], src[k], need[k]))
            die("svt_amd_device_upload");
    }
    victim->buf = p->bufferY, victim->poc = poc, victim->used = ++g_ref_clock, victim->from_device = 0;
    victim->pic.d_y = victim->d[0], victim->pic.d_cb = victim->d[1], victim->pic.d_cr = victim->d[2];
    victim->pic.strideY = p->strideY, victim->pic.strideC = p->strideCb, victim->pic.originX = p->originX, victim->pic.originY = p->originY;
    victim->pic.width = p->width, victim->pic.height = p->height;
    victim->pins = 1, *slot = (int)(victim - g_refs);
    svt_hook_timeline("refupload", poc, (int)((need[0] + need[1] + need[2]) >> 20), 0, t_up, svt_hook_now());
    g_inter_uploads++;
    return &victim->pic;
}

/* for the device-resident encode pass (svt_hook_encdec.c): a reference picture the DEVICE finished (encode pass -> deblocking -> SAO ->
 * padding) enters the cache by a device-to-device copy; the encoder's own copy of it is never uploaded */
void svt_hook_register_device_reference(const EbPictureBufferDesc_t *p, uint64_t poc, size_t bps, const SvtAmdRefPicture *dev)
{
    if (dev->strideY != p->strideY || dev->strideC != p->strideCb || dev->originX != p->originX || dev->originY != p->originY)
        return; /* another padding geometry: the upload path serves it */
    svt_hook_lock(&g_lock);
    struct RefSlot *victim = NULL;
    for (int i = 0; i < REF_CACHE && !victim; i++)
        if (g_refs[i].buf == p->bufferY && g_refs[i].poc == poc && g_refs[i].d[0] && !g_refs[i].pins) /* (a pinned copy of this very buffer + POC is what it was: keep it) */
            victim = &g_refs[i];
    if (!victim) {
        /* a PINNED copy of this very buffer + POC (somebody still reads it) is superseded: it keeps its memory until its users let go, but no later lookup may match it
         * - the fresh copy below is the one */
        for (int i = 0; i < REF_CACHE; i++)
            if (g_refs[i].buf == p->bufferY && g_refs[i].poc == poc && g_refs[i].d[0])
                g_refs[i].buf = NULL;
        victim = ref_victim();
    }
    const uint32_t rowsY = p->height + 2 * p->originY, rowsC = rowsY >> 1;
    const size_t need[3] = {(size_t)rowsY * p->strideY * bps, (size_t)rowsC * p->strideCb * bps, (size_t)rowsC * p->strideCr * bps};
    const void *src[3] = {dev->d_y, dev->d_cb, dev->d_cr};
    for (int k = 0; k < 3; k++) {
        if (victim->bytes[k] < need[k]) {
            if (victim->d[k] && svt_amd_device_free(g_ctx, victim->d[k]))
                die("svt_amd_device_free");
            if (svt_amd_device_alloc(g_ctx, need[k], &victim->d[k]))
                die("svt_amd_device_alloc");
            victim->bytes[k] = need[k];
        }
        if (svt_amd_device_copy(g_ctx, victim->d[k], src[k], need[k]))
            die("svt_amd_device_copy");
    }
    victim->buf = p->bufferY, victim->poc = poc, victim->used = ++g_ref_clock, victim->from_device = 1;
    victim->pic.d_y = victim->d[0], victim->pic.d_cb = victim->d[1], victim->pic.d_cr = victim->d[2];
    victim->pic.strideY = p->strideY, victim->pic.strideC = p->strideCb, victim->pic.originX = p->originX, victim->pic.originY = p->originY;
    victim->pic.width = p->width, victim->pic.height = p->height;
    g_ref_from_device++;
    svt_hook_unlock(&g_lock);
}
void svt_hook_reference_report(FILE *out)
{
    if (g_ref_from_device)
        fprintf(out, "svt_hook_me: %lu reference pictures finished on the device (encode pass -> deblocking -> SAO -> padding) and never uploaded; %lu "
                     "compared with the encoder's own, %lu differ\n", g_ref_from_device, g_ref_dev_checked, g_ref_dev_mismatch);
}

/* for the device-resident encode pass (svt_hook_encdec.c): the reference pictures of both lists as device copies */
void svt_hook_resident_references(SvtAmdContext *lane, const PictureControlSet_t *pcs, int wide, SvtAmdRefPicture out[2], int have[2], int slot[2])
{
    svt_hook_lock(&g_lock);
    for (int l = 0; l < 2; l++) {
        have[l] = l == 0 ? pcs->sliceType != EB_I_PICTURE : pcs->sliceType == EB_B_PICTURE;
        slot[l] = -1;
        if (!have[l])
            continue;
        const EbReferenceObject_t *ro = (const EbReferenceObject_t *)pcs->refPicPtrArray[l]->objectPtr;
        out[l] = *resident_reference_via(lane ? lane : g_ctx, wide ? ro->referencePicture16bit : ro->referencePicture, ro->refPOC, wide ? 2 : 1, &slot[l]); /* pinned: svt_hook_release_references */
    }
    svt_hook_unlock(&g_lock);
}

EB_ERRORTYPE __wrap_EncodePassInterPrediction(MvUnit_t *mvUnit, EB_U16 puOriginX, EB_U16 puOriginY, EB_U8 puWidth, EB_U8 puHeight,
                                              PictureControlSet_t *pcs, EbPictureBufferDesc_t *predictionPtr,
                                              MotionCompensationPredictionContext_t *mcpContext)
{
    if (svt_hook_ep_active) /* the device encoded this LCU: the reconstruction table slot brings the samples */
        return EB_ErrorNone;
    if (g_inter_state == 0)
        g_inter_state = getenv("SVT_HOOK_INTER") ? 1 : -1;
    if (g_inter_state < 0 || !g_ctx || predictionPtr->colorFormat != EB_YUV420 || puWidth < 8 || puHeight < 8 || puWidth > 64 ||
        puHeight > 64 || mvUnit->predDirection > BI_PRED || predictionPtr->strideCb != predictionPtr->strideCr) {
        COUNT_CPU(EncodePassInterPrediction);
        return __real_EncodePassInterPrediction(mvUnit, puOriginX, puOriginY, puWidth, puHeight, pcs, predictionPtr, mcpContext);
    }
    SvtAmdInterPuJob job;
    memset(&job, 0, sizeof(job));
    job.pu_x = puOriginX, job.pu_y = puOriginY, job.pu_w = puWidth, job.pu_h = puHeight, job.pred_dir = mvUnit->predDirection;
    svt_hook_lock(&g_lock);
    const SvtAmdRefPicture *refs[2] = {NULL, NULL};
    SvtAmdRefPicture copy[2];
    int pin[2] = {-1, -1};
    for (int l = 0; l < 2; l++) {
        job.mv[l][0] = mvUnit->mv[l].x, job.mv[l][1] = mvUnit->mv[l].y;
        if (mvUnit->predDirection == l || mvUnit->predDirection == BI_PRED) {
            const EbReferenceObject_t *ro = (const EbReferenceObject_t *)pcs->refPicPtrArray[l]->objectPtr;
            copy[l] = *resident_reference(ro->referencePicture, ro->refPOC, &pin[l]); /* pinned until the unit's samples are back: the other list's lookup cannot recycle it */
            refs[l] = &copy[l];
        }
    }
    if (!g_inter_scratch[0])
        for (int k = 0; k < 3; k++)
            if (svt_amd_device_alloc(g_ctx, k ? 1024 : 4096, &g_inter_scratch[k]))
                die("svt_amd_device_alloc");
    if (svt_amd_inter_pu_batch(g_ctx, &job, 1, refs[0], refs[1], (uint8_t *)g_inter_scratch[0], puWidth, (uint8_t *)g_inter_scratch[1],
                               (uint8_t *)g_inter_scratch[2], puWidth >> 1))
        die("svt_amd_inter_pu_batch");
    uint8_t hy[4096], hcb[1024], hcr[1024];
    if (svt_amd_device_download(g_ctx, hy, g_inter_scratch[0], (size_t)puWidth * puHeight) ||
        svt_amd_device_download(g_ctx, hcb, g_inter_scratch[1], (size_t)puWidth * puHeight / 4) ||
        svt_amd_device_download(g_ctx, hcr, g_inter_scratch[2], (size_t)puWidth * puHeight / 4))
        die("svt_amd_device_download");
    if (g_inter_gpu++ == 0 && g_verbose)
        fprintf(stderr, "svt_hook_me: encode-pass inter prediction (EncodePassInterPrediction) on the GPU\n");
    ref_unpin(pin[0]), ref_unpin(pin[1]); /* the samples are back (the downloads above are blocking) */
    svt_hook_unlock(&g_lock);
    const uint32_t oy = (predictionPtr->originY + puOriginY) * predictionPtr->strideY + predictionPtr->originX + puOriginX;
    const uint32_t oc = (((predictionPtr->originY + puOriginY) * predictionPtr->strideCb) >> 1) + ((predictionPtr->originX + puOriginX) >> 1);
    for (uint32_t y = 0; y < puHeight; y++)
        memcpy(predictionPtr->bufferY + oy + y * predictionPtr->strideY, hy + y * puWidth, puWidth);
    for (uint32_t y = 0; y < (uint32_t)(puHeight >> 1); y++) {
        memcpy(predictionPtr->bufferCb + oc + y * predictionPtr->strideCb, hcb + y * (puWidth >> 1), puWidth >> 1);
        memcpy(predictionPtr->bufferCr + oc + y * predictionPtr->strideCr, hcr + y * (puWidth >> 1), puWidth >> 1);
    }
    return EB_ErrorNone;
}

/* The 16-bit twin (10-bit encodes): EncodePassInterPrediction16bit (EbInterPrediction.c:928) reads referencePicture16bit and
 * writes 16-bit samples; same switch, same cache (keyed by buffer address), svt_amd_inter_pu_batch16bit. */
EB_ERRORTYPE __real_EncodePassInterPrediction16bit(MvUnit_t *mvUnit, EB_U16 puOriginX, EB_U16 puOriginY, EB_U8 puWidth, EB_U8 puHeight,
                                                   PictureControlSet_t *pcs, EbPictureBufferDesc_t *predictionPtr,
                                                   MotionCompensationPredictionContext_t *mcpContext);
static void *g_inter16_scratch[3];
static unsigned long g_inter16_gpu;

EB_ERRORTYPE __wrap_EncodePassInterPrediction16bit(MvUnit_t *mvUnit, EB_U16 puOriginX, EB_U16 puOriginY, EB_U8 puWidth, EB_U8 puHeight,
                                                   PictureControlSet_t *pcs, EbPictureBufferDesc_t *predictionPtr,
                                                   MotionCompensationPredictionContext_t *mcpContext)
{
    if (svt_hook_ep_active)
        return EB_ErrorNone;
    if (g_inter_state == 0)
        g_inter_state = getenv("SVT_HOOK_INTER") ? 1 : -1;
    if (g_inter_state < 0 || !g_ctx || predictionPtr->colorFormat != EB_YUV420 || puWidth < 8 || puHeight < 8 || puWidth > 64 ||
        puHeight > 64 || mvUnit->predDirection > BI_PRED || predictionPtr->strideCb != predictionPtr->strideCr) {
        COUNT_CPU(EncodePassInterPrediction16bit);
        return __real_EncodePassInterPrediction16bit(mvUnit, puOriginX, puOriginY, puWidth, puHeight, pcs, predictionPtr, mcpContext);
    }
    SvtAmdInterPuJob job;
    memset(&job, 0, sizeof(job));
    job.pu_x = puOriginX, job.pu_y = puOriginY, job.pu_w = puWidth, job.pu_h = puHeight, job.pred_dir = mvUnit->predDirection;
    svt_hook_lock(&g_lock);
    const SvtAmdRefPicture *refs[2] = {NULL, NULL};
    SvtAmdRefPicture copy[2];
    int pin[2] = {-1, -1};
    for (int l = 0; l < 2; l++) {
        job.mv[l][0] = mvUnit->mv[l].x, job.mv[l][1] = mvUnit->mv[l].y;
        if (mvUnit->predDirection == l || mvUnit->predDirection == BI_PRED) {
            const EbReferenceObject_t *ro = (const EbReferenceObject_t *)pcs->refPicPtrArray[l]->objectPtr;
            copy[l] = *resident_reference_bps(ro->referencePicture16bit, ro->refPOC, 2, &pin[l]);
            refs[l] = &copy[l];
        }
    }
    if (!g_inter16_scratch[0])
        for (int k = 0; k < 3; k++)
            if (svt_amd_device_alloc(g_ctx, k ? 2048 : 8192, &g_inter16_scratch[k]))
                die("svt_amd_device_alloc");
    if (svt_amd_inter_pu_batch16bit(g_ctx, &job, 1, refs[0], refs[1], (uint16_t *)g_inter16_scratch[0], puWidth,
                                    (uint16_t *)g_inter16_scratch[1], (uint16_t *)g_inter16_scratch[2], puWidth >> 1))
        die("svt_amd_inter_pu_batch16bit");
    uint16_t hy[4096], hcb[1024], hcr[1024];
    if (svt_amd_device_download(g_ctx, hy, g_inter16_scratch[0], (size_t)puWidth * puHeight * 2) ||
        svt_amd_device_download(g_ctx, hcb, g_inter16_scratch[1], (size_t)puWidth * puHeight / 2) ||
        svt_amd_device_download(g_ctx, hcr, g_inter16_scratch[2], (size_t)puWidth * puHeight / 2))
        die("svt_amd_device_download");
    if (g_inter16_gpu++ == 0 && g_verbose)
        fprintf(stderr, "svt_hook_me: encode-pass inter prediction (EncodePassInterPrediction16bit) on the GPU\n");
    ref_unpin(pin[0]), ref_unpin(pin[1]); /* the samples are back (the downloads above are blocking) */
    svt_hook_unlock(&g_lock);
    const uint32_t oy = (predictionPtr->originY + puOriginY) * predictionPtr->strideY + predictionPtr->originX + puOriginX;
    const uint32_t oc = (((predictionPtr->originY + puOriginY) * predictionPtr->strideCb) >> 1) + ((predictionPtr->originX + puOriginX) >> 1);
    uint16_t *py = (uint16_t *)predictionPtr->bufferY, *pcb = (uint16_t *)predictionPtr->bufferCb, *pcr = (uint16_t *)predictionPtr->bufferCr;
    for (uint32_t y = 0; y < puHeight; y++)
        memcpy(py + oy + y * predictionPtr->strideY, hy + y * puWidth, 2 * (size_t)puWidth);
    for (uint32_t y = 0; y < (uint32_t)(puHeight >> 1); y++) {
        memcpy(pcb + oc + y * predictionPtr->strideCb, hcb + y * (puWidth >> 1), puWidth);
        memcpy(pcr + oc + y * predictionPtr->strideCr, hcr + y * (puWidth >> 1), puWidth);
    }
    return EB_ErrorNone;
}

/*
 * Mode-decision inter prediction: Inter2Nx2NPuPredictionHevc (EbInterPrediction.c:469; entries of the prediction tables
 * PredictionFunTableOl / Cl, EbProductCodingLoop.c:218-230) does the same clamp + interpolation as the encode-pass
 * function, for the candidate's vectors, into the candidate's LCU-local prediction buffer (64-sample pitch) and for the
 * planes of componentMask.  Same switch and the same resident reference pictures as above; 8-bit encoders only.
 */
EB_ERRORTYPE __real_Inter2Nx2NPuPredictionHevc(ModeDecisionContext_t *mdContextPtr, EB_U32 componentMask, PictureControlSet_t *pcs,
                                               ModeDecisionCandidateBuffer_t *candidateBufferPtr);
static unsigned long g_md_inter_gpu;

EB_ERRORTYPE __wrap_Inter2Nx2NPuPredictionHevc(ModeDecisionContext_t *mdContextPtr, EB_U32 componentMask, PictureControlSet_t *pcs,
                                               ModeDecisionCandidateBuffer_t *candidateBufferPtr)
{
    if (g_inter_state == 0)
        g_inter_state = getenv("SVT_HOOK_INTER") ? 1 : -1;
    const SequenceControlSet_t *scs = (const SequenceControlSet_t *)pcs->sequenceControlSetWrapperPtr->objectPtr;
    const ModeDecisionCandidate_t *c = candidateBufferPtr->candidatePtr;
    const EB_U32 size = mdContextPtr->cuStats->size, dir = c->predictionDirection[mdContextPtr->puItr];
    EbPictureBufferDesc_t *dst = candidateBufferPtr->predictionPtr;
    const int msb = scs->staticConfig.encoderBitDepth > EB_8BIT; /* 10-bit encode: 8-bit prediction from the MSBs of the 16-bit references */
    if (g_inter_state < 0 || !g_ctx || mdContextPtr->cuUseRefSrcFlag || size < 8 || size > 64 ||
        dir > BI_PRED || dst->strideY != 64 || dst->strideCb != 32 || dst->strideCr != 32) {
        COUNT_CPU(Inter2Nx2NPuPredictionHevc);
        return __real_Inter2Nx2NPuPredictionHevc(mdContextPtr, componentMask, pcs, candidateBufferPtr);
    }
    SvtAmdInterPuJob job;
    memset(&job, 0, sizeof(job));
    job.pu_x = (uint16_t)mdContextPtr->cuOriginX, job.pu_y = (uint16_t)mdContextPtr->cuOriginY, job.pu_w = job.pu_h = (uint8_t)size;
    job.pred_dir = (uint8_t)dir;
    job.mv[0][0] = c->motionVector_x_L0, job.mv[0][1] = c->motionVector_y_L0, job.mv[1][0] = c->motionVector_x_L1, job.mv[1][1] = c->motionVector_y_L1;
    svt_hook_lock(&g_lock);
    const SvtAmdRefPicture *refs[2] = {NULL, NULL};
    SvtAmdRefPicture copy[2];
    int pin[2] = {-1, -1};
    for (int l = 0; l < 2; l++)
        if (dir == (EB_U32)l || dir == BI_PRED) {
            const EbReferenceObject_t *ro = (const EbReferenceObject_t *)pcs->refPicPtrArray[l]->objectPtr;
            copy[l] = msb ? *resident_reference_bps(ro->referencePicture16bit, ro->refPOC, 2, &pin[l]) : *resident_reference(ro->referencePicture, ro->refPOC, &pin[l]);
            refs[l] = &copy[l];
        }
    if (!g_inter_scratch[0])
        for (int k = 0; k < 3; k++)
            if (svt_amd_device_alloc(g_ctx, k ? 1024 : 4096, &g_inter_scratch[k]))
                die("svt_amd_device_alloc");
    if ((msb ? svt_amd_inter_pu_batch_msb : svt_amd_inter_pu_batch)(g_ctx, &job, 1, refs[0], refs[1], (uint8_t *)g_inter_scratch[0], size,
                                                                   (uint8_t *)g_inter_scratch[1], (uint8_t *)g_inter_scratch[2], size >> 1))
        die("svt_amd_inter_pu_batch");
    uint8_t hy[4096], hcb[1024], hcr[1024];
    if (((componentMask & PICTURE_BUFFER_DESC_LUMA_MASK) && svt_amd_device_download(g_ctx, hy, g_inter_scratch[0], (size_t)size * size)) ||
        ((componentMask & PICTURE_BUFFER_DESC_CHROMA_MASK) && (svt_amd_device_download(g_ctx, hcb, g_inter_scratch[1], (size_t)size * size / 4) ||
                                                               svt_amd_device_download(g_ctx, hcr, g_inter_scratch[2], (size_t)size * size / 4))))
        die("svt_amd_device_download");
    if (g_md_inter_gpu++ == 0 && g_verbose)
        fprintf(stderr, "svt_hook_me: mode-decision inter prediction (Inter2Nx2NPuPredictionHevc) on the GPU\n");
    ref_unpin(pin[0]), ref_unpin(pin[1]); /* the samples are back (the downloads above are blocking) */
    svt_hook_unlock(&g_lock);
    const uint32_t oy = ((mdContextPtr->cuOriginY & 63) * 64) + (mdContextPtr->cuOriginX & 63);
    const uint32_t oc = ((((mdContextPtr->cuOriginY & 63) * 32) + (mdContextPtr->cuOriginX & 63)) >> 1);
    if (componentMask & PICTURE_BUFFER_DESC_LUMA_MASK)
        for (uint32_t y = 0; y < size; y++)
            memcpy(dst->bufferY + oy + y * 64, hy + y * size, size);
    if (componentMask & PICTURE_BUFFER_DESC_CHROMA_MASK)
        for (uint32_t y = 0; y < size / 2; y++) {
            memcpy(dst->bufferCb + oc + y * 32, hcb + y * (size / 2), size / 2);
            memcpy(dst->bufferCr + oc + y * 32, hcr + y * (size / 2), size / 2);
        }
    return EB_ErrorNone;
}

/*
 * Final encode pass, quantiser: UnifiedQuantizeInvQuantize (EbTransforms.c:2978, called from the static EncodeLoop /
 * EncodeLoop16bit) is answered by svt_amd_unified_quantize() with SVT_HOOK_QUANT=1 on its paths without RDOQ / PM-core and
 * without perceptual masking (everything the default configuration reaches); other calls go to the reference code.
 */
void __real_UnifiedQuantizeInvQuantize(EncDecContext_t *contextPtr, PictureControlSet_t *pcs, EB_S16 *coeff, const EB_U32 coeffStride,
                                       EB_S16 *quantCoeff, EB_S16 *reconCoeff, EB_U32 qp, EB_U32 bitDepth, EB_U32 areaSize,
                                       EB_PICTURE sliceType, EB_U32 *yCountNonZeroCoeffs, EB_U8 transCoeffShape,
                                       EB_U8 cleanSparseCeoffPfEncDec, EB_U8 pmpMaskingLevelEncDec, EB_MODETYPE type, EB_U32 enableCbflag,
                                       EB_U8 enableContouringQCUpdateFlag, EB_U32 componentType, EB_U32 temporalLayerIndex,
                                       EB_U32 dZoffset, CabacEncodeContext_t *cabacEncodeCtxPtr, EB_U64 lambda, EB_U32 intraLumaMode,
                                       EB_U32 intraChromaMode, CabacCost_t *CabacCost);
static unsigned long g_quant_gpu, g_quant_pm_gpu;
static int g_quant_state;

void __wrap_UnifiedQuantizeInvQuantize(EncDecContext_t *contextPtr, PictureControlSet_t *pcs, EB_S16 *coeff, const EB_U32 coeffStride,
                                       EB_S16 *quantCoeff, EB_S16 *reconCoeff, EB_U32 qp, EB_U32 bitDepth, EB_U32 areaSize,
                                       EB_PICTURE sliceType, EB_U32 *yCountNonZeroCoeffs, EB_U8 transCoeffShape,
                                       EB_U8 cleanSparseCeoffPfEncDec, EB_U8 pmpMaskingLevelEncDec, EB_MODETYPE type, EB_U32 enableCbflag,
                                       EB_U8 enableContouringQCUpdateFlag, EB_U32 componentType, EB_U32 temporalLayerIndex,
                                       EB_U32 dZoffset, CabacEncodeContext_t *cabacEncodeCtxPtr, EB_U64 lambda, EB_U32 intraLumaMode,
                                       EB_U32 intraChromaMode, CabacCost_t *CabacCost)
{
    if (svt_hook_ep_active) {
        svt_hook_ep_quantize(contextPtr, quantCoeff, reconCoeff, coeffStride, qp, areaSize, yCountNonZeroCoeffs, transCoeffShape,
                             cleanSparseCeoffPfEncDec, pmpMaskingLevelEncDec, enableCbflag, enableContouringQCUpdateFlag, dZoffset);
        return;
    }
    if (g_quant_state == 0)
        g_quant_state = getenv("SVT_HOOK_QUANT") ? 1 : -1;
    if (g_quant_state > 0 && g_ctx && contextPtr->mdContext->rdoqPmCoreMethod == EB_PMCORE && yCountNonZeroCoeffs && areaSize <= 32 &&
        areaSize >= 4 && qp <= 51 && (bitDepth == 8 || bitDepth == 10) && lambda <= 0xffffffffu) {
        /* encMode 1..4: the PM-core variant (EbTransforms.c:3009-3052) */
        SvtAmdPmQuantUnit pu;
        memset(&pu, 0, sizeof(pu));
        pu.size = (uint8_t)areaSize, pu.qp = (uint8_t)qp, pu.bit_depth = (uint8_t)bitDepth, pu.slice_type = (uint8_t)sliceType;
        pu.component = (uint8_t)componentType, pu.cand_type = (uint8_t)type, pu.lambda = (uint32_t)lambda;
        uint32_t pnz = 0;
        svt_hook_lock(&g_lock);
        if (svt_amd_pmcore_quantize(g_ctx, (const SvtAmdCabacCost *)CabacCost, &pu, coeff, coeffStride, quantCoeff, reconCoeff, &pnz))
            die("svt_amd_pmcore_quantize");
        if (g_quant_pm_gpu++ == 0 && g_verbose)
            fprintf(stderr, "svt_hook_me: encode-pass PM-core quantiser (UnifiedQuantizeInvQuantize, EB_PMCORE) on the GPU\n");
        svt_hook_unlock(&g_lock);
        *yCountNonZeroCoeffs = pnz;
        return;
    }
    if (g_quant_state < 0 || !g_ctx || contextPtr->mdContext->rdoqPmCoreMethod || pmpMaskingLevelEncDec || !yCountNonZeroCoeffs ||
        areaSize > 32 || areaSize < 4 || qp > 51 || (bitDepth != 8 && bitDepth != 10)) {
        __real_UnifiedQuantizeInvQuantize(contextPtr, pcs, coeff, coeffStride, quantCoeff, reconCoeff, qp, bitDepth, areaSize, sliceType,
                                          yCountNonZeroCoeffs, transCoeffShape, cleanSparseCeoffPfEncDec, pmpMaskingLevelEncDec, type,
                                          enableCbflag, enableContouringQCUpdateFlag, componentType, temporalLayerIndex, dZoffset,
                                          cabacEncodeCtxPtr, lambda, intraLumaMode, intraChromaMode, CabacCost);
        return;
    }
    SvtAmdQuantUnit u;
    memset(&u, 0, sizeof(u));
    u.size = (uint8_t)areaSize, u.qp = (uint8_t)qp, u.bit_depth = (uint8_t)bitDepth, u.slice_type = (uint8_t)sliceType;
    u.shape = transCoeffShape, u.clean_sparse = cleanSparseCeoffPfEncDec, u.enable_cb_flag = (uint8_t)enableCbflag;
    u.contouring_flag = enableContouringQCUpdateFlag, u.component = (uint8_t)componentType, u.temporal_layer = (uint8_t)temporalLayerIndex;
    u.dz_offset = dZoffset;
    svt_hook_lock(&g_lock);
    uint32_t nz = 0;
    if (svt_amd_unified_quantize(g_ctx, &u, coeff, coeffStride, quantCoeff, reconCoeff, &nz))
        die("svt_amd_unified_quantize");
    if (g_quant_gpu++ == 0 && g_verbose)
        fprintf(stderr, "svt_hook_me: encode-pass quantiser (UnifiedQuantizeInvQuantize) on the GPU\n");
    svt_hook_unlock(&g_lock);
    *yCountNonZeroCoeffs = nz;
}

/* ---- SAO statistics + parameter decision of an LCU -------------------------------------------------------------------------
 * SaoGenerationDecision / SaoGenerationDecision16bit (Codec/EbSampleAdaptiveOffsetGenerationDecision.c:647, :936; called per
 * LCU from EbCodingLoop.c:4711, :4732) are answered, with SVT_HOOK_SAO=1, by the device: the statistics by the library's
 * gather entry points on the same sample windows, the decision by svt_amd_sao_decide_lcu() with the neighbours' parameters.
 */
EB_ERRORTYPE __real_SaoGenerationDecision(SaoStats_t *saoStats, SaoParameters_t *saoParams, MdRateEstimationContext_t *md, EB_U64 fullLambda,
                                          EB_U64 fullChromaLambdaSao, EB_BOOL mmSao, PictureControlSet_t *pcs, EB_U32 tbOriginX,
                                          EB_U32 tbOriginY, EB_U32 lcuWidth, EB_U32 lcuHeight, SaoParameters_t *saoPtr,
                                          SaoParameters_t *leftSaoPtr, SaoParameters_t *upSaoPtr, EB_S64 *saoLumaBestCost,
                                          EB_S64 *saoChromaBestCost);
EB_ERRORTYPE __real_SaoGenerationDecision16bit(EbPictureBufferDesc_t *inputLcuPtr, SaoStats_t *saoStats, SaoParameters_t *saoParams,
                                               MdRateEstimationContext_t *md, EB_U64 fullLambda, EB_U64 fullChromaLambdaSao, EB_BOOL mmSao,
                                               PictureControlSet_t *pcs, EB_U32 tbOriginX, EB_U32 tbOriginY, EB_U32 lcuWidth,
                                               EB_U32 lcuHeight, SaoParameters_t *saoPtr, SaoParameters_t *leftSaoPtr,
                                               SaoParameters_t *upSaoPtr, EB_S64 *saoLumaBestCost, EB_S64 *saoChromaBestCost);
static unsigned long g_sao_gpu;
static int g_sao_state;

static void sao_params_in(SvtAmdSaoLcuParams *d, const SaoParameters_t *s)
{
    memset(d, 0, sizeof(*d));
    d->merge_left = s->saoMergeLeftFlag, d->merge_up = s->saoMergeUpFlag;
    d->type[0] = s->saoTypeIndex[0], d->type[1] = s->saoTypeIndex[1];
    memcpy(d->offset, s->saoOffset, sizeof(d->offset));
    memcpy(d->band, s->saoBandPosition, sizeof(d->band));
}

/* in8 / in16: the three input planes' first sample of this LCU and their strides; same for the reconstruction */
static void sao_on_device(int is16, void *const in[3], const uint32_t inStride[3], void *const rec[3], const uint32_t recStride[3],
                          SaoStats_t *saoStats, MdRateEstimationContext_t *md, EB_U64 fullLambda, EB_U64 fullChromaLambdaSao, EB_BOOL mmSao,
                          PictureControlSet_t *pcs, EB_U32 lcuWidth, EB_U32 lcuHeight, SaoParameters_t *saoPtr, SaoParameters_t *leftSaoPtr,
                          SaoParameters_t *upSaoPtr, EB_S64 *saoLumaBestCost, EB_S64 *saoChromaBestCost)
{
    SvtAmdSaoStats st[3];
    SvtAmdSaoDecisionParams P;
    SvtAmdSaoLcuParams left, up, out;
    int64_t costs[2] = {0, 0};
    memset(st, 0, sizeof(st)), memset(&P, 0, sizeof(P)), memset(&out, 0, sizeof(out));
    P.lambda = fullLambda, P.chroma_lambda = fullChromaLambdaSao;
    for (int k = 0; k < 6; k++)
        P.type_bits[k] = md->saoTypeIndexBits[k];
    for (int k = 0; k < 2; k++)
        P.merge_bits[k] = md->saoMergeFlagBits[k];
    for (int k = 0; k < 8; k++)
        P.offset_bits[k] = md->saoOffsetTrunUnaryBits[k];
    P.is_10bit = (uint8_t)is16, P.mm_sao = mmSao ? 1 : 0, P.temporal_layer = pcs->temporalLayerIndex;
    svt_hook_lock(&g_lock);
    const int ncomp = mmSao ? 3 : (pcs->temporalLayerIndex < 2 ? 1 : 0);
    for (int c = 0; c < ncomp; c++) {
        const uint32_t w = c ? lcuWidth >> 1 : lcuWidth, h = c ? lcuHeight >> 1 : lcuHeight;
        int rc;
        if (mmSao)
            rc = is16 ? svt_amd_GatherSaoStatisticsLcu_62x62_16bit((uint16_t *)in[c], inStride[c], (uint16_t *)rec[c], recStride[c], w, h,
                                                                   st[c].boDiff, st[c].boCount, st[c].eoDiff, st[c].eoCount)
                      : svt_amd_GatherSaoStatisticsLcuLossy_62x62((uint8_t *)in[c], inStride[c], (uint8_t *)rec[c], recStride[c], w, h,
                                                                  st[c].boDiff, st[c].boCount, st[c].eoDiff, st[c].eoCount);
        else
            rc = is16 ? svt_amd_GatherSaoStatisticsLcu_62x62_OnlyEo_90_45_135_16bit((uint16_t *)in[c], inStride[c], (uint16_t *)rec[c],
                                                                                    recStride[c], w, h, st[c].eoDiff, st[c].eoCount)
                      : svt_amd_GatherSaoStatisticsLcu_OnlyEo_90_45_135_Lossy((uint8_t *)in[c], inStride[c], (uint8_t *)rec[c],
                                                                              recStride[c], w, h, st[c].eoDiff, st[c].eoCount);
        if (rc)
            die("svt_amd_GatherSaoStatistics*");
        memcpy(saoStats->eoDiff[c], st[c].eoDiff, sizeof(st[c].eoDiff));
        memcpy(saoStats->eoCount[c], st[c].eoCount, sizeof(st[c].eoCount));
        if (mmSao) {
            memcpy(saoStats->boDiff[c], st[c].boDiff, sizeof(st[c].boDiff));
            memcpy(saoStats->boCount[c], st[c].boCount, sizeof(st[c].boCount));
        }
    }
    if (leftSaoPtr)
        sao_params_in(&left, leftSaoPtr);
    if (upSaoPtr)
        sao_params_in(&up, upSaoPtr);
    if (svt_amd_sao_decide_lcu(g_ctx, &P, &st[0], &st[1], &st[2], leftSaoPtr ? &left : NULL, upSaoPtr ? &up : NULL, &out, costs))
        die("svt_amd_sao_decide_lcu");
    if (g_sao_gpu++ == 0 && g_verbose)
        fprintf(stderr, "svt_hook_me: SAO statistics + decision (SaoGenerationDecision%s) on the GPU\n", is16 ? "16bit" : "");
    svt_hook_unlock(&g_lock);
    saoPtr->saoMergeLeftFlag = out.merge_left, saoPtr->saoMergeUpFlag = out.merge_up;
    saoPtr->saoTypeIndex[0] = out.type[0], saoPtr->saoTypeIndex[1] = out.type[1];
    memcpy(saoPtr->saoOffset, out.offset, sizeof(out.offset));
    memcpy(saoPtr->saoBandPosition, out.band, sizeof(out.band));
    *saoLumaBestCost = costs[0], *saoChromaBestCost = costs[1];
}

EB_ERRORTYPE __wrap_SaoGenerationDecision(SaoStats_t *saoStats, SaoParameters_t *saoParams, MdRateEstimationContext_t *md, EB_U64 fullLambda,
                                          EB_U64 fullChromaLambdaSao, EB_BOOL mmSao, PictureControlSet_t *pcs, EB_U32 tbOriginX,
                                          EB_U32 tbOriginY, EB_U32 lcuWidth, EB_U32 lcuHeight, SaoParameters_t *saoPtr,
                                          SaoParameters_t *leftSaoPtr, SaoParameters_t *upSaoPtr, EB_S64 *saoLumaBestCost,
                                          EB_S64 *saoChromaBestCost)
{
    if (svt_hook_ep_active)
        svt_hook_ep_note_sao(pcs, tbOriginX, tbOriginY, md, fullLambda, fullChromaLambdaSao, mmSao, 0);
    if (g_sao_state == 0)
        g_sao_state = getenv("SVT_HOOK_SAO") ? 1 : -1;
    const EbPictureBufferDesc_t *in = pcs->ParentPcsPtr->enhancedPicturePtr;
    const EbPictureBufferDesc_t *rec = pcs->ParentPcsPtr->isUsedAsReferenceFlag == EB_TRUE
        ? ((EbReferenceObject_t *)pcs->ParentPcsPtr->referencePictureWrapperPtr->objectPtr)->referencePicture : pcs->reconPicturePtr;
    if (g_sao_state < 0 || !g_ctx || saoParams != saoPtr || rec->colorFormat != EB_YUV420) {
        COUNT_CPU(SaoGenerationDecision);
        return __real_SaoGenerationDecision(saoStats, saoParams, md, fullLambda, fullChromaLambdaSao, mmSao, pcs, tbOriginX, tbOriginY,
                                            lcuWidth, lcuHeight, saoPtr, leftSaoPtr, upSaoPtr, saoLumaBestCost, saoChromaBestCost);
    }
    void *ip[3] = {in->bufferY + (in->originY + tbOriginY) * in->strideY + in->originX + tbOriginX,
                   in->bufferCb + (((in->originY + tbOriginY) * in->strideCb) >> 1) + ((in->originX + tbOriginX) >> 1),
                   in->bufferCr + (((in->originY + tbOriginY) * in->strideCr) >> 1) + ((in->originX + tbOriginX) >> 1)};
    void *rp[3] = {rec->bufferY + (rec->originY + tbOriginY) * rec->strideY + rec->originX + tbOriginX,
                   rec->bufferCb + (((rec->originY + tbOriginY) * rec->strideCb) >> 1) + ((rec->originX + tbOriginX) >> 1),
                   rec->bufferCr + (((rec->originY + tbOriginY) * rec->strideCr) >> 1) + ((rec->originX + tbOriginX) >> 1)};
    const uint32_t is_[3] = {in->strideY, in->strideCb, in->strideCr}, rs[3] = {rec->strideY, rec->strideCb, rec->strideCr};
    sao_on_device(0, ip, is_, rp, rs, saoStats, md, fullLambda, fullChromaLambdaSao, mmSao, pcs, lcuWidth, lcuHeight, saoPtr, leftSaoPtr,
                  upSaoPtr, saoLumaBestCost, saoChromaBestCost);
    return EB_ErrorNone;
}

EB_ERRORTYPE __wrap_SaoGenerationDecision16bit(EbPictureBufferDesc_t *inputLcuPtr, SaoStats_t *saoStats, SaoParameters_t *saoParams,
                                               MdRateEstimationContext_t *md, EB_U64 fullLambda, EB_U64 fullChromaLambdaSao, EB_BOOL mmSao,
                                               PictureControlSet_t *pcs, EB_U32 tbOriginX, EB_U32 tbOriginY, EB_U32 lcuWidth,
                                               EB_U32 lcuHeight, SaoParameters_t *saoPtr, SaoParameters_t *leftSaoPtr,
                                               SaoParameters_t *upSaoPtr, EB_S64 *saoLumaBestCost, EB_S64 *saoChromaBestCost)
{
    if (svt_hook_ep_active)
        svt_hook_ep_note_sao(pcs, tbOriginX, tbOriginY, md, fullLambda, fullChromaLambdaSao, mmSao, 1);
    if (g_sao_state == 0)
        g_sao_state = getenv("SVT_HOOK_SAO") ? 1 : -1;
    const EbPictureBufferDesc_t *rec = pcs->ParentPcsPtr->isUsedAsReferenceFlag == EB_TRUE
        ? ((EbReferenceObject_t *)pcs->ParentPcsPtr->referencePictureWrapperPtr->objectPtr)->referencePicture16bit : pcs->reconPicture16bitPtr;
    if (g_sao_state < 0 || !g_ctx || saoParams != saoPtr || rec->colorFormat != EB_YUV420) {
        COUNT_CPU(SaoGenerationDecision16bit);
        return __real_SaoGenerationDecision16bit(inputLcuPtr, saoStats, saoParams, md, fullLambda, fullChromaLambdaSao, mmSao, pcs, tbOriginX,
                                                 tbOriginY, lcuWidth, lcuHeight, saoPtr, leftSaoPtr, upSaoPtr, saoLumaBestCost,
                                                 saoChromaBestCost);
    }
    void *ip[3] = {inputLcuPtr->bufferY, inputLcuPtr->bufferCb, inputLcuPtr->bufferCr};
    void *rp[3] = {(uint16_t *)rec->bufferY + (rec->originY + tbOriginY) * rec->strideY + rec->originX + tbOriginX,
                   (uint16_t *)rec->bufferCb + (((rec->originY + tbOriginY) * rec->strideCb) >> 1) + ((rec->originX + tbOriginX) >> 1),
                   (uint16_t *)rec->bufferCr + (((rec->originY + tbOriginY) * rec->strideCb) >> 1) + ((rec->originX + tbOriginX) >> 1)};
    const uint32_t is_[3] = {inputLcuPtr->strideY, inputLcuPtr->strideCb, inputLcuPtr->strideCr},
                   rs[3] = {rec->strideY, rec->strideCb, rec->strideCr};
    sao_on_device(1, ip, is_, rp, rs, saoStats, md, fullLambda, fullChromaLambdaSao, mmSao, pcs, lcuWidth, lcuHeight, saoPtr, leftSaoPtr,
                  upSaoPtr, saoLumaBestCost, saoChromaBestCost);
    return EB_ErrorNone;
}

/* ---- life cycle: the bindings' device state belongs to an encoder instance, not to the process ------------------------- */
/* The reference's worker threads are created by EbInitEncoder and return when EbDeinitEncoder's end objects reach them
 * (EB_CHECK_END_OBJ, Codec/EbDefinitions.h:584).  The two kernels that call into the bindings are interposed as thread entry points
 * (--wrap=MotionEstimationKernel / EncDecKernel; EbEncHandle.c:1466, :1493 take them by address): when the last of them has returned,
 * nothing can call a binding any more, and everything the bindings hold on the device - EncDec picture objects, lanes, reference cache,
 * front-half lanes, the root context - is released, so that a later EbInitEncoder in the same process (another resolution, ffmpeg's next
 * output) starts from nothing.  Two encoders alive at once share the state until both are gone (sizes are validated on reuse). */
void *__real_MotionEstimationKernel(void *inputPtr);
void *__real_EncDecKernel(void *inputPtr);
void svt_hook_encdec_teardown(void);
static void hook_teardown(void)
{
    svt_hook_encdec_teardown();
    svt_hook_lock(&g_front_lock);
    svt_hook_lock(&g_lock);
    if (g_ctx) {
        svt_amd_synchronize(g_ctx);
        for (int i = 0; i < REF_CACHE; i++)
            for (int k = 0; k < 3; k++)
                if (g_refs[i].d[k])
                    svt_amd_device_free(g_ctx, g_refs[i].d[k]);
        free(g_refs), g_refs = NULL, REF_CACHE = 0;
        for (int k = 0; k < 3; k++) {
            if (g_inter_scratch[k])
                svt_amd_device_free(g_ctx, g_inter_scratch[k]), g_inter_scratch[k] = NULL;
            if (g_inter16_scratch[k])
                svt_amd_device_free(g_ctx, g_inter16_scratch[k]), g_inter16_scratch[k] = NULL;
        }
        for (int i = 0; i < NLANES; i++) {
            if (g_front[i].lane)
                svt_amd_context_destroy(g_front[i].lane);
            memset(&g_front[i], 0, sizeof(g_front[i]));
        }
        (void)svt_amd_host_unregister_all(g_ctx); /* svt_hook_pin_picture: before EbDeinitEncoder frees the picture pools */
        svt_amd_context_destroy(g_ctx);
        g_ctx = NULL;
        memset(g_slot_pic, 0, sizeof(g_slot_pic));
    }
    __atomic_store_n(&g_app_cb, NULL, __ATOMIC_RELEASE);
    g_context_failed = 0;
    __atomic_store_n(&g_reported, 0, __ATOMIC_RELEASE), __atomic_store_n(&g_failed, 0, __ATOMIC_RELEASE);
    svt_hook_unlock(&g_lock);
    svt_hook_unlock(&g_front_lock);
}
static void *kernel_thread(void *(*real)(void *), void *arg)
{
    __atomic_add_fetch(&g_live_threads, 1, __ATOMIC_ACQ_REL);
    t_kernel_thread = 1;
    void *r = real(arg);
    t_kernel_thread = 0;
    if (__atomic_sub_fetch(&g_live_threads, 1, __ATOMIC_ACQ_REL) == 0)
        hook_teardown();
    return r;
}
void *__wrap_MotionEstimationKernel(void *inputPtr) { return kernel_thread(__real_MotionEstimationKernel, inputPtr); }

/*
 * SURVEY 8f-4, the wire format of 10-bit input: the application's 16-bit samples become the encoder's 8-bit plane + 2-bit plane in the UnPack2D threads
 * (Codec/EbPictureOperators.c:512; CopyFrameBuffer, EbEncHandle.c:3485-3551, cuts each plane into row bands and posts one job per band).  With
 * SVT_HOOK_UNPACK=1 a thread keeps the reference's job protocol (take a job, do it, take an end-of-job token, give the job back, post the token) and does the job
 * on the device: svt_amd_EB_ENC_msbUnPack2D = the signature of the table slot the reference thread calls (UnPack2D_funcPtrArray_16Bit).  One job = one
 * band over PCIe and back: this binding proves the kernel inside the encoder (same stream out of the same 16-bit file); the device-side form for planes that
 * stay in HBM is svt_amd_unpack_plane.
 */
void *__real_UnPack2D(void *context);
static unsigned long g_unpack_jobs, g_unpack_samples;
void *__wrap_UnPack2D(void *context)
{
    const char *on = getenv("SVT_HOOK_UNPACK");
    if (!on || atoi(on) <= 0)
        return __real_UnPack2D(context);
    UnPackContext_t *c = (UnPackContext_t *)context;
    for (;;) {
        EbObjectWrapper_t *job, *token;
        EbGetFullObject(c->copyFrameOutputFifoPtr, &job);
        if (job->quitSignal == EB_TRUE)
            break;
        const EBUnPack2DType_t *u = (const EBUnPack2DType_t *)job->objectPtr;
        if (svt_hook_failed())
            EB_ENC_msbUnPack2D(u->in16BitBuffer, u->inStride, u->out8BitBuffer, u->outnBitBuffer, u->out8Stride, u->outnStride, u->width, u->height);
        else {
            svt_amd_EB_ENC_msbUnPack2D(u->in16BitBuffer, u->inStride, u->out8BitBuffer, u->outnBitBuffer, u->out8Stride, u->outnStride, u->width, u->height);
            __atomic_add_fetch(&g_unpack_jobs, 1, __ATOMIC_RELAXED);
            __atomic_add_fetch(&g_unpack_samples, (unsigned long)u->width * u->height, __ATOMIC_RELAXED);
        }
        EbGetEmptyObject(c->unPackInputFifoPtr, &token);
        EbReleaseObject(job);
        EbPostFullObject(token);
    }
    return EB_NULL;
}
static __thread int t_encdec_thread; /* SVT_HOOK_TIMELINE: GeneratePadding calls of EncDec threads are PadRefAndSetFlags's (the picture-analysis threads pad input pictures) */
void *__wrap_EncDecKernel(void *inputPtr)
{
    t_encdec_thread = 1;
    return kernel_thread(__real_EncDecKernel, inputPtr);
}

/* SVT_HOOK_TIMELINE only: what lies between a reference picture's last LCU and the next picture's first on the host - the tail EncDecKernel runs on ONE thread
 * (ApplySaoOffsetsPicture, then PadRefAndSetFlags = three GeneratePadding calls, Codec/EbEncDecProcess.c:3081-3109) and the first LCU of every picture
 * (ModeDecisionConfigureLcu of LCU 0).  Pass-throughs otherwise. */
void __real_GeneratePadding(EB_BYTE srcPic, EB_U32 srcStride, EB_U32 originalSrcWidth, EB_U32 originalSrcHeight, EB_U32 paddingWidth, EB_U32 paddingHeight);
void __wrap_GeneratePadding(EB_BYTE srcPic, EB_U32 srcStride, EB_U32 originalSrcWidth, EB_U32 originalSrcHeight, EB_U32 paddingWidth, EB_U32 paddingHeight)
{
    if (!t_encdec_thread || !svt_hook_timeline_enabled()) {
        __real_GeneratePadding(srcPic, srcStride, originalSrcWidth, originalSrcHeight, paddingWidth, paddingHeight);
        return;
    }
    const double t0 = svt_hook_now();
    __real_GeneratePadding(srcPic, srcStride, originalSrcWidth, originalSrcHeight, paddingWidth, paddingHeight);
    svt_hook_timeline("refpad", 0, (int)originalSrcWidth, (int)originalSrcHeight, t0, svt_hook_now());
}
void __real_ModeDecisionConfigureLcu(ModeDecisionContext_t *contextPtr, LargestCodingUnit_t *lcuPtr, PictureControlSet_t *pcs, SequenceControlSet_t *scs, EB_U8 pictureQp,
                                     EB_U8 lcuQp);
void __wrap_ModeDecisionConfigureLcu(ModeDecisionContext_t *contextPtr, LargestCodingUnit_t *lcuPtr, PictureControlSet_t *pcs, SequenceControlSet_t *scs, EB_U8 pictureQp,
                                     EB_U8 lcuQp)
{
    if (lcuPtr->index == 0 && svt_hook_timeline_enabled()) {
        const double t = svt_hook_now();
        svt_hook_timeline("lcu0", pcs->pictureNumber, pcs->temporalLayerIndex, (int)pcs->sliceType, t, t);
    }
    __real_ModeDecisionConfigureLcu(contextPtr, lcuPtr, pcs, scs, pictureQp, lcuQp);
}

static void hook_report(void)
{
    timeline_write();
    /* the sample application closes stderr before it returns (EbAppConfig.c:648): the report goes to the file SVT_HOOK_REPORT
     * names, or to stdout */
    const char *rp = getenv("SVT_HOOK_REPORT");
    FILE *out = rp ? fopen(rp, "w") : stdout;
    if (!out)
        return;
    svt_hook_encdec_report(out);
    svt_hook_reference_report(out);
    if (g_n_timed)
        fprintf(out, "svt_hook_me: front-half timeline over %lu pictures: submit call %.3f ms, submit -> results on the host %.3f ms, lane held %.3f ms "
                     "(means); %lu waits for a free lane, %.1f ms in total\n", g_n_timed, 1e3 * g_t_submit_call / g_n_timed, 1e3 * g_t_device / g_n_timed,
                1e3 * g_t_lane_held / g_n_timed, g_n_lane_wait, 1e3 * g_t_lane_wait);
    if (g_n_timed && g_verbose) {
        fprintf(out, "svt_hook_me: first pictures (ms since the first front-half call: submitted / results on the host / all LCUs served):");
        for (int i = 0; i < TL_N; i++)
            fprintf(out, " %d: %.1f/%.1f/%.1f", i, 1e3 * g_tl_submit[i], 1e3 * g_tl_ready[i], 1e3 * g_tl_released[i]);
        fprintf(out, "\n");
    }
    if (g_verbose) {
        fprintf(out, "svt_hook_me: %-40s %lu calls left to the reference code\n", "EncodePassInterPrediction", counter_sum(CPU_EncodePassInterPrediction));
        fprintf(out, "svt_hook_me: %-40s %lu calls left to the reference code\n", "EncodePassInterPrediction16bit", counter_sum(CPU_EncodePassInterPrediction16bit));
        fprintf(out, "svt_hook_me: %-40s %lu calls left to the reference code\n", "Inter2Nx2NPuPredictionHevc", counter_sum(CPU_Inter2Nx2NPuPredictionHevc));
        fprintf(out, "svt_hook_me: %-40s %lu calls left to the reference code\n", "Intra4x4IntraPredictionCl", counter_sum(CPU_Intra4x4IntraPredictionCl));
        fprintf(out, "svt_hook_me: %-40s %lu calls left to the reference code\n", "IntraPredictionCl", counter_sum(CPU_IntraPredictionCl));
        fprintf(out, "svt_hook_me: %-40s %lu calls left to the reference code\n", "IntraPredictionOl", counter_sum(CPU_IntraPredictionOl));
        fprintf(out, "svt_hook_me: %-40s %lu calls left to the reference code\n", "SaoGenerationDecision", counter_sum(CPU_SaoGenerationDecision));
        fprintf(out, "svt_hook_me: %-40s %lu calls left to the reference code\n", "SaoGenerationDecision16bit", counter_sum(CPU_SaoGenerationDecision16bit));
        fprintf(out, "svt_hook_me: with the CABAC-context-updating estimator on the GPU: full loop luma %lu chroma %lu\n", g_fl_cabac_gpu, g_cl_cabac_gpu);
        fprintf(out, "svt_hook_me: on the GPU: full loop luma %lu (left to the reference code %lu) chroma %lu (%lu), recon %lu, intra encode pass %lu + 4x4 %lu, "
                        "intra MD closed %lu open %lu 4x4 %lu, inter encode pass %lu + 16-bit %lu, inter MD %lu, quantiser %lu + PM-core %lu, SAO %lu\n",
                g_fl_gpu, g_fl_cpu, g_cl_gpu, g_cl_cpu, g_recon_gpu, g_intra_gpu, g_intra4_gpu, g_md_intra_gpu, g_md_intra_ol_gpu, g_md_intra4_gpu,
                g_inter_gpu, g_inter16_gpu, g_md_inter_gpu, g_quant_gpu, g_quant_pm_gpu, g_sao_gpu);
    }
    if (front_verify())
        fprintf(out, "svt_hook_me: front-half verification: %lu MotionEstimateLcu answers compared with the reference code's, %lu differ; %lu OpenLoopIntraSearchLcu answers compared, %lu differ\n",
                g_me_verified, g_me_mismatch, g_ois_verified, g_ois_mismatch);
    if (g_pinned_at_init)
        fprintf(out, "svt_hook_me: %lu picture buffers of the encoder's pools page-locked while the pools were built (EbInitEncoder)\n", g_pinned_at_init);
    if (g_unpack_jobs)
        fprintf(out, "svt_hook_me: 16-bit input -> 8-bit + 2-bit planes (UnPack2D) on the GPU: %lu jobs, %lu samples\n", g_unpack_jobs, g_unpack_samples);
    if (sbo_on())
        fprintf(out, "svt_hook_me: AC energy (CalculateAcEnergy) of %lu pictures on the GPU, %lu ComputeNxMSatdSadLCU calls answered from it, %lu left to the reference code\n",
                g_sbo_pictures, g_sbo_answers, g_sbo_cpu);
    fprintf(out, "svt_hook_me: %lu pictures / %lu LCUs intra-searched (OIS) on the GPU, 0 on the CPU\n", g_ois_pictures,
            g_ois_lcus);
    fprintf(out, "svt_hook_me: %lu pictures / %lu LCUs estimated on the GPU, 0 on the CPU\n", g_pictures, g_lcus);
    fflush(out);
    if (rp)
        fclose(out);
}
