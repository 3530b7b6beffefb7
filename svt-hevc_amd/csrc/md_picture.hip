/*
 * The host side of the device-resident mode decision (include/svt_hevc_amd.h "Device-resident mode decision"): the mode decision's part of a picture object, the
 * launch budget of the k_md_picture launches in flight, the blocking entries svt_amd_md_encode_picture*, the stream-ordered svt_amd_md_encode_picture_launch, the
 * debug entries and the control and motion-field bindings.  The kernels are md_kernels.hip's; the two units meet in md_picture.h.
 */
#include "md_picture.h"
#include <string.h>
#include <vector>
#include <mutex>
#include <condition_variable>
#include <chrono>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include "md_logic.h"
#include "mdlaunch.h"
#include "md_widths.h"
extern "C" int svt_amd_md_picture_supported(const SvtAmdMdPicture *P) { return P ? md_picture_supported(P) : 0; }
extern "C" int svt_amd_md_picture_supported_inter(const SvtAmdMdPicture *P, const SvtAmdMdInter *X) { return P && X ? md_picture_supported_inter(P, X) : 0; }
extern "C" int svt_amd_md_picture_supported_inter16(const SvtAmdMdPicture *P, const SvtAmdMdInter *X) { return P && X ? md_picture_supported_inter16(P, X) : 0; }
extern "C" int svt_amd_md_lcus_supported(const SvtAmdMdPicture *P, const SvtAmdMdLcu *lcus, int n)
{
    if (!P || !lcus)
        return 0;
    for (int i = 0; i < n; i++)
        if (!md_lcu_supported(P, &lcus[i]))
            return 0;
    return 1;
}

/* the mode decision's part of a picture object: neighbour maps, the picture's source and the per-LCU arrays, all in HBM */
struct SvtAmdMdState {
    MdPictureDev d;
    uint8_t *d_src[3];
    size_t src_cap[3];             /* bytes of d_src[k] (grown when a caller's row pitch needs more than the picture object's own) */
    SvtAmdOisLcuResult *d_ois;
    SvtAmdMdLcu *d_lcus;
    SvtAmdMdPicture *d_P;
    SvtAmdMdLcuOut *d_out;
    void *d_works, *d_results;    /* SvtAmdLcuWork / SvtAmdLcuResult of the picture object's sample width */
    size_t work_bytes, result_bytes;
    uint16_t *d_src16[3];          /* 10-bit pictures: the source as the encode pass codes it (d_src = its 8 MSBs, what the mode decision reads) */
    uint8_t *d_ref8[2][3];         /* ... and the 8-MSB views of the two reference pictures (UnPackReferenceBlock) */
    size_t ref8_bytes[2][3];
    size_t info_bytes, mv_bytes;
    unsigned long long *d_prof;
    unsigned long long *d_trace;
    int trace_lcu, trace_unit;
    int force_butterflies;
    unsigned *d_md_done;           /* epoch of the call whose mode decision finished the LCU */
    unsigned *d_md_ticket;         /* the mode-decision kernel's ticket counter (the encode pass behind it draws from the picture object's own) */
    MdPictureDev *d_D;             /* the descriptor the kernel reads (d, copied per call) */
    hipEvent_t ev_k0, ev_k1, ev_k2; /* around the last launch of k_md_picture on the call's stream (svt_amd_debug_md_kernel_ms), and behind the encode pass that follows it */
    int grid;                      /* its workgroups */
    bool ifree;                    /* the call's picture is a P / B picture coded without sub-sample search (!SvtAmdMdInter.use_subpel): svt_amd_md_kernel_launch's instance */
    /* P / B pictures */
    SvtAmdMdInter *d_X;
    SvtAmdMeLcuResult *d_me;
    SvtAmdTmvpLcu *d_tmvp;
    /* the call's small inputs (picture controls, inter controls, rate tables) come from the caller's stack / the encoder's heap: pageable memory, whose "asynchronous"
     * copy is a staged one the runtime completes inside the call - behind whatever its queue is running (profiles/r05_v: plane copies of one call issued 720 ms apart
     * while other pictures' mode-decision kernels ran).  They go through this page-locked block instead */
    uint8_t *h_stage;
    void *retired[8];              /* source planes outgrown by a caller's row pitch */
    int n_retired;
};
static constexpr size_t MD_STAGE_P = 0, MD_STAGE_X = (sizeof(SvtAmdMdPicture) + 63) & ~(size_t)63, MD_STAGE_COST = MD_STAGE_X + ((sizeof(SvtAmdMdInter) + 63) & ~(size_t)63),
                        MD_STAGE_D = MD_STAGE_COST + ((sizeof(SvtAmdCabacCost) + 63) & ~(size_t)63), MD_STAGE_CHECK = MD_STAGE_D + ((sizeof(MdPictureDev) + 63) & ~(size_t)63),
                        MD_STAGE_BYTES = MD_STAGE_CHECK + ((sizeof(SvtAmdMdCtlCheck) + 63) & ~(size_t)63);

void svt_amd_md_state_free(SvtAmdEncDecPicture *pic)
{
    SvtAmdMdState *m = pic->md;
    if (!m)
        return;
    void *ptrs[] = {m->d.md_rec, m->d.md_info, m->d_src[0], m->d_src[1], m->d_src[2], m->d_ois, m->d_lcus, m->d_P, m->d_out, m->d_works, m->d_results,
                    m->d.md_mv, m->d_X, m->d_me, m->d_tmvp, m->d_prof, m->d_trace, m->d_md_done, m->d_md_ticket, m->d_D, m->d_src16[0], m->d_src16[1], m->d_src16[2],
                    m->d_ref8[0][0], m->d_ref8[0][1], m->d_ref8[0][2], m->d_ref8[1][0], m->d_ref8[1][1], m->d_ref8[1][2]};
    for (void *q : ptrs)
        if (q)
            (void)hipFree(q);
    for (int i = 0; i < m->n_retired; i++)
        (void)hipFree(m->retired[i]);
    if (m->ev_k0)
        (void)hipEventDestroy(m->ev_k0);
    if (m->ev_k1)
        (void)hipEventDestroy(m->ev_k1);
    if (m->ev_k2)
        (void)hipEventDestroy(m->ev_k2);
    if (m->h_stage)
        (void)hipHostFree(m->h_stage);
    free(m);
    pic->md = nullptr;
}

static int md_state(SvtAmdEncDecPicture *pic, SvtAmdMdState **out)
{
    if (pic->md) {
        *out = pic->md;
        return SVT_AMD_OK;
    }
    SvtAmdMdState *m = (SvtAmdMdState *)calloc(1, sizeof(*m));
    if (!m)
        return SVT_AMD_ERR_RESOURCES;
    pic->md = m;
    const size_t n = (size_t)pic->nlcu;
    m->d.md_pitch = pic->d.pitch[0];
    m->d.info_pitch = ((uint32_t)(pic->d.width >> 2) + 63) & ~63u;
    m->info_bytes = sizeof(uint32_t) * (size_t)m->d.info_pitch * (pic->d.height >> 2);
    const size_t bps = pic->d.bps;
    m->work_bytes = bps == 2 ? sizeof(SvtAmdLcuWork16) : sizeof(SvtAmdLcuWork), m->result_bytes = bps == 2 ? sizeof(SvtAmdLcuResult16) : sizeof(SvtAmdLcuResult);
    bool ok = hipMalloc((void **)&m->d.md_rec, pic->plane_bytes[0] / bps) == hipSuccess && hipMalloc((void **)&m->d.md_info, m->info_bytes) == hipSuccess;
    for (int k = 0; k < 3 && ok; k++) {
        /* room for the caller's row pitch (an encoder's padded input pictures: width + up to 512 columns): growing the plane later means a hipFree, which waits for every
         * kernel on the device - the other pictures' mode decisions - with the runtime's memory lock held (profiles/r05_aa: 90 - 300 ms, other threads' copies queueing behind it) */
        const size_t roomy = (size_t)((pic->d.width + 512) >> (k ? 1 : 0)) * (pic->d.height >> (k ? 1 : 0)) + 64;
        const size_t cap = roomy > pic->plane_bytes[k] / bps ? roomy : pic->plane_bytes[k] / bps;
        ok = hipMalloc((void **)&m->d_src[k], cap) == hipSuccess;
        m->src_cap[k] = ok ? cap - 64 : 0;
        if (bps == 2)
            ok = ok && hipMalloc((void **)&m->d_src16[k], pic->plane_bytes[k]) == hipSuccess;
    }
    ok = ok && hipMalloc((void **)&m->d_ois, sizeof(SvtAmdOisLcuResult) * n) == hipSuccess && hipMalloc((void **)&m->d_lcus, sizeof(SvtAmdMdLcu) * n) == hipSuccess &&
         hipMalloc((void **)&m->d_P, sizeof(SvtAmdMdPicture)) == hipSuccess && hipMalloc((void **)&m->d_out, sizeof(SvtAmdMdLcuOut) * n) == hipSuccess &&
         hipMalloc((void **)&m->d_works, m->work_bytes * n) == hipSuccess && hipMalloc((void **)&m->d_results, m->result_bytes * n) == hipSuccess;
    m->d.mv_pitch = ((uint32_t)(pic->d.width >> 3) + 15) & ~15u;
    m->mv_bytes = sizeof(uint4) * (size_t)m->d.mv_pitch * ((pic->d.height + 7) >> 3);
    ok = ok && hipMalloc((void **)&m->d.md_mv, m->mv_bytes) == hipSuccess && hipMalloc((void **)&m->d_X, sizeof(SvtAmdMdInter)) == hipSuccess &&
         hipMalloc((void **)&m->d_me, sizeof(SvtAmdMeLcuResult) * n) == hipSuccess && hipMalloc((void **)&m->d_tmvp, sizeof(SvtAmdTmvpLcu) * (n + 1)) == hipSuccess;
    ok = ok && hipMalloc((void **)&m->d_md_done, sizeof(unsigned) * n) == hipSuccess && hipMemset(m->d_md_done, 0, sizeof(unsigned) * n) == hipSuccess;
    ok = ok && hipMalloc((void **)&m->d_md_ticket, 64) == hipSuccess && hipMalloc((void **)&m->d_D, sizeof(MdPictureDev)) == hipSuccess;
    ok = ok && hipHostMalloc((void **)&m->h_stage, MD_STAGE_BYTES, hipHostMallocDefault) == hipSuccess;
    ok = ok && hipEventCreate(&m->ev_k0) == hipSuccess && hipEventCreateWithFlags(&m->ev_k1, hipEventBlockingSync) == hipSuccess; /* ev_k1: the caller sleeps through the kernel */
    ok = ok && hipEventCreate(&m->ev_k2) == hipSuccess;
    if (!ok) {
        svt_amd_set_error("hipMalloc (mode-decision picture state) failed");
        svt_amd_md_state_free(pic);
        return SVT_AMD_ERR_RESOURCES;
    }
    *out = m;
    return SVT_AMD_OK;
}

/* How much of the device the k_md_picture launches in flight may hold.  A workgroup of this kernel holds a whole CU (its LDS) for the life of the launch, most of it
 * waiting for neighbours: whatever else the encoder needs meanwhile - the next pictures' motion estimation and open-loop intra search, picture preparation, the runtime's
 * copy and fill kernels - waits for a mode-decision launch to END once they fill the part (profiles/r05_a: with 12 - 16 pictures in the encoder's pool the closed loop
 * fell from 57 to 25 fps, launches starting in bursts exactly when others finished).  The launches therefore share a BUDGET of workgroups = CUs - CUs / 16 (240 on an
 * MI355X): a call waits for its grid to fit AFTER its inputs are on the device (lowest temporal layer first among the waiters, then first come) and gives the workgroups
 * back when its kernel has finished, before its records travel back.
 * How wide a launch is decides how many pictures share the device: the wavefront of a 4K picture is 30 LCUs wide at its widest and 16 on average; 40 workgroups (the
 * widest front + the encode passes behind it) give a lone picture its shortest kernel (51.5 ms for a layer-2 picture), 20 cost it 9 % (56.0 ms) and let twelve pictures
 * run side by side - 148 instead of 96 pictures/s of device capacity (profiles/r05_k_md_flights_24q.txt), 93 - 96 instead of 79 fps of encode (r05_k_sweep_grid2.txt).
 * A call therefore takes the wide grid only while the device is nearly idle (at most a third of the budget in use and nobody waiting) and the narrow one (half) otherwise.
 * SVT_AMD_MD_MAX_KERNELS=<n> forces a plain count limit instead, SVT_AMD_MD_GRID=<n> a fixed width (measurement). */
namespace {
std::mutex g_flight_mu;
std::condition_variable g_flight_cv;
/* per DEVICE: a process with contexts on several GPUs must not charge device B's launches against device A's compute units */
struct FlightDevice { int flights = 0, wgs = 0, cus = 0; };
FlightDevice g_flight_dev[64];
unsigned long long g_flight_ticket;
struct FlightWaiter { int prio; unsigned long long ticket; int device; };
std::vector<FlightWaiter> g_flight_wait;
int md_forced_count_limit()
{
    static const int forced = getenv("SVT_AMD_MD_MAX_KERNELS") ? atoi(getenv("SVT_AMD_MD_MAX_KERNELS")) : 0;
    return forced;
}
int md_wg_budget(int device)
{
    int c;
    {
        std::lock_guard<std::mutex> l(g_flight_mu);
        FlightDevice &fd = g_flight_dev[device & 63];
        if (!fd.cus) {
            hipDeviceProp_t pr;
            fd.cus = hipGetDeviceProperties(&pr, device) == hipSuccess ? pr.multiProcessorCount : 256;
        }
        c = fd.cus;
    }
    static const int forced = getenv("SVT_AMD_MD_WG_BUDGET") ? atoi(getenv("SVT_AMD_MD_WG_BUDGET")) : 0; /* measurement */
    return forced > 0 ? forced : c - c / 16;
}
/* SVT_AMD_MD_FLIGHT_STATS=<file> (measurement): one line appended when the process ends - calls, time spent waiting for a place, wide / narrow grants */
struct FlightStats {
    std::atomic<unsigned long long> calls{0}, wide{0}, wait_us{0}, run_us{0}, wgs_seen{0};
    ~FlightStats()
    {
        const char *path = getenv("SVT_AMD_MD_FLIGHT_STATS");
        FILE *f = calls && path ? fopen(path, "a") : nullptr;
        if (!f)
            return;
        fprintf(f, "svt_amd: mode-decision launches: %llu calls (%llu at the wide grid), waiting for a place %.1f ms a call, launch -> kernel done %.1f ms a call, "
                   "%.1f workgroups of other calls in flight at a grant (mean)\n", (unsigned long long)calls, (unsigned long long)wide, 1e-3 * (double)wait_us / (double)calls,
                1e-3 * (double)run_us / (double)calls, (double)wgs_seen / (double)calls);
        fclose(f);
    }
} g_flight_stats;
double flight_now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
struct MdFlight {
    int held = 0; /* workgroups this call holds */
    int dev = 0;
    double t_granted = 0;
    /* waits until the launch fits; returns the grid granted: `wide` when the device is nearly idle, `narrow` otherwise */
    /* lone: the width of a launch that finds the device without any other mode-decision launch (two workgroups per LCU of the widest front); wide / narrow: round 5's pair for
     * a device that is shared - the encoder's steady state is untouched by `lone` */
    int acquire(int device, int budget, int lone, int wide, int narrow, int prio)
    {
        const double t0 = flight_now_us();
        dev = device & 63;
        std::unique_lock<std::mutex> l(g_flight_mu);
        FlightDevice &fd = g_flight_dev[dev];
        const FlightWaiter me = {prio, g_flight_ticket++, dev};
        g_flight_wait.push_back(me);
        const int count_limit = md_forced_count_limit();
        int grant = 0;
        g_flight_cv.wait(l, [&] {
            int waiting_here = 0;
            for (const FlightWaiter &w : g_flight_wait) {
                if (w.device != dev)
                    continue;
                waiting_here++;
                if (w.prio < me.prio || (w.prio == me.prio && w.ticket < me.ticket))
                    return false;
            }
            if (count_limit > 0) {
                grant = wide;
                return fd.flights < count_limit;
            }
            grant = (waiting_here == 1 && fd.flights == 0) ? lone : (waiting_here == 1 && fd.wgs + wide <= budget / 3) ? wide : narrow;
            return fd.wgs + grant <= budget || fd.flights == 0;
        });
        for (size_t i = 0; i < g_flight_wait.size(); i++)
            if (g_flight_wait[i].ticket == me.ticket) {
                g_flight_wait.erase(g_flight_wait.begin() + (long)i);
                break;
            }
        g_flight_stats.calls++, g_flight_stats.wide += (grant == wide || grant == lone) && wide != narrow, g_flight_stats.wgs_seen += (unsigned long long)fd.wgs;
        fd.flights++, fd.wgs += grant, held = grant;
        l.unlock();
        t_granted = flight_now_us();
        g_flight_stats.wait_us += (unsigned long long)(t_granted - t0);
        g_flight_cv.notify_all(); /* the next in line may fit as well */
        return grant;
    }
    void release()
    {
        if (!held)
            return;
        g_flight_stats.run_us += (unsigned long long)(flight_now_us() - t_granted);
        {
            std::lock_guard<std::mutex> l(g_flight_mu);
            g_flight_dev[dev].flights--, g_flight_dev[dev].wgs -= held;
        }
        held = 0;
        g_flight_cv.notify_all();
    }
    ~MdFlight() { release(); }
};
}

/* everything the first svt_amd_md_encode_picture[_inter] call on this picture object would allocate (device state, page-locked staging, events), made now - by a host that
 * builds its picture objects before the clock starts (the encoder binding: EbInitEncoder) */
extern "C" int svt_amd_md_picture_warmup(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic)
{
    if (!ctx || !pic)
        return SVT_AMD_ERR_BAD_PARAM;
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = svt_amd_md_kernel_rate_tables(ctx->device);
    SvtAmdMdState *m = nullptr;
    if (!rc)
        rc = md_state(pic, &m);
    return rc;
}

/* ---- what the blocking entries (md_encode_picture) and svt_amd_md_encode_picture_launch share: each of the following exists once, and both call it ---- */

/* the launch widths (md_widths.h: the formulas and their measurements) under the measurement overrides: SVT_AMD_MD_GRID, a fixed launch width, is read at every call,
 * SVT_AMD_MD_NARROW / _WIDE once per process.  The blocking call hands all three to MdFlight::acquire; a launch takes `lone` or `narrow` */
static MdWidths md_launch_widths(int wl, int hl, int tiles, int n_active)
{
    const char *fg = getenv("SVT_AMD_MD_GRID");
    static const int fnarrow = getenv("SVT_AMD_MD_NARROW") ? atoi(getenv("SVT_AMD_MD_NARROW")) : 0;
    static const int fwide = getenv("SVT_AMD_MD_WIDE") ? atoi(getenv("SVT_AMD_MD_WIDE")) : 0;
    return md_widths(wl, hl, tiles, n_active, fg ? atoi(fg) : 0, fnarrow, fwide);
}

/* ME ([0]) and OIS ([1]) records read where another lane's kernels leave them, in a slot of the root context: this lane's stream orders itself behind those kernels
 * (md_records_wait), and the next launch INTO those slots behind this picture's kernel (md_records_read_mark) */
struct MdSlotRecords {
    SvtAmdContext *root;
    DevPicture *slot[2];
    int index[2];
};

/* the records of kind `which` in slot `slot`, or NULL after the refusal under the entry's name */
static const void *md_slot_records(MdSlotRecords *r, const SvtAmdEncDecPicture *pic, int which, int slot, const char *entry)
{
    const void *d = svt_amd_slot_records(r->root, slot, which, pic->d.width, pic->d.height);
    if (!d && which == 0)
        svt_amd_set_error("%s: slot %d does not hold the motion-estimation records of a %u x %u picture (none launched for the slot's current picture, or only a part of it)", entry,
                          slot, pic->d.width, pic->d.height);
    else if (!d)
        svt_amd_set_error("%s: slot %d does not hold the open-loop intra search records of a %u x %u picture", entry, slot, pic->d.width, pic->d.height);
    else
        r->slot[which] = &r->root->slots[slot], r->index[which] = slot;
    return d;
}

static int md_records_wait(SvtAmdContext *ctx, const MdSlotRecords &r)
{
    int rc = 0;
    for (int k = 0; k < 2 && !rc; k++)
        if (r.slot[k])
            rc = svt_amd_records_wait(ctx, r.slot[k], k, nullptr, nullptr, 0);
    return rc;
}

static int md_records_read_mark(SvtAmdContext *ctx, const MdSlotRecords &r)
{
    int rc = r.slot[0] ? svt_amd_records_read_mark(ctx, r.root, r.index[0]) : 0;
    if (!rc && r.slot[1] && r.slot[1] != r.slot[0])
        rc = svt_amd_records_read_mark(ctx, r.root, r.index[1]);
    return rc;
}

/* the reference pictures as the mode decision reads them: a 10-bit P / B picture decides on their 8 MSBs (the views grow at the first such call on the object, or with
 * reference pictures of more padding than any before) */
static int md_reference_views(hipStream_t st, SvtAmdEncDecPicture *pic, SvtAmdMdState *m, bool inter)
{
    for (int l = 0; l < 2; l++) {
        m->d.mref[l] = pic->d.ref[l];
        if (pic->d.bps == 2 && inter && pic->has_ref[l])
            for (int p = 0; p < 3; p++) {
                const size_t need = (size_t)pic->d.ref[l].size[p ? 1 : 0];
                if (m->ref8_bytes[l][p] < need) {
                    if (m->d_ref8[l][p])
                        (void)hipFree(m->d_ref8[l][p]);
                    m->d_ref8[l][p] = nullptr, m->ref8_bytes[l][p] = 0;
                    HIP_TRY(hipMalloc((void **)&m->d_ref8[l][p], need + 16));
                    m->ref8_bytes[l][p] = need;
                }
                const int rc = svt_amd_md_kernel_msb_view(st, pic->d.ref[l].plane[p], m->d_ref8[l][p], need);
                if (rc)
                    return rc;
                m->d.mref[l].plane[p] = m->d_ref8[l][p];
            }
    }
    return SVT_AMD_OK;
}

/* the descriptor's fields that do not depend on where the inputs come from (after the entry has taken the call's rate tables) */
static void md_descriptor_common(const SvtAmdEncDecPicture *pic, SvtAmdMdState *m)
{
    m->d.prof = m->d_prof, m->d.prof_lcus = pic->nlcu;
    m->d.trace = m->d_trace, m->d.trace_lcu = m->trace_lcu, m->d.trace_unit = m->trace_unit;
    m->d.force_butterflies = m->force_butterflies;
    m->d.P = m->d_P, m->d.out = m->d_out;
    m->d.cost = pic->has_cost ? pic->d_cost : nullptr;
}

/* the picture's arrays as the kernels expect to find them, on the context's stream in front of the kernel */
static int md_reset_arrays(hipStream_t st, SvtAmdEncDecPicture *pic, SvtAmdMdState *m, bool inter)
{
    if (inter)
        HIP_TRY(hipMemsetAsync(m->d.md_mv, 0, m->mv_bytes, st));
    HIP_TRY(hipMemsetAsync(pic->d.mode_map, 0xFF, pic->map_bytes, st));
    HIP_TRY(hipMemsetAsync(m->d.md_info, 0xFF, m->info_bytes, st));
    HIP_TRY(hipMemsetAsync(m->d_results, 0, m->result_bytes * (size_t)pic->nlcu, st));
    HIP_TRY(hipMemsetAsync(m->d_works, 0, m->work_bytes * (size_t)pic->nlcu, st));
    return SVT_AMD_OK;
}

/* the queue step: `grid` workgroups of the mode decision over the n_active LCUs of d_order, the encode pass behind it, the events the measurements read, the marks */
static int md_queue_picture(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, SvtAmdMdState *m, const MdSlotRecords &rec, bool inter, int grid, int n_active,
                            const unsigned *d_order, int tiles)
{
    hipStream_t st = svt_amd_ctx_stream(ctx);
    int rc;
    m->grid = grid;
    HIP_TRY(hipEventRecord(m->ev_k0, st));
    MdPictureLaunch l;
    l.st = st, l.grid = grid, l.d_D = m->d_D, l.d_works = m->d_works, l.n_active = n_active, l.wl = (pic->d.width + 63) / 64;
    l.ticket = m->d_md_ticket, l.md_done = m->d_md_done, l.order = d_order, l.epoch = pic->epoch;
    l.inter = inter, l.ifree = m->ifree, l.profiled = m->d.prof != nullptr, l.bps = pic->d.bps;
    if ((rc = svt_amd_md_kernel_launch(l)) != 0)
        return rc;
    HIP_TRY(hipEventRecord(m->ev_k1, st));
    /* the encode pass of the picture: its own kernel behind the decisions, on the same stream (every LCU's work record is in HBM; LCUs without intra units wait for nobody,
     * so a P / B picture runs as wide as the device is) */
    if (m->d.encode && (rc = svt_amd_ep_launch_behind_md(ctx, pic, m->d_works, m->d_results, n_active, d_order, inter, tiles)) != 0)
        return rc;
    HIP_TRY(hipEventRecord(m->ev_k2, st));
    if ((rc = ep_picture_written(ctx, pic)) != 0)
        return rc;
    return md_records_read_mark(ctx, rec);
}

/* bps: bytes per sample of the source planes, the work / result records and the picture object (1, or 2 = a 10-bit picture: the mode decision on the 8 MSBs of source
 * and reference pictures, the encode pass on the 10-bit samples) */
static int md_encode_picture(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdPicture *P, const SvtAmdMdInter *X, const SvtAmdMdLcu *lcus,
                             const void *src_y, uint32_t stride_y, const void *src_cb, const void *src_cr, uint32_t stride_c, const SvtAmdOisLcuResult *ois,
                             int ois_slot, const SvtAmdMeLcuResult *me, int me_slot, const SvtAmdTmvpLcu *tmvp, const SvtAmdCabacCost *cost, SvtAmdMdLcuOut *md_out,
                             void *works, void *results, uint32_t bps)
{
    /* svt_amd_md_picture_set_controls: a DEVICE array bound for this call, which consumes the binding whether it succeeds or refuses */
    const SvtAmdMdLcu *bound = pic ? pic->md_bound_lcus : nullptr;
    const SvtAmdTmvpLcu *bound_tmvp = pic ? pic->md_bound_tmvp : nullptr;
    if (pic)
        pic->md_bound_tmvp = nullptr;
    if (bound) {
        pic->md_bound_lcus = nullptr;
        if (lcus) {
            svt_amd_set_error("svt_amd_md_encode_picture: host LCU controls AND a bound device array (svt_amd_md_picture_set_controls): pass lcus == NULL; the binding is dropped");
            return SVT_AMD_ERR_BAD_PARAM;
        }
    }
    /* svt_amd_md_picture_set_motion_field: likewise for the co-located motion field - read below only by a P / B call with tmvp_enable, dropped unread otherwise */
    if (bound_tmvp && tmvp) {
        svt_amd_set_error("svt_amd_md_encode_picture_inter: a host motion field AND a bound device array (svt_amd_md_picture_set_motion_field): pass tmvp == NULL; the binding is dropped");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    if (!ctx || !pic || !P || (!lcus && !bound) || !src_y || !src_cb || !src_cr || (!X && !cost))
        return SVT_AMD_ERR_BAD_PARAM;
    if ((X ? !md_picture_supported_inter(P, X) : !md_picture_supported(P)) || P->width != pic->d.width || P->height != pic->d.height || pic->d.bps != bps) {
        svt_amd_set_error("svt_amd_md_encode_picture: picture outside what this revision covers (svt_amd_md_picture_supported[_inter]), or not the picture object's size / sample width");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    if (X && bps != 1 && !md_picture_supported_inter16(P, X)) {
        svt_amd_set_error("svt_amd_md_encode_picture_inter16: use_subpel 0 - a picture coded without sub-sample search predicts through the reference's interpolation-free path, "
                          "which this revision covers for 8-bit pictures only");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    if (X && (!pic->has_cost || !pic->has_ref[0] || (P->slice_type == 0 && !pic->has_ref[1]) || (X->tmvp_enable && !tmvp && !bound_tmvp))) {
        svt_amd_set_error("svt_amd_md_encode_picture_inter: reference pictures / rate tables not set (svt_amd_encdec_picture_set_inter), or no co-located motion field");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    const int n = pic->nlcu, wl = (pic->d.width + 63) / 64, hl = (pic->d.height + 63) / 64;
    int tiles = 0;
    for (int i = 0; lcus && i < n; i++) { /* a bound device array is checked on the device, below */
        if (lcus[i].leaf_count < 1 || lcus[i].leaf_count > SVT_AMD_MD_LEAVES) {
            svt_amd_set_error("svt_amd_md_encode_picture: LCU %d has no leaf list", i);
            return SVT_AMD_ERR_BAD_PARAM;
        }
        for (int k = 0; k < lcus[i].leaf_count; k++)
            if (lcus[i].leaf_index[k] >= SVT_AMD_MD_LEAVES || (k && lcus[i].leaf_index[k] <= lcus[i].leaf_index[k - 1])) {
                svt_amd_set_error("svt_amd_md_encode_picture: LCU %d: leaf list not ascending", i);
                return SVT_AMD_ERR_BAD_PARAM;
            }
        tiles += lcus[i].tile_left && lcus[i].tile_top;
        if (X && !md_lcu_supported(P, &lcus[i])) {
            svt_amd_set_error("svt_amd_md_encode_picture_inter: LCU %d is not decided by ModeDecisionLcu with luma-only candidates", i);
            return SVT_AMD_ERR_BAD_PARAM;
        }
    }
    if (bound && pic->md_rect_n) {
        svt_amd_set_error("svt_amd_md_encode_picture: a bound device array of LCU controls on a picture object with a rank rectangle (svt_amd_encdec_picture_set_rect): "
                          "the rectangle's tile-border check reads host records");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    MdSlotRecords rec = {ctx->parent ? ctx->parent : ctx, {nullptr, nullptr}, {-1, -1}};
    const SvtAmdMeLcuResult *d_me_slot = nullptr;
    if (X && !me && !(d_me_slot = (const SvtAmdMeLcuResult *)md_slot_records(&rec, pic, 0, me_slot, "svt_amd_md_encode_picture_inter")))
        return SVT_AMD_ERR_BAD_PARAM;
    const SvtAmdOisLcuResult *d_ois_slot = nullptr;
    if (!ois && !(d_ois_slot = (const SvtAmdOisLcuResult *)md_slot_records(&rec, pic, 1, ois_slot, "svt_amd_md_encode_picture")))
        return SVT_AMD_ERR_BAD_PARAM;
    if (pic->md_rect_n) { /* a rank's rectangle (svt_amd_encdec_picture_set_rect; host controls only): its borders must be tile borders - an LCU never waits for one outside */
        const SvtAmdRect &r = pic->md_rect;
        const int x0 = r.x / 64, y0 = r.y / 64, x1 = (r.x + r.w + 63) / 64, y1 = (r.y + r.h + 63) / 64;
        for (int y = y0; y < y1; y++)
            for (int x = x0; x < x1; x++) {
                const SvtAmdMdLcu &Lc = lcus[y * wl + x];
                if ((x == x0 && !Lc.tile_left) || (y == y0 && !Lc.tile_top) || (x == x1 - 1 && x1 < wl && !Lc.tile_right) ||
                    (y == y1 - 1 && y1 < hl && !lcus[(y + 1) * wl + x].tile_top)) {
                    svt_amd_set_error("svt_amd_md_encode_picture: the rectangle's border at LCU (%d, %d) is not a tile border", x, y);
                    return SVT_AMD_ERR_BAD_PARAM;
                }
            }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = svt_amd_md_kernel_rate_tables(ctx->device);
    if (rc)
        return rc;
    SvtAmdMdState *m = nullptr;
    if ((rc = md_state(pic, &m)) != 0)
        return rc;
    hipStream_t st = svt_amd_ctx_stream(ctx);
    if ((rc = md_records_wait(ctx, rec)) != 0)
        return rc;
    if (bound) { /* the host loop's refusals, its words and the tile count from the check kernel's record (mdctl_kernels.hip): one small copy, one synchronisation */
        const SvtAmdMdCtlCheck *c = (const SvtAmdMdCtlCheck *)(m->h_stage + MD_STAGE_CHECK);
        if ((rc = svt_amd_mdctl_check_async(ctx, bound, n, P->depth_mode, X != nullptr, (SvtAmdMdCtlCheck *)(m->h_stage + MD_STAGE_CHECK))) != 0)
            return rc;
        HIP_TRY(hipStreamSynchronize(st));
        if (c->first_bad != 0xFFFFFFFFu) {
            if (c->first_kind == 0)
                svt_amd_set_error("svt_amd_md_encode_picture: LCU %d has no leaf list", (int)c->first_bad);
            else if (c->first_kind == 1)
                svt_amd_set_error("svt_amd_md_encode_picture: LCU %d: leaf list not ascending", (int)c->first_bad);
            else
                svt_amd_set_error("svt_amd_md_encode_picture_inter: LCU %d is not decided by ModeDecisionLcu with luma-only candidates", (int)c->first_bad);
            return SVT_AMD_ERR_BAD_PARAM;
        }
        tiles = (int)c->tiles;
    }
    /* debug (SVT_AMD_MD_TIMING): host clock around the call's three parts, with a stream synchronisation after each - one line per call on stderr */
    static const bool timing = getenv("SVT_AMD_MD_TIMING") != nullptr;
    const auto t_call = std::chrono::steady_clock::now();
    if (timing)
        HIP_TRY(hipStreamSynchronize(st)); /* what the stream still had to do + the front half's records */
    const auto t_begin = std::chrono::steady_clock::now();
    auto t_up = t_begin, t_kernel = t_begin;
    auto t_tick = t_begin;
    auto tick = [&](const char *what) { /* SVT_AMD_MD_TIMING: a host call of the upload section that took more than 5 ms names itself */
        if (!timing)
            return;
        const auto now = std::chrono::steady_clock::now();
        const double d = std::chrono::duration<double, std::milli>(now - t_tick).count();
        if (d > 5.0)
            fprintf(stderr, "svt_amd_md_encode_picture: %.1f ms inside the host call '%s'\n", d, what);
        t_tick = now;
    };
    const void *hs[3] = {src_y, src_cb, src_cr};
    /* 8-bit source planes travel as ONE linear transfer each, in the host's row pitch (the device copy keeps that pitch): a strided copy is a shader kernel of the runtime
     * (__amd_rocclr_copyBufferRect: 2 ms per plane, and 40 ms when the mode-decision launches of other pictures hold the CUs - profiles/r05_b), a linear one from page-locked
     * memory is the DMA engine's */
    const bool linear = bps == 1 && stride_y % 4 == 0 && stride_c % 4 == 0 && stride_y < 2 * pic->d.width + 256 && stride_c < pic->d.width + 256;
    for (int k = 0; k < 3; k++) {
        const uint32_t pw = k ? pic->d.width / 2 : pic->d.width, ph = k ? pic->d.height / 2 : pic->d.height;
        if (linear) {
            const size_t hstride = k ? stride_c : stride_y, need = hstride * (ph - 1) + pw;
            if (m->src_cap[k] < need) {
                HIP_TRY(hipStreamSynchronize(st));
                if (m->d_src[k] && m->n_retired < 8)
                    m->retired[m->n_retired++] = m->d_src[k]; /* freed with the state: a hipFree here would wait for every kernel on the device */
                else if (m->d_src[k])
                    (void)hipFree(m->d_src[k]);
                m->d_src[k] = nullptr, m->src_cap[k] = 0;
                HIP_TRY(hipMalloc((void **)&m->d_src[k], need + 64));
                m->src_cap[k] = need;
            }
            const uint8_t *dv = (const uint8_t *)svt_amd_registered_device_ptr(hs[k], need);
            if (dv) {
                if ((rc = svt_amd_md_kernel_fetch_plane(st, k ? 32 : 96, m->d_src[k], dv, need)) != 0)
                    return rc;
            } else {
                HIP_TRY(hipMemcpyAsync(m->d_src[k], hs[k], need, hipMemcpyHostToDevice, st));
            }
            tick(k ? "source chroma plane copy" : "source luma plane copy");
        } else if (bps == 1) {
            HIP_TRY(hipMemcpy2DAsync(m->d_src[k], pic->d.pitch[k], hs[k], k ? stride_c : stride_y, pw, ph, hipMemcpyHostToDevice, st));
        } else { /* strides in samples */
            HIP_TRY(hipMemcpy2DAsync(m->d_src16[k], (size_t)pic->d.pitch[k] * 2, hs[k], (size_t)(k ? stride_c : stride_y) * 2, (size_t)pw * 2, ph, hipMemcpyHostToDevice, st));
            if ((rc = svt_amd_md_kernel_msb_view(st, m->d_src16[k], m->d_src[k], pic->plane_bytes[k] / 2)) != 0)
                return rc;
        }
        m->d.src[k] = m->d_src[k], m->d.src16[k] = bps == 2 ? m->d_src16[k] : nullptr;
    }
    m->d.src_pitch[0] = linear ? stride_y : pic->d.pitch[0], m->d.src_pitch[1] = linear ? stride_c : pic->d.pitch[1];
    if ((rc = md_reference_views(st, pic, m, X != nullptr)) != 0)
        return rc;
    if (lcus)
        HIP_TRY(hipMemcpyAsync(m->d_lcus, lcus, sizeof(SvtAmdMdLcu) * (size_t)n, hipMemcpyHostToDevice, st));
    tick("LCU controls copy");
    memcpy(m->h_stage + MD_STAGE_P, P, sizeof(*P)); /* (the block is free: the previous call on this object returned after its stream had drained) */
    HIP_TRY(hipMemcpyAsync(m->d_P, m->h_stage + MD_STAGE_P, sizeof(*P), hipMemcpyHostToDevice, st));
    if (cost) {
        memcpy(m->h_stage + MD_STAGE_COST, cost, sizeof(*cost));
        HIP_TRY(hipMemcpyAsync(pic->d_cost, m->h_stage + MD_STAGE_COST, sizeof(*cost), hipMemcpyHostToDevice, st));
        pic->has_cost = true;
    }
    m->d.X = nullptr, m->d.me = nullptr, m->d.tmvp = nullptr;
    if (X) {
        memcpy(m->h_stage + MD_STAGE_X, X, sizeof(*X));
        HIP_TRY(hipMemcpyAsync(m->d_X, m->h_stage + MD_STAGE_X, sizeof(*X), hipMemcpyHostToDevice, st));
        tick("picture / inter controls copies");
        if (me)
            HIP_TRY(hipMemcpyAsync(m->d_me, me, sizeof(SvtAmdMeLcuResult) * (size_t)n, hipMemcpyHostToDevice, st));
        tick("ME records copy");
        if (X->tmvp_enable && tmvp) {
            HIP_TRY(hipMemcpyAsync(m->d_tmvp, tmvp, sizeof(SvtAmdTmvpLcu) * (size_t)n, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemsetAsync(m->d_tmvp + n, 0, sizeof(SvtAmdTmvpLcu), st));
            tick("motion-field copy + fill");
        }
        m->d.X = m->d_X, m->d.me = me ? m->d_me : d_me_slot, m->d.tmvp = X->tmvp_enable && bound_tmvp ? bound_tmvp : m->d_tmvp; /* a bound field is read in place */
    }
    int n_active = n;
    const unsigned *d_order = pic->d_sync + 1 + n;
    if (pic->md_rect_n) {
        n_active = pic->md_rect_n, d_order = pic->d_order_md;
        HIP_TRY(hipMemsetAsync(m->d_out, 0, sizeof(SvtAmdMdLcuOut) * (size_t)n, st));
    }
    md_descriptor_common(pic, m);
    m->d.encode = !X || works || results; /* P / B pictures: without a place for the work / result records, the mode decision alone */
    if (ois)
        HIP_TRY(hipMemcpyAsync(m->d_ois, ois, sizeof(SvtAmdOisLcuResult) * (size_t)n, hipMemcpyHostToDevice, st));
    m->d.ois = ois ? m->d_ois : d_ois_slot, m->d.lcus = lcus ? m->d_lcus : bound;
    pic->epoch++;
    pic->deblocked = pic->sao_done = false;
    pic->md_works_whole = false; /* until this call has run to its end */
    HIP_TRY(hipMemsetAsync(pic->d_sync, 0, sizeof(unsigned), st));
    if ((rc = md_reset_arrays(st, pic, m, X != nullptr)) != 0)
        return rc;
    tick("OIS copy + five fills"); /* (and the vector fill of a P / B picture) */
    if (timing) {
        HIP_TRY(hipStreamSynchronize(st));
        tick("stream synchronisation after the uploads");
        t_up = std::chrono::steady_clock::now();
    }
    const MdWidths width = md_launch_widths(wl, hl, tiles, n_active);
    memcpy(m->h_stage + MD_STAGE_D, &m->d, sizeof(m->d));
    HIP_TRY(hipMemcpyAsync(m->d_D, m->h_stage + MD_STAGE_D, sizeof(m->d), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(m->d_md_ticket, 0, sizeof(unsigned), st));
    MdFlight flight;
    /* the inputs first (a call that waits for its place holds no CU and no copy engine meanwhile) */
    HIP_TRY(hipStreamSynchronize(st));
    const int grid = flight.acquire(ctx->device, md_wg_budget(ctx->device), width.lone, width.wide, width.narrow, (int)P->temporal_layer);
    m->ifree = X && !X->use_subpel;
    if ((rc = md_queue_picture(ctx, pic, m, rec, X != nullptr, grid, n_active, d_order, tiles)) != 0)
        return rc;
    if (timing) {
        HIP_TRY(hipStreamSynchronize(st));
        t_kernel = std::chrono::steady_clock::now();
    }
    if (flight.held) { /* the workgroups are free as soon as the kernel has finished: the records' way back needs no CU */
        HIP_TRY(hipEventSynchronize(m->ev_k1));
        flight.release();
    }
    if (md_out)
        HIP_TRY(hipMemcpyAsync(md_out, m->d_out, sizeof(SvtAmdMdLcuOut) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (works)
        HIP_TRY(hipMemcpyAsync(works, m->d_works, m->work_bytes * (size_t)n, hipMemcpyDeviceToHost, st));
    if (results)
        HIP_TRY(hipMemcpyAsync(results, m->d_results, m->result_bytes * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (timing) {
        const auto t_end = std::chrono::steady_clock::now();
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "svt_amd_md_encode_picture%s: layer %d, %d LCUs, stream + front-half records ready %.2f ms, inputs up %.2f ms, kernel %.2f ms, records down %.2f ms\n", X ? "_inter" : "",
                (int)P->temporal_layer, n_active, ms(t_call, t_begin), ms(t_begin, t_up), ms(t_up, t_kernel), ms(t_kernel, t_end));
    }
    pic->md_works_whole = !pic->md_rect_n && m->d.encode; /* (a P / B call that asked for decisions only writes no work records) */
    return SVT_AMD_OK;
}

/* a call the entry refuses by itself consumes the bindings as md_encode_picture would */
static int md_refuse_unbound(SvtAmdEncDecPicture *pic)
{
    if (pic)
        pic->md_bound_lcus = nullptr, pic->md_bound_tmvp = nullptr;
    return SVT_AMD_ERR_BAD_PARAM;
}

extern "C" int svt_amd_md_encode_picture(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdPicture *P, const SvtAmdMdLcu *lcus, const uint8_t *src_y,
                                         uint32_t stride_y, const uint8_t *src_cb, const uint8_t *src_cr, uint32_t stride_c, const SvtAmdOisLcuResult *ois,
                                         int ois_slot, const SvtAmdCabacCost *cost, SvtAmdMdLcuOut *md_out, SvtAmdLcuWork *works, SvtAmdLcuResult *results)
{
    if (!cost)
        return md_refuse_unbound(pic);
    return md_encode_picture(ctx, pic, P, nullptr, lcus, src_y, stride_y, src_cb, src_cr, stride_c, ois, ois_slot, nullptr, -1, nullptr, cost, md_out, works, results, 1);
}
extern "C" int svt_amd_md_encode_picture16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdPicture *P, const SvtAmdMdLcu *lcus, const uint16_t *src_y,
                                           uint32_t stride_y, const uint16_t *src_cb, const uint16_t *src_cr, uint32_t stride_c, const SvtAmdOisLcuResult *ois,
                                           int ois_slot, const SvtAmdCabacCost *cost, SvtAmdMdLcuOut *md_out, SvtAmdLcuWork16 *works, SvtAmdLcuResult16 *results)
{
    if (!cost)
        return md_refuse_unbound(pic);
    return md_encode_picture(ctx, pic, P, nullptr, lcus, src_y, stride_y, src_cb, src_cr, stride_c, ois, ois_slot, nullptr, -1, nullptr, cost, md_out, works, results, 2);
}

extern "C" int svt_amd_md_encode_picture_inter(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdPicture *P, const SvtAmdMdInter *X, const SvtAmdMdLcu *lcus,
                                               const uint8_t *src_y, uint32_t stride_y, const uint8_t *src_cb, const uint8_t *src_cr, uint32_t stride_c,
                                               const SvtAmdOisLcuResult *ois, int ois_slot, const SvtAmdMeLcuResult *me, int me_slot, const SvtAmdTmvpLcu *tmvp,
                                               SvtAmdMdLcuOut *md_out, SvtAmdLcuWork *works, SvtAmdLcuResult *results)
{
    if (!X)
        return md_refuse_unbound(pic);
    return md_encode_picture(ctx, pic, P, X, lcus, src_y, stride_y, src_cb, src_cr, stride_c, ois, ois_slot, me, me_slot, tmvp, nullptr, md_out, works, results, 1);
}
extern "C" int svt_amd_md_encode_picture_inter16(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdPicture *P, const SvtAmdMdInter *X, const SvtAmdMdLcu *lcus,
                                                 const uint16_t *src_y, uint32_t stride_y, const uint16_t *src_cb, const uint16_t *src_cr, uint32_t stride_c,
                                                 const SvtAmdOisLcuResult *ois, int ois_slot, const SvtAmdMeLcuResult *me, int me_slot, const SvtAmdTmvpLcu *tmvp,
                                                 SvtAmdMdLcuOut *md_out, SvtAmdLcuWork16 *works, SvtAmdLcuResult16 *results)
{
    if (!X)
        return md_refuse_unbound(pic);
    return md_encode_picture(ctx, pic, P, X, lcus, src_y, stride_y, src_cb, src_cr, stride_c, ois, ois_slot, me, me_slot, tmvp, nullptr, md_out, works, results, 2);
}

/* ---- the stream-ordered launch on device inputs (include/svt_hevc_amd.h: svt_amd_md_encode_picture_launch) ---- */
#define MDL_ENTRY "svt_amd_md_encode_picture_launch"
#define MDL_BAD(...) do { svt_amd_set_error(MDL_ENTRY ": " __VA_ARGS__); return SVT_AMD_ERR_BAD_PARAM; } while (0)

extern "C" int svt_amd_md_encode_picture_launch(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdLaunchJob *job, SvtAmdMdLaunchStatus *d_status)
{
    /* a binding of svt_amd_md_picture_set_controls / _set_motion_field waits for a blocking call: this one consumes it, as every call on the object does, and refuses */
    const bool pending = pic && (pic->md_bound_lcus || pic->md_bound_tmvp);
    if (pic)
        pic->md_bound_lcus = nullptr, pic->md_bound_tmvp = nullptr;
    if (!ctx || !pic || !job)
        MDL_BAD("a context, a picture object and a job");
    if (pending)
        MDL_BAD("a device array is bound to the picture object (svt_amd_md_picture_set_controls / _set_motion_field): the job carries the arrays; the binding is dropped");
    const SvtAmdMdPicture *P = job->P;
    const SvtAmdMdInter *X = job->X;
    if (job->pad[0] || job->pad[1] || (job->flags & ~SVT_AMD_MD_LAUNCH_DECIDE_ONLY))
        MDL_BAD("a pad word is not 0, or unknown flags 0x%x", job->flags);
    if (!P || !job->d_lcus || !job->d_src[0] || !job->d_src[1] || !job->d_src[2])
        MDL_BAD("the job has no %s", !P ? "picture controls" : !job->d_lcus ? "device array of LCU controls" : "source planes");
    if ((job->flags & SVT_AMD_MD_LAUNCH_DECIDE_ONLY) && !X)
        MDL_BAD("SVT_AMD_MD_LAUNCH_DECIDE_ONLY is the P / B call without work records: an I picture has no such form");
    if (((uintptr_t)job->d_src[0] | (uintptr_t)job->d_src[1] | (uintptr_t)job->d_src[2] | (uintptr_t)d_status) & 3)
        MDL_BAD("source planes at %p, %p, %p and the status record at %p have to be 4-byte aligned", job->d_src[0], job->d_src[1], job->d_src[2], (void *)d_status);
    if (job->src_pitch_y < P->width || job->src_pitch_c < P->width / 2u)
        MDL_BAD("source pitches %u / %u below the plane widths of a %u samples wide picture", job->src_pitch_y, job->src_pitch_c, P->width);
    if ((X ? !md_picture_supported_inter(P, X) : !md_picture_supported(P)) || P->width != pic->d.width || P->height != pic->d.height)
        MDL_BAD("picture outside what this revision covers (svt_amd_md_picture_supported[_inter]), or not the picture object's size");
    const uint32_t bps = pic->d.bps;
    if (X && bps != 1 && !md_picture_supported_inter16(P, X))
        MDL_BAD("use_subpel 0 on a 16-bit picture object - a picture coded without sub-sample search predicts through the reference's interpolation-free path, which this "
                "revision covers for 8-bit pictures only");
    if ((job->src_pitch_y * bps) % 4 || (job->src_pitch_c * bps) % 4)
        MDL_BAD("source pitches of %u / %u samples of %u bytes: rows have to start 4-byte aligned", job->src_pitch_y, job->src_pitch_c, bps);
    const int n = pic->nlcu, wl = (pic->d.width + 63) / 64, hl = (pic->d.height + 63) / 64;
    if (job->tiles < 1 || job->tiles > (uint32_t)n)
        MDL_BAD("%u tiles in a picture of %d LCUs", job->tiles, n);
    if (!X && !job->cost && !pic->has_cost)
        MDL_BAD("no rate tables: the job has none and the picture object holds none (svt_amd_encdec_picture_set_inter)");
    if (X && ((!job->cost && !pic->has_cost) || !pic->has_ref[0] || (P->slice_type == 0 && !pic->has_ref[1]) || (X->tmvp_enable && !job->d_tmvp)))
        MDL_BAD("reference pictures / rate tables not set (svt_amd_encdec_picture_set_inter), or no co-located motion field");
    if (X && X->tmvp_enable && (uintptr_t)job->d_tmvp % 8)
        MDL_BAD("the motion field at %p is not 8-byte aligned", (const void *)job->d_tmvp);
    if (pic->md_rect_n)
        MDL_BAD("the picture object has a rank rectangle (svt_amd_encdec_picture_set_rect): the rectangle's tile-border check reads host records");
    MdSlotRecords rec = {ctx->parent ? ctx->parent : ctx, {nullptr, nullptr}, {-1, -1}};
    const SvtAmdMeLcuResult *d_me = X ? job->d_me : nullptr;
    if (X && !d_me && !(d_me = (const SvtAmdMeLcuResult *)md_slot_records(&rec, pic, 0, job->me_slot, MDL_ENTRY)))
        return SVT_AMD_ERR_BAD_PARAM;
    const SvtAmdOisLcuResult *d_ois = job->d_ois;
    if (!d_ois && !(d_ois = (const SvtAmdOisLcuResult *)md_slot_records(&rec, pic, 1, job->ois_slot, MDL_ENTRY)))
        return SVT_AMD_ERR_BAD_PARAM;

    /* ---- nothing below reads host memory after the call has returned, copies or waits ---- */
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = svt_amd_md_kernel_rate_tables(ctx->device);
    if (rc)
        return rc;
    SvtAmdMdState *m = nullptr;
    if ((rc = md_state(pic, &m)) != 0) /* allocates at the first call on the object */
        return rc;
    hipStream_t st = svt_amd_ctx_stream(ctx);
    if ((rc = md_records_wait(ctx, rec)) != 0)
        return rc;
    /* the source: the caller's planes into the object's own, at the object's pitch (the blocking call's strided form) */
    MdSourcePlanes S;
    memset(&S, 0, sizeof(S));
    for (int k = 0; k < 3; k++) {
        S.src[k] = job->d_src[k];
        S.dst[k] = bps == 2 ? (void *)m->d_src16[k] : (void *)m->d_src[k], S.view[k] = bps == 2 ? m->d_src[k] : nullptr;
        m->d.src[k] = m->d_src[k], m->d.src16[k] = bps == 2 ? m->d_src16[k] : nullptr;
    }
    S.src_pitch[0] = job->src_pitch_y, S.src_pitch[1] = job->src_pitch_c, S.dst_pitch[0] = pic->d.pitch[0], S.dst_pitch[1] = pic->d.pitch[1];
    S.width = pic->d.width, S.height = pic->d.height;
    m->d.src_pitch[0] = pic->d.pitch[0], m->d.src_pitch[1] = pic->d.pitch[1];
    if ((rc = svt_amd_mdlaunch_source(ctx, &S, (int)bps)) != 0)
        return rc;
    if ((rc = md_reference_views(st, pic, m, X != nullptr)) != 0)
        return rc;
    /* the small inputs and the descriptor: by value, in k_md_stage's argument block */
    if (job->cost)
        pic->has_cost = true;
    m->d.X = X ? m->d_X : nullptr, m->d.me = d_me, m->d.tmvp = X ? (X->tmvp_enable ? job->d_tmvp : m->d_tmvp) : nullptr;
    md_descriptor_common(pic, m);
    m->d.encode = !X || !(job->flags & SVT_AMD_MD_LAUNCH_DECIDE_ONLY);
    m->d.ois = d_ois, m->d.lcus = job->d_lcus;
    MdStagePart parts[4];
    int nparts = 0;
    parts[nparts++] = MdStagePart{m->d_P, P, sizeof(*P)};
    if (X)
        parts[nparts++] = MdStagePart{m->d_X, X, sizeof(*X)};
    if (job->cost)
        parts[nparts++] = MdStagePart{pic->d_cost, job->cost, sizeof(*job->cost)};
    parts[nparts++] = MdStagePart{m->d_D, &m->d, sizeof(m->d)};
    if ((rc = svt_amd_mdlaunch_stage(ctx, parts, nparts)) != 0)
        return rc;
    /* the controls: judged where they lie; the gate opens or closes both kernels' ticket counters */
    pic->epoch++;
    pic->deblocked = pic->sao_done = false;
    pic->md_works_whole = false; /* until everything is queued: a launch that fails half-way leaves arrays no consumer may take */
    const SvtAmdMdCtlCheck *d_check = nullptr;
    if ((rc = svt_amd_mdctl_check_device(ctx, job->d_lcus, n, P->depth_mode, X != nullptr, &d_check)) != 0)
        return rc;
    if ((rc = svt_amd_mdlaunch_gate(ctx, d_check, m->d_md_ticket, pic->d_sync, (unsigned)n, d_status)) != 0)
        return rc;
    if ((rc = md_reset_arrays(st, pic, m, X != nullptr)) != 0)
        return rc;
    /* a launch cannot wait for the blocking calls' workgroup budget (MdFlight) and holds none of it: the lone picture's width when the budget shows no flight now */
    const MdWidths width = md_launch_widths(wl, hl, (int)job->tiles, n);
    int flights;
    {
        std::lock_guard<std::mutex> l(g_flight_mu);
        flights = g_flight_dev[ctx->device & 63].flights;
    }
    m->ifree = X && !X->use_subpel;
    if ((rc = md_queue_picture(ctx, pic, m, rec, X != nullptr, flights == 0 ? width.lone : width.narrow, n, pic->d_sync + 1 + n, (int)job->tiles)) != 0)
        return rc;
    pic->md_works_whole = m->d.encode != 0; /* at queue time: the tail and the motion field queue behind this launch in stream order */
    return SVT_AMD_OK;
}

extern "C" int svt_amd_encdec_picture_md_records(SvtAmdEncDecPicture *pic, const SvtAmdMdLcuOut **d_out, const void **d_works, size_t *work_stride, const void **d_results,
                                                 size_t *result_stride)
{
    if (!pic || !pic->md) {
        svt_amd_set_error("svt_amd_encdec_picture_md_records: %s", pic ? "no mode-decision call has run on the picture object" : "a picture object");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    const SvtAmdMdState *m = pic->md;
    if (d_out)
        *d_out = m->d_out;
    if (d_works)
        *d_works = m->d_works;
    if (work_stride)
        *work_stride = m->work_bytes;
    if (d_results)
        *d_results = m->d_results;
    if (result_stride)
        *result_stride = m->result_bytes;
    return SVT_AMD_OK;
}

/* debug: stage clocks of the mode-decision kernel.  First call (out == NULL or not): switches the collection on for the picture object's later
 * calls; with out: 16 sums per LCU - [0] the LCU's surroundings into LDS, [1] lane 0: contexts + candidates, [2] the intra reference, [3] fast loop,
 * [4] lane 0: fast costs + candidate buffers, [5] full loop, [6] lane 0: costs + decision, [7] reconstruction + inter-depth decision, [8] neighbour
 * update + next unit, [9] state leaving LDS, [10] work record (+ merge / skip decisions), [11] encode pass, [12] waiting for neighbours, [15] calls */
extern "C" int svt_amd_debug_md_profile(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, unsigned long long *out)
{
    if (!ctx || !pic)
        return SVT_AMD_ERR_BAD_PARAM;
    HIP_TRY(hipSetDevice(ctx->device));
    SvtAmdMdState *m = nullptr;
    const int rc = md_state(pic, &m);
    if (rc)
        return rc;
    const size_t bytes = sizeof(unsigned long long) * 16 * (size_t)pic->nlcu;
    if (!m->d_prof) {
        HIP_TRY(hipMalloc((void **)&m->d_prof, 10 * bytes)); /* stage sums of every LCU, then sub-stage sums of every LCU, then both by unit depth (4 x 32 per LCU) */
        HIP_TRY(hipMemset(m->d_prof, 0, 10 * bytes));
    }
    if (out) {
        HIP_TRY(svt_amd_ctx_sync(ctx));
        HIP_TRY(hipMemcpy(out, m->d_prof, bytes, hipMemcpyDeviceToHost));
    }
    return SVT_AMD_OK;
}

/* measurement: duration (HIP events on the call's stream) and launch width of the picture object's last k_md_picture launch */
extern "C" int svt_amd_debug_md_kernel_ms(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, float *ms, int *workgroups)
{
    if (!ctx || !pic || !pic->md || !ms)
        return SVT_AMD_ERR_BAD_PARAM;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventSynchronize(pic->md->ev_k1));
    HIP_TRY(hipEventElapsedTime(ms, pic->md->ev_k0, pic->md->ev_k1));
    if (workgroups)
        *workgroups = pic->md->grid;
    return SVT_AMD_OK;
}

/* measurement: duration of the encode-pass kernel that followed the picture object's last mode-decision launch (0 when the call asked for decisions only) */
extern "C" int svt_amd_debug_md_ep_ms(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, float *ms)
{
    if (!ctx || !pic || !pic->md || !ms)
        return SVT_AMD_ERR_BAD_PARAM;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventSynchronize(pic->md->ev_k2));
    HIP_TRY(hipEventElapsedTime(ms, pic->md->ev_k1, pic->md->ev_k2));
    return SVT_AMD_OK;
}

extern "C" int svt_amd_debug_md_flights(int *in_flight, int *workgroups_held, int *waiting)
{
    std::lock_guard<std::mutex> l(g_flight_mu);
    int fl = 0, wg = 0;
    for (const FlightDevice &fd : g_flight_dev)
        fl += fd.flights, wg += fd.wgs;
    if (in_flight)
        *in_flight = fl;
    if (workgroups_held)
        *workgroups_held = wg;
    if (waiting)
        *waiting = (int)g_flight_wait.size();
    return SVT_AMD_OK;
}
extern "C" int svt_amd_debug_md_kernel_lds_bytes(int inter, int bytes_per_sample)
{
    (void)bytes_per_sample; /* (MdShared does not depend on the sample width) */
    return svt_amd_md_kernel_lds_bytes(inter);
}

extern "C" int svt_amd_debug_md_lists_batch(SvtAmdContext *ctx, const SvtAmdMdListJob *d_jobs, const SvtAmdTmvpLcu *d_pool, SvtAmdMdListOut *d_outs, uint32_t n)
{
    if (!ctx || !d_jobs || !d_pool || !d_outs || n == 0) {
        svt_amd_set_error("svt_amd_debug_md_lists_batch: a context, three device arrays and at least one job");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    return svt_amd_md_kernel_lists_batch(svt_amd_ctx_stream(ctx), d_jobs, d_pool, d_outs, n);
}

/* debug: the finer marks of the mode-decision kernel (MD_SUB): 16 sums per LCU, collected together with svt_amd_debug_md_profile's (which switches the collection on) */
extern "C" int svt_amd_debug_md_profile_sub(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, unsigned long long *out)
{
    if (!ctx || !pic || !pic->md || !pic->md->d_prof || !out)
        return SVT_AMD_ERR_BAD_PARAM;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(svt_amd_ctx_sync(ctx));
    const size_t bytes = sizeof(unsigned long long) * 16 * (size_t)pic->nlcu;
    HIP_TRY(hipMemcpy(out, pic->md->d_prof + 16 * (size_t)pic->nlcu, bytes, hipMemcpyDeviceToHost));
    return SVT_AMD_OK;
}

/* debug (-DMD_TRACE builds): lane-0 time stamps of the four waves along the unit chain of LCU `lcu`, units [unit, unit + 2) of its leaf list.  out == NULL: arms the picture
 * object's later calls; with out: [4 waves][1 + 128] words - the count, then (mark << 48 | shader clock) */
extern "C" int svt_amd_debug_md_trace(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, int lcu, int unit, unsigned long long *out)
{
    const size_t bytes = sizeof(unsigned long long) * (size_t)svt_amd_md_kernel_trace_words();
    if (!bytes || !ctx || !pic) /* (no trace build of the kernel unit: nothing to arm or read) */
        return SVT_AMD_ERR_BAD_PARAM;
    HIP_TRY(hipSetDevice(ctx->device));
    SvtAmdMdState *m = nullptr;
    const int rc = md_state(pic, &m);
    if (rc)
        return rc;
    if (!m->d_trace)
        HIP_TRY(hipMalloc((void **)&m->d_trace, bytes));
    if (out) {
        HIP_TRY(svt_amd_ctx_sync(ctx));
        HIP_TRY(hipMemcpy(out, m->d_trace, bytes, hipMemcpyDeviceToHost));
    } else {
        HIP_TRY(hipMemset(m->d_trace, 0, bytes));
        m->trace_lcu = lcu, m->trace_unit = unit;
    }
    return SVT_AMD_OK;
}

/* debug: the picture object's later mode-decision calls run the 16x16 / 32x32 forward transforms of the full loops on the register butterflies (on != 0) instead of the
 * matrix cores - the path a unit outside the matrix form's wrap-free domain takes, which no 8-bit picture reaches by itself */
extern "C" int svt_amd_debug_md_force_butterflies(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, int on)
{
    if (!ctx || !pic)
        return SVT_AMD_ERR_BAD_PARAM;
    HIP_TRY(hipSetDevice(ctx->device));
    SvtAmdMdState *m = nullptr;
    const int rc = md_state(pic, &m);
    if (rc)
        return rc;
    m->force_butterflies = on != 0;
    return SVT_AMD_OK;
}

/* debug: the stage and sub-stage sums by the depth of the unit they were spent on: [LCU][depth 0..3][32] (slots 0..15 as svt_amd_debug_md_profile, 16..31 as _sub) */
extern "C" int svt_amd_debug_md_profile_depth(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, unsigned long long *out)
{
    if (!ctx || !pic || !pic->md || !pic->md->d_prof || !out)
        return SVT_AMD_ERR_BAD_PARAM;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(svt_amd_ctx_sync(ctx));
    HIP_TRY(hipMemcpy(out, pic->md->d_prof + 32 * (size_t)pic->nlcu, sizeof(unsigned long long) * 128 * (size_t)pic->nlcu, hipMemcpyDeviceToHost));
    return SVT_AMD_OK;
}

extern "C" int svt_amd_md_picture_set_controls(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdMdLcu *d_lcus)
{
    if (!ctx || !pic) {
        svt_amd_set_error("svt_amd_md_picture_set_controls: a context and a picture object");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    pic->md_bound_lcus = d_lcus;
    return SVT_AMD_OK;
}

extern "C" int svt_amd_md_picture_set_motion_field(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, const SvtAmdTmvpLcu *d_field)
{
    if (!ctx || !pic) {
        svt_amd_set_error("svt_amd_md_picture_set_motion_field: a context and a picture object");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    if ((uintptr_t)d_field % 8) {
        svt_amd_set_error("svt_amd_md_picture_set_motion_field: the field at %p is not 8-byte aligned", (const void *)d_field);
        return SVT_AMD_ERR_BAD_PARAM;
    }
    pic->md_bound_tmvp = d_field;
    return SVT_AMD_OK;
}

/* the records the mode-decision calls on `pic` leave in HBM, for the picture tail (tail_kernels.hip) */
int svt_amd_md_picture_records(const SvtAmdEncDecPicture *pic, const void **d_works, size_t *work_stride, const void **d_results, size_t *result_stride)
{
    if (!pic->md)
        return 0;
    *d_works = pic->md->d_works, *work_stride = pic->md->work_bytes, *d_results = pic->md->d_results, *result_stride = pic->md->result_bytes;
    return 1;
}

/* the field and the intra-coded area of the picture the last mode-decision call on `pic` decided, from the work records it left in HBM (tmvp_kernels.hip) */
extern "C" int svt_amd_encdec_picture_motion_field(SvtAmdContext *ctx, SvtAmdEncDecPicture *pic, int slice_type, const uint64_t ref_poc[2], SvtAmdTmvpLcu *d_field,
                                                   SvtAmdRefStats *d_stats)
{
    if (!ctx || !pic || !d_field) {
        svt_amd_set_error("svt_amd_encdec_picture_motion_field: a context, a picture object and a device array for the field");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    if (slice_type < 0 || slice_type > 2 || (!ref_poc && slice_type != 2)) {
        svt_amd_set_error("svt_amd_encdec_picture_motion_field: slice type %d%s", slice_type, ref_poc ? "" : " without reference POCs");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    if (pic->md_rect_n) {
        svt_amd_set_error("svt_amd_encdec_picture_motion_field: the picture object has a rank rectangle (svt_amd_encdec_picture_set_rect): the work records of its other LCUs "
                          "are zeroed");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    if (!pic->md || !pic->md_works_whole) {
        svt_amd_set_error("svt_amd_encdec_picture_motion_field: no svt_amd_md_encode_picture* call that writes work records has completed on the picture object");
        return SVT_AMD_ERR_BAD_PARAM;
    }
    SvtAmdMotionFieldJob job;
    memset(&job, 0, sizeof(job));
    job.d_works = pic->md->d_works, job.work_stride = pic->md->work_bytes;
    job.width = pic->d.width, job.height = pic->d.height, job.slice_type = (uint8_t)slice_type;
    if (ref_poc)
        job.ref_poc[0] = ref_poc[0], job.ref_poc[1] = ref_poc[1];
    return svt_amd_motion_field_launch(ctx, &job, d_field, d_stats);
}
