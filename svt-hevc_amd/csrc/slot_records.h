/*
 * slot_records.h - what a picture slot knows about the ME / OIS records in its buffers and who is ordered behind whom ("Lanes and the records they
 * leave in the slots"): one lock per slot, plain fields under it, one kind of marker for the three directions.  Nothing here calls HIP: the functions decide,
 * context.hip issues the stream operation under the same lock (tests/slot_records_check.cpp runs this file alone).
 */
#ifndef SVT_AMD_SLOT_RECORDS_H
#define SVT_AMD_SLOT_RECORDS_H
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <string.h>

struct SvtAmdContext;
/* The completion marker of a launch, borrowed from the ring of the lane that recorded it (SvtAmdContext::ev_launch).  ev == nullptr: nothing to wait for (no
 * launch since the last upload, or the lane is finished and gone). */
struct LaunchMark { hipEvent_t ev; struct SvtAmdContext *lane; };
/* SLOT_ME / SLOT_OIS: behind the kernels that wrote d_me_out / d_ois_out - a reader on another lane waits on it.  SLOT_READ: behind a kernel that read the
 * records in place - the next launch INTO the slot from another lane waits on it. */
enum { SLOT_ME = 0, SLOT_OIS = 1, SLOT_READ = 2, SLOT_MARKS = 3 };
#define SLOT_COV_LCUS (64u * 128u) /* a bit per LCU (8K: 8,160) */

struct SlotRecords { /* lanes run on different host threads: every field is read and written under `lock` only */
    int lock;
    LaunchMark mark[SLOT_MARKS];
    uint32_t me_lcus, ois_lcus; /* LCUs of the picture whose records the buffers hold (0: none yet, or only a part of the picture) */
    uint64_t me_cov[SLOT_COV_LCUS / 64]; /* the LCUs of the slot's CURRENT picture the ME launches since the last upload wrote: bands come in any order, from several lanes */
    uint32_t me_cov_count;
};

static inline void slot_lock(SlotRecords *r) { while (__atomic_exchange_n(&r->lock, 1, __ATOMIC_ACQUIRE)) {} }
static inline void slot_unlock(SlotRecords *r) { __atomic_store_n(&r->lock, 0, __ATOMIC_RELEASE); }

/* ---- these three take the lock themselves ---- */
/* A new picture enters the slot: the records belong to the previous one, and no reader is let at them, so there is no launch to order one behind.  The read
 * marker stays: a kernel may still be reading the previous picture's records where the next launch will write. */
static inline void slot_records_forget(SlotRecords *r)
{
    slot_lock(r);
    r->me_lcus = r->ois_lcus = r->me_cov_count = 0;
    memset(r->me_cov, 0, sizeof(r->me_cov));
    r->mark[SLOT_ME] = r->mark[SLOT_OIS] = LaunchMark{nullptr, nullptr};
    slot_unlock(r);
}
/* `lane` is finished and its ring about to be destroyed */
static inline void slot_forget_lane(SlotRecords *r, const struct SvtAmdContext *lane)
{
    slot_lock(r);
    for (int k = 0; k < SLOT_MARKS; k++)
        if (r->mark[k].lane == lane)
            r->mark[k] = LaunchMark{nullptr, nullptr};
    slot_unlock(r);
}
static inline uint32_t slot_lcus(SlotRecords *r, int which)
{
    slot_lock(r);
    const uint32_t n = which ? r->ois_lcus : r->me_lcus;
    slot_unlock(r);
    return n;
}

/* ---- the caller holds the lock ---- */
/* A launch wrote the ME records of LCUs [begin, end) of a picture of n: the slot holds the picture's records once the launches since the last upload cover it. */
static inline void slot_me_cover(SlotRecords *r, uint32_t n, uint32_t begin, uint32_t end)
{
    for (uint32_t i = begin; i < end && i < n && i < SLOT_COV_LCUS; i++)
        if (!((r->me_cov[i >> 6] >> (i & 63)) & 1ull))
            r->me_cov[i >> 6] |= 1ull << (i & 63), r->me_cov_count++;
    r->me_lcus = r->me_cov_count >= n ? n : 0u;
}
/* What a lane waits on before it reads (SLOT_ME / SLOT_OIS) or writes (SLOT_READ) the slot's records: the held marker unless it is null or its own. */
static inline hipEvent_t slot_wait_for(const SlotRecords *r, int kind, const struct SvtAmdContext *lane)
{
    return r->mark[kind].lane != lane ? r->mark[kind].ev : nullptr;
}
/* The marker chain.  `lane` is about to lend the slot a new marker of `kind`: the event its stream waits on first, so that the new marker stands for
 * everything the held one stood for as well - or nullptr.  The held marker matters when it is another lane's and
 *  SLOT_ME:   earlier launches cover a part of the current picture and this one (`whole`: it writes every LCU) does not replace them;
 *  SLOT_OIS:  never - an OIS launch writes the whole picture;
 *  SLOT_READ: always.
 * Call it before slot_me_cover counts this launch in. */
static inline hipEvent_t slot_chain_behind(const SlotRecords *r, int kind, const struct SvtAmdContext *lane, bool whole)
{
    return kind == SLOT_READ || (kind == SLOT_ME && !whole && r->me_cov_count) ? slot_wait_for(r, kind, lane) : nullptr;
}

#endif
