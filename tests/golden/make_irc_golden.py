#!/usr/bin/env python3
"""Generate the initial-rate-control fixtures from the REFERENCE itself.  The per-LCU checks and the final stationary-edge stage are `static`
(Codec/EbMotionEstimationProcess.c, Codec/EbSourceBasedOperationsProcess.c), and so are the four vector tests of Codec/EbInitialRateControlProcess.c, so two small
C drivers of our own are written into a temporary directory; each #includes reference source files by path and links against oracle/_ref/libsvtref.so.  They
fill calloc'd SequenceControlSet_t / PictureParentControlSet_t objects (lcuParamsArray by the reference's own LcuParamsInit) from the seeded records of
tests/irc_records.py, one control set per picture of the sequence:
  driver A  StationaryEdgeOverUpdateOverTimeLcuPart1 of every LCU of every picture, and Part2 under the condition of the ME process (:811), on an LcuStat_t
            cleared as the EB_MEMSET of EdgeDetectionMeanLumaChroma16x16 leaves it.
  driver B  takes those checks and the seeded edge_cu bits (EdgeDetectionMeanLumaChroma16x16's result is an input: the padetect_* fixtures pin it) into the
            LcuStat_t of every picture, calls EbHevcMeBasedGlobalMotionDetection for each as the kernel does on arrival, builds the real reorder queue - the
            sequence starts where the case says, so the head stands once at the last index - and then, picture by picture from the head, calls the reference's
            functions in the order and under the conditions of InitialRateControlKernel (:1012-1062) and SourceBasedOperationsKernel (:1575).  The kernel
            functions themselves cannot be called (they block on the encoder's queues): the window count framesInSw (:941-959), those conditions and the
            step of the head (:1110-1116) are written here in the driver's own words, on the reference's own fields - no statement of the reference is kept
            in this file.  EbHevcDetectGlobalMotion keeps its five totals in locals: the driver counts them again with the reference's own CheckMvFor*
            functions and checks that they give the flags the reference stored.  The reference's two walks keep what they met in locals too: the driver
            records what stands in the reference's queue where they pass (hom_walked, edge_places), so that the non-vacuity list below needs no restatement.
Nothing compiled is kept.
  -> tests/golden/irc_<name>.npz: the case name and results only (a few KiB each).  Needs the reference tree and `make -C oracle ref`.
Usage: python tests/golden/make_irc_golden.py [name ...]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import irc_numpy as N  # noqa: E402
import irc_records as R  # noqa: E402
import svtlib as S  # noqa: E402

REF_SRC = os.environ.get("SVT_REF_SOURCE", "/root/reference/Source")

COMMON = r"""
#include <stdio.h>
static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) exit(3); }
static void get(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) exit(4); }
extern EB_ERRORTYPE LcuParamsInit(SequenceControlSet_t *sequenceControlSetPtr);
static SequenceControlSet_t *make_scs(uint32_t w, uint32_t h, uint32_t cls, uint32_t lad)
{
    SequenceControlSet_t *scs = calloc(1, sizeof(*scs));
    scs->lumaWidth = w, scs->lumaHeight = h, scs->lcuSize = 64;
    scs->pictureWidthInLcu = (w + 63) / 64, scs->pictureHeightInLcu = (h + 63) / 64, scs->lcuTotalCount = scs->pictureWidthInLcu * scs->pictureHeightInLcu;
    scs->inputResolution = cls;
    scs->staticConfig.lookAheadDistance = lad;
    LcuParamsInit(scs);
    return scs;
}
"""

DRIVER_A = r"""
#include "EbMotionEstimationProcess.c"
""" + COMMON + r"""
int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    uint32_t hd[5];
    if (argc < 3 || !fi || !fo) return 2;
    get(fi, hd, sizeof(hd));
    const uint32_t w = hd[0], h = hd[1], cls = hd[2], pictures = hd[3], lad = hd[4];
    SequenceControlSet_t *scs = make_scs(w, h, cls, lad);
    const uint32_t lcus = scs->lcuTotalCount;
    PictureParentControlSet_t *pcs = calloc(1, sizeof(*pcs));
    pcs->variance = calloc(lcus, sizeof(void *)), pcs->meResults = calloc(lcus, sizeof(void *));
    for (uint32_t i = 0; i < lcus; i++)
        pcs->variance[i] = calloc(MAX_ME_PU_COUNT, 2), pcs->meResults[i] = calloc(MAX_ME_PU_COUNT, sizeof(MeCuResults_t));
    pcs->lcuStatArray = calloc(lcus, sizeof(LcuStat_t));
    for (uint32_t i = 0; i < lcus; i++) {
        uint8_t geo[2] = {scs->lcuParamsArray[i].isCompleteLcu, scs->lcuParamsArray[i].potentialLogoLcu};
        put(fo, geo, 2);
    }
    for (uint32_t k = 0; k < pictures; k++) {
        uint32_t p[3];
        get(fi, p, sizeof(p));
        pcs->sliceType = p[0] == 0 ? EB_I_PICTURE : p[0] == 1 ? EB_P_PICTURE : EB_B_PICTURE;
        pcs->temporalLayerIndex = p[1], pcs->endOfSequenceFlag = p[2];
        for (uint32_t i = 0; i < lcus; i++) {
            uint16_t var[4];
            int16_t mv[2];
            uint32_t dist;
            get(fi, var, 8), get(fi, mv, 4), get(fi, &dist, 4);
            for (int q = 0; q < 4; q++)
                pcs->variance[i][ME_TIER_ZERO_PU_32x32_0 + q] = var[q];
            pcs->meResults[i][0].xMvL0 = mv[0], pcs->meResults[i][0].yMvL0 = mv[1], pcs->meResults[i][0].distortionDirection[0].distortion = dist;
            memset(&pcs->lcuStatArray[i], 0, sizeof(LcuStat_t));     /* EdgeDetectionMeanLumaChroma16x16's EB_MEMSET */
        }
        for (uint32_t i = 0; i < lcus; i++) {                        /* Codec/EbMotionEstimationProcess.c:804-816 */
            StationaryEdgeOverUpdateOverTimeLcuPart1(scs, pcs, i);
            if (lad != 0 && p[2] == 0)                               /* Part2 only for a picture with a look-ahead: not the last of the sequence */
                StationaryEdgeOverUpdateOverTimeLcuPart2(scs, pcs, i);
            const LcuStat_t *ls = &pcs->lcuStatArray[i];
            uint8_t o[4] = {ls->check1ForLogoStationaryEdgeOverTimeFlag, ls->pmCheck1ForLogoStationaryEdgeOverTimeFlag, ls->check2ForLogoStationaryEdgeOverTimeFlag,
                            ls->lowDistLogo};
            put(fo, o, 4);
        }
    }
    fclose(fo);
    return 0;
}
"""

DRIVER_B = r"""
#include "EbSourceBasedOperationsProcess.c"
#include "EbInitialRateControlProcess.c"
#include "EbPredictionStructure.h"
""" + COMMON + r"""
static PictureParentControlSet_t *pcs_at(const InitialRateControlReorderEntry_t *place)      /* NULL: the place is empty */
{
    return place->parentPcsWrapperPtr ? (PictureParentControlSet_t *)place->parentPcsWrapperPtr->objectPtr : NULL;
}
int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    uint32_t hd[7];
    if (argc < 3 || !fi || !fo) return 2;
    get(fi, hd, sizeof(hd));
    const uint32_t w = hd[0], h = hd[1], cls = hd[2], pictures = hd[3], lad = hd[4], period = hd[5], head0 = hd[6];
    SequenceControlSet_t *scs = make_scs(w, h, cls, lad);
    const uint32_t lcus = scs->lcuTotalCount, wl = scs->pictureWidthInLcu;
    EncodeContext_t *enc = calloc(1, sizeof(*enc));
    scs->encodeContextPtr = enc;
    EbObjectWrapper_t *scs_wrap = calloc(1, sizeof(*scs_wrap));
    scs_wrap->objectPtr = scs;
    EbPictureBufferDesc_t enhanced = {0};
    PredictionStructure_t pred = {0};
    enhanced.width = w, enhanced.height = h;
    pred.predStructPeriod = period;
    /* the reorder queue, every entry empty as InitialRateControlReorderEntryCtor leaves it */
    enc->initialRateControlReorderQueue = calloc(INITIAL_RATE_CONTROL_REORDER_QUEUE_MAX_DEPTH, sizeof(void *));
    for (uint32_t q = 0; q < INITIAL_RATE_CONTROL_REORDER_QUEUE_MAX_DEPTH; q++) {
        enc->initialRateControlReorderQueue[q] = calloc(1, sizeof(InitialRateControlReorderEntry_t));
        enc->initialRateControlReorderQueue[q]->pictureNumber = q;
    }
    enc->initialRateControlReorderQueueHeadIndex = head0;
    PictureParentControlSet_t **all = calloc(pictures, sizeof(void *));
    for (uint32_t k = 0; k < pictures; k++) {
        uint32_t p[6];
        get(fi, p, sizeof(p));
        PictureParentControlSet_t *pcs = all[k] = calloc(1, sizeof(*pcs));
        pcs->sequenceControlSetWrapperPtr = scs_wrap, pcs->enhancedPicturePtr = &enhanced, pcs->predStructPtr = &pred;
        pcs->lcuTotalCount = lcus;
        pcs->pictureNumber = p[0];
        pcs->sliceType = p[1] == 0 ? EB_I_PICTURE : p[1] == 1 ? EB_P_PICTURE : EB_B_PICTURE;
        pcs->temporalLayerIndex = p[2], pcs->hierarchicalLevels = p[3], pcs->endOfSequenceFlag = p[4], pcs->sceneChangeFlag = p[5];
        pcs->variance = calloc(lcus, sizeof(void *)), pcs->meResults = calloc(lcus, sizeof(void *));
        pcs->lcuStatArray = calloc(lcus, sizeof(LcuStat_t));         /* cleared, as the EB_MEMSET of EdgeDetectionMeanLumaChroma16x16 leaves it */
        pcs->lcuVarianceOfVarianceOverTime = calloc(lcus, 8), pcs->isLcuHomogeneousOverTime = calloc(lcus, sizeof(EB_BOOL));
        for (uint32_t i = 0; i < lcus; i++) {
            uint8_t checks[4];
            uint16_t edge, var;
            int16_t mv[2];
            get(fi, checks, 4), get(fi, &edge, 2), get(fi, &var, 2), get(fi, mv, 4);
            pcs->variance[i] = calloc(MAX_ME_PU_COUNT, 2), pcs->meResults[i] = calloc(MAX_ME_PU_COUNT, sizeof(MeCuResults_t));
            pcs->variance[i][ME_TIER_ZERO_PU_64x64] = var;
            pcs->meResults[i][0].xMvL0 = mv[0], pcs->meResults[i][0].yMvL0 = mv[1];
            LcuStat_t *ls = &pcs->lcuStatArray[i];
            ls->check1ForLogoStationaryEdgeOverTimeFlag = checks[0], ls->pmCheck1ForLogoStationaryEdgeOverTimeFlag = checks[1];
            ls->check2ForLogoStationaryEdgeOverTimeFlag = checks[2], ls->lowDistLogo = checks[3];
            for (int u = 0; u < 16; u++)
                ls->cuStatArray[RASTER_SCAN_CU_INDEX_16x16_0 + u].edgeCu = edge >> u & 1;
        }
        /* on arrival (:896): the raw flags; the five totals again, with the reference's own tests.  A neighbour is asked for its vector where the LCU has
           one on that side and, to the right and below, where two whole LCUs still fit from the LCU's origin on (:261-294); elsewhere its vector is 0 / 0 */
        EbHevcMeBasedGlobalMotionDetection(scs, pcs);
        uint32_t tot[5] = {0, 0, 0, 0, 0};
        uint8_t *votes = calloc(lcus, 1);
        for (uint32_t i = 0; i < lcus && pcs->sliceType != EB_I_PICTURE; i++) {
            const uint32_t column = i % wl, line = i / wl;
            const int32_t side[4] = {column > 0 ? -1 : 0, line > 0 ? -(int32_t)wl : 0, 64 * column + 128 <= w ? 1 : 0, 64 * line + 128 <= h ? (int32_t)wl : 0};
            EB_S32 own[2] = {0, 0};
            uint8_t v = 0;
            if (!scs->lcuParamsArray[i].isCompleteLcu)
                continue;
            EbHevcGetMv(pcs, i, &own[0], &own[1]);
            for (int q = 0; q < 4; q++) {
                EB_S32 other[2] = {0, 0};
                if (side[q] != 0)
                    EbHevcGetMv(pcs, (uint32_t)((int32_t)i + side[q]), &other[0], &other[1]);
                v |= CheckMvForPan(pcs->hierarchicalLevels, pcs->temporalLayerIndex, &own[0], &own[1], &other[0], &other[1]) ? 1 : 0;
                v |= CheckMvForTilt(pcs->hierarchicalLevels, pcs->temporalLayerIndex, &own[0], &own[1], &other[0], &other[1]) ? 2 : 0;
                v |= CheckMvForPanHighAmp(pcs->hierarchicalLevels, pcs->temporalLayerIndex, &own[0], &other[0]) ? 4 : 0;
                v |= CheckMvForTiltHighAmp(pcs->hierarchicalLevels, pcs->temporalLayerIndex, &own[1], &other[1]) ? 8 : 0;
            }
            votes[i] = v;
            tot[0]++, tot[1] += v & 1, tot[2] += v >> 1 & 1, tot[3] += v >> 2 & 1, tot[4] += v >> 3 & 1;
        }
        uint8_t raw[2] = {pcs->isPan ? 1 : 0, pcs->isTilt ? 1 : 0};
        if (raw[0] != (tot[0] && tot[1] * 100 / tot[0] > PAN_LCU_PERCENTAGE) || raw[1] != (tot[0] && tot[2] * 100 / tot[0] > PAN_LCU_PERCENTAGE))
            return 5;                                                /* the totals do not give the flags the reference stored */
        put(fo, tot, sizeof(tot)), put(fo, raw, 2), put(fo, votes, lcus);
        /* into the queue (EbHevcDeterminePictureOffsetInQueue :745) */
        EbObjectWrapper_t *wr = calloc(1, sizeof(*wr));
        wr->objectPtr = pcs;
        InitialRateControlReorderEntry_t *e = enc->initialRateControlReorderQueue[(head0 + k) % INITIAL_RATE_CONTROL_REORDER_QUEUE_MAX_DEPTH];
        e->parentPcsWrapperPtr = wr, e->pictureNumber = pcs->pictureNumber;
    }
    InitialRateControlReorderEntry_t **ring = enc->initialRateControlReorderQueue;
    const uint32_t depth = INITIAL_RATE_CONTROL_REORDER_QUEUE_MAX_DEPTH;
    for (uint32_t k = 0; k < pictures; k++) {
        /* the picture at the head and its window (:933-968): the pictures that stand in the queue from the head on, lookAheadDistance + 1 of them at most,
           an end-of-sequence picture being the last one counted; the end-of-sequence picture itself has none */
        const uint32_t head = enc->initialRateControlReorderQueueHeadIndex;
        PictureParentControlSet_t *pcs = pcs_at(ring[head]);
        if (pcs == NULL)
            return 6;
        if (pcs != all[k])
            return 8;
        uint32_t window = 0;
        for (uint32_t step = 0; step <= lad && !pcs->endOfSequenceFlag; step++) {
            const PictureParentControlSet_t *later = pcs_at(ring[(head + step) % depth]);
            if (later == NULL)
                return 7;                                            /* the window is not full: the sequence of the case is wrong */
            window++;
            if (later->endOfSequenceFlag)
                break;
        }
        pcs->framesInSw = window;
        /* the branches of :1012-1062 and of Codec/EbSourceBasedOperationsProcess.c:1575: with a look-ahead the four stages over time in the reference's order,
           without one the picture's own motion flags and the reset records */
        const int ahead = lad != 0 && !pcs->endOfSequenceFlag;
        uint32_t toCheck = 1;
        if (ahead) {
            EbHevcUpdateGlobalMotionDetectionOverTime(enc, scs, pcs);
            EbHevcUpdateMotionFieldUniformityOverTime(enc, scs, pcs);
            UpdateHomogeneityOverTime(enc, pcs);
            toCheck = 2 * period + 1;                                /* the smallest of: two periods and a picture, the window, the look-ahead distance */
            toCheck = window < toCheck ? window : toCheck;
            toCheck = lad < toCheck ? lad : toCheck;
            StationaryEdgeOverUpdateOverTimeLcu(scs, toCheck, pcs, pcs->lcuTotalCount);
        } else {
            if (pcs->sliceType != EB_I_PICTURE)
                EbHevcDetectGlobalMotion(scs, pcs);
            ResetHomogeneityStructures(pcs);
        }
        /* what stands in the reference's queue where walks 4 and 5 pass: toCheck - 1 places from the head on - from place 0 on when the head is the last place.
           seen[0]: the places in front of a scene change or the sequence end; seen[1]: bit s set where place s is in front of the sequence end and holds a POC
           that is a multiple of 4 */
        uint32_t seen[2] = {0, 0};
        for (uint32_t s = 0, open4 = 1, open5 = 1; ahead && s + 1 < toCheck; s++) {
            const PictureParentControlSet_t *t = pcs_at(ring[((head == depth - 1 ? 0 : head) + s) % depth]);
            if (t == NULL)
                return 9;
            open4 = open4 && !t->endOfSequenceFlag, open5 = open5 && !t->endOfSequenceFlag && !t->sceneChangeFlag;
            seen[0] += open5;
            seen[1] |= (open4 && (t->pictureNumber & 3) == 0) << s;
        }
        /* ---- results ---- */
        uint8_t b[4] = {pcs->isPan ? 1 : 0, pcs->isTilt ? 1 : 0, pcs->picHomogenousOverTimeLcuPercentage, (uint8_t)toCheck};
        put(fo, b, 4), put(fo, seen, sizeof(seen));
        for (uint32_t i = 0; i < lcus; i++) {
            const LcuStat_t *ls = &pcs->lcuStatArray[i];
            uint16_t counts[32];
            for (int u = 0; u < 16; u++)
                counts[u] = ls->cuStatArray[RASTER_SCAN_CU_INDEX_16x16_0 + u].similarEdgeCount, counts[16 + u] = ls->cuStatArray[RASTER_SCAN_CU_INDEX_16x16_0 + u].pmSimilarEdgeCount;
            uint8_t f[3] = {ls->stationaryEdgeOverTimeFlag, ls->pmStationaryEdgeOverTimeFlag, pcs->isLcuHomogeneousOverTime[i] ? 1 : 0};
            put(fo, counts, sizeof(counts)), put(fo, &pcs->lcuVarianceOfVarianceOverTime[i], 8), put(fo, f, 3);
        }
        /* the picture leaves (:1110-1116): its place is free for the picture a whole ring later, the head moves to the next place */
        ring[head]->parentPcsWrapperPtr = NULL, ring[head]->pictureNumber += depth;
        enc->initialRateControlReorderQueueHeadIndex = (head + 1) % depth;
    }
    fclose(fo);
    return 0;
}
"""


def _compile(td, name, text):
    ref_dir = os.path.dirname(S.REF_SO)
    inc = [ref_dir] + [os.path.join(REF_SRC, d) for d in ("API", "Lib/Codec", "Lib/C_DEFAULT", "Lib/ASM_SSE2", "Lib/ASM_SSSE3", "Lib/ASM_SSE4_1", "Lib/ASM_AVX2")]
    src, exe = os.path.join(td, name + ".c"), os.path.join(td, name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-mavx2", "-msse4.1", "-w"] + ["-I" + i for i in inc] +
                          [src, "-o", exe, "-L" + ref_dir, "-lsvtref", "-Wl,-rpath," + ref_dir, "-lpthread", "-lm"])
    return exe


def run_case(name, exe_a, exe_b, td):
    w, h, cls, seed, seq = R.CASES[name]
    pics, n = seq["pics"], S.lcu_count(w, h)
    recs = R.case_inputs(name)
    fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
    # driver A: the checks
    row_a = np.dtype([("var", "<u2", 4), ("mv", "<i2", 2), ("dist", "<u4")])
    with open(fin, "wb") as f:
        f.write(np.array([w, h, cls, len(pics), seq["lad"]], np.uint32).tobytes())
        for p, r in zip(pics, recs):
            f.write(np.array([p["slice_type"], p["layer"], p["eos"]], np.uint32).tobytes())
            rows = np.zeros(n, row_a)
            rows["var"], rows["mv"], rows["dist"] = r["stats"]["variance"][:, 1:5], r["me"]["pu"]["mv"][:, 0, :2], r["me"]["pu"]["distortion"][:, 0, 0]
            f.write(rows.tobytes())
    subprocess.check_call([exe_a, fin, fout])
    raw = np.fromfile(fout, np.uint8)
    geo, checks = raw[:2 * n].reshape(n, 2), raw[2 * n:].view(R.CHECKS_DTYPE).reshape(len(pics), n)
    # driver B: everything else, fed the checks driver A derived
    row_b = np.dtype([("checks", R.CHECKS_DTYPE), ("edge", "<u2"), ("var", "<u2"), ("mv", "<i2", 2)])
    with open(fin, "wb") as f:
        f.write(np.array([w, h, cls, len(pics), seq["lad"], seq["period"], seq["head0"] % R.QUEUE_DEPTH], np.uint32).tobytes())
        for k, (p, r) in enumerate(zip(pics, recs)):
            f.write(np.array([p["poc"], p["slice_type"], p["layer"], p["hier"], p["eos"], p["scene"]], np.uint32).tobytes())
            rows = np.zeros(n, row_b)
            rows["checks"], rows["edge"], rows["var"], rows["mv"] = checks[k], r["detect"]["edge_cu"], r["stats"]["variance"][:, 0], r["me"]["pu"]["mv"][:, 0, :2]
            f.write(rows.tobytes())
    subprocess.check_call([exe_b, fin, fout])
    arrive_t = np.dtype([("tot", "<u4", 5), ("raw", "u1", 2), ("votes", "u1", n)])
    leave_t = np.dtype([("b", "u1", 4), ("seen", "<u4", 2), ("lcu", np.dtype([("counts", "<u2", 32), ("vov", "<u8"), ("f", "u1", 3)]), n)])
    raw = np.fromfile(fout, np.uint8)
    assert raw.size == len(pics) * (arrive_t.itemsize + leave_t.itemsize), (raw.size, len(pics), arrive_t.itemsize, leave_t.itemsize)
    arrive, leave = raw[:len(pics) * arrive_t.itemsize].view(arrive_t), raw[len(pics) * arrive_t.itemsize:].view(leave_t)
    assert leave["lcu"]["counts"].max() <= 255
    motion, lcu, pic = np.zeros(len(pics), R.MOTION_DTYPE), np.zeros((len(pics), n), R.IRC_LCU_DTYPE), np.zeros(len(pics), R.IRC_PIC_DTYPE)
    for k, f in enumerate(R.MOTION_FIELDS[:5]):
        motion[f] = arrive["tot"][:, k]
    motion["is_pan_raw"], motion["is_tilt_raw"] = arrive["raw"][:, 0], arrive["raw"][:, 1]
    lcu["similar_edge_count"], lcu["pm_similar_edge_count"] = leave["lcu"]["counts"][:, :, :16], leave["lcu"]["counts"][:, :, 16:]
    lcu["var_of_var_over_time"], lcu["homogeneous_over_time"], lcu["motion_votes"] = leave["lcu"]["vov"], leave["lcu"]["f"][:, :, 2], arrive["votes"]
    stationary, pm_stationary = leave["lcu"]["f"][:, :, 0].copy(), leave["lcu"]["f"][:, :, 1].copy()
    pic["is_pan"], pic["is_tilt"], pic["homogeneity_percentage"] = leave["b"][:, 0], leave["b"][:, 1], leave["b"][:, 2]
    pic["homogeneous_lcu_count"] = lcu["homogeneous_over_time"].sum(1)
    for v in range(4):
        pic["stationary_lcu_count"][:, v] = (stationary == v).sum(1)
    res = dict(case=np.array([name]), checks=checks.copy(), motion=motion, lcu=lcu, stationary_edge=stationary, pm_stationary_edge=pm_stationary, picture=pic,
               frames_to_check=leave["b"][:, 3].copy(), hom_walked=leave["seen"][:, 0].copy(), edge_places=leave["seen"][:, 1].copy(),
               complete=geo[:, 0].copy(), logo=geo[:, 1].copy())
    path = os.path.join(S.GOLDEN_DIR, "irc_%s.npz" % name)
    np.savez_compressed(path, **res)
    print("%-18s %2d pictures, %3d LCUs: flags %s, PM %s, pan raw %d / final %d, tilt raw %d, homogeneous %d -> %s (%d KiB)" % (
        name, len(pics), n, np.bincount(stationary.ravel(), minlength=4).tolist(), np.bincount(pm_stationary.ravel(), minlength=4).tolist(),
        int(motion["is_pan_raw"].sum()), int(pic["is_pan"].sum()), int(motion["is_tilt_raw"].sum()), int(lcu["homogeneous_over_time"].sum()),
        os.path.basename(path), os.path.getsize(path) // 1024))
    return name, res


def _window(flag, n, wl, hl):
    x, y = n % wl, n // wl
    return [flag[n + v * wl + c] for v in range(-1 if y > 0 else 0, (1 if y < hl - 1 else 0) + 1) for c in range(-1 if x > 0 else 0, (1 if x < wl - 1 else 0) + 1)]


def assert_not_vacuous(results):
    """every output field takes at least two values across the fixtures, and every quirk of the stage really decides something in them; `results`: name -> the
    arrays of the fixture file - the REFERENCE's records and what driver B met in the reference's queue (hom_walked, edge_places): the restatement is not
    asked.  Also run over the committed files by tests/test_irc_cpu.py."""
    for fields, key in ((R.CHECKS_FIELDS, "checks"), (R.MOTION_FIELDS, "motion"), (R.LCU_FIELDS, "lcu"), (R.PIC_FIELDS, "picture")):
        for f in fields:
            assert len(set(np.concatenate([r[key][f].ravel() for r in results.values()]).tolist())) >= 2, "one value only: " + f
    for key in ("stationary_edge", "pm_stationary_edge"):
        assert set(np.concatenate([r[key].ravel() for r in results.values()]).tolist()) == {0, 1, 2, 3}, key
    seen = dict.fromkeys(("a lone 1 cleared by pass (a)", "a lone PM 1 cleared by pass (a)", "a pair of adjacent 1s left alone", "is_pan differs from is_pan_raw",
                          "is_tilt_raw 1 while is_tilt 0", "the homogeneity divisor exceeds the entries walked", "check2 is 1 on a non-logo LCU",
                          "low_dist_logo takes both values", "an entry's own check1 == 0 withholds a count", "pass (b) marks an incomplete LCU",
                          "the threshold wraps below four pictures"), False)
    low_dist = set()
    for name, r in results.items():
        w, h, cls, seed, seq = R.CASES[name]
        wl, hl, col, row, complete, logo = R.geometry(w, h, cls)
        assert np.array_equal(r["complete"], complete) and np.array_equal(r["logo"], logo)
        recs = R.case_inputs(name)
        for k, p in enumerate(seq["pics"]):
            look_ahead, to_check = bool(seq["lad"] != 0 and not p["eos"]), int(r["frames_to_check"][k])
            checks, lcu, pic, motion = r["checks"][k], r["lcu"][k], r["picture"][k], r["motion"][k]
            seen["is_pan differs from is_pan_raw"] |= bool(pic["is_pan"] != motion["is_pan_raw"])
            seen["is_tilt_raw 1 while is_tilt 0"] |= bool(motion["is_tilt_raw"] == 1 and pic["is_tilt"] == 0)
            seen["check2 is 1 on a non-logo LCU"] |= bool((checks["check2"][~logo] == 1).any())
            low_dist |= set(checks["low_dist_logo"][logo & complete].tolist()) if look_ahead and p["slice_type"] == R.B else set()
            if not look_ahead:
                assert to_check == 1 and r["hom_walked"][k] == 0 and r["edge_places"][k] == 0
                continue
            seen["the homogeneity divisor exceeds the entries walked"] |= to_check - 1 > int(r["hom_walked"][k]) and bool((lcu["var_of_var_over_time"] != 0).any())
            # the flags before the passes, from the reference's counts and checks
            th = (to_check // 4 - 1) & 0xFFFFFFFF
            for counts, c1, key, what in ((lcu["similar_edge_count"], checks["check1"], "stationary_edge", "a lone 1 cleared by pass (a)"),
                                          (lcu["pm_similar_edge_count"], checks["pm_check1"], "pm_stationary_edge", "a lone PM 1 cleared by pass (a)")):
                before = ((c1 != 0) & (checks["check2"] != 0) & ((counts.astype(np.int64) > th).sum(1) >= 4)).astype(np.uint8)
                final = r[key][k]
                seen["the threshold wraps below four pictures"] |= to_check < 4 and bool((counts > 0).any()) and not final.any()
                for n in np.flatnonzero(before):
                    ones = sum(int(v) == 1 for v in _window(before, n, wl, hl))
                    if ones == 1:
                        assert final[n] != 1, (name, k, n)
                        seen[what] = True
                    elif key == "stationary_edge":
                        assert final[n] == 1, (name, k, n)
                        seen["a pair of adjacent 1s left alone"] = True
                seen["pass (b) marks an incomplete LCU"] |= bool((final[~complete] == 2).any())
            # place s of the walk holds picture k + s - one further when the head stands at the last place, where the walk starts at place 0
            first = k + int((seq["head0"] + k) % R.QUEUE_DEPTH == R.QUEUE_DEPTH - 1)
            for e in [first + s for s in range(32) if int(r["edge_places"][k]) >> s & 1]:
                held = (checks["check1"] != 0) & (checks["check2"] != 0) & (r["checks"][e]["check1"] == 0) & (recs[e]["detect"]["edge_cu"] != 0)
                seen["an entry's own check1 == 0 withholds a count"] |= bool(held.any())
    seen["low_dist_logo takes both values"] = low_dist == {0, 1}
    assert all(seen.values()), "decides nothing in the fixtures: " + ", ".join(k for k, v in seen.items() if not v)


if __name__ == "__main__":
    if not os.path.exists(S.REF_SO) or not os.path.isdir(REF_SRC):
        sys.exit("needs oracle/_ref/libsvtref.so (`make -C oracle ref`) and the reference's sources (SVT_REF_SOURCE, default /root/reference/Source)")
    names = sys.argv[1:] or list(R.CASES)
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _compile(tmp, "driver_a", DRIVER_A), _compile(tmp, "driver_b", DRIVER_B)
        done = dict(run_case(nm, a, b, tmp) for nm in names)
    if len(done) == len(R.CASES):
        assert_not_vacuous(done)
