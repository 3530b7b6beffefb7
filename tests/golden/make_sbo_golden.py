#!/usr/bin/env python3
"""Generate the source-based-operations fixtures from the REFERENCE itself.  The functions are `static` (Codec/EbSourceBasedOperationsProcess.c, and
DeriveSimilarCollocatedFlag in Codec/EbMotionEstimationProcess.c), so two small C drivers of our own are written into a temporary directory; each #includes
one reference source file by path and links against oracle/_ref/libsvtref.so.  They fill calloc'd SequenceControlSet_t / PictureParentControlSet_t objects
(lcuParamsArray by the reference's own LcuParamsInit) from the seeded records of tests/sbo_records.py:
  driver A  DeriveSimilarCollocatedFlag of every LCU against a EbPaReferenceObject_t that carries the reference picture's 64x64 means and variances;
  driver B  builds the initial-rate-control reorder queue (the head at the last index, so that the walk wraps) and calls EbHevcUpdateBeaInfoOverTime - or
            EbHevcInitZzCostInfo for an empty window - then calls the static functions in the order of SourceBasedOperationsKernel (:1437-1571) and
            QpmGatherStatistics.  The kernel function itself cannot be called (it blocks on the encoder's queues), so its inline picture part of the QPM
            statistics (:1590-1660) is the one piece the driver spells out, on the reference's own fields and types.  CalculateAcEnergy, SetDefaultDeltaQpRange
            and StationaryEdgeOverUpdateOverTimeLcu are not part of the device entry and are not called.
All pictures of a case run on ONE picture-control-set object that is never cleared in between, as in the encoder's pool: the parent flags of GrassSkinLcu are
recorded after every picture (`parents`), which is how the sticky rule is seen.  Nothing compiled is kept.
  -> tests/golden/sbo_<name>.npz: the case name and results only (a few KiB each).  Needs the reference tree and `make -C oracle ref`.
Usage: python tests/golden/make_sbo_golden.py [name ...]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sbo_records as R  # noqa: E402
import svtlib as S  # noqa: E402

REF_SRC = os.environ.get("SVT_REF_SOURCE", "/root/reference/Source")

COMMON = r"""
#include <stdio.h>
static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) exit(3); }
static void get(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) exit(4); }
"""

DRIVER_A = r"""
#include "EbMotionEstimationProcess.c"
""" + COMMON + r"""
int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    uint32_t hd[2];
    if (argc < 3 || !fi || !fo) return 2;
    get(fi, hd, sizeof(hd));
    const uint32_t lcus = hd[0], jobs = hd[1];
    PictureParentControlSet_t *pcs = calloc(1, sizeof(*pcs));
    EbPaReferenceObject_t *ref = calloc(1, sizeof(*ref));
    EbObjectWrapper_t *wrap = calloc(1, sizeof(*wrap));
    wrap->objectPtr = ref;
    pcs->refPaPicPtrArray[REF_LIST_0] = wrap;
    pcs->yMean = calloc(lcus, sizeof(void *)), pcs->variance = calloc(lcus, sizeof(void *));
    for (uint32_t i = 0; i < lcus; i++)
        pcs->yMean[i] = calloc(MAX_ME_PU_COUNT, 1), pcs->variance[i] = calloc(MAX_ME_PU_COUNT, 2);
    pcs->similarColocatedLcuArray = calloc(lcus, sizeof(EB_BOOL)), pcs->similarColocatedLcuArrayAllLayers = calloc(lcus, sizeof(EB_BOOL));
    for (uint32_t j = 0; j < jobs; j++) {
        uint32_t p[2];
        get(fi, p, sizeof(p));
        pcs->sliceType = p[0] == 0 ? EB_I_PICTURE : p[0] == 1 ? EB_P_PICTURE : EB_B_PICTURE;
        pcs->isUsedAsReferenceFlag = p[1];
        for (uint32_t i = 0; i < lcus; i++) {
            uint16_t v[2];
            uint8_t m[2];
            get(fi, v, 4), get(fi, m, 2);
            pcs->variance[i][0] = v[0], ref->variance[i] = v[1], pcs->yMean[i][0] = m[0], ref->yMean[i] = m[1];
        }
        for (uint32_t i = 0; i < lcus; i++) {
            DeriveSimilarCollocatedFlag(pcs, i);
            uint8_t o[2] = {pcs->similarColocatedLcuArray[i] ? 1 : 0, pcs->similarColocatedLcuArrayAllLayers[i] ? 1 : 0};
            put(fo, o, 2);
        }
    }
    fclose(fo);
    return 0;
}
"""

DRIVER_B = r"""
#include "EbSourceBasedOperationsProcess.c"
#include "EbEncodeContext.h"
#include "EbInitialRateControlReorderQueue.h"
#include "EbPredictionStructure.h"
""" + COMMON + r"""
extern void EbHevcUpdateBeaInfoOverTime(EncodeContext_t *encodeContextPtr, PictureParentControlSet_t *pictureControlSetPtr);
extern void EbHevcInitZzCostInfo(PictureParentControlSet_t *pictureControlSetPtr);
extern EB_ERRORTYPE LcuParamsInit(SequenceControlSet_t *sequenceControlSetPtr);
#define WINDOW 17
int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    uint32_t hd[6];
    if (argc < 3 || !fi || !fo) return 2;
    get(fi, hd, sizeof(hd));
    const uint32_t w = hd[0], h = hd[1], rw = hd[2], rh = hd[3], jobs = hd[4], cls = hd[5];
    const uint32_t wl = (w + 63) / 64, hl = (h + 63) / 64, lcus = wl * hl;
    SequenceControlSet_t *scs = calloc(1, sizeof(*scs));
    scs->lumaWidth = w, scs->lumaHeight = h, scs->lcuSize = 64;
    scs->pictureWidthInLcu = wl, scs->pictureHeightInLcu = hl, scs->lcuTotalCount = lcus;
    scs->pictureAnalysisNumberOfRegionsPerWidth = rw, scs->pictureAnalysisNumberOfRegionsPerHeight = rh;
    scs->inputResolution = cls;
    scs->staticConfig.lookAheadDistance = WINDOW;
    LcuParamsInit(scs);
    EbObjectWrapper_t *scs_wrap = calloc(1, sizeof(*scs_wrap));
    scs_wrap->objectPtr = scs;
    PictureParentControlSet_t *pcs = calloc(1, sizeof(*pcs));
    SourceBasedOperationsContext_t *ctx = calloc(1, sizeof(*ctx));
    EbPictureBufferDesc_t enhanced = {0};
    PredictionStructure_t pred = {0};
    enhanced.width = w, enhanced.height = h;
    pred.predStructPeriod = (WINDOW - 1) / 2;
    pcs->sequenceControlSetWrapperPtr = scs_wrap, pcs->enhancedPicturePtr = &enhanced, pcs->predStructPtr = &pred;
    pcs->lcuTotalCount = lcus;
    pcs->variance = calloc(lcus, sizeof(void *)), pcs->yMean = calloc(lcus, sizeof(void *));
    pcs->cbMean = calloc(lcus, sizeof(void *)), pcs->crMean = calloc(lcus, sizeof(void *));
    pcs->varOfVar32x32BasedLcuArray = calloc(lcus, sizeof(void *));
    pcs->meResults = calloc(lcus, sizeof(void *));
    pcs->oisCu32Cu16Results = calloc(lcus, sizeof(void *)), pcs->oisCu8Results = calloc(lcus, sizeof(void *));
    for (uint32_t i = 0; i < lcus; i++) {
        pcs->variance[i] = calloc(MAX_ME_PU_COUNT, 2), pcs->yMean[i] = calloc(MAX_ME_PU_COUNT, 1);
        pcs->cbMean[i] = calloc(MAX_ME_PU_COUNT, 1), pcs->crMean[i] = calloc(MAX_ME_PU_COUNT, 1);
        pcs->varOfVar32x32BasedLcuArray[i] = calloc(4, 8);
        pcs->meResults[i] = calloc(MAX_ME_PU_COUNT, sizeof(MeCuResults_t));
        pcs->oisCu32Cu16Results[i] = calloc(1, sizeof(OisCu32Cu16Results_t)), pcs->oisCu8Results[i] = calloc(1, sizeof(OisCu8Results_t));
        for (int k = 0; k < 21; k++)
            pcs->oisCu32Cu16Results[i]->sortedOisCandidate[k] = calloc(MAX_OIS_2, sizeof(OisCandidate_t));
        for (int k = 0; k < 64; k++)
            pcs->oisCu8Results[i]->sortedOisCandidate[k] = calloc(MAX_OIS_2, sizeof(OisCandidate_t));
    }
    pcs->lcuStatArray = calloc(lcus, sizeof(LcuStat_t));           /* never cleared between the pictures of the case */
    pcs->lcuHomogeneousAreaArray = calloc(lcus, sizeof(EB_BOOL));
    pcs->edgeResultsPtr = calloc(lcus, sizeof(EdgeLcuResults_t));
    pcs->lcuCmplxContrastArray = calloc(lcus, sizeof(EB_BOOL));
    pcs->nonMovingIndexArray = calloc(lcus, 1), pcs->zzCostArray = calloc(lcus, 1);
    pcs->failingMotionLcuFlag = calloc(lcus, sizeof(EB_BOOL)), pcs->uncoveredAreaLcuFlag = calloc(lcus, sizeof(EB_BOOL));
    pcs->similarColocatedLcuArray = calloc(lcus, sizeof(EB_BOOL)), pcs->similarColocatedLcuArrayAllLayers = calloc(lcus, sizeof(EB_BOOL));
    pcs->lcuIsolatedNonHomogeneousAreaArray = calloc(lcus, sizeof(EB_BOOL));
    pcs->complexLcuArray = calloc(lcus, 1), pcs->cmplxStatusLcu = calloc(lcus, 1);
    pcs->pictureHistogram = calloc(rw, sizeof(void *));
    for (uint32_t a = 0; a < rw; a++) {
        pcs->pictureHistogram[a] = calloc(rh, sizeof(void *));
        for (uint32_t b = 0; b < rh; b++) {
            pcs->pictureHistogram[a][b] = calloc(3, sizeof(void *));
            for (int c = 0; c < 3; c++)
                pcs->pictureHistogram[a][b][c] = calloc(HISTOGRAM_NUMBER_OF_BINS, 4);
        }
    }
    /* the reorder queue: the pictures behind the current one sit at the indices after the head, which is the last one */
    EncodeContext_t *enc = calloc(1, sizeof(*enc));
    enc->initialRateControlReorderQueue = calloc(INITIAL_RATE_CONTROL_REORDER_QUEUE_MAX_DEPTH, sizeof(void *));
    enc->initialRateControlReorderQueueHeadIndex = INITIAL_RATE_CONTROL_REORDER_QUEUE_MAX_DEPTH - 1;
    PictureParentControlSet_t *ahead[WINDOW - 1];
    for (int k = 0; k < WINDOW - 1; k++) {
        InitialRateControlReorderEntry_t *e = calloc(1, sizeof(*e));
        EbObjectWrapper_t *wr = calloc(1, sizeof(*wr));
        ahead[k] = calloc(1, sizeof(PictureParentControlSet_t));
        ahead[k]->sliceType = EB_B_PICTURE;
        ahead[k]->nonMovingIndexArray = calloc(lcus, 1), ahead[k]->zzCostArray = calloc(lcus, 1);
        wr->objectPtr = ahead[k], e->parentPcsWrapperPtr = wr;
        enc->initialRateControlReorderQueue[k] = e;
    }
    for (uint32_t j = 0; j < jobs; j++) {
        uint32_t p[8];
        get(fi, p, sizeof(p));
        const uint32_t zz_count = p[3], qpm = p[6];
        pcs->sliceType = p[0] == 0 ? EB_I_PICTURE : p[0] == 1 ? EB_P_PICTURE : EB_B_PICTURE;
        pcs->temporalLayerIndex = p[1], pcs->isUsedAsReferenceFlag = p[2], pcs->skipOis8x8 = p[4], pcs->cu8x8Mode = p[5];
        pcs->framesInSw = zz_count;
        for (uint32_t i = 0; i < lcus; i++) {
            uint8_t flags[4];
            uint32_t me[85], ois[85];
            get(fi, pcs->variance[i], 85 * 2), get(fi, pcs->yMean[i], 85), get(fi, pcs->cbMean[i], 21), get(fi, pcs->crMean[i], 21);
            get(fi, pcs->varOfVar32x32BasedLcuArray[i], 32), get(fi, flags, 4), get(fi, me, sizeof(me)), get(fi, ois, sizeof(ois));
            pcs->similarColocatedLcuArray[i] = flags[0], pcs->similarColocatedLcuArrayAllLayers[i] = flags[1];
            pcs->lcuHomogeneousAreaArray[i] = flags[2], pcs->edgeResultsPtr[i].edgeBlockNum = flags[3];
            for (int k = 0; k < 85; k++)
                pcs->meResults[i][k].distortionDirection[0].distortion = me[k];
            for (int k = 1; k < 21; k++)
                pcs->oisCu32Cu16Results[i]->sortedOisCandidate[k][0].oisResults = ois[k];
            for (int k = 0; k < 64; k++)
                pcs->oisCu8Results[i]->sortedOisCandidate[k][0].oisResults = ois[21 + k];
        }
        for (uint32_t a = 0; a < rw; a++)
            for (uint32_t b = 0; b < rh; b++)
                get(fi, pcs->pictureHistogram[a][b][0], 1024);
        for (uint32_t k = 0; k < zz_count; k++) {
            PictureParentControlSet_t *q = k ? ahead[k - 1] : pcs;
            get(fi, q->zzCostArray, lcus), get(fi, q->nonMovingIndexArray, lcus);
        }
        /* ---- the initial rate control's step ---- */
        if (zz_count)
            EbHevcUpdateBeaInfoOverTime(enc, pcs);
        else
            EbHevcInitZzCostInfo(pcs);
        /* ---- SourceBasedOperationsKernel, :1423-1571 ---- */
        pcs->darkBackGroundlightForeGround = EB_FALSE;
        ctx->pictureNumGrassLcu = 0, ctx->countOfMovingLcus = 0, ctx->countOfNonMovingLcus = 0, ctx->yNonMovingMean = 0, ctx->yMovingMean = 0;
        ctx->toBeIntraCodedProbability = 0, ctx->depth1BlockNum = 0;
        for (uint32_t i = 0; i < lcus; i++) {
            LcuParams_t *lp = &scs->lcuParamsArray[i];
            pcs->lcuCmplxContrastArray[i] = 0;
            EB_BOOL isCompleteLcu = lp->isCompleteLcu;
            ctx->yMeanPtr = pcs->yMean[i], ctx->crMeanPtr = pcs->crMean[i], ctx->cbMeanPtr = pcs->cbMean[i];
            GrassSkinLcu(ctx, scs, pcs, i);
            if (isCompleteLcu)
                SpatialHighContrastClassifier(ctx, pcs, i);
            LumaContrastDetectorLcu(ctx, scs, pcs, i);
            pcs->failingMotionLcuFlag[i] = EB_FALSE;
            if (pcs->sliceType != EB_I_PICTURE && isCompleteLcu)
                FailingMotionLcu(scs, pcs, i);
            pcs->uncoveredAreaLcuFlag[i] = EB_FALSE;
            if (pcs->temporalLayerIndex == 0 && pcs->sliceType != EB_I_PICTURE)
                if (isCompleteLcu && (!pcs->similarColocatedLcuArray[i]))
                    DetectUncoveredLcu(scs, pcs, i);
            if (isCompleteLcu) {
                TemporalHighContrastClassifier(ctx, pcs, i);
                if (ctx->highContrastNum && ctx->highDist)
                    PopulateFromCurrentLcuToNeighborLcus(pcs, (ctx->highContrastNum && ctx->highDist), pcs->lcuCmplxContrastArray, i, lp->originX, lp->originY);
            }
        }
        LumaContrastDetectorPicture(ctx, pcs);
        DeriveHighDarkAreaDensityFlag(scs, pcs);
        DetermineIsolatedNonHomogeneousRegionInPicture(scs, pcs);
        DetermineMorePotentialAuraAreas(scs, pcs);
        DerivePictureActivityStatistics(scs, pcs);
        DeriveBlockinessPresentFlag(scs, pcs);
        GrassSkinPicture(ctx, pcs);
        ComplexityClassifier32x32(scs, pcs);
        uint32_t q[9][4];
        memset(q, 0, sizeof(q));
        if (qpm) { /* :1590-1660, on the reference's fields */
            for (int d = 0; d < 4; ++d) {
                pcs->intraComplexityMin[d] = ~0u, pcs->intraComplexityMax[d] = 0, pcs->intraComplexityAccum[d] = 0, pcs->intraComplexityAvg[d] = 0;
                pcs->interComplexityMin[d] = ~0u, pcs->interComplexityMax[d] = 0, pcs->interComplexityAccum[d] = 0, pcs->interComplexityAvg[d] = 0;
                pcs->processedleafCount[d] = 0;
            }
            for (uint32_t i = 0; i < lcus; i++)
                QpmGatherStatistics(scs, pcs, i);
            EB_U32 totDepths = pcs->skipOis8x8 ? 3 : 4;
            for (EB_U8 d = 0; d < totDepths; ++d) {
                pcs->intraComplexityAvg[d] = pcs->intraComplexityAccum[d] / pcs->processedleafCount[d];
                pcs->interComplexityAvg[d] = pcs->interComplexityAccum[d] / pcs->processedleafCount[d];
                EB_S32 intraMinDistance = ABS(((EB_S32)pcs->intraComplexityMin[d] - (EB_S32)pcs->intraComplexityAvg[d]));
                EB_S32 intraMaxDistance = ((EB_S32)pcs->intraComplexityMax[d] - (EB_S32)pcs->intraComplexityAvg[d]);
                if (intraMinDistance < intraMaxDistance)
                    pcs->intraComplexityMax[d] = pcs->intraComplexityAvg[d] + intraMinDistance;
                else
                    pcs->intraComplexityMin[d] = pcs->intraComplexityAvg[d] - intraMaxDistance;
                EB_S32 interMinDistance = 0, interMaxDistance = 0;
                if (pcs->sliceType != EB_I_PICTURE) {
                    interMinDistance = ABS(((EB_S32)pcs->interComplexityMin[d] - (EB_S32)pcs->interComplexityAvg[d]));
                    interMaxDistance = ((EB_S32)pcs->interComplexityMax[d] - (EB_S32)pcs->interComplexityAvg[d]);
                }
                if (interMinDistance < interMaxDistance)
                    pcs->interComplexityMax[d] = pcs->interComplexityAvg[d] + interMinDistance;
                else
                    pcs->interComplexityMin[d] = pcs->interComplexityAvg[d] - interMaxDistance;
            }
            for (int d = 0; d < 4; d++) {
                q[0][d] = pcs->intraComplexityMin[d], q[1][d] = pcs->intraComplexityMax[d], q[2][d] = pcs->intraComplexityAccum[d], q[3][d] = pcs->intraComplexityAvg[d];
                q[4][d] = pcs->interComplexityMin[d], q[5][d] = pcs->interComplexityMax[d], q[6][d] = pcs->interComplexityAccum[d], q[7][d] = pcs->interComplexityAvg[d];
                q[8][d] = pcs->processedleafCount[d];
            }
        }
        /* ---- results ---- */
        for (uint32_t i = 0; i < lcus; i++) {
            LcuStat_t *ls = &pcs->lcuStatArray[i];
            uint16_t mask[4] = {0, 0, 0, 0};
            uint8_t parents[4][5], children_ok = 1;
            for (int k = 0; k < 16; k++) {
                const CuStat_t *cu = &ls->cuStatArray[RASTER_SCAN_TO_MD_SCAN[RASTER_SCAN_CU_INDEX_16x16_0 + k]];
                if (!scs->lcuParamsArray[i].rasterScanCuValidity[RASTER_SCAN_CU_INDEX_16x16_0 + k])
                    continue; /* units outside the picture are never written */
                mask[0] |= (uint16_t)((cu->grassArea ? 1 : 0) << k), mask[1] |= (uint16_t)((cu->skinArea ? 1 : 0) << k);
                mask[2] |= (uint16_t)((cu->highLuma ? 1 : 0) << k), mask[3] |= (uint16_t)((cu->highChroma ? 1 : 0) << k);
                for (int c = 1; c < 5; c++)
                    children_ok &= cu[c].grassArea == cu->grassArea && cu[c].skinArea == cu->skinArea && cu[c].highLuma == cu->highLuma && cu[c].highChroma == cu->highChroma;
            }
            for (int c = 0; c < 5; c++) {
                const CuStat_t *cu = &ls->cuStatArray[RASTER_SCAN_TO_MD_SCAN[c]];
                parents[0][c] = cu->grassArea ? 1 : 0, parents[1][c] = cu->skinArea ? 1 : 0, parents[2][c] = cu->highLuma ? 1 : 0, parents[3][c] = cu->highChroma ? 1 : 0;
            }
            uint8_t b[10] = {pcs->zzCostArray[i], pcs->nonMovingIndexArray[i], pcs->similarColocatedLcuArray[i] ? 1 : 0,
                             pcs->similarColocatedLcuArrayAllLayers[i] ? 1 : 0, pcs->failingMotionLcuFlag[i] ? 1 : 0, pcs->uncoveredAreaLcuFlag[i] ? 1 : 0,
                             pcs->lcuCmplxContrastArray[i] ? 1 : 0, pcs->lcuIsolatedNonHomogeneousAreaArray[i] ? 1 : 0, pcs->cmplxStatusLcu[i], pcs->complexLcuArray[i]};
            put(fo, mask, 8), put(fo, b, 10), put(fo, parents, 20), put(fo, &children_ok, 1);
            uint8_t geo[2] = {scs->lcuParamsArray[i].isCompleteLcu, scs->lcuParamsArray[i].isEdgeLcu};
            put(fo, geo, 2);
        }
        uint32_t complete = 0;
        for (uint32_t i = 0; i < lcus; i++)
            complete += scs->lcuParamsArray[i].isCompleteLcu;
        uint32_t head[2] = {complete, pcs->zzCostAverage};
        uint16_t nm = pcs->nonMovingIndexAverage;
        uint8_t pb[8] = {pcs->lowMotionContentFlag ? 1 : 0, pcs->darkBackGroundlightForeGround ? 1 : 0, pcs->intraCodedBlockProbability, pcs->grassPercentageInPicture,
                         pcs->percentageOfEdgeinLightBackground, pcs->highDarkAreaDensityFlag ? 1 : 0, pcs->highDarkLowLightAreaDensityFlag ? 1 : 0,
                         pcs->blackAreaPercentage};
        put(fo, head, 8), put(fo, &nm, 2), put(fo, pb, 8), put(fo, q, sizeof(q));
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


LCU_OUT = np.dtype([("mask", "<u2", 4), ("b", "u1", 10), ("parents", "u1", (4, 5)), ("children_ok", "u1"), ("complete", "u1"), ("edge_lcu", "u1")])


def run_case(name, exe_a, exe_b, td):
    w, h, rw, rh, seed, jobs = R.CASES[name]
    n = S.lcu_count(w, h)
    recs = R.case_inputs(name)
    fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
    # driver A: the similarity flags
    with open(fin, "wb") as f:
        f.write(np.array([n, len(jobs)], np.uint32).tobytes())
        for jb, r in zip(jobs, recs):
            f.write(np.array([jb["slice_type"], jb["ref"]], np.uint32).tobytes())
            rows = np.zeros(n, np.dtype([("v", "<u2", 2), ("m", "u1", 2)]))
            rows["v"][:, 0], rows["v"][:, 1] = r["stats"]["variance"][:, 0], r["ref_stats"]["variance"][:, 0]
            rows["m"][:, 0], rows["m"][:, 1] = r["stats"]["y_mean"][:, 0], r["ref_stats"]["y_mean"][:, 0]
            f.write(rows.tobytes())
    subprocess.check_call([exe_a, fin, fout])
    similar = np.fromfile(fout, np.uint8).reshape(len(jobs), n, 2)
    # driver B: everything else, fed the flags driver A derived
    assert all(jb["cls"] == jobs[0]["cls"] for jb in jobs)
    with open(fin, "wb") as f:
        f.write(np.array([w, h, rw, rh, len(jobs), jobs[0]["cls"]], np.uint32).tobytes())
        for j, (jb, r) in enumerate(zip(jobs, recs)):
            f.write(np.array([jb["slice_type"], jb["layer"], jb["ref"], jb["zz_count"], jb["skip"], jb["cu8"], jb["qpm"], 0], np.uint32).tobytes())
            for i in range(n):
                f.write(r["stats"]["variance"][i].tobytes()), f.write(r["stats"]["y_mean"][i].tobytes())
                f.write(r["chroma"]["cb_mean"][i].tobytes()), f.write(r["chroma"]["cr_mean"][i].tobytes())
                f.write(r["detect"]["var_of_var_32x32"][i].tobytes())
                f.write(bytes([int(similar[j, i, 0]), int(similar[j, i, 1]), int(r["detect"]["homogeneous"][i]), int(r["detect"]["edge_block_num"][i])]))
                f.write(np.ascontiguousarray(r["me"]["pu"]["distortion"][i, :, 0]).tobytes()), f.write(np.ascontiguousarray(r["ois"]["candidate"][i, :, 0]).tobytes())
            f.write(r["histogram"].tobytes())
            for k in range(jb["zz_count"]):
                f.write(np.ascontiguousarray(r["zz"][k]["zz_cost"]).tobytes()), f.write(np.ascontiguousarray(r["zz"][k]["non_moving_index"]).tobytes())
    subprocess.check_call([exe_b, fin, fout])
    pic_t = np.dtype([("lcu", LCU_OUT, n), ("complete_lcu_count", "<u4"), ("zz_cost_average", "<u4"), ("non_moving_index_average", "<u2"), ("b", "u1", 8),
                      ("qpm", "<u4", (9, 4))])
    raw = np.fromfile(fout, np.uint8)
    assert raw.size == len(jobs) * pic_t.itemsize, (raw.size, len(jobs), pic_t.itemsize)
    out = raw.view(pic_t)
    assert out["lcu"]["children_ok"].all(), "an 8x8 child whose flags differ from its 16x16 unit"
    assert np.array_equal(out["lcu"]["b"][:, :, 2:4], similar)
    lcu, pic = np.zeros((len(jobs), n), R.SBO_LCU_DTYPE), np.zeros(len(jobs), R.SBO_PIC_DTYPE)
    for k, f in enumerate(("grass", "skin", "high_luma", "high_chroma")):
        lcu[f] = out["lcu"]["mask"][:, :, k]
    for k, f in enumerate(R.LCU_FIELDS[4:]):
        lcu[f] = out["lcu"]["b"][:, :, k]
    for f in ("complete_lcu_count", "zz_cost_average", "non_moving_index_average"):
        pic[f] = out[f]
    for k, f in enumerate(R.PIC_FIELDS[3:11]):
        pic[f] = out["b"][:, k]
    for k, f in enumerate(R.QPM_FIELDS):
        pic[f] = out["qpm"][:, k]
    res = dict(case=np.array([name]), lcu=lcu, picture=pic, parents=out["lcu"]["parents"].copy(), complete=out["lcu"]["complete"][0].copy(),
               edge_lcu=out["lcu"]["edge_lcu"][0].copy())
    path = os.path.join(S.GOLDEN_DIR, "sbo_%s.npz" % name)
    np.savez_compressed(path, **res)
    print("%-18s %d pictures, %3d LCUs: contrast %d, isolated %d, failing %d, uncovered %d, noise %d, complex %s -> %s (%d KiB)" % (
        name, len(jobs), n, int(lcu["cmplx_contrast"].sum()), int(lcu["isolated_non_homogeneous"].sum()), int(lcu["failing_motion"].sum()),
        int(lcu["uncovered_area"].sum()), int((lcu["cmplx_status"] == 4).sum()), np.bincount(lcu["complex_lcu"].ravel(), minlength=3).tolist(),
        os.path.basename(path), os.path.getsize(path) // 1024))
    return name, res


def assert_not_vacuous(results):
    """every output field takes at least two values across the fixtures, and every order or quirk rule really decides an LCU in them; `results`: name -> the
    arrays of the fixture file.  Also run over the committed files by tests/test_sbo_cpu.py."""
    import sbo_numpy as N
    for fields, key in ((R.LCU_FIELDS, "lcu"), (R.PIC_FIELDS, "picture")):
        for f in fields:
            assert len(set(np.concatenate([r[key][f].ravel() for r in results.values()]).tolist())) >= 2, "one value only: " + f
    assert set(np.concatenate([r["lcu"]["complex_lcu"].ravel() for r in results.values()]).tolist()) == {0, 1, 2}
    seen = dict.fromkeys(("sticky parent", "contrast mark kept in front of its trigger", "contrast mark wiped behind its trigger", "trigger next to a partial column",
                          "trigger next to a partial row", "homogeneous side neighbours that do not count", "exactly two flat neighbours",
                          "incomplete LCUs left out of the averages", "ME below OIS on a tested LCU"), False)
    for name, r in results.items():
        w, h, rw, rh, seed, jobs = R.CASES[name]
        wl, hl, col, row, complete = R.geometry(w, h)
        assert np.array_equal(r["complete"], complete)
        for j, (jb, rec) in enumerate(zip(jobs, R.case_inputs(name))):
            lcu = r["lcu"][j]
            near = lambda a, b: 0 <= b < lcu.size and abs(a % wl - b % wl) <= 1  # noqa: E731
            # item 3: a parent flag that is set although no unit of this picture sets it
            own = np.zeros_like(r["parents"][j])
            for kind, f in enumerate(("grass", "skin", "high_luma", "high_chroma")):
                own[:, kind, 0] = lcu[f] != 0
                for q in range(4):
                    own[:, kind, 1 + q] = (lcu[f] & sum(1 << k for k in range(16) if N.PARENT_32[k] == 1 + q)) != 0
            assert not (r["parents"][j] < own).any()
            seen["sticky parent"] |= bool((r["parents"][j] > own).any())
            # item 4: a neighbour in front of a trigger keeps the mark; one behind it, with no trigger behind itself, has lost it
            trig = _triggers(w, h, rec, jb)
            for m in np.flatnonzero(trig):
                for n in (m - 1, m - wl, m - wl - 1, m - wl + 1):
                    seen["contrast mark kept in front of its trigger"] |= bool(near(m, n) and lcu["cmplx_contrast"][n])
                for n in (m + 1, m + wl, m + wl - 1, m + wl + 1):
                    if near(m, n) and not any(trig[t] for t in (n + 1, n + wl, n + wl - 1, n + wl + 1) if near(n, t)):
                        seen["contrast mark wiped behind its trigger"] |= not lcu["cmplx_contrast"][n]
                seen["trigger next to a partial column"] |= bool(col[m] == wl - 2 and w % 64)
                seen["trigger next to a partial row"] |= bool(row[m] == hl - 2 and h % 64)
            # item 8: the four side neighbours are not counted; two flat neighbours are enough
            v64, det = rec["stats"]["variance"][:, 0], rec["detect"]
            for n in np.flatnonzero((col > 0) & (col < wl - 1) & (row > 0) & (row < hl - 1)):
                ring = [(n + v * wl + c, v, c) for v in (-1, 0, 1) for c in (-1, 0, 1) if v or c]
                flat = sum(int(v64[a] <= 50 and (complete[a] or (v <= 0 and c <= 0 and (v, c) != (-1, 1)) or (v, c) in ((-1, 0),))) for a, v, c in ring)
                if flat > 1 and (det["var_of_var_32x32"][n] > 4096).any():
                    every = sum(int(det["homogeneous"][a]) for a, v, c in ring)
                    seen["homogeneous side neighbours that do not count"] |= bool(every >= 2 and not lcu["isolated_non_homogeneous"][n])
                    seen["exactly two flat neighbours"] |= bool(flat == 2 and lcu["isolated_non_homogeneous"][n])
            # item 10: the averages are those of the complete LCUs
            if jb["zz_count"] and not complete.all():
                seen["incomplete LCUs left out of the averages"] |= int(lcu["non_moving_index"].astype(int).sum()) // lcu.size != int(r["picture"]["non_moving_index_average"][j])
            # item 6: ME below OIS on an LCU that is tested
            if jb["slice_type"] != 0:
                me0, o = rec["me"]["pu"]["distortion"][:, 0, 0].astype(np.int64), (rec["ois"]["candidate"][:, 1:5, 0] & 0xFFFFF).astype(np.int64).sum(1)
                seen["ME below OIS on a tested LCU"] |= bool((complete & (lcu["similar_colocated"] == 0) & ((me0 < o) | (me0 >= 1 << 31))).any())
    assert all(seen.values()), "decides nothing in the fixtures: " + ", ".join(k for k, v in seen.items() if not v)


def _triggers(w, h, rec, jb):
    """highContrastNum && highDist of the complete LCUs, from the inputs"""
    wl, hl, col, row, complete = R.geometry(w, h)
    st, ch = rec["stats"], rec["chroma"]
    y, cb, cr, var = (a[:, 5:21].astype(int) for a in (st["y_mean"], ch["cb_mean"], ch["cr_mean"], st["variance"]))
    spatial = ((var > 10) & (var < 300) & (y > 70) & (y < 145) & (abs(cb - 140) < 10) & (abs(cr - 115) < 15)).any(1)
    nsad = rec["me"]["pu"]["distortion"][:, 1:5, 0] >> 10
    temporal = (nsad >= (10 if jb["layer"] == 0 else 5)).any(1) & (jb["slice_type"] == 2)
    return complete & spatial & temporal


if __name__ == "__main__":
    if not os.path.exists(S.REF_SO) or not os.path.isdir(REF_SRC):
        sys.exit("needs oracle/_ref/libsvtref.so (`make -C oracle ref`) and the reference's sources (SVT_REF_SOURCE, default /root/reference/Source)")
    names = sys.argv[1:] or list(R.CASES)
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _compile(tmp, "driver_a", DRIVER_A), _compile(tmp, "driver_b", DRIVER_B)
        done = dict(run_case(nm, a, b, tmp) for nm in names)
    if len(done) == len(R.CASES):
        assert_not_vacuous(done)
