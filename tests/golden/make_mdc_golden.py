#!/usr/bin/env python3
"""Generate the mode-decision-configuration fixtures from the REFERENCE itself.  The functions of Codec/EbModeDecisionConfigurationProcess.c are `static`, so
a small C driver of our own is written into a temporary directory; it #includes that source file by path and links against oracle/_ref/libsvtref.so
(EarlyModeDecisionLcu, LcuParamsInit and the rate-estimation initialisers are exported symbols).  It fills calloc'd sequence, parent and child control sets,
lcuPtrArray, mdcLcuArray and two reference objects from the seeded records of tests/mdc_records.py (lcuParamsArray by the reference's own LcuParamsInit, the
rate tables by MdRateEstimationContextInit) and calls the static functions in the order of ModeDecisionConfigurationKernel (:1936-2080).  The kernel function
itself cannot be called (it blocks on the encoder's queues), so the statements of its loop between the input queue and the output queue (:1936-2080) are cut
out of the reference's file when the driver is built and #included into a block that declares the three pointers under the reference's names: no statement of
the reference is kept in this file.  What the reference leaves stale between pictures - leaf lists of BDP LCUs, pred64 of LCUs that run no early
decision, intervalCost beyond numberOfSegments - is cleared in front of every picture, and the budgeting fields of a picture that is not PICT_LCU_SWITCH are
recorded as 0.  Nothing compiled is kept.
  -> tests/golden/mdc_<name>.npz: the case name and results only (leaf lists cut to leaf_count), with the SAD lambda and splitFlagBits[0] / [3] the
     reference's tables gave each picture.  Needs the reference tree and `make -C oracle ref`.
Usage: python tests/golden/make_mdc_golden.py [name ...]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mdc_records as R  # noqa: E402
import svtlib as S  # noqa: E402

REF_SRC = os.environ.get("SVT_REF_SOURCE", "/root/reference/Source")

DRIVER = r"""
#include "EbModeDecisionConfigurationProcess.c"
#include "EbEncodeContext.h"
#include "EbCabacContextModel.h"
#include "EbMdRateEstimation.h"
#include <stdio.h>
static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) exit(3); }
static void get(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) exit(4); }
extern EB_ERRORTYPE LcuParamsInit(SequenceControlSet_t *sequenceControlSetPtr);
/* the passes of DeriveOptimalBudgetPerLcu are a local of it: the driver is compiled with -finstrument-functions and counts the entries of SetLcuBudget */
/* ... and records lcuMinScore / lcuMaxScore as DeriveLcuScore left them at the entry of PerformOutlierRemoval */
static unsigned long budget_calls;
static ModeDecisionConfigurationContext_t *hook_ctx;
static uint32_t raw_lo, raw_hi;
void __cyg_profile_func_enter(void *fn, void *site) __attribute__((no_instrument_function));
void __cyg_profile_func_exit(void *fn, void *site) __attribute__((no_instrument_function));
void __cyg_profile_func_enter(void *fn, void *site) 
{
    (void)site;
    if (fn == (void *)SetLcuBudget) budget_calls++;
    if (fn == (void *)PerformOutlierRemoval) raw_lo = hook_ctx->lcuMinScore, raw_hi = hook_ctx->lcuMaxScore;
}
void __cyg_profile_func_exit(void *fn, void *site) { (void)fn, (void)site; }
typedef struct { int16_t mv[4]; uint32_t dist; uint8_t dir[3], total; } InPu;
typedef struct { InPu pu[85]; uint16_t var64; uint8_t mean64, edge_block_num, sharp_edge, similar_all, similar, failing, nmi, complex_lcu, stationary, pad; } InLcu;
typedef struct { uint8_t leaf_count, leaf[85][2], md_mode, aura, pred64, avc, pad0; uint32_t score; uint8_t cost, pad[3]; } OutLcu;
typedef struct { int32_t v[12]; uint32_t budget, predicted, lo, hi; int8_t th[7]; uint8_t interval[7], iterations, pad; uint32_t lambda, split[2], raw_lo, raw_hi; } OutPic;
int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    uint32_t hd[3];
    if (argc < 3 || !fi || !fo) return 2;
    get(fi, hd, sizeof(hd));
    const uint32_t w = hd[0], h = hd[1], jobs = hd[2];
    const uint32_t wl = (w + 63) / 64, hl = (h + 63) / 64, lcus = wl * hl;
    SequenceControlSet_t *scs = calloc(1, sizeof(*scs));
    scs->lumaWidth = w, scs->lumaHeight = h, scs->lcuSize = 64, scs->maxLcuDepth = 4;
    scs->pictureWidthInLcu = wl, scs->pictureHeightInLcu = hl, scs->lcuTotalCount = lcus;
    LcuParamsInit(scs);
    EncodeContext_t *enc = calloc(1, sizeof(*enc));
    enc->cabacContextModelArray = calloc(TOTAL_NUMBER_OF_CABAC_CONTEXT_MODEL_BUFFERS, sizeof(ContextModelEncContext_t));
    EncodeCabacContextModelInit(enc->cabacContextModelArray);
    enc->mdRateEstimationArray = calloc(TOTAL_NUMBER_OF_MD_RATE_ESTIMATION_CASE_BUFFERS, sizeof(MdRateEstimationContext_t));
    MdRateEstimationContextInit(enc->mdRateEstimationArray, enc->cabacContextModelArray);
    scs->encodeContextPtr = enc;
    EbObjectWrapper_t *scs_wrap = calloc(1, sizeof(*scs_wrap));
    scs_wrap->objectPtr = scs;
    PictureParentControlSet_t *pp = calloc(1, sizeof(*pp));
    PictureControlSet_t *pcs = calloc(1, sizeof(*pcs));
    pcs->ParentPcsPtr = pp, pcs->sequenceControlSetWrapperPtr = scs_wrap, pp->sequenceControlSetWrapperPtr = scs_wrap;
    pcs->lcuTotalCount = lcus, pp->lcuTotalCount = lcus;
    pcs->lcuPtrArray = calloc(lcus, sizeof(void *));
    pcs->mdcLcuArray = calloc(lcus, sizeof(MdcLcuData_t));
    pp->meResults = calloc(lcus, sizeof(void *));
    pp->oisCu32Cu16Results = calloc(lcus, sizeof(void *)), pp->oisCu8Results = calloc(lcus, sizeof(void *));
    pp->variance = calloc(lcus, sizeof(void *)), pp->yMean = calloc(lcus, sizeof(void *));
    for (uint32_t i = 0; i < lcus; i++) {
        LargestCodingUnit_t *l = calloc(1, sizeof(*l));
        l->pictureControlSetPtr = pcs, l->index = i, l->originX = (i % wl) * 64, l->originY = (i / wl) * 64;
        pcs->lcuPtrArray[i] = l;
        pp->meResults[i] = calloc(MAX_ME_PU_COUNT, sizeof(MeCuResults_t));
        pp->variance[i] = calloc(MAX_ME_PU_COUNT, 2), pp->yMean[i] = calloc(MAX_ME_PU_COUNT, 1);
        pp->oisCu32Cu16Results[i] = calloc(1, sizeof(OisCu32Cu16Results_t)), pp->oisCu8Results[i] = calloc(1, sizeof(OisCu8Results_t));
        for (int k = 0; k < 21; k++)
            pp->oisCu32Cu16Results[i]->sortedOisCandidate[k] = calloc(MAX_OIS_2, sizeof(OisCandidate_t));
        for (int k = 0; k < 64; k++)
            pp->oisCu8Results[i]->sortedOisCandidate[k] = calloc(MAX_OIS_2, sizeof(OisCandidate_t));
    }
    pp->edgeResultsPtr = calloc(lcus, sizeof(EdgeLcuResults_t));
    pp->lcuStatArray = calloc(lcus, sizeof(LcuStat_t));
    pp->sharpEdgeLcuFlag = calloc(lcus, 1);
    pp->similarColocatedLcuArray = calloc(lcus, sizeof(EB_BOOL)), pp->similarColocatedLcuArrayAllLayers = calloc(lcus, sizeof(EB_BOOL));
    pp->failingMotionLcuFlag = calloc(lcus, sizeof(EB_BOOL));
    pp->nonMovingIndexArray = calloc(lcus, 1);
    pp->complexLcuArray = calloc(lcus, sizeof(*pp->complexLcuArray));
    pp->lcuMdModeArray = calloc(lcus, sizeof(*pp->lcuMdModeArray));
    EbReferenceObject_t *ref[2] = {calloc(1, sizeof(EbReferenceObject_t)), calloc(1, sizeof(EbReferenceObject_t))};
    for (int k = 0; k < 2; k++) {
        EbObjectWrapper_t *wr = calloc(1, sizeof(*wr));
        wr->objectPtr = ref[k];
        pcs->refPicPtrArray[k] = wr;
    }
    ModeDecisionConfigurationContext_t *ctx = calloc(1, sizeof(*ctx));
    ctx->mdRateEstimationPtr = calloc(1, sizeof(MdRateEstimationContext_t));
    ctx->lcuScoreArray = calloc(lcus, sizeof(*ctx->lcuScoreArray)), ctx->lcuCostArray = calloc(lcus, sizeof(*ctx->lcuCostArray));
    hook_ctx = ctx;
    InLcu *in = calloc(lcus, sizeof(InLcu));
    for (uint32_t j = 0; j < jobs; j++) {
        int32_t p[40];
        get(fi, p, sizeof(p));
        get(fi, in, lcus * sizeof(InLcu));
        const int slice = p[0], layer = p[1], hier = p[2], is_ref = p[3], depth_mode = p[4];
        pcs->sliceType = pp->sliceType = slice == 1 ? EB_P_PICTURE : EB_B_PICTURE;
        pcs->temporalLayerIndex = pp->temporalLayerIndex = layer, pp->hierarchicalLevels = hier, pp->isUsedAsReferenceFlag = is_ref;
        pp->depthMode = depth_mode, pp->encMode = p[5], scs->inputResolution = p[6], pcs->pictureQp = pp->pictureQp = p[7];
        pp->isPan = p[8], pp->isTilt = p[9], pp->noiseDetectionTh = p[10], pp->picHomogenousOverTimeLcuPercentage = p[11];
        scs->staticConfig.frameRate = (p[12] ? 60u : 30u) << 16, pp->cu8x8Mode = p[13], pp->averageIntensity[0] = p[14];
        for (int k = 0; k < 2; k++)
            ref[k]->averageIntensity = p[15 + k], ref[k]->intraCodedArea = p[17 + k], ref[k]->tmpLayerIdx = p[19 + k], ref[k]->penalizeSkipflag = p[21 + k];
        pp->picNoiseClass = p[23], pp->logoPicFlag = p[24], pp->highDarkLowLightAreaDensityFlag = p[25], pp->blackAreaPercentage = p[26];
        pp->grassPercentageInPicture = p[27], pp->nonMovingIndexAverage = p[28], pp->zzCostAverage = p[29], pp->intraCodedBlockProbability = p[30];
        pp->interComplexityMinPre = (uint32_t)p[31], pp->interComplexityMaxPre = (uint32_t)p[32];
        const int have_stationary = p[33];
        pp->idrFlag = EB_FALSE;
        for (uint32_t i = 0; i < lcus; i++) {
            const InLcu *s = &in[i];
            for (int k = 0; k < 85; k++) {
                MeCuResults_t *m = &pp->meResults[i][k];
                m->xMvL0 = s->pu[k].mv[0], m->yMvL0 = s->pu[k].mv[1], m->xMvL1 = s->pu[k].mv[2], m->yMvL1 = s->pu[k].mv[3];
                m->distortionDirection[0].distortion = s->pu[k].dist;
                for (int c = 0; c < 3; c++)
                    m->distortionDirection[c].direction = s->pu[k].dir[c];
                m->totalMeCandidateIndex = s->pu[k].total;
            }
            pp->variance[i][0] = s->var64, pp->yMean[i][0] = s->mean64;
            pp->edgeResultsPtr[i].edgeBlockNum = s->edge_block_num, pp->sharpEdgeLcuFlag[i] = s->sharp_edge;
            pp->similarColocatedLcuArrayAllLayers[i] = s->similar_all, pp->similarColocatedLcuArray[i] = s->similar;
            pp->failingMotionLcuFlag[i] = s->failing, pp->nonMovingIndexArray[i] = s->nmi, pp->complexLcuArray[i] = s->complex_lcu;
            pp->lcuStatArray[i].stationaryEdgeOverTimeFlag = have_stationary ? s->stationary : 0;
            pp->lcuMdModeArray[i] = 0;
            pcs->lcuPtrArray[i]->pred64 = 0;
        }
        memset(pcs->mdcLcuArray, 0, lcus * sizeof(MdcLcuData_t));
        memset(ctx->intervalCost, 0, sizeof(ctx->intervalCost));
        /* ---- the body of ModeDecisionConfigurationKernel's loop (:1936-2080), spliced out of the reference's file when the driver is built ---- */
        if (pp->depthMode >= PICT_OPEN_LOOP_DEPTH_MODE)
            return 5; /* no picture of this reference (Codec/EbPictureDecisionProcess.c:383-405) */
        budget_calls = 0, raw_lo = raw_hi = 0;
        {
            ModeDecisionConfigurationContext_t *contextPtr = ctx;
            PictureControlSet_t *pictureControlSetPtr = pcs;
            SequenceControlSet_t *sequenceControlSetPtr = scs;
            EB_U32 pictureWidthInLcu, pictureHeightInLcu;
#include "kernel_body.inc"
            if (pictureWidthInLcu != wl || pictureHeightInLcu != hl) return 6;
        }
        /* ---- results ---- */
        const int adp = pp->depthMode == PICT_LCU_SWITCH_DEPTH_MODE;
        for (uint32_t i = 0; i < lcus; i++) {
            OutLcu o;
            memset(&o, 0, sizeof(o));
            const MdcLcuData_t *m = &pcs->mdcLcuArray[i];
            o.leaf_count = m->leafCount;
            for (int k = 0; k < 85; k++)
                o.leaf[k][0] = m->leafDataArray[k].leafIndex, o.leaf[k][1] = m->leafDataArray[k].splitFlag ? 1 : 0;
            o.md_mode = adp ? pp->lcuMdModeArray[i] : 0, o.aura = pcs->lcuPtrArray[i]->auraStatus, o.pred64 = pcs->lcuPtrArray[i]->pred64;
            o.avc = adp && IsAvcPartitioningMode(scs, pcs, pcs->lcuPtrArray[i]) ? 1 : 0;
            o.score = adp ? ctx->lcuScoreArray[i] : 0, o.cost = adp ? ctx->lcuCostArray[i] : 0;
            put(fo, &o, sizeof(o));
        }
        OutPic q;
        memset(&q, 0, sizeof(q));
        q.v[0] = pcs->sceneCaracteristicId, q.v[1] = pcs->adjustMinQPFlag ? 1 : 0, q.v[2] = pcs->highIntraSlection, q.v[3] = pcs->sliceCbQpOffset;
        q.v[4] = pcs->sliceCrQpOffset, q.v[5] = pcs->tcOffset, q.v[6] = pcs->betaOffset, q.v[7] = pp->averageQp;
        if (adp) {
            q.v[8] = ctx->adpDepthSensitivePictureClass, q.v[9] = ctx->adpRefinementMode, q.v[10] = ctx->numberOfSegments;
            q.v[11] = (pcs->bdpPresentFlag ? 1 : 0) | (pcs->mdPresentFlag ? 2 : 0);
            q.budget = ctx->budget, q.predicted = ctx->predictedCost, q.lo = ctx->lcuMinScore, q.hi = ctx->lcuMaxScore;
            memcpy(q.th, ctx->scoreTh, 7), memcpy(q.interval, ctx->intervalCost, 7);
            q.iterations = (uint8_t)(budget_calls / lcus), q.raw_lo = raw_lo, q.raw_hi = raw_hi;
            q.lambda = (uint32_t)ctx->lambda, q.split[0] = ctx->mdRateEstimationPtr->splitFlagBits[0], q.split[1] = ctx->mdRateEstimationPtr->splitFlagBits[3];
        }
        put(fo, &q, sizeof(q));
    }
    fclose(fo);
    return 0;
}
"""

IN_PU = np.dtype([("mv", "<i2", 4), ("dist", "<u4"), ("dir", "u1", 3), ("total", "u1")])
IN_LCU = np.dtype([("pu", IN_PU, 85), ("var64", "<u2"), ("mean64", "u1"), ("edge_block_num", "u1"), ("sharp_edge", "u1"), ("similar_all", "u1"), ("similar", "u1"),
                   ("failing", "u1"), ("nmi", "u1"), ("complex_lcu", "u1"), ("stationary", "u1"), ("pad", "u1")])
OUT_LCU = np.dtype([("leaf_count", "u1"), ("leaf", "u1", (85, 2)), ("md_mode", "u1"), ("aura", "u1"), ("pred64", "u1"), ("avc", "u1"), ("pad0", "u1"), ("score", "<u4"), ("cost", "u1"),
                    ("pad", "u1", 3)])
OUT_PIC = np.dtype([("v", "<i4", 12), ("budget", "<u4"), ("predicted", "<u4"), ("lo", "<u4"), ("hi", "<u4"), ("th", "i1", 7), ("interval", "u1", 7), ("iterations", "u1"), ("pad", "u1"),
                    ("lambda", "<u4"), ("split", "<u4", 2), ("raw_lo", "<u4"), ("raw_hi", "<u4")])
assert IN_PU.itemsize == 16 and IN_LCU.itemsize == 85 * 16 + 12 and OUT_LCU.itemsize == 184 and OUT_PIC.itemsize == 100


KERNEL_FILE = "Lib/Codec/EbModeDecisionConfigurationProcess.c"


def splice_kernel_body(td):
    """the statements of ModeDecisionConfigurationKernel between taking the picture from the input queue and posting the results (:1936-2080) -> kernel_body.inc
    in the temporary directory.  Found by its first and last statement, so that a reference whose lines have moved is noticed"""
    with open(os.path.join(REF_SRC, KERNEL_FILE)) as f:
        lines = f.readlines()
    func = next(i for i, ln in enumerate(lines) if ln.startswith("void* ModeDecisionConfigurationKernel"))
    first = next(i for i in range(func, len(lines)) if "SignalDerivationModeDecisionConfigKernelOq(" in lines[i])
    last = next(i for i in range(first, len(lines)) if "Post the results to the MD processes" in lines[i])
    assert (first + 1, last + 1) == (1936, 2082), (first + 1, last + 1)
    with open(os.path.join(td, "kernel_body.inc"), "w") as f:
        f.writelines(lines[first:last])


def _compile(td, name, text):
    ref_dir = os.path.dirname(S.REF_SO)
    inc = [td, ref_dir] + [os.path.join(REF_SRC, d) for d in ("API", "Lib/Codec", "Lib/C_DEFAULT", "Lib/ASM_SSE2", "Lib/ASM_SSSE3", "Lib/ASM_SSE4_1", "Lib/ASM_AVX2")]
    src, exe = os.path.join(td, name + ".c"), os.path.join(td, name)
    with open(src, "w") as f:
        f.write(text)
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-fno-inline", "-finstrument-functions", "-mavx2", "-msse4.1", "-w"] + ["-I" + i for i in inc] +
                          [src, "-o", exe, "-L" + ref_dir, "-lsvtref", "-Wl,-rpath," + ref_dir, "-lpthread", "-lm"])
    return exe


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same results give the same file"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def pack_inputs(rec, n):
    rows = np.zeros(n, IN_LCU)
    pu = rec["me"]["pu"]
    rows["pu"]["mv"], rows["pu"]["dist"], rows["pu"]["dir"], rows["pu"]["total"] = pu["mv"], pu["distortion"][:, :, 0], pu["direction"], pu["total"]
    rows["var64"], rows["mean64"] = rec["stats"]["variance"][:, 0], rec["stats"]["y_mean"][:, 0]
    rows["edge_block_num"], rows["sharp_edge"] = rec["detect"]["edge_block_num"], rec["detect"]["sharp_edge"]
    sl = rec["sbo_lcu"]
    rows["similar_all"], rows["similar"], rows["failing"] = sl["similar_colocated_all_layers"], sl["similar_colocated"], sl["failing_motion"]
    rows["nmi"], rows["complex_lcu"] = sl["non_moving_index"], sl["complex_lcu"]
    if rec["stationary_edge"] is not None:
        rows["stationary"] = rec["stationary_edge"]
    return rows


def run_case(name, exe, td):
    w, h, seed, jobs = R.CASES[name]
    n = S.lcu_count(w, h)
    recs = R.case_inputs(name)
    fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, len(jobs)], np.uint32).tobytes())
        for jb, r in zip(jobs, recs):
            sp = r["sbo_pic"][0]
            p = [jb[k] for k in R.SCALARS] + [int(r["noise_pic"][0]["pic_noise_class"]), int(r["pic_detect"][0]["logo_pic"]), int(sp["high_dark_low_light_area_density"]),
                                              int(sp["black_area_percentage"]), int(sp["grass_percentage"]), int(sp["non_moving_index_average"]), int(sp["zz_cost_average"]),
                                              int(sp["intra_coded_block_probability"]), int(sp["inter_complexity_min"][0]), int(sp["inter_complexity_max"][0]),
                                              int(r["stationary_edge"] is not None)]
            f.write(np.array(p + [0] * (40 - len(p)), np.int32).tobytes())
            f.write(pack_inputs(r, n).tobytes())
    subprocess.check_call([exe, fin, fout])
    pic_t = np.dtype([("lcu", OUT_LCU, n), ("pic", OUT_PIC)])
    raw = np.fromfile(fout, np.uint8)
    assert raw.size == len(jobs) * pic_t.itemsize, (raw.size, len(jobs), pic_t.itemsize)
    out = raw.view(pic_t)
    lcu, pic = np.zeros((len(jobs), n), R.MDC_LCU_DTYPE), np.zeros(len(jobs), R.MDC_PIC_DTYPE)
    o = out["lcu"]
    lcu["leaf_count"], lcu["lcu_md_mode"], lcu["aura_status"], lcu["pred64"], lcu["avc_partitioning"] = o["leaf_count"], o["md_mode"], o["aura"], o["pred64"], o["avc"]
    lcu["lcu_score"], lcu["lcu_cost"] = o["score"], o["cost"]
    used = np.arange(85)[None, None, :] < o["leaf_count"][:, :, None]          # the lists cut to leaf_count: what lies behind is stale in the reference
    lcu["leaf_index"], lcu["leaf_split"] = np.where(used, o["leaf"][:, :, :, 0], 0), np.where(used, o["leaf"][:, :, :, 1], 0)
    q = out["pic"]
    for k, f in enumerate(R.PIC_FIELDS[:11]):   # scene_characteristic_id .. number_of_segments
        pic[f] = q["v"][:, k]
    pic["bdp_present"], pic["md_present"] = q["v"][:, 11] & 1, q["v"][:, 11] >> 1
    pic["budget"], pic["predicted_cost"], pic["lcu_min_score"], pic["lcu_max_score"] = q["budget"], q["predicted"], q["lo"], q["hi"]
    pic["score_th"], pic["interval_cost"], pic["iterations"] = q["th"], q["interval"], q["iterations"]
    res = dict(case=np.array([name]), lcu=lcu, picture=pic, lambda_=q["lambda"].copy(), split_bits=q["split"].copy(),
               raw_min_max=np.stack([q["raw_lo"], q["raw_hi"]], 1))
    path = os.path.join(S.GOLDEN_DIR, "mdc_%s.npz" % name)
    save_npz(path, res)
    modes = np.bincount(lcu["lcu_md_mode"].ravel(), minlength=11)[1:].tolist()
    print("%-16s %2d pictures, %3d LCUs: modes %s, aura %s, avc %d, leaf counts %d -> %s (%d KiB)" % (
        name, len(jobs), n, modes, np.bincount(lcu["aura_status"].ravel(), minlength=2)[:2].tolist(), int(lcu["avc_partitioning"].sum()),
        len(set(lcu["leaf_count"].ravel().tolist())), os.path.basename(path), os.path.getsize(path) // 1024))
    return name, res


def assert_not_vacuous(results):
    """the conditions that make the fixtures worth having, from the reference's records (`results`: name -> the arrays of the fixture file).  One of them leans
    on the restatement: WHICH clause of IsAvcPartitioningMode decides an LCU is not observable from outside the function, so it is derived by
    mdc_numpy.is_avc_partitioning from the seeded inputs and the reference's own aura status and picture signals, and held against the reference's flag.
    Also run over the committed files by tests/test_mdc_cpu.py."""
    import mdc_numpy as N
    modes, aura, clauses, refinement, classes, passes, shooting, moved, counts, partial_counts, pred64 = (set() for _ in range(11))
    for name, r in results.items():
        w, h, seed, jobs = R.CASES[name]
        wl, hl, col, row, complete, edge = R.geometry(w, h)
        for j, (jb, rec) in enumerate(zip(jobs, R.case_inputs(name))):
            lcu, pic = r["lcu"][j], r["picture"][j]
            aura |= set(lcu["aura_status"].tolist())
            counts |= set(lcu["leaf_count"].tolist())
            partial_counts |= set(lcu["leaf_count"][~complete].tolist())
            if jb["depth_mode"] != R.PICT_LCU_SWITCH:
                assert not lcu["lcu_md_mode"].any() and pic["budget"] == 0
                continue
            modes |= set(lcu["lcu_md_mode"].tolist())
            refinement.add(int(pic["adp_refinement_mode"])), classes.add(int(pic["adp_depth_sensitive_picture_class"])), passes.add(int(pic["iterations"]))
            pred64 |= set(lcu["pred64"][np.isin(lcu["lcu_md_mode"], (R.LCU_OPEN_LOOP, R.LCU_LIGHT_OPEN_LOOP, R.LCU_PRED_OPEN_LOOP, R.LCU_PRED_OPEN_LOOP_1_NFL))].tolist())
            for i in range(lcu.size):                            # the deciding clause of IsAvcPartitioningMode, on the reference's aura status and picture signals
                c = N.is_avc_partitioning(rec, jb, int(pic["scene_characteristic_id"]), int(pic["high_intra_selection"]), lcu["aura_status"], complete, i)
                assert (c != 0) == bool(lcu["avc_partitioning"][i]), (name, j, i)
                clauses.add(c)
            first = 100 // int(pic["number_of_segments"])       # scoreTh[0] as DeriveDefaultSegments left it: it falls while under-shooting and rises while over-shooting
            shooting.add("under" if pic["score_th"][0] < first else "over" if pic["score_th"][0] > first else "none")
            raw_lo, raw_hi = (int(v) for v in r["raw_min_max"][j])   # lcuMinScore / lcuMaxScore at the entry of PerformOutlierRemoval
            moved |= ({"min"} if pic["lcu_min_score"] != raw_lo else set()) | ({"max"} if pic["lcu_max_score"] != raw_hi else set())
    assert len(modes - {0}) >= 8, sorted(modes)
    assert {0, 1} <= aura and {1, 2, 3, 4, 5} <= clauses and refinement == {0, 1, 2} and classes == {0, 1, 2}, (aura, clauses, refinement, classes)
    assert 1 in passes and max(passes) > 10 and {"under", "over"} <= shooting and moved == {"min", "max"}, (sorted(passes), shooting, moved)
    assert len(counts) >= 12 and len(partial_counts - {0}) >= 3 and pred64 == {0, 1}, (sorted(counts), sorted(partial_counts), pred64)


if __name__ == "__main__":
    if not os.path.exists(S.REF_SO) or not os.path.isdir(REF_SRC):
        sys.exit("needs oracle/_ref/libsvtref.so (`make -C oracle ref`) and the reference's sources (SVT_REF_SOURCE, default /root/reference/Source)")
    names = sys.argv[1:] or list(R.CASES)
    with tempfile.TemporaryDirectory() as tmp:
        splice_kernel_body(tmp)
        exe = _compile(tmp, "driver", DRIVER)
        done = dict(run_case(nm, exe, tmp) for nm in names)
    if len(done) == len(R.CASES):
        assert_not_vacuous(done)
