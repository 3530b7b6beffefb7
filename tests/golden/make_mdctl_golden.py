#!/usr/bin/env python3
"""Generate the fixtures of the mode decision's per-LCU controls from the REFERENCE itself.  A small C driver of our own is written into a temporary directory; it
#includes reference files by path (Codec/EbModeDecisionConfigurationProcess.c for the `static` Forward85 / 84CuToModeDecision) and the project's
integration/svt_md_fill.h, and links against oracle/_ref/libsvtref.so.  For every picture of a case it lets the reference's own PictureParentControlSetCtor make
the parent control set - which derives the tile starts and the LCU edge info (Codec/EbPictureControlSet.c:743, ConfigureLcuEdgeInfo :36) and allocates every
array the rules read -, LcuParamsInit make the LCU parameters, fills the arrays from the seeded records of tests/mdctl_records.py, lets the reference's
Forward85 / 84CuToModeDecision write the leaf lists of a picture without configuration records, and then, LCU by LCU, calls the reference's ConfigureChroma and the
project's svt_md_fill_lcu - which calls the reference's DeriveContouringClass.  It checks that svt_md_fill_lcu's chroma mode is the one ConfigureChroma left in
lcuPtr and records the 191-byte records.  A second run with the sticky bits cleared records the chroma modes they changed.  No statement of the reference is kept
in this file; nothing compiled is kept.
  -> tests/golden/mdctl_<name>.npz: the case name and results only (a few KiB each).  Needs the reference tree and `make -C oracle ref`.
Usage: python tests/golden/make_mdctl_golden.py [name ...]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mdctl_records as R  # noqa: E402
import svtlib as S  # noqa: E402
from mdc_records import INVALID_AURA_STATUS, PICT_FULL84, geometry  # noqa: E402

REF_SRC = os.environ.get("SVT_REF_SOURCE", "/root/reference/Source")

DRIVER = r"""
#include "EbModeDecisionConfigurationProcess.c"
#include "EbModeDecisionProcess.h"
#include "EbCodingUnit.h"
#include "@ROOT@/integration/svt_md_fill.h"
#include <stdio.h>
static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) exit(3); }
static void get(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) exit(4); }
extern EB_ERRORTYPE LcuParamsInit(SequenceControlSet_t *sequenceControlSetPtr);
extern EB_ERRORTYPE PictureParentControlSetCtor(PictureParentControlSet_t *objectPtr, EB_PTR objectInitDataPtr);
extern void ConfigureChroma(PictureControlSet_t *pictureControlSetPtr, ModeDecisionContext_t *contextPtr, LargestCodingUnit_t *lcuPtr);
#pragma pack(push, 1)
typedef struct {
    uint8_t leaf_count, leaf_index[85], leaf_split[85], md_mode, aura;
    uint16_t variance;
    uint8_t y_mean, edge_block_num, homogeneous, high_luma, high_chroma, non_moving, complex_lcu, cmplx_status, isolated, stationary, hom_over_time;
    uint64_t energy[5];
} Row;
#pragma pack(pop)
int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    uint32_t hd[4];
    if (argc < 3 || !fi || !fo) return 2;
    get(fi, hd, sizeof(hd));
    const uint32_t w = hd[0], h = hd[1], cls = hd[2], pictures = hd[3];
    SequenceControlSet_t *scs = calloc(1, sizeof(*scs));
    scs->lumaWidth = w, scs->lumaHeight = h, scs->lcuSize = 64;
    scs->pictureWidthInLcu = (w + 63) / 64, scs->pictureHeightInLcu = (h + 63) / 64, scs->lcuTotalCount = scs->pictureWidthInLcu * scs->pictureHeightInLcu;
    scs->inputResolution = cls;
    LcuParamsInit(scs);
    const uint32_t lcus = scs->lcuTotalCount;
    EbObjectWrapper_t *scs_wrap = calloc(1, sizeof(*scs_wrap));
    scs_wrap->objectPtr = scs;
    for (uint32_t k = 0; k < pictures; k++) {
        uint32_t p[10];
        get(fi, p, sizeof(p));
        const uint32_t depth_mode = p[0], chroma_level = p[1], pan = p[2], tilt = p[3], c422 = p[4], tile_cols = p[5], tile_rows = p[6], has_mdc = p[7], grass = p[9];
        PictureControlSetInitData_t init;
        memset(&init, 0, sizeof(init));
        init.pictureWidth = w, init.pictureHeight = h, init.lcuSize = 64, init.maxDepth = 4, init.colorFormat = EB_YUV420;
        init.tileColumnCount = tile_cols, init.tileRowCount = tile_rows;
        PictureParentControlSet_t *pp = calloc(1, sizeof(*pp));
        if (PictureParentControlSetCtor(pp, &init) != EB_ErrorNone) return 6;
        memset(pp->lcuStatArray, 0, lcus * sizeof(LcuStat_t));
        pp->sequenceControlSetWrapperPtr = scs_wrap;
        pp->depthMode = (EB_PICTURE_DEPTH_MODE)depth_mode;
        pp->isPan = pan, pp->isTilt = tilt, pp->grassPercentageInPicture = grass;
        PictureControlSet_t *pcs = calloc(1, sizeof(*pcs));
        pcs->ParentPcsPtr = pp, pcs->lcuTotalCount = lcus, pcs->colorFormat = c422 ? EB_YUV422 : EB_YUV420;
        pcs->mdcLcuArray = calloc(lcus, sizeof(MdcLcuData_t));
        if (!has_mdc) {                      /* an I picture's way: the picture-level walk of its depth mode */
            if (depth_mode == 1) Forward85CuToModeDecision(scs, pcs); else if (depth_mode == 2) Forward84CuToModeDecision(scs, pcs); else return 7;
        }
        ModeDecisionContext_t *md = calloc(1, sizeof(*md));
        md->chromaLevel = chroma_level;
        for (uint32_t i = 0; i < lcus; i++) {
            Row r;
            get(fi, &r, sizeof(r));
            if (has_mdc) {
                pcs->mdcLcuArray[i].leafCount = r.leaf_count;
                for (int u = 0; u < r.leaf_count; u++)
                    pcs->mdcLcuArray[i].leafDataArray[u].leafIndex = r.leaf_index[u], pcs->mdcLcuArray[i].leafDataArray[u].splitFlag = r.leaf_split[u];
            }
            pp->lcuMdModeArray[i] = (EB_LCU_DEPTH_MODE)r.md_mode;
            pp->variance[i][0] = r.variance, pp->yMean[i][0] = r.y_mean;
            pp->edgeResultsPtr[i].edgeBlockNum = r.edge_block_num, pp->lcuHomogeneousAreaArray[i] = r.homogeneous;
            pp->lcuStatArray[i].cuStatArray[0].highLuma = r.high_luma, pp->lcuStatArray[i].cuStatArray[0].highChroma = r.high_chroma;
            pp->lcuStatArray[i].stationaryEdgeOverTimeFlag = r.stationary;
            pp->nonMovingIndexArray[i] = r.non_moving, pp->complexLcuArray[i] = (EB_LCU_COMPLEXITY_STATUS)r.complex_lcu, pp->cmplxStatusLcu[i] = r.cmplx_status;
            pp->lcuIsolatedNonHomogeneousAreaArray[i] = r.isolated, pp->isLcuHomogeneousOverTime[i] = r.hom_over_time;
            for (int q = 0; q < 5; q++)
                pp->lcuYSrcEnergyCuArray[i][q] = r.energy[q];
            LargestCodingUnit_t lcu;
            memset(&lcu, 0, sizeof(lcu));
            lcu.index = i, lcu.size = 64, lcu.lcuEdgeInfoPtr = &pp->lcuEdgeInfoArray[i], lcu.auraStatus = r.aura;
            ConfigureChroma(pcs, md, &lcu);
            SvtAmdMdLcu L;
            svt_md_fill_lcu(&L, scs, pcs, &lcu, md);
            if (L.chroma_encode_mode != lcu.chromaEncodeMode) return 5;
            put(fo, &L, sizeof(L));
        }
    }
    fclose(fo);
    return 0;
}
"""

ROW = np.dtype([("leaf_count", "u1"), ("leaf_index", "u1", 85), ("leaf_split", "u1", 85), ("md_mode", "u1"), ("aura", "u1"), ("variance", "<u2"), ("y_mean", "u1"),
                ("edge_block_num", "u1"), ("homogeneous", "u1"), ("high_luma", "u1"), ("high_chroma", "u1"), ("non_moving", "u1"), ("complex_lcu", "u1"),
                ("cmplx_status", "u1"), ("isolated", "u1"), ("stationary", "u1"), ("hom_over_time", "u1"), ("energy", "<u8", 5)])


def _compile(td, name, text):
    ref_dir = os.path.dirname(S.REF_SO)
    inc = [ref_dir] + [os.path.join(REF_SRC, d) for d in ("API", "Lib/Codec", "Lib/C_DEFAULT", "Lib/ASM_SSE2", "Lib/ASM_SSSE3", "Lib/ASM_SSE4_1", "Lib/ASM_AVX2")]
    src, exe = os.path.join(td, name + ".c"), os.path.join(td, name)
    with open(src, "w") as f:
        f.write(text.replace("@ROOT@", S.ROOT))
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-mavx2", "-msse4.1", "-w"] + ["-I" + i for i in inc] +
                          [src, "-o", exe, "-L" + ref_dir, "-lsvtref", "-Wl,-rpath," + ref_dir, "-lpthread", "-lm"])
    return exe


def rows_of(rec, jb, n, sticky=True):
    """what the driver puts into the reference's arrays for one picture.  The pool object's parent flags are the caller's sticky bits OR-ed with the picture's own
    (the header's note on cuStatArray[parent]); without the initial rate control's records no LCU is homogeneous over time"""
    rows = np.zeros(n, ROW)
    mdc = rec["mdc_lcu"]
    if mdc is not None:
        for f in ("leaf_count", "leaf_index", "leaf_split"):
            rows[f] = mdc[f]
        rows["md_mode"], rows["aura"] = mdc["lcu_md_mode"], mdc["aura_status"]
    else:
        rows["aura"] = INVALID_AURA_STATUS
    sk = rec["sticky"] if rec["sticky"] is not None and sticky else np.zeros(n, np.uint8)
    rows["variance"], rows["y_mean"] = rec["stats"]["variance"][:, 0], rec["stats"]["y_mean"][:, 0]
    rows["edge_block_num"], rows["homogeneous"] = rec["detect"]["edge_block_num"], rec["detect"]["homogeneous"]
    rows["high_luma"] = ((sk & 1) != 0) | (rec["sbo_lcu"]["high_luma"] != 0)
    rows["high_chroma"] = ((sk & 2) != 0) | (rec["sbo_lcu"]["high_chroma"] != 0)
    for f, g in (("non_moving", "non_moving_index"), ("complex_lcu", "complex_lcu"), ("cmplx_status", "cmplx_status"), ("isolated", "isolated_non_homogeneous")):
        rows[f] = rec["sbo_lcu"][g]
    if rec["stationary_edge"] is not None:
        rows["stationary"] = rec["stationary_edge"]
    if rec["irc_lcu"] is not None:
        rows["hom_over_time"], rows["energy"] = rec["irc_lcu"]["homogeneous_over_time"], rec["ac_energy"]
    return rows


def _drive(exe, td, w, h, jobs, recs, sticky):
    n = S.lcu_count(w, h)
    fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([w, h, jobs[0]["cls"], len(jobs)], np.uint32).tobytes())
        for jb, rec in zip(jobs, recs):
            f.write(np.array([jb["depth_mode"], jb["chroma_level"], jb["pan"], jb["tilt"], jb["c422"], jb["tile_cols"], jb["tile_rows"], int(rec["mdc_lcu"] is not None),
                              int(rec["irc_lcu"] is not None), int(rec["sbo_pic"]["grass_percentage"][0])], np.uint32).tobytes())
            f.write(rows_of(rec, jb, n, sticky).tobytes())
    subprocess.check_call([exe, fin, fout])
    return np.fromfile(fout, np.uint8).view(R.MD_LCU_DTYPE).reshape(len(jobs), n).copy()


def run_case(name, exe, td):
    w, h, seed, jobs = R.CASES[name]
    recs = R.case_inputs(name)
    assert len({jb["cls"] for jb in jobs}) == 1
    lcu = _drive(exe, td, w, h, jobs, recs, True)
    plain = _drive(exe, td, w, h, jobs, recs, False)
    for f in R.MD_LCU_DTYPE.names:
        if f != "chroma_encode_mode":
            assert np.array_equal(lcu[f], plain[f]), f
    res = dict(case=np.array([name]), lcu=lcu, chroma_without_sticky=plain["chroma_encode_mode"].copy())
    path = os.path.join(S.GOLDEN_DIR, "mdctl_%s.npz" % name)
    np.savez_compressed(path, **res)
    print("%-18s %2d pictures, %3d LCUs: contouring classes %s, chroma modes %s, %d changed by a sticky bit -> %s (%d KiB)" % (
        name, len(jobs), lcu.shape[1], np.bincount(lcu["contouring_class"].ravel(), minlength=4).tolist(), np.bincount(lcu["chroma_encode_mode"].ravel(), minlength=3)[1:].tolist(),
        int((lcu["chroma_encode_mode"] != plain["chroma_encode_mode"]).sum()), os.path.basename(path), os.path.getsize(path) // 1024))
    return name, res


def assert_not_vacuous(results):
    """the list of the issue, on the REFERENCE's records and the seeded inputs alone - the restatement is not asked.  `results`: name -> the arrays of the fixture
    file.  Also run over the committed files by tests/test_mdctl_cpu.py."""
    seen = dict.fromkeys(["class %d on an edge LCU" % c for c in (0, 2, 3)] + ["class %d on a non-edge LCU" % c for c in range(4)] +
                         ["an energy in [2048, 3072) on an edge LCU is class 3", "100000000 on an incomplete LCU that is homogeneous over time", "a sticky bit changes a chroma mode",
                          "the 4:2:2 override", "no_stop_split by the aura arm below class 3", "no aura arm at class 3", "2 x 2 tiles", "1 x 1 tiles",
                          "no configuration records at FULL84", "no configuration records at FULL85"] +
                         ["chroma mode %d at level %d" % (m, lv) for lv in (2, 3, 4, 5) for m in (1, 2)] + ["condition %d decides alone" % c for c in range(4)] +
                         ["%s = %d" % (f, v) for f in R.FLAG_FIELDS for v in (0, 1)], False)
    relevant = {2: (0, 1, 2), 3: (0, 1), 4: (2, 3), 5: (0,)}
    for name, r in results.items():
        w, h, seed, jobs = R.CASES[name]
        wl, hl, col, row, complete, edge = geometry(w, h)
        recs = R.case_inputs(name)
        assert np.array_equal(r["lcu"]["is_complete"], np.broadcast_to(complete, r["lcu"]["is_complete"].shape))
        for k, (jb, rec) in enumerate(zip(jobs, recs)):
            L = r["lcu"][k]
            n = len(L)
            assert not L["pad"].any()
            for f in R.FLAG_FIELDS:
                for v in (0, 1):
                    seen["%s = %d" % (f, v)] |= bool((L[f] == v).any())
                assert set(L[f].tolist()) <= {0, 1}, f
            seen["%d x %d tiles" % (jb["tile_cols"], jb["tile_rows"])] = True
            if jb["tile_cols"] == 1 and jb["tile_rows"] == 1:         # one tile: left in column 0, top in row 0, right in the last column
                assert np.array_equal(L["tile_left"], col == 0) and np.array_equal(L["tile_top"], row == 0) and np.array_equal(L["tile_right"], col == wl - 1)
            if rec["mdc_lcu"] is None:
                seen["no configuration records at FULL%d" % (84 if jb["depth_mode"] == PICT_FULL84 else 85)] = True
                assert (L["leaf_count"] > 0).all() and not L["lcu_md_mode"].any()
            if rec["irc_lcu"] is not None:
                hom, e = rec["irc_lcu"]["homogeneous_over_time"] != 0, rec["ac_energy"][:, 1:5]
                for c in range(4):
                    seen["class %d on a non-edge LCU" % c] |= bool((L["contouring_class"][~edge & hom] == c).any())
                    if c != 1:
                        seen["class %d on an edge LCU" % c] |= bool((L["contouring_class"][edge & hom] == c).any())
                assert not (L["contouring_class"][edge] == 1).any()
                third = (edge & hom)[:, None] & (e >= 2048) & (e < 3072)
                assert (L["contouring_class"][third] == 3).all()
                seen["an energy in [2048, 3072) on an edge LCU is class 3"] |= bool(third.any())
                far = (~complete & hom)[:, None] & (e == R.INCOMPLETE_ENERGY)
                assert not L["contouring_class"][far].any()
                seen["100000000 on an incomplete LCU that is homogeneous over time"] |= bool(far.any())
            else:
                assert not L["contouring_class"].any()
            seen["a sticky bit changes a chroma mode"] |= bool((L["chroma_encode_mode"] != r["chroma_without_sticky"][k]).any())
            if jb["c422"] and jb["chroma_level"] != 1:
                conds = R.conditions(rec, jb)
                assert (L["chroma_encode_mode"] == 2).all()
                seen["the 4:2:2 override"] |= bool(np.any([conds[c] for c in relevant.get(jb["chroma_level"], ())])) or jb["chroma_level"] == 0
            elif jb["chroma_level"] in relevant:
                conds = R.conditions(rec, jb)
                for m in (1, 2):
                    seen["chroma mode %d at level %d" % (m, jb["chroma_level"])] |= bool((L["chroma_encode_mode"] == m).any())
                held = np.sum([conds[c] for c in relevant[jb["chroma_level"]]], 0)
                for c in relevant[jb["chroma_level"]]:
                    alone = conds[c] & (held == 1)
                    assert (L["chroma_encode_mode"][alone] == 1).all()
                    seen["condition %d decides alone" % c] |= bool(alone.any())
            aura = rec["mdc_lcu"]["aura_status"] if rec["mdc_lcu"] is not None else np.full(n, INVALID_AURA_STATUS)
            by_aura = (aura == 1) & (rec["sbo_lcu"]["isolated_non_homogeneous"] == 0)
            if jb["cls"] < 3:
                assert (L["no_stop_split"][by_aura] == 1).all()
                seen["no_stop_split by the aura arm below class 3"] |= bool(by_aura.any())
            else:
                assert (L["no_stop_split"][by_aura] == 0).all()
                seen["no aura arm at class 3"] |= bool(by_aura.any())
    assert all(seen.values()), "decides nothing in the fixtures: " + ", ".join(k for k, v in seen.items() if not v)


if __name__ == "__main__":
    if not os.path.exists(S.REF_SO) or not os.path.isdir(REF_SRC):
        sys.exit("needs oracle/_ref/libsvtref.so (`make -C oracle ref`) and the reference's sources (SVT_REF_SOURCE, default /root/reference/Source)")
    names = sys.argv[1:] or list(R.CASES)
    with tempfile.TemporaryDirectory() as tmp:
        exe = _compile(tmp, "driver", DRIVER)
        done = dict(run_case(nm, exe, tmp) for nm in names)
    if len(done) == len(R.CASES):
        assert_not_vacuous(done)
