#!/usr/bin/env python3
"""Generate the scene-transition fixtures from the REFERENCE itself.  SceneTransitionDetector is `static` (Codec/EbPictureDecisionProcess.c:73), so a small C
driver of our own is written into a temporary directory; it #includes that source file by path and links against oracle/_ref/libsvtref.so.  The driver reads
the case file of tests/scd_records.py:write_case (any number of cases), builds a PictureDecisionContext_t with the reference's own PictureDecisionContextCtor
and calloc'd SequenceControlSet_t / PictureParentControlSet_t objects in which only the fields the detector reads are filled from the case's records - scdMode,
the two region counts, enhancedPicturePtr->width / height, pictureHistogram, averageIntensityPerRegion, picAvgVariance - and calls the detector job after job.
After each call it records the return value, resetRunningAvg and the three running-average arrays.  No statement of the reference is kept in this file, nothing
compiled is kept.
regionCountThreshold is a local of the detector; what it decides is not: for each of the 16 x 2 (regions, mode) pairs the driver is given, for k = 1 .. regions, a
still call followed by a call in which exactly k regions change abruptly - the threshold is the smallest k that leaves resetRunningAvg set.
The region classes are locals too.  The non-vacuity list below is asserted on the reference's flags and averages where they show it, and on the classes of the
restatement (tests/scd_numpy.py) only after the restatement has been found equal to the reference's record of every job.
  -> tests/golden/scd_<name>.npz: the case name and results only (a few KiB each).  Needs the reference tree and `make -C oracle ref`.
Usage: python tests/golden/make_scd_golden.py [name ...]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scd_numpy as N  # noqa: E402
import scd_records as R  # noqa: E402
import svtlib as S  # noqa: E402

REF_SRC = os.environ.get("SVT_REF_SOURCE", "/root/reference/Source")
CALL_DTYPE = np.dtype([("flag", "u1"), ("reset", "u1"), ("pad", "u1", 2), ("avg", "<u4", (4, 4)), ("avg_cb", "<u4", (4, 4)), ("avg_cr", "<u4", (4, 4))])

DRIVER = r"""
#include "EbPictureDecisionProcess.c"
#include <stdio.h>
static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) exit(3); }
static void get(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) exit(4); }
static PictureParentControlSet_t *make_pcs(uint32_t w, uint32_t h)
{
    PictureParentControlSet_t *pcs = calloc(1, sizeof(*pcs));
    pcs->enhancedPicturePtr = calloc(1, sizeof(*pcs->enhancedPicturePtr));
    pcs->enhancedPicturePtr->width = w, pcs->enhancedPicturePtr->height = h;
    pcs->pictureHistogram = calloc(4, sizeof(void *));
    for (int a = 0; a < 4; a++) {
        pcs->pictureHistogram[a] = calloc(4, sizeof(void *));
        for (int b = 0; b < 4; b++) {
            pcs->pictureHistogram[a][b] = calloc(3, sizeof(void *));
            for (int c = 0; c < 3; c++)
                pcs->pictureHistogram[a][b][c] = calloc(256, sizeof(uint32_t));
        }
    }
    return pcs;
}
int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    int32_t hd[7];
    if (argc < 3 || !fi || !fo) return 2;
    while (fread(hd, sizeof(hd), 1, fi) == 1) {
        const uint32_t w = hd[0], h = hd[1], rw = hd[2], rh = hd[3], jobs = hd[5], n = rw * rh;
        SequenceControlSet_t *scs = calloc(1, sizeof(*scs));
        scs->scdMode = hd[4], scs->pictureAnalysisNumberOfRegionsPerWidth = rw, scs->pictureAnalysisNumberOfRegionsPerHeight = rh;
        PictureDecisionContext_t *ctx = calloc(1, sizeof(*ctx));
        if (PictureDecisionContextCtor(ctx, NULL, NULL) != EB_ErrorNone) return 5;
        if (hd[6]) {
            uint32_t st[49];
            get(fi, st, 196);
            for (uint32_t r = 0; r < n; r++)
                ctx->ahdRunningAvg[r / rh][r % rh] = st[r], ctx->ahdRunningAvgCb[r / rh][r % rh] = st[16 + r], ctx->ahdRunningAvgCr[r / rh][r % rh] = st[32 + r];
            ctx->resetRunningAvg = (st[48] & 0xFF) != 0;
        }
        PictureParentControlSet_t *win[3] = {make_pcs(w, h), make_pcs(w, h), make_pcs(w, h)};
        uint32_t *luma = malloc(n * 1024), *chroma = malloc(n * 2048);
        for (uint32_t i = 0; i < jobs; i++) {
            for (int k = 0; k < 2; k++) {             /* luma of the past, of the current picture */
                get(fi, luma, n * 1024);
                for (uint32_t r = 0; r < n; r++)
                    memcpy(win[k]->pictureHistogram[r / rh][r % rh][0], luma + r * 256, 1024);
            }
            for (int k = 0; k < 2; k++) {             /* chroma of the past, of the current picture */
                get(fi, chroma, n * 2048);
                for (uint32_t r = 0; r < n; r++)
                    for (int c = 0; c < 2; c++)
                        memcpy(win[k]->pictureHistogram[r / rh][r % rh][1 + c], chroma + (r * 2 + c) * 256, 1024);
            }
            for (int k = 0; k < 3; k++) {             /* the luma averages of the past, the current and the future picture */
                uint8_t avg[16];
                get(fi, avg, n);
                for (uint32_t r = 0; r < n; r++)
                    win[k]->averageIntensityPerRegion[r / rh][r % rh][0] = avg[r];
            }
            uint16_t var[2];
            get(fi, var, 4);
            win[0]->picAvgVariance = var[0], win[1]->picAvgVariance = var[1];
            uint8_t o[4] = {0, 0, 0, 0};
            o[0] = SceneTransitionDetector(ctx, scs, win, 0);
            o[1] = ctx->resetRunningAvg;
            put(fo, o, 4);
            uint32_t **sets[3] = {ctx->ahdRunningAvg, ctx->ahdRunningAvgCb, ctx->ahdRunningAvgCr};
            for (int k = 0; k < 3; k++)
                for (int a = 0; a < 4; a++)
                    put(fo, sets[k][a], 16);
        }
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


def _run(exe, td, write, calls):
    fin, fout = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
    with open(fin, "wb") as f:
        write(f)
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, np.uint8)
    assert raw.size == calls * CALL_DTYPE.itemsize, (raw.size, calls)
    return raw.view(CALL_DTYPE)


def compact(avg, rw, rh):
    """the reference's [4][4] array -> [16], region (wi, hi) at wi * rh + hi, 0 behind the regions"""
    out = np.zeros(avg.shape[:-2] + (16,), np.uint32)
    out[..., :rw * rh] = avg[..., :rw, :rh].reshape(avg.shape[:-2] + (rw * rh,))
    return out


def probe_thresholds(exe, td):
    """-> [4][4][2]: regionCountThreshold of (rw, rh, mode), seen through resetRunningAvg"""
    runs = [(rw, rh, mode, k) for rw in range(1, 5) for rh in range(1, 5) for mode in (1, 2) for k in range(1, rw * rh + 1)]

    def write(f):
        for rw, rh, mode, k in runs:
            s = R.Script(64 * rw, 64 * rh, rw, rh, 7)          # 64x64 regions: th 3000, a cut moves 8192
            pics = s.run(2, {2: lambda s, k=k: s.cut(list(range(k)), (0, 1, 2), 20)})
            R.write_case(f, s.w, s.h, rw, rh, mode, [R.window(pics, 0), R.window(pics, 1)])
    calls = _run(exe, td, write, 2 * len(runs)).reshape(len(runs), 2)
    th = np.zeros((4, 4, 2), np.uint8)
    for (rw, rh, mode, k), c in zip(runs, calls):
        assert c["reset"][0] == 0
        if c["reset"][1] and not th[rw - 1, rh - 1, mode - 1]:
            th[rw - 1, rh - 1, mode - 1] = k
    assert th.all()
    return th


def run_case(name, exe, td):
    w, h, rw, rh, mode, jobs, seed, events = R.CASES[name]
    pics = R.case_pictures(name)
    windows = [R.window(pics, i) for i in range(jobs)]
    calls = _run(exe, td, lambda f: R.write_case(f, w, h, rw, rh, mode, windows), jobs)
    res = dict(case=np.array([name]), scene_change=calls["flag"].copy(), reset_running_avg=calls["reset"].copy(), ahd_running_avg=compact(calls["avg"], rw, rh),
               ahd_running_avg_cb=compact(calls["avg_cb"], rw, rh), ahd_running_avg_cr=compact(calls["avg_cr"], rw, rh))
    for f in ("avg", "avg_cb", "avg_cr"):                      # nothing is written outside the regions
        kept = calls[f].copy()
        kept[:, :rw, :rh] = 0
        assert not kept.any()
    # a second run from the state the reference left in the middle: the driver's state input, and the carried state, mean what the entry's mean
    k = jobs // 2
    mid = np.zeros(1, R.STATE_DTYPE)
    for f in ("ahd_running_avg", "ahd_running_avg_cb", "ahd_running_avg_cr", "reset_running_avg"):
        mid[f][0] = res[f][k - 1]
    again = _run(exe, td, lambda f: R.write_case(f, w, h, rw, rh, mode, windows[k:], mid), jobs - k)
    assert again.tobytes() == calls[k:].tobytes(), name
    return name, res


def assert_not_vacuous(results):
    """`results`: name -> the arrays of the fixture file.  Also run over the committed files by tests/test_scd_cpu.py."""
    want = {}
    for name, ref in results.items():
        want[name] = N.restated(name)
        N.same_as_reference(want[name], ref, name)
    flags = np.concatenate([r["scene_change"] for r in results.values()])
    assert set(flags.tolist()) == {0, 1}
    classes = set(np.concatenate([w["picture"]["region_class"].ravel() for w in want.values()]).tolist())
    assert classes == {R.NONE, R.GRADUAL, R.FLASH, R.FADE, R.SCENE}, classes
    for name, ref in results.items():
        reset = [1] + ref["reset_running_avg"].tolist()        # the constructor's flag in front
        ups, downs = sum(a == 0 and b == 1 for a, b in zip(reset, reset[1:])), sum(a == 1 and b == 0 for a, b in zip(reset, reset[1:]))
        assert downs >= 1 and ups >= 1, (name, "reset goes both ways")
    c = results["cut_512x320"]
    assert c["scene_change"].tolist() == [0] * 5 + [1] + [0] * 6 and [1] + c["reset_running_avg"].tolist() == [1] + [0] * 5 + [1] + [0] * 6
    f, wf = results["flash_fade_512x320"], want["flash_fade_512x320"]["picture"]
    assert (wf["region_class"][2] == R.FLASH).all() and (wf["region_class"][6] == R.FADE).all() and f["scene_change"][2] == 0 and f["scene_change"][6] == 0
    assert f["reset_running_avg"][2] == 1 and f["reset_running_avg"][6] == 1
    assert wf["region_count_threshold"][0] == 8 and wf["scene_regions"][9] == 7 and wf["scene_regions"][12] == 8     # threshold - 1, then threshold
    assert f["scene_change"][9] == 0 and f["reset_running_avg"][9] == 0 and f["scene_change"][12] == 1 and f["reset_running_avg"][12] == 1
    ch, wc = results["chroma_only_640x384"], want["chroma_only_640x384"]
    assert ch["scene_change"].tolist() == [0, 0, 1, 0, 0, 0, 1, 0, 0, 0] and not wc["ahd"][:, :, 0].any()            # the luma clause never holds
    assert wc["ahd"][2, :, 1].all() and not wc["ahd"][2, :, 2].any() and wc["ahd"][6, :, 2].all() and not wc["ahd"][6, :, 1].any()
    g, wg = results["gradual_noise_1920x1088"], want["gradual_noise_1920x1088"]["picture"]
    assert (wg["region_class"][2:6] == R.GRADUAL).all() and not g["scene_change"][2:8].any()
    assert (g["ahd_running_avg"][6] > 2 * 46500).all()         # above th = 93000: the still picture 8 has an error above th ...
    assert (g["ahd_running_avg"][7] < g["ahd_running_avg"][6]).all() and g["reset_running_avg"][7] == 0              # ... and is no abrupt change: ahd < error
    assert g["scene_change"][9] == 1 and (wg["region_class"][12] == R.GRADUAL).all() and g["scene_change"][12] == 0  # 120000: above 93000, below 139500
    assert (g["ahd_running_avg"][12] == 30000).all()
    r3 = results["ragged_520x328_r3"]
    assert want["ragged_520x328_r3"]["picture"]["region_count_threshold"][0] == 7 and r3["scene_change"].tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    assert want["ragged_520x328_r3"]["picture"]["scene_regions"][2] == 6
    r5 = want["ragged_536x344_r3"]["picture"]
    assert r5["region_class"][2][:9].tolist() == [R.SCENE, R.SCENE, R.GRADUAL, R.GRADUAL, R.GRADUAL, R.SCENE, R.SCENE, R.SCENE, R.GRADUAL]
    assert ((results["ragged_536x344_r3"]["ahd_running_avg"][2][:9] == 0) == (r5["region_class"][2][:9] == R.SCENE)).all()   # the reference's averages show it
    assert results["one_region_64x64"]["scene_change"].tolist() == [0, 0, 1, 0]
    assert results["tiny_256x128"]["scene_change"].tolist() == [0, 0, 1, 0, 0, 0] and results["zero_th_128x64"]["scene_change"].tolist() == [0, 0, 1, 0, 0, 0]
    assert (want["zero_th_128x64"]["ahd"][2, [0, 3, 5, 6], 0] == 2).all()
    wr = want["wrap_72x78"]["picture"]["region_class"][2]
    assert (wr[:15] == R.SCENE).all() and wr[15] == R.NONE     # the last region's threshold wrapped to a large number
    lg = results["long_256"]
    assert 3 <= int(lg["scene_change"].sum()) < 128 and len(set(want["long_256"]["picture"]["region_class"].ravel().tolist())) == 5


if __name__ == "__main__":
    if not os.path.exists(S.REF_SO) or not os.path.isdir(REF_SRC):
        sys.exit("needs oracle/_ref/libsvtref.so (`make -C oracle ref`) and the reference's sources (SVT_REF_SOURCE, default /root/reference/Source)")
    names = sys.argv[1:] or list(R.CASES)
    with tempfile.TemporaryDirectory() as tmp:
        exe = _compile(tmp, "driver", DRIVER)
        thresholds = probe_thresholds(exe, tmp)
        done = dict(run_case(nm, exe, tmp) for nm in names)
    if len(done) == len(R.CASES):
        assert_not_vacuous(done)
    for name, res in done.items():
        path = os.path.join(S.GOLDEN_DIR, "scd_%s.npz" % name)
        np.savez_compressed(path, **res)
        print("%-26s %3d jobs: %3d scene changes, %3d resets -> %s (%d KiB)" % (name, len(res["scene_change"]), int(res["scene_change"].sum()),
                                                                               int(res["reset_running_avg"].sum()), os.path.basename(path), os.path.getsize(path) // 1024))
    np.savez_compressed(os.path.join(S.GOLDEN_DIR, "scd_vote_thresholds.npz"), region_count_threshold=thresholds)
    print("vote thresholds", thresholds.reshape(16, 2).T.tolist())
