#!/usr/bin/env python3
"""Generate the chroma-statistics / picture-detector fixtures from the REFERENCE itself.  The functions are `static` (GatheringPictureStatistics,
Codec/EbPictureAnalysisProcess.c:3995, and everything it calls), so a small C driver of our own is written into a temporary directory; it #includes the
reference's EbPictureAnalysisProcess.c by path, links against oracle/_ref/libsvtref.so and calls GatheringPictureStatistics whole on seeded planes, with
lcuParamsArray filled by the reference's own LcuParamsInit / DeriveInputResolution.  Nothing compiled is kept.
  -> tests/golden/padetect_<name>.npz: seeds and results (no planes).  Needs the reference tree and `make -C oracle ref`.
Usage: python tests/golden/make_pa_detect_golden.py [name ...]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pa_detect_pictures as P  # noqa: E402
import svtlib as S  # noqa: E402

REF_SRC = os.environ.get("SVT_REF_SOURCE", "/root/reference/Source")

#          kind, width, height, seed, regions_w, regions_h, [(picture number, want_edge16), ...]
CASES = {
    # 6.5 x 3.75 LCUs: a partial right column and bottom row (zeroed chroma means, all-ones var-of-var); interior LCUs for edgeBlockNum / sharpEdge
    "motion_416x240": ("motion", 416, 240, 7, 4, 4, [(4, 1), (5, 0)]),
    # 200 / 3 and 136 / 3 leave remainders, the region origins are odd before the >> 1
    "noise_200x136": ("noise", 200, 136, 11, 3, 3, [(0, 1)]),
    # 11 x 10 LCUs: two bright LCUs whose 9x9 neighbourhoods overlap, LCUs behind the later one (the order rule), one step-edge LCU
    "islands_704x640": ("islands", 704, 640, 5, 4, 4, [(0, 1)]),
    # the next resolution class: the other potentialLogoLcu map
    "objects_1280x720": ("objects", 1280, 720, 3, 4, 4, [(4, 1)]),
}

DRIVER = r"""
#include "EbPictureAnalysisProcess.c"
#include <stdio.h>
static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) exit(3); }
static void get(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) exit(4); }
int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    uint32_t hd[5];
    if (argc < 3 || !fi || !fo) return 2;
    get(fi, hd, sizeof(hd));
    const uint32_t w = hd[0], h = hd[1], rw = hd[2], rh = hd[3], n = hd[4];
    const uint32_t wl = (w + 63) / 64, hl = (h + 63) / 64, lcus = wl * hl, pw = w + 64, ph = h + 64;
    SequenceControlSet_t *scs = calloc(1, sizeof(*scs));
    scs->lumaWidth = w, scs->lumaHeight = h, scs->lcuSize = 64;
    scs->pictureWidthInLcu = wl, scs->pictureHeightInLcu = hl, scs->lcuTotalCount = lcus;
    scs->pictureAnalysisNumberOfRegionsPerWidth = rw, scs->pictureAnalysisNumberOfRegionsPerHeight = rh;
    scs->scdMode = SCD_MODE_1;
    DeriveInputResolution(scs, w * h);
    LcuParamsInit(scs);
    PictureParentControlSet_t *pcs = calloc(1, sizeof(*pcs));
    PictureAnalysisContext_t *ctx = calloc(1, sizeof(*ctx));
    pcs->lcuTotalCount = lcus;
    pcs->variance = calloc(lcus, sizeof(void *)), pcs->yMean = calloc(lcus, sizeof(void *));
    pcs->cbMean = calloc(lcus, sizeof(void *)), pcs->crMean = calloc(lcus, sizeof(void *));
    pcs->varOfVar32x32BasedLcuArray = calloc(lcus, sizeof(void *));
    ctx->grad = calloc(lcus, sizeof(void *));
    for (uint32_t i = 0; i < lcus; i++) {
        pcs->variance[i] = calloc(MAX_ME_PU_COUNT, 2), pcs->yMean[i] = calloc(MAX_ME_PU_COUNT, 1);
        pcs->cbMean[i] = calloc(MAX_ME_PU_COUNT, 1), pcs->crMean[i] = calloc(MAX_ME_PU_COUNT, 1);
        pcs->varOfVar32x32BasedLcuArray[i] = calloc(4, 8);
        ctx->grad[i] = calloc(CU_MAX_COUNT, 2);
    }
    pcs->lcuHomogeneousAreaArray = calloc(lcus, sizeof(EB_BOOL));
    pcs->lcuStatArray = calloc(lcus, sizeof(LcuStat_t));
    pcs->edgeResultsPtr = calloc(lcus, sizeof(EdgeLcuResults_t));
    pcs->sharpEdgeLcuFlag = calloc(lcus, 1);
    pcs->pictureHistogram = calloc(rw, sizeof(void *));
    for (uint32_t a = 0; a < rw; a++) {
        pcs->pictureHistogram[a] = calloc(rh, sizeof(void *));
        for (uint32_t b = 0; b < rh; b++) {
            pcs->pictureHistogram[a][b] = calloc(3, sizeof(void *));
            for (int c = 0; c < 3; c++)
                pcs->pictureHistogram[a][b][c] = calloc(HISTOGRAM_NUMBER_OF_BINS, 4);
        }
    }
    uint8_t *luma = malloc(pw * ph), *six = malloc((w / 4) * (h / 4)), *cb = malloc((w / 2) * (h / 2)), *cr = malloc((w / 2) * (h / 2));
    EbPictureBufferDesc_t in = {0}, pad = {0}, dec = {0};
    in.bufferY = luma, in.bufferCb = cb, in.bufferCr = cr, in.strideY = pw, in.strideCb = in.strideCr = w / 2, in.width = w, in.height = h;
    pad = in;
    dec.bufferY = six, dec.strideY = w / 4, dec.width = w / 4, dec.height = h / 4;
    for (uint32_t p = 0; p < n; p++) {
        uint64_t number;
        get(fi, &number, 8);
        get(fi, luma, pw * ph), get(fi, six, (w / 4) * (h / 4)), get(fi, cb, (w / 2) * (h / 2)), get(fi, cr, (w / 2) * (h / 2));
        pcs->pictureNumber = number;
        GatheringPictureStatistics(scs, pcs, ctx, &in, &pad, &dec, lcus);
        for (uint32_t i = 0; i < lcus; i++) {
            put(fo, pcs->variance[i], 85 * 2), put(fo, pcs->yMean[i], 85), put(fo, pcs->cbMean[i], 21), put(fo, pcs->crMean[i], 21);
            put(fo, pcs->varOfVar32x32BasedLcuArray[i], 32);
            uint16_t edge = 0;
            for (int k = 0; k < 16; k++)
                edge |= (uint16_t)((pcs->lcuStatArray[i].cuStatArray[5 + k].edgeCu ? 1 : 0) << k);
            uint8_t b[6] = {pcs->lcuHomogeneousAreaArray[i] ? 1 : 0, pcs->edgeResultsPtr[i].edgeBlockNum, pcs->edgeResultsPtr[i].isolatedHighIntensityLcu,
                            pcs->sharpEdgeLcuFlag[i], scs->lcuParamsArray[i].potentialLogoLcu, scs->lcuParamsArray[i].isCompleteLcu};
            put(fo, &edge, 2), put(fo, b, 6);
        }
        for (uint32_t a = 0; a < rw; a++)
            for (uint32_t b = 0; b < rh; b++) {
                for (int c = 0; c < 3; c++)
                    put(fo, pcs->pictureHistogram[a][b][c], 1024);
                uint8_t avg[3] = {(uint8_t)pcs->averageIntensityPerRegion[a][b][0], (uint8_t)pcs->averageIntensityPerRegion[a][b][1],
                                  (uint8_t)pcs->averageIntensityPerRegion[a][b][2]};
                put(fo, avg, 3);
            }
        uint16_t pav = pcs->picAvgVariance;
        uint8_t pic[7] = {pcs->veryLowVarPicFlag, pcs->logoPicFlag, pcs->lcuBlockPercentage, pcs->averageIntensity[0], pcs->averageIntensity[1],
                          pcs->averageIntensity[2], scs->inputResolution};
        put(fo, &pav, 2), put(fo, pic, 7);
        /* the two chroma sums are locals of GatheringPictureStatistics: the histogram leaf once more (it starts from the bins' initial value) */
        uint64_t sums[2] = {0, 0};
        SubSampleChromaGeneratePixelIntensityHistogramBins(scs, pcs, &in, &sums[0], &sums[1]);
        put(fo, sums, 16);
    }
    fclose(fo);
    return 0;
}
"""


def run_reference(w, h, rw, rh, pictures):
    """pictures: [(number, luma, cb, cr)] -> dict of arrays, picture first"""
    ref_dir = os.path.dirname(S.REF_SO)
    rs = REF_SRC
    inc = [ref_dir] + [os.path.join(rs, d) for d in ("API", "Lib/Codec", "Lib/C_DEFAULT", "Lib/ASM_SSE2", "Lib/ASM_SSSE3", "Lib/ASM_SSE4_1", "Lib/ASM_AVX2")]
    nl, n = S.lcu_count(w, h), len(pictures)
    with tempfile.TemporaryDirectory() as td:
        src, exe, fin, fout = (os.path.join(td, x) for x in ("driver.c", "driver", "in.bin", "out.bin"))
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-mavx2", "-msse4.1", "-w"] + ["-I" + i for i in inc] +
                              [src, "-o", exe, "-L" + ref_dir, "-lsvtref", "-Wl,-rpath," + ref_dir, "-lpthread", "-lm"])
        with open(fin, "wb") as f:
            f.write(np.array([w, h, rw, rh, n], np.uint32).tobytes())
            for number, luma, cb, cr in pictures:
                f.write(np.uint64(number).tobytes())
                f.write(P.padded(luma).tobytes()), f.write(np.ascontiguousarray(luma[::4, ::4]).tobytes())      # the 1/16 picture: point decimation
                f.write(cb.tobytes()), f.write(cr.tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = np.fromfile(fout, np.uint8)
    lcu_t = np.dtype([("variance", "<u2", 85), ("y_mean", "u1", 85), ("cb_mean", "u1", 21), ("cr_mean", "u1", 21), ("var_of_var_32x32", "<u8", 4),
                      ("edge_cu", "<u2"), ("homogeneous", "u1"), ("edge_block_num", "u1"), ("isolated_high_intensity", "u1"), ("sharp_edge", "u1"),
                      ("potential_logo", "u1"), ("complete", "u1")])
    reg_t = np.dtype([("hist", "<u4", (3, 256)), ("avg", "u1", 3)])
    pic_t = np.dtype([("lcu", lcu_t, nl), ("region", reg_t, (rw, rh)), ("pic_avg_variance", "<u2"), ("very_low_var_pic", "u1"), ("logo_pic", "u1"),
                      ("lcu_block_percentage", "u1"), ("average_intensity", "u1", 3), ("resolution_class", "u1"), ("sum_chroma", "<u8", 2)])
    assert raw.size == n * pic_t.itemsize, (raw.size, n, pic_t.itemsize)
    return raw.view(pic_t)


def run_case(name):
    kind, w, h, seed, rw, rh, pics = CASES[name]
    frames = [(t,) + (P.gen_luma(kind, w, h, t, seed),) + P.gen_chroma(kind, w, h, t, seed) for t, _ in pics]
    r = run_reference(w, h, rw, rh, frames)
    lcu = r["lcu"]
    want = np.array([e for _, e in pics], np.uint8)
    # the reference computes the 16x16 edge map only on every 4th picture and clears it otherwise (:3535): the fixture's want_edge16 is that rule
    assert all(int(e) == int((t & 3) == 0) for t, e in pics)
    assert int(r["resolution_class"][0]) == P.resolution_class(w, h)
    out = dict(clip=np.array([kind, str(w), str(h), str(seed), str(rw), str(rh)]), picture_number=np.array([t for t, _ in pics], np.uint64), want_edge16=want,
               resolution_class=r["resolution_class"].copy(),
               variance=lcu["variance"].copy(), y_mean=lcu["y_mean"].copy(), cb_mean=lcu["cb_mean"].copy(), cr_mean=lcu["cr_mean"].copy(),
               histogram=np.ascontiguousarray(r["region"]["hist"][:, :, :, 1:3]), luma_histogram=np.ascontiguousarray(r["region"]["hist"][:, :, :, 0]),
               region_average=np.ascontiguousarray(r["region"]["avg"][:, :, :, 1:3]), luma_region_average=np.ascontiguousarray(r["region"]["avg"][:, :, :, 0]),
               sum_chroma=r["sum_chroma"].copy(), average_intensity=r["average_intensity"].copy(),
               var_of_var_32x32=lcu["var_of_var_32x32"].copy(), edge_cu=lcu["edge_cu"].copy(), homogeneous=lcu["homogeneous"].copy(),
               edge_block_num=lcu["edge_block_num"].copy(), isolated_high_intensity=lcu["isolated_high_intensity"].copy(), sharp_edge=lcu["sharp_edge"].copy(),
               potential_logo=lcu["potential_logo"].copy(), pic_avg_variance=r["pic_avg_variance"].copy(), very_low_var_pic=r["very_low_var_pic"].copy(),
               logo_pic=r["logo_pic"].copy(), lcu_block_percentage=r["lcu_block_percentage"].copy())
    path = os.path.join(S.GOLDEN_DIR, "padetect_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("%-20s %d pictures, %d LCUs: edge_block %d, sharp %d, isolated %d, edge_cu words %d, pic_avg_variance %s -> %s (%d KiB)" % (
        name, len(pics), lcu.shape[1], int(lcu["edge_block_num"].sum()), int(lcu["sharp_edge"].sum()), int(lcu["isolated_high_intensity"].sum()),
        int((lcu["edge_cu"] != 0).sum()), r["pic_avg_variance"].tolist(), os.path.basename(path), os.path.getsize(path) // 1024))
    return name, out


def assert_not_vacuous(results):
    """every rule the fixtures are there for really decides something in them"""
    for field in ("isolated_high_intensity", "sharp_edge", "edge_block_num", "edge_cu"):
        assert any(o[field].any() for o in results.values()), "no LCU with " + field
    if "islands_704x640" in results:
        o = results["islands_704x640"]
        wl = 11
        iso = o["isolated_high_intensity"][0]
        inside = [n for bx, by in P.ISLANDS_BRIGHT for n in range(iso.size) if abs(n % wl - bx) <= 4 and abs(n // wl - by) <= 4]
        assert any(iso[n] == 0 for n in inside), "the order rule of isolatedHighIntensityLcu decides nothing in islands"
        assert any(iso[n] == 1 for n in inside)
    if "motion_416x240" in results:
        o = results["motion_416x240"]
        assert not o["edge_cu"][1].any() and (o["var_of_var_32x32"][0][6] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and not o["cb_mean"][0][6].any()


if __name__ == "__main__":
    if not os.path.exists(S.REF_SO) or not os.path.isdir(REF_SRC):
        sys.exit("needs oracle/_ref/libsvtref.so (`make -C oracle ref`) and the reference's sources (SVT_REF_SOURCE, default /root/reference/Source)")
    names = sys.argv[1:] or list(CASES)
    done = dict(run_case(nm) for nm in names)
    if len(done) == len(CASES):
        assert_not_vacuous(done)
