#!/usr/bin/env python3
"""Generate the noise-detection fixtures from the REFERENCE itself.  PicturePreProcessingOperations (Codec/EbPictureAnalysisProcess.c:3338) and what it calls are
`static`, so a small C driver of our own is written into a temporary directory; it #includes the reference's EbPictureAnalysisProcess.c by path, links against
oracle/_ref/libsvtref.so, fills lcuParamsArray with the reference's own LcuParamsInit and calls PicturePreProcessingOperations whole, with enableDenoiseSrcFlag 0
(the only value the reference assigns, Codec/EbResourceCoordinationProcess.c:304), on seeded planes.  Nothing compiled is kept.
Every case runs with ASM_TYPES 0 (the C routines) and, where this CPU has AVX2, again with what EbHevcGetCpuAsmType() returns; the two runs must agree byte
for byte, and the fixture records which paths were compared.
The picture's sum of noiseBlkVar >> 16 and totLcuCount are locals of the reference's functions.  The driver counts the evaluated blocks with the reference's
loop bounds (lcuParamsArray[..].isCompleteLcu for the full method) and takes the sum as the one integer s with (double)s / (double)count ==
picNoiseVarianceFloat - it checks that s - 1 and s + 1 give other quotients.
  -> tests/golden/panoise_<name>.npz: picture specifications and results (no planes).  Needs the reference tree and `make -C oracle ref`.
Usage: python tests/golden/make_pa_noise_golden.py [name ...]"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pa_noise_numpy as N  # noqa: E402
import pa_noise_pictures as P  # noqa: E402
import svtlib as S  # noqa: E402

REF_SRC = os.environ.get("SVT_REF_SOURCE", "/root/reference/Source")
PAD = 64

DRIVER = r"""
#include "EbPictureAnalysisProcess.c"
#include <stdio.h>
EB_U32 EbHevcGetCpuAsmType(void);
static void put(FILE *f, const void *p, size_t n) { if (fwrite(p, 1, n, f) != n) exit(3); }
static void get(FILE *f, void *p, size_t n) { if (fread(p, 1, n, f) != n) exit(4); }
static void desc(EbPictureBufferDesc_t *d, uint32_t w, uint32_t h)
{
    memset(d, 0, sizeof(*d));
    d->strideY = w + 2 * DRV_PAD, d->originX = d->originY = DRV_PAD, d->width = w, d->height = h;
    d->bufferY = calloc((size_t)d->strideY * (h + 2 * DRV_PAD), 1);
}
int main(int argc, char **argv)
{
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    uint32_t hd[4];
    if (argc < 4 || !fi || !fo) return 2;
    ASM_TYPES = argv[3][0] == 'c' ? 0 : EbHevcGetCpuAsmType();
    printf("%u\n", (unsigned)ASM_TYPES);
    get(fi, hd, sizeof(hd));
    const uint32_t w = hd[0], h = hd[1], method = hd[2], n = hd[3];
    const uint32_t wl = (w + 63) / 64, hl = (h + 63) / 64, lcus = wl * hl;
    SequenceControlSet_t *scs = calloc(1, sizeof(*scs));
    scs->lumaWidth = w, scs->lumaHeight = h, scs->lcuSize = 64;
    scs->pictureWidthInLcu = wl, scs->pictureHeightInLcu = hl, scs->lcuTotalCount = lcus;
    DeriveInputResolution(scs, w * h);
    LcuParamsInit(scs);
    PictureParentControlSet_t *pcs = calloc(1, sizeof(*pcs));
    PictureAnalysisContext_t *ctx = calloc(1, sizeof(*ctx));
    EbPictureBufferDesc_t in, den, noise, quarter, sixteenth;
    desc(&in, w, h), desc(&den, w, h), desc(&noise, w, 64), desc(&quarter, w / 2, h / 2), desc(&sixteenth, w / 4, h / 4);
    pcs->lcuTotalCount = lcus;
    pcs->enhancedPicturePtr = &in;
    pcs->lcuFlatNoiseArray = malloc(lcus);
    ctx->denoisedPicturePtr = &den, ctx->noisePicturePtr = &noise;
    /* totLcuCount: the blocks the reference's loops evaluate */
    uint32_t count = 0;
    if (method == NOISE_DETECT_FULL_PRECISION) {
        for (uint32_t i = 0; i < lcus; i++)
            count += scs->lcuParamsArray[i].isCompleteLcu ? 1 : 0;
    } else {
        const EbPictureBufferDesc_t *d = method == NOISE_DETECT_HALF_PRECISION ? &sixteenth : &quarter;
        const uint32_t size = method == NOISE_DETECT_HALF_PRECISION ? 16 : 32;
        for (uint32_t v = 0; v < (uint32_t)(d->height / 64); v++)
            for (uint32_t z = 0; z < (uint32_t)(d->width / 64); z++)
                for (uint32_t by = 64 * v; by < 64 * v + 64; by += size)
                    for (uint32_t bx = 64 * z; bx < 64 * z + 64; bx += size)
                        count += bx + size <= d->width && by + size <= d->height;
    }
    for (uint32_t p = 0; p < n; p++) {
        uint32_t th;
        get(fi, &th, 4);
        get(fi, in.bufferY, (size_t)in.strideY * (h + 2 * DRV_PAD));
        memset(pcs->lcuFlatNoiseArray, 0xAA, lcus);
        pcs->noiseDetectionMethod = (EB_NOISE_DETECT_MODE)method, pcs->noiseDetectionTh = (EB_U8)th, pcs->enableDenoiseSrcFlag = EB_FALSE;
        pcs->picNoiseClass = 0xEE;
        ctx->picNoiseVarianceFloat = 0;
        PicturePreProcessingOperations(pcs, ctx, scs, &quarter, &sixteenth, lcus, wl);
        const double f = ctx->picNoiseVarianceFloat;
        uint64_t sum = count ? (uint64_t)(f * (double)count + 0.5) : 0;
        if (count && ((double)sum / (double)count != f || (double)(sum + 1) / (double)count == f || (sum && (double)(sum - 1) / (double)count == f)))
            return 5;
        uint8_t cls = pcs->picNoiseClass;
        put(fo, pcs->lcuFlatNoiseArray, lcus), put(fo, &cls, 1), put(fo, &f, 8), put(fo, &sum, 8), put(fo, &count, 4);
    }
    fclose(fo);
    return 0;
}
"""


def run_reference(w, h, method, pictures, asm):
    """pictures: [(luma, threshold)] -> (records, the ASM_TYPES value the run had)"""
    ref_dir = os.path.dirname(S.REF_SO)
    inc = [ref_dir] + [os.path.join(REF_SRC, d) for d in ("API", "Lib/Codec", "Lib/C_DEFAULT", "Lib/ASM_SSE2", "Lib/ASM_SSSE3", "Lib/ASM_SSE4_1", "Lib/ASM_AVX2")]
    nl = N.lcu_count(w, h)
    with tempfile.TemporaryDirectory() as td:
        src, exe, fin, fout = (os.path.join(td, x) for x in ("driver.c", "driver", "in.bin", "out.bin"))
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-mavx2", "-msse4.1", "-w", "-DDRV_PAD=%d" % PAD] + ["-I" + i for i in inc] +
                              [src, "-o", exe, "-L" + ref_dir, "-lsvtref", "-Wl,-rpath," + ref_dir, "-lpthread", "-lm"])
        with open(fin, "wb") as f:
            f.write(np.array([w, h, method, len(pictures)], np.uint32).tobytes())
            for luma, th in pictures:
                f.write(np.uint32(th).tobytes())
                f.write(np.ascontiguousarray(np.pad(luma, PAD, mode="edge")).tobytes())
        asm_types = int(subprocess.check_output([exe, fin, fout, asm], text=True).split()[0])
        raw = np.fromfile(fout, np.uint8)
    rec_t = np.dtype([("flat", "u1", nl), ("cls", "u1"), ("variance_float", "<f8"), ("sum", "<u8"), ("count", "<u4")])
    assert raw.size == len(pictures) * rec_t.itemsize, (raw.size, len(pictures), rec_t.itemsize)
    return raw.view(rec_t), asm_types


def has_avx2():
    try:
        with open("/proc/cpuinfo") as f:
            return " avx2" in f.read()
    except OSError:
        return False


def run_case(name):
    method, w, h = P.CASES[name]
    specs = P.case_specs(name)
    pictures = [(P.picture(w, h, s), th) for s in specs for th in (0, 1)]
    r, asm0 = run_reference(w, h, method, pictures, "c")
    assert asm0 == 0
    paths = ["C_DEFAULT (ASM_TYPES 0)"]
    if has_avx2():
        r2, asm = run_reference(w, h, method, pictures, "best")
        assert asm & 2, "EbHevcGetCpuAsmType() %d has no AVX2 bit on a CPU with AVX2" % asm
        assert r.tobytes() == r2.tobytes(), "%s: the C and the AVX2 routines disagree" % name
        paths.append("AVX2 (ASM_TYPES %d)" % asm)
    n = len(specs)
    assert set(np.unique(r["flat"]).tolist()) <= {0, 1}                  # the reference resets the array before it sets flags
    out = dict(case=np.array([name, str(method), str(w), str(h)]), specs=np.array(json.dumps(specs)), paths=np.array(paths),
               flat_noise=r["flat"].reshape(n, 2, -1).copy(), pic_noise_class=r["cls"].reshape(n, 2).copy(),
               noise_variance_float=r["variance_float"].reshape(n, 2).copy(), noise_variance_sum=r["sum"].reshape(n, 2).copy(),
               block_count=r["count"].reshape(n, 2).copy())
    path = os.path.join(S.GOLDEN_DIR, "panoise_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("%-18s %2d pictures x 2 thresholds, %3d LCUs, %3d blocks: classes th0 %s, flagged th0 %s th1 %s; %s -> %s (%d KiB)" % (
        name, n, r["flat"].shape[1], int(r["count"][0]), out["pic_noise_class"][:, 0].tolist(), out["flat_noise"][:, 0].sum(axis=1).tolist(),
        out["flat_noise"][:, 1].sum(axis=1).tolist(), " = ".join(paths), os.path.basename(path), os.path.getsize(path) // 1024))
    return name, out


def evaluated(method, w, h):
    """the LCUs a method evaluates, as a mask over the picture's LCUs"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    m = np.zeros((hl, wl), bool)
    if method == P.FULL:
        m[:h // 64, :w // 64] = True
    else:
        step, per = (4, 4) if method == P.HALF else (2, 2)
        m[:(h // step // 64) * per, :(w // step // 64) * per] = True
    return m.reshape(-1)


def assert_not_vacuous(results):
    """every rule the fixtures are there for really decides something in them"""
    by_method = {m: [o for nm, o in results.items() if P.CASES[nm][0] == m] for m in (P.HALF, P.QUARTER, P.FULL)}
    for m, outs in by_method.items():
        seen = set(int(c) for o in outs for c in o["pic_noise_class"].reshape(-1))
        assert seen == {1, 2, 3, 4}, "method %s: classes %s" % (P.METHOD_NAME[m], sorted(seen))
    mixed = threshold = stacked = shared = folded = False
    for nm, o in results.items():
        method, w, h = P.CASES[nm]
        wl = (w + 63) // 64
        ev = evaluated(method, w, h)
        assert int(ev.sum()) == int(o["block_count"][0, 0]), nm
        assert not o["flat_noise"][:, :, ~ev].any(), nm + ": a flag on an LCU the method never evaluates"
        specs = json.loads(str(o["specs"]))
        for i, s in enumerate(specs):
            for t in (0, 1):
                f = o["flat_noise"][i, t]
                mixed |= bool(f[ev].any() and not f[ev].all())
                value = int(o["noise_variance_sum"][i, t]) // max(int(o["block_count"][i, t]), 1)
                if method == P.FULL and value >= 20 + (25 if h <= 720 else 0):
                    assert o["pic_noise_class"][i, t] == 4, nm
                    folded = True
            threshold |= bool((o["flat_noise"][i, 0] != o["flat_noise"][i, 1]).any())
            if method != P.FULL and s["amp"]:
                # two vertically stacked blocks of ONE 64x64 block of the decimated picture with the same background noise in their own rows and different
                # flags: the textured LCU of P.RECTS and the plain LCU above it.  Both are judged with ONE noise variance (that of the top rows of their
                # 64x64 block); what differs is their denoised variance.  This pair alone does not show the shared rule deciding - the next check does.
                per = 4 if method == P.HALF else 2
                f = o["flat_noise"][i, 1]
                for tx, ty in [(r[0], r[1]) for r in s["rects"] if r[4] == "texture" and r[2] == 1 and r[3] == 1]:
                    if ty == 0 or (ty - 1) // per != ty // per or (ty + 1) * 64 > h:
                        continue
                    a, b = (ty - 1) * wl + tx, ty * wl + tx
                    stacked |= bool(ev[a] and ev[b] and f[a] != f[b])
                # ... and the shared top-rows rule deciding: some flag differs from what the block's OWN rows of noise would give
                own, _ = N.detect(P.picture(w, h, s), method, 1, own_rows=True)
                shared |= bool((own[:f.size] != f).any())
    assert mixed, "no picture with flagged and unflagged evaluated LCUs"
    assert threshold, "no LCU whose flag differs between threshold 0 and 1"
    assert stacked, "no stacked blocks of one 64x64 block with the same noise and different flags"
    assert shared, "the shared noise strip decides no flag"
    assert folded, "no full-method picture at or above 20 + noiseTh"


if __name__ == "__main__":
    if not os.path.exists(S.REF_SO) or not os.path.isdir(REF_SRC):
        sys.exit("needs oracle/_ref/libsvtref.so (`make -C oracle ref`) and the reference's sources (SVT_REF_SOURCE, default /root/reference/Source)")
    names = sys.argv[1:] or list(P.CASES)
    done = dict(run_case(nm) for nm in names)
    if len(done) == len(P.CASES):
        assert_not_vacuous(done)
        print("the fixtures are not vacuous")
