"""numpy restatement of the two batched picture-analysis entries svt_amd_chroma_stats_batch_launch / svt_amd_picture_detect_batch_launch
(svt-hevc_amd/csrc/detect_kernels.hip), written from the reference's Codec/EbPictureAnalysisProcess.c - the lines are cited at each step.  The CPU suite pins
it on what the reference itself computed (tests/golden/padetect_*.npz, tests/test_pa_detect_cpu.py); the GPU tests then use it as the checker for seeded
variants.  Everything is integer arithmetic, bit-exact."""
import ctypes as C

import numpy as np

import svtlib as S

vp = C.c_void_p
CHROMA_MEANS, CHROMA_HISTOGRAM, CHROMA_REGION_AVG, CHROMA_SUM = range(4)
DETECT_LCU, DETECT_PICTURE = range(2)
LCU_CHROMA_DTYPE = np.dtype([("cb_mean", "u1", 21), ("cr_mean", "u1", 21), ("pad", "u1", 6)])
LCU_DETECT_DTYPE = np.dtype([("var_of_var_32x32", "<u8", 4), ("edge_cu", "<u2"), ("homogeneous", "u1"), ("edge_block_num", "u1"),
                             ("isolated_high_intensity", "u1"), ("sharp_edge", "u1"), ("pad", "u1", 10)])
PIC_DETECT_DTYPE = np.dtype([("pic_avg_variance", "<u2"), ("very_low_var_pic", "u1"), ("logo_pic", "u1"), ("lcu_block_percentage", "u1"), ("pad", "u1", 3)])
ALL_ONES = 0xFFFFFFFFFFFFFFFF
M64 = (1 << 64) - 1


class ChromaJob(C.Structure):
    _fields_ = [("cb", vp), ("cr", vp), ("pitch", C.c_uint32), ("want_means", C.c_uint8), ("want_histogram", C.c_uint8), ("pad", C.c_uint8 * 2)]


class ChromaArrays(C.Structure):
    _fields_ = [("means", vp), ("histogram", vp), ("region_average", vp), ("sum_chroma", vp)]


class DetectJob(C.Structure):
    _fields_ = [("stats", vp), ("chroma", vp), ("want_edge16", C.c_uint8), ("resolution_class", C.c_uint8), ("pad", C.c_uint8 * 6)]


class DetectArrays(C.Structure):
    _fields_ = [("lcu", vp), ("picture", vp)]


def declare(lib):
    lib.svt_amd_chroma_stats_batch_launch.restype = C.c_int
    lib.svt_amd_chroma_stats_batch_launch.argtypes = [vp, C.POINTER(ChromaJob), C.c_int, C.c_uint16, C.c_uint16, C.c_int, C.c_int, C.POINTER(ChromaArrays)]
    lib.svt_amd_chroma_stats_bytes.restype = C.c_size_t
    lib.svt_amd_chroma_stats_bytes.argtypes = [C.c_uint16, C.c_uint16, C.c_int, C.c_int, C.c_int]
    lib.svt_amd_picture_detect_batch_launch.restype = C.c_int
    lib.svt_amd_picture_detect_batch_launch.argtypes = [vp, C.POINTER(DetectJob), C.c_int, C.c_uint16, C.c_uint16, C.POINTER(DetectArrays)]
    lib.svt_amd_picture_detect_bytes.restype = C.c_size_t
    lib.svt_amd_picture_detect_bytes.argtypes = [C.c_uint16, C.c_uint16, C.c_int]
    lib.svt_amd_last_error.restype = C.c_char_p
    return lib


def chroma_sizes(w, h, rw, rh):
    """bytes of ONE picture in each array of svt_amd_chroma_stats_batch_launch"""
    return [S.lcu_count(w, h) * 48, rw * rh * 2 * 1024, 128, 16]


def detect_sizes(w, h):
    return [S.lcu_count(w, h) * 48, 8]


# ---- entry 1 ---------------------------------------------------------------------------------------------------------------------------------

def chroma_means(cb, cr, w, h):
    """ComputeChromaBlockMean (:1448) / ZeroOutChromaBlockMean (:1383) of every LCU -> LCU_CHROMA_DTYPE[lcus]"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    out = np.zeros(wl * hl, LCU_CHROMA_DTYPE)
    for n in range(wl * hl):
        x, y = 64 * (n % wl), 64 * (n // wl)
        if x + 64 > w or y + 64 > h:
            continue                                                    # incomplete LCUs: zeros (:3924)
        for name, plane in (("cb_mean", cb), ("cr_mean", cr)):
            blk = plane[y // 2:y // 2 + 32, x // 2:x // 2 + 32].astype(np.int64)
            # ComputeSubMean8x8_SSE2_INTRIN (ASM_SSE2/EbComputeMean_Intrinsic_SSE2.c:53): rows 0, 2, 4, 6 of each 8x8, << 3
            m16 = blk[::2].reshape(4, 4, 4, 8).sum(axis=(1, 3)) << 3    # [by][bx]
            m32 = [(m16[2 * qy, 2 * qx] + m16[2 * qy, 2 * qx + 1] + m16[2 * qy + 1, 2 * qx] + m16[2 * qy + 1, 2 * qx + 1]) >> 2 for qy in range(2) for qx in range(2)]
            m64 = (m32[0] + m32[1] + m32[3] + m32[3]) >> 2               # :1586-1587: block 3 twice, block 2 never
            out[n][name][0] = m64 >> 8
            out[n][name][1:5] = [m >> 8 for m in m32]
            out[n][name][5:21] = (m16 >> 8).reshape(16)
    return out


def regions_of(w, h, rw, rh):
    """(a, b, x0, y0, width, height) of the luma regions (:3458-3476): width / regions, the remainder to the last one"""
    ww, hh = w // rw, h // rh
    return [(a, b, a * ww, b * hh, w - a * ww if a == rw - 1 else ww, h - b * hh if b == rh - 1 else hh) for a in range(rw) for b in range(rh)]


def chroma_histograms(cb, cr, w, h, rw, rh):
    """SubSampleChromaGeneratePixelIntensityHistogramBins (:3440) -> histogram[rw][rh][2][256], region_average[64][2], sum_chroma[2]"""
    hist, ravg, total = np.zeros((rw, rh, 2, 256), np.uint32), np.zeros((64, 2), np.uint8), np.zeros(2, np.uint64)
    for a, b, x0, y0, ww, hh in regions_of(w, h, rw, rh):
        for c, plane in enumerate((cb, cr)):
            # CalculateHistogram (:204) at decimStep 4 from the luma origin >> 1 over the luma size >> 1
            s = plane[y0 >> 1:(y0 >> 1) + (hh >> 1):4, x0 >> 1:(x0 >> 1) + (ww >> 1):4]
            hist[a, b, c] = (np.bincount(s.reshape(-1), minlength=256) + 1) << 4          # bins start at 1, end << 4 (:3467, :3493)
            total_c = int(s.sum(dtype=np.uint64)) << 4                                    # :3489
            total[c] += np.uint64(total_c)
            ravg[a * rh + b, c] = ((total_c + ((ww * hh) >> 3)) // ((ww * hh) >> 2)) & 0xFF  # :3491
    return hist, ravg, total


def average_intensity(total, w, h):
    """CalculateInputAverageIntensity (:3983-3984) of one plane's sum"""
    return ((int(total) + ((w * h) >> 3)) // ((w * h) >> 2)) & 0xFF


# ---- entry 2 ---------------------------------------------------------------------------------------------------------------------------------

def potential_logo(w, h, cls):
    """lcuParams->potentialLogoLcu (Codec/EbSequenceControlSet.c:253-272); the comparisons are signed, as in the reference"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    cols, rows = ((3, 2), (7, 4), (7, 4), (14, 8))[cls]
    out = np.zeros(wl * hl, np.uint8)
    for n in range(wl * hl):
        ox, oy = 64 * (n % wl), 64 * (n // wl)
        out[n] = ((ox >= w - cols * 64 or ox < cols * 64) and oy < rows * 64) or oy >= h - rows * 64
    return out


def grad16(y, cr, cb, k):
    """contextPtr->grad[lcu][5 + k] (:3551-3594); y / cr / cb: the sixteen 16x16 means as ints"""
    d = lambda i, j: abs(y[i] - y[j]) + abs(cr[i] - cr[j]) + abs(cb[i] - cb[j])
    x, r = k & 3, k >> 2
    gx = gy = nx = ny = 0
    if x != 0:
        gx, nx = gx + d(k, k - 1), nx + 1
    if x != 3:
        gx, nx = gx + d(k + 1, k), nx + 1
    if r != 0:
        gy, ny = gy + d(k, k - 4), ny + 1
    if r != 3:
        gy, ny = gy + d(k + 4, k), ny + 1
    return (gx // nx + gy // ny) & 0xFFFF


def detect(variance, y_mean, chroma, w, h, want_edge16, cls):
    """ComputePictureSpatialStatistics (:3879) after the block statistics: variance[lcus][85] (u16), y_mean[lcus][85], chroma: LCU_CHROMA_DTYPE[lcus] or None
    -> (LCU_DETECT_DTYPE[lcus], PIC_DETECT_DTYPE scalar record)"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    n_lcu = wl * hl
    var = np.asarray(variance).astype(object)                          # Python integers: no silent wrap anywhere
    mean = np.asarray(y_mean).astype(np.int64)
    lcu, pic = np.zeros(n_lcu, LCU_DETECT_DTYPE), np.zeros(1, PIC_DETECT_DTYPE)[0]
    complete = np.array([64 * (n % wl) + 64 <= w and 64 * (n // wl) + 64 <= h for n in range(n_lcu)])
    # picAvgVariance (:3930-3933): ALL LCUs, truncated to 16 bits
    avg = (sum(int(var[n][0]) for n in range(n_lcu)) // n_lcu) & 0xFFFF
    pic["pic_avg_variance"] = avg
    # DetermineHomogeneousRegionInPicture (:3751)
    low = cnt = 0
    for n in range(n_lcu):
        lcu[n]["homogeneous"] = 1
        if not complete[n]:
            lcu[n]["var_of_var_32x32"] = ALL_ONES                      # :3850
            continue
        cnt += 1
        low += int(var[n][0]) < 5                                      # LCU_LOW_VAR_TH
        v8 = [int(v) for v in var[n][21:85]]
        for q in range(4):
            blk = [v8[(4 * (q >> 1) + r) * 8 + 4 * (q & 1) + c] for r in range(4) for c in range(4)]
            # the squares of the 16-bit variances summed in 64 bits, >> 4; the subtraction is unsigned 64-bit (:3808-3810)
            lcu[n]["var_of_var_32x32"][q] = ((sum(v * v for v in blk) >> 4) - (sum(blk) >> 4) ** 2) & M64
        vov64 = ((sum(v * v for v in v8) >> 6) - (sum(v8) >> 6) ** 2) & M64
        if vov64 > 64 * 64:                                            # VAR_BASED_DETAIL_PRESERVATION_SELECTOR_THRSLHD (:3840)
            lcu[n]["homogeneous"] = 0
    pct = low * 100 // cnt if cnt else 0
    pic["very_low_var_pic"], pic["logo_pic"] = pct > 60, pct > 80      # :3856-3868
    # EdgeDetectionMeanLumaChroma16x16 (:3522)
    if want_edge16:
        logo = potential_logo(w, h, cls)
        grads, max_grad = {}, 1
        for n in range(n_lcu):
            if logo[n] and complete[n]:
                y, cr, cb = ([int(v) for v in a] for a in (mean[n][5:21], chroma[n]["cr_mean"][5:21], chroma[n]["cb_mean"][5:21]))
                grads[n] = [grad16(y, cr, cb, k) for k in range(16)]
                max_grad = max(max_grad, max(grads[n]))
        for n, g in grads.items():
            lcu[n]["edge_cu"] = sum((min(g[k] * 765 // max_grad, 255) >= 30) << k for k in range(16))   # :3609
    # EdgeDetection (:3627)
    thr = avg * 70 // 100
    edges = 0
    trigger = np.zeros(n_lcu, bool)
    for n in range(n_lcu):
        col, row = n % wl, n // wl
        if not (0 < col < wl - 1 and 0 < row < hl - 1):
            continue
        lcu[n]["edge_block_num"] = int(var[n][0]) > thr
        edges += int(lcu[n]["edge_block_num"])
        if int(var[n][0]) > 200 and sum(int(v) < 20 for v in var[n][5:21]) > 4:
            lcu[n]["sharp_edge"] = 1
        if 3 < col < wl - 4 and 3 < row < hl - 4 and mean[n][0] > 180:
            trigger[n] = any(mean[m][0] < 120 for m in (n - 1, n + 1, n - wl, n + wl))
    # isolatedHighIntensityLcu: LCU n clears its own flag when the raster loop reaches it (:3669), a trigger m marks its 9x9 (:3726-3731):
    # the final state of n is 1 exactly when some trigger m >= n lies within +-4 columns and rows
    for m in np.flatnonzero(trigger):
        for i in range(-4, 5):
            for j in range(-4, 5):
                n = m + i * wl + j
                if n <= m:
                    lcu[n]["isolated_high_intensity"] = 1
    pic["lcu_block_percentage"] = (edges * 100 // n_lcu) & 0xFF          # :3743
    return lcu, pic


def detect_sequential(variance, y_mean, w, h):
    """isolatedHighIntensityLcu by running the reference's raster loop literally (clear, then mark): pins the closed form above"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    mean = np.asarray(y_mean).astype(np.int64)
    iso = np.zeros(wl * hl, np.uint8)
    for n in range(wl * hl):
        col, row = n % wl, n // wl
        iso[n] = 0
        if 3 < col < wl - 4 and 3 < row < hl - 4 and mean[n][0] > 180 and any(mean[m][0] < 120 for m in (n - 1, n + 1, n - wl, n + wl)):
            for i in range(-4, 5):
                for j in range(-4, 5):
                    iso[n + i * wl + j] = 1
    return iso
