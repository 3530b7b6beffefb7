"""Seeded inputs at the ends of the sample and parameter ranges of the in-loop filters (deblocking cores, SAO statistics, SAO application), shared by
tests/golden/make_filter_extremes_golden.py (which records what the reference computes on them), tests/test_filter_extremes_cpu.py and
tests/test_gpu_filter_extremes.py.  numpy only: every user rebuilds byte-identical inputs from the seeds, the fixtures hold results alone."""
import numpy as np

STRIDE = 80
GATHER_SIZES = [(64, 64), (40, 56), (16, 8), (8, 8)]
GATHER_KINDS = ["clip_all_pos", "clip_all_neg", "clip_half", "flat_band_0", "flat_band_max", "flat_band_mid", "two_bands", "stripes"]


def maxv_of(bps):
    return 255 if bps == 1 else 1023


def dtype_of(bps):
    return np.uint8 if bps == 1 else np.uint16


def _far_pair(rng, bps, shape, positive):
    """(src, rec) whose difference lies beyond the signed 8-bit range everywhere: |src - rec| >= 130 (8 bit), >= 800 (10 bit)"""
    lo = rng.integers(0, 101, shape)
    hi = rng.integers(230, 256, shape) if bps == 1 else rng.integers(900, 1024, shape)
    return (hi, lo) if positive else (lo, hi)


def gather_pattern(kind, bps, w, h, seed, stride=None):
    """-> (src, rec), h rows of `stride` samples; the patterns are described in gather_cases()"""
    stride = stride or (STRIDE if w <= 64 else w)
    rng = np.random.default_rng([11, bps, GATHER_KINDS.index(kind), w, h, seed])
    maxv, shape = maxv_of(bps), (h, stride)
    band = 8 if bps == 1 else 32                       # samples per band
    src = rng.integers(0, maxv + 1, shape)
    if kind in ("clip_all_pos", "clip_all_neg"):
        src, rec = _far_pair(rng, bps, shape, kind == "clip_all_pos")
    elif kind == "clip_half":
        fs, fr = _far_pair(rng, bps, shape, True)
        swap = rng.random(shape) < 0.5
        fs, fr = np.where(swap, fr, fs), np.where(swap, fs, fr)
        near = rng.integers(60, 200, shape)
        far = rng.random(shape) < 0.5
        rec = np.where(far, fr, near)
        src = np.where(far, fs, near + rng.integers(-9, 10, shape))
    elif kind.startswith("flat_band"):
        rec = np.full(shape, {"0": 0, "max": maxv, "mid": (maxv + 1) // 2}[kind[10:]])
    elif kind == "two_bands":
        rec = np.where(np.arange(h)[:, None] < h // 2, 3, 20) * band + rng.integers(0, band, shape)
        src = rec + rng.integers(-20, 21, shape)
    else:                                               # stripes: a sample checker of bands 0 and 31
        r = rng.integers(0, band, shape)
        rec = np.where((np.arange(h)[:, None] + np.arange(stride)[None, :]) & 1, maxv - r, r)
    return np.clip(src, 0, maxv).astype(dtype_of(bps)), np.clip(rec, 0, maxv).astype(dtype_of(bps))


def gather_cases(bps):
    """yields (name, src, rec, w, h), stride 80:
    clip_all_pos / _neg  every difference beyond +127 / -128 (8 bit; the 10-bit twins reach +-1023 and must not clip)
    clip_half            half the samples beyond +-127, half within +-9
    flat_band_0/max/mid  recon constant: one band holds every sample, so every wave takes the one-atomic-per-wave path
    two_bands            rows < h/2 in band 3, the rest in band 20: the wave that holds the interior index across the boundary is mixed
    stripes              neighbouring samples alternate between bands 0 and 31"""
    for kind in GATHER_KINDS:
        for w, h in GATHER_SIZES:
            src, rec = gather_pattern(kind, bps, w, h, 0)
            yield "%s_%dx%d" % (kind, w, h), src, rec, w, h


def gather_picture(bps, w, h, stride, seed):
    """a picture whose 64x64 cells cycle through the gather patterns -> (src, rec)"""
    src, rec = np.zeros((h, stride), dtype_of(bps)), np.zeros((h, stride), dtype_of(bps))
    k = seed
    for y0 in range(0, h, 64):
        for x0 in range(0, stride, 64):
            ch, cw = min(64, h - y0), min(64, stride - x0)
            s, r = gather_pattern(GATHER_KINDS[k % len(GATHER_KINDS)], bps, 64, 64, k, stride=64)
            src[y0:y0 + ch, x0:x0 + cw], rec[y0:y0 + ch, x0:x0 + cw] = s[:ch, :cw], r[:ch, :cw]
            k += 1
    return src, rec


# ---- SAO application -------------------------------------------------------------------------------------------------
APPLY_PLANES = [("blocks", 64, 64), ("checker", 64, 64), ("blocks", 24, 40), ("checker", 8, 8), ("mid", 24, 40)]
APPLY_BANDS = [0, 28, 29, 30, 31]


def apply_m(bps):
    return 7 if bps == 1 else 31


def apply_offsets(bps):
    m = apply_m(bps)
    return [np.array([-m, -m, 0, m, m], np.int8), np.array([m, m, 0, -m, -m], np.int8)]


def saturated(rng, bps, kind, shape):
    """samples within 3 of either end: `blocks` 4x4 blocks at one end each, `checker` a sample checker (its distances from the ends repeat every 16
    samples both ways, which keeps the recorded results small); `mid`: the whole range"""
    maxv = maxv_of(bps)
    h, w = shape
    low = rng.integers(0, 4, shape)
    if kind == "checker":
        low = np.tile(low[:16, :16], ((h + 15) // 16, (w + 15) // 16))[:h, :w]
    if kind == "mid":
        return rng.integers(0, maxv + 1, shape).astype(dtype_of(bps))
    if kind == "blocks":
        top = np.kron(rng.integers(0, 2, ((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), np.int64))[:h, :w]
    else:
        top = (np.arange(h)[:, None] + np.arange(w)[None, :]) & 1
    return np.where(top, maxv - low, low).astype(dtype_of(bps))


def apply_cases(bps):
    """yields (name, rec, left, upper, w, h): rec has h + 2 rows of 80 (the LCU area starts at its first sample), left h + 2 samples, upper w + 3
    samples of which element 0 is the top-left corner"""
    for i, (kind, w, h) in enumerate(APPLY_PLANES):
        rng = np.random.default_rng([12, bps, i])
        rec = saturated(rng, bps, kind, (h + 2, STRIDE))
        left = saturated(rng, bps, kind if kind == "mid" else "checker", (1, h + 2))[0]
        upper = saturated(rng, bps, kind if kind == "mid" else "checker", (1, w + 3))[0]
        yield "%s_%dx%d" % (kind, w, h), rec, left, upper, w, h


def apply_ops():
    """(kind, band or edge class, index into apply_offsets) in the order the fixture stores the results"""
    return [("bo", b, s) for b in APPLY_BANDS for s in (0, 1)] + [("eo", t, s) for t in range(4) for s in (0, 1)]


def apply_meant_to_clip(name, op):
    """Worked out from the inputs: a band offset clips where the band at an end of the range gets an offset pointing outwards - band 0 is offset[0], and
    band 31 is offset[31 - position], i.e. +m for (28, first set) and (30 / 31, second set), 0 for position 29.  An edge offset clips where a sample near
    an end is a local extremum pushed outwards: the first set (valleys down, peaks up) on every saturated plane; the second set needs a valley among
    high samples, which the 4x4 blocks of the larger `blocks` planes have and a sample checker has only along its diagonals."""
    kind, size = name.split("_")
    if kind == "mid":
        return False
    if op[0] == "bo":
        return (op[1], op[2]) in ((0, 0), (28, 0), (30, 1), (31, 1))
    return op[2] == 0 or (kind == "blocks" and size != "8x8")


# ---- deblocking cores ------------------------------------------------------------------------------------------------
def dlf_shift(bps):
    return 0 if bps == 1 else 2


def _step_block(rng, bps, n, vertical, level, step, noise):
    """n x n block, flat at `level` on the p side of the middle edge and `step` away from it (inwards) on the q side"""
    maxv = maxv_of(bps)
    base = {"0": 0, "mid": (maxv + 1) // 2, "max": maxv}[level]
    other = base - step if level == "max" else base + step
    a = np.where(np.arange(n)[None, :] < n // 2, base, other) + np.zeros((n, 1), np.int64)
    if noise:
        a = a + rng.integers(-1, 2, (n, n))
    a = np.clip(a, 0, maxv)
    return np.ascontiguousarray((a if vertical else a.T).astype(dtype_of(bps)))


def dlf_luma_cases(bps):
    """yields dict(block 16x16, off, vertical, tc, beta, filters): step edges of height 0, 1, 2, tc, 5*tc/2 and 10*tc between flat halves at 0, mid-range
    and the maximum, plain and with +-1 noise, (tc, beta) from {0, 1, 24} x {0, 1, 64} (<< 2 for 10 bit).
    `filters`: without noise d = 0 < beta = max; a step s of 2 or tc passes the strong-filter test ((5 * tc + 1) >> 1 > s) and moves q0 to
    p + ((5 * s + 4) >> 3) != q; s = 5 * tc / 2 fails it and takes the normal filter with delta = (9 * s + 8) >> 4, 0 < |delta| < 10 * tc."""
    sh = dlf_shift(bps)
    rng = np.random.default_rng([13, bps])
    for vertical in (1, 0):
        for tc in (0, 1 << sh, 24 << sh):
            for beta in (0, 1 << sh, 64 << sh):
                for step in sorted({0, 1, 2, tc, 5 * tc // 2, 10 * tc}):
                    for level in ("0", "mid", "max"):
                        for noise in (0, 1):
                            yield dict(block=_step_block(rng, bps, 16, vertical, level, step, noise), vertical=vertical, tc=tc, beta=beta,
                                       off=(8 * 16 + 8) if vertical else (8 * 16 + 6),
                                       filters=bool(tc == 24 << sh and beta == 64 << sh and not noise and step in (2, tc, 5 * tc // 2)))


def dlf_chroma_cases(bps):
    """yields dict(cb, cr 8x8, off, vertical, cb_tc, cr_tc, cb_filters, cr_filters); tc from {0, 1, 24} (8 bit) / {0, 4, 96} (10 bit), Cr takes the next
    value of the cycle.  `filters`: without noise delta = clip(+-tc, (3 * s + 4) >> 3) != 0 for tc >= 1 and a step s >= 2."""
    sh = dlf_shift(bps)
    tcs = [0, 1 << sh, 24 << sh]
    rng = np.random.default_rng([14, bps])
    for vertical in (1, 0):
        for i, tc in enumerate(tcs):
            tcr = tcs[(i + 1) % 3]
            for step in sorted({0, 1, 2, tc, 5 * tc // 2, 10 * tc}):
                for level in ("0", "mid", "max"):
                    for noise in (0, 1):
                        yield dict(cb=_step_block(rng, bps, 8, vertical, level, step, noise), cr=_step_block(rng, bps, 8, vertical, level, step, noise),
                                   vertical=vertical, cb_tc=tc, cr_tc=tcr, off=4 * 8 + 4, cb_filters=bool(tc and step >= 2 and not noise),
                                   cr_filters=bool(tcr and step >= 2 and not noise))


def dlf_cases(bps):
    """(luma cases, chroma cases) of one bit depth"""
    return list(dlf_luma_cases(bps)), list(dlf_chroma_cases(bps))


def luma_window(block, vertical):
    """the 8 x 4 samples a luma edge core may write (p3..q3 of the four lines), the edge along the filter direction; + the block without them"""
    b = block if vertical else block.T
    rows = slice(8, 12) if vertical else slice(6, 10)
    rest = b.copy()
    rest[rows, 4:12] = 0
    return b[rows, 4:12].copy(), rest


def chroma_window(block, vertical):
    b = block if vertical else block.T
    rest = b.copy()
    rest[4:6, 2:6] = 0
    return b[4:6, 2:6].copy(), rest


def step_plane(bps, w, h, seed):
    """w x h plane of 8x8 blocks: neighbours differ by 0, 1, 2, 5, 20 and 60 (x 4 for 10 bit) around 0, mid-range and the maximum"""
    rng = np.random.default_rng([15, bps, w, h, seed])
    maxv, sc = maxv_of(bps), 1 << dlf_shift(bps)
    steps = np.array([0, 1, 2, 5, 20, 60]) * sc
    by, bx = (h + 7) // 8, (w + 7) // 8
    band = (np.arange(by)[:, None] * 2 + np.arange(bx)[None, :] // 3 + seed) % 3       # 0: near 0, 1: mid-range, 2: near the maximum
    base = np.choose(band, [0, (maxv + 1) // 2, maxv])
    amount = steps[rng.integers(0, 6, (by, bx))] * ((np.arange(by)[:, None] + np.arange(bx)[None, :]) & 1)
    blocks = np.where(band == 2, base - amount, base + amount)
    return np.clip(np.kron(blocks, np.ones((8, 8), np.int64))[:h, :w], 0, maxv).astype(dtype_of(bps))


DLF_HDR = np.dtype([("width", "<u4"), ("height", "<u4"), ("bytes_per_sample", "<u4"), ("qp_stride", "<u4"),
                    ("tc_offset", "<i4"), ("beta_offset", "<i4"), ("cb_qp_offset", "<i4"), ("cr_qp_offset", "<i4")])
DLF_SETS = {"a": (51, 6, 6, 12, -12), "b": (0, -6, -6, -12, 12), "c": (None, 0, 0, 0, 0)}     # qp, tc / beta offset, Cb / Cr qp offset


def dlf_picture(bps, w, h, which):
    """picture record as tests/test_oracle_dlf_golden.py:oracle_dlf takes it: blocky planes, strength 2 on every edge, one of the parameter sets"""
    qp, tco, bo, cbo, cro = DLF_SETS[which]
    hdr = np.zeros(1, DLF_HDR)[0]
    hdr["width"], hdr["height"], hdr["bytes_per_sample"], hdr["qp_stride"] = w, h, bps, w // 8 + 3
    hdr["tc_offset"], hdr["beta_offset"], hdr["cb_qp_offset"], hdr["cr_qp_offset"] = tco, bo, cbo, cro
    planes = [step_plane(bps, w, h, 0), step_plane(bps, w // 2, h // 2, 1), step_plane(bps, w // 2, h // 2, 2)]
    nlcu = ((w + 63) // 64) * ((h + 63) // 64)
    qs = int(hdr["qp_stride"])
    if qp is None:
        qmap = (((np.arange(h // 8)[:, None] + np.arange(qs)[None, :]) & 1) * 51).astype(np.uint8).reshape(-1)
    else:
        qmap = np.full(qs * (h // 8), qp, np.uint8)
    return dict(hdr=hdr, pre=planes, bsv=np.full((nlcu, 256), 2, np.uint8), bsh=np.full((nlcu, 256), 2, np.uint8), qp=qmap)


# ---- SAO application, whole pictures ---------------------------------------------------------------------------------
SAO_LCU = np.dtype([("merge_left", "u1"), ("merge_up", "u1"), ("edge_flags", "u1"), ("pad", "u1"), ("type", "<u4", 2),
                    ("offset", "<i4", (3, 4)), ("band", "<u4", 3)])


def picture_edge_flags(cols, rows):
    i = np.arange(cols * rows)
    cx, cy = i % cols, i // cols
    return ((cx == 0) * 1 | (cx == cols - 1) * 2 | (cy == 0) * 4 | (cy == rows - 1) * 8).astype(np.uint8)


def sao_apply_picture(bps, w, h):
    """-> (planes, lcus): saturated planes; per LCU a type from 0..5, offsets from -m..m with more than a third at +-m, band positions from 0..31 with
    29, 30 and 31 each on a band-offset LCU (of one component each where the picture has two LCUs only)"""
    rng = np.random.default_rng([16, bps, w, h])
    m = apply_m(bps)
    planes = [saturated(rng, bps, "blocks" if k != 1 else "checker", (ph, pw)) for k, (pw, ph) in enumerate(((w, h), (w // 2, h // 2), (w // 2, h // 2)))]
    cols, rows = (w + 63) // 64, (h + 63) // 64
    n = cols * rows
    lcus = np.zeros(n, SAO_LCU)
    other = np.array([1, 2, 3, 4, 0])[(np.arange(n) // 2) % 5]
    even = np.arange(n) % 2 == 0
    lcus["type"][:, 0], lcus["type"][:, 1] = np.where(even, 5, other), np.where(even, other, 5)     # band offset on every other LCU, luma and chroma in turn
    off = rng.integers(-m, m + 1, (n, 3, 4))
    ends = rng.random((n, 3, 4)) < 0.45
    lcus["offset"] = np.where(ends, np.where(rng.random((n, 3, 4)) < 0.5, -m, m), off)
    lcus["band"] = rng.integers(0, 32, (n, 3))
    for c in range(3):
        five = np.flatnonzero(lcus["type"][:, 0 if c == 0 else 1] == 5)
        for k, i in enumerate(five[:4]):
            lcus["band"][i, c] = ((31, 29, 30, 0), (29, 30, 31, 0), (30, 31, 29, 0))[c][k]
    lcus["edge_flags"] = picture_edge_flags(cols, rows) | (rng.integers(0, 16, n) & rng.integers(0, 16, n)).astype(np.uint8)
    return planes, lcus


# ---- the chain statistics -> decision -> application -------------------------------------------------------------------
CHAIN_KINDS = ["flat", "checker", "ends"]
CHAIN_W, CHAIN_H = 192, 128


def chain_picture(bps, kind):
    """-> (src planes, rec planes) of a 192x128 4:2:0 picture:
    flat     src all 0 against rec all maximum (every LCU one band, count 3,844, the largest differences the decision sees)
    checker  black / white 8x8 blocks, rec = src pulled 3 inwards
    ends     samples within 3 of either end, rec = src + 2 for nine samples in ten and src - 2 for the tenth: the band's offset follows the nine and
             pushes the tenth out of the range"""
    rng = np.random.default_rng([17, bps, CHAIN_KINDS.index(kind)])
    maxv = maxv_of(bps)
    src, rec = [], []
    for pw, ph in ((CHAIN_W, CHAIN_H), (CHAIN_W // 2, CHAIN_H // 2), (CHAIN_W // 2, CHAIN_H // 2)):
        if kind == "flat":
            s, r = np.zeros((ph, pw), np.int64), np.full((ph, pw), maxv)
        elif kind == "checker":
            s = (((np.arange(ph)[:, None] // 8 + np.arange(pw)[None, :] // 8) & 1) * maxv)
            r = np.where(s > 0, s - 3, s + 3)
        else:
            s = saturated(rng, bps, "blocks", (ph, pw)).astype(np.int64)
            r = s + np.where(rng.random((ph, pw)) < 0.9, 2, -2)
        src.append(np.clip(s, 0, maxv).astype(dtype_of(bps)))
        rec.append(np.clip(r, 0, maxv).astype(dtype_of(bps)))
    return src, rec


# ---- running the leaf cases through one implementation ---------------------------------------------------------------
# Three implementations share the cases: the reference's own symbols and the product's leaf wrappers (same signatures, `Leaves`), and the CPU oracle.
import ctypes as C  # noqa: E402

STATS = np.dtype([("boDiff", "<i4", 32), ("boCount", "<u2", 32), ("eoDiff", "<i4", (4, 5)), ("eoCount", "<u2", (4, 5))])
_vp, _u32, _i32, _u8 = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint8
EO_NAMES = ["SAOApplyEO_0", "SAOApplyEO_90", "SAOApplyEO_135", "SAOApplyEO_45"]


def P(a, off=0):
    return a.ctypes.data + off


class Leaves:
    """the reference's C symbols (prefix "") or the product's wrappers of the same signatures (prefix "svt_amd_")"""

    def __init__(self, lib, prefix=""):
        self.lib, self.prefix = lib, prefix

    def fn(self, name):
        return getattr(self.lib, self.prefix + name)

    def gather(self, bps, only, src, rec, stride, w, h, st):
        a = [_vp(P(src)), _u32(stride), _vp(P(rec)), _u32(stride), _u32(w), _u32(h)]
        bo = [_vp(P(st["boDiff"])), _vp(P(st["boCount"]))]
        eo = [_vp(P(st["eoDiff"])), _vp(P(st["eoCount"]))]
        if only:
            self.fn("GatherSaoStatisticsLcu_OnlyEo_90_45_135_Lossy" if bps == 1 else "GatherSaoStatisticsLcu_62x62_OnlyEo_90_45_135_16bit")(*(a + eo))
        else:
            self.fn("GatherSaoStatisticsLcuLossy_62x62" if bps == 1 else "GatherSaoStatisticsLcu_62x62_16bit")(*(a + bo + eo))

    def apply(self, bps, op, rec, left, upper, w, h, off):
        if op[0] == "bo":
            self.fn("SAOApplyBO" + ("" if bps == 1 else "16bit"))(_vp(P(rec)), _u32(STRIDE), _u32(op[1]), _vp(P(off)), _u32(h), _u32(w))
            return
        fn, up = self.fn(EO_NAMES[op[1]] + ("_16bit" if bps == 2 else "")), _vp(P(upper, bps))
        if op[1] == 0:
            fn(_vp(P(rec)), _u32(STRIDE), _vp(P(left)), _vp(P(off)), _u32(h), _u32(w))
        elif op[1] == 1:
            fn(_vp(P(rec)), _u32(STRIDE), up, _vp(P(off)), _u32(h), _u32(w))
        else:
            fn(_vp(P(rec)), _u32(STRIDE), _vp(P(left)), up, _vp(P(off)), _u32(h), _u32(w))

    def luma(self, bps, block, off, vertical, tc, beta):
        self.fn("Luma4SampleEdgeDLFCore" + ("" if bps == 1 else "16bit"))(_vp(P(block, off * bps)), _u32(16), _u8(vertical), _i32(tc), _i32(beta))

    def chroma(self, bps, cb, cr, off, vertical, tcb, tcr):
        self.fn("Chroma2SampleEdgeDLFCore" + ("" if bps == 1 else "16bit"))(_vp(P(cb, off * bps)), _vp(P(cr, off * bps)), _u32(8), _u8(vertical),
                                                                           _u8(tcb), _u8(tcr))


class Oracle:
    def __init__(self, lib):
        self.lib = lib
        lib.svt_oracle_Luma4SampleEdgeDLFCore.argtypes = [C.c_int, _vp, _u32, C.c_int, _i32, _i32]
        lib.svt_oracle_Chroma2SampleEdgeDLFCore.argtypes = [C.c_int, _vp, _vp, _u32, C.c_int, _u8, _u8]
        lib.svt_oracle_GatherSaoStatistics.argtypes = [C.c_int, C.c_int, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]
        lib.svt_oracle_SAOApplyBO.argtypes = [C.c_int, _vp, _u32, _u32, _vp, _u32, _u32]
        lib.svt_oracle_SAOApplyEO.argtypes = [C.c_int, C.c_int, _vp, _u32, _vp, _vp, _vp, _u32, _u32]

    def gather(self, bps, only, src, rec, stride, w, h, st, sp=0, rp=0):
        self.lib.svt_oracle_GatherSaoStatistics(bps, only, P(src, sp), stride, P(rec, rp), stride, w, h, P(st["boDiff"]), P(st["boCount"]),
                                                P(st["eoDiff"]), P(st["eoCount"]))

    def apply(self, bps, op, rec, left, upper, w, h, off):
        if op[0] == "bo":
            self.lib.svt_oracle_SAOApplyBO(bps, P(rec), STRIDE, op[1], P(off), h, w)
        else:
            self.lib.svt_oracle_SAOApplyEO(bps, op[1], P(rec), STRIDE, P(left), P(upper, bps), P(off), h, w)

    def luma(self, bps, block, off, vertical, tc, beta):
        self.lib.svt_oracle_Luma4SampleEdgeDLFCore(bps, P(block, off * bps), 16, vertical, tc, beta)

    def chroma(self, bps, cb, cr, off, vertical, tcb, tcr):
        self.lib.svt_oracle_Chroma2SampleEdgeDLFCore(bps, P(cb, off * bps), P(cr, off * bps), 8, vertical, tcb, tcr)


def stats_record():
    """one statistics record whose four fields can be handed to C separately"""
    return {k: np.zeros(STATS[k].shape, STATS[k].base) for k in STATS.names}


def run_gather(impl, bps):
    """-> STATS[case][only_eo]; with only_eo the band arrays and edge class 0 stay zero, as the reference leaves what it is handed"""
    cases = list(gather_cases(bps))
    out = np.zeros((len(cases), 2), STATS)
    for i, (_, src, rec, w, h) in enumerate(cases):
        for only in (0, 1):
            st = stats_record()
            impl.gather(bps, only, src, rec, STRIDE, w, h, st)
            for k in STATS.names:
                out[i, only][k] = st[k]
            if only:
                out[i, only]["eoDiff"][0], out[i, only]["eoCount"][0] = 0, 0
    return out


def run_apply(impl, bps):
    """-> the filtered w x h areas of every (case, op) one after the other; nothing outside the area may change"""
    out = []
    offsets = apply_offsets(bps)
    for name, rec, left, upper, w, h in apply_cases(bps):
        for op in apply_ops():
            a, lf, up, off = rec.copy(), left.copy(), upper.copy(), offsets[op[2]].copy()
            impl.apply(bps, op, a, lf, up, w, h, off)
            rest = a.copy()
            rest[:h, :w] = rec[:h, :w]
            assert np.array_equal(rest, rec) and np.array_equal(lf, left) and np.array_equal(up, upper), (name, op)
            out.append(a[:h, :w].reshape(-1).copy())
    return np.concatenate(out)


def apply_slices(bps):
    """(name, op, input area, slice into run_apply's result) per (case, op)"""
    at = 0
    for name, rec, _, _, w, h in apply_cases(bps):
        for op in apply_ops():
            yield name, op, rec[:h, :w], slice(at, at + w * h)
            at += w * h


def run_dlf(impl, bps):
    """-> (luma windows [case][4][8], chroma windows [case][Cb, Cr][2][4]); samples outside the windows may not change"""
    lum, chrm = dlf_cases(bps)
    lo, co = np.zeros((len(lum), 4, 8), dtype_of(bps)), np.zeros((len(chrm), 2, 2, 4), dtype_of(bps))
    for i, c in enumerate(lum):
        b = c["block"].copy()
        impl.luma(bps, b, c["off"], c["vertical"], c["tc"], c["beta"])
        lo[i], rest = luma_window(b, c["vertical"])
        assert np.array_equal(rest, luma_window(c["block"], c["vertical"])[1]), i
    for i, c in enumerate(chrm):
        cb, cr = c["cb"].copy(), c["cr"].copy()
        impl.chroma(bps, cb, cr, c["off"], c["vertical"], c["cb_tc"], c["cr_tc"])
        for k, (got, src) in enumerate(((cb, c["cb"]), (cr, c["cr"]))):
            co[i, k], rest = chroma_window(got, c["vertical"])
            assert np.array_equal(rest, chroma_window(src, c["vertical"])[1]), (i, k)
    return lo, co
