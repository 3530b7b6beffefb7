"""Builders for the intra reference on its decisions, shared by tests/test_intra_ref_extremes_cpu.py, tests/test_gpu_intra_ref_extremes.py and
tests/test_gpu_intra_pu.py.  numpy and the CPU oracle only: no product library, no GPU.

A CASE is one intra unit at (0, 0) of an LCU together with every sample and mode type it can read: the 64 samples to its left (left and bottom-left), the 128
above (top and top-right), the corner, and one mode type (1 inter / 2 intra) per 4 luma samples of them.  picture() packs cases into one picture in which the
LCU of every case has host-encoded LCUs to its left, top-left, top and top-right: the device side is a list of SvtAmdLcuBorder records for
svt_amd_encdec_picture_put_borders plus one work record per case for svt_amd_encode_lcus, the oracle side the same samples written straight into rec[] and the
mode map of svt_oracle_encode_lcu.

The strong ("bilinear") filter of a 32x32 unit replaces [1 2 1] when abs(bl + tl - 2 mid) < thr on the left AND the top side, thr = 8 (8-bit) / 32 (10-bit),
with the flag set and a mode that reads the filtered reference.  The THRESHOLD GRID pins tl = mid = base on both sides and the far ends at base + d,
d in {-thr, -(thr-1), thr-1, thr}; the SIZE GATE moves the same pins onto a 16x16 unit; the MASKS make neighbour groups unavailable through constrained intra."""
import ctypes as C

import numpy as np

import svtlib as S

UNFILTERED_32 = (1, 10, 26)                 # intraLumaFilterTable at 32x32: DC, horizontal and vertical read the unfiltered reference
GRID_MODES = (0, 2, 18, 34, 9, 27, 1, 10, 26)
QP = 30


def thr_of(bps):
    return 8 if bps == 1 else 32


def grid_offsets(bps):
    t = thr_of(bps)
    return (-t, -(t - 1), t - 1, t)


def smoothing_classes(recs):
    """bool arrays over intra records (fields of tests/golden/intra_*.npz or of the dump): `available` - 32x32 with every neighbour group there; `fired` - the
    bilinear filter replaces [1 2 1] in what the prediction reads; A - fired with max(|dL|, |dT|) == thr - 1; B - |dL| == thr, |dT| < thr; C - |dT| == thr,
    |dL| < thr (B, C: one step outside, [1 2 1] stays)"""
    ci = np.asarray(recs["constrained_intra"]).astype(bool)
    there = lambda e, c: (e == 2) | ((e == 1) & ~c)
    flag = lambda k: np.asarray(recs[k]).astype(bool)
    avail = (np.asarray(recs["size"]) == 32) & ~flag("pic_left") & ~flag("pic_top") & ~flag("pic_right") & flag("bottom_left_ok") & flag("top_right_ok")
    avail &= there(recs["mode_left"][:, :16], ci[:, None]).all(axis=1) & there(recs["mode_top"][:, :16], ci[:, None]).all(axis=1) & there(recs["mode_tl"], ci)
    thr = np.where(np.asarray(recs["bytes_per_sample"]) == 1, 8, 32)
    left, top, tl = recs["left"][:, 0].astype(np.int64), recs["top"][:, 0].astype(np.int64), recs["tl"][:, 0].astype(np.int64)
    dl, dt = np.abs(left[:, 63] + tl - 2 * left[:, 31]), np.abs(tl + top[:, 63] - 2 * top[:, 31])
    base = avail & flag("strong_smoothing") & ~np.isin(recs["luma_mode"], UNFILTERED_32)
    fired = base & (dl < thr) & (dt < thr)
    return dict(available=avail, fired=fired, A=fired & (np.maximum(dl, dt) == thr - 1), B=base & (dl == thr) & (dt < thr), C=base & (dt == thr) & (dl < thr))


# ---- cases ----

def case(bps, size, mode, left, top, tl, strong=1, constrained=0, mode_left=None, mode_top=None, mode_tl=2, tag=None, seed=0):
    c = dict(bps=bps, size=size, mode=mode, strong=strong, constrained=constrained, left=np.asarray(left, np.int64), top=np.asarray(top, np.int64),
             tl=np.asarray(tl, np.int64), mode_left=np.full(16, 2, np.uint8) if mode_left is None else np.asarray(mode_left, np.uint8),
             mode_top=np.full(32, 2, np.uint8) if mode_top is None else np.asarray(mode_top, np.uint8), mode_tl=mode_tl, tag=tag, seed=seed)
    assert c["left"].shape == (3, 64) and c["top"].shape == (3, 128) and c["tl"].shape == (3,) and c["mode_left"].shape == (16,) and c["mode_top"].shape == (32,)
    assert 0 <= min(c["left"].min(), c["top"].min(), c["tl"].min()) and max(c["left"].max(), c["top"].max(), c["tl"].max()) <= (255 if bps == 1 else 1023)
    return c


def flat_neighbourhood(bps, n, d_left, d_top, base=100, k=6):
    """luma: tl = left[n-1] = top[n-1] = base, left[2n-1] = base + d_left, top[2n-1] = base + d_top, every other sample base +- k alternating (so [1 2 1] and the
    bilinear filter give different references); chroma: a sawtooth around mid-grey, never constant.  8-bit values, times 4 for 10-bit except the offsets."""
    sc = 1 if bps == 1 else 4
    i = np.arange(128)
    alt = (base + k * np.where(i & 1, -1, 1)) * sc
    left, top = np.zeros((3, 64), np.int64), np.zeros((3, 128), np.int64)
    left[0], top[0] = alt[:64], alt
    left[0][n - 1] = top[0][n - 1] = base * sc
    left[0][2 * n - 1], top[0][2 * n - 1] = base * sc + d_left, base * sc + d_top
    for p in (1, 2):
        left[p], top[p] = (128 + (i[:64] * (5 + 2 * p)) % 23 - 11) * sc, (128 + (i * (3 + 4 * p)) % 19 - 9) * sc
    return left, top, np.array([base * sc, (128 + 3) * sc, (128 - 5) * sc])


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def grid_cases(bps):
    """all 16 (dL, dT) pairs x GRID_MODES with the flag set, and the flag clear at the four pairs inside the threshold (the only ones where it matters)"""
    def make():
        t, out = thr_of(bps), []
        for dl in grid_offsets(bps):
            for dt in grid_offsets(bps):
                for strong in (1, 0):         # a flag-off case shares the seed (source, the other units' modes) of its twin
                    if strong or (abs(dl) < t and abs(dt) < t):
                        out += [case(bps, 32, m, *flat_neighbourhood(bps, 32, dl, dt), strong=strong, tag=("grid", dl, dt, m, strong), seed=dl * dl + 3 * abs(dt + 1) + m)
                                for m in GRID_MODES]
        return out
    return cached(("grid", bps), make)


def gate_cases(bps):
    """the size gate: the same pins on a 16x16 unit (left[15], left[31], top[15], top[31]), inside the threshold on both sides, flag set and clear"""
    def make():
        t, out = thr_of(bps), []
        for dl in (-(t - 1), t - 1):
            for dt in (-(t - 1), t - 1):
                for strong in (1, 0):
                    out += [case(bps, 16, m, *flat_neighbourhood(bps, 16, dl, dt), strong=strong, tag=("gate", dl, dt, m, strong), seed=dl * dl + 3 * abs(dt + 1) + m)
                            for m in GRID_MODES]
        return out
    return cached(("gate", bps), make)


MASKS = ("all_inter", "corner_only", "bottom_left_group_only", "last_top_right_group_only", "alternating", "all_but_corner", "left_inter_top_intra")


def named_mask(name, size):
    """(mode_left[16], mode_top[32], mode_tl) - 1 inter, 2 intra; what the unit of `size` at (0, 0) reads are the first size / 2 entries of each side"""
    g = size // 2                 # groups a side
    ml, mt, tl = np.ones(16, np.uint8), np.ones(32, np.uint8), 1
    if name == "corner_only":
        tl = 2
    elif name == "bottom_left_group_only":
        ml[g - 1] = 2
    elif name == "last_top_right_group_only":
        mt[g - 1] = 2
    elif name == "alternating":
        ml[0::2], mt[1::2], tl = 2, 2, 1
    elif name == "all_but_corner":
        ml[:], mt[:], tl = 2, 2, 1
    elif name == "left_inter_top_intra":
        mt[:], tl = 2, 2
    else:
        assert name == "all_inter"
    return ml, mt, tl


def group_samples(rng, bps):
    """one random value per neighbour group (4 luma / 2 chroma samples) and plane: a wrong substitution source shows up"""
    hi = 256 if bps == 1 else 1024
    left = np.stack([np.repeat(rng.integers(0, hi, 16), 4)] + [np.pad(np.repeat(rng.integers(0, hi, 16), 2), (0, 32)) for _ in range(2)])
    top = np.stack([np.repeat(rng.integers(0, hi, 32), 4)] + [np.pad(np.repeat(rng.integers(0, hi, 32), 2), (0, 64)) for _ in range(2)])
    return left, top, rng.integers(0, hi, 3)


def mask_cases(bps):
    """every named mask at unit sizes 32, 16 and 8 (left_inter_top_intra at 32 twice more on the flat grid borders, one step inside and on the threshold of the top
    side: the substituted left side is flat, the top side decides), 30 seeded random masks - each with constrained intra on and, as a control, off"""
    def make():
        rng, t, out = np.random.default_rng(77 + bps), thr_of(bps), []

        def both(size, mode, nb, ml, mt, mtl, tag):
            for ci in (1, 0):
                out.append(case(bps, size, mode, *nb, constrained=ci, mode_left=ml, mode_top=mt, mode_tl=mtl, tag=("mask",) + tag + (ci,), seed=len(out) // 2))
        for size in (32, 16, 8):
            for name in MASKS:
                both(size, 18 if "corner" in name else int(rng.choice([0, 18])), group_samples(rng, bps), *named_mask(name, size), (name, size))
        for dt in (t - 1, t):
            both(32, 34, flat_neighbourhood(bps, 32, t, dt), *named_mask("left_inter_top_intra", 32), ("left_inter_top_intra", 32, dt))
        for k in range(30):
            p = rng.choice([0.2, 0.5, 0.8])
            both(int(rng.choice([32, 16, 8])), int(rng.integers(0, 35)), group_samples(rng, bps), np.where(rng.random(16) < p, 1, 2), np.where(rng.random(32) < p, 1, 2),
                 int(rng.choice([1, 2])), ("random", k))
        return out
    return cached(("mask", bps), make)


def substituted(c):
    """numpy restatement of the substitution process (H.265 8.4.4.2.2) for the unit of the case: the same case with every group available and the samples of the
    unavailable groups replaced, or None when no group is available"""
    n, g = c["size"], c["size"] // 4
    inter = lambda e: c["constrained"] and e == 1
    ok = [not inter(e) for e in c["mode_left"][:2 * g][::-1]] + [not inter(c["mode_tl"])] + [not inter(e) for e in c["mode_top"][:2 * g]]      # scan order
    if not any(ok):
        return None
    left, top, tl = c["left"].copy(), c["top"].copy(), c["tl"].copy()
    for p in range(3):
        m, s = (2 * n, 4) if p == 0 else (n, 2)         # samples a side, samples a group
        b = np.concatenate([left[p][:m][::-1], tl[p:p + 1], top[p][:m]])
        oks = np.concatenate([np.repeat(ok[:2 * g], s), ok[2 * g:2 * g + 1], np.repeat(ok[2 * g + 1:], s)])
        first = int(np.flatnonzero(oks)[0])
        b[:first] = b[first]
        for i in range(first + 1, len(b)):
            if not oks[i]:
                b[i] = b[i - 1]
        left[p][:m], tl[p], top[p][:m] = b[:m][::-1], b[m], b[m + 1:]
    return dict(c, left=left, top=top, tl=tl, constrained=0, mode_left=np.full(16, 2, np.uint8), mode_top=np.full(32, 2, np.uint8), mode_tl=2)


def job_of(c, no_smoothing=0):
    """the SvtAmdIntraPuJob of the case's unit: left / top / tl given directly (svt_amd_intra_pu_batch, svt_oracle_intra_pu)"""
    from test_oracle_intra_golden import JOB
    j = np.zeros(1, JOB)
    j["size"], j["constrained_intra"], j["strong_smoothing"], j["luma_mode"], j["chroma_mode"] = c["size"], c["constrained"], c["strong"], c["mode"], 4
    j["bottom_left_ok"], j["top_right_ok"], j["no_smoothing"], j["mode_tl"] = 1, 1, no_smoothing, c["mode_tl"]
    j["mode_left"], j["mode_top"], j["left"], j["top"], j["tl"] = c["mode_left"], c["mode_top"][:16], c["left"], c["top"][:, :64], c["tl"]
    return j


def oracle_pu(oracle, bps, j):
    """svt_oracle_intra_pu of one job -> the three predicted blocks"""
    oracle.svt_oracle_intra_pu.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    oracle.svt_oracle_intra_pu.restype = None
    s, dt = int(j["size"][0]), np.uint8 if bps == 1 else np.uint16
    out = [np.zeros((s, s), dt), np.zeros((s // 2, s // 2), dt), np.zeros((s // 2, s // 2), dt)]
    oracle.svt_oracle_intra_pu(bps, j.ctypes.data, out[0].ctypes.data, s, out[1].ctypes.data, out[2].ctypes.data, s // 2)
    return out


# ---- pictures ----

def uniform_tree(size):
    """(x, y) of the size x size units of an LCU in Z order"""
    def rec(x, y, s):
        if s == size:
            return [(x, y)]
        h = s // 2
        return [u for dy, dx in ((0, 0), (0, h), (h, 0), (h, h)) for u in rec(x + dx, y + dy, h)]
    return rec(0, 0, 64)


def work_of(c, lcu_x, lcu_y):
    from test_gpu_encodepass import z_available
    wide = c["bps"] == 2
    rng = np.random.default_rng([c["seed"], c["size"], c["mode"]])
    wk = np.zeros(1, S.LCU_WORK16_DTYPE if wide else S.LCU_WORK_DTYPE)[0]
    wk["lcu_x"], wk["lcu_y"], wk["slice_type"], wk["strong_smoothing"], wk["constrained_intra"] = lcu_x, lcu_y, 2, c["strong"], c["constrained"]
    tree = uniform_tree(c["size"])
    wk["num_cus"] = len(tree)
    for i, (x, y) in enumerate(tree):
        cu = wk["cu"][i]
        cu["x"], cu["y"], cu["size"], cu["pred_mode"], cu["intra_luma_mode"] = x, y, c["size"], 2, c["mode"] if i == 0 else rng.integers(0, 35)
        cu["bottom_left_ok"], cu["top_right_ok"] = z_available(x, y, c["size"])
        cu["qp"], cu["chroma_qp"] = QP, 29          # the chroma QP table at 30
    sc, hi = (4, 1023) if wide else (1, 255)
    yy, xx = np.mgrid[0:64, 0:64]
    mid = int(c["tl"][0]) // sc
    src = [np.clip(mid + 18 * np.sin((xx + 3 * c["seed"]) / 9.0) * np.cos(yy / 7.0) + rng.normal(0, 4, (64, 64)), 0, 255)]
    src += [np.clip(128 + 12 * np.sin(xx[::2, ::2] / (5.0 + 2 * k)) + rng.normal(0, 3, (32, 32)), 0, 255) for k in range(2)]
    for nm, a in zip(("src_y", "src_cb", "src_cr"), src):
        a = a.astype(np.int64) * sc + (rng.integers(0, 4, a.shape) if wide else 0)
        wk[nm] = np.clip(a, 0, hi).reshape(-1)
    return wk


def picture(oracle, cases, cols=12):
    """cases (one sample depth) packed into one picture: case i is the LCU at column 2 (i % cols) + 1 of row 2 (i // cols) + 1; the rows and columns between hold
    the host-encoded LCUs.  -> dict(w, h, wide, borders, works, want): borders / works for the device, want = the oracle's results from the same samples written
    into rec[] and the mode map.  The two threads of the border kernel that write the bottom-right cell of an LCU get the same value."""
    bps = cases[0]["bps"]
    assert all(c["bps"] == bps for c in cases)
    wide = bps == 2
    rows = -(-len(cases) // cols)
    wl, hl = 2 * cols + 1, 2 * rows
    w, h = 64 * wl, 64 * hl
    sdt, hi = (np.uint16, 1024) if wide else (np.uint8, 256)
    fill = np.random.default_rng(1234)
    host = {}

    def border(lx, ly):
        if (lx, ly) not in host:
            a = np.zeros(1, S.LCU_BORDER16_DTYPE if wide else S.LCU_BORDER_DTYPE)
            b = a[0]
            b["lcu_x"], b["lcu_y"], b["mode_bottom"], b["mode_right"] = 64 * lx, 64 * ly, 2, 2
            for k in ("bottom_y", "right_y", "bottom_cb", "right_cb", "bottom_cr", "right_cr"):      # cells no case reads: anything but what the oracle sees there
                b[k] = fill.integers(0, hi, b[k].shape)
            host[(lx, ly)] = a
        return host[(lx, ly)][0]

    def corner(b, side):
        """the cell both arrays hold takes the value of the side a case reads"""
        other = "right" if side == "bottom" else "bottom"
        for p, e in (("y", 63), ("cb", 31), ("cr", 31)):
            b[other + "_" + p][e] = b[side + "_" + p][e]
        b["mode_" + other][15] = b["mode_" + side][15]
    pitches = (w + 32, w // 2 + 16, w // 2 + 16)
    rec = [np.full((hh, p), 0xA5A5 if wide else 0xA5, sdt) for hh, p in zip((h, h // 2, h // 2), pitches)]
    mp = np.full((h // 4, w // 4 + 3), 0xFF, np.uint8)
    works = np.zeros(len(cases), S.LCU_WORK16_DTYPE if wide else S.LCU_WORK_DTYPE)
    at = [(2 * (i % cols) + 1, 2 * (i // cols) + 1) for i in range(len(cases))]
    for i, (c, (lx, ly)) in enumerate(zip(cases, at)):
        x0, y0 = 64 * lx, 64 * ly
        works[i] = work_of(c, x0, y0)
        L, T, R = border(lx - 1, ly), border(lx, ly - 1), border(lx + 1, ly - 1)
        for p, nm in enumerate(("y", "cb", "cr")):
            s = 64 >> (p > 0)
            L["right_" + nm], T["bottom_" + nm], R["bottom_" + nm] = c["left"][p][:s], c["top"][p][:s], c["top"][p][s:2 * s]
            xp, yp = x0 >> (p > 0), y0 >> (p > 0)
            rec[p][yp:yp + s, xp - 1], rec[p][yp - 1, xp:xp + 2 * s] = c["left"][p][:s], c["top"][p][:2 * s]
        L["mode_right"], T["mode_bottom"], R["mode_bottom"] = c["mode_left"], c["mode_top"][:16], c["mode_top"][16:]
        mp[y0 // 4:y0 // 4 + 16, x0 // 4 - 1], mp[y0 // 4 - 1, x0 // 4:x0 // 4 + 32] = c["mode_left"], c["mode_top"]
        corner(L, "right"), corner(T, "bottom"), corner(R, "bottom")
    for c, (lx, ly) in zip(cases, at):       # the corners last: the top-left LCU of a case is the top-right LCU of the case before it in the row
        x0, y0 = 64 * lx, 64 * ly
        b = border(lx - 1, ly - 1)
        for p, (nm, e) in enumerate((("y", 63), ("cb", 31), ("cr", 31))):
            b["bottom_" + nm][e] = b["right_" + nm][e] = rec[p][(y0 >> (p > 0)) - 1, (x0 >> (p > 0)) - 1] = c["tl"][p]
        b["mode_bottom"][15] = b["mode_right"][15] = mp[y0 // 4 - 1, x0 // 4 - 1] = c["mode_tl"]
    borders = np.concatenate([host[k] for k in sorted(host)])
    for b in borders:
        assert b["bottom_y"][63] == b["right_y"][63] and b["bottom_cb"][31] == b["right_cb"][31] and b["bottom_cr"][31] == b["right_cr"][31]
        assert b["mode_bottom"][15] == b["mode_right"][15]
    fn = oracle.svt_oracle_encode_lcu16 if wide else oracle.svt_oracle_encode_lcu
    fn.restype = None
    fn.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    pb, rp = (C.c_uint32 * 3)(*pitches), (C.c_void_p * 3)(*[r.ctypes.data for r in rec])
    want = np.zeros(len(cases), S.LCU_RESULT16_DTYPE if wide else S.LCU_RESULT_DTYPE)
    for k in range(len(cases)):
        fn(rp, pb, mp.ctypes.data, mp.shape[1], w, h, works[k:k + 1].ctypes.data, want[k:k + 1].ctypes.data)
    return dict(w=w, h=h, wide=wide, borders=borders, works=works, want=want)


def first_unit(c, res):
    """the reconstruction of the case's unit out of its LCU's result record"""
    n = c["size"]
    return [res["rec_y"].reshape(64, 64)[:n, :n], res["rec_cb"].reshape(32, 32)[:n // 2, :n // 2], res["rec_cr"].reshape(32, 32)[:n // 2, :n // 2]]
