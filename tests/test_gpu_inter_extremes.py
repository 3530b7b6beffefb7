"""-m gpu: every implementation of the inter-prediction interpolation on tap-matched worst-case reference samples (tests/inter_extremes.py), bit-exact
against the oracle, which tests/test_oracle_mcp.py pins to the reference's C_DEFAULT tables on the same planes and tests/test_inter_extremes_cpu.py to the
ends of the 16-bit range: the three k_mcp instances and k_bipred_clip behind the batched and the leaf entries, the encode pass's core (8 and 10 bit) and
the mode decision's 8-bit dot-product cores."""
import ctypes as C

import numpy as np
import pytest

import inter_extremes as X
import svtlib as S
from test_gpu_mcp import BI_BLOCK, MCP_BLOCK
from test_oracle_inter_golden import JOB, RefPicture
from test_oracle_mcp import decl

pytestmark = pytest.mark.gpu
u32, vp, i32 = C.c_uint32, C.c_void_p, C.c_int32

ROWS, COLS, OY, OX = 96, 112, 16, 16        # one plane per (position, sign); blocks start at its phase (16, 16)
DS = 80                                      # stride of the sample destinations
RAW_SENTINEL, UNI_SENTINEL = 31111, 7        # no raw output reaches 31111 (the ends are +-25072)
LUMA_SIZES = {16: [(8, 8), (16, 8), (12, 16)], 32: [(32, 32), (24, 16)], 64: [(64, 64), (48, 24)], 0: [(8, 8), (12, 16), (24, 16), (64, 64)]}
CHROMA_SIZES = {16: [(4, 4), (8, 4), (12, 8)], 32: [(32, 32), (12, 8)], 64: [(32, 32), (8, 4)], 0: [(4, 4), (8, 4), (12, 8), (32, 32)]}
_cache = {}


def ref_buffer(bps, chroma):
    """the + and - planes of every position, one below the other -> (buffer, {(fx, fy, negative): sample offset of the plane's phase})"""
    key = ("ref", bps, chroma)
    if key not in _cache:
        planes, at = [], {}
        for fx, fy in X.positions(chroma):
            for negative in (False, True):
                at[(fx, fy, negative)] = (len(planes) * ROWS + OY) * COLS + OX
                planes.append(X.matched_plane(bps, chroma, fx, fy, negative, ROWS, COLS, OX, OY))
        _cache[key] = (np.ascontiguousarray(np.concatenate(planes)), at)
    return _cache[key]


def block_list(bps, chroma, raw, mbd):
    """{positions} x {+, -} x sizes -> (MCP_BLOCK array, keys, number of destination samples); every destination block is surrounded by samples no
    block owns"""
    _, at = ref_buffer(bps, chroma)
    sizes = (CHROMA_SIZES if chroma else LUMA_SIZES)[mbd]
    keys = [(fx, fy, negative, w, h) for fx, fy in X.positions(chroma) for negative in (False, True) for w, h in sizes]
    blocks = np.zeros(len(keys), MCP_BLOCK)
    cursor = 0
    for i, (fx, fy, negative, w, h) in enumerate(keys):
        blocks[i]["ref_off"], blocks[i]["w"], blocks[i]["h"], blocks[i]["fx"], blocks[i]["fy"] = at[(fx, fy, negative)], w, h, fx, fy
        if raw:
            blocks[i]["dst_off"] = cursor + 8
            cursor += w * h + 16
        else:
            blocks[i]["dst_off"] = (cursor + 1) * DS + 5
            cursor += h + 2
    return blocks, keys, cursor if raw else cursor * DS


def mcp_launch(product, gpu_ctx, oracle, bps, chroma, raw, mbd):
    """one launch of svt_amd_mcp_batch_sized (mbd 0: svt_amd_mcp_batch) over block_list() -> (device result, what the oracle wants, blocks, keys, the
    device tensor); cached, the bi-prediction tests reuse the raw buffers"""
    import torch
    key = ("mcp", bps, chroma, raw, mbd)
    if key in _cache:
        return _cache[key]
    decl(oracle)
    product.svt_amd_mcp_batch.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, u32, vp, u32, vp, u32]
    product.svt_amd_mcp_batch_sized.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, u32, vp, u32, vp, u32, u32]
    ref, _ = ref_buffer(bps, chroma)
    blocks, keys, nsamples = block_list(bps, chroma, raw, mbd)
    dt = np.int16 if raw else X.dtype_of(bps)
    sentinel = RAW_SENTINEL if raw else UNI_SENTINEL
    want = np.full(nsamples, sentinel, dt)
    owned = np.zeros(nsamples, bool)
    for b in blocks:
        w, h, off = int(b["w"]), int(b["h"]), int(b["dst_off"])
        oracle.svt_oracle_mcp(bps, chroma, raw, int(b["fx"]), int(b["fy"]), ref.ctypes.data + int(b["ref_off"]) * bps, COLS,
                              want.ctypes.data + off * want.itemsize, DS, w, h)
        for y in range(h):
            owned[off + y * (w if raw else DS):off + y * (w if raw else DS) + w] = True
    d_ref = torch.from_numpy(ref.view(np.uint8).reshape(-1).copy()).cuda()
    d_blocks = torch.from_numpy(blocks.view(np.uint8).copy()).cuda()
    d_dst = torch.from_numpy(np.full(nsamples, sentinel, dt).view(np.int16 if dt != np.uint8 else np.uint8)).cuda()
    torch.cuda.synchronize()                 # torch's copies run on torch's stream, the library on its own
    if mbd:
        rc = product.svt_amd_mcp_batch_sized(gpu_ctx, bps, chroma, raw, d_ref.data_ptr(), COLS, d_dst.data_ptr(), DS, d_blocks.data_ptr(), len(blocks), mbd)
    else:
        rc = product.svt_amd_mcp_batch(gpu_ctx, bps, chroma, raw, d_ref.data_ptr(), COLS, d_dst.data_ptr(), DS, d_blocks.data_ptr(), len(blocks))
    assert rc == 0, product.svt_amd_last_error()
    product.svt_amd_synchronize(gpu_ctx)
    got = d_dst.cpu().numpy().view(dt)
    _cache[key] = (got, want, owned, blocks, keys, d_dst)
    return _cache[key]


def first_bad(got, want, blocks, keys, raw):
    for b, k in zip(blocks, keys):
        w, h, off = int(b["w"]), int(b["h"]), int(b["dst_off"])
        for y in range(h):
            o = off + y * (w if raw else DS)
            if not np.array_equal(got[o:o + w], want[o:o + w]):
                x = int(np.nonzero(got[o:o + w] != want[o:o + w])[0][0])
                return "(fx, fy, negative, w, h) = %s at (%d, %d): got %d want %d" % (k, x, y, int(got[o + x]), int(want[o + x]))
    return None


# ---- a. k_mcp, all three instances ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mbd", [16, 32, 64, 0])
@pytest.mark.parametrize("raw", [0, 1])
@pytest.mark.parametrize("chroma", [0, 1])
@pytest.mark.parametrize("bps", [1, 2])
def test_mcp_batch_on_matched_planes(product, gpu_ctx, oracle, bps, chroma, raw, mbd):
    got, want, owned, blocks, keys, _ = mcp_launch(product, gpu_ctx, oracle, bps, chroma, raw, mbd)
    assert first_bad(got, want, blocks, keys, raw) is None, first_bad(got, want, blocks, keys, raw)
    assert np.all(got[~owned] == (RAW_SENTINEL if raw else UNI_SENTINEL)), "samples outside the blocks were written"
    assert np.array_equal(got, want)
    if raw and not chroma:                   # the launch did go to the ends (the oracle's values; the device equals them)
        assert int(want[owned].max()) > 24900 and int(want[owned].min()) < -24900
    if not raw:
        assert int(want[owned].min()) == 0 and int(want[owned].max()) == X.maxv_of(bps)


# ---- b. k_bipred_clip on the raw buffers of (a) --------------------------------------------------------------------------
@pytest.mark.parametrize("chroma", [0, 1])
@pytest.mark.parametrize("bps", [1, 2])
def test_bipred_clip_batch_on_the_raw_ends(product, gpu_ctx, oracle, bps, chroma):
    """list 0 / list 1 = + / +, - / -, + / - of every position and size of the 64-instance raw launch; the sums reach 2 x 25055 and 2 x -25072.
    8 bit: Offset5 on the luma buffers, ChromaOffset5 on the chroma ones; 10 bit has its own constant."""
    import torch
    got_raw, want_raw, _, blocks, keys, d_raw = mcp_launch(product, gpu_ctx, oracle, bps, chroma, 1, 64)
    assert np.array_equal(got_raw, want_raw)
    product.svt_amd_bipred_clip_batch.argtypes = [vp, C.c_int, vp, vp, vp, u32, i32, vp, u32]
    off_of = {k: int(b["dst_off"]) for b, k in zip(blocks, keys)}
    pairs = [(fx, fy, a, b, w, h) for fx, fy in X.positions(chroma) for a, b in ((False, False), (True, True), (False, True))
             for w, h in (CHROMA_SIZES if chroma else LUMA_SIZES)[64]]
    bi = np.zeros(len(pairs), BI_BLOCK)
    rows = 0
    for i, (fx, fy, a, b, w, h) in enumerate(pairs):
        bi[i]["l0_off"], bi[i]["l1_off"], bi[i]["w"], bi[i]["h"] = off_of[(fx, fy, a, w, h)], off_of[(fx, fy, b, w, h)], w, h
        bi[i]["dst_off"] = (rows + 1) * DS + 5
        rows += h + 2
    offset = 64 if chroma else 64 + 16384
    dt = X.dtype_of(bps)
    want = np.full(rows * DS, UNI_SENTINEL, dt)
    sums = []
    for k in bi:
        l0, l1 = want_raw[int(k["l0_off"]):], want_raw[int(k["l1_off"]):]
        oracle.svt_oracle_BiPredClipping(bps, int(k["w"]), int(k["h"]), l0.ctypes.data, l1.ctypes.data, want.ctypes.data + int(k["dst_off"]) * bps, DS, offset)
        n = int(k["w"]) * int(k["h"])
        s = l0[:n].astype(np.int32) + l1[:n]
        sums += [int(s.min()), int(s.max())]
    d_bi = torch.from_numpy(bi.view(np.uint8).copy()).cuda()
    d_dst = torch.from_numpy(np.full(rows * DS, UNI_SENTINEL, dt).view(np.int16 if bps == 2 else np.uint8)).cuda()
    torch.cuda.synchronize()
    rc = product.svt_amd_bipred_clip_batch(gpu_ctx, bps, d_raw.data_ptr(), d_raw.data_ptr(), d_dst.data_ptr(), DS, offset, d_bi.data_ptr(), len(bi))
    assert rc == 0, product.svt_amd_last_error()
    product.svt_amd_synchronize(gpu_ctx)
    got = d_dst.cpu().numpy().view(dt)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    if not chroma:
        assert max(sums) > 49800 and min(sums) < -49800          # beyond int16: the sum needs 17 bits
        assert int(want.min()) == 0 and int(want.max()) == X.maxv_of(bps)


# ---- c. the leaf entries (host pointers: the wrapper's extent arithmetic) -------------------------------------------------
LEAF_LUMA = [("LumaInterpolationCopy%s", "LumaInterpolationCopyOutRaw%s", 0, 0), ("LumaInterpolationFilterPosbNew%s", "LumaInterpolationFilterPosbOutRaw%s", 2, 0),
             ("LumaInterpolationFilterPoshNew%s", "LumaInterpolationFilterPoshOutRaw%s", 0, 2), ("LumaInterpolationFilterPosjNew%s", "LumaInterpolationFilterPosjOutRaw%s", 2, 2)]
LEAF_CHROMA = [("Copy", 0, 0), ("FilterOneD", 4, 0), ("FilterOneD", 0, 4), ("FilterTwoD", 4, 4)]


@pytest.mark.parametrize("bps", [1, 2])
def test_leaves_on_matched_planes(product, oracle, bps):
    decl(oracle)
    dt, sfx = X.dtype_of(bps), ("" if bps == 1 else "16bit")
    lists = {}
    for chroma, (w, h) in ((0, (24, 16)), (1, (12, 8))):
        for k in range(4):
            if chroma:
                kind, fx, fy = LEAF_CHROMA[k]
                uni, raw, extra = "ChromaInterpolation%s%s" % (kind, sfx), "ChromaInterpolation%sOutRaw%s" % (kind, sfx), (u32(fx), u32(fy))
            else:
                uni, raw, fx, fy = LEAF_LUMA[k]
                uni, raw, extra = uni % sfx, raw % sfx, ()
            for negative in (False, True):
                plane = X.matched_plane(bps, chroma, fx, fy, negative, ROWS, COLS, OX, OY)
                base = plane.ctypes.data + (OY * COLS + OX) * bps
                want, got = np.full((h, DS), 7, dt), np.full((h, DS), 7, dt)
                getattr(product, "svt_amd_" + uni)(vp(base), u32(COLS), vp(got.ctypes.data), u32(DS), u32(w), u32(h), None, *extra)
                oracle.svt_oracle_mcp(bps, chroma, 0, fx, fy, base, COLS, want.ctypes.data, DS, w, h)
                assert np.array_equal(want, got), (uni, negative)
                want, got = np.full(h * w, 7, np.int16), np.full(h * w, 7, np.int16)
                getattr(product, "svt_amd_" + raw)(vp(base), u32(COLS), vp(got.ctypes.data), u32(w), u32(h), None, *extra)
                oracle.svt_oracle_mcp(bps, chroma, 1, fx, fy, base, COLS, want.ctypes.data, 0, w, h)
                assert np.array_equal(want, got), (raw, negative)
                if k == 3:
                    lists[(chroma, negative)] = want
    assert int(lists[(0, False)].max()) > 24900 and int(lists[(0, True)].min()) < -24900
    # BiPredClipping[16bit] at the sums of (b)
    for chroma, (w, h) in ((0, (24, 16)), (1, (12, 8))):
        for a, b in ((False, False), (True, True), (False, True)):
            l0, l1 = lists[(chroma, a)].copy(), lists[(chroma, b)].copy()
            want, got = np.full((h, DS), 7, dt), np.full((h, DS), 7, dt)
            offset = 64 if chroma else 64 + 16384
            if bps == 1:
                product.svt_amd_BiPredClipping(u32(w), u32(h), vp(l0.ctypes.data), vp(l1.ctypes.data), vp(got.ctypes.data), u32(DS), i32(offset))
            else:
                product.svt_amd_BiPredClipping16bit(u32(w), u32(h), vp(l0.ctypes.data), vp(l1.ctypes.data), vp(got.ctypes.data), u32(DS))
            oracle.svt_oracle_BiPredClipping(bps, w, h, l0.ctypes.data, l1.ctypes.data, want.ctypes.data, DS, offset)
            assert np.array_equal(want, got), (chroma, a, b)


# ---- d. the prediction-unit entries ---------------------------------------------------------------------------------------
PW, PH, POX, POY, GUARD = 128, 64, 68, 68, 96    # the reference's padding (64 + 4); guard rows: a clamped far vector's taps reach beyond the padding
SY, SC = PW + 2 * POX, (PW + 2 * POX) // 2


def pu_planes(kind, negative):
    """[y, cb, cr] of one padded reference picture: luma matched for (2,2), chroma for (4,4), phase (0,0) at the picture origin.
    kind: 1 / 2 bytes per sample, or "msb" (10 bit, matched upper 8 bits, random lower two)"""
    ry, rc = PH + 2 * POY + 2 * GUARD, (PH + 2 * POY) // 2 + 2 * GUARD
    if kind == "msb":
        return [X.matched_plane_msb(0, 2, 2, negative, ry, SY, POX, POY + GUARD, 0), X.matched_plane_msb(1, 4, 4, negative, rc, SC, POX // 2, POY // 2 + GUARD, 1),
                X.matched_plane_msb(1, 4, 4, negative, rc, SC, POX // 2, POY // 2 + GUARD, 2)]
    return [X.matched_plane(kind, 0, 2, 2, negative, ry, SY, POX, POY + GUARD), X.matched_plane(kind, 1, 4, 4, negative, rc, SC, POX // 2, POY // 2 + GUARD),
            X.matched_plane(kind, 1, 4, 4, negative, rc, SC, POX // 2, POY // 2 + GUARD)]


def pu_refs(planes, device):
    """two RefPicture (+ what keeps their memory alive) over host arrays or device copies of them"""
    import torch
    out, keep = [], []
    for pl in planes:
        bps = pl[0].itemsize
        if device:
            t = [torch.from_numpy(a.view(np.int16) if bps == 2 else a).cuda() for a in pl]
            ptrs = [x.data_ptr() for x in t]
            keep.append(t)
        else:
            ptrs = [a.ctypes.data for a in pl]
        skip = [GUARD * SY * bps, GUARD * SC * bps, GUARD * SC * bps]
        r = RefPicture()
        r.d_y, r.d_cb, r.d_cr = [p + k for p, k in zip(ptrs, skip)]
        r.strideY, r.strideC, r.originX, r.originY, r.width, r.height = SY, SC, POX, POY, PW, PH
        out.append(r)
    return out, keep


def pu_jobs():
    """every unit size with its 2NxN halves, the three prediction directions; vectors: all 16 fractions at an integer part that keeps the unit on the
    planes' phase (multiples of 8 samples), vectors at every other phase (among them 4 mod 32 quarter samples: the matched chroma half position), and a
    quarter far outside the picture"""
    rng = np.random.default_rng(41)
    jobs = []
    shapes = [(8, 8), (16, 16), (16, 8), (32, 32), (32, 16), (64, 64), (64, 32)]
    k = a = 0
    for w, h in shapes:
        for rep in range(48):
            j = np.zeros(1, JOB)[0]
            j["pu_w"], j["pu_h"], j["pred_dir"] = w, h, k % 3
            j["pu_x"], j["pu_y"] = 8 * int(rng.integers(0, (PW - w) // 8 + 1)), 8 * int(rng.integers(0, (PH - h) // 8 + 1))
            mv = np.zeros((2, 2), np.int64)
            for l in range(2):
                if rep % 4 == 3:                                # far outside: the clamp
                    mv[l] = rng.integers(-1200, 1200, 2)
                elif rep % 4 == 2:                              # every other phase
                    mv[l] = 32 * rng.integers(-2, 3, 2) + 4 * rng.integers(0, 8, 2) + rng.integers(0, 4, 2)
                    if rep % 8 == 2:
                        mv[l] = 32 * rng.integers(-2, 3, 2) + 4
                else:                                           # phase-aligned integer part, every fraction in turn
                    f = (a + 5 * l) % 16
                    mv[l] = 32 * rng.integers(-2, 3, 2) + np.array([f & 3, f >> 2])
            a += rep % 4 < 2
            j["mv"] = mv
            jobs.append(j)
            k += 1
    return np.array(jobs, JOB)


def run_pu(product, gpu_ctx, fn, jobs, refs, hbd):
    import torch
    n = len(jobs)
    jobs = jobs.copy()
    jobs["dst_off_y"], jobs["dst_off_c"] = np.arange(n) * 4096, np.arange(n) * 1024
    tdt = torch.int16 if hbd else torch.uint8
    d = [torch.zeros(n * 4096, dtype=tdt, device="cuda"), torch.zeros(n * 1024, dtype=tdt, device="cuda"), torch.zeros(n * 1024, dtype=tdt, device="cuda")]
    fn.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, vp, u32]
    torch.cuda.synchronize()
    for w in sorted(set(int(v) for v in jobs["pu_w"])):          # destination strides equal the unit width: one launch per width
        sub = np.ascontiguousarray(jobs[jobs["pu_w"] == w])
        rc = fn(gpu_ctx, sub.ctypes.data, len(sub), C.addressof(refs[0]), C.addressof(refs[1]), d[0].data_ptr(), w, d[1].data_ptr(), d[2].data_ptr(), w // 2)
        assert rc == 0, product.svt_amd_last_error()
    host = [a.cpu().numpy().view(np.uint16 if hbd else np.uint8) for a in d]
    out = []
    for k in range(n):
        w, h = int(jobs["pu_w"][k]), int(jobs["pu_h"][k])
        out.append((host[0][k * 4096:k * 4096 + w * h].reshape(h, w), host[1][k * 1024:k * 1024 + w * h // 4].reshape(h // 2, w // 2),
                    host[2][k * 1024:k * 1024 + w * h // 4].reshape(h // 2, w // 2)))
    return out


def oracle_pu(oracle, jobs, refs, hbd):
    ofn = oracle.svt_oracle_inter_pu16bit if hbd else oracle.svt_oracle_inter_pu
    ofn.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32]
    ofn.restype = None
    dt = np.uint16 if hbd else np.uint8
    out = []
    for k in range(len(jobs)):
        w, h = int(jobs["pu_w"][k]), int(jobs["pu_h"][k])
        want = [np.zeros((h, w), dt), np.zeros((h // 2, w // 2), dt), np.zeros((h // 2, w // 2), dt)]
        ofn(jobs[k:k + 1].ctypes.data, C.addressof(refs[0]), C.addressof(refs[1]), want[0].ctypes.data, w, want[1].ctypes.data, want[2].ctypes.data, w // 2)
        out.append(want)
    return out


def compare_pu(got, want, jobs, what):
    for k in range(len(jobs)):
        for p in range(3):
            assert np.array_equal(got[k][p], want[k][p]), (what, k, p, jobs[k])


def check_job_cover(jobs, want, maxv):
    assert {(int(a), int(b)) for a, b in zip(jobs["pu_w"], jobs["pu_h"])} == {(8, 8), (16, 16), (16, 8), (32, 32), (32, 16), (64, 64), (64, 32)}
    assert set(jobs["pred_dir"].tolist()) == {0, 1, 2}
    for l in range(2):                                                              # every fraction at a phase-aligned integer part, in both lists
        aligned = {(int(j["mv"][l][0]) & 3, int(j["mv"][l][1]) & 3) for j in jobs
                   if j["pred_dir"] in (l, 2) and (int(j["mv"][l][0]) >> 2) % 8 == 0 and (int(j["mv"][l][1]) >> 2) % 8 == 0}
        assert len(aligned) == 16, (l, sorted(aligned))
    clamped = 0
    for j in jobs:                                                                  # the position clamp of the entry, restated
        for l in range(2):
            px, py = ((int(j["pu_x"]) + POX) << 2) + int(j["mv"][l][0]), ((int(j["pu_y"]) + POY) << 2) + int(j["mv"][l][1])
            if j["pred_dir"] in (l, 2) and not ((POX - 71) << 2 <= px <= (PW + POX + 7) << 2 and (POY - 71) << 2 <= py <= (PH + POY + 7) << 2):
                clamped += 1
                break
    assert clamped >= len(jobs) // 8
    luma = np.concatenate([w[0].reshape(-1) for w in want])
    assert int(luma.min()) == 0 and int(luma.max()) == maxv


@pytest.mark.parametrize("hbd", [False, True])
def test_inter_pu_batch_on_matched_pictures(product, gpu_ctx, oracle, hbd):
    planes = [pu_planes(2 if hbd else 1, False), pu_planes(2 if hbd else 1, True)]      # picture 0 is +, picture 1 is -
    jobs = pu_jobs()
    host, _ = pu_refs(planes, False)
    dev, keep = pu_refs(planes, True)
    want = oracle_pu(oracle, jobs, host, hbd)
    check_job_cover(jobs, want, 1023 if hbd else 255)
    got = run_pu(product, gpu_ctx, product.svt_amd_inter_pu_batch16bit if hbd else product.svt_amd_inter_pu_batch, jobs, dev, hbd)
    compare_pu(got, want, jobs, "16bit" if hbd else "8bit")
    del keep


def test_inter_pu_batch_msb_on_matched_pictures(product, gpu_ctx, oracle):
    """the 8-MSB prediction of a 10-bit encode's mode decision: 16-bit planes whose upper 8 bits are matched and whose lower two are random, against the
    oracle on plane >> 2 (truncation: 255.75 stays 255) and against the 8-bit entry on the same narrowed planes"""
    planes = [pu_planes("msb", False), pu_planes("msb", True)]
    assert all(int((a & 3).max()) == 3 and int(a.max()) == 1023 for pl in planes for a in pl)
    narrow = [[(a >> 2).astype(np.uint8) for a in pl] for pl in planes]
    jobs = pu_jobs()
    host, _ = pu_refs(narrow, False)
    want = oracle_pu(oracle, jobs, host, False)
    check_job_cover(jobs, want, 255)
    dev, keep = pu_refs(planes, True)
    got = run_pu(product, gpu_ctx, product.svt_amd_inter_pu_batch_msb, jobs, dev, False)
    compare_pu(got, want, jobs, "msb vs oracle")
    dev8, keep8 = pu_refs(narrow, True)
    got8 = run_pu(product, gpu_ctx, product.svt_amd_inter_pu_batch, jobs, dev8, False)
    compare_pu(got, got8, jobs, "msb vs the 8-bit entry")
    del keep, keep8


# ---- e. the encode pass's core ----------------------------------------------------------------------------------------------
EP_W, EP_H, EP_QP, EP_SEED = 200, 136, 30, 6      # the seed: chosen on the CPU for the unit counts asserted below (23 bi, 43 uni, 37 on the phase)


def fractional_units(works):
    """(bi-predicted, uni-predicted, on the planes' phase) inter units whose used vectors have a fractional part in both components"""
    bi = uni = on_phase = 0
    for wk in works:
        for cu in wk["cu"][:int(wk["num_cus"])]:
            if int(cu["pred_mode"]) != 1:
                continue
            used = [0, 1] if int(cu["inter_dir"]) == 2 else [int(cu["inter_dir"])]
            if all(int(cu["mv"][l][0]) & 3 and int(cu["mv"][l][1]) & 3 for l in used):
                bi, uni = bi + (len(used) == 2), uni + (len(used) == 1)
                on_phase += all(int(cu["mv"][l][c]) % 32 == 2 for l in used for c in (0, 1))
    return bi, uni, on_phase


@pytest.mark.parametrize("wide", [False, True])
def test_encode_picture_predicts_from_matched_reference_pictures(product, oracle, wide):
    """ep_inter_predict_core<T>, 8 and 10 bit: a B picture of random units whose two reference pictures are the matched planes (+ in list 0, - in list 1);
    every third inter unit's vectors are half-sample ones on the planes' phase, so its prediction runs through the ends of both passes"""
    from test_gpu_encodepass import random_inter_picture, set_inter_random, sig_picture
    from test_oracle_encodepass_golden import compare_lcu
    lib = product
    sig_picture(lib)
    works, want, refs_geom, cost = random_inter_picture(oracle, EP_W, EP_H, EP_QP, EP_SEED, matched=True, wide=wide)
    bi, uni, on_phase = fractional_units(works)
    assert bi >= 20 and uni >= 20 and on_phase >= 20, (bi, uni, on_phase)
    ctx, pic = C.c_void_p(), C.c_void_p()
    assert lib.svt_amd_context_create(0, EP_W, EP_H, 1, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    try:
        assert lib.svt_amd_encdec_picture_create(ctx, EP_W, EP_H, 2 if wide else 1, C.byref(pic)) == 0, lib.svt_amd_last_error()
        keep = set_inter_random(lib, ctx, pic, refs_geom, cost)
        got = np.zeros(len(works), S.LCU_RESULT16_DTYPE if wide else S.LCU_RESULT_DTYPE)
        fn = lib.svt_amd_encode_picture16 if wide else lib.svt_amd_encode_picture
        assert fn(ctx, pic, works.ctypes.data, got.ctypes.data) == 0, lib.svt_amd_last_error()
        for k in range(len(works)):
            compare_lcu(works[k], want[k], got[k], EP_W, EP_H, ("matched B picture", wide, k))
        del keep
        lib.svt_amd_encdec_picture_destroy(ctx, pic)
    finally:
        lib.svt_amd_context_destroy(ctx)


# ---- f. the mode decision's dot-product cores --------------------------------------------------------------------------------
@pytest.mark.parametrize("butterflies", [0, 1])
@pytest.mark.parametrize("name,k,signs", X.MD_CASES)
def test_md_decides_on_matched_reference_pictures(product, oracle, name, k, signs, butterflies):
    """md_predict_tile / ep_mc8_tile (on the staged window where it lies and on the scratch copy md_window_from_plane makes of any other): a recorded P / B picture's source, ME records and controls with both
    reference pictures replaced by matched planes (the signs of the two lists' planes: inter_extremes.MD_CASES); every tested leaf's decisions AND costs against the oracle's on the same inputs, so one wrong prediction
    sample in a tested leaf shows.  Once more with every forward transform on the register butterflies: the full-loop residuals are the largest there.
    Nothing pins the oracle's mode decision to the reference on substituted inputs: its interpolation is pinned at these ends by tests/test_oracle_mcp.py,
    everything else by the recorded fixtures (tests/test_oracle_md_golden.py).  That inter candidates do win here: tests/test_inter_extremes_cpu.py."""
    import os
    from test_gpu_md import md_encode_inter, sig
    from test_oracle_md_golden import compare_md, oracle_md_picture
    lib = product
    sig(lib)
    lib.svt_amd_debug_md_force_butterflies.restype = C.c_int
    lib.svt_amd_debug_md_force_butterflies.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    g = np.load(os.path.join(S.GOLDEN_DIR, "md_%s.npz" % name))
    planes = X.md_matched_planes(g, k, signs)
    want, _ = oracle_md_picture(oracle, g, k, planes)
    frac, bi = X.md_inter_winners(want)
    assert frac >= 10, (frac, bi)
    w, h = int(g["pic"][0]["width"]), int(g["pic"][0]["height"])
    ctx, pic = C.c_void_p(), C.c_void_p()
    assert lib.svt_amd_context_create(0, w, (h + 7) & ~7, 2, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    try:
        assert lib.svt_amd_encdec_picture_create(ctx, w, h, 1, C.byref(pic)) == 0, lib.svt_amd_last_error()
        assert lib.svt_amd_debug_md_force_butterflies(ctx, pic, butterflies) == 0, lib.svt_amd_last_error()
        out, _, _ = md_encode_inter(lib, ctx, pic, g, k, planes=planes)
        compare_md(out, want, "%s picture %d on matched planes %s, butterflies forced: %d" % (name, k, signs, butterflies))
        lib.svt_amd_encdec_picture_destroy(ctx, pic)
    finally:
        lib.svt_amd_context_destroy(ctx)
