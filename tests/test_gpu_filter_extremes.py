"""-m gpu: the in-loop filters where the other GPU tests do not go - SAO statistics whose differences leave the signed 8-bit range, waves that fall into one
band or straddle two, LCU sizes 8 .. 128 (128: the path that reads global memory directly); SAO offsets of +-7 / +-31 on samples at the ends of the range and
band positions 29 .. 31; deblocking with tc / beta of 0, 1 and the table maxima on planes at 0 and at the maximum, the 10-bit chroma edge batch, QP maps of 0
and 51 with the offsets at their ends; and the chain statistics -> decision -> application on saturated pictures without a download in between.  Every
comparison is bit-exact: the leaves against what the reference computed on the same seeded inputs (tests/golden/filterx_*.npz), the picture-level entries
against the CPU oracle, which tests/test_filter_extremes_cpu.py pins to the same records.  Every guard is computed from the inputs, the records or the
oracle's result, never from the device's."""
import ctypes as C

import numpy as np
import pytest

import filter_extremes as X
from test_filter_extremes_cpu import chain_params, fixture, oracle_chain, same_apply, same_dlf, same_stats
from test_gpu_dlf_picture import gpu_dlf
from test_gpu_loopfilter import STATS, libs  # noqa: F401  (the fixture that declares the batched entries)
from test_oracle_dlf_golden import oracle_dlf, oracle_sao
from test_oracle_saodec_golden import LCU

pytestmark = pytest.mark.gpu
vp, u32 = C.c_void_p, C.c_uint32
BPS = [1, 2]


def leaves(product):
    return X.Leaves(product, "svt_amd_")


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def from_dev(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


# ---- leaves against the reference's records --------------------------------------------------------------------------
@pytest.mark.parametrize("bps", BPS)
def test_gather_leaves_match_reference_records(product, bps):
    same_stats(X.run_gather(leaves(product), bps), fixture("gather")["g%d" % bps], bps)


@pytest.mark.parametrize("bps", BPS)
def test_apply_leaves_match_reference_records(product, bps):
    same_apply(X.run_apply(leaves(product), bps), fixture("apply")["a%d" % bps], bps)


@pytest.mark.parametrize("bps", BPS)
def test_dlf_leaves_match_reference_records(product, bps):
    same_dlf(X.run_dlf(leaves(product), bps), (fixture("dlf")["l%d" % bps], fixture("dlf")["c%d" % bps]), bps)


# ---- statistics of whole pictures, every LCU size --------------------------------------------------------------------
@pytest.mark.parametrize("bps", BPS)
@pytest.mark.parametrize("lcu_size,w,h,stride", [(64, 200, 136, 208), (32, 200, 136, 208), (16, 200, 136, 200), (8, 200, 136, 203), (128, 320, 192, 320)])
def test_sao_gather_picture_lcu_sizes(libs, gpu_ctx, bps, lcu_size, w, h, stride):
    """200x136: the right column is 8 wide and the bottom row 8 high at every LCU size; 320x192 at LCU size 128 has full LCUs, a right column 64 wide, a bottom
    row 64 high (both read from global memory: one side exceeds the 64x64 staging tile) and a 64x64 corner that is staged.  The cells of the pictures cycle
    through the patterns of the leaf cases.  The output is prefilled with 0xA5 so that a record nobody wrote cannot pass."""
    import torch
    product, oracle = libs
    impl = X.Oracle(oracle)
    assert (min(lcu_size, w) - 2) * (min(lcu_size, h) - 2) <= 126 * 126 <= 65535      # no 16-bit count can wrap
    src, rec = X.gather_picture(bps, w, h, stride, lcu_size)
    ds, dr = to_dev(src), to_dev(rec)
    lw, lh = -(-w // lcu_size), -(-h // lcu_size)
    shapes = set()
    for only in (0, 1):
        out = torch.full((lw * lh * STATS.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()  # torch fills/copies run on torch's stream, the library on its own
        rc = product.svt_amd_sao_gather_picture(gpu_ctx, bps, ds.data_ptr(), stride, dr.data_ptr(), stride, w, h, lcu_size, only, out.data_ptr())
        assert rc == 0, product.svt_amd_last_error()
        product.svt_amd_synchronize(gpu_ctx)
        got = out.cpu().numpy().view(STATS)
        for l in range(lw * lh):
            x0, y0 = (l % lw) * lcu_size, (l // lw) * lcu_size
            o = (y0 * stride + x0) * bps
            st = X.stats_record()
            impl.gather(bps, only, src, rec, stride, min(lcu_size, w - x0), min(lcu_size, h - y0), st, o, o)
            shapes.add((min(lcu_size, w - x0), min(lcu_size, h - y0)))
            if not only:
                assert np.array_equal(got[l]["boDiff"], st["boDiff"]) and np.array_equal(got[l]["boCount"], st["boCount"]), (l, only)
            k0 = 1 if only else 0
            assert np.array_equal(got[l]["eoDiff"][k0:], st["eoDiff"][k0:]) and np.array_equal(got[l]["eoCount"][k0:], st["eoCount"][k0:]), (l, only)
    assert len(shapes) == (4 if lcu_size > 8 else 1)     # full, right-partial, bottom-partial and corner LCUs (at size 8 the 8-wide column is a full LCU)


# ---- SAO application of whole pictures -------------------------------------------------------------------------------
def gpu_sao(product, gpu_ctx, src, bps, width, height, lcus, pad_y, pad_c):
    import torch
    dsrc, ddst, strides = [], [], []
    for k, p in enumerate(src):
        buf = np.zeros((p.shape[0], p.shape[1] + (pad_c if k else pad_y)), p.dtype)
        buf[:, :p.shape[1]] = p
        dsrc.append(to_dev(buf))
        ddst.append(torch.zeros_like(dsrc[-1]))
        strides.append(buf.shape[1])
    dl = to_dev(lcus)
    product.svt_amd_sao_apply_picture.argtypes = [vp, C.c_int, vp, vp, u32, u32, u32, u32, vp, C.c_int, C.c_int]
    ps, pd = (vp * 3)(*[t.data_ptr() for t in dsrc]), (vp * 3)(*[t.data_ptr() for t in ddst])
    torch.cuda.synchronize()
    rc = product.svt_amd_sao_apply_picture(gpu_ctx, bps, ps, pd, strides[0], strides[1], width, height, dl.data_ptr(), 1, 1)
    assert rc == 0, product.svt_amd_last_error()
    product.svt_amd_synchronize(gpu_ctx)
    return [from_dev(t, p.dtype, (p.shape[0], s))[:, :p.shape[1]] for t, p, s in zip(ddst, src, strides)]


@pytest.mark.parametrize("bps", BPS)
@pytest.mark.parametrize("w,h,pad_c", [(72, 40, 4), (200, 136, 4)])
def test_sao_apply_picture_at_the_ends(product, gpu_ctx, oracle, bps, w, h, pad_c):
    """saturated planes, offsets up to +-7 / +-31, band positions up to 31; luma stride w with chroma stride w / 2 + 4 (both multiples of 8: the kernel's
    8-samples-a-store form) and both strides + 3 (the sample-by-sample form)"""
    planes, lcus = X.sao_apply_picture(bps, w, h)
    maxv, m = X.maxv_of(bps), X.apply_m(bps)
    want = oracle_sao(oracle, planes, bps, w, h, lcus, 1, 1)
    for c in range(3):
        assert (((want[c] == 0) | (want[c] == maxv)) & (want[c] != planes[c])).any(), c
    on5 = {int(lcus["band"][i, c]) for i in range(len(lcus)) for c in range(3) if lcus["type"][i, 0 if c == 0 else 1] == 5}
    assert {29, 30, 31} <= on5 and set(lcus["type"].reshape(-1).tolist()) >= ({1, 5} if len(lcus) < 6 else set(range(6)))
    assert (np.abs(lcus["offset"]) == m).mean() > 1 / 3 and np.abs(lcus["offset"]).max() == m
    assert (w % 8, (w // 2 + pad_c) % 8) == (0, 0)
    for pad_y, pc in ((0, pad_c), (3, 3)):
        got = gpu_sao(product, gpu_ctx, planes, bps, w, h, lcus, pad_y, pc)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), (c, pad_y, np.argwhere(got[c] != want[c])[:5].tolist())


# ---- deblocking: the batched edge lists ------------------------------------------------------------------------------
LUMA_EDGE = np.dtype([("offset", "<i4"), ("tc", "<i2"), ("beta", "<i2"), ("v", "u1"), ("pad", "u1", 3)])
CHROMA_EDGE = np.dtype([("offset", "<i4"), ("cb", "u1"), ("cr", "u1"), ("v", "u1"), ("pad", "u1")])
BW, BH = 128, 64


@pytest.mark.parametrize("bps", BPS)
def test_dlf_luma_batched_ends(libs, gpu_ctx, bps):
    """all vertical, then all horizontal edges of a 128x64 plane of saturated steps; (tc, beta) cycle through {0, 1, 24} x {0, 1, 64} (<< 2 for 10 bit)"""
    import torch
    product, oracle = libs
    sh = X.dlf_shift(bps)
    plane = X.step_plane(bps, BW, BH, 3)
    want, dev = plane.copy(), to_dev(plane)
    for vertical in (1, 0):
        at = [(y, x) for y in range(0, BH, 4) for x in range(8, BW, 8)] if vertical else [(y, x) for y in range(8, BH, 8) for x in range(0, BW, 4)]
        arr = np.zeros(len(at), LUMA_EDGE)
        k = np.arange(len(at))
        arr["offset"], arr["v"] = [y * BW + x for y, x in at], vertical
        arr["tc"], arr["beta"] = np.array([0, 1, 24])[k % 3] << sh, np.array([0, 1, 64])[(k // 3 + k // 9) % 3] << sh
        assert {(int(e["tc"]), int(e["beta"])) for e in arr} == {(t << sh, b << sh) for t in (0, 1, 24) for b in (0, 1, 64)}
        d_edges = to_dev(arr)
        torch.cuda.synchronize()
        rc = product.svt_amd_dlf_luma_edges_batch(gpu_ctx, dev.data_ptr(), BW, bps, d_edges.data_ptr(), len(arr))
        assert rc == 0, product.svt_amd_last_error()
        product.svt_amd_synchronize(gpu_ctx)
        for e in arr:
            oracle.svt_oracle_Luma4SampleEdgeDLFCore(bps, X.P(want, int(e["offset"]) * bps), BW, vertical, int(e["tc"]), int(e["beta"]))
    assert not np.array_equal(want, plane) and want.min() == 0 and want.max() == X.maxv_of(bps)
    got = from_dev(dev, plane.dtype, plane.shape)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


@pytest.mark.parametrize("bps", BPS)
def test_dlf_chroma_batched_ends(libs, gpu_ctx, bps):
    """the chroma edge batch with 1 and 2 bytes a sample (the second is the instantiation no other test launches); tc cycles through {0, 1, 24} (8 bit) /
    {0, 4, 96} (10 bit), Cb and Cr out of step"""
    import torch
    product, oracle = libs
    sh = X.dlf_shift(bps)
    cb, cr = X.step_plane(bps, BW, BH, 4), X.step_plane(bps, BW, BH, 5)
    wb, wr, db, dr = cb.copy(), cr.copy(), to_dev(cb), to_dev(cr)
    for vertical in (1, 0):
        at = [(y, x) for y in range(0, BH, 2) for x in range(8, BW, 8)] if vertical else [(y, x) for y in range(8, BH, 8) for x in range(0, BW, 2)]
        arr = np.zeros(len(at), CHROMA_EDGE)
        k = np.arange(len(at))
        arr["offset"], arr["v"] = [y * BW + x for y, x in at], vertical
        arr["cb"], arr["cr"] = np.array([0, 1, 24])[k % 3] << sh, np.array([0, 1, 24])[(k // 3 + k + 1) % 3] << sh
        assert {int(v) for v in arr["cb"]} == {int(v) for v in arr["cr"]} == {0, 1 << sh, 24 << sh}
        d_edges = to_dev(arr)
        torch.cuda.synchronize()
        rc = product.svt_amd_dlf_chroma_edges_batch(gpu_ctx, db.data_ptr(), dr.data_ptr(), BW, bps, d_edges.data_ptr(), len(arr))
        assert rc == 0, product.svt_amd_last_error()
        product.svt_amd_synchronize(gpu_ctx)
        for e in arr:
            o = int(e["offset"]) * bps
            oracle.svt_oracle_Chroma2SampleEdgeDLFCore(bps, X.P(wb, o), X.P(wr, o), BW, vertical, int(e["cb"]), int(e["cr"]))
    assert not np.array_equal(wb, cb) and not np.array_equal(wr, cr)
    if bps == 2:
        assert max(wb.max(), wr.max()) > 255 and ((wb != cb) & (wb > 255)).any()    # a filter that clipped to 255 would differ
    gb, gr = from_dev(db, cb.dtype, cb.shape), from_dev(dr, cr.dtype, cr.shape)
    assert np.array_equal(gb, wb) and np.array_equal(gr, wr), (np.argwhere(gb != wb)[:5].tolist(), np.argwhere(gr != wr)[:5].tolist())


# ---- deblocking of whole pictures at the ends of the tables ------------------------------------------------------------
@pytest.mark.parametrize("bps", BPS)
@pytest.mark.parametrize("w,h", [(64, 64), (72, 40)])
@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_dlf_picture_table_ends(product, gpu_ctx, oracle, bps, w, h, which):
    """Strength 2 on every edge of blocky planes around 0, mid-range and the maximum.
    a  QP 51 everywhere, tc / beta offsets +6, Cb / Cr QP offsets +12 / -12: the last entries of the tc and beta tables, chroma QP 63 > 57
    b  QP 0 everywhere, offsets -6, Cb / Cr QP offsets -12 / +12: tc = beta = 0, so luma and Cr stay untouched - but Cb is filtered: the reference's
       convertToChromaQp result is stored into an EB_U8 (Codec/EbDeblockingFilter.c), so chroma QP -12 becomes 244 and indexes the end of the tc table.
       That wrap is restated from reading the reference; no recorded run reaches it, and the oracle's behaviour is kept.
    c  QP alternating 0 / 51 from 8x8 block to block, offsets 0: every edge averages the two ends"""
    pic = X.dlf_picture(bps, w, h, which)
    want = oracle_dlf(oracle, pic)
    changed = [not np.array_equal(a, b) for a, b in zip(want, pic["pre"])]
    if which == "a":
        assert changed == [True, True, True]
    if which == "b":
        assert changed == [False, True, False]
    got = gpu_dlf(product, gpu_ctx, pic, pad=4 * (w == 72))
    for p in range(3):
        assert np.array_equal(got[p], want[p]), (p, np.argwhere(got[p] != want[p])[:5].tolist())


# ---- the chain statistics -> decision -> application, resident on the device ---------------------------------------------
@pytest.mark.parametrize("bps", BPS)
@pytest.mark.parametrize("kind", X.CHAIN_KINDS)
def test_sao_chain_on_saturated_pictures(libs, gpu_ctx, bps, kind):
    """luma statistics per 64x64 LCU and chroma per 32x32, the decision and the application launched back to back on the library's stream; only then are the
    statistics, parameters, costs and planes downloaded and compared with the same chain through the oracle (whose choices test_chain_oracle_guards checks)"""
    import torch
    product, oracle = libs
    want = oracle_chain(oracle, bps, kind)
    W, H, n = X.CHAIN_W, X.CHAIN_H, 6
    dsrc, drec = [to_dev(p) for p in want["src"]], [to_dev(p) for p in want["rec"]]
    ddst = [torch.zeros_like(t) for t in drec]
    dstats = [torch.full((n * STATS.itemsize,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(3)]
    dparams = to_dev(want["pic"]["params"])
    dcosts = torch.full((n, 2), -1, dtype=torch.int64).cuda()
    P = chain_params(bps)
    product.svt_amd_sao_decide_picture.argtypes = [vp, vp, vp, vp, vp, u32, u32, vp, vp, vp]
    product.svt_amd_sao_apply_picture.argtypes = [vp, C.c_int, vp, vp, u32, u32, u32, u32, vp, C.c_int, C.c_int]
    torch.cuda.synchronize()
    for c in range(3):
        pw, ph = (W, H) if c == 0 else (W // 2, H // 2)
        rc = product.svt_amd_sao_gather_picture(gpu_ctx, bps, dsrc[c].data_ptr(), pw, drec[c].data_ptr(), pw, pw, ph, 64 if c == 0 else 32, 0,
                                                dstats[c].data_ptr())
        assert rc == 0, product.svt_amd_last_error()
    rc = product.svt_amd_sao_decide_picture(gpu_ctx, P.ctypes.data, dstats[0].data_ptr(), dstats[1].data_ptr(), dstats[2].data_ptr(), 3, 2, None,
                                            dparams.data_ptr(), dcosts.data_ptr())
    assert rc == 0, product.svt_amd_last_error()
    ps, pd = (vp * 3)(*[t.data_ptr() for t in drec]), (vp * 3)(*[t.data_ptr() for t in ddst])
    rc = product.svt_amd_sao_apply_picture(gpu_ctx, bps, ps, pd, W, W // 2, W, H, dparams.data_ptr(), 1, 1)
    assert rc == 0, product.svt_amd_last_error()
    product.svt_amd_synchronize(gpu_ctx)
    for c in range(3):
        got = dstats[c].cpu().numpy().view(STATS)
        for k in STATS.names:
            assert np.array_equal(got[k], want["stats"][c][k]), (c, k)
    params = dparams.cpu().numpy().view(LCU)
    bad = [i for i in range(n) if params[i].tobytes() != want["params"][i].tobytes()]
    assert not bad, (bad, params[bad[0]], want["params"][bad[0]])
    assert np.array_equal(dcosts.cpu().numpy(), want["costs"])
    for c in range(3):
        got = from_dev(ddst[c], want["final"][c].dtype, want["final"][c].shape)
        assert np.array_equal(got, want["final"][c]), (c, np.argwhere(got != want["final"][c])[:5].tolist())
