"""CPU-only: the in-loop filter leaves at the ends of their ranges.  tests/golden/filterx_*.npz hold what the reference's own symbols computed on the seeded
inputs of tests/filter_extremes.py (made by tests/golden/make_filter_extremes_golden.py); the oracle must reproduce them bit for bit, and so must the
reference itself where oracle/_ref is built.  The guards below are worked out from the inputs and the recorded results, never from the code under test: they
fail if a fixture stops reaching the branch it is there for (the signed 8-bit clip of the SAO statistics, the clip of the SAO offsets to the sample range, the
tc = 0 / beta = 0 ends of the deblocking cores).  The picture-level SAO oracle and the chain statistics -> decision -> application are pinned here on
saturated pictures before tests/test_gpu_filter_extremes.py compares the device against them."""
import os

import numpy as np
import pytest

import filter_extremes as X
import svtlib as S
from test_oracle_dlf_golden import oracle_sao
from test_oracle_saodec_golden import STATS as DEC_STATS, oracle_decide_picture

ref = S.load_ref()
needs_ref = pytest.mark.skipif(ref is None, reason="oracle/_ref/libsvtref.so not built")
BPS = [1, 2]
_fixtures = {}


def fixture(kind):
    if kind not in _fixtures:
        g = np.load(os.path.join(S.GOLDEN_DIR, "filterx_%s.npz" % kind))
        _fixtures[kind] = {k: g[k] for k in g.files}
        for a in _fixtures[kind].values():
            a.setflags(write=False)
    return _fixtures[kind]


def same_stats(got, want, bps):
    names = [n for n, *_ in X.gather_cases(bps)]
    for i, name in enumerate(names):
        for only in (0, 1):
            for k in X.STATS.names:
                assert np.array_equal(got[i, only][k], want[i, only][k]), (name, only, k, got[i, only][k], want[i, only][k])


def same_apply(got, want, bps):
    assert got.shape == want.shape and got.dtype == want.dtype
    for name, op, _, sl in X.apply_slices(bps):
        assert np.array_equal(got[sl], want[sl]), (name, op, np.flatnonzero(got[sl] != want[sl])[:5].tolist())


def same_dlf(got, want, bps):
    for g, w, what in zip(got, want, ("luma", "chroma")):
        assert g.shape == w.shape and g.dtype == w.dtype
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))
        assert len(bad) == 0, (what, bps, bad[:5].tolist(), g[bad[0]].tolist(), w[bad[0]].tolist())


def check_all(impl, bps):
    same_stats(X.run_gather(impl, bps), fixture("gather")["g%d" % bps], bps)
    same_apply(X.run_apply(impl, bps), fixture("apply")["a%d" % bps], bps)
    same_dlf(X.run_dlf(impl, bps), (fixture("dlf")["l%d" % bps], fixture("dlf")["c%d" % bps]), bps)


@pytest.mark.parametrize("bps", BPS)
def test_oracle_matches_recorded_reference(oracle, bps):
    check_all(X.Oracle(oracle), bps)


@needs_ref
@pytest.mark.parametrize("bps", BPS)
def test_live_reference_matches_its_records(bps):
    check_all(X.Leaves(ref), bps)


def test_fixture_layout():
    for bps in BPS:
        n = len(list(X.gather_cases(bps)))
        assert n == len(X.GATHER_KINDS) * len(X.GATHER_SIZES) and fixture("gather")["g%d" % bps].shape == (n, 2)
        assert fixture("apply")["a%d" % bps].size == sum(w * h for _, w, h in X.APPLY_PLANES) * len(X.apply_ops())
        lum, chrm = X.dlf_cases(bps)
        assert fixture("dlf")["l%d" % bps].shape == (len(lum), 4, 8) and fixture("dlf")["c%d" % bps].shape == (len(chrm), 2, 2, 4)
    for name in ("gather", "apply", "dlf"):
        assert os.path.getsize(os.path.join(S.GOLDEN_DIR, "filterx_%s.npz" % name)) <= 90 * 1024


# ---- vacuity guards --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bps", BPS)
def test_gather_fixture_reaches_the_clip(bps):
    """8 bit: in clip_all every interior difference lies beyond the signed 8-bit range and the recorded sums are those of the clipped differences, not of
    the plain ones; clip_half has both kinds of sample.  10 bit: the recorded sums are the plain ones (differences up to +-1023)."""
    want = fixture("gather")["g%d" % bps]
    seen_clip = 0
    for i, (name, src, rec, w, h) in enumerate(X.gather_cases(bps)):
        d = src[1:h - 1, 1:w - 1].astype(np.int64) - rec[1:h - 1, 1:w - 1]
        plain, clipped = int(d.sum()), int(np.clip(d, -128, 127).sum())
        got = int(want[i, 0]["boDiff"].sum())
        assert int(want[i, 0]["boCount"].sum()) == d.size
        if name.startswith("clip_all"):
            assert (np.abs(d) > 127).all() and (d > 0).all() != (d < 0).all()
        if name.startswith("clip_half"):
            far = np.abs(d) > 127
            assert far.any() and (~far).any() and (w < 40 or 0.3 < far.mean() < 0.7)
        if bps == 1:
            assert got == clipped
            if name.startswith("clip_"):
                assert plain != clipped
                seen_clip += 1
        else:
            assert got == plain
            if name.startswith("clip_all"):
                assert plain != clipped and np.abs(d).max() > 900
        # every class of the edge statistics sums the same differences
        assert int(want[i, 0]["eoCount"][:, :4].sum()) <= 4 * d.size
    assert bps == 2 or seen_clip == 3 * len(X.GATHER_SIZES)


@pytest.mark.parametrize("bps", BPS)
def test_gather_fixture_reaches_one_band_waves_and_mixed_waves(bps):
    """from the inputs: flat_band puts every interior sample into one band; two_bands has a 64-sample run of the row-major interior index that holds both
    bands; stripes alternates bands 0 and 31 from sample to sample"""
    sh = 3 if bps == 1 else 5
    want = fixture("gather")["g%d" % bps]
    for i, (name, src, rec, w, h) in enumerate(X.gather_cases(bps)):
        bands = (rec[1:h - 1, 1:w - 1] >> sh).reshape(-1)
        if name.startswith("flat_band"):
            assert len(np.unique(bands)) == 1 and np.count_nonzero(want[i, 0]["boCount"]) == 1
            assert want[i, 0]["boCount"].max() == (w - 2) * (h - 2)
        if name.startswith("two_bands"):
            runs = [np.unique(bands[k:k + 64]) for k in range(0, len(bands), 64)]
            assert any(len(r) == 2 for r in runs) and set(np.unique(bands).tolist()) == {3, 20}
        if name.startswith("stripes"):
            assert set(np.unique(bands).tolist()) == {0, 31} and (bands.reshape(h - 2, w - 2)[:, 1:] != bands.reshape(h - 2, w - 2)[:, :-1]).all()


@pytest.mark.parametrize("bps", BPS)
def test_apply_fixture_reaches_the_sample_range_clip(bps):
    want, maxv = fixture("apply")["a%d" % bps], X.maxv_of(bps)
    meant = 0
    for name, op, area, sl in X.apply_slices(bps):
        if X.apply_meant_to_clip(name, op):
            out, src = want[sl], area.reshape(-1)
            assert (((out == 0) | (out == maxv)) & (out != src)).any(), (name, op)
            meant += 1
    assert meant == 4 * 4 + 4 * 4 + 2 * 4    # four saturated planes: four band offsets and the four edge classes of set one each; set two on the two larger `blocks` planes
    assert set(X.APPLY_BANDS) >= {29, 30, 31} and abs(int(X.apply_offsets(2)[0][0])) == 31


@pytest.mark.parametrize("bps", BPS)
def test_dlf_fixture_ends(bps):
    """tc == 0 or beta == 0 leaves the luma block as it was, tc == 0 the chroma plane; the cases listed as filtering do change samples"""
    lum, chrm = X.dlf_cases(bps)
    lw, cw = fixture("dlf")["l%d" % bps], fixture("dlf")["c%d" % bps]
    sh = X.dlf_shift(bps)
    off = filt = 0
    for i, c in enumerate(lum):
        before = X.luma_window(c["block"], c["vertical"])[0]
        if c["tc"] == 0 or c["beta"] == 0:
            assert np.array_equal(lw[i], before), i
            off += 1
        if c["filters"]:
            assert not np.array_equal(lw[i], before), (i, c["tc"], c["beta"])
            filt += 1
    assert off > 100 and filt == 2 * 3 * 3      # directions x levels x the steps 2, tc and 5 * tc / 2
    assert {c["tc"] for c in lum} == {0, 1 << sh, 24 << sh} and {c["beta"] for c in lum} == {0, 1 << sh, 64 << sh}
    off = filt = 0
    for i, c in enumerate(chrm):
        for k, (plane, tc, f) in enumerate(((c["cb"], c["cb_tc"], c["cb_filters"]), (c["cr"], c["cr_tc"], c["cr_filters"]))):
            before = X.chroma_window(plane, c["vertical"])[0]
            if tc == 0:
                assert np.array_equal(cw[i, k], before), (i, k)
                off += 1
            if f:
                assert not np.array_equal(cw[i, k], before), (i, k, tc)
                filt += 1
    assert off > 50 and filt > 50
    assert {c["cb_tc"] for c in chrm} == ({0, 1, 24} if bps == 1 else {0, 4, 96})


# ---- the picture-level SAO oracle against the leaf records -----------------------------------------------------------
@pytest.mark.parametrize("bps", BPS)
@pytest.mark.parametrize("w", [64, 128])
def test_sao_picture_oracle_matches_leaf_records(oracle, bps, w):
    """A 64x64 and a 128x64 picture whose luma LCUs are the 64x64 planes of the apply cases: band offset (type 5) must give the leaf's recorded LCU, an edge
    class the leaf's interior (the border samples see other neighbours, or are skipped at a flagged edge).  Once with the picture's own edges flagged,
    once with all four flags set on every LCU."""
    want = fixture("apply")["a%d" % bps]
    planes = [(name, area, {op: want[sl].reshape(64, 64) for n2, op, _, sl in X.apply_slices(bps) if n2 == name})
              for name, op0, area, _ in X.apply_slices(bps) if name.endswith("64x64") and op0 == X.apply_ops()[0]]
    assert len(planes) == 2
    cols = w // 64
    luma = np.concatenate([planes[k][1] for k in range(cols)], axis=1)
    chroma = np.full((32, w // 2), 7, X.dtype_of(bps))
    offsets = X.apply_offsets(bps)
    for flags in (X.picture_edge_flags(cols, 1), np.full(cols, 15, np.uint8)):
        for op in X.apply_ops():
            lcus = np.zeros(cols, X.SAO_LCU)
            lcus["edge_flags"] = flags
            o = offsets[op[2]]
            lcus["type"][:, 0] = 5 if op[0] == "bo" else op[1] + 1
            lcus["offset"][:, 0] = o[:4] if op[0] == "bo" else o[[0, 1, 3, 4]]
            lcus["band"][:, 0] = op[1] if op[0] == "bo" else 0
            got = oracle_sao(oracle, [luma, chroma, chroma], bps, w, 64, lcus, 1, 0)
            assert np.array_equal(got[1], chroma) and np.array_equal(got[2], chroma)
            for k in range(cols):
                lcu, leaf = got[0][:, 64 * k:64 * k + 64], planes[k][2][op]
                if op[0] == "bo":
                    assert np.array_equal(lcu, leaf), (op, k)
                else:
                    assert np.array_equal(lcu[1:63, 1:63], leaf[1:63, 1:63]), (op, k)
                    assert not np.array_equal(lcu, luma[:, 64 * k:64 * k + 64])


# ---- the chain statistics -> decision -> application through the oracle --------------------------------------------------
CHAIN_LAMBDA = {1: (1 << 10, 1 << 10), 2: (1 << 10, 1 << 10)}


def chain_params(bps):
    """rate tables of test_gpu_saodec.random_picture (seed 7), full mode, layer 0; lambdas small enough that the small differences of the `ends` picture
    still pay for their offsets (checked by test_chain_oracle_guards)"""
    from test_gpu_saodec import random_picture
    P = random_picture(np.random.default_rng(7), 3, 2, int(bps == 2), 1, 0, 0, 0)["P"]
    P["lambda"], P["chroma_lambda"] = CHAIN_LAMBDA[bps]
    return P


_chains = {}


def oracle_chain(oracle, bps, kind):
    """-> dict(src, rec, stats[3][lcu], params, costs, final): luma statistics per 64x64 LCU, chroma per 32x32, computed once"""
    if (bps, kind) not in _chains:
        impl = X.Oracle(oracle)
        src, rec = X.chain_picture(bps, kind)
        cols, rows = X.CHAIN_W // 64, X.CHAIN_H // 64
        stats = np.zeros((3, cols * rows), DEC_STATS)
        for c in range(3):
            L, (ph, pw) = (64 if c == 0 else 32), src[c].shape
            for i in range(cols * rows):
                x0, y0 = (i % cols) * L, (i // cols) * L
                st, o = X.stats_record(), (y0 * pw + x0) * bps
                impl.gather(bps, 0, src[c], rec[c], pw, min(L, pw - x0), min(L, ph - y0), st, o, o)
                for k in X.STATS.names:
                    stats[c][i][k] = st[k]
        params = np.zeros(cols * rows, X.SAO_LCU)
        params["edge_flags"] = X.picture_edge_flags(cols, rows)
        pic = dict(P=chain_params(bps), stats=stats, enable=np.ones(cols * rows, np.uint8), params=params, cols=cols, rows=rows)
        out, costs = oracle_decide_picture(oracle, pic)
        final = oracle_sao(oracle, rec, bps, X.CHAIN_W, X.CHAIN_H, out, 1, 1)
        _chains[(bps, kind)] = dict(src=src, rec=rec, stats=stats, params=out, costs=costs, final=final, pic=pic)
    return _chains[(bps, kind)]


def chain_pushed_out(bps, ch):
    """samples whose offset, taken from the decided parameters, leads out of the sample range: what the final clip is there for"""
    maxv, n = X.maxv_of(bps), 0
    for c in range(3):
        L = 64 if c == 0 else 32
        rec = ch["rec"][c].astype(np.int64)
        for i, p in enumerate(ch["params"]):
            if p["type"][0 if c == 0 else 1] != 5:
                continue
            x0, y0 = (i % 3) * L, (i // 3) * L
            a = rec[y0:y0 + L, x0:x0 + L]
            k = (a >> (3 if bps == 1 else 5)) - int(p["band"][c])
            o = np.where((k >= 0) & (k < 4), np.asarray(p["offset"][c])[np.clip(k, 0, 3)], 0)
            n += int(((a + o < 0) | (a + o > maxv)).sum())
    return n


@pytest.mark.parametrize("bps", BPS)
def test_chain_oracle_guards(oracle, bps):
    """Over the three pictures together the oracle's chain picks an edge class somewhere and, in 8 bit, a band offset whose application has to be clipped (the
    10-bit decision has no band search: SaoGenerationDecision16bit only weighs the edge classes).  The flat picture feeds the decision its largest input: one
    band with count 3,844 and difference 3,844 x -128 (8 bit, clipped) / 3,844 x -1,023 (10 bit)."""
    chains = [oracle_chain(oracle, bps, k) for k in X.CHAIN_KINDS]
    types = np.concatenate([c["params"]["type"] for c in chains])
    assert ((types >= 1) & (types <= 4)).any()
    flat = chains[0]["stats"][0]
    assert (flat["boCount"][:, 31] == 3844).all() and (flat["boDiff"][:, 31] == 3844 * (-128 if bps == 1 else -1023)).all()
    if bps == 1:
        assert (types[:, 0] == 5).any()
        assert sum(chain_pushed_out(bps, c) for c in chains) > 0
    for c in chains:
        assert (c["params"]["band"] <= 28).all()
