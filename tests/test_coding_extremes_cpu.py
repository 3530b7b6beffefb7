"""CPU-only guards of the saturated fixtures at the ends of the QP range (tests/golden/*_xc_*.npz, recorded from the reference by the make_*_golden.py recorders on the
"xc_" clips: luma and chroma of 0 and 255).  The glob-driven CPU and GPU tests of the mode decision, the encode pass and the two full loops compare the oracle and the
kernels with these records; the conditions here prove that the records are where their names claim - saturated planes, picture QPs at both ends, levels in the
thousands, units with and without coefficients, both matrix-core transform sizes - so that a re-recording that drifts away from the bounds fails here and not silently.
They read fixtures only."""
import glob
import os

import numpy as np

import svtlib as S
from test_oracle_md_golden import md_stats


def _names(prefix):
    return sorted(os.path.basename(p)[len(prefix) + 1:-4] for p in glob.glob(os.path.join(S.GOLDEN_DIR, prefix + "_*.npz")) if "_xc_" in "_" + os.path.basename(p))


def _load(prefix, name):
    return np.load(os.path.join(S.GOLDEN_DIR, "%s_%s.npz" % (prefix, name)))


MD, EP, FL, CL = _names("md"), _names("encodepass"), _names("fullloop"), _names("chromaloop")
MD_I = [n for n in MD if n.startswith("i_")]
MD_PB = [n for n in MD if not n.startswith("i_")]
LEAF_SIZE = np.array([md_stats(leaf)[1] for leaf in range(85)])


def _units(g, field, sub):
    """`sub` of every coding unit the records of an encode-pass fixture hold"""
    return np.concatenate([g[field][i]["cu"][sub][:g["work"][i]["num_cus"]] for i in range(len(g["work"]))])


def test_the_fixtures_are_there():
    assert len(MD_I) >= 3 and len(MD_PB) >= 4 and len(EP) >= 6 and len(FL) >= 3 and len(CL) >= 2
    for prefix in ("b_", "bref_"):   # both kinds of B picture: the luma-only candidates and the CHROMA_MODE_FULL ones (the 8x8 chroma pair of a 16x16 unit)
        assert any(n.startswith(prefix) for n in MD_PB), prefix
    assert any(_load("md", n)["pic"]["chroma_level"].max() == 4 for n in MD_PB if n.startswith("bref_"))
    assert sum(n.startswith("cabac_") for n in FL) >= 1 and sum(not n.startswith("cabac_") for n in FL) >= 2
    assert any(n.startswith("sao_") for n in EP) and any(n.startswith("i10_") for n in EP) and any(n.startswith("p_") for n in EP) and any(n.startswith("b_") for n in EP)


def test_source_planes_hold_only_the_saturated_values():
    """luma AND chroma: {0, 255} for the 8-bit kinds, 0..3 and 1020..1023 for the 10-bit kind ((8 bit << 2) | two noise bits)"""
    for n in MD:
        g = _load("md", n)
        for k in ("src_y", "src_cb", "src_cr"):
            assert set(np.unique(g[k]).tolist()) == {0, 255}, (n, k)
        if "ref0_y" in g.files:   # ... and the reference pictures are reconstructions of such planes: both ends of the range are in them
            assert g["ref0_y"].min() == 0 and g["ref0_y"].max() == 255, n
    for n in EP:
        w = _load("encodepass", n)["work"]
        for k in ("src_y", "src_cb", "src_cr"):
            v = np.unique(w[k])
            if n.split("_")[0].endswith("10"):
                assert ((v <= 3) | (v >= 1020)).all() and v.min() <= 3 and v.max() >= 1020 and v.max() <= 1023, (n, k, v)
            else:
                assert set(v.tolist()) == {0, 255}, (n, k)
    for prefix, names in (("fullloop", FL), ("chromaloop", CL)):   # these records hold residuals: both bounds are reached, none is passed
        for n in names:
            r = _load(prefix, n)["residual"]
            assert r.min() == -255 and r.max() == 255, (prefix, n)


def test_picture_qps_reach_both_ends():
    qi = np.concatenate([_load("md", n)["pic"]["qp"] for n in MD_I])
    assert (qi == 0).any() and (qi == 51).any()
    qpb = np.concatenate([_load("md", n)["pic"]["qp"] for n in MD_PB])
    assert qpb.max() == 51
    # the reference's own value: from -q 0 its layer offsets give the P / B pictures of a three-level random-access encode QP 3 (layer 1) and 5 (layers 2 and 3)
    assert qpb.min() == 3
    for n in MD_PB:
        g = _load("md", n)
        want = {"q0": {1: 3, 2: 5, 3: 5}, "q51": {1: 51, 2: 51, 3: 51}}[n.rsplit("_", 1)[1]]
        for pic in g["pic"]:
            assert int(pic["qp"]) == want[int(pic["temporal_layer"])], (n, int(pic["temporal_layer"]), int(pic["qp"]))
    # the chroma QP table's ends: 0 at QP 0, and the clamped layer offsets of the QP 51 pictures reach its last entries
    cq = np.concatenate([_load("md", n)["pic"]["chroma_qp"] for n in MD])
    assert cq.min() == 0 and cq.max() == 47
    for n in EP:
        g = _load("encodepass", n)
        q = _units(g, "work", "qp")
        assert (q.max() == 51 and q.min() == 51) if n.endswith("q51") else q.min() <= 3, (n, q.min(), q.max())
    for n in FL:
        q = _load("fullloop", n)["qp"]
        assert q.max() == 51 if n.endswith("q51") else q.min() == 0, n
    for n in CL:
        q = _load("chromaloop", n)["cb_qp"]
        assert q.max() == 47 if n.endswith("q51") else q.min() == 3, n


def test_low_qp_records_hold_levels_in_the_thousands():
    """a flat residual of 128 in a 32x32 unit at QP 0 gives a level of about 128 * 128 * 26214 >> 16 = 6500: at least 1024 leaves a wide margin and is already past the
    prefix of the escape binarisation and far into the de-quantiser's products"""
    for n in EP:
        if n.endswith("q0"):
            r = _load("encodepass", n)["result"]
            assert max(int(np.abs(r[k].astype(np.int32)).max()) for k in ("coeff_y", "coeff_cb", "coeff_cr")) >= 1024, n
    for prefix, names in (("fullloop", FL), ("chromaloop", CL)):
        for n in names:
            if n.endswith("q0"):
                assert int(np.abs(_load(prefix, n)["quant"].astype(np.int32)).max()) >= 1024, (prefix, n)


def test_high_qp_records_hold_units_with_and_without_coefficients():
    for n in MD:
        if n.endswith("q51"):
            o = _load("md", n)["out"]
            y = o["ycbf"][o["tested"] == 1]
            assert (y != 0).any() and (y == 0).any(), n
    for n in EP:
        if n.endswith("q51"):
            cbf = _units(_load("encodepass", n), "result", "cbf")
            assert (cbf[:, 0] != 0).any() and (cbf[:, 0] == 0).any(), n   # luma; the saturated chroma planes keep coefficients in almost every unit
            assert (cbf != 0).any(axis=0).all(), n
    for n in FL:
        if n.endswith("q51"):
            y = _load("fullloop", n)["ycbf_after"]
            assert (y != 0).any() and (y == 0).any(), n
    for n in CL:
        if n.endswith("q51"):
            c = _load("chromaloop", n)["cbf_out"]
            assert (c != 0).any() and (c == 0).any(), n


def test_both_matrix_core_transform_sizes_are_tested_leaves():
    """16x16 and 32x32 leaves (64x64 leaves are four 32x32 transforms), in I pictures and in both kinds of B picture"""
    for names in (MD_I, [n for n in MD_PB if n.startswith("b_")], [n for n in MD_PB if n.startswith("bref_")]):
        got = {16: 0, 32: 0}
        for n in names:
            o = _load("md", n)["out"]
            for s in got:
                got[s] += int((o["tested"][..., LEAF_SIZE == s] == 1).sum())
        assert got[16] > 0 and got[32] > 0, (names, got)
