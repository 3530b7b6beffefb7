"""CPU-only: the restatement of the temporal motion field and the intra-coded area (tests/tmvp_numpy.py) against the reference's own results
(tests/golden/tmvp_*.npz, tests/golden/make_tmvp_golden.py) - the field a reader of the reference recorded, on the fields it can see; the area
CopyStatisticsToRefObject left; the skip-cost bias the reference derived from the areas - and against the mode-decision fixtures that pair up: the final trees of
md_bref_* picture q give the field md_b_* picture p read.  The last test holds the fixtures to what they are meant to exercise."""
import os

import numpy as np
import pytest

import svtlib as S
import tmvp_numpy as N
import tmvplib as T


def dims(g):
    return int(g["clip"][1]), int(g["clip"][2])


@pytest.mark.parametrize("name", T.CASES)
def test_field_from_the_trees_is_the_field_the_reference_read(name):
    g = T.load_case(name)
    w, h = dims(g)
    for k, q in enumerate(g["q_poc"]):
        f = N.field(g["q_heads"][k], w, h, g["q_ref_poc"][k])
        assert N.mismatches(f, g["q_tmvp"][k], w, h) == 0, (name, int(q))
        ins, avail, _ = N.observable(g["q_tmvp"][k], w, h)
        assert np.array_equal(f["available"][:-1] != 0, avail), (name, int(q))       # (nothing outside the picture is available in the restatement)
        assert not f[-1].tobytes().strip(b"\0")
        if g["q_slice_type"][k] == 2:
            assert not f["available"].any()


@pytest.mark.parametrize("name", T.CASES)
def test_area_is_what_the_reference_object_holds(name):
    g = T.load_case(name)
    w, h = dims(g)
    for k, poc in enumerate(g["pic_poc"]):
        assert N.intra_coded_area(int(g["pic_area_sum"][k]), w, h, int(g["pic_slice_type"][k])) == int(g["pic_area"][k]), (name, int(poc))
    for k, q in enumerate(g["q_poc"]):                # ... and the sum is the sum over the trees
        at = int(np.nonzero(g["pic_poc"] == q)[0][0])
        assert N.intra_area_sum(g["q_heads"][k]) == int(g["pic_area_sum"][at]), (name, int(q))
        assert int(g["q_heads"][k][0]["slice_type"]) == int(g["pic_slice_type"][at]) and int(g["q_heads"][k][0]["temporal_layer"]) == int(g["pic_layer"][at])


@pytest.mark.parametrize("name", T.CASES)
def test_skip_cost_bias_is_the_area_rule(name):
    """every recorded non-reference B picture (test_fixtures_are_not_vacuous: the bias occurs set and clear)"""
    g = T.load_case(name)
    pocs = g["pic_poc"].tolist()
    for k, p in enumerate(g["r_poc"]):
        if g["r_slice_type"][k] != 0 or g["r_is_reference"][k]:
            continue
        refs = [pocs.index(int(r)) for r in g["r_ref_poc"][k]]
        want = N.skip_cost_bias(0, 0, [g["pic_area"][i] for i in refs], [g["pic_layer"][i] for i in refs])
        assert want == int(g["r_skip_cost_bias"][k]), (name, int(p))


def md_pair_fields(name, q, p):
    """(the field rebuilt from md_bref_<name> picture q, the field md_b_<name> picture p read, w, h, p's inter record)"""
    gq, gp = (np.load(os.path.join(S.GOLDEN_DIR, "md_%s_%s.npz" % (kind, name))) for kind in ("bref", "b"))
    kq, kp = gq["picture_number"].tolist().index(q), gp["picture_number"].tolist().index(p)
    w, h = int(gq["pic"][kq]["width"]), int(gq["pic"][kq]["height"])
    wl = (w + 63) // 64
    heads = np.stack([N.tree_from_out(o, min(64, w - 64 * (n % wl)), min(64, h - 64 * (n // wl))) for n, o in enumerate(gq["out"][kq])])
    assert int(gp["inter"][kp]["colocated_poc"]) == q and gp["tmvp_present"][kp]
    return N.field(heads, w, h, gq["inter"][kq]["ref_poc"]), gp["tmvp"][kp], w, h, gp["inter"][kp]


@pytest.mark.parametrize("name,q,p", [(name, q, p) for name, pairs in T.MD_PAIRS for q, p in pairs])
def test_recorded_decisions_of_q_give_the_field_p_read(name, q, p):
    f, want, w, h, _ = md_pair_fields(name, q, p)
    assert N.mismatches(f, want, w, h) == 0


def test_fixtures_are_not_vacuous():
    seen = set()
    for name in T.CASES:
        g = T.load_case(name)
        w, h = dims(g)
        ins = N.inside(w, h)
        if (w, h) in ((416, 240), (200, 136)):
            assert not ins.all() and ins.any()
            seen.add("outside %dx%d" % (w, h))
        for k in range(len(g["q_poc"])):
            f = N.field(g["q_heads"][k], w, h, g["q_ref_poc"][k])
            for d in range(3):
                if ((f["pred_dir"] == d) & (f["available"] != 0)).any():
                    seen.add("direction %d" % d)
            st = int(g["q_slice_type"][k])
            if st == 2:
                seen.add("I picture as q")
                at = int(np.nonzero(g["pic_poc"] == g["q_poc"][k])[0][0])
                if g["pic_area"][at] == 0 and g["pic_area_sum"][at] == sum(min(64, w - x) * min(64, h - y) for y in range(0, h, 64) for x in range(0, w, 64)):
                    seen.add("I picture: area 0 with every unit intra")
            for hd in g["q_heads"][k]:
                cus = hd["cu"][:int(hd["num_cus"])]
                if st != 2 and (cus["pred_mode"] == 2).any():
                    seen.add("intra unit in a P / B picture")
                if (cus["size"] == 64).any():
                    seen.add("64x64 unit")
                for a in cus[(cus["size"] == 8) & (cus["x"] % 16 == 0) & (cus["y"] % 16 == 0)]:
                    sib = cus[(cus["size"] == 8) & (cus["x"] // 16 == a["x"] // 16) & (cus["y"] // 16 == a["y"] // 16)]
                    keys = set((int(c["pred_mode"]), int(c["inter_dir"]), c["mv"].tobytes()) if c["pred_mode"] == 1 else (2,) for c in sib)
                    if len(sib) == 4 and len(keys) > 1:
                        seen.add("16x16 of differing 8x8 units")
        if (g["pic_area"][g["pic_slice_type"] != 2] == 0).any():
            seen.add("area 0")
        if (g["pic_area"] > 90).any():
            seen.add("area above 90")
        if (g["r_skip_cost_bias"] != 0).any():
            seen.add("skip-cost bias set")
        if ((g["r_skip_cost_bias"] == 0) & (g["r_slice_type"] == 0) & (g["r_is_reference"] == 0)).any():
            seen.add("skip-cost bias clear")
    want = {"outside 416x240", "outside 200x136", "direction 0", "direction 1", "direction 2", "I picture as q", "I picture: area 0 with every unit intra",
            "intra unit in a P / B picture", "64x64 unit", "16x16 of differing 8x8 units", "area 0", "area above 90", "skip-cost bias set", "skip-cost bias clear"}
    assert want <= seen, want - seen
