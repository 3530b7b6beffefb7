"""CPU-only: the restatement of the mode decision's per-LCU controls (tests/mdctl_numpy.py) against the records the REFERENCE's own ConfigureChroma,
DeriveContouringClass, Forward85 / 84CuToModeDecision and edge-info derivation left through the project's svt_md_fill_lcu for the seeded records
(tests/golden/mdctl_*.npz, written by tests/golden/make_mdctl_golden.py), in every byte; the non-vacuity list on the fixtures alone; the restated tile flags
against the records of the mode-decision fixtures recorded from whole encodes; and the restated check summary against a direct loop."""
import importlib.util
import os

import numpy as np
import pytest

import mdctl_numpy as N
import mdctl_records as R
import svtlib as S

CASES = list(R.CASES)


def load_case(name):
    g = np.load(os.path.join(S.GOLDEN_DIR, "mdctl_%s.npz" % name))
    assert str(g["case"][0]) == name
    return {k: g[k] for k in g.files}


def same(got, want, tag):
    """two arrays of MD_LCU_DTYPE records: every byte, the first differing field named"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    for f in R.MD_LCU_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (tag, f, np.argwhere(got[f] != want[f])[:4].tolist())
    assert got.tobytes() == want.tobytes(), tag


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("make_mdctl_golden", os.path.join(S.GOLDEN_DIR, "make_mdctl_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_there_are_eight_fixtures_at_most_and_each_is_small():
    files = [f for f in os.listdir(S.GOLDEN_DIR) if f.startswith("mdctl_") and f.endswith(".npz")]
    assert sorted(files) == sorted("mdctl_%s.npz" % c for c in CASES) and len(files) <= 8
    assert all(os.path.getsize(os.path.join(S.GOLDEN_DIR, f)) < 1 << 20 for f in files)


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_gives_the_references_records_in_every_byte(name):
    w, h, seed, jobs = R.CASES[name]
    g = load_case(name)
    recs = R.case_inputs(name)
    for k, (jb, rec) in enumerate(zip(jobs, recs)):
        same(N.md_controls(w, h, rec, jb), g["lcu"][k], (name, k))
        if rec["sticky"] is not None:
            assert np.array_equal(N.md_controls(w, h, dict(rec, sticky=None), jb)["chroma_encode_mode"], g["chroma_without_sticky"][k]), (name, k)


def test_the_fixtures_are_not_vacuous(generator):
    generator.assert_not_vacuous({name: load_case(name) for name in CASES})


@pytest.mark.parametrize("name,tiles", [("md_b_tiles_motion_640x384_m8", (2, 2)), ("md_b_motion_416x240_m8", (1, 1)), ("md_i_tiles_motion_640x384_m9", (2, 2))])
def test_restated_tile_flags_against_recorded_encodes(name, tiles):
    g = np.load(os.path.join(S.GOLDEN_DIR, name + ".npz"))
    w, h = int(g["pic"][0]["width"]), int(g["pic"][0]["height"])
    left, top, right = N.tile_flags((w + 63) // 64, (h + 63) // 64, *tiles)
    for k in range(len(g["lcu"])):
        lcu = g["lcu"][k]
        assert np.array_equal(lcu["tile_left"], left) and np.array_equal(lcu["tile_top"], top) and np.array_equal(lcu["tile_right"], right), (name, k)
        assert int((left & top).sum()) == tiles[0] * tiles[1]


@pytest.mark.parametrize("wl,hl,cols,rows", [(1, 1, 1, 1), (7, 4, 7, 4), (11, 10, 3, 4), (33, 18, 5, 7), (60, 34, 20, 22)])
def test_tile_flags_mark_every_tile_once(wl, hl, cols, rows):
    left, top, right = N.tile_flags(wl, hl, cols, rows)
    assert int((left & top).sum()) == cols * rows and int(left.sum()) == cols * hl == int(right.sum()) and int(top.sum()) == rows * wl


def test_fixed_leaf_lists_are_the_references(generator):
    """the restated Forward85 / 84 lists are pinned by the fixtures' pictures without configuration records: count them"""
    seen = set()
    for name in CASES:
        w, h, seed, jobs = R.CASES[name]
        g = load_case(name)
        for k, jb in enumerate(jobs):
            if not jb["mdc"]:
                want = N.fixed_leaves(w, h, jb["depth_mode"])
                for f in ("leaf_count", "leaf_index", "leaf_split"):
                    assert np.array_equal(g["lcu"][k][f], want[f]), (name, k, f)
                seen.add((jb["depth_mode"], int(g["lcu"][k]["leaf_count"].max())))
    assert {(1, 85), (2, 84)} <= seen


def _damaged(seed):
    """records of a fixture with every refusal of the mode-decision call planted somewhere"""
    rng = np.random.default_rng(seed)
    lcus = load_case("uneven_704x640")["lcu"][0].copy()
    n = len(lcus)
    for i in rng.choice(n, 5, replace=False):
        lcus["leaf_count"][i] = rng.choice((0, 86, 255))
    for i in rng.choice(n, 5, replace=False):
        c = int(lcus["leaf_count"][i])
        if 2 <= c <= 85:
            lcus["leaf_index"][i, c - 1] = lcus["leaf_index"][i, c - 2] if rng.random() < 0.5 else 85
    for i in rng.choice(n, 5, replace=False):
        lcus["chroma_encode_mode"][i] = rng.choice((0, 3))
    lcus["lcu_md_mode"][rng.choice(n, 9, replace=False)] = rng.choice((0, 3, 4, 15, 16, 200), 9)
    return lcus


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("depth_mode,inter", [(0, 1), (0, 0), (1, 1), (2, 0), (3, 1), (5, 1)])
def test_the_restated_check_summary_equals_a_direct_loop(seed, depth_mode, inter):
    lcus = _damaged(seed) if seed else load_case("uneven_704x640")["lcu"][0]
    a, b = N.check_summary(lcus, depth_mode, inter), N.check_summary_loop(lcus, depth_mode, inter)
    assert a.tobytes() == b.tobytes(), (a, b)
    if seed == 0 and (depth_mode in (1, 2, 5) or not inter):   # (the records carry the methods 3 and 4, which a P / B call under PICT_LCU_SWITCH refuses)
        assert int(a["first_bad"]) == 0xFFFFFFFF and int(a["tiles"]) == 12 and int(a["md_mode"].sum()) == len(lcus)
    if seed:
        assert int(a["first_bad"]) != 0xFFFFFFFF and int(a["bad_leaf_count"]) == 5 and int(a["bad_chroma"]) == 5


def test_the_check_summary_accepts_what_the_library_accepts():
    """first_bad is none exactly where the host loop of svt_amd_md_encode_picture_inter passes: leaf counts, leaf lists and svt_amd_md_lcus_supported"""
    import ctypes as C
    assert os.path.exists(S.PRODUCT_SO), "run `python __graft_entry__.py build` first"
    lib = C.CDLL(S.PRODUCT_SO)
    lib.svt_amd_md_lcus_supported.restype, lib.svt_amd_md_lcus_supported.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int]
    P = np.zeros(1, S.MD_PICTURE_DTYPE)
    for seed in range(6):
        lcus = np.ascontiguousarray(_damaged(seed) if seed else load_case("uneven_704x640")["lcu"][0])
        for depth_mode in (0, 1, 3):
            P["depth_mode"] = depth_mode
            for i in range(len(lcus)):
                assert lib.svt_amd_md_lcus_supported(P.ctypes.data, lcus[i:i + 1].ctypes.data, 1) == int(N.lcu_supported(depth_mode, lcus[i])), (seed, depth_mode, i)
