"""CPU-only: P / B pictures coded WITHOUT sub-sample search (useSubpelFlag 0 - encMode 9 at the 4K input class, temporal layers above 0).
 - the two recorded pictures (tests/golden/mdifree_*.npz, tests/golden/make_md_ifree_golden.py) are what the GPU tests need them to be;
 - the support predicates accept them in 8 bits, refuse them in 10 (svt_amd_md_picture_supported_inter16) and refuse them with any one field outside the device call;
 - the positions of the interpolation-free prediction (svt-hevc_amd/csrc/inter_position.h: whole-sample rounding, interpolation-free luma position, nearest chroma sample)
   as a plain C program of its own (tools/inter_ifree_check.c) built with -fsanitize=address,undefined and run directly, against a restatement in Python integers of
   RoundMv / RoundMvOnTheFly (Codec/EbModeDecision.c:200, Codec/EbInterPrediction.c:46) and UniPredIFreeRef8Bit (Codec/EbAvcStyleMcp.c:172) - and, where the reference
   library is built, against its own RoundMvOnTheFly."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import svtlib as S

FIXTURES = sorted(glob.glob(os.path.join(S.GOLDEN_DIR, "mdifree_*.npz")))
NAMES = [os.path.basename(f) for f in FIXTURES]
W, H = 200, 136
VECTORS = (-32768, -5, -3, -2, -1, 0, 1, 2, 3, 5, 6, 7, 32767)
# IntegerPosoffsetTabX / IntegerPosoffsetTabY (Codec/EbAvcStyleMcp.c:19-27), index = fracX + 4 fracY
OFFSET_X = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0)
OFFSET_Y = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1)


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------------------------------

def test_there_are_two_fixtures_a_layer_2_and_a_layer_1_picture():
    assert len(FIXTURES) == 2, FIXTURES
    pics = [np.load(f)["pic"][0] for f in FIXTURES]
    assert sorted((int(p["temporal_layer"]), int(p["is_reference"])) for p in pics) == [(1, 1), (2, 0)]


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_the_fixture_is_a_whole_picture_without_sub_sample_search(path):
    assert os.path.getsize(path) <= 1 << 20, os.path.getsize(path)                                  # (the issue allows 2.3 MB; a committed file has to stay below 1 MiB)
    g = np.load(path)
    assert len(g["picture_number"]) == 1
    P, X, lcus, o = g["pic"][0], g["inter"][0], g["lcu"][0], g["out"][0]
    w, h = int(P["width"]), int(P["height"])
    assert w * h >= 0x29F630                                                   # INPUT_SIZE_4K_TH: the input class whose encMode 9 switches the sub-sample search off
    assert int(X["use_subpel"]) == 0 and int(P["slice_type"]) == 0 and int(P["enc_mode"]) == 9
    assert len(lcus) == len(o) == S.lcu_count(w, h)                            # every LCU is recorded
    assert set(lcus["chroma_encode_mode"].tolist()) == ({2} if int(P["temporal_layer"]) == 2 else {1})   # CHROMA_MODE_BEST on layer 2, CHROMA_MODE_FULL on layer 1
    # the co-located picture is a P / B picture: fractional vectors reach the picture through the temporal candidate
    assert bool(g["tmvp_present"][0]) and ((g["tmvp"][0]["mv"] & 3) != 0).any()
    tested = o["tested"] != 0
    inter = tested & (o["pred_mode"] == 1)
    frac_l = ((o["mv"] & 3) != 0).any(axis=-1)                                 # (LCU, leaf, list)
    d = o["inter_dir"]
    frac = inter & (((d != 1) & frac_l[..., 0]) | ((d != 0) & frac_l[..., 1]))
    merge = inter & (o["merge_flag"] == 1)
    print("FIXTURE %s: %d bytes, tested units %d, with a fractional vector component %d (merge %d, bi-predicted merge %d), uni-predicted merge units %d" %
          (os.path.basename(path), os.path.getsize(path), int(tested.sum()), int(frac.sum()), int((frac & merge).sum()), int((frac & merge & (d == 2)).sum()),
           int((merge & (d != 2)).sum())))
    assert frac.sum() >= 300
    assert (frac & merge & (d == 2)).sum() >= 20
    # Merge units of both uni- and bi-prediction are among the tested units.  A FRACTIONAL uni-predicted one cannot exist in a B picture of these encodes: every
    # candidate of the motion estimation is rounded at its injection, so a fraction enters through the temporal merge candidate alone, which a B slice builds bi-predicted
    # (md_merge_list_regs: add(MD_BI, t0, t1)), and a spatial neighbour hands a candidate on with its direction.  The uni-predicted merge units take the same rounding
    # and the same copy with whole vectors.
    assert (merge & (d != 2)).sum() >= 20 and (merge & (d == 2)).sum() >= 20
    assert not (frac & (d != 2)).any()
    # a unit that is no merge unit carries whole vectors (RoundMv at the injection)
    assert not (frac & ~merge).any()


# ---- the support predicates -----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(S.PRODUCT_SO)                                                 # host functions only: no device is opened
    for f in ("svt_amd_md_picture_supported_inter", "svt_amd_md_picture_supported_inter16"):
        getattr(lib, f).restype, getattr(lib, f).argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    return lib


OUTSIDE_P = dict(slice_type=2, intra_md_open_loop=0, coeff_cabac_update=1, intra4x4_level=1, rdoq_pmcore_method=1, single_fast_loop=1, spatial_sse_full_loop=1, pf_md_level=2,
                 nfl_level_md=3, intra_injection_method=2, limit_ois_to_dc_mode=1, mpm_search=1, enc_mode=10, width=2692, height=1020)
OUTSIDE_X = dict(unrestricted_mv=0, generate_amvp_table_md=0, extra_injection=1, improve_sharpness=1)


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_the_predicates_accept_the_recorded_headers_in_8_bits_only(lib, path):
    g = np.load(path)
    P, X = np.ascontiguousarray(g["pic"][0:1]), np.ascontiguousarray(g["inter"][0:1])
    assert lib.svt_amd_md_picture_supported_inter(P.ctypes.data, X.ctypes.data) == 1
    assert lib.svt_amd_md_picture_supported_inter16(P.ctypes.data, X.ctypes.data) == 0        # a 10-bit picture: the 16-bit entries' predicate
    Xs = X.copy()
    Xs["use_subpel"] = 1                                                                      # ... which the flag alone decides
    assert lib.svt_amd_md_picture_supported_inter16(P.ctypes.data, Xs.ctypes.data) == 1
    for field, value in OUTSIDE_P.items():
        Pb = P.copy()
        assert int(Pb[field][0]) != value
        Pb[field] = value
        assert lib.svt_amd_md_picture_supported_inter(Pb.ctypes.data, X.ctypes.data) == 0, field
    for field, value in OUTSIDE_X.items():
        Xb = X.copy()
        assert int(Xb[field][0]) != value
        Xb[field] = value
        assert lib.svt_amd_md_picture_supported_inter(P.ctypes.data, Xb.ctypes.data) == 0, field


# ---- the positions --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("inter_ifree") / "inter_ifree_check"
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(S.ROOT, "tools", "inter_ifree_check.c"), "-o", str(exe)])
    return str(exe)


def run(checker, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([checker] + [str(v) for v in args], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]


def rounded(v):
    """RoundMv: (v + 2) & ~3 in int, stored into an EB_S16"""
    r = ((v + 2) & ~3) & 0xFFFF
    return r - 0x10000 if r >= 0x8000 else r


def clamped(at, mv, origin, extent):
    return sorted((4 * (origin - 71), 4 * (at + origin) + mv, 4 * (extent + origin + 7)))[1]


def restated(at, mvx, mvy, origin):
    """(qx, qy, luma x, luma y, chroma x, chroma y) of UniPredIFreeRef8Bit for the clamped position of a vector"""
    qx, qy = clamped(at, mvx, origin, W), clamped(at, mvy, origin, H)
    f = (qx & 3) + ((qy & 3) << 2)
    return (qx, qy, (qx >> 2) + OFFSET_X[f], (qy >> 2) + OFFSET_Y[f], (qx >> 3) + ((qx & 7) > 4), (qy >> 3) + ((qy & 7) > 4))


def test_the_pinned_roundings(checker):
    values = (-32768, -32767, -7, -6, -5, -3, -2, -1, 0, 1, 2, 3, 5, 6, 7, 32765, 32766, 32767)
    got = [g[0] for g in run(checker, ["round"] + list(values))]
    # halves round up; the last two wrap as the reference's 16-bit store does
    assert got == [-32768, -32768, -8, -4, -4, -4, 0, 0, 0, 0, 4, 4, 4, 8, 8, 32764, -32768, -32768], got
    assert got == [rounded(v) for v in values]
    assert [g[0] for g in run(checker, ["round"] + got)] == got                # applied twice it changes nothing more


@pytest.mark.parametrize("origin", [8, 80])
def test_the_sweep_equals_the_restatement(checker, origin):
    rows = run(checker, ["sweep", W, H, origin])
    assert len(rows) == 25 * 13 * 13
    seen, fractions, bumped = set(), set(), 0
    for row in rows:
        at, mvx, mvy, rx, ry, r2x, r2y = row[:7]
        seen.add((at, mvx, mvy))
        assert (rx, ry) == (rounded(mvx), rounded(mvy)) == (r2x, r2y), row
        assert row[7:13] == restated(at, mvx, mvy, origin), row
        assert row[13:19] == restated(at, rx, ry, origin), row
        qx, qy, lx, ly, cx, cy = row[7:13]
        fractions.add((qx & 3, qy & 3))
        bumped += (lx, ly) != (qx >> 2, qy >> 2)
        # the rounded vector's position is a whole luma sample: the luma copy starts there, the chroma copy at the sample below a half
        Qx, Qy, Lx, Ly, Cx, Cy = row[13:19]
        assert Qx % 4 == 0 and Qy % 4 == 0 and (Lx, Ly, Cx, Cy) == (Qx // 4, Qy // 4, Qx // 8, Qy // 8), row
    assert seen == {(at, a, b) for at in range(0, 193, 8) for a in VECTORS for b in VECTORS}
    assert len(fractions) == 16 and bumped > 0                                 # every entry of the two tables is read, the four non-zero ones among them


def test_the_rounding_equals_the_references_own(checker):
    ref = S.load_ref()
    if ref is None:
        return                                                                  # the reference library is test infrastructure: built only where its sources are
    ref.RoundMvOnTheFly.restype, ref.RoundMvOnTheFly.argtypes = None, [C.POINTER(C.c_int16), C.POINTER(C.c_int16)]
    values = sorted(set(VECTORS) | set(range(-40, 41)) | {32764, 32765, 32766, -32767, -32766})
    ours = [g[0] for g in run(checker, ["round"] + values)]
    for v, want in zip(values, ours):
        x, y = C.c_int16(v), C.c_int16(-v if v != -32768 else 0)
        ref.RoundMvOnTheFly(C.byref(x), C.byref(y))
        assert x.value == want and y.value == rounded(-v if v != -32768 else 0), (v, x.value, want)


def test_a_bad_command_line_is_not_run(checker):
    assert subprocess.run([checker, "sweep", "1"], capture_output=True, text=True).returncode == 2
