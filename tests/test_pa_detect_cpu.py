"""CPU-only: the C-ABI of the batched chroma statistics / picture detectors (include/svt_hevc_amd.h "Batched chroma statistics", "Batched picture detectors") -
the four entries are exported, the size helpers and record layouts are the documented ones - and the numpy restatement (tests/pa_detect_numpy.py) against what
the REFERENCE's GatheringPictureStatistics computed on seeded pictures (tests/golden/padetect_*.npz, tests/golden/make_pa_detect_golden.py): every array."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import pa_detect_numpy as N
import pa_detect_pictures as P
import svtlib as S
from abi_util import exported, open_library
from pa_batch_util import refused, refused_as
from test_oracle_pa import oracle_picture as pa_oracle

CASES = sorted(os.path.basename(p)[9:-4] for p in glob.glob(os.path.join(S.GOLDEN_DIR, "padetect_*.npz")))


def load_case(name):
    g = np.load(os.path.join(S.GOLDEN_DIR, "padetect_%s.npz" % name))
    kind, w, h, seed, rw, rh = str(g["clip"][0]), int(g["clip"][1]), int(g["clip"][2]), int(g["clip"][3]), int(g["clip"][4]), int(g["clip"][5])
    return g, kind, w, h, seed, rw, rh


@pytest.fixture(scope="module")
def lib():
    return open_library(N.declare)


def test_have_the_four_cases():
    assert CASES == ["islands_704x640", "motion_416x240", "noise_200x136", "objects_1280x720"]


def test_entries_are_exported():
    assert {"svt_amd_chroma_stats_batch_launch", "svt_amd_chroma_stats_bytes", "svt_amd_picture_detect_batch_launch", "svt_amd_picture_detect_bytes"} <= exported()


def test_record_layouts(tmp_path):
    assert N.LCU_CHROMA_DTYPE.itemsize == 48 and N.LCU_DETECT_DTYPE.itemsize == 48 and N.PIC_DETECT_DTYPE.itemsize == 8
    assert C.sizeof(N.ChromaJob) == 24 and C.sizeof(N.DetectJob) == 24
    assert C.sizeof(N.ChromaArrays) == 4 * C.sizeof(C.c_void_p) and C.sizeof(N.DetectArrays) == 2 * C.sizeof(C.c_void_p)
    assert N.LCU_DETECT_DTYPE.fields["edge_cu"][1] == 32 and N.LCU_DETECT_DTYPE.fields["sharp_edge"][1] == 37
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "svt_hevc_amd.h"\n'
                   '_Static_assert(sizeof(SvtAmdPaLcuChroma) == 48 && offsetof(SvtAmdPaLcuChroma, cr_mean) == 21, "chroma means");\n'
                   '_Static_assert(sizeof(SvtAmdPaLcuDetect) == 48 && offsetof(SvtAmdPaLcuDetect, edge_cu) == 32 && offsetof(SvtAmdPaLcuDetect, sharp_edge) == 37, "lcu");\n'
                   '_Static_assert(sizeof(SvtAmdPaPicDetect) == 8 && offsetof(SvtAmdPaPicDetect, lcu_block_percentage) == 4, "picture");\n'
                   '_Static_assert(sizeof(SvtAmdChromaJob) == 24 && sizeof(SvtAmdDetectJob) == 24, "jobs");\n'
                   '_Static_assert(sizeof(SvtAmdChromaArrays) == 4 * sizeof(void *) && sizeof(SvtAmdDetectArrays) == 2 * sizeof(void *), "arrays");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(S.ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


@pytest.mark.parametrize("w,h", [(56, 56), (200, 136), (416, 240), (1920, 1080), (3840, 2160)])
def test_bytes_per_picture_are_the_documented_sizes(lib, w, h):
    n = S.lcu_count(w, h)
    for rw, rh in ((4, 4), (1, 1), (8, 8), (3, 5)):
        got = [lib.svt_amd_chroma_stats_bytes(w, h, k, rw, rh) for k in range(4)]
        assert got == [n * 48, rw * rh * 2 * 256 * 4, 128, 16] == N.chroma_sizes(w, h, rw, rh)
    assert [lib.svt_amd_picture_detect_bytes(w, h, k) for k in range(2)] == [n * 48, 8] == N.detect_sizes(w, h)
    for which in (-1, 4, 99):
        assert lib.svt_amd_chroma_stats_bytes(w, h, which, 4, 4) == 0
    for which in (-1, 2, 99):
        assert lib.svt_amd_picture_detect_bytes(w, h, which) == 0
    for rw, rh in ((0, 4), (4, 0), (9, 8), (-1, -1)):
        assert lib.svt_amd_chroma_stats_bytes(w, h, N.CHROMA_HISTOGRAM, rw, rh) == 0


def test_bad_parameters_are_refused_without_a_device(lib):
    cj, dj = (N.ChromaJob * 1)(), (N.DetectJob * 1)()
    ca, da = N.ChromaArrays(), N.DetectArrays()
    fake = C.create_string_buffer(4096)          # never read: the job count is checked first
    refused(lib, lib.svt_amd_chroma_stats_batch_launch(None, cj, 1, 416, 240, 4, 4, C.byref(ca)), "svt_amd_chroma_stats_batch_launch")
    refused(lib, lib.svt_amd_picture_detect_batch_launch(None, dj, 1, 416, 240, C.byref(da)), "svt_amd_picture_detect_batch_launch")
    for n in (0, -1, 257, 1 << 20):
        refused(lib, lib.svt_amd_chroma_stats_batch_launch(fake, cj, n, 416, 240, 4, 4, C.byref(ca)), "svt_amd_chroma_stats_batch_launch", n)
        refused(lib, lib.svt_amd_picture_detect_batch_launch(fake, dj, n, 416, 240, C.byref(da)), "svt_amd_picture_detect_batch_launch", n)
        assert b"1..256 jobs" in lib.svt_amd_last_error()
    refused(lib, lib.svt_amd_chroma_stats_batch_launch(fake, None, 1, 416, 240, 4, 4, C.byref(ca)), "svt_amd_chroma_stats_batch_launch")
    refused(lib, lib.svt_amd_picture_detect_batch_launch(fake, dj, 1, 416, 240, None), "svt_amd_picture_detect_batch_launch")
    # ... nor for the picture's size: the bound of the kernels is tested first
    refused_as(lib, lib.svt_amd_picture_detect_batch_launch(fake, dj, 1, 0, 64, C.byref(da)), "svt_amd_picture_detect_batch_launch: job 0: a picture of 0x64 (at most 16384 LCUs)")
    refused_as(lib, lib.svt_amd_picture_detect_batch_launch(fake, dj, 1, 16384, 16384, C.byref(da)),
               "svt_amd_picture_detect_batch_launch: job 0: a picture of 16384x16384 (at most 16384 LCUs)")


@pytest.mark.parametrize("name", CASES)
def test_fixture_block_statistics_are_those_of_the_existing_path(oracle, name):
    """the luma variance / y_mean the detectors were recorded with equal what the block-statistics checker (oracle/svt_oracle_pa.c) gives for the same seeds"""
    g, kind, w, h, seed, rw, rh = load_case(name)
    for i, t in enumerate(g["picture_number"].tolist()):
        stats, _, _, _ = pa_oracle(oracle, P.padded(P.gen_luma(kind, w, h, int(t), seed)), w, h)
        assert np.array_equal(stats["variance"], g["variance"][i]) and np.array_equal(stats["y_mean"], g["y_mean"][i]), (name, t)


@pytest.mark.parametrize("name", CASES)
def test_numpy_checker_reproduces_every_array_of_the_fixture(name):
    g, kind, w, h, seed, rw, rh = load_case(name)
    assert int(g["resolution_class"][0]) == P.resolution_class(w, h)
    assert np.array_equal(N.potential_logo(w, h, int(g["resolution_class"][0])), g["potential_logo"][0])
    for i, t in enumerate(g["picture_number"].tolist()):
        what = (name, t)
        cb, cr = P.gen_chroma(kind, w, h, int(t), seed)
        means = N.chroma_means(cb, cr, w, h)
        assert np.array_equal(means["cb_mean"], g["cb_mean"][i]) and np.array_equal(means["cr_mean"], g["cr_mean"][i]), what
        hist, ravg, total = N.chroma_histograms(cb, cr, w, h, rw, rh)
        assert np.array_equal(hist, g["histogram"][i]), what
        assert np.array_equal(ravg[:rw * rh].reshape(rw, rh, 2), g["region_average"][i]) and not ravg[rw * rh:].any(), what
        assert np.array_equal(total, g["sum_chroma"][i]), what
        assert [N.average_intensity(total[c], w, h) for c in range(2)] == g["average_intensity"][i][1:].tolist(), what
        lcu, pic = N.detect(g["variance"][i], g["y_mean"][i], means, w, h, int(g["want_edge16"][i]), int(g["resolution_class"][i]))
        for field in ("var_of_var_32x32", "edge_cu", "homogeneous", "edge_block_num", "isolated_high_intensity", "sharp_edge"):
            assert np.array_equal(lcu[field], g[field][i]), what + (field, np.argwhere(lcu[field] != g[field][i])[:4].tolist())
        for field in ("pic_avg_variance", "very_low_var_pic", "logo_pic", "lcu_block_percentage"):
            assert int(pic[field]) == int(g[field][i]), what + (field,)
        assert not lcu["pad"].any() and not pic["pad"].any() and not means["pad"].any()
        assert np.array_equal(N.detect_sequential(g["variance"][i], g["y_mean"][i], w, h), g["isolated_high_intensity"][i]), what


def test_fixtures_are_not_vacuous():
    seen = {f: False for f in ("isolated_high_intensity", "sharp_edge", "edge_block_num", "edge_cu")}
    for name in CASES:
        g = load_case(name)[0]
        for f in seen:
            seen[f] |= bool(g[f].any())
    assert all(seen.values()), seen
    g = load_case("islands_704x640")[0]
    iso = g["isolated_high_intensity"][0]
    inside = [n for bx, by in P.ISLANDS_BRIGHT for n in range(iso.size) if abs(n % 11 - bx) <= 4 and abs(n // 11 - by) <= 4]
    assert any(iso[n] == 0 for n in inside) and any(iso[n] == 1 for n in inside)      # the order rule decides flags
    g = load_case("motion_416x240")[0]
    assert not g["edge_cu"][1].any() and g["edge_cu"][0].any()                          # want_edge16 0 / 1
    assert (g["var_of_var_32x32"][0][6] == np.uint64(N.ALL_ONES)).all() and not g["cb_mean"][0][6].any() and g["homogeneous"][0][6] == 1
