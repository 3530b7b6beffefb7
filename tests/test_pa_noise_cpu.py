"""CPU-only: the C-ABI of the batched noise detection (include/svt_hevc_amd.h "Batched noise detection") - the two entries are exported, the size helper and
the record layouts are the documented ones - and the numpy restatement (tests/pa_noise_numpy.py) against what the REFERENCE's PicturePreProcessingOperations
computed on seeded pictures (tests/golden/panoise_*.npz, tests/golden/make_pa_noise_golden.py): every field."""
import ctypes as C
import glob
import json
import os
import subprocess

import numpy as np
import pytest

import pa_noise_numpy as N
import pa_noise_pictures as P
import svtlib as S
from abi_util import exported, open_library
from pa_batch_util import refused

CASES = sorted(os.path.basename(p)[8:-4] for p in glob.glob(os.path.join(S.GOLDEN_DIR, "panoise_*.npz")))


def load_case(name):
    """-> (fixture, method, width, height, picture specifications)"""
    g = np.load(os.path.join(S.GOLDEN_DIR, "panoise_%s.npz" % name))
    assert str(g["case"][0]) == name
    return g, int(g["case"][1]), int(g["case"][2]), int(g["case"][3]), json.loads(str(g["specs"]))


@pytest.fixture(scope="module")
def lib():
    return open_library(N.declare)


def test_have_the_eight_cases():
    assert CASES == sorted(P.CASES)
    for name in CASES:
        g, method, w, h, specs = load_case(name)
        assert (method, w, h) == P.CASES[name] and specs == P.case_specs(name)
        assert "C_DEFAULT (ASM_TYPES 0)" in g["paths"].tolist()


def test_entries_are_exported():
    assert {"svt_amd_noise_detect_batch_launch", "svt_amd_noise_detect_bytes"} <= exported()


def test_record_layouts(tmp_path):
    assert N.PIC_DTYPE.itemsize == 16 and N.PIC_DTYPE.fields["block_count"][1] == 8 and N.PIC_DTYPE.fields["pic_noise_class"][1] == 12
    assert C.sizeof(N.NoiseJob) == 8 and C.sizeof(N.NoiseArrays) == 2 * C.sizeof(C.c_void_p)
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "svt_hevc_amd.h"\n'
                   '_Static_assert(sizeof(SvtAmdNoisePic) == 16 && offsetof(SvtAmdNoisePic, block_count) == 8 && offsetof(SvtAmdNoisePic, pic_noise_class) == 12, "picture");\n'
                   '_Static_assert(sizeof(SvtAmdNoiseJob) == 8 && offsetof(SvtAmdNoiseJob, method) == 4 && offsetof(SvtAmdNoiseJob, noise_detection_th) == 5, "job");\n'
                   '_Static_assert(sizeof(SvtAmdNoiseArrays) == 2 * sizeof(void *), "arrays");\n'
                   '_Static_assert(SVT_AMD_NOISE_HALF == 0 && SVT_AMD_NOISE_QUARTER == 1 && SVT_AMD_NOISE_FULL == 2, "EB_NOISE_DETECT_MODE");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(S.ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])
    assert (N.HALF, N.QUARTER, N.FULL) == (P.HALF, P.QUARTER, P.FULL) == (0, 1, 2)


@pytest.mark.parametrize("w,h,lcus", [(64, 64, 1), (200, 136, 12), (704, 640, 110), (256, 1152, 72), (1920, 1080, 510), (3840, 2160, 2040), (4096, 64, 64), (4160, 64, 65)])
def test_bytes_per_picture_are_the_documented_sizes(lib, w, h, lcus):
    assert N.lcu_count(w, h) == lcus
    rounded = (lcus + 63) // 64 * 64
    assert [lib.svt_amd_noise_detect_bytes(w, h, k) for k in range(2)] == [rounded, 16] == N.sizes(w, h)
    for which in (-1, 2, 99):
        assert lib.svt_amd_noise_detect_bytes(w, h, which) == 0


def test_bad_parameters_are_refused_without_a_device(lib):
    jobs, arrays = (N.NoiseJob * 1)(), N.NoiseArrays()
    fake = C.create_string_buffer(4096)          # never read: the job count is checked first
    refused(lib, lib.svt_amd_noise_detect_batch_launch(None, jobs, 1, C.byref(arrays)), "svt_amd_noise_detect_batch_launch")
    for n in (0, -1, 257, 1 << 20):
        refused(lib, lib.svt_amd_noise_detect_batch_launch(fake, jobs, n, C.byref(arrays)), "svt_amd_noise_detect_batch_launch", n)
        assert b"1..256 jobs" in lib.svt_amd_last_error()
    refused(lib, lib.svt_amd_noise_detect_batch_launch(fake, None, 1, C.byref(arrays)), "svt_amd_noise_detect_batch_launch")
    refused(lib, lib.svt_amd_noise_detect_batch_launch(fake, jobs, 1, None), "svt_amd_noise_detect_batch_launch")


@pytest.mark.parametrize("name", CASES)
def test_numpy_checker_reproduces_every_field_of_the_fixture(name):
    g, method, w, h, specs = load_case(name)
    lcus = N.lcu_count(w, h)
    assert g["flat_noise"].shape == (len(specs), 2, lcus)
    for i, s in enumerate(specs):
        luma = P.picture(w, h, s)
        blocks = N.block_variances(luma, method)
        for th in (0, 1):
            what = (name, i, th)
            flat, pic = N.detect(luma, method, th, blocks=blocks)
            assert np.array_equal(flat[:lcus], g["flat_noise"][i, th]) and not flat[lcus:].any(), what + (np.argwhere(flat[:lcus] != g["flat_noise"][i, th])[:4].tolist(),)
            assert int(pic["noise_variance_sum"]) == int(g["noise_variance_sum"][i, th]), what
            assert int(pic["block_count"]) == int(g["block_count"][i, th]), what
            assert int(pic["pic_noise_class"]) == int(g["pic_noise_class"][i, th]), what
            assert N.variance_float(pic) == float(g["noise_variance_float"][i, th]), what      # picNoiseVarianceFloat, exactly, from the two integers
            assert not pic["pad"].any()


def test_fixtures_are_not_vacuous():
    """what tests/golden/make_pa_noise_golden.py asserts when it writes them, read back from the files"""
    classes = {m: set() for m in (P.HALF, P.QUARTER, P.FULL)}
    mixed = threshold = folded = stacked = False
    for name in CASES:
        g, method, w, h, specs = load_case(name)
        wl = (w + 63) // 64
        classes[method] |= set(int(c) for c in g["pic_noise_class"].reshape(-1))
        f = g["flat_noise"]
        threshold |= bool((f[:, 0] != f[:, 1]).any())
        value = g["noise_variance_sum"] // np.maximum(g["block_count"], 1)
        if method == P.FULL:
            high = value >= 20 + (25 if h <= 720 else 0)
            assert (g["pic_noise_class"][high] == 4).all()
            folded |= bool(high.any())
            done = np.zeros(f.shape[2], bool).reshape(-1, wl)
            done[:h // 64, :w // 64] = True
        else:
            step, per = (4, 4) if method == P.HALF else (2, 2)
            done = np.zeros(f.shape[2], bool).reshape(-1, wl)
            done[:(h // step // 64) * per, :(w // step // 64) * per] = True
            tx, ty = P.TEXTURED
            if done.shape[0] > ty and done[ty, tx] and (ty - 1) // per == ty // per:
                # the textured LCU and the plain one above it: one 64x64 block, ONE noise variance, different denoised variances
                stacked |= bool((f[:, 1, (ty - 1) * wl + tx] != f[:, 1, ty * wl + tx]).any())
        done = done.reshape(-1)
        assert not f[:, :, ~done].any(), name
        assert (g["block_count"] == done.sum()).all(), name
        ev = f[:, :, done]
        mixed |= bool((ev.any(axis=2) & ~ev.all(axis=2)).any()) if done.any() else False
    assert all(c == {1, 2, 3, 4} for c in classes.values()), classes
    assert mixed and threshold and folded and stacked
    g, method, w, h, specs = load_case("half_64x64")
    assert not g["block_count"].any() and not g["noise_variance_sum"].any() and (g["pic_noise_class"] == 1).all() and not g["flat_noise"].any()


def test_the_shared_noise_strip_decides_flags():
    """half 704x640, background amplitude 9: the clean LCU (1, 1) is flat noise because it is judged with the noise variance of LCU (1, 0) above it - the rows the
    reference's one-strip noise picture holds at offset 0 (:3127).  Judged with its own rows it would not be."""
    g, method, w, h, specs = load_case("half_704x640")
    i = [s["amp"] for s in specs].index(9)
    luma = P.picture(w, h, specs[i])
    flat, _ = N.detect(luma, method, 1)
    own, _ = N.detect(luma, method, 1, own_rows=True)
    assert flat[11 + 1] == 1 and own[11 + 1] == 0 and g["flat_noise"][i, 1, 11 + 1] == 1
