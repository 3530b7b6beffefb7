"""GPU: the device mode decision of P / B pictures coded WITHOUT sub-sample search (SvtAmdMdInter.use_subpel == 0: encMode 9 at the 4K input class, temporal layers above
0) - the candidates of the motion estimation rounded to whole samples at their injection, the merge candidates predicted at the rounded position, prediction through the
reference's interpolation-free path (luma copy, NEAREST chroma sample, the average of two copies) - against the REFERENCE's own ModeDecisionLcu records of two whole
2688x1024 pictures (tests/golden/mdifree_*.npz, tests/golden/make_md_ifree_golden.py): a layer-2 picture (CHROMA_MODE_BEST LCUs: the chroma of the winning merge candidate
behind the decisions) and a layer-1 picture (CHROMA_MODE_FULL LCUs: chroma in both loops).  The blocking entry, the stream-ordered launch on device inputs against it, and
the refusal of the 16-bit entries.  The CPU checker is not run on these pictures: its prediction (oracle/) holds the filters only - the reference's records are the yardstick."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import mdlaunchlib as M
import svtlib as S
from pa_batch_util import BAD_PARAM, ok
from test_gpu_md_launch import World, launched, lib, tiles_of  # noqa: F401  (lib: the module's fixture of the declared library)
from test_gpu_mdctl_batch import same_call
from test_oracle_md_golden import compare_kinds, compare_md

pytestmark = pytest.mark.gpu
FIXTURES = sorted(glob.glob(os.path.join(S.GOLDEN_DIR, "mdifree_*.npz")))
NAMES = [os.path.basename(f)[:-4] for f in FIXTURES]
RESULTS = {}                           # fixture -> (the blocking call's three arrays, the launch's), computed once


def both_entries(lib, path):
    """the launch on a fresh object, then the blocking call on the same object (tests/test_gpu_md_launch.py case_one's order: nothing of a blocking call can be left in
    the arrays the launch wrote)"""
    if path not in RESULTS:
        g = np.load(path)
        world = World(lib, g, 0, 1)
        inp = world.inputs()
        try:
            got, st = launched(lib, world, inp)
            assert st.check.first_bad == 0xFFFFFFFF
            rc, want = world.call(host=world.lcus)
            assert rc == 0, lib.svt_amd_last_error()
            RESULTS[path] = (want, got)
        finally:
            inp.free()
            world.free()
    return RESULTS[path]


def test_there_are_two_recorded_pictures():
    assert len(FIXTURES) == 2, FIXTURES


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_the_blocking_entry_decides_what_the_reference_decided(lib, path):
    """every field of every leaf the reference tested (split, mode, luma cbf, direction, merge flag and index, vectors - a merge unit KEEPS its fractional vector -, cost,
    merge and skip cost), and in the work records of the encode pass the final trees' vectors, directions and merge / skip decisions (for the layer-2 picture made by
    AddChromaEncDec's chroma of the winning merge candidate, predicted at the rounded position)"""
    g = np.load(path)
    assert int(g["inter"][0]["use_subpel"]) == 0
    want, _ = both_entries(lib, path)
    tag = os.path.basename(path)
    out = np.frombuffer(want[0], S.MD_LCU_OUT_DTYPE)
    ref_out, ref_kinds = g["out"][0], g["ep_kind"][0]                          # (read once: every access to a member of the file decompresses it)
    compare_md(out, ref_out, tag)
    works = np.frombuffer(want[1], S.LCU_WORK_DTYPE)
    kinds = np.full((len(works), 85), 0xFF, np.uint8)
    for i in range(len(works)):
        n = int(works[i]["num_cus"])
        cu = works[i]["cu"][:n]
        inter = cu["pred_mode"] == 1
        kinds[i, cu["leaf_index"][inter]] = cu["inter_kind"][inter]
        assert np.array_equal(cu["mv"][inter], ref_out[i]["mv"][cu["leaf_index"][inter]]), (tag, i)
        assert np.array_equal(cu["inter_dir"][inter], ref_out[i]["inter_dir"][cu["leaf_index"][inter]]), (tag, i)
    compare_kinds(kinds, ref_kinds, tag)


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_the_launch_on_device_inputs_equals_the_blocking_entry(lib, path):
    """decisions (every byte the call defines, tests/test_gpu_mdctl_batch.py decisions), work records and results of the encode pass: byte for byte; and the launch's
    decisions are the reference's by themselves"""
    g = np.load(path)
    want, got = both_entries(lib, path)
    same_call(want, got, os.path.basename(path))
    compare_md(np.frombuffer(got[0], S.MD_LCU_OUT_DTYPE), g["out"][0], os.path.basename(path) + " (launch)")


def test_the_16_bit_entries_refuse_the_picture_and_say_why(lib):
    """UnpackUniPredRef10Bit / UnpackBiPredRef10Bit - the interpolation-free prediction from 10-bit reference pictures - is a path of its own: both 16-bit entries refuse,
    name the flag, and write nothing"""
    g = np.load(FIXTURES[0])
    world = World(lib, g, 0, 2)
    inp = world.inputs()
    try:
        rc, arrays = world.call(host=world.lcus)
        text = lib.svt_amd_last_error()
        assert rc == BAD_PARAM and text.startswith(b"svt_amd_md_encode_picture_inter16: use_subpel 0"), (rc, text)
        assert all((np.frombuffer(a, np.uint8) == 0xA5).all() for a in arrays)
        rc = M.launch(lib, world.ctx, world.pic, M.make_job(world, inp, tiles_of(world.lcus)), inp)
        text = lib.svt_amd_last_error()
        assert rc == BAD_PARAM and text.startswith(b"svt_amd_md_encode_picture_launch: use_subpel 0"), (rc, text)
        ok(lib, lib.svt_amd_synchronize(world.ctx))
        # with the flag set the same object takes the same picture (what the refusal turns on, nothing else)
        world.X = world.X.copy()
        world.X["use_subpel"] = 1
        rc, _ = world.call(host=world.lcus)
        assert rc == 0, lib.svt_amd_last_error()
    finally:
        inp.free()
        world.free()
