"""GPU: the motion-vector candidate lists the P / B unit loop executes (svt-hevc_amd/csrc/md_lists.h: md_list_consts, md_tmvp_position, md_amvp_one_list,
md_temporal_mvp_dev, md_merge_list_regs, md_choose_mvp_one - the REGISTER form of the lists, a second text beside md_logic.h's) against what the reference's own
GenerateL0L1AmvpMergeLists and ChooseMVPIdx_V2 answered on the seeded jobs of tests/golden/mvlists_seeded.npz: POC distances beyond the +-128 clips, scale factors
and scaled components at their clips, co-located list 1, no motion field, ClipMV at the far corner of 4096 x 2304 pictures.  svt_amd_debug_md_lists_batch runs those
__device__ functions on one job per lane.  Neither the reference nor oracle/_ref is needed here; tests/test_oracle_mvlists.py pins the fixture and the CPU text."""
import ctypes as C
import os

import numpy as np
import pytest

import mvlists_jobs as J
import svtlib as S

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def fixture():
    g = np.load(os.path.join(S.GOLDEN_DIR, "mvlists_seeded.npz"))
    return np.ascontiguousarray(g["jobs"]), np.ascontiguousarray(g["pool"]), g["outs"]


@pytest.fixture(scope="module")
def dev(product, gpu_ctx, fixture):
    """the jobs and the pool on the device, room for the outs and one record more behind them"""
    jobs, pool, _ = fixture
    assert int(jobs["pool"].max()) < len(pool)      # the entry cannot check device-resident indices
    product.svt_amd_debug_md_lists_batch.restype = C.c_int
    product.svt_amd_debug_md_lists_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    ptrs = []
    for nbytes in (jobs.nbytes, pool.nbytes, (len(jobs) + 1) * J.OUT_DTYPE.itemsize):
        p = C.c_void_p()
        assert product.svt_amd_device_alloc(gpu_ctx, nbytes, C.byref(p)) == 0, product.svt_amd_last_error()
        ptrs.append(p)
    assert product.svt_amd_device_upload(gpu_ctx, ptrs[0], jobs.ctypes.data, jobs.nbytes) == 0, product.svt_amd_last_error()
    assert product.svt_amd_device_upload(gpu_ctx, ptrs[1], pool.ctypes.data, pool.nbytes) == 0, product.svt_amd_last_error()
    yield ptrs
    for p in ptrs:
        product.svt_amd_device_free(gpu_ctx, p)


def run(product, gpu_ctx, dev, n_total, launches):
    """launches: (first job, count) each; the outs array starts as SENTINEL bytes.  -> the n_total + 1 records"""
    d_jobs, d_pool, d_outs = dev
    host = np.full((n_total + 1) * J.OUT_DTYPE.itemsize, SENTINEL, np.uint8)
    assert product.svt_amd_device_upload(gpu_ctx, d_outs, host.ctypes.data, host.nbytes) == 0, product.svt_amd_last_error()
    for first, count in launches:
        rc = product.svt_amd_debug_md_lists_batch(gpu_ctx, C.c_void_p(d_jobs.value + first * J.JOB_DTYPE.itemsize), d_pool,
                                                  C.c_void_p(d_outs.value + first * J.OUT_DTYPE.itemsize), count)
        assert rc == 0, product.svt_amd_last_error()
    assert product.svt_amd_synchronize(gpu_ctx) == 0, product.svt_amd_last_error()
    assert product.svt_amd_device_download(gpu_ctx, host.ctypes.data, d_outs, host.nbytes) == 0, product.svt_amd_last_error()
    return host.view(J.OUT_DTYPE)


@pytest.fixture(scope="module")
def one_launch(product, gpu_ctx, dev, fixture):
    return run(product, gpu_ctx, dev, len(fixture[0]), [(0, len(fixture[0]))])


def test_device_lists_equal_reference_records(fixture, one_launch):
    jobs, _, outs = fixture
    J.compare_outs(jobs, one_launch[:len(jobs)], outs, "svt_amd_debug_md_lists_batch against the reference's records")


def test_nothing_written_behind_the_last_out(fixture, one_launch):
    n = len(fixture[0])
    assert (one_launch[n:].view(np.uint8) == SENTINEL).all()
    assert (one_launch[:n]["pad"] == 0).all()       # every byte of an out is written: the sentinel is gone from the padding too


def test_split_launches_give_the_same_bytes(product, gpu_ctx, dev, fixture, one_launch):
    """launches of 1, 63, 65 jobs and the remainder: the entry's own tail handling (a wave is 64 lanes)"""
    n = len(fixture[0])
    got = run(product, gpu_ctx, dev, n, [(0, 1), (1, 63), (64, 65), (129, n - 129)])
    assert got.tobytes() == one_launch.tobytes()
    # a short launch leaves everything behind its last job alone
    part = run(product, gpu_ctx, dev, n, [(0, 65)])
    assert part[:65].tobytes() == one_launch[:65].tobytes() and (part[65:].view(np.uint8) == SENTINEL).all()


def test_refusals(product, gpu_ctx, dev):
    d_jobs, d_pool, d_outs = dev
    host = np.full(4 * J.OUT_DTYPE.itemsize, SENTINEL, np.uint8)
    assert product.svt_amd_device_upload(gpu_ctx, d_outs, host.ctypes.data, host.nbytes) == 0
    f = product.svt_amd_debug_md_lists_batch
    for args in ((None, d_jobs, d_pool, d_outs, 4), (gpu_ctx, None, d_pool, d_outs, 4), (gpu_ctx, d_jobs, None, d_outs, 4), (gpu_ctx, d_jobs, d_pool, None, 4),
                 (gpu_ctx, d_jobs, d_pool, d_outs, 0)):
        assert f(*args) == -1                       # SVT_AMD_ERR_BAD_PARAM
        assert b"svt_amd_debug_md_lists_batch" in product.svt_amd_last_error()
    assert product.svt_amd_synchronize(gpu_ctx) == 0
    back = np.zeros_like(host)
    assert product.svt_amd_device_download(gpu_ctx, back.ctypes.data, d_outs, back.nbytes) == 0
    assert (back == SENTINEL).all()                 # nothing was queued
