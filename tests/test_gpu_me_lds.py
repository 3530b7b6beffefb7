"""-m gpu: the LDS budget of the motion-estimation search kernel as a test (four workgroups share a CU's 160 KiB when a
workgroup needs at most 40,960 B, static and dynamic together), and parity with the CPU oracle on the control combinations the
job-dependent LDS layout is most likely to break and tests/test_gpu_me.py does not hold."""
import ctypes as C

import numpy as np
import pytest

import svtlib as S
from golden_util import load_case
from gpu_util import default_params, me_picture, upload

pytestmark = pytest.mark.gpu

LDS_PER_CU = 160 * 1024


def lds_bytes(product, params, phase):
    product.svt_amd_debug_me_kernel_lds_bytes.argtypes = [C.c_void_p, C.c_int]
    product.svt_amd_debug_me_kernel_lds_bytes.restype = C.c_int
    return product.svt_amd_debug_me_kernel_lds_bytes(C.byref(params) if params is not None else None, phase)


@pytest.mark.parametrize("case", ["b_3840x2160_m7", "p_1920x1080_m9"])
def test_search_kernel_fits_four_workgroups_a_cu(product, case):
    """k_me<1> with the controls the reference encoder used (recorded fixtures): at most 160 KiB / 4 of LDS a workgroup, and the
    figure the bound is computed from is what the launcher requests (compiler's static size + the launcher's pool)."""
    g = load_case(case)
    p = S.params_from_record(g["params"][0])
    w, h = p.luma_width, p.luma_height
    want = lds_bytes(product, p, 1)
    print("%s: k_me<1> %d B, k_me<0> %d B of LDS a workgroup" % (case, want, lds_bytes(product, p, 0)))
    assert 0 < want <= LDS_PER_CU // 4
    ctx = C.c_void_p()
    assert product.svt_amd_context_create(0, w, (h + 7) & ~7, 3, C.byref(ctx)) == 0, product.svt_amd_last_error()
    try:
        for s_ in range(3):
            upload(product, ctx, s_, S.gen_luma("motion", w, h, s_, 11))
        me_picture(product, ctx, p, 1, [0, 2])
        assert lds_bytes(product, None, 1) == want
        assert lds_bytes(product, None, 0) == lds_bytes(product, p, 0)
    finally:
        product.svt_amd_context_destroy(ctx)


def test_lds_bytes_rejects_a_bad_phase(product):
    assert lds_bytes(product, default_params(640, 384), 2) == -1


CASES = [
    # two lists, SSD search method: the pool carries MeSearchSsd in front of the windows
    ("motion", 448, 328, dict(num_lists=2, temporal_layer_index=1, fractional_search_method=2, fractional_search_model=0,
                              fractional_search_64x64=1, cu8x8_mode=0)),
    ("noise", 256, 192, dict(num_lists=2, temporal_layer_index=1, fractional_search_method=2)),
    # two lists, a search width that is not a multiple of 4
    ("motion", 448, 328, dict(num_lists=2, temporal_layer_index=1, search_area_width=21, search_area_height=13, cu8x8_mode=0)),
    # partial last LCU column and row, two lists, sub-pel on every tier
    ("noise", 328, 264, dict(num_lists=2, temporal_layer_index=1, fractional_search_model=0, fractional_search_64x64=1, cu8x8_mode=0)),
    ("motion", 328, 264, dict(num_lists=2, temporal_layer_index=2, fractional_search_model=0, fractional_search_64x64=1, cu8x8_mode=0)),
    # a search area above 48 x 48 (the slow staging path of the F window), two lists
    ("motion", 448, 328, dict(num_lists=2, temporal_layer_index=1, search_area_width=75, search_area_height=70, cu8x8_mode=0)),
]


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_me_matches_oracle_on_layout_corners(product, gpu_ctx, oracle, ci):
    kind, w, h, kw = CASES[ci]
    frames = [S.gen_luma(kind, w, h, t, 31 + ci) for t in range(3)]
    for s_, f in enumerate(frames):
        upload(product, gpu_ctx, s_, f)
    pics = [S.OraclePicture(oracle, f) for f in frames]
    p = default_params(w, h, **kw)
    got = me_picture(product, gpu_ctx, p, 1, [0, 2])
    want = S.oracle_me_picture(oracle, p, pics[1], pics[0], pics[2])
    S.compare_me(got, want, 2, "%s %dx%d case %d" % (kind, w, h, ci))
    for k in S.ME_LCU_DTYPE.names:  # two lists: every field of the record is defined
        if k != "pu":
            assert np.array_equal(got[k], want[k]), k
    # (compare_me holds the candidate records: distortion / direction up to each PU's candidate count, which is all the reference defines)
    assert np.array_equal(got["pu"]["mv"], want["pu"]["mv"]) and np.array_equal(got["pu"]["total"], want["pu"]["total"])
