"""GPU: the intra reference of the encode pass (ep_intra_predict_plane in svt-hevc_amd/csrc/encdec_device.h, run by svt_amd_encode_lcus[16]) on designed
neighbourhoods.  svt_amd_encdec_picture_put_borders[16] writes the last row, last column and edge mode types of host-encoded LCUs into the device picture, which
fixes every sample and mode type the unit at (0, 0) of a device-encoded LCU reads; the oracle gets the same samples written into rec[] and its mode map
(tests/intra_ref_extremes.py).  That the cases sit on the decisions they are named for is shown on the CPU: tests/test_intra_ref_extremes_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import intra_ref_extremes as X
import svtlib as S
from test_gpu_encodepass import encode, sig
from test_oracle_encodepass_golden import compare_lcu

pytestmark = pytest.mark.gpu

FAMILIES = {"threshold grid": X.grid_cases, "size gate": X.gate_cases, "constrained-intra masks": X.mask_cases}


@pytest.mark.parametrize("bps", [1, 2])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_encode_lcus_on_designed_neighbourhoods_match_oracle(product, oracle, gpu_ctx, family, bps):
    """one picture, one svt_amd_encdec_picture_put_borders call and one svt_amd_encode_lcus call per family and depth: every device LCU has host-encoded LCUs to
    its left, top-left, top and top-right.  Threshold grid: tl = mid = base on both sides of a 32x32 unit, the far ends at base + d, d in {-thr, -(thr-1),
    thr-1, thr} in all 16 pairs, filtered and unfiltered modes, the flag clear where it matters.  Size gate: the same pins on 16x16 units.  Masks: constrained
    intra with every group inter, one group left, alternating groups, the left side flat by substitution, seeded random masks - and each again as a control"""
    lib = product
    sig(lib)
    cases = FAMILIES[family](bps)
    P = X.picture(oracle, cases)
    assert len(P["works"]) == len(cases) <= 1024 and len(P["borders"]) <= 4096
    put = lib.svt_amd_encdec_picture_put_borders16 if P["wide"] else lib.svt_amd_encdec_picture_put_borders
    pic = C.c_void_p()
    assert lib.svt_amd_encdec_picture_create(gpu_ctx, P["w"], P["h"], bps, C.byref(pic)) == 0, lib.svt_amd_last_error()
    try:
        assert lib.svt_amd_encdec_picture_begin(gpu_ctx, pic) == 0
        borders = np.ascontiguousarray(P["borders"])
        assert put(gpu_ctx, pic, borders.ctypes.data, len(borders)) == 0, lib.svt_amd_last_error()
        got = encode(lib, gpu_ctx, pic, P["works"])
        for c, wk, want, r in zip(cases, P["works"], P["want"], got):
            compare_lcu(wk, want, r, P["w"], P["h"], (family, bps) + tuple(c["tag"]))
    finally:
        lib.svt_amd_encdec_picture_destroy(gpu_ctx, pic)
