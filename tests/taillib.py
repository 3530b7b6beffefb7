"""ctypes views and prototypes of the picture tail on the device (include/svt_hevc_amd.h "Picture tail on the device"); tests/test_tail_abi.py holds them against
the header."""
import ctypes as C

import numpy as np

import svtlib as S
import tail_numpy as N
from test_oracle_saodec_golden import DEC, LCU

ENTRY = "svt_amd_encdec_picture_tail_launch"
WARMUP_ENTRY = "svt_amd_encdec_picture_tail_warmup"
DEBUG_ENTRY = "svt_amd_debug_picture_tail_maps"
LCU_PARAMS, CHECK = 0, 1           # SVT_AMD_TAIL_LCU_PARAMS, SVT_AMD_TAIL_CHECK
u8, u16, u32, u64, i8 = C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64, C.c_int8
vp = C.c_void_p
LIST_BYTES = 1584                  # head + unit list of a work record
RESULT_CU_BYTES = 768              # SvtAmdLcuResult.cu


class DeblockParams(C.Structure):
    _fields_ = [("tc_offset", i8), ("beta_offset", i8), ("cb_qp_offset", i8), ("cr_qp_offset", i8), ("slice_type", u8), ("pad", u8 * 3), ("ref_poc", u64 * 2)]


class SaoDecisionParams(C.Structure):
    _fields_ = [("lambda_", u64), ("chroma_lambda", u64), ("type_bits", u32 * 6), ("merge_bits", u32 * 2), ("offset_bits", u32 * 8), ("is_10bit", u8), ("mm_sao", u8),
                ("temporal_layer", u8), ("pad", u8)]


class TailJob(C.Structure):
    _fields_ = [("d_works", vp), ("work_stride", C.c_size_t), ("d_results", vp), ("result_stride", C.c_size_t), ("d_sao_enable", vp), ("deblock", DeblockParams),
                ("sao", SaoDecisionParams), ("origin_x", u32), ("origin_y", u32), ("stages", u32), ("pad", u32)]


class TailCheck(C.Structure):
    _fields_ = [("bad_lcus", u32), ("first_bad_lcu", u32), ("bad_units", u32), ("first_bad_unit_lcu", u32)]


class CuMapEntry(C.Structure):
    _fields_ = [("mode", u8), ("dir", u8), ("size_log2", u8), ("pad", u8), ("mv", (C.c_int16 * 2) * 2)]


assert C.sizeof(SaoDecisionParams) == DEC.itemsize == 88 and C.sizeof(TailCheck) == N.CHECK_DTYPE.itemsize == 16 and C.sizeof(CuMapEntry) == N.CU_MAP_DTYPE.itemsize == 12


def job(d_works, work_stride, d_results, result_stride, stages, slice_type=2, ref_poc=(0, 0), sao=None, d_enable=None, origin=(0, 0)):
    """sao: a DEC record (test_oracle_saodec_golden.params_of) or None"""
    j = TailJob()
    j.d_works, j.work_stride, j.d_results, j.result_stride, j.stages, j.d_sao_enable = d_works, work_stride, d_results, result_stride, stages, d_enable
    j.deblock.slice_type, j.deblock.ref_poc[0], j.deblock.ref_poc[1] = slice_type, int(ref_poc[0]), int(ref_poc[1])
    if sao is not None:
        raw = np.ascontiguousarray(sao).view(np.uint8).reshape(-1)[:88]
        C.memmove(C.addressof(j.sao), raw.ctypes.data, 88)
    j.origin_x, j.origin_y = origin
    return j


def declare(lib):
    lib.svt_amd_picture_tail_bytes.restype, lib.svt_amd_picture_tail_bytes.argtypes = C.c_size_t, [u16, u16, C.c_int]
    lib.svt_amd_encdec_picture_tail_launch.restype, lib.svt_amd_encdec_picture_tail_launch.argtypes = C.c_int, [vp, vp, vp, vp, vp, vp]
    lib.svt_amd_encdec_picture_tail_warmup.restype, lib.svt_amd_encdec_picture_tail_warmup.argtypes = C.c_int, [vp, vp, u32, u32]
    lib.svt_amd_debug_picture_tail_maps.restype, lib.svt_amd_debug_picture_tail_maps.argtypes = C.c_int, [vp] * 10
    for f in (lib.svt_amd_encode_picture_device, lib.svt_amd_encode_picture_device16):
        f.restype, f.argtypes = C.c_int, [vp, vp, vp, vp, C.c_int]
    for f in (lib.svt_amd_encode_picture_device_inter, lib.svt_amd_encode_picture_device_inter16):
        f.restype, f.argtypes = C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int]
    lib.svt_amd_last_error.restype = C.c_char_p
    return lib


def cbf0_of(results):
    """[lcus][64]: the luma cbf of every result slot"""
    return np.ascontiguousarray(results["cu"]["cbf"][:, :, 0])


def malformed_cases(rng_heads):
    """the records the host loops refuse, made from one valid picture of 128x64 (two LCUs, `rng_heads`): name -> (heads, expected check record as a tuple)"""
    out = {}
    NONE = N.NONE

    def fresh():
        return rng_heads.copy()
    h = fresh()
    h[1]["lcu_x"] = 0
    out["an LCU at the wrong position"] = (h, (1, 1, 0, NONE))
    h = fresh()
    h[0]["cu"][0]["size"] = 4
    out["size 4"] = (h, (0, NONE, 1, 0))
    h = fresh()
    h[1]["cu"][0]["x"], h[1]["cu"][0]["size"] = 56, 16
    out["x + size > 64"] = (h, (0, NONE, 1, 1))
    h = fresh()
    h[0]["num_cus"] = 65
    out["num_cus 65"] = (h, (1, 0, 0, NONE))
    return out


def outside_case(heads_200x136):
    """a unit outside the picture: the last LCU of a 200x136 picture (8 samples wide and high inside it) with one 16x16 unit"""
    h = heads_200x136.copy()
    h[-1]["num_cus"] = 1
    h[-1]["cu"][0]["x"], h[-1]["cu"][0]["y"], h[-1]["cu"][0]["size"] = 0, 0, 16
    return h, (0, N.NONE, 1, len(h) - 1)
