"""ctypes views and numpy layouts of the temporal motion field on the device (include/svt_hevc_amd.h "Temporal motion field on the device"): the job, the
statistics record, the field record (SvtAmdTmvpLcu), the part of a work record the producer reads (head + unit list) and the prototypes.
tests/test_tmvp_abi.py holds the three forms - header, ctypes, numpy - against one another."""
import ctypes as C
import os

import numpy as np

import svtlib as S

ENTRY = "svt_amd_motion_field_launch"
PICTURE_ENTRY = "svt_amd_encdec_picture_motion_field"
BIND_ENTRY = "svt_amd_md_picture_set_motion_field"
FIELD, STATS = 0, 1                # SVT_AMD_MOTION_FIELD, SVT_AMD_MOTION_FIELD_STATS
MAX_LCUS = 16384                   # SVT_AMD_MDCTL_MAX_LCUS
u8, u16, u32, u64, i16 = C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64, C.c_int16
vp = C.c_void_p


class MotionFieldJob(C.Structure):
    _fields_ = [("d_works", vp), ("work_stride", C.c_size_t), ("width", u16), ("height", u16), ("slice_type", u8), ("pad", u8 * 3), ("ref_poc", u64 * 2)]


class RefStats(C.Structure):
    _fields_ = [("intra_area_sum", u32), ("intra_coded_area", u8), ("pad", u8 * 3)]


class TmvpLcu(C.Structure):
    _fields_ = [("mv", ((i16 * 2) * 16) * 2), ("ref_poc", (u64 * 16) * 2), ("pred_dir", u8 * 16), ("available", u8 * 16)]


class LcuCu(C.Structure):
    _fields_ = [("x", u8), ("y", u8), ("size", u8), ("pred_mode", u8), ("intra_luma_mode", u8), ("bottom_left_ok", u8), ("top_right_ok", u8), ("qp", u8),
                ("chroma_qp", u8), ("leaf_index", u8), ("inter_dir", u8), ("inter_kind", u8), ("dz_offset", u32), ("mv", (i16 * 2) * 2)]


class LcuWorkHead(C.Structure):
    """SvtAmdLcuWork / SvtAmdLcuWork16 up to the source samples: all the producer reads"""
    _fields_ = [("lcu_x", u16), ("lcu_y", u16), ("num_cus", u8), ("slice_type", u8), ("temporal_layer", u8), ("constrained_intra", u8), ("strong_smoothing", u8),
                ("tile_left", u8), ("tile_top", u8), ("tile_right", u8), ("pad", u8 * 4), ("full_lambda", u32), ("luma_cbf_bits", u32 * 4), ("pm_core", u8),
                ("pad2", u8 * 11), ("cu", LcuCu * 64)]


REF_STATS_DTYPE = np.dtype([("intra_area_sum", "<u4"), ("intra_coded_area", "u1"), ("pad", "u1", 3)])
TMVP_LCU_DTYPE = S.MD_TMVP_LCU_DTYPE
# the head of svtlib.LCU_WORK_DTYPE / LCU_WORK16_DTYPE: every field in front of src_y
WORK_HEAD_DTYPE = np.dtype([(n, S.LCU_WORK_DTYPE.fields[n][0]) for n in S.LCU_WORK_DTYPE.names[:S.LCU_WORK_DTYPE.names.index("src_y")]])
HEAD_BYTES = 48                    # in front of cu[]
LIST_BYTES = 1584                  # head + unit list
WORK_BYTES = S.LCU_WORK_DTYPE.itemsize
WORK16_BYTES = LIST_BYTES + 2 * (4096 + 2 * 1024)
assert WORK_HEAD_DTYPE.itemsize == LIST_BYTES and WORK_HEAD_DTYPE.fields["cu"][1] == HEAD_BYTES and WORK_BYTES == LIST_BYTES + 6144


def job(d_works, stride, w, h, slice_type, ref_poc=(0, 0)):
    j = MotionFieldJob()
    j.d_works, j.work_stride, j.width, j.height, j.slice_type = d_works, stride, w, h, slice_type
    j.ref_poc[0], j.ref_poc[1] = int(ref_poc[0]), int(ref_poc[1])
    return j


def declare(lib):
    lib.svt_amd_motion_field_bytes.restype, lib.svt_amd_motion_field_bytes.argtypes = C.c_size_t, [u16, u16, C.c_int]
    lib.svt_amd_motion_field_launch.restype, lib.svt_amd_motion_field_launch.argtypes = C.c_int, [vp, vp, vp, vp]
    lib.svt_amd_encdec_picture_motion_field.restype = C.c_int
    lib.svt_amd_encdec_picture_motion_field.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    lib.svt_amd_md_picture_set_motion_field.restype, lib.svt_amd_md_picture_set_motion_field.argtypes = C.c_int, [vp, vp, vp]
    lib.svt_amd_md_picture_set_controls.restype, lib.svt_amd_md_picture_set_controls.argtypes = C.c_int, [vp, vp, vp]
    lib.svt_amd_last_error.restype = C.c_char_p
    return lib


CASES = ("b_objects_416x240_m8", "p_objects_320x192_m8_ld", "b_xc_binary_200x136_m8_q51", "bref_tiles_motion_640x384_m8", "b_noise_320x256_m9_q24")
# the mode-decision fixtures that pair up: reference B picture q of md_bref_<name> is the co-located picture of non-reference B picture p of md_b_<name>
MD_PAIRS = (("motion_416x240_m8", ((2, 3), (4, 5), (6, 7))), ("noise_320x256_m9_q24", ((2, 3), (4, 5), (6, 7))), ("objects_640x360_m9_q36", ((2, 3),)),
            ("xc_binary_200x136_m8_q51", ((4, 5), (6, 7))), ("forced_static_416x240_m8", ((2, 3), (4, 5), (6, 7))))


def load_case(name):
    return np.load(os.path.join(S.GOLDEN_DIR, "tmvp_%s.npz" % name))
