"""ctypes views of the batched mode-decision LCU controls (include/svt_hevc_amd.h "Batched mode-decision LCU controls"): the job, the record it writes
(SvtAmdMdLcu), the check record of a bound array, the prototypes, and the step from a job of tests/mdctl_records.py to the C job.  The numpy layouts are
svtlib.MD_LCU_DTYPE and mdctl_records.CHECK_DTYPE; tests/test_mdctl_abi.py holds the three forms - header, ctypes, numpy - against one another."""
import ctypes as C

ENTRY = "svt_amd_md_controls_batch_launch"
MDCTL_LCU = 0
MAX_LCUS = 16384
MAX_BATCH = 256                    # SVT_AMD_MAX_BATCH
u8, u16, u32 = C.c_uint8, C.c_uint16, C.c_uint32
vp = C.c_void_p


class MdCtlJob(C.Structure):
    _fields_ = [("mdc_lcu", vp), ("stats", vp), ("detect", vp), ("sbo_lcu", vp), ("sbo_pic", vp), ("irc_lcu", vp), ("ac_energy", vp), ("stationary_edge", vp),
                ("sticky", vp), ("slice_type", u8), ("depth_mode", u8), ("chroma_level", u8), ("resolution_class", u8), ("is_pan", u8), ("is_tilt", u8),
                ("color_format_422_or_444", u8), ("pad0", u8), ("tile_cols", u16), ("tile_rows", u16), ("pad", u8 * 4)]


class MdLcu(C.Structure):
    _fields_ = [("leaf_count", u8), ("leaf_index", u8 * 85), ("leaf_split", u8 * 85), ("tile_left", u8), ("tile_top", u8), ("tile_right", u8), ("is_complete", u8),
                ("complexity_status_2", u8), ("contouring_class", u8 * 4), ("chroma_encode_mode", u8), ("restrict_intra_global_motion", u8), ("lcu_md_mode", u8),
                ("skip_small_cu", u8), ("cmplx_noise", u8), ("variance_below_200", u8), ("edge_block", u8), ("no_stop_split", u8), ("pad", u8 * 3)]


class MdCtlCheck(C.Structure):
    _fields_ = [("bad_leaf_count", u32), ("bad_leaf_list", u32), ("md_mode", u32 * 16), ("bad_chroma", u32), ("tiles", u32), ("first_bad", u32), ("first_kind", u32)]


SCALAR_FIELDS = (("slice_type", "slice_type"), ("depth_mode", "depth_mode"), ("chroma_level", "chroma_level"), ("resolution_class", "cls"), ("is_pan", "pan"),
                 ("is_tilt", "tilt"), ("color_format_422_or_444", "c422"), ("tile_cols", "tile_cols"), ("tile_rows", "tile_rows"))
POINTER_FIELDS = ("mdc_lcu", "stats", "detect", "sbo_lcu", "sbo_pic", "irc_lcu", "ac_energy", "stationary_edge", "sticky")


def fill_job(j, jb, at):
    """the job of a picture: the scalars of mdctl_records.job; at(kind) -> the device address of the picture's array `kind`, or None"""
    for field, name in SCALAR_FIELDS:
        setattr(j, field, jb[name])
    for field in POINTER_FIELDS:
        setattr(j, field, at(field))
    return j


def declare(lib):
    lib.svt_amd_md_controls_batch_launch.restype = C.c_int
    lib.svt_amd_md_controls_batch_launch.argtypes = [vp, vp, C.c_int, C.c_uint16, C.c_uint16, vp]
    lib.svt_amd_md_controls_bytes.restype, lib.svt_amd_md_controls_bytes.argtypes = C.c_size_t, [C.c_uint16, C.c_uint16, C.c_int]
    lib.svt_amd_md_picture_set_controls.restype, lib.svt_amd_md_picture_set_controls.argtypes = C.c_int, [vp, vp, vp]
    lib.svt_amd_debug_md_controls_check.restype = C.c_int
    lib.svt_amd_debug_md_controls_check.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp]
    lib.svt_amd_debug_launch_markers.restype = C.c_int
    lib.svt_amd_debug_launch_markers.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.svt_amd_last_error.restype = C.c_char_p
    return lib
