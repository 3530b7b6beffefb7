"""ctypes views of the batched mode-decision configuration (include/svt_hevc_amd.h "Batched mode-decision configuration"): the job, the two records and the
array table, the prototypes, and the step from a job of tests/mdc_records.py to the C job.  The numpy layouts of the records are mdc_records.MDC_LCU_DTYPE and
MDC_PIC_DTYPE; tests/test_mdc_abi.py holds the three forms - header, ctypes, numpy - against one another."""
import ctypes as C

import mdc_records as R

ENTRY = "svt_amd_md_config_batch_launch"
MDC_LCU, MDC_PICTURE = 0, 1
MAX_LCUS = 13854
MAX_BATCH = 256                    # SVT_AMD_MAX_BATCH
u8, i8, u32 = C.c_uint8, C.c_int8, C.c_uint32


class MdcJob(C.Structure):
    _fields_ = [("me", C.c_void_p), ("stats", C.c_void_p), ("detect", C.c_void_p), ("sbo_lcu", C.c_void_p), ("sbo_pic", C.c_void_p), ("pic_detect", C.c_void_p),
                ("noise_pic", C.c_void_p), ("stationary_edge", C.c_void_p), ("cur_slot", C.c_int32), ("slice_type", u8), ("temporal_layer_index", u8),
                ("hierarchical_levels", u8), ("is_used_as_reference", u8), ("depth_mode", u8), ("enc_mode", u8), ("resolution_class", u8), ("qp", u8), ("is_pan", u8),
                ("is_tilt", u8), ("noise_detection_th", u8), ("homogeneity_percentage", u8), ("frame_rate_30", u8), ("cu8x8_mode", u8), ("average_intensity", u8),
                ("ref_average_intensity", u8 * 2), ("ref_intra_coded_area", u8 * 2), ("ref_temporal_layer", u8 * 2), ("ref_penalize_skip", u8 * 2), ("pad", u8),
                ("lambda_sad", u32), ("split_flag_bits", u32 * 2)]


class MdcLcu(C.Structure):
    _fields_ = [("leaf_count", u8), ("leaf_index", u8 * 85), ("leaf_split", u8 * 85), ("lcu_md_mode", u8), ("aura_status", u8), ("pred64", u8), ("avc_partitioning", u8),
                ("pad0", u8), ("lcu_score", u32), ("lcu_cost", u8), ("pad", u8 * 3)]


class MdcPic(C.Structure):
    _fields_ = [("scene_characteristic_id", u8), ("adjust_min_qp", u8), ("high_intra_selection", u8), ("slice_cb_qp_offset", i8), ("slice_cr_qp_offset", i8),
                ("tc_offset", i8), ("beta_offset", i8), ("average_qp", u8), ("adp_depth_sensitive_picture_class", u8), ("adp_refinement_mode", u8),
                ("number_of_segments", u8), ("pad0", u8), ("budget", u32), ("predicted_cost", u32), ("lcu_min_score", u32), ("lcu_max_score", u32), ("score_th", i8 * 7),
                ("interval_cost", u8 * 7), ("iterations", u8), ("bdp_present", u8), ("md_present", u8), ("pad", u8 * 3)]


class MdcArrays(C.Structure):
    _fields_ = [("lcu", C.c_void_p), ("picture", C.c_void_p)]


# job field of the header <- scalar of mdc_records.SCALARS
SCALAR_FIELDS = (("slice_type", "slice_type"), ("temporal_layer_index", "layer"), ("hierarchical_levels", "hier"), ("is_used_as_reference", "ref"),
                 ("depth_mode", "depth_mode"), ("enc_mode", "enc_mode"), ("resolution_class", "cls"), ("qp", "qp"), ("is_pan", "pan"), ("is_tilt", "tilt"),
                 ("noise_detection_th", "ndth"), ("homogeneity_percentage", "homog"), ("frame_rate_30", "fr30"), ("cu8x8_mode", "cu8"), ("average_intensity", "avg_int"))
PAIR_FIELDS = (("ref_average_intensity", "ref_int"), ("ref_intra_coded_area", "ref_intra"), ("ref_temporal_layer", "ref_layer"), ("ref_penalize_skip", "ref_skip"))
assert {s for _, s in SCALAR_FIELDS} | {s + k for _, s in PAIR_FIELDS for k in "01"} == set(R.SCALARS)


def fill_scalars(j, jb, lam, split_bits):
    """the host-owned part of a job: the scalars of mdc_records.job, the picture's SAD lambda and splitFlagBits[0], [3]"""
    for field, name in SCALAR_FIELDS:
        setattr(j, field, jb[name])
    for field, name in PAIR_FIELDS:
        getattr(j, field)[0], getattr(j, field)[1] = jb[name + "0"], jb[name + "1"]
    j.lambda_sad, j.split_flag_bits[0], j.split_flag_bits[1] = lam, split_bits[0], split_bits[1]
    return j


def declare(lib):
    lib.svt_amd_md_config_batch_launch.restype = C.c_int
    lib.svt_amd_md_config_batch_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint16, C.c_uint16, C.c_void_p]
    lib.svt_amd_md_config_bytes.restype, lib.svt_amd_md_config_bytes.argtypes = C.c_size_t, [C.c_uint16, C.c_uint16, C.c_int]
    lib.svt_amd_debug_md_config_stages.restype, lib.svt_amd_debug_md_config_stages.argtypes = None, [C.c_int]
    lib.svt_amd_debug_launch_markers.restype = C.c_int
    lib.svt_amd_debug_launch_markers.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.svt_amd_last_error.restype = C.c_char_p
    return lib
