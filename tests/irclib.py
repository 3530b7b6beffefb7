"""ctypes views of the batched initial rate control (include/svt_hevc_amd.h "Batched initial rate control"): the job, the four records and the array table, the
prototypes, and the step from a picture of tests/irc_records.py and its window lists (irc_numpy.window_lists) to the C job.  The numpy layouts of the records
are irc_records.CHECKS_DTYPE, MOTION_DTYPE, IRC_LCU_DTYPE and IRC_PIC_DTYPE; tests/test_irc_abi.py holds the three forms - header, ctypes, numpy - against one
another."""
import ctypes as C

ENTRY = "svt_amd_initial_rc_batch_launch"
IRC_CHECKS, IRC_MOTION, IRC_LCU, IRC_STATIONARY, IRC_PM_STATIONARY, IRC_PICTURE = range(6)
MAX_LCUS = 16384
MAX_BATCH = 256                    # SVT_AMD_MAX_BATCH
u8, u16, u32, u64 = C.c_uint8, C.c_uint16, C.c_uint32, C.c_uint64


class IrcJob(C.Structure):
    _fields_ = [("me", C.c_void_p), ("stats", C.c_void_p), ("edge_checks", C.c_void_p * 4), ("edge_detect", C.c_void_p * 4), ("hom_stats", C.c_void_p * 16),
                ("pan_motion", C.c_void_p * 8), ("cur_slot", C.c_int32), ("edge_count", u8), ("hom_count", u8), ("pan_count", u8), ("slice_type", u8),
                ("temporal_layer_index", u8), ("hierarchical_levels", u8), ("resolution_class", u8), ("look_ahead", u8), ("frames_to_check", u8), ("pad", u8 * 3)]


class IrcChecks(C.Structure):
    _fields_ = [("check1", u8), ("pm_check1", u8), ("check2", u8), ("low_dist_logo", u8)]


class IrcMotion(C.Structure):
    _fields_ = [("total_checked_lcus", u32), ("total_pan_lcus", u32), ("total_tilt_lcus", u32), ("total_pan_high_amp_lcus", u32), ("total_tilt_high_amp_lcus", u32),
                ("is_pan_raw", u8), ("is_tilt_raw", u8), ("pad", u8 * 2)]


class IrcLcu(C.Structure):
    _fields_ = [("similar_edge_count", u8 * 16), ("pm_similar_edge_count", u8 * 16), ("var_of_var_over_time", u64), ("homogeneous_over_time", u8), ("motion_votes", u8),
                ("pad", u8 * 6)]


class IrcPic(C.Structure):
    _fields_ = [("is_pan", u8), ("is_tilt", u8), ("homogeneity_percentage", u8), ("pad0", u8), ("homogeneous_lcu_count", u16), ("stationary_lcu_count", u16 * 4),
                ("pad", u8 * 2)]


class IrcArrays(C.Structure):
    _fields_ = [("checks", C.c_void_p), ("motion", C.c_void_p), ("lcu", C.c_void_p), ("stationary_edge", C.c_void_p), ("pm_stationary_edge", C.c_void_p),
                ("picture", C.c_void_p)]


def fill_job(j, p, cls, lists, at):
    """the job of picture `p` (a dict of irc_records.sequence) with the window lists `lists` of irc_numpy.window_lists; at(kind, k) -> the device address of
    array `kind` ('stats', 'detect', 'checks', 'motion') of picture k of the sequence.  me / stats / cur_slot are the caller's"""
    for k, e in enumerate(lists["edge"]):
        j.edge_checks[k], j.edge_detect[k] = at("checks", e), at("detect", e)
    for k, e in enumerate(lists["hom"]):
        j.hom_stats[k] = at("stats", e)
    for k, e in enumerate(lists["pan"]):
        j.pan_motion[k] = at("motion", e)
    j.edge_count, j.hom_count, j.pan_count = len(lists["edge"]), len(lists["hom"]), len(lists["pan"])
    j.slice_type, j.temporal_layer_index, j.hierarchical_levels, j.resolution_class = p["slice_type"], p["layer"], p["hier"], cls
    j.look_ahead, j.frames_to_check = lists["look_ahead"], lists["frames_to_check"]
    return j


def declare(lib):
    lib.svt_amd_initial_rc_batch_launch.restype = C.c_int
    lib.svt_amd_initial_rc_batch_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint16, C.c_uint16, C.c_void_p]
    lib.svt_amd_initial_rc_bytes.restype, lib.svt_amd_initial_rc_bytes.argtypes = C.c_size_t, [C.c_uint16, C.c_uint16, C.c_int]
    lib.svt_amd_debug_launch_markers.restype = C.c_int
    lib.svt_amd_debug_launch_markers.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.svt_amd_last_error.restype = C.c_char_p
    return lib
