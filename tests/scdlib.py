"""ctypes views of the batched scene-transition detection (include/svt_hevc_amd.h "Batched scene-transition detection"): the job, the picture record, the state
and the array table, and the prototypes.  The numpy layouts of the records are scd_records.PIC_DTYPE and STATE_DTYPE; tests/test_scd_abi.py holds the three forms -
header, ctypes, numpy - against one another."""
import ctypes as C

ENTRY = "svt_amd_scene_detect_batch_launch"
SCD_PICTURE, SCD_AHD, SCD_STATE = range(3)
MAX_LCUS = 16384
MAX_REGIONS = 16
MAX_BATCH = 256                    # SVT_AMD_MAX_BATCH
u8, u32 = C.c_uint8, C.c_uint32
JOB_FIELDS = ("past_histogram", "cur_histogram", "past_chroma_histogram", "cur_chroma_histogram", "past_region_average", "cur_region_average",
              "future_region_average", "past_detect", "cur_detect")


class ScdJob(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in JOB_FIELDS]


class ScdPic(C.Structure):
    _fields_ = [("scene_change", u8), ("reset_running_avg", u8), ("abrupt_regions", u8), ("scene_regions", u8), ("region_count_threshold", u8), ("pad", u8 * 3),
                ("region_class", u8 * 16)]


class ScdState(C.Structure):
    _fields_ = [("ahd_running_avg", u32 * 16), ("ahd_running_avg_cb", u32 * 16), ("ahd_running_avg_cr", u32 * 16), ("reset_running_avg", u8), ("pad", u8 * 3)]


class ScdArrays(C.Structure):
    _fields_ = [("picture", C.c_void_p), ("ahd", C.c_void_p), ("state", C.c_void_p)]


def declare(lib):
    lib.svt_amd_scene_detect_batch_launch.restype = C.c_int
    lib.svt_amd_scene_detect_batch_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint16, C.c_uint16, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.svt_amd_scene_detect_bytes.restype, lib.svt_amd_scene_detect_bytes.argtypes = C.c_size_t, [C.c_int, C.c_int, C.c_int]
    lib.svt_amd_debug_scene_detect_stages.restype, lib.svt_amd_debug_scene_detect_stages.argtypes = None, [C.c_int]
    lib.svt_amd_debug_launch_markers.restype = C.c_int
    lib.svt_amd_debug_launch_markers.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.svt_amd_last_error.restype = C.c_char_p
    return lib
