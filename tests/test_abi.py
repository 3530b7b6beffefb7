"""CPU-only: the C-ABI library builds, loads, and exports every symbol include/svt_hevc_amd.h
declares; Python-side struct views match the C layout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import svtlib as S


def _declared_symbols():
    text = open(os.path.join(S.ROOT, "include", "svt_hevc_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(svt_amd_\w+)\s*\(", text))
    names |= {"svt_amd_" + n for n in re.findall(r"^SVT_AMD_DECL_(?:TRANSFORM|INTRA|INTRA_ANG|MCP_UNI|MCP_RAW|MCP_CUNI|MCP_CRAW)\((\w+)", text, flags=re.M)}
    return sorted(names)


def test_header_symbols_exported():
    assert os.path.exists(S.PRODUCT_SO), "run `python __graft_entry__.py build` first"
    out = subprocess.check_output(["nm", "-D", "--defined-only", S.PRODUCT_SO], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    declared = _declared_symbols()
    assert len(declared) >= 190
    missing = [s for s in declared if s not in exported]
    assert not missing, "declared but not exported: %s" % missing
    stray = [s for s in exported if not s.startswith("svt_amd_")]
    assert not stray, "non-API symbols exported: %s" % stray


def test_library_loads_without_gpu():
    lib = C.CDLL(S.PRODUCT_SO)
    lib.svt_amd_version.restype = C.c_char_p
    assert b"gfx950" in lib.svt_amd_version()


def test_struct_layouts():
    assert C.sizeof(S.MeParams) == S.ME_PARAMS_DTYPE.itemsize == 108
    assert C.sizeof(S.MeCuResult) == S.ME_CU_DTYPE.itemsize == 24
    assert C.sizeof(S.MeLcuResult) == S.ME_LCU_DTYPE.itemsize == 3420
    assert S.DUMP_DTYPE.itemsize == 3592


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "svt_hevc_amd.h"\n'
                   '_Static_assert(sizeof(SvtAmdMeParams) == 108, "params");\n'
                   '_Static_assert(sizeof(SvtAmdMeLcuResult) == 3420, "lcu result");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(S.ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "t.o")])


def test_no_gpu_means_loud_failure():
    """Without a device the batched layer must fail (no CPU fallback)."""
    import torch
    if torch.cuda.is_available():
        return
    lib = S.load_product()
    ctx = C.c_void_p()
    rc = lib.svt_amd_context_create(0, 640, 384, 2, C.byref(ctx))
    assert rc != 0 and not ctx.value
    assert lib.svt_amd_last_error()


# the reference's public API, Source/API/EbApi.h:682-783
EB_API = {"EbInitHandle", "EbH265EncSetParameter", "EbInitEncoder", "EbH265EncStreamHeader", "EbH265EncReleaseStreamHeader", "EbH265EncEosNal",
          "EbH265EncReleaseEosNal", "EbH265EncSendPicture", "EbH265GetPacket", "EbH265ReleaseOutBuffer", "EbH265GetRecon", "EbDeinitEncoder",
          "EbDeinitHandle"}
DROP_IN = S.DROP_IN


def test_drop_in_library_is_the_reference_outer_abi():
    """oracle/_ref/hooked/libSvtHevcEnc.so.1 (reference objects + the bindings) is what ffmpeg / gstreamer / the sample application
    load in place of the reference's library: SONAME libSvtHevcEnc.so.1, version node SVT_HEVC_1, exactly the 13 Eb* entry points
    (SURVEY 8b outer ABI).  The library is prebuilt by __graft_entry__.build() (needs /root/reference), so it is present wherever
    the tests run."""
    assert os.path.exists(DROP_IN), "run `python __graft_entry__.py build` first (needs /root/reference)"
    out = subprocess.check_output(["nm", "-D", "--defined-only", DROP_IN], text=True)
    names = [line.split()[-1] for line in out.splitlines() if " T " in line or " A " in line]
    funcs = {n.split("@")[0] for n in names if " A " not in n and not n.startswith("SVT_HEVC_1")}
    assert funcs == EB_API, (sorted(funcs - EB_API), sorted(EB_API - funcs))
    assert all(n.endswith("@@SVT_HEVC_1") for n in names if n.split("@")[0] in EB_API), names
    dyn = subprocess.check_output(["readelf", "-d", DROP_IN], text=True)
    assert "Library soname: [libSvtHevcEnc.so.1]" in dyn
    assert "libsvt_hevc_amd.so" in dyn                      # the HIP hot path is a NEEDED library of the drop-in
    assert os.path.islink(os.path.join(os.path.dirname(DROP_IN), "libSvtHevcEnc.so"))


def test_drop_in_library_answers_the_api_without_the_sample_app():
    """dlopen + EbInitHandle / EbH265EncSetParameter / EbDeinitHandle through the exported names only (no GPU needed: the device
    context is created by EbInitEncoder, which this test does not reach)."""
    code = r'''
import ctypes as C, sys
lib = C.CDLL(%r)
h = C.c_void_p()
cfg = C.create_string_buffer(4096)          # EB_H265_ENC_CONFIGURATION is ~600 bytes; EbInitHandle fills in the defaults
lib.EbInitHandle.restype = C.c_uint32
lib.EbInitHandle.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
rc = lib.EbInitHandle(C.byref(h), None, cfg)
assert rc == 0 and h.value, hex(rc)
lib.EbDeinitHandle.restype = C.c_uint32
lib.EbDeinitHandle.argtypes = [C.c_void_p]
assert lib.EbDeinitHandle(h) == 0
print("OUTER_ABI_OK", any(cfg.raw))
''' % DROP_IN
    r = subprocess.run([os.sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert "OUTER_ABI_OK True" in r.stdout, r.stdout[-500:] + r.stderr[-1500:]


HIP_APP = S.HIP_APP


def _run_hooked(tmp_path, env):
    yuv = str(tmp_path / "c.yuv")
    S.write_clip(yuv, "motion", 128, 64, 3, 7)
    return subprocess.run([HIP_APP, "-i", yuv, "-w", "128", "-h", "64", "-n", "3", "-b", str(tmp_path / "o.265"), "-encMode", "9"],
                          capture_output=True, text=True, timeout=120, env=dict(os.environ, **env))


def test_device_failure_at_init_is_an_error_code_not_a_core_dump(tmp_path):
    """SURVEY 8b "Errors": a device that cannot be brought up fails EbInitEncoder with EB_ErrorInsufficientResources (the sample
    application prints its out-of-memory line and exits 1) - the host process is not aborted.  Device 99 exists nowhere, so the test
    means the same with and without a GPU."""
    assert os.path.exists(HIP_APP), "run `python __graft_entry__.py build` first (needs /root/reference)"
    r = _run_hooked(tmp_path, {"SVT_AMD_DEVICE": "99"})
    assert r.returncode == 1, (r.returncode, r.stderr[-800:])                   # a signal would be negative
    assert "Could not allocate enough memory for channel 1" in r.stdout       # EB_ErrorInsufficientResources (App/EbAppMain.c)
    assert "svt_amd_context_create (device 99)" in r.stderr


def test_device_failure_inside_the_pipeline_reaches_the_error_handler(tmp_path):
    """A failure after start-up (here: the lazily created context) goes to appCallbackPtr->ErrorHandler: the application receives an
    error packet (EbH265GetPacket -> EB_ErrorMax), reports it and shuts the encoder down itself."""
    assert os.path.exists(HIP_APP)
    r = _run_hooked(tmp_path, {"SVT_AMD_DEVICE": "99", "SVT_HOOK_LAZY_INIT": "1"})
    assert r.returncode >= 0, (r.returncode, r.stderr[-800:])
    assert "Error encoding at channel 1" in r.stdout and "Encoder finished" in r.stdout
