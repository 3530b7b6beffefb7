"""The bookkeeping of a slot's ME / OIS records (svt-hevc_amd/csrc/slot_records.h) on the CPU: tests/slot_records_check.cpp includes the header alone, with the
HIP types from the ROCm headers and no HIP call, and checks coverage and publication, reset, the chain decision of each kind of marker, and two threads posting
the bands of one picture side by side."""
import os
import subprocess

import svtlib as S


def test_slot_records_program(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "slot_records_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           "-I", os.path.join(S.ROOT, "svt-hevc_amd", "csrc"), os.path.join(S.ROOT, "tests", "slot_records_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert run.returncode == 0 and run.stdout == b"ok\n", run.stdout.decode()
