"""What the CPU-only tests of the C-ABI share: the built library, its exported names, header checks through a C compiler and the comparison of a ctypes view
with a numpy layout."""
import ctypes as C
import os
import subprocess

import numpy as np

import svtlib as S


def open_library(declare):
    """the built library with the prototypes `declare` (of a *lib.py / *_records.py) gives it"""
    assert os.path.exists(S.PRODUCT_SO), "run `python __graft_entry__.py build` first"
    return declare(C.CDLL(S.PRODUCT_SO))


def exported():
    """the names the library defines"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", S.PRODUCT_SO], text=True)
    return set(line.split()[-1] for line in out.splitlines() if " T " in line)


def compiles(tmp_path, std, checks):
    """every expression of `checks` holds as gcc -std=`std` sees include/svt_hevc_amd.h (_Static_assert is gcc's extension in C99)"""
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "svt_hevc_amd.h"\n' + "".join('_Static_assert(%s, "%s");\n' % (c, c.replace('"', "")) for c in checks) +
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=" + std, "-Wall", "-Werror", "-I", os.path.join(S.ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "t.o")])


def view_matches_dtype(view, dtype):
    """the ctypes structure and the numpy layout have the same fields at the same offsets, of the same sizes and - but for nested structures - scalar types"""
    assert C.sizeof(view) == dtype.itemsize
    assert [f for f, _ in view._fields_] == list(dtype.names)
    for f, t in view._fields_:
        sub, offset = dtype.fields[f][:2]
        assert getattr(view, f).offset == offset and C.sizeof(t) == sub.itemsize, f
        scalar = t
        while hasattr(scalar, "_length_"):
            scalar = scalar._type_
        if not issubclass(scalar, C.Structure):
            assert np.dtype(scalar) == sub.base.newbyteorder("="), f
