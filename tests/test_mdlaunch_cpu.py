"""CPU-only: the row arithmetic of k_md_source (svt-hevc_amd/csrc/md_source_logic.h: which 16-byte chunks of a row are whole, where its tail starts, the 8-MSB view
of 16-bit samples) as a plain C program of its own (tools/md_source_check.c) built with -fsanitize=address,undefined and run directly: source and destination lie
in heap blocks of their exact sizes, the output must equal a row-by-row memcpy and sample >> 2."""
import os
import subprocess

import pytest

import svtlib as S

WIDTHS = (8, 24, 100, 104, 192, 200, 416)
BASES = (0, 4, 8, 12)
ROWS = 5


def pitches(width):
    return (width, width + 4, width + 12, (width + 31) & ~15)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("md_source") / "md_source_check"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(S.ROOT, "tools", "md_source_check.c"), "-o", str(exe)])
    return str(exe)


def run(checker, cases):
    """cases: (bytes per sample, width, rows, source pitch, base, destination pitch, seed) -> rows that took the 16-byte path, per case"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([checker] + [str(v) for c in cases for v in c], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    out = [int(v) for v in r.stdout.split()]
    assert len(out) == len(cases)
    return out


@pytest.mark.parametrize("bps", [1, 2])
def test_every_shape_equals_the_row_by_row_copy(checker, bps):
    cases, seed = [], 1
    for w in WIDTHS:
        for sp in pitches(w):
            for base in BASES:
                for dp in ((w + 127) & ~127, sp):                       # the picture object's pitch, and a destination as awkward as the source
                    cases.append((bps, w, ROWS, sp, base, dp, seed))
                    seed += 1
    chunk_rows = run(checker, cases)
    for c, got in zip(cases, chunk_rows):
        _, w, rows, sp, base, dp, _ = c
        # the 16-byte path is taken by exactly the rows whose source and destination both start 16-byte aligned (heap blocks are; the view row at dp is 8-byte
        # aligned whenever the 16-bit destination row at 2 dp is 16-byte aligned)
        want = sum(1 for y in range(rows) if (base + y * sp * bps) % 16 == 0 and (y * dp * bps) % 16 == 0 and w * bps >= 16)
        assert got == want, (c, got, want)
    assert any(chunk_rows) and not all(chunk_rows)


def test_a_bad_shape_is_not_run(checker):
    r = subprocess.run([checker, "1", "100", "5", "96", "0", "128", "1"], capture_output=True, text=True)
    assert r.returncode == 2
