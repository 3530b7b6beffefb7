"""CPU-only: the launch widths of the mode-decision picture kernel (svt-hevc_amd/csrc/md_widths.h: the one computation behind the blocking entries and
svt_amd_md_encode_picture_launch) as a plain C program of its own (tools/md_widths_check.c) built with -fsanitize=address,undefined and run directly.  No result of a
picture depends on its launch width, so nothing else notices a retune that changes one: the widths DESIGN.md quotes are pinned here as literals, and a sweep holds the
header against a restatement of the formula and against the order 1 <= narrow <= wide <= lone <= min(n_active, 224)."""
import os
import subprocess

import pytest

import svtlib as S

# (width, height, tiles, n_active or None = the whole picture, (grid, narrow, wide) overrides) -> (lone, wide, narrow)
PINS = [
    ((64, 64, 1, None, (0, 0, 0)), (1, 1, 1)),
    ((192, 128, 1, None, (0, 0, 0)), (6, 5, 5)),
    ((200, 136, 1, None, (0, 0, 0)), (6, 5, 5)),
    ((320, 192, 1, None, (0, 0, 0)), (8, 6, 6)),
    ((416, 240, 1, None, (0, 0, 0)), (10, 7, 7)),
    ((640, 360, 1, None, (0, 0, 0)), (12, 9, 8)),
    ((640, 384, 4, None, (0, 0, 0)), (42, 24, 12)),
    ((1920, 1080, 1, None, (0, 0, 0)), (32, 21, 11)),
    ((3840, 2160, 1, None, (0, 0, 0)), (62, 40, 20)),                       # the widths DESIGN.md 3.25 and 8 name
    ((3840, 2160, 16, None, (0, 0, 0)), (224, 224, 224)),
    ((7680, 4320, 4, None, (0, 0, 0)), (224, 224, 129)),
    ((416, 240, 1, 5, (0, 0, 0)), (5, 5, 5)),
    ((3840, 2160, 1, None, (300, 0, 0)), (224, 224, 224)),
    ((3840, 2160, 1, None, (0, 3, 0)), (62, 40, 3)),
    ((3840, 2160, 1, None, (0, 0, 50)), (50, 50, 20)),
]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("md_widths") / "md_widths_check"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(S.ROOT, "tools", "md_widths_check.c"), "-o", str(exe)])
    return str(exe)


def run(checker, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([checker] + [str(v) for v in args], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]


def restated(wl, hl, tiles, n_active):
    """the formula without overrides, written independently of the header: workgroups per LCU of the widest wavefront, capped by the LCUs there are and by 224"""
    front = min((wl + 1) // 2, hl) * max(tiles, 1)
    cap = min(n_active, 224)
    wide = min(front + 2 + (wl + 7) // 8, cap)
    lone = max(min(2 * front + 2, cap), wide)
    narrow = min(max((front + 2 + (wl + 7) // 8 + 1) // 2, 8), wide)
    return lone, wide, narrow


def test_the_pinned_widths(checker):
    args = []
    for (w, h, tiles, n_active, over), _ in PINS:
        wl, hl = (w + 63) // 64, (h + 63) // 64
        args += [wl, hl, tiles, wl * hl if n_active is None else n_active, *over]
    got = run(checker, args)
    assert got == [want for _, want in PINS], list(zip(PINS, got))


def test_the_sweep_equals_the_restatement_and_keeps_the_order(checker):
    rows = run(checker, ["sweep", 130, 70])
    assert len(rows) == 130 * 70 * 4 * 3
    seen = set()
    for wl, hl, tiles, n_active, lone, wide, narrow in rows:
        seen.add((wl, hl, tiles, n_active))
        assert (lone, wide, narrow) == restated(wl, hl, tiles, n_active), (wl, hl, tiles, n_active)
        assert 1 <= narrow <= wide <= lone <= min(n_active, 224), (wl, hl, tiles, n_active, lone, wide, narrow)
    want = {(wl, hl, t, a) for wl in range(1, 131) for hl in range(1, 71) for t in (1, 2, 4, 16) for a in (1, max(wl * hl // 2, 1), wl * hl)}
    assert seen == want


def test_a_bad_command_line_is_not_run(checker):
    r = subprocess.run([checker, "1", "2", "3"], capture_output=True, text=True)
    assert r.returncode == 2
