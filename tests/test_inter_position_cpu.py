"""CPU-only: the position clamp of inter prediction and its integer / fraction split (svt-hevc_amd/csrc/inter_position.h: the one text behind ep_inter_predict_core,
md_predict_tile, the two staged-window fills and the host half of svt_amd_inter_pu_batch) as a plain C program of its own (tools/inter_position_check.c) built with
-fsanitize=address,undefined and run directly.  Literal pins from the formula of Codec/EbInterPrediction.c:802-812 - a position is kept between 71 samples before the
picture and 7 samples behind it, in quarter samples of the padded plane - and a sweep against a restatement in Python integers."""
import os
import subprocess

import pytest

import svtlib as S

W, H = 200, 136
VECTORS = (-32768, -300, -1, 0, 1, 3, 5, 299, 32767)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("inter_position") / "inter_position_check"
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(S.ROOT, "tools", "inter_position_check.c"), "-o", str(exe)])
    return str(exe)


def run(checker, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([checker] + [str(v) for v in args], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    return [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]


def restated(at, mv, origin, extent):
    """one component, written independently of the header: (q, luma integer, luma fraction, chroma integer, chroma fraction); floor division is the arithmetic shift"""
    q = sorted((4 * (origin - 71), 4 * (at + origin) + mv, 4 * (extent + origin + 7)))[1]
    return (q,) + divmod(q, 4) + divmod(q, 8)


def test_the_pinned_positions(checker):
    got = run(checker, [0, 0, -32768, -32768, 80, 80, W, H,
                        192, 192, 32767, 32767, 80, 80, W, H,
                        64, 64, 0, 0, 80, 80, W, H,
                        64, 64, 3, 3, 80, 80, W, H])
    assert [g[:2] for g in got] == [(36, 36), (1148, 892), (576, 576), (579, 579)], got
    # qx qy | luma ix fx iy fy | chroma ix fx iy fy
    assert got[2][2:] == (144, 0, 144, 0, 72, 0, 72, 0), got[2]
    assert got[3][2:] == (144, 3, 144, 3, 72, 3, 72, 3), got[3]
    # the ends do not depend on where the unit is
    assert [g[:2] for g in run(checker, [192, 192, -32768, -32768, 80, 80, W, H, 0, 0, 32767, 32767, 80, 80, W, H])] == [(36, 36), (1148, 892)]


@pytest.mark.parametrize("origin", [8, 80])
def test_the_sweep_equals_the_restatement(checker, origin):
    rows = run(checker, ["sweep", W, H, origin])
    assert len(rows) == 25 * 9 * 9
    seen = set()
    for at, mvx, mvy, qx, qy, lix, lfx, liy, lfy, cix, cfx, ciy, cfy in rows:
        seen.add((at, mvx, mvy))
        assert (qx, lix, lfx, cix, cfx) == restated(at, mvx, origin, W), (at, mvx, origin)
        assert (qy, liy, lfy, ciy, cfy) == restated(at, mvy, origin, H), (at, mvy, origin)
        assert 4 * (origin - 71) <= qx <= 4 * (W + origin + 7) and 4 * (origin - 71) <= qy <= 4 * (H + origin + 7)
    assert seen == {(at, a, b) for at in range(0, 193, 8) for a in VECTORS for b in VECTORS}


def test_a_bad_command_line_is_not_run(checker):
    r = subprocess.run([checker, "1", "2", "3"], capture_output=True, text=True)
    assert r.returncode == 2
