"""CPU-only: the restatement of the picture tail (tests/tail_numpy.py) against the pinned restatements of the two host loops
(tests/test_oracle_encodepass_golden.py:deblock_maps, :sao_inputs_of_picture) on every picture of the 14 deblocking / SAO fixtures and on seeded quadtrees, what the
fixtures hold, the documented counts on malformed records, the stage rules, and the per-LCU routine the device compiles (svt-hevc_amd/csrc/tail_logic.h) as a plain
C program under -fsanitize=address,undefined over the same inputs."""
import os
import subprocess

import numpy as np
import pytest

import svtlib as S
import tail_numpy as N
import taillib as T
from test_gpu_tmvp import random_heads
from tmvplib import WORK_HEAD_DTYPE
from test_oracle_encodepass_golden import DLF_CASES, SAO_CASES, allows_mismatch, deblock_maps, is16, load_case, sao_inputs_of_picture

FIXTURES = DLF_CASES + SAO_CASES
SEEDED = [(64, 64, 2, 3), (136, 72, 0, 5), (200, 136, 0, 7), (200, 136, 1, 11)]


def pictures(name):
    g, w, h = load_case(name)
    nl = S.lcu_count(w, h)
    for first in range(0, len(g["work"]), nl):
        yield g, w, h, int(g["picture_number"][first]), g["work"][first:first + nl], g["result"][first:first + nl]


def seeded_picture(w, h, slice_type, seed):
    """seeded quadtrees with a QP per unit (random_heads), random luma cbf in every result slot and random tile flags"""
    rng = np.random.default_rng(seed)
    heads = random_heads(rng, w, h, slice_type)
    for f in ("tile_left", "tile_top", "tile_right"):
        heads[f] = rng.integers(0, 2, len(heads)) * rng.integers(1, 256, len(heads))     # any non-zero byte is a set flag
    results = np.zeros(len(heads), S.LCU_RESULT_DTYPE)
    results["cu"]["cbf"] = rng.integers(0, 2, results["cu"]["cbf"].shape)
    return heads, results


def follow_of(works, w, h):
    """the follow bits as tests/test_oracle_encodepass_golden.py:encoder_order_lcu is called: an LCU follows to the right / below, inside the same tile"""
    cols = (w + 63) // 64
    out = np.zeros(len(works), np.uint8)
    for k, wk in enumerate(works):
        x0, y0 = int(wk["lcu_x"]), int(wk["lcu_y"])
        lw, lh = min(64, w - x0), min(64, h - y0)
        right = x0 + lw < w and not wk["tile_right"]
        below = y0 + lh < h and not (k + cols >= len(works) or works[k + cols]["tile_top"])
        out[k] = right | below << 1
    return out


def same_as_host_loops(works, results, w, h, sao_like, tag):
    got = N.maps(works, T.cbf0_of(results), w, h)
    cumap, cbf, qp, edge = deblock_maps(works, results, w, h)
    assert got["cumap"].tobytes() == cumap.tobytes() and got["cbf"].tobytes() == cbf.tobytes() and got["qp"].tobytes() == qp.tobytes(), tag
    assert np.array_equal(got["edge"], edge), tag
    _, _, params, _, _ = sao_inputs_of_picture(sao_like, -1, works, w, h)
    assert np.array_equal(got["sao_edge"], params["edge_flags"]), tag
    assert np.array_equal(got["follow"], follow_of(works, w, h)), tag
    assert not got["status"].any() and N.check(got["status"]).tolist() == (0, N.NONE, 0, N.NONE), tag
    return got


@pytest.fixture(scope="module")
def empty_sao():
    """a fixture-shaped record set without a record: sao_inputs_of_picture then derives the edge flags alone"""
    g, _, _ = load_case(SAO_CASES[0])
    return dict(sao=g["sao"][:0])


def test_there_are_fourteen_fixtures():
    assert len(FIXTURES) == 14


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_host_loops_on_every_fixture_picture(name, empty_sao):
    n = 0
    for g, w, h, f, works, results in pictures(name):
        same_as_host_loops(works, results, w, h, empty_sao, (name, f))
        n += 1
    assert n >= 1


@pytest.mark.parametrize("w,h,slice_type,seed", SEEDED)
def test_restatement_equals_the_host_loops_on_seeded_quadtrees(w, h, slice_type, seed, empty_sao):
    heads, results = seeded_picture(w, h, slice_type, seed)
    got = same_as_host_loops(heads, results, w, h, empty_sao, (w, h, seed))
    if (w, h) == (200, 136):
        assert len(np.unique(got["qp"])) > 8 and set(np.unique(got["cbf"]).tolist()) == {0, 1} and len(set(got["sao_edge"].tolist())) > 2


def test_the_fixtures_hold_what_the_tail_must_handle():
    """64x64 inter units, 8x8 units, intra units in P / B pictures, partial LCUs of 8 samples in both directions, 2-column and 2x2 tiles, one allowEncDecMismatch picture,
    two 10-bit I pictures, cbf 0 and 1; and NOT an LCU with SAO shut off or QPs that differ inside a picture (seeded inputs cover those)"""
    seen = dict(inter64=False, unit8=False, intra_in_pb=False, partial=False, tile_cols=False, tile_grid=False, mismatch=set(), i10=set(), cbf=set(), sao_off=False, qps=False)
    for name in FIXTURES:
        for g, w, h, f, works, results in pictures(name):
            cols = (w + 63) // 64
            if name.startswith("sao_"):
                if allows_mismatch(g, w, h, works[0]):
                    seen["mismatch"].add(name)
                _, enable, _, _, idx = sao_inputs_of_picture(g, f, works, w, h)
                seen["sao_off"] |= len(idx) not in (0, len(works))
            if is16(g) and int(works[0]["slice_type"]) == 2:
                seen["i10"].add(name)
            seen["partial"] |= w % 64 == 8 and h % 64 == 8
            inner_left = [k for k, wk in enumerate(works) if wk["tile_left"] and k % cols]
            inner_top = [k for k, wk in enumerate(works) if wk["tile_top"] and k >= cols]
            seen["tile_cols"] |= bool(inner_left)
            seen["tile_grid"] |= bool(inner_left) and bool(inner_top)
            qps = set()
            for wk, rs in zip(works, results):
                cu = wk["cu"][:int(wk["num_cus"])]
                seen["inter64"] |= bool(((cu["size"] == 64) & (cu["pred_mode"] == 1)).any())
                seen["unit8"] |= bool((cu["size"] == 8).any())
                seen["intra_in_pb"] |= int(wk["slice_type"]) != 2 and bool((cu["pred_mode"] == 2).any())
                seen["cbf"].update(rs["cu"]["cbf"][:len(cu), 0].tolist())
                qps.update(cu["qp"].tolist())
            seen["qps"] |= len(qps) > 1
    assert seen["inter64"] and seen["unit8"] and seen["intra_in_pb"] and seen["partial"] and seen["tile_cols"] and seen["tile_grid"], seen
    assert seen["mismatch"] == {"sao_b_motion_320x192_m8"} and len(seen["i10"]) == 2 and seen["cbf"] == {0, 1}, seen
    assert not seen["sao_off"] and not seen["qps"], seen


def malformed():
    two = random_heads(np.random.default_rng(21), 128, 64, 0)
    cases = {k: (v[0], 128, 64, v[1]) for k, v in T.malformed_cases(two).items()}
    h, want = T.outside_case(random_heads(np.random.default_rng(22), 200, 136, 0))
    cases["a unit outside the picture"] = (h, 200, 136, want)
    return cases


@pytest.mark.parametrize("what", sorted(malformed()))
def test_malformed_records_give_the_documented_counts(what):
    heads, w, h, want = malformed()[what]
    results = np.ones(len(heads), S.LCU_RESULT_DTYPE)
    got = N.maps(heads, T.cbf0_of(results), w, h)
    assert N.check(got["status"]).tolist() == want, what
    bad = np.nonzero(got["status"])[0]
    assert len(bad) == 1
    cols, k = (w + 63) // 64, int(bad[0])
    y8, x8 = (k // cols) * 8, (k % cols) * 8
    if got["status"][k] & N.LCU_BAD or int(heads[k]["num_cus"]) == 1:       # nothing of the LCU is taken: its cells stay 0
        assert not got["cumap"][y8:y8 + 8, x8:x8 + 8].tobytes().strip(b"\0") and not got["qp"][y8:y8 + 8, x8:x8 + 8].any()
        assert not got["cbf"][2 * y8:2 * y8 + 16, 2 * x8:2 * x8 + 16].any()
    planes, known = N.source_planes(np.zeros(len(heads), S.LCU_WORK_DTYPE), got["status"], w, h)
    assert known[0].all() != bool(got["status"][k] & N.LCU_BAD)


def test_stage_rules():
    D, S_, A, R = N.DEBLOCK, N.SAO_DECIDE, N.SAO_APPLY, N.REFERENCE
    for stages in range(0, 18):
        why = N.stages_refused(stages, 0, True, 80, 80)
        want = "stages" if stages in (0, 16, 17) else "apply" if stages & A and (stages & (D | S_)) != (D | S_) else None
        assert why == want, stages
    assert N.stages_refused(R, 0, False, 80, 80) == "reference" and N.stages_refused(R, 0, True, 6, 80) == "reference" and N.stages_refused(R, 0, True, 80, 81) == "reference"
    assert N.stages_refused(D, 1, True, 80, 80) == "stages"
    assert N.latest_stage(D | S_ | A, False, False) == (True, True, "fin") and N.latest_stage(S_ | R, False, False) == (False, False, "rec")
    assert N.latest_stage(D | R, False, False) == (True, False, "dbk")


# ---- the routine the device compiles, as a plain C program under the sanitizers ----

@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tail_logic") / "tail_logic_check"
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(S.ROOT, "tools", "tail_logic_check.c"), "-o", str(exe)])
    return str(exe)


def run_checker(checker, tmp_path, heads, results, w, h):
    n = len(heads)
    raw = np.zeros((n, T.LIST_BYTES + T.RESULT_CU_BYTES), np.uint8)
    raw[:, :T.LIST_BYTES] = np.ascontiguousarray(heads).view(np.uint8).reshape(n, -1)[:, :T.LIST_BYTES]
    raw[:, T.LIST_BYTES:] = np.ascontiguousarray(results).view(np.uint8).reshape(n, -1)[:, :T.RESULT_CU_BYTES]
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([w, h, n], np.int32).tobytes() + raw.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([checker, str(src), str(dst)], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = np.fromfile(dst, np.uint8)
    c8 = (w // 8) * (h // 8)
    cuts = np.cumsum([12 * c8, 4 * c8, c8, 4 * n, 16])
    assert len(out) == cuts[-1]
    cumap, cbf, qp, by, chk = np.split(out, cuts[:-1])
    return dict(cumap=cumap.view(N.CU_MAP_DTYPE).reshape(h // 8, w // 8), cbf=cbf.reshape(h // 4, w // 4), qp=qp.reshape(h // 8, w // 8), edge=by[:n], sao_edge=by[n:2 * n],
                follow=by[2 * n:3 * n], status=by[3 * n:]), chk.view(N.CHECK_DTYPE)[0]


def same_as_restatement(got, chk, heads, results, w, h, tag):
    want = N.maps(heads, T.cbf0_of(results), w, h)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), (tag, k)
    assert chk.tolist() == N.check(want["status"]).tolist(), tag


@pytest.mark.parametrize("name", FIXTURES)
def test_sanitized_routine_on_the_fixtures(checker, tmp_path, name):
    for g, w, h, f, works, results in pictures(name):
        got, chk = run_checker(checker, tmp_path, works, results, w, h)
        same_as_restatement(got, chk, works, results, w, h, (name, f))


@pytest.mark.parametrize("w,h,slice_type,seed", SEEDED)
def test_sanitized_routine_on_seeded_quadtrees(checker, tmp_path, w, h, slice_type, seed):
    heads, results = seeded_picture(w, h, slice_type, seed)
    got, chk = run_checker(checker, tmp_path, heads, results, w, h)
    same_as_restatement(got, chk, heads, results, w, h, (w, h, seed))


@pytest.mark.parametrize("what", sorted(malformed()))
def test_sanitized_routine_on_malformed_records(checker, tmp_path, what):
    heads, w, h, want = malformed()[what]
    results = np.ones(len(heads), S.LCU_RESULT_DTYPE)
    got, chk = run_checker(checker, tmp_path, heads, results, w, h)
    same_as_restatement(got, chk, heads, results, w, h, what)
    assert chk.tolist() == want


def test_sanitized_routine_on_random_bytes(checker, tmp_path):
    """records of random bytes - every geometry field at any value: nothing leaves the arrays (the sanitizers stay silent) and the restatement counts the same"""
    rng = np.random.default_rng(33)
    w, h = 200, 136
    n = S.lcu_count(w, h)
    heads = np.frombuffer(rng.bytes(n * T.LIST_BYTES), WORK_HEAD_DTYPE).copy()
    cols = (w + 63) // 64
    for k in range(n):          # half of the LCUs at their position, so that their random units are looked at
        if k % 2:
            heads[k]["lcu_x"], heads[k]["lcu_y"], heads[k]["num_cus"] = 64 * (k % cols), 64 * (k // cols), rng.integers(0, 65)
            heads[k]["cu"]["size"] = rng.choice([4, 8, 16, 32, 64, 128], 64)
            heads[k]["cu"]["x"], heads[k]["cu"]["y"] = rng.choice([0, 4, 8, 32, 56, 60, 255], (2, 64))
    results = np.zeros(n, S.LCU_RESULT_DTYPE)
    results["cu"]["cbf"] = rng.integers(0, 256, results["cu"]["cbf"].shape)
    got, chk = run_checker(checker, tmp_path, heads, results, w, h)
    same_as_restatement(got, chk, heads, results, w, h, "random bytes")
    assert chk["bad_lcus"] > 0 and chk["bad_units"] > 0
