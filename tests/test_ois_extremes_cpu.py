"""CPU-only: what keeps tests/test_gpu_ois_extremes.py honest.  The oracle and the committed records alone show that the inputs of those tests reach what
they are meant to reach: carried 32x32 CUs (tests/ois_extremes.py) at every CU index and with several carried modes in the reference's own records of
x_islands, every stage-1 total and first distortions taken out of an earlier CU's array in the seeded island jobs, distortions of 261,120 on every path,
and edge filters clipped at both ends in the records of xc_blocks."""
import numpy as np
import pytest

import ois_extremes as X
import svtlib as S
from test_oracle_ois_golden import load_ois_case

ISLAND_FIXTURES = ["x_islands_320x256_m9", "x_islands_320x256_m6"]


def test_islands_frames_are_what_they_claim():
    """Flat even frames of both polarities; on odd frames no two blocks touch, every block lies a CU inside the picture and all 4N + 1 reference samples of a
    block are of the other colour; the layouts hold a twin LCU (t = 1) and a chained LCU (t = 3)."""
    kind, w, h, seed = X.ISLANDS
    assert [int(S.gen_luma(kind, w, h, t, seed)[0, 0]) for t in (0, 2, 4, 6)] == [255, 0, 255, 0]
    for t in range(0, 8, 2):
        assert len(np.unique(S.gen_luma(kind, w, h, t, seed))) == 1
    for t in (1, 3, 5, 7):
        luma, lay, g = S.gen_luma(kind, w, h, t, seed), S.islands_layout(w, h, t, seed), S.islands_ground(t)
        blocks = [(x, y, 255 - g) for x, y in lay["islands"]] + [(x, y, g) for x, y in lay["twins"]]
        assert len(lay["islands"]) >= 6 and set(lay["chained"]) <= set(lay["islands"])
        for x, y, inner in blocks:
            assert x % 32 == 0 and y % 32 == 0 and x >= 32 and y >= 32 and x + 64 <= w and y + 64 <= h
            assert (luma[y:y + 32, x:x + 32] == inner).all()
            assert (luma[y - 1, x - 1:x + 64] == 255 - inner).all() and (luma[y - 1:y + 64, x - 1] == 255 - inner).all()
        for i, (x, y, _) in enumerate(blocks):
            for x2, y2, _ in blocks[i + 1:]:  # but for a twin's ground block and the island at CU 1 of its LCU
                assert max(abs(x - x2), abs(y - y2)) >= 64 or ((x2, y2) in lay["twins"] and (x, y) == (x2 - 32, y2 - 32)), (t, x, y, x2, y2)
        assert set(np.unique(luma).tolist()) == {0, 255}
    assert S.islands_layout(w, h, 1, seed)["twins"] and S.islands_layout(w, h, 3, seed)["chained"]


@pytest.mark.parametrize("name", ISLAND_FIXTURES)
def test_reference_records_of_islands_hold_carried_cus(oracle, name):
    g, kind, w, h, seed = load_ois_case(name)
    per_cu, first_modes, by_type = np.zeros(4, int), set(), {}
    for i, (pn, slice_type, _) in enumerate(g["meta"]):
        sat = X.saturated(oracle, kind, w, h, int(pn), seed)
        after = g["after"][i]
        car = X.carried(sat, after) if X.stage1_path(g["params"][i]) else np.zeros_like(sat)
        per_cu += car.sum(axis=0)
        first_modes |= set((after["candidate"][:, 1:5, 0][car] >> 24).tolist())
        assert (g["me_sad"][i][:, 1:5][car] == X.SAT).all(), (name, int(pn))
        seen = by_type.setdefault(int(slice_type), [0, 0])
        seen[0] += int(sat.sum())
        seen[1] += int(car.sum())
    print(name, "carried per CU index", per_cu.tolist(), "first modes", sorted(first_modes), "saturated / carried by slice type", by_type)
    assert (per_cu >= 4).all(), per_cu
    assert 30 in first_modes and len(first_modes) >= 3, first_modes
    assert any(s > 0 and c == 0 for s, c in by_type.values()), by_type  # saturated CUs that no state is carried into (I: planar only; B: ME SAD 0)
    assert any(c > 0 for _, c in by_type.values())


def test_seeded_island_jobs_reach_the_carried_state_in_every_form(oracle):
    totals, borrowed, in_a_row, two, polarities = set(), [], 0, 0, set()
    for j in range(len(X.ISLAND_JOBS)):
        luma, p, me, want, sat = X.island_job(oracle, j)
        polarities.add(int(luma[0, 0]))
        car = X.carried(sat, want)
        totals |= set(want["total"][:, 1:5][car].tolist())
        dist = want["candidate"][:, 1:5, 0][car] & 0xFFFFF
        borrowed += [int(d) for d in dist if d not in (0, X.SAT)]
        for l in np.nonzero(car.sum(axis=1) >= 2)[0]:  # only CU 1 and CU 4 of an LCU can both be saturated (svtlib.islands_layout)
            assert car[l].tolist() == [True, False, False, True]
            two += 1
            in_a_row += want["total"][l, 2:4].tolist() == [1, 1]  # neither CU between them tested a mode: CU 4 gets what CU 1 left
        assert (me["pu"]["distortion"][:, 1:5, 0][car] != 0).all()
    print("carried totals", sorted(totals), "first distortions out of an earlier CU's array", len(borrowed), "LCUs with two carried CUs", two,
          "of them in a row", in_a_row)
    assert polarities == {0, 255}
    assert totals == {3, 5, 7, 9}, totals
    assert len(borrowed) >= 3, borrowed
    assert in_a_row >= 1 and two > in_a_row


def test_distortion_261120_on_every_path(oracle):
    """In the reference's records: the stage-1 path (x_islands P pictures), the 35-mode ranking (x_binary at encMode 4: whole candidate lists of equal
    maxima are not there - see the count) and planar of I pictures; in the oracle's records of an island picture: the DC-only path and the ranking."""
    seen = {}
    for name in ISLAND_FIXTURES + ["x_binary_192x128_m4", "x_stripes_192x128_m7", "xc_blocks_192x128_m9"]:
        g, kind, w, h, seed = load_ois_case(name)
        for i in range(len(g["meta"])):
            p, after = g["params"][i], g["after"][i]
            path = "intra" if p["slice_is_intra"] else "ranked" if p["ois_kernel_level"] else "dc" if p["limit_ois_to_dc_mode"] else "stage1"
            written = after["total"][:, 1:5] != 0xFF if path != "intra" else np.ones((len(after), 4), bool)
            d = after["candidate"][:, 1:5, 0] & 0xFFFFF
            seen[path] = seen.get(path, 0) + int(((d == X.SAT) & written).sum())
            top = max(seen.get("max", 0), int(d[written].max()) if written.any() else 0)
            seen["max"] = top
    kind, w, h, seed = X.ISLANDS
    luma = X.frame(kind, w, h, 1, seed)
    dc = S.oracle_ois_picture(oracle, X.params(w, h, limit_ois_to_dc_mode=1, skip_ois_8x8=1), luma, X.me_of(np.zeros((S.lcu_count(w, h), 85), np.uint32)))
    ranked = S.oracle_ois_picture(oracle, X.params(w, h, ois_kernel_level=1, skip_ois_8x8=1), luma, None)
    n_dc = int(((dc["candidate"][:, 1:5, 0] & 0xFFFFF) == X.SAT).sum())
    all_equal = int(((ranked["candidate"][:, 1:5, :] & 0xFFFFF) == X.SAT).all(axis=2).sum())
    print("first distortions of 261,120 in the reference's records", seen, "oracle: DC-only", n_dc, "ranked lists of 18 equal maxima", all_equal)
    assert seen["stage1"] >= 8 and seen["intra"] >= 8 and seen["max"] == X.SAT
    assert n_dc >= 6 and all_equal >= 6


def test_xc_blocks_records_clip_both_edge_filters_at_both_ends():
    """Plain Python restatement of the two N < 32 edge filters over the CUs whose records show that the filtered modes were tested."""
    g, kind, w, h, seed = load_ois_case("xc_blocks_192x128_m9")
    below = above = dc_below = dc_above = 0
    for i, (pn, slice_type, _) in enumerate(g["meta"]):
        p, after = g["params"][i], g["after"][i]
        luma = S.gen_luma(kind, w, h, int(pn), seed)
        lw = (w + 63) // 64
        for l in range(len(after)):
            for cu in range(5, 85 if p["slice_is_intra"] or not (p["skip_ois_8x8"] or p["cu8x8_mode"] == 1) else 21):
                n = 16 if cu < 21 else 8
                k = cu - 5 if cu < 21 else cu - 21
                per = 4 if cu < 21 else 8
                ox, oy = (l % lw) * 64 + (k % per) * n, (l // lw) * 64 + (k // per) * n
                tot = int(after["total"][l, cu])
                if tot == 0xFF or ox + n > w or oy + n > h:
                    continue
                b, a, db, da = X.edge_filter_extremes(luma, ox, oy, n)
                if p["slice_is_intra"] or (X.stage1_path(p) and tot >= 3):  # modes 10 and 26 were predicted
                    below, above = below + b, above + a
                if p["slice_is_intra"] or not p["ois_kernel_level"]:         # DC was predicted
                    dc_below, dc_above = dc_below + db, dc_above + da
    print("xc_blocks: samples of the mode 10 / 26 edge filter below 0:", below, "above 255:", above, "DC edge filter, neighbour 127 or more below the DC value:",
          dc_below, "above:", dc_above)
    assert below >= 16 and above >= 16 and dc_below >= 16 and dc_above >= 16
