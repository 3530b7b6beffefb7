"""numpy restatement of what the stream-ordered entropy hand-off (svt-hevc_amd/csrc/handoff_kernels.hip) judges and copies by itself: the validity rules of the
records, the check sums of its head and the copies of the record heads.  The scan itself is the existing checker's (svt_oracle_coeff_scan_lcu) - run on
`sanitized` records, in which everything the rules refuse codes nothing."""
import numpy as np

NONE = 0xFFFFFFFF
MAX_CUS = 64
WORK_HEAD_BYTES, RESULT_HEAD_BYTES = 1584, 768


def unit_ok(cu, num_cus):
    """a unit is scanned when its size is 8 / 16 / 32 / 64, x and y are multiples of 8, it lies inside the LCU and - a 64x64 unit - it is the LCU's only unit"""
    x, y, s = int(cu["x"]), int(cu["y"]), int(cu["size"])
    if s not in (8, 16, 32, 64) or x % 8 or y % 8 or x + s > 64 or y + s > 64:
        return False
    return s != 64 or num_cus == 1


def lcu_status(work):
    """(the LCU is refused, its number of refused units - 0 for a refused LCU, whose units are not looked at)"""
    n = int(work["num_cus"])
    if n > MAX_CUS:
        return True, 0
    ok = [unit_ok(work["cu"][c], n) for c in range(n)]
    covered = sum(int(work["cu"][c]["size"]) ** 2 for c in range(n) if ok[c])
    if covered > 64 * 64:              # well-formed units that overlap: more sub-blocks than an LCU's lists hold
        return True, 0
    return False, n - sum(ok)


def check(works):
    """{bad_lcus, first_bad_lcu, bad_units, first_bad_unit_lcu} of the records, as SvtAmdTailCheck counts"""
    out = {"bad_lcus": 0, "first_bad_lcu": NONE, "bad_units": 0, "first_bad_unit_lcu": NONE}
    for k, w in enumerate(works):
        refused, units = lcu_status(w)
        if refused:
            out["bad_lcus"] += 1
            out["first_bad_lcu"] = min(out["first_bad_lcu"], k)
        elif units:
            out["bad_units"] += units
            out["first_bad_unit_lcu"] = min(out["first_bad_unit_lcu"], k)
    return out


def bad_slots(work):
    """result slots that must read "nothing to code" whatever their cbf says: all 64 of a refused LCU; of a refused unit its own slot, and slots 0..4 where it is
    the lone 64x64 unit of its LCU (whose transform units are slots 1..4)"""
    n = int(work["num_cus"])
    if lcu_status(work)[0]:
        return list(range(MAX_CUS))
    slots = []
    for c in range(n):
        if not unit_ok(work["cu"][c], n):
            slots += list(range(5)) if n == 1 and int(work["cu"][c]["size"]) == 64 else [c]
    return slots


def sanitized(works, results):
    """copies of the records in which what the rules refuse is not coded: cbf 0 in every refused slot, no unit in a refused LCU.  On these the existing checker
    gives what the hand-off must give on the original records"""
    works, results = works.copy(), results.copy()
    for k in range(len(works)):
        for c in bad_slots(works[k]):
            results[k]["cu"][c]["cbf"] = 0
        if lcu_status(works[k])[0]:
            works[k]["num_cus"] = 0
    return works, results


def head_copies(works, results):
    """the first 1584 / 768 bytes of every record"""
    wb = np.ascontiguousarray(works).view(np.uint8).reshape(len(works), -1)[:, :WORK_HEAD_BYTES]
    rb = np.ascontiguousarray(results).view(np.uint8).reshape(len(results), -1)[:, :RESULT_HEAD_BYTES]
    return wb, rb


def exclusive_sums(counts):
    c = np.asarray(counts, np.int64)
    return np.concatenate([[0], np.cumsum(c)[:-1]])


MALFORMED_CHECK = {"bad_lcus": 2, "first_bad_lcu": 2, "bad_units": 5, "first_bad_unit_lcu": 7}


def malformed(works, results):
    """copies of a picture's records (20 LCUs or more, two units or more each) with seven of them rewritten, each refused unit with cbf 1 in all three planes, so that
    a forgotten guard would scan it: (works, results, the rewritten LCUs); check() of them is MALFORMED_CHECK"""
    works, results = works.copy(), results.copy()
    assert len(works) >= 20 and int(works["num_cus"].min()) >= 2

    def unit(k, c, **fields):
        for f, v in fields.items():
            works[k]["cu"][c][f] = v
        results[k]["cu"][c]["cbf"], results[k]["cu"][c]["nz"] = 1, 3

    works[2]["num_cus"] = 65
    works[5]["num_cus"] = 255
    unit(7, 0, size=12)
    unit(9, 1, x=60, y=0, size=16)
    unit(11, 0, y=4)
    works[13]["num_cus"] = 2                                                   # a 64x64 unit in a two-unit LCU
    unit(13, 0, x=0, y=0, size=64)
    works[13]["cu"][1]["x"], works[13]["cu"][1]["y"], works[13]["cu"][1]["size"] = 0, 0, 8
    works[16]["num_cus"] = 1                                                   # a lone 64x64 unit at (32, 0)
    unit(16, 0, x=32, y=0, size=64)
    for c in range(1, 5):
        results[16]["cu"][c]["cbf"] = 1
    assert check(works) == MALFORMED_CHECK
    return works, results, (2, 5, 7, 9, 11, 13, 16)
