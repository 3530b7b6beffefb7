"""Seeded single-unit jobs for the motion-vector candidate lists (AMVP, merge, predictor choice) at the ends of their input ranges, the numpy views of
SvtAmdMdListJob / SvtAmdMdListOut (include/svt_hevc_amd.h), the comparison the tests share and a plain-Python model of the lists that says WHICH path a job
takes (a clip, a rounding term, a temporal position ...): the coverage counts of tests/test_oracle_mvlists.py.  Nothing here comes from the reference encoder;
tests/golden/make_mvlists_golden.py runs the reference on these jobs and stores what it answers.

Input ranges: POC distances in [-1000, 1000] and never 0, vectors over all of int16, pictures from 72x72 to 4096x2304 (multiples of 8, partial LCUs at the
right and at the bottom), units of 8..64 wholly inside the picture.  colocated_poc is ref_poc[colocated list] (list 0 in P pictures): the reference reads
both from one object.  Neighbours of a P picture use list 0 only, and so does its motion-estimation candidate."""
import numpy as np

NB_DTYPE = np.dtype([("mv", "<i2", (2, 2)), ("dir", "u1"), ("avail", "u1"), ("pad", "u1", 2)])
JOB_DTYPE = np.dtype([("width", "<u2"), ("height", "<u2"), ("ox", "<u2"), ("oy", "<u2"), ("size", "u1"), ("slice_type", "u1"), ("colocated_pu_ref_list", "u1"),
                      ("is_low_delay", "u1"), ("has_field", "u1"), ("total_merge", "u1"), ("tile_left", "u1"), ("tile_top", "u1"), ("tile_right", "u1"),
                      ("me_dir", "u1"), ("pool", "<u2", 2), ("me_mv", "<i2", (2, 2)), ("pad", "u1", 2), ("picture_number", "<u8"), ("ref_poc", "<u8", 2),
                      ("colocated_poc", "<u8"), ("nb", NB_DTYPE, 5), ("pad2", "u1", 4)])
OUT_DTYPE = np.dtype([("amvp", "<i2", (2, 2, 2)), ("amvp_count", "u1", 2), ("merge_count", "u1"), ("mvp_idx", "u1", 2), ("merge_dir", "u1", 5),
                      ("merge_mv", "<i2", (5, 2, 2)), ("cand_mv", "<i2", (2, 2)), ("mvp", "<i2", (2, 2)), ("pad", "u1", 14)])
TMVP_DTYPE = np.dtype([("mv", "<i2", (2, 16, 2)), ("ref_poc", "<u8", (2, 16)), ("pred_dir", "u1", 16), ("available", "u1", 16)])
assert NB_DTYPE.itemsize == 12 and JOB_DTYPE.itemsize == 128 and OUT_DTYPE.itemsize == 96 and TMVP_DTYPE.itemsize == 416

A0, A1, B0, B1, B2 = range(5)
PICTURES = [(72, 72), (136, 200), (416, 240), (1000, 520), (1920, 1080), (4096, 2304), (4088, 2296), (3848, 2168)]
DISTANCES = [1, -1, 2, -2, 3, -3, 4, -4, 8, -8, 15, 16, 17, -15, -16, -17, 64, -64, 127, 128, 129, 130, -127, -128, -129, -130, 255, 256, -256, 500, -500, 999,
             1000, -999, -1000]
POOL_GROUPS = [5000, 20000, 70000, (1 << 33) + 12345]   # the colocated_poc of the jobs that read a record of the group
POOL_PER_GROUP = 12


def z_available(x, y, s):
    """isBottomLeftAvailable / isUpperRightAvailable of a unit inside its LCU (the rule of tests/test_gpu_encodepass.py)"""
    def zidx(px, py):
        z = 0
        for b in range(4):
            z |= ((px >> (b + 2)) & 1) << (2 * b) | ((py >> (b + 2)) & 1) << (2 * b + 1)
        return z
    me = zidx(x, y)
    bl = x > 0 and y + s < 64 and zidx(x - 4, y + s) < me
    if x == 0:
        bl = y + s < 64
    tr = y > 0 and x + s < 64 and zidx(x + s, y - 4) < me
    if y == 0:
        tr = True
    return bool(bl), bool(tr)


def allowed_neighbours(w, h, ox, oy, s, tile_left, tile_top, tile_right):
    """which of A0, A1, B0, B1, B2 a unit may use at all: decoding order, the picture's bounds, the tile edges of its LCU"""
    bl, tr = z_available(ox & 63, oy & 63, s)
    left_edge = ox == 0 or (tile_left and (ox & 63) == 0)
    top_edge = oy == 0 or (tile_top and (oy & 63) == 0)
    right_edge = tile_right and ((ox + s) & 63) == 0
    return [bl and not left_edge and oy + s < h, not left_edge, tr and not top_edge and not right_edge and ox + s < w, not top_edge,
            not left_edge and not top_edge]


def _mv(rng):
    k = rng.integers(0, 10)
    if k == 0:
        return int(rng.choice([-32768, 32767, -32767, 32766]))
    if k == 1:
        return int(rng.choice([0, 0, 1, -1]))
    if k < 5:
        return int(rng.integers(-600, 601))
    if k == 5:
        return -(2 * int(rng.integers(0, 16384)) + 1)        # negative and odd: the rounding term of a negative product
    return int(rng.integers(-32768, 32768))


def _dist(rng):
    if rng.integers(0, 4):
        return int(rng.choice(DISTANCES))
    d = int(rng.integers(-1000, 1001))
    return d if d else 7


def make_pool(seed):
    """the co-located motion fields the jobs index: POOL_PER_GROUP records per colocated POC, every vector / distance / direction / availability mix"""
    rng = np.random.default_rng(seed)
    pool = np.zeros(len(POOL_GROUPS) * POOL_PER_GROUP, TMVP_DTYPE)
    for r in range(len(pool)):
        c = POOL_GROUPS[r // POOL_PER_GROUP]
        kind = r % POOL_PER_GROUP
        for u in range(16):
            for l in range(2):
                pool[r]["mv"][l, u] = (_mv(rng), _mv(rng))
                pool[r]["ref_poc"][l, u] = c - _dist(rng)
            pool[r]["pred_dir"][u] = rng.integers(0, 3)
            pool[r]["available"][u] = 0 if kind == 0 else 1 if kind == 1 else int(rng.integers(0, 4) != 0)
    return pool


def _geometry(rng, want=None):
    """picture, unit and tile flags.  want: 'all5' (every neighbour may be available), 'br_here' / 'br_right' / 'center' (where the temporal candidate lies),
    'far' (a large picture's far corner: ClipMV's bounds at their ends) or None"""
    for _ in range(1000):
        w, h = PICTURES[rng.integers(0, len(PICTURES))] if want != "far" else PICTURES[rng.integers(5, len(PICTURES))]
        s = int(rng.choice([8, 16, 32, 64]))
        wl, hl = (w + 63) // 64, (h + 63) // 64
        lx = int(rng.choice([0, wl - 1, rng.integers(0, wl)])) if want != "far" else wl - 1 - int(rng.integers(0, 2))
        ly = int(rng.choice([0, hl - 1, rng.integers(0, hl)])) if want != "far" else hl - 1 - int(rng.integers(0, 2))
        n = 64 // s
        ux, uy = int(rng.choice([0, n - 1, rng.integers(0, n)])), int(rng.choice([0, n - 1, rng.integers(0, n)]))
        ox, oy = lx * 64 + ux * s, ly * 64 + uy * s
        if ox + s > w or oy + s > h:
            continue
        tl = int(lx == 0 or rng.integers(0, 8) == 0)
        tt = int(ly == 0 or rng.integers(0, 8) == 0)
        tr = int(lx == wl - 1 or rng.integers(0, 8) == 0)
        center = ox + s >= w or oy + s >= h or (oy & 63) + s >= 64
        if want == "all5" and not all(allowed_neighbours(w, h, ox, oy, s, tl, tt, tr)):
            continue
        if want == "br_here" and (center or (ox & 63) + s >= 64):
            continue
        if want == "br_right" and (center or (ox & 63) + s != 64):
            continue
        if want == "center" and not center:
            continue
        return w, h, ox, oy, s, tl, tt, tr
    raise AssertionError("no geometry for %r" % (want,))


def tmvp_position(j, pool):
    """md_tmvp_position: (bottom_right, lcu_offset, unit)"""
    ox, oy, s = int(j["ox"]), int(j["oy"]), int(j["size"])
    if not (ox + s >= int(j["width"]) or oy + s >= int(j["height"]) or (oy & 63) + s >= 64):
        brx = (ox & 63) + s
        off, unit = brx >> 6, (((oy & 63) + s) >> 4) * 4 + ((brx & 63) >> 4)
        if pool[int(j["pool"][off])]["available"][unit] == 1:
            return 1, off, unit
    return 0, 0, (((oy & 63) + (s >> 1)) >> 4) * 4 + (((ox & 63) + (s >> 1)) >> 4)


def make_jobs(seed, n, pool):
    """n jobs: aimed recipes in turn (each sets up one path of the lists), every availability pattern, then free mixes of the same ingredients"""
    rng = np.random.default_rng(seed)
    jobs = np.zeros(n, JOB_DTYPE)
    recipes = ["sf_hi", "sf_lo", "comp_hi", "comp_lo", "neg_round", "tb_td_clip", "equal", "scale_a", "scale_b", "same_poc", "dup", "zero_fill", "no_fill",
               "br_here", "br_right", "center", "t_unavail", "no_field", "b2_drop", "b2_keep", "combined", "combined_refused", "zero_merge", "clip_far", "clip_near",
               "tie", "idx1", "pattern", "pattern", "free", "free", "free"]
    for i in range(n):
        j = jobs[i]
        rec = recipes[i % len(recipes)]
        want = {"br_here": "br_here", "br_right": "br_right", "center": "center", "clip_far": "far", "pattern": "all5", "b2_drop": "all5", "b2_keep": "all5",
                "combined": "all5", "combined_refused": "all5", "t_unavail": "center"}.get(rec)
        if rec in ("sf_hi", "sf_lo", "comp_hi", "comp_lo", "neg_round", "scale_a", "scale_b", "dup", "tie", "idx1"):
            want = "all5"
        w, h, ox, oy, s, tl, tt, tr = _geometry(rng, want)
        j["width"], j["height"], j["ox"], j["oy"], j["size"], j["tile_left"], j["tile_top"], j["tile_right"] = w, h, ox, oy, s, tl, tt, tr
        bslice = rng.integers(0, 4) != 0 or rec in ("combined", "combined_refused", "same_poc", "sf_hi", "sf_lo", "comp_hi", "comp_lo", "neg_round", "scale_a", "scale_b")
        j["slice_type"] = 0 if bslice else 1
        j["colocated_pu_ref_list"] = rng.integers(0, 2)
        j["is_low_delay"] = rng.integers(0, 3) == 0
        j["has_field"] = 0 if rec == "no_field" else int(rng.integers(0, 8) != 0)
        j["total_merge"] = rng.choice([2, 3, 5])
        # POCs: the group of the motion field fixes colocated_poc = ref_poc[colocated list]
        g = int(rng.integers(0, len(POOL_GROUPS)))
        kind = 0 if rec == "t_unavail" else 1 if rec in ("br_here", "br_right") else int(rng.integers(0, POOL_PER_GROUP))
        j["pool"][0] = g * POOL_PER_GROUP + kind
        j["pool"][1] = g * POOL_PER_GROUP + (1 if rec == "br_right" else int(rng.integers(0, POOL_PER_GROUP)))
        col = int(j["colocated_pu_ref_list"]) if bslice else 0
        d = [_dist(rng), _dist(rng)]
        if rec == "same_poc" or (bslice and rng.integers(0, 10) == 0):
            d[1] = d[0]
        if rec in ("sf_hi", "comp_hi", "sf_lo", "comp_lo"):      # list 1's factor: tb = d[1] large against td = d[0] small, the sign picks the end
            d[0] = int(rng.choice([1, 2, 3, -1, -2, -3]))
            d[1] = int(rng.integers(60, 1001)) * (1 if (d[0] > 0) == (rec in ("sf_hi", "comp_hi", "comp_lo")) else -1)
            if rec == "comp_lo":
                d[1] = -d[1] if rng.integers(0, 2) else d[1]
        if rec == "neg_round":                                     # factor +-128: the product of an odd vector component ends in .5
            d[0] = int(rng.choice([2, -2, 4, -4, 8]))
            d[1] = d[0] // 2 * int(rng.choice([1, -1]))
        if rec == "tb_td_clip":
            d = [int(rng.choice([129, 130, 500, 1000, -129, -130, -500, -1000])), int(rng.choice([129, 200, 999, -129, -200, -999, 3, -3]))]
        pn = POOL_GROUPS[g] + d[col]
        j["picture_number"], j["colocated_poc"] = pn, POOL_GROUPS[g]
        j["ref_poc"][0], j["ref_poc"][1] = pn - d[0], pn - d[1]
        # neighbours
        allowed = allowed_neighbours(w, h, ox, oy, s, tl, tt, tr)
        for k in range(5):
            u = j["nb"][k]
            u["mv"] = [[_mv(rng), _mv(rng)], [_mv(rng), _mv(rng)]]
            u["dir"] = rng.integers(0, 3) if bslice else 0
            u["avail"] = int(allowed[k] and rng.integers(0, 3) != 0)
        if rec == "pattern":
            p = (i // len(recipes)) % 32
            for k in range(5):
                j["nb"][k]["avail"] = (p >> k) & 1
        nb = j["nb"]
        if rec in ("sf_hi", "sf_lo", "comp_hi", "comp_lo", "neg_round", "scale_a"):   # only A neighbours, of list 0 alone: list 1 takes the scaled vector
            for k in range(5):
                nb[k]["avail"] = int(k in (A0, A1) and (k == A1 or rng.integers(0, 2)))
                nb[k]["dir"] = 0
            big = 32767 if rec == "comp_hi" else -32768
            if rec in ("comp_hi", "comp_lo"):
                sign = 1 if (d[0] > 0) == (d[1] > 0) else -1
                for k in (A0, A1):
                    nb[k]["mv"][0] = (big if sign > 0 else (-32768 if big > 0 else 32767), int(rng.integers(2100, 30000)) * sign * (1 if big > 0 else -1))
            if rec == "neg_round":
                for k in (A0, A1):
                    v = 2 * int(rng.integers(0, 16000)) + 1
                    nb[k]["mv"][0] = (-v if d[1] > 0 else v, _mv(rng)) if (d[0] > 0) else (v if d[1] > 0 else -v, _mv(rng))
        if rec == "scale_b":
            for k in range(5):
                nb[k]["avail"] = int(k in (B0, B1, B2) and rng.integers(0, 2))
                nb[k]["dir"] = 0
            nb[B1]["avail"] = 1
        if rec == "dup":                                           # A and B hold the same vector of the target picture
            for k in range(5):
                nb[k]["avail"], nb[k]["dir"] = int(k in (A1, B1)), 2 if bslice else 0
            nb[B1]["mv"] = nb[A1]["mv"]
        if rec in ("zero_fill", "no_fill"):                        # one spatial candidate and no temporal one
            j["has_field"] = 0
            for k in range(5):
                nb[k]["avail"], nb[k]["dir"] = int(k == A1 and allowed[A1]), 2 if bslice else 0
            nz = int(rng.integers(1, 30000)) * int(rng.choice([1, -1]))
            nb[A1]["mv"] = [[nz, 0 if rec == "no_fill" else -nz]] * 2
        if rec in ("b2_drop", "b2_keep"):                          # five distinct neighbours / four
            for k in range(5):
                nb[k]["avail"] = int(not (rec == "b2_keep" and k == B0))
                nb[k]["mv"] = [[100 + k, k], [-k, 7 * k + 1]]
            j["total_merge"] = 5
        if rec in ("combined", "combined_refused"):                # two candidates, one of each list
            j["total_merge"], j["has_field"] = 5, 0
            for k in range(5):
                nb[k]["avail"] = int(k in (A1, B1))
            nb[A1]["dir"], nb[B1]["dir"] = 0, 1
            if rec == "combined_refused":
                j["ref_poc"][1 - col] = j["ref_poc"][col]          # (the co-located list's picture stays the field's)
                nb[B1]["mv"][1] = nb[A1]["mv"][0]
        if rec == "zero_merge":
            j["total_merge"], j["has_field"] = 5, 0
            for k in range(5):
                nb[k]["avail"] = int(k == B1 and allowed[B1])
        # the motion-estimation candidate
        j["me_dir"] = rng.integers(0, 3) if bslice else 0
        j["me_mv"] = [[_mv(rng), _mv(rng)], [_mv(rng), _mv(rng)]]
        if rec in ("clip_far", "clip_near") or rng.integers(0, 6) == 0:
            e = 32767 if rng.integers(0, 2) else -32768
            j["me_mv"] = [[e, -e - 1 if rng.integers(0, 2) else e], [-e - 1, e if rng.integers(0, 2) else -e - 1]]
        if rec in ("tie", "idx1"):                                 # two distinct candidates in both lists (A1, B1 bi-predictive), the vector on / beyond their middle
            j["has_field"] = 0
            for k in range(5):
                nb[k]["avail"], nb[k]["dir"] = int(k in (A1, B1)), 2 if bslice else 0
            for l in range(2):
                a = (int(rng.integers(-200, 200)), int(rng.integers(-200, 200)))
                dx, dy = 2 * int(rng.integers(1, 40)), 2 * int(rng.integers(0, 40))
                nb[A1]["mv"][l], nb[B1]["mv"][l] = a, (a[0] + dx, a[1] + dy)
                j["me_mv"][l] = (a[0] + dx // 2, a[1] + dy // 2) if rec == "tie" else (a[0] + dx, a[1] + dy + 3)
    return jobs


# ---- the comparison the CPU and the GPU tests share --------------------------------------------------------------------------------------------------------------
def compare_outs(jobs, got, want, what):
    """field by field, every job: the counts; the AMVP candidates below the count of the lists the picture has (P: list 0); a merge candidate's direction and the
    vectors of the lists that direction uses; the motion-estimation candidate's clipped vector, predictor index and predictor of the lists its direction uses"""
    errs = []
    bs = jobs["slice_type"] == 0

    def chk(name, mask, a, b):
        mask = np.broadcast_to(mask.reshape(mask.shape + (1,) * (a.ndim - mask.ndim)), a.shape)
        bad = np.nonzero(((a != b) & mask).reshape(len(jobs), -1).any(axis=1))[0]
        if len(bad):
            k = int(bad[0])
            errs.append("%s: %d jobs, first %d: got %s want %s" % (name, len(bad), k, a[k].tolist(), b[k].tolist()))
    for l in range(2):
        lm = bs | (l == 0)
        chk("amvp_count[%d]" % l, lm, got["amvp_count"][:, l], want["amvp_count"][:, l])
        for k in range(2):
            chk("amvp[%d][%d]" % (l, k), lm & (want["amvp_count"][:, l] > k), got["amvp"][:, l, k], want["amvp"][:, l, k])
        um = (jobs["me_dir"] == 2) | (jobs["me_dir"] == l)
        for f in ("cand_mv", "mvp_idx", "mvp"):
            chk("%s[%d]" % (f, l), um, got[f][:, l], want[f][:, l])
    chk("merge_count", np.ones(len(jobs), bool), got["merge_count"], want["merge_count"])
    for k in range(5):
        km = want["merge_count"] > k
        chk("merge_dir[%d]" % k, km, got["merge_dir"][:, k], want["merge_dir"][:, k])
        for l in range(2):
            chk("merge_mv[%d][%d]" % (k, l), km & ((want["merge_dir"][:, k] == 2) | (want["merge_dir"][:, k] == l)), got["merge_mv"][:, k, l], want["merge_mv"][:, k, l])
    assert not errs, "%s:\n%s" % (what, "\n".join(errs))


# ---- a plain model of the lists that names the paths a job takes -------------------------------------------------------------------------------------------------
def _clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def _s16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def _scale(tb, td, mv, F):
    if td == tb:
        F.add("td==tb")
        return mv
    for name, v in (("tb", tb), ("td", td)):
        if v > 127:
            F.add(name + ">127")
        if v < -128:
            F.add(name + "<-128")
    tb, td = _clip3(-128, 127, tb), _clip3(-128, 127, td)
    q = (0x4000 + abs(td >> 1)) // abs(td)
    temp = _s16(q if td > 0 else -q)
    raw = (tb * temp + 32) >> 6
    if raw > 4095:
        F.add("factor>4095")
    if raw < -4096:
        F.add("factor<-4096")
    sc = _clip3(-4096, 4095, raw)
    out = []
    for v in mv:
        p = sc * v
        r = (p + 127 + (p < 0)) >> 8
        if p < 0 and ((p + 128) >> 8) != ((p + 127) >> 8):
            F.add("negative product: rounding term decides")
        if r > 32767:
            F.add("component>32767")
        if r < -32768:
            F.add("component<-32768")
        out.append(_clip3(-32768, 32767, r))
    return tuple(out)


def model(j, pool):
    """(out as a dict, the set of paths taken) of one job"""
    F = set()
    bs = int(j["slice_type"]) == 0
    pn, rp = int(j["picture_number"]), [int(j["ref_poc"][0]), int(j["ref_poc"][1])]
    nb = [dict(mv=[tuple(int(c) for c in j["nb"][k]["mv"][l]) for l in range(2)], dir=int(j["nb"][k]["dir"]), avail=int(j["nb"][k]["avail"])) for k in range(5)]
    field = bool(j["has_field"])
    pos = tmvp_position(j, pool) if field else None

    def temporal(L):
        br, off, unit = pos
        m = pool[int(j["pool"][off if br else 0])]
        if not br and not m["available"][unit]:
            F.add("temporal: unavailable")
            return None
        F.add("temporal: " + ("centre" if not br else "bottom-right, LCU to the right" if off else "bottom-right, this LCU"))
        cl = L if j["is_low_delay"] else 1 - int(j["colocated_pu_ref_list"])
        pd = int(m["pred_dir"][unit])
        F.add("co-located pred_dir %d" % pd)
        cl = cl if pd == 2 else pd
        return _scale(_s16(pn - rp[L]), _s16(int(j["colocated_poc"]) - int(m["ref_poc"][cl, unit])), tuple(int(c) for c in m["mv"][cl, unit]), F)

    def nonscale(u, L):
        if u["dir"] < 2:
            return (u["mv"][u["dir"]] if rp[L] == rp[u["dir"]] else None)
        return u["mv"][L]

    def scaled(u, L, who):
        F.add("spatial scaling from " + who)
        l2 = L if u["dir"] == 2 else u["dir"]
        return _scale(_s16(pn - rp[L]), _s16(pn - rp[l2]), u["mv"][l2], F)
    out = dict(amvp=[[(0, 0), (0, 0)], [(0, 0), (0, 0)]], amvp_count=[0, 0])
    for L in range(2 if bs else 1):
        c = []
        ax = None
        for k in (A0, A1):
            if ax is None and nb[k]["avail"]:
                ax = nonscale(nb[k], L)
        if ax is None and (nb[A0]["avail"] or nb[A1]["avail"]):
            ax = scaled(nb[A0] if nb[A0]["avail"] else nb[A1], L, "A")
        if ax is not None:
            c.append(ax)
        bx = None
        for k in (B0, B1, B2):
            if bx is None and nb[k]["avail"]:
                bx = nonscale(nb[k], L)
        if bx is not None:
            c.append(bx)
        if ax is None and (nb[B0]["avail"] or nb[B1]["avail"] or nb[B2]["avail"]):
            c.append(scaled(nb[B0] if nb[B0]["avail"] else nb[B1] if nb[B1]["avail"] else nb[B2], L, "B"))
        if len(c) == 2 and c[0] == c[1]:
            F.add("equal AMVP candidates reduced")
            c = c[:1]
        if field and len(c) < 2:
            t = temporal(L)
            if t is not None:
                c.append(t)
        if len(c) == 1 and c[0][0] != 0 and c[0][1] != 0:
            F.add("zero fill after one candidate")
            c.append((0, 0))
        elif len(c) == 1:
            F.add("count 1: a zero component, no fill")
        elif not c:
            c.append((0, 0))
        out["amvp_count"][L] = len(c)
        for k in range(len(c)):
            out["amvp"][L][k] = c[k]
    # merge
    tm = int(j["total_merge"])
    m = []

    def differs(a, b):
        if not bs:
            return a["mv"][0] != b["mv"][0]
        return a["dir"] != b["dir"] or a["mv"] != b["mv"]

    def add(u):
        m.append((u["dir"] if bs else 0, u["mv"][0], u["mv"][1]))
    n = nb
    steps = [(A1, lambda: True), (B1, lambda: not n[A1]["avail"] or differs(n[B1], n[A1])), (B0, lambda: not n[B1]["avail"] or differs(n[B0], n[B1])),
             (A0, lambda: not n[A1]["avail"] or differs(n[A0], n[A1]))]
    for k, ok in steps:
        if len(m) < tm and n[k]["avail"] and ok():
            add(n[k])
    if len(m) < tm and n[B2]["avail"] and (not n[A1]["avail"] or differs(n[B2], n[A1])) and (not n[B1]["avail"] or differs(n[B2], n[B1])):
        if len(m) < 4:
            F.add("B2 kept")
            add(n[B2])
        else:
            F.add("B2 dropped: four candidates stand")
    if len(m) < tm and field:
        t0 = temporal(0)
        if t0 is not None:
            F.add("temporal merge candidate")
            m.append((2, t0, temporal(1)) if bs else (0, t0, (0, 0)))
    if len(m) < tm and bs:
        l0c, l1c = [0, 1, 0, 2, 1, 2, 0, 3, 1, 3, 2, 3], [1, 0, 2, 0, 2, 1, 3, 0, 3, 1, 3, 2]
        end = len(m) * (len(m) - 1)
        f = 0
        while len(m) < tm and f < end:
            c0, c1 = m[l0c[f]], m[l1c[f]]
            if ((c0[0] + 1) & 1) and ((c1[0] + 1) & 2):
                if rp[0] != rp[1] or c0[1] != c1[2]:
                    F.add("combined bi-predictive candidate")
                    m.append((2, c0[1], c1[2]))
                else:
                    F.add("combined candidate refused: equal halves on equal POCs")
            f += 1
    while len(m) < tm:
        F.add("zero-vector merge fill")
        m.append((2 if bs else 0, (0, 0), (0, 0)))
    out["merge"] = m
    # predictor choice
    ox, oy, w, h = int(j["ox"]), int(j["oy"]), int(j["width"]), int(j["height"])
    lo = [_s16(((1 - ox - 8 - 64) << 2)), _s16(((1 - oy - 8 - 64) << 2))]
    hi = [_s16(((w + 8 - ox - 1) << 2)), _s16(((h + 8 - oy - 1) << 2))]
    out["cand_mv"], out["mvp_idx"], out["mvp"] = [None, None], [None, None], [None, None]
    for L in range(2):
        if int(j["me_dir"]) not in (2, L):
            continue
        v = [int(c) for c in j["me_mv"][L]]
        for a in range(2):
            if v[a] < lo[a]:
                F.add("ClipMV: %s raised to its lower bound" % "xy"[a])
            if v[a] > hi[a]:
                F.add("ClipMV: %s lowered to its upper bound" % "xy"[a])
            v[a] = _clip3(lo[a], hi[a], v[a])
        c = out["amvp"][L]
        idx = 0
        if out["amvp_count"][L] == 2:
            d0, d1 = abs(c[0][0] - v[0]) + abs(c[0][1] - v[1]), abs(c[1][0] - v[0]) + abs(c[1][1] - v[1])
            idx = 0 if d0 <= d1 else 1
            F.add("two candidates: tie" if d0 == d1 else "two candidates: mvp_idx %d" % idx)
        out["cand_mv"][L], out["mvp_idx"][L], out["mvp"][L] = tuple(v), idx, c[idx]
    return out, F


def model_out_array(jobs, pool):
    """the model's outs in OUT_DTYPE (fields a comparison does not read are zero) and the per-job path sets"""
    outs = np.zeros(len(jobs), OUT_DTYPE)
    flags = []
    for i in range(len(jobs)):
        o, F = model(jobs[i], pool)
        flags.append(F)
        r = outs[i]
        r["amvp"], r["amvp_count"] = o["amvp"], o["amvp_count"]
        r["merge_count"] = len(o["merge"])
        for k, (d, v0, v1) in enumerate(o["merge"]):
            r["merge_dir"][k], r["merge_mv"][k] = d, (v0, v1)
        for L in range(2):
            if o["cand_mv"][L] is not None:
                r["cand_mv"][L], r["mvp_idx"][L], r["mvp"][L] = o["cand_mv"][L], o["mvp_idx"][L], o["mvp"][L]
    return outs, flags


# the conditions the fixture must hold, and how many jobs each at least
CONDITIONS = {c: 20 for c in (
    "factor>4095", "factor<-4096", "component>32767", "component<-32768", "negative product: rounding term decides", "tb>127", "tb<-128", "td>127", "td<-128",
    "td==tb", "spatial scaling from A", "spatial scaling from B", "ref_poc[0]==ref_poc[1]", "equal AMVP candidates reduced", "zero fill after one candidate",
    "count 1: a zero component, no fill", "temporal: bottom-right, this LCU", "temporal: bottom-right, LCU to the right", "temporal: centre", "temporal: unavailable",
    "co-located pred_dir 0", "co-located pred_dir 1", "co-located pred_dir 2", "B, not low-delay, colocated list 0", "B, not low-delay, colocated list 1", "B, low-delay",
    "P", "no motion field", "merge count 2", "merge count 3", "merge count 5", "B2 kept", "B2 dropped: four candidates stand", "temporal merge candidate",
    "combined bi-predictive candidate", "combined candidate refused: equal halves on equal POCs", "zero-vector merge fill", "ClipMV: x raised to its lower bound",
    "ClipMV: x lowered to its upper bound", "ClipMV: y raised to its lower bound", "ClipMV: y lowered to its upper bound", "two candidates: mvp_idx 0",
    "two candidates: mvp_idx 1", "two candidates: tie")}
CONDITIONS.update({"availability pattern %d" % p: 5 for p in range(32)})
CONDITIONS.update({"neighbour %d dir %d" % (k, d): 20 for k in range(5) for d in range(3)})


def coverage(jobs, flags):
    """condition -> number of jobs: the paths the model names plus what the jobs' own fields say"""
    counts = {c: 0 for c in CONDITIONS}
    for i in range(len(jobs)):
        j = jobs[i]
        F = set(flags[i])
        bs = int(j["slice_type"]) == 0
        if bs and int(j["ref_poc"][0]) == int(j["ref_poc"][1]):
            F.add("ref_poc[0]==ref_poc[1]")
        if bs and j["has_field"]:
            F.add("B, low-delay" if j["is_low_delay"] else "B, not low-delay, colocated list %d" % int(j["colocated_pu_ref_list"]))
        if not bs:
            F.add("P")
        if not j["has_field"]:
            F.add("no motion field")
        F.add("merge count %d" % int(j["total_merge"]))
        F.add("availability pattern %d" % sum(int(j["nb"][k]["avail"]) << k for k in range(5)))
        for k in range(5):
            if j["nb"][k]["avail"]:
                F.add("neighbour %d dir %d" % (k, int(j["nb"][k]["dir"])))
        for c in F:
            if c in counts:
                counts[c] += 1
    return counts


SEED, COUNT, POOL_SEED = 20261021, 4000, 77     # the committed fixture (tests/golden/mvlists_seeded.npz)


def run_lists(fn, jobs, pool, returns=False):
    """svt_ref_mv_lists / svt_oracle_md_lists (host arrays): the outs of the jobs"""
    import ctypes as C
    jobs, pool = np.ascontiguousarray(jobs), np.ascontiguousarray(pool)
    assert jobs.dtype == JOB_DTYPE and pool.dtype == TMVP_DTYPE and int(jobs["pool"].max()) < len(pool)
    outs = np.zeros(len(jobs), OUT_DTYPE)
    fn.restype, fn.argtypes = (C.c_int if returns else None), [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    rc = fn(jobs.ctypes.data, pool.ctypes.data, outs.ctypes.data, len(jobs))
    assert not returns or rc == 0, "job %d is no unit of an LCU, or its colocated_poc is not its co-located reference picture's" % (-1 - rc)
    return outs
