"""The picture tail on the device restated in numpy (include/svt_hevc_amd.h "Picture tail on the device"; svt-hevc_amd/csrc/tail_logic.h, tail_kernels.hip): the
filter inputs one LCU's records give - coding-unit map, QP and luma cbf arrays, the three flag bytes, the status byte - the reduced check record, the source planes
and the stage rules of svt_amd_encdec_picture_tail_launch.  Written unit by unit in list order (the later unit wins) like the host loops of
svt_amd_encdec_picture_deblock / _sao; what those loops refuse is counted here as the kernel counts it."""
import numpy as np

CU_MAP_DTYPE = np.dtype([("mode", "u1"), ("dir", "u1"), ("size_log2", "u1"), ("pad", "u1"), ("mv", "<i2", (2, 2))])
CHECK_DTYPE = np.dtype([("bad_lcus", "<u4"), ("first_bad_lcu", "<u4"), ("bad_units", "<u4"), ("first_bad_unit_lcu", "<u4")])
NONE = 0xFFFFFFFF
LCU_BAD = 0x80
DEBLOCK, SAO_DECIDE, SAO_APPLY, REFERENCE = 1, 2, 4, 8


def unit_bad(u, c, ox, oy, w, h):
    """why unit c of an LCU at (ox, oy) is counted and writes nothing; 0 = it is taken"""
    x, y, s = int(u["x"]), int(u["y"]), int(u["size"])
    if s not in (8, 16, 32, 64):
        return 1
    if x + s > 64 or y + s > 64:
        return 2
    if ox + x + s > w or oy + y + s > h:
        return 3
    if s == 64 and c + 4 >= 64:
        return 4
    return 0


def lcu_bad(wk, i, cols):
    return int(wk["lcu_x"]) != (i % cols) * 64 or int(wk["lcu_y"]) != (i // cols) * 64 or int(wk["num_cus"]) > 64


def maps(works, cbf0, w, h):
    """works: the heads and unit lists of every LCU in raster order (any dtype with the fields of SvtAmdLcuWork in front of src_y); cbf0: [lcus][64] the luma cbf of the
    result slots.  -> dict of cumap (h / 8, w / 8), cbf (h / 4, w / 4), qp (h / 8, w / 8), edge, sao_edge, follow, status [lcus]"""
    cols, n = (w + 63) // 64, len(works)
    cumap, cbf, qp = np.zeros((h // 8, w // 8), CU_MAP_DTYPE), np.zeros((h // 4, w // 4), np.uint8), np.zeros((h // 8, w // 8), np.uint8)
    edge, sao_edge, follow, status = (np.zeros(n, np.uint8) for _ in range(4))
    for i, wk in enumerate(works):
        left, top, right = bool(wk["tile_left"]), bool(wk["tile_top"]), bool(wk["tile_right"])
        bottom = i + cols >= n or bool(works[i + cols]["tile_top"])
        edge[i] = left | top << 1
        sao_edge[i] = left | right << 1 | top << 2 | bottom << 3
        follow[i] = ((i % cols) + 1 < cols and not right) | (not bottom) << 1
        if lcu_bad(wk, i, cols):
            status[i] = LCU_BAD
            continue
        ox, oy = (i % cols) * 64, (i // cols) * 64
        for c in range(int(wk["num_cus"])):
            u = wk["cu"][c]
            if unit_bad(u, c, ox, oy, w, h):
                status[i] += 1
                continue
            x, y, s = int(u["x"]), int(u["y"]), int(u["size"])
            ys, xs = slice((oy + y) // 8, (oy + y + s) // 8), slice((ox + x) // 8, (ox + x + s) // 8)
            e = np.zeros((), CU_MAP_DTYPE)
            e["mode"], e["size_log2"] = u["pred_mode"], s.bit_length() - 1
            if int(u["pred_mode"]) == 1:
                e["dir"], e["mv"] = u["inter_dir"], u["mv"]
            cumap[ys, xs] = e
            qp[ys, xs] = u["qp"]
            if s == 64:
                for t in range(4):
                    ty, tx = (oy + y) // 4 + 8 * (t >> 1), (ox + x) // 4 + 8 * (t & 1)
                    cbf[ty:ty + 8, tx:tx + 8] = cbf0[i][c + 1 + t]
            else:
                cbf[(oy + y) // 4:(oy + y + s) // 4, (ox + x) // 4:(ox + x + s) // 4] = cbf0[i][c]
    return dict(cumap=cumap, cbf=cbf, qp=qp, edge=edge, sao_edge=sao_edge, follow=follow, status=status)


def check(status):
    """SvtAmdTailCheck of the status bytes"""
    out = np.zeros((), CHECK_DTYPE)
    bad = np.nonzero(status & LCU_BAD)[0]
    units = np.nonzero((status & LCU_BAD == 0) & (status != 0))[0]
    out["bad_lcus"], out["first_bad_lcu"] = len(bad), bad[0] if len(bad) else NONE
    out["bad_units"], out["first_bad_unit_lcu"] = int(status[units].astype(np.int64).sum()), units[0] if len(units) else NONE
    return out


def source_planes(works, status, w, h):
    """the LCUs' source samples as planes; a refused LCU scatters nothing (None marks samples the tail leaves as they were)"""
    cols = (w + 63) // 64
    dt = works["src_y"].dtype
    planes = [np.zeros((h, w), dt), np.zeros((h // 2, w // 2), dt), np.zeros((h // 2, w // 2), dt)]
    known = [np.zeros(p.shape, bool) for p in planes]
    for i, wk in enumerate(works):
        if status[i] & LCU_BAD:
            continue
        ox, oy = (i % cols) * 64, (i // cols) * 64
        lw, lh = min(64, w - ox), min(64, h - oy)
        for p, nm in enumerate(("src_y", "src_cb", "src_cr")):
            sh = 1 if p else 0
            blk = wk[nm].reshape(64 >> sh, 64 >> sh)[:lh >> sh, :lw >> sh]
            planes[p][oy >> sh:(oy + lh) >> sh, ox >> sh:(ox + lw) >> sh] = blk
            known[p][oy >> sh:(oy + lh) >> sh, ox >> sh:(ox + lw) >> sh] = True
    return planes, known


def stages_refused(stages, pad, has_ref, origin_x, origin_y):
    """why svt_amd_encdec_picture_tail_launch refuses these stage bits before it looks at anything else; None = they pass"""
    if stages == 0 or stages > 15 or pad:
        return "stages"
    if stages & SAO_APPLY and not (stages & SAO_DECIDE and stages & DEBLOCK):
        return "apply"
    if stages & REFERENCE and not (has_ref and 8 <= origin_x <= 256 and 8 <= origin_y <= 256 and origin_x % 2 == 0 and origin_y % 2 == 0):
        return "reference"
    return None


def latest_stage(stages, deblocked, sao_done):
    """the object's (deblocked, sao_done) after a tail, and which planes SVT_AMD_TAIL_REFERENCE pads: 'fin', 'dbk' or 'rec'"""
    deblocked = deblocked or bool(stages & DEBLOCK)
    sao_done = sao_done or bool(stages & SAO_APPLY)
    return deblocked, sao_done, "fin" if sao_done else "dbk" if deblocked else "rec"
