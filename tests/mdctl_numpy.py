"""The mode decision's per-LCU controls restated in numpy: what svt_amd_md_controls_batch_launch (svt-hevc_amd/csrc/mdctl_kernels.hip) assembles on the device and
integration/svt_md_fill.h:svt_md_fill_lcu reads out of the reference's control sets, with the reference functions behind it spelled out - DeriveContouringClass
(Codec/EbModeDecisionConfiguration.c:395), ConfigureChroma (Codec/EbModeDecisionProcess.c:383), isEdgeLcu / isCompleteLcu (Codec/EbSequenceControlSet.c:206-213),
the tile starts and ConfigureLcuEdgeInfo (Codec/EbPictureControlSet.c:743, :36) - and the summary the mode-decision call takes of a bound device array
(SvtAmdMdCtlCheck).  Pinned on the reference's records by tests/test_mdctl_cpu.py."""
import numpy as np

import mdctl_records as R
from mdc_records import MD_SCAN, INVALID_AURA_STATUS, PICT_LCU_SWITCH, PICT_FULL85, geometry, unit_validity

ANTI_CONTOURING_TH_0, ANTI_CONTOURING_TH_1, ANTI_CONTOURING_TH_2 = 16 * 16, 32 * 32, 2 * 32 * 32       # Codec/EbDefinitions.h:779-781
CHROMA_MODE_FULL, CHROMA_MODE_BEST = 1, 2
DEPTH = np.array([u[0] for u in MD_SCAN])


def tile_flags(wl, hl, tile_cols, tile_rows):
    """-> tile_left, tile_top, tile_right per LCU: the uniformly spaced starts c * columns / tile_cols, an LCU against the tile that holds it"""
    col_start = [c * wl // tile_cols for c in range(tile_cols + 1)]
    row_start = [r * hl // tile_rows for r in range(tile_rows + 1)]
    left, top, right = np.zeros(wl * hl, np.uint8), np.zeros(wl * hl, np.uint8), np.zeros(wl * hl, np.uint8)
    for r in range(tile_rows):
        for c in range(tile_cols):
            for y in range(row_start[r], row_start[r + 1]):
                for x in range(col_start[c], col_start[c + 1]):
                    left[y * wl + x], top[y * wl + x], right[y * wl + x] = x == col_start[c], y == row_start[r], x == col_start[c + 1] - 1
    return left, top, right


def fixed_leaves(w, h, depth_mode):
    """Forward85 / 84CuToModeDecisionLCU (Codec/EbModeDecisionConfiguration.c:370-484): the valid units from depth 0 / 1 on in MD-scan order, split above 8x8"""
    valid = unit_validity(w, h) & (DEPTH >= (0 if depth_mode == PICT_FULL85 else 1))
    out = np.zeros(len(valid), R.MD_LCU_DTYPE)
    for i in range(len(valid)):
        units = np.flatnonzero(valid[i])
        out["leaf_count"][i] = len(units)
        out["leaf_index"][i, :len(units)], out["leaf_split"][i, :len(units)] = units, DEPTH[units] < 3
    return out


def contouring(energy, homogeneous, edge):
    """DeriveContouringClass of leaves 1, 22, 43, 64: [lcus][4]; energy: [lcus][5] of 64-bit values"""
    e = energy[:, 1:5].astype(np.uint64)
    at_edge = np.where(e < ANTI_CONTOURING_TH_1, 2, np.where(e < ANTI_CONTOURING_TH_2, 3, np.where(e < ANTI_CONTOURING_TH_1 + ANTI_CONTOURING_TH_2, 3, 0)))
    inside = np.where(e < ANTI_CONTOURING_TH_0, 1, np.where(e < ANTI_CONTOURING_TH_1, 2, np.where(e < ANTI_CONTOURING_TH_2, 3, 0)))
    return np.where((homogeneous != 0)[:, None], np.where(edge[:, None], at_edge, inside), 0).astype(np.uint8)


def md_controls(w, h, rec, jb):
    """-> MD_LCU_DTYPE[lcus] of one picture: rec of mdctl_records.make_inputs (or downloaded records under the same keys), jb of mdctl_records.job"""
    wl, hl, col, row, complete, edge = geometry(w, h)
    n = wl * hl
    mdc = rec["mdc_lcu"]
    if mdc is not None:
        out = np.zeros(n, R.MD_LCU_DTYPE)
        for f in ("leaf_count", "leaf_index", "leaf_split"):
            out[f] = mdc[f]
        aura = mdc["aura_status"].astype(int)
        out["lcu_md_mode"] = mdc["lcu_md_mode"] if jb["depth_mode"] == PICT_LCU_SWITCH else 0
    else:
        out = fixed_leaves(w, h, jb["depth_mode"])
        aura = np.full(n, INVALID_AURA_STATUS)
    stationary = rec["stationary_edge"][:n].astype(int) if rec["stationary_edge"] is not None else np.zeros(n, int)
    sticky = rec["sticky"].astype(int) if rec["sticky"] is not None else np.zeros(n, int)
    sbo, detect, stats = rec["sbo_lcu"], rec["detect"], rec["stats"]
    out["tile_left"], out["tile_top"], out["tile_right"] = tile_flags(wl, hl, jb["tile_cols"], jb["tile_rows"])
    out["is_complete"] = complete
    out["complexity_status_2"] = sbo["complex_lcu"] == 2
    if rec["irc_lcu"] is not None:
        out["contouring_class"] = contouring(rec["ac_energy"].reshape(n, 5), rec["irc_lcu"]["homogeneous_over_time"], edge)
    high_luma, high_chroma = ((sticky & 1) != 0) | (sbo["high_luma"] != 0), ((sticky & 2) != 0) | (sbo["high_chroma"] != 0)
    c0, c1, c2 = stationary != 0, (detect["homogeneous"] != 0) & high_chroma, ~high_luma
    c3 = (int(np.ravel(rec["sbo_pic"]["grass_percentage"])[0]) > 60) | (aura == 1) | bool(jb["pan"])
    level = jb["chroma_level"]
    full = (np.ones(n, bool), np.zeros(n, bool), c0 | c1 | c2, c0 | c1, c2 | c3, c0)[level]
    out["chroma_encode_mode"] = np.where(full & (not jb["c422"]), CHROMA_MODE_FULL, CHROMA_MODE_BEST)
    out["restrict_intra_global_motion"] = bool(jb["pan"] or jb["tilt"]) & (sbo["non_moving_index"] < 2) & (stats["y_mean"][:, 0] < 50)
    out["skip_small_cu"] = (aura == 0) & (stationary == 0)
    out["cmplx_noise"] = sbo["cmplx_status"] == 4
    out["variance_below_200"] = stats["variance"][:, 0] < 200
    out["edge_block"] = detect["edge_block_num"] != 0
    out["no_stop_split"] = (sbo["isolated_non_homogeneous"] != 0) | ((jb["cls"] < 3) & (aura == 1))
    return out


def lcu_supported(depth_mode, lcu):
    """md_lcu_supported (svt-hevc_amd/csrc/md_logic.h) of one record"""
    if lcu["chroma_encode_mode"] not in (1, 2):
        return False
    if depth_mode == 0:
        return lcu["lcu_md_mode"] not in (0, 3, 4)
    return depth_mode in (1, 2, 5)


def check_summary(lcus, depth_mode, inter):
    """SvtAmdMdCtlCheck of an array of records, vectorised -> CHECK_DTYPE scalar"""
    n = len(lcus)
    count = lcus["leaf_count"].astype(int)
    bad_count = (count < 1) | (count > 85)
    idx = lcus["leaf_index"].astype(int)
    k = np.arange(85)[None, :]
    used = k < np.minimum(count, 85)[:, None]
    prev = np.concatenate([np.full((n, 1), -1), idx[:, :-1]], 1)
    bad_list = (used & ((idx >= 85) | (idx <= prev))).any(1)
    chroma_ok = (lcus["chroma_encode_mode"] == 1) | (lcus["chroma_encode_mode"] == 2)
    mode = lcus["lcu_md_mode"].astype(int)
    supported = chroma_ok & (((mode != 0) & (mode != 3) & (mode != 4)) if depth_mode == 0 else depth_mode in (1, 2, 5))
    out = np.zeros((), R.CHECK_DTYPE)
    out["bad_leaf_count"], out["bad_leaf_list"] = bad_count.sum(), bad_list.sum()
    out["md_mode"] = np.bincount(np.minimum(mode, 15), minlength=16)
    out["bad_chroma"], out["tiles"] = (~chroma_ok).sum(), ((lcus["tile_left"] != 0) & (lcus["tile_top"] != 0)).sum()
    kind = np.where(bad_count, 0, np.where(bad_list, 1, np.where(~supported & bool(inter), 2, 3)))
    offenders = np.flatnonzero(kind < 3)
    out["first_bad"], out["first_kind"] = (offenders[0], kind[offenders[0]]) if len(offenders) else (0xFFFFFFFF, 0)
    return out


def check_summary_loop(lcus, depth_mode, inter):
    """the same, as the host loop of svt_amd_md_encode_picture walks the records: one LCU at a time, the first refusal ends nothing here - everything is counted"""
    out = np.zeros((), R.CHECK_DTYPE)
    out["first_bad"] = 0xFFFFFFFF
    for i, L in enumerate(lcus):
        count = int(L["leaf_count"])
        bad_count = count < 1 or count > 85
        bad_list = any(int(L["leaf_index"][j]) >= 85 or (j and int(L["leaf_index"][j]) <= int(L["leaf_index"][j - 1])) for j in range(min(count, 85)))
        out["bad_leaf_count"] += bad_count
        out["bad_leaf_list"] += bad_list
        out["md_mode"][min(int(L["lcu_md_mode"]), 15)] += 1
        out["bad_chroma"] += int(L["chroma_encode_mode"]) not in (1, 2)
        out["tiles"] += bool(L["tile_left"]) and bool(L["tile_top"])
        kind = 0 if bad_count else 1 if bad_list else 2 if inter and not lcu_supported(depth_mode, L) else None
        if kind is not None and out["first_bad"] == 0xFFFFFFFF:
            out["first_bad"], out["first_kind"] = i, kind
    return out
