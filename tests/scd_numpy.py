"""SceneTransitionDetector (Codec/EbPictureDecisionProcess.c:73-258) restated from the reference, line by line and loop by loop, with every width spelled out:
Python integers masked to the reference's EB_U32 where it has one.  Independent of svt-hevc_amd/csrc/scd_logic.h - no closed form is used here: the region
size is accumulated iteration by iteration as the reference's two `+=` do (:155-156), on an offset that is computed from the size the iterations before left
(:147-153).  Pinned on the reference's own results by tests/test_scd_cpu.py (tests/golden/scd_*.npz)."""
import functools

import numpy as np

import scd_records as R

M32 = 0xFFFFFFFF


def s32(v):
    """(EB_S32) of an EB_U32"""
    v &= M32
    return v - (1 << 32) if v >> 31 else v


def _abs_sum(cur, past):
    """the EB_U32 sum over the 256 bins of ABS((EB_S32)cur - (EB_S32)past)"""
    return int(np.abs(cur.astype(np.int32).astype(np.int64) - past.astype(np.int32).astype(np.int64)).sum()) & M32


def region_count_threshold(regions, scd_mode):
    """:126-128: (EB_U32)(((float)(regions * P) / 100) + 0.5) - a float division, the sum in double, truncated"""
    p = 75 if scd_mode == 2 else 50
    return int(np.float64(np.float32(regions * p) / np.float32(100)) + np.float64(0.5))


def detector_call(state, w, h, rw, rh, scd_mode, past, cur, future):
    """one call.  state: dict(avg, avg_cb, avg_cr: [rw][rh] lists of int, reset: bool), updated in place; a picture: dict(luma [rw * rh][256],
    chroma [rw * rh][2][256], avg [64] bytes, detect) -> (return value, per region: class and the three sums, abrupt count, scene count, the vote threshold)"""
    threshold = region_count_threshold(rw * rh, scd_mode)
    region_width, region_height = w // rw, h // rh                                            # :130-131, once
    cur_var, past_var = int(cur["detect"]["pic_avg_variance"][0]), int(past["detect"]["pic_avg_variance"][0])
    abrupt_count = scene_count = 0
    classes, sums = [], []
    for wi in range(rw):
        for hi in range(rh):
            r = wi * rh + hi
            width_offset = (w - rw * region_width) & M32 if wi == rw - 1 else 0               # :147-149, on the CURRENT regionWidth
            height_offset = (h - rh * region_height) & M32 if hi == rh - 1 else 0             # :151-153
            region_width = (region_width + width_offset) & M32                                # :155
            region_height = (region_height + height_offset) & M32                             # :156
            units = ((region_width * region_height) & M32) >> 12                              # NUM64x64INPIC: an EB_U32 product
            noisy = abs(cur_var - past_var) > 390 and (cur_var > 1500 or past_var > 1500)     # :160-161, EB_S64
            th = ((4500 if noisy else 3000) * units) & M32                                    # :162-163
            th_chroma = th // 4                                                               # :165
            ahd = _abs_sum(cur["luma"][r], past["luma"][r])                                   # :167-172
            ahd_cb = _abs_sum(cur["chroma"][r][0], past["chroma"][r][0])
            ahd_cr = _abs_sum(cur["chroma"][r][1], past["chroma"][r][1])
            if state["reset"]:                                                                # :174-178
                state["avg"][wi][hi], state["avg_cb"][wi][hi], state["avg_cr"][wi][hi] = ahd, ahd_cb, ahd_cr
            err = abs(s32(state["avg"][wi][hi]) - s32(ahd))                                   # :180-182
            err_cb = abs(s32(state["avg_cb"][wi][hi]) - s32(ahd_cb))
            err_cr = abs(s32(state["avg_cr"][wi][hi]) - s32(ahd_cr))
            abrupt = (err > th and ahd >= err) or (err_cb > th_chroma and ahd_cb >= err_cb) or (err_cr > th_chroma and ahd_cr >= err_cr)   # :185-187
            gradual = not abrupt and err > (th >> 1) and ahd >= err                           # :192
            if abrupt:                                                                        # :196-214: the running average is left alone
                f, c, p = int(future["avg"][r]), int(cur["avg"][r]), int(past["avg"][r])
                aid_fp, aid_fpr, aid_pp = abs(f - p) & 0xFF, abs(f - c) & 0xFF, abs(c - p) & 0xFF
                if aid_fp < 5 and aid_fpr >= 5 and aid_pp >= 5:
                    cls = R.FLASH
                elif aid_fpr < 3 and aid_pp < 3:
                    cls = R.FADE
                else:
                    cls = R.SCENE
            else:                                                                             # :215-232: all three arms are one statement
                state["avg"][wi][hi] = ((3 * state["avg"][wi][hi] + ahd) & M32) // 4
                cls = R.GRADUAL if gradual else R.NONE
            abrupt_count += abrupt
            scene_count += cls == R.SCENE
            classes.append(cls), sums.append((ahd, ahd_cb, ahd_cr))
    state["reset"] = abrupt_count >= threshold                                                # :243-248
    return scene_count >= threshold, classes, sums, abrupt_count, scene_count, threshold


@functools.lru_cache(maxsize=None)
def restated(name):
    """the three arrays of a case of scd_records.CASES; shared, so nobody writes into them"""
    w, h, rw, rh, mode = R.CASES[name][:5]
    return scene_detect(w, h, rw, rh, mode, R.case_windows(name))


def same_as_reference(got, ref, tag):
    """three arrays - the restatement's or the device's - against a fixture (scd_records.load_case): flag, reset and the three running averages after every job"""
    assert np.array_equal(got["picture"]["scene_change"], ref["scene_change"]), (tag, "scene_change")
    assert np.array_equal(got["picture"]["reset_running_avg"], ref["reset_running_avg"]) and np.array_equal(got["state"]["reset_running_avg"], ref["reset_running_avg"]), (tag, "reset")
    for f in ("ahd_running_avg", "ahd_running_avg_cb", "ahd_running_avg_cr"):
        assert np.array_equal(got["state"][f], ref[f]), (tag, f)


def state_from_record(rec, rw, rh):
    """SvtAmdScdState (or None: the constructor's state) -> the [rw][rh] lists"""
    if rec is None:
        rec = R.constructor_state()
    rec = rec.reshape(-1)[0]
    grid = lambda f: [[int(rec[f][wi * rh + hi]) for hi in range(rh)] for wi in range(rw)]  # noqa: E731
    return dict(avg=grid("ahd_running_avg"), avg_cb=grid("ahd_running_avg_cb"), avg_cr=grid("ahd_running_avg_cr"), reset=bool(rec["reset_running_avg"]))


def scene_detect(w, h, rw, rh, scd_mode, windows, state_in=None):
    """the entry: `windows` = the (past, current, future) pictures of consecutive calls -> dict(picture, ahd, state) as the three output arrays hold them"""
    n = len(windows)
    state = state_from_record(state_in, rw, rh)
    out = dict(picture=np.zeros(n, R.PIC_DTYPE), ahd=np.zeros((n, 16, 3), R.AHD_DTYPE), state=np.zeros(n, R.STATE_DTYPE))
    for i, (past, cur, future) in enumerate(windows):
        flag, classes, sums, abrupt, scene, threshold = detector_call(state, w, h, rw, rh, scd_mode, past, cur, future)
        p, s = out["picture"][i], out["state"][i]
        p["scene_change"], p["reset_running_avg"], p["abrupt_regions"], p["scene_regions"], p["region_count_threshold"] = flag, state["reset"], abrupt, scene, threshold
        p["region_class"][:rw * rh] = classes
        out["ahd"][i, :rw * rh] = sums
        for f, key in (("ahd_running_avg", "avg"), ("ahd_running_avg_cb", "avg_cb"), ("ahd_running_avg_cr", "avg_cr")):
            s[f][:rw * rh] = [state[key][wi][hi] for wi in range(rw) for hi in range(rh)]
        s["reset_running_avg"] = state["reset"]
    return out
