"""-m gpu: the batched, stream-ordered side statistics (svt_amd_side_stats_batch_launch; svt-hevc_amd/csrc/side_kernels.hip) - block statistics, AC energy,
luma region histograms and the collocated zero-motion SAD of up to 256 pictures per call - against (1) what the REFERENCE encoder gathered
(tests/golden/pa_*.npz), (2) the reference's ComputeNxMSatdSadLCU, (3) the CPU checker, (4) the three blocking single-picture entries byte for byte;
(5) per-picture selection and the parameter checks, (6) three lanes under a root without a stream, (7) extreme pictures.  Everything is bit-exact."""
import ctypes as C
import os

import numpy as np
import pytest

import sidelib as L
import svtlib as S
from gpu_util import default_params, upload
from pa_batch_util import is_sentinel as _sentinel, make_context as _context, ok as _ok, refused as _refused
from test_oracle_pa import CASES, oracle_picture as pa_oracle
from test_oracle_sbo import oracle_picture as sbo_oracle
from test_oracle_zz import oracle_zz

pytestmark = pytest.mark.gpu
vp = C.c_void_p
KINDS4 = ("objects", "noise", "motion", "static")


@pytest.fixture(scope="module")
def lib(product):
    return L.declare(product)


def _mixed_frames(n, w, h, seed):
    """n distinct frames of mixed content: up to eight generated ones (the four kinds, two times each), the rest shifted copies of them"""
    base = [S.gen_luma(KINDS4[i % 4], w, h, 2 + i // 4, seed + i % 4) for i in range(min(n, 8))]
    return [np.ascontiguousarray(np.roll(base[i % 8], (5 * (i // 8), 3 * (i // 8)), (0, 1))) for i in range(n)]


def _assert_equals_checker(oracle, got, i, frame, prev, w, h, what):
    """picture i of a batch (4 x 4 regions) against the CPU checker"""
    stats, hist, ravg, total = pa_oracle(oracle, np.ascontiguousarray(np.pad(frame, ((0, 64), (0, 64)), mode="edge")), w, h)
    assert np.array_equal(got["block_stats"][i]["variance"], stats["variance"]), (what, i, np.argwhere(got["block_stats"][i]["variance"] != stats["variance"])[:4].tolist())
    assert np.array_equal(got["block_stats"][i]["y_mean"], stats["y_mean"]) and not got["block_stats"][i]["pad"].any(), (what, i)
    assert np.array_equal(got["histogram"][i], hist), (what, i, "histogram")
    assert np.array_equal(got["region_average"][i][:16].reshape(4, 4), ravg) and not got["region_average"][i][16:].any(), (what, i)
    assert int(got["sum_luma"][i]) == total, (what, i)
    energy = sbo_oracle(oracle, frame, w, h)
    assert np.array_equal(got["ac_energy"][i], energy), (what, i, np.argwhere(got["ac_energy"][i] != energy)[:4].tolist())
    if prev is not None:
        zz = oracle_zz(oracle, frame, prev)
        assert got["zz"][i].tobytes() == zz.tobytes(), (what, i, "zz")


# ---- 1. the reference's own records ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_one_batch_gives_what_the_encoder_gathered(lib, name):
    g = np.load(os.path.join(S.GOLDEN_DIR, "pa_%s.npz" % name))
    kind, w, h, seed = g["clip"][0], int(g["clip"][1]), int(g["clip"][2]), int(g["clip"][4])
    pictures = g["picture_number"].tolist()
    n = len(pictures)
    ctx = _context(lib, w, h, n)
    try:
        for i, p in enumerate(pictures):
            upload(lib, ctx, i, S.gen_luma(kind, w, h, int(p), seed))
        got = L.run_batch(lib, ctx, L.all_jobs(list(range(n))), w, h)          # ONE batch for the whole clip
        for i, p in enumerate(pictures):
            assert np.array_equal(got["block_stats"][i]["variance"], g["variance"][i]), (name, p, np.argwhere(got["block_stats"][i]["variance"] != g["variance"][i])[:4].tolist())
            assert np.array_equal(got["block_stats"][i]["y_mean"], g["y_mean"][i]), (name, p)
            assert np.array_equal(got["histogram"][i], g["histogram"][i]), (name, p, "histogram")
            assert np.array_equal(got["region_average"][i][:16].reshape(4, 4), g["region_average"][i]), (name, p)
            assert int(g["average_intensity"][i]) == (int(got["sum_luma"][i]) + ((w * h) >> 1)) // (w * h), (name, p)
    finally:
        lib.svt_amd_context_destroy(ctx)


# ---- 2. the reference symbol -----------------------------------------------------------------------------------------------------------------

def test_batch_energies_match_the_reference_symbol(lib):
    ref = S.load_ref()
    if ref is None:
        pytest.skip("oracle/_ref/libsvtref.so not on this box")
    ref.ComputeNxMSatdSadLCU.restype, ref.ComputeNxMSatdSadLCU.argtypes = C.c_uint64, [vp, C.c_uint32, C.c_uint32, C.c_uint32]
    w, h = 640, 384
    frames = [np.ascontiguousarray(S.gen_luma("objects", w, h, t, 2)) for t in (5, 6, 7)]
    ctx = _context(lib, w, h, 3)
    try:
        for i, f in enumerate(frames):
            upload(lib, ctx, i, f)
        out = L.run_batch(lib, ctx, L.all_jobs([0, 1, 2]), w, h)["ac_energy"]
    finally:
        lib.svt_amd_context_destroy(ctx)
    assert out.shape == (3, 60, 5)
    for i, luma in enumerate(frames):
        for k in range(60):
            x, y = 64 * (k % 10), 64 * (k // 10)
            assert out[i, k, 0] == ref.ComputeNxMSatdSadLCU(luma[y:, x:].ctypes.data, w, 64, 64), (i, k)
            for q in range(4):
                assert out[i, k, 1 + q] == ref.ComputeNxMSatdSadLCU(luma[y + 32 * (q >> 1):, x + 32 * (q & 1):].ctypes.data, w, 32, 32), (i, k, q)


# ---- 3. the CPU checker ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,n", [(416, 240, 1), (416, 240, 3), (832, 480, 1), (832, 480, 3), (1920, 1080, 3), (1920, 1080, 64), (3840, 2160, 1), (3840, 2160, 8)])
def test_mixed_content_batches_match_the_checker(lib, oracle, w, h, n):
    frames = _mixed_frames(n, w, h, 40 + n)
    ctx = _context(lib, w, h, n)
    try:
        for i, f in enumerate(frames):
            upload(lib, ctx, i, f)
        # the previous picture of picture 0 is the LAST one of the batch (a batch of one: no zz-SAD)
        got = L.run_batch(lib, ctx, L.all_jobs(list(range(n)), first_prev=n - 1 if n > 1 else -1), w, h)
    finally:
        lib.svt_amd_context_destroy(ctx)
    for i, f in enumerate(frames):
        _assert_equals_checker(oracle, got, i, f, frames[i - 1] if n > 1 else None, w, h, (w, h, n))
    assert (got["ac_energy"][:, :, 0] < L.NOT_COMPUTED).sum() == n * (w // 64) * (h // 64)
    if n == 1:
        assert (got["zz"].view(np.uint8) == L.SENTINEL).all()


# ---- 4. the blocking single-picture entries --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,rw,rh", [(416, 240, 4, 4), (416, 240, 3, 5), (1920, 1080, 4, 4), (1920, 1080, 8, 8)])
def test_batch_equals_the_blocking_entries_byte_for_byte(lib, w, h, rw, rh):
    n = 6
    frames = _mixed_frames(n, w, h, 7)
    ctx = _context(lib, w, h, n)
    first = second = None
    try:
        for i, f in enumerate(frames):
            upload(lib, ctx, i, f)
        order = [4, 1, 5, 0, 3, 2]                                              # slots in mixed order, previous pictures anywhere
        spec_a = [(s, order[(i + 2) % n], 1, 1, 1) for i, s in enumerate(order)]
        spec_b = [(s, (s + 1) % n, 1, 1, 1) for s in range(3)]
        # two batches queued back to back on the one lane, nothing waited for in between: the second one's table must not reach the first one's kernels
        first, second = L.DeviceArrays(lib, ctx, n, w, h, rw, rh), L.DeviceArrays(lib, ctx, 3, w, h, rw, rh)
        _ok(lib, L.launch(lib, ctx, L.make_jobs(spec_a), first, rw, rh))
        _ok(lib, L.launch(lib, ctx, L.make_jobs(spec_b), second, rw, rh))
        got_a, got_b = first.download(), second.download()
        for got, spec in ((got_a, spec_a), (got_b, spec_b)):
            for i, (s, prev, _, _, _) in enumerate(spec):
                L.assert_equals_blocking(lib, ctx, got, i, s, prev, w, h, rw, rh, (w, h, rw, rh))
        assert int(got_a["histogram"].sum()) == n * ((w // 4) * (h // 4) + rw * rh * 256) * 16
    finally:
        for a in (first, second):
            if a:
                a.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 5. selection and the parameter checks ---------------------------------------------------------------------------------------------------

def test_selection_per_picture_and_refused_batches_queue_nothing(lib):
    w, h, n = 832, 480, 6
    frames = _mixed_frames(n, w, h, 11)
    ctx = _context(lib, w, h, n + 2)            # slot n: a picture of another size, slot n + 1: no picture
    arrays = None
    try:
        for i, f in enumerate(frames):
            upload(lib, ctx, i, f)
        upload(lib, ctx, n, S.gen_luma("motion", 416, 240, 0, 3))
        #        slot prev stats energy histogram
        spec = [(0, -1, 1, 1, 1),
                (1, 0, 0, 1, 1),
                (2, 1, 1, 0, 1),
                (3, -1, 1, 1, 0),
                (4, 3, 0, 0, 0),
                (5, -1, 0, 0, 0)]               # nothing at all of the last picture
        arrays = L.DeviceArrays(lib, ctx, n, w, h)
        _ok(lib, L.launch(lib, ctx, L.make_jobs(spec), arrays))
        got = arrays.download()
        for i, (s, prev, bs, ac, hist) in enumerate(spec):
            stats, bhist, ravg, total, energy, zz = L.blocking_picture(lib, ctx, s, prev, w, h)
            assert got["block_stats"][i].tobytes() == stats.tobytes() if bs else _sentinel(got["block_stats"][i]), (i, "block_stats")
            assert got["ac_energy"][i].tobytes() == energy.tobytes() if ac else _sentinel(got["ac_energy"][i]), (i, "ac_energy")
            assert got["zz"][i].tobytes() == zz.tobytes() if prev >= 0 else _sentinel(got["zz"][i]), (i, "zz")
            if hist:
                assert got["histogram"][i].tobytes() == bhist.tobytes() and int(got["sum_luma"][i]) == total, (i, "histogram")
                assert got["region_average"][i].tobytes() == ravg.tobytes() + bytes(48), (i, "region_average")
            else:
                assert _sentinel(got["histogram"][i]) and _sentinel(got["region_average"][i]) and _sentinel(got["sum_luma"][i:i + 1]), (i, "histogram")

        # refused batches: every wanted result without its array, slots without a picture or of another size, bad regions, bad slots
        arrays.fill()
        everything = [(i, i - 1, 1, 1, 1) for i in range(n)]

        def refused(spec, missing=None, rw=4, rh=4):
            t = arrays.table()
            if missing:
                setattr(t, missing, None)
            _refused(lib, L.launch(lib, ctx, L.make_jobs(spec), t, rw, rh), "svt_amd_side_stats_batch_launch", (spec, missing))

        for missing in ("block_stats", "ac_energy", "zz", "histogram"):
            refused(everything, missing)
        refused([(0, -1, 1, 0, 0), (1, -1, 1, 0, 0), (2, -1, 0, 1, 0)], "ac_energy")   # only the LAST job wants what is missing
        refused(everything[:3] + [(n, -1, 1, 1, 1)])                                   # mixed geometry
        refused([(n, -1, 1, 1, 1)] + everything[:3])
        refused([(1, n, 1, 1, 1)])                                                     # the previous picture has another size
        refused([(1, n + 1, 1, 1, 1)])                                                 # the previous slot holds no picture
        refused([(n + 1, -1, 1, 1, 1)])                                                # the slot holds no picture
        refused([(n + 2, -1, 1, 1, 1)])                                                # no such slot
        refused([(-1, -1, 1, 1, 1)])
        refused([(1, n + 2, 1, 1, 1)])
        refused(everything, rw=0)
        refused(everything, rw=9, rh=8)
        _ok(lib, lib.svt_amd_synchronize(ctx))
        for k in range(6):
            assert _sentinel(arrays.raw(k)), ("a refused batch wrote", L.KINDS[k])
        # results the caller does not ask for need no array; region averages and the luma sum are optional beside the histogram
        t = arrays.table()
        t.block_stats = t.zz = t.region_average = t.sum_luma = None
        _ok(lib, L.launch(lib, ctx, L.make_jobs([(i, -1, 0, 1, 1) for i in range(n)]), t))
        got = arrays.download()
        for i in range(n):
            stats, bhist, ravg, total, energy, _ = L.blocking_picture(lib, ctx, i, -1, w, h)
            assert got["ac_energy"][i].tobytes() == energy.tobytes() and got["histogram"][i].tobytes() == bhist.tobytes(), i
        assert _sentinel(got["block_stats"]) and _sentinel(got["zz"]) and _sentinel(got["region_average"]) and _sentinel(got["sum_luma"])
        # ... and a following complete batch on the same context is right
        arrays.fill()
        _ok(lib, L.launch(lib, ctx, L.make_jobs(everything), arrays))
        got = arrays.download()
        for i in range(n):
            L.assert_equals_blocking(lib, ctx, got, i, i, i - 1, w, h, what="after the refused batches")
        assert _sentinel(got["zz"][0])
    finally:
        if arrays:
            arrays.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 6. lanes --------------------------------------------------------------------------------------------------------------------------------

def _bytes(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n,))


def test_three_lanes_under_a_root_without_stream_four_batches(lib):
    """the three-lane pattern of test_gpu_lane_streams.py (copy-in lane -> compute lane -> copy-out lane, two sets of slots and buffers, lane events) with
    the side batch behind the ME / OIS batches on the compute lane and one download per kind on the copy-out lane, four batches queued back to back with
    the slots reused; the previous picture of a batch's first picture is the LAST slot of the batch before (the other set of slots) - the dependency the
    zero-motion SAD really has.  Every batch in pinned memory equals what one lane computes."""
    W, H, B, NSETS, NB = 1920, 1080, 4, 2, 4
    sizes = L.numpy_sizes(W, H, 4, 4)
    frames = _mixed_frames(NB * B, W, H, 21)
    p = default_params(W, H, num_lists=2, temporal_layer_index=1)
    op = S.OisParams()
    op.luma_width, op.luma_height, op.ois_th_set, op.temporal_layer_index = W, H, 1, 1
    root, one = vp(), vp()
    _ok(lib, lib.svt_amd_context_create(0, W, 1088, NSETS * B, C.byref(root)))
    lanes = [vp(), vp(), vp()]
    sets, pinned, h_in = [], [], vp()
    try:
        for lane in lanes:
            _ok(lib, lib.svt_amd_context_fork(root, C.byref(lane)))
        lane_in, lane_k, lane_out = lanes
        _ok(lib, lib.svt_amd_host_alloc(root, NB * B * W * H, C.byref(h_in)))
        _bytes(h_in, NB * B * W * H)[:] = np.concatenate([f.reshape(-1) for f in frames])
        for k in range(NSETS):
            d_stage = vp()
            _ok(lib, lib.svt_amd_device_alloc(root, B * W * H, C.byref(d_stage)))
            slots = (C.c_int * B)(*[k * B + i for i in range(B)])
            ptrs = (vp * B)(*[d_stage.value + i * W * H for i in range(B)])
            jobs, ojobs = (S.MeJob * B)(), (S.OisJob * B)()
            for i in range(B):
                jobs[i].params, jobs[i].cur_slot = p, slots[i]
                jobs[i].ref_slot[0], jobs[i].ref_slot[1] = slots[(i - 1) % B], slots[(i + 1) % B]
                ojobs[i].params, ojobs[i].cur_slot = op, slots[i]
            sets.append(dict(d_stage=d_stage, slots=slots, ptrs=ptrs, jobs=jobs, ojobs=ojobs, arrays=L.DeviceArrays(lib, root, B, W, H)))
        for b in range(NB):
            pinned.append([vp() for _ in range(6)])
            for q in range(6):
                _ok(lib, lib.svt_amd_host_alloc(root, B * sizes[q], C.byref(pinned[b][q])))
                _bytes(pinned[b][q], B * sizes[q])[:] = 0
        EV_STAGE, EV_READY = 0, NSETS
        for b in range(NB):
            k = b % NSETS
            X = sets[k]
            prev_last = -1 if b == 0 else int(sets[(b - 1) % NSETS]["slots"][B - 1])
            side = L.all_jobs([int(s) for s in X["slots"]], first_prev=prev_last)
            table = X["arrays"].table()
            _ok(lib, lib.svt_amd_lane_event_wait(lane_in, lane_k, EV_STAGE + k))
            _ok(lib, lib.svt_amd_device_upload_async(lane_in, X["d_stage"], vp(h_in.value + b * B * W * H), B * W * H))
            _ok(lib, lib.svt_amd_lane_event_record(lane_in, EV_STAGE + k))
            _ok(lib, lib.svt_amd_lane_event_wait(lane_k, lane_in, EV_STAGE + k))
            _ok(lib, lib.svt_amd_lane_event_wait(lane_k, lane_out, EV_STAGE + k))
            _ok(lib, lib.svt_amd_picture_upload_device_batch(lane_k, B, X["slots"], X["ptrs"], W, W, H))
            _ok(lib, lib.svt_amd_lane_event_record(lane_k, EV_STAGE + k))
            _ok(lib, lib.svt_amd_me_batch_launch(lane_k, X["jobs"], B))
            _ok(lib, lib.svt_amd_ois_batch_launch(lane_k, X["ojobs"], B))
            _ok(lib, lib.svt_amd_side_stats_batch_launch(lane_k, side, B, 4, 4, C.byref(table)))
            _ok(lib, lib.svt_amd_lane_event_record(lane_k, EV_READY + k))
            _ok(lib, lib.svt_amd_lane_event_wait(lane_out, lane_k, EV_READY + k))
            for q in range(6):                                                  # one copy per kind for the whole batch
                _ok(lib, lib.svt_amd_device_download_async(lane_out, pinned[b][q], X["arrays"].ptr[q], B * sizes[q]))
            _ok(lib, lib.svt_amd_lane_event_record(lane_out, EV_STAGE + k))
        for lane in lanes:
            _ok(lib, lib.svt_amd_synchronize(lane))
        _ok(lib, lib.svt_amd_synchronize(root))                                # the root queued nothing: it holds no stream and this returns at once
        # one lane: every picture in a slot of its own, one batch on a context of its own; a few pictures also through the blocking entries
        _ok(lib, lib.svt_amd_context_create(0, W, 1088, NB * B, C.byref(one)))
        for i, f in enumerate(frames):
            upload(lib, one, i, f)
        want = L.run_batch(lib, one, L.all_jobs(list(range(NB * B))), W, H)
        for i in (0, B - 1, B, NB * B - 1):
            L.assert_equals_blocking(lib, one, want, i, i, i - 1, W, H, what="one lane")
        for b in range(NB):
            got = L.views([_bytes(pinned[b][q], B * sizes[q]).reshape(B, sizes[q]) for q in range(6)], B, 4, 4)
            for name in L.KINDS:
                assert got[name].tobytes() == want[name][b * B:(b + 1) * B].tobytes(), ("batch", b, name)
        assert L.SENTINEL == want["zz"][0].view(np.uint8).max() == want["zz"][0].view(np.uint8).min()      # picture 0 has no previous picture
    finally:
        for lane in lanes:                      # lanes first: their destruction waits for what they queued
            if lane:
                lib.svt_amd_context_destroy(lane)
        for b in pinned:
            for q in b:
                if q:
                    lib.svt_amd_host_free(root, q)
        if h_in:
            lib.svt_amd_host_free(root, h_in)
        for X in sets:
            X["arrays"].free()
            lib.svt_amd_device_free(root, X["d_stage"])
        if one:
            lib.svt_amd_context_destroy(one)
        lib.svt_amd_context_destroy(root)


# ---- 7. extremes -----------------------------------------------------------------------------------------------------------------------------

def test_extreme_pictures_in_one_batch(lib, oracle):
    rng = np.random.default_rng(4)
    w, h = 256, 128
    frames = [np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8), np.tile(np.array([[0, 255], [255, 0]], np.uint8), (h // 2, w // 2)),
              rng.integers(0, 256, (h, w), dtype=np.uint8)]
    ctx = _context(lib, w, h, 4)
    try:
        for i, f in enumerate(frames):
            upload(lib, ctx, i, f)
        got = L.run_batch(lib, ctx, L.all_jobs([0, 1, 2, 3], first_prev=3), w, h)
        for i, f in enumerate(frames):
            _assert_equals_checker(oracle, got, i, f, frames[i - 1], w, h, "extremes")
            L.assert_equals_blocking(lib, ctx, got, i, i, (i - 1) % 4, w, h, what="extremes")
        assert int(got["zz"][1]["sad"].max()) == 255 * 256 and int(got["sum_luma"][1]) == 255 * (w // 4) * (h // 4) * 16
    finally:
        lib.svt_amd_context_destroy(ctx)
