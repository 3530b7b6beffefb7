"""-m gpu: a context takes its stream at its first stream-ordered use (a root that only allocates, pins, copies blocking and forks
never takes one), a lane may start with a wait on another lane's event, and the batch form of the record pack (one launch for the
whole batch, picture = blockIdx.y) writes what the per-picture compact fetches and the full records say.  Nothing here asserts a
time or an overlap: whether lanes run side by side is shown by the timelines under profiles/."""
import ctypes as C

import numpy as np
import pytest

import svtlib as S
from gpu_util import default_params, me_picture, upload

pytestmark = pytest.mark.gpu

W, H = 1920, 1080                  # 30 x 17 LCUs, the last row 56 lines high
NL = S.lcu_count(W, H)
ME_FULL_B, ME_B = S.ME_LCU_DTYPE.itemsize, S.ME_PU_COUNT * 24
OIS_FULL_B, OIS_CAND_B = S.OIS_LCU_DTYPE.itemsize, S.ME_PU_COUNT * S.OIS_MAX_CAND * 4
vp = C.c_void_p


def ois_b(nc):
    return S.ME_PU_COUNT * nc * 4 + 88


def _bytes(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n,))


def _ok(lib, rc):
    assert rc == 0, lib.svt_amd_last_error()


def _compact_me(full):
    """full ME records of one picture (ME_LCU_DTYPE array) -> the wire bytes: pu[85] of every LCU"""
    return full.view(np.uint8).reshape(len(full), ME_FULL_B)[:, :ME_B].reshape(-1)


def _compact_ois(full, nc):
    """full OIS records of one picture -> the wire bytes: nc candidates of every CU, then the 88 bytes behind the candidates"""
    raw = full.view(np.uint8).reshape(len(full), OIS_FULL_B)
    cand = raw[:, :OIS_CAND_B].reshape(len(full), S.ME_PU_COUNT, S.OIS_MAX_CAND, 4)[:, :, :nc].reshape(len(full), -1)
    return np.concatenate([cand, raw[:, OIS_CAND_B:]], axis=1).reshape(-1)


def _ois_params():
    op = S.OisParams()
    op.luma_width, op.luma_height, op.ois_th_set, op.temporal_layer_index = W, H, 1, 1
    return op


def _frames(n, seed):
    """n distinct 1080p frames: a few frames of the moving clip, the rest shifted copies of them"""
    base = [S.gen_luma("motion", W, H, t, seed) for t in range(4)]
    return [np.ascontiguousarray(np.roll(base[i % 4], (3 * (i // 4), 5 * (i // 4)), (0, 1))) for i in range(n)]


def test_root_without_stream_three_lane_pipeline_every_batch(product):
    """bench.py's step() sequence (copy-in lane -> compute lane -> copy-out lane, two buffer sets, lane events as there) under a root
    that only allocates, pins, copies blocking and forks: every batch of three steps - not only the last - arrives in pinned host
    memory as the one-lane blocking calls compute it."""
    lib = product
    B, NSETS, STEPS = 4, 2, 3
    nb = NSETS * STEPS
    p = default_params(W, H, num_lists=2, temporal_layer_index=1)
    op = _ois_params()
    nc = lib.svt_amd_ois_compact_candidates(C.byref(op))
    me_pic, ois_pic = NL * ME_B, NL * ois_b(nc)
    frames = _frames(8, 21)
    batch_frames = [[frames[(3 * b + i) % 8] for i in range(B)] for b in range(nb)]   # every batch holds other pictures
    root, ref = vp(), vp()
    _ok(lib, lib.svt_amd_context_create(0, W, 1088, NSETS * B, C.byref(root)))
    lanes = [vp(), vp(), vp()]
    try:
        for lane in lanes:
            _ok(lib, lib.svt_amd_context_fork(root, C.byref(lane)))
        lane_in, lane_k, lane_out = lanes
        h_in, d_probe = vp(), vp()
        _ok(lib, lib.svt_amd_host_alloc(root, nb * B * W * H, C.byref(h_in)))
        _bytes(h_in, nb * B * W * H)[:] = np.concatenate([f.reshape(-1) for bf in batch_frames for f in bf])
        # the root's blocking copies work without a stream
        _ok(lib, lib.svt_amd_device_alloc(root, W * H, C.byref(d_probe)))
        _ok(lib, lib.svt_amd_device_upload(root, d_probe, h_in, W * H))
        back = np.zeros(W * H, np.uint8)
        _ok(lib, lib.svt_amd_device_download(root, back.ctypes.data, d_probe, W * H))
        assert np.array_equal(back, batch_frames[0][0].reshape(-1))
        _ok(lib, lib.svt_amd_device_free(root, d_probe))
        sets = []
        for k in range(NSETS):
            d_stage, d_me, d_ois = vp(), vp(), vp()
            _ok(lib, lib.svt_amd_device_alloc(lane_in, B * W * H, C.byref(d_stage)))
            _ok(lib, lib.svt_amd_device_alloc(lane_k, B * me_pic, C.byref(d_me)))
            _ok(lib, lib.svt_amd_device_alloc(lane_k, B * ois_pic, C.byref(d_ois)))
            slots = (C.c_int * B)(*[k * B + i for i in range(B)])
            ptrs = (vp * B)(*[d_stage.value + i * W * H for i in range(B)])
            jobs, ojobs = (S.MeJob * B)(), (S.OisJob * B)()
            for i in range(B):
                jobs[i].params, jobs[i].cur_slot = p, slots[i]
                jobs[i].ref_slot[0], jobs[i].ref_slot[1] = slots[(i - 1) % B], slots[(i + 1) % B]
                ojobs[i].params, ojobs[i].cur_slot = op, slots[i]
            sets.append(dict(d_stage=d_stage, d_me=d_me, d_ois=d_ois, slots=slots, ptrs=ptrs, jobs=jobs, ojobs=ojobs))
        # pinned results of EVERY batch (bench.py keeps one pair per set and overwrites it)
        h_me, h_ois = [vp() for _ in range(nb)], [vp() for _ in range(nb)]
        for b in range(nb):
            _ok(lib, lib.svt_amd_host_alloc(lane_out, B * me_pic, C.byref(h_me[b])))
            _ok(lib, lib.svt_amd_host_alloc(lane_out, B * ois_pic, C.byref(h_ois[b])))
        EV_STAGE, EV_READY = 0, NSETS
        for s in range(STEPS):
            for k, L in enumerate(sets):
                b = s * NSETS + k
                _ok(lib, lib.svt_amd_lane_event_wait(lane_in, lane_k, EV_STAGE + k))
                _ok(lib, lib.svt_amd_device_upload_async(lane_in, L["d_stage"], vp(h_in.value + b * B * W * H), B * W * H))
                _ok(lib, lib.svt_amd_lane_event_record(lane_in, EV_STAGE + k))
                _ok(lib, lib.svt_amd_lane_event_wait(lane_k, lane_in, EV_STAGE + k))
                _ok(lib, lib.svt_amd_lane_event_wait(lane_k, lane_out, EV_STAGE + k))
                _ok(lib, lib.svt_amd_picture_upload_device_batch(lane_k, B, L["slots"], L["ptrs"], W, W, H))
                _ok(lib, lib.svt_amd_lane_event_record(lane_k, EV_STAGE + k))
                _ok(lib, lib.svt_amd_me_batch_launch(lane_k, L["jobs"], B))
                _ok(lib, lib.svt_amd_ois_batch_launch(lane_k, L["ojobs"], B))
                _ok(lib, lib.svt_amd_records_pack_batch_async(lane_k, L["slots"], B, nc, L["d_me"], L["d_ois"]))
                _ok(lib, lib.svt_amd_lane_event_record(lane_k, EV_READY + k))
                _ok(lib, lib.svt_amd_lane_event_wait(lane_out, lane_k, EV_READY + k))
                _ok(lib, lib.svt_amd_device_download_async(lane_out, h_me[b], L["d_me"], B * me_pic))
                _ok(lib, lib.svt_amd_device_download_async(lane_out, h_ois[b], L["d_ois"], B * ois_pic))
                _ok(lib, lib.svt_amd_lane_event_record(lane_out, EV_STAGE + k))
        for lane in lanes:
            _ok(lib, lib.svt_amd_synchronize(lane))
        _ok(lib, lib.svt_amd_synchronize(root))
        # one-lane reference: blocking per-picture calls on a context of its own, packed on the host
        _ok(lib, lib.svt_amd_context_create(0, W, 1088, B, C.byref(ref)))
        for b in range(nb):
            for i in range(B):
                upload(lib, ref, i, batch_frames[b][i])
            got_me = _bytes(h_me[b], B * me_pic).reshape(B, me_pic)
            got_ois = _bytes(h_ois[b], B * ois_pic).reshape(B, ois_pic)
            for i in range(B):
                full = me_picture(lib, ref, p, i, [(i - 1) % B, (i + 1) % B])
                assert np.array_equal(got_me[i], _compact_me(full)), ("ME", b, i)
                ois = np.zeros(NL, S.OIS_LCU_DTYPE)
                _ok(lib, lib.svt_amd_ois_picture(ref, C.byref(op), i, None, ois.ctypes.data))
                assert np.array_equal(got_ois[i], _compact_ois(ois, nc)), ("OIS", b, i)
        for q in h_me + h_ois:
            lib.svt_amd_host_free(lane_out, q)
        lib.svt_amd_host_free(root, h_in)
        for k, L in enumerate(sets):
            lib.svt_amd_device_free(lane_in, L["d_stage"])
            lib.svt_amd_device_free(lane_k, L["d_me"])
            lib.svt_amd_device_free(lane_k, L["d_ois"])
    finally:
        for lane in lanes:
            if lane:
                lib.svt_amd_context_destroy(lane)
        if ref:
            lib.svt_amd_context_destroy(ref)
        lib.svt_amd_context_destroy(root)


def test_lane_starting_with_event_wait_then_download(product):
    """a lane whose first operation is a wait on another lane's recorded event, then a download: the bytes are the producer's"""
    lib = product
    n = 256 << 20
    root, prod, cons = vp(), vp(), vp()
    _ok(lib, lib.svt_amd_context_create(0, 640, 384, 1, C.byref(root)))
    try:
        _ok(lib, lib.svt_amd_context_fork(root, C.byref(prod)))
        _ok(lib, lib.svt_amd_context_fork(root, C.byref(cons)))
        h_src, h_dst, d = vp(), vp(), vp()
        _ok(lib, lib.svt_amd_host_alloc(root, n, C.byref(h_src)))
        _ok(lib, lib.svt_amd_host_alloc(root, n, C.byref(h_dst)))
        _ok(lib, lib.svt_amd_device_alloc(root, n, C.byref(d)))
        src, dst = _bytes(h_src, n), _bytes(h_dst, n)
        dst[:] = 0
        src[:] = 0
        _ok(lib, lib.svt_amd_device_upload(root, d, h_src, n))                  # the device buffer starts as zeros
        src[:] = np.random.default_rng(5).integers(1, 256, size=n, dtype=np.uint8)
        _ok(lib, lib.svt_amd_device_upload_async(prod, d, h_src, n))            # milliseconds of copy in flight
        _ok(lib, lib.svt_amd_lane_event_record(prod, 3))
        _ok(lib, lib.svt_amd_lane_event_wait(cons, prod, 3))                    # the consumer's first operation
        _ok(lib, lib.svt_amd_device_download_async(cons, h_dst, d, n))
        _ok(lib, lib.svt_amd_synchronize(cons))
        assert np.array_equal(dst, src)
        _ok(lib, lib.svt_amd_synchronize(prod))
        lib.svt_amd_device_free(root, d)
        lib.svt_amd_host_free(root, h_src)
        lib.svt_amd_host_free(root, h_dst)
    finally:
        for c in (cons, prod, root):
            if c:
                lib.svt_amd_context_destroy(c)


def test_context_without_stream_synchronize_timer_destroy(product):
    """synchronize and destroy of a context (root and lane) that never had stream-ordered work return without error; the timer is a
    stream-ordered use and works on such a context"""
    lib = product
    root, lane, idle = vp(), vp(), vp()
    _ok(lib, lib.svt_amd_context_create(0, 640, 384, 1, C.byref(root)))
    _ok(lib, lib.svt_amd_context_fork(root, C.byref(lane)))
    _ok(lib, lib.svt_amd_context_fork(root, C.byref(idle)))
    _ok(lib, lib.svt_amd_synchronize(root))
    _ok(lib, lib.svt_amd_synchronize(lane))
    _ok(lib, lib.svt_amd_synchronize(idle))
    lib.svt_amd_context_destroy(idle)          # never used
    ms = C.c_float(-1.0)
    for c in (lane, root):
        _ok(lib, lib.svt_amd_timer_begin(c))
        _ok(lib, lib.svt_amd_timer_end(c, C.byref(ms)))
        assert ms.value >= 0.0
        _ok(lib, lib.svt_amd_synchronize(c))
    lib.svt_amd_context_destroy(lane)
    lib.svt_amd_context_destroy(root)
    # ... and one that is destroyed right after its creation
    _ok(lib, lib.svt_amd_context_create(0, 640, 384, 1, C.byref(root)))
    lib.svt_amd_context_destroy(root)


@pytest.fixture(scope="module")
def filled_slots(product):
    """64 slots at 1080p, each holding the ME and OIS records of a different picture, and those records in full on the host"""
    lib = product
    n = 64
    ctx = vp()
    _ok(lib, lib.svt_amd_context_create(0, W, 1088, n, C.byref(ctx)))
    frames = _frames(n, 33)
    for s, f in enumerate(frames):
        upload(lib, ctx, s, f)
    p = default_params(W, H, num_lists=2, temporal_layer_index=1)
    op = _ois_params()
    op.ois_kernel_level = 1                     # the widest form: 18 candidates per CU are written
    jobs, ojobs = (S.MeJob * n)(), (S.OisJob * n)()
    for i in range(n):
        jobs[i].params, jobs[i].cur_slot = p, i
        jobs[i].ref_slot[0], jobs[i].ref_slot[1] = (i - 1) % n, (i + 1) % n
        ojobs[i].params, ojobs[i].cur_slot = op, i
    _ok(lib, lib.svt_amd_me_batch_launch(ctx, jobs, n))
    _ok(lib, lib.svt_amd_ois_batch_launch(ctx, ojobs, n))
    _ok(lib, lib.svt_amd_synchronize(ctx))
    me_full, ois_full = [], []
    for s in range(n):
        me = np.zeros(NL, S.ME_LCU_DTYPE)
        ois = np.zeros(NL, S.OIS_LCU_DTYPE)
        _ok(lib, lib.svt_amd_me_picture_fetch(ctx, s, me.ctypes.data))
        _ok(lib, lib.svt_amd_ois_picture_fetch(ctx, s, ois.ctypes.data))
        me_full.append(me)
        ois_full.append(ois)
    assert not np.array_equal(me_full[0]["pu"], me_full[1]["pu"]) and not np.array_equal(ois_full[0]["candidate"], ois_full[1]["candidate"])
    yield ctx, me_full, ois_full
    lib.svt_amd_context_destroy(ctx)


@pytest.mark.parametrize("n", [1, 3, 64])
def test_records_pack_batch_equals_per_picture_compact_fetch(product, filled_slots, n):
    """one pack launch for n pictures in mixed slot order, for every candidate count, with either destination absent: byte for byte
    the per-picture compact fetches of the same slots, which in turn are the corresponding parts of the full records"""
    lib = product
    ctx, me_full, ois_full = filled_slots
    order = [int(s) for s in np.random.default_rng(100 + n).permutation(64)[:n]]
    slots = (C.c_int * n)(*order)
    d_me, d_ois = vp(), vp()
    _ok(lib, lib.svt_amd_device_alloc(ctx, n * NL * ME_B, C.byref(d_me)))
    _ok(lib, lib.svt_amd_device_alloc(ctx, n * NL * ois_b(S.OIS_MAX_CAND), C.byref(d_ois)))
    try:
        # per-picture compact fetches (a batch of one each): the reference the batch form must equal
        one_me = np.zeros((n, NL * ME_B), np.uint8)
        for i, s in enumerate(order):
            _ok(lib, lib.svt_amd_me_picture_fetch_compact_async(ctx, s, one_me[i].ctypes.data))
        _ok(lib, lib.svt_amd_synchronize(ctx))
        for i, s in enumerate(order):
            assert np.array_equal(one_me[i], _compact_me(me_full[s])), ("per-picture ME fetch", s)
        for nc in range(1, S.OIS_MAX_CAND + 1):
            mode = ("both", "me only", "ois only")[nc % 3] if nc > 1 else "both"
            ob = NL * ois_b(nc)
            one_ois = np.zeros((n, ob), np.uint8)
            for i, s in enumerate(order):
                _ok(lib, lib.svt_amd_ois_picture_fetch_compact_async(ctx, s, nc, one_ois[i].ctypes.data))
            _ok(lib, lib.svt_amd_synchronize(ctx))
            for i, s in enumerate(order):
                assert np.array_equal(one_ois[i], _compact_ois(ois_full[s], nc)), ("per-picture OIS fetch", s, nc)
            # poison the destinations, so that a NULL destination or a picture left out shows
            poison = np.full(max(n * NL * ME_B, n * ob), 0xA5, np.uint8)
            _ok(lib, lib.svt_amd_device_upload(ctx, d_me, poison.ctypes.data, n * NL * ME_B))
            _ok(lib, lib.svt_amd_device_upload(ctx, d_ois, poison.ctypes.data, n * ob))
            _ok(lib, lib.svt_amd_records_pack_batch_async(ctx, slots, n, nc, d_me if mode != "ois only" else None, d_ois if mode != "me only" else None))
            got_me, got_ois = np.zeros((n, NL * ME_B), np.uint8), np.zeros((n, ob), np.uint8)
            _ok(lib, lib.svt_amd_device_download(ctx, got_me.ctypes.data, d_me, got_me.size))
            _ok(lib, lib.svt_amd_device_download(ctx, got_ois.ctypes.data, d_ois, got_ois.size))
            if mode == "ois only":
                assert (got_me == 0xA5).all(), (nc, mode)
            else:
                assert np.array_equal(got_me, one_me), (nc, mode)
            if mode == "me only":
                assert (got_ois == 0xA5).all(), (nc, mode)
            else:
                assert np.array_equal(got_ois, one_ois), (nc, mode)
    finally:
        lib.svt_amd_device_free(ctx, d_me)
        lib.svt_amd_device_free(ctx, d_ois)
