"""The temporal motion field on the device (svt-hevc_amd/csrc/tmvp_kernels.hip; include/svt_hevc_amd.h "Temporal motion field on the device"):
svt_amd_motion_field_launch against the reference's own results (tests/golden/tmvp_*.npz) on the fields its readers see and against the restatement
(tests/tmvp_numpy.py) in every byte, svt_amd_encdec_picture_motion_field on the work records a mode-decision call left in HBM, and the mode-decision call reading a
field bound with svt_amd_md_picture_set_motion_field in place: the chain q -> field -> p without a synchronisation decides as the same call with the recorded
host array."""
import ctypes as C
import os

import numpy as np
import pytest

import svtlib as S
import tmvp_numpy as N
import tmvplib as T
from pa_batch_util import BAD_PARAM, SENTINEL, DeviceBuffer, is_sentinel, make_context, ok, refused
from test_gpu_mdctl_batch import REC, Rect, _md_sig, decisions, same_call
from test_oracle_md_golden import inter_inputs
from test_tmvp_cpu import dims

pytestmark = pytest.mark.gpu
GUARD = 256                            # sentinel bytes kept behind the last record of an output array
FIELD_REC = T.TMVP_LCU_DTYPE.itemsize  # 416
CHAIN_NAMES = ("motion_416x240_m8", "noise_320x256_m9_q24", "objects_640x360_m9_q36", "xc_binary_200x136_m8_q51")
vp = C.c_void_p


@pytest.fixture(scope="module")
def lib(product):
    _md_sig(product)
    product.svt_amd_encdec_picture_set_rect.restype, product.svt_amd_encdec_picture_set_rect.argtypes = C.c_int, [vp, vp, vp]
    return T.declare(product)


@pytest.fixture(scope="module")
def ctx(lib):
    c = make_context(lib, 640, 384, 2)
    yield c
    lib.svt_amd_context_destroy(c)


def records_at_stride(heads, stride):
    """the heads as the first bytes of records `stride` bytes apart; what would be source samples is junk the producer must not read into its result"""
    raw = np.full((len(heads), stride), 0x5A, np.uint8)
    raw[:, :T.LIST_BYTES] = np.ascontiguousarray(heads).view(np.uint8).reshape(len(heads), T.LIST_BYTES)
    return raw.reshape(-1)


class Produced:
    """one launch: the records uploaded, field and statistics arrays filled with SENTINEL; get() -> (records, the bytes behind them, statistics record)"""

    def __init__(self, lib, ctx, heads, w, h, slice_type, ref_poc, stride=T.WORK_BYTES, stats=True):
        self.lib, self.ctx, self.n = lib, ctx, len(heads)
        self.keep = records_at_stride(heads, stride)
        self.works = DeviceBuffer(lib, ctx, self.keep.nbytes)
        self.works.put(self.keep)
        self.field = DeviceBuffer(lib, ctx, (self.n + 1) * FIELD_REC + GUARD)
        self.stats = DeviceBuffer(lib, ctx, GUARD)
        self.job = T.job(self.works.ptr.value, stride, w, h, slice_type, ref_poc)
        self.with_stats = stats

    def launch(self, field=None):
        return self.lib.svt_amd_motion_field_launch(self.ctx, C.byref(self.job), vp((field or self.field).at(0)), vp(self.stats.at(0)) if self.with_stats else None)

    def get(self, field=None):
        raw = (field or self.field).get()
        st = self.stats.get()
        assert is_sentinel(st[8:])
        return raw[:(self.n + 1) * FIELD_REC].view(T.TMVP_LCU_DTYPE), raw[(self.n + 1) * FIELD_REC:], st[:8].view(T.REF_STATS_DTYPE)[0]

    def free(self):
        for b in (self.works, self.field, self.stats):
            b.free()


def check_against_restatement(got, tail, stats, heads, w, h, slice_type, ref_poc, tag):
    want = N.field(heads, w, h, ref_poc)
    assert got.tobytes() == want.tobytes(), tag
    assert not got[-1].tobytes().strip(b"\0") and is_sentinel(tail), tag
    area = N.intra_area_sum(heads)
    assert (int(stats["intra_area_sum"]), int(stats["intra_coded_area"]), stats["pad"].tolist()) == (area, N.intra_coded_area(area, w, h, slice_type), [0, 0, 0]), tag


def fixture_launches(lib, ctx, name, stride):
    g = T.load_case(name)
    w, h = dims(g)
    out = []
    for k, q in enumerate(g["q_poc"]):
        st = int(g["q_slice_type"][k])
        p = Produced(lib, ctx, g["q_heads"][k], w, h, st, g["q_ref_poc"][k], stride)
        try:
            ok(lib, p.launch())
            got, tail, stats = p.get()
        finally:
            p.free()
        out.append((g, k, w, h, st, got.copy(), tail.copy(), stats.copy()))
    return out


@pytest.mark.parametrize("name", T.CASES)
def test_every_fixture_gives_the_field_the_reference_read(lib, ctx, name):
    """1. q's heads at the full SvtAmdLcuWork stride: the reference's field on the observable fields, the restatement in every byte, record `lcus` zero, the
    sentinel behind it untouched, the statistics the reference object held"""
    for g, k, w, h, st, got, tail, stats in fixture_launches(lib, ctx, name, T.WORK_BYTES):
        tag = (name, int(g["q_poc"][k]))
        assert N.mismatches(got, g["q_tmvp"][k], w, h) == 0, tag
        check_against_restatement(got, tail, stats, g["q_heads"][k], w, h, st, g["q_ref_poc"][k], tag)
        at = int(np.nonzero(g["pic_poc"] == g["q_poc"][k])[0][0])
        assert (int(stats["intra_area_sum"]), int(stats["intra_coded_area"])) == (int(g["pic_area_sum"][at]), int(g["pic_area"][at])), tag


@pytest.mark.parametrize("name", T.CASES)
def test_the_sixteen_bit_stride_gives_the_same_bytes(lib, ctx, name):
    """2. the same records at the SvtAmdLcuWork16 stride"""
    for a, b in zip(fixture_launches(lib, ctx, name, T.WORK_BYTES), fixture_launches(lib, ctx, name, T.WORK16_BYTES)):
        assert a[5].tobytes() == b[5].tobytes() and a[7].tobytes() == b[7].tobytes() and is_sentinel(b[6]), (name, a[1])


def random_heads(rng, w, h, slice_type):
    """seeded valid quadtrees: units of 8 to 64 inside the picture in Z order; intra units, all three directions, vectors at the ends of their range"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    heads = np.zeros(wl * hl, T.WORK_HEAD_DTYPE)
    for n in range(wl * hl):
        lw, lh = min(64, w - 64 * (n % wl)), min(64, h - 64 * (n // wl))
        units = []

        def rec(x, y, s):
            if x >= lw or y >= lh:
                return
            if x + s > lw or y + s > lh or (s > 8 and rng.random() < (0.35 if s == 64 else 0.5)):
                for dy, dx in ((0, 0), (0, s // 2), (s // 2, 0), (s // 2, s // 2)):
                    rec(x + dx, y + dy, s // 2)
            else:
                units.append((x, y, s))
        rec(0, 0, 64)
        hd = heads[n]
        hd["lcu_x"], hd["lcu_y"], hd["num_cus"], hd["slice_type"] = 64 * (n % wl), 64 * (n // wl), len(units), slice_type
        for i, (x, y, s) in enumerate(units):
            cu = hd["cu"][i]
            cu["x"], cu["y"], cu["size"] = x, y, s
            intra = slice_type == 2 or rng.random() < 0.25
            cu["pred_mode"] = 2 if intra else 1
            cu["inter_dir"] = 0 if intra else (0 if slice_type == 1 else rng.integers(0, 3))
            cu["mv"] = rng.choice(np.array([-32768, 32767, -1, 0, 5, -300], np.int16), (2, 2)) if rng.random() < 0.5 else rng.integers(-32768, 32768, (2, 2))
            cu["intra_luma_mode"], cu["qp"], cu["leaf_index"], cu["dz_offset"] = rng.integers(0, 35), rng.integers(0, 52), rng.integers(0, 85), rng.integers(0, 1 << 32)
        # the entries behind the list are never read into the result
        hd["cu"][len(units):] = np.frombuffer(rng.bytes(24 * (64 - len(units))), hd["cu"].dtype)
    return heads


@pytest.mark.parametrize("w,h,slice_type,seed", [(64, 64, 0, 3), (64, 64, 2, 5), (128, 64, 1, 7), (72, 72, 0, 11), (200, 136, 0, 13), (200, 136, 1, 17), (72, 72, 2, 19)])
def test_seeded_quadtrees_match_the_restatement(lib, ctx, w, h, slice_type, seed):
    """3. every byte, POCs with both 32-bit halves set; 72x72 has partial LCUs whose map units are half covered"""
    rng = np.random.default_rng(seed)
    heads = random_heads(rng, w, h, slice_type)
    poc = (0x0123456789ABCDEF, 0xFEDCBA9876543210)
    sizes = np.concatenate([hd["cu"]["size"][:int(hd["num_cus"])] for hd in heads])
    assert set(sizes.tolist()) <= {8, 16, 32, 64}
    if (w, h) == (200, 136):
        assert set(sizes.tolist()) == {8, 16, 32, 64}
    p = Produced(lib, ctx, heads, w, h, slice_type, poc)
    try:
        ok(lib, p.launch())
        got, tail, stats = p.get()
        check_against_restatement(got, tail, stats, heads, w, h, slice_type, poc, (w, h, seed))
        if slice_type != 2:
            assert got["available"].any() and (got["ref_poc"] >> 32).any() and (got["ref_poc"] & 0xFFFFFFFF).any()
    finally:
        p.free()


def test_launches_back_to_back_and_repeated(lib, ctx):
    """4. two launches into two arrays without a synchronisation in between, and one repeated into the same array: byte-identical to the single launch"""
    g = T.load_case("b_objects_416x240_m8")
    w, h = dims(g)
    a = Produced(lib, ctx, g["q_heads"][1], w, h, int(g["q_slice_type"][1]), g["q_ref_poc"][1])
    b = Produced(lib, ctx, g["q_heads"][2], w, h, int(g["q_slice_type"][2]), g["q_ref_poc"][2])
    second = DeviceBuffer(lib, ctx, a.field.n)
    try:
        ok(lib, a.launch())
        ok(lib, b.launch())
        ok(lib, a.launch(second))
        ok(lib, a.launch(second))
        fa, ta, sa = a.get()
        fb, tb, sb = b.get()
        f2, t2, _ = a.get(second)
        for f, t, s, k in ((fa, ta, sa, 1), (fb, tb, sb, 2)):
            check_against_restatement(f, t, s, g["q_heads"][k], w, h, int(g["q_slice_type"][k]), g["q_ref_poc"][k], k)
        assert fa.tobytes() == f2.tobytes() and is_sentinel(t2) and fa.tobytes() != fb.tobytes()
    finally:
        second.free()
        a.free()
        b.free()


# ---- the mode-decision call and the field ------------------------------------------------------------------------------------------------------------

class Pic:
    """a picture object on `ctx` holding picture k of a P / B mode-decision fixture; call(...) -> rc and the three result arrays as bytes, each filled with
    SENTINEL before the call"""

    def __init__(self, lib, ctx, g, k):
        import torch
        self.lib, self.ctx, self.g, self.k = lib, ctx, g, k
        self.w, self.h = int(g["pic"][k]["width"]), int(g["pic"][k]["height"])
        self.pic = vp()
        ok(lib, lib.svt_amd_encdec_picture_create(ctx, self.w, self.h, 1, C.byref(self.pic)))
        self.P = np.ascontiguousarray(g["pic"][k:k + 1])
        self.cost, self.ois = np.ascontiguousarray(g["cost"][k]), np.ascontiguousarray(g["ois"][k])
        self.src = [np.ascontiguousarray(g[n][k]) for n in ("src_y", "src_cb", "src_cr")]
        self.lcus = np.ascontiguousarray(g["lcu"][k])
        self.n = len(self.lcus)
        self.X, self.me, self.tmvp, refs, planes = inter_inputs(g, k)
        self.ref_dev = [[torch.from_numpy(a).cuda() for a in pl] for pl in planes]
        torch.cuda.synchronize()
        rs = [S.RefPicture(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), r.strideY, r.strideC, r.originX, r.originY, r.width, r.height)
              for d, r in zip(self.ref_dev, refs)]
        ok(lib, lib.svt_amd_encdec_picture_set_inter(ctx, self.pic, C.byref(rs[0]), C.byref(rs[1]), self.cost.ctypes.data))

    def call(self, tmvp=None, X=None, lcus="host", records=True):
        n = self.n
        out = np.full(n * S.MD_LCU_OUT_DTYPE.itemsize, SENTINEL, np.uint8)
        works = np.full(n * S.LCU_WORK_DTYPE.itemsize, SENTINEL, np.uint8)
        res = np.full(n * S.LCU_RESULT_DTYPE.itemsize, SENTINEL, np.uint8)
        s, X = self.src, self.X if X is None else X
        rc = self.lib.svt_amd_md_encode_picture_inter(self.ctx, self.pic, self.P.ctypes.data, X.ctypes.data, self.lcus.ctypes.data if lcus == "host" else None,
                                                      s[0].ctypes.data, s[0].shape[1], s[1].ctypes.data, s[2].ctypes.data, s[1].shape[1], self.ois.ctypes.data, 0,
                                                      self.me.ctypes.data, 0, tmvp.ctypes.data if tmvp is not None else None, out.ctypes.data,
                                                      works.ctypes.data if records else None, res.ctypes.data if records else None)
        return rc, (out.tobytes(), works.tobytes(), res.tobytes())

    def free(self):
        self.lib.svt_amd_encdec_picture_destroy(self.ctx, self.pic)


def load_pair(name):
    return tuple(np.load(os.path.join(S.GOLDEN_DIR, "md_%s_%s.npz" % (kind, name))) for kind in ("bref", "b"))


def pair_is_live(gp, kp):
    """by the fixture alone: the reader has the temporal candidate switched on and its recorded field has available units"""
    return bool(gp["inter"][kp]["tmvp_enable"]) and bool(gp["tmvp_present"][kp]) and bool(gp["tmvp"][kp]["available"].any())


def differ(a, b):
    """two calls' results differ somewhere the call defines: decisions, work records or results"""
    return decisions(a[0]) != decisions(b[0]) or a[1] != b[1] or a[2] != b[2]


def test_the_chain_from_q_to_p_on_one_lane(lib):
    """5. q decided on the device, its field produced from the work records in HBM, bound, and p decided from it with tmvp == NULL - nothing synchronises between
    the producer and p's call: works and results raw-equal to the call with the recorded host array, md_out in every byte the call defines.
    The bound array is the only place the right field can come from: p's picture object has uploaded a ZERO field in a host call just before (what a call that
    ignored the binding would read again), and the comparison call with the recorded host array runs on the same object AFTER the bound call (the same object,
    because the kernel never writes the pad of SvtAmdMdLcuOut: it holds what the object's allocation held, and decisions() compares it).  At least one pair runs with
    tmvp_enable and a field that has available units, and in at least one such pair the zero field decides differently from the recorded one (the parent's
    host path says so): there a call that ignored the binding could not pass"""
    live, field_matters = [], []
    for name in CHAIN_NAMES:
        gq, gp = load_pair(name)
        w, h = int(gq["pic"][0]["width"]), int(gq["pic"][0]["height"])
        ctx = make_context(lib, w, (h + 7) & ~7, 2)
        n = S.lcu_count(w, h)
        field, stats = DeviceBuffer(lib, ctx, (n + 1) * FIELD_REC + GUARD), DeviceBuffer(lib, ctx, GUARD)
        nothing = np.zeros(n, T.TMVP_LCU_DTYPE)
        try:
            for q, p in dict(T.MD_PAIRS)[name]:
                tag = (name, q, p)
                kq, kp = gq["picture_number"].tolist().index(q), gp["picture_number"].tolist().index(p)
                Q, Pp = Pic(lib, ctx, gq, kq), Pic(lib, ctx, gp, kp)
                try:
                    assert int(Pp.X["colocated_poc"][0]) == q and Pp.tmvp is not None, tag
                    rc, blind = Pp.call(tmvp=nothing)          # the last field p's own object uploaded: no temporal candidate anywhere
                    assert rc == 0, lib.svt_amd_last_error()
                    rc, qout = Q.call(tmvp=Q.tmvp)
                    assert rc == 0, lib.svt_amd_last_error()
                    field.fill()
                    poc = np.ascontiguousarray(Q.X["ref_poc"][0], np.uint64)
                    ok(lib, lib.svt_amd_encdec_picture_motion_field(ctx, Q.pic, int(Q.P["slice_type"][0]), poc.ctypes.data, field.ptr, stats.ptr))
                    ok(lib, lib.svt_amd_md_picture_set_motion_field(ctx, Pp.pic, field.ptr))
                    rc, bound = Pp.call(tmvp=None)
                    assert rc == 0, lib.svt_amd_last_error()
                    rc, host = Pp.call(tmvp=Pp.tmvp)           # only now does the object upload the recorded field itself
                    assert rc == 0, lib.svt_amd_last_error()
                    same_call(host, bound, tag)
                    raw = field.get()
                    got = raw[:(n + 1) * FIELD_REC].view(T.TMVP_LCU_DTYPE)
                    assert N.mismatches(got, Pp.tmvp, w, h) == 0, tag
                    heads = np.frombuffer(qout[1], S.LCU_WORK_DTYPE)
                    st = stats.get()[:8].view(T.REF_STATS_DTYPE)[0]
                    check_against_restatement(got, raw[(n + 1) * FIELD_REC:], st, heads, w, h, int(Q.P["slice_type"][0]), poc, tag)
                    if pair_is_live(gp, kp):
                        assert got["available"].any(), tag
                        live.append(tag)
                        if differ(host, blind):
                            field_matters.append(tag)
                finally:
                    for o in (Q, Pp):
                        o.free()
        finally:
            field.free()
            stats.free()
            lib.svt_amd_context_destroy(ctx)
    assert live and field_matters, (live, field_matters)


def test_binding_rules(lib):
    """6. each call consumes the binding; a host array plus a binding is refused and drops it; tmvp_enable == 0 drops it unread; it combines with a bound controls
    array; a second call without a new binding is refused as before.  No successful call after the first two passes a host field, so the object's own copy stays
    the zero field throughout"""
    name, (q, p) = "motion_416x240_m8", dict(T.MD_PAIRS)["motion_416x240_m8"][0]
    gp = load_pair(name)[1]
    kp = gp["picture_number"].tolist().index(p)
    assert pair_is_live(gp, kp)
    w, h = int(gp["pic"][kp]["width"]), int(gp["pic"][kp]["height"])
    ctx = make_context(lib, w, (h + 7) & ~7, 2)
    Pp = Pic(lib, ctx, gp, kp)
    n = Pp.n
    field, junk, ctl = DeviceBuffer(lib, ctx, (n + 1) * FIELD_REC), DeviceBuffer(lib, ctx, (n + 1) * FIELD_REC), DeviceBuffer(lib, ctx, n * REC + 64)
    try:
        recorded = np.zeros(n + 1, T.TMVP_LCU_DTYPE)
        recorded[:n] = Pp.tmvp
        field.put(recorded)
        ctl.put(Pp.lcus)

        def bind(buf=field):
            ok(lib, lib.svt_amd_md_picture_set_motion_field(ctx, Pp.pic, buf.ptr))

        def refused_call(tag, text, **kw):
            rc, got = Pp.call(**kw)
            assert rc == BAD_PARAM and all(is_sentinel(np.frombuffer(a, np.uint8)) for a in got), (tag, rc)
            err = lib.svt_amd_last_error()
            assert err.startswith(b"svt_amd_md_encode_picture") and text in err, (tag, err)

        rc, want = Pp.call(tmvp=Pp.tmvp)
        assert rc == 0, lib.svt_amd_last_error()
        # from here on the object's OWN copy holds a zero field, which decides differently: a call that ignored a binding would give `blind`, not `want`
        rc, blind = Pp.call(tmvp=np.zeros(n, T.TMVP_LCU_DTYPE))
        assert rc == 0, lib.svt_amd_last_error()
        assert differ(want, blind), "the recorded field does not matter to this picture: the checks below would prove nothing"
        refused_call("NULL without a binding", b"no co-located motion field")
        bind()
        rc, got = Pp.call()
        assert rc == 0, lib.svt_amd_last_error()
        same_call(want, got, "bound")
        refused_call("the call consumed the binding", b"no co-located motion field")
        bind()
        refused_call("a host array and a binding", b"svt_amd_md_picture_set_motion_field", tmvp=Pp.tmvp)
        refused_call("... which dropped the binding", b"no co-located motion field")
        bind()
        ok(lib, lib.svt_amd_md_picture_set_motion_field(ctx, Pp.pic, None))
        refused_call("NULL drops a binding", b"no co-located motion field")
        bind()
        refused_call("a refused call consumes the binding too", b"", lcus=None)
        refused_call("... so the next has none", b"no co-located motion field")
        bind()
        assert lib.svt_amd_md_encode_picture(ctx, Pp.pic, Pp.P.ctypes.data, Pp.lcus.ctypes.data, Pp.src[0].ctypes.data, w, Pp.src[1].ctypes.data, Pp.src[2].ctypes.data,
                                             w // 2, Pp.ois.ctypes.data, 0, None, None, None, None) == BAD_PARAM
        refused_call("an I-picture call drops it unread", b"no co-located motion field")
        # tmvp_enable == 0: a bound array (of sentinel bytes) is dropped unread
        off = Pp.X.copy()
        off["tmvp_enable"] = 0
        rc, want_off = Pp.call(X=off)
        assert rc == 0, lib.svt_amd_last_error()
        bind(junk)
        rc, got = Pp.call(X=off)
        assert rc == 0, lib.svt_amd_last_error()
        same_call(want_off, got, "tmvp_enable == 0")
        refused_call("... and dropped", b"no co-located motion field")
        # both bindings in one call
        bind()
        ok(lib, lib.svt_amd_md_picture_set_controls(ctx, Pp.pic, ctl.ptr))
        rc, got = Pp.call(lcus=None)
        assert rc == 0, lib.svt_amd_last_error()
        same_call(want, got, "controls and field bound")
        refused(lib, lib.svt_amd_md_picture_set_motion_field(ctx, Pp.pic, vp(field.at(4))), T.BIND_ENTRY)
    finally:
        Pp.free()
        for b in (field, junk, ctl):
            b.free()
        lib.svt_amd_context_destroy(ctx)


def test_refusals_name_the_entry_and_write_nothing(lib, ctx):
    """7. on the device: every refused launch leaves field and statistics as they were"""
    g = T.load_case("b_xc_binary_200x136_m8_q51")
    w, h = dims(g)
    p = Produced(lib, ctx, g["q_heads"][2], w, h, int(g["q_slice_type"][2]), g["q_ref_poc"][2])
    try:
        good = p.job

        def variant(**kw):
            j = T.job(good.d_works, good.work_stride, good.width, good.height, good.slice_type, (good.ref_poc[0], good.ref_poc[1]))
            for f, v in kw.items():
                setattr(j, f, v)
            return j

        f, s = vp(p.field.at(0)), vp(p.stats.at(0))
        refused(lib, lib.svt_amd_motion_field_launch(None, C.byref(good), f, s), T.ENTRY)
        refused(lib, lib.svt_amd_motion_field_launch(ctx, None, f, s), T.ENTRY)
        refused(lib, lib.svt_amd_motion_field_launch(ctx, C.byref(good), None, s), T.ENTRY)
        for tag, j in (("no records", variant(d_works=None)), ("a stride below the head", variant(work_stride=40)), ("a stride below the unit list", variant(work_stride=T.LIST_BYTES - 4)),
                       ("zero width", variant(width=0)), ("zero height", variant(height=0)), ("oversize", variant(width=8256, height=8192)), ("slice type 3", variant(slice_type=3))):
            refused(lib, lib.svt_amd_motion_field_launch(ctx, C.byref(j), f, s), T.ENTRY, tag)
        refused(lib, lib.svt_amd_motion_field_launch(ctx, C.byref(good), vp(p.field.at(4)), s), T.ENTRY, "a misaligned field")
        # a fresh picture object, one whose last call made no work records, and one with a rectangle
        gp = load_pair("xc_binary_200x136_m8_q51")[1]
        pic = Pic(lib, ctx, gp, 0)
        try:
            assert (pic.w, pic.h) == (w, h)
            poc = np.ascontiguousarray(pic.X["ref_poc"][0], np.uint64)
            refused(lib, lib.svt_amd_encdec_picture_motion_field(ctx, pic.pic, 0, poc.ctypes.data, f, s), T.PICTURE_ENTRY, "fresh")
            rc, _ = pic.call(tmvp=pic.tmvp, records=False)
            assert rc == 0, lib.svt_amd_last_error()
            refused(lib, lib.svt_amd_encdec_picture_motion_field(ctx, pic.pic, 0, poc.ctypes.data, f, s), T.PICTURE_ENTRY, "decisions only")
            rc, _ = pic.call(tmvp=pic.tmvp)
            assert rc == 0, lib.svt_amd_last_error()
            rect = Rect(0, 0, 128, 64)
            ok(lib, lib.svt_amd_encdec_picture_set_rect(ctx, pic.pic, C.byref(rect)))
            refused(lib, lib.svt_amd_encdec_picture_motion_field(ctx, pic.pic, 0, poc.ctypes.data, f, s), T.PICTURE_ENTRY, "rectangle")
            assert b"rectangle" in lib.svt_amd_last_error()
            ok(lib, lib.svt_amd_encdec_picture_set_rect(ctx, pic.pic, None))
            refused(lib, lib.svt_amd_encdec_picture_motion_field(ctx, pic.pic, 3, poc.ctypes.data, f, s), T.PICTURE_ENTRY, "slice type")
            refused(lib, lib.svt_amd_encdec_picture_motion_field(ctx, pic.pic, 0, poc.ctypes.data, None, s), T.PICTURE_ENTRY, "no field")
        finally:
            pic.free()
        ok(lib, lib.svt_amd_synchronize(ctx))
        assert is_sentinel(p.field.get()) and is_sentinel(p.stats.get())
        ok(lib, p.launch())                     # ... and the same arrays take the result afterwards
        got, tail, stats = p.get()
        check_against_restatement(got, tail, stats, g["q_heads"][2], w, h, int(g["q_slice_type"][2]), g["q_ref_poc"][2], "after the refusals")
    finally:
        p.free()
