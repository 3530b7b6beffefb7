"""GPU: the picture tail on the device (svt-hevc_amd/csrc/tail_kernels.hip; include/svt_hevc_amd.h "Picture tail on the device") - the filter inputs derived from
the records in HBM against the restatement (tests/tail_numpy.py), svt_amd_encdec_picture_tail_launch against the reference encoder's own output (the 14
tests/golden/encodepass_dlf_* / encodepass_sao_* fixtures) and, byte for byte, against the blocking entries svt_amd_encdec_picture_deblock / _sao / _sao_decide /
_reference on the same inputs; whole sequences that never leave the device; the object form; the 16-bit twins of the device-array encode entries; refusals and
malformed records."""
import ctypes as C
import os

import numpy as np
import pytest

import svtlib as S
import tail_numpy as N
import taillib as T
from pa_batch_util import SENTINEL, DeviceBuffer, is_sentinel, make_context, ok, refused
from test_gpu_encodepass import DeblockParams, device_refs, encoded_picture, set_inter, sig_picture, written_picture
from test_gpu_tmvp import random_heads
from test_oracle_encodepass_golden import DLF_CASES, INTER_CASES, SAO_CASES, allows_mismatch, compare_lcu, is16, load_case, sao_inputs_of_picture
from test_oracle_saodec_golden import LCU, params_of, same_decision

pytestmark = pytest.mark.gpu
GUARD = 256
vp = C.c_void_p
D, SD, A, R = N.DEBLOCK, N.SAO_DECIDE, N.SAO_APPLY, N.REFERENCE
FULL = D | SD | A | R
NONE_POC = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def lib(product):
    sig_picture(product)
    product.svt_amd_encdec_picture_set_inter.restype, product.svt_amd_encdec_picture_set_inter.argtypes = C.c_int, [vp] * 5
    product.svt_amd_encdec_picture_reference.restype = C.c_int
    product.svt_amd_encdec_picture_reference.argtypes = [vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    for f in (product.svt_amd_encdec_picture_deblock, product.svt_amd_encdec_picture_deblock16):
        f.restype, f.argtypes = C.c_int, [vp, vp, vp, vp, C.POINTER(DeblockParams), vp, vp, vp]
    for f in (product.svt_amd_encdec_picture_sao, product.svt_amd_encdec_picture_sao16):
        f.restype, f.argtypes = C.c_int, [vp] * 9
    product.svt_amd_encdec_picture_sao_decide.restype, product.svt_amd_encdec_picture_sao_decide.argtypes = C.c_int, [vp] * 6
    return T.declare(product)


@pytest.fixture(scope="module")
def ctx(lib):
    c = make_context(lib, 640, 384, 2)
    yield c
    lib.svt_amd_context_destroy(c)


def new_picture(lib, ctx, w, h, wide):
    pic = vp()
    ok(lib, lib.svt_amd_encdec_picture_create(ctx, w, h, 2 if wide else 1, C.byref(pic)))
    return pic


def at_stride(records, extra):
    """the records `extra` bytes further apart, junk between them"""
    n, size = len(records), records.dtype.itemsize
    raw = np.full((n, size + extra), 0x5A, np.uint8)
    raw[:, :size] = np.ascontiguousarray(records).view(np.uint8).reshape(n, size)
    return raw.reshape(-1)


class Records:
    """work and result records of one picture in HBM"""

    def __init__(self, lib, ctx, works, results, extra=0):
        self.keep = (at_stride(works, extra), at_stride(results, extra))
        self.work_stride, self.result_stride = works.dtype.itemsize + extra, results.dtype.itemsize + extra
        self.dw, self.dr = DeviceBuffer(lib, ctx, self.keep[0].nbytes), DeviceBuffer(lib, ctx, self.keep[1].nbytes)
        self.dw.put(self.keep[0]), self.dr.put(self.keep[1])

    def free(self):
        self.dw.free(), self.dr.free()


class Tail:
    """one svt_amd_encdec_picture_tail_launch: device outputs with a sentinel behind them, the job, the host `ref`"""

    def __init__(self, lib, ctx, pic, w, h, wide, recs, stages, slice_type=2, ref_poc=(0, 0), sao=None, enable=None, origin=(80, 80)):
        self.lib, self.ctx, self.pic, self.w, self.h, self.wide, self.n = lib, ctx, pic, w, h, wide, S.lcu_count(w, h)
        self.par, self.chk = DeviceBuffer(lib, ctx, self.n * 72 + GUARD), DeviceBuffer(lib, ctx, 16 + GUARD)
        self.en = None
        if enable is not None:
            self.keep_en = np.ascontiguousarray(enable)
            self.en = DeviceBuffer(lib, ctx, self.n)
            self.en.put(self.keep_en)
        self.ref = S.RefPicture()
        self.job = T.job(recs.dw.ptr.value if recs else None, recs.work_stride if recs else 0, recs.dr.ptr.value if recs else None, recs.result_stride if recs else 0, stages,
                         slice_type, ref_poc, sao, self.en.ptr.value if self.en else None, origin)

    def launch(self, ctx=None):
        return self.lib.svt_amd_encdec_picture_tail_launch(ctx or self.ctx, self.pic, C.byref(self.job), self.par.ptr, self.chk.ptr, C.byref(self.ref))

    def params(self, ctx=None):
        raw = self.par.get(ctx)
        assert is_sentinel(raw[self.n * 72:])
        return raw[:self.n * 72].view(LCU)

    def check(self, ctx=None):
        raw = self.chk.get(ctx)
        assert is_sentinel(raw[16:])
        return raw[:16].view(N.CHECK_DTYPE)[0]

    def padded(self, ctx=None):
        """the padded planes behind `ref`, downloaded"""
        sdt = np.uint16 if self.wide else np.uint8
        ox, oy = self.job.origin_x, self.job.origin_y
        assert (self.ref.strideY, self.ref.strideC, self.ref.originX, self.ref.originY, self.ref.width, self.ref.height) == (self.w + 2 * ox, self.w // 2 + ox, ox, oy, self.w, self.h)
        out = []
        for p, ptr in enumerate((self.ref.d_y, self.ref.d_cb, self.ref.d_cr)):
            a = np.zeros(((self.h + 2 * oy) >> (1 if p else 0), (self.w + 2 * ox) >> (1 if p else 0)), sdt)
            ok(self.lib, self.lib.svt_amd_device_download(ctx or self.ctx, a.ctypes.data, vp(ptr), a.nbytes))
            out.append(a)
        return out

    def cropped(self, padded):
        ox, oy = self.job.origin_x, self.job.origin_y
        return [np.ascontiguousarray(a[oy >> s:(oy >> s) + (self.h >> s), ox >> s:(ox >> s) + (self.w >> s)]) for a, s in zip(padded, (0, 1, 1))]

    def free(self):
        for b in (self.par, self.chk, self.en):
            if b:
                b.free()


def fetch_maps(lib, ctx, pic, w, h, wide):
    n = S.lcu_count(w, h)
    sdt = np.uint16 if wide else np.uint8
    got = dict(cumap=np.zeros((h // 8, w // 8), N.CU_MAP_DTYPE), cbf=np.zeros((h // 4, w // 4), np.uint8), qp=np.zeros((h // 8, w // 8), np.uint8))
    by, chk = np.zeros((4, n), np.uint8), np.zeros(1, N.CHECK_DTYPE)
    src = [np.zeros((h, w), sdt), np.zeros((h // 2, w // 2), sdt), np.zeros((h // 2, w // 2), sdt)]
    ok(lib, lib.svt_amd_debug_picture_tail_maps(ctx, pic, got["cumap"].ctypes.data, got["cbf"].ctypes.data, got["qp"].ctypes.data, by.ctypes.data, chk.ctypes.data,
                                                 *[a.ctypes.data for a in src]))
    got.update(edge=by[0], sao_edge=by[1], follow=by[2], status=by[3])
    return got, chk[0], src


def same_maps(got, works, results, w, h, tag):
    want = N.maps(works, T.cbf0_of(results), w, h)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), (tag, k)
    return want


def encode_blocking(lib, ctx, pic, g, refs, first, nl):
    """the existing blocking encode of one fixture picture; -> (works, results as the device returned them)"""
    wide = is16(g)
    works = np.ascontiguousarray(g["work"][first:first + nl])
    got = np.zeros(nl, S.LCU_RESULT16_DTYPE if wide else S.LCU_RESULT_DTYPE)
    if "ref_pocs" in g:
        set_inter(lib, ctx, pic, g, refs, first)
    ok(lib, (lib.svt_amd_encode_picture16 if wide else lib.svt_amd_encode_picture)(ctx, pic, works.ctypes.data, got.ctypes.data))
    return works, got


def fixture_pictures(lib, ctx, name):
    """every picture of a fixture, encoded into one picture object by the blocking entry"""
    g, w, h = load_case(name)
    wide, nl = is16(g), S.lcu_count(w, h)
    refs, keep = device_refs(g, wide) if "ref_pocs" in g else ({}, None)
    pic = new_picture(lib, ctx, w, h, wide)
    try:
        for first in range(0, len(g["work"]), nl):
            works, got = encode_blocking(lib, ctx, pic, g, refs, first, nl)
            poc = [int(v) for v in g["ref_poc"][first]] if "ref_poc" in g else (0, 0)
            yield g, w, h, wide, pic, first, int(g["picture_number"][first]), works, got, poc
    finally:
        lib.svt_amd_encdec_picture_destroy(ctx, pic)


@pytest.mark.parametrize("name", DLF_CASES + SAO_CASES)
def test_maps_of_every_fixture_picture(lib, ctx, name):
    """1. maps, flags and check record of every picture equal the restatement, at the natural record stride and 64 bytes further apart"""
    for g, w, h, wide, pic, first, f, works, got, poc in fixture_pictures(lib, ctx, name):
        for extra in (0, 64):
            recs = Records(lib, ctx, works, got, extra)
            t = Tail(lib, ctx, pic, w, h, wide, recs, D, int(works[0]["slice_type"]), poc)
            try:
                ok(lib, t.launch())
                maps, chk, src = fetch_maps(lib, ctx, pic, w, h, wide)
                same_maps(maps, works, got, w, h, (name, f, extra))
                assert chk.tolist() == (0, N.NONE, 0, N.NONE) and t.check().tolist() == chk.tolist()
                planes, _ = N.source_planes(works, maps["status"], w, h)
                for p in range(3):
                    assert np.array_equal(src[p], planes[p]), (name, f, extra, p)
            finally:
                t.free(), recs.free()


def seeded_records(w, h, slice_type, seed, wide):
    rng = np.random.default_rng(seed)
    heads = random_heads(rng, w, h, slice_type)
    for f in ("tile_left", "tile_top", "tile_right"):
        heads[f] = rng.integers(0, 2, len(heads)) * rng.integers(1, 256, len(heads))
    works = np.zeros(len(heads), S.LCU_WORK16_DTYPE if wide else S.LCU_WORK_DTYPE)
    for f in heads.dtype.names:
        works[f] = heads[f]
    for f in ("src_y", "src_cb", "src_cr"):
        works[f] = rng.integers(0, 1024 if wide else 256, works[f].shape)
    results = np.zeros(len(heads), S.LCU_RESULT16_DTYPE if wide else S.LCU_RESULT_DTYPE)
    results["cu"]["cbf"] = rng.integers(0, 2, results["cu"]["cbf"].shape)
    return works, results


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("w,h,slice_type,seed", [(64, 64, 2, 3), (136, 72, 0, 5), (200, 136, 0, 7), (200, 136, 1, 11)])
def test_maps_and_source_planes_of_seeded_records(lib, ctx, oracle, w, h, slice_type, seed, wide):
    """2. seeded quadtrees (a QP per unit, random cbf, random tile flags, random source samples), 8- and 16-bit records, 16-byte aligned and not: maps, flags and
    the scattered source planes"""
    works, results = seeded_records(w, h, slice_type, seed, wide)
    pic, _, _ = written_picture(lib, ctx, oracle, w, h, wide)
    try:
        for extra in (0, 4):                     # 4: neither the records nor their source rows are 16-byte aligned - the narrow scatter
            recs = Records(lib, ctx, works, results, extra)
            t = Tail(lib, ctx, pic, w, h, wide, recs, D, slice_type, (3, 9))
            try:
                ok(lib, t.launch())
                maps, chk, src = fetch_maps(lib, ctx, pic, w, h, wide)
                want = same_maps(maps, works, results, w, h, (w, h, seed, wide, extra))
                assert chk.tolist() == (0, N.NONE, 0, N.NONE)
                planes, _ = N.source_planes(works, want["status"], w, h)
                for p in range(3):
                    assert np.array_equal(src[p], planes[p]), (w, h, seed, wide, extra, p)
            finally:
                t.free(), recs.free()
    finally:
        lib.svt_amd_encdec_picture_destroy(ctx, pic)


@pytest.mark.parametrize("name", DLF_CASES)
def test_deblocking_matches_the_encoders_output(lib, ctx, name):
    """3. blocking encode, the records uploaded, the tail with SVT_AMD_TAIL_DEBLOCK, one synchronise: the picture is the fixture's (8- and 10-bit)"""
    for g, w, h, wide, pic, first, f, works, got, poc in fixture_pictures(lib, ctx, name):
        recs = Records(lib, ctx, works, got)
        t = Tail(lib, ctx, pic, w, h, wide, recs, D, int(works[0]["slice_type"]), poc)
        try:
            ok(lib, t.launch())
            ok(lib, lib.svt_amd_synchronize(ctx))
            out = encoded_picture(lib, ctx, pic, w, h, np.uint16 if wide else np.uint8)
            for p, nm in enumerate(("recon_y", "recon_cb", "recon_cr")):
                bad = np.argwhere(out[p] != g[nm][f])
                assert len(bad) == 0, (name, f, nm, len(bad), bad[:4].tolist())
        finally:
            t.free(), recs.free()


def stages_of(g, w, h, works, P):
    """what the encoder did with the picture: everything, or - allowEncDecMismatch - the decision alone on the picture as encoded"""
    if allows_mismatch(g, w, h, works[0]):
        return (SD | R) if P is not None else R
    return FULL if P is not None else (D | R)


def fixture_origin(g):
    return (int(g["ref_geom"][2]), int(g["ref_geom"][3])) if "ref_geom" in g else (80, 80)


def check_against_fixture(g, name, f, t, padded, idx=None, want=None, dec=None):
    out = t.cropped(padded)
    for p, nm in enumerate(("recon_y", "recon_cb", "recon_cr")):
        bad = np.argwhere(out[p] != g[nm][f])
        assert len(bad) == 0, (name, f, nm, len(bad), bad[:4].tolist())
    if idx is not None:
        for i in idx:
            assert same_decision(dec[i], want[i]), (name, f, int(i), dec[i], want[i])
    if "ref_pocs" in g and f in g["ref_pocs"].tolist():
        i = g["ref_pocs"].tolist().index(f)
        for p, nm in enumerate(("ref_y", "ref_cb", "ref_cr")):
            assert np.array_equal(padded[p].reshape(-1), g[nm][i]), (name, f, nm)
        return 1
    return 0


@pytest.mark.parametrize("name", SAO_CASES)
def test_sao_and_reference_match_the_encoders_output(lib, ctx, name):
    """4. the full tail (the decision alone plus the padding for the allowEncDecMismatch picture): the encoder's parameters, its finished picture and - padded - the
    reference pictures it predicted from"""
    decided = refs_checked = 0
    for g, w, h, wide, pic, first, f, works, got, poc in fixture_pictures(lib, ctx, name):
        P, enable, params, want, idx = sao_inputs_of_picture(g, f, works, w, h)
        recs = Records(lib, ctx, works, got)
        t = Tail(lib, ctx, pic, w, h, wide, recs, stages_of(g, w, h, works, P), int(works[0]["slice_type"]), poc, P, enable if P is not None else None, fixture_origin(g))
        try:
            ok(lib, t.launch())
            padded = t.padded()
            dec = t.params() if P is not None else None
            refs_checked += check_against_fixture(g, name, f, t, padded, idx if P is not None else None, want, dec)
            if P is not None:
                assert np.array_equal(dec["edge_flags"], params["edge_flags"])
                decided += len(idx)
        finally:
            t.free(), recs.free()
    assert decided >= len(g["work"]) // 2
    assert refs_checked == (len(g["ref_pocs"]) if "ref_pocs" in g else 0)


@pytest.mark.parametrize("name", [c for c in SAO_CASES if "_p_" in c or "_b_" in c])
def test_sequence_stays_on_the_device(lib, ctx, name):
    """5. every picture's records uploaded first; then per picture in coding order set_inter from the earlier tails' `ref`, the device-array encode and the tail - no
    synchronise and no download between the first encode and the last tail; then every picture and every reference is the fixture's"""
    g, w, h = load_case(name)
    assert not is16(g)
    nl = S.lcu_count(w, h)
    firsts = {int(g["picture_number"][k]): k for k in range(0, len(g["work"]), nl)}
    order, known = [], set()
    while len(order) < len(firsts):
        ready = [f for f, k in firsts.items() if f not in known and all(int(v) == NONE_POC or int(v) in known for v in g["ref_poc"][k])]
        assert ready
        order.append(min(ready)), known.add(min(ready))
    recs, pics, tails, inputs = {}, {}, {}, {}
    try:
        for f in order:
            first = firsts[f]
            works = np.ascontiguousarray(g["work"][first:first + nl])
            recs[f] = Records(lib, ctx, works, np.zeros(nl, S.LCU_RESULT_DTYPE))
            pics[f] = new_picture(lib, ctx, w, h, False)
            ok(lib, lib.svt_amd_encdec_picture_tail_warmup(ctx, pics[f], *fixture_origin(g)))
            P, enable, params, want, idx = sao_inputs_of_picture(g, f, works, w, h)
            inputs[f] = (P, want, idx)
            tails[f] = Tail(lib, ctx, pics[f], w, h, False, recs[f], stages_of(g, w, h, works, P), int(works[0]["slice_type"]), [int(v) for v in g["ref_poc"][first]], P,
                            enable if P is not None else None, fixture_origin(g))
        ok(lib, lib.svt_amd_synchronize(ctx))          # the uploads are done; from here on nothing waits
        for f in order:
            first = firsts[f]
            works = g["work"][first:first + nl]
            r0, r1 = (tails[int(v)].ref if int(v) in tails else None for v in g["ref_poc"][first])
            if r0 or r1:
                cost = np.ascontiguousarray(g["cost"][g["cost_pictures"].tolist().index(f)])
                ok(lib, lib.svt_amd_encdec_picture_set_inter(ctx, pics[f], C.byref(r0) if r0 else None, C.byref(r1) if r1 else None, cost.ctypes.data))
            tiles = int(sum(bool(wk["tile_left"]) and bool(wk["tile_top"]) for wk in works))
            free = int(sum(not (wk["cu"]["pred_mode"][:int(wk["num_cus"])] == 2).any() for wk in works))
            ok(lib, lib.svt_amd_encode_picture_device_inter(ctx, pics[f], recs[f].dw.ptr, recs[f].dr.ptr, tiles, free))
            ok(lib, tails[f].launch())
        ok(lib, lib.svt_amd_synchronize(ctx))
        refs_checked = 0
        for f in order:
            P, want, idx = inputs[f]
            t = tails[f]
            assert t.check().tolist() == (0, N.NONE, 0, N.NONE) if t.job.stages & (D | SD) else True
            refs_checked += check_against_fixture(g, name, f, t, t.padded(), idx if P is not None else None, want, t.params() if P is not None else None)
        assert refs_checked == len(g["ref_pocs"])
    finally:
        for f in pics:
            lib.svt_amd_encdec_picture_destroy(ctx, pics[f])
        for f in tails:
            tails[f].free()
        for f in recs:
            recs[f].free()


def blocking_tail(lib, ctx, pic, wide, works, got, prm, P, enable, origin, w, h):
    """the parent's three blocking calls; -> (deblocked planes, finished planes, parameters, padded planes)"""
    sdt = np.uint16 if wide else np.uint8
    dbk = lib.svt_amd_encdec_picture_deblock16 if wide else lib.svt_amd_encdec_picture_deblock
    sao = lib.svt_amd_encdec_picture_sao16 if wide else lib.svt_amd_encdec_picture_sao
    planes = lambda: [np.zeros((h, w), sdt), np.zeros((h // 2, w // 2), sdt), np.zeros((h // 2, w // 2), sdt)]
    d, fin, dec = planes(), planes(), np.zeros(len(works), LCU)
    ok(lib, dbk(ctx, pic, works.ctypes.data, got.ctypes.data, C.byref(prm), *[a.ctypes.data for a in d]))
    ok(lib, sao(ctx, pic, works.ctypes.data, P.ctypes.data, enable.ctypes.data, dec.ctypes.data, *[a.ctypes.data for a in fin]))
    ref = S.RefPicture()
    padded = [np.zeros(((h + 2 * origin[1]) >> s, (w + 2 * origin[0]) >> s), sdt) for s in (0, 1, 1)]
    ok(lib, lib.svt_amd_encdec_picture_reference(ctx, pic, origin[0], origin[1], C.byref(ref), *[a.ctypes.data for a in padded]))
    return d, fin, dec, padded


@pytest.mark.parametrize("name", ["sao_b_tiles_motion_512x320_m6", "sao_i_noise_200x136_m6"])
def test_tail_equals_the_blocking_calls_with_sao_shut_off_in_places(lib, ctx, name):
    """6. a seeded enable mask with a third of the bytes zero: planes, parameters and padded reference byte for byte; a repeated tail gives the same bytes; two objects
    on two lanes, both queued before either is synchronised; the sentinels behind the outputs stay.
    The tail and the blocking calls queue the same device chain (svt_amd_tail_queue_deblock / _sao / _reference), so their equality proves that the two derivations of
    its inputs agree - the blocking entries' host loops against k_tail_maps, context scratch against the object's tail state - and not the chain itself.  The independent
    proof of the chain is the reference encoder's recorded pictures, parameters and padded references: tests 3 to 5 here, and
    test_encode_picture_then_deblock_matches_the_encoders_output, test_encode_deblock_sao_on_the_device_matches_the_encoders_output and
    test_sequence_stays_on_the_device_from_picture_to_picture of tests/test_gpu_encodepass.py; the padding also against numpy.pad
    (test_padded_reference_is_the_edge_replicated_picture there)."""
    g, w, h = load_case(name)
    wide, nl = is16(g), S.lcu_count(w, h)
    refs, keep = device_refs(g, wide) if "ref_pocs" in g else ({}, None)
    rng = np.random.default_rng(61)
    lanes = [vp(), vp()]
    for l in lanes:
        ok(lib, lib.svt_amd_context_fork(ctx, C.byref(l)))
    pics = [new_picture(lib, lanes[k], w, h, wide) for k in range(2)]
    blk = new_picture(lib, ctx, w, h, wide)
    try:
        firsts = list(range(0, len(g["work"]), nl))
        usable = [k for k in firsts if sao_inputs_of_picture(g, int(g["picture_number"][k]), g["work"][k:k + nl], w, h)[0] is not None]
        assert usable
        # the two pictures (two different ones where the fixture has two) in which the encoder switched SAO on most often
        usable.sort(key=lambda k: -int((sao_inputs_of_picture(g, int(g["picture_number"][k]), g["work"][k:k + nl], w, h)[3]["type"] != 0).sum()))
        pair = (usable + usable)[:2]
        want, tails, recs = [], [], []
        for k, first in enumerate(pair):
            f = int(g["picture_number"][first])
            works, got = encode_blocking(lib, ctx, blk, g, refs, first, nl)
            P = sao_inputs_of_picture(g, f, works, w, h)[0]
            enable = (rng.integers(0, 3, nl) != 0).astype(np.uint8)
            assert 0 < int(enable.sum()) < nl
            prm = DeblockParams()
            prm.slice_type = int(works[0]["slice_type"])
            poc = [int(v) for v in g["ref_poc"][first]] if "ref_poc" in g else (0, 0)
            prm.ref_poc[0], prm.ref_poc[1] = poc
            want.append(blocking_tail(lib, ctx, blk, wide, works, got, prm, P, enable, (80, 80), w, h))
            _, got2 = encode_blocking(lib, lanes[k], pics[k], g, refs, first, nl)
            recs.append(Records(lib, lanes[k], works, got2))
            tails.append(Tail(lib, lanes[k], pics[k], w, h, wide, recs[k], FULL, prm.slice_type, poc, P, enable, (80, 80)))
        for l in lanes:
            ok(lib, lib.svt_amd_synchronize(l))       # the uploads
        for rep in range(2):                           # the second round repeats each tail on its object
            for k in range(2):
                ok(lib, tails[k].launch(lanes[k]))     # both lanes hold a tail before either is waited for
            for k in range(2):
                ok(lib, lib.svt_amd_synchronize(lanes[k]))
            for k in range(2):
                d, fin, dec, padded = want[k]
                got_pad = tails[k].padded(lanes[k])
                for p in range(3):
                    assert np.array_equal(got_pad[p], padded[p]), (name, rep, k, "padded", p)
                    assert np.array_equal(tails[k].cropped(got_pad)[p], fin[p]), (name, rep, k, "finished", p)
                assert tails[k].params(lanes[k]).tobytes() == dec.tobytes(), (name, rep, k)
                assert tails[k].check(lanes[k]).tolist() == (0, N.NONE, 0, N.NONE)
                assert (dec["type"][tails[k].keep_en == 0] == 0).all() and (k or (dec["type"] != 0).any())
        # ... and the deblocked planes: a tail that stops there leaves them the latest stage
        for k in range(2):
            tails[k].job.stages = D
            _, got3 = encode_blocking(lib, lanes[k], pics[k], g, refs, pair[k], nl)
            ok(lib, tails[k].launch(lanes[k]))
            out = encoded_picture(lib, lanes[k], pics[k], w, h, np.uint16 if wide else np.uint8)
            for p in range(3):
                assert np.array_equal(out[p], want[k][0][p]), (name, k, "deblocked", p)
    finally:
        for t in tails:
            t.free()
        for r in recs:
            r.free()
        for k in range(2):
            lib.svt_amd_encdec_picture_destroy(lanes[k], pics[k])
        lib.svt_amd_encdec_picture_destroy(ctx, blk)
        for l in lanes:
            lib.svt_amd_context_destroy(l)


@pytest.mark.parametrize("name", ["i_xc_stripes_200x136_m9_q51", "b_xc_binary_200x136_m8_q51"])
def test_object_form_reads_the_records_of_the_mode_decision_call(lib, ctx, name):
    """7. NULL arrays: the records the last svt_amd_md_encode_picture[_inter] call left on the object - equal to the blocking calls on the host records that call
    returned; refused without such a call, after a P / B call without works and results, and on an object with a rank rectangle"""
    from test_gpu_md import md_encode, md_encode_inter, sig as md_sig
    from test_gpu_mdctl_batch import Rect
    md_sig(lib)
    lib.svt_amd_encdec_picture_set_rect.restype, lib.svt_amd_encdec_picture_set_rect.argtypes = C.c_int, [vp, vp, vp]
    g = np.load(os.path.join(S.GOLDEN_DIR, "md_%s.npz" % name))
    w, h = int(g["pic"][0]["width"]), int(g["pic"][0]["height"])
    inter = not name.startswith("i_")
    sg, _, _ = load_case("sao_i_noise_200x136_m6")
    P = params_of(sg["sao"][0])
    nl = S.lcu_count(w, h)
    enable = np.ones(nl, np.uint8)
    c2 = make_context(lib, w, (h + 7) & ~7, 2)
    pic = new_picture(lib, c2, w, h, False)
    t = Tail(lib, c2, pic, w, h, False, None, FULL, 0, (1, 3), P, enable, (80, 80))
    try:
        refused(lib, t.launch(), T.ENTRY, "no mode-decision call yet")
        assert b"no svt_amd_md_encode_picture" in lib.svt_amd_last_error()
        if inter:
            md_encode_inter(lib, c2, pic, g, 0, encode=False)
            refused(lib, t.launch(), T.ENTRY, "decisions only")
            out, works, res = md_encode_inter(lib, c2, pic, g, 0, encode=True)
        else:
            out, works, res = md_encode(lib, c2, pic, g, 0)
        t.job.deblock.slice_type = int(works[0]["slice_type"])
        ok(lib, t.launch())
        got_pad, dec = t.padded(), t.params()
        maps, chk, src = fetch_maps(lib, c2, pic, w, h, False)
        same_maps(maps, works, res, w, h, name)
        prm = DeblockParams()
        prm.slice_type, prm.ref_poc[0], prm.ref_poc[1] = int(works[0]["slice_type"]), 1, 3
        d, fin, want_dec, padded = blocking_tail(lib, c2, pic, False, works, res, prm, P, enable, (80, 80), w, h)
        for p in range(3):
            assert np.array_equal(got_pad[p], padded[p]), (name, p)
        assert dec.tobytes() == want_dec.tobytes() and (want_dec["type"] != 0).any()
        # one array without the other is no object form
        t.job.d_works = t.par.ptr.value
        refused(lib, t.launch(), T.ENTRY, "half a pair")
        t.job.d_works = None
        whole = Rect(0, 0, 64, 64)
        ok(lib, lib.svt_amd_encdec_picture_set_rect(c2, pic, C.byref(whole)))
        refused(lib, t.launch(), T.ENTRY, "rank rectangle")
        assert b"rank rectangle" in lib.svt_amd_last_error()
        ok(lib, lib.svt_amd_encdec_picture_set_rect(c2, pic, None))
        ok(lib, t.launch())
    finally:
        t.free()
        lib.svt_amd_encdec_picture_destroy(c2, pic)
        lib.svt_amd_context_destroy(c2)


@pytest.mark.parametrize("name", [c for c in INTER_CASES if c.startswith(("p10_", "b10_"))])
def test_sixteen_bit_device_array_twins_equal_the_host_array_call(lib, ctx, name):
    """8. svt_amd_encode_picture_device16 and svt_amd_encode_picture_device_inter16 against svt_amd_encode_picture16: every result field the contract defines and
    the picture in HBM, byte for byte (the two 10-bit I fixtures run through tests 3 and 4)"""
    g, w, h = load_case(name)
    assert is16(g)
    nl = S.lcu_count(w, h)
    refs, keep = device_refs(g, True)
    pic, dev = new_picture(lib, ctx, w, h, True), new_picture(lib, ctx, w, h, True)
    try:
        for first in range(0, len(g["work"]), nl):
            works, want = encode_blocking(lib, ctx, pic, g, refs, first, nl)
            want_pic = encoded_picture(lib, ctx, pic, w, h, np.uint16)
            tiles = int(sum(bool(wk["tile_left"]) and bool(wk["tile_top"]) for wk in works))
            free = int(sum(not (wk["cu"]["pred_mode"][:int(wk["num_cus"])] == 2).any() for wk in works))
            for how in ("device16", "device_inter16"):
                recs = Records(lib, ctx, works, np.zeros(nl, S.LCU_RESULT16_DTYPE))
                try:
                    set_inter(lib, ctx, dev, g, refs, first)
                    if how == "device16":
                        ok(lib, lib.svt_amd_encode_picture_device16(ctx, dev, recs.dw.ptr, recs.dr.ptr, max(tiles, 1)))
                    else:
                        ok(lib, lib.svt_amd_encode_picture_device_inter16(ctx, dev, recs.dw.ptr, recs.dr.ptr, max(tiles, 1), free))
                    got = recs.dr.get().view(S.LCU_RESULT16_DTYPE)
                    for k in range(nl):
                        compare_lcu(works[k], want[k], got[k], w, h, (name, how, k), rec=not (int(g["dlf_off"][first + k]) & 2))
                    got_pic = encoded_picture(lib, ctx, dev, w, h, np.uint16)
                    for p in range(3):
                        assert np.array_equal(got_pic[p], want_pic[p]), (name, how, first, p)
                finally:
                    recs.free()
    finally:
        lib.svt_amd_encdec_picture_destroy(ctx, pic)
        lib.svt_amd_encdec_picture_destroy(ctx, dev)


def test_refusals_name_the_entry_and_write_nothing(lib, ctx, oracle):
    """9a. on a real object: stage rules, strides of the other sample width, alignment - the outputs keep their sentinel, `ref` stays empty, the object's state stays"""
    w, h = 128, 64
    pic, works, res = written_picture(lib, ctx, oracle, w, h, True)
    recs = Records(lib, ctx, works, res)
    P = params_of(load_case("sao_i_noise_200x136_m6")[0]["sao"][0])
    P["is_10bit"] = 1
    t = Tail(lib, ctx, pic, w, h, True, recs, FULL, 2, (0, 0), P, None, (80, 80))
    try:
        for what, change in (("apply without deblock", dict(stages=SD | A)), ("apply without decide", dict(stages=D | A)), ("no stage", dict(stages=0)), ("stage 16", dict(stages=16)),
                             ("odd padding", dict(origin_x=81)), ("8-bit work stride", dict(work_stride=S.LCU_WORK_DTYPE.itemsize)),
                             ("8-bit result stride", dict(result_stride=S.LCU_RESULT_DTYPE.itemsize)), ("stride no multiple of 4", dict(work_stride=recs.work_stride + 2)),
                             ("pad", dict(pad=7))):
            keep = {k: getattr(t.job, k) for k in change}
            for k, v in change.items():
                setattr(t.job, k, v)
            refused(lib, t.launch(), T.ENTRY, what)
            for k, v in keep.items():
                setattr(t.job, k, v)
        refused(lib, lib.svt_amd_encdec_picture_tail_launch(ctx, pic, C.byref(t.job), t.par.ptr, t.chk.ptr, None), T.ENTRY, "reference without ref")
        refused(lib, lib.svt_amd_encdec_picture_tail_launch(ctx, pic, C.byref(t.job), vp(t.par.ptr.value + 2), t.chk.ptr, C.byref(t.ref)), T.ENTRY, "parameter alignment")
        fresh = new_picture(lib, ctx, w, h, True)
        refused(lib, lib.svt_amd_encdec_picture_tail_launch(ctx, fresh, C.byref(t.job), t.par.ptr, t.chk.ptr, C.byref(t.ref)), T.ENTRY, "nothing encoded")
        lib.svt_amd_encdec_picture_destroy(ctx, fresh)
        refused(lib, lib.svt_amd_debug_picture_tail_maps(ctx, pic, None, None, None, None, None, None, None, None), T.DEBUG_ENTRY, "no tail yet")
        ok(lib, lib.svt_amd_synchronize(ctx))
        assert is_sentinel(t.par.get()) and is_sentinel(t.chk.get()) and t.ref.d_y is None and t.ref.strideY == 0
        ok(lib, t.launch())                            # ... and the same job passes untouched
        assert not is_sentinel(t.params()) and t.check().tolist() == (0, N.NONE, 0, N.NONE) and t.ref.strideY == w + 160
    finally:
        t.free(), recs.free()
        lib.svt_amd_encdec_picture_destroy(ctx, pic)


def malformed():
    two = random_heads(np.random.default_rng(21), 128, 64, 0)
    cases = {k: (v[0], 128, 64, v[1]) for k, v in T.malformed_cases(two).items()}
    hd, want = T.outside_case(random_heads(np.random.default_rng(22), 200, 136, 0))
    cases["a unit outside the picture"] = (hd, 200, 136, want)
    return cases


@pytest.mark.parametrize("what", sorted(malformed()))
def test_malformed_records_are_counted_on_the_device(lib, ctx, oracle, what):
    """9b. the records the host loops refuse (tests/test_tail_cpu.py runs the same routine over them under the sanitizers first): the documented check record, the maps
    of the restatement - an offending unit or LCU writes nothing, its cells are 0 - and source planes untouched where an LCU is refused"""
    heads, w, h, want = malformed()[what]
    works = np.zeros(len(heads), S.LCU_WORK_DTYPE)
    for f in heads.dtype.names:
        works[f] = heads[f]
    works["src_y"], works["src_cb"], works["src_cr"] = 200, 90, 30
    results = np.ones(len(heads), S.LCU_RESULT_DTYPE)
    pic, good_works, good_res = written_picture(lib, ctx, oracle, w, h, False)
    good = Records(lib, ctx, good_works, good_res)
    recs = Records(lib, ctx, works, results)
    t0 = Tail(lib, ctx, pic, w, h, False, good, D)
    t = Tail(lib, ctx, pic, w, h, False, recs, D, 0, (1, 2))
    try:
        ok(lib, t0.launch())                           # the source planes hold the valid picture's samples first
        _, _, before = fetch_maps(lib, ctx, pic, w, h, False)
        ok(lib, t.launch())
        assert t.check().tolist() == want, what
        maps, chk, src = fetch_maps(lib, ctx, pic, w, h, False)
        assert chk.tolist() == want
        wanted = same_maps(maps, works, results, w, h, what)
        planes, known = N.source_planes(works, wanted["status"], w, h)
        for p in range(3):
            assert np.array_equal(src[p], np.where(known[p], planes[p], before[p])), (what, p)
    finally:
        t.free(), t0.free(), recs.free(), good.free()
        lib.svt_amd_encdec_picture_destroy(ctx, pic)
