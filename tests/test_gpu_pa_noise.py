"""-m gpu: the batched noise detection (svt_amd_noise_detect_batch_launch; svt-hevc_amd/csrc/noise_kernels.hip) - (1) against what the REFERENCE's
PicturePreProcessingOperations computed (tests/golden/panoise_*.npz), (2) seeded variants and (3) one batch that mixes the three methods and both thresholds
against the numpy restatement the CPU suite pins on those fixtures (tests/pa_noise_numpy.py), (4) pictures at the extremes, (5) 64x64 with each method,
(6) two batches back to back on one context, (7) planes built on another lane, (8) the parameter checks.  Everything is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import pa_noise_numpy as N
import pa_noise_pictures as P
import svtlib as S
from gpu_util import upload
from pa_batch_util import SENTINEL, DeviceBuffer, make_context as _context, ok as _ok, refused as _refused
from test_pa_noise_cpu import CASES, load_case

pytestmark = pytest.mark.gpu
vp = C.c_void_p
ENTRY = "svt_amd_noise_detect_batch_launch"
METHODS = (P.HALF, P.QUARTER, P.FULL)


@pytest.fixture(scope="module")
def lib(product):
    return N.declare(product)


class Arrays:
    """the two device arrays, with room for `room` pictures, filled with SENTINEL"""

    def __init__(self, lib, ctx, room, w, h):
        self.lib, self.ctx, self.size = lib, ctx, N.sizes(w, h)
        self.buf = [DeviceBuffer(lib, ctx, room * b) for b in self.size]

    def table(self):
        return N.NoiseArrays(self.buf[0].ptr.value, self.buf[1].ptr.value)

    def launch(self, specs, ctx=None, table=None):
        """specs: (slot, method, threshold) per picture; -> the return code"""
        jobs = N.make_jobs(specs)
        t = table or self.table()
        return self.lib.svt_amd_noise_detect_batch_launch(ctx or self.ctx, jobs, len(jobs), C.byref(t))

    def download(self, n, ctx=None):
        """waits for the context's stream -> (flat [n][bytes], picture records [n]); everything beyond picture n must still be the sentinel"""
        raw = []
        for buf, b in zip(self.buf, self.size):
            out = buf.get(ctx)
            assert (out[n * b:] == SENTINEL).all(), "the batch wrote beyond its %d pictures" % n
            raw.append(out[:n * b])
        return raw[0].reshape(n, self.size[0]), raw[1].view(N.PIC_DTYPE).reshape(n)

    def untouched(self):
        """every byte of both arrays is still the sentinel (download(0) asserts it)"""
        flat, pic = self.download(0)
        return flat.size == 0 and pic.size == 0

    def free(self):
        for buf in self.buf:
            buf.free()


def _assert_equals_checker(flat, pic, i, luma, method, th, what):
    want_flat, want_pic = N.detect(luma, method, th)
    assert np.array_equal(flat[i], want_flat), (what, i, "flat_noise", np.argwhere(flat[i] != want_flat)[:4].tolist())
    assert pic[i].tobytes() == want_pic.tobytes(), (what, i, pic[i], want_pic)
    return want_flat, want_pic


def _run(lib, w, h, lumas, specs, room_extra=1):
    """lumas into slots 0.., one batch of specs (slot, method, threshold) -> (flat, picture)"""
    ctx = _context(lib, w, h, len(lumas))
    arrays = None
    try:
        arrays = Arrays(lib, ctx, len(specs) + room_extra, w, h)
        for s, luma in enumerate(lumas):
            upload(lib, ctx, s, luma)
        _ok(lib, arrays.launch(specs))
        return arrays.download(len(specs))
    finally:
        if arrays:
            arrays.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 1. the reference's own records ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_one_batch_per_case_gives_what_the_reference_computed(lib, name):
    g, method, w, h, specs = load_case(name)
    lcus = N.lcu_count(w, h)
    lumas = [P.picture(w, h, s) for s in specs]
    jobs = [(i, method, th) for i in range(len(specs)) for th in (0, 1)]
    flat, pic = _run(lib, w, h, lumas, jobs)
    for k, (i, _, th) in enumerate(jobs):
        what = (name, i, th)
        assert np.array_equal(flat[k][:lcus], g["flat_noise"][i, th]) and not flat[k][lcus:].any(), what + (np.argwhere(flat[k][:lcus] != g["flat_noise"][i, th])[:4].tolist(),)
        assert int(pic[k]["noise_variance_sum"]) == int(g["noise_variance_sum"][i, th]), what
        assert int(pic[k]["block_count"]) == int(g["block_count"][i, th]), what
        assert int(pic[k]["pic_noise_class"]) == int(g["pic_noise_class"][i, th]) and not pic[k]["pad"].any(), what
        assert N.variance_float(pic[k]) == float(g["noise_variance_float"][i, th]), what


# ---- 2. seeded variants against the numpy checker --------------------------------------------------------------------------------------------

def _variants(w, h, seed):
    """other seeds, bases, ramps and rectangles than the recorded pictures: noise and texture rectangles that straddle LCUs"""
    wl, hl = (w + 63) // 64, (h + 63) // 64
    rng = np.random.default_rng(seed)
    out = []
    for amp in (0, 7, 15, 28, 50):
        rects = [(int(rng.integers(0, wl)), int(rng.integers(0, hl)), int(rng.integers(1, 3)), int(rng.integers(1, 3)), kind, int(rng.integers(3, 45)))
                 for kind in ("clean", "noise", "texture", "noise")]
        out.append(P.spec(seed * 100 + amp, amp, base=int(rng.integers(70, 150)), ramp=int(rng.choice([0, 8, 32])), rects=rects))
    return out


@pytest.mark.parametrize("w,h", [(192, 136), (416, 240), (512, 512), (256, 768)])
def test_seeded_variants_match_the_checker(lib, w, h):
    """one batch per geometry: five pictures, each with the three methods and both thresholds; 512x512 has several 64x64 blocks in every method, 256x768 is the
    tall shape (the 1/16 picture 64 x 192: three block rows of one block), 192x136 a partial right column and bottom row"""
    lumas = [P.picture(w, h, s) for s in _variants(w, h, w + h)]
    jobs = [(i, m, th) for i in range(len(lumas)) for m in METHODS for th in (0, 1)]
    flat, pic = _run(lib, w, h, lumas, jobs)
    flagged = 0
    for k, (i, m, th) in enumerate(jobs):
        want_flat, _ = _assert_equals_checker(flat, pic, k, lumas[i], m, th, (w, h, P.METHOD_NAME[m], th))
        flagged += int(want_flat.sum())
    assert flagged


# ---- 3. one batch mixing the methods and the thresholds ----------------------------------------------------------------------------------------

def test_one_batch_mixes_methods_and_thresholds_across_pictures(lib):
    w, h = 704, 640
    specs = [P.spec(900 + i, a, base=100 + 5 * i, ramp=(0, 16, 32)[i % 3]) for i, a in enumerate((5, 9, 14, 22, 33, 47, 6))]
    lumas = [P.picture(w, h, s) for s in specs]
    jobs = [(i, METHODS[i % 3], i & 1) for i in range(len(lumas))] + [(0, P.FULL, 1), (0, P.QUARTER, 0)]          # ... and one slot read by three jobs
    flat, pic = _run(lib, w, h, lumas, jobs)
    for k, (i, m, th) in enumerate(jobs):
        _assert_equals_checker(flat, pic, k, lumas[i], m, th, ("mixed", P.METHOD_NAME[m], th))
    assert len(set(int(p["block_count"]) for p in pic)) == 3 and len(set(int(p["pic_noise_class"]) for p in pic)) > 1


# ---- 4. the extremes ---------------------------------------------------------------------------------------------------------------------------

def test_pictures_at_the_extremes(lib):
    """all 0, all 255, a 0 / 255 checkerboard (the largest filter sums and noise samples: 255 - 127) and one noisy LCU in a flat picture, each with every method"""
    w, h = 320, 256
    rng = np.random.default_rng(3)
    single = np.full((h, w), 90, np.uint8)
    single[64:128, 128:192] = 90 + rng.integers(-9, 10, size=(64, 64))
    lumas = [np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8), P.checkerboard(w, h), single]
    jobs = [(i, m, th) for i in range(4) for m in METHODS for th in (0, 1)]
    flat, pic = _run(lib, w, h, lumas, jobs)
    for k, (i, m, th) in enumerate(jobs):
        want_flat, want_pic = _assert_equals_checker(flat, pic, k, lumas[i], m, th, ("extremes", i, P.METHOD_NAME[m], th))
        if i < 2:
            assert not want_flat.any() and want_pic["noise_variance_sum"] == 0 and want_pic["pic_noise_class"] == 1
        if i == 2 and m == P.FULL:
            assert want_pic["pic_noise_class"] == 4 and want_flat.sum() == 9     # denoised 127, noise 128 / 0; the LCUs without the copied first row, first and last column (the last row is odd: the 64x64 variance does not read it)
        if i == 3 and m == P.FULL:
            assert want_flat.sum() == 1 and want_flat[1 * 5 + 2] == 1


# ---- 5. 64x64 ----------------------------------------------------------------------------------------------------------------------------------

def test_64x64_with_each_method(lib):
    """the full method evaluates the one LCU; the 1/4 picture (32x32) and the 1/16 picture (16x16) hold no 64x64 block: no blocks, sum 0, class 1, no flags"""
    w = h = 64
    lumas = [P.picture(w, h, P.spec(77, 12, rects=()))]
    jobs = [(0, m, th) for m in METHODS for th in (0, 1)]
    flat, pic = _run(lib, w, h, lumas, jobs)
    for k, (i, m, th) in enumerate(jobs):
        _assert_equals_checker(flat, pic, k, lumas[0], m, th, ("64x64", P.METHOD_NAME[m], th))
        if m == P.FULL:
            assert pic[k]["block_count"] == 1 and pic[k]["noise_variance_sum"] > 0 and flat[k][0] == 1
        else:
            assert pic[k].tobytes() == np.array((0, 0, 1, 0), N.PIC_DTYPE).tobytes() and not flat[k].any()


# ---- 6. two batches back to back ---------------------------------------------------------------------------------------------------------------

def test_two_batches_back_to_back_on_one_context(lib):
    """nothing waited for between the two calls: the second batch's descriptor table and its zeroing of the partial sums must not reach the first one's kernels,
    and the sums of the first (noisy) batch must not leak into the second (clean) one, which reuses the same scratch entries"""
    w, h = 416, 240
    ctx = _context(lib, w, h, 5)
    first = second = None
    try:
        first, second = Arrays(lib, ctx, 7, w, h), Arrays(lib, ctx, 4, w, h)
        lumas = [P.picture(w, h, P.spec(500 + i, a)) for i, a in enumerate((40, 25, 60))] + [P.picture(w, h, P.spec(600, 0, ramp=0, rects=())), P.picture(w, h, P.spec(601, 3))]
        for s, luma in enumerate(lumas):
            upload(lib, ctx, s, luma)
        ja = [(0, P.FULL, 0), (1, P.QUARTER, 1), (2, P.HALF, 0), (0, P.QUARTER, 1), (2, P.FULL, 1)]
        jb = [(3, P.FULL, 1), (4, P.QUARTER, 1), (3, P.QUARTER, 0)]
        _ok(lib, first.launch(ja))
        _ok(lib, second.launch(jb))
        fa, pa = first.download(len(ja))                                         # one wait; the tails of both arrays keep the sentinel
        fb, pb = second.download(len(jb))
        for flat, pic, jobs in ((fa, pa, ja), (fb, pb, jb)):
            for k, (i, m, th) in enumerate(jobs):
                _assert_equals_checker(flat, pic, k, lumas[i], m, th, ("batch of %d" % len(jobs), P.METHOD_NAME[m]))
        assert pa[0]["noise_variance_sum"] > 0 and pb[0]["noise_variance_sum"] == 0
    finally:
        for a in (first, second):
            if a:
                a.free()
        lib.svt_amd_context_destroy(ctx)


# ---- 7. planes built on another lane -----------------------------------------------------------------------------------------------------------

def test_planes_built_on_another_lane(lib):
    """the pictures go up and their planes are built on one lane (asynchronously), the batch is launched on another one right away: the entry waits on the
    device for every slot it reads"""
    w, h, n = 704, 640, 4
    root = _context(lib, w, h, n)
    lane_in, lane_k = vp(), vp()
    arrays, d_stage = None, vp()
    try:
        _ok(lib, lib.svt_amd_context_fork(root, C.byref(lane_in)))
        _ok(lib, lib.svt_amd_context_fork(root, C.byref(lane_k)))
        arrays = Arrays(lib, root, n + 1, w, h)
        _ok(lib, lib.svt_amd_device_alloc(root, n * w * h, C.byref(d_stage)))
        lumas = [P.picture(w, h, P.spec(700 + i, a)) for i, a in enumerate((8, 20, 35, 55))]
        staged = np.ascontiguousarray(np.stack(lumas))
        _ok(lib, lib.svt_amd_device_upload_async(lane_in, d_stage, staged.ctypes.data, staged.size))
        for s in range(n):
            _ok(lib, lib.svt_amd_picture_upload_device(lane_in, s, vp(d_stage.value + s * w * h), w, w, h))
        jobs = [(s, METHODS[s % 3], s & 1) for s in range(n)]
        _ok(lib, arrays.launch(jobs, ctx=lane_k))
        flat, pic = arrays.download(n, ctx=lane_k)
        for k, (i, m, th) in enumerate(jobs):
            _assert_equals_checker(flat, pic, k, lumas[i], m, th, ("two lanes", P.METHOD_NAME[m]))
        _ok(lib, lib.svt_amd_synchronize(lane_in))
    finally:
        if arrays:
            arrays.free()
        if d_stage:
            lib.svt_amd_device_free(root, d_stage)
        for lane in (lane_k, lane_in):
            if lane:
                lib.svt_amd_context_destroy(lane)
        lib.svt_amd_context_destroy(root)


# ---- 8. parameter checks -----------------------------------------------------------------------------------------------------------------------

def test_refused_batches_name_the_job_and_queue_nothing(lib):
    w, h = 416, 240
    ctx = _context(lib, w, h, 4)
    arrays = None
    try:
        arrays = Arrays(lib, ctx, 4, w, h)
        lumas = [P.picture(w, h, P.spec(800 + i, 10 + 10 * i)) for i in range(2)]
        for s, luma in enumerate(lumas):
            upload(lib, ctx, s, luma)
        upload(lib, ctx, 2, P.picture(200, 136, P.spec(802, 10)))               # slot 2: a picture of another size; slot 3: none

        def refused(rc, job):
            _refused(lib, rc, ENTRY, job)
            assert ("job %d" % job).encode() in lib.svt_amd_last_error(), lib.svt_amd_last_error()

        good = [(0, P.FULL, 0), (1, P.HALF, 1), (0, P.QUARTER, 1)]
        for missing in ("flat_noise", "picture"):                                # a NULL array
            t = arrays.table()
            setattr(t, missing, None)
            refused(arrays.launch(good, table=t), 0)
        for method in (3, 7, 255):                                               # an unknown method
            refused(arrays.launch([(0, P.FULL, 0), (1, method, 1), (0, P.HALF, 0)]), 1)
        for th in (2, 255):                                                      # a threshold above 1
            refused(arrays.launch([(0, P.FULL, 0), (1, P.HALF, 1), (0, P.QUARTER, th)]), 2)
        for slot in (3, 4, -1):                                                  # a slot without a picture, no such slot
            refused(arrays.launch([(0, P.FULL, 0), (slot, P.FULL, 0)]), 1)
        refused(arrays.launch([(3, P.FULL, 0), (0, P.FULL, 0)]), 0)
        refused(arrays.launch([(0, P.FULL, 0), (1, P.FULL, 0), (2, P.FULL, 0)]), 2)         # a slot of another size than job 0's
        refused(arrays.launch([(2, P.HALF, 0), (1, P.HALF, 0)]), 1)
        big = (N.NoiseJob * 257)()
        t = arrays.table()
        for count in (0, 257):
            _refused(lib, lib.svt_amd_noise_detect_batch_launch(ctx, big, count, C.byref(t)), ENTRY, count)
            assert b"jobs" in lib.svt_amd_last_error()
        _ok(lib, lib.svt_amd_synchronize(ctx))
        assert arrays.untouched(), "a refused batch wrote"
        # ... and a following complete batch on the same context is right
        _ok(lib, arrays.launch(good))
        flat, pic = arrays.download(len(good))
        for k, (i, m, th) in enumerate(good):
            _assert_equals_checker(flat, pic, k, lumas[i], m, th, "after the refused batches")
    finally:
        if arrays:
            arrays.free()
        lib.svt_amd_context_destroy(ctx)
