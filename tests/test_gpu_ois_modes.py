"""-m gpu: open-loop intra search against the oracle where the four-samples-a-lane predictor can go wrong: every one of the 35 modes ranked
(ois_kernel_level = 1) at 32x32, 16x16 and 8x8, the picture's left / top LCU edges (reference samples 128), partial right and bottom LCUs, a
height that is a multiple of 8 but not of 16, and a 64-picture batch at 1920x1080 (parameter sets mixed in one launch) against per-picture
launches."""
import ctypes as C

import numpy as np
import pytest

import svtlib as S
from gpu_util import default_params, me_picture, upload
from test_gpu_ois import VARIANTS, mk_params, ois_picture, same
from test_oracle_ois_golden import me_like

pytestmark = pytest.mark.gpu


def content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "flat":
        return np.full((h, w), 128, np.uint8)
    if kind == "dark":  # far from the 128 that stands in for out-of-picture references, so a wrong edge reference shows in every SAD
        return (20 + rng.integers(0, 8, (h, w))).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "blocks":  # constant 8x8 blocks: exact predictions, many equal SADs (ties between modes)
        b = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8), dtype=np.uint8)
        return np.kron(b, np.ones((8, 8), np.uint8))[:h, :w].copy()
    # "stripes": a direction per 32x32 area, so that every angular mode wins somewhere
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ang = rng.uniform(0, np.pi, ((h + 31) // 32, (w + 31) // 32))
    th = np.kron(ang, np.ones((32, 32)))[:h, :w]
    per = 5.0 + 7.0 * rng.random()
    v = 128 + 90 * np.sin((x * np.cos(th) + y * np.sin(th)) * (2 * np.pi / per)) + rng.integers(-6, 7, (h, w))
    return np.clip(v, 0, 255).astype(np.uint8)


def random_me(params, seed):
    n = S.lcu_count(params.luma_width, params.luma_height)
    rng = np.random.default_rng(seed)
    return me_like(rng.integers(0, 6000, (n, 85)).astype(np.uint32) * (rng.integers(0, 4, (n, 85)) > 0))


# 200 = 3 * 64 + 8, 136 = 2 * 64 + 8: the last LCU column / row holds 8x8 CUs only; 232 = 3 * 64 + 40: one 32x32 and an 8-wide column of
# 8x8 CUs; 200 rows: a multiple of 8 but not of 16 (the API takes multiples of 8)
SIZES = [(200, 136), (232, 200), (328, 264)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kind", ["flat", "dark", "noise", "blocks", "stripes"])
def test_all_modes_ranked_matches_oracle(product, gpu_ctx, oracle, kind, w, h):
    luma = content(kind, w, h, 5)
    upload(product, gpu_ctx, 0, luma)
    params = mk_params(w, h, ois_kernel_level=1, skip_ois_8x8=0, cu8x8_mode=0, temporal_layer_index=1)
    me = random_me(params, 1)
    want = S.oracle_ois_picture(oracle, params, luma, me)
    got = ois_picture(product, gpu_ctx, params, 0, me)
    assert same(got, want), (kind, w, h)
    if kind == "stripes":  # the ranking is real: nearly every mode reaches some CU's top 18
        modes = (want["candidate"][:, 1:, :] >> 24) & 0xFF
        mask = ((want["candidate"][:, 1:, :] >> 23) & 1).astype(bool)
        assert len(set(modes[mask].ravel().tolist())) >= 33


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("v", range(len(VARIANTS)))
def test_variants_at_partial_lcus_match_oracle(product, gpu_ctx, oracle, v, w, h):
    luma = content("stripes", w, h, 7 + v)
    upload(product, gpu_ctx, 0, luma)
    params = mk_params(w, h, **VARIANTS[v])
    me = None if params.slice_is_intra else random_me(params, 10 + v)
    assert same(ois_picture(product, gpu_ctx, params, 0, me), S.oracle_ois_picture(oracle, params, luma, me)), (VARIANTS[v], w, h)


BATCH_PARAMS = [
    dict(skip_ois_8x8=1, cu8x8_mode=1, temporal_layer_index=2),  # the benchmarked configuration
    dict(skip_ois_8x8=0, cu8x8_mode=0, ois_th_set=2, temporal_layer_index=1),
    dict(ois_kernel_level=1, skip_ois_8x8=0, cu8x8_mode=0),
    dict(slice_is_intra=1),
    dict(limit_ois_to_dc_mode=1, skip_ois_8x8=1),
    dict(skip_ois_8x8=0, cu8x8_mode=1, ois_th_set=0, temporal_layer_index=3, set_best_ois_distortion_to_valid=1),
]


def test_batch_64_1080p_matches_single(product, oracle):
    """64 pictures in one launch, twice: with parameter sets that include ois_kernel_level (the 35-column instance runs every picture) and
    without; every picture == its own launch, two of them == the oracle."""
    w, h, n = 1920, 1080, 64
    ctx = C.c_void_p()
    assert product.svt_amd_context_create(0, w, h, n, C.byref(ctx)) == 0, product.svt_amd_last_error()
    try:
        base = [S.gen_luma("motion", w, h, t, 13) for t in range(4)]
        frames = [np.roll(base[t % 4], (7 * (t // 4), 11 * (t // 4)), axis=(0, 1)) for t in range(n)]
        for t, f in enumerate(frames):
            upload(product, ctx, t, f)
        mp = default_params(w, h)
        me = {t: me_picture(product, ctx, mp, t, [t - 1]) for t in range(1, n)}  # ME records stay in the slots: OIS reads them there
        for with_kl in (True, False):
            plist = [p for p in BATCH_PARAMS if with_kl or not p.get("ois_kernel_level")]
            params = [mk_params(w, h, **(plist[t % len(plist)] if t else dict(slice_is_intra=1))) for t in range(n)]
            jobs = (S.OisJob * n)()
            for t in range(n):
                jobs[t].params, jobs[t].cur_slot = params[t], t
            assert product.svt_amd_ois_batch_launch(ctx, jobs, n) == 0, product.svt_amd_last_error()
            batch = []
            for t in range(n):
                got = np.zeros(S.lcu_count(w, h), S.OIS_LCU_DTYPE)
                assert product.svt_amd_ois_picture_fetch(ctx, t, got.ctypes.data) == 0, product.svt_amd_last_error()
                batch.append(got)
            for t in range(n):
                assert same(batch[t], ois_picture(product, ctx, params[t], t, None)), (with_kl, t)
            for t in (1, 2):  # picture 2: ois_kernel_level in the first batch
                assert same(batch[t], S.oracle_ois_picture(oracle, params[t], frames[t], me[t])), (with_kl, t)
    finally:
        product.svt_amd_context_destroy(ctx)
