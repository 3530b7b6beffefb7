"""Seeded pictures of the noise-detection tests (svt_amd_noise_detect_batch_launch): a flat or gently ramped background with seeded uniform noise of a chosen
amplitude, and rectangles that are clean, noisy with their own amplitude, or textured.  tests/golden/make_pa_noise_golden.py and the tests build their inputs
here from the same specification, so both see the same samples; the fixtures hold the specifications, not the planes."""
import numpy as np

HALF, QUARTER, FULL = 0, 1, 2            # the reference's EB_NOISE_DETECT_MODE (Codec/EbDefinitions.h:1207-1209)
METHOD_NAME = {HALF: "half", QUARTER: "quarter", FULL: "full"}

# the rectangles every recorded picture carries, in LCUs (x, y, w, h), kind, amplitude:
#   (1, 1) clean and flat: in a decimated method it stands below the noisy (1, 0) in the same 64x64 block of the decimated picture and takes ITS noise variance
#   (1, 3) textured on top of the background's noise: the same noise in its own rows as (1, 2) above it, but a denoised variance far above 50
#   (2, 0) noise of amplitude 6 on a flat ground: a noise variance between the two thresholds
TEXTURED = (1, 3)                        # the textured LCU; the CPU test reads it from here
RECTS = ((1, 1, 1, 1, "clean", 0), TEXTURED + (1, 1, "texture", 40), (2, 0, 1, 1, "noise", 6))
AMPLITUDES = (0, 4, 6, 9, 13, 17, 21, 26, 31, 36, 42, 48, 56, 64)

#        method, width, height
CASES = {
    "full_200x136": (FULL, 200, 136),        # a partial right column and bottom row; 3 x 2 complete LCUs; noiseTh 25
    "full_320x768": (FULL, 320, 768),        # noiseTh 0
    "half_704x640": (HALF, 704, 640),        # 1/16 picture 176 x 160: LCU columns 8 - 10 and rows 8 - 9 are never evaluated; noiseTh 25
    "half_256x1024": (HALF, 256, 1024),      # taller than wide: the `block64x64Y + 64 > width` path (:3100); noiseTh 10
    "half_256x1152": (HALF, 256, 1152),      # noiseTh 0
    "half_64x64": (HALF, 64, 64),            # zero blocks
    "quarter_416x240": (QUARTER, 416, 240),  # 1/4 picture 208 x 120: one block row; the rows beyond it are not evaluated
    "quarter_256x512": (QUARTER, 256, 512),  # two block rows
}


def spec(seed, amp, base=120, ramp=16, rects=RECTS):
    """a picture specification: plain data, kept in the fixtures"""
    return dict(seed=int(seed), amp=int(amp), base=int(base), ramp=int(ramp), rects=[list(r) for r in rects])


def case_specs(name):
    """the recorded pictures of a case: one per background amplitude (each runs with both thresholds)"""
    k = sorted(CASES).index(name)
    return [spec(1000 * (k + 1) + i, a, base=120 - 8 * (i & 1), ramp=(0, 16)[i & 1]) for i, a in enumerate(AMPLITUDES)]


def picture(w, h, s):
    """the luma of specification s: base (+ one level every `ramp` columns) + uniform noise in [-amp, amp]; rectangles in LCUs"""
    rng = np.random.default_rng(s["seed"])
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    ground = s["base"] + (x // s["ramp"] if s["ramp"] else 0 * x) + 0 * y
    l = ground.astype(np.int64)
    if s["amp"]:
        l = l + rng.integers(-s["amp"], s["amp"] + 1, size=(h, w))
    for rx, ry, rw, rh, kind, amp in s["rects"]:
        x0, y0, x1, y1 = 64 * rx, 64 * ry, min(64 * (rx + rw), w), min(64 * (ry + rh), h)
        if x0 >= x1 or y0 >= y1:
            continue
        if kind == "clean":
            l[y0:y1, x0:x1] = ground[y0:y1, x0:x1]
        elif kind == "noise":
            l[y0:y1, x0:x1] = s["base"] + rng.integers(-amp, amp + 1, size=(y1 - y0, x1 - x0))
        else:                                # texture: 16x16 squares of +-amp on what is there (1/4 picture: 8x8, 1/16 picture: 4x4)
            l[y0:y1, x0:x1] += amp * (1 - 2 * (((x[:, x0:x1] >> 4) + (y[y0:y1] >> 4)) & 1))
    return np.clip(l, 0, 255).astype(np.uint8)


def checkerboard(w, h):
    return (255 * ((np.arange(w)[None, :] + np.arange(h)[:, None]) & 1)).astype(np.uint8)
