"""Seeded pictures of the picture-detector tests (svt_amd_chroma_stats_batch_launch / svt_amd_picture_detect_batch_launch): what svtlib.gen_luma does not
make - 4:2:0 chroma planes with content, and the "islands" picture whose LCUs trigger the edge / intensity detectors of EdgeDetection
(Codec/EbPictureAnalysisProcess.c:3627).  tests/golden/make_pa_detect_golden.py and the GPU tests build their inputs here, so both see the same samples."""
import numpy as np

import svtlib as S

ISLANDS_BRIGHT = ((5, 5), (6, 4))      # (LCU column, LCU row) of the two bright LCUs of the recorded "islands" picture
ISLANDS_STEP = (2, 2)                  # the LCU with the half-LCU step edge


def islands(w, h, seed, bright=ISLANDS_BRIGHT, step=ISLANDS_STEP):
    """a dark, mildly noisy background (mean ~60 < 120), bright LCUs (mean ~215 > 180) and one LCU whose left half is 20 and right half 230: a 64x64 variance
    far above 200 with all sixteen 16x16 variances 0 (sharpEdgeLcuFlag).  Bright LCUs inside the +-4 margin trigger the 9x9 marks of isolatedHighIntensityLcu."""
    rng = np.random.default_rng(seed)
    l = 56 + rng.integers(0, 9, size=(h, w))
    for bx, by in bright:
        l[64 * by:64 * by + 64, 64 * bx:64 * bx + 64] = 208 + rng.integers(0, 16, size=(64, 64))
    if step is not None:
        sx, sy = step
        l[64 * sy:64 * sy + 64, 64 * sx:64 * sx + 32] = 20
        l[64 * sy:64 * sy + 64, 64 * sx + 32:64 * sx + 64] = 230
    return l.astype(np.uint8)


def gen_luma(kind, w, h, t, seed):
    return islands(w, h, seed + t) if kind == "islands" else S.gen_luma(kind, w, h, t, seed)


def gen_chroma(kind, w, h, t, seed):
    """(Cb, Cr) of a 4:2:0 picture, (h / 2, w / 2) each: slow waves, a few flat rectangles (gradients between neighbouring 16x16 means) and noise"""
    rng = np.random.default_rng(seed * 7919 + 31 * t + len(kind))
    cw, ch = w // 2, h // 2
    x = np.arange(cw)[None, :]
    y = np.arange(ch)[:, None]
    cb = 128 + 50 * np.sin((x + 2 * t) / 19.0) * np.cos(y / 13.0) + rng.integers(-6, 7, size=(ch, cw))
    cr = 128 + 45 * np.cos((x - y + t) / 23.0) + rng.integers(-9, 10, size=(ch, cw))
    for _ in range(4 + (cw * ch) // 8192):
        rw, rh = int(rng.integers(6, 41)), int(rng.integers(6, 41))
        x0, y0 = int(rng.integers(0, cw)), int(rng.integers(0, ch))
        cb[y0:y0 + rh, x0:x0 + rw] = int(rng.integers(0, 256))
        cr[y0:y0 + rh, x0:x0 + rw] = int(rng.integers(0, 256))
    return np.clip(np.floor(cb), 0, 255).astype(np.uint8), np.clip(np.floor(cr), 0, 255).astype(np.uint8)


def padded(luma, pad=64):
    """the encoder's padded input picture (edges replicated): the block statistics of partial LCUs read it"""
    return np.ascontiguousarray(np.pad(luma, ((0, pad), (0, pad)), mode="edge"))


def resolution_class(w, h):
    """SequenceControlSet_t.inputResolution (DeriveInputResolution, Codec/EbSequenceControlSet.c:288-300)"""
    size = w * h
    return 0 if size < 0xB71B0 else 1 if size < 0x1AB3F0 else 2 if size < 0x29F630 else 3
