"""The clip of the pictures coded without sub-sample search (tests/golden/make_md_ifree_golden.py, tests/test_gpu_e2e_ifree.py): 2688x1024 reaches the reference's 4K input
class (luma area >= INPUT_SIZE_4K_TH 0x29F630), where encMode 9 sets useSubpelFlag = (temporalLayerIndex == 0).  Flat luma 110 and chroma 128 with 18 squares of 128x128
samples, each a sum of three sinusoids in luma and in both chroma planes, each moving by a multiple of a quarter sample a picture: the motion fields hold fractional vectors
(through the temporal candidate and the neighbours), the chroma planes are not flat (the nearest-sample chroma prediction differs from the 4-tap filter's), and the flat
background keeps a recorded picture below 1 MiB (bzip2 members)."""
import numpy as np

WIDTH, HEIGHT, FRAMES, SEED = 2688, 1024, 9, 5
ENC_ARGS = ["-encMode", "9", "-pred-struct", "2", "-hierarchical-levels", "2", "-q", "34"]
SQUARES, SIDE = 18, 128


def frames(w=WIDTH, h=HEIGHT, n=FRAMES, seed=SEED):
    """yields (Y, Cb, Cr) uint8 planes of picture 0 .. n - 1"""
    rng = np.random.default_rng(seed)
    K = SQUARES
    x0, y0 = rng.integers(40, w - 200, K), rng.integers(40, h - 200, K)
    vx, vy = rng.integers(-9, 10, K) / 4.0, rng.integers(-5, 6, K) / 4.0
    fx, fy, ph = rng.uniform(0.05, 0.45, (K, 3)), rng.uniform(0.05, 0.45, (K, 3)), rng.uniform(0, 6.28, (K, 3))
    cfx, cfy, cph = rng.uniform(0.1, 0.6, (K, 2, 3)), rng.uniform(0.1, 0.6, (K, 2, 3)), rng.uniform(0, 6.28, (K, 2, 3))
    yy, xx = np.mgrid[0:SIDE, 0:SIDE].astype(np.float64)
    cy, cx = np.mgrid[0:SIDE // 2, 0:SIDE // 2].astype(np.float64)
    for t in range(n):
        Y = np.full((h, w), 110.0)
        C = [np.full((h // 2, w // 2), 128.0), np.full((h // 2, w // 2), 128.0)]
        for k in range(K):
            px, py = x0[k] + vx[k] * t, y0[k] + vy[k] * t
            ix, iy = int(np.floor(px)), int(np.floor(py))
            dx, dy = px - ix, py - iy
            Y[iy:iy + SIDE, ix:ix + SIDE] = 128 + 35 * sum(np.sin(fx[k, j] * (xx - dx) + fy[k, j] * (yy - dy) + ph[k, j]) for j in range(3))
            jx, jy = ix >> 1, iy >> 1
            ex, ey = px / 2 - jx, py / 2 - jy
            for p in range(2):
                C[p][jy:jy + SIDE // 2, jx:jx + SIDE // 2] = 128 + 30 * sum(np.sin(cfx[k, p, j] * (cx - ex) + cfy[k, p, j] * (cy - ey) + cph[k, p, j]) for j in range(3))
        yield tuple(np.clip(np.rint(a), 0, 255).astype(np.uint8) for a in (Y, C[0], C[1]))


def write_clip(path, w=WIDTH, h=HEIGHT, n=FRAMES, seed=SEED):
    with open(path, "wb") as f:
        for planes in frames(w, h, n, seed):
            for a in planes:
                f.write(a.tobytes())
