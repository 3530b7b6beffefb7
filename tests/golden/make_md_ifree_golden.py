#!/usr/bin/env python3
"""Generate the fixtures of P / B pictures coded WITHOUT sub-sample search (useSubpelFlag 0: encMode 9 at the 4K input class, temporal layers above 0) from the REFERENCE.

Same recording as make_md_golden.py (its parse_dump and its record assembly, run_case), on the clip of tests/md_ifree_clip.py; each kept picture goes into a file of its
own, tests/golden/mdifree_<name>.npz, in make_md_golden.py's layout with ONE picture (the prefix is not md_: the suites that glob md_*.npz run the CPU checker, whose
prediction knows the filters only).  Kept: a layer-2 picture (non-reference, CHROMA_MODE_BEST LCUs) and a layer-1 picture (reference, CHROMA_MODE_FULL LCUs) whose
co-located picture is a P / B picture - behind an I picture every vector is whole.  Needs /root/reference.  Usage: make_md_ifree_golden.py
"""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svtlib as S  # noqa: E402
import make_md_golden as G  # noqa: E402
import md_ifree_clip as CLIP  # noqa: E402

KIND = "ifree_squares"
KEEP = {5: "b_squares_2688x1024_m9_l2", 6: "bref_squares_2688x1024_m9_l1"}  # picture number -> fixture name
MAX_BYTES = 1 << 20


def save_npz_bzip2(path, arrays):
    """an .npz whose members are bzip2-compressed: np.load reads it like any other, and the sample planes - flat ground, smooth textures - take two thirds of what
    np.savez_compressed's deflate needs (a committed file stays below 1 MiB)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_BZIP2, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_BZIP2, 9)


def fractional_units(out):
    """masks over (LCU, leaf) of one picture's records: tested inter units with a fractional vector component on a list they use, and which of them are bi-predicted"""
    t = (out["tested"] != 0) & (out["pred_mode"] == 1)
    mv = out["mv"].reshape(out["mv"].shape[:2] + (2, 2))
    fr = ((mv & 3) != 0).any(axis=-1)
    d = out["inter_dir"]
    frac = t & (((d != 1) & fr[..., 0]) | ((d != 0) & fr[..., 1]))
    return frac, frac & (d == 2)


def main():
    if not os.path.exists(S.REF_APP):
        sys.exit("oracle/_ref/SvtHevcEncApp_ref missing: run `make -C oracle ref` (needs /root/reference)")
    write_clip, golden_dir = S.write_clip, S.GOLDEN_DIR
    G.CASES[KIND] = (KIND, CLIP.WIDTH, CLIP.HEIGHT, CLIP.FRAMES, CLIP.SEED, CLIP.ENC_ARGS, sorted(KEEP))
    with tempfile.TemporaryDirectory() as td:
        S.write_clip = lambda path, kind, w, h, n, seed: CLIP.write_clip(path, w, h, n, seed) if kind == KIND else write_clip(path, kind, w, h, n, seed)
        S.GOLDEN_DIR = td
        try:
            G.run_case(KIND)
        finally:
            S.write_clip, S.GOLDEN_DIR = write_clip, golden_dir
        g = dict(np.load(os.path.join(td, "md_%s.npz" % KIND)))
    numbers = g["picture_number"].tolist()
    assert numbers == sorted(KEEP), numbers
    for k, p in enumerate(numbers):
        one = {f: (a if f in ("clip", "enc_args") else a[k:k + 1]) for f, a in g.items()}
        assert int(one["inter"][0]["use_subpel"]) == 0
        o = one["out"][0]
        frac, bi = fractional_units(o)
        merge = o["merge_flag"] == 1
        # (a fraction enters a B picture through the temporal merge candidate alone, which is bi-predicted there, and a neighbour hands it on with its direction: the
        # uni-predicted merge units of these pictures carry whole vectors, and go through the same rounding and the same copy)
        uni = (o["tested"] != 0) & (o["pred_mode"] == 1) & merge & (o["inter_dir"] != 2)
        counts = (int((o["tested"] != 0).sum()), int(frac.sum()), int(uni.sum()), int((frac & merge & bi).sum()))
        path = os.path.join(S.GOLDEN_DIR, "mdifree_%s.npz" % KEEP[p])
        save_npz_bzip2(path, one)
        print("picture %d (layer %d, reference %d) -> %s (%d bytes): tested units %d, with a fractional vector %d, uni-predicted merge units %d, bi-predicted merge units with a fractional vector %d" %
              ((p, int(one["pic"][0]["temporal_layer"]), int(one["pic"][0]["is_reference"]), os.path.basename(path), os.path.getsize(path)) + counts))
        assert os.path.getsize(path) <= MAX_BYTES, "fixture too large"
        assert counts[1] >= 300 and counts[2] >= 1 and counts[3] >= 20, "too few fractional units: change CLIP.SEED"


if __name__ == "__main__":
    main()
