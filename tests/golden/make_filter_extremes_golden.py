#!/usr/bin/env python3
"""Record what the REFERENCE's own in-loop filter leaves compute at the ends of their ranges: the seeded inputs of tests/filter_extremes.py go through the
exported C symbols of oracle/_ref/libsvtref.so (GatherSaoStatisticsLcuLossy_62x62, GatherSaoStatisticsLcu_62x62_16bit and the two OnlyEo forms;
SAOApplyBO[16bit], SAOApplyEO_0 / _90 / _135 / _45[_16bit]; Luma4SampleEdgeDLFCore[16bit], Chroma2SampleEdgeDLFCore[16bit]) - the symbols
tests/test_oracle_loopfilter.py calls.  Only the results are stored; the inputs are rebuilt from the seeds.
  -> tests/golden/filterx_gather.npz  g1 / g2: statistics [case][only_eo] of the 8- / 10-bit gather cases
     tests/golden/filterx_apply.npz   a1 / a2: the filtered areas of every (plane, operation), one after the other
     tests/golden/filterx_dlf.npz     l1 / l2, c1 / c2: the 8 x 4 (luma) and 4 x 2 (Cb, Cr) samples around the edge of every deblocking case
The files are written with fixed time stamps: running the script again gives the same bytes.  Needs `make -C oracle ref`.
Usage: python tests/golden/make_filter_extremes_golden.py"""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import filter_extremes as X  # noqa: E402
import svtlib as S  # noqa: E402


def save(path, **arrays):
    """an .npz whose bytes depend on the arrays alone"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


def main():
    ref = S.load_ref()
    if ref is None:
        sys.exit("oracle/_ref/libsvtref.so missing: run `make -C oracle ref`")
    impl = X.Leaves(ref)
    save(os.path.join(S.GOLDEN_DIR, "filterx_gather.npz"), g1=X.run_gather(impl, 1), g2=X.run_gather(impl, 2))
    save(os.path.join(S.GOLDEN_DIR, "filterx_apply.npz"), a1=X.run_apply(impl, 1), a2=X.run_apply(impl, 2))
    l1, c1 = X.run_dlf(impl, 1)
    l2, c2 = X.run_dlf(impl, 2)
    save(os.path.join(S.GOLDEN_DIR, "filterx_dlf.npz"), l1=l1, c1=c1, l2=l2, c2=c2)


if __name__ == "__main__":
    main()
