#!/usr/bin/env python3
"""Record what the REFERENCE's own GenerateL0L1AmvpMergeLists and ChooseMVPIdx_V2 answer on the seeded single-unit jobs of tests/mvlists_jobs.py
(oracle/ref_harness_mvlists.c: svt_ref_mv_lists in oracle/_ref/libsvtref.so).
  -> tests/golden/mvlists_seeded.npz  jobs (SvtAmdMdListJob), pool (the SvtAmdTmvpLcu records the jobs index), outs (SvtAmdMdListOut: the reference's)
The file is written with fixed time stamps: running the script again gives the same bytes.  Prints the coverage counts tests/test_oracle_mvlists.py asserts.
Needs `make -C oracle ref`.
Usage: python tests/golden/make_mvlists_golden.py"""
import io
import os
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvlists_jobs as J  # noqa: E402
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
    pool = J.make_pool(J.POOL_SEED)
    jobs = J.make_jobs(J.SEED, J.COUNT, pool)
    outs = J.run_lists(ref.svt_ref_mv_lists, jobs, pool, returns=True)
    save(os.path.join(S.GOLDEN_DIR, "mvlists_seeded.npz"), jobs=jobs, pool=pool, outs=outs)
    model, flags = J.model_out_array(jobs, pool)
    J.compare_outs(jobs, model, outs, "the counting model against the reference")
    counts = J.coverage(jobs, flags)
    for c in J.CONDITIONS:
        print("%-60s %5d%s" % (c, counts[c], "" if counts[c] >= J.CONDITIONS[c] else "   BELOW %d" % J.CONDITIONS[c]))


if __name__ == "__main__":
    main()
