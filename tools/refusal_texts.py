#!/usr/bin/env python3
"""The error text of every refusal the GPU tests of the records batches provoke (test_refused_batches_... of test_gpu_source_ops.py, test_gpu_mdc_batch.py,
test_gpu_irc_batch.py, test_gpu_mdctl_batch.py and test_gpu_pa_detect.py), one line each in the order of the tests: run it with SVT_PRODUCT_LIB at two builds and
diff the outputs to see that a change of the host half kept every text.  The tests run as they are; only pa_batch_util.refused also writes what it checked.
usage: refusal_texts.py output.txt"""
import os
import sys

import pytest

TESTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
sys.path.insert(0, TESTS)
import pa_batch_util as U       # noqa: E402

FILES = ("test_gpu_source_ops.py", "test_gpu_mdc_batch.py", "test_gpu_irc_batch.py", "test_gpu_mdctl_batch.py", "test_gpu_pa_detect.py")


def main():
    check = U.refused
    with open(sys.argv[1], "w") as out:
        def refused(lib, rc, entry, what=None):
            check(lib, rc, entry, what)
            out.write(lib.svt_amd_last_error().decode() + "\n")
        U.refused = refused     # before the test modules import it
        return pytest.main(["-q", "-p", "no:cacheprovider", "-k", "test_refused_batches"] + [os.path.join(TESTS, f) for f in FILES])


if __name__ == "__main__":
    sys.exit(main())
