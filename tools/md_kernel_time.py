#!/usr/bin/env python3
"""Time of the mode-decision kernel of ONE recorded picture (svt_amd_debug_md_kernel_ms: the events around k_md_picture of the blocking call), median and spread of N
calls after two warm-up calls, on the library SVT_PRODUCT_LIB names (default: the tree's).  One process per library: an A/B of two builds alternates processes.
usage: md_kernel_time.py <fixture .npz under tests/golden, or a path> [calls = 21] [picture index = 0]   -> one JSON line"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import svtlib as S  # noqa: E402


def main():
    name = sys.argv[1]
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 21
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    path = name if os.path.exists(name) else os.path.join(S.GOLDEN_DIR, name)
    lib = S.load_product()
    import mdlaunchlib as M
    from test_gpu_mdctl_batch import _md_sig
    _md_sig(lib)
    M.declare(lib)
    g = np.load(path)
    w, h = int(g["pic"][k]["width"]), int(g["pic"][k]["height"])
    ctx = C.c_void_p()
    assert lib.svt_amd_context_create(0, w, (h + 7) & ~7, 2, C.byref(ctx)) == 0, lib.svt_amd_last_error()
    obj = M.Obj(lib, ctx, g, k)
    ms, wg, times = C.c_float(), C.c_int(), []
    for i in range(calls + 2):
        obj.blocking()
        assert lib.svt_amd_debug_md_kernel_ms(ctx, obj.pic, C.byref(ms), C.byref(wg)) == 0, lib.svt_amd_last_error()
        if i >= 2:
            times.append(float(ms.value))
    obj.free()
    lib.svt_amd_context_destroy(ctx)
    t = np.array(times)
    print(json.dumps({"library": os.environ.get("SVT_PRODUCT_LIB", "tree"), "fixture": os.path.basename(path), "picture": k, "lcus": int(len(g["lcu"][k])), "workgroups": wg.value,
                      "calls": calls, "median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4)}))


if __name__ == "__main__":
    main()
