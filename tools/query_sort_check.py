#!/usr/bin/env python3
"""The query order's sort at the real sizes: fdcap_debug_nn_query_sort on uniform neighbour positions in [0, scene points) against
numpy's stable argsort of the same keys, exact.  tools/query_sort_check.py [--repeat N] [nq ...]   (default: 512 000 = bench config 3
and 512 x 10 475 = config 5).  --repeat runs the sort N more times (for a kernel trace of the rebuild on its own)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fdcap_amd  # noqa: E402,F401
from fdcap_amd import capi, synth  # noqa: E402


def main():
    argv = sys.argv[1:]
    repeat = 0
    if argv and argv[0] == "--repeat":
        repeat, argv = int(argv[1]), argv[2:]
    sizes = [int(a) for a in argv] or [512000, 512 * 10475]
    ctx = capi.Context(synth.make_body_model(400, seed=0), synth.make_vposer(seed=1))
    bad = 0
    for nq in sizes:
        pos = np.random.default_rng(nq).integers(0, 500000, nq).astype(np.int32)
        key = np.minimum(pos >> 7, 0xFFFF)
        ref = np.argsort(key, kind="stable").astype(np.int32)
        groups = (nq + 31) // 32
        for _ in range(1 + repeat):
            hdr = np.arange(groups + 5, dtype=np.int32)
            perm = np.empty(nq, np.int32)
            capi.check(ctx.lib.fdcap_debug_nn_query_sort(ctx.handle, pos.ctypes.data_as(ctypes.c_void_p), nq, groups, len(hdr),
                                                         hdr.ctypes.data_as(ctypes.c_void_p), perm.ctypes.data_as(ctypes.c_void_p), None),
                       "fdcap_debug_nn_query_sort")
            ok = np.array_equal(perm, ref) and (hdr[:groups] == -1).all() and np.array_equal(hdr[groups:], np.arange(groups, groups + 5))
            bad += not ok
        print(f"nq {nq:8d}: {1 + repeat} sorts, " + ("all equal to numpy's stable argsort, headers as specified" if not bad else "MISMATCH"), flush=True)
    ctx.close()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
