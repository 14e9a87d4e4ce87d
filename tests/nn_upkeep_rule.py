"""The schedule of the in-loop search's query-order rebuilds as the tests read it: a plain g++ build of csrc/fdc_forms.h
(tests/nn_upkeep_cpu/nn_upkeep.cpp) and the recurrence from periods to launch numbers.  Shared by tests/test_nn_upkeep_cpu.py, which
checks the rule, and tests/test_gpu_nn_upkeep.py, which holds the library's own rebuild count against it.

How a period becomes launch numbers (fdc_chamfer.h nn_stream_upkeep; launch 1 is the fit's seeding launch): rebuild 1 follows
launch 1; the launch after a rebuild records the new groups' work and is followed by the launch-order sort, which starts the count;
so rebuild r + 1 follows launch  L(r) + 1 + nn_order_period(base, r, nq)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "nn_upkeep_cpu", "nn_upkeep.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")


def build_exe(growth):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "nn_upkeep" if growth else "nn_upkeep_fixed")
    deps = [SRC, os.path.join(CSRC, "fdc_forms.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        flags = [] if growth else ["-DFDC_NN_PERIOD_GROWTH=0"]
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", exe, SRC])
    return exe


NQ = 512_000                                                # (a size the growing period is taken at: bench config 3's queries)


def periods(exe, base, counts, nq=NQ):
    args = [str(v) for r in counts for v in (base, r)]
    out = subprocess.run([exe, "period", str(nq), *args], check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == len(counts)
    return [int(x) for x in out]


def rebuild_launches(exe, base, how_many, nq=NQ):
    """the search launches (1-based; 1 seeds the fit) that the first `how_many` rebuilds follow"""
    at = [1]
    per = periods(exe, base, list(range(1, how_many)), nq)
    for p in per:
        at.append(at[-1] + 1 + p)
    return at


def rebuilds_within(exe, base, launches, nq=NQ):
    """rebuilds of a fit of `launches` search launches over nq queries"""
    if base <= 0 or launches < 1:
        return 0
    n = 1
    while True:
        at = rebuild_launches(exe, base, n + 1, nq)
        if at[-1] > launches:
            return n
        n += 1
