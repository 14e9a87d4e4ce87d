"""The in-loop Chamfer search tests listed boxes against its 32 queries with 2, 4 or 8 lanes per box (fdc_chamfer.h nn_box_stage).
Which width a stage takes, and how a pass's ballot becomes the ordered list of kept entries, are pure functions in csrc/fdc_forms.h
(nn_box_lanes, nn_box_fold, nn_box_rank, nn_box_count).  Checked here without a GPU, through a plain g++ build of the header, against
a naive loop over the entries."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "box_lanes_cpu", "box_lanes.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "box_lanes")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(CSRC, "fdc_forms.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", EXE, SRC])
    return EXE


def _run(exe, *args, stdin=None):
    return subprocess.run([exe, *args], check=True, capture_output=True, text=True, input=stdin).stdout.splitlines()


COUNTS = [0, 1, 8, 9, 16, 17, 32, 33, 64, 65, 128]


def test_lanes_per_box_follow_the_count(exe):
    want = {0: 8, 1: 8, 8: 8, 9: 4, 16: 4, 17: 2, 32: 2, 33: 2, 64: 2, 65: 2, 128: 2}
    assert sorted(want) == COUNTS
    args = [str(v) for n in COUNTS for v in (n, 0)]
    assert [int(x) for x in _run(exe, "lanes", *args)] == [want[n] for n in COUNTS]
    # the widest form that serves the whole stage in one pass of 64 lanes; beyond 32 entries the pair form takes several
    for n in COUNTS:
        assert n * want[n] <= 64 or want[n] == 2


@pytest.mark.parametrize("forced", [2, 4, 8])
def test_a_forced_width_holds_at_every_count(exe, forced):
    args = [str(v) for n in COUNTS for v in (n, forced)]
    assert [int(x) for x in _run(exe, "lanes", *args)] == [forced] * len(COUNTS)


def test_values_that_are_no_width_mean_by_count(exe):
    for forced in (-1, 1, 3, 5, 6, 7, 9, 16):
        args = [str(v) for n in COUNTS for v in (n, forced)]
        assert _run(exe, "lanes", *args) == _run(exe, "lanes", *[str(v) for n in COUNTS for v in (n, 0)])


def _naive(mask, lpb):
    """entry e is kept iff one of its lpb lanes hit; the kept entries land in ascending entry order"""
    kept = [e for e in range(64 // lpb) if any((mask >> (lpb * e + k)) & 1 for k in range(lpb))]
    return kept, {e: at for at, e in enumerate(kept)}


@pytest.mark.parametrize("lpb", [2, 4, 8])
def test_fold_and_rank_against_a_loop_over_the_entries(exe, lpb):
    rng = random.Random(1500 + lpb)
    masks = [0, (1 << 64) - 1]
    masks += [rng.getrandbits(64) for _ in range(4000)]
    masks += [rng.getrandbits(64) & rng.getrandbits(64) & rng.getrandbits(64) for _ in range(3000)]      # sparse: most entries miss
    masks += [rng.getrandbits(64) | rng.getrandbits(64) | rng.getrandbits(64) for _ in range(1500)]      # dense
    masks += [1 << rng.randrange(64) for _ in range(1500)]                                               # a single lane
    assert len(masks) == 10_002
    out = _run(exe, "fold", stdin="".join(f"{lpb} {m:x}\n" for m in masks))
    assert len(out) == len(masks)
    for m, line in zip(masks, out):
        tok = line.split()
        folded, count = int(tok[0], 16), int(tok[1])
        got = {int(e): int(at) for e, at in (t.split(":") for t in tok[2:])}
        kept, where = _naive(m, lpb)
        assert folded == sum(1 << (lpb * e) for e in kept), f"{m:x}"
        assert count == len(kept), f"{m:x}"
        assert got == where, f"{m:x}"
        assert list(got) == kept                      # emitted in ascending entry order
