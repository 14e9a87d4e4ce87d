"""r21: which key the in-loop search's query order sorts by and how fine its work items are -- pure functions in csrc/fdc_forms.h
(nn_order_key_shift, plan_nn_items_per_chunk, nn_item_id / nn_item_chunk / nn_item_of), checked without a GPU through a stand-alone
program (tests/search_items_cpu/search_items.cpp, its own main) built with -fsanitize=address,undefined.

Key shift: the finest of 5 (32-point tile), 6, 7 (quarter) for which the scene's last key (ns - 1) >> shift stays below the
no-neighbour sentinel 0xFFFF.  Items: 8 per chunk while the 16-bit list ids 8 * chunk + item fit, only where the scene has the
eighths' boxes and only for launches of more than 2^21 queries, the size from which they were measured to win; 4 otherwise, and
wherever 4 is forced."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "search_items_cpu", "search_items.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "search_items")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(CSRC, "fdc_forms.h"), os.path.join(CSRC, "fdc_clips.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-I", CSRC, "-o", EXE, SRC])
    return EXE


def _run(exe, *args):
    p = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout, p.stderr[-2000:])
    return p.stdout.split()


NS = (1, 31, 32, 2_097_119, 2_097_120, 2_097_121, 4_194_304)


def _shift(ns):
    return next((s for s in (5, 6) if (ns - 1) >> s < 0xFFFF), 7)


def test_key_shift_is_the_finest_that_keeps_the_sentinel_free(exe):
    got = [int(x) for x in _run(exe, "shift", *NS)]
    assert got == [_shift(ns) for ns in NS] == [5, 5, 5, 5, 5, 6, 7]
    # the bench scenes, 500 k points (config 3) and 2 M points (config 5), both sort by tile; 64-point nodes from 2 097 121 points
    assert [int(x) for x in _run(exe, "shift", 500_000, 2_000_000, 4_194_240, 4_194_241, 0, 1 << 30)] == [5, 5, 6, 7, 5, 7]
    for ns, s in zip(NS, got):
        assert s == 7 or (ns - 1) >> s < 0xFFFF
        assert s == 5 or (ns - 1) >> (s - 1) >= 0xFFFF


NCHUNK = (1, 8191, 8192)
BIG = 5_363_200                                              # config 5's queries: above the size bound


def _ipc(exe, cases):
    return [int(x) for x in _run(exe, "ipc", *[v for c in cases for v in c])]


def test_eight_items_per_chunk_while_their_ids_fit_sixteen_bits(exe):
    assert _ipc(exe, [(BIG, n, 1, 0) for n in NCHUNK]) == [8, 8, 4]
    assert 8 * 8191 + 7 <= 0xFFFF < 8 * 8192 + 7
    for forced, want in ((4, [4, 4, 4]), (8, [8, 8, 4])):                   # 8 asked for where the ids do not fit: still 4
        assert _ipc(exe, [(BIG, n, 1, forced) for n in NCHUNK]) == want
    assert _ipc(exe, [(BIG, n, 0, 8) for n in NCHUNK]) == [4, 4, 4]          # no boxes of eighths


def test_eight_items_only_above_the_measured_size(exe):
    # quarters up to 2^21 queries (measured to win at 512 k, 1.02 M and 2.05 M), eighths above (4.1 M, config 5's 5.36 M)
    sizes = (1, 512_000, 1_024_000, 2_048_000, 1 << 21, (1 << 21) + 1, 4_096_000, BIG)
    assert _ipc(exe, [(nq, 977, 1, 0) for nq in sizes]) == [4, 4, 4, 4, 4, 8, 8, 8]
    assert _ipc(exe, [(nq, 977, 1, 8) for nq in sizes]) == [8] * len(sizes)       # the seam's 8 holds at every size ...
    assert _ipc(exe, [(nq, 977, 1, 4) for nq in sizes]) == [4] * len(sizes)       # ... and its 4


@pytest.mark.parametrize("ipc,nchunk", [(8, 1), (8, 8191), (4, 1), (4, 8192), (4, 16384)])
def test_item_ids_pack_and_unpack_through_sixteen_bits(exe, ipc, nchunk):
    largest, ok = _run(exe, "ids", ipc, nchunk)
    assert ok == "ok" and int(largest) == ipc * nchunk - 1 <= 0xFFFF
