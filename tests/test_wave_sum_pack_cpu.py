"""The packed wave sums of csrc/fdc_math.h (wave_sum64_pack_w: up to sixteen values reduced over the 64 lanes at once, four values
to a quad and sixteen to a row from the steps at which wave_sum64's lanes start to hold copies) must give wave_sum64's bits per value.
Checked without a GPU on the header's sixty-four-lane model of the DPP moves, through a stand-alone program
(tests/wave_sum_pack_cpu/wave_sum_pack.cpp, its own main) built with -fsanitize=address,undefined; the inputs are
tests/wave_sum_cases.py's, which the GPU test runs on the device as well."""
import os
import subprocess

import numpy as np
import pytest

from tests import wave_sum_cases as wsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "wave_sum_pack_cpu", "wave_sum_pack.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "wave_sum_pack")


@pytest.fixture(scope="module")
def results():
    """{(kind, N): (input, packed, wave_sum64, mutant)} as uint32 bit patterns, one run of the program for all cases"""
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(CSRC, "fdc_math.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", CSRC, "-o", EXE, SRC])
    cases = wsc.all_cases()
    text = "".join(f"{n}\n" + " ".join(f"{w:x}" for w in v.view(np.uint32).ravel()) + "\n" for _, n, v in cases)
    p = subprocess.run([EXE], input=text, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert len(lines) == 3 * len(cases)
    out = {}
    for c, (kind, n, v) in enumerate(cases):
        rows = [np.array([int(t, 16) for t in lines[3 * c + k].split()], dtype=np.uint32) for k in range(3)]
        assert all(len(r) == n for r in rows)
        out[kind, n] = (v, *rows)
    return out


@pytest.mark.parametrize("n", wsc.NS)
@pytest.mark.parametrize("kind", wsc.KINDS)
def test_packed_tree_gives_wave_sum64s_bits(results, kind, n):
    v, packed, ref, _ = results[kind, n]
    assert packed.tolist() == ref.tolist()
    # ... and both are the tree as numpy states it (pairs, quads, octets, rows, ((r0 + r1) + r2) + r3)
    want = np.array([wsc.tree_sum(v[:, i]) for i in range(n)], dtype=np.float32).view(np.uint32)
    assert ref.tolist() == want.tolist()


def test_the_inputs_contain_what_they_claim():
    for n in wsc.NS:
        assert np.isnan(wsc.case("naninf", n)).any() and np.isinf(wsc.case("naninf", n)).any()
        z = wsc.case("zeros", n)
        assert np.signbit(z[z == 0]).any() and (n == 1 or (~np.signbit(z[z == 0])).any())
        assert (np.abs(wsc.case("huge", n)) >= 2.0 ** 40).sum() == 4 * n
        s = np.abs(wsc.case("spread", n))
        assert s.min() >= 2.0 ** -20.01 and s.max() <= 2.0 ** 20.01


def test_a_reassociated_tree_shows_on_these_inputs(results):
    """rows added pairwise, (r0 + r1) + (r2 + r3): the mutant must differ from wave_sum64 somewhere, or the inputs are blunt"""
    differ = {k: int((m != r).sum()) for k, (_, _, r, m) in results.items()}
    assert sum(differ.values()) > 0, differ
    # sharp at the sizes the kernels use, not by one lucky value (a single sum survives a reassociation about every other time, so
    # N = 1 and 3 are left to the total)
    for n in (12, 16):
        assert sum(c for (kind, nn), c in differ.items() if nn == n and kind in ("spread", "huge", "cancel")) > 0, (n, differ)
