"""Mode 'local''s second loop for a batch of clips, the parts that need no GPU: the per-clip weights and the second loop's record
set of the clip table (csrc/fdc_clips.h, compiled by plain g++) against numpy float32 evaluations of the expressions a stand-alone
fit evaluates (fdcap_opt_backward_local2, foot_skate_kernel), and the kernel forms of the lengths tests/test_gpu_multiclip_local.py
fits -- the full-mesh products included."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")

f32 = np.float32


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "local2_table")
    src = os.path.join(ROOT, "tests", "local2_cpu", "local2_table.cpp")
    deps = [src, os.path.join(CSRC, "fdc_clips.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", out, src])
    return out


def _bits(x):
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


def _table(exe, w_rec, nv3, npart, lens):
    lines = subprocess.run([exe, str(_bits(w_rec)), str(nv3), str(npart), *map(str, lens)], check=True, capture_output=True,
                           text=True).stdout.splitlines()
    out = {"w": [], "rows": []}
    for ln in lines:
        tok = ln.split()
        out["w" if tok[0] == "w" else "rows"].append(tuple(int(t) for t in tok[1 if tok[0] == "row" else 2:]))
    return out


def _weights(n, w_rec, nv3, npart):
    """fdcap_opt_backward_local2's three expressions and foot_skate_kernel's, in numpy float32 (every product and quotient rounded to
    fp32); the zeros below three and below two frames are what a stand-alone fit of that length uses (or never launches)."""
    XDIM = f32(78)
    wr = f32(w_rec) / (f32(n) * XDIM)
    ws = f32(1) / (f32(n - 2) * XDIM) if n >= 3 else f32(0)
    wv = f32(1) / (f32(n - 2) * f32(nv3)) if n >= 3 else f32(0)
    inv = f32(1) / (f32(n - 1) * f32(npart) * f32(3)) if n >= 2 else f32(0)
    return tuple(_bits(v) for v in (wr, ws, wv, f32(0), inv))


LENS = (1, 2, 3, 10, 300)


@pytest.mark.parametrize("w_rec,nv3,npart", [(1.0, 3 * 10475, 250), (0.9, 3 * 300, 24)])
def test_the_second_loops_weights_equal_the_float32_expressions_bit_for_bit(exe, w_rec, nv3, npart):
    t = _table(exe, w_rec, nv3, npart, LENS)
    want = [_weights(n, w_rec, nv3, npart) for n in LENS]
    assert t["w"] == want
    zero = _bits(0.0)
    # no second difference below three frames (both spaces), no first difference below two
    assert [w[1] == zero for w in want] == [w[2] == zero for w in want] == [True, True, False, False, False]
    assert [w[4] == zero for w in want] == [True, False, False, False, False]
    assert all(w[0] != zero for w in want)


def test_the_second_loops_weights_are_not_the_first_loops(exe):
    """phase1_smooth happens to be 1, phase 2's is 0.5: the second loop's parameter smoothing has no multiplier, its data term none
    but weight_loss_rec, and the vertex-space weight divides by 3 V, not by the 69 world-joint coordinates."""
    (w,) = _table(exe, 1.0, 900, 24, (40,))["w"]
    assert w[1] == _bits(f32(1) / (f32(38) * f32(78))) != _bits(f32(0.5) / (f32(38) * f32(78)))
    assert w[2] == _bits(f32(1) / (f32(38) * f32(900))) != _bits(f32(1) / (f32(39) * f32(69)))


def test_the_second_loops_records_know_clip_index_and_length(exe):
    lens, nv3 = (3, 1, 10), 900
    t = _table(exe, 1.0, nv3, 24, lens)
    rows = t["rows"]
    assert len(rows) == sum(lens) + 4 and [r[0] for r in rows] == list(range(len(rows)))
    r = 2
    for k, n in enumerate(lens):
        want = _weights(n, 1.0, nv3, 24)[:4]
        for g in range(n):
            assert rows[r] == (r, k, g, n, *want), (k, g)
            r += 1
    zero = _bits(0.0)
    # halo rows: a valid clip index for `scale`, no frames, zero weights
    assert rows[0][1:] == rows[1][1:] == (0, 0, 0, zero, zero, zero, zero)
    assert rows[-1][1:] == rows[-2][1:] == (len(lens) - 1, 0, 0, zero, zero, zero, zero)
    # the one-frame clip in the middle: every weight but the data term's is zero
    assert rows[5][1:4] == (1, 0, 1) and rows[5][5:] == (zero, zero, zero) and rows[5][4] != zero


def test_the_gpu_tests_lengths_select_one_set_of_forms():
    """tests/test_gpu_multiclip_local.py asserts bit equality between a batch and its clips' stand-alone mode-'local' fits, which
    holds under equal kernel forms: a 300-vertex body (the second loop's full-mesh blend product runs over rows + 4 buffer rows, its
    data gradient and skinning backward over the rows), 48 contact vertices with 4 weights each, a 9000-point scene."""
    forms_exe = os.path.join(BUILD, "forms_sweep")
    src_dir = os.path.join(ROOT, "tests", "forms_cpu")
    deps = [os.path.join(src_dir, "sweep.cpp"), os.path.join(src_dir, "sweep_driver.h"), os.path.join(CSRC, "fdc_forms.h")]
    if not os.path.exists(forms_exe) or any(os.path.getmtime(d) > os.path.getmtime(forms_exe) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-I", src_dir, "-o", forms_exe,
                               os.path.join(src_dir, "sweep.cpp")])
    env = {k: v for k, v in os.environ.items() if not k.startswith("FDCAP_")}

    def forms(rows):
        out = []
        for q in (f"cfwd:{rows}:48:4:55", f"pfwd:{rows}:48", f"bwd:{rows}:48:1", f"skin:{rows}:48:4", f"nn:{rows}:48:9000",
                  f"pfwd:{rows + 4}:300", f"bwd:{rows}:300:0", f"skinany:{rows}:300"):
            (line,) = subprocess.run([forms_exe, "@" + q], check=True, capture_output=True, text=True, env=env).stdout.splitlines()
            plan = line.split("\t")[1]
            out.append(plan.split(" block=")[0])
        return out

    for batch, clips in ((3 * 24, (24,)), (40 + 33 + 24 + 10, (40, 33, 24, 10)), (1 + 2 + 3 + 3, (1, 2, 3))):
        want = forms(batch)
        for rows in clips:
            assert forms(rows) == want, (batch, rows)
