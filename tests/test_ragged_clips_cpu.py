"""Clips of different lengths in one batch, the parts that need no GPU: the batch planner of `--clips --mix-lengths`
(cli.plan_batches_mixed), the host-built clip table (csrc/fdc_clips.h, compiled by plain g++) against numpy float32 evaluations of
the weights' expressions, the kernel forms of the lengths tests/test_gpu_ragged_clips.py fits, and the CLI's argument check."""
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
cli = importlib.import_module("fdcap_amd.cli")

f32 = np.float32


# ---- the planner ---------------------------------------------------------------------------------------------------
def test_remainder_clips_ride_under_the_row_cap():
    clips = [("a", 300), ("a", 300), ("a", 300), ("a", 124), ("a", 300), ("a", 300), ("a", 101), ("a", 7)]
    assert cli.plan_batches_mixed(clips) == [("a", [0, 1, 2, 3]), ("a", [4, 5, 6, 7])]
    # one row more than fits closes the batch: input order is kept, nothing is reordered to fill a batch
    assert cli.plan_batches_mixed([("a", 300), ("a", 300), ("a", 300), ("a", 125), ("a", 100)]) == [("a", [0, 1, 2]), ("a", [3, 4])]
    assert cli.plan_batches_mixed([("a", 600), ("a", 424), ("a", 1)], row_cap=1024) == [("a", [0, 1]), ("a", [2])]
    assert cli.plan_batches_mixed([]) == []


def test_a_clip_above_the_cap_is_a_batch_of_its_own():
    clips = [("a", 100), ("a", 2000), ("a", 50), ("a", 1025), ("a", 1024)]
    assert cli.plan_batches_mixed(clips) == [("a", [0]), ("a", [1]), ("a", [2]), ("a", [3]), ("a", [4])]
    assert cli.plan_batches_mixed([("a", 30), ("a", 30)], row_cap=10) == [("a", [0]), ("a", [1])]


def test_scenes_are_kept_apart_in_order_of_first_appearance():
    clips = [("b", 300), ("a", 124), ("b", 40), ("a", 300), ("c", 9)]
    assert cli.plan_batches_mixed(clips) == [("b", [0, 2]), ("a", [1, 3]), ("c", [4])]


def test_clips_per_batch_is_honoured_next_to_the_cap():
    clips = [("a", 24), ("a", 17), ("a", 24), ("a", 9), ("a", 1000), ("a", 20), ("a", 20)]
    assert cli.plan_batches_mixed(clips, 3) == [("a", [0, 1, 2]), ("a", [3, 4]), ("a", [5, 6])]
    assert cli.plan_batches_mixed(clips, 1) == [("a", [i]) for i in range(7)]
    assert cli.plan_batches_mixed(clips, 100) == [("a", [0, 1, 2, 3]), ("a", [4, 5]), ("a", [6])]


@pytest.mark.parametrize("n,count,k", [(300, 7, None), (40, 30, None), (40, 30, 4), (1024, 3, None), (1500, 3, None), (300, 7, 2), (512, 5, None)])
def test_one_length_gives_the_batches_of_plan_batches(n, count, k):
    clips = [("a" if i % 3 else "b", n) for i in range(count)]
    want = [(scene, idx) for scene, _, idx in cli.plan_batches(clips, k)]
    assert cli.plan_batches_mixed(clips, k) == want


# ---- the host-built clip table ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "clip_table")
    src = os.path.join(ROOT, "tests", "ragged_cpu", "clip_table.cpp")
    deps = [src, os.path.join(CSRC, "fdc_clips.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", out, src])
    return out


def _bits(x):
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


def _table(exe, lw, w_rec, w_contact, nc, lens, want=None, max_rows=1 << 24):
    rec, smooth, contact, world, world_on = lw
    args = [_bits(rec), _bits(smooth), _bits(contact), _bits(world), int(world_on), _bits(w_rec), _bits(w_contact), nc,
            sum(lens) if want is None else want, max_rows, *lens]
    lines = subprocess.run([exe, *map(str, args)], check=True, capture_output=True, text=True).stdout.splitlines()
    out = {"ok": lines[0] == "ok 1", "w": [], "rows": []}
    for ln in lines[1:]:
        tok = ln.split()
        if tok[0] == "equal":
            out["equal"] = tok[1] == "1"
        elif tok[0] == "starts":
            out["starts"] = [int(t) for t in tok[1:]]
        elif tok[0] == "w":
            out["w"].append(tuple(int(t) for t in tok[2:]))
        elif tok[0] == "row":
            out["rows"].append(tuple(int(t) for t in tok[1:]))
    return out


def _weights(n, lw, w_rec, w_contact, nc):
    """The four expressions of opt_backward_impl, in numpy float32 (every product, sum and quotient rounded to fp32)."""
    rec, smooth, contact, world, world_on = (f32(lw[0]), f32(lw[1]), f32(lw[2]), f32(lw[3]), lw[4])
    XDIM, NJW = f32(78), f32(23)
    wr = rec * f32(w_rec) / (f32(n) * XDIM)
    ws = smooth / (f32(n - 2) * XDIM) if n >= 3 else f32(0)
    ww = world / (f32(n - 1) * NJW * f32(3)) if (world_on and n >= 2) else f32(0)
    co = contact * f32(w_contact) / (f32(n) * f32(nc))
    return tuple(_bits(v) for v in (wr, ws, ww, co))


LENS = (1, 2, 3, 40, 300)
# mode 'global' (fitting.py: PHASE1_CONTACT / PHASE1_SMOOTH / PHASE2_WORLD / PHASE2_SMOOTH), and a set of odd values
PHASES = {"phase 1": (1.0, 1.0, 0.1, 0.0, False), "phase 2": (1.0, 0.5, 0.0, 1.0, True), "odd": (0.7, 0.3, 0.013, 1.7, True)}


@pytest.mark.parametrize("phase", list(PHASES))
def test_the_clip_table_equals_the_float32_expressions_bit_for_bit(exe, phase):
    lw = PHASES[phase]
    w_rec, w_contact, nc = (1.0, 0.1, 500) if phase != "odd" else (0.9, 0.37, 48)
    t = _table(exe, lw, w_rec, w_contact, nc, LENS)
    assert t["ok"] and not t["equal"]
    assert t["starts"] == [0, 1, 3, 6, 46, 346]
    want_w = [_weights(n, lw, w_rec, w_contact, nc) for n in LENS]
    assert t["w"] == want_w
    zero = _bits(0.0)
    # the zeros: no second difference below three frames, no first difference below two (and none while the world term is off)
    assert [w[1] == zero for w in want_w] == [True, True, False, False, False]
    assert [w[2] == zero for w in want_w] == ([True] * 5 if not lw[4] else [True, False, False, False, False])
    rows = t["rows"]
    assert len(rows) == sum(LENS) + 4 and [r[0] for r in rows] == list(range(len(rows)))
    r = 2
    for k, n in enumerate(LENS):
        for g in range(n):
            assert rows[r] == (r, k, g, n, *want_w[k]), (k, g)
            r += 1
    # halo rows: a valid clip index for `scale`, no frames, zero weights
    assert rows[0][1:] == rows[1][1:] == (0, 0, 0, zero, zero, zero, zero)
    assert rows[-1][1:] == rows[-2][1:] == (len(LENS) - 1, 0, 0, zero, zero, zero, zero)


def test_lengths_are_checked(exe):
    lw = PHASES["phase 1"]
    assert _table(exe, lw, 1.0, 0.1, 48, (40, 33, 24))["ok"]
    assert _table(exe, lw, 1.0, 0.1, 48, (40, 40, 40))["equal"]
    assert not _table(exe, lw, 1.0, 0.1, 48, (40, 0, 24), want=64)["ok"]
    assert not _table(exe, lw, 1.0, 0.1, 48, (40, -1, 24), want=63)["ok"]
    assert not _table(exe, lw, 1.0, 0.1, 48, (40, 33, 24), want=96)["ok"]
    assert not _table(exe, lw, 1.0, 0.1, 48, (), want=0)["ok"]
    assert not _table(exe, lw, 1.0, 0.1, 48, (600, 600), max_rows=1024)["ok"]
    assert _table(exe, lw, 1.0, 0.1, 48, (600, 424), max_rows=1024)["ok"]


# ---- the forms of the lengths the GPU tests fit -----------------------------------------------------------------------------
def test_the_gpu_tests_lengths_select_one_set_of_forms():
    """tests/test_gpu_ragged_clips.py asserts bit equality between a batch and its clips' stand-alone fits, which holds under equal
    kernel forms: 48 contact vertices, 4 weights each, a 9000-point scene -- the batch's 107 rows and every clip's rows must plan
    alike (and 9 rows must not: why the shortest clip there has 10 frames)."""
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
        for q in (f"cfwd:{rows}:48:4:55", f"pfwd:{rows}:48", f"bwd:{rows}:48:1", f"skin:{rows}:48:4", f"nn:{rows}:48:9000"):
            (line,) = subprocess.run([forms_exe, "@" + q], check=True, capture_output=True, text=True, env=env).stdout.splitlines()
            plan = line.split("\t")[1]
            out.append(plan.split(" block=")[0])
        return out

    batch = forms(40 + 33 + 24 + 10)
    for rows in (40, 33, 24, 10, 20, 97, 93, 43, 120):
        assert forms(rows) == batch, rows
    assert forms(9) != batch and forms(3) != batch
    # the short batch (1, 2, 3, 3): 9 rows and every clip's rows plan alike too, nn_direct_kernel included
    short = forms(1 + 2 + 3 + 3)
    for rows in (1, 2, 3):
        assert forms(rows) == short, rows


# ---- the CLI's argument check -------------------------------------------------------------------------------------------
def test_mix_lengths_without_clips_is_an_argparse_error(capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["body/", "fit/", "global", "--mix-lengths"])
    assert e.value.code == 2
    assert "--mix-lengths belongs to the multi-clip form" in capsys.readouterr().err     # (the new check, not argparse's unknown-flag error)
