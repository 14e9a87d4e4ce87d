"""Mode 'dct' for a batch of clips, the parts that need no GPU: the window table, the per-clip objective weights and the second
phase's record set of the clip table (csrc/fdc_clips.h, compiled by plain g++) against numpy float32 evaluations of the expressions
a stand-alone fit evaluates (fdcap_opt_dct_fit, fdcap_opt_backward_dct)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")

f32 = np.float32
T = 60


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "dct_table")
    src = os.path.join(ROOT, "tests", "dct_cpu", "dct_table.cpp")
    deps = [src, os.path.join(CSRC, "fdc_clips.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-o", out, src])
    return out


def _bits(x):
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


def _table(exe, lens, weight=10.0, w_rec=0.5, w_contact=0.1, weight_loss_rec=1.0, weight_contact=0.1, nc=16, t=T):
    args = [str(t)] + [str(_bits(v)) for v in (weight, w_rec, w_contact, weight_loss_rec, weight_contact)] + [str(nc)] + [str(n) for n in lens]
    lines = subprocess.run([exe, *args], check=True, capture_output=True, text=True).stdout.splitlines()
    out = {"start": [], "win": [], "wk": [], "row": []}
    for ln in lines:
        tok = ln.split()
        out[tok[0]].append(tuple(int(v) for v in tok[1:]))
    return out


def _want_windows(lens, t=T):
    """(buffer row of the first frame, clip, slot) of every window, clip after clip: clip k starts at buffer row 2 + n_0 + .. + n_{k-1}."""
    wins, starts, s = [], [0], 0
    for k, n in enumerate(lens):
        for w in range(n // t):
            wins.append((2 + s + w * t, k, len(wins)))
        starts.append(len(wins))
        s += n
    return wins, starts


@pytest.mark.parametrize("lens", [(150, 60, 125, 61), (61, 125, 60, 150), (300,), (120, 120, 120), (59, 60)])
def test_the_window_table_follows_each_clips_own_frames(exe, lens):
    t = _table(exe, lens)
    wins, starts = _want_windows(lens)
    assert [s[1] for s in t["start"]] == starts
    assert [w[1:] for w in t["win"]] == wins and [w[0] for w in t["win"]] == list(range(len(wins)))
    # every window lies inside its clip, and no frame of a clip's tail is in one
    off = np.concatenate([[0], np.cumsum(lens)])
    for row, k, slot in wins:
        assert 2 + off[k] <= row and row + T <= 2 + off[k] + (lens[k] // T) * T <= 2 + off[k + 1]


def test_tails_shift_the_rows_of_later_clips(exe):
    """(150, 60, 125, 61): the second clip's window starts at buffer row 2 + 150, not at 2 + 2 * 60 -- window number times T is wrong as
    soon as a clip before it has a tail."""
    wins = [w[1:] for w in _table(exe, (150, 60, 125, 61))["win"]]
    assert wins == [(2, 0, 0), (62, 0, 1), (152, 1, 2), (212, 2, 3), (272, 2, 4), (337, 3, 5)]
    assert [w[0] for w in wins] != [2 + 60 * i for i in range(6)]


@pytest.mark.parametrize("weight", [10.0, 1e-4, 0.7, 0.0])
def test_the_objective_weights_are_the_stand_alone_expression_bit_for_bit(exe, weight):
    lens = (150, 60, 125, 61, 300, 3840)
    t = _table(exe, lens, weight=weight)
    want = [_bits(f32(weight) / (f32(69) * f32(n // T))) for n in lens]
    assert [w[1] for w in t["wk"]] == want
    assert len(set(want)) == (1 if weight == 0.0 else 4)       # W = 2, 1, 2, 1, 5, 64


def test_a_clip_without_a_window_has_no_record_and_a_zero_weight(exe):
    t = _table(exe, (59, 60))
    assert [s[1] for s in t["start"]] == [0, 0, 1] and [w[1:] for w in t["win"]] == [(2 + 59, 1, 0)]
    assert t["wk"][0][1] == _bits(0.0) and t["wk"][1][1] == _bits(f32(10) / (f32(69) * f32(1)))


@pytest.mark.parametrize("weight_loss_rec,weight_contact,nc", [(1.0, 0.1, 16), (0.9, 0.3, 48)])
def test_the_second_phase_records_carry_its_weights_and_no_smoothing(exe, weight_loss_rec, weight_contact, nc):
    lens = (150, 60, 125, 61)
    t = _table(exe, lens, weight_loss_rec=weight_loss_rec, weight_contact=weight_contact, nc=nc)
    rows = t["row"]
    assert len(rows) == sum(lens) + 4 and [r[0] for r in rows] == list(range(len(rows)))
    zero = _bits(0.0)
    r = 2
    for k, n in enumerate(lens):
        # opt_backward_impl's expressions under lw = (rec 0.5, smooth 0, contact 0.1, world off): clip_weights with the clip's own n
        w_rec = f32(0.5) * f32(weight_loss_rec) / (f32(n) * f32(78))
        coef = f32(0.1) * f32(weight_contact) / (f32(n) * f32(nc))
        for g in range(n):
            assert rows[r] == (r, k, g, n, _bits(w_rec), zero, zero, _bits(coef)), (k, g)
            r += 1
    assert rows[0][1:] == rows[1][1:] == (0, 0, 0, zero, zero, zero, zero)
    assert rows[-1][1:] == rows[-2][1:] == (len(lens) - 1, 0, 0, zero, zero, zero, zero)
    # not phase 1's records: those carry a smoothing weight and the data term's multiplier 1
    assert rows[2][4] != _bits(f32(weight_loss_rec) / (f32(150) * f32(78)))
