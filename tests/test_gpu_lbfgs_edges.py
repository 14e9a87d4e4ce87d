"""The batched L-BFGS kernel (include/fdcap.h fdcap_lbfgs_*, csrc/fdc_lbfgs_advance.inc) against its plain twin, round by round.

tests/test_gpu_lbfgs.py compares end states with torch.optim.LBFGS on three families; this module pins what that cannot see: the
lane edges (a lane holds elements [lane] and [lane + 64]), unequal strides with NaN in the gradient's padding, every branch of the
line search and of the stopping rules, histories of 1, 2, 33 and 128 pairs with the ring turning, lr, max_eval, reset, mixed batches
and non-finite objectives.

THE HARNESS (tests/lbfgs_cases.py has the cases and the rule).  Each round the kernel's X is read, every problem's objective is
evaluated in float64 at those float32 points and rounded to float32 (scripted problems take their table's row), and the same f, g
go to the kernel and to three twins (tests/lbfgs_spec.py in float64, float32, float32 summed in reverse).  Up to the first round in
which the twins disagree among themselves, the kernel's directions and evaluations must equal the float64 twin's and its point must
stay within 32 x max(|x_f32 - x_f64|, 2^-24 max|x|) of the float64 twin's.  tests/test_lbfgs_spec_cpu.py shows on the CPU that the
twins agree to the end of every case here, and that every branch is reached; this module asserts the same of its own run (the
kernel leads here, and its points differ by rounding), so no problem is excused.  The public API reports no per-problem "active"
flag: n_active must equal the number of unfinished float64 twins in every round, and a problem the twin has finished must keep its
row and its stats bit for bit.

MEASURED on the MI355X: the worst |x_kernel - x_f64| / bar over all cases, problems and rounds is 0.28 (case concave65; 0.19
elsewhere), i.e. the kernel is at most 9 x as far from the float64 twin as the float32 twin is.  The margin of 32 is the project's
convention (tests/gradient_bars.py): neither tight nor absurdly loose, it is kept.

Non-finite objectives are held to properties, not to the twin: with -fno-honor-nans every comparison with a NaN is the compiler's
to decide."""
import ctypes

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi
from tests import lbfgs_cases as lc

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
CASES = lc.cases()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Handle:
    def __init__(self, n, dim, cfg):
        self.lib, self.h = capi.load_library(), ctypes.c_void_p()
        cf = capi.LbfgsConfig(dim, cfg["history"], cfg["max_iter"], cfg["max_eval"], cfg["max_steps"], cfg["max_ls"], cfg["lr"],
                              cfg["tolerance_grad"], cfg["tolerance_change"], cfg["ftol"], cfg["gtol"])
        capi.check(self.lib.fdcap_lbfgs_create(n, ctypes.byref(cf), ctypes.byref(self.h)), "fdcap_lbfgs_create")

    def reset(self):
        capi.check(self.lib.fdcap_lbfgs_reset(self.h, capi.current_stream()), "fdcap_lbfgs_reset")

    def close(self):
        self.lib.fdcap_lbfgs_destroy(self.h)


def _run(problems, cfg, x_pad=5, g_pad=2, follow=True, max_rounds=400, handle=None, null_active_rounds=None):
    """-> dict(x [rounds][n, dim], it / ev / loss [rounds][n], active [rounds], locks).  null_active_rounds = R: n_active_d is NULL and
    exactly R rounds are made (`active` is then empty)."""
    n, dim = len(problems), problems[0].dim
    xs, gs = dim + x_pad, dim + g_pad
    own = handle is None
    hd = handle or Handle(n, dim, cfg)
    lib = hd.lib
    X = torch.full((n, xs), SENTINEL, device="cuda")
    X[:, :dim] = torch.tensor(np.stack([p.x0 for p in problems]))
    active = torch.zeros(1, dtype=torch.int32, device="cuda")
    it, ev = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    loss = torch.zeros(n, device="cuda")
    out = dict(x=[], it=[], ev=[], loss=[], active=[], locks=[lc.Lockstep(p, cfg) for p in problems] if follow else None)
    try:
        for rnd in range(max_rounds if null_active_rounds is None else null_active_rounds):
            xc = X[:, :dim].cpu().numpy()
            fg = [p.evaluate(xc[i], rnd) for i, p in enumerate(problems)]
            F = torch.tensor(np.array([f for f, _ in fg], dtype=np.float32), device="cuda")
            Gh = np.full((n, gs), np.nan, dtype=np.float32)        # a read past dim poisons whatever it enters
            Gh[:, :dim] = np.stack([g for _, g in fg])
            G = torch.tensor(Gh, device="cuda")
            capi.check(lib.fdcap_lbfgs_advance(hd.h, capi.dptr(X), xs, capi.dptr(F), capi.dptr(G), gs,
                                               None if null_active_rounds is not None else capi.dptr(active), capi.current_stream()),
                       "fdcap_lbfgs_advance")
            capi.check(lib.fdcap_lbfgs_get_stats(hd.h, capi.dptr(it), capi.dptr(ev), capi.dptr(loss), capi.current_stream()), "fdcap_lbfgs_get_stats")
            Xh = X.cpu().numpy()
            assert np.all(Xh[:, dim:] == SENTINEL), "the kernel wrote outside its problem's columns"
            out["x"].append(Xh[:, :dim].copy()), out["it"].append(it.cpu().numpy()), out["ev"].append(ev.cpu().numpy())
            out["loss"].append(loss.cpu().numpy())
            if follow:
                for lock, (f, g) in zip(out["locks"], fg):
                    if not lock.all_done():
                        lock.feed(f, g)
            if null_active_rounds is None:
                out["active"].append(int(active.item()))
                if out["active"][-1] == 0:
                    break
        return out
    finally:
        if own:
            hd.close()


def _same_bits(a, b, i, j=None):
    """problem i of run a and problem j of run b: the same rows and stats in every round, bit for bit"""
    j = i if j is None else j
    assert len(a["x"]) >= 1 and len(b["x"]) >= 1
    for r in range(max(len(a["x"]), len(b["x"]))):
        ka, kb = min(r, len(a["x"]) - 1), min(r, len(b["x"]) - 1)      # (a finished problem keeps its last state)
        for key in ("x", "it", "ev", "loss"):
            assert np.array_equal(_bits(a[key][ka][i]), _bits(b[key][kb][j])), (key, r, i, j)


WORST = {}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_takes_the_twins_decisions_round_by_round(name):
    case = CASES[name]
    problems, cfg = case["problems"], case["cfg"]
    run = _run(problems, cfg, case["x_pad"], case["g_pad"])
    rounds = len(run["x"])
    assert run["active"][-1] == 0, f"{name}: still running after {rounds} rounds"
    worst, horizons = 0.0, []
    for i, lock in enumerate(run["locks"]):
        counts = [(int(run["it"][r][i]), int(run["ev"][r][i])) for r in range(rounds)]
        h, w = lc.compare(counts, [run["x"][r][i] for r in range(rounds)], lock, f"{name}[{i}]")
        t64 = lock.twins["f64"]
        # nothing excused: the twins agree to the end of this very run, and the ring has turned as often as the case is there for
        assert lock.all_done() and h == len(t64.rounds), f"{name}[{i}]: the twins disagree in round {h} of {len(t64.rounds)}"
        assert sum(1 for r, t in t64.tags if t == "ring_drop_oldest" and r < h) >= case["min_drops"], (name, i)
        # a problem the twin has finished keeps its row and stats bit for bit
        for r in range(h, rounds):
            for key in ("x", "it", "ev", "loss"):
                assert np.array_equal(_bits(run[key][r][i]), _bits(run[key][h - 1][i])), (name, i, key, r)
        worst = max(worst, w)
        horizons.append(h)
    # the branches this case is in the catalogue for were taken, by some problem, in this run
    for tag in (t for t, c in lc.CATALOGUE.items() if c == name):
        assert any(t == tag for lock in run["locks"] for _, t in lock.twins["f64"].tags), f"{name}: {tag} not reached"
    for r in range(rounds):
        assert run["active"][r] == sum(1 for lock in run["locks"] if len(lock.twins["f64"].rounds) > r and not lock.twins["f64"].rounds[r][2]), (name, r)
    assert rounds == max(horizons) == int(run["ev"][-1].max())
    for key in ("x", "loss"):
        assert all(np.all(np.isfinite(a)) for a in run[key]), (name, key)
    WORST[name] = worst
    print(f"{name}: {len(problems)} problems, {rounds} rounds, worst |x - x_f64| / bar = {worst:.4f} (so far, all cases: {max(WORST.values()):.4f})")


MIXED_CFG = dict(lc.BASE, max_iter=12, tolerance_grad=1e-3)


def test_a_mixed_batch_of_70_equals_70_batches_of_one():
    """a flat problem (done in its first round), quick finishers and slow ones in one launch: a finished problem's row stays put,
    the batch takes as many rounds as its slowest problem has evaluations, and nobody sees its neighbours"""
    problems = [lc.Flat(40)] + [lc.Quadratic(40, 3.0 if s % 3 else 300.0, 7000 + s) for s in range(69)]
    run = _run(problems, MIXED_CFG, follow=False)
    rounds = len(run["x"])
    assert run["active"][-1] == 0 and rounds == int(run["ev"][-1].max())
    assert run["it"][0][0] == 0 and run["ev"][0][0] == 1 and run["loss"][0][0] == 1.5 and np.array_equal(run["x"][0][0], problems[0].x0)
    assert run["active"][0] == 69
    last = run["ev"][-1]
    assert len(set(last.tolist())) > 3, "no mix of quick and slow problems"
    for i in range(70):
        done = int(last[i]) - 1                                    # the round in which its last evaluation was consumed
        for r in range(done, rounds):
            for key in ("x", "it", "ev", "loss"):
                assert np.array_equal(_bits(run[key][r][i]), _bits(run[key][done][i])), (i, key, r)
    hd = Handle(1, 40, MIXED_CFG)
    try:
        for i, p in enumerate(problems):
            hd.reset()
            _same_bits(run, _run([p], MIXED_CFG, follow=False, handle=hd), i, 0)
    finally:
        hd.close()


def test_reset_gives_a_fresh_optimiser_and_a_null_counter_is_accepted():
    case = CASES["history2"]                                       # (the ring has turned: a reset that left a pair behind would show)
    other = [lc.Quadratic(40, 30.0, 9000 + s) for s in range(3)]
    fresh = _run(case["problems"], case["cfg"], follow=False)
    hd = Handle(3, 40, case["cfg"])
    try:
        _run(other, case["cfg"], follow=False, handle=hd)          # leave another run's state behind
        hd.reset()
        again = _run(case["problems"], case["cfg"], follow=False, handle=hd)
        hd.reset()
        blind = _run(case["problems"], case["cfg"], follow=False, handle=hd, null_active_rounds=len(fresh["x"]))
    finally:
        hd.close()
    assert len(again["x"]) == len(fresh["x"]) == len(blind["x"]) and again["active"] == fresh["active"]
    for i in range(3):
        _same_bits(fresh, again, i)
        _same_bits(fresh, blind, i)


def test_a_non_finite_objective_stops_its_problem_within_one_step_and_leaves_its_neighbours_alone():
    """max_steps = 30.  A NaN objective (with a finite gradient, and with a NaN one), an infinite one at the start, an infinite and a NaN
    one at the first trial point only (lbfgs_cases.Poisoned): every problem is done within the evaluations ONE optimizer.step() can make (max_eval + max_ls + 1: a search opens while the step has
    spent less than max_eval and makes at most max_ls + 1) -- a NaN loss at the start of a step must end the outer loop as an infinite
    one does.  The host loop has a fixed round cap; nothing here can fault: the kernel only ever computes with these floats.

    MEASURED on the kernel before the fix (`!(fabsf(loss) <= 3e38f)` compiled with -fno-honor-nans is false for NaN): the "nan" problem
    had made 304 evaluations when the round cap of 4 x 76 ended the loop, and was still running; with the fix it makes 27."""
    cfg, bound = lc.POISON_CFG, lc.one_step_bound(lc.POISON_CFG)
    neighbours = [lc.Quadratic(10, 10.0, 8000 + s) for s in range(3)]
    poisoned = [lc.Poisoned(lc.poison_base(), how) for how in lc.POISONS]
    problems = [neighbours[0], poisoned[0], poisoned[1], neighbours[1], poisoned[2], poisoned[3], neighbours[2], poisoned[4]]
    where = {how: k for how, k in zip(lc.POISONS, (1, 2, 4, 5, 7))}
    run = _run(problems, cfg, follow=False, max_rounds=4 * bound)
    ev, it = run["ev"][-1], run["it"][-1]
    print("non-finite objectives: rounds", len(run["x"]), "still active", run["active"][-1], "evaluations", {h: int(ev[k]) for h, k in where.items()},
          "directions", {h: int(it[k]) for h, k in where.items()}, "one-step bound", bound)
    for how, k in where.items():
        assert ev[k] <= bound, f"{how}: {int(ev[k])} evaluations, one step makes at most {bound}"
    assert run["active"][-1] == 0
    k = where["inf_trial"]
    f_start = problems[k].base.evaluate(problems[k].x0, 0)[0]
    assert np.all(np.isfinite(run["x"][-1][k])) and np.isfinite(run["loss"][-1][k]) and run["loss"][-1][k] <= f_start
    alone = _run(neighbours, cfg, follow=False)
    for j, i in enumerate((0, 3, 6)):
        _same_bits(run, alone, i, j)
        assert np.all(np.isfinite(run["x"][-1][i])) and np.isfinite(run["loss"][-1][i])
