"""No GPU: the twin of the L-BFGS kernel (tests/lbfgs_spec.py) is checked against torch.optim.LBFGS itself, and the cases of
tests/test_gpu_lbfgs_edges.py (tests/lbfgs_cases.py) are shown to reach every branch of the algorithm with the three twin variants
in agreement, and to catch every listed mutant -- so that the GPU test may demand exact decisions with no problem excused."""
import functools

import numpy as np
import pytest
import torch

from tests import lbfgs_cases as lc
from tests.lbfgs_spec import MUTANTS, TAGS, LbfgsSpec
from tests.test_gpu_lbfgs import CFG, Quadratic, RobustFit, Rosenbrock, _as_double, _torch_lbfgs, _value_and_grad


def _no_search_reached_torchs_cap(twin):
    """Current torch caps a line search at max_eval - (evaluations of the step so far) rounds after its first evaluation, the twin
    and the kernel at max_ls.  A search of `used` evaluations has made used - 1 such rounds; the two rules take the same decisions
    in it when the two caps are equal, or when used - 1 stays below both.  (The issue's wording, "no search used as many evaluations
    as torch's cap", is stricter than that and does not hold: a step that has spent max_eval - 1 when a search opens gives it cap 1,
    and a search that accepts its first point uses 1 -- with either rule.)"""
    max_ls = twin.cfg["max_ls"]
    return all(cap == max_ls or used - 1 < min(cap, max_ls) for used, cap in twin.searches)


@pytest.mark.parametrize("family,cfg,seed,n", [
    (Quadratic, dict(CFG, max_iter=40), 11, 12),
    (Quadratic, dict(CFG, max_iter=40, history=5), 11, 12),
    (Rosenbrock, dict(CFG, max_iter=15), 11, 12),
    (Rosenbrock, dict(CFG, max_iter=400), 11, 12),
    (RobustFit, dict(CFG, max_iter=50), 11, 12),
    (RobustFit, dict(CFG, max_iter=8, max_steps=30, ftol=2e-9, gtol=1e-9), 5, 6),
], ids=["quadratic", "quadratic-history5", "rosenbrock-first15", "rosenbrock-converged", "robust", "robust-outer-loop"])
def test_twin_in_float64_takes_torchs_decisions_on_the_existing_families(family, cfg, seed, n):
    """the 66 problems of tests/test_gpu_lbfgs.py, everything in float64: the same directions, the same objective calls, the same point"""
    rng = np.random.Generator(np.random.PCG64(seed))
    for i in range(n):
        fun = _as_double(family(rng))
        xr, _, itr, evr = _torch_lbfgs(fun, cfg)
        twin = LbfgsSpec(fun.x0.numpy(), dict(cfg, max_ls=25), np.float64)
        while not twin.done:
            f, g = _value_and_grad(fun, torch.tensor(twin.x))
            twin.advance(f, g.numpy())
        assert (twin.directions, twin.evaluations) == (itr, evr), (i, twin.directions, itr, twin.evaluations, evr)
        assert np.abs(twin.x - xr.numpy()).max() <= 1e-8, i
        assert _no_search_reached_torchs_cap(twin), (i, twin.searches)


def _torch_lbfgs64(cfg, x0):
    x = torch.tensor(np.asarray(x0, dtype=np.float64), requires_grad=True)
    return x, torch.optim.LBFGS([x], lr=cfg["lr"], max_iter=cfg["max_iter"], max_eval=cfg["max_eval"] if cfg["max_eval"] > 0 else None,
                                history_size=cfg["history"], tolerance_grad=cfg["tolerance_grad"], tolerance_change=cfg["tolerance_change"],
                                line_search_fn="strong_wolfe")


def _torch_scripted(table, x0, cfg):
    """one step() of torch.optim.LBFGS in float64 whose closure returns the table's rows -> (the points it asked for, n_iter)"""
    x, opt = _torch_lbfgs64(cfg, x0)
    points = []

    def closure():
        f, g = table[min(len(points), len(table) - 1)]
        points.append(x.detach().numpy().copy())
        x.grad = torch.tensor(np.asarray(g, dtype=np.float64))
        return torch.tensor(float(f), dtype=torch.float64)
    opt.step(closure)
    return points, opt.state[x]["n_iter"], x.detach().numpy().copy()


def _torch_on(problem, cfg):
    """SMPLify-X's loop around torch.optim.LBFGS.step in float64 on problem.fg -> (n_iter, evaluations as the kernel counts them, x, loss)"""
    x, opt = _torch_lbfgs64(cfg, problem.x0)
    calls = [0]

    def closure():
        f, g = problem.fg(x.detach().numpy())
        calls[0] += 1
        x.grad = torch.tensor(g)
        return torch.tensor(float(f), dtype=torch.float64)
    prev, steps = None, 0
    for n in range(cfg["max_steps"]):
        loss = float(opt.step(closure))
        steps += 1
        if not np.isfinite(loss):
            break
        if n > 0 and cfg["ftol"] > 0 and abs(prev - loss) / max(abs(prev), abs(loss), 1.0) <= cfg["ftol"]:
            break
        if np.abs(problem.fg(x.detach().numpy())[1]).max() < cfg["gtol"]:
            break
        prev = loss
    xe = x.detach().numpy().copy()
    return opt.state[x]["n_iter"], calls[0] - (steps - 1), xe, problem.fg(xe)[0]   # (the call that opens a later step evaluates nothing new)


def _twin64_on(problem, cfg):
    twin = LbfgsSpec(problem.x0, cfg, np.float64)
    while not twin.done:
        twin.advance(*problem.fg(twin.x))
    return twin


CASES = lc.cases()
SMOOTH = [n for n, c in CASES.items() if not isinstance(c["problems"][0], lc.Scripted)]
# torch is no checker where a search reaches torch's own, smaller cap: max_ls = 1 leaves one zoom round where torch allows several
TORCHS_CAP_DIFFERS = {"rosenbrock_max_ls1"}
# 80 and 150 directions at condition 3e4 and 1e5 with both tolerances 0: two float64 summation orders (numpy's dot, torch's) drift apart
# in x (measured: 2.5e-7 and 3.5e-5 of the loss) while every count still agrees; these two are compared on the counts
DRIFTING = {"history33", "history128"}


@pytest.mark.parametrize("name", SMOOTH)
def test_twin_in_float64_takes_torchs_decisions_on_the_gpu_tests_cases(name):
    """Every smooth case of tests/test_gpu_lbfgs_edges.py -- dimensions, histories, lr, max_eval, the tolerances, the outer loop's stops,
    and the cap-limited searches at max_eval = max_ls + 1, where torch's cap on a step's first search equals the fixed one."""
    case = CASES[name]
    compared = 0
    for i, p in enumerate(case["problems"]):
        twin = _twin64_on(p, case["cfg"])
        if not _no_search_reached_torchs_cap(twin):          # (sufficient, not necessary: some of these would agree all the same)
            continue
        compared += 1
        it, ev, x, loss = _torch_on(p, case["cfg"])
        assert (twin.directions, twin.evaluations) == (it, ev), (name, i, twin.directions, it, twin.evaluations, ev)
        if name in DRIFTING:
            continue
        assert abs(float(twin.loss) - loss) <= 1e-9 * max(1.0, abs(loss)), (name, i)
        assert np.abs(twin.x - x).max() <= 1e-8 * max(1.0, np.abs(x).max()), (name, i)
    assert (compared > 0) == (name not in TORCHS_CAP_DIFFERS), (name, compared)


@pytest.mark.parametrize("name", list(lc.SCRIPTS))
def test_twin_asks_for_torchs_points_on_scripted_objectives(name):
    """The state machine only consumes f and g, so a table of (f, g) per call drives it through branches no smooth objective reaches
    robustly; torch.optim.LBFGS is driven the same way.  Every trial point equal to 1e-12, the same number of them, the same n_iter."""
    table, cfg = lc.SCRIPTS[name], lc.SCRIPT_CFG
    points, n_iter, x_end = _torch_scripted(table, lc.Scripted(table).x0, cfg)
    twin, asked, rnd = LbfgsSpec(lc.Scripted(table).x0, cfg, np.float64), [], 0
    while not twin.done:
        asked.append(twin.x.copy())
        twin.advance(*table[min(rnd, len(table) - 1)])
        rnd += 1
    assert len(asked) == len(points) and twin.directions == n_iter, (len(asked), len(points), twin.directions, n_iter)
    scale = max(1.0, max(np.abs(p).max() for p in points))
    assert max(np.abs(a - p).max() for a, p in zip(asked, points)) <= 1e-12 * scale
    assert np.abs(twin.x - x_end).max() <= 1e-12 * scale
    assert _no_search_reached_torchs_cap(twin)


@functools.lru_cache(maxsize=None)
def _led_by_float32(name):
    """every problem of a case with a float32 twin in the kernel's place -> [(counts, points, Lockstep)]"""
    return [lc.lead_on_cpu(p, CASES[name]["cfg"]) for p in CASES[name]["problems"]]


@pytest.mark.parametrize("name", list(CASES))
def test_the_three_variants_agree_on_every_round_of_every_case(name):
    """float64, float32 and float32 summed in reverse take identical decisions to the end of every problem: nothing in the GPU test
    is excused.  (The GPU test asserts the same of its own run: its leader is the kernel, whose points differ by rounding.)"""
    for i, (counts, xs, lock) in enumerate(_led_by_float32(name)):
        h, worst = lc.compare(counts, xs, lock, f"{name}[{i}]")
        assert lock.all_done() and h == len(lock.twins["f64"].rounds) == len(counts), (name, i, h, len(counts))
        drops = sum(1 for r, t in lock.twins["f64"].tags if t == "ring_drop_oldest" and r < h)
        assert drops >= CASES[name]["min_drops"], (name, i, drops)


def test_every_branch_is_reached_by_a_case_of_the_gpu_test():
    assert set(lc.CATALOGUE) | set(lc.UNREACHABLE_WHEN_FINITE) == set(TAGS) and not set(lc.CATALOGUE) & set(lc.UNREACHABLE_WHEN_FINITE)
    for tag, name in lc.CATALOGUE.items():
        reached = [i for i, (_, _, lock) in enumerate(_led_by_float32(name))
                   if any(t == tag and r < lock.horizon() for r, t in lock.twins["f64"].tags)]
        assert reached, f"{tag}: not reached by case {name} inside the twins' horizon"


def test_the_poisoned_problems_reach_the_two_branches_no_finite_value_reaches():
    """... and the twin itself has the properties the GPU test asks of the kernel: done within one step's evaluations"""
    cfg, seen = lc.POISON_CFG, set()
    for how in lc.POISONS:
        p = lc.Poisoned(lc.poison_base(), how)
        for _, dtype, dot in lc.VARIANTS:
            twin, rnd = LbfgsSpec(p.x0, lc.as_float32(cfg), dtype, dot), 0
            while not twin.done:
                assert rnd <= lc.one_step_bound(cfg)
                twin.advance(*p.evaluate(twin.x.astype(np.float32), rnd))
                rnd += 1
            assert twin.evaluations <= lc.one_step_bound(cfg)
            seen |= {t for _, t in twin.tags}
            if how == "inf_trial":
                assert np.all(np.isfinite(twin.x)) and np.isfinite(twin.loss) and twin.loss <= p.base.evaluate(p.x0, 0)[0]
    assert set(lc.UNREACHABLE_WHEN_FINITE) <= seen, seen


def test_a_nan_minimiser_is_clipped_by_the_ieee_rule():
    twin = LbfgsSpec(np.zeros(2), {}, np.float32)
    with np.errstate(all="ignore"):
        nan = np.float32(np.nan)
        f = np.float32
        # f2 = +inf: d1 = -inf, d2 = inf, (g2 + d2 - d1) / (g2 - g1 + 2 d2) = inf / inf: the minimiser is NaN, the result the lower bound
        assert twin._cubic(f(0), f(1), f(-1), f(2), f(np.inf), f(1), bounds=(f(2.5), f(20))) == 2.5
        # ... and a NaN value leaves no real minimiser at all: the middle
        assert twin._cubic(f(0), f(1), f(-1), f(2), nan, f(1), bounds=(f(2.5), f(20))) == 11.25


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_of_the_twin_leaves_the_gpu_tests_bars(mutant):
    """A float32 twin with one deliberate mistake, in the kernel's place: on its designated case the rule of lbfgs_cases.compare fails --
    a count differs from the float64 twin's, or a trial point leaves the bar."""
    name = lc.MUTANT_CASES[mutant]
    caught = []
    for i, p in enumerate(CASES[name]["problems"]):
        counts, xs, lock = lc.lead_on_cpu(p, CASES[name]["cfg"], mutant=mutant)
        try:
            lc.compare(counts, xs, lock, f"{name}[{i}]")
        except AssertionError as e:
            caught.append(str(e))
    print(mutant, name, caught[:1])
    assert caught, f"{mutant} passes on case {name}"
