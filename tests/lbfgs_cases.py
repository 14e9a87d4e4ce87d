"""The problems, settings and comparison rule shared by tests/test_lbfgs_spec_cpu.py (no GPU: the twin against torch, the branch
catalogue, the mutants) and tests/test_gpu_lbfgs_edges.py (the kernel against the twin, round by round).

LOCKSTEP.  Somebody leads -- the kernel on the GPU, a float32 twin or a mutant of it on the CPU: each round the objective is
evaluated in float64 at the leader's float32 point and rounded to float32 (a scripted problem takes its table's row instead), and
the same f, g go to the leader and to three followers: the twin of tests/lbfgs_spec.py in float64, in float32, and in float32 with
its dot products summed in reverse.  All see identical inputs; what differs is the optimiser's own arithmetic.

THE RULE (`compare`).  Up to the first round in which the three followers disagree among themselves on (directions, evaluations,
done) -- the horizon -- the leader must report the float64 twin's counts exactly, and its point must stay within
MARGIN x max(|x_f32 - x_f64|, 2^-24 max|x_f64|) of the float64 twin's, per problem and round: a bar made of the twins alone."""
import numpy as np

from tests.lbfgs_spec import LbfgsSpec, dot_forward, dot_reversed

MARGIN = 32.0
VARIANTS = (("f64", np.float64, dot_forward), ("f32", np.float32, dot_forward), ("f32r", np.float32, dot_reversed))


# ---- objectives: float64 at a float32 point, rounded to float32 --------------------------------------------------------------
class Problem:
    def evaluate(self, x, rnd):
        with np.errstate(all="ignore"):
            f, g = self.fg(np.asarray(x, dtype=np.float64))
            return np.float32(f), np.asarray(g, dtype=np.float32)


class Quadratic(Problem):
    """f = 1/2 x'Ax - b'x, A symmetric positive definite with condition number `cond`"""
    def __init__(self, dim, cond, seed):
        rng = np.random.default_rng(seed)
        q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
        self.dim, self.A = dim, (q * np.geomspace(1.0, cond, dim)) @ q.T
        self.A = 0.5 * (self.A + self.A.T)
        self.b, self.x0 = rng.standard_normal(dim), rng.standard_normal(dim).astype(np.float32)

    def fg(self, x):
        return 0.5 * x @ (self.A @ x) - self.b @ x, self.A @ x - self.b


class Rosenbrock(Problem):
    def __init__(self, dim, seed):
        self.dim, self.x0 = dim, np.random.default_rng(seed).uniform(-1.5, 1.5, dim).astype(np.float32)

    def fg(self, x):
        a, b = x[1:] - x[:-1] ** 2, 1.0 - x[:-1]
        g = np.zeros_like(x)
        g[:-1] = -400.0 * a * x[:-1] - 2.0 * b
        g[1:] += 200.0 * a
        return np.sum(100.0 * a ** 2 + b ** 2), g


class Concave(Problem):
    """f = -sum (1 + x^2)^(5/8): descent without end, so bracketing extrapolates until it is out of evaluations.  (Growing like
    |x|^1.25 it keeps its curvature far out, where -sqrt(1 + x^2) turns linear and its cubics degenerate into ties.)"""
    def __init__(self, dim, seed):
        self.dim, self.x0 = dim, np.random.default_rng(seed).uniform(0.1, 1.0, dim).astype(np.float32)

    def fg(self, x):
        r = 1.0 + x * x
        return -np.sum(r ** 0.625), -1.25 * x * r ** -0.375


class Flat(Problem):
    def __init__(self, dim):
        self.dim, self.x0 = dim, np.arange(dim, dtype=np.float32)

    def fg(self, x):
        return 1.5, np.zeros_like(x)


class Scripted(Problem):
    """(f, g) per round from a table, whatever the point: the state machine only consumes f and g"""
    def __init__(self, table, x0=(0.25, -0.5)):
        self.table, self.x0, self.dim = table, np.asarray(x0, dtype=np.float32), len(x0)

    def evaluate(self, x, rnd):
        f, g = self.table[min(rnd, len(self.table) - 1)]
        return np.float32(f), np.asarray(g, dtype=np.float32)


class Poisoned(Problem):
    """`base` with a non-finite objective:
      "nan"        f = NaN at every point, with a gradient that never changes (the start's): no search ever finds a point to accept, so
                   the problem spends all the evaluations it is given -- what ends it is the loop around step() alone;
      "nan_all"    f and every gradient entry NaN at every point;
      "inf_start"  f = +inf at the start;  "inf_trial"  f = +inf at the first trial point only;
      "nan_trial"  f = NaN at the first trial point, with a gradient that makes the point close the bracket (the zoom's cubic then has
                   no real minimiser: the one way into its bisection)"""
    def __init__(self, base, how):
        self.base, self.how, self.dim, self.x0 = base, how, base.dim, base.x0
        self.g0 = base.evaluate(base.x0, 0)[1]

    def evaluate(self, x, rnd):
        f, g = self.base.evaluate(x, rnd)
        if self.how == "nan":
            return np.float32(np.nan), self.g0
        if self.how == "nan_all":
            return np.float32(np.nan), np.full_like(g, np.nan)
        if (self.how, rnd) in (("inf_start", 0), ("inf_trial", 1)):
            return np.float32(np.inf), g
        if (self.how, rnd) == ("nan_trial", 1):
            return np.float32(np.nan), -self.g0
        return f, g


# ---- lockstep -----------------------------------------------------------------------------------------------------------------
def as_float32(cfg):
    """the settings as the kernel holds them: float32 (so that no comparison with a tolerance differs by the tolerance's own rounding)"""
    return {k: float(np.float32(v)) if isinstance(v, float) else v for k, v in cfg.items()}


class Lockstep:
    """the three followers of one problem"""
    def __init__(self, problem, cfg):
        self.twins = {n: LbfgsSpec(problem.x0, as_float32(cfg), dt, dot) for n, dt, dot in VARIANTS}
        self.xs = {n: [] for n in self.twins}

    def feed(self, f, g):
        for n, t in self.twins.items():
            if not t.done:
                t.advance(f, g)
                self.xs[n].append(t.x.copy())

    def horizon(self):
        """the first round in which the followers disagree; with no disagreement, the number of rounds they all ran"""
        recs = [t.rounds for t in self.twins.values()]
        n = min(len(r) for r in recs)
        for r in range(n):
            if not (recs[0][r] == recs[1][r] == recs[2][r]):
                return r
        return n

    def all_done(self):
        return all(t.done for t in self.twins.values())


def compare(lead_counts, lead_xs, lock, what=""):
    """THE RULE of the module's docstring.  lead_counts[r] = (directions, evaluations) or (directions, evaluations, done) after
    round r, lead_xs[r] the leader's point.  -> (horizon, worst |error| / bar); AssertionError where the rule is broken."""
    h, t64 = lock.horizon(), lock.twins["f64"]
    worst = 0.0
    for r in range(min(h, len(lead_counts))):
        ref = t64.rounds[r]
        assert tuple(lead_counts[r]) == ref[:len(lead_counts[r])], f"{what} round {r}: counts {tuple(lead_counts[r])}, the float64 twin's {ref}"
        x64, x32 = lock.xs["f64"][r], lock.xs["f32"][r].astype(np.float64)
        bar = MARGIN * max(np.abs(x32 - x64).max(), 2.0 ** -24 * np.abs(x64).max())
        err = np.abs(np.asarray(lead_xs[r], dtype=np.float64) - x64).max()
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else np.inf)
        assert ratio <= 1.0, f"{what} round {r}: |x - x_f64| = {err:.3e}, {ratio:.2f} bars"
        worst = max(worst, ratio)
    assert len(lead_counts) >= h, f"{what}: the leader stopped after {len(lead_counts)} rounds, the twins agree on {h}"
    return h, worst


def lead_on_cpu(problem, cfg, mutant=None, max_rounds=2000):
    """a float32 twin (or a mutant of it) in the kernel's place -> (its counts, its points, the Lockstep of its followers)"""
    lead, lock = LbfgsSpec(problem.x0, as_float32(cfg), np.float32, mutant=mutant), Lockstep(problem, cfg)
    xs = []
    for rnd in range(max_rounds):
        if lead.done:
            break
        f, g = problem.evaluate(lead.x.astype(np.float32), rnd)
        lead.advance(f, g)
        xs.append(lead.x.copy())
        if not lock.all_done():
            lock.feed(f, g)
    return lead.rounds, xs, lock


# ---- the cases of tests/test_gpu_lbfgs_edges.py (tests/test_lbfgs_spec_cpu.py runs every one of them here first) ---------------
BASE = dict(history=100, max_iter=12, max_eval=0, max_steps=1, max_ls=25, lr=1.0, tolerance_grad=1e-7, tolerance_change=1e-9,
            ftol=0.0, gtol=0.0)
_END = (-0.01, 0.0)                                              # a last row's gradient: small, so that whatever follows is accepted
SCRIPTS = {
    # f does not decrease after two extrapolations although Armijo holds (torch's 15 trial points equal the twin's to 1e-12)
    "not_decreasing": [(0, [-1, .5]), (-.6, [-1, .5]), (-3, [-1, .5]), (-2.9, [-1, .5]), (-3.2, [-.1, .05])] + [(-3.2, [-.01, 0])] * 10,
    # a zoom whose cubic lands within 10 % of an end twice in a row: moved the second time; the bracket shrinks below tolerance_change
    "insuf_twice": [(0.0, [-1.0, 0.5]), (-3.375, [0.625, 0.375]), (0.5, [-0.75, 1.625]), (-0.75, [-1.0, -0.75]), (-0.25, [0.75, 0.5]),
                    (-0.25, _END)],
    # ... lands ON an end: moved at once; a replaced high end that is lower than the low end: the two swap
    "insuf_at_end": [(0.0, [-1.0, 0.5]), (0.625, [-0.875, 1.375]), (0.875, [-1.75, -1.5]), (-0.125, [-0.125, -1.625]), (-1.25, [0.125, 0.5]),
                     (-1.625, [-1.75, -1.5]), (-1.625, [-0.375, 0.125]), (-1.25, [-2.0, 0.875]), (-0.5, [1.0, 0.125]),
                     (-0.375, [0.125, 1.875]), (-3.75, [-1.875, 1.875]), (-3.75, _END)],
    "swap": [(0.0, [-1.0, 0.5]), (-0.875, [-1.125, 1.375]), (-1.625, [0.75, -1.75]), (-1.625, [-1.125, -1.125]), (-1.75, [1.125, 1.25]),
             (-2.125, [1.75, -1.125]), (-2.5, [-0.25, 0.375]), (0.5, [1.0, -0.875]), (-1.125, [0.125, -1.625]), (0.5, [-0.875, -0.875]),
             (0.5, _END)],
    "new_low": [(0.0, [-1.0, 0.5]), (-3.0, [0.625, 0.0]), (0.125, [-0.25, 1.125]), (0.75, [-1.5, -0.5]), (-0.625, [1.75, -1.75]),
                (-0.375, [-1.25, 1.75]), (-3.25, [1.875, -2.0]), (-3.25, _END)],
    "old_low_becomes_high": [(0.0, [-1.0, 0.5]), (1.0, [-1.75, -1.875]), (-0.25, [1.375, 1.875]), (0.75, [1.625, 1.5]), (0.5, [0.375, -1.875]),
                             (0.5, [-0.75, 0.375]), (-3.5, [0.75, -1.625]), (-3.5, _END)],
    "history_skip": [(0.0, [-1.0, 0.5]), (-0.375, [0.0, -0.375]), (-0.75, [1.25, 1.5]), (0.625, [2.0, -0.625]), (-2.75, [0.125, -2.0]),
                     (-1.875, [0.875, 0.25]), (-1.125, [2.0, -0.25]), (-0.625, [-1.0, -0.625]), (-3.75, [1.25, -1.375]), (-3.75, _END)],
    # Armijo with equality in every arithmetic: at f = 2^60 the bound f + c1 t g'd rounds to f in float32 and float64 alike
    "armijo_tie": [(2.0 ** 60, [-1, .5]), (2.0 ** 60, [-1, .5]), (2.0 ** 60 - 2.0 ** 40, [-.1, .05]), (2.0 ** 60 - 2.0 ** 40, _END)],
    # the second trial is no lower than the first, Armijo holds: only from the third on may that close the bracket
    "second_not_lower": [(0, [-1, .5]), (-3, [-1, .5]), (-2.9, [-1, .5]), (-3.2, [-.1, .05])] + [(-3.2, [-.01, 0])] * 4,
}
SCRIPT_CFG = dict(BASE, max_iter=3, max_eval=40)
# A new high end below the low end (Armijo fails by a hair, yet f < f_low): the two swap, and the search runs out of evaluations before
# anything else is accepted -- the step taken is the swapped low end
SCRIPT_SWAP_THEN_OUT = [(0, [-1, .5]), (1, [1, -.5]), (-2.0 ** -20, [-.5, .25]), (1, [1, -.5]), (1, [1, -.5])]


def _case(problems, cfg, x_pad=5, g_pad=2, min_drops=0, **kw):
    return dict(problems=problems, cfg=cfg, x_pad=x_pad, g_pad=g_pad, min_drops=min_drops, **kw)


def cases():
    """name -> dict(problems, cfg, x_pad / g_pad: the x and g rows are dim + pad floats wide, min_drops: the ring must have dropped
    its oldest pair that often before the twins' horizon)"""
    c = {}
    for dim in (1, 2, 63, 64, 65, 127, 128):                     # a lane holds elements [lane] and [lane + 64]
        c[f"dim{dim}"] = _case([Quadratic(dim, 300.0, 100 * dim + s) for s in (1, 2)], BASE, x_pad=0 if dim == 128 else 5)
    for hist in (1, 2):
        c[f"history{hist}"] = _case([Quadratic(40, 300.0, 4000 + s) for s in (1, 2, 3)], dict(BASE, history=hist, max_iter=25),
                                    min_drops=24 - hist)
    open_end = dict(tolerance_grad=0.0, tolerance_change=0.0)
    c["history33"] = _case([Quadratic(64, 3e4, 6400 + s) for s in (1, 2)], dict(BASE, history=33, max_iter=80, **open_end), min_drops=33)
    c["history128"] = _case([Quadratic(128, 1e5, 12800 + s) for s in (1, 2)], dict(BASE, history=128, max_iter=150, **open_end), min_drops=5)
    c["lr0.25"] = _case([Quadratic(40, 300.0, 4100 + s) for s in (1, 2, 3)], dict(BASE, lr=0.25))
    c["lr2"] = _case([Quadratic(40, 300.0, 4100 + s) for s in (1, 2, 3)], dict(BASE, lr=2.0))
    c["max_eval"] = _case([Quadratic(40, 300.0, 4200 + s) for s in (1, 2, 3)], dict(BASE, max_eval=7, max_steps=3))
    c["tolerance_grad"] = _case([Quadratic(20, 10.0, 2000 + s) for s in (1, 2, 3)], dict(BASE, max_iter=60, tolerance_grad=1e-3, max_steps=2))
    c["gtol"] = _case([Quadratic(20, 10.0, 2100 + s) for s in (1, 2, 3)], dict(BASE, max_iter=4, gtol=1e-2, max_steps=10))
    c["ftol"] = _case([Quadratic(20, 10.0, 2200 + s) for s in (1, 2, 3)], dict(BASE, max_iter=2, max_eval=6, ftol=1e-2, max_steps=30))
    for dim in (1, 64, 65, 128):                                 # max_eval = max_ls + 1: torch's cap equals the fixed one in every step's first search
        c[f"concave{dim}"] = _case([Concave(dim, dim), Concave(dim, dim + 1000)], dict(BASE, max_ls=4, max_eval=5, max_steps=3))
    c["rosenbrock_max_ls1"] = _case([Rosenbrock(10, 0)], dict(BASE, max_ls=1, max_iter=15))
    c["rosenbrock"] = _case([Rosenbrock(10, s) for s in (1, 2, 3)], dict(BASE, max_iter=60))
    c["scripted"] = _case([Scripted(t) for t in SCRIPTS.values()], SCRIPT_CFG)
    c["scripted_max_ls2"] = _case([Scripted(SCRIPT_SWAP_THEN_OUT)], dict(BASE, max_iter=1, max_eval=40, max_ls=2))
    return c


# tag -> a case that reaches it inside the twins' horizon (tests/test_lbfgs_spec_cpu.py checks every line, and that TAGS has no other)
CATALOGUE = {
    "step_start_optimal": "tolerance_grad", "first_direction": "dim64", "history_update": "dim64", "history_skip": "scripted",
    "ring_drop_oldest": "history2", "flat_direction": "rosenbrock",
    "bracket_armijo": "dim65", "bracket_not_decreasing": "scripted", "bracket_wolfe": "dim1", "bracket_rising": "dim127",
    "bracket_extrapolate": "dim63", "bracket_out_of_evals": "concave65",
    "zoom_out_of_evals": "rosenbrock_max_ls1", "zoom_bracket_small": "scripted", "extrapolate_bisect": "concave128",
    "insuf_first_time": "scripted", "insuf_moved_at_end": "scripted", "insuf_moved_second_time": "scripted",
    "zoom_replace_high": "scripted", "zoom_low_high_swap": "scripted", "zoom_wolfe": "dim128", "zoom_old_low_becomes_high": "scripted",
    "zoom_new_low": "scripted",
    "stop_max_iter": "dim64", "stop_max_eval": "max_eval", "stop_tolerance_grad": "tolerance_grad", "stop_small_step": "scripted",
    "stop_small_change": "scripted",
    "outer_ftol": "ftol", "outer_gtol": "gtol", "outer_max_steps": "dim64",
}
# Not reachable with finite values (the poisoned problems of tests/test_gpu_lbfgs_edges.py reach them; they are held to properties):
#   outer_nonfinite   by its meaning;
#   zoom_bisect       the zoom's cubic has a real minimiser whenever its inputs are finite.  The bracket keeps f_low <= f_high and the
#                     slope at the low end pointing into the bracket: with h = x_high - x_low, g_low h < 0.  d1 = g_low + g_high - 3 (f_high -
#                     f_low) / h.  If g_low g_high <= 0 then d1^2 - g_low g_high >= 0 at once.  Otherwise both slopes have the sign of -h, so
#                     (g_low + g_high) and -3 (f_high - f_low) / h have the same sign (f_high - f_low >= 0): |d1| >= |g_low + g_high| >=
#                     2 sqrt(g_low g_high), and d1^2 >= 4 g_low g_high > g_low g_high.  (Bracketing's extrapolation has no such invariant:
#                     extrapolate_bisect is reached, by the concave cases.)
UNREACHABLE_WHEN_FINITE = ("outer_nonfinite", "zoom_bisect")

# mutant of tests/lbfgs_spec.py -> the case that catches it
MUTANT_CASES = {
    "ring_keeps_oldest": "history2", "recursion_wrong_order": "dim64", "no_H_diag_update": "dim64", "armijo_ge": "scripted",
    "no_ls_iter_gt_1": "scripted", "no_safeguard": "scripted", "low_not_recomputed": "scripted_max_ls2", "first_step_unscaled": "dim64",
    "lr_ignored_later": "lr0.25", "max_eval_ignored": "max_eval", "evals_not_reset": "max_eval", "ftol_uses_loss": "ftol",
}


# ---- non-finite objectives: properties, not equality (tests/test_gpu_lbfgs_edges.py) -----------------------------------------------
POISON_CFG = dict(BASE, max_iter=40, max_steps=30, tolerance_grad=1e-2)
POISONS = ("nan", "inf_start", "inf_trial", "nan_trial", "nan_all")


def poison_base():
    return Quadratic(10, 10.0, 77)


def one_step_bound(cfg):
    """evaluations of one optimizer.step(): a search opens while the step has spent < max_eval, and makes at most max_ls + 1"""
    max_eval = cfg["max_eval"] if cfg["max_eval"] > 0 else cfg["max_iter"] * 5 // 4
    return max_eval + cfg["max_ls"] + 1
