"""torch.optim.LBFGS(line_search_fn="strong_wolfe") with SMPLify-X's loop around optimizer.step(), as a plain numpy twin of the
batched L-BFGS kernel (include/fdcap.h fdcap_lbfgs_*, csrc/fdc_lbfgs.h).

Written from torch/optim/lbfgs.py and the header's description of the settings, not from the kernel: the history is three Python
lists with pop(0), the line search is the nested loops torch has, and "resumable" is a generator that yields wherever the algorithm
calls its closure.  `advance(f, g)` hands it the objective at the point `x` it asked for; afterwards `x` is the next point to
evaluate, or the result when `done`.

The rules as the kernel documents them (they are torch's unless said otherwise):
  * max_eval <= 0 means max_iter * 5 // 4;
  * a line search may make max_ls extrapolation / zoom rounds after its first evaluation, whatever the step has spent.  Current
    torch passes max_eval - (evaluations of this step so far) instead; the two coincide wherever no search reaches the smaller cap;
  * c1 = 1e-4, c2 = 0.9, history skipped when y's <= 1e-10;
  * the loop around step(): stop when the loss at the start of a step is not finite, when it differs from the previous step's start
    by <= ftol relative to max(|a|, |b|, 1) (ftol > 0, from the second step on), when every gradient entry at the accepted point is
    below gtol, or after max_steps steps.  `evaluations` does not count the closure call that opens a later step (nothing new is
    evaluated there: the accepted point's loss and gradient are known).

NON-FINITE INTERPOLANTS.  The minimiser of a cubic is clipped with the IEEE rule fmin(fmax(m, lo), hi): a NaN minimiser gives `lo`
(C's fminf / fmaxf return the other operand), where Python's min(max(...)) would pass the NaN on.  A NaN minimiser needs a non-finite
loss or gradient; such runs are held to properties (they stop, they stay finite where they can), not to equality with anything.

`dtype` is the arithmetic of every scalar and vector; `dot` is the inner product (so that a second float32 variant can sum in another
order); `mutant` names one deliberate mistake (MUTANTS): tests/test_lbfgs_spec_cpu.py shows that each leaves the bars of
tests/test_gpu_lbfgs_edges.py.  Per branch taken the twin records (round, tag) in `tags`, per round (directions, evaluations, done)
in `rounds`, and per line search (evaluations it used, the cap current torch would have given it) in `searches`."""
import numpy as np

TAGS = (
    "step_start_optimal",            # step(): the gradient is already within tolerance_grad
    "first_direction", "history_update", "history_skip", "ring_drop_oldest",
    "flat_direction",                # g'd > -tolerance_change
    "bracket_armijo", "bracket_not_decreasing", "bracket_wolfe", "bracket_rising", "bracket_extrapolate", "bracket_out_of_evals",
    "zoom_out_of_evals", "zoom_bracket_small", "extrapolate_bisect", "zoom_bisect",
    "insuf_first_time", "insuf_moved_at_end", "insuf_moved_second_time",
    "zoom_replace_high", "zoom_low_high_swap", "zoom_wolfe", "zoom_old_low_becomes_high", "zoom_new_low",
    "stop_max_iter", "stop_max_eval", "stop_tolerance_grad", "stop_small_step", "stop_small_change",
    "outer_nonfinite", "outer_ftol", "outer_gtol", "outer_max_steps",
)
MUTANTS = ("ring_keeps_oldest", "recursion_wrong_order", "no_H_diag_update", "armijo_ge", "no_ls_iter_gt_1", "no_safeguard",
           "low_not_recomputed", "first_step_unscaled", "lr_ignored_later", "max_eval_ignored", "evals_not_reset", "ftol_uses_loss")

DEFAULTS = dict(history=100, max_iter=20, max_eval=0, max_steps=1, max_ls=25, lr=1.0, tolerance_grad=1e-7, tolerance_change=1e-9,
                ftol=0.0, gtol=0.0)


def dot_forward(a, b):
    return np.dot(a, b)


def dot_reversed(a, b):
    return np.dot(np.ascontiguousarray(a[::-1]), np.ascontiguousarray(b[::-1]))


class LbfgsSpec:
    def __init__(self, x0, cfg, dtype=np.float64, dot=dot_forward, mutant=None):
        assert mutant is None or mutant in MUTANTS, mutant
        self.T, self.dot, self.mutant = dtype, dot, mutant
        self.cfg = c = dict(DEFAULTS, **cfg)
        if c["max_eval"] <= 0:
            c["max_eval"] = c["max_iter"] * 5 // 4
        self.x = np.array(x0, dtype=dtype)
        self.done = False
        self.directions = self.evaluations = 0
        self.loss = None                                        # the objective at the accepted point
        self.tags, self.rounds, self.searches = [], [], []
        self._run = self._fit()
        next(self._run)                                         # up to the first closure call

    # ---- the resumable surface --------------------------------------------------------------------------------------------
    def advance(self, f, g):
        assert not self.done
        with np.errstate(all="ignore"):
            try:
                self._run.send((self.T(f), np.array(g, dtype=self.T)))
            except StopIteration:
                self.done = True
        self.rounds.append((self.directions, self.evaluations, self.done))

    def tag(self, name):
        assert name in TAGS, name
        self.tags.append((len(self.rounds), name))

    def _closure(self, x):
        self.x = x
        f, g = yield
        self.evaluations += 1
        return f, g

    def _absmax(self, v):
        return np.max(np.abs(v))

    # ---- SMPLify-X's loop around optimizer.step() -------------------------------------------------------------------------
    def _fit(self):
        c, T = self.cfg, self.T
        self.loss, self.grad = yield from self._closure(self.x)
        self.old_dirs, self.old_stps, self.ro, self.H_diag = [], [], [], T(1)
        self.d = self.t = self.prev_grad = self.prev_loss = None
        self.step_evals = 0
        prev = None
        for n in range(c["max_steps"]):
            orig_loss = self.loss
            yield from self._step()
            cur = self.loss if self.mutant == "ftol_uses_loss" else orig_loss
            if not np.isfinite(orig_loss):
                return self.tag("outer_nonfinite")
            if n > 0 and c["ftol"] > 0 and abs(prev - cur) / max(abs(prev), abs(cur), T(1)) <= T(c["ftol"]):
                return self.tag("outer_ftol")
            if self._absmax(self.grad) < T(c["gtol"]):
                return self.tag("outer_gtol")
            prev = cur
        self.tag("outer_max_steps")

    # ---- torch.optim.LBFGS.step ---------------------------------------------------------------------------------------------
    def _step(self):
        c, T, dot, mutant = self.cfg, self.T, self.dot, self.mutant
        tol_grad, tol_change, lr = T(c["tolerance_grad"]), T(c["tolerance_change"]), T(c["lr"])
        current_evals = self.step_evals + 1 if mutant == "evals_not_reset" else 1
        if self._absmax(self.grad) <= tol_grad:
            return self.tag("step_start_optimal")
        n_iter = 0
        while n_iter < c["max_iter"]:
            n_iter += 1
            self.directions += 1
            g = self.grad
            if self.directions == 1:
                self.tag("first_direction")
                d = -g
            else:
                y, s = g - self.prev_grad, self.d * self.t
                ys = dot(y, s)
                if ys > T(1e-10):
                    if len(self.old_dirs) == c["history"]:
                        self.tag("ring_drop_oldest")
                        drop = -1 if mutant == "ring_keeps_oldest" else 0
                        self.old_dirs.pop(drop), self.old_stps.pop(drop), self.ro.pop(drop)
                    self.tag("history_update")
                    self.old_dirs.append(y), self.old_stps.append(s), self.ro.append(T(1) / ys)
                    if mutant != "no_H_diag_update":
                        self.H_diag = ys / dot(y, y)
                else:
                    self.tag("history_skip")
                k = len(self.old_dirs)
                al = [None] * k
                q = -g
                for i in (range(k) if mutant == "recursion_wrong_order" else reversed(range(k))):
                    al[i] = dot(self.old_stps[i], q) * self.ro[i]
                    q = q - al[i] * self.old_dirs[i]
                d = q * self.H_diag
                for i in range(k):
                    be = dot(self.old_dirs[i], d) * self.ro[i]
                    d = d + (al[i] - be) * self.old_stps[i]
            self.d, self.prev_grad, self.prev_loss = d, g.copy(), self.loss
            if self.directions == 1 and mutant != "first_step_unscaled":
                t = min(T(1), T(1) / dot(np.abs(g), np.ones_like(g))) * lr
            else:
                t = T(1) if mutant == "lr_ignored_later" and self.directions > 1 else lr
            self.t = t
            gtd = dot(g, d)
            if gtd > -tol_change:
                self.tag("flat_direction")
                break
            x_init = self.x.copy()
            before = self.evaluations
            self.loss, self.grad, self.t = yield from self._strong_wolfe(x_init, t, d, self.loss, g, gtd)
            self.x = x_init + self.t * d
            used = self.evaluations - before
            self.searches.append((used, c["max_eval"] - current_evals))
            current_evals += used
            self.step_evals = current_evals
            if n_iter == c["max_iter"]:
                self.tag("stop_max_iter")
                break
            if current_evals >= c["max_eval"] and mutant != "max_eval_ignored":
                self.tag("stop_max_eval")
                break
            if self._absmax(self.grad) <= tol_grad:
                self.tag("stop_tolerance_grad")
                break
            if self._absmax(d * self.t) <= tol_change:
                self.tag("stop_small_step")
                break
            if abs(self.loss - self.prev_loss) < tol_change:
                self.tag("stop_small_change")
                break

    # ---- torch.optim.lbfgs._cubic_interpolate, _strong_wolfe ---------------------------------------------------------------
    def _cubic(self, x1, f1, g1, x2, f2, g2, bounds=None):
        """the minimiser of the cubic through two points with slopes, clipped to `bounds` (without: to the two abscissae)"""
        T = self.T
        lo, hi = bounds if bounds is not None else (np.fmin(x1, x2), np.fmax(x1, x2))
        d1 = g1 + g2 - T(3) * (f1 - f2) / (x1 - x2)
        d2_square = d1 * d1 - g1 * g2
        if d2_square >= 0:
            d2 = np.sqrt(d2_square)
            if x1 <= x2:
                m = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + T(2) * d2))
            else:
                m = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + T(2) * d2))
            return np.fmin(np.fmax(m, lo), hi)                  # (the IEEE rule: see the module's docstring)
        self.tag("zoom_bisect" if bounds is None else "extrapolate_bisect")     # no real minimiser: the middle
        return (lo + hi) / T(2)

    def _strong_wolfe(self, x, t, d, f, g, gtd):
        T, dot, mutant = self.T, self.dot, self.mutant
        c1, c2, tol_change, max_ls = T(1e-4), T(0.9), T(self.cfg["tolerance_change"]), self.cfg["max_ls"]

        def armijo_fails(f_new, t):
            bound = f + c1 * t * gtd
            return f_new >= bound if mutant == "armijo_ge" else f_new > bound
        d_norm = self._absmax(d)
        f_new, g_new = yield from self._closure(x + t * d)
        gtd_new = dot(g_new, d)
        t_prev, f_prev, g_prev, gtd_prev = T(0), f, g, gtd
        done, ls_iter = False, 0
        while ls_iter < max_ls:
            not_decreasing = (ls_iter > 1 or mutant == "no_ls_iter_gt_1") and f_new >= f_prev
            if armijo_fails(f_new, t) or not_decreasing:
                self.tag("bracket_armijo" if armijo_fails(f_new, t) else "bracket_not_decreasing")
                bracket, bracket_f, bracket_g, bracket_gtd = [t_prev, t], [f_prev, f_new], [g_prev, g_new], [gtd_prev, gtd_new]
                break
            if abs(gtd_new) <= -c2 * gtd:
                self.tag("bracket_wolfe")
                bracket, bracket_f, bracket_g, done = [t], [f_new], [g_new], True
                break
            if gtd_new >= 0:
                self.tag("bracket_rising")
                bracket, bracket_f, bracket_g, bracket_gtd = [t_prev, t], [f_prev, f_new], [g_prev, g_new], [gtd_prev, gtd_new]
                break
            self.tag("bracket_extrapolate")
            min_step, max_step = t + T(0.01) * (t - t_prev), t * T(10)
            t_next = self._cubic(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, bounds=(min_step, max_step))
            t_prev, f_prev, g_prev, gtd_prev, t = t, f_new, g_new, gtd_new, t_next
            f_new, g_new = yield from self._closure(x + t * d)
            gtd_new = dot(g_new, d)
            ls_iter += 1
        if ls_iter == max_ls:
            self.tag("bracket_out_of_evals")
            bracket, bracket_f, bracket_g, done = [T(0), t], [f, f_new], [g, g_new], True       # (no zoom round is left)

        insuf_progress = False
        low, high = (0, 1) if bracket_f[0] <= bracket_f[-1] else (1, 0)
        while not done:
            if ls_iter >= max_ls:
                self.tag("zoom_out_of_evals")
                break
            if abs(bracket[1] - bracket[0]) * d_norm < tol_change:
                self.tag("zoom_bracket_small")
                break
            t = self._cubic(bracket[0], bracket_f[0], bracket_gtd[0], bracket[1], bracket_f[1], bracket_gtd[1])
            b_max, b_min = np.fmax(bracket[0], bracket[1]), np.fmin(bracket[0], bracket[1])
            eps = T(0.1) * (b_max - b_min)
            if np.fmin(b_max - t, t - b_min) < eps and mutant != "no_safeguard":
                if insuf_progress or t >= b_max or t <= b_min:
                    self.tag("insuf_moved_second_time" if insuf_progress else "insuf_moved_at_end")
                    t = b_max - eps if abs(t - b_max) < abs(t - b_min) else b_min + eps
                    insuf_progress = False
                else:
                    self.tag("insuf_first_time")
                    insuf_progress = True
            else:
                insuf_progress = False
            f_new, g_new = yield from self._closure(x + t * d)
            gtd_new = dot(g_new, d)
            ls_iter += 1
            if armijo_fails(f_new, t) or f_new >= bracket_f[low]:
                self.tag("zoom_replace_high")
                bracket[high], bracket_f[high], bracket_g[high], bracket_gtd[high] = t, f_new, g_new, gtd_new
                if mutant != "low_not_recomputed":
                    was = low
                    low, high = (0, 1) if bracket_f[0] <= bracket_f[1] else (1, 0)
                    if low != was:
                        self.tag("zoom_low_high_swap")
            else:
                if abs(gtd_new) <= -c2 * gtd:
                    self.tag("zoom_wolfe")
                    done = True
                elif gtd_new * (bracket[high] - bracket[low]) >= 0:
                    self.tag("zoom_old_low_becomes_high")
                    bracket[high], bracket_f[high], bracket_g[high], bracket_gtd[high] = \
                        bracket[low], bracket_f[low], bracket_g[low], bracket_gtd[low]
                else:
                    self.tag("zoom_new_low")
                bracket[low], bracket_f[low], bracket_g[low], bracket_gtd[low] = t, f_new, g_new, gtd_new
        return bracket_f[low], bracket_g[low], bracket[low]
