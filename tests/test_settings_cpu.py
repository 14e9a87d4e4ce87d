"""Loss weights, step sizes and intrinsics away from their defaults: what needs no GPU.

The reference's defaults coincide pairwise (weight_contact == phase1_contact == 0.1, weight_loss_rec == phase1_smooth ==
phase2_world == 1, fx == fy, w_pose == w_hand, w_data == 1), so a suite that only runs the defaults cannot see two settings wired
to each other's place.  tests/test_gpu_settings.py runs the kernels at ONE odd set (ODD below: pairwise distinct, none 0, 1 or a
default) against the oracle; this file holds what both share -- the odd set, the cases, the oracle's per-term gradients, the bars
-- and evaluates on the CPU

  * the sensitivity conditions: every swap of two settings and every single setting put back to its default must move the
    ORACLE's result out of the bar the GPU test uses by a factor (20 for the gradients), so none of those tests can pass with such a
    mistake in the wiring;
  * the yardsticks: the fp64 oracle against the fp32 oracle at the odd settings, which a bar for a whole fit must exceed 3x;
  * the host build of the kernels' math (tests/host_pipeline.py) at the odd settings against fp64 autograd;
  * the oracle's new keywords at their defaults against the loop body as it was written before they existed."""
import functools
import itertools

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import synth
from fdcap_amd.fitting import find_outliers
from oracle import rotrepr
from oracle.fitting import FittingOracle
from oracle.innerfit import InnerFitOracle
from oracle.smoother import SmootherOracle
from oracle.smplx import SMPLXOracle
from oracle.vposer import VPoserDecoder

# Two values are not the ones first proposed for this set (phase2_world 1.6, scale_init 1.45).  With those the sensitivity condition
# below failed for single outputs: the world term's gradient (max 0.08 per unit weight) set atol = 2e-4 max|g| of the phase-2 row
# gradient so high that weight_loss_rec -> default moved it only 10.4 bars (five more alternatives 11 .. 18), and d loss / d scale at
# scale 1.45 is within 3.9 % = 19.4 bars of its value at 1.8.  With phase2_world 0.43 and scale_init 1.3 the smallest move of any
# output that an alternative changes is 41.6 bars (measured on the CPU, both cases).
ODD = dict(lr=0.0123, weight_loss_rec=0.7, weight_loss_vposer=0.013, weight_contact=0.37, phase1_contact=0.23, phase1_smooth=1.9,
           phase2_world=0.43, phase2_smooth=0.31, scale_init=1.3)
DEFAULTS = dict(lr=0.005, weight_loss_rec=1.0, weight_loss_vposer=0.001, weight_contact=0.1, phase1_contact=0.1, phase1_smooth=1.0,
                phase2_world=1.0, phase2_smooth=0.5, scale_init=1.8)
GRAD_RTOL, GRAD_ATOL = 2e-3, 2e-4          # the mixed-term gradient bar: rtol, atol = 2e-4 max|g| (tests/test_gpu_parity.py _gradient_check; per term and block: tests/gradient_bars.py)
LOG_RTOL = 1e-5                            # ... and its bar for the logged terms (1e-4 for the world term)
FACTOR = 20.0
GRAD_CASES = {"n12": (12, 300, 800, 20, 0), "ragged": (7, 777, 801, 7, 12)}      # n, V, ns, per_part, seed
# The short fit's clip: the gradient cases' clip seed, WITHOUT outlier rows (num_outliers = 0).  Adam turns a gradient into a step of about
# lr whatever its size.  An outlier row has no data term, so the only gradient of its hand columns is the 1e-7 the contact term leaks
# through the pose blend shapes -- below the project's own gradient bar (atol = 2e-4 max|g| = 2e-6), hence free to differ between two
# correct implementations, and Adam makes O(lr) of the difference: with the outlier row in, the host build of the kernels' math parts
# from the oracle by up to 2.6e-2 in the hand columns of that row and its neighbours, the GPU by 8.4e-5, while every other bar holds.
# The "kink-free hand columns" bar presupposes rows with a data term; without outlier rows the hand columns of three CPU implementations
# agree to 7.5e-7 on every clip seed 2 .. 7.  (Outlier rows at the odd settings: the gradient cases, whose clips have one, and the batches,
# whose clips have two each.)  A limitation that remains: three loss terms are L1, and where a residual passes zero within rounding two
# correct implementations part by O(lr) in the other columns; at lr = 0.0123 that happens within 12 iterations
# on clip seeds 4, 5 and 6 of 2 .. 7 (q99 9e-4 .. 4e-3) and not on 2, 3 and 7 (max 4e-7).  That this clip is a well-conditioned one is
# asserted in test_short_fit_yardstick_and_sensitivity_at_the_odd_settings, not assumed.
FIT_CASE = (10, 300, 800, 20, 0, 0)        # ..., num_outliers
FIT_ITERS = 12                             # first_phase2_iter(12) = 10


def alternatives():
    """(name, settings): every swap of two settings of the odd set, every single setting at its default."""
    out = []
    for a, b in itertools.combinations(ODD, 2):
        s = dict(ODD)
        s[a], s[b] = ODD[b], ODD[a]
        out.append((f"{a}<->{b}", s))
    for a in ODD:
        out.append((f"{a}->default", dict(ODD, **{a: DEFAULTS[a]})))
    return out


@functools.lru_cache(maxsize=None)
def make_case(n, V, ns, per_part, seed, num_outliers=None):
    """The models of tests/test_gpu_parity.py _make_fop."""
    bm = synth.make_body_model(V, seed=seed)
    vp = synth.make_vposer(seed=seed + 1)
    clip = synth.make_clip(n, seed=seed + 2, num_outliers=num_outliers)
    scene = synth.make_scene(ns, seed=seed + 3)
    left, right = synth.make_contact_ids(bm.v_template, per_part=per_part, seed=seed + 4)
    return bm, vp, clip, scene, np.concatenate([left, right]), n


def make_oracle(case, settings, dtype, num_iter=500, unit_weights=False):
    bm, vp, clip, scene, vid, n = case
    s = settings
    w = (1.0, 1.0, 1.0) if unit_weights else (s["weight_loss_rec"], s["weight_loss_vposer"], s["weight_contact"])
    return FittingOracle(SMPLXOracle(bm, dtype), VPoserDecoder.from_data(vp, dtype), scene, vid, clip.camerapose_lines, n,
                         init_lr_h=s["lr"], num_iter=num_iter, weight_loss_rec=w[0], weight_loss_vposer=w[1], weight_contact=w[2], dtype=dtype,
                         phase1_contact=s["phase1_contact"], phase1_smooth=s["phase1_smooth"], phase2_world=s["phase2_world"],
                         phase2_smooth=s["phase2_smooth"], scale_init=s["scale_init"])


def perturbation(n):
    """Moves the rows off the data so that |x0 - x| has a definite sign everywhere (as _gradient_check)."""
    return 0.01 * torch.randn((n, 78), generator=torch.Generator().manual_seed(5), dtype=torch.float64)


TERMS = ("rec", "vp", "sm", "con", "ws")


def term_gradients(case, scale_init, dtype=torch.float64, terms=TERMS, as_the_gpu_holds_it=False, body_cls=SMPLXOracle, vposer_cls=VPoserDecoder,
                   edit=None):
    """Values and gradients of the UNWEIGHTED terms (rec, vposer, smoothing, contact, world smoothing) at the perturbed start, each
    term's gradient taken on its own.  -> {"val": {term: float}, "g": {term: (d rows [n,78], d scale, d camera_ext [n,16])}, ...}
    as_the_gpu_holds_it: the start rows, the perturbation, their sum, scale and camera_ext rounded to fp32 before the oracle
    (in `dtype`) sees them -- the state a FittingOP holds after init() and `rows += perturbation.float()`.
    body_cls / vposer_cls: the oracle's models, or subclasses that override tap() (tests/gradient_bars.py).
    edit (with as_the_gpu_holds_it; None: the clip as it is): `edit.clip(body_params [n,75]) -> [n,75]` replaces the clip's rows and
    `edit.rows(x78 fp32 [n,78]) -> [n,78]` the start rows before init() (tests/rotation_edges.py HalfTurnClip)."""
    bm, vp, clip, scene, vid, n = case
    assert edit is None or as_the_gpu_holds_it
    if as_the_gpu_holds_it:
        scale_init = float(np.float32(scale_init))
    s = dict(DEFAULTS, scale_init=scale_init)
    f = FittingOracle(body_cls(bm, dtype), vposer_cls.from_data(vp, dtype), scene, vid, clip.camerapose_lines, n, init_lr_h=s["lr"],
                      weight_loss_rec=1.0, weight_loss_vposer=1.0, weight_contact=1.0, dtype=dtype, scale_init=scale_init)
    body_params = clip.body_params if edit is None else edit.clip(clip.body_params)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(body_params, dtype=torch.float64)).detach()
    idx1, _ = find_outliers(x78.numpy().astype(np.float32))
    if as_the_gpu_holds_it:
        x78 = x78.float() if edit is None else edit.rows(x78.float())
        f.init(x78)
        f.body_rotation_rec.data = (f.body_rotation_rec.data + perturbation(n).float()).to(dtype)       # the sum in fp32, as on the device
        f.camera_ext.data = f.camera_ext.data.float().to(dtype)                                         # (rounded from its fp64 inverse)
        x78 = x78.to(dtype)
    else:
        x78 = x78.to(dtype)
        f.init(x78)
        f.body_rotation_rec.data += perturbation(n).to(dtype)
    l_rec, l_vp, l_con, l_sm, l_ws = f.cal_loss(x78, idx1)
    leaves = (f.body_rotation_rec, f.scale, f.camera_ext)
    out = {"val": {}, "g": {}, "x78": x78, "idx1": idx1, "rows": f.body_rotation_rec.detach().clone(), "cam": f.camera_ext.detach().clone(), "oracle": f}
    for name, l in (("rec", l_rec), ("vp", l_vp), ("sm", l_sm), ("con", l_con), ("ws", l_ws)):
        if name not in terms:
            continue
        g = torch.autograd.grad(l, leaves, retain_graph=True, allow_unused=True)
        g = [torch.zeros_like(p) if gi is None else gi for gi, p in zip(g, leaves)]
        out["val"][name] = float(l.detach())
        out["g"][name] = (g[0].numpy().astype(np.float64), float(g[1]), g[2].numpy().reshape(n, 16).astype(np.float64))
    return out


@functools.lru_cache(maxsize=None)
def oracle_terms(case_key, scale_init):
    """term_gradients of a case of GRAD_CASES in fp64, at the fp64 start."""
    return term_gradients(make_case(*GRAD_CASES[case_key]), scale_init)


def coefficients(s, phase2):
    """The multiplier of every unweighted term in the loss total of a phase (:570 / :582)."""
    if phase2:
        return {"rec": s["weight_loss_rec"], "sm": s["phase2_smooth"], "con": 0.0, "ws": s["phase2_world"], "vp": 0.0}
    return {"rec": s["weight_loss_rec"], "sm": s["phase1_smooth"], "con": s["phase1_contact"] * s["weight_contact"], "ws": 0.0, "vp": 0.0}


def expected(case_key, s, phase2):
    """The oracle's gradient and printed terms for the settings s: the linear combination of the per-term gradients."""
    t = oracle_terms(case_key, s["scale_init"])
    c = coefficients(s, phase2)
    gx = sum(c[k] * t["g"][k][0] for k in c)
    gs = sum(c[k] * t["g"][k][1] for k in c)
    gc = sum(c[k] * t["g"][k][2] for k in c)
    v = t["val"]
    l_rec, l_vp, l_con = s["weight_loss_rec"] * v["rec"], s["weight_loss_vposer"] * v["vp"], s["weight_contact"] * v["con"]
    total = (l_rec + s["phase2_world"] * v["ws"] + s["phase2_smooth"] * v["sm"]) if phase2 else \
        (s["phase1_contact"] * l_con + s["phase1_smooth"] * v["sm"] + l_rec)
    return {"gx": gx, "dscale": gs, "dcam": gc, "logged": np.array([l_rec, l_vp, v["sm"], l_con, v["ws"], total])}


def leaves_bar(alt, ref, rtol, atol, factor=FACTOR):
    """True when `alt` lies at least `factor` bars away from `ref` in at least one entry."""
    alt, ref = np.asarray(alt, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.any(np.abs(alt - ref) >= factor * (atol + rtol * np.abs(ref))))


def gradient_sensitivity_failures(case_key):
    """Every (alternative, phase, output) that the gradient checks of tests/test_gpu_settings.py (and of the host twin below) would NOT
    notice although the alternative changes that output: nothing is ORed over outputs or phases."""
    odd = {p: expected(case_key, ODD, p) for p in (False, True)}
    bad = []
    for name, s in alternatives():
        alt = {p: expected(case_key, s, p) for p in (False, True)}
        changed = {k for k in ODD if s[k] != ODD[k]}
        if changed == {"weight_contact", "phase1_contact"}:
            # the two enter the gradient only as a product: the printed contact term carries weight_contact alone
            a, o = alt[False]["logged"][3], odd[False]["logged"][3]
            if not abs(a - o) >= FACTOR * LOG_RTOL * abs(o):
                bad.append((name, "logged contact", a, o))
            continue
        if changed <= {"lr", "weight_loss_vposer"}:
            # neither reaches a gradient: weight_loss_vposer is printed only (the printed l_vposer pins it), lr is pinned by the
            # first optimiser step (every entry moves by lr within 1e-5 lr)
            seen = ("weight_loss_vposer" in changed and abs(alt[False]["logged"][1] - odd[False]["logged"][1]) >= FACTOR * LOG_RTOL * abs(odd[False]["logged"][1])) \
                or ("lr" in changed and abs(s["lr"] - ODD["lr"]) >= FACTOR * 1e-5 * ODD["lr"])
            if not seen:
                bad.append((name, "printed l_vposer / first step"))
            continue
        # every output the alternative changes at all, in each phase on its own: d rows, d scale (phase 1), d camera_ext (phase 2)
        reached = 0
        for p in (False, True):
            for out in ("gx", "dcam" if p else "dscale"):
                a, o = np.asarray(alt[p][out]), np.asarray(odd[p][out])
                if not np.any(a != o):
                    continue
                reached += 1
                if not leaves_bar(a, o, GRAD_RTOL, 0.0 if out == "dscale" else GRAD_ATOL * np.abs(o).max()):
                    bad.append((name, "phase 2" if p else "phase 1", out))
        if not reached:
            bad.append((name, "reaches no gradient"))
    return bad


@pytest.mark.parametrize("case_key", sorted(GRAD_CASES))
def test_every_swap_and_every_default_moves_the_oracle_gradient_out_of_the_bar(case_key):
    """Part 1's sensitivity condition, from the oracle's per-term gradients alone: 36 swaps and 9 defaults; in each phase, each of
    d rows, d scale (phase 1) and d camera_ext (phase 2) that the alternative changes at all must move 20 x (rtol 2e-3, atol 2e-4
    max|g|) in at least one entry.  The swap weight_contact <-> phase1_contact
    leaves the gradient as it is and must show in the printed contact term; lr and weight_loss_vposer reach no gradient."""
    t = oracle_terms(case_key, ODD["scale_init"])
    for k in ("rec", "sm", "con", "ws"):
        assert np.abs(t["g"][k][0]).max() > 0, k
    assert t["g"]["con"][1] != 0 and np.abs(t["g"]["ws"][2]).max() > 0
    bad = gradient_sensitivity_failures(case_key)
    assert not bad, bad


@pytest.mark.parametrize("phase2", [False, True])
def test_logged_losses_puts_every_weight_in_its_place(phase2, monkeypatch):
    """fitting.logged_losses (device sums -> the printed terms) on sums built from the oracle's unweighted terms: the six printed
    values at the odd settings (whose weights are pairwise distinct, so a swap inside logged_losses changes a value)."""
    from fdcap_amd import fitting
    for name, key in (("PHASE1_CONTACT", "phase1_contact"), ("PHASE1_SMOOTH", "phase1_smooth"), ("PHASE2_WORLD", "phase2_world"),
                      ("PHASE2_SMOOTH", "phase2_smooth")):
        monkeypatch.setattr(fitting, name, ODD[key])
    n, _, _, per_part, _ = GRAD_CASES["n12"]
    nc = 2 * per_part
    v = oracle_terms("n12", ODD["scale_init"])["val"]
    sums = np.array([v["rec"] * n * 78, v["vp"] * n * 32, v["sm"] * (n - 2) * 78, v["con"] * n * nc, v["ws"] * (n - 1) * 69, 0, 0, 0])
    got = np.array(fitting.logged_losses(sums, n, nc, ODD["weight_loss_rec"], ODD["weight_loss_vposer"], ODD["weight_contact"], phase2))
    want = expected("n12", ODD, phase2)["logged"]
    np.testing.assert_allclose(got, want, rtol=1e-12)


ROW_SUMS = np.array([41.7, 3.9, 0.83, 17.3, 5.1, 2.2e3, 0.061, 9.4])       # losses_d of one logged iteration: any positive sums


@pytest.mark.parametrize("n", [1, 2, 3, 300])
def test_local2_losses_is_the_second_loops_printed_row(n, recwarn):
    """fitting.local2_losses (mode 'local''s second loop, global_optimization.py:404-429, :547-552): the means over an n-frame clip
    of V vertices from the device's sums, each term as written out here (the divisor n - 2 as it is: -1 for one frame); a mean
    over nothing (n = 2) is inf, NaN for a zero sum, position for position, and nothing warns."""
    from fdcap_amd import fitting
    V, w_rec = 217, ODD["weight_loss_rec"]
    for s in (ROW_SUMS, np.where(np.arange(8) == 2, 0.0, ROW_SUMS)):
        with np.errstate(divide="ignore", invalid="ignore"):
            nf = np.float64(n)
            l_rec = w_rec * s[0] / (nf * 78)                  # weight_loss_rec * mean |x - data| over [n,78]
            l_loc = s[2] / ((nf - 2) * 78)                    # mean of the second differences of the rows [n-2,78]
            l_sm = s[5] / ((nf - 2) * (3 * V))                # mean of the second differences of the world vertices [n-2,V,3] (:404-405)
            l_cs = s[6]                                       # the two contact-smoothing means (:429), divided on the device
            want = [l_rec, l_loc, l_sm, l_cs, l_sm * 1.0 + l_loc + l_rec + l_cs]      # (:547)
        got = fitting.local2_losses(s, n, V, w_rec)
        assert len(got) == 5
        np.testing.assert_array_equal(np.array(got, dtype=np.float64), np.array(want, dtype=np.float64))
        assert all(np.isfinite(got)) == (n != 2)
    assert not [w for w in recwarn.list if issubclass(w.category, RuntimeWarning)]


@pytest.mark.parametrize("n", [1, 2, 3, 300])
def test_dct2_losses_is_the_second_phases_printed_row(n, recwarn):
    """fitting.dct2_losses (mode 'dct''s second phase, :620-626) at the odd weights: each term as written out here, loss_smoothing NaN
    below three frames, total = loss_dct*0.0001 + loss_rec*0.5 + loss_contact*0.1."""
    from fdcap_amd import fitting
    assert fitting.DCT_PHASE2 == (0.0001, 0.5, 0.1)
    s, W, nc = ROW_SUMS, 5, 16
    w_rec, w_vp, w_con = ODD["weight_loss_rec"], ODD["weight_loss_vposer"], ODD["weight_contact"]
    l_rec = w_rec * s[0] / (n * 78)
    l_vp = w_vp * s[1] / (n * 32)
    l_sm = s[2] / ((n - 2) * 78) if n >= 3 else float("nan")
    l_con = w_con * s[3] / (n * nc)
    l_dct = s[7] / (69 * W)                                    # mean over [W,23,3] trajectories
    want = [l_rec, l_vp, l_sm, l_con, l_dct, 0.0001 * l_dct + 0.5 * l_rec + 0.1 * l_con]
    got = fitting.dct2_losses(s, n, W, nc, w_rec, w_vp, w_con)
    assert len(got) == 6 and np.isnan(got[2]) == (n < 3)
    np.testing.assert_array_equal(np.array(got, dtype=np.float64), np.array(want, dtype=np.float64))
    # no contact vertices: the mean runs over one, as in logged_losses
    assert fitting.dct2_losses(s, n, W, 0, w_rec, w_vp, w_con)[3] == w_con * s[3] / n
    assert not [w for w in recwarn.list if issubclass(w.category, RuntimeWarning)]


def test_dct_first_phase2_iter_is_the_one_place_of_the_split():
    from fdcap_amd.fitting import dct_first_phase2_iter
    for k in range(1, 401):
        assert dct_first_phase2_iter(k) == int(np.ceil(k * 0.95 - 1e-9)), k
    assert dct_first_phase2_iter(200) == 190 and dct_first_phase2_iter(40) == 38 and dct_first_phase2_iter(10000) == 9500


def test_fitlog_appends_a_row_of_logged_losses():
    from fdcap_amd.fitting import FitLog
    log = FitLog()
    log.append(3, (1.0, 2.0, 3.0, 4.0, 5.0, 6.0))
    log.append(7, (1.5, 2.5, 3.5, 4.5, 5.5, 6.5))
    assert log == FitLog([3, 7], [1.0, 1.5], [2.0, 2.5], [3.0, 3.5], [4.0, 4.5], [5.0, 5.5], [6.0, 6.5])
    assert FitLog().iters is not FitLog().iters


# ---- the host twin: the kernels' math compiled for the host ---------------------------------------------------------------------
@pytest.mark.parametrize("phase2", [False, True])
def test_host_build_of_the_kernels_math_at_the_odd_settings_matches_autograd(phase2):
    """tests/test_host_math.py test_hand_derived_gradients_match_autograd at the odd settings (its bar): HostPipeline.backward
    mirrors fdcap_opt_backward's launches, the expected gradient is the odd combination of the fp64 per-term gradients."""
    from tests.host_pipeline import HostPipeline, f32
    case = make_case(*GRAD_CASES["n12"])
    bm, vp, clip, scene, vid, n = case
    t = oracle_terms("n12", ODD["scale_init"])
    want = expected("n12", ODD, phase2)
    hp = HostPipeline(bm, vp, scene, vid)
    mask = np.ones(n, np.float32)
    mask[t["idx1"]] = 0
    cfg = {k: ODD[k] for k in ("weight_loss_rec", "weight_contact", "phase1_contact", "phase1_smooth", "phase2_world", "phase2_smooth")}
    out = hp.backward(f32(t["rows"].numpy()), f32(t["x78"].numpy()), mask, f32(t["cam"].numpy().reshape(n, 16)), ODD["scale_init"], n, 0, 0, n, phase2, cfg)
    gx = want["gx"]
    np.testing.assert_allclose(out["dX"], gx, rtol=GRAD_RTOL, atol=GRAD_ATOL * np.abs(gx).max())
    if phase2:
        gc = want["dcam"].reshape(n, 4, 4)
        np.testing.assert_allclose(out["dCAM"][:, :3], gc[:, :3], rtol=GRAD_RTOL, atol=GRAD_ATOL * np.abs(gc).max())
        assert np.all(out["dCAM"][:, 3] == 0) and np.all(gc[:, 3] == 0)
    else:
        np.testing.assert_allclose(out["dscale"], want["dscale"], rtol=GRAD_RTOL)
    s, lg = out["losses"], want["logged"]
    np.testing.assert_allclose(ODD["weight_loss_rec"] * s[0] / (n * 78), lg[0], rtol=LOG_RTOL)
    np.testing.assert_allclose(ODD["weight_loss_vposer"] * s[1] / (n * 32), lg[1], rtol=LOG_RTOL)
    np.testing.assert_allclose(s[2] / ((n - 2) * 78), lg[2], rtol=LOG_RTOL)
    np.testing.assert_allclose(s[4] / ((n - 1) * 69), lg[4], rtol=1e-4)
    if not phase2:
        np.testing.assert_allclose(ODD["weight_contact"] * s[3] / (n * len(vid)), lg[3], rtol=LOG_RTOL)


# ---- the oracle's new keywords ----------------------------------------------------------------------------------------------------
class _OracleBeforeTheKeywords(FittingOracle):
    """step() with the reference's constants written out, as oracle/fitting.py had it before the keywords existed."""

    def step(self, ii, body_data_rotation, idx1):
        self.optimizer.zero_grad(set_to_none=not self.legacy_zero_grad)
        l_rec, l_vp, l_con, l_sm, l_ws = self.cal_loss(body_data_rotation, idx1)
        if ii < self.num_iter * self.phase_split:
            self.camera_ext.requires_grad = False
            self.scale.requires_grad = True
            self.body_rotation_rec.requires_grad = True
            loss = l_con * 0.1 + l_sm * 1.0 + l_rec
        else:
            self.camera_ext.requires_grad = True
            self.scale.requires_grad = False
            self.body_rotation_rec.requires_grad = True
            loss = l_rec + l_ws * 1 + l_sm * 0.5
        self.loss_log.append([float(v.detach()) for v in (l_rec, l_vp, l_sm, l_con, l_ws, loss)])
        loss.backward()
        self.optimizer.step()
        return loss


def test_the_oracles_new_keywords_at_their_defaults_change_no_bit():
    """5 iterations (phase 2 from iteration 4): parameters, scale, camera_ext and every printed value, bit for bit."""
    bm, vp, clip, scene, vid, n = make_case(*FIT_CASE)
    outs = []
    for cls, kw in ((_OracleBeforeTheKeywords, {}), (FittingOracle, {}),
                    (FittingOracle, dict(phase1_contact=0.1, phase1_smooth=1.0, phase2_world=1.0, phase2_smooth=0.5, scale_init=1.8))):
        f = cls(SMPLXOracle(bm), VPoserDecoder.from_data(vp), scene, vid, clip.camerapose_lines, n, num_iter=5, **kw)
        body, scale, cam = f.fitting(torch.tensor(clip.body_params))
        assert float(f.scale.detach()) != 1.8 and not torch.equal(cam, f.camera_ext.detach() * 0)
        outs.append((body.numpy(), np.asarray(scale), cam.numpy(), np.array(f.loss_log)))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert a.dtype == b.dtype and np.array_equal(a, b)


# ---- a short fit: yardstick and sensitivity ------------------------------------------------------------------------------------------
# The project's bars for a short fit against the fp32 oracle (tests/test_gpu_general_k.py, tests/test_gpu_parity.py): quantiles of
# |body - oracle|, its maximum (three sign flips of one entry: proportional to the step, 6 lr), the kink-free hand columns, scale,
# and the first two printed contact values (before any sign flip can act).  l_vposer: the same 2e-6 on the first two printed values
# (a mean of order 4e-3 in fp32; this file's addition, so that weight_loss_vposer shows in the fit too).
FIT_BARS = dict(q50=1e-6, q90=1e-4, q99=3e-3, max=6 * ODD["lr"], hands=2e-6, scale=1e-4, contact2=2e-6, vposer2=2e-6)


@functools.lru_cache(maxsize=None)
def oracle_fit(settings_items, dtype):
    s = dict(settings_items)
    case = make_case(*FIT_CASE)
    f = make_oracle(case, s, dtype, num_iter=FIT_ITERS)
    body, scale, cam = f.fitting(torch.tensor(case[2].body_params))
    return body.numpy().astype(np.float64), float(scale), cam.numpy().astype(np.float64), np.array(f.loss_log, dtype=np.float64)


def fit_figures(got, want):
    """(body [n,75], scale, camera_ext, log [iters, 6]) x 2 -> the figures FIT_BARS bounds."""
    err = np.abs(np.asarray(got[0], dtype=np.float64) - want[0])
    q50, q90, q99 = np.quantile(err, [0.5, 0.9, 0.99])
    lg, lw = np.asarray(got[3], dtype=np.float64), want[3]
    return dict(q50=q50, q90=q90, q99=q99, max=err.max(), hands=err[:, 48:72].max(), scale=abs(float(got[1]) - want[1]),
                contact2=np.abs(lg[:2, 3] - lw[:2, 3]).max(), vposer2=np.abs(lg[:2, 1] - lw[:2, 1]).max())


def fit_violations(got, want, bars=None):
    bars = FIT_BARS if bars is None else bars
    fig = fit_figures(got, want)
    return {k: (fig[k], bars[k]) for k in bars if not fig[k] <= bars[k]}


def host_fit(case, s, num_iter):
    """The loop of fitting.FittingOP.fitting on the host build of the kernels' math (tests/test_host_math.py _host_fit, with the
    settings as arguments).  -> (body [n,75], scale)"""
    from fdcap_amd.fitting import first_phase2_iter
    from fdcap_amd.io import read_camerapose
    from tests.host_pipeline import HostPipeline, P as ptr, f32
    bm, vp, clip, scene, vid, n = case
    hp = HostPipeline(bm, vp, scene, vid)
    x78 = np.zeros((n, 78), np.float32)
    hp.lib.h_75_to_78(ptr(f32(clip.body_params)), n, ptr(x78))
    idx1, pos = find_outliers(x78)
    X = x78.copy()
    if idx1.size:
        X[idx1] = x78[pos]
    mask = np.ones(n, np.float32)
    mask[idx1] = 0
    CAM = f32(read_camerapose(clip.camerapose_lines).reshape(n, 16)).copy()
    scale = np.array([s["scale_init"]], np.float32)
    st = {k: np.zeros_like(v) for k, v in (("mX", X), ("vX", X), ("mC", CAM), ("vC", CAM), ("mS", scale), ("vS", scale))}
    P_, lr = first_phase2_iter(num_iter), s["lr"]
    for ii in range(num_iter):
        out = hp.backward(X, x78, mask, CAM, float(scale[0]), n, 0, 0, n, ii >= P_, s)
        hp.adam(X, st["mX"], st["vX"], out["dX"], lr, ii + 1)
        if ii < P_:
            hp.adam(scale, st["mS"], st["vS"], np.array([out["dscale"]], np.float32), lr, ii + 1)
        if ii >= P_ + 1:
            hp.adam(CAM, st["mC"], st["vC"], f32(out["dCAM"].reshape(n, 16)), lr, ii - P_)
    body = np.zeros((n, 75), np.float32)
    hp.lib.h_78_to_75(ptr(X), n, ptr(body))
    return body, float(scale[0])


def test_short_fit_yardstick_and_sensitivity_at_the_odd_settings():
    """Part 5 on the CPU.  Yardsticks at the odd settings, 10 frames, 12 iterations -- what correct implementations differ by: the fp64
    oracle against the fp32 oracle, and the host build of the kernels' math (another order of operations) against the fp32 oracle.
    Measured on the CPU (x86-64, torch 2 CPU kernels), fp64 / host build: q50 1.3e-8 / 0, q90 6.9e-8 / 1.5e-8, q99 2.1e-7 / 6.0e-8,
    max 2.8e-7 / 2.4e-7, hands 5.7e-8 / 3.0e-8, scale 2.2e-9 / 0, first two printed contact values 9.4e-9, l_vposer 2.5e-10.  Every
    bar of FIT_BARS -- the project's own: q50 1e-6, q90 1e-4, q99 3e-3, max 6 lr, hands 2e-6, scale 1e-4 -- is at least 3 x both
    figures (asserted), so all of them stay.
    Sensitivity: with any one setting at its default the fp32 oracle's fit leaves the bars around the odd-set fit."""
    odd32 = oracle_fit(tuple(ODD.items()), torch.float32)
    odd64 = oracle_fit(tuple(ODD.items()), torch.float64)
    yard = fit_figures(odd32, odd64)
    print("short-fit yardstick (fp32 oracle vs fp64 oracle, odd settings):", {k: float(v) for k, v in yard.items()})
    for k, bar in FIT_BARS.items():
        assert bar >= 3 * yard[k], (k, bar, yard[k])
    hb, hs = host_fit(make_case(*FIT_CASE), ODD, FIT_ITERS)
    herr = np.abs(hb - odd32[0])
    host = dict(zip(("q50", "q90", "q99"), np.quantile(herr, [0.5, 0.9, 0.99])), max=herr.max(), hands=herr[:, 48:72].max(), scale=abs(hs - odd32[1]))
    print("short-fit yardstick (host build of the kernels' math vs fp32 oracle):", {k: float(v) for k, v in host.items()})
    for k, v in host.items():
        assert FIT_BARS[k] >= 3 * v, (k, FIT_BARS[k], v)
    for name in ODD:
        alt = oracle_fit(tuple(dict(ODD, **{name: DEFAULTS[name]}).items()), torch.float32)
        v = fit_violations(alt, odd32)
        print(f"{name} -> default leaves the bars at", sorted(v))
        assert v, name
    # scale_init on its own: the world vertices / joints before the first step (the GPU test's bar: 3e-5) and the first printed contact term
    a, b = oracle_terms("n12", ODD["scale_init"]), oracle_terms("n12", DEFAULTS["scale_init"])
    assert abs(a["val"]["con"] - b["val"]["con"]) * ODD["weight_contact"] >= FACTOR * FIT_BARS["contact2"]
    ja, jb = forward_world(ODD["scale_init"]), forward_world(DEFAULTS["scale_init"])
    assert leaves_bar(jb[0], ja[0], 0.0, 3e-5) and leaves_bar(jb[1], ja[1], 0.0, 3e-5)


@functools.lru_cache(maxsize=None)
def forward_world(scale_init, dtype=torch.float32):
    """World contact vertices and joints of the fit case's start (before any step)."""
    case = make_case(*FIT_CASE)
    f = make_oracle(case, dict(ODD, scale_init=scale_init), dtype)
    f.init(rotrepr.convert_to_6D_rot(torch.tensor(case[2].body_params, dtype=dtype)).detach())
    with torch.no_grad():
        _, verts, joints = f.forward_world()
    return verts[:, case[4]].numpy(), joints.numpy()


# ---- the 2D inner fit ---------------------------------------------------------------------------------------------------------------
FIT2D_STAGE = dict(fx=710.0, fy=655.0, cx=612.0, cy=377.0, rho=63.0, w_data=1.7, w_pose=3.1, w_shape=6.3, w_hand=2.2)
# The same stage with a data weight so small (w_data^2 = 9e-6: the data gradient shrinks from 2e5 to about 1) that the priors' gradient
# 2 w^2 x dominates every column it reaches: the second evaluation, which pins w_pose, w_shape and w_hand in the GRADIENT of each
# of their column blocks under the whole-gradient bar (at FIT2D_STAGE the data gradient hides them under atol = 40).
FIT2D_PRIOR_STAGE = dict(FIT2D_STAGE, w_data=0.003)
FIT2D_SUM_RTOL = 2e-5


@functools.lru_cache(maxsize=None)
def fit2d_case():
    """tests/test_gpu_innerfit.py _case(16, 7) with a third of the detected keypoints displaced by +-150 px in u and v: GMoF
    (rho = 63) is then past its bend for those and on its quadratic part for the rest, so rho is observed."""
    from tests.test_gpu_innerfit import _case
    n = 16
    bm, vp, gt, init, kp = _case(n, 7)
    rng = np.random.Generator(np.random.PCG64(1234))
    moved = (rng.random((n, 23)) < 1.0 / 3.0) & (kp[..., 2] > 0)
    kp = kp.copy()
    kp[..., :2] += (150.0 * moved[..., None] * rng.choice([-1.0, 1.0], (n, 23, 2))).astype(np.float32)
    return bm, vp, init, kp, n


def fit2d_oracle(stage, rows78, w_data_squared=True):
    """fp64 data / prior sums and d (data + prior) / d rows of the inner fit's objective at rows78 for a stage (dict as FIT2D_STAGE)."""
    bm, vp, init, kp, n = fit2d_case()
    dt = torch.float64
    orc = InnerFitOracle(SMPLXOracle(bm, dtype=dt), VPoserDecoder.from_data(vp, dtype=dt), intrinsics=(stage["fx"], stage["fy"], stage["cx"], stage["cy"]),
                         rho=stage["rho"], dtype=dt)
    x = torch.as_tensor(rows78, dtype=dt).clone().requires_grad_(True)
    w_data = stage["w_data"] if w_data_squared else stage["w_data"] ** 0.5
    data, prior = orc.loss(x, torch.tensor(kp, dtype=dt), (w_data, stage["w_pose"], stage["w_shape"], stage["w_hand"]))
    (data + prior).backward()
    with torch.no_grad():
        res = (torch.tensor(kp[..., :2], dtype=dt) - orc.project(orc.joints_cam(x))).numpy()
    return float(data.detach()), float(prior.detach()), x.grad.numpy(), res


def fit2d_alternatives():
    s = FIT2D_STAGE
    return [("fx<->fy", dict(s, fx=s["fy"], fy=s["fx"]), True), ("w_pose<->w_hand", dict(s, w_pose=s["w_hand"], w_hand=s["w_pose"]), True),
            ("w_data unsquared", s, False), ("rho=100", dict(s, rho=100.0), True)]


HANDS = slice(51, 75)                      # the hand PCA columns of a row: joints 0..22 do not depend on them, so their gradient is the prior's alone


def hand_block_bar(g):
    return GRAD_ATOL * np.abs(g[:, HANDS]).max()


def fit2d_check_case(rows78):
    """Asserts what makes the case a test of rho, and that each alternative stage moves the oracle's result out of the bars.
    fx <-> fy, w_data unsquared and rho = 100 move the whole gradient 20 bars.  w_pose <-> w_hand does not: with a third of the
    keypoints 150 px off, max|g| is 2e5 (the translation columns) and atol = 2e-4 max|g| = 40 hides every prior gradient (at most
    2 w^2 |x| = 10).  That swap is seen by the prior sum (rtol 2e-5) and by the hand columns under the same bar taken over
    their own block (rtol 2e-3, atol 2e-4 max|g[:, 51:75]|), which tests/test_gpu_settings.py therefore asserts as well."""
    bm, vp, init, kp, n = fit2d_case()
    data, prior, g, res = fit2d_oracle(FIT2D_STAGE, rows78)
    r = np.abs(res[kp[..., 2] > 0]).reshape(-1)
    assert (r > FIT2D_STAGE["rho"]).mean() >= 0.25 and (r < FIT2D_STAGE["rho"] / 2).mean() >= 0.25, ((r > 63).mean(), (r < 31.5).mean())
    assert np.abs(g[:, HANDS]).max() > 0
    for name, stage, squared in fit2d_alternatives():
        da, pa, ga, _ = fit2d_oracle(stage, rows78, squared)
        whole = leaves_bar(ga, g, GRAD_RTOL, GRAD_ATOL * np.abs(g).max())
        hands = leaves_bar(ga[:, HANDS], g[:, HANDS], GRAD_RTOL, hand_block_bar(g))
        sums = leaves_bar([da, pa], [data, prior], FIT2D_SUM_RTOL, 0.0)
        assert (hands and sums) if name == "w_pose<->w_hand" else whole, (name, whole, hands, sums)
    return data, prior, g


LATENT, BETAS = slice(19, 51), slice(9, 19)


def fit2d_check_prior_case(rows78):
    """At FIT2D_PRIOR_STAGE every swap among w_pose, w_shape and w_hand moves the oracle's gradient 20 whole-gradient bars in EACH of
    the two column blocks whose weight it changes (latent 19:51, betas 9:19, hands 51:75).  -> (data, prior, gradient)"""
    st = FIT2D_PRIOR_STAGE
    data, prior, g, _ = fit2d_oracle(st, rows78)
    atol = GRAD_ATOL * np.abs(g).max()
    blocks = {"w_pose": LATENT, "w_shape": BETAS, "w_hand": HANDS}
    for a, b in itertools.combinations(blocks, 2):
        _, _, ga, _ = fit2d_oracle(dict(st, **{a: st[b], b: st[a]}), rows78)
        for k in (a, b):
            assert leaves_bar(ga[:, blocks[k]], g[:, blocks[k]], GRAD_RTOL, atol), (a, b, k)
    return data, prior, g


def test_inner_fit_case_observes_rho_and_every_stage_setting():
    """Part 7's conditions at the evaluation point (the 6D form of the start rows): at least a quarter of the detected residuals
    beyond rho, a quarter below rho / 2; fx <-> fy, w_data unsquared and rho = 100 each move the gradient 20 bars, w_pose <-> w_hand the
    prior sum and the hand columns (fit2d_check_case says why)."""
    bm, vp, init, kp, n = fit2d_case()
    rows = rotrepr.convert_to_6D_rot(torch.tensor(init, dtype=torch.float64)).numpy()
    fit2d_check_case(rows)
    fit2d_check_prior_case(rows)


# ---- the per-frame smoother -----------------------------------------------------------------------------------------------------------
SMOOTHER = dict(init_lr_h=0.037, num_iter=17, weight_loss_rec=0.6, weight_loss_vposer=0.02)
SMOOTHER_BAR = 1e-5


def smoother_clip():
    return synth.make_clip(40, seed=41, num_outliers=2).body_params


def test_smoother_yardstick_and_sensitivity():
    """Part 8 on the CPU.  Yardstick: the fp64 smoother oracle against the fp32 one at (lr 0.037, 17 iterations, weights 0.6 / 0.02)
    on the 40-frame clip: measured max 1.72e-6 on the CPU (x86-64, torch 2 CPU kernels), so the project's bar 1e-5 is 5.8 x the yardstick and stays.
    Sensitivity: the oracle at the defaults (lr 0.1, 50 iterations, 1 / 0.001) is more than 100 bars away, and so is it with any single
    one of the four values at its default."""
    rows = smoother_clip()
    odd32 = SmootherOracle(**SMOOTHER).fitting_clip(rows).numpy().astype(np.float64)
    odd64 = SmootherOracle(**SMOOTHER, dtype=torch.float64).fitting_clip(rows).numpy()
    yard = np.abs(odd32 - odd64).max()
    print("smoother yardstick (fp32 oracle vs fp64 oracle):", yard)
    assert SMOOTHER_BAR >= 3 * yard
    dflt = SmootherOracle().fitting_clip(rows).numpy()
    assert np.abs(dflt - odd32).max() > 100 * SMOOTHER_BAR
    base = dict(init_lr_h=0.1, num_iter=50, weight_loss_rec=1.0, weight_loss_vposer=0.001)
    for k in SMOOTHER:
        one = SmootherOracle(**dict(SMOOTHER, **{k: base[k]})).fitting_clip(rows).numpy()
        print(f"smoother, {k} at its default: max difference", np.abs(one - odd32).max())
        assert np.abs(one - odd32).max() > 100 * SMOOTHER_BAR, k
