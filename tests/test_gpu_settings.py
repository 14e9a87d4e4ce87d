"""The kernels at loss weights, step sizes and intrinsics away from their defaults (tests/test_settings_cpu.py: the odd set ODD, the
cases, the oracle's per-term gradients, the bars, and -- evaluated there without a GPU -- the sensitivity conditions that keep
these tests from passing with two settings wired to each other's place).

  1  gradient and printed terms of both phases against fp64 autograd (the odd combination of the per-term gradients);
  2  weight_loss_vposer is printed only;
  3  the zero switches (phase1_contact, phase1_smooth, phase2_world, phase2_smooth, weight_loss_rec = 0): gradient, exact semantics
     of `0 * term` under autograd, and the same bytes whichever way the iterations are issued, pose trim on and off;
  4  the optimiser step against Adam in fp64 on the GPU's own gradients, the three step counters, and lr itself;
  5  a short fit end to end against the fp32 oracle;
  6  batches: the weights read from the clip table on the device;
  7  the 2D inner fit at odd intrinsics, rho and stage weights;
  8  the per-frame smoother at odd lr / iterations / weights.

The phase weights and SCALE_INIT are module constants of fdcap_amd.fitting, read when an optimiser is created and when a log row is
formed: the tests monkeypatch them; lr and the lossconfig weights go through the constructor's dictionaries."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
import tests.test_settings_cpu as sc
from fdcap_amd import capi, synth
from fdcap_amd import fitting as fit_mod
from fdcap_amd.fitting import ClipBatchFitter, FittingOP, first_phase2_iter, is_logging_iteration
from fdcap_amd.innerfit import InnerFitOP
from fdcap_amd.io import read_camerapose
from fdcap_amd.smoother import FittingOP as SmootherOP
from oracle.smoother import SmootherOracle

pytestmark = pytest.mark.gpu
ODD = sc.ODD
BIG = 10 ** 6
ZERO_CASES = ("phase1_contact", "phase1_smooth", "phase2_world", "phase2_smooth", "weight_loss_rec")


def _patch(monkeypatch, s):
    for name, key in (("PHASE1_CONTACT", "phase1_contact"), ("PHASE1_SMOOTH", "phase1_smooth"), ("PHASE2_WORLD", "phase2_world"),
                      ("PHASE2_SMOOTH", "phase2_smooth"), ("SCALE_INIT", "scale_init")):
        monkeypatch.setattr(fit_mod, name, s[key])


def _configs(s, num_iter):
    return ({"num_iter": num_iter, "init_lr_h": s["lr"]},
            {"weight_loss_rec": s["weight_loss_rec"], "weight_loss_vposer": s["weight_loss_vposer"], "weight_contact": s["weight_contact"]})


def _fop(monkeypatch, case, s, num_iter=500):
    _patch(monkeypatch, s)
    bm, vp, clip, scene, vid, n = case
    return FittingOP(*_configs(s, num_iter), n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                     camera_ext=read_camerapose(clip.camerapose_lines))


def _init_from_clip(fop, clip):
    n = clip.body_params.shape[0]
    x78 = torch.empty(n, 78, device="cuda")
    capi.check(fop.ctx.lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(clip.body_params).cuda()), n, capi.dptr(x78), capi.current_stream()), "75->78")
    fop.init(x78)


def _init_perturbed(fop, case_key, s):
    """The state of sc.oracle_terms on the GPU: the fp32 start rows + the same perturbation."""
    t = sc.oracle_terms(case_key, s["scale_init"])
    n = t["rows"].shape[0]
    fop.init(torch.tensor(t["x78"].numpy(), dtype=torch.float32).cuda())
    fop._rows_x[2:2 + n] += sc.perturbation(n).float().cuda()
    return n


def _backward(fop, n, ii, P, log_terms):
    lib, h = fop.ctx.lib, fop.ctx.handle
    capi.check(lib.fdcap_opt_backward(h, ii, P, log_terms, capi.current_stream()), "backward")
    dx = torch.empty(n, 78, device="cuda")
    dcam = torch.empty(n, 16, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), capi.dptr(dcam), capi.current_stream()), "grads")
    torch.cuda.synchronize()
    return dx.cpu().numpy(), dcam.cpu().numpy()


def _step(fop, ii, P):
    capi.check(fop.ctx.lib.fdcap_opt_step(fop.ctx.handle, ii, P, capi.current_stream()), "step")
    torch.cuda.synchronize()


def _state(fop, n):
    capi.check(fop.ctx.lib.fdcap_opt_sync(fop.ctx.handle, capi.current_stream()), "sync")
    torch.cuda.synchronize()
    return {"rows": fop._rows_x[2:2 + n].cpu().numpy(), "cam": fop._rows_cam[2:2 + n].cpu().numpy(), "scale": fop._scale.cpu().numpy()}


def _check_gradient(got_dx, got_dcam, got_dscale, want, phase2):
    gx = want["gx"]
    np.testing.assert_allclose(got_dx, gx, rtol=sc.GRAD_RTOL, atol=sc.GRAD_ATOL * np.abs(gx).max())
    if phase2:
        gc = want["dcam"]
        np.testing.assert_allclose(got_dcam, gc, rtol=sc.GRAD_RTOL, atol=sc.GRAD_ATOL * np.abs(gc).max())
    else:
        np.testing.assert_allclose(got_dscale, want["dscale"], rtol=sc.GRAD_RTOL, atol=0)


def _check_logged(fop, s, n, want, phase2, only=None):
    """The device sums through fitting.logged_losses at the settings s: rtol 1e-5 per printed term, 1e-4 for the world term; the
    phase-2 total contains phase2_world * l_ws and gets the bar its terms imply."""
    got = np.array(fit_mod.logged_losses(fop._losses.cpu().numpy(), n, fop.ctx.num_contact, s["weight_loss_rec"], s["weight_loss_vposer"],
                                         s["weight_contact"], phase2), dtype=np.float64)
    lg = want["logged"]
    print("logged (phase 2)" if phase2 else "logged (phase 1)", got, lg)
    for k in (range(5) if only is None else only):
        np.testing.assert_allclose(got[k], lg[k], rtol=1e-4 if k == 4 else sc.LOG_RTOL, err_msg=f"term {k}")
    if only is None:
        atol = 1e-4 * s["phase2_world"] * abs(lg[4]) if phase2 else 0.0
        np.testing.assert_allclose(got[5], lg[5], rtol=sc.LOG_RTOL, atol=atol, err_msg="total")
    return got


# ---- 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase2", [False, True])
@pytest.mark.parametrize("case_key", ["n12", "ragged"])
def test_gradient_and_printed_terms_at_the_odd_settings_match_autograd(case_key, phase2, monkeypatch):
    """n = 12, V = 300, 800 scene points, 2 x 20 contact vertices, and the ragged n = 7, V = 777, 801, 2 x 7.  Expected: the odd
    combination of the gradients of the four unweighted terms, each taken on its own from the fp64 oracle.  The sensitivity
    condition (tests/test_settings_cpu.py gradient_sensitivity_failures) is asserted here again, from the same per-term gradients."""
    assert not sc.gradient_sensitivity_failures(case_key)
    fop = _fop(monkeypatch, sc.make_case(*sc.GRAD_CASES[case_key]), ODD)
    n = _init_perturbed(fop, case_key, ODD)
    assert float(fop._scale.cpu()) == np.float32(ODD["scale_init"])
    dx, dcam = _backward(fop, n, 5, 0 if phase2 else BIG, 1)
    want = sc.expected(case_key, ODD, phase2)
    _check_gradient(dx, dcam, float(fop._dscale.cpu()), want, phase2)
    _check_logged(fop, ODD, n, want, phase2)
    fop.close()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------------
def test_weight_loss_vposer_is_printed_only(monkeypatch):
    """0.013 -> 0.5: no bit of either phase's gradient, no bit of a 4-iteration fit; the printed l_vposer scales by the ratio."""
    res = []
    case = sc.make_case(*sc.FIT_CASE)
    for wv in (ODD["weight_loss_vposer"], 0.5):
        s = dict(ODD, weight_loss_vposer=wv)
        fop = _fop(monkeypatch, sc.make_case(*sc.GRAD_CASES["n12"]), s)
        n = _init_perturbed(fop, "n12", s)
        grads = []
        for phase2 in (False, True):
            dx, dcam = _backward(fop, n, 5, 0 if phase2 else BIG, 1)
            grads += [dx, dcam if phase2 else fop._dscale.cpu().numpy()]
        fop.close()
        fop = _fop(monkeypatch, case, s, num_iter=4)
        body, scale, cam = fop.fitting(torch.tensor(case[2].body_params).cuda(), "global", log_every=1)
        res.append((grads, body.cpu().numpy(), np.float32(scale), cam.cpu().numpy(), dataclasses.asdict(fop.log)))
        fop.close()
    a, b = res
    for x, y in zip(a[0], b[0]):
        assert np.abs(x).max() > 0 and x.tobytes() == y.tobytes()
    for k in (1, 2, 3):
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
    for k in a[4]:
        if k != "l_vposer":
            assert np.array_equal(np.array(a[4][k], dtype=np.float64), np.array(b[4][k], dtype=np.float64), equal_nan=True), k
    la, lb = np.array(a[4]["l_vposer"]), np.array(b[4]["l_vposer"])
    assert len(la) == 4 and np.all(la > 0)
    np.testing.assert_allclose(lb / 0.5, la / ODD["weight_loss_vposer"], rtol=1e-15)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ZERO_CASES)
def test_a_zero_weight_gives_the_gradient_and_the_semantics_of_zero_times_the_term(which, monkeypatch):
    """One setting zero, the others odd; the contact set and the scene stay.  In the phase(s) the setting belongs to the gradient
    is the oracle's, whose total contains 0 * term.  phase1_contact = 0: d loss / d scale is exactly 0, `scale` keeps its bits over
    three phase-1 steps (Adam on an exactly zero gradient from zero moments does not move) and a logging iteration still prints
    the oracle's contact term.  phase2_world = 0: d loss / d camera_ext is all zeros and camera_ext keeps its bits over three steps
    at ii > P."""
    s = dict(ODD, **{which: 0.0})
    phases = {"phase1_contact": (False,), "phase1_smooth": (False,), "phase2_world": (True,), "phase2_smooth": (True,), "weight_loss_rec": (False, True)}[which]
    for phase2 in phases:
        fop = _fop(monkeypatch, sc.make_case(*sc.GRAD_CASES["n12"]), s)
        n = _init_perturbed(fop, "n12", s)
        P = 0 if phase2 else BIG
        dx, dcam = _backward(fop, n, 5, P, 1)
        want = sc.expected("n12", s, phase2)
        assert np.abs(want["gx"]).max() > 0
        _check_gradient(dx, dcam, float(fop._dscale.cpu()), want, phase2)
        _check_logged(fop, s, n, want, phase2)
        if which == "phase1_contact":
            assert want["dscale"] == 0.0 and want["logged"][3] > 0
            assert float(fop._dscale.cpu()) == 0.0
            before = _state(fop, n)
            for ii in range(3):
                _backward(fop, n, ii, P, 0)
                _step(fop, ii, P)
                assert float(fop._dscale.cpu()) == 0.0
            after = _state(fop, n)
            assert after["scale"].tobytes() == before["scale"].tobytes() == np.float32([ODD["scale_init"]]).tobytes()
            assert not np.array_equal(after["rows"], before["rows"])
        if which == "phase2_world":
            assert not want["dcam"].any() and not dcam.any()
            before = _state(fop, n)
            for ii in (1, 2, 3):
                _, dc = _backward(fop, n, ii, P, 0)
                assert not dc.any()
                _step(fop, ii, P)
            after = _state(fop, n)
            assert after["cam"].tobytes() == before["cam"].tobytes()
            assert not np.array_equal(after["rows"], before["rows"])
        fop.close()


def _run_sequence(fop, case, iters, P, log_every, how):
    """`iters` iterations from the clip's start, issued as fdcap_opt_backward + fdcap_opt_step ("two"), fdcap_opt_backward_and_step
    ("fused") or one fdcap_opt_run ("run"); logging iterations as FittingOP.fitting issues them (log_terms = 2, the sums straight
    into their history row).  -> rows, camera_ext, scale and the history as bytes-comparable arrays."""
    lib, h, n = fop.ctx.lib, fop.ctx.handle, case[5]
    _init_from_clip(fop, case[2])
    logged = [ii for ii in range(iters) if is_logging_iteration(ii, iters, log_every)]
    hist = torch.zeros(max(len(logged), 1), capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
    st = capi.current_stream()
    try:
        if how == "run":
            n_done = ctypes.c_int32(0)
            capi.check(lib.fdcap_opt_run(h, 0, iters, iters, P, log_every, capi.dptr(hist) if logged else None, len(logged), 0, ctypes.byref(n_done), st), "run")
            assert n_done.value == len(logged)
        else:
            for ii in range(iters):
                do_log = ii in logged
                if do_log:
                    capi.check(lib.fdcap_opt_set_loss_output(h, capi.dptr(hist[logged.index(ii)])), "set_loss_output")
                if how == "fused":
                    capi.check(lib.fdcap_opt_backward_and_step(h, ii, P, 2 if do_log else 0, st), "backward_and_step")
                else:
                    capi.check(lib.fdcap_opt_backward(h, ii, P, 2 if do_log else 0, st), "backward")
                    capi.check(lib.fdcap_opt_step(h, ii, P, st), "step")
    finally:
        capi.check(lib.fdcap_opt_sync(h, st), "sync")
        capi.check(lib.fdcap_opt_set_loss_output(h, capi.dptr(fop._losses)), "set_loss_output")
    out = _state(fop, n)
    out["hist"] = hist.cpu().numpy()[:len(logged)]
    return out


def _same_bytes(a, b, zero_sign_may_differ=False):
    """zero_sign_may_differ (pose trim on against off, as tests/test_gpu_pose_trim.py): an accumulator that took -0 terms from the
    dropped joints may hold +0 -- equal values, and bits that differ only where the value is zero."""
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype and np.all(np.isfinite(x)), k
        if zero_sign_may_differ:
            assert np.array_equal(x, y), (k, np.abs(x - y).max())
            bits = np.uint32 if x.dtype.itemsize == 4 else np.uint64
            assert np.all(x[x.view(bits) != y.view(bits)] == 0), k
        else:
            assert x.tobytes() == y.tobytes(), (k, np.abs(x - y).max())


@pytest.mark.parametrize("log_every", [0, 1, 2])
@pytest.mark.parametrize("which", ZERO_CASES)
def test_a_zero_weight_gives_the_same_bytes_however_the_iterations_are_issued(which, log_every, monkeypatch):
    """6 iterations, P = 3, so that logging and non-logging iterations alternate in both phases and the contact forward comes and
    goes: two calls per iteration and the fused call, each with the limited joint sets and with FDCAP_POSE_TRIM=0."""
    s = dict(ODD, **{which: 0.0})
    case = sc.make_case(*sc.FIT_CASE)
    res = {}
    for trim in (True, False):
        if trim: monkeypatch.delenv("FDCAP_POSE_TRIM", raising=False)
        else: monkeypatch.setenv("FDCAP_POSE_TRIM", "0")                  # (read by every fdcap_opt_create)
        for how in ("two", "fused"):
            fop = _fop(monkeypatch, case, s)
            res[trim, how] = _run_sequence(fop, case, 6, 3, log_every, how)
            fop.close()
    _same_bytes(res[True, "two"], res[True, "fused"])
    _same_bytes(res[False, "two"], res[False, "fused"])
    _same_bytes(res[True, "two"], res[False, "two"], zero_sign_may_differ=True)
    if log_every:
        assert res[True, "two"]["hist"].shape[0] == len([i for i in range(6) if is_logging_iteration(i, 6, log_every)])
        assert np.all(res[True, "two"]["hist"][:, 3] > 0)                 # the contact term is printed whatever its weight in the total


# ---- 4 ----------------------------------------------------------------------------------------------------------------------------
def _ulp32(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def test_the_optimiser_step_is_adam_in_fp64_on_the_gpus_own_gradients(monkeypatch):
    """lr = 0.0123, P = 2, ii = 0 .. 5, legacy_zero_grad = 0.  Each step is replayed in numpy float64 (beta 0.9 / 0.999, eps 1e-8):
    the moments are carried in float64 from the GPU's gradients, x restarts from the GPU's previous value, so one step's rounding
    is compared.  Step count ii + 1 for the rows, and for `scale` while ii < P; camera_ext does not step before ii = P + 1 and then
    counts ii - P (its moments start there: the gradient of ii = P is not accumulated); `scale` keeps its bits from ii = P on.
    d loss / d scale is read after the step, which forms it (a backward with log_terms = 0 leaves it to the step: include/fdcap.h).
    Bar, from fp32 rounding of the update and of the subtraction: |x_gpu - x_ref| <= ulp_fp32(max|x|) + 1e-5 lr per entry.
    Measured on an MI355X (max over the six steps): rows 1.19e-7 (bar 3.61e-7), camera_ext 2.32e-7 (bar 6.00e-7), scale 2.8e-8
    (bar 2.42e-7).
    lr itself: after the first step from zero moments Adam moves an entry by lr |g| / (|g| + eps); every entry with
    |g| > 1e-4 max|g| has moved by that within 1e-5 lr + ulp_fp32(|x|) / 2 (the subtraction rounds to the nearest fp32), and within
    1e-5 lr alone wherever that rounding is below 1e-6 lr; `scale` has moved by lr itself within 1e-5 lr."""
    case = sc.make_case(*sc.FIT_CASE)
    n, lr, P = case[5], ODD["lr"], 2
    fop = _fop(monkeypatch, case, ODD)
    _init_from_clip(fop, case[2])
    b1, b2, eps = 0.9, 0.999, 1e-8
    mom = {k: [0.0, 0.0] for k in ("rows", "cam", "scale")}
    worst = {"rows": 0.0, "cam": 0.0, "scale": 0.0}

    def adam(key, x_prev, g, t):
        m, v = mom[key]
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        mom[key] = [m, v]
        return x_prev - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)

    for ii in range(6):
        dx, dcam = _backward(fop, n, ii, P, 0)
        before = _state(fop, n)
        _step(fop, ii, P)
        after = _state(fop, n)
        dscale = float(fop._dscale.cpu())
        ref = {"rows": adam("rows", before["rows"].astype(np.float64), dx.astype(np.float64), ii + 1)}
        if ii < P:
            assert dscale != 0.0
            ref["scale"] = adam("scale", before["scale"].astype(np.float64), np.float64(dscale), ii + 1)
        else:
            assert after["scale"].tobytes() == before["scale"].tobytes()
        if ii >= P + 1:
            assert np.abs(dcam).max() > 0
            ref["cam"] = adam("cam", before["cam"].astype(np.float64), dcam.astype(np.float64), ii - P)
        else:
            assert after["cam"].tobytes() == before["cam"].tobytes()
        for k, want in ref.items():
            err = np.abs(after[k].astype(np.float64) - want).max()
            worst[k] = max(worst[k], err)
            bar = _ulp32(before[k]) + 1e-5 * lr
            print(f"ii={ii} {k}: max |gpu - fp64 Adam| {err:.3e} (bar {bar:.3e})")
            assert err <= bar, (ii, k, err, bar)
        if ii == 0:
            for k, g in (("rows", dx.astype(np.float64)), ("scale", np.array([dscale]))):
                x0, x1 = before[k].astype(np.float64), after[k].astype(np.float64)
                sel = np.abs(g) > 1e-4 * np.abs(g).max()
                dev = np.abs(np.abs(x1 - x0) - lr * np.abs(g) / (np.abs(g) + eps))[sel]
                half_ulp = 0.5 * np.spacing(np.abs(before[k][sel]).astype(np.float32)).astype(np.float64)
                assert sel.sum() >= (1 if k == "scale" else n * 40) and np.all(dev <= 1e-5 * lr + half_ulp), (k, dev.max())
                fine = half_ulp <= 1e-6 * lr
                if k == "rows":
                    assert fine.sum() >= 50 and np.all(dev[fine] <= 1e-5 * lr), dev[fine].max()
                else:
                    # `scale`: |g| = 1.3e-2 (eps / |g| = 8e-7) and half an ulp of 1.3 is 6e-8 = 0.5e-5 lr: it has moved by lr itself
                    assert abs(abs(float(x1[0] - x0[0])) - lr) <= 1e-5 * lr, abs(float(x1[0] - x0[0]))
                assert np.all(np.sign(x0 - x1)[sel] == np.sign(g)[sel])
    print("Adam replay, max over the steps:", worst)
    fop.close()


@pytest.mark.parametrize("log_every", [0, 1])
def test_three_ways_to_issue_the_iterations_give_the_same_bits_at_the_odd_settings(log_every, monkeypatch):
    """6 iterations, P = 2: fdcap_opt_backward + fdcap_opt_step, fdcap_opt_backward_and_step, one fdcap_opt_run -- rows, camera_ext,
    scale and the logged sums (tests/test_gpu_parity.py shows it at the defaults, through whole fits)."""
    case = sc.make_case(*sc.FIT_CASE)
    res = {}
    for how in ("two", "fused", "run"):
        fop = _fop(monkeypatch, case, ODD)
        res[how] = _run_sequence(fop, case, 6, 2, log_every, how)
        fop.close()
    _same_bytes(res["two"], res["fused"])
    _same_bytes(res["two"], res["run"])
    assert res["two"]["scale"][0] != np.float32(ODD["scale_init"])
    if log_every:
        assert res["two"]["hist"].shape == (6, capi.NUM_LOSSES) and np.all(res["two"]["hist"][:, [1, 2, 3, 4]] > 0)
        assert res["two"]["hist"][0, 0] == 0 and np.all(res["two"]["hist"][1:, 0] > 0)     # (the data term: the fit starts on the data)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------------
def test_a_short_fit_at_the_odd_settings_matches_the_oracle(monkeypatch):
    """10 frames, 12 iterations (phase 2 from iteration 10), every iteration logged, against the fp32 oracle at the same settings.
    Bars: tests/test_settings_cpu.py FIT_BARS -- the project's, each at least 3 x the yardsticks measured there (fp64 oracle and
    the host build of the kernels' math against the fp32 oracle); FIT_CASE says how the clip was chosen.  Before the first step the world contact vertices and joints are the oracle's (3e-5): that and the first printed contact
    term pin scale_init."""
    case = sc.make_case(*sc.FIT_CASE)
    bm, vp, clip, scene, vid, n = case
    fop = _fop(monkeypatch, case, ODD, num_iter=sc.FIT_ITERS)
    _init_from_clip(fop, clip)
    v = torch.empty(n, len(vid), 3, device="cuda")
    j = torch.empty(n, 23, 3, device="cuda")
    capi.check(fop.ctx.lib.fdcap_opt_forward_world(fop.ctx.handle, capi.dptr(v), capi.dptr(j), capi.current_stream()), "fw")
    ov, oj = sc.forward_world(ODD["scale_init"])
    np.testing.assert_allclose(v.cpu().numpy(), ov, atol=3e-5)
    np.testing.assert_allclose(j.cpu().numpy(), oj, atol=3e-5)
    body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=1)
    assert first_phase2_iter(sc.FIT_ITERS) == 10 and fop.log.iters == list(range(sc.FIT_ITERS))
    log = np.array([fop.log.l_rec, fop.log.l_vposer, fop.log.loss_smoothing, fop.log.loss_contact, fop.log.loss_world_smoothing, fop.log.total]).T
    want = sc.oracle_fit(tuple(ODD.items()), torch.float32)
    got = (body.cpu().numpy(), float(scale), cam.cpu().numpy(), log)
    print("short fit vs the fp32 oracle:", {k: float(x) for k, x in sc.fit_figures(got, want).items()})
    bad = sc.fit_violations(got, want)
    assert not bad, bad
    # the first iteration's six printed values, before any step: the total is the odd combination
    np.testing.assert_allclose(log[0, [0, 1, 2, 3, 5]], want[3][0, [0, 1, 2, 3, 5]], rtol=2e-5)
    np.testing.assert_allclose(log[0, 4], want[3][0, 4], rtol=1e-4)
    fop.close()


# ---- 6 ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch_model():
    """The model of tests/test_gpu_ragged_clips.py."""
    bm = synth.make_body_model(300, seed=31)
    vp = synth.make_vposer(seed=32)
    scene = synth.make_scene(9000, seed=34)
    l, r = synth.make_contact_ids(bm.v_template, per_part=24, seed=35)
    return bm, vp, scene, np.concatenate([l, r])


LOG_FIELDS = ("iters", "l_rec", "l_vposer", "loss_smoothing", "loss_contact", "loss_world_smoothing", "total")


@pytest.mark.parametrize("lens", [(9, 9), (3, 9, 12)])
def test_a_batch_at_the_odd_settings_gives_each_clip_its_stand_alone_bytes(lens, batch_model, monkeypatch):
    """Two clips of one length (fdcap_opt_create_clips) and three of different lengths (fdcap_opt_create_clips_var: the kernels
    read every weight from the clip table on the device), 10 iterations across the switch, every iteration logged, pose trim on:
    parameters, scale, camera_ext and the logged rows of each clip are those of its stand-alone FittingOP fit at the same settings.
    Each clip's `scale` has left scale_init by less than the eight phase-1 steps can move it (scale_init did arrive); that the
    other settings arrive in a stand-alone fit is what the tests above show."""
    bm, vp, scene, vid = batch_model
    _patch(monkeypatch, ODD)
    monkeypatch.delenv("FDCAP_POSE_TRIM", raising=False)
    cfgs = _configs(ODD, 10)
    clips = []
    for k, n in enumerate(lens):
        c = synth.make_clip(n, seed=81 + k, num_outliers=2)
        clips.append((c.body_params, read_camerapose(c.camerapose_lines)))
    f = ClipBatchFitter(*cfgs, body_model=bm, vposer=vp, contact_ids=vid)
    res = f.fit(clips, scene, log_every=1)
    batch = [(b.cpu().numpy(), np.float32(s), c.cpu().numpy(), log) for (b, s, c), log in zip(res, f.logs)]
    f.close()
    for k, (body_in, cam_in) in enumerate(clips):
        fop = FittingOP(*cfgs, lens[k], body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=cam_in)
        b, s, c = fop.fitting(torch.tensor(body_in).cuda(), "global", log_every=1)
        alone = (b.cpu().numpy(), np.float32(s), c.cpu().numpy(), fop.log)
        fop.close()
        assert batch[k][0].tobytes() == alone[0].tobytes(), (k, np.abs(batch[k][0] - alone[0]).max())
        assert batch[k][1].tobytes() == alone[1].tobytes(), (k, batch[k][1], alone[1])
        assert batch[k][2].tobytes() == alone[2].tobytes(), (k, np.abs(batch[k][2] - alone[2]).max())
        for fld in LOG_FIELDS:
            x, y = np.array(getattr(batch[k][3], fld), dtype=np.float64), np.array(getattr(alone[3], fld), dtype=np.float64)
            assert len(x) == 10 and np.all(np.isfinite(x)) and x.tobytes() == y.tobytes(), (k, fld)
        assert alone[1] != np.float32(ODD["scale_init"]) and abs(float(alone[1]) - ODD["scale_init"]) < 10 * ODD["lr"]


# ---- 7 ----------------------------------------------------------------------------------------------------------------------------
def test_fit2d_gradient_and_sums_at_odd_intrinsics_rho_and_stage_weights():
    """fx 710, fy 655, cx 612, cy 377, rho 63, w_data 1.7, w_pose 3.1, w_shape 6.3, w_hand 2.2 on _case(16, 7) of
    tests/test_gpu_innerfit.py with a third of the detected keypoints 150 px off.  sc.fit2d_check_case asserts, at the very point the
    kernel is evaluated at, that a quarter of the detected residuals lie beyond rho and a quarter below rho / 2, and that fx <-> fy,
    w_data unsquared and rho = 100 move the oracle's gradient 20 bars, w_pose <-> w_hand the prior sum and the hand columns' block --
    which is why the hand columns (a pure prior gradient) are also held to the bar taken over their own block."""
    bm, vp, init, kp, n = sc.fit2d_case()
    st = sc.FIT2D_STAGE
    op = InnerFitOP(bm, vp, n, intrinsics=(st["fx"], st["fy"], st["cx"], st["cy"]), rho=st["rho"], iters_per_stage=0)
    op.fitting(init, kp)
    lib, h = op.ctx.lib, op.ctx.handle
    sg = capi.Fit2dStage(st["fx"], st["fy"], st["cx"], st["cy"], st["rho"], st["w_data"], st["w_pose"], st["w_shape"], st["w_hand"])
    capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 1, capi.current_stream()), "backward_fit2d")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, capi.current_stream()), "get_grads")
    s = op._losses.cpu().numpy()
    dx = dx.cpu().numpy()
    data, prior, g = sc.fit2d_check_case(op.body_rotation_rec.detach().cpu().double().numpy())
    np.testing.assert_allclose(s[:2], [data, prior], rtol=sc.FIT2D_SUM_RTOL)
    np.testing.assert_allclose(dx, g, rtol=sc.GRAD_RTOL, atol=sc.GRAD_ATOL * np.abs(g).max())
    np.testing.assert_allclose(dx[:, sc.HANDS], g[:, sc.HANDS], rtol=sc.GRAD_RTOL, atol=sc.hand_block_bar(g))
    # second evaluation, w_data = 0.003: the priors' gradient dominates every column it reaches, and sc.fit2d_check_prior_case asserts
    # that a swap among w_pose / w_shape / w_hand moves each of its two column blocks 20 whole-gradient bars
    sp = sc.FIT2D_PRIOR_STAGE
    sg = capi.Fit2dStage(sp["fx"], sp["fy"], sp["cx"], sp["cy"], sp["rho"], sp["w_data"], sp["w_pose"], sp["w_shape"], sp["w_hand"])
    capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 1, capi.current_stream()), "backward_fit2d")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, capi.current_stream()), "get_grads")
    s = op._losses.cpu().numpy()
    data, prior, g = sc.fit2d_check_prior_case(op.body_rotation_rec.detach().cpu().double().numpy())
    np.testing.assert_allclose(s[:2], [data, prior], rtol=sc.FIT2D_SUM_RTOL)
    np.testing.assert_allclose(dx.cpu().numpy(), g, rtol=sc.GRAD_RTOL, atol=sc.GRAD_ATOL * np.abs(g).max())
    op.close()


def test_fit2d_first_adam_step_moves_by_the_configured_lr():
    """InnerFitOP(lr = 0.023, one stage, one iteration): from zero moments Adam moves an entry by lr |g| / (|g| + 1e-8); every entry
    with |g| > 1e-4 max|g| has moved by that within 1e-5 lr + ulp_fp32(|x|) / 2 (the subtraction rounds to the nearest fp32), in the
    gradient's direction, and an entry without a gradient has not moved; wherever that rounding is below 1e-6 lr the entry has moved
    by lr itself within 1e-5 lr (|g| > 20 there, so eps does not show)."""
    bm, vp, init, kp, n = sc.fit2d_case()
    st = sc.FIT2D_STAGE
    lr = 0.023
    kw = dict(intrinsics=(st["fx"], st["fy"], st["cx"], st["cy"]), rho=st["rho"], lr=lr,
              stages=((st["w_data"], st["w_pose"], st["w_shape"], st["w_hand"]),))
    op = InnerFitOP(bm, vp, n, iters_per_stage=0, **kw)
    op.fitting(init, kp)
    sg = capi.Fit2dStage(st["fx"], st["fy"], st["cx"], st["cy"], st["rho"], st["w_data"], st["w_pose"], st["w_shape"], st["w_hand"])
    capi.check(op.ctx.lib.fdcap_opt_backward_fit2d(op.ctx.handle, ctypes.byref(sg), 0, capi.current_stream()), "backward_fit2d")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(op.ctx.lib.fdcap_opt_get_grads(op.ctx.handle, capi.dptr(dx), None, capi.current_stream()), "get_grads")
    g = dx.cpu().numpy().astype(np.float64)
    x0 = op.body_rotation_rec.detach().cpu().numpy()
    op.close()
    op = InnerFitOP(bm, vp, n, iters_per_stage=1, **kw)
    op.fitting(init, kp)
    x1 = op.body_rotation_rec.detach().cpu().numpy()
    op.close()
    sel = np.abs(g) > 1e-4 * np.abs(g).max()
    assert sel.sum() >= n * 20
    moved = x1.astype(np.float64) - x0.astype(np.float64)
    dev = np.abs(np.abs(moved) - lr * np.abs(g) / (np.abs(g) + 1e-8))[sel]
    half_ulp = 0.5 * np.spacing(np.abs(x0[sel])).astype(np.float64)
    print("inner fit, first step: max deviation from lr", dev.max(), "of", sel.sum(), "entries")
    assert np.all(dev <= 1e-5 * lr + half_ulp), dev.max()
    fine = half_ulp <= 1e-6 * lr                                       # where the subtraction's rounding is negligible: lr itself, plainly
    assert fine.sum() >= 50 and np.all(np.abs(np.abs(moved[sel][fine]) - lr) <= 1e-5 * lr), np.abs(np.abs(moved[sel][fine]) - lr).max()
    assert np.all(np.sign(-moved[sel]) == np.sign(g[sel]))
    assert np.all(moved[g == 0] == 0)


# ---- 8 ----------------------------------------------------------------------------------------------------------------------------
def test_smoother_at_odd_lr_iterations_and_weights_matches_the_oracle():
    """lr 0.037, 17 iterations, weight_loss_rec 0.6, weight_loss_vposer 0.02 on the 40-frame clip of
    test_smoother_file_by_file_equals_one_launch_and_the_oracle, against SmootherOracle with the same four values at the project's
    1e-5 (5.8 x the fp64-vs-fp32 yardstick of tests/test_settings_cpu.py; the oracle at the defaults is 1e5 bars away)."""
    rows = sc.smoother_clip()
    c = sc.SMOOTHER
    out = SmootherOP({"init_lr_h": c["init_lr_h"], "num_iter": c["num_iter"]},
                     {"weight_loss_rec": c["weight_loss_rec"], "weight_loss_vposer": c["weight_loss_vposer"]}).fitting_clip(rows).cpu().numpy()
    ref = SmootherOracle(**c).fitting_clip(rows).numpy()
    print("smoother at the odd settings, GPU vs oracle: max", np.abs(out - ref).max())
    assert np.abs(out - ref).max() < sc.SMOOTHER_BAR
