"""GPU tests of the inner fit's free expression coefficients (csrc/fdc_keypoints.h fit2d_kp_expr_kernel / fit2d_kp_expr_jaw_kernel,
lbfgs_advance_expr_kernel; fdcap_opt_set_expression, fdcap_opt_get_expression, fdcap_opt_set_expression_prior) through the C-ABI, against
the fp64 torch twin tests/expression_spec.py.  The body is synth.make_body_model(240) with lbs_nnz 4 and 8, 1 and 16 frames, both blend
forms pinned with FDCAP_KP_BLEND; the maps are tests/test_gpu_face.face_map's and one of joints 0..22 alone.

Bars.  Loss sums 2e-5 relative; the 78-column gradient and the expression block 2e-3 relative + 2e-4 of the BLOCK's largest entry
(tests/test_gpu_keypoints.py); the jaw block and the prior alone tests/gradient_bars.py's formula 32 max(max|g32 - g64|, 2^-24 max|g64|),
g32 / g64 the twin's two precisions; positions the same formula.  Fitted rows: the bars of tests/test_gpu_keypoints.py's fit.  The fp32
twin's own distance from the fp64 twin is printed next to every error.  No bar is taken from a HIP result."""
import ctypes

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.innerfit import DEFAULT_BEND_RATIO, InnerFitOP, KeypointMap
from oracle import rotrepr
from tests import gradient_bars as gb
from tests.expression_spec import NEXPR, ExpressionSpec
from tests.keypoint_spec import COLUMN_BLOCKS, column_errors
from tests.test_gpu_face import _case, _extra, _loss_and_grads, _models, _set_extra, face_map

pytestmark = pytest.mark.gpu
STAGE = (1.0, 4.78, 5.0, 4.78)
W_JAW, W_BEND, W_EXPR = (47.8, 478.0, 478.0), DEFAULT_BEND_RATIO * STAGE[1], 5.0
E_ARG, E_STATE = -1, -2
PSI_SIGMA = 1.5


def joints_map(bm):
    return KeypointMap([3, 15, 22, 7, 20], np.zeros((5, 3)), np.zeros((5, 3)))


def _open(n, lbs_nnz, form, monkeypatch, seed=7, **kw):
    """an InnerFitOP whose state stands at the start rows: form "kernel" / "panel" pin the blend form on face_map's map, "jointmap" is the
    map of joints 0..22 alone -> op, (bm, vp, kmap), start rows [n, 75], keypoints, psi ~ N(0, 1.5^2), an open jaw"""
    monkeypatch.setenv("FDCAP_KP_BLEND", form if form in ("kernel", "panel") else "kernel")
    bm, vp, kmap, gt, init, kp = _case(n, seed, lbs_nnz, joints_map if form == "jointmap" else face_map)
    rng = np.random.Generator(np.random.PCG64(seed + 11))
    psi = (PSI_SIGMA * rng.standard_normal((n, NEXPR))).astype(np.float32)
    jaw = rng.standard_normal((n, 3))
    jaw = (0.3 * jaw / np.linalg.norm(jaw, axis=1, keepdims=True)).astype(np.float32)
    op = InnerFitOP(bm, vp, n, keypoint_map=kmap, **kw)
    return op, (bm, vp, kmap), init, kp, psi, jaw


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _set(op, psi=None, jaw=None, w_expr=None, w_jaw=None, w_bend=0.0):
    """psi / jaw: numpy arrays, or None to leave the call out"""
    lib, h, st = op.ctx.lib, op.ctx.handle, capi.current_stream()
    if jaw is not None:
        capi.check(lib.fdcap_opt_set_jaw(h, capi.dptr(_dev(jaw)), st), "fdcap_opt_set_jaw")
    if psi is not None:
        capi.check(lib.fdcap_opt_set_expression(h, capi.dptr(_dev(psi)), st), "fdcap_opt_set_expression")
    if w_expr is not None:
        capi.check(lib.fdcap_opt_set_expression_prior(h, float(w_expr)), "fdcap_opt_set_expression_prior")
    ex = _extra(w_bend)
    if w_jaw is not None:
        ex.w_jaw[0], ex.w_jaw[1], ex.w_jaw[2] = w_jaw
    assert _set_extra(op, ex) == 0


def _get(op, n, what):
    lib, h, st = op.ctx.lib, op.ctx.handle, capi.current_stream()
    out = torch.empty(n, 3 if "jaw" in what else NEXPR, device="cuda")
    args = {"psi": (lib.fdcap_opt_get_expression, out, None), "dpsi": (lib.fdcap_opt_get_expression, None, out),
            "jaw": (lib.fdcap_opt_get_jaw, out, None), "djaw": (lib.fdcap_opt_get_jaw, None, out)}[what]
    capi.check(args[0](h, capi.dptr(args[1]), capi.dptr(args[2]), st), what)
    return out.cpu().numpy()


def _positions(op, n, nkp):
    out = torch.empty(n, nkp, 3, device="cuda")
    capi.check(op.ctx.lib.fdcap_debug_keypoints3d(op.ctx.handle, capi.dptr(out), capi.current_stream()), "fdcap_debug_keypoints3d")
    return out.cpu().numpy()


def _spec(m, **kw):
    bm, vp, kmap = m
    return ExpressionSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, **kw)


# ---- 1. positions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lbs_nnz,form,with_jaw", [(1, 4, "kernel", False), (16, 8, "kernel", True), (16, 4, "panel", True), (16, 4, "jointmap", False)])
def test_mapped_positions_with_expression_match_the_spec(n, lbs_nnz, form, with_jaw, monkeypatch):
    op, m, init, kp, psi, jaw = _open(n, lbs_nnz, form, monkeypatch, iters_per_stage=0)
    op.fitting(init, kp)
    x = op.body_rotation_rec.detach().cpu().numpy()
    p0 = _positions(op, n, len(m[2]))
    _set(op, psi, jaw if with_jaw else None)
    got = _positions(op, n, len(m[2]))
    jw = jaw if with_jaw else None
    p64, p32 = _spec(m).positions(x, jw, psi), _spec(m, dtype=torch.float32).positions(x, jw, psi)
    bar = 32.0 * max(float(np.abs(p32 - p64).max()), 2.0 ** -24 * float(np.abs(p64).max()))
    err = float(np.abs(got - p64).max())
    print(f"positions n {n} lbs_nnz {lbs_nnz} {form} jaw {with_jaw}: max|err| {err:.3e} bar {bar:.3e}  moved by psi (and the jaw): {np.abs(got - p0).max():.3e}")
    assert err <= bar and np.abs(got - p0).max() > 100 * bar
    op.close()


# ---- 2. loss sums and every gradient block ---------------------------------------------------------------------------------------------------
GRAD_CASES = [(1, 4, "kernel", "expr"), (16, 4, "kernel", "expr_jaw"), (16, 8, "kernel", "expr_jaw_bend"), (1, 4, "panel", "expr_jaw"),
              (16, 4, "panel", "expr"), (16, 8, "panel", "expr_jaw_bend"), (16, 4, "jointmap", "expr"), (1, 8, "jointmap", "expr")]


@pytest.mark.parametrize("n,lbs_nnz,form,mode", GRAD_CASES)
def test_loss_and_gradient_with_free_expression_match_fp64_autograd(n, lbs_nnz, form, mode, monkeypatch):
    op, m, init, kp, psi, jaw = _open(n, lbs_nnz, form, monkeypatch, iters_per_stage=0)
    kp[0, 2, 2] = 0.0
    op.fitting(init, kp)
    jw, wj = (jaw, W_JAW) if "jaw" in mode else (None, None)
    wb = W_BEND if "bend" in mode else 0.0
    _set(op, psi, jw, W_EXPR, wj, wb)
    s, dx = _loss_and_grads(op, n)
    de = _get(op, n, "dpsi")
    dj = _get(op, n, "djaw") if jw is not None else None
    assert np.array_equal(_get(op, n, "psi"), psi)
    x = op.body_rotation_rec.detach().cpu().numpy()
    s64, g64, j64, e64 = _spec(m).grads(x, kp, STAGE, jw, wj, wb, psi, W_EXPR)
    s32, g32, j32, e32 = _spec(m, dtype=torch.float32).grads(x, kp, STAGE, jw, wj, wb, psi, W_EXPR)
    err, twin = column_errors(dx, g64), column_errors(g32, g64)
    print(f"expression, n {n} lbs_nnz {lbs_nnz} {form} {mode}: loss rel err", np.abs(s - s64) / np.abs(s64), " fp32 twin", np.abs(s32 - s64) / np.abs(s64))
    for k in COLUMN_BLOCKS:
        print(f"  d {k:7s} max|err| {err[k][0]:.3e}  fp32 twin {twin[k][0]:.3e}  max|g| {err[k][1]:.3e}")
    print(f"  d expr    max|err| {np.abs(de - e64).max():.3e}  fp32 twin {np.abs(e32 - e64).max():.3e}  max|g| {np.abs(e64).max():.3e}")
    np.testing.assert_allclose(s, s64, rtol=2e-5)
    for k, sl in COLUMN_BLOCKS.items():
        assert np.all(np.abs(dx[:, sl] - g64[:, sl]) <= 2e-3 * np.abs(g64[:, sl]) + 2e-4 * err[k][1]), (k, err[k], twin[k])
    assert np.abs(e64).max() > 0 and np.all(np.abs(de - e64) <= 2e-3 * np.abs(e64) + 2e-4 * np.abs(e64).max())
    if dj is not None:
        jbar = 32.0 * max(float(np.abs(j32 - j64).max()), 2.0 ** -24 * float(np.abs(j64).max()))
        print(f"  d jaw     max|err| {np.abs(dj - j64).max():.3e}  bar {jbar:.3e}")
        assert np.abs(dj - j64).max() <= jbar
    op.close()


# ---- 3. the prior alone ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,form", [(16, "kernel"), (16, "panel"), (1, "jointmap")])
def test_the_expression_prior_alone_is_inside_the_twins_rounding_bars(n, form, monkeypatch):
    stage0 = (1.0, 0.0, 0.0, 0.0)
    op, m, init, kp, psi, jaw = _open(n, 4, form, monkeypatch, iters_per_stage=0)
    kp[:, :, 2] = 0.0
    op.fitting(init, kp)
    _set(op, psi, None, W_EXPR)
    s, dx = _loss_and_grads(op, n, stage0)
    de = _get(op, n, "dpsi")
    x = op.body_rotation_rec.detach().cpu().numpy()
    s64, _, _, e64 = _spec(m).grads(x, kp, stage0, None, None, 0.0, psi, W_EXPR)
    s32, _, _, e32 = _spec(m, dtype=torch.float32).grads(x, kp, stage0, None, None, 0.0, psi, W_EXPR)
    bar = gb.bars({"expr": e32}, {"expr": e64})
    r = gb.ratios({"expr": de}, {"expr": e64}, bar)
    print(f"expression prior alone, n {n} {form}: prior rel err", abs(s[1] - s64[1]) / s64[1], "fp32 twin", abs(s32[1] - s64[1]) / s64[1], "max|err| / bar", r)
    assert s[0] == 0.0 and s64[1] > 0
    np.testing.assert_allclose(s[1], s64[1], rtol=2e-5)
    assert all(v <= 1.0 for v in r.values()), r
    assert np.all(dx == 0)                                   # the prior reaches the coefficients only
    op.close()


# ---- 4. off is off -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lbs_nnz,form,with_jaw", [(16, 4, "kernel", False), (16, 8, "kernel", True), (16, 4, "panel", True), (1, 4, "panel", False),
                                                     (16, 4, "jointmap", False)])
def test_coefficients_at_zero_give_the_bits_of_a_context_that_never_called(n, lbs_nnz, form, with_jaw, monkeypatch):
    res = []
    for call in (False, True):
        op, m, init, kp, psi, jaw = _open(n, lbs_nnz, form, monkeypatch, iters_per_stage=0)
        op.fitting(init, kp)
        _set(op, np.zeros_like(psi) if call else None, jaw if with_jaw else None, 0.0 if call else None, W_JAW if with_jaw else None, W_BEND)
        pos = _positions(op, n, len(m[2]))
        s, dx = _loss_and_grads(op, n)
        res.append((pos, s, dx, _get(op, n, "djaw") if with_jaw else None))
        if call:
            assert np.abs(_get(op, n, "dpsi")).max() > 0     # (the keypoints pull on coefficients that stand at zero)
        op.close()
    for a, b in zip(*res):
        assert a is None or np.array_equal(a, b)


@pytest.mark.parametrize("form", ["kernel", "panel"])
def test_set_and_cleared_again_a_whole_fit_keeps_its_bits(form, monkeypatch):
    n, outs = 16, []
    for touch in (False, True):
        op, m, init, kp, psi, jaw = _open(n, 4, form, monkeypatch, seed=21, iters_per_stage=6, fit_jaw=True)
        if touch:
            setup = op._setup

            def setup_and_touch(*a, _op=op, _setup=setup):
                _setup(*a)
                lib, h, st = _op.ctx.lib, _op.ctx.handle, capi.current_stream()
                capi.check(lib.fdcap_opt_set_expression(h, capi.dptr(_dev(psi)), st), "set")
                capi.check(lib.fdcap_opt_set_expression_prior(h, 3.0), "prior")
                capi.check(lib.fdcap_opt_set_expression(h, None, st), "clear")
            op._setup = setup_and_touch
        outs.append((op.fitting(init, kp).cpu().numpy(), op.jaw_pose.cpu().numpy()))
        op.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ---- 5. a five-stage Adam fit -----------------------------------------------------------------------------------------------------------------
FIT_STAGES = (STAGE,) * 5
FIT_JAW_PRIOR, FIT_EXPR_PRIOR = ((4.78,) * 3,) * 5, (0.5,) * 5


def _fit_case(n, seed, lbs_nnz=4, psi_sigma=0.5, noise=0.1, kmap_of=face_map):
    """ground truth near the priors' optimum, psi_gt != 0 and an open jaw; keypoints = its mapped points + `noise` px; start = ground
    truth rows with the camera translation off by 2 cm, psi = 0, the jaw shut"""
    bm, vp = _models(seed, lbs_nnz)
    kmap = kmap_of(bm)
    clip = synth.make_clip(n, seed=seed + 2, num_outliers=0)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    gt = clip.body_params.astype(np.float32).copy()
    gt[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32) + 0.05 * rng.standard_normal((n, 3)).astype(np.float32)
    gt[:, 6:72] = 0.05 * rng.standard_normal((n, 66)).astype(np.float32)
    jaw_gt = np.tile(np.array([0.25, 0.02, -0.03], np.float32), (n, 1)) + 0.03 * rng.standard_normal((n, 3)).astype(np.float32)
    psi_gt = (psi_sigma * rng.standard_normal((n, NEXPR))).astype(np.float32)
    spec = ExpressionSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary)
    x6 = rotrepr.convert_to_6D_rot(torch.tensor(gt, dtype=torch.float64)).numpy()
    uv = spec.project(torch.tensor(spec.positions(x6, jaw_gt, psi_gt))).numpy()
    kp = np.concatenate([uv + noise * rng.standard_normal(uv.shape), rng.uniform(0.3, 1.0, (n, len(kmap), 1))], -1).astype(np.float32)
    init = gt.copy()
    init[:, 72:75] += 0.02 * rng.standard_normal((n, 3)).astype(np.float32)
    return (bm, vp, kmap), init, kp, psi_gt, jaw_gt


@pytest.mark.parametrize("form", ["kernel", "panel"])
def test_five_stage_fit_with_free_expression_matches_the_twin_and_finds_the_coefficients(form, monkeypatch):
    n, iters = 16, 20
    monkeypatch.setenv("FDCAP_KP_BLEND", form)
    m, init, kp, psi_gt, jaw_gt = _fit_case(n, 21)
    op = InnerFitOP(m[0], m[1], n, keypoint_map=m[2], stages=FIT_STAGES, iters_per_stage=iters, fit_jaw=True, jaw_prior=FIT_JAW_PRIOR,
                    fit_expression=True, expression_prior=FIT_EXPR_PRIOR)
    out = op.fitting(init, kp).cpu().numpy()
    psi, jaw = op.expression.cpu().numpy(), op.jaw_pose.cpu().numpy()
    op.close()
    threads, twin = torch.get_num_threads(), []
    try:
        for t in (1, 4):
            torch.set_num_threads(t)
            s32 = _spec(m, dtype=torch.float32)
            r = s32.fitting_expr(init, kp, FIT_STAGES, iters, np.zeros((n, NEXPR), np.float32), FIT_EXPR_PRIOR, np.zeros((n, 3), np.float32), FIT_JAW_PRIOR)
            twin.append([v.numpy() for v in r])
    finally:
        torch.set_num_threads(threads)
    for name, got, k in (("rows", out, 0), ("jaw", jaw, 1), ("expression", psi, 2)):
        err, spread = np.abs(got - twin[0][k]), np.abs(twin[0][k] - twin[1][k])
        print(f"fit with free expression, {form}: {name} vs fp32 twin: max {err.max():.3e} q50 {np.quantile(err, 0.5):.3e} q99 {np.quantile(err, 0.99):.3e}"
              f"  fp32 twin, 1 thread vs 4: max {spread.max():.3e}")
        bar = 4.0 * spread.max()
        assert np.quantile(err, 0.5) < max(2e-5, bar) and np.quantile(err, 0.99) < max(3e-3, bar) and err.max() < max(0.1, bar)
    before, after = float(np.abs(psi_gt).mean()), float(np.abs(psi - psi_gt).mean())
    print(f"  mean |psi - psi_gt|: {before:.4f} at the start, {after:.4f} after the fit (twin {np.abs(twin[0][2] - psi_gt).mean():.4f})")
    assert after <= 0.5 * before


# ---- 6. an L-BFGS stage --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,with_jaw,max_rounds", [("kernel", False, 4000), ("panel", True, 4000), ("kernel", True, 28), ("panel", False, 28)])
def test_lbfgs_stage_with_free_expression_reports_the_specs_objective_at_the_returned_point(form, with_jaw, max_rounds, monkeypatch):
    """A stage that runs to its end (40 rounds here) and one cut short at 28 rounds, where 15 of the 16 frames wait inside a line search and
    are rolled back to their accepted points.  In both, every frame ends no higher than where it started and no higher than the same
    stage with psi fixed at zero.  The budget is not shorter because the second comparison has no meaning in a fit's first rounds: L-BFGS's
    first step is min(1, 1 / |g|_1) lr, which shrinks with every unknown the gradient gains, so the run with ten more unknowns starts
    with the shorter step and the two runs' accepted points are ordered only once both have left their first directions behind
    (measured with both runs cut at 3, 5, 7, 10, 14, 20 rounds: one to six frames up to 2.3 % higher with psi free)."""
    n = 16
    monkeypatch.setenv("FDCAP_KP_BLEND", form)
    m, init, kp, psi_gt, jaw_gt = _fit_case(n, 33, psi_sigma=1.0, noise=1.0)
    kp[2, :, 2] = 0.0
    kw = dict(keypoint_map=m[2], stages=(STAGE,), optimizer="lbfgs", lbfgs=dict(max_iter=10, max_steps=3), max_rounds=max_rounds)
    if with_jaw:
        kw.update(fit_jaw=True, jaw_prior=(W_JAW,))
    loss = {}
    for free in (False, True):
        op = InnerFitOP(m[0], m[1], n, fit_expression=free, expression_prior=(W_EXPR,) if free else None, **kw)
        op.fitting(init, kp)
        loss[free] = op.frame_loss[0]
        if free:
            x, psi = op.body_rotation_rec.detach().cpu().numpy(), op.expression.cpu().numpy()
            jaw = op.jaw_pose.cpu().numpy() if with_jaw else None
            back = ctypes.c_int32(-1)
            capi.check(op.ctx.lib.fdcap_opt_fit2d_lbfgs_rolled_back(op.ctx.handle, ctypes.byref(back)), "fdcap_opt_fit2d_lbfgs_rolled_back")
            rounds = op.rounds[0]
        op.close()
    t = lambda a: None if a is None else torch.tensor(a, dtype=torch.float64)
    with torch.no_grad():
        want = _spec(m).frame_loss(t(x), t(kp), STAGE, t(jaw), W_JAW if with_jaw else None, 0.0, t(psi), W_EXPR).numpy()
    rel = np.abs(loss[True] - want) / np.abs(want)
    print(f"L-BFGS with free expression, {form} jaw {with_jaw} max_rounds {max_rounds}: rounds {rounds}, rolled back {back.value}, objective rel err max {rel.max():.3e};"
          f" objective / objective with psi fixed: max {np.max(loss[True] / loss[False]):.4f} mean {np.mean(loss[True] / loss[False]):.4f}; |psi| max {np.abs(psi).max():.3f}")
    np.testing.assert_allclose(loss[True], want, rtol=2e-5)
    assert np.abs(psi).max() > 0
    if max_rounds < 100:
        assert rounds == max_rounds and back.value > 0       # (cut short inside line searches: psi is rolled back with its row)
    else:
        assert back.value == 0
    # no frame ends higher than it started (the accepted points of a line search only descend), nor higher than with psi fixed at zero
    # (2e-5: the loss sums' bar)
    x0 = rotrepr.convert_to_6D_rot(torch.tensor(init, dtype=torch.float64))
    with torch.no_grad():
        start = _spec(m).frame_loss(x0, t(kp), STAGE, t(np.zeros((n, 3))) if with_jaw else None, W_JAW if with_jaw else None, 0.0,
                                    t(np.zeros((n, NEXPR))), W_EXPR).numpy()
    print(f"  objective / start: max {np.max(loss[True] / np.maximum(start, 1e-30)):.4f}")
    assert np.all(loss[True] <= start * (1.0 + 2e-5))
    assert np.all(loss[True] <= loss[False] * (1.0 + 2e-5))


# ---- 7. the path of init=, and what is refused ------------------------------------------------------------------------------------------------------
def face_and_torso_map(bm):
    """face_map's keypoints and the shoulders and hips the start from keypoints alone reads (innerfit.DEFAULT_INIT)"""
    f = face_map(bm)
    return KeypointMap(np.concatenate([f.joint, [16, 17, 1, 2]]), np.concatenate([f.tri, np.zeros((4, 3), np.int32)]),
                       np.concatenate([f.bary, np.zeros((4, 3), np.float32)]))


def test_the_twin_select_path_leaves_the_chosen_problems_coefficients(monkeypatch):
    n = 3
    monkeypatch.setenv("FDCAP_KP_BLEND", "kernel")
    m, init, kp, psi_gt, jaw_gt = _fit_case(n, 41, kmap_of=face_and_torso_map)
    op = InnerFitOP(m[0], m[1], n, keypoint_map=m[2], stages=(STAGE, STAGE), iters_per_stage=4, fit_jaw=True, jaw_prior=(W_JAW, W_JAW),
                    fit_expression=True, expression_prior=(W_EXPR, W_EXPR), init={}, orientations="both")
    out = op.fitting(init, kp, expression_init=0.2 * psi_gt)
    psi, jaw, chosen, fl = op.expression.cpu().numpy(), op.jaw_pose.cpu().numpy(), op.chosen, op.final_loss.cpu().numpy()
    x_all = op.body_rotation_rec.detach().cpu().numpy()      # the n frames followed by their n twins
    op.close()
    assert psi.shape == (n, NEXPR) and fl.shape == (2 * n,) and x_all.shape == (2 * n, 78) and tuple(out.shape) == (n, 75)
    kept = np.where(chosen != 0, n + np.arange(n), np.arange(n))
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    with torch.no_grad():
        want = _spec(m).frame_loss(t(x_all[kept]), t(kp), STAGE, t(jaw), W_JAW, 0.0, t(psi), W_EXPR).numpy()
    print("init= with twins: chosen", chosen, "objective of the kept problems rel err", np.abs(fl[kept] - want) / np.abs(want))
    np.testing.assert_allclose(fl[kept], want, rtol=2e-5)    # the kept problem's rows, jaw AND coefficients


def test_what_the_expression_calls_refuse(monkeypatch):
    n = 2
    op, m, init, kp, psi, jaw = _open(n, 4, "kernel", monkeypatch, iters_per_stage=0)
    lib, h, st = op.ctx.lib, op.ctx.handle, capi.current_stream()
    buf = torch.empty(n, NEXPR, device="cuda")
    assert lib.fdcap_opt_set_expression(h, capi.dptr(_dev(psi)), st) == E_STATE          # no optimiser yet
    op.fitting(init, kp)
    assert lib.fdcap_opt_get_expression(h, capi.dptr(buf), None, st) == E_STATE          # no free expression
    assert lib.fdcap_opt_set_expression(h, capi.dptr(_dev(psi)), st) == 0
    assert lib.fdcap_opt_get_expression(h, None, None, st) == E_ARG
    assert lib.fdcap_opt_get_expression(h, None, capi.dptr(buf), st) == E_STATE          # no evaluation yet
    assert lib.fdcap_opt_get_expression(h, capi.dptr(buf), None, st) == 0
    for w in (float("nan"), float("inf")):
        assert lib.fdcap_opt_set_expression_prior(h, w) == E_ARG
    assert lib.fdcap_opt_set_expression_prior(h, 2.0) == 0
    sg = capi.Fit2dStage(692, 692, 640, 360, 100.0, *STAGE)
    # the 23-joint layout, at the evaluation
    kp23 = _dev(np.concatenate([kp, kp], 1)[:, :23])
    capi.check(lib.fdcap_opt_set_keypoints(h, capi.dptr(kp23), st), "fdcap_opt_set_keypoints")
    assert lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 0, st) == E_STATE
    capi.check(lib.fdcap_opt_set_keypoints_mapped(h, capi.dptr(_dev(kp)), st), "fdcap_opt_set_keypoints_mapped")
    assert lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 0, st) == 0
    assert lib.fdcap_opt_get_expression(h, None, capi.dptr(buf), st) == 0
    op.close()
    # the self-interpenetration term, on a body with a surface and its mesh registered (the jaw shut): with free expression the
    # term's setter refuses, and with the term set first and the coefficients freed afterwards the evaluation does
    bmm, part, parent = synth.make_body_mesh(300, seed=7, lbs_nnz=4)
    ids = np.random.Generator(np.random.PCG64(5)).permutation(bmm.num_verts)
    kmm = KeypointMap([3, 15, 20] + [-1] * 6, [(0, 0, 0)] * 3 + [(int(v),) * 3 for v in ids[:6]], [(0, 0, 0)] * 3 + [(1, 0, 0)] * 6)
    kpm = np.ascontiguousarray(np.concatenate([kp, kp], 1)[:, :len(kmm)])
    opc = InnerFitOP(bmm, m[1], n, keypoint_map=kmm, iters_per_stage=0, collision=dict(face_part=part, part_parent=parent, weights=(0.0,) * 5))
    opc.fitting(init, kpm)
    lc, hc = opc.ctx.lib, opc.ctx.handle
    prm = capi.CollisionParams(0.5, 1.0, 4096, 0)
    assert lc.fdcap_opt_set_fit2d_collision(hc, ctypes.byref(prm)) == 0                  # (the mesh is there and the term is accepted)
    assert lc.fdcap_opt_set_fit2d_collision(hc, None) == 0
    assert lc.fdcap_opt_set_expression(hc, capi.dptr(_dev(psi)), st) == 0
    assert lc.fdcap_opt_set_fit2d_collision(hc, ctypes.byref(prm)) == E_STATE            # free expression: refused
    assert lc.fdcap_opt_backward_fit2d(hc, ctypes.byref(sg), 0, st) == 0                 # (the term is still off)
    assert lc.fdcap_opt_set_expression(hc, None, st) == 0
    assert lc.fdcap_opt_set_fit2d_collision(hc, ctypes.byref(prm)) == 0                  # fixed at zero again: accepted
    assert lc.fdcap_opt_backward_fit2d(hc, ctypes.byref(sg), 0, st) == 0
    assert lc.fdcap_opt_set_expression(hc, capi.dptr(_dev(psi)), st) == 0                # the term first, the coefficients freed afterwards
    assert lc.fdcap_opt_backward_fit2d(hc, ctypes.byref(sg), 0, st) == E_STATE
    assert lc.fdcap_opt_set_expression(hc, None, st) == 0
    assert lc.fdcap_opt_backward_fit2d(hc, ctypes.byref(sg), 0, st) == 0
    torch.cuda.synchronize()
    opc.close()
    # a model without expression directions
    bm10 = synth.make_body_model(240, seed=7, lbs_nnz=4)
    bm10.shapedirs = np.ascontiguousarray(np.asarray(bm10.shapedirs)[:, :, :10])
    op10 = InnerFitOP(bm10, m[1], n, keypoint_map=m[2], iters_per_stage=0)
    op10.fitting(init, kp)
    assert op10.ctx.lib.fdcap_opt_set_expression(op10.ctx.handle, capi.dptr(_dev(psi)), st) == E_STATE
    op10.close()
    with pytest.raises(capi.FdcapError):
        InnerFitOP(bm10, m[1], n, keypoint_map=m[2], fit_expression=True)
    # the Python side: no map, the collision term
    with pytest.raises(capi.FdcapError):
        InnerFitOP(m[0], m[1], n, fit_expression=True)
    with pytest.raises(capi.FdcapError):
        InnerFitOP(m[0], m[1], n, keypoint_map=m[2], fit_expression=True, collision={})
    with pytest.raises(capi.FdcapError):
        InnerFitOP(m[0], m[1], n, keypoint_map=m[2], expression_prior=(1.0,) * 5)


def test_a_batch_of_clips_refuses_free_expression():
    bm, vp = _models(7, 4)
    ctx = capi.Context(bm, vp)
    N, K, st = 6, 2, capi.current_stream()
    oc = capi.OptConfig(N, N, 0, 0.01, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)
    state = [torch.zeros(K * N + 4, 78, device="cuda"), torch.zeros(K * N + 4, 16, device="cuda"), torch.ones(K, device="cuda"),
             torch.zeros(K, device="cuda"), torch.zeros(K, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)]
    ctx.set_scene(np.zeros((0, 3), np.float32))
    assert ctx.lib.fdcap_opt_create_clips(ctx.handle, ctypes.byref(oc), K, *[capi.dptr(t) for t in state]) == 0
    assert ctx.lib.fdcap_opt_set_expression(ctx.handle, capi.dptr(torch.zeros(K * N, NEXPR, device="cuda")), st) == E_STATE
    assert ctx.lib.fdcap_opt_set_expression_prior(ctx.handle, 1.0) == E_STATE
    torch.cuda.synchronize()
    ctx.close()
