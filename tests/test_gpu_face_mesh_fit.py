"""GPU tests of the inner fit's self-interpenetration term ON THE FITTED FACE (fdcap_opt_set_fit2d_collision_face,
InnerFitOP(collision=dict(..., follow_face=True), fit_jaw=..., fit_expression=...)) through the C-ABI, against the fp64 twin
tests/face_mesh_spec.fit_spec: tests/expression_spec.ExpressionSpec's objective plus tests/collision_spec.penalty on ExprBody's vertices
under the jaw and psi.  In the pattern of tests/test_gpu_collision_fit.py: the body is synth.make_body_mesh(300) (496 vertices on tubes
around the bones, 64 of them skinned to the jaw; parts by bone, a part not tested against itself or its parent), capacity 2048, sigma 0.5,
w_coll 30; the jaw is open by 0.3 rad, psi ~ N(0, 1.5^2).

Bars.  Logged sums, the per-frame objective and every gradient block -- the rows' column blocks, "psi" and "jaw" -- are held at
tests/gradient_bars.py's formula 32 max(max|g32 - g64|, 2^-24 max|g64|) from the twin's two precisions, which must find the same pair
sets; every frame must have a pair and none more than the capacity; the term must reach psi and the jaw.  No bar is taken from a HIP
result."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.innerfit import DEFAULT_BEND_RATIO, DEFAULT_BEND_TERMS, DEFAULT_STAGES, InnerFitOP, KeypointMap, collision_filter
from oracle import rotrepr
from tests import face_mesh_spec as fs
from tests import gradient_bars as gb

pytestmark = pytest.mark.gpu
STAGE = (1.0, 4.78, 5.0, 4.78)
ALONE = (1.0, 0.0, 0.0, 0.0)
W_JAW, W_EXPR, W_BEND = (47.8, 478.0, 478.0), 5.0, DEFAULT_BEND_RATIO * STAGE[1]
SIGMA, W_COLL, CAPACITY = 0.5, 30.0, 2048
E_ARG, E_STATE = -1, -2
SLOT = 4                                                     # FDCAP_LOSS_FIT2D_COLLISION
SEED = 7


@functools.lru_cache(maxsize=None)
def _models(lbs_nnz):
    bm, part, parent = synth.make_body_mesh(300, seed=SEED, lbs_nnz=lbs_nnz)
    return bm, synth.make_vposer(seed=SEED + 1), part, parent


def vertex_map(bm):
    """joints 3, 15 and 20, six plain vertices, two surface points (tests/test_gpu_collision_fit.py's map)"""
    rng = np.random.Generator(np.random.PCG64(500))
    ids = rng.permutation(bm.num_verts)
    joint = [3, 15, 20] + [-1] * 8
    tri = [(0, 0, 0)] * 3 + [(int(v),) * 3 for v in ids[:6]] + [tuple(int(v) for v in ids[6:9]), tuple(int(v) for v in ids[9:12])]
    bary = [(0, 0, 0)] * 3 + [(1, 0, 0)] * 6 + [tuple(rng.dirichlet((1.0, 1.0, 1.0))) for _ in range(2)]
    return KeypointMap(joint, tri, bary)


def _case(n, lbs_nnz):
    bm, vp, part, parent = _models(lbs_nnz)
    kmap = vertex_map(bm)
    clip = synth.make_clip(n, seed=SEED + 2, num_outliers=0)
    rng = np.random.Generator(np.random.PCG64(SEED + 3))
    gt = clip.body_params.astype(np.float32).copy()
    gt[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32) + 0.05 * rng.standard_normal((n, 3)).astype(np.float32)
    jaw = rng.standard_normal((n, 3))
    jaw = (0.3 * jaw / np.linalg.norm(jaw, axis=1, keepdims=True)).astype(np.float32)
    psi = (1.5 * rng.standard_normal((n, 10))).astype(np.float32)
    ign = collision_filter(part, parent)
    s64 = fs.fit_spec(bm, vp, kmap, bm.faces, part, ign)
    with torch.no_grad():
        uv = s64.project(s64.joints_cam(rotrepr.convert_to_6D_rot(torch.tensor(gt, dtype=torch.float64)), torch.tensor(jaw, dtype=torch.float64),
                                        torch.tensor(psi, dtype=torch.float64))).numpy()
    kp = np.concatenate([uv + 2.0 * rng.standard_normal(uv.shape), rng.uniform(0.3, 1.0, (n, len(kmap), 1))], -1).astype(np.float32)
    init = gt.copy()
    init[:, 3:6] += 0.1 * rng.standard_normal((n, 3)).astype(np.float32)
    init[:, 16:48] += 0.4 * rng.standard_normal((n, 32)).astype(np.float32)
    init[:, 72:75] += 0.05 * rng.standard_normal((n, 3)).astype(np.float32)
    return bm, vp, part, parent, ign, kmap, init, kp, jaw, psi


def _coll(part, parent, weights=None, stages=DEFAULT_STAGES, **kw):
    return dict(face_part=part, part_parent=parent, sigma=SIGMA, weights=(W_COLL,) * len(stages) if weights is None else weights, capacity=CAPACITY, **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _set_face(op, jaw, psi, w_jaw, w_expr, w_bend):
    """jaw / psi: numpy arrays or None (not free in this case)"""
    lib, h, st = op.ctx.lib, op.ctx.handle, capi.current_stream()
    if jaw is not None:
        capi.check(lib.fdcap_opt_set_jaw(h, capi.dptr(_dev(jaw)), st), "fdcap_opt_set_jaw")
    if psi is not None:
        capi.check(lib.fdcap_opt_set_expression(h, capi.dptr(_dev(psi)), st), "fdcap_opt_set_expression")
        capi.check(lib.fdcap_opt_set_expression_prior(h, float(w_expr)), "fdcap_opt_set_expression_prior")
    ex = capi.Fit2dExtra()
    if w_bend:
        ex.w_bend, ex.n_bend = w_bend, len(DEFAULT_BEND_TERMS)
        for t, (j, a, s) in enumerate(DEFAULT_BEND_TERMS):
            ex.joint[t], ex.axis[t], ex.sign[t] = j, a, s
    ex.w_jaw[0], ex.w_jaw[1], ex.w_jaw[2] = w_jaw
    capi.check(lib.fdcap_opt_set_fit2d_extra(h, ctypes.byref(ex)), "fdcap_opt_set_fit2d_extra")


def _evaluate(op, n, stage, jaw_free, psi_free):
    """-> losses [8], per-frame objective [n], {"rows", "jaw", "psi"} gradients"""
    lib, h, st = op.ctx.lib, op.ctx.handle, capi.current_stream()
    sg = capi.Fit2dStage(692, 692, 640, 360, 100.0, *stage)
    capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 1, st), "backward_fit2d")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, st), "get_grads")
    g = {"rows": dx.cpu().numpy()}
    if jaw_free:
        dj = torch.empty(n, 3, device="cuda")
        capi.check(lib.fdcap_opt_get_jaw(h, None, capi.dptr(dj), st), "get_jaw")
        g["jaw"] = dj.cpu().numpy()
    if psi_free:
        dp = torch.empty(n, 10, device="cuda")
        capi.check(lib.fdcap_opt_get_expression(h, None, capi.dptr(dp), st), "get_expression")
        g["psi"] = dp.cpu().numpy()
    losses = op._losses.cpu().numpy().copy()
    fl = torch.empty(n, device="cuda")
    capi.check(lib.fdcap_opt_fit2d_frame_loss(h, ctypes.byref(sg), capi.dptr(fl), st), "frame_loss")
    return losses, fl.cpu().numpy(), g


def _blocks(g):
    out = gb.blocks(rows=g["rows"])
    out.update({k: np.asarray(g[k], dtype=np.float64) for k in ("jaw", "psi") if k in g})
    return out


def _fbar(f32, f64):
    return gb.M * max(float(np.abs(f32 - f64).max()), gb.EPS32 * float(np.abs(f64).max()))


# ---- 1. evaluations ------------------------------------------------------------------------------------------------------------------------
CASES = [(1, 4, "kernel", "jaw", False), (3, 8, "kernel", "psi", False), (3, 4, "kernel", "both", True), (1, 8, "kernel", "both", False),
         (1, 4, "panel", "psi", False), (3, 8, "panel", "jaw", False), (1, 8, "panel", "both", True), (3, 4, "panel", "both", False)]


@pytest.mark.parametrize("n,lbs_nnz,form,face,bend", CASES)
def test_evaluation_with_the_term_on_the_fitted_face_matches_fp64_autograd(n, lbs_nnz, form, face, bend, monkeypatch):
    monkeypatch.setenv("FDCAP_KP_BLEND", form)
    bm, vp, part, parent, ign, kmap, init, kp, jaw, psi = _case(n, lbs_nnz)
    jaw_free, psi_free = face != "psi", face != "jaw"
    jw, ps = (jaw if jaw_free else None), (psi if psi_free else None)
    op = InnerFitOP(bm, vp, n, keypoint_map=kmap, iters_per_stage=0, fit_jaw=jaw_free, fit_expression=psi_free,
                    collision=_coll(part, parent, follow_face=True))
    op.fitting(init, kp)
    x = op.body_rotation_rec.detach().cpu().numpy()
    twins = {d: fs.fit_spec(bm, vp, kmap, bm.faces, part, ign, dtype=d) for d in (torch.float64, torch.float32)}
    w_bend = W_BEND if bend else 0.0
    zero3 = (0.0, 0.0, 0.0)
    _, _, g_alone = twins[torch.float64].grads_coll(x, kp * np.array([1, 1, 0], np.float32), ALONE, SIGMA, W_COLL, jw, zero3, 0.0, ps, 0.0)
    for label, stage, kpx, wj, we, wb in (("the term alone", ALONE, kp * np.array([1, 1, 0], np.float32), zero3, 0.0, 0.0),
                                          ("whole objective", STAGE, kp, W_JAW, W_EXPR, w_bend)):
        if label == "the term alone" and bend:
            continue                                           # (alone means alone: the cases without the prior)
        capi.check(op.ctx.lib.fdcap_opt_set_keypoints_mapped(op.ctx.handle, capi.dptr(_dev(kpx)), capi.current_stream()), "set_keypoints")
        _set_face(op, jw, ps, wj, we, wb)
        losses, fl, g = _evaluate(op, n, stage, jaw_free, psi_free)
        s64, f64, g64 = twins[torch.float64].grads_coll(x, kpx, stage, SIGMA, W_COLL, jw, wj, wb, ps, we)
        s32, f32, g32 = twins[torch.float32].grads_coll(x, kpx, stage, SIGMA, W_COLL, jw, wj, wb, ps, we)
        sets = twins[torch.float64].last_pairs
        assert sets == twins[torch.float32].last_pairs, "the twin's two precisions find different pairs: take another seed"
        assert all(0 < len(p) <= CAPACITY for p in sets) and s64[2] > 0
        bar = gb.bars(_blocks(g32), _blocks(g64))
        r = gb.ratios(_blocks(g), _blocks(g64), bar)
        fbar = _fbar(f32, f64)
        sbar = gb.M * np.maximum(np.abs(s32 - s64), gb.EPS32 * np.abs(s64))
        got = np.array([losses[0], losses[1], losses[SLOT]])
        share = {k: float(np.abs(g_alone[k]).max() / np.abs(g64[k]).max()) for k in ("jaw", "psi") if k in g64}
        print(f"{label}, n {n} lbs_nnz {lbs_nnz} {form} {face} bend {bend}: pairs {[len(p) for p in sets]} sums {got} err/bar "
              f"{np.abs(got - s64) / np.maximum(sbar, 1e-300)} frame objective err/bar {np.abs(fl - f64).max() / fbar:.3g} gradient max|err| / bar",
              {k: f"{v:.3g}" for k, v in r.items()}, "the term's max|g| over this objective's:", share)
        assert all(np.abs(g_alone[k]).max() > 0 for k in share)                  # the term reaches the jaw and psi
        assert np.all(np.abs(got - s64) <= sbar), (got, s64, sbar)
        assert np.abs(fl - f64).max() <= fbar
        assert all(v <= 1.0 for v in r.values()), r
        if label == "the term alone":
            assert got[0] == 0.0 and got[1] == 0.0
    op.close()


# ---- 2. fits ---------------------------------------------------------------------------------------------------------------------------------
def _twin_objective(m, x, kp, stage, jaw, psi, w_jaw, w_expr, w_bend, w_coll=W_COLL):
    bm, vp, part, ign, kmap = m
    out = []
    for d in (torch.float64, torch.float32):
        t = fs.fit_spec(bm, vp, kmap, bm.faces, part, ign, dtype=d)
        c = lambda a: torch.tensor(np.asarray(a), dtype=d)
        with torch.no_grad():
            out.append(t.objective(c(x), c(kp), stage, SIGMA, w_coll, c(jaw), w_jaw, w_bend, c(psi), w_expr).numpy().astype(np.float64))
        out.append(t.last_pairs)
    assert out[1] == out[3], "the twin's two precisions find different pairs: take another seed"
    print("pairs at the returned point:", [len(p) for p in out[1]])
    assert all(0 < len(p) <= CAPACITY for p in out[1]), "a frame without a pair, or with more than the list holds: take another start"
    return out[0], out[2]


def test_adam_fit_reports_the_twins_objective_at_the_returned_rows_psi_and_jaw(monkeypatch):
    monkeypatch.setenv("FDCAP_KP_BLEND", "kernel")
    n = 3
    bm, vp, part, parent, ign, kmap, init, kp, jaw, psi = _case(n, 4)
    op = InnerFitOP(bm, vp, n, keypoint_map=kmap, iters_per_stage=3, fit_jaw=True, fit_expression=True, collision=_coll(part, parent, follow_face=True))
    psi = 0.5 * psi                                           # (1 071 .. 1 262 pairs per frame at the start: room under the capacity for the steps)
    op.fitting(init, kp, jaw_init=jaw, expression_init=psi)
    x, jw, ps = op.body_rotation_rec.detach().cpu().numpy(), op.jaw_pose.cpu().numpy(), op.expression.cpu().numpy()
    assert np.abs(jw - jaw).max() > 0 and np.abs(ps - psi).max() > 0
    fl = torch.empty(n, device="cuda")
    capi.check(op.ctx.lib.fdcap_opt_fit2d_frame_loss(op.ctx.handle, ctypes.byref(op._last_stage), capi.dptr(fl), capi.current_stream()), "frame_loss")
    si = len(DEFAULT_STAGES) - 1
    stage = DEFAULT_STAGES[si]
    f64, f32 = _twin_objective((bm, vp, part, ign, kmap), x, kp, stage, jw, ps, tuple(op.jaw_prior[si]), float(op.expression_prior[si]), 0.0)
    err, bar = float(np.abs(fl.cpu().numpy() - f64).max()), _fbar(f32, f64)
    print(f"Adam with the term on the fitted face: reported objective max|err| {err:.3e} bar {bar:.3e} of {f64}")
    assert err <= bar
    op.close()


def test_lbfgs_stage_reports_the_twins_objective_at_the_returned_rows_psi_and_jaw(monkeypatch):
    monkeypatch.setenv("FDCAP_KP_BLEND", "kernel")
    n = 3
    bm, vp, part, parent, ign, kmap, init, kp, jaw, psi = _case(n, 4)
    op = InnerFitOP(bm, vp, n, keypoint_map=kmap, stages=(STAGE,), optimizer="lbfgs", lbfgs=dict(max_iter=8, max_steps=2), fit_jaw=True,
                    fit_expression=True, jaw_prior=(W_JAW,), expression_prior=(W_EXPR,), collision=_coll(part, parent, stages=(STAGE,), follow_face=True))
    psi = 0.5 * psi                                           # (1 071 .. 1 262 pairs per frame at the start: room under the capacity for the steps)
    op.fitting(init, kp, jaw_init=jaw, expression_init=psi)
    x, jw, ps = op.body_rotation_rec.detach().cpu().numpy(), op.jaw_pose.cpu().numpy(), op.expression.cpu().numpy()
    f64, f32 = _twin_objective((bm, vp, part, ign, kmap), x, kp, STAGE, jw, ps, W_JAW, W_EXPR, 0.0)
    got = np.asarray(op.frame_loss[0], dtype=np.float64)
    err, bar = float(np.abs(got - f64).max()), _fbar(f32, f64)
    print(f"L-BFGS with the term on the fitted face: rounds {op.rounds} reported loss max|err| {err:.3e} bar {bar:.3e} of {f64}")
    assert np.abs(jw - jaw).max() > 0 and np.abs(ps - psi).max() > 0
    assert err <= bar
    op.close()


def _fit_bits(op, init, kp, **kw):
    rows = op.fitting(init, kp, **kw).cpu().numpy()
    out = [rows, op.body_rotation_rec.detach().cpu().numpy().copy()]
    if op.fit_jaw:
        out.append(op.jaw_pose.cpu().numpy())
    if op.fit_expression:
        out.append(op.expression.cpu().numpy())
    op.close()
    return out


@pytest.mark.parametrize("form", ["kernel", "panel"])
def test_follow_face_with_the_face_fixed_gives_the_bits_of_the_collision_fit_without_it(form, monkeypatch):
    monkeypatch.setenv("FDCAP_KP_BLEND", form)
    n = 3
    bm, vp, part, parent, ign, kmap, init, kp, jaw, psi = _case(n, 4)
    a = _fit_bits(InnerFitOP(bm, vp, n, keypoint_map=kmap, iters_per_stage=3, collision=_coll(part, parent)), init, kp)
    b = _fit_bits(InnerFitOP(bm, vp, n, keypoint_map=kmap, iters_per_stage=3, collision=_coll(part, parent, follow_face=True)), init, kp)
    plain = _fit_bits(InnerFitOP(bm, vp, n, keypoint_map=kmap, iters_per_stage=3), init, kp)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], plain[0])                  # (the term was on in both)


@pytest.mark.parametrize("form", ["kernel", "panel"])
def test_the_term_off_gives_the_bits_of_a_context_that_never_called_the_setter(form, monkeypatch):
    monkeypatch.setenv("FDCAP_KP_BLEND", form)
    n = 3
    bm, vp, part, parent, ign, kmap, init, kp, jaw, psi = _case(n, 4)
    kw = dict(keypoint_map=kmap, iters_per_stage=3, fit_jaw=True, fit_expression=True)
    a = _fit_bits(InnerFitOP(bm, vp, n, **kw), init, kp, jaw_init=jaw, expression_init=psi)
    b = _fit_bits(InnerFitOP(bm, vp, n, collision=_coll(part, parent, weights=(0.0,) * 5, follow_face=True), **kw), init, kp, jaw_init=jaw,
                  expression_init=psi)
    on = _fit_bits(InnerFitOP(bm, vp, n, collision=_coll(part, parent, follow_face=True), **kw), init, kp, jaw_init=jaw, expression_init=psi)
    assert len(a) == 4 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], on[0]) and not np.array_equal(a[2], on[2]) and not np.array_equal(a[3], on[3])     # rows, jaw, psi move under the term
