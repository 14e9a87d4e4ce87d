"""GPU tests of the inner fit's self-interpenetration term (fdcap_opt_set_fit2d_collision, InnerFitOP(collision=...)) through the C-ABI,
against the fp64 twin tests/collision_spec.fit_spec.  The body is synth.make_body_mesh(300): 496 vertices on tubes around the bones, 558
faces, parts by bone; a part is not tested against itself or its parent part, and what is left collides in every pose of these cases
(the tubes of the collar bones and the upper arms run through the torso's): the pair sets are asserted non-empty.

Bars.  The term alone (no confidence, no prior: nothing larger to hide behind) and the whole objective are both held at
tests/gradient_bars.py's formula per column block, from the twin's two precisions, which must find the same pair sets.  No bar is
taken from a HIP result."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.innerfit import DEFAULT_BEND_RATIO, DEFAULT_BEND_TERMS, DEFAULT_STAGES, InnerFitOP, KeypointMap, collision_filter
from oracle import rotrepr
from tests import collision_spec as spec
from tests import gradient_bars as gb

pytestmark = pytest.mark.gpu
STAGE = (1.0, 4.78, 5.0, 4.78)
W_BEND = DEFAULT_BEND_RATIO * STAGE[1]
SIGMA, W_COLL = 0.5, 30.0
E_ARG, E_STATE = -1, -2
SLOT = 4                                                     # FDCAP_LOSS_FIT2D_COLLISION


@functools.lru_cache(maxsize=None)
def _models(seed, lbs_nnz):
    bm, part, parent = synth.make_body_mesh(300, seed=seed, lbs_nnz=lbs_nnz)
    return bm, synth.make_vposer(seed=seed + 1), part, parent


def vertex_map(bm, seed=0):
    """joints 3, 15 and 20, six plain vertices, two surface points"""
    rng = np.random.Generator(np.random.PCG64(500 + seed))
    ids = rng.permutation(bm.num_verts)
    joint = [3, 15, 20] + [-1] * 8
    tri = [(0, 0, 0)] * 3 + [(int(v),) * 3 for v in ids[:6]] + [tuple(int(v) for v in ids[6:9]), tuple(int(v) for v in ids[9:12])]
    bary = [(0, 0, 0)] * 3 + [(1, 0, 0)] * 6 + [tuple(rng.dirichlet((1.0, 1.0, 1.0))) for _ in range(2)]
    return KeypointMap(joint, tri, bary)


def _case(n, seed, lbs_nnz, path):
    bm, vp, part, parent = _models(seed, lbs_nnz)
    kmap = KeypointMap.joints23() if path == "joints23" else vertex_map(bm)
    clip = synth.make_clip(n, seed=seed + 2, num_outliers=0)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    gt = clip.body_params.astype(np.float32).copy()
    gt[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32) + 0.05 * rng.standard_normal((n, 3)).astype(np.float32)
    ign = collision_filter(part, parent)
    s64 = spec.fit_spec(bm, vp, kmap, bm.faces, part, ign)
    with torch.no_grad():
        uv = s64.project(s64.joints_cam(rotrepr.convert_to_6D_rot(torch.tensor(gt, dtype=torch.float64)))).numpy()
    kp = np.concatenate([uv + 2.0 * rng.standard_normal(uv.shape), rng.uniform(0.3, 1.0, (n, len(kmap), 1))], -1).astype(np.float32)
    init = gt.copy()
    init[:, 3:6] += 0.1 * rng.standard_normal((n, 3)).astype(np.float32)
    init[:, 16:48] += 0.4 * rng.standard_normal((n, 32)).astype(np.float32)
    init[:, 72:75] += 0.05 * rng.standard_normal((n, 3)).astype(np.float32)
    return bm, vp, part, parent, ign, kmap, init, kp


def _open(n, lbs_nnz, path, monkeypatch, seed=7, collision=True, **kw):
    monkeypatch.setenv("FDCAP_KP_BLEND", path if path in ("kernel", "panel") else "kernel")
    bm, vp, part, parent, ign, kmap, init, kp = _case(n, seed, lbs_nnz, path)
    if collision:
        kw["collision"] = dict(face_part=part, part_parent=parent, sigma=SIGMA, weights=(W_COLL,) * len(kw.get("stages", DEFAULT_STAGES)), capacity=2048)
    op = InnerFitOP(bm, vp, n, keypoint_map=None if path == "joints23" else kmap, **kw)
    return op, (bm, vp, part, ign, kmap), init, kp


def _set_coll(op, prm):
    return op.ctx.lib.fdcap_opt_set_fit2d_collision(op.ctx.handle, None if prm is None else ctypes.byref(capi.CollisionParams(*prm)))


def _set_bend(op, w_bend):
    ex = capi.Fit2dExtra()
    ex.w_bend, ex.n_bend = w_bend, len(DEFAULT_BEND_TERMS)
    for t, (j, a, s) in enumerate(DEFAULT_BEND_TERMS):
        ex.joint[t], ex.axis[t], ex.sign[t] = j, a, s
    assert op.ctx.lib.fdcap_opt_set_fit2d_extra(op.ctx.handle, ctypes.byref(ex)) == 0


def _evaluate(op, n, stage=STAGE):
    """-> losses [8], per-frame objective [n], gradient [n, 78]"""
    lib, h = op.ctx.lib, op.ctx.handle
    sg = capi.Fit2dStage(692, 692, 640, 360, 100.0, *stage)
    capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 1, capi.current_stream()), "backward_fit2d")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, capi.current_stream()), "get_grads")
    losses = op._losses.cpu().numpy().copy()
    fl = torch.empty(n, device="cuda")
    capi.check(lib.fdcap_opt_fit2d_frame_loss(h, ctypes.byref(sg), capi.dptr(fl), capi.current_stream()), "frame_loss")
    return losses, fl.cpu().numpy(), dx.cpu().numpy()


CASES = [(1, 4, "joints23", False), (3, 8, "joints23", True), (3, 4, "kernel", True), (1, 8, "kernel", False), (3, 4, "panel", False),
         (1, 8, "panel", True), (3, 8, "panel", True), (3, 4, "joints23", True)]


@pytest.mark.parametrize("n,lbs_nnz,path,bend", CASES)
def test_evaluation_with_the_term_matches_fp64_autograd(n, lbs_nnz, path, bend, monkeypatch):
    op, (bm, vp, part, ign, kmap), init, kp = _open(n, lbs_nnz, path, monkeypatch, iters_per_stage=0)
    op.fitting(init, kp)
    x = op.body_rotation_rec.detach().cpu().numpy()
    twins = {d: spec.fit_spec(bm, vp, kmap, bm.faces, part, ign, dtype=d) for d in (torch.float64, torch.float32)}
    w_bend = W_BEND if bend else 0.0
    if bend:
        _set_bend(op, w_bend)
    for label, stage, kpx in (("the term alone", (1.0, 0.0, 0.0, 0.0), kp * np.array([1, 1, 0], np.float32)), ("whole objective", STAGE, kp)):
        if label == "the term alone" and bend:
            continue                                           # (alone means alone: the cases without the prior)
        kd = torch.tensor(kpx, device="cuda").contiguous()
        setter = op.ctx.lib.fdcap_opt_set_keypoints if path == "joints23" else op.ctx.lib.fdcap_opt_set_keypoints_mapped
        capi.check(setter(op.ctx.handle, capi.dptr(kd), capi.current_stream()), "set_keypoints")
        losses, fl, dx = _evaluate(op, n, stage)
        s64, f64, g64 = twins[torch.float64].grads_coll(x, kpx, stage, SIGMA, W_COLL, w_bend)
        s32, f32, g32 = twins[torch.float32].grads_coll(x, kpx, stage, SIGMA, W_COLL, w_bend)
        sets = twins[torch.float64].last_pairs
        assert sets == twins[torch.float32].last_pairs, "the twin's two precisions find different pairs: take another seed"
        assert all(len(p) > 0 for p in sets) and s64[2] > 0
        bar = gb.bars(gb.blocks(rows=g32), gb.blocks(rows=g64))
        r = gb.ratios(gb.blocks(rows=dx), gb.blocks(rows=g64), bar)
        fbar = gb.M * max(float(np.abs(f32 - f64).max()), gb.EPS32 * float(np.abs(f64).max()))
        sbar = gb.M * np.maximum(np.abs(s32 - s64), gb.EPS32 * np.abs(s64))
        got = np.array([losses[0], losses[1], losses[SLOT]])
        print(f"{label}, n {n} lbs_nnz {lbs_nnz} path {path} bend {bend}: pairs {[len(p) for p in sets]} sums {got} err/bar {np.abs(got - s64) / np.maximum(sbar, 1e-300)}"
              f" frame objective err/bar {np.abs(fl - f64).max() / fbar:.3g}  gradient max|err| / bar", {k: f"{v:.3g}" for k, v in r.items()},
              " share of the term in max|g|:", float(np.abs(g64).max()))
        assert np.all(np.abs(got - s64) <= sbar), (got, s64, sbar)
        assert np.abs(fl - f64).max() <= fbar
        assert all(v <= 1.0 for v in r.values()), r
        if label == "the term alone":
            assert got[0] == 0.0 and got[1] == 0.0
    op.close()


def _manual_fit(op, n, iters=3):
    lib, h = op.ctx.lib, op.ctx.handle
    for stage in DEFAULT_STAGES:
        sg = capi.Fit2dStage(692, 692, 640, 360, 100.0, *stage)
        capi.check(lib.fdcap_opt_reset_adam(h, capi.current_stream()), "reset_adam")
        for it in range(iters):
            capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 0, capi.current_stream()), "backward_fit2d")
            capi.check(lib.fdcap_opt_step_x(h, it + 1, capi.current_stream()), "step_x")
    return op.body_rotation_rec.detach().cpu().numpy().copy()


@pytest.mark.parametrize("path", ["kernel", "panel", "joints23"])
def test_switched_off_again_gives_the_bits_of_a_context_that_never_called(path, monkeypatch):
    n = 3
    res = []
    for touch in (False, True):
        op, _, init, kp = _open(n, 4, path, monkeypatch, collision=touch, iters_per_stage=0)
        op.fitting(init, kp)
        if touch:
            on = _evaluate(op, n)
            assert _set_coll(op, None) == 0
        ev = _evaluate(op, n)
        if touch:                                              # weight 0: off as well
            assert _set_coll(op, (SIGMA, 0.0, 2048, 0)) == 0
            zero = _evaluate(op, n)
        res.append(ev + (_manual_fit(op, n),))
        op.close()
    assert on[0][SLOT] > 0 and not np.array_equal(on[2], res[0][2]) and not np.array_equal(on[1], res[0][1])
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    for a, b in zip(res[0][:3], zero):
        assert np.array_equal(a, b)
    assert res[0][0][SLOT] == 0.0


def test_five_stage_fit_with_the_term_matches_the_twin_and_lowers_the_penalty(monkeypatch):
    """HIP fit's distance from the fp64 twin's fit <= 4 x the fp32 twin's distance from it (the factor covers a different summation
    order).  Measured: HIP 4.66e-6, fp32 twin 5.18e-6, ratio 0.90.  The twin's E at the final rows, at weight 1, is lower with the term than without."""
    n, iters = 3, 4
    weights = (0.0, 0.0, 0.0, 3.0, 30.0)
    bm, vp, part, parent, ign, kmap, init, kp = _case(n, 7, 4, "kernel")
    monkeypatch.setenv("FDCAP_KP_BLEND", "kernel")
    op = InnerFitOP(bm, vp, n, keypoint_map=kmap, iters_per_stage=iters,
                    collision=dict(face_part=part, part_parent=parent, sigma=SIGMA, weights=weights, capacity=2048))
    out = op.fitting(init, kp).cpu().numpy()
    op.close()
    plain = InnerFitOP(bm, vp, n, keypoint_map=kmap, iters_per_stage=iters)
    out_plain = plain.fitting(init, kp).cpu().numpy()
    plain.close()
    t64, t32 = (spec.fit_spec(bm, vp, kmap, bm.faces, part, ign, dtype=d) for d in (torch.float64, torch.float32))
    f64, f32 = t64.fit_coll(init, kp, DEFAULT_STAGES, iters, SIGMA, weights).numpy(), t32.fit_coll(init, kp, DEFAULT_STAGES, iters, SIGMA, weights).numpy()
    assert t64.visited == t32.visited and len(t64.visited) == 2 * iters, "the twin's two precisions visit different pair sets: take another seed"
    d_hip, d_32 = np.abs(out - f64).max(), np.abs(f32 - f64).max()
    print(f"fit with the term: HIP vs fp64 twin {d_hip:.3e}, fp32 twin vs fp64 twin {d_32:.3e}, ratio {d_hip / d_32:.2f}; moved by the term {np.abs(out - out_plain).max():.3e}")
    assert d_hip <= 4.0 * d_32
    with torch.no_grad():
        e_on = t64.collision(rotrepr.convert_to_6D_rot(torch.tensor(out, dtype=torch.float64)), SIGMA, 1.0).numpy()
        e_off = t64.collision(rotrepr.convert_to_6D_rot(torch.tensor(out_plain, dtype=torch.float64)), SIGMA, 1.0).numpy()
    print("the twin's E at the final rows, weight 1: with the term", e_on, "without", e_off)
    assert e_on.sum() < e_off.sum() and np.abs(out - out_plain).max() > 100 * d_hip


def test_lbfgs_stage_with_the_term_reports_the_specs_objective_at_the_returned_rows(monkeypatch):
    n = 3
    op, (bm, vp, part, ign, kmap), init, kp = _open(n, 4, "kernel", monkeypatch, seed=7, stages=(STAGE,), optimizer="lbfgs",
                                                    lbfgs=dict(max_iter=8, max_steps=2))
    t64 = spec.fit_spec(bm, vp, kmap, bm.faces, part, ign)
    op.fitting(init, kp)
    x1 = op.body_rotation_rec.detach().cpu().double()
    k64 = torch.tensor(kp, dtype=torch.float64)
    with torch.no_grad():
        e1 = t64.collision(x1, SIGMA, W_COLL).numpy()
        f1 = t64.frame_loss(x1, k64, STAGE).numpy() + e1
    got = op.frame_loss[0]
    print("L-BFGS with the term: rounds", op.rounds, "rel err of the reported loss", np.abs(got - f1) / np.abs(f1), "the term's share", e1 / f1)
    np.testing.assert_allclose(got, f1, rtol=2e-5)            # (the bar of tests/test_gpu_face.py's bending prior, measured the same way)
    assert np.all(e1 > 2e-4 * f1)                              # a reported loss without the term would leave the bar
    op.close()


def test_refusals(monkeypatch):
    n = 2
    bm, vp, part, parent, ign, kmap, init, kp = _case(n, 7, 4, "kernel")
    prm = (SIGMA, 1.0, 256, 0)
    op = InnerFitOP(bm, vp, n, keypoint_map=kmap, iters_per_stage=0)
    assert _set_coll(op, prm) == E_STATE                        # no optimiser yet
    op.fitting(init, kp)
    assert _set_coll(op, prm) == E_STATE                        # no registered mesh
    assert _set_coll(op, None) == 0
    op.close()
    op, _, init, kp = _open(n, 4, "kernel", monkeypatch, iters_per_stage=0)
    op.fitting(init, kp)
    for bad in ((0.0, 1.0, 256, 0), (1.0, 1.0, 256, 0), (SIGMA, -1.0, 256, 0), (SIGMA, float("nan"), 256, 0), (SIGMA, float("inf"), 256, 0),
                (SIGMA, 1.0, 0, 0), (SIGMA, 1.0, -4, 0)):
        assert _set_coll(op, bad) == E_ARG, bad
    assert _set_coll(op, prm) == 0
    # a jaw set free afterwards: the evaluation refuses
    jaw = torch.zeros(n, 3, device="cuda")
    assert op.ctx.lib.fdcap_opt_set_jaw(op.ctx.handle, capi.dptr(jaw), capi.current_stream()) == 0
    sg = capi.Fit2dStage(692, 692, 640, 360, 100.0, *STAGE)
    assert op.ctx.lib.fdcap_opt_backward_fit2d(op.ctx.handle, ctypes.byref(sg), 0, capi.current_stream()) == E_STATE
    assert _set_coll(op, prm) == E_STATE                        # ... and so does the setter while the jaw is free
    assert op.ctx.lib.fdcap_opt_set_jaw(op.ctx.handle, None, capi.current_stream()) == 0
    assert op.ctx.lib.fdcap_opt_backward_fit2d(op.ctx.handle, ctypes.byref(sg), 0, capi.current_stream()) == 0
    op.close()
    # Python: before anything touches the device
    coll = dict(face_part=part, part_parent=parent)
    for kw in (dict(collision=dict(coll, fit=1)), dict(collision=coll, fit_jaw=True, keypoint_map=kmap), dict(collision=dict(coll, weights=(1.0,))),
               dict(collision=dict(coll, sigma=1.5)), dict(collision=dict(coll, capacity=0)), dict(collision=dict(coll, faces=bm.faces[:2])),
               dict(collision=dict(coll, weights=(0, 0, 0, -1.0, 1.0)))):
        with pytest.raises(capi.FdcapError):
            InnerFitOP(bm, vp, n, **kw)
    with pytest.raises(capi.FdcapError):
        InnerFitOP(synth.make_body_model(200), vp, n, collision={})             # a model without faces
    # a batch of clips and one rank's share of a clip refuse it as they refuse the rest of the inner fit
    ctx = capi.Context(bm, vp)
    ctx.set_collision_mesh(bm.faces, part, ign)
    ctx.set_scene(np.zeros((0, 3), np.float32))
    N, K = 6, 2
    oc = capi.OptConfig(N, N, 0, 0.01, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)
    state = [torch.zeros(K * N + 4, 78, device="cuda"), torch.zeros(K * N + 4, 16, device="cuda"), torch.ones(K, device="cuda"),
             torch.zeros(K, device="cuda"), torch.zeros(K, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)]
    assert ctx.lib.fdcap_opt_create_clips(ctx.handle, ctypes.byref(oc), K, *[capi.dptr(t) for t in state]) == 0
    assert ctx.lib.fdcap_opt_set_fit2d_collision(ctx.handle, ctypes.byref(capi.CollisionParams(*prm))) == E_STATE
    torch.cuda.synchronize()
    ctx.lib.fdcap_opt_destroy(ctx.handle)
    oc = capi.OptConfig(2 * N, N, N, 0.01, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)          # the second half of a clip of 12
    state = [torch.zeros(N + 4, 78, device="cuda"), torch.zeros(N + 4, 16, device="cuda"), torch.ones(1, device="cuda"),
             torch.zeros(1, device="cuda"), torch.zeros(capi.NUM_LOSSES, device="cuda", dtype=torch.float64)]
    assert ctx.lib.fdcap_opt_create(ctx.handle, ctypes.byref(oc), *[capi.dptr(t) for t in state]) == 0
    assert ctx.lib.fdcap_opt_set_fit2d_collision(ctx.handle, ctypes.byref(capi.CollisionParams(*prm))) == E_STATE
    torch.cuda.synchronize()
    ctx.close()
