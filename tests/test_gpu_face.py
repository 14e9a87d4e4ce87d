"""GPU tests of the inner fit's bending prior (csrc/fdc_fit2d.h fit2d_bend_kernel, fdcap_opt_set_fit2d_extra) and free jaw
(csrc/fdc_keypoints.h fit2d_kp_jaw_kernel, fdcap_opt_set_jaw; second half of the file) through the C-ABI,
against the fp64 torch twin tests/face_spec.py.  The body is synth.make_body_model(240) with lbs_nnz 4 and 8, 1 and 16 frames, both
blend forms pinned with FDCAP_KP_BLEND; the map takes its face from the vertices skinned to the jaw (joint 22).

Bars.  Loss sums 2e-5 relative; the 78-column gradient 2e-3 relative + 2e-4 of the BLOCK's largest entry (tests/test_gpu_keypoints.py).
The prior ALONE (every other weight zero, so that no larger term's size hides it) is held at tests/gradient_bars.py's formula
32 max(max|g32 - g64|, 2^-24 max|g64|) per column block, g32 / g64 the twin's two precisions.  Fitted rows: the bars of
tests/test_gpu_keypoints.py's fit.  The fp32 twin's own distance from the fp64 twin is printed next to every error (DESIGN.md
section 7 records both).  No bar is taken from a HIP result."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.innerfit import DEFAULT_BEND_RATIO, DEFAULT_BEND_TERMS, DEFAULT_JAW_PRIOR, DEFAULT_STAGES, InnerFitOP, KeypointMap
from oracle import rotrepr
from tests import gradient_bars as gb
from tests.face_spec import FaceSpec
from tests.keypoint_spec import COLUMN_BLOCKS, column_errors

pytestmark = pytest.mark.gpu
V = 240
STAGE = (1.0, 4.78, 5.0, 4.78)
W_BEND = DEFAULT_BEND_RATIO * STAGE[1]
E_ARG, E_STATE = -1, -2


@functools.lru_cache(maxsize=None)
def _models(seed, lbs_nnz):
    return synth.make_body_model(V, seed=seed, lbs_nnz=lbs_nnz), synth.make_vposer(seed=seed + 1)


def face_map(bm, seed=0):
    """Joints 3, 15, 22 (through Jw), finger joint 40; eight plain vertices skinned to the jaw; four landmarks whose corners are such
    vertices; the first jaw vertex once more (a vertex shared by two keypoints, and a corner of the first landmark); six vertices
    elsewhere on the body."""
    rng = np.random.Generator(np.random.PCG64(300 + seed))
    jv = np.flatnonzero(np.asarray(bm.lbs_weights)[:, 22] > 0)
    assert len(jv) >= 8
    jv = rng.permutation(jv)
    joint, tri, bary = [], [], []

    def add(j=-1, t=(0, 0, 0), b=(0.0, 0.0, 0.0)):
        joint.append(j); tri.append(tuple(int(v) for v in t)); bary.append(tuple(float(v) for v in b))
    for j in (3, 15, 22, 40):
        add(j)
    for v in jv[:8]:
        add(t=(v, v, v), b=(1, 0, 0))
    for q in range(4):
        add(t=(jv[q], jv[(q + 3) % len(jv)], jv[(q + 5) % len(jv)]), b=rng.dirichlet((1.0, 1.0, 1.0)))
    add(t=(jv[0],) * 3, b=(1, 0, 0))
    for v in rng.permutation(np.setdiff1d(np.arange(V), jv))[:6]:
        add(t=(v, v, v), b=(1, 0, 0))
    return KeypointMap(joint, tri, bary)


def _case(n, seed, lbs_nnz, kmap_of=face_map):
    """Ground truth -> the mapped points projected by the spec (+ 2 px noise, confidences); start = perturbed ground truth."""
    bm, vp = _models(seed, lbs_nnz)
    kmap = kmap_of(bm)
    clip = synth.make_clip(n, seed=seed + 2, num_outliers=0)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    gt = clip.body_params.astype(np.float32).copy()
    gt[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32) + 0.05 * rng.standard_normal((n, 3)).astype(np.float32)
    gt[:, 48:72] += 0.1 * rng.standard_normal((n, 24)).astype(np.float32)
    spec = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary)
    with torch.no_grad():
        uv = spec.project(spec.joints_cam(rotrepr.convert_to_6D_rot(torch.tensor(gt, dtype=torch.float64)))).numpy()
    kp = np.concatenate([uv + 2.0 * rng.standard_normal(uv.shape), rng.uniform(0.3, 1.0, (n, len(kmap), 1))], -1).astype(np.float32)
    init = gt.copy()
    init[:, 3:6] += 0.15 * rng.standard_normal((n, 3)).astype(np.float32)
    init[:, 16:48] += 0.5 * rng.standard_normal((n, 32)).astype(np.float32)
    init[:, 72:75] += 0.1 * rng.standard_normal((n, 3)).astype(np.float32)
    return bm, vp, kmap, gt, init, kp


def _extra(w_bend, terms=DEFAULT_BEND_TERMS):
    ex = capi.Fit2dExtra()
    ex.w_bend, ex.n_bend = w_bend, len(terms)
    for t, (j, a, s) in enumerate(terms):
        ex.joint[t], ex.axis[t], ex.sign[t] = j, a, s
    return ex


def _set_extra(op, ex):
    return op.ctx.lib.fdcap_opt_set_fit2d_extra(op.ctx.handle, None if ex is None else ctypes.byref(ex))


def _loss_and_grads(op, n, stage=STAGE):
    lib, h = op.ctx.lib, op.ctx.handle
    sg = capi.Fit2dStage(692, 692, 640, 360, 100.0, *stage)
    capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 1, capi.current_stream()), "backward_fit2d")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, capi.current_stream()), "get_grads")
    return op._losses.cpu().numpy()[:2].copy(), dx.cpu().numpy()


@pytest.fixture
def blend_form(request, monkeypatch):
    form = getattr(request, "param", None)
    if form:
        monkeypatch.setenv("FDCAP_KP_BLEND", form)
    else:
        monkeypatch.delenv("FDCAP_KP_BLEND", raising=False)
    return form


def _kp23(kp, n):
    """23 rows of plausible pixels for the 23-joint layout"""
    return np.ascontiguousarray(np.concatenate([kp, kp], 1)[:, :23])


PATHS = [(1, 4, "kernel"), (16, 4, "kernel"), (16, 8, "kernel"), (1, 4, "panel"), (16, 4, "panel"), (16, 8, "panel"), (1, 4, "joints23"),
         (16, 8, "joints23"), (16, 4, "jointmap")]


def _open(n, lbs_nnz, path, monkeypatch, seed=7, **kw):
    """an InnerFitOP on one of the three paths of the bending prior's launch: a map with vertices (dPF added to, both blend forms), the
    23-joint layout without a map, a map of joints 0..22 alone (dPF assigned on both) -> op, spec arguments, start rows, keypoints"""
    monkeypatch.setenv("FDCAP_KP_BLEND", path if path in ("kernel", "panel") else "kernel")
    if path == "joints23":
        bm, vp, _, gt, init, kp = _case(n, seed, lbs_nnz)
        kmap, kp = KeypointMap.joints23(), _kp23(kp, n)
        op = InnerFitOP(bm, vp, n, **kw)
    else:
        bm, vp, kmap, gt, init, kp = _case(n, seed, lbs_nnz, face_map if path != "jointmap" else (lambda bm: KeypointMap([3, 15, 22, 7, 20], np.zeros((5, 3)), np.zeros((5, 3)))))
        op = InnerFitOP(bm, vp, n, keypoint_map=kmap, **kw)
    return op, (bm, vp, kmap), init, kp


# ---- 1. loss sums and the full gradient with the prior on, on every path -------------------------------------------------------------
@pytest.mark.parametrize("n,lbs_nnz,path", PATHS)
def test_loss_and_gradient_with_the_bending_prior_match_fp64_autograd(n, lbs_nnz, path, monkeypatch):
    op, (bm, vp, kmap), init, kp = _open(n, lbs_nnz, path, monkeypatch, iters_per_stage=0)
    kp[0, 2, 2] = 0.0
    op.fitting(init, kp)
    assert _set_extra(op, _extra(W_BEND)) == 0
    s, dx = _loss_and_grads(op, n)
    x = op.body_rotation_rec.detach().cpu().numpy()
    s64, g64, _ = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary).grads(x, kp, STAGE, w_bend=W_BEND)
    s32, g32, _ = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, dtype=torch.float32).grads(x, kp, STAGE, w_bend=W_BEND)
    err, twin = column_errors(dx, g64), column_errors(g32, g64)
    print(f"bend on, n {n} lbs_nnz {lbs_nnz} path {path}: loss rel err", np.abs(s - s64) / np.abs(s64), " fp32 twin", np.abs(s32 - s64) / np.abs(s64))
    for k in COLUMN_BLOCKS:
        print(f"  d {k:7s} max|err| {err[k][0]:.3e}  fp32 twin {twin[k][0]:.3e}  max|g| {err[k][1]:.3e}")
    np.testing.assert_allclose(s, s64, rtol=2e-5)
    for k, sl in COLUMN_BLOCKS.items():
        assert np.all(np.abs(dx[:, sl] - g64[:, sl]) <= 2e-3 * np.abs(g64[:, sl]) + 2e-4 * err[k][1]), (k, err[k], twin[k])
    op.close()


# ---- 2. the prior alone, at the bars of the twin's two precisions -----------------------------------------------------------------------
@pytest.mark.parametrize("n,lbs_nnz,path", [(16, 4, "kernel"), (16, 4, "panel"), (1, 4, "joints23"), (16, 8, "joints23"), (16, 4, "jointmap")])
def test_the_bending_prior_alone_is_inside_the_twins_rounding_bars(n, lbs_nnz, path, monkeypatch):
    """every confidence and every other weight zero: losses [1] and the gradient are the prior's, with two terms on one joint and all
    eight terms in use"""
    terms = DEFAULT_BEND_TERMS + ((18, 0, -1.0), (1, 2, 1.0), (21, 1, 1.0), (12, 0, -1.0))
    stage0 = (1.0, 0.0, 0.0, 0.0)
    op, (bm, vp, kmap), init, kp = _open(n, lbs_nnz, path, monkeypatch, iters_per_stage=0)
    kp[:, :, 2] = 0.0
    op.fitting(init, kp)
    assert _set_extra(op, _extra(2.5, terms)) == 0
    s, dx = _loss_and_grads(op, n, stage0)
    x = op.body_rotation_rec.detach().cpu().numpy()
    s64, g64, _ = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, bend_terms=terms).grads(x, kp, stage0, w_bend=2.5)
    s32, g32, _ = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, bend_terms=terms, dtype=torch.float32).grads(x, kp, stage0, w_bend=2.5)
    bar = gb.bars(gb.blocks(rows=g32), gb.blocks(rows=g64))
    r = gb.ratios(gb.blocks(rows=dx), gb.blocks(rows=g64), bar)
    print(f"bend alone, n {n} lbs_nnz {lbs_nnz} path {path}: prior rel err", abs(s[1] - s64[1]) / s64[1], "fp32 twin", abs(s32[1] - s64[1]) / s64[1],
          "max|err| / bar per block", {k: f"{v:.3g}" for k, v in r.items()}, "latent bar", bar["latent"], "max|g|", float(np.abs(g64[:, 19:51]).max()))
    assert s[0] == 0.0 and s64[1] > 0
    np.testing.assert_allclose(s[1], s64[1], rtol=2e-5)
    assert np.abs(g64[:, 19:51]).max() > 0 and all(v <= 1.0 for v in r.values()), r
    assert np.all(dx[:, :19] == 0) and np.all(dx[:, 51:] == 0)      # the prior reaches the latent columns only
    op.close()


# ---- 3. fits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["kernel", "panel"])
def test_five_stage_fit_with_the_bending_prior_matches_the_twin(path, monkeypatch):
    n, iters = 16, 10
    op, (bm, vp, kmap), init, kp = _open(n, 4, path, monkeypatch, seed=21, iters_per_stage=iters, bend_prior={})
    out = op.fitting(init, kp).cpu().numpy()
    plain = InnerFitOP(bm, vp, n, iters_per_stage=iters, keypoint_map=kmap)
    out_plain = plain.fitting(init, kp).cpu().numpy()
    plain.close(); op.close()
    threads = torch.get_num_threads()
    twin = []
    try:
        for t in (1, 4):
            torch.set_num_threads(t)
            s32 = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, dtype=torch.float32)
            twin.append(s32.fitting_face(init, kp, DEFAULT_STAGES, iters, bend_ratio=DEFAULT_BEND_RATIO)[0].numpy())
    finally:
        torch.set_num_threads(threads)
    err, spread = np.abs(out - twin[0]), np.abs(twin[0] - twin[1])
    print("fit with the bending prior vs fp32 twin: max", err.max(), "q50", np.quantile(err, 0.5), "q99", np.quantile(err, 0.99),
          " fp32 twin, 1 thread vs 4: max", spread.max(), " distance from the fit without the prior: max", np.abs(out - out_plain).max())
    bar = 4.0 * spread.max()
    assert np.quantile(err, 0.5) < max(2e-5, bar) and np.quantile(err, 0.99) < max(3e-3, bar) and err.max() < max(0.1, bar)
    assert np.quantile(np.abs(out - out_plain), 0.99) > 10 * np.quantile(err, 0.99)       # the prior moved the fit by more than the bars


@pytest.mark.parametrize("path", ["kernel", "panel"])
def test_lbfgs_stage_with_the_bending_prior_reports_the_specs_objective_at_the_returned_rows(path, monkeypatch):
    n = 16
    op, (bm, vp, kmap), init, kp = _open(n, 4, path, monkeypatch, seed=33, stages=(STAGE,), optimizer="lbfgs", lbfgs=dict(max_iter=10, max_steps=3),
                                         bend_prior={})
    kp[2, :, 2] = 0.0
    spec = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary)
    x0 = rotrepr.convert_to_6D_rot(torch.tensor(init, dtype=torch.float64))
    op.fitting(init, kp)
    x1 = op.body_rotation_rec.detach().cpu().double()
    k64 = torch.tensor(kp, dtype=torch.float64)
    with torch.no_grad():
        f0, f1 = spec.frame_loss(x0, k64, STAGE, w_bend=W_BEND).numpy(), spec.frame_loss(x1, k64, STAGE, w_bend=W_BEND).numpy()
        b1 = spec.extra_prior(x1, w_bend=W_BEND).numpy()
    got = op.frame_loss[0]
    print("L-BFGS with the bending prior: rounds", op.rounds, "rel err of the reported loss", np.abs(got - f1) / np.abs(f1), "the prior's share", b1 / f1)
    np.testing.assert_allclose(got, f1, rtol=2e-5)
    assert np.all(b1 > 2e-4 * f1)                            # (a reported loss without the prior would leave the bar)
    assert np.all(f1 <= f0) and f1.sum() < 0.5 * f0.sum()
    op.close()


# ---- 4. off is off -------------------------------------------------------------------------------------------------------------------
def _manual_fit(op, n, iters=4):
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
    n = 16
    res = []
    for touch in (False, True):
        op, _, init, kp = _open(n, 4, path, monkeypatch, iters_per_stage=0)
        op.fitting(init, kp)
        if touch:
            assert _set_extra(op, _extra(W_BEND)) == 0
            s_on, g_on = _loss_and_grads(op, n)
            assert _set_extra(op, None) == 0
        s, g = _loss_and_grads(op, n)
        res.append((s, g, _manual_fit(op, n)))
        op.close()
    assert not np.array_equal(s_on, res[0][0]) and not np.array_equal(g_on, res[0][1])
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    # weight 0, or no terms: off as well
    op, _, init, kp = _open(n, 4, path, monkeypatch, iters_per_stage=0)
    op.fitting(init, kp)
    for ex in (_extra(0.0), _extra(W_BEND, ())):
        assert _set_extra(op, ex) == 0
        s, g = _loss_and_grads(op, n)
        assert np.array_equal(s, res[0][0]) and np.array_equal(g, res[0][1])
    op.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    n = 4
    op, (bm, vp, kmap), init, kp = _open(n, 4, "kernel", monkeypatch, iters_per_stage=0)
    assert op.ctx.lib.fdcap_opt_set_fit2d_extra(op.ctx.handle, ctypes.byref(_extra(1.0))) == E_STATE      # no optimiser yet
    op.fitting(init, kp)
    for terms in (((0, 1, 1.0),), ((22, 1, 1.0),), ((4, 3, 1.0),), ((4, -1, 1.0),), ((4, 0, float("nan")),)):
        assert _set_extra(op, _extra(1.0, terms)) == E_ARG, terms
    ex = _extra(1.0)
    ex.n_bend = 9
    assert _set_extra(op, ex) == E_ARG
    ex.n_bend = -1
    assert _set_extra(op, ex) == E_ARG
    assert _set_extra(op, _extra(float("inf"))) == E_ARG
    assert _set_extra(op, _extra(1.0, DEFAULT_BEND_TERMS * 2)) == 0 and _set_extra(op, None) == 0
    op.close()
    with pytest.raises(capi.FdcapError):
        InnerFitOP(bm, vp, n, bend_prior=dict(terms=((22, 0, 1.0),)))
    with pytest.raises(capi.FdcapError):
        InnerFitOP(bm, vp, n, bend_prior=dict(weight=1.0))
    ctx = capi.Context(bm, vp)                               # a batch of clips refuses it as it refuses the rest of the inner fit
    N, K = 6, 2
    oc = capi.OptConfig(N, N, 0, 0.01, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)
    state = [torch.zeros(K * N + 4, 78, device="cuda"), torch.zeros(K * N + 4, 16, device="cuda"), torch.ones(K, device="cuda"),
             torch.zeros(K, device="cuda"), torch.zeros(K, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)]
    ctx.set_scene(np.zeros((0, 3), np.float32))
    assert ctx.lib.fdcap_opt_create_clips(ctx.handle, ctypes.byref(oc), K, *[capi.dptr(t) for t in state]) == 0
    assert ctx.lib.fdcap_opt_set_fit2d_extra(ctx.handle, ctypes.byref(_extra(1.0))) == E_STATE
    torch.cuda.synchronize()
    ctx.close()


# ======== the free jaw (csrc/fdc_keypoints.h fit2d_kp_jaw_kernel, fdcap_opt_set_jaw / fdcap_opt_get_jaw) ================================
# Bars as above; the jaw's own gradient block at tests/gradient_bars.py's formula 32 max(max|g32 - g64|, 2^-24 max|g64|) from the
# twin's two precisions.
W_JAW = (47.8, 478.0, 478.0)
JAW_GT = np.array([0.35, 0.05, -0.05], np.float32)


def _random_jaw(n, size=0.3, seed=1):
    j = np.random.Generator(np.random.PCG64(seed)).standard_normal((n, 3))
    return (size * j / np.linalg.norm(j, axis=1, keepdims=True)).astype(np.float32)


def _extra_jaw(w_jaw=W_JAW, w_bend=0.0):
    ex = _extra(w_bend) if w_bend else capi.Fit2dExtra()
    ex.w_jaw[0], ex.w_jaw[1], ex.w_jaw[2] = w_jaw
    return ex


def _get_jaw(op, n, grad=True):
    jaw, dj = torch.empty(n, 3, device="cuda"), torch.empty(n, 3, device="cuda")
    capi.check(op.ctx.lib.fdcap_opt_get_jaw(op.ctx.handle, capi.dptr(jaw), capi.dptr(dj) if grad else None, capi.current_stream()), "get_jaw")
    return jaw.cpu().numpy(), dj.cpu().numpy()


# ---- 1. positions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lbs_nnz", [(1, 4), (16, 4), (16, 8)])
def test_keypoints3d_with_a_jaw_pose_match_the_spec(n, lbs_nnz, monkeypatch):
    op, (bm, vp, kmap), init, kp = _open(n, lbs_nnz, "kernel", monkeypatch, seed=11, iters_per_stage=0, fit_jaw=True)
    jaw = _random_jaw(n)
    if n > 1:
        jaw[3] = 0.0
    op.fitting(init, kp, jaw_init=jaw)
    out = torch.empty(n, len(kmap), 3, device="cuda")
    capi.check(op.ctx.lib.fdcap_debug_keypoints3d(op.ctx.handle, capi.dptr(out), capi.current_stream()), "debug_keypoints3d")
    spec = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary)
    x = op.body_rotation_rec.detach().cpu().double()
    with torch.no_grad():
        want = spec.joints_cam(x, torch.tensor(jaw, dtype=torch.float64)).numpy()
        fixed = spec.joints_cam(x).numpy()
    got = out.cpu().numpy()
    moved = np.abs(want - fixed).max((0, 2))
    print("keypoints3d with a jaw: max|err|", np.abs(got - want).max(), " the jaw moves the keypoints by up to", moved.round(4))
    np.testing.assert_allclose(got, want, atol=3e-5)
    assert np.all(moved[:4] == 0) and np.all(moved[4:17] > 0) and moved[4:17].max() > 1e-3      # no joint moves (22 among them); every jaw vertex and landmark does
    if n > 1:
        assert np.abs(got[3] - fixed[3]).max() <= 3e-5                   # a frame whose jaw stands at zero
    op.close()


# ---- 2. loss and gradient -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lbs_nnz,path", [(1, 4, "kernel"), (16, 4, "kernel"), (16, 8, "kernel"), (1, 4, "panel"), (16, 4, "panel"), (16, 8, "panel"),
                                            (16, 4, "jointmap")])
@pytest.mark.parametrize("w_bend", [0.0, W_BEND])
def test_loss_and_gradient_with_a_free_jaw_match_fp64_autograd(n, lbs_nnz, path, w_bend, monkeypatch):
    op, (bm, vp, kmap), init, kp = _open(n, lbs_nnz, path, monkeypatch, iters_per_stage=0, fit_jaw=True)
    jaw = _random_jaw(n, seed=n)
    if n > 1:
        jaw[5] = 0.0
    op.fitting(init, kp, jaw_init=jaw)
    assert _set_extra(op, _extra_jaw(W_JAW, w_bend)) == 0
    s, dx = _loss_and_grads(op, n)
    jaw_back, dj = _get_jaw(op, n)
    assert np.array_equal(jaw_back, jaw)
    x = op.body_rotation_rec.detach().cpu().numpy()
    s64, g64, j64 = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary).grads(x, kp, STAGE, jaw, W_JAW, w_bend)
    s32, g32, j32 = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, dtype=torch.float32).grads(x, kp, STAGE, jaw, W_JAW, w_bend)
    err, twin = column_errors(dx, g64), column_errors(g32, g64)
    jaw_bar = gb.M * max(float(np.abs(j32 - j64).max()), gb.EPS32 * float(np.abs(j64).max()))
    print(f"jaw free, bend {w_bend:.3g}, n {n} lbs_nnz {lbs_nnz} path {path}: loss rel err", np.abs(s - s64) / np.abs(s64), " fp32 twin", np.abs(s32 - s64) / np.abs(s64))
    for k in COLUMN_BLOCKS:
        print(f"  d {k:7s} max|err| {err[k][0]:.3e}  fp32 twin {twin[k][0]:.3e}  max|g| {err[k][1]:.3e}")
    print(f"  d jaw     max|err| {np.abs(dj - j64).max():.3e}  fp32 twin {np.abs(j32 - j64).max():.3e}  max|g| {np.abs(j64).max():.3e}  bar {jaw_bar:.3e}")
    np.testing.assert_allclose(s, s64, rtol=2e-5)
    for k, sl in COLUMN_BLOCKS.items():
        assert np.all(np.abs(dx[:, sl] - g64[:, sl]) <= 2e-3 * np.abs(g64[:, sl]) + 2e-4 * err[k][1]), (k, err[k], twin[k])
    assert np.abs(dj - j64).max() <= jaw_bar
    op.close()


# ---- 3. fits -------------------------------------------------------------------------------------------------------------------------
def jaw_fit_map(bm):
    """every vertex skinned to the jaw, joints (22 among them), a finger joint, twenty vertices elsewhere"""
    jv = np.flatnonzero(np.asarray(bm.lbs_weights)[:, 22] > 0)
    other = np.setdiff1d(np.arange(V), jv)[::12]
    k = len(jv) + len(other)
    return KeypointMap([3, 15, 22, 40, 12, 16, 17] + [-1] * k, [(0, 0, 0)] * 7 + [(int(v),) * 3 for v in jv] + [(int(v),) * 3 for v in other],
                       [(0, 0, 0)] * 7 + [(1, 0, 0)] * k)


JAW_FIT = dict(lr=0.015, jaw_prior=np.asarray(DEFAULT_JAW_PRIOR) * 0.01)


def _jaw_fit_case(n, seed):
    """a body near the mean pose two metres from the camera, its jaw open by about JAW_GT; start: the body slightly off, the jaw shut.
    The seed of the fit test, 23, is chosen with the twin ALONE, by two criteria: the fp32 twin's fitted rows and jaws lie 1.7e-6 from
    the fp64 twin's (on most seeds two or three frames sit at a LeakyReLU kink and the twin's own two precisions end 0.1 .. 0.2 apart,
    e.g. seed 21: 0.16 -- no yardstick for fp32 arithmetic), and the twin takes |jaw - jaw_gt| over the batch to 0.38 of its start.
    Per frame it reaches 0.17 .. 0.73: not every frame halves, and of seeds 21 .. 45 none gave both a stable twin and every frame
    halved.  With InnerFitOP's own defaults (DEFAULT_JAW_PRIOR, lr 0.01) the same twin leaves about 0.9 of the distance: fifty Adam
    steps under the default prior do not open the jaw.  On the body of _case -- far from the mean pose, so that the first stages'
    priors move the head -- the jaw runs the wrong way in the twin too.  The data are chosen so that the twin recovers the jaw,
    nothing else."""
    bm, vp = _models(seed, 4)
    kmap = jaw_fit_map(bm)
    clip = synth.make_clip(n, seed=seed + 2, num_outliers=0)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    gt = clip.body_params.astype(np.float32).copy()
    gt[:, 72:75] = np.array([0.1, -0.2, 2.0], np.float32) + 0.05 * rng.standard_normal((n, 3)).astype(np.float32)
    gt[:, 16:48] *= 0.05
    gt[:, 6:16] *= 0.05
    jaw_gt = (JAW_GT + 0.02 * rng.standard_normal((n, 3))).astype(np.float32)
    spec = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary)
    with torch.no_grad():
        uv = spec.project(spec.joints_cam(rotrepr.convert_to_6D_rot(torch.tensor(gt, dtype=torch.float64)), torch.tensor(jaw_gt, dtype=torch.float64))).numpy()
    kp = np.concatenate([uv + 0.5 * rng.standard_normal(uv.shape), rng.uniform(0.6, 1.0, (n, len(kmap), 1))], -1).astype(np.float32)
    init = gt.copy()
    init[:, 3:6] += 0.015 * rng.standard_normal((n, 3)).astype(np.float32)
    init[:, 16:48] += 0.05 * rng.standard_normal((n, 32)).astype(np.float32)
    init[:, 72:75] += 0.01 * rng.standard_normal((n, 3)).astype(np.float32)
    return bm, vp, kmap, init, kp, jaw_gt


@pytest.mark.parametrize("path", ["kernel", "panel"])
def test_five_stage_fit_matches_the_twin_and_halves_the_jaws_distance_over_the_batch(path, monkeypatch):
    """The fitted rows and jaws at the fitted-row bars of the fp32 twin; and |jaw - jaw_gt|, taken as ONE norm over the batch's frames,
    falls to at most half its start in the twin alone and in the library.  No per-frame claim: see _jaw_fit_case."""
    n, iters = 16, 10
    monkeypatch.setenv("FDCAP_KP_BLEND", path)
    bm, vp, kmap, init, kp, jaw_gt = _jaw_fit_case(n, 23)
    op = InnerFitOP(bm, vp, n, iters_per_stage=iters, keypoint_map=kmap, fit_jaw=True, bend_prior={}, **JAW_FIT)
    out = op.fitting(init, kp).cpu().numpy()
    jaw = op.jaw_pose.cpu().numpy()
    op.close()
    threads = torch.get_num_threads()
    twin = []
    try:
        for t in (1, 4):
            torch.set_num_threads(t)
            s32 = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, dtype=torch.float32, lr=JAW_FIT["lr"])
            r, j = s32.fitting_face(init, kp, DEFAULT_STAGES, iters, jaw_init=np.zeros((n, 3), np.float32), jaw_prior=JAW_FIT["jaw_prior"],
                                    bend_ratio=DEFAULT_BEND_RATIO)
            twin.append(np.concatenate([r.numpy(), j.numpy()], 1))
    finally:
        torch.set_num_threads(threads)
    got = np.concatenate([out, jaw], 1)                      # [n, 75 + 3]: the jaw columns are held at the rows' bars
    err, spread = np.abs(got - twin[0]), np.abs(twin[0] - twin[1])
    d0, d_twin, d_hip = np.linalg.norm(jaw_gt), np.linalg.norm(twin[0][:, 75:] - jaw_gt), np.linalg.norm(jaw - jaw_gt)
    print("fit with a free jaw vs fp32 twin: max", err.max(), "q50", np.quantile(err, 0.5), "q99", np.quantile(err, 0.99), "jaw columns max", err[:, 75:].max(),
          " fp32 twin, 1 thread vs 4: max", spread.max(), " |jaw - jaw_gt| / start over the batch: twin", d_twin / d0, "library", d_hip / d0)
    bar = 4.0 * spread.max()
    assert np.quantile(err, 0.5) < max(2e-5, bar) and np.quantile(err, 0.99) < max(3e-3, bar) and err.max() < max(0.1, bar)
    assert d_twin <= 0.5 * d0 and d_hip <= 0.5 * d0


@pytest.mark.parametrize("path", ["kernel", "panel"])
@pytest.mark.parametrize("max_rounds", [4000, 3, 5])
def test_lbfgs_stage_with_a_free_jaw_reports_the_specs_objective_at_the_returned_rows_and_jaw(max_rounds, path, monkeypatch):
    """max_rounds 3 and 5: the budget ends inside line searches -- rows and jaws are the last accepted points, where the reported
    objective is the twin's (a jaw left at its trial point next to rolled-back rows would leave the bar)"""
    n = 16
    monkeypatch.setenv("FDCAP_KP_BLEND", path)
    bm, vp, kmap, init, kp, jaw_gt = _jaw_fit_case(n, 33)
    w_jaw = tuple(float(v) for v in JAW_FIT["jaw_prior"][4])
    op = InnerFitOP(bm, vp, n, stages=(STAGE,), optimizer="lbfgs", lbfgs=dict(max_iter=10, max_steps=3), keypoint_map=kmap, fit_jaw=True,
                    jaw_prior=[w_jaw], bend_prior={}, max_rounds=max_rounds)
    spec = FaceSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary)
    x0 = rotrepr.convert_to_6D_rot(torch.tensor(init, dtype=torch.float64))
    op.fitting(init, kp)
    x1, j1 = op.body_rotation_rec.detach().cpu().double(), op.jaw_pose.cpu().double()
    k64 = torch.tensor(kp, dtype=torch.float64)
    with torch.no_grad():
        f0 = spec.frame_loss(x0, k64, STAGE, torch.zeros(n, 3, dtype=torch.float64), w_jaw, W_BEND).numpy()
        f1 = spec.frame_loss(x1, k64, STAGE, j1, w_jaw, W_BEND).numpy()
        f1_shut = spec.frame_loss(x1, k64, STAGE, torch.zeros(n, 3, dtype=torch.float64), w_jaw, W_BEND).numpy()
    got = op.frame_loss[0]
    back = ctypes.c_int32(-1)
    capi.check(op.ctx.lib.fdcap_opt_fit2d_lbfgs_rolled_back(op.ctx.handle, ctypes.byref(back)), "fdcap_opt_fit2d_lbfgs_rolled_back")
    print("L-BFGS with a free jaw:", path, "budget", max_rounds, "frames rolled back", back.value, "rounds", op.rounds, "rel err of the reported loss", np.abs(got - f1) / np.abs(f1),
          " the jaw's share of it", np.abs(f1_shut - f1) / f1, " |jaw|", np.linalg.norm(j1.numpy(), axis=1))
    np.testing.assert_allclose(got, f1, rtol=2e-5)
    assert np.all(f1 <= f0 * (1 + 1e-6)) and (max_rounds < 5 or np.abs(j1.numpy()).max() > 0)
    if max_rounds > 100:
        assert op.rounds[0] < max_rounds and f1.sum() < 0.5 * f0.sum() and back.value == 0
    else:                                                    # the budget ended inside line searches: those frames' rows AND jaws were put back
        assert op.rounds[0] == max_rounds and back.value > 0
    op.close()


# ---- 4. off is off --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["kernel", "panel"])
def test_a_jaw_set_free_and_fixed_again_gives_the_bits_of_a_context_that_never_called(path, monkeypatch):
    n = 16
    res = []
    for touch in (False, True):
        op, _, init, kp = _open(n, 4, path, monkeypatch, iters_per_stage=0)
        op.fitting(init, kp)
        if touch:
            lib, h = op.ctx.lib, op.ctx.handle
            capi.check(lib.fdcap_opt_set_jaw(h, capi.dptr(torch.tensor(_random_jaw(n), device="cuda")), capi.current_stream()), "set_jaw")
            assert _set_extra(op, _extra_jaw(W_JAW, W_BEND)) == 0
            s_on, g_on = _loss_and_grads(op, n)
            capi.check(lib.fdcap_opt_step_x(h, 1, capi.current_stream()), "step_x")
            op._rows_x[2:2 + n] = res[0][3]                  # (the step moved the rows: put the start back; its moments are reset below)
            capi.check(lib.fdcap_opt_set_jaw(h, None, capi.current_stream()), "set_jaw")
            assert _set_extra(op, None) == 0
            assert lib.fdcap_opt_get_jaw(h, capi.dptr(torch.empty(n, 3, device="cuda")), None, capi.current_stream()) == E_STATE
        x_start = op._rows_x[2:2 + n].clone()
        s, g = _loss_and_grads(op, n)
        res.append((s, g, _manual_fit(op, n), x_start))
        op.close()
    assert not np.array_equal(s_on, res[0][0]) and not np.array_equal(g_on, res[0][1])
    for a, b in zip(res[0][:3], res[1][:3]):
        assert np.array_equal(a, b)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_jaw_refusals(monkeypatch):
    import copy
    n = 4
    op, (bm, vp, kmap), init, kp = _open(n, 4, "kernel", monkeypatch, iters_per_stage=0)
    lib, h, st = op.ctx.lib, op.ctx.handle, capi.current_stream()
    jaw = torch.zeros(n, 3, device="cuda")
    assert lib.fdcap_opt_set_jaw(h, capi.dptr(jaw), st) == E_STATE and lib.fdcap_opt_get_jaw(h, capi.dptr(jaw), None, st) == E_STATE     # no optimiser
    op.fitting(init, kp)
    assert lib.fdcap_opt_get_jaw(h, capi.dptr(jaw), None, st) == E_STATE                    # before fdcap_opt_set_jaw
    assert lib.fdcap_opt_set_jaw(h, capi.dptr(jaw), st) == 0
    assert lib.fdcap_opt_get_jaw(h, None, None, st) == E_ARG
    assert lib.fdcap_opt_get_jaw(h, capi.dptr(jaw), capi.dptr(torch.empty(n, 3, device="cuda")), st) == E_STATE      # no evaluation yet: no gradient
    assert lib.fdcap_opt_get_jaw(h, capi.dptr(jaw), None, st) == 0
    ex = _extra_jaw((1.0, float("nan"), 1.0))
    assert _set_extra(op, ex) == E_ARG
    # the 23-joint layout has no keypoint that follows the jaw: an evaluation with a free jaw is refused there
    capi.check(lib.fdcap_opt_set_keypoints(h, capi.dptr(torch.tensor(_kp23(kp, n), device="cuda")), st), "set_keypoints")
    sg = capi.Fit2dStage(692, 692, 640, 360, 100.0, *STAGE)
    assert lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 0, st) == E_STATE
    assert lib.fdcap_opt_set_jaw(h, None, st) == 0 and lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 0, st) == 0
    op.close()
    with pytest.raises(capi.FdcapError):
        InnerFitOP(bm, vp, n, fit_jaw=True)                  # no map
    with pytest.raises(capi.FdcapError):
        InnerFitOP(bm, vp, n, keypoint_map=kmap, jaw_prior=DEFAULT_JAW_PRIOR)
    with pytest.raises(capi.FdcapError):
        InnerFitOP(bm, vp, n, keypoint_map=kmap, fit_jaw=True, jaw_prior=DEFAULT_JAW_PRIOR[:2])
    # a model whose joint 22 has a child: the leaf argument does not hold
    bm2 = copy.copy(bm)
    bm2.parents = np.array(bm.parents).copy()
    bm2.parents[23] = 22
    op2 = InnerFitOP(bm2, vp, n, iters_per_stage=0, keypoint_map=kmap)
    op2.fitting(init, kp)
    assert op2.ctx.lib.fdcap_opt_set_jaw(op2.ctx.handle, capi.dptr(jaw), st) == E_ARG
    op2.close()
    ctx = capi.Context(bm, vp)                               # a batch of clips
    N, K = 6, 2
    oc = capi.OptConfig(N, N, 0, 0.01, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)
    state = [torch.zeros(K * N + 4, 78, device="cuda"), torch.zeros(K * N + 4, 16, device="cuda"), torch.ones(K, device="cuda"),
             torch.zeros(K, device="cuda"), torch.zeros(K, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)]
    ctx.set_scene(np.zeros((0, 3), np.float32))
    assert ctx.lib.fdcap_opt_create_clips(ctx.handle, ctypes.byref(oc), K, *[capi.dptr(t) for t in state]) == 0
    assert ctx.lib.fdcap_opt_set_jaw(ctx.handle, capi.dptr(torch.zeros(K * N, 3, device="cuda")), st) == E_STATE
    torch.cuda.synchronize()
    ctx.close()
