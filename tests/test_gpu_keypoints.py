"""GPU tests of the inner fit on mapped keypoints (csrc/fdc_keypoints.h: joints 0..54, mesh vertices, barycentric surface points)
through the C-ABI, against the fp64 torch twin tests/keypoint_spec.py.  The body is synth.make_body_model(240), at most 16 frames.

Bars.  Loss sums 2e-5 relative; gradients 2e-3 relative + 2e-4 of the largest entry (tests/test_gpu_innerfit.py), held for the whole
[n, 78] matrix and, so that no block hides behind the largest one's size, for every column block against the BLOCK's largest entry.
The vertex branch needed no wider bar; the spec's own fp32 twin's distance from its fp64 twin is printed next to every error
(DESIGN.md section 7 records both).  Fitted rows: the bars of the 23-joint fit's comparison, or 4 x the fp32 twin's spread between
two thread counts.  No bar is taken from a HIP result."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.innerfit import (DEFAULT_STAGES, OPENPOSE_BODY25, OPENPOSE_LHAND, OPENPOSE_RHAND, InnerFitOP, KeypointMap)
from oracle import rotrepr
from tests.keypoint_spec import COLUMN_BLOCKS, KeypointSpec, column_errors

pytestmark = pytest.mark.gpu
V = 240
STAGE = (1.0, 4.78, 5.0, 4.78)
SG = (692, 692, 640, 360, 100.0) + STAGE
E_ARG, E_STATE = -1, -2


def make_map(n_kp, seed=0):
    """Joints 3, 20, 22 (through Jw) and 23, 25, 39, 40, 54 (pseudo-vertices); six plain vertices; four barycentric triples; a plain
    vertex that is also a corner of the first triple; the first triple once more; then, up to n_kp, a random mix of the three kinds."""
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    ids = rng.permutation(V)
    joint, tri, bary = [], [], []

    def add(j=-1, t=(0, 0, 0), b=(0.0, 0.0, 0.0)):
        joint.append(j); tri.append(tuple(int(v) for v in t)); bary.append(tuple(float(v) for v in b))
    for j in (3, 20, 22, 23, 25, 39, 40, 54):
        add(j)
    for v in ids[:6]:
        add(t=(v, v, v), b=(1, 0, 0))
    for q in range(4):
        w = rng.dirichlet((1.0, 1.0, 1.0))
        add(t=ids[6 + 3 * q:9 + 3 * q], b=w)
    add(t=(ids[7],) * 3, b=(1, 0, 0))                       # two keypoints on one vertex
    add(t=tri[14], b=bary[14])                               # one keypoint twice
    while len(joint) < n_kp:
        kind = rng.integers(3)
        if kind == 0:
            add(int(rng.integers(55)))
        elif kind == 1:
            v = int(rng.integers(V))
            add(t=(v, v, v), b=(1, 0, 0))
        else:
            add(t=rng.choice(V, 3, replace=False), b=rng.dirichlet((1.0, 1.0, 1.0)))
    return KeypointMap(joint[:n_kp], tri[:n_kp], bary[:n_kp])


def openpose_map(seed=0):
    """BODY_25 + both hands (67) over 21 vertex ids the test picks: the synthetic body has no named vertices"""
    extra = np.random.Generator(np.random.PCG64(200 + seed)).permutation(V)[:21]
    return KeypointMap.from_smplx_indices(OPENPOSE_BODY25 + OPENPOSE_LHAND + OPENPOSE_RHAND, extra)


@functools.lru_cache(maxsize=None)
def _models(seed, lbs_nnz=4):
    return synth.make_body_model(V, seed=seed, lbs_nnz=lbs_nnz), synth.make_vposer(seed=seed + 1)


def _case(n, seed, kmap, lbs_nnz=4, hands=0.0):
    """Ground truth -> the mapped points projected by the spec (+ 2 px noise, confidences); start = perturbed ground truth."""
    bm, vp = _models(seed, lbs_nnz)
    clip = synth.make_clip(n, seed=seed + 2, num_outliers=0)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    gt = clip.body_params.astype(np.float32).copy()
    gt[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32) + 0.05 * rng.standard_normal((n, 3)).astype(np.float32)
    gt[:, 48:72] += hands * rng.standard_normal((n, 24)).astype(np.float32)
    spec = KeypointSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary)
    with torch.no_grad():
        uv = spec.project(spec.joints_cam(rotrepr.convert_to_6D_rot(torch.tensor(gt, dtype=torch.float64)))).numpy()
    kp = np.concatenate([uv + 2.0 * rng.standard_normal(uv.shape), rng.uniform(0.3, 1.0, (n, len(kmap), 1))], -1).astype(np.float32)
    init = gt.copy()
    init[:, 3:6] += 0.15 * rng.standard_normal((n, 3)).astype(np.float32)
    init[:, 16:48] += 0.5 * rng.standard_normal((n, 32)).astype(np.float32)
    init[:, 72:75] += 0.1 * rng.standard_normal((n, 3)).astype(np.float32)
    return bm, vp, spec, gt, init, kp


def _stage():
    return capi.Fit2dStage(*SG)


def _loss_and_grads(op, n):
    lib, h = op.ctx.lib, op.ctx.handle
    sg = _stage()
    capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 1, capi.current_stream()), "backward_fit2d")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, capi.current_stream()), "get_grads")
    return op._losses.cpu().numpy()[:2].copy(), dx.cpu().numpy()


# ---- 1. the identity map is the 23-joint path, bit for bit ------------------------------------------------------------------------
def test_joints23_map_gives_the_bits_of_the_23_joint_path():
    n = 16
    kmap = KeypointMap.joints23()
    bm, vp, spec, gt, init, kp = _case(n, 7, kmap)
    kp[:, 22, 2] = 0.0
    res = []
    for m in (None, kmap):
        op = InnerFitOP(bm, vp, n, iters_per_stage=10, keypoint_map=m)
        rows = op.fitting(init, kp, log_every=1).cpu().numpy()
        res.append((np.array(op.log), rows) + _loss_and_grads(op, n))
        op.close()
    (log_a, rows_a, s_a, g_a), (log_b, rows_b, s_b, g_b) = res
    assert log_a.shape == (50, 2) and np.array_equal(log_a, log_b)
    assert np.array_equal(rows_a, rows_b)
    assert np.array_equal(s_a, s_b) and np.array_equal(g_a, g_b)
    assert np.abs(rows_a - init).max() > 1e-3                # (the fit moved)


# ---- 2. the mapped points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lbs_nnz", [4, 8])
def test_keypoints3d_match_the_spec(lbs_nnz):
    n = 5
    kmap = make_map(20)
    bm, vp, spec, gt, init, kp = _case(n, 11, kmap, lbs_nnz)
    op = InnerFitOP(bm, vp, n, iters_per_stage=0, keypoint_map=kmap)
    op.fitting(init, kp)
    out = torch.empty(n, len(kmap), 3, device="cuda")
    capi.check(op.ctx.lib.fdcap_debug_keypoints3d(op.ctx.handle, capi.dptr(out), capi.current_stream()), "debug_keypoints3d")
    with torch.no_grad():
        want = spec.joints_cam(op.body_rotation_rec.detach().cpu().double()).numpy()
    got = out.cpu().numpy()
    print("keypoints3d max|err|", np.abs(got - want).max(), "per kind (Jw joints, finger joints, vertices, triples)",
          [float(np.abs(got[:, a:b] - want[:, a:b]).max()) for a, b in ((0, 3), (3, 8), (8, 14), (14, 18))])
    np.testing.assert_allclose(got, want, atol=3e-5)         # (fdcap_smplx_forward's vertices against the oracle: tests/test_gpu_ops_autograd.py)
    assert np.array_equal(got[:, 14], got[:, 19])            # the duplicated keypoint
    op.close()


# ---- 3. loss sums and the full gradient ---------------------------------------------------------------------------------------------
def _spec_grads(spec_cls_args, x_np, kp, dtype):
    bm, vp, kmap = spec_cls_args
    spec = KeypointSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, dtype=dtype)
    x = torch.tensor(x_np, dtype=dtype, requires_grad=True)
    data, prior = spec.loss(x, torch.tensor(kp, dtype=dtype), STAGE)
    (data + prior).backward()
    return np.array([float(data.detach()), float(prior.detach())]), x.grad.numpy().astype(np.float64)


@pytest.fixture
def blend_form(request, monkeypatch):
    """where the set's blend products run (csrc/fdc_keypoints.h kp_blend_by_panels): these sizes all take the kernel's own by size;
    "panel" pins the panel products around it"""
    form = getattr(request, "param", None)
    if form:
        monkeypatch.setenv("FDCAP_KP_BLEND", form)
    else:
        monkeypatch.delenv("FDCAP_KP_BLEND", raising=False)
    return form


@pytest.mark.parametrize("n,n_kp,lbs_nnz,blend_form", [(1, 67, 4, None), (16, 67, 4, None), (1, 136, 4, None), (16, 136, 4, None), (16, 136, 8, None),
                                                       (1, 67, 4, "panel"), (16, 136, 4, "panel"), (16, 136, 8, "panel")], indirect=["blend_form"])
def test_mapped_loss_and_gradient_match_fp64_autograd(n, n_kp, lbs_nnz, blend_form):
    kmap = make_map(n_kp, seed=n_kp)
    bm, vp, spec, gt, init, kp = _case(n, 7, kmap, lbs_nnz, hands=0.2)
    kp[0, 5, 2] = 0.0                                        # one keypoint undetected
    if n > 1:
        kp[n // 2, :, 2] = 0.0                               # one whole frame undetected
    op = InnerFitOP(bm, vp, n, iters_per_stage=0, keypoint_map=kmap)
    op.fitting(init, kp)
    s, dx = _loss_and_grads(op, n)
    x = op.body_rotation_rec.detach().cpu().numpy()
    s64, g64 = _spec_grads((bm, vp, kmap), x, kp, torch.float64)
    s32, g32 = _spec_grads((bm, vp, kmap), x, kp, torch.float32)
    err, twin = column_errors(dx, g64), column_errors(g32, g64)
    print(f"n {n} n_kp {n_kp} lbs_nnz {lbs_nnz} blend {blend_form or 'by size'}: loss rel err", np.abs(s - s64) / np.abs(s64), " fp32 twin", np.abs(s32 - s64) / np.abs(s64))
    for k in COLUMN_BLOCKS:
        print(f"  d {k:7s} max|err| {err[k][0]:.3e}  fp32 twin {twin[k][0]:.3e}  max|g| {err[k][1]:.3e}")
    np.testing.assert_allclose(s, s64, rtol=2e-5)
    np.testing.assert_allclose(dx, g64, rtol=2e-3, atol=2e-4 * np.abs(g64).max())
    for k, sl in COLUMN_BLOCKS.items():
        assert np.all(np.abs(dx[:, sl] - g64[:, sl]) <= 2e-3 * np.abs(g64[:, sl]) + 2e-4 * err[k][1]), (k, err[k], twin[k])
    if n > 1:                                                # an undetected frame keeps the priors' gradient alone
        f = n // 2
        assert np.all(dx[f, 0:9] == 0) and np.all(dx[f, 75:78] == 0)
        np.testing.assert_allclose(dx[f, 9:19], 2 * STAGE[2] ** 2 * x[f, 9:19], rtol=1e-6)
    op.close()


# ---- 4. a five-stage Adam fit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend_form", [None, "panel"], indirect=True)
def test_five_stage_fit_on_openpose_keypoints_matches_the_twin_and_pulls_in_feet_and_fingertips(blend_form):
    n, iters = 8, 10
    kmap = openpose_map()
    bm, vp, spec, gt, init, kp = _case(n, 21, kmap, hands=0.1)
    kp[:, 17, 2] = 0.0                                       # an ear never detected
    kp[3, 25:46, 2] = 0.0                                    # one frame without its left hand
    op = InnerFitOP(bm, vp, n, iters_per_stage=iters, keypoint_map=kmap)
    out = op.fitting(init, kp).cpu().numpy()
    op.close()
    threads = torch.get_num_threads()
    twin = []
    try:
        for t in (1, 4):
            torch.set_num_threads(t)
            s32 = KeypointSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, dtype=torch.float32)
            twin.append(s32.fitting(init, kp, DEFAULT_STAGES, iters).numpy())
    finally:
        torch.set_num_threads(threads)
    err, spread = np.abs(out - twin[0]), np.abs(twin[0] - twin[1])
    blocks = ((0, 3), (3, 6), (6, 16), (16, 48), (48, 72), (72, 75))
    print("mapped fit vs fp32 twin: max", err.max(), "q50", np.quantile(err, 0.5), "q99", np.quantile(err, 0.99),
          "per block (transl, aa, betas, latent, hands, cam_t)", [float(err[:, a:b].max()) for a, b in blocks])
    print("fp32 twin, 1 thread vs 4: max", spread.max(), "per block", [float(spread[:, a:b].max()) for a, b in blocks])
    # the 23-joint fit's bars against its oracle (tests/test_gpu_innerfit.py: LeakyReLU slopes flip between two fp32 evaluations and
    # Adam amplifies it), or 4 x the twin's own spread between two thread counts
    bar = 4.0 * spread.max()
    assert np.quantile(err, 0.5) < max(2e-5, bar) and np.quantile(err, 0.99) < max(3e-3, bar) and err.max() < max(0.1, bar)

    tips = np.array([k for k, i in enumerate(OPENPOSE_BODY25 + OPENPOSE_LHAND + OPENPOSE_RHAND) if i >= 60])   # toes, heels, fingertips

    def px_err(rows):
        with torch.no_grad():
            uv = spec.project(spec.joints_cam(rotrepr.convert_to_6D_rot(torch.tensor(rows, dtype=torch.float64)))).numpy()
        w = kp[:, tips, 2] > 0
        return float(np.sqrt(((uv - kp[..., :2]) ** 2).sum(-1))[:, tips][w].mean())
    assert len(tips) == 16
    e0, e1 = px_err(init), px_err(out)
    print("mean reprojection error of toes, heels and fingertips (px): start", e0, "end", e1)
    assert e1 <= 0.5 * e0


# ---- 5. one L-BFGS stage ------------------------------------------------------------------------------------------------------
def test_lbfgs_stage_reports_the_specs_objective_at_the_returned_rows():
    n = 8
    kmap = openpose_map(1)
    bm, vp, spec, gt, init, kp = _case(n, 33, kmap, hands=0.1)
    kp[2, :, 2] = 0.0
    op = InnerFitOP(bm, vp, n, stages=(STAGE,), optimizer="lbfgs", lbfgs=dict(max_iter=10, max_steps=3), keypoint_map=kmap)
    x0 = rotrepr.convert_to_6D_rot(torch.tensor(init, dtype=torch.float64))
    op.fitting(init, kp)
    x1 = op.body_rotation_rec.detach().cpu().double()
    k64 = torch.tensor(kp, dtype=torch.float64)
    with torch.no_grad():
        f0, f1 = spec.frame_loss(x0, k64, STAGE).numpy(), spec.frame_loss(x1, k64, STAGE).numpy()
    got = op.frame_loss[0]
    print("L-BFGS on mapped keypoints: rounds", op.rounds, "iterations", op.frame_iterations[0], "rel err of the reported loss",
          np.abs(got - f1) / np.abs(f1), "start", f0, "end", f1)
    np.testing.assert_allclose(got, f1, rtol=2e-5)
    assert np.all(f1 <= f0) and f1.sum() < 0.5 * f0.sum()
    op.close()


# ---- 6. refusals, and the way back ------------------------------------------------------------------------------------------------
def test_refusals_and_the_old_path_after_set_keypoints():
    n = 4
    kmap = make_map(20)
    bm, vp, spec, gt, init, kp = _case(n, 5, kmap)
    kp23 = np.ascontiguousarray(np.concatenate([kp, kp[:, :3]], 1))      # 23 rows of plausible pixels for the 23-joint layout
    plain = InnerFitOP(bm, vp, n, iters_per_stage=0)
    plain.fitting(init, kp23)
    lib, h, st = plain.ctx.lib, plain.ctx.handle, capi.current_stream()
    d = torch.tensor(kp, device="cuda")
    assert lib.fdcap_opt_set_keypoints_mapped(h, capi.dptr(d), st) == E_STATE            # no map
    out = torch.empty(n, len(kmap), 3, device="cuda")
    assert lib.fdcap_debug_keypoints3d(h, capi.dptr(out), st) == E_STATE
    with pytest.raises(capi.FdcapError, match="FDCAP_E_STATE"):                           # a map under a live optimiser
        plain.ctx.set_keypoint_map(kmap.joint, kmap.tri, kmap.bary)
    s_ref, g_ref = _loss_and_grads(plain, n)
    plain.close()

    ctx = capi.Context(bm, vp)
    bad = lambda j, t, b: ctx.lib.fdcap_set_keypoint_map(ctx.handle, len(j), (ctypes.c_int32 * len(j))(*j), (ctypes.c_int32 * (3 * len(j)))(*t),
                                                         (ctypes.c_float * (3 * len(j)))(*b))
    assert bad([55], [0, 0, 0], [1, 0, 0]) == E_ARG and bad([-1], [0, V, 0], [1, 0, 0]) == E_ARG and bad([-1], [0, -1, 0], [1, 0, 0]) == E_ARG
    assert bad([-1], [0, 1, 2], [1, float("nan"), 0]) == E_ARG and bad([-1], [0, 1, 2], [1, float("inf"), 0]) == E_ARG
    assert bad([0] * 161, [0] * 483, [0] * 483) == E_ARG and ctx.lib.fdcap_set_keypoint_map(ctx.handle, -1, None, None, None) == E_ARG
    assert bad([54, -1], [0] * 3 + [0, 1, V - 1], [0] * 3 + [0.5, 0.25, 0.25]) == 0 and bad([], [], []) == 0
    ctx.set_keypoint_map(kmap.joint, kmap.tri, kmap.bary)
    N, K = 6, 2                                              # a batch of clips refuses the mapped keypoints as it refuses the 23
    oc = capi.OptConfig(N, N, 0, 0.01, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)
    state = [torch.zeros(K * N + 4, 78, device="cuda"), torch.zeros(K * N + 4, 16, device="cuda"), torch.ones(K, device="cuda"),
             torch.zeros(K, device="cuda"), torch.zeros(K, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)]
    ctx.set_scene(np.zeros((0, 3), np.float32))
    assert ctx.lib.fdcap_opt_create_clips(ctx.handle, ctypes.byref(oc), K, *[capi.dptr(t) for t in state]) == 0
    big = torch.zeros(K * N, len(kmap), 3, device="cuda")
    assert ctx.lib.fdcap_opt_set_keypoints_mapped(ctx.handle, capi.dptr(big), st) == E_STATE
    assert ctx.lib.fdcap_debug_keypoints3d(ctx.handle, capi.dptr(big), st) == E_STATE
    torch.cuda.synchronize()
    ctx.close()

    op = InnerFitOP(bm, vp, n, iters_per_stage=0, keypoint_map=kmap)
    op.fitting(init, kp)
    s_map, g_map = _loss_and_grads(op, n)
    assert not np.array_equal(g_map, g_ref)
    capi.check(op.ctx.lib.fdcap_opt_set_keypoints(op.ctx.handle, capi.dptr(torch.tensor(kp23, device="cuda")), capi.current_stream()), "set_keypoints")
    s_back, g_back = _loss_and_grads(op, n)
    assert np.array_equal(s_back, s_ref) and np.array_equal(g_back, g_ref)
    op.close()


# ---- 7. per-stage group weights ---------------------------------------------------------------------------------------------------
def test_group_weights_scale_the_confidences_stage_by_stage():
    """hands at weight 0 in every stage = the hands' confidences zeroed by the caller; weight 1 = no weights at all: same bits"""
    n, iters = 4, 3
    kmap = openpose_map()
    bm, vp, spec, gt, init, kp = _case(n, 9, kmap, hands=0.1)
    group_of = [0] * 25 + [1] * 42
    stages = DEFAULT_STAGES[:3]

    def fit(keypoints, **kw):
        op = InnerFitOP(bm, vp, n, stages=stages, iters_per_stage=iters, keypoint_map=kmap, **kw)
        rows = op.fitting(init, keypoints).cpu().numpy()
        op.close()
        return rows
    no_hands = kp.copy()
    no_hands[:, 25:, 2] = 0.0
    assert np.array_equal(fit(kp, group_of=group_of, group_weights=[[1.0, 0.0]] * 3), fit(no_hands))
    assert np.array_equal(fit(kp, group_of=group_of, group_weights=[[1.0, 1.0]] * 3), fit(kp))
    late = fit(kp, group_of=group_of, group_weights=[[1.0, 0.0], [1.0, 0.0], [1.0, 2.0]])
    assert not np.array_equal(late, fit(no_hands)) and not np.array_equal(late, fit(kp))
    with pytest.raises(capi.FdcapError):
        InnerFitOP(bm, vp, n, stages=stages, keypoint_map=kmap, group_of=group_of, group_weights=[[1.0, 1.0]] * 2)
    with pytest.raises(capi.FdcapError):
        InnerFitOP(bm, vp, n, group_of=group_of)
