"""GPU tests of the full mesh under a jaw pose and expression coefficients (csrc/fdc_face_mesh.h: face_fwd_kernel, expr_offsets_kernel,
expr_dpsi_kernel, face_bwd_kernel; fdcap_smplx_forward_face / fdcap_smplx_backward_face, fdcap_body_forward_face, fdcap_world_mesh_face)
through ops.BodyModel, ops.body_forward_from_params, ops.world_mesh and the C-ABI, against the fp64 torch twin tests/face_mesh_spec.py.

Bars.  Every block -- the eight inputs' gradients, the vertices, the 55 joints -- is held to tests/gradient_bars.py's formula
32 max(max|x32 - x64|, 2^-24 max|x64|), x32 / x64 the twin's two precisions at the same fp32-rounded inputs; a block whose bar is zero (the
jaw's gradient under a joints-only loss: the jaw moves no joint) must be matched exactly.  No bar is taken from a HIP result;
tests/test_face_mesh_cpu.py shows that a gradient with one piece of the correction missing leaves them."""
import dataclasses

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, ops, synth
from fdcap_amd.innerfit import InnerFitOP
from tests import face_mesh_spec as fs
from tests import gradient_bars as gb

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -2
# (B, V, lbs_nnz): one partial 256-thread block; a ragged last block and ten chunks of the d psi reduction, the last one ragged; a frame count that crosses
# 64 (and the reductions' sixteen-frame slices: 65 = 4 x 16 + 1).  K <= 4 takes the skinning kernels' vpack path, 8 and 12 the wider ones.
CASES = [(1, 150, 4), (3, 777, 8), (65, 300, 12)]
_ctx = {}


def _model(V, lbs_nnz):
    if (V, lbs_nnz) not in _ctx:
        bm, vp = synth.make_body_model(V, seed=0, lbs_nnz=lbs_nnz), synth.make_vposer(seed=1)
        _ctx[(V, lbs_nnz)] = (bm, vp, capi.Context(bm, vp))
    return _ctx[(V, lbs_nnz)]


def _dev(a, grad=False):
    return torch.tensor(np.asarray(a), dtype=torch.float32).cuda().requires_grad_(grad)


def _run_operator(ctx, inp, face, wv, wj):
    """ops.BodyModel with the face's keys -> {block: numpy} of vertices, joints and every input's gradient"""
    g = {k: _dev(inp[k], True) for k in fs.INPUTS + fs.FACE[face]}
    out = ops.BodyModel(ctx)(return_verts=True, **g)
    got = {"vertices": out.vertices.detach().cpu().numpy(), "joints": out.joints.detach().cpu().numpy()}
    if wv is not None or wj is not None:
        loss = 0
        if wv is not None:
            loss = loss + (out.vertices * _dev(wv)).sum()
        if wj is not None:
            loss = loss + (out.joints * _dev(wj)).sum()
        loss.backward()
        got.update({k: v.grad.cpu().numpy() for k, v in g.items()})
    return got


# ---- 1. forward and backward against the fp64 twin ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("upstream", ["vertices", "joints", "both"])
@pytest.mark.parametrize("face", ["jaw", "psi", "both"])
@pytest.mark.parametrize("B,V,lbs_nnz", CASES)
def test_operator_forward_and_backward_match_the_fp64_twin(B, V, lbs_nnz, face, upstream):
    bm, vp, ctx = _model(V, lbs_nnz)
    inp, wv, wj = fs.make_inputs(B, V, seed=B)
    wv, wj = (wv if upstream != "joints" else None), (wj if upstream != "vertices" else None)
    b64, b32, bar = fs.bars_of(bm, inp, face, wv, wj)
    got = _run_operator(ctx, inp, face, wv, wj)
    shut = ops.BodyModel(ctx)(return_verts=True, **{k: _dev(inp[k]) for k in fs.INPUTS})
    moved = float(np.abs(got["vertices"] - shut.vertices.cpu().numpy()).max())
    r = gb.ratios(got, b64, bar)
    r32 = gb.ratios(b32, b64, bar)
    print(f"B {B} V {V} lbs_nnz {lbs_nnz} {face} d {upstream}: the face moves a vertex by {moved:.3e}; max|err| / bar (the fp32 twin's in brackets): "
          + " ".join(f"{k} {v:.3g} ({r32[k]:.3g})" for k, v in r.items()))
    assert moved > 100 * bar["vertices"]                     # (a call that ignored the two keys would sit here)
    for k in fs.FACE[face]:                                  # the new blocks carry a gradient wherever the loss can see the face
        if not (k == "jaw_pose" and upstream == "joints"):
            assert np.abs(b64[k]).max() > 100 * bar[k]
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad


# ---- 2. NULL / NULL is the entry point without `_face`, byte for byte --------------------------------------------------------------------
def test_null_null_equals_the_plain_entry_points_byte_for_byte():
    B, V, lbs_nnz = 3, 777, 8
    bm, vp, ctx = _model(V, lbs_nnz)
    lib, h, st = ctx.lib, ctx.handle, capi.current_stream()
    inp, wv, wj = fs.make_inputs(B, V, seed=B)
    a = [_dev(inp[k]) for k in fs.INPUTS]
    p = [capi.dptr(t) for t in a]
    new = lambda *s: torch.full(s, float("nan"), device="cuda")
    v0, j0, v1, j1 = new(B, V, 3), new(B, 55, 3), new(B, V, 3), new(B, 55, 3)
    capi.check(lib.fdcap_smplx_forward(h, *p, B, capi.dptr(v0), capi.dptr(j0), st), "fdcap_smplx_forward")
    capi.check(lib.fdcap_smplx_forward_face(h, *p, B, None, None, capi.dptr(v1), capi.dptr(j1), st), "fdcap_smplx_forward_face")
    assert torch.equal(v0, v1) and torch.equal(j0, j1)
    gv, gj = _dev(wv), _dev(wj)
    g0, g1 = [new(*t.shape) for t in a], [new(*t.shape) for t in a]
    capi.check(lib.fdcap_smplx_backward(h, *p, B, capi.dptr(gv), capi.dptr(gj), *[capi.dptr(t) for t in g0], st), "fdcap_smplx_backward")
    capi.check(lib.fdcap_smplx_backward_face(h, *p, B, None, None, capi.dptr(gv), capi.dptr(gj), *[capi.dptr(t) for t in g1], None, None, st),
               "fdcap_smplx_backward_face")
    assert all(torch.equal(x, y) for x, y in zip(g0, g1))
    # a gradient for an input that was not given
    assert lib.fdcap_smplx_backward_face(h, *p, B, None, None, capi.dptr(gv), capi.dptr(gj), *[capi.dptr(t) for t in g1], capi.dptr(new(B, 3)), None, st) == E_ARG
    rows = _dev(synth.make_clip(B, seed=3).body_params)
    v0, j0, v1, j1 = new(B, V, 3), new(B, 55, 3), new(B, V, 3), new(B, 55, 3)
    capi.check(lib.fdcap_body_forward(h, capi.dptr(rows), B, capi.dptr(v0), capi.dptr(j0), st), "fdcap_body_forward")
    capi.check(lib.fdcap_body_forward_face(h, capi.dptr(rows), B, None, None, capi.dptr(v1), capi.dptr(j1), st), "fdcap_body_forward_face")
    assert torch.equal(v0, v1) and torch.equal(j0, j1)
    cam, sc = _dev(_cameras(B)), _dev([1.8])
    v0, v1 = new(B, V, 3), new(B, V, 3)
    capi.check(lib.fdcap_world_mesh(h, capi.dptr(rows), B, capi.dptr(cam), capi.dptr(sc), capi.dptr(v0), st), "fdcap_world_mesh")
    capi.check(lib.fdcap_world_mesh_face(h, capi.dptr(rows), B, None, None, capi.dptr(cam), capi.dptr(sc), capi.dptr(v1), st), "fdcap_world_mesh_face")
    assert torch.equal(v0, v1) and not torch.isnan(v1).any()
    # ... and the Python layer: None takes the old call
    assert torch.equal(ops.world_mesh(ctx, rows, 1.8, cam.view(B, 4, 4)), v0)
    assert torch.equal(ops.body_forward_from_params(ctx, rows)[0], ops.body_forward_from_params(ctx, rows, jaw_pose=None, expression=None)[0])


# ---- 3. two backward calls give the same bytes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,lbs_nnz", CASES[1:])
def test_two_backward_calls_give_identical_bytes(B, V, lbs_nnz):
    bm, vp, ctx = _model(V, lbs_nnz)
    inp, wv, wj = fs.make_inputs(B, V, seed=B)
    a = _run_operator(ctx, inp, "both", wv, wj)
    ops.BodyModel(ctx)(return_verts=True, **{k: _dev(inp[k]) for k in fs.INPUTS})      # (another call's workspaces in between)
    b = _run_operator(ctx, inp, "both", wv, wj)
    assert set(a) == set(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
    assert np.abs(a["expression"]).max() > 0 and np.abs(a["jaw_pose"]).max() > 0


# ---- 4. the world mesh and the one-call forward -----------------------------------------------------------------------------------------------
def _cameras(n, seed=5):
    rng = np.random.default_rng(seed)
    from oracle import rotrepr
    cam = np.tile(np.eye(4), (n, 1, 1))
    cam[:, :3, :3] = rotrepr.aa2matrot(torch.tensor(rng.standard_normal((n, 3)), dtype=torch.float64)).numpy()
    cam[:, :3, 3] = rng.standard_normal((n, 3))
    return cam.astype(np.float32).reshape(n, 16)


@pytest.mark.parametrize("face", ["jaw", "psi", "both"])
def test_world_mesh_with_the_face_matches_the_viewers_formula(face):
    B, V, lbs_nnz = 5, 300, 12
    bm, vp, ctx = _model(V, lbs_nnz)
    rows = synth.make_clip(B, seed=3).body_params.astype(np.float32)
    inp, _, _ = fs.make_inputs(B, V, seed=9)
    jaw = inp["jaw_pose"] if face != "psi" else None
    psi = inp["expression"] if face != "jaw" else None
    cams, scale = _cameras(B), np.float32(1.8)
    w64 = fs.world_vertices(bm, vp, rows, scale, cams, jaw, psi)
    w32 = fs.world_vertices(bm, vp, rows, scale, cams, jaw, psi, dtype=torch.float32)
    bar = gb.bars({"v": w32.astype(np.float64)}, {"v": w64})["v"]
    t = lambda a: None if a is None else _dev(a)
    got = ops.world_mesh(ctx, _dev(rows), float(scale), _dev(cams).view(B, 4, 4), jaw_pose=t(jaw), expression=t(psi)).cpu().numpy()
    shut = ops.world_mesh(ctx, _dev(rows), float(scale), _dev(cams).view(B, 4, 4)).cpu().numpy()
    err = float(np.abs(got - w64).max())
    print(f"world mesh {face}: max|err| {err:.3e} bar {bar:.3e}, the fp32 twin {np.abs(w32 - w64).max():.3e}; moved by the face {np.abs(got - shut).max():.3e}")
    assert err <= bar and np.abs(got - shut).max() > 100 * bar
    # the one-call forward in the body frame: scale 1, the identity camera, no camera translation
    r0 = rows.copy()
    r0[:, 72:75] = 0
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (B, 1))
    b64, b32 = fs.world_vertices(bm, vp, r0, 1.0, eye, jaw, psi), fs.world_vertices(bm, vp, r0, 1.0, eye, jaw, psi, dtype=torch.float32)
    bar = gb.bars({"v": b32.astype(np.float64)}, {"v": b64})["v"]
    verts, joints = ops.body_forward_from_params(ctx, _dev(rows), jaw_pose=t(jaw), expression=t(psi))
    assert float(np.abs(verts.cpu().numpy() - b64).max()) <= bar and joints.shape == (B, 55, 3)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_expression_on_a_model_without_expression_directions_is_refused():
    B, V = 2, 150
    bm, vp = synth.make_body_model(V, seed=0), synth.make_vposer(seed=1)
    bm10 = dataclasses.replace(bm, shapedirs=np.ascontiguousarray(np.asarray(bm.shapedirs)[:, :, :10]))
    ctx = capi.Context(bm10, vp)
    lib, h, st = ctx.lib, ctx.handle, capi.current_stream()
    inp, wv, wj = fs.make_inputs(B, V, seed=B)
    a = [_dev(inp[k]) for k in fs.INPUTS]
    p = [capi.dptr(t) for t in a]
    psi, jaw, rows = _dev(inp["expression"]), _dev(inp["jaw_pose"]), _dev(synth.make_clip(B, seed=3).body_params)
    v, j = torch.empty(B, V, 3, device="cuda"), torch.empty(B, 55, 3, device="cuda")
    cam, sc, gv = _dev(_cameras(B)), _dev([1.8]), _dev(wv)
    gt = [torch.empty(B, w, device="cuda") for w in (3, 63, 10, 12, 12, 3, 10)]
    g = [capi.dptr(t) for t in gt[:6]]
    assert lib.fdcap_smplx_forward_face(h, *p, B, None, capi.dptr(psi), capi.dptr(v), capi.dptr(j), st) == E_STATE
    assert lib.fdcap_smplx_backward_face(h, *p, B, None, capi.dptr(psi), capi.dptr(gv), None, *g, None, capi.dptr(gt[6]), st) == E_STATE
    assert lib.fdcap_body_forward_face(h, capi.dptr(rows), B, None, capi.dptr(psi), capi.dptr(v), capi.dptr(j), st) == E_STATE
    assert lib.fdcap_world_mesh_face(h, capi.dptr(rows), B, None, capi.dptr(psi), capi.dptr(cam), capi.dptr(sc), capi.dptr(v), st) == E_STATE
    with pytest.raises(capi.FdcapError):
        ops.BodyModel(ctx)(return_verts=True, **{k: _dev(inp[k]) for k in fs.INPUTS}, expression=psi)
    # the jaw alone needs no expression directions
    capi.check(lib.fdcap_smplx_forward_face(h, *p, B, capi.dptr(jaw), None, capi.dptr(v), capi.dptr(j), st), "fdcap_smplx_forward_face")
    b64, _, bar = fs.bars_of(bm, inp, "jaw", None, None)
    assert np.abs(v.cpu().numpy() - b64["vertices"]).max() <= bar["vertices"]
    ctx.close()


# ---- 6. the collision term's opt-in: who may call it, and what stays refused without it ------------------------------------------------------
def _coll_op(n, monkeypatch, **kw):
    """an inner fit on synth.make_body_mesh(300) with a registered collision mesh and a map with vertices, standing at its start rows"""
    from fdcap_amd.innerfit import KeypointMap, collision_filter
    monkeypatch.setenv("FDCAP_KP_BLEND", "kernel")
    bm, part, parent = synth.make_body_mesh(300, seed=7)
    vp = synth.make_vposer(seed=8)
    kmap = KeypointMap([3, 15, 20, -1, -1], [(0, 0, 0)] * 3 + [(5, 5, 5), (1, 7, 9)], [(0, 0, 0)] * 3 + [(1, 0, 0), (0.5, 0.3, 0.2)])
    rows = synth.make_clip(n, seed=9, num_outliers=0).body_params.astype(np.float32).copy()
    rows[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32)
    kp = np.concatenate([np.random.default_rng(1).uniform(200, 1000, (n, len(kmap), 2)), np.full((n, len(kmap), 1), 0.7)], -1).astype(np.float32)
    op = InnerFitOP(bm, vp, n, keypoint_map=kmap, iters_per_stage=0, collision=dict(face_part=part, part_parent=parent, capacity=2048, **kw))
    op.fitting(rows, kp)
    return op, (bm, vp, part, collision_filter(part, parent))


def test_collision_opt_in_refusals(monkeypatch):
    import ctypes
    n = 2
    prm = ctypes.byref(capi.CollisionParams(0.5, 1.0, 2048, 0))
    sg = ctypes.byref(capi.Fit2dStage(692, 692, 640, 360, 100.0, 1.0, 4.78, 5.0, 4.78))
    # with the opt-in off, a free jaw and free psi are refused exactly as before: by the setter while they are free, by the evaluation when
    # they are set free afterwards
    op, _ = _coll_op(n, monkeypatch)
    lib, h, st = op.ctx.lib, op.ctx.handle, capi.current_stream()
    jaw, psi = torch.zeros(n, 3, device="cuda"), torch.zeros(n, 10, device="cuda")
    for name, tensor in (("fdcap_opt_set_jaw", jaw), ("fdcap_opt_set_expression", psi)):
        assert lib.fdcap_opt_set_fit2d_collision(h, prm) == 0
        assert getattr(lib, name)(h, capi.dptr(tensor), st) == 0
        assert lib.fdcap_opt_backward_fit2d(h, sg, 0, st) == E_STATE
        assert lib.fdcap_opt_set_fit2d_collision(h, prm) == E_STATE
        # ... and accepted with it: the same calls go through, and off again they are refused again
        assert lib.fdcap_opt_set_fit2d_collision_face(h, 1) == 0
        assert lib.fdcap_opt_set_fit2d_collision(h, prm) == 0
        assert lib.fdcap_opt_backward_fit2d(h, sg, 0, st) == 0
        assert lib.fdcap_opt_set_fit2d_collision_face(h, 0) == 0
        assert lib.fdcap_opt_backward_fit2d(h, sg, 0, st) == E_STATE
        assert getattr(lib, name)(h, None, st) == 0
        assert lib.fdcap_opt_backward_fit2d(h, sg, 0, st) == 0
    torch.cuda.synchronize()
    op.close()
    # Python: without the key the two errors stay, with it the combination is accepted (checked before anything touches the device)
    bm, part, parent = synth.make_body_mesh(300, seed=7)
    vp = synth.make_vposer(seed=8)
    from fdcap_amd.innerfit import KeypointMap
    kmap = KeypointMap([3, 15, 20, -1], [(0, 0, 0)] * 3 + [(5, 5, 5)], [(0, 0, 0)] * 3 + [(1, 0, 0)])
    for kw in (dict(fit_jaw=True), dict(fit_expression=True)):
        with pytest.raises(capi.FdcapError):
            InnerFitOP(bm, vp, n, keypoint_map=kmap, collision=dict(face_part=part, part_parent=parent), **kw)
        InnerFitOP(bm, vp, n, keypoint_map=kmap, collision=dict(face_part=part, part_parent=parent, follow_face=True), **kw).close()
    # no optimiser, a batch of clips and one rank's share of a clip refuse the opt-in as they refuse the term
    ctx = capi.Context(bm, vp)
    ctx.set_collision_mesh(bm.faces, part, None)
    ctx.set_scene(np.zeros((0, 3), np.float32))
    assert ctx.lib.fdcap_opt_set_fit2d_collision_face(ctx.handle, 1) == E_STATE
    N, K = 6, 2
    oc = capi.OptConfig(N, N, 0, 0.01, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)
    state = [torch.zeros(K * N + 4, 78, device="cuda"), torch.zeros(K * N + 4, 16, device="cuda"), torch.ones(K, device="cuda"),
             torch.zeros(K, device="cuda"), torch.zeros(K, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)]
    assert ctx.lib.fdcap_opt_create_clips(ctx.handle, ctypes.byref(oc), K, *[capi.dptr(t) for t in state]) == 0
    assert ctx.lib.fdcap_opt_set_fit2d_collision_face(ctx.handle, 1) == E_STATE
    assert ctx.lib.fdcap_opt_set_fit2d_collision(ctx.handle, prm) == E_STATE
    torch.cuda.synchronize()
    ctx.lib.fdcap_opt_destroy(ctx.handle)
    oc = capi.OptConfig(2 * N, N, N, 0.01, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)          # the second half of a clip of 12
    state = [torch.zeros(N + 4, 78, device="cuda"), torch.zeros(N + 4, 16, device="cuda"), torch.ones(1, device="cuda"),
             torch.zeros(1, device="cuda"), torch.zeros(capi.NUM_LOSSES, device="cuda", dtype=torch.float64)]
    assert ctx.lib.fdcap_opt_create(ctx.handle, ctypes.byref(oc), *[capi.dptr(t) for t in state]) == 0
    assert ctx.lib.fdcap_opt_set_fit2d_collision_face(ctx.handle, 1) == E_STATE
    assert ctx.lib.fdcap_opt_set_fit2d_collision(ctx.handle, prm) == E_STATE
    torch.cuda.synchronize()
    ctx.close()


# ---- 7. the fitted face as a mesh -------------------------------------------------------------------------------------------------------------
def test_innerfit_face_mesh_is_the_twin_at_the_fitted_rows_jaw_and_expression(monkeypatch):
    from fdcap_amd.innerfit import KeypointMap
    from oracle import rotrepr
    from tests.expression_spec import ExpressionSpec
    monkeypatch.setenv("FDCAP_KP_BLEND", "kernel")
    n = 3
    bm, vp = synth.make_body_model(240, seed=7, lbs_nnz=4), synth.make_vposer(seed=8)
    jv = np.flatnonzero(np.asarray(bm.lbs_weights)[:, 22] > 0)              # vertices that follow the jaw: what sees it and psi
    joint = [3, 15, 22, 40] + [-1] * 9
    tri = [(0, 0, 0)] * 4 + [(int(v),) * 3 for v in jv[:8]] + [(int(jv[0]), int(jv[3]), int(jv[5]))]
    bary = [(0, 0, 0)] * 4 + [(1, 0, 0)] * 8 + [(0.5, 0.3, 0.2)]
    kmap = KeypointMap(joint, tri, bary)
    rng = np.random.Generator(np.random.PCG64(10))
    gt = synth.make_clip(n, seed=9, num_outliers=0).body_params.astype(np.float32).copy()
    gt[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32)
    jaw0 = (0.3 * np.array([[1.0, 0.0, 0.0]] * n)).astype(np.float32)
    psi0 = (1.5 * rng.standard_normal((n, 10))).astype(np.float32)
    spec = ExpressionSpec(bm, vp, joint, tri, bary)
    x = rotrepr.convert_to_6D_rot(torch.tensor(gt, dtype=torch.float64)).numpy()
    uv = spec.project(torch.tensor(spec.positions(x, jaw0, psi0))).numpy()
    kp = np.concatenate([uv, np.full((n, len(kmap), 1), 0.8)], -1).astype(np.float32)
    init = gt
    op = InnerFitOP(bm, vp, n, keypoint_map=kmap, fit_jaw=True, fit_expression=True, iters_per_stage=3)
    with pytest.raises(capi.FdcapError):
        op.face_mesh()
    rows = op.fitting(init, kp)
    got = op.face_mesh().cpu().numpy()
    r, jaw, psi = rows.cpu().numpy(), op.jaw_pose.cpu().numpy(), op.expression.cpu().numpy()
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n, 1))
    w64, w32 = fs.world_vertices(bm, vp, r, 1.0, eye, jaw, psi), fs.world_vertices(bm, vp, r, 1.0, eye, jaw, psi, dtype=torch.float32)
    shut = fs.world_vertices(bm, vp, r, 1.0, eye)
    bar = gb.bars({"v": w32.astype(np.float64)}, {"v": w64})["v"]
    err = float(np.abs(got - w64).max())
    print(f"face_mesh: max|err| {err:.3e} bar {bar:.3e}; the fitted face moves a vertex by {np.abs(w64 - shut).max():.3e}")
    assert np.abs(jaw).max() > 0 and np.abs(psi).max() > 0 and np.abs(w64 - shut).max() > 10 * bar
    assert err <= bar
    op.close()
