"""GPU parity tests: every call goes through the C-ABI (libfdcap_hip.so) on a real MI355X and is
compared with the oracle on the same seeded inputs, with the committed reference-generated
goldens, and -- at BASELINE sizes -- through size-independent properties."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, ops, synth
from fdcap_amd.fitting import FittingOP, find_outliers, first_phase2_iter
from fdcap_amd.io import read_camerapose
from oracle import rotrepr
from oracle.chamfer import nn_direct, pairwise_dist
from oracle.fitting import FittingOracle
from oracle.smplx import SMPLXOracle
from oracle.vposer import VPoserDecoder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    bm = synth.make_body_model(300, seed=0)
    vp = synth.make_vposer(seed=1)
    ctx = capi.Context(bm, vp)
    yield bm, vp, ctx
    ctx.close()


def _nn_check(q, t, dist, idx):
    """dist/idx from the HIP path vs the oracle's direct-difference scan.  Distances must agree
    to fp32 rounding (the kernel contracts to FMA, torch-CPU does not); an index may differ only
    between candidates whose oracle distances are equal to that rounding."""
    od, oi = nn_direct(torch.from_numpy(q), torch.from_numpy(t))
    od, oi = od.numpy(), oi.numpy()
    np.testing.assert_allclose(dist, od, rtol=2e-6, atol=1e-12)
    diff = idx != oi
    if diff.any():
        d_at = ((q[diff] - t[idx[diff]]) ** 2).sum(1)
        np.testing.assert_allclose(d_at, od[diff], rtol=4e-6, atol=1e-12)
    assert diff.mean() < 1e-3


@pytest.mark.parametrize("B,n,m", [(1, 1, 1), (2, 37, 5), (3, 64, 1024), (2, 300, 1500), (1, 513, 9000), (4, 100, 33000)])
def test_chamfer_shared_scene_matches_oracle(small, B, n, m):
    _, _, ctx = small
    rng = np.random.default_rng(B * 1000 + n + m)
    q = rng.uniform(-3, 3, (B, n, 3)).astype(np.float32)
    t = rng.uniform(-3, 3, (m, 3)).astype(np.float32)
    cd = ops.chamferDist(ctx, both=False)
    d1, _ = cd(torch.tensor(q).cuda(), torch.tensor(t).cuda().unsqueeze(0).expand(B, -1, -1))
    _nn_check(q.reshape(-1, 3), t, d1.cpu().numpy().reshape(-1), cd.last_idx1.cpu().numpy().reshape(-1).astype(np.int64))


def test_chamfer_both_directions_and_backward(small):
    """The reference's own call shape: per-batch scene copies, both directions (:292-294)."""
    _, _, ctx = small
    from oracle.chamfer import chamferDist as OracleChamfer
    rng = np.random.default_rng(7)
    a = rng.uniform(-1, 1, (3, 50, 3)).astype(np.float32)
    b = rng.uniform(-1, 1, (3, 700, 3)).astype(np.float32)
    ta, tb = torch.tensor(a, requires_grad=True), torch.tensor(b, requires_grad=True)
    o1, o2 = OracleChamfer(False)(ta, tb)
    w1 = torch.tensor(rng.standard_normal((3, 50)).astype(np.float32))
    w2 = torch.tensor(rng.standard_normal((3, 700)).astype(np.float32))
    ((o1 * w1).sum() + (o2 * w2).sum()).backward()
    ga, gb = torch.tensor(a).cuda().requires_grad_(True), torch.tensor(b).cuda().requires_grad_(True)
    d1, d2 = ops.chamferDist(ctx, both=True)(ga, gb)
    ((d1 * w1.cuda()).sum() + (d2 * w2.cuda()).sum()).backward()
    np.testing.assert_allclose(d1.detach().cpu().numpy(), o1.detach().numpy(), rtol=2e-6)
    np.testing.assert_allclose(d2.detach().cpu().numpy(), o2.detach().numpy(), rtol=2e-6)
    np.testing.assert_allclose(ga.grad.cpu().numpy(), ta.grad.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gb.grad.cpu().numpy(), tb.grad.numpy(), rtol=1e-5, atol=1e-6)


def test_chamfer_equal_sizes_vs_reference_chamfer_python(small):
    """chamfer_python.pairwise_dist (expansion form, equal sizes only, chamfer_python.py:4-9)."""
    _, _, ctx = small
    rng = np.random.default_rng(3)
    x = rng.uniform(-8, 8, (256, 3)).astype(np.float32)
    y = rng.uniform(-8, 8, (256, 3)).astype(np.float32)
    P = pairwise_dist(torch.tensor(x), torch.tensor(y))
    d1, _ = ops.chamferDist(ctx, both=False)(torch.tensor(x).cuda()[None], torch.tensor(y).cuda()[None])
    # the expansion form loses ~1e-4 absolute at this coordinate scale
    np.testing.assert_allclose(d1.cpu().numpy()[0], P.min(dim=1)[0].numpy(), atol=2e-4)


def test_chamfer_vs_the_reference_files_own_outputs(small, golden_dir):
    """A18 against tests/golden/ref_chamfer_python.npz: outputs of /root/reference/chamfer_python.py itself
    (pairwise_dist, NN_loss, distChamfer; make_golden.py --chamfer).  The reference file uses the expansion form
    ||x||^2 + ||y||^2 - 2 x.y, which loses ~1e-7 * (||x||^2 + ||y||^2) per entry against the direct-difference form the
    CUDA extension and the HIP kernel use: that, stated per case, is the bar.  distChamfer returns (y->x, x->y, ...) --
    the opposite order of chamferDist's (dist1 = x->y, dist2 = y->x), chamfer_python.py:28."""
    _, _, ctx = small
    g = np.load(os.path.join(golden_dir, "ref_chamfer_python.npz"))
    cd = ops.chamferDist(ctx, both=True)
    for tag in ("a", "b", "c"):
        x, y = g[f"{tag}_x"], g[f"{tag}_y"]
        tol = 4e-6 * float((x * x).sum(1).max() + (y * y).sum(1).max())
        d1, d2 = cd(torch.tensor(x).cuda()[None], torch.tensor(y).cuda()[None])
        d1, d2 = d1.cpu().numpy()[0], d2.cpu().numpy()[0]
        if f"{tag}_P" in g.files:
            pmin_x, pmin_y = g[f"{tag}_P"].min(axis=1), g[f"{tag}_P"].min(axis=0)
        else:
            pmin_x, pmin_y = g[f"{tag}_Pmin1"], g[f"{tag}_Pmin0"]
        np.testing.assert_allclose(d1, pmin_x, rtol=0, atol=tol)            # x -> y = min over the y index
        np.testing.assert_allclose(d2, pmin_y, rtol=0, atol=tol)
        np.testing.assert_allclose(d2.mean(), float(g[f"{tag}_nn0"]), rtol=0, atol=tol)   # NN_loss(dim=0): mean over y of min over x
        np.testing.assert_allclose(d1.mean(), float(g[f"{tag}_nn1"]), rtol=0, atol=tol)
    a, b = g["d_a"], g["d_b"]
    tol = 4e-6 * float((a * a).sum(-1).max() + (b * b).sum(-1).max())
    d1, d2 = cd(torch.tensor(a).cuda(), torch.tensor(b).cuda())
    np.testing.assert_allclose(d2.cpu().numpy(), g["d_ret0"], rtol=0, atol=tol)   # distChamfer's FIRST output is y -> x
    np.testing.assert_allclose(d1.cpu().numpy(), g["d_ret1"], rtol=0, atol=tol)
    assert (cd.last_idx1.cpu().numpy() == g["d_ret3"]).mean() > 0.98              # (argmins may differ between rounding ties)


def test_chamfer_full_size_properties(small):
    """BASELINE config 2 size (256 frames x 500 contact verts vs a 100k scene): properties."""
    _, _, ctx = small
    rng = np.random.default_rng(11)
    scene = synth.make_scene(100_000, seed=2)
    q = (rng.uniform(-2, 2, (256, 500, 3)) * [1, 1, 0.3]).astype(np.float32)
    tq, ts = torch.tensor(q).cuda(), torch.tensor(scene).cuda()
    cd = ops.chamferDist(ctx, both=False)
    d, _ = cd(tq, ts.unsqueeze(0).expand(256, -1, -1))
    idx = cd.last_idx1.long()
    assert int(idx.min()) >= 0 and int(idx.max()) < scene.shape[0]
    # (1) the reported distance is the distance to the reported neighbour
    nb = ts[idx.reshape(-1)].reshape(256, 500, 3)
    rec = ((tq - nb) ** 2).sum(-1)
    torch.testing.assert_close(d, rec, rtol=2e-6, atol=1e-12)
    # (2) no sampled scene point is closer
    samp = ts[torch.randint(0, scene.shape[0], (4096,), device="cuda")]
    dmin = ((tq.reshape(-1, 3)[:4096, None, :] - samp[None, :, :]) ** 2).sum(-1).min(dim=1)[0]   # direct form
    assert bool((d.reshape(-1)[:4096] <= dmin * (1 + 4e-6) + 1e-12).all())
    # (3) shuffling the scene leaves every distance unchanged
    perm = torch.randperm(scene.shape[0], device="cuda")
    d2, _ = cd(tq, ts[perm].unsqueeze(0).expand(256, -1, -1))
    assert torch.equal(d, d2)
    # (4) exact agreement with the oracle on a slice the CPU finishes in seconds
    od, oi = nn_direct(torch.tensor(q[0]), torch.tensor(scene))
    np.testing.assert_allclose(d[0].cpu().numpy(), od.numpy(), rtol=2e-6)


@pytest.mark.parametrize("case", ["uniform", "floor", "ties", "far_queries", "tiny_scene"])
def test_mfma_filtered_nn_is_bit_identical_to_direct_scan(small, case):
    """The bf16-split MFMA score only filters; every reported (dist, idx) must equal the plain
    fp32 scan's bit for bit -- including adversarial inputs: exact ties (lowest index wins),
    queries far from their workgroup centroid (large filter slack), scenes smaller than a tile."""
    _, _, ctx = small
    rng = np.random.default_rng(21)
    B, n, m = 40, 300, 40_000
    q = rng.uniform(-2, 2, (B, n, 3)).astype(np.float32)
    t = rng.uniform(-5, 5, (m, 3)).astype(np.float32)
    if case == "floor":
        t[:, 2] = rng.normal(0, 0.005, m)
        q[..., 2] = np.abs(q[..., 2]) * 0.05
    elif case == "ties":
        t = np.round(t * 4) / 4                          # lattice: many exactly equidistant points
        t = np.concatenate([t, t[:5000]])                # and exact duplicates at higher indices
        q = np.round(q * 8) / 8
    elif case == "far_queries":
        q[::7] += rng.uniform(-60, 60, (q[::7].shape[0], 1, 3)).astype(np.float32)   # whole frames far away
        q[:, ::11] += rng.uniform(-30, 30, (B, q[:, ::11].shape[1], 3)).astype(np.float32)  # stragglers inside a workgroup
    elif case == "tiny_scene":
        t = t[:37]
        B, n = 64, 512
        q = rng.uniform(-2, 2, (B, n, 3)).astype(np.float32)
    tq, tt = torch.tensor(q).cuda(), torch.tensor(t).cuda()
    res = {}
    for mode in (1, 2):
        capi.check(ctx.lib.fdcap_set_nn_kernel(mode), "set_nn_kernel")
        cd = ops.chamferDist(ctx, both=False)
        d, _ = cd(tq, tt.unsqueeze(0).expand(tq.shape[0], -1, -1))
        res[mode] = (d.clone(), cd.last_idx1.clone())
    capi.check(ctx.lib.fdcap_set_nn_kernel(0), "set_nn_kernel")
    assert torch.equal(res[1][0], res[2][0])
    assert torch.equal(res[1][1], res[2][1])
    if case == "ties":   # lowest index among exact ties, as an ascending strict-< scan gives
        od, oi = nn_direct(torch.tensor(q[0]), torch.tensor(t))
        assert np.array_equal(res[2][1][0].cpu().numpy(), oi.numpy())


def test_vposer_decode_matches_oracle(small):
    bm, vp, ctx = small
    rng = np.random.default_rng(5)
    for B in (1, 7, 130):
        z = rng.standard_normal((B, 32)).astype(np.float32)
        orc = VPoserDecoder.from_data(vp)
        want_rot = orc.decode(torch.tensor(z), output_type="matrot").numpy()
        want_aa = orc.decode(torch.tensor(z), output_type="aa").numpy()
        v = ops.VPoser(ctx)
        # K=512 fp32 accumulation order differs (MFMA k-ordered fmaf chain vs blocked CPU GEMM); Gram-Schmidt
        # amplifies the ~1e-6 differences of the 6D code by 1/|u|: measured max 1.2e-5 on rotation entries
        np.testing.assert_allclose(v.decode(torch.tensor(z).cuda(), "matrot").cpu().numpy(), want_rot, atol=4e-5)
        np.testing.assert_allclose(v.decode(torch.tensor(z).cuda(), "aa").cpu().numpy(), want_aa, atol=1e-4)


def test_body_model_operator_matches_oracle(small):
    bm, vp, ctx = small
    rng = np.random.default_rng(9)
    B = 5
    kw = dict(body_pose=rng.standard_normal((B, 63)) * 0.3, transl=rng.standard_normal((B, 3)),
              global_orient=rng.standard_normal((B, 3)), betas=rng.standard_normal((B, 10)),
              left_hand_pose=rng.standard_normal((B, 12)), right_hand_pose=rng.standard_normal((B, 12)))
    kw = {k: torch.tensor(v, dtype=torch.float32) for k, v in kw.items()}
    want = SMPLXOracle(bm)(return_verts=True, **kw)
    got = ops.BodyModel(ctx)(return_verts=True, **{k: v.cuda() for k, v in kw.items()})
    np.testing.assert_allclose(got.vertices.cpu().numpy(), want.vertices.numpy(), atol=2e-5)
    np.testing.assert_allclose(got.joints.cpu().numpy(), want.joints.numpy(), atol=2e-5)


def test_body_forward_from_file_rows(small):
    """[N,75] rows -> vertices: VPoser decode + SMPL-X as global_vis.py:131-146 chains them."""
    bm, vp, ctx = small
    clip = synth.make_clip(9, seed=4)
    p = torch.tensor(clip.body_params)
    aa = VPoserDecoder.from_data(vp).decode(p[:, 16:48], output_type="aa").view(9, -1)
    want = SMPLXOracle(bm)(return_verts=True, body_pose=aa, transl=p[:, 0:3], global_orient=p[:, 3:6], betas=p[:, 6:16],
                           left_hand_pose=p[:, 48:60], right_hand_pose=p[:, 60:72])
    verts, joints = ops.body_forward_from_params(ctx, p.cuda())
    np.testing.assert_allclose(verts.cpu().numpy(), want.vertices.numpy(), atol=3e-5)
    np.testing.assert_allclose(joints.cpu().numpy(), want.joints.numpy(), atol=3e-5)


def test_param_conversions_vs_reference_golden(small, golden_dir):
    _, _, ctx = small
    u = np.load(os.path.join(golden_dir, "ref_units.npz"))
    x75 = torch.tensor(u["x75"]).cuda()
    x78 = torch.empty(16, 78, device="cuda")
    capi.check(ctx.lib.fdcap_params_75_to_78(capi.dptr(x75), 16, capi.dptr(x78), capi.current_stream()), "75->78")
    np.testing.assert_allclose(x78.cpu().numpy(), u["x78"], atol=1e-6)       # device sin/cos: 1-2 ulp
    back = torch.empty(16, 75, device="cuda")
    capi.check(ctx.lib.fdcap_params_78_to_75(capi.dptr(torch.tensor(u["x78"]).cuda()), 16, capi.dptr(back),
                                             capi.current_stream()), "78->75")
    np.testing.assert_allclose(back.cpu().numpy(), u["x75_back"], atol=3e-6)


def _make_fop(n, V, ns, per_part, num_iter, seed=0, weight_contact=0.1):
    bm = synth.make_body_model(V, seed=seed)
    vp = synth.make_vposer(seed=seed + 1)
    clip = synth.make_clip(n, seed=seed + 2)
    scene = synth.make_scene(ns, seed=seed + 3)
    left, right = synth.make_contact_ids(bm.v_template, per_part=per_part, seed=seed + 4)
    vid = np.concatenate([left, right])
    fop = FittingOP({"num_iter": num_iter}, {"weight_contact": weight_contact}, n, body_model=bm, vposer=vp,
                    scene_verts=scene, contact_ids=vid, camera_ext=read_camerapose(clip.camerapose_lines))
    return fop, bm, vp, clip, scene, vid


@pytest.mark.parametrize("phase2", [False, True])
def test_optimiser_gradients_match_autograd(phase2):
    _gradient_check(12, 300, 800, 20, 0, phase2)


@pytest.mark.parametrize("n,V,ns,per_part,seed", [(4, 120, 50, 1, 11), (7, 777, 801, 7, 12), (19, 300, 5000, 40, 13), (33, 150, 333, 3, 14),
                                                   (65, 512, 2049, 17, 15), (130, 240, 1000, 9, 16)])
def test_optimiser_gradients_match_autograd_at_ragged_shapes(n, V, ns, per_part, seed):
    """The same check at shapes nobody tuned for: frames not a multiple of the 16-row blocks, vertex counts not a multiple of
    anything, one contact vertex per leg, scenes smaller than a k-d chunk and just past a power of two; both phases."""
    _gradient_check(n, V, ns, per_part, seed, seed % 2 == 0)


def _gradient_check(n, V, ns, per_part, seed, phase2):
    fop, bm, vp, clip, scene, vid = _make_fop(n, V, ns, per_part, 500, seed=seed)
    dt = torch.float64
    f = FittingOracle(SMPLXOracle(bm, dt), VPoserDecoder.from_data(vp, dt), scene, vid, clip.camerapose_lines, n, dtype=dt)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(clip.body_params, dtype=dt)).detach()
    f.init(x78)
    g = torch.Generator().manual_seed(5)
    pert = 0.01 * torch.randn(f.body_rotation_rec.shape, generator=g, dtype=dt)
    f.body_rotation_rec.data += pert
    idx1, _ = find_outliers(x78.numpy().astype(np.float32))
    l_rec, l_vp, l_con, l_sm, l_ws = f.cal_loss(x78, idx1)
    ((l_rec + l_ws + 0.5 * l_sm) if phase2 else (0.1 * l_con + l_sm + l_rec)).backward()
    # same state on the GPU
    x78g = torch.tensor(x78.numpy(), dtype=torch.float32).cuda()
    fop.init(x78g)
    fop._rows_x[2:2 + n] += pert.float().cuda()
    lib, h = fop.ctx.lib, fop.ctx.handle
    P = 0 if phase2 else 10 ** 6
    capi.check(lib.fdcap_opt_backward(h, 5, P, 1, capi.current_stream()), "backward")
    dx = torch.empty(n, 78, device="cuda")
    dcam = torch.empty(n, 16, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), capi.dptr(dcam), capi.current_stream()), "grads")
    torch.cuda.synchronize()
    gx = f.body_rotation_rec.grad.numpy()
    np.testing.assert_allclose(dx.cpu().numpy(), gx, rtol=2e-3, atol=2e-4 * np.abs(gx).max())
    s = fop._losses.cpu().numpy()
    np.testing.assert_allclose(s[0] / (n * 78), float(l_rec.detach()), rtol=1e-5)
    np.testing.assert_allclose(0.001 * s[1] / (n * 32), float(l_vp.detach()), rtol=1e-5)
    np.testing.assert_allclose(s[2] / ((n - 2) * 78), float(l_sm.detach()), rtol=1e-5)
    np.testing.assert_allclose(s[4] / ((n - 1) * 69), float(l_ws.detach()), rtol=1e-4)
    np.testing.assert_allclose(0.1 * s[3] / (n * len(vid)), float(l_con.detach()), rtol=1e-5)
    if phase2:
        gc = f.camera_ext.grad.numpy().reshape(n, 16)
        np.testing.assert_allclose(dcam.cpu().numpy(), gc, rtol=2e-3, atol=2e-4 * np.abs(gc).max())
    else:
        np.testing.assert_allclose(float(fop._dscale.cpu()), float(f.scale.grad), rtol=2e-3)
    fop.close()


def test_forward_world_matches_oracle():
    n = 10
    fop, bm, vp, clip, scene, vid = _make_fop(n, 300, 800, 20, 500)
    f = FittingOracle(SMPLXOracle(bm), VPoserDecoder.from_data(vp), scene, vid, clip.camerapose_lines, n)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(clip.body_params)).detach()
    f.init(x78)
    with torch.no_grad():
        _, verts, joints = f.forward_world()
    fop.init(x78.cuda())
    v = torch.empty(n, len(vid), 3, device="cuda")
    j = torch.empty(n, 23, 3, device="cuda")
    capi.check(fop.ctx.lib.fdcap_opt_forward_world(fop.ctx.handle, capi.dptr(v), capi.dptr(j), capi.current_stream()), "fw")
    np.testing.assert_allclose(v.cpu().numpy(), verts[:, vid].numpy(), atol=3e-5)
    np.testing.assert_allclose(j.cpu().numpy(), joints.numpy(), atol=3e-5)
    fop.close()


@pytest.mark.parametrize("name", ["ref_global_5it.npz", "ref_global_20it.npz"])
def test_trajectory_matches_reference_golden(golden_dir, name):
    """FittingOP.fitting on the GPU vs what the REFERENCE'S OWN loop produced on the same inputs.
    Tolerances: see tests/test_host_math.py (Adam + L1 kinks; yardstick = fp64 oracle vs the fp32
    reference run: q50 2e-8, q90 2e-7, q99 4e-4, max 1.1e-2)."""
    g = np.load(os.path.join(golden_dir, name))
    bm = synth.make_body_model(int(g["num_verts"]), seed=int(g["model_seed"]))
    vp = synth.make_vposer(seed=int(g["vposer_seed"]))
    num_iter = int(g["num_iter"])
    fop = FittingOP({"num_iter": num_iter}, {}, 300, body_model=bm, vposer=vp, scene_verts=g["scene"],
                    contact_ids=g["vid"], camera_ext=read_camerapose(list(g["camerapose"])))
    body, scale, cam = fop.fitting(torch.tensor(g["body_in"]).cuda(), "global", log_every=1)
    np.testing.assert_array_equal(fop.idx1, g["idx1"])
    err = np.abs(body.cpu().numpy() - g["body_rec"])
    q50, q90, q99 = np.quantile(err, [0.5, 0.9, 0.99])
    assert err.max() <= 6 * 0.005          # (three sign flips of one entry; measured <= 1.1e-2.  The r3 bound 2 lr num_iter held for ANY Adam run)
    assert q50 < 1e-6 and q90 < 1e-4 and q99 < 3e-3, (q50, q90, q99)
    assert err[:, 48:72].max() <= 2e-6
    np.testing.assert_allclose(float(scale), float(g["scale"]), atol=1e-4)
    P = first_phase2_iter(num_iter)
    np.testing.assert_allclose(cam.cpu().numpy(), g["camera_ext"], atol=2 * 0.005 * max(num_iter - P - 1, 0) + 1e-6)
    tol = 3e-6 + 2e-6 * np.arange(num_iter)
    log = fop.log
    assert np.all(np.abs(np.array(log.l_rec) - g["log"][:, 1]) <= tol)
    assert np.all(np.abs(np.array(log.l_vposer) - g["log"][:, 2]) <= tol)
    assert np.all(np.abs(np.array(log.loss_smoothing) - g["log"][:, 3]) <= tol)
    # in phase 2 the contact term is log-only and sees camera_ext moving +-lr per step (sign-normalised)
    assert np.all(np.abs(np.array(log.loss_contact) - g["log"][:, 4]) <= np.where(np.arange(num_iter) > P, 4 * tol, tol))
    # the phase-2 total contains the camera_ext-sensitive world term (see below)
    assert np.all(np.abs(np.array(log.total) - g["log"][:, 6]) <= np.where(np.arange(num_iter) > P, 5 * tol, 2 * tol))
    # same camera_ext sensitivity: measured up to 6e-5 at iteration 19 depending on GEMM summation order
    assert np.all(np.abs(np.array(log.loss_world_smoothing)[P:] - g["log"][P:, 5]) <= 4 * tol[P:])
    fop.close()


def test_seeding_the_nn_bound_does_not_change_results():
    """The optimiser seeds each NN search with the previous call's neighbour (an exact upper bound
    that only prunes) and skips scene cells (k-d boxes) that are out of every query's reach:
    cold search, search seeded by its own result, and search seeded by a STALE result (state moved
    in between), with and without chunk culling, must all equal the plain answer bit for bit."""
    n = 64
    clip_x = None

    def contact(fop):
        d = torch.empty(n, len(fop.vid), device="cuda")
        i = torch.empty(n, len(fop.vid), device="cuda", dtype=torch.int32)
        capi.check(fop.ctx.lib.fdcap_opt_forward_world(fop.ctx.handle, capi.dptr(torch.empty(n, len(fop.vid), 3, device="cuda")),
                                                       None, capi.current_stream()), "fw")
        capi.check(fop.ctx.lib.fdcap_opt_get_contact(fop.ctx.handle, capi.dptr(d), capi.dptr(i), capi.current_stream()), "gc")
        torch.cuda.synchronize()
        return d.clone(), i.clone()

    res = {}
    for flag, cull in (("0", "0"), ("1", "0"), ("1", "1")):
        os.environ["FDCAP_NN_SEED"] = flag
        os.environ["FDCAP_NN_CULL"] = cull
        fop, bm, vp, clip, scene, vid = _make_fop(n, 300, 70_000, 40, 8, seed=60)
        x78 = torch.empty(n, 78, device="cuda")
        capi.check(fop.ctx.lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(clip.body_params).cuda()), n, capi.dptr(x78),
                                                     capi.current_stream()), "75->78")
        fop.init(x78)
        a = contact(fop)                 # cold
        b = contact(fop)                 # seeded by its own result (flag 1)
        g = torch.Generator(device="cuda").manual_seed(3)
        fop._rows_x[2:2 + n, 0:3] += 0.03 * torch.randn(n, 3, device="cuda", generator=g)     # move the bodies
        fop._rows_x[2:2 + n, 19:51] += 0.05 * torch.randn(n, 32, device="cuda", generator=g)
        c = contact(fop)                 # seeded by a stale result (flag 1)
        res[flag + cull] = (a, b, c)
        fop.close()
    os.environ.pop("FDCAP_NN_SEED")
    os.environ.pop("FDCAP_NN_CULL")
    for cfg in ("10", "11"):          # seeded; seeded + culled (k-d-cell-ordered scene, cell boxes)
        for k in range(3):
            assert torch.equal(res["00"][k][0], res[cfg][k][0]) and torch.equal(res["00"][k][1], res[cfg][k][1]), (cfg, k)
    assert not torch.equal(res["11"][1][1], res["11"][2][1])     # the stale seeds really were stale


@pytest.mark.parametrize("n,per_part", [(64, 40), (256, 200)])       # 5 k queries: four waves per group; 102 k: one-wave workgroups
def test_kept_work_lists_do_not_change_results(n, per_part):
    """The in-loop NN launch keeps each group's work list (built with slack) while the queries stay inside the region it was
    built for.  That only prunes: over a sequence of millimetre moves (lists kept), a 3 cm jump (lists rebuilt) and more small
    moves, every launch must equal the launch without kept lists, bit for bit -- for a slack that is never outrun, the
    default, and one that is outrun at almost every launch."""
    def run(slack):
        os.environ["FDCAP_NN_CACHE_SLACK"] = slack
        try:
            fop, bm, vp, clip, scene, vid = _make_fop(n, 1000, 70_000, per_part, 8, seed=60)
            x78 = torch.empty(n, 78, device="cuda")
            capi.check(fop.ctx.lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(clip.body_params).cuda()), n, capi.dptr(x78),
                                                         capi.current_stream()), "75->78")
            fop.init(x78)
            g = torch.Generator(device="cuda").manual_seed(11)
            out = []
            for k in range(45):
                step = 0.03 if k == 25 else 0.001
                fop._rows_x[2:2 + n, 0:3] += step * torch.randn(n, 3, device="cuda", generator=g)
                d = torch.empty(n, len(fop.vid), device="cuda")
                i = torch.empty(n, len(fop.vid), device="cuda", dtype=torch.int32)
                capi.check(fop.ctx.lib.fdcap_opt_forward_world(fop.ctx.handle, capi.dptr(torch.empty(n, len(fop.vid), 3, device="cuda")),
                                                               None, capi.current_stream()), "fw")
                capi.check(fop.ctx.lib.fdcap_opt_get_contact(fop.ctx.handle, capi.dptr(d), capi.dptr(i), capi.current_stream()), "gc")
                out.append((d.clone(), i.clone()))
            torch.cuda.synchronize()
            fop.close()
            return out
        finally:
            os.environ.pop("FDCAP_NN_CACHE_SLACK")

    base = run("0")
    for slack in ("0.04", "0.5", "0.002"):
        got = run(slack)
        for k, ((d0, i0), (d1, i1)) in enumerate(zip(base, got)):
            assert torch.equal(d0, d1) and torch.equal(i0, i1), (slack, k)
    assert not torch.equal(base[24][1], base[25][1])                 # the jump really changed neighbours


def test_far_stale_seeds_overflow_the_work_list_and_stay_exact():
    """A seed is only an upper bound: after the bodies jump by metres every query's ball covers most of a 160k-point scene
    (313 k-d cells), more than a wave can list (ST4_MAXCELL = 256 chunks / ST4_MAXLIST = 768 quarter chunks), and the
    streaming kernel has to fall back to scanning its whole share -- the result must still be the plain scan's, bit for bit."""
    n = 48
    res = {}
    for flag, cull in (("0", "0"), ("1", "1")):
        os.environ["FDCAP_NN_SEED"] = flag
        os.environ["FDCAP_NN_CULL"] = cull
        try:
            fop, bm, vp, clip, scene, vid = _make_fop(n, 300, 160_000, 40, 8, seed=90)
            x78 = torch.empty(n, 78, device="cuda")
            capi.check(fop.ctx.lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(clip.body_params).cuda()), n, capi.dptr(x78),
                                                         capi.current_stream()), "75->78")
            fop.init(x78)

            def contact():
                d = torch.empty(n, len(fop.vid), device="cuda")
                i = torch.empty(n, len(fop.vid), device="cuda", dtype=torch.int32)
                capi.check(fop.ctx.lib.fdcap_opt_forward_world(fop.ctx.handle, capi.dptr(torch.empty(n, len(fop.vid), 3, device="cuda")),
                                                               None, capi.current_stream()), "fw")
                capi.check(fop.ctx.lib.fdcap_opt_get_contact(fop.ctx.handle, capi.dptr(d), capi.dptr(i), capi.current_stream()), "gc")
                torch.cuda.synchronize()
                return d.clone(), i.clone()

            a = contact()
            fop._rows_x[2:2 + n, 0:3] += torch.tensor([4.0, -3.0, 2.5], device="cuda")        # metres away from the seeds
            b = contact()
            fop._rows_x[2:2 + n, 0:3] -= torch.tensor([4.0, -3.0, 2.5], device="cuda")        # and back: seeds from far away again
            c = contact()
            res[flag + cull] = (a, b, c)
            fop.close()
        finally:
            os.environ.pop("FDCAP_NN_SEED")
            os.environ.pop("FDCAP_NN_CULL")
    for k in range(3):
        assert torch.equal(res["00"][k][0], res["11"][k][0]) and torch.equal(res["00"][k][1], res["11"][k][1]), k
    assert torch.equal(res["11"][0][0], res["11"][2][0])


@pytest.mark.parametrize("ns", [40, 600, 5000])
def test_in_loop_nn_state_survives_the_timing_api_and_small_scenes(ns):
    """The seeded launch keeps each neighbour's coordinates next to its index; a brute-force timing launch rewrites the
    indices only.  After fit -> brute-force timing -> in-loop timing the contact result must still be the oracle's NN.
    Scenes smaller than one k-d cell / one tile go through the same calls."""
    n = 24
    fop, bm, vp, clip, scene, vid = _make_fop(n, 300, ns, 40, 6, seed=70 + ns)
    lib, h = fop.ctx.lib, fop.ctx.handle
    lib.fdcap_set_nn_kernel(2)                       # the MFMA / streaming kernels whatever the size (default: plain scan below 4 M pairs)
    try:
        _in_loop_nn_state_body(fop, clip, scene, vid, n, lib, h)
    finally:
        lib.fdcap_set_nn_kernel(0)
        fop.close()


def _in_loop_nn_state_body(fop, clip, scene, vid, n, lib, h):
    fop.fitting(torch.tensor(clip.body_params).cuda(), "global")
    ms = ctypes.c_float(0)
    for brute in (1, 0, 0):
        capi.check(lib.fdcap_opt_time_chamfer(h, 2, brute, ctypes.byref(ms), capi.current_stream()), "time_chamfer")
    verts = torch.empty(n, len(vid), 3, device="cuda")
    capi.check(lib.fdcap_opt_forward_world(h, capi.dptr(verts), None, capi.current_stream()), "fw")
    d = torch.empty(n, len(vid), device="cuda")
    i = torch.empty(n, len(vid), device="cuda", dtype=torch.int32)
    capi.check(lib.fdcap_opt_get_contact(h, capi.dptr(d), capi.dptr(i), capi.current_stream()), "gc")
    _nn_check(verts.cpu().numpy().reshape(-1, 3), scene, d.cpu().numpy().reshape(-1), i.cpu().numpy().reshape(-1).astype(np.int64))


def test_runs_are_bit_reproducible():
    """No float atomics on the gradient path: two runs of the same clip give identical bits -- and, with every loss term
    logged every iteration (per-frame partial sums + one fixed-order reduction, no atomics either), identical logs; logging
    does not change the fit."""
    outs = []
    for log_every in (0, 1, 1):
        fop, bm, vp, clip, scene, vid = _make_fop(48, 300, 20_000, 40, 12, seed=70)
        body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=log_every)
        log = np.array([fop.log.l_rec, fop.log.l_vposer, fop.log.loss_smoothing, fop.log.loss_contact, fop.log.loss_world_smoothing, fop.log.total]) if log_every else None
        outs.append((body.clone(), float(scale), cam.clone(), log))
        fop.close()
    for a, b in ((0, 1), (1, 2)):
        assert torch.equal(outs[a][0], outs[b][0]) and outs[a][1] == outs[b][1] and torch.equal(outs[a][2], outs[b][2])
    assert outs[1][3].shape[1] == 12 and np.array_equal(outs[1][3], outs[2][3])


@pytest.mark.parametrize("mode,legacy,log_every", [("global", False, 0), ("global", True, 0), ("local", False, 0), ("global", False, 1),
                                                   ("global", True, 3), ("local", False, 1)])
def test_deferred_optimiser_step_gives_the_same_bits(mode, legacy, log_every):
    """fdcap_opt_step_deferred (r4): optimizer.step() (:592) without a launch of its own -- the next iteration's decoder and
    per-frame pose kernels apply the Adam update where they read the parameters.  Same arithmetic in the same order as the Adam
    kernel: whole fits (30 iterations across the phase switch; torch < 2 zero_grad semantics, where `scale` keeps coasting in
    phase 2; mode 'local' with its second loop behind it) agree bit for bit with FDCAP_DEFER_STEP=0, and a snapshot taken in
    the middle of the deferred run (which forces the pending step out through the ordinary launch) equals the same snapshot of
    the other run.  log_every > 0: the printed sums of a logging iteration are reduced by the extra workgroup that steps
    `scale` (phase 2: by that workgroup alone) instead of the Adam launch -- the same fixed-order tree, the same log."""
    outs = []
    for flag in ("0", "1"):
        os.environ["FDCAP_DEFER_STEP"] = flag
        try:
            n = 37
            bm = synth.make_body_model(300, seed=72)
            vp = synth.make_vposer(seed=73)
            clip = synth.make_clip(n, seed=74)
            scene = synth.make_scene(6000, seed=75)
            left, right = synth.make_contact_ids(bm.v_template, per_part=20, seed=76)
            fop = FittingOP({"num_iter": 30}, {}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=np.concatenate([left, right]),
                            camera_ext=read_camerapose(clip.camerapose_lines), legacy_zero_grad=legacy, n_left=len(left))
            kw = {"snapshot_at": [7, 26]} if mode == "global" else {}
            body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), mode, log_every=log_every, **kw)
            snaps = [tuple(t.clone() for t in fop.snapshots[k]) for k in sorted(fop.snapshots)]
            outs.append((body.clone(), float(scale), cam.clone(), snaps, fop.log))
            fop.close()
        finally:
            os.environ.pop("FDCAP_DEFER_STEP")
    a, b = outs
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2])
    for sa, sb in zip(a[3], b[3]):
        assert all(torch.equal(x, y) for x, y in zip(sa, sb))
    if log_every:
        import dataclasses
        la, lb = dataclasses.asdict(a[4]), dataclasses.asdict(b[4])
        assert len(la["iters"]) >= 30 // log_every and la["iters"][-1] == 29
        for k in la:                                                       # (NaN-safe: phase-1 rows carry no world term)
            np.testing.assert_array_equal(np.asarray(la[k], dtype=np.float64), np.asarray(lb[k], dtype=np.float64), err_msg=k)


@pytest.mark.parametrize("mode,log_every,extras", [("global", 0, False), ("global", 1, True), ("global", 7, True), ("local", 1, False)])
def test_the_loop_inside_the_library_gives_the_same_bits(mode, log_every, extras, tmp_path, capsys):
    """fdcap_opt_run (r4): the loop :560-593 as ONE C call per stretch of iterations -- the Python `for` (FDCAP_C_LOOP=0) issues the
    same entry points in the same order, so parameters, log, snapshots and checkpoints agree bit for bit.  extras: everything that
    cuts the loop into stretches at once -- snapshots, a finite check every 5 iterations, a checkpoint every 11, and a verbose fit
    long enough (120 iterations) for in-loop flushes of the loss history."""
    import dataclasses
    outs = []
    for flag in ("0", "1"):
        os.environ["FDCAP_C_LOOP"] = flag
        try:
            n = 23
            bm = synth.make_body_model(300, seed=92)
            vp = synth.make_vposer(seed=93)
            clip = synth.make_clip(n, seed=94)
            scene = synth.make_scene(5000, seed=95)
            left, right = synth.make_contact_ids(bm.v_template, per_part=16, seed=96)
            fop = FittingOP({"num_iter": 120 if extras else 30}, {}, n, body_model=bm, vposer=vp, scene_verts=scene,
                            contact_ids=np.concatenate([left, right]), camera_ext=read_camerapose(clip.camerapose_lines), n_left=len(left))
            kw = {}
            if extras:
                fop.verbose = True
                kw = dict(snapshot_at=[1, 50, 97, 120], check_finite_every=5, checkpoint_every=11, checkpoint_path=str(tmp_path / f"ck{flag}.npz"))
            body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), mode, log_every=log_every, **kw)
            printed = capsys.readouterr().out
            ck = dict(np.load(tmp_path / f"ck{flag}.npz")) if extras else {}
            outs.append((body.clone(), float(scale), cam.clone(), dataclasses.asdict(fop.log) if log_every else {},
                         {k: tuple(t.clone() for t in v) for k, v in fop.snapshots.items()}, ck, printed))
            fop.close()
        finally:
            os.environ.pop("FDCAP_C_LOOP")
    a, b = outs
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and torch.equal(a[2], b[2])
    assert a[3].keys() == b[3].keys()
    for k in a[3]:
        np.testing.assert_array_equal(np.asarray(a[3][k], dtype=np.float64), np.asarray(b[3][k], dtype=np.float64), err_msg=k)
    assert sorted(a[4]) == sorted(b[4]) == ([1, 50, 97, 120] if extras else [])
    for k in a[4]:
        assert all(torch.equal(x, y) for x, y in zip(a[4][k], b[4][k])), k
    assert a[5].keys() == b[5].keys()
    for k in a[5]:
        np.testing.assert_array_equal(a[5][k], b[5][k], err_msg=k)
    if extras:
        assert int(a[5]["next_iter"]) == 110                       # (the last checkpoint before the end)
        assert a[6] == b[6] and a[6].count("[INFO][fitting] iter=") == len(a[3]["iters"])


@pytest.mark.parametrize("n,per_part", [(48, 40), (5, 250)])
def test_vector_staged_skinning_backward_equals_the_scalar_kernel(n, per_part):
    """skin_bwd_vec_kernel (16-byte staging through LDS, packed per-vertex constants) evaluates the same terms in the same
    order as skin_bwd_small_kernel: whole fits agree bit for bit (80 and 500 contact vertices; the second is the bench's set)."""
    outs = []
    for flag in ("0", "1"):
        os.environ["FDCAP_SKIN_VEC"] = flag
        try:
            fop, bm, vp, clip, scene, vid = _make_fop(n, 1200, 20_000, per_part, 12, seed=71)
            body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), "global")
            outs.append((body.clone(), float(scale), cam.clone()))
            fop.close()
        finally:
            os.environ.pop("FDCAP_SKIN_VEC")
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])


@pytest.mark.parametrize("n,per_part", [(384, 250), (417, 40), (1000, 6)])
def test_fused_blend_and_skinning_launch_equals_the_two_launches(n, per_part):
    """blend_skin_fwd_kernel (clip-sized shares: the contact set's blend product and its skinning in one launch, the static operand's
    columns permuted so that x, y and z of a vertex meet in LDS) against panel_gemm3_rb2_kernel + skin_fwd_kernel
    (FDCAP_FUSE_SKIN=0): the same products in the same order per column and the same skinning expressions -- whole fits bit for
    bit, logs included (ragged frame counts, vertex sets that do not fill their last block of 64)."""
    outs = []
    for flag in ("0", "1"):
        os.environ["FDCAP_FUSE_SKIN"] = flag
        try:
            fop, bm, vp, clip, scene, vid = _make_fop(n, 1200, 20_000, per_part, 12, seed=73)
            body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=1)
            outs.append((body.clone(), float(scale), cam.clone(), np.array(fop.log.loss_contact)))
            fop.close()
        finally:
            os.environ.pop("FDCAP_FUSE_SKIN")
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
    assert np.array_equal(outs[0][3], outs[1][3]) and np.isfinite(outs[0][3]).all() and (outs[0][3] > 0).all()


@pytest.mark.parametrize("jmax,count", [(24, 256), (36, 500), (55, 300)])
def test_fused_contact_forward_with_wider_joint_ranges(jmax, count):
    """The fused launch stages the skinning transforms of joints < ja_hi for 32 frames in LDS (1.5 KB per joint): contact sets that reach
    24 and 36 joints still take it, one that reaches all 55 does not fit and takes the two launches -- either way the fit equals the
    two-launch form bit for bit."""
    n, V = 400, 3000
    bm = synth.make_body_model(V, seed=81)
    top = (bm.lbs_weights > 0).astype(np.int64) * np.arange(55)[None, :]
    vid = np.nonzero(top.max(axis=1) < jmax)[0]
    assert vid.size >= count and (top[vid].max() >= min(jmax, 55) - 8)
    vid = vid[np.linspace(0, vid.size - 1, count).astype(np.int64)]
    vp = synth.make_vposer(seed=82)
    clip = synth.make_clip(n, seed=83)
    scene = synth.make_scene(20_000, seed=84)
    outs = []
    for flag in ("0", "1"):
        os.environ["FDCAP_FUSE_SKIN"] = flag
        try:
            fop = FittingOP({"num_iter": 8}, {}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                            camera_ext=read_camerapose(clip.camerapose_lines))
            body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=1)
            outs.append((body.clone(), float(scale), cam.clone(), np.array(fop.log.loss_contact)))
            fop.close()
        finally:
            os.environ.pop("FDCAP_FUSE_SKIN")
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1] and torch.equal(outs[0][2], outs[1][2])
    assert np.array_equal(outs[0][3], outs[1][3]) and np.isfinite(outs[0][3]).all()


def test_no_contact_config_and_ragged_sizes():
    """BASELINE config 1 (8 frames, no scene: rec + temporal only) and awkward sizes."""
    for n, ns in ((8, 0), (3, 0), (17, 1100)):
        fop, bm, vp, clip, scene, vid = _make_fop(n, 200, ns, 7, 10, seed=20 + n)
        body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=1)
        orc = FittingOracle(SMPLXOracle(bm), VPoserDecoder.from_data(vp), scene, vid, clip.camerapose_lines, n, num_iter=10)
        ob, osc, ocam = orc.fitting(torch.tensor(clip.body_params))
        err = np.abs(body.cpu().numpy() - ob.numpy())
        assert np.quantile(err, 0.9) < 1e-4 and err.max() <= 0.1, (n, ns, err.max())
        assert abs(float(scale) - float(osc)) < 1e-3
        if ns == 0:
            assert float(scale) == pytest.approx(1.8)       # no gradient path -> never stepped
        fop.close()


@pytest.mark.parametrize("n", [1, 2, 63, 65, 1100])
def test_logged_sums_at_ragged_clip_lengths(n):
    """The printed loss terms (:573-575, :587-589) are per-frame partial sums reduced on the device, one wave per term, lane l
    taking frames l, l + 64, ... (csrc/fdc_loss.h loss_rows_reduce_block): clips shorter than a wave, one frame past it, and longer
    than one trip of its sixteen-load batch (1024 frames) against the oracle's means -- five logged iterations, the last one in
    phase 2, BASELINE config 1's loss (no scene).  N < 3 / N < 2: the smoothing means are means over nothing (nan), as in the
    reference."""
    fop, bm, vp, clip, scene, vid = _make_fop(n, 200, 0, 7, 5, seed=300 + n)
    fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=1)
    orc = FittingOracle(SMPLXOracle(bm), VPoserDecoder.from_data(vp), scene, vid, clip.camerapose_lines, n, num_iter=5)
    orc.fitting(torch.tensor(clip.body_params))
    want = np.array(orc.loss_log, dtype=np.float64)                     # [5, (l_rec, l_vp, l_sm, l_con, l_ws, total)]
    got = np.array([fop.log.l_rec, fop.log.l_vposer, fop.log.loss_smoothing, fop.log.loss_contact, fop.log.loss_world_smoothing,
                    fop.log.total], dtype=np.float64).T
    assert got.shape == want.shape == (5, 6) and fop.log.iters == [0, 1, 2, 3, 4] and first_phase2_iter(5) == 4
    for it in range(5):
        for c in (0, 1, 2, 4, 5):
            if np.isnan(want[it, c]):
                assert np.isnan(got[it, c]), (n, it, c, got[it, c])
            else:
                # iteration 0 to rounding; later ones within what one differently-rounded Adam step can move a mean
                np.testing.assert_allclose(got[it, c], want[it, c], rtol=2e-5 if it == 0 else 2e-3, atol=1e-7, err_msg=f"n={n} it={it} term={c}")
    fop.close()


def test_library_fails_loudly_without_gpu_fallback(small):
    _, _, ctx = small
    with pytest.raises(capi.FdcapError):
        ops.chamferDist(ctx)(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))    # host tensors are refused


def test_cli_file_interface_end_to_end(tmp_path):
    """body_gen/results/*/*.pkl + camerapose.txt + scene .ply + body_segments/*.json in,
    smoothed_body/body_gen_%06d.pkl out (global_optimization.py:658-714), synthetic assets injected."""
    import json
    import pickle
    from fdcap_amd import io
    n = 10
    fop, bm, vp, clip, scene, vid = _make_fop(n, 220, 900, 8, 6, seed=40)
    fop.close()
    root = tmp_path / "data"
    body_path = root / "sampleA" / "body_gen"
    io.write_body_gen(clip.body_params, str(body_path))
    (root / "sampleA" / "camerapose.txt").write_text("\n".join(clip.camerapose_lines) + "\n")
    io.write_ply_points(str(root / "sampleA" / "meshed-poisson.ply"), scene)
    seg = tmp_path / "body_segments"
    seg.mkdir()
    half = len(vid) // 2
    (seg / "L_Leg.json").write_text(json.dumps({"verts_ind": [int(v) for v in vid[:half]], "faces_ind": [0]}))
    (seg / "R_Leg.json").write_text(json.dumps({"verts_ind": [int(v) for v in vid[half:]], "faces_ind": [0]}))
    cfg = {"scene_verts_path": str(root / "sampleA" / "meshed-poisson.ply"),
           "camera_path": str(root / "sampleA" / "camerapose.txt"), "contact_id_folder": str(seg), "num_iter": 6}
    data = io.load_body_gen(str(body_path))
    f2 = FittingOP(cfg, {}, n, body_model=bm, vposer=vp)
    body, scale, cam = f2.fitting(torch.tensor(data).cuda(), "global")
    files = f2.save_result(body, scale, cam, str(tmp_path / "smoothed_body"))
    assert len(files) == n
    d = pickle.load(open(files[-1], "rb"))
    np.testing.assert_allclose(d["transl"], body[-1:, 0:3].cpu().numpy())
    np.testing.assert_allclose(d["camera_ext"], cam[-1].cpu().numpy())
    # same numbers as the array-injected path up to set() ordering of the contact ids (sum order)
    orc = FittingOracle(SMPLXOracle(bm), VPoserDecoder.from_data(vp), scene, f2.vid, clip.camerapose_lines, n, num_iter=6)
    ob, osc, _ = orc.fitting(torch.tensor(clip.body_params))
    assert np.quantile(np.abs(body.cpu().numpy() - ob.numpy()), 0.9) < 1e-4
    f2.close()


def test_all_vertices_as_contacts_penetration_stress_config():
    """BASELINE config 5 shape (every body vertex is a contact vertex, `weight_collision` has no
    reference implementation): nc > 1024 exercises the chunked skinning backward, 3*nc columns the
    wide pose-blend GEMM tiles.  Gradients vs the oracle's fp64 autograd, then a short trajectory."""
    n, V = 6, 1500
    bm = synth.make_body_model(V, seed=80)
    vp = synth.make_vposer(seed=81)
    clip = synth.make_clip(n, seed=82)
    scene = synth.make_scene(5000, seed=83)
    vid = np.arange(V, dtype=np.int64)
    fop = FittingOP({"num_iter": 500}, {}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                    camera_ext=read_camerapose(clip.camerapose_lines))
    dt = torch.float64
    f = FittingOracle(SMPLXOracle(bm, dt), VPoserDecoder.from_data(vp, dt), scene, vid, clip.camerapose_lines, n, dtype=dt)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(clip.body_params, dtype=dt)).detach()
    f.init(x78)
    idx1, _ = find_outliers(x78.numpy().astype(np.float32))
    l_rec, l_vp, l_con, l_sm, l_ws = f.cal_loss(x78, idx1)
    (0.1 * l_con + l_sm + l_rec).backward()
    fop.init(torch.tensor(x78.numpy(), dtype=torch.float32).cuda())
    lib, h = fop.ctx.lib, fop.ctx.handle
    capi.check(lib.fdcap_opt_backward(h, 0, 10 ** 6, 1, capi.current_stream()), "backward")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, capi.current_stream()), "grads")
    gx = f.body_rotation_rec.grad.numpy()
    # at x == x0 the L1 data term has sign(0) = 0 in both implementations
    np.testing.assert_allclose(dx.cpu().numpy(), gx, rtol=3e-3, atol=3e-4 * np.abs(gx).max())
    np.testing.assert_allclose(float(fop._dscale.cpu()), float(f.scale.grad), rtol=3e-3)
    s = fop._losses.cpu().numpy()
    np.testing.assert_allclose(0.1 * s[3] / (n * V), float(l_con.detach()), rtol=1e-5)
    fop.close()
    fop2 = FittingOP({"num_iter": 6}, {}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                     camera_ext=read_camerapose(clip.camerapose_lines))
    body, scale, cam = fop2.fitting(torch.tensor(clip.body_params).cuda(), "global")
    orc = FittingOracle(SMPLXOracle(bm), VPoserDecoder.from_data(vp), scene, vid, clip.camerapose_lines, n, num_iter=6)
    ob, osc, _ = orc.fitting(torch.tensor(clip.body_params))
    err = np.abs(body.cpu().numpy() - ob.numpy())
    assert np.quantile(err, 0.9) < 1e-4 and err.max() <= 0.06 and abs(float(scale) - float(osc)) < 1e-3
    fop2.close()


def test_full_size_body_model_and_wide_gemm():
    """V = 10475 (SMPL-X size): the full-mesh operator runs the [B,486] x [486,31425] pose-blend GEMM
    on the 128x128-tile MFMA kernel; compared with the oracle on a few frames."""
    bm = synth.make_body_model(10475, seed=0)
    vp = synth.make_vposer(seed=1)
    ctx = capi.Context(bm, vp)
    clip = synth.make_clip(140, seed=4)        # M*N large enough for the 128x128 tiles
    p = torch.tensor(clip.body_params)
    verts, joints = ops.body_forward_from_params(ctx, p.cuda())
    sel = [0, 57, 139]
    aa = VPoserDecoder.from_data(vp).decode(p[sel, 16:48], output_type="aa").view(len(sel), -1)
    want = SMPLXOracle(bm)(return_verts=True, body_pose=aa, transl=p[sel, 0:3], global_orient=p[sel, 3:6],
                           betas=p[sel, 6:16], left_hand_pose=p[sel, 48:60], right_hand_pose=p[sel, 60:72])
    np.testing.assert_allclose(verts[sel].cpu().numpy(), want.vertices.numpy(), atol=5e-5)
    np.testing.assert_allclose(joints[sel].cpu().numpy(), want.joints.numpy(), atol=5e-5)
    assert bool(torch.isfinite(verts).all())
    ctx.close()


def test_local_mode_matches_reference_golden(golden_dir):
    """mode='local' (:499-556) on the GPU vs the reference's own run: first loop (0.2*contact, no world
    term, camera_ext never stepped), detect_contact (== 0.5), then the cal_loss2 loop with the
    vertex-space smoothing over ALL mesh vertices (full pose-blend GEMM forward + backward) and the
    foot-skate term."""
    g = np.load(os.path.join(golden_dir, "ref_local_10it.npz"))
    bm = synth.make_body_model(int(g["num_verts"]), seed=int(g["model_seed"]))
    vp = synth.make_vposer(seed=int(g["vposer_seed"]))
    num_iter = int(g["num_iter"])
    cam0 = read_camerapose(list(g["camerapose"]))
    fop = FittingOP({"num_iter": num_iter}, {}, 300, body_model=bm, vposer=vp, scene_verts=g["scene"], contact_ids=g["vid"],
                    camera_ext=cam0, n_left=int(g["n_left"]))
    body, scale, cam = fop.fitting(torch.tensor(g["body_in"]).cuda(), "local", log_every=1)
    assert bool((fop.contact_weight == 0.5).all())
    err = np.abs(body.cpu().numpy() - g["body_rec"])
    q50, q90, q99 = np.quantile(err, [0.5, 0.9, 0.99])
    assert err.max() <= 2 * 0.005 * 14 and q50 < 1e-6 and q90 < 1e-4 and q99 < 3e-3, (q50, q90, q99, err.max())
    np.testing.assert_allclose(float(scale), float(g["scale"]), atol=1e-4)
    np.testing.assert_array_equal(cam.cpu().numpy(), cam0)                 # camera_ext is never stepped in this mode
    ref2 = g["log2"]
    log2 = np.array(fop.log2)
    tol = 3e-6 + 2e-6 * (num_iter + np.arange(len(ref2)))
    for k in range(1, 6):
        assert np.all(np.abs(log2[:, k] - ref2[:, k]) <= 2 * tol), (k, np.abs(log2[:, k] - ref2[:, k]).max())
    fop.close()


def test_local_mode_checkpoint_resume_is_bit_identical(tmp_path):
    """Mode 'local' (r5): 20 iterations of the first loop + 8 of the second; checkpoints every 6 iterations of the whole fit.  New
    optimisers resumed from iteration 16 (first loop, at its phase switch) and from iteration 24 (inside the second loop: detect_contact's weights come
    from the file) end on the uninterrupted fit's bits."""
    n = 24
    fop, bm, vp, clip, scene, vid = _make_fop(n, 200, 1500, 10, 20, seed=70)
    body = torch.tensor(clip.body_params).cuda()
    a = fop.fitting(body, "local", log_every=1)
    a = (a[0].clone(), float(a[1]), np.array(fop.log2))
    fop.close()
    for stop, every in ((16, 16), (24, 6)):
        ck = str(tmp_path / f"l{stop}.npz")
        f1, *_ = _make_fop(n, 200, 1500, 10, 20, seed=70)
        b = f1.fitting(body, "local", checkpoint_every=every, checkpoint_path=ck, check_finite_every=5)
        assert torch.equal(a[0], b[0]) and a[1] == float(b[1])
        f1.close()
        last = int(np.load(ck)["next_iter"])
        assert last == stop and str(np.load(ck)["mode"]) == "local"
        f2, *_ = _make_fop(n, 200, 1500, 10, 20, seed=70)
        c = f2.fitting(body, "local", log_every=1, resume=ck)
        assert torch.equal(a[0], c[0]) and a[1] == float(c[1]), stop
        np.testing.assert_array_equal(np.array(f2.log2), a[2][max(stop - 20, 0):])
        f2.close()


def test_local_mode_second_loop_gradient_matches_autograd():
    """The whole-matrix bar with all four terms mixed; the tight check, per column block, is tests/test_gpu_local2_bars.py."""
    n = 10
    fop, bm, vp, clip, scene, vid = _make_fop(n, 260, 700, 12, 500, seed=90)
    dt = torch.float64
    f = FittingOracle(SMPLXOracle(bm, dt), VPoserDecoder.from_data(vp, dt), scene, vid, clip.camerapose_lines, n, dtype=dt)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(clip.body_params, dtype=dt)).detach()
    f.init(x78)
    g = torch.Generator().manual_seed(6)
    pert = 0.01 * torch.randn(f.body_rotation_rec.shape, generator=g, dtype=dt)
    f.body_rotation_rec.data += pert
    idx1, _ = find_outliers(x78.numpy().astype(np.float32))
    w = torch.full((n,), 0.5, dtype=dt)
    w[3] = 0.8            # exercise the thresholding of (:421-422): left weight 0.2 -> 0, right 0.8
    w[6] = 0.3
    n_left = len(vid) // 2
    l_rec, l_loc, l_sm, l_cs = f.cal_loss2(x78, idx1, w, n_left)
    (l_sm + l_loc + l_rec + l_cs).backward()
    fop._mode = "local"
    fop.init(torch.tensor(x78.numpy(), dtype=torch.float32).cuda())
    fop._rows_x[2:2 + n] += pert.float().cuda()
    lib, h = fop.ctx.lib, fop.ctx.handle
    capi.check(lib.fdcap_opt_backward_local2(h, capi.dptr(w.float().cuda()), n_left, capi.current_stream()), "local2")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, capi.current_stream()), "grads")
    gx = f.body_rotation_rec.grad.numpy()
    np.testing.assert_allclose(dx.cpu().numpy(), gx, rtol=3e-3, atol=3e-4 * np.abs(gx).max())
    s = fop._losses.cpu().numpy()
    np.testing.assert_allclose(s[5] / ((n - 2) * 3 * 260), float(l_sm.detach()), rtol=1e-5)
    np.testing.assert_allclose(s[6], float(l_cs.detach()), rtol=1e-5)
    np.testing.assert_allclose(s[2] / ((n - 2) * 78), float(l_loc.detach()), rtol=1e-5)
    fop.close()


def test_world_mesh_export_matches_viewer_math(tmp_path):
    """smoothed_body pickles -> world-space mesh exactly as global_vis.py:116-152 composes it."""
    from fdcap_amd import io
    n = 7
    fop, bm, vp, clip, scene, vid = _make_fop(n, 240, 600, 8, 4, seed=95)
    body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), "global")
    fop.save_result(body, scale, cam, str(tmp_path / "smoothed_body"))
    rows, sc, cams = io.load_smoothed_body(str(tmp_path / "smoothed_body"))
    got = ops.world_mesh(fop.ctx, torch.tensor(rows).cuda(), sc, torch.tensor(cams).cuda(), shape_from_first=True)
    p = torch.tensor(rows)
    p[:, 6:16] = p[0:1, 6:16]
    aa = VPoserDecoder.from_data(vp).decode(p[:, 16:48], output_type="aa").view(n, -1)
    out = SMPLXOracle(bm)(return_verts=True, body_pose=aa, transl=p[:, 0:3], global_orient=p[:, 3:6], betas=p[:, 6:16],
                          left_hand_pose=p[:, 48:60], right_hand_pose=p[:, 60:72])
    want = []
    for i in range(n):                                   # the viewer's per-frame numpy arithmetic
        camera_pose = np.eye(4)
        camera_pose[:3, 3] = rows[i, 72:75] * sc
        body_trans = cams[i].astype(np.float64) @ camera_pose
        v = out.vertices[i].numpy().astype(np.float64) * sc
        want.append((np.c_[v, np.ones(len(v))] @ body_trans.T)[:, :3])
    np.testing.assert_allclose(got.cpu().numpy(), np.stack(want), atol=5e-5)
    fop.close()


def test_checkpoint_resume_is_bit_identical_and_finite_check_fires(tmp_path):
    """SURVEY §5 items the reference lacks: a fit interrupted after 7 of 12 iterations and resumed by a NEW optimiser from the
    checkpoint file ends on the uninterrupted run's bits (the phase switch at iteration 10 lies after the resume point, the
    Chamfer search's seeds / kept lists are rebuilt -- pruning state only); the opt-in finite check raises on NaN input."""
    n = 40
    ck = str(tmp_path / "fit.ckpt.npz")
    fop, bm, vp, clip, scene, vid = _make_fop(n, 300, 3000, 20, 12)
    body = torch.tensor(clip.body_params).cuda()
    a = fop.fitting(body, "global", log_every=1, checkpoint_every=7, checkpoint_path=ck, check_finite_every=3)
    full_log = np.array(fop.log.total)
    a = (a[0].clone(), float(a[1]), a[2].clone())
    fop.close()
    fop2, *_ = _make_fop(n, 300, 3000, 20, 12)
    b = fop2.fitting(body, "global", log_every=1, resume=ck)
    assert fop2.log.iters == list(range(7, 12))
    assert torch.equal(a[0], b[0]) and a[1] == float(b[1]) and torch.equal(a[2], b[2])
    np.testing.assert_array_equal(np.array(fop2.log.total), full_log[7:])
    fop2.close()
    fop3, *_ = _make_fop(n, 300, 3000, 20, 12)
    bad = clip.body_params.copy()
    bad[5, 20] = np.nan
    with pytest.raises(capi.FdcapError, match="non-finite"):
        fop3.fitting(torch.tensor(bad).cuda(), "global", check_finite_every=2)
    fop3.close()
    fop4, *_ = _make_fop(n, 300, 3000, 20, 10)
    with pytest.raises(capi.FdcapError, match="another clip"):
        fop4.fitting(body, "global", resume=ck)              # written for a 12-iteration budget
    fop4.close()


def test_every_streaming_kernel_variant_gives_the_same_bits(tmp_path):
    """FDCAP_NN_STREAM selects the instantiation of the in-loop Chamfer kernel (waves per query group; read once per process):
    11 / 21 / 41 and the staged kernel (0) against the default choice, after a few
    optimiser iterations (seeds, kept lists, queued candidates all in play): distances and indices bit for bit.  The one-wave
    variant (11) also runs with its launch order off and re-sorted after every launch (FDCAP_NN_ORDER): the order decides when
    a query group runs, never what it returns."""
    import subprocess
    import sys
    code = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
import fdcap_amd
from fdcap_amd import capi
from tests.test_gpu_parity import _make_fop
n = 96
fop, bm, vp, clip, scene, vid = _make_fop(n, 300, 60_000, 40, 8, seed=60)
x78 = torch.empty(n, 78, device="cuda")
lib, h = fop.ctx.lib, fop.ctx.handle
capi.check(lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(clip.body_params).cuda()), n, capi.dptr(x78), capi.current_stream()), "75->78")
fop.init(x78)
for ii in range(4):
    capi.check(lib.fdcap_opt_backward(h, ii, 400, 0, capi.current_stream()), "backward")
    capi.check(lib.fdcap_opt_step(h, ii, 400, capi.current_stream()), "step")
d = torch.empty(n, len(vid), device="cuda"); i = torch.empty(n, len(vid), device="cuda", dtype=torch.int32)
capi.check(lib.fdcap_opt_forward_world(h, capi.dptr(torch.empty(n, len(vid), 3, device="cuda")), None, capi.current_stream()), "fw")
capi.check(lib.fdcap_opt_get_contact(h, capi.dptr(d), capi.dptr(i), capi.current_stream()), "gc")
torch.cuda.synchronize()
np.savez(sys.argv[1], d=d.cpu().numpy(), i=i.cpu().numpy(), x=fop._rows_x.cpu().numpy())
''' % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for mode in ("", "11", "11/0", "11/1", "21", "41", "0"):
        out = str(tmp_path / ("nn_%s.npz" % (mode.replace("/", "_") or "default")))
        env = dict(os.environ)
        env.pop("FDCAP_NN_STREAM", None)
        env.pop("FDCAP_NN_ORDER", None)
        if mode:
            env["FDCAP_NN_STREAM"] = mode.split("/")[0]
        if "/" in mode:
            env["FDCAP_NN_ORDER"] = mode.split("/")[1]
        subprocess.run([sys.executable, "-c", code, out], check=True, env=env, timeout=300)
        res[mode] = np.load(out)
    ref = res[""]
    assert np.isfinite(ref["d"]).all() and (ref["i"] >= 0).all()
    for mode, r in res.items():
        assert np.array_equal(r["d"], ref["d"]) and np.array_equal(r["i"], ref["i"]) and np.array_equal(r["x"], ref["x"]), mode


def test_roctx_ranges_are_bound_on_request_and_change_nothing(tmp_path):
    """FDCAP_ROCTX=1 makes the library bracket the blend products, the Chamfer search, the
    optimiser step and every backward with roctx ranges (csrc/fdc_trace.h; the marker library is bound at run time).  Without
    a profiler attached the ranges go nowhere: a child process runs a short fit with the switch on and must report the
    marker library loaded (/proc/self/maps) and the same parameters, bit for bit, as this process without it."""
    import subprocess
    import sys
    fop, bm, vp, clip, scene, vid = _make_fop(9, 300, 2000, 20, 12, seed=91)
    body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=2)
    ref = body.cpu().numpy()
    fop.close()
    out = tmp_path / "roctx.npy"
    code = f"""
import numpy as np, torch, sys
sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})
import fdcap_amd
from tests.test_gpu_parity import _make_fop
fop, bm, vp, clip, scene, vid = _make_fop(9, 300, 2000, 20, 12, seed=91)
body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=2)
np.save({str(out)!r}, body.cpu().numpy())
maps = open("/proc/self/maps").read()
print("ROCTX_BOUND", int("roctx" in maps))
"""
    env = dict(os.environ, FDCAP_ROCTX="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ROCTX_BOUND 1" in r.stdout, r.stdout[-500:]
    np.testing.assert_array_equal(np.load(out), ref)


def test_the_library_side_loop_refuses_what_it_cannot_run():
    """fdcap_opt_run's argument checks (include/fdcap.h): a range outside the fit, a logging iteration without a history (or with a
    history too short), the exchange tail without a communicator -- error codes, no launches, and the context still fits afterwards."""
    import ctypes
    fop, bm, vp, clip, scene, vid = _make_fop(9, 300, 2000, 20, 10, seed=97)
    body = torch.tensor(clip.body_params).cuda()
    ref = fop.fitting(body, "global")[0].clone()
    lib, h, st = fop.ctx.lib, fop.ctx.handle, capi.current_stream()
    n = ctypes.c_int32(-1)
    hist = torch.zeros(2, capi.NUM_LOSSES, dtype=torch.float64, device="cuda")
    E_ARG, E_STATE = -1, -2
    assert lib.fdcap_opt_run(h, 0, 11, 10, 8, 0, None, 0, 0, ctypes.byref(n), st) == E_ARG and n.value == 0       # ii1 > num_iter
    assert lib.fdcap_opt_run(h, 5, 3, 10, 8, 0, None, 0, 0, ctypes.byref(n), st) == E_ARG                          # ii1 < ii0
    assert lib.fdcap_opt_run(h, 0, 2, 10, 8, 1, None, 0, 0, ctypes.byref(n), st) == E_ARG and n.value == 0        # logging, no history
    assert lib.fdcap_opt_run(h, 0, 1, 10, 8, 0, None, 0, 2, ctypes.byref(n), st) == E_STATE                        # exchange tail, no communicator
    # a history of two rows takes two logged iterations, the third is refused (and says how many it wrote)
    assert lib.fdcap_opt_run(h, 0, 3, 10, 8, 1, capi.dptr(hist), 2, 0, ctypes.byref(n), st) == E_ARG and n.value == 2
    assert lib.fdcap_opt_run(h, 4, 4, 10, 8, 0, None, 0, 0, ctypes.byref(n), st) == 0 and n.value == 0             # an empty stretch is fine
    again = fop.fitting(body, "global")[0]
    assert torch.equal(again, ref)
    fop.close()
