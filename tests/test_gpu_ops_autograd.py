"""The three drop-in operators as torch.autograd.Functions over the C-ABI's forward / backward pairs (ops.py):
each backward against the oracle's fp64 autograd, and a REFERENCE-SHAPED loop -- the reference's own cal_loss
(/root/reference/global_optimization.py:249-312), its flag toggling (:563-568, :577-580), loss.backward() (:591) and
torch.optim.Adam (:188, :592) written out in torch, with only the three third-party operator calls replaced by ops.VPoser /
ops.BodyModel / ops.chamferDist -- against the reference's own 5-iteration run (tests/golden/ref_global_5it.npz)."""
import os

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, ops, synth
from fdcap_amd.io import read_camerapose
from oracle import rotrepr
from oracle.fitting import find_outliers_and_sources, verts_transform
from oracle.smplx import SMPLXOracle
from oracle.vposer import VPoserDecoder
from tests import gradient_bars

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    bm = synth.make_body_model(300, seed=0)
    vp = synth.make_vposer(seed=1)
    ctx = capi.Context(bm, vp)
    yield bm, vp, ctx
    ctx.close()


def _close(got, want, want32, name=""):
    """An operator's gradient of one input tensor against the oracle's fp64 autograd.  The bar of tests/gradient_bars.py, per
    tensor: 32 x max(max|fp32 oracle - fp64 oracle|, 2^-24 max|g|), absolute, no rtol -- from the oracle's own two precisions at
    the same fp32-rounded inputs.  Every element is held to the smaller of that and the older bar (rtol 2e-3, atol 2e-4 max|g|):
    the new one is below the old atol alone for every tensor of these cases but the hand poses of the joints-only one
    (tests/test_gradient_bars_cpu.py), so nowhere else has the old rtol anything left to do."""
    want, err = np.asarray(want, dtype=np.float64), np.abs(np.asarray(got, dtype=np.float64) - want)
    gmax = np.abs(want).max()
    new = gradient_bars.M * max(np.abs(np.asarray(want32, dtype=np.float64) - want).max(), gradient_bars.EPS32 * gmax)
    old = 2e-4 * gmax + 2e-3 * np.abs(want)
    print(f"{name or 'gradient'}: max|err| / bar {err.max() / new if new else float(err.max() > 0):.3g}, bar {new:.3g} = {new / gmax if gmax else 0:.2g} max|g|")
    assert (err <= np.minimum(old, new)).all(), (name, err.max(), new, gmax)


def _f32(a):
    """rounded to fp32 (what the device is given), held in fp64"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _vposer_oracle(vp, B, output_type):
    """-> z, w (fp32 values), the fp64 oracle's output, d (out . w) / dz from the fp64 and from the fp32 oracle"""
    rng = np.random.default_rng(B)
    z = _f32(rng.standard_normal((B, 32)))
    w = _f32(rng.standard_normal((B, 21 * (3 if output_type == "aa" else 9))))
    res = []
    for dt in (torch.float64, torch.float32):
        zt = torch.tensor(z, dtype=dt, requires_grad=True)
        out = VPoserDecoder.from_data(vp, dt).decode(zt, output_type=output_type).reshape(B, -1)
        (out * torch.tensor(w, dtype=dt)).sum().backward()
        res.append((out.detach().numpy(), zt.grad.numpy()))
    return z, w, res[0][0], res[0][1], res[1][1]


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("output_type", ["aa", "matrot"])
def test_vposer_decode_backward_matches_autograd(small, B, output_type):
    bm, vp, ctx = small
    z, w, out, g64, g32 = _vposer_oracle(vp, B, output_type)
    zg = torch.tensor(z, dtype=torch.float32).cuda().requires_grad_(True)
    got = ops.VPoser(ctx).decode(zg, output_type=output_type).reshape(B, -1)
    np.testing.assert_allclose(got.detach().cpu().numpy(), out, atol=5e-5)
    (got * torch.tensor(w, dtype=torch.float32).cuda()).sum().backward()
    _close(zg.grad.cpu().numpy(), g64, g32, f"d latent ({output_type}, B = {B})")


def _body_model_oracle(bm, B, use_verts, use_joints):
    """-> inputs, vertex and joint weights (fp32 values), the fp64 oracle's vertices, {input: gradient} from the fp64 and from the
    fp32 oracle"""
    V = bm.v_template.shape[0]
    rng = np.random.default_rng(B)
    inp = {"global_orient": rng.standard_normal((B, 3)) * 0.8, "body_pose": rng.standard_normal((B, 63)) * 0.4,
           "betas": rng.standard_normal((B, 10)) * 0.5, "left_hand_pose": rng.standard_normal((B, 12)) * 0.3,
           "right_hand_pose": rng.standard_normal((B, 12)) * 0.3, "transl": rng.standard_normal((B, 3))}
    inp = {k: _f32(v) for k, v in inp.items()}
    wv, wj = _f32(rng.standard_normal((B, V, 3))), _f32(rng.standard_normal((B, 55, 3)))
    res = []
    for dt in (torch.float64, torch.float32):
        t = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in inp.items()}
        out = SMPLXOracle(bm, dt)(return_verts=True, **t)
        loss = 0
        if use_verts:
            loss = loss + (out.vertices * torch.tensor(wv, dtype=dt)).sum()
        if use_joints:
            loss = loss + (out.joints[:, :55] * torch.tensor(wj, dtype=dt)).sum()
        loss.backward()
        res.append((out.vertices.detach().numpy(), {k: v.grad.numpy() for k, v in t.items()}))
    return inp, wv, wj, res[0][0], res[0][1], res[1][1]


def _body_model_case(bm, ctx, B, use_verts, use_joints):
    inp, wv, wj, verts, g64, g32 = _body_model_oracle(bm, B, use_verts, use_joints)
    g = {k: torch.tensor(v, dtype=torch.float32).cuda().requires_grad_(True) for k, v in inp.items()}
    got = ops.BodyModel(ctx)(return_verts=True, **g)
    lg = 0
    if use_verts:
        lg = lg + (got.vertices * torch.tensor(wv, dtype=torch.float32).cuda()).sum()
    if use_joints:
        lg = lg + (got.joints * torch.tensor(wj, dtype=torch.float32).cuda()).sum()
    lg.backward()
    np.testing.assert_allclose(got.vertices.detach().cpu().numpy(), verts, atol=3e-5)
    for k in inp:
        _close(g[k].grad.cpu().numpy(), g64[k], g32[k], f"d {k} (V = {bm.v_template.shape[0]}, B = {B})")


@pytest.mark.parametrize("B,use_verts,use_joints", [(3, True, True), (40, True, False), (5, False, True)])
def test_body_model_backward_matches_autograd(small, B, use_verts, use_joints):
    bm, vp, ctx = small
    _body_model_case(bm, ctx, B, use_verts, use_joints)


# Exact-fp32 products (FDCAP_GEMM_SPLIT3=0) on a mesh of more than 2048 vertices: the blend product's data gradient has K = 3 V >
# 6144 columns, no fp32 panel of its operand is kept, and gemm_f32_nt (csrc/fdc_gemm.h) serves it -- one of four kernels by row count
# (16x16 tiles while 16 ceil(B / 32) < 256, i.e. up to 480 rows) and operand alignment (3 V a multiple of 4: float4 staging).  The
# smallest shapes that select each; K is ragged against the 128- / 256-deep slabs in all of them, B = 5 leaves a partial 16-row tile
# and B = 481 a 32-row tile that holds one row.
EXACT_BIG_K_CASES = {(2052, 5): "gemm_f32_mfma_ksplit16_v4_kernel", (2051, 5): "gemm_f32_mfma_ksplit16_kernel",
                     (2052, 481): "gemm_f32_mfma_ksplit_v4_kernel", (2051, 481): "gemm_f32_mfma_ksplit_kernel"}
_EXACT_BIG_K_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, %r)
import fdcap_amd
from fdcap_amd import capi, synth
from tests.test_gpu_ops_autograd import EXACT_BIG_K_CASES, _body_model_case
res = {}
buf = ctypes.create_string_buffer(4096)
for V, B in EXACT_BIG_K_CASES:
    bm = synth.make_body_model(V, seed=0)
    ctx = capi.Context(bm, synth.make_vposer(seed=1))
    ctx.lib.fdcap_debug_kernel_forms(buf, 4096, 1)             # (reset)
    err = None
    try:
        _body_model_case(bm, ctx, B, True, False)
    except AssertionError as e:
        err = str(e)[-1500:]
    ctx.lib.fdcap_debug_kernel_forms(buf, 4096, 0)
    res["%%d-%%d" %% (V, B)] = {"forms": buf.value.decode(), "error": err}
    ctx.close()
print("RESULT " + json.dumps(res))
"""


@pytest.fixture(scope="module")
def exact_big_k():
    """All four cases in ONE child process (the switch is read once per process); each test below asserts its own case."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", _EXACT_BIG_K_CHILD % root], env=dict(os.environ, FDCAP_GEMM_SPLIT3="0"), capture_output=True,
                       text=True, timeout=600, cwd=root)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    assert p.returncode == 0 and line, p.stderr[-2000:]
    return json.loads(line[-1][7:])


@pytest.mark.parametrize("V,B", list(EXACT_BIG_K_CASES))
def test_body_model_backward_matches_autograd_on_exact_fp32_beyond_the_panels(exact_big_k, V, B):
    """test_body_model_backward_matches_autograd's body and bars (the oracle's fp64 autograd, _close) where the data gradient of the
    blend product leaves the panels: each case must have run the kernel of gemm_f32_nt it was sized for."""
    r = exact_big_k["%d-%d" % (V, B)]
    print(V, B, r["forms"])
    assert EXACT_BIG_K_CASES[(V, B)] in r["forms"].split(";"), r["forms"]
    assert not [f for f in r["forms"].split(";") if f.startswith("gemm_f32_") and f != EXACT_BIG_K_CASES[(V, B)]], r["forms"]
    assert r["error"] is None, r["error"]


class ReferenceShapedFitting:
    """FittingOP as /root/reference/global_optimization.py writes it (:142-188, :191-206, :249-312, :450-489, :558-593),
    on the GPU, with the three third-party operators bound to ops.* (HIP kernels through autograd.Functions)."""

    def __init__(self, ctx, scene, vid, camera_ext, n, num_iter, lr=0.005):
        dev = "cuda"
        self.vposer = ops.VPoser(ctx)
        self.body_mesh_model = ops.BodyModel(ctx)
        self.chamfer = ops.chamferDist(ctx, both=True)                                       # ext.chamferDist() (:292)
        self.s_verts_batch = torch.tensor(scene, device=dev).unsqueeze(0).expand(n, -1, -1)  # (:175-176: repeat; same values)
        self.vid = torch.tensor(np.asarray(vid), device=dev, dtype=torch.long)
        self.batch_size = self.num_body = n
        self.num_iter = num_iter
        self.weight_loss_rec, self.weight_loss_vposer, self.weight_contact = 1.0, 0.001, 0.1
        self.scale = torch.tensor(1.8, device=dev, requires_grad=True)                       # :179
        self.body_rotation_rec = torch.zeros(n, 78, device=dev, requires_grad=True)          # :180 (+ .data replaced, :454)
        self.camera_ext = torch.zeros(n, 4, 4, device=dev, requires_grad=True)               # :182
        self._cam0 = torch.tensor(camera_ext, device=dev)
        self.optimizer = torch.optim.Adam([self.body_rotation_rec, self.scale, self.camera_ext], lr=lr)   # :188
        self.log = []

    def body2world(self):                                                                    # :191-206, vectorised
        n = self.num_body
        pose = torch.eye(4, device="cuda").unsqueeze(0).repeat(n, 1, 1)
        cam_t = self.body_rotation_rec[:, -3:] * self.scale
        pose = torch.cat([pose[:, :, :3], torch.cat([cam_t, torch.ones(n, 1, device="cuda")], 1).unsqueeze(-1)], 2)
        return torch.matmul(self.camera_ext, pose)

    def cal_loss(self, body_data_rotation, idx1):                                            # :249-312
        body2world = self.body2world()
        weights = torch.ones_like(body_data_rotation)
        weights[idx1, :] = 0.0
        loss_rec = self.weight_loss_rec * torch.mean(torch.abs(body_data_rotation - self.body_rotation_rec) * weights)
        body_rec = rotrepr.convert_to_3D_rot(self.body_rotation_rec)                         # :261
        loss_vposer = self.weight_loss_vposer * torch.mean(body_rec[:, 16:48] ** 2)
        diff = self.body_rotation_rec[0:-1, :] - self.body_rotation_rec[1:, :]
        loss_smoothing = torch.mean(torch.abs(diff[0:-1, :] - diff[1:, :]))
        joint_rot = self.vposer.decode(body_rec[:, 16:48], output_type="aa").view(self.batch_size, -1)      # :270-271
        out = self.body_mesh_model(return_verts=True, body_pose=joint_rot, transl=body_rec[:, 0:3],
                                   global_orient=body_rec[:, 3:6], betas=body_rec[:, 6:16],
                                   left_hand_pose=body_rec[:, 48:60], right_hand_pose=body_rec[:, 60:72])    # :280-283
        verts = verts_transform(out.vertices * self.scale, body2world)                        # :284-285
        contact = verts[:, self.vid, :]                                                       # :290
        dist1, _ = self.chamfer(contact.contiguous(), self.s_verts_batch)                     # :292-294
        r = torch.sqrt(dist1 + 1e-4)
        loss_contact = self.weight_contact * torch.mean(r / (r + 1.0))                        # :295
        joints = verts_transform(out.joints[:, 0:23, :], body2world)                          # :298-299
        loss_world_smoothing = torch.mean(torch.abs(joints[0:-1] - joints[1:]))               # :304
        return loss_rec, loss_vposer, loss_contact, loss_smoothing, loss_world_smoothing

    def fitting(self, body_data):
        x78 = rotrepr.convert_to_6D_rot(torch.tensor(body_data)).cuda()                       # :493
        self.body_rotation_rec.data = x78.clone()                                             # init(), :454-455
        self.camera_ext.data = self._cam0.clone()
        idx1, pos = find_outliers_and_sources(x78.cpu())
        if len(idx1) and len(pos):
            self.body_rotation_rec.data[idx1, :] = x78[pos, :]
        x78 = x78.detach()
        for ii in range(self.num_iter):                                                       # :560-593
            self.optimizer.zero_grad()
            l_rec, l_vp, l_con, l_sm, l_ws = self.cal_loss(x78, idx1)
            if ii < self.num_iter * 0.8:
                self.camera_ext.requires_grad = False
                self.scale.requires_grad = True
                self.body_rotation_rec.requires_grad = True
                loss = l_con * 0.1 + l_sm * 1.0 + l_rec
            else:
                self.camera_ext.requires_grad = True
                self.scale.requires_grad = False
                self.body_rotation_rec.requires_grad = True
                loss = l_rec + l_ws * 1 + l_sm * 0.5
            self.log.append([float(v.detach()) for v in (l_rec, l_vp, l_sm, l_con, l_ws, loss)])
            loss.backward()
            self.optimizer.step()
        return rotrepr.convert_to_3D_rot(self.body_rotation_rec).detach(), float(self.scale), self.camera_ext.detach(), idx1


def test_reference_shaped_loop_lands_on_the_reference_run(golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_global_5it.npz"))
    bm = synth.make_body_model(int(g["num_verts"]), seed=int(g["model_seed"]))
    vp = synth.make_vposer(seed=int(g["vposer_seed"]))
    ctx = capi.Context(bm, vp)
    num_iter = int(g["num_iter"])
    f = ReferenceShapedFitting(ctx, g["scene"], g["vid"], read_camerapose(list(g["camerapose"])).reshape(-1, 4, 4), 300, num_iter)
    body, scale, cam, idx1 = f.fitting(g["body_in"])
    np.testing.assert_array_equal(idx1, g["idx1"])
    err = np.abs(body.cpu().numpy() - g["body_rec"])
    q50, q90, q99 = np.quantile(err, [0.5, 0.9, 0.99])
    print("reference-shaped loop vs the reference run: max", err.max(), "q50/q90/q99", q50, q90, q99)
    # the bars of test_trajectory_matches_reference_golden (Adam + L1 kinks: tests/test_host_math.py)
    assert err.max() <= 6 * 0.005          # (three sign flips of one entry at most; 2 lr num_iter would hold for any Adam run)
    assert q50 < 1e-6 and q90 < 1e-4 and q99 < 3e-3, (q50, q90, q99)
    assert err[:, 48:72].max() <= 2e-6                                    # kink-free columns (hands)
    assert (err <= 2e-5).mean() > 0.995                                   # (measured 0.9977: a few L1 sign flips, +-lr each)
    np.testing.assert_allclose(scale, float(g["scale"]), atol=1e-4)
    np.testing.assert_allclose(cam.cpu().numpy(), g["camera_ext"], atol=1e-6)           # (never stepped within 5 iterations)
    log = np.array(f.log)
    tol = 3e-6 + 2e-6 * np.arange(num_iter)
    for col, gcol in ((0, 1), (1, 2), (2, 3), (3, 4)):                  # rec, vposer, smoothing, contact
        assert np.all(np.abs(log[:, col] - g["log"][:, gcol]) <= tol), (col, np.abs(log[:, col] - g["log"][:, gcol]).max())
    assert np.all(np.abs(log[:, 5] - g["log"][:, 6]) <= 2 * tol)
    ctx.close()


def test_operators_accept_inputs_without_grad_and_propagate_none(small):
    """No silent detaching: outputs of grad-requiring inputs carry a grad_fn; inputs that need no gradient get none."""
    bm, vp, ctx = small
    z = torch.randn(4, 32, device="cuda", requires_grad=True)
    aa = ops.VPoser(ctx).decode(z, "aa")
    assert aa.requires_grad and aa.grad_fn is not None
    betas = torch.zeros(4, 10, device="cuda", requires_grad=True)
    out = ops.BodyModel(ctx)(return_verts=True, body_pose=aa.view(4, -1), betas=betas, transl=torch.zeros(4, 3, device="cuda"))
    assert out.vertices.requires_grad and out.joints.requires_grad
    out.joints.sum().backward()
    assert z.grad is not None and betas.grad is not None and float(z.grad.abs().max()) > 0
    with torch.no_grad():
        out2 = ops.BodyModel(ctx)(return_verts=False, body_pose=aa.view(4, -1))
    assert out2.vertices is None and not out2.joints.requires_grad


@pytest.mark.parametrize("B,n,ns", [(64, 200, 120_000), (3, 17, 5000), (256, 500, 100_000)])
def test_chamfer_operator_takes_the_culled_search_for_the_registered_scene(B, n, ns):
    """VERDICT r4 (next 6): ops.chamferDist with the registered scene as xyz2 goes through the optimiser loop's search
    (fdcap_chamfer_fwd_scene: k-d-sorted scene, cell boxes, the previous call's neighbours as seeds, kept work lists) -- and
    returns what the every-pair scan of a foreign target returns, values and indices, bit for bit, call after call while the
    queries move (millimetres, then a jump of 30 cm, then a change of shape); the gradient is the same as well."""
    bm = synth.make_body_model(300, seed=0)
    ctx = capi.Context(bm, synth.make_vposer(seed=1))
    scene = synth.make_scene(ns, seed=9)
    ctx.set_scene(scene)
    s_dev = torch.tensor(scene, device="cuda")
    s_batch = s_dev.unsqueeze(0).expand(B, -1, -1)                      # the reference's repeat(N,1,1) without the copies (:176)
    fast, slow = ops.chamferDist(ctx, both=False), ops.chamferDist(ctx, both=False, use_registered_scene=False)
    rng = np.random.default_rng(B)
    base = scene[rng.integers(0, ns, size=(B, n))] + rng.normal(0, 0.02, size=(B, n, 3)).astype(np.float32)
    x = torch.tensor(base, dtype=torch.float32, device="cuda")
    for step, move in enumerate([0.0, 0.001, 0.002, 0.3, 0.001, 0.05]):
        x = (x + move * torch.randn_like(x)).detach().requires_grad_(True)
        xs = x.detach().clone().requires_grad_(True)
        d_f, _ = fast(x, s_batch)
        d_s, _ = slow(xs, s_batch)
        assert torch.equal(d_f, d_s), (step, float((d_f - d_s).abs().max()))
        assert torch.equal(fast.last_idx1, slow.last_idx1), step
        w = torch.randn_like(d_f)
        (d_f * w).sum().backward()
        (d_s * w).sum().backward()
        assert torch.equal(x.grad, xs.grad), step
    # another shape: fresh seeds, same answers
    x2 = x.detach()[: max(B // 2, 1), : n - 3].contiguous()
    d_f, _ = fast(x2, s_batch[: x2.shape[0]])
    d_s, _ = slow(x2, s_batch[: x2.shape[0]])
    assert torch.equal(d_f, d_s) and torch.equal(fast.last_idx1, slow.last_idx1)
    # a target that is NOT the registered scene (one point moved) is recognised and takes the generic path
    other = s_dev.clone()
    other[7] += 0.5
    d_o, _ = fast(x2, other.unsqueeze(0).expand(x2.shape[0], -1, -1))
    d_r, _ = slow(x2, other.unsqueeze(0).expand(x2.shape[0], -1, -1))
    assert torch.equal(d_o, d_r)
    # ... and an in-place edit of the recognised tensor is noticed (its version changed)
    s_dev[11] += 0.25
    d_e, _ = fast(x2, s_dev.unsqueeze(0).expand(x2.shape[0], -1, -1))
    d_g, _ = slow(x2, s_dev.unsqueeze(0).expand(x2.shape[0], -1, -1))
    assert torch.equal(d_e, d_g)
    # without a registered scene the C entry point says so
    ctx2 = capi.Context(bm, synth.make_vposer(seed=1))
    d1 = torch.empty(2, 5, device="cuda"); i1 = torch.empty(2, 5, device="cuda", dtype=torch.int32)
    rc = ctx2.lib.fdcap_chamfer_fwd_scene(ctx2.handle, capi.dptr(x2), 2, 5, capi.dptr(d1), capi.dptr(i1), 0, capi.current_stream())
    assert rc == -2
    ctx2.close()
    ctx.close()


def test_registered_scene_verdict_does_not_outlive_the_scene_or_the_tensor():
    """the memo that remembers "this target tensor IS the registered scene" must not survive (1) a re-registration of
    another scene of the same size, (2) the freeing of the compared tensor and a new point set allocated at the same address,
    (3) temporaries made by .contiguous() on a non-contiguous target.  Each case is checked against the generic scan."""
    bm = synth.make_body_model(300, seed=0)
    ctx = capi.Context(bm, synth.make_vposer(seed=1))
    ns = 6000
    scene_a, scene_b = synth.make_scene(ns, seed=9), synth.make_scene(ns, seed=10)
    fast, slow = ops.chamferDist(ctx, both=False), ops.chamferDist(ctx, both=False, use_registered_scene=False)
    x = torch.tensor(scene_a[:90].reshape(3, 30, 3) + 0.05, device="cuda")

    def same(target):
        t = target.unsqueeze(0).expand(3, -1, -1)
        d_f, _ = fast(x, t)
        d_s, _ = slow(x, t)
        return torch.equal(d_f, d_s) and torch.equal(fast.last_idx1, slow.last_idx1)

    ctx.set_scene(scene_a)
    a_dev = torch.tensor(scene_a, device="cuda")
    assert same(a_dev) and fast._memo["same"] is True
    # (1) another scene of the same point count is registered: the old tensor is no longer "the scene"
    ctx.set_scene(scene_b)
    assert same(a_dev) and fast._memo["same"] is False
    b_dev = torch.tensor(scene_b, device="cuda")
    assert same(b_dev) and fast._memo["same"] is True
    # (2) free the recognised tensor, allocate other points of the same shape (the caching allocator hands the block back):
    # the memo's reference keeps the old storage alive, so the new tensor cannot alias the remembered address
    ptr = b_dev.untyped_storage().data_ptr()
    del b_dev
    c_dev = torch.tensor(scene_a, device="cuda")
    assert c_dev.untyped_storage().data_ptr() != ptr
    assert same(c_dev) and fast._memo["same"] is False
    # (3) a non-contiguous target (every second row of a wider buffer): compared on every call, nothing remembered about the copy
    wide = torch.zeros(ns, 6, device="cuda")
    wide[:, :3] = torch.tensor(scene_b, device="cuda")
    key = fast._memo["key"]
    assert same(wide[:, :3]) and fast._memo["key"] == key
    wide[:, :3] = torch.tensor(scene_a, device="cuda")
    assert same(wide[:, :3]) and fast._memo["key"] == key
    ctx.close()
