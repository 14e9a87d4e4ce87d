"""The inner fit's start from keypoints alone (csrc/fdc_fit2d_init.h) as a torch twin: the depth guess, the camera stage's objective
and its two optimisers, the 180-degree twin and the choice between the two fits.  Built on tests/keypoint_spec.KeypointSpec /
oracle.innerfit.InnerFitOracle and changing nothing in them.

The camera objective is evaluated through the FULL model forward (decoder, 55 joints, vertices where the map has them) with autograd
over the whole row, never through the closed form the kernels use: that reduction -- Jw_k = base + R_root q_k + cam_t with
q_k = R_root0^T (G_k.t - G_0.t) fixed at set-up -- is itself under test.  `closed_form_grad` restates the reduction in torch with
switches that break it (MUTANTS), for tests/test_fit2d_init_cpu.py to show that the bars see each piece.

A SLOT indexes a frame's keypoint array (its joint: self.joint[slot]); settings are a dict with the keys of
fdcap_amd.innerfit.DEFAULT_INIT resolved to slots: edges [(a, b)], torso [slots], shoulders (a, b), conf_thr, default_depth,
side_view_px, w_data, w_depth."""
import numpy as np
import torch

from oracle import rotrepr
from oracle.innerfit import InnerFitOracle
from tests.keypoint_spec import KeypointSpec

FREE = list(range(3, 9)) + list(range(75, 78))               # the camera stage's nine columns of a 78-wide row
FIXED = [c for c in range(78) if c not in FREE]
MUTANTS = ("q_not_rotated_back", "no_depth_term")


def rodrigues(aa):
    """exp([aa]x), float64 numpy [.., 3] -> [.., 3, 3] (the exact map: no epsilon)"""
    aa = np.asarray(aa, dtype=np.float64)
    th = np.linalg.norm(aa, axis=-1)[..., None, None]
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -aa[..., 2], aa[..., 1], aa[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -aa[..., 0], -aa[..., 1], aa[..., 0]
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0, np.sin(ths) / ths)
    b = np.where(small, 0.5, (1.0 - np.cos(ths)) / ths ** 2)
    return np.eye(3) + a * K + b * (K @ K)


def flip_rotation(aa):
    """the rotation the flipped global_orient must be: R(aa) R_y(pi)"""
    return rodrigues(aa) @ np.diag([-1.0, 1.0, -1.0])


def select(loss, src):
    """-> chosen [n] (0 / 1) and the problem index each frame takes; loss [n + m], src [m] ascending and unique"""
    loss = np.asarray(loss, dtype=np.float64)
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    n = loss.shape[0] - src.shape[0]
    l = np.where(np.isnan(loss), np.inf, loss)
    chosen, take = np.zeros(n, np.int32), np.arange(n)
    for i, f in enumerate(src):
        if l[n + i] < l[f]:
            chosen[f], take[f] = 1, n + i
    return chosen, take


class Fit2dInitSpec(KeypointSpec):
    def __init__(self, bm, vp, settings, joint=None, tri=None, bary=None, intrinsics=(692.0, 692.0, 640.0, 360.0), dtype=torch.float64):
        if joint is None:                                    # the 23-joint layout: slot k is joint k
            joint, tri, bary = np.arange(23), np.zeros((23, 3), np.int64), np.zeros((23, 3))
        super().__init__(bm, vp, joint, tri, bary, intrinsics=intrinsics, dtype=dtype)
        self.s = dict(settings)

    def _t(self, a):
        return torch.as_tensor(np.asarray(a), dtype=self.dtype)

    # ---- the depth guess ----------------------------------------------------------------------------------------------------------
    def depth_guess(self, x78, kp):
        """-> z [n], valid [n]"""
        x78, kp, s = self._t(x78), self._t(kp), self.s
        with torch.no_grad():
            J = self.joints_cam(x78)
        z, valid = [], []
        for f in range(x78.shape[0]):
            l3, l2 = [], []
            for a, b in s["edges"]:
                if not (kp[f, a, 2] > s["conf_thr"] and kp[f, b, 2] > s["conf_thr"]):
                    continue
                l3.append(float(torch.linalg.norm(J[f, a] - J[f, b])))
                l2.append(float(np.hypot(float(kp[f, a, 0] - kp[f, b, 0]) / self.fx, float(kp[f, a, 1] - kp[f, b, 1]) / self.fy)))
            ok = len(l3) > 0 and np.mean(l2) >= 1e-6
            z.append(np.mean(l3) / np.mean(l2) if ok else s["default_depth"])
            valid.append(int(ok))
        return np.array(z), np.array(valid, np.int32)

    def shoulder_distance(self, kp):
        kp = np.asarray(kp, dtype=np.float64)
        a, b = self.s["shoulders"]
        return np.hypot(kp[:, a, 0] - kp[:, b, 0], kp[:, a, 1] - kp[:, b, 1])

    def side_view(self, kp):
        kp = np.asarray(kp, dtype=np.float64)
        a, b = self.s["shoulders"]
        return ((kp[:, a, 2] > self.s["conf_thr"]) & (kp[:, b, 2] > self.s["conf_thr"])
                & (self.shoulder_distance(kp) < self.s["side_view_px"])).astype(np.int32)

    # ---- the camera stage's objective, through the full model ------------------------------------------------------------------------
    def camera_frame_loss(self, x78, kp, z0):
        """[n]; x78 a tensor (autograd reaches every column), kp / z0 tensors"""
        s = self.s
        uv = self.project(self.joints_cam(x78))[:, s["torso"]]
        k = kp[:, s["torso"]]
        gate = (k[..., 2] > s["conf_thr"]).to(self.dtype)
        data = s["w_data"] ** 2 * (gate[..., None] * (uv - k[..., :2]) ** 2).sum((1, 2))
        return data + s["w_depth"] ** 2 * (x78[:, 77] - z0) ** 2

    def camera_grads(self, x78, kp, z0):
        """-> frame loss [n], d / d row [n, 78] (the nine FREE columns are the stage's gradient)"""
        x = self._t(x78).clone().requires_grad_(True)
        fl = self.camera_frame_loss(x, self._t(kp), self._t(z0))
        g, = torch.autograd.grad(fl.sum(), x)
        return fl.detach().numpy().astype(np.float64), g.numpy().astype(np.float64)

    def closed_form_grad(self, x78, x78_setup, kp, z0, mutant=None):
        """The kernels' reduction restated: set-up at x78_setup (q_k, the pelvis base), one evaluation at x78 -> loss [n], gradient of the
        nine FREE columns [n, 9].  mutant in MUTANTS breaks one piece of it (None: the reduction as built)."""
        assert mutant is None or mutant in MUTANTS
        s, kp, z0 = self.s, self._t(kp), self._t(z0)
        xs = self._t(x78_setup)
        with torch.no_grad():
            Js = self.joints_cam(xs) - xs[:, None, 75:78]                                # G_k.t + transl
            pel = self.pelvis(xs)
            R0 = rotrepr.decode_6d(xs[:, 3:9])
            d = Js[:, s["torso"]] - pel[:, None]
            q = d if mutant == "q_not_rotated_back" else torch.einsum("nji,nkj->nki", R0, d)
        x = self._t(x78).clone().requires_grad_(True)
        R = rotrepr.decode_6d(x[:, 3:9])
        J = pel[:, None] + torch.einsum("nij,nkj->nki", R, q) + x[:, None, 75:78]
        k = kp[:, s["torso"]]
        gate = (k[..., 2] > s["conf_thr"]).to(self.dtype)
        fl = s["w_data"] ** 2 * (gate[..., None] * (self.project(J) - k[..., :2]) ** 2).sum((1, 2))
        if mutant != "no_depth_term":
            fl = fl + s["w_depth"] ** 2 * (x[:, 77] - z0) ** 2
        g, = torch.autograd.grad(fl.sum(), x)
        return fl.detach().numpy().astype(np.float64), g.numpy().astype(np.float64)[:, FREE]

    def pelvis(self, x78):
        """G_0.t + transl [n, 3]: joint 0, whether or not the map holds it"""
        return InnerFitOracle.joints_cam(self, x78)[:, 0] - x78[:, 75:78]

    # ---- the camera stage's optimisers: only the nine FREE columns are unknowns ------------------------------------------------------
    def _free_problem(self, x78, kp):
        x0 = self._t(x78).clone()
        return x0, self._t(kp), x0[:, 77].clone()

    def _compose(self, x0, free):
        return x0.index_copy(1, torch.tensor(FREE), free)

    def camera_stage_adam(self, x78, kp, iters, lr):
        x0, kpt, z0 = self._free_problem(x78, kp)
        free = x0[:, FREE].clone().requires_grad_(True)
        opt = torch.optim.Adam([free], lr=lr)
        for _ in range(iters):
            opt.zero_grad()
            self.camera_frame_loss(self._compose(x0, free), kpt, z0).sum().backward()
            opt.step()
        return self._compose(x0, free.detach()).numpy()

    def camera_stage_lbfgs(self, x78, kp, history=100, max_iter=30, max_eval=0, max_steps=30, lr=1.0, tolerance_grad=1e-7,
                           tolerance_change=1e-9, ftol=2e-9, gtol=1e-9):
        """oracle.innerfit.InnerFitOracle.fitting_lbfgs's loop, per frame, on the camera objective and its nine unknowns"""
        x0, kpt, z0 = self._free_problem(x78, kp)
        out = x0.clone()
        for f in range(x0.shape[0]):
            free = x0[f:f + 1, FREE].clone().requires_grad_(True)
            opt = torch.optim.LBFGS([free], lr=lr, max_iter=max_iter, max_eval=max_eval if max_eval > 0 else None, history_size=history,
                                    tolerance_grad=tolerance_grad, tolerance_change=tolerance_change, line_search_fn="strong_wolfe")
            loss_of = lambda: self.camera_frame_loss(self._compose(x0[f:f + 1], free), kpt[f:f + 1], z0[f:f + 1]).sum()

            def closure():
                opt.zero_grad()
                loss = loss_of()
                loss.backward()
                return loss
            prev = None
            for n in range(max_steps):
                loss = float(opt.step(closure).detach())
                if not (abs(loss) < float("inf")):
                    break
                if n > 0 and prev is not None and ftol > 0 and abs(prev - loss) / max(abs(prev), abs(loss), 1.0) <= ftol:
                    break
                g, = torch.autograd.grad(loss_of(), free)
                if float(g.abs().max()) < gtol:
                    break
                prev = loss
            out[f] = self._compose(x0[f:f + 1], free.detach())[0]
        return out.numpy()

    def torso_error(self, x78, kp):
        """mean pixel distance of the gated torso keypoints [n]"""
        s, kp = self.s, self._t(kp)
        with torch.no_grad():
            uv = self.project(self.joints_cam(self._t(x78)))[:, s["torso"]]
        k = kp[:, s["torso"]]
        gate = (k[..., 2] > s["conf_thr"]).to(self.dtype)
        d = torch.sqrt(((uv - k[..., :2]) ** 2).sum(-1))
        return ((gate * d).sum(1) / gate.sum(1).clamp(min=1)).numpy()


# ---- shared cases (tests/test_fit2d_init_cpu.py, tests/test_gpu_fit2d_init.py) ------------------------------------------------------
L_SHOULDER, R_SHOULDER, L_HIP, R_HIP = 16, 17, 1, 2
# a map that mixes the three kinds of keypoint: joints 0..22, joints 23..54 (pseudo-vertices) and surface points
MAP_JOINTS = (0, R_SHOULDER, L_SHOULDER, -1, R_HIP, L_HIP, 12, 40, 4, 5, -1, 20, 21, 28)
INTRINSICS = (692.0, 640.0, 640.0, 360.0)                    # fx != fy


def settings_for(joint_of_slot, torso_joints=(L_SHOULDER, R_SHOULDER, L_HIP, R_HIP), **over):
    """settings in SLOTS for a layout given as the joint of every slot (-1: a surface point)"""
    slot = {int(j): k for k, j in reversed(list(enumerate(joint_of_slot))) if j >= 0}
    s = dict(edges=[(slot[L_SHOULDER], slot[L_HIP]), (slot[R_SHOULDER], slot[R_HIP])], torso=[slot[j] for j in torso_joints],
             shoulders=(slot[L_SHOULDER], slot[R_SHOULDER]), conf_thr=0.0, default_depth=2.5, side_view_px=25.0, w_data=1000.0 / 720.0,
             w_depth=100.0)
    s.update(over)
    return s


def make_case(n, seed, mapped, synth, torso_joints=(L_SHOULDER, R_SHOULDER, L_HIP, R_HIP), depth=(2.0, 4.0), noise_px=1.0):
    """A synthetic body (240 vertices), a ground-truth clip `depth` metres in front of the camera and its projected keypoints
    (+ noise_px pixels of noise, confidences in 0.3..1) in the 23-joint layout or in MAP_JOINTS' order.
    -> dict(bm, vp, map (joint, tri, bary) or None, joint_of_slot, settings, gt78 [n,78] fp32, kp [n,n_kp,3] fp32)"""
    bm, vp = synth.make_body_model(240, seed=seed), synth.make_vposer(seed=seed + 1)
    clip = synth.make_clip(n, seed=seed + 2, num_outliers=0)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    gt = clip.body_params.astype(np.float32).copy()
    gt[:, 72:75] = np.stack([0.2 * rng.standard_normal(n), 0.2 * rng.standard_normal(n), rng.uniform(*depth, n)], 1)
    if mapped:
        joint = np.array(MAP_JOINTS)
        tri = np.zeros((len(joint), 3), np.int64)
        bary = np.zeros((len(joint), 3))
        for k in np.flatnonzero(joint < 0):
            tri[k], bary[k] = rng.choice(240, 3, replace=False), rng.dirichlet(np.ones(3))
        m = (joint, tri, bary)
    else:
        joint, m = np.arange(23), None
    settings = settings_for(joint, torso_joints)
    spec = Fit2dInitSpec(bm, vp, settings, *(m or ()), intrinsics=INTRINSICS)
    gt78 = rotrepr.convert_to_6D_rot(torch.tensor(gt, dtype=torch.float64)).numpy().astype(np.float32)
    with torch.no_grad():
        uv = spec.project(spec.joints_cam(torch.tensor(gt78, dtype=torch.float64))).numpy()
    kp = np.concatenate([uv + noise_px * rng.standard_normal(uv.shape), rng.uniform(0.3, 1.0, uv.shape[:2] + (1,))], -1).astype(np.float32)
    return dict(bm=bm, vp=vp, map=m, joint_of_slot=joint, settings=settings, gt78=gt78, kp=kp)


def spec_of(case, dtype=torch.float64, **over):
    return Fit2dInitSpec(case["bm"], case["vp"], {**case["settings"], **over}, *(case["map"] or ()), intrinsics=INTRINSICS, dtype=dtype)


def turned(x78, angle, rng):
    """rows with global_orient turned by `angle` rad about a random axis (6D of R_axis(angle) R), fp32"""
    x = np.array(x78, dtype=np.float64)
    ax = rng.standard_normal((x.shape[0], 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    R = rotrepr.decode_6d(torch.tensor(x[:, 3:9])).numpy()
    x[:, 3:9] = (rodrigues(angle * ax) @ R)[:, :, :2].reshape(-1, 6)
    return x.astype(np.float32)
