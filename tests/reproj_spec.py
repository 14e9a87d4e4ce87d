"""Specification of the clip-level fit's 2D-keypoint reprojection term (include/fdcap.h fdcap_opt_set_reproj):
a torch twin in the precision it is given, on the oracle's body model, decoder and rotation conversions (imported, not edited).

Per frame i of a clip of N frames and SMPL-X joint j in 0..22

    p_ij  = J_ij(rows_i) + cam_t_i                   J: the posed body-frame joint (G.t + transl), cam_t = row columns 75:78 as they are
    u, v  = fx p.x / p.z + cx,  fy p.y / p.z + cy
    loss  = weight / (23 N) * sum_ij conf_ij^2 [ GMoF_rho(k^u_ij - u) + GMoF_rho(k^v_ij - v) ],   GMoF_rho(r) = rho^2 r^2 / (r^2 + rho^2)

with a keypoint of conf == 0 skipped (exact zeros, whatever its coordinates hold) but counted in 23 N.  The reference has no such
term (parity-unpinned): this file is what the kernels are checked against.  `scale` and camera_ext are leaves of the twin's graph
that the term does not use: their gradients are the exact zeros autograd gives an unused leaf.

MUTANTS are the same term with one deliberate defect; tests/test_reproj_cpu.py shows that each leaves the bars the GPU test holds
the kernels to (tests/gradient_bars.py's formula from the twin's two precisions) by a factor.

make_keypoints / start_rows / check_inputs are the input rules of the GPU tests, run on the CPU by both files."""
import functools

import numpy as np
import torch

import tests.gradient_bars as gb
import tests.test_settings_cpu as sc
from oracle import rotrepr
from oracle.fitting import body_params_encapsulate_batch
from oracle.smplx import SMPLXOracle
from oracle.vposer import VPoserDecoder

NJW = 23
DEPTH = (0.1, -0.2, 3.5)                    # where the pelvis lands in front of the projection (tests/test_gpu_world_frame.py _gt_of_clip)
INTRINSICS = (692.0, 673.0, 640.0, 360.0)   # fx != fy: a swap of the two shows
RHO = 100.0
WEIGHT = 2e-3                               # the term's gradient then has the size of the L1 terms' (1 / (78 N) per column)
MUTANTS = ("no_dcamt", "camt_scale", "conf_linear")
# the shapes of the GPU tests: (n, V, scene points, contact vertices per part, seed) of tests/test_settings_cpu.make_case
CASES = [(12, 300, 800, 20, 0), (4, 120, 50, 1, 11), (7, 777, 801, 7, 12), (65, 512, 2049, 17, 15), (1, 120, 50, 1, 21)]
OUTLIER, UNDETECTED, EMPTY_FRAME = (0, 4), (-1, 7), 2      # (frame, joint) 150 px off; (frame, joint) undetected; the frame without detections (n >= 4)


def gmof(r, rho):
    return rho * rho * r * r / (r * r + rho * rho)


class ReprojTwin:
    def __init__(self, bm, vp, dtype=torch.float64, intrinsics=INTRINSICS, rho=RHO):
        self.dtype = dtype
        self.body = SMPLXOracle(bm, dtype)
        self.vposer = VPoserDecoder.from_data(vp, dtype)
        self.intrinsics, self.rho = intrinsics, rho

    def joints_cam(self, rows, scale=None, mutant=None):
        """rows [n,78] -> the 23 camera-frame joints [n,23,3]"""
        n = rows.shape[0]
        p = body_params_encapsulate_batch(rotrepr.convert_to_3D_rot(rows))
        aa = self.vposer.decode(p["body_pose_vp"], output_type="aa").view(n, -1)
        out = self.body(return_verts=True, body_pose=aa, transl=p["transl"], global_orient=p["global_orient"], betas=p["betas"],
                        left_hand_pose=p["left_hand_pose"], right_hand_pose=p["right_hand_pose"])
        cam_t = rows[:, 75:78]
        if mutant == "no_dcamt":            # the d cam_t sum dropped: the same values, no gradient
            cam_t = cam_t.detach()
        if mutant == "camt_scale":          # the world-joint formula: cam_t times `scale`
            cam_t = cam_t * scale
        return out.joints[:, :NJW, :] + cam_t[:, None, :]

    def project(self, p):
        fx, fy, cx, cy = self.intrinsics
        return fx * p[..., 0] / p[..., 2] + cx, fy * p[..., 1] / p[..., 2] + cy

    def raw_sum(self, rows, kp, scale=None, mutant=None):
        """sum_ij conf^2 [GMoF + GMoF]: what the library leaves in slot 6 of losses_d"""
        kp = torch.as_tensor(np.asarray(kp)).to(self.dtype)
        conf = kp[..., 2]
        on = conf != 0
        zero = torch.zeros_like(conf)
        ku, kv = torch.where(on, kp[..., 0], zero), torch.where(on, kp[..., 1], zero)     # (an undetected keypoint may hold NaN)
        u, v = self.project(self.joints_cam(rows, scale, mutant))
        w = conf if mutant == "conf_linear" else conf * conf
        return torch.where(on, w * (gmof(ku - u, self.rho) + gmof(kv - v, self.rho)), zero).sum()

    def loss(self, rows, kp, weight, scale=None, mutant=None):
        return weight / (NJW * rows.shape[0]) * self.raw_sum(rows, kp, scale, mutant)

    def grads(self, rows_np, kp, weight=WEIGHT, scale=1.8, cams=None, mutant=None):
        """-> {"value", "raw", "rows" [n,78], "dscale", "dcam" [n,16]} (float64 arrays) at rows_np in this twin's precision"""
        n = len(rows_np)
        rows = torch.tensor(np.asarray(rows_np), dtype=self.dtype, requires_grad=True)
        s = torch.tensor(float(scale), dtype=self.dtype, requires_grad=True)
        cam = torch.tensor(np.tile(np.eye(4), (n, 1, 1)) if cams is None else np.asarray(cams).reshape(n, 4, 4), dtype=self.dtype, requires_grad=True)
        raw = self.raw_sum(rows, kp, s, mutant)
        val = weight / (NJW * n) * raw
        g = torch.autograd.grad(val, (rows, s, cam), allow_unused=True)
        g = [torch.zeros_like(p) if gi is None else gi for gi, p in zip(g, (rows, s, cam))]
        return {"value": float(val.detach()), "raw": float(raw.detach()), "rows": g[0].numpy().astype(np.float64), "dscale": float(g[1]),
                "dcam": g[2].numpy().reshape(n, 16).astype(np.float64)}

    def pixel_error(self, rows_np, kp):
        """mean distance in pixels between the detected keypoints (conf > 0) and the projections"""
        kp = np.asarray(kp, dtype=np.float64)
        on = kp[..., 2] != 0
        with torch.no_grad():
            u, v = self.project(self.joints_cam(torch.tensor(np.asarray(rows_np), dtype=self.dtype)))
        d = np.hypot(np.where(on, kp[..., 0], 0) - u.numpy(), np.where(on, kp[..., 1], 0) - v.numpy())
        return float(d[on].mean())


@functools.lru_cache(maxsize=None)
def twin(case, dtype=torch.float64):
    c = sc.make_case(*case)
    return ReprojTwin(c[0], c[1], dtype)


@functools.lru_cache(maxsize=None)
def camera_translation(case):
    """(0.1, -0.2, 3.5) + 0.05 randn per frame, fp32: synth's clips have none, and at z ~ 0 the projection is degenerate"""
    n, seed = case[0], case[4]
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    return np.array(DEPTH, np.float32) + 0.05 * rng.standard_normal((n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ground_truth(case):
    """the clip's rows [n,75] carrying the camera translation"""
    gt = sc.make_case(*case)[2].body_params.astype(np.float32).copy()
    gt[:, 72:75] = camera_translation(case)
    return gt


def rows78(body75):
    """[n,75] -> the fp32 6D rows [n,78] a FittingOP holds after init()"""
    return rotrepr.convert_to_6D_rot(torch.tensor(np.asarray(body75), dtype=torch.float64)).detach().float().numpy()


@functools.lru_cache(maxsize=None)
def make_keypoints(case):
    """[n,23,3] fp32: the fp64 twin's projections of the ground truth + 2 px noise, confidences in [0.3, 1]; one keypoint 150 px off
    (past GMoF's bend), one undetected (conf 0, NaN coordinates), and -- n >= 4 -- one whole frame undetected."""
    n, seed = case[0], case[4]
    t = twin(case)
    with torch.no_grad():
        u, v = t.project(t.joints_cam(torch.tensor(rows78(ground_truth(case)), dtype=torch.float64)))
    rng = np.random.Generator(np.random.PCG64(seed + 17))
    kp = np.stack([u.numpy() + 2.0 * rng.standard_normal((n, NJW)), v.numpy() + 2.0 * rng.standard_normal((n, NJW)),
                   rng.uniform(0.3, 1.0, (n, NJW))], axis=-1).astype(np.float32)
    kp[OUTLIER[0], OUTLIER[1], 0] += 150.0
    kp[UNDETECTED[0], UNDETECTED[1]] = (np.nan, np.nan, 0.0)
    if n >= 4:
        kp[EMPTY_FRAME] = (np.nan, np.nan, 0.0)
    return kp


class DepthEdit:
    """tests/test_settings_cpu.term_gradients' `edit`: the clip's rows carry the camera translation (hashable: one per case)"""

    def __init__(self, case):
        self.case = case

    def clip(self, body_params):
        out = np.asarray(body_params).copy()
        out[:, 72:75] = camera_translation(self.case)
        return out

    def rows(self, x78):
        return x78


@functools.lru_cache(maxsize=None)
def depth_edit(case):
    return DepthEdit(case)


@functools.lru_cache(maxsize=None)
def start_state(case):
    """What the device is given and then holds when the term is differentiated: gb.start_state of the clip with the depth offset in
    cam_t -- "x78" for init(), "rows" after init() (outlier rows replaced) and `+= fp32(perturbation)`, all in fp32."""
    return gb.start_state(case, depth_edit(case))


def start_rows(case):
    return start_state(case)["rows"]


def check_inputs(case, rows=None, kp=None):
    """The conditions under which a comparison means something, asserted before anything is compared."""
    n = case[0]
    rows = start_rows(case) if rows is None else rows
    kp = make_keypoints(case) if kp is None else kp
    t = twin(case)
    with torch.no_grad():
        for r in (rows, rows78(ground_truth(case))):
            z = t.joints_cam(torch.tensor(r, dtype=torch.float64))[..., 2]
            assert float(z.min()) >= 2.0, f"a camera-frame joint at z = {float(z.min())}"
        u, v = t.project(t.joints_cam(torch.tensor(rows78(ground_truth(case)), dtype=torch.float64)))
    on = kp[..., 2] != 0
    res = np.hypot(np.where(on, kp[..., 0], 0) - u.numpy(), np.where(on, kp[..., 1], 0) - v.numpy())
    assert np.all((kp[..., 2][on] >= 0.3) & (kp[..., 2][on] <= 1.0)) and np.all(np.isfinite(kp[on]))
    assert res[OUTLIER] > RHO, "the keypoint past GMoF's bend"
    others = on.copy()
    others[OUTLIER] = False
    assert others.any() and res[others].max() < 15.0, "the noisy detections"
    assert kp[UNDETECTED][2] == 0 and np.all(np.isnan(kp[UNDETECTED][:2])), "the undetected keypoint"
    if n >= 4:
        assert np.all(kp[EMPTY_FRAME][:, 2] == 0) and np.all(np.isnan(kp[EMPTY_FRAME][:, :2])), "the frame without detections"
        assert on[[i for i in range(n) if i != EMPTY_FRAME]].any(axis=1).all()


@functools.lru_cache(maxsize=None)
def isolated(case):
    """-> {"g64", "g32": {block: array}, "bar": {block: float}, "raw64", "rows", "kp"}: the term alone (weight WEIGHT) at start_rows in the
    twin's two precisions, cut into tests/gradient_bars.py's blocks (rows, d scale, d camera_ext), and the bars of its formula."""
    check_inputs(case)
    rows, kp = start_rows(case), make_keypoints(case)
    g = {}
    for name, dtype in (("g64", torch.float64), ("g32", torch.float32)):
        t = twin(case, dtype).grads(rows, kp)
        g[name] = gb.blocks(rows=t["rows"], dscale=t["dscale"], dcam=t["dcam"])
        g["raw" + name[1:]] = t["raw"]
    return dict(g, bar=gb.bars(g["g32"], g["g64"]), rows=rows, kp=kp)


def fit75(case):
    """The comparative fit's data: the ground truth displaced by the perturbation (its columns for the 75-d layout), fp32 [n,75]"""
    p = sc.perturbation(case[0]).numpy()
    return (ground_truth(case) + np.concatenate([p[:, 0:6], p[:, 9:78]], axis=1)).astype(np.float32)


def adam_fit(case, weight, iters, dtype=torch.float32):
    """The oracle's mode 'global' loop over `iters` iterations at the default weights from fit75(case), with the term (weight; 0: off)
    in both phase totals -> the rows [n,78] it ends at (float64 array)."""
    f = sc.make_oracle(sc.make_case(*case), sc.DEFAULTS, dtype, num_iter=iters)
    t = twin(case, dtype)
    kp = make_keypoints(case)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(fit75(case), dtype=torch.float64)).detach().float().to(dtype)
    idx1 = f.init(x78)
    for ii in range(iters):
        f.optimizer.zero_grad(set_to_none=True)
        l_rec, l_vp, l_con, l_sm, l_ws = f.cal_loss(x78, idx1)
        phase1 = ii < iters * f.phase_split
        f.camera_ext.requires_grad = not phase1
        f.scale.requires_grad = phase1
        loss = (l_con * f.phase1_contact + l_sm * f.phase1_smooth + l_rec) if phase1 else (l_rec + l_ws * f.phase2_world + l_sm * f.phase2_smooth)
        if weight:
            loss = loss + t.loss(f.body_rotation_rec, kp, weight)
        loss.backward()
        f.optimizer.step()
    return f.body_rotation_rec.detach().numpy().astype(np.float64)
