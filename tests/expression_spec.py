"""The inner fit's objective with free expression coefficients, as a torch twin (csrc/fdc_keypoints.h).

Extends tests/face_spec.FaceSpec and changes nothing under oracle/: the body model is a subclass of face_spec.JawBody whose forward
puts `expression` [B, 10] into smplx's shape_components -- v_shaped = v_template + S betas + E psi, joints regressed from v_shaped:
the DIRECT form.  float64 is the yardstick of tests/test_gpu_expression.py, float32 the twin its run-to-run bars come from.

CORRECTION FORM.  `correction=True` evaluates the chain at psi = 0 as the oracle does and then exactly what the kernel does on top of
it: delta_j = JE_j psi (JE = J_regressor E), Dt_0 = delta_0, Dt_j = Dt_p + R_p (delta_j - delta_p), A_j.t += Dt_j - R_j delta_j, joints
0..22 += Dt_j, joints 23..54 as pseudo-vertices A'_j [J_j + delta_j; 1], the vertices' rest positions += E_u psi, and the jaw's leaf form
on the corrected A_22 with J22 + delta_22.  `mutant` detaches one piece of it (values unchanged, a contribution to the gradient
missing): tests/test_expression_cpu.py shows that the two forms agree and that every mutant leaves the bars of the GPU test."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rotrepr
from oracle.fitting import body_params_encapsulate_batch
from oracle.innerfit import DEFAULT_INTRINSICS
from oracle.smplx import batch_rigid_transform, batch_rodrigues
from tests.face_spec import DEFAULT_BEND_TERMS, JAW, FaceSpec, JawBody

NEXPR = 10
MUTANTS = ("rot_addend", "parent_term", "jw", "pseudo_rows", "real_rows", "jaw_delta", "prior")


def chain_correction(RG, delta, parents, mutant=None):
    """RG [b, 55, 3, 3] the chain's rotations, delta [b, 55, 3] -> (Dt [b, 55, 3], the addend Dt_j - R_j delta_j to A_j.t)"""
    dts = [delta[:, 0]]
    for j in range(1, delta.shape[1]):
        p = int(parents[j])
        dp = delta[:, p].detach() if mutant == "parent_term" else delta[:, p]
        dts.append(dts[p] + torch.matmul(RG[:, p], (delta[:, j] - dp).unsqueeze(-1))[..., 0])
    dt = torch.stack(dts, dim=1)
    Rj = RG.detach() if mutant == "rot_addend" else RG
    return dt, dt - torch.matmul(Rj, delta.unsqueeze(-1))[..., 0]


class ExprBody(JawBody):
    """JawBody.forward with expression [B, 10] in shape_components (direct), or as the correction of the chain at psi = 0."""
    correction, mutant = False, None

    def forward(self, return_verts=True, body_pose=None, transl=None, global_orient=None, betas=None, left_hand_pose=None,
                right_hand_pose=None, jaw_pose=None, expression=None, **unused):
        b = body_pose.shape[0]
        m = self.mutant
        z3 = torch.zeros(b, 3, dtype=self.dtype)
        jaw = z3 if jaw_pose is None else jaw_pose
        psi = torch.zeros(b, NEXPR, dtype=self.dtype) if expression is None else expression
        corr = self.correction
        lh = torch.einsum("bi,ij->bj", left_hand_pose, self.lh_comp)
        rh = torch.einsum("bi,ij->bj", right_hand_pose, self.rh_comp)
        full_pose = torch.cat([global_orient, body_pose, z3 if corr else jaw, z3, z3, lh, rh], dim=1)
        full_pose = full_pose + self.pose_mean
        S, E = self.shapedirs[:, :, :10], self.shapedirs[:, :, 10:10 + NEXPR]
        if corr:
            v_shaped = self.v_template + torch.einsum("bl,mkl->bmk", betas, S)
        else:
            v_shaped = self.v_template + torch.einsum("bl,mkl->bmk", torch.cat([betas, psi], dim=-1), self.shapedirs)
        J = torch.einsum("bik,ji->bjk", v_shaped, self.J_regressor)
        rot_mats = batch_rodrigues(full_pose.reshape(-1, 3)).view(b, -1, 3, 3)
        ident = torch.eye(3, dtype=self.dtype)
        pose_feature = (rot_mats[:, 1:] - ident).reshape(b, -1)
        if corr:                                                 # the jaw's block, zero in the chain
            Rw = batch_rodrigues(jaw)
            pose_feature = torch.cat([pose_feature[:, :9 * (JAW - 1)], (Rw - ident).reshape(b, 9), pose_feature[:, 9 * JAW:]], dim=1)
            v_rest = v_shaped + torch.einsum("bl,mkl->bmk", psi.detach() if m == "real_rows" else psi, E)
        else:
            v_rest = v_shaped
        v_posed = v_rest + torch.matmul(pose_feature, self.posedirs).view(b, -1, 3)
        J_transformed, A = batch_rigid_transform(rot_mats, J, self.parents)
        joints = J_transformed
        if corr:
            JE = torch.einsum("mkl,jm->jkl", E, self.J_regressor)            # [55, 3, 10]
            delta = torch.einsum("jkl,bl->bjk", JE, psi)
            RG = A[:, :, :3, :3]
            dt, add = chain_correction(RG, delta, self.parents, m)
            tA = A[:, :, :3, 3] + add
            # joints 0..22: the world joints' correction; joints 23..54: pseudo-vertices of the keypoint set
            jw = J_transformed[:, :23] + (dt[:, :23].detach() if m == "jw" else dt[:, :23])
            rest = J[:, 23:] + (delta[:, 23:].detach() if m == "pseudo_rows" else delta[:, 23:])
            pseudo = torch.matmul(RG[:, 23:], rest.unsqueeze(-1))[..., 0] + tA[:, 23:]
            joints = torch.cat([jw, pseudo], dim=1)
            # the jaw's leaf form on the corrected A_22, with J22 + delta_22
            RA, J22 = RG[:, JAW], J[:, JAW] + (delta[:, JAW].detach() if m == "jaw_delta" else delta[:, JAW])
            lever = torch.matmul(ident - Rw, J22.unsqueeze(-1))
            t22 = tA[:, JAW] + torch.matmul(RA, lever)[..., 0]
            rot = torch.cat([RG[:, :JAW], torch.matmul(RA, Rw).unsqueeze(1), RG[:, JAW + 1:]], dim=1)
            tA = torch.cat([tA[:, :JAW], t22.unsqueeze(1), tA[:, JAW + 1:]], dim=1)
            A = F.pad(torch.cat([rot, tA.unsqueeze(-1)], dim=3), [0, 0, 0, 1])
        W = self.lbs_weights.unsqueeze(0).expand(b, -1, -1)
        nj = self.J_regressor.shape[0]
        T = torch.matmul(W, A.reshape(b, nj, 16)).view(b, -1, 4, 4)
        homo = torch.cat([v_posed, torch.ones(b, v_posed.shape[1], 1, dtype=self.dtype)], dim=2)
        verts = torch.matmul(T, homo.unsqueeze(-1))[:, :, :3, 0]
        if transl is not None:
            joints = joints + transl.unsqueeze(1)
            verts = verts + transl.unsqueeze(1)
        return SimpleNamespace(vertices=verts, joints=joints, full_pose=full_pose)


class ExpressionSpec(FaceSpec):
    """expr [n, 10] (None: fixed at zero, FaceSpec's model) and w_expr (the prior w_expr^2 |psi|^2) are arguments of every method."""

    def __init__(self, bm, vp, joint, tri, bary, intrinsics=DEFAULT_INTRINSICS, rho=100.0, lr=0.01, dtype=torch.float64,
                 bend_terms=DEFAULT_BEND_TERMS, correction=False, mutant=None):
        super().__init__(bm, vp, joint, tri, bary, intrinsics, rho, lr, dtype, bend_terms)
        assert mutant is None or mutant in MUTANTS
        self.body_mesh_model = ExprBody(bm, dtype=dtype)
        self.body_mesh_model.correction, self.body_mesh_model.mutant = bool(correction or mutant), mutant
        self.mutant = mutant

    def joints_cam(self, x78, jaw=None, expr=None):
        n = x78.shape[0]
        p = body_params_encapsulate_batch(rotrepr.convert_to_3D_rot(x78))
        joint_rot = self.vposer.decode(p["body_pose_vp"], output_type="aa").view(n, -1)
        out = self.body_mesh_model(return_verts=True, body_pose=joint_rot, transl=p["transl"], global_orient=p["global_orient"],
                                   betas=p["betas"], left_hand_pose=p["left_hand_pose"], right_hand_pose=p["right_hand_pose"], jaw_pose=jaw,
                                   expression=expr)
        is_joint = self.joint >= 0
        from_joints = out.joints[:, self.joint.clamp(min=0), :]
        from_surface = (out.vertices[:, self.tri, :] * self.bary[None, :, :, None]).sum(2)
        return torch.where(is_joint[None, :, None], from_joints, from_surface) + x78[:, 75:78].unsqueeze(1)

    def frame_terms(self, x78, kp, stage, jaw=None, w_jaw=None, w_bend=0.0, expr=None, w_expr=0.0):
        """(data [n], prior [n]) per frame"""
        w_data, w_pose, w_shape, w_hand = stage
        r2 = (kp[..., :2] - self.project(self.joints_cam(x78, jaw, expr))) ** 2
        data = w_data ** 2 * (kp[..., 2:3] ** 2 * self.rho ** 2 * r2 / (r2 + self.rho ** 2)).sum((1, 2))
        prior = (w_pose ** 2 * (x78[:, 19:51] ** 2).sum(1) + w_shape ** 2 * (x78[:, 9:19] ** 2).sum(1)
                 + w_hand ** 2 * (x78[:, 51:75] ** 2).sum(1)) + self.extra_prior(x78, jaw, w_jaw, w_bend)
        if expr is not None and w_expr:
            prior = prior + w_expr ** 2 * ((expr.detach() if self.mutant == "prior" else expr) ** 2).sum(1)
        return data, prior

    def frame_loss(self, x78, kp, stage, jaw=None, w_jaw=None, w_bend=0.0, expr=None, w_expr=0.0):
        data, prior = self.frame_terms(x78, kp, stage, jaw, w_jaw, w_bend, expr, w_expr)
        return data + prior

    def loss(self, x78, kp, stage, jaw=None, w_jaw=None, w_bend=0.0, expr=None, w_expr=0.0):
        data, prior = self.frame_terms(x78, kp, stage, jaw, w_jaw, w_bend, expr, w_expr)
        return data.sum(), prior.sum()

    def positions(self, x_np, jaw_np=None, expr_np=None):
        t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=self.dtype)
        with torch.no_grad():
            return self.joints_cam(t(x_np), t(jaw_np), t(expr_np)).numpy()

    def grads(self, x_np, kp_np, stage, jaw_np=None, w_jaw=None, w_bend=0.0, expr_np=None, w_expr=0.0):
        """-> (sums [2], d rows [n, 78], d jaw [n, 3] or None, d expr [n, 10] or None) at numpy inputs, in this twin's precision"""
        leaf = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=self.dtype, requires_grad=True)
        x, jaw, expr = leaf(x_np), leaf(jaw_np), leaf(expr_np)
        data, prior = self.loss(x, torch.tensor(np.asarray(kp_np), dtype=self.dtype), stage, jaw, w_jaw, w_bend, expr, w_expr)
        (data + prior).backward()
        g = lambda v: None if v is None else (torch.zeros_like(v) if v.grad is None else v.grad).numpy().astype(np.float64)
        return np.array([float(data.detach()), float(prior.detach())]), g(x), g(jaw), g(expr)

    def fitting_expr(self, rows75, keypoints, stages, iters_per_stage, expr_init, expr_prior, jaw_init=None, jaw_prior=None, bend_ratio=0.0):
        """FaceSpec.fitting_face with the coefficients as one more Adam parameter of the same lr and step count -> rows75, jaw, expr"""
        x = rotrepr.convert_to_6D_rot(torch.as_tensor(rows75).to(self.dtype)).detach().clone().requires_grad_(True)
        jaw = None if jaw_init is None else torch.as_tensor(jaw_init).to(self.dtype).detach().clone().requires_grad_(True)
        expr = torch.as_tensor(expr_init).to(self.dtype).detach().clone().requires_grad_(True)
        kp = torch.as_tensor(keypoints).to(self.dtype)
        for si, stage in enumerate(stages):
            opt = torch.optim.Adam([v for v in (x, jaw, expr) if v is not None], lr=self.lr)
            for _ in range(iters_per_stage):
                opt.zero_grad()
                data, prior = self.loss(x, kp, stage, jaw, None if jaw_prior is None else jaw_prior[si], bend_ratio * stage[1], expr,
                                        float(expr_prior[si]))
                (data + prior).backward()
                opt.step()
        self.x78 = x.detach()
        return rotrepr.convert_to_3D_rot(x).detach(), None if jaw is None else jaw.detach(), expr.detach()
