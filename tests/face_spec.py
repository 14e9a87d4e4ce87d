"""The inner fit's objective with a free jaw and SMPLify-X's bending prior, as a torch twin (csrc/fdc_keypoints.h, csrc/fdc_fit2d.h).

Extends tests/keypoint_spec.KeypointSpec and changes nothing under oracle/: the body model is a subclass of oracle.smplx.SMPLXOracle
whose forward puts `jaw_pose` where the oracle writes its first z3 (joint 22), the two priors come from vposer.decode(..., 'aa') and
the jaw itself.  float64 is the yardstick of tests/test_gpu_face.py, float32 the twin its run-to-run bars come from.

LEAF FORM.  Joint 22 has parent 15 and no child, so a free jaw changes two things only: the pose-feature block 189..197 = R_w - I and
the skinning transform A'_22 = (R_A R_w, t_A + R_A (I - R_w) J22), with (R_A, t_A) the transform the chain gives at jaw = 0 and J22
the joint's rest position.  `leaf=True` evaluates exactly that on top of the oracle's chain at jaw = 0 -- the form the kernel uses --
and `mutant` detaches one piece of it (values unchanged, a contribution to the gradient missing): tests/test_face_cpu.py shows that
the two forms agree and that every mutant leaves the bars of tests/test_gpu_face.py."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import rotrepr
from oracle.fitting import body_params_encapsulate_batch
from oracle.innerfit import DEFAULT_INTRINSICS
from oracle.smplx import SMPLXOracle, batch_rigid_transform, batch_rodrigues
from tests.keypoint_spec import KeypointSpec

JAW = 22
DEFAULT_BEND_TERMS = ((18, 1, 1.0), (19, 1, -1.0), (4, 0, -1.0), (5, 0, -1.0))
MUTANTS = ("pf_block", "A_rot", "A_transl", "dJ22", "dA_addend", "no_bend")


class JawBody(SMPLXOracle):
    """SMPLXOracle.forward line for line, with jaw_pose [B, 3] in joint 22's slot of the full pose."""
    leaf, mutant = False, None

    def forward(self, return_verts=True, body_pose=None, transl=None, global_orient=None, betas=None, left_hand_pose=None,
                right_hand_pose=None, jaw_pose=None, **unused):
        b = body_pose.shape[0]
        z3 = torch.zeros(b, 3, dtype=self.dtype)
        jaw = z3 if jaw_pose is None else jaw_pose
        expression = torch.zeros(b, 10, dtype=self.dtype)
        lh = torch.einsum("bi,ij->bj", left_hand_pose, self.lh_comp)
        rh = torch.einsum("bi,ij->bj", right_hand_pose, self.rh_comp)
        full_pose = torch.cat([global_orient, body_pose, z3 if self.leaf else jaw, z3, z3, lh, rh], dim=1)
        full_pose = full_pose + self.pose_mean
        shape_components = torch.cat([betas, expression], dim=-1)
        v_shaped = self.v_template + torch.einsum("bl,mkl->bmk", shape_components, self.shapedirs)
        J = torch.einsum("bik,ji->bjk", self.tap("v_shaped_to_joints", v_shaped), self.J_regressor)
        rot_mats = batch_rodrigues(full_pose.reshape(-1, 3)).view(b, -1, 3, 3)
        ident = torch.eye(3, dtype=self.dtype)
        pose_feature = (rot_mats[:, 1:] - ident).reshape(b, -1)
        Rw = batch_rodrigues(jaw) if self.leaf else None
        if self.leaf:                                            # the block that is zero at jaw = 0
            blk = (Rw - ident).reshape(b, 9)
            if self.mutant == "pf_block":
                blk = blk.detach()
            pose_feature = torch.cat([pose_feature[:, :9 * (JAW - 1)], blk, pose_feature[:, 9 * JAW:]], dim=1)
        pose_feature = self.tap("pose_feature", pose_feature)
        v_posed = self.tap("v_posed", v_shaped + torch.matmul(pose_feature, self.posedirs).view(b, -1, 3))
        J_transformed, A = batch_rigid_transform(rot_mats, J, self.parents)
        if self.leaf:
            m = self.mutant
            RA, tA, J22 = A[:, JAW, :3, :3], A[:, JAW, :3, 3], J[:, JAW]
            rot = torch.matmul(RA, Rw.detach() if m == "A_rot" else Rw)
            lever = torch.matmul(ident - Rw, (J22.detach() if m == "dJ22" else J22).unsqueeze(-1))
            shift = torch.matmul(RA.detach() if m == "dA_addend" else RA, lever)[..., 0]
            if m == "A_transl":
                shift = shift.detach()
            A22 = F.pad(torch.cat([rot, (tA + shift).unsqueeze(-1)], dim=2), [0, 0, 0, 1])
            A = torch.cat([A[:, :JAW], A22.unsqueeze(1), A[:, JAW + 1:]], dim=1)
        W = self.lbs_weights.unsqueeze(0).expand(b, -1, -1)
        nj = self.J_regressor.shape[0]
        T = torch.matmul(W, A.reshape(b, nj, 16)).view(b, -1, 4, 4)
        homo = torch.cat([v_posed, torch.ones(b, v_posed.shape[1], 1, dtype=self.dtype)], dim=2)
        verts = torch.matmul(T, homo.unsqueeze(-1))[:, :, :3, 0]
        joints = J_transformed
        if transl is not None:
            joints = joints + transl.unsqueeze(1)
            verts = verts + transl.unsqueeze(1)
        return SimpleNamespace(vertices=verts, joints=joints, full_pose=full_pose)


class FaceSpec(KeypointSpec):
    """w_jaw [3] (None: no jaw prior) and w_bend (0: off) with `bend_terms` (joint 1..21, axis, sign) are the current stage's; the
    jaw [n, 3] is an argument of every method (None: fixed at zero, KeypointSpec's model)."""

    def __init__(self, bm, vp, joint, tri, bary, intrinsics=DEFAULT_INTRINSICS, rho=100.0, lr=0.01, dtype=torch.float64,
                 bend_terms=DEFAULT_BEND_TERMS, leaf=False, mutant=None):
        super().__init__(bm, vp, joint, tri, bary, intrinsics, rho, lr, dtype)
        assert mutant is None or mutant in MUTANTS
        self.body_mesh_model = JawBody(bm, dtype=dtype)
        self.body_mesh_model.leaf, self.body_mesh_model.mutant = bool(leaf or mutant), mutant
        self.bend_terms, self.mutant = tuple(bend_terms), mutant

    def joints_cam(self, x78, jaw=None):
        n = x78.shape[0]
        p = body_params_encapsulate_batch(rotrepr.convert_to_3D_rot(x78))
        joint_rot = self.vposer.decode(p["body_pose_vp"], output_type="aa").view(n, -1)
        out = self.body_mesh_model(return_verts=True, body_pose=joint_rot, transl=p["transl"], global_orient=p["global_orient"],
                                   betas=p["betas"], left_hand_pose=p["left_hand_pose"], right_hand_pose=p["right_hand_pose"], jaw_pose=jaw)
        is_joint = self.joint >= 0
        from_joints = out.joints[:, self.joint.clamp(min=0), :]
        from_surface = (out.vertices[:, self.tri, :] * self.bary[None, :, :, None]).sum(2)
        return torch.where(is_joint[None, :, None], from_joints, from_surface) + x78[:, 75:78].unsqueeze(1)

    def extra_prior(self, x78, jaw=None, w_jaw=None, w_bend=0.0):
        """[n]: the jaw prior sum_c (w_jaw[c] jaw[c])^2 and the bending prior w_bend sum_t exp(sign_t aa_{joint_t}[axis_t])^2"""
        out = torch.zeros(x78.shape[0], dtype=self.dtype)
        if jaw is not None and w_jaw is not None:
            out = out + ((torch.as_tensor(w_jaw, dtype=self.dtype) * jaw) ** 2).sum(1)
        if w_bend and self.bend_terms:
            aa = self.vposer.decode(x78[:, 19:51], output_type="aa").view(x78.shape[0], 21, 3)
            if self.mutant == "no_bend":
                aa = aa.detach()
            for j, a, s in self.bend_terms:
                out = out + w_bend * torch.exp(s * aa[:, j - 1, a]) ** 2
        return out

    def frame_loss(self, x78, kp, stage, jaw=None, w_jaw=None, w_bend=0.0):
        w_data, w_pose, w_shape, w_hand = stage
        r2 = (kp[..., :2] - self.project(self.joints_cam(x78, jaw))) ** 2
        data = w_data ** 2 * (kp[..., 2:3] ** 2 * self.rho ** 2 * r2 / (r2 + self.rho ** 2)).sum((1, 2))
        prior = (w_pose ** 2 * (x78[:, 19:51] ** 2).sum(1) + w_shape ** 2 * (x78[:, 9:19] ** 2).sum(1)
                 + w_hand ** 2 * (x78[:, 51:75] ** 2).sum(1))
        return data + prior + self.extra_prior(x78, jaw, w_jaw, w_bend)

    def loss(self, x78, kp, stage, jaw=None, w_jaw=None, w_bend=0.0):
        """(data, prior) summed over the frames, as InnerFitOracle.loss; jaw = None and w_bend = 0: KeypointSpec's values exactly"""
        if jaw is None and not w_bend:
            return super().loss(x78, kp, stage)
        w_data, w_pose, w_shape, w_hand = stage
        r2 = (kp[..., :2] - self.project(self.joints_cam(x78, jaw))) ** 2
        gm = self.rho ** 2 * r2 / (r2 + self.rho ** 2)
        data = w_data ** 2 * torch.sum(kp[..., 2:3] ** 2 * gm)
        prior = (w_pose ** 2 * torch.sum(x78[:, 19:51] ** 2) + w_shape ** 2 * torch.sum(x78[:, 9:19] ** 2)
                 + w_hand ** 2 * torch.sum(x78[:, 51:75] ** 2))
        return data, prior + self.extra_prior(x78, jaw, w_jaw, w_bend).sum()

    def grads(self, x_np, kp_np, stage, jaw_np=None, w_jaw=None, w_bend=0.0):
        """-> (sums [2], d rows [n, 78], d jaw [n, 3] or None) at numpy inputs, in this twin's precision"""
        x = torch.tensor(np.asarray(x_np), dtype=self.dtype, requires_grad=True)
        jaw = None if jaw_np is None else torch.tensor(np.asarray(jaw_np), dtype=self.dtype, requires_grad=True)
        data, prior = self.loss(x, torch.tensor(np.asarray(kp_np), dtype=self.dtype), stage, jaw, w_jaw, w_bend)
        (data + prior).backward()
        gj = None if jaw is None else (torch.zeros_like(jaw) if jaw.grad is None else jaw.grad).numpy().astype(np.float64)
        return np.array([float(data.detach()), float(prior.detach())]), x.grad.numpy().astype(np.float64), gj

    def fitting_face(self, rows75, keypoints, stages, iters_per_stage, jaw_init=None, jaw_prior=None, bend_ratio=0.0):
        """InnerFitOracle.fitting with the jaw (jaw_init [n, 3]; None: fixed at zero) as a second Adam parameter of the same lr and
        step count, jaw_prior [stages][3] and w_bend = bend_ratio x the stage's w_pose -> rows75 [n, 75], jaw [n, 3] or None"""
        x = rotrepr.convert_to_6D_rot(torch.as_tensor(rows75).to(self.dtype)).detach().clone().requires_grad_(True)
        jaw = None if jaw_init is None else torch.as_tensor(jaw_init).to(self.dtype).detach().clone().requires_grad_(True)
        kp = torch.as_tensor(keypoints).to(self.dtype)
        for si, stage in enumerate(stages):
            opt = torch.optim.Adam([x] if jaw is None else [x, jaw], lr=self.lr)
            for _ in range(iters_per_stage):
                opt.zero_grad()
                data, prior = self.loss(x, kp, stage, jaw, None if jaw_prior is None else jaw_prior[si], bend_ratio * stage[1])
                (data + prior).backward()
                opt.step()
        self.x78 = x.detach()
        return rotrepr.convert_to_3D_rot(x).detach(), None if jaw is None else jaw.detach()
