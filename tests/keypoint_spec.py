"""The inner fit's objective on mapped keypoints, as a torch twin (csrc/fdc_keypoints.h): the oracle's 55 joints and vertices, the
mapped points formed from them -- joint j, or bary . vertices[tri] -- and oracle.innerfit.InnerFitOracle's objective, its Adam loop
and its L-BFGS loop evaluated on those points instead of joints 0..22.  Imports the oracle and changes nothing in it; dtype float64
is the yardstick of tests/test_gpu_keypoints.py, float32 the twin its run-to-run bars come from."""
import numpy as np
import torch

from oracle import rotrepr
from oracle.fitting import body_params_encapsulate_batch
from oracle.innerfit import DEFAULT_INTRINSICS, InnerFitOracle
from oracle.smplx import SMPLXOracle
from oracle.vposer import VPoserDecoder

COLUMN_BLOCKS = {"transl": slice(0, 3), "sixd": slice(3, 9), "betas": slice(9, 19), "latent": slice(19, 51), "hands": slice(51, 75),
                 "camt": slice(75, 78)}


class KeypointSpec(InnerFitOracle):
    def __init__(self, bm, vp, joint, tri, bary, intrinsics=DEFAULT_INTRINSICS, rho=100.0, lr=0.01, dtype=torch.float64):
        super().__init__(SMPLXOracle(bm, dtype=dtype), VPoserDecoder.from_data(vp, dtype=dtype), intrinsics, rho, lr, dtype)
        self.joint = torch.as_tensor(np.asarray(joint), dtype=torch.long)
        self.tri = torch.as_tensor(np.asarray(tri), dtype=torch.long)
        self.bary = torch.as_tensor(np.asarray(bary, dtype=np.float32)).to(dtype)      # (the weights the library holds: fp32 values)

    def joints_cam(self, x78):
        """[n, n_kp, 3]: the mapped points in the camera frame (SMPL-X output + transl + camera_translation)."""
        n = x78.shape[0]
        p = body_params_encapsulate_batch(rotrepr.convert_to_3D_rot(x78))
        joint_rot = self.vposer.decode(p["body_pose_vp"], output_type="aa").view(n, -1)
        out = self.body_mesh_model(return_verts=True, body_pose=joint_rot, transl=p["transl"], global_orient=p["global_orient"],
                                   betas=p["betas"], left_hand_pose=p["left_hand_pose"], right_hand_pose=p["right_hand_pose"])
        is_joint = self.joint >= 0
        from_joints = out.joints[:, self.joint.clamp(min=0), :]
        from_surface = (out.vertices[:, self.tri, :] * self.bary[None, :, :, None]).sum(2)
        return torch.where(is_joint[None, :, None], from_joints, from_surface) + x78[:, 75:78].unsqueeze(1)

    def frame_loss(self, x78, kp, stage):
        """the objective per frame [n] (what a per-frame line search sees)"""
        w_data, w_pose, w_shape, w_hand = stage
        r2 = (kp[..., :2] - self.project(self.joints_cam(x78))) ** 2
        data = w_data ** 2 * (kp[..., 2:3] ** 2 * self.rho ** 2 * r2 / (r2 + self.rho ** 2)).sum((1, 2))
        prior = (w_pose ** 2 * (x78[:, 19:51] ** 2).sum(1) + w_shape ** 2 * (x78[:, 9:19] ** 2).sum(1)
                 + w_hand ** 2 * (x78[:, 51:75] ** 2).sum(1))
        return data + prior


def column_errors(got, want):
    """max|got - want| per column block of a [n, 78] array, and the block's max|want|"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return {k: (float(np.abs(got[:, s] - want[:, s]).max()), float(np.abs(want[:, s]).max())) for k, s in COLUMN_BLOCKS.items()}
