"""Restatement of FittingOP (mode='global') -- the hot path this repo accelerates.

TEST INFRASTRUCTURE (see oracle/__init__.py).  Follows /root/reference/global_optimization.py:
  qvec2rotmat :51-61 · extract_ext :208-230 · body2world :191-206 · verts_transform :119-127 ·
  cal_loss :249-312 · init :450-489 · fitting('global') :558-593 · return :632-635 ·
  cal_dctloss :232-246 · fitting('dct') :595-630.
Pinned by tests/golden/*.npz, which the reference's own code produced (tests/golden/make_golden.py).

Deliberate deviations (all no-ops at the reference's N=300):
  * clip length N is free: `avg = sum/300.0` (:465) -> `sum/N`, `np.ones(300)` (:472) -> N;
  * an empty outlier set is allowed (the reference raises IndexError);
  * `cal_dctloss` (:232-246, :310) is evaluated only in mode 'dct': its value never enters a 'global' or
    'local' total; its windows generalise from 5 x 60 frames (:41-42) to N // 60 windows of 60 frames;
  * Ns == 0 / weight_contact == 0 skips the Chamfer term (BASELINE config 1).
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import rotrepr
from .chamfer import chamferDist


def qvec2rotmat(q):
    """global_optimization.py:51-61 (float64 numpy)."""
    return np.array([
        [1 - 2 * q[2] ** 2 - 2 * q[3] ** 2, 2 * q[1] * q[2] - 2 * q[0] * q[3],
         2 * q[3] * q[1] + 2 * q[0] * q[2]],
        [2 * q[1] * q[2] + 2 * q[0] * q[3], 1 - 2 * q[1] ** 2 - 2 * q[3] ** 2,
         2 * q[2] * q[3] - 2 * q[0] * q[1]],
        [2 * q[3] * q[1] - 2 * q[0] * q[2], 2 * q[2] * q[3] + 2 * q[0] * q[1],
         1 - 2 * q[1] ** 2 - 2 * q[2] ** 2]])


def extract_ext(lines, dtype=torch.float32):
    """global_optimization.py:208-230: inv([R(q)|t]) per ' qw qx qy qz tx ty tz' line, computed
    in float64 numpy and cast."""
    out = []
    for line in lines:
        items = line.rstrip("\n").split(" ")
        qvec = np.array([float(items[1]), float(items[2]), float(items[3]), float(items[4])])
        tvec = np.array([float(items[5]), float(items[6]), float(items[7])])
        E = np.eye(4)
        E[:3, 3] = tvec
        E[0:3, 0:3] = qvec2rotmat(qvec)
        out.append(torch.tensor(np.linalg.inv(E), dtype=dtype))
    return torch.stack(out, dim=0)


def verts_transform(verts_batch, cam_ext_batch):
    """global_optimization.py:119-127."""
    homo = F.pad(verts_batch, (0, 1), mode="constant", value=1)
    return torch.matmul(homo, cam_ext_batch.permute(0, 2, 1))[:, :, :-1]


def body_params_encapsulate_batch(body_rec):
    """The method the reference calls (:268) but never defines; slicing per cvae.py:196-201."""
    return {"transl": body_rec[:, 0:3], "global_orient": body_rec[:, 3:6],
            "betas": body_rec[:, 6:16], "body_pose_vp": body_rec[:, 16:48],
            "left_hand_pose": body_rec[:, 48:60], "right_hand_pose": body_rec[:, 60:72]}


def find_outliers_and_sources(x78, dtype=torch.float32):
    """init() :459-487 -> (idx1 outlier rows, pos = nearest inlier row for each)."""
    n = x78.shape[0]
    body_par = rotrepr.convert_to_3D_rot(x78)
    stats = torch.sum(body_par[:, 16:48] ** 2, 1)
    avg = torch.sum(stats) / float(n)
    idx1 = torch.where(stats > avg * 1.8)[0].cpu().numpy()
    temp = np.ones(n)
    temp[idx1] = 0.0
    index_one = np.where(temp == 1)[0]
    index_zero = np.where(temp == 0)[0]
    if index_zero.shape[0] == 0 or index_one.shape[0] == 0:
        return idx1, np.zeros(0, dtype=np.int64)
    w = index_one.shape[0]
    h = index_zero.shape[0]
    io = np.tile(index_one, (h, 1))
    iz = np.tile(index_zero, (w, 1)).T
    pos = np.argmin(np.abs(iz - io), axis=1)
    return idx1, io[0, pos]


class FittingOracle:
    def __init__(self, body_model, vposer, scene_verts, contact_vid, camerapose_lines, num_body,
                 init_lr_h=0.005, num_iter=500, weight_loss_rec=1.0, weight_loss_vposer=0.001,
                 weight_contact=0.1, dtype=torch.float32, legacy_zero_grad=False,
                 one_direction_chamfer=True, phase_split=0.8, dct_mtx=None, c_dct_init=None,
                 phase1_contact=0.1, phase1_smooth=1.0, phase2_world=1.0, phase2_smooth=0.5, scale_init=1.8):
        """phase1_* / phase2_* / scale_init: the constants the reference buries in fitting() (:570, :582) and __init__ (:179), as
        keywords so that the tests can move them off their defaults; the defaults are the reference's."""
        self.dtype = dtype
        self.body_mesh_model = body_model
        self.vposer = vposer
        self.batch_size = self.num_body = num_body
        sv = torch.as_tensor(scene_verts).to(dtype)
        # :175-176 repeats the scene per frame; expand() is the same values without the copy
        self.s_verts_batch = sv.unsqueeze(0).expand(num_body, -1, -1) if sv.shape[0] else None
        self.vid = np.asarray(contact_vid, dtype=np.int64)
        self.camerapose_lines = camerapose_lines
        self.init_lr_h = init_lr_h
        self.num_iter = num_iter
        self.weight_loss_rec = weight_loss_rec
        self.weight_loss_vposer = weight_loss_vposer
        self.weight_contact = weight_contact
        self.legacy_zero_grad = legacy_zero_grad
        self.one_direction_chamfer = one_direction_chamfer
        self.phase_split = phase_split
        self.phase1_contact, self.phase1_smooth = phase1_contact, phase1_smooth
        self.phase2_world, self.phase2_smooth = phase2_world, phase2_smooth
        self.scale = torch.tensor(scale_init, dtype=dtype, requires_grad=True)          # :179
        self.body_rotation_rec = torch.zeros(num_body, 78, dtype=dtype, requires_grad=True)
        self.camera_ext = torch.zeros(num_body, 4, 4, dtype=dtype, requires_grad=True)  # :182
        params = [self.body_rotation_rec, self.scale, self.camera_ext]
        self.dct_mtx = self.c_dct = None
        if dct_mtx is not None:                                                         # :184-186
            self.dct_mtx = torch.as_tensor(dct_mtx).to(dtype)                           # [60, 5]
            self.c_dct = torch.as_tensor(c_dct_init).to(dtype).clone().requires_grad_(True)   # [W, 23, 3, 5]
            params.append(self.c_dct)
        self.optimizer = torch.optim.Adam(params, lr=init_lr_h)                         # :188
        self.loss_log = []

    # :191-206 (the per-frame Python loop builds exactly this matrix)
    def body2world(self):
        cam_t = self.body_rotation_rec[:, -3:] * self.scale
        n = self.num_body
        pose = torch.eye(4, dtype=self.dtype).unsqueeze(0).repeat(n, 1, 1)
        pose = torch.cat([pose[:, :, :3],
                          torch.cat([cam_t, torch.ones(n, 1, dtype=self.dtype)], 1).unsqueeze(-1)], 2)
        return torch.matmul(self.camera_ext, pose)

    def forward_world(self):
        """Shared by cal_loss: world-space vertices and the 23 world joints (:253, :261-285, :298-299)."""
        body2world = self.body2world()
        body_rec = rotrepr.convert_to_3D_rot(self.body_rotation_rec)
        p = body_params_encapsulate_batch(body_rec)
        joint_rot = self.vposer.decode(p["body_pose_vp"], output_type="aa").view(self.batch_size, -1)
        out = self.body_mesh_model(return_verts=True, body_pose=joint_rot,
                                   transl=p["transl"], global_orient=p["global_orient"],
                                   betas=p["betas"], left_hand_pose=p["left_hand_pose"],
                                   right_hand_pose=p["right_hand_pose"])
        verts = verts_transform(out.vertices * self.scale, body2world)
        joints = verts_transform(out.joints[:, 0:23, :], body2world)
        return body_rec, verts, joints

    def cal_loss(self, body_data_rotation, idx1):
        weights = torch.ones(body_data_rotation.size(), dtype=self.dtype)
        weights[idx1, :] = 0.0
        loss_rec = self.weight_loss_rec * torch.mean(
            torch.abs(body_data_rotation - self.body_rotation_rec) * weights)             # :259
        body_rec, verts, joints = self.forward_world()
        loss_vposer = self.weight_loss_vposer * torch.mean(body_rec[:, 16:48] ** 2)        # :263
        diff = self.body_rotation_rec[0:-1, :] - self.body_rotation_rec[1:, :]
        loss_smoothing = torch.mean(torch.abs(diff[0:-1, :] - diff[1:, :]))                # :267
        if self.s_verts_batch is not None and self.weight_contact != 0.0:
            contact = verts[:, self.vid, :]                                                # :290
            d, _ = chamferDist(self.one_direction_chamfer)(contact.contiguous(), self.s_verts_batch)
            r = torch.sqrt(d + 1e-4)
            loss_contact = self.weight_contact * torch.mean(r / (r + 1.0))                 # :295
        else:
            loss_contact = torch.zeros((), dtype=self.dtype)
        loss_world_smoothing = torch.mean(torch.abs(joints[0:-1] - joints[1:]))            # :304
        return loss_rec, loss_vposer, loss_contact, loss_smoothing, loss_world_smoothing

    def cal_dctloss(self, joints):
        """:232-246.  One objective per (joint i, axis j, window k): sum over the window's frames of the
        Geman-McClure residual e/(e+1), e = (trajectory - dct_mtx @ c_dct[k,i,j])^2; mean over objectives."""
        T = self.dct_mtx.shape[0]
        W = self.c_dct.shape[0]
        traj = joints[:T * W].reshape(W, T, 23, 3)
        pred = torch.einsum("tc,kijc->ktij", self.dct_mtx, self.c_dct)
        err = (traj - pred) ** 2
        return torch.mean(torch.sum(err / (err + 1.0), dim=1))

    def step_dct(self, ii, body_data_rotation, idx1):
        """One pass of the :597-630 loop body.  legacy_zero_grad (torch < 2): gradients are zeroed, not dropped, so from
        the 95 % switch on the frozen c_dct keeps a zero gradient and Adam keeps moving it on its moments."""
        self.optimizer.zero_grad(set_to_none=not self.legacy_zero_grad)
        frozen = not (self.body_rotation_rec.requires_grad or self.scale.requires_grad or self.camera_ext.requires_grad)
        if frozen and getattr(self, "_dct_cache", None) is not None:
            # the body / scale / camera leaves are frozen (flags of the previous iteration), so this forward
            # repeats the previous one value for value: reuse it (test-speed only, no arithmetic change)
            l_rec, l_vp, l_sm, l_con, joints = self._dct_cache
        else:
            weights = torch.ones(body_data_rotation.size(), dtype=self.dtype)
            weights[idx1, :] = 0.0
            l_rec = self.weight_loss_rec * torch.mean(torch.abs(body_data_rotation - self.body_rotation_rec) * weights)
            body_rec, verts, joints = self.forward_world()
            l_vp = self.weight_loss_vposer * torch.mean(body_rec[:, 16:48] ** 2)
            diff = self.body_rotation_rec[0:-1, :] - self.body_rotation_rec[1:, :]
            l_sm = torch.mean(torch.abs(diff[0:-1, :] - diff[1:, :]))
            if self.s_verts_batch is not None and self.weight_contact != 0.0:
                d, _ = chamferDist(self.one_direction_chamfer)(verts[:, self.vid, :].contiguous(), self.s_verts_batch)
                r = torch.sqrt(d + 1e-4)
                l_con = self.weight_contact * torch.mean(r / (r + 1.0))
            else:
                l_con = torch.zeros((), dtype=self.dtype)
            self._dct_cache = tuple(v.detach() for v in (l_rec, l_vp, l_sm, l_con, joints)) if frozen else None
        l_dct = self.cal_dctloss(joints)                                                   # :310
        if ii < self.num_iter * 0.95:                                                      # :601
            self.camera_ext.requires_grad = False
            self.scale.requires_grad = False
            self.body_rotation_rec.requires_grad = False
            self.c_dct.requires_grad = True
            loss = l_dct * 10                                                              # :607
        else:
            self.camera_ext.requires_grad = False
            self.scale.requires_grad = True
            self.body_rotation_rec.requires_grad = True
            self.c_dct.requires_grad = False
            loss = l_dct * 0.0001 + l_rec * 0.5 + l_con * 0.1                              # :620
        self.loss_log.append([float(v.detach()) for v in (l_rec, l_vp, l_sm, l_con, l_dct, loss)])
        if loss.requires_grad:
            loss.backward()
        self.optimizer.step()

    def fitting_dct(self, body_data, num_iter=10000):
        """mode='dct' (:595-630): the reference forces num_iter = 10000 (:596)."""
        self.num_iter = num_iter
        body_data_rotation = rotrepr.convert_to_6D_rot(torch.as_tensor(body_data).to(self.dtype))
        idx1 = self.init(body_data_rotation)
        body_data_rotation = body_data_rotation.detach()
        self.idx1 = idx1
        for ii in range(self.num_iter):
            self.step_dct(ii, body_data_rotation, idx1)
        body_rec = rotrepr.convert_to_3D_rot(self.body_rotation_rec)
        return body_rec.detach(), self.scale.detach().cpu().numpy().squeeze(), self.camera_ext.detach()

    def init(self, body_data_rotation):
        self.body_rotation_rec.data = body_data_rotation.clone()                           # :454
        self.camera_ext.data = extract_ext(self.camerapose_lines, self.dtype).clone()      # :455
        idx1, pos = find_outliers_and_sources(body_data_rotation, self.dtype)
        if idx1.shape[0] and pos.shape[0]:
            self.body_rotation_rec.data[idx1, :] = body_data_rotation[pos, :]              # :487
        return idx1

    def step(self, ii, body_data_rotation, idx1):
        """One pass of the :560-593 loop body."""
        self.optimizer.zero_grad(set_to_none=not self.legacy_zero_grad)
        l_rec, l_vp, l_con, l_sm, l_ws = self.cal_loss(body_data_rotation, idx1)
        if ii < self.num_iter * self.phase_split:                                          # :564
            self.camera_ext.requires_grad = False
            self.scale.requires_grad = True
            self.body_rotation_rec.requires_grad = True
            loss = l_con * self.phase1_contact + l_sm * self.phase1_smooth + l_rec         # :570
        else:
            self.camera_ext.requires_grad = True
            self.scale.requires_grad = False
            self.body_rotation_rec.requires_grad = True
            loss = l_rec + l_ws * self.phase2_world + l_sm * self.phase2_smooth            # :582
        self.loss_log.append([float(v.detach()) for v in (l_rec, l_vp, l_sm, l_con, l_ws, loss)])
        loss.backward()
        self.optimizer.step()
        return loss

    # ---- 'local' mode: detect_contact :315-365, cal_loss2 :368-447 ----
    def detect_contact(self, n_left):
        """Per-frame mean Chamfer distance of the left / right leg sets; the reference then returns
        left / (left + left) (:364) -- identically 0.5 (NaN where the distance is 0) -- reproduced as is."""
        with torch.no_grad():
            _, verts, _ = self.forward_world()
            left = verts[:, self.vid[:n_left], :].contiguous()
            right = verts[:, self.vid[n_left:], :].contiguous()
            dl, _ = chamferDist(self.one_direction_chamfer)(left, self.s_verts_batch)
            dr, _ = chamferDist(self.one_direction_chamfer)(right, self.s_verts_batch)
            dl, dr = dl.mean(dim=1), dr.mean(dim=1)
            self.contact_dist_left, self.contact_dist_right = dl, dr
            return (dl / (dl + dl)).detach()

    def cal_loss2(self, body_data_rotation, idx1, contact_weight, n_left):
        weights = torch.ones(body_data_rotation.size(), dtype=self.dtype)
        weights[idx1, :] = 0.0
        loss_rec = self.weight_loss_rec * torch.mean(
            torch.abs(body_data_rotation - self.body_rotation_rec) * weights)             # :376
        diff_local = self.body_rotation_rec[0:-1, :] - self.body_rotation_rec[1:, :]
        loss_local_smoothing = torch.mean(torch.abs(diff_local[0:-1, :] - diff_local[1:, :]))   # :382
        _, verts, _ = self.forward_world()
        diff = verts[0:-1, :] - verts[1:, :]
        loss_smoothing = torch.mean(torch.abs(diff[0:-1, :] - diff[1:, :]))                # :404-405
        cl = verts[:, self.vid[:n_left], :]
        cr = verts[:, self.vid[n_left:], :]
        dleft = cl[0:-1] - cl[1:]
        dright = cr[0:-1] - cr[1:]
        weight_right = contact_weight.clone()
        weight_left = 1 - weight_right
        weight_left[weight_left < 0.5] = 0.0                                                # :421-422
        weight_right[weight_right < 0.5] = 0.0
        wr = weight_right[1:].unsqueeze(1).unsqueeze(1)
        wl = weight_left[1:].unsqueeze(1).unsqueeze(1)
        loss_contact_smoothing = torch.mean(torch.abs(dleft * wl)) + torch.mean(torch.abs(dright * wr))   # :429
        return loss_rec, loss_local_smoothing, loss_smoothing, loss_contact_smoothing

    def step_local_a(self, ii, body_data_rotation, idx1):
        """Phase A of mode 'local' (:501-532): like 'global' but 0.2*contact and no world term."""
        self.optimizer.zero_grad(set_to_none=not self.legacy_zero_grad)
        l_rec, l_vp, l_con, l_sm, l_ws = self.cal_loss(body_data_rotation, idx1)
        if ii < self.num_iter * self.phase_split:
            self.camera_ext.requires_grad = False
            self.scale.requires_grad = True
            self.body_rotation_rec.requires_grad = True
            loss = l_con * 0.2 + l_sm * 1.0 + l_rec                                        # :511
        else:
            self.camera_ext.requires_grad = True
            self.scale.requires_grad = False
            self.body_rotation_rec.requires_grad = True
            loss = l_rec + l_sm * 0.5                                                      # :523
        self.loss_log.append([float(v.detach()) for v in (l_rec, l_vp, l_sm, l_con, l_ws, loss)])
        loss.backward()
        self.optimizer.step()

    def step_local_b(self, body_data_rotation, idx1, contact_weight, n_left):
        """One pass of the second loop of mode 'local' (:536-556)."""
        self.optimizer.zero_grad(set_to_none=not self.legacy_zero_grad)
        l_rec, l_loc, l_sm, l_cs = self.cal_loss2(body_data_rotation, idx1, contact_weight, n_left)
        self.camera_ext.requires_grad = False
        self.scale.requires_grad = False
        self.body_rotation_rec.requires_grad = True
        loss = l_sm * 1.0 + l_loc + l_rec + l_cs                                           # :547
        self.loss_log2.append([float(v.detach()) for v in (l_rec, l_loc, l_sm, l_cs, loss)])
        loss.backward()
        self.optimizer.step()

    def fitting_local(self, body_data, n_left):
        """mode='local' (:499-556).  n_left = number of L_Leg entries at the head of the contact ids."""
        body_data_rotation = rotrepr.convert_to_6D_rot(torch.as_tensor(body_data).to(self.dtype))
        idx1 = self.init(body_data_rotation)
        body_data_rotation = body_data_rotation.detach()
        self.idx1 = idx1
        self.loss_log2 = []
        for ii in range(self.num_iter):
            self.step_local_a(ii, body_data_rotation, idx1)
        self.contact_weight = self.detect_contact(n_left)                                  # :534
        for ii in range(int(0.4 * self.num_iter)):
            self.step_local_b(body_data_rotation, idx1, self.contact_weight, n_left)
        body_rec = rotrepr.convert_to_3D_rot(self.body_rotation_rec)
        return body_rec.detach(), self.scale.detach().cpu().numpy().squeeze(), self.camera_ext.detach()

    def fitting(self, body_data):
        """[N,75] -> (body_rec [N,75], scale ndarray scalar, camera_ext [N,4,4])."""
        body_data_rotation = rotrepr.convert_to_6D_rot(torch.as_tensor(body_data).to(self.dtype))
        idx1 = self.init(body_data_rotation)
        body_data_rotation = body_data_rotation.detach()
        self.idx1 = idx1
        for ii in range(self.num_iter):
            self.step(ii, body_data_rotation, idx1)
        body_rec = rotrepr.convert_to_3D_rot(self.body_rotation_rec)                       # :633
        return body_rec.detach(), self.scale.detach().cpu().numpy().squeeze(), self.camera_ext.detach()


# ---- the reference's per-iteration host loops (bench.py's overhead ablation) ----
def body2world_frame_loop(body_rotation_rec, scale, camera_ext):
    """body2world as the reference writes it (:191-206): one 4x4 per frame built on the host and stacked."""
    cam_t = body_rotation_rec[:, -3:]
    poses = []
    for i in range(body_rotation_rec.shape[0]):
        pose = torch.eye(4, dtype=body_rotation_rec.dtype)
        pose[:3, 3] = cam_t[i, :] * scale
        poses.append(pose)
    return torch.matmul(camera_ext, torch.stack(poses, dim=0))


def cal_dctloss_triple_loop(joints, dct_mtx, c_dct, frames_per_window=60):
    """cal_dctloss as the reference writes it (:232-246): 23 x 3 x W small matrix-vector products."""
    objs = []
    for i in range(23):
        for j in range(3):
            for k in range(c_dct.shape[0]):
                traj = joints[frames_per_window * k:frames_per_window * (k + 1), i, j]
                pred = torch.squeeze(torch.matmul(dct_mtx, torch.unsqueeze(c_dct[k, i, j], -1)))
                err = (traj - pred) ** 2
                objs.append(torch.sum(err / (err + 1.0)))
    return torch.mean(torch.stack(objs))


def reference_host_loop_overhead(n=300, repeats=3, seed=0):
    """Seconds per iteration (forward + backward) of the two host loops every reference iteration runs around a trivial
    stand-in body (joints = the body2world translation), reference style vs the vectorised forms the oracle uses --
    the part of the original's iteration that is Python overhead, not arithmetic (90 ms at N = 300)."""
    import time
    g = torch.Generator().manual_seed(seed)
    W = max(n // 60, 1)
    x = torch.randn(n, 78, generator=g).requires_grad_(True)
    s = torch.tensor(1.8, requires_grad=True)
    cam = torch.eye(4).repeat(n, 1, 1).clone().requires_grad_(True)
    c_dct = torch.randn(W, 23, 3, 5, generator=g).requires_grad_(True)
    D = torch.randn(60, 5, generator=g)
    out = {}
    for name in ("reference_loops", "vectorised"):
        ts = []
        for _ in range(repeats + 1):
            t0 = time.perf_counter()
            if name == "reference_loops":
                b2w = body2world_frame_loop(x, s, cam)
            else:
                pose = torch.eye(4).unsqueeze(0).repeat(n, 1, 1)
                pose = torch.cat([pose[:, :, :3], torch.cat([x[:, -3:] * s, torch.ones(n, 1)], 1).unsqueeze(-1)], 2)
                b2w = torch.matmul(cam, pose)
            joints = b2w[:, :3, 3].unsqueeze(1).expand(-1, 23, -1)
            if n >= 60:
                if name == "reference_loops":
                    l = cal_dctloss_triple_loop(joints, D, c_dct)
                else:
                    traj = joints[:60 * W].reshape(W, 60, 23, 3)
                    err = (traj - torch.einsum("tc,kijc->ktij", D, c_dct)) ** 2
                    l = torch.mean(torch.sum(err / (err + 1.0), dim=1))
            else:
                l = joints.sum()
            l.backward()
            ts.append(time.perf_counter() - t0)
        out[name] = float(np.mean(ts[1:]))
    return out
