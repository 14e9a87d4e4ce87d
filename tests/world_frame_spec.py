"""The inner fit's twins under a world transform other than the identity: a wrapper, not a copy.

`world_frame(cls)` returns a subclass of any of the twins -- oracle.innerfit.InnerFitOracle, tests/keypoint_spec.KeypointSpec,
tests/face_spec.FaceSpec, tests/expression_spec.ExpressionSpec, the FaceCollisionSpec of tests/face_mesh_spec.fit_spec and the
CollisionFitSpec of tests/collision_spec.fit_spec -- whose `joints_cam` (and `world_vertices`) applies the clip-level loop's transform,
restated from oracle/fitting.py (body2world, forward_world).  With R, t the rotation and translation of a frame's camera_ext and
s = scale:

    surface points (and the joints 23..54, which the keypoint kernel forms as pseudo-vertices)    R s (v + transl + cam_t) + t
    joints 0..22                                                                                 R ((J + transl) + s cam_t) + t

The wrapped class is asked for its points at cam_t = 0 (the body's own points, p), and the transform is ONE torch.autograd.Function
around them, written in the terms the kernels use -- M = [R | R s cam_t + t], the per-frame sums dM [3 x 4] and d scale of the vertices,
then d camera_ext, d cam_t and d scale from them (csrc/fdc_skin.h skin_backward_vertex, csrc/fdc_frame.h pose_backward) -- so that a
MUTANT is that backward with one deliberate defect; tests/test_world_frame_cpu.py shows that the Function without a mutant is plain
autograd's gradient of the formulas above and that every mutant leaves a bar of tests/test_gpu_world_frame.py.  At the identity and
s = 1 the forward multiplies by exact ones and adds exact zeros: the wrapped class's bits.

Imports the twins and the oracle and changes nothing in them.  `cameras` and `check_inputs` are the input rules of the GPU test, run on
the CPU by both files."""
import numpy as np
import torch

NJW = 23                                    # joints 0..22: the world joints (csrc/fdc_frame.h world_joint)
TARGET = (0.1, -0.2, 3.5)                   # where the pelvis lands in front of the projection
MUTANTS = ("joints_R", "verts_R", "expr_R", "gv_no_s", "ds_no_rot", "dM_vb", "dM_no_transl", "dcamt_no_s", "next_frame", "dM_no_expr")
ROTATION_MUTANTS = ("joints_R", "verts_R", "expr_R")          # R for R^T: invisible at W = I
SCALE_MUTANTS = ("gv_no_s", "ds_no_rot", "dM_vb", "dcamt_no_s")     # a factor s, or the scale's own gradient: invisible at s = 1


class _WorldTransform(torch.autograd.Function):
    """p [n, K, 3] the body's points without cam_t, camt [n, 3], cams [n, 4, 4], s [] -> world points [n, K, 3]; is_joint [K] bool."""

    @staticmethod
    def forward(ctx, p, camt, cams, s, is_joint, mutant):
        R, t = cams[:, :3, :3], cams[:, :3, 3]
        body = torch.where(is_joint[None, :, None], p + s * camt[:, None], s * (p + camt[:, None]))
        ctx.save_for_backward(p, camt, cams, s, is_joint)
        ctx.mutant = mutant
        return torch.matmul(body, R.transpose(1, 2)) + t[:, None]

    @staticmethod
    def backward(ctx, g):
        p, camt, cams, s, is_joint = ctx.saved_tensors
        m = ctx.mutant
        R = cams[:, :3, :3]
        if m == "next_frame":                               # frame f's camera used for frame f + 1
            R = torch.roll(R, 1, 0)
        Rt = R.transpose(1, 2)
        J = is_joint[None, :, None]
        zero = torch.zeros_like(g)
        gj, gv = torch.where(J, g, zero), torch.where(J, zero, g)
        # x R = R^T x per point (rows): back through the rotation
        rtj = torch.matmul(gj, Rt if m == "joints_R" else R)
        rtv = torch.matmul(gv, Rt if m == "verts_R" else R)
        gp = rtj + (rtv if m == "gv_no_s" else s * rtv)      # skin_backward_vertex's gv; the world joints' W^T dJw
        # the vertices' per-frame sums (the keypoint kernel's sixteen, skin_bwd's): dM [3 x 4] with vb = p, d scale
        dMR = torch.einsum("nki,nkc->nic", gv, p if m == "dM_vb" else s * p) + torch.einsum("nki,nkc->nic", gj, p)
        dMt = gj.sum(1) if m == "dM_no_transl" else g.sum(1)
        dsv = (gv * p).sum() if m == "ds_no_rot" else (torch.matmul(gv, R) * p).sum()
        # pose_backward: M.t = E.R (s ct) + E.t
        q = torch.matmul(dMt[:, None], R)[:, 0]
        dcams = torch.zeros_like(cams)
        dcams[:, :3, :3] = dMR + torch.einsum("ni,nc->nic", dMt, s * camt)
        dcams[:, :3, 3] = dMt
        dcamt = q if m == "dcamt_no_s" else s * q
        ds = dsv + (q * camt).sum()
        return gp, dcamt, dcams, ds, None, None


def plain_transform(p, camt, cams, s, is_joint):
    """the two formulas as plain torch operations (autograd's own backward): what _WorldTransform is checked against"""
    R, t = cams[:, :3, :3], cams[:, :3, 3]
    rot = lambda v: torch.einsum("nic,nkc->nki", R, v) + t[:, None]
    return torch.where(is_joint[None, :, None], rot(p + s * camt[:, None]), rot(s * (p + camt[:, None])))


def loss_grads(twin, x_np, kp_np, stage):
    """(sums [2], d rows [n, 78]) of a twin without a grads helper of its own (InnerFitOracle, KeypointSpec), in its precision"""
    x = torch.tensor(np.asarray(x_np), dtype=twin.dtype, requires_grad=True)
    data, prior = twin.loss(x, torch.tensor(np.asarray(kp_np), dtype=twin.dtype), stage)
    (data + prior).backward()
    return np.array([float(data.detach()), float(prior.detach())]), x.grad.numpy().astype(np.float64)


def world_frame(cls):
    """-> a subclass of the twin `cls` under the cameras and scale of set_world()"""

    class WorldFrame(cls):
        cams = scale = world_mutant = None

        def set_world(self, cams, scale=1.0, mutant=None):
            """cams [n, 4, 4] or [n, 16] (row-major camera_ext) and scale, held as tensors of the twin's dtype; mutant: one of MUTANTS"""
            assert mutant is None or mutant in MUTANTS
            self.cams = torch.as_tensor(np.asarray(cams)).to(self.dtype).reshape(-1, 4, 4).clone()
            self.scale = torch.tensor(float(scale), dtype=self.dtype)
            self.world_mutant = mutant
            return self

        def _kinds(self, k):
            joint = getattr(self, "joint", None)
            if joint is None:                                 # InnerFitOracle: joints 0..22
                return torch.ones(k, dtype=torch.bool)
            return (joint >= 0) & (joint < NJW)

        def _to_world(self, points_of, x78, face, surface_only):
            n = x78.shape[0]
            assert self.cams is not None and self.cams.shape[0] == n, "set_world() with one camera per frame first"
            camt = x78[:, 75:78]
            at_zero = lambda x: torch.cat([x[:, :75], torch.zeros_like(x[:, 75:78])], dim=1)
            p = points_of(at_zero(x78), *face)
            is_joint = torch.zeros(p.shape[1], dtype=torch.bool) if surface_only else self._kinds(p.shape[1])
            m = self.world_mutant
            if m == "dM_no_expr":
                # the defect the GPU test found in the kernels: d camera_ext's rotation part formed from joints 0..22 WITHOUT the expression
                # correction Dt_j (sum_j dJw_j (x) Dt_j missing -- also what zeroing dMv after the keypoint kernel wrote it gives).  The
                # values and every other gradient are the true ones: a - b is an exact zero whose only gradient is the cameras', through
                # the joints at psi = 0.  WARNING for the next reader: keep the two applications identical but for cams.detach().
                w = _WorldTransform.apply(p, camt, self.cams.detach(), self.scale, is_joint, None)
                if surface_only or len(face) < 2 or face[1] is None:
                    return _WorldTransform.apply(p, camt, self.cams, self.scale, is_joint, None)
                p0 = points_of(at_zero(x78), *[torch.zeros_like(v) if i == 1 else v for i, v in enumerate(face)])
                pj = torch.where(is_joint[None, :, None], p0, p)
                a = _WorldTransform.apply(pj, camt, self.cams, self.scale, is_joint, None)
                b = _WorldTransform.apply(pj, camt, self.cams.detach(), self.scale, is_joint, None)
                return w + (a - b)
            if m != "expr_R":
                return _WorldTransform.apply(p, camt, self.cams, self.scale, is_joint, m)
            # WARNING for the next reader: intricate on purpose -- values must stay w's bits (wp - wp.detach() is an exact zero) and only
            # d psi may pass through the defective backward; a change to the order of `face` (jaw, psi) breaks it silently.
            # the expression correction's joint addend alone: the same values once more with psi as the only variable, sent through
            # the defective backward on the joints' path; the first pass holds psi fixed
            w = _WorldTransform.apply(points_of(at_zero(x78), *[v if i != 1 or v is None else v.detach() for i, v in enumerate(face)]), camt, self.cams,
                                      self.scale, is_joint, None)
            if len(face) < 2 or face[1] is None:
                return w
            fixed = [v if i == 1 or v is None else v.detach() for i, v in enumerate(face)]
            wp = _WorldTransform.apply(points_of(at_zero(x78.detach()), *fixed), camt.detach(), self.cams.detach(), self.scale.detach(), is_joint, "joints_R")
            return w + (wp - wp.detach())

        def joints_cam(self, x78, *face, **kw):
            face = face + tuple(kw[k] for k in ("jaw", "expr")[len(face):] if k in kw)
            return self._to_world(super().joints_cam, x78, face, False)

        def world_vertices(self, x78, *face, **kw):
            face = face + tuple(kw[k] for k in ("jaw", "expr")[len(face):] if k in kw)
            return self._to_world(super().world_vertices, x78, face, True)

        def _free_world(self, call):
            """run `call` (which ends in backward()) with the cameras and the scale as leaves -> its result, d cams [n, 16], d scale"""
            cams, scale = self.cams, self.scale
            self.cams, self.scale = cams.detach().clone().requires_grad_(True), scale.detach().clone().requires_grad_(True)
            try:
                out = call()
                g = lambda v: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().astype(np.float64)
                return out, g(self.cams).reshape(-1, 16), float(g(self.scale))
            finally:
                self.cams, self.scale = cams, scale

        def grads(self, x_np, kp_np, stage, *a, **kw):
            """the wrapped class's grads (InnerFitOracle, KeypointSpec: (sums [2], d rows [n, 78])) and d cams [n, 16] next to them;
            d scale stays in self.last_dscale"""
            if hasattr(super(), "grads"):
                call = lambda: super(WorldFrame, self).grads(x_np, kp_np, stage, *a, **kw)
            else:
                call = lambda: loss_grads(self, x_np, kp_np, stage)
            out, dcams, self.last_dscale = self._free_world(call)
            return tuple(out) + (dcams,)

        def grads_coll(self, *a, **kw):
            out, dcams, self.last_dscale = self._free_world(lambda: super(WorldFrame, self).grads_coll(*a, **kw))
            return tuple(out) + (dcams,)

        def positions(self, x_np, *face):
            t = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=self.dtype)
            with torch.no_grad():
                return self.joints_cam(t(x_np), *[t(v) for v in face]).numpy()

    WorldFrame.__name__ = "World" + cls.__name__
    return WorldFrame


# ---- the input rules ------------------------------------------------------------------------------------------------------------------
def rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def cameras(pelvis, cam_t, scale, seed, identity_frames=(), dtype=np.float32):
    """pelvis [n, 3] (J0 + transl, without cam_t) and cam_t [n, 3] at the state the test evaluates -> camera_ext [n, 4, 4], fp32 values: per
    frame its own rotation by 0.5 .. 2.5 rad about an axis with no component below 1 / 3 in size, and the t that puts the pelvis --
    R (pelvis + s cam_t) + t -- at TARGET + 5 cm of noise.  identity_frames keep the identity."""
    rng = np.random.Generator(np.random.PCG64(9000 + seed))
    n = pelvis.shape[0]
    out = np.tile(np.eye(4), (n, 1, 1))
    for f in range(n):
        axis = rng.choice([-1.0, 1.0], 3) * rng.uniform(0.5, 1.0, 3)
        R = rodrigues(axis, rng.uniform(0.5, 2.5))
        t = np.asarray(TARGET) + 0.05 * rng.standard_normal(3) - R @ (np.asarray(pelvis[f], dtype=np.float64) + scale * np.asarray(cam_t[f], dtype=np.float64))
        if f not in identity_frames:
            out[f, :3, :3], out[f, :3, 3] = R, t
    return out.astype(dtype)


def rotation_angle_axis(R):
    R = np.asarray(R, dtype=np.float64)
    angle = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return angle, w / max(np.linalg.norm(w), 1e-300)


def check_inputs(cams, world_points, residuals, conf, rho, identity_frames=()):
    """The conditions of a case, asserted before anything is compared: cams [n, 4, 4]; world_points [n, K, 3] and residuals [n, K, 2]
    (pixels) the fp64 twin's at the state evaluated; conf [n, K].  Every frame has its own camera, a rigid one; off the
    identity_frames its angle lies in 0.5 .. 2.5 rad about an axis with no component below 0.3; every mapped point stands at
    Z >= 1 m; and the detected keypoints' residuals lie on both sides of GMoF's bend under either reading of it -- some below
    rho / sqrt(3), where rho^2 r^2 / (r^2 + rho^2) turns from convex to concave, and some above rho itself."""
    cams = np.asarray(cams, dtype=np.float64).reshape(-1, 4, 4)
    n = cams.shape[0]
    for f in range(n):
        R = cams[f, :3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6 and np.array_equal(cams[f, 3], [0, 0, 0, 1])
        if f in identity_frames:
            assert np.array_equal(cams[f], np.eye(4))
            continue
        angle, axis = rotation_angle_axis(R)
        assert 0.5 <= angle <= 2.5 and np.abs(axis).min() >= 0.3, (f, angle, axis)
        assert np.abs(R - R.T).max() > 0.2                   # far from symmetric
    moved = [f for f in range(n) if f not in identity_frames]
    assert len({cams[f].tobytes() for f in moved}) == len(moved)
    assert np.asarray(world_points)[..., 2].min() >= 1.0, float(np.asarray(world_points)[..., 2].min())
    r = np.abs(np.asarray(residuals))[np.asarray(conf) > 0]
    assert r.size and r.min() < rho / np.sqrt(3.0) and r.max() > rho, (float(r.min()), float(r.max()))
