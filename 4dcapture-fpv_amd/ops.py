"""Drop-in operators with the call signatures of the three third-party ops on the reference's
hot path, backed by libfdcap_hip.so:

  Op 1  chamferDist()(xyz1, xyz2) -> (dist1, dist2)          global_optimization.py:292-294
  Op 2  body_model(return_verts=True, body_pose=..., ...)    global_optimization.py:280-283
  Op 3  vposer.decode(z, output_type='aa')                   global_optimization.py:270-271

They exist so reference-style code (and the parity tests, which read like the reference's call
sites) can call the HIP kernels one operator at a time, keeping its own loop, torch.optim.Adam and
`loss.backward()` (:591): all three are torch.autograd.Functions over the C-ABI's forward / backward
pairs.  The optimiser itself (fitting.py) uses the fused iteration and never goes through autograd.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from . import capi


def _ctx_of(obj):
    if isinstance(obj, capi.Context):
        return obj
    return obj.ctx


def _is_registered_scene(fctx, x2, memo, memoise=True):
    """Does the [m,3] device tensor x2 hold exactly the points registered with fctx.set_scene?  Compared ON THE DEVICE and
    remembered in `memo` -- the caller's loop passes the same tensor every iteration (:176, :293).  The remembered verdict is
    tied to everything it depends on: the context's scene GENERATION (Context.set_scene bumps it: a re-registered scene of the
    same size is looked at again), the tensor's storage address + offset + version (any in-place write bumps the version), and
    the memo holds a strong reference to the compared tensor, so its storage cannot be freed and handed to another point set at
    the same address while the verdict is alive.  `memoise=False` (a temporary the caller made, e.g. by .contiguous()): compared
    on every call, never remembered."""
    host = getattr(fctx, "_scene_host", None)
    if host is None or tuple(x2.shape) != tuple(host.shape):
        return False
    if getattr(fctx, "_scene_dev", None) is None or fctx._scene_dev.device != x2.device:
        fctx._scene_dev = torch.from_numpy(host).to(x2.device)
    if not memoise:
        return bool(torch.equal(x2, fctx._scene_dev))
    key = (getattr(fctx, "_scene_gen", 0), x2.untyped_storage().data_ptr(), x2.storage_offset(), x2._version, x2.device)
    if memo.get("key") != key:
        memo["key"], memo["same"], memo["tensor"] = key, bool(torch.equal(x2, fctx._scene_dev)), x2
    return memo["same"]


class _ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, fctx, both, memo):
        B, n, _ = xyz1.shape
        m = xyz2.shape[1]
        shared = xyz2.stride(0) == 0 or xyz2.shape[0] == 1
        x1 = xyz1.contiguous()
        x2v = xyz2[0] if shared else xyz2
        x2 = x2v.contiguous()                                # (a view of the caller's storage when x2v is contiguous, else a temporary)
        stride2 = 0 if shared else m * 3
        dev = x1.device
        d1 = torch.empty(B, n, device=dev)
        i1 = torch.empty(B, n, device=dev, dtype=torch.int32)
        d2 = torch.zeros(B, m, device=dev) if both else None
        i2 = torch.zeros(B, m, device=dev, dtype=torch.int32) if both else None
        # the shared target IS the registered scene: body -> scene through the optimiser loop's culled, seeded search (same bits)
        scene = memo is not None and shared and _is_registered_scene(fctx, x2, memo, memoise=x2v.is_contiguous())
        if scene:
            capi.check(fctx.lib.fdcap_chamfer_fwd_scene(fctx.handle, capi.dptr(x1), B, n, capi.dptr(d1), capi.dptr(i1), 0,
                                                        capi.current_stream()), "fdcap_chamfer_fwd_scene")
        if not scene or both:
            capi.check(fctx.lib.fdcap_chamfer_fwd(fctx.handle, capi.dptr(x1), capi.dptr(x2), B, n, m, stride2,
                                                  None if scene else capi.dptr(d1), None if scene else capi.dptr(i1),
                                                  capi.dptr(d2), capi.dptr(i2), capi.current_stream()), "fdcap_chamfer_fwd")
        ctx.fctx, ctx.shared, ctx.both, ctx.scene = fctx, shared, both, scene
        ctx.reduce2 = xyz2.shape[0] == 1              # a [1,m,3] target gets a [1,m,3] gradient; an expand()ed view [B,m,3]
        ctx.save_for_backward(x1, x2, i1, i2 if both else i1)
        ctx.mark_non_differentiable(i1)
        if both:
            return d1, d2, i1
        return d1, torch.zeros(B, m, device=dev), i1

    @staticmethod
    def backward(ctx, g1, g2, _gi):
        x1, x2, i1, i2 = ctx.saved_tensors
        B, n, _ = x1.shape
        m = x2.shape[-2]
        fctx = ctx.fctx
        g1 = g1.contiguous()
        need2 = ctx.needs_input_grad[1]
        if ctx.both or need2:
            # the whole backward -- the target's gradient, the dist2 half -- by the library, in a defined order (reproducible bits)
            gx1 = torch.empty_like(x1) if ctx.needs_input_grad[0] else None
            gx2 = None
            if need2:
                gx2 = torch.empty((1, m, 3) if ctx.reduce2 else (B, m, 3), device=x1.device)
            g2 = g2.contiguous() if ctx.both else None
            capi.check(fctx.lib.fdcap_chamfer_bwd_both(fctx.handle, capi.dptr(x1), capi.dptr(x2), B, n, m, 0 if ctx.shared else m * 3,
                                                       capi.dptr(g1), capi.dptr(i1), capi.dptr(g2), capi.dptr(i2) if ctx.both else None,
                                                       capi.dptr(gx1), capi.dptr(gx2), 1 if (need2 and ctx.reduce2) else 0,
                                                       capi.current_stream()), "fdcap_chamfer_bwd_both")
            return gx1, gx2, None, None, None
        gx1 = torch.empty_like(x1)
        if ctx.scene:
            capi.check(fctx.lib.fdcap_chamfer_bwd_scene(fctx.handle, capi.dptr(x1), B, n, capi.dptr(g1), capi.dptr(i1),
                                                        capi.dptr(gx1), capi.current_stream()), "fdcap_chamfer_bwd_scene")
        else:
            capi.check(fctx.lib.fdcap_chamfer_bwd(fctx.handle, capi.dptr(x1), capi.dptr(x2), B, n, m,
                                                  0 if ctx.shared else m * 3, capi.dptr(g1),
                                                  capi.dptr(i1), capi.dptr(gx1), capi.current_stream()),
                       "fdcap_chamfer_bwd")
        return gx1, None, None, None, None


class chamferDist(torch.nn.Module):
    """`chamferDist(ctx)()`-style module: forward(xyz1[B,n,3], xyz2[B,m,3]) -> (dist1, dist2),
    squared distances.  `both=False` skips the scene->body half the reference discards (dist2 is
    returned as zeros).  xyz2 may be an expand()ed [1,m,3] scene: it is then read once.

    Differentiable with respect to BOTH inputs through both halves, by kernels of the library alone (fdcap_chamfer_bwd_both: terms
    summed in a defined order, so two backward passes give the same bits).  A target passed as [1,m,3] gets its gradient as
    [1,m,3], summed over the batch inside the kernel; an expand()ed view gets [B,m,3], the shape autograd asks for.  A loop that
    needs only the query-side gradient of dist1 (`both=False`, target without grad) stays on fdcap_chamfer_bwd[_scene]."""

    def __init__(self, ctx, both: bool = True, use_registered_scene: bool = True):
        """use_registered_scene: when xyz2 is one shared point set that equals the scene registered on the context
        (Context.set_scene), dist1 comes from the optimiser loop's culled, seeded search instead of the every-pair scan --
        the same values and indices bit for bit, found ~two orders of magnitude faster at scene sizes.  False: always the
        generic scan (what a foreign target gets)."""
        super().__init__()
        self.fctx = _ctx_of(ctx)
        self.both = both
        self.last_idx1 = None
        self._memo = {} if use_registered_scene else None

    def forward(self, input1, input2):
        d1, d2, i1 = _ChamferFn.apply(input1, input2, self.fctx, self.both, self._memo)
        self.last_idx1 = i1
        return d1, d2


class _VPoserFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, fctx, want_aa):
        B = z.shape[0]
        rot = torch.empty(B, 21, 9, device=z.device)
        aa = torch.empty(B, 63, device=z.device) if want_aa else None
        capi.check(fctx.lib.fdcap_vposer_decode(fctx.handle, capi.dptr(z), z.stride(0), B, capi.dptr(rot), capi.dptr(aa),
                                                capi.current_stream()), "fdcap_vposer_decode")
        ctx.fctx, ctx.want_aa = fctx, want_aa
        ctx.save_for_backward(z)
        return aa if want_aa else rot

    @staticmethod
    def backward(ctx, g):
        (z,) = ctx.saved_tensors
        B = z.shape[0]
        g = g.contiguous().float()
        gz = torch.empty(B, 32, device=z.device)
        fctx = ctx.fctx
        capi.check(fctx.lib.fdcap_vposer_decode_bwd(fctx.handle, capi.dptr(z), z.stride(0), B,
                                                    None if ctx.want_aa else capi.dptr(g), capi.dptr(g) if ctx.want_aa else None,
                                                    capi.dptr(gz), capi.current_stream()), "fdcap_vposer_decode_bwd")
        return gz, None, None


class VPoser:
    """Decoder half of VPoser v1.0 with the reference's call: decode(z, output_type='aa'); differentiable."""

    def __init__(self, ctx):
        self.fctx = _ctx_of(ctx)

    def decode(self, Zin, output_type="matrot"):
        z = Zin.reshape(-1, 32).float().contiguous()
        B = z.shape[0]
        out = _VPoserFn.apply(z, self.fctx, output_type == "aa")
        if output_type == "aa":
            return out.view(B, 1, 21, 3)
        return out.view(B, 1, 21, 9)

    def to(self, *a, **k):
        return self

    def eval(self):
        return self


class _BodyModelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, go, bp, be, lh, rh, tr, fctx, return_verts):
        B, dev = bp.shape[0], bp.device
        V = fctx.num_verts
        verts = torch.empty(B, V, 3, device=dev) if return_verts else None
        joints = torch.empty(B, 55, 3, device=dev)
        capi.check(fctx.lib.fdcap_smplx_forward(fctx.handle, capi.dptr(go), capi.dptr(bp), capi.dptr(be), capi.dptr(lh),
                                                capi.dptr(rh), capi.dptr(tr), B, capi.dptr(verts), capi.dptr(joints),
                                                capi.current_stream()), "fdcap_smplx_forward")
        ctx.fctx, ctx.return_verts = fctx, return_verts
        ctx.save_for_backward(go, bp, be, lh, rh, tr)
        if return_verts:
            return verts, joints
        return torch.zeros(0, device=dev), joints

    @staticmethod
    def backward(ctx, gv, gj):
        go, bp, be, lh, rh, tr = ctx.saved_tensors
        fctx = ctx.fctx
        B = bp.shape[0]
        gv = gv.contiguous().float() if (ctx.return_verts and gv is not None) else None
        gj = gj.contiguous().float() if gj is not None else None
        if gv is None and gj is None:
            return (None,) * 8
        outs = [torch.empty_like(t) if need else None for t, need in zip((go, bp, be, lh, rh, tr), ctx.needs_input_grad[:6])]
        capi.check(fctx.lib.fdcap_smplx_backward(fctx.handle, capi.dptr(go), capi.dptr(bp), capi.dptr(be), capi.dptr(lh),
                                                 capi.dptr(rh), capi.dptr(tr), B, capi.dptr(gv), capi.dptr(gj),
                                                 *[capi.dptr(o) for o in outs], capi.current_stream()), "fdcap_smplx_backward")
        return (*outs, None, None)


class _BodyModelFaceFn(torch.autograd.Function):
    """_BodyModelFn with the fitted face: jaw_pose [B,3] and / or expression [B,10] (either may be None, not both), through
    fdcap_smplx_forward_face / fdcap_smplx_backward_face."""

    @staticmethod
    def forward(ctx, go, bp, be, lh, rh, tr, jaw, expr, fctx, return_verts):
        B, dev = bp.shape[0], bp.device
        V = fctx.num_verts
        verts = torch.empty(B, V, 3, device=dev) if return_verts else None
        joints = torch.empty(B, 55, 3, device=dev)
        capi.check(fctx.lib.fdcap_smplx_forward_face(fctx.handle, capi.dptr(go), capi.dptr(bp), capi.dptr(be), capi.dptr(lh),
                                                     capi.dptr(rh), capi.dptr(tr), B, capi.dptr(jaw), capi.dptr(expr), capi.dptr(verts),
                                                     capi.dptr(joints), capi.current_stream()), "fdcap_smplx_forward_face")
        ctx.fctx, ctx.return_verts, ctx.has = fctx, return_verts, (jaw is not None, expr is not None)
        ctx.save_for_backward(go, bp, be, lh, rh, tr, *[t for t in (jaw, expr) if t is not None])
        if return_verts:
            return verts, joints
        return torch.zeros(0, device=dev), joints

    @staticmethod
    def backward(ctx, gv, gj):
        go, bp, be, lh, rh, tr, *face = ctx.saved_tensors
        jaw = face.pop(0) if ctx.has[0] else None
        expr = face.pop(0) if ctx.has[1] else None
        fctx = ctx.fctx
        B = bp.shape[0]
        gv = gv.contiguous().float() if (ctx.return_verts and gv is not None) else None
        gj = gj.contiguous().float() if gj is not None else None
        if gv is None and gj is None:
            return (None,) * 10
        ins = (go, bp, be, lh, rh, tr, jaw, expr)
        outs = [torch.empty_like(t) if (t is not None and need) else None for t, need in zip(ins, ctx.needs_input_grad[:8])]
        capi.check(fctx.lib.fdcap_smplx_backward_face(fctx.handle, capi.dptr(go), capi.dptr(bp), capi.dptr(be), capi.dptr(lh),
                                                      capi.dptr(rh), capi.dptr(tr), B, capi.dptr(jaw), capi.dptr(expr), capi.dptr(gv),
                                                      capi.dptr(gj), *[capi.dptr(o) for o in outs], capi.current_stream()),
                   "fdcap_smplx_backward_face")
        return (*outs, None, None)


class BodyModel:
    """smplx.create(..., model_type='smplx', num_pca_comps=12) stand-in, differentiable with respect to all six inputs and -- when
    given -- `jaw_pose` [B,3] (joint 22's axis-angle) and `expression` [B,10] (shapedirs' columns 10..19): the two keys the inner fit
    writes (io.load_body_face).  `joints` holds the 55 posed joints (the reference reads [:, 0:23])."""

    def __init__(self, ctx):
        self.fctx = _ctx_of(ctx)

    def __call__(self, return_verts=True, body_pose=None, transl=None, global_orient=None, betas=None,
                 left_hand_pose=None, right_hand_pose=None, jaw_pose=None, expression=None, **unused):
        given = [t for t in (body_pose, transl, global_orient, betas, left_hand_pose, right_hand_pose, jaw_pose, expression) if t is not None]
        if not given:
            raise capi.FdcapError("BodyModel: at least one argument must be given (the batch size and the device are read from it)")
        B, dev = given[0].shape[0], given[0].device                 # (body_pose = None is the rest pose, like every other argument)
        c = lambda t, w: (torch.zeros(B, w, device=dev) if t is None else t.reshape(B, w).float().contiguous())
        go, bp, be = c(global_orient, 3), c(body_pose, 63), c(betas, 10)
        lh, rh, tr = c(left_hand_pose, 12), c(right_hand_pose, 12), c(transl, 3)
        if jaw_pose is None and expression is None:
            verts, joints = _BodyModelFn.apply(go, bp, be, lh, rh, tr, self.fctx, bool(return_verts))
        else:
            jaw = None if jaw_pose is None else c(jaw_pose, 3)
            expr = None if expression is None else c(expression, 10)
            verts, joints = _BodyModelFaceFn.apply(go, bp, be, lh, rh, tr, jaw, expr, self.fctx, bool(return_verts))
        return SimpleNamespace(vertices=verts if return_verts else None, joints=joints)

    def to(self, *a, **k):
        return self


class _SelfCollisionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, fctx, sigma, weight, capacity, every_pair):
        n, V, _ = verts.shape
        v = verts.contiguous()
        dev = v.device
        pairs = torch.empty(n, capacity, 2, device=dev, dtype=torch.int32)
        count = torch.empty(n, device=dev, dtype=torch.int32)
        loss = torch.empty(n, device=dev)
        grad = torch.empty_like(v) if verts.requires_grad else None
        prm = capi.CollisionParams(sigma, weight, capacity, 1 if every_pair else 0)
        capi.check(fctx.lib.fdcap_collision_eval(fctx.handle, capi.dptr(v), n, prm, capi.dptr(pairs), capi.dptr(count), capi.dptr(loss),
                                                 capi.dptr(grad), capi.current_stream()), "fdcap_collision_eval")
        ctx.grad = grad
        ctx.mark_non_differentiable(pairs, count)
        return loss, pairs, count

    @staticmethod
    def backward(ctx, g, _gp, _gc):
        return ctx.grad * g.reshape(-1, 1, 1), None, None, None, None, None


class SelfCollision(torch.nn.Module):
    """Self-interpenetration of the context's registered mesh (Context.set_collision_mesh): forward(verts [n,V,3]) -> the per-frame
    penalty [n]; differentiable with respect to `verts` (the total derivative, computed with the forward by the library in a defined
    order, so two calls give the same bits).  last_pairs [n,capacity,2] (registered face ids, -1 behind a frame's kept pairs) and
    last_count [n] (pairs FOUND: above `capacity` the list overflowed) are the last call's.  `every_pair`: the tree-less checker."""

    def __init__(self, ctx, sigma: float = 0.5, weight: float = 1.0, capacity: int = 4096, every_pair: bool = False):
        super().__init__()
        self.fctx = _ctx_of(ctx)
        if not (0.0 < sigma < 1.0) or not (weight >= 0.0 and np.isfinite(weight)) or capacity <= 0:
            raise capi.FdcapError("SelfCollision: sigma in (0, 1), a finite weight >= 0 and capacity > 0")
        self.sigma, self.weight, self.capacity, self.every_pair = float(sigma), float(weight), int(capacity), bool(every_pair)
        self.last_pairs = self.last_count = None

    def forward(self, verts):
        if verts.dim() != 3 or verts.shape[1] != self.fctx.num_verts or verts.shape[2] != 3 or verts.dtype != torch.float32:
            raise capi.FdcapError(f"SelfCollision: verts must be float32 [n, {self.fctx.num_verts}, 3]")
        loss, self.last_pairs, self.last_count = _SelfCollisionFn.apply(verts, self.fctx, self.sigma, self.weight, self.capacity, self.every_pair)
        return loss


def _face_rows(t, B, w, dev, name):
    if t is None:
        return None
    t = torch.as_tensor(t, dtype=torch.float32, device=dev).reshape(-1, w).contiguous()
    if t.shape[0] != B:
        raise capi.FdcapError(f"{name} must be [{B}, {w}]")
    return t


def body_forward_from_params(ctx, params75: torch.Tensor, want_vertices=True, jaw_pose=None, expression=None):
    """[B,75] SMPLify-X rows -> (vertices [B,V,3], joints [B,55,3]) through VPoser + SMPL-X in one
    call (what global_vis.py:131-146 does per frame on the CPU).  jaw_pose [B,3] / expression [B,10]: the fitted face
    (io.load_body_face); None each: the jaw shut, psi = 0."""
    fctx = _ctx_of(ctx)
    p = params75.float().contiguous()
    B = p.shape[0]
    verts = torch.empty(B, fctx.num_verts, 3, device=p.device) if want_vertices else None
    joints = torch.empty(B, 55, 3, device=p.device)
    jaw, expr = _face_rows(jaw_pose, B, 3, p.device, "jaw_pose"), _face_rows(expression, B, 10, p.device, "expression")
    if jaw is None and expr is None:
        capi.check(fctx.lib.fdcap_body_forward(fctx.handle, capi.dptr(p), B, capi.dptr(verts), capi.dptr(joints),
                                               capi.current_stream()), "fdcap_body_forward")
    else:
        capi.check(fctx.lib.fdcap_body_forward_face(fctx.handle, capi.dptr(p), B, capi.dptr(jaw), capi.dptr(expr), capi.dptr(verts),
                                                    capi.dptr(joints), capi.current_stream()), "fdcap_body_forward_face")
    return verts, joints


def world_mesh(ctx, params75: torch.Tensor, scale, camera_ext: torch.Tensor, shape_from_first: bool = False, jaw_pose=None,
               expression=None):
    """World-space vertices [B,V,3] of optimised results: what global_vis.py:116-152 computes frame by
    frame on the CPU (`verts * scale`, then `camera_ext @ T(camera_translation * scale)`).
    shape_from_first=True reuses frame 0's betas for every frame like the viewer does (:118-119, :141).
    jaw_pose [B,3] / expression [B,10]: the fitted face (io.load_body_face); None each: the jaw shut, psi = 0."""
    fctx = _ctx_of(ctx)
    p = params75.float().contiguous().clone()
    if shape_from_first:
        p[:, 6:16] = p[0:1, 6:16]
    B = p.shape[0]
    cam = camera_ext.float().reshape(B, 16).contiguous()
    s = torch.as_tensor(scale, dtype=torch.float32, device=p.device).reshape(1).contiguous()
    verts = torch.empty(B, fctx.num_verts, 3, device=p.device)
    jaw, expr = _face_rows(jaw_pose, B, 3, p.device, "jaw_pose"), _face_rows(expression, B, 10, p.device, "expression")
    if jaw is None and expr is None:
        capi.check(fctx.lib.fdcap_world_mesh(fctx.handle, capi.dptr(p), B, capi.dptr(cam), capi.dptr(s), capi.dptr(verts),
                                             capi.current_stream()), "fdcap_world_mesh")
    else:
        capi.check(fctx.lib.fdcap_world_mesh_face(fctx.handle, capi.dptr(p), B, capi.dptr(jaw), capi.dptr(expr), capi.dptr(cam), capi.dptr(s),
                                                  capi.dptr(verts), capi.current_stream()), "fdcap_world_mesh_face")
    return verts
