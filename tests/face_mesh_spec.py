"""The full mesh under a jaw pose and expression coefficients, as a torch twin of csrc/fdc_face_mesh.h's operators
(fdcap_smplx_forward_face / fdcap_smplx_backward_face, fdcap_body_forward_face, fdcap_world_mesh_face).

The body model is tests/expression_spec.ExprBody as it is: DIRECT form (smplx with `expression` in the shape components and `jaw_pose`
in joint 22's slot) in float64 -- the yardstick -- and float32, the twin the bars come from:

    bar_b = 32 max(max|g32_b - g64_b|, 2^-24 max|g64_b|)        (tests/gradient_bars.bars)

per block b, the blocks being the operator's eight inputs (the new ones: "expression" and "jaw_pose"), the vertices and the joints.
`correction=True` is the form the kernels compute (the chain at jaw = 0, psi = 0, corrected afterwards); `mutant` detaches one piece of
it (tests/expression_spec.MUTANTS), or -- MESH_MUTANT -- the expression directions' rows of the last third of the mesh, the vertices
whose columns sit in the later chunks of expr_dpsi_kernel's reduction.  Values never change under a mutant, only a gradient
contribution goes missing."""
import numpy as np
import torch

from oracle.vposer import VPoserDecoder
from tests import gradient_bars as gb
from tests.expression_spec import MUTANTS, NEXPR, ExprBody

MESH_MUTANT = "mesh_rows"
ALL_MUTANTS = tuple(MUTANTS) + (MESH_MUTANT,)
INPUTS = ("global_orient", "body_pose", "betas", "left_hand_pose", "right_hand_pose", "transl")
FACE = {"jaw": ("jaw_pose",), "psi": ("expression",), "both": ("jaw_pose", "expression")}


def f32(a):
    """rounded to fp32 (what the device is given), held in fp64"""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def make_inputs(B, V, seed, psi_sigma=1.5, jaw_angle=0.3):
    """the operator's inputs at the sizes of tests/test_gpu_ops_autograd.py, an open jaw of `jaw_angle` rad about a random axis,
    psi ~ N(0, psi_sigma^2), and upstream weights for the vertices and the 55 joints; all fp32 values"""
    rng = np.random.default_rng(seed)
    inp = {"global_orient": rng.standard_normal((B, 3)) * 0.8, "body_pose": rng.standard_normal((B, 63)) * 0.4,
           "betas": rng.standard_normal((B, 10)) * 0.5, "left_hand_pose": rng.standard_normal((B, 12)) * 0.3,
           "right_hand_pose": rng.standard_normal((B, 12)) * 0.3, "transl": rng.standard_normal((B, 3))}
    jaw = rng.standard_normal((B, 3))
    inp["jaw_pose"] = jaw_angle * jaw / np.linalg.norm(jaw, axis=1, keepdims=True)
    inp["expression"] = psi_sigma * rng.standard_normal((B, NEXPR))
    inp = {k: f32(v) for k, v in inp.items()}
    return inp, f32(rng.standard_normal((B, V, 3))), f32(rng.standard_normal((B, 55, 3)))


class FaceMeshTwin:
    def __init__(self, bm, dtype=torch.float64, correction=False, mutant=None):
        assert mutant is None or mutant in ALL_MUTANTS
        self.dtype, self.mutant = dtype, mutant
        self.body = ExprBody(bm, dtype=dtype)
        self.body.correction = bool(correction or mutant)
        self.body.mutant = mutant if mutant in MUTANTS else None
        self.cut = None
        if mutant == MESH_MUTANT:                              # the same body with every vertex's E row detached: its tail is taken
            self.cut = ExprBody(bm, dtype=dtype)
            self.cut.correction, self.cut.mutant = True, "real_rows"

    def model(self, t):
        """t: {name: tensor} of the operator's inputs ("jaw_pose" / "expression" may be absent) -> vertices [B,V,3], joints [B,55,3]"""
        out = self.body(return_verts=True, **t)
        verts = out.vertices
        if self.cut is not None and "expression" in t:
            V = verts.shape[1]
            tail = (torch.arange(V) >= V - V // 3)[None, :, None]
            verts = torch.where(tail, self.cut(return_verts=True, **t).vertices, verts)
        return verts, out.joints[:, :55]

    def run(self, inp, face, wv=None, wj=None):
        """inp: make_inputs' dict; face: "jaw" / "psi" / "both"; wv / wj: upstream weights (None: that output carries no gradient)
        -> vertices, joints (numpy), {input: gradient of sum(wv . vertices) + sum(wj . joints)} (empty without weights)"""
        keys = INPUTS + FACE[face]
        t = {k: torch.tensor(inp[k], dtype=self.dtype, requires_grad=True) for k in keys}
        verts, joints = self.model(t)
        grads = {}
        if wv is not None or wj is not None:
            loss = 0
            if wv is not None:
                loss = loss + (verts * torch.tensor(wv, dtype=self.dtype)).sum()
            if wj is not None:
                loss = loss + (joints * torch.tensor(wj, dtype=self.dtype)).sum()
            loss.backward()
            grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().astype(np.float64) for k, v in t.items()}
        return verts.detach().numpy().astype(np.float64), joints.detach().numpy().astype(np.float64), grads


def bars_of(bm, inp, face, wv, wj):
    """-> the fp64 twin's (vertices, joints, grads) and the bar of every block from the twin's two precisions, vertices and joints included"""
    v64, j64, g64 = FaceMeshTwin(bm).run(inp, face, wv, wj)
    v32, j32, g32 = FaceMeshTwin(bm, dtype=torch.float32).run(inp, face, wv, wj)
    b64, b32 = dict(g64, vertices=v64, joints=j64), dict(g32, vertices=v32, joints=j32)
    return b64, b32, gb.bars(b32, b64)


def world_vertices(bm, vp, rows75, scale, cams, jaw=None, psi=None, dtype=torch.float64):
    """global_vis.py's composition (tests/test_gpu_parity.py test_world_mesh_export_matches_viewer_math) on the twin's vertices:
    camera_ext @ T(camera_translation scale) applied to scale (SMPL-X + transl) -> [B,V,3] numpy"""
    p = torch.tensor(np.asarray(rows75), dtype=dtype)
    n = p.shape[0]
    aa = VPoserDecoder.from_data(vp, dtype).decode(p[:, 16:48], output_type="aa").view(n, -1)
    t = dict(body_pose=aa, transl=p[:, 0:3], global_orient=p[:, 3:6], betas=p[:, 6:16], left_hand_pose=p[:, 48:60], right_hand_pose=p[:, 60:72])
    if jaw is not None:
        t["jaw_pose"] = torch.tensor(np.asarray(jaw), dtype=dtype)
    if psi is not None:
        t["expression"] = torch.tensor(np.asarray(psi), dtype=dtype)
    with torch.no_grad():
        verts = ExprBody(bm, dtype=dtype)(return_verts=True, **t).vertices
    cam = torch.tensor(np.asarray(cams), dtype=dtype).reshape(n, 4, 4)
    T = torch.eye(4, dtype=dtype).repeat(n, 1, 1)
    T[:, :3, 3] = p[:, 72:75] * float(scale)
    M = torch.matmul(cam, T)
    vh = torch.cat([verts * float(scale), torch.ones(n, verts.shape[1], 1, dtype=dtype)], 2)
    return torch.matmul(vh, M.transpose(1, 2))[:, :, :3].numpy()


def fit_spec(bm, vp, kmap, faces, face_part=None, ignore=None, dtype=torch.float64):
    """-> a tests/expression_spec.ExpressionSpec that also knows the self-interpenetration term ON THE FITTED FACE: world vertices of ExprBody
    under the jaw and psi (camera frame + camera_translation: the inner fit's scale is 1 and its camera the identity), the collision set of
    every frame by testing every pair in this twin's precision (tests/collision_spec.collision_set), tests/collision_spec.penalty on it"""
    from oracle import rotrepr
    from oracle.fitting import body_params_encapsulate_batch
    from tests import collision_spec as cs
    from tests.expression_spec import ExpressionSpec

    class FaceCollisionSpec(ExpressionSpec):
        def world_vertices(self, x78, jaw=None, expr=None):
            n = x78.shape[0]
            p = body_params_encapsulate_batch(rotrepr.convert_to_3D_rot(x78))
            joint_rot = self.vposer.decode(p["body_pose_vp"], output_type="aa").view(n, -1)
            out = self.body_mesh_model(return_verts=True, body_pose=joint_rot, transl=p["transl"], global_orient=p["global_orient"],
                                       betas=p["betas"], left_hand_pose=p["left_hand_pose"], right_hand_pose=p["right_hand_pose"], jaw_pose=jaw,
                                       expression=expr)
            return out.vertices + x78[:, 75:78].unsqueeze(1)

        def pair_sets(self, verts):
            np_dtype = np.float64 if self.dtype == torch.float64 else np.float32
            return [sorted(cs.collision_set(verts[f].detach().numpy(), faces, face_part, ignore, dtype=np_dtype)) for f in range(verts.shape[0])]

        def collision(self, x78, sigma, w_coll, jaw=None, expr=None, pairs=None):
            """[n]; leaves the pair sets used in self.last_pairs and the vertices in self.last_verts"""
            verts = self.world_vertices(x78, jaw, expr)
            self.last_verts = verts.detach().numpy()
            self.last_pairs = self.pair_sets(verts) if pairs is None else pairs
            return cs.penalty(verts, faces, self.last_pairs, sigma, w_coll)

        def objective(self, x, kp, stage, sigma, w_coll, jaw=None, w_jaw=None, w_bend=0.0, expr=None, w_expr=0.0):
            """per-frame objective [n] with the term"""
            return self.frame_loss(x, kp, stage, jaw, w_jaw, w_bend, expr, w_expr) + self.collision(x, sigma, w_coll, jaw, expr)

        def grads_coll(self, x_np, kp_np, stage, sigma, w_coll, jaw_np=None, w_jaw=None, w_bend=0.0, expr_np=None, w_expr=0.0):
            """-> sums [data, prior, collision], per-frame objective [n], {"rows" [n, 78], "jaw" [n, 3], "psi" [n, 10]} (the free ones)"""
            leaf = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=self.dtype, requires_grad=True)
            x, jaw, expr = leaf(x_np), leaf(jaw_np), leaf(expr_np)
            kp = torch.tensor(np.asarray(kp_np), dtype=self.dtype)
            data, prior = self.frame_terms(x, kp, stage, jaw, w_jaw, w_bend, expr, w_expr)
            e = self.collision(x, sigma, w_coll, jaw, expr)
            (data + prior + e).sum().backward()
            g = {k: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().astype(np.float64)
                 for k, v in (("rows", x), ("jaw", jaw), ("psi", expr)) if v is not None}
            return (np.array([float(data.sum().detach()), float(prior.sum().detach()), float(e.sum().detach())]),
                    (data + prior + e).detach().numpy().astype(np.float64), g)

    return FaceCollisionSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, dtype=dtype)
