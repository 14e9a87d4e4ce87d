"""Per-frame inner fit with a true 2D-keypoint reprojection residual, batched over frames on one GPU
(BASELINE config 4) over `fdcap_opt_backward_fit2d` (include/fdcap.h, csrc/fdc_fit2d.h).

Not part of the reference repository (there it is the external SMPLify-X step, README.md:14-17); the objective is the
published SMPLify-X data term + L2 priors in five weight stages, optimised either as SMPLify-X does -- L-BFGS with a
strong-Wolfe line search, every frame its own problem, a fresh optimiser per stage (`optimizer="lbfgs"`: the batched state
machine of csrc/fdc_lbfgs.h through `fdcap_opt_fit2d_lbfgs`) -- or with Adam (`optimizer="adam"`, round 3's form).
Inputs / outputs use the repository's own parameter layout ([N,75] rows, SMPLify-X pkl keys), so the result can feed
`global_optimization_hip.py` directly."""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi

# (w_data, w_pose, w_shape, w_hand) per stage
DEFAULT_STAGES = ((1.0, 404.0, 100.0, 404.0), (1.0, 404.0, 50.0, 404.0), (1.0, 57.4, 10.0, 57.4), (1.0, 4.78, 5.0, 4.78),
                  (1.0, 4.78, 5.0, 4.78))
DEFAULT_INTRINSICS = (692.0, 692.0, 640.0, 360.0)      # vis.py:358-360
# SMPLify-X's optimiser settings (fit_smplx.yaml: maxiters 30, ftol 2e-9, gtol 1e-9, lr 1.0) over torch.optim.LBFGS's
# defaults (history 100, tolerance_grad 1e-7, tolerance_change 1e-9, max_eval = max_iter * 5 / 4, 25 line-search evaluations)
DEFAULT_LBFGS = dict(history=100, max_iter=30, max_eval=0, max_steps=30, max_ls=25, lr=1.0, tolerance_grad=1e-7,
                     tolerance_change=1e-9, ftol=2e-9, gtol=1e-9)


# OpenPose's keypoint orders as indices into smplx's 127-joint output (55 joints, 21 vertex joints, 51 + 17 face landmarks).
# [upstream-recall: SMPLify-X's smpl_to_openpose(model_type="smplx", use_hands=True, openpose_format="coco25"); neither smplx nor
# SMPLify-X is part of this repository, so a caller who has them passes the lists they give instead]
OPENPOSE_BODY25 = (55, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65)
OPENPOSE_LHAND = (20, 37, 38, 39, 66, 25, 26, 27, 67, 28, 29, 30, 68, 34, 35, 36, 69, 31, 32, 33, 70)
OPENPOSE_RHAND = (21, 52, 53, 54, 71, 40, 41, 42, 72, 43, 44, 45, 73, 49, 50, 51, 74, 46, 47, 48, 75)
NUM_SMPLX_JOINTS, NUM_EXTRA_VERTEX_JOINTS = 55, 21
# The bending prior's terms (body joint 1..21, axis, sign): elbows about y, knees about x, and its weight as a multiple of the
# stage's w_pose.  [upstream-recall: SMPLify-X's angle_prior_idxs 55, 58, 12, 15 of the full pose minus the global orientation's
# three entries, with signs (1, -1, -1, -1); fitting.py's bending_prior_weight = 3.17 * body_pose_weight.  Neither package is part of
# this repository: defaults a caller can replace through bend_prior, never constants of a kernel]
DEFAULT_BEND_TERMS = ((18, 1, 1.0), (19, 1, -1.0), (4, 0, -1.0), (5, 0, -1.0))
DEFAULT_BEND_RATIO = 3.17
MAX_BEND_TERMS = 8      # FDCAP_MAX_BEND_TERMS
# The jaw prior's weights (x, y, z of the jaw's axis-angle) per stage.  [upstream-recall: fit_smplx.yaml's jaw_pose_prior_weights]
DEFAULT_JAW_PRIOR = ((4.04e3, 4.04e4, 4.04e4), (4.04e3, 4.04e4, 4.04e4), (574.0, 5740.0, 5740.0), (47.8, 478.0, 478.0), (47.8, 478.0, 478.0))
# The expression prior's weight per stage: w^2 |expression|^2.  [upstream-recall: fit_smplx.yaml's expr_weights; not part of this
# repository: a default a caller can replace through expression_prior, never a constant of a kernel]
DEFAULT_EXPRESSION_PRIOR = (1e2, 5e1, 1e1, 0.5e1, 0.5e1)
NUM_EXPRESSION = 10

# How a fit starts from keypoints alone (csrc/fdc_fit2d_init.h), as SMPL-X JOINTS -- resolved to keypoint slots per layout: the depth
# guess's torso edges (left shoulder - left hip, right shoulder - right hip), the camera stage's keypoints (both shoulders, both hips)
# and weights, the shoulders of the side-view test.  w_data None: 1000 / image height, the height taken as 2 cy.
# [upstream-recall: SMPLify-X's guess_init (edge_idxs 5-12 and 2-9 of OpenPose's BODY_25), init_joints_idxs 9, 12, 2, 5,
# data_weight = 1000 / H, depth_loss_weight 1e2, side_view_thsh 25, its default init_t depth 2.5 and fitting.py's camera loss without
# a robustifier or confidences; not part of this repository: defaults a caller can replace through init, never constants of a kernel]
DEFAULT_INIT = dict(edges=((16, 1), (17, 2)), torso=(16, 17, 1, 2), shoulders=(16, 17), conf_thr=0.0, default_depth=2.5, side_view_px=25.0,
                    w_data=None, w_depth=100.0)
MAX_INIT_EDGES, MAX_INIT_TORSO = 4, 8       # fdcap_fit2d_init's lists

# The self-interpenetration term (csrc/fdc_collide.h): the cone's opening, the weight per stage (on in the last two), pairs kept per
# frame, and which pairs of body parts are never tested (a part with itself, a part with its parent part, the listed pairs).
# [upstream-recall: SMPLify-X's fit_smplx.yaml coll_loss_weights 0, 0, 0, 0.01, 1.0, penalize_outside / df_cone_height 0.5 with
# torch-mesh-isect's DistanceFieldPenetrationLoss (sigma 0.5, point2plane false), max_collisions 128 per BVH query, and its
# part_segm_fn / ign_part_pairs filter of a part against itself and its parent; neither package nor the segmentation file is part of
# this repository: defaults a caller can replace through collision, never constants of a kernel]
DEFAULT_COLLISION = dict(faces=None, face_part=None, part_parent=None, ignore_pairs=(), same_part=True, sigma=0.5,
                         weights=(0.0, 0.0, 0.0, 0.01, 1.0), capacity=4096, follow_face=False)
COLLISION_PARTS = 64    # parts of include/fdcap.h's 64 x 64 bit matrix


def joints23_from_openpose(rows):
    """io.read_openpose_json rows, one per frame ([n, >= 25, 3] or a list of [>= 25, 3] arrays: u, v, confidence with BODY_25 first)
    -> [n,23,3] float32 in SMPL-X joint order, the layout fdcap_opt_set_keypoints and FittingOP.fitting(keypoints=...) take.  The 14
    BODY_25 keypoints whose OPENPOSE_BODY25 target is a body joint (below 23) go to that joint; every other joint -- the pelvis' three
    spine joints, the collars, the feet -- gets zeros: confidence 0, no data term.  Pure host code."""
    rows = [np.asarray(r, dtype=np.float32) for r in rows]
    out = np.zeros((len(rows), 23, 3), np.float32)
    for i, r in enumerate(rows):
        if r.ndim != 2 or r.shape[0] < len(OPENPOSE_BODY25) or r.shape[1] != 3:
            raise ValueError(f"frame {i}: expected [>= {len(OPENPOSE_BODY25)}, 3] keypoint rows, got {r.shape}")
        for k, j in enumerate(OPENPOSE_BODY25):
            if j < 23:
                out[i, j] = r[k]
    return out


def collision_filter(face_part=None, part_parent=None, ignore_pairs=(), same_part=True):
    """-> [64] uint64, the 64 x 64 bit matrix of fdcap_set_collision_mesh: bit b of row a drops every pair of faces of parts a and b
    (either way round).  Sets the listed `ignore_pairs` (a, b); with `same_part` a part with itself and -- `part_parent` [<= 64],
    -1 for none -- a part with its parent part.  `face_part` limits `same_part` to the parts that occur (None: all 64).  Pure host code."""
    m = [0] * COLLISION_PARTS

    def put(a, b):
        a, b = int(a), int(b)
        if not (0 <= a < COLLISION_PARTS and 0 <= b < COLLISION_PARTS):
            raise capi.FdcapError(f"a part must be in 0..{COLLISION_PARTS - 1}: ({a}, {b})")
        m[a] |= 1 << b
        m[b] |= 1 << a

    for a, b in ignore_pairs:
        put(a, b)
    if same_part:
        parts = range(COLLISION_PARTS) if face_part is None else sorted(set(int(p) for p in np.asarray(face_part).reshape(-1)))
        for a in parts:
            put(a, a)
        if part_parent is not None:
            pp = np.asarray(part_parent).reshape(-1)
            if pp.shape[0] > COLLISION_PARTS:
                raise capi.FdcapError(f"part_parent has more than {COLLISION_PARTS} entries")
            for a, b in enumerate(pp):
                if b >= 0:
                    put(a, b)
    return np.array(m, dtype=np.uint64)


class KeypointMap:
    """Which body point each detected keypoint is (include/fdcap.h fdcap_set_keypoint_map): joint[k] >= 0 an SMPL-X joint, else the
    surface point bary[k] . vertices[tri[k]] (a plain vertex: (v, v, v), (1, 0, 0))."""

    def __init__(self, joint, tri, bary):
        self.joint = np.ascontiguousarray(joint, dtype=np.int32).reshape(-1)
        self.tri = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1, 3)
        self.bary = np.ascontiguousarray(bary, dtype=np.float32).reshape(-1, 3)
        n = self.joint.shape[0]
        if self.tri.shape[0] != n or self.bary.shape[0] != n:
            raise capi.FdcapError("joint [n], tri [n,3] and bary [n,3] must describe the same keypoints")
        if n > capi.MAX_KEYPOINTS:
            raise capi.FdcapError(f"{n} keypoints: a map holds at most {capi.MAX_KEYPOINTS}")

    def __len__(self):
        return int(self.joint.shape[0])

    @classmethod
    def joints23(cls):
        """SMPL-X joints 0..22 in order: the layout fitting() takes without a map."""
        return cls(np.arange(23), np.zeros((23, 3)), np.zeros((23, 3)))

    @classmethod
    def from_smplx_indices(cls, indices, extra_vertex_ids, lmk_vertex_triples=None, lmk_bary=None):
        """indices in smplx's 127-joint output convention: < 55 a joint; 55..75 the caller's 21 `extra_vertex_ids` in smplx's order
        (nose, eyes, ears, big toe / small toe / heel left then right, the ten fingertips: smplx.vertex_ids, never hard-coded here);
        >= 76 landmark i - 76 = lmk_bary[i - 76] . vertices[lmk_vertex_triples[i - 76]] (the model file's lmk_faces_idx resolved
        through its faces, and lmk_bary_coords)."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        n = idx.shape[0]
        joint, tri, bary = np.full(n, -1, np.int32), np.zeros((n, 3), np.int32), np.zeros((n, 3), np.float32)
        extra = np.asarray(extra_vertex_ids, dtype=np.int64).reshape(-1)
        first_lmk = NUM_SMPLX_JOINTS + NUM_EXTRA_VERTEX_JOINTS
        for k, i in enumerate(idx):
            if i < 0:
                raise capi.FdcapError(f"keypoint {k}: index {i}")
            if i < NUM_SMPLX_JOINTS:
                joint[k] = i
            elif i < first_lmk:
                if extra.shape[0] != NUM_EXTRA_VERTEX_JOINTS:
                    raise capi.FdcapError(f"extra_vertex_ids must hold smplx's {NUM_EXTRA_VERTEX_JOINTS} vertex joints")
                tri[k], bary[k] = extra[i - NUM_SMPLX_JOINTS], (1.0, 0.0, 0.0)
            else:
                if lmk_vertex_triples is None or lmk_bary is None or i - first_lmk >= len(lmk_vertex_triples):
                    raise capi.FdcapError(f"keypoint {k}: landmark {i - first_lmk} without lmk_vertex_triples / lmk_bary")
                tri[k], bary[k] = lmk_vertex_triples[i - first_lmk], lmk_bary[i - first_lmk]
        return cls(joint, tri, bary)


def init_slots(joints, keypoint_map):
    """SMPL-X joints -> slots of a frame's keypoint array: the joint itself in the 23-joint layout (keypoint_map None), else the first
    entry of the map that is this joint"""
    out = []
    for j in joints:
        j = int(j)
        if keypoint_map is None:
            if not 0 <= j < 23:
                raise capi.FdcapError(f"init: joint {j} is not in the 23-joint layout")
            out.append(j)
        else:
            hit = np.flatnonzero(keypoint_map.joint == j)
            if j < 0 or hit.size == 0:
                raise capi.FdcapError(f"init: joint {j} is not a keypoint of the map")
            out.append(int(hit[0]))
    return out


def init_struct(settings, keypoint_map, intrinsics):
    """capi.Fit2dInit of a full settings dict (DEFAULT_INIT's keys, joints) for this keypoint layout and camera"""
    edges = [init_slots(e, keypoint_map) for e in settings["edges"]]
    torso, shoulders = init_slots(settings["torso"], keypoint_map), init_slots(settings["shoulders"], keypoint_map)
    if not 1 <= len(edges) <= MAX_INIT_EDGES or any(len(e) != 2 for e in edges) or not 1 <= len(torso) <= MAX_INIT_TORSO or len(shoulders) != 2:
        raise capi.FdcapError(f"init: 1..{MAX_INIT_EDGES} edges of two joints, 1..{MAX_INIT_TORSO} torso joints, two shoulders")
    ci = capi.Fit2dInit()
    ci.n_edge, ci.n_torso = len(edges), len(torso)
    for e, (a, b) in enumerate(edges):
        ci.edge[e][0], ci.edge[e][1] = a, b
    for k, v in enumerate(torso):
        ci.torso[k] = v
    ci.shoulder[0], ci.shoulder[1] = shoulders
    w_data = 1000.0 / (2.0 * intrinsics[3]) if settings["w_data"] is None else settings["w_data"]
    ci.conf_thr, ci.default_depth, ci.side_view_px = float(settings["conf_thr"]), float(settings["default_depth"]), float(settings["side_view_px"])
    ci.w_data, ci.w_depth = float(w_data), float(settings["w_depth"])
    return ci


class InnerFitOP:
    def __init__(self, body_model, vposer, num_frames, intrinsics=DEFAULT_INTRINSICS, rho=100.0, lr=0.01,
                 stages=DEFAULT_STAGES, iters_per_stage=30, optimizer="adam", lbfgs=None, max_rounds=4000,
                 keypoint_map=None, group_of=None, group_weights=None, fit_jaw=False, jaw_prior=None,
                 bend_prior=None, init=None, orientations="auto", collision=None, fit_expression=False, expression_prior=None):
        """optimizer "adam": iters_per_stage steps of Adam(lr) per stage; "lbfgs": per frame and stage, SMPLify-X's L-BFGS loop
        with the settings `lbfgs` (keys of DEFAULT_LBFGS; missing ones take their defaults), at most max_rounds objective
        evaluations per stage.
        keypoint_map (KeypointMap): fitting() then takes keypoints [N, len(map), 3] in the map's order.  group_of [len(map)] names
        each keypoint's group (0 without it) and group_weights[stage][group] multiplies the group's confidences before that stage's
        upload -- SMPLify-X's per-stage hand and face data weights; default all 1.
        fit_jaw: the jaw pose (SMPL-X joint 22, a leaf: the vertices skinned to it follow, no joint moves) is a free axis-angle per
        frame next to the row -- needs a keypoint_map, whose face landmarks are what sees it; fitting() leaves it in self.jaw_pose.
        jaw_prior [stages][3]: the weights of sum_c (w[c] jaw[c])^2 per stage (default DEFAULT_JAW_PRIOR when stages has its five).
        bend_prior: None (off: not one more library call), or dict(terms=DEFAULT_BEND_TERMS, ratio=DEFAULT_BEND_RATIO) -- SMPLify-X's
        bending prior ratio * w_pose * sum exp(sign * aa_joint[axis])^2 over the (joint 1..21, axis, sign) terms, added to every
        stage's priors (missing keys take their defaults; the weight is not squared).
        init: None (off: fitting() needs rows that already stand in front of the camera, and not one call differs), or a dict with
        keys of DEFAULT_INIT (missing ones take their defaults; {} is all defaults): fitting() then starts as SMPLify-X does -- a depth
        guess from torso edge lengths, a camera stage over global_orient and camera_translation alone on the torso keypoints, and
        by `orientations` a twin problem per frame with the body turned 180 degrees about y, the fit with the lower final objective
        kept: "auto" for the frames whose shoulders nearly coincide in the image, "both" for all, "given" for none.
        collision: None (off: not one more library call), or a dict with keys of DEFAULT_COLLISION (missing ones take their defaults):
        the self-interpenetration term of csrc/fdc_collide.h on `faces` [F,3] (default: body_model.faces), weighted per stage by
        `weights`; `face_part` [F] in 0..63, `part_parent`, `ignore_pairs` and `same_part` go through collision_filter.  With
        fit_jaw or fit_expression it needs `follow_face=True`: the term's full-mesh pass then skins the fitted face
        (fdcap_opt_set_fit2d_collision_face) and its gradient reaches the jaw and the coefficients; without the key the pass would skin
        with the shut jaw at expression zero, and both combinations are refused.
        fit_expression: SMPL-X's ten expression coefficients are free per frame next to the row (and the jaw) -- needs a keypoint_map,
        whose face landmarks are what sees them, and a body model with expression directions (shapedirs [V,3,20]); with collision only
        under its `follow_face=True`; fitting() leaves them in self.expression.  expression_prior [stages]: the weight
        w of w^2 |expression|^2 per stage (default DEFAULT_EXPRESSION_PRIOR when stages has its five)."""
        import torch
        follow = bool(collision.get("follow_face", False)) if collision is not None else False
        if collision is not None and fit_expression and not follow:         # (checked before anything touches the device)
            raise capi.FdcapError("collision does not go with fit_expression: the full-mesh pass skins at expression zero")
        if fit_expression and keypoint_map is None:
            raise capi.FdcapError("fit_expression needs a keypoint_map: the correction runs in the mapped data term")
        if expression_prior is not None and not fit_expression:
            raise capi.FdcapError("expression_prior belongs to fit_expression")
        self.fit_expression, self.expression_prior, self.expression = bool(fit_expression), None, None
        if self.fit_expression:
            ep = np.asarray(DEFAULT_EXPRESSION_PRIOR if expression_prior is None else expression_prior, dtype=np.float32).reshape(-1)
            if ep.shape != (len(tuple(stages)),) or not np.all(np.isfinite(ep)):
                raise capi.FdcapError("expression_prior must be [stages], finite")
            if np.asarray(body_model.shapedirs).shape[2] < 10 + NUM_EXPRESSION:
                raise capi.FdcapError("fit_expression needs a body model with expression directions: shapedirs [V,3,20]")
            self.expression_prior = ep
        self.collision = None
        if collision is not None:                             # (checked before anything touches the device)
            unknown = set(collision) - set(DEFAULT_COLLISION)
            if unknown:
                raise capi.FdcapError(f"unknown collision settings {sorted(unknown)}")
            q = {**DEFAULT_COLLISION, **collision}
            if fit_jaw and not follow:
                raise capi.FdcapError("collision does not go with fit_jaw: the full-mesh pass skins with the shut jaw's transforms")
            faces = q["faces"] if q["faces"] is not None else getattr(body_model, "faces", None)
            if faces is None:
                raise capi.FdcapError("collision needs faces: the body model has none, pass collision=dict(faces=...)")
            faces = np.ascontiguousarray(faces, dtype=np.int32).reshape(-1, 3)
            nv = int(np.asarray(body_model.v_template).shape[0])
            if not 3 <= faces.shape[0] <= 65535 or faces.min() < 0 or faces.max() >= nv:
                raise capi.FdcapError("collision: 3 .. 65535 faces with vertex indices inside the body model")
            w = tuple(float(v) for v in q["weights"])
            if len(w) != len(tuple(stages)) or any(not (v >= 0.0 and np.isfinite(v)) for v in w):
                raise capi.FdcapError("collision weights: one finite weight >= 0 per stage")
            if not 0.0 < float(q["sigma"]) < 1.0 or int(q["capacity"]) <= 0:
                raise capi.FdcapError("collision: sigma in (0, 1) and capacity > 0")
            ign = collision_filter(q["face_part"], q["part_parent"], q["ignore_pairs"], q["same_part"]) if q["face_part"] is not None or q["ignore_pairs"] else None
            self.collision = dict(faces=faces, face_part=q["face_part"], ignore=ign, sigma=float(q["sigma"]), weights=w, capacity=int(q["capacity"]),
                                  follow_face=follow)
        if not torch.cuda.is_available():
            raise capi.FdcapError("no HIP device: the fdcap_amd inner fit only runs on the GPU")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.ctx = capi.Context(body_model, vposer)
        self.ctx.set_scene(np.zeros((0, 3), np.float32))
        if self.collision is not None:
            self.ctx.set_collision_mesh(self.collision["faces"], self.collision["face_part"], self.collision["ignore"])
        self.n = int(num_frames)
        self.intrinsics, self.rho, self.lr = tuple(float(v) for v in intrinsics), float(rho), float(lr)
        self.stages, self.iters_per_stage = tuple(stages), int(iters_per_stage)
        if optimizer not in ("adam", "lbfgs"):
            raise capi.FdcapError(f"optimizer must be 'adam' or 'lbfgs', not {optimizer!r}")
        unknown = set(lbfgs or {}) - set(DEFAULT_LBFGS)
        if unknown:
            raise capi.FdcapError(f"unknown L-BFGS settings {sorted(unknown)}")
        self.optimizer, self.lbfgs, self.max_rounds = optimizer, {**DEFAULT_LBFGS, **(lbfgs or {})}, int(max_rounds)
        self.keypoint_map, self.group_of, self.group_weights = keypoint_map, None, None
        if keypoint_map is None:
            if group_of is not None or group_weights is not None:
                raise capi.FdcapError("group_of / group_weights belong to a keypoint_map")
        else:
            self.group_of = np.zeros(len(keypoint_map), np.int64) if group_of is None else np.asarray(group_of, dtype=np.int64).reshape(-1)
            if self.group_of.shape[0] != len(keypoint_map) or (len(keypoint_map) and self.group_of.min() < 0):
                raise capi.FdcapError("group_of must name a group >= 0 for every keypoint of the map")
            if group_weights is not None:
                gw = np.asarray(group_weights, dtype=np.float32)
                if gw.ndim != 2 or gw.shape[0] != len(self.stages) or gw.shape[1] <= int(self.group_of.max(initial=0)):
                    raise capi.FdcapError("group_weights must be [stages][groups]")
                self.group_weights = gw
            self.ctx.set_keypoint_map(keypoint_map.joint, keypoint_map.tri, keypoint_map.bary)
        self.fit_jaw, self.jaw_prior, self.jaw_pose = bool(fit_jaw), None, None
        self.rows75 = None                                    # the rows the last fitting() returned [N,75] (device tensor): what face_mesh() skins
        if self.fit_jaw:
            if keypoint_map is None:
                raise capi.FdcapError("fit_jaw needs a keypoint_map: no keypoint of the 23-joint layout follows the jaw")
            jp = DEFAULT_JAW_PRIOR if jaw_prior is None else jaw_prior
            self.jaw_prior = np.asarray(jp, dtype=np.float32)
            if self.jaw_prior.shape != (len(self.stages), 3):
                raise capi.FdcapError("jaw_prior must be [stages][3]")
        elif jaw_prior is not None:
            raise capi.FdcapError("jaw_prior belongs to fit_jaw")
        self.bend_prior = None
        if bend_prior is not None:
            unknown = set(bend_prior) - {"terms", "ratio"}
            if unknown:
                raise capi.FdcapError(f"unknown bend_prior settings {sorted(unknown)}")
            terms = tuple((int(j), int(a), float(s)) for j, a, s in bend_prior.get("terms", DEFAULT_BEND_TERMS))
            if len(terms) > MAX_BEND_TERMS or any(not (1 <= j <= 21 and 0 <= a <= 2) for j, a, _ in terms):
                raise capi.FdcapError(f"bend_prior: at most {MAX_BEND_TERMS} terms (joint 1..21, axis 0..2, sign)")
            self.bend_prior = (terms, float(bend_prior.get("ratio", DEFAULT_BEND_RATIO)))
        self.init = None
        if orientations not in ("auto", "both", "given"):
            raise capi.FdcapError(f"orientations must be 'auto', 'both' or 'given', not {orientations!r}")
        self.orientations = orientations
        if init is not None:
            unknown = set(init) - set(DEFAULT_INIT)
            if unknown:
                raise capi.FdcapError(f"unknown init settings {sorted(unknown)}")
            self.init = init_struct({**DEFAULT_INIT, **init}, keypoint_map, self.intrinsics)
        self.depth_guess = self.depth_valid = self.tried_both = self.chosen = self.camera_rows = self.final_loss = None
        self.camera_rounds = []
        self.log, self.rounds, self.frame_iterations, self.frame_loss = [], [], [], []

    def _set_extra(self, si, w_pose):
        """this stage's jaw prior weights and bending prior (ratio * w_pose on the terms)"""
        ex = capi.Fit2dExtra()
        if self.jaw_prior is not None:
            ex.w_jaw[0], ex.w_jaw[1], ex.w_jaw[2] = (float(v) for v in self.jaw_prior[si])
        if self.bend_prior is not None:
            terms, ratio = self.bend_prior
            ex.w_bend, ex.n_bend = ratio * w_pose, len(terms)
            for t, (j, a, s) in enumerate(terms):
                ex.joint[t], ex.axis[t], ex.sign[t] = j, a, s
        capi.check(self.ctx.lib.fdcap_opt_set_fit2d_extra(self.ctx.handle, ctypes.byref(ex)), "fdcap_opt_set_fit2d_extra")

    def fitting(self, rows75, keypoints, log_every=0, jaw_init=None, expression_init=None):
        """rows75 [N,75] initial parameters (device tensor or numpy), keypoints [N,23,3] (u, v, confidence) -- with a keypoint_map
        [N,len(map),3] in its order -- -> optimised rows [N,75] (device tensor).  fit_jaw: the jaw starts from jaw_init [N,3] (default
        zero) and ends in self.jaw_pose [N,3] (device tensor); fit_expression: the coefficients start from expression_init [N,10]
        (default zero) and end in self.expression [N,10] (device tensor).
        With init: rows75 may be None (neutral rows: all zero); of given rows everything but camera_translation is kept.  Leaves
        self.depth_guess / depth_valid [N] (numpy), self.camera_rows [N,75] (the rows after the camera stage), self.tried_both [N]
        (numpy bool), self.chosen [N] (numpy, 1: the turned body won), self.camera_rounds (L-BFGS: the camera stages' evaluations) and, when a
        twin was tried, self.final_loss [N + twins] (device: the full objective under the last stage);
        self.rounds / frame_iterations / frame_loss / body_rotation_rec then cover the N frames followed by the twins."""
        if self.init is None:
            if rows75 is None:
                raise capi.FdcapError("fitting(None, ...) needs init: without it the rows must already stand in front of the camera")
            self.rows75 = self._fit(self.n, rows75, keypoints, log_every, jaw_init, expression_init)
        else:
            self.rows75 = self._fit_from_keypoints(rows75, keypoints, log_every, jaw_init, expression_init)
        return self.rows75

    def face_mesh(self):
        """Vertices [N,V,3] (device tensor) of the rows fitting() returned, WITH the fitted face -- self.jaw_pose and self.expression where
        they were free -- in the frame the keypoints are projected from: SMPL-X's output + transl + camera_translation.  The full mesh
        through ops.body_forward_from_params (fdcap_body_forward_face)."""
        from . import ops
        if self.rows75 is None:
            raise capi.FdcapError("face_mesh() needs fitted rows: call fitting() first")
        verts, _ = ops.body_forward_from_params(self.ctx, self.rows75, True, jaw_pose=self.jaw_pose if self.fit_jaw else None,
                                                expression=self.expression if self.fit_expression else None)
        return verts + self.rows75[:, None, 72:75]

    def _tensor(self, a):
        import torch
        return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))).to(self.device, torch.float32).contiguous()

    def _camera_stage(self, n, rows75, kp, guess):
        """n problems: [the depth guess into camera_translation,] the camera stage -> the rows after it (+ z, valid, side_view [n])"""
        import torch
        lib, h, dev = self.ctx.lib, self.ctx.handle, self.device
        self._setup(n, rows75, kp)
        fx, fy, cx, cy = self.intrinsics
        sg = capi.Fit2dStage(fx, fy, cx, cy, self.rho, 1.0, 0.0, 0.0, 0.0)
        ci = ctypes.byref(self.init)
        found = None
        if guess:
            found = (torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev))
            capi.check(lib.fdcap_opt_fit2d_guess(h, ctypes.byref(sg), ci, *(capi.dptr(v) for v in found), capi.current_stream()), "fdcap_opt_fit2d_guess")
        if self.optimizer == "lbfgs":
            q = self.lbfgs
            cf = capi.LbfgsConfig(capi.XDIM, q["history"], q["max_iter"], q["max_eval"], q["max_steps"], q["max_ls"], q["lr"],
                                  q["tolerance_grad"], q["tolerance_change"], q["ftol"], q["gtol"])
            rounds = ctypes.c_int32(0)
            capi.check(lib.fdcap_opt_fit2d_camera_lbfgs(h, ctypes.byref(sg), ci, ctypes.byref(cf), self.max_rounds, ctypes.byref(rounds),
                                                        capi.current_stream()), "fdcap_opt_fit2d_camera_lbfgs")
            self.camera_rounds.append(int(rounds.value))
        else:
            capi.check(lib.fdcap_opt_reset_adam(h, capi.current_stream()), "fdcap_opt_reset_adam")
            for it in range(self.iters_per_stage):
                capi.check(lib.fdcap_opt_backward_fit2d_camera(h, ctypes.byref(sg), ci, 0, capi.current_stream()), "fdcap_opt_backward_fit2d_camera")
                capi.check(lib.fdcap_opt_step_x(h, it + 1, capi.current_stream()), "fdcap_opt_step_x")
        out = torch.empty(n, capi.PDIM, device=dev)
        capi.check(lib.fdcap_opt_get_results(h, capi.dptr(out), None, None, capi.current_stream()), "fdcap_opt_get_results")
        return out, found

    def _fit_from_keypoints(self, rows75, keypoints, log_every, jaw_init, expression_init=None):
        import torch
        lib, h, dev, n = self.ctx.lib, self.ctx.handle, self.device, self.n
        kp = self._tensor(keypoints)
        start = torch.zeros(n, capi.PDIM, device=dev) if rows75 is None else self._tensor(rows75).clone()
        if not self.stages:
            raise capi.FdcapError("init needs at least one stage: the two fits of a frame are compared under the last one")
        self.camera_rounds = []
        rows, (z, valid, side) = self._camera_stage(n, start, kp, True)
        self.depth_guess, self.depth_valid = z.cpu().numpy(), valid.cpu().numpy()            # (the one set-up synchronisation)
        flagged = {"auto": side.cpu().numpy() != 0, "both": np.ones(n, bool), "given": np.zeros(n, bool)}[self.orientations]
        self.tried_both, self.chosen, self.camera_rows = flagged, np.zeros(n, np.int32), rows
        src = torch.from_numpy(np.flatnonzero(flagged).astype(np.int32)).to(dev)
        m = int(src.shape[0])
        if m == 0:
            return self._fit(n, rows, kp, log_every, jaw_init, expression_init)
        # the twins: the same start at the guessed depth, the body turned, their own camera stage -- then all n + m through the stages
        pick = src.long()
        twin = start[pick].contiguous()
        twin[:, 72:74], twin[:, 74] = 0.0, z[pick]
        capi.check(lib.fdcap_fit2d_flip_orient(capi.dptr(twin), m, capi.current_stream()), "fdcap_fit2d_flip_orient")
        twin, _ = self._camera_stage(m, twin, kp[pick].contiguous(), False)
        jaw_all = None
        if jaw_init is not None:
            jaw0 = self._tensor(jaw_init)
            jaw_all = torch.cat([jaw0, jaw0[pick]]).contiguous()
        expr_all = None
        if expression_init is not None:
            expr0 = self._tensor(expression_init)
            expr_all = torch.cat([expr0, expr0[pick]]).contiguous()
        both = self._fit(n + m, torch.cat([rows, twin]).contiguous(), torch.cat([kp, kp[pick]]).contiguous(), log_every, jaw_all, expr_all)
        floss = torch.empty(n + m, device=dev)
        capi.check(lib.fdcap_opt_fit2d_frame_loss(h, ctypes.byref(self._last_stage), capi.dptr(floss), capi.current_stream()), "fdcap_opt_fit2d_frame_loss")
        out, chosen = torch.empty(n, capi.PDIM, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        jaw_out = torch.empty(n, 3, device=dev) if self.fit_jaw else None
        capi.check(lib.fdcap_fit2d_select(capi.dptr(both), capi.dptr(floss), capi.dptr(src), n, m, capi.dptr(self.jaw_pose) if self.fit_jaw else None,
                                          capi.dptr(out), capi.dptr(jaw_out), capi.dptr(chosen), capi.current_stream()), "fdcap_fit2d_select")
        self.chosen, self.final_loss = chosen.cpu().numpy(), floss
        if self.fit_jaw:
            self.jaw_pose = jaw_out
        if self.fit_expression:                               # (fdcap_fit2d_select does not carry them: the twin's where it won)
            twin_of = torch.full((n,), -1, dtype=torch.long, device=dev)
            twin_of[pick] = n + torch.arange(m, device=dev)
            take = torch.where(chosen.long() != 0, twin_of, torch.arange(n, device=dev))
            self.expression = self.expression[take].contiguous()
        return out

    def _setup(self, n, rows75, kp):
        """the optimiser state of n problems at these rows and keypoints"""
        import torch
        lib, h, dev = self.ctx.lib, self.ctx.handle, self.device
        nkp = 23 if self.keypoint_map is None else len(self.keypoint_map)
        if tuple(rows75.shape) != (n, capi.PDIM) or tuple(kp.shape) != (n, nkp, 3):
            raise capi.FdcapError(f"expected rows [{n},75] and keypoints [{n},{nkp},3]")
        st = capi.current_stream()
        x78 = torch.empty(n, capi.XDIM, device=dev)
        capi.check(lib.fdcap_params_75_to_78(capi.dptr(rows75), n, capi.dptr(x78), st), "fdcap_params_75_to_78")
        # the optimiser state of the clip-level loop, with scale = 1 and camera_ext = identity: its "world" joints are
        # then the camera-frame joints + camera_translation; no contact / temporal term is ever evaluated
        oc = capi.OptConfig(n, n, 0, self.lr, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)
        R = n + 4
        self._rows_x = torch.zeros(R, capi.XDIM, device=dev)
        self._rows_cam = torch.zeros(R, 16, device=dev)
        self._scale, self._dscale = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        self._losses = torch.zeros(capi.NUM_LOSSES, device=dev, dtype=torch.float64)
        torch.cuda.current_stream().synchronize()
        capi.check(lib.fdcap_opt_create(h, ctypes.byref(oc), capi.dptr(self._rows_x), capi.dptr(self._rows_cam),
                                        capi.dptr(self._scale), capi.dptr(self._dscale), capi.dptr(self._losses)), "fdcap_opt_create")
        eye = torch.eye(4, device=dev).reshape(1, 16).repeat(n, 1).contiguous()
        self._rows_cam[:] = torch.eye(4, device=dev).reshape(1, 16)          # halo rows too (their forward is evaluated, never used)
        capi.check(lib.fdcap_opt_set_inputs(h, capi.dptr(x78), capi.dptr(x78), capi.dptr(torch.ones(n, device=dev)), capi.dptr(eye), st),
                   "fdcap_opt_set_inputs")
        if self.keypoint_map is None:
            capi.check(lib.fdcap_opt_set_keypoints(h, capi.dptr(kp), st), "fdcap_opt_set_keypoints")
        else:
            capi.check(lib.fdcap_opt_set_keypoints_mapped(h, capi.dptr(kp), st), "fdcap_opt_set_keypoints_mapped")

    def _fit(self, n, rows75, keypoints, log_every, jaw_init, expression_init=None):
        """the stages over n problems from rows that stand in front of the camera"""
        import torch
        lib, h, dev = self.ctx.lib, self.ctx.handle, self.device
        t = self._tensor
        rows75, kp = t(rows75), t(keypoints)
        self._setup(n, rows75, kp)
        st = capi.current_stream()
        if self.collision is not None and self.collision["follow_face"]:      # (before the jaw and the coefficients are set free)
            capi.check(lib.fdcap_opt_set_fit2d_collision_face(h, 1), "fdcap_opt_set_fit2d_collision_face")
        if self.fit_jaw:
            jaw0 = torch.zeros(n, 3, device=dev) if jaw_init is None else t(jaw_init)
            if tuple(jaw0.shape) != (n, 3):
                raise capi.FdcapError(f"expected jaw_init [{n},3]")
            capi.check(lib.fdcap_opt_set_jaw(h, capi.dptr(jaw0), st), "fdcap_opt_set_jaw")
        elif jaw_init is not None:
            raise capi.FdcapError("jaw_init belongs to fit_jaw")
        if self.fit_expression:
            expr0 = torch.zeros(n, NUM_EXPRESSION, device=dev) if expression_init is None else t(expression_init)
            if tuple(expr0.shape) != (n, NUM_EXPRESSION):
                raise capi.FdcapError(f"expected expression_init [{n},{NUM_EXPRESSION}]")
            capi.check(lib.fdcap_opt_set_expression(h, capi.dptr(expr0), st), "fdcap_opt_set_expression")
        elif expression_init is not None:
            raise capi.FdcapError("expression_init belongs to fit_expression")
        self.log, self.rounds, self.frame_iterations, self.frame_loss = [], [], [], []
        fx, fy, cx, cy = self.intrinsics
        for si, (w_data, w_pose, w_shape, w_hand) in enumerate(self.stages):
            if self.group_weights is not None:                 # this stage's confidences: the detector's times the groups' weights
                kps = kp.clone()
                kps[:, :, 2] *= torch.from_numpy(self.group_weights[si][self.group_of]).to(dev)
                capi.check(lib.fdcap_opt_set_keypoints_mapped(h, capi.dptr(kps), capi.current_stream()), "fdcap_opt_set_keypoints_mapped")
            sg = self._last_stage = capi.Fit2dStage(fx, fy, cx, cy, self.rho, w_data, w_pose, w_shape, w_hand)
            if self.bend_prior is not None or self.fit_jaw:
                self._set_extra(si, w_pose)
            if self.fit_expression:
                capi.check(lib.fdcap_opt_set_expression_prior(h, float(self.expression_prior[si])), "fdcap_opt_set_expression_prior")
            if self.collision is not None:                    # this stage's weight (0: the term is off, no launch)
                q = self.collision
                prm = capi.CollisionParams(q["sigma"], q["weights"][si], q["capacity"], 0)
                capi.check(lib.fdcap_opt_set_fit2d_collision(h, ctypes.byref(prm)), "fdcap_opt_set_fit2d_collision")
            if self.optimizer == "lbfgs":
                q = self.lbfgs
                cf = capi.LbfgsConfig(capi.XDIM, q["history"], q["max_iter"], q["max_eval"], q["max_steps"], q["max_ls"], q["lr"],
                                      q["tolerance_grad"], q["tolerance_change"], q["ftol"], q["gtol"])
                rounds = ctypes.c_int32(0)
                capi.check(lib.fdcap_opt_fit2d_lbfgs(h, ctypes.byref(sg), ctypes.byref(cf), self.max_rounds, ctypes.byref(rounds),
                                                     capi.current_stream()), "fdcap_opt_fit2d_lbfgs")
                self.rounds.append(int(rounds.value))
                it = torch.zeros(n, dtype=torch.int32, device=dev)
                fl = torch.zeros(n, device=dev)
                capi.check(lib.fdcap_opt_fit2d_lbfgs_stats(h, capi.dptr(it), None, capi.dptr(fl), capi.current_stream()),
                           "fdcap_opt_fit2d_lbfgs_stats")
                self.frame_iterations.append(it.cpu().numpy())      # per frame: L-BFGS directions taken in this stage
                self.frame_loss.append(fl.cpu().numpy())            # ... and the objective where it stopped
                if log_every:                                   # the objective where the stage ended
                    capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 1, capi.current_stream()), "fdcap_opt_backward_fit2d")
                    s = self._losses.cpu().numpy()
                    self.log.append([float(s[0]), float(s[1])])
                continue
            capi.check(lib.fdcap_opt_reset_adam(h, capi.current_stream()), "fdcap_opt_reset_adam")
            for it in range(self.iters_per_stage):
                st = capi.current_stream()
                do_log = bool(log_every) and it % log_every == 0
                capi.check(lib.fdcap_opt_backward_fit2d(h, ctypes.byref(sg), 1 if do_log else 0, st), "fdcap_opt_backward_fit2d")
                if do_log:
                    s = self._losses.cpu().numpy()
                    self.log.append([float(s[0]), float(s[1])])
                capi.check(lib.fdcap_opt_step_x(h, it + 1, st), "fdcap_opt_step_x")
        out = torch.empty(n, capi.PDIM, device=dev)
        capi.check(lib.fdcap_opt_get_results(h, capi.dptr(out), None, None, capi.current_stream()), "fdcap_opt_get_results")
        self.body_rotation_rec = self._rows_x[2:2 + n]
        if self.fit_jaw:
            self.jaw_pose = torch.empty(n, 3, device=dev)
            capi.check(lib.fdcap_opt_get_jaw(h, capi.dptr(self.jaw_pose), None, capi.current_stream()), "fdcap_opt_get_jaw")
        if self.fit_expression:
            self.expression = torch.empty(n, NUM_EXPRESSION, device=dev)
            capi.check(lib.fdcap_opt_get_expression(h, capi.dptr(self.expression), None, capi.current_stream()), "fdcap_opt_get_expression")
        return out

    def close(self):
        if getattr(self, "ctx", None) is not None:
            self.ctx.close()
            self.ctx = None
