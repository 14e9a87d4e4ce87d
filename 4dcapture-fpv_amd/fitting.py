"""FittingOP mirror: the reference's optimiser driver (global_optimization.py:141-188, :450-489,
:491-635, :637-653) over the fused HIP iteration (include/fdcap.h fdcap_opt_*).

Same constructor dictionaries, same `fitting(body_gpu, mode) -> (body_rec, scale, camera_ext)`
and `save_result(...)`.  Differences that are documented deviations, not behaviour changes:
clip length is free (the reference hard-codes 300), an empty outlier set is legal, the scene is
stored once, and log-only terms are evaluated only when logging is requested."""
from __future__ import annotations

import ctypes
import math
import os
import time
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

from . import capi, innerfit, io
from .dist import (FrameShard, agree_on, allgather_packed, allreduce_scalars, exchange_halos, same_on_all_ranks,
                   staged_collective)

# loss-total constants buried in fitting() (global_optimization.py:564, :570, :582)
PHASE_SPLIT = 0.8
PHASE1_CONTACT = 0.1
LOCAL_PHASE1_CONTACT = 0.2      # mode 'local' (:511)
LOCAL_SECOND_LOOP = 0.4         # int(0.4 * num_iter) iterations of cal_loss2 (:536)
PHASE1_SMOOTH = 1.0
PHASE2_WORLD = 1.0
PHASE2_SMOOTH = 0.5
SCALE_INIT = 1.8
OUTLIER_FACTOR = 1.8
VERBOSE_FLUSH = 50              # a verbose fit reads its device-side loss history back every this many logged iterations
# mode 'dct' (:41-45, :595-630)
BATCH_FRAME_NUM = 60            # frames per DCT window (:41)
DCT_NUM = 5                     # coefficients per trajectory (:43)
DCT_NUM_ITER = 10000            # forced inside fitting() (:596)
DCT_PHASE_SPLIT = 0.95          # (:601)
DCT_PHASE1_WEIGHT = 10.0        # loss = loss_dct*10 (:607)
DCT_PHASE2 = (0.0001, 0.5, 0.1)  # loss_dct, loss_rec, loss_contact (:620)

DEFAULT_FITTINGCONFIG = {
    "scene_verts_path": None, "camera_path": None, "human_model_path": "./models",
    "vposer_ckpt_path": "./vposer/", "init_lr_h": 0.005, "num_iter": 500, "batch_size": 1,
    "device": "cuda", "contact_id_folder": "./body_segments", "contact_part": ["L_Leg", "R_Leg"],
    "verbose": False,
}
# weight_reproj (not in the reference; 0 = off): the clip-level 2D-keypoint reprojection term, FittingOP.fitting(keypoints=...)
DEFAULT_LOSSCONFIG = {"weight_loss_rec": 1, "weight_loss_vposer": 0.001, "weight_contact": 0.1,
                      "weight_collision": 0.5, "weight_reproj": 0}


def first_phase2_iter(num_iter: int) -> int:
    """Smallest ii with not (ii < num_iter*0.8) (:564)."""
    return int(math.ceil(num_iter * PHASE_SPLIT - 1e-12))


def dct_first_phase2_iter(num_iter: int) -> int:
    """Mode 'dct': smallest ii with not (ii < num_iter*0.95) (:601)."""
    return int(math.ceil(num_iter * DCT_PHASE_SPLIT - 1e-9))


def is_logging_iteration(ii: int, num_iter: int, log_every: int) -> bool:
    """Every log_every-th iteration and the fit's last one (the reference prints every iteration: log_every = 1)."""
    return bool(log_every) and (ii % log_every == 0 or ii == num_iter - 1)


def stretch_end(ii: int, num_iter: int, log_every: int = 0, snapshot_at=frozenset(), check_finite_every: int = 0,
                checkpoint_every: int = 0, flush_every: int = 0, unflushed_rows: int = 0) -> int:
    """The loop runs inside the library (fdcap_opt_run) in stretches [ii, end): `end` is the number of iterations done when this
    side next has something to do -- a snapshot after `end` steps, a finite check or a checkpoint every k-th iteration (no
    checkpoint after the last one), or a read-back of the loss history once `flush_every` logged rows wait (0: never inside the
    loop; `unflushed_rows` wait already) -- else num_iter.  Pure host logic (tests/test_host_math.py)."""
    end, rows = ii, unflushed_rows
    while end < num_iter:
        end += 1
        logged = is_logging_iteration(end - 1, num_iter, log_every)
        rows += 1 if logged else 0
        if (end in snapshot_at or (check_finite_every and end % check_finite_every == 0) or
                (checkpoint_every and end % checkpoint_every == 0 and end < num_iter) or
                (flush_every and logged and rows >= flush_every)):
            break
    return end


def find_outliers(x78: np.ndarray):
    """init() :459-487.  x78 [N,78] fp32 (6D form).  Returns (idx1 outlier rows, pos nearest
    inlier for each, ties -> lower index).  Generalised from the hard-coded 300 to N."""
    x78 = np.asarray(x78, dtype=np.float32)
    n = x78.shape[0]
    z = x78[:, 19:51]
    stats = np.sum(z * z, axis=1, dtype=np.float32)
    avg = np.float32(np.sum(stats, dtype=np.float32) / np.float32(n))
    idx1 = np.where(stats > avg * np.float32(OUTLIER_FACTOR))[0]
    temp = np.ones(n)
    temp[idx1] = 0.0
    index_one = np.where(temp == 1)[0]
    index_zero = np.where(temp == 0)[0]
    if index_zero.size == 0 or index_one.size == 0:
        return idx1, np.zeros(0, dtype=np.int64)
    diff = np.abs(index_zero[:, None] - index_one[None, :])
    pos = index_one[np.argmin(diff, axis=1)]
    return idx1, pos


def clip_inputs(x78: np.ndarray):
    """init() :459-487 for one clip: x78 [N,78] fp32 (6D form) -> (idx1 outlier rows, init78 [N,78] = the data with every
    outlier row replaced by its nearest inlier's, mask [N] = 0 on the outliers)."""
    x78 = np.asarray(x78, dtype=np.float32)
    idx1, pos = find_outliers(x78)
    init78 = x78.copy()
    if idx1.size and pos.size:
        init78[idx1, :] = x78[pos, :]
    mask = np.ones(x78.shape[0], np.float32)
    mask[idx1] = 0.0
    return idx1, init78, mask


# ---- one function per printed row: the un-normalised partial sums s (losses_d, float64) of an n-frame clip -> the printed terms --------
MAIN_TERMS = ("l_rec", "l_vposer", "loss_smoothing", "loss_contact", "loss_world_smoothing", "total_loss")
LOCAL2_TERMS = ("l_rec", "loss_local_smoothing", "loss_smoothing", "loss_contact_smoothing", "total_loss")
DCT2_TERMS = ("l_rec", "l_vposer", "loss_smoothing", "loss_contact", "loss_dct", "total_loss")


def logged_losses(s, n, nc, weight_loss_rec, weight_loss_vposer, weight_contact, phase2, local=False):
    """One logged iteration of the main loop (:573-575, :587-589) as (l_rec, l_vposer, loss_smoothing, loss_contact,
    loss_world_smoothing, total)."""
    nc = max(nc, 1)
    l_rec = weight_loss_rec * s[0] / (n * capi.XDIM)
    l_vp = weight_loss_vposer * s[1] / (n * 32)
    l_sm = s[2] / ((n - 2) * capi.XDIM) if n >= 3 else float("nan")
    l_con = weight_contact * s[3] / (n * nc)
    l_ws = s[4] / ((n - 1) * 69) if n >= 2 else float("nan")
    total = (l_rec + (0.0 if local else PHASE2_WORLD * l_ws) + PHASE2_SMOOTH * l_sm) if phase2 else \
        ((LOCAL_PHASE1_CONTACT if local else PHASE1_CONTACT) * l_con + PHASE1_SMOOTH * l_sm + l_rec)
    return l_rec, l_vp, l_sm, l_con, l_ws, total


def reproj_loss(s, n, weight_reproj):
    """The reprojection term of one logged iteration from its un-normalised partial sum (slot capi.LOSS_REPROJ of losses_d):
    weight_reproj / (23 n) * sum conf^2 [GMoF + GMoF]; it joins the total of either phase with coefficient 1."""
    return weight_reproj * s[capi.LOSS_REPROJ] / (23 * n)


def check_keypoints(keypoints, num_body, intrinsics, rho):
    """The reprojection term's inputs, checked on the host -> (keypoints [num_body,23,3] float32, (fx, fy, cx, cy), rho)."""
    if keypoints is None:
        raise ValueError("weight_reproj is non-zero: fitting() needs keypoints [N,23,3] (u, v, confidence) in SMPL-X joint order")
    kp = np.ascontiguousarray(keypoints.detach().cpu().numpy() if hasattr(keypoints, "detach") else keypoints, dtype=np.float32)
    if kp.shape != (num_body, 23, 3):
        raise ValueError(f"keypoints must be [{num_body},23,3], got {kp.shape}")
    intr = tuple(float(v) for v in intrinsics)
    if len(intr) != 4 or not all(math.isfinite(v) for v in intr) or intr[0] <= 0 or intr[1] <= 0:
        raise ValueError(f"intrinsics must be finite (fx, fy, cx, cy) with positive focal lengths, got {intrinsics}")
    if not (math.isfinite(rho) and rho > 0):
        raise ValueError(f"rho must be finite and positive, got {rho}")
    return kp, intr, float(rho)


def local2_losses(s, n, num_verts, weight_loss_rec):
    """One logged iteration of mode 'local''s second loop (:404-429) as [l_rec, loss_local_smoothing, loss_smoothing,
    loss_contact_smoothing, total]; a mean over nothing (n = 2) is inf or NaN, without a warning."""
    n = np.float64(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        l_rec = weight_loss_rec * s[0] / (n * capi.XDIM)
        l_loc = s[2] / ((n - 2) * capi.XDIM)
        l_sm = s[5] / ((n - 2) * (3 * num_verts))
        l_cs = s[6]
        return [l_rec, l_loc, l_sm, l_cs, l_sm + l_loc + l_rec + l_cs]


def dct2_losses(s, n, W, nc, weight_loss_rec, weight_loss_vposer, weight_contact, weights=DCT_PHASE2):
    """One logged iteration of mode 'dct''s second phase (:620) of a clip of W windows as [l_rec, l_vposer, loss_smoothing,
    loss_contact, loss_dct, total]; `weights`: of (loss_dct, l_rec, loss_contact) in the total."""
    wd, wr, wc = weights
    nc = max(nc, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        l_rec = weight_loss_rec * s[0] / (n * capi.XDIM)
        l_vp = weight_loss_vposer * s[1] / (n * 32)
        l_sm = s[2] / ((n - 2) * capi.XDIM) if n >= 3 else float("nan")
        l_con = weight_contact * s[3] / (n * nc)
        l_dct = s[7] / (69 * W)
        return [l_rec, l_vp, l_sm, l_con, l_dct, wd * l_dct + wr * l_rec + wc * l_con]


@dataclass
class FitLog:
    """Per-logged-iteration losses in the reference's print order (:573-575, :587-589)."""
    iters: list = field(default_factory=list)
    l_rec: list = field(default_factory=list)
    l_vposer: list = field(default_factory=list)
    loss_smoothing: list = field(default_factory=list)
    loss_contact: list = field(default_factory=list)
    loss_world_smoothing: list = field(default_factory=list)
    total: list = field(default_factory=list)
    reproj: list = field(default_factory=list)      # loss_reproj per logged iteration, while the term is on (else empty)

    def append(self, ii, terms):
        """terms: the six of logged_losses"""
        self.iters.append(ii)
        for column, v in zip((self.l_rec, self.l_vposer, self.loss_smoothing, self.loss_contact, self.loss_world_smoothing, self.total), terms):
            column.append(v)


@dataclass
class _Fit:
    """What one FittingOP.fitting() call decided, handed to the loops that carry it out."""
    multi: bool                     # the sharded iteration tail (more than one rank, or FDCAP_FORCE_EXCHANGE)
    log_every: int
    ii0: int                        # first iteration to run (0, or where the resumed checkpoint left off)
    ck_every: int
    ck_path: str | None
    finite_every: int
    snapshot_at: frozenset
    resumed: dict                   # the mode's own arrays a resumed checkpoint carried (contact_weight; c_dct, dct_m, dct_v)


def _c_dct_start(c_dct_init, W, C, name="c_dct_init"):
    """One clip's start of c_dct [W,23,3,C] on the host: `c_dct_init`, or torch.randn as the reference draws it (:186)."""
    import torch
    c0 = torch.randn(W, 23, 3, C) if c_dct_init is None else torch.as_tensor(np.asarray(c_dct_init, dtype=np.float32).reshape(W, 23, 3, -1))
    if tuple(c0.shape) != (W, 23, 3, C):
        raise capi.FdcapError(f"{name} must be [{W},23,3,{C}], got {tuple(c0.shape)}")
    return c0


class _Fitter:
    """What FittingOP and ClipBatchFitter share: the configuration on attributes, the models, the contact ids and the context, and
    the library plumbing that does not depend on how the rows are laid out."""
    _n_left_from_files = True       # contact ids read from the parts' files: the left part's size is the first file's

    def __init__(self, fittingconfig, lossconfig, body_model, vposer, contact_ids, n_left, legacy_zero_grad, dct_num_iter):
        import torch
        for defaults, given in ((DEFAULT_FITTINGCONFIG, fittingconfig), (DEFAULT_LOSSCONFIG, lossconfig)):
            for k, v in {**defaults, **(given or {})}.items():
                setattr(self, k, v)
        self.legacy_zero_grad = bool(legacy_zero_grad)
        self.dct_num_iter = int(dct_num_iter)
        self._mode = "global"
        if not torch.cuda.is_available():
            raise capi.FdcapError("no HIP device: the fdcap_amd optimiser only runs on the GPU")
        self.device = torch.device("cuda", torch.cuda.current_device())
        if body_model is None or vposer is None:
            from . import assets
            body_model = body_model or assets.load_smplx_npz(self.human_model_path)
            vposer = vposer or assets.load_vposer_snapshot(self.vposer_ckpt_path)
        self.setup_s = {}
        self.ctx = self._timed("ctx_create", capi.Context, body_model, vposer)
        if contact_ids is None:
            parts = [io.read_contact_ids(self.contact_id_folder, [p]) for p in self.contact_part]
            contact_ids = np.concatenate(parts)
            if self._n_left_from_files:
                n_left = len(parts[0])
        self.vid = np.asarray(contact_ids, dtype=np.int64)
        # mode 'local' treats the two contact parts separately (L_Leg ids first, :341-347)
        self.n_left = int(n_left) if n_left is not None else len(self.vid) // 2

    def _timed(self, what, call, *args):
        """Host seconds of a registration call (each returns with its device work done) -> self.setup_s[what]: what a one-clip process
        pays before its first iteration -- bench.py publishes them as `setup` (the reference's counterpart: __init__, :142-188)."""
        t0 = time.perf_counter()
        out = call(*args)
        self.setup_s[what] = time.perf_counter() - t0
        return out

    def _opt_config(self, n_total, n_local, frame0):
        """The library's configuration for self._mode: mode 'local' has its own first-loop weights (:511, :523), 'dct' mode 'global''s."""
        local = self._mode == "local"
        return capi.OptConfig(n_total, n_local, frame0, float(self.init_lr_h), float(self.weight_loss_rec),
                              float(self.weight_loss_vposer), float(self.weight_contact),
                              LOCAL_PHASE1_CONTACT if local else PHASE1_CONTACT, PHASE1_SMOOTH,
                              0.0 if local else PHASE2_WORLD, PHASE2_SMOOTH, SCALE_INIT, int(self.legacy_zero_grad))

    def _new_state(self, rows, K, losses_shape):
        """The optimiser's state -- `rows` rows (two halo rows either side included) of K clips -- is owned here (torch tensors) and
        registered with the library, so the same storage is what RCCL exchanges / reduces -> the five pointers fdcap_opt_create* take."""
        import torch
        dev = self.device
        self._rows_x, self._rows_cam = torch.zeros(rows, capi.XDIM, device=dev), torch.zeros(rows, 16, device=dev)
        self._scale, self._dscale = torch.zeros(K, device=dev), torch.zeros(K, device=dev)
        self._losses = torch.zeros(*losses_shape, device=dev, dtype=torch.float64)
        torch.cuda.current_stream().synchronize()
        return [capi.dptr(t) for t in (self._rows_x, self._rows_cam, self._scale, self._dscale, self._losses)]

    def _results(self, rows, K):
        """fdcap_opt_get_results -> (body_rec [rows,75], scale [K], camera_ext [rows,16]), fresh device tensors"""
        import torch
        body_rec = torch.empty(rows, capi.PDIM, device=self.device)
        scale = torch.empty(K, device=self.device)
        cam = torch.empty(rows, 16, device=self.device)
        capi.check(self.ctx.lib.fdcap_opt_get_results(self.ctx.handle, capi.dptr(body_rec), capi.dptr(scale), capi.dptr(cam),
                                                      capi.current_stream()), "fdcap_opt_get_results")
        return body_rec, scale, cam

    def _opt_run(self, ii, end, P, log_every, rows, multi=False):
        """Iterations ii .. end-1 of the main loop as ONE fdcap_opt_run; `rows`: the history rows of their logging iterations
        (None: none logs).  FDCAP_DEFER_STEP=0: every optimiser step as its own launch (A/B; the same bits either way)."""
        flags = (0 if os.environ.get("FDCAP_DEFER_STEP", "1") != "0" else 1) | (2 if multi else 0)
        n_rows, n_done = 0 if rows is None else rows.shape[0], ctypes.c_int32(0)
        capi.check(self.ctx.lib.fdcap_opt_run(self.ctx.handle, ii, end, int(self.num_iter), P, int(log_every or 0), capi.dptr(rows), n_rows, flags,
                                              ctypes.byref(n_done), capi.current_stream()), "fdcap_opt_run")
        assert n_done.value == n_rows

    def _dct_state(self, W, C):
        """c_dct [W,69*C] with its two Adam moments, read from the device"""
        import torch
        lib, h, st = self.ctx.lib, self.ctx.handle, capi.current_stream()
        cd = torch.empty(W, 69 * C, device=self.device)
        dm, dv = torch.empty_like(cd), torch.empty_like(cd)
        capi.check(lib.fdcap_opt_get_dct(h, capi.dptr(cd), st), "fdcap_opt_get_dct")
        capi.check(lib.fdcap_opt_get_dct_state(h, capi.dptr(dm), capi.dptr(dv), st), "fdcap_opt_get_dct_state")
        return {"c_dct": cd, "dct_m": dm, "dct_v": dv}


class FittingOP(_Fitter):
    def __init__(self, fittingconfig, lossconfig, num_body, body_model=None, vposer=None, scene_verts=None,
                 contact_ids=None, camera_ext=None, group=None, legacy_zero_grad=False, n_left=None,
                 dct_mtx=None, c_dct_init=None, dct_num_iter=DCT_NUM_ITER):
        """`body_model` / `vposer`: objects with the SMPL-X npz / VPoser state-dict arrays
        (synth.BodyModelData / synth.VPoserData or assets.load_*).  `scene_verts`, `contact_ids`,
        `camera_ext` override the paths in `fittingconfig` when given (synthetic runs).
        `dct_mtx` [60,5]: load_dct_base() (:131-136; default: `fittingconfig['dct_mat_path']` if that .mat
        exists, else the orthonormal DCT-II basis); `c_dct_init` [N//60,23,3,5]: start of c_dct (the
        reference draws torch.randn, :186 -- so does the default); `dct_num_iter`: the 10000 of :596.
        `group`: torch.distributed process group for frame sharding (None = single GPU);
        `num_body` is the clip length N (the reference's batch_size = num_body, :152)."""
        super().__init__(fittingconfig, lossconfig, body_model, vposer, contact_ids, n_left, legacy_zero_grad, dct_num_iter)
        self.snapshot_hook = None      # tools: called with k right after the snapshot of step k was taken (`fitting(snapshot_at=...)`)
        self.batch_size = self.num_body = int(num_body)
        if scene_verts is None and self.scene_verts_path:
            scene_verts = io.read_scene_points(self.scene_verts_path)
        if scene_verts is None:
            scene_verts = np.zeros((0, 3), np.float32)
        self._timed("set_scene", self.ctx.set_scene, scene_verts)
        self._timed("set_contact_ids", self.ctx.set_contact_ids, self.vid)
        if camera_ext is None and self.camera_path:
            camera_ext = io.read_camerapose(self.camera_path)
        self._camera_ext_init = None if camera_ext is None else np.asarray(camera_ext, np.float32).reshape(-1, 4, 4)
        self.shard = FrameShard(self.num_body, group)
        self.group = group
        # The exchange inside the library (fdcap_comm_* / fdcap_opt_exchange: RCCL on the compute stream, two C calls per
        # iteration) whenever the group runs over RCCL; FDCAP_C_COMM=0 keeps torch.distributed's collectives (the path the
        # gloo tests -- ranks sharing one GPU, which RCCL refuses -- always take).
        self._c_comm = False
        if group is not None:
            import torch.distributed as dist
            if dist.get_backend(group) == "nccl":
                if agree_on(self.shard, int(os.environ.get("FDCAP_C_COMM", "1") != "0")):      # (rank 0's setting, for everyone)
                    self._init_c_comm()
        self.dct_mtx = None if dct_mtx is None else np.ascontiguousarray(dct_mtx, dtype=np.float32)
        self._c_dct_init = c_dct_init
        self.c_dct = self.scale = self.camera_ext = self.body_rotation_rec = self.log = self.idx1 = None     # (a fit's results)

    def _init_c_comm(self):
        """Rank 0 draws the RCCL unique id, torch.distributed carries it to the other ranks (the out-of-band channel any
        launcher has), every rank joins the library's own communicator.  Whether the library's exchange is used is ONE decision
        for the whole group (a rank on the other path would issue other collectives and hang its peers): every step that can
        fail on one rank alone -- binding librccl, creating the communicator, a first sum over it -- is followed by an
        agreement over torch.distributed, and any failure anywhere sends every rank to torch.distributed's collectives
        (RCCL as well; same kernels either side of the all-gather, same results), with a warning on rank 0."""
        import warnings
        import torch
        import torch.distributed as dist
        lib, h = self.ctx.lib, self.ctx.handle
        sh = self.shard

        def all_ok(rc, what):
            lo, hi = same_on_all_ranks(sh, int(rc))
            if lo == 0 and hi == 0:
                return True
            if sh.rank == 0:
                why = lib.fdcap_comm_last_error(h) or b""
                warnings.warn(f"fdcap: {what} failed on some rank (codes {lo}..{hi}; this rank: {rc} {why.decode()!r}); "
                              "using torch.distributed's collectives instead")
            return False

        idb = (ctypes.c_uint8 * 128)()
        rc = lib.fdcap_comm_unique_id(idb)                  # (every rank: this is where librccl is bound; only rank 0's id is used)
        if not all_ok(rc, "binding librccl (fdcap_comm_unique_id)"):
            return
        t = torch.tensor(list(idb), dtype=torch.uint8, device=self.device)
        dist.broadcast(t, src=sh.global_rank(0), group=self.group)
        idb = (ctypes.c_uint8 * 128)(*t.cpu().tolist())
        rc = lib.fdcap_comm_create(h, idb, sh.rank, sh.world)
        if not all_ok(rc, "fdcap_comm_create"):
            lib.fdcap_comm_destroy(h)
            return
        # first use: sum of (rank + 1) over the communicator, on every rank
        probe = torch.tensor([float(sh.rank + 1)], dtype=torch.float64, device=self.device)
        rc = lib.fdcap_comm_allreduce_f64(h, capi.dptr(probe), 1, capi.current_stream())
        got = float(probe.item()) if rc == 0 else -1.0
        if not all_ok(rc if rc else int(got != sh.world * (sh.world + 1) / 2), "the first all-reduce over the library's communicator"):
            lib.fdcap_comm_destroy(h)
            return
        self._c_comm = True

    def _halos(self):
        """Halo rows <- the neighbouring ranks' boundary rows as they are."""
        if self._c_comm:
            capi.check(self.ctx.lib.fdcap_opt_halo_exchange(self.ctx.handle, capi.current_stream()), "fdcap_opt_halo_exchange")
        else:
            exchange_halos(self.shard, self._rows_x, self._rows_cam)

    def _sum_over_ranks(self, t64):
        """In-place sum of a float64 device tensor over the ranks (logged loss partial sums)."""
        import torch
        if self._c_comm:
            capi.check(self.ctx.lib.fdcap_comm_allreduce_f64(self.ctx.handle, capi.dptr(t64), t64.numel(), capi.current_stream()),
                       "fdcap_comm_allreduce_f64")
        else:
            allreduce_scalars(self.shard, torch.zeros(1, device=self.device), t64)

    # ---- :450-489 -------------------------------------------------------------------------
    def init(self, body_data_rotation):
        """body_data_rotation: [N,78] device tensor (whole clip).  Host-side index logic on a
        copy; returns idx1 like the reference and stages the optimiser's inputs."""
        import torch
        x78 = body_data_rotation.detach().cpu().numpy()
        idx1, init78, mask = clip_inputs(x78)
        if self._camera_ext_init is None or self._camera_ext_init.shape[0] != self.num_body:
            raise capi.FdcapError("camera_ext / camerapose.txt must have one pose per frame (:455)")
        sh = self.shard
        lo, hi = sh.frame0, sh.frame0 + sh.n_local
        oc = self._opt_config(self.num_body, sh.n_local, sh.frame0)
        lib = self.ctx.lib
        dev = self.device
        capi.check(lib.fdcap_opt_create(self.ctx.handle, ctypes.byref(oc), *self._new_state(sh.n_local + 4, 1, (capi.NUM_LOSSES,))), "fdcap_opt_create")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_data, d_init = body_data_rotation[lo:hi].contiguous(), t(init78[lo:hi])
        d_mask, d_cam = t(mask[lo:hi]), t(self._camera_ext_init[lo:hi].reshape(-1, 16))
        st = capi.current_stream()
        capi.check(lib.fdcap_opt_set_inputs(self.ctx.handle, capi.dptr(d_data), capi.dptr(d_init), capi.dptr(d_mask),
                                            capi.dptr(d_cam), st), "fdcap_opt_set_inputs")
        torch.cuda.current_stream().synchronize()
        self._halos()
        xl = int(lib.fdcap_exchange_len())
        self._xch_send = torch.zeros(xl, device=dev)
        self._xch_all = torch.zeros(self.shard.world, xl, device=dev)
        self.idx1 = idx1
        return idx1

    # ---- :491-635 -------------------------------------------------------------------------
    def fitting(self, body_data, mode="global", log_every=0, checkpoint_every=0, checkpoint_path=None, resume=None,
                check_finite_every=0, snapshot_at=(), keypoints=None, intrinsics=innerfit.DEFAULT_INTRINSICS, rho=100.0):
        """body_data: [N,75] (device tensor or numpy), SMPLify-X layout (:64-76).
        Returns (body_rec [N_local,75] device tensor, scale numpy scalar, camera_ext [N_local,4,4])
        -- the whole clip when not sharded, exactly the reference's triple (:635).
        Not in the reference:
          checkpoint_every=k, checkpoint_path: after every k-th iteration write parameters + Adam moments to
            `checkpoint_path` (sharded runs: one file per rank, suffix .rank<r>).  All three modes (r5): mode 'local' counts its
            second loop's iterations on from num_iter and keeps detect_contact's weights in the file; mode 'dct' counts the
            iterations of its own budget (`dct_num_iter`, the 10000 of :596), cuts the one-launch first phase at the checkpoint
            iterations and keeps c_dct with its Adam moments (with log_every: k must be a multiple of it);
          resume=path: continue such a run from where the file left off -- bit-identical to the uninterrupted run;
          check_finite_every=k: every k iterations count the non-finite parameters on the device and raise if any
            (the opt-in counterpart of the reference's set_detect_anomaly(True), :561); all three modes -- mode 'dct' checks the
            DCT coefficients and their Adam moments through its first phase (every lcm(k, log_every) iterations there), the body
            parameters from then on;
          snapshot_at=(k, ...) (mode 'global'): after the k-th optimiser step keep device copies of (body_rotation_rec [N_local,78],
            scale, camera_ext [N_local,16]) in self.snapshots[k] -- no host sync; for trajectory comparisons (tests/test_gpu_parity500.py).
          keypoints=[N,23,3] (u, v, confidence; SMPL-X joint order, the whole clip on every rank; innerfit.joints23_from_openpose),
            intrinsics=(fx, fy, cx, cy), rho: with lossconfig['weight_reproj'] != 0 (mode 'global' only) the loss total of both phases
            gains weight_reproj / (23 N) * sum conf^2 GMoF_rho(keypoint - projection) on the body joints in the camera frame (DESIGN.md
            section 5.7); the logged value is kept in self.log.reproj and printed as a trailing loss_reproj.  Keypoints are an input,
            not state: a resumed fit is handed them again.  With weight_reproj == 0 they are ignored and nothing changes.
        Sharded runs: every argument of this call and `num_iter` must be the same on all ranks (they decide which collectives
        are issued).  `verbose` may differ -- prints come from rank 0 only, and rank 0's flag alone decides whether the loss
        history is read back (all-reduced) during the loop, so a rank-0-only verbose run is legal."""
        import torch
        if mode not in ("global", "local", "dct"):
            raise ValueError("mode must be 'local', 'global' or 'dct' (global_optimization.py:660)")
        snapshot_at = frozenset(int(k) for k in snapshot_at)
        self.snapshots = {}
        if snapshot_at and mode != "global":
            raise ValueError("snapshot_at is implemented for mode 'global'")
        if checkpoint_every and not checkpoint_path:
            raise ValueError("checkpoint_every needs checkpoint_path")
        self._reproj = None
        if float(self.weight_reproj) != 0.0:                 # (all of it on the host, before anything touches the device)
            if mode != "global":
                raise ValueError("weight_reproj: the reprojection term is implemented for mode 'global'")
            if not (math.isfinite(float(self.weight_reproj)) and float(self.weight_reproj) > 0):
                raise ValueError(f"weight_reproj must be finite and positive (0: off), got {self.weight_reproj}")
            self._reproj = check_keypoints(keypoints, self.num_body, intrinsics, rho)
        if mode == "dct" and checkpoint_every and log_every and checkpoint_every % log_every:
            raise ValueError("mode 'dct': checkpoint_every must be a multiple of log_every (the first phase's objective history is "
                             "written by the launch itself, every log_every-th iteration counted from the launch's first)")
        self._mode = mode
        dev = self.device
        if not torch.is_tensor(body_data):
            body_data = torch.from_numpy(np.ascontiguousarray(body_data, dtype=np.float32))
        body_data = body_data.to(dev, torch.float32).contiguous()
        n = body_data.shape[0]
        if n != self.num_body:
            raise capi.FdcapError(f"body_data has {n} frames, FittingOP was built for {self.num_body}")
        x78 = torch.empty(n, capi.XDIM, device=dev)
        capi.check(self.ctx.lib.fdcap_params_75_to_78(capi.dptr(body_data), n, capi.dptr(x78), capi.current_stream()), "fdcap_params_75_to_78")
        self.init(x78)                                                                      # :495
        ii0, resumed = self._load_checkpoint(resume) if resume else (0, {})
        if self._reproj is not None:
            self._set_reproj(*self._reproj)
        # FDCAP_FORCE_EXCHANGE=1: run the sharded iteration tail (pack -> all-gather -> unpack) even on a one-rank
        # group -- lets a single-GPU box exercise the RCCL calls of the multi-GPU path
        multi = self.shard.world > 1 or (self.group is not None and os.environ.get("FDCAP_FORCE_EXCHANGE") == "1")
        fit = _Fit(multi, log_every, ii0, int(checkpoint_every), checkpoint_path, int(check_finite_every), snapshot_at, resumed)
        # FDCAP_XCH_OVERLAP=1: the forward ahead of the exchange from the first iteration on (_per_iteration_issuer)
        self.exchange_overlap = multi and os.environ.get("FDCAP_XCH_OVERLAP", "auto") == "1" and not self._c_comm
        if mode == "dct":
            log = FitLog()
            self._dct_loops(fit)
        else:
            log = self._main_loop(fit)
            if mode == "local":
                self._local_second_loop(fit)
        nl = self.shard.n_local
        body_rec, scale, cam = self._results(nl, 1)
        self.scale = scale
        self.camera_ext = cam.view(nl, 4, 4)
        self.body_rotation_rec = self._rows_x[2:2 + nl]
        self.log = log
        return body_rec, scale.detach().cpu().numpy().squeeze(), self.camera_ext

    # ---- the main loop of modes 'global' and 'local' (:558-593) -----------------------------------------------------------------
    def _main_loop(self, fit):
        """Iterations [fit.ii0, num_iter) -> their FitLog.  The loop runs in stretches [ii, end) between two things THIS side has to
        do -- a verbose flush, a snapshot, a finite check, a checkpoint; none of them in a plain fit: one stretch for all 500.
        The reference prints every loss term in every iteration (:573-575, :587-589) with five .item() syncs.  Here the
        partial sums of a logging iteration are written into a device-side history row (no host sync inside the loop) and
        read back -- and, when sharded, all-reduced -- after the last iteration (a verbose fit: in batches of VERBOSE_FLUSH logged
        iterations, to show its progress)."""
        import torch
        lib, h = self.ctx.lib, self.ctx.handle
        num_iter, log_every, multi = self.num_iter, fit.log_every, fit.multi
        P = first_phase2_iter(num_iter)
        log = FitLog()
        # in-loop read-backs of the loss history are collectives when sharded: one flag for the whole group (rank 0's)
        flush_in_loop = bool(agree_on(self.shard, 1 if self.verbose else 0)) if multi else bool(self.verbose)
        is_log = lambda i: is_logging_iteration(i, num_iter, log_every)
        if log_every:
            hist = torch.zeros(max(sum(1 for i in range(fit.ii0, num_iter) if is_log(i)), 1), capi.NUM_LOSSES, device=self.device, dtype=torch.float64)
        logged = []
        flushed = 0

        def flush(upto):
            # history rows [flushed, upto) -> log entries (and the reference's per-iteration print when verbose)
            nonlocal flushed
            if upto <= flushed:
                return
            part = hist[flushed:upto]
            if multi:
                part = part.clone()
                self._sum_over_ranks(part)
            rows = part.cpu().numpy()
            for k in range(upto - flushed):
                self._append_log(log, logged[flushed + k], logged[flushed + k] >= P, rows[k])
            flushed = upto

        # A stretch is ONE library call (fdcap_opt_run) wherever the iteration is C calls only: one rank, or ranks exchanging through
        # the library's communicator.  FDCAP_C_LOOP=0 keeps the calls of the single iterations (the same, in the same order: same bits).
        c_loop = os.environ.get("FDCAP_C_LOOP", "1") != "0" and (not multi or self._c_comm)
        issue = (lambda ii, end, rows: self._opt_run(ii, end, P, log_every, rows, multi)) if c_loop else self._per_iteration_issuer(fit, P)
        ii = fit.ii0
        try:
            while ii < num_iter:
                # the stretch [ii, end): ends after the first iteration that leaves this side something to do
                end = stretch_end(ii, num_iter, log_every, fit.snapshot_at, fit.finite_every, fit.ck_every,
                                  VERBOSE_FLUSH if flush_in_loop else 0, len(logged) - flushed)
                rows = [i for i in range(ii, end) if is_log(i)]
                issue(ii, end, hist[len(logged):len(logged) + len(rows)] if rows else None)
                logged.extend(rows)
                if flush_in_loop and is_log(end - 1) and len(logged) - flushed >= VERBOSE_FLUSH:
                    flush(len(logged))
                if end in fit.snapshot_at:
                    capi.check(lib.fdcap_opt_sync(h, capi.current_stream()), "fdcap_opt_sync")      # (applies a deferred step first)
                    nl = self.shard.n_local
                    self.snapshots[end] = (self._rows_x[2:2 + nl].clone(), self._scale.clone(), self._rows_cam[2:2 + nl].clone())
                    if self.snapshot_hook:
                        self.snapshot_hook(end)
                if fit.finite_every and end % fit.finite_every == 0:
                    self._check_finite(end - 1)
                if fit.ck_every and end % fit.ck_every == 0 and end < num_iter:
                    self._save_checkpoint(fit.ck_path, end)
                ii = end
        finally:
            # never leave the library pointing into `hist` (freed with this frame if the loop raised).  (After fdcap_opt_run, which
            # re-registers the old output itself, there have always been two of these calls: tests/driver_trace.json pins them)
            for _ in range((2 if c_loop else 1) if logged else 0):
                capi.check(lib.fdcap_opt_set_loss_output(h, capi.dptr(self._losses)), "fdcap_opt_set_loss_output")
        flush(len(logged))
        return log

    def _per_iteration_issuer(self, fit, P):
        """-> issue(ii, end, rows): iterations ii .. end-1 call by call (the arguments of _opt_run, which issues them as one)."""
        import torch
        lib, h = self.ctx.lib, self.ctx.handle
        num_iter, log_every, multi = self.num_iter, fit.log_every, fit.multi
        defer = os.environ.get("FDCAP_DEFER_STEP", "1") != "0"
        # Forward ahead of the exchange (fdcap_opt_forward_ahead): FDCAP_XCH_OVERLAP=1 always, =0 never; otherwise the rank
        # times eight iterations of either schedule early in phase 1 and keeps the faster one.  The two give the same bits,
        # and the choice is local to a rank (the collective is the same call either way).  Why not simply "always": handing
        # work between the collective's stream and this one costs ~17 us per iteration on a one-rank RCCL group
        # (tools/host_issue_probe.py), so the overlap only pays when the all-gather takes longer than that to come back.
        # (The library's own exchange runs on the compute stream: nothing to overlap.)
        overlap = self.exchange_overlap
        tune = None
        if multi and not self._c_comm and os.environ.get("FDCAP_XCH_OVERLAP", "auto") not in ("0", "1") and fit.ii0 + 18 <= min(P, num_iter):
            tune = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

        def issue(first, end, rows):
            nonlocal overlap, tune
            n_logged = 0
            for ii in range(first, end):                                                     # :560
                do_log = is_logging_iteration(ii, num_iter, log_every)
                st = capi.current_stream()
                if tune is not None:                     # iterations ii0+2..9 plain, ii0+10..17 with the forward ahead
                    k = ii - fit.ii0
                    if k in (2, 10, 18):
                        tune[(k - 2) // 8].record()
                    if k == 10:
                        overlap = True
                    elif k == 18:
                        tune[2].synchronize()
                        overlap = tune[1].elapsed_time(tune[2]) < 0.97 * tune[0].elapsed_time(tune[1])
                        self.exchange_overlap = overlap
                        tune = None
                if do_log:                               # this iteration's partial sums go straight into their history row
                    capi.check(lib.fdcap_opt_set_loss_output(h, capi.dptr(rows[n_logged])), "fdcap_opt_set_loss_output")
                    n_logged += 1
                if defer and not multi and ii + 1 < num_iter:
                    # loss.backward() + optimizer.step() in one call, the step without a launch of its own (fdcap.h): `scale` (and a
                    # logging iteration's printed sums) ride in the backward's last launch, the rows are stepped by the next
                    # iteration's first two launches; whoever reads the registered tensors before that calls fdcap_opt_sync first
                    # (the snapshots; export_state does it itself)
                    capi.check(lib.fdcap_opt_backward_and_step(h, ii, P, 2 if do_log else 0, st), "fdcap_opt_backward_and_step")
                    continue
                # (2: the logged sums are delivered by the step launch that follows -- one launch less per logged iteration)
                capi.check(lib.fdcap_opt_backward(h, ii, P, 2 if do_log else 0, st), "fdcap_opt_backward")
                ahead = None
                if overlap and ii + 1 < num_iter:
                    # the next iteration's decoder / pose state / blend product of the owned rows need neither `scale`
                    # nor the halo rows: they run while the messages travel
                    def ahead(ii=ii, st=st):
                        capi.check(lib.fdcap_opt_forward_ahead(h, ii + 1, P, 2 if is_logging_iteration(ii + 1, num_iter, log_every) else 0, st),
                                   "fdcap_opt_forward_ahead")
                self._step(fit, ii, P, ahead)
        return issue

    def _step(self, fit, ii, P, ahead=None):
        """After the backward of iteration ii of a loop whose second phase begins at P: the optimiser step.  `ahead`: enqueues work
        that needs nothing of the exchange, for the time the messages travel (torch.distributed's collectives only)."""
        lib, h, sh, st = self.ctx.lib, self.ctx.handle, self.shard, capi.current_stream()
        if fit.multi and self._c_comm:
            # the tail inside the library: Adam on the rows + message, ncclAllGather on this stream, unpack + scale
            capi.check(lib.fdcap_opt_exchange(h, ii, P, st), "fdcap_opt_exchange")
        elif fit.multi:
            # one collective per iteration: boundary rows (after Adam) + the scale-gradient partial travel
            # together; every rank then sums the partials in rank order and steps `scale` identically
            capi.check(lib.fdcap_opt_step_rows_and_pack(h, ii, P, capi.dptr(self._xch_send), st), "step_rows_and_pack")
            allgather_packed(sh, self._xch_send, self._xch_all, ahead)
            capi.check(lib.fdcap_opt_unpack_and_step_scale(h, ii, P, capi.dptr(self._xch_all), sh.rank, sh.world, st),
                       "unpack_and_step_scale")
        else:
            capi.check(lib.fdcap_opt_step(h, ii, P, st), "fdcap_opt_step")

    def _set_reproj(self, kp, intr, rho):
        """fdcap_opt_set_reproj with this rank's keypoint rows (after init(): every fdcap_opt_create switches the term off)"""
        import torch
        sh = self.shard
        d_kp = torch.from_numpy(kp[sh.frame0:sh.frame0 + sh.n_local]).to(self.device)
        par = capi.ReprojParams(*intr, rho, float(self.weight_reproj))
        capi.check(self.ctx.lib.fdcap_opt_set_reproj(self.ctx.handle, ctypes.byref(par), capi.dptr(d_kp), capi.current_stream()), "fdcap_opt_set_reproj")
        torch.cuda.current_stream().synchronize()           # (d_kp is copied by then)

    def _append_log(self, log, ii, phase2, s):
        terms = logged_losses(s, self.num_body, self.ctx.num_contact, self.weight_loss_rec, self.weight_loss_vposer, self.weight_contact,
                              phase2, self._mode == "local")
        names = list(MAIN_TERMS)
        if getattr(self, "_reproj", None) is not None:      # the total gains the term, the row one more trailing field
            l_rp = reproj_loss(s, self.num_body, float(self.weight_reproj))
            terms = terms[:5] + (terms[5] + l_rp, l_rp)
            names.append("loss_reproj")
            log.reproj.append(l_rp)
        log.append(ii, terms[:6])
        shown = [0, 1, 2, 3, 4, 5] if phase2 else [0, 1, 2, 3, 5]         # (phase 1 prints no loss_world_smoothing, :573-575)
        shown += [6] if len(terms) > 6 else []
        self._print_row(ii, [names[k] for k in shown], [terms[k] for k in shown])

    def _print_row(self, ii, names, values):
        """the reference's per-iteration print, from rank 0 of a verbose fit"""
        if self.verbose and self.shard.rank == 0:
            print('[INFO][fitting] iter={:d}, '.format(ii) + ', '.join('{}={:f}'.format(k, v) for k, v in zip(names, values)))

    def _logged_sums(self, fit):
        """the partial sums the last backward logged, summed over the ranks, on the host (one sync)"""
        import torch
        s = self._losses.clone()
        if fit.multi:
            allreduce_scalars(self.shard, torch.zeros(1, device=self.device), s)
        return s.cpu().numpy()

    # ---- checkpoint / resume / finite check (not in the reference) ---------------------
    def _ckpt_file(self, path):
        return path if self.shard.world == 1 else f"{path}.rank{self.shard.rank}"

    def _budget(self):
        """the iteration budget a checkpoint belongs to (mode 'dct' runs its own, :596)"""
        return int(self.dct_num_iter if self._mode == "dct" else self.num_iter)

    def _save_checkpoint(self, path, next_iter, extra_fn=None, **extra):
        """`extra_fn`: callable returning more arrays for the file (mode 'dct': c_dct and its moments, read from the device).
        EVERYTHING that can fail on one rank alone -- the allocation, the library's state export, the extras' read-back, the
        write -- runs inside the try whose outcome the ranks then agree on (a HIP error or an out-of-memory in the
        export used to raise before the agreement and leave the peers waiting in it)."""
        import torch
        lib, h, nl = self.ctx.lib, self.ctx.handle, self.shard.n_local
        fn = self._ckpt_file(path)
        tmp = fn + ".tmp.npz"
        err = None
        try:
            state = torch.empty(int(lib.fdcap_opt_state_len(h)), device=self.device)
            capi.check(lib.fdcap_opt_export_state(h, capi.dptr(state), capi.current_stream()), "fdcap_opt_export_state")   # (applies a deferred step first)
            if extra_fn is not None:
                extra = dict(extra, **extra_fn())
            np.savez(tmp, next_iter=np.int64(next_iter), num_iter=np.int64(self._budget()), n_total=np.int64(self.num_body),
                     frame0=np.int64(self.shard.frame0), n_local=np.int64(nl), rows_x=self._rows_x[2:2 + nl].cpu().numpy(),
                     rows_cam=self._rows_cam[2:2 + nl].cpu().numpy(), scale=self._scale.cpu().numpy(), state=state.cpu().numpy(),
                     mode=np.array(self._mode),
                     **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in extra.items()})
        except Exception as e:  # noqa: BLE001 -- agreed on below: one rank's failed write must not leave its peers in a collective
            err = e
        # sharded: nobody replaces its file before every rank has written its new one (a crash during the writes leaves the
        # previous, mutually consistent set); a crash between the renames is caught on resume (next_iter must agree).  The
        # agreement doubles as that barrier AND carries every rank's outcome (a bare barrier turned one rank's
        # disk-full exception into a group hang): any failure anywhere -> nobody renames, everybody raises.
        lo, hi = same_on_all_ranks(self.shard, 0 if err is None else 1)
        if hi != 0:
            try:
                os.remove(tmp)
            except OSError:
                pass
            if err is not None:
                raise err
            raise capi.FdcapError(f"checkpoint for iteration {next_iter}: another rank could not write its file; none was replaced")
        os.replace(tmp, fn)                                      # (a crash mid-write leaves the previous checkpoint intact)

    def _load_checkpoint(self, path):
        """After init(): parameters and Adam moments <- the file; returns (the iteration to continue with, the mode's own arrays in
        the file -- contact_weight; c_dct, dct_m, dct_v)."""
        import torch
        lib, h, nl = self.ctx.lib, self.ctx.handle, self.shard.n_local
        with np.load(self._ckpt_file(path)) as ck:
            if (int(ck["n_total"]), int(ck["frame0"]), int(ck["n_local"]), int(ck["num_iter"])) != \
                    (self.num_body, self.shard.frame0, nl, self._budget()):
                raise capi.FdcapError("checkpoint was written for another clip length / sharding / iteration budget")
            ck_mode = str(ck["mode"]) if "mode" in ck.files else "global"
            if ck_mode != self._mode:
                raise capi.FdcapError(f"checkpoint was written by a mode {ck_mode!r} fit, this is mode {self._mode!r}")
            extra = {k: np.array(ck[k]) for k in ("contact_weight", "c_dct", "dct_m", "dct_v") if k in ck.files}
            t = lambda k: torch.from_numpy(np.ascontiguousarray(ck[k], dtype=np.float32)).to(self.device)
            self._rows_x[2:2 + nl] = t("rows_x")
            self._rows_cam[2:2 + nl] = t("rows_cam")
            self._scale.copy_(t("scale"))
            state = t("state").contiguous()
            nxt = int(ck["next_iter"])
        if state.numel() != int(lib.fdcap_opt_state_len(h)):
            raise capi.FdcapError("checkpoint state has the wrong size")
        lo, hi = same_on_all_ranks(self.shard, nxt)
        if lo != hi:
            raise capi.FdcapError(f"the ranks' checkpoint files are from different iterations ({lo} .. {hi}): a run died between "
                                  f"two ranks' writes; resume from an older, complete set")
        capi.check(lib.fdcap_opt_import_state(h, capi.dptr(state), capi.current_stream()), "fdcap_opt_import_state")
        torch.cuda.current_stream().synchronize()
        self._halos()
        return nxt, extra

    def _check_finite(self, ii):
        import torch
        cnt = torch.zeros(1, device=self.device, dtype=torch.int32)
        capi.check(self.ctx.lib.fdcap_opt_check_finite(self.ctx.handle, capi.dptr(cnt), capi.current_stream()), "fdcap_opt_check_finite")
        bad = int(cnt.cpu())
        if self.shard.world > 1:
            t = torch.tensor([float(bad)], device=self.device)
            allreduce_scalars(self.shard, t)
            bad = int(t.cpu())
        if bad:
            raise capi.FdcapError(f"{bad} non-finite optimiser parameters after iteration {ii}")

    # ---- mode 'dct' (:595-630) ---------------------------------------------------------------
    def _dct_loops(self, fit):
        """mode 'dct'.  First 95 % of the iterations: only c_dct moves (loss_dct*10, :601-607) against frozen
        joint trajectories -- ONE launch; iteration ceil(0.95*num_iter) is a no-op (every leaf's flag was
        flipped after its forward, :615-618, so nothing receives a gradient); the rest optimise
        body_rotation_rec + scale with loss_dct*1e-4 + loss_rec*0.5 + loss_contact*0.1 (:620).
        Sharded: every rank fits its own windows and ends up with all windows' coefficients (_dct_merge_windows)."""
        import torch
        d = self._dct_setup(fit)
        self._dct_first_phase(fit, d)
        if fit.multi and fit.ii0 <= d.P:                       # (a checkpoint from after the phase holds merged coefficients)
            self._dct_merge_windows(d)
        self._dct_second_phase(fit, d)
        if fit.multi and self.legacy_zero_grad:                # (each rank coasted its own windows)
            self._dct_merge_windows(d)
        cd = torch.empty(d.W, 23, 3, d.C, device=self.device)
        capi.check(self.ctx.lib.fdcap_opt_get_dct(self.ctx.handle, capi.dptr(cd), capi.current_stream()), "fdcap_opt_get_dct")
        self.c_dct = cd

    def _dct_setup(self, fit):
        """The refusals, the basis and c_dct (with its Adam moments as an interrupted fit left them) registered -> W windows of C
        coefficients, the second phase's first iteration P, `own`: the windows this rank fits."""
        import torch
        lib, h, st = self.ctx.lib, self.ctx.handle, capi.current_stream()
        N, T, dev, sh = self.num_body, BATCH_FRAME_NUM, self.device, self.shard
        W = N // T
        if W < 1:
            raise capi.FdcapError(f"mode 'dct' needs at least one {T}-frame window (:41-42); clip has {N} frames")
        if fit.multi and any(sh.bounds(r)[0] % T for r in range(sh.world)):
            raise capi.FdcapError(f"mode 'dct': frame shards must start on {T}-frame window boundaries "
                                  f"(N={N}, world={sh.world})")
        if self.dct_mtx is None:
            self.dct_mtx = io.load_dct_base(getattr(self, "dct_mat_path", None), T, DCT_NUM)
        D = np.ascontiguousarray(self.dct_mtx, np.float32)
        C = D.shape[1]
        resumed = "c_dct" in fit.resumed
        if fit.ii0 and not resumed:
            raise capi.FdcapError("the checkpoint holds no c_dct: not written by a mode 'dct' fit")
        if fit.ii0 and fit.log_every and fit.ii0 % fit.log_every:
            raise ValueError(f"mode 'dct': resuming at iteration {fit.ii0} needs a log_every that divides it")
        c0 = _c_dct_start(fit.resumed["c_dct"] if resumed else self._c_dct_init, W, C).to(dev, torch.float32).contiguous()
        capi.check(lib.fdcap_opt_set_dct(h, D.ctypes.data_as(ctypes.c_void_p), D.shape[0], C, capi.dptr(c0), st),
                   "fdcap_opt_set_dct")
        if resumed:
            dm, dv = (torch.as_tensor(fit.resumed[k]).to(dev, torch.float32).contiguous() for k in ("dct_m", "dct_v"))
            capi.check(lib.fdcap_opt_set_dct_state(h, capi.dptr(dm), capi.dptr(dv), st), "fdcap_opt_set_dct_state")
        w0, w1 = ctypes.c_int32(), ctypes.c_int32()
        lib.fdcap_opt_dct_windows(h, ctypes.byref(w0), ctypes.byref(w1))
        return SimpleNamespace(W=W, C=C, P=dct_first_phase2_iter(self.dct_num_iter), own=slice(w0.value, w1.value))

    def _save_dct_checkpoint(self, fit, d, next_iter):
        """parameters + Adam moments + c_dct with ITS moments (read inside _save_checkpoint's agreed-on try)"""
        self._save_checkpoint(fit.ck_path, next_iter, extra_fn=lambda: self._dct_state(d.W, d.C))

    def _dct_first_phase(self, fit, d):
        """Iterations [ii0, P): ONE launch -- or one per stretch between two checkpoint / finite-check iterations (the launch keeps
        coefficients and moments in registers and writes them back at its end; Adam's step counter runs on through step0: same
        bits).  Leaves its objective history in self.log_dct."""
        import torch
        lib, h, st = self.ctx.lib, self.ctx.handle, capi.current_stream()
        ii0, P, log_every = fit.ii0, d.P, fit.log_every
        ntraj = 69 * (d.own.stop - d.own.start)
        hist = None
        if log_every and ntraj and P > ii0:
            hist = torch.zeros((P - ii0 + log_every - 1) // log_every, ntraj, device=self.device)
        # (a stretch's logged rows are counted from its first iteration: a cut must fall on a logging iteration -- checkpoints
        #  already require it; the finite check of this phase therefore runs every lcm(check_finite_every, log_every) iterations)
        finite_cut = math.lcm(fit.finite_every, log_every) if (fit.finite_every and log_every) else fit.finite_every
        ii = ii0
        while ii < P:
            end = P                                            # cut at the next checkpoint / finite-check iteration, if any
            for every in (fit.ck_every, finite_cut):
                if every:
                    end = min(end, (ii // every + 1) * every)
            row = capi.dptr(hist[(ii - ii0) // log_every]) if hist is not None else None
            capi.check(lib.fdcap_opt_dct_fit(h, end - ii, ii, DCT_PHASE1_WEIGHT, row, max(int(log_every), 1), st), "fdcap_opt_dct_fit")
            ii = end
            if finite_cut and (ii % finite_cut == 0 or ii == P):
                self._check_dct_finite(fit, d, ii)
            if fit.ck_every and ii % fit.ck_every == 0 and ii < self.dct_num_iter:
                self._save_dct_checkpoint(fit, d, ii)          # (sharded: every rank's own windows; merged after the phase)
        self.log_dct = []
        if hist is not None:
            part = hist.sum(dim=1, dtype=torch.float64)
            if fit.multi:
                allreduce_scalars(self.shard, torch.zeros(1, device=self.device), part)
            self.log_dct = [[ii0 + k * log_every, float(v) / (69 * d.W)] for k, v in enumerate(part.cpu().numpy())]

    def _check_dct_finite(self, fit, d, done):
        """the first phase moves only c_dct: count ITS non-finite entries (and its moments') in this rank's windows"""
        import torch
        bad = sum((~torch.isfinite(t[d.own])).sum() for t in self._dct_state(d.W, d.C).values()).to(torch.float32).reshape(1)
        if fit.multi:
            allreduce_scalars(self.shard, bad)
        if int(bad.cpu()):
            raise capi.FdcapError(f"{int(bad.cpu())} non-finite DCT coefficients / Adam moments after iteration {done - 1}")

    def _dct_merge_windows(self, d):
        """every rank ends up with all windows' coefficients"""
        import torch
        lib, h = self.ctx.lib, self.ctx.handle
        full = torch.zeros(d.W, 69 * d.C, device=self.device)
        capi.check(lib.fdcap_opt_get_dct(h, capi.dptr(full), capi.current_stream()), "fdcap_opt_get_dct")
        own = torch.zeros_like(full)
        own[d.own] = full[d.own]
        own = staged_collective(self.group, own)
        capi.check(lib.fdcap_opt_set_dct_coef(h, capi.dptr(own.contiguous()), capi.current_stream()), "fdcap_opt_set_dct_coef")

    def _dct_second_phase(self, fit, d):
        """Iterations P+1 .. of the budget (P itself moves nothing); leaves their printed rows in self.log2.
        legacy_zero_grad (torch < 2: zero_grad() zeroes gradients instead of dropping them): body / scale / camera never
        hold a gradient before the switch, so the first phase is the same; from iteration P on the frozen c_dct keeps a zero
        gradient and Adam keeps stepping it on its decaying moments."""
        lib, h = self.ctx.lib, self.ctx.handle
        num_iter, P, legacy = self.dct_num_iter, d.P, self.legacy_zero_grad
        if legacy and num_iter > P and fit.ii0 <= P:           # iteration P: nothing receives a gradient, c_dct coasts
            capi.check(lib.fdcap_opt_dct_fit(h, 1, P, 0.0, None, 1, capi.current_stream()), "fdcap_opt_dct_fit")
        wd, wr, wc = DCT_PHASE2
        self.log2 = []
        for k in range(max(fit.ii0 - P - 1, 0), max(num_iter - P - 1, 0)):     # ii = P + 1 + k; Adam step counters k + 1
            ii = P + 1 + k
            st = capi.current_stream()
            do_log = is_logging_iteration(ii, num_iter, fit.log_every)
            capi.check(lib.fdcap_opt_backward_dct(h, wd, wr, wc, 1 if do_log else 0, st), "fdcap_opt_backward_dct")
            if do_log:
                self.log2.append([ii, *dct2_losses(self._logged_sums(fit), self.num_body, d.W, self.ctx.num_contact, self.weight_loss_rec,
                                                   self.weight_loss_vposer, self.weight_contact)])
                self._print_row(ii, DCT2_TERMS, self.log2[-1][1:])
            self._step(fit, k, 2 ** 30)                        # (a phase split never reached: `scale` is stepped throughout)
            if legacy:                                         # optimizer.step() of this iteration also moves the frozen c_dct
                capi.check(lib.fdcap_opt_dct_fit(h, 1, ii, 0.0, None, 1, st), "fdcap_opt_dct_fit")
            if fit.finite_every and (ii + 1) % fit.finite_every == 0:
                self._check_finite(ii)
            if fit.ck_every and (ii + 1) % fit.ck_every == 0 and ii + 1 < num_iter:
                self._save_dct_checkpoint(fit, d, ii + 1)

    # ---- mode 'local' (:534-556) -------------------------------------------------------------
    def _local_second_loop(self, fit):
        """detect_contact + the cal_loss2 loop of mode 'local' (:534-556).  Resumed inside this loop (the fit's iterations count on
        from num_iter): the contact weights (a function of the parameters as the FIRST loop left them) come from the checkpoint."""
        import torch
        lib, h = self.ctx.lib, self.ctx.handle
        sh, log_every = self.shard, fit.log_every
        jj0 = max(fit.ii0 - self.num_iter, 0)
        if jj0 and "contact_weight" not in fit.resumed:
            raise capi.FdcapError("the checkpoint holds no contact weights: not written inside mode 'local''s second loop")
        if jj0:
            weight = torch.as_tensor(fit.resumed["contact_weight"]).to(self.device, torch.float32).contiguous()
        else:
            weight = torch.empty(sh.n_local, device=self.device)
            capi.check(lib.fdcap_opt_detect_contact(h, self.n_left, capi.dptr(weight), capi.current_stream()),
                       "fdcap_opt_detect_contact")
            if fit.multi:                                      # every rank needs the weight of its right neighbour's first frame
                parts = [torch.empty(sh.bounds(r)[1] - sh.bounds(r)[0], device=self.device) for r in range(sh.world)]
                weight = torch.cat(staged_collective(self.group, weight, parts)).contiguous()
        self.contact_weight = weight
        self.log2 = []
        n2 = int(LOCAL_SECOND_LOOP * self.num_iter)
        for jj in range(jj0, n2):
            st = capi.current_stream()
            capi.check(lib.fdcap_opt_backward_local2(h, capi.dptr(weight), self.n_left, st), "fdcap_opt_backward_local2")
            if log_every and (jj % log_every == 0):
                self.log2.append([jj, *local2_losses(self._logged_sums(fit), self.num_body, self.ctx.num_verts, self.weight_loss_rec)])
                self._print_row(jj, LOCAL2_TERMS, self.log2[-1][1:])
            capi.check(lib.fdcap_opt_step_x(h, self.num_iter + jj + 1, st), "fdcap_opt_step_x")
            if fit.multi:
                self._halos()
            done = self.num_iter + jj + 1                    # iterations of the whole fit made so far
            if fit.finite_every and done % fit.finite_every == 0:
                self._check_finite(done - 1)
            if fit.ck_every and done % fit.ck_every == 0 and jj + 1 < n2:
                self._save_checkpoint(fit.ck_path, done, contact_weight=weight)

    # ---- :637-653 -------------------------------------------------------------------------
    def save_result(self, body_rec, scale, camera_ext, fit_path):
        import torch
        br = body_rec.detach().cpu().numpy() if torch.is_tensor(body_rec) else np.asarray(body_rec)
        ce = camera_ext.detach().cpu().numpy() if torch.is_tensor(camera_ext) else np.asarray(camera_ext)
        return io.save_result(br, scale, ce, fit_path)

    def close(self):
        if getattr(self, "ctx", None) is not None:
            self.ctx.close()
            self.ctx = None


class ClipBatchFitter(_Fitter):
    """Several clips of one scene as ONE optimisation (fdcap_opt_create_clips): K clips share the scene, the contact ids, the
    body model, VPoser and the configuration; each keeps its own rows, `scale`, Adam moments, outlier set, loss means (over its
    own frames) and logged sums, and the temporal stencils are cut at clip boundaries.  The clips may have different lengths
    (fdcap_opt_create_clips_var: clip k in rows clip_starts[k] .. + clip_lens[k] of the batch).  A clip's result equals its
    stand-alone FittingOP fit bit for bit whenever both select the same kernel forms (include/fdcap.h).

    The fitter owns ONE context for its whole life -- the persistent worker: the body model and the contact ids are registered
    once, a scene once per run of batches of that scene (`fit(..., scene_key=...)` skips the registration when the key is the
    previous batch's).

    Modes 'global', 'local' and 'dct' (`fit(..., mode=...)`).  Mode 'local' runs its first loop as fdcap_opt_run under the 'local' config
    and its second loop -- detect_contact and the cal_loss2 iterations (:534-556) -- as ONE fdcap_opt_run_local2 call; it leaves
    each clip's second-loop log in self.logs2 and detect_contact's weights in self.contact_weights.  Mode 'dct' (:595-630) is
    fdcap_opt_set_dct_clips + ONE fdcap_opt_run_dct call of `dct_num_iter` iterations: every clip has its own 60-frame windows over
    its own frames (so at least 60 frames), and the first phase is one launch over all clips' trajectories; it leaves each clip's
    c_dct [W_k,23,3,C] in self.c_dct, its first-phase log in self.logs_dct and its second-phase log in self.logs2."""
    _n_left_from_files = False      # (the left part is half of the contact ids unless `n_left` says otherwise)

    def __init__(self, fittingconfig, lossconfig, body_model=None, vposer=None, contact_ids=None, legacy_zero_grad=False, n_left=None,
                 dct_num_iter=DCT_NUM_ITER):
        if float((lossconfig or {}).get("weight_reproj", 0) or 0) != 0.0:        # (before anything touches the device)
            raise ValueError("weight_reproj: the reprojection term is implemented for one clip (FittingOP, mode 'global'), not for a batch of clips")
        super().__init__(fittingconfig, lossconfig, body_model, vposer, contact_ids, n_left, legacy_zero_grad, dct_num_iter)
        self.ctx.set_contact_ids(self.vid)
        self.scene_key = None
        self._slot_keys = [None] * capi.MAX_SCENES          # the keys of the scenes in slots 1.. (slot 0's is scene_key)
        self._has_opt = False
        self.logs, self.logs2, self.logs_dct, self.contact_weights, self.idx1, self.c_dct = [], [], [], [], [], []      # (a batch's results)
        self._dct_in = (None, None)

    def _destroy_opt(self):
        if self._has_opt:
            self.ctx.lib.fdcap_opt_destroy(self.ctx.handle)
            self._has_opt = False

    def set_scene(self, scene_verts, key=None):
        """Register the scene of the following batches (after the optimiser of the previous batch is gone: the library refuses a
        new scene while one exists).  `key` (e.g. the scene's path): nothing is done when it is the key of the registered scene."""
        if key is not None and key == self.scene_key:
            return
        self._destroy_opt()
        self.ctx.set_scene(np.zeros((0, 3), np.float32) if scene_verts is None else scene_verts)
        self.scene_key = key

    @staticmethod
    def _check_mode(clips, mode):
        """the refusals that need no device"""
        if mode not in ("global", "local", "dct"):
            raise ValueError("a batch of clips fits in mode 'global', 'local' or 'dct'")
        if mode == "dct" and any(int(np.shape(body)[0]) < BATCH_FRAME_NUM for body, _ in clips):
            raise ValueError(f"mode 'dct' needs at least one {BATCH_FRAME_NUM}-frame window in every clip (:41-42); "
                             "shorter clips fit in mode 'global' or 'local'")

    def fit(self, clips, scene_verts=None, scene_key=None, log_every=0, mode="global", c_dct_init=None, dct_mtx=None, scenes=None,
            clip_scene=None):
        """clips: sequence of K (body_data [N_k,75], camera_ext [N_k,4,4]) pairs (numpy or device tensors); every clip has its own N_k.
        scene_verts / scene_key: the batch's scene (see set_scene; both None: the registered scene).
        scenes / clip_scene: clips of DIFFERENT scenes in one batch (mode 'global') -- scenes: a list whose entries are the points
        [ns,3] or (key, points) pairs (points None: a slot holds the key already), clip_scene: for every clip its entry of scenes;
        at most capi.MAX_SCENES scenes in use.  The scenes go into the context's slots (a key a slot holds is not registered
        again), the clips enter the batch ordered so that every scene is one run (fdcap_opt_create_clips_scenes), and the results,
        self.logs and self.idx1 come back in the caller's order.  One scene in use: the one-scene batch.
        mode: 'global', 'local' (the reference's default, :491) or 'dct' -- then c_dct_init: K arrays [W_k,23,3,C], W_k = N_k // 60
        (None: torch.randn, clip after clip, :186), dct_mtx [60,C] (None: load_dct_base, as FittingOP).
        Returns a list of K (body_rec [N_k,75] device tensor, scale numpy scalar, camera_ext [N_k,4,4] device tensor) -- what
        FittingOP.fitting returns for each clip -- and leaves each clip's FitLog in self.logs, its outlier rows in self.idx1; mode
        'local' also each clip's second-loop rows [jj, l_rec, l_loc, l_sm, l_cs, total] (FittingOP.log2, the means over the clip's
        own frames) in self.logs2 and detect_contact's per-frame weights in self.contact_weights; mode 'dct' each clip's c_dct in
        self.c_dct, its rows [ii, loss_dct] of the first phase in self.logs_dct and [ii, l_rec, l_vposer, loss_smoothing, loss_contact,
        loss_dct, total] of the second in self.logs2 (FittingOP.log_dct / log2, over the clip's own frames and windows)."""
        self._check_mode(clips, mode)
        if scenes is not None or clip_scene is not None:
            return self._fit_scenes(clips, scenes, clip_scene, log_every, mode, c_dct_init, dct_mtx)
        if scene_verts is not None or scene_key is not None:
            self.set_scene(scene_verts, scene_key)
        self.prepare(clips, mode, c_dct_init, dct_mtx)
        return self.run(log_every)

    @staticmethod
    def plan_scene_runs(clip_scene, n_scenes, max_scenes=capi.MAX_SCENES):
        """clip_scene[k]: the entry of `scenes` clip k is fitted against.  -> (the scenes in use in order of first use, the order
        in which the clips enter the batch: every scene ONE run of adjacent clips, runs in order of first use, clips in input order
        within a run).  Needs no device."""
        cs = [int(s) for s in clip_scene]
        if any(s < 0 or s >= n_scenes for s in cs):
            raise ValueError(f"clip_scene names a scene outside [0, {n_scenes})")
        used = list(dict.fromkeys(cs))
        if len(used) > max_scenes:
            raise ValueError(f"a batch holds clips of at most {max_scenes} scenes (got {len(used)}): split it (cli.plan_batches_scenes)")
        rank = {s: r for r, s in enumerate(used)}
        return used, sorted(range(len(cs)), key=lambda k: rank[cs[k]])

    def _fit_scenes(self, clips, scenes, clip_scene, log_every, mode, c_dct_init, dct_mtx):
        """fit() for clips of several scenes: registers the scenes in slots (a scene whose key a slot already holds is reused),
        orders the clips so that every scene is one run, fits the batch and hands everything back in the caller's order."""
        if scenes is None or clip_scene is None or len(clip_scene) != len(clips):
            raise ValueError("scenes=[...] and clip_scene=[one entry of scenes per clip] go together")
        # an entry of `scenes`: the points [ns,3], or (key, points) -- points may be None when a slot already holds the key
        ent = [(s[0], s[1]) if isinstance(s, tuple) else (None, s) for s in scenes]
        used, order = self.plan_scene_runs(clip_scene, len(ent))
        if len(used) > 1 and mode != "global":
            raise ValueError(f"clips of several scenes fit in mode 'global' only (got mode '{mode}'): modes 'local' and 'dct' take "
                             "batches of one scene")
        if len(used) == 1:                                   # one scene: the batch it always was
            key, pts = ent[used[0]]
            if key is not None and key == self.scene_key:
                pts = None
            elif key is not None and key in self._slot_keys[1:]:      # held by another slot: the one-scene batch on that slot
                self.prepare(clips, mode, c_dct_init, dct_mtx, clip_slots=[self._slot_keys.index(key, 1)] * len(clips))
                return self.run(log_every)
            elif pts is None:
                raise ValueError(f"scene {key!r} is not registered and no points were given")
            return self.fit(clips, pts, key, log_every, mode, c_dct_init, dct_mtx)
        # slots: first the scenes whose key a slot holds, then the others into the slots this batch leaves free
        keys = [self.scene_key] + self._slot_keys[1:]
        slot_of = {}
        for s in used:
            key = ent[s][0]
            if key is not None and key in keys and keys.index(key) not in slot_of.values():
                slot_of[s] = keys.index(key)
        free = [i for i in range(capi.MAX_SCENES) if i not in slot_of.values()]
        free.sort(key=lambda i: (keys[i] is not None or (i == 0 and self.ctx.num_scene > 0), i))     # empty slots first
        for s in used:
            if s in slot_of:
                continue
            key, pts = ent[s]
            if pts is None:
                raise ValueError(f"scene {key!r} is not registered and no points were given")
            i = free.pop(0)
            if i == 0:
                self.set_scene(pts, key)
            else:
                self._destroy_opt()                          # (the library refuses a new scene while an optimiser exists)
                self.ctx.set_scene_slot(i, pts)
                self._slot_keys[i] = key
            slot_of[s] = i
        batch = [clips[k] for k in order]
        self.prepare(batch, mode, c_dct_init, dct_mtx, clip_slots=[slot_of[int(clip_scene[k])] for k in order])
        res = self.run(log_every)
        back = [0] * len(order)
        for pos, k in enumerate(order):
            back[k] = pos
        self.logs = [self.logs[p] for p in back]
        self.idx1 = [self.idx1[p] for p in back]
        return [res[p] for p in back]

    def prepare(self, clips, mode="global", c_dct_init=None, dct_mtx=None, clip_slots=None):
        """init() of a batch (:450-489 per clip): creates the batch's optimiser on the registered scene and stages its inputs.
        mode 'local': the config of its first loop (:511, :523), as FittingOP.init builds it; mode 'dct': mode 'global''s, as there.
        clip_slots (optional): the registered scene slot of every clip (fdcap_opt_create_clips_scenes)."""
        import torch
        self._check_mode(clips, mode)
        if clip_slots is not None and len(set(clip_slots)) > 1 and mode != "global":
            raise ValueError("clips of several scenes fit in mode 'global' only")
        self._mode = mode
        self._dct_in = (c_dct_init, dct_mtx)
        K = len(clips)
        if K < 1:
            raise ValueError("a batch needs at least one clip")
        dev = self.device
        bodies, cams = [], []
        for body, cam in clips:
            b = body if torch.is_tensor(body) else torch.from_numpy(np.ascontiguousarray(body, dtype=np.float32))
            bodies.append(b.to(dev, torch.float32))
            c = cam.detach().cpu().numpy() if torch.is_tensor(cam) else np.asarray(cam)
            cams.append(np.asarray(c, np.float32).reshape(-1, 16))
        lens = [int(b.shape[0]) for b in bodies]
        if min(lens) < 1 or any(c.shape[0] != n for c, n in zip(cams, lens)):
            raise capi.FdcapError("every clip of a batch has at least one frame, and one camera pose per frame (:455)")
        starts = [0]
        for n in lens:
            starts.append(starts[-1] + n)
        total = starts[-1]
        equal = all(n == lens[0] for n in lens)
        lib, h = self.ctx.lib, self.ctx.handle
        st = capi.current_stream()
        body = torch.cat(bodies).contiguous()
        x78 = torch.empty(total, capi.XDIM, device=dev)
        capi.check(lib.fdcap_params_75_to_78(capi.dptr(body), total, capi.dptr(x78), st), "fdcap_params_75_to_78")
        # init() per clip (:459-487): outliers, their replacement rows and the mask of the data term, each clip on its own rows
        x78_h = x78.cpu().numpy()
        ins = [clip_inputs(x78_h[starts[k]:starts[k + 1]]) for k in range(K)]
        self.idx1 = [i[0] for i in ins]
        # one length: the clip's frames, as fdcap_opt_create_clips takes it; different lengths: the batch's rows
        n_cfg = lens[0] if equal else total
        oc = self._opt_config(n_cfg, n_cfg, 0)
        state = self._new_state(total + 4, K, (K, capi.NUM_LOSSES))
        if clip_slots is not None:
            if len(clip_slots) != K:
                raise ValueError("clip_slots holds one scene slot per clip")
            oc = self._opt_config(total, total, 0)           # (the batch's rows, as fdcap_opt_create_clips_var takes them)
            capi.check(lib.fdcap_opt_create_clips_scenes(h, ctypes.byref(oc), K, (ctypes.c_int32 * K)(*lens), (ctypes.c_int32 * K)(*clip_slots),
                                                         *state), "fdcap_opt_create_clips_scenes")
        elif equal:
            capi.check(lib.fdcap_opt_create_clips(h, ctypes.byref(oc), K, *state), "fdcap_opt_create_clips")
        else:
            capi.check(lib.fdcap_opt_create_clips_var(h, ctypes.byref(oc), K, (ctypes.c_int32 * K)(*lens), *state), "fdcap_opt_create_clips_var")
        self._has_opt = True
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_init = t(np.concatenate([i[1] for i in ins]))
        d_mask = t(np.concatenate([i[2] for i in ins]))
        d_cam = t(np.concatenate(cams))
        capi.check(lib.fdcap_opt_set_inputs(h, capi.dptr(x78), capi.dptr(d_init), capi.dptr(d_mask), capi.dptr(d_cam), st),
                   "fdcap_opt_set_inputs")
        self.num_clips, self.clip_lens, self.clip_starts = K, lens, starts
        self.num_body = lens[0] if equal else None           # (the one length of a batch of equal clips)

    def run(self, log_every=0):
        """The loop of the prepared batch (:558-593) and its results (see fit)."""
        import torch
        if self._mode == "dct":
            return self._run_dct(log_every)
        K, lens = self.num_clips, self.clip_lens
        lib, h = self.ctx.lib, self.ctx.handle
        # the loop in the library, as FittingOP.fitting runs a plain fit: one fdcap_opt_run for all iterations
        num_iter = int(self.num_iter)
        P = first_phase2_iter(num_iter)
        logged = [ii for ii in range(num_iter) if is_logging_iteration(ii, num_iter, log_every)]
        hist = torch.zeros(max(len(logged), 1), K, capi.NUM_LOSSES, device=self.device, dtype=torch.float64)
        try:
            self._opt_run(0, num_iter, P, log_every, hist if logged else None)
        finally:
            if logged:
                capi.check(lib.fdcap_opt_set_loss_output(h, capi.dptr(self._losses)), "fdcap_opt_set_loss_output")
        local = self._mode == "local"
        self.logs2, self.contact_weights = [], []
        if local:
            self._run_local2(log_every)
        results = self._results(self.clip_starts[-1], K)
        rows = hist.cpu().numpy()
        self.logs = []
        for k in range(K):
            log = FitLog()
            for j, ii in enumerate(logged):
                # (the printed means of a clip run over its own frames)
                log.append(ii, logged_losses(rows[j, k], lens[k], self.ctx.num_contact, self.weight_loss_rec, self.weight_loss_vposer,
                                             self.weight_contact, ii >= P, local))
            self.logs.append(log)
        return self._per_clip(*results)

    def _per_clip(self, body_rec, scale, cam):
        """the batch's results -> each clip's triple, as FittingOP.fitting returns it"""
        lens, starts = self.clip_lens, self.clip_starts
        sc = scale.cpu().numpy()
        return [(body_rec[starts[k]:starts[k + 1]], sc[k], cam[starts[k]:starts[k + 1]].view(lens[k], 4, 4)) for k in range(self.num_clips)]

    def _run_local2(self, log_every):
        """detect_contact + the cal_loss2 loop (:534-556) of every clip of the prepared batch in ONE call; its history is read back once"""
        import torch
        K, lens, starts, dev = self.num_clips, self.clip_lens, self.clip_starts, self.device
        lib, h = self.ctx.lib, self.ctx.handle
        num_iter = int(self.num_iter)
        n2 = int(LOCAL_SECOND_LOOP * num_iter)
        logged2 = [jj for jj in range(n2) if log_every and jj % log_every == 0]
        hist2 = torch.zeros(max(len(logged2), 1), K, capi.NUM_LOSSES, device=dev, dtype=torch.float64)
        weight = torch.empty(starts[-1], device=dev)
        n_done = ctypes.c_int32(0)
        try:
            capi.check(lib.fdcap_opt_run_local2(h, self.n_left, 0, n2, num_iter, int(log_every or 0), capi.dptr(weight),
                                                capi.dptr(hist2) if logged2 else None, len(logged2), 0, ctypes.byref(n_done),
                                                capi.current_stream()), "fdcap_opt_run_local2")
        finally:
            capi.check(lib.fdcap_opt_set_loss_output(h, capi.dptr(self._losses)), "fdcap_opt_set_loss_output")
        assert n_done.value == len(logged2)
        rows2 = hist2.cpu().numpy()
        self.contact_weights = [weight[starts[k]:starts[k + 1]] for k in range(K)]
        self.logs2 = [[[jj, *local2_losses(rows2[j, k], lens[k], self.ctx.num_verts, self.weight_loss_rec)] for j, jj in enumerate(logged2)]
                      for k in range(K)]

    def _run_dct(self, log_every=0):
        """mode 'dct' of the prepared batch: fdcap_opt_set_dct_clips, ONE fdcap_opt_run_dct, the read-backs."""
        import torch
        K, lens, dev = self.num_clips, self.clip_lens, self.device
        T = BATCH_FRAME_NUM
        lib, h = self.ctx.lib, self.ctx.handle
        st = capi.current_stream()
        c_init, D = self._dct_in
        if D is None:
            D = io.load_dct_base(getattr(self, "dct_mat_path", None), T, DCT_NUM)
        D = np.ascontiguousarray(D, np.float32)
        C = D.shape[1]
        Wk = [n // T for n in lens]
        ws = [0]
        for w in Wk:
            ws.append(ws[-1] + w)
        if c_init is not None and len(c_init) != K:
            raise capi.FdcapError(f"c_dct_init must hold one array per clip ({K}), got {len(c_init)}")
        c0 = [_c_dct_start(None if c_init is None else c_init[k], Wk[k], C, f"c_dct_init[{k}]") for k in range(K)]
        c0 = torch.cat(c0).to(dev, torch.float32).contiguous()
        capi.check(lib.fdcap_opt_set_dct_clips(h, D.ctypes.data_as(ctypes.c_void_p), D.shape[0], C, capi.dptr(c0), st), "fdcap_opt_set_dct_clips")
        num_iter = self.dct_num_iter
        P = dct_first_phase2_iter(num_iter)
        log_every = int(log_every or 0)
        logged1 = list(range(0, P, log_every)) if log_every else []
        logged2 = [ii for ii in range(P + 1, num_iter) if is_logging_iteration(ii, num_iter, log_every)]
        hist1 = torch.zeros(max(len(logged1), 1), 69 * ws[-1], device=dev)
        hist2 = torch.zeros(max(len(logged2), 1), K, capi.NUM_LOSSES, device=dev, dtype=torch.float64)
        wd, wr, wc = DCT_PHASE2
        n_done = ctypes.c_int32(0)
        try:
            capi.check(lib.fdcap_opt_run_dct(h, 0, num_iter, num_iter, DCT_PHASE1_WEIGHT, wd, wr, wc, log_every,
                                             capi.dptr(hist1) if logged1 else None, capi.dptr(hist2) if logged2 else None, len(logged2), 0,
                                             ctypes.byref(n_done), st), "fdcap_opt_run_dct")
        finally:
            capi.check(lib.fdcap_opt_set_loss_output(h, capi.dptr(self._losses)), "fdcap_opt_set_loss_output")
        assert n_done.value == len(logged2)
        results = self._results(self.clip_starts[-1], K)
        cd = torch.empty(ws[-1], 23, 3, C, device=dev)
        capi.check(lib.fdcap_opt_get_dct(h, capi.dptr(cd), st), "fdcap_opt_get_dct")
        self.c_dct = [cd[ws[k]:ws[k + 1]] for k in range(K)]
        self.logs, self.contact_weights = [], []
        self.logs_dct, self.logs2 = [], []
        rows2 = hist2.cpu().numpy()
        for k in range(K):
            part = hist1[:, 69 * ws[k]:69 * ws[k + 1]].sum(dim=1, dtype=torch.float64).cpu().numpy()
            self.logs_dct.append([[ii, float(part[j]) / (69 * Wk[k])] for j, ii in enumerate(logged1)])
            self.logs2.append([[ii, *dct2_losses(rows2[j, k], lens[k], Wk[k], self.ctx.num_contact, self.weight_loss_rec,
                                                 self.weight_loss_vposer, self.weight_contact)] for j, ii in enumerate(logged2)])
        return self._per_clip(*results)

    def close(self):
        if getattr(self, "ctx", None) is not None:
            self._destroy_opt()
            self.ctx.close()
            self.ctx = None
