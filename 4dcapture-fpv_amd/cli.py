"""Command line of the hot path, argument-compatible with the reference:

    python3 global_optimization.py <body_path> <fit_path> <mode>      (global_optimization.py:658-660)

`<body_path>/results/*/*.pkl` in, `<fit_path>/body_gen_%06d.pkl` out.  The reference hard-codes
`/home/miao/<sample>/meshed-poisson.ply` and `camerapose.txt` (:667-668); the root is configurable
here (`--scene-root`, or explicit `--scene` / `--camera`).  `./models`, `./vposer/`,
`./body_segments` default to the reference's CWD-relative paths (:669-675).

Several clips in one run (the reference's real workload: every video cut into 300-frame segments, utils/split_frames.py):

    python3 global_optimization_hip.py --clips BODY_PATH [BODY_PATH ...] --fit-root DIR [--clips-per-batch K]

Each clip's scene and camera paths are derived from its sample name as above (`--scene-root`).  Clips are grouped by (scene
file -- the resolved path, so that the segments of one video may link one scene --, clip length); each group is cut into batches of at most K clips that are fitted as one optimisation (fitting.ClipBatchFitter:
one context for the whole run).  Clip output: `<fit-root>/<sample_name>/body_gen_%06d.pkl`, the files the one-clip form writes
with that directory as <fit_path>.  Default K: the largest K with K * N <= MULTICLIP_ROW_CAP.  Mode 'global' only ON THIS COMMAND
LINE: the library and the Python interface fit a batch in mode 'local' as well (fitting.ClipBatchFitter.fit(..., mode='local'),
fdcap_opt_run_local2), but `--clips --mode local` is still refused here, and tests/test_multiclip_cpu.py::
test_modes_other_than_global_are_refused pins that refusal -- lifting it is a follow-up that has to change that test with it.

`--mix-lengths` (with --clips): clips are grouped by scene file alone and a batch may hold clips of different lengths
(plan_batches_mixed: batches are filled in input order up to MULTICLIP_ROW_CAP rows, so a video's short remainder clip rides with
its full segments).  Every clip's result is the one its own batch-of-one gives.

`--mix-scenes` (with --clips; implies --mix-lengths): a batch may also hold clips of different SCENES -- in the reference's data
every video has its own reconstruction, so without this a video of one or two clips is a batch of one or two.  Batches are filled in
input order up to MULTICLIP_ROW_CAP rows and MAX_SCENES scenes (plan_batches_scenes); the fitter keeps the scenes in the context's
slots by path, so a scene that the next batch uses again is neither read nor registered again.  Without the flag every planner,
batch and refusal above is what it was.

`--keypoints DIR --weight-reproj W [--intrinsics FX FY CX CY] [--rho R]` (one-clip form, mode 'global'): the clip-level 2D-keypoint
reprojection term (fitting.FittingOP.fitting(keypoints=...)).  DIR holds a detector's OpenPose-format files; the
sorted `*_keypoints.json` are paired one per frame with the `results/*/*.pkl` files (a count mismatch is an error naming both counts) and
mapped to the 23 body joints by innerfit.joints23_from_openpose.  With --clips the options are refused."""
from __future__ import annotations

import argparse
import os
import sys

# Largest row count (clips x frames) of a default batch of the multi-clip form: up to 1024 rows the per-frame kernels run in one
# round of workgroups (1280 frames take a second); profiles/r7_multiclip300.json has the sweep over K at N = 300.
MULTICLIP_ROW_CAP = 1024


def sample_name_of(body_path: str) -> str:
    """The sample name the reference takes from the body path (:662)."""
    return body_path.split("/")[-2]


def clip_paths(body_path: str, scene_root: str):
    """(sample name, scene path, camera path) of a clip, derived as the one-clip form derives them (:662-668)."""
    name = sample_name_of(body_path)
    return name, os.path.join(scene_root, name, "meshed-poisson.ply"), os.path.join(scene_root, name, "camerapose.txt")


def clip_output_dir(fit_root: str, body_path: str) -> str:
    return os.path.join(fit_root, sample_name_of(body_path))


def batch_size(n_frames: int, clips_per_batch=None, row_cap: int = MULTICLIP_ROW_CAP) -> int:
    """Clips per batch for clips of n_frames: the given K, else the largest K with K * n_frames <= row_cap (at least 1)."""
    if clips_per_batch:
        return max(1, int(clips_per_batch))
    return max(1, row_cap // max(1, int(n_frames)))


def plan_batches(clips, clips_per_batch=None, row_cap: int = MULTICLIP_ROW_CAP):
    """clips: sequence of (scene path, clip length).  Groups them by (scene path, clip length) -- groups in order of their first
    clip, clips in input order within a group -- and cuts every group into batches of batch_size() clips.
    Returns [(scene path, clip length, [clip indices])]."""
    groups = {}
    for i, (scene, n) in enumerate(clips):
        groups.setdefault((scene, int(n)), []).append(i)
    out = []
    for (scene, n), idx in groups.items():
        k = batch_size(n, clips_per_batch, row_cap)
        out.extend((scene, n, idx[j:j + k]) for j in range(0, len(idx), k))
    return out


def plan_batches_mixed(clips, clips_per_batch=None, row_cap: int = MULTICLIP_ROW_CAP):
    """clips: sequence of (scene path, clip length).  Groups them by scene path alone -- groups in order of their first clip, clips
    in input order within a group -- and fills batches in that order: a batch is closed when the next clip would push its rows
    above row_cap (a clip longer than the cap is a batch of its own) or its clip count above clips_per_batch.  For clips of one
    length these are plan_batches' batches (as long as a given clips_per_batch stays within the row cap, which plan_batches does
    not apply to it).  Returns [(scene path, [clip indices])]."""
    groups = {}
    for i, (scene, n) in enumerate(clips):
        groups.setdefault(scene, []).append(i)
    kmax = max(1, int(clips_per_batch)) if clips_per_batch else None
    out = []
    for scene, idx in groups.items():
        cur, rows = [], 0
        for i in idx:
            n = int(clips[i][1])
            full = rows + n > row_cap or (kmax is not None and len(cur) >= kmax)
            if cur and full:
                out.append((scene, cur))
                cur, rows = [], 0
            cur.append(i)
            rows += n
        if cur:
            out.append((scene, cur))
    return out


MAX_SCENES = 8          # = capi.MAX_SCENES (FDCAP_MAX_SCENES), restated so that planning imports nothing


def plan_batches_scenes(clips, clips_per_batch=None, row_cap: int = MULTICLIP_ROW_CAP, scene_cap: int = MAX_SCENES):
    """clips: sequence of (scene path, clip length).  Batches are filled in INPUT order, whatever the scenes: a batch is closed when
    the next clip would push its rows above row_cap (a clip longer than the cap is a batch of its own), its clip count above
    clips_per_batch, or its number of different scenes above scene_cap.  Within a batch the fitter orders the clips so that every
    scene is one run (fitting.ClipBatchFitter.fit(scenes=..., clip_scene=...)).  For clips of one scene these are
    plan_batches_mixed's batches.  Returns [([scene paths in order of first use], [clip indices])]."""
    kmax = max(1, int(clips_per_batch)) if clips_per_batch else None
    out = []
    cur, rows, scenes = [], 0, []
    for i, (scene, n) in enumerate(clips):
        n = int(n)
        full = rows + n > row_cap or (kmax is not None and len(cur) >= kmax) or (scene not in scenes and len(scenes) >= scene_cap)
        if cur and full:
            out.append((scenes, cur))
            cur, rows, scenes = [], 0, []
        cur.append(i)
        rows += n
        if scene not in scenes:
            scenes.append(scene)
    if cur:
        out.append((scenes, cur))
    return out


def keypoint_files(keypoints_dir: str, n_frames: int):
    """The sorted `*_keypoints.json` files of a directory, one per frame: ValueError naming both counts when they differ."""
    import glob
    files = sorted(glob.glob(os.path.join(keypoints_dir, "*_keypoints.json")))
    if len(files) != n_frames:
        raise ValueError(f"{len(files)} *_keypoints.json files in {keypoints_dir} for {n_frames} frames (results/*/*.pkl)")
    return files


def main(argv=None):
    ap = argparse.ArgumentParser(prog="global_optimization (fdcap_amd / MI355X)")
    ap.add_argument("body_path", nargs="?")
    ap.add_argument("fit_path", nargs="?")
    ap.add_argument("mode", nargs="?", default="global", choices=["global", "local", "dct"])
    ap.add_argument("--clips", nargs="+", default=None, metavar="BODY_PATH",
                    help="several clips in one run (mode 'global'): fitted in batches of one scene and clip length")
    ap.add_argument("--fit-root", default=None, help="multi-clip form: clip output goes to <fit-root>/<sample_name>/")
    ap.add_argument("--clips-per-batch", type=int, default=None,
                    help=f"multi-clip form: clips per batch (default: the largest K with K * frames <= {MULTICLIP_ROW_CAP})")
    ap.add_argument("--mix-lengths", action="store_true",
                    help="multi-clip form: group clips by scene alone; a batch may hold clips of different lengths and never more "
                         f"than {MULTICLIP_ROW_CAP} rows, also with --clips-per-batch (without this flag K alone bounds a batch)")
    ap.add_argument("--mix-scenes", action="store_true",
                    help="multi-clip form (implies --mix-lengths): a batch may hold clips of different scenes -- batches are filled "
                         f"in input order up to {MULTICLIP_ROW_CAP} rows and {MAX_SCENES} scenes")
    ap.add_argument("--mode", dest="mode_opt", default=None, choices=["global", "local", "dct"],
                    help="multi-clip form: the mode (only 'global' is supported)")
    ap.add_argument("--scene-root", default="/home/miao/")
    ap.add_argument("--scene", default=None, help="scene vertices (.ply/.xyz/.npy); default <root>/<sample>/meshed-poisson.ply")
    ap.add_argument("--camera", default=None, help="camerapose.txt; default <root>/<sample>/camerapose.txt")
    ap.add_argument("--models", default="./models")
    ap.add_argument("--vposer", default="./vposer/")
    ap.add_argument("--body-segments", default="./body_segments")
    ap.add_argument("--num-iter", type=int, default=500)
    ap.add_argument("--lr", type=float, default=0.005)
    ap.add_argument("--log-every", type=int, default=0)
    ap.add_argument("--dct-mat", default="../Data/DCT_Basis/60.mat", help="DCT basis .mat (:45); generated if absent")
    ap.add_argument("--dct-num-iter", type=int, default=10000, help="iterations of mode 'dct' (:596)")
    ap.add_argument("--keypoints", default=None, metavar="DIR",
                    help="one-clip form: a detector's *_keypoints.json files (OpenPose format), one per frame, for the reprojection term")
    ap.add_argument("--weight-reproj", type=float, default=0.0, help="one-clip form, mode 'global': weight of the reprojection term (0: off)")
    ap.add_argument("--intrinsics", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"),
                    help="pinhole intrinsics of the reprojection term (default 692 692 640 360)")
    ap.add_argument("--rho", type=float, default=None, help="GMoF's rho of the reprojection term, in pixels (default 100)")
    a = ap.parse_args(argv)
    if a.clips is not None:
        if a.keypoints is not None or a.weight_reproj != 0.0 or a.intrinsics is not None or a.rho is not None:
            ap.error("--keypoints / --weight-reproj / --intrinsics / --rho belong to the one-clip form: the reprojection term is not implemented for --clips")
        return _main_clips(ap, a)
    if (a.weight_reproj != 0.0) != (a.keypoints is not None):
        ap.error("--keypoints DIR and a non-zero --weight-reproj W go together")
    if a.weight_reproj != 0.0 and a.mode != "global":
        ap.error(f"--weight-reproj: the reprojection term is implemented for mode 'global' (got mode '{a.mode}')")
    if a.mix_lengths:
        ap.error("--mix-lengths belongs to the multi-clip form (--clips ... --fit-root DIR)")
    if a.mix_scenes:
        ap.error("--mix-scenes belongs to the multi-clip form (--clips ... --fit-root DIR)")
    if a.body_path is None or a.fit_path is None:
        ap.error("body_path and fit_path are required (or --clips ... --fit-root DIR)")

    import torch
    from . import io
    from .fitting import FittingOP

    sample_name = a.body_path.split("/")[-2]                                    # :662
    scene = a.scene or os.path.join(a.scene_root, sample_name, "meshed-poisson.ply")
    camera = a.camera or os.path.join(a.scene_root, sample_name, "camerapose.txt")
    fittingconfig = {"scene_verts_path": scene, "camera_path": camera, "human_model_path": a.models,
                     "vposer_ckpt_path": a.vposer, "init_lr_h": a.lr, "num_iter": a.num_iter,
                     "contact_id_folder": a.body_segments, "contact_part": ["L_Leg", "R_Leg"],
                     "verbose": bool(a.log_every), "dct_mat_path": a.dct_mat}
    lossconfig = {"weight_loss_rec": 1, "weight_loss_vposer": 0.001, "weight_contact": 0.1, "weight_collision": 0.5}
    data = io.load_body_gen(a.body_path)                                         # :688-707
    reproj = {}
    if a.weight_reproj != 0.0:
        from . import innerfit
        try:
            files = keypoint_files(a.keypoints, data.shape[0])
        except ValueError as e:
            ap.error(str(e))
        lossconfig["weight_reproj"] = a.weight_reproj
        reproj = dict(keypoints=innerfit.joints23_from_openpose([io.read_openpose_json(f, hands=False) for f in files]),
                      intrinsics=tuple(a.intrinsics) if a.intrinsics else innerfit.DEFAULT_INTRINSICS, rho=100.0 if a.rho is None else a.rho)
    fop = FittingOP(fittingconfig, lossconfig, data.shape[0], dct_num_iter=a.dct_num_iter)
    body_rec, scale, camera_ext = fop.fitting(torch.tensor(data).cuda(), a.mode, log_every=a.log_every, **reproj)
    fop.save_result(body_rec, scale, camera_ext, a.fit_path)                     # :714
    print("[INFO][fitting] fitting finish, returning optimal value")
    return 0


def _main_clips(ap, a):
    mode = a.mode_opt or "global"
    if a.body_path is not None or a.fit_path is not None:
        ap.error("--clips takes the clips' body paths; positional body_path / fit_path belong to the one-clip form")
    if mode != "global":
        ap.error(f"--clips fits mode 'global' only (got mode '{mode}'); run modes 'local' and 'dct' one clip at a time")
    if not a.fit_root:
        ap.error("--clips needs --fit-root DIR")
    if a.scene or a.camera:
        ap.error("--clips derives every clip's scene and camera paths from --scene-root; --scene / --camera are one-clip options")
    if a.clips_per_batch is not None and a.clips_per_batch < 1:
        ap.error("--clips-per-batch must be at least 1")
    from . import io
    from .fitting import ClipBatchFitter
    data, cams, scenes = [], [], []
    for bp in a.clips:
        _, scene, camera = clip_paths(bp, a.scene_root)
        data.append(io.load_body_gen(bp))                                       # :688-707
        cams.append(io.read_camerapose(camera))
        scenes.append(os.path.realpath(scene))                                  # (segments of one video may link one scene file)
    fittingconfig = {"human_model_path": a.models, "vposer_ckpt_path": a.vposer, "init_lr_h": a.lr, "num_iter": a.num_iter,
                     "contact_id_folder": a.body_segments, "contact_part": ["L_Leg", "R_Leg"], "verbose": bool(a.log_every)}
    lossconfig = {"weight_loss_rec": 1, "weight_loss_vposer": 0.001, "weight_contact": 0.1, "weight_collision": 0.5}
    fitter = ClipBatchFitter(fittingconfig, lossconfig)
    try:
        sized = [(s, d.shape[0]) for s, d in zip(scenes, data)]
        if a.mix_scenes:
            for paths, idx in plan_batches_scenes(sized, a.clips_per_batch):
                # (a scene some slot holds under its path is not read again: the fitter reuses the slot)
                held = {fitter.scene_key, *fitter._slot_keys}
                ent = [(p, None if p in held else io.read_scene_points(p)) for p in paths]
                res = fitter.fit([(data[i], cams[i]) for i in idx], log_every=a.log_every, scenes=ent,
                                 clip_scene=[paths.index(sized[i][0]) for i in idx])
                for i, (body_rec, scale, camera_ext) in zip(idx, res):
                    io.save_result(body_rec.detach().cpu().numpy(), scale, camera_ext.detach().cpu().numpy(),
                                   clip_output_dir(a.fit_root, a.clips[i]))
                frames = sorted({sized[i][1] for i in idx})
                print(f"[INFO][fitting] batch of {len(idx)} clips x {'/'.join(map(str, frames))} frames on {len(paths)} scenes fitted")
            print("[INFO][fitting] fitting finish, returning optimal value")
            return 0
        batches = plan_batches_mixed(sized, a.clips_per_batch) if a.mix_lengths else \
            [(scene, idx) for scene, _, idx in plan_batches(sized, a.clips_per_batch)]
        for scene, idx in batches:
            pts = None if scene == fitter.scene_key else io.read_scene_points(scene)
            res = fitter.fit([(data[i], cams[i]) for i in idx], pts, scene_key=scene, log_every=a.log_every)
            for i, (body_rec, scale, camera_ext) in zip(idx, res):
                io.save_result(body_rec.detach().cpu().numpy(), scale, camera_ext.detach().cpu().numpy(),
                               clip_output_dir(a.fit_root, a.clips[i]))
            frames = sorted({sized[i][1] for i in idx})
            print(f"[INFO][fitting] batch of {len(idx)} clips x {'/'.join(map(str, frames))} frames fitted ({scene})")
    finally:
        fitter.close()
    print("[INFO][fitting] fitting finish, returning optimal value")
    return 0


if __name__ == "__main__":
    sys.exit(main())
