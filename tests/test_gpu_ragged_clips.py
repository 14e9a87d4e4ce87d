"""A batch of clips of DIFFERENT lengths (fdcap_opt_create_clips_var, fitting.ClipBatchFitter, cli --mix-lengths) against the
stand-alone fits of its clips: the same bits wherever both select the same kernel forms, nothing leaks across clip boundaries and a
clip's offset in the batch does not matter, equal lengths are fdcap_opt_create_clips' batch, checkpoint / resume, refusals, the CLI.
Shapes and helpers as tests/test_gpu_multiclip.py: a 300-vertex body, a 9000-point scene, 2 x 24 contact vertices, 10 iterations
(the phase switch at first_phase2_iter(10) = 8 is crossed), every iteration logged, two outlier rows per clip."""
import ctypes
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.fitting import ClipBatchFitter, FittingOP, first_phase2_iter
from fdcap_amd.io import read_camerapose

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 10
LOG_FIELDS = ("iters", "l_rec", "l_vposer", "loss_smoothing", "loss_contact", "loss_world_smoothing", "total")
E_ARG, E_STATE = -1, -2


@pytest.fixture(scope="module")
def model():
    bm = synth.make_body_model(300, seed=31)
    vp = synth.make_vposer(seed=32)
    scene = synth.make_scene(9000, seed=34)
    l, r = synth.make_contact_ids(bm.v_template, per_part=24, seed=35)
    return bm, vp, scene, np.concatenate([l, r])


def _clip(seed, n):
    c = synth.make_clip(n, seed=seed, num_outliers=2)
    return c.body_params, read_camerapose(c.camerapose_lines)


def _forms(reset):
    buf = ctypes.create_string_buffer(4096)
    capi.load_library().fdcap_debug_kernel_forms(buf, 4096, 1 if reset else 0)
    return buf.value.decode()


def _alone(model, clip, iters=ITERS):
    bm, vp, scene, vid = model
    _forms(True)
    fop = FittingOP({"num_iter": iters}, {}, clip[0].shape[0], body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                    camera_ext=clip[1])
    body, scale, cam = fop.fitting(torch.tensor(clip[0]).cuda(), "global", log_every=1)
    out = (body.cpu().numpy(), float(scale), cam.cpu().numpy(), fop.log, fop.idx1)
    fop.close()
    return out, _forms(False)


def _batch(model, clips, iters=ITERS):
    bm, vp, scene, vid = model
    _forms(True)
    f = ClipBatchFitter({"num_iter": iters}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    res = f.fit(clips, scene, log_every=1)
    out = [(b.cpu().numpy(), float(s), c.cpu().numpy(), log, i1) for (b, s, c), log, i1 in zip(res, f.logs, f.idx1)]
    f.close()
    return out, _forms(False)


def _same(a, b, nan_terms=()):
    """nan_terms: printed terms that are NaN on BOTH sides (a mean over no elements, as torch prints it: a clip of one or two
    frames has no second difference, of one frame no first difference) -- they must be NaN in the same places."""
    assert a[0].shape == b[0].shape
    assert np.array_equal(a[0], b[0]), np.abs(a[0] - b[0]).max()
    assert a[1] == b[1], (a[1], b[1])
    assert np.array_equal(a[2], b[2]), np.abs(a[2] - b[2]).max()
    for k in LOG_FIELDS:
        x, y = np.array(getattr(a[3], k), dtype=np.float64), np.array(getattr(b[3], k), dtype=np.float64)
        assert np.array_equal(x, y, equal_nan=k in nan_terms), k
        assert np.all(np.isfinite(x)) or k in nan_terms, k
    assert np.array_equal(a[4], b[4])


def test_a_batch_of_four_lengths_gives_each_clip_its_stand_alone_bits(model):
    """Lengths (40, 33, 24, 10).  The shortest clip is 10 frames, not 3: with 48 contact vertices a stand-alone fit of 9 frames or
    fewer takes nn_direct_kernel for the in-loop search (fdc_forms.h, evaluated on the CPU: tests/test_ragged_clips_cpu.py), the
    107-row batch nn_stream4_kernel, and the contract is bit equality under EQUAL forms.  From 10 rows on every plan agrees.  The
    3-frame clip -- the shortest with a second difference -- runs in test_a_three_frame_clip_fits_at_either_end_of_a_batch."""
    clips = [_clip(s, n) for s, n in ((41, 40), (42, 33), (43, 24), (44, 10))]
    batch, bforms = _batch(model, clips)
    assert any(len(b[4]) for b in batch), "no clip has outliers"
    for k, clip in enumerate(clips):
        alone, aforms = _alone(model, clip)
        assert sorted(set(aforms.split(";"))) == sorted(set(bforms.split(";"))), (aforms, bforms)
        _same(batch[k], alone)


def test_a_batch_of_one_two_and_three_frames_gives_each_clip_its_stand_alone_bits(model):
    """Lengths (1, 2, 3, 3): nine rows, which plan exactly as each clip's own rows do (nn_direct_kernel included;
    tests/test_ragged_clips_cpu.py evaluates the plans), so the contract holds against the stand-alone FittingOP fits -- which fit
    one, two and three frames.  On the device: the stencils of a 3-frame clip (one second difference, two first differences), the
    (n - 2) and (n - 1) denominators, the zero weights below three and below two frames, `scale` stepped over 1 .. 3 rows.  The
    printed smoothing term of the 1- and 2-frame clips and the world-smoothing term of the 1-frame clip are means over nothing: NaN
    in the batch's log and in the stand-alone fit's alike (with them the printed total)."""
    lens = (1, 2, 3, 3)
    clips = [_clip(s, n) for s, n in zip((57, 58, 59, 60), lens)]
    batch, bforms = _batch(model, clips)
    assert "nn_direct_kernel" in bforms
    nan_terms = {1: ("loss_smoothing", "loss_world_smoothing", "total"), 2: ("loss_smoothing", "total"), 3: ()}
    for k, clip in enumerate(clips):
        alone, aforms = _alone(model, clip)
        assert sorted(set(aforms.split(";"))) == sorted(set(bforms.split(";"))), (aforms, bforms)
        _same(batch[k], alone, nan_terms[lens[k]])
    assert min(batch[2][3].loss_smoothing) > 0.0 and min(batch[3][3].loss_smoothing) > 0.0


def test_a_three_frame_clip_fits_at_either_end_of_a_batch(model):
    """3 frames: one second difference, two first differences.  Whether it is the batch's first or last clip -- rows 2 .. 5 or the
    last three -- it gets the same bits, and so does its 40-frame neighbour; every printed term is finite and the smoothing term
    is not zero (the stencil of frame 0 reaches frames 1 and 2, the others' are cut)."""
    T, A = _clip(45, 3), _clip(46, 40)
    r1, _ = _batch(model, [T, A])
    r2, _ = _batch(model, [A, T])
    _same(r1[0], r2[1])
    _same(r1[1], r2[0])
    log = r1[0][3]
    for k in LOG_FIELDS:
        assert np.all(np.isfinite(np.array(getattr(log, k), dtype=np.float64))), k
    assert min(log.loss_smoothing) > 0.0
    assert np.all(np.isfinite(r1[0][0])) and np.isfinite(r1[0][1])


def test_clips_of_a_ragged_batch_do_not_see_each_other_and_offsets_do_not_matter(model):
    A, B, B2, C = _clip(47, 40), _clip(48, 33), _clip(49, 20), _clip(50, 24)
    r1, _ = _batch(model, [A, B, C])
    r2, _ = _batch(model, [A, B2, C])
    _same(r1[0], r2[0])
    _same(r1[2], r2[2])                                         # (C starts at row 2 + 73 in one batch, 2 + 60 in the other)
    # (the evidence is above: A and C keep their bits.  This line only shows that the middle clips really differed)
    assert r1[1][0].shape != r2[1][0].shape and r1[1][1] != r2[1][1]


def test_equal_lengths_through_the_new_call_are_the_equal_length_batch(model, monkeypatch):
    clips = [_clip(s, 40) for s in (51, 52, 53)]
    ref, rforms = _batch(model, clips)
    lib = capi.load_library()
    calls = []

    def through_var(h, cfg_ref, K, *bufs):                      # ClipBatchFitter calls fdcap_opt_create_clips for equal lengths
        oc = cfg_ref._obj
        n = oc.n_total
        fields = [getattr(oc, name) for name, _ in capi.OptConfig._fields_]
        oc2 = capi.OptConfig(*fields)
        oc2.n_total = oc2.n_local = K * n
        calls.append(K)
        return lib.fdcap_opt_create_clips_var(h, ctypes.byref(oc2), K, (ctypes.c_int32 * K)(*([n] * K)), *bufs)

    monkeypatch.setattr(lib, "fdcap_opt_create_clips", through_var)
    got, gforms = _batch(model, clips)
    assert calls == [3]
    assert sorted(set(gforms.split(";"))) == sorted(set(rforms.split(";")))
    for a, b in zip(got, ref):
        _same(a, b)


def test_checkpoint_of_a_ragged_batch_resumes_to_the_same_bits(model):
    bm, vp, scene, vid = model
    lens = (40, 33, 24)
    total = sum(lens)
    clips = [_clip(s, n) for s, n in zip((54, 55, 56), lens)]
    P = first_phase2_iter(ITERS)

    def fitter():
        f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
        f.set_scene(scene)
        f.prepare(clips)
        return f

    def run(f, ii0, ii1):
        n = ctypes.c_int32(0)
        capi.check(f.ctx.lib.fdcap_opt_run(f.ctx.handle, ii0, ii1, ITERS, P, 0, None, 0, 0, ctypes.byref(n), capi.current_stream()), "run")

    def results(f):
        h, st = f.ctx.handle, capi.current_stream()
        body, sc, cam = torch.empty(total, 75, device="cuda"), torch.empty(3, device="cuda"), torch.empty(total, 16, device="cuda")
        capi.check(f.ctx.lib.fdcap_opt_get_results(h, capi.dptr(body), capi.dptr(sc), capi.dptr(cam), st), "results")
        return body.cpu().numpy(), sc.cpu().numpy(), cam.cpu().numpy()

    f = fitter()
    run(f, 0, ITERS)
    ref = results(f)
    f.close()
    f = fitter()
    run(f, 0, 5)
    lib, h, st = f.ctx.lib, f.ctx.handle, capi.current_stream()
    assert lib.fdcap_opt_state_len(h) == 2 * total * (78 + 16) + 2 * 3
    state = torch.empty(lib.fdcap_opt_state_len(h), device="cuda")
    capi.check(lib.fdcap_opt_export_state(h, capi.dptr(state), st), "export")
    rows_x, rows_cam, scale = f._rows_x.clone(), f._rows_cam.clone(), f._scale.clone()
    f.close()
    g = fitter()
    g._rows_x.copy_(rows_x)
    g._rows_cam.copy_(rows_cam)
    g._scale.copy_(scale)
    capi.check(g.ctx.lib.fdcap_opt_import_state(g.ctx.handle, capi.dptr(state), capi.current_stream()), "import")
    run(g, 5, ITERS)
    got = results(g)
    g.close()
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


def test_the_new_call_refuses_bad_lengths_and_a_ragged_batch_what_a_batch_does_not_do(model):
    bm, vp, scene, vid = model
    f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    f.set_scene(scene)
    lib, h = f.ctx.lib, f.ctx.handle
    t = [torch.zeros(4 * 40 + 8, 78, device="cuda") for _ in range(5)]
    p = [capi.dptr(x) for x in t]

    def create(lens, n_total, n_local=None, frame0=0):
        oc = capi.OptConfig(n_total, n_total if n_local is None else n_local, frame0, 0.005, 1.0, 0.001, 0.1, 0.1, 1.0, 1.0, 0.5, 1.8, 0)
        arr = None if lens is None else (ctypes.c_int32 * len(lens))(*lens)
        return lib.fdcap_opt_create_clips_var(h, ctypes.byref(oc), 2 if lens is None else len(lens), arr, *p)

    assert create((40, 0, 24), 64) == E_ARG                     # a zero length
    assert create((40, -3, 24), 61) == E_ARG
    assert create(None, 64) == E_ARG                            # no array
    assert create((40, 33, 24), 96) == E_ARG                    # a sum that is not the config's
    assert create((40, 33, 24), 97, 96) == E_ARG
    assert create((40, 33, 24), 97, 97, 1) == E_ARG
    assert create((40, 33, 24), 97) == 0
    st = capi.current_stream()
    stage = capi.Fit2dStage(1, 1, 0, 0, 1, 1, 0, 0, 0)
    n = ctypes.c_int32(0)
    assert lib.fdcap_opt_detect_contact(h, 1, p[0], st) == E_STATE
    assert lib.fdcap_opt_backward_local2(h, p[0], 1, st) == E_STATE
    assert lib.fdcap_opt_set_dct(h, p[0], 60, 5, p[1], st) == E_STATE
    assert lib.fdcap_opt_backward_dct(h, 1.0, 1.0, 1.0, 0, st) == E_STATE
    assert lib.fdcap_opt_set_keypoints(h, p[0], st) == E_STATE
    assert lib.fdcap_opt_backward_fit2d(h, ctypes.byref(stage), 0, st) == E_STATE
    assert lib.fdcap_opt_step_x(h, 1, st) == E_STATE
    assert lib.fdcap_opt_forward_ahead(h, 0, 8, 0, st) == E_STATE
    assert lib.fdcap_opt_halo_exchange(h, st) == E_STATE
    assert lib.fdcap_opt_exchange(h, 0, 8, st) == E_STATE
    assert lib.fdcap_opt_step_rows_and_pack(h, 0, 8, p[0], st) == E_STATE
    assert lib.fdcap_opt_unpack_and_step_scale(h, 0, 8, p[0], 0, 1, st) == E_STATE
    assert lib.fdcap_opt_run(h, 0, 1, ITERS, 8, 0, None, 0, 2, ctypes.byref(n), st) == E_STATE
    torch.cuda.synchronize()
    f.close()


# Clip boundaries through the clip-sized forms, in a child process (FDCAP_CLIP_FORMS_MIN_ROWS is read once per process): the full
# body (10 475 vertices, 500 contact vertices), lengths (100, 75, 81) = 256 rows -- clips start at rows 100 and 175 of the batch,
# both strictly inside a block of 32 frames, no length a multiple of 32 -- so blend_skin_fwd_kernel's blocks 3 and 5 straddle a
# boundary, and the K-split data gradient's two row blocks per workgroup do as well.  Every stand-alone fit (100, 75, 81 >= 64
# rows) selects the same two forms.
_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch
import fdcap_amd
from fdcap_amd import capi, synth
from fdcap_amd.fitting import ClipBatchFitter, FittingOP
from fdcap_amd.io import read_camerapose
LENS, ITERS = (100, 75, 81), 6
bm = synth.make_body_model(10475, seed=0); vp = synth.make_vposer(seed=1)
scene = synth.make_scene(50000, seed=2); l, r = synth.make_contact_ids(bm.v_template, per_part=250, seed=4)
vid = np.concatenate([l, r])
clips = []
for s, n in zip((61, 62, 63), LENS):
    c = synth.make_clip(n, seed=s, num_outliers=2)
    clips.append((c.body_params, read_camerapose(c.camerapose_lines)))
lib = capi.load_library()
buf = ctypes.create_string_buffer(4096)
def forms(reset):
    lib.fdcap_debug_kernel_forms(buf, 4096, 1 if reset else 0)
    return sorted(set(buf.value.decode().split(";")))
out = {"ok": True, "bad": []}
forms(True)
f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
f.set_scene(scene)
res = f.fit(clips, log_every=1)
batch = [(b.cpu().numpy(), float(s), c.cpu().numpy(), f.logs[k], f.idx1[k]) for k, (b, s, c) in enumerate(res)]
f.close()
out["bforms"] = forms(False)
for k, (body, cam) in enumerate(clips):
    forms(True)
    fop = FittingOP({"num_iter": ITERS}, {}, LENS[k], body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=cam)
    b, s, c = fop.fitting(torch.tensor(body).cuda(), "global", log_every=1)
    a = (b.cpu().numpy(), float(s), c.cpu().numpy(), fop.log, fop.idx1)
    z = batch[k]
    if not np.array_equal(a[0], z[0]): out["bad"].append([k, "body", float(np.abs(a[0] - z[0]).max())])
    if a[1] != z[1]: out["bad"].append([k, "scale", a[1], z[1]])
    if not np.array_equal(a[2], z[2]): out["bad"].append([k, "cam", float(np.abs(a[2] - z[2]).max())])
    for fld in ("iters", "l_rec", "l_vposer", "loss_smoothing", "loss_contact", "loss_world_smoothing", "total"):
        if not np.array_equal(np.array(getattr(a[3], fld)), np.array(getattr(z[3], fld))): out["bad"].append([k, fld])
    if not np.array_equal(a[4], z[4]): out["bad"].append([k, "idx1"])
    fop.close()
    af = forms(False)
    for name in ("blend_skin_fwd_kernel", "panel_gemm3_rb2k_kernel"):
        if name not in af: out["bad"].append([k, "stand-alone forms", af])
out["ok"] = not out["bad"]
print("RESULT " + json.dumps(out))
"""


def test_clip_boundaries_inside_the_blocks_of_the_clip_sized_forms():
    env = dict(os.environ)
    env["FDCAP_CLIP_FORMS_MIN_ROWS"] = "64"
    p = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and line, (p.stdout[-1500:], p.stderr[-3000:])
    r = json.loads(line[-1][7:])
    assert "blend_skin_fwd_kernel" in r["bforms"] and "panel_gemm3_rb2k_kernel" in r["bforms"], r["bforms"]
    assert r["ok"], r["bad"]


def test_mix_lengths_cli_writes_what_the_one_clip_cli_writes(tmp_path, monkeypatch, model):
    from fdcap_amd import assets, cli, io
    bm, vp, scene, vid = model
    monkeypatch.setattr(assets, "load_smplx_npz", lambda *a, **k: bm)
    monkeypatch.setattr(assets, "load_vposer_snapshot", lambda *a, **k: vp)
    monkeypatch.setattr(io, "read_contact_ids", lambda folder, parts: vid[:len(vid) // 2] if parts[0] == "L_Leg" else vid[len(vid) // 2:])
    root, bodies = tmp_path / "scenes", tmp_path / "bodies"
    os.makedirs(root)
    io.write_ply_points(str(root / "room.ply"), scene)
    paths, lens = [], (24, 17, 24, 9)
    for i, n in enumerate(lens):
        c = synth.make_clip(n, seed=70 + i)
        name = f"video-{i}"
        bp = str(bodies / name) + "/"
        io.write_body_gen(c.body_params, bp)
        os.makedirs(root / name)
        os.symlink(root / "room.ply", root / name / "meshed-poisson.ply")
        with open(root / name / "camerapose.txt", "w") as fh:
            fh.write("\n".join(c.camerapose_lines) + "\n")
        paths.append(bp)
    common = ["--scene-root", str(root), "--num-iter", "6"]
    assert cli.plan_batches_mixed([("room", n) for n in lens], 3) == [("room", [0, 1, 2]), ("room", [3])]
    assert cli.main(["--clips", *paths, "--fit-root", str(tmp_path / "multi"), "--mix-lengths", "--clips-per-batch", "3", *common]) == 0
    for bp, n in zip(paths, lens):
        one = str(tmp_path / "one" / cli.sample_name_of(bp))
        assert cli.main([bp, one, "global", *common]) == 0
        multi = cli.clip_output_dir(str(tmp_path / "multi"), bp)
        files = sorted(os.listdir(one))
        assert files == sorted(os.listdir(multi)) and len(files) == n
        for fn in files:
            with open(os.path.join(one, fn), "rb") as fh:
                a = pickle.load(fh)
            with open(os.path.join(multi, fn), "rb") as fh:
                b = pickle.load(fh)
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (bp, fn, k)
