"""A batch of clips (fdcap_opt_create_clips, fitting.ClipBatchFitter) against the stand-alone fits of its clips: the same bits
wherever both select the same kernel forms, no leak across clip boundaries, checkpoint / resume, refusals, the multi-clip CLI."""
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
N, ITERS = 40, 10
LOG_FIELDS = ("iters", "l_rec", "l_vposer", "loss_smoothing", "loss_contact", "loss_world_smoothing", "total")


def _model():
    bm = synth.make_body_model(300, seed=31)
    vp = synth.make_vposer(seed=32)
    scene = synth.make_scene(9000, seed=34)
    l, r = synth.make_contact_ids(bm.v_template, per_part=24, seed=35)
    return bm, vp, scene, np.concatenate([l, r])


def _clip(seed, n=N):
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


def _same(a, b):
    assert np.array_equal(a[0], b[0]), np.abs(a[0] - b[0]).max()
    assert a[1] == b[1], (a[1], b[1])
    assert np.array_equal(a[2], b[2]), np.abs(a[2] - b[2]).max()
    for k in LOG_FIELDS:
        assert np.array_equal(np.array(getattr(a[3], k)), np.array(getattr(b[3], k))), k
    assert np.array_equal(a[4], b[4])


def test_a_batch_gives_each_clip_its_stand_alone_bits():
    model = _model()
    clips = [_clip(s) for s in (41, 42, 43)]
    batch, bforms = _batch(model, clips)
    assert any(len(b[4]) for b in batch), "no clip has outliers"
    for k, clip in enumerate(clips):
        alone, aforms = _alone(model, clip)
        assert sorted(set(aforms.split(";"))) == sorted(set(bforms.split(";"))), (aforms, bforms)
        _same(batch[k], alone)


def test_one_clip_through_the_batch_entry_point_is_fdcap_opt_create():
    model = _model()
    clip = _clip(44)
    (b,), _ = _batch(model, [clip])
    a, _ = _alone(model, clip)
    _same(b, a)


def test_clips_of_a_batch_do_not_see_each_other():
    model = _model()
    A, B, B2, C = _clip(45), _clip(46), _clip(47), _clip(48)
    r1, _ = _batch(model, [A, B, C])
    r2, _ = _batch(model, [A, B2, C])
    _same(r1[0], r2[0])
    _same(r1[2], r2[2])
    assert not np.array_equal(r1[1][0], r2[1][0]) and r1[1][1] != r2[1][1]


def test_checkpoint_of_a_batch_resumes_to_the_same_bits():
    bm, vp, scene, vid = _model()
    clips = [_clip(s) for s in (51, 52, 53)]
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
        body, sc, cam = torch.empty(3 * N, 75, device="cuda"), torch.empty(3, device="cuda"), torch.empty(3 * N, 16, device="cuda")
        capi.check(f.ctx.lib.fdcap_opt_get_results(h, capi.dptr(body), capi.dptr(sc), capi.dptr(cam), st), "results")
        return body.cpu().numpy(), sc.cpu().numpy(), cam.cpu().numpy()

    f = fitter()
    run(f, 0, ITERS)
    ref = results(f)
    f.close()
    f = fitter()
    run(f, 0, 5)
    lib, h, st = f.ctx.lib, f.ctx.handle, capi.current_stream()
    assert lib.fdcap_opt_state_len(h) == 2 * 3 * N * (78 + 16) + 2 * 3
    state = torch.empty(lib.fdcap_opt_state_len(h), device="cuda")
    capi.check(lib.fdcap_opt_export_state(h, capi.dptr(state), st), "export")
    rows_x, rows_cam, scale = f._rows_x.clone(), f._rows_cam.clone(), f._scale.clone()
    f.close()
    g = fitter()
    g._rows_x.copy_(rows_x)
    g._rows_cam.copy_(rows_cam)
    g._scale.copy_(scale)
    capi.check(g.ctx.lib.fdcap_opt_import_state(g.ctx.handle, capi.dptr(state), capi.current_stream()), "import")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.check(g.ctx.lib.fdcap_opt_check_finite(g.ctx.handle, capi.dptr(cnt), capi.current_stream()), "finite")
    run(g, 5, ITERS)
    got = results(g)
    g.close()
    assert int(cnt.item()) == 0
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)


def test_a_batch_refuses_what_it_does_not_do():
    bm, vp, scene, vid = _model()
    f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    f.set_scene(scene)
    lib, h = f.ctx.lib, f.ctx.handle
    t = [torch.zeros(4 * N + 8, 78, device="cuda") for _ in range(5)]
    p = [capi.dptr(x) for x in t]

    def create(K, n_total, n_local, frame0):
        oc = capi.OptConfig(n_total, n_local, frame0, 0.005, 1.0, 0.001, 0.1, 0.1, 1.0, 1.0, 0.5, 1.8, 0)
        return lib.fdcap_opt_create_clips(h, ctypes.byref(oc), K, *p)

    E_ARG, E_STATE = -1, -2
    assert create(0, N, N, 0) == E_ARG
    assert create(2, 2 * N, N, 0) == E_ARG
    assert create(2, N, N // 2, N // 2) == E_ARG
    assert create(2, N, N, 0) == 0
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


# the same three clips at the reference's size, in a child process: FDCAP_CLIP_FORMS_MIN_ROWS is read once per process
_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, %(root)r)
import numpy as np, torch
import fdcap_amd
from fdcap_amd import capi, synth
from fdcap_amd.fitting import ClipBatchFitter, FittingOP, first_phase2_iter
from fdcap_amd.io import read_camerapose
N, K, ITERS, GRAD = 300, 3, 10, %(grad)d
bm = synth.make_body_model(10475, seed=0); vp = synth.make_vposer(seed=1)
scene = synth.make_scene(50000, seed=2); l, r = synth.make_contact_ids(bm.v_template, per_part=250, seed=4)
vid = np.concatenate([l, r])
clips = []
for s in (61, 62, 63):
    c = synth.make_clip(N, seed=s)
    clips.append((c.body_params, read_camerapose(c.camerapose_lines)))
lib = capi.load_library()
buf = ctypes.create_string_buffer(4096)
P = first_phase2_iter(ITERS)
def forms(reset):
    lib.fdcap_debug_kernel_forms(buf, 4096, 1 if reset else 0)
    return sorted(set(buf.value.decode().split(";")))
def grads(lib, h, n):
    capi.check(lib.fdcap_opt_backward(h, 0, P, 0, capi.current_stream()), "backward")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, capi.current_stream()), "grads")
    return dx.cpu().numpy()
out = {"ok": True, "bad": []}
forms(True)
f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
f.set_scene(scene)
if GRAD:
    f.prepare(clips); gb = grads(f.ctx.lib, f.ctx.handle, K * N)
else:
    res = f.fit(clips, log_every=1)
    batch = [(b.cpu().numpy(), float(s), c.cpu().numpy(), f.logs[k]) for k, (b, s, c) in enumerate(res)]
f.close()
bforms = forms(False)
for k, (body, cam) in enumerate(clips):
    forms(True)
    fop = FittingOP({"num_iter": ITERS}, {}, N, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=cam)
    if GRAD:
        x78 = torch.empty(N, 78, device="cuda")
        capi.check(fop.ctx.lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(body).cuda()), N, capi.dptr(x78), capi.current_stream()), "p78")
        fop.init(x78)
        ga = grads(fop.ctx.lib, fop.ctx.handle, N)
        g = gb[k * N:(k + 1) * N]
        ok = np.abs(ga).max() > 0 and np.allclose(g, ga, rtol=2e-4, atol=2e-6 * np.abs(ga).max())
        if not ok: out["bad"].append([k, "grad", float(np.abs(g - ga).max())])
    else:
        b, s, c = fop.fitting(torch.tensor(body).cuda(), "global", log_every=1)
        a = (b.cpu().numpy(), float(s), c.cpu().numpy(), fop.log)
        z = batch[k]
        if not np.array_equal(a[0], z[0]): out["bad"].append([k, "body", float(np.abs(a[0] - z[0]).max())])
        if a[1] != z[1]: out["bad"].append([k, "scale", a[1], z[1]])
        if not np.array_equal(a[2], z[2]): out["bad"].append([k, "cam", float(np.abs(a[2] - z[2]).max())])
        for fld in ("l_rec", "l_vposer", "loss_smoothing", "loss_contact", "loss_world_smoothing", "total"):
            if not np.array_equal(np.array(getattr(a[3], fld)), np.array(getattr(z[3], fld))): out["bad"].append([k, fld])
    fop.close()
    af = forms(False)
    if af != bforms: out["bad"].append([k, "forms", af, bforms])
out["ok"] = not out["bad"]
print("RESULT " + json.dumps(out))
"""


def _child(grad, clip_forms):
    env = dict(os.environ)
    env.pop("FDCAP_CLIP_FORMS_MIN_ROWS", None)
    if clip_forms:
        env["FDCAP_CLIP_FORMS_MIN_ROWS"] = "256"
    p = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "grad": grad}], env=env, capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and line, (p.stdout[-1500:], p.stderr[-3000:])
    return json.loads(line[-1][7:])


def test_a_batch_at_the_reference_size_gives_each_clip_its_stand_alone_bits():
    r = _child(grad=0, clip_forms=True)
    assert r["ok"], r["bad"]


def test_default_forms_at_the_reference_size_give_each_clip_its_stand_alone_gradient():
    r = _child(grad=1, clip_forms=False)
    bad = [b for b in r["bad"] if b[1] != "forms"]          # (900 rows select the clip-sized forms, 300 do not: the point of this test)
    assert not bad, bad


def test_multi_clip_cli_writes_what_the_one_clip_cli_writes(tmp_path, monkeypatch):
    from fdcap_amd import assets, cli, io
    bm, vp, scene, vid = _model()
    monkeypatch.setattr(assets, "load_smplx_npz", lambda *a, **k: bm)
    monkeypatch.setattr(assets, "load_vposer_snapshot", lambda *a, **k: vp)
    monkeypatch.setattr(io, "read_contact_ids", lambda folder, parts: vid[:len(vid) // 2] if parts[0] == "L_Leg" else vid[len(vid) // 2:])
    root, bodies = tmp_path / "scenes", tmp_path / "bodies"
    os.makedirs(root)
    io.write_ply_points(str(root / "room.ply"), scene)
    paths = []
    for i in range(4):
        c = synth.make_clip(24, seed=70 + i)
        name = f"video-{i}"
        bp = str(bodies / name) + "/"
        io.write_body_gen(c.body_params, bp)
        os.makedirs(root / name)
        os.symlink(root / "room.ply", root / name / "meshed-poisson.ply")
        with open(root / name / "camerapose.txt", "w") as fh:
            fh.write("\n".join(c.camerapose_lines) + "\n")
        paths.append(bp)
    common = ["--scene-root", str(root), "--num-iter", "6"]
    assert cli.main(["--clips", *paths, "--fit-root", str(tmp_path / "multi"), "--clips-per-batch", "3", *common]) == 0
    for bp in paths:
        one = str(tmp_path / "one" / cli.sample_name_of(bp))
        assert cli.main([bp, one, "global", *common]) == 0
        multi = cli.clip_output_dir(str(tmp_path / "multi"), bp)
        files = sorted(os.listdir(one))
        assert files == sorted(os.listdir(multi)) and len(files) == 24
        for fn in files:
            with open(os.path.join(one, fn), "rb") as fh:
                a = pickle.load(fh)
            with open(os.path.join(multi, fn), "rb") as fh:
                b = pickle.load(fh)
            assert a.keys() == b.keys()
            for k in a:
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (bp, fn, k)
