"""The pose kernels limited to the joints an iteration's loss can reach (plan_pose_joints, csrc/fdc_forms.h) against the same
fit with FDCAP_POSE_TRIM=0, where they treat all 55 joints alike: the same bytes.  19 frames (one full 16-row block and a ragged
one), a 400-vertex body, a 2000-point scene, 10 iterations (eight of phase 1, two of phase 2).  The contact sets: the legs (32 per
leg); the legs and one vertex whose highest skinning joint lies in 12 .. 22; the legs and one vertex skinned to the last finger
joint, which makes the plan the full one.  Compared: body_rec, scale, camera_ext and the whole loss history; a difference may only
be the sign of a zero (an accumulator that took -0 terms from the dropped joints may hold +0).  A fit without a contact term
(weight_contact = 0) reaches the chain in phase 1 through nothing at all -- the plan is the root alone, (jn, jr, nlev) = (1, 1, 1)
-- and the gradient of a phase-1 backward issued AFTER the fit's phase-2 iterations is compared too: whatever a limited launch
does not compute (the decoder-output gradient of the body joints at or above jr) it must still write."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.fitting import ClipBatchFitter, FittingOP, first_phase2_iter
from fdcap_amd.io import read_camerapose
from tests.pose_trim_build import cpu_plan

pytestmark = pytest.mark.gpu
N, V, NS, ITERS = 19, 400, 2000, 10
FULL = (55, 55, 11, 1)


@pytest.fixture(scope="module")
def model():
    bm = synth.make_body_model(V, seed=51)
    vp = synth.make_vposer(seed=52)
    scene = synth.make_scene(NS, seed=53)
    left, right = synth.make_contact_ids(bm.v_template, per_part=32, seed=54)
    assert len(left) == 32 and len(right) == 32
    top = np.array([np.flatnonzero(w).max() for w in bm.lbs_weights])       # highest joint each vertex is skinned to
    legs = np.concatenate([left, right])
    mid = np.flatnonzero((top >= 12) & (top <= 22) & ~np.isin(np.arange(V), legs))
    finger = np.flatnonzero(top == 54)
    assert mid.size and finger.size
    sets = {"legs": (left, right), "legs+mid": (left, np.append(right, mid[0])), "legs+finger": (left, np.append(right, finger[0]))}
    ja = {k: int(top[np.concatenate(v)].max()) + 1 for k, v in sets.items()}
    assert ja["legs"] <= 12 < ja["legs+mid"] <= 23 and ja["legs+finger"] == 55, ja
    return bm, vp, scene, sets, ja


def _joint_sets(ctx):
    out = (ctypes.c_int32 * 8)()
    capi.check(ctx.lib.fdcap_debug_pose_joint_sets(ctx.handle, out), "fdcap_debug_pose_joint_sets")
    return tuple(out[:4]), tuple(out[4:])


def _fit(model, which, log_every, trim, monkeypatch, probe=False, weight_contact=None):
    bm, vp, scene, sets, _ = model
    lossconfig = {} if weight_contact is None else {"weight_contact": weight_contact}
    left, right = sets[which]
    clip = synth.make_clip(N, seed=55, num_outliers=2)
    if trim: monkeypatch.delenv("FDCAP_POSE_TRIM", raising=False)
    else: monkeypatch.setenv("FDCAP_POSE_TRIM", "0")                      # (read by every fdcap_opt_create)
    fop = FittingOP({"num_iter": ITERS}, lossconfig, N, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=np.concatenate([left, right]),
                    camera_ext=read_camerapose(clip.camerapose_lines), n_left=len(left))
    body, scale, cam = fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=log_every)
    out = {"body": body.cpu().numpy(), "scale": np.float32(scale), "cam": cam.cpu().numpy()}
    if log_every:
        for k, v in dataclasses.asdict(fop.log).items(): out["log_" + k] = np.asarray(v, dtype=np.float64)
    plans = {"last": _joint_sets(fop.ctx)[1]}                             # the backward of the fit's last iteration: phase 2
    if probe:
        # one more backward of iteration 0 (phase 1) on the finished fit, without and with logging: the plans of phase 1
        lib, h, P = fop.ctx.lib, fop.ctx.handle, first_phase2_iter(ITERS)
        for name, log_terms in (("phase1", 0), ("phase1_log", 1)):
            capi.check(lib.fdcap_opt_backward(h, 0, P, log_terms, capi.current_stream()), "fdcap_opt_backward")
            plans[name] = _joint_sets(fop.ctx)
            dx = torch.full((N, 78), float("nan"), device="cuda")
            capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, capi.current_stream()), "fdcap_opt_get_grads")
            out["grad_" + name] = dx.cpu().numpy()
        torch.cuda.synchronize()
    fop.close()
    return out, plans


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.atleast_1d(a[k]), np.atleast_1d(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert np.all(np.isfinite(x)), k
        assert np.array_equal(x, y), (k, np.abs(x - y).max())
        bits = np.uint32 if x.dtype.itemsize == 4 else np.uint64
        differ = x.view(bits) != y.view(bits)
        assert np.all(x[differ] == 0), (k, "bits differ somewhere else than in the sign of a zero")


@pytest.mark.parametrize("log_every", [0, 1, 3])
@pytest.mark.parametrize("which", ["legs", "legs+mid", "legs+finger"])
def test_a_fit_with_limited_joint_sets_gives_the_bytes_of_the_full_sets(model, which, log_every, monkeypatch):
    got, _ = _fit(model, which, log_every, True, monkeypatch)
    want, _ = _fit(model, which, log_every, False, monkeypatch)
    if log_every: assert len(got["log_total"]) == len([i for i in range(ITERS) if i % log_every == 0 or i == ITERS - 1])
    _same(got, want)


@pytest.mark.parametrize("which", ["legs", "legs+mid", "legs+finger"])
def test_the_joint_sets_of_the_launches_are_the_cpu_plans(model, which, monkeypatch):
    ja = model[4][which]
    got, plans = _fit(model, which, 0, True, monkeypatch, probe=True)
    # phase 2 has no contact state and reads the world joints; phase 1 reaches the chain through the contact set's joints only,
    # unless the iteration logs.  Forward and backward of an iteration take the same sets.
    assert plans["last"] == cpu_plan(0, False, True)
    assert plans["phase1"] == (cpu_plan(ja, True, False),) * 2
    assert plans["phase1_log"] == (cpu_plan(ja, True, True),) * 2
    if which == "legs": assert plans["phase1"][0][0] <= 12 and plans["last"][:2] == (23, 23)
    if which == "legs+mid": assert 12 < plans["phase1"][0][0] <= 23
    if which == "legs+finger": assert plans["phase1"][0] == FULL
    want, plans = _fit(model, which, 0, False, monkeypatch, probe=True)
    assert plans == {"last": FULL, "phase1": (FULL, FULL), "phase1_log": (FULL, FULL)}, plans
    assert cpu_plan(ja, True, False, trim=False) == FULL
    _same(got, want)                                                      # (with the gradients of the two phase-1 backwards after phase 2)


@pytest.mark.parametrize("log_every", [0, 3])
def test_a_fit_without_a_contact_term_gives_the_bytes_of_the_full_sets(model, log_every, monkeypatch):
    """weight_contact = 0: a phase-1 iteration that does not log needs neither the contact state nor the world joints, its plan is
    the root alone and no body joint but the root has a rotation backward.  The fit, and the gradient of a phase-1 backward that
    follows the fit's phase-2 iterations (whose launch left non-zero decoder-output gradients behind), equal the full sets'."""
    got, plans = _fit(model, "legs", log_every, True, monkeypatch, probe=True, weight_contact=0.0)
    assert plans["phase1"] == (cpu_plan(0, False, False),) * 2 == ((1, 1, 1, 0),) * 2
    assert plans["phase1_log"] == (cpu_plan(0, False, True),) * 2
    want, plans = _fit(model, "legs", log_every, False, monkeypatch, probe=True, weight_contact=0.0)
    assert plans["phase1"] == (FULL, FULL)
    assert np.abs(want["grad_phase1"]).max() > 0
    _same(got, want)


def test_a_batch_of_clips_with_limited_joint_sets_gives_the_bytes_of_the_full_sets(model, monkeypatch):
    bm, vp, scene, sets, _ = model
    left, right = sets["legs"]
    clips = []
    for seed, n in ((61, 7), (62, 6), (63, 6)):
        c = synth.make_clip(n, seed=seed, num_outliers=1)
        clips.append((c.body_params, read_camerapose(c.camerapose_lines)))
    res = []
    for trim in (True, False):
        if trim: monkeypatch.delenv("FDCAP_POSE_TRIM", raising=False)
        else: monkeypatch.setenv("FDCAP_POSE_TRIM", "0")
        f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=np.concatenate([left, right]))
        out = {}
        for k, ((b, s, c), log) in enumerate(zip(f.fit(clips, scene, log_every=1), f.logs)):
            out[f"{k}_body"] = b.cpu().numpy(); out[f"{k}_scale"] = np.float32(s); out[f"{k}_cam"] = c.cpu().numpy()
            for name, v in dataclasses.asdict(log).items(): out[f"{k}_log_{name}"] = np.asarray(v, dtype=np.float64)
        res.append((out, _joint_sets(f.ctx)[1]))
        f.close()
    # (the last iteration logs: the contact term is printed in phase 2 as well, so its launches keep the contact state)
    assert res[0][1] == cpu_plan(model[4]["legs"], True, True) and res[1][1] == FULL
    _same(res[0][0], res[1][0])
