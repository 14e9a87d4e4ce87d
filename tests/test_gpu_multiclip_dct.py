"""Mode 'dct' for a batch of clips (fdcap_opt_set_dct_clips + fdcap_opt_run_dct, ClipBatchFitter.fit(mode='dct')) against the stand-alone
mode-'dct' fits of its clips (FittingOP): the same bits -- one clip, equal lengths, different lengths with tails in either order --
nothing leaks across clip boundaries, the second phase's gradient against the fp64 oracle per clip, the reference's own 'dct' run as a
batch of two copies, legacy_zero_grad, the refusals and a stretch cut in either phase.
Shapes as tests/test_gpu_dct_smoother.py::_dct_case: a 200-vertex body, a 1500-point scene, 2 x 8 contact vertices, 200 iterations
(first phase 0..189 in one launch, iteration 190 a no-op, nine second-phase iterations), two outlier rows per clip.
tests/test_dct_clips_cpu.py pins the tables of the lengths used here.

A batch equals its clips' stand-alone fits bit for bit where both select the same kernel forms (include/fdcap.h), and several stages
pick theirs by row count: 360 and 396 rows of a batch take the clip-sized forms, 60 to 150 rows of a stand-alone fit do not.  The
comparisons of a batch of several clips against stand-alone fits therefore run in ONE child process (this file as a script) that pins
the forms for both sides -- FDCAP_CLIP_FORMS_MIN_ROWS=32 is read once per process, fdcap_set_nn_kernel(2) selects the MFMA-filtered
search at every size -- and compares what fdcap_debug_kernel_forms noted; each test below asserts its scenario's outcome."""
import ctypes
import json
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.fitting import ClipBatchFitter, FittingOP
from fdcap_amd.io import load_dct_base, read_camerapose
from oracle.fitting import FittingOracle
from oracle.smplx import SMPLXOracle
from oracle.vposer import VPoserDecoder

pytestmark = pytest.mark.gpu
ITERS = 200
P = int(np.ceil(ITERS * 0.95 - 1e-9))
N2 = ITERS - P - 1
E_ARG, E_STATE = -1, -2


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    return _model()


def _model():
    bm = synth.make_body_model(200, seed=131)
    vp = synth.make_vposer(seed=132)
    scene = synth.make_scene(1500, seed=134)
    l, r = synth.make_contact_ids(bm.v_template, per_part=8, seed=135)
    return bm, vp, scene, np.concatenate([l, r]), load_dct_base(None)


_CLIPS = {}


def _clip(seed, n):
    """(body [n,75], camera_ext [n,4,4], c_dct_init [n // 60,23,3,5], camerapose lines), made once"""
    if (seed, n) not in _CLIPS:
        c = synth.make_clip(n, seed=seed, num_outliers=2)
        rng = np.random.Generator(np.random.PCG64(seed + 1000))
        c0 = rng.standard_normal((n // 60, 23, 3, 5)).astype(np.float32)
        _CLIPS[(seed, n)] = (c.body_params, read_camerapose(c.camerapose_lines), c0, c.camerapose_lines)
    return _CLIPS[(seed, n)]


def _forms(reset):
    buf = ctypes.create_string_buffer(4096)
    capi.load_library().fdcap_debug_kernel_forms(buf, 4096, 1 if reset else 0)
    return buf.value.decode()


def _formset(s):
    return sorted(set(s.split(";")))


_ALONE = {}


def _alone(model, seed, n, legacy=False, log_every=1):
    """The stand-alone mode-'dct' fit of clip (seed, n), computed once per module and never changed."""
    key = (seed, n, legacy, log_every)
    if key not in _ALONE:
        bm, vp, scene, vid, D = model
        body, cam, c0, _ = _clip(seed, n)
        _forms(True)
        fop = FittingOP({}, {}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=cam, dct_mtx=D, c_dct_init=c0,
                        dct_num_iter=ITERS, legacy_zero_grad=legacy)
        b, s, c = fop.fitting(torch.tensor(body).cuda(), "dct", log_every=log_every)
        out = (b.cpu().numpy(), float(s), c.cpu().numpy(), fop.c_dct.cpu().numpy(), np.array(fop.log_dct, dtype=np.float64),
               np.array(fop.log2, dtype=np.float64), fop.idx1)
        fop.close()
        _ALONE[key] = (out, _forms(False))
    return _ALONE[key]


def _batch(model, spec, legacy=False, log_every=1, c0=None):
    """spec: ((seed, n), ...) -> each clip's results as _alone gives them, and the forms the batch noted."""
    bm, vp, scene, vid, D = model
    clips = [_clip(s, n) for s, n in spec]
    _forms(True)
    f = ClipBatchFitter({}, {}, body_model=bm, vposer=vp, contact_ids=vid, legacy_zero_grad=legacy, dct_num_iter=ITERS)
    res = f.fit([(c[0], c[1]) for c in clips], scene, log_every=log_every, mode="dct", dct_mtx=D,
                c_dct_init=[c[2] for c in clips] if c0 is None else c0)
    out = [(b.cpu().numpy(), float(s), c.cpu().numpy(), f.c_dct[k].cpu().numpy(), np.array(f.logs_dct[k], dtype=np.float64),
            np.array(f.logs2[k], dtype=np.float64), f.idx1[k]) for k, (b, s, c) in enumerate(res)]
    f.close()
    return out, _forms(False)


def _same(a, b, one_clip=False, logs=True):
    """Bit for bit: body_rec, scale, camera_ext, c_dct, the outlier rows.  The logs: the first phase's rows are sums in double of the
    same per-trajectory floats, the second phase's rec / vposer / smoothing sums add the same per-frame float partials into a double
    with atomics in arrival order, the contact sum is a fixed-order reduction: 1e-12 relative.  The second phase's DCT sum of a batch
    adds one float partial per wavefront and clip where the stand-alone kernel adds one per workgroup: each partial is a float sum of
    at most 256 non-negative terms, relative error <= 255 * 2^-24 = 1.5e-5 on either side, hence 3e-5 on loss_dct and on the total it
    dominates (one clip through the batch path takes the stand-alone launch: 1e-12 there too)."""
    assert a[0].shape == b[0].shape
    assert np.array_equal(a[0], b[0]), np.abs(a[0] - b[0]).max()
    assert np.all(np.isfinite(a[0])) and np.isfinite(a[1])
    assert a[1] == b[1], (a[1], b[1])
    assert np.array_equal(a[2], b[2])
    assert a[3].shape == b[3].shape and np.array_equal(a[3], b[3]), np.abs(a[3] - b[3]).max()
    assert np.array_equal(a[6], b[6])
    if not logs:
        return
    assert a[4].shape == b[4].shape == (P, 2) and a[5].shape == b[5].shape == (N2, 7)
    assert np.all(np.isfinite(a[4])) and np.all(np.isfinite(a[5]))
    assert np.array_equal(a[4][:, 0], b[4][:, 0]) and np.array_equal(a[5][:, 0], b[5][:, 0])
    print("log_dct max relative difference", np.max(np.abs(a[4][:, 1] - b[4][:, 1]) / np.abs(b[4][:, 1])),
          "log2", np.max(np.abs(a[5][:, 1:] - b[5][:, 1:]) / np.maximum(np.abs(b[5][:, 1:]), 1e-300), axis=0))
    np.testing.assert_allclose(a[4][:, 1], b[4][:, 1], rtol=1e-12, atol=0)
    np.testing.assert_allclose(a[5][:, 1:5], b[5][:, 1:5], rtol=1e-12, atol=0)
    np.testing.assert_allclose(a[5][:, 5:], b[5][:, 5:], rtol=1e-12 if one_clip else 3e-5, atol=0)


def test_one_clip_through_the_batch_path_is_the_stand_alone_fit(model):
    """150 frames (30 outside every window): fit([clip], mode='dct') against FittingOP.fitting(body, 'dct'), logged and not."""
    alone, _ = _alone(model, 171, 150)
    (got,), _ = _batch(model, ((171, 150),))
    _same(got, alone, one_clip=True)
    assert int(got[5][0, 0]) == P + 1 and int(got[4][-1, 0]) == P - 1
    (quiet,), _ = _batch(model, ((171, 150),), log_every=0)
    _same(quiet, alone, logs=False)
    assert quiet[4].size == 0 and quiet[5].size == 0
    quiet_alone, _ = _alone(model, 171, 150, log_every=0)
    _same(quiet, quiet_alone, logs=False)


def _scn_equal_lengths(model):
    spec = ((141, 120), (142, 120), (143, 120))
    batch, bforms = _batch(model, spec)
    assert any(len(b[6]) for b in batch), "no clip has outliers"
    for k, (seed, n) in enumerate(spec):
        alone, aforms = _alone(model, seed, n)
        assert _formset(aforms) == _formset(bforms), (aforms, bforms)
        _same(batch[k], alone)
    assert not np.array_equal(batch[0][3], batch[1][3])


def _scn_different_lengths(model, reverse=False):
    spec = ((144, 150), (145, 60), (146, 125), (147, 61))
    if reverse:
        spec = spec[::-1]
    batch, bforms = _batch(model, spec)
    for k, (seed, n) in enumerate(spec):
        alone, aforms = _alone(model, seed, n)
        assert _formset(aforms) == _formset(bforms), (aforms, bforms)
        _same(batch[k], alone)
        assert batch[k][3].shape == (n // 60, 23, 3, 5)


def _scn_different_lengths_reversed(model):
    _scn_different_lengths(model, reverse=True)


def test_clips_of_a_batch_do_not_see_each_other(model):
    A, B, B2, C = (150, 75), (151, 60), (152, 60), (153, 61)
    r1, _ = _batch(model, (A, B, C))
    c0 = [_clip(*A)[2], 2.0 * _clip(*B2)[2], _clip(*C)[2]]
    r2, _ = _batch(model, (A, B2, C), c0=c0)
    for k in (0, 2):
        _same(r1[k], r2[k], logs=False)
        np.testing.assert_allclose(r1[k][4], r2[k][4], rtol=1e-12, atol=0)
        np.testing.assert_allclose(r1[k][5], r2[k][5], rtol=1e-12, atol=0)
    assert not np.array_equal(r1[1][0], r2[1][0]) and not np.array_equal(r1[1][3], r2[1][3])


def test_second_phase_gradient_of_a_ragged_batch_matches_the_fp64_oracle(model):
    """(120, 75, 60), 40 iterations (38 c_dct steps, a no-op, one body / scale step), then iteration 39 again, unstepped (flags bit 0),
    under weights (0.7, 0.5, 0.1) -- large enough for the DCT term to dominate, as test_dct_gradient_matches_autograd -- each clip's
    d loss / d (body_rotation_rec, scale) against fp64 autograd of that clip alone, with that test's bars."""
    bm, vp, scene, vid, D = model
    spec = ((160, 120), (161, 75), (162, 60))
    clips = [_clip(s, n) for s, n in spec]
    lens = [n for _, n in spec]
    K, total = len(lens), sum(lens)
    fit = ClipBatchFitter({}, {}, body_model=bm, vposer=vp, contact_ids=vid, dct_num_iter=40)
    fit.set_scene(scene)
    fit.prepare([(c[0], c[1]) for c in clips], "dct")
    lib, h, st = fit.ctx.lib, fit.ctx.handle, capi.current_stream()
    c0 = torch.cat([torch.tensor(c[2]) for c in clips]).cuda().contiguous()
    assert lib.fdcap_opt_set_dct_clips(h, D.ctypes.data_as(ctypes.c_void_p), 60, 5, capi.dptr(c0), st) == 0
    ws = (ctypes.c_int32 * (K + 1))()
    assert lib.fdcap_opt_dct_clip_windows(h, ws, K + 1) == 0 and list(ws) == [0, 2, 3, 4]
    assert lib.fdcap_opt_dct_clip_windows(h, ws, K) == E_ARG
    assert lib.fdcap_opt_dct_windows(h, None, None) == 4
    n_log = ctypes.c_int32(0)
    assert lib.fdcap_opt_run_dct(h, 0, 40, 40, 10.0, 1e-4, 0.5, 0.1, 0, None, None, 0, 0, ctypes.byref(n_log), st) == 0
    x_before, s_before = fit._rows_x.clone(), fit._scale.clone()
    hist = torch.zeros(1, K, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
    # (other rec / contact multipliers than the records were built under: refused, never replaced)
    assert lib.fdcap_opt_run_dct(h, 39, 40, 40, 10.0, 0.7, 0.6, 0.1, 1, None, capi.dptr(hist), 1, 1, ctypes.byref(n_log), st) == E_STATE
    assert lib.fdcap_opt_run_dct(h, 39, 40, 40, 10.0, 0.7, 0.5, 0.1, 1, None, capi.dptr(hist), 1, 1, ctypes.byref(n_log), st) == 0
    assert n_log.value == 1
    dx = torch.empty(total, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, st), "get_grads")
    assert torch.equal(x_before, fit._rows_x) and torch.equal(s_before, fit._scale)      # (flags bit 0: nothing was stepped)
    cd = torch.empty(4, 23, 3, 5, device="cuda")
    capi.check(lib.fdcap_opt_get_dct(h, capi.dptr(cd), st), "get_dct")
    dx, dscale, cd, sums = dx.cpu().numpy(), fit._dscale.cpu().numpy(), cd.cpu().numpy(), hist.cpu().numpy()[0]
    rows, scales = fit._rows_x.cpu().double(), fit._scale.cpu().double()
    starts = fit.clip_starts
    dt = torch.float64
    for k, n in enumerate(lens):
        body_in = torch.tensor(clips[k][0]).cuda()
        x78_gpu = torch.empty(n, 78, device="cuda")
        capi.check(lib.fdcap_params_75_to_78(capi.dptr(body_in), n, capi.dptr(x78_gpu), st), "75_to_78")
        orc = FittingOracle(SMPLXOracle(bm, dtype=dt), VPoserDecoder.from_data(vp, dtype=dt), scene, vid, clips[k][3], n, dtype=dt,
                            dct_mtx=D, c_dct_init=cd[ws[k]:ws[k + 1]])
        x78 = x78_gpu.cpu().double()
        idx1 = orc.init(x78)
        orc.body_rotation_rec.data = rows[2 + starts[k]:2 + starts[k + 1]].clone()
        orc.scale.data = scales[k].reshape(())
        l_rec, l_vp, l_con, l_sm, l_ws = orc.cal_loss(x78.detach(), idx1)
        _, _, joints = orc.forward_world()
        l_dct = orc.cal_dctloss(joints)
        (0.7 * l_dct + 0.5 * l_rec + 0.1 * l_con).backward()
        g = orc.body_rotation_rec.grad.numpy()
        mine = dx[starts[k]:starts[k + 1]]
        print("clip", k, "max |g - gx|", np.abs(mine - g).max(), "max |gx|", np.abs(g).max(), "dscale", dscale[k], float(orc.scale.grad))
        np.testing.assert_allclose(mine, g, rtol=2e-3, atol=2e-4 * np.abs(g).max())
        np.testing.assert_allclose(dscale[k], float(orc.scale.grad), rtol=2e-3)
        np.testing.assert_allclose(sums[k, 7] / (69 * (n // 60)), float(l_dct.detach()), rtol=1e-5)
    fit.close()


def test_the_references_own_dct_run_as_a_batch_of_two_copies(golden_dir):
    """tests/golden/ref_dct_10000it.npz fitted as a batch of two copies of its clip: the two clips' results are bit-identical, and each
    meets the bars test_gpu_dct_smoother.py::test_dct_mode_matches_reference_golden applies to the stand-alone fit."""
    g = np.load(os.path.join(golden_dir, "ref_dct_10000it.npz"))
    bm = synth.make_body_model(int(g["num_verts"]), seed=int(g["model_seed"]))
    vp = synth.make_vposer(seed=int(g["vposer_seed"]))
    cam0 = read_camerapose(list(g["camerapose"]))
    f = ClipBatchFitter({}, {}, body_model=bm, vposer=vp, contact_ids=g["vid"])
    res = f.fit([(g["body_in"], cam0), (g["body_in"], cam0)], g["scene"], log_every=1, mode="dct", dct_mtx=g["dct_mtx"],
                c_dct_init=[g["c_dct0"], g["c_dct0"]])
    out = [(b.cpu().numpy(), float(s), c.cpu().numpy(), f.c_dct[k].cpu().numpy(), np.array(f.logs_dct[k]), np.array(f.logs2[k]), f.idx1[k])
           for k, (b, s, c) in enumerate(res)]
    f.close()
    a, b = out
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.array_equal(a[4], b[4])
    logd = g["logd"]
    ref1, ref2 = logd[logd[:, 0] < 9400], logd[logd[:, 0] >= 9501]
    for body, scale, cam, c_dct, log_dct, log2, idx1 in out:
        np.testing.assert_array_equal(idx1, g["idx1"])
        dc = np.abs(c_dct - g["c_dct"])
        assert np.quantile(dc, 0.9) < 1e-5 and dc.max() < 3e-3
        sel = np.isin(log_dct[:, 0], ref1[:, 0])
        np.testing.assert_allclose(log_dct[sel, 1], ref1[:, 5], rtol=0, atol=8e-6)
        assert log2.shape[0] == ref2.shape[0] == 499 and int(log2[0, 0]) == 9501
        np.testing.assert_allclose(log2[:4, 1:], ref2[:4, 1:], rtol=0, atol=5e-6)
        err = np.abs(body - g["body_rec"])
        q50, q90, q99 = np.quantile(err, [0.5, 0.9, 0.99])
        print("dct golden as a batch: max", err.max(), "q50/q90/q99", q50, q90, q99, "scale", scale, float(g["scale"]))
        assert q50 < 1e-3 and q90 < 5e-3 and q99 < 1e-2 and err.max() <= 2 * 0.005 * 499
        np.testing.assert_allclose(scale, float(g["scale"]), atol=2e-3)
        np.testing.assert_array_equal(cam.reshape(-1, 16), np.asarray(cam0, np.float32).reshape(-1, 16))


def _scn_legacy_zero_grad(model):
    spec = ((148, 120), (149, 75))
    batch, bforms = _batch(model, spec, legacy=True)
    for k, (seed, n) in enumerate(spec):
        alone, aforms = _alone(model, seed, n, legacy=True)
        assert _formset(aforms) == _formset(bforms), (aforms, bforms)
        _same(batch[k], alone)
        plain, _ = _alone(model, seed, n)
        assert np.abs(alone[3] - plain[3]).max() > 1e-3        # (the coasting steps really moved the coefficients)


def test_the_new_calls_refuse_what_they_do_not_do_and_a_cut_stretch_gives_the_one_call_bits(model):
    bm, vp, scene, vid, D = model
    Dp = D.ctypes.data_as(ctypes.c_void_p)
    f = ClipBatchFitter({}, {}, body_model=bm, vposer=vp, contact_ids=vid, dct_num_iter=ITERS)
    lib, h, st = f.ctx.lib, f.ctx.handle, capi.current_stream()
    n = ctypes.c_int32(7)
    hist = torch.zeros(N2, 2, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
    hp = capi.dptr(hist)

    def run(ii0=0, ii1=ITERS, log_every=0, hist_d=None, rows=0, flags=0, obj=None):
        return lib.fdcap_opt_run_dct(h, ii0, ii1, ITERS, 10.0, 1e-4, 0.5, 0.1, log_every, obj, hist_d, rows, flags, ctypes.byref(n), st)

    coef = torch.zeros(8 * 69 * 5, device="cuda")
    assert run() == E_STATE and n.value == 0                     # no optimiser
    assert lib.fdcap_opt_set_dct_clips(h, Dp, 60, 5, capi.dptr(coef), st) == E_STATE
    with pytest.raises(ValueError, match="'global' or 'local'"):
        f.fit([_clip(180, 59)[:2], _clip(181, 120)[:2]], scene, mode="dct")
    f.set_scene(scene)
    spec = ((182, 120), (183, 75))
    clips = [_clip(*s) for s in spec]
    f.prepare([(c[0], c[1]) for c in clips], "dct")
    assert run() == E_STATE                                      # fdcap_opt_run_dct before fdcap_opt_set_dct_clips
    assert lib.fdcap_opt_get_dct(h, capi.dptr(coef), st) == E_STATE and lib.fdcap_opt_dct_windows(h, None, None) == 0
    assert lib.fdcap_opt_set_dct_clips(h, Dp, 60, 9, capi.dptr(coef), st) == E_ARG
    c0 = torch.cat([torch.tensor(c[2]) for c in clips]).cuda().contiguous()
    assert lib.fdcap_opt_set_dct_clips(h, Dp, 60, 5, capi.dptr(c0), st) == 0
    assert run(ii0=-1) == E_ARG and run(ii0=3, ii1=2) == E_ARG and run(ii1=ITERS + 1) == E_ARG and run(log_every=-1) == E_ARG
    assert run(log_every=1) == E_ARG                             # logging iterations and no history
    assert run(log_every=1, hist_d=hp, rows=N2 - 1) == E_ARG     # ... a history one row short
    assert run(ii0=0, ii1=P + 1, log_every=1) == 0 and n.value == 0          # (a stretch without second-phase logging needs none)
    # the old single steps still refuse a batch
    assert lib.fdcap_opt_set_dct(h, Dp, 60, 5, capi.dptr(c0), st) == E_STATE
    assert lib.fdcap_opt_dct_fit(h, 1, 0, 10.0, None, 1, st) == E_STATE
    assert lib.fdcap_opt_backward_dct(h, 1e-4, 0.5, 0.1, 0, st) == E_STATE
    torch.cuda.synchronize()

    # a stretch cut inside the first phase, at the no-op iteration and inside the second phase, against one call
    def fit(cuts):
        f.prepare([(c[0], c[1]) for c in clips], "dct")
        assert lib.fdcap_opt_set_dct_clips(h, Dp, 60, 5, capi.dptr(c0), st) == 0
        hist.zero_()
        k = 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert lib.fdcap_opt_run_dct(h, a, b, ITERS, 10.0, 1e-4, 0.5, 0.1, 1, None, capi.dptr(hist[k:]), N2 - k, 0, ctypes.byref(n), st) == 0
            k += n.value
        assert k == N2
        body, sc, cd = torch.empty(195, 75, device="cuda"), torch.empty(2, device="cuda"), torch.empty(3 * 69 * 5, device="cuda")
        capi.check(lib.fdcap_opt_get_results(h, capi.dptr(body), capi.dptr(sc), None, st), "results")
        capi.check(lib.fdcap_opt_get_dct(h, capi.dptr(cd), st), "get_dct")
        return body.cpu().numpy(), sc.cpu().numpy(), cd.cpu().numpy(), hist.cpu().numpy().copy()

    one = fit((0, ITERS))
    cut = fit((0, 77, P, P + 1, 194, 197, ITERS))
    for a, b in zip(one[:3], cut[:3]):
        assert np.array_equal(a, b)
    np.testing.assert_allclose(cut[3], one[3], rtol=1e-12, atol=0)
    f._destroy_opt()
    # one clip's optimiser: a shard of a clip is refused; a clip below T frames has no window
    t = [torch.zeros(124, 78, device="cuda") for _ in range(2)] + [torch.zeros(8, device="cuda") for _ in range(2)]
    losses = torch.zeros(capi.NUM_LOSSES, device="cuda", dtype=torch.float64)

    def create(n_total, n_local, frame0):
        oc = capi.OptConfig(n_total, n_local, frame0, 0.005, 1.0, 0.001, 0.1, 0.1, 1.0, 1.0, 0.5, 1.8, 0)
        return lib.fdcap_opt_create(h, ctypes.byref(oc), *[capi.dptr(x) for x in t], capi.dptr(losses))

    assert create(120, 60, 60) == 0
    assert lib.fdcap_opt_set_dct_clips(h, Dp, 60, 5, capi.dptr(c0), st) == E_STATE
    assert lib.fdcap_opt_set_dct(h, Dp, 60, 5, capi.dptr(c0), st) == 0       # (FittingOP's sharded path keeps working)
    assert run() == E_STATE
    assert create(59, 59, 0) == 0
    assert lib.fdcap_opt_set_dct_clips(h, Dp, 60, 5, capi.dptr(c0), st) == E_ARG
    lens = (ctypes.c_int32 * 2)(61, 59)
    oc = capi.OptConfig(120, 120, 0, 0.005, 1.0, 0.001, 0.1, 0.1, 1.0, 1.0, 0.5, 1.8, 0)
    losses2 = torch.zeros(2, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
    assert lib.fdcap_opt_create_clips_var(h, ctypes.byref(oc), 2, lens, *[capi.dptr(x) for x in t], capi.dptr(losses2)) == 0
    assert lib.fdcap_opt_set_dct_clips(h, Dp, 60, 5, capi.dptr(c0), st) == E_ARG
    torch.cuda.synchronize()
    lib.fdcap_opt_destroy(h)
    f.close()


# ---- the comparisons that need pinned kernel forms: one child process for all of them --------------------------------------------
_SCENARIOS = {"equal_lengths": _scn_equal_lengths, "different_lengths": _scn_different_lengths,
              "different_lengths_reversed": _scn_different_lengths_reversed, "legacy_zero_grad": _scn_legacy_zero_grad}


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ)
    env["FDCAP_CLIP_FORMS_MIN_ROWS"] = "32"
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and line, (p.stdout[-1500:], p.stderr[-3000:])
    print(p.stdout[-3000:])
    return json.loads(line[-1][7:])


def test_equal_lengths_give_each_clip_its_stand_alone_bits(child):
    """3 x 120 frames."""
    assert child["equal_lengths"] == "ok", child["equal_lengths"]


@pytest.mark.parametrize("name", ["different_lengths", "different_lengths_reversed"])
def test_different_lengths_with_tails_give_each_clip_its_stand_alone_bits(child, name):
    """(150, 60, 125, 61) and the reverse: 30, 0, 5 and 1 frames outside every window; the window of the second clip starts at buffer
    row 152, not 122, and the workgroups of the DCT gradient straddle every clip boundary (a row is 69 threads of 256)."""
    assert child[name] == "ok", child[name]


def test_legacy_zero_grad_lets_every_clips_c_dct_coast(child):
    """(120, 75) against the stand-alone legacy fits, the coasting c_dct included."""
    assert child["legacy_zero_grad"] == "ok", child["legacy_zero_grad"]


if __name__ == "__main__":
    assert capi.load_library().fdcap_set_nn_kernel(2) == 0
    m, result = _model(), {}
    for name, fn in _SCENARIOS.items():
        try:
            fn(m)
            result[name] = "ok"
        except Exception:
            result[name] = traceback.format_exc()[-2500:]
    print("RESULT " + json.dumps(result))
