"""Mode 'local' for a batch of clips (fdcap_opt_run_local2, ClipBatchFitter.fit(mode='local')) against the stand-alone mode-'local'
fits of its clips (FittingOP): the same bits wherever both select the same kernel forms -- one clip, equal lengths, ragged lengths,
clips of three, two and one frames -- nothing leaks across clip boundaries, the second loop's logged sums and its gradient against
the fp64 oracle with each clip's own denominators, the reference's own 'local' run as a batch, and the refusals.
Shapes as tests/test_gpu_multiclip.py: a 300-vertex body, a 9000-point scene, 2 x 24 contact vertices (n_left = 24), 10 iterations
(the first loop crosses its phase switch at 8, the second loop has int(0.4 * 10) = 4 iterations), every iteration logged, two
outlier rows per clip.  tests/test_local2_clips_cpu.py evaluates the plans of the lengths used here."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.fitting import LOCAL_SECOND_LOOP, ClipBatchFitter, FittingOP, find_outliers, first_phase2_iter
from fdcap_amd.io import read_camerapose
from oracle import rotrepr
from oracle.fitting import FittingOracle
from oracle.smplx import SMPLXOracle
from oracle.vposer import VPoserDecoder

pytestmark = pytest.mark.gpu
ITERS = 10
N2 = int(LOCAL_SECOND_LOOP * ITERS)
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


def _formset(s):
    return sorted(set(s.split(";")))


_ALONE = {}


def _alone(model, seed, n):
    """The stand-alone mode-'local' fit of clip (seed, n), computed once per module and never changed."""
    if (seed, n) not in _ALONE:
        bm, vp, scene, vid = model
        clip = _clip(seed, n)
        _forms(True)
        fop = FittingOP({"num_iter": ITERS}, {}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=clip[1])
        with np.errstate(divide="ignore", invalid="ignore"):       # (a clip of two frames prints a mean over nothing)
            body, scale, cam = fop.fitting(torch.tensor(clip[0]).cuda(), "local", log_every=1)
        out = (body.cpu().numpy(), float(scale), cam.cpu().numpy(), fop.log, fop.idx1, fop.contact_weight.cpu().numpy(),
               np.array(fop.log2, dtype=np.float64))
        fop.close()
        _ALONE[(seed, n)] = (out, _forms(False), clip[1])
    return _ALONE[(seed, n)]


def _batch(model, spec):
    """spec: ((seed, n), ...) -> each clip's results as _alone gives them, and the forms the batch noted."""
    bm, vp, scene, vid = model
    clips = [_clip(s, n) for s, n in spec]
    _forms(True)
    f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    res = f.fit(clips, scene, log_every=1, mode="local")
    out = [(b.cpu().numpy(), float(s), c.cpu().numpy(), f.logs[k], f.idx1[k], f.contact_weights[k].cpu().numpy(),
            np.array(f.logs2[k], dtype=np.float64)) for k, (b, s, c) in enumerate(res)]
    f.close()
    return out, _forms(False)


def _same(a, b, nan_terms=(), nan_log2=False):
    """Bit for bit: body_rec, scale, camera_ext, the contact weights, the first loop's log.  The second loop's printed terms to
    1e-12 relative: both sides add per-workgroup float partials into a double with atomics in arrival order -- at most a few hundred
    partials at <= 2^-53 relative error each.  nan_terms / nan_log2: means over nothing, NaN on both sides in the same places."""
    assert a[0].shape == b[0].shape
    assert np.array_equal(a[0], b[0]), np.abs(a[0] - b[0]).max()
    assert np.all(np.isfinite(a[0])) and np.isfinite(a[1])
    assert a[1] == b[1], (a[1], b[1])
    assert np.array_equal(a[2], b[2]), np.abs(a[2] - b[2]).max()
    for k in LOG_FIELDS:
        x, y = np.array(getattr(a[3], k), dtype=np.float64), np.array(getattr(b[3], k), dtype=np.float64)
        assert np.array_equal(x, y, equal_nan=k in nan_terms), k
        assert np.all(np.isfinite(x)) or k in nan_terms, k
    assert np.array_equal(a[4], b[4])
    assert np.array_equal(a[5], b[5]) and a[5].shape == (a[0].shape[0],)
    assert a[6].shape == b[6].shape == (N2, 6)
    assert np.array_equal(np.isnan(a[6]), np.isnan(b[6]))
    assert nan_log2 or np.all(np.isfinite(a[6]))
    ok = ~np.isnan(a[6])
    print("log2 max relative difference", np.max(np.abs(a[6][ok] - b[6][ok]) / np.maximum(np.abs(b[6][ok]), 1e-300)))
    np.testing.assert_allclose(a[6][ok], b[6][ok], rtol=1e-12, atol=0)


def test_one_clip_through_the_new_call_is_the_python_second_loop(model):
    """fdcap_opt_run_local2 on a plain fdcap_opt_create optimiser, after fdcap_opt_run with the 'local' config, against
    FittingOP.fitting(body, 'local', log_every=1): 24 frames."""
    bm, vp, scene, vid = model
    n = 24
    ref, _, cam_in = _alone(model, 71, n)
    clip = _clip(71, n)
    fop = FittingOP({"num_iter": ITERS}, {}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=clip[1])
    lib, h, st = fop.ctx.lib, fop.ctx.handle, capi.current_stream()
    x78 = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(clip[0]).cuda()), n, capi.dptr(x78), st), "p78")
    fop._mode = "local"
    fop.init(x78)                                                # (fdcap_opt_create under the 'local' config)
    P = first_phase2_iter(ITERS)
    hist = torch.zeros(ITERS, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
    hist2 = torch.zeros(N2, 1, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
    w = torch.full((n,), -1.0, device="cuda")
    k = ctypes.c_int32(0)
    capi.check(lib.fdcap_opt_run(h, 0, ITERS, ITERS, P, 1, capi.dptr(hist), ITERS, 0, ctypes.byref(k), st), "run")
    assert k.value == ITERS
    capi.check(lib.fdcap_opt_run_local2(h, 24, 0, N2, ITERS, 1, capi.dptr(w), capi.dptr(hist2), N2, 0, ctypes.byref(k), st), "run_local2")
    assert k.value == N2
    body, sc, cam = torch.empty(n, 75, device="cuda"), torch.empty(1, device="cuda"), torch.empty(n, 16, device="cuda")
    capi.check(lib.fdcap_opt_get_results(h, capi.dptr(body), capi.dptr(sc), capi.dptr(cam), st), "results")
    assert np.array_equal(body.cpu().numpy(), ref[0])
    assert float(sc.item()) == ref[1]
    assert np.array_equal(cam.cpu().numpy().reshape(n, 4, 4), ref[2]) and np.array_equal(ref[2], cam_in)
    assert np.array_equal(w.cpu().numpy(), ref[5])
    # the sums of the logging iterations, against the stand-alone log's terms (same denominators: one clip)
    s = hist2.cpu().numpy()[:, 0]
    got = np.stack([s[:, 0] / (n * 78), s[:, 2] / ((n - 2) * 78), s[:, 5] / ((n - 2) * 900), s[:, 6]], axis=1)
    np.testing.assert_allclose(got, ref[6][:, 1:5], rtol=1e-12, atol=0)
    # (the registered output is registered again: the next plain backward writes there, not into the history)
    before = hist2.clone()
    capi.check(lib.fdcap_opt_backward_local2(h, capi.dptr(w), 24, st), "local2")
    assert torch.equal(before, hist2) and float(fop._losses[5].item()) > 0.0
    fop.close()


def test_equal_lengths_give_each_clip_its_stand_alone_bits(model):
    spec = ((41, 24), (42, 24), (43, 24))
    batch, bforms = _batch(model, spec)
    assert any(len(b[4]) for b in batch), "no clip has outliers"
    for name in ("skin_fwd_kernel", "panel_gemm3_kernel", "panel_gemm3_ksw_kernel", "skin_bwd_kernel(one workgroup per frame)"):
        assert name in bforms, bforms                            # (the full-mesh launches are among the noted forms)
    for k, (seed, n) in enumerate(spec):
        alone, aforms, cam_in = _alone(model, seed, n)
        assert _formset(aforms) == _formset(bforms), (aforms, bforms)
        _same(batch[k], alone)
        assert np.array_equal(batch[k][2], cam_in)               # camera_ext is never stepped in this mode


def test_ragged_lengths_give_each_clip_its_stand_alone_bits(model):
    spec = ((44, 40), (45, 33), (46, 24), (47, 10))
    batch, bforms = _batch(model, spec)
    assert any(len(b[4]) for b in batch), "no clip has outliers"
    for k, (seed, n) in enumerate(spec):
        alone, aforms, cam_in = _alone(model, seed, n)
        assert _formset(aforms) == _formset(bforms), (aforms, bforms)
        _same(batch[k], alone)
        assert np.array_equal(batch[k][2], cam_in)


def test_a_three_frame_clip_fits_at_either_end_of_a_batch(model):
    """3 frames: exactly one second difference (parameter and vertex space), two foot-skate pairs.  Its bits do not depend on which
    end of the batch it sits at, nor do its 40-frame neighbour's; every printed term is finite, the vertex smoothing not zero."""
    r1, _ = _batch(model, ((48, 3), (49, 40)))
    r2, _ = _batch(model, ((49, 40), (48, 3)))
    _same(r1[0], r2[1])
    _same(r1[1], r2[0])
    assert np.all(r1[0][6][:, 1:] > 0.0)


def test_clips_of_one_two_and_three_frames_give_their_stand_alone_bits(model):
    """Lengths (1, 2, 3, 3): nine rows plan as each clip's own rows do (tests/test_local2_clips_cpu.py).  The second differences of
    the 1- and 2-frame clips are means over nothing: NaN in the batch's logs and the stand-alone fit's alike (the 2-frame clip's two
    smoothing terms, with them its total); zero weights below three and below two frames; every parameter finite."""
    spec = ((57, 1), (58, 2), (59, 3), (60, 3))
    batch, bforms = _batch(model, spec)
    nan_terms = {1: ("loss_smoothing", "loss_world_smoothing", "total"), 2: ("loss_smoothing", "total"), 3: ()}
    for k, (seed, n) in enumerate(spec):
        alone, aforms, _ = _alone(model, seed, n)
        assert _formset(aforms) == _formset(bforms), (aforms, bforms)
        _same(batch[k], alone, nan_terms[n], nan_log2=n < 3)
    assert np.all(np.isnan(batch[1][6][:, [2, 3, 5]])) and np.all(np.isfinite(batch[1][6][:, [1, 4]]))
    assert np.all(np.isfinite(batch[2][6])) and np.all(batch[2][6][:, 3] > 0.0)


def test_clips_of_a_batch_do_not_see_each_other_and_offsets_do_not_matter(model):
    A, B, B2, C = (50, 40), (51, 33), (52, 20), (53, 24)
    r1, _ = _batch(model, (A, B, C))
    r2, _ = _batch(model, (A, B2, C))
    _same(r1[0], r2[0])
    _same(r1[2], r2[2])                                         # (C starts at row 2 + 73 in one batch, 2 + 60 in the other)
    assert r1[1][0].shape != r2[1][0].shape and r1[1][1] != r2[1][1]


def test_second_loop_gradient_of_a_ragged_batch_matches_the_fp64_oracle(model):
    """Lengths (10, 7, 3), parameters perturbed by 0.01 randn, the caller's own weights through jj0 = 1, jj1 = 2, flags = 1: two
    frames per clip at 0.8 and 0.3 (the thresholding of :421-422 on both sides of 0.5), a clip's first and a clip's last frame among
    them (pair (i, i + 1) uses w[i + 1] of the SAME clip).  Each clip's gradient against cal_loss2 of that clip alone; the bars are
    those of test_gpu_parity.py::test_local_mode_second_loop_gradient_matches_autograd (the same arithmetic).
    The tight check of a batch's gradient, per clip and column block, is tests/test_gpu_local2_bars.py."""
    bm, vp, scene, vid = model
    lens = (10, 7, 3)
    clips_d = [synth.make_clip(n, seed=90 + k, num_outliers=2) for k, n in enumerate(lens)]
    clips = [(c.body_params, read_camerapose(c.camerapose_lines)) for c in clips_d]
    set_w = {0: ((0, 0.8), (6, 0.3)), 1: ((3, 0.8), (6, 0.3)), 2: ((0, 0.3), (2, 0.8))}      # frame 0 of clips 0 and 2, the last of 1 and 2
    dt = torch.float64
    n_left = len(vid) // 2
    want, perts, ws = [], [], []
    for k, n in enumerate(lens):
        f = FittingOracle(SMPLXOracle(bm, dt), VPoserDecoder.from_data(vp, dt), scene, vid, clips_d[k].camerapose_lines, n, dtype=dt)
        x78 = rotrepr.convert_to_6D_rot(torch.tensor(clips_d[k].body_params, dtype=dt)).detach()
        f.init(x78)
        pert = 0.01 * torch.randn(f.body_rotation_rec.shape, generator=torch.Generator().manual_seed(6 + k), dtype=dt)
        f.body_rotation_rec.data += pert
        idx1, _ = find_outliers(x78.numpy().astype(np.float32))
        w = torch.full((n,), 0.5, dtype=dt)
        for i, v in set_w[k]:
            w[i] = v
        l_rec, l_loc, l_sm, l_cs = f.cal_loss2(x78, idx1, w, n_left)
        (l_sm + l_loc + l_rec + l_cs).backward()
        want.append((f.body_rotation_rec.grad.numpy(), float(l_loc.detach()), float(l_sm.detach()), float(l_cs.detach())))
        perts.append(pert)
        ws.append(w)
    fit = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    fit.set_scene(scene)
    fit.prepare(clips, "local")
    total = sum(lens)
    fit._rows_x[2:2 + total] += torch.cat(perts).float().cuda()
    w_d = torch.cat(ws).float().cuda().contiguous()
    lib, h, st = fit.ctx.lib, fit.ctx.handle, capi.current_stream()
    hist = torch.zeros(1, len(lens), capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
    k_log = ctypes.c_int32(0)
    x_before = fit._rows_x.clone()
    capi.check(lib.fdcap_opt_run_local2(h, n_left, 1, 2, ITERS, 1, capi.dptr(w_d), capi.dptr(hist), 1, 1, ctypes.byref(k_log), st), "run_local2")
    assert k_log.value == 1
    dx = torch.empty(total, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, st), "grads")
    assert torch.equal(x_before, fit._rows_x)                    # (flags bit 0: the stretch's last iteration is not stepped)
    assert torch.equal(w_d, torch.cat(ws).float().cuda())        # (jj0 > 0: the weights are an input)
    dx, s = dx.cpu().numpy(), hist.cpu().numpy()[0]
    fit.close()
    for k, n in enumerate(lens):
        gx, l_loc, l_sm, l_cs = want[k]
        g = dx[fit.clip_starts[k]:fit.clip_starts[k + 1]]
        print("clip", k, "max |g - gx|", np.abs(g - gx).max(), "max |gx|", np.abs(gx).max())
        np.testing.assert_allclose(g, gx, rtol=3e-3, atol=3e-4 * np.abs(gx).max())
        np.testing.assert_allclose(s[k, 5] / ((n - 2) * 3 * 300), l_sm, rtol=1e-5)
        np.testing.assert_allclose(s[k, 6], l_cs, rtol=1e-5)
        np.testing.assert_allclose(s[k, 2] / ((n - 2) * 78), l_loc, rtol=1e-5)


def test_the_references_own_local_run_as_a_batch_of_two_copies(golden_dir):
    """tests/golden/ref_local_10it.npz fitted as a batch of two copies of its clip: the two clips' results are bit-identical, and
    each meets the bars test_gpu_parity.py::test_local_mode_matches_reference_golden applies to the stand-alone fit."""
    g = np.load(os.path.join(golden_dir, "ref_local_10it.npz"))
    bm = synth.make_body_model(int(g["num_verts"]), seed=int(g["model_seed"]))
    vp = synth.make_vposer(seed=int(g["vposer_seed"]))
    num_iter = int(g["num_iter"])
    cam0 = read_camerapose(list(g["camerapose"]))
    f = ClipBatchFitter({"num_iter": num_iter}, {}, body_model=bm, vposer=vp, contact_ids=g["vid"], n_left=int(g["n_left"]))
    res = f.fit([(g["body_in"], cam0), (g["body_in"], cam0)], g["scene"], log_every=1, mode="local")
    out = [(b.cpu().numpy(), float(s), c.cpu().numpy(), f.contact_weights[k].cpu().numpy(), np.array(f.logs2[k]))
           for k, (b, s, c) in enumerate(res)]
    f.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and np.array_equal(out[0][2], out[1][2])
    assert np.array_equal(out[0][3], out[1][3])
    ref2 = g["log2"]
    tol = 3e-6 + 2e-6 * (num_iter + np.arange(len(ref2)))
    for body, scale, cam, w, log2 in out:
        assert bool((w == 0.5).all())
        err = np.abs(body - g["body_rec"])
        q50, q90, q99 = np.quantile(err, [0.5, 0.9, 0.99])
        assert err.max() <= 2 * 0.005 * 14 and q50 < 1e-6 and q90 < 1e-4 and q99 < 3e-3, (q50, q90, q99, err.max())
        np.testing.assert_allclose(scale, float(g["scale"]), atol=1e-4)
        np.testing.assert_array_equal(cam, cam0)                 # camera_ext is never stepped in this mode
        for k in range(1, 6):
            assert np.all(np.abs(log2[:, k] - ref2[:, k]) <= 2 * tol), (k, np.abs(log2[:, k] - ref2[:, k]).max())


def test_the_new_call_and_the_fitter_refuse_what_they_do_not_do(model):
    bm, vp, scene, vid = model
    f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    lib, h, st = f.ctx.lib, f.ctx.handle, capi.current_stream()
    n = ctypes.c_int32(7)
    w = torch.full((64,), 0.5, device="cuda")
    hist = torch.zeros(4, 2, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
    wp, hp = capi.dptr(w), capi.dptr(hist)

    def run(n_left=24, jj0=1, jj1=2, log_every=0, weight=wp, hist_d=None, rows=0, flags=1):
        return lib.fdcap_opt_run_local2(h, n_left, jj0, jj1, ITERS, log_every, weight, hist_d, rows, flags, ctypes.byref(n), st)

    assert run() == E_STATE and n.value == 0                     # no optimiser
    with pytest.raises(ValueError, match="'global' or 'local'"):
        f.fit([_clip(80, 24), _clip(81, 24)], scene, mode="dct")
    f.set_scene(scene)
    f.prepare([_clip(80, 24), _clip(81, 24)], "local")
    assert run(n_left=0) == E_ARG and run(n_left=-1) == E_ARG and run(n_left=48) == E_ARG
    assert run(jj0=-1) == E_ARG and run(jj0=3, jj1=2) == E_ARG
    assert run(weight=None) == E_ARG
    assert run(log_every=1) == E_ARG                             # a logging iteration and no history
    assert run(jj0=1, jj1=3, log_every=1, hist_d=hp, rows=1) == E_ARG      # ... a history one row short
    x = f._rows_x.clone()
    assert run(jj0=1, jj1=3, log_every=1, hist_d=hp, rows=2) == 0 and n.value == 2
    assert not torch.equal(x, f._rows_x)                         # (the stretch's first iteration was stepped)
    # the three single steps still refuse a batch
    assert lib.fdcap_opt_detect_contact(h, 24, wp, st) == E_STATE
    assert lib.fdcap_opt_backward_local2(h, wp, 24, st) == E_STATE
    assert lib.fdcap_opt_step_x(h, 1, st) == E_STATE
    torch.cuda.synchronize()
    f._destroy_opt()
    # one clip's optimiser: a shard of a clip (frame0 > 0), a DCT term, no contact set
    t = [torch.zeros(44, 78, device="cuda") for _ in range(2)] + [torch.zeros(8, device="cuda") for _ in range(2)]
    losses = torch.zeros(capi.NUM_LOSSES, device="cuda", dtype=torch.float64)

    def create(n_total, n_local, frame0, weight_contact=0.1):
        oc = capi.OptConfig(n_total, n_local, frame0, 0.005, 1.0, 0.001, weight_contact, 0.2, 1.0, 0.0, 0.5, 1.8, 0)
        return lib.fdcap_opt_create(h, ctypes.byref(oc), *[capi.dptr(x) for x in t], capi.dptr(losses))

    assert create(40, 20, 20) == 0
    assert run() == E_STATE
    assert create(40, 40, 0) == 0
    dct = np.ones((20, 2), np.float32)
    coef = torch.zeros(2 * 69 * 2, device="cuda")
    assert lib.fdcap_opt_set_dct(h, dct.ctypes.data_as(ctypes.c_void_p), 20, 2, capi.dptr(coef), st) == 0
    assert run() == E_STATE
    assert create(40, 40, 0, weight_contact=0.0) == 0
    assert run() == E_STATE
    torch.cuda.synchronize()
    lib.fdcap_opt_destroy(h)
    f.close()
