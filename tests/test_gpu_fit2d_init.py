"""GPU tests of the inner fit's start from keypoints alone (csrc/fdc_fit2d_init.h through the C-ABI, innerfit.InnerFitOP(init=...),
innerfit_hip.py) against the torch twin tests/fit2d_init_spec.py, which evaluates the camera objective through the full model and
never through the kernels' closed form.  Value and gradient bars are tests/gradient_bars.py's formula,
32 max(max|s32 - s64|, 2^-24 max|s64|), from the twin's two precisions at the fp32 state the GPU holds."""
import ctypes
import json

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, cli_innerfit, synth
from fdcap_amd import io as fio
from fdcap_amd.innerfit import DEFAULT_LBFGS, DEFAULT_STAGES, OPENPOSE_BODY25, InnerFitOP, KeypointMap
from oracle import rotrepr
from tests import fit2d_init_spec as fs
from tests.gradient_bars import EPS32, M

pytestmark = pytest.mark.gpu
TORSO8 = (fs.L_SHOULDER, fs.R_SHOULDER, fs.L_HIP, fs.R_HIP, 12, 0, 4, 5)


def _struct(s):
    """capi.Fit2dInit of settings in slots"""
    ci = capi.Fit2dInit()
    ci.n_edge, ci.n_torso = len(s["edges"]), len(s["torso"])
    for e, (a, b) in enumerate(s["edges"]):
        ci.edge[e][0], ci.edge[e][1] = a, b
    for k, v in enumerate(s["torso"]):
        ci.torso[k] = v
    ci.shoulder[0], ci.shoulder[1] = s["shoulders"]
    ci.conf_thr, ci.default_depth, ci.side_view_px, ci.w_data, ci.w_depth = s["conf_thr"], s["default_depth"], s["side_view_px"], s["w_data"], s["w_depth"]
    return ci


def _stage():
    return capi.Fit2dStage(*fs.INTRINSICS, 100.0, 1.0, 0.0, 0.0, 0.0)


def _rows75(x78):
    return rotrepr.convert_to_3D_rot(torch.tensor(np.asarray(x78), dtype=torch.float64)).numpy().astype(np.float32)


def _op(case, n, **kw):
    km = None if case["map"] is None else KeypointMap(*case["map"])
    return InnerFitOP(case["bm"], case["vp"], n, intrinsics=fs.INTRINSICS, keypoint_map=km, **{"iters_per_stage": 0, **kw})


def _load(case, n, x78, **kw):
    """an optimiser state of n problems at these rows (rounded through the 75-wide layout) -> op, the fp32 rows the GPU holds"""
    op = _op(case, n, **kw)
    op.fitting(_rows75(x78), case["kp"])                      # (no iterations: everything is set up, nothing has run)
    return op, op._rows_x[2:2 + n].cpu().numpy().copy()


def _set_rows(op, n, x78):
    """new rows through fdcap_opt_set_inputs"""
    x = torch.tensor(np.asarray(x78, dtype=np.float32)).cuda().contiguous()
    eye = torch.eye(4, device="cuda").reshape(1, 16).repeat(n, 1).contiguous()
    capi.check(op.ctx.lib.fdcap_opt_set_inputs(op.ctx.handle, capi.dptr(x), capi.dptr(x), capi.dptr(torch.ones(n, device="cuda")), capi.dptr(eye),
                                               capi.current_stream()), "fdcap_opt_set_inputs")


def _lbfgs_cfg(**over):
    q = {**DEFAULT_LBFGS, **over}
    return capi.LbfgsConfig(capi.XDIM, q["history"], q["max_iter"], q["max_eval"], q["max_steps"], q["max_ls"], q["lr"], q["tolerance_grad"],
                            q["tolerance_change"], q["ftol"], q["gtol"])


def _bar(a32, a64):
    return M * max(float(np.abs(a32 - a64).max()), EPS32 * float(np.abs(a64).max()))


# ---- the depth guess --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mapped", [(1, False), (1, True), (5, False), (5, True), (67, False), (67, True)])
def test_guess_writes_the_depth_and_nothing_else(n, mapped):
    case = fs.make_case(n, 100 + n, mapped, synth)
    s, kp = case["settings"], case["kp"]
    (ls, lh), (rs, rh) = s["edges"]
    for f in range(n):
        if f % 4 == 1:
            kp[f, ls, 2] = 0.0                               # an undetected shoulder: the other edge alone
        if f % 4 == 3:
            kp[f, ls, 2] = kp[f, rh, 2] = 0.0                # no edge with both ends: the default depth
    if n >= 5:                                               # shoulders 24.9 and 25.1 pixels apart
        for f, d in ((0, 24.9), (2, 25.1)):
            kp[f, rs, :2] = kp[f, ls, :2] + np.float32(d) * np.array([0.6, 0.8], np.float32)
    x = case["gt78"].copy()
    x[:, 75:78] = (0.3, -0.2, 9.0)                           # (whatever the rows held: overwritten)
    op, state = _load(case, n, x)
    lib, h = op.ctx.lib, op.ctx.handle
    before = op._rows_x.clone()
    z, valid, side = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    sg, ci = _stage(), _struct(s)
    capi.check(lib.fdcap_opt_fit2d_guess(h, ctypes.byref(sg), ctypes.byref(ci), capi.dptr(z), capi.dptr(valid), capi.dptr(side), capi.current_stream()), "guess")
    after, z, valid, side = op._rows_x.cpu().numpy(), z.cpu().numpy(), valid.cpu().numpy(), side.cpu().numpy()
    z64, v64 = fs.spec_of(case).depth_guess(state, kp)
    z32, _ = fs.spec_of(case, dtype=torch.float32).depth_guess(state, kp)
    bar = M * np.maximum(np.abs(z32 - z64), EPS32 * np.abs(z64))
    print(f"n {n} mapped {mapped}: max |z - z64| / bar {float((np.abs(z - z64) / bar).max()):.3g}, valid {valid.tolist()[:8]}")
    assert np.array_equal(valid, v64) and [int(v) for v in v64[:4]] == [1, 1, 1, 0][:min(n, 4)]
    assert np.all(np.abs(z - z64) <= bar) and np.all(z[v64 == 0] == np.float32(2.5))
    keep = list(range(75))
    assert np.array_equal(after[:, keep].view(np.uint32), before.cpu().numpy()[:, keep].view(np.uint32))      # every other column, halo rows too: the same bits
    assert np.array_equal(after[2:2 + n, 75:78], np.stack([np.zeros(n), np.zeros(n), z], 1).astype(np.float32)) and np.all(after[[0, 1, -2, -1], 75:78] == 0)
    want_side = fs.spec_of(case).side_view(kp)
    assert np.array_equal(side, want_side)
    if n >= 5:
        d = fs.spec_of(case).shoulder_distance(kp)
        assert 24.8 < d[0] < 25.0 < d[2] < 25.2 and side[0] == 1 and side[2] == 0
    # only the optional outputs differ when they are left out
    capi.check(lib.fdcap_opt_fit2d_guess(h, ctypes.byref(sg), ctypes.byref(ci), None, None, None, capi.current_stream()), "guess")
    assert np.array_equal(op._rows_x.cpu().numpy().view(np.uint32), after.view(np.uint32))
    op.close()


# ---- one evaluation of the camera stage -------------------------------------------------------------------------------------------------
def _camera_eval(op, n, ci, log_terms):
    lib, h = op.ctx.lib, op.ctx.handle
    sg = _stage()
    capi.check(lib.fdcap_opt_backward_fit2d_camera(h, ctypes.byref(sg), ctypes.byref(ci), log_terms, capi.current_stream()), "backward_fit2d_camera")
    dx = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, capi.current_stream()), "get_grads")
    return dx.cpu().numpy(), op._losses.cpu().numpy().copy()


def _frame_values(op, n, ci):
    """the objective per frame at the current rows: one round of the L-BFGS driver, whose budget then ends inside every frame's line
    search -- the rows come back (roll-back) and the stats hold the value at the accepted point, the start"""
    lib, h = op.ctx.lib, op.ctx.handle
    sg, cf, rounds, left = _stage(), _lbfgs_cfg(), ctypes.c_int32(0), ctypes.c_int32(-1)
    capi.check(lib.fdcap_opt_fit2d_camera_lbfgs(h, ctypes.byref(sg), ctypes.byref(ci), ctypes.byref(cf), 1, ctypes.byref(rounds), capi.current_stream()), "camera_lbfgs")
    fl = torch.empty(n, device="cuda")
    capi.check(lib.fdcap_opt_fit2d_lbfgs_stats(h, None, None, capi.dptr(fl), capi.current_stream()), "stats")
    capi.check(lib.fdcap_opt_fit2d_lbfgs_rolled_back(h, ctypes.byref(left)), "rolled_back")
    assert rounds.value == 1
    return fl.cpu().numpy(), left.value


def _check_eval(case, spec_kw, x, z0, dx, sums, fl, label):
    f64, g64 = fs.spec_of(case, **spec_kw).camera_grads(x, case["kp"], z0)
    f32, g32 = fs.spec_of(case, dtype=torch.float32, **spec_kw).camera_grads(x, case["kp"], z0)
    bar_f = M * np.maximum(np.abs(f32 - f64), EPS32 * np.abs(f64))
    blocks = {"sixd": fs.FREE[:6], "camt": fs.FREE[6:]}
    ratios = {k: float(np.abs(dx[:, c] - g64[:, c]).max()) / _bar(g32[:, c], g64[:, c]) for k, c in blocks.items()}
    print(f"{label}: max|err| / bar: gradient {ratios}, frame values {float((np.abs(fl - f64) / bar_f).max()) if fl is not None else None}, "
          f"sum {abs(sums[0] + sums[1] - f64.sum()) / bar_f.sum():.3g}")
    assert max(ratios.values()) <= 1.0, ratios
    assert np.all(dx[:, fs.FIXED] == 0)                      # the other 69 columns: exact zeros
    assert abs(sums[0] + sums[1] - f64.sum()) <= bar_f.sum()
    depth = case["settings"]["w_depth"] ** 2 * float(((x[:, 77].astype(np.float64) - z0) ** 2).sum())
    assert abs(sums[1] - depth) <= 1e-5 * max(depth, 1e-30) + 1e-12
    if fl is not None:
        assert np.all(np.abs(fl - f64) <= bar_f), (fl, f64, bar_f)


@pytest.mark.parametrize("n,n_torso,mapped", [(1, 1, False), (1, 4, True), (1, 8, False), (5, 1, True), (5, 4, False), (5, 8, True), (67, 1, False),
                                              (67, 4, True), (67, 8, False)])
def test_camera_objective_value_and_gradient(n, n_torso, mapped):
    case = fs.make_case(n, 200 + n + n_torso, mapped, synth, torso_joints=TORSO8[:n_torso], noise_px=15.0)
    rng = np.random.Generator(np.random.PCG64(7 * n + n_torso))
    s = dict(case["settings"], conf_thr=0.25)
    kw = {"conf_thr": 0.25}
    if n_torso > 1:
        case["kp"][:, s["torso"][1], 2] = 0.25               # one keypoint gated out (conf == conf_thr), whatever the others say
    ci = _struct(s)
    xs = case["gt78"].copy()
    xs[:, 75:77] = 0.0
    op, xs = _load(case, n, xs)
    z0 = xs[:, 77].astype(np.float64)
    _camera_eval(op, n, ci, 2)                               # set-up at xs
    # the evaluation point: 0.3 rad and some centimetres away from the set-up's rows, so q_k is not trivially current
    x = fs.turned(xs, 0.3, rng)
    x[:, 75:78] += (0.05 * rng.standard_normal((n, 3))).astype(np.float32)
    op._rows_x[2:2 + n] = torch.tensor(x).cuda()
    dx, sums = _camera_eval(op, n, ci, 1)
    fl, left = _frame_values(op, n, ci)
    assert left == n and np.array_equal(op._rows_x[2:2 + n].cpu().numpy().view(np.uint32), x.view(np.uint32))      # rolled back to x, bit for bit
    _check_eval(case, kw, x, z0, dx, sums, fl, f"n {n} torso {n_torso} mapped {mapped}")
    # new rows through fdcap_opt_set_inputs: the set-up is refreshed without being asked for
    x2 = fs.turned(case["gt78"], 0.5, rng)
    x2[:, 0:3] += np.float32(0.1)
    x2[:, 75:78] = case["gt78"][:, 75:78] * np.float32(1.1)
    _set_rows(op, n, x2)
    dx2, sums2 = _camera_eval(op, n, ci, 1)
    _check_eval(case, kw, x2, x2[:, 77].astype(np.float64), dx2, sums2, None, "  after set_inputs")
    op.close()


# ---- the camera stage -------------------------------------------------------------------------------------------------------------------
STAGE_SEED, STAGE_N, ADAM_ITERS, ADAM_LR = 51, 3, 60, 0.01
# Margins and the fraction, fixed from the twin alone (this seed, 23-joint layout; its figures: the test's docstring):
#   L-BFGS: termination lies inside a flat valley (SMPLify-X's ftol 2e-9 is below fp32's resolution of the loss), where two fp32
#           computations stop at different points; the fp32 twin's own largest per-frame distance to the fp64 minimiser estimates the
#           valley's extent from three samples, and the library is one more sample of it: 4 x that figure.
#   Adam:   a deterministic path; the library's gradient differs from the fp64 one by up to the gradient bars, 32 x the fp32 twin's own
#           error, and Adam's update is linear in a small relative gradient error: 32 x the fp32 twin's distance.
#   the mean torso reprojection error ends below 0.1 of its start: the twin's own figures are in the tests' docstrings.
LBFGS_MARGIN, ADAM_MARGIN, ERROR_FRACTION = 4.0, M, 0.1
_twin_cache = {}


def _stage_start(n, seed):
    case = fs.make_case(n, seed, False, synth)
    x = fs.turned(case["gt78"], 0.4, np.random.Generator(np.random.PCG64(seed + 1)))
    return case, x


def _guess(op, n, ci):
    z = torch.empty(n, device="cuda")
    sg = _stage()
    capi.check(op.ctx.lib.fdcap_opt_fit2d_guess(op.ctx.handle, ctypes.byref(sg), ctypes.byref(ci), capi.dptr(z), None, None, capi.current_stream()), "guess")
    return op._rows_x[2:2 + n].cpu().numpy().copy()


def _run_stage(op, n, ci, optimizer):
    lib, h = op.ctx.lib, op.ctx.handle
    sg = _stage()
    if optimizer == "lbfgs":
        cf, rounds = _lbfgs_cfg(), ctypes.c_int32(0)
        capi.check(lib.fdcap_opt_fit2d_camera_lbfgs(h, ctypes.byref(sg), ctypes.byref(ci), ctypes.byref(cf), 4000, ctypes.byref(rounds), capi.current_stream()), "camera_lbfgs")
        assert 0 < rounds.value < 4000
    else:
        capi.check(lib.fdcap_opt_reset_adam(h, capi.current_stream()), "reset_adam")
        for it in range(ADAM_ITERS):
            capi.check(lib.fdcap_opt_backward_fit2d_camera(h, ctypes.byref(sg), ctypes.byref(ci), 0, capi.current_stream()), "backward_fit2d_camera")
            capi.check(lib.fdcap_opt_step_x(h, it + 1, capi.current_stream()), "step_x")
    return op._rows_x[2:2 + n].cpu().numpy().copy()


def _stage_twin(case, start, optimizer):
    key = (optimizer, start.tobytes())
    if key not in _twin_cache:
        s64, s32 = fs.spec_of(case), fs.spec_of(case, dtype=torch.float32)
        run = (lambda s: s.camera_stage_lbfgs(start, case["kp"])) if optimizer == "lbfgs" else (lambda s: s.camera_stage_adam(start, case["kp"], ADAM_ITERS, ADAM_LR))
        _twin_cache[key] = (run(s64), run(s32))
    return _twin_cache[key]


@pytest.mark.parametrize("optimizer", ["lbfgs", "adam"])
def test_camera_stage_reaches_the_twins_minimiser_and_keeps_the_fixed_columns(optimizer):
    """Twin alone, seed 51, three frames, start (0, 0, z_guess) and 0.4 rad off the truth.  L-BFGS: the fp32 twin ends
    [6.9e-5, 2.5e-5, 2.5e-4] from the fp64 twin's minimiser (largest column difference per frame), mean torso error 56.28 -> 1.748 px in
    both precisions: fraction 0.031.  Adam, 60 steps of 0.01: the fp32 twin ends within 3e-7 of the fp64 twin, mean torso error
    56.28 -> 3.351 px: fraction 0.060."""
    n = STAGE_N
    case, x = _stage_start(n, STAGE_SEED)
    ci = _struct(case["settings"])
    op, _ = _load(case, n, x, lr=ADAM_LR)
    start = _guess(op, n, ci)
    assert np.all(start[:, 75:77] == 0) and np.all(start[:, 77] > 1.5)
    end = _run_stage(op, n, ci, optimizer)
    assert np.array_equal(end[:, fs.FIXED].view(np.uint32), start[:, fs.FIXED].view(np.uint32))            # the 69 fixed columns keep their bits
    t64, t32 = _stage_twin(case, start, optimizer)
    d32 = np.abs(t32[:, fs.FREE] - t64[:, fs.FREE]).max(1)
    d = np.abs(end[:, fs.FREE] - t64[:, fs.FREE]).max(1)
    s64 = fs.spec_of(case)
    e0, e64, e32, e = (float(s64.torso_error(r, case["kp"]).mean()) for r in (start, t64, t32, end))
    print(f"{optimizer}: distance to the fp64 twin's end, fp32 twin {d32}, library {d}; mean torso error start {e0:.3f} fp64 {e64:.3f} fp32 {e32:.3f} library {e:.3f}")
    if optimizer == "lbfgs":
        assert d.max() <= LBFGS_MARGIN * d32.max()
    else:
        assert np.all(d <= ADAM_MARGIN * np.maximum(d32, EPS32 * np.abs(t64[:, fs.FREE]).max(1)))
    assert e64 < ERROR_FRACTION * e0 and e32 < ERROR_FRACTION * e0 and e < ERROR_FRACTION * e0
    op.close()


@pytest.mark.parametrize("optimizer,mapped", [("lbfgs", True), ("adam", False)])
def test_camera_stage_on_67_frames_keeps_the_fixed_columns(optimizer, mapped):
    n = 67
    case = fs.make_case(n, 300, mapped, synth)
    x = fs.turned(case["gt78"], 0.4, np.random.Generator(np.random.PCG64(301)))
    ci = _struct(case["settings"])
    op, _ = _load(case, n, x, lr=ADAM_LR)
    start = _guess(op, n, ci)
    end = _run_stage(op, n, ci, optimizer)
    assert np.array_equal(end[:, fs.FIXED].view(np.uint32), start[:, fs.FIXED].view(np.uint32))
    assert np.abs(end[:, fs.FREE] - start[:, fs.FREE]).max(1).min() > 1e-3                                  # (every frame moved)
    s64 = fs.spec_of(case)
    e0, e = float(s64.torso_error(start, case["kp"]).mean()), float(s64.torso_error(end, case["kp"]).mean())
    print(f"{optimizer} mapped {mapped}: mean torso error {e0:.3f} -> {e:.3f}")
    assert e < ERROR_FRACTION * e0
    op.close()


# ---- flip and select --------------------------------------------------------------------------------------------------------------------
def test_flip_kernel_turns_the_body_about_y():
    rng = np.random.Generator(np.random.PCG64(400))
    n = 67
    rows = rng.standard_normal((n, 75)).astype(np.float32)
    rows[0, 3:6] = 0.0
    rows[1:, 3:6] *= (rng.uniform(0.1, 2.9, (n - 1, 1)) / np.linalg.norm(rows[1:, 3:6], axis=1, keepdims=True)).astype(np.float32)
    d = torch.tensor(rows).cuda()
    lib = capi.load_library()
    capi.check(lib.fdcap_fit2d_flip_orient(capi.dptr(d), n, capi.current_stream()), "flip")
    once = d.cpu().numpy()
    capi.check(lib.fdcap_fit2d_flip_orient(capi.dptr(d), n, capi.current_stream()), "flip")
    twice = d.cpu().numpy()
    keep = [c for c in range(75) if not 3 <= c < 6]
    assert np.array_equal(once[:, keep].view(np.uint32), rows[:, keep].view(np.uint32))
    err = np.abs(fs.rodrigues(once[:, 3:6]) - fs.flip_rotation(rows[:, 3:6])).max()
    print("flip: max|R err|", err, "twice max|err|", np.abs(twice - rows).max())
    assert err <= 2e-6 and np.abs(twice - rows).max() <= 1e-6         # (tests/test_fit2d_init_cpu.py's bars)
    assert capi.load_library().fdcap_fit2d_flip_orient(None, 3, None) == -1 and lib.fdcap_fit2d_flip_orient(capi.dptr(d), 0, None) == -1


def _select(rows, loss, src, n, jaw=None):
    lib = capi.load_library()
    m = len(src)
    dev = lambda a, dt: None if a is None else torch.tensor(np.asarray(a)).to(dt).cuda().contiguous()
    rows_d, loss_d, src_d, jaw_d = dev(rows, torch.float32), dev(loss, torch.float32), dev(src, torch.int32) if m else None, dev(jaw, torch.float32)
    out, chosen = torch.full((n, 75), np.nan, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda")
    jaw_out = None if jaw is None else torch.full((n, 3), np.nan, device="cuda")
    capi.check(lib.fdcap_fit2d_select(capi.dptr(rows_d), capi.dptr(loss_d), capi.dptr(src_d), n, m, capi.dptr(jaw_d), capi.dptr(out), capi.dptr(jaw_out),
                                      capi.dptr(chosen), capi.current_stream()), "select")
    return out.cpu().numpy(), chosen.cpu().numpy(), None if jaw is None else jaw_out.cpu().numpy()


@pytest.mark.parametrize("n,src,with_jaw", [(1, [], False), (1, [0], True), (5, [], True), (5, [0, 1, 2, 3, 4], False), (5, [0, 4], True), (67, [0, 3, 31, 32, 33, 66], True),
                                            (67, list(range(67)), True)])
def test_select_copies_the_better_problem(n, src, with_jaw):
    rng = np.random.Generator(np.random.PCG64(500 + n + len(src)))
    m = len(src)
    rows = rng.standard_normal((n + m, 75)).astype(np.float32)
    jaw = rng.standard_normal((n + m, 3)).astype(np.float32) if with_jaw else None
    loss = rng.uniform(1.0, 2.0, n + m).astype(np.float32)
    for i, f in enumerate(src):                              # ties, NaN on either side and on both, inf against NaN
        kind = i % 6
        if kind == 1:
            loss[n + i] = loss[f]
        if kind == 2:
            loss[f] = np.nan
        if kind == 3:
            loss[n + i] = np.nan
        if kind == 4:
            loss[f] = loss[n + i] = np.nan
        if kind == 5:
            loss[f], loss[n + i] = np.inf, np.nan
    want_chosen, take = fs.select(loss, src)
    out, chosen, jaw_out = _select(rows, loss, src, n, jaw)
    assert np.array_equal(chosen, want_chosen)
    assert np.array_equal(out.view(np.uint32), rows[take].view(np.uint32))                                  # exact copies
    if with_jaw:
        assert np.array_equal(jaw_out.view(np.uint32), jaw[take].view(np.uint32))
    if m >= 6:
        assert set(chosen[src].tolist()) == {0, 1}


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    n = 4
    case = fs.make_case(n, 600, True, synth)
    s = case["settings"]
    sg, ok, z = _stage(), _struct(s), torch.empty(n, device="cuda")
    cf, fl = _lbfgs_cfg(), torch.empty(n, device="cuda")
    op = _op(case, n)
    lib, h = op.ctx.lib, op.ctx.handle
    calls = lambda ci: (lib.fdcap_opt_fit2d_guess(h, ctypes.byref(sg), ctypes.byref(ci), capi.dptr(z), None, None, None),
                        lib.fdcap_opt_backward_fit2d_camera(h, ctypes.byref(sg), ctypes.byref(ci), 0, None),
                        lib.fdcap_opt_fit2d_camera_lbfgs(h, ctypes.byref(sg), ctypes.byref(ci), ctypes.byref(cf), 10, None, None))
    E_ARG, E_STATE = -1, -2
    assert calls(ok) == (E_STATE,) * 3 and lib.fdcap_opt_fit2d_frame_loss(h, ctypes.byref(sg), capi.dptr(fl), None) == E_STATE       # no optimiser
    op.fitting(_rows75(case["gt78"]), case["kp"])
    assert calls(ok) == (0, 0, 0) and lib.fdcap_opt_fit2d_frame_loss(h, ctypes.byref(sg), capi.dptr(fl), None) == 0
    surface = int(np.flatnonzero(case["joint_of_slot"] < 0)[0])
    nine = _struct(dict(s, torso=(s["torso"] * 2)[:8]))
    nine.n_torso = 9
    five = _struct(s)
    five.n_edge = 5
    bad = [dict(s, edges=[]), dict(s, torso=[]), dict(s, torso=[len(case["joint_of_slot"])] + s["torso"][1:]), dict(s, torso=[-1] + s["torso"][1:]),
           dict(s, torso=[surface] + s["torso"][1:]), dict(s, edges=[(surface, s["edges"][0][1]), s["edges"][1]]), dict(s, shoulders=(s["shoulders"][0], 99))]
    bad += [dict(s, **{k: v}) for k in ("conf_thr", "default_depth", "side_view_px", "w_data", "w_depth") for v in (float("nan"), float("inf"))]
    for b in bad:
        assert calls(_struct(b)) == (E_ARG,) * 3, b
    assert calls(nine) == (E_ARG,) * 3 and calls(five) == (E_ARG,) * 3
    assert lib.fdcap_opt_fit2d_guess(h, None, ctypes.byref(ok), None, None, None, None) == E_ARG
    assert lib.fdcap_opt_backward_fit2d_camera(h, ctypes.byref(sg), None, 0, None) == E_ARG
    assert lib.fdcap_opt_fit2d_camera_lbfgs(h, ctypes.byref(sg), ctypes.byref(ok), None, 10, None, None) == E_ARG
    assert lib.fdcap_opt_fit2d_camera_lbfgs(h, ctypes.byref(sg), ctypes.byref(ok), ctypes.byref(cf), 0, None, None) == E_ARG
    assert lib.fdcap_opt_fit2d_frame_loss(h, ctypes.byref(sg), None, None) == E_ARG
    rows, loss, out = torch.zeros(6, 75, device="cuda"), torch.zeros(6, device="cuda"), torch.zeros(4, 75, device="cuda")
    src, jaw = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(6, 3, device="cuda")
    sel = lambda *a: lib.fdcap_fit2d_select(*[capi.dptr(v) if torch.is_tensor(v) else v for v in a], None)
    assert sel(rows, loss, src, 4, 2, None, out, None, None) == 0
    assert sel(None, loss, src, 4, 2, None, out, None, None) == E_ARG and sel(rows, loss, None, 4, 2, None, out, None, None) == E_ARG
    assert sel(rows, loss, src, 4, 5, None, out, None, None) == E_ARG and sel(rows, loss, src, 0, 0, None, out, None, None) == E_ARG
    assert sel(rows, loss, src, 4, 2, jaw, out, None, None) == E_ARG and sel(rows, loss, src, 4, -1, None, out, None, None) == E_ARG
    torch.cuda.synchronize()
    op.close()
    # a batch of clips, a shard of a clip, an optimiser without keypoints: FDCAP_E_STATE
    for kind in ("batch", "shard", "no_keypoints"):
        ctx = capi.Context(case["bm"], case["vp"])
        ctx.set_scene(np.zeros((0, 3), np.float32))
        ctx.set_keypoint_map(*case["map"])
        nl, clips = (n, 2) if kind == "batch" else (n, 1)
        oc = capi.OptConfig(n if kind != "shard" else 2 * n, nl, 0, 0.01, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)
        R = nl * clips + 4
        bufs = (torch.zeros(R, 78, device="cuda"), torch.zeros(R, 16, device="cuda"), torch.zeros(clips, device="cuda"), torch.zeros(clips, device="cuda"),
                torch.zeros(clips * capi.NUM_LOSSES, device="cuda", dtype=torch.float64))
        capi.check(ctx.lib.fdcap_opt_create_clips(ctx.handle, ctypes.byref(oc), clips, *(capi.dptr(b) for b in bufs)), "create")
        if kind == "shard":
            capi.check(ctx.lib.fdcap_opt_set_keypoints_mapped(ctx.handle, capi.dptr(torch.tensor(case["kp"]).cuda()), None), "set_keypoints_mapped")
        h2 = ctx.handle
        got = (ctx.lib.fdcap_opt_fit2d_guess(h2, ctypes.byref(sg), ctypes.byref(ok), capi.dptr(z), None, None, None),
               ctx.lib.fdcap_opt_backward_fit2d_camera(h2, ctypes.byref(sg), ctypes.byref(ok), 0, None),
               ctx.lib.fdcap_opt_fit2d_camera_lbfgs(h2, ctypes.byref(sg), ctypes.byref(ok), ctypes.byref(cf), 10, None, None),
               ctx.lib.fdcap_opt_fit2d_frame_loss(h2, ctypes.byref(sg), capi.dptr(fl), None))
        assert got == (E_STATE,) * 4, (kind, got)
        torch.cuda.synchronize()
        ctx.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
E2E_FRAMES = (0, 10, 16, 19, 12, 14)      # of the pool below: flagged 0, 16, 19, 14 (the twin takes the turned body for 16 alone), 10 and 12 not flagged
E2E_ITERS, E2E_LR, E2E_SIDE_PX = 30, 0.03, 60.0


def _e2e_case():
    """Keypoints of ground-truth bodies 2.2 to 3 m in front of the camera, turned about y by about (10, -25, 140, 215, 130, 60, 170, -160)
    degrees in turn (the second half faces the other way), 1 px of noise.  The frames were CHOSEN WITH THE TWIN ALONE from a pool of 24
    (seeds 700 / 701).  Adam from the neutral start does not reach a minimum in 30 steps a stage, and for most frames of the pool the
    order of the two hypotheses' final objectives changes with where within 1e-3 of the neutral rows the start stands (the twin cannot
    stand ON them: _e2e_twin) -- frame 15's ratio first / turned is 2.36, 0.73, 0.81 or 0.72 for four such starts.  Kept are the frames
    whose ratio stays beyond a factor 1.5 on one side for all four starts in fp64 and for the first of them in fp32:
        frame 0: 0.38 .. 0.66    frame 14: 0.49 .. 0.66    frame 16: 1.73 .. 2.13    frame 19: 0.26 .. 0.54
    (starts: latent +1e-3, -1e-3, 1e-3 with random signs, 1e-5 with random signs).  Frames 10 and 12 are not flagged as side views
    (shoulders 60 px apart or more).  Every frame's stage sequence brings the mean reprojection error from 70 .. 130 px after the guess
    to 4 .. 9 px.  Frames are independent problems, so the subset's fits are the pool's."""
    n = 24
    rng = np.random.Generator(np.random.PCG64(700))
    th = np.deg2rad(np.tile([10.0, -25.0, 140.0, 215.0, 130.0, 60.0, 170.0, -160.0], 3) + rng.uniform(-10, 10, n))
    zs = rng.uniform(2.2, 3.0, n)
    bm, vp = synth.make_body_model(240, seed=61), synth.make_vposer(seed=702)
    rng = np.random.Generator(np.random.PCG64(704))
    gt = np.zeros((n, 75), np.float32)
    R = fs.rodrigues(np.stack([np.zeros(n), th, np.zeros(n)], 1)) @ fs.rodrigues(0.1 * rng.standard_normal((n, 3)))
    gt[:, 3:6] = rotrepr.matrot2aa(torch.tensor(R)).numpy()
    gt[:, 6:16], gt[:, 16:48] = 0.3 * rng.standard_normal((n, 10)), 1.0 * rng.standard_normal((n, 32))
    gt[:, 72:75] = np.stack([0.2 * rng.standard_normal(n), 0.2 * rng.standard_normal(n), zs], 1)
    settings = fs.settings_for(np.arange(23), side_view_px=E2E_SIDE_PX)
    spec = fs.Fit2dInitSpec(bm, vp, settings, intrinsics=fs.INTRINSICS)
    gt78 = rotrepr.convert_to_6D_rot(torch.tensor(gt, dtype=torch.float64)).numpy().astype(np.float32)
    with torch.no_grad():
        uv = spec.project(spec.joints_cam(torch.tensor(gt78, dtype=torch.float64))).numpy()
    kp = np.concatenate([uv + 1.0 * rng.standard_normal(uv.shape), rng.uniform(0.5, 1.0, uv.shape[:2] + (1,))], -1).astype(np.float32)
    pick = list(E2E_FRAMES)
    return dict(bm=bm, vp=vp, map=None, joint_of_slot=np.arange(23), settings=settings, gt78=gt78[pick], kp=kp[pick])


def _to75(x78, dtype=torch.float64):
    return rotrepr.convert_to_3D_rot(torch.tensor(np.asarray(x78), dtype=dtype)).numpy().astype(np.float32)


def _e2e_twin(spec, kp):
    """InnerFitOP(init=..., optimizer="adam")'s sequence in the twin.  The oracle's log map has a NaN gradient at the identity, which
    the neutral rows' orientation and (with the synthetic decoder) every body joint at latent 0 are: the twin starts 1e-3 next to
    them, the library at the neutral rows themselves."""
    n = kp.shape[0]
    r0 = torch.zeros(n, 75, dtype=torch.float64)
    r0[:, 4], r0[:, 16:48] = 1e-3, 1e-3
    x0 = rotrepr.convert_to_6D_rot(r0).numpy()
    z, _ = spec.depth_guess(x0, kp)
    x0[:, 77] = z
    x0 = x0.astype(np.float32)
    first = spec.camera_stage_adam(x0, kp, E2E_ITERS, E2E_LR)
    src = np.flatnonzero(spec.side_view(kp))
    t0 = _to75(x0[src])
    t0[:, 3:6] = rotrepr.matrot2aa(torch.tensor(fs.flip_rotation(t0[:, 3:6]))).numpy()
    twin = spec.camera_stage_adam(rotrepr.convert_to_6D_rot(torch.tensor(t0, dtype=torch.float64)).numpy().astype(np.float32), kp[src], E2E_ITERS, E2E_LR)
    kps = np.concatenate([kp, kp[src]])
    spec.lr = E2E_LR
    out = spec.fitting(np.concatenate([_to75(first), _to75(twin)]), kps, DEFAULT_STAGES, E2E_ITERS).numpy()
    with torch.no_grad():
        fl = spec.frame_loss(spec.x78, torch.tensor(kps, dtype=spec.dtype), DEFAULT_STAGES[-1]).numpy()
    chosen, take = fs.select(fl, src)
    return dict(x0=x0, src=src, loss=fl, chosen=chosen, rows=out[take])


def _px_error(spec, rows75, kp):
    with torch.no_grad():
        uv = spec.project(spec.joints_cam(rotrepr.convert_to_6D_rot(torch.tensor(np.asarray(rows75), dtype=torch.float64)))).numpy()
    return np.sqrt(((uv - kp[..., :2]) ** 2).sum(-1)).mean(1)


def test_end_to_end_from_keypoints_alone_and_given_orientations_are_todays_calls():
    case = _e2e_case()
    n, kp = len(E2E_FRAMES), case["kp"]
    spec = fs.spec_of(case)
    tw = _e2e_twin(spec, kp)
    n_src = len(tw["src"])
    ratio = tw["loss"][tw["src"]] / tw["loss"][n:]
    print("twin: flagged", tw["src"], "objective first / turned", ratio, "chosen", tw["chosen"])
    assert tw["src"].tolist() == [0, 2, 3, 5] and tw["chosen"].tolist() == [0, 0, 1, 0, 0, 0] and np.all(np.maximum(ratio, 1 / ratio) > 1.5)
    kw = dict(intrinsics=fs.INTRINSICS, lr=E2E_LR, iters_per_stage=E2E_ITERS, init=dict(side_view_px=E2E_SIDE_PX))
    op = InnerFitOP(case["bm"], case["vp"], n, **kw)
    out = op.fitting(None, kp).cpu().numpy()
    lib_ratio = op.final_loss.cpu().numpy()[tw["src"]] / op.final_loss.cpu().numpy()[n:]
    after_guess = np.zeros((n, 75), np.float32)
    after_guess[:, 74] = op.depth_guess
    e_guess, e_end, e_twin = _px_error(spec, after_guess, kp), _px_error(spec, out, kp), _px_error(spec, tw["rows"], kp)
    print("library: objective first / turned", lib_ratio, "chosen", op.chosen, "mean reprojection error after the guess", e_guess, "at the end", e_end, "twin's end", e_twin)
    z64, _ = spec.depth_guess(tw["x0"], kp)
    assert np.all(op.depth_valid == 1) and np.allclose(op.depth_guess, z64, rtol=1e-3)                       # (the twin's rows stand 1e-3 off the neutral ones)
    assert op.tried_both.tolist() == [True, False, True, True, False, True] and op.chosen.tolist() == tw["chosen"].tolist()
    assert len(op.frame_loss) == 0 and op.body_rotation_rec.shape[0] == n + n_src
    assert e_end.mean() <= 0.5 * e_guess.mean() and e_twin.mean() <= 0.5 * e_guess.mean()
    assert np.all(np.isfinite(out)) and tuple(out.shape) == (n, 75)
    # orientations="given": today's call sequence from the rows the camera stage left, bit for bit
    given = InnerFitOP(case["bm"], case["vp"], n, orientations="given", **kw)
    out_g = given.fitting(None, kp).cpu().numpy()
    assert not given.tried_both.any() and not given.chosen.any()
    plain = InnerFitOP(case["bm"], case["vp"], n, **{k: v for k, v in kw.items() if k != "init"})
    out_p = plain.fitting(given.camera_rows, kp).cpu().numpy()
    assert np.array_equal(out_g.view(np.uint32), out_p.view(np.uint32))
    # ... and the camera stage moved only camera_translation and global_orient of the neutral rows
    cam = given.camera_rows.cpu().numpy()
    assert np.all(cam[:, 0:3] == 0) and np.all(cam[:, 6:72] == 0) and np.abs(cam[:, 3:6]).max() > 0.05
    with pytest.raises(capi.FdcapError):
        plain.fitting(None, kp)
    for o in (op, given, plain):
        o.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_command_line_fits_a_folder_of_openpose_files(tmp_path):
    n = 6
    body25 = [i for i in OPENPOSE_BODY25 if i < 55]
    cols = [c for c, i in enumerate(OPENPOSE_BODY25) if i < 55]
    base = fs.make_case(n, 800, False, synth, depth=(2.5, 3.5))
    kmap = KeypointMap.from_smplx_indices(body25, [])
    spec = fs.Fit2dInitSpec(base["bm"], base["vp"], fs.settings_for(kmap.joint), kmap.joint, kmap.tri, kmap.bary, intrinsics=fs.INTRINSICS)
    with torch.no_grad():
        uv = spec.project(spec.joints_cam(torch.tensor(base["gt78"], dtype=torch.float64))).numpy()
    kp = np.zeros((n, 25, 3), np.float32)
    kp[:, cols, :2], kp[:, cols, 2] = uv, 0.9
    (tmp_path / "kp").mkdir()
    for f in range(n):
        rec = {"people": [{"pose_keypoints_2d": [float(v) for v in kp[f].reshape(-1)]}]}
        (tmp_path / "kp" / f"clip_{f:012d}_keypoints.json").write_text(json.dumps(rec))
    body_path = str(tmp_path / "body")
    argv = [str(tmp_path / "kp"), body_path, "--optimizer", "adam", "--frames-per-batch", "4", "--intrinsics", *(str(v) for v in fs.INTRINSICS)]
    assert cli_innerfit.main(argv, body_model=base["bm"], vposer=base["vp"]) == 0
    rows = fio.load_body_gen(body_path)
    assert rows.shape == (n, 75) and np.all(np.isfinite(rows)) and np.all(rows[:, 74] > 1.5)
    # the command line is plumbing: its first batch is InnerFitOP's own result on the same keypoints
    op = InnerFitOP(base["bm"], base["vp"], 4, intrinsics=fs.INTRINSICS, optimizer="adam", keypoint_map=kmap, init={})
    want = op.fitting(None, kp[:4][:, cols]).cpu().numpy()
    assert np.array_equal(rows[:4].view(np.uint32), want.view(np.uint32))
    op.close()
