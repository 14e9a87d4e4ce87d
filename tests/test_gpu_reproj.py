"""GPU tests of the clip-level reprojection term (fdcap_opt_set_reproj; pose_bwd_reproj_kernel, csrc/fdc_k_pose_bwd.inc) against the
twin of tests/reproj_spec.py.  Inputs: the models and clips of tests/test_settings_cpu.make_case at rs.CASES (12 frames; 4 frames
with one contact vertex per leg; 7 frames of odd sizes; 65 frames, one past a 64-row edge; one frame) and the 4-frame case without a
scene and without contact ids; rows at gb.start_state of the clip carrying the depth offset, keypoints rs.make_keypoints (2 px
noise, one keypoint 150 px off, one undetected with NaN coordinates, one whole frame undetected where n >= 4); rs.check_inputs
asserts the conditions before anything is compared.

Bars: the isolated gradient per block at tests/gradient_bars.py's formula (M = 32) from the twin's two precisions -- no bar is taken
from a HIP result; tests/test_reproj_cpu.py shows on the CPU that the mutants leave them by a factor of 20 -- with exact zeros where
the fp64 gradient is all zero (lh, rh, d scale, all 16 entries of every d camera_ext row); the logged value at LOG_RTOL; the mixed
gradient at GRAD_RTOL / GRAD_ATOL (tests/test_settings_cpu.py).

Worst measured max|err| / bar per block of the isolated gradient over the six cases, both phases, log_terms 0 and 1 (MI355X), fp16
planes / exact fp32:  transl 0.061 / 0.056   sixd 0.031 / 0.045   betas 0.033 / 0.041   latent 0.030 / 0.035   camt 0.061 / 0.056
lh, rh, dscale, cam_rot, cam_transl, cam_bottom 0 / 0 (exact zeros).  The logged value: at most 2.6e-7 relative off the fp64 twin.
Beside the other terms: max|err| 4.8e-7 at max|g| 0.34 (12 frames), 4.1e-7 at 1.2 (7 frames).  The comparative fit: mean pixel error
10.53 at the start, 21.86 after 40 iterations without the term, 5.62 with it (the CPU twin's own Adam loop: 10.53 / 21.86 / 5.62)."""
import ctypes
import dataclasses
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
import tests.gradient_bars as gb
import tests.test_settings_cpu as sc
from fdcap_amd import capi
from fdcap_amd import fitting as fit_mod
from fdcap_amd.fitting import ClipBatchFitter, FittingOP
from fdcap_amd.io import read_camerapose
from tests import reproj_spec as rs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 10 ** 6
NO_SCENE = "no-scene"                       # rs.CASES[1]'s models and clip without a scene and without contact ids
CASES = list(rs.CASES) + [NO_SCENE]
ZERO_BLOCKS = ("lh", "rh", "dscale", "cam_rot", "cam_transl", "cam_bottom")
FIT_CASE, FIT_ITERS, FIT_WEIGHT = rs.CASES[0], 40, 2e-2        # (tests/test_reproj_cpu.py: the same fit with the twin's own Adam loop)


def _case(case):
    return rs.CASES[1] if case == NO_SCENE else case


def _ids(c):
    return c if isinstance(c, str) else "-".join(map(str, c))


def make_fop(case, lossconfig, num_iter=500, fittingconfig=None):
    bm, vp, clip, scene, vid, n = sc.make_case(*_case(case))
    if case == NO_SCENE:
        scene, vid = None, np.zeros(0, np.int64)
    return FittingOP(dict({"num_iter": num_iter}, **(fittingconfig or {})), lossconfig, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                     camera_ext=read_camerapose(clip.camerapose_lines), n_left=len(vid) // 2)


def at_start(fop, case):
    """init() + the perturbation: the device holds exactly the rows the twin differentiates"""
    st = rs.start_state(_case(case))
    n = fop.num_body
    fop.init(torch.tensor(st["x78"]).cuda())
    fop._rows_x[2:2 + n] += sc.perturbation(n).float().cuda()
    assert np.array_equal(fop._rows_x[2:2 + n].cpu().numpy(), st["rows"])
    return st


def set_reproj(fop, case, weight=rs.WEIGHT, kp=None):
    fop.weight_reproj = weight
    fop._set_reproj(rs.make_keypoints(_case(case)) if kp is None else kp, rs.INTRINSICS, rs.RHO)


def joint_sets(fop):
    out = (ctypes.c_int32 * 8)()
    capi.check(fop.ctx.lib.fdcap_debug_pose_joint_sets(fop.ctx.handle, out), "fdcap_debug_pose_joint_sets")
    return tuple(out[:4]), tuple(out[4:])


def backward(fop, ii, P, log_terms):
    n = fop.num_body
    lib, h = fop.ctx.lib, fop.ctx.handle
    capi.check(lib.fdcap_opt_backward(h, ii, P, log_terms, capi.current_stream()), "fdcap_opt_backward")
    dx, dcam = torch.empty(n, 78, device="cuda"), torch.empty(n, 16, device="cuda")
    capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), capi.dptr(dcam), capi.current_stream()), "fdcap_opt_get_grads")
    torch.cuda.synchronize()
    return dx.cpu().numpy(), dcam.cpu().numpy(), fop._losses.cpu().numpy().copy(), float(fop._dscale.cpu()[0])


def isolated_backward(case, phase2, log_terms):
    """fdcap_opt_backward with the term alone: weight_loss_rec = 0, weight_contact = 0, the smoothing and world coefficients patched to 0.
    -> (blocks, losses_d with the term, losses_d of the same backward without it -- log_terms = 1 only --, the joint sets)"""
    with pytest.MonkeyPatch.context() as mp:
        for name in ("PHASE1_SMOOTH", "PHASE2_SMOOTH", "PHASE2_WORLD"):
            mp.setattr(fit_mod, name, 0.0)
        fop = make_fop(case, {"weight_loss_rec": 0.0, "weight_contact": 0.0})
        try:
            at_start(fop, case)
            set_reproj(fop, case)
            dx, dcam, losses, dscale = backward(fop, 5, 0 if phase2 else BIG, log_terms)
            sets = joint_sets(fop)
            out = gb.blocks(rows=dx, dcam=dcam)
            losses_off = None
            if log_terms:                                        # (d loss / d scale is summed over the frames by a logging backward only)
                out.update(gb.blocks(dscale=dscale))
                capi.check(fop.ctx.lib.fdcap_opt_set_reproj(fop.ctx.handle, None, None, capi.current_stream()), "fdcap_opt_set_reproj")
                losses_off = backward(fop, 5, 0 if phase2 else BIG, log_terms)[2]
        finally:
            fop.close()
    return out, losses, losses_off, sets


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from tests.test_gpu_reproj import CASES, isolated_backward
out = {}
for i, case in enumerate(CASES):
    for phase2 in (0, 1):
        for log_terms in (0, 1):
            for k, v in isolated_backward(case, bool(phase2), log_terms)[0].items():
                out["%%d/%%d/%%d/%%s" %% (i, phase2, log_terms, k)] = v
np.savez(sys.argv[1], **out)
print("RESULT ok")
"""


@pytest.fixture(scope="module")
def exact_fp32(tmp_path_factory):
    """All cases in ONE child process with the exact-fp32 products (FDCAP_GEMM_SPLIT3=0, read once per process)"""
    path = str(tmp_path_factory.mktemp("reproj_fp32") / "grads.npz")
    p = subprocess.run([sys.executable, "-c", _CHILD % ROOT, path], env=dict(os.environ, FDCAP_GEMM_SPLIT3="0"), capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stderr[-2000:]
    out = {}
    with np.load(path) as z:
        for key in z.files:
            i, phase2, log_terms, block = key.split("/")
            out.setdefault((int(i), int(phase2), int(log_terms)), {})[block] = z[key]
    return out


def _check_blocks(got, it, label):
    """every block within its bar, the all-zero blocks exact zeros; prints max|err| / bar per block -> the blocks that fail"""
    want = {k: it["g64"][k] for k in got}
    bad = gb.check(got, want, {k: it["bar"][k] for k in got}, 1.0, label)
    for k in ZERO_BLOCKS:
        if k in got and not np.all(np.asarray(got[k]) == 0):
            bad[k + " (exact zeros)"] = float(np.abs(got[k]).max())
    return bad


@pytest.mark.parametrize("index", range(len(CASES)), ids=[_ids(c) for c in CASES])
def test_isolated_gradient_and_logged_value(index, exact_fp32):
    """Checks 1 and 2: the term alone in both phases at log_terms 0 and 1, both product forms, every row block within its bar and
    lh, rh, d scale and every entry of d camera_ext exact zeros; slot 6 of a logging backward, normalised, against the fp64 twin
    at LOG_RTOL, slots 0..4 the bits of the same backward without the term, and jn >= 23 in every launch."""
    case = CASES[index]
    it = rs.isolated(_case(case))
    n = _case(case)[0]
    bad = {}
    for phase2 in (False, True):
        for log_terms in (0, 1):
            got, losses, losses_off, sets = isolated_backward(case, phase2, log_terms)
            assert sets[0][0] >= 23 and sets[1][0] >= 23, sets
            for form, blocks in (("fp16 planes", got), ("exact fp32", exact_fp32[(index, int(phase2), log_terms)])):
                b = _check_blocks(blocks, it, f"{form} {_ids(case)} phase {2 if phase2 else 1} log_terms {log_terms}")
                if b:
                    bad[(form, phase2, log_terms)] = b
            if log_terms:
                value = fit_mod.reproj_loss(losses, n, rs.WEIGHT)
                want = rs.WEIGHT * it["raw64"] / (23 * n)
                print(f"logged loss_reproj {value:.9g} vs fp64 twin {want:.9g}: rel {abs(value - want) / want:.3g}")
                assert abs(value - want) <= sc.LOG_RTOL * want
                assert losses[:5].tobytes() == losses_off[:5].tobytes() and losses_off[capi.LOSS_REPROJ] == 0.0
    assert not bad, f"blocks outside their bar {{block: (err / bar, bar, max|g|)}}: {bad}"


@pytest.mark.parametrize("phase2", [False, True])
@pytest.mark.parametrize("case", [rs.CASES[0], rs.CASES[2]], ids=_ids)
def test_beside_the_other_terms(case, phase2):
    """Check 3: default weights plus the term -- phase 1 with the contact term on the legs (ja_hi < 23: dA and dJb both live below and
    above it), phase 2 with world smoothing (dJw and dJb both live) -- the row gradient at the project's mixed-term bar against
    oracle + twin; the pose launches keep jn >= 23."""
    n = case[0]
    c = sc.make_case(*case)
    t = sc.term_gradients(c, sc.DEFAULTS["scale_init"], torch.float64, ("rec", "sm", "con", "ws"), as_the_gpu_holds_it=True, edit=rs.depth_edit(case))
    assert np.array_equal(t["rows"].numpy(), rs.start_rows(case).astype(np.float64))
    co = sc.coefficients(sc.DEFAULTS, phase2)
    own = rs.isolated(case)
    want = sum(co[k] * t["g"][k][0] for k in ("rec", "sm", "con", "ws")) + np.concatenate([own["g64"][k] for k in gb.ROW_BLOCKS], axis=1)
    fop = make_fop(case, {})
    try:
        at_start(fop, case)
        set_reproj(fop, case)
        dx, dcam, _, _ = backward(fop, 5, 0 if phase2 else BIG, 0)
        sets = joint_sets(fop)
        ja_hi = int(np.max([np.flatnonzero(w).max() for w in c[0].lbs_weights[c[4]]])) + 1
    finally:
        fop.close()
    assert sets[0][0] >= 23 and sets[1][0] >= 23, sets
    if not phase2:
        assert ja_hi < 23, ja_hi
    share = np.abs(np.concatenate([own["g64"][k] for k in gb.ROW_BLOCKS], axis=1)).max()
    print(f"{_ids(case)} phase {2 if phase2 else 1}: max|err| {np.abs(dx - want).max():.3g}, max|g| {np.abs(want).max():.3g}, the term's largest entry {share:.3g}")
    np.testing.assert_allclose(dx, want, rtol=sc.GRAD_RTOL, atol=sc.GRAD_ATOL * np.abs(want).max())
    if phase2:
        gc = sum(co[k] * t["g"][k][2] for k in ("rec", "sm", "con", "ws"))
        np.testing.assert_allclose(dcam, gc, rtol=sc.GRAD_RTOL, atol=sc.GRAD_ATOL * np.abs(gc).max())


def _fit(case, lossconfig, iters, log_every, hook=None, monkeypatch=None, c_loop=True, data=None, **kw):
    """One FittingOP.fitting of mode 'global' -> (results and log as arrays, the kernel forms its launches took)"""
    forms = ctypes.create_string_buffer(8192)
    monkeypatch.setenv("FDCAP_C_LOOP", "1" if c_loop else "0")
    if hook is not None:
        orig = FittingOP.init

        def init(self, x):
            r = orig(self, x)
            hook(self)
            return r
        monkeypatch.setattr(FittingOP, "init", init)
    fop = make_fop(case, lossconfig, iters)
    try:
        capi.check(fop.ctx.lib.fdcap_debug_kernel_forms(forms, len(forms), 1), "kernel_forms")
        clip = sc.make_case(*_case(case))[2]
        body, scale, cam = fop.fitting(torch.tensor(clip.body_params if data is None else data).cuda(), "global", log_every=log_every, **kw)
        torch.cuda.synchronize()
        capi.check(fop.ctx.lib.fdcap_debug_kernel_forms(forms, len(forms), 0), "kernel_forms")
        out = {"body": body.cpu().numpy(), "scale": np.float32(scale), "cam": cam.cpu().numpy(), "rows": fop.body_rotation_rec.cpu().numpy()}
        if log_every:
            for k, v in dataclasses.asdict(fop.log).items():
                out["log_" + k] = np.asarray(v, dtype=np.float64)
    finally:
        fop.close()
        if hook is not None:
            monkeypatch.setattr(FittingOP, "init", orig)
    return out, forms.value.decode().split(";")


def _same_bytes(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_off_means_untouched(monkeypatch):
    """Check 4: 12 iterations across the phase switch with log_every = 1 -- a fit that never calls fdcap_opt_set_reproj, one that calls
    it with weight 0, one that calls it with params = NULL after a non-zero call: results and history byte-equal, the same forms."""
    case = rs.CASES[0]
    kp = torch.tensor(rs.make_keypoints(case)).cuda()

    def call(fop, par):
        capi.check(fop.ctx.lib.fdcap_opt_set_reproj(fop.ctx.handle, None if par is None else ctypes.byref(par), capi.dptr(kp), capi.current_stream()),
                   "fdcap_opt_set_reproj")

    def weight0(fop):
        call(fop, capi.ReprojParams(*rs.INTRINSICS, rs.RHO, 0.0))

    def on_then_null(fop):
        call(fop, capi.ReprojParams(*rs.INTRINSICS, rs.RHO, 0.5))
        call(fop, None)

    plain, f0 = _fit(case, {}, 12, 1, None, monkeypatch)
    for hook in (weight0, on_then_null):
        got, f1 = _fit(case, {}, 12, 1, hook, monkeypatch)
        _same_bytes(plain, got)
        assert f1 == f0
    assert "pose_bwd_reproj_kernel" not in f0 and plain["log_reproj"].size == 0 and len(plain["log_total"]) == 12
    # ... and with keypoints handed to a fit whose weight is 0
    got, f1 = _fit(case, {"weight_reproj": 0}, 12, 1, None, monkeypatch, keypoints=rs.make_keypoints(case), intrinsics=rs.INTRINSICS, rho=rs.RHO)
    _same_bytes(plain, got)
    assert f1 == f0


@pytest.mark.parametrize("log_every", [0, 1, 5])
def test_one_loop_gives_the_bits_of_the_single_calls(log_every, monkeypatch):
    """Check 5: with the term on, fdcap_opt_run over 12 iterations equals the per-iteration calls bit for bit -- results and history,
    slot 6 included -- and a second run gives the same bits."""
    case = rs.CASES[0]
    kw = dict(keypoints=rs.make_keypoints(case), intrinsics=rs.INTRINSICS, rho=rs.RHO)
    run, forms = _fit(case, {"weight_reproj": rs.WEIGHT}, 12, log_every, None, monkeypatch, c_loop=True, **kw)
    again, _ = _fit(case, {"weight_reproj": rs.WEIGHT}, 12, log_every, None, monkeypatch, c_loop=True, **kw)
    calls, _ = _fit(case, {"weight_reproj": rs.WEIGHT}, 12, log_every, None, monkeypatch, c_loop=False, **kw)
    _same_bytes(run, again)
    _same_bytes(run, calls)
    assert "pose_bwd_reproj_kernel" in forms
    if log_every:
        assert len(run["log_reproj"]) == len(run["log_total"]) > 0 and np.all(run["log_reproj"] > 0)
    off, _ = _fit(case, {}, 12, log_every, None, monkeypatch)
    assert not np.array_equal(off["body"], run["body"])


@pytest.mark.parametrize("phase2", [False, True])
@pytest.mark.parametrize("case", [rs.CASES[0], rs.CASES[4], NO_SCENE], ids=_ids)
def test_the_step_consumes_the_gradient(case, phase2):
    """Check 6, first part: the term alone, one iteration.  Adam's first step is lr g / (|g| + 1e-8): every column whose |g64| exceeds
    its block's bar moves against sign(g64), the cam_t columns included; lh, rh, `scale` and camera_ext do not move (nor does a row
    without detections).  The size of the step: "within 1e-3 of lr" holds as written only where 1e-8 / |g| < 1e-3 -- the betas block
    has live columns down to |g| ~ 1e-7, whose step is 0.9 lr by Adam's own formula (first GPU run: 9.0e-6 = 1.8e-3 lr off lr in
    betas, every other block inside) -- so each column is held to the interval Adam's formula gives for a gradient within the
    block's bar of g64, lr (|g| -+ bar) / (|g| -+ bar + 1e-8), widened by 1e-3 lr; where |g| > 1e-4 that is the issue's
    "lr within 1e-3 lr", asserted as such."""
    it = rs.isolated(_case(case))
    lr = 0.005
    with pytest.MonkeyPatch.context() as mp:
        for name in ("PHASE1_SMOOTH", "PHASE2_SMOOTH", "PHASE2_WORLD"):
            mp.setattr(fit_mod, name, 0.0)
        fop = make_fop(case, {"weight_loss_rec": 0.0, "weight_contact": 0.0})
        try:
            st = at_start(fop, case)
            set_reproj(fop, case)
            n = fop.num_body
            cam0, scale0 = fop._rows_cam[2:2 + n].cpu().numpy().copy(), fop._scale.cpu().numpy().copy()
            lib, h, P = fop.ctx.lib, fop.ctx.handle, (0 if phase2 else BIG)
            capi.check(lib.fdcap_opt_backward(h, 0, P, 0, capi.current_stream()), "fdcap_opt_backward")
            capi.check(lib.fdcap_opt_step(h, 0, P, capi.current_stream()), "fdcap_opt_step")
            torch.cuda.synchronize()
            rows1 = fop._rows_x[2:2 + n].cpu().numpy().astype(np.float64)
            cam1, scale1 = fop._rows_cam[2:2 + n].cpu().numpy(), fop._scale.cpu().numpy()
        finally:
            fop.close()
    d = rows1 - st["rows"].astype(np.float64)
    moved = 0
    for k, sl in gb.ROW_BLOCKS.items():
        g = it["g64"][k]
        live = np.abs(g) > it["bar"][k]
        if k in ("lh", "rh"):
            assert not live.any() and np.all(d[:, sl] == 0), k
            continue
        assert live.any(), k
        # the size of the step a gradient within its bar of g64 gives: lr a / (a + 1e-8) grows with a = |g|
        step = lambda a: lr * a / (a + 1e-8)
        lo, hi = step(np.abs(g) - it["bar"][k]) - 1e-3 * lr, step(np.abs(g) + it["bar"][k]) + 1e-3 * lr
        size = -np.sign(g) * d[:, sl]
        out = np.maximum(lo - size, size - hi)[live]
        print(f"{_ids(case)} {k}: {int(live.sum())} live columns, step / lr in {size[live].min() / lr:.6f} .. {size[live].max() / lr:.6f}, "
              f"worst distance from the interval {out.max() / lr:.3g} lr")
        assert out.max() <= 0, (k, out.max())
        big = live & (np.abs(g) > 1e-4)                         # (there 1e-8 / |g| < 1e-4: the step is lr within 1e-3 lr, whatever the bar)
        assert np.all(np.abs(size - lr)[big] <= 1e-3 * lr), k
        moved += int(live.sum())
    assert moved > 0 and np.array_equal(cam1, cam0) and np.array_equal(scale1, scale0)
    if n >= 4:
        assert np.all(d[rs.EMPTY_FRAME] == 0)


def test_comparative_fit(monkeypatch):
    """Check 6, second part: n = 12, 40 iterations, default weights, the data displaced from the ground truth by the perturbation: the
    mean pixel error (fp64 twin, on the returned rows) is lower with the term than without it, and lower than on the rows the fit
    starts from (init()'s)."""
    from oracle import rotrepr
    from oracle.fitting import find_outliers_and_sources
    t, kp = rs.twin(FIT_CASE), rs.make_keypoints(FIT_CASE)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(rs.fit75(FIT_CASE), dtype=torch.float64)).detach().float()
    idx1, pos = find_outliers_and_sources(x78)
    start = x78.clone()
    start[idx1] = x78[pos]
    e_start = t.pixel_error(start.numpy(), kp)
    off, _ = _fit(FIT_CASE, {}, FIT_ITERS, 0, None, monkeypatch, data=rs.fit75(FIT_CASE))
    on, _ = _fit(FIT_CASE, {"weight_reproj": FIT_WEIGHT}, FIT_ITERS, 0, None, monkeypatch, data=rs.fit75(FIT_CASE), keypoints=kp,
                 intrinsics=rs.INTRINSICS, rho=rs.RHO)
    e_off, e_on = t.pixel_error(off["rows"], kp), t.pixel_error(on["rows"], kp)
    print(f"mean pixel error: start {e_start:.3f}, term off {e_off:.3f}, term on {e_on:.3f}")
    assert e_on < e_off and e_on < e_start


# ---- sharded: two ranks on one GPU (gloo), each with its own keypoint rows -------------------------------------------------------
SH_CASE, SH_ITERS = (14, 300, 800, 20, 0), 10


def _sharded_fit(group):
    bm, vp, clip, scene, vid, n = sc.make_case(*SH_CASE)
    fop = FittingOP({"num_iter": SH_ITERS}, {"weight_reproj": rs.WEIGHT}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                    camera_ext=read_camerapose(clip.camerapose_lines), group=group)
    body, scale, cam = fop.fitting(torch.tensor(rs.ground_truth(SH_CASE)).cuda(), "global", log_every=1, keypoints=rs.make_keypoints(SH_CASE),
                                   intrinsics=rs.INTRINSICS, rho=rs.RHO)
    out = (fop.shard.frame0, body.cpu().numpy(), float(scale), cam.cpu().numpy(), np.array(fop.log.total), np.array(fop.log.reproj))
    fop.close()
    return out


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank,) + _sharded_fit(dist.group.WORLD))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_sharded_run_matches_single_rank():
    """Check 7: n = 14 over two ranks against the one-rank fit at the bars of tests/test_gpu_sharded.py
    test_sharded_gpu_run_matches_single_rank: atol 5e-6 for rows and camera, rtol 2e-6 for the summed history, the term's included."""
    import torch.multiprocessing as mp
    from fdcap_amd.dist import FrameShard
    from tests.shared_gpu import retry_on_shared_gpu_glitch
    ref = _sharded_fit(None)
    world = 2

    def check():
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        res = sorted(q.get(timeout=600) for _ in range(world))
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
        assert [r[1] for r in res] == [FrameShard(SH_CASE[0], None, rank=i, world=world).frame0 for i in range(world)]
        np.testing.assert_allclose(np.concatenate([r[2] for r in res]), ref[1], rtol=0, atol=5e-6)
        np.testing.assert_allclose(np.concatenate([r[4] for r in res]), ref[3], rtol=0, atol=5e-6)
        for r in res:
            assert abs(r[3] - ref[2]) < 2e-6
            np.testing.assert_allclose(r[5], ref[4], rtol=2e-6)
            np.testing.assert_allclose(r[6], ref[5], rtol=2e-6)
            assert len(r[6]) == SH_ITERS and np.all(r[6] > 0)

    retry_on_shared_gpu_glitch(check)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_term_as_it_was():
    """Check 8: every FDCAP_E_ARG / FDCAP_E_STATE case of fdcap.h; after a refused call the term's state is what it was (the gradient
    of the next backward says so)."""
    case = rs.CASES[1]
    n = case[0]
    E_ARG, E_STATE = -1, -2
    nan, inf = float("nan"), float("inf")
    kp = torch.tensor(rs.make_keypoints(case)).cuda()
    st = capi.current_stream()
    fop = make_fop(case, {})
    try:
        lib, h = fop.ctx.lib, fop.ctx.handle
        good = capi.ReprojParams(*rs.INTRINSICS, rs.RHO, rs.WEIGHT)
        assert lib.fdcap_opt_set_reproj(h, ctypes.byref(good), capi.dptr(kp), st) == E_STATE          # no optimiser
        at_start(fop, case)
        off = backward(fop, 5, BIG, 0)[0]

        def refused(par, kp_d=kp):
            return lib.fdcap_opt_set_reproj(h, ctypes.byref(par), capi.dptr(kp_d) if kp_d is not None else None, st)

        bad = [capi.ReprojParams(v, 673.0, 640.0, 360.0, rs.RHO, rs.WEIGHT) for v in (0.0, -692.0, nan, inf)]
        bad += [capi.ReprojParams(692.0, v, 640.0, 360.0, rs.RHO, rs.WEIGHT) for v in (0.0, -673.0, nan, inf)]
        bad += [capi.ReprojParams(692.0, 673.0, 640.0, 360.0, v, rs.WEIGHT) for v in (0.0, -100.0, nan, inf)]
        bad += [capi.ReprojParams(692.0, 673.0, 640.0, 360.0, rs.RHO, v) for v in (-1e-3, nan, inf)]
        for par in bad:
            assert refused(par) == E_ARG
        assert refused(good, None) == E_ARG                      # kp_d NULL with a non-zero weight
        assert backward(fop, 5, BIG, 0)[0].tobytes() == off.tobytes()          # still off
        assert refused(good) == 0
        on = backward(fop, 5, BIG, 0)[0]
        assert on.tobytes() != off.tobytes()
        for par in bad:
            assert refused(par) == E_ARG
        assert refused(good, None) == E_ARG
        assert backward(fop, 5, BIG, 0)[0].tobytes() == on.tobytes()           # still on, the same keypoints and parameters
        # while the term is on: mode 'local''s second loop and the DCT calls
        w = torch.full((n,), 0.5, device="cuda")
        D = np.ascontiguousarray(np.ones((4, 2), np.float32))
        c0 = torch.zeros((n // 4) * 69 * 2, device="cuda")
        hist = torch.zeros(4, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
        nl = ctypes.c_int32(0)
        assert lib.fdcap_opt_run_local2(h, 1, 0, 1, 10, 0, capi.dptr(w), capi.dptr(hist), 4, 0, ctypes.byref(nl), st) == E_STATE
        assert lib.fdcap_opt_backward_local2(h, capi.dptr(w), 1, st) == E_STATE
        assert lib.fdcap_opt_step_x(h, 1, st) == E_STATE
        assert lib.fdcap_opt_set_dct(h, D.ctypes.data_as(ctypes.c_void_p), 4, 2, capi.dptr(c0), st) == E_STATE
        assert lib.fdcap_opt_set_dct_clips(h, D.ctypes.data_as(ctypes.c_void_p), 4, 2, capi.dptr(c0), st) == E_STATE
        assert lib.fdcap_opt_dct_fit(h, 1, 0, 10.0, None, 1, st) == E_STATE
        assert lib.fdcap_opt_backward_dct(h, 1e-4, 0.5, 0.1, 0, st) == E_STATE
        assert lib.fdcap_opt_run_dct(h, 0, 1, 10, 10.0, 1e-4, 0.5, 0.1, 0, None, capi.dptr(hist), 4, 0, ctypes.byref(nl), st) == E_STATE
        assert backward(fop, 5, BIG, 0)[0].tobytes() == on.tobytes()
        # a DCT term set up: the term cannot be switched on
        capi.check(lib.fdcap_opt_set_reproj(h, None, None, st), "fdcap_opt_set_reproj")
        capi.check(lib.fdcap_opt_set_dct(h, D.ctypes.data_as(ctypes.c_void_p), 4, 2, capi.dptr(c0), st), "fdcap_opt_set_dct")
        assert refused(good) == E_STATE
        torch.cuda.synchronize()
    finally:
        fop.close()
    # a batch of clips
    bm, vp, clip, scene, vid, _ = sc.make_case(*case)
    f = ClipBatchFitter({"num_iter": 1}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    try:
        f.fit([(clip.body_params, read_camerapose(clip.camerapose_lines))] * 2, scene)
        assert f.ctx.lib.fdcap_opt_set_reproj(f.ctx.handle, ctypes.byref(good), capi.dptr(torch.cat([kp, kp])), st) == E_STATE
    finally:
        f.close()


# ---- the command line, end to end -------------------------------------------------------------------------------------------------
def test_cli_end_to_end(tmp_path, monkeypatch, capsys):
    """Check 9: a synthetic clip with OpenPose-shaped JSON written here: the output files exist and the logged loss_reproj of the last
    iteration is below that of the first."""
    import re
    from fdcap_amd import assets, cli, innerfit, io
    case = rs.CASES[0]
    bm, vp, clip, scene, vid, n = sc.make_case(*case)
    monkeypatch.setattr(assets, "load_smplx_npz", lambda *a, **k: bm)
    monkeypatch.setattr(assets, "load_vposer_snapshot", lambda *a, **k: vp)
    monkeypatch.setattr(io, "read_contact_ids", lambda folder, parts: vid[:len(vid) // 2] if parts[0] == "L_Leg" else vid[len(vid) // 2:])
    root, name = tmp_path / "scenes", "video-0"
    os.makedirs(root / name)
    io.write_ply_points(str(root / name / "meshed-poisson.ply"), scene)
    with open(root / name / "camerapose.txt", "w") as fh:
        fh.write("\n".join(clip.camerapose_lines) + "\n")
    bp = str(tmp_path / "bodies" / name) + "/"
    io.write_body_gen(rs.fit75(case), bp)
    kp23 = rs.make_keypoints(case)
    kdir = tmp_path / "openpose"
    os.makedirs(kdir)
    for i in range(n):
        body25 = np.zeros((25, 3), np.float32)
        for k, j in enumerate(innerfit.OPENPOSE_BODY25):
            if j < 23 and kp23[i, j, 2] != 0:
                body25[k] = kp23[i, j]
        with open(kdir / f"{name}_{i:012d}_keypoints.json", "w") as fh:
            json.dump({"version": 1.3, "people": [{"pose_keypoints_2d": [float(v) for v in body25.reshape(-1)]}]}, fh)
    out = str(tmp_path / "fit")
    fx, fy, cx, cy = rs.INTRINSICS
    assert cli.main([bp, out, "global", "--scene-root", str(root), "--num-iter", "20", "--log-every", "1", "--keypoints", str(kdir),
                     "--weight-reproj", str(FIT_WEIGHT), "--intrinsics", str(fx), str(fy), str(cx), str(cy), "--rho", str(rs.RHO)]) == 0
    assert sorted(os.listdir(out)) == [f"body_gen_{i:06d}.pkl" for i in range(n)]
    vals = [float(m) for m in re.findall(r"loss_reproj=([0-9.eE+-]+)", capsys.readouterr().out)]
    assert len(vals) == 20 and vals[-1] < vals[0], vals
