"""Mode 'local''s second loop (fdcap_opt_backward_local2, fdcap_opt_run_local2) and mode 'dct''s trajectory term alone
(fdcap_opt_backward_dct with w_rec = w_contact = 0), every column block of the gradient held to a bar of its own from the oracle's two
precisions: tests/local2_bars.py, tests/dct_bars.py (bar = 32 x max(fp32 oracle - fp64 oracle, 2^-24 max|g|) per block; no rtol;
tests/test_local2_bars_cpu.py shows on the CPU that a stride-loop tail left out, one denominator for both contact parts, the pair
weight w[i], the threshold dropped, the blend products' backward missing, ... leave these bars by a factor of 20 at least).

Second loop, one clip: cases A .. F of tests/local2_bars.py, each with the contact ids split at n_left = 1, nc // 2 and nc - 1 --
3 V = 255, 258, 1023, 1026 and 2100 around vert_smooth_kernel's 256 and 4 x 256 elements per trip, 3 nc = 258 and 900 for two and
four trips of foot_skate_kernel, clips of 3, 4 and 5 frames for the stencil's cuts, a duplicated triple of frames for sgn(0),
weights on both sides of 0.5 next to it.  A batch of clips (the clip_n / ctab branches): lengths (5, 3, 4) and (4, 4) on case C's
models, n_left = 1 and nc - 1, each clip against the bars of that clip alone.  The logged sums against the fp64 terms to 1e-5.
The DCT term: n = 60 (one window, the last workgroup ragged) and n = 125 (two windows and five tail rows), d rows and d scale
within their bars, the hand blocks and the tail rows exactly zero, the logged objective sum to 1e-5.

Every case runs with the default products (two fp16 planes) in this process and with the exact-fp32 products (FDCAP_GEMM_SPLIT3=0,
read once per process) in one child for all cases; both forms are held to the same bars.

Kernel forms of the second loop's full-mesh launches (fdcap_debug_kernel_forms, asserted per case; the same at every n_left):
  A, B                       skin_fwd_kernel; panel_gemm3_kernel; skin_bwd_kernel(one workgroup per frame)
  C, D, E, F, both batches   skin_fwd_kernel; panel_gemm3_kernel; panel_gemm3_ksw_kernel; skin_bwd_kernel(one workgroup per frame)

Worst measured max|err| / bar per block (MI355X), fp16 planes / exact fp32:
  one clip (A .. F x 3 splits)   transl 0.036 / 0.036   sixd 0.067 / 0.082   betas 0.050 / 0.104   latent 0.036 / 0.049
                                 lh 0.036 / 0.051   rh 0.056 / 0.100   camt 0.030 / 0.030
  batches (5 clips x 2 splits)   transl 0.040 / 0.040   sixd 0.062 / 0.079   betas 0.034 / 0.085   latent 0.036 / 0.048
                                 lh 0.035 / 0.050   rh 0.040 / 0.051   camt 0.005 / 0.005
  DCT term (n = 60, 125)         transl 0.023 / 0.027   sixd 0.029 / 0.032   betas 0.021 / 0.023   latent 0.022 / 0.029
                                 lh, rh 0 / 0 (exact zeros)   camt 0.022 / 0.028   dscale 0.005 / 0.020
No block landed outside its bar, and no kernel was changed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
import tests.dct_bars as db
import tests.gradient_bars as gb
import tests.local2_bars as lb
import tests.test_settings_cpu as sc
from fdcap_amd import capi, ops
from fdcap_amd.fitting import ClipBatchFitter, FittingOP

pytestmark = pytest.mark.gpu
LOG_RTOL = sc.LOG_RTOL
ITERS = 10
FORMS = ("fp16 planes", "exact fp32")
SLOTS = {"rec": 0, "loc": 2, "sm": 5, "cs": 6}


def _forms(lib, reset):
    buf = ctypes.create_string_buffer(4096)
    capi.check(lib.fdcap_debug_kernel_forms(buf, len(buf), 1 if reset else 0), "kernel_forms")
    return sorted(set(buf.value.decode().split(";")) - {""})


def second_loop_backward(name):
    """Case `name` on the device at the helper's state, one backward per n_left
    -> {n_left: (d rows [n, 78], losses [NUM_LOSSES], forms)}, and for `dup` the world vertices of the whole clip."""
    case, dup = lb.CASES[name]
    bm, vp, clip, scene, vid, n = lb.make_case(case)
    st = lb.start_state(case, dup)
    fop = FittingOP({"num_iter": 500}, {}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=st["cam"])
    out, verts = {}, None
    try:
        fop._mode = "local"
        idx1 = fop.init(torch.tensor(st["x78"]).cuda())
        assert np.array_equal(np.asarray(idx1), st["idx1"])
        fop._rows_x[2:2 + n] = torch.tensor(st["rows"]).cuda()
        # the oracle differentiates at exactly the state the device holds
        assert np.array_equal(fop._rows_x[2:2 + n].cpu().numpy(), st["rows"])
        assert np.array_equal(fop._rows_cam[2:2 + n].cpu().numpy(), st["cam"].reshape(n, 16))
        assert np.float32(fop._scale.cpu().numpy()[0]) == st["scale"]
        lib, h, stream = fop.ctx.lib, fop.ctx.handle, capi.current_stream()
        w = torch.tensor(st["w"]).cuda()
        for n_left in lb.n_lefts(case):
            _forms(lib, True)
            capi.check(lib.fdcap_opt_backward_local2(h, capi.dptr(w), n_left, stream), "local2")
            dx = torch.empty(n, 78, device="cuda")
            capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, stream), "grads")
            torch.cuda.synchronize()
            out[n_left] = (dx.cpu().numpy(), fop._losses.cpu().numpy().copy(), _forms(lib, False))
        assert np.array_equal(fop._rows_x[2:2 + n].cpu().numpy(), st["rows"]) and np.array_equal(w.cpu().numpy(), st["w"])
        if dup is not None:
            body75, scale, cam = fop._results(n, 1)
            verts = ops.world_mesh(fop.ctx, body75, scale, cam).cpu().numpy()
    finally:
        fop.close()
    return out, verts


def batch_backward(name):
    """Batch `name` through ClipBatchFitter.prepare(..., 'local') and fdcap_opt_run_local2 with the caller's weights (jj0 = 1,
    jj1 = 2, flags = 1: one logged backward, not stepped) -> {n_left: (d rows [total, 78], losses [clips, NUM_LOSSES], forms)}"""
    batch = lb.BATCHES[name]
    offs = lb.batch_offsets(batch)
    bm, vp, _, scene, vid, _ = lb.make_case(batch[0])
    states = [lb.start_state(c, None, o) for c, o in zip(batch, offs)]
    clips = [(lb.make_case(c)[2].body_params, s["cam"]) for c, s in zip(batch, states)]
    total = sum(c[0] for c in batch)
    rows = torch.tensor(np.concatenate([s["rows"] for s in states])).cuda()
    w_h = np.concatenate([s["w"] for s in states])
    assert np.array_equal(w_h, lb.weights(total))                # (the pattern runs on through the batch)
    fit = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    out = {}
    try:
        fit.set_scene(scene)
        fit.prepare(clips, "local")
        assert list(fit.clip_starts[:-1]) == list(offs)
        for k, s in enumerate(states):
            assert np.array_equal(np.asarray(fit.idx1[k]), s["idx1"]), k
        fit._rows_x[2:2 + total] = rows
        assert np.array_equal(fit._rows_cam[2:2 + total].cpu().numpy(), np.concatenate([s["cam"].reshape(-1, 16) for s in states]))
        assert all(np.float32(v) == states[0]["scale"] for v in fit._scale.cpu().numpy())
        lib, h, stream = fit.ctx.lib, fit.ctx.handle, capi.current_stream()
        w_d = torch.tensor(w_h).cuda()
        for n_left in lb.BATCH_N_LEFTS:
            hist = torch.zeros(1, len(batch), capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
            k_log = ctypes.c_int32(0)
            _forms(lib, True)
            capi.check(lib.fdcap_opt_run_local2(h, n_left, 1, 2, ITERS, 1, capi.dptr(w_d), capi.dptr(hist), 1, 1, ctypes.byref(k_log), stream), "run_local2")
            assert k_log.value == 1
            dx = torch.empty(total, 78, device="cuda")
            capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, stream), "grads")
            torch.cuda.synchronize()
            out[n_left] = (dx.cpu().numpy(), hist.cpu().numpy()[0], _forms(lib, False))
        assert torch.equal(fit._rows_x[2:2 + total], rows) and np.array_equal(w_d.cpu().numpy(), w_h)
    finally:
        fit.close()
    return out


def dct_backward(n):
    """A short mode-'dct' fit (38 steps of c_dct, one of the rows and `scale`), then the trajectory term alone
    -> the state the device holds, d rows, d scale and the logged sums."""
    bm, vp, clip, scene, vid, c0, D = db.make_case(n)
    from fdcap_amd.io import read_camerapose
    fop = FittingOP({}, {}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=read_camerapose(clip.camerapose_lines),
                    dct_mtx=D, c_dct_init=c0, dct_num_iter=40)
    try:
        fop.fitting(torch.tensor(clip.body_params).cuda(), "dct")
        lib, h, stream = fop.ctx.lib, fop.ctx.handle, capi.current_stream()
        capi.check(lib.fdcap_opt_backward_dct(h, 1.0, 0.0, 0.0, 1, stream), "backward_dct")
        dx = torch.empty(n, 78, device="cuda")
        capi.check(lib.fdcap_opt_get_grads(h, capi.dptr(dx), None, stream), "grads")
        torch.cuda.synchronize()
        state = {"rows": fop._rows_x[2:2 + n].cpu().numpy(), "scale": np.float32(fop._scale.cpu().numpy()[0]),
                 "cam": fop._rows_cam[2:2 + n].cpu().numpy(), "c_dct": fop.c_dct.cpu().numpy()}
        assert state["scale"] != np.float32(1.8) and not np.array_equal(state["c_dct"], c0)      # (the short fit moved both)
        return dict(state, dx=dx.cpu().numpy(), dscale=np.float64(fop._dscale.cpu().numpy()[0]), losses=fop._losses.cpu().numpy().copy())
    finally:
        fop.close()


_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import tests.local2_bars as lb
import tests.dct_bars as db
from tests.test_gpu_local2_bars import second_loop_backward, batch_backward, dct_backward
out = {}
for name in sorted(lb.CASES):
    res, verts = second_loop_backward(name)
    for n_left, (dx, losses, forms) in res.items():
        out["one/%%s/%%d/dx" %% (name, n_left)], out["one/%%s/%%d/losses" %% (name, n_left)] = dx, losses
    if verts is not None:
        out["one/%%s/verts" %% name] = verts
for name in sorted(lb.BATCHES):
    for n_left, (dx, losses, forms) in batch_backward(name).items():
        out["batch/%%s/%%d/dx" %% (name, n_left)], out["batch/%%s/%%d/losses" %% (name, n_left)] = dx, losses
for n in db.CASES:
    for k, v in dct_backward(n).items():
        out["dct/%%d/%%s" %% (n, k)] = v
np.savez(sys.argv[1], **out)
print("RESULT ok")
"""


@pytest.fixture(scope="module")
def exact_fp32(tmp_path_factory):
    """All cases in ONE child process with the exact-fp32 products -> {key: array}"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path_factory.mktemp("exact_fp32") / "local2.npz")
    p = subprocess.run([sys.executable, "-c", _CHILD % root, path], env=dict(os.environ, FDCAP_GEMM_SPLIT3="0"), capture_output=True, text=True,
                       timeout=600, cwd=root)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stderr[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _check_clip(case, dup, n_left, w_offset, dx, losses, label):
    """One clip's gradient against its bars, its four logged sums against the fp64 terms -> the blocks outside their bar"""
    ref = lb.reference(case, dup, n_left, w_offset)
    bad = gb.check(gb.blocks(rows=dx), ref["g64"], ref["bar"], 1.0, f"{label} {case} n_left {n_left}")
    got = lb.logged_terms(losses, case[0], case[1])
    for k, want in ref["terms"].items():
        assert losses[SLOTS[k]] > 0, k
        np.testing.assert_allclose(got[k], want, rtol=LOG_RTOL, err_msg=f"{label} {case} n_left {n_left} logged {k}")
    return bad


def _full_mesh_forms(forms):
    return [f for f in forms if f == "skin_fwd_kernel" or f.startswith("panel_gemm3") or f.startswith("skin_bwd")]


@pytest.mark.parametrize("name", sorted(lb.CASES))
def test_second_loop_gradient_within_its_per_block_bars(name, exact_fp32):
    """One clip, cases A .. F at n_left = 1, nc // 2 and nc - 1, both product forms: every block within its bar, the four logged
    sums to 1e-5, the full-mesh launches among the noted forms; case E: the three duplicated frames' world vertices bitwise equal."""
    case, dup = lb.CASES[name]
    res, verts = second_loop_backward(name)
    bad = {}
    for n_left, (dx, losses, forms) in res.items():
        print(name, "n_left", n_left, "forms:", "; ".join(_full_mesh_forms(forms)))
        assert "skin_fwd_kernel" in forms and any(f.startswith("panel_gemm3") for f in forms) and any(f.startswith("skin_bwd") for f in forms), forms
        for form, (g, l) in ((FORMS[0], (dx, losses)), (FORMS[1], (exact_fp32[f"one/{name}/{n_left}/dx"], exact_fp32[f"one/{name}/{n_left}/losses"]))):
            b = _check_clip(case, dup, n_left, 0, g, l, form)
            if b:
                bad[(form, n_left)] = b
    if dup is not None:
        i, j, k = dup
        for v in (verts, exact_fp32[f"one/{name}/verts"]):
            assert v.shape == (case[0], case[1], 3) and np.array_equal(v[i], v[j]) and np.array_equal(v[i], v[k])
            assert not np.array_equal(v[i], v[i - 1])
    assert not bad, f"blocks outside their bar {{block: (err / bar, bar, max|g|)}}: {bad}"


@pytest.mark.parametrize("name", sorted(lb.BATCHES))
def test_second_loop_gradient_of_a_batch_within_each_clips_bars(name, exact_fp32):
    """Lengths (5, 3, 4) through the clip table and (4, 4) through arithmetic on the one length, n_left = 1 and nc - 1, both product
    forms: each clip's rows of the gradient within the bars of that clip alone, its logged sums with its own denominators."""
    batch = lb.BATCHES[name]
    offs = lb.batch_offsets(batch)
    bad = {}
    for n_left, (dx, losses, forms) in batch_backward(name).items():
        print(name, "n_left", n_left, "forms:", "; ".join(_full_mesh_forms(forms)))
        assert "skin_fwd_kernel" in forms and any(f.startswith("panel_gemm3") for f in forms) and any(f.startswith("skin_bwd") for f in forms), forms
        for form, (g, l) in ((FORMS[0], (dx, losses)), (FORMS[1], (exact_fp32[f"batch/{name}/{n_left}/dx"], exact_fp32[f"batch/{name}/{n_left}/losses"]))):
            for k, (case, off) in enumerate(zip(batch, offs)):
                b = _check_clip(case, None, n_left, off, g[off:off + case[0]], l[k], f"{form} clip {k}")
                if b:
                    bad[(form, n_left, k)] = b
    assert not bad, f"blocks outside their bar {{block: (err / bar, bar, max|g|)}}: {bad}"


@pytest.mark.parametrize("n", db.CASES)
def test_dct_term_alone_within_its_per_block_bars(n, exact_fp32):
    """fdcap_opt_backward_dct(1, 0, 0) after a 40-iteration fit, both product forms, against the oracle at the state read back:
    every block of d rows and d scale within its bar, lh / rh and every tail row exactly zero, the logged objective sum to 1e-5."""
    bad = {}
    here = dct_backward(n)
    child = {k: exact_fp32[f"dct/{n}/{k}"] for k in here}
    W = n // db.T
    for form, r in ((FORMS[0], here), (FORMS[1], child)):
        ref = db.reference(n, r)
        got = gb.blocks(rows=r["dx"], dscale=float(r["dscale"]))
        b = gb.check(got, ref["g64"], ref["bar"], 1.0, f"{form} dct n = {n}")
        if b:
            bad[form] = b
        assert not got["lh"].any() and not got["rh"].any()
        assert not r["dx"][db.T * W:].any() and r["dx"][:db.T * W].any(axis=1).all()
        np.testing.assert_allclose(r["losses"][7] / (69 * W), ref["l_dct"], rtol=LOG_RTOL)
    assert not bad, f"blocks outside their bar {{block: (err / bar, bar, max|g|)}}: {bad}"
