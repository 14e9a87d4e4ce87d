"""Per-block gradient bars for mode 'dct''s trajectory term alone (cal_dctloss, global_optimization.py:232-246;
dct_joint_grad_kernel in csrc/fdc_dct.h and the joint chain behind it), from the oracle's own two precisions (no GPU needed).

tests/test_gpu_dct_smoother.py::test_dct_gradient_matches_autograd holds 0.7 dct + 0.5 rec + 0.1 contact to rtol 2e-3,
atol 2e-4 max|g| over the whole matrix at one shape; fdcap_opt_backward_dct takes the three weights directly, so the DCT term can
be had alone (w_rec = w_contact = 0) and held to the bars of tests/gradient_bars.py,

    bar_b = M * max( max|g32_b - g64_b| , 2^-24 max|g64_b| )        per block of d rows, and for d scale;  M = 32

g32 / g64: the oracle's autograd of cal_dctloss(joints) in fp32 / fp64 at the SAME fp32 state (rows, scale, camera_ext, c_dct) --
on the GPU the state read back from the device after a short fit, on the CPU cpu_state().  The term is smooth: no sign conditions.
The joints 0 .. 22 do not depend on the hand columns: the lh and rh blocks are exactly zero in both precisions, their bar is 0, and
gb.ratios then demands exact zeros.

CASES (the models of tests/test_gpu_dct_smoother.py _dct_case(n, 160, 900, seed=77)):
    n = 60     one window; 60 x 69 = 4140 elements: dct_joint_grad_kernel's last workgroup of 256 is ragged
    n = 125    two windows and 5 tail rows, which belong to no window and get no gradient

MUTANTS are alternative forms of cal_dctloss; tests/test_local2_bars_cpu.py shows that each leaves a bar by a factor of 20 where it
applies (`tail_window`: a clip with tail rows; `mean_69`: more than one window)."""
import functools

import numpy as np
import torch

import tests.gradient_bars as gb
import tests.test_settings_cpu as sc
from fdcap_amd import synth
from fdcap_amd.io import load_dct_base
from oracle import rotrepr
from oracle.fitting import FittingOracle, find_outliers_and_sources
from oracle.smplx import SMPLXOracle
from oracle.vposer import VPoserDecoder

CASES = (60, 125)
T = 60
MUTANTS = ("den", "basis_row", "tail_window", "mean_69")


@functools.lru_cache(maxsize=None)
def make_case(n):
    """tests/test_gpu_dct_smoother.py _dct_case(n, 160, 900, seed=77) -> bm, vp, clip, scene, vid, c0 [n // 60, 23, 3, 5], D [60, 5]"""
    seed = 77
    bm = synth.make_body_model(160, seed=seed)
    vp = synth.make_vposer(seed=seed + 1)
    clip = synth.make_clip(n, seed=seed + 2, num_outliers=2)
    scene = synth.make_scene(900, seed=seed + 3)
    left, right = synth.make_contact_ids(bm.v_template, per_part=8, seed=seed + 4)
    rng = np.random.Generator(np.random.PCG64(seed + 5))
    c0 = rng.standard_normal((n // T, 23, 3, 5)).astype(np.float32)
    return bm, vp, clip, scene, np.concatenate([left, right]), c0, load_dct_base(None)


def applies(mutant, n):
    return {"tail_window": n % T != 0, "mean_69": n // T > 1}.get(mutant, True)


def cpu_state(n):
    """A state of the kind the device holds, without a device: the fp32 start rows after init() + fp32(perturbation), scale
    fp32(1.8), camera_ext in fp32, the start coefficients."""
    from fdcap_amd.io import read_camerapose
    bm, vp, clip, scene, vid, c0, D = make_case(n)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(clip.body_params, dtype=torch.float64)).detach().float()
    idx1, pos = find_outliers_and_sources(x78)
    rows = x78.clone()
    if len(idx1) and len(pos):
        rows[idx1] = x78[pos]
    rows += sc.perturbation(n).float()
    return {"rows": rows.numpy(), "scale": np.float32(sc.DEFAULTS["scale_init"]), "cam": read_camerapose(clip.camerapose_lines), "c_dct": c0}


class _Residual(torch.autograd.Function):
    """e / (e + 1), e = r^2, with d / d r = 2 r / (e + 1)^power: power 2 is the derivative, power 1 the mutant `den`."""

    @staticmethod
    def forward(ctx, r, power):
        ctx.save_for_backward(r)
        ctx.power = power
        e = r * r
        return e / (e + 1.0)

    @staticmethod
    def backward(ctx, g):
        (r,) = ctx.saved_tensors
        return g * 2.0 * r / (r * r + 1.0) ** ctx.power, None


def dct_loss(f, joints, mutant=None):
    """FittingOracle.cal_dctloss, or one of MUTANTS (the same value where the form allows it)."""
    W = f.c_dct.shape[0]
    traj = joints[:T * W].reshape(W, T, 23, 3)
    D = torch.roll(f.dct_mtx, -1, 0) if mutant == "basis_row" else f.dct_mtx        # frame f takes basis row (f + 1) % T
    pred = torch.einsum("tc,kijc->ktij", D, f.c_dct)
    if mutant == "den":
        obj = _Residual.apply(traj - pred, 1)
    else:
        err = (traj - pred) ** 2
        obj = err / (err + 1.0)
    loss = torch.mean(torch.sum(obj, dim=1))
    if mutant == "tail_window":                                  # tail rows treated as frames of window W - 1
        tail = joints[T * W:]
        e = (tail - pred[W - 1, :tail.shape[0]]) ** 2
        extra = torch.sum(e / (e + 1.0)) / (69 * W)
        loss = loss + (extra - extra.detach())
    if mutant == "mean_69":                                      # the mean's denominator 69 W replaced by 69
        loss = loss * W - (loss * (W - 1)).detach()
    return loss


def _gradient(n, state, dtype, mutant=None):
    bm, vp, clip, scene, vid, c0, D = make_case(n)
    f = FittingOracle(SMPLXOracle(bm, dtype), VPoserDecoder.from_data(vp, dtype), scene, vid, clip.camerapose_lines, n, dtype=dtype,
                      dct_mtx=D, c_dct_init=np.asarray(state["c_dct"], dtype=np.float32), scale_init=float(np.float32(state["scale"])))
    f.body_rotation_rec.data = torch.tensor(np.asarray(state["rows"], dtype=np.float32)).to(dtype)
    f.camera_ext.data = torch.tensor(np.asarray(state["cam"], dtype=np.float32).reshape(n, 4, 4)).to(dtype)
    _, _, joints = f.forward_world()
    loss = dct_loss(f, joints, mutant)
    if mutant is None:
        assert torch.equal(loss.detach(), f.cal_dctloss(joints).detach())
    g_rows, g_scale = torch.autograd.grad(loss, (f.body_rotation_rec, f.scale))
    return gb.blocks(rows=g_rows.numpy(), dscale=float(g_scale)), float(loss.detach())


def reference(n, state):
    """state: {"rows" [n, 78], "scale", "cam" [n, 4, 4] or [n, 16], "c_dct" [W, 23, 3, 5]} in fp32, as the device holds it
    -> {"g64", "g32", "bar": {block: ...}, "l_dct": the fp64 value}: d cal_dctloss / d (rows, scale), unweighted."""
    g64, l64 = _gradient(n, state, torch.float64)
    g32, _ = _gradient(n, state, torch.float32)
    for k in ("lh", "rh"):
        assert not g64[k].any() and not g32[k].any(), k
    assert not g64["transl"][T * (n // T):].any() and np.abs(g64["transl"]).max() > 0
    return {"g64": g64, "g32": g32, "bar": gb.bars(g32, g64), "l_dct": l64}


def mutant_gradient(n, state, mutant):
    assert mutant in MUTANTS, mutant
    return _gradient(n, state, torch.float64, mutant)[0]
