"""The inner fit's free jaw and bending prior, the parts that need no GPU: the host-callable arithmetic of csrc/fdc_keypoints.h
(jaw_forward, jaw_backward) and csrc/fdc_fit2d.h (jaw_grad, fit2d_bend_term, fit2d_bend_check), compiled by plain g++
(tests/face_cpu/face_check.cpp), against fp64 autograd of the formulas and of oracle/tgm.py; the leaf argument on the synthetic body;
and, with the twin tests/face_spec.py alone, that a gradient with any one piece of the jaw's chain or the bending prior missing
leaves the bars tests/test_gpu_face.py holds the kernels to."""
import importlib
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

from oracle import rotrepr, tgm
from oracle.smplx import batch_rodrigues
from tests.face_spec import MUTANTS, FaceSpec
from tests.keypoint_spec import COLUMN_BLOCKS, KeypointSpec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
synth = importlib.import_module("fdcap_amd.synth")
fio = importlib.import_module("fdcap_amd.io")
innerfit = importlib.import_module("fdcap_amd.innerfit")
STAGE = (1.0, 4.78, 5.0, 4.78)
W_JAW, W_BEND = (47.8, 478.0, 478.0), 3.17 * 4.78


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "face_check")
    src = os.path.join(ROOT, "tests", "face_cpu", "face_check.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", out, src])
    return out


def _run(exe, tmp_path, mode, tokens):
    fn = os.path.join(tmp_path, "in.txt")
    with open(fn, "w") as f:
        f.write(" ".join(t if isinstance(t, str) else repr(float(t)) for t in tokens))
    out = {}
    for ln in subprocess.run([exe, mode, fn], check=True, capture_output=True, text=True).stdout.splitlines():
        name, *vals = ln.split()
        out[name] = np.array([float(v) for v in vals])
    return out


def _f32(a):
    return np.asarray(a, dtype=np.float32)


# ---- the jaw's arithmetic -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle", [0.0, 1e-4, 0.3, 1.2])
def test_jaw_forward_and_backward_match_fp64_autograd_of_the_formulas(exe, tmp_path, angle):
    rng = np.random.Generator(np.random.PCG64(int(angle * 1e4) + 5))
    axis = rng.standard_normal(3)
    w = _f32(angle * axis / np.linalg.norm(axis))
    J = _f32(rng.standard_normal(3) * 0.3)
    RA = rotrepr.aa2matrot(torch.tensor(rng.standard_normal((1, 3)), dtype=torch.float64))[0].numpy()
    A = _f32(np.concatenate([RA, rng.standard_normal((3, 1))], 1))
    dAp, gP = _f32(rng.standard_normal((3, 4))), _f32(rng.standard_normal(9))
    got = _run(exe, tmp_path, "jaw", [*w, *J, *A.reshape(-1), *dAp.reshape(-1), *gP, *W_JAW])

    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    wt, Jt, At = t(w), t(J), t(A)
    Rw = batch_rodrigues(wt[None])[0]
    Rw_leaf = Rw.detach().clone().requires_grad_(True)

    def transform(Rw_):
        return torch.cat([At[:, :3] @ Rw_, (At[:, 3] + At[:, :3] @ ((torch.eye(3, dtype=torch.float64) - Rw_) @ Jt))[:, None]], 1)
    Ap = transform(Rw)
    skin = (torch.tensor(dAp, dtype=torch.float64) * Ap).sum()
    full = skin + (torch.tensor(gP, dtype=torch.float64) * (Rw - torch.eye(3, dtype=torch.float64)).reshape(-1)).sum() \
        + ((torch.tensor(W_JAW, dtype=torch.float64) * wt) ** 2).sum()
    g_w, = torch.autograd.grad(full, wt, retain_graph=True)
    g_A, g_J = torch.autograd.grad(skin, (At, Jt))
    g_Rw, = torch.autograd.grad((torch.tensor(dAp, dtype=torch.float64) * transform(Rw_leaf)).sum(), Rw_leaf)

    def close(name, want, scale=None):
        want = np.asarray(want, dtype=np.float64).reshape(-1)
        bar = 2e-6 * max(float(np.abs(want).max()) if scale is None else scale, 1.0)
        err = float(np.abs(got[name] - want).max())
        print(f"|w| {angle}: {name} max|err| {err:.3e} bar {bar:.3e}")
        assert err <= bar, (name, err, bar)
    close("A", Ap.detach().numpy())
    close("pf9", (Rw - torch.eye(3, dtype=torch.float64)).detach().numpy())
    close("dRw", g_Rw.numpy())
    close("dA22", g_A.numpy())
    close("dJ22", g_J.numpy(), scale=float(np.abs(dAp).max()))
    # (Rodrigues' backward divides by the angle: its error is relative to the gradient's own size, which the prior's weights set)
    close("grad", g_w.numpy())
    if angle == 0.0:                                         # the fixed model: A' is A bit for bit, nothing reaches J22 or the block
        assert np.array_equal(_f32(got["A"]), A.reshape(-1)) and np.all(got["dJ22"] == 0) and np.all(got["pf9"] == 0)
        assert np.array_equal(_f32(got["dA22"]).reshape(3, 4), dAp)


# ---- the bending term ------------------------------------------------------------------------------------------------------------------
def _branch(R):
    """the quaternion branch oracle/tgm.py's rotmat -> quaternion selects for R, and the sign of its cosine"""
    rt = R.T
    if rt[2, 2] < 1e-6:
        b = 0 if rt[0, 0] > rt[1, 1] else 1
    else:
        b = 2 if rt[0, 0] < -rt[1, 1] else 3
    qw = [rt[1, 2] - rt[2, 1], rt[2, 0] - rt[0, 2], rt[0, 1] - rt[1, 0], 1.0][b]
    return b, qw < 0


def test_bending_term_matches_fp64_autograd_of_the_oracles_log_map_in_every_branch(exe, tmp_path):
    rng = np.random.Generator(np.random.PCG64(9))
    aas = [0.4 * rng.standard_normal(3) for _ in range(4)]
    for ax in range(3):                                      # about x, y, z by +-2.9 rad: the three large-angle branches, both signs
        for sgn in (1.0, -1.0):
            v = 0.05 * rng.standard_normal(3)
            v[ax] = 2.9 * sgn
            aas.append(v)
    Rs = rotrepr.aa2matrot(torch.tensor(np.array(aas), dtype=torch.float64)).numpy()
    seen = {_branch(R) for R in Rs}
    assert {b for b, _ in seen} == {0, 1, 2, 3} and all((b, s) in seen for b in (0, 1, 2) for s in (False, True)), seen
    items, want = [], []
    for k, R in enumerate(Rs):
        axis, sign, w = k % 3, (1.0, -1.0)[k % 2], 1.5 + 0.1 * k
        R32 = _f32(R)
        items += [*R32.reshape(-1), float(axis), sign, w]
        Rt = torch.tensor(R32.astype(np.float64), requires_grad=True)
        aa = tgm.rotation_matrix_to_angle_axis(torch.nn.functional.pad(Rt[None], [0, 1]))[0]
        val = w * torch.exp(sign * aa[axis]) ** 2
        g, = torch.autograd.grad(val, Rt)
        want.append(np.concatenate([[float(val.detach())], g.numpy().reshape(-1)]))
    got = _run(exe, tmp_path, "bend", items)
    for k, wnt in enumerate(want):
        err, size = np.abs(got[f"item{k}"] - wnt), np.abs(wnt)
        print(f"rotation {k} branch {_branch(Rs[k])}: value rel err {err[0] / size[0]:.2e}, dR max|err| {err[1:].max():.2e} of {size[1:].max():.2e}")
        # fp32 at angles up to 2.9 rad, where exp(2 a) amplifies the angle's rounding by 2 and the log map divides by sin(theta / 2) ~ 1
        assert err[0] <= 2e-5 * size[0] and err[1:].max() <= 2e-5 * size[1:].max(), (k, err, size)


def test_bending_terms_are_validated(exe, tmp_path):
    res = lambda w, n, j, a, s: int(_run(exe, tmp_path, "terms", [w, str(n), *[str(v) for v in j], *[str(v) for v in a], *s])["result"][0])
    assert res(1.0, 4, [18, 19, 4, 5], [1, 1, 0, 0], [1, -1, -1, -1]) == 0 and res(0.0, 0, [], [], []) == 0
    assert res(1.0, 8, [1] * 8, [2] * 8, [1.0] * 8) == 0 and res(1.0, 9, [1] * 9, [2] * 9, [1.0] * 9) == -1
    assert res(1.0, 1, [0], [0], [1.0]) == -1 and res(1.0, 1, [22], [0], [1.0]) == -1 and res(1.0, 1, [21], [0], [1.0]) == 0
    assert res(1.0, 1, [4], [3], [1.0]) == -1 and res(1.0, 1, [4], [-1], [1.0]) == -1
    assert res(1.0, 1, [4], [0], ["nan"]) == -1 and res("inf", 1, [4], [0], [1.0]) == -1 and res(1.0, -1, [], [], []) == -1
    assert innerfit.MAX_BEND_TERMS == 8 and "#define FDCAP_MAX_BEND_TERMS 8" in open(os.path.join(ROOT, "include", "fdcap.h")).read()
    assert all(1 <= j <= 21 and 0 <= a <= 2 and s in (1.0, -1.0) for j, a, s in innerfit.DEFAULT_BEND_TERMS)
    assert np.asarray(innerfit.DEFAULT_JAW_PRIOR).shape == (len(innerfit.DEFAULT_STAGES), 3)


# ---- the leaf argument, and the twin ------------------------------------------------------------------------------------------------------
def _twin_case(n=4, lbs_nnz=4):
    bm, vp = synth.make_body_model(240, seed=7, lbs_nnz=lbs_nnz), synth.make_vposer(seed=8)
    jv = np.flatnonzero(np.asarray(bm.lbs_weights)[:, 22] > 0)
    assert len(jv) >= 8
    joint = [3, 15, 22, 40] + [-1] * 11
    tri = [(0, 0, 0)] * 4 + [(int(v),) * 3 for v in jv[:8]] + [(int(jv[0]), int(jv[3]), int(jv[5])), (int(jv[0]),) * 3, (5, 5, 5)]
    bary = [(0, 0, 0)] * 4 + [(1, 0, 0)] * 8 + [(0.5, 0.3, 0.2), (1, 0, 0), (1, 0, 0)]
    clip = synth.make_clip(n, seed=9, num_outliers=0)
    rng = np.random.Generator(np.random.PCG64(10))
    gt = clip.body_params.astype(np.float32).copy()
    gt[:, 72:75] = np.array([0.1, -0.2, 3.5], np.float32)
    x = rotrepr.convert_to_6D_rot(torch.tensor(gt, dtype=torch.float64)).numpy().astype(np.float32)
    jaw = rng.standard_normal((n, 3))
    jaw = (0.3 * jaw / np.linalg.norm(jaw, axis=1, keepdims=True)).astype(np.float32)
    spec = FaceSpec(bm, vp, joint, tri, bary)
    with torch.no_grad():
        uv = spec.project(spec.joints_cam(torch.tensor(x, dtype=torch.float64), torch.tensor(jaw, dtype=torch.float64))).numpy()
    kp = np.concatenate([uv + 3.0 * rng.standard_normal(uv.shape), rng.uniform(0.3, 1.0, (n, len(joint), 1))], -1).astype(np.float32)
    x[:, 19:51] += 0.3 * rng.standard_normal((n, 32)).astype(np.float32)
    return bm, vp, (joint, tri, bary), x, jaw, kp


@pytest.mark.parametrize("lbs_nnz", [4, 8])
def test_joint_22_is_a_leaf_and_the_leaf_form_is_the_model(lbs_nnz):
    assert synth.SMPLX_PARENTS[22] == 15 and 22 not in list(synth.SMPLX_PARENTS)
    bm, vp, m, x, jaw, kp = _twin_case(lbs_nnz=lbs_nnz)
    assert int((np.asarray(bm.lbs_weights)[:, 22] > 0).sum()) >= 8 and np.abs(np.asarray(bm.posedirs)[189:198]).max() > 0
    plain = FaceSpec(bm, vp, *m).grads(x, kp, STAGE, jaw, W_JAW, W_BEND)
    leaf = FaceSpec(bm, vp, *m, leaf=True).grads(x, kp, STAGE, jaw, W_JAW, W_BEND)
    for a, b in zip(plain, leaf):
        np.testing.assert_allclose(b, a, rtol=1e-11, atol=1e-11 * np.abs(a).max())
    # jaw = 0 and both priors off: KeypointSpec's values exactly
    ks = KeypointSpec(bm, vp, *m)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    d, p = ks.loss(xt, torch.tensor(kp, dtype=torch.float64), STAGE)
    (d + p).backward()
    s, g, _ = FaceSpec(bm, vp, *m).grads(x, kp, STAGE)
    assert s[0] == float(d.detach()) and s[1] == float(p.detach()) and np.array_equal(g, xt.grad.numpy())
    s0, g0, j0 = FaceSpec(bm, vp, *m).grads(x, kp, STAGE, np.zeros_like(jaw), W_JAW, 0.0)
    np.testing.assert_allclose(s0, s, rtol=1e-13)
    np.testing.assert_allclose(g0, g, rtol=1e-9, atol=1e-12 * np.abs(g).max())
    assert np.abs(j0).max() > 0                              # (the landmarks pull on a jaw that stands at zero)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_gradient_with_one_piece_missing_leaves_the_bars(mutant):
    """the bars of tests/test_gpu_face.py: rows 2e-3 relative + 2e-4 of the block's largest entry, the jaw block
    32 max(max|g32 - g64|, 2^-24 max|g64|) from the twin's two precisions"""
    bm, vp, m, x, jaw, kp = _twin_case()
    s64, g64, j64 = FaceSpec(bm, vp, *m).grads(x, kp, STAGE, jaw, W_JAW, W_BEND)
    _, g32, j32 = FaceSpec(bm, vp, *m, dtype=torch.float32).grads(x, kp, STAGE, jaw, W_JAW, W_BEND)
    sm, gm, jm = FaceSpec(bm, vp, *m, mutant=mutant).grads(x, kp, STAGE, jaw, W_JAW, W_BEND)
    np.testing.assert_allclose(sm, s64, rtol=1e-13)          # values unchanged: only the gradient lacks the piece
    jaw_bar = 32.0 * max(float(np.abs(j32 - j64).max()), 2.0 ** -24 * float(np.abs(j64).max()))
    out = {"jaw": float(np.abs(jm - j64).max()) / jaw_bar}
    for k, sl in COLUMN_BLOCKS.items():
        out[k] = float((np.abs(gm[:, sl] - g64[:, sl]) / (2e-3 * np.abs(g64[:, sl]) + 2e-4 * np.abs(g64[:, sl]).max())).max())
        assert np.all(np.abs(g32[:, sl] - g64[:, sl]) <= 2e-3 * np.abs(g64[:, sl]) + 2e-4 * np.abs(g64[:, sl]).max())     # (the fp32 twin itself passes)
    print(mutant, "max|err| / bar:", {k: round(v, 2) for k, v in out.items()})
    assert max(out.values()) > 2.0, out


def test_write_body_gen_adds_the_jaw_pose_key_and_the_loader_ignores_it(tmp_path):
    rows = np.random.Generator(np.random.PCG64(1)).standard_normal((3, 75)).astype(np.float32)
    jaw = np.arange(9, dtype=np.float32).reshape(3, 3)
    fio.write_body_gen(rows, str(tmp_path / "a"), jaw_pose=jaw)
    fio.write_body_gen(rows, str(tmp_path / "b"))
    rec = pickle.load(open(tmp_path / "a" / "results" / "frame_000001" / "000.pkl", "rb"))
    assert rec["jaw_pose"].shape == (1, 3) and np.array_equal(rec["jaw_pose"][0], jaw[1])
    assert "jaw_pose" not in pickle.load(open(tmp_path / "b" / "results" / "frame_000001" / "000.pkl", "rb"))
    assert np.array_equal(fio.load_body_gen(str(tmp_path / "a")), fio.load_body_gen(str(tmp_path / "b")))
    with pytest.raises(ValueError):
        fio.write_body_gen(rows, str(tmp_path / "c"), jaw_pose=jaw[:2])
