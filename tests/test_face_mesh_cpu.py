"""The full mesh under a jaw pose and expression coefficients, the parts that need no GPU: the twin's two forms (tests/face_mesh_spec.py:
smplx with the two keys against the kernels' correction of the chain at jaw = 0, psi = 0) for full-mesh vertices, the 55 joints and every
gradient block; the host-callable per-frame arithmetic of csrc/fdc_face_mesh.h compiled by plain g++
(tests/face_mesh_cpu/face_mesh_check.cpp) against fp64 autograd of the correction's formulas; that a gradient with any one piece of the
correction missing leaves the bars tests/test_gpu_face_mesh.py holds the operators to; and io.load_body_face."""
import importlib
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import rotrepr
from oracle.smplx import batch_rodrigues
from tests import face_mesh_spec as fs
from tests import gradient_bars as gb
from tests.expression_spec import NEXPR, chain_correction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
synth = importlib.import_module("fdcap_amd.synth")
fio = importlib.import_module("fdcap_amd.io")
JAW = 22
# the blocks a mutant must leave (measured below by ratio and printed).  "prior" belongs to the inner fit's objective: the operators
# have no prior, so in them it must change nothing at all.
TARGETS = {"rot_addend": ("global_orient", "body_pose", "left_hand_pose", "right_hand_pose"), "parent_term": ("expression",),
           "jw": ("global_orient", "body_pose", "expression"), "pseudo_rows": ("expression",), "real_rows": ("expression",),
           "jaw_delta": ("expression",), "prior": (), fs.MESH_MUTANT: ("expression",)}


# ---- (a) the two forms of the twin ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("face", ["jaw", "psi", "both"])
@pytest.mark.parametrize("V,lbs_nnz", [(150, 4), (300, 12)])
def test_the_correction_form_is_the_direct_form_to_fp64_rounding(V, lbs_nnz, face):
    bm = synth.make_body_model(V, seed=0, lbs_nnz=lbs_nnz)
    inp, wv, wj = fs.make_inputs(3, V, seed=3)
    vd, jd, gd = fs.FaceMeshTwin(bm).run(inp, face, wv, wj)
    vc, jc, gc = fs.FaceMeshTwin(bm, correction=True).run(inp, face, wv, wj)
    v0, j0, _ = fs.FaceMeshTwin(bm).run(dict(inp, jaw_pose=0 * inp["jaw_pose"], expression=0 * inp["expression"]), face)
    print(f"V {V} lbs_nnz {lbs_nnz} {face}: the face moves a vertex by up to {np.abs(vd - v0).max() * 100:.2f} cm, a joint by {np.abs(jd - j0).max() * 1000:.2f} mm")
    assert np.abs(vd - v0).max() > 1e-3
    np.testing.assert_allclose(vc, vd, rtol=0, atol=1e-13)
    np.testing.assert_allclose(jc, jd, rtol=0, atol=1e-13)
    assert set(gc) == set(gd) == set(fs.INPUTS + fs.FACE[face])
    for k in gd:
        print(f"  {k}: max|direct - correction| {np.abs(gd[k] - gc[k]).max():.3e} of {np.abs(gd[k]).max():.3e}")
        np.testing.assert_allclose(gc[k], gd[k], rtol=1e-10, atol=1e-11 * np.abs(gd[k]).max())
        assert np.abs(gd[k]).max() > 0
    if face == "jaw":                                       # the jaw moves no joint
        assert np.array_equal(jd, j0)


# ---- (b) the host-callable arithmetic -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "face_mesh_check")
    src = os.path.join(ROOT, "tests", "face_mesh_cpu", "face_mesh_check.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", out, src])
    return out


def _run(exe, mode, path, arrays):
    with open(path, "w") as f:
        f.write(" ".join(repr(float(v)) for a in arrays for v in np.asarray(a).reshape(-1)))
    got = {}
    for ln in subprocess.run([exe, mode, path], check=True, capture_output=True, text=True).stdout.splitlines():
        name, *vals = ln.split()
        got[name] = np.array([float(v) for v in vals])
    return got


@pytest.mark.parametrize("face,with_gj,with_dap", [("jaw", False, True), ("psi", True, True), ("both", True, True), ("psi", True, False),
                                                    ("both", False, True)])
def test_the_frame_functions_match_fp64_autograd_of_the_correction(exe, tmp_path, face, with_gj, with_dap):
    rng = np.random.Generator(np.random.PCG64(60 + len(face) + 2 * with_gj + with_dap))
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    has_psi, has_jaw = face != "jaw", face != "psi"
    parents = np.asarray(synth.SMPLX_PARENTS, dtype=np.int64)
    R = rotrepr.aa2matrot(torch.tensor(rng.standard_normal((55, 3)), dtype=torch.float64)).numpy()
    A = f32(np.concatenate([R, rng.standard_normal((55, 3, 1))], 2))
    JE, Jt, Jd = f32(0.002 * rng.standard_normal((55, 3, NEXPR))), f32(rng.standard_normal((55, 3))), f32(0.02 * rng.standard_normal((55, 3, 10)))
    betas, psi = f32(0.5 * rng.standard_normal(10)), f32(1.5 * rng.standard_normal(NEXPR))
    jaw = rng.standard_normal(3)
    jaw = f32(0.3 * jaw / np.linalg.norm(jaw))
    dAp, gJ, dpv = f32(rng.standard_normal((55, 3, 4))), f32(rng.standard_normal((55, 3))), f32(rng.standard_normal(NEXPR))
    got = _run(exe, "frame", os.path.join(tmp_path, "in.txt"), ([has_psi, has_jaw, with_gj, with_dap], parents, JE, Jt, Jd, betas, psi, jaw, A, dAp, gJ, dpv))

    t = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=g)
    At, psit, jawt, betat = t(A, True), t(psi, True), t(jaw), t(betas, True)
    Rw = batch_rodrigues(jawt[None])[0].detach().requires_grad_(True)
    delta = torch.einsum("jkl,l->jk", t(JE), psit) if has_psi else torch.zeros(55, 3, dtype=torch.float64)
    dt, add = chain_correction(At[None, :, :, :3], delta[None], parents)
    tA = At[:, :, 3] + add[0]
    rot = At[:, :, :3]
    if has_jaw:
        J22 = t(Jt)[JAW] + torch.matmul(t(Jd)[JAW], betat) + delta[JAW]
        t22 = tA[JAW] + torch.matmul(rot[JAW], torch.matmul(torch.eye(3, dtype=torch.float64) - Rw, J22))
        rot = torch.cat([rot[:JAW], torch.matmul(rot[JAW], Rw)[None], rot[JAW + 1:]])
        tA = torch.cat([tA[:JAW], t22[None], tA[JAW + 1:]])
    Ap = torch.cat([rot, tA.unsqueeze(-1)], 2)
    val = (t(dAp) * Ap).sum() * (1.0 if with_dap else 0.0) + ((t(gJ) * dt[0]).sum() if with_gj else 0.0)
    if has_psi:
        val = val + (t(dpv) * psit).sum()
    g_A, g_psi, g_Rw, g_beta = torch.autograd.grad(val, (At, psit, Rw, betat), allow_unused=True)

    def close(name, want, size=None):
        want = np.asarray(want, dtype=np.float64).reshape(-1)
        bar = 4e-6 * max(float(np.abs(want).max()) if size is None else size, 1e-30)
        err = float(np.abs(got[name] - want).max())
        print(f"{face} gJ {with_gj} dAp {with_dap}: {name} max|err| {err:.3e} bar {bar:.3e}")
        assert err <= bar, (name, err, bar)
    close("A2", Ap.detach().numpy())
    close("dt", dt[0].detach().numpy(), size=float(delta.detach().abs().max()) * 12 or 1.0)
    close("dA", g_A.numpy(), size=float(np.abs(g_A.numpy()).max()) * 4)
    if has_psi:
        assert np.abs(g_psi.numpy()).max() > 0
        close("dpsi", g_psi.numpy(), size=float(np.abs(dpv).max() + np.abs(JE).max() * 55 * 3 * 20))
    else:
        assert np.all(got["dt"] == 0)
    if has_jaw:
        close("pf9", (Rw - torch.eye(3, dtype=torch.float64)).detach().numpy(), size=1.0)
        if with_dap:
            assert np.abs(g_Rw.numpy()).max() > 0 and np.abs(g_beta.numpy()).max() > 0
        close("R9", np.zeros(9) if g_Rw is None else g_Rw.numpy(), size=float(np.abs(dAp).max()) * 8)
        close("dbeta", np.zeros(10) if g_beta is None else g_beta.numpy(), size=float(np.abs(Jd).max() * np.abs(dAp).max() * 6))
    else:                                                    # the chain's own rotation and nothing of the jaw's
        assert np.array_equal(f32(got["A2"]).reshape(55, 3, 4)[:, :, :3], A[:, :, :3])
        assert np.all(got["R9"] == 0) and np.all(got["dbeta"] == 0)


@pytest.mark.parametrize("ncol", [450, 1024, 2331])          # two chunks with a ragged second one, four full chunks, ten chunks with a ragged last one
def test_the_two_reductions_frame_forms(exe, tmp_path, ncol):
    rng = np.random.Generator(np.random.PCG64(ncol))
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    E, psi, Voff, dV = f32(0.01 * rng.standard_normal((NEXPR, ncol))), f32(1.5 * rng.standard_normal(NEXPR)), f32(0.05 * rng.standard_normal(ncol)), f32(rng.standard_normal(ncol))
    got = _run(exe, "sums", os.path.join(tmp_path, "in.txt"), ([ncol], E, psi, Voff, dV))
    d = lambda a: np.asarray(a, dtype=np.float64)
    want_v, want_p = d(Voff) + d(psi) @ d(E), d(E) @ d(dV)
    ev = np.abs(got["Voff"] - want_v).max()
    ep = np.abs(got["dpsi_v"] - want_p).max()
    # the project's M = 32 times fp32's unit roundoff of the sum of magnitudes: a chain of n terms is bounded by n 2^-24 of it (n = 11 for an
    # offset; a chunk's 256 columns and the chunks for d psi) and sits near sqrt(n) 2^-24
    bar_v = 12 * 2.0 ** -24 * float((np.abs(d(Voff)) + np.abs(d(psi)) @ np.abs(d(E))).max())
    bar_p = 32 * 2.0 ** -24 * float((np.abs(d(E)) @ np.abs(d(dV))).max())
    print(f"ncol {ncol}: offsets max|err| {ev:.3e} bar {bar_v:.3e}; d psi max|err| {ep:.3e} bar {bar_p:.3e}")
    assert ev <= bar_v and ep <= bar_p


# ---- (c) every mutant leaves the GPU test's bars ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mutant_case():
    """(3, 777, 8): ten chunks of expr_dpsi_kernel's reduction; jaw and psi both given, upstream gradients on vertices and joints"""
    bm = synth.make_body_model(777, seed=0, lbs_nnz=8)
    inp, wv, wj = fs.make_inputs(3, 777, seed=3)
    return (bm, inp, wv, wj) + fs.bars_of(bm, inp, "both", wv, wj)


@pytest.mark.parametrize("mutant", fs.ALL_MUTANTS)
def test_a_gradient_with_one_piece_missing_leaves_the_bars_in_its_block(mutant_case, mutant):
    bm, inp, wv, wj, b64, b32, bar = mutant_case
    assert max(gb.ratios(b32, b64, bar).values()) <= 1.0     # (the fp32 twin itself passes)
    vm, jm, gm = fs.FaceMeshTwin(bm, mutant=mutant).run(inp, "both", wv, wj)
    assert np.abs(vm - b64["vertices"]).max() < 1e-12 and np.abs(jm - b64["joints"]).max() < 1e-12     # values unchanged
    r = gb.ratios(gm, {k: b64[k] for k in gm}, bar)
    print(mutant, "max|err| / bar:", {k: round(v, 2) for k, v in r.items()})
    for k in TARGETS[mutant]:
        assert r[k] > 2.0, (mutant, k, r[k])
    if not TARGETS[mutant]:
        assert max(r.values()) < 1e-3, r


# ---- (d) the result files -----------------------------------------------------------------------------------------------------------------------
def test_load_body_face_round_trips_write_body_gen(tmp_path):
    rng = np.random.Generator(np.random.PCG64(2))
    rows = rng.standard_normal((4, 75)).astype(np.float32)
    jaw, expr = rng.standard_normal((4, 3)).astype(np.float32), rng.standard_normal((4, 10)).astype(np.float32)
    fio.write_body_gen(rows, str(tmp_path / "both"), jaw_pose=jaw, expression=expr)
    fio.write_body_gen(rows, str(tmp_path / "jaw"), jaw_pose=jaw)
    fio.write_body_gen(rows, str(tmp_path / "none"))
    j, e = fio.load_body_face(str(tmp_path / "both"))
    assert j.dtype == np.float32 and e.dtype == np.float32 and np.array_equal(j, jaw) and np.array_equal(e, expr)
    j, e = fio.load_body_face(str(tmp_path / "jaw"))
    assert np.array_equal(j, jaw) and e is None
    assert fio.load_body_face(str(tmp_path / "none")) == (None, None)
    assert np.array_equal(fio.load_body_gen(str(tmp_path / "both")), rows)
    fio.write_body_gen(rows[:1], str(tmp_path / "jaw"))      # frame 0 rewritten without the key: three of four files have it
    with pytest.raises(ValueError):
        fio.load_body_face(str(tmp_path / "jaw"))
    with pytest.raises(FileNotFoundError):
        fio.load_body_face(str(tmp_path / "nothing"))
