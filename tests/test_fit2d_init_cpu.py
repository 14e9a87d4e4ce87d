"""The inner fit's start from keypoints alone, the parts that need no GPU: the host-callable arithmetic of csrc/fdc_fit2d_init.h
(depth guess, side-view test, the camera term and its set-up, the flip, the select rule, the settings' validation), compiled by plain
g++ (tests/fit2d_init_cpu/init_check.cpp), against numpy / torch fp64; with the twin tests/fit2d_init_spec.py alone, that the closed
form the kernels use is the full model's objective and that a gradient with a piece of it missing leaves the bars
tests/test_gpu_fit2d_init.py holds the kernels to; and the planning functions of the command line."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import rotrepr
from tests import fit2d_init_spec as fs
from tests.gradient_bars import EPS32, M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
synth = importlib.import_module("fdcap_amd.synth")
innerfit = importlib.import_module("fdcap_amd.innerfit")
cli = importlib.import_module("fdcap_amd.cli_innerfit")
fio = importlib.import_module("fdcap_amd.io")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "fit2d_init_check")
    src = os.path.join(ROOT, "tests", "fit2d_init_cpu", "init_check.cpp")
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


def _ints(a):
    return [str(int(v)) for v in np.asarray(a).reshape(-1)]


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def _transforms(rng):
    """55 rigid transforms [55, 3, 4] (fp32 values): what the pose forward leaves in G"""
    R = rotrepr.aa2matrot(torch.tensor(rng.standard_normal((55, 3)), dtype=torch.float64)).numpy()
    return _f32(np.concatenate([R, 0.4 * rng.standard_normal((55, 3, 1))], 2))


# ---- the depth guess and the side-view test ------------------------------------------------------------------------------------------
EDGES = ((16, 1), (17, 2))


def _depth_want(G, kp, edges, fx, fy, thr, default):
    l3 = [np.linalg.norm(G[a, :, 3] - G[b, :, 3]) for a, b in edges if kp[a, 2] > thr and kp[b, 2] > thr]
    l2 = [np.hypot((kp[a, 0] - kp[b, 0]) / fx, (kp[a, 1] - kp[b, 1]) / fy) for a, b in edges if kp[a, 2] > thr and kp[b, 2] > thr]
    if not l3 or np.mean(l2) < 1e-6:
        return default, 0
    return np.mean(l3) / np.mean(l2), 1


@pytest.mark.parametrize("case", ["both", "left_shoulder_missing", "right_hip_below_threshold", "none", "coincident", "four_edges"])
def test_depth_guess_matches_fp64_and_falls_back(exe, tmp_path, case):
    rng = np.random.Generator(np.random.PCG64(11))
    G = _transforms(rng)
    kp = _f32(np.concatenate([rng.uniform(100, 1100, (23, 2)), rng.uniform(0.3, 1.0, (23, 1))], 1))
    edges, thr = list(EDGES), 0.25                          # (a binary fraction: the same number in fp32 and fp64)
    if case == "left_shoulder_missing":
        kp[16, 2] = 0.0
    if case == "right_hip_below_threshold":
        kp[2, 2] = 0.25                                      # (the gate is strict: conf > conf_thr)
    if case == "none":
        kp[16, 2] = kp[2, 2] = 0.0
    if case == "coincident":
        kp[1, :2], kp[2, :2] = kp[16, :2], kp[17, :2]
    if case == "four_edges":
        edges += [(16, 17), (1, 2)]
    pad = edges + [(0, 0)] * (4 - len(edges))
    got = _run(exe, tmp_path, "depth", [692.0, 640.0, "23", str(len(edges)), *_ints(pad), "16", "17", thr, 2.5, 25.0, *G.reshape(-1), *kp.reshape(-1)])["guess"]
    z, valid = _depth_want(G.astype(np.float64), kp.astype(np.float64), edges, 692.0, 640.0, thr, 2.5)
    print(case, "z", got[0], "want", z, "valid", got[1])
    assert int(got[1]) == valid == (0 if case in ("none", "coincident") else 1)
    # two square roots, two means and a quotient in fp32: a few units of 2^-24 (differences of pixel coordinates are exact to 2^-24 x 1100)
    assert abs(got[0] - z) <= 16 * EPS32 * abs(z) if valid else got[0] == 2.5


def test_side_view_needs_both_shoulders_and_a_distance_below_the_threshold(exe, tmp_path):
    G = _transforms(np.random.Generator(np.random.PCG64(12)))
    for dist, conf, want in ((24.9, (0.9, 0.9), 1), (25.1, (0.9, 0.9), 0), (24.9, (0.0, 0.9), 0), (24.9, (0.9, 0.0), 0), (0.0, (0.5, 0.5), 1)):
        kp = np.ones((23, 3), np.float32)
        kp[16], kp[17] = (500.0, 300.0, conf[0]), (500.0 + 0.6 * dist, 300.0 + 0.8 * dist, conf[1])
        got = _run(exe, tmp_path, "depth", [692.0, 640.0, "23", "2", *_ints(list(EDGES) + [(0, 0)] * 2), "16", "17", 0.0, 2.5, 25.0, *G.reshape(-1), *kp.reshape(-1)])
        assert int(got["guess"][2]) == want, (dist, conf)


# ---- the camera term --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_torso", [1, 4, 8])
def test_camera_term_and_gradient_match_fp64_autograd_of_the_formula(exe, tmp_path, n_torso):
    rng = np.random.Generator(np.random.PCG64(20 + n_torso))
    G = _transforms(rng)
    G[0, :, :3] = _f32(rotrepr.aa2matrot(torch.tensor([[0.3, -0.5, 0.2]], dtype=torch.float64))[0].numpy())
    torso = [16, 17, 1, 2, 12, 0, 4, 5][:n_torso]
    fx, fy, cx, cy, thr, w_data, w_depth = 692.0, 640.0, 640.0, 360.0, 0.1, 1000.0 / 720.0, 100.0
    xs, x = _f32(rng.standard_normal(78) * 0.1), None
    xs[3:9] = G[0, :, :2].reshape(-1)                        # the set-up's rows hold the root rotation the forward used
    xs[75:78] = (0.0, 0.0, 3.0)
    x = xs.copy()
    x[3:9] += _f32(0.2 * rng.standard_normal(6))             # (not normalised, not the set-up's orientation)
    x[75:78] = (0.05, -0.1, 3.2)
    q64 = np.einsum("ji,kj->ki", G[0, :, :3].astype(np.float64), (G[torso, :, 3] - G[0, :, 3]).astype(np.float64))
    base = G[0, :, 3].astype(np.float64) + xs[0:3]
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    Jt = torch.tensor(base) + torch.einsum("ij,kj->ki", rotrepr.decode_6d(xt[None, 3:9])[0], torch.tensor(q64)) + xt[75:78]
    uv = torch.stack([fx * Jt[:, 0] / Jt[:, 2] + cx, fy * Jt[:, 1] / Jt[:, 2] + cy], 1)
    kp = np.ones((23, 3), np.float32)
    kp[torso, :2] = _f32(uv.detach().numpy() + 20.0 * rng.standard_normal((n_torso, 2)))
    kp[:, 2] = _f32(rng.uniform(0.3, 1.0, 23))
    if n_torso > 1:
        kp[torso[1], 2] = 0.1                                # one keypoint gated out (conf == conf_thr)
    gate = torch.tensor((kp[torso, 2] > np.float32(thr)).astype(np.float64))
    loss = w_data ** 2 * (gate[:, None] * (uv - torch.tensor(kp[torso, :2].astype(np.float64))) ** 2).sum() + w_depth ** 2 * (xt[77] - 3.0) ** 2
    g, = torch.autograd.grad(loss, xt)
    loss = float(loss.detach())
    got = _run(exe, tmp_path, "camera", [fx, fy, cx, cy, "23", str(n_torso), *_ints(torso + [0] * (8 - n_torso)), thr, w_data, w_depth,
                                         *G.reshape(-1), *xs, *x, *kp.reshape(-1)])
    setup = got["setup"]
    np.testing.assert_allclose(setup[:3 * n_torso].reshape(-1, 3), q64, atol=4e-7)       # a 3 x 3 product of entries below 1.5
    assert np.all(setup[3 * n_torso:24] == 0) and setup[27] == 3.0
    np.testing.assert_allclose(setup[24:27], base, atol=2e-7)
    g = g.numpy()
    # residuals of tens of pixels formed from coordinates of hundreds (2^-24 x 640 / 10 relative each), a dozen operations on top
    bar = lambda want: 2e-5 * float(np.abs(want).max())
    print(f"n_torso {n_torso}: loss rel err {abs(got['loss'][0] - loss) / loss:.2e}, sixd max|err| {np.abs(got['g9'][:6] - g[3:9]).max():.2e} "
          f"of {np.abs(g[3:9]).max():.2e}, camt max|err| {np.abs(got['g9'][6:] - g[75:78]).max():.2e} of {np.abs(g[75:78]).max():.2e}")
    assert abs(got["loss"][0] - loss) <= 2e-5 * loss
    assert np.abs(got["g9"][:6] - g[3:9]).max() <= bar(g[3:9]) and np.abs(got["g9"][6:] - g[75:78]).max() <= bar(g[75:78])


# ---- flip and select ------------------------------------------------------------------------------------------------------------------
def _flip_inputs():
    rng = np.random.Generator(np.random.PCG64(30))
    aas = [np.zeros(3), np.array([0.0, 1e-4, 0.0]), np.array([0.0, 1.2, 0.0]), np.array([2.0, 0.3, -0.4]), np.array([0.1, -2.6, 0.2])]
    aas += [s * v / np.linalg.norm(v) for s, v in zip((0.3, 0.9, 1.7, 2.4, 2.9), rng.standard_normal((5, 3)))]
    return _f32(np.array(aas))


def test_flip_is_a_half_turn_about_the_bodys_y_and_twice_is_the_identity(exe, tmp_path):
    aas = _flip_inputs()
    got = _run(exe, tmp_path, "flip", aas.reshape(-1))
    for k, aa in enumerate(aas):
        once, twice = got[f"item{k}"][:3], got[f"item{k}"][3:]
        err = np.abs(fs.rodrigues(once) - fs.flip_rotation(aa.astype(np.float64))).max()
        print(f"aa {aa}: once {once} max|R err| {err:.2e}; twice max|err| {np.abs(twice - aa).max():.2e}")
        assert err <= 2e-6                                   # fp32 Rodrigues, log map and exp map again: some tens of 2^-24 on entries <= 1
        assert np.abs(twice - aa).max() <= 1e-6


def test_select_takes_the_twin_only_when_strictly_lower_and_nan_counts_as_inf(exe, tmp_path):
    pairs = [(1.0, 2.0, 0), (2.0, 1.0, 1), (1.0, 1.0, 0), ("nan", 1.0, 1), (1.0, "nan", 0), ("nan", "nan", 0), ("inf", "nan", 0), ("nan", "inf", 0),
             ("inf", 1e30, 1), (0.0, -0.0, 0)]
    got = _run(exe, tmp_path, "select", [v for a, b, _ in pairs for v in (a, b)])
    assert [int(got[f"item{k}"][0]) for k in range(len(pairs))] == [w for _, _, w in pairs]
    # ... and the twin's rule is the same one
    chosen, take = fs.select([1.0, np.nan, 3.0, np.nan, 0.5, 2.0, 3.0, np.nan], [0, 1, 2, 3])
    assert chosen.tolist() == [1, 1, 0, 0] and take.tolist() == [4, 5, 2, 3]


def test_settings_are_validated(exe, tmp_path):
    def res(n_kp=23, n_edge=2, edge=((16, 1), (17, 2)), n_torso=4, torso=(16, 17, 1, 2), shoulder=(16, 17), num=(0.0, 2.5, 25.0, 1.4, 100.0), surface=-1):
        edge, torso = list(edge) + [(0, 0)] * (4 - len(edge)), list(torso) + [0] * (8 - len(torso))
        return int(_run(exe, tmp_path, "build", [str(n_kp), str(n_edge), *_ints(edge), str(n_torso), *_ints(torso), *_ints(shoulder), *num, str(surface)])["result"][0])
    assert res() == 0 and res(n_edge=4, edge=((16, 1), (17, 2), (16, 17), (1, 2))) == 0 and res(n_torso=8, torso=range(8)) == 0 and res(n_torso=1) == 0
    assert res(n_edge=0) == -1 and res(n_edge=5) == -1 and res(n_torso=0) == -1 and res(n_torso=9) == -1
    assert res(edge=((23, 1), (17, 2))) == -1 and res(edge=((16, 1), (17, -1))) == -1 and res(torso=(16, 17, 1, 23)) == -1 and res(shoulder=(16, 40)) == -1
    assert res(n_kp=17) == -1 and res(n_kp=18) == 0                                       # (slot 17 is the last one used)
    assert res(surface=16) == -1 and res(surface=2) == -1 and res(surface=5) == 0         # a surface point in an edge / the torso; elsewhere
    for i in range(5):
        for bad in ("nan", "inf"):
            num = [0.0, 2.5, 25.0, 1.4, 100.0]
            num[i] = bad
            assert res(num=num) == -1


# ---- the twin alone: the closed form is the full model's objective, and the bars see its pieces ---------------------------------------
def _twin_state(mapped, n=4):
    """set-up rows (the ground truth at (0, 0, z0)) and evaluation rows 0.3 rad and some centimetres away from them"""
    case = fs.make_case(n, 41, mapped, synth, noise_px=15.0)
    rng = np.random.Generator(np.random.PCG64(42))
    xs = case["gt78"].copy()
    xs[:, 75:77] = 0.0
    x = fs.turned(xs, 0.3, rng)
    x[:, 75:78] += _f32(0.05 * rng.standard_normal((n, 3)))
    return case, xs, x


@pytest.mark.parametrize("mapped", [False, True])
def test_closed_form_is_the_full_models_camera_objective_and_mutants_leave_the_bars(mapped):
    case, xs, x = _twin_state(mapped)
    z0 = xs[:, 77]
    f64, g64 = fs.spec_of(case).camera_grads(x, case["kp"], z0)
    f32, g32 = fs.spec_of(case, dtype=torch.float32).camera_grads(x, case["kp"], z0)
    bar_f = M * np.maximum(np.abs(f32 - f64), EPS32 * np.abs(f64))
    bars = {k: M * max(float(np.abs(g32[:, c] - g64[:, c]).max()), EPS32 * float(np.abs(g64[:, c]).max())) for k, c in (("sixd", fs.FREE[:6]), ("camt", fs.FREE[6:]))}
    fc, gc = fs.spec_of(case).closed_form_grad(x, xs, case["kp"], z0)
    ratio = lambda g: {"sixd": float(np.abs(g[:, :6] - g64[:, fs.FREE[:6]]).max()) / bars["sixd"], "camt": float(np.abs(g[:, 6:] - g64[:, fs.FREE[6:]]).max()) / bars["camt"]}
    print("closed form vs full model, max|err| / bar:", ratio(gc), "value", float((np.abs(fc - f64) / bar_f).max()))
    assert max(ratio(gc).values()) <= 1.0 and np.all(np.abs(fc - f64) <= bar_f)
    for mutant in fs.MUTANTS:
        fm, gm = fs.spec_of(case).closed_form_grad(x, xs, case["kp"], z0, mutant=mutant)
        r = ratio(gm)
        print(mutant, "max|err| / bar:", r)
        assert max(r.values()) > 2.0, (mutant, r)


# ---- the settings' defaults and the command line's planning -----------------------------------------------------------------------------
def test_default_init_resolves_on_both_layouts():
    assert "[upstream-recall" in open(os.path.join(ROOT, "4dcapture-fpv_amd", "innerfit.py")).read().split("DEFAULT_INIT = ")[0][-900:]
    d = innerfit.DEFAULT_INIT
    assert d["edges"] == ((16, 1), (17, 2)) and d["torso"] == (16, 17, 1, 2) and d["shoulders"] == (16, 17)
    assert (d["conf_thr"], d["default_depth"], d["side_view_px"], d["w_depth"], d["w_data"]) == (0.0, 2.5, 25.0, 100.0, None)
    ci = innerfit.init_struct(dict(d), None, (692.0, 692.0, 640.0, 360.0))
    assert [list(e) for e in ci.edge][:2] == [[16, 1], [17, 2]] and list(ci.torso)[:4] == [16, 17, 1, 2] and (ci.n_edge, ci.n_torso) == (2, 4)
    assert ci.w_data == np.float32(1000.0 / 720.0) and ci.w_depth == 100.0
    kmap = innerfit.KeypointMap.from_smplx_indices([i for i in innerfit.OPENPOSE_BODY25 if i < 55], [])
    ci = innerfit.init_struct(dict(d), kmap, (692.0, 692.0, 640.0, 360.0))
    slot_joint = kmap.joint
    assert [[int(slot_joint[s]) for s in e] for e in ci.edge][:2] == [[16, 1], [17, 2]] and [int(slot_joint[s]) for s in list(ci.torso)[:4]] == [16, 17, 1, 2]
    assert [int(slot_joint[s]) for s in ci.shoulder] == [16, 17]
    # BODY_25's own order: shoulders 2 (right) and 5 (left), hips 9 and 12 -- the nose (column 0) has no joint and is not in this map
    assert list(ci.shoulder) == [5 - 1, 2 - 1] and list(ci.torso)[:4] == [5 - 1, 2 - 1, 12 - 1, 9 - 1]
    with pytest.raises(innerfit.capi.FdcapError):
        innerfit.init_struct({**d, "torso": (16, 17, 1, 30)}, None, (692.0, 692.0, 640.0, 360.0))
    with pytest.raises(innerfit.capi.FdcapError):
        innerfit.init_struct({**d, "torso": (16, 17, 1, 3)}, kmap, (692.0, 692.0, 640.0, 360.0))       # (joint 3 is no BODY_25 keypoint)
    with pytest.raises(innerfit.capi.FdcapError):
        innerfit.init_struct({**d, "edges": ()}, None, (692.0, 692.0, 640.0, 360.0))


def test_command_line_planning(tmp_path):
    cols, idx = cli.plan_keypoints(False, False)
    assert idx == [i for i in innerfit.OPENPOSE_BODY25 if i < 55] and len(cols) == 14 and 0 not in cols and all(c < 25 for c in cols)
    cols, idx = cli.plan_keypoints(True, False)
    assert len(cols) == 14 + 2 * 16 and all(i < 55 for i in idx) and cols == sorted(cols)
    assert [c for c in cols if c >= 25][:2] == [25, 26] and 25 + 4 not in cols               # a hand's wrist and first joints; its first fingertip is a vertex
    cols, idx = cli.plan_keypoints(True, True)
    assert cols == list(range(67)) and idx == list(innerfit.OPENPOSE_BODY25 + innerfit.OPENPOSE_LHAND + innerfit.OPENPOSE_RHAND)
    cols, idx = cli.plan_keypoints(False, True)
    assert cols == list(range(25)) and max(idx) == 65
    assert cli.plan_frame_batches(10, 4) == [(0, 4), (4, 8), (8, 10)] and cli.plan_frame_batches(8, 4) == [(0, 4), (4, 8)]
    assert cli.plan_frame_batches(3, 256) == [(0, 3)]
    with pytest.raises(ValueError):
        cli.plan_frame_batches(0, 4)
    for text in (json.dumps(list(range(100, 121))), " ".join(str(v) for v in range(100, 121))):
        (tmp_path / "ids.txt").write_text(text)
        assert cli.read_vertex_ids(str(tmp_path / "ids.txt")).tolist() == list(range(100, 121))
    (tmp_path / "ids.txt").write_text("1 2 3")
    with pytest.raises(ValueError):
        cli.read_vertex_ids(str(tmp_path / "ids.txt"))
    for name in ("b_000000000001_keypoints.json", "b_000000000000_keypoints.json", "other.json"):
        (tmp_path / name).write_text("{}")
    assert [os.path.basename(f) for f in cli.keypoint_files(str(tmp_path))] == ["b_000000000000_keypoints.json", "b_000000000001_keypoints.json"]
    with pytest.raises(FileNotFoundError):
        cli.keypoint_files(str(tmp_path / "nothing"))
    assert fio.read_openpose_json(str(tmp_path / "b_000000000000_keypoints.json"), hands=False).shape == (25, 3)
