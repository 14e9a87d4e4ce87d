"""The inner fit on mapped keypoints, the parts that need no GPU: the keypoint map's validation and de-duplication and the
per-keypoint math of csrc/fdc_keypoints.h (compiled by plain g++, tests/keypoints_cpu/kp_check.cpp) against fp64 autograd at the bars
of tests/test_innerfit_cpu.py, innerfit.KeypointMap's constructors, and io.read_openpose_json on files the test writes."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
innerfit = importlib.import_module("fdcap_amd.innerfit")
fio = importlib.import_module("fdcap_amd.io")
capi = importlib.import_module("fdcap_amd.capi")


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "kp_check")
    src = os.path.join(ROOT, "tests", "keypoints_cpu", "kp_check.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("fdc_keypoints.h", "fdc_fit2d.h", "fdc_skin.h", "fdc_frame.h", "fdc_math.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", out, src])
    return out


def _run(exe, tmp_path, mode, V, joint, tri, bary, extra=(), n=None):
    fn = os.path.join(tmp_path, "in.txt")
    tok = [V, len(joint) if n is None else n, *joint, *np.asarray(tri).reshape(-1).tolist(), *[repr(float(b)) for b in np.asarray(bary).reshape(-1)]]
    for a in extra:
        tok += [repr(float(v)) for v in np.asarray(a, dtype=np.float32).reshape(-1)]
    with open(fn, "w") as f:
        f.write(" ".join(str(t) for t in tok))
    lines = subprocess.run([exe, mode, fn], check=True, capture_output=True, text=True).stdout.splitlines()
    if lines[0] == "err":
        return None
    out = {"head": [int(t) for t in lines[0].split()[1:]]}
    for ln in lines[1:]:
        name, *vals = ln.split()
        out[name] = np.array([float(v) for v in vals])
    return out


# joints through Jw (3, 20, 22), finger joints (40, 25, 40 again), plain vertices, triples that share vertex 9 with a plain vertex,
# a zero weight, and keypoint 5 once more as keypoint 11
JOINT = [3, -1, 40, -1, 22, -1, 25, 20, -1, 40, 3, -1]
TRI = [(0, 0, 0), (9, 9, 9), (0, 0, 0), (30, 9, 4), (0, 0, 0), (7, 30, 2), (0, 0, 0), (0, 0, 0), (9, 9, 9), (0, 0, 0), (0, 0, 0), (7, 30, 2)]
BARY = [(0, 0, 0), (1, 0, 0), (0, 0, 0), (0.5, 0.25, 0.25), (0, 0, 0), (0.75, 0.0, 0.25), (0, 0, 0), (0, 0, 0), (1, 0, 0), (0, 0, 0), (0, 0, 0),
        (0.75, 0.0, 0.25)]


def test_duplicates_and_shared_vertices_resolve_to_one_fixed_order(exe, tmp_path):
    t = _run(exe, tmp_path, "map", 40, JOINT, TRI, BARY)
    assert t["head"] == [12, 5, 2]
    assert t["real_ids"].tolist() == [2, 4, 7, 9, 30] and t["pseudo_joint"].tolist() == [25, 40]
    assert t["kjoint"].tolist() == [3, -1, -1, -1, 22, -1, -1, 20, -1, -1, 3, -1]
    kref = t["kref"].reshape(12, 3).tolist()
    assert kref[1] == [3, 3, 3] and kref[3] == [4, 3, 1] and kref[5] == [2, 4, 0] and kref[11] == [2, 4, 0]
    assert kref[2] == [6, 6, 6] and kref[9] == [6, 6, 6] and kref[6] == [5, 5, 5]              # pseudo-vertices behind the real ones
    assert t["kbary"].reshape(12, 3)[2].tolist() == [1, 0, 0]
    # per set vertex the keypoints that touch it, ascending in (keypoint, corner); the corner of weight 0 (vertex 30 of keypoints 5, 11) is left out
    lists = [list(zip(t["vl_k"][a:b].astype(int).tolist(), t["vl_w"][a:b].tolist())) for a, b in zip(t["vl_start"][:-1].astype(int), t["vl_start"][1:].astype(int))]
    assert lists == [[(5, 0.25), (11, 0.25)], [(3, 0.25)], [(5, 0.75), (11, 0.75)], [(1, 1.0), (3, 0.25), (8, 1.0)], [(3, 0.5)], [(6, 1.0)],
                     [(2, 1.0), (9, 1.0)]]
    js = t["jl_start"].astype(int)
    assert len(js) == 24 and t["jl_k"][js[3]:js[4]].tolist() == [0, 10] and t["jl_k"][js[20]:js[21]].tolist() == [7] and t["jl_k"][js[22]:js[23]].tolist() == [4]
    assert js[-1] == 4


def test_every_refusal(exe, tmp_path):
    ok = lambda *a, **k: _run(exe, tmp_path, "map", 40, *a, **k) is not None
    assert ok([54, -1], [(0, 0, 0), (0, 39, 1)], [(0, 0, 0), (0.2, 0.3, 0.5)])
    assert ok([], [], []) and ok([0] * 160, [(0, 0, 0)] * 160, [(0, 0, 0)] * 160)
    assert not ok([0] * 161, [(0, 0, 0)] * 161, [(0, 0, 0)] * 161)                        # more than FDCAP_MAX_KEYPOINTS
    assert not ok([], [], [], n=-1)
    assert not ok([55], [(0, 0, 0)], [(0, 0, 0)])                                         # no such joint
    assert not ok([-1], [(0, 40, 1)], [(1, 0, 0)]) and not ok([-1], [(-1, 0, 1)], [(1, 0, 0)])      # vertex ids outside [0, V)
    assert not ok([-1], [(0, 1, 2)], [(1, float("nan"), 0)]) and not ok([-1], [(0, 1, 2)], [(float("inf"), 0, 0)])
    assert ok([7], [(99, -5, 0)], [(float("nan"), 0, 0)])                                 # a joint's triple is not read
    assert capi.MAX_KEYPOINTS == 160 and "#define FDCAP_MAX_KEYPOINTS 160" in open(os.path.join(ROOT, "include", "fdcap.h")).read()


def test_keypoint_math_matches_fp64_autograd(exe, tmp_path):
    rng = np.random.Generator(np.random.PCG64(4))
    V, n = 40, len(JOINT)
    J = (rng.standard_normal((55, 3)) * 0.4 + np.array([0.0, 0.0, 3.0])).astype(np.float32)
    verts = (rng.standard_normal((V, 3)) * 0.4 + np.array([0.0, 0.0, 3.0])).astype(np.float32)
    kp = np.concatenate([rng.uniform(100, 1100, (n, 2)), rng.uniform(0.1, 1.0, (n, 1))], -1).astype(np.float32)
    kp[8, 2] = 0.0                                                                       # an undetected keypoint
    stage = np.array([692, 650, 640, 360, 100, 1.3, 4.78, 5.0, 2.5], np.float32)
    t = _run(exe, tmp_path, "math", V, JOINT, TRI, BARY, extra=(stage, J, verts, kp))
    Jt, vt, k = torch.tensor(J, dtype=torch.float64, requires_grad=True), torch.tensor(verts, dtype=torch.float64, requires_grad=True), torch.tensor(kp, dtype=torch.float64)
    joint, tri = torch.tensor(JOINT), torch.tensor(TRI)
    bary = torch.tensor(np.asarray(BARY, dtype=np.float32), dtype=torch.float64)
    pos = torch.where((joint >= 0)[:, None], Jt[joint.clamp(min=0)], (vt[tri] * bary[:, :, None]).sum(1))
    fx, fy, cx, cy, rho, wd = [float(v) for v in stage[:6]]
    uv = torch.stack([fx * pos[:, 0] / pos[:, 2] + cx, fy * pos[:, 1] / pos[:, 2] + cy], -1)
    r2 = (k[:, :2] - uv) ** 2
    data = wd ** 2 * torch.sum(k[:, 2:3] ** 2 * rho ** 2 * r2 / (r2 + rho ** 2))
    data.backward()
    np.testing.assert_allclose(t["data"][0], float(data.detach()), rtol=2e-6)
    np.testing.assert_allclose(t["pos"].reshape(n, 3), pos.detach().numpy(), rtol=1e-6)
    gJ, gV = Jt.grad.numpy(), vt.grad.numpy()
    gmax = max(np.abs(gJ).max(), np.abs(gV).max())
    got_V, got_J = np.zeros((V, 3)), np.zeros((55, 3))
    nr = t["head"][1]
    gvw = t["gvw"].reshape(-1, 3)
    got_V[t["real_ids"].astype(int)] = gvw[:nr]
    got_J[t["pseudo_joint"].astype(int)] = gvw[nr:]
    got_J[:23] = t["dJw"].reshape(23, 3)
    np.testing.assert_allclose(got_J, gJ, rtol=2e-5, atol=1e-6 * gmax)
    np.testing.assert_allclose(got_V, gV, rtol=2e-5, atol=1e-6 * gmax)
    assert np.abs(gV[30]).max() > 0 and np.abs(gJ[3]).max() > 0 and np.all(got_V[[0, 1, 3]] == 0)
    # the duplicated keypoint and the shared vertex are sums, not overwrites: vertex 9 carries keypoints 1 and 3 (keypoint 8 is undetected)
    assert np.abs(got_V[9] - gV[9]).max() <= 2e-5 * np.abs(gV[9]).max()


def test_where_the_blend_product_runs(exe, tmp_path):
    """by size: the kernel's own multiply-adds below 64 frames x 300 columns, the set's panel products from there; the switch pins one"""
    fn = os.path.join(tmp_path, "blend.txt")
    cases = [(64, 63), (1024, 63), (64, 299), (64, 300), (16, 450), (43, 450), (1024, 522), (1, 1440), (14, 1440), (1024, 0)]
    open(fn, "w").write(" ".join(f"{a} {b}" for a, b in cases))

    def run(pin):
        env = {k: v for k, v in os.environ.items() if k != "FDCAP_KP_BLEND"}
        if pin:
            env["FDCAP_KP_BLEND"] = pin
        return [int(l) for l in subprocess.run([exe, "blend", fn], check=True, capture_output=True, text=True, env=env).stdout.split()]
    assert run(None) == [0, 1, 0, 1, 0, 1, 1, 0, 1, 0]
    assert run("kernel") == [0] * 10
    assert run("panel") == [1] * 9 + [0]                      # (a set without real vertices has no product)
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("| `FDCAP_KP_BLEND")]
    assert len(rows) == 1


def test_keypoint_map_constructors():
    m = innerfit.KeypointMap.joints23()
    assert len(m) == 23 and m.joint.tolist() == list(range(23)) and not m.tri.any() and not m.bary.any()
    extra = np.arange(1000, 1021)
    lm_tri, lm_b = np.array([[5, 6, 7], [8, 9, 10]]), np.array([[0.2, 0.3, 0.5], [1.0, 0.0, 0.0]])
    m = innerfit.KeypointMap.from_smplx_indices([0, 54, 55, 75, 76, 77], extra, lm_tri, lm_b)
    assert m.joint.tolist() == [0, 54, -1, -1, -1, -1]
    assert m.tri.tolist() == [[0, 0, 0], [0, 0, 0], [1000] * 3, [1020] * 3, [5, 6, 7], [8, 9, 10]]
    np.testing.assert_array_equal(m.bary, np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0], [0.2, 0.3, 0.5], [1, 0, 0]], np.float32))
    body = innerfit.KeypointMap.from_smplx_indices(innerfit.OPENPOSE_BODY25 + innerfit.OPENPOSE_LHAND + innerfit.OPENPOSE_RHAND, extra)
    assert len(body) == 67 and int((body.joint < 0).sum()) == 21 and sorted(body.tri[body.joint < 0, 0].tolist()) == extra.tolist()
    assert sorted(set(innerfit.OPENPOSE_LHAND) | set(innerfit.OPENPOSE_RHAND)) == [20, 21] + list(range(25, 55)) + list(range(66, 76))
    with pytest.raises(capi.FdcapError):
        innerfit.KeypointMap.from_smplx_indices([76], extra)                   # a landmark without the landmark tables
    with pytest.raises(capi.FdcapError):
        innerfit.KeypointMap.from_smplx_indices([60], extra[:5])
    with pytest.raises(capi.FdcapError):
        innerfit.KeypointMap(np.zeros(161), np.zeros((161, 3)), np.zeros((161, 3)))


def test_read_openpose_json(tmp_path):
    rng = np.random.Generator(np.random.PCG64(1))
    part = lambda n: rng.uniform(0, 1000, (n, 3)).round(3)
    body, lh, rh, face = part(25), part(21), part(21), part(70)
    person = {"pose_keypoints_2d": body.reshape(-1).tolist(), "hand_left_keypoints_2d": lh.reshape(-1).tolist(),
              "hand_right_keypoints_2d": rh.reshape(-1).tolist(), "face_keypoints_2d": face.reshape(-1).tolist()}
    other = {k: [0.0] * len(v) for k, v in person.items()}
    fn = os.path.join(tmp_path, "full.json")
    json.dump({"version": 1.3, "people": [person, other]}, open(fn, "w"))
    kp = fio.read_openpose_json(fn)
    assert kp.shape == (67, 3) and kp.dtype == np.float32
    np.testing.assert_array_equal(kp, np.concatenate([body, lh, rh]).astype(np.float32))          # people[0], BODY_25 | left | right
    np.testing.assert_array_equal(fio.read_openpose_json(fn, hands=True, face=True), np.concatenate([body, lh, rh, face]).astype(np.float32))
    assert fio.read_openpose_json(fn, hands=False).shape == (25, 3)
    json.dump({"people": []}, open(fn, "w"))
    assert fio.read_openpose_json(fn).shape == (67, 3) and not fio.read_openpose_json(fn).any()    # nobody: confidence 0
    del person["hand_left_keypoints_2d"], person["hand_right_keypoints_2d"]
    json.dump({"people": [person]}, open(fn, "w"))
    kp = fio.read_openpose_json(fn)
    np.testing.assert_array_equal(kp[:25], body.astype(np.float32))
    assert kp.shape == (67, 3) and not kp[25:].any()                                               # hands absent
