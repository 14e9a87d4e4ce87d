"""The clip-level reprojection term (fdcap_opt_set_reproj): what needs no GPU.

The first four tests below (gradcheck, the zero blocks, the mutants, the twin's Adam loop) pin the SPECIFICATION, tests/reproj_spec.py,
on the oracle alone: they do not touch the library and would pass without it -- they are what makes the GPU test's bars mean
something.  The others run the library's host parts and the Python and command-line layers.

  * the specification (tests/reproj_spec.py): the twin's fp64 gradient against torch.autograd.gradcheck, d scale and d camera_ext
    exactly zero, and the mutants -- the d cam_t sum dropped, cam_t times `scale` (the world-joint formula), conf in place of
    conf^2 -- each leaving the bars tests/test_gpu_reproj.py holds the kernels to by a factor, so that test cannot pass vacuously;
  * the comparative fit's ordering with the twin's own Adam loop;
  * the host parts: plan_pose_joints' new argument and reproj_joint (tests/reproj_cpu/reproj_check.cpp, built with the sanitizers),
    innerfit.joints23_from_openpose, the command line's pairing and refusals, the ValueErrors of the other modes and of a batch,
    the logged row with the term."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
import tests.gradient_bars as gb
from fdcap_amd import capi, cli, fitting, innerfit, io
from tests import reproj_spec as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 20.0
FIT_CASE, FIT_ITERS, FIT_WEIGHT = rs.CASES[0], 40, 2e-2
# the blocks each mutant must leave (a factor FACTOR outside the bar)
TARGETS = {"no_dcamt": ("camt",), "camt_scale": ("transl", "sixd", "betas", "latent", "camt", "dscale"),
           "conf_linear": ("transl", "sixd", "betas", "latent", "camt")}


def test_twin_gradient_passes_gradcheck():
    """fp64, a small clip: the analytic gradient autograd gives the twin against central differences, NaN keypoints included."""
    case = rs.CASES[1]
    rs.check_inputs(case)
    t, kp = rs.twin(case), rs.make_keypoints(case)
    rows = torch.tensor(rs.start_rows(case), dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda r: t.loss(r, kp, 1.0), (rows,), eps=1e-6, atol=1e-7, rtol=1e-5)


@pytest.mark.parametrize("case", rs.CASES, ids=lambda c: "-".join(map(str, c)))
def test_twin_has_no_gradient_to_scale_and_camera_and_none_to_the_hands(case):
    it = rs.isolated(case)
    for prec in ("g64", "g32"):
        g = it[prec]
        for k in ("lh", "rh", "dscale", "cam_rot", "cam_transl", "cam_bottom"):
            assert np.all(g[k] == 0), (prec, k)
        for k in ("transl", "sixd", "betas", "latent", "camt"):
            assert np.abs(g[k]).max() > 0, (prec, k)
    # an undetected keypoint and a frame without detections: exact zeros, NaN coordinates notwithstanding
    assert all(np.all(np.isfinite(v)) for v in it["g64"].values())
    if case[0] >= 4:
        assert np.all(rs.twin(case).grads(it["rows"], it["kp"])["rows"][rs.EMPTY_FRAME] == 0)
    # d transl = d cam_t = sum_j dJb_j: the same numbers
    np.testing.assert_allclose(it["g64"]["transl"], it["g64"]["camt"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("mutant", rs.MUTANTS)
@pytest.mark.parametrize("case", rs.CASES, ids=lambda c: "-".join(map(str, c)))
def test_mutants_leave_the_bars(case, mutant):
    it = rs.isolated(case)
    g = rs.twin(case).grads(it["rows"], it["kp"], mutant=mutant)
    r = gb.ratios(gb.blocks(rows=g["rows"], dscale=g["dscale"], dcam=g["dcam"]), it["g64"], it["bar"])
    for k in TARGETS[mutant]:
        assert r[k] >= FACTOR, (mutant, k, r[k])


def test_comparative_fit_orders_with_the_twins_own_adam_loop():
    """n = 12, 40 iterations, default weights, the data displaced from the ground truth by the perturbation: the mean pixel error on
    the rows the loop ends at is lower with the term than without it, and lower than on the rows the loop starts from (init()'s: the
    outlier row replaced by its neighbour's -- the frame the term alone sees).  No other seed had to be tried."""
    from oracle import rotrepr
    from oracle.fitting import find_outliers_and_sources
    t, kp = rs.twin(FIT_CASE), rs.make_keypoints(FIT_CASE)
    x78 = rotrepr.convert_to_6D_rot(torch.tensor(rs.fit75(FIT_CASE), dtype=torch.float64)).detach().float()
    idx1, pos = find_outliers_and_sources(x78)
    assert len(idx1) >= 1
    start = x78.clone()
    start[idx1] = x78[pos]
    e_start = t.pixel_error(start.numpy(), kp)
    e_off = t.pixel_error(rs.adam_fit(FIT_CASE, 0.0, FIT_ITERS), kp)
    e_on = t.pixel_error(rs.adam_fit(FIT_CASE, FIT_WEIGHT, FIT_ITERS), kp)
    print(f"mean pixel error: start {e_start:.3f}, term off {e_off:.3f}, term on {e_on:.3f}")
    assert e_on < e_off and e_on < e_start


def test_host_program_plan_and_joint(tmp_path):
    """tests/reproj_cpu/reproj_check.cpp under -fsanitize=address,undefined"""
    exe = str(tmp_path / "reproj_check")
    src = os.path.join(ROOT, "tests", "reproj_cpu", "reproj_check.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-g", "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout[-2000:], p.stderr[-2000:])


def test_joints23_from_openpose_on_a_hand_made_row():
    row = np.zeros((67, 3), np.float32)                       # BODY_25 | hands, as io.read_openpose_json gives
    row[:, 0] = 10 + np.arange(67)
    row[:, 1] = 500 - np.arange(67)
    row[:, 2] = 0.5 + 0.005 * np.arange(67)
    out = innerfit.joints23_from_openpose([row, row[:25] * 2])
    assert out.shape == (2, 23, 3) and out.dtype == np.float32
    want = {12: 1, 17: 2, 19: 3, 21: 4, 16: 5, 18: 6, 20: 7, 0: 8, 2: 9, 5: 10, 8: 11, 1: 12, 4: 13, 7: 14}     # joint <- BODY_25 keypoint
    assert sum(1 for j in innerfit.OPENPOSE_BODY25 if j < 23) == 14 == len(want)
    for j in range(23):
        if j in want:
            np.testing.assert_array_equal(out[0, j], row[want[j]])
            np.testing.assert_array_equal(out[1, j], 2 * row[want[j]])
        else:
            assert np.all(out[:, j] == 0)
    with pytest.raises(ValueError):
        innerfit.joints23_from_openpose([row[:24]])


def _write_openpose(path, n, start=0):
    os.makedirs(path, exist_ok=True)
    for i in range(n):
        kp = np.zeros((25, 3), np.float32)
        kp[8] = (600 + i, 400, 0.9)                           # mid hip -> the pelvis
        with open(os.path.join(path, f"frame_{start + i:06d}_keypoints.json"), "w") as fh:
            json.dump({"people": [{"pose_keypoints_2d": kp.reshape(-1).tolist()}]}, fh)


def test_cli_pairs_keypoint_files_with_frames_and_refuses(tmp_path):
    d = str(tmp_path / "kp")
    _write_openpose(d, 5)
    open(os.path.join(d, "notes.txt"), "w").close()
    files = cli.keypoint_files(d, 5)
    assert [os.path.basename(f) for f in files] == [f"frame_{i:06d}_keypoints.json" for i in range(5)]
    j = innerfit.joints23_from_openpose([io.read_openpose_json(f, hands=False) for f in files])
    assert j.shape == (5, 23, 3) and np.array_equal(j[:, 0, 0], 600 + np.arange(5, dtype=np.float32)) and np.all(j[:, 1:] == 0)
    with pytest.raises(ValueError, match=r"5 \*_keypoints.json files .* for 7 frames"):
        cli.keypoint_files(d, 7)
    for argv in (["--clips", "/x/a/", "--fit-root", "/tmp/never", "--keypoints", d, "--weight-reproj", "0.1"],
                 ["--clips", "/x/a/", "--fit-root", "/tmp/never", "--weight-reproj", "0.1"],
                 ["--clips", "/x/a/", "--fit-root", "/tmp/never", "--intrinsics", "1", "1", "0", "0"],
                 ["--clips", "/x/a/", "--fit-root", "/tmp/never", "--rho", "100"],
                 ["body/x/results", "fit", "global", "--weight-reproj", "0.1"],
                 ["body/x/results", "fit", "global", "--keypoints", d],
                 ["body/x/results", "fit", "local", "--keypoints", d, "--weight-reproj", "0.1"],
                 ["body/x/results", "fit", "dct", "--keypoints", d, "--weight-reproj", "0.1"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv


def test_other_modes_and_a_batch_raise_before_anything_touches_the_device(monkeypatch):
    """FittingOP.fitting's refusals come before the call's first device work (no FittingOP can be built without a GPU, so the method
    runs on a bare object here); ClipBatchFitter's comes before its context exists."""
    assert fitting.DEFAULT_LOSSCONFIG["weight_reproj"] == 0
    with pytest.raises(ValueError, match="weight_reproj"):
        fitting.ClipBatchFitter({}, {"weight_reproj": 0.1})
    fop = object.__new__(fitting.FittingOP)
    fop.weight_reproj, fop.num_body = 0.1, 4
    kp = np.zeros((4, 23, 3), np.float32)
    for mode in ("local", "dct"):
        with pytest.raises(ValueError, match="mode 'global'"):
            fop.fitting(np.zeros((4, 75), np.float32), mode, keypoints=kp)
    with pytest.raises(ValueError, match="keypoints"):
        fop.fitting(np.zeros((4, 75), np.float32), "global")
    with pytest.raises(ValueError, match=r"\[4,23,3\]"):
        fop.fitting(np.zeros((4, 75), np.float32), "global", keypoints=kp[:3])
    with pytest.raises(ValueError, match="intrinsics"):
        fop.fitting(np.zeros((4, 75), np.float32), "global", keypoints=kp, intrinsics=(0.0, 692.0, 640.0, 360.0))
    with pytest.raises(ValueError, match="rho"):
        fop.fitting(np.zeros((4, 75), np.float32), "global", keypoints=kp, rho=float("nan"))
    fop.weight_reproj = -1.0
    with pytest.raises(ValueError, match="weight_reproj"):
        fop.fitting(np.zeros((4, 75), np.float32), "global", keypoints=kp)


def test_logged_row_gains_the_term_and_is_unchanged_without_it(capsys):
    s = np.array([41.7, 3.9, 0.83, 17.3, 5.1, 0.0, 6100.0, 0.0])
    n, nc = 12, 40
    fop = object.__new__(fitting.FittingOP)
    fop.num_body, fop.ctx, fop._mode, fop.verbose = n, type("C", (), {"num_contact": nc})(), "global", True
    fop.weight_loss_rec, fop.weight_loss_vposer, fop.weight_contact, fop.weight_reproj = 1.0, 0.001, 0.1, 0.25
    fop.shard = type("S", (), {"rank": 0})()
    for phase2 in (False, True):
        base = fitting.logged_losses(s, n, nc, 1.0, 0.001, 0.1, phase2)
        fop._reproj = None
        log = fitting.FitLog()
        fop._append_log(log, 3, phase2, s)
        off = capsys.readouterr().out
        assert log.total == [base[5]] and log.reproj == [] and "loss_reproj" not in off
        fop._reproj = (None, None, None)
        log = fitting.FitLog()
        fop._append_log(log, 3, phase2, s)
        on = capsys.readouterr().out
        l_rp = 0.25 * 6100.0 / (23 * n)
        assert fitting.reproj_loss(s, n, 0.25) == l_rp and capi.LOSS_REPROJ == 6
        assert log.reproj == [l_rp] and log.total == [base[5] + l_rp] and log.l_rec == [base[0]]
        assert on.strip().endswith("loss_reproj={:f}".format(l_rp)) and on.startswith(off.strip().rsplit("total_loss", 1)[0])
    assert fitting.MAIN_TERMS == ("l_rec", "l_vposer", "loss_smoothing", "loss_contact", "loss_world_smoothing", "total_loss")
