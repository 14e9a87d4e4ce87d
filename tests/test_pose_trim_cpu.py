"""The pose kernels' joint sets without a GPU: csrc/fdc_frame.h limited to the joints a launch's loss can reach against the
full sets, and the rule that chooses them (plan_pose_joints, csrc/fdc_forms.h).  The stand-alone program
tests/pose_trim_cpu/trim_check.cpp does the work, built with -fsanitize=address,undefined: SMPL-X's tree, random rows,
(jn, jr) in {(12, 55), (23, 23), (17, 55), (55, 55), (1, 1)}; scratch, every output and every row >= jn of G / A / Jrest / dA are NaN
before the limited run; every output row the contract says is written, and all of dx / dO / dcam_ext / dscale, must equal the
full run's as floats and bit for bit but for the sign of a zero.  The full run gets the same dA with the rows >= jn zeroed."""
import subprocess

import pytest

from tests.pose_trim_build import build_exe, cpu_plan


@pytest.fixture(scope="module")
def exe():
    return build_exe(True)


def test_limited_joint_sets_equal_the_full_sets_and_the_plan_rules_hold(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("all checks hold")


def test_the_plans_of_the_bench_and_of_the_gpu_tests():
    # (jn, jr, nlev, world); SMPL-X's tree has 11 levels
    assert cpu_plan(12, True, False) == (12, 55, 5, 0)        # phase 1, leg-only contacts: BASELINE config 3
    assert cpu_plan(12, True, True) == (23, 55, 8, 1)         # ... on a logging iteration
    assert cpu_plan(0, False, True) == (23, 23, 8, 1)         # phase 2
    assert cpu_plan(17, True, False) == (17, 55, 6, 0)        # a contact skinned to a joint in 12..22
    assert cpu_plan(55, True, False) == (55, 55, 11, 1)       # every vertex a contact (config 5): the full plan
    assert cpu_plan(0, False, False) == (1, 1, 1, 0)          # no contact term, phase 1, no logging: the root alone
    assert cpu_plan(12, True, False, trim=False) == (55, 55, 11, 1)       # FDCAP_POSE_TRIM=0
    assert cpu_plan(0, False, True, trim=False) == (55, 55, 11, 1)
