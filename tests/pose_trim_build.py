"""Builds tests/pose_trim_cpu/trim_check.cpp (test infrastructure shared by tests/test_pose_trim_cpu.py and
tests/test_gpu_pose_trim.py): csrc/fdc_frame.h and csrc/fdc_forms.h for the host, as a stand-alone program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "pose_trim_cpu", "trim_check.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("fdc_forms.h", "fdc_frame.h", "fdc_host_setup.h", "fdc_math.h")]


def build_exe(sanitize: bool) -> str:
    """sanitize: with -fsanitize=address,undefined (every finding ends the program with a non-zero status)."""
    exe = os.path.join(BUILD, "pose_trim_check_san" if sanitize else "pose_trim_check")
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
        # -ffp-contract=off as the host harness (tests/host_pipeline.py): the same expressions, no fused multiply-adds
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", *san, "-o", exe, SRC])
    return exe


def cpu_plan(ja_hi: int, contact_state: bool, need_world: bool, trim: bool = True):
    """plan_pose_joints on SMPL-X's tree: (jn, jr, nlev, world)."""
    out = subprocess.run([build_exe(False), "plan", str(ja_hi), str(int(contact_state)), str(int(need_world)), str(int(trim))],
                         check=True, capture_output=True, text=True).stdout.split()
    return tuple(int(v) for v in out)
