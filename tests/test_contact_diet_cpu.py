"""What the skinning backward forms instead of staging (csrc/fdc_skin.h, csrc/fdc_math.h), without a GPU: the stand-alone program
tests/contact_diet_cpu/recompute_check.cpp, built with -fsanitize=address,undefined, checks that the helper the forward kernels and
the backward share is the forward's expression bit for bit (random inputs, NaN, infinities), that the distance of a query without a
neighbour is the constant the backward uses, and that the rows of A below ja_hi cover every joint id of random weight lists."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "contact_diet_cpu", "recompute_check.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("fdc_skin.h", "fdc_math.h")]


def build_exe() -> str:
    exe = os.path.join(BUILD, "contact_diet_check_san")
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        # -ffp-contract=off as the host harness (tests/host_pipeline.py): the same expressions, no fused multiply-adds
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-g", "-o", exe, SRC])
    return exe


def test_the_helper_the_constant_and_the_staged_rows():
    r = subprocess.run([build_exe()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("all checks hold")
