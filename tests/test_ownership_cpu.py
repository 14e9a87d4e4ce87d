"""csrc/fdc_own.h -- the types that own every device block, pinned block and HIP event of the library -- on a CPU: a stand-alone
program (tests/ownership_cpu/own_check.cpp) defines counting stand-ins for the HIP names the header uses, lets the allocating ones
fail on the k-th call, and runs under AddressSanitizer + UndefinedBehaviorSanitizer.  What it asserts: growing frees exactly the
old block, a failed grow leaves an empty buffer, moves transfer and free, structs / arrays / event lists free everything at the end
of their scope or on `delete`, an early return frees what was made, and a failure at any position of a create sequence leaves
nothing live."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owning_types_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "own_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-g", "-o", exe, os.path.join(ROOT, "tests", "ownership_cpu", "own_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "own_check: ok" in out.stdout
