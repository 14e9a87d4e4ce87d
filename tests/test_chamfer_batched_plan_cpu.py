"""plan_nn_batched (csrc/fdc_forms.h): the grid of the every-pair search with a batch axis, as a pure function, without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "chamfer_plan_cpu", "plan.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "chamfer_plan")

SIZES = [(1, 1, 1), (500, 10475, 1), (500, 10475, 64), (500, 10475, 1024), (10475, 500, 1024), (100000, 500, 256), (2048, 2304, 2),
         (2048, 2047, 2), (512, 8192, 3), (513, 8192, 3), (2, 3, 65535), (2, 3, 65536), (2, 3, 200000), (300, 9000, 2),
         (1000, 5_000_000, 4), (7, 1 << 30, 1)]


@pytest.fixture(scope="module")
def plans():
    os.makedirs(BUILD, exist_ok=True)
    deps = [SRC, os.path.join(CSRC, "fdc_forms.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", EXE, SRC])
    args = [str(v) for s in SIZES for mode in (0, 1, 2) for v in (*s, mode)]
    env = {k: v for k, v in os.environ.items() if not k.startswith("FDCAP_")}
    out = subprocess.run([EXE, *args], check=True, capture_output=True, text=True, env=env).stdout.splitlines()
    rows = {}
    for line in out:
        nq, nt, B, mode, name, mfma, nsplit, qblocks, grid_x, block, launches, split_len = line.split()
        rows[(int(nq), int(nt), int(B), int(mode))] = dict(name=name, mfma=int(mfma), nsplit=int(nsplit), qblocks=int(qblocks),
                                                          grid_x=int(grid_x), block=int(block), launches=int(launches),
                                                          split_len=int(split_len))
    assert len(rows) == 3 * len(SIZES)
    return rows


def test_the_kernel_is_the_one_a_single_batch_selects(plans):
    for (nq, nt, B, mode), p in plans.items():
        want = {0: nq * nt >= (1 << 22), 1: False, 2: True}[mode]                 # nn_use_mfma on ONE batch's sizes, whatever B
        assert p["mfma"] == int(want), (nq, nt, B, mode)
        assert p["name"] == ("nn_mfma_batched" if want else "nn_direct_batched")


def test_the_grid_covers_every_query_block_of_every_split_and_every_batch(plans):
    for (nq, nt, B, mode), p in plans.items():
        assert p["block"] == 256 and p["qblocks"] == (nq + 511) // 512            # both kernels: 512 queries per workgroup
        assert p["grid_x"] == p["qblocks"] * p["nsplit"] >= 1
        assert p["launches"] == (B + 65534) // 65535 >= 1                          # the batch on blockIdx.y, at most 65 535 per launch
        ns = p["nsplit"]
        assert ns >= 1 and ns & (ns - 1) == 0
        assert p["split_len"] % 512 == 0 and p["split_len"] * ns >= nt             # chunk-aligned splits that cover the targets
        assert p["split_len"] // 512 <= 2048                                       # ... each within the survivor list's reach


def test_more_batches_never_ask_for_more_splits(plans):
    """The splits exist to fill the machine when there are few query blocks; batches fill it too."""
    assert plans[(500, 10475, 1, 0)]["nsplit"] >= plans[(500, 10475, 64, 0)]["nsplit"] >= plans[(500, 10475, 1024, 0)]["nsplit"]
    assert plans[(500, 10475, 1, 0)]["nsplit"] == 4 and plans[(10475, 500, 1024, 0)]["nsplit"] == 1
