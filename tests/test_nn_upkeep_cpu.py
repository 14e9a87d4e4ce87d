"""When the in-loop Chamfer search rebuilds its query order is a pure function in csrc/fdc_forms.h: nn_order_period(base, rebuilds,
nq), the period in search launches that follows the fit's `rebuilds`-th rebuild of an order over nq queries.  base is FDCAP_NN_ORDER.
The period grows for orders of up to 2 097 152 queries (the sizes it was measured to win at); above, it is the base.  Checked here without a GPU,
through a plain g++ build of the header (twice: as shipped, and with -DFDC_NN_PERIOD_GROWTH=0, the fixed period of earlier builds).

How a period becomes launch numbers (fdc_chamfer.h nn_stream_upkeep; launch 1 is the fit's seeding launch): rebuild 1 follows
launch 1; the launch after a rebuild records the new groups' work and is followed by the launch-order sort, which starts the count;
so rebuild r + 1 follows launch  L(r) + 1 + nn_order_period(base, r, nq).  tests/nn_upkeep_rule.py holds the build and that recurrence,
shared with tests/test_gpu_nn_upkeep.py, which holds the library's own count against it."""
import subprocess

import pytest

from tests.nn_upkeep_rule import build_exe, periods, rebuild_launches, rebuilds_within

BASES = [1, 2, 7, 8, 16, 31, 32, 33, 48, 64, 100, 127, 128]
COUNTS = list(range(0, 41)) + [100, 1000, 1 << 20, (1 << 31) - 1]


@pytest.fixture(scope="module")
def exe():
    return build_exe(True)


@pytest.fixture(scope="module")
def exe_fixed():
    return build_exe(False)


def test_constants(exe, exe_fixed):
    run = lambda e: subprocess.run([e, "constants"], check=True, capture_output=True, text=True).stdout.split()
    assert run(exe) == ["3", "128", "2097152", "1"]
    assert run(exe_fixed) == ["3", "128", "2097152", "0"]


@pytest.mark.parametrize("base", BASES)
def test_period_is_positive_never_decreases_and_stops_at_128(exe, base):
    got = periods(exe, base, COUNTS)
    assert got[0] == got[1] == base                                       # before and after the seeding launch's rebuild: the base
    assert all(1 <= p <= 128 for p in got), got
    assert all(a <= b for a, b in zip(got, got[1:])), got
    assert got[-1] == 128                                                 # every base reaches the cap ...
    assert got.index(128) <= 3 + 7 or base == 128                         # ... after at most seven doublings behind the hold


@pytest.mark.parametrize("nq", [1, 90_400, 512_000, 2_048_000, 1 << 21])
def test_the_rule_is_the_same_at_every_size_it_is_taken_at(exe, nq):
    for base in (8, 32):
        assert periods(exe, base, COUNTS, nq) == periods(exe, base, COUNTS)


@pytest.mark.parametrize("nq", [(1 << 21) + 1, 5_363_200, (1 << 31) - 1])
def test_above_the_largest_size_measured_to_win_the_period_is_the_base(exe, nq):
    for base in BASES:
        assert periods(exe, base, COUNTS, nq) == [base] * len(COUNTS)
    assert rebuilds_within(exe, 32, 400, nq) == 13           # config 5 keeps the 13 rebuilds of the fixed period


def test_base_zero_or_negative_is_off(exe, exe_fixed):
    for e in (exe, exe_fixed):
        for base in (0, -1, -32):
            assert periods(e, base, COUNTS) == [0] * len(COUNTS)


def test_a_base_above_the_cap_stays_as_given(exe):
    for base in (129, 200, 4096):
        assert periods(exe, base, COUNTS) == [base] * len(COUNTS)


@pytest.mark.parametrize("base", BASES + [129, 500])
def test_growth_compiled_out_is_the_fixed_period(exe_fixed, base):
    assert periods(exe_fixed, base, COUNTS) == [base] * len(COUNTS)


# By hand from the rule: three rebuilds at the base period, then doubling up to 128; a rebuild follows the last one by
# 1 + period launches.
#   base 32: periods 32 32 32 64 128 128 ...  -> steps 33 33 33 65 129 129 ...
#   base  8: periods  8  8  8 16  32  64 128 128 ... -> steps 9 9 9 17 33 65 129 129 ...
LAUNCHES_32 = [1, 34, 67, 100, 165, 294, 423, 552, 681, 810, 939, 1068, 1197, 1326, 1455, 1584, 1713, 1842, 1971, 2100]
LAUNCHES_8 = [1, 10, 19, 28, 45, 78, 143, 272, 401, 530, 659, 788, 917, 1046, 1175, 1304, 1433, 1562, 1691, 1820]


def test_launches_of_the_first_twenty_rebuilds(exe):
    assert len(LAUNCHES_32) == len(LAUNCHES_8) == 20
    assert rebuild_launches(exe, 32, 20) == LAUNCHES_32
    assert rebuild_launches(exe, 8, 20) == LAUNCHES_8


def test_fixed_period_launches(exe_fixed):
    assert rebuild_launches(exe_fixed, 32, 13) == [1 + 33 * k for k in range(13)]      # the 13 rebuilds of a 400-launch fit before r18
    assert rebuilds_within(exe_fixed, 32, 400) == 13


def test_rebuild_counts_of_whole_fits(exe):
    assert rebuilds_within(exe, 32, 400) == 6                             # a 500-iteration fit: 400 phase-1 launches
    assert rebuilds_within(exe, 32, 800) == 9
    assert rebuilds_within(exe, 8, 112) == 6 and rebuilds_within(exe, 8, 140) == 6
    assert rebuilds_within(exe, 8, 143) == 7
    assert rebuilds_within(exe, 32, 1) == 1 and rebuilds_within(exe, 32, 33) == 1 and rebuilds_within(exe, 32, 34) == 2
    assert rebuilds_within(exe, 0, 400) == 0
