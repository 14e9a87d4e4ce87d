"""Clips of different scenes in one batch, the parts that need no GPU: the segment table (csrc/fdc_clips.h, compiled by plain g++),
the decision between the one-launch and the per-segment search (plan_nn_segments, csrc/fdc_forms.h) over the sizes and switches
tests/test_gpu_multiscene.py uses, the batch planner of `--clips --mix-scenes` (cli.plan_batches_scenes), the order in which a
fitter puts the clips of a batch (ClipBatchFitter.plan_scene_runs) and the refusals that need no device."""
import importlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
cli = importlib.import_module("fdcap_amd.cli")
SEGMENTS = "nn_stream4_kernel(1 wave per group, segments)"


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "segment_table")
    src = os.path.join(ROOT, "tests", "multiscene_cpu", "segment_table.cpp")
    deps = [src, os.path.join(CSRC, "fdc_clips.h"), os.path.join(CSRC, "fdc_forms.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, "-o", out, src])
    return out


def _segments(exe, nc, lens, slots):
    """-> (slots admissible, [(row0, rows, slot, clip0, nclips, q0, nq, g0, groups)])"""
    lines = subprocess.run([exe, "seg", str(nc), str(len(lens)), *map(str, lens), *map(str, slots)], check=True, capture_output=True,
                           text=True).stdout.splitlines()
    return lines[0] == "ok 1", [tuple(int(t) for t in ln.split()[1:]) for ln in lines[1:]]


def _spec(nc, lens, slots):
    """the table by its definition: maximal runs of adjacent clips of one slot"""
    out, start = [], 0
    for k, (n, s) in enumerate(zip(lens, slots)):
        if out and out[-1]["slot"] == s:
            out[-1]["rows"] += n
            out[-1]["nclips"] += 1
        else:
            out.append({"row0": 2 + start, "rows": n, "slot": s, "clip0": k, "nclips": 1})
        start += n
    g0, res = 0, []
    for g in out:
        nq = g["rows"] * nc
        groups = (nq + 31) // 32
        res.append((g["row0"], g["rows"], g["slot"], g["clip0"], g["nclips"], (g["row0"] - 2) * nc, nq, g0, groups))
        g0 += groups
    return res


# ---- the segment table ---------------------------------------------------------------------------------------------------
def test_a_slot_that_comes_back_is_a_segment_of_its_own(exe):
    ok, segs = _segments(exe, 32, (40, 33, 24), (0, 1, 0))
    assert ok
    assert segs == [(2, 40, 0, 0, 1, 0, 1280, 0, 40), (42, 33, 1, 1, 1, 1280, 1056, 40, 33), (75, 24, 0, 2, 1, 2336, 768, 73, 24)]
    assert segs == _spec(32, (40, 33, 24), (0, 1, 0))


def test_all_clips_on_one_slot_are_one_segment(exe):
    for slot in (0, 5, 7):
        ok, segs = _segments(exe, 20, (40, 33, 24, 3), (slot,) * 4)
        assert ok and segs == [(2, 100, slot, 0, 4, 0, 2000, 0, 63)]


def test_adjacent_clips_of_one_slot_share_a_segment_and_one_clip_can_be_one(exe):
    lens, slots = (3, 40, 33, 3, 1), (2, 0, 0, 7, 2)
    ok, segs = _segments(exe, 12, lens, slots)
    assert ok and segs == _spec(12, lens, slots)
    assert [(s[1], s[2], s[4]) for s in segs] == [(3, 2, 1), (73, 0, 2), (3, 7, 1), (1, 2, 1)]
    # every segment starts a group of its own: 36 queries are two groups, and the next segment's first group is not shared
    assert [s[7:] for s in segs] == [(0, 2), (2, 28), (30, 2), (32, 1)]
    # the query ranges tile the batch's rows x nc queries
    assert segs[0][5] == 0 and all(a[5] + a[6] == b[5] for a, b in zip(segs, segs[1:])) and segs[-1][5] + segs[-1][6] == sum(lens) * 12


@pytest.mark.parametrize("slots", [(0, 8), (-1, 0), (0, 1, 99)])
def test_slots_out_of_range_are_refused(exe, slots):
    ok, segs = _segments(exe, 16, (10,) * len(slots), slots)
    assert not ok and segs == []


# ---- one launch, or one launch set per segment ----------------------------------------------------------------------------------
def _plan(exe, nn_stream, loop, mode, culled, frags, sip, nq, nt):
    tok = subprocess.run([exe, "plan", *map(str, (nn_stream, int(loop), mode, int(culled), int(frags), int(sip), len(nq), *nq, *nt))], check=True,
                         capture_output=True, text=True).stdout.split(maxsplit=5)
    assert tok[0] == "plan"
    return {"one": tok[1] == "1", "grid": (int(tok[2]), int(tok[3])), "block": int(tok[4]), "name": tok[5].strip()}


# (segment queries, scene points) of tests/test_gpu_multiscene.py: 32 contacts; clips (40, 33, 24) on scenes of 3 000 / 4 133 points,
# a 3-frame clip at either end, the full body's (100, 75) frames x 500 contacts on 20 000-point scenes
GPU_CASES = [((1280, 1056, 768), (3000, 4133, 3000)), ((96, 1280, 96), (4133, 3000, 4133)), ((50000, 37500), (20000, 20000))]


@pytest.mark.parametrize("nq,nt", GPU_CASES)
def test_the_pinned_one_wave_form_takes_all_segments_in_one_launch(exe, nq, nt):
    p = _plan(exe, 11, False, 2, True, True, True, nq, nt)
    groups = (max(nq) + 31) // 32
    assert p["one"] and p["name"] == SEGMENTS and p["block"] == 64
    assert p["grid"] == ((groups + 7) // 8 * 8, len(nq))          # grid.x: the largest segment's workgroups, grid.y: the segments


@pytest.mark.parametrize("nq,nt", GPU_CASES)
def test_the_switch_and_every_non_streaming_plan_take_the_loop(exe, nq, nt):
    assert not _plan(exe, 11, True, 2, True, True, True, nq, nt)["one"]            # FDCAP_NN_SEGMENTS=loop
    assert not _plan(exe, 11, False, 1, True, True, True, nq, nt)["one"]           # fdcap_set_nn_kernel(1): the plain scan
    assert not _plan(exe, 11, False, 2, False, True, True, nq, nt)["one"]          # unculled targets (FDCAP_NN_CULL=0 / no seeds)
    assert not _plan(exe, 11, False, 2, True, False, True, nq, nt)["one"]
    assert not _plan(exe, 11, False, 2, True, True, False, nq, nt)["one"]          # seeds not in place
    assert not _plan(exe, 0, False, 2, True, True, True, nq, nt)["one"]            # FDCAP_NN_STREAM=0: the staged kernel
    assert not _plan(exe, 41, False, 2, True, True, True, nq, nt)["one"]           # four waves per group pinned
    p = _plan(exe, 11, True, 2, True, True, True, nq, nt)
    assert p["name"] == "-" and p["grid"] == (0, 0)


def test_by_size_the_largest_segment_decides(exe):
    big, small = 300 * 500, 40 * 500                      # 4688 groups: one wave per group by size; 625 groups: four
    assert _plan(exe, -2, False, 0, True, True, True, (big, big, big), (500000,) * 3)["one"]
    assert _plan(exe, -2, False, 0, True, True, True, (small, big), (500000, 20000))["one"]
    assert not _plan(exe, -2, False, 0, True, True, True, (small, small, small), (500000,) * 3)["one"]
    assert not _plan(exe, -2, False, 0, True, True, True, (2816 * 32 - 32, 100), (500000,) * 2)["one"]
    assert _plan(exe, -2, False, 0, True, True, True, (2816 * 32 - 31, 100), (500000,) * 2)["one"]
    # one segment is the unsegmented launch; more than the kernel argument holds take the loop; a scene beyond the 16-bit work list too
    assert not _plan(exe, 11, False, 2, True, True, True, (big,), (500000,))["one"]
    assert _plan(exe, 11, False, 2, True, True, True, (640,) * 16, (3000,) * 16)["one"]
    assert not _plan(exe, 11, False, 2, True, True, True, (640,) * 17, (3000,) * 17)["one"]
    assert not _plan(exe, 11, False, 2, True, True, True, (big, big), (500000, 16385 * 512))["one"]


def test_the_switch_is_read_in_one_place_and_documented():
    """FDCAP_NN_SEGMENTS is named where segments are defined (fdc_clips.h), read through forms_read_env() alone, and has its row in
    INTEGRATION.md's switch table with the lifetime of every per-optimiser switch"""
    import re
    where = [f for f in sorted(os.listdir(CSRC)) if '"FDCAP_NN_SEGMENTS"' in open(os.path.join(CSRC, f)).read()]
    assert where == ["fdc_clips.h"]
    callers = [f for f in sorted(os.listdir(CSRC)) if re.search(r"clip_segments_loop_env\(\)", open(os.path.join(CSRC, f)).read())]
    assert callers == ["fdc_clips.h", "fdc_forms.h"]
    forms = open(os.path.join(CSRC, "fdc_forms.h")).read()
    assert re.search(r"inline FormSwitches forms_read_env\(\) \{.*?clip_segments_loop_env\(\).*?return s;", forms, re.S)
    rows = [l.split(" | ") for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("| `FDCAP_NN_SEGMENTS")]
    assert len(rows) == 1 and rows[0][1] == "every `fdcap_opt_create[_clips]`"


# ---- the planner ---------------------------------------------------------------------------------------------------
def test_batches_fill_in_input_order_across_scenes():
    clips = [("a", 300), ("b", 300), ("a", 124), ("c", 300), ("b", 40), ("d", 7)]
    assert cli.plan_batches_scenes(clips) == [(["a", "b", "c"], [0, 1, 2, 3]), (["b", "d"], [4, 5])]
    assert cli.plan_batches_scenes([]) == []
    # a clip above the cap is a batch of its own; one row more than fits closes the batch
    assert cli.plan_batches_scenes([("a", 100), ("b", 2000), ("c", 50)]) == [(["a"], [0]), (["b"], [1]), (["c"], [2])]
    assert cli.plan_batches_scenes([("a", 600), ("b", 424), ("c", 1)]) == [(["a", "b"], [0, 1]), (["c"], [2])]


def test_the_row_cap_and_the_scene_cap_hold():
    clips = [(f"s{i % 11}", 10 + i % 7) for i in range(200)]
    for k, rows, scenes in ((None, 1024, 8), (5, 1024, 8), (None, 100, 8), (None, 1024, 3), (None, 1024, 1)):
        batches = cli.plan_batches_scenes(clips, k, row_cap=rows, scene_cap=scenes)
        assert [i for _, idx in batches for i in idx] == list(range(200))                 # input order, every clip once
        for paths, idx in batches:
            assert sum(clips[i][1] for i in idx) <= rows and len(paths) <= scenes and (k is None or len(idx) <= k)
            assert paths == list(dict.fromkeys(clips[i][0] for i in idx))
    nine = [(f"s{i}", 10) for i in range(9)]
    assert cli.plan_batches_scenes(nine) == [([f"s{i}" for i in range(8)], list(range(8))), (["s8"], [8])]
    assert cli.MAX_SCENES == importlib.import_module("fdcap_amd.capi").MAX_SCENES


@pytest.mark.parametrize("k", [None, 1, 3, 100])
def test_clips_of_one_scene_are_plan_batches_mixed_batches(k):
    clips = [("a", n) for n in (300, 300, 300, 124, 300, 300, 101, 7, 1500, 24, 17, 24, 9, 1000, 20, 20)]
    assert [idx for _, idx in cli.plan_batches_scenes(clips, k)] == [idx for _, idx in cli.plan_batches_mixed(clips, k)]
    assert all(paths == ["a"] for paths, _ in cli.plan_batches_scenes(clips, k))


def test_without_the_flag_the_existing_planners_are_what_they_were():
    clips = [("b", 300), ("a", 124), ("b", 40), ("a", 300), ("c", 9)]
    assert cli.plan_batches_mixed(clips) == [("b", [0, 2]), ("a", [1, 3]), ("c", [4])]
    assert cli.plan_batches(clips) == [("b", 300, [0]), ("a", 124, [1]), ("b", 40, [2]), ("a", 300, [3]), ("c", 9, [4])]


def test_mix_scenes_belongs_to_the_multi_clip_form():
    with pytest.raises(SystemExit):
        cli.main(["body/x/results", "fit", "global", "--mix-scenes"])


# ---- the fitter's order ---------------------------------------------------------------------------------------------------
def test_every_scene_becomes_one_run_in_order_of_first_use():
    fitting = importlib.import_module("fdcap_amd.fitting")
    plan = fitting.ClipBatchFitter.plan_scene_runs
    assert plan([0, 1, 0], 2) == ([0, 1], [0, 2, 1])
    assert plan([2, 0, 2, 1, 0], 3) == ([2, 0, 1], [0, 2, 1, 4, 3])
    assert plan([1, 1, 1], 4) == ([1], [0, 1, 2])
    with pytest.raises(ValueError):
        plan([0, 3], 3)
    with pytest.raises(ValueError):
        plan(list(range(9)), 9)
    assert plan(list(range(8)), 8) == (list(range(8)), list(range(8)))
