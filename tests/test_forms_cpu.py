"""Which kernel form every launch takes is a pure function of sizes and switches (csrc/fdc_forms.h).  Pinned here without a GPU:
against tests/forms_table.json -- what the code selected before the policy had a header of its own, recorded over every row count
1 .. 1408 and 2048, twelve vertex sets x 4 / 8 / 12 weights per vertex, four scene sizes, default switches and each value of each
switch the tests use, one at a time -- and against the anchors DESIGN.md and the GPU tests state, written out by hand below so that a
wrong transcription of the table cannot pin itself."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
SRC_DIR = os.path.join(ROOT, "tests", "forms_cpu")
BUILD = os.path.join(ROOT, "tests", "_build")
EXE = os.path.join(BUILD, "forms_sweep")
TABLE = os.path.join(ROOT, "tests", "forms_table.json")

SWITCHES = ["FDCAP_CLIP_FORMS_MIN_ROWS", "FDCAP_PN_RB2", "FDCAP_PN_NW", "FDCAP_PN_KSW", "FDCAP_GEMM_SPLIT3", "FDCAP_NN_STREAM", "FDCAP_NN_SEED",
            "FDCAP_NN_CULL", "FDCAP_NN_ORDER", "FDCAP_NN_CACHE_SLACK", "FDCAP_SKIN_VEC", "FDCAP_FUSE_SKIN", "FDCAP_POSE_TRIM",
            "FDCAP_NN_KEEP_RECORDS", "FDCAP_CONTACT_RECOMPUTE", "FDCAP_NN_BOX_LANES"]


@pytest.fixture(scope="module")
def exe():
    os.makedirs(BUILD, exist_ok=True)
    deps = [os.path.join(SRC_DIR, "sweep.cpp"), os.path.join(SRC_DIR, "sweep_driver.h"), os.path.join(CSRC, "fdc_forms.h")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        # plain g++: the header must not need HIP; -ffp-contract=off: panel_map compares costs in double
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, "-I", SRC_DIR, "-o", EXE,
                               os.path.join(SRC_DIR, "sweep.cpp")])
    return EXE


def _run(exe, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("FDCAP_")}
    return subprocess.run([exe, *args], check=True, capture_output=True, text=True, env=env).stdout.splitlines()


def _fields(text):
    return dict(tok.split("=", 1) for tok in re.split(r" (?=[A-Za-z_]+=)", text) if tok)       # (a form's name may hold blanks)


def _sweep(exe, setting):
    tab = {}
    for line in _run(exe, *([] if setting == "default" else [setting])):
        key, r0, r1, plan, first, last, h = line.split("\t")
        tab.setdefault(key, []).append([int(r0), int(r1), plan, first, last, h])
    return tab


with open(TABLE) as _f:
    _TABLE = json.load(_f)["settings"]


@pytest.mark.parametrize("setting", list(_TABLE))
def test_every_plan_equals_the_recorded_selection(exe, setting):
    want = dict(_TABLE["default"])
    want.update(_TABLE[setting])                      # (a setting lists only the keys it changes)
    got = _sweep(exe, setting)
    assert sorted(got) == sorted(want)
    for key in want:
        assert [r[:2] for r in got[key]] == [r[:2] for r in want[key]], f"{setting}: {key}: the plan changes at other rows"
        for g, w in zip(got[key], want[key]):
            where = f"{setting}: {key}: rows {w[0]}..{w[1]}"
            assert _fields(g[2]) == _fields(w[2]), where
            assert _fields(g[3]) == _fields(w[3]), where + " (first row)"
            assert _fields(g[4]) == _fields(w[4]), where + " (last row)"
            assert g[5] == w[5], where + ": grid / workgroup map differ at some row inside the run"


def _at(exe, query, *settings):
    (line,) = _run(exe, "@" + query, *settings)
    q, plan, per_row = line.split("\t")
    d = _fields(plan)
    d.update(_fields(per_row))
    return d


def test_the_selections_the_documents_and_gpu_tests_state(exe):
    """Contact set of 500 vertices, 4 weights each, reaching 37 joints or fewer: forward panel K = 496, 94 column tiles; gradient panel
    K = 1500, 31 tiles.  Queries: pfwd:rows:vertices, bwd:rows:vertices:may_split, cfwd:rows:vertices:weights:joints,
    skin:rows:vertices:weights, nn:rows:vertices:scene points."""
    at = lambda q, *s: _at(exe, q, *s)
    # BASELINE config 3: 1024 rows, 500 k scene points
    assert at("cfwd:1024:500:4:37")["form"] == "blend_skin_fwd_kernel"
    g = at("bwd:1024:500:1")
    assert g["form"] == "panel_gemm3_rb2k_kernel" and g["two_partials"] == "1"
    assert at("skin:1024:500:4")["form"] == "skin_bwd_vec_kernel"
    s = at("nn:1024:500:500000")
    assert s["groups"] == "16000" and s["form"] == "nn_stream4_kernel<1,1,1>"
    # config 2: 256 rows (a shard of it: 128)
    assert at("cfwd:256:500:4:37")["form"] == "skin_fwd_kernel"
    f = at("pfwd:256:500")
    assert f["form"] == "panel_gemm3_kernel" and f["nw"] == "8"
    assert at("pfwd:128:500")["nw"] == "4"
    for rows, T in ((256, "2"), (128, "1"), (160, "2")):
        g = at(f"bwd:{rows}:500:1")
        assert g["form"] == "panel_gemm3_ksw_kernel" and g["T"] == T, rows
    # waves per query group by the number of groups of 32 queries (32 queries per row: groups = rows)
    for rows, wpg in ((2303, "4"), (2304, "2"), (2815, "2"), (2816, "1")):
        s = at(f"nn:{rows}:32:500000")
        assert s["groups"] == str(rows) and s["wpg"] == wpg, rows
    s = at("nn:128:500:500000")
    assert s["groups"] == "2000" and s["form"] == "nn_stream4_kernel(4 waves per group)"
    # the clip-sized forms: data gradient from 257 rows, forward from 336
    assert at("bwd:256:500:1")["form"] == "panel_gemm3_ksw_kernel" and at("bwd:257:500:1")["form"] == "panel_gemm3_rb2k_kernel"
    assert at("cfwd:335:500:4:37")["form"] == "skin_fwd_kernel" and at("pfwd:335:500")["form"] == "panel_gemm3_kernel"
    assert at("cfwd:336:500:4:37")["form"] == "blend_skin_fwd_kernel"
    assert at("cfwd:336:500:4:37", "FDCAP_FUSE_SKIN=0")["form"] == "skin_fwd_kernel"
    assert at("pfwd:336:500", "FDCAP_FUSE_SKIN=0")["form"] == "panel_gemm3_rb2_kernel"
    # a 300-row clip (what test_gpu_fullsize_golden.py asserts)
    assert [at("cfwd:300:500:4:37")["form"], at("pfwd:300:500")["form"], at("bwd:300:500:1")["form"]] == \
        ["skin_fwd_kernel", "panel_gemm3_kernel", "panel_gemm3_rb2k_kernel"]
    m = "FDCAP_CLIP_FORMS_MIN_ROWS=256"
    assert at("cfwd:256:500:4:37", m)["form"] == "blend_skin_fwd_kernel" and at("cfwd:255:500:4:37", m)["form"] == "skin_fwd_kernel"
    assert at("bwd:256:500:1", m)["form"] == "panel_gemm3_rb2k_kernel" and at("bwd:255:500:1", m)["form"] == "panel_gemm3_ksw_kernel"
    assert at("pfwd:256:500", m)["form"] == "panel_gemm3_rb2_kernel" and at("pfwd:255:500", m)["form"] == "panel_gemm3_kernel"
    # config 5: 512 rows, all 10 475 vertices (1965 forward tiles)
    f = at("pfwd:512:10475")
    assert (f["form"], f["cs"], f["grid"]) == ("panel_gemm3_wide_kernel", "2", "256")
    g = at("bwd:512:10475:1")
    assert (g["form"], g["ks"], g["grid"]) == ("panel_gemm3_kloop_kernel", "8", "256")
    g = at("bwd:384:10475:1")
    assert (g["ks"], g["grid"]) == ("8", "192")
    assert at("skin:512:10475:4")["form"] == "skin_bwd_kernel(chunks, MFMA dA)"
    # the K-split form reaches K = 1536; the K-loop form from K = 1664 at >= 384 rows and K = 1904 at >= 192 rows; at 128 rows one image up to K = 2528
    assert at("bwd:1024:512:1")["form"] == "panel_gemm3_rb2k_kernel" and at("bwd:1024:513:1")["form"] != "panel_gemm3_rb2k_kernel"
    kloop = "panel_gemm3_kloop_kernel"
    assert at("bwd:384:555:1")["form"] == kloop and at("bwd:383:555:1")["form"] != kloop and at("bwd:384:554:1")["form"] != kloop
    assert at("bwd:192:635:1")["form"] == kloop and at("bwd:191:635:1")["form"] != kloop and at("bwd:192:634:1")["form"] != kloop
    assert at("bwd:128:842:1")["form"] in ("panel_gemm3_ksw_kernel", "panel_gemm3_kernel") and at("bwd:128:843:1")["form"] == kloop


def test_every_plan_of_the_sweep_can_be_launched(exe):
    """Dynamic LDS within a gfx950 CU's 160 KB (150 KB for the two kernels whose attribute is raised to 150 KB), a grid of at least one
    workgroup, and for the K-loop product ks x column blocks a multiple of 8 (the gradient panel has 31 tiles = 2 column blocks of
    16 tiles, so ks = 4 is admissible at every size)."""
    n = 0
    for line in _run(exe, "--every-row"):
        key, r0, r1, plan, first, last, h = line.split("\t")
        p, g = _fields(plan), _fields(first)
        lds = int(p.get("lds", 0))
        cap = 150 * 1024 if p["form"] in ("panel_gemm3_kloop_kernel", "blend_skin_fwd_kernel") else 160 * 1024
        assert lds <= cap, line
        assert int(p.get("max_lds", lds)) >= lds and int(p.get("max_lds", 0)) <= 160 * 1024, line
        assert all(int(v) >= 1 for v in g["grid"].split(",")), line
        if p["form"] == "panel_gemm3_kloop_kernel":
            assert 1 <= int(p["ks"]) <= 64 and (int(p["ks"]) * 2) % 8 == 0, line
        n += 1
    assert n > 200_000


def test_the_switches_are_read_in_one_place_and_documented():
    names = set()
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f)).read()
        read = set(re.findall(r'"(FDCAP_[A-Z0-9_]+)"', text))
        if f == "fdc_forms.h":
            names = read
        else:
            assert not (read & set(SWITCHES)), f"{f} reads {sorted(read & set(SWITCHES))}: selection switches belong to fdc_forms.h"
    assert names == set(SWITCHES)
    rows = [l for l in open(os.path.join(ROOT, "INTEGRATION.md")).read().splitlines() if l.startswith("| `")]
    process, create = "once per process", "every `fdcap_opt_create[_clips]`"
    when = {"FDCAP_CLIP_FORMS_MIN_ROWS": process, "FDCAP_PN_RB2": process, "FDCAP_PN_NW": process, "FDCAP_PN_KSW": process, "FDCAP_NN_STREAM": process,
            "FDCAP_GEMM_SPLIT3": process + " (`fdcap_panel_gemm`: every call)", "FDCAP_NN_SEED": create, "FDCAP_NN_CULL": create,
            "FDCAP_SKIN_VEC": create, "FDCAP_FUSE_SKIN": create, "FDCAP_NN_ORDER": create, "FDCAP_POSE_TRIM": create,
            "FDCAP_NN_KEEP_RECORDS": create, "FDCAP_CONTACT_RECOMPUTE": create, "FDCAP_NN_BOX_LANES": create,
            "FDCAP_NN_CACHE_SLACK": create + " (`fdcap_chamfer_fwd_scene`: once per process)"}
    for name in SWITCHES:
        mine = [l.split(" | ") for l in rows if f"`{name}" in l.split(" | ")[0]]
        assert len(mine) == 1, f"{name}: one row in INTEGRATION.md's switch table"
        assert mine[0][1] == when[name], name
