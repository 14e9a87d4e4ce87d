"""r21: the key of the in-loop search's query order is the k-d node of each query's neighbour at a shift the scene's size selects
(csrc/fdc_forms.h nn_order_key_shift: 5, the 32-point tile, wherever the tiles fit the 16-bit key), no longer the quarter (7) alone.
Scheduling only: every key gives the same neighbours, distances and fit, bit for bit.

Sort: fdcap_debug_nn_query_sort_shift against numpy's stable argsort of min(pos >> s, 0xFFFF) for s = 5 and 6 -- sizes 1, 63, 4097
(two 2048-key tiles and one key) and 70 000 (35 tiles, more keys than the 65 536 key values), the "uniform", "descending" and
"clamped" patterns of tests/test_gpu_query_sort.py, whose shift-7 cases stay where they are.

Search: fdcap_chamfer_fwd_scene under FDCAP_NN_STREAM=11 -- the one-wave form with kept work lists, no query order -- with 4 and 8
work items per chunk against nn_direct_kernel's every-pair scan and against each other, byte for byte: 3 x 32 + 5 queries on a
2048-point scene (four chunks), on a 300-point scene (padding rows), on a doubled lattice (exact ties, duplicate points) and with NaN
queries (their own three records: 4 against 8 items alone); four launches each -- seeding, the kept lists, the queries 3 cm further (the lists are void), the new lists.  (The order's
key only reaches a launch through the optimiser's query order: the fits below cross it with the items.)

Fit: a 19-frame clip (608 queries, 19 one-wave groups) on a 3 000-point scene under two contact sets, with log_every 0 and 1: the
automatic form and every (key_shift, items_per_chunk) of {7, 6, 5} x {4, 8} against fdcap_debug_nn_search_form(7, 4), the order and
the items every earlier build had -- parameters, scale, cameras, the logged sums, the last search's distances and neighbours and its
neighbour records.  A (7, 6, 6) batch of clips on one scene and on scenes (A, B, A), where every segment has its own order.

Search and fits run in a child process (this file as a script) under FDCAP_NN_STREAM=11, read once per process, and
fdcap_set_nn_kernel(2): only the one-wave form has a query order and work items of two sizes, and the size rule gives launches this
small the four-wave form."""
import ctypes
import json
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.fitting import ClipBatchFitter, FittingOP
from fdcap_amd.io import read_camerapose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_WAVE, SEGMENTS = "nn_stream4_kernel<1,1,1>", "nn_stream4_kernel(1 wave per group, segments)"
E_ARG, E_STATE = -1, -2
SIZES = (1, 63, 4097, 70000)
PATTERNS = ("uniform", "descending", "clamped")
SHIFTS = (5, 6)
TAIL = 11
N, ITERS = 19, 40
# (key_shift, items_per_chunk): the first is the reference -- the order and the work items of every earlier build --, then automatic
FORMS = ((7, 4), (0, 0), (7, 8), (6, 4), (6, 8), (5, 4), (5, 8))
FIELDS = ("iters", "l_rec", "l_vposer", "loss_smoothing", "loss_contact", "loss_world_smoothing", "total")


# ---- the sort ---------------------------------------------------------------------------------------------------------------------
def _positions(pattern, nq, shift):
    rng = np.random.default_rng(100 * PATTERNS.index(pattern) + nq % 991 + shift)
    if pattern == "uniform":                          # config 3's scene: tiles 0 .. 15 624 under shift 5, both digits populated
        pos = rng.integers(0, 500000, nq)
    elif pattern == "descending":                     # nodes descend (strictly up to 65 536 queries, then in runs of equal length)
        step = (nq + 65535) // 65536
        pos = ((nq - 1 - np.arange(nq)) // step) << shift
    else:                                             # clamped: nodes from 0xFFFF on clamp and tie with the -1 sentinel
        pos = rng.integers(0, 1 << 24, nq)
        pos[rng.random(nq) < 0.02] = -1
    return np.ascontiguousarray(pos, dtype=np.int32)


def _reference(pos, shift):
    key = np.where(pos >= 0, np.minimum(pos >> shift, 0xFFFF), 0xFFFF)
    return key, np.argsort(key, kind="stable").astype(np.int32)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nq", SIZES)
def test_reference_has_the_properties_the_patterns_are_for(nq, pattern, shift):
    pos = _positions(pattern, nq, shift)
    key, ref = _reference(pos, shift)
    assert np.array_equal(np.sort(ref), np.arange(nq))
    if pattern == "descending" and nq > 1:
        assert key[0] == key.max() and key[-1] == 0 and (np.diff(key) <= 0).all() and (nq > 65536 or (np.diff(key) < 0).all())
    if pattern == "clamped" and nq >= 4097:
        assert (pos < 0).any() and ((pos >> shift) > 0xFFFF).any()
        last = np.flatnonzero(key == 0xFFFF)
        assert np.array_equal(ref[nq - len(last):], last)
    if pattern == "uniform" and nq >= 4097:
        assert len(np.unique(key & 255)) == 256 and len(np.unique(key >> 8)) > 8
        assert not np.array_equal(ref, _reference(pos, 7)[1])               # a finer key is another order


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(synth.make_body_model(400, seed=0), synth.make_vposer(seed=1))
    yield c
    c.close()


def _sort(ctx, pos, groups, hdr, shift):
    perm = np.full(len(pos), -7, np.int32)
    code = ctx.lib.fdcap_debug_nn_query_sort_shift(ctx.handle, pos.ctypes.data_as(ctypes.c_void_p), len(pos), groups, len(hdr),
                                                   hdr.ctypes.data_as(ctypes.c_void_p), perm.ctypes.data_as(ctypes.c_void_p), shift, None)
    return code, perm


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("nq", SIZES)
def test_sort_by_the_shifted_key_is_the_stable_order(ctx, nq, pattern, shift):
    pos = _positions(pattern, nq, shift)
    _, ref = _reference(pos, shift)
    groups = (nq + 31) // 32
    fill = (5 * np.arange(groups + TAIL) + 2).astype(np.int32)
    hdr = fill.copy()
    code, perm = _sort(ctx, pos, groups, hdr, shift)
    capi.check(code, "fdcap_debug_nn_query_sort_shift")
    bad = np.flatnonzero(perm != ref)
    assert not len(bad), f"{len(bad)} of {nq} slots differ, first at slot {bad[0]}: {perm[bad[0]]} for {ref[bad[0]]}"
    assert (hdr[:groups] == -1).all() and np.array_equal(hdr[groups:], fill[groups:])


@pytest.mark.gpu
def test_shift_seven_is_the_quarter_sort_and_other_shifts_are_refused(ctx):
    pos = _positions("uniform", 4097, 7)
    groups = (len(pos) + 31) // 32
    code, perm = _sort(ctx, pos, groups, np.zeros(groups, np.int32), 7)
    capi.check(code, "fdcap_debug_nn_query_sort_shift")
    old = np.full(len(pos), -7, np.int32)
    hdr = np.zeros(groups, np.int32)
    capi.check(ctx.lib.fdcap_debug_nn_query_sort(ctx.handle, pos.ctypes.data_as(ctypes.c_void_p), len(pos), groups, groups,
                                                 hdr.ctypes.data_as(ctypes.c_void_p), old.ctypes.data_as(ctypes.c_void_p), None), "sort")
    assert np.array_equal(perm, old) and np.array_equal(perm, _reference(pos, 7)[1])
    for shift in (4, 8, 0, -1):
        code, perm = _sort(ctx, pos, groups, np.zeros(groups, np.int32), shift)
        assert code == E_ARG and (perm == -7).all()


# ---- fits (child process) -----------------------------------------------------------------------------------------------------------
def _forms(reset):
    buf = ctypes.create_string_buffer(4096)
    capi.load_library().fdcap_debug_kernel_forms(buf, 4096, 1 if reset else 0)
    return buf.value.decode()


def _set_form(lib, h, form):
    capi.check(lib.fdcap_debug_nn_search_form(h, form[0], form[1]), "fdcap_debug_nn_search_form")


def _fit(bm, vp, scene, vid, clip, log_every, form):
    """one stand-alone fit with the search's form set right after the optimiser exists; everything it computed, as bytes-comparable arrays"""
    fop = FittingOP({"num_iter": ITERS}, {}, N, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                    camera_ext=read_camerapose(clip.camerapose_lines))
    lib, h = fop.ctx.lib, fop.ctx.handle
    init = fop.init

    def init_then_form(x78):
        r = init(x78)
        _set_form(lib, h, form)
        return r
    fop.init = init_then_form
    _forms(True)
    b, s, c = fop.fitting(torch.tensor(clip.body_params).cuda(), "global", log_every=log_every)
    nc = len(vid)
    d = torch.empty(N, nc, device="cuda")
    i = torch.empty(N, nc, device="cuda", dtype=torch.int32)
    rec = torch.empty(N, nc, 4, device="cuda")
    capi.check(lib.fdcap_opt_sync(h, capi.current_stream()), "sync")
    capi.check(lib.fdcap_opt_get_contact(h, capi.dptr(d), capi.dptr(i), capi.current_stream()), "get_contact")
    capi.check(lib.fdcap_debug_nn_records(h, capi.dptr(rec), capi.current_stream()), "nn_records")
    torch.cuda.synchronize()
    diet = (ctypes.c_int32 * 4)()
    capi.check(lib.fdcap_debug_contact_diet(h, diet), "contact_diet")
    out = {"body": b.cpu().numpy(), "scale": np.float64(s), "cam": c.cpu().numpy(), "dist": d.cpu().numpy(), "idx": i.cpu().numpy(),
           "records": rec.cpu().numpy().view(np.int32)}
    if log_every:
        out.update({"log_" + f: np.array(getattr(fop.log, f), dtype=np.float64) for f in FIELDS})
    forms = _forms(False)
    fop.close()
    assert ONE_WAVE in forms, forms                              # the form that takes a query order ...
    assert diet[2] > 0 and diet[3] >= 1, list(diet)             # ... ran under one, rebuilt after the seeding launch
    return out


def _differs(a, b):
    return [k for k in a if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]


def _sc_fit():
    bm = synth.make_body_model(300, seed=131)
    vp = synth.make_vposer(seed=132)
    scene = synth.make_scene(3000, seed=134)
    clip = synth.make_clip(N, seed=61, num_outliers=2)
    bad = []
    for per_part, seed in ((16, 135), (16, 211)):                # two contact sets of 2 x 16 vertices
        l, r = synth.make_contact_ids(bm.v_template, per_part=per_part, seed=seed)
        vid = np.concatenate([l, r])
        for log_every in (0, 1):
            ref = _fit(bm, vp, scene, vid, clip, log_every, FORMS[0])
            assert np.isfinite(ref["body"]).all() and (ref["idx"] >= 0).all()
            for form in FORMS[1:]:
                d = _differs(ref, _fit(bm, vp, scene, vid, clip, log_every, form))
                if d:
                    bad.append(f"contacts {seed} log_every {log_every} form {form}: {d}")
    assert not bad, bad
    return "ok"


def _sc_batch():
    bm = synth.make_body_model(300, seed=131)
    vp = synth.make_vposer(seed=132)
    l, r = synth.make_contact_ids(bm.v_template, per_part=16, seed=135)
    vid = np.concatenate([l, r])
    scenes = [synth.make_scene(3000, seed=134), (synth.make_scene(4133, seed=137) + np.array([0.0, 0.0, 0.3], np.float32)).astype(np.float32)]
    clips = []
    for seed, n in ((61, 7), (62, 6), (63, 6)):
        c = synth.make_clip(n, seed=seed, num_outliers=0)
        clips.append((c.body_params, read_camerapose(c.camerapose_lines)))
    bad = []
    for slots, want in ((None, ONE_WAVE), ([0, 1, 0], SEGMENTS)):
        res = {}
        for form in FORMS:
            f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
            try:
                for k, sc in enumerate(scenes):
                    f.ctx.set_scene_slot(k, sc)
                f.prepare(clips, clip_slots=slots)
                _set_form(f.ctx.lib, f.ctx.handle, form)
                _forms(True)
                out = f.run(1)
                forms = _forms(False)
                assert want in forms, forms
                res[form] = {}
                for k, (b, s, c) in enumerate(out):
                    res[form].update({f"body{k}": b.cpu().numpy(), f"scale{k}": np.float64(s), f"cam{k}": c.cpu().numpy()})
                    res[form].update({f"log{k}_" + fl: np.array(getattr(f.logs[k], fl), dtype=np.float64) for fl in FIELDS})
            finally:
                f.close()
        for form in FORMS[1:]:
            d = _differs(res[FORMS[0]], res[form])
            if d:
                bad.append(f"slots {slots} form {form}: {d}")
    assert not bad, bad
    return "ok"


def _sc_refusals():
    ctx = capi.Context(synth.make_body_model(300, seed=131), synth.make_vposer(seed=132))
    try:
        lib, h = ctx.lib, ctx.handle
        got = {a: lib.fdcap_debug_nn_search_form(h, *a) for a in ((4, 0), (8, 4), (-1, 0), (5, 2), (0, 16), (7, 6), (0, -4))}
        assert all(v == E_ARG for v in got.values()), got
        assert lib.fdcap_debug_nn_search_form(None, 0, 0) == E_STATE
        assert all(lib.fdcap_debug_nn_search_form(h, *a) == 0 for a in FORMS + ((0, 0),))      # (no optimiser, no scene: nothing to drop)
    finally:
        ctx.close()
    return "ok"


# ---- the search alone: fdcap_chamfer_fwd_scene, the one-wave form with kept lists, against the every-pair scan -------------------------
NQ = 3 * 32 + 5                                              # three whole groups and a ragged one


def _bits(d, i):
    torch.cuda.synchronize()
    return d.cpu().numpy().view(np.int32).copy(), i.cpu().numpy().copy()


def _scan(ctx, q, scene_d):
    """nn_direct_kernel over every (query, scene point) pair"""
    d = torch.empty(1, NQ, device="cuda")
    i = torch.empty(1, NQ, device="cuda", dtype=torch.int32)
    capi.check(ctx.lib.fdcap_set_nn_kernel(1), "fdcap_set_nn_kernel")
    try:
        capi.check(ctx.lib.fdcap_chamfer_fwd(ctx.handle, capi.dptr(q), capi.dptr(scene_d), 1, NQ, scene_d.shape[0], 0, capi.dptr(d),
                                             capi.dptr(i), None, None, capi.current_stream()), "fdcap_chamfer_fwd")
    finally:
        capi.check(ctx.lib.fdcap_set_nn_kernel(2), "fdcap_set_nn_kernel")
    return _bits(d, i)


def _search(ctx, q, forget):
    d = torch.empty(1, NQ, device="cuda")
    i = torch.empty(1, NQ, device="cuda", dtype=torch.int32)
    capi.check(ctx.lib.fdcap_chamfer_fwd_scene(ctx.handle, capi.dptr(q), 1, NQ, capi.dptr(d), capi.dptr(i), forget, capi.current_stream()),
               "fdcap_chamfer_fwd_scene")
    return _bits(d, i)


def _search_cases():
    rng = np.random.default_rng(2100)
    out = {}
    for name, ns in (("2048 points, four chunks", 2048), ("300 points, padding rows", 300)):
        xyz = synth.make_scene(ns, seed=140 + ns % 7)
        q = xyz[rng.integers(0, ns, NQ)] + np.concatenate([rng.normal(0, 0.02, (NQ, 2)), rng.uniform(0.05, 0.3, (NQ, 1))], 1)
        out[name] = (xyz, q.astype(np.float32))
    # exact ties and duplicate points: a 16 x 16 x 4 lattice of pitch 1/4 m, every point twice; queries ON lattice points (two
    # copies tie), at edge midpoints (four points tie) and at cell centres (sixteen tie) -- every coordinate exact in fp32
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(4), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 0.25
    lattice = np.concatenate([g, g])[rng.permutation(2048)]
    base = g[rng.integers(0, len(g), NQ)]
    off = np.zeros((NQ, 3), np.float32)
    off[NQ // 3:2 * NQ // 3, 0] = 0.125
    off[2 * NQ // 3:] = 0.125
    out["ties and duplicates"] = (lattice, base + off)
    xyz, q = out["2048 points, four chunks"]
    q = q.copy()
    q[7], q[40, 1], q[NQ - 1, 2] = np.nan, np.nan, np.nan
    out["NaN queries"] = (xyz, q)
    return out


def _sc_search():
    ctx = capi.Context(synth.make_body_model(300, seed=131), synth.make_vposer(seed=132))
    bad = []
    try:
        lib, h = ctx.lib, ctx.handle
        for name, (xyz, q0) in _search_cases().items():
            ctx.set_scene(xyz)
            scene_d = torch.tensor(xyz, device="cuda")
            # launches: seeding | the kept lists | the queries 3 cm further: the lists are void (3 cm of slack) | the new lists
            steps = [q0, q0, q0 + np.array([0.03, 0.0, 0.0], np.float32), q0 + np.array([0.03, 0.0, 0.0], np.float32)]
            qs = [torch.tensor(x.reshape(1, NQ, 3), device="cuda") for x in steps]
            ref = [_scan(ctx, x, scene_d) for x in qs]
            real = ~np.isnan(q0).any(1)                       # (a NaN query has no neighbour; how the scan spells that is its own: 4 against 8 below)
            assert real.sum() >= NQ - 3 and all((r[1][0, real] >= 0).all() for r in ref)
            got = {}
            for items in (4, 8):
                _set_form(lib, h, (7, items))
                _forms(True)
                got[items] = [_search(ctx, x, 1 if k == 0 else 0) for k, x in enumerate(qs)]
                assert ONE_WAVE in _forms(False)
                for k, ((sd, si), (rd, ri)) in enumerate(zip(got[items], ref)):
                    n = int(((sd != rd) | (si != ri))[0, real].sum())
                    if n:
                        bad.append(f"{name}, {items} items per chunk, launch {k}: {n} of {NQ} queries differ from the scan")
            for k in range(len(qs)):
                if not (np.array_equal(got[4][k][0], got[8][k][0]) and np.array_equal(got[4][k][1], got[8][k][1])):
                    bad.append(f"{name}, launch {k}: 4 and 8 items per chunk differ")
        _set_form(lib, h, (0, 0))
    finally:
        ctx.close()
    assert not bad, bad
    return "ok"


_SCENARIOS = {"search": _sc_search, "fit": _sc_fit, "batch": _sc_batch, "refusals": _sc_refusals}


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ)
    env["FDCAP_NN_STREAM"] = "11"
    env["FDCAP_CLIP_FORMS_MIN_ROWS"] = "1024"
    env.pop("FDCAP_NN_SEGMENTS", None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and line, (p.stdout[-1500:], p.stderr[-3000:])
    return json.loads(line[-1][7:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_SCENARIOS))
def test_scenario(child, name):
    assert child[name] == "ok", child[name]


if __name__ == "__main__":
    assert capi.load_library().fdcap_set_nn_kernel(2) == 0          # (the matrix-pipe search at every size: the streaming forms are its)
    result = {}
    for name, fn in _SCENARIOS.items():
        try:
            result[name] = fn()
        except Exception:
            result[name] = traceback.format_exc()[-2500:]
    print("RESULT " + json.dumps(result))
