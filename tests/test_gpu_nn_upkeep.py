"""WHEN the in-loop Chamfer search rebuilds its query order (fdc_chamfer.h nn_stream_upkeep, fdc_forms.h nn_order_period) is
scheduling only: the order decides which queries share a wave and when a group runs, never what a query returns.  So a fit under the
growing period (FDCAP_NN_ORDER=8: periods 8 8 8 16 32 64 ...), a fit without any order (=0) and a fit under the default base (=32)
return the same bytes -- and the number of rebuilds a fit did is the number the CPU rule (tests/nn_upkeep_rule.py) gives for its
search launches, in every fit on one optimiser: the count restarts with the fit's seeding launch.

Shapes: a 400-vertex body with every vertex a contact, 226 frames, a 20 000-point scene, 140 iterations = 112 phase-1 iterations
with one search launch each (the search runs in phase 1).  226 x 400 queries are 2 825 groups of 32, the smallest clip of this body
whose search takes the one-wave form under default switches (from 2 816 groups: plan_nn_search, fdc_forms.h) -- the only form that
takes a query order.  Base 8 puts rebuilds behind launches 1, 10, 19, 28, 45 and 78 of the 112: six rebuilds, three period changes.

Cases: the plain clip; the clip with one frame whose parameters are NaN (its queries have no neighbour and sort last); a batch of two
clips of two scenes, which runs the segmented search with one order state per segment.  A batch of 2 x 113 frames does NOT reach the
segmented one-launch form: that form is taken when the LARGEST segment's own plan is the one-wave form (plan_nn_segments), and 113
frames are 1 413 groups (four waves per group, no order at all).  The smallest batch that takes it has one segment of 226 frames;
the second segment here has 113, so the two segments differ in size, and both run under an order of their own.

The query order's radix sort, at the tile edges (a scatter block takes 2 048 or 4 096 keys, by the query count) and with key
patterns at the digit boundary of its two 8-bit passes, against numpy's stable argsort: exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.fitting import ClipBatchFitter, first_phase2_iter
from fdcap_amd.io import read_camerapose
from tests.nn_upkeep_rule import build_exe, rebuilds_within

pytestmark = pytest.mark.gpu

V, N, NS, ITERS = 400, 226, 20_000, 140
N_SMALL = 113                                               # the second segment of the two-scene batch
LAUNCHES = first_phase2_iter(ITERS)                         # search launches of a fit
BASE = 8
ONE_WAVE, SEGMENTS = "nn_stream4_kernel<1,1,1>", "nn_stream4_kernel(1 wave per group, segments)"
SWITCHES = ("FDCAP_NN_ORDER", "FDCAP_NN_CACHE_SLACK", "FDCAP_NN_SEED", "FDCAP_NN_CULL", "FDCAP_NN_KEEP_RECORDS", "FDCAP_CONTACT_RECOMPUTE",
            "FDCAP_SKIN_VEC", "FDCAP_FUSE_SKIN", "FDCAP_POSE_TRIM", "FDCAP_NN_BOX_LANES", "FDCAP_NN_SEGMENTS")      # (read by every fdcap_opt_create)
CASES = ("plain", "nan_frame", "two_scenes")
NAN_FRAME = 7


@pytest.fixture(scope="module")
def model():
    bm = synth.make_body_model(V, seed=181)
    scene_b = (synth.make_scene(NS + 777, seed=184) + np.array([0.0, 0.0, 0.3], np.float32)).astype(np.float32)
    return bm, synth.make_vposer(seed=182), {"A": synth.make_scene(NS, seed=183), "B": scene_b}


def _clip(n, seed, nan_frame=None):
    c = synth.make_clip(n, seed=seed)
    body = np.array(c.body_params, copy=True)
    if nan_frame is not None:
        body[nan_frame, 0:3] = np.nan
    return body, read_camerapose(c.camerapose_lines)


def _forms(reset):
    buf = ctypes.create_string_buffer(4096)
    capi.check(capi.load_library().fdcap_debug_kernel_forms(buf, len(buf), 1 if reset else 0), "kernel_forms")
    return buf.value.decode()


def _fits(model, case, order, fits=1):
    """`fits` fits of the case on ONE optimiser state under FDCAP_NN_ORDER=order -> per fit (the arrays, the diet counters, the
    one-wave launches by box width, the forms)"""
    bm, vp, scenes = model
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ["FDCAP_NN_ORDER"] = str(order)
    f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=np.arange(V))
    out = []
    try:
        if case == "two_scenes":
            f.ctx.set_scene_slot(0, scenes["A"])
            f.ctx.set_scene_slot(1, scenes["B"])
            clips, slots = [_clip(N, 191), _clip(N_SMALL, 192)], [0, 1]
        else:
            f.set_scene(scenes["A"])
            clips, slots = [_clip(N, 191, NAN_FRAME if case == "nan_frame" else None)], None
        rows = sum(len(b) for b, _ in clips)
        lib, h = f.ctx.lib, f.ctx.handle
        for _ in range(fits):
            _forms(True)
            f.prepare(clips, clip_slots=slots)              # fdcap_opt_create*: the optimiser state is reused, its order state starts over
            res = f.run()
            d = torch.empty(rows, V, device="cuda")
            i = torch.empty(rows, V, device="cuda", dtype=torch.int32)
            capi.check(lib.fdcap_opt_sync(h, capi.current_stream()), "sync")
            capi.check(lib.fdcap_opt_get_contact(h, capi.dptr(d), capi.dptr(i), capi.current_stream()), "get_contact")
            torch.cuda.synchronize()
            arrays = {"dist": d.cpu().numpy(), "idx": i.cpu().numpy()}
            for k, (body_rec, scale, cam) in enumerate(res):
                arrays[f"body_rec{k}"] = body_rec.cpu().numpy()
                arrays[f"scale{k}"] = np.asarray(scale, dtype=np.float32).reshape(1)
                arrays[f"camera_ext{k}"] = cam.cpu().numpy()
            diet, box = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
            capi.check(lib.fdcap_debug_contact_diet(h, diet), "contact_diet")
            capi.check(lib.fdcap_debug_nn_box_tests(h, box), "nn_box_tests")
            out.append((arrays, tuple(diet), tuple(box), _forms(False)))
    finally:
        f.close()
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v
    return out


_RUNS = {}


def _run(model, case, order):
    """computed once per (case, order), shared by the tests, never changed; base 8 runs two fits on its optimiser"""
    if (case, order) not in _RUNS:
        _RUNS[(case, order)] = _fits(model, case, order, fits=2 if order == BASE else 1)
    return _RUNS[(case, order)]


def _same_bytes(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert a[k].tobytes() == b[k].tobytes(), k          # bytes, not values: a frame without neighbours carries NaNs


@pytest.mark.parametrize("case", CASES)
def test_rebuild_schedule_moves_no_byte(model, case):
    got = _run(model, case, BASE)[0]
    form = SEGMENTS if case == "two_scenes" else ONE_WAVE
    for other in (0, 32):
        want = _run(model, case, other)[0]
        assert form in want[3] and form in got[3], (want[3], got[3])
        _same_bytes(got[0], want[0])
    nseg = 2 if case == "two_scenes" else 1
    assert _run(model, case, 0)[0][1][2:] == (0, 0)          # no order: no launch under one, no rebuild
    assert got[1][2] == nseg * (LAUNCHES - 1), got[1]        # every launch but the seeding one ran under a query order
    idx = got[0]["idx"]
    if case == "nan_frame":
        assert (idx[NAN_FRAME] < 0).all() and idx[:NAN_FRAME].min() >= 0 and idx[NAN_FRAME + 1:].min() >= 0
    else:
        assert idx.min() >= 0 and np.isfinite(got[0]["dist"]).all()
    assert len(np.unique(idx[idx >= 0])) > 32                # (more neighbours than a wave has queries: the order has something to group)


@pytest.mark.parametrize("case", CASES)
def test_rebuild_count_is_the_cpu_rule_s_in_every_fit(model, case):
    exe = build_exe(True)
    nseg = 2 if case == "two_scenes" else 1
    assert LAUNCHES == 112
    first, second = _run(model, case, BASE)
    if nseg == 1:
        assert sum(first[2]) == LAUNCHES and sum(second[2]) == LAUNCHES, (first[2], second[2])     # one-wave launches of each fit
    want = rebuilds_within(exe, BASE, LAUNCHES, N * V)        # (both segments' orders are below the size where the period stops growing)
    assert want == 6                                         # behind launches 1, 10, 19, 28, 45, 78 (tests/test_nn_upkeep_cpu.py)
    assert first[1][3] == nseg * want, first[1]
    assert second[1][3] == nseg * want, second[1]            # the counter restarted with the second fit's seeding launch
    _same_bytes(first[0], second[0])
    assert _run(model, case, 32)[0][1][3] == nseg * rebuilds_within(exe, 32, LAUNCHES) == nseg * 4      # launches 1, 34, 67, 100


# ---- the sort ----------------------------------------------------------------------------------------------------------
SORT_SIZES = (1, 2047, 2048, 2049, 70_001)
SORT_PATTERNS = ("all_equal", "ascending", "descending", "all_16_bits", "high_byte_only")


def _keys(pattern, nq):
    rng = np.random.default_rng(1800 + 31 * SORT_PATTERNS.index(pattern) + nq % 1009)
    if pattern == "all_equal":
        key = np.full(nq, 0x1234)
    elif pattern == "ascending":                             # (non-decreasing where there are more queries than keys)
        key = (np.arange(nq, dtype=np.int64) * 0x10000) // max(nq, 1)
    elif pattern == "descending":
        key = 0xFFFE - (np.arange(nq, dtype=np.int64) * 0xFFFF) // max(nq, 1)
    elif pattern == "all_16_bits":                           # both digits take every value, 0xFFFF (the "no neighbour" key) included
        key = rng.integers(0, 0x10000, nq)
        key[: min(nq, 4)] = [0xFFFF, 0x0000, 0x00FF, 0xFF00][: min(nq, 4)]
    else:                                                    # the low digit is one value: pass 0 moves nothing, pass 1 does all the work
        key = (rng.integers(0, 256, nq) << 8) | 0x5A
    return np.ascontiguousarray(key, dtype=np.int64)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(synth.make_body_model(V, seed=181), synth.make_vposer(seed=182))
    yield c
    c.close()


def _check_sort(ctx, nq, pattern):
    key = _keys(pattern, nq)
    assert key.min() >= 0 and key.max() <= 0xFFFF
    if pattern == "all_16_bits" and nq > 70_000:
        assert len(np.unique(key & 255)) == 256 and len(np.unique(key >> 8)) == 256
    if pattern == "high_byte_only" and nq >= 2047:
        assert len(np.unique(key & 255)) == 1 and len(np.unique(key >> 8)) > 200
    rng = np.random.default_rng(nq)
    pos = ((key << 7) + rng.integers(0, 128, nq)).astype(np.int32)       # the key is pos >> 7: the low seven bits must not matter
    ref = np.argsort(key, kind="stable").astype(np.int32)
    groups = (nq + 31) // 32
    hdr = np.arange(groups + 5, dtype=np.int32) + 11
    perm = np.full(nq, -7, np.int32)
    capi.check(ctx.lib.fdcap_debug_nn_query_sort(ctx.handle, pos.ctypes.data_as(ctypes.c_void_p), nq, groups, len(hdr),
                                                 hdr.ctypes.data_as(ctypes.c_void_p), perm.ctypes.data_as(ctypes.c_void_p), None), "nn_query_sort")
    bad = np.flatnonzero(perm != ref)
    assert not len(bad), f"{len(bad)} of {nq} slots differ, first at slot {bad[0]}: {perm[bad[0]]} for {ref[bad[0]]}"
    assert (hdr[:groups] == -1).all() and np.array_equal(hdr[groups:], np.arange(groups, groups + 5, dtype=np.int32) + 11)


@pytest.mark.parametrize("pattern", SORT_PATTERNS)
@pytest.mark.parametrize("nq", SORT_SIZES)
def test_sort_at_tile_edges_and_digit_boundaries(ctx, nq, pattern):
    _check_sort(ctx, nq, pattern)


# nn_query_order_rounds (fdc_scene.h): 2 048-key tiles while 4 096-key tiles would be fewer than 256 blocks, i.e. up to
# 255 x 4 096 queries; from one query more, 4 096-key tiles.  Both sides of that size, and config 3's 512 000 (250 tiles of 2 048).
@pytest.mark.parametrize("pattern", ["all_16_bits", "descending"])
@pytest.mark.parametrize("nq", [512_000, 255 * 4096, 255 * 4096 + 1])
def test_sort_on_both_sides_of_the_tile_choice(ctx, nq, pattern):
    _check_sort(ctx, nq, pattern)
