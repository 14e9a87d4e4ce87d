"""The collision search (csrc/fdc_collide.h) at the production tree and at its input edges: every tree shape the header distinguishes
up to the 1024-leaf limit, more frames than one block of the frame sum, every return of the penalty's Y(h), unusable faces of every
kind, part 63, scratch reuse across call sizes, and the refit's node boxes read back (fdcap_debug_collision_nodes).

Pair lists, counts and node boxes are compared with ZERO tolerance: the culled search, the every-pair launch, the header compiled by
g++ behind collision_spec.sweep_pairs and the numpy restatement collision_spec.node_boxes apply the same fp32 predicate, min and max.
Loss and dverts are held at tests/gradient_bars.py's formula, the bar taken from the twin's two precisions on the GPU's own kept
lists, as tests/test_gpu_collision.py does.  No bar is taken from a HIP result."""
import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from tests import collision_spec as spec
from tests import gradient_bars as gb
from tests.test_gpu_collision import as_set, check_order, evaluate, kept, make_ctx, twin_blocks

pytestmark = pytest.mark.gpu


def tree_info(ctx):
    leaf, order = ctx.collision_tree()
    NL, NLp = len(order) // leaf, 1
    while NLp < NL:
        NLp *= 2
    return leaf, NL, NLp, order


def check_nodes(ctx, verts, faces):
    """the refit kernel's boxes of every frame == the specification, bit for bit (node 0 is unspecified) -> the boxes [n, 2 NLp, 6]"""
    leaf, NL, NLp, order = tree_info(ctx)
    got = ctx.collision_nodes(torch.as_tensor(np.asarray(verts, np.float32)).cuda().contiguous()).cpu().numpy()
    assert got.shape == (len(verts), 2 * NLp, 6) and got.dtype == np.float32
    for f in range(len(verts)):
        want = spec.node_boxes(verts[f], faces, order, leaf, NL, NLp)
        assert got[f, 1:].tobytes() == want[1:].tobytes(), (f, np.nonzero((got[f, 1:] != want[1:]).any(1))[0][:8] + 1)
    return got


def bar_ratios(verts, faces, lists, sigma, weight, loss, dv):
    t64, t32 = (twin_blocks(verts, faces, lists, sigma, weight, d) for d in (torch.float64, torch.float32))
    return gb.ratios({"loss": loss, "dverts": dv}, t64, gb.bars(t32, t64)), t64


def sliced_tubes(F, rings, around, r):
    """collision_spec.crossing_tubes with the first ceil(F / 2) faces of the one tube and the first floor(F / 2) of the other"""
    v, f, moving = spec.crossing_tubes(rings, around, r)
    m, na = len(f) // 2, (F + 1) // 2
    f = np.concatenate([f[:na], f[m:m + F - na]])
    assert len(f) == F
    return v, f, moving


#          id               leaf asked   F      tube (rings, around, r)   leaf, NL, NLp       n
SHAPES = [("leaf32_F64", 32, 64, (4, 6, 0.05), (32, 2, 2), 2),                    # NL == NLp with more than one leaf
          ("leaf32_F128", 32, 128, (5, 8, 0.05), (32, 4, 4), 2),                  # npos = 128 < the refit's 256 threads
          ("leaf32_F256", 32, 256, (9, 8, 0.05), (32, 8, 8), 2),                  # exactly one pass of 256 threads
          ("leaf64_F16", 64, 16, (2, 4, 0.08), (64, 1, 1), 2),                    # one ragged leaf
          ("leaf64_F64", 64, 64, (4, 6, 0.05), (64, 1, 1), 2),                    # one full leaf
          ("leaf64_F65", 64, 65, (4, 6, 0.05), (64, 2, 2), 2),                    # the second leaf holds one face
          ("leaf64_F200", 64, 200, (7, 9, 0.05), (64, 4, 4), 2),                  # NL = 4, ragged
          ("leaf32_F16512", 32, 16512, 130, (32, 516, 1024), 2),                  # H = 10, the 48 KiB refit, upper-level loop of > 1 pass
          ("forced64_F32896", None, 32896, 258, (64, 514, 1024), 1)]              # coll_pick_leaf's size-forced leaf 64


@pytest.mark.parametrize("name,leaf_want,F,tube,tree,n", SHAPES, ids=[s[0] for s in SHAPES])
def test_tree_shapes(name, leaf_want, F, tube, tree, n, tmp_path, monkeypatch):
    """Every shape: culled == every-pair launch byte for byte on pairs, count, loss and dverts; the kept list as a set == sweep_pairs;
    the list's order; the refit's boxes == node_boxes; loss and dverts inside the bars.  At F = 32 896, one frame, the every-pair
    call takes 28.7 ms on an MI355X (device events, four calls 28.69-28.74; the culled one 0.93 ms), at F = 16 512 14.5 ms: both
    launches stay in the test at every size, nothing is left to sweep_pairs alone."""
    if leaf_want == 64:
        monkeypatch.setenv("FDCAP_COLL_LEAF", "64")
    else:
        monkeypatch.delenv("FDCAP_COLL_LEAF", raising=False)
    v, faces, moving = spec.long_tubes(tube) if isinstance(tube, int) else sliced_tubes(F, *tube)
    assert len(faces) == F
    ctx = make_ctx(v, faces)
    assert tree_info(ctx)[:3] == tree
    verts = spec.frames_of(v, faces, 6, moving)[[0, 5][:n]]
    cap, sigma, weight = 4096, 0.5, 1.0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    cull = evaluate(ctx, verts, capacity=cap)
    ev[1].record()
    every = evaluate(ctx, verts, capacity=cap, every_pair=True)
    ev[2].record()
    torch.cuda.synchronize()
    for a, b in zip(cull, every):
        assert a.tobytes() == b.tobytes()
    lists = [kept(cull[0], cull[1], f) for f in range(n)]
    for f in range(n):
        assert 0 < cull[1][f] < cap and len(lists[f]) == cull[1][f]
        assert as_set(lists[f]) == spec.sweep_pairs(verts[f], faces, None, None, tmp_path)
        check_order(ctx, lists[f])
    boxes = check_nodes(ctx, verts, faces)
    if n > 1:
        assert as_set(lists[0]) != as_set(lists[1]) and boxes[0, 1:].tobytes() != boxes[1, 1:].tobytes()     # frames that differ
    r, t64 = bar_ratios(verts, faces, lists, sigma, weight, cull[2], cull[3])
    print(name, "pairs per frame", cull[1], "max|err| / bar:", r,
          f"wall incl. copies: culled {ev[0].elapsed_time(ev[1]):.1f} ms, every pair {ev[1].elapsed_time(ev[2]):.1f} ms")
    assert (t64["loss"] > 0).all() and all(x <= 1.0 for x in r.values()), r
    ctx.close()


def test_sixty_five_frames_in_mixed_states_then_a_small_call_on_the_same_scratch(tmp_path):
    """n = 65 puts a frame into coll_frame_sum_kernel's second block; by frames_of's drift the second tube leaves the first around
    frame 38, so the batch holds frames with no pair, frames below the capacity and frames above it.  Then n = 1, capacity = 1 on the
    same context: the bytes of a fresh context's identical call."""
    vt, faces, v0, moving = spec.mesh_case("tubes")
    n = 65
    verts = spec.frames_of(v0, faces, n, moving)
    sets = [spec.sweep_pairs(verts[f], faces, None, None, tmp_path) for f in range(n)]
    found = np.array([len(s) for s in sets])
    assert (found == 0).any() and found[64] == 0 and found[0] > 0
    cap = int(found[found > 0].min() + found.max()) // 2
    assert ((found > 0) & (found <= cap)).any() and (found > cap).any()
    ctx = make_ctx(vt, faces)
    full = evaluate(ctx, verts, capacity=int(found.max()))
    full_lists = [kept(full[0], full[1], f) for f in range(n)]
    assert [as_set(l) for l in full_lists] == sets
    sigma, weight = 0.4, 2.5
    for every in (False, True):
        cut = evaluate(ctx, verts, capacity=cap, every_pair=every, sigma=sigma, weight=weight)
        np.testing.assert_array_equal(cut[1], found)                            # count: the number FOUND
        lists = [kept(cut[0], cut[1], f) for f in range(n)]                     # (kept: -1 stands behind the list)
        assert lists == [l[:cap] for l in full_lists]                           # the prefix of the full list
        empty = found == 0
        assert (cut[2][empty] == 0.0).all() and not cut[3][empty].any() and (cut[0][empty] == -1).all()
        assert (cut[2][~empty] > 0).all()
        r, _ = bar_ratios(verts, faces, lists, sigma, weight, cut[2], cut[3])
        print("every pair" if every else "culled", "pairs found", found.tolist(), "capacity", cap, "max|err| / bar:", r)
        assert all(x <= 1.0 for x in r.values()), r
    small = evaluate(ctx, verts[:1], capacity=1)
    fresh_ctx = make_ctx(vt, faces)
    fresh = evaluate(fresh_ctx, verts[:1], capacity=1)
    for a, b in zip(small, fresh):
        assert a.tobytes() == b.tobytes()
    assert small[1][0] == found[0] and [tuple(p) for p in small[0][0].tolist()] == full_lists[0][:1]
    for c in (ctx, fresh_ctx):
        c.close()


def test_every_return_of_the_penalty_runs_on_the_device():
    """sigma = 0.05 on the crossing tubes: the kept lists reach h >= sigma, phi >= 1, the deep branch and the quadratic one (sigma = 0.5,
    what every other test uses, reaches neither the deep branch nor the h >= sigma return), and the fp32 and the fp64 twin take the
    same return for every intruder -- a condition on the inputs, without which the bar would compare two different functions"""
    vt, faces, v0, moving = spec.mesh_case("tubes")
    n, sigma, weight = 3, 0.05, 0.7
    ctx = make_ctx(vt, faces)
    verts = spec.frames_of(v0, faces, n, moving)
    pairs, count, loss, dv = evaluate(ctx, verts, sigma=sigma, weight=weight)
    lists = [kept(pairs, count, f) for f in range(n)]
    for f in range(n):
        pr = np.array(lists[f])
        P = np.concatenate([verts[f][faces[pr[:, 0]]], verts[f][faces[pr[:, 1]]]], 1)
        t64, t32 = spec.psi_tags(P, sigma), spec.psi_tags(P, sigma, torch.float32)
        hist = np.bincount(t64.reshape(-1), minlength=5)
        print("frame", f, "pairs", len(pr), dict(zip(spec.TAG_NAMES, hist.tolist())))
        assert (t64 == t32).all()
        assert all(hist[t] > 0 for t in (spec.TAG_ABOVE, spec.TAG_OUTSIDE, spec.TAG_DEEP, spec.TAG_QUAD)) and hist[spec.TAG_RHO] == 0
    r, t64 = bar_ratios(verts, faces, lists, sigma, weight, loss, dv)
    print("sigma", sigma, "pairs", count, "loss", loss, "max|err| / bar:", r)
    assert (t64["loss"] > 0).all() and all(x <= 1.0 for x in r.values()), r
    only = evaluate(ctx, verts, sigma=sigma, weight=weight, grad=False, want_pairs=False)
    assert only[2].tobytes() == loss.tobytes() and only[1].tobytes() == count.tobytes()
    ctx.close()


def test_unusable_faces_of_every_kind(tmp_path):
    """frames 0 and 3 untouched; 1: a coordinate +inf; 2: a coordinate -inf; 4: a face with the same position twice (exactly zero area);
    5: NaN throughout, no usable face, every box (+inf, -inf)"""
    vt, faces, v0, moving = spec.mesh_case("tubes")
    ctx = make_ctx(vt, faces)
    n = 6
    verts = spec.frames_of(v0, faces, n, moving)
    clean = evaluate(ctx, verts)
    clean_lists = [kept(clean[0], clean[1], f) for f in range(n)]
    dirty_in = verts.copy()
    silenced = {}
    for f, val in ((1, np.inf), (2, -np.inf)):
        bad = int(faces[clean_lists[f][0][0]][0])                               # a corner of a face that collides in this frame
        dirty_in[f, bad, f % 3] = val
        silenced[f] = {int(i) for i in np.nonzero((faces == bad).any(1))[0]}
    flat = clean_lists[4][0][1]
    dirty_in[4, faces[flat][1]] = dirty_in[4, faces[flat][0]]
    dirty_in[5] = np.nan
    want_sets = [spec.sweep_pairs(dirty_in[f], faces, None, None, tmp_path) for f in range(n)]
    for every in (False, True):
        dirty = evaluate(ctx, dirty_in, every_pair=every)
        lists = [kept(dirty[0], dirty[1], f) for f in range(n)]
        assert [as_set(l) for l in lists] == want_sets and [len(l) for l in lists] == dirty[1].tolist()
        for f in (1, 2):                                                        # the silenced faces' pairs disappear, the others stay
            assert lists[f] == [p for p in clean_lists[f] if not (set(p) & silenced[f])] and 0 < len(lists[f]) < len(clean_lists[f])
        assert not any(flat in p for p in lists[4]) and len(lists[4]) > 0
        assert np.isfinite(dirty[2]).all() and np.isfinite(dirty[3]).all()
        for f in (0, 3):
            for a, b in zip(clean, dirty):
                assert a[f].tobytes() == b[f].tobytes()
        assert dirty[1][5] == 0 and dirty[2][5] == 0.0 and not dirty[3][5].any() and (dirty[0][5] == -1).all()
        r, _ = bar_ratios(np.nan_to_num(dirty_in, nan=0.0, posinf=0.0, neginf=0.0), faces, lists, 0.5, 1.0, dirty[2], dirty[3])
        print("every pair" if every else "culled", "pairs", dirty[1], "clean", clean[1], "max|err| / bar:", r)
        assert all(x <= 1.0 for x in r.values()), r
    boxes = check_nodes(ctx, dirty_in, faces)
    assert (boxes[5, 1:, :3] == np.inf).all() and (boxes[5, 1:, 3:] == -np.inf).all()
    assert np.isfinite(boxes[1:5, 1]).all()                                     # an unusable face is in no box: the roots stay finite
    ctx.close()


@pytest.mark.parametrize("name", ["tubes", "random"])
def test_part_63_and_bit_63(name, tmp_path):
    """the two tubes as parts 0 and 63: a one-sided bit (63, 0) or (0, 63) drops every pair across the tubes, bit (63, 63) alone the pairs
    inside the tube that is part 63.  `tubes` has pairs across only (48); `random`, vertices unrelated to the template, has all three
    kinds (3777 pairs, 1785 of them across)"""
    vt, faces, v0, _ = spec.mesh_case(name)
    verts = v0[None]
    part = np.where(np.arange(len(faces)) < 96, 0, 63).astype(np.uint8)
    base = spec.sweep_pairs(v0, faces, None, None, tmp_path)
    across = {p for p in base if (p[0] < 96) != (p[1] < 96)}
    inside = lambda lo, hi: {p for p in base if lo <= p[0] < hi and lo <= p[1] < hi}
    assert len(across) > 40
    if name == "random":
        assert len(across) > 100 and len(inside(0, 96)) > 100 and len(inside(96, 192)) > 100

    def matrix(a, b):
        m = np.zeros(64, np.uint64)
        m[a] = np.uint64(1) << np.uint64(b)
        return m
    for prt, ign, want in ((part, matrix(63, 0), base - across), (part, matrix(0, 63), base - across), (part, matrix(63, 63), base - inside(96, 192)),
                           (63 - part, matrix(63, 63), base - inside(0, 96))):
        assert spec.sweep_pairs(v0, faces, prt, ign, tmp_path) == want
        ctx = make_ctx(vt, faces, prt, ign)
        for every in (False, True):
            pairs, count, _, _ = evaluate(ctx, verts, capacity=4096, every_pair=every)
            lst = kept(pairs, count, 0)
            assert len(lst) == count[0] == len(want) and as_set(lst) == want
            check_order(ctx, lst)
        print(name, "parts 0 / 63: pairs", len(want), "of", len(base))
        ctx.close()


def test_refusals_of_the_node_readback():
    import dataclasses
    from fdcap_amd import capi, synth
    vt, faces, v0, _ = spec.mesh_case("tubes")
    ctx = capi.Context(dataclasses.replace(synth.make_body_model(len(vt), seed=1), v_template=vt), synth.make_vposer())
    v = torch.tensor(v0[None], device="cuda")
    out = torch.zeros(1, 2 * 8, 6, device="cuda")
    call = lambda verts=v, n=1, out=out: ctx.lib.fdcap_debug_collision_nodes(ctx.handle, capi.dptr(verts), n, capi.dptr(out), capi.current_stream())
    assert call() == -2                                                         # FDCAP_E_STATE: no registered mesh
    with pytest.raises(capi.FdcapError):
        ctx.collision_nodes(v)
    ctx.set_collision_mesh(faces)
    assert call() == 0
    assert call(verts=None) == -1 and call(out=None) == -1 and call(n=0) == -1 and call(n=-1) == -1
    with pytest.raises(capi.FdcapError):
        ctx.collision_nodes(torch.zeros(1, len(vt) + 1, 3, device="cuda"))
    torch.cuda.synchronize()
    ctx.close()
