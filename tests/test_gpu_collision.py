"""GPU tests of the self-interpenetration operator (csrc/fdc_collide.h, fdcap_set_collision_mesh / fdcap_collision_eval,
ops.SelfCollision) against the twin tests/collision_spec.py and against the header itself compiled by g++.

Pair sets are compared with zero tolerance: the culled search, the every-pair launch and the host run the same fp32 predicate.  Value
and gradient are held at tests/gradient_bars.py's formula, the bar taken from the twin's two precisions ON THE GPU'S OWN PAIR LIST, so
no marginal pair enters.  No bar is taken from a HIP result."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, ops, synth
from fdcap_amd.innerfit import collision_filter
from tests import collision_spec as spec
from tests import gradient_bars as gb

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -2


def make_ctx(template, faces, part=None, ignore=None):
    """a context whose body template is `template` (the tree is built on it); every other model array is synth's at that size"""
    bm = dataclasses.replace(synth.make_body_model(len(template), seed=1), v_template=np.asarray(template, np.float32))
    ctx = capi.Context(bm, synth.make_vposer())
    ctx.set_collision_mesh(faces, part, ignore)
    return ctx


def evaluate(ctx, verts, sigma=0.5, weight=1.0, capacity=2048, every_pair=False, grad=True, want_pairs=True):
    v = torch.as_tensor(np.asarray(verts, np.float32)).cuda().contiguous()
    n = v.shape[0]
    pairs = torch.full((n, capacity, 2), -7, dtype=torch.int32, device="cuda") if want_pairs else None
    count = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    loss = torch.full((n,), np.nan, device="cuda")
    dv = torch.full_like(v, np.nan) if grad else None
    prm = capi.CollisionParams(sigma, weight, capacity, 1 if every_pair else 0)
    code = ctx.lib.fdcap_collision_eval(ctx.handle, capi.dptr(v), n, prm, capi.dptr(pairs), capi.dptr(count), capi.dptr(loss), capi.dptr(dv),
                                        capi.current_stream())
    torch.cuda.synchronize()
    assert code == 0, code
    return (pairs.cpu().numpy() if want_pairs else None, count.cpu().numpy(), loss.cpu().numpy(), dv.cpu().numpy() if grad else None)


def kept(pairs, count, f):
    k = min(int(count[f]), pairs.shape[1])
    assert (pairs[f, k:] == -1).all()
    return [tuple(p) for p in pairs[f, :k].tolist()]


def as_set(lst):
    return {(min(a, b), max(a, b)) for a, b in lst}


# the meshes: tests/collision_spec.py holds them, for the CPU tests too
from tests.collision_spec import MESHES, bent_tube, crossing_tubes, frames_of, mesh_case  # noqa: E402,F401


def check_order(ctx, lst):
    """the list stands by (owner's tree position, other's tree position), the owner first"""
    leaf, order = ctx.collision_tree()
    pos = np.full(order.max() + 1, -1)
    pos[order[order >= 0]] = np.nonzero(order >= 0)[0]
    keys = [(pos[a], pos[b]) for a, b in lst]
    assert all(a < b for a, b in keys) and keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("name", MESHES)
def test_culled_search_equals_every_pair_launch_equals_host(name, n, tmp_path, monkeypatch):
    vt, faces, v0, moving = mesh_case(name)
    if name == "tubes64":
        monkeypatch.setenv("FDCAP_COLL_LEAF", "64")
    ctx = make_ctx(vt, faces)
    assert ctx.collision_tree()[0] == (64 if name == "tubes64" else 32)
    verts = frames_of(v0, faces, n, moving)
    cull = evaluate(ctx, verts, capacity=4096)
    every = evaluate(ctx, verts, capacity=4096, every_pair=True)
    again = evaluate(ctx, verts, capacity=4096)
    for a, b in zip(cull, again):
        assert a.tobytes() == b.tobytes()                                       # the same call twice: the same bits
    for a, b in zip(cull, every):
        assert a.tobytes() == b.tobytes()                                       # lists, counts, loss, gradient
    sets = []
    for f in range(n):
        lst = kept(cull[0], cull[1], f)
        assert len(lst) == cull[1][f]
        check_order(ctx, lst)
        host = spec.host_pairs(verts[f], faces, None, None, tmp_path)
        assert as_set(lst) == host
        twin, margins = spec.collision_set(verts[f], faces, with_margins=True)  # the fp64 twin: they differ in marginal pairs at most
        assert all(spec.marginal(p in twin, *margins[p]) for p in host ^ twin) and len(host ^ twin) <= 0.02 * len(twin)
        sets.append(host)
    print(name, n, "pairs per frame", [len(s) for s in sets])
    if name == "grid":
        assert all(len(s) == 0 for s in sets) and not cull[2].any() and not cull[3].any()
    else:
        assert all(len(s) > 0 for s in sets)
        if n > 1 and name != "one_leaf":
            assert len({frozenset(s) for s in sets}) > 1                        # frames that differ
    if name == "bent":
        leaf, order = ctx.collision_tree()
        pos = {int(f): p for p, f in enumerate(order) if f >= 0}
        assert max(abs(pos[a] - pos[b]) for a, b in sets[0]) > 8 * leaf         # far apart in tree order
    ctx.close()


def test_mid_size_mesh_culled_against_every_pair():
    """F = 4992, n = 2: no host side; 157 leaves under a 256-leaf tree, more than one workgroup per frame in every kernel"""
    va, fa = spec.tube((-0.5, 0.0, 3.0), (0.5, 0.0, 3.0), 0.08, 40, 32)
    vb, fb = spec.tube((0.03, -0.5, 3.02), (0.0, 0.5, 3.05), 0.08, 40, 32, phase=0.1)
    v, f = np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)])
    assert len(f) == 4992
    ctx = make_ctx(v, f)
    verts = frames_of(v, f, 2, np.arange(len(va), len(v)))
    cull = evaluate(ctx, verts, capacity=4096)
    every = evaluate(ctx, verts, capacity=4096, every_pair=True)
    for a, b in zip(cull, every):
        assert a.tobytes() == b.tobytes()
    print("pairs per frame", cull[1])
    assert (cull[1] > 100).all() and (cull[1] < 4096).all() and cull[1][0] != cull[1][1]
    for fr in range(2):
        check_order(ctx, kept(cull[0], cull[1], fr))
    assert np.isfinite(cull[2]).all() and np.isfinite(cull[3]).all() and (cull[2] > 0).all()
    ctx.close()


def test_a_nan_vertex_silences_its_faces_and_no_other_frame():
    vt, faces, v0, moving = mesh_case("tubes")
    ctx = make_ctx(vt, faces)
    verts = frames_of(v0, faces, 3, moving)
    clean = evaluate(ctx, verts)
    lst = kept(clean[0], clean[1], 1)
    bad_vertex = int(faces[lst[0][0]][0])                                       # a corner of a face that collides in frame 1
    dirty_in = verts.copy()
    dirty_in[1, bad_vertex, 1] = np.nan
    for every in (False, True):
        dirty = evaluate(ctx, dirty_in, every_pair=every)
        touched = {int(i) for i in np.nonzero((faces == bad_vertex).any(1))[0]}
        got = kept(dirty[0], dirty[1], 1)
        assert got == [p for p in lst if not (set(p) & touched)] and len(got) < len(lst)
        assert np.isfinite(dirty[2]).all() and np.isfinite(dirty[3]).all()
        for f in (0, 2):
            for a, b in zip(clean, dirty):
                assert a[f].tobytes() == b[f].tobytes()
    ctx.close()


def twin_blocks(verts, faces, lists, sigma, weight, dtype):
    t = torch.tensor(np.asarray(verts, np.float32), dtype=dtype, requires_grad=True)
    e = spec.penalty(t, faces, lists, sigma, weight)
    e.sum().backward()
    return {"loss": e.detach().numpy().astype(np.float64), "dverts": t.grad.numpy().astype(np.float64)}


def test_list_order_and_overflow():
    vt, faces, v0, moving = mesh_case("tubes")
    ctx = make_ctx(vt, faces)
    verts = frames_of(v0, faces, 3, moving)
    full = evaluate(ctx, verts)
    cap = int(full[1].min()) - 3                                                 # below every frame's count
    assert cap > 4
    for every in (False, True):
        cut = evaluate(ctx, verts, capacity=cap, every_pair=every, sigma=0.4, weight=2.5)
        np.testing.assert_array_equal(cut[1], full[1])                          # count: the number FOUND
        lists = [kept(cut[0], cut[1], f) for f in range(3)]
        assert lists == [kept(full[0], full[1], f)[:cap] for f in range(3)]     # the prefix of the full list
        t64, t32 = (twin_blocks(verts, faces, lists, 0.4, 2.5, d) for d in (torch.float64, torch.float32))
        r = gb.ratios({"loss": cut[2], "dverts": cut[3]}, t64, gb.bars(t32, t64))
        print("kept pairs only, max|err| / bar:", r)
        assert all(v <= 1.0 for v in r.values()), r
        more = twin_blocks(verts, faces, [kept(full[0], full[1], f) for f in range(3)], 0.4, 2.5, torch.float64)
        assert (more["loss"] > t64["loss"] * (1 + 1e-6)).all()                   # the dropped pairs would have counted
    ctx.close()


def test_part_matrix_and_shared_vertices():
    vt, faces, v0, moving = mesh_case("tubes")
    part = (np.arange(len(faces)) * 7 % 5).astype(np.uint8)
    part[96:] += 40
    verts = frames_of(v0, faces, 1, moving)
    base_ctx = make_ctx(vt, faces)
    base = as_set(kept(*evaluate(base_ctx, verts)[:2], 0))
    assert all(not (set(faces[a]) & set(faces[b])) for a, b in base)             # no pair shares a vertex index ...
    welded = faces.copy()
    a0, b0 = sorted(base)[0]
    welded[b0, 2] = welded[a0, 0]                                                # ... and welding two colliding faces removes their pair
    wctx = make_ctx(vt, welded)
    assert (a0, b0) not in as_set(kept(*evaluate(wctx, verts)[:2], 0))
    wctx.close()
    pa, pb = int(part[a0]), int(part[b0])                                         # the parts of a pair that collides
    assert pa < 40 <= pb
    for ign in (collision_filter(ignore_pairs=[(pa, pb)], same_part=False), collision_filter(ignore_pairs=[(pb, pa), (0, 40)], same_part=False)):
        ctx = make_ctx(vt, faces, part, ign)
        got = as_set(kept(*evaluate(ctx, verts)[:2], 0))
        drop = lambda a, b: bool((int(ign[part[a]]) >> int(part[b])) & 1) or bool((int(ign[part[b]]) >> int(part[a])) & 1)
        assert got == {p for p in base if not drop(*p)} and len(got) < len(base)
        assert got == as_set(kept(*evaluate(ctx, verts, every_pair=True)[:2], 0))
        ctx.close()
    # one-sided bits drop the pair both ways round; parts without a matrix, and a matrix without parts (all part 0), drop nothing
    one = np.zeros(64, np.uint64)
    one[pb] = np.uint64(1) << np.uint64(pa)
    ctx = make_ctx(vt, faces, part, one)
    assert as_set(kept(*evaluate(ctx, verts)[:2], 0)) == {p for p in base if {int(part[p[0]]), int(part[p[1]])} != {pa, pb}}
    ctx.set_collision_mesh(faces, part, None)
    assert as_set(kept(*evaluate(ctx, verts)[:2], 0)) == base
    ctx.set_collision_mesh(faces, None, one)
    assert as_set(kept(*evaluate(ctx, verts)[:2], 0)) == base
    ctx.close()
    base_ctx.close()


@pytest.mark.parametrize("name,n", [("tubes", 3), ("bent", 1)])
def test_value_and_gradient_against_the_fp64_twin(name, n):
    vt, faces, v0, moving = mesh_case(name)
    ctx = make_ctx(vt, faces)
    verts = frames_of(v0, faces, n, moving)
    sigma, weight = 0.5, 0.7
    pairs, count, loss, dv = evaluate(ctx, verts, sigma=sigma, weight=weight)
    lists = [kept(pairs, count, f) for f in range(n)]
    t64, t32 = (twin_blocks(verts, faces, lists, sigma, weight, d) for d in (torch.float64, torch.float32))
    bar = gb.bars(t32, t64)
    r = gb.ratios({"loss": loss, "dverts": dv}, t64, bar)
    print(name, "pairs", count, "loss", loss, "max|err| / bar:", r, "fp32 twin's:", gb.ratios(t32, t64, bar))
    assert (t64["loss"] > 0).all() and np.abs(t64["dverts"]).max() > 0
    assert all(v <= 1.0 for v in r.values()), r
    # the forward alone (dverts NULL, pairs NULL) gives the same loss bits
    only = evaluate(ctx, verts, sigma=sigma, weight=weight, grad=False, want_pairs=False)
    assert only[2].tobytes() == loss.tobytes() and only[1].tobytes() == count.tobytes()
    # vertices no kept pair touches have an exactly zero gradient
    used = np.zeros((n, len(vt)), bool)
    for f in range(n):
        for a, b in lists[f]:
            used[f, faces[a]] = used[f, faces[b]] = True
    assert not dv[~used].any() and (~used).any()
    ctx.close()


def test_autograd_through_the_operator():
    vt, faces, v0, moving = mesh_case("tubes")
    ctx = make_ctx(vt, faces)
    verts = frames_of(v0, faces, 2, moving)
    op = ops.SelfCollision(ctx, sigma=0.5, weight=1.3, capacity=1024)
    v = torch.tensor(verts, device="cuda", requires_grad=True)
    loss = op(v)
    coef = torch.tensor([0.5, 2.0], device="cuda")
    (loss * coef).sum().backward()
    lists = [kept(op.last_pairs.cpu().numpy(), op.last_count.cpu().numpy(), f) for f in range(2)]

    def twin(dtype):
        t = torch.tensor(verts, dtype=dtype, requires_grad=True)
        e = spec.penalty(t, faces, lists, 0.5, 1.3)
        (e * coef.cpu().to(dtype)).sum().backward()
        return {"loss": e.detach().numpy().astype(np.float64), "dverts": t.grad.numpy().astype(np.float64)}
    t64, t32 = twin(torch.float64), twin(torch.float32)
    r = gb.ratios({"loss": loss.detach().cpu().numpy(), "dverts": v.grad.cpu().numpy()}, t64, gb.bars(t32, t64))
    print("ops.SelfCollision, max|err| / bar:", r)
    assert all(x <= 1.0 for x in r.values()), r
    # a directional derivative of the operator's loss agrees with its gradient (fp64 central difference of the twin's value on the same list)
    d = np.random.Generator(np.random.PCG64(2)).standard_normal(verts.shape)
    h = 1e-7
    ep, em = (spec.penalty(torch.tensor(verts.astype(np.float64) + s * h * d), faces, lists, 0.5, 1.3).numpy() for s in (1, -1))
    fd = ((ep - em) / (2 * h) * coef.cpu().numpy()).sum()
    an = float((v.grad.cpu().numpy().astype(np.float64) * d).sum())
    assert abs(fd - an) <= 1e-4 * abs(fd) + 1e-9, (fd, an)
    no_grad = op(torch.tensor(verts, device="cuda"))
    assert no_grad.cpu().numpy().tobytes() == loss.detach().cpu().numpy().tobytes()
    for bad in (dict(sigma=0.0), dict(sigma=1.0), dict(weight=-1.0), dict(weight=float("nan")), dict(capacity=0)):
        with pytest.raises(capi.FdcapError):
            ops.SelfCollision(ctx, **bad)
    with pytest.raises(capi.FdcapError):
        op(torch.zeros(2, len(vt) + 1, 3, device="cuda"))
    ctx.close()


def test_refusals_of_the_operator():
    vt, faces, v0, _ = mesh_case("tubes")
    bm = dataclasses.replace(synth.make_body_model(len(vt), seed=1), v_template=vt)
    ctx = capi.Context(bm, synth.make_vposer())
    v = torch.tensor(v0[None], device="cuda")
    count, loss = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")

    def call(prm=(0.5, 1.0, 64, 0), verts=v, n=1, count=count, loss=loss, params=True):
        p = capi.CollisionParams(*prm)
        return ctx.lib.fdcap_collision_eval(ctx.handle, capi.dptr(verts), n, p if params else None, None, capi.dptr(count), capi.dptr(loss), None,
                                            capi.current_stream())
    assert call() == E_STATE                                                     # no registered mesh
    with pytest.raises(capi.FdcapError):
        ctx.collision_tree()
    def reg(f, part=None):
        fa = np.ascontiguousarray(f, np.int32)
        pa = None if part is None else np.ascontiguousarray(part, np.uint8)
        return ctx.lib.fdcap_set_collision_mesh(ctx.handle, len(fa), fa.ctypes.data, None if pa is None else pa.ctypes.data, None)
    assert reg(faces[:2]) == E_ARG                                               # F < 3
    bad = faces.copy()
    bad[5, 1] = len(vt)
    assert reg(bad) == E_ARG
    bad[5, 1] = -1
    assert reg(bad) == E_ARG
    assert reg(np.zeros((65536, 3), np.int32)) == E_ARG
    assert reg(faces, np.full(len(faces), 64)) == E_ARG
    with pytest.raises(capi.FdcapError):
        ctx.set_collision_mesh(faces, np.full(len(faces), 64))
    with pytest.raises(capi.FdcapError):
        ctx.set_collision_mesh(faces, np.zeros(3))
    assert call() == E_STATE                                                     # a refused registration registers nothing
    assert reg(faces, np.full(len(faces), 63)) == 0
    assert call() == 0
    for prm in ((0.0, 1.0, 64, 0), (1.0, 1.0, 64, 0), (float("nan"), 1.0, 64, 0), (0.5, -1.0, 64, 0), (0.5, float("inf"), 64, 0),
                (0.5, float("nan"), 64, 0), (0.5, 1.0, 0, 0), (0.5, 1.0, -1, 0)):
        assert call(prm) == E_ARG, prm
    assert call(n=0) == E_ARG and call(verts=None) == E_ARG and call(count=None) == E_ARG and call(loss=None) == E_ARG and call(params=False) == E_ARG
    assert call((0.5, 0.0, 64, 0)) == 0                                          # weight 0 is a value, not an error
    torch.cuda.synchronize()
    assert float(loss[0]) == 0.0 and int(count[0]) > 0
    # while an optimiser lives the mesh cannot change (as the scene)
    n = 2
    oc = capi.OptConfig(n, n, 0, 0.01, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0)
    keep = [torch.zeros(n + 4, capi.XDIM, device="cuda"), torch.zeros(n + 4, 16, device="cuda"), torch.zeros(1, device="cuda"),
            torch.zeros(1, device="cuda"), torch.zeros(capi.NUM_LOSSES, device="cuda", dtype=torch.float64)]
    ctx.set_scene(np.zeros((0, 3), np.float32))
    torch.cuda.synchronize()
    capi.check(ctx.lib.fdcap_opt_create(ctx.handle, ctypes.byref(oc), *(capi.dptr(t) for t in keep)), "fdcap_opt_create")
    assert reg(faces) == E_STATE and reg(faces[:0]) == E_STATE
    assert call() == 0                                                           # ... and the operator still runs beside it
    ctx.lib.fdcap_opt_destroy(ctx.handle)
    # clearing
    assert reg(faces[:0]) == 0 and call() == E_STATE
    ctx.close()
