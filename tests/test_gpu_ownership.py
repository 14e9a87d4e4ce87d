"""Whatever the library allocates is freed by the destroy call of what owns it (csrc/fdc_own.h: device blocks, the pinned block
and HIP events free themselves; the destroy entry points are `delete`).  Read through fdcap_debug_live_allocations -- {live blocks,
their bytes, live events} of the whole process -- as differences inside one test, so contexts other tests keep alive do not matter.

Shapes: a 400-vertex body, a 4 097-point scene (eight cells and one point), 40 contact ids, 8 frames -- except for the optimiser of
the first test.  That test asserts that the in-loop search ran under a query order (whose buffer, OptState::nnq_buf, no release
list of the parent held), and with default switches only the search's one-wave form takes one: from 2 816 groups of 32 queries
(plan_nn_search, fdc_forms.h).  8 frames x 40 contacts are 10 groups.  So its optimiser holds 226 frames x all 400 vertices as
contacts = 2 825 groups, the smallest clip of this body that reaches the form (225 frames: 2 813); every other step of that test
and all the other tests keep the small shapes.  Allocation failures are not provoked on the device: tests/test_ownership_cpu.py covers them."""
import ctypes

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, ops, synth
from fdcap_amd.fitting import ClipBatchFitter
from fdcap_amd.io import read_camerapose

pytestmark = pytest.mark.gpu
V, NS, NFRAMES = 400, 4097, 8
SWITCHES = ("FDCAP_NN_ORDER", "FDCAP_NN_CACHE_SLACK", "FDCAP_NN_SEED", "FDCAP_NN_CULL", "FDCAP_NN_KEEP_RECORDS", "FDCAP_CONTACT_RECOMPUTE",
            "FDCAP_SKIN_VEC", "FDCAP_FUSE_SKIN", "FDCAP_POSE_TRIM", "FDCAP_NN_BOX_LANES")      # (read by every fdcap_opt_create)


def _live():
    out = (ctypes.c_int64 * 3)()
    capi.check(capi.load_library().fdcap_debug_live_allocations(out), "fdcap_debug_live_allocations")
    return tuple(out)


@pytest.fixture(scope="module")
def model():
    bm = synth.make_body_model(V, seed=21)
    left, right = synth.make_contact_ids(bm.v_template, per_part=20, seed=24)
    return bm, synth.make_vposer(seed=22), synth.make_scene(NS, seed=23), np.concatenate([left, right])


def _clip(n, seed):
    c = synth.make_clip(n, seed=seed)
    return c.body_params, read_camerapose(c.camerapose_lines)


def _fitter(model, monkeypatch, vid=None, iters=3):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    bm, vp, scene, ids = model
    f = ClipBatchFitter({"num_iter": iters}, {}, body_model=bm, vposer=vp, contact_ids=ids if vid is None else vid)
    f.set_scene(scene)
    return f


def _run_operators(ctx, scene):
    """every stand-alone operator once, so that its workspaces in the context exist"""
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    # Op 1, both halves, backward to both inputs: a foreign target per batch, then the registered scene
    x1, x2 = rnd(2, 33, 3).requires_grad_(), rnd(2, 65, 3).requires_grad_()
    d1, d2 = ops.chamferDist(ctx, both=True)(x1, x2)
    (d1.sum() + d2.sum()).backward()
    assert x1.grad is not None and x2.grad is not None
    q, sc = rnd(2, 33, 3).requires_grad_(), torch.from_numpy(scene)[None].cuda().requires_grad_()
    op = ops.chamferDist(ctx, both=True)
    d1, d2 = op(q, sc)
    (d1.sum() + d2.sum()).backward()
    assert q.grad is not None and sc.grad.shape == (1, NS, 3)
    assert op._memo.get("same") is True                                   # (it was the registered scene's own search)
    # the body model from SMPLify-X rows with vertices: builds the full-mesh skin set
    verts, joints = ops.body_forward_from_params(ctx, torch.tensor(synth.make_clip(2, seed=6).body_params).cuda())
    assert verts.shape == (2, V, 3) and joints.shape == (2, 55, 3)
    # the VPoser decoder and its backward
    z = (0.1 * rnd(3, 32)).requires_grad_()
    ops.VPoser(ctx).decode(z, output_type="aa").sum().backward()
    assert z.grad is not None
    torch.cuda.synchronize()


def test_a_context_s_whole_life_returns_every_block_and_event(model, monkeypatch):
    bm, vp, scene, _ = model
    n = 226                                                               # (see the module's docstring)
    L0 = _live()
    f = _fitter(model, monkeypatch, vid=np.arange(V))
    lib, h = f.ctx.lib, f.ctx.handle
    Lc = _live()
    assert Lc[0] > L0[0] and Lc[1] > L0[1] and Lc[2] == L0[2], (L0, Lc)    # (the counters see the context)
    _run_operators(f.ctx, scene)
    L1 = _live()
    assert L1[0] > Lc[0] and L1[2] == L0[2], (Lc, L1)                     # ... and the operators' workspaces; no event so far
    f.prepare([_clip(n, 31)])                                             # the optimiser, default switches
    Lo = _live()
    assert lib.fdcap_opt_nn_timing(h, -1) == -1 and lib.fdcap_opt_launch_timing(h, -1) == -1      # a negative count: FDCAP_E_ARG ...
    assert _live() == Lo and Lo[2] == L1[2]                               # ... and no event is made
    capi.check(lib.fdcap_opt_nn_timing(h, 4), "fdcap_opt_nn_timing")
    capi.check(lib.fdcap_opt_launch_timing(h, 64), "fdcap_opt_launch_timing")
    L2 = _live()
    assert L2[0] > L1[0] and L2[1] > L1[1] and L2[2] == L1[2] + 2 * 4 + 64, (L1, L2)
    # three iterations, two of them in phase 1 (with the search), the first and the last logging
    hist = torch.zeros(2, 1, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
    n_done = ctypes.c_int32(0)
    capi.check(lib.fdcap_opt_run(h, 0, 3, 3, 2, 2, capi.dptr(hist), 2, 0, ctypes.byref(n_done), capi.current_stream()), "fdcap_opt_run")
    torch.cuda.synchronize()
    assert n_done.value == 2 and bool(torch.isfinite(hist).all())
    diet = (ctypes.c_int32 * 4)()
    capi.check(lib.fdcap_debug_contact_diet(h, diet), "fdcap_debug_contact_diet")
    assert diet[2] >= 1 and diet[3] >= 1, tuple(diet)                     # a search launch ran under the query order built after the first
    assert _live() == L2                                                  # (the loop allocates nothing)
    f._destroy_opt()
    assert _live() == L1
    f.close()
    assert _live() == L0


def test_repeated_optimisers_on_one_context_leave_the_same_counts(model, monkeypatch):
    f = _fitter(model, monkeypatch, iters=2)
    before = _live()
    after = []
    for k in range(3):
        f.prepare([_clip(NFRAMES, 40 + k)])
        assert _live()[0] > before[0]
        f.run(log_every=1)
        f._destroy_opt()
        after.append(_live())
    assert after[0] == after[1] == after[2], after                        # (the parent grew by the query order's buffer per cycle)
    assert after[0] == before, (before, after[0])                         # ... and these fits grow no workspace of the context
    f.close()


def test_clips_of_different_lengths_return_their_tables(model, monkeypatch):
    f = _fitter(model, monkeypatch)
    before = _live()
    f.prepare([_clip(5, 51), _clip(8, 52)])                               # fdcap_opt_create_clips_var
    assert f.num_body is None and _live()[0] > before[0]
    f._destroy_opt()
    assert _live() == before
    f.close()


def test_lbfgs_state_returns_its_buffers_and_the_pinned_block():
    lib = capi.load_library()
    torch.zeros(1, device="cuda")                                         # (a device is initialised)
    before = _live()
    cf = capi.LbfgsConfig(10, 100, 30, 0, 1, 25, 1.0, 1e-7, 1e-9, 0.0, 0.0)
    h = ctypes.c_void_p()
    capi.check(lib.fdcap_lbfgs_create(4, ctypes.byref(cf), ctypes.byref(h)), "fdcap_lbfgs_create")
    now = _live()
    assert now[0] == before[0] + 5 and now[1] > before[1] and now[2] == before[2], (before, now)      # four device blocks + the pinned one
    lib.fdcap_lbfgs_destroy(h)
    assert _live() == before


def test_a_re_registered_larger_scene_replaces_its_tables(model):
    bm, vp, scene, _ = model
    L0 = _live()
    ctx = capi.Context(bm, vp)
    ctx.set_scene(scene[:1000])
    a = _live()
    ctx.set_scene(scene)
    b = _live()
    assert b[0] == a[0] and b[1] > a[1] and b[2] == a[2], (a, b)          # every table grew in place: the same blocks, more bytes
    ctx.close()
    assert _live() == L0
