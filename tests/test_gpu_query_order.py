"""Which queries share a wave of the in-loop Chamfer search (fdc_chamfer.h NNCache::perm) is scheduling only: any order of the
queries gives the same neighbours, the same distances and the same fit, bit for bit.

255 frames x 500 contacts = 127 500 queries: the one-wave form of the search (the only one that takes a query order), and
nq % 32 = 12, so the last wave is ragged.  fdcap_debug_nn_query_order imposes the order: 0 the default (grouped by the k-d quarter
of each query's neighbour, rebuilt after the seeding launch and every 32 launches, kept lists alive in between), 1 query order,
2 an order given by the caller.
"""
import ctypes

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.fitting import FittingOP
from fdcap_amd.io import read_camerapose

pytestmark = pytest.mark.gpu

N, NS, V, PER_PART = 255, 100_000, 10475, 250
NQ = N * 2 * PER_PART
P = 32                                                      # phase-1 iterations of the short fit below (the search runs in phase 1)


@pytest.fixture(scope="module")
def assets():
    bm = synth.make_body_model(V, seed=0)
    vp = synth.make_vposer(seed=1)
    clip = synth.make_clip(N, seed=3)
    scene = synth.make_scene(NS, seed=2)
    left, right = synth.make_contact_ids(bm.v_template, per_part=PER_PART, seed=4)
    return bm, vp, clip, scene, np.concatenate([left, right])


def _orders():
    rng = np.random.default_rng(7)
    return {
        "reversed": np.arange(NQ, dtype=np.int32)[::-1].copy(),
        "random": rng.permutation(NQ).astype(np.int32),
    }


def _set_order(fop, mode, perm=None):
    p = None if perm is None else perm.ctypes.data
    capi.check(fop.ctx.lib.fdcap_debug_nn_query_order(fop.ctx.handle, mode, p, NQ if perm is not None else 0), "nn_query_order")


def _start(assets):
    bm, vp, clip, scene, vid = assets
    assert NQ % 32 != 0 and len(vid) == 2 * PER_PART
    fop = FittingOP({"num_iter": 40}, {}, N, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                    camera_ext=read_camerapose(clip.camerapose_lines))
    x78 = torch.empty(N, capi.XDIM, device="cuda")
    capi.check(fop.ctx.lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(clip.body_params).cuda()), N, capi.dptr(x78),
                                                 capi.current_stream()), "75->78")
    fop._mode = "global"
    fop.init(x78)
    return fop


def _iterate(fop, first, count):
    lib, h = fop.ctx.lib, fop.ctx.handle
    for ii in range(first, first + count):
        capi.check(lib.fdcap_opt_backward(h, ii, P, 0, capi.current_stream()), "backward")
        capi.check(lib.fdcap_opt_step(h, ii, P, capi.current_stream()), "step")


def _state(fop):
    """the last search's distances and neighbours + the optimiser's rows, scale and cameras"""
    lib, h = fop.ctx.lib, fop.ctx.handle
    d = torch.empty(N, 2 * PER_PART, device="cuda")
    i = torch.empty(N, 2 * PER_PART, device="cuda", dtype=torch.int32)
    capi.check(lib.fdcap_opt_sync(h, capi.current_stream()), "sync")
    capi.check(lib.fdcap_opt_get_contact(h, capi.dptr(d), capi.dptr(i), capi.current_stream()), "get_contact")
    torch.cuda.synchronize()
    return [d.cpu(), i.cpu(), fop._rows_x.cpu(), fop._scale.cpu(), fop._rows_cam.cpu()]


def _run(assets, mode, perm=None, iters=40, switch=None):
    """a short fit (32 phase-1 + 8 phase-2 iterations) under one query order; switch = (iteration, mode, perm): change it there"""
    fop = _start(assets)
    _set_order(fop, mode, perm)
    forms = ctypes.create_string_buffer(4096)
    capi.check(fop.ctx.lib.fdcap_debug_kernel_forms(forms, len(forms), 1), "kernel_forms")   # (reset)
    if switch is None:
        _iterate(fop, 0, iters)
    else:
        at, m2, p2 = switch
        _iterate(fop, 0, at)
        _set_order(fop, m2, p2)
        _iterate(fop, at, iters - at)
    out = _state(fop)
    capi.check(fop.ctx.lib.fdcap_debug_kernel_forms(forms, len(forms), 0), "kernel_forms")
    assert "nn_stream4_kernel<1,1,1>" in forms.value.decode()         # the one form that takes a query order
    fop.close()
    return out


def _same(a, b):
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def identity(assets):
    return {it: _run(assets, 1, iters=it) for it in (P, 40)}


@pytest.mark.parametrize("name", ["default", "reversed", "random"])
def test_query_orders_give_the_same_fit(assets, identity, name):
    perm = _orders().get(name)
    mode = 0 if perm is None else 2
    _same(_run(assets, mode, perm, iters=P), identity[P])   # the last search of phase 1: dist / idx as the loop saw them
    _same(_run(assets, mode, perm, iters=40), identity[40])  # through the phase switch


def test_order_changes_mid_fit_change_nothing(assets, identity):
    # kept lists built under one order, then a new order imposed (lists dropped, the launch order re-recorded)
    _same(_run(assets, 1, iters=40, switch=(13, 2, _orders()["random"])), identity[40])
    _same(_run(assets, 2, _orders()["reversed"], iters=40, switch=(17, 0, None)), identity[40])


def test_seam_rejects_what_is_not_a_permutation(assets):
    fop = _start(assets)
    lib, h = fop.ctx.lib, fop.ctx.handle
    bad = np.arange(NQ, dtype=np.int32)
    bad[5] = 4                                               # a duplicate
    assert lib.fdcap_debug_nn_query_order(h, 2, bad.ctypes.data, NQ) != 0
    bad[5] = NQ                                              # out of range
    assert lib.fdcap_debug_nn_query_order(h, 2, bad.ctypes.data, NQ) != 0
    assert lib.fdcap_debug_nn_query_order(h, 2, bad.ctypes.data, NQ - 1) != 0
    assert lib.fdcap_debug_nn_query_order(h, 3, None, 0) != 0
    fop.close()
