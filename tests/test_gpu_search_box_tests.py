"""How the in-loop Chamfer search runs its per-query box tests is scheduling only (fdc_chamfer.h nn_box_stage): 2, 4 or 8 lanes per
listed box (FDCAP_NN_BOX_LANES; 0 = by each stage's count) keep the same entries in the same order, so the search visits the same
quarters and every neighbour, distance and optimiser row has the same bits as with a pair of lanes per box everywhere (= 2, every
launch before the switch existed).  A setting is that width; the reference is 2.

Shapes as in tests/test_gpu_query_order.py: 255 frames x 500 contacts = 127 500 queries (one-wave workgroups, a ragged last wave)
against 100 000 scene points, 32 phase-1 + 8 phase-2 iterations.  A forced width holds at every count (tests/test_box_lanes_cpu.py),
so a forced 8 serves eight entries per pass and a forced 4 sixteen: stages of the lengths a fit meets (profiles/r15_nn_list_lengths.txt:
7 near chunks per batch, ~20 quarters per quarter stage, 12-20 per filter list) take several passes with them, and every width and the
multi-pass compaction run.  Further cases: a 2 000-point scene (four chunks, one super-cell, lists of a few entries), every frame's
translation shifted by 3 cm between two iterations (the kept lists are void at the next launch and the waves build again), and one
frame whose queries are NaN.

The 128- and 160-frame cases (four / two waves per group) check less: those forms keep the pair form whatever the switch says, so
their three settings run the same code -- the cases pin that the shared helper serves those forms and that the switch does not
reach them.

Every run asserts the form the search took, and through fdcap_debug_nn_box_tests that its one-wave launches were given the setting
under test (lanes per box): a setting that never reached the kernel's argument would make the comparison empty.  What a stage does with the argument is nn_box_lanes, pinned on the CPU.
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

V, PER_PART = 10475, 250
P, ITERS = 32, 40                                           # phase-1 iterations (the search runs there), iterations in all
REFERENCE = 2
W1, W2, W4 = "nn_stream4_kernel<1,1,1>", "nn_stream4_kernel(2 waves per group)", "nn_stream4_kernel(4 waves per group)"


@pytest.fixture(scope="module")
def assets():
    bm = synth.make_body_model(V, seed=0)
    left, right = synth.make_contact_ids(bm.v_template, per_part=PER_PART, seed=4)
    scenes = {ns: synth.make_scene(ns, seed=2) for ns in (100_000, 2_000)}
    return bm, synth.make_vposer(seed=1), scenes, np.concatenate([left, right])


def _fit(assets, monkeypatch, setting, n=255, ns=100_000, form=W1, shift_at=None, nan_frame=None):
    """the last search's distances and neighbours + the optimiser's rows, scale and cameras after a short fit under one setting"""
    bm, vp, scenes, vid = assets
    monkeypatch.setenv("FDCAP_NN_BOX_LANES", str(setting))             # (read by every fdcap_opt_create)
    clip = synth.make_clip(n, seed=3)
    params = np.array(clip.body_params, copy=True)
    if nan_frame is not None: params[nan_frame, 0:3] = np.nan
    fop = FittingOP({"num_iter": ITERS}, {}, n, body_model=bm, vposer=vp, scene_verts=scenes[ns], contact_ids=vid,
                    camera_ext=read_camerapose(clip.camerapose_lines))
    lib, h = fop.ctx.lib, fop.ctx.handle
    x78 = torch.empty(n, capi.XDIM, device="cuda")
    capi.check(lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(params).cuda()), n, capi.dptr(x78), capi.current_stream()), "75->78")
    fop._mode = "global"
    fop.init(x78)
    forms = ctypes.create_string_buffer(4096)
    capi.check(lib.fdcap_debug_kernel_forms(forms, len(forms), 1), "kernel_forms")   # (reset)
    for ii in range(ITERS):
        if ii == shift_at:
            capi.check(lib.fdcap_opt_sync(h, capi.current_stream()), "sync")
            fop._rows_x[2:2 + n, 0:3] += 0.03
        capi.check(lib.fdcap_opt_backward(h, ii, P, 0, capi.current_stream()), "backward")
        capi.check(lib.fdcap_opt_step(h, ii, P, capi.current_stream()), "step")
    d = torch.empty(n, 2 * PER_PART, device="cuda")
    i = torch.empty(n, 2 * PER_PART, device="cuda", dtype=torch.int32)
    capi.check(lib.fdcap_opt_sync(h, capi.current_stream()), "sync")
    capi.check(lib.fdcap_opt_get_contact(h, capi.dptr(d), capi.dptr(i), capi.current_stream()), "get_contact")
    torch.cuda.synchronize()
    out = [d.cpu(), i.cpu(), fop._rows_x.cpu(), fop._scale.cpu(), fop._rows_cam.cpu()]
    capi.check(lib.fdcap_debug_kernel_forms(forms, len(forms), 0), "kernel_forms")
    assert form in forms.value.decode(), forms.value.decode()
    box = (ctypes.c_int32 * 4)()
    diet = (ctypes.c_int32 * 4)()
    capi.check(lib.fdcap_debug_nn_box_tests(h, box), "nn_box_tests")
    capi.check(lib.fdcap_debug_contact_diet(h, diet), "contact_diet")
    box, slot = list(box), {0: 0, 2: 1, 4: 2, 8: 3}[setting]
    if form == W1:
        assert box[slot] >= P and sum(box) == box[slot], box               # every one-wave launch under the width asked for
        assert diet[2] >= P - 2, list(diet)                                 # ... nearly all of them under a query order
    else:
        assert box == [0, 0, 0, 0], box                                     # no one-wave launch: nothing the switch reaches
    fop.close()
    return out


def _same(a, b):
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
        # bits, not values: a frame without neighbours carries NaNs, and NaN != NaN
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


_references = {}


def _reference(assets, monkeypatch, **case):
    key = tuple(sorted(case.items()))
    if key not in _references:                                # computed once per case, shared by its settings, never changed
        _references[key] = _fit(assets, monkeypatch, REFERENCE, **case)
    return _references[key]


# (the ids are the ones these cases had while a setting was a pair: a case keeps its name)
@pytest.mark.parametrize("setting", [0, 4, 8], ids=["setting0", "setting1", "setting2"])
def test_every_width_gives_the_fit_of_a_pair_per_box(assets, monkeypatch, setting):
    want = _reference(assets, monkeypatch)
    assert int(want[1].min()) >= 0 and bool(torch.isfinite(want[0]).all())
    _same(_fit(assets, monkeypatch, setting), want)


CASES = {
    "a scene of four chunks": dict(ns=2_000),
    "lists voided by a 3 cm shift": dict(shift_at=20),
    "a frame without neighbours": dict(nan_frame=7),
    "four waves per group": dict(n=128, form=W4),
    "two waves per group": dict(n=160, form=W2),
}


@pytest.mark.parametrize("setting", [0, 8], ids=["setting0", "setting1"])
@pytest.mark.parametrize("case", list(CASES))
def test_other_lists_and_forms(assets, monkeypatch, case, setting):
    want = _reference(assets, monkeypatch, **CASES[case])
    if case == "a frame without neighbours":
        assert bool((want[1][7] < 0).all()) and int(want[1][:7].min()) >= 0      # its queries found nothing, the others did
    if case == "lists voided by a 3 cm shift":
        assert not torch.equal(want[1], _reference(assets, monkeypatch)[1])       # the shift really changed neighbours
    _same(_fit(assets, monkeypatch, setting, **CASES[case]), want)
