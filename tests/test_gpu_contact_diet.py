"""Contact data an iteration already holds is neither stored nor staged again, and nothing computed changes by a bit.

1. The in-loop search writes a neighbour record (idx[q], seedpt[q]) only when the neighbour changed (fdc_chamfer.h NNCache::keep).
   The sequence of tests/test_gpu_parity.py::test_kept_work_lists_do_not_change_results -- 45 launches, 1 mm random moves, one 3 cm
   jump at launch 25 -- once with FDCAP_NN_KEEP_RECORDS=0 (every record rewritten in every launch) and once by default: dist, idx and
   the records (fdcap_debug_nn_records) are equal at every launch, the records' coordinates are the scene points of idx, and at a
   launch before the jump some neighbours changed and some did not, so both branches of the store ran.  5 120 queries take the
   four-wave form, 102 400 the one-wave workgroups with the query order (rebuilt once inside the sequence).
   fdcap_debug_contact_diet says which path the launches took.  Only the one-wave form keeps records (in the other forms the
   bookkeeping cost more than the stores): in the large case 44 of the 45 default launches keep records (the first one seeds), none
   of the reference's, and the launches run under a query order that is built after the seeding launch and rebuilt inside the
   sequence; in the small case no launch keeps records and both settings must still leave the same memory.

2. skin_bwd_vec_kernel forms the world vertex and the distance instead of staging Vw and dist, and stages ja_hi rows of A
   (ContactGradIn::recompute).  tests/test_gpu_pose_trim.py's shapes (19 frames, a 400-vertex body, a 2000-point scene), 12
   iterations, against FDCAP_CONTACT_RECOMPUTE=0 FDCAP_NN_KEEP_RECORDS=0: body_rec, scale, camera_ext and every logged loss have the
   same bytes.  Contact sets: one leg; both legs; both legs and a vertex skinned to a joint >= 12 (ja_hi > 12) -- that vertex takes
   the place of one leg vertex, because the vec form serves sets of a multiple of four vertices and the test asserts that it ran.
   Also a (7, 6, 6) batch, a body with 8 skinning weights per vertex (G = 2), and a clip in which one frame's translation is NaN:
   its queries have no neighbour, and the bytes compared include the NaNs.
   These fits are far below the size at which the search takes its streaming form by itself (2^22 query-scene pairs), and only that
   form leaves the records the backward forms its distance from: fdcap_set_nn_kernel(2) selects it for them whatever the size, as
   tests/test_gpu_parity.py does for the in-loop state.  Every fit asserts that nn_stream4_kernel ran, that the default run's
   skinning backwards formed Vw and dist themselves and its searches kept records, and that the reference run did neither.
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from fdcap_amd.fitting import ClipBatchFitter, FittingOP, first_phase2_iter
from fdcap_amd.io import read_camerapose

pytestmark = pytest.mark.gpu
SWITCHES = ("FDCAP_NN_KEEP_RECORDS", "FDCAP_CONTACT_RECOMPUTE")


def _set(monkeypatch, default):
    for name in SWITCHES:                                  # (read by every fdcap_opt_create)
        if default: monkeypatch.delenv(name, raising=False)
        else: monkeypatch.setenv(name, "0")


def _diet(ctx):
    """(search launches that kept records, skinning backwards that formed Vw / dist, launches under a query order, its rebuilds)"""
    out = (ctypes.c_int32 * 4)()
    capi.check(ctx.lib.fdcap_debug_contact_diet(ctx.handle, out), "fdcap_debug_contact_diet")
    return tuple(out)


def _forms(reset):
    buf = ctypes.create_string_buffer(4096)
    capi.check(capi.load_library().fdcap_debug_kernel_forms(buf, len(buf), 1 if reset else 0), "kernel_forms")
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the search's records

def _sequence(n, per_part, keep, monkeypatch):
    if keep: monkeypatch.delenv("FDCAP_NN_KEEP_RECORDS", raising=False)
    else: monkeypatch.setenv("FDCAP_NN_KEEP_RECORDS", "0")
    seed = 60
    bm = synth.make_body_model(1000, seed=seed)
    vp = synth.make_vposer(seed=seed + 1)
    clip = synth.make_clip(n, seed=seed + 2)
    scene = synth.make_scene(70_000, seed=seed + 3)
    left, right = synth.make_contact_ids(bm.v_template, per_part=per_part, seed=seed + 4)
    vid = np.concatenate([left, right])
    fop = FittingOP({"num_iter": 8}, {"weight_contact": 0.1}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid,
                    camera_ext=read_camerapose(clip.camerapose_lines))
    lib, h = fop.ctx.lib, fop.ctx.handle
    x78 = torch.empty(n, 78, device="cuda")
    capi.check(lib.fdcap_params_75_to_78(capi.dptr(torch.tensor(clip.body_params).cuda()), n, capi.dptr(x78), capi.current_stream()), "75->78")
    fop.init(x78)
    _forms(True)
    g = torch.Generator(device="cuda").manual_seed(11)
    nc = len(vid)
    out = []
    for k in range(45):
        step = 0.03 if k == 25 else 0.001
        fop._rows_x[2:2 + n, 0:3] += step * torch.randn(n, 3, device="cuda", generator=g)
        d = torch.empty(n, nc, device="cuda")
        i = torch.empty(n, nc, device="cuda", dtype=torch.int32)
        rec = torch.full((n, nc, 4), float("nan"), device="cuda")
        capi.check(lib.fdcap_opt_forward_world(h, capi.dptr(torch.empty(n, nc, 3, device="cuda")), None, capi.current_stream()), "fw")
        capi.check(lib.fdcap_opt_get_contact(h, capi.dptr(d), capi.dptr(i), capi.current_stream()), "gc")
        capi.check(lib.fdcap_debug_nn_records(h, capi.dptr(rec), capi.current_stream()), "records")
        out.append((d, i, rec))
    torch.cuda.synchronize()
    out = [(d.cpu(), i.cpu(), r.cpu()) for d, i, r in out]
    forms = _forms(False)
    diet = _diet(fop.ctx)
    fop.close()
    return out, forms, torch.tensor(scene), diet


@pytest.mark.parametrize("n,per_part,form", [(64, 40, "nn_stream4_kernel(4 waves per group)"), (256, 200, "nn_stream4_kernel<1,1,1>")])
def test_records_written_only_when_changed_equal_records_always_written(n, per_part, form, monkeypatch):
    want, forms0, _, diet0 = _sequence(n, per_part, False, monkeypatch)
    got, forms1, scene, diet1 = _sequence(n, per_part, True, monkeypatch)
    assert form in forms0 and form in forms1, (forms0, forms1)
    if "<1,1,1>" in form:
        assert diet0[0] == 0 and diet1[0] == 44, (diet0, diet1)                   # every launch but the seeding one kept records
        assert diet1[2] >= 40 and diet1[3] >= 2 and diet0[2:] == diet1[2:], (diet0, diet1)   # the query order: in use, rebuilt inside the sequence
    else:                                                                         # only the one-wave form keeps records (and takes a query order)
        assert diet0[0] == 0 and diet1[0] == 0 and diet1[2] == 0, (diet0, diet1)
    for k, ((d0, i0, r0), (d1, i1, r1)) in enumerate(zip(want, got)):
        assert torch.equal(d0, d1) and torch.equal(i0, i1), k
        assert torch.equal(r0.view(torch.int32), r1.view(torch.int32)), k          # (bits: .w carries an integer)
        assert int(i1.min()) >= 0
        assert torch.equal(r1[..., :3], scene[i1.long()]), k                      # the records are the coordinates of idx
    changed = [float((got[k][1] != got[k - 1][1]).float().mean()) for k in range(1, 25)]
    print("share of queries whose neighbour changed, launches 1..24:", " ".join(f"{c:.4f}" for c in changed))
    assert any(0.0 < c < 1.0 for c in changed), changed                           # both branches of the store ran
    assert not torch.equal(got[24][1], got[25][1])                                # the jump really changed neighbours


# ---------------------------------------------------------------------------------------------------------------------
# 2. the bytes of a fit

N, V, NS, ITERS = 19, 400, 2000, 12


@pytest.fixture(scope="module")
def model():
    out = {}
    for nnz in (4, 8):
        bm = synth.make_body_model(V, seed=51, lbs_nnz=nnz)
        left, right = synth.make_contact_ids(bm.v_template, per_part=32, seed=54)
        assert len(left) == 32 and len(right) == 32
        top = np.array([np.flatnonzero(w).max() for w in bm.lbs_weights])       # highest joint each vertex is skinned to
        legs = np.concatenate([left, right])
        high = np.flatnonzero((top >= 12) & ~np.isin(np.arange(V), legs))
        assert high.size
        sets = {"one leg": (left, left[:0]), "legs": (left, right), "legs+high": (left, np.append(right[:-1], high[0]))}
        ja = {k: int(top[np.concatenate(v)].max()) + 1 for k, v in sets.items()}
        out[nnz] = (bm, sets, ja)
    assert out[4][2]["legs+high"] > 12 and all(len(np.concatenate(s)) % 4 == 0 for s in out[4][1].values())
    return out, synth.make_vposer(seed=52), synth.make_scene(NS, seed=53)


@pytest.fixture(autouse=True)
def _streaming_search():
    lib = capi.load_library()
    capi.check(lib.fdcap_set_nn_kernel(2), "set_nn_kernel")            # the streaming search whatever the size (module docstring)
    yield
    capi.check(lib.fdcap_set_nn_kernel(0), "set_nn_kernel")


def _check_paths(default, forms, diet, n_phase1):
    assert "skin_bwd_vec_kernel" in forms and "nn_stream4_kernel" in forms, forms
    if default: assert diet[1] == n_phase1, diet                              # every phase-1 backward (the searches of fits this small: a multi-wave form, records not kept)
    else: assert diet[0] == 0 and diet[1] == 0, diet


def _fit(model, which, log_every, default, monkeypatch, nnz=4, nan_frame=None):
    per, vp, scene = model
    bm, sets, _ = per[nnz]
    left, right = sets[which]
    clip = synth.make_clip(N, seed=55, num_outliers=2)
    params = np.array(clip.body_params, copy=True)
    if nan_frame is not None: params[nan_frame, 0:3] = np.nan
    _set(monkeypatch, default)
    _forms(True)
    fop = FittingOP({"num_iter": ITERS}, {}, N, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=np.concatenate([left, right]),
                    camera_ext=read_camerapose(clip.camerapose_lines), n_left=len(left))
    body, scale, cam = fop.fitting(torch.tensor(params).cuda(), "global", log_every=log_every)
    out = {"body": body.cpu().numpy(), "scale": np.float32(scale), "cam": cam.cpu().numpy()}
    if log_every:
        for k, v in dataclasses.asdict(fop.log).items(): out["log_" + k] = np.asarray(v, dtype=np.float64)
    _check_paths(default, _forms(False), _diet(fop.ctx), first_phase2_iter(ITERS))
    fop.close()
    return out


def _same_bytes(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.ascontiguousarray(np.atleast_1d(a[k])), np.ascontiguousarray(np.atleast_1d(b[k]))
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert x.tobytes() == y.tobytes(), (k, int((x.view(np.uint8) != y.view(np.uint8)).sum()), "bytes differ")


@pytest.mark.parametrize("log_every", [0, 1, 3])
@pytest.mark.parametrize("which", ["one leg", "legs", "legs+high"])
def test_a_fit_that_forms_vw_and_dist_gives_the_bytes_of_the_staged_ones(model, which, log_every, monkeypatch):
    got = _fit(model, which, log_every, True, monkeypatch)
    want = _fit(model, which, log_every, False, monkeypatch)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    if log_every: assert len(got["log_total"]) == len([i for i in range(ITERS) if i % log_every == 0 or i == ITERS - 1])
    _same_bytes(got, want)


def test_eight_skinning_weights_per_vertex(model, monkeypatch):
    got = _fit(model, "legs", 1, True, monkeypatch, nnz=8)
    want = _fit(model, "legs", 1, False, monkeypatch, nnz=8)
    assert all(np.all(np.isfinite(v)) for v in got.values())
    _same_bytes(got, want)


def test_a_frame_without_neighbours(model, monkeypatch):
    """One frame's translation is NaN: its world vertices are NaN, its queries find no neighbour, the search leaves them the distance
    the backward now has to supply itself.  The first logged iteration still has finite frames next to it."""
    got = _fit(model, "legs", 1, True, monkeypatch, nan_frame=7)
    want = _fit(model, "legs", 1, False, monkeypatch, nan_frame=7)
    assert np.isnan(got["body"]).any()
    _same_bytes(got, want)


def test_a_batch_of_clips(model, monkeypatch):
    per, vp, scene = model
    bm, sets, _ = per[4]
    left, right = sets["legs"]
    clips = []
    for seed, n in ((61, 7), (62, 6), (63, 6)):
        c = synth.make_clip(n, seed=seed, num_outliers=1)
        clips.append((c.body_params, read_camerapose(c.camerapose_lines)))
    res = []
    for default in (True, False):
        _set(monkeypatch, default)
        _forms(True)
        f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=np.concatenate([left, right]))
        out = {}
        for k, ((b, s, c), log) in enumerate(zip(f.fit(clips, scene, log_every=1), f.logs)):
            out[f"{k}_body"] = b.cpu().numpy(); out[f"{k}_scale"] = np.float32(s); out[f"{k}_cam"] = c.cpu().numpy()
            for name, v in dataclasses.asdict(log).items(): out[f"{k}_log_{name}"] = np.asarray(v, dtype=np.float64)
        _check_paths(default, _forms(False), _diet(f.ctx), first_phase2_iter(ITERS))
        f.close()
        res.append(out)
    _same_bytes(res[0], res[1])
