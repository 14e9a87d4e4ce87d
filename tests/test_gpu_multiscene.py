"""Clips of DIFFERENT scenes in one batch (fdcap_set_scene_slot + fdcap_opt_create_clips_scenes, ClipBatchFitter.fit(scenes=...,
clip_scene=...)) against the stand-alone fits of its clips, each against its own scene: the same bits through the one-launch
segmented search and through the per-segment loop (FDCAP_NN_SEGMENTS=loop), the neighbour records of one forward against the
every-pair operator, edge shapes, independence of the segments, the full body through the clip-sized forms, the refusals and the
ownership of the slots.  Shapes: a 300-vertex body, 2 x 16 contact vertices, scene A of 3 000 points, scene B of 4 133 points (no
multiple of the 512-point cell) -- A's kind of surface 0.3 m higher, sampled anew and shuffled --, 20 iterations (phase switch at 16).
tests/test_multiscene_cpu.py pins the segment tables and the launch decisions of the sizes used here.

A clip of a batch equals its stand-alone fit bit for bit where both select the same kernel forms (include/fdcap.h).  The comparisons
therefore run in child processes (this file as a script) that pin the forms for both sides: FDCAP_CLIP_FORMS_MIN_ROWS (read once per
process; 1024 keeps every fit here, 3 to 97 rows, below the clip-sized forms, 64 puts the full body's 100 and 75 rows on them),
FDCAP_NN_STREAM=11 (the one-wave streaming search at every size, the form the segmented launch is) and
fdcap_set_nn_kernel(2); each test below asserts its scenario's outcome."""
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
from fdcap_amd.fitting import ClipBatchFitter, FittingOP, first_phase2_iter
from fdcap_amd.io import read_camerapose

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 20
E_ARG, E_STATE = -1, -2
SEGMENTS, ONE_WAVE = "nn_stream4_kernel(1 wave per group, segments)", "nn_stream4_kernel<1,1,1>"
FIELDS = ("iters", "l_rec", "l_vposer", "loss_smoothing", "loss_contact", "loss_world_smoothing", "total")


def _scenes(n_a=3000, n_b=4133):
    b = synth.make_scene(n_b, seed=137) + np.array([0.0, 0.0, 0.3], np.float32)
    b2 = synth.make_scene(n_b, seed=139) + np.array([0.0, 0.0, 0.45], np.float32)
    return {"A": synth.make_scene(n_a, seed=134), "B": b.astype(np.float32), "B2": b2.astype(np.float32)}


def _model():
    bm = synth.make_body_model(300, seed=131)
    vp = synth.make_vposer(seed=132)
    l, r = synth.make_contact_ids(bm.v_template, per_part=16, seed=135)
    return bm, vp, np.concatenate([l, r]), _scenes()


_CLIPS = {}


def _clip(seed, n):
    if (seed, n) not in _CLIPS:
        c = synth.make_clip(n, seed=seed, num_outliers=2 if n >= 8 else 0)
        _CLIPS[(seed, n)] = (c.body_params, read_camerapose(c.camerapose_lines))
    return _CLIPS[(seed, n)]


def _forms(reset):
    buf = ctypes.create_string_buffer(4096)
    capi.load_library().fdcap_debug_kernel_forms(buf, 4096, 1 if reset else 0)
    return buf.value.decode()


def _pack(body, scale, cam, log, idx1):
    return (body.cpu().numpy(), float(scale), cam.cpu().numpy(), {f: np.array(getattr(log, f), dtype=np.float64) for f in FIELDS}, np.asarray(idx1))


_ALONE = {}


def _alone(model, seed, n, scene, iters=ITERS):
    """The stand-alone fit of clip (seed, n) against `scene`, computed once per process and never changed."""
    key = (seed, n, scene, iters)
    if key not in _ALONE:
        bm, vp, vid, scenes = model
        body, cam = _clip(seed, n)
        _forms(True)
        fop = FittingOP({"num_iter": iters}, {}, n, body_model=bm, vposer=vp, scene_verts=scenes[scene], contact_ids=vid, camera_ext=cam)
        b, s, c = fop.fitting(torch.tensor(body).cuda(), "global", log_every=1)
        _ALONE[key] = (_pack(b, s, c, fop.log, fop.idx1), _forms(False))
        fop.close()
    return _ALONE[key]


def _batch(model, spec, loop=False, via_fit=False, iters=ITERS, plain=False):
    """spec: ((seed, n, scene name), ...) in batch order -> each clip's results as _alone gives them, and the forms the batch noted.
    via_fit: through ClipBatchFitter.fit(scenes=, clip_scene=), which orders the clips itself; else the clips enter the batch in
    spec's order (prepare(clip_slots=...)), slots in order of first use.  plain: fdcap_opt_create_clips[_var] on slot 0 (one scene)."""
    bm, vp, vid, scenes = model
    clips = [_clip(s, n) for s, n, _ in spec]
    names = [sc for _, _, sc in spec]
    uniq = list(dict.fromkeys(names))
    if loop:
        os.environ["FDCAP_NN_SEGMENTS"] = "loop"
    _forms(True)
    f = ClipBatchFitter({"num_iter": iters}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    try:
        if via_fit:
            res = f.fit(clips, log_every=1, scenes=[(nm, scenes[nm]) for nm in uniq], clip_scene=[uniq.index(nm) for nm in names])
        else:
            for i, nm in enumerate(uniq):
                f.ctx.set_scene_slot(i, scenes[nm])
            f.prepare(clips, clip_slots=None if plain else [uniq.index(nm) for nm in names])
            res = f.run(1)
        out = [_pack(b, s, c, f.logs[k], f.idx1[k]) for k, (b, s, c) in enumerate(res)]
    finally:
        f.close()
        os.environ.pop("FDCAP_NN_SEGMENTS", None)
    return out, _forms(False)


def _diff(a, b):
    """what differs between two packed results (bit for bit: the logged sums are per-frame float partials in one fixed order)"""
    bad = []
    if a[0].shape != b[0].shape or not np.array_equal(a[0], b[0]):
        bad.append("body_rec")
    if not (np.all(np.isfinite(a[0])) and np.isfinite(a[1])):
        bad.append("not finite")
    if a[1] != b[1]:
        bad.append(f"scale {a[1]!r} {b[1]!r}")
    if not np.array_equal(a[2], b[2]):
        bad.append("camera_ext")
    for f in FIELDS:
        if a[3][f].shape != b[3][f].shape or not np.array_equal(a[3][f], b[3][f]):
            bad.append("log " + f)
    if not np.array_equal(a[4], b[4]):
        bad.append("idx1")
    return bad


def _formset(s):
    return sorted(set(s.split(";")) - {""})


def _against_alone(model, spec, out, iters=ITERS, forms=None):
    """forms: what the batch noted -- every stand-alone fit must have noted the same forms, the search's one launch for all segments
    standing for the one-wave launch it is"""
    bad = []
    for k, (seed, n, scene) in enumerate(spec):
        alone, aforms = _alone(model, seed, n, scene, iters)
        bad += [f"clip {k} ({n} frames, scene {scene}): {d}" for d in _diff(out[k], alone)]
        if forms is not None and _formset(forms.replace(SEGMENTS, ONE_WAVE)) != _formset(aforms):
            bad.append(f"clip {k}: forms {_formset(forms)} vs stand-alone {_formset(aforms)}")
    return bad


MAIN = ((61, 40, "A"), (62, 33, "B"), (63, 24, "A"))


def _sc_main_segmented(model):
    """(40, 33, 24) frames on (A, B, A): three segments, one launch"""
    out, forms = _batch(model, MAIN)
    assert SEGMENTS in forms, forms
    assert len(out[0][3]["iters"]) == ITERS and first_phase2_iter(ITERS) == 16
    bad = _against_alone(model, MAIN, out, forms=forms)
    assert not bad, bad
    assert SEGMENTS not in _alone(model, 61, 40, "A")[1] and ONE_WAVE in _alone(model, 61, 40, "A")[1]
    # not vacuous: clip B fitted against scene A is another fit
    assert "body_rec" in _diff(out[1], _alone(model, 62, 33, "A")[0])
    return "ok"


def _sc_main_loop(model):
    out, forms = _batch(model, MAIN, loop=True)
    assert SEGMENTS not in forms and ONE_WAVE in forms, forms
    bad = _against_alone(model, MAIN, out, forms=forms)
    assert not bad, bad
    return "ok"


def _sc_fit_orders_the_clips(model):
    """fit(scenes=, clip_scene=) makes every scene one run (A, A, B) and hands the results back in the caller's order (A, B, A)"""
    out, forms = _batch(model, MAIN, via_fit=True)
    assert SEGMENTS in forms, forms
    bad = _against_alone(model, MAIN, out, forms=forms)
    assert not bad, bad
    return "ok"


def _sc_records(model):
    """after ONE forward: dist / idx of every clip against fdcap_chamfer_fwd of its contact vertices and its own scene"""
    bm, vp, vid, scenes = model
    bad = []
    for loop in (False, True):
        if loop:
            os.environ["FDCAP_NN_SEGMENTS"] = "loop"
        f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
        try:
            f.ctx.set_scene_slot(0, scenes["A"])
            f.ctx.set_scene_slot(1, scenes["B"])
            f.prepare([_clip(s, n) for s, n, _ in MAIN], clip_slots=[0, 1, 0])
            lib, h, st = f.ctx.lib, f.ctx.handle, capi.current_stream()
            total, nc = sum(n for _, n, _ in MAIN), len(vid)
            verts = torch.empty(total, nc, 3, device="cuda")
            d = torch.empty(total, nc, device="cuda")
            i = torch.empty(total, nc, device="cuda", dtype=torch.int32)
            _forms(True)
            capi.check(lib.fdcap_opt_forward_world(h, capi.dptr(verts), None, st), "forward_world")
            capi.check(lib.fdcap_opt_get_contact(h, capi.dptr(d), capi.dptr(i), st), "get_contact")
            assert (SEGMENTS in _forms(False)) == (not loop)
            row = 0
            for k, (_, n, scene) in enumerate(MAIN):
                tgt = torch.tensor(scenes[scene]).cuda().contiguous()
                q = verts[row:row + n].reshape(1, n * nc, 3).contiguous()
                d1 = torch.empty(1, n * nc, device="cuda")
                i1 = torch.empty(1, n * nc, device="cuda", dtype=torch.int32)
                capi.check(lib.fdcap_chamfer_fwd(h, capi.dptr(q), capi.dptr(tgt), 1, n * nc, tgt.shape[0], 0, capi.dptr(d1), capi.dptr(i1), None, None, st),
                           "chamfer_fwd")
                torch.cuda.synchronize()
                if not torch.equal(d[row:row + n].reshape(-1), d1.reshape(-1)):
                    bad.append(f"loop={loop} clip {k}: dist")
                if not torch.equal(i[row:row + n].reshape(-1), i1.reshape(-1)):
                    bad.append(f"loop={loop} clip {k}: idx")
                if not (int(i[row:row + n].min()) >= 0 and int(i[row:row + n].max()) < tgt.shape[0]):
                    bad.append(f"loop={loop} clip {k}: idx outside its scene")
                row += n
        finally:
            f.close()
            os.environ.pop("FDCAP_NN_SEGMENTS", None)
    assert not bad, bad
    return "ok"


def _sc_edges(model):
    bad = []
    # a 3-frame clip as a segment of its own at either end
    spec = ((71, 3, "B"), (61, 40, "A"), (72, 3, "B"))
    for loop in (False, True):
        out, forms = _batch(model, spec, loop=loop)
        assert (SEGMENTS in forms) == (not loop), forms
        bad += [f"loop={loop} {b}" for b in _against_alone(model, spec, out, forms=forms)]
    # a one-clip batch through the new call, on a slot that is not slot 0's scene
    bm, vp, vid, scenes = model
    f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    try:
        f.ctx.set_scene_slot(0, scenes["A"])
        f.ctx.set_scene_slot(1, scenes["B"])
        f.prepare([_clip(62, 33)], clip_slots=[1])
        (b, s, c), = f.run(1)
        bad += [f"one clip on slot 1: {d}" for d in _diff(_pack(b, s, c, f.logs[0], f.idx1[0]), _alone(model, 62, 33, "B")[0])]
    finally:
        f.close()
    # all clips on slot 0: fdcap_opt_create_clips_var's bits (different lengths) and fdcap_opt_create_clips' (one length)
    for spec in (((61, 40, "A"), (64, 33, "A"), (63, 24, "A")), ((61, 40, "A"), (65, 40, "A"))):
        new, forms = _batch(model, spec)
        old, _ = _batch(model, spec, plain=True)
        assert SEGMENTS not in forms, forms
        for k in range(len(spec)):
            bad += [f"one slot, clip {k}: {d}" for d in _diff(new[k], old[k])]
    assert not bad, bad
    return "ok"


def _sc_independence(model):
    """clip A's bits do not move with scene B's points or clip B's data"""
    base, _ = _batch(model, ((61, 40, "A"), (62, 33, "B")))
    bad = []
    for name, spec in (("scene B changed", ((61, 40, "A"), (62, 33, "B2"))), ("clip B changed", ((61, 40, "A"), (66, 33, "B"))),
                       ("clip B longer", ((61, 40, "A"), (67, 57, "B")))):
        out, forms = _batch(model, spec)
        assert SEGMENTS in forms
        bad += [f"{name}: {d}" for d in _diff(out[0], base[0])]
        assert "body_rec" in _diff(out[1], base[1]), name           # (the other clip did change)
    assert not bad, bad
    return "ok"


def _live():
    out = (ctypes.c_int64 * 3)()
    capi.check(capi.load_library().fdcap_debug_live_allocations(out), "live_allocations")
    return tuple(out)


def _sc_refusals(model):
    bm, vp, vid, scenes = model
    torch.cuda.synchronize()
    start = _live()
    f = ClipBatchFitter({"num_iter": ITERS}, {}, body_model=bm, vposer=vp, contact_ids=vid)
    try:
        lib, h, st = f.ctx.lib, f.ctx.handle, capi.current_stream()
        clips = [_clip(s, n) for s, n, _ in MAIN]
        f.ctx.set_scene_slot(0, scenes["A"])
        f.ctx.set_scene_slot(1, scenes["B"])
        # a named slot that holds no scene; slots out of range
        with pytest.raises(capi.FdcapError, match="FDCAP_E_STATE"):
            f.prepare(clips, clip_slots=[0, 5, 0])
        for slots in ([0, 8, 0], [0, -1, 0]):
            with pytest.raises(capi.FdcapError, match="FDCAP_E_ARG"):
                f.prepare(clips, clip_slots=slots)
        f._destroy_opt()
        pts = np.ascontiguousarray(scenes["A"][:600])
        assert lib.fdcap_set_scene_slot(h, capi.MAX_SCENES, pts.ctypes.data_as(ctypes.c_void_p), 600) == E_ARG
        assert lib.fdcap_set_scene_slot(h, -1, pts.ctypes.data_as(ctypes.c_void_p), 600) == E_ARG
        for slot in range(2, capi.MAX_SCENES):                       # every slot filled
            f.ctx.set_scene_slot(slot, scenes["B" if slot % 2 else "A"][:1000 + 37 * slot])
        filled = _live()
        f.ctx.set_scene_slot(5, np.zeros((0, 3), np.float32))        # ns = 0 clears a slot and frees its tables
        assert _live()[0] == filled[0] - 8 and _live()[1] < filled[1]
        with pytest.raises(capi.FdcapError, match="FDCAP_E_STATE"):
            f.prepare(clips, clip_slots=[0, 5, 0])
        f._destroy_opt()
        f.ctx.set_scene_slot(5, scenes["B"][:1185])
        f.prepare(clips, clip_slots=[0, 1, 0])
        # a live optimiser: no slot is registered again, as fdcap_set_scene
        assert lib.fdcap_set_scene_slot(h, 3, pts.ctypes.data_as(ctypes.c_void_p), 600) == E_STATE
        assert lib.fdcap_set_scene_slot(h, 0, pts.ctypes.data_as(ctypes.c_void_p), 600) == E_STATE
        assert lib.fdcap_set_scene(h, pts.ctypes.data_as(ctypes.c_void_p), 600) == E_STATE
        total = sum(n for _, n, _ in MAIN)
        w = torch.zeros(total, device="cuda")
        hist = torch.zeros(4, 3, capi.NUM_LOSSES, device="cuda", dtype=torch.float64)
        D = np.ascontiguousarray(np.eye(60, 5, dtype=np.float32))
        c0 = torch.zeros(8, 23, 3, 5, device="cuda")
        n_done, f0, f1 = ctypes.c_int32(0), ctypes.c_float(0), ctypes.c_float(0)
        P = first_phase2_iter(ITERS)
        refused = {
            "run_local2": lib.fdcap_opt_run_local2(h, len(vid) // 2, 0, 2, ITERS, 0, capi.dptr(w), capi.dptr(hist), 4, 0, ctypes.byref(n_done), st),
            "detect_contact": lib.fdcap_opt_detect_contact(h, len(vid) // 2, capi.dptr(w), st),
            "backward_local2": lib.fdcap_opt_backward_local2(h, capi.dptr(w), len(vid) // 2, st),
            "set_dct_clips": lib.fdcap_opt_set_dct_clips(h, D.ctypes.data_as(ctypes.c_void_p), 60, 5, capi.dptr(c0), st),
            "set_dct": lib.fdcap_opt_set_dct(h, D.ctypes.data_as(ctypes.c_void_p), 60, 5, capi.dptr(c0), st),
            "run_dct": lib.fdcap_opt_run_dct(h, 0, 2, ITERS, 1.0, 1.0, 0.5, 0.1, 0, None, capi.dptr(hist), 4, 0, ctypes.byref(n_done), st),
            "set_keypoints": lib.fdcap_opt_set_keypoints(h, capi.dptr(w), st),
            "backward_fit2d": lib.fdcap_opt_backward_fit2d(h, None, 0, st),
            "fit2d_lbfgs": lib.fdcap_opt_fit2d_lbfgs(h, None, None, 1, None, st),
            "halo_exchange": lib.fdcap_opt_halo_exchange(h, st),
            "exchange": lib.fdcap_opt_exchange(h, 0, P, st),
            "time_exchange": lib.fdcap_opt_time_exchange(h, 1, ctypes.byref(f0), ctypes.byref(f1), st),
            "step_rows_and_pack": lib.fdcap_opt_step_rows_and_pack(h, 0, P, capi.dptr(w), st),
            "unpack_and_step_scale": lib.fdcap_opt_unpack_and_step_scale(h, 0, P, capi.dptr(w), 0, 1, st),
            "forward_ahead": lib.fdcap_opt_forward_ahead(h, 0, P, 0, st),
            "nn_query_order": lib.fdcap_debug_nn_query_order(h, 1, None, 0),
        }
        assert all(v == E_STATE for v in refused.values()), refused
        # ... and mode 'global' still runs after all of them
        res = f.run(1)
        assert len(res) == 3 and all(bool(torch.isfinite(b).all()) for b, _, _ in res)
        # Python: modes 'local' and 'dct' with several scenes raise before anything touches the device
        for mode in ("local", "dct"):
            f2 = ClipBatchFitter.__new__(ClipBatchFitter)            # (no context at all: reaching the device would raise AttributeError)
            f2.scene_key, f2._slot_keys = None, [None] * capi.MAX_SCENES
            with pytest.raises(ValueError, match="several scenes"):
                f2._fit_scenes([_clip(61, 60), _clip(62, 60)], [scenes["A"], scenes["B"]], [0, 1], 0, mode, None, None)
    finally:
        f.close()
    torch.cuda.synchronize()
    assert _live() == start, (_live(), start)
    return "ok"


_SCENARIOS = {"main_segmented": _sc_main_segmented, "main_loop": _sc_main_loop, "fit_orders_the_clips": _sc_fit_orders_the_clips,
              "records": _sc_records, "edges": _sc_edges, "independence": _sc_independence, "refusals": _sc_refusals}


def _sc_full_body():
    """(100, 75) frames on two 20 000-point scenes, 10 475 vertices, 500 contacts, FDCAP_CLIP_FORMS_MIN_ROWS=64: the fused contact forward's
    32-frame blocks and the K-split gradient's row blocks straddle the boundary between the two segments (rows 100 | 75)"""
    bm = synth.make_body_model(10475, seed=0)
    vp = synth.make_vposer(seed=1)
    l, r = synth.make_contact_ids(bm.v_template, per_part=250, seed=4)
    model = (bm, vp, np.concatenate([l, r]), _scenes(20000, 20000))
    spec, iters = ((61, 100, "A"), (62, 75, "B")), 6
    bad = []
    for loop in (False, True):
        out, forms = _batch(model, spec, loop=loop, iters=iters)
        assert (SEGMENTS in forms) == (not loop), forms
        assert "blend_skin_fwd_kernel" in forms and "panel_gemm3_rb2k_kernel" in forms, forms
        bad += [f"loop={loop} {b}" for b in _against_alone(model, spec, out, iters, forms)]
    for seed, n, scene in spec:
        af = _alone(model, seed, n, scene, iters)[1]
        assert "blend_skin_fwd_kernel" in af and "panel_gemm3_rb2k_kernel" in af and ONE_WAVE in af, af
    assert not bad, bad
    return "ok"


def _run_child(min_rows, *args):
    env = dict(os.environ)
    env["FDCAP_CLIP_FORMS_MIN_ROWS"] = str(min_rows)
    env["FDCAP_NN_STREAM"] = "11"
    env.pop("FDCAP_NN_SEGMENTS", None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), *args], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
    assert p.returncode == 0 and line, (p.stdout[-1500:], p.stderr[-3000:])
    print(p.stdout[-3000:])
    return json.loads(line[-1][7:])


@pytest.fixture(scope="module")
def child():
    # (above every row count here: the batch's 97 rows and a stand-alone fit's 3 to 57 all take the forms below the clip sizes --
    #  the switch's smallest value, 32, would still leave the 24- and 3-frame stand-alone fits on other forms than their batch)
    return _run_child(1024)


@pytest.mark.parametrize("name", sorted(_SCENARIOS))
def test_scenario(child, name):
    assert child[name] == "ok", child[name]


def test_full_body_segments_through_the_clip_sized_forms():
    assert _run_child(64, "full_body")["full_body"] == "ok"


if __name__ == "__main__":
    assert capi.load_library().fdcap_set_nn_kernel(2) == 0
    result = {}
    if sys.argv[1:] == ["full_body"]:
        todo = {"full_body": lambda m: _sc_full_body()}
        m = None
    else:
        todo, m = _SCENARIOS, _model()
    for name, fn in todo.items():
        try:
            result[name] = fn(m)
        except Exception:
            result[name] = traceback.format_exc()[-2500:]
    print("RESULT " + json.dumps(result))
