"""The Python drivers' side of the library boundary, pinned: for every mode and switch of FittingOP.fitting and ClipBatchFitter.fit
the sequence of library calls with their scalar arguments, and every logged number, equal what tests/driver_trace.json holds -- the
project's own recording (this file run as a script: `python tests/test_gpu_driver_trace.py OUT.json`), made before fitting.py's
loops were folded into one skeleton.  A driver change that adds, drops, reorders or re-parametrises a call shows here by name.

Shapes: a 200-vertex body, a 1500-point scene, 2 x 8 contact vertices; 7 frames and num_iter = 10 (phase 2 from iteration 8, a second
loop of 4) for 'global' / 'local'; 60 frames and dct_num_iter = 40 (second phase from iteration 38) for 'dct'.  The sharded paths
need several processes and are pinned bit for bit by tests/test_gpu_sharded.py."""
import ctypes
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import synth
from fdcap_amd.fitting import ClipBatchFitter, FittingOP
from fdcap_amd.io import load_dct_base, read_camerapose

pytestmark = pytest.mark.gpu
STORE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "driver_trace.json")
_POINTERS = (ctypes._Pointer, ctypes.c_void_p, ctypes.Array, type(ctypes.byref(ctypes.c_int32())))


class Recorder:
    """Stands in for ctx.lib: forwards every attribute, notes (function name, [scalar arguments]) per call -- ints and floats as
    they are, None as null, every pointer as "p"."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = []

    @staticmethod
    def _arg(a):
        if a is None or isinstance(a, (int, float)):
            return int(a) if isinstance(a, bool) else a
        if isinstance(a, _POINTERS):
            return "p"
        raise TypeError(f"argument of a kind the recorder does not know: {a!r}")

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append([name, [self._arg(a) for a in args]])
            return fn(*args)
        return call


def _traced(owner, fit):
    """fit() with owner.ctx.lib recorded -> (what fit returned, the calls)"""
    lib = owner.ctx.lib
    rec = owner.ctx.lib = Recorder(lib)
    try:
        return fit(), rec.calls
    finally:
        owner.ctx.lib = lib


def _hex(v):
    """a logged structure with every float as its hex string (nothing rounded; NaN as 'nan')"""
    if isinstance(v, (list, tuple)):
        return [_hex(x) for x in v]
    if isinstance(v, (float, np.floating)):
        return float(v).hex()
    return int(v)


_MODEL = []


def _model():
    if not _MODEL:
        bm = synth.make_body_model(200, seed=131)
        l, r = synth.make_contact_ids(bm.v_template, per_part=8, seed=135)
        _MODEL.append((bm, synth.make_vposer(seed=132), synth.make_scene(1500, seed=134), np.concatenate([l, r]), load_dct_base(None)))
    return _MODEL[0]


def _clip(seed, n):
    """(body [n,75], camera_ext [n,4,4], c_dct_init [n // 60,23,3,5])"""
    c = synth.make_clip(n, seed=seed, num_outliers=2 if n >= 60 else 1)
    c0 = np.random.Generator(np.random.PCG64(seed + 1000)).standard_normal((n // 60, 23, 3, 5)).astype(np.float32)
    return c.body_params, read_camerapose(c.camerapose_lines), c0


OPTIONS = dict(log_every=3, snapshot_at=[2, 10], check_finite_every=4, checkpoint_every=5)
DCT = dict(log_every=5, checkpoint_every=10, check_finite_every=4)
# name: (mode, fitting()'s keywords, environment, legacy_zero_grad)
SINGLE = {
    "global": ("global", {}, {}, False),
    "global-options": ("global", OPTIONS, {}, False),
    "global-python-loop": ("global", {}, {"FDCAP_C_LOOP": "0"}, False),
    "global-options-python-loop": ("global", OPTIONS, {"FDCAP_C_LOOP": "0"}, False),
    "global-step-launches": ("global", {}, {"FDCAP_DEFER_STEP": "0"}, False),
    "global-resumed": ("global", dict(log_every=3, snapshot_at=[10], check_finite_every=4, resume=True), {}, False),
    "local": ("local", dict(log_every=2, checkpoint_every=6, check_finite_every=3), {}, False),
    "dct": ("dct", DCT, {}, False),
    "dct-legacy": ("dct", DCT, {}, True),
}
# name: (mode, log_every, clip lengths)
BATCH = {
    "clips-global": ("global", 2, (7, 7)), "clips-global-ragged": ("global", 2, (7, 5)),
    "clips-local": ("local", 2, (7, 7)), "clips-local-ragged": ("local", 2, (7, 5)),
    "clips-dct": ("dct", 5, (60, 60)), "clips-dct-ragged": ("dct", 5, (60, 75)),
}


def _single(name, tmp):
    mode, kw, env, legacy = SINGLE[name]
    bm, vp, scene, vid, D = _model()
    n = 60 if mode == "dct" else 7
    body, cam, c0 = _clip(140, n)
    kw = dict(kw)

    def fop():
        return FittingOP({"num_iter": 10}, {}, n, body_model=bm, vposer=vp, scene_verts=scene, contact_ids=vid, camera_ext=cam,
                         dct_mtx=D, c_dct_init=c0, dct_num_iter=40, legacy_zero_grad=legacy)
    if kw.get("checkpoint_every"):
        kw["checkpoint_path"] = os.path.join(tmp, name + ".npz")
    if kw.pop("resume", False):               # the iteration-5 checkpoint: what a fit with checkpoint_every=5 leaves (none after the last)
        kw["resume"] = os.path.join(tmp, name + ".from.npz")
        f = fop()
        f.fitting(torch.tensor(body).cuda(), mode, checkpoint_every=5, checkpoint_path=kw["resume"])
        f.close()
    f = fop()
    _, calls = _traced(f, lambda: f.fitting(torch.tensor(body).cuda(), mode, **kw))
    logs = {"log": [f.log.iters, f.log.l_rec, f.log.l_vposer, f.log.loss_smoothing, f.log.loss_contact, f.log.loss_world_smoothing,
                    f.log.total],
            "log2": getattr(f, "log2", []), "log_dct": getattr(f, "log_dct", [])}
    f.close()
    return calls, logs


def _batch(name):
    mode, log_every, lens = BATCH[name]
    bm, vp, scene, vid, D = _model()
    clips = [_clip(150 + k, n) for k, n in enumerate(lens)]
    f = ClipBatchFitter({"num_iter": 10}, {}, body_model=bm, vposer=vp, contact_ids=vid, dct_num_iter=40)
    _, calls = _traced(f, lambda: f.fit([(c[0], c[1]) for c in clips], scene, log_every=log_every, mode=mode, dct_mtx=D,
                                        c_dct_init=[c[2] for c in clips] if mode == "dct" else None))
    logs = {"logs": [[g.iters, g.l_rec, g.l_vposer, g.loss_smoothing, g.loss_contact, g.loss_world_smoothing, g.total] for g in f.logs],
            "logs2": f.logs2, "logs_dct": f.logs_dct}
    f.close()
    return calls, logs


def run_case(name, tmp):
    """-> {"calls": [[function, [arguments]], ...], "logs": {attribute: hex floats}} of one case, under the case's environment"""
    env = SINGLE[name][2] if name in SINGLE else {}
    old = {k: os.environ.get(k) for k in ("FDCAP_C_LOOP", "FDCAP_DEFER_STEP")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        calls, logs = _single(name, tmp) if name in SINGLE else _batch(name)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return {"calls": calls, "logs": {k: _hex(v) for k, v in logs.items()}}


def _dump(cases, path):
    """one call / one log per line: a changed call is a changed line"""
    out = ["{"]
    for i, (name, c) in enumerate(cases.items()):
        out.append(f' {json.dumps(name)}: {{"calls": [')
        out.append(",\n".join("  " + json.dumps(call) for call in c["calls"]))
        out.append(' ], "logs": {')
        out.append(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in c["logs"].items()))
        out.append(" }}" + ("," if i + 1 < len(cases) else ""))
    out.append("}")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


@pytest.fixture(scope="module")
def stored():
    with open(STORE) as f:
        return json.load(f)


def test_the_recording_holds_exactly_these_cases(stored):
    assert sorted(stored) == sorted([*SINGLE, *BATCH])


@pytest.mark.parametrize("name", [*SINGLE, *BATCH])
def test_library_calls_and_logged_numbers_are_the_recorded_ones(name, stored, tmp_path):
    got = json.loads(json.dumps(run_case(name, str(tmp_path))))
    want = stored[name]
    assert len(want["calls"]) > 0
    for k, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, f"call {k}: {g} -- recorded: {w}"
    assert len(got["calls"]) == len(want["calls"])
    assert got["logs"] == want["logs"]
    if name == "global":
        assert [c[0] for c in got["calls"]].count("fdcap_opt_run") == 1


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp_dir:
        _dump({name: run_case(name, tmp_dir) for name in [*SINGLE, *BATCH]}, sys.argv[1])
