"""fdcap_set_scene's eight tables against the independent specification of tests/scene_spec.py, byte for byte, and the search that
prunes with them against the every-pair scan on the scenes where the tables have edges.

test_gpu_setup.py compares the hashes of a device build and a FDCAP_SCENE_BUILD=host build: that pins the cell ORDER only, since
both take their boxes, fragments and centres from the same kernels (sc_finalize_kernel, sc_super_kernel).  Here both builds must
equal scene_spec.tables_spec(xyz, scene_spec.order_spec(xyz)) -- all eight tables, every byte -- on every count of filled quarters
in the last cell, ragged super cells, extent-0 boxes, flat axes, ties, signed zeros and scenes far from the origin; and
fdcap_chamfer_fwd_scene must return what the plain scan returns, bit for bit, for queries near the surface, ON the padded cell and
quarter faces, on exact copies of scene points (the lowest index wins) and far away."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, synth
from tests import scene_spec as S
from tests.test_gpu_parity import _nn_check

pytestmark = pytest.mark.gpu

_EDGE = list(S.edge_scenes())
_IDS = [n for n, _ in _EDGE]
_DIMS = {"scene": ("point", "field x/y/z/index"), "sorted": ("position", "field x/y/z/index"), "inv": ("index",),
         "bounds": ("cell", "lo/hi", "field"), "qbounds": ("cell", "quarter", "lo/hi", "field"), "sbounds": ("super", "lo/hi", "field"),
         "frags": ("cell", "tile", "k-half", "point", "word"), "centers": ("cell", "field x/y/z/radius")}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(synth.make_body_model(400, seed=0), synth.make_vposer(seed=1))
    yield c
    c.close()


def _register(ctx, xyz, how):
    old = os.environ.get("FDCAP_SCENE_BUILD")
    try:
        if how == "host":
            os.environ["FDCAP_SCENE_BUILD"] = "host"
        else:
            os.environ.pop("FDCAP_SCENE_BUILD", None)
        ctx.set_scene(xyz)
    finally:
        if old is None:
            os.environ.pop("FDCAP_SCENE_BUILD", None)
        else:
            os.environ["FDCAP_SCENE_BUILD"] = old


def _read_tables(ctx, like):
    out = {}
    for k, name in enumerate(S.TABLES):
        nb = ctypes.c_int64(-1)
        capi.check(ctx.lib.fdcap_debug_scene_table(ctx.handle, k, None, ctypes.byref(nb)), "fdcap_debug_scene_table(size)")
        assert nb.value == like[name].nbytes, (name, nb.value, like[name].nbytes)
        buf = np.empty(like[name].shape, like[name].dtype)
        capi.check(ctx.lib.fdcap_debug_scene_table(ctx.handle, k, buf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nb)),
                   "fdcap_debug_scene_table")
        out[name] = buf
    return out


def _mismatches(spec, got):
    """'' when every table is equal byte for byte, else one line per table: the first differing element as (table, cell, field)"""
    lines = []
    for name in S.TABLES:
        w, g = spec[name].view(np.uint32), got[name].view(np.uint32)
        bad = w != g
        if bad.any():
            at = np.unravel_index(int(np.argmax(bad)), w.shape)
            where = ", ".join(f"{d} {i}" for d, i in zip(_DIMS[name], at))
            lines.append(f"{name}: {int(bad.sum())} words differ, first at {where}: spec {int(w[at]):#010x} "
                         f"({w[at].view(np.float32)!r}) device {int(g[at]):#010x} ({g[at].view(np.float32)!r})")
    return "\n".join(lines)


@pytest.mark.parametrize("name,xyz", _EDGE, ids=_IDS)
def test_both_builds_give_the_specified_tables(ctx, name, xyz):
    spec = S.scene_tables(xyz)
    for how in ("device", "host"):
        _register(ctx, xyz, how)
        msg = _mismatches(spec, _read_tables(ctx, spec))
        assert not msg, f"{how} build of {name}:\n{msg}"


def test_table_readback_refuses_bad_calls(ctx):
    nb = ctypes.c_int64(0)
    fresh = capi.Context(synth.make_body_model(400, seed=0), synth.make_vposer(seed=1))
    try:
        assert fresh.lib.fdcap_debug_scene_table(fresh.handle, 0, None, ctypes.byref(nb)) == -2        # no scene: FDCAP_E_STATE
    finally:
        fresh.close()
    ctx.set_scene(np.random.default_rng(0).uniform(-1, 1, (700, 3)).astype(np.float32))
    for which in (-1, 8):
        assert ctx.lib.fdcap_debug_scene_table(ctx.handle, which, None, ctypes.byref(nb)) == -1      # FDCAP_E_ARG
    capi.check(ctx.lib.fdcap_debug_scene_table(ctx.handle, 5, None, ctypes.byref(nb)), "size")
    assert nb.value == 32                                                                             # one super cell
    buf = np.zeros(64, np.uint8)
    nb.value = 31
    assert ctx.lib.fdcap_debug_scene_table(ctx.handle, 5, buf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nb)) == -1
    assert not buf.any()


# ---- the registered-scene search ----------------------------------------------------------------------------------------------------
def _queries(xyz, t, rng):
    """408 queries: 160 near the surface, 128 on padded cell and quarter faces (read back from the tables), 96 exact copies of
    scene points, 24 at 10 - 1000 m.  Returns them and the slice of the copies."""
    ns = len(xyz)
    near = xyz[rng.integers(0, ns, 160)] + rng.normal(0, 0.01, (160, 3)).astype(np.float32)
    faces = []
    for boxes in (t["bounds"][:, :, :3], t["qbounds"].reshape(-1, 2, 4)[:, :, :3]):
        boxes = boxes[np.isfinite(boxes).all((1, 2))]                        # (quarters without points: +inf)
        pick = boxes[rng.integers(0, len(boxes), 64)]
        lo, hi = pick[:, 0].astype(np.float64), pick[:, 1].astype(np.float64)
        f = (lo + rng.uniform(0, 1, lo.shape) * (hi - lo)).astype(np.float32)
        ax, side = rng.integers(0, 3, 64), rng.integers(0, 2, 64)
        f[np.arange(64), ax] = pick[np.arange(64), side, ax]                 # one coordinate exactly on a face
        f[:8], f[8:16] = pick[:8, 0], pick[8:16, 1]                          # ... and corners
        faces.append(f)
    copies = xyz[rng.integers(0, ns, 96)]
    d = rng.standard_normal((24, 3))
    far = xyz.mean(0, dtype=np.float64) + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(10, 1000, (24, 1))
    q = np.concatenate([near, *faces, copies, far.astype(np.float32)]).astype(np.float32)
    return q, slice(288, 384)


def _scan(ctx, q, scene_d):
    """the plain every-pair scan (nn_direct_kernel) over the same points"""
    B, n = q.shape[:2]
    d = torch.empty(B, n, device="cuda")
    i = torch.empty(B, n, device="cuda", dtype=torch.int32)
    capi.check(ctx.lib.fdcap_set_nn_kernel(1), "fdcap_set_nn_kernel")
    try:
        capi.check(ctx.lib.fdcap_chamfer_fwd(ctx.handle, capi.dptr(q), capi.dptr(scene_d), B, n, scene_d.shape[0], 0, capi.dptr(d),
                                             capi.dptr(i), None, None, capi.current_stream()), "fdcap_chamfer_fwd")
    finally:
        capi.check(ctx.lib.fdcap_set_nn_kernel(0), "fdcap_set_nn_kernel")
    torch.cuda.synchronize()
    return d, i


def _search(ctx, q, forget, mode):
    B, n = q.shape[:2]
    d = torch.empty(B, n, device="cuda")
    i = torch.empty(B, n, device="cuda", dtype=torch.int32)
    capi.check(ctx.lib.fdcap_set_nn_kernel(mode), "fdcap_set_nn_kernel")
    try:
        capi.check(ctx.lib.fdcap_chamfer_fwd_scene(ctx.handle, capi.dptr(q), B, n, capi.dptr(d), capi.dptr(i), forget,
                                                   capi.current_stream()), "fdcap_chamfer_fwd_scene")
    finally:
        capi.check(ctx.lib.fdcap_set_nn_kernel(0), "fdcap_set_nn_kernel")
    torch.cuda.synchronize()
    return d, i


def _sequence(ctx, q0, scene_d, rng, what):
    """forget = 1, then twice forget = 0 while the queries move by 1 mm; under both search modes, each call against the scan"""
    step = rng.standard_normal(q0.shape)
    step = torch.tensor((step / np.linalg.norm(step, axis=-1, keepdims=True) * 1e-3).astype(np.float32), device="cuda")
    for mode in (0, 2):
        q = q0
        for call, forget in enumerate((1, 0, 0)):
            if call:
                q = q + step
            sd, si = _search(ctx, q, forget, mode)
            rd, ri = _scan(ctx, q, scene_d)
            bad = (sd.view(torch.int32) != rd.view(torch.int32)) | (si != ri)
            assert not bool(bad.any()), (what, mode, call, int(bad.sum()), int(torch.nonzero(bad.reshape(-1))[0]))


@pytest.mark.parametrize("name,xyz", _EDGE, ids=_IDS)
def test_registered_scene_search_equals_the_plain_scan(ctx, name, xyz):
    rng = np.random.default_rng(len(xyz))
    ctx.set_scene(xyz)
    q, copies = _queries(xyz, _read_tables(ctx, S.scene_tables(xyz)), rng)
    scene_d = torch.tensor(xyz, device="cuda")
    q_d = torch.tensor(q.reshape(3, -1, 3), device="cuda")
    _sequence(ctx, q_d, scene_d, rng, "pool")
    for B, n in ((1, 1), (1, 31), (3, 11)):                                  # B n = 1, 31, 33
        sub = torch.tensor(q[rng.permutation(len(q))[:B * n]].reshape(B, n, 3), device="cuda")
        _sequence(ctx, sub, scene_d, rng, f"B{B}n{n}")
    # the scan itself against the oracle (the far queries left out: at 1 km, fp32 distances of points centimetres apart tie, and
    # the scan's FMA form and the oracle's may then round a different one lower -- the search is pinned to the scan above)
    rd, ri = _scan(ctx, q_d, scene_d)
    dist, idx = rd.cpu().numpy().reshape(-1), ri.cpu().numpy().reshape(-1).astype(np.int64)
    _nn_check(q[:384], xyz, dist[:384], idx[:384])
    # exact copies of scene points: distance 0 at the lowest index that holds the same point
    for k in range(copies.start, copies.stop):
        same = np.flatnonzero((xyz == q[k]).all(1))
        assert dist[k] == 0.0 and idx[k] == same[0], (k, dist[k], idx[k], same[:3])
