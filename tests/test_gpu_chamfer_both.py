"""Op 1 as a two-sided operator: fdcap_chamfer_bwd_both (the whole backward, by the library, in a defined order) against the numpy
specification tests/chamfer_bwd_spec.py BIT FOR BIT; ops.chamferDist's gradients with respect to both inputs through it; and
fdcap_chamfer_fwd's batched every-pair search against the per-batch loop it replaces (FDCAP_CHAMFER_BATCHED=0), bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fdcap_amd  # noqa: F401
from fdcap_amd import capi, ops, synth
from oracle import chamfer as oracle_chamfer
from tests import chamfer_bwd_spec as spec

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 37, 5), (2, 64, 1), (4, 700, 50), (3, 300, 1500), (2, 5000, 70000)]
# ... and: long runs on the target side inside the sort (one lane sums 6667 terms), a third key byte on the target side
SHAPES += [(2, 20000, 3), (2, 17000, 40000)]
VARIANTS = ["per_batch", "shared_full", "shared_reduce", "dist1_only", "dist2_only"]
E_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(synth.make_body_model(300, seed=0), synth.make_vposer(seed=1))
    yield c
    c.close()


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _forward(ctx, x1, x2, shared, want1=True, want2=True):
    """fdcap_chamfer_fwd on device tensors x1 [B,n,3], x2 [B,m,3] or [m,3] (shared) -> d1, i1, d2, i2 (None where not wanted)."""
    B, n, _ = x1.shape
    m = x2.shape[-2]
    d1 = torch.empty(B, n, device="cuda") if want1 else None
    i1 = torch.empty(B, n, device="cuda", dtype=torch.int32) if want1 else None
    d2 = torch.empty(B, m, device="cuda") if want2 else None
    i2 = torch.empty(B, m, device="cuda", dtype=torch.int32) if want2 else None
    capi.check(ctx.lib.fdcap_chamfer_fwd(ctx.handle, capi.dptr(x1), capi.dptr(x2), B, n, m, 0 if shared else m * 3, capi.dptr(d1),
                                         capi.dptr(i1), capi.dptr(d2), capi.dptr(i2), capi.current_stream()), "fdcap_chamfer_fwd")
    torch.cuda.synchronize()
    return d1, i1, d2, i2


def _backward_rc(ctx, x1, x2, shared, g1, i1, g2, i2, out1, out2, reduce2, B=None, n=None, m=None, stride2=None):
    Bx, nx, _ = x1.shape
    mx = x2.shape[-2]
    rc = ctx.lib.fdcap_chamfer_bwd_both(ctx.handle, capi.dptr(x1), capi.dptr(x2), Bx if B is None else B, nx if n is None else n,
                                        mx if m is None else m, (0 if shared else mx * 3) if stride2 is None else stride2,
                                        capi.dptr(g1), capi.dptr(i1), capi.dptr(g2), capi.dptr(i2), capi.dptr(out1), capi.dptr(out2),
                                        1 if reduce2 else 0, capi.current_stream())
    torch.cuda.synchronize()
    return rc


def _backward(ctx, x1, x2, shared, g1, i1, g2, i2, want1=True, want2=True, reduce2=False):
    B, n, _ = x1.shape
    m = x2.shape[-2]
    # (filled with NaN: every element must be written)
    out1 = torch.full((B, n, 3), float("nan"), device="cuda") if want1 else None
    out2 = torch.full((m, 3) if reduce2 else (B, m, 3), float("nan"), device="cuda") if want2 else None
    capi.check(_backward_rc(ctx, x1, x2, shared, g1, i1, g2, i2, out1, out2, reduce2), "fdcap_chamfer_bwd_both")
    return out1, out2


@pytest.fixture(scope="module")
def cases(ctx):
    """Inputs (spec.make_case) and the library's own neighbours, once per (shape, shared)."""
    memo = {}

    def get(B, n, m, shared):
        key = (B, n, m, shared)
        if key not in memo:
            x1, x2, g1, g2 = spec.make_case(B, n, m, shared)
            _, i1, _, i2 = _forward(ctx, _dev(x1), _dev(x2[0] if shared else x2), shared)
            memo[key] = (x1, x2, g1, i1.cpu().numpy(), g2, i2.cpu().numpy())
        return memo[key]
    return get


def _forms(ctx, reset):
    buf = ctypes.create_string_buffer(4096)
    ctx.lib.fdcap_debug_kernel_forms(buf, 4096, 1 if reset else 0)
    return buf.value.decode().split(";")


# ---- 1-3: fdcap_chamfer_bwd_both against the specification ------------------------------------------------------------------
@pytest.mark.parametrize("B,n,m", SHAPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_bwd_both_equals_the_specification_bit_for_bit(ctx, cases, B, n, m, variant):
    shared = variant in ("shared_full", "shared_reduce", "dist2_only")
    reduce2 = variant in ("shared_reduce", "dist2_only")
    x1, x2, g1, i1, g2, i2 = cases(B, n, m, shared)
    if variant == "dist1_only":
        g2 = i2 = None
    if variant == "dist2_only":
        g1 = i1 = None
    want1, want2 = spec.bwd_both(x1, x2, g1, i1, g2, i2, reduce2=reduce2)
    got1, got2 = _backward(ctx, _dev(x1), _dev(x2[0] if shared else x2), shared, _dev(g1), _dev(i1), _dev(g2), _dev(i2), reduce2=reduce2)
    assert tuple(got2.shape) == want2.shape
    assert np.array_equal(_bits(got1), _bits(want1)), int((_bits(got1) != _bits(want1)).sum())
    assert np.array_equal(_bits(got2), _bits(want2)), int((_bits(got2) != _bits(want2)).sum())
    # one output at a time: the same bits
    only1, none2 = _backward(ctx, _dev(x1), _dev(x2[0] if shared else x2), shared, _dev(g1), _dev(i1), _dev(g2), _dev(i2), want2=False)
    assert none2 is None and torch.equal(only1.view(torch.int32), got1.view(torch.int32))


@pytest.mark.parametrize("shared,reduce2", [(False, False), (True, False), (True, True)])
def test_indices_out_of_range_contribute_nothing_and_are_never_addresses(ctx, cases, shared, reduce2):
    B, n, m = 3, 300, 1500
    x1, x2, g1, i1, g2, i2 = cases(B, n, m, shared)
    clean1, clean2 = _backward(ctx, _dev(x1), _dev(x2[0] if shared else x2), shared, _dev(g1), _dev(i1), _dev(g2), _dev(i2), reduce2=reduce2)
    b1, b2 = i1.copy(), i2.copy()
    rng = np.random.default_rng(5)
    p1 = rng.choice(B * n, size=40, replace=False)
    p2 = rng.choice(B * m, size=40, replace=False)
    bad1 = np.array([-1, m, m + 1, 1 << 30, -(1 << 31), (1 << 31) - 1, -2, m + 70000], dtype=np.int64)
    bad2 = np.array([-1, n, n + 1, 1 << 30, -(1 << 31), (1 << 31) - 1, -2, n + 70000], dtype=np.int64)
    b1.reshape(-1)[p1] = bad1[np.arange(40) % 8].astype(np.int32)
    b2.reshape(-1)[p2] = bad2[np.arange(40) % 8].astype(np.int32)
    want1, want2 = spec.bwd_both(x1, x2, g1, b1, g2, b2, reduce2=reduce2)
    got1, got2 = _backward(ctx, _dev(x1), _dev(x2[0] if shared else x2), shared, _dev(g1), _dev(b1), _dev(g2), _dev(b2), reduce2=reduce2)
    assert np.array_equal(_bits(got1), _bits(want1)) and np.array_equal(_bits(got2), _bits(want2))
    # every row that neither lost its own term nor one of its scattered terms is what it was without the bad entries
    touched1 = np.zeros(B * n, dtype=bool)
    touched1[p1] = True
    touched1[(p2 // m) * n + i2.reshape(-1)[p2]] = True
    same1 = _bits(got1).reshape(-1, 3)[~touched1] == _bits(clean1).reshape(-1, 3)[~touched1]
    assert same1.all() and (~touched1).sum() > B * n - 90
    if reduce2:
        touched2 = np.zeros(m, dtype=bool)
        touched2[p2 % m] = True
        touched2[i1.reshape(-1)[p1]] = True
    else:
        touched2 = np.zeros(B * m, dtype=bool)
        touched2[p2] = True
        touched2[(p1 // n) * m + i1.reshape(-1)[p1]] = True
    same2 = _bits(got2).reshape(-1, 3)[~touched2] == _bits(clean2).reshape(-1, 3)[~touched2]
    assert same2.all() and (~touched2).sum() > touched2.size - 90


@pytest.mark.parametrize("B,n,m", SHAPES)
@pytest.mark.parametrize("shared", [False, True])
def test_dist1_term_and_gxyz1_alone_is_fdcap_chamfer_bwd(ctx, cases, B, n, m, shared):
    x1, x2, g1, i1, _, _ = cases(B, n, m, shared)
    dx1, dx2, dg1, di1 = _dev(x1), _dev(x2[0] if shared else x2), _dev(g1), _dev(i1)
    old = torch.full((B, n, 3), float("nan"), device="cuda")
    capi.check(ctx.lib.fdcap_chamfer_bwd(ctx.handle, capi.dptr(dx1), capi.dptr(dx2), B, n, m, 0 if shared else m * 3, capi.dptr(dg1),
                                         capi.dptr(di1), capi.dptr(old), capi.current_stream()), "fdcap_chamfer_bwd")
    new, _ = _backward(ctx, dx1, dx2, shared, dg1, di1, None, None, want2=False)
    assert torch.equal(old.view(torch.int32), new.view(torch.int32))


# ---- 4-5: through ops.chamferDist ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["per_batch", "expanded", "one_row"])
def test_operator_gradients_of_both_inputs_through_both_halves(ctx, cases, kind):
    """Gradients of (d1 w1).sum() + (d2 w2).sum(): the specification's bits, the float64 oracle within the ordered sums' rounding
    bound 2^-24 (k + 3) (|own term| + sum |scattered terms|), and the same bits from a second backward pass of the same graph."""
    B, n, m = 3, 300, 1500
    shared = kind != "per_batch"
    x1, x2, w1, i1, w2, i2 = cases(B, n, m, shared)
    t1 = _dev(x1).requires_grad_(True)
    leaf2 = _dev(x2).requires_grad_(True)                                  # [B,m,3] or [1,m,3]
    arg2 = leaf2.expand(B, -1, -1) if kind == "expanded" else leaf2        # (expanded: the gradient autograd asks for is [B,m,3])
    op = ops.chamferDist(ctx, both=True)
    d1, d2 = op(t1, arg2)
    assert np.array_equal(op.last_idx1.cpu().numpy(), i1)
    loss = (d1 * _dev(w1)).sum() + (d2 * _dev(w2)).sum()
    first = torch.autograd.grad(loss, [t1, arg2], retain_graph=True)
    second = torch.autograd.grad(loss, [t1, arg2], retain_graph=True)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    reduce2 = kind == "one_row"
    want1, want2 = spec.bwd_both(x1, x2, w1, i1, w2, i2, reduce2=reduce2)
    g1, g2 = first
    assert tuple(g2.shape) == ((1, m, 3) if reduce2 else (B, m, 3))
    assert np.array_equal(_bits(g1), _bits(want1))
    assert np.array_equal(_bits(g2).reshape(want2.shape), _bits(want2))
    loss.backward()
    assert tuple(leaf2.grad.shape) == tuple(leaf2.shape)                    # [1,m,3] stays [1,m,3]
    assert torch.equal(t1.grad.view(torch.int32), g1.view(torch.int32))
    if kind != "expanded":
        assert torch.equal(leaf2.grad.view(torch.int32), g2.view(torch.int32))
    # the float64 oracle
    o1 = torch.tensor(x1, dtype=torch.float64, requires_grad=True)
    oleaf = torch.tensor(x2, dtype=torch.float64, requires_grad=True)
    o2 = oleaf.expand(B, -1, -1).contiguous() if shared else oleaf
    if kind == "expanded":
        o2.retain_grad()
    e1, e2 = oracle_chamfer.chamferDist()(o1, o2)
    ((e1 * torch.tensor(w1, dtype=torch.float64)).sum() + (e2 * torch.tensor(w2, dtype=torch.float64)).sum()).backward()
    og2 = (o2.grad if kind == "expanded" else oleaf.grad).numpy().reshape(want2.shape)
    _, _, (mag1, k1), (mag2, k2) = spec.bwd_both(x1, x2, w1, i1, w2, i2, reduce2=reduce2, dtype=np.float64, with_bound=True)
    err1 = np.abs(g1.cpu().numpy().astype(np.float64) - o1.grad.numpy())
    err2 = np.abs(g2.cpu().numpy().astype(np.float64).reshape(want2.shape) - og2)
    print(f"{kind}: worst error / bound: gxyz1 {float((err1 / np.maximum(spec.error_bound(mag1, k1), 1e-300)).max()):.3f}, "
          f"gxyz2 {float((err2 / np.maximum(spec.error_bound(mag2, k2), 1e-300)).max()):.3f}")
    assert np.all(err1 <= spec.error_bound(mag1, k1)) and np.all(err2 <= spec.error_bound(mag2, k2))


class _Recorder:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.startswith("fdcap_chamfer"):
            self.calls.append(name)
        return fn


def test_registered_scene_path_keeps_its_backward():
    """both=False against the registered scene, no target gradient: fdcap_chamfer_fwd_scene and fdcap_chamfer_bwd_scene, nothing
    else, and the gradient fdcap_chamfer_bwd gives bit for bit."""
    c = capi.Context(synth.make_body_model(300, seed=0), synth.make_vposer(seed=1))
    try:
        B, n, ns = 5, 120, 20000
        scene = synth.make_scene(ns, seed=9)
        c.set_scene(scene)
        s_dev = torch.tensor(scene, device="cuda")
        rng = np.random.default_rng(3)
        x = torch.tensor(scene[rng.integers(0, ns, size=(B, n))] + rng.normal(0, 0.02, size=(B, n, 3)).astype(np.float32),
                         dtype=torch.float32, device="cuda").requires_grad_(True)
        w = torch.randn(B, n, device="cuda")
        op = ops.chamferDist(c, both=False)
        real = c.lib
        c.lib = rec = _Recorder(real)
        try:
            d1, _ = op(x, s_dev.unsqueeze(0).expand(B, -1, -1))
            (d1 * w).sum().backward()
        finally:
            c.lib = real
        assert rec.calls == ["fdcap_chamfer_fwd_scene", "fdcap_chamfer_bwd_scene"]
        ref = torch.empty(B, n, 3, device="cuda")
        capi.check(c.lib.fdcap_chamfer_bwd(c.handle, capi.dptr(x.detach()), capi.dptr(s_dev), B, n, ns, 0, capi.dptr(w),
                                           capi.dptr(op.last_idx1), capi.dptr(ref), capi.current_stream()), "fdcap_chamfer_bwd")
        assert torch.equal(x.grad.view(torch.int32), ref.view(torch.int32))
        # ... and a foreign target without grad stays on fdcap_chamfer_bwd
        x2 = x.detach().clone().requires_grad_(True)
        other = s_dev.clone()
        other[7] += 0.5
        c.lib = rec = _Recorder(real)
        try:
            d1, _ = op(x2, other.unsqueeze(0).expand(B, -1, -1))
            (d1 * w).sum().backward()
        finally:
            c.lib = real
        assert rec.calls == ["fdcap_chamfer_fwd", "fdcap_chamfer_bwd"]
    finally:
        c.close()


# ---- 6: the batched forward ---------------------------------------------------------------------------------------------------
def _fwd_case(name):
    rng = np.random.default_rng(len(name) * 7919 + 13)
    if name == "ties":
        # a coarse integer grid: many exact ties in distance, duplicate points within and between the sets
        B, n, m = 3, 333, 700
        x1 = rng.integers(-3, 4, size=(B, n, 3)).astype(np.float32)
        x2 = rng.integers(-3, 4, size=(B, m, 3)).astype(np.float32)
        x2[:, 100:140] = x2[:, 0:40]
        x1[:, 10:20] = x2[:, 5:15]
        return x1, x2, False, True
    B, n, m, shared = {"3x50x700": (3, 50, 700, False), "3x700x50": (3, 700, 50, False), "2x300x9000_shared": (2, 300, 9000, True),
                       "5x1x1": (5, 1, 1, False), "2x2048x2304_mfma": (2, 2048, 2304, False),
                       "2x2304x2048_shared_mfma": (2, 2304, 2048, True), "3x600x5000": (3, 600, 5000, False)}[name]
    x1 = rng.uniform(-1, 1, size=(B, n, 3)).astype(np.float32)
    x2 = rng.uniform(-1, 1, size=(1 if shared else B, m, 3)).astype(np.float32)
    return x1, (x2[0] if shared else x2), shared, True


FWD_CASES = ["3x50x700", "3x700x50", "2x300x9000_shared", "5x1x1", "2x2048x2304_mfma", "2x2304x2048_shared_mfma", "3x600x5000", "ties"]


@pytest.mark.parametrize("name", FWD_CASES)
def test_batched_forward_equals_the_per_batch_loop_bit_for_bit(ctx, name):
    x1, x2, shared, want2 = _fwd_case(name)
    dx1, dx2 = _dev(x1), _dev(x2)
    saved = os.environ.get("FDCAP_CHAMFER_BATCHED")
    try:
        os.environ["FDCAP_CHAMFER_BATCHED"] = "0"
        _forms(ctx, True)
        loop = _forward(ctx, dx1, dx2, shared, True, want2)
        forms_loop = _forms(ctx, True)
        os.environ.pop("FDCAP_CHAMFER_BATCHED")
        batched = _forward(ctx, dx1, dx2, shared, True, want2)
        forms_batched = _forms(ctx, True)
        only2 = _forward(ctx, dx1, dx2, shared, False, True)
    finally:
        if saved is None:
            os.environ.pop("FDCAP_CHAMFER_BATCHED", None)
        else:
            os.environ["FDCAP_CHAMFER_BATCHED"] = saved
    for a, b in zip(loop, batched):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(only2[2].view(torch.int32), loop[2].view(torch.int32)) and torch.equal(only2[3], loop[3])
    assert not [f for f in forms_loop if f.endswith("_batched")], forms_loop
    n, m = x1.shape[1], x2.shape[-2]
    want = "nn_mfma_batched" if n * m >= (1 << 22) else "nn_direct_batched"
    assert want in forms_batched, forms_batched
    # the lowest index among ties, as an ascending strict-< scan gives it (fp32, the search's own distance)
    if name in ("ties", "5x1x1"):
        for b in range(x1.shape[0]):
            t = x2 if shared else x2[b]
            d = ((x1[b][:, None, :] - t[None, :, :]) ** 2).sum(-1)
            assert np.array_equal(batched[1][b].cpu().numpy(), np.argmin(d, axis=1))
            assert np.array_equal(batched[3][b].cpu().numpy(), np.argmin(d, axis=0))


def test_batched_forward_beyond_one_grid_of_batches(ctx):
    """More than 65 535 batches: the batch axis takes a second launch.  Small-integer coordinates, so every squared distance is
    exact and numpy's first minimum is the lowest index among ties."""
    B, n, m = 65535 + 3, 2, 3
    rng = np.random.default_rng(B)
    x1 = rng.integers(-4, 5, size=(B, n, 3)).astype(np.float32)
    x2 = rng.integers(-4, 5, size=(B, m, 3)).astype(np.float32)
    d = ((x1[:, :, None, :] - x2[:, None, :, :]) ** 2).sum(-1)             # [B,n,m]
    _forms(ctx, True)
    d1, i1, d2, i2 = _forward(ctx, _dev(x1), _dev(x2), False)
    assert "nn_direct_batched" in _forms(ctx, True)
    assert np.array_equal(i1.cpu().numpy(), d.argmin(axis=2)) and np.array_equal(d1.cpu().numpy(), d.min(axis=2))
    assert np.array_equal(i2.cpu().numpy(), d.argmin(axis=1)) and np.array_equal(d2.cpu().numpy(), d.min(axis=1))
    # ... and its whole backward in the same breath: O(1) launches for 65 538 batches
    g1, g2 = rng.standard_normal((B, n)).astype(np.float32), rng.standard_normal((B, m)).astype(np.float32)
    want1, want2 = spec.bwd_both(x1, x2, g1, i1.cpu().numpy(), g2, i2.cpu().numpy())
    got1, got2 = _backward(ctx, _dev(x1), _dev(x2), False, _dev(g1), i1, _dev(g2), i2)
    assert np.array_equal(_bits(got1), _bits(want1)) and np.array_equal(_bits(got2), _bits(want2))


# ---- 7: refusals ----------------------------------------------------------------------------------------------------------------
def test_bwd_both_refuses_what_the_header_says_it_refuses(ctx):
    B, n, m = 2, 7, 5
    x1, x2 = torch.zeros(B, n, 3, device="cuda"), torch.zeros(B, m, 3, device="cuda")
    g1, g2 = torch.zeros(B, n, device="cuda"), torch.zeros(B, m, device="cuda")
    i1, i2 = torch.zeros(B, n, device="cuda", dtype=torch.int32), torch.zeros(B, m, device="cuda", dtype=torch.int32)
    o1, o2 = torch.empty(B, n, 3, device="cuda"), torch.empty(B, m, 3, device="cuda")
    lib, st = ctx.lib, capi.current_stream()
    p = capi.dptr

    def call(h=ctx.handle, a=x1, b=x2, B_=B, n_=n, m_=m, s2=m * 3, G1=g1, I1=i1, G2=g2, I2=i2, O1=o1, O2=o2, red=0):
        return lib.fdcap_chamfer_bwd_both(h, p(a), p(b), B_, n_, m_, s2, p(G1), p(I1), p(G2), p(I2), p(O1), p(O2), red, st)

    assert call() == 0
    assert call(h=None) == E_ARG and call(a=None) == E_ARG and call(b=None) == E_ARG
    for kw in ({"B_": 0}, {"n_": 0}, {"m_": 0}, {"B_": -1}, {"n_": -3}, {"m_": -3}):
        assert call(**kw) == E_ARG, kw
    assert call(I1=None) == E_ARG and call(G1=None) == E_ARG and call(I2=None) == E_ARG and call(G2=None) == E_ARG
    assert call(G1=None, I1=None, G2=None, I2=None) == E_ARG             # no term at all
    assert call(O1=None, O2=None) == E_ARG                               # no output at all
    assert call(red=1) == E_ARG                                          # reduce2 with per-batch targets
    assert call(s2=0, red=1) == 0 and call(s2=0) == 0
    big = 1 << 30                                                        # B * n = B * m = 2^31 > 2^31 - 1 (refused before anything is read)
    assert call(B_=2, n_=big) == E_ARG and call(B_=2, m_=big) == E_ARG and call(B_=1 << 16, n_=1 << 15) == E_ARG
    assert call(G2=None, I2=None) == 0 and call(G1=None, I1=None) == 0 and call(O1=None) == 0 and call(O2=None) == 0
    torch.cuda.synchronize()
