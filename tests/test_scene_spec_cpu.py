"""The numpy specification of the scene tables (tests/scene_spec.py) checked on its own, without a GPU: its bf16 rounding against
torch's, its cell order against the rules it states, and -- in fp64 -- that the tables it specifies are SOUND for the search that
prunes with them: every point inside its cell, quarter and super-cell box, inside its cell's radius bound, its fragments within
2^-16 of y', and the MFMA filter's score within eps / 1.5 of the true distance (the claim of fdc_chamfer.h's nn_stream4_kernel).
tests/test_gpu_scene_tables.py then pins the device build to these tables byte for byte."""
import numpy as np
import pytest
import torch

from tests import scene_spec as S


def _torch_bf16_bits(a):
    return torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def test_bf16_rounding_is_torchs():
    rng = np.random.default_rng(0)
    vals = [rng.standard_normal(20000).astype(np.float32) * np.float32(10.0) ** rng.integers(-30, 30, 20000).astype(np.float32),
            rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)]
    # exact halfway ties: dropped half == 0x8000 above an even and an odd kept mantissa, both signs, several binades
    keep = rng.integers(0, 0x7F7F, 4000).astype(np.uint32)
    keep = keep[((keep >> 7) & 0xFF) != 0xFF]
    ties = (keep << 16) | 0x8000
    vals.append(np.concatenate([ties, ties | 0x80000000, ties & np.uint32(0xFFFEFFFF), ties | np.uint32(0x10000)]).astype(np.uint32).view(np.float32))
    # subnormals (smallest, largest, ties among them), +-0, the largest finite values (round to inf) and their neighbours
    sub = np.array([1, 2, 0x7FFF, 0x8000, 0x8001, 0x18000, 0x28000, 0x7FFFFF, 0x7F8000, 0x7FFFFF - 0x8000], np.uint32)
    vals.append(np.concatenate([sub, sub | 0x80000000]).view(np.float32))
    vals.append(np.array([0.0, -0.0, 3.3895314e38, -3.3895314e38, np.finfo(np.float32).max, -np.finfo(np.float32).max,
                          np.float32(3.389e38), 1.0, -1.0, np.inf, -np.inf], np.float32))
    for v in vals:
        v = v[~np.isnan(v)]
        np.testing.assert_array_equal(S.bf16_bits(v), _torch_bf16_bits(v))
    # the tie cases really are ties that go both ways
    t = ties.view(np.float32)
    up = S.bf16_bits(t) != (ties >> 16)
    assert up.any() and (~up).any()
    assert S.bf16_bits(np.float32([-0.0]))[0] == 0x8000


# ---- the order ----------------------------------------------------------------------------------------------------------------------
def _check_order(xyz, order, nodes):
    """The rules of order_spec's docstring, checked on its output: a permutation; every cut on the longest axis (lower on a tie)
    with the stated nleft, left <= right by (coordinate with -0 == +0, index); leaves of <= 32 points in input order."""
    n = len(xyz)
    assert sorted(order.tolist()) == list(range(n))
    cuts = {a_m[:2]: a_m[2:] for a_m in nodes}
    stack = [(0, n)] if n else []
    leaves = 0
    while stack:
        a, m = stack.pop()
        seg = order[a:a + m]
        if m <= 32:
            assert (a, m) not in cuts
            assert np.all(np.diff(seg) > 0), (a, m)
            leaves += m
            continue
        ax, nleft = cuts[(a, m)]
        p = xyz[seg]
        ext = p.max(0) - p.min(0)
        assert ext[ax] == ext.max() and not np.any(ext[:ax] == ext.max()), (a, m, ext, ax)
        unit = 512 if m > 512 else 32
        assert nleft == min(m - 1, ((m + unit - 1) // unit // 2) * unit)
        key = [(float(xyz[i, ax]) + 0.0, int(i)) for i in seg]
        assert max(key[:nleft]) < min(key[nleft:]), (a, m)
        stack += [(a, nleft), (a + nleft, m - nleft)]
    assert leaves == n


def _hand_scenes():
    rng = np.random.default_rng(1)
    yield "one", np.float32([[1, 2, 3]])
    yield "tile", rng.uniform(-1, 1, (32, 3)).astype(np.float32)
    yield "y_line33", np.stack([np.zeros(33), np.arange(33.0), np.zeros(33)], 1).astype(np.float32)
    cube = np.float32([[0, 0, 0], [1, 1, 1]] * 20)                                  # all three extents equal: axis 0
    yield "equal_extents", cube
    yz = np.float32([[0, 0, 0], [0.5, 1, 1]] * 20)                                  # y and z tie above x: axis 1
    yield "yz_tie", yz
    g = np.repeat(np.float32([[0, 0, 0], [1, 0, 0]]), 50, axis=0)                  # 50 equal x then 50 equal x: a cut inside a tie run
    yield "tie_runs", g[rng.permutation(100)]
    z = np.zeros((64, 3), np.float32)
    z[:40:2, 0], z[1:40:2, 0] = 0.0, -0.0
    z[40:, 0] = -1.0
    yield "signed_zeros", z
    yield "mixed_1100", np.round(rng.uniform(-2, 2, (1100, 3)) * 4).astype(np.float32) / np.float32(4)
    yield "flat_2000", np.stack([rng.uniform(-1, 1, 2000), rng.uniform(-3, 3, 2000), np.full(2000, 0.5)], 1).astype(np.float32)


@pytest.mark.parametrize("name,xyz", list(_hand_scenes()), ids=[n for n, _ in _hand_scenes()])
def test_order_follows_its_rules(name, xyz):
    nodes = []
    order = S.order_spec(xyz, nodes)
    _check_order(xyz, order, nodes)


def test_order_on_scenes_worked_by_hand():
    # 40 points, x falling with the index: the one cut (unit 32) puts the 32 smallest x left, each tile in input order
    x = np.stack([-np.arange(40.0), np.zeros(40), np.zeros(40)], 1).astype(np.float32)
    assert S.order_spec(x).tolist() == list(range(8, 40)) + list(range(8))
    # 64 points: indices 40..63 at x = -1, the rest at +0 / -0 alternating.  -0 == +0, so the zeros go by index: the left tile
    # takes 40..63 and the zeros 0..7 (an order with -0 < +0 would take the odd ones)
    z = np.zeros((64, 3), np.float32)
    z[1:40:2, 0] = -0.0
    z[40:, 0] = -1.0
    assert S.order_spec(z).tolist() == list(range(8)) + list(range(40, 64)) + list(range(8, 40))
    # ties straddling a cut: 50 points at x = 0 and 50 at x = 1 (interleaved); the cut at 64 takes all of x = 0 and the 14 lowest
    # indices of x = 1
    g = np.zeros((100, 3), np.float32)
    g[1::2, 0] = 1.0
    o = S.order_spec(g)
    left = sorted(list(range(0, 100, 2)) + list(range(1, 28, 2)))
    assert sorted(o[:64].tolist()) == left
    # 1100 points: the first cut is at 512 (cells), not at the median
    nodes = []
    S.order_spec(np.random.default_rng(2).uniform(-1, 1, (1100, 3)).astype(np.float32), nodes)
    assert nodes[0][:2] == (0, 1100) and nodes[0][3] == 512


# ---- soundness of the specified tables ----------------------------------------------------------------------------------------------
_EDGE = list(S.edge_scenes())
_WORST = {}


def _dirs():
    d = np.concatenate([np.eye(3), -np.eye(3), np.random.default_rng(3).standard_normal((4, 3))])
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@pytest.mark.parametrize("name,xyz", _EDGE, ids=[n for n, _ in _EDGE])
def test_spec_tables_are_sound_for_the_search(name, xyz):
    t = S.scene_tables(xyz)
    ns = len(xyz)
    pos = np.arange(ns)
    ch, qd = pos // S.MF_CH, (pos % S.MF_CH) // S.QUARTER
    p = t["sorted"][:, :3].astype(np.float64)
    # boxes: every point inside its cell's, its quarter's and its super cell's box; quarters without points are (+inf, +inf)
    for lo, hi, what in ((t["bounds"][ch, 0, :3], t["bounds"][ch, 1, :3], "cell"),
                         (t["qbounds"][ch, qd, 0, :3], t["qbounds"][ch, qd, 1, :3], "quarter"),
                         (t["sbounds"][ch // S.SUPER, 0, :3], t["sbounds"][ch // S.SUPER, 1, :3], "super")):
        bad = ~((lo <= p) & (p <= hi)).all(1)
        assert not bad.any(), (what, int(np.argmax(bad)))
        assert (hi - lo > 0).all(), what                                   # the pad: never a box of extent 0
    nchunk = len(t["centers"])
    empty = (np.arange(nchunk)[:, None] * S.MF_CH + np.arange(4)[None, :] * S.QUARTER) >= ns
    assert np.all(np.isposinf(t["qbounds"][empty][:, :, :3]))
    # the radius bound and the fragments' reconstruction of y' = p - c
    c = t["centers"][ch].astype(np.float64)
    y = p - c[:, :3]
    assert (np.linalg.norm(y, axis=1) <= c[:, 3]).all()
    for cc in range(nchunk):
        H, L, _ = S.frag_parts(t["frags"], cc)
        k = min(S.MF_CH, ns - cc * S.MF_CH)
        yy = y[cc * S.MF_CH:cc * S.MF_CH + k]
        rec = (H[:k] + L[:k]) / -2.0
        assert (np.abs(rec - yy) <= 2.0 ** -16 * np.abs(yy)).all(), cc
    # the filter's error against eps / 1.5 for queries at 0, 0.5, 1, 2 and 10 cell radii from every cell's centre
    dirs = _dirs()
    worst = 0.0
    for cc in range(nchunk):
        cen, rc = t["centers"][cc, :3].astype(np.float64), float(t["centers"][cc, 3])
        q = np.concatenate([cen[None, :] + r * rc * dirs for r in (0.0, 0.5, 1.0, 2.0, 10.0)]).astype(np.float32)
        err, eps = S.filter_error(t, q, cc)
        worst = max(worst, float((err / (eps[:, None] / 1.5)).max()))
    _WORST[name] = worst
    print(f"[{name}] worst filter_error / (eps / 1.5) = {worst:.4f}  (all scenes so far: {max(_WORST.values()):.4f})")
    assert worst <= 1.0, worst
