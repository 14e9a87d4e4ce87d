"""tests/chamfer_bwd_spec.py -- the ordered float32 arithmetic fdcap_chamfer_bwd_both is held to bit for bit on the GPU -- checked
without a GPU: the array form against the plain loop that defines it (bit for bit), both against a float64 evaluation of the same
formula within the rounding bound of the ordered sums, and the three output modes against each other."""
import numpy as np
import pytest

from tests import chamfer_bwd_spec as spec

SHAPES = [(1, 1, 1), (2, 37, 5), (2, 64, 1), (4, 700, 50), (3, 300, 1500), (2, 5000, 70000)]
LOOP_SHAPES = [(1, 1, 1), (2, 37, 5), (2, 64, 1), (3, 90, 40)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _case(B, n, m, shared):
    x1, x2, g1, g2 = spec.make_case(B, n, m, shared)
    idx1 = np.stack([spec.nn_indices(x1[b], x2[0 if shared else b]) for b in range(B)])
    idx2 = np.stack([spec.nn_indices(x2[0 if shared else b], x1[b]) for b in range(B)])
    return x1, x2, g1, idx1, g2, idx2


@pytest.fixture(scope="module")
def cases():
    memo = {}

    def get(B, n, m, shared):
        if (B, n, m, shared) not in memo:
            memo[(B, n, m, shared)] = _case(B, n, m, shared)
        return memo[(B, n, m, shared)]
    return get


@pytest.mark.parametrize("B,n,m", LOOP_SHAPES)
@pytest.mark.parametrize("mode", ["per_batch", "shared", "reduce", "dist1_only", "dist2_only"])
def test_array_form_equals_the_defining_loop(cases, B, n, m, mode):
    x1, x2, g1, i1, g2, i2 = cases(B, n, m, mode in ("shared", "reduce"))
    if mode == "dist1_only":
        g2 = i2 = None
    if mode == "dist2_only":
        g1 = i1 = None
    want = spec.bwd_both_loop(x1, x2, g1, i1, g2, i2, reduce2=mode == "reduce")
    got = spec.bwd_both(x1, x2, g1, i1, g2, i2, reduce2=mode == "reduce")
    for w, g in zip(want, got):
        assert w.shape == g.shape and np.array_equal(_bits(w), _bits(g))


def test_array_form_equals_the_loop_with_indices_out_of_range(cases):
    x1, x2, g1, i1, g2, i2 = cases(2, 37, 5, False)
    i1, i2 = i1.copy(), i2.copy()
    i1[0, 3] = -1; i1[1, 7] = 5; i1[1, 8] = 1 << 30
    i2[0, 1] = -1; i2[1, 4] = 37
    want = spec.bwd_both_loop(x1, x2, g1, i1, g2, i2)
    got = spec.bwd_both(x1, x2, g1, i1, g2, i2)
    for w, g in zip(want, got):
        assert np.array_equal(_bits(w), _bits(g))
    # an entry out of range is an entry whose weight is zero, except that it leaves +0 where the product would leave -0
    z1, z2 = g1.copy(), g2.copy()
    z1[0, 3] = z1[1, 7] = z1[1, 8] = 0
    z2[0, 1] = z2[1, 4] = 0
    ref = spec.bwd_both(x1, x2, z1, np.clip(i1, 0, 4), z2, np.clip(i2, 0, 36))
    for r, g in zip(ref, got):
        assert np.array_equal(r, g)


@pytest.mark.parametrize("B,n,m", SHAPES)
@pytest.mark.parametrize("mode", ["per_batch", "shared", "reduce"])
def test_ordered_float32_stays_within_its_rounding_bound_of_float64(cases, B, n, m, mode):
    """|fp32 ordered - fp64| <= 2^-24 (k + 3) (|own term| + sum |scattered terms|) per component, k the number of terms added:
    two roundings per term, k adds, one subtract.  (Measured on these inputs: at most 0.63 of the bound.)"""
    x1, x2, g1, i1, g2, i2 = cases(B, n, m, mode != "per_batch")
    r = mode == "reduce"
    got = spec.bwd_both(x1, x2, g1, i1, g2, i2, reduce2=r)
    e1, e2, b1, b2 = spec.bwd_both(x1, x2, g1, i1, g2, i2, reduce2=r, dtype=np.float64, with_bound=True)
    worst = 0.0
    for g, e, (mag, k) in ((got[0], e1, b1), (got[1], e2, b2)):
        bound = spec.error_bound(mag, k)
        err = np.abs(g.astype(np.float64) - e)
        assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"{(B, n, m)} {mode}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("B,n,m", [(2, 37, 5), (4, 700, 50), (3, 300, 1500)])
def test_output_modes_agree_where_the_formula_says_so(cases, B, n, m):
    """One shared target: gxyz1 does not depend on how gxyz2 is laid out; the [B,m,3] rows are u[b,j] - S2[b,j], and the reduced
    row is U - A with U the ordered sum over b of u[b,j] and A the ordered sum over (b, i) of the a terms -- so with only the
    dist2 term (A = 0) the reduced output IS the ordered sum over b of the [B,m,3] rows, and with only the dist1 term (U = 0) it
    is minus the concatenation of the per-batch runs, summed in order."""
    x1, x2, g1, i1, g2, i2 = cases(B, n, m, True)
    f = np.float32
    full1, full2 = spec.bwd_both(x1, x2, g1, i1, g2, i2)
    red1, red2 = spec.bwd_both(x1, x2, g1, i1, g2, i2, reduce2=True)
    assert full2.shape == (B, m, 3) and red2.shape == (m, 3)
    assert np.array_equal(_bits(full1), _bits(red1))
    # dist2 term alone
    _, rows = spec.bwd_both(x1, x2, None, None, g2, i2)
    _, red = spec.bwd_both(x1, x2, None, None, g2, i2, reduce2=True)
    U = np.zeros((m, 3), dtype=f)
    for b in range(B):
        U = U + rows[b]
    assert np.array_equal(_bits(red), _bits(U - f(0)))
    # dist1 term alone: A over (b, i) ascending = the loop below
    _, red = spec.bwd_both(x1, x2, g1, i1, None, None, reduce2=True)
    a1, _ = spec.bwd_both(x1, x2, g1, i1, None, None)               # gxyz1 = a - 0: the a terms themselves
    A = np.zeros((m, 3), dtype=f)
    for b in range(B):
        for i in range(n):
            A[i1[b, i]] = A[i1[b, i]] + a1[b, i]
    assert np.array_equal(_bits(red), _bits(f(0) - A))
    # and everything together, in float64 where the order does not matter at this tolerance
    e1, e2 = spec.bwd_both(x1, x2, g1, i1, g2, i2, dtype=np.float64)
    _, er = spec.bwd_both(x1, x2, g1, i1, g2, i2, reduce2=True, dtype=np.float64)
    assert np.allclose(er, e2.sum(axis=0), rtol=0, atol=1e-12 * max(1.0, float(np.abs(e2).max())) * B * n)
