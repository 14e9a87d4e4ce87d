"""The arithmetic of fdcap_chamfer_bwd_both (include/fdcap.h), restated in numpy -- an independent specification the device
result is compared with bit for bit (tests/test_gpu_chamfer_both.py) and whose own rounding error is checked against a float64
evaluation of the same formula (tests/test_chamfer_bwd_spec_cpu.py).  Nothing here calls into the library.

    a[b,i,k] = (2 g1[b,i]) (x1[b,i,k] - x2[b,j,k]),  j = idx1[b,i]        +0 without the dist1 term
    u[b,j,k] = (2 g2[b,j]) (x2[b,j,k] - x1[b,i,k]),  i = idx2[b,j]        +0 without the dist2 term
    gxyz1[b,i,k] = a[b,i,k] - S1,   S1 = +0, then + u[b,j,k] over idx2[b,j] == i in ascending j
    gxyz2[b,j,k] = u[b,j,k] - S2,   S2 = +0, then + a[b,i,k] over idx1[b,i] == j in ascending i
    reduce2:  gxyz2[j,k] = U - A,   U = +0, then + u[b,j,k] in ascending b;  A = +0, then + a[b,i,k] over idx1[b,i] == j in
                                    ascending (b, i)

An index outside its range (-1: no neighbour) makes its term +0 and is never used as an address.  numpy arithmetic on arrays of
one dtype rounds every operation on its own (no fused multiply-add), which is the contract.

`bwd_both_loop` is the definition: a plain loop, one rounded add at a time.  `bwd_both` computes the same bits with array
operations -- the r-th term of every destination's run is added in round r, so each destination still sees its terms one at a
time in ascending order -- and is what the larger shapes use; the CPU test holds the two to each other bit for bit."""
import numpy as np


def _terms(xa, xb, g, idx, dtype):
    """(2 g[b,i]) (xa[b,i] - xb[b,idx[b,i]]) for xa [B,na,3], xb [B or 1,nb,3]; +0 where idx is outside [0, nb).  None without g."""
    if g is None:
        return None
    B, na, _ = xa.shape
    nb = xb.shape[1]
    ok = (idx >= 0) & (idx < nb)
    j = np.where(ok, idx, 0).astype(np.int64)
    bsel = np.arange(B)[:, None] if xb.shape[0] == B else np.zeros((B, 1), dtype=np.int64)      # (one shared set: batch 0)
    nbr = xb[bsel, j]                                               # [B,na,3]
    two_g = (dtype(2) * g.astype(dtype))[..., None]
    t = two_g * (xa.astype(dtype) - nbr.astype(dtype))
    return np.where(ok[..., None], t, dtype(0)).astype(dtype)


def _ordered_sum(ndest, key, t, dtype):
    """S[d] = +0, then + t[p] for every position p with key[p] == d, in ascending p (key < 0: the position contributes nothing).
    Returns S [ndest,3], sum of |t| per destination in float64, and the run lengths."""
    S = np.zeros((ndest, 3), dtype=dtype)
    mag = np.zeros((ndest, 3), dtype=np.float64)
    cnt = np.zeros(ndest, dtype=np.int64)
    pos = np.nonzero(key >= 0)[0]
    if pos.size == 0:
        return S, mag, cnt
    k = key[pos]
    order = np.argsort(k, kind="stable")
    ks, ps = k[order], pos[order]
    rank = np.arange(ks.size) - np.searchsorted(ks, ks, side="left")
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.searchsorted(rank[by_rank], np.arange(rank.max() + 2), side="left")
    for r in range(rank.max() + 1):
        sel = by_rank[bounds[r]:bounds[r + 1]]                      # at most one position per destination
        S[ks[sel]] = S[ks[sel]] + t[ps[sel]]
    np.add.at(mag, k, np.abs(t[pos].astype(np.float64)))
    cnt += np.bincount(k, minlength=ndest)
    return S, mag, cnt


def _keys(idx, ndest, per_batch):
    B, cnt = idx.shape
    ok = (idx >= 0) & (idx < ndest)
    key = idx.astype(np.int64) + (np.arange(B, dtype=np.int64)[:, None] * ndest if per_batch else 0)
    return np.where(ok, key, -1).reshape(-1)


def _as_batched(x2):
    x2 = np.asarray(x2)
    return x2[None] if x2.ndim == 2 else x2


def bwd_both(x1, x2, g1, idx1, g2, idx2, reduce2=False, dtype=np.float32, with_bound=False):
    """x1 [B,n,3]; x2 [B,m,3], or [m,3] / [1,m,3] for one shared target.  g1 / idx1 [B,n] or both None; g2 / idx2 [B,m] or both None.
    Returns (gxyz1 [B,n,3], gxyz2 [B,m,3] or, with reduce2, [m,3]) in `dtype`.  with_bound: also, per output, the pair
    (sum of the absolute values of every term that enters the component, number of terms added into its sums), in float64 /
    int64 -- what the error bound of the ordered float32 evaluation is made of."""
    x1 = np.asarray(x1)
    x2 = _as_batched(x2)
    B, n, _ = x1.shape
    m = x2.shape[1]
    assert not reduce2 or x2.shape[0] == 1
    a = _terms(x1, x2, g1, idx1, dtype)                              # [B,n,3] or None
    x2b = np.broadcast_to(x2, (B, m, 3))
    u = _terms(x2b, x1, g2, idx2, dtype)                             # [B,m,3] or None
    zero1, zero2 = np.zeros((B, n, 3), dtype=dtype), np.zeros((B, m, 3), dtype=dtype)
    # gxyz1
    if u is not None:
        S1, mag1, k1 = _ordered_sum(B * n, _keys(idx2, n, True), u.reshape(-1, 3), dtype)
    else:
        S1, mag1, k1 = zero1.reshape(-1, 3), np.zeros((B * n, 3)), np.zeros(B * n, dtype=np.int64)
    own1 = a if a is not None else zero1
    gx1 = (own1.reshape(-1, 3) - S1).reshape(B, n, 3).astype(dtype)
    b1 = (np.abs(own1.astype(np.float64)).reshape(-1, 3) + mag1).reshape(B, n, 3), k1.reshape(B, n)
    # gxyz2
    own2 = u if u is not None else zero2
    if reduce2:
        if a is not None:
            A, mag2, k2 = _ordered_sum(m, _keys(idx1, m, False), a.reshape(-1, 3), dtype)
        else:
            A, mag2, k2 = np.zeros((m, 3), dtype=dtype), np.zeros((m, 3)), np.zeros(m, dtype=np.int64)
        U = np.zeros((m, 3), dtype=dtype)
        for b in range(B):
            U = U + own2[b]
        gx2 = (U - A).astype(dtype)
        b2 = np.abs(own2.astype(np.float64)).sum(axis=0) + mag2, k2 + B
    else:
        if a is not None:
            S2, mag2, k2 = _ordered_sum(B * m, _keys(idx1, m, True), a.reshape(-1, 3), dtype)
        else:
            S2, mag2, k2 = zero2.reshape(-1, 3), np.zeros((B * m, 3)), np.zeros(B * m, dtype=np.int64)
        gx2 = (own2.reshape(-1, 3) - S2).reshape(B, m, 3).astype(dtype)
        b2 = (np.abs(own2.astype(np.float64)).reshape(-1, 3) + mag2).reshape(B, m, 3), k2.reshape(B, m)
    if with_bound:
        return gx1, gx2, b1, b2
    return gx1, gx2


def bwd_both_loop(x1, x2, g1, idx1, g2, idx2, reduce2=False):
    """The definition, in float32, one scalar operation at a time."""
    f = np.float32
    x1 = np.asarray(x1, dtype=f)
    x2 = _as_batched(np.asarray(x2, dtype=f))
    B, n, _ = x1.shape
    m = x2.shape[1]
    t2 = lambda b: x2[0] if x2.shape[0] == 1 else x2[b]
    a = np.zeros((B, n, 3), dtype=f)
    u = np.zeros((B, m, 3), dtype=f)
    for b in range(B):
        for i in range(n if g1 is not None else 0):
            j = int(idx1[b, i])
            if 0 <= j < m:
                for k in range(3):
                    a[b, i, k] = f(f(2) * f(g1[b, i])) * f(x1[b, i, k] - t2(b)[j, k])
        for j in range(m if g2 is not None else 0):
            i = int(idx2[b, j])
            if 0 <= i < n:
                for k in range(3):
                    u[b, j, k] = f(f(2) * f(g2[b, j])) * f(t2(b)[j, k] - x1[b, i, k])
    S1 = np.zeros((B, n, 3), dtype=f)
    S2 = np.zeros((B, m, 3), dtype=f)
    A = np.zeros((m, 3), dtype=f)
    U = np.zeros((m, 3), dtype=f)
    for b in range(B):
        for j in range(m if g2 is not None else 0):
            i = int(idx2[b, j])
            if 0 <= i < n:
                for k in range(3):
                    S1[b, i, k] = f(S1[b, i, k] + u[b, j, k])
        for i in range(n if g1 is not None else 0):
            j = int(idx1[b, i])
            if 0 <= j < m:
                for k in range(3):
                    S2[b, j, k] = f(S2[b, j, k] + a[b, i, k])
                    A[j, k] = f(A[j, k] + a[b, i, k])
        for j in range(m):
            for k in range(3):
                U[j, k] = f(U[j, k] + u[b, j, k])
    gx1 = (a - S1).astype(f)
    gx2 = (U - A).astype(f) if reduce2 else (u - S2).astype(f)
    return gx1, gx2


def error_bound(mag, k):
    """|float32 ordered result - exact| per component: every term is a product of a rounded difference and a weight (two roundings:
    2 ulp/2 of its magnitude), each of the k adds and the final subtract rounds a partial result that no partial sum of absolute
    values exceeds: 2^-24 (k + 3) (|own term| + sum |scattered terms|)."""
    return 2.0 ** -24 * (k[..., None] + 3) * mag


def exact_nn(q, t):
    """Lowest-index nearest neighbour of every q [nq,3] among t [nt,3], squared distance by direct differences in the points' own
    float32: sum in the order x, y, z.  Any valid index array would do as input of the specification; this is what a search gives."""
    q, t = np.asarray(q, dtype=np.float32), np.asarray(t, dtype=np.float32)
    out = np.empty(q.shape[0], dtype=np.int32)
    step = max(1, (1 << 22) // max(t.shape[0], 1))
    for s in range(0, q.shape[0], step):
        d = q[s:s + step, None, :] - t[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        out[s:s + step] = np.argmin(d2, axis=1)
    return out


def nn_indices(q, t):
    """exact_nn; beyond 2^22 pairs a k-d tree on the same points when scipy is there (float64 distances of float32 points: the
    same neighbour except among near-ties, which the specification does not care about)."""
    if q.shape[0] * t.shape[0] > (1 << 22):
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            return exact_nn(q, t)
        return cKDTree(np.asarray(t, dtype=np.float64)).query(np.asarray(q, dtype=np.float64))[1].astype(np.int32)
    return exact_nn(q, t)


def make_case(B, n, m, shared=False):
    """The inputs the tests use: uniform(-1, 1) coordinates, standard-normal weights, seed 1000 B + n + m."""
    rng = np.random.default_rng(1000 * B + n + m)
    x1 = rng.uniform(-1, 1, size=(B, n, 3)).astype(np.float32)
    x2 = rng.uniform(-1, 1, size=(1 if shared else B, m, 3)).astype(np.float32)
    g1 = rng.standard_normal((B, n)).astype(np.float32)
    g2 = rng.standard_normal((B, m)).astype(np.float32)
    return x1, x2, g1, g2
