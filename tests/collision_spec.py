"""The self-interpenetration term as a twin (csrc/fdc_collide.h states the same in words): the collision set by testing every pair
(numpy, fp64 or fp32), the penalty with torch autograd (fp64 or fp32), the face order of the registered tree.  Not a test itself:
tests/test_collision_cpu.py, tests/test_gpu_collision.py and tests/test_gpu_collision_edges.py check the header and the kernels against it.

Parity with SMPLify-X / torch-mesh-isect is UNPINNED (neither is available): the specification is restated from Tzionas et al.
(IJCV 2016) and this file is the checker."""
import functools
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "4dcapture-fpv_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
EPS32 = 2.0 ** -24
DEGENERATE = 1e-30


def host_exe():
    """tests/collision_cpu/coll_check.cpp, the header through plain g++ with contraction off"""
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, "coll_check")
    src = os.path.join(ROOT, "tests", "collision_cpu", "coll_check.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("fdc_collide.h", "fdc_math.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC, "-o", out, src])
    return out


def run_host(mode, words, tmp_path):
    """words: a list of numpy arrays of 32-bit items, written one after the other -> the program's output lines"""
    fn = os.path.join(str(tmp_path), f"{mode}.bin")
    with open(fn, "wb") as f:
        for a in words:
            a = np.ascontiguousarray(a)
            assert a.dtype.itemsize == 4 or a.dtype == np.uint64, a.dtype
            f.write(a.tobytes())
    return subprocess.run([host_exe(), mode, fn], check=True, capture_output=True, text=True).stdout.splitlines()


def host_pairs(verts, faces, face_part, ignore, tmp_path):
    """every pair of faces of one frame through the header's coll_pair_test -> set of (i, j), i < j by face id"""
    V, F = verts.shape[0], faces.shape[0]
    part = np.zeros(F, np.int32) if face_part is None else np.asarray(face_part, np.int32)
    ign = np.zeros(64, np.uint64) if ignore is None else np.asarray(ignore, np.uint64)
    head = np.array([V, F, 0 if face_part is None else 1, 0 if ignore is None else 1], np.int32)
    lines = run_host("pairs", [head, verts.astype(np.float32), faces.astype(np.int32), part, ign], tmp_path)
    return {tuple(int(t) for t in ln.split()) for ln in lines}


def _sweep_candidates(lo, hi, ids, axis, strict, chunk=1 << 22):
    """the usable faces `ids` sorted by lo[axis]; face a's candidates are the faces b behind it in that order with lo_b <= hi_a
    (strict: <, the mutant of tests/test_collision_cpu.py) -- lo_a <= lo_b <= hi_b gives the other half of the overlap on this axis --
    -> yields (a, b) arrays of face ids whose boxes overlap on all three axes"""
    o = ids[np.argsort(lo[ids, axis], kind="stable")]
    lox, hix = lo[o, axis], hi[o, axis]
    end = np.searchsorted(lox, hix, side="left" if strict else "right")           # the first position whose lo is > (strict: >=) hi_a
    cnt = np.maximum(end - (np.arange(len(o)) + 1), 0)
    other = [k for k in range(3) if k != axis]
    a0 = 0
    while a0 < len(o):
        a1 = a0 + max(1, int(np.searchsorted(np.cumsum(cnt[a0:]), chunk, side="right")))
        c = cnt[a0:a1]
        ia = np.repeat(np.arange(a0, a1), c)
        ib = np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c) + ia + 1
        fa, fb = o[ia], o[ib]
        for k in other:
            keep = (lo[fa, k] <= hi[fb, k]) & (lo[fb, k] <= hi[fa, k])
            fa, fb = fa[keep], fb[keep]
        yield fa, fb
        a0 = a1


def sweep_pairs(verts, faces, face_part, ignore, tmp_path, strict=False):
    """host_pairs' set without testing every pair (that takes 15 s at 16 512 faces and 52 s at 32 896): the predicate's steps in the header's
    order, the cheap ones here and the 17 axes by the header itself.  (0) face_ok in fp32; (1) per-face fp32 boxes (min, max and <=
    are exact, so numpy and the header cannot differ) and a sort-and-sweep along the axis that leaves the fewest candidates, the other
    two axes compared directly; (2) shared vertex index; (3) the part matrix, either way round; (4) `coll_check sat` on what is left.
    -> set of (i, j), i < j by face id.  strict: the sweep axis's overlap test made strict -- wrong, for the test that shows the sweep
    is looked at."""
    v = np.asarray(verts, np.float32)
    faces = np.asarray(faces)
    F = faces.shape[0]
    P = v[faces]
    with np.errstate(all="ignore"):
        ids = np.nonzero(face_ok(P))[0]
        lo, hi = P.min(1), P.max(1)
    if len(ids) < 2:
        return set()

    def n_candidates(axis):
        l = np.sort(lo[ids, axis])
        return int(np.searchsorted(l, hi[ids, axis], side="right").sum())
    axis = min(range(3), key=n_candidates)
    part = np.zeros(F, np.int64) if face_part is None else np.asarray(face_part, np.int64)
    ign = None if ignore is None else np.asarray(ignore, np.uint64)
    bit = lambda a, b: (ign[a] >> b.astype(np.uint64)) & np.uint64(1)
    A, B = [], []
    for fa, fb in _sweep_candidates(lo, hi, ids, axis, strict):
        keep = ~(faces[fa][:, :, None] == faces[fb][:, None, :]).any((1, 2))
        if ign is not None:
            keep &= (bit(part[fa], part[fb]) | bit(part[fb], part[fa])) == 0
        A.append(fa[keep]); B.append(fb[keep])
    A, B = np.concatenate(A), np.concatenate(B)
    if len(A) == 0:
        return set()
    got = np.array([int(l) for l in run_host("sat", [np.array([len(A)], np.int32), np.concatenate([P[A], P[B]], 1)], tmp_path)])
    assert not (got == 2).any(), "face_ok here and coll_face_ok in the header disagree"
    i, j = np.minimum(A, B)[got == 1], np.maximum(A, B)[got == 1]
    return {(int(a), int(b)) for a, b in zip(i, j)}


# ---- the collision set ---------------------------------------------------------------------------------------------------------------
def _axes(S, T):
    """S, T [N,3,3] -> axes [N,17,3] and the product of the lengths of the vectors each is a cross product of [N,17]"""
    es = np.stack([S[:, (i + 1) % 3] - S[:, i] for i in range(3)], 1)
    et = np.stack([T[:, (i + 1) % 3] - T[:, i] for i in range(3)], 1)
    ns = np.cross(es[:, 0], S[:, 2] - S[:, 0])
    nt = np.cross(et[:, 0], T[:, 2] - T[:, 0])
    ln = lambda v: np.linalg.norm(v, axis=-1)
    ax, sc = [ns, nt], [ln(es[:, 0]) * ln(S[:, 2] - S[:, 0]), ln(et[:, 0]) * ln(T[:, 2] - T[:, 0])]
    for i in range(3):
        for j in range(3):
            ax.append(np.cross(es[:, i], et[:, j])); sc.append(ln(es[:, i]) * ln(et[:, j]))
    for i in range(3):
        ax.append(np.cross(ns, es[:, i])); sc.append(sc[0] * ln(es[:, i]))
    for i in range(3):
        ax.append(np.cross(nt, et[:, i])); sc.append(sc[1] * ln(et[:, i]))
    return np.stack(ax, 1), np.stack(sc, 1), np.maximum(ln(es).max(1), ln(et).max(1))


def sat(S, T, in_plane=True):
    """S, T [N,3,3] in the dtype to compute in -> hit [N] (no separating axis among the 17; in_plane=False: among the first 11),
    gap [N,17] (> 0: separated by that much on the axis, <= 0: minus the overlap; in units of |a| x the longer edge), kappa [N,17]
    (conditioning of the axis: lengths' product / |a|; inf for a zero axis, which never separates)"""
    ax, sc, L = _axes(S, T)
    qs, qt = S - S[:, :1], T - S[:, :1]
    ps, pt = np.einsum("nak,nck->nac", ax, qs), np.einsum("nak,nck->nac", ax, qt)
    gap = np.maximum(pt.min(-1) - ps.max(-1), ps.min(-1) - pt.max(-1))
    an = np.linalg.norm(ax, axis=-1)
    zero = an == 0
    use = np.ones(17, bool)
    if not in_plane:
        use[11:] = False
    hit = ~((gap > 0) & use[None]).any(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(zero, np.inf, sc / an)
        g = np.where(zero, -np.inf, gap / (an * L[:, None]))
    return hit, g, kappa


def face_ok(P):
    """P [N,3,3] -> usable [N]"""
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        return np.isfinite(P).all((1, 2)) & ((w * w).sum(-1) > DEGENERATE)


def collision_set(verts, faces, face_part=None, ignore=None, dtype=np.float64, in_plane=True, with_margins=False):
    """One frame.  verts [V,3], faces [F,3] -> set of (i, j), i < j by face id (with_margins: also {pair: (gap [17], kappa [17])} of every
    candidate pair that reached the axis test)"""
    verts = np.asarray(verts, dtype=dtype)
    F = faces.shape[0]
    P = verts[faces]
    ok = face_ok(P)
    with np.errstate(invalid="ignore"):
        lo, hi = P.min(1), P.max(1)
        i, j = np.triu_indices(F, 1)
        keep = ok[i] & ok[j] & (lo[i] <= hi[j]).all(1) & (lo[j] <= hi[i]).all(1)
    i, j = i[keep], j[keep]
    share = (faces[i][:, :, None] == faces[j][:, None, :]).any((1, 2))
    keep = ~share
    if ignore is not None:
        part = np.zeros(F, np.int64) if face_part is None else np.asarray(face_part, np.int64)
        bit = lambda a, b: (np.asarray(ignore, np.uint64)[a] >> b.astype(np.uint64)) & np.uint64(1)
        keep &= (bit(part[i], part[j]) | bit(part[j], part[i])) == 0
    i, j = i[keep], j[keep]
    if len(i) == 0:
        return (set(), {}) if with_margins else set()
    hit, g, kappa = sat(P[i], P[j], in_plane)
    pairs = {(int(a), int(b)) for a, b in zip(i[hit], j[hit])}
    if with_margins:
        return pairs, {(int(a), int(b)): (g[k], kappa[k]) for k, (a, b) in enumerate(zip(i, j))}
    return pairs


def tau(kappa):
    """The fp32 error of the header's comparison on one axis, in units of |a| x the longer edge L.  The header takes the corners
    relative to s0 (q = p - s0, one rounding: |dq| <= eps |q|), edges from the corners (|de| <= eps |e|) and an axis as a cross product,
    each component x y - z w with three roundings on top of its factors' own: |da| <= 7 eps |e| |e'| (twice that for n x e, whose n is
    itself such a product) = 14 eps kappa |a| at most.  A projection a . q then carries 3 eps |a| |q| of its own two adds and three
    products, eps |a| |q| from q and |da| |q| from the axis: (4 + 14 kappa) eps |a| |q|, and a comparison has two of them.  |q| <= D, the
    pair's diameter, and D <= 2 sqrt(3) L < 3.5 L for a pair whose boxes overlap (others never reach the axis test).  So
        tau = 3.5 (8 + 28 kappa) 2^-24."""
    return 3.5 * (8.0 + 28.0 * kappa) * EPS32


def marginal(hit, gap, kappa):
    """A hit is marginal when some non-zero axis overlaps by less than its tau; a miss when no axis separates by at least its tau."""
    t = tau(kappa)
    if hit:
        return bool(((-gap < t) & np.isfinite(kappa)).any())
    return not bool((gap >= t).any())


# ---- the penalty ------------------------------------------------------------------------------------------------------------------------
def _field(a, b, c):
    u, v = b - a, c - a
    w = torch.cross(u, v, dim=-1)
    w2 = (w * w).sum(-1, keepdim=True)
    m = (u * u).sum(-1, keepdim=True) * v - (v * v).sum(-1, keepdim=True) * u
    orel = torch.cross(m, w, dim=-1) / (2.0 * w2)
    return w / torch.sqrt(w2), a + orel, torch.sqrt((orel * orel).sum(-1))


def _psi2(n, o, r, p, sigma):
    d = p - o
    h = (n * d).sum(-1)
    rho = r - (r / sigma) * h
    t = d - h[..., None] * n
    t2 = (t * t).sum(-1)
    pos = t2 > 0
    tn = torch.where(pos, torch.sqrt(torch.where(pos, t2, torch.ones_like(t2))), torch.zeros_like(t2))
    phi = tn / torch.where(rho > 0, rho, torch.ones_like(rho))
    quad = -(1.0 - 2.0 * sigma) / (4.0 * sigma * sigma) * h * h - h / (2.0 * sigma) + (3.0 - 2.0 * sigma) / 4.0
    ups = torch.where(h <= -sigma, -h + 1.0 - sigma, quad)
    psi = (1.0 - phi) * ups
    return torch.where((h < sigma) & (rho > 0) & (phi < 1), psi * psi, torch.zeros_like(psi))


def pair_values(P, sigma, detach_receiver=False):
    """P [N,6,3] (s0 s1 s2 t0 t1 t2) -> e [N]"""
    e = 0.0
    for recv in (0, 1):
        R, O = P[:, 3 * recv:3 * recv + 3], P[:, 3 * (1 - recv):3 * (1 - recv) + 3]
        n, o, r = _field(R[:, 0], R[:, 1], R[:, 2])
        if detach_receiver:
            n, o, r = n.detach(), o.detach(), r.detach()
        e = e + sum(_psi2(n, o, r, O[:, k], sigma) for k in range(3))
    return e


TAG_ABOVE, TAG_RHO, TAG_OUTSIDE, TAG_DEEP, TAG_QUAD = range(5)
TAG_NAMES = ("h >= sigma", "rho <= 0", "phi >= 1", "deep (h <= -sigma)", "quadratic")


def psi_tags(P, sigma, dtype=torch.float64):
    """P [N,6,3] (s0 s1 s2 t0 t1 t2), computed in `dtype` with _psi2's expressions -> tags [N,2,3] (pair, receiver: 0 = the first face,
    intruder corner): which return of the header's coll_psi2 is taken, in its order -- TAG_ABOVE (h >= sigma: zero), TAG_RHO (rho <= 0:
    zero), TAG_OUTSIDE (phi >= 1: zero), TAG_DEEP (Y's linear branch), TAG_QUAD (Y's quadratic branch).
    TAG_RHO cannot be reached: rho = r (1 - h / sigma), and behind the first return h < sigma, while r > 0 for a usable face; only a
    rounding of (r / sigma) h up to r itself, h within an ulp of sigma, could give it.  No case is asked to hit it."""
    P = torch.as_tensor(np.asarray(P), dtype=dtype)
    out = np.zeros((P.shape[0], 2, 3), np.int64)
    for recv in (0, 1):
        R, O = P[:, 3 * recv:3 * recv + 3], P[:, 3 * (1 - recv):3 * (1 - recv) + 3]
        n, o, r = _field(R[:, 0], R[:, 1], R[:, 2])
        for k in range(3):
            d = O[:, k] - o
            h = (n * d).sum(-1)
            rho = r - (r / sigma) * h
            t = d - h[..., None] * n
            t2 = (t * t).sum(-1)
            pos = t2 > 0
            tn = torch.where(pos, torch.sqrt(torch.where(pos, t2, torch.ones_like(t2))), torch.zeros_like(t2))
            phi = tn / torch.where(rho > 0, rho, torch.ones_like(rho))
            tag = torch.where(h <= -sigma, TAG_DEEP, TAG_QUAD)
            tag = torch.where(~(phi < 1), TAG_OUTSIDE, tag)
            tag = torch.where(~(rho > 0), TAG_RHO, tag)
            tag = torch.where(~(h < sigma), TAG_ABOVE, tag)
            out[:, recv, k] = tag.numpy()
    return out


def penalty(verts, faces, pairs, sigma, w_coll, detach_receiver=False):
    """verts [n,V,3] torch (its dtype is the precision), pairs: per frame a list of (owner face, other face) -> E [n]"""
    faces = torch.as_tensor(np.asarray(faces), dtype=torch.long)
    out = []
    for f in range(verts.shape[0]):
        pr = torch.as_tensor(np.asarray(pairs[f], dtype=np.int64).reshape(-1, 2))
        if pr.shape[0] == 0:
            out.append(verts[f].sum() * 0.0)
            continue
        P = torch.cat([verts[f][faces[pr[:, 0]]], verts[f][faces[pr[:, 1]]]], 1)
        out.append(w_coll * pair_values(P, sigma, detach_receiver).sum())
    return torch.stack(out)


# ---- the tree ---------------------------------------------------------------------------------------------------------------------------
def pick_leaf(F, want=32):
    leaf = 64 if want == 64 else 32
    return 64 if -(-F // leaf) > 1024 else leaf


def face_order(v_template, faces, leaf_want=32):
    """-> leaf, NL, NLp, order [NL * leaf] (tree position -> face id, -1 padding), by the specification in csrc/fdc_collide.h"""
    vt = np.asarray(v_template, np.float32)
    F = faces.shape[0]
    leaf = pick_leaf(F, leaf_want)
    NL = -(-F // leaf)
    NLp = 1
    while NLp < NL:
        NLp *= 2
    c = (vt[faces[:, 0]] + vt[faces[:, 1]]) + vt[faces[:, 2]]              # fp32, in this order

    def split(ids, w):
        if w == 1 or len(ids) == 0:
            return sorted(ids)
        nleft = min(len(ids), (w // 2) * leaf)
        if nleft == len(ids):
            return split(ids, w // 2)
        cc = c[ids]
        ext = cc.max(0) - cc.min(0)
        axis = int(np.argmax(ext))                                          # (the first of equal extents)
        ids = sorted(ids, key=lambda f: (c[f, axis], f))
        return split(ids[:nleft], w // 2) + split(ids[nleft:], w // 2)

    order = np.full(NL * leaf, -1, np.int32)
    order[:F] = split(list(range(F)), NLp)
    return leaf, NL, NLp, order


def node_boxes(verts_frame, faces, order, leaf, NL, NLp):
    """The refit's specification, numpy fp32 (min and max are exact): -> [2 NLp, 6] {lo, hi} in heap numbering (root 1, children 2 i and
    2 i + 1, leaf l = node NLp + l).  A leaf's box is the min / max over the corners of its usable faces (face_ok), an upper node's the
    min / max of its children's, an empty node's (+inf, -inf).  Node 0 is unspecified (here: empty)."""
    v = np.asarray(verts_frame, np.float32)
    order = np.asarray(order)
    assert order.shape == (NL * leaf,) and NLp >= NL
    box = np.empty((2 * NLp, 6), np.float32)
    box[:, :3], box[:, 3:] = np.inf, -np.inf
    with np.errstate(all="ignore"):
        for l in range(NL):
            ids = order[l * leaf:(l + 1) * leaf]
            P = v[np.asarray(faces)[ids[ids >= 0]]]
            P = P[face_ok(P)]
            if len(P):
                box[NLp + l, :3], box[NLp + l, 3:] = P.min((0, 1)), P.max((0, 1))
    for i in range(NLp - 1, 0, -1):
        box[i, :3] = np.minimum(box[2 * i, :3], box[2 * i + 1, :3])
        box[i, 3:] = np.maximum(box[2 * i, 3:], box[2 * i + 1, 3:])
    return box


# ---- meshes the tests share ----------------------------------------------------------------------------------------------------------------
def tube(center0, center1, radius, rings, around, phase=0.0):
    """an open tube from center0 to center1 -> verts [rings * around, 3] float32, faces [2 (rings - 1) around, 3]"""
    a, b = np.asarray(center0, float), np.asarray(center1, float)
    d = (b - a) / np.linalg.norm(b - a)
    e1 = np.cross(d, [0.0, 0.0, 1.0])
    if np.linalg.norm(e1) < 1e-6:
        e1 = np.cross(d, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(d, e1)
    t = np.linspace(0, 1, rings)[:, None, None]
    ang = phase + np.arange(around) * 2 * np.pi / around
    v = a + t * (b - a) + radius * (np.cos(ang)[None, :, None] * e1 + np.sin(ang)[None, :, None] * e2)
    r, k = np.meshgrid(np.arange(rings - 1), np.arange(around), indexing="ij")
    v00, v01 = r * around + k, r * around + (k + 1) % around
    f = np.concatenate([np.stack([v00, v01, v01 + around], -1).reshape(-1, 3), np.stack([v00, v01 + around, v00 + around], -1).reshape(-1, 3)])
    return v.reshape(-1, 3).astype(np.float32), f.astype(np.int32)


def flat_grid(nx, ny, h=0.1):
    """a flat nx x ny grid of squares cut into triangles, in the plane z = 0.25 -> verts, faces"""
    x, y = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    v = np.stack([x * h, y * h, np.full(x.shape, 0.25)], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    v00 = i * (ny + 1) + j
    f = np.concatenate([np.stack([v00, v00 + ny + 1, v00 + ny + 2], -1).reshape(-1, 3), np.stack([v00, v00 + ny + 2, v00 + 1], -1).reshape(-1, 3)])
    return v, f.astype(np.int32)


def frames_of(verts, faces, n, moving):
    """n frames that differ: the vertices `moving` shifted a little more in every frame"""
    out = np.repeat(verts[None], n, 0).copy()
    for f in range(n):
        out[f, moving] += np.array([0.004, -0.003, 0.002], np.float32) * f
    return out


def crossing_tubes(rings=7, around=8, r=0.05):
    va, fa = tube((-0.3, 0.0, 3.0), (0.3, 0.0, 3.0), r, rings, around)
    vb, fb = tube((0.02, -0.3, 3.01), (0.0, 0.3, 3.03), r, rings, around, phase=0.2)
    return np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)]), np.arange(len(va), len(va) + len(vb))


def bent_tube():
    """a straight tube (the template) folded into a hairpin whose legs run through each other: faces far apart in tree order collide"""
    rings, around, r = 41, 8, 0.04
    vt, f = tube((0.0, 0.0, 3.0), (1.6, 0.0, 3.0), r, rings, around)
    s = vt[:, 0].astype(np.float64)                                            # arc length along the axis
    half = 0.8
    off = vt.astype(np.float64) - np.stack([s, np.zeros_like(s), np.full_like(s, 3.0)], 1)
    back = s > half
    x = np.where(back, 2 * half - s, s)                                         # out, then back
    y = np.where(back, 0.05 + 0.0 * s, 0.0)                                     # the return leg 0.05 beside the first: closer than 2 r
    off[back, 0] *= -1
    v = np.stack([x, y, np.full_like(s, 3.0)], 1) + off
    v[:, 2] += 0.01 * np.sin(9 * s)                                             # no two legs exactly parallel
    return vt, f, v.astype(np.float32)


MESHES = ("tubes", "tubes64", "bent", "grid", "two_leaves_5", "one_leaf", "random")


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    """-> template [V,3], faces, frame vertices [V,3], indices that move from frame to frame"""
    if name in ("tubes", "tubes64"):
        v, f, mv = crossing_tubes()
        assert len(f) == 2 * 96
        return v, f, v, mv
    if name == "bent":
        vt, f, v = bent_tube()
        return vt, f, v, np.arange(len(v) // 2, len(v))
    if name == "grid":
        v, f = flat_grid(6, 5)
        return v, f, v, np.arange(10)
    if name == "two_leaves_5":                                                  # F = 2 x 32 + 5
        v, f, mv = crossing_tubes(rings=4, around=6)
        f = np.concatenate([f[:36], f[36:69]])
        assert len(f) == 69
        return v, f, v, mv
    if name == "one_leaf":
        v, f, mv = crossing_tubes(rings=2, around=4, r=0.08)
        assert len(f) == 16
        return v, f, v, mv
    if name == "random":                                                        # vertices unrelated to the template the tree was built on
        vt, f, _ = crossing_tubes()
        rng = np.random.Generator(np.random.PCG64(8))
        v = (rng.standard_normal(vt.shape) * 0.08 + np.array([0.0, 0.0, 3.0])).astype(np.float32)
        return vt, f, v, np.arange(0, len(v), 3)
    raise KeyError(name)


def long_tubes(rings, around=32, r=0.08):
    """two tubes of 2 (rings - 1) around faces each that cross at right angles, both diagonal in x, y: no coordinate axis along which
    one of them is a single heap of overlapping boxes (sweep_pairs, and the tree's boxes, see both spread out) -> verts, faces,
    the second tube's vertices"""
    va, fa = tube((-0.35, -0.35, 3.0), (0.35, 0.35, 3.0), r, rings, around)
    vb, fb = tube((-0.33, 0.36, 3.02), (0.37, -0.34, 3.05), r, rings, around, phase=0.1)
    return np.concatenate([va, vb]), np.concatenate([fa, fb + len(va)]), np.arange(len(va), len(va) + len(vb))


# ---- the inner fit with the term ---------------------------------------------------------------------------------------------------------
def fit_spec(bm, vp, kmap, faces, face_part=None, ignore=None, dtype=torch.float64, **kw):
    """-> a tests/face_spec.FaceSpec that also knows the term: world vertices (camera frame + camera_translation: the inner fit's scale
    is 1 and its camera the identity), the collision set of every frame by testing every pair in this twin's precision, the penalty on it"""
    from oracle import rotrepr
    from oracle.fitting import body_params_encapsulate_batch
    from tests.face_spec import FaceSpec

    class CollisionFitSpec(FaceSpec):
        def world_vertices(self, x78):
            n = x78.shape[0]
            p = body_params_encapsulate_batch(rotrepr.convert_to_3D_rot(x78))
            joint_rot = self.vposer.decode(p["body_pose_vp"], output_type="aa").view(n, -1)
            out = self.body_mesh_model(return_verts=True, body_pose=joint_rot, transl=p["transl"], global_orient=p["global_orient"],
                                       betas=p["betas"], left_hand_pose=p["left_hand_pose"], right_hand_pose=p["right_hand_pose"])
            return out.vertices + x78[:, 75:78].unsqueeze(1)

        def pair_sets(self, verts):
            np_dtype = np.float64 if self.dtype == torch.float64 else np.float32
            return [sorted(collision_set(verts[f].detach().numpy(), faces, face_part, ignore, dtype=np_dtype)) for f in range(verts.shape[0])]

        def collision(self, x78, sigma, w_coll, pairs=None):
            """[n]; leaves the pair sets used in self.last_pairs"""
            verts = self.world_vertices(x78)
            self.last_pairs = self.pair_sets(verts) if pairs is None else pairs
            return penalty(verts, faces, self.last_pairs, sigma, w_coll)

        def grads_coll(self, x_np, kp_np, stage, sigma, w_coll, w_bend=0.0, pairs=None):
            """-> sums [data, prior, collision], per-frame objective [n], d rows [n, 78]"""
            x = torch.tensor(np.asarray(x_np), dtype=self.dtype, requires_grad=True)
            kp = torch.tensor(np.asarray(kp_np), dtype=self.dtype)
            base = self.frame_loss(x, kp, stage, w_bend=w_bend)
            data, prior = self.loss(x, kp, stage, None, None, w_bend)
            e = self.collision(x, sigma, w_coll, pairs)
            (base + e).sum().backward()
            return (np.array([float(data.detach()), float(prior.detach()), float(e.sum().detach())]), (base + e).detach().numpy().astype(np.float64),
                    x.grad.numpy().astype(np.float64))

        def fit_coll(self, rows75, keypoints, stages, iters, sigma, weights, capacity=None):
            """five-stage Adam as InnerFitOracle.fitting with the term at weights[stage] -> rows75 [n, 75]; self.visited: the pair sets
            of every step"""
            x = rotrepr.convert_to_6D_rot(torch.as_tensor(rows75).to(self.dtype)).detach().clone().requires_grad_(True)
            kp = torch.as_tensor(keypoints).to(self.dtype)
            self.visited = []
            for si, stage in enumerate(stages):
                opt = torch.optim.Adam([x], lr=self.lr)
                for _ in range(iters):
                    opt.zero_grad()
                    data, prior = self.loss(x, kp, stage)
                    total = data + prior
                    if weights[si] > 0:
                        total = total + self.collision(x, sigma, weights[si]).sum()
                        self.visited.append(self.last_pairs)
                    total.backward()
                    opt.step()
            self.x78 = x.detach()
            return rotrepr.convert_to_3D_rot(x).detach()

    return CollisionFitSpec(bm, vp, kmap.joint, kmap.tri, kmap.bary, dtype=dtype, **kw)
