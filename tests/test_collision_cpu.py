"""The self-interpenetration term, the parts that need no GPU: the host-callable arithmetic of csrc/fdc_collide.h (the 17-axis test,
coll_pair_forward / coll_pair_backward, the face-order builder, the parameter check) compiled by plain g++
(tests/collision_cpu/coll_check.cpp) against the twin tests/collision_spec.py; innerfit.collision_filter; synth.make_body_mesh."""
import hashlib
import importlib

import numpy as np
import pytest
import torch

from tests import collision_spec as spec
from tests import gradient_bars as gb

synth = importlib.import_module("fdcap_amd.synth")
innerfit = importlib.import_module("fdcap_amd.innerfit")
capi = importlib.import_module("fdcap_amd.capi")


def _sat_host(S, T, tmp_path):
    P = np.concatenate([S, T], 1).astype(np.float32)
    return np.array([int(l) for l in spec.run_host("sat", [np.array([len(P)], np.int32), P], tmp_path)])


def _random_pairs(rng, n, size, needle=False):
    """triangle pairs whose centres are closer than their size, around (0.3, -0.2, 3): about a third intersect"""
    S = rng.standard_normal((n, 3, 3)) * size
    T = rng.standard_normal((n, 3, 3)) * size + rng.standard_normal((n, 1, 3)) * size * 0.4
    if needle:                                          # one corner pulled to 1 % of the way off its opposite edge, centroids 0.3 % apart
        for X in (S, T):
            foot = 0.5 * (X[:, 0] + X[:, 1])
            X[:, 2] = foot + 0.01 * (X[:, 2] - foot)
        T += S.mean(1, keepdims=True) - T.mean(1, keepdims=True) + rng.standard_normal((n, 1, 3)) * size * 0.003
    c = np.array([0.3, -0.2, 3.0])
    return (S + c).astype(np.float32), (T + c).astype(np.float32)


def _grazing_pairs(rng, n, size):
    """one corner of t a hair above or below the inside of s, the other two well above: hit or miss by 1e-6 of the size"""
    S = rng.standard_normal((n, 3, 3)) * size
    nrm = np.cross(S[:, 1] - S[:, 0], S[:, 2] - S[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    T = S.mean(1, keepdims=True) + rng.standard_normal((n, 3, 3)) * size * 0.1 + nrm[:, None] * size
    T[:, 0] = S.mean(1) + nrm * rng.uniform(-1e-6, 1e-6, (n, 1)) * size
    c = np.array([0.3, -0.2, 3.0])
    return (S + c).astype(np.float32), (T + c).astype(np.float32)


def test_axis_test_matches_the_fp64_twin_outside_its_margin(tmp_path):
    """Non-marginal pairs agree exactly; a pair is marginal when the twin's overlap (a hit) or gap (a miss), in units of |a| x the longer
    edge, is below tau of its axis (collision_spec.tau derives it from the header's expressions).  At most 2 % of the twin's hits
    may be marginal: measured 1.0 % on these seeds (25 of 2421 hits, most of them the grazing pairs built to be marginal)."""
    rng = np.random.Generator(np.random.PCG64(11))
    sets = [_random_pairs(rng, 3000, 0.03), _random_pairs(rng, 1500, 0.4), _grazing_pairs(rng, 30, 0.03), _random_pairs(rng, 1500, 0.03, needle=True)]
    S, T = np.concatenate([s for s, _ in sets]), np.concatenate([t for _, t in sets])
    got = _sat_host(S, T, tmp_path)
    assert not (got == 2).any()
    hit, gap, kappa = spec.sat(S.astype(np.float64), T.astype(np.float64))
    marg = np.array([spec.marginal(hit[i], gap[i], kappa[i]) for i in range(len(S))])
    print(f"pairs {len(S)}  twin hits {int(hit.sum())}  marginal hits {int((marg & hit).sum())}  marginal misses {int((marg & ~hit).sum())}  "
          f"disagreements inside the margin {int((got.astype(bool) != hit).sum())}")
    assert 0.1 * len(S) < hit.sum() < 0.9 * len(S) and marg.sum() > 10
    assert (marg & hit).sum() <= 0.02 * hit.sum()
    np.testing.assert_array_equal(got.astype(bool)[~marg], hit[~marg])
    # the needles alone: thin faces are decided too
    assert hit[-1500:].sum() > 20 and (~marg[-1500:]).sum() > 1200


def test_axis_test_on_exact_cases(tmp_path):
    """coordinates that fp32 holds and multiplies exactly: touching counts, coplanar faces are told apart, a zero axis never separates"""
    tri = lambda *p: np.array(p, np.float32)
    base = tri((0, 0, 0), (4, 0, 0), (0, 4, 0))
    cases = [
        (base, tri((1, 1, 0), (1, 1, 3), (2, 1, 3)), 1),                   # a corner on the face: touching is a hit
        (base, tri((1, 1, 1), (1, 1, 3), (2, 1, 3)), 0),                   # the same, lifted off
        (base, tri((1, 1, -1), (1, 1, 3), (2, 1, 3)), 1),                  # through the face
        (base, tri((1, 1, 0), (3, 1, 0), (1, 3, 0)), 1),                   # coplanar, inside
        (base, tri((3, 3, 0), (5, 3, 0), (3, 5, 0)), 0),                   # coplanar, beyond the long edge: only the in-plane normals separate
        (base, tri((5, 0, 0), (9, 0, 0), (5, 4, 0)), 0),                   # coplanar, beside
        (base, tri((4, 0, 0), (8, 0, 0), (4, 4, 0)), 1),                   # coplanar, touching at a corner (no shared INDEX here)
        (base, tri((0, 0, 1), (4, 0, 1), (0, 4, 1)), 0),                   # parallel planes: nine zero axes
        (base, tri((1, 1, 0), (1, 1, 0), (2, 1, 3)), 2),                   # degenerate: two equal corners
        (base, tri((1, 1, 0), (2, 2, 0), (3, 3, 0)), 2),                   # degenerate: collinear
        (tri((0, 0, 0), (np.nan, 0, 0), (0, 4, 0)), tri((1, 1, -1), (1, 1, 3), (2, 1, 3)), 2),
        (base, tri((1, 1, -1), (1, np.inf, 3), (2, 1, 3)), 2),
    ]
    S, T, want = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), [c[2] for c in cases]
    assert _sat_host(S, T, tmp_path).tolist() == want
    assert _sat_host(T, S, tmp_path).tolist() == want                       # either way round
    ok = spec.face_ok(S.astype(np.float64)) & spec.face_ok(T.astype(np.float64))
    hit, _, _ = spec.sat(S[ok].astype(np.float64), T[ok].astype(np.float64))
    assert hit.astype(int).tolist() == [w for w in want if w != 2]


def test_the_in_plane_axes_are_what_keeps_a_flat_patch_clean(tmp_path):
    v, f = spec.flat_grid(4, 4)
    assert spec.collision_set(v, f) == set()
    false_pairs = spec.collision_set(v, f, in_plane=False)
    disjoint = sum(1 for i in range(len(f)) for j in range(i + 1, len(f)) if not set(f[i]) & set(f[j]))
    print(f"flat 4 x 4 grid: {len(false_pairs)} of its {disjoint} vertex-disjoint pairs are reported without the six in-plane axes")
    assert len(false_pairs) >= 40                                            # second-ring neighbours whose boxes touch: all coplanar
    assert spec.host_pairs(v, f, None, None, tmp_path) == set()


def _penalty_cases(rng, n, scale, hlo, hhi):
    """receiver faces of edge ~scale and intruders inside their cones: [n,6,3], the receiver of the first three corners' Psi being the
    second face and the reverse -- both faces are built as receivers of the other's corners"""
    P = np.zeros((n, 6, 3))
    for i in range(n):
        a = rng.standard_normal((3, 3)) * scale
        u, v = a[1] - a[0], a[2] - a[0]
        nrm = np.cross(u, v)
        nrm /= np.linalg.norm(nrm)
        cen = a.mean(0)
        e1 = u / np.linalg.norm(u)
        e2 = np.cross(nrm, e1)
        r = np.linalg.norm(a - cen, axis=1).max()
        b = cen + (rng.uniform(-0.4, 0.4, (3, 1)) * e1 + rng.uniform(-0.4, 0.4, (3, 1)) * e2) * r + rng.uniform(hlo, hhi, (3, 1)) * nrm
        P[i, :3], P[i, 3:] = a, b
    return (P + np.array([0.3, -0.2, 3.0])).astype(np.float32)


def test_pair_penalty_and_total_gradient_match_fp64_autograd(tmp_path):
    """coll_pair_forward / coll_pair_backward at tests/gradient_bars.py's formula from the twin's two precisions; the gradient that
    holds the receiver's field fixed leaves those bars (recorded: max|err| / bar 1.7e3, against 0.03 for the header)"""
    rng = np.random.Generator(np.random.PCG64(5))
    sigma = 0.5
    # small faces: |h| < sigma; metre-sized ones deep behind the face: h <= -sigma
    P = np.concatenate([_penalty_cases(rng, 150, 0.03, -0.02, 0.02), _penalty_cases(rng, 60, 1.5, -1.4, -0.6), _penalty_cases(rng, 40, 1.5, -0.4, 0.7)])
    lines = spec.run_host("penalty", [np.array([len(P)], np.int32), np.array([sigma], np.float32), P], tmp_path)
    bw = np.array([[float(t) for t in ln.split()] for ln in lines[:len(P)]])
    fw = np.array([float(ln) for ln in lines[len(P):]])
    np.testing.assert_array_equal(bw[:, 0], fw)                              # the two entry points give the same value

    def twin(dtype, detach=False):
        t = torch.tensor(P, dtype=dtype, requires_grad=True)
        e = spec.pair_values(t, sigma, detach_receiver=detach)
        e.sum().backward()
        return {"value": e.detach().numpy().astype(np.float64), "grad": t.grad.numpy().astype(np.float64)}

    t64, t32 = twin(torch.float64), twin(torch.float32)
    assert (t64["value"] > 0).mean() > 0.9                                    # the cones are hit
    bar = gb.bars(t32, t64)
    got = {"value": bw[:, 0], "grad": bw[:, 1:].reshape(-1, 6, 3)}
    r = gb.ratios(got, t64, bar)
    print("header against fp64, max|err| / bar:", r)
    assert all(v <= 1.0 for v in r.values()), r
    # both branches of Y and a zero outside the cone are in the set
    deep = spec.pair_values(torch.tensor(P[150:210], dtype=torch.float64), sigma)
    assert (deep > 1.0).any()
    frozen = twin(torch.float64, detach=True)
    rf = gb.ratios({"grad": frozen["grad"]}, {"grad": t64["grad"]}, {"grad": bar["grad"]})
    print("gradient with the receiver's n, o, r held fixed, max|err| / bar:", rf)
    assert rf["grad"] > 100.0                                                 # measured 1.7e3
    np.testing.assert_array_equal(frozen["value"], t64["value"])


def test_collision_filter():
    f = innerfit.collision_filter
    bit = lambda m, a, b: (int(m[a]) >> b) & 1
    m = f(ignore_pairs=[(3, 40), (63, 0)], same_part=False)
    assert m.dtype == np.uint64 and m.shape == (64,)
    assert bit(m, 3, 40) and bit(m, 40, 3) and bit(m, 63, 0) and bit(m, 0, 63) and sum(bin(int(x)).count("1") for x in m) == 4
    parent = np.full(64, -1)
    parent[[4, 5, 7]] = [1, 2, 4]
    m = f(face_part=np.array([1, 4, 4, 7, 2]), part_parent=parent, same_part=True)
    assert all(bit(m, a, a) for a in (1, 2, 4, 7)) and not bit(m, 5, 5) and not bit(m, 0, 0)       # only parts that occur
    assert bit(m, 4, 1) and bit(m, 1, 4) and bit(m, 7, 4) and bit(m, 5, 2) and not bit(m, 7, 1)    # parent, not grandparent
    assert not f(same_part=False).any()
    assert all(bit(f(), a, a) for a in range(64))
    for bad in ([(64, 0)], [(0, -1)]):
        with pytest.raises(capi.FdcapError):
            f(ignore_pairs=bad)
    with pytest.raises(capi.FdcapError):
        f(part_parent=np.zeros(65, int))
    d = innerfit.DEFAULT_COLLISION
    assert d["weights"] == (0.0, 0.0, 0.0, 0.01, 1.0) and d["sigma"] == 0.5 and d["capacity"] > 0
    assert "[upstream-recall" in open(innerfit.__file__).read().split("DEFAULT_COLLISION = ")[0].rsplit("\n\n", 1)[-1]


def _order_host(vt, faces, leaf_want, tmp_path, part=None, V=None, F=None):
    V = len(vt) if V is None else V
    F = len(faces) if F is None else F
    words = [np.array([V, F, leaf_want, 0 if part is None else 1], np.int32), np.asarray(vt, np.float32), np.asarray(faces, np.int32),
             np.zeros(len(faces), np.int32) if part is None else np.asarray(part, np.int32)]
    lines = spec.run_host("order", words, tmp_path)
    if lines[0] == "err":
        return None
    leaf, NL, NLp = [int(t) for t in lines[0].split()[1:]]
    return leaf, NL, NLp, np.array(lines[1].split(), np.int32), np.array(lines[2].split(), np.int32).reshape(-1, 4)


@pytest.mark.parametrize("leaf", [32, 64])
def test_face_order_builder(leaf, tmp_path):
    rng = np.random.Generator(np.random.PCG64(7))
    for F in (3, leaf, leaf + 1, 2 * leaf + 5, 9 * leaf - 1):
        V = F + 2
        vt = rng.standard_normal((V, 3)).astype(np.float32)
        vt[V // 2:] = vt[V // 2]                                              # half the vertices coincide: many equal centroids
        vt[:, 1] = np.round(vt[:, 1] * 2) / 2                                 # ... and ties on an axis among the rest
        faces = np.stack([np.arange(F), np.arange(F) + 1, np.arange(F) + 2], 1).astype(np.int32)
        faces = faces[rng.permutation(F)]
        part = rng.integers(0, 64, F)
        got = _order_host(vt, faces, leaf, tmp_path, part=part)
        want = spec.face_order(vt, faces, leaf)
        assert got[:3] == want[:3] == (leaf, -(-F // leaf), got[2]) and got[2] >= got[1] and got[2] & (got[2] - 1) == 0 and got[2] < 2 * max(got[1], 1)
        np.testing.assert_array_equal(got[3], want[3])
        order = got[3]
        assert sorted(order[order >= 0].tolist()) == list(range(F)) and (order[:F] >= 0).all() and (order[F:] == -1).all()
        for l in range(got[1]):                                               # inside a leaf: ascending face id
            ids = order[l * leaf:(l + 1) * leaf]
            ids = ids[ids >= 0]
            assert (np.diff(ids) > 0).all()
        tri = got[4]
        np.testing.assert_array_equal(tri[:F, :3], faces[order[:F]])
        np.testing.assert_array_equal(tri[:F, 3], part[order[:F]])
        assert (tri[F:, 0] == -1).all()


def test_face_order_rules_by_hand(tmp_path):
    """130 faces along x with the centroid of every fourth one repeated: leaves of 32 are cut at the sorted positions 64 (root: left
    child full), then 32, 96 and 128; equal centroids fall on either side of a cut by face id"""
    F = 130
    x = np.repeat(np.arange((F + 3) // 4), 4)[:F].astype(np.float32)          # 0 0 0 0 1 1 1 1 ...
    perm = np.random.Generator(np.random.PCG64(3)).permutation(F)
    vt = np.zeros((3 * F, 3), np.float32)
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    for f in range(F):
        vt[3 * f:3 * f + 3] = np.array([[x[perm[f]], 0, 0], [x[perm[f]], 0.25, 0], [x[perm[f]], 0, 0.25]])
    leaf, NL, NLp, order, _ = _order_host(vt, faces, 32, tmp_path)
    assert (leaf, NL, NLp) == (32, 5, 8)
    by_key = sorted(range(F), key=lambda f: (x[perm[f]], f))
    for l in range(5):
        assert sorted(order[32 * l:32 * l + 32][order[32 * l:32 * l + 32] >= 0].tolist()) == sorted(by_key[32 * l:32 * l + 32])


def test_registration_refusals_of_the_builder(tmp_path):
    vt = np.random.Generator(np.random.PCG64(1)).standard_normal((10, 3)).astype(np.float32)
    faces = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], np.int32)
    assert _order_host(vt, faces, 32, tmp_path) is not None
    assert _order_host(vt, faces[:2], 32, tmp_path) is None                  # F < 3
    assert _order_host(vt, np.array([[0, 1, 10], [3, 4, 5], [6, 7, 8]]), 32, tmp_path) is None
    assert _order_host(vt, np.array([[0, 1, -1], [3, 4, 5], [6, 7, 8]]), 32, tmp_path) is None
    assert _order_host(vt, faces, 32, tmp_path, part=[0, 63, 5]) is not None
    assert _order_host(vt, faces, 32, tmp_path, part=[0, 64, 5]) is None
    big = np.zeros((65536, 3), np.int32)
    assert _order_host(vt, big, 32, tmp_path) is None
    got = _order_host(vt, big[:65535] + np.array([0, 1, 2]), 32, tmp_path)   # the largest mesh: leaves of 64, since 32 would need 2048
    assert got[:3] == (64, 1024, 1024)
    assert _order_host(vt, big[:32768] + np.array([0, 1, 2]), 32, tmp_path)[:3] == (32, 1024, 1024)
    prm = lambda s, w, c: spec.run_host("params", [np.array([s, w], np.float32), np.array([c], np.int32)], tmp_path) == ["1"]
    assert prm(0.5, 1.0, 1) and prm(0.999, 0.0, 10)
    assert not prm(0.0, 1.0, 1) and not prm(1.0, 1.0, 1) and not prm(np.nan, 1.0, 1) and not prm(-0.5, 1.0, 1)
    assert not prm(0.5, -1.0, 1) and not prm(0.5, np.inf, 1) and not prm(0.5, np.nan, 1) and not prm(0.5, 1.0, 0) and not prm(0.5, 1.0, -3)


def _digest(bm):
    h = hashlib.sha256()
    for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights", "hands_componentsl", "hands_componentsr",
              "hands_meanl", "hands_meanr"):
        h.update(np.ascontiguousarray(getattr(bm, k)).tobytes())
    return h.hexdigest()


def test_make_body_mesh_and_the_unchanged_body_model():
    # digests of make_body_model taken before synth.py learnt about faces
    assert _digest(synth.make_body_model(400, 0, 4)) == "0e456e0e011c0c0c8101e1529b5f29c168a82f44c00e6e88b1bbf40e15a5a985"
    assert _digest(synth.make_body_model(300, 3, 8)) == "dcc11a358aa4ea4b60735229bdd2f8281248f89c02cbb575bff0b8f7da715a8a"
    assert _digest(synth.make_body_model(1000, 1, 12)) == "be5dd9fb296497cc9d8adfc35f5569ec322151d948d6656b61f3d432f0e971b7"
    assert synth.make_body_model(200).faces is None
    bm0 = synth.make_body_model(200)
    assert synth.BodyModelData(*[getattr(bm0, k) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights",
                                                           "hands_componentsl", "hands_componentsr", "hands_meanl", "hands_meanr")]).faces is None
    for nv, nnz in ((300, 4), (2000, 8)):
        bm, part, parent = synth.make_body_mesh(nv, seed=2, lbs_nnz=nnz)
        V, f = bm.num_verts, bm.faces
        assert f.dtype == np.int32 and f.min() >= 0 and f.max() < V and sorted(set(f.reshape(-1).tolist())) == list(range(V))
        assert spec.face_ok(bm.v_template[f].astype(np.float64)).all()
        assert part.shape == (len(f),) and part.dtype == np.uint8 and part.max() < 64 and parent.shape == (64,)
        assert parent[4] == 1 and parent[18] == 16 and parent[1] == -1 and parent[0] == -1
        assert bm.posedirs.shape == (486, 3 * V) and bm.lbs_weights.shape == (V, 55) and ((bm.lbs_weights > 0).sum(1) == nnz).all()
        bm2, part2, _ = synth.make_body_mesh(nv, seed=2, lbs_nnz=nnz)
        assert _digest(bm2) == _digest(bm) and np.array_equal(bm2.faces, f) and np.array_equal(part2, part)
        assert _digest(synth.make_body_mesh(nv, seed=3, lbs_nnz=nnz)[0]) != _digest(bm)
    assert abs(synth.make_body_mesh(10475)[0].num_verts - 10475) < 200


# ---- the twin's additions for tests/test_gpu_collision_edges.py ---------------------------------------------------------------------------
def _case_digest(name):
    h = hashlib.sha256()
    vt, f, v, mv = spec.mesh_case(name)
    for a in (vt, f, v, mv, spec.frames_of(v, f, 3, mv)):
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def test_the_moved_mesh_builders_give_the_bytes_they_gave_in_the_gpu_module():
    """digests of (template, faces, frame, moving, three frames of it) taken from tests/test_gpu_collision.py's builders before they
    moved to tests/collision_spec.py"""
    want = {"tubes": "8791fa45d59f93730db8208bb0bb533723f180eda50b32e3f8694d7ad682558f",
            "tubes64": "8791fa45d59f93730db8208bb0bb533723f180eda50b32e3f8694d7ad682558f",
            "bent": "44165e2be7c62fb3fb4facd0f876c692550065e9f500edc8633919dd471cd438",
            "grid": "7b26691e9ab7ee5d156bd6aec4f44053323da6dfde8fc6c6f4fb4ca89bbddc41",
            "two_leaves_5": "b870f2ecbe5a6754fbe4fb6362260d19d2c313ac979ef90988cd6bbea001b658",
            "one_leaf": "72dbc002bf3ae1a7e0fdd859b572420f3296892f69cd8e61b8791871d6748a1b",
            "random": "8f6b14695d5c5a040a32ff4bf64b1791b29daf12ab232fee2795bb4a05668cfa"}
    assert set(want) == set(spec.MESHES)
    assert {name: _case_digest(name) for name in spec.MESHES} == want


@pytest.mark.parametrize("name", spec.MESHES)
def test_sweep_pairs_equals_every_pair_on_the_host(name, tmp_path):
    vt, faces, v0, moving = spec.mesh_case(name)
    verts = spec.frames_of(v0, faces, 3, moving)
    sizes = []
    for f in (0, 2):
        host = spec.host_pairs(verts[f], faces, None, None, tmp_path)
        assert spec.sweep_pairs(verts[f], faces, None, None, tmp_path) == host
        sizes.append(len(host))
    print(name, "pairs", sizes)
    assert name == "grid" or min(sizes) > 0


def test_sweep_pairs_with_parts_a_matrix_and_unusable_faces(tmp_path):
    vt, faces, v0, moving = spec.mesh_case("tubes")
    verts = spec.frames_of(v0, faces, 2, moving)[1]
    base = spec.host_pairs(verts, faces, None, None, tmp_path)
    part = (np.arange(len(faces)) * 7 % 5).astype(np.uint8)
    part[96:] += 40
    a0, b0 = sorted(base)[0]
    one_sided = np.zeros(64, np.uint64)
    one_sided[int(part[b0])] = np.uint64(1) << np.uint64(int(part[a0]))
    top = np.where(np.arange(len(faces)) < 96, 0, 63).astype(np.uint8)           # part 63 and bit 63
    bit = lambda a, b: np.uint64(1) << np.uint64(b)
    m63_0, m0_63, m63_63 = (np.zeros(64, np.uint64) for _ in range(3))
    m63_0[63], m0_63[0], m63_63[63] = bit(63, 0), bit(0, 63), bit(63, 63)
    for p, ign in ((part, innerfit.collision_filter(ignore_pairs=[(int(part[a0]), int(part[b0])), (0, 40)], same_part=False)), (part, one_sided),
                   (part, None), (None, one_sided), (top, m63_0), (top, m0_63), (top, m63_63), (top[::-1].copy(), m63_63)):
        host = spec.host_pairs(verts, faces, p, ign, tmp_path)
        assert spec.sweep_pairs(verts, faces, p, ign, tmp_path) == host
        if p is part and ign is not None:
            assert 0 < len(host) < len(base)
    assert spec.host_pairs(verts, faces, top, m63_0, tmp_path) == spec.host_pairs(verts, faces, top, m0_63, tmp_path) == \
        {p for p in base if (p[0] < 96) == (p[1] < 96)}                          # either one-sided bit drops every cross-tube pair
    # unusable faces: +inf, -inf, NaN, an exactly zero-area face, and a frame with no usable face
    hit = sorted({i for p in base for i in p})
    for k, (val, how) in enumerate(((np.inf, "coord"), (-np.inf, "coord"), (np.nan, "coord"), (None, "flat"))):
        v = verts.copy()
        f = faces[hit[k]]
        if how == "coord":
            v[f[0], 1] = val
            gone = {int(i) for i in np.nonzero((faces == f[0]).any(1))[0]}
        else:
            v[f[1]] = v[f[0]]                                                    # the same position twice: e0 = 0 exactly
            gone = {hit[k]}
        host = spec.host_pairs(v, faces, None, None, tmp_path)
        assert spec.sweep_pairs(v, faces, None, None, tmp_path) == host
        assert not any(set(p) & gone for p in host) and len(host) > 0
        if how == "coord":                                                       # (the moved corner of the flat face bends its neighbours)
            assert host == {p for p in base if not set(p) & gone} and len(host) < len(base)
    dead = np.full_like(verts, np.nan)
    assert spec.sweep_pairs(dead, faces, None, None, tmp_path) == spec.host_pairs(dead, faces, None, None, tmp_path) == set()


def test_sweep_pairs_a_strict_sweep_loses_boxes_that_touch(tmp_path):
    """two faces that meet in the one point (4, 4, 0), where their boxes touch on all three axes (exact in fp32): a hit for the header,
    kept by the sweep's <=, lost by the mutant's < whichever axis it sweeps"""
    v = np.array([(0, 0, 0), (4, 4, 0), (0, 4, 0), (4, 4, 0), (8, 4, 0), (4, 8, 3), (20, 20, 20), (21, 20, 20), (20, 21, 20)], np.float32)
    f = np.arange(9, dtype=np.int32).reshape(3, 3)
    host = spec.host_pairs(v, f, None, None, tmp_path)
    assert host == {(0, 1)}
    assert spec.sweep_pairs(v, f, None, None, tmp_path) == host
    assert spec.sweep_pairs(v, f, None, None, tmp_path, strict=True) == set()
    # ... and on a mesh, where a strict sweep is otherwise right, faces moved to touch in this way are what it loses
    vt, faces, v0, _ = spec.mesh_case("tubes")
    vv = np.concatenate([v0, v[:6] + np.array([16, 16, 0], np.float32)])           # (clear of the tubes)
    ff = np.concatenate([faces, f[:2] + len(v0)])
    host = spec.host_pairs(vv, ff, None, None, tmp_path)
    assert spec.sweep_pairs(vv, ff, None, None, tmp_path) == host
    assert host - spec.sweep_pairs(vv, ff, None, None, tmp_path, strict=True) == {(len(faces), len(faces) + 1)}


def _tube_pairs(f, tmp_path):
    vt, faces, v0, moving = spec.mesh_case("tubes")
    verts = spec.frames_of(v0, faces, f + 1, moving)[f]
    pr = np.array(sorted(spec.host_pairs(verts, faces, None, None, tmp_path)))
    return np.concatenate([verts[faces[pr[:, 0]]], verts[faces[pr[:, 1]]]], 1)


def test_psi_tags_names_the_return_taken(tmp_path):
    """the tubes' frame 0 (48 pairs x 6 intruders): sigma 0.5 never reaches the deep branch or the h >= sigma return, sigma 0.05 reaches all
    four; the fp32 and the fp64 twin take the same return for every intruder of frames 0..2 at every sigma tried"""
    P = _tube_pairs(0, tmp_path)
    assert P.shape == (48, 6, 3)
    count = lambda sigma: np.bincount(spec.psi_tags(P, sigma).reshape(-1), minlength=5).tolist()
    assert count(0.5) == [0, 0, 75, 0, 213]
    assert count(0.05) == [64, 0, 73, 19, 132]
    for f in range(3):
        Pf = _tube_pairs(f, tmp_path)
        for sigma in (0.5, 0.05, 0.02, 0.01):
            t64, t32 = spec.psi_tags(Pf, sigma), spec.psi_tags(Pf, sigma, torch.float32)
            assert (t64 == t32).all() and not (t64 == spec.TAG_RHO).any(), (f, sigma)
            # against the twin's own value: zero exactly where a zero return is named, per intruder
            Pt = torch.tensor(Pf, dtype=torch.float64)
            for recv in (0, 1):
                R, O = Pt[:, 3 * recv:3 * recv + 3], Pt[:, 3 * (1 - recv):3 * (1 - recv) + 3]
                n, o, r = spec._field(R[:, 0], R[:, 1], R[:, 2])
                for k in range(3):
                    val = spec._psi2(n, o, r, O[:, k], sigma).numpy()
                    np.testing.assert_array_equal(val == 0, t64[:, recv, k] <= spec.TAG_OUTSIDE)
    # by hand: a unit right triangle in z = 0 (circumcentre (0.5, 0.5, 0), r = 0.7071), intruders above its circumcentre
    recv = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], float)
    intr = np.array([(0.5, 0.5, 0.3), (0.5, 0.5, -0.3), (0.5, 0.5, 0.1)])       # sigma 0.2: above, deep, quadratic
    tags = spec.psi_tags(np.concatenate([recv, intr])[None], 0.2)[0, 0]
    assert tags.tolist() == [spec.TAG_ABOVE, spec.TAG_DEEP, spec.TAG_QUAD]
    wide = np.array([(3.0, 0.5, 0.1), (0.5, 0.5, 0.1), (0.5, 0.5, 0.1)])         # beside the cone: phi >= 1
    assert spec.psi_tags(np.concatenate([recv, wide])[None], 0.2)[0, 0, 0] == spec.TAG_OUTSIDE


def test_node_boxes_by_hand_and_by_their_properties():
    # by hand: five faces in leaves of two under a four-leaf tree; the face at x = 2 has a NaN corner
    v = np.zeros((15, 3), np.float32)
    for f in range(5):
        v[3 * f:3 * f + 3] = np.array([(f, 0, 0), (f + 0.5, 0, 1), (f, 0.25, 0)])
    v[7, 2] = np.nan
    faces = np.arange(15, dtype=np.int32).reshape(5, 3)
    order = np.array([0, 1, 2, 3, 4, -1], np.int32)
    b = spec.node_boxes(v, faces, order, 2, 3, 4)
    inf = np.inf
    assert b.dtype == np.float32 and b.shape == (8, 6)
    assert b[4].tolist() == [0, 0, 0, 1.5, 0.25, 1] and b[5].tolist() == [3, 0, 0, 3.5, 0.25, 1] and b[6].tolist() == [4, 0, 0, 4.5, 0.25, 1]
    assert b[7].tolist() == [inf, inf, inf, -inf, -inf, -inf]
    assert b[2].tolist() == [0, 0, 0, 3.5, 0.25, 1] and b[3].tolist() == b[6].tolist() and b[1].tolist() == [0, 0, 0, 4.5, 0.25, 1]
    # properties on a mesh whose frame has nothing to do with the template
    vt, faces, v0, _ = spec.mesh_case("random")
    for leaf_want in (32, 64):
        leaf, NL, NLp, order = spec.face_order(vt, faces, leaf_want)
        v = v0.copy()
        v[faces[order[0]][0], 0] = np.inf
        b = spec.node_boxes(v, faces, order, leaf, NL, NLp)
        ok = spec.face_ok(v[faces])
        assert not ok.all()
        P = v[faces[ok]]
        assert b[1, :3].tolist() == P.min((0, 1)).tolist() and b[1, 3:].tolist() == P.max((0, 1)).tolist() and np.isfinite(b[1]).all()
        for p, f in enumerate(order):
            if f >= 0 and ok[f]:
                node = NLp + p // leaf
                while node >= 1:                                              # inside its leaf's box and every ancestor's
                    assert (b[node, :3] <= v[faces[f]].min(0)).all() and (v[faces[f]].max(0) <= b[node, 3:]).all()
                    node //= 2
        assert (b[NLp + NL:, :3] == inf).all() and (b[NLp + NL:, 3:] == -inf).all()
    dead = spec.node_boxes(np.full_like(v0, np.nan), faces, order, leaf, NL, NLp)
    assert (dead[:, :3] == inf).all() and (dead[:, 3:] == -inf).all()
