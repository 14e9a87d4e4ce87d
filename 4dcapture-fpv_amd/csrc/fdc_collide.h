// Self-interpenetration of the body mesh (fdcap_set_collision_mesh, fdcap_collision_eval): which pairs of faces of one frame's world
// mesh intersect, and the penalty of Tzionas et al. (IJCV 2016) on them with its total gradient.  Everything is a function of the
// inputs alone: no float atomics, integer stores only where their order cannot matter.
//
// THE COLLISION SET of a frame: every unordered pair {s, t} of registered faces that
//   (0) are both usable: all nine coordinates finite and |e0 x e1|^2 > 1e-30, e0 = p1 - p0, e1 = p2 - p0          (coll_face_ok)
//   (1) have overlapping boxes: lo_s <= hi_t and lo_t <= hi_s on x, y, z (implied by (4) in exact arithmetic; here so that
//       the culled search and the every-pair launch apply the same predicate)                                      (coll_box_overlap)
//   (2) share no vertex index                                                                                       (coll_share_vertex)
//   (3) are not dropped by the part matrix: bit (part[s], part[t]) or bit (part[t], part[s])
//   (4) have no separating axis among 17: the two normals, the nine edge x edge products, the six in-plane edge normals n x e
//       (the last six make disjoint COPLANAR faces miss: on a flat patch all the others are zero or the common normal).
//       Separated on a: max_s < min_t or max_t < min_s, strictly -- an all-zero axis never separates, touching is a hit.  (coll_tri_sat)
// fp32 throughout, every operation rounded on its own (contraction off where it is written: g++ -ffp-contract=off and the device then
// round alike -- fdc_chamfer_bwd.h on why the *_rn intrinsics do not do that), in the order written here.  A NaN makes every comparison
// false: a face that touches one fails (0) and is in no pair; no coordinate is ever turned into an address.
//
// THE TREE.  Registration (coll_mesh_build, pure host code) orders the faces once, by the TEMPLATE's face centroids, into NL = ceil(F /
// LEAF) leaves of LEAF consecutive tree positions under an implicit complete binary tree over NLp = 2^H >= NL leaves (heap numbering:
// root 1, children 2 i and 2 i + 1, leaf l = node NLp + l; leaves NL.. are empty).  Specification of the order:
//   centroid   c = (p0 + p1) + p2 per component in fp32 (three times the centroid: only compared)
//   a node that spans w > 1 leaves and holds m faces gives its left child the first min(m, (w / 2) LEAF) faces and the right child
//   the rest (cut rule: the left subtree is filled first, so every leaf but the last is full), in the order
//     (c[axis], face id) ascending, axis = the one with the largest extent max c - min c over the node's faces, the lowest axis on a
//     tie (tie rule: equal centroids go by face id)
//   inside a leaf the faces stand by ascending face id.
// The tree's shape never changes; per evaluation only its boxes are refit (coll_refit_kernel).  A tree that fits badly (a pose far from
// the template) costs time, never a pair.
//
// THE LIST of a frame: the owner of a pair is the face earlier in tree order; pairs stand by (owner's tree position, other's tree
// position).  A count pass, an in-place exclusive prefix per frame and an emit pass give that order without a sort: one wave serves one
// (frame, leaf), walks the tree left to right (stackless: the heap numbering gives the next node), keeps the leaves at or after its own
// whose boxes meet its own, holds its faces one per lane (LEAF = 32: each face on two lanes, which take the other leaf's even and odd
// faces) and takes the other leaf's faces through LDS.  count[frame] is the number FOUND; the first `capacity` are kept.
// coll_every_kernel is the same predicate over all pairs with no tree: the checker the culled search must equal.
//
// THE PENALTY of a kept pair (s owner, t other; corners 0..5 = s0 s1 s2 t0 t1 t2).  For a receiver face (a, b, c): u = b - a, v = c - a,
// w = u x v, n = w / |w|, circumcentre o = a + ((|u|^2 v - |v|^2 u) x w) / (2 |w|^2), circumradius r = |o - a|.  For an intruder p:
//   h = n . (p - o)    rho = r - (r / sigma) h    Phi = |(p - o) - h n| / rho    Psi = (1 - Phi) Y(h) if rho > 0, Phi < 1, h < sigma; else 0
//   Y(h) = -h + 1 - sigma (h <= -sigma);  -(1 - 2 sigma) / (4 sigma^2) h^2 - h / (2 sigma) + (3 - 2 sigma) / 4 (|h| < sigma)
//   e = (Psi_s(t0)^2 + Psi_s(t1)^2 + Psi_s(t2)^2) + (Psi_t(s0)^2 + Psi_t(s1)^2 + Psi_t(s2)^2), added left to right
// A frame's value is w_coll x (its kept pairs' e added in list order).  The gradient is the TOTAL derivative with respect to all six
// vertices, through n, o and r of the receiver too: forward-mode derivatives, three directions (one vertex) at a time (coll_pair_backward),
// grouped by destination vertex with fdc_chamfer_bwd.h's stable radix sort (key frame x V + vertex) and added per vertex in
// ascending (list position, corner) order.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "fdc_math.h"

#if defined(__clang__)
#define FDC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define FDC_NO_CONTRACT
#endif

namespace fdc {

constexpr int COLL_MIN_FACES = 3, COLL_MAX_FACES = 65535, COLL_PARTS = 64;
constexpr int COLL_MAX_LEAVES = 1024;           // NLp: a frame's 2 NLp boxes of six floats stay inside 48 KiB of LDS
constexpr float COLL_DEGENERATE = 1e-30f;

// ---- the predicate ---------------------------------------------------------------------------------------------------------------
// false for NaN and the infinities -- by the exponent's bits: the library is built with -fno-honor-nans, under which a floating-point
// comparison may be assumed to see no NaN
FDC_HD bool coll_finite(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    return (u & 0x7f800000u) != 0x7f800000u;
}

FDC_HD void coll_cross(const float a[3], const float b[3], float r[3]) {
    FDC_NO_CONTRACT
    r[0] = a[1] * b[2] - a[2] * b[1];
    r[1] = a[2] * b[0] - a[0] * b[2];
    r[2] = a[0] * b[1] - a[1] * b[0];
}
FDC_HD float coll_dot(const float a[3], const float b[3]) {
    FDC_NO_CONTRACT
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
FDC_HD void coll_sub(const float a[3], const float b[3], float r[3]) { FDC_NO_CONTRACT r[0] = a[0] - b[0]; r[1] = a[1] - b[1]; r[2] = a[2] - b[2]; }

FDC_HD bool coll_face_ok(const float p[3][3]) {
    bool fin = true;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) fin = fin && coll_finite(p[i][k]);
    float e0[3], e1[3], w[3];
    coll_sub(p[1], p[0], e0); coll_sub(p[2], p[0], e1);
    coll_cross(e0, e1, w);
    return fin && coll_dot(w, w) > COLL_DEGENERATE;
}
FDC_HD void coll_face_box(const float p[3][3], float lo[3], float hi[3]) {
    for (int k = 0; k < 3; ++k) { lo[k] = fminf(fminf(p[0][k], p[1][k]), p[2][k]); hi[k] = fmaxf(fmaxf(p[0][k], p[1][k]), p[2][k]); }
}
FDC_HD bool coll_box_overlap(const float alo[3], const float ahi[3], const float blo[3], const float bhi[3]) {
    return alo[0] <= bhi[0] && blo[0] <= ahi[0] && alo[1] <= bhi[1] && blo[1] <= ahi[1] && alo[2] <= bhi[2] && blo[2] <= ahi[2];
}
FDC_HD bool coll_share_vertex(const int32_t a[3], const int32_t b[3]) {
    bool s = false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s = s || a[i] == b[j];
    return s;
}
// ign: the 64 x 64 bit matrix made symmetric at registration
FDC_HD bool coll_part_dropped(const unsigned long long* ign, int ps, int pt) { return ((ign[ps] >> pt) & 1ull) != 0ull; }

// projections on `a` of the six corners, taken relative to s[0] (qs, qt): separated, strictly
FDC_HD bool coll_axis_separates(const float a[3], const float qs[3][3], const float qt[3][3]) {
    const float s0 = coll_dot(a, qs[0]), s1 = coll_dot(a, qs[1]), s2 = coll_dot(a, qs[2]);
    const float t0 = coll_dot(a, qt[0]), t1 = coll_dot(a, qt[1]), t2 = coll_dot(a, qt[2]);
    const float smin = fminf(fminf(s0, s1), s2), smax = fmaxf(fmaxf(s0, s1), s2);
    const float tmin = fminf(fminf(t0, t1), t2), tmax = fmaxf(fmaxf(t0, t1), t2);
    return smax < tmin || tmax < smin;
}
// true: no separating axis among the 17.  Edges from the corners themselves (k: p[k+1] - p[k], cyclic), normals (p1 - p0) x (p2 - p0).
FDC_HD bool coll_tri_sat(const float s[3][3], const float t[3][3]) {
    float qs[3][3], qt[3][3], es[3][3], et[3][3], ns[3], nt[3], a[3], d[3];
    for (int i = 0; i < 3; ++i) {
        coll_sub(s[i], s[0], qs[i]); coll_sub(t[i], s[0], qt[i]);
        coll_sub(s[(i + 1) % 3], s[i], es[i]); coll_sub(t[(i + 1) % 3], t[i], et[i]);
    }
    coll_sub(s[2], s[0], d); coll_cross(es[0], d, ns);
    coll_sub(t[2], t[0], d); coll_cross(et[0], d, nt);
    if (coll_axis_separates(ns, qs, qt) || coll_axis_separates(nt, qs, qt)) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            coll_cross(es[i], et[j], a);
            if (coll_axis_separates(a, qs, qt)) return false;
        }
    for (int i = 0; i < 3; ++i) {
        coll_cross(ns, es[i], a);
        if (coll_axis_separates(a, qs, qt)) return false;
    }
    for (int i = 0; i < 3; ++i) {
        coll_cross(nt, et[i], a);
        if (coll_axis_separates(a, qs, qt)) return false;
    }
    return true;
}
// the whole predicate on one pair, in the order box, shared vertex, part matrix, 17 axes
FDC_HD bool coll_pair_test(const float s[3][3], const int32_t si[3], int sp, const float t[3][3], const int32_t ti[3], int tp,
                           const unsigned long long* ign) {
    if (!coll_face_ok(s) || !coll_face_ok(t)) return false;
    float slo[3], shi[3], tlo[3], thi[3];
    coll_face_box(s, slo, shi); coll_face_box(t, tlo, thi);
    if (!coll_box_overlap(slo, shi, tlo, thi)) return false;
    if (coll_share_vertex(si, ti)) return false;
    if (coll_part_dropped(ign, sp, tp)) return false;
    return coll_tri_sat(s, t);
}

// ---- the penalty: values that carry N directional derivatives ---------------------------------------------------------------------
template <int N>
struct CollD { float v = 0.f; float d[N > 0 ? N : 1] = {}; };

template <int N> FDC_HD CollD<N> cd_const(float v) { CollD<N> r; r.v = v; for (int i = 0; i < N; ++i) r.d[i] = 0.f; return r; }
template <int N> FDC_HD CollD<N> cd_add(const CollD<N>& a, const CollD<N>& b) { FDC_NO_CONTRACT CollD<N> r; r.v = a.v + b.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
template <int N> FDC_HD CollD<N> cd_sub(const CollD<N>& a, const CollD<N>& b) { FDC_NO_CONTRACT CollD<N> r; r.v = a.v - b.v; for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
template <int N> FDC_HD CollD<N> cd_mul(const CollD<N>& a, const CollD<N>& b) {
    FDC_NO_CONTRACT
    CollD<N> r; r.v = a.v * b.v;
    for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
    return r;
}
template <int N> FDC_HD CollD<N> cd_scale(float s, const CollD<N>& a) { FDC_NO_CONTRACT CollD<N> r; r.v = s * a.v; for (int i = 0; i < N; ++i) r.d[i] = s * a.d[i]; return r; }
template <int N> FDC_HD CollD<N> cd_div(const CollD<N>& a, const CollD<N>& b) {
    FDC_NO_CONTRACT
    CollD<N> r; const float ib = 1.f / b.v; r.v = a.v * ib;
    for (int i = 0; i < N; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * ib;
    return r;
}
template <int N> FDC_HD CollD<N> cd_sqrt(const CollD<N>& a) {            // (a.v > 0)
    FDC_NO_CONTRACT
    CollD<N> r; r.v = sqrtf(a.v); const float h = 0.5f / r.v;
    for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * h;
    return r;
}
template <int N> FDC_HD CollD<N> cd_dot(const CollD<N> a[3], const CollD<N> b[3]) { return cd_add(cd_add(cd_mul(a[0], b[0]), cd_mul(a[1], b[1])), cd_mul(a[2], b[2])); }
template <int N> FDC_HD void cd_cross(const CollD<N> a[3], const CollD<N> b[3], CollD<N> r[3]) {
    r[0] = cd_sub(cd_mul(a[1], b[2]), cd_mul(a[2], b[1]));
    r[1] = cd_sub(cd_mul(a[2], b[0]), cd_mul(a[0], b[2]));
    r[2] = cd_sub(cd_mul(a[0], b[1]), cd_mul(a[1], b[0]));
}

template <int N>
struct CollField { CollD<N> n[3], o[3], r; };

template <int N>
FDC_HD CollField<N> coll_field(const CollD<N> a[3], const CollD<N> b[3], const CollD<N> c[3]) {
    CollField<N> f;
    CollD<N> u[3], v[3], w[3], m[3], cc[3];
    for (int k = 0; k < 3; ++k) { u[k] = cd_sub(b[k], a[k]); v[k] = cd_sub(c[k], a[k]); }
    cd_cross(u, v, w);
    const CollD<N> w2 = cd_dot(w, w), uu = cd_dot(u, u), vv = cd_dot(v, v);
    for (int k = 0; k < 3; ++k) m[k] = cd_sub(cd_mul(uu, v[k]), cd_mul(vv, u[k]));
    cd_cross(m, w, cc);
    const CollD<N> den = cd_scale(2.f, w2), wl = cd_sqrt(w2);
    CollD<N> orel[3];
    for (int k = 0; k < 3; ++k) { orel[k] = cd_div(cc[k], den); f.o[k] = cd_add(a[k], orel[k]); f.n[k] = cd_div(w[k], wl); }
    f.r = cd_sqrt(cd_dot(orel, orel));
    return f;
}
// Psi_f(p)^2
template <int N>
FDC_HD CollD<N> coll_psi2(const CollField<N>& f, const CollD<N> p[3], float sigma) {
    CollD<N> d[3], t[3];
    for (int k = 0; k < 3; ++k) d[k] = cd_sub(p[k], f.o[k]);
    const CollD<N> h = cd_dot(f.n, d);
    if (!(h.v < sigma)) return cd_const<N>(0.f);                        // Y = 0 (and rho <= 0)
    const CollD<N> rho = cd_sub(f.r, cd_mul(cd_scale(1.f / sigma, f.r), h));
    if (!(rho.v > 0.f)) return cd_const<N>(0.f);
    for (int k = 0; k < 3; ++k) t[k] = cd_sub(d[k], cd_mul(h, f.n[k]));
    const CollD<N> t2 = cd_dot(t, t);
    const CollD<N> phi = t2.v > 0.f ? cd_div(cd_sqrt(t2), rho) : cd_const<N>(0.f);      // (on the axis: Phi = 0, flat)
    if (!(phi.v < 1.f)) return cd_const<N>(0.f);
    CollD<N> ups;
    if (h.v <= -sigma) ups = cd_sub(cd_const<N>(1.f - sigma), h);
    else {
        const float c2 = -(1.f - 2.f * sigma) / (4.f * sigma * sigma), c1 = -1.f / (2.f * sigma), c0 = (3.f - 2.f * sigma) / 4.f;
        ups = cd_add(cd_add(cd_scale(c2, cd_mul(h, h)), cd_scale(c1, h)), cd_const<N>(c0));
    }
    const CollD<N> psi = cd_mul(cd_sub(cd_const<N>(1.f), phi), ups);
    return cd_mul(psi, psi);
}

// P: the six corners s0 s1 s2 t0 t1 t2.  -> e
FDC_HD float coll_pair_forward(const float P[6][3], float sigma) {
    FDC_NO_CONTRACT
    float e[2];
    for (int recv = 0; recv < 2; ++recv) {
        CollD<0> R[3][3], O[3];
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) R[i][k] = cd_const<0>(P[3 * recv + i][k]);
        const CollField<0> f = coll_field<0>(R[0], R[1], R[2]);
        float acc = 0.f;
        for (int i = 0; i < 3; ++i) {
            for (int k = 0; k < 3; ++k) O[k] = cd_const<0>(P[3 * (1 - recv) + i][k]);
            const float v = coll_psi2<0>(f, O, sigma).v;
            acc = i == 0 ? v : acc + v;
        }
        e[recv] = acc;
    }
    return e[0] + e[1];
}
// -> e; g[6][3] = d e / d P, total (the receiver's n, o, r move with its corners)
FDC_HD float coll_pair_backward(const float P[6][3], float sigma, float g[6][3]) {
    FDC_NO_CONTRACT
    for (int i = 0; i < 6; ++i)
        for (int k = 0; k < 3; ++k) g[i][k] = 0.f;
    for (int recv = 0; recv < 2; ++recv) {
        const int rb = 3 * recv, ob = 3 * (1 - recv);
        CollD<3> R[3][3], O[3];
        // through the receiver's field: one receiver corner's three directions at a time
        for (int seed = 0; seed < 3; ++seed) {
            for (int i = 0; i < 3; ++i)
                for (int k = 0; k < 3; ++k) { R[i][k] = cd_const<3>(P[rb + i][k]); if (i == seed) R[i][k].d[k] = 1.f; }
            const CollField<3> f = coll_field<3>(R[0], R[1], R[2]);
            for (int i = 0; i < 3; ++i) {
                for (int k = 0; k < 3; ++k) O[k] = cd_const<3>(P[ob + i][k]);
                const CollD<3> v = coll_psi2<3>(f, O, sigma);
                for (int k = 0; k < 3; ++k) g[rb + seed][k] = g[rb + seed][k] + v.d[k];
            }
        }
        // through the intruder
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) R[i][k] = cd_const<3>(P[rb + i][k]);
        const CollField<3> f = coll_field<3>(R[0], R[1], R[2]);
        for (int i = 0; i < 3; ++i) {
            for (int k = 0; k < 3; ++k) { O[k] = cd_const<3>(P[ob + i][k]); O[k].d[k] = 1.f; }
            const CollD<3> v = coll_psi2<3>(f, O, sigma);
            for (int k = 0; k < 3; ++k) g[ob + i][k] = g[ob + i][k] + v.d[k];
        }
    }
    return coll_pair_forward(P, sigma);
}

// ---- registration: validation and the face order (pure host code; tests/collision_cpu) -----------------------------------------------
struct CollTables {
    int F = 0, V = 0, leaf = 0, NL = 0, NLp = 0, H = 0;
    std::vector<int32_t> order;          // [NL * leaf] tree position -> face id, -1 behind the last face
    std::vector<int32_t> tri;            // [NL * leaf][4] v0 v1 v2 part of the face at a tree position (v0 = -1: none)
    std::vector<unsigned long long> ign; // [64] the part matrix, made symmetric
};
// leaf size of a mesh of F faces: `want` (32 or 64; anything else: 32), raised to 64 where 32 would need more than COLL_MAX_LEAVES
inline int coll_pick_leaf(int F, int want) {
    const int leaf = want == 64 ? 64 : 32;
    return (F + leaf - 1) / leaf > COLL_MAX_LEAVES ? 64 : leaf;
}
// 0, or nonzero for what fdcap_set_collision_mesh refuses with FDCAP_E_ARG: F outside [3, 65535], a vertex index outside [0, V), a
// part above 63 (face_part NULL: all 0; ignore NULL: none dropped)
inline int coll_mesh_build(int F, const int32_t* faces, const uint8_t* face_part, const uint64_t* ignore, int V, const float* vt,
                           int leaf_want, CollTables* out) {
    FDC_NO_CONTRACT
    if (F < COLL_MIN_FACES || F > COLL_MAX_FACES || !faces || !vt || V <= 0) return 1;
    for (int i = 0; i < 3 * F; ++i) if (faces[i] < 0 || faces[i] >= V) return 1;
    if (face_part) for (int i = 0; i < F; ++i) if (face_part[i] >= COLL_PARTS) return 1;
    CollTables& t = *out;
    t.F = F; t.V = V; t.leaf = coll_pick_leaf(F, leaf_want);
    t.NL = (F + t.leaf - 1) / t.leaf;
    t.NLp = 1; t.H = 0;
    while (t.NLp < t.NL) { t.NLp *= 2; ++t.H; }
    std::vector<float> c((size_t)3 * F);
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k) c[3 * (size_t)f + k] = (vt[3 * (size_t)faces[3 * f] + k] + vt[3 * (size_t)faces[3 * f + 1] + k]) + vt[3 * (size_t)faces[3 * f + 2] + k];
    std::vector<int32_t> idx((size_t)F);
    for (int f = 0; f < F; ++f) idx[f] = f;
    struct Span { int lo, hi, w; };
    std::vector<Span> todo{{0, F, t.NLp}};
    while (!todo.empty()) {
        const Span s = todo.back(); todo.pop_back();
        if (s.w == 1 || s.hi - s.lo <= 0) { std::sort(idx.begin() + s.lo, idx.begin() + s.hi); continue; }
        const int nleft = std::min(s.hi - s.lo, (s.w / 2) * t.leaf);
        if (nleft < s.hi - s.lo) {
            int axis = 0; float best = -1.f;
            for (int k = 0; k < 3; ++k) {
                float lo = c[3 * (size_t)idx[s.lo] + k], hi = lo;
                for (int i = s.lo + 1; i < s.hi; ++i) { const float v = c[3 * (size_t)idx[i] + k]; lo = std::min(lo, v); hi = std::max(hi, v); }
                if (hi - lo > best) { best = hi - lo; axis = k; }
            }
            std::sort(idx.begin() + s.lo, idx.begin() + s.hi, [&](int32_t a, int32_t b) {
                const float ca = c[3 * (size_t)a + axis], cb = c[3 * (size_t)b + axis];
                return ca < cb || (ca == cb && a < b);
            });
            todo.push_back({s.lo + nleft, s.hi, s.w / 2});
        }
        todo.push_back({s.lo, s.lo + nleft, s.w / 2});
    }
    const size_t np = (size_t)t.NL * t.leaf;
    t.order.assign(np, -1); t.tri.assign(4 * np, 0);
    for (size_t p = 0; p < np; ++p) {
        t.tri[4 * p] = -1;
        if (p >= (size_t)F) continue;
        const int f = idx[p];
        t.order[p] = f;
        for (int k = 0; k < 3; ++k) t.tri[4 * p + k] = faces[3 * f + k];
        t.tri[4 * p + 3] = face_part ? face_part[f] : 0;
    }
    t.ign.assign(COLL_PARTS, 0ull);
    if (ignore)
        for (int a = 0; a < COLL_PARTS; ++a)
            for (int b = 0; b < COLL_PARTS; ++b)
                if ((ignore[a] >> b) & 1ull) { t.ign[a] |= 1ull << b; t.ign[b] |= 1ull << a; }
    return 0;
}
// what fdcap_collision_eval refuses with FDCAP_E_ARG
inline bool coll_params_ok(float sigma, float w_coll, int capacity) {
    return coll_finite(sigma) && sigma > 0.f && sigma < 1.f && coll_finite(w_coll) && w_coll >= 0.f && capacity > 0;
}

#if defined(__HIPCC__)
// ---- the kernels -------------------------------------------------------------------------------------------------------------------
struct CollMesh {
    int F, leaf, NL, NLp, H;
    const int4* tri;                     // [NL * leaf] v0 v1 v2 part
    const int* order;                    // [NL * leaf]
    const unsigned long long* ign;       // [64]
};

__device__ __forceinline__ void coll_load_face(const float* __restrict__ vf, const int4 t, float p[3][3]) {
    const int id[3] = {t.x, t.y, t.z};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) p[i][k] = vf[3 * (size_t)id[i] + k];
}

// One workgroup per frame: face boxes -> leaf boxes -> the upper levels in LDS -> nodes [frame][2 NLp][6] {lo, hi} (node 0 unused).
// An unusable face (coll_face_ok) is in no box; an empty box is {+inf, -inf} and meets nothing.
template <int LEAF>
__global__ __launch_bounds__(256) void coll_refit_kernel(CollMesh m, const float* __restrict__ verts, int V, float* __restrict__ nodes) {
    extern __shared__ __attribute__((aligned(16))) float coll_lds[];       // [2 NLp][6]
    const int frame = blockIdx.x, tid = threadIdx.x;
    const float* const vf = verts + (size_t)frame * V * 3;
    const int npos = m.NLp * LEAF, nreal = m.NL * LEAF;
    for (int base = 0; base < npos; base += 256) {
        const int pos = base + tid;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (pos < nreal) {
            const int4 t = m.tri[pos];
            if (t.x >= 0) {
                float p[3][3];
                coll_load_face(vf, t, p);
                if (coll_face_ok(p)) coll_face_box(p, lo, hi);
            }
        }
#pragma unroll
        for (int sh = 1; sh < LEAF; sh *= 2)
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], sh)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], sh)); }
        // (the fold above runs on all 256 lanes; a tree of fewer than 256 positions -- F <= 128 -- has no leaf behind npos to store)
        if (pos < npos && pos % LEAF == 0) {
            float* const b = coll_lds + 6 * (size_t)(m.NLp + pos / LEAF);
#pragma unroll
            for (int k = 0; k < 3; ++k) { b[k] = lo[k]; b[3 + k] = hi[k]; }
        }
    }
    __syncthreads();
    for (int w = m.NLp / 2; w >= 1; w >>= 1) {
        for (int i = w + tid; i < 2 * w; i += 256) {
            const float* const a = coll_lds + 6 * (size_t)(2 * i);
            float* const b = coll_lds + 6 * (size_t)i;
#pragma unroll
            for (int k = 0; k < 3; ++k) { b[k] = fminf(a[k], a[6 + k]); b[3 + k] = fmaxf(a[3 + k], a[9 + k]); }
        }
        __syncthreads();
    }
    float* const out = nodes + (size_t)frame * 2 * m.NLp * 6;
    for (int i = 6 + tid; i < 12 * m.NLp; i += 256) out[i] = coll_lds[i];
}

// what a wave keeps of the other leaf's faces in LDS, one array of LEAF words per field
constexpr int COLL_STAGE_WORDS = 20;     // 9 coordinates, box lo / hi, v0 v1 v2, part, usable

// One wave per (frame, leaf).  EMIT = false: cnt[frame][pos] <- pairs owned by the face at tree position pos.  EMIT = true: cnt holds the
// frame's exclusive prefix; the pairs go to list[frame][slot] = {owner's position, other's position} while slot < capacity.
template <int LEAF, bool EMIT>
__global__ __launch_bounds__(256) void coll_search_kernel(CollMesh m, const float* __restrict__ verts, int V, const float* __restrict__ nodes,
                                                          int* __restrict__ cnt, int capacity, int2* __restrict__ list) {
    constexpr int SUB = 64 / LEAF;                                      // lanes per own face
    __shared__ float stage_all[4][COLL_STAGE_WORDS][LEAF];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, frame = blockIdx.y;
    const int L = blockIdx.x * 4 + wave;
    if (L >= m.NL) return;                                              // (whole waves; nothing below synchronises the workgroup)
    float (*const stage)[LEAF] = stage_all[wave];
    const float* const vf = verts + (size_t)frame * V * 3;
    const float* const nb = nodes + (size_t)frame * 2 * m.NLp * 6;
    const int own = lane % LEAF, half = lane / LEAF, mypos = L * LEAF + own;
    const int4 mt = m.tri[mypos];
    float s[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, slo[3] = {0.f, 0.f, 0.f}, shi[3] = {0.f, 0.f, 0.f};
    bool sok = false;
    if (mt.x >= 0) { coll_load_face(vf, mt, s); sok = coll_face_ok(s); coll_face_box(s, slo, shi); }
    const int32_t si[3] = {mt.x, mt.y, mt.z};
    const unsigned long long myrow = m.ign[mt.w & 63];
    float blo[3], bhi[3];                                               // the own leaf's box (wave-uniform)
#pragma unroll
    for (int k = 0; k < 3; ++k) { blo[k] = nb[6 * (size_t)(m.NLp + L) + k]; bhi[k] = nb[6 * (size_t)(m.NLp + L) + 3 + k]; }
    int found = 0;
    const int base = EMIT ? cnt[(size_t)frame * m.NL * LEAF + mypos] : 0;
    int node = 1, depth = 0;
    while (true) {
        // leaves of this subtree: [first, last]
        const int first = (node << (m.H - depth)) - m.NLp, last = ((node + 1) << (m.H - depth)) - m.NLp - 1;
        const float* const b = nb + 6 * (size_t)node;
        const bool meet = last >= L && first < m.NL && coll_box_overlap(blo, bhi, b, b + 3);
        if (meet && depth < m.H) { node = 2 * node; ++depth; continue; }
        if (meet) {
            const int M = first;                                        // a leaf at or after the own one whose box meets it
            {   // its faces, one per lane, into LDS
                const int j = lane % LEAF;
                const int4 ot = m.tri[M * LEAF + j];
                float p[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}}, lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
                bool ok = false;
                if (ot.x >= 0) { coll_load_face(vf, ot, p); ok = coll_face_ok(p); coll_face_box(p, lo, hi); }
                if (half == 0) {
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int k = 0; k < 3; ++k) stage[3 * i + k][j] = p[i][k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) { stage[9 + k][j] = lo[k]; stage[12 + k][j] = hi[k]; }
                    stage[15][j] = __int_as_float(ot.x); stage[16][j] = __int_as_float(ot.y); stage[17][j] = __int_as_float(ot.z);
                    stage[18][j] = __int_as_float(ot.w); stage[19][j] = __int_as_float(ok ? 1 : 0);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int it = 0; it < LEAF / SUB; ++it) {
                const int j = it * SUB + half;
                bool hit = false;
                if (sok && (M > L || j > own) && __float_as_int(stage[19][j]) != 0) {
                    const float tlo[3] = {stage[9][j], stage[10][j], stage[11][j]}, thi[3] = {stage[12][j], stage[13][j], stage[14][j]};
                    if (coll_box_overlap(slo, shi, tlo, thi)) {
                        const int32_t ti[3] = {__float_as_int(stage[15][j]), __float_as_int(stage[16][j]), __float_as_int(stage[17][j])};
                        const int tp = __float_as_int(stage[18][j]);
                        if (!coll_share_vertex(si, ti) && ((myrow >> tp) & 1ull) == 0ull) {
                            float t[3][3];
#pragma unroll
                            for (int i = 0; i < 3; ++i)
#pragma unroll
                                for (int k = 0; k < 3; ++k) t[i][k] = stage[3 * i + k][j];
                            hit = coll_tri_sat(s, t);
                        }
                    }
                }
                // the own face's lanes take j ascending: lane `half` stands behind the hits of the lanes before it
                int before = 0, all = hit ? 1 : 0;
                if (SUB == 2) {
                    const int h0 = __shfl(hit ? 1 : 0, own), h1 = __shfl(hit ? 1 : 0, own + LEAF);
                    before = half == 1 ? h0 : 0; all = h0 + h1;
                }
                if (EMIT && hit) {
                    const int slot = base + found + before;
                    if (slot < capacity) list[(size_t)frame * capacity + slot] = make_int2(mypos, M * LEAF + j);
                }
                found += all;
            }
            __builtin_amdgcn_wave_barrier();
        }
        // the next node in left-to-right order: the sibling, or an ancestor's
        node = node + 1;
        const int up = __builtin_ctz(node);
        node >>= up; depth -= up;
        if (node == 1) break;
    }
    if (!EMIT && half == 0) cnt[(size_t)frame * m.NL * LEAF + mypos] = found;
}

// The same predicate over all pairs, no tree: one lane per (frame, owner position), every later position in turn.
template <bool EMIT>
__global__ __launch_bounds__(256) void coll_every_kernel(CollMesh m, const float* __restrict__ verts, int V, int* __restrict__ cnt, int capacity,
                                                         int2* __restrict__ list) {
    const int npos = m.NL * m.leaf, pos = blockIdx.x * 256 + threadIdx.x, frame = blockIdx.y;
    if (pos >= npos) return;
    const float* const vf = verts + (size_t)frame * V * 3;
    const int4 mt = m.tri[pos];
    int found = 0;
    if (mt.x >= 0) {
        float s[3][3];
        coll_load_face(vf, mt, s);
        const int32_t si[3] = {mt.x, mt.y, mt.z};
        const int base = EMIT ? cnt[(size_t)frame * npos + pos] : 0;
        for (int j = pos + 1; j < npos; ++j) {
            const int4 ot = m.tri[j];
            if (ot.x < 0) continue;
            float t[3][3];
            coll_load_face(vf, ot, t);
            const int32_t ti[3] = {ot.x, ot.y, ot.z};
            if (!coll_pair_test(s, si, mt.w & 63, t, ti, ot.w & 63, m.ign)) continue;
            if (EMIT && base + found < capacity) list[(size_t)frame * capacity + base + found] = make_int2(pos, j);
            ++found;
        }
    }
    if (!EMIT) cnt[(size_t)frame * npos + pos] = found;
}

// One workgroup per frame: cnt[frame][0 .. npos) -> its exclusive prefix, in place; count[frame] <- the total (the pairs FOUND)
__global__ __launch_bounds__(256) void coll_prefix_kernel(int* __restrict__ cnt, int npos, int* __restrict__ count) {
    __shared__ int part[256];
    const int frame = blockIdx.x, tid = threadIdx.x, per = (npos + 255) / 256;
    int* const c = cnt + (size_t)frame * npos;
    const int lo = min(tid * per, npos), hi = min(lo + per, npos);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += c[i];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
        count[frame] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int i = lo; i < hi; ++i) { const int v = c[i]; c[i] = run; run += v; }
}

// One lane per (frame, slot): the kept pair's value and its 18 gradient components (x w_coll), the destination vertex of each corner
// for the grouping (-1 behind the kept pairs: cb_keys_kernel gives those the key behind the last vertex), the caller's pair list.
__global__ __launch_bounds__(256) void coll_penalty_kernel(CollMesh m, const float* __restrict__ verts, int V, int n, const int* __restrict__ count,
                                                           int capacity, const int2* __restrict__ list, float sigma, float w_coll,
                                                           float* __restrict__ val, float* __restrict__ grad, int* __restrict__ dest,
                                                           int* __restrict__ pairs_out) {
    FDC_NO_CONTRACT
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)n * capacity) return;
    const int frame = (int)(q / capacity), slot = (int)(q - (long long)frame * capacity);
    const bool kept = slot < min(count[frame], capacity);
    int2 pr = make_int2(0, 0);
    if (kept) pr = list[q];
    // (positions the search wrote: inside [0, npos) by construction; held there all the same before they address anything)
    const int npos = m.NL * m.leaf;
    const bool ok = kept && pr.x >= 0 && pr.x < npos && pr.y >= 0 && pr.y < npos;
    if (pairs_out) { pairs_out[2 * q] = ok ? m.order[pr.x] : -1; pairs_out[2 * q + 1] = ok ? m.order[pr.y] : -1; }
    if (!ok) {
        val[q] = 0.f;
        if (dest)
            for (int c = 0; c < 6; ++c) dest[6 * q + c] = -1;
        return;
    }
    const int4 a = m.tri[pr.x], b = m.tri[pr.y];
    const float* const vf = verts + (size_t)frame * V * 3;
    float P[6][3], g[6][3];
    {
        float p[3][3];
        coll_load_face(vf, a, p);
        for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) P[i][k] = p[i][k];
        coll_load_face(vf, b, p);
        for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) P[3 + i][k] = p[i][k];
    }
    if (!dest) { val[q] = coll_pair_forward(P, sigma); return; }
    val[q] = coll_pair_backward(P, sigma, g);
    const int id[6] = {a.x, a.y, a.z, b.x, b.y, b.z};
    for (int c = 0; c < 6; ++c) {
        dest[6 * q + c] = id[c];
        for (int k = 0; k < 3; ++k) grad[18 * q + 3 * c + k] = w_coll * g[c][k];
    }
}

// loss[frame] = w_coll x (the kept pairs' values added in list order); one lane per frame
__global__ __launch_bounds__(64) void coll_frame_sum_kernel(const float* __restrict__ val, const int* __restrict__ count, int n, int capacity,
                                                            float w_coll, float* __restrict__ loss) {
    FDC_NO_CONTRACT
    const int frame = blockIdx.x * 64 + threadIdx.x;
    if (frame >= n) return;
    const int kept = min(count[frame], capacity);
    float acc = 0.f;
    for (int p = 0; p < kept; ++p) acc = acc + val[(size_t)frame * capacity + p];
    loss[frame] = w_coll * acc;
}

// One lane per (frame, vertex) = its key: the run of its contributions in the grouped order, added as they stand
__global__ __launch_bounds__(256) void coll_gather_kernel(const unsigned* __restrict__ skey, const int* __restrict__ sval, int nsorted,
                                                          const float* __restrict__ grad, long long ndest, float* __restrict__ dverts) {
    FDC_NO_CONTRACT
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= ndest) return;
    const unsigned want = (unsigned)t;
    int lo = 0, hi = nsorted;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (skey[mid] < want) lo = mid + 1; else hi = mid;
    }
    float acc[3] = {0.f, 0.f, 0.f};
    for (int s = lo; s < nsorted && skey[s] == want; ++s) {
        const float* const g = grad + 3 * (size_t)sval[s];
        for (int k = 0; k < 3; ++k) acc[k] = acc[k] + g[k];
    }
    for (int k = 0; k < 3; ++k) dverts[3 * (size_t)t + k] = acc[k];
}
#endif  // __HIPCC__

}  // namespace fdc
