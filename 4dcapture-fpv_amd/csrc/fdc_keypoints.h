// The inner fit's data term on a detector's keypoints: a static map from keypoints to SMPL-X joints and
// points of the mesh surface, and the loss / backward of the mapped points.  Objective: csrc/fdc_fit2d.h, unchanged -- only the
// set of projected points differs.
//
// A mapped keypoint is a JOINT j in 0..54 or a SURFACE POINT b0 v[t0] + b1 v[t1] + b2 v[t2] (a plain vertex: (v, v, v), (1, 0, 0)).
// Its position is "SMPL-X output + transl + camera_translation" for every kind: the inner fit's set-up (camera_ext rows =
// identity, scale = 1, include/fdcap.h).
//   joints 0..22   : read from the pose forward's world joints Jw, gradient into dJw -- the 23-joint path's own numbers
//   joints 23..54  : a PSEUDO-VERTEX of the keypoint set: rest position Jt_j + Jd_j beta (the collapsed regressor of the pose
//                    tables), no pose-blend offset, skinning weight 1 on joint j.  A_j [J_j; 1] is the translation of G_j
//                    (A = G - pad(G [J; 0])), so it lands on the posed joint and its gradient reaches the pose backward
//                    as dA / d betas like any vertex's -- no wider Jw, no change to the pose kernels
//   surface points : the unique real vertices the triples name, skinned here
// The keypoint set (real vertices first, then pseudo-vertices; at most 3 x 160) is skinned, combined, projected and differentiated
// by ONE workgroup per frame (fit2d_kp_kernel) with nothing in between in global memory -- but for the set's two blend products
// where they run as panel products around it (kp_blend_by_panels).  Sums over keypoints that share a vertex or a joint run in the
// fixed order of the map's lists: no float atomics, a frame's gradient is reproducible.
//
// The first part is pure host code (validation + de-duplication, plain g++ -std=c++17: tests/test_keypoints_cpu.py), the second the
// per-keypoint math as host / device functions, the third the kernel.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "fdc_fit2d.h"
#include "fdc_lbfgs.h"
#include "fdc_skin.h"

namespace fdc {

constexpr int KP_MAX = 160;            // = FDCAP_MAX_KEYPOINTS (asserted where both are visible)
constexpr int KP_MAXV = 3 * KP_MAX;    // vertices of the keypoint set

// ---- the map, validated and de-duplicated (host) ---------------------------------------------------------------------------------
struct KeypointTables {
    int n_kp = 0, nr = 0, np = 0;            // keypoints, unique real vertices, pseudo-vertices; set vertex u: real u < nr, pseudo nr + i
    std::vector<int32_t> real_ids;           // [nr] mesh vertex ids, ascending
    std::vector<int32_t> pseudo_joint;       // [np] joints 23..54 in use, ascending
    std::vector<int32_t> kjoint;             // [n_kp] the joint 0..22 a keypoint reads from Jw, else -1
    std::vector<int32_t> kref;               // [n_kp][3] set vertices of a keypoint that is not read from Jw (else 0)
    std::vector<float> kbary;                // [n_kp][3] their weights (a joint 23..54: (1, 0, 0))
    // per set vertex, the keypoints that touch it: entries [vl_start[u], vl_start[u + 1]) ascending in (keypoint, corner);
    // corners of weight 0 contribute an exact zero and are left out
    std::vector<int32_t> vl_start, vl_k;
    std::vector<float> vl_w;
    // per joint 0..22, the keypoints that read it, ascending
    std::vector<int32_t> jl_start, jl_k;
    int nu() const { return nr + np; }
};

// 0, or -1 (FDCAP_E_ARG): n_kp outside [0, KP_MAX], joint >= 55, a surface point with a vertex id outside [0, V) or a non-finite weight
inline int keypoint_map_build(int n_kp, const int32_t* joint, const int32_t* tri, const float* bary, int V, KeypointTables* out) {
    *out = KeypointTables();
    if (n_kp < 0 || n_kp > KP_MAX) return -1;
    if (n_kp > 0 && (!joint || !tri || !bary)) return -1;
    for (int k = 0; k < n_kp; ++k) {
        if (joint[k] >= 55) return -1;
        if (joint[k] >= 0) continue;
        for (int i = 0; i < 3; ++i)
            if (tri[3 * k + i] < 0 || tri[3 * k + i] >= V || !std::isfinite(bary[3 * k + i])) return -1;
    }
    KeypointTables& t = *out;
    t.n_kp = n_kp;
    for (int k = 0; k < n_kp; ++k) {
        if (joint[k] >= 23) t.pseudo_joint.push_back(joint[k]);
        else if (joint[k] < 0) for (int i = 0; i < 3; ++i) t.real_ids.push_back(tri[3 * k + i]);
    }
    auto uniq = [](std::vector<int32_t>& v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); };
    uniq(t.real_ids); uniq(t.pseudo_joint);
    t.nr = (int)t.real_ids.size(); t.np = (int)t.pseudo_joint.size();
    auto find = [](const std::vector<int32_t>& v, int32_t x) { return (int32_t)(std::lower_bound(v.begin(), v.end(), x) - v.begin()); };
    t.kjoint.assign((size_t)n_kp, -1); t.kref.assign((size_t)3 * n_kp, 0); t.kbary.assign((size_t)3 * n_kp, 0.f);
    for (int k = 0; k < n_kp; ++k) {
        if (joint[k] >= 0 && joint[k] < 23) { t.kjoint[k] = joint[k]; continue; }
        if (joint[k] >= 23) {
            const int32_t u = t.nr + find(t.pseudo_joint, joint[k]);
            t.kref[3 * k] = t.kref[3 * k + 1] = t.kref[3 * k + 2] = u;
            t.kbary[3 * k] = 1.f;
            continue;
        }
        for (int i = 0; i < 3; ++i) { t.kref[3 * k + i] = find(t.real_ids, tri[3 * k + i]); t.kbary[3 * k + i] = bary[3 * k + i]; }
    }
    const int nu = t.nu();
    t.vl_start.assign((size_t)nu + 1, 0);
    for (int u = 0; u < nu; ++u) {
        t.vl_start[u] = (int32_t)t.vl_k.size();
        for (int k = 0; k < n_kp; ++k) {
            if (t.kjoint[k] >= 0) continue;
            for (int i = 0; i < 3; ++i)
                if (t.kref[3 * k + i] == u && t.kbary[3 * k + i] != 0.f) { t.vl_k.push_back(k); t.vl_w.push_back(t.kbary[3 * k + i]); }
        }
    }
    t.vl_start[nu] = (int32_t)t.vl_k.size();
    t.jl_start.assign(24, 0);
    for (int j = 0; j < 23; ++j) {
        t.jl_start[j] = (int32_t)t.jl_k.size();
        for (int k = 0; k < n_kp; ++k) if (t.kjoint[k] == j) t.jl_k.push_back(k);
    }
    t.jl_start[23] = (int32_t)t.jl_k.size();
    return 0;
}

// Where the pose + shape blend product of the set's real vertices runs.  In the kernel (plain fp32 multiply-adds, every workgroup
// streams the set's blend matrix from L2: 2 x 496 x 3 nr x 4 bytes per frame, forward and backward) or as the set's panel products
// around it (blend_forward / blend_backward: two more launches and [frames, 3 nu] offsets and gradients through HBM, but the matrix is
// read once per sixteen frames by the matrix cores).  Measured (profiles/keypoints_fit.json): the kernel's own
// product wins while frames x columns is small; FDCAP_KP_BLEND=kernel / =panel pins one (read by fdcap_opt_set_keypoints_mapped).
constexpr long KP_PANEL_MIN_WORK = 64L * 300;          // frames x (3 nr) from which the panel products take over
inline bool kp_blend_by_panels(int frames, int ncol) {
    const char* e = getenv("FDCAP_KP_BLEND");
    if (e && !strcmp(e, "kernel")) return false;
    if (ncol <= 0) return false;
    if (e && !strcmp(e, "panel")) return true;
    return (long)frames * ncol >= KP_PANEL_MIN_WORK;
}

// ---- the per-keypoint math (host and device) --------------------------------------------------------------------------------------
// position of a keypoint: its joint's row of Jw [23][3], or the combination of its set vertices' positions vw [nu][3]
FDC_HD V3 kp_position(int kj, const int32_t* ref, const float* b, const float* Jw, const float* vw) {
    if (kj >= 0) return v3(Jw[3 * kj], Jw[3 * kj + 1], Jw[3 * kj + 2]);
    const float *p0 = vw + 3 * ref[0], *p1 = vw + 3 * ref[1], *p2 = vw + 3 * ref[2];
    return v3(b[0] * p0[0] + b[1] * p1[0] + b[2] * p2[0], b[0] * p0[1] + b[1] * p1[1] + b[2] * p2[1],
              b[0] * p0[2] + b[1] * p1[2] + b[2] * p2[2]);
}
// d loss / d position of set vertex u: its list's entries in order, weight x d loss / d keypoint (dkp [n_kp][3])
FDC_HD V3 kp_vertex_grad(int u, const int32_t* vl_start, const int32_t* vl_k, const float* vl_w, const float* dkp) {
    V3 g = v3(0.f, 0.f, 0.f);
    for (int q = vl_start[u]; q < vl_start[u + 1]; ++q) {
        const float* d = dkp + 3 * vl_k[q];
        const float w = vl_w[q];
        g.x += w * d[0]; g.y += w * d[1]; g.z += w * d[2];
    }
    return g;
}
// d loss / d world joint j < 23: the first keypoint's gradient as it is (one keypoint per joint: the 23-joint path's bits), then the others
FDC_HD V3 kp_joint_grad(int j, const int32_t* jl_start, const int32_t* jl_k, const float* dkp) {
    const int q0 = jl_start[j], q1 = jl_start[j + 1];
    if (q0 == q1) return v3(0.f, 0.f, 0.f);
    V3 g = v3(dkp[3 * jl_k[q0]], dkp[3 * jl_k[q0] + 1], dkp[3 * jl_k[q0] + 2]);
    for (int q = q0 + 1; q < q1; ++q) { const float* d = dkp + 3 * jl_k[q]; g.x += d[0]; g.y += d[1]; g.z += d[2]; }
    return g;
}
// ---- the free jaw (host and device) --------------------------------------------------------------------------------------------
// Joint 22 has parent 15 and no child, so a jaw pose w (axis-angle) changes two things of the model at w = 0 and nothing else: the
// pose-feature block 9 (22 - 1) .. = R_w - I, and the joint's skinning transform A' = (R_A R_w, t_A + R_A (I - R_w) J22), with
// (R_A, t_A) the transform pose_fwd_kernel writes for R_22 = I and J22 the joint's rest position.  The joint's own position, every
// other transform and every Jw row stay.  At w = 0 every line is the fixed model.
constexpr int JAW_J = 22;
// rest position of joint j: Jt_j + Jd_j betas (pose_forward's joint_rest, term for term)
FDC_HD V3 kp_joint_rest(const float* Jt, const float* Jd, const float* betas, int j) {
    float p[3];
    for (int c = 0; c < 3; ++c) {
        float acc = Jt[3 * j + c];
        for (int l = 0; l < NBETA; ++l) acc += Jd[(3 * j + c) * NBETA + l] * betas[l];
        p[c] = acc;
    }
    return v3(p[0], p[1], p[2]);
}
struct JawFwd { M3 Rw, RA; V3 J22, lever; };               // lever = (I - R_w) J22
// A22 [12] (rows [R | t]): A_22 in, A'_22 out; pf9 (=) R_w - I
FDC_HD JawFwd jaw_forward(V3 w, V3 J22, float* A22, float* pf9) {
    JawFwd f;
    f.Rw = rodrigues_forward(w);
    f.J22 = J22;
    for (int i = 0; i < 3; ++i) for (int c = 0; c < 3; ++c) f.RA.m[3 * i + c] = A22[4 * i + c];
    f.lever = J22 - m3_vec(f.Rw, J22);
    const M3 R = m3_mul(f.RA, f.Rw);
    const V3 sh = m3_vec(f.RA, f.lever);
    for (int i = 0; i < 3; ++i) for (int c = 0; c < 3; ++c) A22[4 * i + c] = R.m[3 * i + c];
    A22[3] += sh.x; A22[7] += sh.y; A22[11] += sh.z;
    for (int e = 0; e < 9; ++e) pf9[e] = f.Rw.m[e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
    return f;
}
// dAp [12] = (dR', dt'): d loss / d A'_22  ->  the skinning part of d loss / d R_w (the pose-feature block's gradient g_P is added by
// whoever consumes the jaw's gradient: jaw_grad), what the pose backward receives as d loss / d A_22, and d loss / d J22
struct JawBwd { M3 dRw; float dA22[12]; V3 dJ22; };
FDC_HD JawBwd jaw_backward(const JawFwd& f, const float* dAp) {
    JawBwd b;
    M3 dRp;
    for (int i = 0; i < 3; ++i) for (int c = 0; c < 3; ++c) dRp.m[3 * i + c] = dAp[4 * i + c];
    const V3 dtp = v3(dAp[3], dAp[7], dAp[11]);
    const V3 q = m3t_vec(f.RA, dtp);                       // R_A^T dt' = d loss / d lever
    b.dRw = m3_mul_at(f.RA, dRp);                          // R_A^T dR' - q J22^T
    m3_add_outer(b.dRw, -1.f * q, f.J22);
    M3 r = m3_mul_bt(dRp, f.Rw);                           // dR' R_w^T + dt' lever^T
    m3_add_outer(r, dtp, f.lever);
    for (int i = 0; i < 3; ++i) for (int c = 0; c < 3; ++c) b.dA22[4 * i + c] = r.m[3 * i + c];
    b.dA22[3] = dtp.x; b.dA22[7] = dtp.y; b.dA22[11] = dtp.z;
    b.dJ22 = q - m3t_vec(f.Rw, q);                         // (I - R_w)^T q
    return b;
}

// ---- the free expression (host and device) --------------------------------------------------------------------------------------
// SMPL-X's expression coefficients psi [10] are ten more shape directions: v_shaped = v_template + S betas + E psi, and the joints
// are regressed from v_shaped, so every joint's rest position moves by delta_j = JE_j psi (JE = J_regressor E, [55 3][10]).  The pose
// forward ran at psi = 0; with (R_j, t_j) its chain (R_j = the rotation of A_j) and p the parent of j
//     Dt_0 = delta_0,  Dt_j = Dt_p + R_p (delta_j - delta_p),   A_j.t += Dt_j - R_j delta_j,   Jw_j += W Dt_j  (j < 23)
// which is the model itself, not an approximation.  The set's real vertices gain E_u psi in front of the skinning and a pseudo-vertex
// delta_j; rotations and the pose feature stay.  The recursion is unrolled per joint -- Dt_j = delta_0 + the sum over j's path to the
// root -- so that 55 lanes walk their own paths side by side and nobody waits for a level.
// Backward, from d loss / d A' (the kernel's sums) and d loss / d Jw: own_j = dA'_j.t + W^T dJw_j is what reaches Dt_j directly, S_j
// the sum of own over j's strict descendants -- S_j = the sum over j's children c of g_c, g_j = S_j + own_j, formed level by level from
// the deepest (expr_subtree_children; lane j = joint j of one wave, as the pose backward's subtree sums) -- and
//     d delta_j = -R_j^T (dA'_j.t + S_j) + (j > 0 ? R_p^T g_j : g_0)
//     dA_j.R   += -dA'_j.t delta_j^T + sum over the children c of j of g_c (delta_c - delta_j)^T
// pose_bwd_kernel then differentiates the unchanged chain from the augmented dA.  All sums in a fixed order.
constexpr int NEXPR = 10;
FDC_HD float expr_delta_entry(const float* JE, const float* psi, int e) {          // delta [55 3], entry e = 3 j + c
    float acc = 0.f;
    for (int l = 0; l < NEXPR; ++l) acc += JE[e * NEXPR + l] * psi[l];
    return acc;
}
// Dt_j; A: [55][12] rows [R | t] (only the rotations are read)
FDC_HD V3 expr_chain_shift(const float* A, const int* parents, const float* delta, int j) {
    V3 acc = v3(0.f, 0.f, 0.f);
    for (int a = j, p = parents[j]; p >= 0; a = p, p = parents[p]) {
        const float* R = A + 12 * p;
        const V3 d = v3(delta[3 * a] - delta[3 * p], delta[3 * a + 1] - delta[3 * p + 1], delta[3 * a + 2] - delta[3 * p + 2]);
        acc = acc + v3(R[0] * d.x + R[1] * d.y + R[2] * d.z, R[4] * d.x + R[5] * d.y + R[6] * d.z, R[8] * d.x + R[9] * d.y + R[10] * d.z);
    }
    return acc + v3(delta[0], delta[1], delta[2]);
}
// joint j: A_j.t += Dt_j - R_j delta_j (reads rotations only, writes A_j's translation only: the joints run side by side); -> Dt_j
FDC_HD V3 expr_forward(float* A, const int* parents, const float* delta, int j) {
    const V3 dt = expr_chain_shift(A, parents, delta, j);
    float* a = A + 12 * j;
    const V3 d = v3(delta[3 * j], delta[3 * j + 1], delta[3 * j + 2]);
    a[3] += dt.x - (a[0] * d.x + a[1] * d.y + a[2] * d.z);
    a[7] += dt.y - (a[4] * d.x + a[5] * d.y + a[6] * d.z);
    a[11] += dt.z - (a[8] * d.x + a[9] * d.y + a[10] * d.z);
    return dt;
}
// S_j: g_c = S_c + own_c over the children c of j, ascending -- the children's S must be there: joints by level, the deepest first
FDC_HD V3 expr_subtree_children(const int* child_start, const int* child_list, const float* own, const float* S, int j) {
    V3 acc = v3(0.f, 0.f, 0.f);
    for (int q = child_start[j]; q < child_start[j + 1]; ++q) {
        const int c = child_list[q];
        acc = acc + v3(S[3 * c] + own[3 * c], S[3 * c + 1] + own[3 * c + 1], S[3 * c + 2] + own[3 * c + 2]);
    }
    return acc;
}
// d delta_j; dA: [55][12] d loss / d A' (its translation column is read)
FDC_HD V3 expr_backward_delta(const float* A, const int* parents, const float* own, const float* S, const float* dA, int j) {
    const float* R = A + 12 * j;
    const V3 s = v3(S[3 * j], S[3 * j + 1], S[3 * j + 2]);
    const V3 g = s + v3(own[3 * j], own[3 * j + 1], own[3 * j + 2]);
    const V3 v = v3(dA[12 * j + 3], dA[12 * j + 7], dA[12 * j + 11]) + s;
    const V3 a = v3(R[0] * v.x + R[4] * v.y + R[8] * v.z, R[1] * v.x + R[5] * v.y + R[9] * v.z, R[2] * v.x + R[6] * v.y + R[10] * v.z);
    const int p = parents[j];
    if (p < 0) return g - a;
    const float* P = A + 12 * p;
    return v3(P[0] * g.x + P[4] * g.y + P[8] * g.z, P[1] * g.x + P[5] * g.y + P[9] * g.z, P[2] * g.x + P[6] * g.y + P[10] * g.z) - a;
}
// the addend to entry (i, col) of dA_j's rotation
FDC_HD float expr_backward_rot_entry(const int* child_start, const int* child_list, const float* delta, const float* own, const float* S,
                                     const float* dA, int j, int i, int col) {
    float acc = -dA[12 * j + 4 * i + 3] * delta[3 * j + col];
    for (int q = child_start[j]; q < child_start[j + 1]; ++q) {
        const int c = child_list[q];
        acc += (S[3 * c + i] + own[3 * c + i]) * (delta[3 * c + col] - delta[3 * j + col]);
    }
    return acc;
}
// JE = J_regressor E in double, as host_pose_setup builds Jd.  E10: [V 3][10] (shapedirs' columns 10..19), JE: [55 3][10]
inline void expr_joint_dirs(int V, const float* E10, const float* J_regressor, float* JE) {
    for (int j = 0; j < NJ; ++j)
        for (int k = 0; k < 3; ++k) {
            double d[NEXPR] = {0};
            for (int v = 0; v < V; ++v) {
                const double w = J_regressor[(size_t)j * V + v];
                if (w == 0.0) continue;
                for (int l = 0; l < NEXPR; ++l) d[l] += w * E10[((size_t)3 * v + k) * NEXPR + l];
            }
            for (int l = 0; l < NEXPR; ++l) JE[(3 * j + k) * NEXPR + l] = (float)d[l];
        }
}

// One frame on the host, in the kernel's order: positions, data term and d loss / d keypoint, then the gradients of the set
// vertices' positions (gvw [nu][3]) and of the 23 world joints (dJw [23][3]).  Returns the frame's data term.
inline float kp_frame_host(const Fit2dStage& s, const KeypointTables& t, const float* Jw, const float* vw, const float* kp, float* pos,
                           float* dkp, float* gvw, float* dJw) {
    float data = 0.f;
    for (int k = 0; k < t.n_kp; ++k) {
        const V3 p = kp_position(t.kjoint[k], &t.kref[3 * k], &t.kbary[3 * k], Jw, vw);
        pos[3 * k] = p.x; pos[3 * k + 1] = p.y; pos[3 * k + 2] = p.z;
        V3 d;
        data += fit2d_joint(s, p, kp[3 * k], kp[3 * k + 1], kp[3 * k + 2], &d);
        dkp[3 * k] = d.x; dkp[3 * k + 1] = d.y; dkp[3 * k + 2] = d.z;
    }
    for (int u = 0; u < t.nu(); ++u) {
        const V3 g = kp_vertex_grad(u, t.vl_start.data(), t.vl_k.data(), t.vl_w.data(), dkp);
        gvw[3 * u] = g.x; gvw[3 * u + 1] = g.y; gvw[3 * u + 2] = g.z;
    }
    for (int j = 0; j < 23; ++j) {
        const V3 g = kp_joint_grad(j, t.jl_start.data(), t.jl_k.data(), dkp);
        dJw[3 * j] = g.x; dJw[3 * j + 1] = g.y; dJw[3 * j + 2] = g.z;
    }
    return data;
}

#if defined(__HIPCC__)
// ---- the keypoint set on the device ------------------------------------------------------------------------------------------------
struct KpSet {
    int n_kp, nr, np, K, ldb;                  // K: skinning weights per set vertex (zero-padded), ldb: row stride of B
    const int32_t *kjoint, *kref; const float* kbary;
    const int32_t *vl_start, *vl_k; const float* vl_w;
    const int32_t *jl_start, *jl_k;
    const float* vt;                           // [nr][3] template positions of the real vertices
    const int32_t* pjoint;                     // [np]
    const int32_t* wj; const float* ww;        // [nu][K]
    const int32_t *csc_start, *csc_u; const float* csc_w;      // per joint, the set vertices skinned to it (ascending)
    const float* B;                            // [496][ldb]: [posedirs ; shapedirs^T] of the set's vertices, columns 3 u + c (pseudo: Jd^T in the betas' rows)
    const float* Bt;                           // [3 nr][496]: the real vertices' columns transposed (the in-kernel backward reads along k)
    const float *Jt, *Jd;                      // the collapsed joint regressor (pseudo-vertices' rest positions)
};
constexpr int KP_NT = 1024, KP_PART = 4096;     // sixteen waves per frame: the in-kernel products are chains of L2 round trips, hidden only by waves

// One workgroup per frame.  POS: only the mapped points' positions, to pos_out [frame][n_kp][3] (fdcap_debug_keypoints3d).
// Else dX (=) prior gradients, dJw (=) the joints' 0..22 reprojection gradients, and -- a set with vertices -- dA, dPF (betas in
// columns 486..), dtransl_v, dMv, dsv (=) the vertex branch's sums for pose_bwd_kernel; losses / floss as fit2d_loss_kernel's.
// PANEL (kp_blend_by_panels): the real vertices' offsets arrive in Voff [frame][3 nu] (blend_forward) and every set vertex's
// d loss / d v_posed leaves in dVoff [frame][3 nu] for blend_backward, which then forms dPF with the betas' columns (dPF is not written
// here); else both products are plain fp32 multiply-adds here, over the real vertices' columns only (pseudo-vertices have none).
// JAW (fit2d_kp_jaw_kernel): a free jaw, jw.jaw [frame][3].  After staging, thread 0 replaces A_22 and the pose-feature block in LDS
// (PANEL: the block's nine-row share of the offsets is added here, blend_forward ran on a PF whose block is zero); in the backward
// the sum for A'_22 goes through jaw_backward: d A_22 to dA, the skinning part of d loss / d R_w to jw.R9 [frame][9] (the consumer of
// the jaw's gradient adds dPF's block -- written here or by blend_backward afterwards -- and applies Rodrigues' backward: jaw_grad),
// and Jd_22^T dJ22 is added to the betas' entries of this frame's dX row by the threads that wrote them.  The jaw prior's three terms
// join `prior` on threads XDIM .. XDIM + 2.  No float atomics.  The kernel's text is csrc/fdc_keypoints_kernel.inc, included once per form, so
// that fit2d_kp_kernel is compiled from exactly the text it had: not one instruction differs.
struct JawIO { const float* jaw; float* R9; float w[3]; };
#define FDC_KP_KERNEL fit2d_kp_kernel
#define FDC_KP_JAW 0
#include "fdc_keypoints_kernel.inc"
#undef FDC_KP_KERNEL
#undef FDC_KP_JAW
#define FDC_KP_KERNEL fit2d_kp_jaw_kernel
#define FDC_KP_JAW 1
#include "fdc_keypoints_kernel.inc"
#undef FDC_KP_KERNEL
#undef FDC_KP_JAW

// The inner fit's L-BFGS with a free jaw: 81 unknowns per frame, the row's 78 and the jaw, which lives in its own array and whose gradient
// jaw_grad completes (csrc/fdc_fit2d.h) -- the advance kernel's form with three more columns in a second array (csrc/fdc_lbfgs.h).
#define FDC_LB_KERNEL lbfgs_advance_tail_kernel
#define FDC_LB_TAIL 1
#define FDC_LB_TAIL_T JawGradIn
#define FDC_LB_TAIL_X2(t) (t).jaw
#define FDC_LB_TAIL_GRAD(t, p) jaw_grad_frame(t, p)
#include "fdc_lbfgs_advance.inc"
#undef FDC_LB_KERNEL
#undef FDC_LB_TAIL
#undef FDC_LB_TAIL_T
#undef FDC_LB_TAIL_X2
#undef FDC_LB_TAIL_GRAD

// The free expression: the same text with FDC_KP_EXPR 1, without and with the jaw (fit2d_kp_expr_kernel, fit2d_kp_expr_jaw_kernel).
// psi [frame][10] in, dpsi [frame][10] out -- complete when the kernel ends: the chain's share, the set vertices' through E (PANEL too:
// blend_backward knows nothing of psi) and the prior w^2 |psi|^2, whose ten terms join `prior` on threads XDIM + 3 .. XDIM + 12.
// E [10][lde]: per set vertex column 3 u + c the expression directions (a pseudo-vertex: JE_j's rows), JE [55 3][10]; the tree's arrays
// (parents, children, each joint's level) are the pose model's.  A map of joints 0..22 alone still stages A and M, and dA and dMv are written
// on every path: pose_bwd_kernel must be handed both.  dMv's rotation part carries sum_j dJw_j (x) Dt_j, the world joints' correction's share
// of d camera_ext, which the pose backward -- it forms d M from G_j.t + transl -- cannot know (zero at psi = 0, and without joints 0..22).
struct ExprIO {
    const float* psi; float* dpsi; float w;
    const float* E; int lde; const float* JE;
    const int *parents, *child_start, *child_list, *depth; int nlevels;
};
#define FDC_KP_EXPR 1
#define FDC_KP_KERNEL fit2d_kp_expr_kernel
#define FDC_KP_JAW 0
#include "fdc_keypoints_kernel.inc"
#undef FDC_KP_KERNEL
#undef FDC_KP_JAW
#define FDC_KP_KERNEL fit2d_kp_expr_jaw_kernel
#define FDC_KP_JAW 1
#include "fdc_keypoints_kernel.inc"
#undef FDC_KP_KERNEL
#undef FDC_KP_JAW
#undef FDC_KP_EXPR

// The inner fit's L-BFGS with free expression coefficients: 88 unknowns per frame, or 91 with the jaw -- [the row's 78 | psi 10 | jaw 3],
// the advance kernel's form with a tail of the width its argument carries.  psi's gradient is the array the data term's kernel left,
// the jaw's is completed here as in the three-column form.
struct ExprTail { float* psi; const float* dpsi; JawGradIn jg; int w; };       // w = 10, or 13 with jg.jaw
__device__ __forceinline__ float expr_tail_ld(const ExprTail& t, int p, int c) {
    return c < NEXPR ? t.psi[(size_t)p * NEXPR + c] : t.jg.jaw[(size_t)p * 3 + c - NEXPR];
}
__device__ __forceinline__ void expr_tail_st(const ExprTail& t, int p, int c, float v) {
    if (c < NEXPR) t.psi[(size_t)p * NEXPR + c] = v;
    else t.jg.jaw[(size_t)p * 3 + c - NEXPR] = v;
}
__device__ __forceinline__ float expr_tail_grad(const ExprTail& t, int p, int c) {
    if (c < NEXPR) return t.dpsi[(size_t)p * NEXPR + c];
    const V3 g = jaw_grad_frame(t.jg, p);
    return c == NEXPR ? g.x : c == NEXPR + 1 ? g.y : g.z;
}
#define FDC_LB_KERNEL lbfgs_advance_expr_kernel
#define FDC_LB_TAIL 2
#define FDC_LB_TAIL_T ExprTail
#define FDC_LB_TAIL_W(t) (t).w
#define FDC_LB_TAIL_LD(t, p, c) expr_tail_ld(t, p, c)
#define FDC_LB_TAIL_ST(t, p, c, v) expr_tail_st(t, p, c, v)
#define FDC_LB_TAIL_G(t, p, c) expr_tail_grad(t, p, c)
#include "fdc_lbfgs_advance.inc"
#undef FDC_LB_KERNEL
#undef FDC_LB_TAIL
#undef FDC_LB_TAIL_T
#undef FDC_LB_TAIL_W
#undef FDC_LB_TAIL_LD
#undef FDC_LB_TAIL_ST
#undef FDC_LB_TAIL_G
// ... and a stopped line search's starting point put back into psi (columns col0 .. col0 + 9 of the vector): launched BEFORE
// lbfgs_finalize_kernel, as lbfgs_finalize_tail_kernel is for the jaw (the vector's last three columns)
__global__ __launch_bounds__(64) void lbfgs_finalize_expr_kernel(LbfgsCfg cf, const LbfgsScalars* __restrict__ S, const float* __restrict__ W,
                                                                float* __restrict__ psi, int col0, int n) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n) return;
    const int phase = S[p].phase;
    if (phase != LB_WAIT_BRACKET && phase != LB_WAIT_ZOOM) return;
    const float* xi = W + (size_t)p * lbfgs_ws_floats(cf.hist) + (size_t)LV_XINIT * LB_DPAD;
    for (int c = 0; c < NEXPR; ++c) psi[(size_t)p * NEXPR + c] = xi[col0 + c];
}
// one Adam step of psi with the gradient an evaluation left: thread per entry
__global__ void expr_adam_kernel(float* __restrict__ psi, const float* __restrict__ dpsi, float* __restrict__ m, float* __restrict__ v, int n,
                                 AdamScalars a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) adam_update(psi[e], m[e], v[e], dpsi[e], a);
}
#endif

}  // namespace fdc
