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
template <bool POS, bool PANEL>
__global__ __launch_bounds__(KP_NT) void fit2d_kp_kernel(Fit2dStage s, KpSet ks, const float* __restrict__ X, const float* __restrict__ PF,
                                                         const float* __restrict__ A, const float* __restrict__ M,
                                                         const float* __restrict__ scale, const float* __restrict__ Jw,
                                                         const float* __restrict__ kp, int row0, float* __restrict__ dX,
                                                         float* __restrict__ dJw, float* __restrict__ dA, float* __restrict__ dPF,
                                                         float* __restrict__ dtransl_v, float* __restrict__ dMv, float* __restrict__ dsv,
                                                         double* __restrict__ losses, float* __restrict__ floss, float* __restrict__ pos_out,
                                                         const float* __restrict__ Voff, float* __restrict__ dVoff) {
    __shared__ float s_x[XDIM + 2], s_pf[NPFX], s_A[NJ * 12], s_M[12], s_jw[NJW * 3 + 3], s_kp[KP_MAX * 3], s_dk[KP_MAX * 3];
    __shared__ float s_v[KP_MAXV * 3];         // pose + shape offsets of the real vertices, later every set vertex's d loss / d v_posed
    __shared__ float s_vp[KP_MAXV * 3], s_vb[KP_MAXV * 3], s_vw[KP_MAXV * 3], s_gv[KP_MAXV * 3];   // (s_vw: positions, later their gradients)
    __shared__ float s_part[KP_PART];
    __shared__ float s_red[16][16], s_sred[4][2], s_db[NBETA];
    const int tid = threadIdx.x, r = row0 + blockIdx.x;
    const int nr = ks.nr, nu = ks.nr + ks.np, nkp = ks.n_kp, ncol = 3 * ks.nr;
    // everything of this frame, requested in one batch in front of the first barrier
    for (int e = tid; e < XDIM; e += KP_NT) s_x[e] = X[(size_t)r * XDIM + e];
    for (int e = tid; e < NJW * 3; e += KP_NT) s_jw[e] = Jw[(size_t)r * NJW * 3 + e];
    if (!POS) for (int e = tid; e < nkp * 3; e += KP_NT) s_kp[e] = kp[(size_t)blockIdx.x * nkp * 3 + e];
    if (nu > 0) {
        for (int e = tid; e < NPFX; e += KP_NT) s_pf[e] = PF[(size_t)r * NPFX + e];
        for (int e = tid; e < NJ * 12; e += KP_NT) s_A[e] = A[(size_t)r * NJ * 12 + e];
        if (tid < 12) s_M[tid] = M[(size_t)r * 12 + tid];
        if (PANEL) for (int e = tid; e < ncol; e += KP_NT) s_v[e] = Voff[(size_t)blockIdx.x * 3 * nu + e];
    }
    const float sc = scale[0];
    __syncthreads();
    // pose + shape offsets of the real vertices: s_v[c] = sum_k pf[k] B[k][c], K split over as many parts as the workspace holds
    if (!PANEL && ncol > 0) {
        const int nparts = min(16, KP_PART / ncol), kper = (NPFX + nparts - 1) / nparts;
        for (int w = tid; w < nparts * ncol; w += KP_NT) {
            const int p = w / ncol, c = w - p * ncol, k1 = min(NPFX, (p + 1) * kper);
            float acc = 0.f;
#pragma unroll 8
            for (int k = p * kper; k < k1; ++k) acc += s_pf[k] * ks.B[(size_t)k * ks.ldb + c];
            s_part[w] = acc;
        }
        __syncthreads();
        for (int c = tid; c < ncol; c += KP_NT) {
            float acc = s_part[c];
            for (int p = 1; p < nparts; ++p) acc += s_part[p * ncol + c];
            s_v[c] = acc;
        }
        __syncthreads();
    }
    const V3 transl = v3(s_x[X_TRANSL], s_x[X_TRANSL + 1], s_x[X_TRANSL + 2]);
    // v_posed of a set vertex and its skinning transform T = sum_k w_k A_{j_k}
    auto vertex_posed = [&](int u) {
        if (u < nr) return v3(ks.vt[3 * u] + s_v[3 * u], ks.vt[3 * u + 1] + s_v[3 * u + 1], ks.vt[3 * u + 2] + s_v[3 * u + 2]);
        const int j = ks.pjoint[u - nr];
        float p[3];
        for (int c = 0; c < 3; ++c) {                      // (pose_forward's joint_rest, term for term)
            float acc = ks.Jt[3 * j + c];
            for (int l = 0; l < NBETA; ++l) acc += ks.Jd[(3 * j + c) * NBETA + l] * s_x[X_BETAS + l];
            p[c] = acc;
        }
        return v3(p[0], p[1], p[2]);
    };
    auto vertex_T = [&](int u, float* T) {
        for (int e = 0; e < 12; ++e) T[e] = 0.f;
        for (int k = 0; k < ks.K; ++k) {
            const float w = ks.ww[(size_t)u * ks.K + k];
            const float* a = s_A + 12 * ks.wj[(size_t)u * ks.K + k];
            for (int e = 0; e < 12; ++e) T[e] += w * a[e];
        }
    };
    for (int u = tid; u < nu; u += KP_NT) {
        const V3 p = vertex_posed(u);
        float T[12];
        vertex_T(u, T);
        const V3 vb = v3(T[0] * p.x + T[1] * p.y + T[2] * p.z + T[3], T[4] * p.x + T[5] * p.y + T[6] * p.z + T[7],
                         T[8] * p.x + T[9] * p.y + T[10] * p.z + T[11]) + transl;
        const V3 vw = skin_world_vertex(vb, sc, s_M);
        s_vp[3 * u] = p.x; s_vp[3 * u + 1] = p.y; s_vp[3 * u + 2] = p.z;
        s_vb[3 * u] = vb.x; s_vb[3 * u + 1] = vb.y; s_vb[3 * u + 2] = vb.z;
        s_vw[3 * u] = vw.x; s_vw[3 * u + 1] = vw.y; s_vw[3 * u + 2] = vw.z;
    }
    __syncthreads();
    // keypoint tid: position, data term, d loss / d position -- fit2d_loss_kernel's thread for thread (and its sums' order)
    float data = 0.f, prior = 0.f;
    if (tid < nkp) {
        const V3 p = kp_position(ks.kjoint[tid], ks.kref + 3 * tid, ks.kbary + 3 * tid, s_jw, s_vw);
        if (POS) {
            float* o = pos_out + ((size_t)blockIdx.x * nkp + tid) * 3;
            o[0] = p.x; o[1] = p.y; o[2] = p.z;
        } else {
            V3 dJ;
            data = fit2d_joint(s, p, s_kp[3 * tid], s_kp[3 * tid + 1], s_kp[3 * tid + 2], &dJ);
            s_dk[3 * tid] = dJ.x; s_dk[3 * tid + 1] = dJ.y; s_dk[3 * tid + 2] = dJ.z;
        }
    }
    if (POS) return;
    if (tid < XDIM) dX[(size_t)r * XDIM + tid] = fit2d_prior_grad(s, tid, s_x[tid], &prior);
    if (losses || floss) {
        float vals[2] = {data, prior};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float v = vals[i];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((tid & 63) == 0 && tid < 256) s_sred[tid >> 6][i] = v;         // (keypoints and parameters sit in the first four waves)
        }
    }
    __syncthreads();
    if (floss && tid == 0)
        floss[blockIdx.x] = ((s_sred[0][0] + s_sred[1][0]) + (s_sred[2][0] + s_sred[3][0])) + ((s_sred[0][1] + s_sred[1][1]) + (s_sred[2][1] + s_sred[3][1]));
    if (losses && tid < 2) atomicAdd(&losses[tid], (double)((s_sred[0][tid] + s_sred[1][tid]) + (s_sred[2][tid] + s_sred[3][tid])));
    if (tid < NJW) {
        const V3 g = kp_joint_grad(tid, ks.jl_start, ks.jl_k, s_dk);
        float* o = dJw + ((size_t)r * NJW + tid) * 3;
        o[0] = g.x; o[1] = g.y; o[2] = g.z;
    }
    if (nu == 0) return;                                   // (kernel-uniform: no vertex branch, nothing else is written or read)
    // set vertex u: its position's gradient from its list, back through the world transform and the skinning
    for (int u = tid; u < nu; u += KP_NT) {
        const V3 g = kp_vertex_grad(u, ks.vl_start, ks.vl_k, ks.vl_w, s_dk);
        SkinFwd f;
        f.vp = v3(s_vp[3 * u], s_vp[3 * u + 1], s_vp[3 * u + 2]);
        f.vb = v3(s_vb[3 * u], s_vb[3 * u + 1], s_vb[3 * u + 2]);
        vertex_T(u, f.T);
        const SkinBwd b = skin_backward_vertex(f, s_M, sc, g);
        s_vw[3 * u] = g.x; s_vw[3 * u + 1] = g.y; s_vw[3 * u + 2] = g.z;
        s_gv[3 * u] = b.gv.x; s_gv[3 * u + 1] = b.gv.y; s_gv[3 * u + 2] = b.gv.z;
        s_v[3 * u] = b.dvp.x; s_v[3 * u + 1] = b.dvp.y; s_v[3 * u + 2] = b.dvp.z;
    }
    __syncthreads();
    // dA_j = sum over the vertices skinned to j, ascending, of w dT,  dT = gv (x) [v_posed; 1] (skin_backward_vertex's dT, formed here)
    for (int it = tid; it < NJ * 12; it += KP_NT) {
        const int j = it / 12, e = it - 12 * j, i = e >> 2, c = e & 3;
        float acc = 0.f;
        for (int q = ks.csc_start[j]; q < ks.csc_start[j + 1]; ++q) {
            const int u = ks.csc_u[q];
            acc += ks.csc_w[q] * (c < 3 ? s_gv[3 * u + i] * s_vp[3 * u + c] : s_gv[3 * u + i]);
        }
        dA[(size_t)r * NJ * 12 + it] = acc;
    }
    // the sixteen per-frame sums over the set's vertices -- dM [12], d scale, d transl [3] (skin_backward_vertex's dM, ds, gv) -- in two
    // steps: sixteen partial sums over u = part, part + 16, .. each, then those in order
    if (tid < 256) {
        const int o = tid & 15, part = tid >> 4;
        float acc = 0.f;
        for (int u = part; u < nu; u += 16) {
            const V3 g = v3(s_vw[3 * u], s_vw[3 * u + 1], s_vw[3 * u + 2]), vb = v3(s_vb[3 * u], s_vb[3 * u + 1], s_vb[3 * u + 2]);
            if (o < 12) {
                const int i = o >> 2, c = o & 3;
                const float gi = i == 0 ? g.x : i == 1 ? g.y : g.z;
                const V3 sv = sc * vb;
                acc += c == 0 ? gi * sv.x : c == 1 ? gi * sv.y : c == 2 ? gi * sv.z : gi;
            } else if (o == 12) {
                const V3 gs = v3(s_M[0] * g.x + s_M[4] * g.y + s_M[8] * g.z, s_M[1] * g.x + s_M[5] * g.y + s_M[9] * g.z,
                                 s_M[2] * g.x + s_M[6] * g.y + s_M[10] * g.z);
                acc += dot(gs, vb);
            } else
                acc += s_gv[3 * u + o - 13];
        }
        s_red[part][o] = acc;
    }
    if (PANEL) {                                           // the products' share is blend_backward's
        for (int e = tid; e < 3 * nu; e += KP_NT) dVoff[(size_t)blockIdx.x * 3 * nu + e] = s_v[e];
        __syncthreads();
    } else {
    // d betas through the pseudo-vertices' rest positions: Jd^T d v_posed, pseudo-vertices ascending
    if (tid >= 256 && tid < 256 + NBETA) {
        const int b = tid - 256;
        float acc = 0.f;
        for (int u = nr; u < nu; ++u) {
            const int j = ks.pjoint[u - nr];
            for (int c = 0; c < 3; ++c) acc += ks.Jd[(3 * j + c) * NBETA + b] * s_v[3 * u + c];
        }
        s_db[b] = acc;
    }
    // dPF[k] = sum_c Bt[c][k] d v_posed[c] over the real vertices' columns, in eight parts
    constexpr int BP = 8;
    static_assert(BP * NPFX <= KP_PART, "the workspace holds the backward's partial sums");
    const int cper = (ncol + BP - 1) / BP;
    for (int w = tid; w < BP * NPFX; w += KP_NT) {
        const int p = w / NPFX, k = w - p * NPFX, c1 = min(ncol, (p + 1) * cper);
        float acc = 0.f;
#pragma unroll 8
        for (int c = p * cper; c < c1; ++c) acc += ks.Bt[(size_t)c * NPFX + k] * s_v[c];
        s_part[w] = acc;
    }
    __syncthreads();
    for (int k = tid; k < NPFX; k += KP_NT) {
        float acc = ((s_part[k] + s_part[NPFX + k]) + (s_part[2 * NPFX + k] + s_part[3 * NPFX + k])) +
                    ((s_part[4 * NPFX + k] + s_part[5 * NPFX + k]) + (s_part[6 * NPFX + k] + s_part[7 * NPFX + k]));
        if (k >= NPF) acc += s_db[k - NPF];
        dPF[(size_t)r * NPFX + k] = acc;
    }
    }
    if (tid < 16) {
        float acc = s_red[0][tid];
        for (int p = 1; p < 16; ++p) acc += s_red[p][tid];
        if (tid < 12) dMv[(size_t)r * 12 + tid] = acc;
        else if (tid == 12) dsv[r] = acc;
        else dtransl_v[(size_t)r * 3 + tid - 13] = acc;
    }
}
#endif

}  // namespace fdc
