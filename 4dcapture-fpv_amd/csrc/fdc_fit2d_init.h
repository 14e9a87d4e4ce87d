// How the inner fit starts from keypoints alone: SMPLify-X's depth guess, its camera stage, and the choice
// between a body and its twin turned 180 degrees about y.  Objective and layout: csrc/fdc_fit2d.h, csrc/fdc_keypoints.h.
//
// NOT in the reference repository (the per-frame fit is the external SMPLify-X step); restated from the published method, its
// constants being the caller's (fdcap_fit2d_init; defaults in innerfit.py), never a kernel's:
//   depth guess : z = mean_e |G_a.t - G_b.t| / mean_e |((u_a - u_b) / fx, (v_a - v_b) / fy)| over the edges e = (a, b) whose two
//                 confidences exceed conf_thr -- with fx = fy SMPLify-X's focal * height3d / height2d
//   camera stage: w_data^2 sum_{k in T, conf_k > conf_thr} [(u_k - kp_k.u)^2 + (v_k - kp_k.v)^2] + w_depth^2 (cam_t.z - z0)^2
//                 over global_orient (6D) and camera_translation alone: plain squares, no GMoF, no confidence weight but the gate
// Under the inner fit's set-up (camera_ext = I, scale = 1; world_joint, fdc_frame.h) a joint in the camera frame is
//   Jw_k = (G_0.t + transl) + R_root q_k + cam_t,      q_k = R_root0^T (G_k.t - G_0.t)
// and q_k does not depend on the two free blocks: the body model runs ONCE per stage (fit2d_camera_setup_kernel stores q_k, the
// pelvis base G_0.t + transl and z0), an evaluation is gs_forward of the row's 6D, up to eight projections and
// dR = sum_k dJ_k q_k^T through gs_backward (fit2d_camera_kernel).  Neither the pose backward nor the decoder's runs.
// The other 69 columns of the gradient row are written as exact zeros: the L-BFGS advance kernel (and Adam from zero moments)
// then forms a zero direction for them, so they keep their bits through the stage.
//
// First part: the configuration, checked on the host (plain g++ -std=c++17: tests/test_fit2d_init_cpu.py).  Second: the math as
// host / device functions.  Third: the kernels.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "fdc_fit2d.h"
#include "fdc_frame.h"
#include "fdc_math.h"

namespace fdc {

constexpr int INIT_MAX_EDGE = 4, INIT_MAX_TORSO = 8;
constexpr int CAM_SETUP_LD = 3 * INIT_MAX_TORSO + 4;          // per frame: q [8][3], the pelvis base [3], z0

// fdcap_fit2d_init with every slot resolved: a SLOT indexes the frame's keypoint array, its JOINT (0..54) the pose forward's G
struct Fit2dInit {
    int n_edge, edge[INIT_MAX_EDGE][2], edge_joint[INIT_MAX_EDGE][2];
    int n_torso, torso[INIT_MAX_TORSO], torso_joint[INIT_MAX_TORSO];
    int shoulder[2];
    float conf_thr, default_depth, side_view_px, w_data, w_depth;
};

// slot_joint [n_kp]: the joint each slot of the keypoint array is, -1 for a surface point (the 23-joint layout: slot k is joint k).
// 0, or -1 (FDCAP_E_ARG): 1..4 edges and 1..8 torso slots, every slot inside the array and on a joint, finite settings
inline int fit2d_init_build(int n_edge, const int32_t (*edge)[2], int n_torso, const int32_t* torso, const int32_t* shoulder, float conf_thr,
                            float default_depth, float side_view_px, float w_data, float w_depth, int n_kp, const int32_t* slot_joint,
                            Fit2dInit* out) {
    if (n_edge < 1 || n_edge > INIT_MAX_EDGE || n_torso < 1 || n_torso > INIT_MAX_TORSO) return -1;
    if (!std::isfinite(conf_thr) || !std::isfinite(default_depth) || !std::isfinite(side_view_px) || !std::isfinite(w_data) || !std::isfinite(w_depth))
        return -1;
    auto joint_of = [&](int32_t slot) { return slot >= 0 && slot < n_kp ? slot_joint[slot] : -1; };
    Fit2dInit t = {};
    t.n_edge = n_edge; t.n_torso = n_torso;
    for (int e = 0; e < n_edge; ++e)
        for (int i = 0; i < 2; ++i) {
            if (joint_of(edge[e][i]) < 0) return -1;
            t.edge[e][i] = edge[e][i]; t.edge_joint[e][i] = joint_of(edge[e][i]);
        }
    for (int k = 0; k < n_torso; ++k) {
        if (joint_of(torso[k]) < 0) return -1;
        t.torso[k] = torso[k]; t.torso_joint[k] = joint_of(torso[k]);
    }
    for (int i = 0; i < 2; ++i) {
        if (joint_of(shoulder[i]) < 0) return -1;
        t.shoulder[i] = shoulder[i];
    }
    t.conf_thr = conf_thr; t.default_depth = default_depth; t.side_view_px = side_view_px; t.w_data = w_data; t.w_depth = w_depth;
    *out = t;
    return 0;
}
// the same torso in the same order: what a stored set-up (q_k per torso entry) stays valid for
inline bool fit2d_init_same_torso(const Fit2dInit& a, const Fit2dInit& b) {
    if (a.n_torso != b.n_torso) return false;
    for (int k = 0; k < a.n_torso; ++k) if (a.torso[k] != b.torso[k] || a.torso_joint[k] != b.torso_joint[k]) return false;
    return true;
}

// ---- the math (host and device) ------------------------------------------------------------------------------------------------------
// One frame's depth guess.  G [55][12]: the pose forward's transforms, kp [n_kp][3] (u, v, confidence).  *valid = 0 and the default
// depth when no edge has both ends detected or the mean image length is below 1e-6.
FDC_HD float fit2d_depth_guess(const Fit2dInit& c, float fx, float fy, const float* G, const float* kp, int* valid) {
    float s3 = 0.f, s2 = 0.f;
    int cnt = 0;
    for (int e = 0; e < c.n_edge; ++e) {
        const float *ka = kp + 3 * c.edge[e][0], *kb = kp + 3 * c.edge[e][1];
        if (!(ka[2] > c.conf_thr && kb[2] > c.conf_thr)) continue;
        const V3 d = g_trn(G + 12 * c.edge_joint[e][0]) - g_trn(G + 12 * c.edge_joint[e][1]);
        const float du = (ka[0] - kb[0]) / fx, dv = (ka[1] - kb[1]) / fy;
        s3 += sqrtf(dot(d, d));
        s2 += sqrtf(du * du + dv * dv);
        ++cnt;
    }
    const float m2 = cnt > 0 ? s2 / (float)cnt : 0.f;
    if (cnt == 0 || !(m2 >= 1e-6f)) { *valid = 0; return c.default_depth; }
    *valid = 1;
    return (s3 / (float)cnt) / m2;
}
// both shoulders detected and closer than side_view_px in the image
FDC_HD int fit2d_side_view(const Fit2dInit& c, const float* kp) {
    const float *a = kp + 3 * c.shoulder[0], *b = kp + 3 * c.shoulder[1];
    if (!(a[2] > c.conf_thr && b[2] > c.conf_thr)) return 0;
    const float du = a[0] - b[0], dv = a[1] - b[1];
    return sqrtf(du * du + dv * dv) < c.side_view_px ? 1 : 0;
}

// what the camera stage keeps of the body model: torso entry k's offset from the pelvis in the root's own frame
FDC_HD V3 fit2d_camera_offset(const float* G, int joint) {
    return m3t_vec(g_rot(G), g_trn(G + 12 * joint) - g_trn(G));
}
// One torso keypoint of one evaluation: its squared residuals (0 and dJ = 0 when it is gated out), d loss / d camera-frame joint.
// base = G_0.t + transl, R = gs_forward of the row's 6D.
FDC_HD float fit2d_camera_joint(const Fit2dStage& s, const Fit2dInit& c, V3 base, const M3& R, V3 q, V3 camt, const float* kp, V3* dJ) {
    *dJ = v3(0.f, 0.f, 0.f);
    if (!(kp[2] > c.conf_thr)) return 0.f;
    const V3 J = (base + m3_vec(R, q)) + camt;
    const float iz = 1.f / J.z, w = c.w_data * c.w_data;
    const float ru = (s.fx * J.x * iz + s.cx) - kp[0], rv = (s.fy * J.y * iz + s.cy) - kp[1];
    const float du = 2.f * w * ru, dv = 2.f * w * rv;
    dJ->x = du * s.fx * iz;
    dJ->y = dv * s.fy * iz;
    dJ->z = -(du * s.fx * J.x + dv * s.fy * J.y) * iz * iz;
    return w * (ru * ru + rv * rv);
}
// The frame's sums in the torso's order: g9 = d loss / d (6D [6], camera_translation [3]), vals = {data term, depth term}
FDC_HD void fit2d_camera_reduce(const Fit2dInit& c, const GsCache& gc, const V3* dJ, const float* val, const V3* q, float camt_z, float z0,
                                float* g9, float* vals) {
    M3 dR = m3_zero();
    V3 dc = v3(0.f, 0.f, 0.f);
    float data = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < INIT_MAX_TORSO; ++k) {               // (a fixed trip count: the three arrays stay in registers)
        if (k >= c.n_torso) continue;
        m3_add_outer(dR, dJ[k], q[k]);
        dc = dc + dJ[k];
        data += val[k];
    }
    const float wz = c.w_depth * c.w_depth, rz = camt_z - z0;
    gs_backward(gc, dR, g9, 1);
    g9[6] = dc.x; g9[7] = dc.y; g9[8] = dc.z + 2.f * wz * rz;
    vals[0] = data; vals[1] = wz * rz * rz;
}
// One frame on one thread: the host twin of fit2d_camera_kernel, term for term.  setup [CAM_SETUP_LD], x [78], kp [n_kp][3].
FDC_HD float fit2d_camera_frame(const Fit2dStage& s, const Fit2dInit& c, const float* setup, const float* x, const float* kp, float* g9) {
    GsCache gc;
    const M3 R = gs_forward(x + X_SIXD, 1, &gc);
    const V3 base = v3(setup[3 * INIT_MAX_TORSO], setup[3 * INIT_MAX_TORSO + 1], setup[3 * INIT_MAX_TORSO + 2]);
    const V3 camt = v3(x[X_CAMT], x[X_CAMT + 1], x[X_CAMT + 2]);
    V3 dJ[INIT_MAX_TORSO], q[INIT_MAX_TORSO];
    float val[INIT_MAX_TORSO], vals[2];
    for (int k = 0; k < c.n_torso; ++k) {
        q[k] = v3(setup[3 * k], setup[3 * k + 1], setup[3 * k + 2]);
        val[k] = fit2d_camera_joint(s, c, base, R, q[k], camt, kp + 3 * c.torso[k], &dJ[k]);
    }
    fit2d_camera_reduce(c, gc, dJ, val, q, camt.z, setup[3 * INIT_MAX_TORSO + 3], g9, vals);
    return vals[0] + vals[1];
}

// global_orient turned 180 degrees about the body's y: log(R(aa) R_y(pi)).  R_y(pi) = diag(-1, 1, -1) negates columns 0 and 2.
FDC_HD V3 fit2d_flip_orient(V3 aa) {
    M3 R = rodrigues_forward(aa);
    for (int r = 0; r < 3; ++r) { R.m[3 * r] = -R.m[3 * r]; R.m[3 * r + 2] = -R.m[3 * r + 2]; }
    return tgm_rotmat_to_aa(R);
}
// the twin is taken iff its loss is strictly lower; a NaN loss counts as +inf (both NaN: the first stays).  NaN is read from the
// bits: the library is built with -fno-honor-nans, under which x != x is folded away
FDC_HD float fit2d_nan_as_inf(float x) {
    uint32_t u;
    memcpy(&u, &x, sizeof u);
    return (u & 0x7fffffffu) > 0x7f800000u ? INFINITY : x;
}
FDC_HD int fit2d_select_twin(float loss_first, float loss_twin) {
    return fit2d_nan_as_inf(loss_twin) < fit2d_nan_as_inf(loss_first) ? 1 : 0;
}

#if defined(__HIPCC__)
// entry i of a list of the kernel's argument, i a lane's index: a chain of selects over the argument registers (indexing the
// argument by a lane's value would copy the struct to scratch memory)
__device__ __forceinline__ int init_pick(const int (&a)[INIT_MAX_TORSO], int i) {
    int v = a[0];
#pragma unroll
    for (int k = 1; k < INIT_MAX_TORSO; ++k) v = i == k ? a[k] : v;
    return v;
}

// thread per frame: the depth guess into the row's camera_translation (0, 0, z) -- nothing else of the row is written -- and the
// three per-frame outputs (each optional)
__global__ __launch_bounds__(64) void fit2d_guess_kernel(Fit2dInit c, float fx, float fy, const float* __restrict__ G, const float* __restrict__ kp,
                                                         int n_kp, int row0, int n, float* __restrict__ X, float* __restrict__ z_out,
                                                         int* __restrict__ valid_out, int* __restrict__ side_out) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    const float* k = kp + (size_t)f * n_kp * 3;
    int valid;
    const float z = fit2d_depth_guess(c, fx, fy, G + (size_t)(row0 + f) * NJ * 12, k, &valid);
    float* x = X + (size_t)(row0 + f) * XDIM + X_CAMT;
    x[0] = 0.f; x[1] = 0.f; x[2] = z;
    if (z_out) z_out[f] = z;
    if (valid_out) valid_out[f] = valid;
    if (side_out) side_out[f] = fit2d_side_view(c, k);
}

// wave per frame, after one pose forward: lane k < n_torso its q_k, lane 0 the pelvis base and z0
__global__ __launch_bounds__(64) void fit2d_camera_setup_kernel(Fit2dInit c, const float* __restrict__ X, const float* __restrict__ G, int row0,
                                                                float* __restrict__ setup) {
    const int tid = threadIdx.x, r = row0 + blockIdx.x;
    const float* g = G + (size_t)r * NJ * 12;
    const float* x = X + (size_t)r * XDIM;
    float* o = setup + (size_t)blockIdx.x * CAM_SETUP_LD;
    if (tid < INIT_MAX_TORSO) {
        const V3 q = tid < c.n_torso ? fit2d_camera_offset(g, init_pick(c.torso_joint, tid)) : v3(0.f, 0.f, 0.f);
        o[3 * tid] = q.x; o[3 * tid + 1] = q.y; o[3 * tid + 2] = q.z;
    }
    if (tid == 0) {
        const V3 b = g_trn(g) + v3(x[X_TRANSL], x[X_TRANSL + 1], x[X_TRANSL + 2]);
        o[3 * INIT_MAX_TORSO] = b.x; o[3 * INIT_MAX_TORSO + 1] = b.y; o[3 * INIT_MAX_TORSO + 2] = b.z;
        o[3 * INIT_MAX_TORSO + 3] = x[X_CAMT + 2];
    }
}

// wave per frame, one evaluation of the camera stage: lane k < n_torso projects its keypoint, lane 0 adds the terms in the torso's
// order (no atomics on floats) and runs the 6D backward, then the wave writes the WHOLE gradient row: nine columns, 69 exact zeros.
// losses (optional, logging): [0] += data term, [1] += depth term; floss [frame] = their sum.
__global__ __launch_bounds__(64) void fit2d_camera_kernel(Fit2dStage s, Fit2dInit c, const float* __restrict__ X, const float* __restrict__ setup,
                                                          const float* __restrict__ kp, int n_kp, int row0, float* __restrict__ dX,
                                                          double* __restrict__ losses, float* __restrict__ floss) {
    __shared__ float s_dj[INIT_MAX_TORSO][3], s_q[INIT_MAX_TORSO][3], s_val[INIT_MAX_TORSO], s_g9[9];
    const int tid = threadIdx.x, r = row0 + blockIdx.x;
    const float* x = X + (size_t)r * XDIM;
    const float* su = setup + (size_t)blockIdx.x * CAM_SETUP_LD;
    GsCache gc;
    const M3 R = gs_forward(x + X_SIXD, 1, &gc);
    const float camt_z = x[X_CAMT + 2];
    if (tid < c.n_torso) {
        const int slot = init_pick(c.torso, tid);
        const V3 q = v3(su[3 * tid], su[3 * tid + 1], su[3 * tid + 2]);
        const V3 base = v3(su[3 * INIT_MAX_TORSO], su[3 * INIT_MAX_TORSO + 1], su[3 * INIT_MAX_TORSO + 2]);
        V3 dJ;
        s_val[tid] = fit2d_camera_joint(s, c, base, R, q, v3(x[X_CAMT], x[X_CAMT + 1], camt_z), kp + ((size_t)blockIdx.x * n_kp + slot) * 3, &dJ);
        s_dj[tid][0] = dJ.x; s_dj[tid][1] = dJ.y; s_dj[tid][2] = dJ.z;
        s_q[tid][0] = q.x; s_q[tid][1] = q.y; s_q[tid][2] = q.z;
    }
    __syncthreads();
    if (tid == 0) {
        V3 dJ[INIT_MAX_TORSO], q[INIT_MAX_TORSO];
        float val[INIT_MAX_TORSO], g9[9], vals[2];
#pragma unroll
        for (int k = 0; k < INIT_MAX_TORSO; ++k) {
            const bool on = k < c.n_torso;                  // (the entries above were never written)
            dJ[k] = on ? v3(s_dj[k][0], s_dj[k][1], s_dj[k][2]) : v3(0.f, 0.f, 0.f);
            q[k] = on ? v3(s_q[k][0], s_q[k][1], s_q[k][2]) : v3(0.f, 0.f, 0.f);
            val[k] = on ? s_val[k] : 0.f;
        }
        fit2d_camera_reduce(c, gc, dJ, val, q, camt_z, su[3 * INIT_MAX_TORSO + 3], g9, vals);
        for (int e = 0; e < 9; ++e) s_g9[e] = g9[e];
        if (floss) floss[blockIdx.x] = vals[0] + vals[1];
        if (losses) { atomicAdd(&losses[0], (double)vals[0]); atomicAdd(&losses[1], (double)vals[1]); }
    }
    __syncthreads();
    for (int e = tid; e < XDIM; e += 64) {
        float g = 0.f;
        if (e >= X_SIXD && e < X_SIXD + 6) g = s_g9[e - X_SIXD];
        else if (e >= X_CAMT) g = s_g9[6 + e - X_CAMT];
        dX[(size_t)r * XDIM + e] = g;
    }
}

// thread per row of [n, 75]: global_orient (columns 3..5) turned 180 degrees about y, in place
__global__ __launch_bounds__(64) void fit2d_flip_kernel(float* __restrict__ rows75, int n) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    float* p = rows75 + (size_t)f * 75 + 3;
    const V3 a = fit2d_flip_orient(v3(p[0], p[1], p[2]));
    p[0] = a.x; p[1] = a.y; p[2] = a.z;
}

// block per frame f < n: its twin is problem n + i with src[i] == f (src ascending and unique: a binary search whose result never
// indexes anything but src [m] and problems n .. n + m - 1); the chosen problem's row (and jaw) is copied, element per thread
__global__ __launch_bounds__(128) void fit2d_select_kernel(const float* __restrict__ rows, const float* __restrict__ loss, const int* __restrict__ src,
                                                           int n, int m, const float* __restrict__ jaw, float* __restrict__ rows_out,
                                                           float* __restrict__ jaw_out, int* __restrict__ chosen) {
    const int f = blockIdx.x, tid = threadIdx.x;
    int lo = 0, hi = m;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (src[mid] < f) lo = mid + 1; else hi = mid; }
    const bool twin = lo < m && src[lo] == f && fit2d_select_twin(loss[f], loss[n + lo]);
    const int p = twin ? n + lo : f;
    if (tid < 75) rows_out[(size_t)f * 75 + tid] = rows[(size_t)p * 75 + tid];
    if (jaw && jaw_out && tid >= 96 && tid < 99) jaw_out[(size_t)f * 3 + tid - 96] = jaw[(size_t)p * 3 + tid - 96];
    if (chosen && tid == 0) chosen[f] = twin ? 1 : 0;
}
#endif

}  // namespace fdc
