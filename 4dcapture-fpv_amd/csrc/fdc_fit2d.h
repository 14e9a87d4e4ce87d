// Per-frame inner fit with a true 2D-keypoint reprojection residual (BASELINE config 4).
//
// NOT in the reference repository: the per-frame fit is the external SMPLify-X step (/root/reference/README.md:14-17;
// the only 2D projection in-repo is a viewer overlay, local_vis.py:368-378, with the fixed pinhole intrinsics
// fx = fy = 692, cx = 640, cy = 360 of vis.py:358-360).  Restated from the published SMPLify-X objective:
//   data  : w_data^2 * sum_j conf_j^2 * [ GMoF_rho(u_j - kp_j.u) + GMoF_rho(v_j - kp_j.v) ],   GMoF_rho(r) = rho^2 r^2 / (r^2 + rho^2)
//   priors: w_pose^2 * |z|^2 (VPoser latent) + w_shape^2 * |betas|^2 + w_hand^2 * (|lh|^2 + |rh|^2)
// on the camera-frame joints J_j = SMPL-X(VPoser(z)) joint j + transl + camera_translation (the optimiser's
// body2world with camera_ext = I and scale = 1), projected u = fx X / Z + cx, v = fy Y / Z + cy.
// Frames are independent problems (no temporal term), so one launch covers a whole batch of frames.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "fdc_frame.h"
#include "fdc_loss.h"
#include "fdc_math.h"

namespace fdc {

struct Fit2dStage { float fx, fy, cx, cy, rho, w_data, w_pose, w_shape, w_hand; };

// value and derivative of GMoF_rho at residual r
FDC_HD float gmof(float r, float rho2, float* dg) {
    float r2 = r * r, den = r2 + rho2;
    *dg = 2.f * r * rho2 * rho2 / (den * den);
    return rho2 * r2 / den;
}

// One joint of one frame: camera-frame joint J, keypoint (u, v, conf) -> d loss / d J and the joint's data term.
FDC_HD float fit2d_joint(const Fit2dStage& s, V3 J, float ku, float kv, float conf, V3* dJ) {
    const float iz = 1.f / J.z;
    const float u = s.fx * J.x * iz + s.cx, v = s.fy * J.y * iz + s.cy;
    const float w = s.w_data * s.w_data * conf * conf;
    float dgu, dgv;
    const float gu = gmof(ku - u, s.rho * s.rho, &dgu), gv = gmof(kv - v, s.rho * s.rho, &dgv);
    const float du = -w * dgu, dv = -w * dgv;                  // d loss / d u, d v  (residual = keypoint - projection)
    dJ->x = du * s.fx * iz;
    dJ->y = dv * s.fy * iz;
    dJ->z = -(du * s.fx * J.x + dv * s.fy * J.y) * iz * iz;
    return w * (gu + gv);
}

// ---- the clip-level fit's reprojection term (fdcap_opt_set_reproj) --------------------------------------------
//   weight / (23 N) * sum_ij conf_ij^2 [ GMoF_rho(k^u_ij - u_ij) + GMoF_rho(k^v_ij - v_ij) ]   on   p_ij = G_ij.t + transl_i + cam_t_i
// the frame SMPLify-X fitted in: no `scale`, no camera_ext.  kp: this rank's rows [n_local][23][3] (u, v, conf); wn = weight / (23 N);
// loss_rows: a logging backward's per-frame partials (slot 6, un-normalised: without wn), else null.
struct ReprojIn { const float* kp; float fx, fy, cx, cy, rho, wn; float* loss_rows; };
// The term's joint: fit2d_joint at w_data = 1, with an undetected keypoint (conf == 0) skipped -- its value and gradient are exact
// zeros whatever its coordinates hold (NaN included) and whatever J.z is.  The inner fit's callers keep fit2d_joint as it is.
FDC_HD float reproj_joint(const ReprojIn& rp, V3 J, float ku, float kv, float conf, V3* dJ) {
    if (conf == 0.f) {
        dJ->x = dJ->y = dJ->z = 0.f;
        return 0.f;
    }
    const Fit2dStage s = {rp.fx, rp.fy, rp.cx, rp.cy, rp.rho, 1.f, 0.f, 0.f, 0.f};
    const float val = fit2d_joint(s, J, ku, kv, conf, dJ);
    dJ->x *= rp.wn; dJ->y *= rp.wn; dJ->z *= rp.wn;           // (the gradient carries the normalisation, the logged partial does not)
    return val;
}
// 0, or -1 (FDCAP_E_ARG): a non-finite or non-positive focal length or rho, a non-finite or negative weight
// (finite by the exponent's bits: the library is built with -fno-honor-nans, under which a floating-point test for NaN may be folded away)
inline bool reproj_finite(float v) {
    uint32_t u;
    memcpy(&u, &v, sizeof(u));
    return (u & 0x7f800000u) != 0x7f800000u;
}
inline int reproj_params_check(float fx, float fy, float cx, float cy, float rho, float weight) {
    if (!reproj_finite(fx) || !reproj_finite(fy) || !reproj_finite(rho) || !reproj_finite(cx) || !reproj_finite(cy) || !reproj_finite(weight)) return -1;
    if (!(fx > 0.f) || !(fy > 0.f) || !(rho > 0.f) || weight < 0.f) return -1;
    return 0;
}

// gradient of the L2 priors on element e of the 78-d row
FDC_HD float fit2d_prior_grad(const Fit2dStage& s, int e, float x, float* val) {
    float w = 0.f;
    if (e >= X_LATENT && e < X_LATENT + 32) w = s.w_pose * s.w_pose;
    else if (e >= X_BETAS && e < X_BETAS + NBETA) w = s.w_shape * s.w_shape;
    else if (e >= X_LH && e < X_CAMT) w = s.w_hand * s.w_hand;
    *val = w * x * x;
    return 2.f * w * x;
}

// ---- SMPLify-X's bending prior on the body joints (its angle prior: elbows and knees must not bend backwards) ----------------------
//   w_bend * sum_t exp(sign_t * aa_{joint_t}[axis_t])^2,   aa_j = tgm_rotmat_to_aa(R_j)
// R_j: the local rotation of body joint j in 1..21 as the pose chain uses it (Gram-Schmidt of the decoder's output; pose feature
// block j + I), aa_j what the reference's vposer.decode(z, 'aa') returns for it.  The terms are the caller's (fdcap_fit2d_extra);
// w_bend enters as it is, not squared.
constexpr int FIT2D_MAX_BEND = 8;
struct Fit2dBend { float w; int n; int joint[FIT2D_MAX_BEND], axis[FIT2D_MAX_BEND]; float sign[FIT2D_MAX_BEND]; };
// 0, or -1 (FDCAP_E_ARG): more than FIT2D_MAX_BEND terms, a joint outside 1..21, an axis outside 0..2, a non-finite weight or sign
inline int fit2d_bend_check(float w, int n, const int32_t* joint, const int32_t* axis, const float* sign) {
    if (n < 0 || n > FIT2D_MAX_BEND || !std::isfinite(w)) return -1;
    for (int t = 0; t < n; ++t)
        if (joint[t] < 1 || joint[t] > 21 || axis[t] < 0 || axis[t] > 2 || !std::isfinite(sign[t])) return -1;
    return 0;
}
// One term: its value, and d value / d R (row-major) -- an addend to joint j's block of d loss / d pose feature (PF_j = R_j - I), which
// the pose backward carries on through its Gram-Schmidt backward.  That Jacobian maps into the tangent space of the rotations, so how
// the log map's formula continues off the manifold does not matter.
FDC_HD float fit2d_bend_term(float w, int axis, float sign, const M3& R, M3* dR) {
    const V3 aa = tgm_rotmat_to_aa(R);
    const float a = axis == 0 ? aa.x : axis == 1 ? aa.y : aa.z;
    const float e = expf(sign * a);
    const float val = w * (e * e);
    const float g = 2.f * sign * val;
    *dR = tgm_rotmat_to_aa_backward(R, v3(axis == 0 ? g : 0.f, axis == 1 ? g : 0.f, axis == 2 ? g : 0.f));
    return val;
}
// R_j from a frame's pose-feature row
FDC_HD M3 fit2d_joint_rotation(const float* pf, int j) {
    M3 R;
    for (int e = 0; e < 9; ++e) R.m[e] = pf[9 * (j - 1) + e] + ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
    return R;
}

// ---- the free jaw's prior and gradient (the model: csrc/fdc_keypoints.h) ------------------------------------------------------------
//   sum_c (w_jaw[c] * jaw[c])^2
// d objective / d jaw of one frame: d loss / d R_w -- the skinning part fit2d_kp_jaw_kernel left in R9 [9] plus the pose-feature block's
// gradient gP [9] (dPF columns 9 (22 - 1) .., written by that kernel or by blend_backward after it; nullptr: no vertex follows the
// jaw) -- through Rodrigues' backward, plus the prior's.  Whoever consumes the gradient calls this: the L-BFGS advance kernel, the
// Adam step, fdcap_opt_get_jaw.
FDC_HD V3 jaw_grad(V3 w, const float* R9, const float* gP, const float* w_jaw) {
    M3 d;
    for (int e = 0; e < 9; ++e) d.m[e] = R9[e] + (gP ? gP[e] : 0.f);
    V3 g = rodrigues_backward(w, d);
    g.x += 2.f * w_jaw[0] * w_jaw[0] * w.x; g.y += 2.f * w_jaw[1] * w_jaw[1] * w.y; g.z += 2.f * w_jaw[2] * w_jaw[2] * w.z;
    return g;
}
// where a frame's jaw, its gradient's two parts and the prior's weights are (device pointers; jaw == nullptr: no free jaw)
struct JawGradIn { float* jaw = nullptr; const float* R9 = nullptr; const float* gP = nullptr; size_t gp_stride = 0; float w[3] = {0.f, 0.f, 0.f}; };

#if defined(__HIPCC__)
__device__ __forceinline__ V3 jaw_grad_frame(const JawGradIn& jg, int f) {
    const float wj[3] = {jg.w[0], jg.w[1], jg.w[2]};
    const float* w = jg.jaw + (size_t)f * 3;
    return jaw_grad(v3(w[0], w[1], w[2]), jg.R9 + (size_t)f * 9, jg.gP ? jg.gP + (size_t)f * jg.gp_stride : nullptr, wj);
}
// thread per frame: djaw [n][3] (=) the gradient (fdcap_opt_get_jaw), or -- m != nullptr -- one Adam step of the jaw with moments m, v
__global__ void jaw_grad_kernel(JawGradIn jg, int n, float* __restrict__ djaw, float* __restrict__ m, float* __restrict__ v, AdamScalars a) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const V3 g = jaw_grad_frame(jg, f);
    const float gg[3] = {g.x, g.y, g.z};
    for (int c = 0; c < 3; ++c) {
        if (djaw) djaw[(size_t)f * 3 + c] = gg[c];
        if (m) adam_update(jg.jaw[(size_t)f * 3 + c], m[(size_t)f * 3 + c], v[(size_t)f * 3 + c], gg[c], a);
    }
}

// The bending prior of every frame: one small launch between the data term (and, with a keypoint set, its blend backward) and
// pose_bwd_kernel, on every path of the inner fit -- the route that leaves fit2d_kp_kernel, the panel products and the pose kernels as
// they are.  One wave per frame; lane t forms term t, the first nine lanes add the terms' gradients in the list's order (two terms
// may name one joint): no float atomics.
// ADD: dPF holds the vertex branch's sums (written by fit2d_kp_kernel or blend_backward) and the terms are added to their joints'
// blocks; else nothing has written dPF (no vertex branch) and the whole row is assigned: zero but for the terms' blocks (d betas,
// columns NPF.., are not handed to the pose backward on that path).
// losses[1] += the frames' priors, floss[frame] += this frame's (both optional, as fit2d_loss_kernel's).
template <bool ADD>
__global__ __launch_bounds__(64) void fit2d_bend_kernel(Fit2dBend b, const float* __restrict__ PF, int row0, float* __restrict__ dPF,
                                                        double* __restrict__ losses, float* __restrict__ floss) {
    __shared__ float s_dr[FIT2D_MAX_BEND][9], s_val[FIT2D_MAX_BEND], s_sign[FIT2D_MAX_BEND];
    __shared__ int s_joint[FIT2D_MAX_BEND], s_axis[FIT2D_MAX_BEND];
    const int tid = threadIdx.x, r = row0 + blockIdx.x;
    float* const drow = dPF + (size_t)r * NPFX;
    if (tid == 0) {                                          // (the list by a lane's index: from LDS, not from the argument registers)
#pragma unroll
        for (int t = 0; t < FIT2D_MAX_BEND; ++t) { s_joint[t] = b.joint[t]; s_axis[t] = b.axis[t]; s_sign[t] = b.sign[t]; }
    }
    if (!ADD) for (int e = tid; e < NPFX; e += 64) drow[e] = 0.f;
    __syncthreads();
    if (tid < b.n) {
        M3 dR;
        s_val[tid] = fit2d_bend_term(b.w, s_axis[tid], s_sign[tid], fit2d_joint_rotation(PF + (size_t)r * NPFX, s_joint[tid]), &dR);
        for (int e = 0; e < 9; ++e) s_dr[tid][e] = dR.m[e];
    }
    __syncthreads();
    if (tid < 9)
        for (int t = 0; t < b.n; ++t) drow[9 * (s_joint[t] - 1) + tid] += s_dr[t][tid];
    if (tid == 0 && (losses || floss)) {
        float sum = s_val[0];
        for (int t = 1; t < b.n; ++t) sum += s_val[t];
        if (floss) floss[blockIdx.x] += sum;
        if (losses) atomicAdd(&losses[1], (double)sum);
    }
}

// block (128 threads) per frame: dX (=) prior gradients, dJw (=) reprojection gradients of the 23 joints;
// losses (optional, logging): [0] += data term, [1] += priors; floss (optional) [frame] = this frame's data term + priors
// (the value a per-frame line search needs: fdcap_opt_fit2d_lbfgs)
__global__ __launch_bounds__(128) void fit2d_loss_kernel(Fit2dStage s, const float* __restrict__ X, const float* __restrict__ Jw,
                                                         const float* __restrict__ kp, int row0, float* __restrict__ dX,
                                                         float* __restrict__ dJw, double* __restrict__ losses,
                                                         float* __restrict__ floss = nullptr) {
    __shared__ float sred[2][2];
    const int tid = threadIdx.x, r = row0 + blockIdx.x;
    float data = 0.f, prior = 0.f;
    if (tid < XDIM) dX[(size_t)r * XDIM + tid] = fit2d_prior_grad(s, tid, X[(size_t)r * XDIM + tid], &prior);
    if (tid < NJW) {
        const float* j = Jw + ((size_t)r * NJW + tid) * 3;
        const float* k = kp + ((size_t)blockIdx.x * NJW + tid) * 3;
        V3 dJ;
        data = fit2d_joint(s, v3(j[0], j[1], j[2]), k[0], k[1], k[2], &dJ);
        float* o = dJw + ((size_t)r * NJW + tid) * 3;
        o[0] = dJ.x; o[1] = dJ.y; o[2] = dJ.z;
    }
    if (!losses && !floss) return;
    float vals[2] = {data, prior};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float v = vals[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 63) == 0) sred[tid >> 6][i] = v;
    }
    __syncthreads();
    if (floss && tid == 0) floss[blockIdx.x] = (sred[0][0] + sred[1][0]) + (sred[0][1] + sred[1][1]);
    if (losses && tid < 2) atomicAdd(&losses[tid], (double)(sred[0][tid] + sred[1][tid]));
}
#endif

}  // namespace fdc
