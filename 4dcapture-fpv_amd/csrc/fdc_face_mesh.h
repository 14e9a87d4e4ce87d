// The full mesh under a jaw pose and expression coefficients: what turns the inner fit's `jaw_pose` and
// `expression` back into vertices, forward and backward, for the body-model operator (fdcap_smplx_forward_face / _backward_face,
// fdcap_body_forward_face, fdcap_world_mesh_face) and for the inner fit's self-interpenetration term on the fitted face
// (fdcap_opt_set_fit2d_collision_face: fit2d_collision_pass_face, csrc/fdc_api_modes.h).
//
// The model is csrc/fdc_keypoints.h's, piece for piece (jaw_forward / jaw_backward, expr_forward, expr_backward_delta, ...): the chain
// runs at jaw = 0, psi = 0 (pose_fwd_kernel, untouched) and a frame's transforms are CORRECTED afterwards -- delta_j = JE_j psi,
// Dt_j along the joint's path to the root, A_j.t += Dt_j - R_j delta_j, the jaw's leaf form on the corrected A_22 with J22 + delta_22 --
// into a side buffer A'; the pose-feature row gets its jaw block R_w - I in a copy, and the offsets blend_forward wrote gain E psi in
// place.  skin_fwd_kernel, skin_bwd_any, blend_forward and blend_backward then run unchanged on A' and the completed offsets.
// Backward: face_bwd_kernel takes d loss / d A' (skin_bwd_any), the joints' gradient and the vertex part of d psi (expr_dpsi_kernel's
// partial sums) to d loss / d A in the chain's own frame, d psi, the skinning part of d loss / d R_w and J22's share of d betas;
// pose_bwd_op_kernel differentiates the unchanged chain from there.  Every sum runs in a fixed order: no float atomics.
//
// The first part is the per-frame arithmetic as plain host functions in the kernels' order (g++ -std=c++17: tests/test_face_mesh_cpu.py),
// the second the four kernels.
#pragma once
#include "fdc_keypoints.h"

namespace fdc {

// the model's tables the two per-frame kernels read (device pointers; the host functions take the same struct with host pointers)
struct FaceTabs {
    const float *JE, *Jt, *Jd;                 // [55 3][10], the collapsed joint regressor [55 3], [55 3][10]
    const int *parents, *child_start, *child_list, *depth;
    int nlevels;
};

// ---- one frame on the host, in the kernels' order --------------------------------------------------------------------------------
// A [55][12] (rows [R | t], as pose_fwd_kernel wrote them) -> A' in place; pf9 (=) the jaw's pose-feature block (jaw only);
// dt [55][3] (=) the joints' shifts Dt_j (zero without psi).  psi / jaw may be null on their own.
inline void face_forward_frame(const FaceTabs& t, const float* betas, const float* psi, const float* jaw, float* A, float* pf9, float* dt) {
    float delta[NJ * 3];
    for (int e = 0; e < NJ * 3; ++e) delta[e] = psi ? expr_delta_entry(t.JE, psi, e) : 0.f;
    for (int e = 0; e < NJ * 3; ++e) dt[e] = 0.f;
    if (psi) {
        float t3[NJ * 3];                                  // every joint reads rotations only and writes its own translation: any order
        for (int j = 0; j < NJ; ++j) { const V3 d = expr_forward(A, t.parents, delta, j); t3[3 * j] = d.x; t3[3 * j + 1] = d.y; t3[3 * j + 2] = d.z; }
        for (int e = 0; e < NJ * 3; ++e) dt[e] = t3[e];
    }
    if (jaw) {
        const V3 J22 = kp_joint_rest(t.Jt, t.Jd, betas, JAW_J) + v3(delta[3 * JAW_J], delta[3 * JAW_J + 1], delta[3 * JAW_J + 2]);
        jaw_forward(v3(jaw[0], jaw[1], jaw[2]), J22, A + 12 * JAW_J, pf9);
    }
}

// A: the chain's transforms (NOT A'); dAp [55][12] d loss / d A' (null: zero); gJ [55][3] d loss / d joints (null: zero; read with psi
// only -- the jaw moves no joint); dpsi_v [10] the vertices' share E^T d v_posed (null: zero).
// dA (=) d loss / d A for the pose backward; dpsi [10] (=) complete (psi only); R9 (=) the skinning part of d loss / d R_w and
// dbeta [10] (=) Jd_22^T dJ22 (jaw only).
inline void face_backward_frame(const FaceTabs& t, const float* betas, const float* psi, const float* jaw, const float* A, const float* dAp,
                                const float* gJ, const float* dpsi_v, float* dA, float* dpsi, float* R9, float* dbeta) {
    float delta[NJ * 3], da[NJ * 12], own[NJ * 3], S[NJ * 3], dd[NJ * 3];
    for (int e = 0; e < NJ * 3; ++e) delta[e] = psi ? expr_delta_entry(t.JE, psi, e) : 0.f;
    for (int e = 0; e < NJ * 12; ++e) da[e] = dAp ? dAp[e] : 0.f;
    V3 dJ22 = v3(0.f, 0.f, 0.f);
    if (jaw) {
        float a22[12], pf9[9];
        for (int e = 0; e < 12; ++e) a22[e] = A[12 * JAW_J + e];
        const V3 J22 = kp_joint_rest(t.Jt, t.Jd, betas, JAW_J) + v3(delta[3 * JAW_J], delta[3 * JAW_J + 1], delta[3 * JAW_J + 2]);
        const JawFwd f = jaw_forward(v3(jaw[0], jaw[1], jaw[2]), J22, a22, pf9);
        const JawBwd b = jaw_backward(f, da + 12 * JAW_J);
        for (int e = 0; e < 12; ++e) da[12 * JAW_J + e] = b.dA22[e];
        for (int e = 0; e < 9; ++e) R9[e] = b.dRw.m[e];
        dJ22 = b.dJ22;
        for (int l = 0; l < NBETA; ++l) {
            float acc = 0.f;
            acc += t.Jd[(3 * JAW_J) * NBETA + l] * dJ22.x; acc += t.Jd[(3 * JAW_J + 1) * NBETA + l] * dJ22.y; acc += t.Jd[(3 * JAW_J + 2) * NBETA + l] * dJ22.z;
            dbeta[l] = acc;
        }
    }
    if (!psi) { for (int e = 0; e < NJ * 12; ++e) dA[e] = da[e]; return; }
    for (int e = 0; e < NJ * 3; ++e) { own[e] = da[12 * (e / 3) + 4 * (e % 3) + 3] + (gJ ? gJ[e] : 0.f); S[e] = 0.f; }
    for (int L = t.nlevels - 1; L >= 0; --L)
        for (int j = 0; j < NJ; ++j)
            if (t.depth[j] == L) { const V3 s = expr_subtree_children(t.child_start, t.child_list, own, S, j); S[3 * j] = s.x; S[3 * j + 1] = s.y; S[3 * j + 2] = s.z; }
    for (int j = 0; j < NJ; ++j) {
        V3 d = expr_backward_delta(A, t.parents, own, S, da, j);
        if (jaw && j == JAW_J) d = d + dJ22;               // (J22 = its rest position + delta_22)
        dd[3 * j] = d.x; dd[3 * j + 1] = d.y; dd[3 * j + 2] = d.z;
    }
    for (int q = 0; q < NJ * 12; ++q) {
        const int j = q / 12, e = q - 12 * j, i = e >> 2, c = e & 3;
        float v = da[q];
        if (c < 3) v += expr_backward_rot_entry(t.child_start, t.child_list, delta, own, S, da, j, i, c);
        dA[q] = v;
    }
    for (int l = 0; l < NEXPR; ++l) {                      // sixteen partial sums per coefficient, then those in order (the kernel's)
        float pp[16];
        for (int part = 0; part < 16; ++part) {
            float acc = 0.f;
            for (int e = part; e < NJ * 3; e += 16) acc += t.JE[e * NEXPR + l] * dd[e];
            pp[part] = acc;
        }
        float acc = pp[0];
        for (int p = 1; p < 16; ++p) acc += pp[p];
        dpsi[l] = acc + (dpsi_v ? dpsi_v[l] : 0.f);
    }
}

// Voff [ncol] += E psi, E [10][lde]: one frame of expr_offsets_kernel;  dpsi_v [10] (=) E^T dV in expr_dpsi_kernel's order: chunks of
// FACE_CHUNK columns, a chunk's columns ascending in one sum, then the chunks ascending
constexpr int FACE_FS = 16, FACE_CHUNK = 256;
inline int face_nchunk(int ncol) { return (ncol + FACE_CHUNK - 1) / FACE_CHUNK; }
inline void face_offsets_frame(const float* E, int lde, int ncol, const float* psi, float* Voff) {
    for (int c = 0; c < ncol; ++c) {
        float acc = 0.f;
        for (int l = 0; l < NEXPR; ++l) acc += E[(size_t)l * lde + c] * psi[l];
        Voff[c] += acc;
    }
}
inline void face_dpsi_frame(const float* E, int lde, int ncol, const float* dV, float* dpsi_v) {
    for (int l = 0; l < NEXPR; ++l) {
        float tot = 0.f;
        for (int ch = 0; ch < face_nchunk(ncol); ++ch) {
            float part = 0.f;
            for (int c = ch * FACE_CHUNK; c < (ch + 1) * FACE_CHUNK && c < ncol; ++c) part += E[(size_t)l * lde + c] * dV[c];
            tot = ch == 0 ? part : tot + part;
        }
        dpsi_v[l] = tot;
    }
}

#if defined(__HIPCC__)
constexpr int FACE_NT = 256;

// One workgroup per frame: A' [row][55][12] and -- jaw -- PF' [row][496] (the PF row with the jaw's block set) into side buffers, the 55
// body-frame joints G.t + transl + Dt_j to joints [frame][55][3] (optional).  A, PF, G, X, A2, PF2 are indexed by row0 + blockIdx.x, psi,
// jaw and joints by blockIdx.x.  Joints walk their own root paths side by side from LDS copies of the rotations and the tree.
__global__ __launch_bounds__(FACE_NT) void face_fwd_kernel(FaceTabs ft, const float* __restrict__ A, const float* __restrict__ PF,
                                                           const float* __restrict__ G, const float* __restrict__ X, int ldx, int beta_off,
                                                           int transl_off, int row0, const float* __restrict__ psi, const float* __restrict__ jaw,
                                                           float* __restrict__ A2, float* __restrict__ PF2, float* __restrict__ joints) {
    __shared__ float s_A[NJ * 12], s_dl[NJ * 3], s_psi[NEXPR], s_pf9[9];
    __shared__ int s_par[NJ];
    const int tid = threadIdx.x;
    const size_t r = (size_t)(row0 + blockIdx.x);
    for (int e = tid; e < NJ * 12; e += FACE_NT) s_A[e] = A[r * NJ * 12 + e];
    if (tid < NJ) s_par[tid] = ft.parents[tid];
    if (psi && tid >= 64 && tid < 64 + NEXPR) s_psi[tid - 64] = psi[(size_t)blockIdx.x * NEXPR + tid - 64];
    __syncthreads();
    if (tid < NJ * 3) s_dl[tid] = psi ? expr_delta_entry(ft.JE, s_psi, tid) : 0.f;
    __syncthreads();
    V3 dt = v3(0.f, 0.f, 0.f);
    if (psi && tid < NJ) dt = expr_forward(s_A, s_par, s_dl, tid);
    if (joints && tid < NJ) {
        const float* g = G + (r * NJ + tid) * 12;
        const float* x = X + r * ldx + transl_off;
        float* o = joints + ((size_t)blockIdx.x * NJ + tid) * 3;
        o[0] = g[3] + x[0] + dt.x; o[1] = g[7] + x[1] + dt.y; o[2] = g[11] + x[2] + dt.z;
    }
    if (jaw) {                                             // (kernel-uniform)
        __syncthreads();
        if (tid == 0) {
            const float* w = jaw + (size_t)blockIdx.x * 3;
            const V3 J22 = kp_joint_rest(ft.Jt, ft.Jd, X + r * ldx + beta_off, JAW_J) + v3(s_dl[3 * JAW_J], s_dl[3 * JAW_J + 1], s_dl[3 * JAW_J + 2]);
            jaw_forward(v3(w[0], w[1], w[2]), J22, s_A + 12 * JAW_J, s_pf9);
        }
    }
    __syncthreads();
    for (int e = tid; e < NJ * 12; e += FACE_NT) A2[r * NJ * 12 + e] = s_A[e];
    if (jaw && PF2)
        for (int e = tid; e < NPFX; e += FACE_NT) {
            const int b = e - 9 * (JAW_J - 1);
            PF2[r * NPFX + e] = (b >= 0 && b < 9) ? s_pf9[b] : PF[r * NPFX + e];
        }
}

// Voff [frame][ldv] += E psi_frame in place on the offsets blend_forward wrote.  Grid (ceil(ncol / 256), ceil(n / FACE_FS)): a thread
// keeps its column's ten directions in registers and walks a slice of FACE_FS frames, whose psi sit in LDS -- E is read once per slice.
__global__ __launch_bounds__(256) void expr_offsets_kernel(const float* __restrict__ E, int lde, int ncol, const float* __restrict__ psi, int n,
                                                           float* __restrict__ Voff, size_t ldv) {
    __shared__ float s_psi[FACE_FS * NEXPR];
    const int tid = threadIdx.x, f0 = blockIdx.y * FACE_FS, nf = min(FACE_FS, n - f0);
    const int col = blockIdx.x * 256 + tid, cc = min(col, ncol - 1);
    for (int e = tid; e < nf * NEXPR; e += 256) s_psi[e] = psi[(size_t)f0 * NEXPR + e];
    float e10[NEXPR];
#pragma unroll
    for (int l = 0; l < NEXPR; ++l) e10[l] = E[(size_t)l * lde + cc];
    __syncthreads();
    if (col >= ncol) return;
    for (int f = 0; f < nf; ++f) {
        float acc = 0.f;
#pragma unroll
        for (int l = 0; l < NEXPR; ++l) acc += e10[l] * s_psi[f * NEXPR + l];
        Voff[(size_t)(f0 + f) * ldv + col] += acc;
    }
}

// part [frame][nch][10] (=) the partial sums of E^T dVoff_frame over chunk blockIdx.x of FACE_CHUNK columns (face_dpsi_frame's order);
// face_bwd_kernel adds a frame's chunks in ascending order.  Grid (nch, ceil(n / FACE_FS)): the chunk's ten directions and its columns of
// the slice's frames go to LDS once (coalesced), then thread (frame, coefficient) walks the chunk's columns in one sum -- no cross-lane
// reduction.  Rows are padded by one word so that the lanes of a wave, which differ in frame and coefficient, hit different banks.
__global__ __launch_bounds__(FACE_CHUNK) void expr_dpsi_kernel(const float* __restrict__ E, int lde, int ncol, const float* __restrict__ dVoff,
                                                               size_t ldv, int n, float* __restrict__ part, int nch) {
    __shared__ float s_E[NEXPR][FACE_CHUNK + 1], s_d[FACE_FS][FACE_CHUNK + 1];
    const int tid = threadIdx.x, f0 = blockIdx.y * FACE_FS, nf = min(FACE_FS, n - f0);
    const int col = blockIdx.x * FACE_CHUNK + tid;
    const bool in = col < ncol;                              // (columns behind the last one enter as zeros: a sum's value does not change)
#pragma unroll
    for (int l = 0; l < NEXPR; ++l) s_E[l][tid] = in ? E[(size_t)l * lde + col] : 0.f;
    for (int f = 0; f < nf; ++f) s_d[f][tid] = in ? dVoff[(size_t)(f0 + f) * ldv + col] : 0.f;
    __syncthreads();
    if (tid < nf * NEXPR) {
        const int f = tid / NEXPR, l = tid - NEXPR * f;
        float acc = 0.f;
#pragma unroll 8
        for (int c = 0; c < FACE_CHUNK; ++c) acc += s_E[l][c] * s_d[f][c];
        part[((size_t)(f0 + f) * nch + blockIdx.x) * NEXPR + l] = acc;
    }
}

// One workgroup per frame: face_backward_frame.  A (the chain's), dAp, X and dA by row0 + blockIdx.x; psi, jaw, gJ, part, dpsi, R9 by
// blockIdx.x.  dA may be dAp (a frame's rows are staged before any is written).  dX [row][ldx]: Jd_22^T dJ22 is ADDED to the betas'
// entries (the pose backward adds its own afterwards).  The subtree sums run by levels on the first wave with wave barriers.
// add != 0 (the inner fit's self-interpenetration term, after the data term's kernel): dpsi and R9 hold the data term's parts and this
// frame's are added to them, first + second, as fit2d_coll_add_kernel adds the vertex branch's sums.
__global__ __launch_bounds__(FACE_NT) void face_bwd_kernel(FaceTabs ft, const float* __restrict__ A, const float* dAp, const float* __restrict__ X,
                                                           int ldx, int beta_off, int row0, const float* __restrict__ psi,
                                                           const float* __restrict__ jaw, const float* __restrict__ gJ,
                                                           const float* __restrict__ part, int nch, float* dA, float* __restrict__ dpsi,
                                                           float* __restrict__ R9, float* __restrict__ dX, int add) {
    __shared__ float s_A[NJ * 12], s_da[NJ * 12], s_dl[NJ * 3], s_own[NJ * 3], s_S[NJ * 3], s_dd[NJ * 3], s_psi[NEXPR], s_pp[16 * NEXPR], s_dj[3];
    __shared__ int s_par[NJ], s_cs[NJ + 1], s_cl[NJ + 1], s_dep[NJ];
    const int tid = threadIdx.x;
    const size_t r = (size_t)(row0 + blockIdx.x);
    for (int e = tid; e < NJ * 12; e += FACE_NT) { s_A[e] = A[r * NJ * 12 + e]; s_da[e] = dAp ? dAp[r * NJ * 12 + e] : 0.f; }
    if (tid < NJ) { s_par[tid] = ft.parents[tid]; s_dep[tid] = ft.depth[tid]; s_cl[tid] = ft.child_list[tid]; }   // (NJ - 1 children and host_pose_setup's one pad)
    if (tid >= 64 && tid < 64 + NJ + 1) s_cs[tid - 64] = ft.child_start[tid - 64];
    if (psi && tid >= 128 && tid < 128 + NEXPR) s_psi[tid - 128] = psi[(size_t)blockIdx.x * NEXPR + tid - 128];
    __syncthreads();
    if (tid < NJ * 3) { s_dl[tid] = psi ? expr_delta_entry(ft.JE, s_psi, tid) : 0.f; s_S[tid] = 0.f; }
    __syncthreads();
    if (jaw) {                                             // (kernel-uniform)
        if (tid == 0) {
            float a22[12], pf9[9];
            for (int e = 0; e < 12; ++e) a22[e] = s_A[12 * JAW_J + e];
            const float* w = jaw + (size_t)blockIdx.x * 3;
            const V3 J22 = kp_joint_rest(ft.Jt, ft.Jd, X + r * ldx + beta_off, JAW_J) + v3(s_dl[3 * JAW_J], s_dl[3 * JAW_J + 1], s_dl[3 * JAW_J + 2]);
            const JawFwd f = jaw_forward(v3(w[0], w[1], w[2]), J22, a22, pf9);
            const JawBwd b = jaw_backward(f, s_da + 12 * JAW_J);
            for (int e = 0; e < 12; ++e) s_da[12 * JAW_J + e] = b.dA22[e];
            for (int e = 0; e < 9; ++e) {
                float* const o = R9 + (size_t)blockIdx.x * 9 + e;
                *o = add ? *o + b.dRw.m[e] : b.dRw.m[e];
            }
            s_dj[0] = b.dJ22.x; s_dj[1] = b.dJ22.y; s_dj[2] = b.dJ22.z;
        }
        __syncthreads();
        if (tid >= 64 && tid < 64 + NBETA) {
            const int l = tid - 64;
            float acc = 0.f;
            for (int c = 0; c < 3; ++c) acc += ft.Jd[(3 * JAW_J + c) * NBETA + l] * s_dj[c];
            dX[r * ldx + beta_off + l] += acc;
        }
    }
    if (!psi) {                                            // (kernel-uniform) the jaw alone: every other row passes through
        for (int e = tid; e < NJ * 12; e += FACE_NT) dA[r * NJ * 12 + e] = s_da[e];
        return;
    }
    if (tid < NJ * 3) {
        const int j = tid / 3, c = tid - 3 * j;
        s_own[tid] = s_da[12 * j + 4 * c + 3] + (gJ ? gJ[(size_t)blockIdx.x * NJ * 3 + tid] : 0.f);
    }
    __syncthreads();
    if (tid < 64) {                                        // lane j = joint j, the levels from the deepest: a wave's LDS operations execute in order
        const int dep = tid < NJ ? s_dep[tid] : -1;
        for (int L = ft.nlevels - 1; L >= 0; --L) {
            if (dep == L) {
                const V3 sj = expr_subtree_children(s_cs, s_cl, s_own, s_S, tid);
                s_S[3 * tid] = sj.x; s_S[3 * tid + 1] = sj.y; s_S[3 * tid + 2] = sj.z;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    if (tid < NJ) {
        V3 d = expr_backward_delta(s_A, s_par, s_own, s_S, s_da, tid);
        if (jaw && tid == JAW_J) d = d + v3(s_dj[0], s_dj[1], s_dj[2]);
        s_dd[3 * tid] = d.x; s_dd[3 * tid + 1] = d.y; s_dd[3 * tid + 2] = d.z;
    }
    for (int q = tid; q < NJ * 12; q += FACE_NT) {
        const int j = q / 12, e = q - 12 * j, i = e >> 2, c = e & 3;
        float v = s_da[q];
        if (c < 3) v += expr_backward_rot_entry(s_cs, s_cl, s_dl, s_own, s_S, s_da, j, i, c);
        dA[r * NJ * 12 + q] = v;
    }
    __syncthreads();
    if (tid < 16 * NEXPR) {                                // sixteen partial sums per coefficient: entries part, part + 16, ..
        const int p = tid & 15, l = tid >> 4;
        float acc = 0.f;
        for (int e = p; e < NJ * 3; e += 16) acc += ft.JE[e * NEXPR + l] * s_dd[e];
        s_pp[16 * l + p] = acc;
    }
    __syncthreads();
    if (dpsi && tid < NEXPR) {
        float acc = s_pp[16 * tid];
        for (int p = 1; p < 16; ++p) acc += s_pp[16 * tid + p];
        if (part) {
            const float* pr = part + (size_t)blockIdx.x * nch * NEXPR + tid;
            float v = pr[0];
            for (int ch = 1; ch < nch; ++ch) v += pr[(size_t)ch * NEXPR];
            acc += v;
        }
        float* const o = dpsi + (size_t)blockIdx.x * NEXPR + tid;
        *o = add ? *o + acc : acc;
    }
}
#endif

}  // namespace fdc
