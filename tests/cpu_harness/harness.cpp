// TEST INFRASTRUCTURE ONLY: compiles the host/device math headers of the HIP kernels with g++
// so their forward/backward formulas can be checked against the oracle's autograd in the
// GPU-less build container.  Each function mirrors the body of the kernel of the same name in
// 4dcapture-fpv_amd/csrc/fdcap.hip with the thread loops run serially.  Nothing in the product
// loads this library.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../4dcapture-fpv_amd/csrc/fdc_dct.h"
#include "../../4dcapture-fpv_amd/csrc/fdc_fit2d.h"
#include "../../4dcapture-fpv_amd/csrc/fdc_frame.h"
#include "../../4dcapture-fpv_amd/csrc/fdc_host_setup.h"
#include "../../4dcapture-fpv_amd/csrc/fdc_loss.h"
#include "../../4dcapture-fpv_amd/csrc/fdc_math.h"
#include "../../4dcapture-fpv_amd/csrc/fdc_skin.h"

using namespace fdc;

struct NoSync { void operator()() const {} };

struct HPose {
    HostPoseSetup hs;
    std::vector<float> hand_comp, hand_mean;
    PoseModel pm() const {
        PoseModel m;
        m.Jt = hs.Jt.data(); m.Jd = hs.Jd.data(); m.parents = hs.parents.data(); m.order = hs.order.data();
        m.level_start = hs.level_start.data(); m.child_start = hs.child_start.data(); m.child_list = hs.child_list.data();
        m.hand_comp = hand_comp.data(); m.hand_mean = hand_mean.data(); m.nlevels = hs.nlevels;
        return m;
    }
};

extern "C" {

void* h_pose_setup(int V, const float* vt, const float* S10, const float* Jreg, const int* parents,
                   const float* hand_comp, const float* hand_mean) {
    HPose* h = new HPose();
    if (!host_pose_setup(V, vt, S10, Jreg, parents, &h->hs)) { delete h; return nullptr; }
    h->hand_comp.assign(hand_comp, hand_comp + 2 * 12 * 45);
    h->hand_mean.assign(hand_mean, hand_mean + 90);
    return h;
}
void h_pose_free(void* h) { delete (HPose*)h; }
void h_pose_get_J(void* hv, float* Jt, float* Jd) {
    HPose* h = (HPose*)hv;
    memcpy(Jt, h->hs.Jt.data(), sizeof(float) * NJ * 3);
    memcpy(Jd, h->hs.Jd.data(), sizeof(float) * NJ * 3 * NBETA);
}

void h_pose_forward(void* hv, int rows, const float* X, const float* O, const float* CAM, float scale, float* Rm,
                    float* PF, float* Jrest, float* G, float* A, float* M, float* Jw) {
    HPose* h = (HPose*)hv;
    PoseModel pm = h->pm();
    static PoseScratch sc;
    for (int r = 0; r < rows; ++r)
        pose_forward(pm, X + (size_t)r * XDIM, O + (size_t)r * ODIM, CAM + (size_t)r * 16, scale, sc,
                     Rm + (size_t)r * NJ * 9, PF + (size_t)r * NPF, Jrest + (size_t)r * NJ * 3, G + (size_t)r * NJ * 12,
                     A + (size_t)r * NJ * 12, M + (size_t)r * 12, Jw + (size_t)r * NJW * 3, 0, 1, NoSync());
}

void h_pose_backward(void* hv, int rows, const float* X, const float* O, const float* CAM, float scale, const float* Rm,
                     const float* Jrest, const float* G, const float* dA, const float* dPF, const float* dJw,
                     const float* dMv, const float* dsv, const float* dbeta_v, const float* dtransl_v, float* dX,
                     float* dO, float* dCAM, float* dscale_row) {
    HPose* h = (HPose*)hv;
    PoseModel pm = h->pm();
    static PoseScratch sc;
    for (int r = 0; r < rows; ++r)
        pose_backward(pm, X + (size_t)r * XDIM, O + (size_t)r * ODIM, CAM + (size_t)r * 16, scale,
                      Rm + (size_t)r * NJ * 9, Jrest + (size_t)r * NJ * 3, G + (size_t)r * NJ * 12,
                      dA ? dA + (size_t)r * NJ * 12 : nullptr, dPF ? dPF + (size_t)r * NPF : nullptr,
                      dJw ? dJw + (size_t)r * NJW * 3 : nullptr, dMv ? dMv + (size_t)r * 12 : nullptr,
                      dsv ? dsv + r : nullptr, dbeta_v ? dbeta_v + (size_t)r * NBETA : nullptr,
                      dtransl_v ? dtransl_v + (size_t)r * 3 : nullptr, sc, dX + (size_t)r * XDIM, dO + (size_t)r * ODIM,
                      dCAM + (size_t)r * 16, dscale_row + r, 0, 1, NoSync());
}

static SkinModel mk_skin(const float* vt, const float* S, const int* wj, const float* ww, int K) {
    SkinModel sm; sm.vt = vt; sm.S = S; sm.wj = wj; sm.ww = ww; sm.K = K; return sm;
}

void h_skin_forward(int nv, int K, const float* vt, const float* S, const int* wj, const float* ww, int rows,
                    const float* X, const float* Voff, const float* A, const float* M, float scale, int world,
                    float* Vout) {
    SkinModel sm = mk_skin(vt, S, wj, ww, K);
    const float ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int r = 0; r < rows; ++r) {
        const float* x = X + (size_t)r * XDIM;
        V3 transl = v3(x[X_TRANSL], x[X_TRANSL + 1], x[X_TRANSL + 2]);
        for (int c = 0; c < nv; ++c) {
            SkinFwd f = skin_forward_vertex(sm, c, x + X_BETAS, Voff + ((size_t)r * nv + c) * 3, A + (size_t)r * NJ * 12,
                                            transl, world ? M + (size_t)r * 12 : ident, world ? scale : 1.f);
            float* o = Vout + ((size_t)r * nv + c) * 3;
            o[0] = f.vw.x; o[1] = f.vw.y; o[2] = f.vw.z;
        }
    }
}

// mirrors skin_bwd_kernel; scene4 is [ns,4]
void h_skin_backward(int nc, int K, const float* vt, const float* S, const int* wj, const float* ww, int rows,
                     const float* X, const float* Voff, const float* A, const float* M, float scale, const float* Vw,
                     const float* dist, const int* idx, const float* scene4, float coef, float* dVoff, float* dA,
                     float* dbeta_v, float* dtransl_v, float* dMv, float* dsv, double* loss_contact_sum) {
    SkinModel sm = mk_skin(vt, S, wj, ww, K);
    for (int r = 0; r < rows; ++r) {
        const float* x = X + (size_t)r * XDIM;
        V3 transl = v3(x[X_TRANSL], x[X_TRANSL + 1], x[X_TRANSL + 2]);
        float* da = dA + (size_t)r * NJ * 12;
        for (int i = 0; i < NJ * 12; ++i) da[i] = 0.f;
        float acc[NBETA + 17];
        for (int i = 0; i < NBETA + 17; ++i) acc[i] = 0.f;
        for (int c = 0; c < nc; ++c) {
            size_t qi = (size_t)r * nc + c;
            float dterm;
            float term = contact_term(dist[qi], &dterm);
            const float* p = scene4 + 4 * (size_t)idx[qi];
            float gg = 2.f * coef * dterm;
            V3 g = v3(gg * (Vw[3 * qi] - p[0]), gg * (Vw[3 * qi + 1] - p[1]), gg * (Vw[3 * qi + 2] - p[2]));
            SkinFwd f = skin_forward_vertex(sm, c, x + X_BETAS, Voff + 3 * qi, A + (size_t)r * NJ * 12, transl,
                                            M + (size_t)r * 12, scale);
            SkinBwd b = skin_backward_vertex(f, M + (size_t)r * 12, scale, g);
            dVoff[3 * qi] = b.dvp.x; dVoff[3 * qi + 1] = b.dvp.y; dVoff[3 * qi + 2] = b.dvp.z;
            for (int l = 0; l < NBETA; ++l)
                acc[l] += S[(3 * c) * 10 + l] * b.dvp.x + S[(3 * c + 1) * 10 + l] * b.dvp.y + S[(3 * c + 2) * 10 + l] * b.dvp.z;
            acc[NBETA] += b.gv.x; acc[NBETA + 1] += b.gv.y; acc[NBETA + 2] += b.gv.z;
            for (int e = 0; e < 12; ++e) acc[NBETA + 3 + e] += b.dM[e];
            acc[NBETA + 15] += b.ds;
            acc[NBETA + 16] += term;
            for (int k = 0; k < K; ++k) {
                float w = ww[c * K + k];
                if (w != 0.f) for (int e = 0; e < 12; ++e) da[wj[c * K + k] * 12 + e] += w * b.dT[e];
            }
        }
        for (int l = 0; l < NBETA; ++l) dbeta_v[(size_t)r * NBETA + l] = acc[l];
        for (int k = 0; k < 3; ++k) dtransl_v[(size_t)r * 3 + k] = acc[NBETA + k];
        for (int e = 0; e < 12; ++e) dMv[(size_t)r * 12 + e] = acc[NBETA + 3 + e];
        dsv[r] = acc[NBETA + 15];
        *loss_contact_sum += acc[NBETA + 16];
    }
}

// mirrors param_loss_kernel; X / X0 / mask / Jw have `rows` rows, the owned ones are [row0, row0+n_own)
void h_param_loss(const float* X, const float* X0, const float* mask, const float* Jw, int row0, int n_own, int frame0,
                  int n_total, float w_rec_over_cnt, float w_sm_over_cnt, float w_ws_over_cnt, int world_grad, float* dX,
                  float* dJw, double* losses) {
    for (int b = 0; b < n_own; ++b) {
        int r = row0 + b, g = frame0 + b;
        for (int t = 0; t < XDIM; ++t) {
            const float* x = X + (size_t)r * XDIM + t;
            float xm2 = (g >= 2) ? x[-2 * XDIM] : 0.f, xm1 = (g >= 1) ? x[-XDIM] : 0.f;
            float xp1 = (g + 1 < n_total) ? x[XDIM] : 0.f, xp2 = (g + 2 < n_total) ? x[2 * XDIM] : 0.f;
            float rec, sm;
            dX[(size_t)r * XDIM + t] = param_loss_grad(g, n_total, xm2, xm1, x[0], xp1, xp2, X0[(size_t)r * XDIM + t],
                                                       mask[r], w_rec_over_cnt, w_sm_over_cnt, &rec, &sm);
            losses[0] += rec; losses[2] += sm;
            if (t >= X_LATENT && t < X_LATENT + 32) losses[1] += x[0] * x[0];
        }
        for (int t = 0; t < NJW * 3; ++t) {
            const float* j = Jw + (size_t)r * NJW * 3 + t;
            float jm1 = (g >= 1) ? j[-NJW * 3] : 0.f, jp1 = (g + 1 < n_total) ? j[NJW * 3] : 0.f;
            float ws;
            float gr = world_smooth_grad(g, n_total, jm1, j[0], jp1, w_ws_over_cnt, &ws);
            if (world_grad) dJw[(size_t)r * NJW * 3 + t] = gr;
            losses[4] += ws;
        }
    }
}

void h_adam(float* p, float* m, float* v, const float* g, int64_t n, double lr, int step, int zero_grad) {
    AdamScalars a = adam_scalars(lr, step);
    for (int64_t i = 0; i < n; ++i) adam_update(p[i], m[i], v[i], zero_grad ? 0.f : g[i], a);
}

void h_75_to_78(const float* in, int B, float* out) {
    for (int b = 0; b < B; ++b) {
        const float* p = in + (size_t)b * 75;
        float* x = out + (size_t)b * XDIM;
        for (int i = 0; i < 3; ++i) x[i] = p[i];
        M3 R = tgm_aa_to_rotmat(v3(p[3], p[4], p[5]));
        x[3] = R.m[0]; x[4] = R.m[1]; x[5] = R.m[3]; x[6] = R.m[4]; x[7] = R.m[6]; x[8] = R.m[7];
        for (int i = 6; i < 75; ++i) x[i + 3] = p[i];
    }
}

void h_78_to_75(const float* in, int B, float* out) {
    for (int b = 0; b < B; ++b) {
        const float* x = in + (size_t)b * XDIM;
        float* p = out + (size_t)b * 75;
        for (int i = 0; i < 3; ++i) p[i] = x[i];
        V3 aa = tgm_rotmat_to_aa(gs_forward(x + X_SIXD, 1, nullptr));
        p[3] = aa.x; p[4] = aa.y; p[5] = aa.z;
        for (int i = 9; i < XDIM; ++i) p[i - 3] = x[i];
    }
}

// fit2d_loss_kernel with the threads run serially: X [n,78], Jw [n,23,3], kp [n,23,3] -> dX [n,78], dJw [n,23,3], losses[2]
void h_fit2d_loss(const float* stage9, const float* X, const float* Jw, const float* kp, int n, float* dX, float* dJw,
                  double* losses) {
    Fit2dStage s = {stage9[0], stage9[1], stage9[2], stage9[3], stage9[4], stage9[5], stage9[6], stage9[7], stage9[8]};
    losses[0] = losses[1] = 0.0;
    for (int r = 0; r < n; ++r) {
        for (int e = 0; e < XDIM; ++e) {
            float val;
            dX[(size_t)r * XDIM + e] = fit2d_prior_grad(s, e, X[(size_t)r * XDIM + e], &val);
            losses[1] += val;
        }
        for (int j = 0; j < NJW; ++j) {
            const float* p = Jw + ((size_t)r * NJW + j) * 3;
            const float* k = kp + ((size_t)r * NJW + j) * 3;
            V3 dJ;
            losses[0] += fit2d_joint(s, v3(p[0], p[1], p[2]), k[0], k[1], k[2], &dJ);
            float* o = dJw + ((size_t)r * NJW + j) * 3;
            o[0] = dJ.x; o[1] = dJ.y; o[2] = dJ.z;
        }
    }
}

// frame_smoother_kernel with the element threads run serially
void h_frame_smoother(const float* data78, int N, int iters, double lr, float w_rec, float w_vposer, float w_prev,
                      float* out78) {
    SmootherWeights w = smoother_weights(w_rec, w_vposer, w_prev);
    for (int e = 0; e < 78; ++e) {
        float m = 0.f, v = 0.f, prev = 0.f;
        for (int f = 0; f < N; ++f) {
            const float xd = data78[(size_t)f * 78 + e];
            float x = xd;
            for (int it = 0; it < iters; ++it)
                adam_update(x, m, v, smoother_grad(e, x, xd, prev, f > 0, w), adam_scalars(lr, f * iters + it + 1));
            out78[(size_t)f * 78 + e] = x;
            prev = x;
        }
    }
}

// dct_fit_kernel for one trajectory with the lane sums run serially (frame-ascending)
void h_dct_fit(const float* traj, int T, int C, const float* D, float* coef, float* m, float* v, int iters, int step0,
               double lr, float w_over_cnt, float* obj_hist) {
    for (int it = 0; it < iters; ++it) {
        float g[DCT_MAXC] = {0}, osum = 0.f;
        for (int f = 0; f < T; ++f) {
            float p = 0.f;
            for (int c = 0; c < C; ++c) p += D[f * C + c] * coef[c];
            float obj;
            float gp = dct_residual(traj[f], p, &obj) * w_over_cnt;
            osum += obj;
            for (int c = 0; c < C; ++c) g[c] += D[f * C + c] * gp;
        }
        if (obj_hist) obj_hist[it] = osum;
        AdamScalars a = adam_scalars(lr, step0 + it + 1);
        for (int c = 0; c < C; ++c) adam_update(coef[c], m[c], v[c], g[c], a);
    }
}

// dct_joint_grad_kernel: dJw [n,69] and the un-normalised objective sum
double h_dct_joint_grad(const float* Jw, int n, int T, int C, int W, const float* D, const float* coef, float w_over_cnt,
                        float* dJw) {
    double sum = 0.0;
    for (int i = 0; i < n * 69; ++i) {
        int g = i / 69, ij = i % 69, k = g / T, f = g % T;
        float grad = 0.f, obj = 0.f;
        if (k < W) {
            const float* c = coef + ((size_t)k * 69 + ij) * C;
            float p = 0.f;
            for (int q = 0; q < C; ++q) p += D[f * C + q] * c[q];
            grad = -dct_residual(Jw[i], p, &obj) * w_over_cnt;
        }
        dJw[i] = grad;
        sum += obj;
    }
    return sum;
}

void h_rotmat_to_aa(const float* R, int n, float* aa) {
    for (int i = 0; i < n; ++i) {
        M3 m; for (int e = 0; e < 9; ++e) m.m[e] = R[(size_t)i * 9 + e];
        V3 a = tgm_rotmat_to_aa(m);
        aa[3 * i] = a.x; aa[3 * i + 1] = a.y; aa[3 * i + 2] = a.z;
    }
}

void h_rotmat_to_aa_bwd(const float* R, const float* g, int n, float* dR) {
    for (int i = 0; i < n; ++i) {
        M3 m; for (int e = 0; e < 9; ++e) m.m[e] = R[(size_t)i * 9 + e];
        M3 d = tgm_rotmat_to_aa_backward(m, v3(g[3 * i], g[3 * i + 1], g[3 * i + 2]));
        for (int e = 0; e < 9; ++e) dR[(size_t)i * 9 + e] = d.m[e];
    }
}

// the bare Gram-Schmidt and Rodrigues pairs (tests/test_rotation_edges_cpu.py): s [n,6] in the decoder's interleaved layout,
// r [n,3], R / dR [n,9] row-major
void h_gs_forward(const float* s, int n, float* R) {
    for (int i = 0; i < n; ++i) {
        M3 m = gs_forward(s + (size_t)i * 6, 1, nullptr);
        for (int e = 0; e < 9; ++e) R[(size_t)i * 9 + e] = m.m[e];
    }
}
void h_gs_backward(const float* s, const float* dR, int n, float* ds) {
    for (int i = 0; i < n; ++i) {
        GsCache c;
        gs_forward(s + (size_t)i * 6, 1, &c);
        M3 d; for (int e = 0; e < 9; ++e) d.m[e] = dR[(size_t)i * 9 + e];
        gs_backward(c, d, ds + (size_t)i * 6, 1);
    }
}
void h_rodrigues(const float* r, int n, float* R) {
    for (int i = 0; i < n; ++i) {
        M3 m = rodrigues_forward(v3(r[3 * i], r[3 * i + 1], r[3 * i + 2]));
        for (int e = 0; e < 9; ++e) R[(size_t)i * 9 + e] = m.m[e];
    }
}
void h_rodrigues_bwd(const float* r, const float* dR, int n, float* dr) {
    for (int i = 0; i < n; ++i) {
        M3 d; for (int e = 0; e < 9; ++e) d.m[e] = dR[(size_t)i * 9 + e];
        V3 g = rodrigues_backward(v3(r[3 * i], r[3 * i + 1], r[3 * i + 2]), d);
        dr[3 * i] = g.x; dr[3 * i + 1] = g.y; dr[3 * i + 2] = g.z;
    }
}

// operator-level body model (fdcap_smplx_forward / fdcap_smplx_backward): global_orient + body pose as axis-angle rows AA
// [rows,66], gradient of the 55 body-frame joints dJb [rows,165] -> dX rows (transl, betas, hands) and dAA [rows,66]
void h_pose_forward_aa(void* hv, int rows, const float* X, const float* AA, float* Rm, float* PF, float* Jrest, float* G, float* A) {
    HPose* h = (HPose*)hv;
    PoseModel pm = h->pm();
    static PoseScratch sc;
    const float cam[16] = {0};
    for (int r = 0; r < rows; ++r)
        pose_forward(pm, X + (size_t)r * XDIM, (const float*)nullptr, cam, 0.f, sc, Rm + (size_t)r * NJ * 9, PF + (size_t)r * NPF,
                     Jrest + (size_t)r * NJ * 3, G + (size_t)r * NJ * 12, A + (size_t)r * NJ * 12, (float*)nullptr, (float*)nullptr,
                     0, 1, NoSync(), AA + (size_t)r * 66);
}
void h_pose_backward_aa(void* hv, int rows, const float* X, const float* AA, const float* Rm, const float* Jrest, const float* G,
                        const float* dA, const float* dPF, const float* dbeta_v, const float* dtransl_v, const float* dJb,
                        float* dX, float* dAA) {
    HPose* h = (HPose*)hv;
    PoseModel pm = h->pm();
    static PoseScratch sc;
    const float cam[16] = {0};
    float dO[ODIM], dcam[16], dsc;
    for (int r = 0; r < rows; ++r)
        pose_backward(pm, X + (size_t)r * XDIM, (const float*)nullptr, cam, 0.f, Rm + (size_t)r * NJ * 9, Jrest + (size_t)r * NJ * 3,
                      G + (size_t)r * NJ * 12, dA ? dA + (size_t)r * NJ * 12 : nullptr, dPF ? dPF + (size_t)r * NPF : nullptr,
                      (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                      dbeta_v ? dbeta_v + (size_t)r * NBETA : nullptr, dtransl_v ? dtransl_v + (size_t)r * 3 : nullptr, sc,
                      dX + (size_t)r * XDIM, dO, dcam, &dsc, 0, 1, NoSync(), AA + (size_t)r * 66, dAA + (size_t)r * 66,
                      dJb ? dJb + (size_t)r * NJ * 3 : nullptr);
}

}  // extern "C"
