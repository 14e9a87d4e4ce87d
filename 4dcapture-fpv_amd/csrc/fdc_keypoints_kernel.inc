// The keypoint kernel's text (csrc/fdc_keypoints.h includes it twice): FDC_KP_KERNEL is the kernel's name, FDC_KP_JAW 0 the kernel as
// it stands without a jaw -- fit2d_kp_kernel, whose code the second form must not perturb -- and 1 the form with a free jaw
// (fit2d_kp_jaw_kernel: one more argument, the blocks between #if FDC_KP_JAW).  FDC_KP_EXPR 1 (the includer leaves it undefined for
// the two kernels above: 0) adds the free expression coefficients, with or without the jaw: one more argument again and the blocks
// between #if FDC_KP_EXPR -- none of which reaches the text of the forms without it.  No include guard, on purpose.
#ifndef FDC_KP_EXPR
#define FDC_KP_EXPR 0
#define FDC_KP_EXPR_DEFAULTED
#endif
template <bool POS, bool PANEL>
__global__ __launch_bounds__(KP_NT) void FDC_KP_KERNEL(Fit2dStage s, KpSet ks, const float* __restrict__ X, const float* __restrict__ PF,
                                                         const float* __restrict__ A, const float* __restrict__ M,
                                                         const float* __restrict__ scale, const float* __restrict__ Jw,
                                                         const float* __restrict__ kp, int row0, float* __restrict__ dX,
                                                         float* __restrict__ dJw, float* __restrict__ dA, float* __restrict__ dPF,
                                                         float* __restrict__ dtransl_v, float* __restrict__ dMv, float* __restrict__ dsv,
                                                         double* __restrict__ losses, float* __restrict__ floss, float* __restrict__ pos_out,
                                                         const float* __restrict__ Voff, float* __restrict__ dVoff
#if FDC_KP_JAW
                                                         , JawIO jw
#endif
#if FDC_KP_EXPR
                                                         , ExprIO ex
#endif
                                                         ) {
    __shared__ float s_x[XDIM + 2], s_pf[NPFX], s_A[NJ * 12], s_M[12], s_jw[NJW * 3 + 3], s_kp[KP_MAX * 3], s_dk[KP_MAX * 3];
    __shared__ float s_v[KP_MAXV * 3];         // pose + shape offsets of the real vertices, later every set vertex's d loss / d v_posed
    __shared__ float s_vp[KP_MAXV * 3], s_vb[KP_MAXV * 3], s_vw[KP_MAXV * 3], s_gv[KP_MAXV * 3];   // (s_vw: positions, later their gradients)
    __shared__ float s_part[KP_PART];
    __shared__ float s_red[16][16], s_sred[4][2], s_db[NBETA];
#if FDC_KP_JAW
    __shared__ JawFwd s_jf;                    // the jaw's forward, kept for the backward
#endif
#if FDC_KP_EXPR
    __shared__ float s_psi[NEXPR], s_dl[NJ * 3], s_djw[NJW * 3];      // the coefficients, delta = JE psi (kept for the backward), d loss / d Jw
    __shared__ float s_dt[NJW * 3];            // the world joints' correction before W (kept for the backward: d M's rotation part)
    __shared__ int s_par[NJ], s_cs[NJ + 1], s_cl[NJ + 1], s_dep[NJ];  // the tree: walked from LDS, not through dependent global loads
    __shared__ float s_eb[PANEL ? NJ * 12 + 3 * NJ * 3 + 16 * NEXPR : 1];   // the backward's transients where the products' workspace is not there
#endif
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
#if FDC_KP_EXPR
    if (nu == 0) {                                         // (a map of joints 0..22 alone: the chain's correction still needs A and M)
        for (int e = tid; e < NJ * 12; e += KP_NT) s_A[e] = A[(size_t)r * NJ * 12 + e];
        if (tid < 12) s_M[tid] = M[(size_t)r * 12 + tid];
    }
    if (tid < NEXPR) s_psi[tid] = ex.psi[(size_t)blockIdx.x * NEXPR + tid];
    if (tid >= 64 && tid < 64 + NJ) { s_par[tid - 64] = ex.parents[tid - 64]; s_dep[tid - 64] = ex.depth[tid - 64]; }
    if (tid >= 128 && tid < 128 + NJ + 1) s_cs[tid - 128] = ex.child_start[tid - 128];
    if (tid >= 192 && tid < 192 + NJ) s_cl[tid - 192] = ex.child_list[tid - 192];      // (NJ - 1 children and host_pose_setup's one pad)
#endif
    const float sc = scale[0];
    __syncthreads();
#if FDC_KP_EXPR
    {   // delta, then every joint's own path to the root side by side (expr_forward); the world joints follow by W = M's rotation
        if (tid < NJ * 3) s_dl[tid] = expr_delta_entry(ex.JE, s_psi, tid);
        __syncthreads();
        if (tid < NJ) {
            const V3 dt = expr_forward(s_A, s_par, s_dl, tid);
            if (tid < NJW) {
                s_dt[3 * tid] = dt.x; s_dt[3 * tid + 1] = dt.y; s_dt[3 * tid + 2] = dt.z;
                s_jw[3 * tid] += s_M[0] * dt.x + s_M[1] * dt.y + s_M[2] * dt.z;
                s_jw[3 * tid + 1] += s_M[4] * dt.x + s_M[5] * dt.y + s_M[6] * dt.z;
                s_jw[3 * tid + 2] += s_M[8] * dt.x + s_M[9] * dt.y + s_M[10] * dt.z;
            }
        }
        if (PANEL)                                         // (blend_forward knows nothing of psi)
            for (int c = tid; c < ncol; c += KP_NT) {
                float acc = 0.f;
                for (int l = 0; l < NEXPR; ++l) acc += ex.E[(size_t)l * ex.lde + c] * s_psi[l];
                s_v[c] += acc;
            }
        __syncthreads();
    }
#endif
#if FDC_KP_JAW
    if (nu > 0) {
        if (tid == 0) {
            const float* w = jw.jaw + (size_t)blockIdx.x * 3;
#if FDC_KP_EXPR
            s_jf = jaw_forward(v3(w[0], w[1], w[2]), kp_joint_rest(ks.Jt, ks.Jd, s_x + X_BETAS, JAW_J) + v3(s_dl[3 * JAW_J], s_dl[3 * JAW_J + 1], s_dl[3 * JAW_J + 2]),
                               s_A + 12 * JAW_J, s_pf + 9 * (JAW_J - 1));
#else
            s_jf = jaw_forward(v3(w[0], w[1], w[2]), kp_joint_rest(ks.Jt, ks.Jd, s_x + X_BETAS, JAW_J), s_A + 12 * JAW_J, s_pf + 9 * (JAW_J - 1));
#endif
        }
        __syncthreads();
        if (PANEL) {
            for (int c = tid; c < ncol; c += KP_NT) {
                float acc = 0.f;
                for (int e = 0; e < 9; ++e) acc += s_pf[9 * (JAW_J - 1) + e] * ks.B[(size_t)(9 * (JAW_J - 1) + e) * ks.ldb + c];
                s_v[c] += acc;
            }
            __syncthreads();
        }
    }
#endif
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
#if FDC_KP_EXPR
            float ea = 0.f;
            for (int l = 0; l < NEXPR; ++l) ea += ex.E[(size_t)l * ex.lde + c] * s_psi[l];
            acc += ea;
#endif
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
#if FDC_KP_EXPR
            acc += s_dl[3 * j + c];
#endif
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
#if FDC_KP_JAW
    if (tid >= XDIM && tid < XDIM + 3) {
        const int c = tid - XDIM;
        const float v = (c == 0 ? jw.w[0] : c == 1 ? jw.w[1] : jw.w[2]) * jw.jaw[(size_t)blockIdx.x * 3 + c];
        prior = v * v;
    }
#endif
#if FDC_KP_EXPR
    if (tid >= XDIM + 3 && tid < XDIM + 3 + NEXPR) {
        const float v = ex.w * s_psi[tid - (XDIM + 3)];
        prior = v * v;
    }
#endif
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
#if FDC_KP_EXPR
        s_djw[3 * tid] = g.x; s_djw[3 * tid + 1] = g.y; s_djw[3 * tid + 2] = g.z;
#endif
    }
#if FDC_KP_EXPR
    // The correction's backward (csrc/fdc_keypoints.h): s_ew holds d loss / d A' [55][12]; dA (=) that plus the rotation addends, and
    // dpsi (=) JE^T d delta + E^T d v_posed + the prior's, complete when the kernel ends.  s_ew: the products' workspace, free between the
    // two products -- the panel form has none (its products run outside), so there the transients have 5.3 KB of their own.
    float* const s_ew = PANEL ? s_eb : s_part;
    auto expr_bwd = [&]() {
        float *const s_da = s_ew, *const s_own = s_ew + NJ * 12, *const s_S = s_own + NJ * 3, *const s_dd = s_S + NJ * 3, *const s_pp = s_dd + NJ * 3;
        static_assert(NJ * 12 + 3 * NJ * 3 + 16 * NEXPR <= KP_PART, "the workspace holds the expression's backward");
        if (tid < NJ * 3) {
            const int j = tid / 3, c = tid - 3 * j;
            float o = s_da[12 * j + 4 * c + 3];
            // W^T dJw_j, W = the rotation of M (rows of four: [R | t], as A's): column c; the forward above applies the same rows
            // (tests/test_gpu_world_frame.py runs both under cameras other than the identity)
            if (j < NJW) o += (s_M[c] * s_djw[3 * j] + s_M[4 + c] * s_djw[3 * j + 1]) + s_M[8 + c] * s_djw[3 * j + 2];
            s_own[tid] = o;
        }
        __syncthreads();
        if (tid < 64) {                                    // lane j = joint j, the levels from the deepest: a wave's LDS operations execute in order
            const int dep = tid < NJ ? s_dep[tid] : -1;
            for (int L = ex.nlevels - 1; L >= 0; --L) {
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
#if FDC_KP_JAW
            if (tid == JAW_J && nu > 0) d = d + v3(s_dk[16], s_dk[17], s_dk[18]);      // (J22 = its rest position + delta_22)
#endif
            s_dd[3 * tid] = d.x; s_dd[3 * tid + 1] = d.y; s_dd[3 * tid + 2] = d.z;
        }
        if (tid >= 64 && tid < 64 + NJ * 12) {             // (beside the first wave's joints)
            const int q = tid - 64, j = q / 12, e = q - 12 * j, i = e >> 2, c = e & 3;
            float v = s_da[q];
            if (c < 3) v += expr_backward_rot_entry(s_cs, s_cl, s_dl, s_own, s_S, s_da, j, i, c);
            dA[(size_t)r * NJ * 12 + q] = v;
        }
        __syncthreads();
        if (tid < 16 * NEXPR) {                            // sixteen partial sums per coefficient: entries part, part + 16, ..
            const int part = tid & 15, l = tid >> 4;
            float acc = 0.f;
            for (int e = part; e < NJ * 3; e += 16) acc += ex.JE[e * NEXPR + l] * s_dd[e];
            for (int c = part; c < 3 * nu; c += 16) acc += ex.E[(size_t)l * ex.lde + c] * s_v[c];
            s_pp[tid] = acc;
        }
        __syncthreads();
        if (tid < NEXPR) {
            float acc = s_pp[16 * tid];
            for (int p = 1; p < 16; ++p) acc += s_pp[16 * tid + p];
            ex.dpsi[(size_t)blockIdx.x * NEXPR + tid] = acc + 2.f * ex.w * ex.w * s_psi[tid];
        }
        __syncthreads();
    };
#endif
#if FDC_KP_JAW
    if (nu == 0 && tid < 9) jw.R9[(size_t)blockIdx.x * 9 + tid] = 0.f;                // (no vertex follows the jaw)
#endif
#if FDC_KP_EXPR
    if (nu == 0) {                                         // (kernel-uniform) only the world joints' gradients reach the chain's correction
        for (int e = tid; e < NJ * 12; e += KP_NT) s_ew[e] = 0.f;
        __syncthreads();
        expr_bwd();
        // Jw_j = W (G_j.t + Dt_j + transl) + M.t: pose_bwd_kernel forms d M's rotation part from G_j.t + transl, which it knows; the
        // correction's share, sum_j dJw_j (x) Dt_j, is this kernel's to add -- here it is all of dMv (no vertex: the other sums stay unread)
        if (tid < 12) {
            const int i = tid >> 2, c = tid & 3;
            float acc = 0.f;
            if (c < 3) for (int j = 0; j < NJW; ++j) acc += s_djw[3 * j + i] * s_dt[3 * j + c];
            dMv[(size_t)r * 12 + tid] = acc;
        }
    }
#endif
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
#if FDC_KP_JAW
        if (j == JAW_J) s_dk[e] = acc;                     // (d loss / d A'_22: through jaw_backward below; s_dk is free by now)
        else
#endif
#if FDC_KP_EXPR
        s_ew[it] = acc;                                    // (d loss / d A': through expr_bwd below)
#else
        dA[(size_t)r * NJ * 12 + it] = acc;
#endif
    }
#if FDC_KP_JAW
    {
        __syncthreads();
        if (tid == 0) {
            const JawBwd b = jaw_backward(s_jf, s_dk);
#if FDC_KP_EXPR
            for (int e = 0; e < 12; ++e) s_ew[12 * JAW_J + e] = b.dA22[e];
            for (int i = 0; i < 3; ++i) for (int c = 0; c < 3; ++c) s_A[12 * JAW_J + 4 * i + c] = s_jf.RA.m[3 * i + c];   // (the chain's rotation again)
#else
            for (int e = 0; e < 12; ++e) dA[(size_t)r * NJ * 12 + 12 * JAW_J + e] = b.dA22[e];
#endif
            for (int e = 0; e < 9; ++e) jw.R9[(size_t)blockIdx.x * 9 + e] = b.dRw.m[e];
            s_dk[16] = b.dJ22.x; s_dk[17] = b.dJ22.y; s_dk[18] = b.dJ22.z;
        }
        __syncthreads();
        if (tid >= X_BETAS && tid < X_BETAS + NBETA) {     // d betas through J22: added by the thread that wrote the entry above
            const int l = tid - X_BETAS;
            float acc = 0.f;
            for (int c = 0; c < 3; ++c) acc += ks.Jd[(3 * JAW_J + c) * NBETA + l] * s_dk[16 + c];
            dX[(size_t)r * XDIM + tid] += acc;
        }
    }
#endif
#if FDC_KP_EXPR
    __syncthreads();
    expr_bwd();
#endif
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
#if FDC_KP_EXPR
        // the world joints' share of d M's rotation part that pose_bwd_kernel cannot form: sum_j dJw_j (x) Dt_j (Jw_j = W (G_j.t + Dt_j +
        // transl) + M.t, and the pose backward knows G_j.t + transl alone); an exact zero at psi = 0
        if (part == 0 && o < 12 && (o & 3) < 3)
            for (int j = 0; j < NJW; ++j) acc += s_djw[3 * j + (o >> 2)] * s_dt[3 * j + (o & 3)];
#endif
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
#ifdef FDC_KP_EXPR_DEFAULTED
#undef FDC_KP_EXPR
#undef FDC_KP_EXPR_DEFAULTED
#endif
