// The text of pose_bwd_kernel and pose_bwd_reproj_kernel (csrc/fdc_k_pose.h includes it twice: FDC_PB_KERNEL the kernel's name,
// FDC_PB_REPROJ 1 with the clip-level reprojection term in the prologue).  No include guard.
__global__ __launch_bounds__(64 * POSE_NW) void FDC_PB_KERNEL(PoseModel pm, const float* __restrict__ X, const float* __restrict__ O,
                                                      const float* __restrict__ CAM, const float* __restrict__ scale,
                                                      int row0, const float* Rm, const float* Jrest, const float* G,
                                                      const float* dA, const float* dPF, const float* dJw,
                                                      const float* dMv, const float* dsv, const float* dbeta_v,
                                                      int dbeta_stride, const float* dtransl_v, float* dX, float* dO,
                                                      float* dCAM, float* dscale_row, ParamLossIn pl, const float* dPF2, int dA_nj = NJ,
                                                      int clip_n = 0, const ClipRow* __restrict__ ctab = nullptr,
                                                      int jn = NJ, int jr = NJ, int nlev = -1
#if FDC_PB_REPROJ
                                                      , ReprojIn rp = ReprojIn()
#endif
                                                      ) {
    // jn, jr, nlev: the joints this launch's loss can reach (plan_pose_joints; pose_backward's comment): the forward wrote rows
    // below jn of G / Jrest only, and only those rows of G and dA are staged
    // ctab != nullptr: a batch of clips of different lengths -- the frame's clip, its index within it, the clip's length and the
    // clip's three weights come from the frame's record (requested here with the staging copies) instead of pl and clip_n
    // clip_n > 0: a batch of clips of clip_n frames (fdcap_opt_create_clips): the frame's `scale` is its clip's, and the temporal
    // stencils of the fused prologue see the frame's index within its clip (pl.frame0 = 0, pl.n_total = clip_n): cut at clip boundaries
    // dA_nj: rows of dA that were written (the rest are zero: SkinModel::ja_hi)
    // dPF2 (optional): second partial of dPF -- the data-gradient product split over K (panel_gemm3_rb2k_kernel); the row is
    // dPF + dPF2, d betas its columns NPF.. (dbeta_v must then be dPF + NPF, stride NPFX)
    __shared__ PoseScratch sc;
    __shared__ PoseStage stg;
    __shared__ float s_dJw[NJW * 3];
    // Everything this frame reads from global memory arrives in ONE batch of LDS-DMA copies (stage_pose_issue's comment): the
    // pose tables, the forward pass's per-joint state, the incoming gradient rows, and what the fused parameter-loss prologue
    // needs (neighbouring rows: two halo rows exist on either side of every owned row).  Fetched phase by phase -- as
    // pose_backward does for its generic callers -- they were ~8 dependent cold round trips.
    __shared__ __attribute__((aligned(16))) float s_dPF[NPFX];
    __shared__ __attribute__((aligned(16))) float s_O[O_LD], s_Jr[JR_LD];
    __shared__ float s_xn[4][XDIM + 2], s_x0[XDIM + 2], s_jw[3][NJW * 3 + 3], s_misc[32];
    __shared__ float s_dx[XDIM + 2];      // the parameter-gradient row: accumulated here (pose_backward adds to it from several
                                          // phases -- read-modify-write round trips on the global row), stored once at the end
#if FDC_PB_REPROJ
    // the frame's keypoint row, d loss / d (G.t + transl) of every joint -- zero from joint 23 on -- and the d cam_t sums
    __shared__ float s_kp[NJW * 3 + 3], s_dJb[NJ * 3 + 3], s_rp[4];
#endif
    FDC_FR_STAMP(1, 0);
    const int r = row0 + blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const float* const xrow = X + (size_t)r * XDIM;
    const float* const camrow = CAM + (size_t)r * 16;
    if (wave == 0) {
        stage_pose_part<0>(pm, stg, xrow, camrow);
        if (pl.X0) {                                         // (the copies are dealt so that every wave issues 12-13 of them)
            const float* j = pl.Jw + (size_t)r * NJW * 3;
            glds4<2>(j - NJW * 3, s_jw[0], NJW * 3); glds4<2>(j, s_jw[1], NJW * 3); glds4<2>(j + NJW * 3, s_jw[2], NJW * 3);
        }
    } else if (wave == 1) {
        stage_pose_part<1>(pm, stg, xrow, camrow);
        glds16<1>(Jrest + (size_t)r * JR_LD, s_Jr, JR_LD / 4);
        glds16<(NJ * 3 + 63) / 64>(G + (size_t)r * NJ * 12, &sc.G[0][0], jn * 3);              // rows of sc.G are 12 floats: a flat copy
        glds16<1>(O + (size_t)r * O_LD, s_O, O_LD / 4);
        if (dMv) glds4<1>(dMv + (size_t)r * 12, s_misc, 12);
        if (dsv) glds4<1>(dsv + r, s_misc + 12, 1);
        if (dtransl_v) glds4<1>(dtransl_v + (size_t)r * 3, s_misc + 13, 3);
        if (dbeta_v) glds4<1>(dbeta_v + (size_t)r * dbeta_stride, s_misc + 16, NBETA);
    } else if (wave == 2) {
        stage_pose_part<2>(pm, stg, xrow, camrow);
        if (dA) {                                          // waits in sc.dG: lane j reads row j, then overwrites it
            const int da_n = dA_nj < jn ? dA_nj : jn;        // (rows >= jn: zero by construction and never read)
            glds16<(NJ * 3 + 63) / 64>(dA + (size_t)r * NJ * 12, &sc.dG[0][0], da_n * 3);
            for (int e = da_n * 12 + (int)(threadIdx.x & 63); e < jn * 12; e += 64) (&sc.dG[0][0])[e] = 0.f;   // rows nobody wrote
        }
        if (dPF) glds16<(NPFX / 4 + 63) / 64>(dPF + (size_t)r * NPFX, s_dPF, NPFX / 4);
        if (dPF2) glds16<(NPFX / 4 + 63) / 64>(dPF2 + (size_t)r * NPFX, &sc.dR[0][0], NPFX / 4);   // parked in sc.dR (written much later)
#if FDC_PB_REPROJ
        glds4<2>(rp.kp + (size_t)blockIdx.x * NJW * 3, s_kp, NJW * 3);     // (kp holds the owned rows alone: no halo)
#endif
    } else if (pl.X0) {
        stage_pose_part<3>(pm, stg, xrow, camrow);
        const float* x = xrow;
        glds4<2>(x - 2 * XDIM, s_xn[0], XDIM); glds4<2>(x - XDIM, s_xn[1], XDIM);
        glds4<2>(x + XDIM, s_xn[2], XDIM); glds4<2>(x + 2 * XDIM, s_xn[3], XDIM);
        glds4<2>(pl.X0 + (size_t)r * XDIM, s_x0, XDIM);
        glds4<1>(pl.mask + r, s_misc + 27, 1);
    } else {
        stage_pose_part<3>(pm, stg, xrow, camrow);
        glds4<2>(dX + (size_t)r * XDIM, s_dx, XDIM);         // the row a separate param_loss_kernel launch initialised
    }
    int pl_g = clip_n > 0 ? (int)blockIdx.x % clip_n : pl.frame0 + (int)blockIdx.x, pl_n = pl.n_total, clip_k = clip_of_row(r, clip_n);
    float w_rec = pl.w_rec, w_sm = pl.w_sm, w_ws = pl.w_ws;
    if (ctab) {                                              // (kernel-uniform; wave-uniform scalar loads)
        const clip_row_cptr cr = clip_row_at(ctab, r);
        clip_k = cr->k; pl_g = cr->g; pl_n = cr->n;
        w_rec = cr->w_rec; w_sm = cr->w_sm; w_ws = cr->w_ws;
    }
    const float sc_v = scale[clip_k];
    __shared__ float s_csum[POSE_NW];
    if (pl.cdist) {                                          // (kernel-uniform) contact_loss_rows_kernel's sum, same threads, same order
        float v = 0.f;
        for (int c = threadIdx.x; c < pl.cnc; c += 256) { float d; v += contact_term(pl.cdist[(size_t)r * pl.cnc + c], &d); }
        v = wave_sum64(v);
        if ((threadIdx.x & 63) == 0) s_csum[threadIdx.x >> 6] = v;
    }
    __syncthreads();                                         // (every wave waits for its copies: vmcnt(0) in front of the barrier)
    if (pl.cdist && threadIdx.x == 0) pl.loss_rows[(size_t)r * LROW + 3] = (s_csum[0] + s_csum[1]) + (s_csum[2] + s_csum[3]);
    // (all four waves stay for their share of pose_backward, split)
    FDC_FR_STAMP(1, 7);
    const PoseModel pml = stage_pose_model(pm, stg);
    const bool w0 = threadIdx.x < 64;
#if FDC_PB_REPROJ
    if (wave == 2) {                                     // (wave-uniform; the host keeps jn >= NJW while the term is on: rows 0..22 of sc.G are staged)
        const int j = (int)(threadIdx.x & 63);
        V3 dJ = v3(0.f, 0.f, 0.f);
        float val = 0.f;
        if (j < NJW) {
            const V3 p = g_trn(sc.G[j]) + v3(stg.x[X_TRANSL], stg.x[X_TRANSL + 1], stg.x[X_TRANSL + 2])
                         + v3(stg.x[X_CAMT], stg.x[X_CAMT + 1], stg.x[X_CAMT + 2]);      // cam_t as it is: not times `scale`
            val = reproj_joint(rp, p, s_kp[3 * j], s_kp[3 * j + 1], s_kp[3 * j + 2], &dJ);
        }
        if (j < NJ) { s_dJb[3 * j] = dJ.x; s_dJb[3 * j + 1] = dJ.y; s_dJb[3 * j + 2] = dJ.z; }
        const float sx = wave_sum64(dJ.x), sy = wave_sum64(dJ.y), sz = wave_sum64(dJ.z);
        if (j == 0) { s_rp[0] = sx; s_rp[1] = sy; s_rp[2] = sz; }
        if (rp.loss_rows) {                              // kernel-uniform: logging iterations only
            val = wave_sum64(val);
            if (j == 0) rp.loss_rows[(size_t)r * LROW + 6] = val;
        }
    }
#endif
    if (dPF2) {
        const float* p2 = &sc.dR[0][0];
        for (int e = threadIdx.x; e < NPFX; e += 64 * POSE_NW) s_dPF[e] += p2[e];
        if (!pl.X0) __syncthreads();                         // (else: the barrier behind the loss prologue covers it)
    }
    if (pl.X0) {
        // param_loss_kernel's gradients formed here: dX row (=) data + temporal terms on the raw rows, world-smoothing
        // gradient of this frame's joints into LDS instead of a round trip through dJw
        const int g = pl_g;
        const float lmask = s_misc[27];
        float l_rec = 0.f, l_vp = 0.f, l_sm = 0.f, l_ws = 0.f;
        // (two waves side by side: the first takes the parameter row's terms, the second the world joints')
        if (w0) {
            for (int e = threadIdx.x; e < XDIM; e += 64) {
                const float xc = stg.x[e];
                float rec = 0.f, sm = 0.f;
                s_dx[e] = param_loss_grad(g, pl_n, g >= 2 ? s_xn[0][e] : 0.f, g >= 1 ? s_xn[1][e] : 0.f, xc,
                                          g + 1 < pl_n ? s_xn[2][e] : 0.f, g + 2 < pl_n ? s_xn[3][e] : 0.f,
                                          s_x0[e], lmask, w_rec, w_sm, &rec, &sm);
                l_rec += rec; l_sm += sm;
                if (e >= X_LATENT && e < X_LATENT + 32) l_vp += xc * xc;
            }
            if (pl.loss_rows) {                              // kernel-uniform: logging iterations only
                l_rec = wave_sum64(l_rec); l_vp = wave_sum64(l_vp); l_sm = wave_sum64(l_sm);
                if (threadIdx.x == 0) {
                    float* lr = pl.loss_rows + (size_t)r * LROW;
                    lr[0] = l_rec; lr[1] = l_vp; lr[2] = l_sm;
                }
            }
        } else if (threadIdx.x < 128 && (pl.world_grad || pl.loss_rows)) {
            for (int e = threadIdx.x - 64; e < NJW * 3; e += 64) {
                float ws = 0.f;
                s_dJw[e] = world_smooth_grad(g, pl_n, g >= 1 ? s_jw[0][e] : 0.f, s_jw[1][e], g + 1 < pl_n ? s_jw[2][e] : 0.f,
                                             w_ws, &ws);
                l_ws += ws;
            }
            if (pl.loss_rows) {
                l_ws = wave_sum64(l_ws);
                if (threadIdx.x == 64) pl.loss_rows[(size_t)r * LROW + 4] = l_ws;
            }
        }
        __syncthreads();
    }
#if FDC_PB_REPROJ
    // (the unfused parameter-loss path, pl.X0 == nullptr, is taken only with a DCT term set up, which the library refuses while this
    //  term is on: kept so that the kernel is right on either path, not reached through the library today)
    if (!pl.X0) __syncthreads();                         // (else: the barrier behind the loss prologue covers s_dJb and s_rp)
    // d cam_t = sum_j dJb_j, no factor `scale`: after the prologue's assignment of s_dx, ahead of pose_backward's first barrier
    if (threadIdx.x < 3) s_dx[X_CAMT + threadIdx.x] += s_rp[threadIdx.x];
#endif
    const float* dJw_row = (pl.X0 && pl.world_grad) ? s_dJw : (dJw ? dJw + (size_t)r * NJW * 3 : nullptr);
    pose_backward(pml, stg.x, s_O, stg.cam, sc_v,
                  (const float*)nullptr, s_Jr, (const float*)nullptr,     // (Rm: not read any more; G: already in sc.G)
                  dA ? &sc.dG[0][0] : nullptr, dPF ? s_dPF : nullptr,
                  dJw_row, dMv ? s_misc : nullptr,
                  dsv ? s_misc + 12 : nullptr, dbeta_v ? (dPF2 ? s_dPF + NPF : s_misc + 16) : nullptr,
                  dtransl_v ? s_misc + 13 : nullptr, sc, s_dx,
                  dO + (size_t)r * ODIM, dCAM + (size_t)r * 16, dscale_row + r, threadIdx.x, 64, SyncBlock(),
                  nullptr, nullptr,
#if FDC_PB_REPROJ
                  s_dJb,
#else
                  nullptr,
#endif
                  1, jn, jr, nlev);
    __syncthreads();
    for (int e = threadIdx.x; e < XDIM; e += 256) dX[(size_t)r * XDIM + e] = s_dx[e];
}
