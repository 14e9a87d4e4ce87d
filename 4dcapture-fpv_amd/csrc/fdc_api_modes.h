// C-ABI, part 3: mode 'dct', the per-frame inner fit (Adam and batched L-BFGS), checkpoint state / finite check, the per-frame
// smoother of optimization.py.  Part of csrc/fdcap.hip.
#pragma once

extern "C" {

// ---- mode 'dct' (global_optimization.py:595-630) -----------------------------------------------
int fdcap_opt_set_dct(fdcap_ctx* c, const float* dct_mtx, int32_t T, int32_t C, const float* c_dct_d, void* stream) {
    if (opt_is_batch(c)) return FDCAP_E_STATE;           // (a batch of clips: mode 'global' only)
    if (opt_has_reproj(c)) return FDCAP_E_STATE;         // (the clip-level reprojection term is on: mode 'global' only)
    if (!c || !c->opt || !dct_mtx || !c_dct_d || T <= 0 || T > DCT_MAXT || C <= 0 || C > DCT_MAXC) return FDCAP_E_ARG;
    OptState* o = c->opt;
    const int W = o->cfg.n_total / T;
    if (W <= 0) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)W * 69 * C;
    HIP_TRY(o->dctD.upload(dct_mtx, (size_t)T * C));
    HIP_TRY(o->dctCoef.ensure(n));
    HIP_TRY(o->dctM.ensure(n));
    HIP_TRY(o->dctV.ensure(n));
    HIP_TRY(hipMemcpyAsync(o->dctCoef.p, c_dct_d, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(o->dctM.p, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(o->dctV.p, 0, n * sizeof(float), st));
    o->dctT = T; o->dctC = C; o->dctW = W;
    return FDCAP_OK;
}

// Mode 'dct' for whole clips (fdcap_opt_create_clips[_var], or one clip): the window table, each clip's first window, the zero row of
// the clips' objective weights and -- clips of different lengths -- the fourth record set, under the second phase's weights
// (:620: rec 0.5, contact 0.1; fdcap_opt_run_dct refuses other multipliers on such a batch, it never replaces them).  One clip
// takes fdcap_opt_set_dct's state and, from then on, the launches of a stand-alone fit.
int fdcap_opt_set_dct_clips(fdcap_ctx* c, const float* dct_mtx, int32_t T, int32_t C, const float* c_dct_d, void* stream) {
    if (!c || !c->opt) return FDCAP_E_STATE;
    OptState* o = c->opt;
    if (!opt_whole_clips(o)) return FDCAP_E_STATE;       // (a shard of a clip: FittingOP's loop, window by window)
    if (o->multi_scene()) return FDCAP_E_STATE;          // (clips of several scenes: mode 'global' only)
    if (opt_has_reproj(c)) return FDCAP_E_STATE;         // (the clip-level reprojection term is on: mode 'global' only)
    if (!dct_mtx || !c_dct_d || T <= 0 || T > DCT_MAXT || C <= 0 || C > DCT_MAXC) return FDCAP_E_ARG;
    if (o->nclip == 1) return fdcap_opt_set_dct(c, dct_mtx, T, C, c_dct_d, stream);
    const int K = o->nclip;
    const int32_t* len = o->clip_lens.data();
    for (int k = 0; k < K; ++k) if (len[k] / T <= 0) return FDCAP_E_ARG;        // (every clip has a window, as a stand-alone fit must)
    hipStream_t st = (hipStream_t)stream;
    o->dct_wstart_h = dct_window_starts(K, len, T);
    const std::vector<DctWindow> tab = dct_window_table(K, len, T);
    const int W = o->dct_wstart_h[(size_t)K];
    const size_t n = (size_t)W * 69 * C;
    HIP_TRY(o->dctD.upload(dct_mtx, (size_t)T * C));
    HIP_TRY(o->dct_wtab.upload(tab.data(), tab.size()));
    HIP_TRY(o->dct_wstart.upload(o->dct_wstart_h.data(), o->dct_wstart_h.size()));
    HIP_TRY(o->dct_wk.ensure((size_t)3 * K));
    HIP_TRY(hipMemsetAsync(o->dct_wk.p, 0, (size_t)3 * K * sizeof(float), st));
    for (int s = 0; s < 3; ++s) o->dct_wk_weight[s] = 0.f;
    o->dct_lw = dct_phase2_weights(0.f, 0.5f, 0.1f);
    if (o->ragged) {
        const std::vector<ClipRow> rows = clip_rows_build_dct2(K, len, o->dct_lw.rec, o->dct_lw.contact, o->cfg.weight_loss_rec, o->cfg.weight_contact, c->nc);
        if (rows.size() != (size_t)o->R) return FDCAP_E_STATE;
        HIP_TRY(o->clip_rows_dct.upload(rows.data(), rows.size()));
    }
    HIP_TRY(o->dctCoef.ensure(n));
    HIP_TRY(o->dctM.ensure(n));
    HIP_TRY(o->dctV.ensure(n));
    HIP_TRY(hipMemcpyAsync(o->dctCoef.p, c_dct_d, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(o->dctM.p, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(o->dctV.p, 0, n * sizeof(float), st));
    o->dctT = T; o->dctC = C; o->dctW = W;
    o->dct_clips = true;
    return FDCAP_OK;
}

// each clip's first window in c_dct, starts[n_clips + 1] (the last entry: fdcap_opt_dct_windows' total); n = n_clips + 1
int fdcap_opt_dct_clip_windows(fdcap_ctx* c, int32_t* starts, int32_t n) {
    if (!c || !c->opt || c->opt->dctW <= 0) return FDCAP_E_STATE;
    const OptState* o = c->opt;
    if (!starts || n != o->nclip + 1) return FDCAP_E_ARG;
    if (o->dct_clips) for (int k = 0; k < n; ++k) starts[k] = o->dct_wstart_h[(size_t)k];
    else { starts[0] = 0; starts[1] = o->dctW; }
    return FDCAP_OK;
}

// `iters` Adam iterations on c_dct from step counter step0 in ONE launch: one clip (or one rank's windows of one), or every window
// of a batch (fdcap_opt_run_dct) through the window table
static int opt_dct_fit_impl(fdcap_ctx* c, int32_t iters, int32_t step0, float weight, float* obj_hist, int32_t log_stride, hipStream_t st) {
    { int es_ = opt_sync(c, st); if (es_) return es_; }
    OptState* o = c->opt;
    if (o->dctW <= 0) return FDCAP_E_STATE;
    const fdcap_opt_config& cf = o->cfg;
    const int T = o->dctT;
    // windows that lie completely inside this rank's frames (the caller shards on window boundaries); a batch: all of them
    const int w0 = o->dct_clips ? 0 : (cf.frame0 + T - 1) / T;
    const int w1 = o->dct_clips ? o->dctW : std::min((cf.frame0 + cf.n_local) / T, o->dctW);
    if (iters == 0 || w1 <= w0) return FDCAP_OK;
    // weight 0: every gradient is exactly zero whatever the trajectories are (Adam coasts on its moments: the torch < 2
    // zero_grad semantics of a frozen c_dct) -- no forward needed
    if (weight != 0.f) {
        int row_lo, row_hi;
        opt_row_range(o, 1, &row_lo, &row_hi);
        int e = opt_pose_forward(c, row_lo, row_hi, st);
        if (e) return e;
    }
    o->adam_tab_h.resize(iters);
    for (int i = 0; i < iters; ++i) o->adam_tab_h[i] = adam_scalars(cf.lr, step0 + i + 1);
    HIP_TRY(o->adam_tab.ensure(iters));
    HIP_TRY(hipMemcpyAsync(o->adam_tab.p, o->adam_tab_h.data(), (size_t)iters * sizeof(AdamScalars), hipMemcpyHostToDevice, st));
    if (o->dct_clips) {
        const float* wk = nullptr;
        { int ew = opt_dct_clip_weights(o, 1, weight, st, &wk); if (ew) return ew; }
        hipLaunchKernelGGL(dct_fit_clips_kernel, dim3(o->dctW * 69), dim3(64), 0, st, o->Jw.p, o->dct_wtab.p, T, o->dctC, o->dctD.p, o->dctCoef.p,
                           o->dctM.p, o->dctV.p, o->adam_tab.p, iters, wk, obj_hist, log_stride > 0 ? log_stride : 1);
    } else
        hipLaunchKernelGGL(dct_fit_kernel, dim3((w1 - w0) * 69), dim3(64), 0, st, o->Jw.p, 2 + (w0 * T - cf.frame0), T, o->dctC,
                           o->dctD.p, o->dctCoef.p, o->dctM.p, o->dctV.p, w0, o->adam_tab.p, iters,
                           weight / (69.f * (float)o->dctW), obj_hist, log_stride > 0 ? log_stride : 1);
    return (int)hipGetLastError();
}

int fdcap_opt_dct_fit(fdcap_ctx* c, int32_t iters, int32_t step0, float weight, float* obj_hist, int32_t log_stride,
                      void* stream) {
    if (opt_is_batch(c)) return FDCAP_E_STATE;           // (a batch of clips: through fdcap_opt_run_dct only)
    if (opt_has_reproj(c)) return FDCAP_E_STATE;         // (the clip-level reprojection term is on: mode 'global' only)
    if (!c || !c->opt || iters < 0 || step0 < 0 || (obj_hist && log_stride <= 0)) return FDCAP_E_ARG;
    return opt_dct_fit_impl(c, iters, step0, weight, obj_hist, log_stride, (hipStream_t)stream);
}

// one backward of the second phase's loss (:620) for one clip, one rank's share of one, or a batch (fdcap_opt_run_dct)
static int opt_backward_dct_impl(fdcap_ctx* c, float w_dct, float w_rec, float w_contact, int32_t log_terms, hipStream_t st) {
    if (c->opt->dctW <= 0) return FDCAP_E_STATE;
    return opt_backward_impl(c, dct_phase2_weights(w_dct, w_rec, w_contact), log_terms, st);
}

int fdcap_opt_backward_dct(fdcap_ctx* c, float w_dct, float w_rec, float w_contact, int32_t log_terms, void* stream) {
    if (opt_is_batch(c)) return FDCAP_E_STATE;           // (a batch of clips: through fdcap_opt_run_dct only)
    if (opt_has_reproj(c)) return FDCAP_E_STATE;         // (the clip-level reprojection term is on: mode 'global' only)
    if (!c || !c->opt) return FDCAP_E_STATE;
    return opt_backward_dct_impl(c, w_dct, w_rec, w_contact, log_terms, (hipStream_t)stream);
}

int fdcap_opt_set_dct_coef(fdcap_ctx* c, const float* c_dct_d, void* stream) {
    if (opt_is_batch(c) && c->opt->dctW <= 0) return FDCAP_E_STATE;     // (a batch of clips without a DCT term: fdcap_opt_set_dct_clips)
    if (!c || !c->opt || !c_dct_d) return FDCAP_E_ARG;
    OptState* o = c->opt;
    if (o->dctW <= 0) return FDCAP_E_STATE;
    HIP_TRY(hipMemcpyAsync(o->dctCoef.p, c_dct_d, (size_t)o->dctW * 69 * o->dctC * sizeof(float), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return FDCAP_OK;
}

int fdcap_opt_get_dct(fdcap_ctx* c, float* c_dct_d, void* stream) {
    if (opt_is_batch(c) && c->opt->dctW <= 0) return FDCAP_E_STATE;     // (a batch of clips without a DCT term: fdcap_opt_set_dct_clips)
    if (!c || !c->opt || !c_dct_d) return FDCAP_E_ARG;
    OptState* o = c->opt;
    if (o->dctW <= 0) return FDCAP_E_STATE;
    HIP_TRY(hipMemcpyAsync(c_dct_d, o->dctCoef.p, (size_t)o->dctW * 69 * o->dctC * sizeof(float), hipMemcpyDeviceToDevice,
                           (hipStream_t)stream));
    return FDCAP_OK;
}
// Adam's moments of c_dct, [W,69,C] each: what a checkpoint of mode 'dct' needs next to fdcap_opt_get_dct / fdcap_opt_export_state
static int dct_state_copy(fdcap_ctx* c, float* m_d, float* v_d, bool out, hipStream_t st) {
    if (opt_is_batch(c) && c->opt->dctW <= 0) return FDCAP_E_STATE;     // (a batch of clips without a DCT term: fdcap_opt_set_dct_clips)
    if (!c || !c->opt || !m_d || !v_d) return FDCAP_E_ARG;
    OptState* o = c->opt;
    if (o->dctW <= 0) return FDCAP_E_STATE;
    const size_t bytes = (size_t)o->dctW * 69 * o->dctC * sizeof(float);
    HIP_TRY(hipMemcpyAsync(out ? m_d : o->dctM.p, out ? o->dctM.p : m_d, bytes, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(out ? v_d : o->dctV.p, out ? o->dctV.p : v_d, bytes, hipMemcpyDeviceToDevice, st));
    return FDCAP_OK;
}
int fdcap_opt_get_dct_state(fdcap_ctx* c, float* m_d, float* v_d, void* stream) { return dct_state_copy(c, m_d, v_d, true, (hipStream_t)stream); }
int fdcap_opt_set_dct_state(fdcap_ctx* c, const float* m_d, const float* v_d, void* stream) {
    return dct_state_copy(c, (float*)m_d, (float*)v_d, false, (hipStream_t)stream);
}
int32_t fdcap_opt_dct_windows(fdcap_ctx* c, int32_t* w0, int32_t* w1) {
    if (!c || !c->opt || c->opt->dctW <= 0) return 0;
    if (c->opt->dct_clips) {                             // a batch: every window of every clip (fdcap_opt_dct_clip_windows: per clip)
        if (w0) *w0 = 0;
        if (w1) *w1 = c->opt->dctW;
        return c->opt->dctW;
    }
    const fdcap_opt_config& cf = c->opt->cfg;
    const int T = c->opt->dctT;
    int a = (cf.frame0 + T - 1) / T, b = std::min((cf.frame0 + cf.n_local) / T, c->opt->dctW);
    if (w0) *w0 = a;
    if (w1) *w1 = std::max(a, b);
    return c->opt->dctW;
}

// ---- per-frame inner fit with a 2D reprojection term (outside the reference) ------
int fdcap_opt_set_keypoints(fdcap_ctx* c, const float* kp_d, void* stream) {
    if (opt_is_batch(c)) return FDCAP_E_STATE;           // (a batch of clips: mode 'global' only)
    if (!c || !c->opt || !kp_d) return FDCAP_E_ARG;
    OptState* o = c->opt;
    const size_t n = (size_t)o->cfg.n_local * NJW * 3;
    HIP_TRY(o->kp2d.ensure(n));
    HIP_TRY(hipMemcpyAsync(o->kp2d.p, kp_d, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    o->kp_mapped = false;
    return FDCAP_OK;
}

// ---- ... on a detector's keypoints: the keypoint map (csrc/fdc_keypoints.h) --------------------------------------------------
static_assert(KP_MAX == FDCAP_MAX_KEYPOINTS, "fdc_keypoints.h restates the largest map");
int fdcap_set_keypoint_map(fdcap_ctx* c, int32_t n_kp, const int32_t* joint, const int32_t* tri, const float* bary) {
    if (!c) return FDCAP_E_ARG;
    KeypointTables t;
    if (keypoint_map_build(n_kp, joint, tri, bary, c->V, &t)) return FDCAP_E_ARG;
    if (c->opt) return FDCAP_E_STATE;                  // (see fdcap_set_scene: a live optimiser may hold keypoints in this map's order)
    KeypointSet& ks = c->kpset;
    ks.release();
    if (n_kp == 0) return FDCAP_OK;
    const int nr = t.nr, np = t.np, nu = nr + np, V = c->V;
    // skinning weights of the set: a real vertex's non-zero ones, a pseudo-vertex's single 1 on its joint; and their transpose
    int K = 1;
    for (int u = 0; u < nr; ++u) {
        int k = 0;
        for (int j = 0; j < NJ; ++j) k += c->h_lbs[(size_t)t.real_ids[u] * NJ + j] != 0.f;
        K = std::max(K, k);
    }
    std::vector<int32_t> wj((size_t)nu * K, 0), csc_start(NJ + 1, 0), csc_u;
    std::vector<float> ww((size_t)nu * K, 0.f), csc_w, vt((size_t)nr * 3);
    auto weight = [&](int u, int j) { return u < nr ? c->h_lbs[(size_t)t.real_ids[u] * NJ + j] : (t.pseudo_joint[u - nr] == j ? 1.f : 0.f); };
    for (int u = 0; u < nu; ++u) {
        int k = 0;
        for (int j = 0; j < NJ; ++j) { const float w = weight(u, j); if (w != 0.f) { wj[(size_t)u * K + k] = j; ww[(size_t)u * K + k] = w; ++k; } }
        if (u < nr) for (int e = 0; e < 3; ++e) vt[3 * u + e] = c->h_vt[(size_t)3 * t.real_ids[u] + e];
    }
    for (int j = 0; j < NJ; ++j) {
        csc_start[j] = (int32_t)csc_u.size();
        for (int u = 0; u < nu; ++u) { const float w = weight(u, j); if (w != 0.f) { csc_u.push_back(u); csc_w.push_back(w); } }
    }
    csc_start[NJ] = (int32_t)csc_u.size();
    // the set's blend matrix [posedirs ; shapedirs^T]: the real vertices' columns gathered on the device as every vertex set's
    // (build_skin_set), a pseudo-vertex's columns zero but for Jd_j^T in the betas' rows (its d betas through the panel product);
    // the real columns' transpose for the in-kernel backward; and the panels of both products
    const int ldb = (3 * nu + 3) & ~3, ldr = (3 * nr + 3) & ~3;
    std::vector<float> b((size_t)NPFX * ldb, 0.f), bt((size_t)3 * nr * NPFX);
    if (nr > 0) {
        DevBuf<float> d_b;
        DevBuf<int> d_ids;
        HIP_TRY(d_b.ensure((size_t)NPFX * ldr));
        HIP_TRY(d_ids.upload(t.real_ids.data(), t.real_ids.size()));
        hipLaunchKernelGGL(blend_rows_gather_kernel, dim3((ldr + 255) / 256, NPFX), dim3(256), 0, 0, c->d_posedirs.p, c->d_S10.p, V, d_ids.p, nr, ldr, d_b.p);
        const hipError_t e_ = hipGetLastError(), es_ = hipDeviceSynchronize();   // (the two are freed at the brace: wait, whatever the launch said)
        HIP_TRY(e_ != hipSuccess ? e_ : es_);
        std::vector<float> br((size_t)NPFX * ldr);
        HIP_TRY(hipMemcpy(br.data(), d_b.p, br.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int k = 0; k < NPFX; ++k)
            for (int col = 0; col < 3 * nr; ++col) bt[(size_t)col * NPFX + k] = b[(size_t)k * ldb + col] = br[(size_t)k * ldr + col];
    }
    if (np > 0) {
        std::vector<float> jd((size_t)NJ * 3 * NBETA);
        HIP_TRY(hipMemcpy(jd.data(), c->Jd.p, jd.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int i = 0; i < np; ++i)
            for (int e = 0; e < 3; ++e)
                for (int l = 0; l < NBETA; ++l) b[(size_t)(NPF + l) * ldb + 3 * (nr + i) + e] = jd[(size_t)(3 * t.pseudo_joint[i] + e) * NBETA + l];
    }
    SkinSet& ss = ks.ss;
    ss.nv = nu; ss.ldp = ldb;
    HIP_TRY(ss.posedirs.upload(b.data(), b.size()));
    HIP_TRY(ks.Bt.upload(bt.data(), bt.size()));
    if (nu > 0) {
        const float* pd = ss.posedirs.p;
        const size_t pdn = b.size();
        int nt = 0, ns = 0, e = panel_pack_dev(pd, pdn, ldb, 1, NPFX, 3 * nu, ss.pn_fwd_f, &nt, &ns);
        if (e) return e;
        ss.pn_fwd.f = (const float4*)ss.pn_fwd_f.p; ss.pn_fwd.ntile = nt; ss.pn_fwd.nss = ns;
        e = panel_pack_dev(pd, pdn, 1, ldb, 3 * nu, NPFX, ss.pn_bwd_f, &nt, &ns);
        if (e) return e;
        ss.pn_bwd.f = (const float4*)ss.pn_bwd_f.p; ss.pn_bwd.ntile = nt; ss.pn_bwd.nss = ns;
        e = pnf_pack_dev(pd, pdn, ldb, 1, NPFX, 3 * nu, ss.pn_fwd3_f, ss.pn_fwd3_s, &ss.pn_fwd3.ntile, &ss.pn_fwd3.nst);
        if (e) return e;
        ss.pn_fwd3.f = (const uint4*)ss.pn_fwd3_f.p; ss.pn_fwd3.isc = ss.pn_fwd3_s.p;
        e = pnf_pack_dev(pd, pdn, 1, ldb, 3 * nu, NPFX, ss.pn_bwd3_f, ss.pn_bwd3_s, &ss.pn_bwd3.ntile, &ss.pn_bwd3.nst);
        if (e) return e;
        ss.pn_bwd3.f = (const uint4*)ss.pn_bwd3_f.p; ss.pn_bwd3.isc = ss.pn_bwd3_s.p;
        HIP_TRY(hipDeviceSynchronize());
    }
    HIP_TRY(ks.kjoint.upload(t.kjoint.data(), t.kjoint.size())); HIP_TRY(ks.kref.upload(t.kref.data(), t.kref.size()));
    HIP_TRY(ks.kbary.upload(t.kbary.data(), t.kbary.size()));
    HIP_TRY(ks.vl_start.upload(t.vl_start.data(), t.vl_start.size())); HIP_TRY(ks.vl_k.upload(t.vl_k.data(), t.vl_k.size()));
    HIP_TRY(ks.vl_w.upload(t.vl_w.data(), t.vl_w.size()));
    HIP_TRY(ks.jl_start.upload(t.jl_start.data(), t.jl_start.size())); HIP_TRY(ks.jl_k.upload(t.jl_k.data(), t.jl_k.size()));
    HIP_TRY(ks.pjoint.upload(t.pseudo_joint.data(), t.pseudo_joint.size()));
    HIP_TRY(ks.wj.upload(wj.data(), wj.size())); HIP_TRY(ks.ww.upload(ww.data(), ww.size())); HIP_TRY(ks.vt.upload(vt.data(), vt.size()));
    HIP_TRY(ks.csc_start.upload(csc_start.data(), csc_start.size())); HIP_TRY(ks.csc_u.upload(csc_u.data(), csc_u.size()));
    HIP_TRY(ks.csc_w.upload(csc_w.data(), csc_w.size()));
    if (!c->h_E10.empty()) {                           // the free expression's tables (fdcap_opt_set_expression)
        const int lde = std::max(ldb, 4);
        std::vector<float> es((size_t)NEXPR * lde, 0.f);
        for (int u = 0; u < nu; ++u)
            for (int e = 0; e < 3; ++e)
                for (int l = 0; l < NEXPR; ++l)
                    es[(size_t)l * lde + 3 * u + e] = u < nr ? c->h_E10[((size_t)3 * t.real_ids[u] + e) * NEXPR + l]
                                                             : c->h_JE[(size_t)(3 * t.pseudo_joint[u - nr] + e) * NEXPR + l];
        HIP_TRY(ks.E.upload(es.data(), es.size())); HIP_TRY(ks.JE.upload(c->h_JE.data(), c->h_JE.size()));
        ks.lde = lde;
    }
    ks.K = K;
    ks.h = std::move(t);                               // (last: a failure above leaves no map)
    return FDCAP_OK;
}

int fdcap_opt_set_keypoints_mapped(fdcap_ctx* c, const float* kp_d, void* stream) {
    if (opt_is_batch(c)) return FDCAP_E_STATE;           // (a batch of clips: mode 'global' only)
    if (!c || !c->opt || !kp_d) return FDCAP_E_ARG;
    if (c->kpset.h.n_kp <= 0) return FDCAP_E_STATE;
    OptState* o = c->opt;
    const size_t n = (size_t)o->cfg.n_local * c->kpset.h.n_kp * 3;
    HIP_TRY(o->kp2d.ensure(n));
    HIP_TRY(hipMemcpyAsync(o->kp2d.p, kp_d, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    o->kp_mapped = true;
    o->kp_panel = kp_blend_by_panels(o->cfg.n_local, 3 * c->kpset.h.nr);
    if (o->kp_panel) {
        const size_t nv = (size_t)o->cfg.n_local * 3 * c->kpset.h.nu();
        HIP_TRY(o->kpV.ensure(nv));
        HIP_TRY(o->kpdV.ensure(nv));
    }
    return FDCAP_OK;
}

int fdcap_debug_keypoints3d(fdcap_ctx* c, float* out_d, void* stream) {
    if (opt_is_batch(c)) return FDCAP_E_STATE;
    if (!c || !c->opt || !out_d) return FDCAP_E_ARG;
    if (c->kpset.h.n_kp <= 0) return FDCAP_E_STATE;
    hipStream_t st = (hipStream_t)stream;
    { int es_ = opt_sync(c, st); if (es_) return es_; }
    OptState* o = c->opt;
    int row_lo, row_hi;
    opt_row_range(o, 1, &row_lo, &row_hi);
    int e = opt_pose_forward(c, row_lo, row_hi, st);
    if (e) return e;
    if (o->expr_on) {                                         // (positions only: no gradient is written)
        const ExprIO ex = c->expr_view(o->psi.p, nullptr, 0.f);
        if (o->jaw_on)
            hipLaunchKernelGGL((fit2d_kp_expr_jaw_kernel<true, false>), dim3(o->cfg.n_local), dim3(KP_NT), 0, st, Fit2dStage(), c->kp_view(), o->X.p, o->PF.p,
                               o->A.p, o->M.p, o->scale.p, o->Jw.p, (const float*)nullptr, 2, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                               (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, (double*)nullptr, (float*)nullptr, out_d,
                               (const float*)nullptr, (float*)nullptr, JawIO{o->jaw.p, o->jawR9.p, {0.f, 0.f, 0.f}}, ex);
        else
            hipLaunchKernelGGL((fit2d_kp_expr_kernel<true, false>), dim3(o->cfg.n_local), dim3(KP_NT), 0, st, Fit2dStage(), c->kp_view(), o->X.p, o->PF.p,
                               o->A.p, o->M.p, o->scale.p, o->Jw.p, (const float*)nullptr, 2, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                               (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr, (double*)nullptr, (float*)nullptr, out_d,
                               (const float*)nullptr, (float*)nullptr, ex);
    } else
    if (o->jaw_on)
        hipLaunchKernelGGL((fit2d_kp_jaw_kernel<true, false>), dim3(o->cfg.n_local), dim3(KP_NT), 0, st, Fit2dStage(), c->kp_view(), o->X.p, o->PF.p, o->A.p,
                           o->M.p, o->scale.p, o->Jw.p, (const float*)nullptr, 2, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                           (float*)nullptr, (float*)nullptr, (float*)nullptr, (double*)nullptr, (float*)nullptr, out_d, (const float*)nullptr,
                           (float*)nullptr, JawIO{o->jaw.p, o->jawR9.p, {0.f, 0.f, 0.f}});
    else
    hipLaunchKernelGGL((fit2d_kp_kernel<true, false>), dim3(o->cfg.n_local), dim3(KP_NT), 0, st, Fit2dStage(), c->kp_view(), o->X.p, o->PF.p, o->A.p, o->M.p,
                       o->scale.p, o->Jw.p, (const float*)nullptr, 2, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                       (float*)nullptr, (float*)nullptr, (float*)nullptr, (double*)nullptr, (float*)nullptr, out_d, (const float*)nullptr,
                       (float*)nullptr);
    return (int)hipGetLastError();
}

static int fit2d_eval(fdcap_ctx* c, const fdcap_fit2d_stage* sg, double* losses, float* floss, hipStream_t st, bool fold = true);
int fdcap_opt_backward_fit2d(fdcap_ctx* c, const fdcap_fit2d_stage* sg, int32_t log_terms, void* stream) {
    if (opt_is_batch(c)) return FDCAP_E_STATE;           // (a batch of clips: mode 'global' only)
    if (!c || !c->opt || !sg) return FDCAP_E_ARG;
    { int es_ = opt_sync(c, (hipStream_t)stream); if (es_) return es_; }
    OptState* o = c->opt;
    if (!o->kp2d.p) return FDCAP_E_STATE;
    hipStream_t st = (hipStream_t)stream;
    double* const losses = log_terms ? o->losses.p : nullptr;
    if (losses) HIP_TRY(hipMemsetAsync(losses, 0, FDCAP_NUM_LOSSES * sizeof(double), st));
    // (the latent gradient stays in the VPoser backward's four partials: fdcap_opt_step_x / fdcap_opt_get_grads add them)
    return fit2d_eval(c, sg, losses, nullptr, st, false);
}

static_assert(FIT2D_MAX_BEND == FDCAP_MAX_BEND_TERMS, "fdc_fit2d.h restates the longest list of bending terms");
int fdcap_opt_set_fit2d_extra(fdcap_ctx* c, const fdcap_fit2d_extra* ex) {
    if (!c || !c->opt || opt_is_batch(c) || !opt_whole_clips(c->opt)) return FDCAP_E_STATE;
    Fit2dBend b = {};
    if (ex) {
        if (fit2d_bend_check(ex->w_bend, ex->n_bend, ex->joint, ex->axis, ex->sign)) return FDCAP_E_ARG;
        for (int e = 0; e < 3; ++e) if (!std::isfinite(ex->w_jaw[e])) return FDCAP_E_ARG;
        b.w = ex->w_bend; b.n = ex->w_bend != 0.f ? ex->n_bend : 0;      // (weight 0: every term and gradient an exact zero -- no launch)
        for (int t = 0; t < b.n; ++t) { b.joint[t] = ex->joint[t]; b.axis[t] = ex->axis[t]; b.sign[t] = ex->sign[t]; }
    }
    for (int e = 0; e < 3; ++e) c->opt->w_jaw[e] = ex ? ex->w_jaw[e] : 0.f;
    c->opt->bend = b;
    return FDCAP_OK;
}

// ---- the free jaw (csrc/fdc_keypoints.h) -----------------------------------------------------------------------------------------
static JawGradIn opt_jaw_grad_in(fdcap_ctx* c) {
    OptState* o = c->opt;
    JawGradIn jg;
    jg.jaw = o->jaw.p; jg.R9 = o->jawR9.p;
    jg.gP = o->jaw_gp ? o->dPF.p + (size_t)2 * NPFX + 9 * (JAW_J - 1) : nullptr; jg.gp_stride = NPFX;
    for (int e = 0; e < 3; ++e) jg.w[e] = o->w_jaw[e];
    return jg;
}
int fdcap_opt_set_jaw(fdcap_ctx* c, const float* jaw_d, void* stream) {
    if (!c || !c->opt || opt_is_batch(c) || !opt_whole_clips(c->opt)) return FDCAP_E_STATE;
    OptState* o = c->opt;
    hipStream_t st = (hipStream_t)stream;
    o->jaw_eval = false;
    if (!jaw_d) { o->jaw_on = false; return FDCAP_OK; }
    for (int j = 0; j < NJ; ++j) if (c->h_parents[j] == JAW_J) return FDCAP_E_ARG;      // (the leaf argument needs a leaf)
    const size_t n = (size_t)o->cfg.n_local;
    HIP_TRY(o->jaw.ensure(3 * n)); HIP_TRY(o->mJaw.ensure(3 * n)); HIP_TRY(o->vJaw.ensure(3 * n)); HIP_TRY(o->jawR9.ensure(9 * n));
    HIP_TRY(hipMemcpyAsync(o->jaw.p, jaw_d, 3 * n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(o->mJaw.p, 0, 3 * n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(o->vJaw.p, 0, 3 * n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(o->jawR9.p, 0, 9 * n * sizeof(float), st));
    o->jaw_on = true;
    return FDCAP_OK;
}
int fdcap_opt_get_jaw(fdcap_ctx* c, float* jaw_d, float* djaw_d, void* stream) {
    if (!c || !c->opt || !c->opt->jaw_on) return FDCAP_E_STATE;
    if (!jaw_d && !djaw_d) return FDCAP_E_ARG;
    OptState* o = c->opt;
    hipStream_t st = (hipStream_t)stream;
    const int n = o->cfg.n_local;
    if (djaw_d && !o->jaw_eval) return FDCAP_E_STATE;        // (no evaluation since fdcap_opt_set_jaw: no gradient)
    if (jaw_d) HIP_TRY(hipMemcpyAsync(jaw_d, o->jaw.p, (size_t)3 * n * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (djaw_d)
        hipLaunchKernelGGL(jaw_grad_kernel, dim3((n + 63) / 64), dim3(64), 0, st, opt_jaw_grad_in(c), n, djaw_d, (float*)nullptr, (float*)nullptr,
                           AdamScalars());
    return (int)hipGetLastError();
}

// ---- the free expression coefficients (csrc/fdc_keypoints.h) ------------------------------------------------------------------
int fdcap_opt_set_expression(fdcap_ctx* c, const float* expr_d, void* stream) {
    if (!c || !c->opt || opt_is_batch(c) || !opt_whole_clips(c->opt)) return FDCAP_E_STATE;
    OptState* o = c->opt;
    hipStream_t st = (hipStream_t)stream;
    o->expr_eval = false;
    if (!expr_d) { o->expr_on = false; return FDCAP_OK; }
    if (c->h_E10.empty()) return FDCAP_E_STATE;               // (a model without expression directions: num_shape < 20)
    for (int j = 1; j < NJ; ++j) if (c->h_parents[j] >= j) return FDCAP_E_ARG;         // (pose_forward's own condition: a joint follows its parent)
    const size_t n = (size_t)o->cfg.n_local * NEXPR;
    HIP_TRY(o->psi.ensure(n)); HIP_TRY(o->dpsi.ensure(n)); HIP_TRY(o->mPsi.ensure(n)); HIP_TRY(o->vPsi.ensure(n));
    HIP_TRY(hipMemcpyAsync(o->psi.p, expr_d, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemsetAsync(o->dpsi.p, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(o->mPsi.p, 0, n * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(o->vPsi.p, 0, n * sizeof(float), st));
    o->expr_on = true;
    return FDCAP_OK;
}
int fdcap_opt_get_expression(fdcap_ctx* c, float* expr_d, float* dexpr_d, void* stream) {
    if (!c || !c->opt || !c->opt->expr_on) return FDCAP_E_STATE;
    if (!expr_d && !dexpr_d) return FDCAP_E_ARG;
    OptState* o = c->opt;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)o->cfg.n_local * NEXPR;
    if (dexpr_d && !o->expr_eval) return FDCAP_E_STATE;      // (no evaluation since fdcap_opt_set_expression: no gradient)
    if (expr_d) HIP_TRY(hipMemcpyAsync(expr_d, o->psi.p, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (dexpr_d) HIP_TRY(hipMemcpyAsync(dexpr_d, o->dpsi.p, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    return FDCAP_OK;
}
int fdcap_opt_set_expression_prior(fdcap_ctx* c, float w_expr) {
    if (!c || !c->opt || opt_is_batch(c) || !opt_whole_clips(c->opt)) return FDCAP_E_STATE;
    if (!std::isfinite(w_expr)) return FDCAP_E_ARG;
    c->opt->w_expr = w_expr;
    return FDCAP_OK;
}

// ---- batched L-BFGS (csrc/fdc_lbfgs.h) ------------------------------------------------------------------------------
static int lbfgs_cfg_ok(const fdcap_lbfgs_config* cf) {
    return cf && cf->dim > 0 && cf->dim <= LB_DPAD && cf->history > 0 && cf->history <= LB_HMAX && cf->max_iter > 0 && cf->max_steps > 0 &&
           cf->max_ls > 0 && cf->lr > 0.f;
}
int fdcap_lbfgs_create(int32_t n, const fdcap_lbfgs_config* cf, fdcap_lbfgs** out) {
    if (!out || n <= 0 || !lbfgs_cfg_ok(cf)) return FDCAP_E_ARG;
    { int nd = 0; if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return FDCAP_E_NODEVICE; }
    fdcap_lbfgs* L = new (std::nothrow) fdcap_lbfgs();
    if (!L) return FDCAP_E_ARG;
    L->n = n;
    L->cf = {cf->dim, cf->history, cf->max_iter, cf->max_eval > 0 ? cf->max_eval : cf->max_iter * 5 / 4, cf->max_steps, cf->max_ls,
             cf->lr, cf->tolerance_grad, cf->tolerance_change, cf->ftol, cf->gtol};
    hipError_t e = L->S.ensure(n);
    if (e == hipSuccess) e = L->W.ensure((size_t)n * lbfgs_ws_floats(cf->history));
    if (e == hipSuccess) e = L->RO.ensure((size_t)n * LB_HMAX);
    if (e == hipSuccess) e = L->active.ensure(2);
    if (e == hipSuccess) e = L->active_h.alloc();
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)lbfgs_advance_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lbfgs_lds_bytes(LB_HMAX));
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)lbfgs_advance_tail_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lbfgs_lds_bytes(LB_HMAX));
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*)lbfgs_advance_expr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lbfgs_lds_bytes(LB_HMAX));
    if (e == hipSuccess) { int r = fdcap_lbfgs_reset(L, nullptr); if (r == 0) e = hipDeviceSynchronize(); else e = (hipError_t)r; }
    if (e != hipSuccess) { fdcap_lbfgs_destroy(L); return (int)e; }
    *out = L;
    return FDCAP_OK;
}
void fdcap_lbfgs_destroy(fdcap_lbfgs* L) { delete L; }
int fdcap_lbfgs_reset(fdcap_lbfgs* L, void* stream) {
    if (!L) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(L->S.p, 0, (size_t)L->n * sizeof(LbfgsScalars), st));      // phase 0 = LB_INIT
    HIP_TRY(hipMemsetAsync(L->W.p, 0, (size_t)L->n * lbfgs_ws_floats(L->cf.hist) * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(L->RO.p, 0, (size_t)L->n * LB_HMAX * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(L->active.p, 0, 2 * sizeof(int), st));
    L->round = 0;
    return FDCAP_OK;
}
static int lbfgs_advance_impl(fdcap_lbfgs* L, float* x, int32_t x_stride, const float* f, const float* g, int32_t g_stride, int32_t* n_active,
                              LbfgsFold fold, void* stream, JawGradIn tail = JawGradIn(), ExprTail et = ExprTail());
int fdcap_lbfgs_advance(fdcap_lbfgs* L, float* x, int32_t x_stride, const float* f, const float* g, int32_t g_stride, int32_t* n_active,
                        void* stream) {
    return lbfgs_advance_impl(L, x, x_stride, f, g, g_stride, n_active, LbfgsFold(), stream);
}
static int lbfgs_advance_impl(fdcap_lbfgs* L, float* x, int32_t x_stride, const float* f, const float* g, int32_t g_stride, int32_t* n_active,
                              LbfgsFold fold, void* stream, JawGradIn tail, ExprTail et) {
    if (et.psi) {                                             // the wide tail: psi's ten columns (and the jaw's three) in their own arrays
        const int row = L ? L->cf.dim - et.w : 0;
        if (!L || !x || !f || !g || row < 64 || x_stride < row || g_stride < row) return FDCAP_E_ARG;
        int* const cnt = L->active.p + (L->round & 1);
        hipLaunchKernelGGL(lbfgs_advance_expr_kernel, dim3(L->n), dim3(LB_NT), lbfgs_lds_bytes(L->cf.hist), (hipStream_t)stream, L->cf, L->S.p, L->W.p,
                           L->RO.p, x, x_stride, f, g, g_stride, cnt, L->active.p + ((L->round + 1) & 1), fold, et);
        L->round++;
        if (n_active) HIP_TRY(hipMemcpyAsync(n_active, cnt, sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return (int)hipGetLastError();
    }
    const int in_row = L ? L->cf.dim - (tail.jaw ? 3 : 0) : 0;          // (the tail's three columns live in its own array)
    if (!L || !x || !f || !g || in_row <= 0 || x_stride < in_row || g_stride < in_row || (tail.jaw && in_row < 64)) return FDCAP_E_ARG;   // (the tail form keeps its three columns in a lane's second element)
    hipStream_t st = (hipStream_t)stream;
    int* const cnt = L->active.p + (L->round & 1);            // this round's counter was zeroed by the previous round's launch
    if (tail.jaw)
        hipLaunchKernelGGL(lbfgs_advance_tail_kernel, dim3(L->n), dim3(LB_NT), lbfgs_lds_bytes(L->cf.hist), st, L->cf, L->S.p, L->W.p, L->RO.p, x, x_stride,
                           f, g, g_stride, cnt, L->active.p + ((L->round + 1) & 1), fold, tail);
    else
    hipLaunchKernelGGL(lbfgs_advance_kernel, dim3(L->n), dim3(LB_NT), lbfgs_lds_bytes(L->cf.hist), st, L->cf, L->S.p, L->W.p, L->RO.p, x, x_stride,
                       f, g, g_stride, cnt, L->active.p + ((L->round + 1) & 1), fold);
    L->round++;
    if (n_active) HIP_TRY(hipMemcpyAsync(n_active, cnt, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return (int)hipGetLastError();
}
// in_tail: the last columns of the vector that are NOT in the x row (the tail form; lbfgs_finalize_tail_kernel has put them back)
static int lbfgs_finalize_impl(fdcap_lbfgs* L, float* x, int32_t x_stride, int32_t* n_unfinished, int in_tail, hipStream_t st) {
    if (!L || !x || x_stride < L->cf.dim - in_tail) return FDCAP_E_ARG;
    if (n_unfinished) HIP_TRY(hipMemsetAsync(n_unfinished, 0, sizeof(int32_t), st));
    LbfgsCfg cf = L->cf;
    cf.dim -= in_tail;
    hipLaunchKernelGGL(lbfgs_finalize_kernel, dim3(L->n), dim3(LB_DPAD), 0, st, cf, L->S.p, L->W.p, x, x_stride, n_unfinished);
    return (int)hipGetLastError();
}
int fdcap_lbfgs_finalize(fdcap_lbfgs* L, float* x, int32_t x_stride, int32_t* n_unfinished, void* stream) {
    return lbfgs_finalize_impl(L, x, x_stride, n_unfinished, 0, (hipStream_t)stream);
}
namespace {
__global__ void lbfgs_stats_kernel(const LbfgsScalars* __restrict__ S, int n, int* __restrict__ it, int* __restrict__ ev, float* __restrict__ loss) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (it) it[p] = S[p].n_iter_total;
    if (ev) ev[p] = S[p].evals_total;
    if (loss) loss[p] = S[p].loss;
}
}
int fdcap_lbfgs_get_stats(fdcap_lbfgs* L, int32_t* it, int32_t* ev, float* loss, void* stream) {
    if (!L) return FDCAP_E_ARG;
    hipLaunchKernelGGL(lbfgs_stats_kernel, dim3((L->n + 127) / 128), dim3(128), 0, (hipStream_t)stream, L->S.p, L->n, it, ev, loss);
    return (int)hipGetLastError();
}

// ---- the inner fit's self-interpenetration term (csrc/fdc_collide.h) ---------------------------------------------------------------
int fdcap_opt_set_fit2d_collision(fdcap_ctx* c, const fdcap_collision_params* p) {
    if (!c || !c->opt || opt_is_batch(c) || !opt_whole_clips(c->opt)) return FDCAP_E_STATE;
    OptState* o = c->opt;
    if (!p) { o->coll_on = false; return FDCAP_OK; }
    if (!coll_params_ok(p->sigma, p->w_coll, p->capacity)) return FDCAP_E_ARG;
    // no registered mesh; a free jaw or free expression coefficients without the opt-in (the full-mesh pass then skins with the pose
    // kernels' A: the shut jaw, psi = 0)
    if (c->coll.h.F <= 0 || ((o->jaw_on || o->expr_on) && !o->coll_face)) return FDCAP_E_STATE;
    o->coll = *p;
    o->coll_on = p->w_coll != 0.f;                            // (weight 0: every value and gradient an exact zero -- no launch)
    return FDCAP_OK;
}
// on != 0: the term follows a free jaw and free expression coefficients -- its full-mesh pass corrects the transforms, the PF row and the
// offsets (csrc/fdc_face_mesh.h) and its share of d psi and of the jaw's two gradient parts joins the data term's.  0 (the default): both
// are refused as before, and not one launch or argument of an evaluation differs.
int fdcap_opt_set_fit2d_collision_face(fdcap_ctx* c, int32_t on) {
    if (!c || !c->opt || opt_is_batch(c) || !opt_whole_clips(c->opt)) return FDCAP_E_STATE;
    c->opt->coll_face = on != 0;
    return FDCAP_OK;
}

namespace {
// the second buffers: the first ones' shapes one behind the other, [dA R x 660 | dPF R x 496 | dtransl_v R x 3 | dMv R x 12 | dsv R]
constexpr int COLL2_DPF = NJ * 12, COLL2_DT = COLL2_DPF + NPFX, COLL2_DM = COLL2_DT + 3, COLL2_DS = COLL2_DM + 12, COLL2_LD = COLL2_DS + 1;
struct Coll2 { float *dA, *dPF, *dtv, *dMv, *dsv; };
inline Coll2 coll2_view(float* b, int R) {
    return Coll2{b, b + (size_t)R * COLL2_DPF, b + (size_t)R * COLL2_DT, b + (size_t)R * COLL2_DM, b + (size_t)R * COLL2_DS};
}
// first <- first + second, elementwise, for the five sums of the vertex branch of row row0 + blockIdx.x
__global__ __launch_bounds__(256) void fit2d_coll_add_kernel(Coll2 s, int row0, float* __restrict__ dA, float* __restrict__ dPF,
                                                             float* __restrict__ dtv, float* __restrict__ dMv, float* __restrict__ dsv) {
    const size_t r = (size_t)(row0 + blockIdx.x);
    for (int e = threadIdx.x; e < COLL2_LD; e += 256) {
        float* d; const float* a;
        if (e < COLL2_DPF) { d = dA + r * NJ * 12 + e; a = s.dA + r * NJ * 12 + e; }
        else if (e < COLL2_DT) { d = dPF + r * NPFX + (e - COLL2_DPF); a = s.dPF + r * NPFX + (e - COLL2_DPF); }
        else if (e < COLL2_DM) { d = dtv + r * 3 + (e - COLL2_DT); a = s.dtv + r * 3 + (e - COLL2_DT); }
        else if (e < COLL2_DS) { d = dMv + r * 12 + (e - COLL2_DM); a = s.dMv + r * 12 + (e - COLL2_DM); }
        else { d = dsv + r; a = s.dsv + r; }
        *d = *d + *a;
    }
}
// floss[frame] += the frame's value; losses[FDCAP_LOSS_FIT2D_COLLISION] = the frames' values added in frame order (both optional)
__global__ __launch_bounds__(64) void fit2d_coll_value_kernel(const float* __restrict__ val, int n, float* __restrict__ floss, double* __restrict__ losses) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (floss && f < n) floss[f] += val[f];
    if (losses && f == 0) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += (double)val[i];
        losses[FDCAP_LOSS_FIT2D_COLLISION] = sum;
    }
}
}  // namespace

// The term's pass of one evaluation, after the pose forward and the data term: full-mesh blend and skinning forward over the n_local
// rows, fdcap_collision_eval on the world vertices, skinning and blend backward.  second: the data term has assigned the vertex
// branch's five sums, so these go to buffers of their own and one launch adds them on; else they are the only ones.
// ... with a free jaw and / or free psi (fdcap_opt_set_fit2d_collision_face): face_fwd_kernel corrects the frame's transforms into faceA and
// -- jaw -- copies the PF row with the jaw's block into facePF (o->A and o->PF stay: the keypoint kernels read them), expr_offsets_kernel
// completes the offsets, and the skinning kernels run on those.  Backward: expr_dpsi_kernel, blend_backward, then face_bwd_kernel takes the
// sums for A' to sums for A in place, ADDS the term's share to d psi and to the jaw's skinning part where the data term left its own, and
// J22's share to the betas' entries of dX.  The sums always go to the second buffers and are added on: the first ones hold the data term's,
// or -- `assigned` false: a map without vertices -- are zeroed here where the data term's kernel wrote none.
static int fit2d_collision_pass_face(fdcap_ctx* c, bool assigned, double* losses, float* floss, hipStream_t st) {
    OptState* o = c->opt;
    const int nl = o->cfg.n_local, R = o->R, V = c->V;
    const size_t nv3 = (size_t)3 * V;
    const float* const psi = o->expr_on ? o->psi.p : nullptr;
    const float* const jaw = o->jaw_on ? o->jaw.p : nullptr;
    const int nch = face_nchunk(3 * V);
    if (psi) { int e = ensure_face_tables(c); if (e) return e; }
    HIP_TRY(o->coll2.ensure((size_t)R * COLL2_LD)); HIP_TRY(o->faceA.ensure((size_t)R * NJ * 12));
    if (jaw) HIP_TRY(o->facePF.ensure((size_t)R * NPFX));
    if (psi) HIP_TRY(o->face_part.ensure((size_t)nl * nch * NEXPR));
    const Coll2 first = {o->dA.p, o->dPF.p, o->dtransl_v.p, o->dMv.p, o->dsv.p};
    const Coll2 t = coll2_view(o->coll2.p, R);
    if (!assigned) {                                          // (the expression forms write dA on every path)
        if (!psi) HIP_TRY(hipMemsetAsync(first.dA + (size_t)2 * NJ * 12, 0, (size_t)nl * NJ * 12 * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(first.dPF + (size_t)2 * NPFX, 0, (size_t)nl * NPFX * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(first.dtv + 2 * 3, 0, (size_t)nl * 3 * sizeof(float), st));
        if (!psi) HIP_TRY(hipMemsetAsync(first.dMv + 2 * 12, 0, (size_t)nl * 12 * sizeof(float), st));    // (... and dMv)
        HIP_TRY(hipMemsetAsync(first.dsv + 2, 0, (size_t)nl * sizeof(float), st));
    }
    float* const PF2 = jaw ? o->facePF.p : nullptr;
    hipLaunchKernelGGL(face_fwd_kernel, dim3(nl), dim3(FACE_NT), 0, st, c->face_tabs(), (const float*)o->A.p, (const float*)o->PF.p, (const float*)nullptr,
                       (const float*)o->X.p, XDIM, X_BETAS, X_TRANSL, 2, psi, jaw, o->faceA.p, PF2, (float*)nullptr);
    HIP_TRY(blend_forward(c->full, (PF2 ? PF2 : o->PF.p) + 2 * NPFX, nl, o->VoffF.p + 2 * nv3, st));
    if (psi)
        hipLaunchKernelGGL(expr_offsets_kernel, dim3((3 * V + 255) / 256, (nl + FACE_FS - 1) / FACE_FS), dim3(256), 0, st, c->d_Ef.p, c->lde_f, 3 * V, psi,
                           nl, o->VoffF.p + 2 * nv3, nv3);
    note_form(form_name(F_SKIN_FWD));
    hipLaunchKernelGGL(skin_fwd_kernel, dim3((V + 255) / 256, nl), dim3(256), 0, st, c->full.model(), V, o->X.p, XDIM, X_BETAS, X_TRANSL, o->VoffF.p,
                       o->faceA.p, o->M.p, o->scale.p, 2, 1, o->VwF.p);
    { int e = fdcap_collision_eval(c, o->VwF.p + 2 * nv3, nl, &o->coll, nullptr, o->coll_count.p, o->coll_loss.p, o->dVF.p + 2 * nv3, st); if (e) return e; }
    { int es = skin_bwd_any<false>(c->ws_skin, st, nl, c->full.model(), V, o->X.p, o->VoffF.p, o->faceA.p, o->M.p, o->scale.p, 2, o->dVF.p, o->dVF.p, t.dA,
                                   (float*)nullptr, t.dtv, t.dMv, t.dsv, ContactGradIn()); if (es) return es; }
    if (psi)
        hipLaunchKernelGGL(expr_dpsi_kernel, dim3(nch, (nl + FACE_FS - 1) / FACE_FS), dim3(256), 0, st, c->d_Ef.p, c->lde_f, 3 * V,
                           (const float*)(o->dVF.p + 2 * nv3), nv3, nl, o->face_part.p, nch);
    HIP_TRY(blend_backward(c->full, o->dVF.p + 2 * nv3, nl, t.dPF + 2 * NPFX, 0, c->ws_kpart, st));
    hipLaunchKernelGGL(face_bwd_kernel, dim3(nl), dim3(FACE_NT), 0, st, c->face_tabs(), (const float*)o->A.p, (const float*)t.dA, (const float*)o->X.p, XDIM,
                       X_BETAS, 2, psi, jaw, (const float*)nullptr, psi ? (const float*)o->face_part.p : nullptr, nch, t.dA, psi ? o->dpsi.p : nullptr,
                       jaw ? o->jawR9.p : nullptr, o->dX.p, 1);
    hipLaunchKernelGGL(fit2d_coll_add_kernel, dim3(nl), dim3(256), 0, st, t, 2, first.dA, first.dPF, first.dtv, first.dMv, first.dsv);
    if (jaw) o->jaw_gp = true;                                // (dPF's jaw block is there now, whatever the map holds)
    if (floss || losses)
        hipLaunchKernelGGL(fit2d_coll_value_kernel, dim3((nl + 63) / 64), dim3(64), 0, st, (const float*)o->coll_loss.p, nl, floss, losses);
    return (int)hipGetLastError();
}

static int fit2d_collision_pass(fdcap_ctx* c, bool second, double* losses, float* floss, hipStream_t st) {
    OptState* o = c->opt;
    const int nl = o->cfg.n_local, R = o->R, V = c->V;
    const size_t nv3 = (size_t)3 * V;
    { int e = ensure_full_set(c); if (e) return e; }
    HIP_TRY(o->VoffF.ensure((size_t)R * nv3)); HIP_TRY(o->VwF.ensure((size_t)R * nv3)); HIP_TRY(o->dVF.ensure((size_t)R * nv3));
    HIP_TRY(o->coll_loss.ensure(nl)); HIP_TRY(o->coll_count.ensure(nl));
    if (o->coll_face && (o->jaw_on || o->expr_on)) return fit2d_collision_pass_face(c, second, losses, floss, st);
    if (second) HIP_TRY(o->coll2.ensure((size_t)R * COLL2_LD));
    HIP_TRY(blend_forward(c->full, o->PF.p + 2 * NPFX, nl, o->VoffF.p + 2 * nv3, st));
    note_form(form_name(F_SKIN_FWD));
    hipLaunchKernelGGL(skin_fwd_kernel, dim3((V + 255) / 256, nl), dim3(256), 0, st, c->full.model(), V, o->X.p, XDIM, X_BETAS, X_TRANSL, o->VoffF.p,
                       o->A.p, o->M.p, o->scale.p, 2, 1, o->VwF.p);
    { int e = fdcap_collision_eval(c, o->VwF.p + 2 * nv3, nl, &o->coll, nullptr, o->coll_count.p, o->coll_loss.p, o->dVF.p + 2 * nv3, st); if (e) return e; }
    const Coll2 first = {o->dA.p, o->dPF.p, o->dtransl_v.p, o->dMv.p, o->dsv.p};
    const Coll2 t = second ? coll2_view(o->coll2.p, R) : first;
    { int es = skin_bwd_any<false>(c->ws_skin, st, nl, c->full.model(), V, o->X.p, o->VoffF.p, o->A.p, o->M.p, o->scale.p, 2, o->dVF.p, o->dVF.p, t.dA,
                                   (float*)nullptr, t.dtv, t.dMv, t.dsv, ContactGradIn()); if (es) return es; }
    HIP_TRY(blend_backward(c->full, o->dVF.p + 2 * nv3, nl, t.dPF + 2 * NPFX, 0, c->ws_kpart, st));
    if (second) hipLaunchKernelGGL(fit2d_coll_add_kernel, dim3(nl), dim3(256), 0, st, t, 2, first.dA, first.dPF, first.dtv, first.dMv, first.dsv);
    if (floss || losses)
        hipLaunchKernelGGL(fit2d_coll_value_kernel, dim3((nl + 63) / 64), dim3(64), 0, st, (const float*)o->coll_loss.p, nl, floss, losses);
    return (int)hipGetLastError();
}

// one evaluation of the inner fit's objective: forward, loss (+ per-frame value), backward
static int fit2d_eval(fdcap_ctx* c, const fdcap_fit2d_stage* sg, double* losses, float* floss, hipStream_t st, bool fold) {
    OptState* o = c->opt;
    const int nl = o->cfg.n_local;
    Fit2dStage s = {sg->fx, sg->fy, sg->cx, sg->cy, sg->rho, sg->w_data, sg->w_pose, sg->w_shape, sg->w_hand};
    PoseModel pm = c->pose_model();
    if (o->jaw_on && !o->kp_mapped) return FDCAP_E_STATE;     // (no keypoint of the 23-joint layout follows the jaw)
    const bool coll = o->coll_on;                             // (fdcap_opt_set_fit2d_collision; off: not one launch or argument differs)
    if (coll && ((o->jaw_on && !o->coll_face) || c->coll.h.F <= 0)) return FDCAP_E_STATE;
    const bool expr = o->expr_on;                             // (fdcap_opt_set_expression; off: not one launch or argument differs)
    if (expr && (!o->kp_mapped || (coll && !o->coll_face) || c->kpset.E.p == nullptr)) return FDCAP_E_STATE;      // (the 23-joint layout; without the opt-in the full-mesh pass skins at psi = 0)
    const JawIO jw = {o->jaw.p, o->jawR9.p, {o->w_jaw[0], o->w_jaw[1], o->w_jaw[2]}};
    const bool bend = o->bend.n > 0;                          // (fdcap_opt_set_fit2d_extra; off: not one launch or argument differs)
    int row_lo, row_hi;
    opt_row_range(o, 1, &row_lo, &row_hi);
    int e = opt_pose_forward(c, row_lo, row_hi, st);
    if (e) return e;
    if (o->kp_mapped) {
        // the mapped data term: one launch in the loss kernel's place; a map with surface points or finger joints hands the pose
        // backward its vertex branch's sums as mode 'local''s full-mesh pass does (dA, dPF with betas, dtransl_v, dMv, dsv)
        // (kp_panel: the set's two blend products as panel products around it, kp_blend_by_panels)
        const bool vb = c->kpset.h.nu() > 0;
        if (o->jaw_on) { o->jaw_eval = true; o->jaw_gp = vb; }
        if (expr) {
            // the same three places with the expression forms: the kernel corrects A and Jw for psi itself, writes dA on every path
            // (a map of joints 0..22 alone: only the rotation addends) and leaves d psi complete
            const ExprIO ex = c->expr_view(o->psi.p, o->dpsi.p, o->w_expr);
            o->expr_eval = true;
            if (o->kp_panel) HIP_TRY(blend_forward(c->kpset.ss, o->PF.p + 2 * NPFX, nl, o->kpV.p, st));
            const float* const vin = o->kp_panel ? o->kpV.p : nullptr;
            float* const vout = o->kp_panel ? o->kpdV.p : nullptr;
#define FDC_EXPR_LAUNCH(KERNEL, ...)                                                                                                             \
            hipLaunchKernelGGL(KERNEL, dim3(nl), dim3(KP_NT), 0, st, s, c->kp_view(), o->X.p, o->PF.p, o->A.p, o->M.p, o->scale.p, o->Jw.p, o->kp2d.p, 2, \
                               o->dX.p, o->dJw.p, o->dA.p, o->dPF.p, o->dtransl_v.p, o->dMv.p, o->dsv.p, losses, floss, (float*)nullptr, vin, vout, __VA_ARGS__)
            if (o->kp_panel && o->jaw_on) FDC_EXPR_LAUNCH((fit2d_kp_expr_jaw_kernel<false, true>), jw, ex);
            else if (o->kp_panel) FDC_EXPR_LAUNCH((fit2d_kp_expr_kernel<false, true>), ex);
            else if (o->jaw_on) FDC_EXPR_LAUNCH((fit2d_kp_expr_jaw_kernel<false, false>), jw, ex);
            else FDC_EXPR_LAUNCH((fit2d_kp_expr_kernel<false, false>), ex);
#undef FDC_EXPR_LAUNCH
            if (o->kp_panel) HIP_TRY(blend_backward(c->kpset.ss, o->kpdV.p, nl, o->dPF.p + 2 * NPFX, 0, c->ws_kpart, st));
            // the self-interpenetration term on the fitted face (fdcap_opt_set_fit2d_collision_face; off: vs = vb, nothing differs)
            if (coll) { int ec = fit2d_collision_pass(c, vb, losses, floss, st); if (ec) return ec; }
            const bool vs = vb || coll;
            if (bend && vs) hipLaunchKernelGGL(fit2d_bend_kernel<true>, dim3(nl), dim3(64), 0, st, o->bend, o->PF.p, 2, o->dPF.p, losses, floss);
            else if (bend) hipLaunchKernelGGL(fit2d_bend_kernel<false>, dim3(nl), dim3(64), 0, st, o->bend, o->PF.p, 2, o->dPF.p, losses, floss);
            hipLaunchKernelGGL(pose_bwd_kernel, dim3(nl), dim3(64 * POSE_NW), 0, st, pm, o->X.p, o->O.p, o->CAM.p, o->scale.p, 2, o->Rm.p,
                               o->Jrest.p, o->G.p, (const float*)o->dA.p, (vs || bend) ? o->dPF.p : (const float*)nullptr, o->dJw.p,
                               (const float*)o->dMv.p /* (written on every path, as dA: the correction's share of d M) */, vs ? o->dsv.p : (const float*)nullptr,
                               vs ? o->dPF.p + NPF : (const float*)nullptr, vs ? NPFX : 0, vs ? o->dtransl_v.p : (const float*)nullptr, o->dX.p, o->dO.p,
                               o->dCAM.p, o->dscale_row.p, ParamLossIn(), (const float*)nullptr);
            { int eb = opt_vposer_backward(c, fold, st); if (eb) return eb; }
            return (int)hipGetLastError();
        }
        if (o->kp_panel) {
            HIP_TRY(blend_forward(c->kpset.ss, o->PF.p + 2 * NPFX, nl, o->kpV.p, st));
            if (o->jaw_on)
                hipLaunchKernelGGL((fit2d_kp_jaw_kernel<false, true>), dim3(nl), dim3(KP_NT), 0, st, s, c->kp_view(), o->X.p, o->PF.p, o->A.p, o->M.p,
                                   o->scale.p, o->Jw.p, o->kp2d.p, 2, o->dX.p, o->dJw.p, o->dA.p, o->dPF.p, o->dtransl_v.p, o->dMv.p, o->dsv.p, losses,
                                   floss, (float*)nullptr, o->kpV.p, o->kpdV.p, jw);
            else
            hipLaunchKernelGGL((fit2d_kp_kernel<false, true>), dim3(nl), dim3(KP_NT), 0, st, s, c->kp_view(), o->X.p, o->PF.p, o->A.p, o->M.p, o->scale.p,
                               o->Jw.p, o->kp2d.p, 2, o->dX.p, o->dJw.p, o->dA.p, o->dPF.p, o->dtransl_v.p, o->dMv.p, o->dsv.p, losses, floss,
                               (float*)nullptr, o->kpV.p, o->kpdV.p);
            HIP_TRY(blend_backward(c->kpset.ss, o->kpdV.p, nl, o->dPF.p + 2 * NPFX, 0, c->ws_kpart, st));
        } else if (o->jaw_on)
            hipLaunchKernelGGL((fit2d_kp_jaw_kernel<false, false>), dim3(nl), dim3(KP_NT), 0, st, s, c->kp_view(), o->X.p, o->PF.p, o->A.p, o->M.p,
                               o->scale.p, o->Jw.p, o->kp2d.p, 2, o->dX.p, o->dJw.p, o->dA.p, o->dPF.p, o->dtransl_v.p, o->dMv.p, o->dsv.p, losses,
                               floss, (float*)nullptr, (const float*)nullptr, (float*)nullptr, jw);
        else
            hipLaunchKernelGGL((fit2d_kp_kernel<false, false>), dim3(nl), dim3(KP_NT), 0, st, s, c->kp_view(), o->X.p, o->PF.p, o->A.p, o->M.p, o->scale.p,
                               o->Jw.p, o->kp2d.p, 2, o->dX.p, o->dJw.p, o->dA.p, o->dPF.p, o->dtransl_v.p, o->dMv.p, o->dsv.p, losses, floss,
                               (float*)nullptr, (const float*)nullptr, (float*)nullptr);
        // the bending prior: its launch adds to the dPF the vertex branch left (the kernel's or blend_backward's), or -- a map of
        // joints 0..22 alone -- assigns the row, which pose_bwd_kernel then reads without the branch's other sums
        // the self-interpenetration term: its full-mesh pass adds to the vertex branch's sums, or -- no vertex branch -- leaves the only ones
        if (coll) { int ec = fit2d_collision_pass(c, vb, losses, floss, st); if (ec) return ec; }
        const bool vs = vb || coll;                               // the vertex branch's sums are there
        if (bend && vs) hipLaunchKernelGGL(fit2d_bend_kernel<true>, dim3(nl), dim3(64), 0, st, o->bend, o->PF.p, 2, o->dPF.p, losses, floss);
        else if (bend) hipLaunchKernelGGL(fit2d_bend_kernel<false>, dim3(nl), dim3(64), 0, st, o->bend, o->PF.p, 2, o->dPF.p, losses, floss);
        hipLaunchKernelGGL(pose_bwd_kernel, dim3(nl), dim3(64 * POSE_NW), 0, st, pm, o->X.p, o->O.p, o->CAM.p, o->scale.p, 2, o->Rm.p,
                           o->Jrest.p, o->G.p, vs ? o->dA.p : (const float*)nullptr, (vs || bend) ? o->dPF.p : (const float*)nullptr, o->dJw.p,
                           vs ? o->dMv.p : (const float*)nullptr, vs ? o->dsv.p : (const float*)nullptr,
                           vs ? o->dPF.p + NPF : (const float*)nullptr, vs ? NPFX : 0, vs ? o->dtransl_v.p : (const float*)nullptr, o->dX.p, o->dO.p,
                           o->dCAM.p, o->dscale_row.p, ParamLossIn(), (const float*)nullptr);
        { int eb = opt_vposer_backward(c, fold, st); if (eb) return eb; }
        return (int)hipGetLastError();
    }
    hipLaunchKernelGGL(fit2d_loss_kernel, dim3(nl), dim3(128), 0, st, s, o->X.p, o->Jw.p, o->kp2d.p, 2, o->dX.p, o->dJw.p, losses, floss);
    if (coll) {                                                 // the full-mesh pass's sums are the only vertex-branch sums: straight to the pose backward
        { int ec = fit2d_collision_pass(c, false, losses, floss, st); if (ec) return ec; }
        if (bend) hipLaunchKernelGGL(fit2d_bend_kernel<true>, dim3(nl), dim3(64), 0, st, o->bend, o->PF.p, 2, o->dPF.p, losses, floss);
        hipLaunchKernelGGL(pose_bwd_kernel, dim3(nl), dim3(64 * POSE_NW), 0, st, pm, o->X.p, o->O.p, o->CAM.p, o->scale.p, 2, o->Rm.p,
                           o->Jrest.p, o->G.p, (const float*)o->dA.p, (const float*)o->dPF.p, o->dJw.p, (const float*)o->dMv.p, (const float*)o->dsv.p,
                           (const float*)(o->dPF.p + NPF), NPFX, (const float*)o->dtransl_v.p, o->dX.p, o->dO.p, o->dCAM.p, o->dscale_row.p, ParamLossIn(),
                           (const float*)nullptr);
        { int eb = opt_vposer_backward(c, fold, st); if (eb) return eb; }
        return (int)hipGetLastError();
    }
    if (bend) hipLaunchKernelGGL(fit2d_bend_kernel<false>, dim3(nl), dim3(64), 0, st, o->bend, o->PF.p, 2, o->dPF.p, losses, floss);
    hipLaunchKernelGGL(pose_bwd_kernel, dim3(nl), dim3(64 * POSE_NW), 0, st, pm, o->X.p, o->O.p, o->CAM.p, o->scale.p, 2, o->Rm.p,
                       o->Jrest.p, o->G.p, (const float*)nullptr, bend ? o->dPF.p : (const float*)nullptr, o->dJw.p, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, 0, (const float*)nullptr, o->dX.p, o->dO.p, o->dCAM.p,
                       o->dscale_row.p, ParamLossIn(), (const float*)nullptr);
    { int eb = opt_vposer_backward(c, fold, st); if (eb) return eb; }
    return (int)hipGetLastError();
}

int fdcap_opt_fit2d_lbfgs(fdcap_ctx* c, const fdcap_fit2d_stage* sg, const fdcap_lbfgs_config* cfg, int32_t max_rounds, int32_t* rounds_out,
                          void* stream) {
    if (opt_is_batch(c)) return FDCAP_E_STATE;           // (a batch of clips: mode 'global' only)
    if (!c || !c->opt || !sg || !cfg || max_rounds <= 0) return FDCAP_E_ARG;
    { int es_ = opt_sync(c, (hipStream_t)stream); if (es_) return es_; }
    OptState* o = c->opt;
    if (!o->kp2d.p) return FDCAP_E_STATE;
    hipStream_t st = (hipStream_t)stream;
    const int nl = o->cfg.n_local;
    fdcap_lbfgs_config cf = *cfg;
    cf.dim = o->jaw_on ? XDIM + 3 : XDIM;                     // a free jaw: [the row | the jaw], the last three in the jaw's own array
    if (o->expr_on) cf.dim += NEXPR;                          // free expression: [the row | psi | the jaw], psi in its own array too
    if (!lbfgs_cfg_ok(&cf)) return FDCAP_E_ARG;
    if (o->lbfgs && (o->lbfgs->n != nl || o->lbfgs->cf.hist != cf.history)) { fdcap_lbfgs_destroy(o->lbfgs); o->lbfgs = nullptr; }
    if (!o->lbfgs) { int e = fdcap_lbfgs_create(nl, &cf, &o->lbfgs); if (e) return e; }
    fdcap_lbfgs* L = o->lbfgs;
    L->cf = {cf.dim, cf.history, cf.max_iter, cf.max_eval > 0 ? cf.max_eval : cf.max_iter * 5 / 4, cf.max_steps, cf.max_ls,
             cf.lr, cf.tolerance_grad, cf.tolerance_change, cf.ftol, cf.gtol};
    { int e = fdcap_lbfgs_reset(L, st); if (e) return e; }
    HIP_TRY(o->floss.ensure(nl));
    o->ahead = false; o->log_pending = false; o->log_dst = nullptr;
    int rounds = 0, e = 0;
    const int poll = 8;                                       // rounds between two looks at the number of frames still running
    while (rounds < max_rounds) {
        e = fit2d_eval(c, sg, nullptr, o->floss.p, st, false);   // (the latent gradient's four partials are folded by the advance kernel)
        if (e) break;
        LbfgsFold fold;
        fold.part = o->dZpart.p + (size_t)2 * VP_Z; fold.stride = (size_t)o->R * VP_Z; fold.col0 = X_LATENT; fold.n = VP_Z;
        e = lbfgs_advance_impl(L, o->X.p + 2 * XDIM, XDIM, o->floss.p, o->dX.p + 2 * XDIM, XDIM, nullptr, fold, st,
                               o->jaw_on && !o->expr_on ? opt_jaw_grad_in(c) : JawGradIn(),
                               o->expr_on ? ExprTail{o->psi.p, o->dpsi.p, o->jaw_on ? opt_jaw_grad_in(c) : JawGradIn(), o->jaw_on ? NEXPR + 3 : NEXPR}
                                          : ExprTail());
        if (e) break;
        ++rounds;
        if (rounds % poll == 0 || rounds == max_rounds) {
            HIP_TRY(hipMemcpyAsync(L->active_h.p, L->active.p + ((L->round - 1) & 1), sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (*L->active_h.p == 0) break;
        }
    }
    if (rounds_out) *rounds_out = rounds;
    // out of rounds with frames still inside a line search: their rows hold trial points -- roll them back to the accepted ones
    o->lbfgs_rolled_back = 0;
    if (!e && rounds >= max_rounds && *L->active_h.p != 0) {
        o->lbfgs_rolled_back = *L->active_h.p;               // (a problem that is not finished waits inside a line search, a trial point in its row)
        if (o->jaw_on) hipLaunchKernelGGL(lbfgs_finalize_tail_kernel, dim3((nl + 63) / 64), dim3(64), 0, st, L->cf, L->S.p, L->W.p, o->jaw.p, nl);
        if (o->expr_on) hipLaunchKernelGGL(lbfgs_finalize_expr_kernel, dim3((nl + 63) / 64), dim3(64), 0, st, L->cf, L->S.p, L->W.p, o->psi.p, XDIM, nl);
        e = lbfgs_finalize_impl(L, o->X.p + 2 * XDIM, XDIM, nullptr, (o->jaw_on ? 3 : 0) + (o->expr_on ? NEXPR : 0), st);
    }
    if (o->dz_pending) {                                      // leave dX complete, as every other backward of the API does
        hipLaunchKernelGGL(vposer_fold_dz_kernel, dim3((nl * VP_Z + 255) / 256), dim3(256), 0, st, o->dZpart.p, (size_t)o->R * VP_Z, 2, nl, o->dX.p);
        o->dz_pending = false;
    }
    if (e) return e;
    HIP_TRY(hipStreamSynchronize(st));
    return FDCAP_OK;
}

int fdcap_opt_fit2d_lbfgs_rolled_back(fdcap_ctx* c, int32_t* n_frames) {
    if (opt_is_batch(c)) return FDCAP_E_STATE;
    if (!c || !c->opt || !c->opt->lbfgs) return FDCAP_E_STATE;
    if (!n_frames) return FDCAP_E_ARG;
    *n_frames = c->opt->lbfgs_rolled_back;
    return FDCAP_OK;
}

int fdcap_opt_fit2d_lbfgs_stats(fdcap_ctx* c, int32_t* it, int32_t* ev, float* loss, void* stream) {
    if (opt_is_batch(c)) return FDCAP_E_STATE;           // (a batch of clips: mode 'global' only)
    if (!c || !c->opt || !c->opt->lbfgs) return FDCAP_E_STATE;
    return fdcap_lbfgs_get_stats(c->opt->lbfgs, it, ev, loss, stream);
}

// ---- the inner fit's start from keypoints alone (csrc/fdc_fit2d_init.h) ----------------------------------------------------------
static_assert(sizeof(((fdcap_fit2d_init*)nullptr)->edge) == sizeof(int32_t) * INIT_MAX_EDGE * 2 && sizeof(((fdcap_fit2d_init*)nullptr)->torso) == sizeof(int32_t) * INIT_MAX_TORSO,
              "fdc_fit2d_init.h restates the longest lists of fdcap_fit2d_init");
// the state the three calls need, then the caller's settings with their slots resolved against the current keypoint layout
static int fit2d_init_resolve(fdcap_ctx* c, const fdcap_fit2d_stage* sg, const fdcap_fit2d_init* in, Fit2dInit* out, int* n_kp) {
    if (!c || !c->opt || opt_is_batch(c) || !opt_whole_clips(c->opt) || !c->opt->kp2d.p) return FDCAP_E_STATE;
    if (!sg || !in) return FDCAP_E_ARG;
    std::vector<int32_t> slot_joint;
    if (c->opt->kp_mapped) {                                  // (a joint 23..54 is a pseudo-vertex of the set: KeypointTables)
        const KeypointTables& t = c->kpset.h;
        for (int k = 0; k < t.n_kp; ++k)
            slot_joint.push_back(t.kjoint[k] >= 0 ? t.kjoint[k] : t.kref[3 * k] >= t.nr ? t.pseudo_joint[t.kref[3 * k] - t.nr] : -1);
    } else
        for (int k = 0; k < NJW; ++k) slot_joint.push_back(k);
    *n_kp = (int)slot_joint.size();
    if (fit2d_init_build(in->n_edge, in->edge, in->n_torso, in->torso, in->shoulder, in->conf_thr, in->default_depth, in->side_view_px, in->w_data,
                         in->w_depth, *n_kp, slot_joint.data(), out))
        return FDCAP_E_ARG;
    return FDCAP_OK;
}
static int fit2d_full_forward(fdcap_ctx* c, hipStream_t st) {
    int row_lo, row_hi;
    opt_row_range(c->opt, 1, &row_lo, &row_hi);
    return opt_pose_forward(c, row_lo, row_hi, st);
}

int fdcap_opt_fit2d_guess(fdcap_ctx* c, const fdcap_fit2d_stage* sg, const fdcap_fit2d_init* init, float* z_d, int32_t* valid_d, int32_t* side_view_d,
                          void* stream) {
    Fit2dInit ci;
    int n_kp = 0;
    { int e = fit2d_init_resolve(c, sg, init, &ci, &n_kp); if (e) return e; }
    hipStream_t st = (hipStream_t)stream;
    { int es_ = opt_sync(c, st); if (es_) return es_; }
    OptState* o = c->opt;
    const int nl = o->cfg.n_local;
    { int e = fit2d_full_forward(c, st); if (e) return e; }
    hipLaunchKernelGGL(fit2d_guess_kernel, dim3((nl + 63) / 64), dim3(64), 0, st, ci, sg->fx, sg->fy, o->G.p, o->kp2d.p, n_kp, 2, nl, o->X.p, z_d,
                       (int*)valid_d, (int*)side_view_d);
    return (int)hipGetLastError();
}

// one evaluation of the camera stage (set-up first where it is due): the whole of dX's owned rows, optionally the per-frame value
static int fit2d_camera_eval(fdcap_ctx* c, const fdcap_fit2d_stage* sg, const Fit2dInit& ci, int n_kp, bool setup, double* losses, float* floss,
                             hipStream_t st) {
    OptState* o = c->opt;
    const int nl = o->cfg.n_local;
    if (setup || !o->cam_ready || !fit2d_init_same_torso(o->cam_init, ci)) {
        HIP_TRY(o->cam_setup.ensure((size_t)nl * CAM_SETUP_LD));
        { int e = fit2d_full_forward(c, st); if (e) return e; }
        hipLaunchKernelGGL(fit2d_camera_setup_kernel, dim3(nl), dim3(64), 0, st, ci, o->X.p, o->G.p, 2, o->cam_setup.p);
        o->cam_ready = true;
        o->cam_init = ci;
    }
    const Fit2dStage s = {sg->fx, sg->fy, sg->cx, sg->cy, sg->rho, sg->w_data, sg->w_pose, sg->w_shape, sg->w_hand};
    hipLaunchKernelGGL(fit2d_camera_kernel, dim3(nl), dim3(64), 0, st, s, ci, o->X.p, o->cam_setup.p, o->kp2d.p, n_kp, 2, o->dX.p, losses, floss);
    o->dz_pending = false;                                    // (the latent's columns are zeros of this launch: no partial belongs to them)
    o->jaw_eval = false;                                      // (... and no gradient part to a free jaw: a step leaves it where it is)
    o->expr_eval = false;                                     // (... nor to free expression coefficients)
    return (int)hipGetLastError();
}

int fdcap_opt_backward_fit2d_camera(fdcap_ctx* c, const fdcap_fit2d_stage* sg, const fdcap_fit2d_init* init, int32_t log_terms, void* stream) {
    Fit2dInit ci;
    int n_kp = 0;
    { int e = fit2d_init_resolve(c, sg, init, &ci, &n_kp); if (e) return e; }
    hipStream_t st = (hipStream_t)stream;
    { int es_ = opt_sync(c, st); if (es_) return es_; }
    double* const losses = (log_terms & 1) ? c->opt->losses.p : nullptr;
    if (losses) HIP_TRY(hipMemsetAsync(losses, 0, FDCAP_NUM_LOSSES * sizeof(double), st));
    return fit2d_camera_eval(c, sg, ci, n_kp, (log_terms & 2) != 0, losses, nullptr, st);
}

int fdcap_opt_fit2d_camera_lbfgs(fdcap_ctx* c, const fdcap_fit2d_stage* sg, const fdcap_fit2d_init* init, const fdcap_lbfgs_config* cfg,
                                 int32_t max_rounds, int32_t* rounds_out, void* stream) {
    Fit2dInit ci;
    int n_kp = 0;
    { int e = fit2d_init_resolve(c, sg, init, &ci, &n_kp); if (e) return e; }
    if (!cfg || max_rounds <= 0) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    { int es_ = opt_sync(c, st); if (es_) return es_; }
    OptState* o = c->opt;
    const int nl = o->cfg.n_local;
    fdcap_lbfgs_config cf = *cfg;
    cf.dim = XDIM;                                            // the whole row: 69 of its columns never get a gradient, so never a direction
    if (!lbfgs_cfg_ok(&cf)) return FDCAP_E_ARG;
    if (o->lbfgs && (o->lbfgs->n != nl || o->lbfgs->cf.hist != cf.history)) { fdcap_lbfgs_destroy(o->lbfgs); o->lbfgs = nullptr; }
    if (!o->lbfgs) { int e = fdcap_lbfgs_create(nl, &cf, &o->lbfgs); if (e) return e; }
    fdcap_lbfgs* L = o->lbfgs;
    L->cf = {cf.dim, cf.history, cf.max_iter, cf.max_eval > 0 ? cf.max_eval : cf.max_iter * 5 / 4, cf.max_steps, cf.max_ls,
             cf.lr, cf.tolerance_grad, cf.tolerance_change, cf.ftol, cf.gtol};
    { int e = fdcap_lbfgs_reset(L, st); if (e) return e; }
    HIP_TRY(o->floss.ensure(nl));
    o->ahead = false; o->log_pending = false; o->log_dst = nullptr;
    int rounds = 0, e = 0;
    const int poll = 8;                                       // (fdcap_opt_fit2d_lbfgs's)
    while (rounds < max_rounds) {
        e = fit2d_camera_eval(c, sg, ci, n_kp, false, nullptr, o->floss.p, st);
        if (e) break;
        e = lbfgs_advance_impl(L, o->X.p + 2 * XDIM, XDIM, o->floss.p, o->dX.p + 2 * XDIM, XDIM, nullptr, LbfgsFold(), st);
        if (e) break;
        ++rounds;
        if (rounds % poll == 0 || rounds == max_rounds) {
            HIP_TRY(hipMemcpyAsync(L->active_h.p, L->active.p + ((L->round - 1) & 1), sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (*L->active_h.p == 0) break;
        }
    }
    if (rounds_out) *rounds_out = rounds;
    o->lbfgs_rolled_back = 0;
    if (!e && rounds >= max_rounds && *L->active_h.p != 0) {   // out of rounds inside a line search: back to the accepted points
        o->lbfgs_rolled_back = *L->active_h.p;
        e = lbfgs_finalize_impl(L, o->X.p + 2 * XDIM, XDIM, nullptr, 0, st);
    }
    if (e) return e;
    HIP_TRY(hipStreamSynchronize(st));
    return FDCAP_OK;
}

int fdcap_opt_fit2d_frame_loss(fdcap_ctx* c, const fdcap_fit2d_stage* sg, float* floss_d, void* stream) {
    if (!c || !c->opt || opt_is_batch(c) || !opt_whole_clips(c->opt) || !c->opt->kp2d.p) return FDCAP_E_STATE;
    if (!sg || !floss_d) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    { int es_ = opt_sync(c, st); if (es_) return es_; }
    OptState* o = c->opt;
    HIP_TRY(o->floss.ensure(o->cfg.n_local));
    { int e = fit2d_eval(c, sg, nullptr, o->floss.p, st, true); if (e) return e; }
    HIP_TRY(hipMemcpyAsync(floss_d, o->floss.p, (size_t)o->cfg.n_local * sizeof(float), hipMemcpyDeviceToDevice, st));
    return FDCAP_OK;
}

int fdcap_fit2d_flip_orient(float* rows75_d, int32_t n, void* stream) {
    if (!rows75_d || n <= 0) return FDCAP_E_ARG;
    hipLaunchKernelGGL(fit2d_flip_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, rows75_d, n);
    return (int)hipGetLastError();
}

int fdcap_fit2d_select(const float* rows_d, const float* loss_d, const int32_t* src_d, int32_t n, int32_t m, const float* jaw_d, float* rows_out_d,
                       float* jaw_out_d, int32_t* chosen_d, void* stream) {
    if (!rows_d || !loss_d || !rows_out_d || n <= 0 || m < 0 || m > n || (m > 0 && !src_d) || (jaw_d == nullptr) != (jaw_out_d == nullptr))
        return FDCAP_E_ARG;
    hipLaunchKernelGGL(fit2d_select_kernel, dim3(n), dim3(128), 0, (hipStream_t)stream, rows_d, loss_d, (const int*)src_d, n, m, jaw_d, rows_out_d,
                       jaw_out_d, (int*)chosen_d);
    return (int)hipGetLastError();
}

// zero Adam's moments of body_rotation_rec (SMPLify-X builds a fresh optimiser for every stage of the fit)
int fdcap_opt_reset_adam(fdcap_ctx* c, void* stream) {
    if (!c || !c->opt) return FDCAP_E_STATE;
    { int es_ = opt_sync(c, (hipStream_t)stream); if (es_) return es_; }
    OptState* o = c->opt;
    const size_t n = (size_t)o->R * XDIM * sizeof(float);
    o->log_pending = false; o->log_dst = nullptr;
    HIP_TRY(hipMemsetAsync(o->mX.p, 0, n, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(o->vX.p, 0, n, (hipStream_t)stream));
    if (o->jaw_on) {
        HIP_TRY(hipMemsetAsync(o->mJaw.p, 0, (size_t)3 * o->cfg.n_local * sizeof(float), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(o->vJaw.p, 0, (size_t)3 * o->cfg.n_local * sizeof(float), (hipStream_t)stream));
    }
    if (o->expr_on) {
        HIP_TRY(hipMemsetAsync(o->mPsi.p, 0, (size_t)NEXPR * o->cfg.n_local * sizeof(float), (hipStream_t)stream));
        HIP_TRY(hipMemsetAsync(o->vPsi.p, 0, (size_t)NEXPR * o->cfg.n_local * sizeof(float), (hipStream_t)stream));
    }
    return FDCAP_OK;
}

// ---- checkpoint / resume of the optimiser state, finite check (the reference has neither) -----------
int32_t fdcap_opt_state_len(fdcap_ctx* c) {
    if (!c || !c->opt) return 0;
    return (int32_t)(2 * ((size_t)c->opt->cfg.n_local * (XDIM + 16)) + 2 * (size_t)c->opt->nclip);
}
static int opt_state_copy(fdcap_ctx* c, float* state, bool to_state, hipStream_t st) {
    OptState* o = c->opt;
    const size_t nl = o->cfg.n_local, nx = nl * XDIM, ncam = nl * 16;
    struct Part { float* lib; size_t n; } parts[] = {{o->mX.p + 2 * XDIM, nx}, {o->vX.p + 2 * XDIM, nx}, {o->mCAM.p + 2 * 16, ncam},
                                                     {o->vCAM.p + 2 * 16, ncam}, {o->mS.p, (size_t)o->nclip}, {o->vS.p, (size_t)o->nclip}};
    size_t off = 0;
    for (const Part& p : parts) {
        HIP_TRY(hipMemcpyAsync(to_state ? state + off : p.lib, to_state ? p.lib : state + off, p.n * sizeof(float), hipMemcpyDeviceToDevice, st));
        off += p.n;
    }
    return FDCAP_OK;
}
int fdcap_opt_export_state(fdcap_ctx* c, float* state_d, void* stream) {
    if (!c || !c->opt || !state_d) return FDCAP_E_ARG;
    { int es_ = opt_sync(c, (hipStream_t)stream); if (es_) return es_; }
    return opt_state_copy(c, state_d, true, (hipStream_t)stream);
}
int fdcap_opt_import_state(fdcap_ctx* c, const float* state_d, void* stream) {
    if (!c || !c->opt || !state_d) return FDCAP_E_ARG;
    { int es_ = opt_sync(c, (hipStream_t)stream); if (es_) return es_; }
    c->opt->log_pending = false;
    c->opt->ahead = false;
    return opt_state_copy(c, (float*)state_d, false, (hipStream_t)stream);
}
int fdcap_opt_check_finite(fdcap_ctx* c, int32_t* count_d, void* stream) {
    if (!c || !c->opt || !count_d) return FDCAP_E_ARG;
    { int es_ = opt_sync(c, (hipStream_t)stream); if (es_) return es_; }
    OptState* o = c->opt;
    hipStream_t st = (hipStream_t)stream;
    const size_t nx = (size_t)o->cfg.n_local * XDIM, ncam = (size_t)o->cfg.n_local * 16;
    HIP_TRY(hipMemsetAsync(count_d, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(count_nonfinite_kernel, dim3((unsigned)((nx + 255) / 256)), dim3(256), 0, st, o->X.p + 2 * XDIM, nx, count_d);
    hipLaunchKernelGGL(count_nonfinite_kernel, dim3((unsigned)((ncam + 255) / 256)), dim3(256), 0, st, o->CAM.p + 2 * 16, ncam, count_d);
    hipLaunchKernelGGL(count_nonfinite_kernel, dim3((o->nclip + 63) / 64), dim3(64), 0, st, o->scale.p, (size_t)o->nclip, count_d);
    return (int)hipGetLastError();
}

// ---- optimization.py: the per-frame smoother (:185-238, :334-348) ------------------------------
int fdcap_frame_smoother(fdcap_ctx* c, const float* data78, int32_t N, int32_t iters, float lr, float w_rec, float w_vposer,
                         float w_prev, float* state, int32_t step0, int32_t has_prev, float* out78, void* stream) {
    if (!data78 || !out78 || N <= 0 || iters <= 0 || step0 < 0 || ((step0 > 0 || has_prev) && !state)) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)N * iters;
    std::vector<AdamScalars> local_h;
    std::vector<AdamScalars>& tab_h = c ? c->ws_adam_h : local_h;
    tab_h.resize(n);
    for (size_t i = 0; i < n; ++i) tab_h[i] = adam_scalars(lr, step0 + (int)(i + 1));
    DevBuf<AdamScalars> local_d;
    DevBuf<AdamScalars>& tab_d = c ? c->ws_adam : local_d;      // ctx == NULL: a temporary, freed on return after a stream sync
    HIP_TRY(tab_d.ensure(n));
    HIP_TRY(hipMemcpyAsync(tab_d.p, tab_h.data(), n * sizeof(AdamScalars), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(frame_smoother_kernel, dim3(1), dim3(128), 0, st, data78, N, iters, tab_d.p,
                       smoother_weights(w_rec, w_vposer, w_prev), state, (step0 > 0 || has_prev) ? 1 : 0, has_prev ? 1 : 0, out78);
    if (!c) HIP_TRY(hipStreamSynchronize(st));
    return (int)hipGetLastError();
}

namespace {
int opt_step_launch(fdcap_ctx* c, int32_t ii, int32_t P, bool do_rows, bool do_scale, bool reduce_scale, hipStream_t st, float* xch) {
    OptState* o = c->opt;
    const int nl = o->cfg.n_local;
    if (do_rows) o->ahead = false;                         // the rows change: a forward that ran ahead of this step is stale
    const StepPlan sp = opt_step_plan(o, ii, P, do_rows, do_scale);
    const bool tail = sp.step_scale || reduce_scale;                 // the last block(s): (reduction +) scale (+ message tail)
    if (sp.nb_x + sp.nb_cam + (tail ? 1 : 0) + (o->log_pending ? 1 : 0) == 0) return FDCAP_OK;
    TraceRange tr_("fdcap:adam(K22)");
    const int K = o->nclip, rpc = o->rows_per_clip();               // (a batch of clips: one scale block and one log block per clip)
    const LogReduceIn lg = {o->loss_rows.p, o->log_dst, o->log_mask, o->log_assign, rpc};
    hipLaunchKernelGGL(adam_step_kernel, dim3(sp.nb_x + sp.nb_cam + K + (o->log_pending ? K : 0)), dim3(256), 0, st, sp.x, sp.cam, sp.sc, sp.nb_x, sp.nb_cam,
                       o->dscale_row.p, 2, reduce_scale ? rpc : 0, o->dscale.p, (sp.step_scale && ii >= P) ? 1 : 0, xch, nl, o->CAM.p,
                       (do_rows && o->dz_pending) ? (const float*)o->dZpart.p : (const float*)nullptr, (size_t)o->R * VP_Z, lg, K, o->cspan());
    o->log_pending = false;
    if (do_rows) o->dz_pending = false;
    return (int)hipGetLastError();
}
}  // namespace

static int opt_step_impl(fdcap_ctx* c, int32_t ii, int32_t P, bool do_rows, bool do_scale, bool reduce_scale, void* stream,
                         float* xch = nullptr) {
    if (!c || !c->opt) return FDCAP_E_STATE;
    int e = opt_sync(c, (hipStream_t)stream);              // (a deferred step nobody consumed comes first)
    if (e) return e;
    return opt_step_launch(c, ii, P, do_rows, do_scale, reduce_scale, (hipStream_t)stream, xch);
}

int fdcap_opt_sync(fdcap_ctx* c, void* stream) {
    if (!c || !c->opt) return FDCAP_E_STATE;
    return opt_sync(c, (hipStream_t)stream);
}

}  // extern "C"
