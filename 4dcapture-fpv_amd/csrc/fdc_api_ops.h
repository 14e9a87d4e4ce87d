// C-ABI, part 1 (include/fdcap.h): context, scene and contact-set registration, the three operators (Chamfer, VPoser decode,
// body model) with their backward passes, parameter conversions.  Part of csrc/fdcap.hip.
#pragma once

extern "C" {

const char* fdcap_version(void) { return "fdcap-hip 0.4 (gfx950)"; }
const char* fdcap_build_info(void) {
#ifdef FDC_BUILD_NO_PK_F32
    return "packed_fp32=off";
#else
    return "packed_fp32=on";
#endif
}

#ifdef FDC_DEBUG_BUFFERS
int fdcap_debug_stage_bad(unsigned* out) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stage_bad), sizeof(unsigned) * 8 * 16));
    return 0;
}
// instrumentation build only (tools/pk_where.py): row r0.. of an internal per-frame buffer, `per_row` floats per row
// which: 0 O [126], 1 PF [NPFX], 2 A [55*12], 3 M [12], 4 Voff [3 nc], 5 Vw [3 nc], 6 G [55*12], 7 Opart q=0 [126], 8 H2 [512], 9 Jw [69], 10 Rm [55*9], 11 Jrest [55*3]
int fdcap_debug_rows(fdcap_ctx* c, int which, float* dst, void* stream) {
    if (!c || !c->opt) return FDCAP_E_STATE;
    OptState* o = c->opt;
    const int nl = o->cfg.n_local, nc = c->nc;
    const float* src = nullptr; size_t w = 0;
    switch (which) {
        case 0: src = o->O.p; w = O_LD; break;       // (padded rows)
        case 1: src = o->PF.p; w = NPFX; break;
        case 2: src = o->A.p; w = NJ * 12; break;
        case 3: src = o->M.p; w = 12; break;
        case 4: src = o->Voff.p; w = (size_t)3 * nc; break;
        case 5: src = o->Vw.p; w = (size_t)3 * nc; break;
        case 6: src = o->G.p; w = NJ * 12; break;
        case 7: src = o->Opart.p; w = ODIM; break;
        case 8: src = o->H2.p; w = VP_H; break;
        case 9: src = o->Jw.p; w = NJW * 3; break;
        case 10: src = o->Rm.p; w = RM_LD; break;
        case 11: src = o->Jrest.p; w = JR_LD; break;
        default: return FDCAP_E_ARG;
    }
    HIP_TRY(hipMemcpyAsync(dst, src + 2 * w, (size_t)nl * w * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return (int)w;
}
#endif
#ifdef FDC_NN_STATS
int fdcap_debug_nn_hist(unsigned long long* out) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nn_hist), 96 * sizeof(unsigned long long)));
    unsigned long long z[96] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_nn_hist), z, sizeof(z)));
    return 0;
}
// r15: counts entering the three box-test stages since the last call (g_nn_box: 3 sites x {<= 8, <= 16, <= 32, > 32, sum, largest})
int fdcap_debug_nn_box_hist(unsigned long long* out) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nn_box), 18 * sizeof(unsigned long long)));
    unsigned long long z[18] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_nn_box), z, sizeof(z)));
    return 0;
}
int fdcap_debug_nn_stats(unsigned long long* out) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nn_stats), 8 * sizeof(unsigned long long)));
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_nn_stats), z, sizeof(z)));
    return 0;
}
#endif

#ifdef FDC_NN_TIMELINE
int fdcap_debug_nn_timeline(unsigned long long* out, int n) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nn_timeline), (size_t)n * sizeof(unsigned long long)));
    return 0;
}
#endif
#ifdef FDC_PN_TIMING
int fdcap_debug_frame_times(unsigned long long* out) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fr_times), sizeof(unsigned long long) * 3 * 2048 * 8));
    return 0;
}
int fdcap_debug_panel_reset(void) {
    HIP_TRY(hipDeviceSynchronize());
    static std::vector<unsigned long long> z(8192 * 8, 0ull);
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_pn_times), z.data(), z.size() * sizeof(unsigned long long)));
    return 0;
}
int fdcap_debug_panel_times(unsigned long long* out, int n) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pn_times), (size_t)n * sizeof(unsigned long long)));
    return 0;
}
#endif

// test / diagnosis: the kernel forms launched since the last call with reset != 0 (fdc_math.h FormLog), "a;b;c" into buf
int fdcap_debug_kernel_forms(char* buf, int32_t len, int32_t reset) {
    if (!buf || len <= 0) return FDCAP_E_ARG;
    FormLog& f = form_log();
    std::string s;
    for (int i = 0; i < f.n; ++i) { if (i) s += ";"; s += f.name[i]; }
    snprintf(buf, (size_t)len, "%s", s.c_str());
    if (reset) f.n = 0;
    return FDCAP_OK;
}

// test / diagnosis: the packed wave sums (fdc_math.h wave_sum64_pack) next to wave_sum64 per value, one wave on in_h [64][n]
int fdcap_debug_wave_sum_pack(const float* in_h, int32_t n, float* packed_h, float* each_h) {
    if (!in_h || !packed_h || !each_h || n < 1 || n > 16) return FDCAP_E_ARG;
    DevBuf<float> in, out;
    hipError_t e = in.upload(in_h, (size_t)64 * n);
    if (e == hipSuccess) e = out.ensure((size_t)2 * n);
    if (e != hipSuccess) return (int)e;
    switch (n) {
#define FDC_WSP_CASE(N) case N: wave_sum_pack_debug_kernel<N><<<1, 64>>>(in.p, out.p, out.p + n); break;
    FDC_WSP_CASE(1) FDC_WSP_CASE(2) FDC_WSP_CASE(3) FDC_WSP_CASE(4) FDC_WSP_CASE(5) FDC_WSP_CASE(6) FDC_WSP_CASE(7) FDC_WSP_CASE(8)
    FDC_WSP_CASE(9) FDC_WSP_CASE(10) FDC_WSP_CASE(11) FDC_WSP_CASE(12) FDC_WSP_CASE(13) FDC_WSP_CASE(14) FDC_WSP_CASE(15) FDC_WSP_CASE(16)
#undef FDC_WSP_CASE
    }
    e = hipGetLastError();
    const hipError_t es = hipDeviceSynchronize();                // (the buffers are freed on return: wait, whatever the launch said)
    if (e == hipSuccess) e = es;
    if (e == hipSuccess) e = hipMemcpy(packed_h, out.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(each_h, out.p + n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    return e == hipSuccess ? FDCAP_OK : (int)e;
}

// test / diagnosis: what the owning types of fdc_own.h hold in this process right now: out3 = {blocks (device and pinned host), their
// bytes, events}.  Tests take differences around a create ... destroy pair.
int fdcap_debug_live_allocations(int64_t* out3) {
    if (!out3) return FDCAP_E_ARG;
    out3[0] = g_live_blocks.load(); out3[1] = g_live_bytes.load(); out3[2] = g_live_events.load();
    return FDCAP_OK;
}

// test / diagnosis: the joint sets (plan_pose_joints, fdc_forms.h) of the optimiser's last pose forward and pose backward launch:
// out8 = {forward jn, jr, nlev, world; backward jn, jr, nlev, world}
int fdcap_debug_pose_joint_sets(fdcap_ctx* c, int32_t* out8) {
    if (!c || !c->opt || !out8) return FDCAP_E_STATE;
    const PoseJoints* p[2] = {&c->opt->pj_fwd, &c->opt->pj_bwd};
    for (int k = 0; k < 2; ++k) { out8[4 * k] = p[k]->jn; out8[4 * k + 1] = p[k]->jr; out8[4 * k + 2] = p[k]->nlev; out8[4 * k + 3] = p[k]->world ? 1 : 0; }
    return FDCAP_OK;
}

int fdcap_set_nn_kernel(int32_t mode) {
    if (mode < 0 || mode > 2) return FDCAP_E_ARG;
    nn_mode_ref() = mode;
    return FDCAP_OK;
}

int fdcap_ctx_create(const fdcap_model_desc* md, fdcap_ctx** out) {
    if (!md || !out || md->num_verts <= 0 || md->num_shape < NBETA) return FDCAP_E_ARG;
    if (!md->v_template || !md->shapedirs || !md->posedirs || !md->J_regressor || !md->parents ||
        !md->lbs_weights || !md->hands_componentsl || !md->hands_componentsr || !md->hands_meanl ||
        !md->hands_meanr || !md->vp_fc1_w || !md->vp_fc1_b || !md->vp_fc2_w || !md->vp_fc2_b || !md->vp_out_w ||
        !md->vp_out_b)
        return FDCAP_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return FDCAP_E_NODEVICE;
    SetupTrace tr("fdcap_ctx_create");
    fdcap_ctx* c = new fdcap_ctx();
    const int V = c->V = md->num_verts;
    c->h_vt.assign(md->v_template, md->v_template + (size_t)V * 3);
    c->h_S10.resize((size_t)V * 30);
    for (size_t i = 0; i < (size_t)V * 3; ++i)
        for (int l = 0; l < NBETA; ++l) c->h_S10[i * NBETA + l] = md->shapedirs[i * md->num_shape + l];
    c->h_lbs.assign(md->lbs_weights, md->lbs_weights + (size_t)V * NJ);
    if (md->num_shape >= NBETA + NEXPR) {                 // the expression directions, kept for fdcap_set_keypoint_map's tables
        c->h_E10.resize((size_t)V * 3 * NEXPR);
        for (size_t i = 0; i < (size_t)V * 3; ++i)
            for (int l = 0; l < NEXPR; ++l) c->h_E10[i * NEXPR + l] = md->shapedirs[i * md->num_shape + NBETA + l];
        c->h_JE.resize((size_t)NJ * 3 * NEXPR);
        expr_joint_dirs(V, c->h_E10.data(), md->J_regressor, c->h_JE.data());
    }
    tr.mark("host copies of the model");
    {   // posedirs (61 MB for SMPL-X) goes straight to the device: vertex sets gather their blend matrix there (build_skin_set)
        hipError_t e_ = c->d_posedirs.upload(md->posedirs, (size_t)NPF * 3 * V);
        if (e_ == hipSuccess) e_ = c->d_S10.upload(c->h_S10.data(), c->h_S10.size());
        if (e_ != hipSuccess) { fdcap_ctx_destroy(c); return (int)e_; }
    }
    tr.mark("posedirs upload");
    HostPoseSetup hs;
    if (!host_pose_setup(V, c->h_vt.data(), c->h_S10.data(), md->J_regressor, md->parents, &hs)) { delete c; return FDCAP_E_ARG; }
    tr.mark("host_pose_setup");
    std::vector<float>&Jt = hs.Jt, &Jd = hs.Jd;
    std::vector<int>&parents = hs.parents, &order = hs.order, &level_start = hs.level_start,
                    &child_start = hs.child_start, &child_list = hs.child_list;
    c->nlevels = hs.nlevels;
    c->h_parents = hs.parents; c->h_depth = hs.depth;
    std::vector<float> hc(2 * 12 * 45), hm(90);
    memcpy(hc.data(), md->hands_componentsl, 12 * 45 * sizeof(float));
    memcpy(hc.data() + 12 * 45, md->hands_componentsr, 12 * 45 * sizeof(float));
    memcpy(hm.data(), md->hands_meanl, 45 * sizeof(float));
    memcpy(hm.data() + 45, md->hands_meanr, 45 * sizeof(float));
    int err = 0;
#define UP(buf, ptr, cnt) if (!err) { hipError_t e_ = (buf).upload(ptr, cnt); if (e_ != hipSuccess) err = (int)e_; }
    UP(c->Jt, Jt.data(), Jt.size()) UP(c->Jd, Jd.data(), Jd.size())
    UP(c->parents, parents.data(), parents.size()) UP(c->order, order.data(), order.size())
    UP(c->level_start, level_start.data(), level_start.size())
    UP(c->child_start, child_start.data(), child_start.size()) UP(c->child_list, child_list.data(), child_list.size())
    UP(c->depth, hs.depth.data(), hs.depth.size())
    UP(c->hand_comp, hc.data(), hc.size()) UP(c->hand_mean, hm.data(), hm.size())
    {   // the same tables once more, laid out as PoseStage's static part
        std::vector<float> img((size_t)PS_STATIC_FLOATS, 0.f);
        auto put = [&](size_t off_bytes, const void* src, size_t n_words) { memcpy((char*)img.data() + off_bytes, src, n_words * 4); };
        put(offsetof(PoseStage, Jd), Jd.data(), Jd.size());
        put(offsetof(PoseStage, hand_comp), hc.data(), hc.size());
        put(offsetof(PoseStage, Jt), Jt.data(), Jt.size());
        put(offsetof(PoseStage, hand_mean), hm.data(), hm.size());
        put(offsetof(PoseStage, parents), parents.data(), parents.size());
        put(offsetof(PoseStage, order), order.data(), order.size());
        put(offsetof(PoseStage, level_start), level_start.data(), std::min<size_t>(level_start.size(), MAX_LEVELS + 4));
        put(offsetof(PoseStage, child_start), child_start.data(), child_start.size());
        put(offsetof(PoseStage, child_list), child_list.data(), child_list.size());
        put(offsetof(PoseStage, depth), hs.depth.data(), hs.depth.size());
        UP(c->pose_tab, img.data(), img.size())
    }
    UP(c->W1, md->vp_fc1_w, 512 * 32) UP(c->b1, md->vp_fc1_b, 512)
    UP(c->W2, md->vp_fc2_w, 512 * 512) UP(c->b2, md->vp_fc2_b, 512)
    UP(c->W3, md->vp_out_w, ODIM * 512) UP(c->b3, md->vp_out_b, ODIM)
#undef UP
    tr.mark("small uploads");
    if (!err) {
        // decoder weights in MFMA fragment order.  torch Linear weights are [out, in]: forward y = x W^T -> B(k, n) = W[n][k];
        // data gradient dx = dy W -> B(k, n) = W[k][n]
        struct { const float* w; long sk, sn; int K, N; PanelB* dst; } pk[6] = {
            {md->vp_fc1_w, 1, VP_Z, VP_Z, VP_H, &c->vp.w1}, {md->vp_fc2_w, 1, VP_H, VP_H, VP_H, &c->vp.w2},
            {md->vp_out_w, 1, VP_H, VP_H, ODIM, &c->vp.w3}, {md->vp_out_w, VP_H, 1, ODIM, VP_H, &c->vp.w3t},
            {md->vp_fc2_w, VP_H, 1, VP_H, VP_H, &c->vp.w2t}, {md->vp_fc1_w, VP_Z, 1, VP_H, VP_Z, &c->vp.w1t}};
        const float* dw[6] = {c->W1.p, c->W2.p, c->W3.p, c->W3.p, c->W2.p, c->W1.p};        // the same weights on the device (uploaded above)
        const size_t dwn[6] = {(size_t)512 * 32, (size_t)512 * 512, (size_t)ODIM * 512, (size_t)ODIM * 512, (size_t)512 * 512, (size_t)512 * 32};
        for (int i = 0; i < 6 && !err; ++i) {
            int nt = 0, ns = 0;
            err = panel_pack_dev(dw[i], dwn[i], pk[i].sk, pk[i].sn, pk[i].K, pk[i].N, c->vp_pn[i], &nt, &ns);
            pk[i].dst->f = (const float4*)c->vp_pn[i].p; pk[i].dst->ntile = nt; pk[i].dst->nss = ns;
        }
        c->vp.b1 = c->b1.p; c->vp.b2 = c->b2.p; c->vp.b3 = c->b3.p;
        PanelB3* dst3[6] = {&c->vp3.w1, &c->vp3.w2, &c->vp3.w3, &c->vp3.w3t, &c->vp3.w2t, &c->vp3.w1t};
        float c1n[6];                                                      // largest column 1-norm of each operand (VPoserPanels3::c1 ...)
        for (int i = 0; i < 6 && !err; ++i) {
            err = pnf_pack_dev(dw[i], dwn[i], pk[i].sk, pk[i].sn, pk[i].K, pk[i].N, c->vp_pn3[i], c->vp_pn3s[i], &dst3[i]->ntile, &dst3[i]->nst);
            dst3[i]->f = (const uint4*)c->vp_pn3[i].p; dst3[i]->isc = c->vp_pn3s[i].p;
            double mx = 0.0;
            for (int n = 0; n < pk[i].N; ++n) {
                double a = 0.0;
                for (int k = 0; k < pk[i].K; ++k) a += fabs((double)pk[i].w[(long)k * pk[i].sk + (long)n * pk[i].sn]);
                mx = std::max(mx, a);
            }
            c1n[i] = (float)(mx * 1.001);
        }
        auto amax = [](const float* b, int n) { float m = 0.f; for (int i = 0; i < n; ++i) m = std::max(m, fabsf(b[i])); return m * 1.001f; };
        c->vp3.c1 = c1n[0]; c->vp3.c2 = c1n[1]; c->vp3.c3t = c1n[3]; c->vp3.c2t = c1n[4];
        c->vp3.b1max = amax(md->vp_fc1_b, 512); c->vp3.b2max = amax(md->vp_fc2_b, 512);
        c->vp3.b1 = c->b1.p; c->vp3.b2 = c->b2.p; c->vp3.b3 = c->b3.p;
    }
    tr.mark("decoder panels");
    if (err) { fdcap_ctx_destroy(c); return err; }
    *out = c;
    return FDCAP_OK;
}

void fdcap_ctx_destroy(fdcap_ctx* c) {
    if (!c) return;
    fdcap_opt_destroy(c);
    (void)fdcap_comm_destroy(c);                            // (before the exchange buffers, which `delete` frees with everything else)
    delete c;
}

// the table set of one slot (fdcap_set_scene: slot 0)
static int scene_set_build(SceneSet* c, const float* xyz, int64_t ns) {
    c->ns = 0;                                              // (no scene until the new tables are complete: a failure below leaves none)
    static_assert(SC_SUPER == ST4_SUPER, "fdc_scene.h builds the super-cell boxes the search reads");
    // Spatial order by recursive median splits (k-d cells): every MF_CH-point chunk is one cell and every 32-point MFMA tile inside it
    // a sub-cell, so the boxes the NN scan culls with are compact and disjoint (runs of a Morton curve jump across quadrant borders
    // and give long, overlapping boxes).  r6: sorted, boxed and packed ON THE DEVICE (fdc_scene.h); FDCAP_SCENE_BUILD=host takes the
    // order from the host recursion of r1-r5 instead (the same order by specification: tests compare the
    // tables of the two, and of both with tests/scene_spec.py).
    // Results never depend on this order.
    const int64_t nchunk = (ns + MF_CH - 1) / MF_CH, nsuper = (nchunk + ST4_SUPER - 1) / ST4_SUPER;
    HIP_TRY(c->scene.ensure((size_t)ns)); HIP_TRY(c->scene_sorted.ensure((size_t)ns)); HIP_TRY(c->scene_inv.ensure((size_t)ns));
    HIP_TRY(c->scene_bounds.ensure((size_t)nchunk * 2)); HIP_TRY(c->scene_qbounds.ensure((size_t)nchunk * 24));    // (quarters, then eighths)
    HIP_TRY(c->scene_frags.ensure((size_t)nchunk * (MF_CH / 32) * 64)); HIP_TRY(c->scene_centers.ensure((size_t)nchunk));
    {
        std::vector<float4> sb((size_t)std::max<int64_t>(nsuper, 1) * 2, make_float4(0.f, 0.f, 0.f, 0.f));
        HIP_TRY(c->scene_sbounds.upload(sb.data(), sb.size()));
    }
    const char* how = getenv("FDCAP_SCENE_BUILD");
    std::vector<int> order;
    const bool host_order = how && !strcmp(how, "host");
    if (host_order) scene_order_host(xyz, ns, order);
    const SceneTables T{c->scene.p, c->scene_sorted.p, c->scene_inv.p, c->scene_bounds.p, c->scene_qbounds.p, c->scene_sbounds.p,
                        c->scene_frags.p, c->scene_centers.p};
    HIP_TRY(scene_build_device(xyz, ns, T, host_order ? order.data() : nullptr));
    c->ns = ns;
    return FDCAP_OK;
}

int fdcap_set_scene(fdcap_ctx* c, const float* xyz, int64_t ns) {
    // FDCAP_MAX_SCENE_POINTS: the in-loop NN launch streams the scene's MFMA fragments (32 B per point) through one buffer
    // resource with 32-bit byte offsets; beyond 2 GiB of fragments its loads would silently return zeros
    if (!c || ns < 0 || (ns > 0 && !xyz) || ns > FDCAP_MAX_SCENE_POINTS) return FDCAP_E_ARG;
    // a live optimiser holds buffers sized for, and pruning state (seeds, kept work lists) valid for, the registered scene
    if (c->opt) return FDCAP_E_STATE;
    c->sop.nq = 0;                                          // (the scene operator's seeds / kept lists were for the old scene)
    return scene_set_build(&c->scenes[0], xyz, ns);
}

// Slot 0 is fdcap_set_scene.  The other slots follow its rules; ns = 0 frees the slot's tables.
int fdcap_set_scene_slot(fdcap_ctx* c, int32_t slot, const float* xyz, int64_t ns) {
    if (!c || slot < 0 || slot >= FDCAP_MAX_SCENES) return FDCAP_E_ARG;
    if (slot == 0) return fdcap_set_scene(c, xyz, ns);
    if (ns < 0 || (ns > 0 && !xyz) || ns > FDCAP_MAX_SCENE_POINTS) return FDCAP_E_ARG;
    if (c->opt) return FDCAP_E_STATE;
    if (ns == 0) { c->scenes[slot].release(); return FDCAP_OK; }
    return scene_set_build(&c->scenes[slot], xyz, ns);
}

// test / diagnosis: FNV-1a hashes of the registered scene's eight device tables (input-order points, sorted points, inverse
// permutation, cell boxes, quarter boxes, super-cell boxes, fragments, centres), so two builds of the same scene can be compared
int fdcap_debug_scene_hash(fdcap_ctx* c, uint64_t* out8) {
    if (!c || !out8) return FDCAP_E_ARG;
    HIP_TRY(hipDeviceSynchronize());
    const int64_t ns = c->ns, nchunk = (ns + MF_CH - 1) / MF_CH, nsuper = std::max<int64_t>((nchunk + ST4_SUPER - 1) / ST4_SUPER, 1);
    struct { const void* p; size_t bytes; } t[8] = {
        {c->scene.p, (size_t)ns * 16}, {c->scene_sorted.p, (size_t)ns * 16}, {c->scene_inv.p, (size_t)ns * 4},
        {c->scene_bounds.p, (size_t)nchunk * 32}, {c->scene_qbounds.p, (size_t)nchunk * 128}, {c->scene_sbounds.p, (size_t)nsuper * 32},
        {c->scene_frags.p, (size_t)nchunk * (MF_CH / 32) * 64 * 16}, {c->scene_centers.p, (size_t)nchunk * 16}};
    std::vector<unsigned char> h;
    for (int i = 0; i < 8; ++i) {
        h.resize(t[i].bytes);
        if (t[i].bytes) HIP_TRY(hipMemcpy(h.data(), t[i].p, t[i].bytes, hipMemcpyDeviceToHost));
        uint64_t v = 1469598103934665603ull;
        for (size_t k = 0; k < t[i].bytes; ++k) { v ^= h[k]; v *= 1099511628211ull; }
        out8[i] = v;
    }
    return FDCAP_OK;
}

// test / diagnosis: one of the same eight tables copied to the host as it is, so a test can compare it with a specification
// (tests/scene_spec.py).  `which` in the order of fdcap_debug_scene_hash; host_out == nullptr: *bytes <- the table's size
int fdcap_debug_scene_table(fdcap_ctx* c, int32_t which, void* host_out, int64_t* bytes) {
    if (!c || !bytes || which < 0 || which > 7) return FDCAP_E_ARG;
    if (c->ns <= 0 || !c->scene_sorted.p) return FDCAP_E_STATE;
    const int64_t ns = c->ns, nchunk = (ns + MF_CH - 1) / MF_CH, nsuper = std::max<int64_t>((nchunk + ST4_SUPER - 1) / ST4_SUPER, 1);
    const void* p[8] = {c->scene.p, c->scene_sorted.p, c->scene_inv.p, c->scene_bounds.p, c->scene_qbounds.p, c->scene_sbounds.p,
                        c->scene_frags.p, c->scene_centers.p};
    const int64_t sz[8] = {ns * 16, ns * 16, ns * 4, nchunk * 32, nchunk * 128, nsuper * 32, nchunk * (MF_CH / 32) * 64 * 16, nchunk * 16};
    if (!host_out) { *bytes = sz[which]; return FDCAP_OK; }
    if (*bytes != sz[which]) return FDCAP_E_ARG;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, p[which], (size_t)sz[which], hipMemcpyDeviceToHost));
    return FDCAP_OK;
}

int fdcap_set_contact_ids(fdcap_ctx* c, const int64_t* vid, int32_t nc) {
    if (!c || nc < 0 || (nc > 0 && !vid)) return FDCAP_E_ARG;
    if (c->opt) return FDCAP_E_STATE;                  // (see fdcap_set_scene)
    SetupTrace tr("fdcap_set_contact_ids");
    for (int i = 0; i < nc; ++i) if (vid[i] < 0 || vid[i] >= c->V) return FDCAP_E_ARG;
    // Internal slot order = Morton order of the template positions: the 256 consecutive queries of an NN
    // workgroup are then spatially compact, so far fewer scene chunks survive its bound test (with all
    // 10 475 vertices as contacts a workgroup would otherwise span the whole body).  The loss is a mean
    // over the contact set, so the order is free; outputs go back in the caller's order via contact_perm.
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
    for (int i = 0; i < nc; ++i)
        for (int k = 0; k < 3; ++k) {
            float v = c->h_vt[3 * vid[i] + k];
            lo[k] = std::min(lo[k], v); hi[k] = std::max(hi[k], v);
        }
    auto spread = [](uint32_t v) { v &= 1023; v = (v | (v << 16)) & 0x030000FF; v = (v | (v << 8)) & 0x0300F00F;
                                   v = (v | (v << 4)) & 0x030C30C3; v = (v | (v << 2)) & 0x09249249; return v; };
    std::vector<std::pair<uint32_t, int>> key((size_t)nc);
    for (int i = 0; i < nc; ++i) {
        uint32_t code = 0;
        for (int k = 0; k < 3; ++k) {
            float ext = hi[k] - lo[k];
            float u = ext > 0.f ? (c->h_vt[3 * vid[i] + k] - lo[k]) / ext : 0.f;
            code |= spread((uint32_t)std::min(1023.f, std::max(0.f, u * 1023.f))) << k;
        }
        key[i] = {code, i};
    }
    std::sort(key.begin(), key.end());
    std::vector<int64_t> ids((size_t)nc);
    std::vector<int> perm((size_t)std::max(nc, 1), 0), v32((size_t)std::max(nc, 1), 0);
    for (int sl = 0; sl < nc; ++sl) { ids[sl] = vid[key[sl].second]; perm[sl] = key[sl].second; }
    for (int i = 0; i < nc; ++i) v32[i] = (int)vid[i];
    tr.mark("slot order");
    int e = build_skin_set(c, ids, &c->contact);
    if (e) return e;
    tr.mark("build_skin_set");
    HIP_TRY(c->contact_vid.upload(v32.data(), v32.size()));
    HIP_TRY(c->contact_perm.upload(perm.data(), perm.size()));
    c->nc = nc;
    return FDCAP_OK;
}

// ---- Op 1 ----------------------------------------------------------------------------------
int fdcap_chamfer_fwd(fdcap_ctx* c, const float* xyz1, const float* xyz2, int32_t B, int32_t n, int32_t m,
                      int64_t stride2, float* dist1, int32_t* idx1, float* dist2, int32_t* idx2, void* stream) {
    if (!c || !xyz1 || !xyz2 || B <= 0 || n <= 0 || m <= 0) return FDCAP_E_ARG;
    if ((dist1 && !idx1) || (dist2 && !idx2) || (!dist1 && !dist2)) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const bool shared = (stride2 == 0);
    size_t big = (size_t)std::max(n, m);
    // Per-batch targets and the reverse direction: one launch set for all batches (nn_search_batched), or -- FDCAP_CHAMFER_BATCHED=0,
    // read on every call -- the per-batch loop at the end, which is the specification: the batched path returns its bits.
    const char* const sw = getenv("FDCAP_CHAMFER_BATCHED");
    const bool batched = !(sw && sw[0] == '0') && (!shared || dist2);
    // packed targets: the loop keeps the shared scene [m] and one batch's set behind it; the batched path packs all B sets of one
    // direction at the front (the launches that read the buffer are ordered on the stream, so the directions take turns)
    if (batched) HIP_TRY(c->ws_p.ensure(std::max(shared ? (size_t)m : dist1 ? (size_t)B * m : 0, dist2 ? (size_t)B * n : 0)));
    else HIP_TRY(c->ws_p.ensure(shared ? (size_t)m + (dist2 ? big : 0) : big));
    if (shared && dist1) {
        hipLaunchKernelGGL(pack_points_kernel, dim3((m + 255) / 256), dim3(256), 0, st, xyz2, m, c->ws_p.p);
        int nq = B * n;
        int nsplit = nn_pick_nsplit(nq, m);
        HIP_TRY(c->ws_f[0].ensure((size_t)nsplit * nq));
        HIP_TRY(c->ws_i[0].ensure((size_t)nsplit * nq));
        { NNTarget T{c->ws_p.p, m, nullptr, nullptr, nullptr, nullptr, nullptr}; HIP_TRY(nn_search(xyz1, nq, T, dist1, idx1, c->ws_f[0].p, c->ws_i[0].p, nsplit, st)); }
    }
    if (batched) {
        const int mode = nn_mode_ref();
        if (!shared && dist1) {                                  // x1[b] -> x2[b]
            const NNBatchPlan pl = plan_nn_batched(n, m, B, mode);
            HIP_TRY(c->ws_f[0].ensure((size_t)B * pl.nsplit * n));
            HIP_TRY(c->ws_i[0].ensure((size_t)B * pl.nsplit * n));
            HIP_TRY(nn_search_batched(pl, xyz1, (long long)n * 3, n, xyz2, stride2, m, B, c->ws_p.p, dist1, idx1, c->ws_f[0].p, c->ws_i[0].p, st));
        }
        if (dist2) {                                             // x2[b] (or the one shared x2) -> x1[b]
            const NNBatchPlan pl = plan_nn_batched(m, n, B, mode);
            HIP_TRY(c->ws_f[1].ensure((size_t)B * pl.nsplit * m));
            HIP_TRY(c->ws_i[1].ensure((size_t)B * pl.nsplit * m));
            HIP_TRY(nn_search_batched(pl, xyz2, stride2, m, xyz1, (long long)n * 3, n, B, c->ws_p.p, dist2, idx2, c->ws_f[1].p, c->ws_i[1].p, st));
        }
        return (int)hipGetLastError();
    }
    for (int b = 0; b < B && (!shared || dist2); ++b) {
        const float* x1 = xyz1 + (size_t)b * n * 3;
        const float* x2 = xyz2 + (size_t)b * stride2;
        float4* pk = c->ws_p.p + (shared ? m : 0);
        if (!shared && dist1) {
            hipLaunchKernelGGL(pack_points_kernel, dim3((m + 255) / 256), dim3(256), 0, st, x2, m, pk);
            int nsplit = nn_pick_nsplit(n, m);
            HIP_TRY(c->ws_f[0].ensure((size_t)nsplit * n));
            HIP_TRY(c->ws_i[0].ensure((size_t)nsplit * n));
            { NNTarget T{pk, m, nullptr, nullptr, nullptr, nullptr, nullptr}; HIP_TRY(nn_search(x1, n, T, dist1 + (size_t)b * n, idx1 + (size_t)b * n, c->ws_f[0].p, c->ws_i[0].p, nsplit, st)); }
        }
        if (dist2) {
            hipLaunchKernelGGL(pack_points_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x1, n, pk);
            int nsplit = nn_pick_nsplit(m, n);
            HIP_TRY(c->ws_f[1].ensure((size_t)nsplit * m));
            HIP_TRY(c->ws_i[1].ensure((size_t)nsplit * m));
            { NNTarget T{pk, n, nullptr, nullptr, nullptr, nullptr, nullptr}; HIP_TRY(nn_search(x2, m, T, dist2 + (size_t)b * m, idx2 + (size_t)b * m, c->ws_f[1].p, c->ws_i[1].p, nsplit, st)); }
        }
    }
    return (int)hipGetLastError();
}

int fdcap_chamfer_bwd(fdcap_ctx* c, const float* xyz1, const float* xyz2, int32_t B, int32_t n, int32_t m,
                      int64_t stride2, const float* gdist1, const int32_t* idx1, float* gxyz1, void* stream) {
    if (!c || !xyz1 || !xyz2 || !gdist1 || !idx1 || !gxyz1 || B <= 0 || n <= 0 || m <= 0) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c->ws_p.ensure(m));
    if (stride2 == 0) {
        hipLaunchKernelGGL(pack_points_kernel, dim3((m + 255) / 256), dim3(256), 0, st, xyz2, m, c->ws_p.p);
        int nq = B * n;
        hipLaunchKernelGGL(nn_grad_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, xyz1, c->ws_p.p, gdist1, idx1, nq, gxyz1);
    } else {
        for (int b = 0; b < B; ++b) {
            hipLaunchKernelGGL(pack_points_kernel, dim3((m + 255) / 256), dim3(256), 0, st, xyz2 + (size_t)b * stride2, m, c->ws_p.p);
            hipLaunchKernelGGL(nn_grad_kernel, dim3((n + 255) / 256), dim3(256), 0, st, xyz1 + (size_t)b * n * 3, c->ws_p.p,
                               gdist1 + (size_t)b * n, idx1 + (size_t)b * n, n, gxyz1 + (size_t)b * n * 3);
        }
    }
    return (int)hipGetLastError();
}

// The whole backward of Op 1 in a defined order (fdc_chamfer_bwd.h): both halves, both inputs, no atomics, O(1) launches in B.
// Workspace (context-owned, grown on demand): ws_ck / ws_cv, the sort scratch of the larger of the two sides.
int fdcap_chamfer_bwd_both(fdcap_ctx* c, const float* xyz1, const float* xyz2, int32_t B, int32_t n, int32_t m, int64_t stride2,
                           const float* gdist1, const int32_t* idx1, const float* gdist2, const int32_t* idx2, float* gxyz1,
                           float* gxyz2, int32_t reduce2, void* stream) {
    if (!c || !xyz1 || !xyz2 || B <= 0 || n <= 0 || m <= 0) return FDCAP_E_ARG;
    if ((gdist1 != nullptr) != (idx1 != nullptr) || (gdist2 != nullptr) != (idx2 != nullptr)) return FDCAP_E_ARG;
    if ((!gdist1 && !gdist2) || (!gxyz1 && !gxyz2)) return FDCAP_E_ARG;
    if (reduce2 != 0 && stride2 != 0) return FDCAP_E_ARG;
    const long long N1 = (long long)B * n, N2 = (long long)B * m;
    if (N1 > 0x7fffffffLL || N2 > 0x7fffffffLL) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    // side 1's terms are grouped by target for gxyz2, side 2's by query for gxyz1
    const bool sort1 = gxyz2 && gdist1, sort2 = gxyz1 && gdist2;
    const long long ns = std::max(sort1 ? N1 : 0, sort2 ? N2 : 0);
    if (ns > CB_MAX_SORT) return FDCAP_E_ARG;                  // (the sort's tiles index with int)
    if (ns > 0) {
        HIP_TRY(c->ws_ck.ensure(cb_key_words(ns)));
        HIP_TRY(c->ws_cv.ensure(2 * (size_t)ns));
    }
    const long long s1 = (long long)n * 3;
    if (gxyz2) {
        const CbSide side{xyz2, (long long)stride2, xyz1, s1, B, m, n, gdist2, idx2, gdist1, reduce2 != 0 ? 1 : 0};
        const long long nd = reduce2 ? (long long)m : N2;
        const unsigned* skey = nullptr;
        const int* sval = nullptr;
        if (sort1) {
            int buf = 0;
            HIP_TRY(cb_group(idx1, B, n, m, reduce2 == 0, c->ws_ck.p, c->ws_cv.p, c->ws_ck.p + 2 * (size_t)N1, st, &buf));
            skey = c->ws_ck.p + (size_t)buf * N1; sval = c->ws_cv.p + (size_t)buf * N1;
        }
        hipLaunchKernelGGL(cb_gather_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, side, skey, sval, (int)N1, gxyz2);
    }
    if (gxyz1) {
        const CbSide side{xyz1, s1, xyz2, (long long)stride2, B, n, m, gdist1, idx1, gdist2, 0};
        const unsigned* skey = nullptr;
        const int* sval = nullptr;
        if (sort2) {                                           // (the scratch is reused: the launches are ordered on the stream)
            int buf = 0;
            HIP_TRY(cb_group(idx2, B, m, n, true, c->ws_ck.p, c->ws_cv.p, c->ws_ck.p + 2 * (size_t)N2, st, &buf));
            skey = c->ws_ck.p + (size_t)buf * N2; sval = c->ws_cv.p + (size_t)buf * N2;
        }
        hipLaunchKernelGGL(cb_gather_kernel, dim3((unsigned)((N1 + 255) / 256)), dim3(256), 0, st, side, skey, sval, (int)N2, gxyz1);
    }
    return (int)hipGetLastError();
}


// Op 1 against the REGISTERED scene.  The operator API's call site (:292-294) passes the same scene in every iteration of the
// caller's loop; fdcap_chamfer_fwd has to treat it as a foreign point set (unsorted: every pair visited, nn_mfma_kernel).  A caller
// that says "xyz2 is the scene I registered" gets the optimiser loop's search: the k-d-sorted scene with its cell boxes and
// precomputed fragments, seeds from nn_seed_kernel in the first call and from the previous call's neighbours afterwards (while
// B * n stays the same), kept work lists in between.  Results: the same (dist, lowest index among ties) bit for bit.
int fdcap_chamfer_fwd_scene(fdcap_ctx* c, const float* xyz1, int32_t B, int32_t n, float* dist1, int32_t* idx1, int32_t forget,
                            void* stream) {
    if (!c || !xyz1 || !dist1 || !idx1 || B <= 0 || n <= 0 || (int64_t)B * n > 0x7fffffff) return FDCAP_E_ARG;
    if (c->ns <= 0 || !c->scene_sorted.p) return FDCAP_E_STATE;
    hipStream_t st = (hipStream_t)stream;
    fdcap_ctx::SceneOp& so = c->sop;
    const int nq = B * n;
    const bool fresh = forget || so.nq != nq;
    if (so.nq != nq) {
        const size_t ng = ((size_t)nq + 31) / 32, ng4 = 4 * ng;
        HIP_TRY(so.dist.ensure(nq)); HIP_TRY(so.idx.ensure(nq)); HIP_TRY(so.seedpt.ensure(nq));
        HIP_TRY(so.ids.ensure(ng4 * NN_CACHE_CAP)); HIP_TRY(so.hdr.ensure(ng4 + 3 * ng)); HIP_TRY(so.anchor.ensure((size_t)4 * nq));
    }
    if (fresh) {
        const size_t ng = ((size_t)nq + 31) / 32, ng4 = 4 * ng;
        HIP_TRY(hipMemsetAsync(so.idx.p, 0xFF, (size_t)nq * sizeof(int), st));                 // -1: no seed
        HIP_TRY(hipMemsetAsync(so.hdr.p, 0xFF, ng4 * sizeof(int), st));                        // -1: nothing kept
        HIP_TRY(hipMemsetAsync(so.hdr.p + ng4, 0, 3 * ng * sizeof(int), st));
        HIP_TRY(hipMemsetAsync(so.anchor.p, 0, (size_t)4 * nq * sizeof(float4), st));
    }
    so.nq = nq;
    const NNTarget T = c->nn_target(true);
    const int nsplit = nn_pick_nsplit(nq, (int)c->ns, true);
    HIP_TRY(c->ws_f[0].ensure((size_t)nsplit * nq));
    HIP_TRY(c->ws_i[0].ensure((size_t)nsplit * nq));
    static const float slack = forms_read_env().nn_cache_slack;      // (once per process, at the first call)
    const NNCache cache{slack > 0.f ? so.ids.p : nullptr, slack > 0.f ? so.hdr.p : nullptr, so.anchor.p, slack};
    bool pt_written = false;
    HIP_TRY(nn_search(xyz1, nq, T, so.dist.p, so.idx.p, c->ws_f[0].p, c->ws_i[0].p, nsplit, st, so.idx.p, fresh, so.seedpt.p, &pt_written,
                      &cache, nullptr));
    if (!pt_written) so.nq = 0;                             // (a size the streaming search does not take: the next call re-seeds)
    HIP_TRY(hipMemcpyAsync(dist1, so.dist.p, (size_t)nq * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(idx1, so.idx.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToDevice, st));
    return (int)hipGetLastError();
}

// ... and its gradient wrt the queries: the scene points come from the library's own copy (no pack pass per call)
int fdcap_chamfer_bwd_scene(fdcap_ctx* c, const float* xyz1, int32_t B, int32_t n, const float* gdist1, const int32_t* idx1, float* gxyz1,
                            void* stream) {
    if (!c || !xyz1 || !gdist1 || !idx1 || !gxyz1 || B <= 0 || n <= 0) return FDCAP_E_ARG;
    if (c->ns <= 0 || !c->scene.p) return FDCAP_E_STATE;
    const int nq = B * n;
    hipLaunchKernelGGL(nn_grad_kernel, dim3((nq + 255) / 256), dim3(256), 0, (hipStream_t)stream, xyz1, c->scene.p, gdist1, idx1, nq, gxyz1);
    return (int)hipGetLastError();
}

// ---- Op 3 ----------------------------------------------------------------------------------
int fdcap_vposer_decode(fdcap_ctx* c, const float* z, int32_t ldz, int32_t B, float* rot, float* aa, void* stream) {
    if (!c || !z || B <= 0 || ldz < 32 || (!rot && !aa)) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(c->ws_f[2].ensure((size_t)B * 512));
    HIP_TRY(c->ws_f[3].ensure((size_t)B * 512));
    HIP_TRY(c->ws_f[4].ensure((size_t)B * ODIM));
    HIP_TRY(c->ws_part.ensure((size_t)4 * B * ODIM));
    int e = vposer_forward(c, z, ldz, 0, 0, B, c->ws_f[2].p, c->ws_f[3].p, c->ws_part.p, (size_t)B * ODIM, c->ws_f[4].p, st);
    if (e) return e;
    int n = B * 21;
    hipLaunchKernelGGL(sixd_to_rot_kernel, dim3((n + 255) / 256), dim3(256), 0, st, c->ws_f[4].p, n, rot, aa);
    return (int)hipGetLastError();
}

int fdcap_vposer_decode_bwd(fdcap_ctx* c, const float* z, int32_t ldz, int32_t B, const float* g_rot, const float* g_aa, float* g_z,
                            void* stream) {
    if (!c || !z || !g_z || B <= 0 || ldz < 32 || (!g_rot && !g_aa)) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    DevBuf<float>* w = c->ws_b;
    HIP_TRY(w[0].ensure((size_t)B * 512)); HIP_TRY(w[1].ensure((size_t)B * 512)); HIP_TRY(w[2].ensure((size_t)B * ODIM));
    HIP_TRY(w[3].ensure((size_t)B * ODIM)); HIP_TRY(w[4].ensure((size_t)4 * B * VP_Z));
    HIP_TRY(c->ws_part.ensure((size_t)4 * B * ODIM));
    // recompute the forward's activations (the operator keeps no state between calls), then the data-gradient chain
    int e = vposer_forward(c, z, ldz, 0, 0, B, w[0].p, w[1].p, c->ws_part.p, (size_t)B * ODIM, w[2].p, st);
    if (e) return e;
    const int n = B * 21;
    hipLaunchKernelGGL(vposer_out_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w[2].p, n, g_rot, g_aa, w[3].p);
    const size_t ps = (size_t)B * VP_Z;
    if (plan_decoder(gemm_split3_enabled()) == F_VPOSER_SPLIT)
        hipLaunchKernelGGL(vposer_bwd_split3_kernel, dim3(4 * ((B + 15) / 16)), dim3(512), 0, st, c->vp3, w[3].p, 0, B, w[0].p, w[1].p, w[4].p, ps, ScaleTail());
    else
        hipLaunchKernelGGL(vposer_bwd_fused_kernel, dim3(4 * ((B + 15) / 16)), dim3(512), 0, st, c->vp, w[3].p, 0, B, w[0].p, w[1].p, w[4].p, ps, ScaleTail());
    hipLaunchKernelGGL(vposer_fold_dz_rows_kernel, dim3((B * VP_Z + 255) / 256), dim3(256), 0, st, w[4].p, ps, B, g_z);
    return (int)hipGetLastError();
}

// ---- parameter conversions -------------------------------------------------------------------
int fdcap_params_75_to_78(const float* p75, int32_t B, float* x78, void* stream) {
    if (!p75 || !x78 || B <= 0) return FDCAP_E_ARG;
    hipLaunchKernelGGL(p75_to_78_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)stream, p75, B, x78);
    return (int)hipGetLastError();
}
int fdcap_params_78_to_75(const float* x78, int32_t B, float* p75, void* stream) {
    if (!p75 || !x78 || B <= 0) return FDCAP_E_ARG;
    hipLaunchKernelGGL(p78_to_75_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)stream, x78, B, p75);
    return (int)hipGetLastError();
}

// ---- Op 2 ----------------------------------------------------------------------------------
// shared by fdcap_body_forward (body frame) and fdcap_world_mesh (scale + camera_ext @ T(cam_t * scale))
static int body_forward_impl(fdcap_ctx* c, const float* params, int32_t B, const float* cam_ext, const float* scale,
                             float* vertices, float* joints, hipStream_t st) {
    if (vertices && !c->full_ready) {
        std::vector<int64_t> all(c->V);
        for (int i = 0; i < c->V; ++i) all[i] = i;
        int e = build_skin_set(c, all, &c->full);
        if (e) return e;
        c->full_ready = true;
    }
    const int V = c->V;
    const bool world = cam_ext != nullptr && scale != nullptr;
    DevBuf<float>* w = c->ws_f;
    HIP_TRY(w[2].ensure((size_t)B * 512)); HIP_TRY(w[3].ensure((size_t)B * 512)); HIP_TRY(w[4].ensure((size_t)B * ODIM));
    HIP_TRY(w[5].ensure((size_t)B * XDIM)); HIP_TRY(w[6].ensure((size_t)B * NPFX)); HIP_TRY(w[7].ensure((size_t)B * NJ * 12));
    HIP_TRY(w[8].ensure((size_t)B * NJ * 12)); HIP_TRY(w[9].ensure((size_t)B * 16)); HIP_TRY(w[10].ensure(1));
    HIP_TRY(w[1].ensure((size_t)B * 12));
    float* X = w[5].p;
    hipLaunchKernelGGL(p75_to_78_kernel, dim3((B + 127) / 128), dim3(128), 0, st, params, B, X);
    HIP_TRY(c->ws_part.ensure((size_t)4 * B * ODIM));
    int e = vposer_forward(c, X, XDIM, X_LATENT, 0, B, w[2].p, w[3].p, c->ws_part.p, (size_t)B * ODIM, w[4].p, st);
    if (e) return e;
    if (!world) {
        HIP_TRY(hipMemsetAsync(w[9].p, 0, (size_t)B * 16 * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(w[10].p, 0, sizeof(float), st));
    }
    const float* CAM = world ? cam_ext : w[9].p;
    const float* S = world ? scale : w[10].p;
    hipLaunchKernelGGL(pose_fwd_kernel<false>, dim3(B), dim3(64 * POSE_NW), 0, st, c->pose_model(), X, w[4].p, CAM, S, 0,
                       (float*)nullptr, w[6].p, (float*)nullptr, w[7].p, w[8].p, w[1].p, (float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (size_t)0);
    if (joints) hipLaunchKernelGGL(joints_out_kernel, dim3((B * NJ + 255) / 256), dim3(256), 0, st, w[7].p, X, XDIM, B, joints);
    if (vertices) {
        HIP_TRY(w[11].ensure((size_t)B * 3 * V));
        HIP_TRY(blend_forward(c->full, w[6].p, B, w[11].p, st));
        hipLaunchKernelGGL(skin_fwd_kernel, dim3((V + 255) / 256, B), dim3(256), 0, st, c->full.model(), V, X, XDIM, X_BETAS,
                           X_TRANSL, w[11].p, w[8].p, (const float*)w[1].p, S, 0, world ? 1 : 0, vertices);
    }
    return (int)hipGetLastError();
}

int fdcap_body_forward(fdcap_ctx* c, const float* params, int32_t B, float* vertices, float* joints, void* stream) {
    if (!c || !params || B <= 0 || (!vertices && !joints)) return FDCAP_E_ARG;
    return body_forward_impl(c, params, B, nullptr, nullptr, vertices, joints, (hipStream_t)stream);
}

int fdcap_world_mesh(fdcap_ctx* c, const float* params, int32_t B, const float* cam_ext, const float* scale, float* vertices,
                     void* stream) {
    if (!c || !params || B <= 0 || !cam_ext || !scale || !vertices) return FDCAP_E_ARG;
    return body_forward_impl(c, params, B, cam_ext, scale, vertices, nullptr, (hipStream_t)stream);
}

int fdcap_smplx_forward(fdcap_ctx* c, const float* go, const float* bp, const float* betas, const float* lh, const float* rh,
                        const float* transl, int32_t B, float* vertices, float* joints, void* stream) {
    if (!c || !go || !bp || !betas || !lh || !rh || !transl || B <= 0 || (!vertices && !joints)) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (vertices && !c->full_ready) {
        std::vector<int64_t> all(c->V);
        for (int i = 0; i < c->V; ++i) all[i] = i;
        int e = build_skin_set(c, all, &c->full);
        if (e) return e;
        c->full_ready = true;
    }
    const int V = c->V;
    DevBuf<float>* w = c->ws_f;
    HIP_TRY(w[4].ensure((size_t)B * 66));
    HIP_TRY(w[5].ensure((size_t)B * XDIM)); HIP_TRY(w[6].ensure((size_t)B * NPFX)); HIP_TRY(w[7].ensure((size_t)B * NJ * 12));
    HIP_TRY(w[8].ensure((size_t)B * NJ * 12)); HIP_TRY(w[9].ensure((size_t)B * 16)); HIP_TRY(w[10].ensure(1));
    float* X = w[5].p;
    hipLaunchKernelGGL(assemble_rows_kernel, dim3((B + 127) / 128), dim3(128), 0, st, go, bp, betas, lh, rh, transl, B, X, w[4].p);
    HIP_TRY(hipMemsetAsync(w[9].p, 0, (size_t)B * 16 * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(w[10].p, 0, sizeof(float), st));
    hipLaunchKernelGGL(pose_fwd_kernel<false>, dim3(B), dim3(64 * POSE_NW), 0, st, c->pose_model(), X, (float*)nullptr, w[9].p, w[10].p, 0,
                       (float*)nullptr, w[6].p, (float*)nullptr, w[7].p, w[8].p, (float*)nullptr, (float*)nullptr, (const float*)w[4].p,
                       (const float*)nullptr, (size_t)0);
    if (joints) hipLaunchKernelGGL(joints_out_kernel, dim3((B * NJ + 255) / 256), dim3(256), 0, st, w[7].p, X, XDIM, B, joints);
    if (vertices) {
        HIP_TRY(w[11].ensure((size_t)B * 3 * V));
        HIP_TRY(blend_forward(c->full, w[6].p, B, w[11].p, st));
        hipLaunchKernelGGL(skin_fwd_kernel, dim3((V + 255) / 256, B), dim3(256), 0, st, c->full.model(), V, X, XDIM, X_BETAS,
                           X_TRANSL, w[11].p, w[8].p, (const float*)nullptr, (const float*)nullptr, 0, 0, vertices);
    }
    return (int)hipGetLastError();
}

int fdcap_smplx_backward(fdcap_ctx* c, const float* go, const float* bp, const float* betas, const float* lh, const float* rh,
                         const float* transl, int32_t B, const float* g_vertices, const float* g_joints, float* g_go, float* g_bp,
                         float* g_betas, float* g_lh, float* g_rh, float* g_transl, void* stream) {
    if (!c || !go || !bp || !betas || !lh || !rh || !transl || B <= 0 || (!g_vertices && !g_joints)) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (g_vertices && !c->full_ready) {
        std::vector<int64_t> all(c->V);
        for (int i = 0; i < c->V; ++i) all[i] = i;
        int e = build_skin_set(c, all, &c->full);
        if (e) return e;
        c->full_ready = true;
    }
    const int V = c->V;
    const size_t nv3 = (size_t)3 * V;
    DevBuf<float>* w = c->ws_b;
    // forward state (recomputed: the operator keeps none): X rows, AA, PF, Rm, Jrest, G, A
    HIP_TRY(w[0].ensure((size_t)B * XDIM)); HIP_TRY(w[1].ensure((size_t)B * 66)); HIP_TRY(w[2].ensure((size_t)B * NPFX));
    HIP_TRY(w[3].ensure((size_t)B * NJ * 9)); HIP_TRY(w[4].ensure((size_t)B * NJ * 3)); HIP_TRY(w[5].ensure((size_t)B * NJ * 12));
    HIP_TRY(w[6].ensure((size_t)B * NJ * 12));
    // gradients: dA, [dtransl_v 3 | dMv 12 | dsv 1 | identity M 12 | cam 16] per row + scale, dPF, dX, dAA
    HIP_TRY(w[7].ensure((size_t)B * NJ * 12)); HIP_TRY(w[8].ensure((size_t)B * 44 + 4)); HIP_TRY(w[9].ensure((size_t)B * NPFX));
    HIP_TRY(w[10].ensure((size_t)B * XDIM)); HIP_TRY(w[11].ensure((size_t)B * 66));
    float* X = w[0].p; float* AA = w[1].p; float* PF = w[2].p;
    float* dtv = w[8].p; float* dMv = dtv + (size_t)B * 3; float* dsv = dMv + (size_t)B * 12; float* Mid = dsv + B;
    float* cam0 = Mid + (size_t)B * 12; float* one = cam0 + (size_t)B * 16;
    hipLaunchKernelGGL(assemble_rows_kernel, dim3((B + 127) / 128), dim3(128), 0, st, go, bp, betas, lh, rh, transl, B, X, AA);
    HIP_TRY(hipMemsetAsync(cam0, 0, ((size_t)B * 16 + 4) * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(w[10].p, 0, (size_t)B * XDIM * sizeof(float), st));
    hipLaunchKernelGGL(pose_fwd_kernel<false>, dim3(B), dim3(64 * POSE_NW), 0, st, c->pose_model(), X, (float*)nullptr, cam0, one /* = 0 here */, 0,
                       w[3].p, PF, w[4].p, w[5].p, w[6].p, (float*)nullptr, (float*)nullptr, (const float*)AA, (const float*)nullptr,
                       (size_t)0);
    const float* dA = nullptr; const float* dPF = nullptr; const float* dtr = nullptr;
    if (g_vertices) {
        // body-frame vertices = the world form with M = [I | 0] and scale = 1
        hipLaunchKernelGGL(identity_rows_kernel, dim3((B * 12 + 255) / 256), dim3(256), 0, st, Mid, B, one);
        DevBuf<float>* wf = c->ws_f;
        HIP_TRY(wf[11].ensure((size_t)B * nv3));                 // pose + shape blend offsets
        HIP_TRY(wf[0].ensure((size_t)B * nv3));                  // d offsets
        HIP_TRY(blend_forward(c->full, PF, B, wf[11].p, st));
        { int es = skin_bwd_any<false>(c->ws_skin, st, B, c->full.model(), V, X, wf[11].p, w[6].p, Mid, one, 0, g_vertices, wf[0].p, w[7].p,
                                       (float*)nullptr, dtv, dMv, dsv, ContactGradIn()); if (es) return es; }
        HIP_TRY(blend_backward(c->full, wf[0].p, B, w[9].p, 0, c->ws_kpart, st));
        dA = w[7].p; dPF = w[9].p; dtr = dtv;
    }
    hipLaunchKernelGGL(pose_bwd_op_kernel, dim3(B), dim3(64), 0, st, c->pose_model(), X, AA, w[3].p, w[4].p, w[5].p, dA, dPF, dtr,
                       g_joints, w[10].p, w[11].p);
    hipLaunchKernelGGL(smplx_bwd_split_kernel, dim3((B + 127) / 128), dim3(128), 0, st, w[10].p, w[11].p, B, g_go, g_bp, g_betas, g_lh,
                       g_rh, g_transl);
    return (int)hipGetLastError();
}

static int ensure_full_set(fdcap_ctx* c) {
    if (c->full_ready) return FDCAP_OK;
    std::vector<int64_t> all(c->V);
    for (int i = 0; i < c->V; ++i) all[i] = i;
    int e = build_skin_set(c, all, &c->full);
    if (e) return e;
    c->full_ready = true;
    return FDCAP_OK;
}

// ---- Op 2 with the fitted face (fdc_face_mesh.h) ---------------------------------------------------------------------------------------
// jaw_pose [B,3] and expression [B,10], each NULL on its own; both NULL: the entry point without `_face`, launch for launch.  The chain
// runs as it does there (jaw = 0, psi = 0); face_fwd_kernel corrects its transforms into ws_face[0] (and the PF row into ws_face[1]),
// expr_offsets_kernel completes the offsets, and the skinning kernels run on those.
// the full mesh's expression table, a coefficient's directions along a row, and JE: built at the first call that needs them (as
// ensure_full_set builds the full vertex set), so that a context that never asks for the face is created as before
static int ensure_face_tables(fdcap_ctx* c) {
    if (c->d_JEf.p) return FDCAP_OK;
    if (c->h_E10.empty()) return FDCAP_E_STATE;            // (a model without expression directions: num_shape < 20)
    const int V = c->V;
    c->lde_f = (3 * V + 3) & ~3;
    std::vector<float> ef((size_t)NEXPR * c->lde_f, 0.f);
    for (size_t i = 0; i < (size_t)V * 3; ++i)
        for (int l = 0; l < NEXPR; ++l) ef[(size_t)l * c->lde_f + i] = c->h_E10[i * NEXPR + l];
    HIP_TRY(c->d_Ef.upload(ef.data(), ef.size()));
    HIP_TRY(c->d_JEf.upload(c->h_JE.data(), c->h_JE.size()));
    return FDCAP_OK;
}
static int face_args_check(fdcap_ctx* c, const float* jaw, const float* expr) {
    if (expr) { int e = ensure_face_tables(c); if (e) return e; }
    if (jaw) for (int j = 0; j < NJ; ++j) if (c->h_parents[j] == JAW_J) return FDCAP_E_ARG;     // (the leaf argument needs a leaf)
    if (expr) for (int j = 1; j < NJ; ++j) if (c->h_parents[j] >= j) return FDCAP_E_ARG;        // (pose_forward's own condition)
    return FDCAP_OK;
}
// after the pose forward: A' (and PF'), the joints, then -- vertices -- the blend product, E psi and the skinning on A'
static int face_forward_tail(fdcap_ctx* c, int32_t B, const float* X, const float* PF, const float* G, const float* A, const float* jaw,
                             const float* expr, const float* Mw, const float* S, int world, float* Voff, float* vertices, float* joints,
                             hipStream_t st) {
    const int V = c->V;
    HIP_TRY(c->ws_face[0].ensure((size_t)B * NJ * 12));
    if (jaw) HIP_TRY(c->ws_face[1].ensure((size_t)B * NPFX));
    float* const A2 = c->ws_face[0].p;
    float* const PF2 = jaw && vertices ? c->ws_face[1].p : nullptr;
    hipLaunchKernelGGL(face_fwd_kernel, dim3(B), dim3(FACE_NT), 0, st, c->face_tabs(), A, PF, G, X, XDIM, X_BETAS, X_TRANSL, 0, expr, jaw, A2, PF2,
                       joints);
    if (vertices) {
        HIP_TRY(blend_forward(c->full, PF2 ? PF2 : PF, B, Voff, st));
        if (expr)
            hipLaunchKernelGGL(expr_offsets_kernel, dim3((3 * V + 255) / 256, (B + FACE_FS - 1) / FACE_FS), dim3(256), 0, st, c->d_Ef.p, c->lde_f,
                               3 * V, expr, B, Voff, (size_t)3 * V);
        hipLaunchKernelGGL(skin_fwd_kernel, dim3((V + 255) / 256, B), dim3(256), 0, st, c->full.model(), V, X, XDIM, X_BETAS, X_TRANSL, Voff, A2, Mw,
                           S, 0, world, vertices);
    }
    return (int)hipGetLastError();
}

static int body_forward_face_impl(fdcap_ctx* c, const float* params, int32_t B, const float* jaw, const float* expr, const float* cam_ext,
                                  const float* scale, float* vertices, float* joints, hipStream_t st) {
    { int e = face_args_check(c, jaw, expr); if (e) return e; }
    if (vertices) { int e = ensure_full_set(c); if (e) return e; }
    const int V = c->V;
    const bool world = cam_ext != nullptr && scale != nullptr;
    DevBuf<float>* w = c->ws_f;
    HIP_TRY(w[2].ensure((size_t)B * 512)); HIP_TRY(w[3].ensure((size_t)B * 512)); HIP_TRY(w[4].ensure((size_t)B * ODIM));
    HIP_TRY(w[5].ensure((size_t)B * XDIM)); HIP_TRY(w[6].ensure((size_t)B * NPFX)); HIP_TRY(w[7].ensure((size_t)B * NJ * 12));
    HIP_TRY(w[8].ensure((size_t)B * NJ * 12)); HIP_TRY(w[9].ensure((size_t)B * 16)); HIP_TRY(w[10].ensure(1));
    HIP_TRY(w[1].ensure((size_t)B * 12));
    if (vertices) HIP_TRY(w[11].ensure((size_t)B * 3 * V));
    float* X = w[5].p;
    hipLaunchKernelGGL(p75_to_78_kernel, dim3((B + 127) / 128), dim3(128), 0, st, params, B, X);
    HIP_TRY(c->ws_part.ensure((size_t)4 * B * ODIM));
    int e = vposer_forward(c, X, XDIM, X_LATENT, 0, B, w[2].p, w[3].p, c->ws_part.p, (size_t)B * ODIM, w[4].p, st);
    if (e) return e;
    if (!world) {
        HIP_TRY(hipMemsetAsync(w[9].p, 0, (size_t)B * 16 * sizeof(float), st));
        HIP_TRY(hipMemsetAsync(w[10].p, 0, sizeof(float), st));
    }
    const float* CAM = world ? cam_ext : w[9].p;
    const float* S = world ? scale : w[10].p;
    hipLaunchKernelGGL(pose_fwd_kernel<false>, dim3(B), dim3(64 * POSE_NW), 0, st, c->pose_model(), X, w[4].p, CAM, S, 0,
                       (float*)nullptr, w[6].p, (float*)nullptr, w[7].p, w[8].p, w[1].p, (float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (size_t)0);
    return face_forward_tail(c, B, X, w[6].p, w[7].p, w[8].p, jaw, expr, w[1].p, S, world ? 1 : 0, w[11].p, vertices, joints, st);
}

int fdcap_body_forward_face(fdcap_ctx* c, const float* params, int32_t B, const float* jaw_pose, const float* expression, float* vertices,
                            float* joints, void* stream) {
    if (!jaw_pose && !expression) return fdcap_body_forward(c, params, B, vertices, joints, stream);
    if (!c || !params || B <= 0 || (!vertices && !joints)) return FDCAP_E_ARG;
    return body_forward_face_impl(c, params, B, jaw_pose, expression, nullptr, nullptr, vertices, joints, (hipStream_t)stream);
}

int fdcap_world_mesh_face(fdcap_ctx* c, const float* params, int32_t B, const float* jaw_pose, const float* expression, const float* cam_ext,
                          const float* scale, float* vertices, void* stream) {
    if (!jaw_pose && !expression) return fdcap_world_mesh(c, params, B, cam_ext, scale, vertices, stream);
    if (!c || !params || B <= 0 || !cam_ext || !scale || !vertices) return FDCAP_E_ARG;
    return body_forward_face_impl(c, params, B, jaw_pose, expression, cam_ext, scale, vertices, nullptr, (hipStream_t)stream);
}

int fdcap_smplx_forward_face(fdcap_ctx* c, const float* go, const float* bp, const float* betas, const float* lh, const float* rh,
                             const float* transl, int32_t B, const float* jaw_pose, const float* expression, float* vertices, float* joints,
                             void* stream) {
    if (!jaw_pose && !expression) return fdcap_smplx_forward(c, go, bp, betas, lh, rh, transl, B, vertices, joints, stream);
    if (!c || !go || !bp || !betas || !lh || !rh || !transl || B <= 0 || (!vertices && !joints)) return FDCAP_E_ARG;
    { int e = face_args_check(c, jaw_pose, expression); if (e) return e; }
    hipStream_t st = (hipStream_t)stream;
    if (vertices) { int e = ensure_full_set(c); if (e) return e; }
    const int V = c->V;
    DevBuf<float>* w = c->ws_f;
    HIP_TRY(w[4].ensure((size_t)B * 66));
    HIP_TRY(w[5].ensure((size_t)B * XDIM)); HIP_TRY(w[6].ensure((size_t)B * NPFX)); HIP_TRY(w[7].ensure((size_t)B * NJ * 12));
    HIP_TRY(w[8].ensure((size_t)B * NJ * 12)); HIP_TRY(w[9].ensure((size_t)B * 16)); HIP_TRY(w[10].ensure(1));
    if (vertices) HIP_TRY(w[11].ensure((size_t)B * 3 * V));
    float* X = w[5].p;
    hipLaunchKernelGGL(assemble_rows_kernel, dim3((B + 127) / 128), dim3(128), 0, st, go, bp, betas, lh, rh, transl, B, X, w[4].p);
    HIP_TRY(hipMemsetAsync(w[9].p, 0, (size_t)B * 16 * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(w[10].p, 0, sizeof(float), st));
    hipLaunchKernelGGL(pose_fwd_kernel<false>, dim3(B), dim3(64 * POSE_NW), 0, st, c->pose_model(), X, (float*)nullptr, w[9].p, w[10].p, 0,
                       (float*)nullptr, w[6].p, (float*)nullptr, w[7].p, w[8].p, (float*)nullptr, (float*)nullptr, (const float*)w[4].p,
                       (const float*)nullptr, (size_t)0);
    return face_forward_tail(c, B, X, w[6].p, w[7].p, w[8].p, jaw_pose, expression, nullptr, nullptr, 0, w[11].p, vertices, joints, st);
}

// g_jaw_pose [B,3] / g_expression [B,10]: may be NULL each (the input is then a constant of the call); an input that is NULL has no
// gradient: its output must be NULL too.  Two calls give the same bits: every sum in a fixed order.
int fdcap_smplx_backward_face(fdcap_ctx* c, const float* go, const float* bp, const float* betas, const float* lh, const float* rh,
                              const float* transl, int32_t B, const float* jaw_pose, const float* expression, const float* g_vertices,
                              const float* g_joints, float* g_go, float* g_bp, float* g_betas, float* g_lh, float* g_rh, float* g_transl,
                              float* g_jaw_pose, float* g_expression, void* stream) {
    if ((g_jaw_pose && !jaw_pose) || (g_expression && !expression)) return FDCAP_E_ARG;
    if (!jaw_pose && !expression)
        return fdcap_smplx_backward(c, go, bp, betas, lh, rh, transl, B, g_vertices, g_joints, g_go, g_bp, g_betas, g_lh, g_rh, g_transl, stream);
    if (!c || !go || !bp || !betas || !lh || !rh || !transl || B <= 0 || (!g_vertices && !g_joints)) return FDCAP_E_ARG;
    { int e = face_args_check(c, jaw_pose, expression); if (e) return e; }
    hipStream_t st = (hipStream_t)stream;
    if (g_vertices) { int e = ensure_full_set(c); if (e) return e; }
    const int V = c->V;
    const size_t nv3 = (size_t)3 * V;
    const int nch = face_nchunk(3 * V);
    DevBuf<float>* w = c->ws_b;
    // forward state (recomputed: the operator keeps none): X rows, AA, PF, Rm, Jrest, G, A; then A' and PF'
    HIP_TRY(w[0].ensure((size_t)B * XDIM)); HIP_TRY(w[1].ensure((size_t)B * 66)); HIP_TRY(w[2].ensure((size_t)B * NPFX));
    HIP_TRY(w[3].ensure((size_t)B * NJ * 9)); HIP_TRY(w[4].ensure((size_t)B * NJ * 3)); HIP_TRY(w[5].ensure((size_t)B * NJ * 12));
    HIP_TRY(w[6].ensure((size_t)B * NJ * 12));
    HIP_TRY(w[7].ensure((size_t)B * NJ * 12)); HIP_TRY(w[8].ensure((size_t)B * 44 + 4)); HIP_TRY(w[9].ensure((size_t)B * NPFX));
    HIP_TRY(w[10].ensure((size_t)B * XDIM)); HIP_TRY(w[11].ensure((size_t)B * 66));
    HIP_TRY(c->ws_face[0].ensure((size_t)B * NJ * 12)); HIP_TRY(c->ws_face[1].ensure((size_t)B * NPFX));
    HIP_TRY(c->ws_face[2].ensure((size_t)B * nch * NEXPR)); HIP_TRY(c->ws_face[3].ensure((size_t)B * 9));
    float* X = w[0].p; float* AA = w[1].p; float* PF = w[2].p;
    float* dtv = w[8].p; float* dMv = dtv + (size_t)B * 3; float* dsv = dMv + (size_t)B * 12; float* Mid = dsv + B;
    float* cam0 = Mid + (size_t)B * 12; float* one = cam0 + (size_t)B * 16;
    float* const A2 = c->ws_face[0].p;
    float* const PF2 = jaw_pose && g_vertices ? c->ws_face[1].p : nullptr;
    float* const R9 = c->ws_face[3].p;
    hipLaunchKernelGGL(assemble_rows_kernel, dim3((B + 127) / 128), dim3(128), 0, st, go, bp, betas, lh, rh, transl, B, X, AA);
    HIP_TRY(hipMemsetAsync(cam0, 0, ((size_t)B * 16 + 4) * sizeof(float), st));
    HIP_TRY(hipMemsetAsync(w[10].p, 0, (size_t)B * XDIM * sizeof(float), st));
    hipLaunchKernelGGL(pose_fwd_kernel<false>, dim3(B), dim3(64 * POSE_NW), 0, st, c->pose_model(), X, (float*)nullptr, cam0, one /* = 0 here */, 0,
                       w[3].p, PF, w[4].p, w[5].p, w[6].p, (float*)nullptr, (float*)nullptr, (const float*)AA, (const float*)nullptr,
                       (size_t)0);
    hipLaunchKernelGGL(face_fwd_kernel, dim3(B), dim3(FACE_NT), 0, st, c->face_tabs(), (const float*)w[6].p, (const float*)PF, (const float*)nullptr,
                       (const float*)X, XDIM, X_BETAS, X_TRANSL, 0, expression, jaw_pose, A2, PF2, (float*)nullptr);
    const float* dPF = nullptr; const float* dtr = nullptr; const float* part = nullptr;
    if (g_vertices) {
        hipLaunchKernelGGL(identity_rows_kernel, dim3((B * 12 + 255) / 256), dim3(256), 0, st, Mid, B, one);
        DevBuf<float>* wf = c->ws_f;
        HIP_TRY(wf[11].ensure((size_t)B * nv3));                 // pose + shape + expression offsets
        HIP_TRY(wf[0].ensure((size_t)B * nv3));                  // d offsets
        HIP_TRY(blend_forward(c->full, PF2 ? PF2 : PF, B, wf[11].p, st));
        if (expression)
            hipLaunchKernelGGL(expr_offsets_kernel, dim3((3 * V + 255) / 256, (B + FACE_FS - 1) / FACE_FS), dim3(256), 0, st, c->d_Ef.p, c->lde_f,
                               3 * V, expression, B, wf[11].p, nv3);
        { int es = skin_bwd_any<false>(c->ws_skin, st, B, c->full.model(), V, X, wf[11].p, A2, Mid, one, 0, g_vertices, wf[0].p, w[7].p,
                                       (float*)nullptr, dtv, dMv, dsv, ContactGradIn()); if (es) return es; }
        HIP_TRY(blend_backward(c->full, wf[0].p, B, w[9].p, 0, c->ws_kpart, st));
        if (g_expression) {
            hipLaunchKernelGGL(expr_dpsi_kernel, dim3(nch, (B + FACE_FS - 1) / FACE_FS), dim3(256), 0, st, c->d_Ef.p, c->lde_f, 3 * V,
                               (const float*)wf[0].p, nv3, B, c->ws_face[2].p, nch);
            part = c->ws_face[2].p;
        }
        dPF = w[9].p; dtr = dtv;
    }
    // d loss / d A' -> d loss / d A in place (w[7]; without vertices the kernel takes d loss / d A' as zero and assigns every row)
    hipLaunchKernelGGL(face_bwd_kernel, dim3(B), dim3(FACE_NT), 0, st, c->face_tabs(), (const float*)w[6].p, g_vertices ? (const float*)w[7].p : nullptr,
                       (const float*)X, XDIM, X_BETAS, 0, expression, jaw_pose, g_joints, part, nch, w[7].p, g_expression, R9, w[10].p, 0);
    if (g_jaw_pose) {                                        // the fit's own consumer of the jaw's two parts (fdc_fit2d.h), without a prior
        JawGradIn jg;
        jg.jaw = const_cast<float*>(jaw_pose); jg.R9 = R9; jg.gP = dPF ? dPF + 9 * (JAW_J - 1) : nullptr; jg.gp_stride = NPFX;
        hipLaunchKernelGGL(jaw_grad_kernel, dim3((B + 63) / 64), dim3(64), 0, st, jg, B, g_jaw_pose, (float*)nullptr, (float*)nullptr, AdamScalars());
    }
    hipLaunchKernelGGL(pose_bwd_op_kernel, dim3(B), dim3(64), 0, st, c->pose_model(), X, AA, w[3].p, w[4].p, w[5].p, (const float*)w[7].p, dPF, dtr,
                       g_joints, w[10].p, w[11].p);
    hipLaunchKernelGGL(smplx_bwd_split_kernel, dim3((B + 127) / 128), dim3(128), 0, st, w[10].p, w[11].p, B, g_go, g_bp, g_betas, g_lh,
                       g_rh, g_transl);
    return (int)hipGetLastError();
}

// ---- Op 4: self-interpenetration (fdc_collide.h) -------------------------------------------------------------------------------------

int fdcap_set_collision_mesh(fdcap_ctx* c, int32_t n_faces, const int32_t* faces, const uint8_t* face_part, const uint64_t* ignore) {
    if (!c || n_faces < 0) return FDCAP_E_ARG;
    if (c->opt) return FDCAP_E_STATE;                  // (see fdcap_set_scene)
    if (n_faces == 0) { c->coll.h = CollTables(); return FDCAP_OK; }
    // FDCAP_COLL_LEAF=64: leaves of 64 faces instead of 32 (read at every registration; a mesh too large for 32 takes 64 anyway)
    const char* lf = getenv("FDCAP_COLL_LEAF");
    CollTables t;
    if (coll_mesh_build(n_faces, faces, face_part, ignore, c->V, c->h_vt.data(), lf && !strcmp(lf, "64") ? 64 : 32, &t)) return FDCAP_E_ARG;
    c->coll.h = CollTables();                          // (no mesh until the new tables are on the device)
    HIP_TRY(c->coll.tri.upload(t.tri.data(), t.tri.size()));
    HIP_TRY(c->coll.order.upload(t.order.data(), t.order.size()));
    HIP_TRY(c->coll.ign.upload(t.ign.data(), t.ign.size()));
    int e = ensure_full_set(c);                        // what the inner fit's full-mesh pass skins with
    if (e) return e;
    c->coll.h = std::move(t);
    return FDCAP_OK;
}

// test / diagnosis: the registered mesh's tree: info4 = {F, leaf, NL, NLp}; order_out (may be NULL) [NL * leaf] tree position -> face id, -1 padding
int fdcap_debug_collision_tree(fdcap_ctx* c, int32_t* info4, int32_t* order_out) {
    if (!c || !info4) return FDCAP_E_ARG;
    const CollTables& t = c->coll.h;
    if (t.F <= 0) return FDCAP_E_STATE;
    info4[0] = t.F; info4[1] = t.leaf; info4[2] = t.NL; info4[3] = t.NLp;
    if (order_out) memcpy(order_out, t.order.data(), t.order.size() * sizeof(int32_t));
    return FDCAP_OK;
}

// test / diagnosis: coll_refit_kernel alone on verts [n,V,3] -> nodes_out (device) [n][2 NLp][6] {lo, hi}; node 0 is whatever the
// workspace held (the kernel never writes it)
int fdcap_debug_collision_nodes(fdcap_ctx* c, const float* verts, int32_t n, float* nodes_out, void* stream) {
    if (!c || !verts || !nodes_out || n <= 0) return FDCAP_E_ARG;
    fdcap_ctx::CollisionSet& cs = c->coll;
    if (cs.h.F <= 0) return FDCAP_E_STATE;
    const CollMesh m = cs.view();
    const size_t words = (size_t)n * 2 * m.NLp * 6;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(cs.nodes.ensure(words));
    const size_t lds = (size_t)2 * m.NLp * 6 * sizeof(float);
    if (m.leaf == 64) hipLaunchKernelGGL(coll_refit_kernel<64>, dim3(n), dim3(256), lds, st, m, verts, c->V, cs.nodes.p);
    else hipLaunchKernelGGL(coll_refit_kernel<32>, dim3(n), dim3(256), lds, st, m, verts, c->V, cs.nodes.p);
    HIP_TRY(hipMemcpyAsync(nodes_out, cs.nodes.p, words * sizeof(float), hipMemcpyDeviceToDevice, st));
    return (int)hipGetLastError();
}

int fdcap_collision_eval(fdcap_ctx* c, const float* verts, int32_t n, const fdcap_collision_params* p, int32_t* pairs, int32_t* count,
                         float* loss, float* dverts, void* stream) {
    if (!c || !verts || !p || !count || !loss || n <= 0) return FDCAP_E_ARG;
    if (!coll_params_ok(p->sigma, p->w_coll, p->capacity)) return FDCAP_E_ARG;
    fdcap_ctx::CollisionSet& cs = c->coll;
    if (cs.h.F <= 0) return FDCAP_E_STATE;
    const CollMesh m = cs.view();
    const int V = c->V, cap = p->capacity, npos = m.NL * m.leaf;
    const long long slots = (long long)n * cap, total = 6 * slots;
    // the grouping's keys are frame x V + vertex in 32 bits, its positions ints
    if (total > CB_MAX_SORT || (long long)n * V >= 0xffffffffLL || (long long)n * npos > 0x7fffffffLL) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(cs.cnt.ensure((size_t)n * npos)); HIP_TRY(cs.list.ensure(2 * (size_t)slots)); HIP_TRY(cs.val.ensure((size_t)slots));
    int2* const list = (int2*)cs.list.p;
    if (p->every_pair) {
        const dim3 g((npos + 255) / 256, n);
        hipLaunchKernelGGL(coll_every_kernel<false>, g, dim3(256), 0, st, m, verts, V, cs.cnt.p, cap, list);
        hipLaunchKernelGGL(coll_prefix_kernel, dim3(n), dim3(256), 0, st, cs.cnt.p, npos, count);
        hipLaunchKernelGGL(coll_every_kernel<true>, g, dim3(256), 0, st, m, verts, V, cs.cnt.p, cap, list);
    } else {
        HIP_TRY(cs.nodes.ensure((size_t)n * 2 * m.NLp * 6));
        const size_t lds = (size_t)2 * m.NLp * 6 * sizeof(float);
        const dim3 g((m.NL + 3) / 4, n);
        if (m.leaf == 64) {
            hipLaunchKernelGGL(coll_refit_kernel<64>, dim3(n), dim3(256), lds, st, m, verts, V, cs.nodes.p);
            hipLaunchKernelGGL((coll_search_kernel<64, false>), g, dim3(256), 0, st, m, verts, V, cs.nodes.p, cs.cnt.p, cap, list);
            hipLaunchKernelGGL(coll_prefix_kernel, dim3(n), dim3(256), 0, st, cs.cnt.p, npos, count);
            hipLaunchKernelGGL((coll_search_kernel<64, true>), g, dim3(256), 0, st, m, verts, V, cs.nodes.p, cs.cnt.p, cap, list);
        } else {
            hipLaunchKernelGGL(coll_refit_kernel<32>, dim3(n), dim3(256), lds, st, m, verts, V, cs.nodes.p);
            hipLaunchKernelGGL((coll_search_kernel<32, false>), g, dim3(256), 0, st, m, verts, V, cs.nodes.p, cs.cnt.p, cap, list);
            hipLaunchKernelGGL(coll_prefix_kernel, dim3(n), dim3(256), 0, st, cs.cnt.p, npos, count);
            hipLaunchKernelGGL((coll_search_kernel<32, true>), g, dim3(256), 0, st, m, verts, V, cs.nodes.p, cs.cnt.p, cap, list);
        }
    }
    if (dverts) { HIP_TRY(cs.grad.ensure(18 * (size_t)slots)); HIP_TRY(cs.dest.ensure((size_t)total)); }
    hipLaunchKernelGGL(coll_penalty_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, m, verts, V, n, (const int*)count, cap,
                       (const int2*)list, p->sigma, p->w_coll, cs.val.p, dverts ? cs.grad.p : nullptr, dverts ? cs.dest.p : nullptr, pairs);
    hipLaunchKernelGGL(coll_frame_sum_kernel, dim3((n + 63) / 64), dim3(64), 0, st, cs.val.p, (const int*)count, n, cap, p->w_coll, loss);
    if (dverts) {
        HIP_TRY(cs.key.ensure(cb_key_words(total))); HIP_TRY(cs.sval.ensure(2 * (size_t)total));
        int buf = 0;
        HIP_TRY(cb_group(cs.dest.p, n, 6 * cap, V, true, cs.key.p, cs.sval.p, cs.key.p + 2 * (size_t)total, st, &buf));
        const long long nd = (long long)n * V;
        hipLaunchKernelGGL(coll_gather_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, cs.key.p + (size_t)buf * total,
                           cs.sval.p + (size_t)buf * total, (int)total, cs.grad.p, nd, dverts);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
