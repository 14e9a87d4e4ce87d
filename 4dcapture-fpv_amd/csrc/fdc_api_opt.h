// C-ABI, part 2: the clip optimiser -- create / inputs / the iteration (forward, losses, backward), fdcap_opt_backward[_and_step].
// Part of csrc/fdcap.hip.
#pragma once

extern "C" {

// ---- optimiser -------------------------------------------------------------------------------
void fdcap_opt_destroy(fdcap_ctx* c) {
    if (!c || !c->opt) return;
    OptState* o = c->opt;
    if (o->lbfgs) fdcap_lbfgs_destroy(o->lbfgs);           // (an incomplete type where OptState is defined: not a member it can own)
    delete o;
    c->opt = nullptr;
}

static_assert(LROW == FDCAP_NUM_LOSSES, "a batch's per-clip loss slots are LROW apart on the device");
static_assert(CLIP_XDIM == XDIM && CLIP_NJW == NJW, "fdc_clips.h restates the two dimensions its weights divide by");
static_assert(POSE_NJ == NJ && POSE_NJW == NJW, "fdc_forms.h restates the two joint counts plan_pose_joints works with");

// the loss total of iteration ii of mode 'global' (:570 / :582): phase 1 below first_phase2_iter, phase 2 from it
static LossWeights opt_phase_weights(const fdcap_opt_config& cf, bool phase2) {
    LossWeights lw;
    lw.rec = 1.f;
    lw.smooth = phase2 ? cf.phase2_smooth : cf.phase1_smooth;
    lw.contact = phase2 ? 0.f : cf.phase1_contact;
    lw.world = phase2 ? cf.phase2_world : 0.f;
    lw.dct = 0.f;
    lw.world_on = phase2;
    return lw;
}

// var_len == nullptr: n_clips clips of cfg->n_total frames each (one clip, one rank's share of one, or a batch of one length).
// var_len != nullptr: clips of these lengths, not all equal; cfg holds the batch's rows (n_total = n_local = their sum, checked
// by the caller).
// scene_slot: the registered scene the optimiser searches.  segments (fdcap_opt_create_clips_scenes; two or more, fdc_clips.h):
// each run of clips searches its own slot's scene -- the search state is built per segment (OptState::segs) -- and scene_slot is
// ignored; everything else is the batch it would be on one scene.
static int opt_create_impl(fdcap_ctx* c, const fdcap_opt_config* cfg, int32_t n_clips, const int32_t* var_len, float* rows_x, float* rows_cam,
                           float* scale_d, float* dscale_d, double* losses_d, int32_t scene_slot = 0,
                           const std::vector<ClipSegment>* segments = nullptr) {
    SetupTrace tr("fdcap_opt_create");
    // (every named slot holds a scene: a batch has one contact switch, and a clip without a scene would have no contact term)
    if (segments) for (const ClipSegment& g : *segments) if (c->scenes[g.slot].ns <= 0) return FDCAP_E_STATE;
    if (segments) scene_slot = (*segments)[0].slot;
    const SceneSet& sc0 = c->scenes[scene_slot];
    // a second clip of the same shape reuses the scratch allocations (every buffer is re-zeroed below)
    OptState* o = c->opt ? c->opt : new OptState();
    c->opt = o;
    o->cfg = *cfg;
    o->nclip = n_clips;
    o->clip_len = var_len ? 0 : cfg->n_total;
    o->ragged = var_len != nullptr;
    if (var_len) o->clip_lens.assign(var_len, var_len + n_clips);
    else o->clip_lens.assign((size_t)n_clips, cfg->n_total);
    o->clip_start = clip_starts(n_clips, o->clip_lens.data());
    if (n_clips > 1 && !var_len) o->cfg.n_total = o->cfg.n_local = n_clips * cfg->n_total;     // the batch's rows: clip k owns 2 + k N .. 2 + (k + 1) N
    cfg = &o->cfg;
    o->cam_steps = 0;
    o->dz_pending = false;
    o->log_pending = false;
    o->kp_mapped = false;
    o->reproj = fdcap_reproj_params{};                      // (the reprojection term is an input of a fit, handed over after every create)
    o->cam_ready = false;
    o->seeded = false;
    o->nnpt_valid = false;
    o->n_recompute = 0;
    o->skb_valid = false;
    o->dctT = o->dctC = o->dctW = 0;
    o->dct_clips = false;
    o->dct_grad = false;
    const int R = o->R = cfg->n_local + 4;
    o->scene_slot = scene_slot;
    o->nnpt_filled = false;
    o->segs.clear();
    o->contact_on = sc0.ns > 0 && c->nc > 0 && cfg->weight_contact != 0.f;
    const size_t nq = (size_t)R * std::max(c->nc, 1);
    o->sw = forms_read_env();                               // (every create: tests flip the per-fit switches between fits in one process)
    const int nq_all = (int)((size_t)cfg->n_local * c->nc);
    o->nsplit = o->contact_on ? nn_pick_nsplit(nq_all, (int)sc0.ns, o->sw.nn_seed && o->sw.nn_cull) : 1;
    o->nsplit_bf = o->contact_on ? nn_pick_nsplit(nq_all, (int)sc0.ns, false) : 1;
    size_t pd_floats = (size_t)std::max(o->nsplit, o->nsplit_bf) * nq;
    if (segments) {                                         // every segment splits its own scene for its own queries; one workspace serves them in turn
        o->segs.resize(segments->size());
        pd_floats = 0;
        for (size_t s = 0; s < segments->size(); ++s) {
            SegSearch& g = o->segs[s];
            g.seg = (*segments)[s];
            g.nsplit = nn_pick_nsplit(g.seg.nq, (int)c->scenes[g.seg.slot].ns, o->sw.nn_seed && o->sw.nn_cull);
            pd_floats = std::max(pd_floats, (size_t)g.nsplit * g.seg.nq);
        }
        o->nsplit = o->nsplit_bf = 1;
    }
    int err = 0;
#define AL(buf, cnt) if (!err) { hipError_t e_ = (buf).ensure(cnt); if (e_ != hipSuccess) err = (int)e_; else e_ = hipMemset((buf).p, 0, (size_t)(cnt) * sizeof(*(buf).p)); }
    o->X.p = rows_x; o->CAM.p = rows_cam; o->scale.p = scale_d; o->dscale.p = dscale_d; o->losses.p = losses_d;
    o->pend.on = false;
    AL(o->X0, (size_t)R * XDIM) AL(o->mask, R)
    AL(o->mX, (size_t)R * XDIM) AL(o->vX, (size_t)R * XDIM) AL(o->mCAM, (size_t)R * 16) AL(o->vCAM, (size_t)R * 16)
    AL(o->mS, n_clips) AL(o->vS, n_clips)
    AL(o->H1, (size_t)R * 512) AL(o->H2, (size_t)R * 512) AL(o->O, (size_t)R * O_LD) AL(o->dO, (size_t)R * ODIM)
    AL(o->Opart, (size_t)4 * R * ODIM) AL(o->dZpart, (size_t)4 * R * VP_Z)
    AL(o->Rm, (size_t)R * RM_LD) AL(o->PF, (size_t)R * NPFX) AL(o->Jrest, (size_t)R * JR_LD) AL(o->G, (size_t)R * NJ * 12)
    AL(o->A, (size_t)R * NJ * 12) AL(o->M, (size_t)R * 12) AL(o->Jw, (size_t)R * NJW * 3)
    AL(o->dA, (size_t)R * NJ * 12) AL(o->dtransl_v, (size_t)R * 3) AL(o->dMv, (size_t)R * 12)
    AL(o->dsv, R) AL(o->dPF, (size_t)2 * R * NPFX)   /* [2][R, 496]: the second half only as the K-split product's second partial */
    AL(o->dJw, (size_t)R * NJW * 3) AL(o->dX, (size_t)R * XDIM)
    AL(o->dCAM, (size_t)R * 16) AL(o->dscale_row, R) AL(o->loss_rows, (size_t)R * LROW)
    if (o->contact_on) {
        AL(o->Voff, nq * 3) AL(o->Vw, nq * 3) AL(o->dist, nq) AL(o->idx, nq) AL(o->dVoff, nq * 3) AL(o->seedpt, nq)
        AL(o->pd, pd_floats) AL(o->pi, pd_floats)
    }
#undef AL
    tr.mark("buffers");
    if (!err && o->contact_on) {
        hipError_t e_ = hipMemset(o->idx.p, 0xFF, nq * sizeof(int));      // -1: no seed yet
        if (e_ != hipSuccess) err = (int)e_;
    }
    for (SegSearch& g : o->segs) {                         // clips of several scenes: the same state, one set per segment
        if (err || !o->contact_on) break;
        o->nn_order = NNOrder{};                            // (the one-scene state: unused here)
        const int every = o->sw.nn_order;
        g.ord = NNOrder{};
        g.seeded = false;
        if (o->sw.nn_cache_slack > 0.f) {
            const size_t ng = (size_t)g.seg.groups, ng4 = ng * 4, snq = (size_t)g.seg.nq;
            hipError_t e_ = g.ids.ensure(ng4 * NN_CACHE_CAP);
            if (e_ == hipSuccess) e_ = g.hdr.ensure(ng4 + 3 * ng);
            if (e_ == hipSuccess) e_ = g.anchor.ensure(4 * snq);
            if (e_ == hipSuccess && every > 0) e_ = g.qbuf.ensure(nn_query_order_ints((int)snq));
            if (e_ == hipSuccess) e_ = hipMemset(g.hdr.p, 0xFF, ng4 * sizeof(int));
            if (e_ == hipSuccess) e_ = hipMemset(g.hdr.p + ng4, 0, 3 * ng * sizeof(int));
            if (e_ == hipSuccess) e_ = hipMemset(g.anchor.p, 0, 4 * snq * sizeof(float4));
            if (e_ != hipSuccess) err = (int)e_;
            if (every > 0) { g.ord.on = true; g.ord.every = every; g.ord.qbuf = g.qbuf.p; }
        }
    }
    if (!err && o->contact_on && o->segs.empty()) {
        const int every = o->sw.nn_order;
        o->nn_order = NNOrder{};
        if (o->sw.nn_cache_slack > 0.f) {                                        // groups of 32 queries x up to 4 waves per group
            const size_t ng = ((size_t)nq_all + 31) / 32, ng4 = ng * 4;
            hipError_t e_ = o->nnc_ids.ensure(ng4 * NN_CACHE_CAP);
            if (e_ == hipSuccess) e_ = o->nnc_hdr.ensure(ng4 + 3 * ng);                                        // + work counts [ng] + two launch-order tables [ng]
            if (e_ == hipSuccess) e_ = o->nnc_anchor.ensure((size_t)4 * nq_all);
            if (e_ == hipSuccess && every > 0) e_ = o->nnq_buf.ensure(nn_query_order_ints(nq_all));
            if (e_ == hipSuccess) e_ = hipMemset(o->nnc_hdr.p, 0xFF, ng4 * sizeof(int));                       // -1: nothing kept
            if (e_ == hipSuccess) e_ = hipMemset(o->nnc_hdr.p + ng4, 0, 3 * ng * sizeof(int));
            if (e_ == hipSuccess) e_ = hipMemset(o->nnc_anchor.p, 0, (size_t)4 * nq_all * sizeof(float4));
            if (e_ != hipSuccess) err = (int)e_;
            if (every > 0) { o->nn_order.on = true; o->nn_order.every = every; o->nn_order.qbuf = o->nnq_buf.p; }
        }
    }
    if (!err) {
        const std::vector<float> s((size_t)n_clips, cfg->scale_init);
        hipError_t e_ = hipMemcpy(o->scale.p, s.data(), s.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e_ != hipSuccess) err = (int)e_;
    }
    if (!err && o->ragged) {
        // the clip tables (fdc_clips.h): every row's record under the weights of phase 1, then of phase 2, then of mode 'local''s
        // second loop, and the clips' spans
        std::vector<ClipRow> rows = clip_rows_build(n_clips, var_len, opt_phase_weights(*cfg, false), cfg->weight_loss_rec, cfg->weight_contact, c->nc);
        const std::vector<ClipRow> rows2 = clip_rows_build(n_clips, var_len, opt_phase_weights(*cfg, true), cfg->weight_loss_rec, cfg->weight_contact, c->nc);
        const std::vector<ClipRow> rows3 = clip_rows_build_local2(n_clips, var_len, cfg->weight_loss_rec, (size_t)3 * c->V);
        rows.insert(rows.end(), rows2.begin(), rows2.end());
        rows.insert(rows.end(), rows3.begin(), rows3.end());
        std::vector<int> span((size_t)2 * n_clips);
        for (int k = 0; k < n_clips; ++k) { span[(size_t)2 * k] = o->clip_start[(size_t)k]; span[(size_t)2 * k + 1] = var_len[k]; }
        hipError_t e_ = rows.size() == (size_t)3 * R ? o->clip_rows.upload(rows.data(), rows.size()) : hipErrorInvalidValue;
        if (e_ == hipSuccess) e_ = o->clip_span.upload(span.data(), span.size());
        if (e_ != hipSuccess) err = (int)e_;
    }
    tr.mark("search state");
    if (err) { fdcap_opt_destroy(c); return err; }
    return FDCAP_OK;
}

int fdcap_opt_create_clips(fdcap_ctx* c, const fdcap_opt_config* cfg, int32_t n_clips, float* rows_x, float* rows_cam, float* scale_d,
                           float* dscale_d, double* losses_d) {
    if (!c || !cfg || !rows_x || !rows_cam || !scale_d || !dscale_d || !losses_d || cfg->n_local <= 0 || cfg->n_total < cfg->n_local || cfg->frame0 < 0 ||
        cfg->frame0 + cfg->n_local > cfg->n_total || n_clips < 1)
        return FDCAP_E_ARG;
    // a batch holds whole clips of one length: no shard of a clip, and K N rows that still index as int
    if (n_clips > 1 && (cfg->frame0 != 0 || cfg->n_local != cfg->n_total || (int64_t)n_clips * cfg->n_total > (1 << 24)))
        return FDCAP_E_ARG;
    return opt_create_impl(c, cfg, n_clips, nullptr, rows_x, rows_cam, scale_d, dscale_d, losses_d);
}

// Clips of their own lengths.  Equal lengths are fdcap_opt_create_clips' batch (its path, its bits: no table).
int fdcap_opt_create_clips_var(fdcap_ctx* c, const fdcap_opt_config* cfg, int32_t n_clips, const int32_t* clip_len, float* rows_x, float* rows_cam,
                               float* scale_d, float* dscale_d, double* losses_d) {
    if (!c || !cfg || !rows_x || !rows_cam || !scale_d || !dscale_d || !losses_d || cfg->frame0 != 0 || cfg->n_local != cfg->n_total ||
        !clip_lengths_ok(n_clips, clip_len, cfg->n_total, (int64_t)1 << 24))
        return FDCAP_E_ARG;
    if (clip_lengths_equal(n_clips, clip_len)) {
        fdcap_opt_config one = *cfg;
        one.n_total = one.n_local = clip_len[0];
        return fdcap_opt_create_clips(c, &one, n_clips, rows_x, rows_cam, scale_d, dscale_d, losses_d);
    }
    return opt_create_impl(c, cfg, n_clips, clip_len, rows_x, rows_cam, scale_d, dscale_d, losses_d);
}

// Clips that name their scene slot.  One slot for all: fdcap_opt_create_clips_var's optimiser on that slot's scene (its path, its
// bits).  Several: the search state per segment (fdc_clips.h), everything else that batch.
int fdcap_opt_create_clips_scenes(fdcap_ctx* c, const fdcap_opt_config* cfg, int32_t n_clips, const int32_t* clip_len, const int32_t* clip_scene,
                                  float* rows_x, float* rows_cam, float* scale_d, float* dscale_d, double* losses_d) {
    if (!c || !cfg || !rows_x || !rows_cam || !scale_d || !dscale_d || !losses_d || cfg->frame0 != 0 || cfg->n_local != cfg->n_total ||
        !clip_lengths_ok(n_clips, clip_len, cfg->n_total, (int64_t)1 << 24) || !clip_scenes_ok(n_clips, clip_scene, FDCAP_MAX_SCENES))
        return FDCAP_E_ARG;
    const std::vector<ClipSegment> segments = clip_segments(n_clips, clip_len, clip_scene, c->nc, FDCAP_MAX_SCENES);
    const bool equal = clip_lengths_equal(n_clips, clip_len);
    fdcap_opt_config one = *cfg;
    if (equal) one.n_total = one.n_local = clip_len[0];         // (one length: fdcap_opt_create_clips' batch, no table)
    if (equal && n_clips > 1 && (int64_t)n_clips * clip_len[0] > (1 << 24)) return FDCAP_E_ARG;
    return opt_create_impl(c, &one, n_clips, equal ? nullptr : clip_len, rows_x, rows_cam, scale_d, dscale_d, losses_d, segments[0].slot,
                           segments.size() > 1 ? &segments : nullptr);
}

int fdcap_opt_create(fdcap_ctx* c, const fdcap_opt_config* cfg, float* rows_x, float* rows_cam, float* scale_d,
                     float* dscale_d, double* losses_d) {
    return fdcap_opt_create_clips(c, cfg, 1, rows_x, rows_cam, scale_d, dscale_d, losses_d);
}

int fdcap_opt_set_inputs(fdcap_ctx* c, const float* data78, const float* init78, const float* mask, const float* cam,
                         void* stream) {
    if (!c || !c->opt || !data78 || !init78 || !mask || !cam) return FDCAP_E_ARG;
    { int es_ = opt_sync(c, (hipStream_t)stream); if (es_) return es_; }
    OptState* o = c->opt;
    hipStream_t st = (hipStream_t)stream;
    const size_t n = o->cfg.n_local;
    o->cam_ready = false;                                   // (new rows: the camera stage sets itself up again, csrc/fdc_fit2d_init.h)
    o->log_pending = false; o->log_dst = nullptr;
    HIP_TRY(hipMemcpyAsync(o->X0.p + 2 * XDIM, data78, n * XDIM * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->X.p + 2 * XDIM, init78, n * XDIM * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->mask.p + 2, mask, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(o->CAM.p + 2 * 16, cam, n * 16 * sizeof(float), hipMemcpyDeviceToDevice, st));
    return FDCAP_OK;
}

// The clip-level fit's 2D-keypoint reprojection term (fdcap.h; csrc/fdc_fit2d.h ReprojIn).  A refused call changes nothing.
int fdcap_opt_set_reproj(fdcap_ctx* c, const fdcap_reproj_params* p, const float* kp_d, void* stream) {
    if (!c || !c->opt) return FDCAP_E_STATE;
    OptState* o = c->opt;
    if (o->nclip > 1 || o->dctW > 0) return FDCAP_E_STATE;  // (a batch of clips, a DCT term set up: the term is mode 'global''s, one clip)
    if (!p || (reproj_finite(p->weight) && p->weight == 0.f)) {     // off: every launch is again the one it was
        o->reproj = fdcap_reproj_params{};
        return FDCAP_OK;
    }
    if (reproj_params_check(p->fx, p->fy, p->cx, p->cy, p->rho, p->weight) || !kp_d) return FDCAP_E_ARG;
    const size_t n = (size_t)o->cfg.n_local * NJW * 3;
    HIP_TRY(o->reproj_kp.ensure(n));
    HIP_TRY(hipMemcpyAsync(o->reproj_kp.p, kp_d, n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    o->reproj = *p;
    return FDCAP_OK;
}

// The in-loop search of a batch of clips of several scenes: every segment against its own scene with its own pruning state, into
// the flat dist / idx / seedpt.  One launch for all segments where plan_nn_segments says so, else -- the specification -- one
// nn_search launch set per segment in segment order.  Either way seedpt holds every neighbour's coordinates afterwards: the
// backward has ONE scene pointer, so after a form that keeps no records they are gathered from each segment's own scene.
static int opt_search_segments(fdcap_ctx* c, hipStream_t st) {
    OptState* o = c->opt;
    const int nc = c->nc, nseg = (int)o->segs.size();
    const bool seeds = o->sw.nn_seed, cull = o->sw.nn_cull;
    std::vector<int> snq((size_t)nseg), snt((size_t)nseg);
    for (int s = 0; s < nseg; ++s) { snq[s] = o->segs[s].seg.nq; snt[s] = (int)c->scenes[o->segs[s].seg.slot].ns; }
    // (as nn_search sees each segment: culled = seeds and boxes, fragments with the boxes, seeds in place with their coordinates)
    FormSwitches sw = proc_switches();                       // (nn_stream: once per process, as nn_search reads it)
    sw.nn_segments_loop = o->sw.nn_segments_loop;            // (every create)
    const NNSegPlan pl = plan_nn_segments(nseg, snq.data(), snt.data(), seeds && cull, cull, seeds, 1, nn_mode_ref(), sw);
    o->nnpt_filled = false;
    NNSegSearch sg[NN_MAX_SEGS];
    for (int s = 0; s < nseg; ++s) {
        SegSearch& g = o->segs[s];
        const SceneSet& sc = c->scenes[g.seg.slot];
        const size_t base = (size_t)2 * nc + g.seg.q0;
        const float* const q = o->Vw.p + 3 * base;
        float* const dist = o->dist.p + base;
        int* const idx = o->idx.p + base;
        float4* const seedpt = o->seedpt.p + base;
        if (pl.one_launch) {
            sg[s] = NNSegSearch{q, g.seg.nq, sc.nn_target(cull), dist, idx, seedpt, o->nn_cache_of(g), &g.ord, !g.seeded};
        } else {
            const NNCache cache = o->nn_cache_of(g);
            bool written = false;
            HIP_TRY(nn_search(q, g.seg.nq, sc.nn_target(cull), dist, idx, o->pd.p, o->pi.p, g.nsplit, st, seeds ? idx : nullptr, !g.seeded, seedpt,
                              &written, &cache, &g.ord));
            if (!written) {
                hipLaunchKernelGGL(nn_records_gather_kernel, dim3((g.seg.nq + 255) / 256), dim3(256), 0, st, (const int*)idx, g.seg.nq,
                                   (const float4*)sc.scene.p, (const int*)sc.scene_inv.p, seedpt);
                o->nnpt_filled = true;
            }
        }
        g.seeded = true;
    }
    if (pl.one_launch) HIP_TRY(nn_search_segments(pl, sg, nseg, st));
    o->nnpt_valid = true;
    return (int)hipGetLastError();
}

static int opt_contact_forward(fdcap_ctx* c, hipStream_t st, bool blend_done = false) {
    OptState* o = c->opt;
    const int nl = o->cfg.n_local, nc = c->nc;
    const size_t off = (size_t)2 * nc * 3;
    // clip-sized shares: the blend product and the skinning in one launch, else two (plan_contact_forward, fdc_forms.h)
    const SkinModel smf = c->contact.model();
    FormSwitches sw = proc_switches();
    sw.fuse_skin = o->sw.fuse_skin; sw.gemm_split3 = gemm_split3_enabled();
    const ContactFwdPlan pl = plan_contact_forward(nl, nc, NPFX, PNF, blend_done, c->contact.pn_fwdS.f != nullptr, smf.vpack != nullptr, smf.K, smf.ja_hi, sw);
    if (smf.ja_hi > o->pj_fwd.jn) return FDCAP_E_STATE;        // (the skinning reads rows below ja_hi of A: the forward must have written them)
    if (pl.form == F_BLEND_SKIN_FWD) {
        static std::atomic<uint64_t> attr{0};                  // per DEVICE: the attribute belongs to one device's code object
        HIP_TRY(fdc_allow_lds(attr, pl.max_lds, {(const void*)blend_skin_fwd_kernel}));
        note_form(form_name(pl.form));
        hipLaunchKernelGGL(blend_skin_fwd_kernel, dim3(pl.grid), dim3(pl.block), pl.lds, st, o->PF.p, nl,
                           c->contact.pn_fwdS, smf, nc, smf.ja_hi, o->X.p, XDIM, X_TRANSL, o->A.p, o->M.p, o->scale.p, 2, o->Voff.p, o->Vw.p,
                           o->kclip_n(), o->ctab(false));
    } else {
        if (!blend_done) HIP_TRY(blend_forward(c->contact, o->PF.p + 2 * NPFX, nl, o->Voff.p + off, st));
        note_form(form_name(pl.form));
        hipLaunchKernelGGL(skin_fwd_kernel, dim3(pl.grid, pl.grid_y), dim3(pl.block), 0, st, smf, nc, o->X.p, XDIM,
                           X_BETAS, X_TRANSL, o->Voff.p, o->A.p, o->M.p, o->scale.p, 2, 1, o->Vw.p, o->kclip_n(), o->ctab(false));
    }
    lt_mark(o, FDCAP_LT_CONTACT_FWD, st);
    const int nq = nl * nc;
    // the first contact forward of a fit has no neighbours from a previous iteration yet (idx = -1)
    const NNCache cache = o->nn_cache(0);
    const bool timed = o->nn_timing && o->nn_ev_used + 2 <= (int)o->nn_ev.size();
    if (timed) HIP_TRY(hipEventRecord(o->nn_ev[o->nn_ev_used], st));
    if (o->multi_scene()) {
        TraceRange tr_("fdcap:chamfer_nn(K14)");
        int es = opt_search_segments(c, st);
        if (es) return es;
    } else {
        TraceRange tr_("fdcap:chamfer_nn(K14)");
        HIP_TRY(nn_search(o->Vw.p + off, nq, c->scenes[o->scene_slot].nn_target(o->sw.nn_cull), o->dist.p + 2 * nc, o->idx.p + 2 * nc, o->pd.p, o->pi.p,
                          o->nsplit, st, o->sw.nn_seed ? o->idx.p + 2 * nc : nullptr, !o->seeded, o->seedpt.p + 2 * nc, &o->nnpt_valid,
                          &cache, &o->nn_order));
    }
    if (timed) { HIP_TRY(hipEventRecord(o->nn_ev[o->nn_ev_used + 1], st)); o->nn_ev_used += 2; }
    lt_mark(o, FDCAP_LT_CHAMFER_NN, st);
    o->seeded = true;
    return 0;
}

// Mode 'dct' for a batch: row `slot` of dct_wk -- the clips' objective weights weight / (69 W_k) as the host evaluates them
// (dct_clip_weights) -- uploaded when `weight` is not what the row holds.  slot 0 is the zero row (written at fdcap_opt_set_dct_clips).
static int opt_dct_clip_weights(OptState* o, int slot, float weight, hipStream_t st, const float** out) {
    const size_t K = (size_t)o->nclip;
    if (weight == 0.f) slot = 0;
    else if (o->dct_wk_weight[slot] != weight) {
        o->dct_wk_h[slot] = dct_clip_weights(o->nclip, o->clip_lens.data(), o->dctT, weight);
        HIP_TRY(hipMemcpyAsync(o->dct_wk.p + (size_t)slot * K, o->dct_wk_h[slot].data(), K * sizeof(float), hipMemcpyHostToDevice, st));
        o->dct_wk_weight[slot] = weight;
    }
    *out = o->dct_wk.p + (size_t)slot * K;
    return 0;
}

// fuse_ii >= 0 (fdcap_opt_backward_and_step): this backward is followed by the optimiser step of iteration fuse_ii -- `scale`
// is stepped by one more workgroup of the last launch, the rows' part is left pending for the next forward (DeferredStep)
// (clips of different lengths: the kernels take each frame's clip, denominators, stencil extent and weights from the half of the
//  clip table that was built with exactly these lw -- phase 1's or phase 2's; any other weights are refused, never replaced)
static int opt_backward_impl(fdcap_ctx* c, const LossWeights& lw, int32_t log_terms, hipStream_t st, int fuse_ii = -1, int fuse_P = 0) {
    OptState* o = c->opt;
    const fdcap_opt_config& cf = o->cfg;
    // N: the clip length -- the denominators of the means and the stencils' extent (a batch: every clip has N frames)
    const int nl = cf.n_local, nc = c->nc, N = o->clip_len, rpc = o->rows_per_clip(), kn = o->kclip_n();
    const ClipRow* ctab = nullptr;
    if (o->ragged) {
        const auto same = [&lw](const LossWeights& t) {
            return t.rec == lw.rec && t.smooth == lw.smooth && t.contact == lw.contact && t.world == lw.world && t.dct == lw.dct && t.world_on == lw.world_on;
        };
        if (same(opt_phase_weights(cf, false))) ctab = o->ctab(false);
        else if (same(opt_phase_weights(cf, true))) ctab = o->ctab(true);
        // mode 'dct', second phase: the fourth set (the DCT weight is no part of a record: dct_clip_weights)
        else if (o->dct_clips && lw.rec == o->dct_lw.rec && lw.smooth == 0.f && lw.contact == o->dct_lw.contact && lw.world == 0.f && !lw.world_on)
            ctab = o->ctab_dct();
        else return FDCAP_E_STATE;
    }
    const int* const cspan = o->cspan();
    const bool dct_on = lw.dct != 0.f && o->dctW > 0;
    PoseModel pm = c->pose_model();
    TraceRange tr_(fuse_ii >= 0 ? "fdcap:backward_and_step" : "fdcap:backward");
    if (o->log_pending) {                               // a deferred reduction nobody stepped after: deliver it before loss_rows is rewritten
        hipLaunchKernelGGL(loss_rows_reduce_kernel, dim3(o->nclip), dim3(256), 0, st, o->loss_rows.p, 2, rpc, o->log_mask, o->log_assign, o->log_dst,
                           o->dscale_row.p, o->dscale.p, cspan);
        o->log_pending = false;
    }
    double* const losses = log_terms ? o->losses.p : nullptr;       // the partial sums are only formed on logging iterations
    // Logging without a DCT term: every printed term leaves per-frame partials in loss_rows (inside the kernels that run
    // anyway), one small launch sums them.  With the DCT term the separate param_loss_kernel / dct kernel add into losses[].
    const bool rows_log = losses && o->dctW == 0;
    if (losses && !rows_log) HIP_TRY(hipMemsetAsync(losses, 0, (size_t)o->nclip * FDCAP_NUM_LOSSES * sizeof(double), st));
    int row_lo, row_hi;
    opt_row_range(o, 1, &row_lo, &row_hi);
    const bool ahead = o->ahead, blend_done = o->ahead && o->ahead_blend;
    const bool contact_grad = o->contact_on && lw.contact != 0.f;
    const bool contact_fwd = o->contact_on && (contact_grad || log_terms);
    o->lt.phase = contact_grad ? 0 : 1;
    o->skb_valid = false;                                   // (fdcap_debug_skin_bwd_sums: set again below where this backward has a contact gradient)
    // The joints this iteration's loss can reach (plan_pose_joints, fdc_forms.h): the contact terms through the skinning transforms of
    // the joints the contact set is skinned to, everything else through the world joints -- phase 2's world smoothing (world_on), the
    // DCT term, every printed term of a logging iteration.  A sharded run keeps the world joints too: its run-ahead forward and the
    // world-only rows of the launch that follows it read G.  The forward and the backward of one iteration take the same sets.
    // (Mode 'dct' -- a DCT term is set up -- keeps the full sets, as every caller outside this function does.)
    const bool contact_state = contact_fwd || (dct_on || o->dctW > 0);
    const bool need_world = lw.world_on || dct_on || o->dctW > 0 || log_terms != 0 || ahead || cf.n_local != cf.n_total;
    // (The reprojection term reads the body-frame joints 0..22 -- G's translations -- in every iteration: jn >= 23 while it is on.)
    const bool reproj = o->reproj_on();
    if (reproj && (o->dctW > 0 || o->nclip > 1)) return FDCAP_E_STATE;
    const PoseJoints pj = plan_pose_joints(c->h_parents.data(), c->h_depth.data(), contact_fwd ? c->contact.ja_hi : 0, contact_state, need_world,
                                           o->sw.pose_trim && o->dctW == 0, reproj);
    if (contact_grad && (pj.jr != NJ || pj.jn < c->contact.ja_hi)) return FDCAP_E_STATE;     // (dPF reaches every rotation, dA the rows below ja_hi)
    int e = ahead ? opt_pose_forward_rest(c, row_lo, row_hi, st) : opt_pose_forward(c, row_lo, row_hi, st, contact_state, &pj);
    o->ahead = false;
    if (e) return e;
    if (contact_fwd) { e = opt_contact_forward(c, st, blend_done); if (e) return e; }
    // one length: every clip's weights.  Clips of different lengths (N = 0): cw and rpc below are placeholders that only keep
    // ParamLossIn / ContactGradIn / ScaleTail filled in -- the kernels read the table's weights and the tails clip_span's counts
    const ClipWeights cw = clip_weights(std::max(N, 1), lw, cf.weight_loss_rec, cf.weight_contact, nc);
    const float w_rec = cw.w_rec, w_sm = cw.w_sm, w_ws = cw.w_ws;
    // the parameter-space terms: their own kernel when the loss sums are wanted or the DCT term also writes dJw, else
    // formed inside pose_bwd_kernel (one launch less per iteration)
    const bool fuse_pl = (!losses || rows_log) && !(o->dctW > 0 && dct_on);
    ParamLossIn pli = {};
    if (fuse_pl) pli = ParamLossIn{o->X0.p, o->mask.p, o->Jw.p, cf.frame0, N, w_rec, w_sm, w_ws, lw.world_on ? 1 : 0,
                                   rows_log ? o->loss_rows.p : nullptr};
    else                                                  // (a batch -- mode 'dct' through fdcap_opt_run_dct -- in the clip-aware form)
        hipLaunchKernelGGL(param_loss_kernel, dim3(nl), dim3(128), 0, st, o->X.p, o->X0.p, o->mask.p, o->Jw.p, 2, cf.frame0, N,
                           w_rec, w_sm, w_ws, lw.world_on ? 1 : 0, o->dX.p, o->dJw.p, losses, kn, ctab);
    if (o->dct_clips && (dct_on || log_terms)) {          // a batch: every row finds its clip's window, weight and loss slot
        const float* wk = nullptr;
        { int ew = opt_dct_clip_weights(o, 2, dct_on ? lw.dct : 0.f, st, &wk); if (ew) return ew; }
        hipLaunchKernelGGL(dct_joint_grad_clips_kernel, dim3((nl * 69 + 255) / 256), dim3(256), 0, st, o->Jw.p, 2, nl, o->dctT, o->dctC, kn, ctab,
                           o->dct_wstart.p, o->dctD.p, o->dctCoef.p, wk, lw.world_on ? 1 : 0, o->dJw.p, losses);
    } else if (o->dctW > 0 && (dct_on || log_terms))
        hipLaunchKernelGGL(dct_joint_grad_kernel, dim3((nl * 69 + 255) / 256), dim3(256), 0, st, o->Jw.p, 2, cf.frame0, nl, o->dctT,
                           o->dctC, o->dctW, o->dctD.p, o->dctCoef.p, dct_on ? lw.dct / (69.f * (float)o->dctW) : 0.f,
                           lw.world_on ? 1 : 0, o->dJw.p, losses ? losses + 7 : nullptr);
    o->dct_grad = dct_on;
    bool dpf_split = false;
    int dA_rows = NJ;                                       // rows of dA the skinning backward writes (the others are zero and skipped)
    if (contact_grad) {
        ContactGradIn cg;
        // (clips of several scenes: nnpt is always there -- opt_search_segments -- and `scene` is never read)
        cg.Vw = o->Vw.p; cg.dist = o->dist.p; cg.idx = o->idx.p; cg.scene = c->scenes[o->scene_slot].scene.p;
        cg.nnpt = o->nnpt_valid ? o->seedpt.p : nullptr;
        cg.coef = cw.coef;
        cg.loss_rows = losses ? o->loss_rows.p : nullptr;
        const SkinModel smc = c->contact.model();
        const int nnz = c->contact.nnz;
        const bool aligned16 = (((size_t)o->Vw.p | (size_t)o->Voff.p | (size_t)o->dVoff.p | (size_t)o->A.p) & 15) == 0;
        const SkinBwdPlan pl = plan_contact_skin_bwd(nl, nc, nnz, smc.K, smc.vpack != nullptr, smc.csc_v16 != nullptr, aligned16, smc.wf_tab != nullptr,
                                                     o->sw.skin_vec);
        if (pl.ja_rows) dA_rows = c->contact.ja_hi;
        // (gathered records stand in for the scene pointer only: the launch stays the one a stand-alone fit's staged search leads to)
        cg.recompute = pl.form == F_SKIN_BWD_VEC && cg.nnpt != nullptr && o->sw.contact_recompute && !(o->multi_scene() && o->nnpt_filled);
        o->n_recompute += cg.recompute;
        o->skb_cg = cg; o->skb_kn = kn; o->skb_ctab = ctab; o->skb_valid = true;
        const dim3 grid(pl.grid), block(pl.block);
#define FDC_SKC(KERNEL) hipLaunchKernelGGL(KERNEL, grid, block, pl.lds, st, smc, nc, nnz, o->X.p, o->Voff.p, o->A.p, o->M.p, o->scale.p, 2, o->dVoff.p, \
                                           o->dA.p, o->dtransl_v.p, o->dMv.p, o->dsv.p, cg, kn, ctab)
        switch (pl.form) {
        case F_SKIN_BWD_VEC:
            note_form(form_name(pl.form));
            if (pl.G == 1) FDC_SKC(skin_bwd_vec_kernel<1>); else if (pl.G == 2) FDC_SKC(skin_bwd_vec_kernel<2>); else FDC_SKC(skin_bwd_vec_kernel<3>);
            break;
        case F_SKIN_BWD_SMALL: case F_SKIN_BWD_SMALL_K:
            note_form(form_name(pl.form));
            if (pl.vpt == 2 && pl.kc == 8) FDC_SKC((skin_bwd_small_kernel<2, 8>));
            else if (pl.vpt == 2) FDC_SKC((skin_bwd_small_kernel<2, 24>));
            else if (pl.kc == 16) FDC_SKC((skin_bwd_small_kernel<4, 16>));
            else FDC_SKC((skin_bwd_small_kernel<4, 24>));
            break;
        default:
            { int es = skin_bwd_any<true>(c->ws_skin, st, nl, smc, nc, o->X.p, o->Voff.p, o->A.p, o->M.p, o->scale.p, 2,
                                          (const float*)nullptr, o->dVoff.p, o->dA.p, (float*)nullptr, o->dtransl_v.p, o->dMv.p, o->dsv.p, cg, kn, ctab);
              if (es) return es; }
        }
#undef FDC_SKC
        lt_mark(o, FDCAP_LT_SKIN_BWD, st);
        HIP_TRY(blend_backward(c->contact, o->dVoff.p + (size_t)2 * nc * 3, nl, o->dPF.p + 2 * NPFX, (size_t)o->R * NPFX, c->ws_kpart, st, &dpf_split));
        lt_mark(o, FDCAP_LT_BLEND_BWD, st);
    } else if (contact_fwd && losses) {
        if (fuse_pl && rows_log) { pli.cdist = o->dist.p; pli.cnc = nc; }        // (rides in pose_bwd_kernel's prologue: one launch less)
        else hipLaunchKernelGGL(contact_loss_rows_kernel, dim3(nl), dim3(256), 0, st, o->dist.p, nc, 2, o->loss_rows.p);
    }
    const bool joint_grad = lw.world_on || dct_on;
#define FDC_POSE_BWD(KERNEL, ...) \
    hipLaunchKernelGGL(KERNEL, dim3(nl), dim3(64 * POSE_NW), 0, st, pm, o->X.p, o->O.p, o->CAM.p, o->scale.p, 2, o->Rm.p, \
                       o->Jrest.p, o->G.p, contact_grad ? o->dA.p : nullptr, contact_grad ? o->dPF.p : nullptr, \
                       joint_grad ? o->dJw.p : nullptr, contact_grad ? o->dMv.p : nullptr, contact_grad ? o->dsv.p : nullptr, \
                       contact_grad ? o->dPF.p + NPF : nullptr, NPFX, contact_grad ? o->dtransl_v.p : nullptr, o->dX.p, o->dO.p, \
                       o->dCAM.p, o->dscale_row.p, pli, (contact_grad && dpf_split) ? (const float*)(o->dPF.p + (size_t)o->R * NPFX) : (const float*)nullptr, \
                       dA_rows, kn, ctab, pj.jn, pj.jr, pj.nlev, ##__VA_ARGS__)
    if (reproj) {
        // the term rides in this launch (csrc/fdc_k_pose_bwd.inc with FDC_PB_REPROJ): no launch more than without it, booked on FDCAP_LT_POSE_BWD
        if (pj.jn < NJW) return FDCAP_E_STATE;
        const fdcap_reproj_params& q = o->reproj;
        const ReprojIn rp = {o->reproj_kp.p, q.fx, q.fy, q.cx, q.cy, q.rho, q.weight / (float)(NJW * (double)cf.n_total),
                             rows_log ? o->loss_rows.p : nullptr};
        note_form("pose_bwd_reproj_kernel");
        FDC_POSE_BWD(pose_bwd_reproj_kernel, rp);
    } else
        FDC_POSE_BWD(pose_bwd_kernel);
#undef FDC_POSE_BWD
    o->pj_bwd = pj;
    lt_mark(o, FDCAP_LT_POSE_BWD, st);
    // 0 rec, 1 z^2, 2 smoothing, 4 world | 3 contact | 6 reprojection
    const unsigned log_mask = (rows_log ? 0x17u : 0u) | (contact_fwd ? 0x8u : 0u) | (reproj && rows_log ? 0x40u : 0u);
    bool log_in_tail = false;
    {
        ScaleTail tail;
        if (fuse_ii >= 0) {
            const StepPlan sp = opt_step_plan(o, fuse_ii, fuse_P, false, true);
            tail.dscale_row = o->dscale_row.p; tail.row0 = 2;
            if (sp.step_scale) {
                tail.block = 0; tail.sc = sp.sc; tail.dscale = o->dscale.p; tail.n = rpc;
                tail.zero_grad = fuse_ii >= fuse_P ? 1 : 0;
            }
            if (log_terms == 2 && rows_log) {           // the printed sums: same extra workgroup (loss_rows is complete before this launch)
                tail.block = 0; tail.lg = LogReduceIn{o->loss_rows.p, losses, log_mask, 1, rpc};
                log_in_tail = true;
            }
        }
        int eb = opt_vposer_backward(c, false, st, tail);
        if (eb) return eb;
        if (fuse_ii >= 0) { o->pend.on = true; o->pend.ii = fuse_ii; o->pend.P = fuse_P; }
    }
    // d loss / d scale of this rank = sum of the per-frame partials: formed by the step kernels (fused with Adam /
    // the exchange packing); on logging iterations also here, so a caller can read dscale_d right after the backward
    if (log_terms && !log_in_tail) {
        if (log_terms == 2 && rows_log) {               // the sums ride in the step launch that follows (one launch less per iteration)
            o->log_pending = true; o->log_mask = log_mask; o->log_assign = 1; o->log_dst = losses;
        } else
            hipLaunchKernelGGL(loss_rows_reduce_kernel, dim3(o->nclip), dim3(256), 0, st, o->loss_rows.p, 2, rpc, log_mask, rows_log ? 1 : 0, losses,
                               o->dscale_row.p, o->dscale.p, cspan);
    }
    return (int)hipGetLastError();
}

int fdcap_opt_set_loss_output(fdcap_ctx* c, double* losses_d) {
    if (!c || !c->opt || !losses_d) return FDCAP_E_ARG;
    // a logging backward (log_terms = 2) that no step followed left its reduction pending, aimed at the OLD output: that
    // memory may be gone by now (a caller's history row) -- the pending delivery is dropped, never redirected or kept
    c->opt->log_pending = false;
    c->opt->log_dst = nullptr;
    c->opt->losses.p = losses_d;
    return FDCAP_OK;
}

// The part of iteration ii's forward that depends neither on `scale` nor on the halo rows, for the owned rows: decoder, pose
// state, and (when that iteration has a contact term or logs one) the contact set's pose-blend product.  A sharded run issues
// it between fdcap_opt_step_rows_and_pack and fdcap_opt_unpack_and_step_scale, so that it runs while the all-gather is in
// flight ("overlap C1 with the start of the next forward"); fdcap_opt_backward(ii) then only adds the rest.
int fdcap_opt_forward_ahead(fdcap_ctx* c, int32_t ii, int32_t P, int32_t log_terms, void* stream) {
    if (!c || !c->opt || c->opt->nclip > 1) return FDCAP_E_STATE;
    { int es_ = opt_sync(c, (hipStream_t)stream); if (es_) return es_; }
    OptState* o = c->opt;
    hipStream_t st = (hipStream_t)stream;
    const int nl = o->cfg.n_local, nc = c->nc;
    int e = opt_pose_forward(c, 2, 2 + nl, st);
    if (e) return e;
    const bool contact_fwd = o->contact_on && ((ii < P && o->cfg.phase1_contact != 0.f) || log_terms);
    if (contact_fwd) HIP_TRY(blend_forward(c->contact, o->PF.p + 2 * NPFX, nl, o->Voff.p + (size_t)2 * nc * 3, st));
    o->ahead = true;
    o->ahead_blend = contact_fwd;
    return (int)hipGetLastError();
}

int fdcap_opt_backward(fdcap_ctx* c, int32_t ii, int32_t P, int32_t log_terms, void* stream) {
    if (!c || !c->opt) return FDCAP_E_STATE;
    const fdcap_opt_config& cf = c->opt->cfg;
    const bool phase2 = ii >= P;
    const LossWeights lw = opt_phase_weights(cf, phase2);
    return opt_backward_impl(c, lw, log_terms, (hipStream_t)stream);
}

// loss.backward() + optimizer.step() of iteration ii (:591-592) in one call and WITHOUT a launch for the step: `scale` is stepped by
// one more workgroup of the backward's last launch; the rows of body_rotation_rec / camera_ext take their Adam update in the first
// two launches of the NEXT forward, where they are read anyway (DeferredStep, csrc/fdc_loss.h) -- or in the ordinary Adam launch as
// soon as anything else needs them (every other entry point; fdcap_opt_sync).  Same arithmetic in the same order: same bits as
// fdcap_opt_backward + fdcap_opt_step, which is also what this call falls back to where the deferral cannot apply (sharded runs:
// the exchange needs the stepped rows; log_terms == 2: the logged sums ride in the step launch).
int fdcap_opt_backward_and_step(fdcap_ctx* c, int32_t ii, int32_t P, int32_t log_terms, void* stream) {
    if (!c || !c->opt) return FDCAP_E_STATE;
    OptState* o = c->opt;
    const fdcap_opt_config& cf = o->cfg;
    const bool fuse = opt_whole_clips(o) && o->dctW == 0;
    if (!fuse) {
        const int e = fdcap_opt_backward(c, ii, P, log_terms, stream);
        return e ? e : fdcap_opt_step(c, ii, P, stream);
    }
    const bool phase2 = ii >= P;
    const LossWeights lw = opt_phase_weights(cf, phase2);
    return opt_backward_impl(c, lw, log_terms, (hipStream_t)stream, ii, P);
}

// Tests / diagnosis: which queries share a wave of the in-loop search (fdc_chamfer.h NNCache::perm).  The kept work lists go.
int fdcap_debug_nn_query_order(fdcap_ctx* c, int32_t mode, const int32_t* perm_host, int32_t n) {
    if (!c || !c->opt) return FDCAP_E_STATE;
    if (mode < 0 || mode > 2) return FDCAP_E_ARG;
    OptState* o = c->opt;
    NNOrder& ord = o->nn_order;
    if (!o->contact_on || ord.qbuf == nullptr || o->multi_scene()) return FDCAP_E_STATE;    // (several scenes: an order per segment, none to impose)
    const int nq = o->cfg.n_local * c->nc;
    if (mode == 2) {                                         // a permutation of [0, nq), or nothing is changed
        if (!perm_host || n != nq) return FDCAP_E_ARG;
        std::vector<char> seen((size_t)nq, 0);
        for (int i = 0; i < nq; ++i) {
            if (perm_host[i] < 0 || perm_host[i] >= nq || seen[perm_host[i]]) return FDCAP_E_ARG;
            seen[perm_host[i]] = 1;
        }
    }
    HIP_TRY(hipDeviceSynchronize());                         // (no launch in flight reads the table or the lists)
    if (mode == 2) HIP_TRY(hipMemcpy(ord.qbuf, perm_host, (size_t)nq * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(o->nnc_hdr.p, 0xFF, (size_t)(nq + 31) / 32 * sizeof(int)));
    ord.perm_mode = mode;
    ord.perm_n = mode == 2 ? nq : 0;                         // mode 0: the next launch runs in query order and builds one after it
    ord.sorted_groups = 0;
    ord.age = 0;
    return FDCAP_OK;
}

// Tests / diagnosis (r22): what the skinning backward of the last fdcap_opt_backward with a contact gradient left, per frame: dA
// [n_local][55 * 12] (rows below *ja_hi_out are written), dtransl [n_local][3], dM [n_local][12], ds [n_local], dVoff [n_local][nc][3].
// reference != 0: not what the launch left but the same state run again through skin_bwd_small_kernel<., ., false> -- every sum by
// wave_sum on its own, as every build before r22 formed them -- into buffers of its own (contact sets of at most 512 vertices).
int fdcap_debug_skin_bwd_sums(fdcap_ctx* c, int32_t reference, float* dA_d, float* dtransl_d, float* dMv_d, float* dsv_d, float* dVoff_d,
                              int32_t* ja_hi_out, void* stream) {
    if (!c || !c->opt) return FDCAP_E_STATE;
    if (!dA_d || !dtransl_d || !dMv_d || !dsv_d || !dVoff_d || !ja_hi_out) return FDCAP_E_ARG;
    OptState* o = c->opt;
    if (!o->skb_valid) return FDCAP_E_STATE;
    hipStream_t st = (hipStream_t)stream;
    const int nl = o->cfg.n_local, nc = c->nc;
    const size_t R = (size_t)o->R;
    const float *sA = o->dA.p, *sT = o->dtransl_v.p, *sM = o->dMv.p, *sS = o->dsv.p, *sV = o->dVoff.p;
    DevBuf<float> tA, tT, tM, tS, tV;
    if (reference) {
        const SkinModel smc = c->contact.model();
        const int nnz = c->contact.nnz;
        const size_t lds = (size_t)6 * nc * sizeof(float) + (size_t)nnz * sizeof(float) + (((size_t)nnz * 2 + 15) & ~(size_t)15);
        if (nc > 512 || nnz > SKS_MAXNNZ || lds > 57000) return FDCAP_E_STATE;
        HIP_TRY(tA.ensure(R * NJ * 12)); HIP_TRY(tT.ensure(R * 3)); HIP_TRY(tM.ensure(R * 12)); HIP_TRY(tS.ensure(R)); HIP_TRY(tV.ensure(R * nc * 3));
        HIP_TRY(hipMemsetAsync(tA.p, 0, R * NJ * 12 * sizeof(float), st));
        ContactGradIn cg = o->skb_cg;
        cg.recompute = 0; cg.loss_rows = nullptr;
        if (nnz <= 2048)
            hipLaunchKernelGGL((skin_bwd_small_kernel<2, 8, false>), dim3(nl), dim3(256), lds, st, smc, nc, nnz, o->X.p, o->Voff.p, o->A.p, o->M.p,
                               o->scale.p, 2, tV.p, tA.p, tT.p, tM.p, tS.p, cg, o->skb_kn, o->skb_ctab);
        else
            hipLaunchKernelGGL((skin_bwd_small_kernel<2, 24, false>), dim3(nl), dim3(256), lds, st, smc, nc, nnz, o->X.p, o->Voff.p, o->A.p, o->M.p,
                               o->scale.p, 2, tV.p, tA.p, tT.p, tM.p, tS.p, cg, o->skb_kn, o->skb_ctab);
        HIP_TRY(hipGetLastError());
        sA = tA.p; sT = tT.p; sM = tM.p; sS = tS.p; sV = tV.p;
    }
    *ja_hi_out = c->contact.ja_hi;
    hipError_t e = hipMemcpyAsync(dA_d, sA + (size_t)2 * NJ * 12, (size_t)nl * NJ * 12 * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dtransl_d, sT + 2 * 3, (size_t)nl * 3 * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dMv_d, sM + 2 * 12, (size_t)nl * 12 * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dsv_d, sS + 2, (size_t)nl * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dVoff_d, sV + (size_t)2 * nc * 3, (size_t)nl * nc * 3 * sizeof(float), hipMemcpyDeviceToDevice, st);
    const hipError_t es = hipStreamSynchronize(st);            // (the reference's buffers are freed on return)
    if (e == hipSuccess) e = es;
    return e == hipSuccess ? FDCAP_OK : (int)e;
}

// Tests / diagnosis: the query order's sort on its own (nn_query_order, exactly as nn_search launches it) on neighbour positions
// given by the caller, under the key pos >> shift.  Owns its buffers; needs no optimiser state.
int fdcap_debug_nn_query_sort_shift(fdcap_ctx* c, const int32_t* pos_host, int32_t nq, int32_t groups, int32_t hdr_len, int32_t* hdr_io,
                                    int32_t* perm_out, int32_t shift, void* stream) {
    if (!c || !pos_host || !hdr_io || !perm_out || nq <= 0 || groups < 0 || hdr_len < groups) return FDCAP_E_ARG;
    if (shift < NN_KEY_SHIFT_MIN || shift > NN_KEY_SHIFT_MAX) return FDCAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    std::vector<float4> sp((size_t)nq);
    for (int i = 0; i < nq; ++i) {                           // (seedpt[i].w carries the position's int bits)
        sp[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        memcpy(&sp[i].w, &pos_host[i], sizeof(int32_t));
    }
    DevBuf<float4> seedpt;
    DevBuf<int> qbuf, hdr;
    hipError_t e = seedpt.upload(sp.data(), (size_t)nq);
    if (e == hipSuccess) e = qbuf.ensure(nn_query_order_ints(nq));
    if (e == hipSuccess) e = hdr.upload(hdr_io, (size_t)hdr_len);
    if (e == hipSuccess) {                                   // (the three buffers are freed on return: wait, whatever the launches said)
        e = nn_query_order(seedpt.p, nq, qbuf.p, hdr.p, groups, shift, st);
        const hipError_t es = hipStreamSynchronize(st);
        if (e == hipSuccess) e = es;
    }
    if (e == hipSuccess) e = hipMemcpy(perm_out, qbuf.p, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess && hdr_len > 0) e = hipMemcpy(hdr_io, hdr.p, (size_t)hdr_len * sizeof(int), hipMemcpyDeviceToHost);
    return e == hipSuccess ? FDCAP_OK : (int)e;
}
// ... under the quarter key every build before r21 sorted by (pos >> 7)
int fdcap_debug_nn_query_sort(fdcap_ctx* c, const int32_t* pos_host, int32_t nq, int32_t groups, int32_t hdr_len, int32_t* hdr_io,
                              int32_t* perm_out, void* stream) {
    return fdcap_debug_nn_query_sort_shift(c, pos_host, nq, groups, hdr_len, hdr_io, perm_out, 7, stream);
}

// Tests / diagnosis (r21): the streaming search's scheduling choices in one build, process-wide as fdcap_set_nn_kernel.  key_shift: the
// query order's key is the neighbour's position >> key_shift (5, 6, 7; 0: by the scene, nn_order_key_shift).  items_per_chunk: work
// items per 512-point chunk of the one-wave form (4: quarters; 8: 64-point eighths, where their ids fit 16 bits; 0:
// plan_nn_items_per_chunk).  The kept work lists of this context go -- they hold item ids -- the scene operator starts over and an
// optimiser's order is rebuilt after its next launch.
int fdcap_debug_nn_search_form(fdcap_ctx* c, int32_t key_shift, int32_t items_per_chunk) {
    if (!c) return FDCAP_E_STATE;
    if (key_shift != 0 && (key_shift < NN_KEY_SHIFT_MIN || key_shift > NN_KEY_SHIFT_MAX)) return FDCAP_E_ARG;
    if (items_per_chunk != 0 && items_per_chunk != 4 && items_per_chunk != 8) return FDCAP_E_ARG;
    HIP_TRY(hipDeviceSynchronize());                         // (no launch in flight reads the table or the lists)
    nn_key_shift_ref() = key_shift;
    nn_items_ref() = items_per_chunk;
    c->sop.nq = 0;
    OptState* o = c->opt;
    if (!o || !o->contact_on) return FDCAP_OK;
    auto reset = [&](NNOrder& ord, int* hdr, size_t groups) -> hipError_t {
        if (hdr == nullptr || groups == 0) return hipSuccess;
        if (ord.qbuf != nullptr) {
            if (ord.perm_mode == 0) ord.perm_n = 0;           // the next launch runs in query order and builds one after it
            ord.sorted_groups = 0;
            ord.age = 0;
        }
        return hipMemset(hdr, 0xFF, groups * sizeof(int));
    };
    if (!o->segs.empty()) {                                   // (clips of several scenes: an order per segment)
        for (SegSearch& g : o->segs) HIP_TRY(reset(g.ord, g.hdr.p, (size_t)g.seg.groups));
    } else {
        HIP_TRY(reset(o->nn_order, o->nnc_hdr.p, ((size_t)o->cfg.n_local * c->nc + 31) / 32));
    }
    return FDCAP_OK;
}

}  // extern "C"
