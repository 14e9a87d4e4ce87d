// Host side: device buffers, the context (model constants, scene, contact set, operator workspaces), the optimiser state and
// the helpers every entry point shares (row ranges, step plans, the decoder / pose forward pair).  Part of csrc/fdcap.hip.
#pragma once

namespace {

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// FDCAP_SETUP_TRACE=1: the set-up entry points (fdcap_ctx_create, fdcap_set_contact_ids, fdcap_opt_create) print the host time
// of their stages to stderr (tools/setup_timing.py reads the totals from outside; this says where they go)
struct SetupTrace {
    bool on;
    const char* who;
    std::chrono::steady_clock::time_point t0, last;
    explicit SetupTrace(const char* w) : who(w) {
        const char* e = getenv("FDCAP_SETUP_TRACE");
        on = e && e[0] == '1';
        if (on) t0 = last = std::chrono::steady_clock::now();
    }
    void mark(const char* what) {
        if (!on) return;
        (void)hipDeviceSynchronize();
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[fdcap setup] %s: %-28s %8.3f ms (at %8.3f)\n", who, what, std::chrono::duration<double, std::milli>(now - last).count(),
                std::chrono::duration<double, std::milli>(now - t0).count());
        last = now;
    }
};

// skin_bwd_kernel for any vertex set: one workgroup per frame up to a chunk of vertices, the split form + its reduction beyond
// (`part`: workspace, grown as needed).  Same arguments as the kernel.
template <bool CONTACT>
static int skin_bwd_any(DevBuf<float>& part, hipStream_t st, int nrows, SkinModel sm, int nc, const float* X, const float* Voff, const float* A,
                        const float* M, const float* scale, int row0, const float* dVw, float* dVoff, float* dA, float* dbeta_v,
                        float* dtransl_v, float* dMv, float* dsv, ContactGradIn cg, int clip_n = 0, const ClipRow* ctab = nullptr) {
    const SkinBwdPlan pl = plan_skin_bwd_any(nrows, nc, sm.wf_tab != nullptr);
    note_form(form_name(pl.form));
    if (pl.form == F_SKIN_BWD_FRAME) {
        hipLaunchKernelGGL((skin_bwd_kernel<CONTACT, false>), dim3(pl.grid), dim3(pl.block), pl.lds, st, sm, nc, X, Voff, A, M, scale, row0, dVw, dVoff, dA,
                           dbeta_v, dtransl_v, dMv, dsv, cg, (float*)nullptr, clip_n, ctab);
        return (int)hipGetLastError();
    }
    hipError_t e = part.ensure((size_t)nrows * pl.nch * SKP_STRIDE);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((skin_bwd_kernel<CONTACT, true>), dim3(pl.grid, pl.nch), dim3(pl.block), pl.lds, st, sm, nc, X, Voff, A, M, scale, row0, dVw, dVoff, dA,
                       dbeta_v, dtransl_v, dMv, dsv, cg, part.p, clip_n, ctab);
    hipLaunchKernelGGL(skin_bwd_reduce_kernel, dim3(nrows), dim3(256), 0, st, part.p, pl.nch, row0, dA, dbeta_v, dtransl_v, dMv, dsv,
                       CONTACT ? cg.loss_rows : (float*)nullptr);
    return (int)hipGetLastError();
}

struct SkinSet {          // skinning constants for a vertex set (all V, or the contact subset)
    int nv = 0, K = 0, nnz = 0;
    int ldp = 0;                                // row stride of posedirs: 3*nv rounded up to a multiple of 4 (16-byte rows)
    DevBuf<float> vt, ww, posedirs, csc_w;      // posedirs [496, ldp] = [posedirs ; shapedirs^T], zero padding
    DevBuf<int> wj, csc_start, csc_v, csc_chunk;
    int nch = 0, ja_hi = NJ;
    DevBuf<int> wf_tab; DevBuf<uint2> wf_step; DevBuf<float4> wf_frag;              // SkinModel::wf_*
    DevBuf<float4> vpack;                       // SkinModel::vpack / csc_v16 (K <= 4 and nv <= 65535 only)
    DevBuf<unsigned short> csc_v16;
    // the blend matrix in MFMA fragment order (fdc_panel.h), built for vertex sets whose K = 3 nv image fits the LDS slabs:
    // pn_fwd: B(k, n) = posedirs[k, n] (offsets = [pose feature | betas] x B), pn_bwd: B(k, n) = posedirs[n, k] (data gradient)
    DevBuf<float> pn_fwd_f, pn_bwd_f;
    PanelB pn_fwd, pn_bwd;
    DevBuf<unsigned> pn_fwd3_f, pn_bwd3_f;      // the same two operands as split planes (format PnF: panel_gemm3_* kernels)
    DevBuf<float> pn_fwd3_s, pn_bwd3_s;         // their column tiles' inverse scales (PnH2)
    // the forward operand once more with its columns permuted for blend_skin_fwd_kernel (fdc_k_skin.h): sets of <= 512 vertices, K <= 4
    DevBuf<unsigned> pn_fwdS_f; DevBuf<float> pn_fwdS_s; PanelB3 pn_fwdS;
    PanelB3 pn_fwd3, pn_bwd3;
    SkinModel model() const {
        SkinModel m; m.vt = vt.p; m.S = nullptr; m.wj = wj.p; m.ww = ww.p; m.K = K;
        m.csc_start = csc_start.p; m.csc_v = csc_v.p; m.csc_w = csc_w.p;
        m.vpack = (const float*)vpack.p; m.csc_v16 = csc_v16.p;
        m.csc_chunk = csc_chunk.p; m.nch = nch; m.ja_hi = ja_hi;
        m.wf_tab = wf_tab.p; m.wf_step = (const unsigned*)wf_step.p; m.wf_frag = (const float*)wf_frag.p;
        return m;
    }
};

// The keypoint map of the inner fit (fdcap_set_keypoint_map, fdc_keypoints.h): the host tables and the keypoint set's constants
struct KeypointSet {
    KeypointTables h;
    int K = 1;
    DevBuf<int32_t> kjoint, kref, vl_start, vl_k, jl_start, jl_k, pjoint, wj, csc_start, csc_u;
    DevBuf<float> kbary, vl_w, vt, ww, csc_w, Bt;
    SkinSet ss;               // the set's blend matrix (posedirs, ldp) and its panels: what blend_forward / blend_backward take; nothing else of it is filled
    // the free expression's tables (a model with expression directions: fdcap_ctx::h_E10): E [10][lde] the set's expression directions
    // per column 3 u + c (a pseudo-vertex: JE_j's rows), JE [55 3][10]
    DevBuf<float> E, JE;
    int lde = 0;
    void release() { *this = KeypointSet(); }
};

// One registered scene: the full table set fdcap_set_scene builds (fdc_scene.h)
struct SceneSet {
    DevBuf<float4> scene;          // original order {x,y,z,bits(i)}: gradient gather by index
    DevBuf<float4> scene_sorted;   // k-d cell order {x,y,z,bits(original index)}: what the NN scan streams
    DevBuf<float4> scene_bounds;   // axis-aligned box {lo},{hi} of each MF_CH-point chunk of scene_sorted
    DevBuf<float4> scene_sbounds;  // ... of each run of ST4_SUPER chunks
    DevBuf<float4> scene_qbounds;  // ... of each quarter chunk (128 points = four MFMA tiles, one k-d node): [chunk][4]{lo},{hi}; then [chunk][8] of the eighths
    DevBuf<int> scene_inv;         // original index -> position in scene_sorted
    DevBuf<uint4> scene_frags;     // precomputed chunk-centred bf16 MFMA A fragments of scene_sorted
    DevBuf<float4> scene_centers;  // chunk centres {x,y,z,radius}
    int64_t ns = 0;
    NNTarget nn_target(bool cull) const {
        NNTarget t; t.pts = scene_sorted.p; t.n = (int)ns; t.bounds = cull ? scene_bounds.p : nullptr; t.inv_perm = scene_inv.p;
        t.sbounds = cull ? scene_sbounds.p : nullptr; t.qbounds = cull ? scene_qbounds.p : nullptr;
        t.frags = cull ? scene_frags.p : nullptr; t.centers = scene_centers.p;
        return t;
    }
    void release() {
        scene.release(); scene_sorted.release(); scene_bounds.release(); scene_sbounds.release(); scene_qbounds.release();
        scene_inv.release(); scene_frags.release(); scene_centers.release();
        ns = 0;
    }
};
static_assert(CLIP_MAX_SCENES == FDCAP_MAX_SCENES, "fdc_clips.h restates the number of scene slots");

// The search state of ONE segment of a batch of clips of several scenes (fdc_clips.h): what OptState keeps once for a one-scene
// optimiser -- kept lists, headers + launch-order tables, anchors, the query order and its host bookkeeping, whether it has seeds.
struct SegSearch {
    ClipSegment seg = {};
    DevBuf<unsigned short> ids;
    DevBuf<int> hdr;
    DevBuf<float4> anchor;
    DevBuf<int> qbuf;
    NNOrder ord;
    int nsplit = 1;           // scene splits of the segment's staged scans (nn_pick_nsplit for its own queries and scene)
    bool seeded = false;
};

struct OptState {
    fdcap_opt_config cfg;     // a batch of clips (fdcap_opt_create_clips): n_total = n_local = nclip * clip length, frame0 = 0
    int R = 0;            // rows = n_local + 4
    // the clips this optimiser holds: nclip clips of clip_len frames each, clip k in rows 2 + k clip_len .. (one clip or one rank's
    // share of one: nclip = 1, clip_len = n_total).  Each clip has its own scale / moments / dscale / losses slot.
    int nclip = 1, clip_len = 0;
    // clips of DIFFERENT lengths (fdcap_opt_create_clips_var, fdc_clips.h): clip k has clip_lens[k] frames in rows 2 + clip_start[k] ..;
    // clip_len = 0.  The kernels then take clip_n = 0 and the device tables: clip_rows [3][R] ClipRow -- one record per buffer row
    // with the clip's weights of phase 1, then of phase 2 (the only two weight sets mode 'global' has), then of mode 'local''s
    // second loop (clip_weights_local2); built once per create, so no upload in the loop -- and clip_span [nclip][2]
    // {start, length} for the per-clip tail workgroups.  (Mode 'dct''s second phase: a fourth set, clip_rows_dct below.)
    bool ragged = false;
    std::vector<int32_t> clip_lens, clip_start;
    DevBuf<ClipRow> clip_rows;
    DevBuf<int> clip_span;
    const ClipRow* ctab(bool phase2) const { return ragged ? clip_rows.p + (phase2 ? (size_t)R : 0) : nullptr; }
    const ClipRow* ctab_local2() const { return ragged ? clip_rows.p + (size_t)2 * R : nullptr; }
    const int* cspan() const { return ragged ? clip_span.p : nullptr; }
    // what the kernels take as clip_n (clip_of_row, fdc_loss.h): 0 unless the optimiser holds several clips of one length
    int kclip_n() const { return nclip > 1 ? clip_len : 0; }
    // one clip's rows.  Clips of different lengths have no such number: 1, which only says "there are rows" to the tail workgroups
    // (ScaleTail::n, LogReduceIn::n, adam_step_kernel's reduce_n) -- every launch that takes it also takes cspan(), and the
    // kernels read each clip's start and count from there
    int rows_per_clip() const { return ragged ? 1 : cfg.n_local / nclip; }
    bool contact_on = false;
    int nsplit = 8;           // scene splits of the in-loop NN launch
    int nsplit_bf = 8;        // ... of a brute-force launch (timing API)
    struct Ext { float* p = nullptr; } X, CAM, scale, dscale;   // caller-owned, registered
    struct ExtD { double* p = nullptr; } losses;
    DevBuf<float> X0, mask, mX, vX, mCAM, vCAM, mS, vS;
    // fdcap_opt_backward_and_step: the rows' part of iteration ii's optimiser step, to be applied by the next forward's first two
    // launches (DeferredStep, fdc_loss.h; `scale` was stepped by the backward's last launch) -- or by opt_sync()
    struct { bool on = false; int ii = 0, P = 0; } pend;
    DevBuf<float> H1, H2, O, dO;
    DevBuf<float> Opart, dZpart;       // [4][R*126] partial decoder outputs, [4][R*32] partial latent gradients (fdc_panel.h)
    bool dz_pending = false;           // the last backward left the latent gradient as partials: the next Adam launch (or
                                       // fdcap_opt_get_grads) folds them into dX
    // Which rows are defined (plan_pose_joints): a forward writes rows [0, jn) of G / A / Jrest, rows [0, jr) of
    // PF and Jw only with `world`; whatever else these buffers hold is an older launch's and nobody may read it
    DevBuf<float> Rm, PF, Jrest, G, A, M, Jw;
    PoseJoints pj_fwd, pj_bwd;         // the joint sets of the last pose_fwd_kernel / pose_bwd_kernel launch (fdcap_debug_pose_joint_sets)
    DevBuf<float> Voff, Vw, dist, pd, dVoff;
    DevBuf<int> idx, pi;
    // the clip-level reprojection term (fdcap_opt_set_reproj): on while reproj.weight != 0 -- the library's copy of this rank's
    // keypoint rows [n_local,23,3] and the parameters; off (the state after every fdcap_opt_create*): no launch or argument differs
    DevBuf<float> reproj_kp;
    fdcap_reproj_params reproj = {};
    bool reproj_on() const { return reproj.weight != 0.f; }
    DevBuf<float> kp2d;       // per-frame inner fit: 2D keypoints [n_local,23,3] (u, v, confidence), or [n_local,n_kp,3] in map order
    bool kp_mapped = false;   // ... the latter (fdcap_opt_set_keypoints_mapped): the data term runs over the context's keypoint map
    bool kp_panel = false;    // ... with the set's blend products as panel products around the kernel (kp_blend_by_panels)
    DevBuf<float> kpV, kpdV;  // ... their output and input: the set's offsets / offset gradients [n_local, 3 nu]
    DevBuf<float> floss;      // ... and the per-frame objective of its L-BFGS variant
    DevBuf<float> jaw, mJaw, vJaw, jawR9;   // ... its free jaw (fdcap_opt_set_jaw) [n_local, 3], Adam's moments of it, and the skinning part of
                              // d loss / d R_w [n_local, 9] an evaluation leaves (fit2d_kp_jaw_kernel; jaw_grad adds dPF's block)
    DevBuf<float> psi, dpsi, mPsi, vPsi;    // ... its free expression coefficients (fdcap_opt_set_expression) [n_local, 10], the gradient an
                              // evaluation leaves (complete: fit2d_kp_expr_kernel) and Adam's moments
    bool expr_on = false, expr_eval = false;                   // free; an evaluation's gradient is there (until a step consumes it)
    float w_expr = 0.f;                                        // the expression prior's weight (fdcap_opt_set_expression_prior)
    bool jaw_on = false, jaw_eval = false, jaw_gp = false;     // free; an evaluation's gradient parts are there (until a step consumes them); ... with dPF (a set with vertices)
    int lbfgs_rolled_back = 0;                                 // frames the last fdcap_opt_fit2d_lbfgs call found inside a line search when its rounds ran out
    float w_jaw[3] = {0.f, 0.f, 0.f};                          // the jaw prior's weights (fdcap_opt_set_fit2d_extra)
    Fit2dBend bend = {};      // ... its bending prior (fdcap_opt_set_fit2d_extra): w_bend and the terms; n = 0: off
    bool coll_on = false;     // ... its self-interpenetration term (fdcap_opt_set_fit2d_collision; off: not one launch or argument differs)
    fdcap_collision_params coll = {};
    DevBuf<float> coll_loss;  // ... the term's per-frame values [n_local]
    DevBuf<int> coll_count;   // ... and pairs found [n_local]
    bool coll_face = false;   // ... may follow a free jaw and free psi (fdcap_opt_set_fit2d_collision_face; off: both are refused as before)
    DevBuf<float> faceA, facePF, face_part;     // ... then: the corrected transforms [R, 660], the PF rows with the jaw's block [R, 496], d psi's chunk partials
    DevBuf<float> coll2;      // ... the full-mesh pass's sums where the keypoint kernel has assigned the first buffers: dA | dPF | dtransl_v | dMv | dsv
    DevBuf<float> cam_setup;  // ... its camera stage (csrc/fdc_fit2d_init.h): per frame the torso's offsets, the pelvis base and z0 [n_local, CAM_SETUP_LD]
    bool cam_ready = false;   // ... they belong to the current rows and to cam_init's torso (fdcap_opt_set_inputs, any other pose forward: no longer)
    Fit2dInit cam_init = {};
    fdcap_lbfgs* lbfgs = nullptr;
    DevBuf<float4> seedpt;    // coordinates (+ position in the sorted scene) of each query's current neighbour: next launch's seed
    // work-list cache of the in-loop NN launch (fdc_chamfer.h NNCache): ids [groups * 4][64], hdr [groups * 4], anchors [4][nq]
    FormSwitches sw;               // the switches as fdcap_opt_create[_clips] read them (fdc_forms.h): nn_seed, nn_cull, skin_vec, fuse_skin,
                                   // nn_cache_slack, nn_order, pose_trim, nn_keep_records, contact_recompute, nn_box_lanes hold for this
                                   // optimiser; the others are per process (proc_switches())
    DevBuf<float> loss_rows;       // [R][LROW] per-frame partial sums of the printed loss terms (logging iterations)
    bool log_pending = false;      // a logging backward (log_terms = 2) left the reduction of loss_rows to the next step launch
    unsigned log_mask = 0;
    int log_assign = 0;
    double* log_dst = nullptr;
    DevBuf<unsigned short> nnc_ids;
    DevBuf<int> nnc_hdr;
    DevBuf<float4> nnc_anchor;
    DevBuf<int> nnq_buf;                   // the in-loop NN launch's query order + its sort scratch (fdc_chamfer.h NNOrder::qbuf)
    NNOrder nn_order;                      // launch order of the in-loop NN launch (fdc_chamfer.h NNOrder; its tables sit behind nnc_hdr); FDCAP_NN_ORDER=0 turns it off, =k re-sorts every k launches
    // fdcap_opt_launch_timing (r6): a HIP event on the launch stream at every boundary between two launches of an iteration; the time
    // from one event to the next is booked on the launch in between (its ~1 us dependent-launch gap included), per phase of the fit
    struct LaunchTimes {
        bool on = false;
        int used = 0, phase = 0;
        DevEvents ev;
        std::vector<signed char> what;         // what[k]: the stage that ended at event k (FDCAP_LT_*; -1: an iteration's first event), + 16 in phase 2
    } lt;
    // fdcap_opt_nn_timing: HIP events around every in-loop NN launch of a fit (the bench's roofline figure)
    bool nn_timing = false;
    DevEvents nn_ev;
    int nn_ev_used = 0;
    NNCache nn_cache(int) {
        NNCache nc{sw.nn_cache_slack > 0.f ? nnc_ids.p : nullptr, sw.nn_cache_slack > 0.f ? nnc_hdr.p : nullptr, nnc_anchor.p, sw.nn_cache_slack};
        nc.keep = sw.nn_keep_records;                        // (nn_search decides per launch whether the records may be kept)
        nc.box_lanes = sw.nn_box_lanes;
        return nc;
    }
    // Clips of several scenes (fdcap_opt_create_clips_scenes): one entry per segment, each with the search state the members above
    // are for a one-scene optimiser (which keeps none here: segs is empty, and every path is the one it was).  Mode 'global' only.
    std::vector<SegSearch> segs;
    bool multi_scene() const { return segs.size() > 1; }
    int scene_slot = 0;            // the registered scene a one-scene optimiser searches (fdcap_ctx::scenes)
    // several scenes, and the last search took a form that keeps no records: seedpt was filled from each segment's own scene
    // afterwards (the backward's one `scene` pointer cannot serve several), so it holds coordinates but was not the search's own
    bool nnpt_filled = false;
    NNCache nn_cache_of(SegSearch& g) {
        NNCache nc{sw.nn_cache_slack > 0.f ? g.ids.p : nullptr, sw.nn_cache_slack > 0.f ? g.hdr.p : nullptr, g.anchor.p, sw.nn_cache_slack};
        nc.keep = sw.nn_keep_records;
        nc.box_lanes = sw.nn_box_lanes;
        return nc;
    }
    DevBuf<float> dA, dtransl_v, dMv, dsv, dPF, dJw, dX, dCAM, dscale_row;     // d betas: columns 486.. of dPF
    DevBuf<float> VoffF, VwF, dVF;      // mode 'local' second loop: full-mesh pose offsets / world vertices / gradient
    int cam_steps = 0;
    // mode 'dct': basis [T,C], coefficients + Adam moments [W,69,C] (W = n_total / T windows of the whole clip)
    DevBuf<float> dctD, dctCoef, dctM, dctV;
    DevBuf<AdamScalars> adam_tab;
    std::vector<AdamScalars> adam_tab_h;
    int dctT = 0, dctC = 0, dctW = 0;
    // mode 'dct' for a batch (fdcap_opt_set_dct_clips; fdc_clips.h): dctW = the windows of all clips, clip after clip.
    // dct_wtab [dctW] one record per window; dct_wstart [nclip + 1] each clip's first window (host copy: dct_wstart_h);
    // dct_wk [3][nclip] the clips' objective weights weight / (69 W_k) from the host -- row 0 zeros (a coasting step, a logging
    // backward without the term), row 1 under the first phase's weight, row 2 under a backward's -- uploaded when the weight changes;
    // clip_rows_dct [R]: the fourth record set of clips of different lengths, under the second phase's weights (dct_lw: its rec and
    // contact multipliers, the only ones a record depends on)
    bool dct_clips = false;
    DevBuf<DctWindow> dct_wtab;
    DevBuf<int> dct_wstart;
    std::vector<int32_t> dct_wstart_h;
    DevBuf<float> dct_wk;
    std::vector<float> dct_wk_h[3];
    float dct_wk_weight[3] = {0.f, 0.f, 0.f};
    DevBuf<ClipRow> clip_rows_dct;
    LossWeights dct_lw = {};
    const ClipRow* ctab_dct() const { return ragged && dct_clips ? clip_rows_dct.p : nullptr; }
    bool dct_grad = false;    // the last backward gave `scale` a gradient through the DCT term
    bool seeded = false;      // a contact forward has run since fdcap_opt_create (idx holds neighbours)
    // fdcap_opt_forward_ahead ran for the owned rows and nothing has touched them since: the next backward only adds the halo
    // rows and the scale-dependent outputs (ahead_blend: the contact set's pose-blend product is done as well)
    bool ahead = false, ahead_blend = false;
    bool nnpt_valid = false;  // the last contact forward left the neighbours' coordinates in seedpt
    // tests / diagnosis (fdcap_debug_skin_bwd_sums): what the last skinning backward with a contact gradient was launched with
    ContactGradIn skb_cg{};
    int skb_kn = 0;
    const ClipRow* skb_ctab = nullptr;
    bool skb_valid = false;
    int n_recompute = 0;      // tests / diagnosis (fdcap_debug_contact_diet): skinning backwards launched with ContactGradIn::recompute
};

// (fdcap_opt_launch_timing) the stage `what` ended here; -1: an iteration begins
inline void lt_mark(OptState* o, int what, hipStream_t st) {
    OptState::LaunchTimes& t = o->lt;
    if (!t.on || t.used >= (int)t.ev.size()) return;
    if (hipEventRecord(t.ev[t.used], st) != hipSuccess) return;
    t.what[t.used++] = (signed char)(what < 0 ? -1 : what + 16 * t.phase);
}

}  // namespace

struct fdcap_lbfgs {          // batched L-BFGS (csrc/fdc_lbfgs.h): n independent problems
    int n = 0;
    LbfgsCfg cf{};
    DevBuf<LbfgsScalars> S;
    DevBuf<float> W, RO;      // per problem: vector workspace, 1 / (y . s) of the history pairs
    DevBuf<int> active;
    PinnedBuf<int> active_h;  // the host's copy of the current counter
    int round = 0;            // rounds since the last reset: active[round & 1] is the counter of the current one
};

struct fdcap_ctx {
    int V = 0;
    // host copies needed to build vertex subsets
    std::vector<float> h_vt, h_S10, h_lbs;
    std::vector<float> h_E10, h_JE;     // a model with num_shape >= 20: shapedirs' columns 10..19 [3V, 10] and J_regressor times them [55 3][10] (else empty)
    DevBuf<float> d_posedirs, d_S10;    // posedirs [486, 3V] and shapedirs' first ten [3V, 10]: what a vertex set's blend matrix is gathered from (r6: on the device)
    // the full mesh's expression directions as expr_offsets_kernel / expr_dpsi_kernel read them, [10][lde_f] (column 3 v + k; lde_f = 3V
    // rounded up to 4), and JE [55 3][10] (csrc/fdc_face_mesh.h; built by the first call that needs them: ensure_face_tables)
    DevBuf<float> d_Ef, d_JEf;
    int lde_f = 0;
    // device constants
    DevBuf<float> Jt, Jd, hand_comp, hand_mean;
    DevBuf<int> parents, order, level_start, child_start, child_list, depth;
    DevBuf<float> pose_tab;        // all of the above as ONE image in PoseStage's layout (what the staged pose kernels copy)
    int nlevels = 0;
    std::vector<int> h_parents, h_depth;   // host copies of the tree: what plan_pose_joints (fdc_forms.h) decides a launch's joint sets from
    DevBuf<float> W1, b1, W2, b2, W3, b3;
    DevBuf<float> vp_pn[6];            // decoder weights in MFMA fragment order: forward w1 w2 w3, backward w3t w2t w1t
    VPoserPanels vp;
    DevBuf<unsigned> vp_pn3[6];        // ... and as split planes each (format VpF; the default form of the products)
    DevBuf<float> vp_pn3s[6];          // their output columns' inverse scales (PnH2)
    VPoserPanels3 vp3;
    SkinSet full, contact;
    bool full_ready = false;
    KeypointSet kpset;             // fdcap_set_keypoint_map (h.n_kp = 0: no map)
    // fdcap_set_collision_mesh (h.F = 0: no mesh): the faces in tree order, and fdcap_collision_eval's workspace (fdc_collide.h)
    struct CollisionSet {
        CollTables h;
        DevBuf<int32_t> tri, order;
        DevBuf<unsigned long long> ign;
        DevBuf<float> nodes, val, grad;     // node boxes [n][2 NLp][6]; per kept pair its value and 18 gradient components
        DevBuf<int> cnt, list, dest;        // per tree position pairs owned / their prefix; kept pairs {owner, other}; corner -> vertex
        DevBuf<unsigned> key;               // the grouping's sort scratch (cb_key_words)
        DevBuf<int> sval;
        CollMesh view() const { return CollMesh{h.F, h.leaf, h.NL, h.NLp, h.H, (const int4*)tri.p, order.p, ign.p}; }
    } coll;
    KpSet kp_view() const {
        const KeypointSet& k = kpset;
        return KpSet{k.h.n_kp, k.h.nr, k.h.np, k.K, k.ss.ldp, k.kjoint.p, k.kref.p, k.kbary.p, k.vl_start.p, k.vl_k.p, k.vl_w.p, k.jl_start.p, k.jl_k.p,
                     k.vt.p, k.pjoint.p, k.wj.p, k.ww.p, k.csc_start.p, k.csc_u.p, k.csc_w.p, k.ss.posedirs.p, k.Bt.p, Jt.p, Jd.p};
    }
    ExprIO expr_view(const float* psi, float* dpsi, float w) const {
        return ExprIO{psi, dpsi, w, kpset.E.p, kpset.lde, kpset.JE.p, parents.p, child_start.p, child_list.p, depth.p, nlevels};
    }
    // The registered scenes: slot 0 is THE scene of every one-scene entry point (fdcap_set_scene, the scene operator, the
    // diagnostics); the other slots only serve a batch whose clips name them (fdcap_opt_create_clips_scenes).
    SceneSet scenes[FDCAP_MAX_SCENES];
    DevBuf<float4>& scene = scenes[0].scene;
    DevBuf<float4>& scene_sorted = scenes[0].scene_sorted;
    DevBuf<float4>& scene_bounds = scenes[0].scene_bounds;
    DevBuf<float4>& scene_sbounds = scenes[0].scene_sbounds;
    DevBuf<float4>& scene_qbounds = scenes[0].scene_qbounds;
    DevBuf<int>& scene_inv = scenes[0].scene_inv;
    DevBuf<uint4>& scene_frags = scenes[0].scene_frags;
    DevBuf<float4>& scene_centers = scenes[0].scene_centers;
    int64_t& ns = scenes[0].ns;
    NNTarget nn_target(bool cull) const { return scenes[0].nn_target(cull); }
    int nc = 0;
    DevBuf<int> contact_vid;       // mesh vertex of each contact id (caller's order)
    DevBuf<int> contact_perm;      // internal contact slot -> position in the caller's id array
    // growable workspaces for the stand-alone operators
    DevBuf<AdamScalars> ws_adam;
    std::vector<AdamScalars> ws_adam_h;
    DevBuf<float> ws_f[12];
    DevBuf<float> ws_b[12];         // ... of their backward passes (fdcap_vposer_decode_bwd, fdcap_smplx_backward)
    DevBuf<float> ws_part;          // partial decoder outputs of the stand-alone operators
    DevBuf<int> ws_i[2];
    DevBuf<float4> ws_p;
    DevBuf<unsigned> ws_ck;         // fdcap_chamfer_bwd_both: sort keys [2][N] + tile histogram + digit totals (fdc_chamfer_bwd.h cb_key_words)
    DevBuf<int> ws_cv;              // ... and the positions that travel with them [2][N]; N = max(B n, B m) of the largest call so far
    DevBuf<float> ws_skin;         // chunk partials of the split skinning backward (skin_bwd_any)
    DevBuf<float> ws_kpart;         // K-part partial products of the full-mesh data gradient (blend_backward)
    DevBuf<float> ws_face[4];       // the `_face` operators: A' [B, 660], PF' [B, 496], d psi's chunk partials [B, nch, 10], the jaw's R9 [B, 9]
    // Op 1 against the registered scene (fdcap_chamfer_fwd_scene): the previous call's neighbours = the next call's seeds
    struct SceneOp {
        DevBuf<float> dist;
        DevBuf<int> idx, hdr;
        DevBuf<float4> seedpt, anchor;
        DevBuf<unsigned short> ids;
        int nq = 0;                 // queries of the call that left the state (0: none)
    } sop;
    OptState* opt = nullptr;
    Comm comm;                      // fdcap_comm_create: RCCL communicator of the sharded optimiser
    DevBuf<float> xch_send, xch_all;
    std::string comm_err;

    FaceTabs face_tabs() const { return FaceTabs{d_JEf.p, Jt.p, Jd.p, parents.p, child_start.p, child_list.p, depth.p, nlevels}; }
    PoseModel pose_model() const {
        PoseModel pm;
        pm.tab = pose_tab.p;
        pm.Jt = Jt.p; pm.Jd = Jd.p; pm.parents = parents.p; pm.order = order.p; pm.level_start = level_start.p;
        pm.child_start = child_start.p; pm.child_list = child_list.p; pm.hand_comp = hand_comp.p;
        pm.hand_mean = hand_mean.p; pm.nlevels = nlevels; pm.depth = depth.p;
        return pm;
    }
};

namespace {

// largest K = 3 nv for which the blend products run on the fragment-ordered panels (both copies: 2 x 496 x K floats)
constexpr int PANEL_MAX_K = 6144;

// [posedirs ; shapedirs^T] of a vertex set, rows of ldp floats: pd[r, 3 i + k] = component k of vertex ids[i], zero padding
__global__ __launch_bounds__(256) void blend_rows_gather_kernel(const float* __restrict__ posedirs, const float* __restrict__ S10, int V,
                                                                const int* __restrict__ ids, int nv, int ldp, float* __restrict__ pd) {
    const int col = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (col >= ldp) return;
    float v = 0.f;
    if (col < 3 * nv) {
        const int src = 3 * ids[col / 3] + col % 3;
        v = r < NPF ? posedirs[(size_t)r * 3 * V + src] : S10[(size_t)src * NBETA + (r - NPF)];
    }
    pd[(size_t)r * ldp + col] = v;
}
// its columns permuted for blend_skin_fwd_kernel: block b = vertices 64 b .. + 63, tile 3 g + c = component c of vertices 64 b + 16 g .. + 15
__global__ __launch_bounds__(256) void blend_rows_permute_kernel(const float* __restrict__ pd, int ldp, int nv, int ncs, float* __restrict__ ps) {
    const int dst = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (dst >= ncs) return;
    const int b = dst / 192, t = (dst % 192) / 16, jj = dst % 16;
    const int v = 64 * b + 16 * (t / 3) + jj;
    ps[(size_t)k * ncs + dst] = v < nv ? pd[(size_t)k * ldp + 3 * v + (t % 3)] : 0.f;
}

// FDCAP_PANEL_PACK=host: the static operands are packed by the host loops of fdc_panel.h (r1-r5) instead of the device kernels --
// the same arithmetic, kept as the specification (tests compare whole fits of the two, bit for bit).  Read at every call.
inline bool panel_pack_on_host() { const char* e = getenv("FDCAP_PANEL_PACK"); return e && !strcmp(e, "host"); }

// B(k, n) = src[k * sk + n * sn] (DEVICE pointer; sk == 1 or sn == 1) -> fp32 fragment order
int panel_pack_dev(const float* src, size_t src_floats, long sk, long sn, int K, int N, DevBuf<float>& out, int* ntile, int* nss) {
    const int nt = (N + 15) / 16, ns = (K + 15) / 16;
    *ntile = nt; *nss = ns;
    if (panel_pack_on_host()) {
        std::vector<float> h(src_floats), pf;
        HIP_TRY(hipMemcpy(h.data(), src, src_floats * sizeof(float), hipMemcpyDeviceToHost));
        panel_pack(h.data(), sk, sn, K, N, pf, ntile, nss);
        return (int)out.upload(pf.data(), pf.size());
    }
    const size_t lanes = (size_t)nt * ns * 64;
    HIP_TRY(out.ensure(lanes * 4));
    hipLaunchKernelGGL(panel_pack_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, 0, src, sk, sn, K, N, nt, ns, (float4*)out.p);
    return (int)hipGetLastError();
}
// ... -> the split format PnH2 (planes + the column tiles' inverse scales)
int pnf_pack_dev(const float* src, size_t src_floats, long sk, long sn, int K, int N, DevBuf<unsigned>& out, DevBuf<float>& isc, int* ntile,
                 int* nst) {
    const int nt = (N + 15) / 16, ns = (K + 31) / 32;
    if (panel_pack_on_host() || (sk != 1 && sn != 1)) {
        std::vector<float> h(src_floats), sc;
        std::vector<unsigned> p3;
        HIP_TRY(hipMemcpy(h.data(), src, src_floats * sizeof(float), hipMemcpyDeviceToHost));
        PnH2::pack(h.data(), sk, sn, K, N, p3, sc, ntile, nst);
        HIP_TRY(out.upload(p3.data(), p3.size()));
        return (int)isc.upload(sc.data(), sc.size());
    }
    *ntile = nt; *nst = ns;
    const size_t lanes = (size_t)nt * ns * 64;
    HIP_TRY(out.ensure(lanes * 2 * 4)); HIP_TRY(isc.ensure((size_t)nt * 16));
    DevBuf<float> scl;                                            // the columns' scales: only the packing launch needs them
    HIP_TRY(scl.ensure((size_t)nt * 16));
    if (sn == 1) hipLaunchKernelGGL(pnh2_colscale_rowmajor_kernel, dim3((nt * 16 + 255) / 256), dim3(256), 0, 0, src, sk, K, N, nt * 16, scl.p, isc.p);
    else hipLaunchKernelGGL(pnh2_colscale_colmajor_kernel, dim3(nt * 16), dim3(256), 0, 0, src, sn, K, N, nt * 16, scl.p, isc.p);
    hipLaunchKernelGGL(pnh2_pack_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, 0, src, sk, sn, K, N, nt, ns, scl.p, (uint4*)out.p);
    const hipError_t e = hipGetLastError(), es = hipDeviceSynchronize();     // (scl is freed on return: wait, whatever the launches said)
    return (int)(e != hipSuccess ? e : es);
}

int build_skin_set(fdcap_ctx* c, const std::vector<int64_t>& ids, SkinSet* out) {
    SetupTrace tr("build_skin_set");
    const int V = c->V;
    const int nv = (int)ids.size();
    int K = 1;
    for (int v : ids) {
        int k = 0;
        for (int j = 0; j < NJ; ++j) k += c->h_lbs[(size_t)v * NJ + j] != 0.f;
        K = std::max(K, k);
    }
    const int ldp = (3 * nv + 3) & ~3;
    std::vector<float> vt((size_t)nv * 3), ww((size_t)nv * K, 0.f);
    std::vector<int> wj((size_t)nv * K, 0);
    for (int i = 0; i < nv; ++i) {
        int64_t v = ids[i];
        for (int k = 0; k < 3; ++k) vt[3 * i + k] = c->h_vt[3 * v + k];
        int k = 0;
        for (int j = 0; j < NJ; ++j) {
            float w = c->h_lbs[(size_t)v * NJ + j];
            if (w != 0.f) { wj[(size_t)i * K + k] = j; ww[(size_t)i * K + k] = w; ++k; }
        }
    }
    // the set's blend matrix [posedirs ; shapedirs^T] (rows 486..495: the betas part, so [pose feature | betas] x this matrix =
    // pose offsets + shape offsets), gathered on the device from the context's copies
    const size_t pd_floats = (size_t)NPFX * ldp;
    HIP_TRY(out->posedirs.ensure(pd_floats));
    {
        std::vector<int> id32((size_t)std::max(nv, 1), 0);
        for (int i = 0; i < nv; ++i) id32[i] = (int)ids[i];
        DevBuf<int> d_ids;
        HIP_TRY(d_ids.upload(id32.data(), id32.size()));
        if (ldp > 0) hipLaunchKernelGGL(blend_rows_gather_kernel, dim3((ldp + 255) / 256, NPFX), dim3(256), 0, 0, c->d_posedirs.p, c->d_S10.p, V, d_ids.p, nv, ldp, out->posedirs.p);
        const hipError_t e_ = hipGetLastError(), es_ = hipDeviceSynchronize();   // (d_ids is freed at the brace: wait, whatever the launch said)
        HIP_TRY(e_ != hipSuccess ? e_ : es_);
    }
    const float* pd = out->posedirs.p;
    tr.mark("gather vt / weights / posedirs");
    std::vector<int> csc_start(NJ + 1, 0), csc_v;
    std::vector<float> csc_w;
    for (int j = 0; j < NJ; ++j) {
        csc_start[j] = (int)csc_v.size();
        for (int i = 0; i < nv; ++i) {
            float w = c->h_lbs[(size_t)ids[i] * NJ + j];
            if (w != 0.f) { csc_v.push_back(i); csc_w.push_back(w); }
        }
    }
    csc_start[NJ] = (int)csc_v.size();
    out->nnz = (int)csc_v.size();
    if (csc_v.empty()) { csc_v.push_back(0); csc_w.push_back(0.f); }
    while (csc_w.size() & 3) csc_w.push_back(0.f);           // 16-byte staging reads whole float4s
    out->nv = nv; out->K = K; out->ldp = ldp;
    out->vpack.release(); out->csc_v16.release();
    if (K <= 12 && nv > 0 && nv <= 65535) {
        // planes of float4 per vertex (SkinModel::vpack): {template xyz, ids 0-3 as bytes}, {w0..w3}; for K > 4 also {w4..w7}
        // (, {w8..w11}) and last {bits(ids 4-7), bits(ids 8-11), 0, 0} -- skin_vpack_planes(K) planes in all
        const int G = (K + 3) / 4, NP = skin_vpack_planes(K);
        std::vector<float4> vp((size_t)nv * NP);
        for (int i = 0; i < nv; ++i) {
            unsigned jb[3] = {0, 0, 0};
            float w12[12] = {0.f};
            for (int k = 0; k < K; ++k) { jb[k >> 2] |= (unsigned)wj[(size_t)i * K + k] << (8 * (k & 3)); w12[k] = ww[(size_t)i * K + k]; }
            float jf[3]; memcpy(jf, jb, 12);
            vp[(size_t)i] = make_float4(vt[3 * i], vt[3 * i + 1], vt[3 * i + 2], jf[0]);
            for (int g = 0; g < G; ++g) vp[(size_t)(1 + g) * nv + i] = make_float4(w12[4 * g], w12[4 * g + 1], w12[4 * g + 2], w12[4 * g + 3]);
            if (G > 1) vp[(size_t)(1 + G) * nv + i] = make_float4(jf[1], jf[2], 0.f, 0.f);
        }
        std::vector<unsigned short> v16((csc_v.size() + 7) & ~(size_t)7, 0);
        for (size_t i = 0; i < csc_v.size(); ++i) v16[i] = (unsigned short)csc_v[i];
        HIP_TRY(out->vpack.upload(vp.data(), vp.size()));
        HIP_TRY(out->csc_v16.upload(v16.data(), v16.size()));
    }
    {   // chunk entry points of every joint's list (skin_bwd_kernel's chunks of SKB_VCH vertices)
        const int nch = std::max(1, (nv + SKB_VCH - 1) / SKB_VCH);
        std::vector<int> cc((size_t)NJ * (nch + 1), 0);
        for (int j = 0; j < NJ; ++j) {
            int i = csc_start[j];
            for (int ch = 0; ch <= nch; ++ch) {
                while (i < csc_start[j + 1] && csc_v[i] < ch * SKB_VCH) ++i;
                cc[(size_t)j * (nch + 1) + ch] = ch == nch ? csc_start[j + 1] : i;
            }
        }
        out->nch = nch;
        out->ja_hi = skin_ja_hi(csc_start.data(), NJ);
        HIP_TRY(out->csc_chunk.upload(cc.data(), cc.size()));
    }
    tr.mark("lists, vpack, chunk table");
    out->wf_tab.release(); out->wf_step.release(); out->wf_frag.release();
    {   // the weights as MFMA fragments for skin_bwd_kernel's dA (SkinModel::wf_*): vertex sets beyond the contact-set kernels' reach
        // (512 vertices or fewer keep the ordered list form)
        if (nv > 512) {
            const int nchm = (nv + SKB_VCH - 1) / SKB_VCH;
            std::vector<int> tab((size_t)nchm * 16 + 1, 0);
            std::vector<uint2> steps;
            std::vector<float4> frag;
            for (int ch = 0; ch < nchm; ++ch)
                for (int q = 0; q < 4; ++q)
                    for (int jt = 0; jt < 4; ++jt) {
                        tab[((size_t)ch * 4 + q) * 4 + jt] = (int)steps.size();
                        std::vector<int> st;                               // the steps of this quarter that touch the tile
                        std::vector<float> fr;                             // their fragments [step][64]
                        for (int s = 64 * q; s < 64 * q + 64; ++s) {
                            const int v0 = ch * SKB_VCH + 4 * s;
                            if (v0 >= nv) break;
                            float f[64];
                            bool any = false;
                            for (int l = 0; l < 64; ++l) f[l] = 0.f;
                            for (int kk = 0; kk < 4 && v0 + kk < nv; ++kk)
                                for (int k = 0; k < K; ++k) {
                                    const int j = wj[(size_t)(v0 + kk) * K + k];
                                    const float w = ww[(size_t)(v0 + kk) * K + k];
                                    if (w != 0.f && (j >> 4) == jt) { f[16 * kk + (j & 15)] += w; any = true; }
                                }
                            if (any) { st.push_back(s); fr.insert(fr.end(), f, f + 64); }
                        }
                        while (st.size() & 3) { st.push_back(st.empty() ? 0 : st.back()); fr.insert(fr.end(), 64, 0.f); }   // zero weights: no contribution
                        for (size_t g = 0; g < st.size(); g += 4) {
                            steps.push_back(make_uint2((unsigned)st[g] | ((unsigned)st[g + 1] << 16), (unsigned)st[g + 2] | ((unsigned)st[g + 3] << 16)));
                            for (int l = 0; l < 64; ++l)
                                frag.push_back(make_float4(fr[(g + 0) * 64 + l], fr[(g + 1) * 64 + l], fr[(g + 2) * 64 + l], fr[(g + 3) * 64 + l]));
                        }
                    }
            tab.back() = (int)steps.size();
            if (steps.empty()) { steps.push_back(make_uint2(0u, 0u)); frag.resize(64, make_float4(0.f, 0.f, 0.f, 0.f)); }
            HIP_TRY(out->wf_tab.upload(tab.data(), tab.size()));
            HIP_TRY(out->wf_step.upload(steps.data(), steps.size()));
            HIP_TRY(out->wf_frag.upload(frag.data(), frag.size()));
        }
    }
    tr.mark("weight fragments");
    HIP_TRY(out->csc_start.upload(csc_start.data(), csc_start.size()));
    HIP_TRY(out->csc_v.upload(csc_v.data(), csc_v.size()));
    HIP_TRY(out->csc_w.upload(csc_w.data(), csc_w.size()));
    HIP_TRY(out->vt.upload(vt.data(), vt.size()));
    HIP_TRY(out->ww.upload(ww.data(), ww.size()));
    HIP_TRY(out->wj.upload(wj.data(), wj.size()));
    tr.mark("uploads");
    out->pn_fwd = PanelB(); out->pn_bwd = PanelB();
    if (nv > 0) {                                  // forward panel for every set (the full mesh takes the wide form of the kernel)
        int nt = 0, ns = 0;
        int e = panel_pack_dev(pd, pd_floats, ldp, 1, NPFX, 3 * nv, out->pn_fwd_f, &nt, &ns);
        if (e) return e;
        out->pn_fwd.f = (const float4*)out->pn_fwd_f.p; out->pn_fwd.ntile = nt; out->pn_fwd.nss = ns;
    }
    if (nv > 0 && 3 * nv <= PANEL_MAX_K) {         // data-gradient panel while a 16-row block of K = 3 nv columns fits the LDS slabs
        int nt = 0, ns = 0;
        int e = panel_pack_dev(pd, pd_floats, 1, ldp, 3 * nv, NPFX, out->pn_bwd_f, &nt, &ns);
        if (e) return e;
        out->pn_bwd.f = (const float4*)out->pn_bwd_f.p; out->pn_bwd.ntile = nt; out->pn_bwd.nss = ns;
    }
    tr.mark("fp32 panels");
    out->pn_fwd3 = PanelB3(); out->pn_bwd3 = PanelB3();
    if (nv > 0) {                                 // the forward operand of every set also as split planes (format PnF)
        int e = pnf_pack_dev(pd, pd_floats, ldp, 1, NPFX, 3 * nv, out->pn_fwd3_f, out->pn_fwd3_s, &out->pn_fwd3.ntile, &out->pn_fwd3.nst);
        if (e) return e;
        out->pn_fwd3.f = (const uint4*)out->pn_fwd3_f.p; out->pn_fwd3.isc = out->pn_fwd3_s.p;
    }
    tr.mark("split forward panel");
    out->pn_fwdS = PanelB3();
    if (nv > 0 && nv <= 512 && K <= 4) {          // ... and with permuted columns (blend_rows_permute_kernel)
        const int nb = (nv + 63) / 64, ncs = nb * 192;
        DevBuf<float> ps;
        HIP_TRY(ps.ensure((size_t)NPFX * ncs));
        hipLaunchKernelGGL(blend_rows_permute_kernel, dim3((ncs + 255) / 256, NPFX), dim3(256), 0, 0, pd, ldp, nv, ncs, ps.p);
        int e = (int)hipGetLastError();
        if (!e) e = pnf_pack_dev(ps.p, (size_t)NPFX * ncs, ncs, 1, NPFX, ncs, out->pn_fwdS_f, out->pn_fwdS_s, &out->pn_fwdS.ntile, &out->pn_fwdS.nst);
        const int es = (int)hipDeviceSynchronize();      // (ps is freed at the brace: wait, whatever the launches said)
        if (e || es) return e ? e : es;
        out->pn_fwdS.f = (const uint4*)out->pn_fwdS_f.p; out->pn_fwdS.isc = out->pn_fwdS_s.p;
    }
    tr.mark("permuted forward panel");
    if (nv > 0) {                                 // ... and the data-gradient operand (one LDS image up to K = 2528: panel_gemm3 / _rb2k / _ksw; beyond: panel_gemm3_kloop)
        int e = pnf_pack_dev(pd, pd_floats, 1, ldp, 3 * nv, NPFX, out->pn_bwd3_f, out->pn_bwd3_s, &out->pn_bwd3.ntile, &out->pn_bwd3.nst);
        if (e) return e;
        out->pn_bwd3.f = (const uint4*)out->pn_bwd3_f.p; out->pn_bwd3.isc = out->pn_bwd3_s.p;
    }
    HIP_TRY(hipDeviceSynchronize());
    tr.mark("split gradient panel");
    return 0;
}

// dense products on the split formats of fdc_panel.h (FDCAP_GEMM_SPLIT3=0: exact-fp32 MFMA chains instead)
inline bool gemm_split3_enabled() {
    static const bool on = forms_read_env().gemm_split3;       // (once per process, at the first product)
    return on;
}
// pose + shape blend offsets of a vertex set: Voff[M, 3 nv] = PF[M, 496] x [posedirs ; shapedirs^T]
hipError_t blend_forward(const SkinSet& ss, const float* PF, int M, float* Voff, hipStream_t st) {
    TraceRange tr_("fdcap:blend_fwd(K8)");
    if (gemm_split3_enabled() && ss.pn_fwd3.f) return panel_gemm3(PF, NPFX, M, NPFX, ss.pn_fwd3, Voff, 3 * ss.nv, 3 * ss.nv, st);
    if (ss.pn_fwd.f) return panel_gemm(PF, NPFX, M, NPFX, ss.pn_fwd, Voff, 3 * ss.nv, 3 * ss.nv, st);
    return hipSuccess;                            // no vertices (build_skin_set packs both panels for every set with nv > 0): nothing to do
}

// its data gradient: dPF[M, 496] = dVoff[M, 3 nv] x [posedirs ; shapedirs^T]^T.  *split (optional): the product was left as TWO partial
// sums, dPF and dPF + part2_stride (the consumer adds them: pose_bwd_kernel's dPF2); without it the sum is formed here.
hipError_t blend_backward(const SkinSet& ss, const float* dV, int M, float* dPF, size_t part2_stride, DevBuf<float>& ws, hipStream_t st,
                          bool* split = nullptr) {
    TraceRange tr_("fdcap:blend_bwd(K8)");
    if (split) *split = false;
    const int K = 3 * ss.nv;
    if (gemm_split3_enabled() && ss.pn_bwd3.f) {
        const PanelPlan pl = plan_blend_backward(M, K, ss.pn_bwd3.ntile, ss.pn_bwd3.nst, PNF, split && part2_stride, proc_switches());
        if (split) *split = pl.two_partials;
        switch (pl.form) {
        case F_PANEL3_RB2K: return panel_gemm3_rb2k(pl, dV, K, M, K, ss.pn_bwd3, dPF, part2_stride, NPFX, NPFX, st);
        case F_PANEL3_KSW: return panel_gemm3_ksw(pl, dV, K, M, K, ss.pn_bwd3, dPF, NPFX, NPFX, st);
        case F_PANEL3_KLOOP: {
            hipError_t e = ws.ensure((size_t)pl.ks * M * NPFX);
            if (e != hipSuccess) return e;
            return panel_gemm3_kloop(pl, dV, K, M, K, ss.pn_bwd3, ws.p, dPF, NPFX, NPFX, st);
        }
        default: return panel_gemm3(dV, K, M, K, ss.pn_bwd3, dPF, NPFX, NPFX, st);      // one image, the forward's forms
        }
    }
    if (ss.pn_bwd.f) return panel_gemm(dV, K, M, K, ss.pn_bwd, dPF, NPFX, NPFX, st);
    // FDCAP_GEMM_SPLIT3=0 and 3 nv > PANEL_MAX_K (more than 2048 vertices: the full mesh, an all-vertices contact set): no fp32 panel of
    // the operand is kept (build_skin_set) -- the product reads the set's blend matrix as it lies, [496, ldp]
    return gemm_f32_nt(dV, K, ss.posedirs.p, ss.ldp, dPF, NPFX, M, NPFX, K, st);
}

// VPoser decoder forward for rows [row_lo, row_hi) of X (latent read in place at column latent_off): H1, H2 and the four
// partial outputs Opart (fdc_panel.h); O != nullptr: also the summed output (one more small launch -- the optimiser's
// pose_fwd_kernel<true> adds the partials itself instead)
// (row2_lo < row2_hi: a second row range in the same launch -- the halo rows on the far side of a shard's owned rows)
int vposer_forward(fdcap_ctx* c, const float* X, int ldx, int latent_off, int row_lo, int row_hi, float* H1, float* H2,
                   float* Opart, size_t part_stride, float* O, hipStream_t st, int row2_lo = 0, int row2_hi = 0,
                   const DeferredStep& ds = DeferredStep()) {
    const int rows = row_hi - row_lo, rows2 = std::max(row2_hi - row2_lo, 0);
    if (rows <= 0 && rows2 <= 0) return 0;
    if (rows <= 0) { row_lo = row2_lo; row_hi = row2_hi; return vposer_forward(c, X, ldx, latent_off, row_lo, row_hi, H1, H2, Opart, part_stride, O, st, 0, 0, ds); }
    VpRows two;
    const int nb1 = (rows + 15) / 16, nb2 = (rows2 + 15) / 16;
    if (rows2 > 0) { two.nb1 = nb1; two.row2_lo = row2_lo; two.row2_hi = row2_hi; }
    if (O && rows2 > 0) return FDCAP_E_ARG;                   // (the summed output is only formed for one range)
    if (plan_decoder(gemm_split3_enabled()) == F_VPOSER_SPLIT)
        hipLaunchKernelGGL(vposer_fwd_split3_kernel, dim3(4 * (nb1 + nb2)), dim3(512), 0, st, c->vp3, X + latent_off, ldx, row_lo,
                           row_hi, H1, H2, Opart, part_stride, two, ds);
    else
        hipLaunchKernelGGL(vposer_fwd_fused_kernel, dim3(4 * (nb1 + nb2)), dim3(512), 0, st, c->vp, X + latent_off, ldx, row_lo,
                           row_hi, H1, H2, Opart, part_stride, two, ds);
    if (O) {
        const size_t n = (size_t)rows * ODIM;
        hipLaunchKernelGGL(vposer_sum_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Opart, part_stride,
                           (size_t)row_lo * ODIM, n, O);
    }
    return (int)hipGetLastError();
}

// The optimiser holds whole clips -- one clip, or a batch of them (fdcap_opt_create_clips) -- rather than one rank's share of a
// sharded clip: no halo rows, no exchange, and the single-GPU schedule (deferred row step, `scale` stepped by the backward's tail).
inline bool opt_whole_clips(const OptState* o) { return o->cfg.frame0 == 0 && o->cfg.n_local == o->cfg.n_total; }

// a batch of several clips (fdcap_opt_create_clips): the single-step entry points of modes 'local' / 'dct', the per-frame inner fit
// and the sharded exchange refuse it (FDCAP_E_STATE); it reaches those two modes through fdcap_opt_run_local2 / fdcap_opt_run_dct
inline bool opt_is_batch(const fdcap_ctx* c) { return c && c->opt && c->opt->nclip > 1; }
// ... of clips of several scenes (fdcap_opt_create_clips_scenes, more than one segment): mode 'global' only -- on top of what a batch
// is refused, fdcap_opt_run_local2, fdcap_opt_set_dct_clips and fdcap_opt_run_dct return FDCAP_E_STATE
inline bool opt_is_multi_scene(const fdcap_ctx* c) { return c && c->opt && c->opt->multi_scene(); }
// the clip-level reprojection term is on (fdcap_opt_set_reproj): mode 'global' only -- mode 'local''s second loop and every DCT call
// return FDCAP_E_STATE
inline bool opt_has_reproj(const fdcap_ctx* c) { return c && c->opt && c->opt->reproj_on(); }

// rows of the optimiser's buffers whose pose is needed: the owned frames plus `halo` frames on each side that has a neighbour
void opt_row_range(const OptState* o, int halo, int* lo, int* hi) {
    const fdcap_opt_config& cf = o->cfg;
    if (opt_whole_clips(o)) { *lo = 2; *hi = cf.n_local + 2; return; }
    *lo = cf.frame0 > 0 ? 2 - halo : 2;
    *hi = cf.n_local + 2 + (cf.frame0 + cf.n_local < cf.n_total ? halo : 0);
}

// The optimiser step of iteration ii as tensors for the Adam kernels (global_optimization.py:563-568, :577-580, :592 restated as
// arithmetic): which parameters are stepped, with which bias corrections.
struct StepPlan { AdamTensor x = {}, cam = {}, sc = {}; int nb_x = 0, nb_cam = 0; bool step_scale = false; };
StepPlan opt_step_plan(const OptState* o, int ii, int P, bool do_rows, bool do_scale) {
    const fdcap_opt_config& cf = o->cfg;
    const int nl = cf.n_local;
    StepPlan sp;
    // body_rotation_rec: every iteration, its own step counter = ii + 1
    if (do_rows) {
        sp.x = AdamTensor{o->X.p + 2 * XDIM, o->mX.p + 2 * XDIM, o->vX.p + 2 * XDIM, o->dX.p + 2 * XDIM, (size_t)nl * XDIM, adam_scalars(cf.lr, ii + 1)};
        sp.nb_x = (int)((sp.x.n + 255) / 256);
    }
    // camera_ext: first gradient at ii = P + 1 (flag flips after the forward of ii = P); mode 'local': the late-phase
    // loss has no camera_ext path -> grad None, never stepped
    if (do_rows && ii >= P + 1 && cf.phase2_world != 0.f) {
        sp.cam = AdamTensor{o->CAM.p + 2 * 16, o->mCAM.p + 2 * 16, o->vCAM.p + 2 * 16, o->dCAM.p + 2 * 16, (size_t)nl * 16, adam_scalars(cf.lr, ii - P)};
        sp.nb_cam = (int)((sp.cam.n + 255) / 256);
    }
    // scale: receives a gradient while ii < P (and only if a term that reaches it exists)
    sp.step_scale = do_scale && (o->contact_on || o->dct_grad) && (ii < P || cf.legacy_zero_grad);
    if (sp.step_scale) sp.sc = AdamTensor{o->scale.p, o->mS.p, o->vS.p, o->dscale.p, 1, adam_scalars(cf.lr, ii + 1)};
    return sp;
}
int opt_step_launch(fdcap_ctx* c, int32_t ii, int32_t P, bool do_rows, bool do_scale, bool reduce_scale, hipStream_t st, float* xch);

// Everything the caller registered (rows_x_d, rows_cam_d) and the Adam moments are current after this: the rows' part of a
// deferred step that no forward has consumed is applied by the ordinary Adam launch (`scale` was stepped with the backward).
int opt_sync(fdcap_ctx* c, hipStream_t st) {
    OptState* o = c->opt;
    if (!o || !o->pend.on) return 0;
    o->pend.on = false;
    return opt_step_launch(c, o->pend.ii, o->pend.P, true, false, false, st, nullptr);
}

// decoder + per-frame pose state (Rm, PF, Jrest, G, A, M, Jw) of rows [lo, hi): two launches.  A deferred optimiser step is
// applied by these two launches when they cover exactly the frames it steps (no halo rows: one rank), else by its own launch first.
// contact_state = false: the pose feature PF and the skinning transforms A -- read by the contact forward only -- are not written
// (phase 2 of a fit that does not log: 4.7 MB less for the end of the launch to write back, tools/launch_overhead_probe.hip)
// pj: the joints the caller's loss can reach (plan_pose_joints, fdc_forms.h) -- it then reads no row of G / A / Jrest at or above
// pj->jn and Jw only with pj->world; nullptr: the full sets
int opt_pose_forward(fdcap_ctx* c, int lo, int hi, hipStream_t st, bool contact_state = true, const PoseJoints* pj = nullptr) {
    OptState* o = c->opt;
    const PoseJoints full = plan_pose_joints(c->h_parents.data(), c->h_depth.data(), NJ, true, true, false);
    const PoseJoints& js = pj ? *pj : full;
    o->pj_fwd = js;
    o->ahead = false;                                       // (whatever ran ahead is recomputed here)
    o->cam_ready = false;                                   // (whoever runs the model may step any column: the camera stage sets itself up again, fdc_fit2d_init.h)
    const size_t ps = (size_t)o->R * ODIM;
    const int nl = o->cfg.n_local;
    DeferredStep ds;
    if (o->pend.on) {
        if (lo == 2 && hi == 2 + nl && opt_whole_clips(o) && !o->log_pending) {
            const StepPlan sp = opt_step_plan(o, o->pend.ii, o->pend.P, true, false);
            ds.on = 1; ds.x = sp.x; ds.cam = sp.cam; ds.row0 = 2;
            ds.dzpart = o->dz_pending ? o->dZpart.p : nullptr; ds.dz_stride = (size_t)o->R * VP_Z;
        } else {
            int e = opt_sync(c, st);
            if (e) return e;
        }
    }
    lt_mark(o, -1, st);
    int e = vposer_forward(c, o->X.p, XDIM, X_LATENT, lo, hi, o->H1.p, o->H2.p, o->Opart.p, ps, nullptr, st, 0, 0, ds);
    if (e) return e;
    lt_mark(o, FDCAP_LT_VPOSER_FWD, st);
    hipLaunchKernelGGL(pose_fwd_kernel<true>, dim3(hi - lo), dim3(64 * POSE_NW), 0, st, c->pose_model(), o->X.p, o->O.p, o->CAM.p, o->scale.p, lo,
#ifdef FDC_DEBUG_BUFFERS
                       o->Rm.p,                                // (the per-joint rotations: nobody reads them back but fdcap_debug_rows)
#else
                       (float*)nullptr,
#endif
                       contact_state ? o->PF.p : (float*)nullptr, o->Jrest.p, o->G.p, contact_state ? o->A.p : (float*)nullptr, o->M.p,
                       js.world ? o->Jw.p : (float*)nullptr, (const float*)nullptr, (const float*)o->Opart.p, ps, 0, 0, ds, o->kclip_n(), o->ctab(false),
                       js.jn, js.jr, js.nlev);
    lt_mark(o, FDCAP_LT_POSE_FWD, st);
    if (ds.on) {                                            // the step has been issued: the launches that follow see its results
        o->pend.on = false;
        o->dz_pending = false;
    }
    return (int)hipGetLastError();
}

// After fdcap_opt_forward_ahead: what is left of opt_pose_forward(lo, hi) -- the halo rows on either side of the owned rows in
// full (their parameters arrived with the exchange), and M / Jw of the owned rows (`scale` was stepped by the exchange's tail).
// Two launches, nearly empty.
int opt_pose_forward_rest(fdcap_ctx* c, int lo, int hi, hipStream_t st) {
    OptState* o = c->opt;
    const int nl = o->cfg.n_local;
    const size_t ps = (size_t)o->R * ODIM;
    int e = vposer_forward(c, o->X.p, XDIM, X_LATENT, lo, 2, o->H1.p, o->H2.p, o->Opart.p, ps, nullptr, st, 2 + nl, hi);
    if (e) return e;
    hipLaunchKernelGGL(pose_fwd_kernel<true>, dim3(hi - lo), dim3(64 * POSE_NW), 0, st, c->pose_model(), o->X.p, o->O.p, o->CAM.p, o->scale.p, lo,
                       (float*)nullptr /* Rm: see opt_pose_forward */, o->PF.p, o->Jrest.p, o->G.p, o->A.p, o->M.p, o->Jw.p, (const float*)nullptr, (const float*)o->Opart.p, ps,
                       2, 2 + nl);
    return (int)hipGetLastError();
}

// VPoser data-gradient dO -> d latent of the owned rows, left as four partials in dZpart (fold = true: added into dX here)
// (tail.block >= 0: one more workgroup that steps `scale` -- ScaleTail, fdc_loss.h)
int opt_vposer_backward(fdcap_ctx* c, bool fold, hipStream_t st, ScaleTail tail = ScaleTail()) {
    OptState* o = c->opt;
    const int nl = o->cfg.n_local;
    const size_t ps = (size_t)o->R * VP_Z;
    const int nb = 4 * ((nl + 15) / 16);
    if (tail.block >= 0) tail.block = 0;                   // (first in the grid: fdc_panel.h)
    tail.nclip = o->nclip; tail.clip_n = o->rows_per_clip();      // (a batch: one tail workgroup per clip)
    tail.clip_span = o->cspan();
    const bool split3 = plan_decoder(gemm_split3_enabled()) == F_VPOSER_SPLIT;
    if (split3 && tail.lg.rows && nb >= LROW && o->nclip == 1) {
        tail.lg_spread = 1;                                // the logged sums: one regular workgroup per term (ScaleTail::lg_spread)
        if (tail.n <= 0) tail.block = -1;                  // ... and with no `scale` step there is nothing left for an extra workgroup
    }
    if (split3)
        hipLaunchKernelGGL(vposer_bwd_split3_kernel, dim3(nb + (tail.block >= 0 ? tail.nclip : 0)), dim3(512), 0, st, c->vp3, o->dO.p, 2, 2 + nl, o->H1.p, o->H2.p,
                           o->dZpart.p, ps, tail);
    else
        hipLaunchKernelGGL(vposer_bwd_fused_kernel, dim3(nb + (tail.block >= 0 ? tail.nclip : 0)), dim3(512), 0, st, c->vp, o->dO.p, 2, 2 + nl, o->H1.p, o->H2.p,
                           o->dZpart.p, ps, tail);
    lt_mark(o, FDCAP_LT_VPOSER_BWD, st);
    if (fold) {
        hipLaunchKernelGGL(vposer_fold_dz_kernel, dim3((nl * VP_Z + 255) / 256), dim3(256), 0, st, o->dZpart.p, ps, 2, nl, o->dX.p);
        o->dz_pending = false;
    } else {
        o->dz_pending = true;
    }
    return (int)hipGetLastError();
}

}  // namespace
