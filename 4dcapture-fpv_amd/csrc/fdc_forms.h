// Which kernel FORM every launch takes, as pure functions of sizes, layout flags and switches: no HIP types, no getenv inside a
// plan.  The launch sites (fdc_panel.h, fdc_state.h, fdc_api_opt.h, fdc_chamfer.h) ask for a plan and switch on its form; they keep
// only what needs HIP.  Compiles with plain g++ -std=c++17 (tests/test_forms_cpu.py pins every plan against tests/forms_table.json)
// and with hipcc.  Every threshold's measurement sits next to the threshold.
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include <algorithm>

#include "fdc_clips.h"

#if defined(__HIPCC__)
#define FDC_FORMS_HD __host__ __device__
#else
#define FDC_FORMS_HD
#endif

namespace fdc {

// ---------------------------------------------------------------------------------------------------------------------
// The selection / pruning switches as data.  forms_read_env() is the only place that reads them; WHEN it is called is the
// switch's lifetime ("read when"):
//   once per process     proc_switches(): clip_fwd_rows, clip_kgrad_rows, pn_rb2, pn_nw, pn_ksw, nn_stream;
//                        gemm_split3 through gemm_split3_enabled(); nn_cache_slack as fdcap_chamfer_fwd_scene uses it
//   every opt_create     nn_seed, nn_cull, skin_vec, fuse_skin, nn_cache_slack, nn_order, pose_trim, nn_keep_records,
//                        contact_recompute, nn_box_lanes, nn_segments_loop (copied into the optimiser state)
//   every call           gemm_split3 in fdcap_panel_gemm
struct FormSwitches {
    // FDCAP_CLIP_FORMS_MIN_ROWS: row count from which the clip-sized forms are selected; it overrides BOTH thresholds -- tests run
    // the reference's own 300-frame fixtures (the reference hard-codes 300, :41-42) through the forms BASELINE configs 2 / 3 / 5 select.
    //   forward (two row blocks per fragment stream in the blend product, the fused contact forward): measured break-even 336 (r6
    //   sweep: contact forward as two launches / fused 11.7 / 12.6 us at 320 rows, 13.7 / 12.8 at 352; 384 until then).
    int clip_fwd_rows = 336;
    //   K-split data gradient (panel_gemm3_rb2k): from 257 rows.  r6 (tools/launch_times.py): the one-tile-stream form
    //   (panel_gemm3_ksw) keeps one workgroup per CU, so from 17 row blocks x 16 column groups = 272 workgroups on it runs in two
    //   rounds -- 16.6 us at 272-352 rows against 9.7 at 256 -- while the two-row-block K-split form takes 10.7-11.0 us there: a
    //   300-frame clip (the reference's real clip length) 42.4 -> 40.0 ms per fit.  At 256 rows and below the one-round form wins
    //   (9.7 vs 11.2 us).
    int clip_kgrad_rows = 257;
    int pn_rb2 = 1;              // FDCAP_PN_RB2 (A/B): 0 one row block per fragment stream everywhere, 1 both forms, 2 forward only, 3 K-split only
    int pn_nw = 0;               // FDCAP_PN_NW (A/B): 8 / 4 / 2 pins panel_gemm3_kernel's waves per workgroup
    bool pn_ksw = true;          // FDCAP_PN_KSW=0: never the K-split-over-waves data gradient
    bool gemm_split3 = true;     // FDCAP_GEMM_SPLIT3=0: exact-fp32 MFMA chains instead of the split formats of fdc_panel.h
    // FDCAP_NN_STREAM (tests: each form the size rule picks, forced): 0 the staged kernel; 11 / 21 / 41 nn_stream4_kernel with
    // 1 / 2 / 4 waves per group of 32 queries; unset (< 0): waves per group by launch size
    int nn_stream = -2;
    bool nn_seed = true, nn_cull = true;      // FDCAP_NN_SEED=0 / FDCAP_NN_CULL=0: no seeds from the last iteration / no chunk culling
    int nn_order = 32;           // FDCAP_NN_ORDER: base re-sort period of the in-loop search's launch and query order (nn_order_period below); 0 turns it off
    float nn_cache_slack = 0.03f;             // FDCAP_NN_CACHE_SLACK: metres; 0 disables the kept work lists
    bool skin_vec = true;        // FDCAP_SKIN_VEC=0 (A/B): the scalar-load skinning backward
    bool fuse_skin = true;       // FDCAP_FUSE_SKIN=0 (A/B): blend product and skinning forward as two launches
    // FDCAP_POSE_TRIM=0: the pose kernels treat all 55 joints alike (plan_pose_joints' full plan).
    bool pose_trim = true;
    // r14.  FDCAP_NN_KEEP_RECORDS=0: the in-loop search rewrites every neighbour record in every launch (NNCache::keep,
    // fdc_chamfer.h).  FDCAP_CONTACT_RECOMPUTE=0: skin_bwd_vec_kernel stages the world vertices, the distances and all 55 skinning
    // transforms instead of forming the first two and staging the rows below ja_hi.
    bool nn_keep_records = true;
    bool contact_recompute = true;
    // r15.  FDCAP_NN_BOX_LANES: lanes that share one box in the in-loop search's per-query box tests (nn_box_lanes below): 0 by the
    // pass's count, 2 a pair everywhere (every launch before r15), 4 / 8 forced; anything else is 0.
    int nn_box_lanes = 0;
    // FDCAP_NN_SEGMENTS=loop: a batch of clips of several scenes (fdcap_opt_create_clips_scenes) searches segment after segment, one
    // nn_search launch set each -- the specification of the one-launch form (plan_nn_segments below) -- whatever the sizes.
    bool nn_segments_loop = false;
};
inline FormSwitches forms_read_env() {
    FormSwitches s;
    const auto off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
    if (const char* e = getenv("FDCAP_CLIP_FORMS_MIN_ROWS")) s.clip_fwd_rows = s.clip_kgrad_rows = std::max(32, atoi(e));
    if (const char* e = getenv("FDCAP_PN_RB2")) s.pn_rb2 = atoi(e);
    if (const char* e = getenv("FDCAP_PN_NW")) s.pn_nw = atoi(e);
    s.pn_ksw = !off("FDCAP_PN_KSW");
    s.gemm_split3 = !off("FDCAP_GEMM_SPLIT3");
    if (const char* e = getenv("FDCAP_NN_STREAM")) s.nn_stream = atoi(e);
    s.nn_seed = !off("FDCAP_NN_SEED");
    s.nn_cull = !off("FDCAP_NN_CULL");
    if (const char* e = getenv("FDCAP_NN_ORDER")) s.nn_order = atoi(e);
    if (const char* e = getenv("FDCAP_NN_CACHE_SLACK")) s.nn_cache_slack = (float)atof(e);
    s.skin_vec = !off("FDCAP_SKIN_VEC");
    s.fuse_skin = !off("FDCAP_FUSE_SKIN");
    s.pose_trim = !off("FDCAP_POSE_TRIM");
    s.nn_keep_records = !off("FDCAP_NN_KEEP_RECORDS");
    s.contact_recompute = !off("FDCAP_CONTACT_RECOMPUTE");
    if (const char* e = getenv("FDCAP_NN_BOX_LANES")) { const int v = atoi(e); s.nn_box_lanes = (v == 2 || v == 4 || v == 8) ? v : 0; }
    s.nn_segments_loop = clip_segments_loop_env();           // FDCAP_NN_SEGMENTS=loop (named where segments are defined: fdc_clips.h)
    return s;
}
inline const FormSwitches& proc_switches() { static const FormSwitches s = forms_read_env(); return s; }

// ---------------------------------------------------------------------------------------------------------------------
// Forms and the names fdcap_debug_kernel_forms reports for them (nullptr: the launch is not reported)
enum Form {
    F_NONE = 0,               // no admissible split form: the caller's exact-fp32 path (or an argument error)
    F_PANEL3, F_PANEL3_RB2, F_PANEL3_WIDE, F_PANEL3_RB2K, F_PANEL3_KSW, F_PANEL3_KLOOP,
    F_BLEND_SKIN_FWD, F_SKIN_FWD,
    F_SKIN_BWD_VEC, F_SKIN_BWD_SMALL, F_SKIN_BWD_SMALL_K, F_SKIN_BWD_FRAME, F_SKIN_BWD_CHUNKS_MFMA, F_SKIN_BWD_CHUNKS_LIST,
    F_NN_STREAM_W4, F_NN_STREAM_W2, F_NN_STREAM_W1, F_NN_MFMA, F_NN_DIRECT,
    F_VPOSER_SPLIT, F_VPOSER_FP32,
    F_COUNT
};
inline const char* form_name(Form f) {
    static const char* const names[F_COUNT] = {
        nullptr,
        "panel_gemm3_kernel", "panel_gemm3_rb2_kernel", "panel_gemm3_wide_kernel", "panel_gemm3_rb2k_kernel", "panel_gemm3_ksw_kernel",
        "panel_gemm3_kloop_kernel",
        "blend_skin_fwd_kernel", "skin_fwd_kernel",
        "skin_bwd_vec_kernel", "skin_bwd_small_kernel", "skin_bwd_small_kernel(K > 4)", "skin_bwd_kernel(one workgroup per frame)",
        "skin_bwd_kernel(chunks, MFMA dA)", "skin_bwd_kernel(chunks, list dA)",
        // (labels that tests and tests/forms_table.json pin, not template spellings: the one-wave form is nn_stream4_kernel<1, 1>)
        "nn_stream4_kernel(4 waves per group)", "nn_stream4_kernel(2 waves per group)", "nn_stream4_kernel<1,1,1>", "nn_mfma_kernel",
        "nn_direct_kernel",
        nullptr, nullptr,
    };
    return names[f];
}

// ---------------------------------------------------------------------------------------------------------------------
// Split products (fdc_panel.h).  `np`: planes of the operand format (PnH2: 2); ntile = ceil(N / 16) column tiles and
// nst = ceil(K / 32) steps of the static operand.

// uint4 per 16-row LDS image of kpad columns (behind the planes: 16 inverse row scales + 16 partial maxima per wave, <= 12 waves);
// bytes of rb of them
constexpr int PN_SC_U4 = 4 + 4 * 12;
constexpr FDC_FORMS_HD int pn_img_u4(int np, int kpad) { return np * (kpad >> 3) * 16 + PN_SC_U4; }
constexpr FDC_FORMS_HD size_t pn_lds_bytes(int np, int kpad, int rb) { return (size_t)rb * pn_img_u4(np, kpad) * 16; }
// longest K whose single-slab LDS image (pn_lds_bytes(2, kpad, 1)) fits the 160 KB of a gfx950 CU
constexpr int PN3_MAX_K = 2528;
static_assert(pn_lds_bytes(2, PN3_MAX_K, 1) <= 160 * 1024, "one image per CU");
constexpr bool panel_gemm3_fits(int K) { return ((K + 31) & ~31) <= PN3_MAX_K; }
constexpr size_t pn_b_bytes(int np, int ntile, int nst) { return (size_t)ntile * nst * np * 1024; }

// Workgroup -> (row block, column block), XCD-aware.  The dispatcher deals consecutive workgroups to the 8 XCDs round-robin
// (b % 8), and each XCD has its own 4 MiB L2: with a plain 2-D grid every XCD pulls nearly all of A AND all of B through the
// fabric in every launch (measured: 5.6 k cycles just to stage a 31 KB A block, fragment loads at Infinity-Cache latency).
// Here XCD x owns the rectangle (row group x / xc, column group x % xc): its slice of the STATIC operand B stays resident in
// its L2 from one optimiser iteration to the next, and A crosses the fabric xc times instead of 8.
struct PnMap { int nrb, ncb, xc, rpg, cpg, rfast; };   // row / column blocks; column groups; blocks per group; slot order
inline PnMap panel_map(int nrb, int ncb, size_t a_bytes, size_t b_bytes) {
    PnMap best{nrb, ncb, 1, (nrb + 7) / 8, ncb, 0};
    double best_cost = 1e300;
    for (int xc = 1; xc <= 8; xc *= 2) {
        const int xr = 8 / xc;
        const int rpg = (nrb + xr - 1) / xr, cpg = (ncb + xc - 1) / xc;
        // fabric bytes per launch: A once per column group; B once per row group unless an XCD's slice is small enough to
        // stay in its L2 between launches; + a penalty for idle slots of ragged groups
        double cost = (double)xc * a_bytes + ((b_bytes / xc <= (size_t)(3u << 19)) ? 0.0 : (double)xr * b_bytes);
        cost *= (double)(8 * rpg * cpg) / (double)(nrb * ncb);
        if (cost < best_cost) { best_cost = cost; best = PnMap{nrb, ncb, xc, rpg, cpg, 0}; }
    }
    // an XCD's slice of B does not fit its L2 (wide outputs): walk the row blocks of one column block first, so the
    // workgroups resident at any time share a few column blocks of B and each slice crosses the fabric once
    best.rfast = b_bytes / best.xc > (size_t)(3u << 19);
    return best;
}

// K-loop product: steps (32 columns each) per slab -- two 16-row images of 768 columns = 144 KB; 16-row blocks per fragment stream
// and column tiles per wave (measured at 512 / 128 rows: RB 4 T 1 192 / 55 us, RB 2 T 2 139 / 44, RB 4 T 2 166 / 57 with 55
// spilled registers)
constexpr int PN3_KLOOP_SLAB = 24;
constexpr int PN3_KLOOP_RB = 2, PN3_KLOOP_T = 2;
// parts of K for M rows and ntile tiles: enough workgroups for 256 CUs, ks x column blocks a multiple of 8 (XCD <-> slice of B), <= 64
inline int panel_gemm3_kloop_parts(int M, int ntile) {
    constexpr int rb = PN3_KLOOP_RB, T = PN3_KLOOP_T, wgs = 256;
    const int ncb = (ntile + 8 * T - 1) / (8 * T), nrp = (M + 16 * rb - 1) / (16 * rb);
    // r6: the LARGEST admissible part count that still fits one round of workgroups (a workgroup fills a CU's LDS: one per CU).  The
    // count used to be rounded UP to the next admissible one -- 288-336 workgroups at 96 / 192 / 320 / 384 / 448 rows, two rounds:
    // 141.8 us at 384 rows against 113.9 at 512 (tools/launch_times.py --config c5 sweep).
    int ks = std::min(64, std::max(1, wgs / (ncb * nrp)));
    while (ks > 1 && (ks * ncb) % 8 != 0) --ks;
    if ((ks * ncb) % 8 != 0) { ks = 1; while ((ks * ncb) % 8 != 0 && ks < 64) ++ks; }       // (nothing admissible below: the smallest above)
    return std::min(ks, 64);
}

// One plan for every product of the panel_gemm3_* family.  Template parameters the form implies: nw (F_PANEL3: waves per workgroup),
// T (F_PANEL3_KSW: column tiles per workgroup), cs (F_PANEL3_WIDE: column parts), ks (F_PANEL3_KLOOP: parts of K).
struct PanelPlan {
    Form form = F_NONE;
    int nw = 0, T = 0, cs = 0, ks = 0;
    int grid = 0, block = 0;
    size_t lds = 0;            // dynamic LDS bytes
    size_t max_lds = 0;        // != 0: the kernel's MaxDynamicSharedMemorySize attribute must be raised to this
    PnMap mp = {};             // F_PANEL3, F_PANEL3_KSW
    bool two_partials = false; // the product is left as two partial sums (the consumer adds them)
};

// C[M, N] = A[M, K] x B, all of K in one LDS image (the blend forward; the data gradient of small sets).  F_NONE: K too long.
inline PanelPlan plan_panel3(int M, int K, int ntile, int nst, int np, const FormSwitches& sw) {
    PanelPlan p;
    const int kpad = (K + 31) & ~31;
    if (kpad > PN3_MAX_K) return p;
    const size_t b_bytes = pn_b_bytes(np, ntile, nst);
    if (b_bytes > (size_t)(16u << 20) && M >= 32 && kpad <= 768) {
        // wide outputs: one workgroup per CU (the 98 KB image leaves room for one): as many column parts as it takes to reach 256
        // workgroups.  (r2-r4 ran one column part.  r5: two column tiles per wave, as in the K-loop product, measured no faster
        // here: 0.186 vs 0.179 ms at 1024 rows, equal at 512.  r6: 64 rows per workgroup -- half the fragment bytes per MFMA -- took
        // 70 us instead of 90 at 512 rows, yet made the config-5 fit 5 % slower: that configuration runs at the chip's power limit.)
        const int nrb = (M + 31) / 32, ncb = (ntile + 7) / 8, cpg = (ncb + 7) / 8;
        p.form = F_PANEL3_WIDE;
        p.cs = std::max(1, std::min(cpg, (256 + 8 * nrb - 1) / (8 * nrb)));
        p.grid = 8 * nrb * p.cs; p.block = 512; p.lds = pn_lds_bytes(np, kpad, 2);
        return p;
    }
    if ((sw.pn_rb2 == 1 || sw.pn_rb2 == 2) && M >= sw.clip_fwd_rows && kpad <= 768 && ntile >= 48) {
        // two row blocks per fragment stream (measured: 256 rows 50.2 vs 49.8 ms per step, 384 rows 56.7 vs 57.8).  (r5: six waves x
        // two tiles over the same 32 x 192 block -- half the LDS bytes per MFMA, the lever that took the K-loop product from 192 to
        // 139 us -- is SLOWER here: 14.4 vs 12.8 us; with K = 512 the twelve waves' latency hiding is worth more)
        p.form = F_PANEL3_RB2;
        p.grid = 8 * ((M + 31) / 32); p.block = 768; p.lds = pn_lds_bytes(np, kpad, 2);
        return p;
    }
    // waves per workgroup: eight while that gives >= 128 workgroups, else four (measured at 128 rows: forward 7.8 -> 6.6 us with four
    // waves; two waves stage too slowly)
    const int nrb = (M + 15) / 16;
    p.form = F_PANEL3;
    p.nw = 8;
    if (nrb * ((ntile + 7) / 8) < 128 && nrb * ((ntile + 3) / 4) >= 128) p.nw = 4;
    if (sw.pn_nw == 8 || sw.pn_nw == 4 || sw.pn_nw == 2) p.nw = sw.pn_nw;
    p.mp = panel_map(nrb, (ntile + p.nw - 1) / p.nw, (size_t)M * K * 4, b_bytes);
    p.grid = 8 * p.mp.rpg * p.mp.cpg; p.block = 64 * p.nw; p.lds = pn_lds_bytes(np, kpad, 1);
    return p;
}

// The blend product's data gradient dPF[M, N] = dV[M, K] x B (K = 3 x vertices).  may_split: the caller can take two partial sums.
inline PanelPlan plan_blend_backward(int M, int K, int ntile, int nst, int np, bool may_split, const FormSwitches& sw) {
    PanelPlan p;
    const int kpad = (K + 31) & ~31, nst_all = (K + 31) >> 5;
    // clip sizes: each workgroup takes HALF of K for two row blocks; N <= 32 tiles, half of K <= 768 columns (K <= 1536)
    if (may_split && (sw.pn_rb2 == 1 || sw.pn_rb2 == 3) && M >= sw.clip_kgrad_rows && ntile <= 32 && nst_all >= 2 &&
        32 * ((nst_all + 1) / 2) <= 768) {
        p.form = F_PANEL3_RB2K;
        p.two_partials = true;
        p.grid = 8 * ((M + 31) / 32); p.block = 512; p.lds = pn_lds_bytes(np, 32 * ((nst_all + 1) / 2), 2);
        return p;
    }
    // r6: the K-loop form also where one LDS image would still fit, from K = 1664 at clip sizes and K = 1904 from 192 rows -- contact
    // sets of 560-840 vertices ran the one-image forms at 17-35 us where the K-loop form takes 14-21 (tools/launch_times.py
    // --per-leg 280 / 320 / 375 / 420 at 1024 / 512 / 256 / 128 rows; at 128 rows the one-image forms stay ahead).
    constexpr int kmin = 1664;
    const bool big_k = (M >= 384 && K >= kmin) || (M >= 192 && K >= kmin + 240);
    // K split over the eight waves of a workgroup: when a long K sits in one LDS image and there are few row blocks
    if (!big_k && sw.pn_ksw && kpad <= PN3_MAX_K && kpad >= 768 && ((M + 15) / 16) * ((ntile + 7) / 8) < 128) {
        // column tiles per workgroup: two while that still gives >= 192 workgroups, else one -- r6: and two whenever one tile per
        // workgroup would mean more workgroups than CUs (one workgroup fits a CU: 129-176 rows ran in two rounds, 14.7 us at 160 rows
        // against 8.8 at 128 and 9.5 at 192: tools/launch_times.py sweep)
        const int nrb = (M + 15) / 16;
        p.form = F_PANEL3_KSW;
        p.T = (nrb * ((ntile + 1) / 2) >= 192 || nrb * ntile > 256) ? 2 : 1;
        p.mp = panel_map(nrb, (ntile + p.T - 1) / p.T, (size_t)M * K * 4, pn_b_bytes(np, ntile, nst));
        p.grid = 8 * p.mp.rpg * p.mp.cpg; p.block = 512; p.lds = pn_lds_bytes(np, kpad, 1);
        p.max_lds = pn_lds_bytes(np, PN3_MAX_K, 1);
        return p;
    }
    if (!big_k && panel_gemm3_fits(K)) return plan_panel3(M, K, ntile, nst, np, sw);
    // K far beyond any LDS image (the FULL mesh's data gradient, K = 3 V = 31 425), or big_k: K in `ks` parts, a partial product each
    constexpr int rb = PN3_KLOOP_RB, T = PN3_KLOOP_T;
    p.form = F_PANEL3_KLOOP;
    p.ks = panel_gemm3_kloop_parts(M, ntile);
    p.grid = p.ks * ((ntile + 8 * T - 1) / (8 * T)) * ((M + 16 * rb - 1) / (16 * rb)); p.block = 512;
    p.lds = pn_lds_bytes(np, 32 * PN3_KLOOP_SLAB, rb);
    p.max_lds = 150 * 1024;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------
// Contact forward: the blend product and the skinning in one launch (blend_skin_fwd_kernel) at clip sizes, else two launches
// (the blend product by plan_panel3, then skin_fwd_kernel)
inline size_t blend_skin_lds_bytes(int np, int kfeat, int ja) {
    return pn_lds_bytes(np, (kfeat + 31) & ~31, 2) + (size_t)(32 * ja * 12 + 32 * 12 + 32 * 4 + 2 * 64 * 4 + 3 * 32 * 64) * sizeof(float);
}
struct ContactFwdPlan { Form form = F_SKIN_FWD; int grid = 0, grid_y = 1, block = 0; size_t lds = 0, max_lds = 0; };
// permuted_panel / vpack: the set has the permuted forward operand / the packed vertex layout (sets of <= 512 vertices, K <= 4 weights)
inline ContactFwdPlan plan_contact_forward(int nl, int nc, int kfeat, int np, bool blend_done, bool permuted_panel, bool vpack, int K, int ja_hi,
                                           const FormSwitches& sw) {
    ContactFwdPlan p;
    if (!blend_done && sw.fuse_skin && sw.gemm_split3 && permuted_panel && vpack && K <= 4 && nl >= sw.clip_fwd_rows &&
        blend_skin_lds_bytes(np, kfeat, ja_hi) <= (size_t)150 * 1024) {
        p.form = F_BLEND_SKIN_FWD;
        p.grid = 8 * ((nl + 31) / 32); p.block = 768; p.lds = blend_skin_lds_bytes(np, kfeat, ja_hi); p.max_lds = 150 * 1024;
        return p;
    }
    p.grid = (nc + 255) / 256; p.grid_y = nl; p.block = 256;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------
// Skinning backward (fdc_k_skin.h)
constexpr int SKB_VCH = 1024;                  // vertices per LDS chunk of skin_bwd_kernel
constexpr int SKB_ROW = 6;                     // floats per vertex of the factored dT rows (matrix-form dA): gv[3] | vp[3]
constexpr int SKS_MAXV = 1024, SKS_MAXNNZ = 6144;      // reach of the contact-set kernels (skin_bwd_small_kernel)
struct SkinBwdPlan {
    Form form = F_NONE;
    int G = 0;                 // F_SKIN_BWD_VEC: weight groups per vertex
    int vpt = 0, kc = 0;       // F_SKIN_BWD_SMALL[_K]: skin_bwd_small_kernel<vpt, kc>
    int nch = 1;               // F_SKIN_BWD_CHUNKS_*: chunks of SKB_VCH vertices (grid y)
    int grid = 0, block = 256;
    size_t lds = 0;
    bool ja_rows = false;      // the kernel writes only the first ja_hi joints' rows of dA
};
// skin_bwd_kernel for any vertex set: one workgroup per frame up to a chunk of vertices, the split form + its reduction beyond.
// mfma_da: the set has the weights as MFMA fragments (sets of more than 512 vertices).
inline SkinBwdPlan plan_skin_bwd_any(int nrows, int nc, bool mfma_da) {
    SkinBwdPlan p;
    // dT rows: 12 floats per vertex for the list form; the matrix form keeps them factored (SKB_ROW = 6 floats) and reuses the space
    // for its four waves' partial tiles (16 KB: more than 512 vertices of rows, which is when the matrix form is built)
    p.lds = mfma_da ? std::max((size_t)std::min(nc, SKB_VCH) * SKB_ROW, (size_t)4 * 64 * 16) * sizeof(float)
                    : (size_t)std::min(nc, SKB_VCH) * 12 * sizeof(float);
    p.grid = nrows;
    if (nc <= SKB_VCH) { p.form = F_SKIN_BWD_FRAME; return p; }
    p.nch = (nc + SKB_VCH - 1) / SKB_VCH;
    p.form = mfma_da ? F_SKIN_BWD_CHUNKS_MFMA : F_SKIN_BWD_CHUNKS_LIST;
    return p;
}
// ... of the optimiser's contact set (nnz skinning weights, K per vertex).  vpack / csc_v16: the packed layouts exist; aligned16: Vw,
// Voff, dVoff and A are 16-byte aligned.
inline SkinBwdPlan plan_contact_skin_bwd(int nl, int nc, int nnz, int K, bool vpack, bool csc_v16, bool aligned16, bool mfma_da, bool skin_vec) {
    const size_t lds_small = (size_t)6 * nc * sizeof(float) + (size_t)nnz * sizeof(float) + (((size_t)nnz * 2 + 15) & ~(size_t)15);
    if (!(nc <= SKS_MAXV && nnz <= SKS_MAXNNZ && lds_small <= 57000)) return plan_skin_bwd_any(nl, nc, mfma_da);   // (+ 6.4 KB of static LDS <= 64 KB)
    SkinBwdPlan p;
    p.grid = nl; p.lds = lds_small; p.ja_rows = true;
    const int G = (K + 3) / 4;                           // weight groups per vertex: the packed layout covers K <= 12
    const size_t ldsv = (size_t)9 * nc * sizeof(float) + (size_t)((nnz + 3) & ~3) * sizeof(float) + (size_t)((nnz + 7) & ~7) * 2;
    if (skin_vec && nc <= 512 && G <= 3 && nnz <= 2048 * G && ldsv <= 60000 && (nc & 3) == 0 && vpack && csc_v16 && aligned16) {
        p.form = F_SKIN_BWD_VEC; p.G = G; p.lds = ldsv;
        return p;
    }
    // VPT vertices and KC weight-list entries per thread in registers (130 VGPRs for 4 / 16 cost a wave per SIMD: the loop's 500
    // vertices / 2000 weights take the 2 / 8 instance)
    p.form = F_SKIN_BWD_SMALL;
    if (nc <= 512 && nnz <= 2048) { p.vpt = 2; p.kc = 8; }
    else if (nc <= 512) { p.form = F_SKIN_BWD_SMALL_K; p.vpt = 2; p.kc = 24; }   // (K > 4 at the loop's contact-set size: up to 6144 list entries)
    else if (nnz <= 4096) { p.vpt = 4; p.kc = 16; }
    else { p.vpt = 4; p.kc = 24; }
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------
// Nearest-neighbour search (fdc_chamfer.h)
#ifndef FDC_MF_CH
#define FDC_MF_CH 512
#endif
constexpr int MF_CH = FDC_MF_CH;       // scene points per chunk of the MFMA scans = one k-d cell = culling granularity
constexpr int MF_MAXCHUNK = 2048;      // chunks per split the survivor list can hold (host keeps splits below it)
constexpr FDC_FORMS_HD int nn_split_len(int nt, int nsplit) {
    return ((nt + nsplit - 1) / nsplit + MF_CH - 1) / MF_CH * MF_CH;      // chunk-aligned so bounds[] indexes uniformly
}
constexpr int nn_grid_blocks(int qblocks, int nsplit) { return (qblocks + 7) / 8 * 8 * nsplit; }
// mode (fdcap_set_nn_kernel): 0 = by size (MFMA-filtered for non-trivial sizes), 1 = plain VALU scan, 2 = MFMA-filtered
constexpr bool nn_use_mfma(int nq, int nt, int mode) { return mode == 1 ? false : mode == 2 ? true : (long long)nq * nt >= (1LL << 22); }
inline int nn_pick_nsplit(int nq, int nt, bool culled = false) {
    // Each split re-reads the queries / seeds and writes its own partial minima, so fewer, longer
    // splits win once there are enough query blocks to occupy 256 CUs x 3 resident workgroups.
    // Measured on 1024 frames x 500 contacts vs 500k points: brute-force scan nsplit 2 (9.7 ms) beats
    // 1 (11.1) and 8 (9.9); seeded + chunk-culled scan nsplit 1 (1.09 ms) beats 2 (1.23) and 4 (1.43).
    int qblocks = culled ? (nq + 255) / 256 : (nq + 511) / 512;
    int ns = 1;
    const int target = culled ? 1536 : 1024;
    while (qblocks * ns < target && ns < 64 && nt / (ns * 2) >= 4 * MF_CH) ns *= 2;
    if (!culled && qblocks >= 512 && nt >= 8 * MF_CH) ns = std::max(ns, 2);
    while (nn_split_len(nt, ns) / MF_CH > MF_MAXCHUNK) ns *= 2;
    return ns;
}
// The streaming search's per-query box tests (nn_box_stage, fdc_chamfer.h): a pass gives each of up to 64 / LPB listed boxes LPB
// lanes, and each of them walks 32 / LPB of the group's 32 queries.  r3 fixed LPB = 2 for kept lists of ~22 quarters; since the
// queries are sorted by their neighbour's k-d quarter (r7) a steady filter list of a config-3 fit holds 11.8 quarters on average,
// at most 16 in 92 % of the stages (profiles/r15_nn_list_lengths.txt), and a pair per box left most of the wave idle for 16 iterations.  Lanes per box by the wave-uniform count n of a stage: the widest form that still takes the
// whole stage in one pass.  forced in {2, 4, 8} overrides (FDCAP_NN_BOX_LANES; longer stages then take several passes).
constexpr FDC_FORMS_HD int nn_box_lanes(int n, int forced) {
    return (forced == 2 || forced == 4 || forced == 8) ? forced : n <= 8 ? 8 : n <= 16 ? 4 : 2;
}
// The wave's ballot of such a pass (bit l: lane l's share of the queries met its box) -> bit lpb * e set iff any of entry e's lpb
// lanes hit; every other bit clear.  lpb in {2, 4, 8}.
constexpr FDC_FORMS_HD unsigned long long nn_box_fold(unsigned long long hits, int lpb) {
    hits |= hits >> 1;
    if (lpb >= 4) hits |= hits >> 2;
    if (lpb >= 8) hits |= hits >> 4;
    return hits & (lpb == 2 ? 0x5555555555555555ull : lpb == 4 ? 0x1111111111111111ull : 0x0101010101010101ull);
}
// ... and where the entry led by `lane` (lane % lpb == 0, its bit set in `folded`) lands among the pass's kept entries: they are
// written in ascending entry order.  nn_box_count: how many the pass keeps.
FDC_FORMS_HD inline int nn_box_rank(unsigned long long folded, int lane) { return __builtin_popcountll(folded & ((1ull << lane) - 1ull)); }
FDC_FORMS_HD inline int nn_box_count(unsigned long long folded) { return __builtin_popcountll(folded); }

// r18.  When the streaming search's query order is rebuilt (fdc_chamfer.h NNOrder, nn_stream_upkeep): the period, in search
// launches, that follows the fit's `rebuilds`-th rebuild (1: the one after the seeding launch) of an order over nq queries.  base
// is FDCAP_NN_ORDER; 0: off.  A rebuild costs about 80 us at 512 k queries (six sort launches 57, the launch-order sort 13, the next
// search launch's dropped lists 10) and pays only while the neighbours still move between quarters: on a config-3 fit a fixed
// period of 128 loses to 32 only in launches 25-125 (+0.9 .. +3.4 us per launch, 240 us in all), 64 to 32 only in launches 25-75,
// and from launch 130 on 32, 64 and 128 run the same launches within 1 us (profiles/r18_search_upkeep_ab.txt).  So the first
// NN_PERIOD_HOLD rebuilds keep the base period -- about a hundred launches at the default 32 -- and every later one doubles it, up
// to NN_PERIOD_MAX.  A shorter first period gained nothing (16 against 32 over launches 1-100: 51.3 / 51.3 us per launch), so
// there is none.  The rule knows the rebuild count alone, not the fit's length.  Never decreasing in `rebuilds`; a base above
// NN_PERIOD_MAX stays as given.
// The rule is open-loop: the host enqueues a whole fit ahead of the device and cannot see how far the bodies still move.  What a
// skipped rebuild saves is a rebuild (60-100 us up to 2 M queries); what a stale order can cost grows with the search launch.
// Config 5 (5.36 M queries, 0.6 ms per launch) still moves its bodies by centimetres in launches 100-300, and there the growing
// period LOSES: launches 200-300 ran 549-771 us against 436-627 under the fixed 32, 2.8 % of the step.  With config 3's body and
// scene the growing period wins at 128 k, 150 k, 512 k, 1.02 M and 2.05 M queries (search launch unchanged or faster, 7 rebuilds
// fewer).  So it is taken up to NN_PERIOD_GROW_MAX_QUERIES, the largest size it was measured to win at; above, the fixed base.
// -DFDC_NN_PERIOD_GROWTH=0 (A/B): the fixed period of every build before r18.
#ifndef FDC_NN_PERIOD_GROWTH
#define FDC_NN_PERIOD_GROWTH 1
#endif
constexpr int NN_PERIOD_HOLD = 3, NN_PERIOD_MAX = 128, NN_PERIOD_GROW_MAX_QUERIES = 1 << 21;
constexpr FDC_FORMS_HD int nn_order_period(int base, int rebuilds, int nq) {
    if (base <= 0) return 0;
    int p = base;
    if (FDC_NN_PERIOD_GROWTH && nq <= NN_PERIOD_GROW_MAX_QUERIES)
        for (int r = NN_PERIOD_HOLD; r < rebuilds && p < NN_PERIOD_MAX; ++r) p = 2 * p < NN_PERIOD_MAX ? 2 * p : NN_PERIOD_MAX;
    return p;
}

// r21.  The query order's key is the k-d node of each query's current neighbour: its position in a sorted scene of ns points,
// shifted down by this.  5 is the 32-point MFMA tile, the unit the main loop scores; the two 8-bit radix passes hold 16 bits and
// 0xFFFF stays the no-neighbour sentinel, so the finest of tile (5), 64-point node (6) and quarter (7) whose last key stays below
// it: 5 up to 2 097 120 points (both bench scenes), 6 up to 4 194 240, 7 beyond (where the far end of the scene clamps onto the sentinel, as before).
constexpr int NN_KEY_SHIFT_MIN = 5, NN_KEY_SHIFT_MAX = 7;
constexpr FDC_FORMS_HD int nn_order_key_shift(int ns) {
    int s = NN_KEY_SHIFT_MIN;
    while (s < NN_KEY_SHIFT_MAX && ((ns > 0 ? ns - 1 : 0) >> s) >= 0xFFFF) ++s;
    return s;
}

// r21.  Work items of the one-wave streaming form: ipc per 512-point chunk -- 4 quarters (128 points) or 8 eighths (64 points).
// A work list holds 16-bit ids ipc * chunk + item, so eighths are taken while 8 * nchunk <= 0xFFFF (8191 chunks, 4.19 M points);
// larger scenes keep quarters, as every other form does.  eighths: the scene has their boxes (behind NNTarget::qbounds).
// Eighths cut the tiles a wave scores by a third (config 3: 18.5 -> 12.7 per wave) and lengthen its lists by 60 % (10.5 -> 17
// listed, 4.7 -> 6.3 scanned items): they pay where a launch is bound by what its waves score, not by a wave's set-up chain.  With
// config 3's body and scene, us per launch, quarters / eighths: 512 k queries 42.9 / 43.5, 1.02 M 68.6 / 69.0, 2.05 M 125.6 / 127.7,
// 4.1 M 300.5 / 281.9; config 5 (5.36 M) 571.8 / 531.8 and 408.5 -> 392.1 ms per step (profiles/r21_search_items_ab.txt).  So
// eighths are taken above NN_ITEMS8_MIN_QUERIES, the largest size they were measured to lose at; the crossing lies between 2.05 M
// and 4.1 M queries.  forced: 0 automatic, 4 or 8 as fdcap_debug_nn_search_form asked -- 8 still only where the ids fit.
constexpr int NN_ITEM_ID_MAX = 0xFFFF, NN_ITEMS8_MIN_QUERIES = 1 << 21;
constexpr FDC_FORMS_HD int plan_nn_items_per_chunk(int nq, int nchunk, bool eighths, int forced) {
    return eighths && forced != 4 && 8LL * nchunk <= NN_ITEM_ID_MAX && (forced == 8 || nq > NN_ITEMS8_MIN_QUERIES) ? 8 : 4;
}
// (ipc is 4 or 8: shifts and masks, the kernel's own arithmetic)
constexpr FDC_FORMS_HD int nn_item_id(int ipc, int chunk, int item) { return ipc * chunk + item; }
constexpr FDC_FORMS_HD int nn_item_chunk(int ipc, int id) { return id >> (ipc == 8 ? 3 : 2); }
constexpr FDC_FORMS_HD int nn_item_of(int ipc, int id) { return id & (ipc - 1); }

struct NNPlan {
    Form form = F_NN_DIRECT;
    int wpg = 0;               // F_NN_STREAM_*: waves per group of 32 queries
    int nq_blocks = 0;         // F_NN_MFMA: query blocks of 32 per wave (nn_mfma_kernel<2> / <4>)
    int groups = 0;            // F_NN_STREAM_*: groups of 32 queries
    int grid = 0, block = 256;
};
// culled: seeds + chunk boxes are there; frags: the scene has precomputed fragments; seed_in_place: the seeds are the last results
// (seed == idx) and their coordinates are kept.  nsplit: the scene splits the caller sized its partial buffers for (nn_pick_nsplit).
inline NNPlan plan_nn_search(int nq, int nt, bool culled, bool frags, bool seed_in_place, int nsplit, int mode, const FormSwitches& sw) {
    NNPlan p;
    const bool mfma = nn_use_mfma(nq, nt, mode);
    // (the streaming kernel's work list holds 16-bit ids 4 k + quarter: scenes up to 16384 chunks = 8.4 M points; beyond, the staged kernel)
    if (culled && frags && sw.nn_stream != 0 && mfma && seed_in_place && (nt + MF_CH - 1) / MF_CH <= 16384) {
        p.groups = (nq + 31) / 32;
        if (sw.nn_stream < 0) {
            // enough waves to fill 1024 SIMDs x 4 twice over, no more (the per-group setup is repeated by every wave of the group).
            // (Groups of 64 queries, two query blocks per wave, lost: 92.2 vs 78.2 ms per step.)  Measured (1024 / 512 / 256 / 128
            // frames x 500 queries): 11: 0.139 / 0.095 / 0.054 / 0.072 ms, 21: 0.140 / 0.087 / 0.049 / 0.047, 41: 0.153 / 0.086 /
            // 0.047 / 0.036.  r6 sweep (tools/launch_times.py at 64 .. 224 frames x 500 queries, us per launch; waves per group 1 / 2 /
            // 4): 2000 groups 25.8 / 23.7 / 22.7, 2500: 25.1 / 24.2 / 25.5, 3000: 25.8 / 26.8 / 28.7, 3500: 24.1 / 26.9 / 30.1
            // (3072 / 4 until r6).  Re-measured with quarter work items: 128 / 256 / 512 / 768 frames: 11: 0.036 / 0.033 / 0.057 /
            // 0.068 ms, 21: 0.028 / 0.034 / 0.059 / 0.074, 41: 0.024 / 0.036 / 0.063 / 0.084
            p.wpg = p.groups >= 2816 ? 1 : p.groups >= 2304 ? 2 : 4;
        } else {
            p.wpg = (sw.nn_stream / 10 == 4) ? 4 : (sw.nn_stream / 10 == 2) ? 2 : 1;
        }
        // one-wave groups run as one-wave workgroups (a workgroup's slot is only handed on when its slowest wave is done)
        const int wpb = p.wpg == 1 ? 1 : 4;
        p.form = p.wpg == 4 ? F_NN_STREAM_W4 : p.wpg == 2 ? F_NN_STREAM_W2 : F_NN_STREAM_W1;
        p.grid = ((p.groups * p.wpg + wpb - 1) / wpb + 7) / 8 * 8; p.block = 64 * wpb;
        return p;
    }
    // Query blocks per workgroup: 4 waves x NQ x 32.  A brute-force scan wants NQ = 4 (most MFMAs per staged chunk: 9.7 ms vs 10.9 at
    // NQ = 2); a seeded + chunk-culled scan wants NQ = 2 (the union of the chunks 256 queries need is smaller than what 512 need,
    // twice the workgroups: 0.92 ms vs 1.10 ms at NQ = 4, 1.09 ms at NQ = 1).
    if (mfma) { p.form = F_NN_MFMA; p.nq_blocks = culled ? 2 : 4; }
    p.grid = nn_grid_blocks(mfma && culled ? (nq + 255) / 256 : (nq + 511) / 512, nsplit);
    return p;
}

// The in-loop search of a batch of clips of several scenes (fdc_clips.h: segments, each with its own scene, queries and pruning
// state).  The plain form -- the specification -- is one nn_search launch set per segment, in segment order.  When the LARGEST
// segment's own plan is the one-wave streaming form, all segments go through that form in ONE launch instead
// (nn_stream4_kernel<1, 1, true>: blockIdx.y the segment, grid.x the largest segment's groups; a smaller segment's surplus
// workgroups return at once).  Smaller segments then take the one-wave form too where their own size would pick two or four waves
// per group -- results never depend on the form.  Not taken: with FDCAP_NN_SEGMENTS=loop, for one segment (today's launch), for
// more segments than the kernel argument holds, and whenever some segment cannot stream at all (its plan is a staged scan).
// seg_nq / seg_nt [nseg]: each segment's queries and scene points; the other arguments as plan_nn_search takes them.
constexpr int NN_MAX_SEGS = 16;                  // segment descriptors in the kernel argument (152 B each)
struct NNSegPlan {
    bool one_launch = false;
    const char* name = nullptr;                   // what fdcap_debug_kernel_forms reports for the one launch (the plain form reports each segment's own)
    int grid_x = 0, grid_y = 0, block = 64;
};
inline NNSegPlan plan_nn_segments(int nseg, const int* seg_nq, const int* seg_nt, bool culled, bool frags, bool seed_in_place, int nsplit, int mode,
                                  const FormSwitches& sw) {
    NNSegPlan p;
    if (nseg < 2 || nseg > NN_MAX_SEGS || sw.nn_segments_loop) return p;
    int big = 0;
    for (int s = 0; s < nseg; ++s) {
        if (seg_nq[s] > seg_nq[big]) big = s;
        if (plan_nn_search(seg_nq[s], seg_nt[s], culled, frags, seed_in_place, nsplit, mode, sw).wpg == 0) return p;
    }
    const NNPlan pl = plan_nn_search(seg_nq[big], seg_nt[big], culled, frags, seed_in_place, nsplit, mode, sw);
    if (pl.form != F_NN_STREAM_W1) return p;
    p.one_launch = true;
    p.name = "nn_stream4_kernel(1 wave per group, segments)";
    p.grid_x = pl.grid; p.grid_y = nseg; p.block = pl.block;
    return p;
}

// The every-pair search with a batch axis (fdcap_chamfer_fwd: per-batch targets, the reverse direction): B independent searches of
// nq queries against nt targets in one launch set, the batch on blockIdx.y in chunks of at most NN_MAX_GRID_Y.  The kernel is the
// one a single batch's sizes select (nn_use_mfma(nq, nt)), so a batch is scanned by the kernel the per-batch loop gives it; both
// kernels serve 512 queries per workgroup (nn_direct_kernel<2>, nn_mfma_kernel<4>).  grid_x = query blocks x splits, no padding to
// the XCD count (the batch axis supplies the workgroups).  nsplit: as nn_pick_nsplit for the B * qblocks query blocks the launch
// has -- results do not depend on it ((d, index) merge).  Partial minima: [batch][split][query].
constexpr int NN_MAX_GRID_Y = 65535;
struct NNBatchPlan {
    bool mfma = false;
    const char* name = "nn_direct_batched";       // what fdcap_debug_kernel_forms reports
    int nsplit = 1, qblocks = 1, grid_x = 1, block = 256;
    int launches = 1;                              // ceil(B / NN_MAX_GRID_Y)
};
inline NNBatchPlan plan_nn_batched(int nq, int nt, int B, int mode) {
    NNBatchPlan p;
    p.mfma = nn_use_mfma(nq, nt, mode);
    p.name = p.mfma ? "nn_mfma_batched" : "nn_direct_batched";
    p.qblocks = (int)(((long long)nq + 511) / 512);
    const long long flat = std::min<long long>((long long)p.qblocks * 512 * B, 1LL << 30);
    p.nsplit = nn_pick_nsplit((int)flat, nt);
    p.grid_x = p.qblocks * p.nsplit;
    p.launches = (B + NN_MAX_GRID_Y - 1) / NN_MAX_GRID_Y;
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------
// Pose kernels (fdc_frame.h, fdc_k_pose.h): the joints one launch's loss can reach.  The loss meets the kinematic chain through the
// skinning transforms A of the joints the contact set is skinned to (rows below SkinModel::ja_hi) and through the world positions of
// the first POSE_NJW joints; the local rotations of all joints are needed whenever the pose feature PF is written.
//   joints [0, jn) need their world transform (chain, G, A, rest position), joints [0, jr) their local rotation,
//   nlev = 1 + the deepest level among [0, jn).
// The prefix form needs parents[j] < j below jn (SMPL-X numbers its joints that way); else, and with trim = false
// (FDCAP_POSE_TRIM=0: the reference the tests compare against), the plan is the full one.
constexpr int POSE_NJ = 55, POSE_NJW = 23;
struct PoseJoints {
    int jn = POSE_NJ, jr = POSE_NJ, nlev = -1;     // nlev < 0: every level of the tree (pose_forward / pose_backward take it so)
    bool world = true;                             // the world joints Jw are written
};
// body_joints: the loss also reads the posed body-frame joints 0 .. POSE_NJW - 1 (the clip-level reprojection term,
// fdcap_opt_set_reproj): jn >= POSE_NJW in every iteration, whether or not the world joints are written (`world` and jr are as without it).
inline PoseJoints plan_pose_joints(const int* parents, const int* depth, int ja_hi, bool contact_state, bool need_world, bool trim = true,
                                   bool body_joints = false) {
    PoseJoints p;                                  // the full plan: what every launch was before the sets existed
    p.nlev = 0;
    for (int j = 0; j < POSE_NJ; ++j) p.nlev = std::max(p.nlev, depth[j] + 1);
    if (!trim) return p;
    const int jn = std::min(POSE_NJ, std::max(1, std::max(contact_state ? ja_hi : 0, (need_world || body_joints) ? POSE_NJW : 0)));
    if (jn == POSE_NJ) return p;                   // (every vertex a contact: the identical launch)
    for (int j = 0; j < jn; ++j) if (parents[j] >= j) return p;
    p.jn = jn;
    p.jr = contact_state ? POSE_NJ : jn;           // (PF is written with the contact state: the blend product reads every pose feature)
    p.world = need_world;
    p.nlev = 0;
    for (int j = 0; j < jn; ++j) p.nlev = std::max(p.nlev, depth[j] + 1);
    return p;
}

// ---------------------------------------------------------------------------------------------------------------------
// VPoser decoder (forward and data gradient): the split-plane kernels, or the exact-fp32 ones
inline Form plan_decoder(bool gemm_split3) { return gemm_split3 ? F_VPOSER_SPLIT : F_VPOSER_FP32; }

}  // namespace fdc
