// A batch of clips of DIFFERENT lengths (fdcap_opt_create_clips_var): which clip a row belongs to, where in it, and with which
// normalised loss weights -- as pure host functions, no HIP types.  Compiles with plain g++ -std=c++17
// (tests/test_ragged_clips_cpu.py pins the table against numpy float32 evaluations of the same expressions) and with hipcc.
//
// Clip k of lengths n_0 .. n_{K-1} owns buffer rows 2 + s_k .. 2 + s_k + n_k, s_k = n_0 + .. + n_{k-1} (two halo rows on either
// side of the batch, as for one clip).  A batch of equal lengths never builds this table: its kernels find a row's clip by
// arithmetic on the one length (clip_of_row, fdc_loss.h).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#if defined(__HIPCC__)
#define FDC_CLIPS_HD __host__ __device__
#else
#define FDC_CLIPS_HD
#endif

namespace fdc {

constexpr int CLIP_XDIM = 78;      // = XDIM (fdc_frame.h; asserted where both are visible)
constexpr int CLIP_NJW = 23;       // = NJW

// weights of the loss total of one iteration (multipliers of the lossconfig weights, :570 / :582 / :620)
struct LossWeights { float rec, smooth, contact, world, dct; bool world_on; };

// The four weights a clip of n frames puts in front of its un-normalised sums: the means' denominators are the clip's OWN frame
// count.  These are the float expressions every fit uses (a stand-alone fit evaluates them with n = its clip length), so a clip
// of a batch gets the bits of its stand-alone fit.
struct ClipWeights { float w_rec, w_sm, w_ws, coef; };
inline ClipWeights clip_weights(int n, const LossWeights& lw, float weight_loss_rec, float weight_contact, int nc) {
    ClipWeights w;
    w.w_rec = lw.rec * weight_loss_rec / ((float)n * CLIP_XDIM);
    w.w_sm = (n >= 3) ? lw.smooth / ((float)(n - 2) * CLIP_XDIM) : 0.f;                          // no second difference below three frames
    w.w_ws = (lw.world_on && n >= 2) ? lw.world / ((float)(n - 1) * CLIP_NJW * 3) : 0.f;         // no first difference below two
    w.coef = nc > 0 ? lw.contact * weight_contact / ((float)n * nc) : 0.f;                       // (ContactGradIn::coef)
    return w;
}

// Mode 'local', second loop (cal_loss2, global_optimization.py:536-556): its loss total has no phases and no lossconfig multipliers but
// weight_loss_rec -- l_rec + the parameter-space second difference + the VERTEX-space second difference over all nv3 = 3 V
// coordinates + the foot-skate term -- so its weights are a set of their own, never the phase-1 or phase-2 ones.  These are the
// float expressions fdcap_opt_backward_local2 evaluates for a stand-alone fit of n frames.  In the returned ClipWeights (and in
// the records built from it) w_ws carries the vertex-space weight 1 / ((n - 2) nv3) -- this loop has no world-joint term -- and
// coef is zero (the contact term is the foot-skate one, below).
inline ClipWeights clip_weights_local2(int n, float weight_loss_rec, size_t nv3) {
    ClipWeights w;
    w.w_rec = weight_loss_rec / ((float)n * CLIP_XDIM);
    w.w_sm = (n >= 3) ? 1.f / ((float)(n - 2) * CLIP_XDIM) : 0.f;                                // no second difference below three frames
    w.w_ws = (n >= 3) ? 1.f / ((float)(n - 2) * (float)nv3) : 0.f;
    w.coef = 0.f;
    return w;
}
// ... and the foot-skate term's 1 / ((n - 1) npart 3) of one contact part of npart vertices (:415-429; foot_skate_kernel evaluates
// it per thread): a mean over the n - 1 first differences, so zero below two frames
FDC_CLIPS_HD inline float clip_foot_skate_inv(int n, int npart) {
    return (n >= 2) ? 1.f / ((float)(n - 1) * (float)npart * 3.f) : 0.f;
}

// What a per-frame kernel needs to know about its row, in ONE 32-byte record (one scalar load, requested with the kernel's first
// batch of loads; a row -> clip -> weights chain would be three dependent round trips): clip index k (selects scale[k]), index
// within the clip g, the clip's length n (the stencils' extent), and the clip's four weights.
struct ClipRow { int32_t k, g, n; float w_rec, w_sm, w_ws, coef; int32_t pad; };
static_assert(sizeof(ClipRow) == 32, "one s_load_dwordx8 per row");

// lengths that make a batch: every one positive, their sum what the caller's config says and within `max_rows`
inline bool clip_lengths_ok(int32_t n_clips, const int32_t* len, int64_t want_total, int64_t max_rows) {
    if (n_clips < 1 || !len) return false;
    int64_t sum = 0;
    for (int32_t k = 0; k < n_clips; ++k) {
        if (len[k] <= 0) return false;
        sum += len[k];
        if (sum > max_rows) return false;
    }
    return sum == want_total;
}
inline bool clip_lengths_equal(int32_t n_clips, const int32_t* len) {
    for (int32_t k = 1; k < n_clips; ++k) if (len[k] != len[0]) return false;
    return true;
}

// starts [K + 1]: s_0 = 0 .. s_K = the batch's rows
inline std::vector<int32_t> clip_starts(int32_t n_clips, const int32_t* len) {
    std::vector<int32_t> s((size_t)n_clips + 1, 0);
    for (int32_t k = 0; k < n_clips; ++k) s[(size_t)k + 1] = s[(size_t)k] + len[k];
    return s;
}

// [rows + 4] records indexed by BUFFER row.  The halo rows (no frame of any clip) carry the neighbouring clip's index, so that a
// kernel that covers them reads a valid `scale`, with n = 0 and zero weights: every stencil test fails and every term is zero.
// (w: one ClipWeights per clip)
inline std::vector<ClipRow> clip_rows_fill(int32_t n_clips, const int32_t* len, const std::vector<ClipWeights>& w) {
    const std::vector<int32_t> s = clip_starts(n_clips, len);
    std::vector<ClipRow> rows((size_t)s[(size_t)n_clips] + 4);
    const ClipRow halo_lo = {0, 0, 0, 0.f, 0.f, 0.f, 0.f, 0}, halo_hi = {n_clips - 1, 0, 0, 0.f, 0.f, 0.f, 0.f, 0};
    rows[0] = rows[1] = halo_lo;
    rows[rows.size() - 2] = rows[rows.size() - 1] = halo_hi;
    for (int32_t k = 0; k < n_clips; ++k)
        for (int32_t g = 0; g < len[k]; ++g)
            rows[(size_t)2 + s[(size_t)k] + g] = ClipRow{k, g, len[k], w[(size_t)k].w_rec, w[(size_t)k].w_sm, w[(size_t)k].w_ws, w[(size_t)k].coef, 0};
    return rows;
}
inline std::vector<ClipRow> clip_rows_build(int32_t n_clips, const int32_t* len, const LossWeights& lw, float weight_loss_rec,
                                            float weight_contact, int nc) {
    std::vector<ClipWeights> w;
    for (int32_t k = 0; k < n_clips; ++k) w.push_back(clip_weights(len[k], lw, weight_loss_rec, weight_contact, nc));
    return clip_rows_fill(n_clips, len, w);
}
// the same records under the weights of mode 'local''s second loop (clip_weights_local2: w_ws is the vertex-space weight there)
inline std::vector<ClipRow> clip_rows_build_local2(int32_t n_clips, const int32_t* len, float weight_loss_rec, size_t nv3) {
    std::vector<ClipWeights> w;
    for (int32_t k = 0; k < n_clips; ++k) w.push_back(clip_weights_local2(len[k], weight_loss_rec, nv3));
    return clip_rows_fill(n_clips, len, w);
}

// ---- clips of different scenes (fdcap_opt_create_clips_scenes) ------------------------------------------------------------------
// Clip k names the registered scene slot clip_scene[k].  A SEGMENT is a maximal run of adjacent clips of one slot (a slot may come
// back: A, B, A are three segments); only the Chamfer search knows segments -- its pruning state (kept lists, launch order, query
// order, seeds) is cut along them, and each searches its own scene.  Everything per query (dist, idx, seedpt) stays flat.
constexpr int CLIP_MAX_SCENES = 8;     // = FDCAP_MAX_SCENES (asserted where both are visible)
// row0: the segment's first BUFFER row (2 + its first clip's start); q0: its first query among the batch's rows x nc queries
// (frame-major: (row0 - 2) nc), nq = rows nc of them; g0 / groups: its one-wave workgroups (32 queries each) among the batch's,
// segment after segment -- every segment starts a group of its own, so sum(groups) >= ceil(sum(nq) / 32)
struct ClipSegment { int32_t row0, rows, slot, clip0, nclips, q0, nq, g0, groups; };
inline bool clip_scenes_ok(int32_t n_clips, const int32_t* clip_scene, int32_t n_slots = CLIP_MAX_SCENES) {
    if (n_clips < 1 || !clip_scene) return false;
    for (int32_t k = 0; k < n_clips; ++k) if (clip_scene[k] < 0 || clip_scene[k] >= n_slots) return false;
    return true;
}
// (empty: slots out of range)
inline std::vector<ClipSegment> clip_segments(int32_t n_clips, const int32_t* len, const int32_t* clip_scene, int nc,
                                              int32_t n_slots = CLIP_MAX_SCENES) {
    std::vector<ClipSegment> segs;
    if (!clip_scenes_ok(n_clips, clip_scene, n_slots)) return segs;
    const std::vector<int32_t> s = clip_starts(n_clips, len);
    for (int32_t k = 0; k < n_clips; ++k) {
        if (segs.empty() || segs.back().slot != clip_scene[k]) {
            ClipSegment g = {};
            g.row0 = 2 + s[(size_t)k]; g.slot = clip_scene[k]; g.clip0 = k;
            g.q0 = s[(size_t)k] * nc;
            g.g0 = segs.empty() ? 0 : segs.back().g0 + segs.back().groups;
            segs.push_back(g);
        }
        ClipSegment& g = segs.back();
        g.rows += len[k]; ++g.nclips;
        g.nq = g.rows * nc;
        g.groups = (g.nq + 31) / 32;
    }
    return segs;
}

// FDCAP_NN_SEGMENTS=loop in the environment: the search of such a batch runs segment after segment, one launch set each -- the
// specification of the one-launch form.  Read by forms_read_env() alone (FormSwitches::nn_segments_loop, fdc_forms.h), at every
// fdcap_opt_create*; any other value, or none: the form plan_nn_segments picks.
inline bool clip_segments_loop_env() {
    const char* e = getenv("FDCAP_NN_SEGMENTS");
    return e && e[0] == 'l' && e[1] == 'o' && e[2] == 'o' && e[3] == 'p' && e[4] == 0;
}

// ---- mode 'dct' for a batch (fdcap_opt_set_dct_clips) -------------------------------------------------------------------------
// Clip k of n_k frames has W_k = n_k / T windows over its own frames [0, W_k T); its trailing n_k % T frames belong to no window,
// as in a stand-alone fit.  The batch's windows are numbered clip after clip: that number is the window's slot in c_dct.
// starts [K + 1]: the first window of each clip, starts[K] = the batch's windows
inline std::vector<int32_t> dct_window_starts(int32_t n_clips, const int32_t* len, int32_t T) {
    std::vector<int32_t> s((size_t)n_clips + 1, 0);
    for (int32_t k = 0; k < n_clips; ++k) s[(size_t)k + 1] = s[(size_t)k] + (T > 0 ? len[k] / T : 0);
    return s;
}
// One record per window, what the first phase's wavefronts read once: the BUFFER row of the window's first frame (2 + s_k + w T --
// never (window number) T: wrong as soon as a clip before it has a tail), its clip (selects the clip's objective weight) and its
// slot in c_dct / the Adam moments.
struct DctWindow { int32_t row, clip, slot, pad; };
static_assert(sizeof(DctWindow) == 16, "one s_load_dwordx4 per window");
inline std::vector<DctWindow> dct_window_table(int32_t n_clips, const int32_t* len, int32_t T) {
    const std::vector<int32_t> s = clip_starts(n_clips, len), ws = dct_window_starts(n_clips, len, T);
    std::vector<DctWindow> tab((size_t)ws[(size_t)n_clips]);
    for (int32_t k = 0; k < n_clips; ++k)
        for (int32_t w = 0; w < ws[(size_t)k + 1] - ws[(size_t)k]; ++w)
            tab[(size_t)ws[(size_t)k] + w] = DctWindow{2 + s[(size_t)k] + w * T, k, ws[(size_t)k] + w, 0};
    return tab;
}
// The weight in front of clip k's un-normalised objective sum: the mean runs over the clip's OWN 69 W_k trajectories.  This is the
// float expression the stand-alone launches evaluate on the host (fdcap_opt_dct_fit, opt_backward_impl) with W = W_k, so the bits
// are the stand-alone fit's; the batch kernels read the result, they never divide.  (W_k = 0: no window reads it; 0.)
inline std::vector<float> dct_clip_weights(int32_t n_clips, const int32_t* len, int32_t T, float weight) {
    std::vector<float> w((size_t)n_clips, 0.f);
    for (int32_t k = 0; k < n_clips; ++k) {
        const int32_t W = T > 0 ? len[k] / T : 0;
        if (W > 0) w[(size_t)k] = weight / (69.f * (float)W);
    }
    return w;
}
// Mode 'dct', second phase (global_optimization.py:620): loss_dct w_dct + loss_rec w_rec + loss_contact w_contact -- no smoothing, no world
// term.  Its records are a set of their own (w_sm = w_ws = 0); the DCT weight is no part of a record (dct_clip_weights).
inline LossWeights dct_phase2_weights(float w_dct, float w_rec, float w_contact) {
    LossWeights lw;
    lw.rec = w_rec; lw.smooth = 0.f; lw.contact = w_contact; lw.world = 0.f; lw.dct = w_dct; lw.world_on = false;
    return lw;
}
inline std::vector<ClipRow> clip_rows_build_dct2(int32_t n_clips, const int32_t* len, float w_rec, float w_contact, float weight_loss_rec,
                                                 float weight_contact, int nc) {
    return clip_rows_build(n_clips, len, dct_phase2_weights(0.f, w_rec, w_contact), weight_loss_rec, weight_contact, nc);
}

}  // namespace fdc
