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

#include <vector>

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
inline std::vector<ClipRow> clip_rows_build(int32_t n_clips, const int32_t* len, const LossWeights& lw, float weight_loss_rec,
                                            float weight_contact, int nc) {
    const std::vector<int32_t> s = clip_starts(n_clips, len);
    std::vector<ClipRow> rows((size_t)s[(size_t)n_clips] + 4);
    const ClipRow halo_lo = {0, 0, 0, 0.f, 0.f, 0.f, 0.f, 0}, halo_hi = {n_clips - 1, 0, 0, 0.f, 0.f, 0.f, 0.f, 0};
    rows[0] = rows[1] = halo_lo;
    rows[rows.size() - 2] = rows[rows.size() - 1] = halo_hi;
    for (int32_t k = 0; k < n_clips; ++k) {
        const ClipWeights w = clip_weights(len[k], lw, weight_loss_rec, weight_contact, nc);
        for (int32_t g = 0; g < len[k]; ++g) rows[(size_t)2 + s[(size_t)k] + g] = ClipRow{k, g, len[k], w.w_rec, w.w_sm, w.w_ws, w.coef, 0};
    }
    return rows;
}

}  // namespace fdc
