// Prints csrc/fdc_clips.h's tables of mode 'dct' for a batch of clips for tests/test_dct_clips_cpu.py.  Plain g++: the header must
// not need HIP.
//   dct_table T WEIGHT W_REC W_CONTACT WEIGHT_LOSS_REC WEIGHT_CONTACT NC LEN...     (the floats as uint32 bit patterns)
// Output: "start k first-window" per clip and one for the total, "win i row clip slot" per window, "wk k bits(weight / (69 W_k))"
// per clip, then "row r k g n bits(w_rec) bits(w_sm) bits(w_ws) bits(coef)" per buffer row of the second phase's record set.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fdc_clips.h"

static float f_of(const char* s) { const uint32_t u = (uint32_t)strtoul(s, nullptr, 10); float f; memcpy(&f, &u, 4); return f; }
static unsigned u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
    if (argc < 9) return 2;
    const int32_t T = (int32_t)atoi(argv[1]);
    const float weight = f_of(argv[2]), w_rec = f_of(argv[3]), w_contact = f_of(argv[4]), weight_loss_rec = f_of(argv[5]),
                weight_contact = f_of(argv[6]);
    const int nc = atoi(argv[7]);
    std::vector<int32_t> len;
    for (int i = 8; i < argc; ++i) len.push_back((int32_t)atoi(argv[i]));
    const int32_t K = (int32_t)len.size();
    const std::vector<int32_t> ws = fdc::dct_window_starts(K, len.data(), T);
    for (size_t k = 0; k < ws.size(); ++k) printf("start %zu %d\n", k, ws[k]);
    const std::vector<fdc::DctWindow> tab = fdc::dct_window_table(K, len.data(), T);
    for (size_t i = 0; i < tab.size(); ++i) printf("win %zu %d %d %d\n", i, tab[i].row, tab[i].clip, tab[i].slot);
    const std::vector<float> wk = fdc::dct_clip_weights(K, len.data(), T, weight);
    for (size_t k = 0; k < wk.size(); ++k) printf("wk %zu %u\n", k, u_of(wk[k]));
    const std::vector<fdc::ClipRow> rows = fdc::clip_rows_build_dct2(K, len.data(), w_rec, w_contact, weight_loss_rec, weight_contact, nc);
    for (size_t r = 0; r < rows.size(); ++r)
        printf("row %zu %d %d %d %u %u %u %u\n", r, rows[r].k, rows[r].g, rows[r].n, u_of(rows[r].w_rec), u_of(rows[r].w_sm), u_of(rows[r].w_ws),
               u_of(rows[r].coef));
    return 0;
}
