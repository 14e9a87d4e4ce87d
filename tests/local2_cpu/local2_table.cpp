// Prints csrc/fdc_clips.h's weights and records of mode 'local''s second loop for tests/test_local2_clips_cpu.py.  Plain g++: the
// header must not need HIP.
//   local2_table W_REC NV3 NPART LEN...     (W_REC as its uint32 bit pattern)
// Output: one "w k bits(w_rec) bits(w_sm) bits(w_vs) bits(coef) bits(foot-skate inv)" per clip, then one
// "row r k g n bits bits bits bits" per buffer row of the second loop's record set.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fdc_clips.h"

static float f_of(const char* s) { const uint32_t u = (uint32_t)strtoul(s, nullptr, 10); float f; memcpy(&f, &u, 4); return f; }
static unsigned u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const float w_rec = f_of(argv[1]);
    const size_t nv3 = (size_t)atoll(argv[2]);
    const int npart = atoi(argv[3]);
    std::vector<int32_t> len;
    for (int i = 4; i < argc; ++i) len.push_back((int32_t)atoi(argv[i]));
    const int32_t K = (int32_t)len.size();
    for (int32_t k = 0; k < K; ++k) {
        const fdc::ClipWeights w = fdc::clip_weights_local2(len[k], w_rec, nv3);
        printf("w %d %u %u %u %u %u\n", k, u_of(w.w_rec), u_of(w.w_sm), u_of(w.w_ws), u_of(w.coef), u_of(fdc::clip_foot_skate_inv(len[k], npart)));
    }
    const std::vector<fdc::ClipRow> rows = fdc::clip_rows_build_local2(K, len.data(), w_rec, nv3);
    for (size_t r = 0; r < rows.size(); ++r)
        printf("row %zu %d %d %d %u %u %u %u\n", r, rows[r].k, rows[r].g, rows[r].n, u_of(rows[r].w_rec), u_of(rows[r].w_sm), u_of(rows[r].w_ws),
               u_of(rows[r].coef));
    return 0;
}
