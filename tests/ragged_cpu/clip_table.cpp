// Prints csrc/fdc_clips.h's clip table for tests/test_ragged_clips_cpu.py.  Plain g++: the header must not need HIP.
//   clip_table REC SMOOTH CONTACT WORLD WORLD_ON W_REC W_CONTACT NC WANT_TOTAL MAX_ROWS LEN...     (floats as their uint32 bit patterns)
// Output: "ok 0|1", "equal 0|1", then (lengths ok only) "starts ...", one "w k bits bits bits bits" per clip and one
// "row r k g n bits bits bits bits" per buffer row.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fdc_clips.h"

static float f_of(const char* s) { const uint32_t u = (uint32_t)strtoul(s, nullptr, 10); float f; memcpy(&f, &u, 4); return f; }
static unsigned u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
    if (argc < 11) return 2;
    fdc::LossWeights lw;
    lw.rec = f_of(argv[1]); lw.smooth = f_of(argv[2]); lw.contact = f_of(argv[3]); lw.world = f_of(argv[4]); lw.dct = 0.f;
    lw.world_on = atoi(argv[5]) != 0;
    const float w_rec = f_of(argv[6]), w_contact = f_of(argv[7]);
    const int nc = atoi(argv[8]);
    const long long want = atoll(argv[9]), max_rows = atoll(argv[10]);
    std::vector<int32_t> len;
    for (int i = 11; i < argc; ++i) len.push_back((int32_t)atoi(argv[i]));
    const int32_t K = (int32_t)len.size();
    const bool ok = fdc::clip_lengths_ok(K, len.empty() ? nullptr : len.data(), want, max_rows);
    printf("ok %d\n", ok ? 1 : 0);
    if (!ok) return 0;
    printf("equal %d\n", fdc::clip_lengths_equal(K, len.data()) ? 1 : 0);
    const std::vector<int32_t> s = fdc::clip_starts(K, len.data());
    printf("starts");
    for (int32_t v : s) printf(" %d", v);
    printf("\n");
    for (int32_t k = 0; k < K; ++k) {
        const fdc::ClipWeights w = fdc::clip_weights(len[k], lw, w_rec, w_contact, nc);
        printf("w %d %u %u %u %u\n", k, u_of(w.w_rec), u_of(w.w_sm), u_of(w.w_ws), u_of(w.coef));
    }
    const std::vector<fdc::ClipRow> rows = fdc::clip_rows_build(K, len.data(), lw, w_rec, w_contact, nc);
    for (size_t r = 0; r < rows.size(); ++r)
        printf("row %zu %d %d %d %u %u %u %u\n", r, rows[r].k, rows[r].g, rows[r].n, u_of(rows[r].w_rec), u_of(rows[r].w_sm), u_of(rows[r].w_ws),
               u_of(rows[r].coef));
    return 0;
}
