// Host harness of tests/test_multiscene_cpu.py: the segment table of a batch of clips of several scenes (csrc/fdc_clips.h) and the
// decision between the one-launch and the per-segment search (plan_nn_segments, csrc/fdc_forms.h), as plain g++ compiles them.
//   segment_table seg  NC K len_0 .. len_{K-1} slot_0 .. slot_{K-1}
//       -> "ok 0|1", then one line "seg row0 rows slot clip0 nclips q0 nq g0 groups" per segment
//   segment_table plan NN_STREAM LOOP MODE CULLED FRAGS SEED_IN_PLACE S nq_0 .. nq_{S-1} nt_0 .. nt_{S-1}
//       -> "plan one_launch grid_x grid_y block name"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fdc_clips.h"
#include "fdc_forms.h"

using namespace fdc;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "seg")) {
        if (argc < 4) return 2;
        const int nc = atoi(argv[2]), K = atoi(argv[3]);
        if (K < 0 || argc != 4 + 2 * K) return 2;
        std::vector<int32_t> len((size_t)K), slot((size_t)K);
        for (int k = 0; k < K; ++k) { len[(size_t)k] = atoi(argv[4 + k]); slot[(size_t)k] = atoi(argv[4 + K + k]); }
        printf("ok %d\n", clip_scenes_ok(K, slot.data()) ? 1 : 0);
        for (const ClipSegment& g : clip_segments(K, len.data(), slot.data(), nc))
            printf("seg %d %d %d %d %d %d %d %d %d\n", g.row0, g.rows, g.slot, g.clip0, g.nclips, g.q0, g.nq, g.g0, g.groups);
        return 0;
    }
    if (!strcmp(argv[1], "plan")) {
        if (argc < 9) return 2;
        FormSwitches sw;
        sw.nn_stream = atoi(argv[2]);
        sw.nn_segments_loop = atoi(argv[3]) != 0;
        const int mode = atoi(argv[4]);
        const bool culled = atoi(argv[5]) != 0, frags = atoi(argv[6]) != 0, sip = atoi(argv[7]) != 0;
        const int S = atoi(argv[8]);
        if (S < 0 || argc != 9 + 2 * S) return 2;
        std::vector<int> nq((size_t)S), nt((size_t)S);
        for (int s = 0; s < S; ++s) { nq[(size_t)s] = atoi(argv[9 + s]); nt[(size_t)s] = atoi(argv[9 + S + s]); }
        const NNSegPlan p = plan_nn_segments(S, nq.data(), nt.data(), culled, frags, sip, 1, mode, sw);
        printf("plan %d %d %d %d %s\n", p.one_launch ? 1 : 0, p.grid_x, p.grid_y, p.block, p.name ? p.name : "-");
        return 0;
    }
    return 2;
}
