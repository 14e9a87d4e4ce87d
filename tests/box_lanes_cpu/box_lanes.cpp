// Host harness of tests/test_box_lanes_cpu.py: the pure functions behind the streaming search's box-test stages (fdc_forms.h),
// exactly as the kernel calls them.
//   box_lanes lanes n forced ...     one line per (n, forced) pair: nn_box_lanes(n, forced)
//   box_lanes fold                   stdin: lines "lpb hexmask"; per line: folded mask (hex), count, then entry:position for every
//                                    lane that would emit (lane % lpb == 0, its bit set in the folded mask), in lane order
#include <stdio.h>
#include <string.h>

#include "fdc_forms.h"

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "lanes")) {
        for (int i = 2; i + 1 < argc; i += 2) printf("%d\n", fdc::nn_box_lanes(atoi(argv[i]), atoi(argv[i + 1])));
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "fold")) {
        int lpb;
        unsigned long long m;
        while (scanf("%d %llx", &lpb, &m) == 2) {
            const unsigned long long f = fdc::nn_box_fold(m, lpb);
            printf("%llx %d", f, fdc::nn_box_count(f));
            for (int lane = 0; lane < 64; ++lane)
                if (lane % lpb == 0 && ((f >> lane) & 1ull)) printf(" %d:%d", lane / lpb, fdc::nn_box_rank(f, lane));
            printf("\n");
        }
        return 0;
    }
    return 2;
}
