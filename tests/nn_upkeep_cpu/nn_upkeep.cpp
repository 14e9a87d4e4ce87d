// Host harness of tests/test_nn_upkeep_cpu.py: the schedule of the streaming search's query-order rebuilds (fdc_forms.h
// nn_order_period), exactly as nn_stream_upkeep calls it.
//   nn_upkeep period nq base rebuilds ...    one line per (base, rebuilds) pair: nn_order_period(base, rebuilds, nq)
//   nn_upkeep constants                      NN_PERIOD_HOLD NN_PERIOD_MAX NN_PERIOD_GROW_MAX_QUERIES FDC_NN_PERIOD_GROWTH
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fdc_forms.h"

static_assert(fdc::nn_order_period(0, 5, 1) == 0 && fdc::nn_order_period(32, 0, 1) == 32, "usable in constant expressions");

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "period")) {
        const int nq = argc >= 3 ? atoi(argv[2]) : 0;
        for (int i = 3; i + 1 < argc; i += 2) printf("%d\n", fdc::nn_order_period(atoi(argv[i]), atoi(argv[i + 1]), nq));
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "constants")) {
        printf("%d %d %d %d\n", fdc::NN_PERIOD_HOLD, fdc::NN_PERIOD_MAX, fdc::NN_PERIOD_GROW_MAX_QUERIES, (int)FDC_NN_PERIOD_GROWTH);
        return 0;
    }
    return 2;
}
