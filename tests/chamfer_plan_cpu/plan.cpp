// plan_nn_batched (csrc/fdc_forms.h) printed for the sizes given on the command line: nq nt B mode ...
#include <stdio.h>
#include <stdlib.h>

#include "fdc_forms.h"

int main(int argc, char** argv) {
    for (int i = 1; i + 3 < argc; i += 4) {
        const int nq = atoi(argv[i]), nt = atoi(argv[i + 1]), B = atoi(argv[i + 2]), mode = atoi(argv[i + 3]);
        const fdc::NNBatchPlan p = fdc::plan_nn_batched(nq, nt, B, mode);
        printf("%d %d %d %d %s %d %d %d %d %d %d %d\n", nq, nt, B, mode, p.name, p.mfma ? 1 : 0, p.nsplit, p.qblocks, p.grid_x, p.block, p.launches,
               fdc::nn_split_len(nt, p.nsplit));
    }
    return 0;
}
