// The pure functions behind r21's search scheduling (csrc/fdc_forms.h), through a plain host build with its own main:
//   search_items shift <ns> ...                  nn_order_key_shift(ns), one per line
//   search_items ipc <nq> <nchunk> <eighths> <forced> ...   plan_nn_items_per_chunk, one per line
//   search_items ids <ipc> <nchunk>              packs and unpacks every id of a scene of nchunk chunks; prints the largest id and "ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fdc_forms.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "shift")) {
        for (int i = 2; i < argc; ++i) printf("%d\n", fdc::nn_order_key_shift(atoi(argv[i])));
        return 0;
    }
    if (!strcmp(argv[1], "ipc")) {
        if ((argc - 2) % 4) return 2;
        for (int i = 2; i + 3 < argc; i += 4)
            printf("%d\n", fdc::plan_nn_items_per_chunk(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]) != 0, atoi(argv[i + 3])));
        return 0;
    }
    if (!strcmp(argv[1], "ids") && argc == 4) {
        const int ipc = atoi(argv[2]), nchunk = atoi(argv[3]);
        if ((ipc != 4 && ipc != 8) || nchunk < 1) return 2;
        std::vector<unsigned short> list((size_t)ipc * nchunk);              // a work list's element type
        int largest = -1;
        for (int c = 0; c < nchunk; ++c)
            for (int it = 0; it < ipc; ++it) {
                const int id = fdc::nn_item_id(ipc, c, it);
                if (id < 0 || id >= ipc * nchunk) { printf("id %d of chunk %d item %d leaves the table\n", id, c, it); return 1; }
                list[(size_t)id] = (unsigned short)id;
                largest = id > largest ? id : largest;
            }
        for (size_t k = 0; k < list.size(); ++k) {                           // dense, in (chunk, item) order, and back through 16 bits
            const int id = (int)list[k], c = fdc::nn_item_chunk(ipc, id), it = fdc::nn_item_of(ipc, id);
            if ((size_t)id != k || c != (int)(k / ipc) || it != (int)(k % ipc)) { printf("slot %zu unpacks to chunk %d item %d\n", k, c, it); return 1; }
        }
        printf("%d\nok\n", largest);
        return 0;
    }
    return 2;
}
