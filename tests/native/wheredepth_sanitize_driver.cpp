// Driver of the sanitizer build of the depth rule and the cost rule of the mask route (make wheredepth_asan; tests/test_where_mask_cpu.py).
// stdin: lines "k selected live B d i8"; stdout: per line "depth cheaper", where depth = sqe_where_depth(k, selected, live) and
// cheaper = where_mask_cheaper(live, selected, B, k, d, i8).
#include <inttypes.h>
#include <stdio.h>

#include "fieldpred.h"

int main() {
    int k, B, d, i8;
    int64_t selected, live;
    while (scanf("%d %" SCNd64 " %" SCNd64 " %d %d %d", &k, &selected, &live, &B, &d, &i8) == 6) {
        const int depth = sqe_where_depth(k, selected, live);
        if (depth != sqe::where_depth(k, selected, live)) return 2;
        printf("%d %d\n", depth, sqe::where_mask_cheaper(live, selected, B, k, d, i8 != 0) ? 1 : 0);
    }
    return 0;
}
