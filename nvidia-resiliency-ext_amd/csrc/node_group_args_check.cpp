// node_group_args_check.cpp -- a stand-alone host program for `make node-group-args-check`: it drives the argument checks of
// nvrx_node_group_score and nvrx_report_node_group with INVALID arguments only, so no call reaches a device, and is meant to be
// built together with nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.  Exit status 0
// when every call returned the error the header promises.
#include "args_check.h"

int main() {
    float *table = reinterpret_cast<float *>(uintptr_t{8192});  // never dereferenced: every call below fails its checks
    int32_t *cells = reinterpret_cast<int32_t *>(uintptr_t{12288});
    void *out = reinterpret_cast<void *>(uintptr_t{16384});
    void *odd = reinterpret_cast<void *>(uintptr_t{16392});
    // (table, R, K, S, cells, C, Gp, Gn, max_cell, max_group_cells, max_node_cells, min_members, min_nodes, min_peers, first_rank,
    //  n_ranks, out, stream)
    auto score = [&](const float *t, int R, int K, int S, const int32_t *c, int C, int Gp, int Gn, int mc, int mg, int mn, int mm,
                     int mnod, int mp, int first, int n, void *o) {
        return nvrx_node_group_score(t, R, K, S, c, C, Gp, Gn, mc, mg, mn, mm, mnod, mp, first, n, o, nullptr);
    };
    expect("R 0", score(table, 0, 5, 2, cells, 1, 1, 1, 1, 1, 1, 2, 3, 2, 0, 1, out), NVRX_ERR_INVALID, "shape");
    expect("K < 0", score(table, 8, -1, 2, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_INVALID, "shape");
    expect("R too large", score(table, NVRX_ROBUST_MAX_RANKS + 1, 5, 2, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE,
           "ranks");
    expect("S too large", score(table, 8, 5, NVRX_MAX_ROWS + 1, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "ids");
    expect("n_ranks 0", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 0, out), NVRX_ERR_RANGE, "outside");
    expect("ranks past R", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 5, 4, out), NVRX_ERR_RANGE, "outside");
    expect("C 0", score(table, 8, 5, 2, cells, 0, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_INVALID, "groups");
    expect("C > R", score(table, 8, 5, 2, cells, 9, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "groups");
    expect("C too large", score(table, NVRX_PEER_MAX_GROUPS + 2, 5, 2, cells, NVRX_PEER_MAX_GROUPS + 1, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out),
           NVRX_ERR_RANGE, "at most");
    expect("max_cell 0", score(table, 8, 5, 2, cells, 4, 2, 2, 0, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "max_group");
    expect("max_cell > R", score(table, 8, 5, 2, cells, 4, 2, 2, 9, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "max_group");
    expect("min_members 0", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 2, 2, 0, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "min_members");
    expect("min_nodes 0", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 2, 2, 2, 0, 2, 0, 8, out), NVRX_ERR_RANGE, "min_nodes");
    expect("Gp 0", score(table, 8, 5, 2, cells, 4, 0, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "Gp");
    expect("Gp > C", score(table, 8, 5, 2, cells, 4, 5, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "Gp");
    expect("Gn 0", score(table, 8, 5, 2, cells, 4, 2, 0, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "Gn");
    expect("Gn > C", score(table, 8, 5, 2, cells, 4, 2, 5, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "Gn");
    expect("max_group_cells 0", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 0, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "max_group_cells");
    expect("max_group_cells > C", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 5, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "max_group_cells");
    expect("max_node_cells 0", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 2, 0, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "max_node_cells");
    expect("max_node_cells > C", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 2, 5, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "max_node_cells");
    expect("min_peers 0", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 2, 2, 2, 3, 0, 0, 8, out), NVRX_ERR_RANGE, "min_peers");
    expect("null table", score(nullptr, 8, 5, 2, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_INVALID, "null");
    expect("null cells", score(table, 8, 5, 2, nullptr, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_INVALID, "null");
    expect("null records", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned records", score(table, 8, 5, 2, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, odd), NVRX_ERR_INVALID, "aligned");
    // the order: nvrx_node_score's (shape, ranks, C, max_cell, min_members, min_nodes), then Gp, Gn, the two maxima, min_peers,
    // then the pointers
    expect("shape before ranks", score(nullptr, 0, 5, 2, nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 4, odd), NVRX_ERR_INVALID, "shape");
    expect("ranks before C", score(nullptr, 8, 5, 2, nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 4, odd), NVRX_ERR_RANGE, "outside");
    expect("C before max_cell", score(nullptr, 8, 5, 2, nullptr, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 8, odd), NVRX_ERR_RANGE, "groups");
    expect("max_cell before min_members", score(nullptr, 8, 5, 2, nullptr, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 8, odd), NVRX_ERR_RANGE, "max_group");
    expect("min_members before min_nodes", score(nullptr, 8, 5, 2, nullptr, 4, 0, 0, 2, 0, 0, 0, 0, 0, 0, 8, odd), NVRX_ERR_RANGE, "min_members");
    expect("min_nodes before Gp", score(nullptr, 8, 5, 2, nullptr, 4, 0, 0, 2, 0, 0, 2, 0, 0, 0, 8, odd), NVRX_ERR_RANGE, "min_nodes");
    expect("Gp before Gn", score(nullptr, 8, 5, 2, nullptr, 4, 0, 0, 2, 0, 0, 2, 3, 0, 0, 8, odd), NVRX_ERR_RANGE, "Gp");
    expect("Gn before max_group_cells", score(nullptr, 8, 5, 2, nullptr, 4, 2, 0, 2, 0, 0, 2, 3, 0, 0, 8, odd), NVRX_ERR_RANGE, "Gn");
    expect("max_group_cells before max_node_cells", score(nullptr, 8, 5, 2, nullptr, 4, 2, 2, 2, 0, 0, 2, 3, 0, 0, 8, odd), NVRX_ERR_RANGE,
           "max_group_cells");
    expect("max_node_cells before min_peers", score(nullptr, 8, 5, 2, nullptr, 4, 2, 2, 2, 2, 0, 2, 3, 0, 0, 8, odd), NVRX_ERR_RANGE,
           "max_node_cells");
    expect("min_peers before pointers", score(nullptr, 8, 5, 2, nullptr, 4, 2, 2, 2, 2, 2, 2, 3, 0, 0, 8, odd), NVRX_ERR_RANGE, "min_peers");

    // nvrx_report_node_group: every check that precedes the look at the context reads the descriptor's shape only, so a context
    // that was never created will do (the state check is the GPU tests' to cover)
    nvrx_ctx *ctx = reinterpret_cast<nvrx_ctx *>(uintptr_t{4096});
    nvrx_report_desc d;
    memset(&d, 0, sizeof d);
    d.R = 8, d.K = 5, d.S = 2;
    expect("null context", nvrx_report_node_group(nullptr, &d, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_INVALID, "null");
    expect("null descriptor", nvrx_report_node_group(ctx, nullptr, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_INVALID, "null");
    expect("report: ranks past R", nvrx_report_node_group(ctx, &d, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 5, 4, out), NVRX_ERR_RANGE, "outside");
    expect("report: C > R", nvrx_report_node_group(ctx, &d, cells, 9, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "groups");
    expect("report: Gp > C", nvrx_report_node_group(ctx, &d, cells, 4, 5, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE, "Gp");
    expect("report: max_node_cells 0", nvrx_report_node_group(ctx, &d, cells, 4, 2, 2, 2, 2, 0, 2, 3, 2, 0, 8, out), NVRX_ERR_RANGE,
           "max_node_cells");
    expect("report: min_peers 0", nvrx_report_node_group(ctx, &d, cells, 4, 2, 2, 2, 2, 2, 2, 3, 0, 0, 8, out), NVRX_ERR_RANGE, "min_peers");
    expect("report: null cells", nvrx_report_node_group(ctx, &d, nullptr, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, out), NVRX_ERR_INVALID, "null");
    expect("report: null records", nvrx_report_node_group(ctx, &d, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("report: misaligned records", nvrx_report_node_group(ctx, &d, cells, 4, 2, 2, 2, 2, 2, 2, 3, 2, 0, 8, odd), NVRX_ERR_INVALID, "aligned");
    d.R = 0;
    expect("report: R 0", nvrx_report_node_group(ctx, &d, cells, 1, 1, 1, 1, 1, 1, 2, 3, 2, 0, 1, out), NVRX_ERR_INVALID, "shape");
    printf("node_group_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
