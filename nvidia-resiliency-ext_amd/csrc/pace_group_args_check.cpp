// pace_group_args_check.cpp -- a stand-alone host program for `make pace-group-args-check`: it drives the argument checks of
// nvrx_pace_group_score and nvrx_report_pace_group with INVALID arguments only, so no call reaches a device, and is meant to
// be built together with nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.  Exit status
// 0 when every call returned the error the header promises.
#include "args_check.h"

int main() {
    float *table = reinterpret_cast<float *>(uintptr_t{8192});  // never dereferenced: every call below fails its checks
    int32_t *groups = reinterpret_cast<int32_t *>(uintptr_t{12288});
    void *out = reinterpret_cast<void *>(uintptr_t{16384});
    void *odd = reinterpret_cast<void *>(uintptr_t{16392});
    // (table, R, K, S, groups, G, max_group, first_rank, n_ranks, min_ranks, min_peers, out, stream)
    expect("R 0", nvrx_pace_group_score(table, 0, 5, 2, groups, 1, 1, 0, 1, 4, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R < 0", nvrx_pace_group_score(table, -3, 5, 2, groups, 1, 1, 0, 1, 4, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("K < 0", nvrx_pace_group_score(table, 8, -1, 2, groups, 2, 4, 0, 8, 4, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S < 0", nvrx_pace_group_score(table, 8, 5, -1, groups, 2, 4, 0, 8, 4, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R too large", nvrx_pace_group_score(table, NVRX_ROBUST_MAX_RANKS + 1, 5, 2, groups, 2, 4, 0, 8, 4, 2, out, nullptr),
           NVRX_ERR_RANGE, "ranks");
    expect("K too large", nvrx_pace_group_score(table, 8, NVRX_MAX_ROWS + 1, 2, groups, 2, 4, 0, 8, 4, 2, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("S too large", nvrx_pace_group_score(table, 8, 5, NVRX_MAX_ROWS + 1, groups, 2, 4, 0, 8, 4, 2, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("first_rank < 0", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, 4, -1, 4, 4, 2, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("n_ranks 0", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, 4, 0, 0, 4, 2, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("ranks past R", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, 4, 5, 4, 4, 2, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("min_ranks 0", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, 4, 0, 8, 0, 2, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("G 0", nvrx_pace_group_score(table, 8, 5, 2, groups, 0, 4, 0, 8, 4, 2, out, nullptr), NVRX_ERR_INVALID, "groups");
    expect("G < 0", nvrx_pace_group_score(table, 8, 5, 2, groups, -1, 4, 0, 8, 4, 2, out, nullptr), NVRX_ERR_INVALID, "groups");
    expect("G > R", nvrx_pace_group_score(table, 8, 5, 2, groups, 9, 4, 0, 8, 4, 2, out, nullptr), NVRX_ERR_RANGE, "groups");
    expect("G too large", nvrx_pace_group_score(table, NVRX_PEER_MAX_GROUPS + 2, 5, 2, groups, NVRX_PEER_MAX_GROUPS + 1, 4, 0, 8, 4, 2,
                                                out, nullptr), NVRX_ERR_RANGE, "at most");
    expect("max_group 0", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, 0, 0, 8, 4, 2, out, nullptr), NVRX_ERR_RANGE, "max_group");
    expect("max_group < 0", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, -4, 0, 8, 4, 2, out, nullptr), NVRX_ERR_RANGE, "max_group");
    expect("max_group > R", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, 9, 0, 8, 4, 2, out, nullptr), NVRX_ERR_RANGE, "max_group");
    expect("min_peers 0", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, 4, 0, 8, 4, 0, out, nullptr), NVRX_ERR_RANGE, "min_peers");
    expect("min_peers < 0", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, 4, 0, 8, 4, -1, out, nullptr), NVRX_ERR_RANGE, "min_peers");
    expect("null table", nvrx_pace_group_score(nullptr, 8, 5, 2, groups, 2, 4, 0, 8, 4, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null groups", nvrx_pace_group_score(table, 8, 5, 2, nullptr, 2, 4, 0, 8, 4, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, 4, 0, 8, 4, 2, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned records", nvrx_pace_group_score(table, 8, 5, 2, groups, 2, 4, 0, 8, 4, 2, odd, nullptr), NVRX_ERR_INVALID, "aligned");
    // the order: a bad shape wins over a bad rank range, that over min_ranks, that over G, that over max_group, that over
    // min_peers, that over the pointers
    expect("shape before ranks", nvrx_pace_group_score(nullptr, 0, 5, 2, nullptr, 0, 0, 5, 4, 0, 0, odd, nullptr), NVRX_ERR_INVALID, "shape");
    expect("ranks before min_ranks", nvrx_pace_group_score(nullptr, 8, 5, 2, nullptr, 0, 0, 5, 4, 0, 0, odd, nullptr), NVRX_ERR_RANGE, "outside");
    expect("min_ranks before G", nvrx_pace_group_score(nullptr, 8, 5, 2, nullptr, 0, 0, 0, 8, 0, 0, odd, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("G before max_group", nvrx_pace_group_score(nullptr, 8, 5, 2, nullptr, 9, 0, 0, 8, 4, 0, odd, nullptr), NVRX_ERR_RANGE, "groups");
    expect("max_group before min_peers", nvrx_pace_group_score(nullptr, 8, 5, 2, nullptr, 2, 0, 0, 8, 4, 0, odd, nullptr), NVRX_ERR_RANGE, "max_group");
    expect("min_peers before pointers", nvrx_pace_group_score(nullptr, 8, 5, 2, nullptr, 2, 4, 0, 8, 4, 0, odd, nullptr), NVRX_ERR_RANGE, "min_peers");

    // nvrx_report_pace_group: every check that precedes the look at the context reads the descriptor's shape only, so a context
    // that was never created will do (the state check -- a report issued through this descriptor -- is the GPU tests' to cover)
    nvrx_ctx *ctx = reinterpret_cast<nvrx_ctx *>(uintptr_t{4096});
    nvrx_report_desc d;
    memset(&d, 0, sizeof d);
    d.R = 8, d.K = 5, d.S = 2;
    expect("null context", nvrx_report_pace_group(nullptr, &d, groups, 2, 4, 0, 8, 4, 2, out), NVRX_ERR_INVALID, "null");
    expect("null descriptor", nvrx_report_pace_group(ctx, nullptr, groups, 2, 4, 0, 8, 4, 2, out), NVRX_ERR_INVALID, "null");
    expect("report: ranks past R", nvrx_report_pace_group(ctx, &d, groups, 2, 4, 5, 4, 4, 2, out), NVRX_ERR_RANGE, "outside");
    expect("report: min_ranks 0", nvrx_report_pace_group(ctx, &d, groups, 2, 4, 0, 8, 0, 2, out), NVRX_ERR_RANGE, "min_ranks");
    expect("report: G 0", nvrx_report_pace_group(ctx, &d, groups, 0, 4, 0, 8, 4, 2, out), NVRX_ERR_INVALID, "groups");
    expect("report: G > R", nvrx_report_pace_group(ctx, &d, groups, 9, 4, 0, 8, 4, 2, out), NVRX_ERR_RANGE, "groups");
    expect("report: max_group > R", nvrx_report_pace_group(ctx, &d, groups, 2, 9, 0, 8, 4, 2, out), NVRX_ERR_RANGE, "max_group");
    expect("report: min_peers 0", nvrx_report_pace_group(ctx, &d, groups, 2, 4, 0, 8, 4, 0, out), NVRX_ERR_RANGE, "min_peers");
    expect("report: null groups", nvrx_report_pace_group(ctx, &d, nullptr, 2, 4, 0, 8, 4, 2, out), NVRX_ERR_INVALID, "null");
    expect("report: null records", nvrx_report_pace_group(ctx, &d, groups, 2, 4, 0, 8, 4, 2, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("report: misaligned records", nvrx_report_pace_group(ctx, &d, groups, 2, 4, 0, 8, 4, 2, odd), NVRX_ERR_INVALID, "aligned");
    d.R = 0;
    expect("report: R 0", nvrx_report_pace_group(ctx, &d, groups, 1, 1, 0, 1, 4, 2, out), NVRX_ERR_INVALID, "shape");
    printf("pace_group_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
