// peer_args_check.cpp -- a stand-alone host program for `make peer-args-check`: it drives the argument checks of
// nvrx_peer_score and nvrx_report_peer with INVALID arguments only, so no call reaches a device, and is meant to be built
// together with nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.  Exit status 0 when
// every call returned the error the header promises.
#include "args_check.h"

int main() {
    float *table = reinterpret_cast<float *>(uintptr_t{8192});  // never dereferenced: every call below fails its checks
    int32_t *groups = reinterpret_cast<int32_t *>(uintptr_t{4096});
    void *out = reinterpret_cast<void *>(uintptr_t{16384});
    void *odd = reinterpret_cast<void *>(uintptr_t{16392});
    expect("R 0", nvrx_peer_score(table, 0, 5, 2, groups, 1, 0, 1, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R < 0", nvrx_peer_score(table, -3, 5, 2, groups, 1, 0, 1, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("K < 0", nvrx_peer_score(table, 8, -1, 2, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S < 0", nvrx_peer_score(table, 8, 5, -1, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R too large", nvrx_peer_score(table, NVRX_ROBUST_MAX_RANKS + 1, 5, 2, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_RANGE, "ranks");
    expect("K too large", nvrx_peer_score(table, 8, NVRX_MAX_ROWS + 1, 2, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("S too large", nvrx_peer_score(table, 8, 5, NVRX_MAX_ROWS + 1, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("first_rank < 0", nvrx_peer_score(table, 8, 5, 2, groups, 2, -1, 4, 2, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("n_ranks 0", nvrx_peer_score(table, 8, 5, 2, groups, 2, 0, 0, 2, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("ranks past R", nvrx_peer_score(table, 8, 5, 2, groups, 2, 5, 4, 2, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("min_ranks 0", nvrx_peer_score(table, 8, 5, 2, groups, 2, 0, 8, 0, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("min_ranks < 0", nvrx_peer_score(table, 8, 5, 2, groups, 2, 0, 8, -2, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("G 0", nvrx_peer_score(table, 8, 5, 2, groups, 0, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "groups");
    expect("G < 0", nvrx_peer_score(table, 8, 5, 2, groups, -1, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "groups");
    expect("G > R", nvrx_peer_score(table, 8, 5, 2, groups, 9, 0, 8, 2, out, nullptr), NVRX_ERR_RANGE, "groups");
    expect("G above the cap", nvrx_peer_score(table, NVRX_ROBUST_MAX_RANKS, 5, 2, groups, NVRX_PEER_MAX_GROUPS + 1, 0, 8, 2, out, nullptr),
           NVRX_ERR_RANGE, "at most");
    expect("null table", nvrx_peer_score(nullptr, 8, 5, 2, groups, 2, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null groups", nvrx_peer_score(table, 8, 5, 2, nullptr, 2, 0, 8, 2, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records", nvrx_peer_score(table, 8, 5, 2, groups, 2, 0, 8, 2, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned records", nvrx_peer_score(table, 8, 5, 2, groups, 2, 0, 8, 2, odd, nullptr), NVRX_ERR_INVALID, "aligned");

    // nvrx_report_peer: every check that precedes the look at the context reads the descriptor's shape only, so a context that
    // was never created will do (the state check -- a report issued through this descriptor -- is the GPU tests' to cover)
    nvrx_ctx *ctx = reinterpret_cast<nvrx_ctx *>(uintptr_t{4096});
    nvrx_report_desc d;
    memset(&d, 0, sizeof d);
    d.R = 8, d.K = 5, d.S = 2;
    expect("null context", nvrx_report_peer(nullptr, &d, groups, 2, 0, 8, 2, out), NVRX_ERR_INVALID, "null");
    expect("null descriptor", nvrx_report_peer(ctx, nullptr, groups, 2, 0, 8, 2, out), NVRX_ERR_INVALID, "null");
    expect("report: ranks past R", nvrx_report_peer(ctx, &d, groups, 2, 5, 4, 2, out), NVRX_ERR_RANGE, "outside");
    expect("report: min_ranks 0", nvrx_report_peer(ctx, &d, groups, 2, 0, 8, 0, out), NVRX_ERR_RANGE, "min_ranks");
    expect("report: G 0", nvrx_report_peer(ctx, &d, groups, 0, 0, 8, 2, out), NVRX_ERR_INVALID, "groups");
    expect("report: G > R", nvrx_report_peer(ctx, &d, groups, 9, 0, 8, 2, out), NVRX_ERR_RANGE, "groups");
    expect("report: null groups", nvrx_report_peer(ctx, &d, nullptr, 2, 0, 8, 2, out), NVRX_ERR_INVALID, "null");
    expect("report: null records", nvrx_report_peer(ctx, &d, groups, 2, 0, 8, 2, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("report: misaligned records", nvrx_report_peer(ctx, &d, groups, 2, 0, 8, 2, odd), NVRX_ERR_INVALID, "aligned");
    d.R = NVRX_ROBUST_MAX_RANKS;
    expect("report: G above the cap", nvrx_report_peer(ctx, &d, groups, NVRX_PEER_MAX_GROUPS + 1, 0, 8, 2, out), NVRX_ERR_RANGE, "at most");
    d.R = 0;
    expect("report: R 0", nvrx_report_peer(ctx, &d, groups, 1, 0, 1, 2, out), NVRX_ERR_INVALID, "shape");
    printf("peer_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
