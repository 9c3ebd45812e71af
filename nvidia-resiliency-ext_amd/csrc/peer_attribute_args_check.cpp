// peer_attribute_args_check.cpp -- a stand-alone host program for `make peer-attribute-args-check`: it drives the argument
// checks of nvrx_peer_attribute and nvrx_report_peer_attribute with INVALID arguments only, so no call reaches a device, and is
// meant to be built together with nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.
// Exit status 0 when every call returned the error the header promises.
#include "args_check.h"

int main() {
    float *table = reinterpret_cast<float *>(uintptr_t{8192});  // never dereferenced: every call below fails its checks
    int32_t *groups = reinterpret_cast<int32_t *>(uintptr_t{4096});
    void *cols = reinterpret_cast<void *>(uintptr_t{32768});
    void *out = reinterpret_cast<void *>(uintptr_t{16384});
    void *odd = reinterpret_cast<void *>(uintptr_t{16392});
    // nvrx_attribute's checks, in its order
    expect("R 0", nvrx_peer_attribute(table, 0, 5, 2, groups, 1, cols, 0, 1, 2, 3, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("K < 0", nvrx_peer_attribute(table, 8, -1, 2, groups, 2, cols, 0, 8, 2, 3, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S < 0", nvrx_peer_attribute(table, 8, 5, -1, groups, 2, cols, 0, 8, 2, 3, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("K too large", nvrx_peer_attribute(table, 8, NVRX_MAX_ROWS + 1, 2, groups, 2, cols, 0, 8, 2, 3, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("top_n 0", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, cols, 0, 8, 2, 0, out, nullptr), NVRX_ERR_RANGE, "top_n");
    expect("top_n 17", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, cols, 0, 8, 2, NVRX_ATTR_MAX_TOP + 1, out, nullptr), NVRX_ERR_RANGE, "top_n");
    expect("top_n before the ranks", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, cols, 5, 4, 2, 0, out, nullptr), NVRX_ERR_RANGE, "top_n");
    expect("first_rank < 0", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, cols, -1, 4, 2, 3, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("n_ranks 0", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, cols, 0, 0, 2, 3, out, nullptr), NVRX_ERR_RANGE, "outside");
    expect("ranks past R", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, cols, 5, 4, 2, 3, out, nullptr), NVRX_ERR_RANGE, "outside");
    // then the peer step's
    expect("R too large", nvrx_peer_attribute(table, NVRX_ROBUST_MAX_RANKS + 1, 5, 2, groups, 2, cols, 0, 8, 2, 3, out, nullptr), NVRX_ERR_RANGE, "ranks");
    expect("S too large", nvrx_peer_attribute(table, 8, 5, NVRX_MAX_ROWS + 1, groups, 2, cols, 0, 8, 2, 3, out, nullptr), NVRX_ERR_RANGE, "section");
    expect("min_ranks 0", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, cols, 0, 8, 0, 3, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("min_ranks before G", nvrx_peer_attribute(table, 8, 5, 2, groups, 0, cols, 0, 8, -2, 3, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("G 0", nvrx_peer_attribute(table, 8, 5, 2, groups, 0, cols, 0, 8, 2, 3, out, nullptr), NVRX_ERR_INVALID, "groups");
    expect("G > R", nvrx_peer_attribute(table, 8, 5, 2, groups, 9, cols, 0, 8, 2, 3, out, nullptr), NVRX_ERR_RANGE, "groups");
    expect("G above the cap", nvrx_peer_attribute(table, NVRX_ROBUST_MAX_RANKS, 5, 2, groups, NVRX_PEER_MAX_GROUPS + 1, cols, 0, 8, 2, 3, out, nullptr),
           NVRX_ERR_RANGE, "at most");
    // the pointers, last
    expect("null table", nvrx_peer_attribute(nullptr, 8, 5, 2, groups, 2, cols, 0, 8, 2, 3, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null groups", nvrx_peer_attribute(table, 8, 5, 2, nullptr, 2, cols, 0, 8, 2, 3, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null column records", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, nullptr, 0, 8, 2, 3, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, cols, 0, 8, 2, 3, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned records", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, cols, 0, 8, 2, 3, odd, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("misaligned column records", nvrx_peer_attribute(table, 8, 5, 2, groups, 2, odd, 0, 8, 2, 3, out, nullptr), NVRX_ERR_INVALID, "d_peer_cols");

    // nvrx_report_peer_attribute: every check that precedes the look at the context reads the descriptor's shape only, so a
    // context that was never created will do (the state check is the GPU tests' to cover)
    nvrx_ctx *ctx = reinterpret_cast<nvrx_ctx *>(uintptr_t{4096});
    nvrx_report_desc d;
    memset(&d, 0, sizeof d);
    d.R = 8, d.K = 5, d.S = 2;
    expect("null context", nvrx_report_peer_attribute(nullptr, &d, groups, 2, cols, 0, 8, 2, 3, out), NVRX_ERR_INVALID, "null");
    expect("null descriptor", nvrx_report_peer_attribute(ctx, nullptr, groups, 2, cols, 0, 8, 2, 3, out), NVRX_ERR_INVALID, "null");
    expect("report: top_n 17", nvrx_report_peer_attribute(ctx, &d, groups, 2, cols, 0, 8, 2, 17, out), NVRX_ERR_RANGE, "top_n");
    expect("report: ranks past R", nvrx_report_peer_attribute(ctx, &d, groups, 2, cols, 5, 4, 2, 3, out), NVRX_ERR_RANGE, "outside");
    expect("report: min_ranks 0", nvrx_report_peer_attribute(ctx, &d, groups, 2, cols, 0, 8, 0, 3, out), NVRX_ERR_RANGE, "min_ranks");
    expect("report: G 0", nvrx_report_peer_attribute(ctx, &d, groups, 0, cols, 0, 8, 2, 3, out), NVRX_ERR_INVALID, "groups");
    expect("report: G > R", nvrx_report_peer_attribute(ctx, &d, groups, 9, cols, 0, 8, 2, 3, out), NVRX_ERR_RANGE, "groups");
    expect("report: null groups", nvrx_report_peer_attribute(ctx, &d, nullptr, 2, cols, 0, 8, 2, 3, out), NVRX_ERR_INVALID, "null");
    expect("report: null column records", nvrx_report_peer_attribute(ctx, &d, groups, 2, nullptr, 0, 8, 2, 3, out), NVRX_ERR_INVALID, "null");
    expect("report: null records", nvrx_report_peer_attribute(ctx, &d, groups, 2, cols, 0, 8, 2, 3, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("report: misaligned records", nvrx_report_peer_attribute(ctx, &d, groups, 2, cols, 0, 8, 2, 3, odd), NVRX_ERR_INVALID, "aligned");
    expect("report: misaligned column records", nvrx_report_peer_attribute(ctx, &d, groups, 2, odd, 0, 8, 2, 3, out), NVRX_ERR_INVALID, "d_peer_cols");
    d.R = 0;
    expect("report: R 0", nvrx_report_peer_attribute(ctx, &d, groups, 1, cols, 0, 1, 2, 3, out), NVRX_ERR_INVALID, "shape");
    printf("peer_attribute_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
