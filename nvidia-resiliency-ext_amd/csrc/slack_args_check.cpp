// slack_args_check.cpp -- a stand-alone host program for `make slack-args-check`: it drives the argument checks of
// nvrx_slack_score and nvrx_slack_local with INVALID arguments only, so no call reaches a device, and is meant to be built
// together with nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.  Exit status 0 when
// every call returned the error the header promises.
#include "args_check.h"

int main() {
    float *slack = reinterpret_cast<float *>(uintptr_t{4096});  // never dereferenced: every call below fails its checks
    float *table = reinterpret_cast<float *>(uintptr_t{8192});
    void *out = reinterpret_cast<void *>(uintptr_t{16384});
    expect("R 0", nvrx_slack_score(slack, table, 0, 5, 2, 4, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R < 0", nvrx_slack_score(slack, table, -3, 5, 2, 4, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("K < 0", nvrx_slack_score(slack, table, 8, -1, 2, 4, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S < 0", nvrx_slack_score(slack, table, 8, 5, -1, 4, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R too large", nvrx_slack_score(slack, table, NVRX_ROBUST_MAX_RANKS + 1, 5, 2, 4, out, nullptr), NVRX_ERR_RANGE, "ranks");
    expect("K too large", nvrx_slack_score(slack, table, 8, NVRX_MAX_ROWS + 1, 2, 4, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("S too large", nvrx_slack_score(slack, table, 8, 5, NVRX_MAX_ROWS + 1, 4, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("min_ranks 0", nvrx_slack_score(slack, table, 8, 5, 2, 0, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("min_ranks < 0", nvrx_slack_score(slack, table, 8, 5, 2, -4, out, nullptr), NVRX_ERR_RANGE, "min_ranks");
    expect("null rows", nvrx_slack_score(nullptr, table, 8, 5, 2, 4, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null table", nvrx_slack_score(slack, nullptr, 8, 5, 2, 4, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records", nvrx_slack_score(slack, table, 8, 5, 2, 4, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records, K 0", nvrx_slack_score(slack, nullptr, 8, 0, 2, 4, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned rows", nvrx_slack_score(reinterpret_cast<float *>(uintptr_t{4100}), table, 8, 5, 2, 4, out, nullptr),
           NVRX_ERR_INVALID, "aligned");
    expect("misaligned records", nvrx_slack_score(slack, table, 8, 5, 2, 4, reinterpret_cast<void *>(uintptr_t{16392}), nullptr),
           NVRX_ERR_INVALID, "aligned");

    // nvrx_slack_local: the checks that read nothing of the context come first, so a context that was never created will do
    // (what depends on the context's geometry -- n and rows against rows_per_rank, rows_active, the descriptor -- is the GPU
    // tests' to cover)
    nvrx_ctx *ctx = reinterpret_cast<nvrx_ctx *>(uintptr_t{4096});
    const int32_t rows[3] = {1, 2, 5}, cols[3] = {0, 63, 7};
    float *stats = reinterpret_cast<float *>(uintptr_t{4096});
    float *send = reinterpret_cast<float *>(uintptr_t{8192});
    expect("null context", nvrx_slack_local(nullptr, nullptr, stats, rows, cols, 3, send, 0, nullptr), NVRX_ERR_INVALID, "null");
    expect("null send", nvrx_slack_local(ctx, nullptr, stats, rows, cols, 3, nullptr, 0, nullptr), NVRX_ERR_INVALID, "null");
    expect("n < 0", nvrx_slack_local(ctx, nullptr, stats, rows, cols, -1, send, 0, nullptr), NVRX_ERR_INVALID, "outside");
    expect("null list", nvrx_slack_local(ctx, nullptr, stats, nullptr, cols, 3, send, 0, nullptr), NVRX_ERR_INVALID, "null");
    expect("null columns", nvrx_slack_local(ctx, nullptr, stats, rows, nullptr, 3, send, 0, nullptr), NVRX_ERR_INVALID, "null");
    const int32_t rows_neg[3] = {-1, 2, 5}, rows_desc[3] = {1, 5, 2}, rows_twice[3] = {1, 2, 2};
    const int32_t cols_hi[3] = {0, 64, 7}, cols_neg[3] = {0, 63, -7};
    expect("row < 0", nvrx_slack_local(ctx, nullptr, stats, rows_neg, cols, 3, send, 0, nullptr), NVRX_ERR_RANGE, "rows[0]");
    expect("rows descending", nvrx_slack_local(ctx, nullptr, stats, rows_desc, cols, 3, send, 0, nullptr), NVRX_ERR_INVALID, "ascending");
    expect("row twice", nvrx_slack_local(ctx, nullptr, stats, rows_twice, cols, 3, send, 0, nullptr), NVRX_ERR_INVALID, "ascending");
    expect("column too large", nvrx_slack_local(ctx, nullptr, stats, rows, cols_hi, 3, send, 0, nullptr), NVRX_ERR_RANGE, "cols[1]");
    expect("column < 0", nvrx_slack_local(ctx, nullptr, stats, rows, cols_neg, 3, send, 0, nullptr), NVRX_ERR_RANGE, "cols[2]");
    expect("null statistics", nvrx_slack_local(ctx, nullptr, nullptr, rows, cols, 3, send, 0, nullptr), NVRX_ERR_INVALID, "statistics");
    expect("misaligned send", nvrx_slack_local(ctx, nullptr, stats, rows, cols, 3, reinterpret_cast<float *>(uintptr_t{8196}), 0, nullptr),
           NVRX_ERR_INVALID, "aligned");
    printf("slack_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
