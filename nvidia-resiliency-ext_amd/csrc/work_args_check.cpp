// work_args_check.cpp -- a stand-alone host program for `make work-args-check`: it drives the argument checks of
// nvrx_work_groups and nvrx_report_work with INVALID arguments only, so no call reaches a device, and is meant to be built
// together with nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.  Exit status 0 when
// every call returned the error the header promises.
#include <cmath>

#include "args_check.h"

int main() {
    float *table = reinterpret_cast<float *>(uintptr_t{8192});  // never dereferenced: every call below fails its checks
    void *out = reinterpret_cast<void *>(uintptr_t{16384});
    void *odd = reinterpret_cast<void *>(uintptr_t{16392});
    expect("R 0", nvrx_work_groups(table, 0, 5, 2, 0.25f, 100000, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("R < 0", nvrx_work_groups(table, -3, 5, 2, 0.25f, 100000, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("K < 0", nvrx_work_groups(table, 8, -1, 2, 0.25f, 100000, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S < 0", nvrx_work_groups(table, 8, 5, -1, 0.25f, 100000, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("K too large", nvrx_work_groups(table, 8, NVRX_MAX_ROWS + 1, 2, 0.25f, 100000, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("S too large", nvrx_work_groups(table, 8, 5, NVRX_MAX_ROWS + 1, 0.25f, 100000, out, nullptr), NVRX_ERR_RANGE, "ids");
    expect("R above the table families' cap", nvrx_work_groups(table, NVRX_ROBUST_MAX_RANKS + 1, 5, 2, 0.25f, 100000, out, nullptr),
           NVRX_ERR_RANGE, "ranks");
    expect("R above the step's cap", nvrx_work_groups(table, NVRX_WORK_MAX_RANKS + 1, 5, 2, 0.25f, 100000, out, nullptr), NVRX_ERR_RANGE,
           "work groups");
    // (the shape comes before the parameters, and R before them too)
    expect("R above the cap, bad parameters", nvrx_work_groups(table, NVRX_WORK_MAX_RANKS + 1, 5, 2, -1.0f, -1, out, nullptr),
           NVRX_ERR_RANGE, "work groups");
    expect("count_tol < 0", nvrx_work_groups(table, 8, 5, 2, -0.5f, 100000, out, nullptr), NVRX_ERR_RANGE, "count_tol");
    expect("count_tol > 16", nvrx_work_groups(table, 8, 5, 2, 16.5f, 100000, out, nullptr), NVRX_ERR_RANGE, "count_tol");
    expect("count_tol NaN", nvrx_work_groups(table, 8, 5, 2, NAN, 100000, out, nullptr), NVRX_ERR_RANGE, "count_tol");
    expect("count_tol inf", nvrx_work_groups(table, 8, 5, 2, INFINITY, 100000, out, nullptr), NVRX_ERR_RANGE, "count_tol");
    expect("max_unlike_ppm < 0", nvrx_work_groups(table, 8, 5, 2, 0.25f, -1, out, nullptr), NVRX_ERR_RANGE, "max_unlike_ppm");
    expect("max_unlike_ppm > 1e6", nvrx_work_groups(table, 8, 5, 2, 0.25f, 1000001, out, nullptr), NVRX_ERR_RANGE, "max_unlike_ppm");
    expect("count_tol before max_unlike_ppm", nvrx_work_groups(table, 8, 5, 2, 17.0f, -1, out, nullptr), NVRX_ERR_RANGE, "count_tol");
    expect("null table", nvrx_work_groups(nullptr, 8, 5, 2, 0.25f, 100000, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null block", nvrx_work_groups(table, 8, 5, 2, 0.25f, 100000, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned block", nvrx_work_groups(table, 8, 5, 2, 0.25f, 100000, odd, nullptr), NVRX_ERR_INVALID, "aligned");
    // (the parameters come before the pointers)
    expect("bad parameter, null table", nvrx_work_groups(nullptr, 8, 5, 2, 0.25f, 1000001, out, nullptr), NVRX_ERR_RANGE, "max_unlike_ppm");

    expect("words: R 0", nvrx_work_words(0, 5, 2), NVRX_ERR_INVALID, "shape");
    expect("words: K < 0", nvrx_work_words(8, -1, 2), NVRX_ERR_INVALID, "shape");
    expect("words: S < 0", nvrx_work_words(8, 5, -2), NVRX_ERR_INVALID, "shape");
    expect("words: S too large", nvrx_work_words(8, 5, NVRX_MAX_ROWS + 1), NVRX_ERR_RANGE, "ids");
    expect("words: R above the step's cap", nvrx_work_words(NVRX_WORK_MAX_RANKS + 1, 5, 2), NVRX_ERR_RANGE, "work groups");
    if (nvrx_work_words(NVRX_WORK_MAX_RANKS, NVRX_MAX_ROWS, NVRX_MAX_ROWS) <= 0) {  // (the largest shape fits an int)
        fprintf(stderr, "FAIL nvrx_work_words of the largest shape = %d\n", nvrx_work_words(NVRX_WORK_MAX_RANKS, NVRX_MAX_ROWS, NVRX_MAX_ROWS));
        failures++;
    }
    // 8 x 7 signatures (56 words), 8 x 1 adjacency words (16), 8 x 1 partial records (32), 8 rank records (64), the job record (4)
    if (nvrx_work_words(8, 5, 2) != 56 + 16 + 32 + 64 + 4) {
        fprintf(stderr, "FAIL nvrx_work_words(8, 5, 2) = %d\n", nvrx_work_words(8, 5, 2));
        failures++;
    }
    // 65 x 3 signatures (195 -> 196), 65 x 2 adjacency words (260), 65 x 2 partial records (520), 65 rank records (520), 4
    if (nvrx_work_words(65, 1, 2) != 196 + 260 + 520 + 520 + 4) {
        fprintf(stderr, "FAIL nvrx_work_words(65, 1, 2) = %d\n", nvrx_work_words(65, 1, 2));
        failures++;
    }

    // nvrx_report_work: every check that precedes the look at the context reads the descriptor's shape only, so a context that
    // was never created will do (the state check -- a report issued through this descriptor -- is the GPU tests' to cover)
    nvrx_ctx *ctx = reinterpret_cast<nvrx_ctx *>(uintptr_t{4096});
    nvrx_report_desc d;
    memset(&d, 0, sizeof d);
    d.R = 8, d.K = 5, d.S = 2;
    expect("null context", nvrx_report_work(nullptr, &d, 0.25f, 100000, out), NVRX_ERR_INVALID, "null");
    expect("null descriptor", nvrx_report_work(ctx, nullptr, 0.25f, 100000, out), NVRX_ERR_INVALID, "null");
    expect("report: count_tol < 0", nvrx_report_work(ctx, &d, -1.0f, 100000, out), NVRX_ERR_RANGE, "count_tol");
    expect("report: count_tol NaN", nvrx_report_work(ctx, &d, NAN, 100000, out), NVRX_ERR_RANGE, "count_tol");
    expect("report: max_unlike_ppm > 1e6", nvrx_report_work(ctx, &d, 0.25f, 1000001, out), NVRX_ERR_RANGE, "max_unlike_ppm");
    expect("report: null block", nvrx_report_work(ctx, &d, 0.25f, 100000, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("report: misaligned block", nvrx_report_work(ctx, &d, 0.25f, 100000, odd), NVRX_ERR_INVALID, "aligned");
    d.R = NVRX_WORK_MAX_RANKS + 1;
    expect("report: R above the step's cap", nvrx_report_work(ctx, &d, 0.25f, 100000, out), NVRX_ERR_RANGE, "work groups");
    d.R = 0;
    expect("report: R 0", nvrx_report_work(ctx, &d, 0.25f, 100000, out), NVRX_ERR_INVALID, "shape");
    printf("work_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
