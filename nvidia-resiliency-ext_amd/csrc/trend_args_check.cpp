// trend_args_check.cpp -- a stand-alone host program for `make trend-args-check`: it drives the argument checks of
// nvrx_score_trend and nvrx_report_trend with INVALID arguments only, so no call reaches a device, and is meant to be built
// together with nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.  Exit status 0 when
// every call returned the error the header promises.
#include "args_check.h"

int main() {
    float *hist = reinterpret_cast<float *>(uintptr_t{4096});  // never dereferenced: every call below fails its checks
    void *out = reinterpret_cast<void *>(uintptr_t{8192});
    nvrx_ctx *ctx = reinterpret_cast<nvrx_ctx *>(uintptr_t{4096});
    const int bad_depths[] = {1, 0, -4, 65, 1000};
    for (int H : bad_depths) {
        expect("score_trend H", nvrx_score_trend(hist, 8, 2, 64, H, 3, out, nullptr), NVRX_ERR_RANGE, "depth");
        expect("report_trend H", nvrx_report_trend(ctx, hist, 8, 2, 64, H, 3, out), NVRX_ERR_RANGE, "depth");
    }
    expect("n_ranks 0", nvrx_score_trend(hist, 0, 2, 64, 8, 3, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("n_ranks < 0", nvrx_score_trend(hist, -1, 2, 64, 8, 3, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S < 0", nvrx_score_trend(hist, 8, -1, 64, 8, 3, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S > S_cap", nvrx_score_trend(hist, 8, 65, 64, 8, 3, out, nullptr), NVRX_ERR_INVALID, "S_cap");
    expect("S_cap too large", nvrx_score_trend(hist, 8, 2, NVRX_MAX_ROWS + 1, 8, 3, out, nullptr), NVRX_ERR_RANGE, "S_cap");
    expect("n_reports 0", nvrx_score_trend(hist, 8, 2, 64, 8, 0, out, nullptr), NVRX_ERR_INVALID, "n_reports");
    expect("null ring", nvrx_score_trend(nullptr, 8, 2, 64, 8, 3, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records", nvrx_score_trend(hist, 8, 2, 64, 8, 3, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned ring", nvrx_score_trend(reinterpret_cast<float *>(uintptr_t{4100}), 8, 2, 64, 8, 3, out, nullptr),
           NVRX_ERR_INVALID, "aligned");
    expect("misaligned records", nvrx_score_trend(hist, 8, 2, 64, 8, 3, reinterpret_cast<void *>(uintptr_t{8200}), nullptr),
           NVRX_ERR_INVALID, "aligned");
    expect("too many waves", nvrx_score_trend(hist, 0x7FFFFFFF, NVRX_MAX_ROWS, NVRX_MAX_ROWS, 64, 3, out, nullptr), NVRX_ERR_RANGE,
           "one launch");
    expect("null context", nvrx_report_trend(nullptr, hist, 8, 2, 64, 8, 3, out), NVRX_ERR_INVALID, "null");
    expect("report n_ranks 0", nvrx_report_trend(ctx, hist, 0, 2, 64, 8, 3, out), NVRX_ERR_INVALID, "shape");
    expect("report S > S_cap", nvrx_report_trend(ctx, hist, 8, 3, 2, 8, 3, out), NVRX_ERR_INVALID, "S_cap");
    expect("report n_reports 0", nvrx_report_trend(ctx, hist, 8, 2, 64, 8, 0, out), NVRX_ERR_INVALID, "n_reports");
    expect("report null ring", nvrx_report_trend(ctx, nullptr, 8, 2, 64, 8, 3, out), NVRX_ERR_INVALID, "null");
    expect("report misaligned records", nvrx_report_trend(ctx, hist, 8, 2, 64, 8, 3, reinterpret_cast<void *>(uintptr_t{8200})),
           NVRX_ERR_INVALID, "aligned");
    printf("trend_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
