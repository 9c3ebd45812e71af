// peer_history_args_check.cpp -- a stand-alone host program for `make peer-history-args-check`: it drives the argument checks
// of nvrx_peer_history, nvrx_report_peer_history, nvrx_peer_trend and nvrx_report_peer_trend with INVALID arguments only, so
// no call reaches a device, and is meant to be built together with nvrx_straggler.hip with AddressSanitizer and
// UndefinedBehaviorSanitizer on the host code.  Exit status 0 when every call returned the error the header promises.
#include <cmath>

#include "args_check.h"

int main() {
    float *peer = reinterpret_cast<float *>(uintptr_t{12288});  // never dereferenced: every call below fails its checks
    float *hist = reinterpret_cast<float *>(uintptr_t{4096});
    void *out = reinterpret_cast<void *>(uintptr_t{8192});
    float *odd_ring = reinterpret_cast<float *>(uintptr_t{4100});
    void *odd_out = reinterpret_cast<void *>(uintptr_t{8200});
    nvrx_ctx *ctx = reinterpret_cast<nvrx_ctx *>(uintptr_t{4096});
    const double thr[2] = {0.75, 0.7}, thr_nan[2] = {0.75, std::nan("")}, thr_inf[2] = {HUGE_VAL, 0.75};
    const int bad_depths[] = {1, 0, -4, 65, 1000};
    for (int H : bad_depths) {
        expect("peer_history H", nvrx_peer_history(peer, 8, 2, hist, 64, H, 3, thr, out, nullptr), NVRX_ERR_RANGE, "depth");
        expect("report_peer_history H", nvrx_report_peer_history(ctx, peer, 8, 2, hist, 64, H, 3, thr, out), NVRX_ERR_RANGE, "depth");
        expect("peer_trend H", nvrx_peer_trend(hist, 8, 2, 64, H, 3, out, nullptr), NVRX_ERR_RANGE, "depth");
        expect("report_peer_trend H", nvrx_report_peer_trend(ctx, hist, 8, 2, 64, H, 3, out), NVRX_ERR_RANGE, "depth");
    }
    // nvrx_peer_history
    expect("n_ranks 0", nvrx_peer_history(peer, 0, 2, hist, 64, 8, 3, thr, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("n_ranks < 0", nvrx_peer_history(peer, -1, 2, hist, 64, 8, 3, thr, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S < 0", nvrx_peer_history(peer, 8, -1, hist, 64, 8, 3, thr, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("S > S_cap", nvrx_peer_history(peer, 8, 65, hist, 64, 8, 3, thr, out, nullptr), NVRX_ERR_INVALID, "S_cap");
    expect("S_cap too large", nvrx_peer_history(peer, 8, 2, hist, NVRX_MAX_ROWS + 1, 8, 3, thr, out, nullptr), NVRX_ERR_RANGE, "S_cap");
    expect("null ring", nvrx_peer_history(peer, 8, 2, nullptr, 64, 8, 3, thr, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records", nvrx_peer_history(peer, 8, 2, hist, 64, 8, 3, thr, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned ring", nvrx_peer_history(peer, 8, 2, odd_ring, 64, 8, 3, thr, out, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("misaligned records", nvrx_peer_history(peer, 8, 2, hist, 64, 8, 3, thr, odd_out, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("NaN threshold", nvrx_peer_history(peer, 8, 2, hist, 64, 8, 3, thr_nan, out, nullptr), NVRX_ERR_INVALID, "finite");
    expect("infinite threshold", nvrx_peer_history(peer, 8, 2, hist, 64, 8, 3, thr_inf, out, nullptr), NVRX_ERR_INVALID, "finite");
    expect("too many waves", nvrx_peer_history(peer, 0x7FFFFFFF, NVRX_MAX_ROWS, hist, NVRX_MAX_ROWS, 64, 3, thr, out, nullptr),
           NVRX_ERR_RANGE, "one launch");
    expect("null scores", nvrx_peer_history(nullptr, 8, 2, hist, 64, 8, 3, thr, out, nullptr), NVRX_ERR_INVALID, "d_peer");
    expect("misaligned scores", nvrx_peer_history(reinterpret_cast<float *>(uintptr_t{12290}), 8, 2, hist, 64, 8, 3, nullptr, out,
                                                  nullptr), NVRX_ERR_INVALID, "d_peer");
    // nvrx_report_peer_history: every check precedes the look at the context, so a context that is never read will do
    expect("null context", nvrx_report_peer_history(nullptr, peer, 8, 2, hist, 64, 8, 3, thr, out), NVRX_ERR_INVALID, "null");
    expect("report n_ranks 0", nvrx_report_peer_history(ctx, peer, 0, 2, hist, 64, 8, 3, thr, out), NVRX_ERR_INVALID, "shape");
    expect("report S > S_cap", nvrx_report_peer_history(ctx, peer, 8, 3, hist, 2, 8, 3, thr, out), NVRX_ERR_INVALID, "S_cap");
    expect("report null ring", nvrx_report_peer_history(ctx, peer, 8, 2, nullptr, 64, 8, 3, thr, out), NVRX_ERR_INVALID, "null");
    expect("report misaligned records", nvrx_report_peer_history(ctx, peer, 8, 2, hist, 64, 8, 3, thr, odd_out), NVRX_ERR_INVALID,
           "aligned");
    expect("report NaN threshold", nvrx_report_peer_history(ctx, peer, 8, 2, hist, 64, 8, 3, thr_nan, out), NVRX_ERR_INVALID, "finite");
    expect("report null scores", nvrx_report_peer_history(ctx, nullptr, 8, 2, hist, 64, 8, 3, thr, out), NVRX_ERR_INVALID, "d_peer");
    // nvrx_peer_trend
    expect("trend n_ranks 0", nvrx_peer_trend(hist, 0, 2, 64, 8, 3, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("trend S < 0", nvrx_peer_trend(hist, 8, -1, 64, 8, 3, out, nullptr), NVRX_ERR_INVALID, "shape");
    expect("trend S > S_cap", nvrx_peer_trend(hist, 8, 65, 64, 8, 3, out, nullptr), NVRX_ERR_INVALID, "S_cap");
    expect("trend S_cap too large", nvrx_peer_trend(hist, 8, 2, NVRX_MAX_ROWS + 1, 8, 3, out, nullptr), NVRX_ERR_RANGE, "S_cap");
    expect("trend n_reports 0", nvrx_peer_trend(hist, 8, 2, 64, 8, 0, out, nullptr), NVRX_ERR_INVALID, "n_reports");
    expect("trend null ring", nvrx_peer_trend(nullptr, 8, 2, 64, 8, 3, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("trend null records", nvrx_peer_trend(hist, 8, 2, 64, 8, 3, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("trend misaligned ring", nvrx_peer_trend(odd_ring, 8, 2, 64, 8, 3, out, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("trend misaligned records", nvrx_peer_trend(hist, 8, 2, 64, 8, 3, odd_out, nullptr), NVRX_ERR_INVALID, "aligned");
    expect("trend too many waves", nvrx_peer_trend(hist, 0x7FFFFFFF, NVRX_MAX_ROWS, NVRX_MAX_ROWS, 64, 3, out, nullptr),
           NVRX_ERR_RANGE, "one launch");
    // nvrx_report_peer_trend
    expect("trend null context", nvrx_report_peer_trend(nullptr, hist, 8, 2, 64, 8, 3, out), NVRX_ERR_INVALID, "null");
    expect("trend report n_ranks 0", nvrx_report_peer_trend(ctx, hist, 0, 2, 64, 8, 3, out), NVRX_ERR_INVALID, "shape");
    expect("trend report S > S_cap", nvrx_report_peer_trend(ctx, hist, 8, 3, 2, 8, 3, out), NVRX_ERR_INVALID, "S_cap");
    expect("trend report n_reports 0", nvrx_report_peer_trend(ctx, hist, 8, 2, 64, 8, 0, out), NVRX_ERR_INVALID, "n_reports");
    expect("trend report null ring", nvrx_report_peer_trend(ctx, nullptr, 8, 2, 64, 8, 3, out), NVRX_ERR_INVALID, "null");
    expect("trend report misaligned records", nvrx_report_peer_trend(ctx, hist, 8, 2, 64, 8, 3, odd_out), NVRX_ERR_INVALID, "aligned");
    printf("peer_history_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
