// report_split_args_check.cpp -- a stand-alone host program for `make report-split-args-check`: it drives the argument checks
// of nvrx_report_issue and nvrx_report_wait (and of nvrx_report, which is the two back to back) with INVALID arguments only,
// so no call reaches a device, and is meant to be built together with nvrx_straggler.hip with AddressSanitizer and
// UndefinedBehaviorSanitizer on the host code.  Exit status 0 when every call returned the error the header promises.
// What it cannot reach without a device is a context: nvrx_report_wait's NVRX_ERR_STATE answers (nothing pending, another
// descriptor) read the context, and are checked where there is one (tests/test_gpu_report_split.py).
#include "args_check.h"

int main() {
    nvrx_ctx *ctx = reinterpret_cast<nvrx_ctx *>(uintptr_t{4096});  // never dereferenced: every call below fails its checks first
    uint32_t word = 0;
    nvrx_report_desc good;
    memset(&good, 0, sizeof(good));
    good.R = 2, good.K = 0, good.S = 4, good.names_ok = 1, good.do_indiv = good.do_rel = 1;
    good.d_stats = reinterpret_cast<float *>(uintptr_t{8192});
    good.d_send = reinterpret_cast<float *>(uintptr_t{12288});
    good.d_table = reinterpret_cast<float *>(uintptr_t{16384});
    good.d_scores = reinterpret_cast<float *>(uintptr_t{20480});
    good.d_flags = reinterpret_cast<uint8_t *>(uintptr_t{24576});
    good.d_meta = reinterpret_cast<uint32_t *>(uintptr_t{28672});
    good.h_seq_word = &word;
    good.seq = 7;
    void *gather = reinterpret_cast<void *>(uintptr_t{32768});  // (an all-gather's address: never called)

    nvrx_report_desc d = good;
    expect("issue: null context", nvrx_report_issue(nullptr, &d, nullptr), NVRX_ERR_INVALID, "null argument");
    expect("issue: null descriptor", nvrx_report_issue(ctx, nullptr, nullptr), NVRX_ERR_INVALID, "null argument");
    expect("issue: both null", nvrx_report_issue(nullptr, nullptr, nullptr), NVRX_ERR_INVALID, "null argument");
    d = good, d.d_stats = nullptr;
    expect("issue: null statistics", nvrx_report_issue(ctx, &d, nullptr), NVRX_ERR_INVALID, "null buffer");
    d = good, d.d_send = nullptr;
    expect("issue: null exchange rows", nvrx_report_issue(ctx, &d, nullptr), NVRX_ERR_INVALID, "null buffer");
    d = good, d.d_scores = nullptr;
    expect("issue: null scores", nvrx_report_issue(ctx, &d, nullptr), NVRX_ERR_INVALID, "null buffer");
    d = good, d.d_meta = nullptr;
    expect("issue: null meta", nvrx_report_issue(ctx, &d, nullptr), NVRX_ERR_INVALID, "null buffer");
    d = good, d.allgather_fn = gather, d.send_count = 16, d.d_table = nullptr;
    expect("issue: exchange without a table", nvrx_report_issue(ctx, &d, nullptr), NVRX_ERR_INVALID, "separate table");
    d = good, d.allgather_fn = gather, d.send_count = 16, d.d_table = d.d_send;
    expect("issue: exchange into its own rows", nvrx_report_issue(ctx, &d, nullptr), NVRX_ERR_INVALID, "separate table");
    d = good, d.allgather_fn = gather, d.send_count = 0;
    expect("issue: exchange of nothing", nvrx_report_issue(ctx, &d, nullptr), NVRX_ERR_INVALID, "send_count");
    d = good, d.h_seq_word = nullptr;
    expect("issue: no completion word", nvrx_report_issue(ctx, &d, nullptr), NVRX_ERR_INVALID, "h_seq_word");
    // the buffers are looked at first: an asynchronous descriptor with a null buffer is told about the buffer
    d = good, d.h_seq_word = nullptr, d.d_meta = nullptr;
    expect("issue: null buffer before the word", nvrx_report_issue(ctx, &d, nullptr), NVRX_ERR_INVALID, "null buffer");
    // a refused issue advanced nothing
    d = good, d.d_scores = nullptr;
    (void)nvrx_report_issue(ctx, &d, nullptr);
    if (d.seq != good.seq) {
        fprintf(stderr, "FAIL a refused issue moved desc.seq from %u to %u\n", good.seq, d.seq);
        failures++;
    }

    d = good;
    expect("wait: null context", nvrx_report_wait(nullptr, &d), NVRX_ERR_INVALID, "null argument");
    expect("wait: null descriptor", nvrx_report_wait(ctx, nullptr), NVRX_ERR_INVALID, "null argument");
    expect("wait: both null", nvrx_report_wait(nullptr, nullptr), NVRX_ERR_INVALID, "null argument");

    // the one-call form is the two phases: the same answers, synchronous or not
    expect("report: null context", nvrx_report(nullptr, &d, nullptr), NVRX_ERR_INVALID, "null argument");
    expect("report: null descriptor", nvrx_report(ctx, nullptr, nullptr), NVRX_ERR_INVALID, "null argument");
    d = good, d.d_send = nullptr;
    expect("report: null buffer, synchronous", nvrx_report(ctx, &d, nullptr), NVRX_ERR_INVALID, "null buffer");
    d = good, d.h_seq_word = nullptr, d.d_send = nullptr;
    expect("report: null buffer, asynchronous", nvrx_report(ctx, &d, nullptr), NVRX_ERR_INVALID, "null buffer");
    d = good, d.allgather_fn = gather, d.send_count = 16, d.d_table = nullptr;
    expect("report: exchange without a table", nvrx_report(ctx, &d, nullptr), NVRX_ERR_INVALID, "separate table");
    printf("report_split_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
