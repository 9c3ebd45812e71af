// stall_args_check.cpp -- a stand-alone host program for `make stall-args-check`: it drives the argument checks of
// nvrx_row_stall, nvrx_stall_score and nvrx_stall_local with INVALID arguments only, so no call reaches a device, and is meant to
// be built together with nvrx_straggler.hip with AddressSanitizer and UndefinedBehaviorSanitizer on the host code.  Exit status
// 0 when every call returned the error the header promises.
#include "args_check.h"
#include <cmath>

int main() {
    float *samples = reinterpret_cast<float *>(uintptr_t{4096});  // never dereferenced: every call below fails its checks
    uint32_t *counts = reinterpret_cast<uint32_t *>(uintptr_t{8192});
    void *out = reinterpret_cast<void *>(uintptr_t{16384});
    void *odd = reinterpret_cast<void *>(uintptr_t{16392});
    const uint32_t ratio = 1500000u;
    // (samples, counts, starts, rows, row_stride, ratio_ppm, min_z, out, stream): the order of row_op_check
    expect("rows < 0", nvrx_row_stall(samples, counts, nullptr, -1, 64, ratio, 6.0f, out, nullptr), NVRX_ERR_INVALID, "negative");
    expect("stride 0", nvrx_row_stall(samples, counts, nullptr, 4, 0, ratio, 6.0f, out, nullptr), NVRX_ERR_INVALID, "multiple of 4");
    expect("stride % 4", nvrx_row_stall(samples, counts, nullptr, 4, 66, ratio, 6.0f, out, nullptr), NVRX_ERR_INVALID, "multiple of 4");
    expect("stride too large", nvrx_row_stall(samples, counts, nullptr, 4, NVRX_MAX_RING_CAP + 4, ratio, 6.0f, out, nullptr), NVRX_ERR_RANGE, "exceeds");
    expect("ratio 1.0", nvrx_row_stall(samples, counts, nullptr, 4, 64, 1000000u, 6.0f, out, nullptr), NVRX_ERR_RANGE, "ratio_ppm");
    expect("ratio 0", nvrx_row_stall(samples, counts, nullptr, 4, 64, 0u, 6.0f, out, nullptr), NVRX_ERR_RANGE, "ratio_ppm");
    expect("ratio too large", nvrx_row_stall(samples, counts, nullptr, 4, 64, 1000000001u, 6.0f, out, nullptr), NVRX_ERR_RANGE, "ratio_ppm");
    expect("min_z < 0", nvrx_row_stall(samples, counts, nullptr, 4, 64, ratio, -0.5f, out, nullptr), NVRX_ERR_RANGE, "min_z");
    expect("min_z NaN", nvrx_row_stall(samples, counts, nullptr, 4, 64, ratio, NAN, out, nullptr), NVRX_ERR_RANGE, "min_z");
    expect("min_z inf", nvrx_row_stall(samples, counts, nullptr, 4, 64, ratio, INFINITY, out, nullptr), NVRX_ERR_RANGE, "min_z");
    expect("null samples", nvrx_row_stall(nullptr, counts, nullptr, 4, 64, ratio, 6.0f, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null counts", nvrx_row_stall(samples, nullptr, nullptr, 4, 64, ratio, 6.0f, out, nullptr), NVRX_ERR_INVALID, "null");
    expect("null records", nvrx_row_stall(samples, counts, nullptr, 4, 64, ratio, 6.0f, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("misaligned samples", nvrx_row_stall(reinterpret_cast<float *>(uintptr_t{4100}), counts, nullptr, 4, 64, ratio, 6.0f, out, nullptr),
           NVRX_ERR_INVALID, "aligned");
    expect("misaligned records", nvrx_row_stall(samples, counts, nullptr, 4, 64, ratio, 6.0f, odd, nullptr), NVRX_ERR_INVALID, "aligned");
    // the order: strides win over the parameters, ratio_ppm over min_z, the parameters over the pointers; a bad parameter is
    // reported for no rows as well, and no rows with good parameters is nothing to do
    expect("rows before stride", nvrx_row_stall(nullptr, nullptr, nullptr, -1, 66, 0u, NAN, odd, nullptr), NVRX_ERR_INVALID, "negative");
    expect("stride before ratio", nvrx_row_stall(nullptr, nullptr, nullptr, 4, 66, 0u, NAN, odd, nullptr), NVRX_ERR_INVALID, "multiple of 4");
    expect("ratio before min_z", nvrx_row_stall(nullptr, nullptr, nullptr, 4, 64, 0u, NAN, odd, nullptr), NVRX_ERR_RANGE, "ratio_ppm");
    expect("min_z before pointers", nvrx_row_stall(nullptr, nullptr, nullptr, 4, 64, ratio, NAN, odd, nullptr), NVRX_ERR_RANGE, "min_z");
    expect("no rows, bad ratio", nvrx_row_stall(nullptr, nullptr, nullptr, 0, 64, 0u, 6.0f, nullptr, nullptr), NVRX_ERR_RANGE, "ratio_ppm");
    expect("no rows", nvrx_row_stall(nullptr, nullptr, nullptr, 0, 64, ratio, 6.0f, nullptr, nullptr), NVRX_OK, nullptr);

    // nvrx_stall_score: plane_score's checks
    float *planes = reinterpret_cast<float *>(uintptr_t{4096}), *table = reinterpret_cast<float *>(uintptr_t{8192});
    float *scratch = reinterpret_cast<float *>(uintptr_t{12288}), *scores = reinterpret_cast<float *>(uintptr_t{16384});
    expect("score: R 0", nvrx_stall_score(planes, table, 0, 5, 2, 0, 1, scratch, scores, nullptr), NVRX_ERR_INVALID, "shape");
    expect("score: K < 0", nvrx_stall_score(planes, table, 8, -1, 2, 0, 8, scratch, scores, nullptr), NVRX_ERR_INVALID, "shape");
    expect("score: S < 0", nvrx_stall_score(planes, table, 8, 5, -1, 0, 8, scratch, scores, nullptr), NVRX_ERR_INVALID, "shape");
    expect("score: K too large", nvrx_stall_score(planes, table, 8, NVRX_MAX_ROWS + 1, 2, 0, 8, scratch, scores, nullptr), NVRX_ERR_RANGE, "ids");
    expect("score: first_rank < 0", nvrx_stall_score(planes, table, 8, 5, 2, -1, 4, scratch, scores, nullptr), NVRX_ERR_RANGE, "outside");
    expect("score: n_ranks 0", nvrx_stall_score(planes, table, 8, 5, 2, 0, 0, scratch, scores, nullptr), NVRX_ERR_RANGE, "outside");
    expect("score: ranks past R", nvrx_stall_score(planes, table, 8, 5, 2, 5, 4, scratch, scores, nullptr), NVRX_ERR_RANGE, "outside");
    expect("score: null planes", nvrx_stall_score(nullptr, table, 8, 5, 2, 0, 8, scratch, scores, nullptr), NVRX_ERR_INVALID, "null");
    expect("score: null table", nvrx_stall_score(planes, nullptr, 8, 5, 2, 0, 8, scratch, scores, nullptr), NVRX_ERR_INVALID, "null");
    expect("score: null scores", nvrx_stall_score(planes, table, 8, 5, 2, 0, 8, scratch, nullptr, nullptr), NVRX_ERR_INVALID, "null");
    expect("score: null scratch", nvrx_stall_score(planes, table, 8, 5, 2, 0, 8, nullptr, scores, nullptr), NVRX_ERR_INVALID, "scratch");

    // nvrx_stall_local: the checks that read nothing of the context come first, so a context that was never created will do
    // (rows_active, the snapshot's state and the descriptor are the GPU tests' to cover)
    nvrx_ctx *ctx = reinterpret_cast<nvrx_ctx *>(uintptr_t{4096});
    float *send = reinterpret_cast<float *>(uintptr_t{8192});
    expect("local: null context", nvrx_stall_local(nullptr, nullptr, ratio, 6.0f, 0.01f, send, 5, 2, 0, nullptr), NVRX_ERR_INVALID, "null");
    expect("local: null send", nvrx_stall_local(ctx, nullptr, ratio, 6.0f, 0.01f, nullptr, 5, 2, 0, nullptr), NVRX_ERR_INVALID, "null");
    expect("local: K < 0", nvrx_stall_local(ctx, nullptr, ratio, 6.0f, 0.01f, send, -1, 2, 0, nullptr), NVRX_ERR_INVALID, "K/S");
    expect("local: S < 0", nvrx_stall_local(ctx, nullptr, ratio, 6.0f, 0.01f, send, 5, -1, 0, nullptr), NVRX_ERR_INVALID, "K/S");
    expect("local: K too large", nvrx_stall_local(ctx, nullptr, ratio, 6.0f, 0.01f, send, NVRX_MAX_ROWS + 1, 2, 0, nullptr), NVRX_ERR_RANGE, "ids");
    expect("local: ratio 1.0", nvrx_stall_local(ctx, nullptr, 1000000u, 6.0f, 0.01f, send, 5, 2, 0, nullptr), NVRX_ERR_RANGE, "ratio_ppm");
    expect("local: min_z < 0", nvrx_stall_local(ctx, nullptr, ratio, -1.0f, 0.01f, send, 5, 2, 0, nullptr), NVRX_ERR_RANGE, "min_z");
    expect("local: min_z NaN", nvrx_stall_local(ctx, nullptr, ratio, NAN, 0.01f, send, 5, 2, 0, nullptr), NVRX_ERR_RANGE, "min_z");
    expect("local: min_share < 0", nvrx_stall_local(ctx, nullptr, ratio, 6.0f, -0.1f, send, 5, 2, 0, nullptr), NVRX_ERR_RANGE, "min_share");
    expect("local: min_share 1", nvrx_stall_local(ctx, nullptr, ratio, 6.0f, 1.0f, send, 5, 2, 0, nullptr), NVRX_ERR_RANGE, "min_share");
    expect("local: min_share NaN", nvrx_stall_local(ctx, nullptr, ratio, 6.0f, NAN, send, 5, 2, 0, nullptr), NVRX_ERR_RANGE, "min_share");
    expect("local: K/S before ratio", nvrx_stall_local(ctx, nullptr, 0u, NAN, NAN, send, -1, 2, 0, nullptr), NVRX_ERR_INVALID, "K/S");
    expect("local: ratio before min_z", nvrx_stall_local(ctx, nullptr, 0u, NAN, NAN, send, 5, 2, 0, nullptr), NVRX_ERR_RANGE, "ratio_ppm");
    expect("local: min_z before min_share", nvrx_stall_local(ctx, nullptr, ratio, NAN, NAN, send, 5, 2, 0, nullptr), NVRX_ERR_RANGE, "min_z");
    printf("stall_args_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
