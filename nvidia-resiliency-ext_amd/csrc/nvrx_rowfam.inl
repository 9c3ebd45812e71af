// nvrx_rowfam.inl -- the host side that the row families (tail, onset, period, episode scores) share.  Part of the
// translation unit nvrx_straggler.hip (included ahead of the four families' files: it uses that file's context, fill kernel
// and error helpers, nvrx_tablefam.inl's ordering behind a report, and nvrx_tail.inl's score launch).  Host code only: every kernel and every kernel-argument struct
// stays with its family.
//
// A row family is one pipeline with its own ring kernel in front ("Row families"): ring kernel by gid into
// [local_ranks][P][K+S] behind a -1 fill -> the caller's all-gather -> k_tail_score on plane 0 with a pitch of P * (K+S).

namespace {

int tail_score_launch(const float *d_tails, int ld, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                      float *d_colmin_scratch, float *d_out, hipStream_t st);  // (nvrx_tail.inl)

// nvrx_row_{quantile,onset,period,episode}: the checks of a stateless row operator, in their order -- strides, the family's
// parameter (param_check() -> code), then, unless rows == 0 (nothing to do: the caller returns), the pointers
// (out_aligned16: d_out takes 16-byte records).
template <class ParamCheck>
int row_op_check(int rows, int row_stride, const float *d_samples, const uint32_t *d_counts, const void *d_out,
                 bool out_aligned16, ParamCheck param_check) {
    if (rows < 0) return fail(NVRX_ERR_INVALID, "rows=%d is negative", rows);
    if (row_stride <= 0 || row_stride % 4 != 0) return fail(NVRX_ERR_INVALID, "row_stride %d is not a positive multiple of 4", row_stride);
    if (row_stride > NVRX_MAX_RING_CAP) return fail(NVRX_ERR_RANGE, "row_stride %d exceeds %d", row_stride, NVRX_MAX_RING_CAP);
    const int rc = param_check();
    if (rc || rows == 0) return rc;
    if (!d_samples || !d_counts || !d_out) return fail(NVRX_ERR_INVALID, "null device pointer");
    if ((reinterpret_cast<uintptr_t>(d_samples) & 15u) != 0) return fail(NVRX_ERR_INVALID, "d_samples is not 16-byte aligned");
    if (out_aligned16 && (reinterpret_cast<uintptr_t>(d_out) & 15u) != 0) return fail(NVRX_ERR_INVALID, "d_out is not 16-byte aligned");
    return NVRX_OK;
}

int min_strength_check(float min_strength) {
    if (!(min_strength >= 0.0f && min_strength <= 1.0f)) return fail(NVRX_ERR_RANGE, "min_strength=%g outside [0,1]", (double)min_strength);
    return NVRX_OK;
}

// nvrx_{tail,onset,period,episode}_score: relative scores from plane 0 of a gathered [R][planes][K+S] table -- a [R][K+S]
// table with a pitch of planes * (K+S)
int plane_score(const float *d_planes, int planes, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                float *d_colmin_scratch, float *d_out, void *stream) {
    if (R <= 0 || K < 0 || S < 0) return fail(NVRX_ERR_INVALID, "bad table shape R=%d K=%d S=%d", R, K, S);
    if (K > NVRX_MAX_ROWS) return fail(NVRX_ERR_RANGE, "K=%d kernel ids, at most %d", K, NVRX_MAX_ROWS);
    if (first_rank < 0 || n_ranks < 1 || first_rank > R - n_ranks)
        return fail(NVRX_ERR_RANGE, "ranks [%d,%d+%d) outside the table's %d", first_rank, first_rank, n_ranks, R);
    if (!d_planes || !d_table || !d_out) return fail(NVRX_ERR_INVALID, "null device pointer");
    const int KS = K + S;
    if (KS > 0 && !d_colmin_scratch) return fail(NVRX_ERR_INVALID, "d_colmin_scratch is null");
    return tail_score_launch(d_planes, planes * KS, d_table, R, K, S, first_rank, n_ranks, d_colmin_scratch, d_out, as_stream(stream));
}

// the window the context's last report read, as a family's ring kernel needs it (copied into the family's argument struct)
struct LocalWindow {
    const float *samples;
    const uint32_t *counts;
    const int32_t *gid;
    const uint32_t *starts;  // slot of every ring's oldest sample; null: 0 everywhere (or the family does not ask)
    int row_stride, uniform_n, rows_active, rows_per_rank;
};

template <class Args>
void window_args(const LocalWindow &w, Args *a) {
    a->samples = w.samples, a->counts = w.counts, a->gid = w.gid;
    a->row_stride = w.row_stride, a->uniform_n = w.uniform_n;
    a->rows_active = w.rows_active, a->rows_per_rank = w.rows_per_rank;
}

// The front of nvrx_{tail,onset,period,episode}_local, in its order: null and K/S checks, the family's parameters
// (param_check() -> code), the rows_active range and default; then, under the context's lock: the ring-start snapshot must be
// on where the family needs it (starts_off_msg: what to say if it is not; null: not needed), the descriptor is the last
// report's, *stream is put behind that report's last kernel (behind_report, nvrx_tablefam.inl), and a wrapped ring's
// starts are uploaded.  Nothing is flushed: counts and ring starts are those of the window the report's statistics kernel read.
template <class ParamCheck>
int local_window(nvrx_ctx *ctx, const nvrx_report_desc *desc, const float *d_send, int K, int S, int rows_active,
                 ParamCheck param_check, const char *starts_off_msg, hipStream_t *stream, LocalWindow *win) {
    if (!ctx || !d_send) return fail(NVRX_ERR_INVALID, "null argument");
    if (K < 0 || S < 0) return fail(NVRX_ERR_INVALID, "bad K/S");
    if (K > NVRX_MAX_ROWS) return fail(NVRX_ERR_RANGE, "K=%d kernel ids, at most %d", K, NVRX_MAX_ROWS);
    const int rc = param_check();
    if (rc) return rc;
    if (rows_active < 0 || rows_active > ctx->rows_per_rank)
        return fail(NVRX_ERR_INVALID, "rows_active %d outside [0,%d]", rows_active, ctx->rows_per_rank);
    if (rows_active == 0) rows_active = ctx->rows_per_rank;
    hipStream_t st = *stream;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (starts_off_msg && !ctx->onset_on) return fail(NVRX_ERR_STATE, "%s", starts_off_msg);
    if (desc) {
        if (const int rc = behind_report(ctx, desc, &st)) return rc;
    } else {
        HIP_TRY(hipSetDevice(ctx->device));
    }
    *win = LocalWindow{};
    win->uniform_n = ctx->tail_uniform_n;
    win->samples = ctx->d_samples, win->counts = ctx->d_counts, win->gid = ctx->d_gid;
    win->row_stride = ctx->row_stride;
    win->rows_active = rows_active, win->rows_per_rank = ctx->rows_per_rank;
    if (starts_off_msg && ctx->onset_wrapped) {  // (rare: a window longer than the ring)
        HIP_TRY(hipMemcpyAsync(ctx->d_onset_starts, ctx->h_onset_starts, (size_t)ctx->onset_rows * sizeof(uint32_t),
                               hipMemcpyHostToDevice, st));
        if (ctx->onset_rows < ctx->rows)
            HIP_TRY(hipMemsetAsync(ctx->d_onset_starts + ctx->onset_rows, 0, (size_t)(ctx->rows - ctx->onset_rows) * sizeof(uint32_t), st));
        win->starts = ctx->d_onset_starts;
    }
    *stream = st;
    return NVRX_OK;
}

// every slot of a family's send rows is written: -1 where no row with samples points
int fill_minus_one(float *d_send, size_t slots, hipStream_t st) {
    hipLaunchKernelGGL(k_fill_f32, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, d_send, slots, -1.0f);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

const char *const STARTS_OFF = "the ring-start snapshot is not enabled on this context (nvrx_onset_enable)";

}  // namespace
