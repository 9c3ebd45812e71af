// nvrx_tablefam.inl -- the host side that the table families (robust, peer, pace, pace-per-group and node scores) share.
// Part of the translation unit nvrx_straggler.hip (included ahead of nvrx_attribute.inl and nvrx_rowfam.inl, which order
// themselves behind a report the same way: it uses that file's context and error helpers).  Host code only: every kernel,
// every kernel-argument struct and every choice of a kernel variant stays with its family.
//
// A table family reads the gathered [R][K+S] table nvrx_score reads and rates ranks against each other ("Table
// families").  Its two entry points -- nvrx_<family>_score on a caller's table and stream, nvrx_report_<family> behind the
// context's last report -- check their arguments in one order: the table's shape and the rank range (table_check), the
// family's thresholds, its groups (groups_check), then the pointers (out_check).

namespace {

int table_check(int R, int K, int S, int first_rank, int n_ranks) {
    if (R <= 0 || K < 0 || S < 0) return fail(NVRX_ERR_INVALID, "bad table shape R=%d K=%d S=%d", R, K, S);
    if (R > NVRX_ROBUST_MAX_RANKS) return fail(NVRX_ERR_RANGE, "R=%d ranks, at most %d", R, NVRX_ROBUST_MAX_RANKS);
    if (K > NVRX_MAX_ROWS || S > NVRX_MAX_ROWS) return fail(NVRX_ERR_RANGE, "K=%d S=%d ids, at most %d each", K, S, NVRX_MAX_ROWS);
    if (first_rank < 0 || n_ranks < 1 || first_rank > R - n_ranks)
        return fail(NVRX_ERR_RANGE, "ranks [%d,%d+%d) outside the table's %d", first_rank, first_rank, n_ranks, R);
    return NVRX_OK;
}

// table_check, then the threshold robust, peer and pace scores share
int table_min_ranks_check(int R, int K, int S, int first_rank, int n_ranks, int min_ranks) {
    const int rc = table_check(R, K, S, first_rank, n_ranks);
    if (rc) return rc;
    if (min_ranks < 1) return fail(NVRX_ERR_RANGE, "min_ranks=%d, at least 1", min_ranks);
    return NVRX_OK;
}

int groups_check(int R, int G) {
    if (G < 1) return fail(NVRX_ERR_INVALID, "G=%d groups, at least 1", G);
    if (G > R) return fail(NVRX_ERR_RANGE, "G=%d groups for R=%d ranks", G, R);
    if (G > NVRX_PEER_MAX_GROUPS) return fail(NVRX_ERR_RANGE, "G=%d groups, at most %d", G, NVRX_PEER_MAX_GROUPS);
    return NVRX_OK;
}

// The pointers, last of an entry's checks: d_out takes 16-byte records.  `others`: the entry's other device pointers are all
// there.  A stateless entry counts a null d_out among them; a report entry (`report`) says of d_out both things at once.
int out_check(const void *d_out, bool others, bool report) {
    const bool misaligned = (reinterpret_cast<uintptr_t>(d_out) & 15u) != 0;
    if (!others || (!report && !d_out)) return fail(NVRX_ERR_INVALID, "null device pointer");
    if (report && (!d_out || misaligned)) return fail(NVRX_ERR_INVALID, "d_out is null or not 16-byte aligned");
    if (misaligned) return fail(NVRX_ERR_INVALID, "d_out is not 16-byte aligned");
    return NVRX_OK;
}

// Under the context's lock: `desc` is the last report's, and *home -- the context's default stream, where every follow-up
// of a report runs -- is put behind that report's last kernel.  Where that kernel ran elsewhere (re-homed onto the caller's
// stream, or the resident scorer's own): kernel-boundary ordering through an event, never the completion word (its stores
// are not fenced).
int behind_report(nvrx_ctx *ctx, const nvrx_report_desc *desc, hipStream_t *home) {
    if (ctx->attr_desc != desc) return fail(NVRX_ERR_STATE, "no report was issued through this descriptor on this context");
    const hipStream_t last = ctx->attr_stream;
    *home = ctx->default_stream;
    HIP_TRY(hipSetDevice(ctx->device));
    if (last != *home) {
        if (!ctx->attr_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->attr_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ctx->attr_ev, last));
        HIP_TRY(hipStreamWaitEvent(*home, ctx->attr_ev, 0));
    }
    return NVRX_OK;
}

// nvrx_report_<follow-up>: behind_report under the lock, and the table that report scored (`table` null: not asked for)
int report_table(nvrx_ctx *ctx, const nvrx_report_desc *desc, hipStream_t *home, const float **table) {
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        const int rc = behind_report(ctx, desc, home);
        if (rc) return rc;
    }
    if (table) *table = desc->allgather_fn ? desc->d_table : desc->d_send;
    return NVRX_OK;
}

}  // namespace
