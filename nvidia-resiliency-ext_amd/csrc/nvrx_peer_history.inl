// nvrx_peer_history.inl -- peer-score history and trends: the score history (nvrx_history.inl) and the score trends
// (nvrx_trend.inl) on the PEER-GROUP scores.  Part of the translation unit nvrx_straggler.hip (included at its end, behind
// nvrx_history.inl and nvrx_trend.inl: it uses their kernels' cell code, checks and launches).
//
// In a job whose ranks legitimately differ (pipeline stages, expert groups, roles) the job-wide relative scores rate a whole
// stage low for ever; the scores that mean something are the peer step's (nvrx_peer.inl).  That step leaves them as a rank
// part f32 [n_ranks][1 + S] behind its column records; a ring of their own, f32 [n_ranks][1 + S_cap][Hs], keeps the last H
// reports of them.  There is ONE definition of a record: the cell (r, j) here is the cell (r, f = 1, j) of the score history
// on score rows whose relative columns hold the peer values.
//
// k_peer_history<HS>  history_cell<HS, true> (nvrx_history.inl): k_score_history's geometry without the family bit; the lane
//   of age 0 reads x from d_peer[r * (1 + S) + j], so a wave's loads of this report's scores are one run of consecutive
//   floats.
// k_peer_trend<HS>    trend_cell<HS> (nvrx_trend.inl), unchanged: it only indexes the ring and the records by the wave's
//   (rank, family) number, which here is the rank.
// No LDS memory, no barrier, no atomics, no scratch, no loop or branch that depends on the ring's contents.

namespace {

int peer_history_check(const float *d_peer, int n_ranks, int S, const void *d_hist, int S_cap, int H, const double *thresholds,
                       const void *d_out) {
    const int rc = history_check(n_ranks, S, 0, n_ranks, d_hist, S_cap, H, thresholds, d_out, 1);
    if (rc) return rc;
    if (!d_peer || (reinterpret_cast<uintptr_t>(d_peer) & 3u) != 0) return fail(NVRX_ERR_INVALID, "d_peer is null or misaligned");
    return NVRX_OK;
}

// The context's stream, where nvrx_report_peer launched: a launch there is behind that step without an event.
int peer_history_home(nvrx_ctx *ctx, hipStream_t *home) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->attr_desc) return fail(NVRX_ERR_STATE, "no report was issued on this context: there is no peer step to follow");
    *home = ctx->default_stream;
    HIP_TRY(hipSetDevice(ctx->device));
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_peer_history(const float *d_peer, int n_ranks, int S, float *d_hist, int S_cap, int H, uint64_t n_before,
                      const double *thresholds, void *d_out, void *stream) {
    const int rc = peer_history_check(d_peer, n_ranks, S, d_hist, S_cap, H, thresholds, d_out);
    if (rc) return rc;
    return history_launch<true>(d_peer, S, 0, n_ranks, d_hist, S_cap, H, n_before, thresholds, d_out, as_stream(stream));
}

int nvrx_report_peer_history(nvrx_ctx *ctx, const float *d_peer, int n_ranks, int S, float *d_hist, int S_cap, int H,
                             uint64_t n_before, const double *thresholds, void *d_out) {
    if (!ctx) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = peer_history_check(d_peer, n_ranks, S, d_hist, S_cap, H, thresholds, d_out);
    if (rc) return rc;
    hipStream_t home = nullptr;
    if (const int rc = peer_history_home(ctx, &home)) return rc;
    return history_launch<true>(d_peer, S, 0, n_ranks, d_hist, S_cap, H, n_before, thresholds, d_out, home);
}

int nvrx_peer_trend(const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports, void *d_out, void *stream) {
    const int rc = trend_check(d_hist, n_ranks, S, S_cap, H, n_reports, d_out, 1);
    if (rc) return rc;
    return trend_launch<true>(d_hist, n_ranks, S, S_cap, H, n_reports, d_out, as_stream(stream));
}

int nvrx_report_peer_trend(nvrx_ctx *ctx, const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports,
                           void *d_out) {
    if (!ctx) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = trend_check(d_hist, n_ranks, S, S_cap, H, n_reports, d_out, 1);
    if (rc) return rc;
    hipStream_t home = nullptr;
    if (const int rc = peer_history_home(ctx, &home)) return rc;
    // no event: the ring's only writers are peer-history steps, and nvrx_report_peer_history launched the last of them here
    return trend_launch<true>(d_hist, n_ranks, S, S_cap, H, n_reports, d_out, home);
}

}  // extern "C"
