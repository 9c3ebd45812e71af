// nvrx_rowfam_group.inl -- the row families' score step per peer group: tail, onset, period and episode scores with a
// column's reference taken inside each rank's OWN group.  Part of the translation unit nvrx_straggler.hip (included behind
// nvrx_peer.inl: it uses that file's column kernel and argument checks, and nvrx_tablefam.inl's pointer check).
//
// nvrx_rowfam.inl's score step (tail_score_launch) takes one reference per column over all R ranks of plane 0: a lockstep
// job.  In a job of pipeline stages the healthy ranks of the slower stage read as tail stragglers, and a beat, a step or a
// stretch that one whole stage shares flags that stage.  Here the caller says which ranks are peers (nvrx_peer_score's array,
// unchanged) and the reference of a column is the smallest present value of plane 0 among the rank's peers.  The gathered
// planes and the table are the ones the job-wide step reads; nothing else is exchanged.
//
// k_peer_cols           nvrx_peer.inl's kernel, unchanged, on the planes: its L is only a pitch, here planes * (K+S).
// k_rowfam_group_rank   one workgroup of 256 per reported rank, shaped like k_tail_score / k_peer_rank: values from the plane
//   row, weights from the table row, records from group[r]'s stretch of block A.  wave_sum_f64 / wave_sum_u32 and one LDS
//   word per wave; no atomics, no scratch, no trip count that depends on the data.
//
// d_groups is data, not an argument the host checks can see: k_peer_cols guards members and starts, and a group id outside
// [0, G) rates the rank NaN here.  Nothing in it can move a load or a store outside the inputs or d_out.

namespace {

// the largest *_PLANES of the header: what `planes` may be
constexpr int ROWFAM_MAX_PLANES = std::max({1, NVRX_ONSET_PLANES, NVRX_PERIOD_PLANES, NVRX_EPISODE_PLANES});

struct RowfamGroupRankArgs {
    const float *planes;    // [R][ld]: plane 0 in the first K+S floats of a row
    int ld;                 // planes * (K+S)
    const float *table;     // [R][L]: the weights (null only at K = 0)
    const int32_t *groups;  // group[R] | ...
    const uint4 *cols;      // [G][KS]
    int K, S, G;
    int first_rank;
    int min_ranks;
    float *out;  // [n_ranks][1 + S]
};

// one workgroup per reported rank: {gpu, section[S]} against the rank's own group
__global__ __launch_bounds__(PGROUP_THREADS) void k_rowfam_group_rank(RowfamGroupRankArgs a) {
    constexpr int NW = PGROUP_THREADS / 64;
    __shared__ double s_sum[2][NW];
    __shared__ uint32_t s_cnt[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, S = a.S, KS = K + S;
    const int L = NVRX_TABLE_LEN(K, S);
    const int r = a.first_rank + (int)blockIdx.x;
    const float *__restrict__ row = a.planes + (size_t)r * (size_t)a.ld;
    const float *__restrict__ wrow = K ? a.table + (size_t)r * L + 2 * KS : nullptr;  // (no table at K = 0)
    float *__restrict__ out = a.out + (size_t)blockIdx.x * (size_t)(1 + S);
    const float NaN = __builtin_nanf("");
    const int g = a.groups[r];
    const bool in_group = (uint32_t)g < (uint32_t)a.G;  // block-uniform
    const uint4 *__restrict__ recs = a.cols + (size_t)(in_group ? g : 0) * (size_t)KS;

    for (int s = tid; s < S; s += PGROUP_THREADS) {
        const float v = row[K + s];
        const uint4 rec = recs[K + s];
        const bool ok = in_group && v >= 0.0f && (int)rec.y >= a.min_ranks;
        out[1 + s] = ok ? (float)((double)__uint_as_float(rec.x) / (double)v) : NaN;
    }
    double ws = 0.0, sr = 0.0;
    uint32_t cnt = 0;
    for (int k = tid; k < K; k += PGROUP_THREADS) {
        const float v = row[k];
        if (!in_group || !(v >= 0.0f)) continue;
        const uint4 rec = recs[k];
        if ((int)rec.y < a.min_ranks) continue;
        const double w = (double)wrow[k];
        sr += w * ((double)__uint_as_float(rec.x) / (double)v);
        ws += w;
        cnt++;
    }
    ws = wave_sum_f64(ws);
    sr = wave_sum_f64(sr);
    cnt = wave_sum_u32(cnt);
    if (lane == 0) {
        s_sum[0][wave] = ws;
        s_sum[1][wave] = sr;
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        ws = sr = 0.0;
        cnt = 0;
        for (int w = 0; w < NW; w++) {
            ws += s_sum[0][w];
            sr += s_sum[1][w];
            cnt += s_cnt[w];
        }
        out[0] = cnt ? (float)(sr / ws) : NaN;
    }
}

// argument checks: plane_score's of the shape and the rank range in its order, `planes`, then peer_check's threshold and
// groups; nothing here touches a device
int rowfam_group_check(int planes, int R, int K, int S, int G, int first_rank, int n_ranks, int min_ranks) {
    if (R <= 0 || K < 0 || S < 0) return fail(NVRX_ERR_INVALID, "bad table shape R=%d K=%d S=%d", R, K, S);
    if (R > NVRX_ROBUST_MAX_RANKS) return fail(NVRX_ERR_RANGE, "R=%d ranks, at most %d", R, NVRX_ROBUST_MAX_RANKS);
    if (K > NVRX_MAX_ROWS || S > NVRX_MAX_ROWS) return fail(NVRX_ERR_RANGE, "K=%d S=%d ids, at most %d each", K, S, NVRX_MAX_ROWS);
    if (first_rank < 0 || n_ranks < 1 || first_rank > R - n_ranks)
        return fail(NVRX_ERR_RANGE, "ranks [%d,%d+%d) outside the table's %d", first_rank, first_rank, n_ranks, R);
    if (planes < 1 || planes > ROWFAM_MAX_PLANES) return fail(NVRX_ERR_RANGE, "planes=%d, within 1..%d", planes, ROWFAM_MAX_PLANES);
    if (min_ranks < 1) return fail(NVRX_ERR_RANGE, "min_ranks=%d, at least 1", min_ranks);
    return groups_check(R, G);
}

}  // namespace

extern "C" {

size_t nvrx_rowfam_group_words(int G, int K, int S, int n_ranks) {
    if (G < 0 || K < 0 || S < 0 || n_ranks < 0) return 0;
    return NVRX_ROWFAM_GROUP_WORDS(G, K, S, n_ranks);
}

int nvrx_rowfam_group_score(const float *d_planes, int planes, const float *d_table, int R, int K, int S,
                            const int32_t *d_groups, int G, int first_rank, int n_ranks, int min_ranks, void *d_out,
                            void *stream) {
    const int rc = rowfam_group_check(planes, R, K, S, G, first_rank, n_ranks, min_ranks);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_planes && d_groups && (d_table || K == 0), false)) return rc;
    hipStream_t st = as_stream(stream);
    const int KS = K + S;
    if (KS > 0) {
        PeerColsArgs c{};
        c.table = d_planes, c.groups = d_groups, c.R = R, c.G = G, c.KS = KS, c.L = planes * KS;
        c.min_ranks = min_ranks;
        c.cols = static_cast<uint4 *>(d_out);
        hipLaunchKernelGGL(k_peer_cols, dim3((KS + PGROUP_TILE - 1) / PGROUP_TILE, G), dim3(PGROUP_THREADS), 0, st, c);
        HIP_TRY(hipGetLastError());
    }
    RowfamGroupRankArgs a{};
    a.planes = d_planes, a.ld = planes * KS, a.table = d_table, a.groups = d_groups;
    a.cols = static_cast<const uint4 *>(d_out);
    a.K = K, a.S = S, a.G = G, a.first_rank = first_rank, a.min_ranks = min_ranks;
    a.out = static_cast<float *>(d_out) + 4 * (size_t)G * (size_t)KS;
    hipLaunchKernelGGL(k_rowfam_group_rank, dim3(n_ranks), dim3(PGROUP_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // extern "C"
