// nvrx_slack.inl -- slack scores: the rank the others wait for in collectives.  Part of the translation unit
// nvrx_straggler.hip (included at its end, behind nvrx_robust.inl: it uses that file's selections, nvrx_rowfam.inl's
// local_window and the key maps, sums and minima of nvrx_straggler.hip).
//
// Every other score compares how long a rank's own work takes.  A rank whose HOST is slow launches late, computes at the usual
// speed and ends its sections in a collective like everybody else: all of those scores read 1.  What shows it is the time the
// ranks spend inside collective kernels -- the rows every report drops before scoring because "their duration is peer-wait
// time".  The rank that arrives last spends only the transfer time there, every other rank that plus the wait for it.  The
// contract is in include/nvrx_straggler.h (nvrx_slack_local, nvrx_slack_score).
//
// k_slack_local  one wave per logical rank, lane c = column c.  The (row, column) list is taken 64 entries at a time: lane i
//   loads entry i and that row's NUM and WEIGHT (one round of independent loads), then the wave walks the chunk in list
//   order through readlane broadcasts and the lane of the entry's column adds: one fixed sequence of f64 additions per
//   (rank, column).
// k_slack_cols   one workgroup per column, strided over the ranks: the minimum of the per-call means (as keys) and the number
//   of present ranks by the wave reductions and one LDS word per wave.
// k_slack_rank   one wave per rank, lane c = column c: three wave sums in f64 and a strided one over the K kernel weights;
//   lane 0 writes the 32-byte record as two 16-byte stores.  A template on GROUPED: <true> is the per-group form's rank kernel
//   (nvrx_slack_group.inl), <false> what the kernel was.
// k_slack_job<T> one workgroup: the lower medians of waited_us and share over the rank records.  T == 0 (R <= 64): rank r in
//   lane r, robust_wave_select; else robust_radix_select over the record words at a stride of 8.  Absent ranks hold NaN in
//   both words and never enter.
// No float atomics, no global atomics, no scratch; workgroups of one launch share nothing.

namespace {

constexpr int SLACK_COLS = NVRX_SLACK_COLS;
static_assert(SLACK_COLS == 64, "lane c = column c");
constexpr uint32_t SLACK_NAN = 0x7FC00000u;
constexpr int SLACK_HEAD_WORDS = 8 + 4 * SLACK_COLS;  // job record, column records
constexpr int SLACK_COLS_THREADS = 256;

struct SlackLocalArgs {
    const float *stats;   // [local_ranks * rows_per_rank][NVRX_STATS_STRIDE]
    const int2 *list;     // [n] {row within a rank, column}
    int n;
    int rows_active, rows_per_rank;
    float *send;  // [local_ranks][2][64]
};

__global__ __launch_bounds__(64) void k_slack_local(SlackLocalArgs a) {
    const int lane = threadIdx.x;
    const float *__restrict__ stats = a.stats + (size_t)blockIdx.x * (size_t)a.rows_per_rank * NVRX_STATS_STRIDE;
    double t = 0.0, n = 0.0;
    bool any = false;
    for (int base = 0; base < a.n; base += 64) {  // wave-uniform
        const int i = base + lane;
        int col = -1;
        float num = 0.0f, weight = 0.0f;
        if (i < a.n) {
            const int2 e = a.list[i];
            if (e.x < a.rows_active) {  // (the host checked 0 <= e.x < rows_per_rank and 0 <= e.y < 64)
                col = e.y;
                num = stats[(size_t)e.x * NVRX_STATS_STRIDE + NVRX_STAT_NUM];
                weight = stats[(size_t)e.x * NVRX_STATS_STRIDE + NVRX_STAT_WEIGHT];
            }
        }
        const int m = min(64, a.n - base);
        for (int j = 0; j < m; j++) {
            const int cj = __builtin_amdgcn_readlane(col, j);
            const float nj = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(num), j));
            const float wj = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(weight), j));
            if (cj == lane && nj >= 1.0f) {
                t += (double)wj;
                n += (double)nj;
                any = true;
            }
        }
    }
    float *__restrict__ out = a.send + (size_t)blockIdx.x * 2 * SLACK_COLS;
    out[lane] = any ? (float)t : -1.0f;
    out[SLACK_COLS + lane] = any ? (float)n : 0.0f;
}

// rank r's entry of column c: whether it is present and its per-call mean
__device__ __forceinline__ bool slack_entry(const float *__restrict__ slack, int r, int c, float *t, float *n, float *avg) {
    *t = slack[(size_t)r * 2 * SLACK_COLS + c];
    *n = slack[(size_t)r * 2 * SLACK_COLS + SLACK_COLS + c];
    const bool present = *n > 0.0f && *t >= 0.0f;
    *avg = (float)((double)*t / (double)*n);
    return present;
}

struct SlackScoreArgs {
    const float *slack;  // [R][2][64]
    const float *table;  // [R][L]
    int R, K, S;
    int min_ranks;  // clamped to R
    uint32_t *out;  // job record | 64 column records | R rank records
};

__global__ __launch_bounds__(SLACK_COLS_THREADS) void k_slack_cols(SlackScoreArgs a) {
    constexpr int WAVES = SLACK_COLS_THREADS / 64;
    __shared__ uint32_t s_min[WAVES], s_cnt[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = (int)blockIdx.x;
    uint32_t mn = 0xFFFFFFFFu, cnt = 0;
    for (int r = tid; r < a.R; r += SLACK_COLS_THREADS) {
        float t, n, avg;
        const bool present = slack_entry(a.slack, r, c, &t, &n, &avg);
        mn = min(mn, present ? f2key(avg) : 0xFFFFFFFFu);
        cnt += present ? 1u : 0u;
    }
    mn = wave_min_u32(mn);
    cnt = wave_sum_u32(cnt);
    if (lane == 0) s_min[wave] = mn, s_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        mn = s_min[0], cnt = s_cnt[0];
#pragma unroll
        for (int w = 1; w < WAVES; w++) mn = min(mn, s_min[w]), cnt += s_cnt[w];
        const bool referenced = cnt != 0u && (int)cnt >= a.min_ranks;
        reinterpret_cast<uint4 *>(a.out + 8)[c] = make_uint4(referenced ? __float_as_uint(key2f(mn)) : SLACK_NAN, cnt, 0u, 0u);
    }
}

// the per-group form's arguments and layout (nvrx_slack_group.inl): G group records | G x 64 pair records | R rank records
struct SlackGroupArgs {
    const float *slack;     // [R][2][64]
    const float *table;     // [R][L]
    const int32_t *groups;  // group[R] | members[R] | start[G+1]
    int R, K, S, G;
    int max_group;  // in 1..R
    int min_ranks, min_peers;
    uint32_t *out;
};
constexpr int SLACK_GROUP_WORDS = 8;  // a group record
__host__ __device__ constexpr size_t slack_group_rank_base(int G) { return (size_t)(SLACK_GROUP_WORDS + 4 * SLACK_COLS) * (size_t)G; }

// GROUPED (a compile-time flag: the job-wide instantiation is what it was): the column records are the pair records of
// group[r], a pair being referenced iff it names a floor rank; words 6 and 7 of the record say how many columns the rank is
// present in at all and its group id (-1 outside [0, G): such a rank has no column).
template <bool GROUPED = false, class Args = SlackScoreArgs>
__global__ __launch_bounds__(256) void k_slack_rank(Args a) {
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (r >= a.R) return;  // wave-uniform
    float t, n, avg;
    const bool present = slack_entry(a.slack, r, lane, &t, &n, &avg);
    uint4 col;
    bool in;
    int g = -1;
    if constexpr (GROUPED) {
        g = a.groups[r];
        g = (uint32_t)g < (uint32_t)a.G ? g : -1;  // wave-uniform
        col = reinterpret_cast<const uint4 *>(a.out + SLACK_GROUP_WORDS * (size_t)a.G)[(size_t)(g < 0 ? 0 : g) * SLACK_COLS + lane];
        in = present && g >= 0 && (int)col.z >= 0;
    } else {
        col = reinterpret_cast<const uint4 *>(a.out + 8)[lane];
        in = present && col.y != 0u && (int)col.y >= a.min_ranks;
    }
    const double coll = wave_sum_f64(in ? (double)t : 0.0);
    const double waited = wave_sum_f64(in ? (double)n * ((double)avg - (double)__uint_as_float(col.x)) : 0.0);
    const double calls = wave_sum_f64(in ? (double)n : 0.0);
    const uint32_t columns = (uint32_t)__popcll(__ballot(in));
    const uint32_t word6 = GROUPED ? (uint32_t)__popcll(__ballot(present)) : 0u, word7 = GROUPED ? (uint32_t)g : 0u;
    const int K = a.K, KS = K + a.S;
    double comp = 0.0;
    if (K > 0) {  // (no table is needed without kernel ids)
        const float *__restrict__ row = a.table + (size_t)r * NVRX_TABLE_LEN(K, a.S);
        for (int k = lane; k < K; k += 64) comp += row[k] >= 0.0f ? (double)row[2 * KS + k] : 0.0;
    }
    comp = wave_sum_f64(comp);
    if (lane == 0) {
        size_t base = SLACK_HEAD_WORDS;
        if constexpr (GROUPED) base = slack_group_rank_base(a.G);
        uint4 *rec = reinterpret_cast<uint4 *>(a.out + base) + 2 * (size_t)r;
        if (columns) {
            const float share = (float)(waited / (coll + comp));
            const uint32_t ncalls = calls >= 4294967295.0 ? 0xFFFFFFFFu : calls >= 0.0 ? (uint32_t)calls : 0u;  // (a NaN reads 0)
            rec[0] = make_uint4(__float_as_uint((float)coll), __float_as_uint((float)waited), __float_as_uint((float)comp),
                                __float_as_uint(share));
            rec[1] = make_uint4(ncalls, columns, word6, word7);
        } else {
            rec[0] = make_uint4(SLACK_NAN, SLACK_NAN, SLACK_NAN, SLACK_NAN);
            rec[1] = make_uint4(0u, 0u, word6, word7);
        }
    }
}

// THREADS == 0: one wave, rank r in lane r (R <= 64); else one workgroup of THREADS
template <int THREADS>
__global__ __launch_bounds__(THREADS ? THREADS : 64) void k_slack_job(SlackScoreArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int R = a.R;
    const float *__restrict__ recs = reinterpret_cast<const float *>(a.out + SLACK_HEAD_WORDS);  // [R][8]
    uint32_t typical[2] = {SLACK_NAN, SLACK_NAN};
    uint32_t with_data = 0;
    if constexpr (THREADS == 0) {
        const bool mine = lane < R;
        with_data = (uint32_t)__popcll(__ballot(mine && a.out[SLACK_HEAD_WORDS + 8 * lane + 5] != 0u));
#pragma unroll
        for (int w = 0; w < 2; w++) {
            const float v = mine ? recs[8 * lane + 1 + 2 * w] : -1.0f;
            const bool present = v >= 0.0f;
            const unsigned long long mask = __ballot(present);
            if (mask) {  // wave-uniform
                const uint32_t target = ((uint32_t)__popcll(mask) - 1u) >> 1;
                const int at = robust_wave_select(f2key(v), present, mask, target, R, lane);
                typical[w] = (uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), at);
            }
        }
    } else {
        constexpr int WAVES = THREADS / 64;
        __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
        __shared__ uint32_t s_wave[WAVES];
        __shared__ uint32_t s_sel[2];
        __shared__ uint32_t s_cnt[3][WAVES];
        const int wave = tid >> 6;
        uint32_t c0 = 0, c1 = 0, cd = 0;
        for (int r = tid; r < R; r += THREADS) {
            c0 += recs[8 * (size_t)r + 1] >= 0.0f ? 1u : 0u;
            c1 += recs[8 * (size_t)r + 3] >= 0.0f ? 1u : 0u;
            cd += a.out[SLACK_HEAD_WORDS + 8 * (size_t)r + 5] != 0u ? 1u : 0u;
        }
        c0 = wave_sum_u32(c0), c1 = wave_sum_u32(c1), cd = wave_sum_u32(cd);
        if (lane == 0) s_cnt[0][wave] = c0, s_cnt[1][wave] = c1, s_cnt[2][wave] = cd;
        __syncthreads();
        uint32_t cnt[2] = {0, 0};
#pragma unroll
        for (int w = 0; w < WAVES; w++) cnt[0] += s_cnt[0][w], cnt[1] += s_cnt[1][w], with_data += s_cnt[2][w];
#pragma unroll 1
        for (int w = 0; w < 2; w++) {
            const uint32_t m = uni(cnt[w]);
            if (m == 0) continue;  // block-uniform
            const float *__restrict__ col = recs + 1 + 2 * w;
            const float v0 = tid < R ? col[8 * (size_t)tid] : -1.0f;
            typical[w] = __float_as_uint(key2f(robust_radix_select<THREADS, false>(col, R, 8, v0, 0.0f, (m - 1u) >> 1, s_hist, s_wave, s_sel)));
            __syncthreads();  // (the next selection clears the histogram and rewrites s_wave / s_sel)
        }
    }
    if (tid < 64) {  // the first wave: lane c = column c
        const uint32_t n = a.out[8 + 4 * lane + 1];
        const uint32_t referenced = (uint32_t)__popcll(__ballot(n != 0u && (int)n >= a.min_ranks));
        if (tid != 0) return;
        reinterpret_cast<uint4 *>(a.out)[0] = make_uint4(typical[0], typical[1], with_data, referenced);
        reinterpret_cast<uint4 *>(a.out)[1] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// argument checks of nvrx_slack_score; nothing here touches a device
int slack_score_check(const float *d_slack, const float *d_table, int R, int K, int S, int min_ranks, const void *d_out) {
    if (R <= 0 || K < 0 || S < 0) return fail(NVRX_ERR_INVALID, "bad table shape R=%d K=%d S=%d", R, K, S);
    if (R > NVRX_ROBUST_MAX_RANKS) return fail(NVRX_ERR_RANGE, "R=%d ranks, at most %d", R, NVRX_ROBUST_MAX_RANKS);
    if (K > NVRX_MAX_ROWS || S > NVRX_MAX_ROWS) return fail(NVRX_ERR_RANGE, "K=%d S=%d ids, at most %d each", K, S, NVRX_MAX_ROWS);
    if (min_ranks < 1) return fail(NVRX_ERR_RANGE, "min_ranks=%d, at least 1", min_ranks);
    if (!d_slack || !d_out || (K > 0 && !d_table)) return fail(NVRX_ERR_INVALID, "null device pointer");
    if ((reinterpret_cast<uintptr_t>(d_slack) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d_out) & 15u) != 0)
        return fail(NVRX_ERR_INVALID, "d_slack or d_out is not 16-byte aligned");
    return NVRX_OK;
}

int slack_score_launch(const float *d_slack, const float *d_table, int R, int K, int S, int min_ranks, void *d_out, hipStream_t st) {
    SlackScoreArgs a{};
    a.slack = d_slack, a.table = d_table;
    a.R = R, a.K = K, a.S = S;
    a.min_ranks = std::min(min_ranks, R);
    a.out = static_cast<uint32_t *>(d_out);
    hipLaunchKernelGGL(k_slack_cols, dim3(SLACK_COLS), dim3(SLACK_COLS_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_slack_rank<false, SlackScoreArgs>), dim3((R + 3) / 4), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (R <= 64)
        hipLaunchKernelGGL(k_slack_job<0>, dim3(1), dim3(64), 0, st, a);
    else if (R <= 1024)
        hipLaunchKernelGGL(k_slack_job<256>, dim3(1), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_slack_job<1024>, dim3(1), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_slack_score(const float *d_slack, const float *d_table, int R, int K, int S, int min_ranks, void *d_out, void *stream) {
    const int rc = slack_score_check(d_slack, d_table, R, K, S, min_ranks, d_out);
    if (rc) return rc;
    return slack_score_launch(d_slack, d_table, R, K, S, min_ranks, d_out, as_stream(stream));
}

int nvrx_slack_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, const float *d_stats, const int32_t *rows, const int32_t *cols,
                     int n, float *d_send, int rows_active, void *stream) {
    // (the checks that need nothing of the context come first: they are reported for any context pointer)
    if (!ctx || !d_send) return fail(NVRX_ERR_INVALID, "null argument");
    if (n < 0) return fail(NVRX_ERR_INVALID, "n=%d collective rows outside [0,rows_per_rank]", n);
    if (n > 0 && (!rows || !cols)) return fail(NVRX_ERR_INVALID, "null row or column list");
    for (int i = 0; i < n; i++) {
        if (rows[i] < 0) return fail(NVRX_ERR_RANGE, "rows[%d]=%d is negative", i, rows[i]);
        if (cols[i] < 0 || cols[i] >= SLACK_COLS) return fail(NVRX_ERR_RANGE, "cols[%d]=%d outside [0,%d)", i, cols[i], SLACK_COLS);
        if (i && rows[i] <= rows[i - 1]) return fail(NVRX_ERR_INVALID, "rows[%d]=%d: the list is not in ascending row order", i, rows[i]);
    }
    if (!desc && !d_stats) return fail(NVRX_ERR_INVALID, "null statistics rows");
    if ((reinterpret_cast<uintptr_t>(d_send) & 15u) != 0) return fail(NVRX_ERR_INVALID, "d_send is not 16-byte aligned");
    if (n > ctx->rows_per_rank) return fail(NVRX_ERR_INVALID, "n=%d collective rows outside [0,%d]", n, ctx->rows_per_rank);
    if (n > 0 && rows[n - 1] >= ctx->rows_per_rank)  // (ascending: the last row is the largest)
        return fail(NVRX_ERR_RANGE, "rows[%d]=%d outside [0,%d)", n - 1, rows[n - 1], ctx->rows_per_rank);
    if (desc) d_stats = desc->d_stats;
    if (!d_stats) return fail(NVRX_ERR_INVALID, "null statistics rows");
    hipStream_t st = as_stream(stream);
    LocalWindow w;
    int rc = local_window(ctx, desc, d_send, 0, 0, rows_active, [] { return NVRX_OK; }, nullptr, &st, &w);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (desc && ctx->stats_stream != st && ctx->stats_stream != ctx->attr_stream) {
        // a resident score kernel left the statistics kernel on a stream that is neither this one nor the one local_window
        // just ordered this one behind
        if (!ctx->attr_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->attr_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ctx->attr_ev, ctx->stats_stream));
        HIP_TRY(hipStreamWaitEvent(st, ctx->attr_ev, 0));
    }
    if (n > 0) {
        bool same = ctx->slack_list_up && ctx->slack_list.size() == 2 * (size_t)n;
        for (int i = 0; same && i < n; i++) same = ctx->slack_list[2 * i] == rows[i] && ctx->slack_list[2 * i + 1] == cols[i];
        if (!same) {  // cold: the set of collective rows changed
            if (!ctx->d_slack_list) HIP_TRY(hipMalloc(&ctx->d_slack_list, (size_t)ctx->rows_per_rank * 2 * sizeof(int32_t)));
            ctx->slack_list_up = false;
            ctx->slack_list.resize(2 * (size_t)n);
            for (int i = 0; i < n; i++) ctx->slack_list[2 * i] = rows[i], ctx->slack_list[2 * i + 1] = cols[i];
            HIP_TRY(hipMemcpyAsync(ctx->d_slack_list, ctx->slack_list.data(), 2 * (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));  // (pageable source: it must not change under the copy)
            ctx->slack_list_up = true;
        }
    }
    SlackLocalArgs a{};
    a.stats = d_stats, a.list = reinterpret_cast<const int2 *>(ctx->d_slack_list), a.n = n;
    a.rows_active = w.rows_active, a.rows_per_rank = w.rows_per_rank;
    a.send = d_send;
    hipLaunchKernelGGL(k_slack_local, dim3(ctx->local_ranks), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // extern "C"
