// nvrx_peer.inl -- peer-group scores: every rank against the fastest rank of ITS OWN group.  Part of the translation unit
// nvrx_straggler.hip (included at its end: it uses that file's key maps and wave sums).
//
// Every relative score of the reference (reporting.py:196-253) divides the median of the fastest rank of the WHOLE JOB by
// this rank's: a lockstep data-parallel model.  In a job of pipeline stages, expert groups or actor / critic roles a section
// legitimately takes a different time on different ranks, and the healthy ranks of a slow stage read as stragglers.  Here the
// caller says which ranks do the same work (d_groups: group id per rank, the ranks sorted by group, the groups' stretches),
// and the reference point of a column is the smallest present value among the rank's peers.  The table is the one nvrx_score
// reads; nothing else is exchanged.
//
// k_peer_cols  grid (ceil((K+S)/64), G), 256 threads.  Lane = column, so a wave's loads of one member's row are one coalesced
//   256-byte run; the four waves take the group's members start[g] + wave, + 4, ... four at a time (four rows' loads in
//   flight), each lane keeping the best (f2key, rank) pair and a count in registers.  One LDS hand-over, one barrier, wave 0
//   merges (smaller key first, then the lower rank) and writes 64 consecutive 16-byte records.  No DPP, no atomics, no scratch.
//   One kernel for every R: at the sizes where a wave-per-column variant could win, the step is launch-latency-bound.
// k_peer_rank  one workgroup per reported rank, shaped like k_robust_rank.
//
// d_groups is data, not an argument the host checks can see: a group id outside [0, G) rates the rank NaN, a member outside
// [0, R) is skipped, start values are clamped to [0, R].  Nothing in it can move a load or a store outside the table, the
// array or d_out.

namespace {

constexpr int PGROUP_TILE = 64;  // columns per workgroup
constexpr int PGROUP_THREADS = 256;
constexpr int PGROUP_UNROLL = 4;  // members per wave in flight

struct PeerColsArgs {
    const float *table;     // [R][L]
    const int32_t *groups;  // group[R] | members[R] | start[G+1]
    int R, G, KS, L;
    int min_ranks;
    uint4 *cols;  // [G][KS] {f32 floor, u32 present, i32 floor_rank, u32 members}
};

__device__ __forceinline__ int peer_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

__global__ __launch_bounds__(PGROUP_THREADS) void k_peer_cols(PeerColsArgs a) {
    constexpr int NW = PGROUP_THREADS / 64;
    __shared__ uint32_t s_key[NW][PGROUP_TILE];
    __shared__ uint32_t s_rank[NW][PGROUP_TILE];
    __shared__ uint32_t s_cnt[NW][PGROUP_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R, KS = a.KS;
    const int g = (int)blockIdx.y;  // < G: the grid's extent
    const int c = (int)blockIdx.x * PGROUP_TILE + lane;
    const int32_t *__restrict__ members = a.groups + R;
    const int32_t *__restrict__ start = a.groups + 2 * (size_t)R;
    const int s0 = peer_clamp(start[g], R), s1 = peer_clamp(start[g + 1], R);

    uint32_t best = 0xFFFFFFFFu;   // above f2key(+inf): no present value has it
    uint32_t brank = 0xFFFFFFFFu;  // (int) -1
    uint32_t cnt = 0;
    for (int i = s0 + wave; i < s1; i += NW * PGROUP_UNROLL) {
        int m[PGROUP_UNROLL];
        float v[PGROUP_UNROLL];
#pragma unroll
        for (int j = 0; j < PGROUP_UNROLL; j++) {
            const int idx = i + NW * j;
            m[j] = idx < s1 ? members[idx] : -1;
            const bool in = (uint32_t)m[j] < (uint32_t)R && c < KS;
            v[j] = in ? a.table[(size_t)m[j] * (size_t)a.L + (size_t)c] : -1.0f;
        }
#pragma unroll
        for (int j = 0; j < PGROUP_UNROLL; j++) {
            const bool present = v[j] >= 0.0f;
            const uint32_t key = f2key(v[j]);
            const bool take = present && (key < best || (key == best && (uint32_t)m[j] < brank));
            best = take ? key : best;
            brank = take ? (uint32_t)m[j] : brank;
            cnt += present ? 1u : 0u;
        }
    }
    s_key[wave][lane] = best;
    s_rank[wave][lane] = brank;
    s_cnt[wave][lane] = cnt;
    __syncthreads();
    if (wave != 0 || c >= KS) return;
#pragma unroll
    for (int w = 1; w < NW; w++) {
        const uint32_t key = s_key[w][lane], rk = s_rank[w][lane];
        const bool take = key < best || (key == best && rk < brank);
        best = take ? key : best;
        brank = take ? rk : brank;
        cnt += s_cnt[w][lane];
    }
    const bool referenced = (int)cnt >= a.min_ranks;  // min_ranks >= 1: a pair with no present member never is
    const uint32_t floor_bits = referenced ? __float_as_uint(key2f(best)) : __float_as_uint(__builtin_nanf(""));
    const uint32_t n_members = s1 > s0 ? (uint32_t)(s1 - s0) : 0u;
    a.cols[(size_t)g * (size_t)KS + (size_t)c] = make_uint4(floor_bits, cnt, referenced ? brank : 0xFFFFFFFFu, n_members);
}

struct PeerRankArgs {
    const float *table;     // [R][L]
    const int32_t *groups;  // group[R] | ...
    const uint4 *cols;      // [G][KS]
    int K, S, G;
    int first_rank;
    int min_ranks;
    float *out;  // [n_ranks][1 + S]
};

// one workgroup per reported rank: {gpu, section[S]} against the rank's own group
__global__ __launch_bounds__(PGROUP_THREADS) void k_peer_rank(PeerRankArgs a) {
    constexpr int NW = PGROUP_THREADS / 64;
    __shared__ double s_sum[2][NW];
    __shared__ uint32_t s_cnt[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, S = a.S, KS = K + S;
    const int L = NVRX_TABLE_LEN(K, S);
    const int r = a.first_rank + (int)blockIdx.x;
    const float *__restrict__ row = a.table + (size_t)r * L;
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
        const double w = (double)row[2 * KS + k];
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

// argument checks shared by both entry points, in robust_check's sequence; nothing here touches a device
int peer_check(int R, int K, int S, int G, int first_rank, int n_ranks, int min_ranks) {
    const int rc = table_min_ranks_check(R, K, S, first_rank, n_ranks, min_ranks);
    return rc ? rc : groups_check(R, G);
}

int peer_launch(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int first_rank, int n_ranks,
                int min_ranks, void *d_out, hipStream_t st) {
    const int KS = K + S;
    if (KS > 0) {
        PeerColsArgs c{};
        c.table = d_table, c.groups = d_groups, c.R = R, c.G = G, c.KS = KS, c.L = NVRX_TABLE_LEN(K, S);
        c.min_ranks = min_ranks;
        c.cols = static_cast<uint4 *>(d_out);
        hipLaunchKernelGGL(k_peer_cols, dim3((KS + PGROUP_TILE - 1) / PGROUP_TILE, G), dim3(PGROUP_THREADS), 0, st, c);
        HIP_TRY(hipGetLastError());
    }
    PeerRankArgs a{};
    a.table = d_table, a.groups = d_groups, a.cols = static_cast<const uint4 *>(d_out);
    a.K = K, a.S = S, a.G = G, a.first_rank = first_rank, a.min_ranks = min_ranks;
    a.out = static_cast<float *>(d_out) + 4 * (size_t)G * (size_t)KS;
    hipLaunchKernelGGL(k_peer_rank, dim3(n_ranks), dim3(PGROUP_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_peer_score(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int first_rank, int n_ranks,
                    int min_ranks, void *d_out, void *stream) {
    const int rc = peer_check(R, K, S, G, first_rank, n_ranks, min_ranks);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_table && d_groups, false)) return rc;
    return peer_launch(d_table, R, K, S, d_groups, G, first_rank, n_ranks, min_ranks, d_out, as_stream(stream));
}

int nvrx_report_peer(nvrx_ctx *ctx, const nvrx_report_desc *desc, const int32_t *d_groups, int G, int first_rank, int n_ranks,
                     int min_ranks, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = peer_check(desc->R, desc->K, desc->S, G, first_rank, n_ranks, min_ranks);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_groups != nullptr, true)) return rc;
    hipStream_t home = nullptr;
    const float *table = nullptr;
    if (const int rc = report_table(ctx, desc, &home, &table)) return rc;
    return peer_launch(table, desc->R, desc->K, desc->S, d_groups, G, first_rank, n_ranks, min_ranks, d_out, home);
}

}  // extern "C"
