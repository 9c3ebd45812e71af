// nvrx_pace_group.inl -- pace scores per peer group: the rank that is a little slower in everything than the ranks doing the
// SAME work.  Part of the translation unit nvrx_straggler.hip (included at its end, behind nvrx_peer.inl and nvrx_pace.inl: it
// uses the former's clamp and the latter's record, marker, radix select and rank kernel).
//
// nvrx_pace.inl's reference point of a column is the lower median of the whole job.  In a job of pipeline stages or expert
// groups that is the wrong one: every healthy rank of the slower stage is slower than the job's median in all of its kernels.
// Here the caller says which ranks are peers (nvrx_peer_score's array, unchanged) and a column's record is taken per (group,
// column): the lower median of the group's members that have the row.  The table is the one nvrx_score reads; nothing else is
// exchanged.
//
// k_pace_group_cols  {ctr, n, above, below} per (group, column); one variant per launch, chosen by the largest group's size.
//   <0>  every group has at most 64 members (a stage's data-parallel replicas): grid (ceil((K+S)/64), G), 256 threads,
//        k_pace_cols<0>'s geometry with the rows taken through members[]: 64 columns x size_g member rows staged in LDS
//        (65-word pitch), each member's row a coalesced 256-byte run (lane = column); then one column per wave at a time,
//        member i's value in lane i, robust_wave_select and two ballots.  One barrier, no atomics.
//   <T>  larger groups: grid (K+S, G), one workgroup of T per pair; pace_radix_select<T, 0> over keys re-read from the L2
//        through members[] (PACE_MARK for an absent or skipped member), and one more strided pass for the counts.  Smaller
//        groups of the same launch take the same path.
// k_pace_rank<.., .., true>  nvrx_pace.inl's rank kernel reading the records of the rank's own group.
//
// d_groups is data, not an argument the host checks can see: start values are clamped to [0, R], a stretch to max_group, a
// member outside [0, R) is skipped, a group id outside [0, G) leaves the rank without a column.  Nothing in it can move a load
// or a store outside the table, the array or d_out.
//   Always exact, ties included; no trip count beyond the group's size, no sort, no scratch, no global atomics, no float atomics.

namespace {

struct PaceGroupColsArgs {
    const float *table;     // [R][L]
    const int32_t *groups;  // group[R] | members[R] | start[G+1]
    int R, KS, L;
    int max_group;  // in 1..R; at most 64 for <0>
    int min_ranks, min_peers;
    uint4 *cols;  // [G][KS] {f32 ctr, u32 n, u32 above, u32 below}
};

// the pair is referenced iff n >= max(min_peers, min(min_ranks, size)); min_peers >= 1, so a pair nobody has never is
__device__ __forceinline__ uint4 pace_group_record(uint32_t ckey, uint32_t n, uint32_t above, uint32_t below, int size,
                                                   const PaceGroupColsArgs &a) {
    const int clamped = a.min_ranks < size ? a.min_ranks : size;
    const int need = a.min_peers > clamped ? a.min_peers : clamped;
    const bool referenced = (int)n >= need;
    return make_uint4(referenced ? __float_as_uint(key2f(ckey)) : __float_as_uint(__builtin_nanf("")), n, above, below);
}

// THREADS == 0: the tiled kernel for groups of at most 64 (ROBUST_THREADS threads); else one workgroup of THREADS per pair
template <int THREADS>
__global__ __launch_bounds__(THREADS ? THREADS : ROBUST_THREADS) void k_pace_group_cols(PaceGroupColsArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R, KS = a.KS;
    const int g = (int)blockIdx.y;  // < G: the grid's extent
    const int32_t *__restrict__ members = a.groups + R;
    const int32_t *__restrict__ start = a.groups + 2 * (size_t)R;
    const int s0 = peer_clamp(start[g], R), s1 = peer_clamp(start[g + 1], R);
    int size = s1 > s0 ? s1 - s0 : 0;
    size = size < a.max_group ? size : a.max_group;
    members += s0;  // members[0 .. size) lie inside the array: s0 + size <= s1 <= R
    uint4 *__restrict__ cols = a.cols + (size_t)g * (size_t)KS;
    if constexpr (THREADS == 0) {
        __shared__ float s_tile[64 * ROBUST_PITCH];
        size = size < 64 ? size : 64;  // (what the host promised with max_group; the tile has 64 rows)
        const int base = (int)blockIdx.x * ROBUST_TILE;
        {
            const int c = base + lane;
            for (int i = wave; i < size; i += ROBUST_THREADS / 64) {
                const int m = members[i];
                const bool in = (uint32_t)m < (uint32_t)R && c < KS;
                s_tile[i * ROBUST_PITCH + lane] = in ? a.table[(size_t)m * (size_t)a.L + (size_t)c] : -1.0f;
            }
        }
        __syncthreads();
        for (int ci = wave; ci < ROBUST_TILE; ci += ROBUST_THREADS / 64) {
            const int c = base + ci;
            if (c >= KS) break;  // wave-uniform
            const float v = lane < size ? s_tile[lane * ROBUST_PITCH + ci] : -1.0f;
            const bool present = v >= 0.0f;
            const uint32_t key = f2key(v);
            const unsigned long long mask = __ballot(present);
            const uint32_t n = (uint32_t)__popcll(mask);
            uint32_t ckey = 0, above = 0, below = 0;
            if (n != 0) {  // wave-uniform
                const int lc = robust_wave_select(key, present, mask, (n - 1u) >> 1, size, lane);
                ckey = (uint32_t)__builtin_amdgcn_readlane((int)key, lc);
                above = (uint32_t)__popcll(__ballot(present && key > ckey));
                below = (uint32_t)__popcll(__ballot(present && key < ckey));
            }
            if (lane == 0) cols[c] = pace_group_record(ckey, n, above, below, size, a);
        }
    } else {
        constexpr int WAVES = THREADS / 64;
        __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
        __shared__ uint32_t s_wave[WAVES];
        __shared__ uint32_t s_sel[2];
        __shared__ uint32_t s_cnt[2][WAVES];
        const int c = (int)blockIdx.x;  // < KS: the grid's extent
        const float *__restrict__ col = a.table + c;
        const int L = a.L;
        // the key of member i < size; the marker where the member is absent or no rank of the table
        auto key_at = [&](int i) -> uint32_t {
            const int m = members[i];
            const float v = (uint32_t)m < (uint32_t)R ? col[(size_t)m * (size_t)L] : -1.0f;
            return v >= 0.0f ? f2key(v) : PACE_MARK;
        };
        uint32_t cnt = 0;
        for (int i = tid; i < size; i += THREADS) cnt += key_at(i) != PACE_MARK ? 1u : 0u;
        cnt = wave_sum_u32(cnt);
        if (lane == 0) s_wave[wave] = cnt;
        __syncthreads();
        uint32_t n = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) n += s_wave[w];
        n = uni(n);
        if (n == 0) {  // block-uniform
            if (tid == 0) cols[c] = pace_group_record(0u, 0u, 0u, 0u, size, a);
            return;
        }
        // (s_wave is rewritten only behind the first pass' two barriers)
        const uint32_t ckey = pace_radix_select<THREADS, 0>(key_at, size, (n - 1u) >> 1, s_hist, s_wave, s_sel);
        uint32_t above = 0, below = 0;
        for (int i = tid; i < size; i += THREADS) {
            const uint32_t key = key_at(i);
            above += (key != PACE_MARK && key > ckey) ? 1u : 0u;
            below += key < ckey ? 1u : 0u;  // (the marker is above every key)
        }
        above = wave_sum_u32(above);
        below = wave_sum_u32(below);
        if (lane == 0) s_cnt[0][wave] = above, s_cnt[1][wave] = below;
        __syncthreads();
        if (tid == 0) {
            above = below = 0;
            for (int w = 0; w < WAVES; w++) above += s_cnt[0][w], below += s_cnt[1][w];
            cols[c] = pace_group_record(ckey, n, above, below, size, a);
        }
    }
}

// argument checks shared by both entry points: nvrx_pace_score's, then nvrx_peer_score's of G, then the two of this family;
// nothing here touches a device
int pace_group_check(int R, int K, int S, int G, int max_group, int first_rank, int n_ranks, int min_ranks, int min_peers) {
    int rc = table_min_ranks_check(R, K, S, first_rank, n_ranks, min_ranks);
    if (!rc) rc = groups_check(R, G);
    if (rc) return rc;
    if (max_group < 1 || max_group > R) return fail(NVRX_ERR_RANGE, "max_group=%d, within 1..%d", max_group, R);
    if (min_peers < 1) return fail(NVRX_ERR_RANGE, "min_peers=%d, at least 1", min_peers);
    return NVRX_OK;
}

// k_pace_group_cols by the largest group's size: cols_launch's thresholds (the tiled kernel takes groups of at most 64)
void pace_group_cols_launch(const PaceGroupColsArgs &c, int G, hipStream_t st) {
    cols_launch(k_pace_group_cols<0>, k_pace_group_cols<256>, k_pace_group_cols<1024>, c.max_group, c.KS, G, c, st);
}

int pace_group_launch(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int max_group, int first_rank,
                      int n_ranks, int min_ranks, int min_peers, void *d_out, hipStream_t st) {
    const int KS = K + S;
    if (KS > 0) {
        PaceGroupColsArgs c{};
        c.table = d_table, c.groups = d_groups, c.R = R, c.KS = KS, c.L = NVRX_TABLE_LEN(K, S);
        c.max_group = max_group, c.min_ranks = min_ranks, c.min_peers = min_peers;
        c.cols = static_cast<uint4 *>(d_out);
        pace_group_cols_launch(c, G, st);
        HIP_TRY(hipGetLastError());
    }
    PaceGroupRankArgs a{};
    a.table = d_table, a.cols = static_cast<const uint4 *>(d_out), a.groups = d_groups;
    a.K = K, a.S = S, a.G = G, a.first_rank = first_rank;
    a.out = static_cast<uint4 *>(d_out) + (size_t)G * (size_t)KS;
    pace_rank_launch<true>(a, n_ranks, st);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_pace_group_score(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int max_group,
                          int first_rank, int n_ranks, int min_ranks, int min_peers, void *d_out, void *stream) {
    const int rc = pace_group_check(R, K, S, G, max_group, first_rank, n_ranks, min_ranks, min_peers);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_table && d_groups, false)) return rc;
    return pace_group_launch(d_table, R, K, S, d_groups, G, max_group, first_rank, n_ranks, min_ranks, min_peers, d_out,
                             as_stream(stream));
}

int nvrx_report_pace_group(nvrx_ctx *ctx, const nvrx_report_desc *desc, const int32_t *d_groups, int G, int max_group,
                           int first_rank, int n_ranks, int min_ranks, int min_peers, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = pace_group_check(desc->R, desc->K, desc->S, G, max_group, first_rank, n_ranks, min_ranks, min_peers);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_groups != nullptr, true)) return rc;
    hipStream_t home = nullptr;
    const float *table = nullptr;
    if (const int rc = report_table(ctx, desc, &home, &table)) return rc;
    return pace_group_launch(table, desc->R, desc->K, desc->S, d_groups, G, max_group, first_rank, n_ranks, min_ranks, min_peers,
                             d_out, home);
}

}  // extern "C"
