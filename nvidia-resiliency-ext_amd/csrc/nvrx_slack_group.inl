// nvrx_slack_group.inl -- slack scores per peer group: the rank that the ranks doing the SAME work wait for.  Part of the
// translation unit nvrx_straggler.hip (included behind nvrx_slack.inl and nvrx_pace_group.inl: it uses the former's entry,
// rank kernel and record layout, nvrx_peer.inl's clamp and nvrx_pace.inl's marker and radix select).
//
// nvrx_slack.inl takes a collective column's floor over ALL ranks and one typical wait for the whole job: a lockstep model.
// In a job of pipeline stages or expert groups the time inside collective kernels is dominated by waits that legitimately
// differ per stage (send / receive bubbles, stage-local all-reduces of different sizes): the stage that waits least sets a
// floor nobody else can reach, and the rank whose host is slow hides behind it.  Here the caller says which ranks are peers
// (nvrx_peer_score's array, unchanged) and the score step runs per group: the floor of a pair (group, column) is the smallest
// per-call mean among the group's members, the typical wait the lower median over the group's members.  The local step, the
// send rows and the all-gather are nvrx_slack.inl's; nothing else is exchanged.
//
// k_slack_group_cols    grid G, 256 threads, lane c = column c.  The four waves take the group's members four at a time, as
//   k_peer_cols does; a member's t row and n row are one coalesced 256-byte run each.  Each lane keeps (best key, rank, count)
//   in registers; one LDS hand-over, one barrier, wave 0 merges (smaller key first, then the lower rank) and writes 64
//   consecutive 16-byte records.
// k_slack_rank<true>    nvrx_slack.inl's rank kernel reading the pair records of group[r].
// k_slack_group_job<T>  grid G.  T == 0 (max_group <= 64): one wave, member i in lane i, robust_wave_select twice; else one
//   workgroup of T: pace_radix_select<T, 0> over the rank-record words gathered through members[].
//
// d_groups is data, not an argument the host checks can see: start values are clamped to [0, R], a stretch to max_group, a
// member outside [0, R) is skipped, a group id outside [0, G) leaves the rank without a column.  Nothing in it can move a load
// or a store outside the inputs or d_out.
//   No trip count beyond the group's size, no sort, no scratch, no atomics; workgroups of one launch share nothing.

namespace {

// the stretch of group g: members[0 .. size) lie inside the array (s0 + size <= s1 <= R)
__device__ __forceinline__ const int32_t *slack_group_stretch(const SlackGroupArgs &a, int g, int *size) {
    const int32_t *__restrict__ start = a.groups + 2 * (size_t)a.R;
    const int s0 = peer_clamp(start[g], a.R), s1 = peer_clamp(start[g + 1], a.R);
    const int n = s1 > s0 ? s1 - s0 : 0;
    *size = n < a.max_group ? n : a.max_group;
    return a.groups + a.R + s0;
}

__global__ __launch_bounds__(PGROUP_THREADS) void k_slack_group_cols(SlackGroupArgs a) {
    constexpr int NW = PGROUP_THREADS / 64;
    __shared__ uint32_t s_key[NW][SLACK_COLS];
    __shared__ uint32_t s_rank[NW][SLACK_COLS];
    __shared__ uint32_t s_cnt[NW][SLACK_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R;
    const int g = (int)blockIdx.x;  // < G: the grid's extent
    int size;
    const int32_t *__restrict__ members = slack_group_stretch(a, g, &size);

    uint32_t best = 0xFFFFFFFFu;   // (a tie with a present key of this value is broken by the rank, so the first one is taken)
    uint32_t brank = 0xFFFFFFFFu;  // (int) -1
    uint32_t cnt = 0;
    for (int i = wave; i < size; i += NW * PGROUP_UNROLL) {
        int m[PGROUP_UNROLL];
        float t[PGROUP_UNROLL], n[PGROUP_UNROLL];
#pragma unroll
        for (int j = 0; j < PGROUP_UNROLL; j++) {
            const int idx = i + NW * j;
            m[j] = idx < size ? members[idx] : -1;
            const bool in = (uint32_t)m[j] < (uint32_t)R;
            t[j] = in ? a.slack[(size_t)m[j] * 2 * SLACK_COLS + lane] : -1.0f;
            n[j] = in ? a.slack[(size_t)m[j] * 2 * SLACK_COLS + SLACK_COLS + lane] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < PGROUP_UNROLL; j++) {
            const bool present = n[j] > 0.0f && t[j] >= 0.0f;  // slack_entry's rule and quotient
            const uint32_t key = f2key((float)((double)t[j] / (double)n[j]));
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
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < NW; w++) {
        const uint32_t key = s_key[w][lane], rk = s_rank[w][lane];
        const bool take = key < best || (key == best && rk < brank);
        best = take ? key : best;
        brank = take ? rk : brank;
        cnt += s_cnt[w][lane];
    }
    // pace_group_record's rule: min_peers >= 1, so a pair nobody has never is referenced
    const int clamped = a.min_ranks < size ? a.min_ranks : size;
    const int need = a.min_peers > clamped ? a.min_peers : clamped;
    const bool referenced = (int)cnt >= need;
    uint4 *__restrict__ pairs = reinterpret_cast<uint4 *>(a.out + SLACK_GROUP_WORDS * (size_t)a.G);
    pairs[(size_t)g * SLACK_COLS + lane] =
        make_uint4(referenced ? __float_as_uint(key2f(best)) : SLACK_NAN, cnt, referenced ? brank : 0xFFFFFFFFu, (uint32_t)size);
}

// THREADS == 0: one wave, member i in lane i (max_group <= 64); else one workgroup of THREADS
template <int THREADS>
__global__ __launch_bounds__(THREADS ? THREADS : 64) void k_slack_group_job(SlackGroupArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int R = a.R;
    const int g = (int)blockIdx.x;  // < G: the grid's extent
    int size;
    const int32_t *__restrict__ members = slack_group_stretch(a, g, &size);
    const uint32_t *__restrict__ words = a.out + slack_group_rank_base(a.G);               // [R][8]
    const float *__restrict__ recs = reinterpret_cast<const float *>(words);
    uint32_t typical[2] = {SLACK_NAN, SLACK_NAN};
    uint32_t with_data = 0;
    if constexpr (THREADS == 0) {
        size = size < 64 ? size : 64;  // (what the host promised with max_group; a wave has 64 lanes)
        const int m = lane < size ? members[lane] : -1;
        const bool mine = (uint32_t)m < (uint32_t)R;
        with_data = (uint32_t)__popcll(__ballot(mine && words[8 * (size_t)(mine ? m : 0) + 5] != 0u));
#pragma unroll
        for (int w = 0; w < 2; w++) {
            const float v = mine ? recs[8 * (size_t)m + 1 + 2 * w] : -1.0f;
            const bool present = v >= 0.0f;
            const unsigned long long mask = __ballot(present);
            if (mask) {  // wave-uniform
                const uint32_t target = ((uint32_t)__popcll(mask) - 1u) >> 1;
                const int at = robust_wave_select(f2key(v), present, mask, target, size, lane);
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
        for (int i = tid; i < size; i += THREADS) {
            const int m = members[i];
            if ((uint32_t)m >= (uint32_t)R) continue;
            c0 += recs[8 * (size_t)m + 1] >= 0.0f ? 1u : 0u;
            c1 += recs[8 * (size_t)m + 3] >= 0.0f ? 1u : 0u;
            cd += words[8 * (size_t)m + 5] != 0u ? 1u : 0u;
        }
        c0 = wave_sum_u32(c0), c1 = wave_sum_u32(c1), cd = wave_sum_u32(cd);
        if (lane == 0) s_cnt[0][wave] = c0, s_cnt[1][wave] = c1, s_cnt[2][wave] = cd;
        __syncthreads();
        uint32_t cnt[2] = {0, 0};
#pragma unroll
        for (int w = 0; w < WAVES; w++) cnt[0] += s_cnt[0][w], cnt[1] += s_cnt[1][w], with_data += s_cnt[2][w];
#pragma unroll 1
        for (int w = 0; w < 2; w++) {
            const uint32_t n = uni(cnt[w]);
            if (n == 0) continue;  // block-uniform
            // the key of member i < size; the marker where it has no value or is no rank of the table
            auto key_at = [&](int i) -> uint32_t {
                const int m = members[i];
                const float v = (uint32_t)m < (uint32_t)R ? recs[8 * (size_t)m + 1 + 2 * w] : -1.0f;
                return v >= 0.0f ? f2key(v) : PACE_MARK;
            };
            typical[w] = __float_as_uint(key2f(pace_radix_select<THREADS, 0>(key_at, size, (n - 1u) >> 1, s_hist, s_wave, s_sel)));
            __syncthreads();  // (the next selection clears the histogram and rewrites s_wave / s_sel)
        }
    }
    if (tid < 64) {  // the first wave: lane c = column c
        const uint32_t holder = a.out[SLACK_GROUP_WORDS * (size_t)a.G + 4 * ((size_t)g * SLACK_COLS + lane) + 2];
        const uint32_t referenced = (uint32_t)__popcll(__ballot((int)holder >= 0));
        if (tid != 0) return;
        uint4 *rec = reinterpret_cast<uint4 *>(a.out) + 2 * (size_t)g;
        rec[0] = make_uint4(typical[0], typical[1], with_data, referenced);
        rec[1] = make_uint4((uint32_t)size, 0u, 0u, 0u);
    }
}

// argument checks of nvrx_slack_group_score: nvrx_slack_score's in its order, then nvrx_peer_score's of G, then the two of the
// per-group families, then the array; nothing here touches a device
int slack_group_check(const float *d_slack, const float *d_table, int R, int K, int S, const int32_t *d_groups, int G,
                      int max_group, int min_ranks, int min_peers, const void *d_out) {
    int rc = slack_score_check(d_slack, d_table, R, K, S, min_ranks, d_out);
    if (!rc) rc = groups_check(R, G);
    if (rc) return rc;
    if (max_group < 1 || max_group > R) return fail(NVRX_ERR_RANGE, "max_group=%d, within 1..%d", max_group, R);
    if (min_peers < 1) return fail(NVRX_ERR_RANGE, "min_peers=%d, at least 1", min_peers);
    if (!d_groups) return fail(NVRX_ERR_INVALID, "null device pointer");
    return NVRX_OK;
}

int slack_group_launch(const float *d_slack, const float *d_table, int R, int K, int S, const int32_t *d_groups, int G,
                       int max_group, int min_ranks, int min_peers, void *d_out, hipStream_t st) {
    SlackGroupArgs a{};
    a.slack = d_slack, a.table = d_table, a.groups = d_groups;
    a.R = R, a.K = K, a.S = S, a.G = G;
    a.max_group = max_group, a.min_ranks = min_ranks, a.min_peers = min_peers;
    a.out = static_cast<uint32_t *>(d_out);
    hipLaunchKernelGGL(k_slack_group_cols, dim3(G), dim3(PGROUP_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_slack_rank<true, SlackGroupArgs>), dim3((R + 3) / 4), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    if (max_group <= 64)
        hipLaunchKernelGGL(k_slack_group_job<0>, dim3(G), dim3(64), 0, st, a);
    else if (max_group <= 1024)
        hipLaunchKernelGGL(k_slack_group_job<256>, dim3(G), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_slack_group_job<1024>, dim3(G), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_slack_group_score(const float *d_slack, const float *d_table, int R, int K, int S, const int32_t *d_groups, int G,
                           int max_group, int min_ranks, int min_peers, void *d_out, void *stream) {
    const int rc = slack_group_check(d_slack, d_table, R, K, S, d_groups, G, max_group, min_ranks, min_peers, d_out);
    if (rc) return rc;
    return slack_group_launch(d_slack, d_table, R, K, S, d_groups, G, max_group, min_ranks, min_peers, d_out, as_stream(stream));
}

}  // extern "C"
