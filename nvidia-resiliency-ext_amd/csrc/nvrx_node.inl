// nvrx_node.inl -- node scores: tell a slow HOST from a slow GPU.  Part of the translation unit nvrx_straggler.hip (included at
// its end, behind nvrx_pace_group.inl: it uses nvrx_peer.inl's clamp, nvrx_pace.inl's marker, radix select and rank kernel and
// nvrx_pace_group.inl's columns kernel and checks).
//
// Every other score rates a rank; an operator cordons a node.  A chassis whose fans failed, a capped PSU or a throttling host
// CPU makes all GPUs of one node a few per cent slower in everything: the pace scores name eight ranks and cannot say that they
// are one incident.  Here the caller says which ranks share a node (nvrx_peer_score's array, unchanged, a node being a group):
// a column's value of a node is the lower median `med` of its present members (block A: exactly nvrx_pace_group_score's column
// block with min_ranks = min_members and min_peers = 1), the reference point of a column is the lower median N_c of the
// referenced nodes' med -- one node, one vote, whatever their sizes -- (block B), a NODE's pace is nvrx_pace_score's rank record
// with v = med and ctr = N_c (block C), and every reported rank gets the same record against N_c (block D), which says whether
// a node's members agree with it.  The table is the one nvrx_score reads; nothing else is exchanged.
//
// k_node_cols    R <= 64 (so G <= 64): blocks A AND B in one launch.  k_pace_group_cols<0>'s tile and pitch, the rows taken
//                through members[0 .. R): `members` is sorted by node, so node g is the lane range [s_g, s_g + size_g), and
//                lane i knows the range of the node it lies in.  1024 threads; a wave takes four of the tile's columns, one
//                at a time.  Every node's select runs AT ONCE: lane i ranks its key among the present members of its own
//                node, one member per step through ds_bpermute -- the trip count is the largest node's size, not R and not
//                G x size --; a ballot names each node's median lane, two more give the counts, masked to the node's lanes.
//                Lane g then takes node g's record from the first lane of its stretch, and one more select runs across
//                lanes 0 .. G-1.  Stretches that overlap (contents only a damaged array has) take a wave-uniform loop over
//                the nodes with a select masked to each node's lanes instead.  One barrier, no atomics, no scratch.
// k_node_across  R > 64: block A is k_pace_group_cols<T>'s launch; this one reads A's med words for block B.
//   <64>   G <= 64: one column per wave (four per workgroup), node g's med in lane g, robust_wave_select.
//   <256>  beyond (NVRX_PEER_MAX_GROUPS = 4096): one workgroup per column, pace_radix_select<256, 0> over the med words
//          re-read from the L2, and one more strided pass for the counts.
// k_pace_rank<.., .., false, true>  block C: nvrx_pace.inl's rank kernel whose "row" is node g's stretch of A at a stride of
//                four words, without the three sums.  Block D is the job-wide k_pace_rank with cols = B and min_ranks = min_nodes.
//
// d_groups is data: the guards are k_pace_group_cols' (clamped starts, a stretch cut to max_group, skipped members).
//   Always exact, ties included; no sort, no scratch, no global atomics, no float atomics.

namespace {

struct NodeColsArgs {
    const float *table;     // [R][L]
    const int32_t *groups;  // group[R] | members[R] | start[G+1]
    int R, KS, L, G;        // R <= 64, G <= R
    int max_group;
    int min_members, min_nodes;
    uint4 *pairs;  // A [G][KS] {f32 med, u32 n, u32 above, u32 below}
    uint4 *cols;   // B [KS] {f32 N_c, u32 nodes, u32 above, u32 below}
};

// robust_wave_select among the lanes [lo, hi) only: the lane whose key has position `target` among the keys of `mask` (a subset
// of those lanes; ties: the lower lane first).  lo, hi and mask are wave-uniform.
__device__ __forceinline__ int node_range_select(uint32_t key, bool counted, unsigned long long mask, uint32_t target, int lo,
                                                 int hi, int lane) {
    uint32_t pos = 0;
    for (int j = lo; j < hi; j++) {
        const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key, j);
        const bool pj = (mask >> j) & 1ull;
        pos += (pj && (kj < key || (kj == key && j < lane))) ? 1u : 0u;
    }
    const unsigned long long hit = __ballot(counted && pos == target);
    return __ffsll((long long)hit) - 1;
}

// block B's record: N_c is a number iff nodes >= min_nodes (min_nodes >= 1); the counts are always written
__device__ __forceinline__ uint4 node_col_record(uint32_t nkey, uint32_t nodes, uint32_t above, uint32_t below, int min_nodes) {
    const bool referenced = nodes != 0 && (int)nodes >= min_nodes;
    return make_uint4(referenced ? __float_as_uint(key2f(nkey)) : __float_as_uint(__builtin_nanf("")), nodes, above, below);
}

constexpr int NODE_THREADS = 1024;  // 16 waves share a tile's 64 columns: four columns per wave, one after the other

__global__ __launch_bounds__(NODE_THREADS) void k_node_cols(NodeColsArgs a) {
    __shared__ float s_tile[64 * ROBUST_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R < 64 ? a.R : 64, KS = a.KS;  // (what the host promised; the tile has 64 rows)
    const int G = a.G < R ? a.G : R;
    const int32_t *__restrict__ members = a.groups + a.R;
    const int32_t *__restrict__ start = a.groups + 2 * (size_t)a.R;
    const int base = (int)blockIdx.x * ROBUST_TILE;
    {
        const int c = base + lane;
        for (int i = wave; i < R; i += NODE_THREADS / 64) {
            const int m = members[i];
            const bool in = (uint32_t)m < (uint32_t)R && c < KS;
            s_tile[i * ROBUST_PITCH + lane] = in ? a.table[(size_t)m * (size_t)a.L + (size_t)c] : -1.0f;
        }
    }
    // lane g < G: node g's lane range [my_s0, my_s0 + my_size), guarded as k_pace_group_cols guards it
    int my_s0 = 0, my_size = 0;
    if (lane < G) {
        const int s0 = peer_clamp(start[lane], R), s1 = peer_clamp(start[lane + 1], R);
        const int size = s1 > s0 ? s1 - s0 : 0;
        my_s0 = s0, my_size = size < a.max_group ? size : a.max_group;  // s0 + size <= s1 <= R <= 64
    }
    // lane i < R: the range [lo, lo + sz) of the node whose stretch holds member i (sz 0: none does), in how many stretches it
    // lies, and the longest stretch.  An array that PeerGroups built has disjoint stretches; contents that make them overlap
    // (d_groups is data) take the loop over the nodes below.
    int lo = 0, sz = 0, holders = 0, longest = 0;
    for (int g = 0; g < G; g++) {  // wave-uniform; once per wave, not per column
        const int s0 = __builtin_amdgcn_readlane(my_s0, g), size = __builtin_amdgcn_readlane(my_size, g);
        longest = size > longest ? size : longest;
        if (lane >= s0 && lane < s0 + size) holders++, lo = s0, sz = size;
    }
    const bool disjoint = __ballot(holders > 1) == 0ull;  // wave-uniform
    const unsigned long long own = sz >= 64 ? ~0ull : sz == 0 ? 0ull : (((1ull << sz) - 1ull) << lo);  // lo + sz <= 64
    const int own_clamped = a.min_members < sz ? a.min_members : sz;
    const int own_need = own_clamped > 1 ? own_clamped : 1;
    __syncthreads();
    const uint32_t nan = __float_as_uint(__builtin_nanf(""));
    for (int ci = wave; ci < ROBUST_TILE; ci += NODE_THREADS / 64) {
        const int c = base + ci;
        if (c >= KS) break;  // wave-uniform
        const float v = lane < R ? s_tile[lane * ROBUST_PITCH + ci] : -1.0f;
        const bool present = v >= 0.0f;
        const uint32_t key = f2key(v);
        const unsigned long long pmask = __ballot(present);
        uint4 rec = make_uint4(nan, 0u, 0u, 0u);  // lane g: node g's record ...
        uint32_t mkey = 0;                        // ... and the key of its med
        bool mref = false;                        // ... where the pair is referenced
        if (disjoint) {
            // every node at once: lane i ranks its key among the present members of ITS node, one member per step
            const unsigned long long nmask = pmask & own;
            const uint32_t n = (uint32_t)__popcll(nmask);
            const bool mine = present && sz != 0;
            uint32_t pos = 0;
            for (int j = 0; j < longest; j++) {  // wave-uniform
                const int idx = (lo + j) & 63;
                const uint32_t kj = (uint32_t)__shfl((int)key, idx);
                const bool pj = j < sz && ((pmask >> idx) & 1ull);
                pos += (pj && (kj < key || (kj == key && idx < lane))) ? 1u : 0u;
            }
            const unsigned long long meds = __ballot(mine && pos == ((n - 1u) >> 1));  // one lane per node that has data
            const int lc = __ffsll((long long)(meds & own)) - 1;                         // its node's: -1 at n = 0
            const uint32_t fetched = (uint32_t)__shfl((int)key, lc & 63);  // (every lane takes part in the exchange)
            const uint32_t ckey = n != 0 ? fetched : 0u;
            const uint32_t above = (uint32_t)__popcll(__ballot(mine && key > ckey) & own);
            const uint32_t below = (uint32_t)__popcll(__ballot(mine && key < ckey) & own);
            const bool referenced = (int)n >= own_need;
            // node g's figures stand in every lane of its stretch: lane g takes them from the first
            const int src = my_s0 & 63;
            const uint32_t gn = (uint32_t)__shfl((int)n, src), gkey = (uint32_t)__shfl((int)ckey, src);
            const uint32_t gabove = (uint32_t)__shfl((int)above, src), gbelow = (uint32_t)__shfl((int)below, src);
            const bool gref = __shfl(referenced ? 1 : 0, src) != 0;
            if (my_size != 0) {  // (lanes at or above G have my_size 0; so has an empty node: the record above)
                rec = make_uint4(gref ? __float_as_uint(key2f(gkey)) : nan, gn, gabove, gbelow);
                mkey = gkey, mref = gref;
            }
        } else {
            for (int g = 0; g < G; g++) {  // wave-uniform
                const int s0 = __builtin_amdgcn_readlane(my_s0, g), size = __builtin_amdgcn_readlane(my_size, g);
                const unsigned long long range = size >= 64 ? ~0ull : size == 0 ? 0ull : (((1ull << size) - 1ull) << s0);
                const unsigned long long nmask = pmask & range;
                const bool mine = (nmask >> lane) & 1ull;
                const uint32_t n = (uint32_t)__popcll(nmask);
                uint32_t ckey = 0, above = 0, below = 0;
                if (n != 0) {  // wave-uniform
                    const int lc = node_range_select(key, mine, nmask, (n - 1u) >> 1, s0, s0 + size, lane);
                    ckey = (uint32_t)__builtin_amdgcn_readlane((int)key, lc);
                    above = (uint32_t)__popcll(__ballot(mine && key > ckey));
                    below = (uint32_t)__popcll(__ballot(mine && key < ckey));
                }
                const int clamped = a.min_members < size ? a.min_members : size;
                const bool referenced = (int)n >= (clamped > 1 ? clamped : 1);
                if (lane == g) {
                    rec = make_uint4(referenced ? __float_as_uint(key2f(ckey)) : nan, n, above, below);
                    mkey = ckey, mref = referenced;
                }
            }
        }
        if (lane < G) a.pairs[(size_t)lane * (size_t)KS + (size_t)c] = rec;
        const unsigned long long rmask = __ballot(mref);  // (mref only in lanes below G)
        const uint32_t nodes = (uint32_t)__popcll(rmask);
        uint32_t nkey = 0, above = 0, below = 0;
        if (nodes != 0) {  // wave-uniform
            const int lc = node_range_select(mkey, mref, rmask, (nodes - 1u) >> 1, 0, G, lane);
            nkey = (uint32_t)__builtin_amdgcn_readlane((int)mkey, lc);
            above = (uint32_t)__popcll(__ballot(mref && mkey > nkey));
            below = (uint32_t)__popcll(__ballot(mref && mkey < nkey));
        }
        if (lane == 0) a.cols[c] = node_col_record(nkey, nodes, above, below, a.min_nodes);
    }
}

struct NodeAcrossArgs {
    const uint4 *pairs;  // A [G][KS]
    int G, KS;
    int min_nodes;
    uint4 *cols;  // B [KS]
};

// THREADS 64: one column per wave, ROBUST_THREADS threads (G <= 64); 256: one workgroup per column
template <int THREADS>
__global__ __launch_bounds__(THREADS == 64 ? ROBUST_THREADS : THREADS) void k_node_across(NodeAcrossArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = a.G, KS = a.KS;
    if constexpr (THREADS == 64) {
        const int c = (int)blockIdx.x * (ROBUST_THREADS / 64) + wave;
        if (c >= KS) return;  // wave-uniform; no barrier below
        const float med = lane < G ? __uint_as_float(a.pairs[(size_t)lane * (size_t)KS + (size_t)c].x) : __builtin_nanf("");
        const bool mref = med == med;  // a referenced pair's med is an actual value, never NaN
        const uint32_t mkey = f2key(med);
        const unsigned long long rmask = __ballot(mref);
        const uint32_t nodes = (uint32_t)__popcll(rmask);
        uint32_t nkey = 0, above = 0, below = 0;
        if (nodes != 0) {  // wave-uniform
            const int lc = robust_wave_select(mkey, mref, rmask, (nodes - 1u) >> 1, G < 64 ? G : 64, lane);
            nkey = (uint32_t)__builtin_amdgcn_readlane((int)mkey, lc);
            above = (uint32_t)__popcll(__ballot(mref && mkey > nkey));
            below = (uint32_t)__popcll(__ballot(mref && mkey < nkey));
        }
        if (lane == 0) a.cols[c] = node_col_record(nkey, nodes, above, below, a.min_nodes);
    } else {
        constexpr int WAVES = THREADS / 64;
        __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
        __shared__ uint32_t s_wave[WAVES];
        __shared__ uint32_t s_sel[2];
        __shared__ uint32_t s_cnt[2][WAVES];
        const int c = (int)blockIdx.x;  // < KS: the grid's extent
        const uint4 *__restrict__ col = a.pairs + c;
        // the key of node i < G; the marker where the pair is not referenced
        auto key_at = [&](int i) -> uint32_t {
            const float med = __uint_as_float(col[(size_t)i * (size_t)KS].x);
            return med == med ? f2key(med) : PACE_MARK;
        };
        uint32_t cnt = 0;
        for (int i = tid; i < G; i += THREADS) cnt += key_at(i) != PACE_MARK ? 1u : 0u;
        cnt = wave_sum_u32(cnt);
        if (lane == 0) s_wave[wave] = cnt;
        __syncthreads();
        uint32_t nodes = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) nodes += s_wave[w];
        nodes = uni(nodes);
        if (nodes == 0) {  // block-uniform
            if (tid == 0) a.cols[c] = node_col_record(0u, 0u, 0u, 0u, a.min_nodes);
            return;
        }
        // (s_wave is rewritten only behind the first pass' two barriers)
        const uint32_t nkey = pace_radix_select<THREADS, 0>(key_at, G, (nodes - 1u) >> 1, s_hist, s_wave, s_sel);
        uint32_t above = 0, below = 0;
        for (int i = tid; i < G; i += THREADS) {
            const uint32_t key = key_at(i);
            above += (key != PACE_MARK && key > nkey) ? 1u : 0u;
            below += key < nkey ? 1u : 0u;  // (the marker is above every key)
        }
        above = wave_sum_u32(above);
        below = wave_sum_u32(below);
        if (lane == 0) s_cnt[0][wave] = above, s_cnt[1][wave] = below;
        __syncthreads();
        if (tid == 0) {
            above = below = 0;
            for (int w = 0; w < WAVES; w++) above += s_cnt[0][w], below += s_cnt[1][w];
            a.cols[c] = node_col_record(nkey, nodes, above, below, a.min_nodes);
        }
    }
}

constexpr int NODE_FUSED_RANKS = 64;  // ranks of the largest table k_node_cols takes

// argument checks shared by both entry points: nvrx_pace_group_score's in its order (its two thresholds are not this family's),
// then the two of this family; nothing here touches a device
int node_check(int R, int K, int S, int G, int max_group, int first_rank, int n_ranks, int min_members, int min_nodes) {
    const int rc = pace_group_check(R, K, S, G, max_group, first_rank, n_ranks, 1, 1);
    if (rc) return rc;
    if (min_members < 1) return fail(NVRX_ERR_RANGE, "min_members=%d, at least 1", min_members);
    if (min_nodes < 1) return fail(NVRX_ERR_RANGE, "min_nodes=%d, at least 1", min_nodes);
    return NVRX_OK;
}

int node_launch(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int max_group, int min_members,
                int min_nodes, int first_rank, int n_ranks, void *d_out, hipStream_t st) {
    const int KS = K + S;
    uint4 *pairs = static_cast<uint4 *>(d_out);
    uint4 *cols = pairs + (size_t)G * (size_t)KS;
    uint4 *nodes = cols + (size_t)KS;
    uint4 *ranks = nodes + 4 * (size_t)G;
    if (KS > 0 && R <= NODE_FUSED_RANKS) {
        NodeColsArgs c{};
        c.table = d_table, c.groups = d_groups, c.R = R, c.KS = KS, c.L = NVRX_TABLE_LEN(K, S), c.G = G;
        c.max_group = max_group, c.min_members = min_members, c.min_nodes = min_nodes;
        c.pairs = pairs, c.cols = cols;
        hipLaunchKernelGGL(k_node_cols, dim3((KS + ROBUST_TILE - 1) / ROBUST_TILE), dim3(NODE_THREADS), 0, st, c);
        HIP_TRY(hipGetLastError());
    } else if (KS > 0) {
        PaceGroupColsArgs c{};
        c.table = d_table, c.groups = d_groups, c.R = R, c.KS = KS, c.L = NVRX_TABLE_LEN(K, S);
        c.max_group = max_group, c.min_ranks = min_members, c.min_peers = 1;
        c.cols = pairs;
        pace_group_cols_launch(c, G, st);
        HIP_TRY(hipGetLastError());
        NodeAcrossArgs x{};
        x.pairs = pairs, x.G = G, x.KS = KS, x.min_nodes = min_nodes, x.cols = cols;
        if (G <= 64)
            hipLaunchKernelGGL(k_node_across<64>, dim3((KS + ROBUST_THREADS / 64 - 1) / (ROBUST_THREADS / 64)), dim3(ROBUST_THREADS), 0, st, x);
        else
            hipLaunchKernelGGL(k_node_across<256>, dim3(KS), dim3(256), 0, st, x);
        HIP_TRY(hipGetLastError());
    }
    // block C: the rank kernel over the nodes' stretches of A (its "table"), every eligible column decided by the two centres
    PaceRankArgs n{};
    n.table = reinterpret_cast<const float *>(pairs), n.cols = cols;
    n.K = K, n.S = S, n.first_rank = 0, n.min_ranks = 1;
    n.out = nodes;
    pace_rank_launch<false, true>(n, G, st);
    HIP_TRY(hipGetLastError());
    // block D: the job-wide rank kernel with block B as its column records
    PaceRankArgs r{};
    r.table = d_table, r.cols = cols;
    r.K = K, r.S = S, r.first_rank = first_rank, r.min_ranks = min_nodes;
    r.out = ranks;
    pace_rank_launch(r, n_ranks, st);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_node_score(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int max_group, int min_members,
                    int min_nodes, int first_rank, int n_ranks, void *d_out, void *stream) {
    const int rc = node_check(R, K, S, G, max_group, first_rank, n_ranks, min_members, min_nodes);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_table && d_groups, false)) return rc;
    return node_launch(d_table, R, K, S, d_groups, G, max_group, min_members, min_nodes, first_rank, n_ranks, d_out,
                       as_stream(stream));
}

int nvrx_report_node(nvrx_ctx *ctx, const nvrx_report_desc *desc, const int32_t *d_groups, int G, int max_group, int min_members,
                     int min_nodes, int first_rank, int n_ranks, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = node_check(desc->R, desc->K, desc->S, G, max_group, first_rank, n_ranks, min_members, min_nodes);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_groups != nullptr, true)) return rc;
    hipStream_t home = nullptr;
    const float *table = nullptr;
    if (const int rc = report_table(ctx, desc, &home, &table)) return rc;
    return node_launch(table, desc->R, desc->K, desc->S, d_groups, G, max_group, min_members, min_nodes, first_rank, n_ranks,
                       d_out, home);
}

}  // extern "C"
