// nvrx_node_group.inl -- node scores per peer group: the slow HOST in a job of pipeline stages, tensor-parallel or expert groups.
// Part of the translation unit nvrx_straggler.hip (included at its end, behind nvrx_node.inl: it uses that file's range select
// and checks, nvrx_pace.inl's marker, radix select, deviation key, store and rank kernel and nvrx_pace_group.inl's columns kernel).
//
// nvrx_node.inl takes a column's centre across ALL nodes of the job: a lockstep model.  With two stages at 1000 and 1500 us the
// lower median of the nodes lies in the fast stage, and every node of the slow one is slower in everything.  Here a node is
// compared with the nodes doing the SAME work.  A CELL is a non-empty intersection of a node and a peer group: a column's value
// of a cell is the lower median `med` of its present members (block A: nvrx_pace_group_score's column block, the cells being
// the groups), the reference of a (peer group, column) is the lower median N_gc of its referenced cells' med -- one cell, one
// vote -- (block B), a NODE's record is taken over all its (cell, column) pairs, each quotient against the centre of the cell's
// own group (block C), and every reported rank gets the pace record against its own group's N_gc (block D: the grouped
// k_pace_rank with cols = B, unchanged).  The table is the one nvrx_score reads; nothing else is exchanged.
//
// k_node_group_cols    R <= 64 (so C <= 64): blocks A AND B in one launch.  k_node_cols' tile, pitch and gather through
//                      members[]; members are sorted by (peer group, node), so cell j is a lane range and group p's cells are
//                      the consecutive lanes [gstart[p], gstart[p+1]) of the lanes that hold the cells' records.  The SAME
//                      segmented select runs twice: every cell's at once over the members (trip count: the largest cell), lane
//                      j < C takes cell j's record, then every group's at once over those lanes (trip count: the largest
//                      group's cell count), lane p < Gp writes B's record.  Stretches that overlap at either level (contents
//                      only a damaged array has) take a wave-uniform loop over the segments.  One barrier, no atomics, no scratch.
// k_node_group_across  R > 64: block A is k_pace_group_cols<T>'s launch on the cell array; this one reads A's med words.
//   <64>   groups of at most 64 cells: one (group, column) per wave, the cell's med in its lane, robust_wave_select.  (One
//          group per wave was kept; packing several small groups into a wave was not tried: docs/MEASUREMENTS.md.)
//   <256>  larger groups: one workgroup per (group, column), pace_radix_select<256, 0> over the med words re-read from the L2 and
//          one more strided pass for the counts.
// k_node_group_rank    block C, grid (Gn, 2).  A node's "row" is a gather: item i is (cell i / ncols of the node's list, column
//                      i % ncols of the part), its quotient N_gc / med with g the CELL's group.
//   <64, 1>    up to 64 items: one wave, robust_wave_select twice.
//   <256, 16>  up to 4096 items: the quotients' keys in registers, pace_radix_select from them for pace and spread.
//   <1024, 0>  beyond: the passes re-read A and B from the L2.
//
// d_cells is data: starts clamped, stretches cut to the stated maxima, entries outside their range skipped.  Nothing in it can
// move a load or a store outside the table, the array or d_out.
//   Always exact, ties included; no sort, no scratch, no global atomics, no float atomics.

namespace {

// d_cells, cut into its parts (include/nvrx_straggler.h states the layout)
struct NodeGroupCells {
    const int32_t *cells;   // cell[R] | members[R] | cstart[C+1]: nvrx_peer_score's array, a cell being a group
    const int32_t *gstart;  // [Gp+1]: group p's cells are the cell ids gstart[p] .. gstart[p+1]
    const int32_t *nstart;  // [Gn+1]: node n's cells are ncells[nstart[n] .. nstart[n+1])
    const int32_t *ncells;  // [C]
    const int32_t *cgroup;  // [C]: the peer group of a cell
    const int32_t *rgroup;  // [R]: the peer group of a rank
};

NodeGroupCells node_group_cut(const int32_t *d, int R, int C, int Gp, int Gn) {
    NodeGroupCells o;
    o.cells = d;
    o.gstart = d + 2 * (size_t)R + (size_t)C + 1;
    o.nstart = o.gstart + Gp + 1;
    o.ncells = o.nstart + Gn + 1;
    o.cgroup = o.ncells + C;
    o.rgroup = o.cgroup + C;
    return o;
}

// A wave's lanes cut into segments: lane g < G describes segment g as [my_s0, my_s0 + my_size), inside [0, 64).  Every lane
// learns the segment it lies in (sz 0: none), the longest segment, and whether any lane lies in two.
struct NodeGroupSegs {
    int lo, sz, longest;
    unsigned long long own;  // the lanes of the lane's own segment
    bool disjoint;           // wave-uniform
};

__device__ __forceinline__ NodeGroupSegs node_group_segs(int my_s0, int my_size, int G, int lane) {
    NodeGroupSegs s;
    s.lo = s.sz = s.longest = 0;
    int holders = 0;
    for (int g = 0; g < G; g++) {  // wave-uniform; once per wave, not per column
        const int s0 = __builtin_amdgcn_readlane(my_s0, g), size = __builtin_amdgcn_readlane(my_size, g);
        s.longest = size > s.longest ? size : s.longest;
        if (lane >= s0 && lane < s0 + size) holders++, s.lo = s0, s.sz = size;
    }
    s.disjoint = __ballot(holders > 1) == 0ull;
    s.own = s.sz >= 64 ? ~0ull : s.sz == 0 ? 0ull : (((1ull << s.sz) - 1ull) << s.lo);  // lo + sz <= 64
    return s;
}

struct NodeGroupSel {
    uint32_t n, ckey, above, below;
};

// EVERY segment's select at once (disjoint segments): each lane ranks its key among the counted lanes of its own segment, one
// lane per step; a ballot names each segment's median lane, two more give the counts.  Every lane of a segment gets the
// segment's figures (zeros where nothing is counted); a lane in no segment gets zeros.
__device__ __forceinline__ NodeGroupSel node_group_select_all(uint32_t key, bool counted, const NodeGroupSegs &s, int lane) {
    const unsigned long long cmask = __ballot(counted);
    NodeGroupSel o;
    o.n = (uint32_t)__popcll(cmask & s.own);
    const bool mine = counted && s.sz != 0;
    uint32_t pos = 0;
    for (int j = 0; j < s.longest; j++) {  // wave-uniform
        const int idx = (s.lo + j) & 63;
        const uint32_t kj = (uint32_t)__shfl((int)key, idx);
        const bool pj = j < s.sz && ((cmask >> idx) & 1ull);
        pos += (pj && (kj < key || (kj == key && idx < lane))) ? 1u : 0u;
    }
    const unsigned long long meds = __ballot(mine && pos == ((o.n - 1u) >> 1));  // one lane per segment that counts anything
    const int lc = __ffsll((long long)(meds & s.own)) - 1;                          // its segment's: -1 at n = 0
    const uint32_t fetched = (uint32_t)__shfl((int)key, lc & 63);                   // (every lane takes part in the exchange)
    o.ckey = o.n != 0 ? fetched : 0u;
    o.above = (uint32_t)__popcll(__ballot(mine && key > o.ckey) & s.own);
    o.below = (uint32_t)__popcll(__ballot(mine && key < o.ckey) & s.own);
    return o;
}

// ONE segment [s0, s0 + size) (wave-uniform, inside [0, 64)): the same figures, wave-uniform.
__device__ __forceinline__ NodeGroupSel node_group_select_one(uint32_t key, unsigned long long cmask, int s0, int size, int lane) {
    const unsigned long long range = size >= 64 ? ~0ull : size == 0 ? 0ull : (((1ull << size) - 1ull) << s0);
    const unsigned long long nmask = cmask & range;
    const bool mine = (nmask >> lane) & 1ull;
    NodeGroupSel o;
    o.n = (uint32_t)__popcll(nmask), o.ckey = o.above = o.below = 0;
    if (o.n != 0) {  // wave-uniform
        const int lc = node_range_select(key, mine, nmask, (o.n - 1u) >> 1, s0, s0 + size, lane);
        o.ckey = (uint32_t)__builtin_amdgcn_readlane((int)key, lc);
        o.above = (uint32_t)__popcll(__ballot(mine && key > o.ckey));
        o.below = (uint32_t)__popcll(__ballot(mine && key < o.ckey));
    }
    return o;
}

// Both levels of the fused kernel: lane g < G takes segment g's figures -- from the first lane of its stretch where the
// segments are disjoint, else from a loop over the segments.
__device__ __forceinline__ NodeGroupSel node_group_level(uint32_t key, bool counted, const NodeGroupSegs &s, int my_s0, int my_size,
                                                         int G, int lane) {
    NodeGroupSel o;
    if (s.disjoint) {
        const NodeGroupSel all = node_group_select_all(key, counted, s, lane);
        const int src = my_s0 & 63;
        o.n = (uint32_t)__shfl((int)all.n, src), o.ckey = (uint32_t)__shfl((int)all.ckey, src);
        o.above = (uint32_t)__shfl((int)all.above, src), o.below = (uint32_t)__shfl((int)all.below, src);
        if (my_size == 0) o.n = o.ckey = o.above = o.below = 0;  // (an empty segment, and the lanes at or above G)
    } else {
        const unsigned long long cmask = __ballot(counted);
        o.n = o.ckey = o.above = o.below = 0;
        for (int g = 0; g < G; g++) {  // wave-uniform
            const int s0 = __builtin_amdgcn_readlane(my_s0, g), size = __builtin_amdgcn_readlane(my_size, g);
            const NodeGroupSel one = node_group_select_one(key, cmask, s0, size, lane);
            if (lane == g) o = one;
        }
    }
    return o;
}

// a record of block A or B: the centre is a number iff n >= max(floor, min(least, size)); floor >= 1
__device__ __forceinline__ bool node_group_referenced(uint32_t n, int size, int least, int floor) {
    const int clamped = least < size ? least : size;
    return (int)n >= (floor > clamped ? floor : clamped);
}

__device__ __forceinline__ uint4 node_group_record(const NodeGroupSel &s, bool referenced) {
    return make_uint4(referenced ? __float_as_uint(key2f(s.ckey)) : __float_as_uint(__builtin_nanf("")), s.n, s.above, s.below);
}

struct NodeGroupColsArgs {
    const float *table;     // [R][L]
    const int32_t *cells;   // cell[R] | members[R] | cstart[C+1]
    const int32_t *gstart;  // [Gp+1]
    int R, KS, L, C, Gp;    // R <= 64, Gp <= C <= R
    int max_cell, max_group_cells;
    int min_members, min_nodes, min_peers;
    uint4 *pairs;  // A [C][KS] {f32 med, u32 n, u32 above, u32 below}
    uint4 *cols;   // B [Gp][KS] {f32 N_gc, u32 nodes, u32 above, u32 below}
};

__global__ __launch_bounds__(NODE_THREADS) void k_node_group_cols(NodeGroupColsArgs a) {
    __shared__ float s_tile[64 * ROBUST_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R < 64 ? a.R : 64, KS = a.KS;  // (what the host promised; the tile has 64 rows)
    const int C = a.C < R ? a.C : R;
    const int Gp = a.Gp < C ? a.Gp : C;
    const int32_t *__restrict__ members = a.cells + a.R;
    const int32_t *__restrict__ cstart = a.cells + 2 * (size_t)a.R;
    const int base = (int)blockIdx.x * ROBUST_TILE;
    {
        const int c = base + lane;
        for (int i = wave; i < R; i += NODE_THREADS / 64) {
            const int m = members[i];
            const bool in = (uint32_t)m < (uint32_t)R && c < KS;
            s_tile[i * ROBUST_PITCH + lane] = in ? a.table[(size_t)m * (size_t)a.L + (size_t)c] : -1.0f;
        }
    }
    // lane j < C: cell j's range of member lanes; lane p < Gp: group p's range of cell lanes.  Both guarded as k_pace_group_cols
    // guards a stretch: s0 + size <= s1 <= the clamp <= 64.
    int c_s0 = 0, c_size = 0, g_s0 = 0, g_size = 0;
    if (lane < C) {
        const int s0 = peer_clamp(cstart[lane], R), s1 = peer_clamp(cstart[lane + 1], R);
        const int size = s1 > s0 ? s1 - s0 : 0;
        c_s0 = s0, c_size = size < a.max_cell ? size : a.max_cell;
    }
    if (lane < Gp) {
        const int s0 = peer_clamp(a.gstart[lane], C), s1 = peer_clamp(a.gstart[lane + 1], C);
        const int size = s1 > s0 ? s1 - s0 : 0;
        g_s0 = s0, g_size = size < a.max_group_cells ? size : a.max_group_cells;
    }
    const NodeGroupSegs cs = node_group_segs(c_s0, c_size, C, lane);
    const NodeGroupSegs gs = node_group_segs(g_s0, g_size, Gp, lane);
    __syncthreads();
    for (int ci = wave; ci < ROBUST_TILE; ci += NODE_THREADS / 64) {
        const int c = base + ci;
        if (c >= KS) break;  // wave-uniform
        const float v = lane < R ? s_tile[lane * ROBUST_PITCH + ci] : -1.0f;
        // block A: lane j < C holds cell j's record and the key of its med
        const NodeGroupSel cell = node_group_level(f2key(v), v >= 0.0f, cs, c_s0, c_size, C, lane);
        const bool mref = node_group_referenced(cell.n, c_size, a.min_members, 1);  // (n = 0 in the lanes at or above C)
        if (lane < C) a.pairs[(size_t)lane * (size_t)KS + (size_t)c] = node_group_record(cell, mref);
        // block B: the same select over the lanes 0 .. C-1, a group's cells a lane range
        const NodeGroupSel grp = node_group_level(cell.ckey, mref, gs, g_s0, g_size, Gp, lane);
        if (lane < Gp)
            a.cols[(size_t)lane * (size_t)KS + (size_t)c] =
                node_group_record(grp, node_group_referenced(grp.n, g_size, a.min_nodes, a.min_peers));
    }
}

struct NodeGroupAcrossArgs {
    const uint4 *pairs;     // A [C][KS]
    const int32_t *gstart;  // [Gp+1]
    int C, KS;
    int max_group_cells;
    int min_nodes, min_peers;
    uint4 *cols;  // B [Gp][KS]
};

// THREADS 64: one (group, column) per wave, ROBUST_THREADS threads, grid (ceil(KS / 4), Gp); 256: one workgroup per (group,
// column), grid (KS, Gp)
template <int THREADS>
__global__ __launch_bounds__(THREADS == 64 ? ROBUST_THREADS : THREADS) void k_node_group_across(NodeGroupAcrossArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, KS = a.KS;
    const int g = (int)blockIdx.y;  // < Gp: the grid's extent
    const int s0 = peer_clamp(a.gstart[g], C), s1 = peer_clamp(a.gstart[g + 1], C);
    int size = s1 > s0 ? s1 - s0 : 0;
    size = size < a.max_group_cells ? size : a.max_group_cells;  // the cells s0 .. s0 + size lie inside A: s0 + size <= s1 <= C
    uint4 *__restrict__ cols = a.cols + (size_t)g * (size_t)KS;
    if constexpr (THREADS == 64) {
        size = size < 64 ? size : 64;  // (what the host promised with max_group_cells)
        const int c = (int)blockIdx.x * (ROBUST_THREADS / 64) + wave;
        if (c >= KS) return;  // wave-uniform; no barrier below
        const float med = lane < size ? __uint_as_float(a.pairs[(size_t)(s0 + lane) * (size_t)KS + (size_t)c].x) : __builtin_nanf("");
        const bool mref = med == med;  // a referenced pair's med is an actual value, never NaN
        const uint32_t mkey = f2key(med);
        const unsigned long long rmask = __ballot(mref);
        NodeGroupSel o;
        o.n = (uint32_t)__popcll(rmask), o.ckey = o.above = o.below = 0;
        if (o.n != 0) {  // wave-uniform
            const int lc = robust_wave_select(mkey, mref, rmask, (o.n - 1u) >> 1, size, lane);
            o.ckey = (uint32_t)__builtin_amdgcn_readlane((int)mkey, lc);
            o.above = (uint32_t)__popcll(__ballot(mref && mkey > o.ckey));
            o.below = (uint32_t)__popcll(__ballot(mref && mkey < o.ckey));
        }
        if (lane == 0) cols[c] = node_group_record(o, node_group_referenced(o.n, size, a.min_nodes, a.min_peers));
    } else {
        constexpr int WAVES = THREADS / 64;
        __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
        __shared__ uint32_t s_wave[WAVES];
        __shared__ uint32_t s_sel[2];
        __shared__ uint32_t s_cnt[2][WAVES];
        const int c = (int)blockIdx.x;  // < KS: the grid's extent
        const uint4 *__restrict__ col = a.pairs + (size_t)s0 * (size_t)KS + (size_t)c;
        // the key of the group's cell i < size; the marker where the pair is not referenced
        auto key_at = [&](int i) -> uint32_t {
            const float med = __uint_as_float(col[(size_t)i * (size_t)KS].x);
            return med == med ? f2key(med) : PACE_MARK;
        };
        uint32_t cnt = 0;
        for (int i = tid; i < size; i += THREADS) cnt += key_at(i) != PACE_MARK ? 1u : 0u;
        cnt = wave_sum_u32(cnt);
        if (lane == 0) s_wave[wave] = cnt;
        __syncthreads();
        NodeGroupSel o;
        o.n = o.ckey = o.above = o.below = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) o.n += s_wave[w];
        o.n = uni(o.n);
        if (o.n == 0) {  // block-uniform
            if (tid == 0) cols[c] = node_group_record(o, false);
            return;
        }
        // (s_wave is rewritten only behind the first pass' two barriers)
        o.ckey = pace_radix_select<THREADS, 0>(key_at, size, (o.n - 1u) >> 1, s_hist, s_wave, s_sel);
        uint32_t above = 0, below = 0;
        for (int i = tid; i < size; i += THREADS) {
            const uint32_t key = key_at(i);
            above += (key != PACE_MARK && key > o.ckey) ? 1u : 0u;
            below += key < o.ckey ? 1u : 0u;  // (the marker is above every key)
        }
        above = wave_sum_u32(above);
        below = wave_sum_u32(below);
        if (lane == 0) s_cnt[0][wave] = above, s_cnt[1][wave] = below;
        __syncthreads();
        if (tid == 0) {
            for (int w = 0; w < WAVES; w++) o.above += s_cnt[0][w], o.below += s_cnt[1][w];
            cols[c] = node_group_record(o, node_group_referenced(o.n, size, a.min_nodes, a.min_peers));
        }
    }
}

struct NodeGroupRankArgs {
    const uint4 *pairs;     // A [C][KS]
    const uint4 *cols;      // B [Gp][KS]
    const int32_t *nstart;  // [Gn+1]
    const int32_t *ncells;  // [C]
    const int32_t *cgroup;  // [C]
    int K, S, C, Gp;
    int max_node_cells;
    uint4 *out;  // C [Gn][2] records of two 16-byte words
};

// One (cell of the node, column of the part) pair: what the counts take from it and the key of its quotient (pace_column's
// arithmetic with v = the cell's med -- NaN, so not present, where the pair is not referenced -- and ctr = the centre of the
// cell's group, a number exactly where that pair is referenced).  list[0 .. cells) lies inside ncells; an entry outside [0, C) or
// a cell whose group is outside [0, Gp) has no eligible column.
struct NodeGroupItem {
    uint32_t qkey;
    bool eligible, slower, faster;
};

__device__ __forceinline__ NodeGroupItem node_group_item(const NodeGroupRankArgs &a, const int32_t *__restrict__ list, int cells,
                                                         int ncols, int base, int i) {
    NodeGroupItem o;
    o.qkey = PACE_MARK, o.eligible = o.slower = o.faster = false;
    if (i < cells * ncols) {
        const int at = i / ncols, col = base + (i - at * ncols);
        const int cell = list[at];
        const int g = (uint32_t)cell < (uint32_t)a.C ? a.cgroup[cell] : -1;
        if ((uint32_t)g < (uint32_t)a.Gp) {
            const size_t KS = (size_t)a.K + (size_t)a.S;
            const float v = __uint_as_float(a.pairs[(size_t)cell * KS + (size_t)col].x);
            const float ctr = __uint_as_float(a.cols[(size_t)g * KS + (size_t)col].x);
            o.eligible = v >= 0.0f && ctr == ctr;
            const uint32_t kv = f2key(v), kc = f2key(ctr);
            o.slower = o.eligible && kv > kc;
            o.faster = o.eligible && kv < kc;
            const float q = (float)((double)ctr / (double)v);
            o.qkey = (o.eligible && q == q) ? f2key(q) : PACE_MARK;
        }
    }
    return o;
}

// THREADS 64 (NREG 1): one wave, one item per lane; 256 with NREG 16: keys in registers; 1024 with NREG 0: re-reading
template <int THREADS, int NREG>
__global__ __launch_bounds__(THREADS) void k_node_group_rank(NodeGroupRankArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int part = (int)blockIdx.y;
    const int ncols = part ? a.S : a.K;
    const int base = part ? a.K : 0;
    const int node = (int)blockIdx.x;  // < Gn: the grid's extent
    const int s0 = peer_clamp(a.nstart[node], a.C), s1 = peer_clamp(a.nstart[node + 1], a.C);
    int cells = s1 > s0 ? s1 - s0 : 0;
    cells = cells < a.max_node_cells ? cells : a.max_node_cells;  // s0 + cells <= s1 <= C; cells * ncols is what the host sized for
    const int32_t *__restrict__ list = a.ncells + s0;
    const int items = cells * ncols;
    uint4 *__restrict__ dst = a.out + ((size_t)node * 2 + (size_t)part) * 2;
    const float NaN = __builtin_nanf("");

    if constexpr (THREADS == 64) {
        const NodeGroupItem it = node_group_item(a, list, cells, ncols, base, lane);
        const bool has_q = it.qkey != PACE_MARK;
        const uint32_t columns = (uint32_t)__popcll(__ballot(it.eligible));
        const uint32_t slower = (uint32_t)__popcll(__ballot(it.slower));
        const uint32_t faster = (uint32_t)__popcll(__ballot(it.faster));
        const unsigned long long mask = __ballot(has_q);
        const uint32_t m = (uint32_t)__popcll(mask);
        float pace = NaN, spread = NaN;
        if (m != 0) {  // wave-uniform
            const uint32_t target = (m - 1u) >> 1;
            const int width = items < 64 ? items : 64;
            const int lp = robust_wave_select(it.qkey, has_q, mask, target, width, lane);
            pace = key2f((uint32_t)__builtin_amdgcn_readlane((int)it.qkey, lp));
            const uint32_t d = pace_dev_key(it.qkey, pace);
            const int ls = robust_wave_select(d, has_q, mask, target, width, lane);
            spread = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)d, ls));
        }
        if (lane == 0) pace_store(dst, pace, spread, columns, slower, faster, 0.0, 0.0, 0.0);
    } else {
        constexpr int WAVES = THREADS / 64;
        constexpr int NKEYS = NREG ? NREG : 1;
        __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
        __shared__ uint32_t s_wave[WAVES];
        __shared__ uint32_t s_sel[2];
        __shared__ uint32_t s_cnt[4][WAVES];
        uint32_t keys[NKEYS];
        uint32_t columns = 0, slower = 0, faster = 0, m = 0;
        auto take = [&](const NodeGroupItem &it) {
            columns += it.eligible ? 1u : 0u;
            slower += it.slower ? 1u : 0u;
            faster += it.faster ? 1u : 0u;
            m += it.qkey != PACE_MARK ? 1u : 0u;
        };
        if constexpr (NREG > 0) {
#pragma unroll
            for (int j = 0; j < NREG; j++) {
                const NodeGroupItem it = node_group_item(a, list, cells, ncols, base, tid + j * THREADS);
                keys[j] = it.qkey;
                take(it);
            }
        } else {
            keys[0] = PACE_MARK;
            for (int i = tid; i < items; i += THREADS) take(node_group_item(a, list, cells, ncols, base, i));
        }
        columns = wave_sum_u32(columns);
        slower = wave_sum_u32(slower);
        faster = wave_sum_u32(faster);
        m = wave_sum_u32(m);
        if (lane == 0) s_cnt[0][wave] = columns, s_cnt[1][wave] = slower, s_cnt[2][wave] = faster, s_cnt[3][wave] = m;
        __syncthreads();
        m = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) m += s_cnt[3][w];
        m = uni(m);
        float pace = NaN, spread = NaN;
        if (m != 0) {  // block-uniform
            const uint32_t target = (m - 1u) >> 1;
            if constexpr (NREG > 0) {
                pace = key2f(pace_radix_select<THREADS, NREG>([&](int j) { return keys[j]; }, items, target, s_hist, s_wave, s_sel));
                spread = __uint_as_float(pace_radix_select<THREADS, NREG>([&](int j) { return pace_dev_key(keys[j], pace); }, items,
                                                                          target, s_hist, s_wave, s_sel));
            } else {
                pace = key2f(pace_radix_select<THREADS, 0>([&](int i) { return node_group_item(a, list, cells, ncols, base, i).qkey; },
                                                           items, target, s_hist, s_wave, s_sel));
                spread = __uint_as_float(pace_radix_select<THREADS, 0>(
                    [&](int i) { return pace_dev_key(node_group_item(a, list, cells, ncols, base, i).qkey, pace); }, items, target,
                    s_hist, s_wave, s_sel));
            }
        }
        if (tid == 0) {
            columns = slower = faster = 0;
            for (int w = 0; w < WAVES; w++) columns += s_cnt[0][w], slower += s_cnt[1][w], faster += s_cnt[2][w];
            pace_store(dst, pace, spread, columns, slower, faster, 0.0, 0.0, 0.0);
        }
    }
}

constexpr int NODE_GROUP_WAVE_CELLS = 64;  // cells of the largest group k_node_group_across<64> takes

// argument checks shared by both entry points: nvrx_node_score's in its order with the cells as its groups, then this family's
// counts, maxima and threshold; nothing here touches a device
int node_group_check(int R, int K, int S, int C, int Gp, int Gn, int max_cell, int max_group_cells, int max_node_cells,
                     int min_members, int min_nodes, int min_peers, int first_rank, int n_ranks) {
    const int rc = node_check(R, K, S, C, max_cell, first_rank, n_ranks, min_members, min_nodes);
    if (rc) return rc;
    if (Gp < 1 || Gp > C) return fail(NVRX_ERR_RANGE, "Gp=%d peer groups, within 1..C=%d", Gp, C);
    if (Gn < 1 || Gn > C) return fail(NVRX_ERR_RANGE, "Gn=%d nodes, within 1..C=%d", Gn, C);
    if (max_group_cells < 1 || max_group_cells > C)
        return fail(NVRX_ERR_RANGE, "max_group_cells=%d, within 1..%d", max_group_cells, C);
    if (max_node_cells < 1 || max_node_cells > C) return fail(NVRX_ERR_RANGE, "max_node_cells=%d, within 1..%d", max_node_cells, C);
    if (min_peers < 1) return fail(NVRX_ERR_RANGE, "min_peers=%d, at least 1", min_peers);
    return NVRX_OK;
}

int node_group_launch(const float *d_table, int R, int K, int S, const int32_t *d_cells, int C, int Gp, int Gn, int max_cell,
                      int max_group_cells, int max_node_cells, int min_members, int min_nodes, int min_peers, int first_rank,
                      int n_ranks, void *d_out, hipStream_t st) {
    const int KS = K + S;
    const NodeGroupCells cut = node_group_cut(d_cells, R, C, Gp, Gn);
    uint4 *pairs = static_cast<uint4 *>(d_out);
    uint4 *cols = pairs + (size_t)C * (size_t)KS;
    uint4 *nodes = cols + (size_t)Gp * (size_t)KS;
    uint4 *ranks = nodes + 4 * (size_t)Gn;
    if (KS > 0 && R <= NODE_FUSED_RANKS) {
        NodeGroupColsArgs c{};
        c.table = d_table, c.cells = cut.cells, c.gstart = cut.gstart;
        c.R = R, c.KS = KS, c.L = NVRX_TABLE_LEN(K, S), c.C = C, c.Gp = Gp;
        c.max_cell = max_cell, c.max_group_cells = max_group_cells;
        c.min_members = min_members, c.min_nodes = min_nodes, c.min_peers = min_peers;
        c.pairs = pairs, c.cols = cols;
        hipLaunchKernelGGL(k_node_group_cols, dim3((KS + ROBUST_TILE - 1) / ROBUST_TILE), dim3(NODE_THREADS), 0, st, c);
        HIP_TRY(hipGetLastError());
    } else if (KS > 0) {
        PaceGroupColsArgs c{};
        c.table = d_table, c.groups = cut.cells, c.R = R, c.KS = KS, c.L = NVRX_TABLE_LEN(K, S);
        c.max_group = max_cell, c.min_ranks = min_members, c.min_peers = 1;
        c.cols = pairs;
        pace_group_cols_launch(c, C, st);
        HIP_TRY(hipGetLastError());
        NodeGroupAcrossArgs x{};
        x.pairs = pairs, x.gstart = cut.gstart, x.C = C, x.KS = KS;
        x.max_group_cells = max_group_cells, x.min_nodes = min_nodes, x.min_peers = min_peers;
        x.cols = cols;
        if (max_group_cells <= NODE_GROUP_WAVE_CELLS)
            hipLaunchKernelGGL(k_node_group_across<64>, dim3((KS + ROBUST_THREADS / 64 - 1) / (ROBUST_THREADS / 64), Gp),
                               dim3(ROBUST_THREADS), 0, st, x);
        else
            hipLaunchKernelGGL(k_node_group_across<256>, dim3(KS, Gp), dim3(256), 0, st, x);
        HIP_TRY(hipGetLastError());
    }
    // block C: every node's gather over its cells, by the most (cell, column) pairs a part of a node can have
    NodeGroupRankArgs n{};
    n.pairs = pairs, n.cols = cols, n.nstart = cut.nstart, n.ncells = cut.ncells, n.cgroup = cut.cgroup;
    n.K = K, n.S = S, n.C = C, n.Gp = Gp, n.max_node_cells = max_node_cells;
    n.out = nodes;
    const long long widest = (long long)max_node_cells * (long long)(K > S ? K : S);  // at most 4096 * 65 536
    if (widest <= PACE_WAVE_COLS)
        hipLaunchKernelGGL((k_node_group_rank<64, 1>), dim3(Gn, 2), dim3(64), 0, st, n);
    else if (widest <= PACE_REG_COLS)
        hipLaunchKernelGGL((k_node_group_rank<256, 16>), dim3(Gn, 2), dim3(256), 0, st, n);
    else
        hipLaunchKernelGGL((k_node_group_rank<1024, 0>), dim3(Gn, 2), dim3(1024), 0, st, n);
    HIP_TRY(hipGetLastError());
    // block D: the grouped rank kernel with block B as its column records and the ranks' peer groups as its group ids
    PaceGroupRankArgs r{};
    r.table = d_table, r.cols = cols, r.groups = cut.rgroup;
    r.K = K, r.S = S, r.G = Gp, r.first_rank = first_rank;
    r.out = ranks;
    pace_rank_launch<true>(r, n_ranks, st);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_node_group_score(const float *d_table, int R, int K, int S, const int32_t *d_cells, int C, int Gp, int Gn, int max_cell,
                          int max_group_cells, int max_node_cells, int min_members, int min_nodes, int min_peers, int first_rank,
                          int n_ranks, void *d_out, void *stream) {
    const int rc = node_group_check(R, K, S, C, Gp, Gn, max_cell, max_group_cells, max_node_cells, min_members, min_nodes, min_peers,
                                    first_rank, n_ranks);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_table && d_cells, false)) return rc;
    return node_group_launch(d_table, R, K, S, d_cells, C, Gp, Gn, max_cell, max_group_cells, max_node_cells, min_members, min_nodes,
                             min_peers, first_rank, n_ranks, d_out, as_stream(stream));
}

int nvrx_report_node_group(nvrx_ctx *ctx, const nvrx_report_desc *desc, const int32_t *d_cells, int C, int Gp, int Gn, int max_cell,
                           int max_group_cells, int max_node_cells, int min_members, int min_nodes, int min_peers, int first_rank,
                           int n_ranks, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = node_group_check(desc->R, desc->K, desc->S, C, Gp, Gn, max_cell, max_group_cells, max_node_cells, min_members,
                                    min_nodes, min_peers, first_rank, n_ranks);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_cells != nullptr, true)) return rc;
    hipStream_t home = nullptr;
    const float *table = nullptr;
    if (const int rc = report_table(ctx, desc, &home, &table)) return rc;
    return node_group_launch(table, desc->R, desc->K, desc->S, d_cells, C, Gp, Gn, max_cell, max_group_cells, max_node_cells,
                             min_members, min_nodes, min_peers, first_rank, n_ranks, d_out, home);
}

}  // extern "C"
