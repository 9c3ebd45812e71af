// nvrx_robust_group.inl -- robust scores per peer group: every rank against the median and spread of the ranks doing the SAME
// work.  Part of the translation unit nvrx_straggler.hip (included at its end, behind nvrx_peer.inl, nvrx_robust.inl and
// nvrx_pace_group.inl: it uses the first's clamp, the second's deviation bits and rank kernel, nvrx_pace.inl's marker and radix
// select and the last one's argument checks).
//
// nvrx_robust.inl's reference point of a column is the lower median of the whole job, its spread the MAD around it.  In a job
// of pipeline stages, tensor-parallel or expert groups the job's median lies in one of the groups and the MAD is that group's:
// every healthy rank of a slower stage gets a huge z.  Here the caller says which ranks are peers (nvrx_peer_score's array,
// unchanged) and a column's record {ctr, mad, scale, n} is taken per (group, column) over the group's members that have the
// row.  The table is the one nvrx_score reads; nothing else is exchanged.
//
// k_robust_group_packed<SLOT>  every group has at most 64 members.  SLOT is the smallest power of two >= max_group (at least
//   2): a wave holds 64 / SLOT groups, each group owns SLOT consecutive lanes (a tensor-parallel group of 4 uses 4 lanes, and
//   16 of them share a wave; one group per wave would idle 60 lanes and launch 16 times the workgroups).  Grid
//   (ceil((K+S)/64), ceil(G / (64/SLOT))), 256 threads.  A workgroup stages 64 columns x 64 slot rows in LDS (65-word pitch):
//   tile row l is member l % SLOT of group pack * (64/SLOT) + l / SLOT, read through members[] as one coalesced 256-byte run
//   (lane = column); -1.0 (absent) where the slot is beyond the group's size, the group beyond G or the member no rank of the
//   table.  After one barrier each wave takes columns in turn, slot row l in lane l.  A lane's position in its group's sorted
//   column is counted over the SLOT keys of its own segment only, read from lane ^ j, j = 1 .. SLOT-1 (an aligned power-of-two
//   segment is closed under xor): DPP quad permutes and row mirrors where SLOT <= 16, ds_bpermute above.  Ties: the lower
//   lane first, as robust_wave_select.  n, the hit lane and the broadcast of the selected key come from the segment's stretch
//   of the ballot masks.  The selection runs on f2key(v), then on the bit patterns of |v - ctr|; the first lane of a segment
//   writes the group's 16-byte record.  No atomics, no scratch, no data-dependent trip count.  SLOT == 64 is one group per
//   wave: the same code.
// k_robust_group_cols<T>  larger groups: grid (K+S, G), one workgroup of T per pair; pace_radix_select<T, 0> (12 + 12 + 8 bits)
//   twice over keys re-read from the L2 through members[] (PACE_MARK for an absent or skipped member).  Smaller groups of the
//   same launch take the same path.
// k_robust_rank<true>  nvrx_robust.inl's rank kernel reading the records of the rank's own group.
//
// d_groups is data, not an argument the host checks can see: start values are clamped to [0, R], a stretch to max_group, a
// member outside [0, R) is skipped, a group id outside [0, G) leaves the rank unrated (NaN).  Nothing in it can move a load or
// a store outside the table, the array or d_out.

namespace {

struct RobustGroupColsArgs {
    const float *table;     // [R][L]
    const int32_t *groups;  // group[R] | members[R] | start[G+1]
    int R, KS, L, G;
    int max_group;  // in 1..R
    int min_ranks, min_peers;
    float floor_rel;
    uint4 *cols;  // [G][KS] {f32 ctr, f32 mad, f32 scale, u32 n}
};

// the pair is referenced iff n >= max(min_peers, min(min_ranks, size)) (pace_group_record's rule; min_peers >= 1, so a pair
// nobody has never is); the scale is robust_record's
__device__ __forceinline__ uint4 robust_group_record(float ctr, float mad, uint32_t n, int size, const RobustGroupColsArgs &a) {
    const int clamped = a.min_ranks < size ? a.min_ranks : size;
    const int need = a.min_peers > clamped ? a.min_peers : clamped;
    if ((int)n < need) {
        const uint32_t nan = __float_as_uint(__builtin_nanf(""));
        return make_uint4(nan, nan, nan, n);
    }
    const float scale = fmaxf(1.4826f * mad, a.floor_rel * ctr);
    return make_uint4(__float_as_uint(ctr), __float_as_uint(mad), __float_as_uint(scale), n);
}

// the members of group g as the kernels take them: start values clamped to [0, R], the stretch cut to `most`
__device__ __forceinline__ void robust_group_stretch(const int32_t *__restrict__ start, int g, int R, int most, int &s0, int &size) {
    s0 = peer_clamp(start[g], R);
    const int s1 = peer_clamp(start[g + 1], R);
    size = s1 > s0 ? s1 - s0 : 0;
    size = size < most ? size : most;  // members[s0 .. s0 + size) lie inside the array: s0 + size <= s1 <= R
}

constexpr int DPP_QUAD_3210 = 0x1b, DPP_ROW_MIRROR = 0x140, DPP_ROW_HALF_MIRROR = 0x141;

// the value of lane ^ Q inside a quad
template <int Q>
__device__ __forceinline__ uint32_t quad_xor(uint32_t v) {
    if constexpr (Q == 0) return v;
    else return dpp0<Q == 1 ? DPP_QUAD_1032 : Q == 2 ? DPP_QUAD_2301 : DPP_QUAD_3210>(v);
}

// the value of lane ^ J, J < 16, on DPP row operations: a half mirror is ^7, a row mirror ^15, a quad permute ^0..3
template <int J>
__device__ __forceinline__ uint32_t row_xor(uint32_t v) {
    constexpr int H = J & 12, Q = J & 3;
    if constexpr (H == 0) return quad_xor<Q>(v);
    else if constexpr (H == 4) return quad_xor<Q ^ 3>(dpp0<DPP_ROW_HALF_MIRROR>(v));
    else if constexpr (H == 8) return quad_xor<Q>(dpp0<DPP_ROW_HALF_MIRROR>(dpp0<DPP_ROW_MIRROR>(v)));
    else return quad_xor<Q ^ 3>(dpp0<DPP_ROW_MIRROR>(v));
}

// whether the key kj of lane `lane ^ j` orders before this lane's (ties: the lower lane first), given that lane is present
template <typename Seg>
__device__ __forceinline__ uint32_t robust_seg_before(uint32_t kj, uint32_t key, Seg seg, int other, int lane, int slot_mask) {
    const bool pj = (seg >> (other & slot_mask)) & 1u;
    return (pj && (kj < key || (kj == key && other < lane))) ? 1u : 0u;
}

template <int SLOT, int J, typename Seg>
__device__ __forceinline__ uint32_t robust_seg_position_dpp(uint32_t key, Seg seg, int lane) {
    if constexpr (J >= SLOT) return 0u;
    else
        return robust_seg_before(row_xor<J>(key), key, seg, lane ^ J, lane, SLOT - 1) +
               robust_seg_position_dpp<SLOT, J + 1>(key, seg, lane);
}

// the position of this lane's key among the present keys of its SLOT-lane segment: SLOT - 1 cross-lane reads
template <int SLOT, typename Seg>
__device__ __forceinline__ uint32_t robust_seg_position(uint32_t key, Seg seg, int lane) {
    if constexpr (SLOT <= 16) {
        return robust_seg_position_dpp<SLOT, 1>(key, seg, lane);
    } else {
        // eight reads in flight at a time; the outer loop stays a loop, so that the SLOT addresses are not kept in registers
        // across the columns (j = 0 is the lane itself and counts nothing)
        uint32_t pos = 0;
#pragma unroll 1
        for (int j0 = 0; j0 < SLOT; j0 += 8) {
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int other = lane ^ (j0 + u);
                const uint32_t kj = (uint32_t)__builtin_amdgcn_ds_bpermute(other << 2, (int)key);
                pos += robust_seg_before(kj, key, seg, other, lane, SLOT - 1);
            }
        }
        return pos;
    }
}

// the key at position `target` among the present keys of this lane's segment, in every lane of the segment (`fallback` where
// the segment has no present key).  Every lane of the wave calls it.
template <int SLOT, typename Seg>
__device__ __forceinline__ uint32_t robust_seg_select(uint32_t key, bool present, Seg seg, uint32_t target, int lane,
                                                      uint32_t fallback) {
    const int base = lane & ~(SLOT - 1);
    const uint32_t pos = robust_seg_position<SLOT>(key, seg, lane);
    const unsigned long long hit = __ballot(present && pos == target);
    const Seg hseg = SLOT == 64 ? (Seg)hit : (Seg)((hit >> base) & ((1ull << (SLOT & 63)) - 1ull));
    const int from = hseg ? base + (SLOT == 64 ? __ffsll((long long)hseg) : __ffs((int)hseg)) - 1 : lane;
    const uint32_t sel = (uint32_t)__builtin_amdgcn_ds_bpermute(from << 2, (int)key);
    return hseg ? sel : fallback;
}

template <int SLOT>
__global__ __launch_bounds__(ROBUST_THREADS) void k_robust_group_packed(RobustGroupColsArgs a) {
    static_assert(SLOT >= 2 && SLOT <= 64 && (SLOT & (SLOT - 1)) == 0, "a power of two that divides a wave");
    constexpr int GPW = 64 / SLOT;  // groups per wave (and per workgroup's tile)
    using Seg = std::conditional_t<SLOT == 64, unsigned long long, uint32_t>;
    __shared__ float s_tile[64 * ROBUST_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R, KS = a.KS, G = a.G;
    const int32_t *__restrict__ members = a.groups + R;
    const int32_t *__restrict__ start = a.groups + 2 * (size_t)R;
    const int most = a.max_group < SLOT ? a.max_group : SLOT;
    const int g0 = (int)blockIdx.y * GPW;
    const int base = (int)blockIdx.x * ROBUST_TILE;
    {
        const int c = base + lane;
        for (int l = wave; l < 64; l += ROBUST_THREADS / 64) {  // wave-uniform: the row's group and member
            const int g = g0 + l / SLOT, i = l % SLOT;
            float v = -1.0f;
            if (g < G) {
                int s0, size;
                robust_group_stretch(start, g, R, most, s0, size);
                if (i < size) {
                    const int m = members[s0 + i];
                    if ((uint32_t)m < (uint32_t)R && c < KS) v = a.table[(size_t)m * (size_t)a.L + (size_t)c];
                }
            }
            s_tile[l * ROBUST_PITCH + lane] = v;
        }
    }
    // this lane's group, its size (the record's rule needs it) and whether the lane writes the group's records
    const int g = g0 + lane / SLOT;
    int size = 0;
    if (g < G) {
        int s0;
        robust_group_stretch(start, g, R, most, s0, size);
    }
    const bool writer = (lane & (SLOT - 1)) == 0 && g < G;
    uint4 *__restrict__ cols = a.cols + (size_t)(g < G ? g : 0) * (size_t)KS;
    const int seg_base = lane & ~(SLOT - 1);
    __syncthreads();
    for (int ci = wave; ci < ROBUST_TILE; ci += ROBUST_THREADS / 64) {
        const int c = base + ci;
        if (c >= KS) break;  // wave-uniform
        const float v = s_tile[lane * ROBUST_PITCH + ci];
        const bool present = v >= 0.0f;
        const unsigned long long mask = __ballot(present);
        const Seg seg = SLOT == 64 ? (Seg)mask : (Seg)((mask >> seg_base) & ((1ull << (SLOT & 63)) - 1ull));
        const uint32_t n = SLOT == 64 ? (uint32_t)__popcll(seg) : (uint32_t)__popc((uint32_t)seg);
        const uint32_t target = (n - 1u) >> 1;  // (n == 0: no lane is present, nothing hits)
        const float ctr = key2f(robust_seg_select<SLOT>(f2key(v), present, seg, target, lane, f2key(0.0f)));
        const uint32_t d = robust_dev_bits(v, ctr);
        const float mad = __uint_as_float(robust_seg_select<SLOT>(d, present, seg, target, lane, 0u));
        if (writer) cols[c] = robust_group_record(ctr, mad, n, size, a);
    }
}

// one workgroup of THREADS per (column, group) pair
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_robust_group_cols(RobustGroupColsArgs a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
    __shared__ uint32_t s_wave[WAVES];
    __shared__ uint32_t s_sel[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R, L = a.L;
    const int c = (int)blockIdx.x, g = (int)blockIdx.y;  // < KS, < G: the grid's extents
    int s0, size;
    robust_group_stretch(a.groups + 2 * (size_t)R, g, R, a.max_group, s0, size);
    const int32_t *__restrict__ members = a.groups + R + s0;
    const float *__restrict__ col = a.table + c;
    uint4 *__restrict__ rec = a.cols + (size_t)g * (size_t)a.KS + c;
    // the value of member i < size; absent where the member has no such row or is no rank of the table
    auto value_at = [&](int i) -> float {
        const int m = members[i];
        return (uint32_t)m < (uint32_t)R ? col[(size_t)m * (size_t)L] : -1.0f;
    };
    auto key_at = [&](int i) -> uint32_t {
        const float v = value_at(i);
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
        if (tid == 0) *rec = robust_group_record(0.0f, 0.0f, 0u, size, a);
        return;
    }
    // (s_wave is rewritten only behind the first pass' two barriers)
    const uint32_t target = (n - 1u) >> 1;
    const float ctr = key2f(pace_radix_select<THREADS, 0>(key_at, size, target, s_hist, s_wave, s_sel));
    auto dev_at = [&](int i) -> uint32_t {  // (a deviation's sign bit is clear: never the marker)
        const float v = value_at(i);
        return v >= 0.0f ? robust_dev_bits(v, ctr) : PACE_MARK;
    };
    const float mad = __uint_as_float(pace_radix_select<THREADS, 0>(dev_at, size, target, s_hist, s_wave, s_sel));
    if (tid == 0) *rec = robust_group_record(ctr, mad, n, size, a);
}

// argument checks shared by both entry points: nvrx_pace_group_score's in its order, then nvrx_robust_score's of floor_rel;
// nothing here touches a device
int robust_group_check(int R, int K, int S, int G, int max_group, int first_rank, int n_ranks, int min_ranks, int min_peers,
                       float floor_rel) {
    const int rc = pace_group_check(R, K, S, G, max_group, first_rank, n_ranks, min_ranks, min_peers);
    if (rc) return rc;
    if (!(floor_rel == floor_rel) || floor_rel - floor_rel != 0.0f) return fail(NVRX_ERR_INVALID, "floor_rel is not finite");
    if (floor_rel < 0.0f || floor_rel > 1.0f) return fail(NVRX_ERR_RANGE, "floor_rel=%g outside [0,1]", (double)floor_rel);
    return NVRX_OK;
}

template <int SLOT>
void robust_group_packed_launch(const RobustGroupColsArgs &c, hipStream_t st) {
    constexpr int GPW = 64 / SLOT;
    hipLaunchKernelGGL(k_robust_group_packed<SLOT>, dim3((c.KS + ROBUST_TILE - 1) / ROBUST_TILE, (c.G + GPW - 1) / GPW),
                       dim3(ROBUST_THREADS), 0, st, c);
}

// one variant per launch, by the largest group's size: packed up to 64 (SLOT the smallest power of two that holds it), one
// workgroup of 256 per pair up to 1024, of 1024 beyond (cols_launch's thresholds)
void robust_group_cols_launch(const RobustGroupColsArgs &c, hipStream_t st) {
    const int m = c.max_group;
    if (m <= 2) robust_group_packed_launch<2>(c, st);
    else if (m <= 4) robust_group_packed_launch<4>(c, st);
    else if (m <= 8) robust_group_packed_launch<8>(c, st);
    else if (m <= 16) robust_group_packed_launch<16>(c, st);
    else if (m <= 32) robust_group_packed_launch<32>(c, st);
    else if (m <= 64) robust_group_packed_launch<64>(c, st);
    else if (m <= 1024) hipLaunchKernelGGL(k_robust_group_cols<256>, dim3(c.KS, c.G), dim3(256), 0, st, c);
    else hipLaunchKernelGGL(k_robust_group_cols<1024>, dim3(c.KS, c.G), dim3(1024), 0, st, c);
}

int robust_group_launch(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int max_group, int first_rank,
                        int n_ranks, int min_ranks, int min_peers, float floor_rel, void *d_out, hipStream_t st) {
    const int KS = K + S;
    if (KS > 0) {
        RobustGroupColsArgs c{};
        c.table = d_table, c.groups = d_groups, c.R = R, c.KS = KS, c.L = NVRX_TABLE_LEN(K, S), c.G = G;
        c.max_group = max_group, c.min_ranks = min_ranks, c.min_peers = min_peers, c.floor_rel = floor_rel;
        c.cols = static_cast<uint4 *>(d_out);
        robust_group_cols_launch(c, st);
        HIP_TRY(hipGetLastError());
    }
    RobustGroupRankArgs a{};
    a.table = d_table, a.cols = static_cast<const uint4 *>(d_out), a.groups = d_groups;
    a.K = K, a.S = S, a.G = G, a.first_rank = first_rank;
    a.out = static_cast<float *>(d_out) + 4 * (size_t)G * (size_t)KS;
    hipLaunchKernelGGL(k_robust_rank<true>, dim3(n_ranks), dim3(ROBUST_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_robust_group_score(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int max_group,
                            int first_rank, int n_ranks, int min_ranks, int min_peers, float floor_rel, void *d_out,
                            void *stream) {
    const int rc = robust_group_check(R, K, S, G, max_group, first_rank, n_ranks, min_ranks, min_peers, floor_rel);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_table && d_groups, false)) return rc;
    return robust_group_launch(d_table, R, K, S, d_groups, G, max_group, first_rank, n_ranks, min_ranks, min_peers, floor_rel,
                               d_out, as_stream(stream));
}

int nvrx_report_robust_group(nvrx_ctx *ctx, const nvrx_report_desc *desc, const int32_t *d_groups, int G, int max_group,
                             int first_rank, int n_ranks, int min_ranks, int min_peers, float floor_rel, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = robust_group_check(desc->R, desc->K, desc->S, G, max_group, first_rank, n_ranks, min_ranks, min_peers, floor_rel);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_groups != nullptr, true)) return rc;
    hipStream_t home = nullptr;
    const float *table = nullptr;
    if (const int rc = report_table(ctx, desc, &home, &table)) return rc;
    return robust_group_launch(table, desc->R, desc->K, desc->S, d_groups, G, max_group, first_rank, n_ranks, min_ranks, min_peers,
                               floor_rel, d_out, home);
}

}  // extern "C"
