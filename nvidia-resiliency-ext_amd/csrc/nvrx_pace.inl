// nvrx_pace.inl -- pace scores: the rank that is a little slower in nearly all of its kernels.  Part of the translation unit
// nvrx_straggler.hip (included at its end: it uses that file's key maps, DPP scans and sums, nvrx_tail.inl's histogram add
// and nvrx_robust.inl's selections).
//
// Every other score asks whether some row of a rank is MUCH slower than a reference.  A card held a clock step down, a
// throttling HBM stack or a marginal power rail loses 3-5 % on every kernel: the relative GPU score reads 0.95, the robust z
// (a weighted MEAN of per-kernel z) about 2, and no rule names the rank.  Here the reference point of a column (one kernel id
// or section id of the exchanged table) is the lower median `ctr` of the ranks that have the row, and a rank's PACE is the
// lower median, across its columns, of the quotients ctr / v: an order statistic across columns gains from all of them
// agreeing where a mean does not.  `spread` is the median absolute deviation of the quotients around the pace, and the counts
// say in how many columns the rank is slower / faster than the job's median.  The table is the one nvrx_score reads; nothing
// else is exchanged.
//
// k_pace_cols  the column geometry of k_robust_cols without the deviation pass: {ctr, n, above, below} per column.
//   <0>  R <= 64: 64 columns x R rows staged in LDS (65-word pitch), one column per wave at a time, rank r's value in lane
//        r, robust_wave_select; the two counts are two ballots against the selected key.
//   <T>  R > 64: one workgroup per column, robust_radix_select<T, false>; the counts take one more strided pass.
// k_pace_rank  grid (n_ranks, 2): part 0 the kernel columns, part 1 the section columns of one reported rank.  A median, then
//   a median of deviations, ACROSS the rank's columns; the row is contiguous, so a wave's loads are coalesced 256-byte runs
//   and the column records one 16-byte load per lane.
//   <64, 1>     up to 64 columns in either part: one wave, one column per lane, robust_wave_select twice.
//   <256, 16>   up to 4096: every lane computes its up to 16 quotients once and keeps their keys in registers (compile-time
//               indices); both selections are the three-pass MSB-first radix select (12 + 12 + 8 bits, 4096-bin LDS
//               histogram, radix_pick) fed from the registers: the table is read once.
//   <1024, 0>   beyond (the table allows 65 536): the passes re-read row and records from the L2, as k_row_quantile<1024>.
//   The quotients of a healthy rank all sit near 1.0 and share sign, exponent and leading mantissa bits: the first pass sends
//   nearly every key to one or two bins, the same-address LDS-atomic case tail_hist_add aggregates per wave.
//   Always exact, ties included; no data-dependent trip count, no sort, no scratch, no global atomics, no float atomics.

#include <type_traits>

namespace {

constexpr uint32_t PACE_MARK = 0xFFFFFFFFu;  // "no quotient here": f2key of no non-NaN float, and above every |x| bit pattern

struct PaceColsArgs {
    const float *table;  // [R][L]
    int R, KS, L;
    int min_ranks;
    uint4 *cols;  // [KS] {f32 ctr, u32 n, u32 above, u32 below}
};

__device__ __forceinline__ uint4 pace_col_record(uint32_t ckey, uint32_t n, uint32_t above, uint32_t below, int min_ranks) {
    const bool referenced = n != 0 && (int)n >= min_ranks;
    return make_uint4(referenced ? __float_as_uint(key2f(ckey)) : __float_as_uint(__builtin_nanf("")), n, above, below);
}

// THREADS == 0: the tiled kernel for R <= 64 (ROBUST_THREADS threads); else one workgroup of THREADS per column
template <int THREADS>
__global__ __launch_bounds__(THREADS ? THREADS : ROBUST_THREADS) void k_pace_cols(PaceColsArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (THREADS == 0) {
        __shared__ float s_tile[64 * ROBUST_PITCH];
        const int R = a.R;
        const int base = (int)blockIdx.x * ROBUST_TILE;
        {
            const int c = base + lane;
            for (int r = wave; r < R; r += ROBUST_THREADS / 64)
                s_tile[r * ROBUST_PITCH + lane] = c < a.KS ? a.table[(size_t)r * (size_t)a.L + c] : -1.0f;
        }
        __syncthreads();
        for (int ci = wave; ci < ROBUST_TILE; ci += ROBUST_THREADS / 64) {
            const int c = base + ci;
            if (c >= a.KS) break;  // wave-uniform
            const float v = lane < R ? s_tile[lane * ROBUST_PITCH + ci] : -1.0f;
            const bool present = v >= 0.0f;
            const uint32_t key = f2key(v);
            const unsigned long long mask = __ballot(present);
            const uint32_t n = (uint32_t)__popcll(mask);
            uint32_t ckey = 0, above = 0, below = 0;
            if (n != 0) {  // wave-uniform
                const int lc = robust_wave_select(key, present, mask, (n - 1u) >> 1, R, lane);
                ckey = (uint32_t)__builtin_amdgcn_readlane((int)key, lc);
                above = (uint32_t)__popcll(__ballot(present && key > ckey));
                below = (uint32_t)__popcll(__ballot(present && key < ckey));
            }
            if (lane == 0) a.cols[c] = pace_col_record(ckey, n, above, below, a.min_ranks);
        }
    } else {
        constexpr int WAVES = THREADS / 64;
        __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
        __shared__ uint32_t s_wave[WAVES];
        __shared__ uint32_t s_sel[2];
        __shared__ uint32_t s_cnt[2][WAVES];
        const int c = (int)blockIdx.x;
        const int R = a.R, L = a.L;
        const float *__restrict__ col = a.table + c;
        const float v0 = tid < R ? col[(size_t)tid * (size_t)L] : -1.0f;
        uint32_t cnt = 0;
        for (int r = tid; r < R; r += THREADS) {
            const float v = r == tid ? v0 : col[(size_t)r * (size_t)L];
            cnt += v >= 0.0f ? 1u : 0u;
        }
        cnt = wave_sum_u32(cnt);
        if (lane == 0) s_wave[wave] = cnt;
        __syncthreads();
        uint32_t n = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) n += s_wave[w];
        n = uni(n);
        if (n == 0) {  // block-uniform
            if (tid == 0) a.cols[c] = pace_col_record(0u, 0u, 0u, 0u, a.min_ranks);
            return;
        }
        // (s_wave is rewritten only behind the first pass' two barriers)
        const uint32_t ckey = robust_radix_select<THREADS, false>(col, R, L, v0, 0.0f, (n - 1u) >> 1, s_hist, s_wave, s_sel);
        uint32_t above = 0, below = 0;
        for (int r = tid; r < R; r += THREADS) {
            const float v = r == tid ? v0 : col[(size_t)r * (size_t)L];
            const uint32_t key = f2key(v);
            above += (v >= 0.0f && key > ckey) ? 1u : 0u;
            below += (v >= 0.0f && key < ckey) ? 1u : 0u;
        }
        above = wave_sum_u32(above);
        below = wave_sum_u32(below);
        if (lane == 0) s_cnt[0][wave] = above, s_cnt[1][wave] = below;
        __syncthreads();
        if (tid == 0) {
            above = below = 0;
            for (int w = 0; w < WAVES; w++) above += s_cnt[0][w], below += s_cnt[1][w];
            a.cols[c] = pace_col_record(ckey, n, above, below, a.min_ranks);
        }
    }
}

struct PaceRankArgs {
    const float *table;  // [R][L]
    const uint4 *cols;   // [KS]
    int K, S;
    int first_rank;
    int min_ranks;
    uint4 *out;  // [n_ranks][2] records of two 16-byte words
};

// k_pace_rank's GROUPED form (nvrx_pace_group.inl): the records of the rank's own group
struct PaceGroupRankArgs {
    const float *table;     // [R][L]
    const uint4 *cols;      // [G][KS]
    const int32_t *groups;  // group[R] | ...
    int K, S, G;
    int first_rank;
    uint4 *out;  // [n_ranks][2] records of two 16-byte words
};

// One column of a rank's part: what the counts and sums take from it, and the key of its quotient.
struct PaceCol {
    uint32_t qkey;  // f2key of (float)((double)ctr / (double)v); PACE_MARK where not eligible or the quotient is NaN
    bool eligible, slower, faster;
    double quot;  // the f64 quotient (read only where qkey is not the marker)
};

// row and recs point at the part's first column; i >= ncols reads nothing.  GROUPED: the records are those of the rank's group,
// whose centre is a number exactly where the pair is referenced, and min_ranks says whether the rank has a group at all (0 / 1).
// NODE (nvrx_node.inl): the "row" is a node's stretch of pair records, its value the first of a record's four words -- NaN, so
// not present, where the pair is not referenced --, and the centre is a number exactly where the column is referenced.
template <bool GROUPED = false, bool NODE = false>
__device__ __forceinline__ PaceCol pace_column(const float *__restrict__ row, const uint4 *__restrict__ recs, int i, int ncols,
                                               int min_ranks) {
    PaceCol o;
    o.qkey = PACE_MARK, o.eligible = o.slower = o.faster = false, o.quot = 0.0;
    if (i < ncols) {
        const float v = row[NODE ? 4 * i : i];
        const uint4 rec = recs[i];
        const float ctr = __uint_as_float(rec.x);
        if constexpr (GROUPED || NODE)
            o.eligible = v >= 0.0f && min_ranks != 0 && ctr == ctr;
        else
            o.eligible = v >= 0.0f && rec.y != 0u && (int)rec.y >= min_ranks;
        const uint32_t kv = f2key(v), kc = f2key(ctr);
        o.slower = o.eligible && kv > kc;
        o.faster = o.eligible && kv < kc;
        o.quot = (double)ctr / (double)v;
        const float q = (float)o.quot;
        o.qkey = (o.eligible && q == q) ? f2key(q) : PACE_MARK;
    }
    return o;
}

// the deviation key of a quotient key: the bit pattern of |q - pace| (a NaN -- inf - inf -- orders above +inf)
__device__ __forceinline__ uint32_t pace_dev_key(uint32_t qkey, float pace) {
    return qkey == PACE_MARK ? PACE_MARK : robust_dev_bits(key2f(qkey), pace);
}

// Three-pass radix select over keys that key_at hands out: NREG > 0, key_at(j) is the lane's j-th key (registers, j a
// compile-time index); NREG == 0, key_at(i) is the key of column i < ncols (recomputed from the L2).  PACE_MARK never enters
// a histogram.  Every thread of the workgroup calls it with the same k (barriers inside).
template <int THREADS, int NREG, typename KeyAt>
__device__ __forceinline__ uint32_t pace_radix_select(KeyAt key_at, int ncols, uint32_t k, uint32_t *s_hist, uint32_t *s_wave,
                                                      uint32_t *s_sel) {
    constexpr int PER = TAIL_BINS / THREADS;
    const int tid = threadIdx.x;
    uint32_t prefix = 0;
#pragma unroll 1
    for (int pass = 0; pass < 3; pass++) {
        const int shift = pass == 0 ? 20 : pass == 1 ? 8 : 0;
        const int up = pass == 0 ? 32 : pass == 1 ? 20 : 8;
        const uint32_t bmask = pass == 2 ? 0xFFu : 0xFFFu;
#pragma unroll
        for (int j = 0; j < PER; j += 4) reinterpret_cast<uint4 *>(s_hist)[(tid * PER + j) >> 2] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        if constexpr (NREG > 0) {
#pragma unroll
            for (int j = 0; j < NREG; j++) {
                const uint32_t key = key_at(j);
                const bool on = key != PACE_MARK && (up == 32 || (key >> up) == prefix);
                tail_hist_add(s_hist, (key >> shift) & bmask, on);
            }
        } else {
            for (int i = tid; i < ncols; i += THREADS) {
                const uint32_t key = key_at(i);
                const bool on = key != PACE_MARK && (up == 32 || (key >> up) == prefix);
                tail_hist_add(s_hist, (key >> shift) & bmask, on);
            }
        }
        __syncthreads();
        const uint32_t bin = radix_pick<THREADS>(s_hist, s_wave, s_sel, k);
        prefix = pass == 2 ? ((prefix << 8) | bin) : ((prefix << 12) | bin);
    }
    return prefix;
}

// lane 0 / thread 0: the 32-byte record as two 16-byte stores
__device__ __forceinline__ void pace_store(uint4 *dst, float pace, float spread, uint32_t columns, uint32_t slower,
                                           uint32_t faster, double total, double slow, double excess) {
    dst[0] = make_uint4(__float_as_uint(pace), __float_as_uint(spread), columns, slower);
    dst[1] = make_uint4(faster, __float_as_uint((float)total), __float_as_uint((float)slow), __float_as_uint((float)excess));
}

// THREADS 64 (NREG 1): one wave, one column per lane; 256 with NREG 16: keys in registers; 1024 with NREG 0: re-reading.
// GROUPED (a compile-time flag: the job-wide instantiations are what they were): the records at cols + group[r] * (K+S), a
// column eligible iff the rank is present and its group's pair is referenced.
// NODE (likewise; nvrx_node.inl): `table` is the [G][K+S] pair records, a row of 4 (K+S) words per node; no weights, so the
// three sums stay +0.0 in both parts.
template <int THREADS, int NREG, bool GROUPED = false, bool NODE = false>
__global__ __launch_bounds__(THREADS) void k_pace_rank(std::conditional_t<GROUPED, PaceGroupRankArgs, PaceRankArgs> a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, S = a.S, KS = K + S;
    const int L = NODE ? 4 * KS : NVRX_TABLE_LEN(K, S);
    const int part = (int)blockIdx.y;
    const int ncols = part ? S : K;
    const int base = part ? K : 0;
    const float *__restrict__ row = a.table + (size_t)(a.first_rank + (int)blockIdx.x) * (size_t)L;
    const float *__restrict__ wrow = row + 2 * (size_t)KS;  // the weights NUM*AVG of the kernel columns (part 0 only)
    const uint4 *__restrict__ recs = a.cols + base;
    int min_ranks;  // GROUPED: 1 where the rank has a group, else 0 (no eligible column)
    if constexpr (GROUPED) {
        const int g = a.groups[a.first_rank + (int)blockIdx.x];
        min_ranks = (uint32_t)g < (uint32_t)a.G ? 1 : 0;  // block-uniform
        recs += (size_t)(min_ranks ? g : 0) * (size_t)KS;
    } else {
        min_ranks = a.min_ranks;
    }
    uint4 *__restrict__ dst = a.out + ((size_t)blockIdx.x * 2 + (size_t)part) * 2;
    const float NaN = __builtin_nanf("");
    row += NODE ? 4 * base : base;

    if constexpr (THREADS == 64) {
        const PaceCol col = pace_column<GROUPED, NODE>(row, recs, lane, ncols, min_ranks);
        const bool has_q = col.qkey != PACE_MARK;
        const double w = (!NODE && part == 0 && col.eligible) ? (double)wrow[lane] : 0.0;
        const double total = wave_sum_f64(w);
        const double slow = wave_sum_f64(col.slower ? w : 0.0);
        const double excess = wave_sum_f64((!NODE && part == 0 && has_q) ? w * (1.0 - col.quot) : 0.0);
        const uint32_t columns = (uint32_t)__popcll(__ballot(col.eligible));
        const uint32_t slower = (uint32_t)__popcll(__ballot(col.slower));
        const uint32_t faster = (uint32_t)__popcll(__ballot(col.faster));
        const unsigned long long mask = __ballot(has_q);
        const uint32_t m = (uint32_t)__popcll(mask);
        float pace = NaN, spread = NaN;
        if (m != 0) {  // wave-uniform
            const uint32_t target = (m - 1u) >> 1;
            const int lp = robust_wave_select(col.qkey, has_q, mask, target, ncols, lane);
            pace = key2f((uint32_t)__builtin_amdgcn_readlane((int)col.qkey, lp));
            const uint32_t d = pace_dev_key(col.qkey, pace);
            const int ls = robust_wave_select(d, has_q, mask, target, ncols, lane);
            spread = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)d, ls));
        }
        if (lane == 0) pace_store(dst, pace, spread, columns, slower, faster, total, slow, excess);
    } else {
        constexpr int WAVES = THREADS / 64;
        constexpr int NKEYS = NREG ? NREG : 1;
        __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
        __shared__ uint32_t s_wave[WAVES];
        __shared__ uint32_t s_sel[2];
        __shared__ double s_sum[3][WAVES];
        __shared__ uint32_t s_cnt[4][WAVES];
        uint32_t keys[NKEYS];
        double total = 0.0, slow = 0.0, excess = 0.0;
        uint32_t columns = 0, slower = 0, faster = 0, m = 0;
        auto take = [&](const PaceCol &col, int i) {
            const bool has_q = col.qkey != PACE_MARK;
            const double w = (!NODE && part == 0 && col.eligible) ? (double)wrow[i] : 0.0;
            total += w;
            slow += col.slower ? w : 0.0;
            excess += (!NODE && part == 0 && has_q) ? w * (1.0 - col.quot) : 0.0;  // (part 1 keeps +0.0: no 0 * inf)
            columns += col.eligible ? 1u : 0u;
            slower += col.slower ? 1u : 0u;
            faster += col.faster ? 1u : 0u;
            m += has_q ? 1u : 0u;
        };
        if constexpr (NREG > 0) {
#pragma unroll
            for (int j = 0; j < NREG; j++) {
                const int i = tid + j * THREADS;
                const PaceCol col = pace_column<GROUPED, NODE>(row, recs, i, ncols, min_ranks);
                keys[j] = col.qkey;
                take(col, i);
            }
        } else {
            keys[0] = PACE_MARK;
            for (int i = tid; i < ncols; i += THREADS) take(pace_column<GROUPED, NODE>(row, recs, i, ncols, min_ranks), i);
        }
        total = wave_sum_f64(total);
        slow = wave_sum_f64(slow);
        excess = wave_sum_f64(excess);
        columns = wave_sum_u32(columns);
        slower = wave_sum_u32(slower);
        faster = wave_sum_u32(faster);
        m = wave_sum_u32(m);
        if (lane == 0) {
            s_sum[0][wave] = total, s_sum[1][wave] = slow, s_sum[2][wave] = excess;
            s_cnt[0][wave] = columns, s_cnt[1][wave] = slower, s_cnt[2][wave] = faster, s_cnt[3][wave] = m;
        }
        __syncthreads();
        m = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) m += s_cnt[3][w];
        m = uni(m);
        float pace = NaN, spread = NaN;
        if (m != 0) {  // block-uniform
            const uint32_t target = (m - 1u) >> 1;
            const int mr = min_ranks;
            if constexpr (NREG > 0) {
                pace = key2f(pace_radix_select<THREADS, NREG>([&](int j) { return keys[j]; }, ncols, target, s_hist, s_wave, s_sel));
                spread = __uint_as_float(pace_radix_select<THREADS, NREG>([&](int j) { return pace_dev_key(keys[j], pace); }, ncols,
                                                                          target, s_hist, s_wave, s_sel));
            } else {
                pace = key2f(pace_radix_select<THREADS, 0>([&](int i) { return pace_column<GROUPED, NODE>(row, recs, i, ncols, mr).qkey; }, ncols,
                                                           target, s_hist, s_wave, s_sel));
                spread = __uint_as_float(pace_radix_select<THREADS, 0>(
                    [&](int i) { return pace_dev_key(pace_column<GROUPED, NODE>(row, recs, i, ncols, mr).qkey, pace); }, ncols, target, s_hist,
                    s_wave, s_sel));
            }
        }
        if (tid == 0) {
            total = slow = excess = 0.0;
            columns = slower = faster = 0;
            for (int w = 0; w < WAVES; w++) {
                total += s_sum[0][w], slow += s_sum[1][w], excess += s_sum[2][w];
                columns += s_cnt[0][w], slower += s_cnt[1][w], faster += s_cnt[2][w];
            }
            pace_store(dst, pace, spread, columns, slower, faster, total, slow, excess);
        }
    }
}

constexpr int PACE_WAVE_COLS = 64;        // columns of a part one wave takes
constexpr int PACE_REG_COLS = 256 * 16;  // ... and 256 threads keep in registers

// The variant of k_pace_rank by the wider of a rank's two parts, one workgroup per (row, part).  GROUPED and NODE as the kernel
// has them; Args is the kernel's argument struct.
template <bool GROUPED = false, bool NODE = false, class Args>
void pace_rank_launch(const Args &a, int rows, hipStream_t st) {
    const int widest = a.K > a.S ? a.K : a.S;
    if (widest <= PACE_WAVE_COLS)
        hipLaunchKernelGGL((k_pace_rank<64, 1, GROUPED, NODE>), dim3(rows, 2), dim3(64), 0, st, a);
    else if (widest <= PACE_REG_COLS)
        hipLaunchKernelGGL((k_pace_rank<256, 16, GROUPED, NODE>), dim3(rows, 2), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_pace_rank<1024, 0, GROUPED, NODE>), dim3(rows, 2), dim3(1024), 0, st, a);
}

int pace_launch(const float *d_table, int R, int K, int S, int first_rank, int n_ranks, int min_ranks, void *d_out,
                hipStream_t st) {
    const int KS = K + S;
    if (KS > 0) {
        PaceColsArgs c{};
        c.table = d_table, c.R = R, c.KS = KS, c.L = NVRX_TABLE_LEN(K, S);
        c.min_ranks = min_ranks;
        c.cols = static_cast<uint4 *>(d_out);
        cols_launch(k_pace_cols<0>, k_pace_cols<256>, k_pace_cols<1024>, R, KS, 1, c, st);
        HIP_TRY(hipGetLastError());
    }
    PaceRankArgs a{};
    a.table = d_table, a.cols = static_cast<const uint4 *>(d_out);
    a.K = K, a.S = S, a.first_rank = first_rank, a.min_ranks = min_ranks;
    a.out = static_cast<uint4 *>(d_out) + (size_t)KS;
    pace_rank_launch(a, n_ranks, st);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_pace_score(const float *d_table, int R, int K, int S, int first_rank, int n_ranks, int min_ranks, void *d_out,
                    void *stream) {
    const int rc = table_min_ranks_check(R, K, S, first_rank, n_ranks, min_ranks);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_table != nullptr, false)) return rc;
    return pace_launch(d_table, R, K, S, first_rank, n_ranks, min_ranks, d_out, as_stream(stream));
}

int nvrx_report_pace(nvrx_ctx *ctx, const nvrx_report_desc *desc, int first_rank, int n_ranks, int min_ranks, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = table_min_ranks_check(desc->R, desc->K, desc->S, first_rank, n_ranks, min_ranks);
    if (rc) return rc;
    if (const int rc = out_check(d_out, true, true)) return rc;
    hipStream_t home = nullptr;
    const float *table = nullptr;
    if (const int rc = report_table(ctx, desc, &home, &table)) return rc;
    return pace_launch(table, desc->R, desc->K, desc->S, first_rank, n_ranks, min_ranks, d_out, home);
}

}  // extern "C"
