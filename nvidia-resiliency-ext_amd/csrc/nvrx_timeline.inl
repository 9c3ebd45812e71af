// nvrx_timeline.inl -- timeline scores: WHEN, inside a report's window, a whole GPU ran slow.  Part of the translation unit
// nvrx_straggler.hip (included behind nvrx_profile.inl, after nvrx_pace.inl: it uses that file's register-fed radix select,
// nvrx_robust.inl's wave select, nvrx_rowfam.inl's host side, and the main file's key maps and DPP reductions).
//
// Every other score looks across a rank's rows (their medians: relative, robust, peer, pace, node scores) or along one row's
// time axis (tail, onset, period, episode, ramp, stall, tail profile) -- never both.  A card that drops a clock step for a
// tenth of the window is 4 % slower in EVERY kernel on the same samples: no median moves, and no single row's stretch stands
// out of its noise.  The evidence is that the rows agree.  Here every ring row is cut into B buckets of its own samples, each
// bucket's mean is divided by the row's typical bucket, and per rank and bucket the lower median ACROSS the rows (`level`)
// and the number of rows above 1 + effect (`slower`) are taken: the pace scores' rule, once per bucket (definition:
// include/nvrx_straggler.h).  A rank exchanges 2 x 3 x B floats.
//
// k_row_timeline<THREADS>: one workgroup per ring row, the row read from device memory ONCE.
//   buckets   sample i of n (time order) lies in bucket i * B / n; wave w owns buckets [ceil(w B / W), ceil((w + 1) B / W)),
//             a contiguous span of the time axis.  A bucket is walked 64 samples a step, sample lo + 64 * step + lane, every
//             lane keeping an f64 partial sum that wave_sum_f64 closes: wave, step and lane follow from n and the TIME index
//             alone, so a rotated ring (un-rotated through `starts`, as k_row_stall does) gives the same bits.
//   end       ONE barrier; wave 0 then holds bucket b's mean in lane b (B <= 64).  The lower median of the B means is rank
//             counting in registers (every lane's key broadcast by readlane, smaller keys counted, ties by lane), the ratios
//             one f64 division per lane; lane b writes x_b.  No LDS histogram, no scratch memory, no global atomic.
// k_timeline_rank<THREADS, NREG>: one workgroup per (logical rank, bucket); the plane [K+S] of that bucket is contiguous.
//   Per family (kernel columns, then section columns) the keys of the slots that took part are taken once -- <64, 1> one per
//   lane, <256, 16> sixteen per lane in registers, <1024, 0> re-read from the L2 in every pass -- and one exact selection (the
//   wave select, else pace_radix_select) gives the level; the two counts ride on the same keys.
// k_timeline_score: one wave per (reported rank, family), lane b holds bucket b.  The reference is one coalesced walk over
//   the ranks' blocks; the slow flags are ONE ballot, and the longest run, its first bucket and the number of slow buckets
//   are scalar bit work on that mask; the run's mean is wave_sum_f64 under the run's mask.

namespace {

constexpr int TIMELINE_MIN_B = NVRX_TIMELINE_MIN_BUCKETS, TIMELINE_MAX_B = NVRX_TIMELINE_MAX_BUCKETS;
constexpr int TIMELINE_FIELDS = 3;  // per (rank, family): rows[B], level[B], slower[B]
constexpr uint32_t TIMELINE_MAX_PPM = 1000000000u;
static_assert(TIMELINE_MAX_B <= 64, "one wave holds a row's buckets, one lane each");

struct TimelineArgs {
    const float *samples;
    const uint32_t *counts;
    const uint32_t *starts;  // [rows] slot of the oldest sample; null: 0 everywhere
    const int32_t *gid;      // by-gid mode (null: by row)
    float *out;              // by row: [B][rows]; by gid: [local_ranks][B][KS]
    int row_stride;
    int uniform_n;  // >= 0: every launched row holds that many samples
    int rows_active, rows_per_rank;  // by-gid mode: the launch covers rows [0, rows_active) of every logical rank
    int KS;                          // ... and a plane of a logical rank has KS slots
    int rows;                        // by row: the pitch of a plane
    int B;
};

// the first sample of bucket b: the smallest i with i * B / n >= b
__device__ __forceinline__ uint32_t timeline_lo(uint32_t b, uint32_t n, uint32_t B) {
    return (uint32_t)(((uint64_t)b * n + B - 1u) / B);
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_row_timeline(TimelineArgs a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ float s_mean[TIMELINE_MAX_B];

    const int tid = threadIdx.x, lane = tid & 63, wave = (int)uni((uint32_t)tid >> 6);
    const uint32_t B = (uint32_t)a.B;
    int row = (int)blockIdx.x;
    float *dst;
    size_t pitch;  // floats between two planes of this row
    if (a.gid) {
        const int lr = (int)blockIdx.x / a.rows_active;
        row = lr * a.rows_per_rank + ((int)blockIdx.x - lr * a.rows_active);
        const int g = a.gid[row];
        if (g < 0 || g >= a.KS) return;  // not exchanged (block-uniform)
        dst = a.out + (size_t)lr * (size_t)B * (size_t)a.KS + g;
        pitch = (size_t)a.KS;
    } else {
        dst = a.out + row;
        pitch = (size_t)a.rows;
    }
    uint32_t n = a.uniform_n >= 0 ? (uint32_t)a.uniform_n : a.counts[row];
    if (n > (uint32_t)a.row_stride) n = (uint32_t)a.row_stride;
    if (n < 4u * B) {  // block-uniform; by gid the slots keep the -1.0 of the fill ahead of this kernel
        if (!a.gid && (uint32_t)tid < B) dst[(size_t)tid * pitch] = -1.0f;
        return;
    }
    uint32_t start = a.starts ? a.starts[row] : 0u;
    if (start >= n) start %= n;
    const float *__restrict__ src = a.samples + (size_t)row * (size_t)a.row_stride;

    // ---- this wave's buckets, each closed by one wave sum
    const uint32_t b_end = ((uint32_t)(wave + 1) * B + WAVES - 1u) / WAVES;
    for (uint32_t b = ((uint32_t)wave * B + WAVES - 1u) / WAVES; b < b_end; b++) {  // (wave-uniform bounds)
        const uint32_t lo = timeline_lo(b, n, B), hi = timeline_lo(b + 1u, n, B);  // (hi - lo >= 4: n >= 4 B)
        double part = 0.0;
#pragma unroll 4
        for (uint32_t i = lo + (uint32_t)lane; i < hi; i += 64u) {
            uint32_t s = start + i;  // (< 2 n <= 2^17)
            if (s >= n) s -= n;
            part += (double)src[s];
        }
        const double sum = wave_sum_f64(part);
        if (lane == 0) s_mean[b] = (float)__ddiv_rn(sum, (double)(hi - lo));
    }
    __syncthreads();
    if (wave != 0) return;

    // ---- end: lane b holds bucket b
    const bool mine = (uint32_t)lane < B;
    const float m = mine ? s_mean[lane] : 0.0f;
    const bool broken = __ballot(mine && !(fabsf(m) < INFINITY)) != 0ull;  // a NaN or an infinity among the means
    const uint32_t key = f2key(m);
    const int lc = robust_wave_select(key, mine, ~0ull >> (64u - B), (B - 1u) >> 1, (int)B, lane);
    const float c = key2f((uint32_t)__builtin_amdgcn_readlane((int)key, lc));
    if (!mine) return;
    if (broken || !(c > 0.0f)) {
        if (!a.gid) dst[(size_t)lane * pitch] = -1.0f;
        return;
    }
    dst[(size_t)lane * pitch] = (float)__ddiv_rn((double)m, (double)c);
}

struct TimelineRankArgs {
    const float *planes;  // [ranks][B][KS]
    float *out;           // [ranks][2][3][B]
    int K, S, B;
    float above;  // (float)(1 + effect_ppm / 1e6)
};

// a slot's key: the marker pace_radix_select skips where the row did not take part (-1.0; a ratio is never negative)
__device__ __forceinline__ uint32_t timeline_key(float x) { return x >= 0.0f ? f2key(x) : PACE_MARK; }

template <int THREADS, int NREG>
__global__ __launch_bounds__(THREADS) void k_timeline_rank(TimelineRankArgs a) {
    constexpr int WAVES = THREADS / 64;
    constexpr int NKEYS = NREG ? NREG : 1;
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[THREADS == 64 ? 4 : TAIL_BINS];
    __shared__ uint32_t s_wave[WAVES];
    __shared__ uint32_t s_sel[2];
    __shared__ uint32_t s_cnt[2][WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int B = a.B, KS = a.K + a.S;
    const int r = (int)blockIdx.x, b = (int)blockIdx.y;
    const float *__restrict__ plane = a.planes + ((size_t)r * B + b) * (size_t)KS;
    const uint32_t akey = f2key(a.above);
#pragma unroll 1
    for (int fam = 0; fam < 2; fam++) {
        const int ncols = fam ? a.S : a.K;
        const float *__restrict__ col = plane + (fam ? a.K : 0);
        float *dst = a.out + (((size_t)r * 2 + fam) * TIMELINE_FIELDS) * (size_t)B + b;
        uint32_t keys[NKEYS];
        uint32_t rows = 0, slower = 0, level = __float_as_uint(-1.0f);
        if constexpr (THREADS == 64) {
            keys[0] = lane < ncols ? timeline_key(col[lane]) : PACE_MARK;
            const bool has = keys[0] != PACE_MARK;
            const unsigned long long mask = __ballot(has);
            rows = (uint32_t)__popcll(mask);
            slower = (uint32_t)__popcll(__ballot(has && keys[0] > akey));
            if (rows != 0) {  // wave-uniform
                const int ls = robust_wave_select(keys[0], has, mask, (rows - 1u) >> 1, ncols, lane);
                level = __float_as_uint(key2f((uint32_t)__builtin_amdgcn_readlane((int)keys[0], ls)));
            }
        } else {
            auto count = [&](uint32_t key) {
                rows += key != PACE_MARK ? 1u : 0u;
                slower += (key != PACE_MARK && key > akey) ? 1u : 0u;
            };
            if constexpr (NREG > 0) {
#pragma unroll
                for (int j = 0; j < NREG; j++) {
                    const int i = tid + j * THREADS;
                    keys[j] = i < ncols ? timeline_key(col[i]) : PACE_MARK;
                    count(keys[j]);
                }
            } else {
                keys[0] = PACE_MARK;
                for (int i = tid; i < ncols; i += THREADS) count(timeline_key(col[i]));
            }
            rows = wave_sum_u32(rows);
            slower = wave_sum_u32(slower);
            __syncthreads();  // (the family before has read s_cnt)
            if (lane == 0) s_cnt[0][wave] = rows, s_cnt[1][wave] = slower;
            __syncthreads();
            rows = slower = 0;
#pragma unroll
            for (int w = 0; w < WAVES; w++) rows += s_cnt[0][w], slower += s_cnt[1][w];
            rows = uni(rows);
            if (rows != 0) {  // block-uniform
                const uint32_t target = (rows - 1u) >> 1;
                if constexpr (NREG > 0)
                    level = pace_radix_select<THREADS, NREG>([&](int j) { return keys[j]; }, ncols, target, s_hist, s_wave, s_sel);
                else
                    level = pace_radix_select<THREADS, 0>([&](int i) { return timeline_key(col[i]); }, ncols, target, s_hist, s_wave, s_sel);
                level = __float_as_uint(key2f(level));
            }
        }
        if (tid == 0) {
            dst[0] = (float)rows;
            dst[B] = __uint_as_float(level);
            dst[2 * B] = (float)slower;
        }
    }
}

constexpr int TIMELINE_WAVE_COLS = 64;        // columns of a family one wave takes
constexpr int TIMELINE_REG_COLS = 256 * 16;  // ... and 256 threads keep in registers

struct TimelineScoreArgs {
    const float *blocks;  // [R][2][3][B]
    uint32_t *out;        // [n_ranks][2][4 + B]
    int R, B, first_rank;
    uint32_t min_rows, breadth_ppm;
    double slow_at;  // 1 + effect_ppm / 1e6
};

__global__ __launch_bounds__(64) void k_timeline_score(TimelineScoreArgs a) {
    const int lane = threadIdx.x, B = a.B, fam = (int)blockIdx.y;
    const bool mine = lane < B;
    const int at = mine ? lane : 0;
    const size_t pitch = (size_t)2 * TIMELINE_FIELDS * B;  // floats of a rank
    const float *__restrict__ col = a.blocks + (size_t)fam * TIMELINE_FIELDS * B + at;
    const float min_rows = (float)a.min_rows;  // (counts travel as floats: exact up to 2^24)
    // ---- the reference of every bucket: the smallest level among the ranks with enough rows there
    float ref = INFINITY;
#pragma unroll 4
    for (int r = 0; r < a.R; r++) {
        const float rows = col[(size_t)r * pitch], level = col[(size_t)r * pitch + B];
        ref = (rows >= min_rows && level < ref) ? level : ref;
    }
    const float *__restrict__ own = col + (size_t)(a.first_rank + (int)blockIdx.x) * pitch;
    const float rows = own[0], level = own[B], slower = own[2 * B];
    const bool rated = mine && rows >= min_rows;
    const float rel = rated ? (float)__ddiv_rn((double)level, (double)ref) : __builtin_nanf("");
    const bool slow = rated && (double)rel >= a.slow_at &&
                      (uint64_t)slower * 1000000ull >= (uint64_t)a.breadth_ppm * (uint64_t)rows;
    // ---- one ballot; the rest is scalar work on its mask
    const unsigned long long mask = __ballot(slow);
    unsigned long long left = mask, last = 0ull;  // bit i of `left` after t steps: buckets i .. i + t are all slow
    uint32_t run_len = 0;
    while (left) {  // (wave-uniform: at most B steps)
        last = left;
        left &= left >> 1;
        run_len++;
    }
    const uint32_t run_first = run_len ? 63u - (uint32_t)__clzll((long long)last) : 0u;  // among equal runs the most recent
    const bool in_run = (uint32_t)lane >= run_first && (uint32_t)lane < run_first + run_len;
    const double sum = wave_sum_f64(in_run ? (double)rel : 0.0);
    const float excess = run_len ? (float)__ddiv_rn(sum, (double)run_len) : 1.0f;
    uint32_t *dst = a.out + ((size_t)blockIdx.x * 2 + fam) * (size_t)(4 + B);
    if (lane == 0) {
        dst[0] = (uint32_t)__popcll(mask), dst[1] = run_first, dst[2] = run_len, dst[3] = __float_as_uint(excess);
    }
    if (mine) dst[4 + lane] = __float_as_uint(rel);
}

// 256 threads for the rows profile_launch gives 256, 1024 beyond
int timeline_launch(const TimelineArgs &a, int blocks, hipStream_t st) {
    if (blocks == 0) return NVRX_OK;
    if (a.row_stride <= PROFILE_STAGE_256)
        hipLaunchKernelGGL((k_row_timeline<256>), dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_row_timeline<1024>), dim3(blocks), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

int timeline_b_check(int B) {
    if (B < TIMELINE_MIN_B || B > TIMELINE_MAX_B) return fail(NVRX_ERR_RANGE, "B=%d buckets outside [%d,%d]", B, TIMELINE_MIN_B, TIMELINE_MAX_B);
    return NVRX_OK;
}

int timeline_ppm_check(const char *name, uint32_t ppm) {
    if (ppm > TIMELINE_MAX_PPM) return fail(NVRX_ERR_RANGE, "%s=%u exceeds %u", name, ppm, TIMELINE_MAX_PPM);
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_row_timeline(const float *d_samples, const uint32_t *d_counts, const uint32_t *d_starts, int rows, int row_stride, int B,
                      float *d_out, void *stream) {
    const int rc = row_op_check(rows, row_stride, d_samples, d_counts, d_out, false, [&] { return timeline_b_check(B); });
    if (rc || rows == 0) return rc;
    TimelineArgs a{};
    a.samples = d_samples, a.counts = d_counts, a.starts = d_starts, a.out = d_out;
    a.row_stride = row_stride, a.uniform_n = -1, a.rows = rows, a.B = B;
    return timeline_launch(a, rows, as_stream(stream));
}

int nvrx_timeline_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, int B, float *d_planes, int K, int S, int rows_active,
                        void *stream) {
    hipStream_t st = as_stream(stream);
    LocalWindow w;
    int rc = local_window(ctx, desc, d_planes, K, S, rows_active, [&] { return timeline_b_check(B); }, STARTS_OFF, &st, &w);
    if (rc) return rc;
    TimelineArgs a{};
    window_args(w, &a);
    a.starts = w.starts;
    a.out = d_planes;
    a.KS = K + S, a.B = B;
    const size_t slots = (size_t)ctx->local_ranks * (size_t)B * (size_t)a.KS;
    if (slots == 0) return NVRX_OK;
    rc = fill_minus_one(d_planes, slots, st);
    if (rc) return rc;
    return timeline_launch(a, ctx->local_ranks * w.rows_active, st);
}

int nvrx_timeline_rank(const float *d_planes, int ranks, int B, int K, int S, uint32_t effect_ppm, float *d_out, void *stream) {
    if (ranks < 0 || K < 0 || S < 0) return fail(NVRX_ERR_INVALID, "bad shape ranks=%d K=%d S=%d", ranks, K, S);
    if (K > NVRX_MAX_ROWS || S > NVRX_MAX_ROWS) return fail(NVRX_ERR_RANGE, "K=%d S=%d column ids, at most %d each", K, S, NVRX_MAX_ROWS);
    if (const int rc = timeline_b_check(B)) return rc;
    if (const int rc = timeline_ppm_check("effect_ppm", effect_ppm)) return rc;
    if (ranks == 0) return NVRX_OK;
    if (!d_out || (K + S > 0 && !d_planes)) return fail(NVRX_ERR_INVALID, "null device pointer");
    TimelineRankArgs a{};
    a.planes = d_planes, a.out = d_out;
    a.K = K, a.S = S, a.B = B;
    a.above = (float)(1.0 + (double)effect_ppm / 1e6);
    hipStream_t st = as_stream(stream);
    const int widest = K > S ? K : S;
    if (widest <= TIMELINE_WAVE_COLS)
        hipLaunchKernelGGL((k_timeline_rank<64, 1>), dim3(ranks, B), dim3(64), 0, st, a);
    else if (widest <= TIMELINE_REG_COLS)
        hipLaunchKernelGGL((k_timeline_rank<256, 16>), dim3(ranks, B), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_timeline_rank<1024, 0>), dim3(ranks, B), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

int nvrx_timeline_score(const float *d_blocks, int R, int B, int first_rank, int n_ranks, uint32_t min_rows, uint32_t effect_ppm,
                        uint32_t breadth_ppm, void *d_out, void *stream) {
    if (R <= 0) return fail(NVRX_ERR_INVALID, "bad table shape R=%d", R);
    if (const int rc = timeline_b_check(B)) return rc;
    if (first_rank < 0 || n_ranks < 1 || first_rank > R - n_ranks)
        return fail(NVRX_ERR_RANGE, "ranks [%d,%d+%d) outside the table's %d", first_rank, first_rank, n_ranks, R);
    if (min_rows < 1u || min_rows > (uint32_t)NVRX_MAX_ROWS)
        return fail(NVRX_ERR_RANGE, "min_rows=%u outside [1,%d]", min_rows, NVRX_MAX_ROWS);
    if (const int rc = timeline_ppm_check("effect_ppm", effect_ppm)) return rc;
    if (breadth_ppm > 1000000u) return fail(NVRX_ERR_RANGE, "breadth_ppm=%u exceeds 1000000", breadth_ppm);
    if (!d_blocks || !d_out) return fail(NVRX_ERR_INVALID, "null device pointer");
    TimelineScoreArgs a{};
    a.blocks = d_blocks, a.out = static_cast<uint32_t *>(d_out);
    a.R = R, a.B = B, a.first_rank = first_rank;
    a.min_rows = min_rows, a.breadth_ppm = breadth_ppm;
    a.slow_at = 1.0 + (double)effect_ppm / 1e6;
    hipLaunchKernelGGL(k_timeline_score, dim3(n_ranks, 2), dim3(64), 0, as_stream(stream), a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // extern "C"
