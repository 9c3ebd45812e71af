// nvrx_robust.inl -- robust scores: every rank against the job's median and spread.  Part of the translation unit
// nvrx_straggler.hip (included at its end: it uses that file's key maps, DPP scans and sums, and nvrx_tail.inl's histogram
// add).
//
// Every relative score of the reference (reporting.py:196-253) divides the FASTEST rank's median by this rank's: one
// anomalously fast rank flags the whole job, the minimum over R ranks drifts with R, and a fixed threshold does not know
// the job's own spread.  Here the reference point of a column (one kernel id or section id of the exchanged table) is the
// lower median `ctr` of the ranks that have the row, its spread the median absolute deviation `mad` around it, and a rank
// gets a ratio ctr / v and a modified z-score (v - ctr) / max(1.4826 * mad, floor_rel * ctr).  The table is the one
// nvrx_score reads; nothing else is exchanged.
//
// k_robust_cols<0>  R <= 64: a 256-thread workgroup stages 64 consecutive columns x R rows in LDS (256 B per table row,
//   rows padded to 65 words so that a wave reading one column touches 64 banks), then every wave takes columns in turn
//   with rank r's value in lane r.  A lane's position in the sorted column is the number of present keys that order
//   before its own (ties: the lower lane first), counted over a readlane broadcast of all R keys; the lane at position
//   (n-1) >> 1 holds the lower median.  The same selection runs on the deviations.  One barrier (after the staging), no
//   atomics, no scratch.
// k_robust_cols<T>  R > 64: one workgroup per column, MSB-first radix select in three fixed passes (12 + 12 + 8 bits,
//   LDS histogram) as k_row_quantile does, first over f2key of the present values (read at stride L from the L2-resident
//   table), then over the bit patterns of |v - ctr| (sign bits clear: unsigned order is value order).  Absent entries
//   never enter a histogram.  Exact, ties and all, no data-dependent path.
// k_robust_rank  one workgroup per reported rank, shaped like k_tail_score.

namespace {

constexpr int ROBUST_TILE = 64;       // columns per workgroup of the small kernel
constexpr int ROBUST_PITCH = 65;      // LDS words per staged table row
constexpr int ROBUST_THREADS = 256;

struct RobustColsArgs {
    const float *table;  // [R][L]
    int R, KS, L;
    int min_ranks;
    float floor_rel;
    uint4 *cols;  // [KS] {f32 ctr, f32 mad, f32 scale, u32 n}
};

__device__ __forceinline__ uint4 robust_record(float ctr, float mad, uint32_t n, const RobustColsArgs &a) {
    if ((int)n < a.min_ranks || n == 0) {
        const uint32_t nan = __float_as_uint(__builtin_nanf(""));
        return make_uint4(nan, nan, nan, n);
    }
    const float scale = fmaxf(1.4826f * mad, a.floor_rel * ctr);
    return make_uint4(__float_as_uint(ctr), __float_as_uint(mad), __float_as_uint(scale), n);
}

// bit pattern of |v - ctr| (a NaN -- inf - inf -- orders above +inf)
__device__ __forceinline__ uint32_t robust_dev_bits(float v, float ctr) { return __float_as_uint(v - ctr) & 0x7FFFFFFFu; }

// the lane whose key has position `target` among the present keys of the wave (ties: the lower lane first)
__device__ __forceinline__ int robust_wave_select(uint32_t key, bool present, unsigned long long mask, uint32_t target, int R,
                                                  int lane) {
    uint32_t pos = 0;
    for (int j = 0; j < R; j++) {
        const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key, j);
        const bool pj = (mask >> j) & 1ull;
        pos += (pj && (kj < key || (kj == key && j < lane))) ? 1u : 0u;
    }
    const unsigned long long hit = __ballot(present && pos == target);
    return __ffsll((long long)hit) - 1;
}

// What every pass of a radix select does once its histogram is complete (the caller's barrier is behind it): thread sums, a
// scan over the workgroup, and the one thread whose stretch holds rank k names the bin.  Returns that bin; k becomes the rank
// inside it.  Every thread of the workgroup calls it (two barriers inside; s_sel and s_wave are rewritten only behind the next
// pass' two barriers).
template <int THREADS>
__device__ __forceinline__ uint32_t radix_pick(const uint32_t *s_hist, uint32_t *s_wave, uint32_t *s_sel, uint32_t &k) {
    constexpr int WAVES = THREADS / 64;
    constexpr int PER = TAIL_BINS / THREADS;
    static_assert(PER % 4 == 0, "a thread's bins are read as 16-byte words");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t h[PER];
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < PER; j += 4) {
        const uint4 q = reinterpret_cast<const uint4 *>(s_hist)[(tid * PER + j) >> 2];
        h[j] = q.x, h[j + 1] = q.y, h[j + 2] = q.z, h[j + 3] = q.w;
        mine += q.x + q.y + q.z + q.w;
    }
    const uint32_t incl = wave_scan_u32(mine);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t below = incl - mine;
#pragma unroll
    for (int w = 0; w < WAVES; w++) below += w < wave ? s_wave[w] : 0u;
    if (k >= below && k < below + mine) {  // exactly one thread
        uint32_t b = 0, acc = below;
        bool found = false;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const bool adv = !found && k >= acc + h[j];
            acc += adv ? h[j] : 0u;
            b += adv ? 1u : 0u;
            found = found || !adv;
        }
        s_sel[0] = (uint32_t)(tid * PER) + b;
        s_sel[1] = acc;
    }
    __syncthreads();
    const uint32_t bin = uni(s_sel[0]);
    k -= uni(s_sel[1]);
    return bin;
}

// three-pass radix select over the column's present entries: the key of rank k.  `dev`: keys are robust_dev_bits(v, ctr),
// else f2key(v).  Every thread of the workgroup calls it with the same arguments (barriers inside).
template <int THREADS, bool DEV>
__device__ __forceinline__ uint32_t robust_radix_select(const float *__restrict__ col, int R, int L, float v0, float ctr,
                                                        uint32_t k, uint32_t *s_hist, uint32_t *s_wave, uint32_t *s_sel) {
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
        for (int r = tid; r < R; r += THREADS) {
            const float v = r == tid ? v0 : col[(size_t)r * (size_t)L];
            const uint32_t key = DEV ? robust_dev_bits(v, ctr) : f2key(v);
            const bool on = v >= 0.0f && (up == 32 || (key >> up) == prefix);
            tail_hist_add(s_hist, (key >> shift) & bmask, on);
        }
        __syncthreads();
        const uint32_t bin = radix_pick<THREADS>(s_hist, s_wave, s_sel, k);
        prefix = pass == 2 ? ((prefix << 8) | bin) : ((prefix << 12) | bin);
        // (s_sel and s_wave are rewritten only behind the next pass' two barriers)
    }
    return prefix;
}

// THREADS == 0: the tiled kernel for R <= 64 (ROBUST_THREADS threads); else one workgroup of THREADS per column
template <int THREADS>
__global__ __launch_bounds__(THREADS ? THREADS : ROBUST_THREADS) void k_robust_cols(RobustColsArgs a) {
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
            const unsigned long long mask = __ballot(present);
            const uint32_t n = (uint32_t)__popcll(mask);
            float ctr = 0.0f, mad = 0.0f;
            if (n != 0 && (int)n >= a.min_ranks) {  // wave-uniform
                const uint32_t target = (n - 1u) >> 1;
                const int lc = robust_wave_select(f2key(v), present, mask, target, R, lane);
                ctr = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), lc));
                const uint32_t d = robust_dev_bits(v, ctr);
                const int lm = robust_wave_select(d, present, mask, target, R, lane);
                mad = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)d, lm));
            }
            if (lane == 0) a.cols[c] = robust_record(ctr, mad, n, a);
        }
    } else {
        constexpr int WAVES = THREADS / 64;
        __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
        __shared__ uint32_t s_wave[WAVES];
        __shared__ uint32_t s_sel[2];
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
        if (n == 0 || (int)n < a.min_ranks) {  // block-uniform
            if (tid == 0) a.cols[c] = robust_record(0.0f, 0.0f, n, a);
            return;
        }
        // (s_wave is rewritten only behind the first pass' two barriers)
        const uint32_t target = (n - 1u) >> 1;
        const float ctr = key2f(robust_radix_select<THREADS, false>(col, R, L, v0, 0.0f, target, s_hist, s_wave, s_sel));
        const float mad = __uint_as_float(robust_radix_select<THREADS, true>(col, R, L, v0, ctr, target, s_hist, s_wave, s_sel));
        if (tid == 0) a.cols[c] = robust_record(ctr, mad, n, a);
    }
}

struct RobustRankArgs {
    const float *table;  // [R][L]
    const uint4 *cols;   // [KS]
    int K, S;
    int first_rank;
    int min_ranks;
    float *out;  // [n_ranks][2][1 + S]
};

// one workgroup per reported rank: {gpu, section[S]} ratios, then the same of z
__global__ __launch_bounds__(ROBUST_THREADS) void k_robust_rank(RobustRankArgs a) {
    constexpr int NW = ROBUST_THREADS / 64;
    __shared__ double s_sum[3][NW];
    __shared__ uint32_t s_cnt[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, S = a.S, KS = K + S;
    const int L = NVRX_TABLE_LEN(K, S);
    const int r = a.first_rank + (int)blockIdx.x;
    const float *__restrict__ row = a.table + (size_t)r * L;
    float *__restrict__ ratio = a.out + (size_t)blockIdx.x * 2 * (size_t)(1 + S);
    float *__restrict__ z = ratio + (1 + S);
    const float NaN = __builtin_nanf("");

    for (int s = tid; s < S; s += ROBUST_THREADS) {
        const float v = row[K + s];
        const uint4 rec = a.cols[K + s];
        const bool ok = v >= 0.0f && rec.w != 0u && (int)rec.w >= a.min_ranks;
        const double ctr = (double)__uint_as_float(rec.x), scale = (double)__uint_as_float(rec.z);
        ratio[1 + s] = ok ? (float)(ctr / (double)v) : NaN;
        z[1 + s] = ok ? (float)(((double)v - ctr) / scale) : NaN;
    }
    double ws = 0.0, sr = 0.0, sz = 0.0;
    uint32_t cnt = 0;
    for (int k = tid; k < K; k += ROBUST_THREADS) {
        const float v = row[k];
        if (!(v >= 0.0f)) continue;
        const uint4 rec = a.cols[k];
        if (rec.w == 0u || (int)rec.w < a.min_ranks) continue;
        const double ctr = (double)__uint_as_float(rec.x), scale = (double)__uint_as_float(rec.z);
        const double w = (double)row[2 * KS + k];
        sr += w * (ctr / (double)v);
        sz += w * (((double)v - ctr) / scale);
        ws += w;
        cnt++;
    }
    ws = wave_sum_f64(ws);
    sr = wave_sum_f64(sr);
    sz = wave_sum_f64(sz);
    cnt = wave_sum_u32(cnt);
    if (lane == 0) {
        s_sum[0][wave] = ws;
        s_sum[1][wave] = sr;
        s_sum[2][wave] = sz;
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        ws = sr = sz = 0.0;
        cnt = 0;
        for (int w = 0; w < NW; w++) {
            ws += s_sum[0][w];
            sr += s_sum[1][w];
            sz += s_sum[2][w];
            cnt += s_cnt[w];
        }
        ratio[0] = cnt ? (float)(sr / ws) : NaN;
        z[0] = cnt ? (float)(sz / ws) : NaN;
    }
}

// argument checks shared by both entry points; nothing here touches a device
int robust_check(int R, int K, int S, int first_rank, int n_ranks, int min_ranks, float floor_rel) {
    const int rc = table_min_ranks_check(R, K, S, first_rank, n_ranks, min_ranks);
    if (rc) return rc;
    if (!(floor_rel == floor_rel) || floor_rel - floor_rel != 0.0f) return fail(NVRX_ERR_INVALID, "floor_rel is not finite");
    if (floor_rel < 0.0f || floor_rel > 1.0f) return fail(NVRX_ERR_RANGE, "floor_rel=%g outside [0,1]", (double)floor_rel);
    return NVRX_OK;
}

// The variant of a columns kernel by the rows a column has (a table's R ranks, or the largest group's members): the tiled kernel
// up to 64 (a row per lane), one workgroup of 256 per column up to 1024, of 1024 beyond.  G > 1: the grid's y, a group each.
template <class Args>
void cols_launch(void (*tiled)(Args), void (*k256)(Args), void (*k1024)(Args), int rows, int KS, int G, const Args &c,
                 hipStream_t st) {
    if (rows <= 64)
        hipLaunchKernelGGL(tiled, dim3((KS + ROBUST_TILE - 1) / ROBUST_TILE, G), dim3(ROBUST_THREADS), 0, st, c);
    else if (rows <= 1024)
        hipLaunchKernelGGL(k256, dim3(KS, G), dim3(256), 0, st, c);
    else
        hipLaunchKernelGGL(k1024, dim3(KS, G), dim3(1024), 0, st, c);
}

int robust_launch(const float *d_table, int R, int K, int S, int first_rank, int n_ranks, int min_ranks, float floor_rel,
                  void *d_out, hipStream_t st) {
    const int KS = K + S;
    if (KS > 0) {
        RobustColsArgs c{};
        c.table = d_table, c.R = R, c.KS = KS, c.L = NVRX_TABLE_LEN(K, S);
        c.min_ranks = min_ranks, c.floor_rel = floor_rel;
        c.cols = static_cast<uint4 *>(d_out);
        cols_launch(k_robust_cols<0>, k_robust_cols<256>, k_robust_cols<1024>, R, KS, 1, c, st);
        HIP_TRY(hipGetLastError());
    }
    RobustRankArgs a{};
    a.table = d_table, a.cols = static_cast<const uint4 *>(d_out);
    a.K = K, a.S = S, a.first_rank = first_rank, a.min_ranks = min_ranks;
    a.out = static_cast<float *>(d_out) + 4 * (size_t)KS;
    hipLaunchKernelGGL(k_robust_rank, dim3(n_ranks), dim3(ROBUST_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_robust_score(const float *d_table, int R, int K, int S, int first_rank, int n_ranks, int min_ranks,
                      float floor_rel, void *d_out, void *stream) {
    const int rc = robust_check(R, K, S, first_rank, n_ranks, min_ranks, floor_rel);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_table != nullptr, false)) return rc;
    return robust_launch(d_table, R, K, S, first_rank, n_ranks, min_ranks, floor_rel, d_out, as_stream(stream));
}

int nvrx_report_robust(nvrx_ctx *ctx, const nvrx_report_desc *desc, int first_rank, int n_ranks, int min_ranks,
                       float floor_rel, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = robust_check(desc->R, desc->K, desc->S, first_rank, n_ranks, min_ranks, floor_rel);
    if (rc) return rc;
    if (const int rc = out_check(d_out, true, true)) return rc;
    hipStream_t home = nullptr;
    const float *table = nullptr;
    if (const int rc = report_table(ctx, desc, &home, &table)) return rc;
    return robust_launch(table, desc->R, desc->K, desc->S, first_rank, n_ranks, min_ranks, floor_rel, d_out, home);
}

}  // extern "C"
