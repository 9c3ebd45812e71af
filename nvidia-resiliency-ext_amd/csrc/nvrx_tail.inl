// nvrx_tail.inl -- tail scores: the q-quantile of every ring row and relative scores built from it.  Part of the
// translation unit nvrx_straggler.hip (included at its end: it uses that file's key maps, DPP reductions, column-minimum
// kernels and context).
//
// Every score of the reference compares MEDIANS (straggler.py:172-197, reporting.py:196-253) and so cannot see a rank that
// is slow on some iterations only.  k_row_quantile selects the nearest-rank q-quantile of a row -- the element of rank
// k = ceil(q * n) - 1 of the row sorted by f2key, an actual sample -- and k_tail_score divides column minima of those
// tails by each rank's own, exactly as k_score does with medians.
//
// k_row_quantile: one workgroup per ring row, MSB-first radix select over the 32-bit keys in three fixed passes
// (12 + 12 + 8 bits).  A pass counts the keys that still match the prefix found so far into a 4096-bin LDS histogram
// (non-returning ds_add), every thread sums its stretch of bins, a DPP scan over the thread sums finds the bin holding
// rank k, and k becomes the rank inside that bin.  After the third pass the prefix IS the key: always exact, ties and
// all, no data-dependent path, no scratch memory, no global atomic.  The row is read three times (the first 16 bytes of
// every lane stay in registers: rows of up to THREADS*4 samples are read once); passes two and three hit the L2.
// Timings of one row share sign, exponent and the leading mantissa bits, so the first pass piles nearly every key into
// one or two bins and same-address LDS atomics serialise: a wave first agrees on the bin of its first active lane and
// adds the popcount of the lanes that share it once (twice over: two hot bins), only the rest add on their own.

namespace {

constexpr int TAIL_BINS = 4096;
constexpr uint32_t TAIL_Q_MIN = 500000u, TAIL_Q_MAX = 999999u;

struct QuantArgs {
    const float *samples;
    const uint32_t *counts;
    const int32_t *gid;  // by-gid mode (null: by row)
    float *out;
    int row_stride;
    int uniform_n;  // >= 0: every launched row holds that many samples
    int rows_active, rows_per_rank;  // by-gid mode: the launch covers rows [0, rows_active) of every logical rank
    int KS;                          // ... and a logical rank's tail row has KS slots
    uint32_t q_ppm;
};

// one key into the pass histogram; `on` lanes only.  Wave-aggregated for up to two hot bins.
__device__ __forceinline__ void tail_hist_add(uint32_t *hist, uint32_t bin, bool on) {
    bool todo = on;
#pragma unroll
    for (int round = 0; round < 2; round++) {
        if (todo) {
            const uint32_t b0 = uni(bin);
            const bool same = bin == b0;
            const unsigned long long m = __ballot(same);  // (of the lanes still in here)
            if (same) {
                if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&hist[b0], (uint32_t)__popcll(m));
                todo = false;
            }
        }
    }
    if (todo) atomicAdd(&hist[bin], 1u);
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_row_quantile(QuantArgs a) {
    constexpr int WAVES = THREADS / 64;
    constexpr int PER = TAIL_BINS / THREADS;  // consecutive bins summed per thread
    static_assert(PER % 4 == 0, "a thread's bins are read as 16-byte words");
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
    __shared__ uint32_t s_wave[WAVES];
    __shared__ uint32_t s_sel[2];  // {bin holding rank k, keys below that bin}

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int row = (int)blockIdx.x;
    float *dst;
    if (a.gid) {
        const int lr = (int)blockIdx.x / a.rows_active;
        row = lr * a.rows_per_rank + ((int)blockIdx.x - lr * a.rows_active);
        const int g = a.gid[row];
        if (g < 0 || g >= a.KS) return;  // not exchanged (block-uniform)
        dst = a.out + (size_t)lr * a.KS + g;
    } else {
        dst = a.out + row;
    }
    uint32_t n = a.uniform_n >= 0 ? (uint32_t)a.uniform_n : a.counts[row];
    if (n > (uint32_t)a.row_stride) n = (uint32_t)a.row_stride;
    if (n == 0) {  // block-uniform; by gid the slot keeps the -1.0 of the fill ahead of this kernel
        if (!a.gid && tid == 0) *dst = -1.0f;
        return;
    }
    // nearest rank: ceil(q * n) - 1 in integers
    uint32_t k = (uint32_t)(((uint64_t)a.q_ppm * n + 999999ull) / 1000000ull) - 1u;

    const float4 *__restrict__ src = reinterpret_cast<const float4 *>(a.samples + (size_t)row * (size_t)a.row_stride);
    const int nvec = (int)((n + 3u) >> 2);  // 16-byte words holding a sample (row_stride % 4 == 0: all inside the row)
    float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < nvec) x0 = src[tid];

    uint32_t prefix = 0;  // the key's bits above `shift`, found so far
#pragma unroll 1
    for (int pass = 0; pass < 3; pass++) {
        const int shift = pass == 0 ? 20 : pass == 1 ? 8 : 0;  // this pass bins bits [shift, shift + 12) (8 in the last)
        const int up = pass == 0 ? 32 : pass == 1 ? 20 : 8;    // bits [up, 32) must equal the prefix
        const uint32_t bmask = pass == 2 ? 0xFFu : 0xFFFu;
#pragma unroll
        for (int j = 0; j < PER; j += 4) reinterpret_cast<uint4 *>(s_hist)[(tid * PER + j) >> 2] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        for (int v = tid; v < nvec; v += THREADS) {
            const float4 x = v == tid ? x0 : src[v];
            const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t key = f2key(xs[c]);
                const bool on = (uint32_t)(v * 4 + c) < n && (up == 32 || (key >> up) == prefix);
                tail_hist_add(s_hist, (key >> shift) & bmask, on);
            }
        }
        __syncthreads();
        // thread sums -> scan over the workgroup -> the one thread whose stretch holds rank k names the bin
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
        if (k >= below && k < below + mine) {  // exactly one thread (the counts of this pass sum to more than k)
            // the first bin whose end is past k; the running sum stops in front of it (no break: h[] stays in registers)
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
        prefix = pass == 2 ? ((prefix << 8) | bin) : ((prefix << 12) | bin);
        // (s_sel and s_wave are rewritten only behind the next pass' two barriers)
    }
    if (tid == 0) *dst = key2f(prefix);
}

struct TailScoreArgs {
    const float *tails;   // [R][KS] with a pitch of ld floats
    int ld;
    const float *table;   // [R][L]: the weights
    const float *colmin;  // [KS]
    int R, K, S;
    int first_rank;
    float *out;  // [n_ranks][1 + S]
};

constexpr int TAIL_SCORE_THREADS = 256;

// one workgroup per reported rank: {gpu_tail, section_tail[S]}
__global__ __launch_bounds__(TAIL_SCORE_THREADS) void k_tail_score(TailScoreArgs a) {
    constexpr int NW = TAIL_SCORE_THREADS / 64;
    __shared__ double s_sum[2][NW];
    __shared__ uint32_t s_cnt[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, S = a.S, KS = K + S;
    const int L = NVRX_TABLE_LEN(K, S);
    const int r = a.first_rank + (int)blockIdx.x;
    const float *__restrict__ tail = a.tails + (size_t)r * (size_t)a.ld;
    const float *__restrict__ wrow = a.table + (size_t)r * L + 2 * KS;
    float *__restrict__ out = a.out + (size_t)blockIdx.x * (size_t)(1 + S);
    const float NaN = __builtin_nanf("");

    for (int s = tid; s < S; s += TAIL_SCORE_THREADS) {
        const float t = tail[K + s];
        out[1 + s] = t >= 0.0f ? (float)((double)a.colmin[K + s] / (double)t) : NaN;
    }
    double ws = 0.0, ss = 0.0;
    uint32_t cnt = 0;
    for (int k = tid; k < K; k += TAIL_SCORE_THREADS) {
        const float t = tail[k];
        if (!(t >= 0.0f)) continue;
        const float ref = a.colmin[k];
        if (!(ref == ref)) continue;
        const double w = (double)wrow[k];
        ss += ((double)ref / (double)t) * w;
        ws += w;
        cnt++;
    }
    ws = wave_sum_f64(ws);
    ss = wave_sum_f64(ss);
    cnt = wave_sum_u32(cnt);
    if (lane == 0) {
        s_sum[0][wave] = ws;
        s_sum[1][wave] = ss;
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        ws = ss = 0.0;
        cnt = 0;
        for (int w = 0; w < NW; w++) {
            ws += s_sum[0][w];
            ss += s_sum[1][w];
            cnt += s_cnt[w];
        }
        out[0] = cnt ? (float)(ss / ws) : NaN;
    }
}

int quantile_launch(const QuantArgs &a, int blocks, hipStream_t st) {
    if (blocks == 0) return NVRX_OK;
    if (a.row_stride <= 256 * 4 * 4)
        hipLaunchKernelGGL(k_row_quantile<256>, dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_row_quantile<1024>, dim3(blocks), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

// column minima of a [R][KS] table whose rows are ld floats apart, then k_tail_score (arguments checked by the caller)
int tail_score_launch(const float *d_tails, int ld, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                      float *d_colmin_scratch, float *d_out, hipStream_t st) {
    const int KS = K + S;
    if (KS > 0) {
        // attr_colmin with the tail table's own pitch: every column of a [R][KS] table
        if (R > 64) {
            const int chunks = std::max(1, std::min(COLMIN_MAX_CHUNKS, (R + 63) / 64));
            const int rows_per_chunk = (R + chunks - 1) / chunks;
            float *part = d_colmin_scratch + KS;
            hipLaunchKernelGGL(k_colmin_part, dim3((KS + 63) / 64, chunks), dim3(256), 0, st, d_tails, R, KS, ld, rows_per_chunk, part);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_colmin_finish, dim3((KS + 255) / 256), dim3(256), 0, st, part, chunks, KS, d_colmin_scratch);
        } else {
            hipLaunchKernelGGL(k_colmin, dim3((KS + 255) / 256), dim3(256), 0, st, d_tails, R, KS, ld, d_colmin_scratch);
        }
        HIP_TRY(hipGetLastError());
    }
    TailScoreArgs a{};
    a.tails = d_tails, a.ld = ld, a.table = d_table, a.colmin = d_colmin_scratch;
    a.R = R, a.K = K, a.S = S, a.first_rank = first_rank, a.out = d_out;
    hipLaunchKernelGGL(k_tail_score, dim3(n_ranks), dim3(TAIL_SCORE_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

int tail_q_check(uint32_t q_ppm) {
    if (q_ppm < TAIL_Q_MIN || q_ppm > TAIL_Q_MAX)
        return fail(NVRX_ERR_RANGE, "q_ppm=%u outside [%u,%u]", q_ppm, TAIL_Q_MIN, TAIL_Q_MAX);
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_row_quantile(const float *d_samples, const uint32_t *d_counts, int rows, int row_stride, uint32_t q_ppm,
                      float *d_out, void *stream) {
    const int rc = row_op_check(rows, row_stride, d_samples, d_counts, d_out, false, [&] { return tail_q_check(q_ppm); });
    if (rc || rows == 0) return rc;
    QuantArgs a{};
    a.samples = d_samples, a.counts = d_counts, a.out = d_out;
    a.row_stride = row_stride, a.uniform_n = -1, a.q_ppm = q_ppm;
    return quantile_launch(a, rows, as_stream(stream));
}

int nvrx_tail_score(const float *d_tails, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                    float *d_colmin_scratch, float *d_out, void *stream) {
    return plane_score(d_tails, 1, d_table, R, K, S, first_rank, n_ranks, d_colmin_scratch, d_out, stream);
}

int nvrx_tail_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, uint32_t q_ppm, float *d_tail_send, int K, int S,
                    int rows_active, void *stream) {
    hipStream_t st = as_stream(stream);
    LocalWindow w;
    int rc = local_window(ctx, desc, d_tail_send, K, S, rows_active, [&] { return tail_q_check(q_ppm); }, nullptr, &st, &w);
    if (rc) return rc;
    QuantArgs a{};
    window_args(w, &a);
    a.out = d_tail_send;
    a.KS = K + S;
    a.q_ppm = q_ppm;
    const size_t slots = (size_t)ctx->local_ranks * (size_t)a.KS;
    if (slots == 0) return NVRX_OK;
    rc = fill_minus_one(d_tail_send, slots, st);
    if (rc) return rc;
    return quantile_launch(a, ctx->local_ranks * w.rows_active, st);
}

}  // extern "C"
