// nvrx_period.inl -- period scores: whether a ring row is slow ON A BEAT (a stall every P-th sample), and relative scores
// built from the excess it finds.  Part of the translation unit nvrx_straggler.hip (included at its end: it uses that file's
// DPP sums and maxima, its fill kernel and context, nvrx_attribute.inl's key map and nvrx_tail.inl's score kernel).
//
// One slow sample in fifty moves no median and no quantile, and a spike train is no step: medians, tails, robust scores and
// onsets cannot see it.  k_row_period folds every row over every candidate period P in [2, Pmax] and keeps, per P, the
// adjusted share a_P of the row's variance that the P phase means explain (definition: include/nvrx_straggler.h).
//
// k_row_period: one workgroup per ring row.
//   stage   the row goes into LDS once, as f32, in TIME order (the ring start leaves the inner loop); the f64 sums of the
//           samples pivoted on the row's first one give T, a second walk over the staged row gives SST.  A row of more than
//           PERIOD_LDS_SAMPLES samples is not staged: every walk below then reads global memory at (start + i) mod n;
//   fold    a wave takes whole periods, round robin (wave w folds P = 2 + w, 2 + w + WAVES, ...: which wave folds a period
//           changes no bit of its result).  For its P, lane f sums d_(f + jP) -- consecutive LDS words across the lanes -- in
//           four interleaved f64 chains, phases in chunks of 64 when P > 64.  n_f takes two values only (n / P, and one more
//           for f < n mod P): S_f^2 is accumulated in-lane into one of two sums, two wave_sum_f64 and two divisions per period;
//   choice  a_P goes into an LDS array; one barrier, a workgroup maximum, a workgroup "lowest P at or above the bar";
//   end     wave 0 folds P* again for the phase with the largest mean; thread 0 writes the record.
// No float atomic, no global atomic, no scratch memory; every sum runs in an order that the row's length and P fix, so a
// row gives the same bits from launch to launch and from a rotated ring.

namespace {

constexpr int PERIOD_PLANES = NVRX_PERIOD_PLANES;  // by gid: {e, peak, rest, strength, period, ago, n}
constexpr uint32_t PERIOD_LDS_SAMPLES = 10240u;    // longest row that is staged in LDS (40 KB of f32)
// LDS of one workgroup, in doubles: the staged row, behind it a_P for P <= n / 4 (or, for a row that is not staged, a_P alone)
constexpr int PERIOD_LDS_BIG = (int)(PERIOD_LDS_SAMPLES / 2 + PERIOD_LDS_SAMPLES / NVRX_PERIOD_MIN_CYCLES + 1);  // 60 KB
constexpr int PERIOD_SMALL_STRIDE = 1024;
constexpr int PERIOD_LDS_SMALL = PERIOD_SMALL_STRIDE / 2 + PERIOD_SMALL_STRIDE / NVRX_PERIOD_MIN_CYCLES + 1;  // 6 KB
static_assert(PERIOD_LDS_BIG >= NVRX_PERIOD_MAX + 1, "a row that is not staged keeps a_P for every P up to NVRX_PERIOD_MAX");

struct PeriodArgs {
    const float *samples;
    const uint32_t *counts;
    const uint32_t *starts;  // [rows] slot of the oldest sample; null: 0 everywhere
    const int32_t *gid;      // by-gid mode (null: by row)
    void *out;               // by row: [rows] 16-byte records; by gid: f32 [local_ranks][7][KS]
    int row_stride;
    int uniform_n;  // >= 0: every launched row holds that many samples
    int rows_active, rows_per_rank;  // by-gid mode: the launch covers rows [0, rows_active) of every logical rank
    int KS;                          // ... and a plane of a logical rank has KS slots
    uint32_t max_period;
    float min_strength;  // by-gid mode: the effective excess counts beats at least this strong
};

// the effective excess of a record (include/nvrx_straggler.h)
__device__ __forceinline__ float period_excess(uint32_t period, float peak, float rest, float strength, float min_strength) {
    return (period > 0u && strength >= min_strength && peak > rest && rest > 0.0f) ? (float)((double)peak / (double)rest) : 1.0f;
}

// the inverse of nvrx_attribute.inl's d2key
__device__ __forceinline__ double key2d(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    return __longlong_as_double((long long)u);
}

// the f64 sum of v over the workgroup, in every thread: lanes by DPP, waves in ascending order
template <int WAVES>
__device__ __forceinline__ double period_block_sum(double v, double *s_red, int wave, int lane) {
    v = wave_sum_f64(v);
    __syncthreads();  // (s_red is free again)
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) t += s_red[w];
    return t;
}

// S_f of phase f at period P: four interleaved chains over d_f, d_(f+P), ... in time order
template <bool STAGED>
__device__ __forceinline__ double period_phase_sum(const float *s_x, const float *__restrict__ src, uint32_t start, uint32_t n,
                                                   double pivot, uint32_t f, uint32_t P) {
    auto d = [&](uint32_t i) -> double {
        if (STAGED) return (double)s_x[i] - pivot;
        uint32_t s = start + i;  // (< 2n <= 2^17)
        if (s >= n) s -= n;
        return (double)src[s] - pivot;
    };
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    uint32_t i = f;
    for (; i + 3u * P < n; i += 4u * P) {
        s0 += d(i);
        s1 += d(i + P);
        s2 += d(i + 2u * P);
        s3 += d(i + 3u * P);
    }
    for (; i < n; i += P) s0 += d(i);
    return (s0 + s1) + (s2 + s3);
}

template <int THREADS, int LDS_DOUBLES>
__global__ __launch_bounds__(THREADS) void k_row_period(PeriodArgs a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ double s_buf[LDS_DOUBLES];  // the staged row (f32), then a_P indexed from the row's end by P
    __shared__ double s_red[WAVES];
    __shared__ uint32_t s_key[WAVES][2];
    __shared__ uint32_t s_min[WAVES];
    __shared__ double s_win[2];            // end: {S_f*, n_f*}
    __shared__ uint32_t s_phase;           // end: f*

    const int tid = threadIdx.x, lane = tid & 63, wave = (int)uni((uint32_t)tid >> 6);
    int row = (int)blockIdx.x;
    float *planes = nullptr;
    if (a.gid) {
        const int lr = (int)blockIdx.x / a.rows_active;
        row = lr * a.rows_per_rank + ((int)blockIdx.x - lr * a.rows_active);
        const int g = a.gid[row];
        if (g < 0 || g >= a.KS) return;  // not exchanged (block-uniform)
        planes = reinterpret_cast<float *>(a.out) + (size_t)lr * PERIOD_PLANES * (size_t)a.KS + g;
    }
    uint32_t n = a.uniform_n >= 0 ? (uint32_t)a.uniform_n : a.counts[row];
    if (n > (uint32_t)a.row_stride) n = (uint32_t)a.row_stride;
    if (n == 0) {  // block-uniform; by gid the slots keep the -1.0 of the fill ahead of this kernel
        if (!a.gid && tid == 0)
            reinterpret_cast<uint4 *>(a.out)[row] = make_uint4(0u, __float_as_uint(-1.0f), __float_as_uint(-1.0f), __float_as_uint(-1.0f));
        return;
    }
    uint32_t start = a.starts ? a.starts[row] : 0u;
    if (start >= n) start %= n;
    uint32_t Pmax = n / (uint32_t)NVRX_PERIOD_MIN_CYCLES;
    if (Pmax > a.max_period) Pmax = a.max_period;
    // block-uniform: a row of the small variant is always staged (n <= row_stride <= PERIOD_SMALL_STRIDE)
    const bool staged = n <= PERIOD_LDS_SAMPLES && (n + 1u) / 2u + Pmax + 1u <= (uint32_t)LDS_DOUBLES;

    const float *__restrict__ src = a.samples + (size_t)row * (size_t)a.row_stride;
    const double pivot = (double)src[start];
    float *s_x = reinterpret_cast<float *>(s_buf);
    double *s_a = staged ? s_buf + (n + 1u) / 2u : s_buf;  // a_P at s_a[P], P <= Pmax

    // ---- stage: the row in time order, T, SST
    double part = 0.0;
    for (uint32_t i = (uint32_t)tid; i < n; i += THREADS) {
        uint32_t s = start + i;
        if (s >= n) s -= n;
        const float x = src[s];
        if (staged) s_x[i] = x;
        part += (double)x - pivot;
    }
    const double T = period_block_sum<WAVES>(part, s_red, wave, lane);  // (its barriers also publish the staged row)
    const double nd = (double)n;
    const double mu = T / nd;
    part = 0.0;
    for (uint32_t i = (uint32_t)tid; i < n; i += THREADS) {
        double d;
        if (staged) {
            d = (double)s_x[i] - pivot;
        } else {
            uint32_t s = start + i;
            if (s >= n) s -= n;
            d = (double)src[s] - pivot;
        }
        const double dev = d - mu;
        part += dev * dev;
    }
    const double SST = period_block_sum<WAVES>(part, s_red, wave, lane);

    const float NaN = __builtin_nanf("");
    uint32_t period = 0, ago = 0;
    float peak, rest, strength;
    bool done = true;  // block-uniform: T and SST are the same bits in every thread
    if (!(fabs(T) < INFINITY) || !(SST < INFINITY)) {  // (SST >= 0 or NaN)
        peak = rest = strength = NaN;
    } else if (Pmax < 2u) {
        peak = rest = (float)(pivot + mu), strength = 0.0f;
    } else if (SST == 0.0) {
        peak = rest = (float)pivot, strength = 0.0f;
    } else {
        done = false;
        peak = rest = (float)(pivot + mu), strength = 0.0f;  // (kept where a_max <= 0)
    }

    if (!done) {
        // ---- fold: whole periods per wave
        for (uint32_t P = 2u + (uint32_t)wave; P <= Pmax; P += WAVES) {  // (wave-uniform bounds)
            const uint32_t more = n % P;  // phases below `more` hold n / P + 1 samples, the others n / P
            double q_hi = 0.0, q_lo = 0.0;
            for (uint32_t c = 0; c < P; c += 64u) {  // (wave-uniform bounds)
                const uint32_t f = c + (uint32_t)lane;
                if (f < P) {
                    const double S = staged ? period_phase_sum<true>(s_x, src, start, n, pivot, f, P)
                                            : period_phase_sum<false>(s_x, src, start, n, pivot, f, P);
                    if (f < more) q_hi += S * S;
                    else q_lo += S * S;
                }
            }
            q_hi = wave_sum_f64(q_hi);
            q_lo = wave_sum_f64(q_lo);
            if (lane == 0) {
                const double k = (double)(n / P);
                const double B = (q_hi / (k + 1.0) + q_lo / k) - T * T / nd;
                s_a[P] = 1.0 - (1.0 - B / SST) * (nd - 1.0) / (nd - (double)P);
            }
        }
        __syncthreads();

        // ---- choice: a_max, then the lowest P at or above the bar
        uint64_t key = 0ull;  // (below every double's key)
        for (uint32_t P = 2u + (uint32_t)tid; P <= Pmax; P += THREADS) {
            const uint64_t k = d2key(s_a[P]);
            key = k > key ? k : key;
        }
        {
            const uint32_t kh = (uint32_t)(key >> 32), kl = (uint32_t)key;
            const uint32_t mh = wave_max_u32(kh);
            const uint32_t ml = wave_max_u32(kh == mh ? kl : 0u);
            if (lane == 0) s_key[wave][0] = mh, s_key[wave][1] = ml;
        }
        __syncthreads();
        key = 0ull;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const uint64_t k = ((uint64_t)s_key[w][0] << 32) | s_key[w][1];
            key = k > key ? k : key;
        }
        const double a_max = key2d(key);
        if (a_max > 0.0) {  // block-uniform
            const double bar = NVRX_PERIOD_BAR * a_max;
            uint32_t low = 0xFFFFFFFFu;
            for (uint32_t P = 2u + (uint32_t)tid; P <= Pmax; P += THREADS)
                if (s_a[P] >= bar) low = min(low, P);
            low = wave_min_u32(low);
            if (lane == 0) s_min[wave] = low;
            __syncthreads();
            low = 0xFFFFFFFFu;
#pragma unroll
            for (int w = 0; w < WAVES; w++) low = min(low, s_min[w]);
            const uint32_t P = low;  // (the period that holds a_max clears the bar: there is one)

            // ---- end: wave 0 folds P* again for the phase with the largest mean, the lowest phase on ties
            if (wave == 0) {
                const uint32_t more = n % P, k = n / P;
                double best_m = 0.0, best_s = 0.0;
                uint32_t best_f = 0xFFFFFFFFu, best_n = 0;
                for (uint32_t c = 0; c < P; c += 64u) {
                    const uint32_t f = c + (uint32_t)lane;
                    if (f < P) {
                        const double S = staged ? period_phase_sum<true>(s_x, src, start, n, pivot, f, P)
                                                : period_phase_sum<false>(s_x, src, start, n, pivot, f, P);
                        const uint32_t nf = k + (f < more ? 1u : 0u);
                        const double m = S / (double)nf;
                        if (best_f == 0xFFFFFFFFu || m > best_m) best_m = m, best_s = S, best_f = f, best_n = nf;  // (ascending f)
                    }
                }
                const bool have = best_f != 0xFFFFFFFFu;
                const uint64_t mk = have ? d2key(best_m) : 0ull;
                const uint32_t kh = (uint32_t)(mk >> 32), kl = (uint32_t)mk, ki = have ? ~best_f : 0u;
                const uint32_t mh = wave_max_u32(kh);
                const uint32_t ml = wave_max_u32(kh == mh ? kl : 0u);
                const uint32_t mi = wave_max_u32((kh == mh && kl == ml) ? ki : 0u);
                if (have && kh == mh && kl == ml && ki == mi) {  // (one lane)
                    s_win[0] = best_s, s_win[1] = (double)best_n;
                    s_phase = best_f;
                }
            }
            __syncthreads();
            if (tid == 0) {
                const double S = s_win[0], nf = s_win[1];
                const uint32_t f = s_phase;
                period = P;
                ago = (n - 1u - f) % P;  // (f < P <= n / 4)
                peak = (float)(pivot + S / nf);
                rest = (float)(pivot + (T - S) / (nd - nf));
                strength = (float)s_a[P];
            }
        }
    }
    if (tid != 0) return;
    if (planes) {
        const size_t KS = (size_t)a.KS;
        planes[0] = period_excess(period, peak, rest, strength, a.min_strength);
        planes[KS] = peak;
        planes[2 * KS] = rest;
        planes[3 * KS] = strength;
        planes[4 * KS] = (float)period;
        planes[5 * KS] = (float)ago;
        planes[6 * KS] = (float)n;
    } else {
        reinterpret_cast<uint4 *>(a.out)[row] =
            make_uint4(period | (ago << 16), __float_as_uint(peak), __float_as_uint(rest), __float_as_uint(strength));
    }
}

int period_launch(const PeriodArgs &a, int blocks, hipStream_t st) {
    if (blocks == 0) return NVRX_OK;
    if (a.row_stride <= PERIOD_SMALL_STRIDE)
        hipLaunchKernelGGL((k_row_period<256, PERIOD_LDS_SMALL>), dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_row_period<1024, PERIOD_LDS_BIG>), dim3(blocks), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

int period_max_check(int max_period) {
    if (max_period < 2 || max_period > NVRX_PERIOD_MAX)
        return fail(NVRX_ERR_RANGE, "max_period=%d outside [2,%d]", max_period, NVRX_PERIOD_MAX);
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_row_period(const float *d_samples, const uint32_t *d_counts, const uint32_t *d_starts, int rows, int row_stride,
                    int max_period, void *d_out, void *stream) {
    const int rc = row_op_check(rows, row_stride, d_samples, d_counts, d_out, true, [&] { return period_max_check(max_period); });
    if (rc || rows == 0) return rc;
    PeriodArgs a{};
    a.samples = d_samples, a.counts = d_counts, a.starts = d_starts, a.out = d_out;
    a.row_stride = row_stride, a.uniform_n = -1, a.max_period = (uint32_t)max_period;
    return period_launch(a, rows, as_stream(stream));
}

int nvrx_period_score(const float *d_period, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                      float *d_colmin_scratch, float *d_out, void *stream) {
    // plane 0 (the effective excesses) of a [R][7][KS] table
    return plane_score(d_period, PERIOD_PLANES, d_table, R, K, S, first_rank, n_ranks, d_colmin_scratch, d_out, stream);
}

int nvrx_period_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, int max_period, float min_strength,
                      float *d_period_send, int K, int S, int rows_active, void *stream) {
    hipStream_t st = as_stream(stream);
    LocalWindow w;
    int rc = local_window(ctx, desc, d_period_send, K, S, rows_active, [&] {
        const int bad = period_max_check(max_period);
        return bad ? bad : min_strength_check(min_strength);
    }, STARTS_OFF, &st, &w);
    if (rc) return rc;
    PeriodArgs a{};
    window_args(w, &a);
    a.starts = w.starts;
    a.out = d_period_send;
    a.KS = K + S;
    a.max_period = (uint32_t)max_period;
    a.min_strength = min_strength;
    const size_t slots = (size_t)ctx->local_ranks * PERIOD_PLANES * (size_t)a.KS;
    if (slots == 0) return NVRX_OK;
    rc = fill_minus_one(d_period_send, slots, st);
    if (rc) return rc;
    return period_launch(a, ctx->local_ranks * w.rows_active, st);
}

}  // extern "C"
