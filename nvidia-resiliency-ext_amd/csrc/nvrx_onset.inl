// nvrx_onset.inl -- onset scores: the least-squares single change point of every ring row in TIME order, and relative
// scores built from the shift it finds.  Part of the translation unit nvrx_straggler.hip (included at its end: it uses that
// file's DPP scans and sums, column-minimum kernels and context, and nvrx_tail.inl's score kernel).
//
// Medians, tails and robust scores are order statistics: none of them looks at the order of the samples, so none can say
// SINCE WHEN a rank is slow.  k_row_onset finds, per row, the split t* of the time axis that explains most of the row's
// variance by one step (definition: include/nvrx_straggler.h), the means on both sides and the explained share.
//
// k_row_onset: one workgroup per ring row; every wave owns a contiguous span of the time axis.
//   pass A  coalesced 16-byte loads, f64 sums of the span's samples pivoted on the row's first one (wave_sum_f64), one LDS
//           word pair per wave; ONE barrier gives every wave its exclusive offset and the row total T;
//   pass B  every wave walks its own span again (from the L2): an f64 DPP scan (wave_scan_f64) over the lanes' four-sample
//           sums gives every sample its prefix C_t, D_t = (t*T - n*C_t)^2 / (n * t * (n - t)) is evaluated where
//           m <= t <= n - m, the sum of (d - T/n)^2 is accumulated, every lane keeps its best split (first one on ties);
//   end     a lexicographic maximum over (bits of the non-negative f64 D, ~t) across the workgroup, as k_attribute takes
//           its maxima; thread 0 writes the record.
// No barrier inside the walk, no sort, no scratch memory, no global atomic, no data-dependent path.  A wrapped ring
// (start != 0: the window was longer than the ring) takes the same walk with 4-byte loads at (start + i) mod n.

namespace {

constexpr uint32_t ONSET_SEG_MIN = 1u, ONSET_SEG_MAX = 500000u;
constexpr uint32_t ONSET_MIN_SEG_SAMPLES = 8u;
constexpr int ONSET_PLANES = NVRX_ONSET_PLANES;  // by gid: {e, before, after, strength, ago, n}

struct OnsetArgs {
    const float *samples;
    const uint32_t *counts;
    const uint32_t *starts;  // [rows] slot of the oldest sample; null: 0 everywhere
    const int32_t *gid;      // by-gid mode (null: by row)
    void *out;               // by row: [rows] 16-byte records; by gid: f32 [local_ranks][6][KS]
    int row_stride;
    int uniform_n;  // >= 0: every launched row holds that many samples
    int rows_active, rows_per_rank;  // by-gid mode: the launch covers rows [0, rows_active) of every logical rank
    int KS;                          // ... and a plane of a logical rank has KS slots
    uint32_t min_seg_ppm;
    float min_strength;  // by-gid mode: the effective shift counts steps at least this strong
};

// the effective shift of a record (include/nvrx_straggler.h)
__device__ __forceinline__ float onset_shift(float before, float after, float strength, float min_strength) {
    return (strength >= min_strength && after > before && before > 0.0f) ? (float)((double)after / (double)before) : 1.0f;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_row_onset(OnsetArgs a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ double s_sum[WAVES];     // pass A: pivoted span sums
    __shared__ double s_sst[WAVES];     // end: sums of squared deviations
    __shared__ double s_c[WAVES];       // end: the prefix at the wave's best split
    __shared__ uint32_t s_best[WAVES][3];  // end: {D high, D low, ~t}

    const int tid = threadIdx.x, lane = tid & 63, wave = (int)uni((uint32_t)tid >> 6);
    int row = (int)blockIdx.x;
    float *planes = nullptr;
    if (a.gid) {
        const int lr = (int)blockIdx.x / a.rows_active;
        row = lr * a.rows_per_rank + ((int)blockIdx.x - lr * a.rows_active);
        const int g = a.gid[row];
        if (g < 0 || g >= a.KS) return;  // not exchanged (block-uniform)
        planes = reinterpret_cast<float *>(a.out) + (size_t)lr * ONSET_PLANES * (size_t)a.KS + g;
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
    const bool wrapped = start != 0;  // block-uniform
    uint32_t m = (uint32_t)(((uint64_t)a.min_seg_ppm * n + 999999ull) / 1000000ull);
    if (m < ONSET_MIN_SEG_SAMPLES) m = ONSET_MIN_SEG_SAMPLES;

    const float *__restrict__ src = a.samples + (size_t)row * (size_t)a.row_stride;
    const double pivot = (double)src[start];
    // spans: whole 64-vector steps of four samples per lane, wave w owns vectors [vbase, vend) of the time axis
    const int nvec = (int)((n + 3u) >> 2);  // (row_stride % 4 == 0: all inside the row)
    const int vper = (((nvec + WAVES - 1) / WAVES) + 63) & ~63;
    const int vbase = wave * vper;
    const int vend = min(vbase + vper, nvec);

    // four consecutive samples of the time axis from vector v, pivoted; 0 behind the row's end
    auto load4 = [&](int v, double d[4]) {
        float xs[4] = {0.f, 0.f, 0.f, 0.f};
        if (v < vend) {
            if (!wrapped) {
                const float4 x = reinterpret_cast<const float4 *>(src)[v];
                xs[0] = x.x, xs[1] = x.y, xs[2] = x.z, xs[3] = x.w;
            } else {
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t i = (uint32_t)(v * 4 + c);
                    uint32_t s = start + i;  // (< 2n <= 2^17)
                    if (s >= n) s -= n;
                    xs[c] = i < n ? src[s] : 0.f;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; c++) d[c] = (v < vend && (uint32_t)(v * 4 + c) < n) ? (double)xs[c] - pivot : 0.0;
    };

    // ---- pass A: span sums -> offsets and the row total
    double part = 0.0;
    for (int v = vbase + lane; v < vend; v += 64) {
        double d[4];
        load4(v, d);
        part += ((d[0] + d[1]) + d[2]) + d[3];
    }
    part = wave_sum_f64(part);
    if (lane == 0) s_sum[wave] = part;
    __syncthreads();
    double run = 0.0, T = 0.0;  // this wave's exclusive offset; the row total
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const double s = s_sum[w];
        run += w < wave ? s : 0.0;
        T += s;
    }
    const double nd = (double)n;
    const double mu = T / nd;

    // ---- pass B: prefixes, D at every admissible split, squared deviations
    double sst = 0.0, best_d = -1.0, best_c = 0.0;
    uint32_t best_t = 0;
    for (int v0 = vbase; v0 < vend; v0 += 64) {  // (wave-uniform bounds)
        const int v = v0 + lane;
        double d[4];
        load4(v, d);
        const double mine = ((d[0] + d[1]) + d[2]) + d[3];
        const double incl = wave_scan_f64(mine);
        double c = run + (incl - mine);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            c += d[k];
            const uint32_t t = (uint32_t)(v * 4 + k) + 1u;  // c = C_t, the sum of the first t samples
            const bool in_row = v < vend && t <= n;
            const double dev = d[k] - mu;
            sst += in_row ? dev * dev : 0.0;
            if (in_row && t >= m && t + m <= n) {
                const double td = (double)t;
                const double num = td * T - nd * c;
                const double D = (num * num) / (nd * td * (nd - td));
                if (D > best_d) best_d = D, best_c = c, best_t = t;  // (ascending t: the first of equals stays; NaN never wins)
            }
        }
        run += wave_last_f64(incl);
    }

    // ---- end: the workgroup's best split, lexicographic over (D's bits, ~t); (0, 0, 0) = no candidate
    const bool have = best_d >= 0.0;
    const uint64_t key = have ? (uint64_t)__double_as_longlong(best_d) : 0ull;
    const uint32_t kh = (uint32_t)(key >> 32), kl = (uint32_t)key, ki = have ? ~best_t : 0u;
    const uint32_t mh = wave_max_u32(kh);
    const uint32_t ml = wave_max_u32(kh == mh ? kl : 0u);
    const uint32_t mi = wave_max_u32((kh == mh && kl == ml) ? ki : 0u);
    sst = wave_sum_f64(sst);
    if (kh == mh && kl == ml && ki == mi) s_c[wave] = best_c;  // (one lane, or -- no candidate -- lanes that all hold 0.0)
    if (lane == 0) {
        s_best[wave][0] = mh, s_best[wave][1] = ml, s_best[wave][2] = mi;
        s_sst[wave] = sst;
    }
    __syncthreads();
    if (tid != 0) return;
    uint32_t ph = 0, pl = 0, pi = 0;
    double C = 0.0, SST = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const uint32_t h = s_best[w][0], l = s_best[w][1], i = s_best[w][2];
        if (h > ph || (h == ph && (l > pl || (l == pl && i > pi)))) ph = h, pl = l, pi = i, C = s_c[w];
        SST += s_sst[w];
    }
    const float NaN = __builtin_nanf("");
    uint32_t ago;
    float before, after, strength;
    if (!(fabs(T) < INFINITY) || !(SST < INFINITY)) {  // (SST >= 0 or NaN)
        ago = 0, before = after = strength = NaN;
    } else if (pi == 0) {  // n < 2m: the row has samples and no onset
        ago = 0, before = after = (float)(pivot + mu), strength = 0.0f;
    } else if (SST == 0.0) {  // a constant row: every split ties at D = 0
        ago = n - m, before = after = (float)pivot, strength = 0.0f;
    } else {
        const uint32_t t = ~pi;
        const double D = __longlong_as_double((long long)(((uint64_t)ph << 32) | pl));
        ago = n - t;
        before = (float)(pivot + C / (double)t);
        after = (float)(pivot + (T - C) / (double)(n - t));
        strength = (float)(D / SST);
    }
    if (planes) {
        const size_t KS = (size_t)a.KS;
        planes[0] = onset_shift(before, after, strength, a.min_strength);
        planes[KS] = before;
        planes[2 * KS] = after;
        planes[3 * KS] = strength;
        planes[4 * KS] = (float)ago;
        planes[5 * KS] = (float)n;
    } else {
        reinterpret_cast<uint4 *>(a.out)[row] = make_uint4(ago, __float_as_uint(before), __float_as_uint(after), __float_as_uint(strength));
    }
}

int onset_launch(const OnsetArgs &a, int blocks, hipStream_t st) {
    if (blocks == 0) return NVRX_OK;
    if (a.row_stride <= 256 * 4 * 4)
        hipLaunchKernelGGL(k_row_onset<256>, dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_row_onset<1024>, dim3(blocks), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

int onset_seg_check(uint32_t min_seg_ppm) {
    if (min_seg_ppm < ONSET_SEG_MIN || min_seg_ppm > ONSET_SEG_MAX)
        return fail(NVRX_ERR_RANGE, "min_seg_ppm=%u outside [%u,%u]", min_seg_ppm, ONSET_SEG_MIN, ONSET_SEG_MAX);
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_row_onset(const float *d_samples, const uint32_t *d_counts, const uint32_t *d_starts, int rows, int row_stride,
                   uint32_t min_seg_ppm, void *d_out, void *stream) {
    const int rc = row_op_check(rows, row_stride, d_samples, d_counts, d_out, true, [&] { return onset_seg_check(min_seg_ppm); });
    if (rc || rows == 0) return rc;
    OnsetArgs a{};
    a.samples = d_samples, a.counts = d_counts, a.starts = d_starts, a.out = d_out;
    a.row_stride = row_stride, a.uniform_n = -1, a.min_seg_ppm = min_seg_ppm;
    return onset_launch(a, rows, as_stream(stream));
}

int nvrx_onset_score(const float *d_onset, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                     float *d_colmin_scratch, float *d_out, void *stream) {
    // plane 0 (the effective shifts) of a [R][6][KS] table
    return plane_score(d_onset, ONSET_PLANES, d_table, R, K, S, first_rank, n_ranks, d_colmin_scratch, d_out, stream);
}

int nvrx_onset_enable(nvrx_ctx *ctx, int on) {
    if (!ctx) return fail(NVRX_ERR_INVALID, "ctx is null");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (on && !ctx->h_onset_starts) {
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ctx->h_onset_starts), (size_t)ctx->rows * sizeof(uint32_t), hipHostMallocDefault));
        memset(ctx->h_onset_starts, 0, (size_t)ctx->rows * sizeof(uint32_t));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->d_onset_starts), (size_t)ctx->rows * sizeof(uint32_t)));
    }
    ctx->onset_on = on != 0;
    ctx->onset_rows = 0, ctx->onset_wrapped = false;
    return NVRX_OK;
}

int nvrx_onset_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, uint32_t min_seg_ppm, float min_strength,
                     float *d_onset_send, int K, int S, int rows_active, void *stream) {
    hipStream_t st = as_stream(stream);
    LocalWindow w;
    int rc = local_window(ctx, desc, d_onset_send, K, S, rows_active, [&] {
        const int bad = onset_seg_check(min_seg_ppm);
        return bad ? bad : min_strength_check(min_strength);
    }, "onset scores are not enabled on this context (nvrx_onset_enable)", &st, &w);
    if (rc) return rc;
    OnsetArgs a{};
    window_args(w, &a);
    a.starts = w.starts;
    a.out = d_onset_send;
    a.KS = K + S;
    a.min_seg_ppm = min_seg_ppm;
    a.min_strength = min_strength;
    const size_t slots = (size_t)ctx->local_ranks * ONSET_PLANES * (size_t)a.KS;
    if (slots == 0) return NVRX_OK;
    rc = fill_minus_one(d_onset_send, slots, st);
    if (rc) return rc;
    return onset_launch(a, ctx->local_ranks * w.rows_active, st);
}

}  // extern "C"
