// nvrx_ramp.inl -- ramp scores: the least-squares hinge of every ring row in TIME order (flat up to a knot, linear from there
// to the window's end), and relative scores built from the rise it finds.  Part of the translation unit nvrx_straggler.hip
// (included behind nvrx_episode.inl: it uses that file's DPP scans and sums and its context, nvrx_rowfam.inl's host side,
// nvrx_onset.inl's segment check and nvrx_tail.inl's score kernel).
//
// Onset scores fit one step, period scores a beat, episode scores one stretch that recovers.  None of them models a row that
// KEEPS GETTING SLOWER (a card heating up, an allocator fragmenting, a link retraining down): a step fitted to a ramp puts its
// `after` at the ramp's mean, not at where the row has got to.  k_row_ramp finds, per row, the knot t* of the model
// d_i ~ a + b * max(0, i - t) that explains most of the row's variance (definition: include/nvrx_straggler.h), where the row
// stood before the rise, where it stands at the window's end, and the explained share.
//
// With the prefixes C_t = sum_{i<t} d_i and V_t = sum_{i<t} i * d_i, the cross moment of the hinge at knot t is
// (W - V_t) - t * (T - C_t), and the hinge's own first and second moments are closed forms of L = n - t: every knot costs O(1).
//
// k_row_ramp<THREADS, STAGE>: one workgroup per ring row; every wave owns a contiguous span of the time axis.
//   pass A  coalesced 16-byte loads; f64 sums of the span's pivoted samples d and of i * d (wave_sum_f64), one LDS word pair
//           per wave and sum; the same loads are stored to LDS as f32 IN TIME ORDER when the row fits the staging buffer
//           (n <= STAGE samples): a wrapped ring (start != 0: 4-byte loads at (start + i) mod n) is un-rotated here, once.
//           ONE barrier gives every wave its two exclusive offsets and the totals T and W;
//   pass B  every wave walks its own span again -- 16-byte LDS reads at unit stride, no modulo, whatever start was; rows
//           beyond the buffer from the L2 through the same loader as pass A: two f64 DPP scans (wave_scan_f64) per 256-sample
//           step give every sample its C_t and V_t; R_t is evaluated at every admissible knot, the sum of (d - T/n)^2 is
//           accumulated, every lane keeps its best knot (first one on ties);
//   end     a lexicographic maximum over (bits of the non-negative f64 R, ~t) across the workgroup, as k_row_onset and
//           k_attribute take theirs; thread 0 recomputes the fit from the winning prefixes, with the closed forms in exact
//           integer-valued f64, and writes the record.
// The staging buffer: STAGE = 4096 samples (16 KB) with 256 threads -- every row of that variant fits -- and 15 360 samples
// (60 KB) with 1024: with the workgroup's bookkeeping words that stays inside 64 KB, two workgroups share a CU's LDS, and
// the default ring of 10 000 samples (40 KB) is fetched from global memory exactly once (worth about 1 % at that size next to
// a second pass from the L2: docs/MEASUREMENTS.md, "Ramp scores" -- the kernel is bound by its f64 arithmetic).
// Every sum runs in an order fixed by n and the time index alone: a row gives the same bits from launch to launch and from a
// rotated ring.  No barrier inside the walk, no sort, no scratch memory, no global atomic, no data-dependent path.

namespace {

constexpr int RAMP_PLANES = NVRX_RAMP_PLANES;  // by gid: {e, base, end, strength, ago, n}
constexpr int RAMP_STAGE_256 = 256 * 4 * 4;    // samples: the longest row the 256-thread variant is launched for
constexpr int RAMP_STAGE_1024 = NVRX_RAMP_LDS_SAMPLES;  // the LDS cut: longer rows take pass B from the L2

struct RampArgs {
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
    float min_strength;  // by-gid mode: the effective rise counts hinges at least this strong
};

// the effective rise of a record (include/nvrx_straggler.h)
__device__ __forceinline__ float ramp_rise(float base, float end, float strength, float min_strength) {
    return (strength >= min_strength && end > base && base > 0.0f) ? (float)((double)end / (double)base) : 1.0f;
}

// the hinge with L rising samples in a row of n: its first moment Sh = sum h and its centred second moment
// Shh_c = sum h^2 - Sh^2 / n, h = 0 .. L - 1 (positive for L >= 2)
struct RampMoments {
    double sh, shh_c;
};
// ... inside the walk: a reciprocal of n and of 6 (a rounding error each, far below the score's tolerance)
__device__ __forceinline__ RampMoments ramp_moments_fast(double Ld, double inv_n) {
    const double lm1 = Ld - 1.0, p = Ld * lm1;
    const double sh = 0.5 * p;
    return RampMoments{sh, p * (2.0 * Ld - 1.0) * (1.0 / 6.0) - sh * sh * inv_n};
}
// ... at the winner: the products are integers below 2^53 and divisible by 2 and 6, so Sh and Shh are exact
__device__ __forceinline__ RampMoments ramp_moments_exact(double Ld, double nd, double *shh) {
    const double lm1 = Ld - 1.0, p = Ld * lm1;
    const double sh = p / 2.0;
    *shh = p * (2.0 * Ld - 1.0) / 6.0;
    return RampMoments{sh, *shh - sh * sh / nd};
}

template <int THREADS, int STAGE>
__global__ __launch_bounds__(THREADS) void k_row_ramp(RampArgs a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ float4 s_x[STAGE / 4];      // the row in time order (rows of at most STAGE samples)
    __shared__ double s_sum[WAVES];        // pass A: pivoted span sums of d
    __shared__ double s_wsum[WAVES];       // ... and of i * d
    __shared__ double s_sst[WAVES];        // end: sums of squared deviations
    __shared__ double s_c[WAVES];          // end: the prefixes C and V at the wave's best knot
    __shared__ double s_v[WAVES];
    __shared__ uint32_t s_best[WAVES][3];  // end: {R high, R low, ~t}

    const int tid = threadIdx.x, lane = tid & 63, wave = (int)uni((uint32_t)tid >> 6);
    int row = (int)blockIdx.x;
    float *planes = nullptr;
    if (a.gid) {
        const int lr = (int)blockIdx.x / a.rows_active;
        row = lr * a.rows_per_rank + ((int)blockIdx.x - lr * a.rows_active);
        const int g = a.gid[row];
        if (g < 0 || g >= a.KS) return;  // not exchanged (block-uniform)
        planes = reinterpret_cast<float *>(a.out) + (size_t)lr * RAMP_PLANES * (size_t)a.KS + g;
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
    const bool wrapped = start != 0;           // block-uniform
    const bool staged = n <= (uint32_t)STAGE;  // block-uniform: the whole row goes through LDS
    uint32_t m = (uint32_t)(((uint64_t)a.min_seg_ppm * n + 999999ull) / 1000000ull);
    if (m < ONSET_MIN_SEG_SAMPLES) m = ONSET_MIN_SEG_SAMPLES;
    const bool fits = n >= 2u * m;  // block-uniform: the row has candidates, t = 0 .. n - m

    const float *__restrict__ src = a.samples + (size_t)row * (size_t)a.row_stride;
    const double pivot = (double)src[start];
    // spans: whole 64-vector steps of four samples per lane, wave w owns vectors [vbase, vend) of the time axis
    const int nvec = (int)((n + 3u) >> 2);  // (row_stride % 4 == 0: all inside the row; staged: nvec <= STAGE / 4)
    const int vper = (((nvec + WAVES - 1) / WAVES) + 63) & ~63;
    const int vbase = wave * vper;
    const int vend = min(vbase + vper, nvec);

    // the four samples of the time axis in vector v < vend, as the ring holds them
    auto load_ring = [&](int v) {
        if (!wrapped) return reinterpret_cast<const float4 *>(src)[v];
        float xs[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint32_t i = (uint32_t)(v * 4 + c);
            uint32_t s = start + i;  // (< 2n <= 2^17)
            if (s >= n) s -= n;
            xs[c] = i < n ? src[s] : 0.f;
        }
        return make_float4(xs[0], xs[1], xs[2], xs[3]);
    };
    // pivoted, with the index weights: d[c] and w[c] = i * d[c]; 0 behind the span's and the row's end
    auto pivoted = [&](int v, float4 x, double d[4], double w[4]) {
        const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint32_t i = (uint32_t)(v * 4 + c);
            d[c] = (v < vend && i < n) ? (double)xs[c] - pivot : 0.0;
            w[c] = (double)i * d[c];
        }
    };

    // ---- pass A: span sums of d and i * d -> offsets and the row totals; the row goes to LDS in time order
    double part_c = 0.0, part_v = 0.0;
    for (int v = vbase + lane; v < vend; v += 64) {
        const float4 x = load_ring(v);
        if (staged) s_x[v] = x;
        double d[4], w[4];
        pivoted(v, x, d, w);
        part_c += ((d[0] + d[1]) + d[2]) + d[3];
        part_v += ((w[0] + w[1]) + w[2]) + w[3];
    }
    part_c = wave_sum_f64(part_c);
    part_v = wave_sum_f64(part_v);
    if (lane == 0) s_sum[wave] = part_c, s_wsum[wave] = part_v;
    __syncthreads();
    double run_c = 0.0, run_v = 0.0, T = 0.0, W = 0.0;  // this wave's exclusive offsets; the row totals
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const double sc = s_sum[w], sv = s_wsum[w];
        run_c += w < wave ? sc : 0.0;
        run_v += w < wave ? sv : 0.0;
        T += sc;
        W += sv;
    }
    const double nd = (double)n, inv_n = 1.0 / nd;
    const double mu = T / nd;

    // ---- pass B: both prefixes, R at every admissible knot, squared deviations
    double sst = 0.0, best_r = -1.0, best_c = 0.0, best_v = 0.0;
    uint32_t best_t = 0;
    for (int v0 = vbase; v0 < vend; v0 += 64) {  // (wave-uniform bounds)
        const int v = v0 + lane;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (v < vend) x = staged ? s_x[v] : load_ring(v);
        double d[4], w[4];
        pivoted(v, x, d, w);
        const double mine_c = ((d[0] + d[1]) + d[2]) + d[3];
        const double mine_v = ((w[0] + w[1]) + w[2]) + w[3];
        const double incl_c = wave_scan_f64(mine_c);
        const double incl_v = wave_scan_f64(mine_v);
        double c = run_c + (incl_c - mine_c), vv = run_v + (incl_v - mine_v);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t t = (uint32_t)(v * 4 + k);  // c = C_t, vv = V_t: the sums over the samples before t
            const bool in_row = v < vend && t < n;
            const double dev = d[k] - mu;
            sst += in_row ? dev * dev : 0.0;
            if (in_row && fits && t + m <= n) {
                const double td = (double)t;
                const RampMoments h = ramp_moments_fast(nd - td, inv_n);
                const double shd_c = ((W - vv) - td * (T - c)) - h.sh * mu;
                const double R = (shd_c * shd_c) / h.shh_c;
                if (R > best_r) best_r = R, best_c = c, best_v = vv, best_t = t;  // (ascending t: the first of equals stays; NaN never wins)
            }
            c += d[k];
            vv += w[k];
        }
        run_c += wave_last_f64(incl_c);
        run_v += wave_last_f64(incl_v);
    }

    // ---- end: the workgroup's best knot, lexicographic over (R's bits, ~t); (0, 0, 0) = no candidate (~t != 0: t <= 2^16)
    const bool have = best_r >= 0.0;
    const uint64_t key = have ? (uint64_t)__double_as_longlong(best_r) : 0ull;
    const uint32_t kh = (uint32_t)(key >> 32), kl = (uint32_t)key, ki = have ? ~best_t : 0u;
    const uint32_t mh = wave_max_u32(kh);
    const uint32_t ml = wave_max_u32(kh == mh ? kl : 0u);
    const uint32_t mi = wave_max_u32((kh == mh && kl == ml) ? ki : 0u);
    sst = wave_sum_f64(sst);
    if (kh == mh && kl == ml && ki == mi) s_c[wave] = best_c, s_v[wave] = best_v;  // (one lane, or -- no candidate -- lanes that all hold 0.0)
    if (lane == 0) {
        s_best[wave][0] = mh, s_best[wave][1] = ml, s_best[wave][2] = mi;
        s_sst[wave] = sst;
    }
    __syncthreads();
    if (tid != 0) return;
    uint32_t ph = 0, pl = 0, pi = 0;
    double C = 0.0, V = 0.0, SST = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const uint32_t h = s_best[w][0], l = s_best[w][1], i = s_best[w][2];
        if (h > ph || (h == ph && (l > pl || (l == pl && i > pi)))) ph = h, pl = l, pi = i, C = s_c[w], V = s_v[w];
        SST += s_sst[w];
    }
    const float NaN = __builtin_nanf("");
    uint32_t ago;
    float base, end, strength;
    if (!(fabs(T) < INFINITY) || !(fabs(W) < INFINITY) || !(SST < INFINITY)) {  // (SST >= 0 or NaN)
        ago = 0, base = end = strength = NaN;
    } else if (pi == 0) {  // n < 2m: the row has samples and no ramp
        ago = 0, base = end = (float)(pivot + mu), strength = 0.0f;
    } else if (SST == 0.0) {  // a constant row: every knot ties at R = 0
        ago = n, base = end = (float)pivot, strength = 0.0f;
    } else {
        const uint32_t t = ~pi;
        const double td = (double)t, Ld = nd - td;
        double shh;
        const RampMoments h = ramp_moments_exact(Ld, nd, &shh);
        const double shd_c = ((W - V) - td * (T - C)) - h.sh * T / nd;
        const double b = shd_c / h.shh_c;
        const double a0 = (T - b * h.sh) / nd;
        const double lo = pivot + a0;
        ago = n - t;
        base = (float)lo;
        end = (float)(lo + b * (Ld - 1.0));
        strength = (float)((shd_c * shd_c) / h.shh_c / SST);
    }
    if (planes) {
        const size_t KS = (size_t)a.KS;
        planes[0] = ramp_rise(base, end, strength, a.min_strength);
        planes[KS] = base;
        planes[2 * KS] = end;
        planes[3 * KS] = strength;
        planes[4 * KS] = (float)ago;
        planes[5 * KS] = (float)n;
    } else {
        reinterpret_cast<uint4 *>(a.out)[row] = make_uint4(ago, __float_as_uint(base), __float_as_uint(end), __float_as_uint(strength));
    }
}

// 256 threads for the rows onset_launch gives 256, 1024 beyond; the staging buffer follows the variant
int ramp_launch(const RampArgs &a, int blocks, hipStream_t st) {
    if (blocks == 0) return NVRX_OK;
    if (a.row_stride <= RAMP_STAGE_256)
        hipLaunchKernelGGL((k_row_ramp<256, RAMP_STAGE_256>), dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_row_ramp<1024, RAMP_STAGE_1024>), dim3(blocks), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_row_ramp(const float *d_samples, const uint32_t *d_counts, const uint32_t *d_starts, int rows, int row_stride,
                  uint32_t min_seg_ppm, void *d_out, void *stream) {
    const int rc = row_op_check(rows, row_stride, d_samples, d_counts, d_out, true, [&] { return onset_seg_check(min_seg_ppm); });
    if (rc || rows == 0) return rc;
    RampArgs a{};
    a.samples = d_samples, a.counts = d_counts, a.starts = d_starts, a.out = d_out;
    a.row_stride = row_stride, a.uniform_n = -1, a.min_seg_ppm = min_seg_ppm;
    return ramp_launch(a, rows, as_stream(stream));
}

int nvrx_ramp_score(const float *d_ramp, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                    float *d_colmin_scratch, float *d_out, void *stream) {
    // plane 0 (the effective rises) of a [R][6][KS] table
    return plane_score(d_ramp, RAMP_PLANES, d_table, R, K, S, first_rank, n_ranks, d_colmin_scratch, d_out, stream);
}

int nvrx_ramp_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, uint32_t min_seg_ppm, float min_strength,
                    float *d_ramp_send, int K, int S, int rows_active, void *stream) {
    hipStream_t st = as_stream(stream);
    LocalWindow w;
    int rc = local_window(ctx, desc, d_ramp_send, K, S, rows_active, [&] {
        const int bad = onset_seg_check(min_seg_ppm);
        return bad ? bad : min_strength_check(min_strength);
    }, STARTS_OFF, &st, &w);
    if (rc) return rc;
    RampArgs a{};
    window_args(w, &a);
    a.starts = w.starts;
    a.out = d_ramp_send;
    a.KS = K + S;
    a.min_seg_ppm = min_seg_ppm;
    a.min_strength = min_strength;
    const size_t slots = (size_t)ctx->local_ranks * RAMP_PLANES * (size_t)a.KS;
    if (slots == 0) return NVRX_OK;
    rc = fill_minus_one(d_ramp_send, slots, st);
    if (rc) return rc;
    return ramp_launch(a, ctx->local_ranks * w.rows_active, st);
}

}  // extern "C"
