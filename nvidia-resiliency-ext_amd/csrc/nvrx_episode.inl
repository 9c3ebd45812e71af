// nvrx_episode.inl -- episode scores: the one contiguous stretch of every ring row, in TIME order, that spent most time above
// the row's mean, and relative scores built from its excess.  Part of the translation unit nvrx_straggler.hip (included at its
// end: it uses that file's DPP scans and sums and its context, and nvrx_tail.inl's score kernel).
//
// Onset scores find a rank that became slow and stayed slow, period scores one that stalls on a beat.  Neither sees a rank
// that was slow for one stretch and then recovered (a thermal excursion, a neighbour's checkpoint, a link that flapped).
// k_row_episode finds, per row, the interval [a, b) with at least m samples of "normal" either side that maximises
// E = (H_b - H_a) / n, H_t = n * C_t - t * T (definition: include/nvrx_straggler.h), the means inside and outside and the
// explained share.
//
// For a fixed b the best a is the one with the smallest H_a among m <= a <= b - m: a running minimum that lags b by m, a
// dependency across the whole row.  k_row_episode: one workgroup per ring row; every wave owns a contiguous span of the time
// axis, walked in blocks of 256 samples (64 lanes x 4).
//   pass A  as k_row_onset: coalesced 16-byte loads, pivoted span sums, ONE barrier -> every wave's offset and the total T;
//   pass B  every wave walks its span: an f64 DPP scan gives every t its prefix C_t; the squared deviations are summed; per
//           block the prefix at its start and the smallest H_a over its admissible a (lowest a on ties) go to LDS: at most
//           256 blocks per row; ONE barrier;
//   pass C  every wave walks its span again as b and, in lock-step, a second stream at a = b - m with a scan carry of its own.
//           The carry starts from the block prefix of the block that holds the span's first a plus one partial block (in
//           pass B's own order), the running minimum of H_a from the minimum over the blocks before it plus the same partial
//           block.  A min-scan across the lanes gives every b the smallest H_a it may pair with; every lane keeps its best
//           (E, b, a, C_a, C_b), the first one on ties;
//   end     a lexicographic maximum over (bits of the positive f64 E, ~b, ~a) across the workgroup, as k_row_onset takes
//           its own; thread 0 writes the record.
// Every sum runs in an order fixed by n, m and the time index alone: a row gives the same bits from launch to launch and from
// a rotated ring.  H is evaluated without fused multiply-adds, so that integer-valued samples (exact sums) decide ties as
// the definition does.  No sort, no scratch memory, no global atomic, no float atomic.  A wrapped ring (start != 0) takes the
// same walk with 4-byte loads at (start + i) mod n; the lagged stream is read with 4-byte loads either way (it is aligned
// only where m % 4 == 0).

namespace {

constexpr uint32_t EPISODE_LEN_MIN = 1u, EPISODE_LEN_MAX = 333333u;
constexpr uint32_t EPISODE_MIN_SAMPLES = 8u;
constexpr int EPISODE_PLANES = NVRX_EPISODE_PLANES;  // by gid: {e, inside, outside, strength, length, ago, n}
constexpr int EPISODE_MAX_BLOCKS = NVRX_MAX_RING_CAP / 256;
constexpr uint32_t EPISODE_NONE = 0xFFFFFFFFu;

struct EpisodeArgs {
    const float *samples;
    const uint32_t *counts;
    const uint32_t *starts;  // [rows] slot of the oldest sample; null: 0 everywhere
    const int32_t *gid;      // by-gid mode (null: by row)
    void *out;               // by row: [rows] 16-byte records; by gid: f32 [local_ranks][7][KS]
    int row_stride;
    int uniform_n;  // >= 0: every launched row holds that many samples
    int rows_active, rows_per_rank;  // by-gid mode: the launch covers rows [0, rows_active) of every logical rank
    int KS;                          // ... and a plane of a logical rank has KS slots
    uint32_t min_len_ppm;
    float min_strength;  // by-gid mode: the effective excess counts episodes at least this strong
};

// the effective excess of a record (include/nvrx_straggler.h)
__device__ __forceinline__ float episode_excess(uint32_t len, float inside, float outside, float strength, float min_strength) {
    return (len > 0 && strength >= min_strength && inside > outside && outside > 0.0f) ? (float)((double)inside / (double)outside)
                                                                                       : 1.0f;
}

// H_t = n * C_t - t * T: two rounded products and one rounded difference, never a fused multiply-add
__device__ __forceinline__ double episode_h(double nd, double c, double td, double T) {
#pragma clang fp contract(off)
    const double p = nd * c;
    const double q = td * T;
    return p - q;
}

// a candidate start: H_a, the prefix C_a, and a (EPISODE_NONE: none)
struct EpMin {
    double h, c;
    uint32_t a;
};
__device__ __forceinline__ EpMin ep_none() { return EpMin{INFINITY, 0.0, EPISODE_NONE}; }
// the smaller H, the lower a on ties (NaN never wins)
__device__ __forceinline__ EpMin ep_min(EpMin x, EpMin y) {
    const bool take_y = y.h < x.h || (y.h == x.h && y.a < x.a);
    return EpMin{take_y ? y.h : x.h, take_y ? y.c : x.c, take_y ? y.a : x.a};
}
__device__ __forceinline__ EpMin ep_shfl_up(EpMin x, int delta) {
    return EpMin{__shfl_up(x.h, delta, 64), __shfl_up(x.c, delta, 64), (uint32_t)__shfl_up((int)x.a, delta, 64)};
}
__device__ __forceinline__ EpMin ep_shfl_xor(EpMin x, int mask) {
    return EpMin{__shfl_xor(x.h, mask, 64), __shfl_xor(x.c, mask, 64), (uint32_t)__shfl_xor((int)x.a, mask, 64)};
}
__device__ __forceinline__ EpMin ep_shfl(EpMin x, int src) {
    return EpMin{__shfl(x.h, src, 64), __shfl(x.c, src, 64), (uint32_t)__shfl((int)x.a, src, 64)};
}
// the wave's minimum, in every lane
__device__ __forceinline__ EpMin ep_wave_min(EpMin x) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) x = ep_min(x, ep_shfl_xor(x, s));
    return x;
}
// inclusive minimum over lanes [0, lane]
__device__ __forceinline__ EpMin ep_wave_scan_min(EpMin x, int lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const EpMin y = ep_shfl_up(x, s);
        if (lane >= s) x = ep_min(x, y);
    }
    return x;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_row_episode(EpisodeArgs a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ double s_sum[WAVES];        // pass A: pivoted span sums
    __shared__ double s_sst[WAVES];        // end: sums of squared deviations
    __shared__ double s_ca[WAVES];         // end: the prefixes at the wave's best interval
    __shared__ double s_cb[WAVES];
    __shared__ uint32_t s_best[WAVES][4];  // end: {E high, E low, ~b, ~a}
    __shared__ double s_blk_c[EPISODE_MAX_BLOCKS];    // pass B: the prefix at the block's start
    __shared__ double s_blk_h[EPISODE_MAX_BLOCKS];    // ... the smallest H_a over the block's admissible a
    __shared__ double s_blk_ca[EPISODE_MAX_BLOCKS];   // ... its prefix C_a
    __shared__ uint32_t s_blk_a[EPISODE_MAX_BLOCKS];  // ... and a (EPISODE_NONE: the block holds no admissible a)

    const int tid = threadIdx.x, lane = tid & 63, wave = (int)uni((uint32_t)tid >> 6);
    int row = (int)blockIdx.x;
    float *planes = nullptr;
    if (a.gid) {
        const int lr = (int)blockIdx.x / a.rows_active;
        row = lr * a.rows_per_rank + ((int)blockIdx.x - lr * a.rows_active);
        const int g = a.gid[row];
        if (g < 0 || g >= a.KS) return;  // not exchanged (block-uniform)
        planes = reinterpret_cast<float *>(a.out) + (size_t)lr * EPISODE_PLANES * (size_t)a.KS + g;
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
    uint32_t m = (uint32_t)(((uint64_t)a.min_len_ppm * n + 999999ull) / 1000000ull);
    if (m < EPISODE_MIN_SAMPLES) m = EPISODE_MIN_SAMPLES;
    const int64_t n64 = (int64_t)n, m64 = (int64_t)m;

    const float *__restrict__ src = a.samples + (size_t)row * (size_t)a.row_stride;
    const double pivot = (double)src[start];
    // spans: whole 64-vector steps of four samples per lane, wave w owns vectors [vbase, vend) of the time axis
    const int nvec = (int)((n + 3u) >> 2);  // (row_stride % 4 == 0: all inside the row)
    const int vper = (((nvec + WAVES - 1) / WAVES) + 63) & ~63;
    const int vbase = wave * vper;
    const int vend = min(vbase + vper, nvec);

    // four consecutive samples of the time axis from vector v < vlim, pivoted; 0 behind the row's end
    auto load4 = [&](int v, int vlim, double d[4]) {
        float xs[4] = {0.f, 0.f, 0.f, 0.f};
        if (v < vlim) {
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
        for (int c = 0; c < 4; c++) d[c] = (v < vlim && (uint32_t)(v * 4 + c) < n) ? (double)xs[c] - pivot : 0.0;
    };
    // one sample of the time axis, pivoted (0 <= j < n)
    auto load1 = [&](uint32_t j) {
        uint32_t s = start + j;
        if (s >= n) s -= n;
        return (double)src[s] - pivot;
    };

    // ---- pass A: span sums -> offsets and the row total
    double part = 0.0;
    for (int v = vbase + lane; v < vend; v += 64) {
        double d[4];
        load4(v, vend, d);
        part += ((d[0] + d[1]) + d[2]) + d[3];
    }
    part = wave_sum_f64(part);
    if (lane == 0) s_sum[wave] = part;
    __syncthreads();
    double run0 = 0.0, T = 0.0;  // this wave's exclusive offset; the row total
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const double s = s_sum[w];
        run0 += w < wave ? s : 0.0;
        T += s;
    }
    const double nd = (double)n;
    const double mu = T / nd;

    // ---- pass B: prefixes, squared deviations, per block its starting prefix and the smallest admissible H_a
    double sst = 0.0;
    {
        double run = run0;
        for (int v0 = vbase; v0 < vend; v0 += 64) {  // (wave-uniform bounds)
            const int v = v0 + lane;
            double d[4];
            load4(v, vend, d);
            const double mine = ((d[0] + d[1]) + d[2]) + d[3];
            const double incl = wave_scan_f64(mine);
            double c = run + (incl - mine);
            EpMin best = ep_none();
#pragma unroll
            for (int k = 0; k < 4; k++) {
                c += d[k];
                const uint32_t t = (uint32_t)(v * 4 + k) + 1u;  // c = C_t, the sum of the first t samples
                const bool in_row = v < vend && t <= n;
                const double dev = d[k] - mu;
                sst += in_row ? dev * dev : 0.0;
                if (in_row && t >= m && (int64_t)t + 2 * m64 <= n64) best = ep_min(best, EpMin{episode_h(nd, c, (double)t, T), c, t});
            }
            best = ep_wave_min(best);
            if (lane == 0) {
                const int blk = v0 >> 6;  // (< EPISODE_MAX_BLOCKS: 4 * 64 * blk < n <= NVRX_MAX_RING_CAP)
                s_blk_c[blk] = run, s_blk_h[blk] = best.h, s_blk_ca[blk] = best.c, s_blk_a[blk] = best.a;
            }
            run += wave_last_f64(incl);
        }
    }
    __syncthreads();

    // ---- pass C: b over the span, a = b - m in lock-step
    double best_e = 0.0, best_ca = 0.0, best_cb = 0.0;  // (only E > 0 is an episode)
    uint32_t best_b = 0, best_a = 0;
    if (vbase < vend && n64 >= 3 * m64) {  // (wave-uniform)
        double run = run0;
        double lag = 0.0;          // C at the lagged stream's position
        EpMin low = ep_none();     // the smallest H_a over every admissible a behind the lagged stream's position
        const int64_t j0 = (int64_t)vbase * 4 - m64;  // the first sample of the lagged stream (negative: before the row)
        if (j0 > 0) {
            const int blk = (int)(j0 >> 8);  // the block that holds sample j0 (it exists: j0 < n)
            for (int q = lane; q < blk; q += 64) low = ep_min(low, EpMin{s_blk_h[q], s_blk_ca[q], s_blk_a[q]});
            lag = s_blk_c[blk];
            // the partial block: samples [256 * blk, j0), in pass B's order
            const int v = blk * 64 + lane;
            double d[4];
            load4(v, nvec, d);
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = (int64_t)v * 4 + k < j0 ? d[k] : 0.0;
            const double mine = ((d[0] + d[1]) + d[2]) + d[3];
            const double incl = wave_scan_f64(mine);
            double c = lag + (incl - mine);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                c += d[k];
                const int64_t t = (int64_t)v * 4 + k + 1;
                if (t <= j0 && t >= m64 && t + 2 * m64 <= n64) low = ep_min(low, EpMin{episode_h(nd, c, (double)t, T), c, (uint32_t)t});
            }
            low = ep_wave_min(low);
            lag += wave_last_f64(incl);
        }
        for (int v0 = vbase; v0 < vend; v0 += 64) {  // (wave-uniform bounds)
            const int v = v0 + lane;
            double d[4], da[4];
            load4(v, vend, d);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int64_t i = (int64_t)v * 4 + k, j = i - m64;
                da[k] = (v < vend && i < n64 && j >= 0) ? load1((uint32_t)j) : 0.0;
            }
            const double mine = ((d[0] + d[1]) + d[2]) + d[3];
            const double incl = wave_scan_f64(mine);
            const double minea = ((da[0] + da[1]) + da[2]) + da[3];
            const double incla = wave_scan_f64(minea);
            // the lagged stream: every lane's progressive minima over its own four a, then the lanes before it
            double ca = lag + (incla - minea);
            EpMin lm[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                ca += da[k];
                const int64_t ta = (int64_t)v * 4 + k + 1 - m64;  // ca = C_ta
                const bool ok = v < vend && ta >= m64 && ta + 2 * m64 <= n64;
                const EpMin cand = ok ? EpMin{episode_h(nd, ca, (double)ta, T), ca, (uint32_t)ta} : ep_none();
                lm[k] = k ? ep_min(lm[k - 1], cand) : cand;
            }
            const EpMin scan = ep_wave_scan_min(lm[3], lane);
            EpMin before = ep_shfl_up(scan, 1);
            if (lane == 0) before = ep_none();
            before = ep_min(low, before);
            double cb = run + (incl - mine);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                cb += d[k];
                const int64_t tb = (int64_t)v * 4 + k + 1;  // cb = C_tb
                const EpMin cur = ep_min(before, lm[k]);   // the best a in [m, tb - m]
                if (v < vend && tb + m64 <= n64 && cur.a != EPISODE_NONE) {
                    const double e = (episode_h(nd, cb, (double)tb, T) - cur.h) / nd;
                    if (e > best_e) best_e = e, best_b = (uint32_t)tb, best_a = cur.a, best_ca = cur.c, best_cb = cb;  // (ascending b: the first of equals stays)
                }
            }
            low = ep_min(low, ep_shfl(scan, 63));
            lag += wave_last_f64(incla);
            run += wave_last_f64(incl);
        }
    }

    // ---- end: the workgroup's best interval, lexicographic over (E's bits, ~b, ~a); all 0 = no candidate
    const bool have = best_e > 0.0;
    const uint64_t key = have ? (uint64_t)__double_as_longlong(best_e) : 0ull;
    const uint32_t kh = (uint32_t)(key >> 32), kl = (uint32_t)key, kb = have ? ~best_b : 0u, ka = have ? ~best_a : 0u;
    const uint32_t mh = wave_max_u32(kh);
    const uint32_t ml = wave_max_u32(kh == mh ? kl : 0u);
    const uint32_t mb = wave_max_u32((kh == mh && kl == ml) ? kb : 0u);
    const uint32_t ma = wave_max_u32((kh == mh && kl == ml && kb == mb) ? ka : 0u);
    sst = wave_sum_f64(sst);
    if (kh == mh && kl == ml && kb == mb && ka == ma) s_ca[wave] = best_ca, s_cb[wave] = best_cb;  // (one lane, or lanes that all hold 0.0)
    if (lane == 0) {
        s_best[wave][0] = mh, s_best[wave][1] = ml, s_best[wave][2] = mb, s_best[wave][3] = ma;
        s_sst[wave] = sst;
    }
    __syncthreads();
    if (tid != 0) return;
    uint32_t ph = 0, pl = 0, pb = 0, pa = 0;
    double Ca = 0.0, Cb = 0.0, SST = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        const uint32_t h = s_best[w][0], l = s_best[w][1], b = s_best[w][2], x = s_best[w][3];
        if (h > ph || (h == ph && (l > pl || (l == pl && (b > pb || (b == pb && x > pa)))))) ph = h, pl = l, pb = b, pa = x, Ca = s_ca[w], Cb = s_cb[w];
        SST += s_sst[w];
    }
    const float NaN = __builtin_nanf("");
    uint32_t ago = 0, len = 0;
    float inside, outside, strength;
    if (!(fabs(T) < INFINITY) || !(SST < INFINITY)) {  // (SST >= 0 or NaN)
        inside = outside = strength = NaN;
    } else if ((ph | pl) == 0) {  // n < 3m, or no interval above the row's mean: the row has samples and no episode
        inside = outside = (float)(pivot + mu), strength = 0.0f;
    } else if (SST == 0.0) {  // (a constant row has E = 0 everywhere: kept for the definition's table)
        inside = outside = (float)pivot, strength = 0.0f;
    } else {
        const uint32_t tb = ~pb, ta = ~pa;
        const double E = __longlong_as_double((long long)(((uint64_t)ph << 32) | pl));
        const double L = (double)(tb - ta), in_sum = Cb - Ca;
        len = tb - ta, ago = n - tb;
        inside = (float)(pivot + in_sum / L);
        outside = (float)(pivot + (T - in_sum) / (nd - L));
        strength = (float)(E * E * nd / (L * (nd - L)) / SST);
    }
    if (planes) {
        const size_t KS = (size_t)a.KS;
        planes[0] = episode_excess(len, inside, outside, strength, a.min_strength);
        planes[KS] = inside;
        planes[2 * KS] = outside;
        planes[3 * KS] = strength;
        planes[4 * KS] = (float)len;
        planes[5 * KS] = (float)ago;
        planes[6 * KS] = (float)n;
    } else {
        reinterpret_cast<uint4 *>(a.out)[row] =
            make_uint4(ago | (len << 16), __float_as_uint(inside), __float_as_uint(outside), __float_as_uint(strength));
    }
}

int episode_launch(const EpisodeArgs &a, int blocks, hipStream_t st) {
    if (blocks == 0) return NVRX_OK;
    if (a.row_stride <= 256 * 4 * 4)
        hipLaunchKernelGGL(k_row_episode<256>, dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL(k_row_episode<1024>, dim3(blocks), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

int episode_len_check(uint32_t min_len_ppm) {
    if (min_len_ppm < EPISODE_LEN_MIN || min_len_ppm > EPISODE_LEN_MAX)
        return fail(NVRX_ERR_RANGE, "min_len_ppm=%u outside [%u,%u]", min_len_ppm, EPISODE_LEN_MIN, EPISODE_LEN_MAX);
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_row_episode(const float *d_samples, const uint32_t *d_counts, const uint32_t *d_starts, int rows, int row_stride,
                     uint32_t min_len_ppm, void *d_out, void *stream) {
    const int rc = row_op_check(rows, row_stride, d_samples, d_counts, d_out, true, [&] { return episode_len_check(min_len_ppm); });
    if (rc || rows == 0) return rc;
    EpisodeArgs a{};
    a.samples = d_samples, a.counts = d_counts, a.starts = d_starts, a.out = d_out;
    a.row_stride = row_stride, a.uniform_n = -1, a.min_len_ppm = min_len_ppm;
    return episode_launch(a, rows, as_stream(stream));
}

int nvrx_episode_score(const float *d_episode, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                       float *d_colmin_scratch, float *d_out, void *stream) {
    // plane 0 (the effective excesses) of a [R][7][KS] table
    return plane_score(d_episode, EPISODE_PLANES, d_table, R, K, S, first_rank, n_ranks, d_colmin_scratch, d_out, stream);
}

int nvrx_episode_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, uint32_t min_len_ppm, float min_strength,
                       float *d_episode_send, int K, int S, int rows_active, void *stream) {
    hipStream_t st = as_stream(stream);
    LocalWindow w;
    int rc = local_window(ctx, desc, d_episode_send, K, S, rows_active, [&] {
        const int bad = episode_len_check(min_len_ppm);
        return bad ? bad : min_strength_check(min_strength);
    }, STARTS_OFF, &st, &w);
    if (rc) return rc;
    EpisodeArgs a{};
    window_args(w, &a);
    a.starts = w.starts;
    a.out = d_episode_send;
    a.KS = K + S;
    a.min_len_ppm = min_len_ppm;
    a.min_strength = min_strength;
    const size_t slots = (size_t)ctx->local_ranks * EPISODE_PLANES * (size_t)a.KS;
    if (slots == 0) return NVRX_OK;
    rc = fill_minus_one(d_episode_send, slots, st);
    if (rc) return rc;
    return episode_launch(a, ctx->local_ranks * w.rows_active, st);
}

}  // extern "C"
