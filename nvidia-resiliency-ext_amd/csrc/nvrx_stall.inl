// nvrx_stall.inl -- stall scores: the rare, isolated, large samples of every ring row -- how many events they form in TIME
// order, when the last one hit, and what share of the row's time they cost above its pace -- and relative scores built from
// them.  Part of the translation unit nvrx_straggler.hip (included behind nvrx_ramp.inl: it uses nvrx_tail.inl's histogram
// adds, bin count and score kernel, nvrx_rowfam.inl's host side, and the main file's key maps and DPP reductions).
//
// Every other row family fits ONE shape to a row (a quantile, a step, a beat, a stretch, a hinge).  Ten samples of 50 x in a
// window of 10 000 at irregular times move none of them: the median and the 0.95-quantile stay inside the noise, there is no
// step and no period, and the best stretch or hinge explains a few thousandths of the variance -- yet the row lost 4.7 % of
// its window, and in a lockstep job so did every other rank.  k_row_stall takes, per row, the lower median (`pace`) and the lower median of the absolute deviations from it
// (`spread`), cuts at max(pace * ratio, pace + min_z * 1.4826 * spread), and counts what lies above (definition:
// include/nvrx_straggler.h).
//
// k_row_stall<THREADS, STAGE>: one workgroup per ring row.
//   select 1  exact MSB-first radix selection of the lower median over f2key(x), k_row_quantile's three passes (12 + 12 + 8
//             bits into a 4096-bin LDS histogram, wave-aggregated adds: tail_hist_add).  Its FIRST pass is also the only read
//             of the row from device memory when the row fits the staging buffer (n <= STAGE): the 16-byte loads are stored
//             to LDS IN TIME ORDER (a wrapped ring is un-rotated here, once), and every later pass reads LDS;
//   select 2  the same selection over f2key(|x - pace|), the key derived on the fly from the staged sample -- no second array;
//   walk      every wave owns a contiguous span of the time axis (ramp's split) and walks it once, 256 samples a step: four
//             ballots of the stall flags x > cut, one per component of a lane's 16-byte word (sample 4 * lane + c of the step).
//             A run starts where a flag is set and its predecessor's is not: component c's predecessor is component c - 1 of
//             the same lane, component 0's is component 3 of the lane before -- (m3 << 1 | carry), the carry being bit 63 of
//             the step before.  Starts and stall samples are popcounts of those masks: scalar work.  Every lane keeps f64
//             partial sums of x and of x - pace over its stall samples and the newest stall index; wave_sum_f64 and a wave
//             maximum close the span;
//   end       ONE barrier; every wave has left {starts with a carry of 0, stall samples, newest, flag of its first and of its
//             last sample, two sums} in LDS, and thread 0 joins the spans in wave order: a span whose first sample continues
//             the run that ended the span before gives one start back.
// Rows beyond STAGE (up to NVRX_MAX_RING_CAP) take every pass from the L2: the selections in slot order (a histogram does not
// care), the walk in time order.
// LDS: the histogram is 16 KB whatever the row; a workgroup's static LDS ends at 64 KB; the per-wave words and the selection's
// bookkeeping take 584 bytes with 16 waves.  STAGE = 12 032 samples (47 KB, 47 steps of 256) leaves 440 bytes spare and holds
// the default ring of 10 000 samples; with 256 threads STAGE = 4096: every row of that variant fits.
// Order of the sums: a sample's lane, step and wave follow from n and its TIME index alone, so a row gives the same bits --
// every field, both f64 sums included -- from launch to launch and from a rotated ring: the order does not depend on `start`.
// No scratch memory, no global atomic, no data-dependent path through the barriers.

namespace {

constexpr int STALL_PLANES = NVRX_STALL_PLANES;  // by gid: {e, pace, level, share, events, last_ago, n}
constexpr int STALL_STAGE_256 = 256 * 4 * 4;     // samples: the longest row the 256-thread variant is launched for
constexpr int STALL_STAGE_1024 = NVRX_STALL_LDS_SAMPLES;  // the LDS cut: longer rows are re-read from the L2
constexpr uint32_t STALL_RATIO_MIN = 1000001u, STALL_RATIO_MAX = 1000000000u;
static_assert(STALL_STAGE_1024 % 256 == 0 && STALL_STAGE_1024 * 4 + TAIL_BINS * 4 + 1024 <= 65536, "staging + histogram + bookkeeping within 64 KB");

struct StallArgs {
    const float *samples;
    const uint32_t *counts;
    const uint32_t *starts;  // [rows] slot of the oldest sample; null: 0 everywhere
    const int32_t *gid;      // by-gid mode (null: by row)
    void *out;               // by row: [rows] 32-byte records; by gid: f32 [local_ranks][7][KS]
    int row_stride;
    int uniform_n;  // >= 0: every launched row holds that many samples
    int rows_active, rows_per_rank;  // by-gid mode: the launch covers rows [0, rows_active) of every logical rank
    int KS;                          // ... and a plane of a logical rank has KS slots
    uint32_t ratio_ppm;
    float min_z;
    float min_share;  // by-gid mode: the effective excess counts rows whose stalls cost at least this share
};

// the effective excess of a record (include/nvrx_straggler.h)
__device__ __forceinline__ float stall_excess(uint32_t events, float pace, float level, float share, float min_share) {
    return (events >= 1u && share >= min_share && level > pace && pace > 0.0f) ? (float)((double)level / (double)pace) : 1.0f;
}

// The key of rank k among the n keys that keys(v, pass, key[4]) hands out for the 16-byte words v < nvec: k_row_quantile's
// three passes.  Every thread asks for the same words in every pass.  Four barriers a pass, all of them uniform.
template <int THREADS, class Keys>
__device__ __forceinline__ uint32_t stall_select(uint32_t *s_hist, uint32_t *s_wave, uint32_t *s_sel, int nvec, uint32_t n,
                                                 uint32_t k, Keys keys) {
    constexpr int WAVES = THREADS / 64;
    constexpr int PER = TAIL_BINS / THREADS;  // consecutive bins summed per thread
    static_assert(PER % 4 == 0, "a thread's bins are read as 16-byte words");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
            uint32_t key[4];
            keys(v, pass, key);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const bool on = (uint32_t)(v * 4 + c) < n && (up == 32 || (key[c] >> up) == prefix);
                tail_hist_add(s_hist, (key[c] >> shift) & bmask, on);
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
        // (s_sel and s_wave are rewritten only behind the next pass' two barriers -- the next selection's included)
    }
    return prefix;
}

template <int THREADS, int STAGE>
__global__ __launch_bounds__(THREADS) void k_row_stall(StallArgs a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ float4 s_x[STAGE / 4];  // the row in time order (rows of at most STAGE samples)
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[TAIL_BINS];
    __shared__ uint32_t s_wave[WAVES];
    __shared__ uint32_t s_sel[2];
    __shared__ double s_t[WAVES];         // end: span sums of x
    __shared__ double s_lost[WAVES];      // ... and of x - pace over the span's stall samples
    __shared__ uint32_t s_cnt[WAVES][4];  // ... {run starts with a carry of 0, stall samples, newest stall index + 1, edge flags}

    const int tid = threadIdx.x, lane = tid & 63, wave = (int)uni((uint32_t)tid >> 6);
    int row = (int)blockIdx.x;
    float *planes = nullptr;
    if (a.gid) {
        const int lr = (int)blockIdx.x / a.rows_active;
        row = lr * a.rows_per_rank + ((int)blockIdx.x - lr * a.rows_active);
        const int g = a.gid[row];
        if (g < 0 || g >= a.KS) return;  // not exchanged (block-uniform)
        planes = reinterpret_cast<float *>(a.out) + (size_t)lr * STALL_PLANES * (size_t)a.KS + g;
    }
    uint32_t n = a.uniform_n >= 0 ? (uint32_t)a.uniform_n : a.counts[row];
    if (n > (uint32_t)a.row_stride) n = (uint32_t)a.row_stride;
    if (n == 0) {  // block-uniform; by gid the slots keep the -1.0 of the fill ahead of this kernel
        if (!a.gid && tid == 0) {
            const uint32_t m1 = __float_as_uint(-1.0f);
            reinterpret_cast<uint4 *>(a.out)[2 * row] = make_uint4(0u, 0u, 0u, m1);
            reinterpret_cast<uint4 *>(a.out)[2 * row + 1] = make_uint4(m1, m1, m1, m1);
        }
        return;
    }
    uint32_t start = a.starts ? a.starts[row] : 0u;
    if (start >= n) start %= n;
    const bool wrapped = start != 0;           // block-uniform
    const bool staged = n <= (uint32_t)STAGE;  // block-uniform: the whole row goes through LDS

    const float *__restrict__ src = a.samples + (size_t)row * (size_t)a.row_stride;
    const int nvec = (int)((n + 3u) >> 2);  // (row_stride % 4 == 0: all inside the row; staged: nvec <= STAGE / 4)

    // the four samples of the time axis in vector v < nvec, as the ring holds them
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
    // a selection's word v: staged rows from device memory in the very first pass only, in time order, and from LDS ever after;
    // longer rows in slot order (slots [0, n) hold the window whatever start is)
    auto fetch = [&](int v, bool first) {
        if (!staged) return reinterpret_cast<const float4 *>(src)[v];
        if (!first) return s_x[v];
        const float4 x = load_ring(v);
        s_x[v] = x;  // (read back by this thread in the selections, by its span's wave behind their barriers)
        return x;
    };

    // ---- select 1: the pace, the lower median by key order
    const uint32_t k = (uint32_t)((500000ull * n + 999999ull) / 1000000ull) - 1u;
    const float pace = key2f(stall_select<THREADS>(s_hist, s_wave, s_sel, nvec, n, k, [&](int v, int pass, uint32_t key[4]) {
        const float4 x = fetch(v, pass == 0);
        key[0] = f2key(x.x), key[1] = f2key(x.y), key[2] = f2key(x.z), key[3] = f2key(x.w);
    }));
    // ---- select 2: the spread, the lower median of |x - pace| (one rounded f32 subtraction; a NaN sorts to the top)
    const float spread = key2f(stall_select<THREADS>(s_hist, s_wave, s_sel, nvec, n, k, [&](int v, int, uint32_t key[4]) {
        const float4 x = fetch(v, false);
        key[0] = f2key(fabsf(x.x - pace)), key[1] = f2key(fabsf(x.y - pace));
        key[2] = f2key(fabsf(x.z - pace)), key[3] = f2key(fabsf(x.w - pace));
    }));
    // (explicitly rounded products and sum: a contracted multiply-add would round differently from the definition)
    const double pd = (double)pace;
    const float cut = (float)fmax(__ddiv_rn(__dmul_rn(pd, (double)a.ratio_ppm), 1e6),
                                  __dadd_rn(pd, __dmul_rn(__dmul_rn((double)a.min_z, 1.4826), (double)spread)));

    // ---- walk: spans of whole 64-vector steps, wave w owns vectors [vbase, vend) of the time axis
    const int vper = (((nvec + WAVES - 1) / WAVES) + 63) & ~63;
    const int vbase = wave * vper;
    const int vend = min(vbase + vper, nvec);
    double part_t = 0.0, part_l = 0.0;
    uint32_t newest = 0;                                  // per lane: its newest stall's time index + 1
    uint32_t starts = 0, stalls = 0, carry = 0, first = 0;  // wave-uniform
    for (int v0 = vbase; v0 < vend; v0 += 64) {           // (wave-uniform bounds)
        const int v = v0 + lane;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (v < vend) x = staged ? s_x[v] : load_ring(v);
        const float xs[4] = {x.x, x.y, x.z, x.w};
        unsigned long long m[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint32_t i = (uint32_t)(v * 4 + c);
            const bool in_row = v < vend && i < n;
            const bool f = in_row && xs[c] > cut;  // (a NaN sample is never one)
            const double xd = in_row ? (double)xs[c] : 0.0;
            part_t += xd;
            part_l += f ? xd - pd : 0.0;
            newest = f ? i + 1u : newest;  // (ascending i)
            m[c] = __ballot(f);
        }
        if (v0 == vbase) first = (uint32_t)(m[0] & 1ull);
        starts += (uint32_t)(__popcll(m[0] & ~((m[3] << 1) | (unsigned long long)carry)) + __popcll(m[1] & ~m[0]) +
                             __popcll(m[2] & ~m[1]) + __popcll(m[3] & ~m[2]));
        stalls += (uint32_t)(__popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]));
        carry = (uint32_t)(m[3] >> 63);
    }
    // (carry: the flag of the span's last sample where the span is full -- a span cut short by the row's end has no successor)
    part_t = wave_sum_f64(part_t);
    part_l = wave_sum_f64(part_l);
    newest = wave_max_u32(newest);
    if (lane == 0) {
        s_t[wave] = part_t, s_lost[wave] = part_l;
        s_cnt[wave][0] = starts, s_cnt[wave][1] = stalls, s_cnt[wave][2] = newest, s_cnt[wave][3] = first | (carry << 1);
    }
    __syncthreads();
    if (tid != 0) return;

    // ---- end: the spans joined in wave order
    double T = 0.0, lost = 0.0;
    uint32_t events = 0, samples = 0, last = 0, prev = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) {
        T += s_t[w];
        lost += s_lost[w];
        const uint32_t edge = s_cnt[w][3];
        events += s_cnt[w][0] - (edge & prev & 1u);  // its first sample continues the run that ended the span before
        samples += s_cnt[w][1];
        last = max(last, s_cnt[w][2]);
        prev = edge >> 1;
    }
    const float NaN = __builtin_nanf("");
    uint32_t last_ago = 0;
    float r_pace = pace, r_spread = spread, r_cut = cut, level = pace, share = 0.0f;
    if (!(fabs(T) < INFINITY) || !(fabs(lost) < INFINITY)) {
        events = samples = 0;
        r_pace = r_spread = r_cut = level = share = NaN;
    } else if (n < (uint32_t)NVRX_STALL_MIN_SAMPLES || samples == 0) {
        events = samples = 0;
    } else {
        last_ago = n - last;  // (last = the newest stall's time index + 1)
        level = (float)__dadd_rn(pd, __ddiv_rn(lost, (double)samples));
        share = (float)__ddiv_rn(lost, T);
    }
    if (planes) {
        const size_t KS = (size_t)a.KS;
        planes[0] = stall_excess(events, r_pace, level, share, a.min_share);
        planes[KS] = r_pace;
        planes[2 * KS] = level;
        planes[3 * KS] = share;
        planes[4 * KS] = (float)events;
        planes[5 * KS] = (float)last_ago;
        planes[6 * KS] = (float)n;
    } else {
        reinterpret_cast<uint4 *>(a.out)[2 * row] = make_uint4(events, samples, last_ago, __float_as_uint(r_pace));
        reinterpret_cast<uint4 *>(a.out)[2 * row + 1] =
            make_uint4(__float_as_uint(r_spread), __float_as_uint(r_cut), __float_as_uint(level), __float_as_uint(share));
    }
}

// 256 threads for the rows ramp_launch gives 256, 1024 beyond; the staging buffer follows the variant
int stall_launch(const StallArgs &a, int blocks, hipStream_t st) {
    if (blocks == 0) return NVRX_OK;
    if (a.row_stride <= STALL_STAGE_256)
        hipLaunchKernelGGL((k_row_stall<256, STALL_STAGE_256>), dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_row_stall<1024, STALL_STAGE_1024>), dim3(blocks), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

int stall_cut_check(uint32_t ratio_ppm, float min_z) {
    if (ratio_ppm < STALL_RATIO_MIN || ratio_ppm > STALL_RATIO_MAX)
        return fail(NVRX_ERR_RANGE, "ratio_ppm=%u outside [%u,%u]", ratio_ppm, STALL_RATIO_MIN, STALL_RATIO_MAX);
    if (!(min_z >= 0.0f && min_z < INFINITY)) return fail(NVRX_ERR_RANGE, "min_z=%g is not a finite number >= 0", (double)min_z);
    return NVRX_OK;
}

int stall_share_check(float min_share) {
    if (!(min_share >= 0.0f && min_share < 1.0f)) return fail(NVRX_ERR_RANGE, "min_share=%g outside [0,1)", (double)min_share);
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_row_stall(const float *d_samples, const uint32_t *d_counts, const uint32_t *d_starts, int rows, int row_stride,
                   uint32_t ratio_ppm, float min_z, void *d_out, void *stream) {
    const int rc = row_op_check(rows, row_stride, d_samples, d_counts, d_out, true, [&] { return stall_cut_check(ratio_ppm, min_z); });
    if (rc || rows == 0) return rc;
    StallArgs a{};
    a.samples = d_samples, a.counts = d_counts, a.starts = d_starts, a.out = d_out;
    a.row_stride = row_stride, a.uniform_n = -1, a.ratio_ppm = ratio_ppm, a.min_z = min_z;
    return stall_launch(a, rows, as_stream(stream));
}

int nvrx_stall_score(const float *d_stall, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                     float *d_colmin_scratch, float *d_out, void *stream) {
    // plane 0 (the effective excesses) of a [R][7][KS] table
    return plane_score(d_stall, STALL_PLANES, d_table, R, K, S, first_rank, n_ranks, d_colmin_scratch, d_out, stream);
}

int nvrx_stall_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, uint32_t ratio_ppm, float min_z, float min_share,
                     float *d_stall_send, int K, int S, int rows_active, void *stream) {
    hipStream_t st = as_stream(stream);
    LocalWindow w;
    int rc = local_window(ctx, desc, d_stall_send, K, S, rows_active, [&] {
        const int bad = stall_cut_check(ratio_ppm, min_z);
        return bad ? bad : stall_share_check(min_share);
    }, STARTS_OFF, &st, &w);
    if (rc) return rc;
    StallArgs a{};
    window_args(w, &a);
    a.starts = w.starts;
    a.out = d_stall_send;
    a.KS = K + S;
    a.ratio_ppm = ratio_ppm, a.min_z = min_z, a.min_share = min_share;
    const size_t slots = (size_t)ctx->local_ranks * STALL_PLANES * (size_t)a.KS;
    if (slots == 0) return NVRX_OK;
    rc = fill_minus_one(d_stall_send, slots, st);
    if (rc) return rc;
    return stall_launch(a, ctx->local_ranks * w.rows_active, st);
}

}  // extern "C"
