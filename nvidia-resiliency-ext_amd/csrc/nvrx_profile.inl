// nvrx_profile.inl -- tail profile: up to seven nearest-rank quantiles of every ring row selected in ONE launch that reads
// the row from device memory once, and relative scores built from them per quantile.  Part of the translation unit
// nvrx_straggler.hip (included behind nvrx_stall.inl: it uses nvrx_tail.inl's histogram adds, quantile range and score rule,
// nvrx_rowfam.inl's host side, and the main file's key maps, DPP scan and column-minimum kernels).
//
// A tail score (nvrx_tail.inl) answers "is this rank slow at q" for ONE q that the operator had to guess: a rank slower on
// 2 % of its samples is invisible at q = 0.95.  Every further q is a further k_row_quantile launch, three passes over the
// window each.  k_row_profile selects Q targets k_0 <= ... <= k_{Q-1} (the tail's integer formula, so plane j is
// nvrx_row_quantile at q_j bit for bit) together.
//
// k_row_profile<THREADS, STAGE>: one workgroup per ring row, MSB-first radix select in three fixed passes of 12 + 10 + 10 bits.
//   keys      pass one loads the row as 16-byte words, maps them through f2key and keeps the ORDER KEYS in LDS (s_key); passes
//             two and three read LDS.  Rows beyond STAGE keep their first STAGE keys there and take the rest from the L2.
//   pass one  every key's top 12 bits go into one 4096-bin histogram that all targets share; thread sums, a DPP scan and the
//             bin search of k_row_quantile then run once per TARGET on those sums: target j gets its bin and its rank in it.
//   groups    targets that fell into the same bin share a prefix.  Targets ascend, so a group is a run of neighbours, named by
//             its first target (its LEADER) -- no compaction, no dynamic index: slot j of seven is live iff target j leads.
//   pass 2, 3 one sweep over the keys whatever Q is: a key's bits above the pass are compared with the leaders' prefixes
//             (wave-uniform values; distinct, so a key counts at most once) and its next 10 bits are counted into the 1024-bin
//             histogram of the leader it matches.  The scan runs per live histogram, the search per target within its group's.
//   end       after the third pass a target's prefix is its key: always exact, ties and all, no data-dependent path through
//             the barriers, no scratch memory, no global atomic.
// Hot bins: a row's samples share sign, exponent and leading mantissa bits, so pass one piles nearly every key into one or two
// bins; tail_hist_add's wave-aggregated add (agree on the first lane's bin, add the popcount once) serves every pass, on the
// combined index (histogram, bin).
// LDS: seven 1024-bin histograms are 28 KB (pass one's 4096 bins live in the first 16 KB of them); the scan's wave sums are
// 7 x 16 words and the picks 7 x 2; a workgroup's static LDS ends at 64 KB: 65 536 - 28 672 - 448 - 56 = 36 360 bytes = 9090
// keys.  STAGE = 8960 (35 steps of 256) leaves 520 bytes spare.  With 256 threads (rows of at most 4096 samples) every row fits.

namespace {

constexpr int PROFILE_MAX_Q = NVRX_PROFILE_MAX_Q;
constexpr int PROFILE_BINS1 = TAIL_BINS;  // pass one: 12 bits
constexpr int PROFILE_BINS = 1024;        // passes two and three: 10 bits each, per group
constexpr int PROFILE_STAGE_256 = 256 * 4 * 4;  // samples: the longest row the 256-thread variant is launched for
constexpr int PROFILE_STAGE_1024 = NVRX_PROFILE_LDS_SAMPLES;
static_assert(PROFILE_MAX_Q * PROFILE_BINS >= PROFILE_BINS1, "pass one's histogram lives in the groups' histograms");
static_assert(PROFILE_STAGE_1024 % 4 == 0 &&
                  PROFILE_STAGE_1024 * 4 + PROFILE_MAX_Q * PROFILE_BINS * 4 + PROFILE_MAX_Q * (16 + 2) * 4 <= 65536,
              "keys + histograms + bookkeeping within 64 KB");

struct ProfileArgs {
    const float *samples;
    const uint32_t *counts;
    const int32_t *gid;  // by-gid mode (null: by row)
    float *out;          // by row: [Q][rows]; by gid: [local_ranks][Q][KS]
    int row_stride;
    int uniform_n;  // >= 0: every launched row holds that many samples
    int rows_active, rows_per_rank;  // by-gid mode: the launch covers rows [0, rows_active) of every logical rank
    int KS;                          // ... and a plane of a logical rank has KS slots
    int rows;                        // by row: the pitch of a plane
    int Q;
    uint32_t q_ppm[PROFILE_MAX_Q];
};

// Behind a sweep: for every live histogram (slot g < Q with lead[g]) of NB bins at s_hist + g * NB, thread sums -> DPP scan ->
// wave sums; then every target j finds, within the histogram of its group slot[j], the bin that holds its rank k[j] and the
// count of keys below that bin: s_sel[j] = {bin, below}.  Two barriers, both uniform (Q, lead and slot are block-uniform).
template <int THREADS, int NB>
__device__ __forceinline__ void profile_pick(const uint32_t *s_hist, uint32_t *s_wave, uint32_t (*s_sel)[2], int Q,
                                             const bool (&lead)[PROFILE_MAX_Q], const int (&slot)[PROFILE_MAX_Q],
                                             const uint32_t (&k)[PROFILE_MAX_Q]) {
    constexpr int WAVES = THREADS / 64;
    constexpr int PER = NB / THREADS;  // consecutive bins summed per thread
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t mine[PROFILE_MAX_Q], incl[PROFILE_MAX_Q];
#pragma unroll
    for (int g = 0; g < PROFILE_MAX_Q; g++) {
        mine[g] = incl[g] = 0;
        if (g < Q && lead[g]) {
#pragma unroll
            for (int i = 0; i < PER; i++) mine[g] += s_hist[g * NB + tid * PER + i];
            incl[g] = wave_scan_u32(mine[g]);
            if (lane == 63) s_wave[g * WAVES + wave] = incl[g];
        }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < PROFILE_MAX_Q; g++) {
        if (g < Q && lead[g]) {
            uint32_t below = incl[g] - mine[g];
#pragma unroll
            for (int w = 0; w < WAVES; w++) below += w < wave ? s_wave[g * WAVES + w] : 0u;
#pragma unroll
            for (int j = g; j < PROFILE_MAX_Q; j++) {
                // exactly one thread per target (the counts of its group's histogram sum to more than k[j])
                if (j < Q && slot[j] == g && k[j] >= below && k[j] < below + mine[g]) {
                    uint32_t b = 0, acc = below;
                    for (; b < (uint32_t)PER - 1u; b++) {  // the first bin whose end is past k[j]
                        const uint32_t h = s_hist[g * NB + tid * PER + (int)b];
                        if (k[j] < acc + h) break;
                        acc += h;
                    }
                    s_sel[j][0] = (uint32_t)(tid * PER) + b;
                    s_sel[j][1] = acc;
                }
            }
        }
    }
    __syncthreads();
}

template <int THREADS, int STAGE>
__global__ __launch_bounds__(THREADS) void k_row_profile(ProfileArgs a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ uint4 s_key[STAGE / 4];  // the row's first STAGE order keys
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[PROFILE_MAX_Q * PROFILE_BINS];
    __shared__ uint32_t s_wave[PROFILE_MAX_Q * WAVES];
    __shared__ uint32_t s_sel[PROFILE_MAX_Q][2];  // per target {bin holding its rank, keys of its group below that bin}

    const int tid = threadIdx.x;
    const int Q = a.Q;
    int row = (int)blockIdx.x;
    float *dst;
    size_t pitch;  // floats between two planes of this row
    if (a.gid) {
        const int lr = (int)blockIdx.x / a.rows_active;
        row = lr * a.rows_per_rank + ((int)blockIdx.x - lr * a.rows_active);
        const int g = a.gid[row];
        if (g < 0 || g >= a.KS) return;  // not exchanged (block-uniform)
        dst = a.out + (size_t)lr * (size_t)Q * (size_t)a.KS + g;
        pitch = (size_t)a.KS;
    } else {
        dst = a.out + row;
        pitch = (size_t)a.rows;
    }
    uint32_t n = a.uniform_n >= 0 ? (uint32_t)a.uniform_n : a.counts[row];
    if (n > (uint32_t)a.row_stride) n = (uint32_t)a.row_stride;
    if (n == 0) {  // block-uniform; by gid the slots keep the -1.0 of the fill ahead of this kernel
        if (!a.gid && tid < Q) dst[(size_t)tid * pitch] = -1.0f;
        return;
    }

    // per target, block-uniform: its rank within its group, the key bits found so far, whether it leads a group, its group's slot
    uint32_t k[PROFILE_MAX_Q], prefix[PROFILE_MAX_Q];
    bool lead[PROFILE_MAX_Q];
    int slot[PROFILE_MAX_Q];
#pragma unroll
    for (int j = 0; j < PROFILE_MAX_Q; j++) {
        // nearest rank: ceil(q * n) - 1 in integers (the tail's formula)
        k[j] = j < Q ? (uint32_t)(((uint64_t)a.q_ppm[j] * n + 999999ull) / 1000000ull) - 1u : 0u;
        prefix[j] = 0u, lead[j] = j == 0, slot[j] = 0;  // pass one: one group of all targets
    }

    const float4 *__restrict__ src = reinterpret_cast<const float4 *>(a.samples + (size_t)row * (size_t)a.row_stride);
    const int nvec = (int)((n + 3u) >> 2);  // 16-byte words holding a sample (row_stride % 4 == 0: all inside the row)
    auto load_keys = [&](int v) {
        const float4 x = src[v];
        return make_uint4(f2key(x.x), f2key(x.y), f2key(x.z), f2key(x.w));
    };

#pragma unroll 1
    for (int pass = 0; pass < 3; pass++) {
        const int shift = pass == 0 ? 20 : pass == 1 ? 10 : 0;  // this pass bins bits [shift, shift + 12) (10 behind the first)
        const int up = pass == 0 ? 32 : pass == 1 ? 20 : 10;    // bits [up, 32) must equal a leader's prefix
        const uint32_t bmask = pass == 0 ? (uint32_t)PROFILE_BINS1 - 1u : (uint32_t)PROFILE_BINS - 1u;
        const int words = pass == 0 ? PROFILE_BINS1 : Q * PROFILE_BINS;  // (slots [0, Q) are the ones that can lead)
        for (int i = tid; i < words / 4; i += THREADS) reinterpret_cast<uint4 *>(s_hist)[i] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        for (int v = tid; v < nvec; v += THREADS) {
            uint4 kv;
            if (pass == 0) {
                kv = load_keys(v);
                if (v < STAGE / 4) s_key[v] = kv;  // (read back by this very thread in the passes behind)
            } else {
                kv = v < STAGE / 4 ? s_key[v] : load_keys(v);
            }
            const uint32_t key[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                bool on = (uint32_t)(v * 4 + c) < n;
                uint32_t at = (key[c] >> shift) & bmask;
                if (pass != 0) {
                    const uint32_t top = key[c] >> up;
                    int g = -1;
#pragma unroll
                    for (int j = 0; j < PROFILE_MAX_Q; j++) g = (j < Q && lead[j] && top == prefix[j]) ? j : g;
                    on = on && g >= 0;
                    at += (uint32_t)(g < 0 ? 0 : g) * (uint32_t)PROFILE_BINS;
                }
                tail_hist_add(s_hist, at, on);
            }
        }
        __syncthreads();
        if (pass == 0)
            profile_pick<THREADS, PROFILE_BINS1>(s_hist, s_wave, s_sel, Q, lead, slot, k);
        else
            profile_pick<THREADS, PROFILE_BINS>(s_hist, s_wave, s_sel, Q, lead, slot, k);
        // every target: its bin joins its group's prefix, its rank counts inside the bin; neighbours with one prefix stay a group
#pragma unroll
        for (int j = 0; j < PROFILE_MAX_Q; j++) {
            if (j < Q) {
                k[j] -= uni(s_sel[j][1]);
                prefix[j] = (prefix[j] << (pass == 0 ? 12 : 10)) | uni(s_sel[j][0]);  // (a group's members held one prefix)
            }
        }
#pragma unroll
        for (int j = 1; j < PROFILE_MAX_Q; j++) {
            if (j < Q) {
                lead[j] = prefix[j] != prefix[j - 1];
                slot[j] = lead[j] ? j : slot[j - 1];
            }
        }
        // (s_sel and s_wave are rewritten only behind the next pass' two barriers)
    }
    if (tid < Q) {
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < PROFILE_MAX_Q; j++) mine = tid == j ? prefix[j] : mine;
        dst[(size_t)tid * pitch] = key2f(mine);
    }
}

struct ProfileScoreArgs {
    const float *profile;  // [R][Q][KS]
    const float *table;    // [R][L]: the weights
    const float *colmin;   // [Q][KS]
    int Q, K, S;
    int first_rank;
    float *out;  // [n_ranks][Q][1 + S]
};

// one workgroup per (reported rank, quantile): k_tail_score's rule on plane q
__global__ __launch_bounds__(TAIL_SCORE_THREADS) void k_profile_score(ProfileScoreArgs a) {
    const int KS = a.K + a.S, q = (int)blockIdx.y;
    const int r = a.first_rank + (int)blockIdx.x;
    tail_score_rank(a.profile + ((size_t)r * a.Q + q) * (size_t)KS, a.table + (size_t)r * NVRX_TABLE_LEN(a.K, a.S) + 2 * KS,
                    a.colmin + (size_t)q * KS, a.K, a.S, a.out + ((size_t)blockIdx.x * a.Q + q) * (size_t)(1 + a.S));
}

// 256 threads for the rows quantile_launch gives 256, 1024 beyond; the key buffer follows the variant
int profile_launch(const ProfileArgs &a, int blocks, hipStream_t st) {
    if (blocks == 0) return NVRX_OK;
    if (a.row_stride <= PROFILE_STAGE_256)
        hipLaunchKernelGGL((k_row_profile<256, PROFILE_STAGE_256>), dim3(blocks), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_row_profile<1024, PROFILE_STAGE_1024>), dim3(blocks), dim3(1024), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

int profile_q_check(const uint32_t *q_ppm, int Q) {
    if (Q < 1 || Q > PROFILE_MAX_Q) return fail(NVRX_ERR_RANGE, "Q=%d quantiles outside [1,%d]", Q, PROFILE_MAX_Q);
    if (!q_ppm) return fail(NVRX_ERR_INVALID, "q_ppm is null");
    for (int j = 0; j < Q; j++) {
        if (const int rc = tail_q_check(q_ppm[j])) return rc;
        if (j && q_ppm[j] <= q_ppm[j - 1])
            return fail(NVRX_ERR_INVALID, "q_ppm[%d]=%u does not ascend from q_ppm[%d]=%u", j, q_ppm[j], j - 1, q_ppm[j - 1]);
    }
    return NVRX_OK;
}

void profile_targets(const uint32_t *q_ppm, int Q, ProfileArgs *a) {
    a->Q = Q;
    for (int j = 0; j < Q; j++) a->q_ppm[j] = q_ppm[j];
}

}  // namespace

extern "C" {

int nvrx_row_profile(const float *d_samples, const uint32_t *d_counts, int rows, int row_stride, const uint32_t *q_ppm, int Q,
                     float *d_out, void *stream) {
    const int rc = row_op_check(rows, row_stride, d_samples, d_counts, d_out, false, [&] { return profile_q_check(q_ppm, Q); });
    if (rc || rows == 0) return rc;
    ProfileArgs a{};
    a.samples = d_samples, a.counts = d_counts, a.out = d_out;
    a.row_stride = row_stride, a.uniform_n = -1, a.rows = rows;
    profile_targets(q_ppm, Q, &a);
    return profile_launch(a, rows, as_stream(stream));
}

int nvrx_profile_score(const float *d_profile, int Q, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                       float *d_colmin_scratch, float *d_out, void *stream) {
    if (Q < 1 || Q > PROFILE_MAX_Q) return fail(NVRX_ERR_RANGE, "Q=%d quantiles outside [1,%d]", Q, PROFILE_MAX_Q);
    if (const int rc = plane_score_check(d_profile, d_table, R, K, S, first_rank, n_ranks, d_colmin_scratch, d_out)) return rc;
    hipStream_t st = as_stream(stream);
    const int KS = K + S;
    // the minima of all Q * KS columns at once: the [R][Q][KS] table is a [R][Q * KS] table with its own pitch
    if (const int rc = colmin_launch(d_profile, Q * KS, R, Q * KS, d_colmin_scratch, st)) return rc;
    ProfileScoreArgs a{};
    a.profile = d_profile, a.table = d_table, a.colmin = d_colmin_scratch;
    a.Q = Q, a.K = K, a.S = S, a.first_rank = first_rank, a.out = d_out;
    hipLaunchKernelGGL(k_profile_score, dim3(n_ranks, Q), dim3(TAIL_SCORE_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

int nvrx_profile_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, const uint32_t *q_ppm, int Q, float *d_send, int K, int S,
                       int rows_active, void *stream) {
    hipStream_t st = as_stream(stream);
    LocalWindow w;
    int rc = local_window(ctx, desc, d_send, K, S, rows_active, [&] { return profile_q_check(q_ppm, Q); }, nullptr, &st, &w);
    if (rc) return rc;
    ProfileArgs a{};
    window_args(w, &a);
    a.out = d_send;
    a.KS = K + S;
    profile_targets(q_ppm, Q, &a);
    const size_t slots = (size_t)ctx->local_ranks * (size_t)Q * (size_t)a.KS;
    if (slots == 0) return NVRX_OK;
    rc = fill_minus_one(d_send, slots, st);
    if (rc) return rc;
    return profile_launch(a, ctx->local_ranks * w.rows_active, st);
}

}  // extern "C"
