// nvrx_trend.inl -- score trends: whether each score of the history ring is falling from report to report.  Part of the
// translation unit nvrx_straggler.hip (included at its end, behind nvrx_history.inl: it uses that file's geometry, its order
// count and the key map and DPP moves of nvrx_straggler.hip).
//
// The score history says for how many reports a score has been below its threshold; nothing says that a score is on its way
// there.  One launch per report reads the ring nvrx_score_history keeps and leaves, per (rank, family, slot), a 16-byte
// record: the Theil-Sen slope (the lower median of the slopes of all pairs of usable entries), the trend line's level at the
// newest report, the Mann-Kendall statistic S and the number of usable entries (include/nvrx_straggler.h, nvrx_score_trend).
//
// k_score_trend<HS>  HS = 16, 32 or 64 ring positions per cell, k_score_history's geometry: a wave takes 64 / HS consecutive
//   slots of one (rank, family), a SEGMENT of HS lanes per slot, lane a of a segment loads the entry of AGE a.  The ring is
//   only read.  Lane a forms, once, the slopes to its older partners a + k, k = 1 .. HS - 1, of its own segment and keeps
//   their keys in HS - 1 registers (compile-time indices; 0xFFFFFFFF marks a pair that does not exist: a partner outside the
//   segment or an entry that is not usable).  The partner's value arrives by a row rotation where a segment is one row, by
//   the same rotation of the lane's own row and of the segment's other row (one ds_swizzle) where it is two, by ds_bpermute
//   where it is the wave: a lane never reads a neighbour segment's lane as a partner.  S is the segment sum of the lanes'
//   sign counts.  The median slope is found by 32 rounds of bisection on the key, most significant bit first: each lane
//   counts its keys below the candidate, one segment sum decides the bit.  Pairs k >= depth apart exist for no lane and are
//   skipped wave-uniformly.  The level is the lower median of the entries moved along the slope to age 0, by
//   k_score_history's order count.  The lane of age 0 writes the record as one 16-byte store.
//   No LDS array, no barrier, no atomics, no scratch, no trip count or branch that depends on the ring's contents; workgroups
//   share nothing.

#include <type_traits>

namespace {

struct TrendArgs {
    const float *hist;  // [n_ranks][2][1 + S_cap][HS]; k_peer_trend: [n_ranks][1 + S_cap][HS]
    uint4 *out;         // [n_ranks][2][1 + S]; k_peer_trend: [n_ranks][1 + S]
    int S, S_cap;
    int H, slot0, depth;  // slot0 = (n_reports - 1) % H, depth = min(n_reports, H)
    uint32_t waves_per_fam, total_waves;
};

constexpr uint32_t TREND_NAN = 0x7FC00000u;

// f(integral_constant<int, I>) for I in [I, N): the indices are compile-time constants (DPP controls, register numbers)
template <int I, int N, class F>
__device__ __forceinline__ void trend_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        trend_for<I + 1, N>(f);
    }
}

__device__ __forceinline__ bool trend_finite(uint32_t bits) { return (bits & 0x7F800000u) != 0x7F800000u; }

// the sum of `v` over the lane's segment, in every lane of the segment
template <int HS>
__device__ __forceinline__ uint32_t trend_seg_sum(uint32_t v) {
    if constexpr (HS == 64) {
        return wave_sum_u32(v);
    } else {
        v += dpp0<DPP_QUAD_1032>(v);
        v += dpp0<DPP_QUAD_2301>(v);
        v += dpp0<0x124>(v);  // row_ror:4
        v += dpp0<0x128>(v);  // row_ror:8 -- every lane of a row holds the row's sum
        if constexpr (HS == 32) v += (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);  // lane ^ 16: the other row's
        return v;
    }
}

// One cell per segment.  A wave's `rf` only indexes the ring and the records, so the same code serves the peer-score ring
// [n_ranks][1 + S_cap][HS] (k_peer_trend: one family, rf is the rank).
template <int HS>
__device__ __forceinline__ void trend_cell(const TrendArgs &a) {
    constexpr int SPW = 64 / HS;  // slots per wave
    constexpr unsigned long long SEG = HS == 64 ? ~0ull : ((1ull << (HS & 63)) - 1ull);
    const int lane = threadIdx.x & 63;
    const uint32_t gw = blockIdx.x * (HISTORY_THREADS / 64) + (threadIdx.x >> 6);
    if (gw >= a.total_waves) return;  // wave-uniform
    const uint32_t rf = gw / a.waves_per_fam, chunk = gw - rf * a.waves_per_fam;
    const int S = a.S;
    const int seg = lane / HS, age = lane & (HS - 1), sh = seg * HS;
    const int j = (int)chunk * SPW + seg;
    const bool slot = j <= S;
    const bool live = slot && age < a.depth;
    int at = a.slot0 - age;
    at += at < 0 ? a.H : 0;

    uint32_t bits = TREND_NAN;
    if (live) bits = __float_as_uint(a.hist[((size_t)rf * (size_t)(1 + a.S_cap) + (size_t)j) * HS + at]);
    const bool usable = trend_finite(bits);
    if (!usable) bits = TREND_NAN;  // travels as a NaN: no pair with it exists
    const float x = __uint_as_float(bits);
    const uint32_t p = (uint32_t)__popcll((__ballot(usable) >> sh) & SEG);

    // the pair slopes to the older partners of the segment, once, into registers
    uint32_t key[HS - 1];
    int sign = 0;
    auto pair = [&](auto K, uint32_t partner, bool inside) {
        constexpr int k = decltype(K)::value;
        const float y = __uint_as_float(partner);
        const bool ok = usable && inside && trend_finite(partner);
        const double s = ((double)x - (double)y) / (double)k;
        key[k - 1] = ok ? f2key((float)s) : HISTORY_ABSENT;
        sign += ok ? (int)(x > y) - (int)(x < y) : 0;
    };
    // (ages at or beyond the launch's depth hold nothing, so a partner k >= depth away exists for no lane: those pairs are
    // skipped by a wave-uniform branch on the kernel argument -- at H = 8 seven slopes are formed, not fifteen)
    const int depth = a.depth;
    if constexpr (HS == 16) {
        trend_for<1, 16>([&](auto K) {
            constexpr int k = decltype(K)::value;
            key[k - 1] = HISTORY_ABSENT;
            if (k < depth) pair(K, dpp<0x120 + 16 - k>(bits, bits), age + k < 16);  // row_ror:16-k -- lane i reads lane (i + k) mod 16 of its row
        });
    } else if constexpr (HS == 32) {
        const uint32_t other = (uint32_t)__builtin_amdgcn_ds_swizzle((int)bits, 0x401F);  // lane ^ 16: the segment's other row
        const int al = age & 15;
        const bool low = age < 16;
        key[15] = HISTORY_ABSENT;
        if (16 < depth) pair(std::integral_constant<int, 16>{}, other, low);
        trend_for<1, 16>([&](auto K) {
            constexpr int k = decltype(K)::value;
            const uint32_t own = dpp<0x120 + 16 - k>(bits, bits), far = dpp<0x120 + 16 - k>(other, other);
            const bool same_row = al + k < 16;
            pair(K, same_row ? own : far, same_row || low);
            key[k + 15] = HISTORY_ABSENT;
            if (k + 16 < depth) pair(std::integral_constant<int, k + 16>{}, far, same_row && low);
        });
    } else {
        trend_for<1, 64>([&](auto K) {
            constexpr int k = decltype(K)::value;
            key[k - 1] = HISTORY_ABSENT;
            if (k < depth) pair(K, (uint32_t)__builtin_amdgcn_ds_bpermute(((lane + k) & 63) << 2, (int)bits), lane + k < 64);
        });
    }
    const uint32_t mk = trend_seg_sum<HS>((uint32_t)sign);

    // the key of rank (N - 1) >> 1 of the N pair slopes: the largest m with fewer than rank + 1 keys below it
    const uint32_t n_pairs = p * (p - 1u) / 2u, rank = (n_pairs - 1u) >> 1;
    uint32_t m = 0;
#pragma nounroll
    for (int bit = 31; bit >= 0; bit--) {
        const uint32_t cand = m | (1u << bit);
        uint32_t c = 0;
#pragma unroll
        for (int i = 0; i < HS - 1; i += 4) {
            if (i + 1 < depth) {  // wave-uniform: four keys at a time, none of them beyond the depth holds a slope
#pragma unroll
                for (int q = i; q < i + 4 && q < HS - 1; q++) c += key[q] < cand ? 1u : 0u;
            }
        }
        c = trend_seg_sum<HS>(c);
        m = c <= rank ? cand : m;
    }
    const float slope = key2f(m);
    const uint32_t slope_bits = p >= 2u ? __float_as_uint(slope) : TREND_NAN;

    // the trend line's value at the newest report: the lower median of the usable entries moved along the slope to age 0
    const float v = p >= 2u ? (float)((double)x + (double)slope * (double)age) : x;
    const uint32_t vb = v == v ? __float_as_uint(v) : TREND_NAN;
    const uint32_t order = history_order<HS>(usable ? f2key(__uint_as_float(vb)) : HISTORY_ABSENT, lane);
    const unsigned long long hit = (__ballot(usable && order == ((p - 1u) >> 1)) >> sh) & SEG;
    const int from = sh + (hit ? __builtin_ctzll(hit) : 0);
    const uint32_t lv = (uint32_t)__builtin_amdgcn_ds_bpermute(from << 2, (int)vb);
    const uint32_t level = hit ? lv : TREND_NAN;
    if (slot && age == 0) a.out[(size_t)rf * (size_t)(1 + S) + (size_t)j] = make_uint4(slope_bits, level, mk, p);
}

template <int HS>
__global__ __launch_bounds__(HISTORY_THREADS) void k_score_trend(TrendArgs a) {
    trend_cell<HS>(a);
}

// (a kernel of its own name, so that a trace tells the two rings' steps apart)
template <int HS>
__global__ __launch_bounds__(HISTORY_THREADS) void k_peer_trend(TrendArgs a) {
    trend_cell<HS>(a);
}

// argument checks shared by the entry points; nothing here touches a device.  fams: 2 for the score history's ring, 1 for
// the peer-score history's
int trend_check(const void *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports, const void *d_out, int fams = 2) {
    if (n_ranks < 1 || S < 0) return fail(NVRX_ERR_INVALID, "bad trend shape n_ranks=%d S=%d", n_ranks, S);
    if (H < 2 || H > NVRX_HISTORY_MAX_DEPTH) return fail(NVRX_ERR_RANGE, "history depth H=%d outside [2,%d]", H, NVRX_HISTORY_MAX_DEPTH);
    if (S > S_cap) return fail(NVRX_ERR_INVALID, "S=%d section ids, the history holds S_cap=%d", S, S_cap);
    if (S_cap > NVRX_MAX_ROWS) return fail(NVRX_ERR_RANGE, "S_cap=%d ids, at most %d", S_cap, NVRX_MAX_ROWS);
    if (n_reports < 1) return fail(NVRX_ERR_INVALID, "n_reports=0: no report was appended to the history");
    if (!d_hist || !d_out) return fail(NVRX_ERR_INVALID, "null device pointer");
    if ((reinterpret_cast<uintptr_t>(d_hist) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d_out) & 15u) != 0)
        return fail(NVRX_ERR_INVALID, "d_hist or d_out is not 16-byte aligned");
    const int per_wave = 64 / NVRX_HISTORY_STRIDE(H);
    const uint64_t waves = (uint64_t)n_ranks * (uint64_t)fams * (uint64_t)((1 + S + per_wave - 1) / per_wave);
    if (waves > 0x7FFFFFFFull) return fail(NVRX_ERR_RANGE, "n_ranks=%d x S=%d is more than one launch covers", n_ranks, S);
    return NVRX_OK;
}

template <bool PEER = false>
int trend_launch(const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports, void *d_out, hipStream_t st) {
    const int HS = NVRX_HISTORY_STRIDE(H), per_wave = 64 / HS;
    TrendArgs a{};
    a.hist = d_hist, a.out = static_cast<uint4 *>(d_out);
    a.S = S, a.S_cap = S_cap;
    a.H = H, a.slot0 = (int)((n_reports - 1) % (uint64_t)H), a.depth = n_reports < (uint64_t)H ? (int)n_reports : H;
    a.waves_per_fam = (uint32_t)((1 + S + per_wave - 1) / per_wave);
    a.total_waves = (uint32_t)n_ranks * (PEER ? 1u : 2u) * a.waves_per_fam;
    const dim3 grid((a.total_waves + HISTORY_THREADS / 64 - 1) / (HISTORY_THREADS / 64)), block(HISTORY_THREADS);
    if constexpr (PEER) {
        if (HS == 16)
            hipLaunchKernelGGL(k_peer_trend<16>, grid, block, 0, st, a);
        else if (HS == 32)
            hipLaunchKernelGGL(k_peer_trend<32>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(k_peer_trend<64>, grid, block, 0, st, a);
    } else if (HS == 16)
        hipLaunchKernelGGL(k_score_trend<16>, grid, block, 0, st, a);
    else if (HS == 32)
        hipLaunchKernelGGL(k_score_trend<32>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(k_score_trend<64>, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_score_trend(const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports, void *d_out, void *stream) {
    const int rc = trend_check(d_hist, n_ranks, S, S_cap, H, n_reports, d_out);
    if (rc) return rc;
    return trend_launch(d_hist, n_ranks, S, S_cap, H, n_reports, d_out, as_stream(stream));
}

int nvrx_report_trend(nvrx_ctx *ctx, const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports,
                      void *d_out) {
    if (!ctx) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = trend_check(d_hist, n_ranks, S, S_cap, H, n_reports, d_out);
    if (rc) return rc;
    hipStream_t home = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        home = ctx->default_stream;
        HIP_TRY(hipSetDevice(ctx->device));
    }
    // no event: the ring's only writers are history steps, and nvrx_report_history launched the last of them on this stream
    return trend_launch(d_hist, n_ranks, S, S_cap, H, n_reports, d_out, home);
}

}  // extern "C"
