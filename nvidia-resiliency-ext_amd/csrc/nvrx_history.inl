// nvrx_history.inl -- score history: how each score behaved over the last H reports.  Part of the translation unit
// nvrx_straggler.hip (included at its end: it uses that file's key map and DPP moves).
//
// Every other score looks inside one report window.  A device ring keeps the last H reports' scores per reported rank, score
// family and slot (the GPU score, then one per section id); one launch per report appends the report's scores -- read where
// the score kernel wrote them -- and leaves, per (rank, family, slot), a 32-byte record: the newest score, the lower median,
// the worst and the best of the ring, how many entries are present and below the threshold, and the streak of newest entries
// that are all below (include/nvrx_straggler.h, nvrx_score_history).
//
// k_score_history<HS>  HS = 16, 32 or 64 ring positions per cell.  A wave takes 64 / HS consecutive slots of one (rank,
//   family): a SEGMENT of HS lanes per slot, lane a of a segment holding the entry of AGE a -- it loads position (n_before -
//   a) mod H, so the lanes are in age order straight from the load and the wave's loads are one run of 64 consecutive floats.
//   The lane of age 0 takes this report's score from the score rows instead and appends it.  Counts are popcounts of ballots
//   masked to the segment, the streak is the number of trailing ones of the segment's below-mask.  A lane's position in its
//   segment's order is the number of keys that order before its own (ties: the lower age first), counted over HS broadcasts
//   inside the segment: row rotations on the DPP path where a segment is one or two rows of 16 lanes, readlane where it is
//   the wave (as k_robust_cols<0> counts).  An absent entry travels as the key 0xFFFFFFFF, which no present value has and
//   which orders behind all of them: no presence mask goes with the broadcasts.  The lanes at positions 0, (present - 1) >> 1
//   and present - 1 hand worst, median and best to the lane of age 0, which writes the record as two 16-byte stores.  No LDS
//   memory, no barrier, no atomics, no scratch, no data-dependent loop; workgroups share nothing.
// k_peer_history<HS>  the same cell code (history_cell<HS, true>) on the peer-score ring, which has one family: see
//   nvrx_peer_history.inl.

namespace {

constexpr int HISTORY_THREADS = 256;
constexpr uint32_t HISTORY_ABSENT = 0xFFFFFFFFu;  // f2key of a NaN: above f2key(+inf), the key of no present value

struct HistoryArgs {
    const float *scores;  // [R][2 + 2S]; k_peer_history: the peer step's rank part [n_ranks][1 + S]
    float *hist;          // [n_ranks][2][1 + S_cap][HS]; k_peer_history: [n_ranks][1 + S_cap][HS]
    uint4 *out;           // [n_ranks][2][1 + S][2]; k_peer_history: [n_ranks][1 + S][2]
    int S, S_cap, first_rank;
    int H, slot0, depth;  // slot0 = n_before % H, depth = min(n_before + 1, H)
    uint32_t waves_per_fam, total_waves;
    double thr[4];  // gpu_rel, section_rel, gpu_indiv, section_indiv
};

// keys of the 16 lanes of `src`'s row that order before `key`, over the rotations T .. 15 of the row.  tie < 0: `src` is the
// lane's own row, of two equal keys the one at the lower row position `al` goes first; else the row lies wholly before
// (tie != 0) or behind (tie == 0) the lane's own.
template <int T>
__device__ __forceinline__ uint32_t history_row_before(uint32_t src, uint32_t key, int al, int tie) {
    if constexpr (T == 16) {
        return 0u;
    } else {
        uint32_t kj = src;
        if constexpr (T != 0) kj = dpp<0x120 + T>(src, src);  // row_ror:T -- lane i of a row reads lane (i - T) mod 16 of it
        const bool first = tie < 0 ? ((al - T) & 15) < al : tie != 0;
        return ((kj < key || (kj == key && first)) ? 1u : 0u) + history_row_before<T + 1>(src, key, al, tie);
    }
}

// the number of keys of the lane's segment that order before its own (ties: the lower age first)
template <int HS>
__device__ __forceinline__ uint32_t history_order(uint32_t key, int lane) {
    if constexpr (HS == 16) {
        return history_row_before<1>(key, key, lane & 15, -1);
    } else if constexpr (HS == 32) {
        const uint32_t other = (uint32_t)__builtin_amdgcn_ds_swizzle((int)key, 0x401F);  // lane ^ 16: the segment's other row
        return history_row_before<1>(key, key, lane & 15, -1) + history_row_before<0>(other, key, lane & 15, (lane >> 4) & 1);
    } else {
        uint32_t pos = 0;
#pragma unroll
        for (int j = 0; j < 64; j++) {
            const uint32_t kj = (uint32_t)__builtin_amdgcn_readlane((int)key, j);
            pos += (kj < key || (kj == key && j < lane)) ? 1u : 0u;
        }
        return pos;
    }
}

// One cell per segment.  PEER: the peer-score history (nvrx_peer_history) -- one family, so a wave's `rf` is the rank itself,
// and the lane of age 0 reads x from the rank part the peer step left, [n_ranks][1 + S], one run of consecutive floats per
// wave; the record is the one family 1 gets, with thr[0] and thr[1].
template <int HS, bool PEER>
__device__ __forceinline__ void history_cell(const HistoryArgs &a) {
    constexpr int SPW = 64 / HS;  // slots per wave
    constexpr unsigned long long SEG = HS == 64 ? ~0ull : ((1ull << (HS & 63)) - 1ull);
    const int lane = threadIdx.x & 63;
    const uint32_t gw = blockIdx.x * (HISTORY_THREADS / 64) + (threadIdx.x >> 6);
    if (gw >= a.total_waves) return;  // wave-uniform
    const uint32_t rf = gw / a.waves_per_fam, chunk = gw - rf * a.waves_per_fam;
    const int f = PEER ? 1 : (int)(rf & 1u), r = PEER ? (int)rf : (int)(rf >> 1);
    const int S = a.S;
    const int seg = lane / HS, age = lane & (HS - 1), sh = seg * HS;
    const int j = (int)chunk * SPW + seg;
    const bool slot = j <= S;
    const bool live = slot && age < a.depth;
    int at = a.slot0 - age;
    at += at < 0 ? a.H : 0;

    float x = __builtin_nanf("");
    if (live) {
        float *cell = a.hist + ((size_t)rf * (size_t)(1 + a.S_cap) + (size_t)j) * HS;
        if (age == 0) {
            if constexpr (PEER) {
                x = a.scores[(size_t)r * (size_t)(1 + S) + (size_t)j];
            } else {
                const int col = j == 0 ? f : 2 + f * S + (j - 1);
                x = a.scores[(size_t)(a.first_rank + r) * (size_t)NVRX_SCORE_LEN(S) + col];
            }
            cell[at] = x;
        } else {
            x = cell[at];
        }
    }
    const double tg = f ? a.thr[0] : a.thr[2], ts = f ? a.thr[1] : a.thr[3];
    const bool present = live && x == x;
    const bool below = present && (double)x < (j == 0 ? tg : ts);
    const unsigned long long pm = (__ballot(present) >> sh) & SEG;
    const unsigned long long bm = (__ballot(below) >> sh) & SEG;
    const uint32_t n_present = (uint32_t)__popcll(pm), n_below = (uint32_t)__popcll(bm);
    const uint32_t streak = bm == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~bm);

    const uint32_t bits = __float_as_uint(x);
    const uint32_t order = history_order<HS>(present ? f2key(x) : HISTORY_ABSENT, lane);
    // the value of the segment's lane at position `target` of its order, in every lane of the segment
    auto pick = [&](uint32_t target) -> uint32_t {
        const unsigned long long hit = (__ballot(present && order == target) >> sh) & SEG;
        const int from = sh + (hit ? __builtin_ctzll(hit) : 0);
        const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute(from << 2, (int)bits);
        return hit ? v : __float_as_uint(__builtin_nanf(""));
    };
    const uint32_t worst = pick(0u), median = pick((n_present - 1u) >> 1), best = pick(n_present - 1u);
    if (slot && age == 0) {
        uint4 *rec = a.out + ((size_t)rf * (size_t)(1 + S) + (size_t)j) * 2;
        rec[0] = make_uint4(bits, median, worst, best);
        rec[1] = make_uint4(streak, n_below, n_present, (uint32_t)a.depth);
    }
}

template <int HS>
__global__ __launch_bounds__(HISTORY_THREADS) void k_score_history(HistoryArgs a) {
    history_cell<HS, false>(a);
}

template <int HS>
__global__ __launch_bounds__(HISTORY_THREADS) void k_peer_history(HistoryArgs a) {
    history_cell<HS, true>(a);
}

// argument checks shared by the entry points; nothing here touches a device.  fams: 2 for the score history (four
// thresholds), 1 for the peer-score history (two)
int history_check(int R, int S, int first_rank, int n_ranks, const void *d_hist, int S_cap, int H, const double *thresholds,
                  const void *d_out, int fams = 2) {
    if (R <= 0 || S < 0) return fail(NVRX_ERR_INVALID, "bad score shape R=%d S=%d", R, S);
    if (H < 2 || H > NVRX_HISTORY_MAX_DEPTH) return fail(NVRX_ERR_RANGE, "history depth H=%d outside [2,%d]", H, NVRX_HISTORY_MAX_DEPTH);
    if (S > S_cap) return fail(NVRX_ERR_INVALID, "S=%d section ids, the history holds S_cap=%d", S, S_cap);
    if (S_cap > NVRX_MAX_ROWS) return fail(NVRX_ERR_RANGE, "S_cap=%d ids, at most %d", S_cap, NVRX_MAX_ROWS);
    if (first_rank < 0 || n_ranks < 1 || first_rank > R - n_ranks)
        return fail(NVRX_ERR_INVALID, "ranks [%d,%d+%d) outside the scores' %d", first_rank, first_rank, n_ranks, R);
    if (!d_hist || !d_out) return fail(NVRX_ERR_INVALID, "null device pointer");
    if ((reinterpret_cast<uintptr_t>(d_hist) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d_out) & 15u) != 0)
        return fail(NVRX_ERR_INVALID, "d_hist or d_out is not 16-byte aligned");
    if (thresholds)
        for (int i = 0; i < 2 * fams; i++)
            if (thresholds[i] - thresholds[i] != 0.0) return fail(NVRX_ERR_INVALID, "thresholds[%d] is not finite", i);
    const int per_wave = 64 / NVRX_HISTORY_STRIDE(H);
    const uint64_t waves = (uint64_t)n_ranks * (uint64_t)fams * (uint64_t)((1 + S + per_wave - 1) / per_wave);
    if (waves > 0x7FFFFFFFull) return fail(NVRX_ERR_RANGE, "n_ranks=%d x S=%d is more than one launch covers", n_ranks, S);
    return NVRX_OK;
}

template <bool PEER = false>
int history_launch(const float *d_scores, int S, int first_rank, int n_ranks, float *d_hist, int S_cap, int H,
                   uint64_t n_before, const double *thresholds, void *d_out, hipStream_t st) {
    const int HS = NVRX_HISTORY_STRIDE(H), per_wave = 64 / HS;
    HistoryArgs a{};
    a.scores = d_scores, a.hist = d_hist, a.out = static_cast<uint4 *>(d_out);
    a.S = S, a.S_cap = S_cap, a.first_rank = first_rank;
    a.H = H, a.slot0 = (int)(n_before % (uint64_t)H), a.depth = n_before + 1 < (uint64_t)H ? (int)(n_before + 1) : H;
    a.waves_per_fam = (uint32_t)((1 + S + per_wave - 1) / per_wave);
    a.total_waves = (uint32_t)n_ranks * (PEER ? 1u : 2u) * a.waves_per_fam;
    for (int i = 0; i < 4; i++) a.thr[i] = thresholds && i < (PEER ? 2 : 4) ? thresholds[i] : 0.75;
    const dim3 grid((a.total_waves + HISTORY_THREADS / 64 - 1) / (HISTORY_THREADS / 64)), block(HISTORY_THREADS);
    if constexpr (PEER) {
        if (HS == 16)
            hipLaunchKernelGGL(k_peer_history<16>, grid, block, 0, st, a);
        else if (HS == 32)
            hipLaunchKernelGGL(k_peer_history<32>, grid, block, 0, st, a);
        else
            hipLaunchKernelGGL(k_peer_history<64>, grid, block, 0, st, a);
    } else if (HS == 16)
        hipLaunchKernelGGL(k_score_history<16>, grid, block, 0, st, a);
    else if (HS == 32)
        hipLaunchKernelGGL(k_score_history<32>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(k_score_history<64>, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_score_history(const float *d_scores, int R, int S, int first_rank, int n_ranks, float *d_hist, int S_cap, int H,
                       uint64_t n_before, const double *thresholds, void *d_out, void *stream) {
    const int rc = history_check(R, S, first_rank, n_ranks, d_hist, S_cap, H, thresholds, d_out);
    if (rc) return rc;
    if (!d_scores || (reinterpret_cast<uintptr_t>(d_scores) & 3u) != 0) return fail(NVRX_ERR_INVALID, "d_scores is null or misaligned");
    return history_launch(d_scores, S, first_rank, n_ranks, d_hist, S_cap, H, n_before, thresholds, d_out, as_stream(stream));
}

int nvrx_report_history(nvrx_ctx *ctx, const nvrx_report_desc *desc, int first_rank, int n_ranks, float *d_hist, int S_cap,
                        int H, uint64_t n_before, const double *thresholds, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = history_check(desc->R, desc->S, first_rank, n_ranks, d_hist, S_cap, H, thresholds, d_out);
    if (rc) return rc;
    hipStream_t home = nullptr;
    if (const int rc = report_table(ctx, desc, &home, nullptr)) return rc;  // (this step reads the report's scores, not its table)
    return history_launch(desc->d_scores, desc->S, first_rank, n_ranks, d_hist, S_cap, H, n_before, thresholds, d_out, home);
}

}  // extern "C"
