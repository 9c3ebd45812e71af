// nvrx_peer_attribute.inl -- peer attribution: the top-N kernels behind a rank's PEER GPU score.  Part of the translation
// unit nvrx_straggler.hip (included at its end: it uses that file's DPP reductions, nvrx_attribute.inl's key maps and
// nvrx_tablefam.inl's checks).
//
// The peer GPU score of rank r in group g (nvrx_peer.inl, k_peer_rank) is p = sum_k(w_k * floor[g][k] / med[r][k]) / W over
// the kernels r holds whose (g, k) pair is referenced.  Its deficit 1 - p = sum_k(n_k) / W with n_k = w_k * (1 - s_k),
// s_k = floor[g][k] / med[r][k]: the microseconds kernel k spent above the pace of the fastest PEER.  k_peer_attribute lists,
// per reported rank, the N kernels with the largest n_k (the order of nvrx_attribute.inl: by value, ties to the lower id,
// NaN after -inf) as 32-byte records that also say whose pace the floor is and how many peers hold the kernel.  The floors are
// the column records the peer step left at the head of its block: nothing is exchanged, reduced or recomputed across ranks.
//
// k_peer_attribute<NTHR, T>  one workgroup per reported rank.  The row is walked ONCE, in tiles of T kernels:
//   load     thread t owns the tile's slots t, t + NTHR, ... (T / NTHR of them): med and w are coalesced 4-byte loads, the
//            group's column record one 16-byte load; all loads of a tile are issued before the first quotient.
//   compute  n_k once per kernel: W, sum n_k and the count go to registers, the 64-bit order-preserving key (+ 1, so that
//            0 is "no candidate" and a NaN's key 0 is still one) to LDS slot k - base.  A slot is read and written by its
//            owner alone, so the tile needs no barrier; it lives in LDS because a winner's slot is cleared by INDEX.
//   select   behind the tile, NVRX_ATTR_MAX_TOP LDS slots hold the running top list (key, id), sorted.  Thread j < 16 takes
//            entry j into registers, then top_n knock-out rounds run over tile + those registers: a lexicographic arg-max on
//            (key, ~id) -- three DPP wave maxima, the winning lane hands {key, ~id, slot} to its wave's LDS slot (two banks
//            by round parity), one barrier, every thread reads the NW slots -- after which the winner's owner clears its
//            slot (or register) and writes list entry j.  Nothing is recomputed and no round filters on the previous winner.
//   records  after the last tile lane j < top_n of wave 0 rebuilds s_k and n_k of list entry j from the table (at most 16
//            quotients) and writes its two words; lane 0 writes the header.
// K <= T is one tile: one pass over global memory, then top_n rounds on LDS.  K f64 quotients per workgroup where k_attribute
// spends (1 + N) K.  No atomics, no global scratch.
//
// d_groups and the records are data: a group id outside [0, G) makes every kernel ineligible (the loads then go to group 0's
// records, which exist: G >= 1), `present` is only compared, floor and floor_rank are only copied or divided.  Every index
// into the table, the block or d_out is built from k < K, r < R and the launch's own numbers.

namespace {

struct PeerAttrArgs {
    const float *table;     // [R][L]
    const int32_t *groups;  // group[R] | ...
    const uint4 *cols;      // [G][K+S] {f32 floor, u32 present, i32 floor_rank, u32 members}
    int K, S, G;
    int first_rank;
    int min_ranks;
    int top_n;
    uint4 *out;  // [n_ranks][1 + top_n][2]
};

constexpr int PATTR_TILE_SMALL = 1024;  // the 256-thread variant serves K <= 1024: always one tile

template <int NTHR, int T>
__global__ __launch_bounds__(NTHR) void k_peer_attribute(PeerAttrArgs a) {
    constexpr int NW = NTHR / 64;
    constexpr int SPT = T / NTHR;  // tile slots per thread
    static_assert(T % NTHR == 0 && NTHR >= NVRX_ATTR_MAX_TOP, "a thread owns whole slots; thread j owns list entry j");
    __shared__ uint64_t s_key[T];                        // key + 1 of tile slot k - base; 0: not eligible or knocked out
    __shared__ uint64_t s_list_key[NVRX_ATTR_MAX_TOP];   // the running top list, best first; 0: empty
    __shared__ uint32_t s_list_id[NVRX_ATTR_MAX_TOP];
    __shared__ uint32_t s_best[2][NW][4];  // [round parity][wave]{key high, key low, ~id, slot}
    __shared__ double s_sum[2][NW];
    __shared__ uint32_t s_cnt[NW];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, KS = a.K + a.S;
    const int L = NVRX_TABLE_LEN(a.K, a.S);
    const int r = a.first_rank + (int)blockIdx.x;
    const float *__restrict__ row = a.table + (size_t)r * L;
    const float *__restrict__ wrow = row + 2 * (size_t)KS;
    const int g = a.groups[r];
    const bool in_group = (uint32_t)g < (uint32_t)a.G;  // block-uniform
    const uint4 *__restrict__ recs = a.cols + (size_t)(in_group ? g : 0) * (size_t)KS;
    uint4 *__restrict__ out = a.out + (size_t)blockIdx.x * 2 * (size_t)(1 + a.top_n);
    const float NaN = __builtin_nanf("");

    if (tid < NVRX_ATTR_MAX_TOP) s_list_key[tid] = 0ull, s_list_id[tid] = 0u;
    __syncthreads();

    double wsum = 0.0, nsum = 0.0;
    uint32_t cnt = 0;
    uint32_t rnd = 0;  // rounds so far: the parity of s_best
    for (int base = 0; base < K; base += T) {
        // the running list into registers (written again only behind this tile's first round barrier)
        uint64_t lkey = 0ull;
        uint32_t lid = 0u;
        if (tid < NVRX_ATTR_MAX_TOP) lkey = s_list_key[tid], lid = s_list_id[tid];

        // the tile: every load first, then n_k once
        float medv[SPT], wv[SPT];
        uint4 rec[SPT];
#pragma unroll
        for (int i = 0; i < SPT; i++) {
            const int k = base + tid + i * NTHR;
            const bool in = k < K;
            medv[i] = in ? row[k] : -1.0f;
            wv[i] = in ? wrow[k] : 0.0f;
            rec[i] = in ? recs[k] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int i = 0; i < SPT; i++) {
            uint64_t key = 0ull;
            if (in_group && medv[i] >= 0.0f && (int)rec[i].y >= a.min_ranks) {  // (k >= K: med -1)
                const double w = (double)wv[i];
                const double n = w * (1.0 - (double)__uint_as_float(rec[i].x) / (double)medv[i]);
                wsum += w;
                nsum += n;
                cnt++;
                key = nk2key(canon_nk(n)) + 1ull;  // (d2key(+inf) < 2^64 - 1: no wrap)
            }
            s_key[tid + i * NTHR] = key;
        }

        for (int j = 0; j < a.top_n; j++, rnd++) {
            uint32_t bh = 0, bl = 0, bi = 0, bs = 0;  // ~id of a real kernel is never 0: bi == 0 is "no candidate"
#pragma unroll
            for (int i = 0; i < SPT; i++) {
                const int s = tid + i * NTHR;
                const uint64_t key = s_key[s];
                const uint32_t kh = (uint32_t)(key >> 32), kl = (uint32_t)key, ki = ~(uint32_t)(base + s);
                if (key != 0ull && (kh > bh || (kh == bh && (kl > bl || (kl == bl && ki > bi))))) bh = kh, bl = kl, bi = ki, bs = (uint32_t)s;
            }
            if (lkey != 0ull) {
                const uint32_t kh = (uint32_t)(lkey >> 32), kl = (uint32_t)lkey, ki = ~lid;
                if (kh > bh || (kh == bh && (kl > bl || (kl == bl && ki > bi)))) bh = kh, bl = kl, bi = ki, bs = (uint32_t)(T + tid);
            }
            // lexicographic maximum over the wave: the word that decides is masked out in the lanes that lost before it
            const uint32_t mh = wave_max_u32(bh);
            const uint32_t ml = wave_max_u32(bh == mh ? bl : 0u);
            const uint32_t mi = wave_max_u32((bh == mh && bl == ml) ? bi : 0u);
            // ids are unique across tile and list, so one lane holds the maximum (none: lane 0 says so)
            if (mi ? (bh == mh && bl == ml && bi == mi) : lane == 0) {
                s_best[rnd & 1][wave][0] = mh;
                s_best[rnd & 1][wave][1] = ml;
                s_best[rnd & 1][wave][2] = mi;
                s_best[rnd & 1][wave][3] = bs;
            }
            __syncthreads();
            uint32_t ph = 0, pl = 0, pi = 0, ps = 0;
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const uint32_t h = s_best[rnd & 1][w][0], l = s_best[rnd & 1][w][1], i = s_best[rnd & 1][w][2];
                if (h > ph || (h == ph && (l > pl || (l == pl && i > pi)))) ph = h, pl = l, pi = i, ps = s_best[rnd & 1][w][3];
            }
            if (pi == 0) {  // block-uniform: nothing left, in this tile or the list; the list's tail is empty
                if (tid >= j && tid < NVRX_ATTR_MAX_TOP) s_list_key[tid] = 0ull, s_list_id[tid] = 0u;
                rnd++;
                break;
            }
            // the winner's owner knocks it out and enters it as the list's entry j
            const bool from_list = ps >= (uint32_t)T;
            if (tid == (int)(from_list ? ps - (uint32_t)T : ps & (uint32_t)(NTHR - 1))) {
                if (from_list)
                    lkey = 0ull;
                else
                    s_key[ps] = 0ull;
                s_list_key[j] = ((uint64_t)ph << 32) | pl;
                s_list_id[j] = ~pi;
            }
        }
        __syncthreads();  // the list is whole before the next tile (or the records) read it
    }

    wsum = wave_sum_f64(wsum);
    nsum = wave_sum_f64(nsum);
    cnt = wave_sum_u32(cnt);
    if (lane == 0) {
        s_sum[0][wave] = wsum;
        s_sum[1][wave] = nsum;
        s_cnt[wave] = cnt;
    }
    __syncthreads();
    if (wave != 0) return;
    wsum = nsum = 0.0;
    cnt = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        wsum += s_sum[0][w];
        nsum += s_sum[1][w];
        cnt += s_cnt[w];
    }

    // the records: lane j rebuilds entry j from the table
    double n = 0.0;
    if (lane < a.top_n) {
        uint4 e0 = make_uint4(0xFFFFFFFFu, __float_as_uint(NaN), __float_as_uint(NaN), __float_as_uint(NaN));
        uint4 e1 = make_uint4(__float_as_uint(NaN), 0xFFFFFFFFu, 0u, 0u);
        if (s_list_key[lane] != 0ull) {  // (never with cnt == 0)
            const int k = (int)s_list_id[lane];
            const uint4 rc = recs[k];
            const double s = (double)__uint_as_float(rc.x) / (double)row[k];
            n = canon_nk((double)wrow[k] * (1.0 - s));
            e0 = make_uint4((uint32_t)k, __float_as_uint((float)(n / wsum)), __float_as_uint((float)s), __float_as_uint((float)n));
            e1 = make_uint4(rc.x, rc.z, rc.y, 0u);
        }
        out[2 + 2 * lane] = e0;
        out[3 + 2 * lane] = e1;
    }
    const double listed = wave_sum_f64(n);
    if (lane == 0) {
        out[0] = cnt ? make_uint4(__float_as_uint((float)(nsum / wsum)), __float_as_uint((float)(listed / wsum)), cnt,
                                  __float_as_uint((float)wsum))
                     : make_uint4(__float_as_uint(NaN), __float_as_uint(NaN), 0u, __float_as_uint(0.0f));
        out[1] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// argument checks shared by both entry points: nvrx_attribute's in its order, then the peer step's; no device is touched
int peer_attr_check(int R, int K, int S, int G, int first_rank, int n_ranks, int min_ranks, int top_n) {
    const int rc = attr_check(R, K, S, first_rank, n_ranks, top_n);
    if (rc) return rc;
    if (R > NVRX_ROBUST_MAX_RANKS) return fail(NVRX_ERR_RANGE, "R=%d ranks, at most %d", R, NVRX_ROBUST_MAX_RANKS);
    if (S > NVRX_MAX_ROWS) return fail(NVRX_ERR_RANGE, "S=%d section ids, at most %d", S, NVRX_MAX_ROWS);
    if (min_ranks < 1) return fail(NVRX_ERR_RANGE, "min_ranks=%d, at least 1", min_ranks);
    return groups_check(R, G);
}

// the pointers, last: the column records are read with 16-byte loads
int peer_attr_pointers(const void *d_out, const void *d_peer_cols, bool others, bool report) {
    if (const int rc = out_check(d_out, others && d_peer_cols, report)) return rc;
    if ((reinterpret_cast<uintptr_t>(d_peer_cols) & 15u) != 0) return fail(NVRX_ERR_INVALID, "d_peer_cols is not 16-byte aligned");
    return NVRX_OK;
}

int peer_attr_launch(const float *d_table, int K, int S, const int32_t *d_groups, int G, const void *d_peer_cols, int first_rank,
                     int n_ranks, int min_ranks, int top_n, void *d_out, hipStream_t st) {
    PeerAttrArgs a{};
    a.table = d_table, a.groups = d_groups, a.cols = static_cast<const uint4 *>(d_peer_cols);
    a.K = K, a.S = S, a.G = G, a.first_rank = first_rank, a.min_ranks = min_ranks, a.top_n = top_n;
    a.out = static_cast<uint4 *>(d_out);
    if (K > PATTR_TILE_SMALL)
        hipLaunchKernelGGL((k_peer_attribute<1024, NVRX_PEER_ATTR_TILE>), dim3(n_ranks), dim3(1024), 0, st, a);
    else
        hipLaunchKernelGGL((k_peer_attribute<256, PATTR_TILE_SMALL>), dim3(n_ranks), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_peer_attribute(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, const void *d_peer_cols,
                        int first_rank, int n_ranks, int min_ranks, int top_n, void *d_out, void *stream) {
    const int rc = peer_attr_check(R, K, S, G, first_rank, n_ranks, min_ranks, top_n);
    if (rc) return rc;
    if (const int rc = peer_attr_pointers(d_out, d_peer_cols, d_table && d_groups, false)) return rc;
    return peer_attr_launch(d_table, K, S, d_groups, G, d_peer_cols, first_rank, n_ranks, min_ranks, top_n, d_out, as_stream(stream));
}

int nvrx_report_peer_attribute(nvrx_ctx *ctx, const nvrx_report_desc *desc, const int32_t *d_groups, int G,
                               const void *d_peer_cols, int first_rank, int n_ranks, int min_ranks, int top_n, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = peer_attr_check(desc->R, desc->K, desc->S, G, first_rank, n_ranks, min_ranks, top_n);
    if (rc) return rc;
    if (const int rc = peer_attr_pointers(d_out, d_peer_cols, d_groups != nullptr, true)) return rc;
    hipStream_t home = nullptr;
    const float *table = nullptr;
    // the context's stream, where nvrx_report_peer wrote the records: behind that step without an event
    if (const int rc = report_table(ctx, desc, &home, &table)) return rc;
    return peer_attr_launch(table, desc->K, desc->S, d_groups, G, d_peer_cols, first_rank, n_ranks, min_ranks, top_n, d_out, home);
}

}  // extern "C"
