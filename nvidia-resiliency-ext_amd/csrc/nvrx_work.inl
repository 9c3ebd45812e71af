// nvrx_work.inl -- work groups: which ranks do the same work, inferred from the table a report gathers.  Part of the
// translation unit nvrx_straggler.hip (included at its end, behind nvrx_node.inl: it uses that file's wave sums and
// nvrx_tablefam.inl's checks and ordering behind a report).  The contract is in include/nvrx_straggler.h (nvrx_work_groups).
//
// The peer, pace-per-group and node scores are told which ranks are peers.  The table says it by itself: which kernel ids and
// section ids a rank has at all, and how often each kernel ran (w / med, the weight being NUM * AVG) do not depend on how
// fast the rank runs.  This is the one O(R^2) step of the library: every pair of ranks over every column.
//
// k_work_sig     one workgroup per rank, strided over its columns (coalesced row reads): the signature plane -- the R (K+S)
//   f64 divisions are done once, so that the pair loop does none -- and the rank's present kernel and section columns, which
//   k_work_groups (ranks with data) and k_work_rank (the record) pick up from the rank record's last two words.
// k_work_pairs   one workgroup of 256 per 64 x 64 tile of rank pairs, every tile of the T x T grid (the block is symmetric by
//   the rule, not by a transposed write).  Columns go by chunks of 64: both rank tiles' chunks are staged in LDS at a pitch
//   of 65 entries -- thread (tx, ty) reads rows ty + 16 i of one tile (two addresses per half wave: broadcasts) and rows
//   tx + 16 j of the other (16 addresses on 16 bank pairs; at a pitch of 64 they would share one) -- and keeps a 4 x 4
//   register tile of {unlike, either}.  Rows beyond R and columns beyond K+S are staged as absent (the loads are clamped,
//   never skipped per lane): they add to neither counter.  A wave stages one rank's chunk, lane = column, so a ballot is that
//   rank's presence word of the chunk, and presence costs two popcounts per pair and chunk.  What is left per pair and column
//   is the count rule, which needs no f64 in the loop: an entry is staged as {q, u}, u the smallest f32 above f * q
//   (work_staged), and hi > f * lo is a.q >= b.u || b.q >= a.u.  The tile's alike bits are ORed into 64 LDS words
//   (non-returning LDS OR) and stored as plain 8-byte vector stores; each row's nearest of the tile is reduced from 16
//   candidates in LDS.
// k_work_groups  one workgroup of 1024: labels in LDS (16 KB at 4096 ranks), min-label propagation over the adjacency bits
//   with pointer jumping until a block-wide "nothing changed" (at most R trips).  Thread r alone writes label r and labels
//   only fall, towards the component's lowest rank, which is where every schedule ends.  Then sizes (LDS integer adds),
//   {root, size} per rank and the job record.
// k_work_rank    one wave per rank: the popcount of its adjacency row, the T partial nearest records reduced in the total
//   order (share, rank), and the 32-byte record as two 16-byte stores.
// No float atomics, no global atomics, no scratch.

namespace {

constexpr int WORK_TILE = 64;
constexpr int WORK_PITCH = WORK_TILE + 1;
constexpr int WORK_GROUPS_THREADS = 1024;
static_assert(NVRX_WORK_MAX_RANKS % WORK_TILE == 0 && NVRX_WORK_MAX_RANKS <= NVRX_ROBUST_MAX_RANKS, "tiles of 64 ranks");

// d_out in 32-bit words: every part starts on a 16-byte boundary
struct WorkLayout {
    size_t adj, part, rank, job, words;  // (the signature plane starts at 0)
    uint32_t sig_pad, adj_pad;           // words that pad parts A and B
};

inline WorkLayout work_layout(int R, int K, int S) {
    const size_t r = (size_t)R, T = (r + WORK_TILE - 1) / WORK_TILE, KS = (size_t)K + (size_t)S;
    WorkLayout l;
    l.adj = (r * KS + 3) & ~size_t{3};
    l.sig_pad = (uint32_t)(l.adj - r * KS);
    l.part = l.adj + ((2 * r * T + 3) & ~size_t{3});
    l.adj_pad = (uint32_t)(l.part - l.adj - 2 * r * T);
    l.rank = l.part + 4 * r * T;
    l.job = l.rank + 8 * r;
    l.words = l.job + 4;
    return l;
}

struct WorkArgs {
    const float *table;  // [R][L]
    int R, K, S, T;
    double factor;  // 1.0 + (double)count_tol
    uint32_t ppm;
    uint32_t sig_pad, adj_pad;
    float *sig;           // A [R][K+S]
    unsigned long long *adj;  // B [R][T]
    uint4 *part;          // C [R][T]
    uint32_t *rank;       // D [R][8]
    uint32_t *job;        // E [4]
};

__global__ __launch_bounds__(256) void k_work_sig(WorkArgs a) {
    __shared__ uint32_t s_cnt[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = (int)blockIdx.x, K = a.K, KS = K + a.S;
    const float *__restrict__ row = a.table + (size_t)r * NVRX_TABLE_LEN(K, a.S);
    float *__restrict__ out = a.sig + (size_t)r * (size_t)KS;
    uint32_t nk = 0, ns = 0;
    for (int c = tid; c < KS; c += 256) {
        const float med = row[c];
        const bool present = med >= 0.0f;  // (a NaN is absent)
        float s = present ? 0.0f : -1.0f;
        if (c < K) {
            const float w = row[2 * KS + c];
            const float q = (float)((double)w / (double)med);
            if (present && med > 0.0f && w > 0.0f && w < INFINITY && q > 0.0f && q < INFINITY) s = q;
            nk += present ? 1u : 0u;
        } else {
            ns += present ? 1u : 0u;
        }
        out[c] = s;
    }
    nk = wave_sum_u32(nk), ns = wave_sum_u32(ns);
    if (lane == 0) s_cnt[0][wave] = nk, s_cnt[1][wave] = ns;
    __syncthreads();
    if (tid == 0) {
        nk = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
        ns = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
        *reinterpret_cast<uint2 *>(a.rank + 8 * (size_t)r + 6) = make_uint2(nk, ns);
    }
    if (r == 0) {  // the words that pad parts A and B (at most 3 and 2)
        if (tid < (int)a.sig_pad) a.sig[(size_t)a.R * (size_t)KS + tid] = 0.0f;
        if (tid < (int)a.adj_pad) reinterpret_cast<uint32_t *>(a.adj + (size_t)a.R * (size_t)a.T)[tid] = 0u;
    }
}

// whether candidate 1 is nearer than candidate 2: the smaller share unlike / either, the lower rank on a tie; a rank of -1 is
// no candidate
__device__ __forceinline__ bool work_nearer(uint32_t u1, uint32_t e1, int r1, uint32_t u2, uint32_t e2, int r2) {
    if (r1 < 0) return false;
    if (r2 < 0) return true;
    const unsigned long long p1 = (unsigned long long)u1 * e2, p2 = (unsigned long long)u2 * e1;
    return p1 < p2 || (p1 == p2 && r1 < r2);
}

// a staged signature as the pair loop wants it: {q, u}.  With f = 1 + count_tol >= 1 the count rule hi > f * lo (one f64
// product, one comparison) is "a > f * b or b > f * a", and for f32 a: a > p  <=>  a >= u, u being the smallest f32 above the
// f64 p = f * b -- p rounded to f32, stepped up one ulp unless the rounding already went up (an overflow to +inf stays +inf:
// no finite a is above it).  A signature without a count is {-inf, +inf}: it compares true against nothing.
__device__ __forceinline__ float2 work_staged(float v, double factor) {
    if (!(v > 0.0f)) return make_float2(-INFINITY, INFINITY);
    const double p = factor * (double)v;
    const float c = (float)p;
    return make_float2(v, (double)c > p ? c : __uint_as_float(__float_as_uint(c) + 1u));
}

__global__ __launch_bounds__(256) void k_work_pairs(WorkArgs a) {
    __shared__ float2 s_a[WORK_TILE * WORK_PITCH], s_b[WORK_TILE * WORK_PITCH];  // {q, u} per (rank of the tile, column of the chunk)
    __shared__ unsigned long long s_pa[WORK_TILE], s_pb[WORK_TILE];              // the chunk's presence bits per rank
    __shared__ uint32_t s_adj[WORK_TILE][2];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int ti = (int)blockIdx.y, tj = (int)blockIdx.x;
    const int R = a.R, KS = a.K + a.S;
    const int lrow = tid >> 6, lcol = tid & 63;
    uint32_t unl[4][4], eit[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) unl[i][j] = 0u, eit[i][j] = 0u;
    if (tid < 2 * WORK_TILE) (&s_adj[0][0])[tid] = 0u;
    // a thread's 16 + 16 signatures of a chunk (rows lrow + 4 k of both tiles, column lcol), loaded one chunk ahead so that
    // the loads are in flight while the chunk before is compared
    float ra[16], rb[16];
    auto load_chunk = [&](int c0) {
        const int c = c0 + lcol;
        const bool col_ok = c < KS;
        const int cc = col_ok ? c : KS - 1;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int row = lrow + 4 * k;
            const int ga = ti * WORK_TILE + row, gb = tj * WORK_TILE + row;
            const float va = a.sig[(size_t)min(ga, R - 1) * (size_t)KS + cc];
            const float vb = a.sig[(size_t)min(gb, R - 1) * (size_t)KS + cc];
            ra[k] = (col_ok && ga < R) ? va : -1.0f;
            rb[k] = (col_ok && gb < R) ? vb : -1.0f;
        }
    };
    if (KS > 0) load_chunk(0);
    for (int c0 = 0; c0 < KS; c0 += WORK_TILE) {  // block-uniform
        __syncthreads();                          // (the previous chunk has been read)
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int row = lrow + 4 * k;  // wave-uniform: a wave stages one rank's chunk, lane = column
            s_a[row * WORK_PITCH + lcol] = work_staged(ra[k], a.factor);
            s_b[row * WORK_PITCH + lcol] = work_staged(rb[k], a.factor);
            const unsigned long long pa = __ballot(ra[k] >= 0.0f), pb = __ballot(rb[k] >= 0.0f);
            if (lcol == 0) s_pa[row] = pa, s_pb[row] = pb;
        }
        __syncthreads();
        if (c0 + WORK_TILE < KS) load_chunk(c0 + WORK_TILE);  // block-uniform
        // presence, 64 columns at a time: a column only one of two ranks has is unlike, and never also apart in its counts
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const unsigned long long pa = s_pa[ty + 16 * i], pb = s_pb[tx + 16 * j];
                eit[i][j] += (uint32_t)__popcll(pa | pb);
                unl[i][j] += (uint32_t)__popcll(pa ^ pb);
            }
        float2 na[4], nb[4];  // the next column's entries, read while this one's are compared
#pragma unroll
        for (int i = 0; i < 4; i++) na[i] = s_a[(ty + 16 * i) * WORK_PITCH];
#pragma unroll
        for (int j = 0; j < 4; j++) nb[j] = s_b[(tx + 16 * j) * WORK_PITCH];
#pragma unroll 1
        for (int x = 0; x < WORK_TILE; x++) {
            float2 va[4], vb[4];
            const int nx = (x + 1) & (WORK_TILE - 1);  // (the last column reads the first again: unused)
#pragma unroll
            for (int i = 0; i < 4; i++) va[i] = na[i], na[i] = s_a[(ty + 16 * i) * WORK_PITCH + nx];
#pragma unroll
            for (int j = 0; j < 4; j++) vb[j] = nb[j], nb[j] = s_b[(tx + 16 * j) * WORK_PITCH + nx];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) unl[i][j] += ((va[i].x >= vb[j].y) | (vb[j].x >= va[i].y)) ? 1u : 0u;
        }
    }
    __syncthreads();  // (s_adj is cleared, also at K+S = 0; the staged chunks are free: the candidates go there)
    uint32_t(*s_cu)[17] = reinterpret_cast<uint32_t(*)[17]>(s_a);
    uint32_t(*s_ce)[17] = s_cu + WORK_TILE;
    int(*s_cr)[17] = reinterpret_cast<int(*)[17]>(s_ce + WORK_TILE);
    static_assert(3 * WORK_TILE * 17 * sizeof(uint32_t) <= sizeof(s_a), "the candidates fit one staged tile");
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = ty + 16 * i, ga = ti * WORK_TILE + row;
        uint32_t lo = 0u, hi = 0u;
        uint32_t bu = 0u, be = 0u;
        int br = -1;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int gb = tj * WORK_TILE + tx + 16 * j;
            const uint32_t u = unl[i][j], e = eit[i][j];
            const bool valid = ga < R && gb < R;
            const bool alike = valid && (ga == gb || (e >= 1u && (unsigned long long)u * 1000000ull <= (unsigned long long)a.ppm * e));
            const uint32_t bit = (alike ? 1u : 0u) << (tx + 16 * (j & 1));
            if (j < 2) lo |= bit; else hi |= bit;
            const int cand = (valid && ga != gb && e >= 1u) ? gb : -1;
            if (work_nearer(u, e, cand, bu, be, br)) bu = u, be = e, br = cand;
        }
        if (lo) atomicOr(&s_adj[row][0], lo);
        if (hi) atomicOr(&s_adj[row][1], hi);
        s_cu[row][tx] = bu, s_ce[row][tx] = be, s_cr[row][tx] = br;
    }
    __syncthreads();
    if (tid < WORK_TILE) {
        const int ga = ti * WORK_TILE + tid;
        if (ga < R) {
            uint32_t bu = 0u, be = 0u;
            int br = -1;
            for (int k = 0; k < 16; k++)
                if (work_nearer(s_cu[tid][k], s_ce[tid][k], s_cr[tid][k], bu, be, br)) bu = s_cu[tid][k], be = s_ce[tid][k], br = s_cr[tid][k];
            const size_t at = (size_t)ga * (size_t)a.T + (size_t)tj;
            a.part[at] = make_uint4(bu, be, (uint32_t)br, 0u);
            a.adj[at] = (unsigned long long)s_adj[tid][0] | ((unsigned long long)s_adj[tid][1] << 32);
        }
    }
}

__global__ __launch_bounds__(WORK_GROUPS_THREADS) void k_work_groups(WorkArgs a) {
    constexpr int WAVES = WORK_GROUPS_THREADS / 64;
    __shared__ int s_label[NVRX_WORK_MAX_RANKS];
    __shared__ uint32_t s_size[NVRX_WORK_MAX_RANKS];
    __shared__ uint32_t s_red[4][WAVES];
    __shared__ int s_changed;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int R = a.R, T = a.T;
    for (int r = tid; r < R; r += WORK_GROUPS_THREADS) s_label[r] = r, s_size[r] = 0u;
    if (tid == 0) s_changed = 0;
    __syncthreads();
    for (int trip = 0; trip < R; trip++) {  // block-uniform
        bool changed = false;
        for (int r = tid; r < R; r += WORK_GROUPS_THREADS) {
            const int old = s_label[r];
            int m = old;
            const unsigned long long *__restrict__ row = a.adj + (size_t)r * (size_t)T;
            for (int j = 0; j < T; j++) {
                unsigned long long w = row[j];
                while (w) {
                    const int b = 64 * j + __builtin_ctzll(w);
                    w &= w - 1;
                    m = min(m, s_label[b]);  // (b < R: bits at or beyond R are clear)
                }
            }
            if (m < old) s_label[r] = m, changed = true;
        }
        __syncthreads();
        for (int r = tid; r < R; r += WORK_GROUPS_THREADS) {  // pointer jumping
            const int l = s_label[r], ll = s_label[l];
            if (ll < l) s_label[r] = ll, changed = true;
        }
        if (changed) s_changed = 1;
        __syncthreads();
        const int any = s_changed;
        __syncthreads();
        if (!any) break;
        if (tid == 0) s_changed = 0;  // (read by nobody before the next trip's barriers)
    }
    for (int r = tid; r < R; r += WORK_GROUPS_THREADS) atomicAdd(&s_size[s_label[r]], 1u);
    __syncthreads();
    uint32_t groups = 0, single = 0, largest = 0, with_data = 0;
    for (int r = tid; r < R; r += WORK_GROUPS_THREADS) {
        const int root = s_label[r];
        const uint32_t size = s_size[root];
        *reinterpret_cast<uint2 *>(a.rank + 8 * (size_t)r) = make_uint2((uint32_t)root, size);
        groups += root == r ? 1u : 0u;
        single += (root == r && size == 1u) ? 1u : 0u;
        largest = max(largest, size);
        const uint2 present = *reinterpret_cast<const uint2 *>(a.rank + 8 * (size_t)r + 6);
        with_data += (present.x | present.y) ? 1u : 0u;
    }
    groups = wave_sum_u32(groups), single = wave_sum_u32(single), with_data = wave_sum_u32(with_data);
    largest = wave_max_u32(largest);
    if (lane == 0) s_red[0][wave] = groups, s_red[1][wave] = single, s_red[2][wave] = largest, s_red[3][wave] = with_data;
    __syncthreads();
    if (tid == 0) {
        groups = single = largest = with_data = 0;
        for (int w = 0; w < WAVES; w++) {
            groups += s_red[0][w], single += s_red[1][w], with_data += s_red[3][w];
            largest = max(largest, s_red[2][w]);
        }
        *reinterpret_cast<uint4 *>(a.job) = make_uint4(groups, single, largest, with_data);
    }
}

__global__ __launch_bounds__(256) void k_work_rank(WorkArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (r >= a.R) return;  // wave-uniform
    const int T = a.T;
    uint32_t bits = 0u, bu = 0u, be = 0u;
    int br = -1;
    for (int j = lane; j < T; j += 64) {
        const size_t at = (size_t)r * (size_t)T + (size_t)j;
        bits += (uint32_t)__popcll(a.adj[at]);
        const uint4 p = a.part[at];
        if (work_nearer(p.x, p.y, (int)p.z, bu, be, br)) bu = p.x, be = p.y, br = (int)p.z;
    }
    bits = wave_sum_u32(bits);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t ou = (uint32_t)__shfl_xor((int)bu, off, 64), oe = (uint32_t)__shfl_xor((int)be, off, 64);
        const int orr = __shfl_xor(br, off, 64);
        if (work_nearer(ou, oe, orr, bu, be, br)) bu = ou, be = oe, br = orr;
    }
    if (lane == 0) {
        uint4 *rec = reinterpret_cast<uint4 *>(a.rank + 8 * (size_t)r);
        const uint2 comp = *reinterpret_cast<const uint2 *>(a.rank + 8 * (size_t)r);          // k_work_groups: {root, size}
        const uint2 present = *reinterpret_cast<const uint2 *>(a.rank + 8 * (size_t)r + 6);  // k_work_sig
        rec[0] = make_uint4(comp.x, comp.y, bits - 1u, (uint32_t)br);
        rec[1] = make_uint4(bu, be, present.x, present.y);
    }
}

// argument checks shared by both entry points (the pointers follow: out_check); nothing here touches a device
int work_check(int R, int K, int S, float count_tol, int max_unlike_ppm) {
    const int rc = table_check(R, K, S, 0, R);
    if (rc) return rc;
    if (R > NVRX_WORK_MAX_RANKS) return fail(NVRX_ERR_RANGE, "R=%d ranks, work groups take at most %d", R, NVRX_WORK_MAX_RANKS);
    if (!(count_tol >= 0.0f && count_tol <= 16.0f)) return fail(NVRX_ERR_RANGE, "count_tol=%g outside [0,16]", (double)count_tol);
    if (max_unlike_ppm < 0 || max_unlike_ppm > 1000000)
        return fail(NVRX_ERR_RANGE, "max_unlike_ppm=%d outside [0,1000000]", max_unlike_ppm);
    return NVRX_OK;
}

int work_launch(const float *d_table, int R, int K, int S, float count_tol, int max_unlike_ppm, void *d_out, hipStream_t st) {
    const WorkLayout l = work_layout(R, K, S);
    uint32_t *out = static_cast<uint32_t *>(d_out);
    WorkArgs a{};
    a.table = d_table;
    a.R = R, a.K = K, a.S = S, a.T = (R + WORK_TILE - 1) / WORK_TILE;
    a.factor = 1.0 + (double)count_tol;
    a.ppm = (uint32_t)max_unlike_ppm;
    a.sig_pad = l.sig_pad, a.adj_pad = l.adj_pad;
    a.sig = reinterpret_cast<float *>(out);
    a.adj = reinterpret_cast<unsigned long long *>(out + l.adj);
    a.part = reinterpret_cast<uint4 *>(out + l.part);
    a.rank = out + l.rank;
    a.job = out + l.job;
    hipLaunchKernelGGL(k_work_sig, dim3(R), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_work_pairs, dim3(a.T, a.T), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_work_groups, dim3(1), dim3(WORK_GROUPS_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_work_rank, dim3((R + 3) / 4), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_work_words(int R, int K, int S) {
    const int rc = table_check(R, K, S, 0, R);
    if (rc) return rc;
    if (R > NVRX_WORK_MAX_RANKS) return fail(NVRX_ERR_RANGE, "R=%d ranks, work groups take at most %d", R, NVRX_WORK_MAX_RANKS);
    return (int)work_layout(R, K, S).words;
}

int nvrx_work_groups(const float *d_table, int R, int K, int S, float count_tol, int max_unlike_ppm, void *d_out, void *stream) {
    const int rc = work_check(R, K, S, count_tol, max_unlike_ppm);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_table != nullptr, false)) return rc;
    return work_launch(d_table, R, K, S, count_tol, max_unlike_ppm, d_out, as_stream(stream));
}

int nvrx_report_work(nvrx_ctx *ctx, const nvrx_report_desc *desc, float count_tol, int max_unlike_ppm, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = work_check(desc->R, desc->K, desc->S, count_tol, max_unlike_ppm);
    if (rc) return rc;
    if (const int rc = out_check(d_out, true, true)) return rc;
    hipStream_t home = nullptr;
    const float *table = nullptr;
    if (const int rc = report_table(ctx, desc, &home, &table)) return rc;
    return work_launch(table, desc->R, desc->K, desc->S, count_tol, max_unlike_ppm, d_out, home);
}

}  // extern "C"
