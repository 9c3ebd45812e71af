// nvrx_comove.inl -- co-movement groups: WHICH ranks ran slow (or fast) at the same times.  Part of the translation unit
// nvrx_straggler.hip (included behind nvrx_timeline.inl: it reads that step's gathered blocks and uses its selections;
// nvrx_work.inl, further down, takes components_label from here).  The contract is in include/nvrx_straggler.h
// (nvrx_comove_groups).
//
// Every score rates a rank, or a node it was told about.  Sixteen ranks on two nodes that each dip 2 % in the same three
// buckets stay below every rank's own threshold; the evidence is that the ranks agree WITH EACH OTHER in time.  A rank's
// timeline is centred on the job's median per bucket, scaled to unit length, and the step is X . X^T over the ranks with an
// inner dimension of 64 buckets, thresholded in the accumulators, then connected components.
//
// k_comove_center<THREADS, NREG>  one workgroup per (bucket, family): the lower median of the rated ranks' levels, the wave
//   select up to 64 ranks and the register-fed radix select beyond (k_timeline_rank's choice).
// k_comove_unit   one wave per (rank, family), lane = bucket: the deviation, the f64 wave sum of squares, the peak and its
//   bucket by a wave max and a ballot; x and d leave as one coalesced 256-byte store each.
// k_comove_pairs  one workgroup of 256 per 64 x 64 tile of rank pairs, every tile of the T x T grid; wave w owns the 32 x 32
//   quadrant (w >> 1, w & 1) and runs 32 steps of v_mfma_f32_32x32x2_f32.
//   operands  v_mfma_f32_32x32x2_f32 takes A[i][k] from lane i + 32 k and B[k][j] from lane j + 32 k (i, j < 32, k < 2).  A
//             dot product does not mind in which order the buckets are walked as long as both operands walk alike, so lane l
//             loads the 32 CONTIGUOUS floats [32 (l / 32), 32 (l / 32) + 32) of row l % 32 -- eight 16-byte global loads, no
//             LDS -- and feeds its element t at step t: step t pairs buckets {t, 32 + t}.  Rows beyond R are clamped in the
//             load and zeroed, never skipped per lane.  s[i][j] and s[j][i] add the same products in the same order.
//   result    accumulator register v of lane l holds row 8 (v / 4) + (v % 4) + 4 (l / 32), column l % 32 of the quadrant
//             (the ISA's layout of a 32 x 32 f32 result: four row blocks of eight, each split between the wave's halves).
//             So ONE ballot over register v is two rows' 32-bit adjacency half-words: bits 0..31 row 8 (v / 4) + (v % 4),
//             bits 32..63 that row + 4.  Sixteen ballots are the quadrant; the half-words meet in 64 x 2 LDS words -- every
//             word has one writer -- and leave as one 8-byte store per row.  The R x R matrix is never written.
//   partner   per accumulator register a half-wave max of (s, the lower rank on a tie) over the 32 lanes of a row; the two
//             quadrants of a row meet in LDS and one {s, partner} per (row, tile) is stored.
// k_comove_groups  k_work_groups' label propagation (components_label, shared), then sizes and {root, size} per rank.
// k_comove_rank    one wave per rank: its degree, the T partial partners reduced, the 32-byte record as two 16-byte stores.
// No float atomics, no global atomics, no scratch.

namespace {

constexpr int COMOVE_TILE = 64;
constexpr int COMOVE_W = 64;  // floats of a unit timeline: buckets B..63 are zero
constexpr int COMOVE_GROUPS_THREADS = 1024;
constexpr int COMOVE_MIN_RATED = 3;  // ranks a bucket needs to have a centre
constexpr int COMOVE_RANK_WORDS = 8;
static_assert(TIMELINE_MAX_B <= COMOVE_W && NVRX_WORK_MAX_RANKS % COMOVE_TILE == 0, "one wave holds a timeline; tiles of 64 ranks");

// d_out in 32-bit words; every part starts on a 16-byte boundary (256, 16 R, 128 R and 4 R T are multiples of 4)
struct ComoveLayout {
    size_t center, rank, dev, unit, adj, part, words;
};

inline ComoveLayout comove_layout(int R) {
    const size_t r = (size_t)R, T = (r + COMOVE_TILE - 1) / COMOVE_TILE;
    ComoveLayout l;
    l.center = 0;                                // [2][64] f32 c, then [2][64] u32 rated ranks
    l.rank = 4 * COMOVE_W;                       // [2][R][8]
    l.dev = l.rank + 2 * COMOVE_RANK_WORDS * r;  // [2][R][64] f32 d
    l.unit = l.dev + 2 * COMOVE_W * r;           // [2][R][64] f32 x
    l.adj = l.unit + 2 * COMOVE_W * r;           // [2][R][T] u64
    l.part = l.adj + 4 * r * T;                  // [2][R][T] {f32 s, i32 partner}
    l.words = l.part + 4 * r * T;
    return l;
}

// Min-label propagation over adjacency bits with pointer jumping, until a block-wide "nothing changed" (at most R trips):
// thread r alone writes label r and labels only fall, towards the component's lowest rank, which is where every schedule
// ends.  Every thread of the workgroup calls it (barriers inside); s_label holds the roots behind it.
template <int THREADS>
__device__ __forceinline__ void components_label(const unsigned long long *__restrict__ adj, int R, int T, int *s_label,
                                                 int *s_changed) {
    const int tid = threadIdx.x;
    for (int r = tid; r < R; r += THREADS) s_label[r] = r;
    if (tid == 0) *s_changed = 0;
    __syncthreads();
    for (int trip = 0; trip < R; trip++) {  // block-uniform
        bool changed = false;
        for (int r = tid; r < R; r += THREADS) {
            const int old = s_label[r];
            int m = old;
            const unsigned long long *__restrict__ row = adj + (size_t)r * (size_t)T;
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
        for (int r = tid; r < R; r += THREADS) {  // pointer jumping
            const int l = s_label[r], ll = s_label[l];
            if (ll < l) s_label[r] = ll, changed = true;
        }
        if (changed) *s_changed = 1;
        __syncthreads();
        const int any = *s_changed;
        __syncthreads();
        if (!any) break;
        if (tid == 0) *s_changed = 0;  // (read by nobody before the next trip's barriers)
    }
}

struct ComoveUnitArgs {
    const float *blocks;  // [R][2][3][B]
    float *center;        // [2][64] c, then [2][64] u32 rated ranks
    uint32_t *rank;       // [2][R][8]
    float *dev, *unit;    // [2][R][64]
    int R, B;
    float min_rows, amplitude;
};

template <int THREADS, int NREG>
__global__ __launch_bounds__(THREADS) void k_comove_center(ComoveUnitArgs a) {
    constexpr int WAVES = THREADS / 64;
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[THREADS == 64 ? 4 : TAIL_BINS];
    __shared__ uint32_t s_wave[WAVES];
    __shared__ uint32_t s_sel[2];
    __shared__ uint32_t s_cnt[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = (int)blockIdx.x, fam = (int)blockIdx.y, B = a.B, R = a.R;
    float *c_out = a.center + fam * COMOVE_W + b;
    uint32_t *n_out = reinterpret_cast<uint32_t *>(a.center) + (2 + fam) * COMOVE_W + b;
    if (b >= B) {  // block-uniform: the words behind the window's buckets
        if (tid == 0) *c_out = 0.0f, *n_out = 0u;
        return;
    }
    const size_t pitch = (size_t)2 * TIMELINE_FIELDS * B;
    const float *__restrict__ col = a.blocks + (size_t)fam * TIMELINE_FIELDS * B + b;
    auto key_of = [&](int r) {  // a rated rank's level, the marker the selections skip elsewhere
        const float rows = col[(size_t)r * pitch], level = col[(size_t)r * pitch + B];
        return rows >= a.min_rows ? f2key(level) : PACE_MARK;
    };
    uint32_t n = 0, c = 0u;  // (+0.0 without a rated rank)
    if constexpr (THREADS == 64) {
        const uint32_t key = lane < R ? key_of(lane) : PACE_MARK;
        const bool has = key != PACE_MARK;
        const unsigned long long mask = __ballot(has);
        n = (uint32_t)__popcll(mask);
        if (n != 0) {  // wave-uniform
            const int ls = robust_wave_select(key, has, mask, (n - 1u) >> 1, R, lane);
            c = __float_as_uint(key2f((uint32_t)__builtin_amdgcn_readlane((int)key, ls)));
        }
    } else {
        uint32_t keys[NREG];
#pragma unroll
        for (int j = 0; j < NREG; j++) {
            const int r = tid + j * THREADS;
            keys[j] = r < R ? key_of(r) : PACE_MARK;
            n += keys[j] != PACE_MARK ? 1u : 0u;
        }
        n = wave_sum_u32(n);
        if (lane == 0) s_cnt[wave] = n;
        __syncthreads();
        n = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) n += s_cnt[w];
        n = uni(n);
        if (n != 0)  // block-uniform
            c = __float_as_uint(key2f(pace_radix_select<THREADS, NREG>([&](int j) { return keys[j]; }, R, (n - 1u) >> 1, s_hist,
                                                                       s_wave, s_sel)));
    }
    if (tid == 0) *c_out = __uint_as_float(c), *n_out = n;
}

__global__ __launch_bounds__(256) void k_comove_unit(ComoveUnitArgs a) {
    const int lane = threadIdx.x & 63, fam = (int)blockIdx.y, B = a.B;
    const int r = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (r >= a.R) return;  // wave-uniform
    const bool mine = lane < B;
    const int at = mine ? lane : 0;
    const float *__restrict__ own = a.blocks + ((size_t)r * 2 + fam) * TIMELINE_FIELDS * (size_t)B + at;
    const float rows = own[0], level = own[B];
    const float c = a.center[fam * COMOVE_W + at];
    const uint32_t n = reinterpret_cast<const uint32_t *>(a.center)[(2 + fam) * COMOVE_W + at];
    const bool on = mine && rows >= a.min_rows && n >= (uint32_t)COMOVE_MIN_RATED && c > 0.0f;
    const float d = on ? (float)(__ddiv_rn((double)level, (double)c) - 1.0) : 0.0f;
    const uint32_t mag = __float_as_uint(d) & 0x7FFFFFFFu;  // (|d| orders as its bit pattern)
    const uint32_t peak = wave_max_u32(mag);
    const int pb = __ffsll((long long)__ballot(mag == peak)) - 1;  // the lowest bucket at the peak (0 where all are 0)
    const bool active = __uint_as_float(peak) >= a.amplitude;     // (a NaN peak is inactive)
    const double ss = wave_sum_f64((double)d * (double)d);
    const float x = active ? (float)__ddiv_rn((double)d, __dsqrt_rn(ss)) : 0.0f;
    const float dp = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(d), pb));
    const size_t row = ((size_t)fam * a.R + r) * COMOVE_W + lane;
    a.unit[row] = x;
    a.dev[row] = d;
    if (lane == 0) {  // (words 0..4 are k_comove_groups' and k_comove_rank's)
        uint32_t *rec = a.rank + ((size_t)fam * a.R + r) * COMOVE_RANK_WORDS;
        rec[5] = peak;
        rec[6] = (uint32_t)pb | (active ? 0x100u : 0u);
        rec[7] = (uint32_t)(dp > 0.0f ? 1 : dp < 0.0f ? -1 : 0);
    }
}

struct ComovePairArgs {
    const float *x;           // [families][R][64]
    unsigned long long *adj;  // [families][R][T]
    uint2 *part;              // [families][R][T]
    uint32_t *rank;           // [families][R][8]
    int R, T;
    float thr;
    int keep_unit;  // words 5..7 of a rank record are k_comove_unit's (else they are written as 0)
};

typedef float comove_f32x16 __attribute__((ext_vector_type(16)));

// whether partner candidate 1 is better than candidate 2: the larger s, the lower rank on a tie; a rank of -1 is no candidate
__device__ __forceinline__ bool comove_better(float s1, int r1, float s2, int r2) {
    if (r1 < 0) return false;
    if (r2 < 0) return true;
    return s1 > s2 || (s1 == s2 && r1 < r2);
}

// a lane's 32 floats of its operand row, and whether any of them is nonzero
__device__ __forceinline__ bool comove_load(const float *__restrict__ x, int row, int R, int half, float (&v)[32]) {
    const float4 *__restrict__ src = reinterpret_cast<const float4 *>(x + (size_t)min(row, R - 1) * COMOVE_W + 32 * half);
    const bool ok = row < R;
    bool nz = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const float4 q = src[k];
        v[4 * k] = ok ? q.x : 0.0f, v[4 * k + 1] = ok ? q.y : 0.0f, v[4 * k + 2] = ok ? q.z : 0.0f, v[4 * k + 3] = ok ? q.w : 0.0f;
        nz = nz || v[4 * k] != 0.0f || v[4 * k + 1] != 0.0f || v[4 * k + 2] != 0.0f || v[4 * k + 3] != 0.0f;
    }
    return nz;
}

__global__ __launch_bounds__(256) void k_comove_pairs(ComovePairArgs a) {
    __shared__ uint32_t s_adj[COMOVE_TILE][2];
    __shared__ uint2 s_best[COMOVE_TILE][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = (int)uni((uint32_t)tid >> 6);
    const int qi = wave >> 1, qj = wave & 1, half = lane >> 5, col = lane & 31;
    const int ti = (int)blockIdx.y, tj = (int)blockIdx.x, fam = (int)blockIdx.z;
    const int R = a.R, T = a.T;
    const float *__restrict__ x = a.x + (size_t)fam * (size_t)R * COMOVE_W;
    const int i0 = ti * COMOVE_TILE + 32 * qi, j0 = tj * COMOVE_TILE + 32 * qj;  // the quadrant's first row and column
    float va[32], vb[32];
    const int nz_a = comove_load(x, i0 + col, R, half, va) ? 1 : 0;
    const int nz_b = comove_load(x, j0 + col, R, half, vb) ? 1 : 0;
    // a row's halves sit in lanes l and l + 32 (every lane takes part in the exchange: no short-circuit in front of it)
    const bool act_a = (nz_a | __shfl_xor(nz_a, 32, 64)) != 0;
    const bool act_b = (nz_b | __shfl_xor(nz_b, 32, 64)) != 0;
    const uint32_t rows_active = (uint32_t)__ballot(act_a);  // bit i: row i of the quadrant has a timeline
    comove_f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; v++) acc[v] = 0.0f;
#pragma unroll
    for (int t = 0; t < 32; t++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(va[t], vb[t], acc, 0, 0, 0);
    const int gj = j0 + col;
    const bool col_ok = gj < R && act_b;
#pragma unroll
    for (int v = 0; v < 16; v++) {
        const int i = 8 * (v >> 2) + (v & 3) + 4 * half;  // this lane's row of the quadrant in register v
        const int gi = i0 + i;
        const float s = acc[v];
        const bool cand = col_ok && gi < R && ((rows_active >> i) & 1u) != 0u && gi != gj;
        const unsigned long long edges = __ballot(cand && s >= a.thr);
        float bs = cand ? s : 0.0f;
        int br = cand ? gj : -1;
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) {  // (stays inside the half wave that holds the row)
            const float os = __shfl_xor(bs, off, 64);
            const int orr = __shfl_xor(br, off, 64);
            if (comove_better(os, orr, bs, br)) bs = os, br = orr;
        }
        if (col == 0) {  // lanes 0 and 32: one writer per (row, quadrant column)
            s_adj[32 * qi + i][qj] = half ? (uint32_t)(edges >> 32) : (uint32_t)edges;
            s_best[32 * qi + i][qj] = make_uint2(__float_as_uint(bs), (uint32_t)br);
        }
    }
    __syncthreads();
    if (tid < COMOVE_TILE) {
        const int gi = ti * COMOVE_TILE + tid;
        if (gi < R) {
            const uint2 p0 = s_best[tid][0], p1 = s_best[tid][1];
            const bool second = comove_better(__uint_as_float(p1.x), (int)p1.y, __uint_as_float(p0.x), (int)p0.y);
            const size_t at = ((size_t)fam * R + gi) * (size_t)T + (size_t)tj;
            a.part[at] = second ? p1 : p0;
            a.adj[at] = (unsigned long long)s_adj[tid][0] | ((unsigned long long)s_adj[tid][1] << 32);
        }
    }
}

__global__ __launch_bounds__(COMOVE_GROUPS_THREADS) void k_comove_groups(ComovePairArgs a) {
    __shared__ int s_label[NVRX_WORK_MAX_RANKS];
    __shared__ uint32_t s_size[NVRX_WORK_MAX_RANKS];
    __shared__ int s_changed;
    const int tid = threadIdx.x, fam = (int)blockIdx.x, R = a.R;
    for (int r = tid; r < R; r += COMOVE_GROUPS_THREADS) s_size[r] = 0u;
    components_label<COMOVE_GROUPS_THREADS>(a.adj + (size_t)fam * R * (size_t)a.T, R, a.T, s_label, &s_changed);
    for (int r = tid; r < R; r += COMOVE_GROUPS_THREADS) atomicAdd(&s_size[s_label[r]], 1u);
    __syncthreads();
    for (int r = tid; r < R; r += COMOVE_GROUPS_THREADS) {
        const int root = s_label[r];
        *reinterpret_cast<uint2 *>(a.rank + ((size_t)fam * R + r) * COMOVE_RANK_WORDS) = make_uint2((uint32_t)root, s_size[root]);
    }
}

__global__ __launch_bounds__(256) void k_comove_rank(ComovePairArgs a) {
    const int lane = threadIdx.x & 63, fam = (int)blockIdx.y;
    const int r = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (r >= a.R) return;  // wave-uniform
    const int T = a.T;
    uint32_t bits = 0u;
    float bs = 0.0f;
    int br = -1;
    for (int j = lane; j < T; j += 64) {
        const size_t at = ((size_t)fam * a.R + r) * (size_t)T + (size_t)j;
        bits += (uint32_t)__popcll(a.adj[at]);
        const uint2 p = a.part[at];
        if (comove_better(__uint_as_float(p.x), (int)p.y, bs, br)) bs = __uint_as_float(p.x), br = (int)p.y;
    }
    bits = wave_sum_u32(bits);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float os = __shfl_xor(bs, off, 64);
        const int orr = __shfl_xor(br, off, 64);
        if (comove_better(os, orr, bs, br)) bs = os, br = orr;
    }
    if (lane == 0) {
        uint4 *rec = reinterpret_cast<uint4 *>(a.rank + ((size_t)fam * a.R + r) * COMOVE_RANK_WORDS);
        const uint4 head = rec[0], tail = rec[1];  // k_comove_groups: {root, size}; k_comove_unit: words 5..7
        rec[0] = make_uint4(head.x, head.y, bits, (uint32_t)br);
        rec[1] = a.keep_unit ? make_uint4(__float_as_uint(bs), tail.y, tail.z, tail.w) : make_uint4(__float_as_uint(bs), 0u, 0u, 0u);
    }
}

// argument checks (nothing here touches a device)
int comove_shape_check(int R) {
    if (R <= 0) return fail(NVRX_ERR_INVALID, "bad table shape R=%d", R);
    if (R > NVRX_WORK_MAX_RANKS) return fail(NVRX_ERR_RANGE, "R=%d ranks, co-movement groups take at most %d", R, NVRX_WORK_MAX_RANKS);
    return NVRX_OK;
}

int comove_unit_check(int R, int B, uint32_t min_rows, uint32_t amplitude_ppm) {
    if (const int rc = comove_shape_check(R)) return rc;
    if (const int rc = timeline_b_check(B)) return rc;
    if (min_rows < 1u || min_rows > (uint32_t)NVRX_MAX_ROWS)
        return fail(NVRX_ERR_RANGE, "min_rows=%u outside [1,%d]", min_rows, NVRX_MAX_ROWS);
    if (amplitude_ppm < 1u || amplitude_ppm > 1000000u) return fail(NVRX_ERR_RANGE, "amplitude_ppm=%u outside [1,1000000]", amplitude_ppm);
    return NVRX_OK;
}

int comove_similarity_check(uint32_t similarity_ppm) {
    if (similarity_ppm < 1u || similarity_ppm > 1000000u)
        return fail(NVRX_ERR_RANGE, "similarity_ppm=%u outside [1,1000000]", similarity_ppm);
    return NVRX_OK;
}

int comove_ptr_check(const void *d_in, const void *d_out) {
    if (!d_in || !d_out) return fail(NVRX_ERR_INVALID, "null device pointer");
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return fail(NVRX_ERR_INVALID, "d_out is not 16-byte aligned");
    return NVRX_OK;
}

int comove_unit_launch(const float *d_blocks, int R, int B, uint32_t min_rows, uint32_t amplitude_ppm, uint32_t *out, hipStream_t st) {
    const ComoveLayout l = comove_layout(R);
    ComoveUnitArgs a{};
    a.blocks = d_blocks;
    a.center = reinterpret_cast<float *>(out + l.center), a.rank = out + l.rank;
    a.dev = reinterpret_cast<float *>(out + l.dev), a.unit = reinterpret_cast<float *>(out + l.unit);
    a.R = R, a.B = B;
    a.min_rows = (float)min_rows;  // (counts travel as floats: exact up to 2^24)
    a.amplitude = (float)((double)amplitude_ppm / 1e6);
    if (R <= 64)
        hipLaunchKernelGGL((k_comove_center<64, 1>), dim3(COMOVE_W, 2), dim3(64), 0, st, a);
    else
        hipLaunchKernelGGL((k_comove_center<256, 16>), dim3(COMOVE_W, 2), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_comove_unit, dim3((R + 3) / 4, 2), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}
static_assert(NVRX_WORK_MAX_RANKS <= 256 * 16, "k_comove_center<256, 16> keeps every rank's key in registers");

// pairs, components and records of `families` planes x [families][R][64]
int comove_pairs_launch(const float *d_x, int R, int families, uint32_t similarity_ppm, int keep_unit, uint32_t *out, hipStream_t st) {
    const ComoveLayout l = comove_layout(R);
    ComovePairArgs a{};
    a.x = d_x;
    a.adj = reinterpret_cast<unsigned long long *>(out + l.adj);
    a.part = reinterpret_cast<uint2 *>(out + l.part);
    a.rank = out + l.rank;
    a.R = R, a.T = (R + COMOVE_TILE - 1) / COMOVE_TILE;
    a.thr = (float)((double)similarity_ppm / 1e6);
    a.keep_unit = keep_unit;
    hipLaunchKernelGGL(k_comove_pairs, dim3(a.T, a.T, families), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_comove_groups, dim3(families), dim3(COMOVE_GROUPS_THREADS), 0, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_comove_rank, dim3((R + 3) / 4, families), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_comove_words(int R, int B) {
    if (const int rc = comove_shape_check(R)) return rc;
    if (const int rc = timeline_b_check(B)) return rc;
    return (int)comove_layout(R).words;
}

int nvrx_comove_unit(const float *d_blocks, int R, int B, uint32_t min_rows, uint32_t amplitude_ppm, void *d_out, void *stream) {
    if (const int rc = comove_unit_check(R, B, min_rows, amplitude_ppm)) return rc;
    if (const int rc = comove_ptr_check(d_blocks, d_out)) return rc;
    return comove_unit_launch(d_blocks, R, B, min_rows, amplitude_ppm, static_cast<uint32_t *>(d_out), as_stream(stream));
}

int nvrx_comove_pairs(const float *d_x, int R, uint32_t similarity_ppm, void *d_out, void *stream) {
    if (const int rc = comove_shape_check(R)) return rc;
    if (const int rc = comove_similarity_check(similarity_ppm)) return rc;
    if (const int rc = comove_ptr_check(d_x, d_out)) return rc;
    if (reinterpret_cast<uintptr_t>(d_x) & 15u) return fail(NVRX_ERR_INVALID, "d_x is not 16-byte aligned");
    return comove_pairs_launch(d_x, R, 1, similarity_ppm, 0, static_cast<uint32_t *>(d_out), as_stream(stream));
}

int nvrx_comove_groups(const float *d_blocks, int R, int B, uint32_t min_rows, uint32_t amplitude_ppm, uint32_t similarity_ppm,
                       void *d_out, void *stream) {
    if (const int rc = comove_unit_check(R, B, min_rows, amplitude_ppm)) return rc;
    if (const int rc = comove_similarity_check(similarity_ppm)) return rc;
    if (const int rc = comove_ptr_check(d_blocks, d_out)) return rc;
    uint32_t *out = static_cast<uint32_t *>(d_out);
    hipStream_t st = as_stream(stream);
    if (const int rc = comove_unit_launch(d_blocks, R, B, min_rows, amplitude_ppm, out, st)) return rc;
    return comove_pairs_launch(reinterpret_cast<const float *>(out + comove_layout(R).unit), R, 2, similarity_ppm, 1, out, st);
}

}  // extern "C"
