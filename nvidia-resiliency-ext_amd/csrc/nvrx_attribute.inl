// nvrx_attribute.inl -- kernel attribution: the top-N kernels behind each rank's GPU score.  Part of the translation unit
// nvrx_straggler.hip (included at its end: it uses that file's DPP reductions, column-minimum kernels and context).
//
// The GPU score of rank r (reporting.py:219-253; score_rank above) is g = sum_k(w_k * ref_k / med_k) / sum_k(w_k) over
// the eligible kernels.  Its deficit 1 - g = sum_k(n_k) / W with n_k = w_k * (1 - ref_k / med_k): the microseconds kernel k
// spent above the reference pace this window.  k_attribute lists, per rank and score family, the N kernels with the
// largest n_k by value (ties, -0.0 against +0.0 among them: the lower kernel id; NaN after -inf) as 16-byte records; the
// table is the one nvrx_score reads, nothing else is exchanged.
//
// One workgroup per (rank, family).  The selection needs no buffer proportional to K: N rounds of a block-wide arg-max
// over the key (order-preserving bits of the canonical f64 n_k -- canon_nk, nk2key -- then ~id), each round admitting only
// keys that order strictly after the previous winner.  A round is three 32-bit DPP wave maxima (high word, low word, ~id: a lexicographic
// maximum), one LDS slot per wave and one barrier (the slots alternate between two banks by round parity).  The n_k are
// recomputed every round: N * K f64 quotients per workgroup, spread over 256 or 1024 lanes.

namespace {

struct AttrArgs {
    const float *table;
    const float *minmed;  // [K] column minima of MED (NaN: some rank lacks the kernel); null when do_rel == 0
    int R, K, S;
    int first_rank;
    int top_n;
    int do_indiv, do_rel;
    uint4 *out;  // [n_ranks][2][1 + top_n]
};

// a < b  <=>  d2key(a) < d2key(b), as f2key does for f32
__device__ __forceinline__ uint64_t d2key(double d) {
    const uint64_t u = (uint64_t)__double_as_longlong(d);
    return u ^ ((u >> 63) ? 0xFFFFFFFFFFFFFFFFull : 0x8000000000000000ull);
}

// The n_k the order and the records see: the order is by VALUE, so -0.0 (a zero weight times a negative 1 - s_k) becomes
// +0.0 and ties with it, and every NaN (0/0, 0 * inf) becomes the one NaN that nk2key puts after -inf
__device__ __forceinline__ double canon_nk(double n) { return n != n ? (double)__builtin_nanf("") : (n == 0.0 ? 0.0 : n); }
__device__ __forceinline__ uint64_t nk2key(double n) { return n != n ? 0ull : d2key(n); }  // (d2key(-inf) > 0)

template <int NTHR>
__global__ __launch_bounds__(NTHR) void k_attribute(AttrArgs a) {
    constexpr int NW = NTHR / 64;
    __shared__ double s_sum[2][NW];
    __shared__ uint32_t s_cnt[NW];
    __shared__ uint32_t s_best[2][NW][4];  // [round parity][wave]{key high, key low, ~id, -}

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, KS = a.K + a.S;
    const int L = NVRX_TABLE_LEN(a.K, a.S);
    const int fam = blockIdx.y;  // 0 individual, 1 relative
    const int r = a.first_rank + (int)blockIdx.x;
    const float *__restrict__ row = a.table + (size_t)r * L;
    // the family's reference per kernel: this rank's history minimum / the column minimum over all ranks
    const float *__restrict__ ref = fam ? a.minmed : row + KS;
    const bool computed = fam ? a.do_rel != 0 : a.do_indiv != 0;
    uint4 *__restrict__ out = a.out + ((size_t)blockIdx.x * 2 + fam) * (size_t)(1 + a.top_n);
    const float NaN = __builtin_nanf("");

    // pass 1: W, sum of n_k and the number of eligible kernels (exactly the ones score_rank sums)
    double wsum = 0.0, nsum = 0.0;
    uint32_t cnt = 0;
    if (computed) {
        for (int k = tid; k < K; k += NTHR) {
            const float medf = row[k];
            if (!(medf >= 0.0f)) continue;
            const float rf = ref[k];
            if (fam && !(rf == rf)) continue;
            const double w = (double)row[2 * KS + k];
            const double s = (double)rf / (double)medf;
            wsum += w;
            nsum += w * (1.0 - s);
            cnt++;
        }
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
    wsum = nsum = 0.0;
    cnt = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        wsum += s_sum[0][w];
        nsum += s_sum[1][w];
        cnt += s_cnt[w];
    }
    if (cnt == 0) {  // block-uniform: the reference reports NaN here (no eligible kernel, family not computed)
        if (tid == 0) out[0] = make_uint4(__float_as_uint(NaN), __float_as_uint(NaN), 0u, __float_as_uint(0.0f));
        for (int j = tid; j < a.top_n; j += NTHR)
            out[1 + j] = make_uint4(0xFFFFFFFFu, __float_as_uint(NaN), __float_as_uint(NaN), __float_as_uint(NaN));
        return;
    }

    // N rounds of a block-wide arg-max; (ph, pl, pi) is the previous winner
    uint32_t ph = 0, pl = 0, pi = 0;
    double listed = 0.0;  // (thread 0) sum of the listed n_k
    for (int j = 0; j < a.top_n; j++) {
        uint32_t bh = 0, bl = 0, bi = 0;  // ~id of a real kernel is never 0: (0, 0, 0) is "no candidate"
        for (int k = tid; k < K; k += NTHR) {
            const float medf = row[k];
            if (!(medf >= 0.0f)) continue;
            const float rf = ref[k];
            if (fam && !(rf == rf)) continue;
            const double n = canon_nk((double)row[2 * KS + k] * (1.0 - (double)rf / (double)medf));
            const uint64_t key = nk2key(n);
            const uint32_t kh = (uint32_t)(key >> 32), kl = (uint32_t)key, ki = ~(uint32_t)k;
            // strictly after the previous winner ...
            if (j > 0 && !(kh < ph || (kh == ph && (kl < pl || (kl == pl && ki < pi))))) continue;
            // ... and the best of this thread so far
            if (kh > bh || (kh == bh && (kl > bl || (kl == bl && ki > bi)))) bh = kh, bl = kl, bi = ki;
        }
        // lexicographic maximum over the wave: the word that decides is masked out in the lanes that lost before it
        const uint32_t mh = wave_max_u32(bh);
        const uint32_t ml = wave_max_u32(bh == mh ? bl : 0u);
        const uint32_t mi = wave_max_u32((bh == mh && bl == ml) ? bi : 0u);
        if (lane == 0) {
            s_best[j & 1][wave][0] = mh;
            s_best[j & 1][wave][1] = ml;
            s_best[j & 1][wave][2] = mi;
        }
        __syncthreads();
        ph = pl = pi = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const uint32_t h = s_best[j & 1][w][0], l = s_best[j & 1][w][1], i = s_best[j & 1][w][2];
            if (h > ph || (h == ph && (l > pl || (l == pl && i > pi)))) ph = h, pl = l, pi = i;
        }
        if (pi == 0) {  // block-uniform: fewer than N eligible kernels, the remaining ids are -1
            for (int q = j + tid; q < a.top_n; q += NTHR)
                out[1 + q] = make_uint4(0xFFFFFFFFu, __float_as_uint(NaN), __float_as_uint(NaN), __float_as_uint(NaN));
            break;
        }
        if (tid == 0) {
            const int k = (int)~pi;
            const double w = (double)row[2 * KS + k];
            const double s = (double)ref[k] / (double)row[k];
            const double n = canon_nk(w * (1.0 - s));
            listed += n;
            out[1 + j] = make_uint4((uint32_t)k, __float_as_uint((float)(n / wsum)), __float_as_uint((float)s),
                                    __float_as_uint((float)n));
        }
    }
    if (tid == 0)
        out[0] = make_uint4(__float_as_uint((float)(nsum / wsum)), __float_as_uint((float)(listed / wsum)), cnt,
                            __float_as_uint((float)wsum));
}

// Column minima of the K kernel medians into scratch[0, K) (scratch: NVRX_ATTR_SCRATCH_FLOATS(K) floats), as score_launch
// takes them beyond 64 ranks: the kernels' columns are the first K of every table row.
int attr_colmin(const float *d_table, int R, int K, int S, float *scratch, hipStream_t st) {
    const int L = NVRX_TABLE_LEN(K, S);
    if (R > 64) {
        const int chunks = std::max(1, std::min(COLMIN_MAX_CHUNKS, (R + 63) / 64));
        const int rows_per_chunk = (R + chunks - 1) / chunks;
        float *part = scratch + K;
        hipLaunchKernelGGL(k_colmin_part, dim3((K + 63) / 64, chunks), dim3(256), 0, st, d_table, R, K, L, rows_per_chunk, part);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_colmin_finish, dim3((K + 255) / 256), dim3(256), 0, st, part, chunks, K, scratch);
    } else {
        hipLaunchKernelGGL(k_colmin, dim3((K + 255) / 256), dim3(256), 0, st, d_table, R, K, L, scratch);
    }
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

// argument checks shared by both entry points; nothing here touches a device
int attr_check(int R, int K, int S, int first_rank, int n_ranks, int top_n) {
    if (R <= 0 || K < 0 || S < 0) return fail(NVRX_ERR_INVALID, "bad table shape R=%d K=%d S=%d", R, K, S);
    if (K > NVRX_MAX_ROWS) return fail(NVRX_ERR_RANGE, "K=%d kernel ids, at most %d", K, NVRX_MAX_ROWS);
    if (top_n < 1 || top_n > NVRX_ATTR_MAX_TOP) return fail(NVRX_ERR_RANGE, "top_n=%d outside [1,%d]", top_n, NVRX_ATTR_MAX_TOP);
    if (first_rank < 0 || n_ranks < 1 || first_rank > R - n_ranks)
        return fail(NVRX_ERR_RANGE, "ranks [%d,%d+%d) outside the table's %d", first_rank, first_rank, n_ranks, R);
    return NVRX_OK;
}

int attr_launch(const float *d_table, int R, int K, int S, int first_rank, int n_ranks, int top_n, int do_indiv, int do_rel,
                float *d_minmed_scratch, void *d_out, hipStream_t st) {
    const bool rel = do_rel && K > 0;
    if (rel) {
        const int rc = attr_colmin(d_table, R, K, S, d_minmed_scratch, st);
        if (rc) return rc;
    }
    AttrArgs a{};
    a.table = d_table;
    a.minmed = rel ? d_minmed_scratch : nullptr;
    a.R = R, a.K = K, a.S = S;
    a.first_rank = first_rank;
    a.top_n = top_n;
    a.do_indiv = do_indiv;
    a.do_rel = rel ? 1 : 0;  // (K == 0: no eligible kernel either way)
    a.out = static_cast<uint4 *>(d_out);
    if (K > 1024)
        hipLaunchKernelGGL(k_attribute<1024>, dim3(n_ranks, 2), dim3(1024), 0, st, a);
    else
        hipLaunchKernelGGL(k_attribute<256>, dim3(n_ranks, 2), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return NVRX_OK;
}

}  // namespace

extern "C" {

int nvrx_attribute(const float *d_table, int R, int K, int S, int first_rank, int n_ranks, int top_n, int do_indiv,
                   int do_rel, float *d_minmed_scratch, void *d_out, void *stream) {
    const int rc = attr_check(R, K, S, first_rank, n_ranks, top_n);
    if (rc) return rc;
    if (const int rc = out_check(d_out, d_table != nullptr, false)) return rc;
    if (do_rel && K > 0 && !d_minmed_scratch) return fail(NVRX_ERR_INVALID, "the relative family needs d_minmed_scratch");
    return attr_launch(d_table, R, K, S, first_rank, n_ranks, top_n, do_indiv, do_rel, d_minmed_scratch, d_out, as_stream(stream));
}

int nvrx_report_attribute(nvrx_ctx *ctx, const nvrx_report_desc *desc, int first_rank, int n_ranks, int top_n, void *d_out) {
    if (!ctx || !desc) return fail(NVRX_ERR_INVALID, "null argument");
    const int rc = attr_check(desc->R, desc->K, desc->S, first_rank, n_ranks, top_n);
    if (rc) return rc;
    if (const int rc = out_check(d_out, true, true)) return rc;
    hipStream_t home = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);  // (held on: the scratch below is the context's)
        if (const int rc = behind_report(ctx, desc, &home)) return rc;
        if (desc->do_rel && desc->K > 0 && ctx->attr_scratch_elems < (size_t)NVRX_ATTR_SCRATCH_FLOATS(desc->K)) {
            // (hipFree waits for the device: nothing still reads the old buffer; every user is on `home`)
            if (ctx->attr_scratch) HIP_TRY(hipFree(ctx->attr_scratch));
            ctx->attr_scratch = nullptr, ctx->attr_scratch_elems = 0;
            const size_t need = std::max<size_t>(NVRX_ATTR_SCRATCH_FLOATS(desc->K), 4096);
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ctx->attr_scratch), need * sizeof(float)));
            ctx->attr_scratch_elems = need;
        }
    }
    const int K = desc->K;
    float *scratch = ctx->attr_scratch;
    const float *table = desc->allgather_fn ? desc->d_table : desc->d_send;
    return attr_launch(table, desc->R, K, desc->S, first_rank, n_ranks, top_n, desc->do_indiv, desc->do_rel, scratch, d_out, home);
}

}  // extern "C"
