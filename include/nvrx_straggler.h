/*
 * nvrx_straggler.h -- C ABI of libnvrx_straggler_hip.so, the MI355X-native (gfx950 HIP) engine behind
 * the straggler-detection scoring hot path of nvidia-resiliency-ext.
 *
 * The reference has NO C/FFI operator interface for this path: its boundary is (1) the public Python
 * API (straggler.Detector / ReportGenerator / Report) and (2) the pybind11 native module
 * `nvrx_cupti_module` (cupti_src/cupti_module_py.cpp:33-55).  This library sits below both; the Python
 * package in nvidia-resiliency-ext_amd/ keeps (1) and (2) intact and calls the entry points below via
 * ctypes.  Each entry point cites the reference code it replaces; paths are relative to
 * /root/reference/src/nvidia_resiliency_ext/attribution/straggler/ .
 *
 * Conventions: plain C, no exceptions across the ABI, no Python/torch types.  Every function returns
 * 0 (NVRX_OK) or a negative errno-style code; nvrx_last_error() returns the calling thread's last
 * message.  Device buffers named d_* are caller-owned HIP device pointers (e.g. tensor.data_ptr());
 * `stream` is a hipStream_t passed as void* (0 = the null stream).  A context is thread-compatible:
 * calls on one context must be serialised by the caller (the Python layer holds a lock, as the
 * reference's CuptiManager does, cupti.py:44).
 */
#ifndef NVRX_STRAGGLER_H
#define NVRX_STRAGGLER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVRX_ABI_VERSION 2

#define NVRX_OK 0
#define NVRX_ERR_INVALID (-22) /* bad argument (EINVAL) */
#define NVRX_ERR_NOMEM (-12)   /* host or device allocation failed (ENOMEM) */
#define NVRX_ERR_HIP (-5)      /* a HIP runtime call failed (EIO); see nvrx_last_error() */
#define NVRX_ERR_STATE (-1)    /* call not valid in the current state (EPERM) */
#define NVRX_ERR_RANGE (-34)   /* size outside what the kernels support (ERANGE) */
#define NVRX_ERR_TIMEOUT (-62) /* wait timed out (ETIME) */

/* Row statistics layout: NVRX_STATS_STRIDE floats per row.
 * Mirrors the Statistic enum (statistics.py:19-35) + the kernel weight NUM*AVG (reporting.py:246).
 * Word 7 has no name: the statistics kernel stores there, as a float, the path its selection of the median took --
 *   0       nothing was selected (no samples, or all samples equal)
 *   1       the range estimated from the row's first tile held
 *   2       the median fell into an edge bin of that estimate: the histogram was rebuilt over the row's exact range
 *   +4      the median's bin was too heavy to rank and was refined (5 = 1+4, 6 = 2+4, 22 = 18+4)
 *   18      (16|2) a sample with the sign bit set: the row was re-keyed, which always rebuilds over the exact range
 * It is a diagnostic and no caller should act on it, but the tests rely on it: tests/test_gpu_row_stats_paths.py compares
 * it, row by row, with a model of the selection's control flow to show that every path ran in every launch shape. */
#define NVRX_STATS_STRIDE 8
#define NVRX_STAT_MIN 0
#define NVRX_STAT_MAX 1
#define NVRX_STAT_MED 2
#define NVRX_STAT_AVG 3
#define NVRX_STAT_STD 4
#define NVRX_STAT_NUM 5
#define NVRX_STAT_WEIGHT 6

/* Row kinds select which of the reference's two statistics conventions applies. */
#define NVRX_KIND_SECTION 0 /* straggler.py:185-195: LOWER median, UNBIASED std (NaN if n==1) */
#define NVRX_KIND_KERNEL 1  /* CuptiProfiler.cpp:44-74: mean-of-middles median, POPULATION std */

/* Largest row (samples per ring) the statistics kernel keeps resident in registers. */
#define NVRX_MAX_RING_CAP 65536
#define NVRX_MAX_ROWS 65536

/* Exchange-table row length for K kernel ids and S section ids (see nvrx_score). */
#define NVRX_TABLE_LEN(K, S) (2 * ((K) + (S)) + (K) + 1)
/* Score row length: {gpu_indiv, gpu_rel, indiv[S], rel[S]}  (reporting.py:353-360). */
#define NVRX_SCORE_LEN(S) (2 + 2 * (S))
/* Number of uint32 words of score-kernel metadata. */
#define NVRX_META_WORDS 8

typedef struct nvrx_ctx nvrx_ctx;

/* ------------------------------------------------------------------------------------------------
 * Library
 * ---------------------------------------------------------------------------------------------- */
int nvrx_abi_version(void);
/* Message of the last failing call made by the calling thread ("" if none). */
const char *nvrx_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Stateless operators (caller-owned device buffers).  These are the kernels; the context API below
 * only adds ring storage, staging and event timing around them.
 * ---------------------------------------------------------------------------------------------- */

/* Per-row statistics of `rows` timing rows, one workgroup per row.
 *   d_samples [rows][row_stride] f32, row_stride % 4 == 0 and base 16-byte aligned;
 *   d_counts  [rows] valid samples per row (clamped to row_stride; 0 => NaN stats, NUM 0);
 *   d_kinds   [rows] NVRX_KIND_* per row, or NULL for all-section;
 *   d_stats   [rows][NVRX_STATS_STRIDE] f32 out.
 * Replaces Detector._get_section_summaries (straggler.py:172-197: torch.tensor(deque) + min/max/
 * median/mean/std per section) and computeStats (CuptiProfiler.cpp:44-74: std::sort + stats per
 * kernel).  MIN/MAX/MED/NUM are exact; AVG/STD are accumulated in f64 and rounded to f32. */
int nvrx_row_stats(const float *d_samples, const uint32_t *d_counts, const uint8_t *d_kinds, int rows,
                   int row_stride, float *d_stats, void *stream);

/* Cross-rank scoring of the exchanged table, for all R ranks at once.
 *   d_table [R][L] f32, L = NVRX_TABLE_LEN(K,S); per rank r:
 *      med  [0, K+S)            MED per id (kernel ids first, then section ids); -1 = no stats
 *      hmin [K+S, 2(K+S))       running minimum of MED on rank r (individual-score reference)
 *      w    [2(K+S), 2(K+S)+K)  kernel weights NUM*AVG
 *      flag [L-1]               1.0 if rank r has ids for all its names, else 0.0
 *   thresholds[4] = {gpu_rel, section_rel, gpu_indiv, section_indiv} (Report.identify_stragglers
 *      argument order, reporting.py:84-90); NULL => 0.75 each;
 *   d_scores [R][NVRX_SCORE_LEN(S)] f32 out, NaN where the reference reports NaN / nothing.  When d_scores and
 *      d_flags are both 16-byte aligned they are written in 16-byte units (R <= 64: one workgroup scores the whole
 *      table; larger jobs: one workgroup per tile of 16 ranks): pad each array to a multiple of 16 bytes;
 *   d_flags  [R][NVRX_SCORE_LEN(S)] u8 out, 1 where score < threshold (strict; NaN never flagged);
 *   d_meta   [NVRX_META_WORDS] u32 out: {all ranks' name flags set, R, K, S, seq, seq of the statistics rows,
 *      wait for the rows [10 ns ticks], (last row -> scores staged) << 16 | (last row -> completion word) [10 ns ticks, 16 bits each]}
 *      (the last two: single-workgroup kernel only);
 *   d_done_counter  device word (zero before the first launch) or NULL.  When given, d_scores /
 *      d_flags / d_meta may point into pinned host memory (nvrx_host_alloc): after every block's
 *      results are visible system-wide the kernel stores `seq` into d_meta[4] with release
 *      semantics, so a host thread can wait with nvrx_poll_u32 instead of a stream sync + D2H.
 *   d_stats_src / d_stats_dst / stats_rows  optional: the kernel also forwards `stats_rows`
 *      statistics rows (16-byte aligned) from device memory to d_stats_dst (pinned host memory), so
 *      they arrive with the scores under the same completion word.
 * Replaces _all_reduce_times (reporting.py:255-296), _compute_sections_perf_scores (:196-217),
 * _compute_gpu_perf_score (:219-253), _get_tensor_from_scores/_get_scores_from_tensor (:338-380) and
 * the thresholding of Report.identify_stragglers (:84-151). */
int nvrx_score(const float *d_table, int R, int K, int S, int do_indiv, int do_rel,
               const double *thresholds, float *d_scores, uint8_t *d_flags, uint32_t *d_meta,
               uint32_t *d_done_counter, uint32_t seq, const float *d_stats_src, float *d_stats_dst,
               int stats_rows, void *stream);

/* Which kernels nvrx_score / a report would launch for this shape and these result arrays; touches no device.  This IS the
 * dispatch (nvrx_score switches on it), so a test can assert the route it believes it covers:
 *   SINGLE    R <= 64, staged results + column minima within 60 KB of LDS, both arrays 16-byte aligned: one workgroup;
 *   ROWS      otherwise R <= 64 and (K+S)*4 <= 48 KB: one workgroup per rank, column minima in its own LDS;
 *   ROWS_PRE  (K+S)*4 > 48 KB at R <= 64, or R > 64 where no tile fits or an array is unaligned: column minima in a
 *             two-level pass of their own, then one workgroup per rank;
 *   TILE16    R > 64, aligned arrays, 16 score rows fit 48 KB of LDS (S <= 306): that pass, then 16 ranks per workgroup;
 *   TILE8     R > 64, aligned arrays, only 8 rows fit (307 <= S <= 613): the same with 8 ranks per workgroup.
 * NVRX_ERR_INVALID for R <= 0, K < 0 or S < 0. */
#define NVRX_SCORE_ROUTE_SINGLE 1
#define NVRX_SCORE_ROUTE_ROWS 2
#define NVRX_SCORE_ROUTE_ROWS_PRE 3
#define NVRX_SCORE_ROUTE_TILE16 4
#define NVRX_SCORE_ROUTE_TILE8 5
int nvrx_score_route(int R, int K, int S, const void *d_scores, const void *d_flags);

/* Kernel attribution: which kernels carry each rank's GPU score deficit.  Extends _compute_gpu_perf_score
 * (reporting.py:219-253), whose weighted mean g = sum_k(w_k * ref_k / med_k) / W keeps no per-kernel term: with
 * s_k = ref_k / med_k and n_k = w_k * (1 - s_k) ("lost microseconds": time above the reference pace), 1 - g = sum_k(n_k) / W.
 * Per reported rank and family (0 individual: ref_k = hmin; 1 relative: ref_k = column minimum of MED, NaN if any rank lacks
 * the kernel) the top_n eligible kernels by n_k, descending, ties to the lower kernel id.  Eligible = what nvrx_score sums.
 * The order is by VALUE: -0.0 and +0.0 tie (a zero n_k is recorded as +0.0), and a NaN n_k (0/0 from a zero median, 0 * inf
 * under a zero weight) comes after -inf whatever its sign bit, NaN among themselves by kernel id.
 *   d_table [R][L] as for nvrx_score; ranks [first_rank, first_rank + n_ranks) are reported;
 *   top_n in [1, NVRX_ATTR_MAX_TOP];
 *   d_minmed_scratch  NVRX_ATTR_SCRATCH_FLOATS(K) floats of device memory (column minima), may be NULL when do_rel == 0;
 *   d_out [n_ranks][2][1 + top_n] records of four 32-bit words, 16-byte aligned (NVRX_ATTR_WORDS(n_ranks, top_n) words):
 *      header {f32 deficit = sum(n_k)/W, f32 explained = sum of the listed shares, u32 eligible kernels, f32 W}
 *      entry  {i32 kernel id, f32 share = n_k/W, f32 score = s_k, f32 lost_us = n_k}
 *      no eligible kernel / family not computed: header {NaN, NaN, 0, 0}, every id -1; fewer than top_n eligible kernels:
 *      the remaining ids are -1 (their floats NaN).  s_k and n_k are the f64 formula rounded to f32.
 * Argument errors (NVRX_ERR_INVALID / NVRX_ERR_RANGE) are reported before any device is touched. */
#define NVRX_ATTR_MAX_TOP 16
#define NVRX_ATTR_SCRATCH_FLOATS(K) (33 * (size_t)(K))
#define NVRX_ATTR_WORDS(n_ranks, top_n) ((size_t)(n_ranks) * 2 * (1 + (size_t)(top_n)) * 4)
int nvrx_attribute(const float *d_table, int R, int K, int S, int first_rank, int n_ranks, int top_n, int do_indiv,
                   int do_rel, float *d_minmed_scratch, void *d_out, void *stream);

/* Tail quantile of timing rows.  Extends the statistics of straggler.py:172-197, whose only order statistic is the median:
 * per row the nearest-rank q-quantile, q = q_ppm / 1e6 with q_ppm in [500000, 999999] -- the element of rank
 * k = (q_ppm * n + 999999) / 1000000 - 1 (64-bit integers) of the row's n valid samples sorted ascending by their raw bit
 * patterns (-inf < negatives < -0.0 < +0.0 < positives < +inf < NaN with a clear sign bit): always an actual sample, for
 * section and kernel rows alike.  At q_ppm = 500000 that is the lower median, the MED of a section row.
 *   d_samples [rows][row_stride], 16-byte aligned, row_stride % 4 == 0, at most NVRX_MAX_RING_CAP; d_counts [rows];
 *   d_out [rows]: -1.0 where the row holds no sample.  Stateless: caller-owned buffers, like nvrx_row_stats.
 * Argument errors (NVRX_ERR_INVALID / NVRX_ERR_RANGE) are reported before any device is touched. */
int nvrx_row_quantile(const float *d_samples, const uint32_t *d_counts, int rows, int row_stride, uint32_t q_ppm,
                      float *d_out, void *stream);
/* Relative tail scores.  Extends _compute_section_relative_scores / _compute_gpu_perf_score (reporting.py:196-253) from
 * medians to tails: d_tails [R][K+S] holds every rank's tail per kernel id and section id (-1.0: none).  Reference per
 * column = the minimum over all R ranks, NaN if any rank has none.  Per reported rank [first_rank, first_rank + n_ranks):
 *   d_out [n_ranks][1 + S] = {GPU tail score, section tail score[S]}
 *   section s: f32 of the f64 quotient ref / tail, NaN where either is missing;
 *   GPU: f32 of sum_k w_k * (ref_k / tail_k) / sum_k w_k in f64 over the kernels with a tail and a reference, w_k the
 *   weights NUM*AVG of that rank in d_table [R][L] (the table nvrx_score reads); NaN when no kernel is eligible.
 *   d_colmin_scratch  NVRX_ATTR_SCRATCH_FLOATS(K+S) floats of device memory.
 * Argument errors (NVRX_ERR_INVALID / NVRX_ERR_RANGE) are reported before any device is touched. */
int nvrx_tail_score(const float *d_tails, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                    float *d_colmin_scratch, float *d_out, void *stream);

/* Onset of a change in timing rows: SINCE WHEN a row is slow.  Extends the statistics of straggler.py:172-197, which are
 * order statistics and do not look at the order of the samples.  Per row with n valid samples:
 *   time order  sample i lives in slot (start + i) mod n, 0 <= start < n (a larger start is taken modulo n): start is 0 for a
 *               ring that has not wrapped since its last reset, total % ring_cap for a wrapped one (then n == ring_cap);
 *   pivoting    d_i = (f64)x_i - (f64)x_0; all sums below are f64 sums of d; T = sum of all d_i, C_t = sum of d_0 .. d_(t-1);
 *   m           max(8, (min_seg_ppm * n + 999999) / 1000000) (64-bit integers), min_seg_ppm in [1, 500000];
 *   D_t         t * (n - t) / n * (after_t - before_t)^2 for every split t in [m, n - m], before_t = C_t / t and
 *               after_t = (T - C_t) / (n - t) the pivoted means of x[0..t) and x[t..n): the least-squares single change point;
 *   t*          the split with the largest D_t, the lowest t on ties;
 *   strength    D_t* / SST, SST = sum of (d_i - T / n)^2: the share of the row's variance that one step explains, in [0, 1].
 * Row record, 16 bytes: {u32 ago = n - t*, f32 before = x_0 + before_t*, f32 after = x_0 + after_t*, f32 strength} -- "the
 * change happened `ago` samples ago".
 *   n == 0 (an absent row)      {0, -1, -1, -1};
 *   T or SST not finite         {0, NaN, NaN, NaN};
 *   0 < n < 2m (no onset)       {0, mean, mean, 0}, mean = x_0 + T / n;
 *   SST == 0 (a constant row)   {n - m, x_0, x_0, 0}: t* = m.
 * Effective shift of a record: e = f32 of the f64 quotient after / before (the record's f32 values) where
 * strength >= min_strength and after > before > 0; 1.0 otherwise ("did not shift"); -1.0 for an absent row.
 *   d_samples [rows][row_stride], 16-byte aligned, row_stride % 4 == 0, at most NVRX_MAX_RING_CAP; d_counts [rows];
 *   d_starts [rows] or NULL (0 everywhere); d_out [rows] records, 16-byte aligned.  Stateless, like nvrx_row_quantile.
 * Argument errors (NVRX_ERR_INVALID / NVRX_ERR_RANGE) are reported before any device is touched. */
int nvrx_row_onset(const float *d_samples, const uint32_t *d_counts, const uint32_t *d_starts, int rows, int row_stride,
                   uint32_t min_seg_ppm, void *d_out, void *stream);
/* Relative onset scores.  d_onset [R][NVRX_ONSET_PLANES][K+S]: per rank six planes {e, before, after, strength, ago as f32,
 * n as f32} per kernel id and section id (-1.0: none; n, the row's sample count, travels along so that "ago" can be read
 * against the window of a rank other than one's own); only plane 0 is read.  Reference per column = the minimum of e over all R ranks, NaN if any
 * rank has none.  Per reported rank [first_rank, first_rank + n_ranks), nvrx_tail_score's arithmetic on e:
 *   d_out [n_ranks][1 + S] = {GPU onset score, section onset score[S]}
 *   section s: f32 of the f64 quotient ref / e, NaN where either is missing;
 *   GPU: f32 of sum_k w_k * (ref_k / e_k) / sum_k w_k in f64, w_k the weights NUM*AVG of that rank in d_table [R][L].
 * Scores are in (0, 1]: 1 = "shifted no more than the steadiest rank"; a phase change of the whole job flags nobody.
 *   d_colmin_scratch  NVRX_ATTR_SCRATCH_FLOATS(K+S) floats of device memory.
 * Argument errors (NVRX_ERR_INVALID / NVRX_ERR_RANGE) are reported before any device is touched. */
#define NVRX_ONSET_PLANES 6
int nvrx_onset_score(const float *d_onset, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                     float *d_colmin_scratch, float *d_out, void *stream);

/* Period of timing rows: whether a row is slow ON A BEAT -- a stall every P-th sample (a data-loader refill, a host-side GC, a
 * log flush, a per-rank checkpoint shard).  Medians, tails, robust scores and onsets cannot see it: one slow sample in fifty
 * moves no median and no 0.95-quantile, and a spike train is no step.  Per row with n valid samples:
 *   time order  as for nvrx_row_onset: sample i lives in slot (start + i) mod n;
 *   pivoting    d_i = (f64)x_i - (f64)x_0; all sums below are f64 sums of d; T = sum of all d_i, SST = sum of (d_i - T / n)^2;
 *   candidates  P in [2, Pmax], Pmax = min(max_period, n / NVRX_PERIOD_MIN_CYCLES) (integer division; fewer than four
 *               repetitions are not a beat), max_period in [2, NVRX_PERIOD_MAX];
 *   fold at P   the phase of sample i is i mod P; S_f = the sum of the d_i of phase f, n_f their count;
 *               B_P = sum_f S_f^2 / n_f - T^2 / n; eta2_P = B_P / SST, the share of the row's variance that the P phase
 *               means explain; a_P = 1 - (1 - eta2_P) * (n - 1) / (n - P), the adjusted R^2 (unadjusted, pure noise explains
 *               (P - 1) / (n - 1));
 *   P*          a_max = the largest a_P; no period if a_max <= 0; else the SMALLEST P with a_P >= NVRX_PERIOD_BAR * a_max (a
 *               fold at any multiple of the true period explains as much as the true one, a divisor P / k at most 1 / k:
 *               the rule lands on the fundamental.  0.95 is a rule, not a measurement);
 *   at P*       f* = the phase with the largest mean S_f / n_f (the lowest f on ties); peak = x_0 + S_f* / n_f*;
 *               rest = x_0 + (T - S_f*) / (n - n_f*); ago = (n - 1 - f*) mod P*, the samples since the slow phase last occurred;
 *               strength = a_P*.
 * Row record, 16 bytes: {u32 period | ago << 16, f32 peak, f32 rest, f32 strength}.
 *   n == 0 (an absent row)        {0, -1, -1, -1};
 *   T or SST not finite           {0, NaN, NaN, NaN};
 *   Pmax < 2, or a_max <= 0       {0, mean, mean, 0}, mean = x_0 + T / n;
 *   SST == 0 (a constant row)     {0, x_0, x_0, 0}.
 * Effective excess of a record: e = f32 of the f64 quotient peak / rest (the record's f32 values) where period > 0,
 * strength >= min_strength and peak > rest > 0; 1.0 otherwise ("no beat"); -1.0 for an absent row.
 * Periods are counted in samples of that row: report-window samples, traced entries with a thinned tracer.  Only the
 * strongest beat of a row is reported, and a row that also stepped has an SST the step dominates: its beat reads weak.
 *   d_samples [rows][row_stride], 16-byte aligned, row_stride % 4 == 0, at most NVRX_MAX_RING_CAP; d_counts [rows];
 *   d_starts [rows] or NULL (0 everywhere); d_out [rows] records, 16-byte aligned.  Stateless, like nvrx_row_onset.
 * Argument errors (NVRX_ERR_INVALID / NVRX_ERR_RANGE) are reported before any device is touched. */
#define NVRX_PERIOD_MIN_CYCLES 4
#define NVRX_PERIOD_MAX 4096
#define NVRX_PERIOD_BAR 0.95
int nvrx_row_period(const float *d_samples, const uint32_t *d_counts, const uint32_t *d_starts, int rows, int row_stride,
                    int max_period, void *d_out, void *stream);
/* Relative period scores.  d_period [R][NVRX_PERIOD_PLANES][K+S]: per rank seven planes {e, peak, rest, strength, period as
 * f32, ago as f32, n as f32} per kernel id and section id (-1.0: none); only plane 0 is read.  Reference per column = the
 * minimum of e over all R ranks, NaN if any rank has none.  Per reported rank [first_rank, first_rank + n_ranks),
 * nvrx_tail_score's arithmetic on e, exactly as nvrx_onset_score:
 *   d_out [n_ranks][1 + S] = {GPU period score, section period score[S]}
 * Scores are in (0, 1]: 1 = "stalls no more than the steadiest rank"; a beat of the whole job (an eval, a checkpoint every
 * rank takes) flags nobody.
 *   d_colmin_scratch  NVRX_ATTR_SCRATCH_FLOATS(K+S) floats of device memory.
 * Argument errors (NVRX_ERR_INVALID / NVRX_ERR_RANGE) are reported before any device is touched. */
#define NVRX_PERIOD_PLANES 7
int nvrx_period_score(const float *d_period, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                      float *d_colmin_scratch, float *d_out, void *stream);

/* Episode of timing rows: whether a row was slow FOR ONE STRETCH of its window and then recovered -- a thermal excursion, a
 * neighbour's checkpoint saturating the host, a link that flapped, an ECC-retry storm.  Extends the statistics of
 * straggler.py:172-197: a stretch of 3 % of a window moves no median and no 0.95-quantile, a pulse is no step and no beat.
 * Per row with n valid samples:
 *   time order  as for nvrx_row_onset: sample i lives in slot (start + i) mod n;
 *   pivoting    d_i = (f64)x_i - (f64)x_0; all sums below are f64 sums of d; T = sum of all d_i, C_t = sum of d_0 .. d_(t-1),
 *               SST = sum of (d_i - T / n)^2;
 *   m           max(8, (min_len_ppm * n + 999999) / 1000000) (64-bit integers), min_len_ppm in [1, 333333];
 *   candidates  every interval [a, b) with a >= m, b <= n - m and b - a >= m: the episode began and ended inside the window,
 *               with at least m samples of "normal" either side (needs n >= 3m; a stretch that runs to the window's end is an
 *               onset);
 *   excess      H_t = n * C_t - t * T, evaluated in this form (two rounded products, one rounded difference);
 *               E_(a,b) = (H_b - H_a) / n: the time the interval spent above the row's mean (the Levin-Kline statistic for an
 *               "epidemic" change);
 *   (a*, b*)    the candidate with the largest E; ties go to the lowest b, then the lowest a; no episode if the largest E <= 0;
 *   at (a*, b*) L = b* - a*; inside = x_0 + (C_b* - C_a*) / L; outside = x_0 + (T - (C_b* - C_a*)) / (n - L);
 *               strength = E^2 * n / (L * (n - L)) / SST, the share of the row's variance that the two-level pulse explains,
 *               in [0, 1]; ago = n - b*, the samples since the episode ended (it began ago + L samples ago).
 * Row record, 16 bytes: {u32 ago | L << 16, f32 inside, f32 outside, f32 strength} (both halves fit 16 bits at
 * NVRX_MAX_RING_CAP).
 *   n == 0 (an absent row)              {0, -1, -1, -1};
 *   T or SST not finite                 {0, NaN, NaN, NaN};
 *   0 < n < 3m, or the largest E <= 0   {0, mean, mean, 0}, mean = x_0 + T / n;
 *   SST == 0 (a constant row)           {0, x_0, x_0, 0}.
 * Effective excess of a record: e = f32 of the f64 quotient inside / outside (the record's f32 values) where L > 0,
 * strength >= min_strength and inside > outside > 0; 1.0 otherwise ("no episode"); -1.0 for an absent row.
 * Rules, not defects: a row that STEPPED UP reads as a strong episode that runs to the last admissible sample (ago == m:
 * "open-ended"; onset scores are the better reading there); a ramp reads as a weaker episode of its upper half (0.71 on a 30 %
 * ramp over 2000 samples; a two-level fit of a ramp explains at most 0.75); a row on a beat reads as none.
 *   d_samples [rows][row_stride], 16-byte aligned, row_stride % 4 == 0, at most NVRX_MAX_RING_CAP; d_counts [rows];
 *   d_starts [rows] or NULL (0 everywhere); d_out [rows] records, 16-byte aligned.  Stateless, like nvrx_row_onset.
 * Argument errors (NVRX_ERR_INVALID / NVRX_ERR_RANGE) are reported before any device is touched. */
int nvrx_row_episode(const float *d_samples, const uint32_t *d_counts, const uint32_t *d_starts, int rows, int row_stride,
                     uint32_t min_len_ppm, void *d_out, void *stream);
/* Relative episode scores (reporting.py:196-253 on the excesses).  d_episode [R][NVRX_EPISODE_PLANES][K+S]: per rank seven
 * planes {e, inside, outside, strength, length as f32, ago as f32, n as f32} per kernel id and section id (-1.0: none); only
 * plane 0 is read.  Reference per column = the minimum of e over all R ranks, NaN if any rank has none.  Per reported rank
 * [first_rank, first_rank + n_ranks), nvrx_tail_score's arithmetic on e, exactly as nvrx_onset_score and nvrx_period_score:
 *   d_out [n_ranks][1 + S] = {GPU episode score, section episode score[S]}
 * Scores are in (0, 1]: 1 = "no stretch slower than the steadiest rank's"; a stretch the whole job shares flags nobody.
 *   d_colmin_scratch  NVRX_ATTR_SCRATCH_FLOATS(K+S) floats of device memory.
 * Argument errors (NVRX_ERR_INVALID / NVRX_ERR_RANGE) are reported before any device is touched. */
#define NVRX_EPISODE_PLANES 7
int nvrx_episode_score(const float *d_episode, const float *d_table, int R, int K, int S, int first_rank, int n_ranks,
                       float *d_colmin_scratch, float *d_out, void *stream);

/* Robust scores: every rank against the job's median and spread. Extends _compute_section_relative_scores /
 * _compute_gpu_perf_score (reporting.py:196-253), whose reference point is the FASTEST rank's median: one anomalously fast
 * rank flags the whole job, the minimum over R ranks drifts with R, and a fixed threshold does not know the job's spread.
 *   d_table [R][L] as for nvrx_score.  Column c in [0, K+S) of its med part: v = table[r][c] is PRESENT iff v >= 0 (the -1
 *   sentinel and NaN are absent).  Per column:
 *      n      present values;
 *      ctr    their LOWER median: the element of rank (n-1) >> 1 sorted by raw bit pattern (-0.0 < +0.0 < ... < +inf),
 *             always an actual value;
 *      mad    the lower median of the n deviations fabsf(v - ctr) (f32; a NaN deviation orders above +inf);
 *      scale  fmaxf(1.4826f * mad, floor_rel * ctr): two f32 products and a maximum;
 *      a column with n < min_ranks has no reference.
 *   Per reported rank r in [first_rank, first_rank + n_ranks), two planes of 1 + S floats:
 *      ratio, section s: f32 of the f64 quotient ctr / v (above 1: faster than the median);
 *      z,     section s: f32 of the f64 (v - ctr) / scale;
 *      NaN where v is absent or the column has no reference;
 *      slot 0 (GPU): f32 of sum_k w_k * x_k / sum_k w_k in f64 over the kernels k < K with v present and a reference, x_k
 *      the f64 ratio / z before rounding, w_k that rank's weights NUM*AVG in the table; NaN when no kernel is eligible.
 *   Zero scales and infinities give IEEE results, never an error.
 *   min_ranks >= 1; floor_rel finite, in [0, 1]: it keeps a column whose ranks agree to the last bit from turning a 0.1 %
 *   difference into z = inf.
 *   d_out  16-byte aligned, NVRX_ROBUST_WORDS(n_ranks, K, S) 32-bit words: K+S column records {f32 ctr, f32 mad, f32 scale,
 *      u32 n} (the floats NaN where there is no reference; n is always written), then [n_ranks][2][1 + S] f32 {ratio, z}.
 * Argument errors (NVRX_ERR_INVALID / NVRX_ERR_RANGE) are reported before any device is touched. */
#define NVRX_ROBUST_MAX_RANKS 65536
#define NVRX_ROBUST_WORDS(n_ranks, K, S) (4 * ((size_t)(K) + (S)) + (size_t)(n_ranks) * 2 * (1 + (size_t)(S)))
int nvrx_robust_score(const float *d_table, int R, int K, int S, int first_rank, int n_ranks, int min_ranks,
                      float floor_rel, void *d_out, void *stream);

/* Peer-group scores: every rank against the fastest rank of ITS OWN group.  The relative scores of reporting.py:196-253 take
 * the fastest rank of the whole job as the reference: a lockstep data-parallel model.  In a job of pipeline stages, expert
 * groups or actor / critic roles, ranks legitimately differ, and the caller says which ranks are peers.
 *   d_table [R][L] as for nvrx_score; R <= NVRX_ROBUST_MAX_RANKS.
 *   d_groups  ONE device array of 2R + G + 1 int32 words, group[R] | members[R] | start[G+1], 1 <= G <= R and G <=
 *      NVRX_PEER_MAX_GROUPS: group[r] is rank r's group id, every rank in exactly one group; members holds the ranks sorted
 *      by (group id, rank); start[g] .. start[g+1] is group g's stretch of members.
 *   Per (group g, column c < K+S of the table's med part), over the members of g: a member is PRESENT iff its value v >= 0
 *   (the -1 sentinel and NaN are absent, as in the robust scores);
 *      floor       the present value whose key (raw bit pattern order: -0.0 < +0.0 < ... < +inf) is smallest;
 *      floor_rank  the lowest rank that holds that key;
 *      the pair is REFERENCED iff present >= min_ranks; one that is not has floor = the canonical NaN 0x7FC00000 and
 *      floor_rank = -1 (present and members are still written; pairs with no present member are written too);
 *      record, 16 bytes: {f32 floor, u32 present, i32 floor_rank, u32 members}, at d_out[g * (K+S) + c] in 16-byte units.
 *   Per reported rank r in [first_rank, first_rank + n_ranks), behind the G * (K+S) records, 1 + S floats:
 *      slot 1 + s: (float)((double)floor / (double)v) of column K + s of r's group; NaN where r is absent or the pair is not
 *      referenced;
 *      slot 0 (GPU): (float)(sum_k w_k * ((double)floor_k / (double)v_k) / sum_k w_k) in f64 over the kernel columns k < K
 *      where r is present and the pair is referenced, w_k = table[r][2(K+S) + k]; NaN when there is no such column (also at
 *      K = 0).  The sum is taken across a wave: its last bits depend on that order.
 *   min_ranks >= 1 and NOT clamped to the group's size: at 2 a rank alone in its group has no peer and is unrated (NaN), not
 *   rated 1.0.  With one group and min_ranks = 1 the section slots are nvrx_score's relative section scores in every section
 *   that every rank has (one that some rank lacks has no job-wide reference, and here rates the ranks that have it).
 *   d_out  16-byte aligned, NVRX_PEER_WORDS(G, n_ranks, K, S) 32-bit words.
 *   The CONTENTS of d_groups are guarded on the device: a group[r] outside [0, G) rates rank r NaN, a members entry outside
 *   [0, R) is skipped, start values are clamped to [0, R] (`members` of a record is the clamped stretch's length); no content
 *   makes a kernel read or write outside the table, the array or d_out.
 * Two launches on `stream` (columns, ranks); no atomics, no scratch.  Argument errors, reported before any device is touched:
 * those of nvrx_robust_score in its order, then NVRX_ERR_INVALID for G < 1, NVRX_ERR_RANGE for G > R or G >
 * NVRX_PEER_MAX_GROUPS, NVRX_ERR_INVALID for a null pointer or a d_out that is not 16-byte aligned. */
#define NVRX_PEER_MAX_GROUPS 4096
#define NVRX_PEER_WORDS(G, n_ranks, K, S) (4 * (size_t)(G) * ((size_t)(K) + (S)) + (size_t)(n_ranks) * (1 + (size_t)(S)))
int nvrx_peer_score(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int first_rank, int n_ranks,
                    int min_ranks, void *d_out, void *stream);

/* Pace scores: the rank that is a LITTLE slower in nearly all of its kernels.  Every score above asks whether some row of a
 * rank is much slower than a reference; a card held a clock step down, a throttling HBM stack or a marginal power rail loses
 * 3-5 % on every kernel, which no threshold on one row and no weighted mean of per-kernel z sees.  Being slower than the job's
 * median in 120 of 120 kernels does not happen by chance: here an order statistic ACROSS a rank's columns says so.
 *   d_table [R][L] as for nvrx_score; R <= NVRX_ROBUST_MAX_RANKS.  A column c < K is a kernel id, K <= c < K+S a section id;
 *   v = table[r][c] is PRESENT iff v >= 0 (the -1 sentinel and NaN are absent, as in the robust scores).
 *   Per column:
 *      n      present values;
 *      ctr    their LOWER median: the element of rank (n-1) >> 1 sorted by raw bit pattern (-0.0 < +0.0 < ... < +inf): exactly
 *             the robust scores' ctr;
 *      the column is REFERENCED iff n >= min_ranks;
 *      above  present values whose key is greater than ctr's, below those whose key is less (both 0 at n = 0);
 *      record, 16 bytes: {f32 ctr (the canonical NaN 0x7FC00000 where not referenced), u32 n, u32 above, u32 below}; the three
 *      counts are always written.
 *   Per reported rank r in [first_rank, first_rank + n_ranks) and part p (0: the kernel columns, 1: the section columns); a
 *   column of the part is ELIGIBLE iff r is present in it and it is referenced:
 *      q_c      (float)((double)ctr_c / (double)v_c): above 1 = faster than the job's median.  The IEEE result is kept: v = 0
 *               gives +inf, or NaN where ctr is 0 too;
 *      columns  eligible columns;
 *      slower   those whose key of v is greater than the key of ctr, faster those where it is less;
 *      pace     the lower median of the q_c that are not NaN: rank (m-1) >> 1 by key over those m values, an actual quotient;
 *               NaN at m = 0;
 *      spread   the lower median of fabsf(q_c - pace) over the same m values (f32; a NaN deviation orders above +inf);
 *      part 0 only, in f64 with w_c = table[r][2(K+S) + c]:
 *      total_us   sum of w_c over the eligible columns;
 *      slower_us  sum of w_c over the slower columns;
 *      excess_us  sum of w_c * (1 - (double)ctr_c / (double)v_c) over the eligible columns with a non-NaN q_c: the
 *                 microseconds this rank spent above the job's median pace in the window (signed);
 *      part 1 writes +0.0 in these three slots;
 *      record, 32 bytes: {f32 pace, f32 spread, u32 columns, u32 slower, u32 faster, f32 total_us, f32 slower_us,
 *      f32 excess_us}.
 *   pace, spread and every count are exact: no sum, and no rounding beyond one f64 quotient and one f32 subtraction.  The three
 *   sums are taken across a workgroup: their last bits depend on that order.
 *   d_out  16-byte aligned, NVRX_PACE_WORDS(n_ranks, K, S) 32-bit words: K+S column records, then [n_ranks][2] rank records.
 * Two launches on `stream` (columns, ranks); no atomics on global memory, no scratch.  Argument errors, reported before any
 * device is touched: those of nvrx_robust_score in its order, without floor_rel. */
#define NVRX_PACE_WORDS(n_ranks, K, S) (4 * ((size_t)(K) + (S)) + 16 * (size_t)(n_ranks))
int nvrx_pace_score(const float *d_table, int R, int K, int S, int first_rank, int n_ranks, int min_ranks, void *d_out,
                    void *stream);

/* Pace scores per peer group: nvrx_pace_score with the lower median of the rank's OWN group as the reference point.  The
 * median of the whole job is the wrong centre in a job of pipeline stages or expert groups: every healthy rank of the slower
 * stage is slower than it in all of its kernels.
 *   d_table [R][L] as for nvrx_score; R <= NVRX_ROBUST_MAX_RANKS.
 *   d_groups  nvrx_peer_score's array, unchanged: group[R] | members[R] | start[G+1], 1 <= G <= R and G <=
 *      NVRX_PEER_MAX_GROUPS.
 *   max_group  in 1..R: the size of the largest group as the host knows it.  It selects the kernel variant (at most 64: one
 *      wave per column; at most 1024: 256 threads per pair; beyond: 1024).
 *   The MEMBERS of group g are members[s .. e), s and e being start[g] and start[g+1] clamped to [0, R], e at least s, and
 *   e - s clamped to max_group; an entry outside [0, R) is skipped.  size_g is that stretch's length (skipped entries count).
 *   Per pair (group g, column c < K+S of the table's med part), over the members of g; a member is PRESENT iff its value
 *   v >= 0:
 *      n      present values;
 *      ctr    their LOWER median: the element of rank (n-1) >> 1 sorted by raw bit pattern, always an actual value;
 *      above  present values whose key is greater than ctr's, below those whose key is less (both 0 at n = 0);
 *      the pair is REFERENCED iff n >= max(min_peers, min(min_ranks, size_g)): min_ranks is clamped to the group's size (the
 *      job-wide rule's caller clamps it to R in the same way) but never goes below min_peers.  At min_peers = 2 a rank alone
 *      in its group has no peer and is unrated, not rated 1.0, and a group of two is rated against its faster member;
 *      record, 16 bytes: {f32 ctr (the canonical NaN 0x7FC00000 where not referenced), u32 n, u32 above, u32 below}, at
 *      d_out[g * (K+S) + c] in 16-byte units; the three counts are always written.
 *   Per reported rank r in [first_rank, first_rank + n_ranks) and part p: exactly nvrx_pace_score's record -- q_c, columns,
 *   slower, faster, pace, spread and for part 0 the three f64 sums -- over the columns where r is present and the pair
 *   (group[r], c) is referenced, ctr being the group's.  A rank whose group[r] is outside [0, G) has no eligible column: NaN,
 *   NaN and zeros.
 *   d_out  16-byte aligned, NVRX_PACE_GROUP_WORDS(G, n_ranks, K, S) 32-bit words: [G][K+S] column records, then [n_ranks][2]
 *   32-byte rank records.
 *   The CONTENTS of d_groups are guarded on the device as stated above; no content makes a kernel read or write outside the
 *   table, the array or d_out.  With one group of all ranks and min_peers = 1 every record is nvrx_pace_score's.
 * Two launches on `stream` (columns, ranks); no atomics on global memory, no scratch.  Argument errors, reported before any
 * device is touched: those of nvrx_pace_score in its order, then nvrx_peer_score's checks of G, then NVRX_ERR_RANGE for a
 * max_group outside 1..R or min_peers < 1, then NVRX_ERR_INVALID for a null pointer or a d_out that is not 16-byte aligned. */
#define NVRX_PACE_GROUP_WORDS(G, n_ranks, K, S) (4 * (size_t)(G) * ((size_t)(K) + (S)) + 16 * (size_t)(n_ranks))
int nvrx_pace_group_score(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int max_group,
                          int first_rank, int n_ranks, int min_ranks, int min_peers, void *d_out, void *stream);

/* Node scores: tell a slow HOST from a slow GPU.  Every score above rates a rank; an operator cordons a node.  A chassis whose
 * fans failed, a capped PSU or a throttling host CPU makes every GPU of one node a few per cent slower in everything: the pace
 * scores name all of its ranks and cannot say that they are one incident.  Here a node votes once per column, with the lower
 * median of its members, and a node's pace is taken against the lower median of the nodes.
 *   d_table [R][L] as for nvrx_score; R <= NVRX_ROBUST_MAX_RANKS.
 *   d_groups  the NODE array, nvrx_peer_score's format unchanged, a node being a group: group[R] | members[R] | start[G+1],
 *      1 <= G <= R and G <= NVRX_PEER_MAX_GROUPS.
 *   max_group  as nvrx_pace_group_score takes it: in 1..R, the size of the largest node as the host knows it.
 *   min_members >= 1: present members a (node, column) pair needs; min_nodes >= 1: referenced nodes a column needs.
 *   Presence (v >= 0), keys (raw bit pattern order), the lower median (rank (n-1) >> 1 by key) and the canonical NaN 0x7FC00000
 *   are the pace scores' own.
 *   Block A, [G][K+S] pair records {f32 med, u32 n, u32 above, u32 below}: exactly nvrx_pace_group_score's column block with
 *      min_ranks = min_members and min_peers = 1 -- med is the lower median of node g's present members, NaN where
 *      n < max(1, min(min_members, size_g)) (the pair is then not REFERENCED); the same guards on the array's contents: start
 *      values clamped to [0, R], a stretch cut to max_group, a member outside [0, R) skipped.
 *   Block B, [K+S] column records {f32 N_c, u32 nodes, u32 above, u32 below} across the nodes: nodes counts the referenced pairs
 *      of the column; N_c is the lower median of their med values -- one node, one vote, whatever the nodes' sizes --, NaN where
 *      nodes < min_nodes (the column is then not referenced); above / below count the referenced nodes whose key of med is
 *      greater / less than the key of that lower median (both 0 at nodes = 0).  The three counts are always written.
 *   Block C, [G][2] node records, 32 bytes each, nvrx_pace_score's rank record with v = the node's med and ctr = N_c; a column
 *      of the part is eligible iff the pair is referenced and the column is referenced: q = (float)((double)N_c / (double)med),
 *      pace, spread, columns, slower, faster as defined there; the three sum slots are +0.0 in both parts.
 *   So every word of A, B and C is exact, ties included.
 *   Block D, [n_ranks][2] rank records: exactly nvrx_pace_score's rank record of each reported rank in [first_rank, first_rank +
 *      n_ranks) with ctr = N_c, a column eligible iff the rank is present and the column is referenced; part 0 keeps the three
 *      f64 sums (taken across a workgroup: their last bits depend on that order).  D says whether a node's members agree with
 *      it, and gives each rank's microseconds above the pace of the job's nodes.
 *   d_out  16-byte aligned, NVRX_NODE_WORDS(G, n_ranks, K, S) 32-bit words: A, B, C, D in this order.
 *   The CONTENTS of d_groups are guarded on the device as stated above; no content makes a kernel read or write outside the
 *   table, the array or d_out.  (group[R] is not read: D's centre is the job's.)
 * R <= 64: three launches on `stream` (A and B in one, C, D); beyond: four (A, B, C, D).  No atomics on global memory, no
 * scratch.  Argument errors, reported before any device is touched: those of nvrx_pace_group_score in its order (without its
 * two thresholds), then NVRX_ERR_RANGE for min_members < 1 or min_nodes < 1, then NVRX_ERR_INVALID for a null pointer or a d_out
 * that is not 16-byte aligned. */
#define NVRX_NODE_WORDS(G, n_ranks, K, S) \
    (4 * (size_t)(G) * ((size_t)(K) + (S)) + 4 * ((size_t)(K) + (S)) + 16 * (size_t)(G) + 16 * (size_t)(n_ranks))
int nvrx_node_score(const float *d_table, int R, int K, int S, const int32_t *d_groups, int G, int max_group, int min_members,
                    int min_nodes, int first_rank, int n_ranks, void *d_out, void *stream);

/* Score history: how each score behaved over the last H reports.  Every score above looks inside one report window; the one
 * thing a report carries over from its predecessors is the running minimum of MED.  Here a device ring keeps the last H
 * reports' scores per reported rank, family f (0 individual, 1 relative: the parity of the score row's first two columns)
 * and slot j (0 = the GPU score, 1 + s = section id s), and one step per report appends the report's scores and says, per
 * (rank, f, j), how long the score has been below its threshold.  Nothing is exchanged: the step reads what nvrx_score wrote.
 *   H       depth, in [2, NVRX_HISTORY_MAX_DEPTH]; Hs = NVRX_HISTORY_STRIDE(H): 16, 32 or 64, the smallest that is >= H;
 *   d_hist  f32 [n_ranks][2][1 + S_cap][Hs], 16-byte aligned (NVRX_HISTORY_FLOATS).  Physical position i < H of a cell holds
 *           the report with (number of that report) % H == i; positions [H, Hs) are never touched.  An ABSENT entry is a NaN:
 *           the caller fills a fresh buffer with bytes 0xFF (a NaN in every word);
 *   d_scores [R][NVRX_SCORE_LEN(S)] as nvrx_score wrote it (it may be the pinned, device-mapped result block); S <= S_cap;
 *   ranks   [first_rank, first_rank + n_ranks) of the R score rows: row r of d_hist / d_out is rank first_rank + r;
 *   n_before  reports appended so far; thresholds[4] in nvrx_score's order, NULL => 0.75 each (finite).
 * The step, per (r, f, j) with j <= S (slots j > S are left alone):
 *   x      = d_scores[first_rank + r][col], col = f for j == 0, else 2 + (j - 1) for f == 0 and 2 + S + (j - 1) for f == 1;
 *   x is stored at position n_before % H; depth = min(n_before + 1, H); x_a, a in [0, depth), is the entry of AGE a -- the one
 *   at position (n_before - a) mod H -- so x_0 = x;
 *   thr    = thresholds[0] for (f, j) = (1, 0), [1] for (1, j > 0), [2] for (0, 0), [3] for (0, j > 0);
 *   x_a is PRESENT iff it is no NaN and BELOW iff (double)x_a < thr -- the comparison behind nvrx_score's d_flags (strict; NaN
 *   is never below; +inf and 0.0 are values);
 *   record, 32 bytes: {f32 latest = x_0, f32 median, f32 worst, f32 best, u32 streak, u32 below, u32 present, u32 depth}
 *      present  number of present entries, below  number of entries below;
 *      streak   number of newest entries x_0, x_1, ... that are all below: 0 if x_0 is not; a NaN ends it, and so does depth;
 *      median, worst, best  the elements of rank (present - 1) >> 1, 0 and present - 1 of the present entries sorted by raw
 *               bit pattern (-0.0 < +0.0 < ... < +inf): the LOWER median, always actual scores; NaN when present == 0.
 *   Every word is exact: no sum, no rounding.
 *   d_out  16-byte aligned, NVRX_HISTORY_WORDS(n_ranks, S) 32-bit words: [n_ranks][2][1 + S][8].
 * A rank is PERSISTENTLY slow on a column when streak >= min_reports; below / present serve "k of the last H".
 * One launch; every (r, f, j) appends its own entry, so steps must only be ordered against each other (one stream).
 * NVRX_ERR_RANGE for H outside [2, 64], S_cap above NVRX_MAX_ROWS, or more cells than one launch covers (n_ranks * 2 *
 * ceil((1 + S) / (64 / Hs)) waves above 2^31 - 1); NVRX_ERR_INVALID for null or misaligned pointers, S > S_cap, a bad rank
 * range or non-finite thresholds -- reported before any device is touched. */
#define NVRX_HISTORY_MAX_DEPTH 64
#define NVRX_HISTORY_STRIDE(H) ((H) <= 16 ? 16 : (H) <= 32 ? 32 : 64)
#define NVRX_HISTORY_FLOATS(n_ranks, S_cap, H) ((size_t)(n_ranks) * 2 * (1 + (size_t)(S_cap)) * NVRX_HISTORY_STRIDE(H))
#define NVRX_HISTORY_WORDS(n_ranks, S) ((size_t)(n_ranks) * 2 * (1 + (size_t)(S)) * 8)
int nvrx_score_history(const float *d_scores, int R, int S, int first_rank, int n_ranks, float *d_hist, int S_cap, int H,
                       uint64_t n_before, const double *thresholds, void *d_out, void *stream);

/* Score trends: whether each score of the history ring is FALLING from report to report.  The history above says for how many
 * reports a score has been below its threshold; a rank that loses a percent per report is invisible to it until it has
 * crossed.  One step per report reads the ring nvrx_score_history keeps -- it writes nothing to it and needs no score rows --
 * and leaves a robust, exact trend estimate per (rank r, family f, slot j) with j <= S (slots j > S are left alone).
 *   d_hist, n_ranks, S, S_cap, H  the ring as nvrx_score_history left it (Hs = NVRX_HISTORY_STRIDE(H));
 *   n_reports  reports appended so far, the latest included (the step's n_before + 1); at least 1.
 * Per cell:
 *   entries  depth = min(n_reports, H); x_a, a in [0, depth), is the entry of AGE a, at position (n_reports - 1 - a) mod H.
 *            An entry is USABLE iff it is finite: NaN (absent) and +-inf are not.  p = number of usable entries;
 *   pair slopes  for every pair of usable ages a < b (a the newer entry)
 *            s_ab = (float)(((double)x_a - (double)x_b) / (double)(b - a)): the change per report, negative when the score
 *            falls; N = p (p - 1) / 2 of them;
 *   slope    the pair slope of rank (N - 1) >> 1 of the N pair slopes sorted by raw bit pattern (-inf < ... < -0.0 < +0.0 < ...
 *            < +inf): the LOWER median of the Theil-Sen estimator, always an actual pair slope; NaN (0x7FC00000) when p < 2;
 *   S        (i32) pairs with x_a > x_b minus pairs with x_a < x_b, as floats compare (-0.0 == +0.0): the Mann-Kendall
 *            statistic, negative when the score falls; tau = S / N is the host's to derive;
 *   level    the trend line's value at the newest report: the lower median, in the same order, of
 *            v_a = (float)((double)x_a + (double)slope * (double)a) over the usable ages (the product is exact in f64, so a
 *            fused multiply-add gives the same bits); the one usable entry when p == 1; NaN (0x7FC00000) when p == 0.  A v_a
 *            that is a NaN -- possible only where the slope is infinite, entries more than FLT_MAX apart -- counts as
 *            0x7FC00000 and orders behind +inf;
 *   record, 16 bytes: {f32 slope, f32 level, i32 S, u32 usable = p}.  Every word is exact: one correctly rounded f64
 *            operation and one conversion per value, no sum.
 *   d_out  16-byte aligned, NVRX_TREND_WORDS(n_ranks, S) 32-bit words: [n_ranks][2][1 + S][4].
 * One launch, behind the history step on its stream; it only reads the ring.  Errors as nvrx_score_history's (H, S_cap, the
 * launch's size: NVRX_ERR_RANGE; pointers, S > S_cap, n_ranks < 1: NVRX_ERR_INVALID), and NVRX_ERR_INVALID for n_reports == 0
 * -- reported before any device is touched. */
#define NVRX_TREND_WORDS(n_ranks, S) ((size_t)(n_ranks) * 2 * (1 + (size_t)(S)) * 4)
int nvrx_score_trend(const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports, void *d_out, void *stream);

/* Peer-score history and trends: the two steps above on the PEER-GROUP scores.  Where ranks legitimately differ (pipeline
 * stages, expert groups) the job-wide relative scores rate a whole stage low in every report; the scores that mean something
 * are nvrx_peer_score's, and these entries keep a ring of THEM.  One family, not two; the NaN of an unrated rank is an absent
 * entry (it ends a streak).  There is one definition of every record -- the two contracts above:
 *   d_peer  the rank part nvrx_peer_score / nvrx_report_peer left: f32 [n_ranks][1 + S] {GPU peer score, section peer
 *           score[S]}, behind the G (K+S) column records of its block (d_out + 16 G (K+S) bytes there); 4-byte aligned;
 *   d_hist  f32 [n_ranks][1 + S_cap][Hs], Hs = NVRX_HISTORY_STRIDE(H), 16-byte aligned (NVRX_PEER_HISTORY_FLOATS); a fresh
 *           ring is bytes 0xFF.  Slot 0 is the GPU peer score, slot 1 + s section id s;
 *   rows    row r of d_peer, d_hist and d_out is the r-th REPORTED rank: the peer block is already cut to the reported ranks,
 *           so there is no first_rank;
 *   thresholds[2]  {gpu, section}, NULL => 0.75 each (finite).
 * nvrx_peer_history: the record of cell (r, j) is word for word the record nvrx_score_history writes for (r, f = 1, j) on
 * score rows whose relative columns hold the peer values (column 1 = d_peer[r][0], column 2 + S + s = d_peer[r][1 + s]), with
 * thresholds[0] and thresholds[1]; the ring cell (r, j) is byte for byte that call's ring cell (r, 1, j).
 *   d_out  16-byte aligned, NVRX_PEER_HISTORY_WORDS(n_ranks, S) 32-bit words: [n_ranks][1 + S][8].
 * nvrx_peer_trend: the record of cell (r, j) is the record nvrx_score_trend writes for that ring cell; the ring is only read.
 *   d_out  16-byte aligned, NVRX_PEER_TREND_WORDS(n_ranks, S) 32-bit words: [n_ranks][1 + S][4].
 * One launch each; steps on one ring must be ordered against each other and behind the peer step they read (one stream).
 * Errors as nvrx_score_history's and nvrx_score_trend's, in their order, with R = n_ranks and one family: NVRX_ERR_RANGE for H
 * outside [2, 64], S_cap above NVRX_MAX_ROWS or more cells than one launch covers (n_ranks * ceil((1 + S) / (64 / Hs)) waves
 * above 2^31 - 1); NVRX_ERR_INVALID for n_ranks < 1, S < 0, S > S_cap, null or misaligned pointers, non-finite thresholds and
 * -- the trend -- n_reports == 0; reported before any device is touched. */
#define NVRX_PEER_HISTORY_FLOATS(n_ranks, S_cap, H) ((size_t)(n_ranks) * (1 + (size_t)(S_cap)) * NVRX_HISTORY_STRIDE(H))
#define NVRX_PEER_HISTORY_WORDS(n_ranks, S) ((size_t)(n_ranks) * (1 + (size_t)(S)) * 8)
#define NVRX_PEER_TREND_WORDS(n_ranks, S) ((size_t)(n_ranks) * (1 + (size_t)(S)) * 4)
int nvrx_peer_history(const float *d_peer, int n_ranks, int S, float *d_hist, int S_cap, int H, uint64_t n_before,
                      const double *thresholds, void *d_out, void *stream);
int nvrx_peer_trend(const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports, void *d_out, void *stream);

/* Slack scores: the rank the others WAIT FOR in collectives.  Every score above compares how long a rank's own work takes; a
 * rank whose host is slow (a busy CPU, a data loader, a GC pause) launches late, computes at the usual speed and ends its
 * sections in a collective like everybody else, so all of them read 1.  The time the ranks spend inside collective kernels
 * shows it: the rank that arrives last spends only the transfer time there, every other rank that plus the wait for it.  The
 * rank with the LEAST time in collectives is the one the job waits for, and what the others spend above that floor is what it
 * costs.  A lockstep job (data parallel, FSDP) is the model.
 *   columns  NVRX_SLACK_COLS = 64.  A collective key (a kernel row whose name is a collective kernel's) has the column
 *            digest(key) % 64, the digest being the name mapper's (64-bit BLAKE2b, little-endian): every rank computes the same column from
 *            the same key, nothing is agreed or exchanged; keys that collide share a column and their times add on every rank
 *            alike.
 * Local step (nvrx_slack_local, below), per logical rank q and column c over the (row, column) list in its order, which is
 * ascending in the row, rows r >= rows_active left out:
 *   a row counts iff NUM >= 1 in its statistics row (the statistics kernel writes NUM = 0 for an empty row);
 *   t = sum of (double)WEIGHT_r (WEIGHT = NUM * AVG, NVRX_STAT_WEIGHT), n = sum of (double)NUM_r: one sequence of f64 additions;
 *   send rows [local_ranks][2][64] f32: plane 0 (float)t, plane 1 (float)n; {-1, 0} for a column without a counting row.
 * Score step (nvrx_slack_score) on the gathered d_slack [R][2][64] and the report's exchanged d_table [R][L] (nvrx_score):
 *   present  rank r in column c iff n > 0 and t >= 0 (a NaN is absent); avg = (float)((double)t / (double)n), the mean per
 *            call -- windows that differ by a call between ranks do not read as slack;
 *   column   referenced iff at least min(min_ranks, R) ranks are present; floor = the minimum of avg over the present ranks;
 *            record, 16 bytes: {f32 floor (NaN 0x7FC00000 where not referenced), u32 present, 0, 0}.  Exact;
 *   rank     over the referenced columns it is present in, sums in f64: collective_us = sum t, waited_us = sum (double)n *
 *            ((double)avg - (double)floor), calls = sum n, columns = their number; compute_us = the sum of the weights
 *            w[r][k] of the kernel ids whose med entry is >= 0 (0 at K = 0; d_table may then be NULL); share = (float)(waited /
 *            (collective + compute)) on the f64 sums: the share of this rank's traced GPU time spent waiting;
 *            record, 32 bytes: {f32 collective_us, f32 waited_us, f32 compute_us, f32 share, u32 calls, u32 columns, 0, 0};
 *            NaN in the four floats and 0 in the counts for a rank without a referenced column.  The sums are taken across a
 *            wave: their last bits depend on that order;
 *   job      record, 32 bytes: {f32 typical_waited, f32 typical_share, u32 ranks_with_data, u32 columns_referenced, 0, 0, 0,
 *            0}: the LOWER medians (rank (m - 1) >> 1 in value order, always an actual value) of waited_us and of share over
 *            the ranks with data (columns > 0) -- a value that is a NaN (inf - inf, 0 / 0) does not enter its median, m
 *            counting the values that do --, NaN 0x7FC00000 when none enters.
 *   d_out    16-byte aligned, NVRX_SLACK_WORDS(R) 32-bit words: job record | 64 column records | R rank records.  All R ranks
 *            are always computed: the medians need them.
 * Three small launches on `stream` (columns, ranks, job); no atomics, no scratch.  NVRX_ERR_INVALID: R <= 0, K or S negative,
 * a null pointer, d_slack or d_out not 16-byte aligned; NVRX_ERR_RANGE: R above NVRX_ROBUST_MAX_RANKS, K or S above
 * NVRX_MAX_ROWS, min_ranks < 1 -- reported before any device is touched.  4 ranks, and the 0.05 / 0.25 of the Python rule
 * built on these records, are defaults, not measurements. */
#define NVRX_SLACK_COLS 64
#define NVRX_SLACK_WORDS(R) (8 + 4 * (size_t)NVRX_SLACK_COLS + 8 * (size_t)(R))
int nvrx_slack_score(const float *d_slack, const float *d_table, int R, int K, int S, int min_ranks, void *d_out, void *stream);

/* Slack scores per peer group: the rank that the ranks doing the SAME work wait for.  nvrx_slack_score's floor of a column is
 * taken over all ranks and its typical wait over the whole job: a lockstep model.  In a job of pipeline stages, tensor-parallel
 * or expert groups the time inside collective kernels is dominated by waits that legitimately differ per stage; the stage
 * that waits least sets a floor no other stage can reach, and a rank whose host is slow is missed or healthy ranks are named.
 * Here the score step runs per peer group; the local step, the send rows and the gathered d_slack are nvrx_slack_score's.
 *   d_groups  nvrx_peer_score's array, unchanged: group[R] | members[R] | start[G+1], 1 <= G <= R and G <=
 *      NVRX_PEER_MAX_GROUPS.
 *   max_group  in 1..R: the size of the largest group as the host knows it.  It selects the variant of the group kernel (at
 *      most 64: one wave, a member per lane; at most 1024: 256 threads; beyond: 1024); a larger value than needed is legal.
 *   The MEMBERS of group g are members[s .. e), s and e being start[g] and start[g+1] clamped to [0, R], e at least s, and
 *   e - s clamped to max_group; an entry outside [0, R) is skipped.  size_g is that stretch's length (skipped entries count).
 *   present, t, n and avg per (rank, column) are nvrx_slack_score's.
 *   Per pair (group g, column c < 64), over the members of g:
 *      present_gc  members present in c;
 *      the pair is REFERENCED iff present_gc >= max(min_peers, min(min_ranks, size_g)) (nvrx_pace_group_score's rule: at
 *      min_peers = 2 a rank alone in its group has no peer and is unrated);
 *      floor       the minimum of avg over the present members by raw bit pattern, floor_rank the member that holds it, the
 *      lower rank on a tie;
 *      record, 16 bytes: {f32 floor, u32 present_gc, i32 floor_rank, u32 size_g}; floor is the NaN 0x7FC00000 and floor_rank
 *      -1 where the pair is not referenced.  Exact.
 *   Per rank r of group g = group[r], over the columns it is present in whose pair (g, c) is referenced: collective_us,
 *      waited_us = sum (double)n * ((double)avg - (double)floor_gc), calls, columns, compute_us and share exactly as
 *      nvrx_slack_score spells them (the same f64 sequences);
 *      record, 32 bytes: {f32 collective_us, f32 waited_us, f32 compute_us, f32 share, u32 calls, u32 columns, u32
 *      present_columns, i32 group}: present_columns counts the columns the rank is present in at all (what tells "no collective
 *      rows" from "rows but no peers"), group is g, -1 where group[r] is outside [0, G) -- such a rank has no column.  NaN
 *      in the four floats and 0 in calls and columns where columns == 0.
 *   Per group g: record, 32 bytes: {f32 typical_waited, f32 typical_share, u32 ranks_with_data, u32 pairs_referenced, u32
 *      size_g, 0, 0, 0}: the LOWER medians (rank (m - 1) >> 1 in value order) of waited_us and of share over the records of the
 *      group's members with data (columns > 0), a NaN not entering, as in nvrx_slack_score's job record; NaN 0x7FC00000 when
 *      none enters.
 *   d_out  16-byte aligned, NVRX_SLACK_GROUP_WORDS(G, R) 32-bit words: G group records | G x 64 pair records | R rank records.
 *      All R ranks are always computed.
 *   The CONTENTS of d_groups are guarded on the device as stated above; no content makes a kernel read or write outside
 *   d_slack, d_table, the array or d_out.  With one group of all ranks and min_peers = 1 the pair records' {floor, present},
 *   words 0-5 of every rank record and the first four words of the group record are nvrx_slack_score's.
 * Three small launches on `stream` (pairs, ranks, groups); no atomics, no scratch.  Argument errors, reported before any
 * device is touched: those of nvrx_slack_score in its order, then nvrx_peer_score's checks of G, then NVRX_ERR_RANGE for a
 * max_group outside 1..R or min_peers < 1, then NVRX_ERR_INVALID for a null d_groups. */
#define NVRX_SLACK_GROUP_WORDS(G, R) ((8 + 4 * (size_t)NVRX_SLACK_COLS) * (size_t)(G) + 8 * (size_t)(R))
int nvrx_slack_group_score(const float *d_slack, const float *d_table, int R, int K, int S, const int32_t *d_groups, int G,
                           int max_group, int min_ranks, int min_peers, void *d_out, void *stream);

/* Row-family scores per peer group: nvrx_{tail,onset,period,episode}_score with a column's reference taken inside each rank's
 * OWN group.  The job-wide step takes one reference per column over all R ranks: in a job of pipeline stages the healthy ranks
 * of the slower stage read as tail stragglers (tails are absolute times), and a step, a beat or a stretch that one whole STAGE
 * shares flags that stage.  One entry serves all four families: they differ in what plane 0 holds, not in how it is scored.
 *   d_planes  [R][planes][K+S], a family's gathered table (-1.0: none); only plane 0 is read, at a pitch of planes * (K+S).
 *      planes in 1..7 (the largest *_PLANES above).
 *   d_table  [R][L] as for nvrx_score: only the weights w[r][k] = table[r][2(K+S) + k], k < K, are read; it may be NULL only
 *      at K = 0.  R <= NVRX_ROBUST_MAX_RANKS.
 *   d_groups  nvrx_peer_score's array, unchanged: group[R] | members[R] | start[G+1], 1 <= G <= R and G <=
 *      NVRX_PEER_MAX_GROUPS, with that entry's guards: a group[r] outside [0, G) rates rank r NaN, a members entry outside
 *      [0, R) is skipped, start values are clamped to [0, R]; no content makes a kernel read or write outside the inputs or
 *      d_out.
 *   d_out  16-byte aligned, NVRX_ROWFAM_GROUP_WORDS(G, K, S, n_ranks) 32-bit words (nvrx_rowfam_group_words returns the same;
 *      0 for a negative argument), two blocks:
 *      A  [G][K+S] records of 16 bytes {f32 floor, u32 present, i32 floor_rank, u32 members}: exactly nvrx_peer_score's column
 *         record taken over plane 0.  A member is PRESENT iff its value v >= 0 (the -1 sentinel and NaN are absent); floor is
 *         the present value with the smallest key (raw bit pattern order), floor_rank the lowest rank that holds it; the pair
 *         is REFERENCED iff present >= min_ranks, else floor is the NaN 0x7FC00000 and floor_rank -1.  min_ranks >= 1 and NOT
 *         clamped to the group's size: at 2 a rank alone in its group is unrated, not rated 1.0.
 *      B  [n_ranks][1 + S] f32 per reported rank r in [first_rank, first_rank + n_ranks), g = group[r]:
 *         slot 1 + s: (float)((double)floor / (double)v) of column K + s of g;
 *         slot 0: (float)(sum_k w_k * ((double)floor_k / (double)v_k) / sum_k w_k) in f64 over the kernel columns k < K that are
 *         eligible in the same way; NaN when none is (also at K = 0).  The sum is taken across a wave: its last bits depend on
 *         that order;
 *         a slot is NaN where g is outside [0, G), r's value is absent or the pair is not referenced.  Zero and +inf values
 *         give the IEEE results, as in nvrx_peer_score.
 *   This rule DIFFERS from the job-wide entries' "NaN if any rank has none": a group's floor is taken over its PRESENT members,
 *   and min_ranks says how many of them a reference needs.  With one group of all ranks, min_ranks = 1 and every rank holding
 *   every column, the section slots are nvrx_tail_score's bit for bit.
 * Two launches on `stream` for every R (k_peer_cols on the planes, k_rowfam_group_rank); no atomics, no scratch.  Argument
 * errors, reported before any device is touched: NVRX_ERR_INVALID for a bad shape, NVRX_ERR_RANGE for R, K or S beyond their
 * limits, for a rank range outside the table, for planes outside 1..7 and for min_ranks < 1, then nvrx_peer_score's checks of
 * G, then NVRX_ERR_INVALID for a null pointer or a d_out that is not 16-byte aligned. */
#define NVRX_ROWFAM_GROUP_WORDS(G, K, S, n_ranks) \
    (4 * (size_t)(G) * ((size_t)(K) + (S)) + (size_t)(n_ranks) * (1 + (size_t)(S)))
int nvrx_rowfam_group_score(const float *d_planes, int planes, const float *d_table, int R, int K, int S,
                            const int32_t *d_groups, int G, int first_rank, int n_ranks, int min_ranks, void *d_out,
                            void *stream);
size_t nvrx_rowfam_group_words(int G, int K, int S, int n_ranks);

/* Work groups: WHICH RANKS DO THE SAME WORK, inferred from the table.  Peer-group scores, pace scores per peer group and node
 * scores take that from the caller (d_groups); the table a report gathers holds a signature of each rank's work that does not
 * depend on how fast the rank runs: which kernel ids and section ids it has at all, and -- the exchanged weight being NUM * AVG
 * -- how OFTEN each kernel ran in the window, w / med.  A slow GPU changes durations, neither the set of kernels nor their call
 * counts, so a rank 1.4 x slower than its peers has exactly its peers' signature.  Every word of the result is an integer, or
 * one correctly rounded f64 division converted to f32: exact.
 *   d_table [R][L] as for nvrx_score; R <= NVRX_WORK_MAX_RANKS; T = ceil(R / 64).
 *   Signature sig[r][c], f32, c < K+S, from med = table[r][c] and, for a kernel id, w = table[r][2(K+S) + c]:
 *      -1.0   absent: unless med >= 0 (the -1 sentinel and NaN are absent, as in the robust scores);
 *      +0.0   present with an unknown count: every present section id (c >= K), and a present kernel id unless
 *      q      = (float)((double)w / (double)med), where med > 0, w is finite and > 0 and q is finite and > 0.
 *   Pair (a, b), a != b, over all K+S columns:
 *      either  columns present on at least one of the two ranks;
 *      unlike  columns present on exactly one of them, plus the columns present on both with both counts > 0 where
 *              (double)hi > (1.0 + (double)count_tol) * (double)lo, hi and lo the larger and the smaller of the two counts;
 *      the two ranks are ALIKE iff either >= 1 and (uint64)unlike * 1000000 <= (uint64)max_unlike_ppm * either.  Symmetric.
 *   count_tol f32 in [0, 16], max_unlike_ppm in [0, 1000000].  The Python package's 0.25 and 100000 are defaults, not
 *   measurements.  NUM is the number of samples a ring row holds: a kernel called more often in a window than its ring has
 *   slots reads ring_cap on every rank alike, and call counts beyond that do not tell ranks apart (presence still does).
 *   Groups are the connected components of the alike relation; root[r] is the lowest rank of r's component.  A rank with
 *   nothing present is alike to nobody and alone.  Single linkage can chain: a component need not be a clique (degree + 1 < size
 *   says so).
 *   Nearest of rank a: the other rank b with either >= 1 whose share unlike / either is smallest, shares compared by 64-bit
 *   cross-multiplication, the lower b on a tie; -1 where there is none.
 *   d_out  16-byte aligned, nvrx_work_words(R, K, S) 32-bit words; five parts, each starting on a 16-byte boundary (the words
 *   that pad a part are written as 0):
 *      A  sig [R][K+S] f32;
 *      B  adjacency [R][T] u64: bit b of word j of row a stands for rank 64 j + b and is set iff the two are alike; the
 *         diagonal is set; bits at or beyond R are clear;
 *      C  partial nearest [R][T], 16 bytes: {u32 unlike, u32 either, i32 rank, 0}, the nearest of rank a among ranks [64 j,
 *         64 j + 64); {0, 0, -1, 0} where that tile has none;
 *      D  rank records [R], 32 bytes: {i32 root, u32 size of the component, u32 degree = alike ranks without the rank itself,
 *         i32 nearest, u32 nearest_unlike, u32 nearest_either, u32 kernels_present, u32 sections_present};
 *      E  job record, 16 bytes: {u32 groups, u32 singletons (groups of one rank), u32 largest, u32 ranks_with_data (ranks
 *         with a present column)}.
 *   All R ranks are always computed.  A, B and C are the hand-over between the kernels and part of the result.
 * Four launches on `stream` (signatures, pairs -- one workgroup per 64 x 64 tile of rank pairs --, components, ranks); no float
 * atomics, no atomics on global memory, no scratch.  Argument errors, reported before any device is touched: the table's shape
 * as for nvrx_robust_score, then NVRX_ERR_RANGE for R > NVRX_WORK_MAX_RANKS, for a count_tol outside [0, 16] (a NaN included)
 * and for a max_unlike_ppm outside [0, 1000000], then NVRX_ERR_INVALID for a null pointer or a d_out that is not 16-byte
 * aligned.  nvrx_work_words returns the block's size (it fits an int: below 2^30 words at the largest shape), or the error
 * nvrx_work_groups reports for that shape (NVRX_ERR_INVALID, NVRX_ERR_RANGE). */
#define NVRX_WORK_MAX_RANKS 4096
int nvrx_work_words(int R, int K, int S);
int nvrx_work_groups(const float *d_table, int R, int K, int S, float count_tol, int max_unlike_ppm, void *d_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Context: device ring buffers + pinned staging + hipEvent timing for `local_ranks` logical ranks
 * of `rows_per_rank` rows each (one logical rank per GPU in production; several per GPU only when a
 * whole job is folded onto fewer GPUs for benchmarking).
 * Replaces CustomSection.cpu_elapsed_times deques (straggler.py:66-83), the native
 * unordered_map<string, CircularBuffer<float>> (CuptiProfiler.h:66, CircularBuffer.h:22-70) and the
 * CUPTI activity machinery (CuptiProfiler.cpp:96-207, BufferPool.cpp).
 * ---------------------------------------------------------------------------------------------- */
int nvrx_ctx_create(int device, int local_ranks, int rows_per_rank, int ring_cap, nvrx_ctx **out);
int nvrx_ctx_destroy(nvrx_ctx *ctx);
/* Stream used for flushes triggered implicitly by a full staging buffer (default: null stream). */
int nvrx_ctx_set_stream(nvrx_ctx *ctx, void *stream);
/* Geometry queries: 0 local_ranks, 1 rows_per_rank, 2 ring_cap, 3 row_stride, 4 device; diagnostics: 5 reports re-homed,
 * 6 verdict of the last re-homing decision, 7 GPU-timed regions skipped because their stream was being captured; 8 rows
 * of a logical rank handed out by nvrx_row_alloc so far. */
int nvrx_ctx_info(const nvrx_ctx *ctx, int what);

/* Hand out the next unused row of a logical rank (the same index in every logical rank of the context), configured as
 * `kind`, not exchanged: the entry of a section name / kernel key seen for the first time -- unordered_map::emplace of
 * CuptiProfiler.cpp:199-203, CustomSection creation of straggler.py:301-305.  Returns the row (>= 0) or NVRX_ERR_RANGE
 * when all rows_per_rank rows are taken.  Thread-safe: the per-kernel tracer calls it on its own thread. */
int nvrx_row_alloc(nvrx_ctx *ctx, int kind);
/* Row metadata: kind (NVRX_KIND_*) and position `gid` in the exchange table (-1 = not exchanged).
 * `row` indexes [0, local_ranks*rows_per_rank). Takes effect at the next flush. */
int nvrx_row_configure(nvrx_ctx *ctx, int row, int kind, int gid);

/* Append one sample (overwrite-oldest beyond ring_cap): deque.append (straggler.py:343) /
 * CircularBuffer::push_back (CircularBuffer.h:53-61).  Staged in pinned host memory; reaches the
 * device ring at the next flush.  O(1), no HIP call unless the staging buffer is full. */
int nvrx_ring_push(nvrx_ctx *ctx, int row, float value);
int nvrx_ring_push_many(nvrx_ctx *ctx, int row, const float *values, int n);
/* Append n (row, value) pairs in arrival order with ONE scatter launch on the context's stream, whatever the number of
 * rows they touch (rows[i] < 0 skips pair i).  Same ring semantics as n calls of nvrx_ring_push.  This is how the
 * per-kernel tracer's drained records reach the rings: the reference appends every CUPTI record to its key's
 * CircularBuffer on the host (CuptiProfiler.cpp:186-207, CircularBuffer.h:53-61). */
int nvrx_ring_push_pairs(nvrx_ctx *ctx, const int32_t *rows, const float *values, int n);
/* The same n pairs appended one by one and STAGED like nvrx_ring_push: nothing is launched unless a staging buffer fills
 * up; thread-safe.  This is the `push` of the per-kernel tracer's sink (include/nvrx_ktrace.h): the tracer's thread
 * appends every kernel record to its key's ring as the records arrive, the way the reference does on CUPTI's thread
 * (CuptiProfiler.cpp:168-207) -- the newest ring_cap durations per key survive (CircularBuffer.h:53-61). */
int nvrx_ring_push_staged(nvrx_ctx *ctx, const int32_t *rows, const float *values, int n);
/* nvrx_ring_push_staged / nvrx_row_alloc with the exact C types of nvrx_ktrace_sink's two function pointers (`void *ctx`):
 * these are the addresses to put into a sink. */
int nvrx_sink_push(void *ctx, const int32_t *rows, const float *values, int n);
int nvrx_sink_row_alloc(void *ctx, int kind);
/* Append n samples that already live in device memory (device-to-device, wraps as needed). */
int nvrx_ring_push_device(nvrx_ctx *ctx, int row, const float *d_values, int n, void *stream);
/* The same for n_rows consecutive rows at once: row first_row + r gets the n samples at d_values + r * ld (ld >= n).  Rows
 * that stand at the same ring position are written with one strided device copy per ring segment.  This is how a whole
 * [sections][samples] matrix (the reference's per-section deques, straggler.py:80-83) is handed over in one call. */
int nvrx_ring_push_device_rows(nvrx_ctx *ctx, int first_row, int n_rows, const float *d_values, int n, int ld, void *stream);
/* Declare that `row` currently holds n valid samples in its device ring (no data movement). */
int nvrx_ring_set_count(nvrx_ctx *ctx, int row, int n);
/* Same for every row of the context at once (benchmark re-arm of resident data). */
int nvrx_ring_set_count_all(nvrx_ctx *ctx, int n);
/* Valid samples in `row` (including staged ones), min(total pushed, ring_cap). */
int nvrx_ring_count(const nvrx_ctx *ctx, int row);
/* Valid-sample counts of rows [0, n) in one call. */
int nvrx_ring_counts(const nvrx_ctx *ctx, int32_t *out, int n);
/* 1 if the SET of rows among [0, n) that hold samples differs from what the previous call saw (or n does, or this is the
 * first call), else 0: a report's name tables -- which sections / kernels have a summary this window, straggler.py:185-195
 * leaves out what holds no samples -- only need rebuilding when this says so.  One call, nothing copied. */
int nvrx_ring_occupancy_changed(nvrx_ctx *ctx, int n);
/* Drop all samples of every row: deque.clear (straggler.py:223-225) / reset (CuptiProfiler.cpp:148-152).
 * History minima and row configuration are kept, as in the reference (reporting.py:186-191).
 * Host state only: nothing is launched and no staging buffer is waited for.  That makes it the ONE ring call allowed while a
 * report is pending between nvrx_report_issue and nvrx_report_wait: the statistics kernel has its counts already -- as the
 * uniform-count argument of its launch, or in the device's count table behind the scatter that was enqueued in front of it
 * on the same stream from a staging buffer this call does not touch. */
int nvrx_ring_reset(nvrx_ctx *ctx);
/* Forget the history minima too (new Detector.initialize). */
int nvrx_history_reset(nvrx_ctx *ctx, void *stream);
/* Push staged samples + row metadata to the device (one kernel reading pinned memory). */
int nvrx_ring_flush(nvrx_ctx *ctx, void *stream);
/* Debug/test: copy a row's ring storage (row_stride floats) to host after a flush. */
int nvrx_ring_read(nvrx_ctx *ctx, int row, float *out, int n, void *stream);

/* GPU timing of a code region with a hipEvent pair on `stream`: the MI355X replacement for the
 * CUPTI activity records (CuptiProfiler.cpp:116-133,168-207).  Elapsed time is appended to `row`
 * in MICROSECONDS f32 (CuptiProfiler.cpp:191) when harvested.  begin/end may nest. */
int nvrx_event_begin(nvrx_ctx *ctx, int row, void *stream);
int nvrx_event_end(nvrx_ctx *ctx, int row, void *stream);
/* Move completed event pairs into their rows.  wait!=0 blocks until every ended pair completes
 * (the role of torch.cuda.synchronize() in straggler.py:234, without a device-wide sync).
 * Returns the number of pairs still pending (>=0) or a negative error. */
int nvrx_event_harvest(nvrx_ctx *ctx, int wait);

/* GPU time of a code region measured on the device (replaces the CUPTI activity records of
 * cupti_src/CuptiProfiler.cpp:168-207 without a hipEvent read-back): nvrx_stamp_begin enqueues a one-thread
 * kernel on `stream` that stores the constant-rate wall clock; nvrx_stamp_end enqueues one that appends the
 * elapsed MICROSECONDS (CuptiProfiler.cpp:191) to `row`'s ring and, when cpu_row >= 0, also appends the
 * host-measured `cpu_value` to `cpu_row`'s ring (the section's wall time, straggler.py:343), so a profiled
 * section entry costs no pinned-memory staging.  Reports are ordered after these kernels on the device;
 * the host never waits for them.  Regions on one row nest LIFO.
 * A region whose stream is being captured into a hipGraph (hipStreamIsCapturing) records nothing -- a captured timestamp
 * would replay into one fixed ring slot, and the reference sees no kernel during a capture either: begin AND the matching
 * end return NVRX_REGION_SKIPPED (> 0), nothing is enqueued, cpu_value is NOT taken (the caller pushes it itself).  The
 * same holds for nvrx_event_begin / nvrx_event_end.  nvrx_ctx_info(ctx, 7) counts such regions. */
#define NVRX_REGION_SKIPPED 1
int nvrx_stamp_begin(nvrx_ctx *ctx, int row, void *stream);
int nvrx_stamp_end(nvrx_ctx *ctx, int row, int cpu_row, float cpu_value, void *stream);

/* Local half of a report: flush -> row statistics for every row -> write this GPU's
 * `local_ranks` exchange rows.
 *   d_stats [local_ranks*rows_per_rank][NVRX_STATS_STRIDE] out
 *   d_send  [local_ranks][L] out, L = NVRX_TABLE_LEN(K,S) (rows without a gid are not exchanged);
 *           NULL = statistics only: nothing is exchanged and the history minima are left alone
 *   names_ok: value of the flag word for these ranks (has ids for all names);
 *   rows_active: only rows [0, rows_active) of every logical rank are processed (0 = all).
 * Replaces straggler.py:236-237 + the packing loops of reporting.py:273-279. Also folds in
 * _update_local_min_times (reporting.py:298-314): hmin[row] = min(hmin[row], MED). */
int nvrx_report_local(nvrx_ctx *ctx, float *d_stats, float *d_send, int K, int S, int names_ok,
                      int rows_active, void *stream);
/* A whole report in ONE call: flush -> row statistics -> [all-gather of the exchange rows] -> scoring of the
 * table -> (optionally) wait for the completion word.  The descriptor is filled once per report shape and reused;
 * the library advances `seq` itself, so a steady-state report is a single FFI crossing.
 * `stream` is where the report runs unless it is RE-HOMED: a synchronous report (h_seq_word given, guard_rings 0) that
 * must follow the work of exactly one other stream -- the stream the window's region stamps (nvrx_stamp_end) were
 * launched on and / or order_after_stream -- is enqueued on THAT stream instead, so that the stream order is the
 * dependency and no event is recorded or waited for (NVRX_DEBUG_REPORT_REHOME=0 keeps it on `stream` behind event waits).
 * Replaces Detector.generate_report's body (straggler.py:236-239) + ReportGenerator.generate_report
 * (reporting.py:421-554) for the case where the summaries never leave the device. */
typedef struct nvrx_report_desc {
    int32_t R, K, S;          /* table shape: ranks, kernel ids, section ids */
    int32_t names_ok;         /* this process has ids for all of its names */
    int32_t rows_active;      /* rows per logical rank to process (0 = all) */
    int32_t do_indiv, do_rel; /* score families to compute */
    int32_t stats_rows;       /* statistics rows to forward to d_stats_dst */
    double thresholds[4];     /* gpu_rel, section_rel, gpu_indiv, section_indiv */
    float *d_stats;           /* [local_ranks*rows_per_rank][NVRX_STATS_STRIDE] device */
    float *d_send;            /* [local_ranks][L] device: this process' exchange rows */
    float *d_table;           /* [R][L] device: all ranks' rows (ignored when allgather_fn is NULL) */
    float *d_scores;          /* result block, device-visible addresses (nvrx_host_alloc's *out_device):    */
    uint8_t *d_flags;         /*   16-byte aligned, each array padded to a multiple of 16 bytes              */
    uint32_t *d_meta;         /*   NVRX_META_WORDS words; [4] is the completion word                         */
    float *d_stats_dst;       /*   or NULL                                                                   */
    uint32_t *d_done_counter; /* device word, zero before the first report */
    void *allgather_fn;       /* NULL = single process, no exchange; else an ncclAllGather-compatible function
                                 int (*)(const void *send, void *recv, size_t count, int dtype, void *comm, void *stream) */
    void *comm;               /* its communicator */
    int32_t send_count;       /* floats this process contributes (local_ranks * L) */
    uint32_t seq;             /* last published sequence number (in/out) */
    const uint32_t *h_seq_word; /* host address of meta[4]; NULL = do not wait */
    double timeout_s;         /* <= 0: wait for ever, like a blocking collective */
    void *order_after_stream; /* hipStream_t whose already-enqueued work the report must follow (device-side wait,
                                 the host does not block), or NULL; takes the place of torch.cuda.synchronize()
                                 in straggler.py:234 for the collectives the caller has enqueued there */
    int32_t order_after_enabled; /* 0: order_after_stream is ignored */
    int32_t resident;         /* nonzero: the library may run the score kernel RESIDENT on a stream of its own next to the
                                 statistics kernel (rows handed over as 8-byte tagged granules instead of through the
                                 stream order); used for synchronous reports without an exchange or with the peer-window
                                 exchange that have no other stream's work to wait for (NVRX_DEBUG_RESIDENT_SCORER=0|1|2: never /
                                 that rule / always).  The statistics rows then land under their own completion word d_meta[5]. */
    int32_t prev_settled;     /* nonzero: the caller has seen this context's previous asynchronous report complete (it polled
                                 that report's completion word): ring writers need not wait for it any more, and an
                                 asynchronous report that comes rarely enough may be enqueued on the one stream it follows */
    int32_t guard_rings;      /* asynchronous reports (h_seq_word == NULL, the caller polls later): nonzero makes later
                                 device-side ring writers on other streams (nvrx_stamp_end) wait, on the device, for this
                                 report's statistics kernel */
} nvrx_report_desc;
int nvrx_report(nvrx_ctx *ctx, nvrx_report_desc *desc, void *stream);
/* The synchronous report in two calls, for a caller that has host work of its own to do while the GPU runs (building the
 * object that will read the result block, emptying the rings): nvrx_report(ctx, desc, stream) with h_seq_word set IS
 * nvrx_report_issue followed by nvrx_report_wait.
 * nvrx_report_issue does everything up to the last launch -- re-homing, the resident score kernel's stream, flush,
 * statistics kernel, the exchange, score kernel -- and decides all of it as a SYNCHRONOUS report (no ring guards, resident
 * scorer allowed); desc->seq is advanced on return.  NVRX_ERR_INVALID, before any device is touched: a null context or
 * descriptor, a null buffer, an exchange without a table of its own, or a descriptor without h_seq_word (asynchronous reports
 * go through nvrx_report).  NVRX_ERR_STATE: a report is already pending on the context.  After a failed issue nothing is
 * pending.
 * nvrx_report_wait waits for that report's completion word (desc->timeout_s, NVRX_ERR_TIMEOUT) and does the bookkeeping the
 * one-call form does behind its wait.  NVRX_ERR_INVALID: null argument; NVRX_ERR_STATE: nothing is pending, or `desc` is not
 * the pending report's descriptor (that report is given up: its results are not to be read).  After any return nothing is
 * pending.
 * Between the two calls the descriptor, the result block and the context's streams are the report's: of this context's
 * entry points only nvrx_ring_reset may be called (see there), and nothing that enqueues on the context's stream -- the
 * wait takes the completion word as proof that the context's stream has drained, which holds for nothing enqueued later.
 * The follow-ups (nvrx_report_attribute, ...) come after the wait. */
int nvrx_report_issue(nvrx_ctx *ctx, nvrx_report_desc *desc, void *stream);
int nvrx_report_wait(nvrx_ctx *ctx, nvrx_report_desc *desc);
/* nvrx_attribute (reporting.py:219-253, above) on the table of the report LAST issued through `desc` on `ctx` (d_table, or
 * d_send without an exchange; shape and families from the descriptor).  The library orders the kernel behind that report's
 * kernels itself: it is enqueued on the context's stream (nvrx_ctx_set_stream), behind an event of the stream the report's
 * last kernel went to when that was another one (a re-homed report, the resident score kernel).  The host does not wait;
 * copy d_out with a D2H on the context's stream.  The caller must not let a later report rewrite the table before this
 * kernel has run (the Python package waits for it at the start of the next report on the same buffers).
 * NVRX_ERR_STATE: no report was issued through this descriptor. */
int nvrx_report_attribute(nvrx_ctx *ctx, const nvrx_report_desc *desc, int first_rank, int n_ranks, int top_n, void *d_out);
/* nvrx_row_quantile (straggler.py:172-197, above) on the rings as the report just issued saw them, packed by gid into
 * d_tail_send [local_ranks][K+S]: kernel ids first, then section ids; every slot is written, -1.0 where no row with samples
 * has that gid.  Staged samples are NOT flushed (the window is the one the report's statistics kernel read) and the history
 * minima are not touched.  desc != NULL: the report went through nvrx_report; the kernel is enqueued on the context's stream
 * behind that report's last kernel, as nvrx_report_attribute orders itself (NVRX_ERR_STATE: no report was issued through
 * this descriptor).  desc == NULL: the stepwise path; it runs on `stream`, where nvrx_report_local ran.  rows_active as for
 * nvrx_report_local.  The host does not wait -- but the caller must: the rings are emptied by count, and the next window's
 * device-side writers on other streams may overwrite slots as soon as they are told to. */
int nvrx_tail_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, uint32_t q_ppm, float *d_tail_send, int K, int S,
                    int rows_active, void *stream);
/* Onset scores on the rings.  nvrx_onset_enable(ctx, 1): from now on every report (nvrx_report_local with a d_send,
 * nvrx_report, nvrx_window_report) snapshots, right after it has flushed the staged samples, the slot of every ring's oldest
 * sample; 0 switches that off again.  With the switch off a report does nothing it did not do before.
 * nvrx_onset_local: nvrx_row_onset on the rings as the report just issued saw them -- its counts, its ring starts, whatever
 * has been pushed since -- packed by gid into d_onset_send [local_ranks][NVRX_ONSET_PLANES][K+S] (planes {e, before, after,
 * strength, ago as f32, n as f32}; kernel ids first, then section ids; every slot is written, -1.0 where no row with samples has that gid).  min_strength
 * in [0, 1].  Ordering, desc, rows_active and the caller's duty to wait are those of nvrx_tail_local.
 * NVRX_ERR_STATE: not enabled, or no report was issued through this descriptor.
 * The snapshot nvrx_onset_enable switches on is also what nvrx_period_local and nvrx_episode_local walk their windows by: a
 * caller that wants period or episode scores enables it whether or not it wants onsets. */
int nvrx_onset_enable(nvrx_ctx *ctx, int on);
int nvrx_onset_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, uint32_t min_seg_ppm, float min_strength,
                     float *d_onset_send, int K, int S, int rows_active, void *stream);
/* Period scores on the rings: nvrx_row_period on the rings as the report just issued saw them -- its counts, its ring starts
 * (the snapshot of nvrx_onset_enable), whatever has been pushed since -- packed by gid into d_period_send
 * [local_ranks][NVRX_PERIOD_PLANES][K+S] (planes {e, peak, rest, strength, period as f32, ago as f32, n as f32}; kernel ids
 * first, then section ids; every slot is written, -1.0 where no row with samples has that gid).  max_period in
 * [2, NVRX_PERIOD_MAX], min_strength in [0, 1].  Ordering, desc, rows_active and the caller's duty to wait are those of
 * nvrx_onset_local.  NVRX_ERR_STATE: the snapshot is not enabled, or no report was issued through this descriptor. */
int nvrx_period_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, int max_period, float min_strength,
                      float *d_period_send, int K, int S, int rows_active, void *stream);
/* Episode scores on the rings (straggler.py:172-197 on the window in time order; reporting.py:196-253 follows with
 * nvrx_episode_score): nvrx_row_episode on the rings as the report just issued saw them -- its counts, its ring starts (the
 * snapshot of nvrx_onset_enable), whatever has been pushed since -- packed by gid into d_episode_send
 * [local_ranks][NVRX_EPISODE_PLANES][K+S] (planes {e, inside, outside, strength, length as f32, ago as f32, n as f32}; kernel
 * ids first, then section ids; every slot is written, -1.0 where no row with samples has that gid).  min_len_ppm in
 * [1, 333333], min_strength in [0, 1].  Ordering, desc, rows_active and the caller's duty to wait are those of
 * nvrx_onset_local.  NVRX_ERR_STATE: the snapshot is not enabled, or no report was issued through this descriptor. */
int nvrx_episode_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, uint32_t min_len_ppm, float min_strength,
                       float *d_episode_send, int K, int S, int rows_active, void *stream);
/* nvrx_robust_score (reporting.py:196-253, above) on the table of the report LAST issued through `desc` on `ctx` (d_table,
 * or d_send without an exchange; shape from the descriptor).  Ordered behind that report's kernels exactly as
 * nvrx_report_attribute orders itself: the context's stream, with an event when the report's last kernel ran elsewhere.  The
 * host does not wait; copy d_out with a D2H on the context's stream, and do not let a later report rewrite the table before
 * the kernels have run.  NVRX_ERR_STATE: no report was issued through this descriptor. */
int nvrx_report_robust(nvrx_ctx *ctx, const nvrx_report_desc *desc, int first_rank, int n_ranks, int min_ranks,
                       float floor_rel, void *d_out);
/* nvrx_peer_score (above) on the table of the report LAST issued through `desc` on `ctx` (d_table, or d_send without an
 * exchange; shape from the descriptor; d_groups sized for the descriptor's R).  Ordered behind that report's kernels exactly
 * as nvrx_report_robust orders itself: the context's stream, with an event when the report was re-homed or scored resident.
 * The host does not wait; copy d_out with a D2H on the context's stream, and do not let a later report rewrite the table
 * before the kernels have run.  NVRX_ERR_STATE: no report was issued through this descriptor. */
int nvrx_report_peer(nvrx_ctx *ctx, const nvrx_report_desc *desc, const int32_t *d_groups, int G, int first_rank, int n_ranks,
                     int min_ranks, void *d_out);
/* nvrx_pace_score (above) on the table of the report LAST issued through `desc` on `ctx` (d_table, or d_send without an
 * exchange; shape from the descriptor).  Ordered behind that report's kernels exactly as nvrx_report_robust orders itself: the
 * context's stream, with an event when the report was re-homed or scored resident.  The host does not wait; copy d_out with a
 * D2H on the context's stream, and do not let a later report rewrite the table before the kernels have run.  NVRX_ERR_STATE:
 * no report was issued through this descriptor. */
int nvrx_report_pace(nvrx_ctx *ctx, const nvrx_report_desc *desc, int first_rank, int n_ranks, int min_ranks, void *d_out);
/* nvrx_pace_group_score (above) on the table of the report LAST issued through `desc` on `ctx` (d_table, or d_send without an
 * exchange; shape from the descriptor; d_groups sized for the descriptor's R).  Ordered behind that report's kernels exactly as
 * nvrx_report_pace orders itself: the context's stream, with an event when the report was re-homed or scored resident.  The
 * host does not wait; copy d_out with a D2H on the context's stream, and do not let a later report rewrite the table before
 * the kernels have run.  NVRX_ERR_STATE: no report was issued through this descriptor. */
int nvrx_report_pace_group(nvrx_ctx *ctx, const nvrx_report_desc *desc, const int32_t *d_groups, int G, int max_group,
                           int first_rank, int n_ranks, int min_ranks, int min_peers, void *d_out);
/* nvrx_node_score (above) on the table of the report LAST issued through `desc` on `ctx` (d_table, or d_send without an
 * exchange; shape from the descriptor; d_groups sized for the descriptor's R).  Ordered behind that report's kernels exactly as
 * nvrx_report_pace_group orders itself: the context's stream, with an event when the report was re-homed or scored resident.
 * The host does not wait; copy d_out with a D2H on the context's stream, and do not let a later report rewrite the table before
 * the kernels have run.  NVRX_ERR_STATE: no report was issued through this descriptor. */
int nvrx_report_node(nvrx_ctx *ctx, const nvrx_report_desc *desc, const int32_t *d_groups, int G, int max_group, int min_members,
                     int min_nodes, int first_rank, int n_ranks, void *d_out);
/* nvrx_work_groups (above) on the table of the report LAST issued through `desc` on `ctx` (d_table, or d_send without an
 * exchange; shape from the descriptor).  Ordered behind that report's kernels exactly as nvrx_report_peer orders itself: the
 * context's stream, with an event when the report was re-homed or scored resident.  The host does not wait; copy d_out with a
 * D2H on the context's stream, and do not let a later report rewrite the table before the kernels have run.  NVRX_ERR_STATE:
 * no report was issued through this descriptor. */
int nvrx_report_work(nvrx_ctx *ctx, const nvrx_report_desc *desc, float count_tol, int max_unlike_ppm, void *d_out);
/* nvrx_score_history (above) on the result block of the report LAST issued through `desc` on `ctx` (desc->d_scores; R and S
 * from the descriptor).  Ordered behind that report's last kernel exactly as nvrx_report_robust orders itself: the context's
 * stream, with an event when the report was re-homed or scored resident.  The host does not wait; copy d_out with a D2H on the
 * context's stream, and do not let a later report rewrite that block before the kernel has run.  NVRX_ERR_STATE: no report
 * was issued through this descriptor. */
int nvrx_report_history(nvrx_ctx *ctx, const nvrx_report_desc *desc, int first_rank, int n_ranks, float *d_hist, int S_cap,
                        int H, uint64_t n_before, const double *thresholds, void *d_out);
/* nvrx_score_trend (above) on the context's stream -- the stream nvrx_report_history launched on.  The ring's only writers
 * are history steps on that stream, so the launch is ordered behind the step it follows without an event.  The host does not
 * wait; copy d_out with a D2H on the context's stream. */
int nvrx_report_trend(nvrx_ctx *ctx, const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports,
                      void *d_out);
/* nvrx_peer_history and nvrx_peer_trend (above) on the context's stream -- the stream nvrx_report_peer launched on, so a
 * step is ordered behind the peer step whose rank part it reads (d_peer: that step's d_out + 16 G (K+S) bytes) and behind the
 * ring's earlier steps without an event.  The host does not wait; copy d_out with a D2H on the context's stream, and do not
 * let a later peer step rewrite the block before the kernel has run.  NVRX_ERR_STATE: no report was issued on this context. */
int nvrx_report_peer_history(nvrx_ctx *ctx, const float *d_peer, int n_ranks, int S, float *d_hist, int S_cap, int H,
                             uint64_t n_before, const double *thresholds, void *d_out);
int nvrx_report_peer_trend(nvrx_ctx *ctx, const float *d_hist, int n_ranks, int S, int S_cap, int H, uint64_t n_reports,
                           void *d_out);
/* The local step of the slack scores (nvrx_slack_score, above) on the STATISTICS of the report last issued -- it reads the
 * statistics rows, not the rings.  rows[i], cols[i], i < n: host arrays, the collective rows of a logical rank (row within the
 * rank, the same for every logical rank) in ascending order with their columns; the library keeps the list in device memory
 * and uploads it, on the step's stream, only when it differs from the one it holds.  d_send [local_ranks][2][64], 16-byte
 * aligned; every slot is written.  desc != NULL: the report went through nvrx_report; the rows are desc->d_stats (the
 * statistics kernel writes them there also when the score kernel ran resident; d_stats is ignored), and the kernel is enqueued
 * on the context's stream behind that report's last kernel and behind its statistics kernel.  desc == NULL: the stepwise path,
 * on `stream` with the d_stats nvrx_report_local wrote there.  rows_active as for nvrx_report_local.  The host does not wait
 * -- but the caller must before the next report, which rewrites the statistics.  NVRX_ERR_INVALID: a null pointer, n outside
 * [0, rows_per_rank], rows not ascending, rows_active out of range, d_send misaligned; NVRX_ERR_RANGE: a row outside [0,
 * rows_per_rank) or a column outside [0, 64); NVRX_ERR_STATE: no report was issued through this descriptor. */
int nvrx_slack_local(nvrx_ctx *ctx, const nvrx_report_desc *desc, const float *d_stats, const int32_t *rows, const int32_t *cols,
                     int n, float *d_send, int rows_active, void *stream);
/* One report WINDOW in one call: what straggler.py:228-244 does around the report in the steady state -- wait for the
 * window's GPU measurements (torch.cuda.synchronize() + the profiler's get_stats there; here the kernel tracer's sync, or a
 * harvest of the region events), check that the set of rows holding samples is the one the caller's name tables were built
 * for, run nvrx_report, empty the rings (straggler.py:241-242).  The kernel tracer lives in another library
 * (include/nvrx_ktrace.h): its three entry points are handed over as plain function pointers.
 * Returns NVRX_OK (the report ran -- for asynchronous ones: was enqueued -- and the rings are empty), NVRX_WINDOW_MISS
 * (NOTHING ran: dispatches still missing after the patience, kernel keys the host has not learnt yet, or the occupied rows
 * changed -- the caller takes its general path), NVRX_WINDOW_NAMES (synchronous only: the report ran and its table says some
 * rank has names without ids; the rings were NOT emptied -- the caller syncs names and reports again), or a negative error. */
#define NVRX_WINDOW_MISS 1
#define NVRX_WINDOW_NAMES 2
typedef struct nvrx_window_desc {
    int (*kt_sync)(double timeout_s);  /* nvrx_ktrace_sync, or NULL: GPU time is measured per region */
    int (*kt_hold)(int on);            /* nvrx_ktrace_hold: brackets "statistics launch + ring reset" of an asynchronous report */
    uint64_t (*kt_counter)(int what);  /* nvrx_ktrace_counter */
    double kt_patience_s;              /* how long a synchronous report waits for the window's kernel records */
    uint64_t kt_rows_known;            /* the host's copies of tracer counters 10 and 6: a difference = kernel keys to learn */
    uint64_t kt_keys_without_row;
    int32_t rows_used;                 /* rows the caller's name tables cover (as for nvrx_ring_occupancy_changed) */
    int32_t asynchronous;              /* nonzero: desc->h_seq_word is NULL, the report is only enqueued, nothing is waited for */
    int32_t harvest_regions;           /* region timing: nvrx_event_harvest before the report */
    int32_t out_names_ok;              /* out: 0 when NVRX_WINDOW_NAMES was returned */
} nvrx_window_desc;
int nvrx_window_report(nvrx_ctx *ctx, nvrx_report_desc *desc, void *stream, nvrx_window_desc *window);
/* Diagnostics: host clocks of this thread's last nvrx_window_report, microseconds on the monotonic clock -- [0] entry, [1]
 * the wait for the window's measurements and the occupancy look are done, nvrx_report begins (its own clocks follow). */
int nvrx_window_clocks(double *out2);
/* Diagnostics: host clocks of this thread's last nvrx_report, microseconds on the monotonic clock -- [0] entry, [1] stream
 * ordering done, [2] staged samples flushed, [3] statistics kernel launched, [4] exchange enqueued, [5] score kernel
 * launched, [6] completion word seen (synchronous reports), [7] spare.  No counterpart in the reference. */
int nvrx_report_clocks(double *out8);
/* sizeof(nvrx_report_desc) as this library was compiled: lets an FFI binding check its own struct layout. */
int nvrx_report_desc_size(void);
/* ------------------------------------------------------------------------------------------------
 * Peer-window exchange: the report's one collective as direct xGMI peer stores between the processes of ONE node.
 * Replaces all_reduce(MIN) + gather of reporting.py:281,397 (as the RCCL all-gather does) without an RCCL kernel:
 * every process owns a window of 8-byte {epoch, f32} granules in fine-grained device memory, mapped by all
 * processes through HIP IPC; nvrx_peer_allgather enqueues ONE single-workgroup kernel that stores this process'
 * floats into every window and polls its own window until every rank's floats of this epoch have arrived.
 * Collective set-up (cold): create -> exchange the 64-byte IPC handles out of band -> connect each peer -> ready.
 * Every process must call nvrx_peer_allgather the same number of times (the epoch is counted, not passed).
 * ---------------------------------------------------------------------------------------------- */
typedef struct nvrx_peer nvrx_peer;
int nvrx_peer_create(int device, int world, int rank, int max_floats_per_rank, nvrx_peer **out);
int nvrx_peer_ipc_handle(nvrx_peer *peer, void *handle64 /* 64 bytes out */);
int nvrx_peer_connect(nvrx_peer *peer, int peer_rank, const void *handle64);
/* PCI bus id of the window's device ("0000:05:00.0"): the same string in every process, whatever HIP_VISIBLE_DEVICES. */
int nvrx_peer_device_id(const nvrx_peer *peer, char *out, int len);
/* Before nvrx_peer_connect: can this window's device store into the device named by peer_pci_bus_id?  0 yes (or the same
 * device); 1 the peer's device is not visible to this process (nothing to check, the IPC mapping decides); negative with
 * nvrx_last_error() saying why not (hipDeviceCanAccessPeer = 0).  The reference has no counterpart: its exchange is
 * torch.distributed (reporting.py:281,397), whose transport NCCL picks. */
int nvrx_peer_check_access(const nvrx_peer *peer, int peer_rank, const char *peer_pci_bus_id);
/* timeout_s: how long the kernel polls for a late peer before it gives up (<= 0 keeps the default 1800 s). */
int nvrx_peer_ready(nvrx_peer *peer, double timeout_s);
/* ncclAllGather-compatible: (send, recv, floats per rank, dtype = 7 (f32), comm = the nvrx_peer, stream); returns 0
 * or a positive code.  Usable as nvrx_report_desc.allgather_fn (address: nvrx_peer_allgather_address()). */
int nvrx_peer_allgather(const void *send, void *recv, size_t count, int dtype, void *comm, void *stream);
void *nvrx_peer_allgather_address(void);
/* Epoch of the last exchange in which the kernel gave up waiting for a peer (0 = never). */
int nvrx_peer_error(const nvrx_peer *peer, uint32_t *epoch_out);
int nvrx_peer_destroy(nvrx_peer *peer);

/* Re-initialise an exchange buffer with the "no stats" sentinels (call when ids change). */
int nvrx_send_init(float *d_send, int rows, int K, int S, void *stream);

/* Kernel-time instrumentation for the benchmark: when enabled, nvrx_report_local launches its
 * statistics kernel through hipExtLaunchKernel with a start/stop hipEvent pair, which receive the
 * kernel's own begin/end timestamps on the launch stream; totals are read back here (blocks until
 * the recorded events complete). */
int nvrx_timing_enable(nvrx_ctx *ctx, int on);
int nvrx_timing_read(nvrx_ctx *ctx, double *total_us, int *launches, int reset);

/* Small asynchronous D2H into pinned memory + completion tracking for the report results. */
/* Pinned, device-mapped host memory; *out_device (optional) receives the address kernels use. */
int nvrx_host_alloc(void **out, void **out_device, size_t bytes);
/* Zero-initialised device memory on the current device, for hosts without an allocator of their own (the Python package
 * hands over tensor.data_ptr(); tests/c_abi/abi_host.c, plain C, uses these).  No counterpart in the reference. */
int nvrx_device_alloc(void **out, size_t bytes);
int nvrx_device_free(void *p);
/* Spin until *h_word == expected (acquire); NVRX_ERR_TIMEOUT after timeout_s seconds. */
int nvrx_poll_u32(const uint32_t *h_word, uint32_t expected, double timeout_s);
int nvrx_host_free(void *p);
int nvrx_copy_to_host(nvrx_ctx *ctx, void *h_dst, const void *d_src, size_t bytes, void *stream);
/* Stateless: asynchronous D2H on `stream`, then wait for the stream (report results -> pinned host). */
int nvrx_d2h_sync(void *h_dst, const void *d_src, size_t bytes, void *stream);
/* Block (spin) until the last nvrx_copy_to_host on this context has landed. */
int nvrx_wait(nvrx_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* NVRX_STRAGGLER_H */
