// cp_bop_match / cp_bop_scores: the last step of BOP's evaluation -- bop_toolkit_lib/pose_matching.py:9-90
// (match_poses) for every (scene, image, object) group and every threshold column in one launch, and score.py:62-137
// (calc_localization_scores) for every column at once.  The reference repeats both once per (tau, threshold) pair, 120 passes of
// Python dict loops for one BOP'19 evaluation; here a column is a lane.
//
// cp_bop_match, one launch (bop_match_kernel), a workgroup per group, lanes over the columns:
//   1. every output row of the group is set to "unmatched" (est_id -1, score / error / error_norm -1.0, the reference's defaults);
//      for a group on the scratch mask, its words are initialised with the INVALID ground truths' bits set;
//   2. the estimates' order: thread i ranks estimate i = #{k: score_k > score_i, or score_k == score_i and k < i} -- Python's stable
//      sorted(reverse=True); NaN ranks below everything, so the ranks are a permutation whatever the scores are.  order[rank] = i
//      goes to the caller's scratch (one int32 per estimate);
//   3. the group's n_e x n_g x C_err error block is staged through LDS when it fits in 4096 doubles, else read where it lies;
//   4. lane c walks the estimates in that order (the first max_ests of them when max_ests > 0) and, for each, scans the ground
//      truths SEQUENTIALLY in slot order (= increasing gt_id): a candidate replaces the best so far only if every element is
//      strictly below it, the best so far starting at the thresholds -- for E = 2 this is no total order and the result depends on
//      the scan order, so there is no arg-min reduction here.  NaN and inf never pass `<`.  The unavailable set (invalid or matched)
//      is a 64-bit register for n_g <= 64 and ceil(n_g / 64) words of the caller's scratch above that (word-major, column-minor:
//      a wave's lanes touch consecutive words).
// No lane waits for another after the one barrier; no private scratch; every output is a function of comparisons and one fp64
// division: bit-identical from call to call, for a group alone or in a batch, a column alone or among others, staged or not,
// register mask or scratch mask.
//
// cp_bop_scores, three launches (bop_scores_zero_kernel, bop_scores_targets_kernel, bop_scores_tp_kernel): integer counts only --
// targets per group = min(n_top, valid ground truths) (or the count when n_top <= 0) added to the total, the object's and the
// scene's bin; true positives = valid ground truths with est_id != -1 per column, counted through LDS bins (64 columns x bins per
// workgroup, one integer atomicAdd per non-zero bin at the end) when 1 + n_obj + n_scene <= 128, else with integer atomics on the
// output.  Integer sums are order-independent; the quotients and means are the caller's, in fp64 (bop_eval.py).
#include "common.h"

namespace {

constexpr int BM_THREADS = 256;
constexpr int BM_LDS_DOUBLES = 4096;              // 32 KiB
constexpr int BS_THREADS = 256, BS_COLS = 64, BS_ROWS = 256, BS_LDS_BINS = 128;

struct BmParams {
  const double* errs;          // (P, C_err)
  const double* est_score;     // (NE)
  const int32_t* est_id;       // (NE)
  const int32_t* est_off;      // (G + 1)
  const int32_t* gt_off;       // (G + 1)
  const long long* pair_off;   // (G + 1)
  const int32_t* gt_rows;      // (NG) slot -> output row, or nullptr = identity
  const uint8_t* gt_valid;     // (NG) by output row, or nullptr = all valid
  const int32_t* col_err;      // (C, E)
  const double* col_th;        // (C, E)
  const int32_t* mask_off;     // (G) first scratch word of the group, or nullptr
  int32_t* out_est;            // (NG, C)
  double* out_score;           // (NG, C)
  double* out_err;             // (NG, C, E)
  double* out_norm;            // (NG, C, E)
  int32_t* order;              // scratch: (NE)
  unsigned long long* masks;   // scratch: (mask_words, C)
  long long P, mask_words;
  int C_err, NE, NG, G, C, E, max_ests;
  unsigned flags;
};

__device__ __forceinline__ bool bm_score_above(double a, double b) { return a > b || (b != b && a == a); }   // NaN is the lowest
__device__ __forceinline__ bool bm_score_same(double a, double b) { return a == b || (a != a && b != b); }

// slot j of the group -> output row, or -1 (a row outside the table: skipped everywhere)
__device__ __forceinline__ int bm_row(const BmParams& p, int g0, int j) {
  const int r = p.gt_rows ? p.gt_rows[g0 + j] : g0 + j;
  return (r >= 0 && r < p.NG) ? r : -1;
}

__device__ __forceinline__ bool bm_usable(const BmParams& p, int g0, int j) {
  const int r = bm_row(p, g0, j);
  return r >= 0 && (!p.gt_valid || p.gt_valid[r] != 0);
}

__global__ __launch_bounds__(BM_THREADS) void bop_match_kernel(BmParams p) {
#pragma clang fp contract(off)
  __shared__ double s_err[BM_LDS_DOUBLES];
  const int g = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int e0 = p.est_off[g], e1 = p.est_off[g + 1], g0 = p.gt_off[g], g1 = p.gt_off[g + 1];
  const long long p0 = p.pair_off[g];
  if (g0 < 0 || g1 < g0 || g1 > p.NG) return;                        // (uniform) nothing of this group can be addressed
  const int n_g = g1 - g0;
  int n_e = e1 - e0;
  if (e0 < 0 || n_e < 0 || e1 > p.NE || p0 < 0 || p0 + (long long)n_e * n_g > p.P) n_e = 0;     // a broken table: all unmatched
  const int words = (n_g + 63) >> 6;
  const bool reg_mask = n_g <= 64 && !(p.flags & CP_BOP_MATCH_SCRATCH_MASK);
  long long mo = 0;
  if (!reg_mask) {
    mo = p.mask_off ? (long long)p.mask_off[g] : -1;
    if (!p.masks || mo < 0 || mo + words > p.mask_words) n_e = 0;
  }
  const long long block = (long long)n_e * n_g * p.C_err;
  const bool staged = block <= BM_LDS_DOUBLES && !(p.flags & CP_BOP_MATCH_NO_LDS);

  // ---- 1. the defaults; the scratch words with the invalid bits set
  for (long long idx = tid; idx < (long long)n_g * p.C; idx += nt) {
    const int j = (int)(idx / p.C), c = (int)(idx % p.C);
    const int r = bm_row(p, g0, j);
    if (r < 0) continue;
    const size_t at = (size_t)r * p.C + c;
    p.out_est[at] = -1;
    p.out_score[at] = -1.0;
    for (int k = 0; k < p.E; ++k) { p.out_err[at * p.E + k] = -1.0; p.out_norm[at * p.E + k] = -1.0; }
  }
  if (!reg_mask && n_e > 0) {
    for (long long idx = tid; idx < (long long)words * p.C; idx += nt) {
      const int w = (int)(idx / p.C), c = (int)(idx % p.C);
      unsigned long long m = 0;
      for (int b = 0; b < 64; ++b) {
        const int j = w * 64 + b;
        if (j >= n_g || !bm_usable(p, g0, j)) m |= 1ull << b;
      }
      p.masks[((size_t)mo + w) * p.C + c] = m;
    }
  }
  // ---- 2. the stable descending order of the scores
  for (int i = tid; i < n_e; i += nt) {
    const double s = p.est_score[e0 + i];
    int rank = 0;
    for (int k = 0; k < n_e; ++k) {
      const double sk = p.est_score[e0 + k];
      rank += (bm_score_above(sk, s) || (bm_score_same(sk, s) && k < i)) ? 1 : 0;
    }
    p.order[e0 + rank] = i;
  }
  // ---- 3. the error block
  if (staged)
    for (int idx = tid; idx < (int)block; idx += nt) s_err[idx] = p.errs[(size_t)p0 * p.C_err + idx];
  __syncthreads();                                                   // the only barrier: LDS, order and mask words are the group's own
  if (n_e == 0) return;
  const double* __restrict__ src = staged ? s_err : p.errs + (size_t)p0 * p.C_err;
  const int n_use = p.max_ests > 0 ? min(n_e, p.max_ests) : n_e;
  const bool two = p.E == 2;

  // ---- 4. a column per lane
  for (int c = tid; c < p.C; c += nt) {
    const int ci0 = p.col_err[(size_t)c * p.E], ci1 = two ? p.col_err[(size_t)c * p.E + 1] : 0;
    if (ci0 < 0 || ci0 >= p.C_err || ci1 < 0 || ci1 >= p.C_err) continue;
    const double th0 = p.col_th[(size_t)c * p.E], th1 = two ? p.col_th[(size_t)c * p.E + 1] : 0.0;
    unsigned long long taken = 0;                                    // register mask: invalid or matched
    if (reg_mask)
      for (int j = 0; j < n_g; ++j)
        if (!bm_usable(p, g0, j)) taken |= 1ull << j;
    for (int k = 0; k < n_use; ++k) {
      const int i = p.order[e0 + k];
      int best = -1;
      double b0 = th0, b1 = th1;
      if (reg_mask) {
        for (int j = 0; j < n_g; ++j) {
          if ((taken >> j) & 1ull) continue;
          const size_t at = ((size_t)i * n_g + j) * p.C_err;
          const double a0 = src[at + ci0], a1 = two ? src[at + ci1] : 0.0;
          if (a0 < b0 && (!two || a1 < b1)) { best = j; b0 = a0; b1 = a1; }
        }
      } else {
        for (int w = 0; w < words; ++w) {
          const unsigned long long m = p.masks[((size_t)mo + w) * p.C + c];
          const int jn = min(64, n_g - w * 64);
          for (int b = 0; b < jn; ++b) {
            if ((m >> b) & 1ull) continue;
            const int j = w * 64 + b;
            const size_t at = ((size_t)i * n_g + j) * p.C_err;
            const double a0 = src[at + ci0], a1 = two ? src[at + ci1] : 0.0;
            if (a0 < b0 && (!two || a1 < b1)) { best = j; b0 = a0; b1 = a1; }
          }
        }
      }
      if (best < 0) continue;
      if (reg_mask) taken |= 1ull << best;
      else p.masks[((size_t)mo + (best >> 6)) * p.C + c] |= 1ull << (best & 63);
      const size_t at = (size_t)bm_row(p, g0, best) * p.C + c;       // (usable, hence a checked row)
      p.out_est[at] = p.est_id[e0 + i];
      p.out_score[at] = p.est_score[e0 + i];
      p.out_err[at * p.E] = b0;
      p.out_norm[at * p.E] = b0 / th0;
      if (two) { p.out_err[at * p.E + 1] = b1; p.out_norm[at * p.E + 1] = b1 / th1; }
    }
  }
}

struct BsParams {
  const int32_t* est;          // (NG, C) cp_bop_match's est_id
  const uint8_t* gt_valid;     // (NG) or nullptr
  const int32_t* gt_obj;       // (NG) index into the caller's object list, -1 = not listed
  const int32_t* gt_scene;     // (NG)
  const int32_t* gt_off;       // (G + 1)
  const int32_t* gt_rows;      // (NG) or nullptr
  int32_t* counts;             // (NB, 1 + C) as [NB targets | NB x C true positives], NB = 1 + n_obj + n_scene
  int NG, G, C, n_obj, n_scene, n_top;
  unsigned flags;
};

__global__ __launch_bounds__(BS_THREADS) void bop_scores_zero_kernel(BsParams p) {
  const long long n = (long long)(1 + p.n_obj + p.n_scene) * (1 + p.C);
  for (long long i = (long long)blockIdx.x * BS_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * BS_THREADS) p.counts[i] = 0;
}

__device__ __forceinline__ bool bs_bins(const BsParams& p, int r, int& o, int& s) {
  o = p.gt_obj[r];
  s = p.gt_scene[r];
  return o >= 0 && o < p.n_obj && s >= 0 && s < p.n_scene;
}

__global__ __launch_bounds__(BS_THREADS) void bop_scores_targets_kernel(BsParams p) {
  const int g = blockIdx.x * BS_THREADS + threadIdx.x;
  if (g >= p.G) return;
  const int g0 = p.gt_off[g], g1 = p.gt_off[g + 1];
  if (g0 < 0 || g1 < g0 || g1 > p.NG) return;
  int count = 0, o = -1, s = -1;
  for (int j = g0; j < g1; ++j) {
    const int r = p.gt_rows ? p.gt_rows[j] : j;
    if (r < 0 || r >= p.NG || (p.gt_valid && !p.gt_valid[r])) continue;
    int oo, ss;
    if (!bs_bins(p, r, oo, ss)) continue;
    o = oo; s = ss;                                                  // (the rows of a group share them)
    count += 1;
  }
  const int t = p.n_top > 0 ? min(p.n_top, count) : count;
  if (t <= 0) return;
  atomicAdd(p.counts, t);
  atomicAdd(p.counts + 1 + o, t);
  atomicAdd(p.counts + 1 + p.n_obj + s, t);
}

__global__ __launch_bounds__(BS_THREADS) void bop_scores_tp_kernel(BsParams p) {
  __shared__ int32_t s_bins[BS_LDS_BINS * BS_COLS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NB = 1 + p.n_obj + p.n_scene;
  const bool lds = NB <= BS_LDS_BINS && !(p.flags & CP_BOP_SCORES_NO_LDS);
  const int c0 = blockIdx.y * BS_COLS, c = c0 + lane;
  if (lds) {
    for (int i = tid; i < NB * BS_COLS; i += BS_THREADS) s_bins[i] = 0;
    __syncthreads();
  }
  int32_t* bins = lds ? s_bins : p.counts + NB;
  const int stride = lds ? BS_COLS : p.C, col = lds ? lane : c;
  const int r0 = blockIdx.x * BS_ROWS, r1 = min(p.NG, r0 + BS_ROWS);
  if (c < p.C) {
    for (int r = r0 + wave; r < r1; r += BS_THREADS / 64) {
      if (p.gt_valid && !p.gt_valid[r]) continue;
      int o, s;
      if (!bs_bins(p, r, o, s)) continue;
      if (p.est[(size_t)r * p.C + c] == -1) continue;
      atomicAdd(bins + col, 1);
      atomicAdd(bins + (size_t)(1 + o) * stride + col, 1);
      atomicAdd(bins + (size_t)(1 + p.n_obj + s) * stride + col, 1);
    }
  }
  if (!lds) return;                                                  // (uniform)
  __syncthreads();
  for (int i = tid; i < NB * BS_COLS; i += BS_THREADS) {
    const int v = s_bins[i], cc = c0 + (i & (BS_COLS - 1));
    if (v != 0 && cc < p.C) atomicAdd(p.counts + NB + (size_t)(i / BS_COLS) * p.C + cc, v);
  }
}

}  // namespace

extern "C" size_t cp_bop_match_scratch_bytes(int NE, long long mask_words, int C) {
  if (NE < 0 || mask_words < 0 || C <= 0) return 0;
  return cp_align16_up((size_t)NE * sizeof(int32_t)) + cp_align16_up((size_t)mask_words * C * sizeof(unsigned long long)) + 16;
}

extern "C" int cp_bop_match(cp_stream_t stream, const double* errs, long long P, int C_err, const double* est_score,
                            const int32_t* est_ids, int NE, const int32_t* est_off, const int32_t* gt_off, const long long* pair_off,
                            int G, const int32_t* gt_rows, const uint8_t* gt_valid, int NG, const int32_t* col_err,
                            const double* col_th, int C, int E, int max_ests, const int32_t* mask_off, long long mask_words,
                            unsigned flags, int32_t* out_est, double* out_score, double* out_err, double* out_norm, void* scratch) {
  if (!est_off || !gt_off || !pair_off || !col_err || !col_th || !out_est || !out_score || !out_err || !out_norm || !scratch)
    return CP_ERR_INVALID;
  if (G <= 0 || NG <= 0 || C <= 0 || C_err <= 0 || NE < 0 || P < 0 || mask_words < 0 || (E != 1 && E != 2)) return CP_ERR_INVALID;
  if ((P > 0 && !errs) || (NE > 0 && (!est_score || !est_ids)) || (mask_words > 0 && !mask_off)) return CP_ERR_INVALID;
  if (flags & ~(unsigned)(CP_BOP_MATCH_NO_LDS | CP_BOP_MATCH_SCRATCH_MASK)) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(errs, 7) || cp_misaligned(est_score, 7) || cp_misaligned(pair_off, 7) ||
      cp_misaligned(col_th, 7) || cp_misaligned(out_score, 7) || cp_misaligned(out_err, 7) || cp_misaligned(out_norm, 7) ||
      cp_misaligned(est_ids, 3) || cp_misaligned(est_off, 3) || cp_misaligned(gt_off, 3) || cp_misaligned(gt_rows, 3) ||
      cp_misaligned(col_err, 3) || cp_misaligned(mask_off, 3) || cp_misaligned(out_est, 3))
    return CP_ERR_ALIGN;
  if (G >= (1 << 30) || (long long)NG * C * E >= (1LL << 40) || P >= (1LL << 40) / C_err) return CP_ERR_RANGE;
  BmParams p = {};
  p.errs = errs; p.P = P; p.C_err = C_err; p.est_score = est_score; p.est_id = est_ids; p.NE = NE; p.est_off = est_off;
  p.gt_off = gt_off; p.pair_off = pair_off; p.G = G; p.gt_rows = gt_rows; p.gt_valid = gt_valid; p.NG = NG; p.col_err = col_err;
  p.col_th = col_th; p.C = C; p.E = E; p.max_ests = max_ests; p.mask_off = mask_off; p.mask_words = mask_words; p.flags = flags;
  p.out_est = out_est; p.out_score = out_score; p.out_err = out_err; p.out_norm = out_norm;
  p.order = (int32_t*)scratch;
  p.masks = mask_words > 0 ? (unsigned long long*)((char*)scratch + cp_align16_up((size_t)NE * sizeof(int32_t))) : nullptr;
  const unsigned threads = C <= 64 ? 64u : (C <= 128 ? 128u : (unsigned)BM_THREADS);
  CP_LAUNCH(bop_match_kernel, dim3((unsigned)G), dim3(threads), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}

extern "C" int cp_bop_scores(cp_stream_t stream, const int32_t* est_ids, const uint8_t* gt_valid, const int32_t* gt_obj,
                             const int32_t* gt_scene, int NG, const int32_t* gt_off, const int32_t* gt_rows, int G, int C,
                             int n_obj, int n_scene, int n_top, unsigned flags, int32_t* counts) {
  if (!est_ids || !gt_obj || !gt_scene || !gt_off || !counts) return CP_ERR_INVALID;
  if (NG <= 0 || G <= 0 || C <= 0 || n_obj <= 0 || n_scene <= 0) return CP_ERR_INVALID;
  if (flags & ~(unsigned)CP_BOP_SCORES_NO_LDS) return CP_ERR_INVALID;
  if (cp_misaligned(est_ids, 3) || cp_misaligned(gt_obj, 3) || cp_misaligned(gt_scene, 3) || cp_misaligned(gt_off, 3) ||
      cp_misaligned(gt_rows, 3) || cp_misaligned(counts, 3))
    return CP_ERR_ALIGN;
  const long long NB = 1LL + n_obj + n_scene;
  if (NB * (1LL + C) >= (1LL << 31) || (long long)NG * C >= (1LL << 40)) return CP_ERR_RANGE;
  const unsigned row_blocks = (unsigned)((NG + BS_ROWS - 1) / BS_ROWS), col_blocks = (unsigned)((C + BS_COLS - 1) / BS_COLS);
  if (col_blocks > 65535u) return CP_ERR_RANGE;
  BsParams p = {};
  p.est = est_ids; p.gt_valid = gt_valid; p.gt_obj = gt_obj; p.gt_scene = gt_scene; p.NG = NG; p.gt_off = gt_off; p.gt_rows = gt_rows;
  p.G = G; p.C = C; p.n_obj = n_obj; p.n_scene = n_scene; p.n_top = n_top; p.flags = flags; p.counts = counts;
  const long long n = NB * (1LL + C);
  const unsigned zero_blocks = (unsigned)((n + BS_THREADS - 1) / BS_THREADS > 1024 ? 1024 : (n + BS_THREADS - 1) / BS_THREADS);
  CP_LAUNCH(bop_scores_zero_kernel, dim3(zero_blocks), dim3(BS_THREADS), 0, (hipStream_t)stream, p);
  CP_LAUNCH(bop_scores_targets_kernel, dim3((unsigned)((G + BS_THREADS - 1) / BS_THREADS)), dim3(BS_THREADS), 0, (hipStream_t)stream, p);
  CP_LAUNCH(bop_scores_tp_kernel, dim3(row_blocks, col_blocks), dim3(BS_THREADS), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}
