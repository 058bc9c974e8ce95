// Calibration of the code logits on the device: how reliable the bits' probabilities are (cp_code_reliability),
// one inverse temperature per group of logit rows fitted by bracketed Newton without a host round trip (cp_fit_code_scale), and whether
// cp_code_confidence's sigma2 is a variance in fact (cp_sigma2_consistency: the histogram of the whitened residuals under the TRUE
// pose).  Rows N32 / N33 read the logits as probabilities; these three are the instrument that says whether they are, and the
// one-parameter-per-row correction when they are not.  The reference has no such step: opt-in, the rule is this project's own
// (tests/calib_stages.py restates it in numpy).
//
// THE RULE.  Everything numeric in fp64 without contraction.  No global atomics; integer results are sums of integers and do not depend
// on the launch shape; every floating sum is formed in ONE fixed order (below), so two calls agree bitwise.
//
// bits (B, rows, N) fp32 logits, `bstride` elements between crops: row 0 the RoI bit, rows 1..r the x bits MSB first, rows 1+r..2r the
// y bits (1 <= r <= 30, rows >= 1 + 2r: the layout cp_code_confidence reads).  Labels: gt_roi (B,1,N), gt_x / gt_y (B,gt_bits >= r,N)
// fp32, a label is SET iff > 0.5 (cp_encode_targets writes 0 / 1).  K = 1 + 2r logit rows.
// Which samples count: row 0 counts every (b, n); the x / y rows count only where the GT RoI bit is set (the reference's
// MaskedCodeLoss, cp_code_report's n_in_roi).
// Per counted sample of row k with logit z (fp32), label y, inverse temperature s_k:
//   z NaN                 the sample goes to n_nan[k] and nowhere else
//   t = (double)z * s_k   one IEEE product; +-inf are ordinary values
//   bin                   = the number of edges <= t (edges ascending, in LOGIT space): a value on an edge goes to the upper bin
//   e = exp(-|t|);  p = t >= 0 ? 1 / (1 + e) : e / (1 + e)
//   nll   = log1p(e) + (y ? max(-t, 0) : max(t, 0))
//   brier = (p - y) (p - y);   g = (p - y) z;   h = (p (1 - p)) (z z)          with z = (double)z: d nll / d s and d2 nll / d s2
// (IEEE all the way: an infinite logit on the right side gives nll 0 and, by 0 * inf, a NaN in g and h; the sums carry it.)
// THE ORDER OF A FLOATING SUM.  The B * N samples, flattened (b, n), are cut into CAL_GRID = 1024 contiguous slices of
// ceil(B N / 1024); workgroup w owns slice w, its 256 lanes take samples slice start + lane + 256 i for i = 0, 1, ..  A lane adds its
// samples in that order (a bin's sum_p: the wave adds the bin's lanes of one step by the butterfly below -- absent lanes add 0.0 --
// then adds that to the bin's running sum); lanes are added by the xor butterfly (v += shuffle_xor(v, d), d = 32, 16, 8, 4, 2, 1);
// the four waves as ((w0 + w1) + w2) + w3; the 1024 workgroup records, in a second one-workgroup launch, in index order from 0.0.
//
// cp_code_reliability -> per (row, bin): count, positives (int64), sum_p; per row: n (the counted samples that are not NaN), n_nan,
//   n_right (the samples whose sign is right: (z > 0) == y, cp_code_report's decision), and the sums of nll, brier, g, h.
// cp_fit_code_scale: every GROUP of rows (group_of_row[k]) minimises the sum of its rows' nll over one shared s: convex in s, g is its
//   derivative and monotone.  The committed iteration per group ("rtsafe"), all of it on the device:
//     s = 1, lo = s_min, hi = s_max (s_min <= 1 <= s_max), evaluation 1, 2, ..:
//       n, nll, g, h at s (the group's rows added in ascending row order); evaluation 1 gives nll_before and n; n == 0: EMPTY, s = 1
//       g < 0 ? lo = s : hi = s
//       c = s - g / h;  if h is not finite, h <= 0 or not lo < c < hi:  c = sqrt(lo * hi)
//       |c - s| <= step_tol * s: CONVERGED (below); else evaluation max_iters reached: NOT_CONVERGED, s = the evaluated point of the
//       lowest nll (the earliest on a tie); else s = c
//     CONVERGED: hi == s_max and s_max - lo <= 3 step_tol s_max (the bracket collapsed onto s_max): s = s_max; lo == s_min and
//       hi - s_min <= 3 step_tol s_min: s = s_min; otherwise s = c.  ONE more evaluation at that s gives nll_after, and decides
//       the capped cases: at s_max, g < 0 is CAPPED_HIGH (the data are separable), at s_min, g > 0 is CAPPED_LOW; everything else OK.
//   A group that has stopped is frozen: later launches skip its rows and leave its numbers untouched.  max_iters + 1 pairs of launches
//   (accumulate over the fixed grid, then one workgroup that adds the records in index order and steps every group) are ENQUEUED at
//   once; no workgroup waits for another.
// cp_sigma2_consistency: per crop, point n counts iff valid, the GT RoI bit is set and both variances are finite and > 0 (row N33's
//   ranked rule); the others go to n_dropped.  du = (double)p2d_x - proj_x, dv likewise; d2 = (du du) / sigma2_x + (dv dv) / sigma2_y;
//   bin = the number of edges <= d2 (chi-square units).  Sums: d2, du / sqrt(sigma2_x), dv / sqrt(sigma2_y) (signed).  One workgroup of
//   256 lanes per crop: lane l adds points l, l + 256, .. in order, then the butterfly, then the waves in order -- a crop alone or in a
//   batch gives the same bits.
// UNPINNED: what a trained network's reliability IS -- no trained weights exist here; this row measures, it does not assume.
#include "common.h"

#pragma clang fp contract(off)

#define CAL_GRID 1024
#define CAL_THREADS 256
#define CAL_WAVES 4
#define CAL_MAX_ROWS 61      // 1 + 2 * 30
#define CAL_MAX_BINS 64
#define CAL_STATE 12         // doubles per group (cp_fit_code_scale_info_doubles)
// state columns
#define CS_S 0
#define CS_LO 1
#define CS_HI 2
#define CS_STATUS 3
#define CS_ITERS 4
#define CS_NLL0 5
#define CS_NLL1 6
#define CS_N 7
#define CS_BEST_S 8
#define CS_BEST_NLL 9
#define CS_PHASE 10          // 0 iterating, 1 the evaluation at the returned s is due, 2 frozen
#define CS_PENDING 11        // phase 1: 0 plain, 1 at s_max, 2 at s_min

namespace {

struct CalTable {            // host tables, passed by value (kernel arguments)
  double scale[CAL_MAX_ROWS];
  double edges[CAL_MAX_BINS - 1];
  int32_t group[CAL_MAX_ROWS];
};

struct CalArgs {
  const float* bits; long long bstride;
  const float* gt_roi; const float* gt_x; const float* gt_y;
  int r, gt_bits, N, M;
  unsigned long long total, chunk;
};

__device__ __forceinline__ double cal_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ unsigned long long cal_wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

struct CalTerm { double t, p, nll, brier, g, h; };
__device__ __forceinline__ CalTerm cal_term(float zf, double s, bool y) {
  CalTerm c;
  const double z = (double)zf;
  c.t = z * s;
  const double e = exp(-fabs(c.t));
  c.p = c.t >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
  const double d = c.p - (y ? 1.0 : 0.0);
  c.nll = log1p(e) + (y ? fmax(-c.t, 0.0) : fmax(c.t, 0.0));
  c.brier = d * d;
  c.g = d * z;
  c.h = (c.p * (1.0 - c.p)) * (z * z);
  return c;
}

// sample i of the flattened (b, n) -> the logit and label of row k, whether it counts
struct CalSample { float z; bool y, counted; };
__device__ __forceinline__ CalSample cal_load(const CalArgs& a, unsigned long long i, bool active, int k) {
  CalSample s;
  s.z = 0.f; s.y = false; s.counted = false;
  if (!active) return s;
  unsigned long long b, n;
  if (i >> 32) { b = i / (unsigned long long)a.N; n = i - b * (unsigned long long)a.N; }
  else { const uint32_t bi = (uint32_t)i / (uint32_t)a.N; b = bi; n = (uint32_t)i - bi * (uint32_t)a.N; }
  const size_t N = (size_t)a.N;
  const float roi = a.gt_roi[b * N + n];
  float lab;
  if (k == 0) { lab = roi; s.counted = true; }
  else {
    s.counted = roi > 0.5f;
    lab = k <= a.r ? a.gt_x[(b * (size_t)a.gt_bits + (size_t)(k - 1)) * N + n] : a.gt_y[(b * (size_t)a.gt_bits + (size_t)(k - 1 - a.r)) * N + n];
  }
  s.y = lab > 0.5f;
  s.z = a.bits[(size_t)b * (size_t)a.bstride + (size_t)k * N + n];
  return s;
}

// ---- reliability: one record of 3 M + 7 eight-byte words per (workgroup, row):
//      [0, M) count | [M, 2M) positives | [2M, 3M) sum_p | n | n_nan | n_right | nll | brier | g | h
__global__ __launch_bounds__(CAL_THREADS) void calib_reliability_kernel(CalArgs a, CalTable tab, unsigned long long* __restrict__ part) {
  __shared__ double sE[CAL_MAX_BINS];
  __shared__ unsigned long long sC[CAL_WAVES][CAL_MAX_BINS], sP[CAL_WAVES][CAL_MAX_BINS];
  __shared__ double sS[CAL_WAVES][CAL_MAX_BINS];
  __shared__ unsigned long long sN[CAL_WAVES][3];
  __shared__ double sR[CAL_WAVES][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.M, K = 1 + 2 * a.r, W = 3 * M + 7;
  if (tid < M - 1) sE[tid] = tab.edges[tid];
  __syncthreads();
  const unsigned long long i0 = (unsigned long long)blockIdx.x * a.chunk;
  const unsigned long long i1 = i0 + a.chunk < a.total ? i0 + a.chunk : a.total;
  for (int k = 0; k < K; ++k) {
    const double s = tab.scale[k];
    unsigned long long binc = 0, binp = 0, n_nan = 0, n = 0, n_right = 0;      // lane m holds bin m of this wave
    double bins = 0.0, nll = 0.0, brier = 0.0, g = 0.0, h = 0.0;
    for (unsigned long long base = i0; base < i1; base += CAL_THREADS) {
      const unsigned long long i = base + (unsigned)tid;
      const CalSample smp = cal_load(a, i, i < i1, k);
      const bool nan = smp.counted && smp.z != smp.z;
      const bool use = smp.counted && !nan;
      int bin = -1;
      double p = 0.0;
      if (nan) ++n_nan;
      if (use) {
        const CalTerm c = cal_term(smp.z, s, smp.y);
        int lo = 0, hi = M - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (sE[mid] <= c.t) lo = mid + 1; else hi = mid;
        }
        bin = lo; p = c.p;
        ++n; n_right += (smp.z > 0.f) == smp.y ? 1u : 0u; nll = nll + c.nll; brier = brier + c.brier; g = g + c.g; h = h + c.h;
      }
      for (int m = 0; m < M; ++m) {
        const unsigned long long mask = __ballot(bin == m);
        if (!mask) continue;                                        // (wave-uniform)
        const unsigned long long pos = __ballot(bin == m && smp.y);
        const double sp = cal_wave_sum(bin == m ? p : 0.0);
        if (lane == m) { binc += (unsigned long long)__popcll(mask); binp += (unsigned long long)__popcll(pos); bins = bins + sp; }
      }
    }
    n = cal_wave_sum_u64(n); n_nan = cal_wave_sum_u64(n_nan); n_right = cal_wave_sum_u64(n_right);
    nll = cal_wave_sum(nll); brier = cal_wave_sum(brier); g = cal_wave_sum(g); h = cal_wave_sum(h);
    sC[wave][lane] = binc; sP[wave][lane] = binp; sS[wave][lane] = bins;
    if (lane == 0) { sN[wave][0] = n; sN[wave][1] = n_nan; sN[wave][2] = n_right; sR[wave][0] = nll; sR[wave][1] = brier; sR[wave][2] = g; sR[wave][3] = h; }
    __syncthreads();
    unsigned long long* rec = part + ((size_t)blockIdx.x * (size_t)K + (size_t)k) * (size_t)W;
    if (tid < M) {
      rec[tid] = ((sC[0][tid] + sC[1][tid]) + sC[2][tid]) + sC[3][tid];
      rec[M + tid] = ((sP[0][tid] + sP[1][tid]) + sP[2][tid]) + sP[3][tid];
      rec[2 * M + tid] = (unsigned long long)__double_as_longlong(((sS[0][tid] + sS[1][tid]) + sS[2][tid]) + sS[3][tid]);
    } else if (tid < M + 3) {
      const int j = tid - M;
      rec[3 * M + j] = ((sN[0][j] + sN[1][j]) + sN[2][j]) + sN[3][j];
    } else if (tid < M + 7) {
      const int j = tid - M - 3;
      rec[3 * M + 3 + j] = (unsigned long long)__double_as_longlong(((sR[0][j] + sR[1][j]) + sR[2][j]) + sR[3][j]);
    }
    __syncthreads();
  }
}

// the records of the CAL_GRID workgroups added in index order: ints (K, 2M + 3) = [count | positives | n | n_nan | n_right],
// sums (K, M + 4) = [sum_p | nll | brier | g | h]
__global__ __launch_bounds__(CAL_THREADS) void calib_reliability_finish_kernel(const unsigned long long* __restrict__ part, int K, int M,
                                                                               long long* __restrict__ ints, double* __restrict__ sums) {
  const int W = 3 * M + 7;
  for (int e = threadIdx.x; e < K * W; e += CAL_THREADS) {
    const int k = e / W, j = e - k * W;
    const bool is_int = j < 2 * M || (j >= 3 * M && j < 3 * M + 3);
    if (is_int) {
      unsigned long long v = 0;
      for (int w = 0; w < CAL_GRID; ++w) v += part[(size_t)w * (size_t)(K * W) + (size_t)e];
      ints[(size_t)k * (size_t)(2 * M + 3) + (size_t)(j < 2 * M ? j : j - M)] = (long long)v;
    } else {
      double v = 0.0;
      for (int w = 0; w < CAL_GRID; ++w) v = v + __longlong_as_double((long long)part[(size_t)w * (size_t)(K * W) + (size_t)e]);
      sums[(size_t)k * (size_t)(M + 4) + (size_t)(j < 3 * M ? j - 2 * M : j - 2 * M - 3)] = v;
    }
  }
}

// ---- the fit: one record of 4 words per (workgroup, row): n | nll | g | h, at the row's group's current s
__global__ __launch_bounds__(CAL_THREADS) void calib_fit_accum_kernel(CalArgs a, CalTable tab, const double* __restrict__ state,
                                                                      unsigned long long* __restrict__ part) {
  __shared__ unsigned long long sN[CAL_WAVES];
  __shared__ double sR[CAL_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = 1 + 2 * a.r;
  const unsigned long long i0 = (unsigned long long)blockIdx.x * a.chunk;
  const unsigned long long i1 = i0 + a.chunk < a.total ? i0 + a.chunk : a.total;
  for (int k = 0; k < K; ++k) {
    const double* st = state + (size_t)tab.group[k] * CAL_STATE;
    if (st[CS_PHASE] == 2.0) continue;                              // frozen (uniform over the workgroup)
    const double s = st[CS_S];
    unsigned long long n = 0;
    double nll = 0.0, g = 0.0, h = 0.0;
    for (unsigned long long base = i0; base < i1; base += CAL_THREADS) {
      const unsigned long long i = base + (unsigned)tid;
      const CalSample smp = cal_load(a, i, i < i1, k);
      if (smp.counted && smp.z == smp.z) {
        const CalTerm c = cal_term(smp.z, s, smp.y);
        ++n; nll = nll + c.nll; g = g + c.g; h = h + c.h;
      }
    }
    n = cal_wave_sum_u64(n); nll = cal_wave_sum(nll); g = cal_wave_sum(g); h = cal_wave_sum(h);
    if (lane == 0) { sN[wave] = n; sR[wave][0] = nll; sR[wave][1] = g; sR[wave][2] = h; }
    __syncthreads();
    unsigned long long* rec = part + ((size_t)blockIdx.x * (size_t)K + (size_t)k) * 4;
    if (tid == 0) rec[0] = ((sN[0] + sN[1]) + sN[2]) + sN[3];
    else if (tid < 4) rec[tid] = (unsigned long long)__double_as_longlong(((sR[0][tid - 1] + sR[1][tid - 1]) + sR[2][tid - 1]) + sR[3][tid - 1]);
    __syncthreads();
  }
}

struct CalFit { double s_min, s_max, step_tol; int max_iters, K, n_groups; };

__global__ __launch_bounds__(64) void calib_fit_init_kernel(CalFit f, double* __restrict__ state) {
  const int gi = threadIdx.x;
  if (gi >= f.n_groups) return;
  double* st = state + (size_t)gi * CAL_STATE;
  st[CS_S] = 1.0; st[CS_LO] = f.s_min; st[CS_HI] = f.s_max; st[CS_STATUS] = -1.0; st[CS_ITERS] = 0.0; st[CS_NLL0] = 0.0; st[CS_NLL1] = 0.0;
  st[CS_N] = 0.0; st[CS_BEST_S] = 1.0; st[CS_BEST_NLL] = 0.0; st[CS_PHASE] = 0.0; st[CS_PENDING] = 0.0;
}

__global__ __launch_bounds__(64) void calib_fit_step_kernel(CalFit f, CalTable tab, const unsigned long long* __restrict__ part,
                                                            double* __restrict__ state, double* __restrict__ scale_out) {
  __shared__ double sRow[CAL_MAX_ROWS][4];
  const int tid = threadIdx.x;
  if (tid < f.K && state[(size_t)tab.group[tid] * CAL_STATE + CS_PHASE] != 2.0) {
    unsigned long long n = 0;
    double nll = 0.0, g = 0.0, h = 0.0;
    for (int w = 0; w < CAL_GRID; ++w) {
      const unsigned long long* rec = part + ((size_t)w * (size_t)f.K + (size_t)tid) * 4;
      n += rec[0];
      nll = nll + __longlong_as_double((long long)rec[1]);
      g = g + __longlong_as_double((long long)rec[2]);
      h = h + __longlong_as_double((long long)rec[3]);
    }
    sRow[tid][0] = (double)n; sRow[tid][1] = nll; sRow[tid][2] = g; sRow[tid][3] = h;
  }
  __syncthreads();
  if (tid < f.n_groups) {
    double* st = state + (size_t)tid * CAL_STATE;
    const double phase = st[CS_PHASE];
    if (phase != 2.0) {
      double n = 0.0, nll = 0.0, g = 0.0, h = 0.0;
      for (int k = 0; k < f.K; ++k)
        if (tab.group[k] == tid) { n = n + sRow[k][0]; nll = nll + sRow[k][1]; g = g + sRow[k][2]; h = h + sRow[k][3]; }
      const double s = st[CS_S];
      if (phase == 1.0) {
        const double pending = st[CS_PENDING];
        st[CS_NLL1] = nll;
        st[CS_STATUS] = (pending == 1.0 && g < 0.0) ? (double)CP_CALIB_CAPPED_HIGH : (pending == 2.0 && g > 0.0) ? (double)CP_CALIB_CAPPED_LOW : (double)CP_CALIB_OK;
        st[CS_PHASE] = 2.0;
      } else {
        const double iters = st[CS_ITERS] + 1.0;
        st[CS_ITERS] = iters;
        if (iters == 1.0) { st[CS_NLL0] = nll; st[CS_N] = n; st[CS_BEST_S] = s; st[CS_BEST_NLL] = nll; }
        else if (nll < st[CS_BEST_NLL]) { st[CS_BEST_S] = s; st[CS_BEST_NLL] = nll; }
        if (iters == 1.0 && n == 0.0) {
          st[CS_STATUS] = (double)CP_CALIB_EMPTY; st[CS_NLL1] = nll; st[CS_PHASE] = 2.0;
        } else {
          double lo = st[CS_LO], hi = st[CS_HI];
          if (g < 0.0) lo = s; else hi = s;
          st[CS_LO] = lo; st[CS_HI] = hi;
          double c = s - g / h;
          const bool h_ok = h > 0.0 && h <= 1.7976931348623157e308;
          if (!(h_ok && c > lo && c < hi)) c = sqrt(lo * hi);
          if (fabs(c - s) <= f.step_tol * s) {
            double pending = 0.0;
            if (hi == f.s_max && f.s_max - lo <= 3.0 * f.step_tol * f.s_max) { c = f.s_max; pending = 1.0; }
            else if (lo == f.s_min && hi - f.s_min <= 3.0 * f.step_tol * f.s_min) { c = f.s_min; pending = 2.0; }
            st[CS_S] = c; st[CS_PENDING] = pending; st[CS_PHASE] = 1.0;
          } else if (iters >= (double)f.max_iters) {
            st[CS_STATUS] = (double)CP_CALIB_NOT_CONVERGED; st[CS_S] = st[CS_BEST_S]; st[CS_NLL1] = st[CS_BEST_NLL]; st[CS_PHASE] = 2.0;
          } else {
            st[CS_S] = c;
          }
        }
      }
    }
  }
  __syncthreads();
  if (tid < f.K) scale_out[tid] = state[(size_t)tab.group[tid] * CAL_STATE + CS_S];
}

// ---- sigma2 against the true projection: one workgroup per crop
struct PitArgs {
  const float* p2d; const double* proj; const double* sigma2; const uint8_t* valid; int valid_stride; const float* gt_roi;
  int N, E;
  int32_t* counts; int32_t* nn; double* sums;
};

__global__ __launch_bounds__(CAL_THREADS) void calib_pit_kernel(PitArgs a, CalTable tab) {
  __shared__ double sE[CAL_MAX_BINS];
  __shared__ int sCnt[CAL_MAX_BINS];
  __shared__ int sN[CAL_WAVES][2];
  __shared__ double sR[CAL_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t b = blockIdx.x, N = (size_t)a.N;
  if (tid < a.E) sE[tid] = tab.edges[tid];
  if (tid < CAL_MAX_BINS) sCnt[tid] = 0;
  __syncthreads();
  int n = 0, nd = 0;
  double s_d2 = 0.0, s_u = 0.0, s_v = 0.0;
  for (size_t i = (size_t)tid; i < N; i += CAL_THREADS) {
    const size_t q = b * N + i;
    const double vx = a.sigma2[2 * q], vy = a.sigma2[2 * q + 1];
    const bool good = a.valid[q * (size_t)a.valid_stride] != 0 && a.gt_roi[q] > 0.5f && vx > 0.0 && vx <= 1.7976931348623157e308 && vy > 0.0 &&
                      vy <= 1.7976931348623157e308;
    if (!good) { ++nd; continue; }
    const double du = (double)a.p2d[2 * q] - a.proj[2 * q], dv = (double)a.p2d[2 * q + 1] - a.proj[2 * q + 1];
    const double d2 = (du * du) / vx + (dv * dv) / vy;
    int lo = 0, hi = a.E;
    if (d2 == d2) {
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sE[mid] <= d2) lo = mid + 1; else hi = mid;
      }
    }                                                               // (a NaN d2 -- a NaN coordinate -- is below every edge: bin 0)
    atomicAdd(&sCnt[lo], 1);                                        // LDS, integers: the order plays no part
    ++n; s_d2 = s_d2 + d2; s_u = s_u + du / sqrt(vx); s_v = s_v + dv / sqrt(vy);
  }
  for (int d = 32; d >= 1; d >>= 1) { n += __shfl_xor(n, d, 64); nd += __shfl_xor(nd, d, 64); }
  s_d2 = cal_wave_sum(s_d2); s_u = cal_wave_sum(s_u); s_v = cal_wave_sum(s_v);
  if (lane == 0) { sN[wave][0] = n; sN[wave][1] = nd; sR[wave][0] = s_d2; sR[wave][1] = s_u; sR[wave][2] = s_v; }
  __syncthreads();
  if (tid <= a.E) a.counts[b * (size_t)(a.E + 1) + (size_t)tid] = sCnt[tid];
  if (tid < 2) a.nn[2 * b + tid] = ((sN[0][tid] + sN[1][tid]) + sN[2][tid]) + sN[3][tid];
  if (tid < 3) a.sums[3 * b + tid] = ((sR[0][tid] + sR[1][tid]) + sR[2][tid]) + sR[3][tid];
}

inline bool cal_finite_positive(double x) { return x > 0.0 && x <= 1.7976931348623157e308; }
// an edge table: no NaN, strictly ascending (infinities are legal ends)
inline bool cal_edges_bad(const double* e, int n) {
  for (int i = 0; i < n; ++i) {
    if (e[i] != e[i]) return true;
    if (i && !(e[i - 1] < e[i])) return true;
  }
  return false;
}
// the bit-side arguments the two entry points share; -> CP_OK or the refusal
inline int cal_check_bits(const float* bits, long long bstride, int rows, int r, const float* gt_roi, const float* gt_x, const float* gt_y,
                          int gt_bits, int B, int N) {
  if (!bits || !gt_roi || !gt_x || !gt_y) return CP_ERR_INVALID;
  if (B < 0 || N <= 0 || r < 1 || r > 30 || rows < 1 + 2 * r || gt_bits < r || bstride < (long long)rows * (long long)N) return CP_ERR_INVALID;
  if (cp_misaligned(bits, 3) || cp_misaligned(gt_roi, 3) || cp_misaligned(gt_x, 3) || cp_misaligned(gt_y, 3)) return CP_ERR_ALIGN;
  return CP_OK;
}
inline CalArgs cal_args(const float* bits, long long bstride, int r, const float* gt_roi, const float* gt_x, const float* gt_y, int gt_bits,
                        int B, int N, int M) {
  CalArgs a;
  a.bits = bits; a.bstride = bstride; a.gt_roi = gt_roi; a.gt_x = gt_x; a.gt_y = gt_y; a.r = r; a.gt_bits = gt_bits; a.N = N; a.M = M;
  a.total = (unsigned long long)B * (unsigned long long)N;
  a.chunk = (a.total + CAL_GRID - 1) / CAL_GRID;
  return a;
}

}  // namespace

extern "C" size_t cp_code_reliability_scratch_bytes(int r, int M) {
  if (r < 1 || r > 30 || M < 1 || M > CAL_MAX_BINS) return 0;
  return (size_t)CAL_GRID * (size_t)(1 + 2 * r) * (size_t)(3 * M + 7) * 8;
}

extern "C" int cp_code_reliability(cp_stream_t stream, const float* bits, long long bits_bstride, int rows, int r, const float* gt_roi,
                                   const float* gt_x, const float* gt_y, int gt_bits, const double* scale_host, const double* edges_host,
                                   int M, int B, int N, long long* ints, double* sums, void* scratch) {
  const int rc = cal_check_bits(bits, bits_bstride, rows, r, gt_roi, gt_x, gt_y, gt_bits, B, N);
  if (rc == CP_ERR_INVALID) return rc;
  if (!scale_host || !ints || !sums || !scratch || M < 1 || M > CAL_MAX_BINS || (M > 1 && !edges_host)) return CP_ERR_INVALID;
  const int K = 1 + 2 * r;
  for (int k = 0; k < K; ++k)
    if (!cal_finite_positive(scale_host[k])) return CP_ERR_INVALID;
  if (cal_edges_bad(edges_host, M - 1)) return CP_ERR_INVALID;
  if (rc != CP_OK) return rc;
  if (cp_misaligned(ints, 7) || cp_misaligned(sums, 7) || cp_misaligned(scratch, 7)) return CP_ERR_ALIGN;
  if (B == 0) return CP_OK;
  CalTable tab = {};
  for (int k = 0; k < K; ++k) tab.scale[k] = scale_host[k];
  for (int m = 0; m + 1 < M; ++m) tab.edges[m] = edges_host[m];
  const CalArgs a = cal_args(bits, bits_bstride, r, gt_roi, gt_x, gt_y, gt_bits, B, N, M);
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(calib_reliability_kernel, dim3(CAL_GRID), dim3(CAL_THREADS), 0, st, a, tab, (unsigned long long*)scratch);
  CP_LAUNCH(calib_reliability_finish_kernel, dim3(1), dim3(CAL_THREADS), 0, st, (const unsigned long long*)scratch, K, M, ints, sums);
  return cp_check_launch();
}

extern "C" int cp_fit_code_scale_info_doubles(void) { return CAL_STATE; }

extern "C" size_t cp_fit_code_scale_scratch_bytes(int r) {
  if (r < 1 || r > 30) return 0;
  return (size_t)CAL_GRID * (size_t)(1 + 2 * r) * 4 * 8;
}

extern "C" int cp_fit_code_scale(cp_stream_t stream, const float* bits, long long bits_bstride, int rows, int r, const float* gt_roi,
                                 const float* gt_x, const float* gt_y, int gt_bits, const int32_t* group_of_row_host, int n_groups, int B,
                                 int N, double s_min, double s_max, double step_tol, int max_iters, double* scale, double* info,
                                 void* scratch) {
  const int rc = cal_check_bits(bits, bits_bstride, rows, r, gt_roi, gt_x, gt_y, gt_bits, B, N);
  if (rc == CP_ERR_INVALID) return rc;
  const int K = 1 + 2 * r;
  if (!group_of_row_host || !scale || !info || !scratch || n_groups < 1 || n_groups > K) return CP_ERR_INVALID;
  for (int k = 0; k < K; ++k)
    if (group_of_row_host[k] < 0 || group_of_row_host[k] >= n_groups) return CP_ERR_INVALID;
  if (!cal_finite_positive(s_min) || !cal_finite_positive(s_max) || !(s_min <= 1.0) || !(s_max >= 1.0) || !(s_min < s_max)) return CP_ERR_INVALID;
  if (!cal_finite_positive(step_tol) || max_iters < 1 || max_iters > CP_CALIB_MAX_ITERS) return CP_ERR_INVALID;
  if (rc != CP_OK) return rc;
  if (cp_misaligned(scale, 7) || cp_misaligned(info, 7) || cp_misaligned(scratch, 7)) return CP_ERR_ALIGN;
  if (B == 0) return CP_OK;
  CalTable tab = {};
  for (int k = 0; k < K; ++k) tab.group[k] = group_of_row_host[k];
  const CalArgs a = cal_args(bits, bits_bstride, r, gt_roi, gt_x, gt_y, gt_bits, B, N, 1);
  CalFit f;
  f.s_min = s_min; f.s_max = s_max; f.step_tol = step_tol; f.max_iters = max_iters; f.K = K; f.n_groups = n_groups;
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(calib_fit_init_kernel, dim3(1), dim3(64), 0, st, f, info);
  cp_mark_kernel("calib_fit_accum_kernel + calib_fit_step_kernel x%d", max_iters + 1);      // (one entry for the chain)
  for (int it = 0; it <= max_iters; ++it) {
    hipLaunchKernelGGL(calib_fit_accum_kernel, dim3(CAL_GRID), dim3(CAL_THREADS), 0, st, a, tab, (const double*)info, (unsigned long long*)scratch);
    hipLaunchKernelGGL(calib_fit_step_kernel, dim3(1), dim3(64), 0, st, f, tab, (const unsigned long long*)scratch, info, scale);
  }
  return cp_check_launch();
}

extern "C" int cp_sigma2_consistency(cp_stream_t stream, const float* p2d, const double* proj_xy, const double* sigma2, const uint8_t* valid,
                                     int valid_stride, const float* gt_roi, const double* edges_host, int E, int B, int N, int32_t* counts,
                                     int32_t* n_counted_dropped, double* sums) {
  if (!p2d || !proj_xy || !sigma2 || !valid || !gt_roi || !counts || !n_counted_dropped || !sums) return CP_ERR_INVALID;
  if (B < 0 || N <= 0 || valid_stride < 1 || E < 0 || E > CAL_MAX_BINS - 1 || (E > 0 && !edges_host)) return CP_ERR_INVALID;
  if (cal_edges_bad(edges_host, E)) return CP_ERR_INVALID;
  if (cp_misaligned(p2d, 3) || cp_misaligned(gt_roi, 3) || cp_misaligned(counts, 3) || cp_misaligned(n_counted_dropped, 3) ||
      cp_misaligned(proj_xy, 7) || cp_misaligned(sigma2, 7) || cp_misaligned(sums, 7))
    return CP_ERR_ALIGN;
  if (B == 0) return CP_OK;
  CalTable tab = {};
  for (int m = 0; m < E; ++m) tab.edges[m] = edges_host[m];
  PitArgs a;
  a.p2d = p2d; a.proj = proj_xy; a.sigma2 = sigma2; a.valid = valid; a.valid_stride = valid_stride; a.gt_roi = gt_roi; a.N = N; a.E = E;
  a.counts = counts; a.nn = n_counted_dropped; a.sums = sums;
  CP_LAUNCH(calib_pit_kernel, dim3((unsigned)B), dim3(CAL_THREADS), 0, (hipStream_t)stream, a, tab);
  return cp_check_launch();
}
