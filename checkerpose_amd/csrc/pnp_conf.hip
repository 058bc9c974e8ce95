// Confidence-guided pose solver on the device: row N4's EPnP + RANSAC (csrc/pnp.hip) fed with the per-keypoint,
// per-axis pixel variances that cp_code_confidence (csrc/code_confidence.hip, row N32) reads from the code logits.  The correspondences
// are ranked by variance, the 5-point samples are drawn PROSAC-style from a pool that grows down the ranking, and inliers are gated on
// the whitened residual.  The reference neither ranks nor whitens: opt-in, the rule is this project's own (tests/cpnp_stages.py restates
// it in numpy); pnp.hip and pnp_core.h are untouched.
//
// THE RULE.  Inputs per crop: p3d, p2d, valid (one column), cam_K as cp_pnp_ransac, plus sigma2 (B,N,2) fp64 in pixels^2 (x, y).
//   1 ranked set  a valid keypoint is RANKED iff both of its variances are finite and > 0 (cp_finite_positive); the other valid ones are
//                 DROPPED for this call -- never sampled, never inliers -- and counted in n_dropped.  Key s = sigma2_x + sigma2_y (one
//                 fp64 add); order = ascending s, ties by ascending keypoint index: a total order, so `order` is unique.  nv = #ranked.
//   2 pool        PROSAC (Chum & Matas, CVPR 2005): the growth function with T_N = the call's `iterations`, in exact integers.
//                 Hypothesis h (0-based) draws from the first n_h of the ranking, n_h = the smallest n in [5, nv] with
//                 C(n,5) * iterations >= (h + 1) * C(nv,5), C(n,5) = n(n-1)(n-2)(n-3)(n-4)/120 in uint64 (nv = 4096, iterations = 256:
//                 the largest product is 2.5e18 < 2^64).  The last hypothesis draws from everything.  Two deliberate differences from
//                 the paper: there is NO forced n-th member (the paper puts the newest member of the pool into every sample), and NO
//                 T' ceiling recursion (the paper grows T'_n by ceil'd increments along one sequential run): here n_h is a function of
//                 h alone, so the hypotheses are independent and are drawn in parallel.  guided = 0: n_h = nv for every h.
//   3 sample      pnp_core.h's sample_distinct<5>(seed, crop, h, n_h): draw k = hash32(seed, crop, h, try) % n_h, duplicates redrawn;
//                 position r of the ranking -> keypoint order[r].  EPnP on the five points as pnp_hypotheses_kernel runs it.
//   4 gate        d2 = du du / sigma2_x + dv dv / sigma2_y with du, dv as in reproj_sq, fp64 without contraction; a ranked keypoint is
//                 an inlier iff d2 <= chi2_threshold (finite, > 0, no default: 5.99 and 9.21 are the 95 % / 99 % quantiles of chi^2 with
//                 2 degrees of freedom).  count = #inliers among the ranked points.
//   5 the rest    as row N4: rounds of 64 hypotheses, hypotheses_run / needed_iters on the recorded counts (OpenCV's rule assumes
//                 uniform sampling: under guidance, whose early samples are cleaner than uniform ones, it asks for at least as many
//                 hypotheses as needed -- merely conservative); winner = the first record with the largest count >= 5; its whitened
//                 inlier set, in ascending keypoint order, goes through epnp_block_refit unchanged (the refit is UNWEIGHTED; the
//                 weighted polish is row N32's); nv == 4: solve_four_points on the four ranked points in ascending keypoint order, all
//                 four inliers; nv < 4: the identity fallback, status 0.  Hypothesis record: row N4's 14 doubles
//                 [count or -1, n_h, R (9), t (3)] -- the slot row N4 leaves unused carries the pool size, written with every record.
// CONTRACTION.  The rule's own arithmetic (the key's add, the gate: cpnp_d2 carries the pragma) is fp64 without contraction.  The EPnP
// pieces are pnp_core.h's, pinned with contraction on (see its head), and the five-point M^T M below is pnp_hypotheses_kernel's
// statement: with equal variances s and chi2 = thr^2 / s the solver sees row N4's problem.  No atomics anywhere.
//
// THREE kernels:
//   pnp_conf_rank_kernel          one 256-thread workgroup per crop: ranked points flagged and compacted (block_compact), bitonic sort of
//                                 (fp64 key bits, index) pairs in LDS -- positive finite doubles order as their bit patterns -- padded
//                                 with a sentinel to the next power of two (<= 4096: 48 KB) -> order (B,N) int32 (-1 beyond nv),
//                                 n_ranked, n_dropped.  Also behind cp_rank_correspondences.
//   pnp_conf_hypotheses_kernel    pnp_hypotheses_kernel's structure: one launch per round, grid B, one wave per workgroup, a hypothesis
//                                 per lane, M^T M and eigenvectors of 64 lanes in 147 KB of LDS, the staged order (uint16) where vidx
//                                 sat; the pool size per lane by binary search; the scoring loop reads sigma2 from global memory
//                                 (every lane the same point: one line serves the wave).
//   pnp_conf_select_refit_kernel  one 256-thread workgroup per crop: selection, whitened inlier list, epnp_block_refit, P3P, identity.
#include "pnp_core.h"

namespace {

struct ConfParams {
  const float* p3d; const float* p2d; const uint8_t* valid; const float* K; const double* sigma2;
  double* pose; uint8_t* inliers; int32_t* status;
  int32_t* order; int32_t* n_ranked; int32_t* n_dropped;
  long long p3d_bs, K_bs;
  int B, N, valid_stride, iters, round, guided;
  double chi2;
  uint32_t seed;
};

// the whitened squared residual of keypoint k under (R, t): du, dv as in pnp_core.h's reproj_sq
__device__ __forceinline__ double cpnp_d2(const Points& P, const double* R, const double* t, int k, double s2x, double s2y) {
#pragma clang fp contract(off)
  const float* pw = P.p3d + 3 * (size_t)k;
  const double X = R[0] * pw[0] + R[1] * pw[1] + R[2] * pw[2] + t[0], Y = R[3] * pw[0] + R[4] * pw[1] + R[5] * pw[2] + t[1];
  const double iz = 1.0 / (R[6] * pw[0] + R[7] * pw[1] + R[8] * pw[2] + t[2]);
  const double du = P.uc + P.fu * X * iz - P.p2d[2 * (size_t)k], dv = P.vc + P.fv * Y * iz - P.p2d[2 * (size_t)k + 1];
  return du * du / s2x + dv * dv / s2y;
}

__device__ __forceinline__ unsigned long long cpnp_c5(unsigned long long n) {          // C(n,5), n >= 4 (0 at n == 4); exact: the product of 5
  return n * (n - 1) * (n - 2) * (n - 3) * (n - 4) / 120ull;                            // consecutive integers is a multiple of 120
}

// ---------------------------------------------------------------------------------------------- the ranking
constexpr unsigned long long CPNP_SENTINEL = ~0ull;          // above every positive finite double's bit pattern

__global__ __launch_bounds__(PNP_THREADS) void pnp_conf_rank_kernel(const double* __restrict__ sigma2, const uint8_t* __restrict__ valid_all,
                                                                    int valid_stride, int N, int P2, int32_t* __restrict__ order,
                                                                    int32_t* __restrict__ n_ranked, int32_t* __restrict__ n_dropped) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* const key = (unsigned long long*)smem;         // [P2] the key's bits
  int32_t* const idx = (int32_t*)(key + P2);                         // [P2] the keypoint
  __shared__ int wsum[PNP_THREADS / 64], s_drop[PNP_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* s2 = sigma2 + (size_t)b * N * 2;
  const uint8_t* valid = valid_all + (size_t)b * N * valid_stride;
  const int vs = valid_stride;
  int dropped = 0;                                                   // this wave's valid points that are not ranked (the same on its 64 lanes)
  for (int c0 = 0; c0 < N; c0 += PNP_THREADS) {
    const int i = c0 + tid;
    const bool d = i < N && valid[(size_t)i * vs] != 0 && !(cp_finite_positive(s2[2 * (size_t)i]) && cp_finite_positive(s2[2 * (size_t)i + 1]));
    dropped += __popcll(__ballot(d));
  }
  if ((tid & 63) == 0) s_drop[tid >> 6] = dropped;
  const int nv = block_compact<PNP_THREADS>(
      [&](int i) { return valid[(size_t)i * vs] != 0 && cp_finite_positive(s2[2 * (size_t)i]) && cp_finite_positive(s2[2 * (size_t)i + 1]); }, N, idx,
      wsum, tid);
  for (int j = tid; j < P2; j += PNP_THREADS) {
    if (j < nv) {
      const size_t k = (size_t)idx[j];
      key[j] = (unsigned long long)__double_as_longlong(s2[2 * k] + s2[2 * k + 1]);
    } else {
      key[j] = CPNP_SENTINEL;
      idx[j] = 0x7fffffff;
    }
  }
  __syncthreads();
  // bitonic network over P2 (key, index) pairs, ascending in the lexicographic order: every pair is distinct, so the result is unique
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P2; i += PNP_THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long ki = key[i], kl = key[l];
          const int32_t ii = idx[i], il = idx[l];
          const bool gt = ki > kl || (ki == kl && ii > il);
          if (gt == ((i & k) == 0)) { key[i] = kl; key[l] = ki; idx[i] = il; idx[l] = ii; }
        }
      }
      __syncthreads();
    }
  for (int j = tid; j < N; j += PNP_THREADS) order[(size_t)b * N + j] = j < nv ? idx[j] : -1;
  if (tid == 0) {
    n_ranked[b] = nv;
    n_dropped[b] = s_drop[0] + s_drop[1] + s_drop[2] + s_drop[3];
  }
}

// ---------------------------------------------------------------------------------------------- launch per round: the hypotheses
__global__ __launch_bounds__(64) void pnp_conf_hypotheses_kernel(const ConfParams p, double* __restrict__ hyp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* const sA = (double*)smem;                          // [144][64]: M^T M of lane l at [e * 64 + l]
  double* const sV = sA + 144 * 64;                          // [144][64]: its eigenvectors
  uint16_t* const sord = (uint16_t*)(sV + 144 * 64);         // [nv] the ranking: position -> keypoint
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nv = p.n_ranked[b];
  const int h = p.round * 64 + tid;
  if (nv < 5) return;                                        // < 4: identity; exactly 4: P3P in the selection launch, no hypotheses
  if (p.round > 0 && hypotheses_run(hyp + (size_t)b * p.iters * PNP_HYP, nv, 5, p.iters, p.round) <= 64 * p.round)
    return;                                                  // the rule was satisfied by the earlier rounds: whole workgroup, uniform
  const int32_t* ord = p.order + (size_t)b * p.N;
  for (int i = tid; i < nv; i += 64) sord[i] = (uint16_t)ord[i];
  __syncthreads();
  if (h >= p.iters) return;
  const Points P = crop_points(p.p3d + (size_t)b * p.p3d_bs, p.p2d + (size_t)b * p.N * 2, p.K + (size_t)b * p.K_bs);
  const double* s2 = p.sigma2 + (size_t)b * p.N * 2;
  const int m = 5;
  int nh = nv;
  if (p.guided) {                                            // the smallest n in [5, nv] with C(n,5) iterations >= (h + 1) C(nv,5)
    const unsigned long long need = (unsigned long long)(h + 1) * cpnp_c5((unsigned long long)nv), it = (unsigned long long)p.iters;
    int lo = 5, hi = nv;                                     // (hi satisfies it: h + 1 <= iterations)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cpnp_c5((unsigned long long)mid) * it >= need) hi = mid; else lo = mid + 1;
    }
    nh = lo;
  }
  // pnp_core.h's sample_distinct over the first nh positions, mapped through the ranking (a permutation: comparing mapped values is
  // comparing positions), in the form pnp_hypotheses_kernel keeps it
  int32_t sel[5];
  int got = 0;
  uint32_t tries = 0;
  while (got < m) {
    const int r = (int)(hash32(p.seed, (uint32_t)b, (uint32_t)h, tries++) % (uint32_t)nh);
    bool dup = false;
    for (int k = 0; k < got; ++k) dup = dup || sel[k] == (int32_t)sord[r];
    if (!dup) sel[got++] = (int32_t)sord[r];
  }
  Points S = P;
  S.idx = sel; S.n = m;
  Frame f;
  double R[9], t[3];
  bool ok = epnp_frame(S, f);
  if (ok) {
    double* const A = sA + tid;
    for (int i = 0; i < 144; ++i) A[i * 64] = 0.0;
    for (int i = 0; i < m; ++i) {
      double r0[12], r1[12];
      m_rows(S, f, i, r0, r1);
#pragma unroll
      for (int a = 0; a < 12; ++a)
#pragma unroll
        for (int c = a; c < 12; ++c) A[(a * 12 + c) * 64] += r0[a] * r0[c] + r1[a] * r1[c];
    }
    for (int a = 0; a < 12; ++a)
      for (int c = 0; c < a; ++c) A[(a * 12 + c) * 64] = A[(c * 12 + a) * 64];
    ok = epnp_finish(S, f, A, sV + tid, 64, R, t);
  }
  double* rec = hyp + ((size_t)b * p.iters + h) * PNP_HYP;
  int cnt = -1;
  if (ok) {
    cnt = 0;
    for (int i = 0; i < nv; ++i) {
      const int k = (int)sord[i];
      cnt += cpnp_d2(P, R, t, k, s2[2 * (size_t)k], s2[2 * (size_t)k + 1]) <= p.chi2 ? 1 : 0;
    }
    for (int i = 0; i < 9; ++i) rec[2 + i] = R[i];
    for (int i = 0; i < 3; ++i) rec[11 + i] = t[i];
  }
  rec[0] = (double)cnt;
  rec[1] = (double)nh;
}

// ---------------------------------------------------------------------------------------------- last launch: selection + final EPnP
__global__ __launch_bounds__(PNP_THREADS) void pnp_conf_select_refit_kernel(const ConfParams p, const double* __restrict__ hyp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* const s3 = (float*)smem;
  float* const s2 = s3 + 3 * p.N;
  int32_t* const vidx = (int32_t*)(s2 + 2 * p.N);            // the ranked points, ascending keypoint index
  int32_t* const iidx = vidx + p.N;                          // the winner's inliers, ascending
  bool* const flag = (bool*)(iidx + p.N);
  __shared__ EpnpRefitLds rl;
  __shared__ int wsum[PNP_THREADS / 64], s_best;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* g3 = p.p3d + (size_t)b * p.p3d_bs;
  const float* g2 = p.p2d + (size_t)b * p.N * 2;
  const double* sg = p.sigma2 + (size_t)b * p.N * 2;
  const int32_t* ord = p.order + (size_t)b * p.N;
  const int nr = p.n_ranked[b];
  for (int i = tid; i < 3 * p.N; i += PNP_THREADS) s3[i] = g3[i];
  for (int i = tid; i < 2 * p.N; i += PNP_THREADS) s2[i] = g2[i];
  for (int i = tid; i < p.N; i += PNP_THREADS) { flag[i] = false; p.inliers[(size_t)b * p.N + i] = 0; }
  __syncthreads();
  for (int i = tid; i < nr; i += PNP_THREADS) flag[ord[i]] = true;
  __syncthreads();
  const int nv = block_compact<PNP_THREADS>([&](int i) { return flag[i]; }, p.N, vidx, wsum, tid);
  double* pose = p.pose + (size_t)b * 12;
  auto identity = [&]() {                                    // the reference's fallback: identity pose, no inliers
    if (tid == 0) {
      write_identity_pose(pose);
      p.status[b] = 0;
    }
  };
  if (nv < 4) { identity(); return; }
  const int m = 5;
  const Points P = crop_points(s3, s2, p.K + (size_t)b * p.K_bs);
  if (nv == 4) {                                             // as row N4: no RANSAC, P3P + the fourth point; all four are inliers
    if (tid == 0) {
      float pw4[12], uv4[8];
      for (int i = 0; i < 4; ++i) {
        const int k = vidx[i];
        for (int c = 0; c < 3; ++c) pw4[3 * i + c] = s3[3 * k + c];
        uv4[2 * i] = s2[2 * k]; uv4[2 * i + 1] = s2[2 * k + 1];
      }
      double R4[9], t4[3];
      if (solve_four_points(pw4, uv4, P.fu, P.fv, P.uc, P.vc, R4, t4)) {
        for (int i = 0; i < 9; ++i) pose[i] = R4[i];
        for (int i = 0; i < 3; ++i) pose[9 + i] = t4[i];
        for (int i = 0; i < 4; ++i) p.inliers[(size_t)b * p.N + vidx[i]] = 1;
        p.status[b] = 1;
      } else {
        write_identity_pose(pose);
        p.status[b] = 0;
      }
    }
    return;
  }
  const double* hb = hyp + (size_t)b * p.iters * PNP_HYP;
  if (tid == 0) {                                            // most inliers, first on ties, at least a full sample
    int best = -1, bc = m - 1;
    const int nrun = hypotheses_run(hb, nv, m, p.iters, PNP_MAX_ITERS / 64);
    for (int h = 0; h < nrun; ++h) {
      const int c = (int)hb[(size_t)h * PNP_HYP];
      if (c > bc) { bc = c; best = h; }
    }
    s_best = best;
  }
  __syncthreads();
  const int best = s_best;
  if (best < 0) { identity(); return; }
  double Rb[9], tb[3];
  for (int i = 0; i < 9; ++i) Rb[i] = hb[(size_t)best * PNP_HYP + 2 + i];
  for (int i = 0; i < 3; ++i) tb[i] = hb[(size_t)best * PNP_HYP + 11 + i];
  __syncthreads();
  for (int i = tid; i < p.N; i += PNP_THREADS) flag[i] = false;
  __syncthreads();
  for (int i = tid; i < nv; i += PNP_THREADS) {
    const int k = vidx[i];
    const bool in = cpnp_d2(P, Rb, tb, k, sg[2 * (size_t)k], sg[2 * (size_t)k + 1]) <= p.chi2;
    flag[k] = in;
    if (in) p.inliers[(size_t)b * p.N + k] = 1;
  }
  __syncthreads();
  const int n = block_compact<PNP_THREADS>([&](int i) { return flag[i]; }, p.N, iidx, wsum, tid);
  Points S = P;
  S.idx = iidx; S.n = n;
  const bool ok = epnp_block_refit(S, rl, tid);
  if (tid == 0) {
    if (ok) {
      for (int i = 0; i < 12; ++i) pose[i] = rl.pose[i];
    } else {                                                 // degenerate inlier set: keep the winning hypothesis
      for (int i = 0; i < 9; ++i) pose[i] = Rb[i];
      for (int i = 0; i < 3; ++i) pose[9 + i] = tb[i];
    }
    p.status[b] = 1;
  }
}

int cpnp_pow2_at_least(int n) {
  int p2 = 2;
  while (p2 < n) p2 <<= 1;
  return p2;
}

void cpnp_launch_rank(hipStream_t st, const double* sigma2, const uint8_t* valid, int valid_stride, int B, int N, int32_t* order,
                      int32_t* n_ranked, int32_t* n_dropped) {
  const int P2 = cpnp_pow2_at_least(N);                      // <= 4096: 12 bytes per pair, <= 48 KB
  CP_LAUNCH(pnp_conf_rank_kernel, dim3((unsigned)B), dim3(PNP_THREADS), (size_t)P2 * 12, st, sigma2, valid, valid_stride, N, P2, order, n_ranked,
            n_dropped);
}

}  // namespace

extern "C" int cp_rank_correspondences(cp_stream_t stream, const double* sigma2, const uint8_t* valid, int valid_stride, int B, int N,
                                       int32_t* order, int32_t* n_ranked, int32_t* n_dropped) {
  if (!sigma2 || !valid || !order || !n_ranked || !n_dropped) return CP_ERR_INVALID;
  if (B < 0 || N <= 0 || N > PNP_NMAX || valid_stride <= 0) return CP_ERR_INVALID;
  if (cp_misaligned(sigma2, 7) || cp_misaligned(order, 3) || cp_misaligned(n_ranked, 3) || cp_misaligned(n_dropped, 3)) return CP_ERR_ALIGN;
  if (B == 0) return CP_OK;
  cpnp_launch_rank((hipStream_t)stream, sigma2, valid, valid_stride, B, N, order, n_ranked, n_dropped);
  return cp_check_launch();
}

extern "C" size_t cp_pnp_conf_scratch_bytes(int B, int N) { (void)N; return (size_t)(B > 0 ? B : 0) * PNP_MAX_ITERS * PNP_HYP * sizeof(double); }

extern "C" int cp_pnp_conf(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* valid, int valid_stride,
                           const double* sigma2, const float* cam_K, long long K_bstride, int B, int N, double chi2_threshold, int iterations,
                           uint32_t seed, int guided, double* pose, uint8_t* inliers, int32_t* status, int32_t* order, int32_t* n_ranked,
                           int32_t* n_dropped, void* scratch) {
  if (!p3d || !p2d || !valid || !sigma2 || !cam_K || !pose || !inliers || !status || !order || !n_ranked || !n_dropped || !scratch)
    return CP_ERR_INVALID;
  if (B <= 0 || N <= 0 || N > PNP_NMAX || valid_stride <= 0 || iterations <= 0 || iterations > PNP_MAX_ITERS) return CP_ERR_INVALID;
  if (!cp_finite_positive(chi2_threshold)) return CP_ERR_INVALID;
  if (cp_p3d_stride_invalid(p3d_bstride, N) || cp_K_stride_invalid(K_bstride)) return CP_ERR_INVALID;
  if (cp_misaligned(pose, 7) || cp_misaligned(scratch, 7) || cp_misaligned(sigma2, 7) || cp_misaligned(status, 3) || cp_misaligned(order, 3) ||
      cp_misaligned(n_ranked, 3) || cp_misaligned(n_dropped, 3))
    return CP_ERR_ALIGN;
  ConfParams p;
  p.p3d = p3d; p.p2d = p2d; p.valid = valid; p.K = cam_K; p.sigma2 = sigma2; p.pose = pose; p.inliers = inliers; p.status = status;
  p.order = order; p.n_ranked = n_ranked; p.n_dropped = n_dropped;
  p.p3d_bs = p3d_bstride; p.K_bs = K_bstride; p.B = B; p.N = N; p.valid_stride = valid_stride; p.iters = iterations; p.round = 0;
  p.guided = guided ? 1 : 0; p.chi2 = chi2_threshold; p.seed = seed;
  const size_t lds1 = (size_t)2 * 144 * 64 * 8 + (size_t)N * 2 + 16, lds2 = (size_t)N * (5 * 4 + 8 + 1) + 16;
  static CpDeviceOnce once;                  // both kernels are sized for PNP_NMAX keypoints, once per device
  const int dev = cp_current_device();
  CP_LDS_ATTR_ONCE(once, dev, cp_set_max_lds((const void*)pnp_conf_hypotheses_kernel, (size_t)2 * 144 * 64 * 8 + PNP_NMAX * 2 + 16) &&
                                  cp_set_max_lds((const void*)pnp_conf_select_refit_kernel, (size_t)PNP_NMAX * 29 + 16));
  hipStream_t st = (hipStream_t)stream;
  cpnp_launch_rank(st, sigma2, valid, valid_stride, B, N, order, n_ranked, n_dropped);
  for (int r = 0; 64 * r < iterations; ++r) {
    p.round = r;
    CP_LAUNCH(pnp_conf_hypotheses_kernel, dim3((unsigned)B), dim3(64), lds1, st, p, (double*)scratch);
  }
  p.round = 0;
  CP_LAUNCH(pnp_conf_select_refit_kernel, dim3((unsigned)B), dim3(PNP_THREADS), lds2, st, p, (const double*)scratch);
  return cp_check_launch();
}
