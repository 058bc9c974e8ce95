// Levenberg-Marquardt polish of solved poses on the device: the non-linear refinement a user of a
// correspondence-based estimator gets from cv2.solvePnPRefineLM / SOLVEPNP_ITERATIVE, over the inlier set of cp_pnp_ransac (row N4)
// or cp_pnp_gc (row N17), so that still only 12 doubles per crop leave the GPU.  The reference does not refine: the row is opt-in,
// and its rule is this project's own (tests/lm_stages.py restates it in numpy; parity with cv2 is UNPINNED).
//
// THE RULE.  Per crop: S = {k : mask[k] != 0}, n = |S|; model points X_k and pixels p_k (fp32), fu, fv, uc, vc = K[0], K[4], K[2],
// K[5]; the input pose (R, t) in fp64.  Everything in fp64, no contraction.
//   residual   Y_k = R X_k, C_k = Y_k + t, r_k = (fu C_x / C_z + uc - p_x, fv C_y / C_z + vc - p_y); cost c = sum_k |r_k|^2
//   increment  d = (w, v): R' = exp([w]x) R (Rodrigues), t' = t + v
//   Jacobian   J_k = P_k [ -[Y_k]x | I ], P_k = [[fu / C_z, 0, -fu C_x / C_z^2], [0, fv / C_z, -fv C_y / C_z^2]]
//              H = sum J^T J, g = sum J^T r   (every quotient by C_z is a product with 1 / C_z: lm_accumulate is the operation order)
//   iteration  lambda = 1e-3; at most max_iters (1..64) times:
//              1. solve (H + lambda diag(H)) d = -g by Cholesky (one thread);
//              2. not positive definite: the trial is rejected with c' = +inf (d, the trial pose and s are recorded as NaN);
//              3. else (R', t') and c'; c' = +inf if a selected point has C'_z <= 0 or c' is not finite;
//              4. accept iff c' < c: the trial pose becomes the state with its H, g, c, lambda = max(lambda / 10, 1e-12);
//                 else lambda = lambda * 10;
//              5. s = max(|w|_inf, |v|_inf / |t|), t from before the step.
//   stopping   s <= step_tol (accepted or not): status 1; lambda > 1e8 after a rejection: status 3; iterations run out: status 2.
//   pass-through (status 0, the output pose is BITWISE the input pose): status_in[b] == 0; n < 6; a non-finite input pose or selected
//              pixel; a selected point with C_z <= 0 (or not comparable) under the input pose.  info then holds NaN but for n.
//   records    17 doubles per executed iteration: [lambda used, c, c', accepted 0/1, s, R' (9), t' (3)]; other slots are not written.
//   returned   bitwise the last accepted trial pose, or the input pose when nothing was accepted.
//
// ONE launch, one 256-thread workgroup per crop.  The selected indices are compacted once (block_compact); the points are read
// from global memory through them (20 bytes per point: after the first pass they sit in L2).  A thread accumulates the 21 + 6 + 1
// sums (upper triangle of H, g, c) over its points i = tid, tid + 256, ... in ascending order; the 256 partial sums meet in
// pnp_core.h's block_sum (shuffle tree inside a wave, then wave 0 + 1 + 2 + 3): a fixed order, no atomics.  Thread 0 damps H, does the
// 6 x 6 Cholesky and Rodrigues (pnp_core.h's lm_solve_step) and publishes the trial pose through LDS; all threads then evaluate the
// trial's sums in ONE pass (H', g' and c' together: an accepted trial needs no second pass, a rejected one wasted 27 multiply-adds per
// point) and a second block_sum.
// Every branch on accept / stop is taken on values every thread holds identically (LDS words or block_sum results): uniform over
// the workgroup.  Every loop is bounded by max_iters; no workgroup waits for another.
#include "pnp_core.h"

#pragma clang fp contract(off)

namespace {

constexpr int LM_REC = 17, LM_INFO = 40, LM_MAX_ITERS = 64, LM_SUMS = 29;      // sums: H (21), g (6), c, #points not in front

struct LmParams {
  const float* p3d; const float* p2d; const uint8_t* mask; const float* K;
  const double* pose_in; const int32_t* status_in;
  double* pose_out; int32_t* status_out; double* info; double* records;
  long long p3d_bs, K_bs;
  int B, N, mask_stride, max_iters;
  double step_tol;
};

// the sums of one thread's points under the pose (R, t): acc[0..20] upper triangle of H row by row, [21..26] g, [27] c, [28] the
// number of points with !(C_z > 0)
__device__ __forceinline__ void lm_accumulate(const float* __restrict__ g3, const float* __restrict__ g2, const int32_t* vidx, int n, int tid,
                                              const double* R, const double* t, double fu, double fv, double uc, double vc, double* acc) {
#pragma unroll
  for (int k = 0; k < LM_SUMS; ++k) acc[k] = 0.0;
  for (int i = tid; i < n; i += PNP_THREADS) {
    const size_t k = (size_t)vidx[i];
    const double X0 = g3[3 * k], X1 = g3[3 * k + 1], X2 = g3[3 * k + 2];
    const double px = g2[2 * k], py = g2[2 * k + 1];
    const double Y0 = R[0] * X0 + R[1] * X1 + R[2] * X2, Y1 = R[3] * X0 + R[4] * X1 + R[5] * X2, Y2 = R[6] * X0 + R[7] * X1 + R[8] * X2;
    const double C0 = Y0 + t[0], C1 = Y1 + t[1], C2 = Y2 + t[2];
    if (!(C2 > 0.0)) acc[28] += 1.0;
    const double iz = 1.0 / C2;
    const double r0 = fu * C0 * iz + uc - px, r1 = fv * C1 * iz + vc - py;
    const double a = fu * iz, b = fv * iz;
    const double pu = -(a * C0 * iz), pv = -(b * C1 * iz);
    const double J0[6] = {pu * Y1, a * Y2 - pu * Y0, -(a * Y1), a, 0.0, pu};
    const double J1[6] = {pv * Y1 - b * Y2, -(pv * Y0), b * Y0, 0.0, b, pv};
    int e = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
      for (int q = p; q < 6; ++q) { acc[e] += J0[p] * J0[q] + J1[p] * J1[q]; ++e; }
#pragma unroll
    for (int p = 0; p < 6; ++p) acc[21 + p] += J0[p] * r0 + J1[p] * r1;
    acc[27] += r0 * r0 + r1 * r1;
  }
}

__global__ __launch_bounds__(PNP_THREADS) void pnp_refine_lm_kernel(const LmParams p) {
  __shared__ int32_t vidx[PNP_NMAX];
  __shared__ double sred[4 * LM_SUMS];
  __shared__ double s_H[28];                                                  // the state's H (21), g (6), c: written and read by thread 0
  __shared__ double s_L[6][6], s_y[6], s_d[6], s_trial[19];
  __shared__ int wsum[PNP_THREADS / 64], s_pd;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* g3 = p.p3d + (size_t)b * p.p3d_bs;
  const float* g2 = p.p2d + (size_t)b * p.N * 2;
  const uint8_t* mask = p.mask + (size_t)b * p.N * p.mask_stride;
  const int ms = p.mask_stride;
  const int n = block_compact<PNP_THREADS>([&](int i) { return mask[(size_t)i * ms] != 0; }, p.N, vidx, wsum, tid);
  const float* K = p.K + (size_t)b * p.K_bs;
  const double fu = K[0], fv = K[4], uc = K[2], vc = K[5];
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = p.pose_in[(size_t)b * 12 + i];
  for (int i = 0; i < 3; ++i) t[i] = p.pose_in[(size_t)b * 12 + 9 + i];
  double* const pose_out = p.pose_out + (size_t)b * 12;
  double* const info = p.info + (size_t)b * LM_INFO;
  bool pass = (p.status_in && p.status_in[b] == 0) || n < 6;                  // every thread reads the same words: uniform
  for (int i = 0; i < 9; ++i) pass = pass || !isfinite(R[i]);
  for (int i = 0; i < 3; ++i) pass = pass || !isfinite(t[i]);
  double c = 0.0, c0 = 0.0, lambda = 1e-3;
  int status = 2, iters = 0;
  // it == -1: the sums at the input pose (the "trial" is the input pose itself); it >= 0: the iterations.  One loop, so that the
  // accumulation exists once in the code
  for (int it = -1; it < p.max_iters && !pass; ++it) {
    double Rn[9], tn[3], s = 0.0, bad = 0.0;
    bool pd = true;
    if (it < 0) {
      for (int i = 0; i < 9; ++i) Rn[i] = R[i];
      for (int i = 0; i < 3; ++i) tn[i] = t[i];
      for (int i = tid; i < n; i += PNP_THREADS) {
        const size_t k = (size_t)vidx[i];
        if (!isfinite(g2[2 * k]) || !isfinite(g2[2 * k + 1])) bad += 1.0;
      }
    } else {
      if (tid == 0) {                                                         // (H + lambda diag H) d = -g, then the trial pose
        lm_load_lower(s_H, s_L);
        for (int q = 0; q < 6; ++q) s_L[q][q] = s_L[q][q] + lambda * s_L[q][q];
        s_pd = lm_solve_step(s_L, s_H + 21, R, t, s_y, s_d, s_trial) ? 1 : 0;
      }
      __syncthreads();
      pd = s_pd != 0;
      for (int i = 0; i < 9; ++i) Rn[i] = s_trial[6 + i];
      for (int i = 0; i < 3; ++i) tn[i] = s_trial[15 + i];
      s = s_trial[18];
    }
    double acc[LM_SUMS];
    double cn = INFINITY;
    if (pd) {
      lm_accumulate(g3, g2, vidx, n, tid, Rn, tn, fu, fv, uc, vc, acc);
      acc[28] += bad;
      block_sum<LM_SUMS>(acc, sred, tid);                                     // (its barriers also fence s_trial and s_pd against the next trial)
      if (acc[28] == 0.0 && isfinite(acc[27])) cn = acc[27];
    } else {
      __syncthreads();
    }
    if (it < 0) {
      if (acc[28] != 0.0) { pass = true; break; }                             // a pixel that is not finite, a point not in front of the camera
      c = c0 = acc[27];                                                       // (not `cn`: a cost that is not finite is still the state's cost)
      if (tid == 0)
        for (int i = 0; i < 28; ++i) s_H[i] = acc[i];
      continue;
    }
    const bool accept = cn < c;
    if (p.records && tid == 0) {
      double* rec = p.records + ((size_t)b * p.max_iters + it) * LM_REC;
      rec[0] = lambda; rec[1] = c; rec[2] = cn; rec[3] = accept ? 1.0 : 0.0; rec[4] = s;
      for (int i = 0; i < 9; ++i) rec[5 + i] = Rn[i];
      for (int i = 0; i < 3; ++i) rec[14 + i] = tn[i];
    }
    if (accept) {
      for (int i = 0; i < 9; ++i) R[i] = Rn[i];
      for (int i = 0; i < 3; ++i) t[i] = tn[i];
      c = cn;
      if (tid == 0)
        for (int i = 0; i < 28; ++i) s_H[i] = acc[i];
      lambda = fmax(lambda / 10.0, 1e-12);
    } else {
      lambda = lambda * 10.0;
    }
    iters = it + 1;
    if (s <= p.step_tol) { status = 1; break; }
    if (!accept && lambda > 1e8) { status = 3; break; }
  }
  if (tid != 0) return;
  for (int i = 0; i < 9; ++i) pose_out[i] = R[i];                             // pass-through: R, t still hold the input's bits
  for (int i = 0; i < 3; ++i) pose_out[9 + i] = t[i];
  if (pass) {
    p.status_out[b] = 0;
    for (int i = 0; i < LM_INFO; ++i) info[i] = NAN;
    info[2] = (double)n;
    info[3] = 0.0;
    return;
  }
  p.status_out[b] = status;
  info[0] = c0; info[1] = c; info[2] = (double)n; info[3] = (double)iters;
  int e = 0;
  for (int a = 0; a < 6; ++a)
    for (int q = a; q < 6; ++q) { info[4 + 6 * a + q] = s_H[e]; info[4 + 6 * q + a] = s_H[e]; ++e; }
}

}  // namespace

extern "C" int cp_pnp_refine_lm_record_doubles(void) { return LM_REC; }
extern "C" int cp_pnp_refine_lm_info_doubles(void) { return LM_INFO; }

extern "C" int cp_pnp_refine_lm(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* mask,
                                int mask_stride, const float* cam_K, long long K_bstride, int B, int N, const double* pose_in,
                                const int32_t* status_in, int max_iters, double step_tol, double* pose_out, int32_t* status_out,
                                double* info, double* records) {
  if (!p3d || !p2d || !mask || !cam_K || !pose_in || !pose_out || !status_out || !info) return CP_ERR_INVALID;
  if (B < 0 || N <= 0 || N > PNP_NMAX || mask_stride <= 0 || max_iters < 1 || max_iters > LM_MAX_ITERS) return CP_ERR_INVALID;
  if (!cp_finite_positive(step_tol) || cp_p3d_stride_invalid(p3d_bstride, N) || cp_K_stride_invalid(K_bstride)) return CP_ERR_INVALID;
  if (cp_misaligned(pose_in, 7) || cp_misaligned(pose_out, 7) || cp_misaligned(info, 7) || cp_misaligned(records, 7) ||
      cp_misaligned(status_out, 3) || cp_misaligned(status_in, 3))
    return CP_ERR_ALIGN;
  if (cp_pose_alias_invalid(pose_in, pose_out, B)) return CP_ERR_INVALID;
  if (B == 0) return CP_OK;
  LmParams p;
  p.p3d = p3d; p.p2d = p2d; p.mask = mask; p.K = cam_K; p.pose_in = pose_in; p.status_in = status_in;
  p.pose_out = pose_out; p.status_out = status_out; p.info = info; p.records = records;
  p.p3d_bs = p3d_bstride; p.K_bs = K_bstride; p.B = B; p.N = N; p.mask_stride = mask_stride; p.max_iters = max_iters; p.step_tol = step_tol;
  CP_LAUNCH(pnp_refine_lm_kernel, dim3((unsigned)B), dim3(PNP_THREADS), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}
