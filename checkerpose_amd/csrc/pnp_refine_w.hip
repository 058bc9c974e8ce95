// Weighted robust Levenberg-Marquardt polish of solved poses on the device: row N22 (csrc/pnp_refine.hip) with
// a per-point, per-axis scale 1 / sigma on the residuals -- cp_code_confidence's (csrc/code_confidence.hip) reading of how sure the
// network was of each keypoint's code -- and a Huber loss, so that the fit can run over every valid correspondence, not only over the
// set a 2-px RANSAC threshold left.  The reference does not refine: opt-in, the rule is this project's own (tests/wlm_stages.py restates
// it in numpy).
//
// THE RULE is row N22's (the top of csrc/pnp_refine.hip: residual r_k, increment d = (w, v), Jacobian rows J_{k,0}, J_{k,1}, damping,
// accept rule, lambda schedule, s, stopping rule, statuses 1 / 2 / 3, the 17-double record, the returned pose bitwise the last accepted
// trial, fp64 without contraction, thread i accumulating points i, i + 256, ... in ascending order, then block_sum) with three changes:
//   scale     (B, N, 2) fp32, 1 / sigma per axis: whitened components u_{k,a} = scale_{k,a} r_{k,a}, their Jacobian rows
//             j_{k,a} = scale_{k,a} J_{k,a}.  The scale meets r and the six row entries BEFORE any product: a scale of exactly 1
//             changes no operand.
//   Huber     delta > 0 (+inf allowed) in whitened units, per scalar component: rho(u) = u^2 if |u| <= delta, else
//             2 delta |u| - delta^2; cost c = sum_{k,a} rho(u_{k,a}); omega = 1 if |u| <= delta, else delta / |u|;
//             H = sum omega j j^T (entry (p, q), p <= q: (omega_0 j_0[p]) j_0[q] + (omega_1 j_1[p]) j_1[q]),
//             g = sum (omega_0 j_0[p]) u_0 + (omega_1 j_1[p]) u_1: exactly half the gradient of c.  Accept iff c' < c on this cost.
//   pass-through (status 0, the output pose BITWISE the input pose) under row N22's conditions, plus: a selected point whose scale is
//             not finite or is <= 0 on either axis.
//   info      42 doubles: row N22's 40 (c at the input pose, c at the returned pose, n, iterations, H at the returned pose: the
//             whitened, omega-weighted matrix, so that its inverse IS the first-order covariance), then the number of components
//             with |u| > delta at the input pose, then at the returned pose.  Pass-through: NaN but for n and 0 iterations.
//
// ONE launch, one 256-thread workgroup per crop, N <= 4096; the launch structure is pnp_refine.hip's, statement by statement: indices
// compacted once (block_compact), 30 sums per thread (H 21, g 6, c, points not usable, components beyond delta) joined by block_sum in
// a fixed order, lm_load_lower / lm_solve_step on thread 0, the trial's sums in one pass.  No atomics, no scratch.  Every branch on
// accept / stop is taken on values every thread holds identically; every loop is bounded by max_iters.
#include "pnp_core.h"

#pragma clang fp contract(off)

namespace {

constexpr int WLM_REC = 17, WLM_INFO = 42, WLM_MAX_ITERS = 64, WLM_SUMS = 30;  // sums: H (21), g (6), c, #points not in front, #|u| > delta

struct WlmParams {
  const float* p3d; const float* p2d; const uint8_t* mask; const float* scale; const float* K;
  const double* pose_in; const int32_t* status_in;
  double* pose_out; int32_t* status_out; double* info; double* records;
  long long p3d_bs, K_bs;
  int B, N, mask_stride, max_iters;
  double step_tol, delta;
};

// the sums of one thread's points under the pose (R, t): acc[0..20] upper triangle of H row by row, [21..26] g, [27] c, [28] the
// number of points with !(C_z > 0), [29] the number of components with |u| > delta
__device__ __forceinline__ void wlm_accumulate(const float* __restrict__ g3, const float* __restrict__ g2, const float* __restrict__ gs,
                                               const int32_t* vidx, int n, int tid, const double* R, const double* t, double fu, double fv,
                                               double uc, double vc, double delta, double* acc) {
#pragma unroll
  for (int k = 0; k < WLM_SUMS; ++k) acc[k] = 0.0;
  for (int i = tid; i < n; i += PNP_THREADS) {
    const size_t k = (size_t)vidx[i];
    const double X0 = g3[3 * k], X1 = g3[3 * k + 1], X2 = g3[3 * k + 2];
    const double px = g2[2 * k], py = g2[2 * k + 1];
    const double s0 = gs[2 * k], s1 = gs[2 * k + 1];
    const double Y0 = R[0] * X0 + R[1] * X1 + R[2] * X2, Y1 = R[3] * X0 + R[4] * X1 + R[5] * X2, Y2 = R[6] * X0 + R[7] * X1 + R[8] * X2;
    const double C0 = Y0 + t[0], C1 = Y1 + t[1], C2 = Y2 + t[2];
    if (!(C2 > 0.0)) acc[28] += 1.0;
    const double iz = 1.0 / C2;
    const double r0 = fu * C0 * iz + uc - px, r1 = fv * C1 * iz + vc - py;
    const double a = fu * iz, b = fv * iz;
    const double pu = -(a * C0 * iz), pv = -(b * C1 * iz);
    const double J0[6] = {pu * Y1, a * Y2 - pu * Y0, -(a * Y1), a, 0.0, pu};
    const double J1[6] = {pv * Y1 - b * Y2, -(pv * Y0), b * Y0, 0.0, b, pv};
    const double u0 = s0 * r0, u1 = s1 * r1;                                  // the scale first: 1 changes no operand
    double j0[6], j1[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) { j0[p] = s0 * J0[p]; j1[p] = s1 * J1[p]; }
    const double a0 = fabs(u0), a1 = fabs(u1);
    const bool k0 = a0 > delta, k1 = a1 > delta;                              // (NaN and delta = +inf: not clipped)
    const double w0 = k0 ? delta / a0 : 1.0, w1 = k1 ? delta / a1 : 1.0;
    const double rho0 = k0 ? 2.0 * delta * a0 - delta * delta : u0 * u0, rho1 = k1 ? 2.0 * delta * a1 - delta * delta : u1 * u1;
    double m0[6], m1[6];
#pragma unroll
    for (int p = 0; p < 6; ++p) { m0[p] = w0 * j0[p]; m1[p] = w1 * j1[p]; }
    int e = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
      for (int q = p; q < 6; ++q) { acc[e] += m0[p] * j0[q] + m1[p] * j1[q]; ++e; }
#pragma unroll
    for (int p = 0; p < 6; ++p) acc[21 + p] += m0[p] * u0 + m1[p] * u1;
    acc[27] += rho0 + rho1;
    acc[29] += (k0 ? 1.0 : 0.0) + (k1 ? 1.0 : 0.0);
  }
}

__global__ __launch_bounds__(PNP_THREADS) void pnp_refine_wlm_kernel(const WlmParams p) {
  __shared__ int32_t vidx[PNP_NMAX];
  __shared__ double sred[4 * WLM_SUMS];
  __shared__ double s_H[28];                                                  // the state's H (21), g (6), c: written and read by thread 0
  __shared__ double s_L[6][6], s_y[6], s_d[6], s_trial[19];
  __shared__ int wsum[PNP_THREADS / 64], s_pd;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* g3 = p.p3d + (size_t)b * p.p3d_bs;
  const float* g2 = p.p2d + (size_t)b * p.N * 2;
  const float* gs = p.scale + (size_t)b * p.N * 2;
  const uint8_t* mask = p.mask + (size_t)b * p.N * p.mask_stride;
  const int ms = p.mask_stride;
  const int n = block_compact<PNP_THREADS>([&](int i) { return mask[(size_t)i * ms] != 0; }, p.N, vidx, wsum, tid);
  const float* K = p.K + (size_t)b * p.K_bs;
  const double fu = K[0], fv = K[4], uc = K[2], vc = K[5];
  const double delta = p.delta;
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = p.pose_in[(size_t)b * 12 + i];
  for (int i = 0; i < 3; ++i) t[i] = p.pose_in[(size_t)b * 12 + 9 + i];
  double* const pose_out = p.pose_out + (size_t)b * 12;
  double* const info = p.info + (size_t)b * WLM_INFO;
  bool pass = (p.status_in && p.status_in[b] == 0) || n < 6;                  // every thread reads the same words: uniform
  for (int i = 0; i < 9; ++i) pass = pass || !isfinite(R[i]);
  for (int i = 0; i < 3; ++i) pass = pass || !isfinite(t[i]);
  double c = 0.0, c0 = 0.0, lambda = 1e-3, clip = 0.0, clip0 = 0.0;
  int status = 2, iters = 0;
  // it == -1: the sums at the input pose (the "trial" is the input pose itself); it >= 0: the iterations
  for (int it = -1; it < p.max_iters && !pass; ++it) {
    double Rn[9], tn[3], s = 0.0, bad = 0.0;
    bool pd = true;
    if (it < 0) {
      for (int i = 0; i < 9; ++i) Rn[i] = R[i];
      for (int i = 0; i < 3; ++i) tn[i] = t[i];
      for (int i = tid; i < n; i += PNP_THREADS) {
        const size_t k = (size_t)vidx[i];
        const float s0 = gs[2 * k], s1 = gs[2 * k + 1];
        if (!isfinite(g2[2 * k]) || !isfinite(g2[2 * k + 1]) || !(s0 > 0.f) || !(s1 > 0.f) || !isfinite(s0) || !isfinite(s1)) bad += 1.0;
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
    double acc[WLM_SUMS];
    double cn = INFINITY;
    if (pd) {
      wlm_accumulate(g3, g2, gs, vidx, n, tid, Rn, tn, fu, fv, uc, vc, delta, acc);
      acc[28] += bad;
      block_sum<WLM_SUMS>(acc, sred, tid);                                    // (its barriers also fence s_trial and s_pd against the next trial)
      if (acc[28] == 0.0 && isfinite(acc[27])) cn = acc[27];
    } else {
      __syncthreads();
    }
    if (it < 0) {
      if (acc[28] != 0.0) { pass = true; break; }                             // a pixel or scale that is not usable, a point not in front
      c = c0 = acc[27];                                                       // (not `cn`: a cost that is not finite is still the state's cost)
      clip = clip0 = acc[29];
      if (tid == 0)
        for (int i = 0; i < 28; ++i) s_H[i] = acc[i];
      continue;
    }
    const bool accept = cn < c;
    if (p.records && tid == 0) {
      double* rec = p.records + ((size_t)b * p.max_iters + it) * WLM_REC;
      rec[0] = lambda; rec[1] = c; rec[2] = cn; rec[3] = accept ? 1.0 : 0.0; rec[4] = s;
      for (int i = 0; i < 9; ++i) rec[5 + i] = Rn[i];
      for (int i = 0; i < 3; ++i) rec[14 + i] = tn[i];
    }
    if (accept) {
      for (int i = 0; i < 9; ++i) R[i] = Rn[i];
      for (int i = 0; i < 3; ++i) t[i] = tn[i];
      c = cn;
      clip = acc[29];
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
    for (int i = 0; i < WLM_INFO; ++i) info[i] = NAN;
    info[2] = (double)n;
    info[3] = 0.0;
    return;
  }
  p.status_out[b] = status;
  info[0] = c0; info[1] = c; info[2] = (double)n; info[3] = (double)iters;
  int e = 0;
  for (int a = 0; a < 6; ++a)
    for (int q = a; q < 6; ++q) { info[4 + 6 * a + q] = s_H[e]; info[4 + 6 * q + a] = s_H[e]; ++e; }
  info[40] = clip0; info[41] = clip;
}

}  // namespace

extern "C" int cp_pnp_refine_wlm_info_doubles(void) { return WLM_INFO; }

extern "C" int cp_pnp_refine_wlm(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* mask,
                                 int mask_stride, const float* scale, const float* cam_K, long long K_bstride, int B, int N,
                                 const double* pose_in, const int32_t* status_in, double huber_delta, int max_iters, double step_tol,
                                 double* pose_out, int32_t* status_out, double* info, double* records) {
  if (!p3d || !p2d || !mask || !scale || !cam_K || !pose_in || !pose_out || !status_out || !info) return CP_ERR_INVALID;
  if (B < 0 || N <= 0 || N > PNP_NMAX || mask_stride <= 0 || max_iters < 1 || max_iters > WLM_MAX_ITERS) return CP_ERR_INVALID;
  if (!cp_finite_positive(step_tol) || cp_p3d_stride_invalid(p3d_bstride, N) || cp_K_stride_invalid(K_bstride)) return CP_ERR_INVALID;
  if (!(huber_delta > 0.0)) return CP_ERR_INVALID;                             // NaN, 0 and negatives; +inf is the unrobust fit
  if (cp_misaligned(pose_in, 7) || cp_misaligned(pose_out, 7) || cp_misaligned(info, 7) || cp_misaligned(records, 7) ||
      cp_misaligned(status_out, 3) || cp_misaligned(status_in, 3))
    return CP_ERR_ALIGN;
  if (cp_pose_alias_invalid(pose_in, pose_out, B)) return CP_ERR_INVALID;
  if (B == 0) return CP_OK;
  WlmParams p;
  p.p3d = p3d; p.p2d = p2d; p.mask = mask; p.scale = scale; p.K = cam_K; p.pose_in = pose_in; p.status_in = status_in;
  p.pose_out = pose_out; p.status_out = status_out; p.info = info; p.records = records;
  p.p3d_bs = p3d_bstride; p.K_bs = K_bstride; p.B = B; p.N = N; p.mask_stride = mask_stride; p.max_iters = max_iters;
  p.step_tol = step_tol; p.delta = huber_delta;
  CP_LAUNCH(pnp_refine_wlm_kernel, dim3((unsigned)B), dim3(PNP_THREADS), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}
