// Pose from correspondences on the device: the solver call of the reference's from_id_to_pose
//   cv2.solvePnPRansac(valid_p3d, valid_disc_p2d, cam_K, None, reprojectionError=2, iterationsCount=150, flags=cv2.SOLVEPNP_EPNP)
// (test_network_with_test_data.py:100-110; identity pose below 4 valid correspondences, :111-114) as a consumer of
// cp_correspondences' output: TWO launches for the whole batch, so the (B, N, 2) coordinates and validity
// masks never leave the GPU -- only 12 doubles per crop do.  opencv-python is not vendored by the reference (and absent here): this
// is the published algorithm -- EPnP (Lepetit, Moreno-Noguer, Fua 2009) in the structure of OpenCV's epnp.cpp inside the RANSAC
// frame of OpenCV's solvePnPRansac -- restated in oracle/pnp_oracle.py, which states the deliberate differences (sample sequence
// from a counter-based hash, no early termination).  All arithmetic in fp64.
//   launch 1 (grid: 64 hypotheses x crop, one wave each; the crop's correspondences staged in LDS, valid indices compacted by
//            ballot scans): lane h draws 5 (4 if only 4 are valid) distinct correspondences, EPnP -> pose h, counts the valid
//            correspondences with squared reprojection error <= threshold^2 -> a 14-double record in scratch;
//   launch 2 (one 256-thread workgroup per crop): best = most inliers (first on ties, at least a full sample); its inlier list
//            is compacted; EPnP over the inliers with every loop over the points shared by the 256 threads (block reductions:
//            centroid, scatter matrix, the 78 entries of M^T M, the candidates' centroids / cross-covariances / errors) and
//            the small dense algebra (12 x 12 Jacobi, betas, Gauss-Newton, 3 x 3 SVD) on single threads.
// (The first version -- everything in one workgroup, serial passes on thread 0 straight from global memory -- took 7.2 ms per
// batch whatever its size; see tools/pnp_bench.py.)
#include "pnp_core.h"

namespace {

struct PnpParams {
  const float* p3d; const float* p2d; const uint8_t* valid; const float* K;
  double* pose; uint8_t* inliers; int32_t* status;
  int32_t* unused;             // (no reader.  Without it the arguments are laid out and fetched differently: 16 more SGPR spills in the
  long long p3d_bs, K_bs;      //  selection kernel, or with the strides last ~1 % on a B = 32 call)
  int B, N, valid_stride, iters, round;
  float thr;
  uint32_t seed;
};


// ---------------------------------------------------------------------------------------------- launch 1: the hypotheses
// one launch per round of 64 hypotheses, grid (1, B), one wave per workgroup, a hypothesis per lane (M^T M and its eigenvectors of
// all 64 lanes in 147 KB of LDS).  Round r > 0 first applies OpenCV's stopping rule to the records of the earlier rounds: with
// 70 % inliers 25 iterations suffice, so rounds 1 and 2 of the default 150 iterations usually return at once
__global__ __launch_bounds__(64) void pnp_hypotheses_kernel(const PnpParams p, double* __restrict__ hyp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* const sA = (double*)smem;                          // [144][64]: M^T M of lane l at [e * 64 + l]
  double* const sV = sA + 144 * 64;                          // [144][64]: its eigenvectors
  uint16_t* const vidx = (uint16_t*)(sV + 144 * 64);         // [N] valid indices, ascending
  __shared__ int wsum[1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint8_t* valid = p.valid + (size_t)b * p.N * p.valid_stride;
  const int vs = p.valid_stride;
  const int nv = block_compact<64>([&](int i) { return valid[(size_t)i * vs] != 0; }, p.N, vidx, wsum, tid);
  const int h = p.round * 64 + tid;
  if (nv < 5) return;                                        // < 4: identity; exactly 4: P3P in the selection launch, no hypotheses
  if (p.round > 0 && hypotheses_run(hyp + (size_t)b * p.iters * PNP_HYP, nv, 5, p.iters, p.round) <= 64 * p.round)
    return;                                                  // the rule was satisfied by the earlier rounds: whole workgroup, uniform
  if (h >= p.iters) return;
  // straight from global memory: the scoring loop reads the SAME point on every lane (one cache line per wave), the solve only its 5 samples
  const Points P = crop_points(p.p3d + (size_t)b * p.p3d_bs, p.p2d + (size_t)b * p.N * 2, p.K + (size_t)b * p.K_bs);
  const double thr2 = (double)p.thr * (double)p.thr;
  const int m = 5;
  // pnp_core.h's sample_distinct, mapped through vidx (ascending, so comparing mapped values is comparing positions), kept as its own
  // loop: with the positions in registers the five-point solve below unrolls differently and every hypothesis moves in its last bits
  int32_t sel[5];
  int got = 0;
  uint32_t tries = 0;
  while (got < m) {
    const int r = (int)(hash32(p.seed, (uint32_t)b, (uint32_t)h, tries++) % (uint32_t)nv);
    bool dup = false;
    for (int k = 0; k < got; ++k) dup = dup || sel[k] == (int32_t)vidx[r];
    if (!dup) sel[got++] = (int32_t)vidx[r];
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
    for (int i = 0; i < nv; ++i) cnt += is_inlier(P, R, t, (int)vidx[i], thr2) ? 1 : 0;
    for (int i = 0; i < 9; ++i) rec[2 + i] = R[i];
    for (int i = 0; i < 3; ++i) rec[11 + i] = t[i];
  }
  rec[0] = (double)cnt;
}

// ---------------------------------------------------------------------------------------------- launch 2: selection + final EPnP

__global__ __launch_bounds__(PNP_THREADS) void pnp_select_refit_kernel(const PnpParams p, const double* __restrict__ hyp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* const s3 = (float*)smem;
  float* const s2 = s3 + 3 * p.N;
  int32_t* const vidx = (int32_t*)(s2 + 2 * p.N);
  int32_t* const iidx = vidx + p.N;
  bool* const flag = (bool*)(iidx + p.N);
  __shared__ double sred[4 * 27];
  __shared__ double s_mtm[144], s_evec[144];
  __shared__ double s_cc[3][4][3], s_Rt[3][12];
  __shared__ Frame s_frame;
  __shared__ int wsum[PNP_THREADS / 64], s_best, s_ok, s_kok[3];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* g3 = p.p3d + (size_t)b * p.p3d_bs;
  const float* g2 = p.p2d + (size_t)b * p.N * 2;
  const uint8_t* valid = p.valid + (size_t)b * p.N * p.valid_stride;
  for (int i = tid; i < 3 * p.N; i += PNP_THREADS) s3[i] = g3[i];
  for (int i = tid; i < 2 * p.N; i += PNP_THREADS) s2[i] = g2[i];
  for (int i = tid; i < p.N; i += PNP_THREADS) { flag[i] = valid[(size_t)i * p.valid_stride] != 0; p.inliers[(size_t)b * p.N + i] = 0; }
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
  if (nv == 4) {                                             // OpenCV: no RANSAC, P3P + the fourth point; all four are inliers
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
  const double thr2 = (double)p.thr * (double)p.thr;
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
    const bool in = is_inlier(P, Rb, tb, k, thr2);
    flag[k] = in;
    if (in) p.inliers[(size_t)b * p.N + k] = 1;
  }
  __syncthreads();
  const int n = block_compact<PNP_THREADS>([&](int i) { return flag[i]; }, p.N, iidx, wsum, tid);
  Points S = P;
  S.idx = iidx; S.n = n;
  // ---- final EPnP over the n inliers, loops over the points shared by the 256 threads, the small dense algebra on thread 0: the
  // statements of pnp_core.h's epnp_block_refit, kept in the kernel.  Behind a call (a function, forced inline or not, or a lambda) the
  // compiler optimises them before it inlines them, and the poses of 26 of the 32 committed cases move in their last bits
  double acc[27];
  for (int k = 0; k < 3; ++k) acc[k] = 0.0;
  for (int i = tid; i < n; i += PNP_THREADS) { const float* pw = s3 + 3 * iidx[i]; acc[0] += pw[0]; acc[1] += pw[1]; acc[2] += pw[2]; }
  block_sum<3>(acc, sred, tid);
  const double pw0[3] = {acc[0] / n, acc[1] / n, acc[2] / n};
  for (int k = 0; k < 6; ++k) acc[k] = 0.0;
  for (int i = tid; i < n; i += PNP_THREADS) {
    const float* pw = s3 + 3 * iidx[i];
    const double d0 = pw[0] - pw0[0], d1 = pw[1] - pw0[1], d2 = pw[2] - pw0[2];
    acc[0] += d0 * d0; acc[1] += d0 * d1; acc[2] += d0 * d2; acc[3] += d1 * d1; acc[4] += d1 * d2; acc[5] += d2 * d2;
  }
  block_sum<6>(acc, sred, tid);
  if (tid == 0) {
    const double Sm[9] = {acc[0], acc[1], acc[2], acc[1], acc[3], acc[4], acc[2], acc[4], acc[5]};
    s_ok = epnp_frame_from(pw0, Sm, n, s_frame) ? 1 : 0;
  }
  __syncthreads();
  bool ok = s_ok != 0;
  if (ok && tid < 78) {                                      // entry (a, c), a <= c, of M^T M per thread
    int a = 0, rem = tid;
    while (rem >= 12 - a) { rem -= 12 - a; ++a; }
    const int c = a + rem;
    double e = 0.0;
    for (int i = 0; i < n; ++i) {
      double r0[12], r1[12];
      m_rows(S, s_frame, i, r0, r1);
      e += r0[a] * r0[c] + r1[a] * r1[c];
    }
    s_mtm[a * 12 + c] = e;
    s_mtm[c * 12 + a] = e;
  }
  __syncthreads();
  if (ok && tid < 64) jacobi_eig12_wave(s_mtm, s_evec, tid);  // wave 0: the 12 x 12 eigen-solve on 12 lanes
  __syncthreads();
  if (ok && tid == 0) {                                      // null-space basis, betas of the three approximations, camera-frame control points
    double v[4][12], cc[3][4][3];
    bool kok[3];
    epnp_betas(S, s_frame, s_mtm, s_evec, -1, v, cc, kok);
    for (int k = 0; k < 3; ++k) {
      s_kok[k] = kok[k] ? 1 : 0;
      for (int j = 0; j < 4; ++j)
        for (int c = 0; c < 3; ++c) s_cc[k][j][c] = cc[k][j][c];
    }
  }
  __syncthreads();
  if (ok) {
    // pc0 of the three candidates (9 sums), then their cross-covariances with the model points (27 sums), then their errors (3)
    auto pc_of = [&](int k, int i, double* pc) {
      double al[4];
      alphas_of(s_frame, s3 + 3 * iidx[i], al);
      for (int c = 0; c < 3; ++c) pc[c] = al[0] * s_cc[k][0][c] + al[1] * s_cc[k][1][c] + al[2] * s_cc[k][2][c] + al[3] * s_cc[k][3][c];
    };
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += PNP_THREADS)
      for (int k = 0; k < 3; ++k) { double pc[3]; pc_of(k, i, pc); acc[3 * k] += pc[0]; acc[3 * k + 1] += pc[1]; acc[3 * k + 2] += pc[2]; }
    block_sum<9>(acc, sred, tid);
    double pc0[3][3];
    for (int k = 0; k < 3; ++k)
      for (int c = 0; c < 3; ++c) pc0[k][c] = acc[3 * k + c] / n;
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += PNP_THREADS) {
      const float* pw = s3 + 3 * iidx[i];
      for (int k = 0; k < 3; ++k) {
        double pc[3];
        pc_of(k, i, pc);
        for (int a = 0; a < 3; ++a)
          for (int c = 0; c < 3; ++c) acc[9 * k + 3 * a + c] += (pc[a] - pc0[k][a]) * (pw[c] - pw0[c]);
      }
    }
    block_sum<27>(acc, sred, tid);
    if (tid < 3 && s_kok[tid]) {                             // absolute orientation of candidate `tid`
      double R[9], t[3];
      procrustes_rotation(acc + 9 * tid, R);
      for (int a = 0; a < 3; ++a) t[a] = pc0[tid][a] - (R[3 * a] * pw0[0] + R[3 * a + 1] * pw0[1] + R[3 * a + 2] * pw0[2]);
      for (int i = 0; i < 9; ++i) s_Rt[tid][i] = R[i];
      for (int i = 0; i < 3; ++i) s_Rt[tid][9 + i] = t[i];
    }
    __syncthreads();
    for (int k = 0; k < 3; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += PNP_THREADS) {
      const int kk = iidx[i];
      const float* pw = s3 + 3 * kk;
      for (int k = 0; k < 3; ++k) {
        if (!s_kok[k]) continue;
        const double* R = s_Rt[k];
        const double X = R[0] * pw[0] + R[1] * pw[1] + R[2] * pw[2] + R[9], Y = R[3] * pw[0] + R[4] * pw[1] + R[5] * pw[2] + R[10];
        const double iz = 1.0 / (R[6] * pw[0] + R[7] * pw[1] + R[8] * pw[2] + R[11]);
        const double du = P.uc + P.fu * X * iz - s2[2 * kk], dv = P.vc + P.fv * Y * iz - s2[2 * kk + 1];
        acc[k] += sqrt(du * du + dv * dv);
      }
    }
    block_sum<3>(acc, sred, tid);
    if (tid == 0) {
      int pick = -1;
      double be = INFINITY;
      for (int k = 0; k < 3; ++k)
        if (s_kok[k] && isfinite(acc[k]) && acc[k] < be) { be = acc[k]; pick = k; }
      if (pick >= 0) {
        for (int i = 0; i < 12; ++i) pose[i] = s_Rt[pick][i];
      } else ok = false;
      s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    ok = s_ok != 0;
  }
  if (tid == 0) {
    if (!ok) {                                               // degenerate inlier set: keep the winning hypothesis
      for (int i = 0; i < 9; ++i) pose[i] = Rb[i];
      for (int i = 0; i < 3; ++i) pose[9 + i] = tb[i];
    }
    p.status[b] = 1;
  }
}

}  // namespace

extern "C" size_t cp_pnp_ransac_scratch_bytes(int B, int N) { (void)N; return (size_t)B * PNP_MAX_ITERS * PNP_HYP * sizeof(double); }

extern "C" int cp_pnp_ransac(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* valid,
                             int valid_stride, const float* cam_K, long long K_bstride, int B, int N, float reproj_threshold,
                             int iterations, uint32_t seed, double* pose, uint8_t* inliers, int32_t* status, void* scratch) {
  if (!p3d || !p2d || !valid || !cam_K || !pose || !inliers || !status || !scratch) return CP_ERR_INVALID;
  if (B <= 0 || N <= 0 || N > PNP_NMAX || valid_stride <= 0 || iterations <= 0 || iterations > PNP_MAX_ITERS || !(reproj_threshold > 0.f))
    return CP_ERR_INVALID;
  if (cp_p3d_stride_invalid(p3d_bstride, N) || cp_K_stride_invalid(K_bstride)) return CP_ERR_INVALID;
  if (cp_misaligned(pose, 7) || cp_misaligned(scratch, 7) || cp_misaligned(status, 3)) return CP_ERR_ALIGN;
  PnpParams p;
  p.p3d = p3d; p.p2d = p2d; p.valid = valid; p.K = cam_K; p.pose = pose; p.inliers = inliers; p.status = status; p.unused = nullptr;
  p.p3d_bs = p3d_bstride; p.K_bs = K_bstride; p.B = B; p.N = N; p.valid_stride = valid_stride; p.iters = iterations; p.thr = reproj_threshold;
  p.seed = seed;
  const size_t lds1 = (size_t)2 * 144 * 64 * 8 + (size_t)N * 2 + 16, lds2 = (size_t)N * (5 * 4 + 8 + 1) + 16;
  static CpDeviceOnce once;                  // both kernels are sized for PNP_NMAX keypoints, once per device
  const int dev = cp_current_device();
  CP_LDS_ATTR_ONCE(once, dev, cp_set_max_lds((const void*)pnp_hypotheses_kernel, (size_t)2 * 144 * 64 * 8 + PNP_NMAX * 2 + 16) &&
                                  cp_set_max_lds((const void*)pnp_select_refit_kernel, (size_t)PNP_NMAX * 29 + 16));
  hipStream_t st = (hipStream_t)stream;
  for (int r = 0; 64 * r < iterations; ++r) {
    p.round = r;
    CP_LAUNCH(pnp_hypotheses_kernel, dim3((unsigned)B), dim3(64), lds1, st, p, (double*)scratch);
  }
  p.round = 0;
  CP_LAUNCH(pnp_select_refit_kernel, dim3((unsigned)B), dim3(PNP_THREADS), lds2, st, p, (const double*)scratch);
  return cp_check_launch();
}
