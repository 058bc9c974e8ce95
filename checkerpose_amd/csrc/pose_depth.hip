#pragma clang fp contract(off)
// Pose from depth-lifted correspondences on the device: RANSAC over a closed-form 3-D -- 3-D minimal solver
// (three pairs, absolute orientation) with a local optimisation, for a user whose RGB-D frame is resident on the device.  Both PnP
// solvers (pnp.hip, pnp_gc.hip) solve a 2-D -- 3-D problem whose pose is weakest along the viewing ray; with the sensor's depth under
// each correspondence the problem is 3-D -- 3-D and needs no mesh and no start pose (icp_refine.hip, row N24, needs both).  The
// reference uses no depth at test time: the row is opt-in and its rule is this project's OWN (tests/depth_pose_stages.py restates it in
// numpy; parity with any library is UNPINNED).
//
// THE RULE.  fp64 without contraction (the pragma above covers pnp_core.h too).  fx, fy, cx, cy = K[0], K[4], K[2], K[5] (fp32 inputs).
//
// Stage A, the lift (cp_lift_correspondences; one lane per (crop, keypoint)).  The image of crop b is image_ids[b], or without ids
//   image 0 when I == 1 and image b when I == B.  A keypoint whose `valid` byte is set, with (u, v) = its fp32 p2d:
//   pixel (x, y) = (floor u, floor v) -- icp_refine.hip's lookup; dropped when the image id is outside 0..I-1, when the pixel is outside
//   the frame (u, v not finite included), or when z = depth[image, y, x] is not finite or <= 0; else
//   Q = (((u - cx) / fx) z, ((v - cy) / fy) z, z) in fp64 from the fp32 inputs, rounded ONCE to fp32: the ray goes through (u, v) as
//   given -- the point both PnP solvers use -- not through the pixel centre.
//   Outputs: Q fp32 (B,N,3) (0 where not lifted), lifted uint8 (B,N), n_lifted int32 (B) = a wave butterfly and one integer atomic per
//   wave (order-free).
//
// Stage B, RANSAC (one 256-thread workgroup per crop).  The n lifted keypoints in ascending order; X_j, Q_j their fp32 model and lifted
//   points.  n < 3, or a threshold that is not finite and > 0: status 0, the identity pose, no inliers (the reference's fallback, as in
//   cp_pnp_ransac).
//   hypothesis h draws 3 distinct positions in [0, n) with pnp_core.h's hash32 (draw k = hash32(seed, crop, h, try) % n, duplicates
//   redrawn: oracle/pnp_oracle.py:sample_indices with m = 3) -> pairs 0, 1, 2.
//   degenerate (record count -1): |(X1 - X0) x (X2 - X0)|^2 <= 1e-12 (max(|X1 - X0|^2, |X2 - X0|^2, |X2 - X1|^2))^2, or rank(H) < 2 below.
//   pose: x = ((X0 + X1) + X2) / 3, q likewise; H[a][c] = sum_i (Q_i[a] - q[a]) (X_i[c] - x[c]) in the order i = 0, 1, 2;
//   R = nearest_rotation(H) (pnp_core.h: the proper rotation nearest H, third direction by the cross product, so rank 2 -- three points,
//   coplanar points -- needs no special case); t[a] = q[a] - ((R[a][0] x[0] + R[a][1] x[1]) + R[a][2] x[2]).
//   inlier test of lifted keypoint j under (R, t): d[a] = (((R[a][0] X[0] + R[a][1] X[1]) + R[a][2] X[2]) + t[a]) - Q[a];
//   (d[0]^2 + d[1]^2) + d[2]^2 <= dist_threshold^2.  count = the inliers among the n lifted keypoints.
//   Hypotheses run in rounds of 64, at most 256 iterations; round r > 0 runs only while 64 r < needed_iters(best count so far, n, 3,
//   iterations) (pnp_core.h, unchanged).  The winner has the most inliers (>= 3), the first on ties; none: status 0, identity.
//
// Stage C, local optimisation.  L = the winner's inliers; fit(L): x, q = the means over L, H = sum over L of (Q - q)(X - x)^T, R, t as above;
//   it fails when rank(H) < 2.  P = fit(L); if that fails the hypothesis's own pose is returned with L.  Then at most 3 times:
//   L' = inliers(P); stop if |L'| <= |L|; P' = fit(L'), stop if it fails; else L = L', P = P'.  Returned: (P, L) with status 1 -- the pose
//   is the least-squares fit over the returned inliers (except after a failed first fit).
//   The sums of a fit: thread t of 256 adds its keypoints t, t + 256, ... in ascending order, block_sum joins the threads (fixed order).
//
// Records (part of the interface; scratch, see cp_pose_depth_ransac): 14 doubles per hypothesis [count or -1, unused, R, t] (pose only
//   when count >= 0), records of rounds that the stopping rule cut off unwritten; 4 step records of 14 doubles per crop
//   [|L| or |L'| of the step, accepted 0 / 1, R, t of the state after the step]: step 0 = the first fit (accepted = it succeeded), steps
//   1..3 the iterations that ran; others unwritten.
//
// The solver kernel keeps X and Q of the lifted keypoints (fp32, 24 bytes each), their indices and two inlier flags in LDS: 28 N bytes,
// 112 KB at N = 4096, requested as large dynamic LDS like pnp.hip's kernels.  A round: wave 0 solves the 64 hypotheses (a lane each, all
// in registers), then the four waves score them -- wave w takes lifted keypoints w, w + 4, ... and lane k hypothesis k, so every LDS
// read is a broadcast -- and integer counts are added through LDS.  Every branch on a round, a winner or a step is taken on LDS words
// or block_sum results that all threads hold identically; every loop is bounded by the iterations, N or 3.
#include "pnp_core.h"

namespace {

constexpr int PD_STEPS = 4, PD_LIFT_THREADS = 256;

struct LiftParams {
  const float* p2d; const uint8_t* valid; const float* K; const float* depth; const int32_t* image_ids;
  float* Q; uint8_t* lifted; int32_t* n_lifted;
  long long K_bs;
  int B, N, valid_stride, I, H, W;
};

__global__ __launch_bounds__(PD_LIFT_THREADS) void pose_depth_lift_kernel(const LiftParams p) {
  const int chunks = (p.N + PD_LIFT_THREADS - 1) / PD_LIFT_THREADS;           // whole chunks per crop: a wave never spans two crops
  const int b = blockIdx.x / chunks, i = (blockIdx.x - b * chunks) * PD_LIFT_THREADS + threadIdx.x;
  int got = 0;
  if (i < p.N) {
    const size_t k = (size_t)b * p.N + i;
    float q0 = 0.f, q1 = 0.f, q2 = 0.f;
    const int img = p.image_ids ? p.image_ids[b] : (p.I == 1 ? 0 : b);
    if (p.valid[k * p.valid_stride] != 0 && img >= 0 && img < p.I) {
      const float u = p.p2d[2 * k], v = p.p2d[2 * k + 1];
      if (u >= 0.f && v >= 0.f && (double)u < (double)p.W && (double)v < (double)p.H) {      // (NaN fails the comparisons)
        const int x = (int)floorf(u), y = (int)floorf(v);
        const float z = p.depth[((size_t)img * p.H + y) * p.W + x];
        if (isfinite(z) && z > 0.f) {
          const float* K = p.K + (size_t)b * p.K_bs;
          const double fx = K[0], fy = K[4], cx = K[2], cy = K[5], zd = z;
          q0 = (float)((((double)u - cx) / fx) * zd);
          q1 = (float)((((double)v - cy) / fy) * zd);
          q2 = z;
          got = 1;
        }
      }
    }
    p.Q[3 * k] = q0; p.Q[3 * k + 1] = q1; p.Q[3 * k + 2] = q2;
    p.lifted[k] = (uint8_t)got;
  }
  int s = got;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(p.n_lifted + b, s);
}

struct PdParams {
  const float* p3d; const float* Q; const uint8_t* lifted; const double* thr_b;
  double* pose; uint8_t* inliers; int32_t* status; double* hyp; double* steps;
  long long p3d_bs;
  double thr;
  int B, N, iters;
  uint32_t seed;
};

__device__ __forceinline__ bool pd_inlier(const double* P, const float* X, const float* Q, double thr2) {
  const double x = X[0], y = X[1], z = X[2];
  const double d0 = (((P[0] * x + P[1] * y) + P[2] * z) + P[9]) - (double)Q[0];
  const double d1 = (((P[3] * x + P[4] * y) + P[5] * z) + P[10]) - (double)Q[1];
  const double d2 = (((P[6] * x + P[7] * y) + P[8] * z) + P[11]) - (double)Q[2];
  return (d0 * d0 + d1 * d1) + d2 * d2 <= thr2;
}

// the pose of three pairs (positions s0, s1, s2 of the staged keypoints) -> P[12]; false: degenerate
__device__ __forceinline__ bool pd_minimal(const float* sX, const float* sQ, int s0, int s1, int s2, double* P) {
  double X[3][3], Q[3][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    X[0][c] = sX[3 * s0 + c]; X[1][c] = sX[3 * s1 + c]; X[2][c] = sX[3 * s2 + c];
    Q[0][c] = sQ[3 * s0 + c]; Q[1][c] = sQ[3 * s1 + c]; Q[2][c] = sQ[3 * s2 + c];
  }
  double e1[3], e2[3], e3[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { e1[c] = X[1][c] - X[0][c]; e2[c] = X[2][c] - X[0][c]; e3[c] = X[2][c] - X[1][c]; }
  const double c0 = e1[1] * e2[2] - e1[2] * e2[1], c1 = e1[2] * e2[0] - e1[0] * e2[2], c2 = e1[0] * e2[1] - e1[1] * e2[0];
  const double l1 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2], l2 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
  const double l3 = (e3[0] * e3[0] + e3[1] * e3[1]) + e3[2] * e3[2];
  const double lm = fmax(fmax(l1, l2), l3);
  if ((c0 * c0 + c1 * c1) + c2 * c2 <= 1e-12 * (lm * lm)) return false;
  double x[3], q[3], H[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) { x[c] = ((X[0][c] + X[1][c]) + X[2][c]) / 3.0; q[c] = ((Q[0][c] + Q[1][c]) + Q[2][c]) / 3.0; }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      H[3 * a + c] = ((Q[0][a] - q[a]) * (X[0][c] - x[c]) + (Q[1][a] - q[a]) * (X[1][c] - x[c])) + (Q[2][a] - q[a]) * (X[2][c] - x[c]);
  if (nearest_rotation(H, P) < 2) return false;
#pragma unroll
  for (int a = 0; a < 3; ++a) P[9 + a] = q[a] - ((P[3 * a] * x[0] + P[3 * a + 1] * x[1]) + P[3 * a + 2] * x[2]);
  return true;
}

__global__ __launch_bounds__(PNP_THREADS) void pose_depth_ransac_kernel(const PdParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* const sX = (float*)smem;                              // [3 n] model points of the lifted keypoints
  float* const sQ = sX + 3 * p.N;                              // [3 n] their lifted points
  uint16_t* const lidx = (uint16_t*)(sQ + 3 * p.N);            // [n] their indices, ascending
  uint8_t* const flagL = (uint8_t*)(lidx + p.N);               // [n] the inlier set L
  uint8_t* const flagN = flagL + p.N;                          // [n] the candidate L'
  __shared__ double sred[4 * 9];
  __shared__ double s_pose[64][12], s_best[12], s_fit[12];
  __shared__ int s_cnt[4][64], s_ok[64], wsum[PNP_THREADS / 64], s_bc, s_bh, s_go, s_fitok;
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint8_t* lifted = p.lifted + (size_t)b * p.N;
  for (int i = tid; i < p.N; i += PNP_THREADS) p.inliers[(size_t)b * p.N + i] = 0;
  const int n = block_compact<PNP_THREADS>([&](int i) { return lifted[i] != 0; }, p.N, lidx, wsum, tid);
  {
    const float* g3 = p.p3d + (size_t)b * p.p3d_bs;
    const float* gq = p.Q + (size_t)b * p.N * 3;
    for (int e = tid; e < 3 * n; e += PNP_THREADS) {
      const int j = e / 3, c = e - 3 * j, k = lidx[j];
      sX[e] = g3[3 * k + c]; sQ[e] = gq[3 * k + c];
    }
  }
  if (tid == 0) { s_bc = 2; s_bh = -1; }
  __syncthreads();
  double* pose = p.pose + (size_t)b * 12;
  auto identity = [&]() {                                      // the reference's fallback: identity pose, no inliers
    if (tid == 0) {
      write_identity_pose(pose);
      p.status[b] = 0;
    }
  };
  const double thr = p.thr_b ? p.thr_b[b] : p.thr;
  if (n < 3 || !cp_finite_positive(thr)) { identity(); return; }
  const double thr2 = thr * thr;
  // ---- stage B
  const int lane = tid & 63, part = tid >> 6;
  for (int r = 0; 64 * r < p.iters; ++r) {
    const int h = 64 * r + lane;
    if (tid < 64) {
      bool ok = false;
      if (h < p.iters) {
        int pos[3];
        double P[12];
        ok = sample_distinct<3>(p.seed, (uint32_t)b, (uint32_t)h, n, pos) && pd_minimal(sX, sQ, pos[0], pos[1], pos[2], P);
        if (ok)
#pragma unroll
          for (int i = 0; i < 12; ++i) s_pose[lane][i] = P[i];
      }
      s_ok[lane] = ok ? 1 : 0;
    }
    __syncthreads();
    {
      int c = 0;
      if (s_ok[lane]) {
        double P[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) P[i] = s_pose[lane][i];
        for (int j = part; j < n; j += 4) c += pd_inlier(P, sX + 3 * j, sQ + 3 * j, thr2) ? 1 : 0;
      }
      s_cnt[part][lane] = c;
    }
    __syncthreads();
    if (tid < 64 && h < p.iters) {
      double* rec = p.hyp + ((size_t)b * p.iters + h) * PNP_HYP;
      if (s_ok[lane]) {
        rec[0] = (double)(((s_cnt[0][lane] + s_cnt[1][lane]) + s_cnt[2][lane]) + s_cnt[3][lane]);
#pragma unroll
        for (int i = 0; i < 12; ++i) rec[2 + i] = s_pose[lane][i];
      } else rec[0] = -1.0;
    }
    if (tid == 0) {
      int bc = s_bc, bh = s_bh;
      const int hn = p.iters - 64 * r < 64 ? p.iters - 64 * r : 64;
      for (int k = 0; k < hn; ++k) {
        if (!s_ok[k]) continue;
        const int c = ((s_cnt[0][k] + s_cnt[1][k]) + s_cnt[2][k]) + s_cnt[3][k];
        if (c > bc) { bc = c; bh = 64 * r + k; for (int i = 0; i < 12; ++i) s_best[i] = s_pose[k][i]; }
      }
      s_bc = bc; s_bh = bh;
      s_go = 64 * (r + 1) < needed_iters(bh >= 0 ? bc : -1, n, 3, p.iters) ? 1 : 0;
    }
    __syncthreads();
    if (!s_go) break;                                          // (uniform: an LDS word)
  }
  if (s_bh < 0) { identity(); return; }
  // ---- stage C
  double P[12];
  for (int i = 0; i < 12; ++i) P[i] = s_best[i];
  auto mark = [&](uint8_t* fl) {                               // fl = inliers(P) -> their number on every thread
    double c[1] = {0.0};
    for (int j = tid; j < n; j += PNP_THREADS) { const bool in = pd_inlier(P, sX + 3 * j, sQ + 3 * j, thr2); fl[j] = in ? 1 : 0; c[0] += in ? 1.0 : 0.0; }
    block_sum<1>(c, sred, tid);
    return c[0];
  };
  auto fit = [&](const uint8_t* fl, double cnt, double* Pn) {  // the least-squares pose over the flagged keypoints -> Pn on every thread
    double acc[9];
    for (int k = 0; k < 6; ++k) acc[k] = 0.0;
    for (int j = tid; j < n; j += PNP_THREADS)
      if (fl[j]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { acc[c] += (double)sX[3 * j + c]; acc[3 + c] += (double)sQ[3 * j + c]; }
      }
    block_sum<6>(acc, sred, tid);
    const double x[3] = {acc[0] / cnt, acc[1] / cnt, acc[2] / cnt}, q[3] = {acc[3] / cnt, acc[4] / cnt, acc[5] / cnt};
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    for (int j = tid; j < n; j += PNP_THREADS)
      if (fl[j]) {
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[3 * a + c] += ((double)sQ[3 * j + a] - q[a]) * ((double)sX[3 * j + c] - x[c]);
      }
    block_sum<9>(acc, sred, tid);
    if (tid == 0) {
      double R[9];
      const bool ok = nearest_rotation(acc, R) >= 2;
      s_fitok = ok ? 1 : 0;
      if (ok) {
        for (int i = 0; i < 9; ++i) s_fit[i] = R[i];
        for (int a = 0; a < 3; ++a) s_fit[9 + a] = q[a] - ((R[3 * a] * x[0] + R[3 * a + 1] * x[1]) + R[3 * a + 2] * x[2]);
      }
    }
    __syncthreads();
    const bool ok = s_fitok != 0;
    if (ok)
      for (int i = 0; i < 12; ++i) Pn[i] = s_fit[i];
    __syncthreads();
    return ok;
  };
  auto step_record = [&](int k, double cnt, bool accepted) {
    if (tid == 0) {
      double* rec = p.steps + ((size_t)b * PD_STEPS + k) * PNP_HYP;
      rec[0] = cnt; rec[1] = accepted ? 1.0 : 0.0;
      for (int i = 0; i < 12; ++i) rec[2 + i] = P[i];
    }
  };
  double nL = mark(flagL);
  uint8_t* fL = flagL;
  uint8_t* fN = flagN;
  double Pn[12];
  bool ok = fit(fL, nL, Pn);
  if (ok)
    for (int i = 0; i < 12; ++i) P[i] = Pn[i];
  step_record(0, nL, ok);
  for (int k = 1; k < PD_STEPS && ok; ++k) {
    const double nN = mark(fN);
    ok = nN > nL;
    if (ok) ok = fit(fN, nN, Pn);
    if (ok) {
      for (int i = 0; i < 12; ++i) P[i] = Pn[i];
      uint8_t* tmp = fL; fL = fN; fN = tmp;
      nL = nN;
    }
    step_record(k, nN, ok);
  }
  for (int j = tid; j < n; j += PNP_THREADS)
    if (fL[j]) p.inliers[(size_t)b * p.N + lidx[j]] = 1;
  if (tid == 0) {
    for (int i = 0; i < 12; ++i) pose[i] = P[i];
    p.status[b] = 1;
  }
}

// ---- host halves
constexpr size_t PD_LDS_PER_POINT = 2 * 3 * sizeof(float) + sizeof(uint16_t) + 2;

inline int pd_common_invalid(const float* p2d, const uint8_t* valid, int valid_stride, const float* cam_K, long long K_bstride, const float* depth,
                             const int32_t* image_ids, int I, int H, int W, int B, int N) {
  if (!p2d || !valid || !cam_K || !depth) return CP_ERR_INVALID;
  if (B < 0 || N <= 0 || N > PNP_NMAX || valid_stride <= 0 || H <= 0 || W <= 0 || I <= 0) return CP_ERR_INVALID;
  if (cp_K_stride_invalid(K_bstride)) return CP_ERR_INVALID;
  if (!image_ids && I != 1 && I != B && B != 0) return CP_ERR_INVALID;
  if (cp_misaligned(p2d, 3) || cp_misaligned(cam_K, 3) || cp_misaligned(depth, 3) || cp_misaligned(image_ids, 3)) return CP_ERR_ALIGN;
  if ((long long)H * W >= (1LL << 31) || B >= (1 << 24)) return CP_ERR_RANGE;
  return CP_OK;
}

int pd_launch_lift(hipStream_t st, const float* p2d, const uint8_t* valid, int valid_stride, const float* cam_K, long long K_bstride,
                   const float* depth, const int32_t* image_ids, int I, int H, int W, int B, int N, float* Q, uint8_t* lifted, int32_t* n_lifted) {
  LiftParams p;
  p.p2d = p2d; p.valid = valid; p.K = cam_K; p.depth = depth; p.image_ids = image_ids; p.Q = Q; p.lifted = lifted; p.n_lifted = n_lifted;
  p.K_bs = K_bstride; p.B = B; p.N = N; p.valid_stride = valid_stride; p.I = I; p.H = H; p.W = W;
  if (hipMemsetAsync(n_lifted, 0, (size_t)B * sizeof(int32_t), st) != hipSuccess) return CP_ERR_HIP;
  CP_LAUNCH(pose_depth_lift_kernel, dim3((unsigned)((N + PD_LIFT_THREADS - 1) / PD_LIFT_THREADS) * (unsigned)B), dim3(PD_LIFT_THREADS), 0, st, p);
  return CP_OK;
}

// the scratch of cp_pose_depth_ransac: [hypothesis records | step records | Q | n_lifted | lifted], byte offsets
struct PdScratch { size_t steps, Q, n_lifted, lifted, total; };
inline PdScratch pd_scratch(int B, int N, int iterations) {
  PdScratch s;
  s.steps = (size_t)B * iterations * PNP_HYP * sizeof(double);
  s.Q = s.steps + (size_t)B * PD_STEPS * PNP_HYP * sizeof(double);
  s.n_lifted = s.Q + (size_t)B * N * 3 * sizeof(float);
  s.lifted = s.n_lifted + (size_t)B * sizeof(int32_t);
  s.total = (s.lifted + (size_t)B * N + 7) & ~(size_t)7;
  return s;
}

}  // namespace

extern "C" int cp_pose_depth_record_doubles(void) { return PNP_HYP; }

extern "C" int cp_lift_correspondences(cp_stream_t stream, const float* p2d, const uint8_t* valid, int valid_stride, const float* cam_K,
                                       long long K_bstride, const float* depth, const int32_t* image_ids, int I, int H, int W, int B, int N,
                                       float* Q, uint8_t* lifted, int32_t* n_lifted) {
  if (!Q || !lifted || !n_lifted) return CP_ERR_INVALID;
  const int rc = pd_common_invalid(p2d, valid, valid_stride, cam_K, K_bstride, depth, image_ids, I, H, W, B, N);
  if (rc != CP_OK) return rc;
  if (cp_misaligned(Q, 3) || cp_misaligned(n_lifted, 3)) return CP_ERR_ALIGN;
  if (B == 0) return CP_OK;
  const int lc = pd_launch_lift((hipStream_t)stream, p2d, valid, valid_stride, cam_K, K_bstride, depth, image_ids, I, H, W, B, N, Q, lifted, n_lifted);
  return lc != CP_OK ? lc : cp_check_launch();
}

extern "C" size_t cp_pose_depth_ransac_scratch_bytes(int B, int N, int iterations) {
  if (B <= 0 || N <= 0 || N > PNP_NMAX || iterations <= 0 || iterations > PNP_MAX_ITERS) return 0;
  return pd_scratch(B, N, iterations).total;
}

extern "C" int cp_pose_depth_ransac(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* valid,
                                    int valid_stride, const float* cam_K, long long K_bstride, const float* depth, const int32_t* image_ids,
                                    int I, int H, int W, int B, int N, double dist_threshold, const double* dist_thresholds, int iterations,
                                    uint32_t seed, double* pose, uint8_t* inliers, int32_t* status, void* scratch) {
  if (!p3d || !pose || !inliers || !status || !scratch) return CP_ERR_INVALID;
  const int rc = pd_common_invalid(p2d, valid, valid_stride, cam_K, K_bstride, depth, image_ids, I, H, W, B, N);
  if (rc == CP_ERR_INVALID) return rc;
  if (iterations <= 0 || iterations > PNP_MAX_ITERS) return CP_ERR_INVALID;
  if ((!dist_thresholds && !cp_finite_positive(dist_threshold)) || cp_p3d_stride_invalid(p3d_bstride, N)) return CP_ERR_INVALID;
  if (rc != CP_OK) return rc;
  if (cp_misaligned(p3d, 3) || cp_misaligned(pose, 7) || cp_misaligned(scratch, 7) || cp_misaligned(status, 3) || cp_misaligned(dist_thresholds, 7))
    return CP_ERR_ALIGN;
  if (B == 0) return CP_OK;
  const PdScratch s = pd_scratch(B, N, iterations);
  char* const base = (char*)scratch;
  hipStream_t st = (hipStream_t)stream;
  static CpDeviceOnce once;                  // the solver kernel is sized for PNP_NMAX keypoints, once per device
  const int dev = cp_current_device();
  CP_LDS_ATTR_ONCE(once, dev, cp_set_max_lds((const void*)pose_depth_ransac_kernel, (size_t)PNP_NMAX * PD_LDS_PER_POINT + 16));
  const int lc = pd_launch_lift(st, p2d, valid, valid_stride, cam_K, K_bstride, depth, image_ids, I, H, W, B, N, (float*)(base + s.Q),
                                (uint8_t*)(base + s.lifted), (int32_t*)(base + s.n_lifted));
  if (lc != CP_OK) return lc;
  PdParams p;
  p.p3d = p3d; p.Q = (const float*)(base + s.Q); p.lifted = (const uint8_t*)(base + s.lifted); p.thr_b = dist_thresholds; p.pose = pose;
  p.inliers = inliers; p.status = status; p.hyp = (double*)base; p.steps = (double*)(base + s.steps); p.p3d_bs = p3d_bstride;
  p.thr = dist_threshold; p.B = B; p.N = N; p.iters = iterations; p.seed = seed;
  CP_LAUNCH(pose_depth_ransac_kernel, dim3((unsigned)B), dim3(PNP_THREADS), (size_t)N * PD_LDS_PER_POINT + 16, st, p);
  return cp_check_launch();
}
