// cp_pose_errors: ADD / ADD-S (ADI) of a batch of poses over the object's mesh vertices, on the device.
// The reference scores one pose at a time on the host (metric.py:8-18 -> bop_toolkit_lib.pose_error.add / .adi :147-184, a cKDTree per
// pose); here the poses cp_pnp_ransac wrote go straight to the metric.
//
// Arithmetic.  Per pose the relative pose is formed in double,
//     Rr = I + R_est^T (R_gt - R_est)  (= R_est^T R_gt for an orthonormal R_est; exactly I for equal poses),   tr = R_est^T (t_gt - t_est),
// rounded to fp32, and everything per vertex runs in fp32 in the MODEL frame: q_i = Rr p_i + tr,
//     ADD = mean_i |q_i - p_i|,      ADI = mean_i min_j |q_i - p_j|
// -- the reference's definition after the rigid change of frame R_est^T (. - t_est), which keeps coordinates at the size of the model
// plus the pose error instead of at camera depth.  Distances are direct differences (3 sub, 1 mul, 2 fma, 1 min per pair): the
// |q|^2 + |p|^2 - 2 q.p expansion would lose exactly the low bits the metric is made of.  One square root per query, after the min.
// Both errors use the same q_i and the same distance expression, and j = i is among the candidates, so ADI <= ADD holds exactly.
//
// Launches.  adi_min_kernel: workgroup = (pose, tile of PE_QTILE queries, candidate split); a lane keeps PE_QPL queries in registers,
// the candidates stream through LDS in tiles of PE_CT vertices padded to 4 floats, every lane reads the same candidate address (a
// broadcast).  It writes min_j |q_i - p_j|^2 per query and split.  pose_error_finish_kernel: one workgroup per pose takes the min
// over the splits, the square roots, ADD's distances, and both means in double in a fixed order (lane-strided partial sums, then a
// tree over the lanes) -- no atomics; min is exact in any order, so neither B nor the split count can change a bit of the result.
#include "common.h"

namespace {

constexpr int PE_THREADS = 256;
constexpr int PE_QPL = 4;                        // queries per lane: each candidate read from LDS serves 4 pairs
constexpr int PE_QTILE = PE_THREADS * PE_QPL;    // queries per workgroup
constexpr int PE_CT = 2048;                      // candidates per LDS tile (32 KiB as float4)
constexpr int PE_TARGET_BLOCKS = 1024;           // candidate splits are added until a launch has about this many workgroups

struct PeParams {
  const double* est;
  const double* gt;
  const float* verts;
  const int32_t* offsets;     // nullptr: one mesh of Vmax vertices
  const int32_t* mesh_id;     // nullptr: mesh 0 for every pose
  float* mind2;               // (B, S, Vmax)
  double* add;
  double* adi;
  int M, B, Vmax, S, tiles_per_split, qtiles, kinds;
};

struct RelPose { float r[9]; float t[3]; };

// relative pose in double, then fp32; explicit fma()s so that both kernels round identically
__device__ inline RelPose rel_pose(const double* __restrict__ e, const double* __restrict__ g) {
  RelPose o;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) {
      double s = e[0 + a] * (g[0 + b] - e[0 + b]);
      s = fma(e[3 + a], g[3 + b] - e[3 + b], s);
      s = fma(e[6 + a], g[6 + b] - e[6 + b], s);
      o.r[3 * a + b] = (float)((a == b ? 1.0 : 0.0) + s);
    }
    double s = e[0 + a] * (g[9] - e[9]);
    s = fma(e[3 + a], g[10] - e[10], s);
    s = fma(e[6 + a], g[11] - e[11], s);
    o.t[a] = (float)s;
  }
  return o;
}

__device__ inline void xform(const RelPose& rp, float x, float y, float z, float& qx, float& qy, float& qz) {
  qx = fmaf(rp.r[2], z, fmaf(rp.r[1], y, fmaf(rp.r[0], x, rp.t[0])));
  qy = fmaf(rp.r[5], z, fmaf(rp.r[4], y, fmaf(rp.r[3], x, rp.t[1])));
  qz = fmaf(rp.r[8], z, fmaf(rp.r[7], y, fmaf(rp.r[6], x, rp.t[2])));
}

__device__ inline float dist2(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// the pose's mesh: first vertex and vertex count; V = 0 marks a pose that cannot be scored (mesh id / size out of range)
__device__ inline void pose_mesh(const PeParams& p, int b, int& first, int& V) {
  first = 0;
  V = p.Vmax;
  if (p.offsets) {
    const int m = p.mesh_id ? p.mesh_id[b] : 0;
    if (m < 0 || m >= p.M) { V = 0; return; }
    first = p.offsets[m];
    V = p.offsets[m + 1] - first;
    if (first < 0 || V <= 0 || V > p.Vmax) V = 0;
  }
}

__global__ __launch_bounds__(PE_THREADS) void adi_min_kernel(PeParams p) {
  __shared__ float4 s_c[PE_CT];
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int qt = blk % p.qtiles;
  blk /= p.qtiles;
  const int s = blk % p.S, b = blk / p.S;
  int first, V;
  pose_mesh(p, b, first, V);
  const int q0 = qt * PE_QTILE;
  if (q0 >= V) return;                                             // (uniform: V = 0 leaves too)
  const float* __restrict__ vt = p.verts + 3 * (size_t)first;
  const RelPose rp = rel_pose(p.est + 12 * (size_t)b, p.gt + 12 * (size_t)b);
  float qx[PE_QPL], qy[PE_QPL], qz[PE_QPL], best[PE_QPL];
#pragma unroll
  for (int k = 0; k < PE_QPL; ++k) {
    const int i = min(q0 + k * PE_THREADS + tid, V - 1);           // tail lanes repeat the last vertex and store nothing
    xform(rp, vt[3 * i], vt[3 * i + 1], vt[3 * i + 2], qx[k], qy[k], qz[k]);
    best[k] = __builtin_inff();
  }
  const int c_begin = s * p.tiles_per_split * PE_CT;
  const int c_end = min(V, c_begin + p.tiles_per_split * PE_CT);   // empty for a small mesh's later splits: best stays +inf
  for (int c0 = c_begin; c0 < c_end; c0 += PE_CT) {
    const int n = min(PE_CT, c_end - c0);
    const int n4 = (n + 3) & ~3;
    __syncthreads();
    for (int j = tid; j < n4; j += PE_THREADS) {                   // the tail of the last group of 4 repeats a real candidate
      const int v = c0 + min(j, n - 1);
      s_c[j] = make_float4(vt[3 * v], vt[3 * v + 1], vt[3 * v + 2], 0.f);
    }
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < n4; j += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 c = s_c[j + u];
#pragma unroll
        for (int k = 0; k < PE_QPL; ++k) best[k] = fminf(best[k], dist2(qx[k], qy[k], qz[k], c.x, c.y, c.z));
      }
    }
  }
  float* __restrict__ out = p.mind2 + ((size_t)b * p.S + s) * p.Vmax;
#pragma unroll
  for (int k = 0; k < PE_QPL; ++k) {
    const int i = q0 + k * PE_THREADS + tid;
    if (i < V) out[i] = best[k];
  }
}

__global__ __launch_bounds__(PE_THREADS) void pose_error_finish_kernel(PeParams p) {
  __shared__ double s_sum[2][PE_THREADS];
  const int tid = threadIdx.x, b = blockIdx.x;
  int first, V;
  pose_mesh(p, b, first, V);
  const float* __restrict__ vt = p.verts + 3 * (size_t)first;
  const RelPose rp = rel_pose(p.est + 12 * (size_t)b, p.gt + 12 * (size_t)b);
  const float* __restrict__ m2 = p.mind2 + (size_t)b * p.S * p.Vmax;
  double sa = 0.0, si = 0.0;
  for (int i = tid; i < V; i += PE_THREADS) {
    if (p.kinds & 1) {
      const float x = vt[3 * i], y = vt[3 * i + 1], z = vt[3 * i + 2];
      float qx, qy, qz;
      xform(rp, x, y, z, qx, qy, qz);
      sa += sqrt((double)dist2(qx, qy, qz, x, y, z));
    }
    if (p.kinds & 2) {
      float m = m2[i];
      for (int s = 1; s < p.S; ++s) m = fminf(m, m2[(size_t)s * p.Vmax + i]);
      si += sqrt((double)m);
    }
  }
  s_sum[0][tid] = sa;
  s_sum[1][tid] = si;
  __syncthreads();
  for (int w = PE_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      s_sum[0][tid] += s_sum[0][tid + w];
      s_sum[1][tid] += s_sum[1][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double nan = __builtin_nan("");
    bool ok = V > 0;                                               // a pose with a NaN / inf entry scores NaN in BOTH errors (min() alone
    for (int k = 0; k < 9; ++k) ok = ok && isfinite(rp.r[k]);      // would drop the NaN and leave ADI at +inf)
    for (int k = 0; k < 3; ++k) ok = ok && isfinite(rp.t[k]);
    if (p.kinds & 1) p.add[b] = ok ? s_sum[0][0] / (double)V : nan;
    if (p.kinds & 2) p.adi[b] = ok ? s_sum[1][0] / (double)V : nan;
  }
}

// candidate splits of a launch: a function of (B, Vmax) alone, so the scratch size query and the launch agree
void pe_plan(int B, int Vmax, int& qtiles, int& S, int& tiles_per_split) {
  qtiles = (Vmax + PE_QTILE - 1) / PE_QTILE;
  const int ctiles = (Vmax + PE_CT - 1) / PE_CT;
  const long long base = (long long)B * qtiles;
  long long want = (PE_TARGET_BLOCKS + base - 1) / base;
  if (want < 1) want = 1;
  if (want > ctiles) want = ctiles;
  tiles_per_split = (int)((ctiles + want - 1) / want);
  S = (ctiles + tiles_per_split - 1) / tiles_per_split;
}

}  // namespace

extern "C" size_t cp_pose_errors_scratch_bytes(int B, int Vmax) {
  if (B <= 0 || Vmax <= 0) return 0;
  int qtiles, S, tps;
  pe_plan(B, Vmax, qtiles, S, tps);
  return (size_t)B * S * Vmax * sizeof(float);
}

extern "C" int cp_pose_errors(cp_stream_t stream, const double* pose_est, const double* pose_gt, const float* verts,
                              const int32_t* offsets, int M, const int32_t* mesh_id, int B, int Vmax, int kinds, double* add,
                              double* adi, void* scratch) {
  if (!pose_est || !pose_gt || !verts) return CP_ERR_INVALID;
  if (kinds <= 0 || (kinds & ~(CP_POSE_ERR_ADD | CP_POSE_ERR_ADI))) return CP_ERR_INVALID;
  if (((kinds & CP_POSE_ERR_ADD) && !add) || ((kinds & CP_POSE_ERR_ADI) && (!adi || !scratch))) return CP_ERR_INVALID;
  if (mesh_id && !offsets) return CP_ERR_INVALID;
  if (B <= 0 || Vmax <= 0 || (offsets && M <= 0)) return CP_ERR_INVALID;
  if (((uintptr_t)verts & 15) || ((uintptr_t)scratch & 15) || ((uintptr_t)pose_est & 7) || ((uintptr_t)pose_gt & 7) ||
      ((uintptr_t)add & 7) || ((uintptr_t)adi & 7) || ((uintptr_t)offsets & 3) || ((uintptr_t)mesh_id & 3))
    return CP_ERR_ALIGN;
  PeParams p;
  p.est = pose_est; p.gt = pose_gt; p.verts = verts; p.offsets = offsets; p.mesh_id = mesh_id; p.mind2 = (float*)scratch;
  p.add = add; p.adi = adi; p.M = M; p.B = B; p.Vmax = Vmax; p.kinds = kinds;
  pe_plan(B, Vmax, p.qtiles, p.S, p.tiles_per_split);
  const long long blocks = (long long)B * p.S * p.qtiles;
  // (a launch holds at most 2^32 - 1 threads: 2^24 - 1 workgroups of PE_THREADS)
  if (blocks * PE_THREADS > 0xFFFFFFFFLL || (long long)B * p.S * Vmax >= (1LL << 40)) return CP_ERR_RANGE;
  hipStream_t st = (hipStream_t)stream;
  if (kinds & CP_POSE_ERR_ADI) CP_LAUNCH(adi_min_kernel, dim3((unsigned)blocks), dim3(PE_THREADS), 0, st, p);
  CP_LAUNCH(pose_error_finish_kernel, dim3((unsigned)B), dim3(PE_THREADS), 0, st, p);
  return cp_check_launch();
}
