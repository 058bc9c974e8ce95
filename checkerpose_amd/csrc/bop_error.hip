// cp_bop_errors: BOP's MSSD, MSPD and projection error of a batch of poses over the object's mesh vertices and
// its symmetry transformations, on the device.  The reference scores one pose at a time on the host
// (bop_toolkit_lib/pose_error.py:96-144 mssd / mspd, :217-232 proj), transforming and projecting the whole mesh once per symmetry.
//
// Arithmetic.  bop_compose_kernel forms, per pose b and symmetry s, in double WITHOUT floating-point contraction
//     R_gs = R_gt R_s,  t_gs = R_gt t_s + t_gt,  D_s = R_est - R_gs,  d_s = t_est - t_gs,  Pg_s = K [R_gs | t_gs]      (24 numbers)
// and per pose  Pe = K [R_est | t_est],  Pgt = K [R_gt | t_gt]  and a validity flag, all rounded to fp32 once.  The hot loop is fp32:
//     MSSD_s = max_v |D_s p_v + d_s|^2      -- linear in the DIFFERENCE of the two poses: the translations (camera depth) never
//                                              meet the vertices, a pose equal to its ground truth has D = 0, d = 0 exactly
//     MSPD_s = max_v |proj(Pe, p_v) - proj(Pg_s, p_v)|^2,   proj(P, p) = (P p_h)_{0,1} * rcp((P p_h)_2)     (no guard on the depth)
// with explicit fma chains (be_affine) shared by both mappings and by the final pass, so a (vertex, symmetry) pair gives the same
// bits wherever it is evaluated.  The maximum is over squared distances; the square root is taken once per (b, s) in double, then
// the minimum over s.  proj sums sqrt((double) d2_v) over the vertices in double in a fixed order (lane-strided partial sums, then
// a tree), as ADD does.  max / min are exact in any order: no output bit depends on the batch, the mapping, the vertex split or
// the kinds asked together.
//
// Launches (at most three).  compose; the main pass in one of two mappings; bop_finish_kernel (one workgroup per pose).
//   small S  bop_small_kernel: a WAVE owns 256 vertices (4 per lane, with their estimate-side projections, in registers) and loops
//            over the pose's symmetries, whose 24 floats sit at a wave-uniform address (hipcc emits six 16-byte VECTOR loads
//            of it, every lane the same address -- not scalar loads); one cross-lane max per symmetry.
//   large S  bop_large_kernel: a lane owns ONE symmetry (24 VGPRs); vertices and their estimate-side projections are staged in LDS
//            in tiles and read as broadcasts; a lane keeps its running max, so the vertex loop has no cross-lane traffic.  The
//            vertex range is split across workgroups.
// Either way the partial maxima go to scratch as (b, split, s) float2 = (MSSD^2, MSPD^2) and the final pass folds the splits that
// the pose's mesh reaches -- no atomics, no initialised scratch.  Smax >= BE_LARGE_S picks the large mapping.
#include "common.h"

namespace {

constexpr int BE_THREADS = 256;                  // compose, small mapping, final pass
constexpr int BE_VPL = 4;                        // small mapping: vertices per lane
constexpr int BE_WSLAB = 64 * BE_VPL;            // ... and per wave (= one split)
constexpr int BE_WAVES = BE_THREADS / 64;
constexpr int BE_LT = 128;                       // large mapping: lanes = symmetries per workgroup (628 = 4.9 x 128, 1256 = 9.8 x 128)
constexpr int BE_VT = 512;                       // large mapping: vertices per LDS tile (10 KiB)
constexpr int BE_TARGET_BLOCKS = 1024;           // large mapping: vertex splits are added until a launch has about this many workgroups
constexpr int BE_LARGE_S = 96;                   // Smax from which the large mapping is taken: the `crossover` table of
                                                 // profiles/bop_error_bench.json (B = 256, V = 4096, both mappings forced)
constexpr int BE_SYM = 24;                       // floats per (b, s): D[9] d[3] Pg[12]
constexpr int BE_POSE = 32;                      // floats per b: Pe[12] Pgt[12] ok[1]

struct BeParams {
  const double* est;
  const double* gt;
  const double* K;
  const float* verts;
  const int32_t* v_off;       // nullptr: one mesh of Vmax vertices
  const double* syms;
  const int32_t* s_off;
  const int32_t* mesh_id;     // nullptr: mesh 0 for every pose
  float* symtab;              // (B, Smax, BE_SYM)
  float* posetab;             // (B, BE_POSE)
  float2* partial;            // (B, nsplit, Smax)
  double* mssd;
  double* mspd;
  double* proj;
  int k_stride, M, B, Vmax, Smax, nsplit, tiles_per_split, stiles, large;
  unsigned kinds;
};

// the pose's mesh and symmetry range; V = 0 marks a pose that cannot be scored (mesh id, mesh size or set size out of range)
__device__ inline void be_pose(const BeParams& p, int b, int& vfirst, int& V, int& sfirst, int& S) {
  vfirst = 0; V = 0; sfirst = 0; S = 0;
  const int m = p.mesh_id ? p.mesh_id[b] : 0;
  if (m < 0 || m >= p.M) return;
  sfirst = p.s_off[m];
  S = p.s_off[m + 1] - sfirst;
  int v = p.Vmax;
  if (p.v_off) {
    vfirst = p.v_off[m];
    v = p.v_off[m + 1] - vfirst;
  }
  if (vfirst < 0 || v <= 0 || v > p.Vmax || sfirst < 0 || S <= 0 || S > p.Smax) return;
  V = v;
}

// row . (x, y, z, 1) of a 3x4 / 3x3+3 fp32 matrix: one fma chain, the same everywhere
__device__ __forceinline__ float be_affine(float a, float b, float c, float d, float x, float y, float z) {
  return fmaf(c, z, fmaf(b, y, fmaf(a, x, d)));
}

__device__ __forceinline__ void be_project(const float* __restrict__ P, float x, float y, float z, float& u, float& v) {
#pragma clang fp contract(off)
  const float pu = be_affine(P[0], P[1], P[2], P[3], x, y, z);
  const float pv = be_affine(P[4], P[5], P[6], P[7], x, y, z);
  const float pw = be_affine(P[8], P[9], P[10], P[11], x, y, z);
  const float iw = __builtin_amdgcn_rcpf(pw);
  u = pu * iw;
  v = pv * iw;
}

__device__ __forceinline__ float be_px2(float u, float v, float ue, float ve) {
#pragma clang fp contract(off)
  const float du = u - ue, dv = v - ve;       // (never fused with the products above: equal projections differ by exactly 0)
  return fmaf(dv, dv, du * du);
}

// one (vertex, symmetry) pair: m = D[9] d[3] Pg[12]
template <bool DS, bool DP>
__device__ __forceinline__ void be_eval(const float* __restrict__ m, float x, float y, float z, float ue, float ve, float& a, float& c) {
#pragma clang fp contract(off)
  if constexpr (DS) {
    const float ex = be_affine(m[0], m[1], m[2], m[9], x, y, z);
    const float ey = be_affine(m[3], m[4], m[5], m[10], x, y, z);
    const float ez = be_affine(m[6], m[7], m[8], m[11], x, y, z);
    a = fmaxf(a, fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
  }
  if constexpr (DP) {
    float u, v;
    be_project(m + 12, x, y, z, u, v);
    c = fmaxf(c, be_px2(u, v, ue, ve));
  }
}

__device__ inline double be_dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
#pragma clang fp contract(off)
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// P = K [R | t] in double -> fp32 (3x4 row-major)
__device__ inline void be_krt(const double* __restrict__ K, const double* R, const double* t, float* __restrict__ P) {
#pragma clang fp contract(off)
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) P[4 * r + c] = (float)be_dot3(K[3 * r], K[3 * r + 1], K[3 * r + 2], R[c], R[3 + c], R[6 + c]);
    P[4 * r + 3] = (float)be_dot3(K[3 * r], K[3 * r + 1], K[3 * r + 2], t[0], t[1], t[2]);
  }
}

__global__ __launch_bounds__(BE_THREADS) void bop_compose_kernel(BeParams p) {
#pragma clang fp contract(off)
  const long long idx = (long long)blockIdx.x * BE_THREADS + threadIdx.x;
  if (idx >= (long long)p.B * p.Smax) return;
  const int b = (int)(idx / p.Smax), s = (int)(idx % p.Smax);
  int vfirst, V, sfirst, S;
  be_pose(p, b, vfirst, V, sfirst, S);
  const double* __restrict__ e = p.est + 12 * (size_t)b;
  const double* __restrict__ g = p.gt + 12 * (size_t)b;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  if (s == 0) {
    float* __restrict__ o = p.posetab + (size_t)b * BE_POSE;
    bool ok = V > 0;
    for (int k = 0; k < 12; ++k) ok = ok && isfinite(e[k]) && isfinite(g[k]);
    for (int k = 0; k < 9; ++k) ok = ok && isfinite(K[k]);
    be_krt(K, e, e + 9, o);
    be_krt(K, g, g + 9, o + 12);
    o[24] = ok ? 1.f : 0.f;
  }
  if (s >= S || V == 0) return;
  const double* __restrict__ y = p.syms + 12 * ((size_t)sfirst + s);
  double Rgs[9], tgs[3];
  for (int a = 0; a < 3; ++a) {
    for (int c = 0; c < 3; ++c) Rgs[3 * a + c] = be_dot3(g[3 * a], g[3 * a + 1], g[3 * a + 2], y[c], y[3 + c], y[6 + c]);
    tgs[a] = be_dot3(g[3 * a], g[3 * a + 1], g[3 * a + 2], y[9], y[10], y[11]) + g[9 + a];
  }
  float* __restrict__ o = p.symtab + ((size_t)b * p.Smax + s) * BE_SYM;
  for (int k = 0; k < 9; ++k) o[k] = (float)(e[k] - Rgs[k]);
  for (int k = 0; k < 3; ++k) o[9 + k] = (float)(e[9 + k] - tgs[k]);
  be_krt(K, Rgs, tgs, o + 12);
}

template <bool DS, bool DP>
__global__ __launch_bounds__(BE_THREADS) void bop_small_kernel(BeParams p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bpp = p.nsplit / BE_WAVES;                               // workgroups per pose
  const int b = blockIdx.x / bpp;
  const int split = (blockIdx.x % bpp) * BE_WAVES + wave;
  int vfirst, V, sfirst, S;
  be_pose(p, b, vfirst, V, sfirst, S);
  const int v0 = split * BE_WSLAB;
  if (v0 >= V) return;                                               // (wave-uniform: V = 0 leaves too; no barrier in this kernel)
  const float* __restrict__ vt = p.verts + 3 * (size_t)vfirst;
  const float* __restrict__ pe = p.posetab + (size_t)b * BE_POSE;
  float x[BE_VPL], y[BE_VPL], z[BE_VPL], ue[BE_VPL], ve[BE_VPL];
#pragma unroll
  for (int k = 0; k < BE_VPL; ++k) {
    const int i = min(v0 + k * 64 + lane, V - 1);                    // tail lanes repeat the last vertex: the max does not change
    x[k] = vt[3 * i]; y[k] = vt[3 * i + 1]; z[k] = vt[3 * i + 2];
    ue[k] = 0.f; ve[k] = 0.f;
    if constexpr (DP) be_project(pe, x[k], y[k], z[k], ue[k], ve[k]);
  }
  float2* __restrict__ out = p.partial + ((size_t)b * p.nsplit + split) * p.Smax;
  const float* __restrict__ tab = p.symtab + (size_t)b * p.Smax * BE_SYM;
  for (int s = 0; s < S; ++s) {
    const float* __restrict__ m = tab + (size_t)s * BE_SYM;          // wave-uniform address
    float a = 0.f, c = 0.f;
#pragma unroll
    for (int k = 0; k < BE_VPL; ++k) be_eval<DS, DP>(m, x[k], y[k], z[k], ue[k], ve[k], a, c);
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
      if constexpr (DS) a = fmaxf(a, __shfl_xor(a, w, 64));
      if constexpr (DP) c = fmaxf(c, __shfl_xor(c, w, 64));
    }
    if (lane == 0) out[s] = make_float2(a, c);
  }
}

template <bool DS, bool DP>
__global__ __launch_bounds__(BE_LT) void bop_large_kernel(BeParams p) {
  __shared__ float4 s_v[BE_VT];                                      // x y z u_est
  __shared__ float s_ve[BE_VT];                                      // v_est
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int st = blk % p.stiles;
  blk /= p.stiles;
  const int split = blk % p.nsplit, b = blk / p.nsplit;
  int vfirst, V, sfirst, S;
  be_pose(p, b, vfirst, V, sfirst, S);
  const int v_begin = split * p.tiles_per_split * BE_VT;
  if (v_begin >= V || st * BE_LT >= S) return;                       // (uniform: V = 0 leaves too)
  const int v_end = min(V, v_begin + p.tiles_per_split * BE_VT);
  const float* __restrict__ vt = p.verts + 3 * (size_t)vfirst;
  const float* __restrict__ pe = p.posetab + (size_t)b * BE_POSE;
  const int s = st * BE_LT + tid;
  float m[BE_SYM];
  {
    const f32x4* __restrict__ src = (const f32x4*)(p.symtab + ((size_t)b * p.Smax + min(s, S - 1)) * BE_SYM);
#pragma unroll
    for (int k = 0; k < BE_SYM / 4; ++k) {
      const f32x4 q = src[k];
      m[4 * k] = q.x; m[4 * k + 1] = q.y; m[4 * k + 2] = q.z; m[4 * k + 3] = q.w;
    }
  }
  float a = 0.f, c = 0.f;
  for (int t0 = v_begin; t0 < v_end; t0 += BE_VT) {
    const int n = min(BE_VT, v_end - t0);
    __syncthreads();
    for (int j = tid; j < n; j += BE_LT) {
      const int i = t0 + j;
      const float x = vt[3 * i], y = vt[3 * i + 1], z = vt[3 * i + 2];
      float u = 0.f, v = 0.f;
      if constexpr (DP) be_project(pe, x, y, z, u, v);
      s_v[j] = make_float4(x, y, z, u);
      s_ve[j] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
      const float4 q = s_v[j];                                       // every lane reads the same address: a broadcast
      be_eval<DS, DP>(m, q.x, q.y, q.z, q.w, s_ve[j], a, c);
    }
  }
  if (s < S) p.partial[((size_t)b * p.nsplit + split) * p.Smax + s] = make_float2(a, c);
}

__global__ __launch_bounds__(BE_THREADS) void bop_finish_kernel(BeParams p) {
  __shared__ double s_red[3][BE_THREADS];
  const int tid = threadIdx.x, b = blockIdx.x;
  int vfirst, V, sfirst, S;
  be_pose(p, b, vfirst, V, sfirst, S);
  const float* __restrict__ pe = p.posetab + (size_t)b * BE_POSE;
  const bool ok = V > 0 && pe[24] != 0.f;
  double ms = __builtin_inf(), mp = __builtin_inf(), sum = 0.0;
  if (ok && (p.kinds & (CP_BOP_ERR_MSSD | CP_BOP_ERR_MSPD))) {
    // the splits this pose's mesh reaches (the others were never written)
    const int reach = p.large ? ((V + BE_VT - 1) / BE_VT + p.tiles_per_split - 1) / p.tiles_per_split : (V + BE_WSLAB - 1) / BE_WSLAB;
    const float2* __restrict__ part = p.partial + (size_t)b * p.nsplit * p.Smax;
    for (int s = tid; s < S; s += BE_THREADS) {
      float a = 0.f, c = 0.f;
      for (int k = 0; k < reach; ++k) {
        const float2 q = part[(size_t)k * p.Smax + s];
        a = fmaxf(a, q.x);
        c = fmaxf(c, q.y);
      }
      ms = fmin(ms, sqrt((double)a));
      mp = fmin(mp, sqrt((double)c));
    }
  }
  if (ok && (p.kinds & CP_BOP_ERR_PROJ)) {
    const float* __restrict__ vt = p.verts + 3 * (size_t)vfirst;
    for (int i = tid; i < V; i += BE_THREADS) {
      const float x = vt[3 * i], y = vt[3 * i + 1], z = vt[3 * i + 2];
      float ue, ve, ug, vg;
      be_project(pe, x, y, z, ue, ve);
      be_project(pe + 12, x, y, z, ug, vg);
      sum += sqrt((double)be_px2(ug, vg, ue, ve));
    }
  }
  s_red[0][tid] = ms;
  s_red[1][tid] = mp;
  s_red[2][tid] = sum;
  __syncthreads();
  for (int w = BE_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) {
      s_red[0][tid] = fmin(s_red[0][tid], s_red[0][tid + w]);
      s_red[1][tid] = fmin(s_red[1][tid], s_red[1][tid + w]);
      s_red[2][tid] += s_red[2][tid + w];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double nan = __builtin_nan("");
    if (p.kinds & CP_BOP_ERR_MSSD) p.mssd[b] = ok ? s_red[0][0] : nan;
    if (p.kinds & CP_BOP_ERR_MSPD) p.mspd[b] = ok ? s_red[1][0] : nan;
    if (p.kinds & CP_BOP_ERR_PROJ) p.proj[b] = ok ? s_red[2][0] / (double)V : nan;
  }
}

// the split plan of a launch: a function of (B, Smax, Vmax, mapping) alone, so the scratch size query and the launch agree
struct BePlan { int large, nsplit, tiles_per_split, stiles; };
BePlan be_plan(int B, int Smax, int Vmax, unsigned map) {
  BePlan pl;
  pl.large = map == CP_BOP_MAP_LARGE || (map != CP_BOP_MAP_SMALL && Smax >= BE_LARGE_S);
  if (!pl.large) {
    pl.nsplit = (Vmax + BE_WSLAB * BE_WAVES - 1) / (BE_WSLAB * BE_WAVES) * BE_WAVES;
    pl.tiles_per_split = 1;
    pl.stiles = 1;
    return pl;
  }
  pl.stiles = (Smax + BE_LT - 1) / BE_LT;
  const int vtiles = (Vmax + BE_VT - 1) / BE_VT;
  const long long base = (long long)B * pl.stiles;
  long long want = (BE_TARGET_BLOCKS + base - 1) / base;
  if (want < 1) want = 1;
  if (want > vtiles) want = vtiles;
  pl.tiles_per_split = (int)((vtiles + want - 1) / want);
  pl.nsplit = (vtiles + pl.tiles_per_split - 1) / pl.tiles_per_split;
  return pl;
}

size_t be_scratch_bytes(int B, int Smax, int Vmax, unsigned map) {
  if (B <= 0 || Smax < 1 || Vmax <= 0) return 0;
  const BePlan pl = be_plan(B, Smax, Vmax, map);
  return ((size_t)B * Smax * BE_SYM + (size_t)B * BE_POSE) * sizeof(float) + (size_t)B * pl.nsplit * Smax * sizeof(float2);
}

}  // namespace

extern "C" size_t cp_bop_errors_scratch_bytes(int B, int Smax, int Vmax) { return be_scratch_bytes(B, Smax, Vmax, 0); }

extern "C" size_t cp_bop_errors_map_scratch_bytes(int B, int Smax, int Vmax, unsigned map) {
  if (map != 0 && map != CP_BOP_MAP_SMALL && map != CP_BOP_MAP_LARGE) return 0;
  return be_scratch_bytes(B, Smax, Vmax, map);
}

extern "C" int cp_bop_errors(cp_stream_t stream, const double* pose_est, const double* pose_gt, const double* cam_K, int k_stride,
                             const float* verts, const int32_t* v_offsets, const double* syms, const int32_t* s_offsets, int M,
                             const int32_t* mesh_ids, int B, int Vmax, int Smax, unsigned kinds, double* mssd, double* mspd,
                             double* proj, void* scratch) {
  const unsigned all = CP_BOP_ERR_MSSD | CP_BOP_ERR_MSPD | CP_BOP_ERR_PROJ;
  const unsigned map = kinds & (CP_BOP_MAP_SMALL | CP_BOP_MAP_LARGE);
  if (!pose_est || !pose_gt || !cam_K || !verts || !syms || !s_offsets || !scratch) return CP_ERR_INVALID;
  if (!(kinds & all) || (kinds & ~(all | CP_BOP_MAP_SMALL | CP_BOP_MAP_LARGE)) || map == (CP_BOP_MAP_SMALL | CP_BOP_MAP_LARGE))
    return CP_ERR_INVALID;
  if (((kinds & CP_BOP_ERR_MSSD) && !mssd) || ((kinds & CP_BOP_ERR_MSPD) && !mspd) || ((kinds & CP_BOP_ERR_PROJ) && !proj))
    return CP_ERR_INVALID;
  if (B <= 0 || M <= 0 || Vmax <= 0 || Smax < 1 || (k_stride != 0 && k_stride != 9)) return CP_ERR_INVALID;
  if ((!mesh_ids || !v_offsets) && M != 1) return CP_ERR_INVALID;
  if (((uintptr_t)scratch & 15) || ((uintptr_t)pose_est & 7) || ((uintptr_t)pose_gt & 7) || ((uintptr_t)cam_K & 7) ||
      ((uintptr_t)syms & 7) || ((uintptr_t)mssd & 7) || ((uintptr_t)mspd & 7) || ((uintptr_t)proj & 7) || ((uintptr_t)verts & 3) ||
      ((uintptr_t)v_offsets & 3) || ((uintptr_t)s_offsets & 3) || ((uintptr_t)mesh_ids & 3))
    return CP_ERR_ALIGN;
  const BePlan pl = be_plan(B, Smax, Vmax, map);
  BeParams p;
  p.est = pose_est; p.gt = pose_gt; p.K = cam_K; p.verts = verts; p.v_off = v_offsets; p.syms = syms; p.s_off = s_offsets;
  p.mesh_id = mesh_ids; p.mssd = mssd; p.mspd = mspd; p.proj = proj; p.k_stride = k_stride; p.M = M; p.B = B; p.Vmax = Vmax;
  p.Smax = Smax; p.nsplit = pl.nsplit; p.tiles_per_split = pl.tiles_per_split; p.stiles = pl.stiles; p.large = pl.large;
  p.kinds = kinds & all;
  p.symtab = (float*)scratch;
  p.posetab = p.symtab + (size_t)B * Smax * BE_SYM;
  p.partial = (float2*)(p.posetab + (size_t)B * BE_POSE);
  const long long compose_blocks = ((long long)B * Smax + BE_THREADS - 1) / BE_THREADS;
  const long long main_blocks = pl.large ? (long long)B * pl.nsplit * pl.stiles : (long long)B * (pl.nsplit / BE_WAVES);
  // (a launch holds at most 2^32 - 1 threads: 2^24 - 1 workgroups of BE_THREADS)
  if (compose_blocks >= (1LL << 24) || main_blocks >= (1LL << 24) || B >= (1 << 24)) return CP_ERR_RANGE;
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(bop_compose_kernel, dim3((unsigned)compose_blocks), dim3(BE_THREADS), 0, st, p);
  const bool ds = p.kinds & CP_BOP_ERR_MSSD, dp = p.kinds & CP_BOP_ERR_MSPD;
  const dim3 grid((unsigned)main_blocks);
  if (pl.large) {
    if (ds && dp) CP_LAUNCH((bop_large_kernel<true, true>), grid, dim3(BE_LT), 0, st, p);
    else if (ds) CP_LAUNCH((bop_large_kernel<true, false>), grid, dim3(BE_LT), 0, st, p);
    else if (dp) CP_LAUNCH((bop_large_kernel<false, true>), grid, dim3(BE_LT), 0, st, p);
  } else {
    if (ds && dp) CP_LAUNCH((bop_small_kernel<true, true>), grid, dim3(BE_THREADS), 0, st, p);
    else if (ds) CP_LAUNCH((bop_small_kernel<true, false>), grid, dim3(BE_THREADS), 0, st, p);
    else if (dp) CP_LAUNCH((bop_small_kernel<false, true>), grid, dim3(BE_THREADS), 0, st, p);
  }
  CP_LAUNCH(bop_finish_kernel, dim3((unsigned)B), dim3(BE_THREADS), 0, st, p);
  return cp_check_launch();
}
