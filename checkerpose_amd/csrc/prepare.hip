// Object preparation on the device: what every other row starts from -- an object's farthest-point keypoints
// (reference preprocess_data/get_fps_points.py:65-90 farthest_point_sample_init_center, the maker of fps_202212/obj_*.pkl) and its
// exact diameter (bop_toolkit_lib/misc.py:279-293 calc_pts_diameter, the `diameter` of models_info.json).
//
// Everything is fp64 and this whole file is compiled with `#pragma clang fp contract(off)` (hipcc's default is -ffp-contract=fast):
// no product is fused into a following sum, square roots are the correctly rounded ones, so every value is numpy's bit for bit.
//
// cp_fps.  The reference's rule, per cloud: start = (max + min) / 2 of the bounding box (NOT a vertex), every dist starts at
// (1.0 * sqrt((dx*dx + dy*dy) + dz*dz)) * 10 of the box extents; per sample d = sqrt((ex*ex + ey*ey) + ez*ez) with e = p - farthest
// (numpy's norm(axis=1), unfused), `if d < dist: dist = d`, the next sample = the FIRST index of the largest dist.  The ROOTS are
// compared, not the squares: two different sums of squares can round to one root, and then the lower index wins.
// Launches: fps_bbox_kernel (one workgroup per cloud: box, centre, initial distance), then ONE fps_step_kernel launch per sample on
// a grid of (G slices, M clouds) and a last one that only collects.  A step launch first reduces, redundantly in every workgroup,
// the G (value, index) partials the launch before it left -- larger value wins, on equal value the smaller index: an exact,
// order-free rule -- workgroup 0 of the cloud records that sample, then every workgroup updates its own slice of dist and leaves
// its slice's partial in the other half of a double buffer (a neighbour may still be reading this launch's input half).  The
// stream's order between launches is the only synchronisation: no workgroup waits for another, no atomics, no cooperative launch.
// Neither G nor M nor a repeated call can change a bit.  Step 0 takes the initial distance instead of reading dist: no fill pass.
//
// cp_pts_diameter.  max over all pairs of ((dx*dx + dy*dy) + dz*dz), one square root at the end: max is exact in any order and
// (p_i - p_j)^2 = (p_j - p_i)^2 bitwise, so the upper triangle of 1024 x 1024 tile pairs is enough.  pts_diameter_kernel: workgroup =
// (tile pair, cloud), adi_min_kernel's shape in fp64 -- a lane keeps DM_QPL queries in registers, the candidate tile sits in LDS
// padded to 4 doubles and every lane reads the same address (a broadcast).  Per-workgroup maxima go to scratch,
// pts_diameter_finish_kernel (one workgroup per cloud) takes their max and the root.
#include <limits.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_WAVES = PR_THREADS / 64;
constexpr int FPS_MAX_SLICES = PR_THREADS;       // the redundant reduction reads one partial per lane
constexpr int FPS_SLICE_POINTS = 512;            // points per slice the automatic choice aims at (two per lane)
constexpr int FPS_TARGET_BLOCKS = 2048;          // ... while a step launch stays at about this many workgroups
constexpr int DM_QPL = 4;                        // queries per lane: each candidate read from LDS serves 4 pairs
constexpr int DM_TILE = PR_THREADS * DM_QPL;     // 1024 queries x 1024 candidates per workgroup
constexpr int DM_MAX_TILES = 5792;               // T (T + 1) / 2 < 2^24 workgroups

struct FpsParams {
  const double* pts;          // (sumV,3)
  const int32_t* offsets;     // (M+1)
  double* dist;               // (sumV)
  double* head;               // (M,4): the box centre and the initial distance
  double* pval;               // (2,M,G) partial maxima ...
  int32_t* pidx;              // (2,M,G) ... and their first indices
  int32_t* ids;               // (M,npoint)
  double* xyz;                // (M,npoint,3)
  int M, G, npoint, step;
};

struct DiamParams {
  const double* pts;
  const int32_t* offsets;
  double* part;               // (M,Pmax) per-workgroup maxima of the squared distance
  double* out;                // (M)
  int M, Pmax;
};

// the order of the argmax: the larger value, on equal values the smaller index (np.argmax's first index)
__device__ inline void take(double& bv, int& bi, double v, int i) {
  if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// argmax over the workgroup, the result in every lane; s_v / s_i: PR_WAVES entries that no other reduction of the launch uses
__device__ inline void wg_argmax(double& bv, int& bi, double* s_v, int* s_i) {
  for (int w = 32; w > 0; w >>= 1) {
    const double ov = __shfl_xor(bv, w, 64);
    const int oi = __shfl_xor(bi, w, 64);
    take(bv, bi, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = bv; s_i[threadIdx.x >> 6] = bi; }
  __syncthreads();
  bv = s_v[0]; bi = s_i[0];
  for (int w = 1; w < PR_WAVES; ++w) take(bv, bi, s_v[w], s_i[w]);
}

__device__ inline double wg_max(double v, double* s_v) {
  for (int w = 32; w > 0; w >>= 1) v = fmax(v, __shfl_xor(v, w, 64));
  if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = v;
  __syncthreads();
  v = s_v[0];
  for (int w = 1; w < PR_WAVES; ++w) v = fmax(v, s_v[w]);
  return v;
}

__global__ __launch_bounds__(PR_THREADS) void fps_bbox_kernel(FpsParams p) {
  __shared__ double s_r[6][PR_WAVES];
  const int tid = threadIdx.x, m = blockIdx.x;
  const int first = p.offsets[m], V = p.offsets[m + 1] - first;
  const double* __restrict__ pt = p.pts + 3 * (size_t)first;
  const double inf = __builtin_inf();
  double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (int i = tid; i < V; i += PR_THREADS) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double c = pt[3 * (size_t)i + a];
      lo[a] = fmin(lo[a], c);
      hi[a] = fmax(hi[a], c);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = -wg_max(-lo[a], s_r[a]);
    hi[a] = wg_max(hi[a], s_r[3 + a]);
  }
  if (tid == 0) {
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    double* h = p.head + 4 * (size_t)m;
#pragma unroll
    for (int a = 0; a < 3; ++a) h[a] = (hi[a] + lo[a]) / 2;
    h[3] = (1.0 * sqrt((dx * dx + dy * dy) + dz * dz)) * 10;
  }
}

__global__ __launch_bounds__(PR_THREADS) void fps_step_kernel(FpsParams p) {
  __shared__ double s_v[2][PR_WAVES];
  __shared__ int s_i[2][PR_WAVES];
  const int tid = threadIdx.x, g = blockIdx.x, m = blockIdx.y, s = p.step;
  const int first = p.offsets[m], V = p.offsets[m + 1] - first;
  const double* __restrict__ pt = p.pts + 3 * (size_t)first;
  const double* __restrict__ h = p.head + 4 * (size_t)m;
  double fx, fy, fz;
  if (s == 0) {
    fx = h[0]; fy = h[1]; fz = h[2];
  } else {                                                       // the sample the launch before this one chose
    const size_t pb = ((size_t)((s - 1) & 1) * p.M + m) * p.G;
    double bv = -1.0;
    int bi = INT_MAX;
    if (tid < p.G) { bv = p.pval[pb + tid]; bi = p.pidx[pb + tid]; }
    wg_argmax(bv, bi, s_v[0], s_i[0]);
    if (bi < 0 || bi >= V) bi = 0;                               // (cannot happen with finite coordinates; keeps every read in bounds)
    fx = pt[3 * (size_t)bi]; fy = pt[3 * (size_t)bi + 1]; fz = pt[3 * (size_t)bi + 2];
    if (g == 0 && tid == 0) {
      const size_t o = (size_t)m * p.npoint + (s - 1);
      p.ids[o] = bi;
      p.xyz[3 * o] = fx; p.xyz[3 * o + 1] = fy; p.xyz[3 * o + 2] = fz;
    }
  }
  if (s == p.npoint) return;                                     // the collecting launch
  const int len = (V + p.G - 1) / p.G;
  const long long i0 = (long long)g * len;
  const int i1 = (int)min((long long)V, i0 + len);
  double* __restrict__ dist = p.dist + first;
  const double init = h[3];
  double bv = -1.0;                                              // an empty slice's partial: below every distance, never chosen
  int bi = INT_MAX;
  for (long long il = i0 + tid; il < i1; il += PR_THREADS) {
    const int i = (int)il;
    const double ex = pt[3 * (size_t)i] - fx, ey = pt[3 * (size_t)i + 1] - fy, ez = pt[3 * (size_t)i + 2] - fz;
    const double d = sqrt((ex * ex + ey * ey) + ez * ez);
    double cur = s == 0 ? init : dist[i];
    if (d < cur || s == 0) {
      if (d < cur) cur = d;
      dist[i] = cur;
    }
    if (cur > bv) { bv = cur; bi = i; }                          // a lane's indices rise: the first of equal values stays
  }
  wg_argmax(bv, bi, s_v[1], s_i[1]);
  if (tid == 0) {
    const size_t pb = ((size_t)(s & 1) * p.M + m) * p.G + g;
    p.pval[pb] = bv;
    p.pidx[pb] = bi;
  }
}

struct __attribute__((aligned(32))) DmPoint { double x, y, z, pad; };

__global__ __launch_bounds__(PR_THREADS) void pts_diameter_kernel(DiamParams p) {
  __shared__ DmPoint s_c[DM_TILE];
  __shared__ double s_r[PR_WAVES];
  const int tid = threadIdx.x, m = blockIdx.y;
  const int first = p.offsets[m], V = p.offsets[m + 1] - first;
  const int T = (V + DM_TILE - 1) / DM_TILE;
  int rest = blockIdx.x, ti = 0;
  if (rest >= T * (T + 1) / 2) return;                           // (uniform) a smaller cloud of the batch has fewer tile pairs
  while (rest >= T - ti) { rest -= T - ti; ++ti; }               // row ti of the upper triangle holds the pairs (ti, ti .. T-1)
  const int tj = ti + rest;
  const double* __restrict__ pt = p.pts + 3 * (size_t)first;
  double qx[DM_QPL], qy[DM_QPL], qz[DM_QPL], best[DM_QPL];
#pragma unroll
  for (int k = 0; k < DM_QPL; ++k) {
    const int i = min(ti * DM_TILE + k * PR_THREADS + tid, V - 1);         // tail lanes repeat the last vertex: the max cannot change
    qx[k] = pt[3 * (size_t)i]; qy[k] = pt[3 * (size_t)i + 1]; qz[k] = pt[3 * (size_t)i + 2];
    best[k] = 0.0;
  }
  const int c0 = tj * DM_TILE;
  const int n = min(DM_TILE, V - c0);
  const int n4 = (n + 3) & ~3;
  for (int j = tid; j < n4; j += PR_THREADS) {                   // the tail of the last group of 4 repeats a real candidate
    const int v = c0 + min(j, n - 1);
    s_c[j].x = pt[3 * (size_t)v]; s_c[j].y = pt[3 * (size_t)v + 1]; s_c[j].z = pt[3 * (size_t)v + 2];
  }
  __syncthreads();
#pragma unroll 2
  for (int j = 0; j < n4; j += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double cx = s_c[j + u].x, cy = s_c[j + u].y, cz = s_c[j + u].z;
#pragma unroll
      for (int k = 0; k < DM_QPL; ++k) {
        const double dx = qx[k] - cx, dy = qy[k] - cy, dz = qz[k] - cz;
        best[k] = fmax(best[k], (dx * dx + dy * dy) + dz * dz);
      }
    }
  }
  const double b = wg_max(fmax(fmax(best[0], best[1]), fmax(best[2], best[3])), s_r);
  if (tid == 0) p.part[(size_t)m * p.Pmax + blockIdx.x] = b;
}

__global__ __launch_bounds__(PR_THREADS) void pts_diameter_finish_kernel(DiamParams p) {
  __shared__ double s_r[PR_WAVES];
  const int tid = threadIdx.x, m = blockIdx.x;
  const int V = p.offsets[m + 1] - p.offsets[m];
  const int T = (V + DM_TILE - 1) / DM_TILE;
  const int P = min(p.Pmax, T * (T + 1) / 2);
  const double* __restrict__ part = p.part + (size_t)m * p.Pmax;
  double b = 0.0;
  for (int i = tid; i < P; i += PR_THREADS) b = fmax(b, part[i]);
  b = wg_max(b, s_r);
  if (tid == 0) p.out[m] = sqrt(b);
}

int fps_slices(int M, int Vmax, int slices) {
  if (slices > 0) return slices;
  int cap = FPS_TARGET_BLOCKS / M;
  cap = cap < 16 ? 16 : (cap > FPS_MAX_SLICES ? FPS_MAX_SLICES : cap);
  const int want = (Vmax + FPS_SLICE_POINTS - 1) / FPS_SLICE_POINTS;
  return want < 1 ? 1 : (want > cap ? cap : want);
}

// the host copy of the offsets: clouds of at least one point each, one after the other from row 0; -> the largest cloud, or 0
int check_offsets(const int32_t* off, int M) {
  if (off[0] != 0) return 0;
  int vmax = 0;
  for (int m = 0; m < M; ++m) {
    if (off[m + 1] <= off[m]) return 0;
    const int v = off[m + 1] - off[m];
    vmax = v > vmax ? v : vmax;
  }
  return vmax;
}

size_t fps_bytes(int M, long long sumV, int G) {
  return sizeof(double) * ((size_t)sumV + 4 * (size_t)M + 2 * (size_t)M * G) + sizeof(int32_t) * 2 * (size_t)M * G;
}

}  // namespace

extern "C" size_t cp_fps_scratch_bytes(int M, long long sumV, int Vmax, int slices) {
  if (M <= 0 || M > 65535 || sumV <= 0 || Vmax <= 0 || Vmax > sumV || slices < 0 || slices > FPS_MAX_SLICES) return 0;
  return fps_bytes(M, sumV, fps_slices(M, Vmax, slices));
}

extern "C" int cp_fps(cp_stream_t stream, const double* pts, const int32_t* offsets, const int32_t* offsets_host, int M, int npoint,
                      int slices, int32_t* ids, double* xyz, void* scratch) {
  if (!pts || !offsets || !offsets_host || !ids || !xyz || !scratch) return CP_ERR_INVALID;
  if (M <= 0 || npoint < 1 || slices < 0 || slices > FPS_MAX_SLICES) return CP_ERR_INVALID;
  const int Vmax = check_offsets(offsets_host, M);
  if (Vmax <= 0) return CP_ERR_INVALID;
  if (((uintptr_t)pts & 7) || ((uintptr_t)xyz & 7) || ((uintptr_t)scratch & 7) || ((uintptr_t)ids & 3) || ((uintptr_t)offsets & 3))
    return CP_ERR_ALIGN;
  if (M > 65535 || npoint == INT_MAX) return CP_ERR_RANGE;       // (grid.y; the collecting launch is step `npoint`)
  const long long sumV = offsets_host[M];
  FpsParams p;
  p.pts = pts; p.offsets = offsets; p.ids = ids; p.xyz = xyz; p.M = M; p.npoint = npoint;
  p.G = fps_slices(M, Vmax, slices);
  p.dist = (double*)scratch;
  p.head = p.dist + sumV;
  p.pval = p.head + 4 * (size_t)M;
  p.pidx = (int32_t*)(p.pval + 2 * (size_t)M * p.G);
  p.step = 0;
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(fps_bbox_kernel, dim3((unsigned)M), dim3(PR_THREADS), 0, st, p);
  cp_mark_kernel("fps_step_kernel x%d", npoint + 1);             // (one entry for the chain: the log keeps 1 KiB of symbols)
  for (int s = 0; s < npoint; ++s) {
    p.step = s;
    hipLaunchKernelGGL(fps_step_kernel, dim3((unsigned)p.G, (unsigned)M), dim3(PR_THREADS), 0, st, p);
  }
  p.step = npoint;
  hipLaunchKernelGGL(fps_step_kernel, dim3(1, (unsigned)M), dim3(PR_THREADS), 0, st, p);
  return cp_check_launch();
}

extern "C" size_t cp_pts_diameter_scratch_bytes(int M, int Vmax) {
  if (M <= 0 || M > 65535 || Vmax <= 0) return 0;
  const long long T = ((long long)Vmax + DM_TILE - 1) / DM_TILE;
  if (T > DM_MAX_TILES) return 0;
  return sizeof(double) * (size_t)M * (size_t)(T * (T + 1) / 2);
}

extern "C" int cp_pts_diameter(cp_stream_t stream, const double* pts, const int32_t* offsets, const int32_t* offsets_host, int M,
                               double* diameters, void* scratch) {
  if (!pts || !offsets || !offsets_host || !diameters || !scratch || M <= 0) return CP_ERR_INVALID;
  const int Vmax = check_offsets(offsets_host, M);
  if (Vmax <= 0) return CP_ERR_INVALID;
  if (((uintptr_t)pts & 7) || ((uintptr_t)diameters & 7) || ((uintptr_t)scratch & 7) || ((uintptr_t)offsets & 3)) return CP_ERR_ALIGN;
  const long long T = ((long long)Vmax + DM_TILE - 1) / DM_TILE;
  if (M > 65535 || T > DM_MAX_TILES) return CP_ERR_RANGE;        // (about 5.9e6 points: 2^24 tile pairs)
  DiamParams p;
  p.pts = pts; p.offsets = offsets; p.part = (double*)scratch; p.out = diameters; p.M = M; p.Pmax = (int)(T * (T + 1) / 2);
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(pts_diameter_kernel, dim3((unsigned)p.Pmax, (unsigned)M), dim3(PR_THREADS), 0, st, p);
  CP_LAUNCH(pts_diameter_finish_kernel, dim3((unsigned)M), dim3(PR_THREADS), 0, st, p);
  return cp_check_launch();
}
