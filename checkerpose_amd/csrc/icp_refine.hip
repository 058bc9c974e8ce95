// Projective point-to-plane ICP of solved poses against the sensor's depth image, on the device: the depth
// refinement step a user with an RGB-D frame expects after an RGB-only estimate, whose error is largest along the viewing ray.  The
// reference does not refine: the row is opt-in, and its rule is this project's OWN (tests/icp_stages.py restates it in numpy; parity
// with any ICP library is UNPINNED).
//
// THE RULE.  Everything after the render in fp64 without contraction.  fx, fy, cx, cy = K[0], K[4], K[2], K[5].
//
// Stage A, surface samples of a pose (cp_surface_samples; ONE raster pass at the INPUT pose).  The render is vsd_raster.h's (its rule,
//   its "a vertex at Z <= 0 is not rendered", its winning face: the smallest index on equal 1 / Z).
//   lattice   rect = the pose's merged vertex rectangle (VsHdr::RECT) intersected with the frame, w x h pixels from (x0, y0);
//             nx = min(grid, w), ny = min(grid, h); column i is pixel x0 + ((2 i + 1) w) / (2 nx), rows likewise (integer divisions);
//             slot j * nx + i of the pose's S = grid * grid slots (grid in 1..64).  No compaction, no atomics: a slot is a sample or
//             empty, and its content depends neither on launch order nor on the image size or the batch.
//   sample    a lattice pixel (x, y) the mesh covers: depth = the render's fp32 depth, face = the winning face,
//             Qr = (((x + 0.5 - cx) depth) / fx, ((y + 0.5 - cy) depth) / fy, depth), X = R^T (Qr - t) the model-space point,
//             N = the unit normal of `face` from its three model vertices ((v1 - v0) x (v2 - v0), normalised), negated where
//             (R N) . Qr > 0 (it points towards the camera).  A face whose normal is not finite leaves the slot empty (face -1).
//
// Stage B, association under a pose (R, t), per sample, with depth now the SENSOR depth of the pose's image:
//   Y = R X, C = Y + t; reject unless C_z > 0;  u = (fx C_x) / C_z + cx, v likewise; pixel (floor u, floor v); reject outside the frame;
//   d = depth[py, px]; reject unless d is finite and > 0;  Q = C (d / C_z): the measured surface point on the sample's own ray;
//   reject unless |C - Q|_2 <= max_dist (occluders and background drop out here);  Np = R N, frozen until the next association.
//   n = the number of pairs.
//
// Stage C, Levenberg-Marquardt over the pairs.  r_i = Np_i . (C_i - Q_i) with Q_i, Np_i fixed; increment d = (w, v): R' = exp([w]x) R,
//   t' = t + v; J_i = [(Y_i x Np_i)^T, Np_i^T]; H = sum J^T J, g = sum J^T r, c = sum r^2; lambda = 1e-3; rho = diameter / 2 of the mesh.
//   At most max_iters (1..64) times:
//     1. solve (H + lambda diag(H) + inertia n diag(rho^2, rho^2, rho^2, 1, 1, 1)) d = -g by Cholesky (one thread);
//     2. not positive definite (s, R', t' recorded as NaN), or |v|_2 > max_dist, or |w|_2 rho > max_dist: rejected with c' = +inf;
//     3. else c' = the cost of (R', t') over the SAME pairs (Q_i, Np_i unchanged); a c' that is not finite counts as +inf;
//     4. accept iff c' < c: the state becomes (R', t'), lambda = max(lambda / 10, 1e-12), stage B runs again under the new state
//        (n, H, g, c are the new pairs'); n < min_pairs then stops with status 3;
//     5. else lambda = 10 lambda; lambda > 1e8 stops with status 3;
//     6. s = max(|w|_inf, |v|_inf / |t|), t from before the step: an ACCEPTED step with s <= step_tol stops with status 1;
//     7. the iterations run out: status 2.
//   pass-through (status 0: the output pose is BITWISE the input pose, info holds NaN but for the counts): status_in == 0; a pose or K
//     entry not finite; a mesh or image id out of range; fewer than min_pairs samples (a render that was refused has none); fewer
//     than min_pairs pairs under the input pose.
//   returned  bitwise the last accepted trial pose, or the input pose when nothing was accepted.
//   info      42 doubles: [c at the input pose, c at the returned pose, samples, pairs at the input pose, pairs at the returned pose,
//             iterations, H (36): the undamped J^T J at the returned pose over its pairs].
//   records   18 doubles per executed iteration: [lambda used, n, c, c', accepted 0/1, s, R' (9), t' (3)]; other slots are not written.
//
// Stage A is the scaffold's three kernels (pose, vertex, 32 x 32 tile with vs_raster_tile<true>; the tile kernel stores only the
// lattice pixels' (depth, face) into the pose's slots) and a finish pass that turns them into pixel, X, N.  Stages B and C are ONE
// launch, one 256-thread workgroup per pose, like pnp_refine.hip: a thread takes slots tid, tid + 256, ... in ascending order,
// pnp_core.h's block_sum joins the 21 + 6 + 1 + 1 sums (H, g, c, n) in a fixed order, no atomics.  Thread 0 damps H, does the Cholesky
// and Rodrigues (pnp_core.h's lm_solve_step; L in LDS), applies the step bound and publishes the trial through LDS; all threads then
// evaluate c'.  The pairs are NOT kept between the passes: stage B is recomputed from the state pose (deterministic; 52 bytes per slot
// and one depth gather, all in L2 after the first pass), which keeps the kernel free of per-thread arrays and of scratch.  Every
// branch on accept / stop is taken on block_sum results or LDS words that all threads hold identically; every loop is bounded by
// max_iters or the slot count; no workgroup waits for another.
#include "pnp_core.h"
#include "vsd_raster.h"

#pragma clang fp contract(off)

namespace {

constexpr int ICP_REC = 18, ICP_INFO = 42, ICP_MAX_ITERS = 64, ICP_SUMS = 29, ICP_GRID_MAX = 64;      // sums: H (21), g (6), c, n
using SsH = VsHdr<1>;
constexpr int SS_HDR = 24;                       // 4-byte words per pose (the rest is spare)

// ------------------------------------------------------------------------------------------------------------------- stage A
struct SsParams {
  VsMesh mesh;
  const double* poses;        // (P, 12)
  const double* K;
  int32_t* rect;              // (P, 4)
  int32_t* shape;             // (P, 2)
  int32_t* pixel;             // (P, S, 2)
  float* depth;               // (P, S)
  int32_t* face;              // (P, S)
  double* X;                  // (P, S, 3)
  double* N;                  // (P, S, 3)
  int32_t* ok;                // (P)
  int32_t* hdr;               // (P, SS_HDR)
  float4* sv;                 // (P, Vmax)
  int k_stride, P, H, W, grid, tx, ty, vchunks;
};

// the lattice of a pose: the header's rectangle intersected with the frame; nx = 0 where that is empty
struct SsLattice { int x0, y0, w, h, nx, ny; };
__device__ __forceinline__ SsLattice ss_lattice(const int32_t* __restrict__ rect, int W, int H, int grid) {
  SsLattice l = {0, 0, 0, 0, 0, 0};
  if (rect[0] == INT_MAX) return l;              // no vertex merged
  const int x0 = max(rect[0], 0), y0 = max(rect[1], 0), x1 = min(rect[2], W - 1), y1 = min(rect[3], H - 1);
  if (x0 > x1 || y0 > y1) return l;
  l.x0 = x0; l.y0 = y0; l.w = x1 - x0 + 1; l.h = y1 - y0 + 1;
  l.nx = min(grid, l.w); l.ny = min(grid, l.h);
  return l;
}
// lattice coordinate i of n over an extent e -> its offset from the extent's first pixel
__device__ __forceinline__ int ss_offset(int i, int e, int n) { return (int)(((2LL * i + 1) * e) / (2LL * n)); }
// the lattice coordinate whose pixel lies d behind the extent's first, or -1: offset(i) lies in [i e / n, (i + 1) e / n), hence
// i is floor(d n / e) or the one after it (offsets increase strictly: n <= e)
__device__ __forceinline__ int ss_index(int d, int e, int n) {
  if (d < 0 || d >= e) return -1;
  const int i0 = (int)(((long long)d * n) / e);
  if (ss_offset(i0, e, n) == d) return i0;
  if (i0 + 1 < n && ss_offset(i0 + 1, e, n) == d) return i0 + 1;
  return -1;
}

__global__ __launch_bounds__(VS_THREADS) void icp_pose_kernel(SsParams p) {
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * SS_HDR;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  const double* __restrict__ q = p.poses + 12 * (size_t)b;
  int vfirst, V, ffirst, F, m;
  bool ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  ok = ok && vs_pose_finite(K, q);
  vs_side_init(K, 1.0, q, (float*)h + SsH::P(0), h + SsH::RECT(0));
  h[SsH::BAD(0)] = 0;
  h[SsH::OK] = ok ? 1 : 0;
}

__global__ __launch_bounds__(VS_THREADS) void icp_vertex_kernel(SsParams p) {
  int b, s, vc;
  vs_vertex_block(p.vchunks, 1, b, s, vc);
  int32_t* __restrict__ h = p.hdr + (size_t)b * SS_HDR;
  if (!h[SsH::OK]) return;                                            // (uniform; no barrier in this kernel)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  vs_vertex_chunk((const float*)h + SsH::P(0), p.mesh.verts + 3 * (size_t)vfirst, V, vc, make_float4(-2.f, (float)p.W + 1.f, -2.f, (float)p.H + 1.f),
                  p.sv + (size_t)b * p.mesh.Vmax, h + SsH::RECT(0), h + SsH::BAD(0));
}

__global__ __launch_bounds__(VS_THREADS) void icp_tile_kernel(SsParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  const VsTile c = vs_tile(p.tx, p.ty, 0, 0);
  const int b = c.b;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * SS_HDR;
  const bool live = h[SsH::OK] && !h[SsH::BAD(0)];
  if (!live || !vs_tile_hit(h + SsH::RECT(0), c.ox, c.oy)) return;    // (uniform) every lattice pixel lies in a tile the rectangle meets
  const SsLattice l = ss_lattice(h + SsH::RECT(0), p.W, p.H, p.grid);
  if (l.nx == 0) return;                                              // (uniform)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  float best[VS_PPL];
  int face[VS_PPL];
  vs_raster_tile<true>(s_tri, &s_n, p.sv + (size_t)b * p.mesh.Vmax, p.mesh.faces + 3 * (size_t)ffirst, F, V, c, best, face);
  const size_t base = (size_t)b * p.grid * p.grid;
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) {
    const int x = c.ox + c.lx, y = c.oy + c.y(k);
    if (x >= p.W || y >= p.H) continue;
    const int i = ss_index(x - l.x0, l.w, l.nx), j = ss_index(y - l.y0, l.h, l.ny);
    if (i < 0 || j < 0) continue;
    const size_t at = base + (size_t)(j * l.nx + i);                  // j * nx + i < nx * ny <= grid * grid
    p.depth[at] = vs_depth_of(best[k]);
    p.face[at] = best[k] > 0.f ? face[k] : -1;
  }
}

// per pose: rect, shape, ok; per slot: pixel, and of a covered lattice pixel X and N; everything else empty
__global__ __launch_bounds__(VS_THREADS) void icp_finish_kernel(SsParams p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * SS_HDR;
  const bool live = h[SsH::OK] && !h[SsH::BAD(0)];
  SsLattice l = {0, 0, 0, 0, 0, 0};
  if (live) l = ss_lattice(h + SsH::RECT(0), p.W, p.H, p.grid);
  const int S = p.grid * p.grid, used = l.nx * l.ny;
  if (tid == 0) {
    const bool have = l.nx > 0;
    int32_t* r = p.rect + 4 * (size_t)b;
    r[0] = have ? l.x0 : -1; r[1] = have ? l.y0 : -1; r[2] = have ? l.x0 + l.w - 1 : -1; r[3] = have ? l.y0 + l.h - 1 : -1;
    p.shape[2 * (size_t)b] = l.nx; p.shape[2 * (size_t)b + 1] = l.ny;
    p.ok[b] = live ? 1 : 0;
  }
  int vfirst = 0, V = 0, ffirst = 0, F = 0, m = 0;
  if (live) vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  const double* __restrict__ q = p.poses + 12 * (size_t)b;
  for (int slot = tid; slot < S; slot += VS_THREADS) {
    const size_t at = (size_t)b * S + slot;
    int px = -1, py = -1, f = -1;
    float dep = 0.f;
    double X[3] = {NAN, NAN, NAN}, N[3] = {NAN, NAN, NAN};
    if (slot < used) {
      px = l.x0 + ss_offset(slot % l.nx, l.w, l.nx);
      py = l.y0 + ss_offset(slot / l.nx, l.h, l.ny);
      dep = p.depth[at];
      f = p.face[at];
      if (f >= F) f = -1;                                             // (cannot happen: the walk only names faces of the mesh)
    }
    if (f >= 0) {
      const double fx = K[0], fy = K[4], cx = K[2], cy = K[5], d = (double)dep;
      const double Q[3] = {(((double)px + 0.5 - cx) * d) / fx, (((double)py + 0.5 - cy) * d) / fy, d};
      const double e[3] = {Q[0] - q[9], Q[1] - q[10], Q[2] - q[11]};
      for (int k = 0; k < 3; ++k) X[k] = vs_dot3(q[k], q[3 + k], q[6 + k], e[0], e[1], e[2]);
      const int32_t* __restrict__ fi = p.mesh.faces + 3 * ((size_t)ffirst + f);
      const float* __restrict__ vt = p.mesh.verts + 3 * (size_t)vfirst;
      const float *v0 = vt + 3 * (size_t)fi[0], *v1 = vt + 3 * (size_t)fi[1], *v2 = vt + 3 * (size_t)fi[2];
      const double a[3] = {(double)v1[0] - (double)v0[0], (double)v1[1] - (double)v0[1], (double)v1[2] - (double)v0[2]};
      const double c[3] = {(double)v2[0] - (double)v0[0], (double)v2[1] - (double)v0[1], (double)v2[2] - (double)v0[2]};
      const double n[3] = {a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]};
      const double len = sqrt(vs_dot3(n[0], n[1], n[2], n[0], n[1], n[2]));
      for (int k = 0; k < 3; ++k) N[k] = n[k] / len;
      double rn[3];
      for (int k = 0; k < 3; ++k) rn[k] = vs_dot3(q[3 * k], q[3 * k + 1], q[3 * k + 2], N[0], N[1], N[2]);
      if (vs_dot3(rn[0], rn[1], rn[2], Q[0], Q[1], Q[2]) > 0.0)
        for (int k = 0; k < 3; ++k) N[k] = -N[k];
      if (!isfinite(N[0]) || !isfinite(N[1]) || !isfinite(N[2])) {
        f = -1;
        for (int k = 0; k < 3; ++k) { X[k] = NAN; N[k] = NAN; }
      }
    }
    p.pixel[2 * at] = px; p.pixel[2 * at + 1] = py;
    p.depth[at] = dep;
    p.face[at] = f;
    for (int k = 0; k < 3; ++k) { p.X[3 * at + k] = X[k]; p.N[3 * at + k] = N[k]; }
  }
}

// ------------------------------------------------------------------------------------------------------------ stages B and C
struct IcpParams {
  const double* pose_in; const double* K; const double* X; const double* N; const int32_t* face;
  const float* depth; const int32_t* image_ids; const double* max_dist; const double* diameters; const int32_t* mesh_ids;
  const int32_t* status_in;
  double* pose_out; int32_t* status_out; double* info; double* records;
  int k_stride, P, S, I, H, W, M, max_iters, min_pairs;
  double step_tol, inertia;
};

struct IcpView {                 // one pose's samples, image and camera
  const double* X; const double* N; const int32_t* face; const float* depth;
  int S, H, W;
  double fx, fy, cx, cy, max_dist;
};

// stage B for one sample under (R, t): false = no pair; else X, Y = R X, Q, Np = R N
__device__ __forceinline__ bool icp_associate(const IcpView& s, int slot, const double* R, const double* t, double* Y, double* Q, double* Np,
                                              double* Xout) {
  if (s.face[slot] < 0) return false;
  const double X0 = s.X[3 * slot], X1 = s.X[3 * slot + 1], X2 = s.X[3 * slot + 2];
  Xout[0] = X0; Xout[1] = X1; Xout[2] = X2;
  Y[0] = R[0] * X0 + R[1] * X1 + R[2] * X2; Y[1] = R[3] * X0 + R[4] * X1 + R[5] * X2; Y[2] = R[6] * X0 + R[7] * X1 + R[8] * X2;
  const double C0 = Y[0] + t[0], C1 = Y[1] + t[1], C2 = Y[2] + t[2];
  if (!(C2 > 0.0)) return false;
  const double u = (s.fx * C0) / C2 + s.cx, v = (s.fy * C1) / C2 + s.cy;
  if (!(u >= 0.0 && u < (double)s.W && v >= 0.0 && v < (double)s.H)) return false;      // (a NaN fails here; floor(u) <= W - 1)
  const int px = (int)floor(u), py = (int)floor(v);
  const double d = (double)s.depth[(size_t)py * s.W + px];
  if (!(isfinite(d) && d > 0.0)) return false;
  const double sc = d / C2;
  Q[0] = C0 * sc; Q[1] = C1 * sc; Q[2] = C2 * sc;
  const double e0 = C0 - Q[0], e1 = C1 - Q[1], e2 = C2 - Q[2];
  if (!(sqrt(e0 * e0 + e1 * e1 + e2 * e2) <= s.max_dist)) return false;
  const double N0 = s.N[3 * slot], N1 = s.N[3 * slot + 1], N2 = s.N[3 * slot + 2];
  Np[0] = R[0] * N0 + R[1] * N1 + R[2] * N2; Np[1] = R[3] * N0 + R[4] * N1 + R[5] * N2; Np[2] = R[6] * N0 + R[7] * N1 + R[8] * N2;
  return true;
}

// one thread's slots under the state (R, t).  TRIAL false: acc[0..20] the upper triangle of H row by row, [21..26] g, [27] c, [28] n;
// TRIAL true: acc[0] = the cost of (Rn, tn) over the state's pairs
template <bool TRIAL>
__device__ __forceinline__ void icp_accumulate(const IcpView& s, int tid, const double* R, const double* t, const double* Rn, const double* tn,
                                               double* acc) {
#pragma unroll
  for (int k = 0; k < (TRIAL ? 1 : ICP_SUMS); ++k) acc[k] = 0.0;
  for (int slot = tid; slot < s.S; slot += PNP_THREADS) {
    double Y[3], Q[3], Np[3], X[3];
    if (!icp_associate(s, slot, R, t, Y, Q, Np, X)) continue;
    if constexpr (TRIAL) {
      const double Y0 = Rn[0] * X[0] + Rn[1] * X[1] + Rn[2] * X[2], Y1 = Rn[3] * X[0] + Rn[4] * X[1] + Rn[5] * X[2],
                   Y2 = Rn[6] * X[0] + Rn[7] * X[1] + Rn[8] * X[2];
      const double r = Np[0] * ((Y0 + tn[0]) - Q[0]) + Np[1] * ((Y1 + tn[1]) - Q[1]) + Np[2] * ((Y2 + tn[2]) - Q[2]);
      acc[0] += r * r;
    } else {
      const double r = Np[0] * ((Y[0] + t[0]) - Q[0]) + Np[1] * ((Y[1] + t[1]) - Q[1]) + Np[2] * ((Y[2] + t[2]) - Q[2]);
      const double J[6] = {Y[1] * Np[2] - Y[2] * Np[1], Y[2] * Np[0] - Y[0] * Np[2], Y[0] * Np[1] - Y[1] * Np[0], Np[0], Np[1], Np[2]};
      int e = 0;
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = p; q < 6; ++q) { acc[e] += J[p] * J[q]; ++e; }
#pragma unroll
      for (int p = 0; p < 6; ++p) acc[21 + p] += J[p] * r;
      acc[27] += r * r;
      acc[28] += 1.0;
    }
  }
}

__global__ __launch_bounds__(PNP_THREADS) void icp_refine_kernel(const IcpParams p) {
  __shared__ double sred[4 * ICP_SUMS];
  __shared__ double s_H[ICP_SUMS];                                            // the state's H (21), g (6), c, n: written and read by thread 0
  __shared__ double s_L[6][6], s_trial[19];
  __shared__ int s_kind;
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* K = p.K + (size_t)p.k_stride * b;
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = p.pose_in[(size_t)b * 12 + i];
  for (int i = 0; i < 3; ++i) t[i] = p.pose_in[(size_t)b * 12 + 9 + i];
  double* const pose_out = p.pose_out + (size_t)b * 12;
  double* const info = p.info + (size_t)b * ICP_INFO;
  const int img = p.image_ids ? p.image_ids[b] : 0, m = p.mesh_ids ? p.mesh_ids[b] : 0;
  bool pass = (p.status_in && p.status_in[b] == 0) || img < 0 || img >= p.I || m < 0 || m >= p.M;      // every thread reads the same words: uniform
  for (int i = 0; i < 9; ++i) pass = pass || !isfinite(R[i]) || !isfinite(K[i]);
  for (int i = 0; i < 3; ++i) pass = pass || !isfinite(t[i]);
  IcpView s;
  s.X = p.X + (size_t)b * p.S * 3; s.N = p.N + (size_t)b * p.S * 3; s.face = p.face + (size_t)b * p.S;
  s.depth = p.depth + (size_t)(pass ? 0 : img) * p.H * p.W;
  s.S = p.S; s.H = p.H; s.W = p.W;
  s.fx = K[0]; s.fy = K[4]; s.cx = K[2]; s.cy = K[5]; s.max_dist = p.max_dist[b];
  const double rho = pass ? 0.0 : p.diameters[m] / 2.0;
  double ns[1] = {0.0};
  for (int slot = tid; slot < p.S; slot += PNP_THREADS) ns[0] += s.face[slot] >= 0 ? 1.0 : 0.0;
  block_sum<1>(ns, sred, tid);
  const double n_samples = ns[0];
  pass = pass || n_samples < (double)p.min_pairs;
  double c = 0.0, c0 = 0.0, n = 0.0, n0 = 0.0, lambda = 1e-3;
  int status = 2, iters = 0;
  double acc[ICP_SUMS];
  if (!pass) {                                                                // the sums at the input pose
    icp_accumulate<false>(s, tid, R, t, R, t, acc);
    block_sum<ICP_SUMS>(acc, sred, tid);
    c = c0 = acc[27]; n = n0 = acc[28];
    if (tid == 0)
      for (int i = 0; i < ICP_SUMS; ++i) s_H[i] = acc[i];
    pass = n0 < (double)p.min_pairs;
  }
  for (int it = 0; it < p.max_iters && !pass; ++it) {
    // thread 0: (H + lambda diag H + inertia n diag(rho^2 x 3, 1 x 3)) d = -g -> kind 0: no Cholesky factor (NaN in s_trial); 1: a trial
    // pose; 2: a trial pose beyond the step bound
    if (tid == 0) {
      const double damp = p.inertia * n;
      lm_load_lower(s_H, s_L);
      for (int q = 0; q < 6; ++q) s_L[q][q] = (s_L[q][q] + lambda * s_L[q][q]) + damp * (q < 3 ? rho * rho : 1.0);
      double y[6], d[6];
      int kind = lm_solve_step(s_L, s_H + 21, R, t, y, d, s_trial) ? 1 : 0;
      if (kind && (sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]) > s.max_dist ||
                   sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) * rho > s.max_dist))
        kind = 2;
      s_kind = kind;
    }
    __syncthreads();
    const int kind = s_kind;
    double Rn[9], tn[3];
    for (int i = 0; i < 9; ++i) Rn[i] = s_trial[6 + i];
    for (int i = 0; i < 3; ++i) tn[i] = s_trial[15 + i];
    const double sstep = s_trial[18];
    double cn = INFINITY;
    if (kind == 1) {
      double a1[1];
      icp_accumulate<true>(s, tid, R, t, Rn, tn, a1);
      block_sum<1>(a1, sred, tid);                                            // (its barriers also fence s_trial and s_kind against the next trial)
      if (isfinite(a1[0])) cn = a1[0];
    } else {
      __syncthreads();
    }
    const bool accept = cn < c;
    if (p.records && tid == 0) {
      double* rec = p.records + ((size_t)b * p.max_iters + it) * ICP_REC;
      rec[0] = lambda; rec[1] = n; rec[2] = c; rec[3] = cn; rec[4] = accept ? 1.0 : 0.0; rec[5] = sstep;
      for (int i = 0; i < 9; ++i) rec[6 + i] = Rn[i];
      for (int i = 0; i < 3; ++i) rec[15 + i] = tn[i];
    }
    iters = it + 1;
    if (accept) {
      for (int i = 0; i < 9; ++i) R[i] = Rn[i];
      for (int i = 0; i < 3; ++i) t[i] = tn[i];
      lambda = fmax(lambda / 10.0, 1e-12);
      icp_accumulate<false>(s, tid, R, t, R, t, acc);                         // stage B again under the new state
      block_sum<ICP_SUMS>(acc, sred, tid);
      c = acc[27]; n = acc[28];
      if (tid == 0)
        for (int i = 0; i < ICP_SUMS; ++i) s_H[i] = acc[i];
      if (n< (double)p.min_pairs) { status = 3; break; }
      if (sstep <= p.step_tol) { status = 1; break; }
    } else {
      lambda = lambda * 10.0;
      if (lambda > 1e8) { status = 3; break; }
    }
  }
  if (tid != 0) return;
  for (int i = 0; i < 9; ++i) pose_out[i] = R[i];                             // pass-through: R, t still hold the input's bits
  for (int i = 0; i < 3; ++i) pose_out[9 + i] = t[i];
  if (pass) {
    p.status_out[b] = 0;
    for (int i = 0; i < ICP_INFO; ++i) info[i] = NAN;
    info[2] = n_samples; info[3] = n0; info[4] = n0; info[5] = 0.0;
    return;
  }
  p.status_out[b] = status;
  info[0] = c0; info[1] = c; info[2] = n_samples; info[3] = n0; info[4] = n; info[5] = (double)iters;
  int e = 0;
  for (int a = 0; a < 6; ++a)
    for (int q = a; q < 6; ++q) { info[6 + 6 * a + q] = s_H[e]; info[6 + 6 * q + a] = s_H[e]; ++e; }
}

}  // namespace

extern "C" size_t cp_surface_samples_scratch_bytes(int P, int Vmax) {
  if (P <= 0 || Vmax < 0) return 0;
  return cp_align16_up((size_t)P * SS_HDR * sizeof(int32_t)) + (size_t)P * Vmax * sizeof(float4);
}

extern "C" int cp_surface_samples(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                                  const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                                  int H, int W, int P, int Vmax, int grid, int32_t* rect, int32_t* shape, int32_t* pixel, float* depth,
                                  int32_t* face, double* X, double* N, int32_t* ok, void* scratch) {
  SsParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !rect || !shape || !pixel || !depth || !face || !X || !N || !ok || !scratch) return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, P) || grid < 1 || grid > ICP_GRID_MAX) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || vs_mesh_misaligned(p.mesh) || cp_misaligned(rect, 3) ||
      cp_misaligned(shape, 3) || cp_misaligned(pixel, 3) || cp_misaligned(depth, 3) || cp_misaligned(face, 3) || cp_misaligned(X, 7) ||
      cp_misaligned(N, 7) || cp_misaligned(ok, 3))
    return CP_ERR_ALIGN;
  VsGrid g;
  if (!vs_grid(W, H, 1, false, P, 1, Vmax, g) || (long long)H * W >= (1LL << 31)) return CP_ERR_RANGE;
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.rect = rect; p.shape = shape; p.pixel = pixel; p.depth = depth; p.face = face;
  p.X = X; p.N = N; p.ok = ok; p.P = P; p.H = H; p.W = W; p.grid = grid; p.tx = g.tx; p.ty = g.ty; p.vchunks = g.vchunks;
  p.hdr = (int32_t*)scratch;
  p.sv = (float4*)((char*)scratch + cp_align16_up((size_t)P * SS_HDR * sizeof(int32_t)));
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(icp_pose_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(icp_vertex_kernel, dim3(g.vert_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(icp_tile_kernel, dim3(g.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(icp_finish_kernel, dim3((unsigned)P), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}

extern "C" int cp_icp_refine_record_doubles(void) { return ICP_REC; }
extern "C" int cp_icp_refine_info_doubles(void) { return ICP_INFO; }

extern "C" int cp_icp_refine(cp_stream_t stream, const double* pose_in, const double* cam_K, int k_stride, const double* X, const double* N,
                             const int32_t* face, int S, const float* depth, const int32_t* image_ids, int I, int H, int W,
                             const double* max_dist, const double* diameters, int M, const int32_t* mesh_ids, const int32_t* status_in,
                             int max_iters, double step_tol, int min_pairs, double inertia, int P, double* pose_out, int32_t* status_out,
                             double* info, double* records) {
  if (!pose_in || !X || !N || !face || !depth || !max_dist || !diameters || !pose_out || !status_out || !info) return CP_ERR_INVALID;
  if (vs_view_invalid(cam_K, k_stride, H, W, P) || vs_images_invalid(image_ids, I) || M <= 0 || (!mesh_ids && M != 1)) return CP_ERR_INVALID;
  if (S < 1 || S > PNP_NMAX || max_iters < 1 || max_iters > ICP_MAX_ITERS || min_pairs < 6) return CP_ERR_INVALID;
  if (!cp_finite_positive(step_tol) || !(inertia >= 0.0) || !(inertia <= 1.7976931348623157e308)) return CP_ERR_INVALID;      // inertia: not negative and finite
  if (cp_misaligned(pose_in, 7) || vs_view_misaligned(cam_K) || cp_misaligned(X, 7) || cp_misaligned(N, 7) || cp_misaligned(face, 3) ||
      cp_misaligned(depth, 3) || cp_misaligned(image_ids, 3) || cp_misaligned(max_dist, 7) || cp_misaligned(diameters, 7) ||
      cp_misaligned(mesh_ids, 3) || cp_misaligned(status_in, 3) || cp_misaligned(pose_out, 7) || cp_misaligned(status_out, 3) ||
      cp_misaligned(info, 7) || cp_misaligned(records, 7))
    return CP_ERR_ALIGN;
  if (cp_pose_alias_invalid(pose_in, pose_out, P)) return CP_ERR_INVALID;
  if ((long long)H * W >= (1LL << 31) || P >= (1 << 24)) return CP_ERR_RANGE;
  IcpParams p;
  p.pose_in = pose_in; p.K = cam_K; p.X = X; p.N = N; p.face = face; p.depth = depth; p.image_ids = image_ids; p.max_dist = max_dist;
  p.diameters = diameters; p.mesh_ids = mesh_ids; p.status_in = status_in; p.pose_out = pose_out; p.status_out = status_out; p.info = info;
  p.records = records; p.k_stride = k_stride; p.P = P; p.S = S; p.I = I; p.H = H; p.W = W; p.M = M; p.max_iters = max_iters;
  p.min_pairs = min_pairs; p.step_tol = step_tol; p.inertia = inertia;
  CP_LAUNCH(icp_refine_kernel, dim3((unsigned)P), dim3(PNP_THREADS), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}
