// Self-occlusion measure on the device: the per-view rule of the reference's
// preprocess_data/get_overall_visibility.py:20-42 compute_vis_hpr -- Katz et al.'s "hidden point removal": flip the cloud through a
// sphere around the viewpoint, take the convex hull of the flipped points plus the viewpoint, a vertex is visible when it is a
// vertex of that hull -- for n_views rigid poses of one cloud in ONE launch.
//
// Everything is fp64 and this whole file is compiled with `#pragma clang fp contract(off)` as prepare.hip is: the flipped
// coordinates are numpy's own expressions, and the hull's decisions are signs of plane values that every test of a face takes from
// the ONE plane stored with that face.  No floating-point atomics; counts is made with integer atomic adds.
//
// hpr_visibility_kernel: G workgroups of 256 lanes share the views (workgroup g takes views g, g + G, ...), one view at a time in
// the workgroup's own slab of scratch (layout: hv_carve).  No workgroup waits for another, every loop has an explicit bound, and a
// view that goes wrong ends with a status code (HV_*), never spins.  Per view:
//   1. pc = R p + t as ((r0 x + r1 y) + r2 z) + t; norm = sqrt((x x + y y) + z z); radius = max norm * 10^radius_param;
//      flipped = pc + (2 (radius - norm)) * (pc / norm); point 0 is the viewpoint (0, 0, 0).
//   2. initial tetrahedron, lowest index on ties: arg-min / arg-max of x, the point farthest from their line, the point farthest
//      from their plane; a zero extent -> HV_DEGENERATE.  A face (a, b, c) stores n = (b - a) x (c - a), off = -n . a, outward;
//      "above" is n . x + off > 0, strictly.
//   3. every point that is not a vertex is assigned to the first of the four faces it lies above, or to none.
//   4. while a pending (assigned) point exists: F = the face of the LOWEST-INDEX pending point (a cursor that only moves forward:
//      a point never becomes pending again); p = arg-max over ALL points of F's plane value, lowest index on ties -- extreme in F's
//      normal direction, so a vertex of the final hull: its flag is final at insertion.  The visible set = every live face with p
//      above it, found by testing all face slots (no adjacency structure).  The horizon = the directed edges of visible faces whose
//      reverse is no edge of a visible face; fewer than 3 edges or a repeated start point -> HV_HORIZON.  The visible faces retire,
//      one face (a, b, p) per horizon edge is staged, the points of retired faces (only those) are tested against the staged faces
//      (only those): a point goes to the face with the LARGEST plane value it lies above, on equal values to the edge with the
//      smaller start point -- a rule that does not depend on the order in which lanes appended to the lists, so no run, batch or
//      workgroup count can change a bit.  The staged faces then take the retired slots and, beyond those, fresh slots at the end.
//   5. at most V + 1 insertions (HV_ITERATIONS); live faces never exceed 2 (V + 1) - 4, and with the slots reused that is the
//      table's size (HV_TABLE_FULL guards it).
//   6. the visible-face list and the horizon list are LDS lists sized for the common case (HV_VIS_LDS faces, HV_HZ_LDS edges: the
//      mean visible set is 3 faces) with a global-memory spill in the slab, entry k of either list living in LDS for k below the
//      LDS size and in the slab otherwise: correct for any size up to the live-face count.
#include <limits.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int HV_THREADS = 256;
constexpr int HV_WAVES = HV_THREADS / 64;
constexpr int HV_VIS_LDS = 4;                    // visible faces kept in LDS (the rest: the slab's vis list)
constexpr int HV_HZ_LDS = HV_VIS_LDS + 2;        // horizon edges / staged faces kept in LDS (a disc of v faces has v + 2 boundary edges)
constexpr int HV_MAX_V = 1 << 22;
constexpr int HV_MAX_WG = 65535;
constexpr int HV_AUTO_WG = 512;                  // the automatic choice: at most this many workgroups ...
constexpr size_t HV_AUTO_BYTES = (size_t)2 << 30;   // ... and at most about this much scratch

enum { HV_OK = 0, HV_DEGENERATE = 1, HV_HORIZON = 2, HV_TABLE_FULL = 3, HV_ITERATIONS = 4, HV_NORM = 5 };
enum { HV_NONE = -1, HV_VERTEX = -2 };           // assign[i]: a face slot >= 0, or one of these
enum { HV_DEAD = 0, HV_LIVE = 1, HV_RETIRED = 2 };

struct HvParams {
  const double* pts;          // (V,3)
  const double* R;            // (n_views,3,3)
  const double* t;            // (3) or (n_views,3)
  int32_t* counts;            // (V)
  uint8_t* mask;              // (n_views,V) or null
  int32_t* status;            // (n_views)
  char* scratch;
  size_t wg_bytes;
  double scale;               // 10^radius_param
  int t_stride, n_views, V, G;
};

// one workgroup's slab: N = V + 1 points, Fcap = 2 V - 2 face slots, Hcap = Fcap + 2 staged faces
struct HvSlab {
  double* P;                  // (N,3) flipped points, row 0 the viewpoint
  double* fpl;                // (Fcap,4) face planes
  double* hpl;                // (Hcap,4) staged planes (entries >= HV_HZ_LDS)
  int* assign;                // (N)
  int* mark;                  // (N) the insertion that last saw the point start a horizon edge
  int* fv;                    // (Fcap,3) face vertices
  int* state;                 // (Fcap)
  int* vis;                   // (Fcap) visible faces (entries >= HV_VIS_LDS)
  int* ha;                    // (Hcap) horizon edge starts ...
  int* hb;                    // (Hcap) ... and ends (entries >= HV_HZ_LDS)
};

__host__ __device__ inline size_t hv_carve(int V, char* base, HvSlab* s) {
  const size_t N = (size_t)V + 1, Fcap = 2 * (size_t)V - 2, Hcap = Fcap + 2;
  size_t o = 0;
  if (s) s->P = (double*)(base + o);
  o += sizeof(double) * 3 * N;
  if (s) s->fpl = (double*)(base + o);
  o += sizeof(double) * 4 * Fcap;
  if (s) s->hpl = (double*)(base + o);
  o += sizeof(double) * 4 * Hcap;
  if (s) s->assign = (int*)(base + o);
  o += sizeof(int) * N;
  if (s) s->mark = (int*)(base + o);
  o += sizeof(int) * N;
  if (s) s->fv = (int*)(base + o);
  o += sizeof(int) * 3 * Fcap;
  if (s) s->state = (int*)(base + o);
  o += sizeof(int) * Fcap;
  if (s) s->vis = (int*)(base + o);
  o += sizeof(int) * Fcap;
  if (s) s->ha = (int*)(base + o);
  o += sizeof(int) * Hcap;
  if (s) s->hb = (int*)(base + o);
  o += sizeof(int) * Hcap;
  return (o + 15) & ~(size_t)15;
}

struct HvLds {
  double rv[HV_WAVES];
  double hpl[HV_HZ_LDS][4];
  int ri[HV_WAVES];
  int vis[HV_VIS_LDS];
  int ha[HV_HZ_LDS], hb[HV_HZ_LDS];
  int nvis, nh, err, pending;
};

// the order of every arg-max here: the larger value, on equal values the smaller index
__device__ inline void hv_take(double& bv, int& bi, double v, int i) {
  if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// arg-max over the workgroup, the result in every lane (ends with a barrier: the next reduction may reuse L.rv / L.ri)
__device__ inline void hv_argmax(double& bv, int& bi, HvLds& L) {
  for (int w = 32; w > 0; w >>= 1) {
    const double ov = __shfl_xor(bv, w, 64);
    const int oi = __shfl_xor(bi, w, 64);
    hv_take(bv, bi, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) { L.rv[threadIdx.x >> 6] = bv; L.ri[threadIdx.x >> 6] = bi; }
  __syncthreads();
  bv = L.rv[0]; bi = L.ri[0];
  for (int w = 1; w < HV_WAVES; ++w) hv_take(bv, bi, L.rv[w], L.ri[w]);
  __syncthreads();
}

__device__ inline double hv_plane(const double* pl, double x, double y, double z) {
  return ((pl[0] * x + pl[1] * y) + pl[2] * z) + pl[3];
}

// the plane of face (a, b, c): n = (b - a) x (c - a), off = -n . a
__device__ inline void hv_make_plane(const double* P, int a, int b, int c, double* pl) {
  const double ax = P[3 * (size_t)a], ay = P[3 * (size_t)a + 1], az = P[3 * (size_t)a + 2];
  const double ex = P[3 * (size_t)b] - ax, ey = P[3 * (size_t)b + 1] - ay, ez = P[3 * (size_t)b + 2] - az;
  const double fx = P[3 * (size_t)c] - ax, fy = P[3 * (size_t)c + 1] - ay, fz = P[3 * (size_t)c + 2] - az;
  pl[0] = ey * fz - ez * fy;
  pl[1] = ez * fx - ex * fz;
  pl[2] = ex * fy - ey * fx;
  pl[3] = -((pl[0] * ax + pl[1] * ay) + pl[2] * az);
}

__device__ inline int hv_vis_get(const HvSlab& S, const HvLds& L, int k) { return k < HV_VIS_LDS ? L.vis[k] : S.vis[k]; }

// one view in the workgroup's slab -> its status, the same in every lane; on HV_OK assign[i] == HV_VERTEX marks the hull's vertices
__device__ int hv_view(const HvParams& p, int view, const HvSlab& S, HvLds& L) {
  const int tid = threadIdx.x, V = p.V, N = V + 1, Fcap = 2 * V - 2, Hcap = Fcap + 2;
  const double inf = __builtin_inf();
  double r[9], tt[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) r[k] = p.R[9 * (size_t)view + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) tt[k] = p.t[(size_t)p.t_stride * view + k];

  // 1. the largest norm, then the flip
  double mx = 0.0;
  int bad = 0;
  for (int i = tid; i < V; i += HV_THREADS) {
    const double x = p.pts[3 * (size_t)i], y = p.pts[3 * (size_t)i + 1], z = p.pts[3 * (size_t)i + 2];
    const double cx = ((r[0] * x + r[1] * y) + r[2] * z) + tt[0];
    const double cy = ((r[3] * x + r[4] * y) + r[5] * z) + tt[1];
    const double cz = ((r[6] * x + r[7] * y) + r[8] * z) + tt[2];
    const double nr = sqrt((cx * cx + cy * cy) + cz * cz);
    if (!(nr > 0.0) || !(nr < inf)) bad = 1;
    mx = fmax(mx, nr);
  }
  {
    int none = INT_MAX;
    hv_argmax(mx, none, L);
  }
  if (__syncthreads_or(bad)) return HV_NORM;
  const double radius = mx * p.scale;
  if (!(radius < inf)) return HV_NORM;
  for (int i = tid; i < V; i += HV_THREADS) {
    const double x = p.pts[3 * (size_t)i], y = p.pts[3 * (size_t)i + 1], z = p.pts[3 * (size_t)i + 2];
    const double cx = ((r[0] * x + r[1] * y) + r[2] * z) + tt[0];
    const double cy = ((r[3] * x + r[4] * y) + r[5] * z) + tt[1];
    const double cz = ((r[6] * x + r[7] * y) + r[8] * z) + tt[2];
    const double nr = sqrt((cx * cx + cy * cy) + cz * cz);
    const double s2 = 2 * (radius - nr);
    double* o = S.P + 3 * (size_t)(i + 1);
    o[0] = cx + s2 * (cx / nr);
    o[1] = cy + s2 * (cy / nr);
    o[2] = cz + s2 * (cz / nr);
  }
  if (tid == 0) { S.P[0] = 0.0; S.P[1] = 0.0; S.P[2] = 0.0; }
  for (int i = tid; i < N; i += HV_THREADS) { S.assign[i] = HV_NONE; S.mark[i] = -1; }
  __syncthreads();

  // 2. the initial tetrahedron
  double bv = -inf;
  int bi = INT_MAX;
  for (int i = tid; i < N; i += HV_THREADS) hv_take(bv, bi, -S.P[3 * (size_t)i], i);
  hv_argmax(bv, bi, L);
  const int i0 = bi;
  bv = -inf; bi = INT_MAX;
  for (int i = tid; i < N; i += HV_THREADS) hv_take(bv, bi, S.P[3 * (size_t)i], i);
  hv_argmax(bv, bi, L);
  const int i1 = bi;
  if (i0 < 0 || i0 >= N || i1 < 0 || i1 >= N) return HV_DEGENERATE;      // (not with finite coordinates; keeps every read in bounds)
  if (!(S.P[3 * (size_t)i1] > S.P[3 * (size_t)i0])) return HV_DEGENERATE;
  const double ax = S.P[3 * (size_t)i0], ay = S.P[3 * (size_t)i0 + 1], az = S.P[3 * (size_t)i0 + 2];
  const double ex = S.P[3 * (size_t)i1] - ax, ey = S.P[3 * (size_t)i1 + 1] - ay, ez = S.P[3 * (size_t)i1 + 2] - az;
  bv = -inf; bi = INT_MAX;
  for (int i = tid; i < N; i += HV_THREADS) {
    const double dx = S.P[3 * (size_t)i] - ax, dy = S.P[3 * (size_t)i + 1] - ay, dz = S.P[3 * (size_t)i + 2] - az;
    const double cx = dy * ez - dz * ey, cy = dz * ex - dx * ez, cz = dx * ey - dy * ex;
    hv_take(bv, bi, (cx * cx + cy * cy) + cz * cz, i);
  }
  hv_argmax(bv, bi, L);
  const int i2 = bi;
  if (i2 < 0 || i2 >= N || !(bv > 0.0)) return HV_DEGENERATE;
  {
    const double fx = S.P[3 * (size_t)i2] - ax, fy = S.P[3 * (size_t)i2 + 1] - ay, fz = S.P[3 * (size_t)i2 + 2] - az;
    const double nx = ey * fz - ez * fy, ny = ez * fx - ex * fz, nz = ex * fy - ey * fx;
    bv = -inf; bi = INT_MAX;
    for (int i = tid; i < N; i += HV_THREADS) {
      const double dx = S.P[3 * (size_t)i] - ax, dy = S.P[3 * (size_t)i + 1] - ay, dz = S.P[3 * (size_t)i + 2] - az;
      hv_take(bv, bi, fabs((nx * dx + ny * dy) + nz * dz), i);
    }
  }
  hv_argmax(bv, bi, L);
  const int i3 = bi;
  if (i3 < 0 || i3 >= N || !(bv > 0.0)) return HV_DEGENERATE;
  if (tid == 0) {
    const int tv[4] = {i0, i1, i2, i3};
    int ok = 1;
    for (int f = 0; f < 4; ++f) {                                          // face f leaves vertex 3 - f out
      const int opp = tv[3 - f];
      int a = tv[f == 3 ? 1 : 0], b = tv[f >= 2 ? 2 : 1], c = tv[f == 0 ? 2 : 3];
      double pl[4];
      hv_make_plane(S.P, a, b, c, pl);
      if (hv_plane(pl, S.P[3 * (size_t)opp], S.P[3 * (size_t)opp + 1], S.P[3 * (size_t)opp + 2]) > 0.0) {
        const int s = b; b = c; c = s;
        hv_make_plane(S.P, a, b, c, pl);
      }
      if (!(hv_plane(pl, S.P[3 * (size_t)opp], S.P[3 * (size_t)opp + 1], S.P[3 * (size_t)opp + 2]) < 0.0)) ok = 0;
      S.fv[3 * f] = a; S.fv[3 * f + 1] = b; S.fv[3 * f + 2] = c;
      for (int k = 0; k < 4; ++k) S.fpl[4 * f + k] = pl[k];
      S.state[f] = HV_LIVE;
      S.assign[tv[f]] = HV_VERTEX;
    }
    L.err = ok ? 0 : 1;
  }
  __syncthreads();
  const int tet_bad = L.err;
  __syncthreads();
  if (tet_bad) return HV_DEGENERATE;

  // 3. the first assignment
  for (int i = tid; i < N; i += HV_THREADS) {
    if (S.assign[i] == HV_VERTEX) continue;
    const double x = S.P[3 * (size_t)i], y = S.P[3 * (size_t)i + 1], z = S.P[3 * (size_t)i + 2];
    for (int f = 0; f < 4; ++f)
      if (hv_plane(S.fpl + 4 * f, x, y, z) > 0.0) { S.assign[i] = f; break; }
  }
  __syncthreads();

  // 4. insertions
  int nslots = 4, cursor = 0, st = HV_ITERATIONS;
  for (int iter = 0; iter <= N; ++iter) {
    int q = -1;
    for (int step = 0; step <= N / HV_THREADS && cursor < N; ++step) {     // the lowest-index pending point, from the cursor on
      if (tid == 0) L.pending = INT_MAX;
      __syncthreads();
      const int i = cursor + tid;
      if (i < N && S.assign[i] >= 0) atomicMin(&L.pending, i);
      __syncthreads();
      const int m = L.pending;
      __syncthreads();
      if (m != INT_MAX) { q = m; cursor = m; break; }
      cursor += HV_THREADS;
    }
    if (q < 0) { st = HV_OK; break; }
    if (iter == N) break;                                                  // more insertions than points
    const int F = S.assign[q];
    if (F < 0 || F >= nslots) { st = HV_HORIZON; break; }
    double pl[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pl[k] = S.fpl[4 * (size_t)F + k];
    bv = -inf; bi = INT_MAX;
    for (int i = tid; i < N; i += HV_THREADS) hv_take(bv, bi, hv_plane(pl, S.P[3 * (size_t)i], S.P[3 * (size_t)i + 1], S.P[3 * (size_t)i + 2]), i);
    hv_argmax(bv, bi, L);
    const int pi = bi;
    if (pi < 0 || pi >= N || !(bv > 0.0)) { st = HV_HORIZON; break; }
    const double px = S.P[3 * (size_t)pi], py = S.P[3 * (size_t)pi + 1], pz = S.P[3 * (size_t)pi + 2];
    if (tid == 0) { L.nvis = 0; L.nh = 0; L.err = 0; }
    __syncthreads();
    for (int f = tid; f < nslots; f += HV_THREADS) {                       // the visible set: every live face with p above it
      if (S.state[f] == HV_LIVE && hv_plane(S.fpl + 4 * (size_t)f, px, py, pz) > 0.0) {
        const int k = atomicAdd(&L.nvis, 1);
        if (k < HV_VIS_LDS) L.vis[k] = f; else S.vis[k] = f;               // (k < nslots <= Fcap)
        S.state[f] = HV_RETIRED;
      }
    }
    __syncthreads();
    const int v = L.nvis;
    for (int e = tid; e < 3 * v; e += HV_THREADS) {                        // the horizon: edges whose reverse no visible face has
      const int f = hv_vis_get(S, L, e / 3), j = e % 3;
      const int a = S.fv[3 * (size_t)f + j], b = S.fv[3 * (size_t)f + (j + 1) % 3];
      bool found = false;
      for (int g = 0; g < v && !found; ++g) {
        const int* w = S.fv + 3 * (size_t)hv_vis_get(S, L, g);
        found = (w[0] == b && w[1] == a) || (w[1] == b && w[2] == a) || (w[2] == b && w[0] == a);
      }
      if (found) continue;
      const int k = atomicAdd(&L.nh, 1);
      if (atomicExch(&S.mark[a], iter) == iter) atomicOr(&L.err, 1);       // a start point twice: not a simple cycle
      if (k >= Hcap) continue;                                             // (counted: HV_TABLE_FULL below)
      double hp[4];
      hv_make_plane(S.P, a, b, pi, hp);
      if (k < HV_HZ_LDS) {
        L.ha[k] = a; L.hb[k] = b;
        for (int c = 0; c < 4; ++c) L.hpl[k][c] = hp[c];
      } else {
        S.ha[k] = a; S.hb[k] = b;
        for (int c = 0; c < 4; ++c) S.hpl[4 * (size_t)k + c] = hp[c];
      }
    }
    __syncthreads();
    const int h = L.nh, herr = L.err;
    if (herr || h < 3) { st = HV_HORIZON; break; }
    const int extra = h > v ? h - v : 0;
    if (h > Hcap || nslots + extra > Fcap) { st = HV_TABLE_FULL; break; }
    for (int i = tid; i < N; i += HV_THREADS) {                            // the points of retired faces against the staged faces
      const int f = S.assign[i];
      if (f < 0 || S.state[f] != HV_RETIRED) continue;
      const double x = S.P[3 * (size_t)i], y = S.P[3 * (size_t)i + 1], z = S.P[3 * (size_t)i + 2];
      int best = -1, ba = INT_MAX;
      double bval = 0.0;
      for (int k = 0; k < h; ++k) {
        const double val = hv_plane(k < HV_HZ_LDS ? L.hpl[k] : S.hpl + 4 * (size_t)k, x, y, z);
        if (!(val > 0.0)) continue;
        const int a = k < HV_HZ_LDS ? L.ha[k] : S.ha[k];
        if (best < 0 || val > bval || (val == bval && a < ba)) { best = k; bval = val; ba = a; }
      }
      S.assign[i] = best < 0 ? HV_NONE : (best < v ? hv_vis_get(S, L, best) : nslots + (best - v));
    }
    __syncthreads();
    if (tid == 0) S.assign[pi] = HV_VERTEX;
    const int kmax = h > v ? h : v;
    for (int k = tid; k < kmax; k += HV_THREADS) {                         // staged faces take the retired slots, then fresh ones
      if (k >= h) { S.state[hv_vis_get(S, L, k)] = HV_DEAD; continue; }
      const int slot = k < v ? hv_vis_get(S, L, k) : nslots + (k - v);
      S.fv[3 * (size_t)slot] = k < HV_HZ_LDS ? L.ha[k] : S.ha[k];
      S.fv[3 * (size_t)slot + 1] = k < HV_HZ_LDS ? L.hb[k] : S.hb[k];
      S.fv[3 * (size_t)slot + 2] = pi;
      for (int c = 0; c < 4; ++c) S.fpl[4 * (size_t)slot + c] = k < HV_HZ_LDS ? L.hpl[k][c] : S.hpl[4 * (size_t)k + c];
      S.state[slot] = HV_LIVE;
    }
    nslots += extra;
    __syncthreads();
  }
  return st;
}

__global__ __launch_bounds__(HV_THREADS) void hpr_visibility_kernel(HvParams p) {
  __shared__ HvLds L;
  HvSlab S;
  hv_carve(p.V, p.scratch + (size_t)blockIdx.x * p.wg_bytes, &S);
  const int nrounds = (p.n_views + p.G - 1) / p.G;
  for (int round = 0; round < nrounds; ++round) {
    const int view = round * p.G + (int)blockIdx.x;
    if (view >= p.n_views) break;                                          // (uniform)
    const int st = hv_view(p, view, S, L);
    __syncthreads();
    for (int i = threadIdx.x; i < p.V; i += HV_THREADS) {
      const int vis = (st == HV_OK && S.assign[i + 1] == HV_VERTEX) ? 1 : 0;
      if (p.mask) p.mask[(size_t)view * p.V + i] = (uint8_t)vis;
      if (vis) atomicAdd(&p.counts[i], 1);
    }
    if (threadIdx.x == 0) p.status[view] = st;
    __syncthreads();
  }
}

int hv_groups(int n_views, int V, int workgroups) {
  if (workgroups > 0) return workgroups < n_views ? workgroups : n_views;
  size_t cap = HV_AUTO_BYTES / hv_carve(V, nullptr, nullptr);
  cap = cap < 1 ? 1 : (cap > (size_t)HV_AUTO_WG ? (size_t)HV_AUTO_WG : cap);
  return (size_t)n_views < cap ? n_views : (int)cap;
}

}  // namespace

extern "C" size_t cp_hpr_visibility_scratch_bytes(int n_views, int V, int workgroups) {
  if (n_views < 1 || V < 4 || V > HV_MAX_V || workgroups < 0 || workgroups > HV_MAX_WG) return 0;
  return hv_carve(V, nullptr, nullptr) * (size_t)hv_groups(n_views, V, workgroups);
}

extern "C" int cp_hpr_visibility(cp_stream_t stream, const double* pts, const double* R, const double* t, int t_stride, int n_views,
                                 int V, double radius_param, int workgroups, int32_t* counts, uint8_t* mask, int32_t* status,
                                 void* scratch) {
  if (!pts || !R || !t || !counts || !status || !scratch) return CP_ERR_INVALID;
  if (n_views < 1 || V < 4 || workgroups < 0 || (t_stride != 0 && t_stride != 3)) return CP_ERR_INVALID;
  if (!(radius_param >= 0.0 && radius_param <= 8.0)) return CP_ERR_INVALID;                  // (NaN fails both comparisons)
  if (((uintptr_t)pts & 7) || ((uintptr_t)R & 7) || ((uintptr_t)t & 7) || ((uintptr_t)scratch & 7) || ((uintptr_t)counts & 3) ||
      ((uintptr_t)status & 3))
    return CP_ERR_ALIGN;
  if (V > HV_MAX_V || workgroups > HV_MAX_WG) return CP_ERR_RANGE;
  HvParams p;
  p.pts = pts; p.R = R; p.t = t; p.counts = counts; p.mask = mask; p.status = status; p.scratch = (char*)scratch;
  p.wg_bytes = hv_carve(V, nullptr, nullptr);
  p.scale = pow(10.0, radius_param);
  p.t_stride = t_stride; p.n_views = n_views; p.V = V; p.G = hv_groups(n_views, V, workgroups);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)V, st) != hipSuccess) return CP_ERR_HIP;
  CP_LAUNCH(hpr_visibility_kernel, dim3((unsigned)p.G), dim3(HV_THREADS), 0, st, p);
  return cp_check_launch();
}
