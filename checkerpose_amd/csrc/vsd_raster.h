// The depth rasteriser and the reference's per-pixel distance / visibility arithmetic, shared by vsd_error.hip (row N8) and
// gt_info.hip (row N10).  Device functions only: the kernels, their launch lists and their reductions stay in the two .hip files.
//
// Render rule.  depth[y, x] = the smallest eye-space Z > 0 at which the ray through image point (x + 0.5, y + 0.5) meets a triangle
// (no back-face culling, background 0), Z taken on the triangle's plane: 1 / Z is affine in the image.  Triangles of zero area
// are skipped.  A pose with any vertex at Z <= 0 is not rendered.
//
//   vs_krt          P = K' [R | t] in double WITHOUT contraction, rounded to fp32 once (K' = fx, fy, cx, cy of K, skew 0)
//   vs_project      a vertex -> screen (u, v, Z, 1 / Z) in fp32 with explicit fma chains, and the pixels its sample can reach
//   vs_rect_merge   a wave's pixel rectangle / "a vertex at Z <= 0" flag into the pose's header through INTEGER atomics
//   vs_raster_tile  a workgroup owns a 32 x 32 pixel tile, a lane 4 pixels of it.  The mesh's triangles are set up 256 at a time: the
//                   ones whose bounding box meets the tile are compacted into LDS as 16 floats (three edge functions and the 1 / Z
//                   plane as affine functions of the TILE-RELATIVE sample index, so fp32 keeps sub-pixel resolution wherever the
//                   tile lies -- also left of or above the frame), then every wave walks the list with broadcast reads and a
//                   wave-uniform reject against its 32 x 8 strip.  max(1 / Z) over triangles is exact in any order, so the order
//                   in which the list is compacted does not reach the result; neither does the image size or the batch.
//   vs_dist         misc.depth_im_to_dist_im_fast at a pixel; vs_visible: visibility.py's 'bop19' test
#pragma once
#include "common.h"

namespace {

constexpr int VS_THREADS = 256;
constexpr int VS_TILE = 32;                      // pixels per tile side
constexpr int VS_PPL = 4;                        // pixels per lane: VS_TILE * VS_TILE / VS_THREADS
constexpr int VS_STRIP = VS_TILE / (VS_THREADS / 64);   // rows per wave (8)
constexpr int VS_CHUNK = 256;                    // triangles set up per round (16 KiB of LDS)

__device__ inline double vs_dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
#pragma clang fp contract(off)
  return (a0 * b0 + a1 * b1) + a2 * b2;
}

// P = [[fx 0 cx] [0 fy cy] [0 0 1]] [R | t] in double -> fp32 (3x4 row-major)
__device__ inline void vs_krt(double fx, double fy, double cx, double cy, const double* q, float* __restrict__ P) {
#pragma clang fp contract(off)
  for (int c = 0; c < 4; ++c) {
    const double r0 = c < 3 ? q[c] : q[9], r1 = c < 3 ? q[3 + c] : q[10], r2 = c < 3 ? q[6 + c] : q[11];
    P[c] = (float)vs_dot3(fx, 0.0, cx, r0, r1, r2);
    P[4 + c] = (float)vs_dot3(0.0, fy, cy, r0, r1, r2);
    P[8 + c] = (float)r2;
  }
}

// mesh m = mesh_id[b] (0 without ids): its rows of the vertex and face tables; false when the id or the tables are out of range
__device__ inline bool vs_mesh_rows(const int32_t* __restrict__ mesh_id, const int32_t* __restrict__ v_off,
                                    const int32_t* __restrict__ f_off, int M, int Vmax, int b, int& vfirst, int& V, int& ffirst, int& F,
                                    int& m) {
  vfirst = 0; V = 0; ffirst = 0; F = 0;
  m = mesh_id ? mesh_id[b] : 0;
  if (m < 0 || m >= M) return false;
  vfirst = v_off[m];
  V = v_off[m + 1] - vfirst;
  ffirst = f_off[m];
  F = f_off[m + 1] - ffirst;
  if (vfirst < 0 || V <= 0 || V > Vmax || ffirst < 0 || F < 0) { V = 0; F = 0; return false; }
  return true;
}

// row . (x, y, z, 1): one fma chain
__device__ __forceinline__ float vs_affine(const float* __restrict__ r, float x, float y, float z) {
  return fmaf(r[2], z, fmaf(r[1], y, fmaf(r[0], x, r[3])));
}

// one vertex under P (3x4 fp32): its screen record, and either bad = 1 (Z <= 0 or a non-finite coordinate) or the pixels whose
// sample can lie at (u, v), clamped IN FLOAT to [xlo, xhi] x [ylo, yhi] first (the rectangle is only ever used to skip work)
__device__ __forceinline__ float4 vs_project(const float* __restrict__ P, const float* __restrict__ vt, float xlo, float xhi, float ylo,
                                             float yhi, int& x0, int& y0, int& x1, int& y1, int& bad) {
#pragma clang fp contract(off)
  const float x = vt[0], y = vt[1], z = vt[2];
  const float pu = vs_affine(P, x, y, z), pv = vs_affine(P + 4, x, y, z), pw = vs_affine(P + 8, x, y, z);
  const float iz = 1.0f / pw;
  const float u = pu / pw, v = pv / pw;
  if (!(pw > 0.f) || !isfinite(u) || !isfinite(v)) {
    bad = 1;
  } else {
    // pixel x is sampled at x + 0.5: the pixels whose sample can lie inside [u_min, u_max]
    const float cu = fminf(fmaxf(u - 0.5f, xlo), xhi), cv = fminf(fmaxf(v - 0.5f, ylo), yhi);
    x0 = (int)floorf(cu); x1 = (int)ceilf(cu);
    y0 = (int)floorf(cv); y1 = (int)ceilf(cv);
  }
  return make_float4(u, v, pw, iz);
}

// the lanes' rectangles and flags -> rect[0..3] = xmin ymin xmax ymax and *bad_word of the pose (order-independent integer atomics)
__device__ __forceinline__ void vs_rect_merge(int x0, int y0, int x1, int y1, int bad, int32_t* __restrict__ rect,
                                              int32_t* __restrict__ bad_word) {
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    x0 = min(x0, __shfl_xor(x0, w, 64)); y0 = min(y0, __shfl_xor(y0, w, 64));
    x1 = max(x1, __shfl_xor(x1, w, 64)); y1 = max(y1, __shfl_xor(y1, w, 64));
    bad |= __shfl_xor(bad, w, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (x0 != INT_MAX) {
      atomicMin(rect, x0); atomicMin(rect + 1, y0);
      atomicMax(rect + 2, x1); atomicMax(rect + 3, y1);
    }
    if (bad) atomicOr(bad_word, 1);
  }
}

// the reference's depth_im_to_dist_im_fast at pixel (x, y): integer x, y (NOT the sample point), float64 throughout
__device__ __forceinline__ double vs_dist(double px, double py, float d) {
#pragma clang fp contract(off)
  const double dd = (double)d;
  const double a = px * dd, c = py * dd;
  return sqrt((a * a + c * c) + dd * dd);
}

// _estimate_visib_mask, 'bop19': (f32(dist_model) - f32(dist_test) <= delta or dist_test == 0) and dist_model > 0
__device__ __forceinline__ bool vs_visible(double dist_test, double dist_model, float delta) {
#pragma clang fp contract(off)
  const float diff = (float)dist_model - (float)dist_test;
  return (diff <= delta || dist_test == 0.0) && dist_model > 0.0;
}

// The tile with its first pixel at (ox, oy) (any sign) of one mesh under one pose: dep[k] = the depth of the lane's pixel
// (lx, ly0 + 2 k), 0 = background.  Called by ALL threads of the workgroup (it holds barriers); s_tri / s_n are the caller's LDS.
//   sv: the pose's screen records (vs_project), faces: the mesh's rows (indices local to the mesh, checked against V)
__device__ __forceinline__ void vs_raster_tile(float4 (*__restrict__ s_tri)[4], int* __restrict__ s_n, const float4* __restrict__ sv,
                                               const int32_t* __restrict__ faces, int F, int V, int ox, int oy, int tid, int lx, int ly0,
                                               int wave, float (&dep)[VS_PPL]) {
  const float fx0 = (float)ox + 0.5f, fy0 = (float)oy + 0.5f;     // the tile's first sample point (exact in fp32)
  const float wy0 = (float)(wave * VS_STRIP), wy1 = wy0 + (float)(VS_STRIP - 1);
  float best[VS_PPL];
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) best[k] = 0.f;                   // the largest 1 / Z so far: max is exact in any order
  for (int f0 = 0; f0 < F; f0 += VS_CHUNK) {
    __syncthreads();
    if (tid == 0) *s_n = 0;
    __syncthreads();
    const int f = f0 + tid;
    if (f < F) {
#pragma clang fp contract(off)
      const int32_t* __restrict__ fi = faces + 3 * (size_t)f;
      const int i0 = fi[0], i1 = fi[1], i2 = fi[2];
      if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
        const float4 a = sv[i0], c = sv[i1], d = sv[i2];
        const float ax = a.x - fx0, ay = a.y - fy0, cx = c.x - fx0, cy = c.y - fy0, dx = d.x - fx0, dy = d.y - fy0;
        const float xmin = fminf(ax, fminf(cx, dx)), xmax = fmaxf(ax, fmaxf(cx, dx));
        const float ymin = fminf(ay, fminf(cy, dy)), ymax = fmaxf(ay, fmaxf(cy, dy));
        // twice the signed area; its sign turns every edge function non-negative inside
        const float area = (cx - ax) * (dy - ay) - (dx - ax) * (cy - ay);
        if (area != 0.f && xmax >= 0.f && xmin <= (float)(VS_TILE - 1) && ymax >= 0.f && ymin <= (float)(VS_TILE - 1)) {
          const float sg = area > 0.f ? 1.f : -1.f, ia = 1.0f / area;
          // edge i is opposite vertex i: E(q) = (x_b - x_a)(q_y - y_a) - (y_b - y_a)(q_x - x_a)
          const float e0a = -(dy - cy), e0b = dx - cx, e0c = (dy - cy) * cx - (dx - cx) * cy;     // c -> d
          const float e1a = -(ay - dy), e1b = ax - dx, e1c = (ay - dy) * dx - (ax - dx) * dy;     // d -> a
          const float e2a = -(cy - ay), e2b = cx - ax, e2c = (cy - ay) * ax - (cx - ax) * ay;     // a -> c
          // 1 / Z = iz_a + (E1 (iz_c - iz_a) + E2 (iz_d - iz_a)) / area
          const float g1 = (c.w - a.w) * ia, g2 = (d.w - a.w) * ia;
          const float pa = e1a * g1 + e2a * g2, pb = e1b * g1 + e2b * g2, pc = a.w + (e1c * g1 + e2c * g2);
          const int at = atomicAdd(s_n, 1);
          s_tri[at][0] = make_float4(sg * e0a, sg * e0b, sg * e0c, ymin);
          s_tri[at][1] = make_float4(sg * e1a, sg * e1b, sg * e1c, ymax);
          s_tri[at][2] = make_float4(sg * e2a, sg * e2b, sg * e2c, 0.f);
          s_tri[at][3] = make_float4(pa, pb, pc, 0.f);
        }
      }
    }
    __syncthreads();
    const int n = *s_n;
    for (int j = 0; j < n; ++j) {
      const float4 q0 = s_tri[j][0], q1 = s_tri[j][1];           // every lane reads the same address: a broadcast
      const float tymin = __builtin_amdgcn_readfirstlane(q0.w), tymax = __builtin_amdgcn_readfirstlane(q1.w);
      if (tymax < wy0 || tymin > wy1) continue;                  // wave-uniform: the triangle misses this wave's strip
      const float4 q2 = s_tri[j][2], q3 = s_tri[j][3];
      const float qx = (float)lx;
#pragma unroll
      for (int k = 0; k < VS_PPL; ++k) {
        const float qy = (float)(ly0 + 2 * k);
        const float w0 = fmaf(q0.x, qx, fmaf(q0.y, qy, q0.z));
        const float w1 = fmaf(q1.x, qx, fmaf(q1.y, qy, q1.z));
        const float w2 = fmaf(q2.x, qx, fmaf(q2.y, qy, q2.z));
        const float iz = fmaf(q3.x, qx, fmaf(q3.y, qy, q3.z));
        if (w0 >= 0.f && w1 >= 0.f && w2 >= 0.f && iz > best[k]) best[k] = iz;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) dep[k] = best[k] > 0.f ? 1.0f / best[k] : 0.f;      // one correctly rounded division per pixel
}

}  // namespace
