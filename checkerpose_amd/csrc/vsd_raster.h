// The tile-raster scaffold of the rows that render a mesh under a pose: vsd_error.hip (row N8), gt_info.hip (N10), mask_error.hip (N12)
// and render_rgb.hip (N14).  All four run a pose kernel, a vertex kernel, a 32 x 32 tile kernel and a finish (or sum) kernel; what these
// share lives here, once.  The .hip files keep their kernels, params structs, per-pixel counting or shading, and entry points.
//
// Render rule.  depth[y, x] = the smallest eye-space Z > 0 at which the ray through image point (x + 0.5, y + 0.5) meets a triangle
// (no back-face culling, background 0), Z taken on the triangle's plane: 1 / Z is affine in the image.  Triangles of zero area
// are skipped.  A pose with any vertex at Z <= 0 is not rendered.
//
//   VsHdr<SIDES>    the words every pose header starts with: P, rectangle and "a vertex at Z <= 0" flag per side, ok; then the file's own
//   vs_finite, vs_pose_finite, vs_side_init, vs_sphere_skip             the pose kernels' prologue
//   vs_krt          P = K' [R | t] in double WITHOUT contraction, rounded to fp32 once (K' = fx, fy, cx, cy of K, skew 0)
//   vs_project      a vertex -> screen (u, v, Z, 1 / Z) in fp32 with explicit fma chains, and the pixels its sample can reach
//   vs_rect_merge   a wave's pixel rectangle / "a vertex at Z <= 0" flag into the pose's header through INTEGER atomics
//   vs_vertex_block, vs_vertex_chunk                          the vertex kernels' body
//   VsTile, vs_tile_hit                                       a workgroup's tile, a lane's pixels of it, "does the rectangle meet it"
//   vs_raster_tile  a workgroup owns a 32 x 32 pixel tile, a lane 4 pixels of it.  The mesh's triangles are set up 256 at a time: the
//                   ones whose bounding box meets the tile are compacted into LDS as 16 floats (three edge functions and the 1 / Z
//                   plane as affine functions of the TILE-RELATIVE sample index, so fp32 keeps sub-pixel resolution wherever the
//                   tile lies -- also left of or above the frame), then every wave walks the list with broadcast reads and a
//                   wave-uniform reject against its 32 x 8 strip.  max(1 / Z) over triangles is exact in any order, so the order
//                   in which the list is compacted does not reach the result; neither does the image size or the batch.
//                   <true> also keeps the winning face: of triangles with equal 1 / Z the SMALLEST index, again whatever the order.
//   vs_depth_of, vs_depth_tile                                1 / Z -> depth by one correctly rounded division
//   vs_dist         misc.depth_im_to_dist_im_fast at a pixel; vs_visible: visibility.py's 'bop19' test
//   vs_acc_identity, vs_acc_combine, vs_acc_waves, vs_acc_reduce     NSUM integer sums, then groups of min min max max
//   vs_box_xywh     xmin ymin xmax ymax -> x, y, w, h, or -1 four times
//   VsMesh, vs_mesh_rows                                      the mesh table of a call and one pose's rows of it
//   vs_image_rows   an image's rows of the image-to-poses CSR (vis_poses.hip, scene_labels.hip)
//   vs_mesh_invalid / _misaligned, vs_view_invalid / _misaligned, vs_images_invalid, vs_csr_invalid / _over     (host) the entry
//                   points' argument rules, by error class
//   vs_grid         (host) the tile grid, the vertex chunks and the block counts of a call
#pragma once
#include "common.h"

namespace {

constexpr int VS_THREADS = 256;
constexpr int VS_TILE = 32;                      // pixels per tile side
constexpr int VS_PPL = 4;                        // pixels per lane: VS_TILE * VS_TILE / VS_THREADS
constexpr int VS_WAVES = VS_THREADS / 64;
constexpr int VS_STRIP = VS_TILE / VS_WAVES;     // rows per wave (8)
constexpr int VS_CHUNK = 256;                    // triangles set up per round (16 KiB of LDS)

// 4-byte words at the start of a pose's header, SIDES = 1 (a pose) or 2 (estimate, ground truth): P[SIDES][12] rect[SIDES][4]
// bad[SIDES] ok, then the file's own words from USER on
template <int SIDES>
struct VsHdr {
  static constexpr int P(int s) { return 12 * s; }
  static constexpr int RECT(int s) { return 12 * SIDES + 4 * s; }          // xmin ymin xmax ymax
  static constexpr int BAD(int s) { return 16 * SIDES + s; }
  static constexpr int OK = 17 * SIDES;
  static constexpr int USER = 17 * SIDES + 1;
};

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

// a[0 .. n) are finite; K (3x3) and the pose rows q (12) are
__device__ inline bool vs_finite(const double* __restrict__ a, int n) {
  bool ok = true;
  for (int k = 0; k < n; ++k) ok = ok && isfinite(a[k]);
  return ok;
}
__device__ inline bool vs_pose_finite(const double* __restrict__ K, const double* __restrict__ q) { return vs_finite(K, 9) && vs_finite(q, 12); }

__device__ inline void vs_rect_set(int32_t* __restrict__ rect, int x0, int y0, int x1, int y1) {
  rect[0] = x0; rect[1] = y0; rect[2] = x1; rect[3] = y1;
}

// one side of a pose's header: P under K * scale (scale 1, 2 or 4: exact), the rectangle empty
__device__ inline void vs_side_init(const double* __restrict__ K, double scale, const double* __restrict__ q, float* __restrict__ P,
                                    int32_t* __restrict__ rect) {
#pragma clang fp contract(off)
  vs_rect_set(rect, INT_MAX, INT_MAX, INT_MIN, INT_MIN);
  vs_krt(K[0] * scale, K[4] * scale, K[2] * scale, K[5] * scale, q, P);
}

// 1 unless misc.overlapping_sphere_projections(radius, t_est, t_gt) (misc.py:309-331), as eval_calc_errors.py:299-318 calls it
__device__ inline int vs_sphere_skip(const double* __restrict__ e, const double* __restrict__ g, double radius) {
#pragma clang fp contract(off)
  bool overlap = false;
  if (!(e[11] == 0.0 || g[11] == 0.0)) {
    const double dx = e[9] / e[11] - g[9] / g[11], dy = e[10] / e[11] - g[10] / g[11];
    overlap = sqrt(dx * dx + dy * dy) < radius * (1.0 / e[11] + 1.0 / g[11]);
  }
  return overlap ? 0 : 1;
}

// The mesh table of a call.  It must stay the FIRST member of every raster row's params struct: where the member stands changes
// hipcc's register allocation of the tile kernels.  Checked on the host by vs_mesh_invalid / vs_mesh_misaligned below.
struct VsMesh {
  const float* verts;         // (sumV, 3)
  const int32_t* v_off;       // (M + 1)
  const int32_t* faces;       // (sumF, 3), indices local to the mesh
  const int32_t* f_off;       // (M + 1)
  const int32_t* mesh_id;     // per pose, or nullptr: mesh 0
  int M, Vmax;
};

// mesh m = mesh_id[b] (0 without ids): its rows of the vertex and face tables; false when the id or the tables are out of range.
// (M and Vmax are read first, together: one scalar load of the kernel's arguments.)
__device__ inline bool vs_mesh_rows(const VsMesh& t, int b, int& vfirst, int& V, int& ffirst, int& F, int& m) {
  vfirst = 0; V = 0; ffirst = 0; F = 0;
  const int M = t.M, Vmax = t.Vmax;
  m = t.mesh_id ? t.mesh_id[b] : 0;
  if (m < 0 || m >= M) return false;
  vfirst = t.v_off[m];
  V = t.v_off[m + 1] - vfirst;
  ffirst = t.f_off[m];
  F = t.f_off[m + 1] - ffirst;
  if (vfirst < 0 || V <= 0 || V > Vmax || ffirst < 0 || F < 0) { V = 0; F = 0; return false; }
  return true;
}

// image img's rows [j0, j1) of the image-to-poses CSR, clamped to [0, P] and, with `cap`, to that many rows (the host checked them --
// vs_csr_invalid, vs_csr_over --; the clamps bound the loops, and scene_labels' shifts, whatever the memory holds)
__device__ __forceinline__ void vs_image_rows(const int32_t* __restrict__ img_off, int P, int img, int& j0, int& j1) {
  j0 = min(max(img_off[img], 0), P);
  j1 = min(max(img_off[img + 1], j0), P);
}
__device__ __forceinline__ void vs_image_rows(const int32_t* __restrict__ img_off, int P, int img, int cap, int& j0, int& j1) {
  vs_image_rows(img_off, P, img, j0, j1);
  j1 = min(j1, j0 + cap);
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

// a vertex kernel's workgroup (blockIdx.x = (b * nsides + s) * vchunks + vc) -> its pose, side and chunk of 256 vertices
__device__ __forceinline__ void vs_vertex_block(int vchunks, int nsides, int& b, int& s, int& vc) {
  int blk = blockIdx.x;
  vc = blk % vchunks;
  blk /= vchunks;
  s = blk % nsides;
  b = blk / nsides;
}

// The body of a vertex kernel, for ALL threads of a live pose's workgroup: vertex i = vc * 256 + threadIdx.x of the mesh's V (verts:
// its first) under the side's P -> sv[i], with the sample's pixels clamped to clip = (xlo, xhi, ylo, yhi); then more(i, vertex) for
// what else the caller keeps per vertex; then the side's rectangle and flag.
template <typename More>
__device__ __forceinline__ void vs_vertex_chunk(const float* __restrict__ P, const float* __restrict__ verts, int V, int vc, float4 clip,
                                                float4* __restrict__ sv, int32_t* __restrict__ rect, int32_t* __restrict__ bad_word,
                                                More more) {
#pragma clang fp contract(off)
  const int i = vc * VS_THREADS + threadIdx.x;
  int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN, bad = 0;
  if (i < V) {
    const float* __restrict__ vt = verts + 3 * (size_t)i;
    sv[i] = vs_project(P, vt, clip.x, clip.y, clip.z, clip.w, x0, y0, x1, y1, bad);
    more(i, vt);
  }
  vs_rect_merge(x0, y0, x1, y1, bad, rect, bad_word);
}
__device__ __forceinline__ void vs_vertex_chunk(const float* __restrict__ P, const float* __restrict__ verts, int V, int vc, float4 clip,
                                                float4* __restrict__ sv, int32_t* __restrict__ rect, int32_t* __restrict__ bad_word) {
  vs_vertex_chunk(P, verts, V, vc, clip, sv, rect, bad_word, [](int, const float*) {});
}

// A tile kernel's workgroup (blockIdx.x = b * tx * ty + t) and thread: pose b, tile t with its first pixel at (ox, oy) (any sign: the
// grid starts at (x0, y0)); the lane's pixels are (lx, y(k)) of the tile, k = 0..3, two rows apart inside the wave's 32 x 8 strip.
struct VsTile {
  int tid, lane, wave, lx, ly0, b, t, ox, oy;
  __device__ __forceinline__ int y(int k) const { return ly0 + 2 * k; }
};
__device__ __forceinline__ VsTile vs_tile(int tx, int ty, int x0, int y0) {
  VsTile c;
  c.tid = threadIdx.x; c.lane = c.tid & 63; c.wave = c.tid >> 6;
  c.lx = c.lane & 31; c.ly0 = c.wave * VS_STRIP + (c.lane >> 5);
  const int tiles = tx * ty;
  c.b = blockIdx.x / tiles; c.t = blockIdx.x % tiles;
  c.ox = x0 + (c.t % tx) * VS_TILE; c.oy = y0 + (c.t / tx) * VS_TILE;
  return c;
}

// the pose's rectangle (xmin ymin xmax ymax) meets the tile whose first pixel is (ox, oy)
__device__ __forceinline__ bool vs_tile_hit(const int32_t* __restrict__ rect, int ox, int oy) {
  return rect[0] <= ox + VS_TILE - 1 && rect[2] >= ox && rect[1] <= oy + VS_TILE - 1 && rect[3] >= oy;
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

// Tile c of one mesh under one pose: best[k] = the largest 1 / Z at the lane's pixel (c.lx, c.y(k)), 0 = background; with FACE also
// face[k] = the face it comes from (the smallest index among equals; INT_MAX = background).  Called by ALL threads of the workgroup
// (it holds barriers); s_tri / s_n are the caller's LDS.
//   sv: the pose's screen records (vs_project), faces: the mesh's rows (indices local to the mesh, checked against V)
template <bool FACE>
__device__ __forceinline__ void vs_raster_tile(float4 (*__restrict__ s_tri)[4], int* __restrict__ s_n, const float4* __restrict__ sv,
                                               const int32_t* __restrict__ faces, int F, int V, const VsTile c, float (&best_out)[VS_PPL],
                                               int (&face_out)[VS_PPL]) {
  const float fx0 = (float)c.ox + 0.5f, fy0 = (float)c.oy + 0.5f;   // the tile's first sample point (exact in fp32)
  const float wy0 = (float)(c.wave * VS_STRIP), wy1 = wy0 + (float)(VS_STRIP - 1);
  // (without FACE the maxima live in locals and are copied out at the end, with FACE the walk works on the caller's arrays: as the two
  // walks did before they became one.  In the other form hipcc compiles the update below differently -- selects instead of branches
  // without FACE -- and a full device measured slower: cp_gt_info at B = 256 by 9 %, cp_render_rgb by 1 - 2 %.)
  float best_local[VS_PPL];
  int face_local[VS_PPL];
  float (&best)[VS_PPL] = FACE ? best_out : best_local;
  int (&face)[VS_PPL] = FACE ? face_out : face_local;
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) { best[k] = 0.f; face[k] = INT_MAX; }     // max is exact in any order
  for (int f0 = 0; f0 < F; f0 += VS_CHUNK) {
    __syncthreads();
    if (c.tid == 0) *s_n = 0;
    __syncthreads();
    const int f = f0 + c.tid;
    if (f < F) {
#pragma clang fp contract(off)
      const int32_t* __restrict__ fi = faces + 3 * (size_t)f;
      const int i0 = fi[0], i1 = fi[1], i2 = fi[2];
      if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
        const float4 a = sv[i0], c1 = sv[i1], d = sv[i2];
        const float ax = a.x - fx0, ay = a.y - fy0, cx = c1.x - fx0, cy = c1.y - fy0, dx = d.x - fx0, dy = d.y - fy0;
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
          const float g1 = (c1.w - a.w) * ia, g2 = (d.w - a.w) * ia;
          const float pa = e1a * g1 + e2a * g2, pb = e1b * g1 + e2b * g2, pc = a.w + (e1c * g1 + e2c * g2);
          const int at = atomicAdd(s_n, 1);
          s_tri[at][0] = make_float4(sg * e0a, sg * e0b, sg * e0c, ymin);
          s_tri[at][1] = make_float4(sg * e1a, sg * e1b, sg * e1c, ymax);
          s_tri[at][2] = make_float4(sg * e2a, sg * e2b, sg * e2c, FACE ? __int_as_float(f) : 0.f);      // the spare word
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
      int fj = 0;
      if constexpr (FACE) fj = __builtin_amdgcn_readfirstlane(__float_as_int(q2.w));
      const float qx = (float)c.lx;
#pragma unroll
      for (int k = 0; k < VS_PPL; ++k) {
        const float qy = (float)c.y(k);
        const float w0 = fmaf(q0.x, qx, fmaf(q0.y, qy, q0.z));
        const float w1 = fmaf(q1.x, qx, fmaf(q1.y, qy, q1.z));
        const float w2 = fmaf(q2.x, qx, fmaf(q2.y, qy, q2.z));
        const float iz = fmaf(q3.x, qx, fmaf(q3.y, qy, q3.z));
        if constexpr (FACE) {
          if (w0 >= 0.f && w1 >= 0.f && w2 >= 0.f && iz > 0.f && (iz > best[k] || (iz == best[k] && fj < face[k]))) {
            best[k] = iz;
            face[k] = fj;
          }
        } else {
          if (w0 >= 0.f && w1 >= 0.f && w2 >= 0.f && iz > best[k]) best[k] = iz;      // (best >= 0: iz > 0 is implied)
        }
      }
    }
  }
  if constexpr (!FACE) {
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) best_out[k] = best[k];
  }
}

// the depth of a pixel from its largest 1 / Z: one correctly rounded division, 0 = background
__device__ __forceinline__ float vs_depth_of(float best) { return best > 0.f ? 1.0f / best : 0.f; }

// vs_raster_tile without the faces: dep[k] = the depth of the lane's pixel (c.lx, c.y(k)) (the same call rules)
__device__ __forceinline__ void vs_depth_tile(float4 (*__restrict__ s_tri)[4], int* __restrict__ s_n, const float4* __restrict__ sv,
                                              const int32_t* __restrict__ faces, int F, int V, const VsTile& c, float (&dep)[VS_PPL]) {
  int face[VS_PPL];
  vs_raster_tile<false>(s_tri, s_n, sv, faces, F, V, c, dep, face);
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) dep[k] = vs_depth_of(dep[k]);
}

// ---- integer accumulators: values 0 .. NSUM - 1 are sums, the rest come in groups of four: min min max max (a box xmin ymin xmax ymax)
template <int NSUM>
__device__ __forceinline__ int vs_acc_identity(int k) { return k < NSUM ? 0 : (((k - NSUM) & 3) < 2 ? INT_MAX : INT_MIN); }
template <int NSUM>
__device__ __forceinline__ int vs_acc_combine(int k, int a, int b) {
  return k < NSUM ? a + b : (((k - NSUM) & 3) < 2 ? min(a, b) : max(a, b));
}

// every wave's combination of its lanes' acc -> s_red[wave] (wave shuffles), then a barrier.  ALL threads of the workgroup.
template <int NSUM, int N>
__device__ __forceinline__ void vs_acc_waves(const int (&acc)[N], int (*__restrict__ s_red)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    int v = acc[k];
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v = vs_acc_combine<NSUM>(k, v, __shfl_xor(v, w, 64));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
}

// a tile's accumulators into the pose's dst[N]: one atomicAdd / Min / Max per value, none for a value at its identity (integers:
// the order in which tiles arrive does not reach the result).  ALL threads of a VS_THREADS workgroup.
template <int NSUM, int N>
__device__ __forceinline__ void vs_acc_reduce(const int (&acc)[N], int (*__restrict__ s_red)[N], int32_t* __restrict__ dst) {
  vs_acc_waves<NSUM, N>(acc, s_red);
  if (threadIdx.x < N) {
    const int k = threadIdx.x;
    int v = s_red[0][k];
    for (int w = 1; w < VS_WAVES; ++w) v = vs_acc_combine<NSUM>(k, v, s_red[w][k]);
    if (v != vs_acc_identity<NSUM>(k)) {
      if (k < NSUM) atomicAdd(dst + k, v);
      else if (((k - NSUM) & 3) < 2) atomicMin(dst + k, v);
      else atomicMax(dst + k, v);
    }
  }
}

// r = xmin ymin xmax ymax -> out = x, y, xmax - xmin, ymax - ymin (no + 1), or -1 four times without a box
__device__ __forceinline__ void vs_box_xywh(const int32_t* __restrict__ r, bool have, int32_t* __restrict__ out) {
  out[0] = have ? r[0] : -1;
  out[1] = have ? r[1] : -1;
  out[2] = have ? r[2] - r[0] : -1;
  out[3] = have ? r[3] - r[1] : -1;
}

// ---- host side
// An entry point's argument rules by error class, as predicates: every entry point returns CP_ERR_INVALID when one of the *_invalid
// (and its own INVALID rules) holds, then CP_ERR_ALIGN for the *_misaligned (and its own), then, with an image-to-poses CSR,
// CP_ERR_INVALID for vs_csr_invalid, then CP_ERR_RANGE for its size rules (vs_csr_over, vs_grid, its own pixel bound).

// the mesh table: a table missing, no mesh or no vertex row, no ids although there are several meshes;  then its alignment
inline bool vs_mesh_invalid(const VsMesh& t) {
  return !t.verts || !t.v_off || !t.faces || !t.f_off || t.M <= 0 || t.Vmax <= 0 || (!t.mesh_id && t.M != 1);
}
inline bool vs_mesh_misaligned(const VsMesh& t) {
  return cp_misaligned(t.verts, 3) || cp_misaligned(t.v_off, 3) || cp_misaligned(t.faces, 3) || cp_misaligned(t.f_off, 3) ||
         cp_misaligned(t.mesh_id, 3);
}
// the camera (one K: k_stride 0, or one per pose or image: k_stride 9) and the frame: H, W and the count of poses positive
inline bool vs_view_invalid(const double* K, int k_stride, int H, int W, int count) {
  return !K || (k_stride != 0 && k_stride != 9) || H <= 0 || W <= 0 || count <= 0;
}
inline bool vs_view_misaligned(const double* K) { return cp_misaligned(K, 7); }
// the images that poses are scored against: none, or no ids although there are several
inline bool vs_images_invalid(const int32_t* image_ids, int I) { return I <= 0 || (!image_ids && I != 1); }
// the image-to-poses CSR (host copies) is no monotone partition of [0, P), or an entry of pose_order is no pose;  vs_csr_over: an image
// has more than `cap` poses
inline bool vs_csr_invalid(const int32_t* img_off, const int32_t* pose_order, int I, int P) {
  if (img_off[0] != 0 || img_off[I] != P) return true;
  for (int i = 0; i < I; ++i)
    if (img_off[i + 1] < img_off[i]) return true;
  for (int j = 0; j < P; ++j)
    if (pose_order[j] < 0 || pose_order[j] >= P) return true;
  return false;
}
inline bool vs_csr_over(const int32_t* img_off, int I, int cap) {
  for (int i = 0; i < I; ++i)
    if (img_off[i + 1] - img_off[i] > cap) return true;
  return false;
}

// The launch plan of B poses with `nsides` sides on a W x H frame sampled f x f per pixel: tx x ty tiles starting at pixel (x0, y0),
// vchunks vertex chunks.  canvas: gt_info's grid over [-W, 2W) x [-H, 2H), anchored so that frame pixel (0, 0) is a tile corner.
// False when a kernel's block count would reach 2^24.  (The callers bound W, H, f first: nothing overflows here.)
struct VsGrid { int tx, ty, x0, y0, vchunks; unsigned pose_blocks, vert_blocks, tile_blocks; };
inline bool vs_grid(int W, int H, int f, bool canvas, int B, int nsides, int Vmax, VsGrid& g) {
  const long long fx = ((long long)f * W + VS_TILE - 1) / VS_TILE, fy = ((long long)f * H + VS_TILE - 1) / VS_TILE;      // the frame's tiles
  const long long tx = canvas ? fx + (2LL * W + VS_TILE - 1) / VS_TILE : fx, ty = canvas ? fy + (2LL * H + VS_TILE - 1) / VS_TILE : fy;
  g.vchunks = (Vmax + VS_THREADS - 1) / VS_THREADS;
  const long long vert_blocks = (long long)B * nsides * g.vchunks;
  if (tx >= (1LL << 24) || ty >= (1LL << 24) || tx * ty >= (1LL << 24) || (long long)B * tx * ty >= (1LL << 24) || vert_blocks >= (1LL << 24))
    return false;
  g.tx = (int)tx; g.ty = (int)ty;
  g.x0 = canvas ? -VS_TILE * (int)fx : 0; g.y0 = canvas ? -VS_TILE * (int)fy : 0;
  g.pose_blocks = (unsigned)((B + VS_THREADS - 1) / VS_THREADS);
  g.vert_blocks = (unsigned)vert_blocks; g.tile_blocks = (unsigned)(B * tx * ty);
  return true;
}

}  // namespace
