// Silhouette refinement of poses against the network's own predicted masks, on the device: the RGB-only twin of
// row N24 (icp_refine.hip), which needs the sensor's depth.  An RGB-only pose is weakest along the viewing ray; the extent of the mask
// fixes the scale of the projection and so the depth.  The operand is a coco_eval.PackedMasks of bit rows, as row N27's cp_paste_masks
// leaves the full (amodal) mask.  The reference does not refine: the row is opt-in, and its rule is this project's OWN
// (tests/mask_refine_stages.py restates it in numpy; parity with any contour tracker is UNPINNED).
//
// THE RULE.  Everything after the render in fp64 without contraction.  fx, fy, cx, cy = K[0], K[4], K[2], K[5].
//
// Mask extents (cp_mask_extents), per mask of NM packed masks (pixel x of a row = bit x & 31 of word x >> 5 of its WW = ceil(W / 32) words):
//   row[y] = (first, last) set column of row y; col[x] = (first, last) set row of column x; (-1, -1) where there is none.  Bits at
//   columns >= W of the last word are ignored.  Integer only, no atomics, every output word written once.
//
// Stage A, contour samples of a pose (cp_contour_samples; ONE raster pass at the INPUT pose).  The render and its refusals are
//   vsd_raster.h's.  The lattice is row N24's: rect = the pose's merged vertex rectangle intersected with the frame, w x h pixels from
//   (x0, y0); nx = min(grid, w), ny = min(grid, h), grid in 1..64; lattice column i is pixel x0 + ((2 i + 1) w) / (2 nx), rows likewise.
//   S = 4 grid slots per pose.  Lattice row j at frame row y: slot 2 j = the FIRST covered pixel of row y (D > 0, anywhere in the frame),
//   slot 2 j + 1 = the LAST.  Lattice column i at frame column x: slot 2 grid + 2 i = the TOPMOST covered pixel of column x, slot
//   2 grid + 2 i + 1 = the BOTTOMMOST.  A slot is empty (pixel -1 -1, depth 0, X NaN) when its line holds no covered pixel, or the pixel
//   lies on the frame's first / last column (row kinds) or first / last row (column kinds): there the contour is the frame's edge, not
//   the object's.  A sample is its pixel (x, y), the render's fp32 depth d,
//   Qr = (((x + 0.5 - cx) d) / fx, ((y + 0.5 - cy) d) / fy, d) and X = R^T (Qr - t).
//   The extremes are merged across tiles by 64-bit INTEGER atomicMin / atomicMax on the key (coordinate << 32) | depth bits: the column
//   (or row) decides, the depth of that one pixel rides along, so a slot's content depends neither on launch order nor on the batch.
//
// Stage B, association under (R, t), per sample:  Y = R X, C = Y + t; reject unless C_z > 0;  a_u = (fx C_x) / C_z, u = a_u + cx,
//   a_v = (fy C_y) / C_z, v = a_v + cy; pixel (px, py) = (floor u, floor v); reject outside the frame.  Row kinds: m = row[mask][py][kind]
//   (first for a left sample, last for a right one); reject when m < 0 or m is the frame's first / last column; b = m + 0.5, r = u - b,
//   g = (fx / C_z, 0, -(a_u / C_z)).  Column kinds: m = col[mask][px][kind], the frame's first / last row, r = v - b,
//   g = (0, fy / C_z, -(a_v / C_z)).  Reject unless |r| <= max_dist (pixels).  The pair keeps (axis, b) frozen until the next
//   association.  n = the number of pairs.
//
// Stage C, Levenberg-Marquardt over the pairs, in row N22's form: increment (w, v) with R' = exp([w]x) R, t' = t + v; r_i as above
//   with b_i fixed; J_i = [(Y_i x g_i)^T, g_i^T]; H = sum J^T J, g = sum J^T r, c = sum r^2; lambda = 1e-3.  At most max_iters (1..64) times:
//     1. solve (H + lambda diag H) d = -g by Cholesky (one thread).  dof "t": only the 3 x 3 translation block is solved (the rotation
//        block is replaced by the identity and its coupling and gradient by zeros, which leaves the factorisation of the translation
//        block exactly the 3 x 3 one), w = 0 and R' is BITWISE R;
//     2. not positive definite: rejected with c' = +inf, the trial recorded as NaN;
//     3. else c' = the cost of the trial over the SAME pairs; a C_z <= 0 or a value that is not finite counts as +inf;
//     4. accept iff c' < c: the state becomes the trial, lambda = max(lambda / 10, 1e-12), stage B runs again;
//     5. n < min_pairs after the re-association: stop with status 3;
//     6. not accepted: lambda = 10 lambda; lambda > 1e8 stops with status 3;
//     7. an ACCEPTED step with s = max(|w|_inf, |v|_inf / |t|) <= step_tol stops with status 1;
//     8. the iterations run out: status 2.
//   pass-through (status 0: the output pose BITWISE the input, info NaN but for the counts): status_in == 0; a pose or K entry not
//     finite; a mesh or mask id out of range; a refused render (both leave `ok` 0 and no sample); fewer than min_pairs (>= 6) pairs
//     under the input pose.
//   info      42 doubles: [c at the input pose, c at the returned pose, samples, pairs at the input pose, pairs at the returned pose,
//             iterations, H (36): the undamped J^T J at the returned pose over its pairs].
//   records   18 doubles per executed iteration: [lambda used, n, c, c', accepted 0/1, s, R' (9), t' (3)]; other slots are not written.
//
// Stage A is the scaffold's pose, vertex and 32 x 32 tile kernels and a finish pass.  In the tile kernel a frame row is held by the 32
// lanes of a half wave: one ballot finds its first and last covered lane, which alone issue the two atomics; a column's extremes are
// folded over the lane's four rows and the wave's two halves first.  Stages B and C are ONE launch, one 256-thread workgroup per pose:
// S <= 256, so a thread owns one slot and keeps its pair (flag, b) in registers; pnp_core.h's block_sum joins the 21 + 6 + 1 + 1 sums
// in a fixed order; thread 0 runs lm_load_lower / lm_solve_step (L in LDS) and publishes the trial through LDS.  The extents of the
// pose's one mask (8 (H + W) bytes) come from L2.  No floating-point atomics, no scratch memory, no per-thread arrays beyond what
// unrolls into registers.  Every branch on accept / stop is taken on block_sum results or LDS words that all threads hold identically;
// every loop is bounded by max_iters; no workgroup waits for another.
#include "pnp_core.h"
#include "vsd_raster.h"

#pragma clang fp contract(off)

namespace {

constexpr int MR_REC = 18, MR_INFO = 42, MR_MAX_ITERS = 64, MR_SUMS = 29, MR_GRID_MAX = 64;      // sums: H (21), g (6), c, n
using MrH = VsHdr<1>;
constexpr int MR_HDR = 24;                       // 4-byte words per pose (the rest is spare)
typedef unsigned long long mr_key_t;
constexpr mr_key_t MR_NONE_MIN = ~0ULL, MR_NONE_MAX = 0ULL;      // the identities of the first / last keys (a real key has depth bits > 0)

// ------------------------------------------------------------------------------------------------------------- mask extents
// item < H: row `item` of the mask; else column item - H.  One thread per item, nothing shared.
__global__ __launch_bounds__(256) void mask_extents_kernel(const uint32_t* __restrict__ bits, int NM, int H, int W, int WW, int chunks,
                                                           int32_t* __restrict__ row, int32_t* __restrict__ col) {
  const int n = blockIdx.x / chunks, item = (blockIdx.x % chunks) * 256 + threadIdx.x;
  if (n >= NM || item >= H + W) return;
  const uint32_t* __restrict__ m = bits + (size_t)n * H * WW;
  const uint32_t tail = (W & 31) ? ((1u << (W & 31)) - 1u) : 0xffffffffu;      // the last word's columns < W
  int first = -1, last = -1;
  if (item < H) {
    const uint32_t* __restrict__ r = m + (size_t)item * WW;
    for (int w = 0; w < WW; ++w) {
      const uint32_t v = r[w] & (w == WW - 1 ? tail : 0xffffffffu);
      if (v) { first = 32 * w + __ffs((int)v) - 1; break; }
    }
    for (int w = WW - 1; w >= 0 && first >= 0; --w) {
      const uint32_t v = r[w] & (w == WW - 1 ? tail : 0xffffffffu);
      if (v) { last = 32 * w + 31 - __clz((int)v); break; }
    }
    row[((size_t)n * H + item) * 2] = first; row[((size_t)n * H + item) * 2 + 1] = last;
  } else {
    const int x = item - H, sh = x & 31;
    const uint32_t* __restrict__ c = m + (x >> 5);                              // (x < W: never a bit beyond the frame)
    for (int y = 0; y < H; ++y)
      if ((c[(size_t)y * WW] >> sh) & 1u) { first = y; break; }
    for (int y = H - 1; y >= 0 && first >= 0; --y)
      if ((c[(size_t)y * WW] >> sh) & 1u) { last = y; break; }
    col[((size_t)n * W + x) * 2] = first; col[((size_t)n * W + x) * 2 + 1] = last;
  }
}

// ------------------------------------------------------------------------------------------------------------------- stage A
struct McParams {
  VsMesh mesh;
  const double* poses;        // (P, 12)
  const double* K;
  int32_t* rect;              // (P, 4)
  int32_t* shape;             // (P, 2)
  int32_t* pixel;             // (P, S, 2)
  float* depth;               // (P, S)
  double* X;                  // (P, S, 3)
  int32_t* ok;                // (P)
  int32_t* hdr;               // (P, MR_HDR)
  mr_key_t* keys;             // (P, S)
  float4* sv;                 // (P, Vmax)
  int k_stride, P, H, W, grid, tx, ty, vchunks;
};

// row N24's lattice (icp_refine.hip: ss_lattice, ss_offset, ss_index), restated: that file keeps its own in its own namespace
struct MrLattice { int x0, y0, w, h, nx, ny; };
__device__ __forceinline__ MrLattice mr_lattice(const int32_t* __restrict__ rect, int W, int H, int grid) {
  MrLattice l = {0, 0, 0, 0, 0, 0};
  if (rect[0] == INT_MAX) return l;              // no vertex merged
  const int x0 = max(rect[0], 0), y0 = max(rect[1], 0), x1 = min(rect[2], W - 1), y1 = min(rect[3], H - 1);
  if (x0 > x1 || y0 > y1) return l;
  l.x0 = x0; l.y0 = y0; l.w = x1 - x0 + 1; l.h = y1 - y0 + 1;
  l.nx = min(grid, l.w); l.ny = min(grid, l.h);
  return l;
}
__device__ __forceinline__ int mr_offset(int i, int e, int n) { return (int)(((2LL * i + 1) * e) / (2LL * n)); }
__device__ __forceinline__ int mr_index(int d, int e, int n) {                 // the lattice coordinate whose pixel lies d behind the first, or -1
  if (d < 0 || d >= e || n <= 0) return -1;
  const int i0 = (int)(((long long)d * n) / e);
  if (mr_offset(i0, e, n) == d) return i0;
  if (i0 + 1 < n && mr_offset(i0 + 1, e, n) == d) return i0 + 1;
  return -1;
}
__device__ __forceinline__ mr_key_t mr_key(int coord, float dep) { return ((mr_key_t)(uint32_t)coord << 32) | (mr_key_t)__float_as_uint(dep); }

__global__ __launch_bounds__(VS_THREADS) void contour_pose_kernel(McParams p) {
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * MR_HDR;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  const double* __restrict__ q = p.poses + 12 * (size_t)b;
  int vfirst, V, ffirst, F, m;
  bool ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  ok = ok && vs_pose_finite(K, q);
  vs_side_init(K, 1.0, q, (float*)h + MrH::P(0), h + MrH::RECT(0));
  h[MrH::BAD(0)] = 0;
  h[MrH::OK] = ok ? 1 : 0;
  const int S = 4 * p.grid;
  mr_key_t* __restrict__ keys = p.keys + (size_t)b * S;
  for (int s = 0; s < S; ++s) keys[s] = (s & 1) ? MR_NONE_MAX : MR_NONE_MIN;
}

__global__ __launch_bounds__(VS_THREADS) void contour_vertex_kernel(McParams p) {
  int b, s, vc;
  vs_vertex_block(p.vchunks, 1, b, s, vc);
  int32_t* __restrict__ h = p.hdr + (size_t)b * MR_HDR;
  if (!h[MrH::OK]) return;                                            // (uniform; no barrier in this kernel)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  vs_vertex_chunk((const float*)h + MrH::P(0), p.mesh.verts + 3 * (size_t)vfirst, V, vc, make_float4(-2.f, (float)p.W + 1.f, -2.f, (float)p.H + 1.f),
                  p.sv + (size_t)b * p.mesh.Vmax, h + MrH::RECT(0), h + MrH::BAD(0));
}

__global__ __launch_bounds__(VS_THREADS) void contour_tile_kernel(McParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  const VsTile c = vs_tile(p.tx, p.ty, 0, 0);
  const int b = c.b;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * MR_HDR;
  const bool live = h[MrH::OK] && !h[MrH::BAD(0)];
  if (!live || !vs_tile_hit(h + MrH::RECT(0), c.ox, c.oy)) return;    // (uniform) every covered pixel lies in a tile the rectangle meets
  const MrLattice l = mr_lattice(h + MrH::RECT(0), p.W, p.H, p.grid);
  if (l.nx == 0) return;                                              // (uniform)
  float dep[VS_PPL];
  {
    const VsMesh mesh = p.mesh;
    int vfirst, V, ffirst, F, m;
    vs_mesh_rows(mesh, b, vfirst, V, ffirst, F, m);
    vs_depth_tile(s_tri, &s_n, p.sv + (size_t)b * mesh.Vmax, mesh.faces + 3 * (size_t)ffirst, F, V, c, dep);
  }
  mr_key_t* __restrict__ keys = p.keys + (size_t)b * 4 * p.grid;      // slots 2 j (+ 1) < 2 ny <= 2 grid; 2 grid + 2 i (+ 1) < 4 grid
  const int x = c.ox + c.lx, half = c.lane >> 5;
  mr_key_t top = MR_NONE_MIN, bottom = MR_NONE_MAX;                   // the lane's column over its four rows
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) {
    const int y = c.oy + c.y(k);
    const bool in = x < p.W && y < p.H && dep[k] > 0.f;
    const unsigned long long lanes = __ballot(in);                    // (all 64 lanes arrive: no divergent exit above)
    const uint32_t mine = (uint32_t)(lanes >> (32 * half));           // the 32 lanes that hold frame row y
    const int j = y < p.H ? mr_index(y - l.y0, l.h, l.ny) : -1;
    if (in) {
      const mr_key_t ky = mr_key(y, dep[k]);
      top = ky < top ? ky : top;
      bottom = ky > bottom ? ky : bottom;
      if (j >= 0) {
        if (c.lx == __ffs((int)mine) - 1) atomicMin(keys + 2 * j, mr_key(x, dep[k]));
        if (c.lx == 31 - __clz((int)mine)) atomicMax(keys + 2 * j + 1, mr_key(x, dep[k]));
      }
    }
  }
  const mr_key_t top2 = __shfl_xor(top, 32), bottom2 = __shfl_xor(bottom, 32);      // the wave's other four rows of this column
  top = top2 < top ? top2 : top;
  bottom = bottom2 > bottom ? bottom2 : bottom;
  if (half == 0 && bottom != MR_NONE_MAX) {
    const int i = mr_index(x - l.x0, l.w, l.nx);                      // (bottom set: x < W)
    if (i >= 0) {
      atomicMin(keys + 2 * p.grid + 2 * i, top);
      atomicMax(keys + 2 * p.grid + 2 * i + 1, bottom);
    }
  }
}

// per pose: rect, shape, ok; per slot: pixel, depth and X of a contour sample, or the empty slot
__global__ __launch_bounds__(VS_THREADS) void contour_finish_kernel(McParams p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * MR_HDR;
  const bool live = h[MrH::OK] && !h[MrH::BAD(0)];
  MrLattice l = {0, 0, 0, 0, 0, 0};
  if (live) l = mr_lattice(h + MrH::RECT(0), p.W, p.H, p.grid);
  const int S = 4 * p.grid;
  if (tid == 0) {
    const bool have = l.nx > 0;
    int32_t* r = p.rect + 4 * (size_t)b;
    r[0] = have ? l.x0 : -1; r[1] = have ? l.y0 : -1; r[2] = have ? l.x0 + l.w - 1 : -1; r[3] = have ? l.y0 + l.h - 1 : -1;
    p.shape[2 * (size_t)b] = l.nx; p.shape[2 * (size_t)b + 1] = l.ny;
    p.ok[b] = live ? 1 : 0;
  }
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  const double* __restrict__ q = p.poses + 12 * (size_t)b;
  for (int slot = tid; slot < S; slot += VS_THREADS) {
    const size_t at = (size_t)b * S + slot;
    const bool column = slot >= 2 * p.grid, far = (slot & 1) != 0;
    const int line = (slot - (column ? 2 * p.grid : 0)) >> 1;
    const mr_key_t key = p.keys[at];
    bool have = line < (column ? l.nx : l.ny) && key != (far ? MR_NONE_MAX : MR_NONE_MIN);
    int px = -1, py = -1;
    float dep = 0.f;
    double X[3] = {NAN, NAN, NAN};
    if (have) {
      const int a = (int)(uint32_t)(key >> 32);
      if (column) { px = l.x0 + mr_offset(line, l.w, l.nx); py = a; have = a != 0 && a != p.H - 1; }
      else { py = l.y0 + mr_offset(line, l.h, l.ny); px = a; have = a != 0 && a != p.W - 1; }
    }
    if (have) {
      dep = __uint_as_float((uint32_t)key);
      const double fx = K[0], fy = K[4], cx = K[2], cy = K[5], d = (double)dep;
      const double Q[3] = {(((double)px + 0.5 - cx) * d) / fx, (((double)py + 0.5 - cy) * d) / fy, d};
      const double e[3] = {Q[0] - q[9], Q[1] - q[10], Q[2] - q[11]};
      for (int k = 0; k < 3; ++k) X[k] = vs_dot3(q[k], q[3 + k], q[6 + k], e[0], e[1], e[2]);
    } else {
      px = -1; py = -1;
    }
    p.pixel[2 * at] = px; p.pixel[2 * at + 1] = py;
    p.depth[at] = dep;
    for (int k = 0; k < 3; ++k) p.X[3 * at + k] = X[k];
  }
}

// ------------------------------------------------------------------------------------------------------------ stages B and C
struct MrParams {
  const double* pose_in; const double* K; const double* X; const int32_t* pixel; const int32_t* ok;
  const int32_t* row; const int32_t* col; const int32_t* mask_ids; const double* max_dist; const int32_t* status_in;
  double* pose_out; int32_t* status_out; double* info; double* records;
  int k_stride, P, grid, NM, H, W, dof, max_iters, min_pairs;
  double step_tol;
};

struct MrSlot {                  // the thread's one slot, its mask line table and camera
  const int32_t* ext;            // row[mask] (row kinds) or col[mask] (column kinds)
  double X0, X1, X2, fx, fy, cx, cy, max_dist;
  int H, W, far;                 // far: 1 = the last / bottommost extent
  bool sample, column;
};

// stage B for the thread's sample under (R, t): false = no pair; else Y = R X, C_z, a = (f C_axis) / C_z, r, b
__device__ __forceinline__ bool mr_associate(const MrSlot& s, const double* R, const double* t, double* Y, double& Cz, double& a, double& r, double& b) {
  if (!s.sample) return false;
  Y[0] = R[0] * s.X0 + R[1] * s.X1 + R[2] * s.X2; Y[1] = R[3] * s.X0 + R[4] * s.X1 + R[5] * s.X2; Y[2] = R[6] * s.X0 + R[7] * s.X1 + R[8] * s.X2;
  const double C0 = Y[0] + t[0], C1 = Y[1] + t[1], C2 = Y[2] + t[2];
  if (!(C2 > 0.0)) return false;
  const double au = (s.fx * C0) / C2, av = (s.fy * C1) / C2;
  const double u = au + s.cx, v = av + s.cy;
  if (!(u >= 0.0 && u < (double)s.W && v >= 0.0 && v < (double)s.H)) return false;      // (a NaN fails here; floor(u) <= W - 1)
  const int px = (int)floor(u), py = (int)floor(v);
  const int m = s.ext[2 * (s.column ? px : py) + s.far];
  if (m <= 0 || m == (s.column ? s.H : s.W) - 1) return false;                          // none, or the frame's first / last line
  b = (double)m + 0.5;
  r = (s.column ? v : u) - b;
  if (!(fabs(r) <= s.max_dist)) return false;
  Cz = C2; a = s.column ? av : au;
  return true;
}

// the thread's terms under the state: acc[0..20] the upper triangle of J^T J row by row, [21..26] J^T r, [27] r^2, [28] 1; zeros without a pair
__device__ __forceinline__ void mr_terms(const MrSlot& s, bool pair, const double* Y, double Cz, double a, double r, double* acc) {
#pragma unroll
  for (int k = 0; k < MR_SUMS; ++k) acc[k] = 0.0;
  if (!pair) return;
  const double ga = (s.column ? s.fy : s.fx) / Cz, g2 = -(a / Cz);
  const double g0 = s.column ? 0.0 : ga, g1 = s.column ? ga : 0.0;
  const double J[6] = {Y[1] * g2 - Y[2] * g1, Y[2] * g0 - Y[0] * g2, Y[0] * g1 - Y[1] * g0, g0, g1, g2};
  int e = 0;
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int q = p; q < 6; ++q) { acc[e] = J[p] * J[q]; ++e; }
#pragma unroll
  for (int p = 0; p < 6; ++p) acc[21 + p] = J[p] * r;
  acc[27] = r * r;
  acc[28] = 1.0;
}

// the thread's squared residual at the trial (Rn, tn) with its pair's (axis, b) frozen; +inf behind the camera
__device__ __forceinline__ double mr_trial_term(const MrSlot& s, bool pair, double b, const double* Rn, const double* tn) {
  if (!pair) return 0.0;
  const double C0 = (Rn[0] * s.X0 + Rn[1] * s.X1 + Rn[2] * s.X2) + tn[0], C1 = (Rn[3] * s.X0 + Rn[4] * s.X1 + Rn[5] * s.X2) + tn[1],
               C2 = (Rn[6] * s.X0 + Rn[7] * s.X1 + Rn[8] * s.X2) + tn[2];
  if (!(C2 > 0.0)) return INFINITY;
  const double w = s.column ? (s.fy * C1) / C2 + s.cy : (s.fx * C0) / C2 + s.cx;
  const double r = w - b;
  return r * r;
}

__global__ __launch_bounds__(PNP_THREADS) void mask_refine_kernel(const MrParams p) {
  __shared__ double sred[4 * MR_SUMS];
  __shared__ double s_H[MR_SUMS];                                             // the state's H (21), g (6), c, n: written and read by thread 0
  __shared__ double s_L[6][6], s_g[6], s_trial[19];
  __shared__ int s_kind;
  const int b = blockIdx.x, tid = threadIdx.x, S = 4 * p.grid;
  const double* K = p.K + (size_t)p.k_stride * b;
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = p.pose_in[(size_t)b * 12 + i];
  for (int i = 0; i < 3; ++i) t[i] = p.pose_in[(size_t)b * 12 + 9 + i];
  double* const pose_out = p.pose_out + (size_t)b * 12;
  double* const info = p.info + (size_t)b * MR_INFO;
  const int mask = p.mask_ids ? p.mask_ids[b] : b;
  bool pass = (p.status_in && p.status_in[b] == 0) || mask < 0 || mask >= p.NM || p.ok[b] == 0;      // every thread reads the same words: uniform
  for (int i = 0; i < 9; ++i) pass = pass || !isfinite(R[i]) || !isfinite(K[i]);
  for (int i = 0; i < 3; ++i) pass = pass || !isfinite(t[i]);
  MrSlot s;
  s.column = tid >= 2 * p.grid; s.far = tid & 1;
  s.H = p.H; s.W = p.W;
  s.fx = K[0]; s.fy = K[4]; s.cx = K[2]; s.cy = K[5]; s.max_dist = p.max_dist[b];
  {
    const size_t m = (size_t)(pass ? 0 : mask);
    s.ext = s.column ? p.col + m * p.W * 2 : p.row + m * p.H * 2;
    const size_t at = (size_t)b * S + (tid < S ? tid : 0);
    s.sample = tid < S && p.pixel[2 * at] >= 0;
    s.X0 = p.X[3 * at]; s.X1 = p.X[3 * at + 1]; s.X2 = p.X[3 * at + 2];
  }
  double ns[1] = {s.sample ? 1.0 : 0.0};
  block_sum<1>(ns, sred, tid);
  const double n_samples = ns[0];
  double c = 0.0, c0 = 0.0, n = 0.0, n0 = 0.0, lambda = 1e-3;
  int status = 2, iters = 0;
  double acc[MR_SUMS];
  bool pair = false;                                                          // the thread's pair under the state, and its frozen b
  double pb = 0.0;
  if (!pass) {                                                                // the sums at the input pose
    double Y[3], Cz, a, r;
    pair = mr_associate(s, R, t, Y, Cz, a, r, pb);
    mr_terms(s, pair, Y, Cz, a, r, acc);
    block_sum<MR_SUMS>(acc, sred, tid);
    c = c0 = acc[27]; n = n0 = acc[28];
    if (tid == 0)
      for (int i = 0; i < MR_SUMS; ++i) s_H[i] = acc[i];
    pass = n0 < (double)p.min_pairs;
  }
  for (int it = 0; it < p.max_iters && !pass; ++it) {
    // thread 0: (H + lambda diag H) d = -g -> kind 0: no Cholesky factor (NaN in s_trial); 1: a trial pose
    if (tid == 0) {
      lm_load_lower(s_H, s_L);
      for (int q = 0; q < 6; ++q) s_g[q] = s_H[21 + q];
      if (p.dof == 0) {                                                       // "t": the rotation block is the identity, uncoupled, its gradient 0
        for (int q = 0; q < 6; ++q)
          for (int r = 0; r < 3; ++r) s_L[q][r] = q == r ? 1.0 : 0.0;
        for (int q = 0; q < 3; ++q) s_g[q] = 0.0;
      }
      for (int q = (p.dof == 0 ? 3 : 0); q < 6; ++q) s_L[q][q] = s_L[q][q] + lambda * s_L[q][q];
      double y[6], d[6];
      const int kind = lm_solve_step(s_L, s_g, R, t, y, d, s_trial) ? 1 : 0;
      if (kind && p.dof == 0) {
        for (int i = 0; i < 3; ++i) s_trial[i] = 0.0;
        for (int i = 0; i < 9; ++i) s_trial[6 + i] = R[i];                    // BITWISE the state's rotation
      }
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
      double a1[1] = {mr_trial_term(s, pair, pb, Rn, tn)};
      block_sum<1>(a1, sred, tid);                                            // (its barriers also fence s_trial and s_kind against the next trial)
      if (isfinite(a1[0])) cn = a1[0];
    } else {
      __syncthreads();
    }
    const bool accept = cn < c;
    if (p.records && tid == 0) {
      double* rec = p.records + ((size_t)b * p.max_iters + it) * MR_REC;
      rec[0] = lambda; rec[1] = n; rec[2] = c; rec[3] = cn; rec[4] = accept ? 1.0 : 0.0; rec[5] = sstep;
      for (int i = 0; i < 9; ++i) rec[6 + i] = Rn[i];
      for (int i = 0; i < 3; ++i) rec[15 + i] = tn[i];
    }
    iters = it + 1;
    if (accept) {
      for (int i = 0; i < 9; ++i) R[i] = Rn[i];
      for (int i = 0; i < 3; ++i) t[i] = tn[i];
      lambda = fmax(lambda / 10.0, 1e-12);
      double Y[3], Cz, a, r;
      pair = mr_associate(s, R, t, Y, Cz, a, r, pb);                          // stage B again under the new state
      mr_terms(s, pair, Y, Cz, a, r, acc);
      block_sum<MR_SUMS>(acc, sred, tid);
      c = acc[27]; n = acc[28];
      if (tid == 0)
        for (int i = 0; i < MR_SUMS; ++i) s_H[i] = acc[i];
      if (n < (double)p.min_pairs) { status = 3; break; }
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
    for (int i = 0; i < MR_INFO; ++i) info[i] = NAN;
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

extern "C" int cp_mask_extents(cp_stream_t stream, const int32_t* bits, int NM, int H, int W, int32_t* row, int32_t* col) {
  if (!bits || !row || !col || NM <= 0 || H <= 0 || W <= 0) return CP_ERR_INVALID;
  if (cp_misaligned(bits, 3) || cp_misaligned(row, 3) || cp_misaligned(col, 3)) return CP_ERR_ALIGN;
  const long long chunks = ((long long)H + W + 255) / 256;
  if ((long long)H * W >= (1LL << 31) || chunks * NM >= (1LL << 31)) return CP_ERR_RANGE;
  CP_LAUNCH(mask_extents_kernel, dim3((unsigned)(chunks * NM)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)bits, NM, H, W, (W + 31) / 32,
            (int)chunks, row, col);
  return cp_check_launch();
}

extern "C" size_t cp_contour_samples_scratch_bytes(int P, int Vmax, int grid) {
  if (P <= 0 || Vmax < 0 || grid < 1 || grid > MR_GRID_MAX) return 0;
  return cp_align16_up((size_t)P * MR_HDR * sizeof(int32_t)) + cp_align16_up((size_t)P * 4 * grid * sizeof(mr_key_t)) + (size_t)P * Vmax * sizeof(float4);
}

extern "C" int cp_contour_samples(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                                  const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                                  int H, int W, int P, int Vmax, int grid, int32_t* rect, int32_t* shape, int32_t* pixel, float* depth,
                                  double* X, int32_t* ok, void* scratch) {
  McParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !rect || !shape || !pixel || !depth || !X || !ok || !scratch) return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, P) || grid < 1 || grid > MR_GRID_MAX) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || vs_mesh_misaligned(p.mesh) || cp_misaligned(rect, 3) ||
      cp_misaligned(shape, 3) || cp_misaligned(pixel, 3) || cp_misaligned(depth, 3) || cp_misaligned(X, 7) || cp_misaligned(ok, 3))
    return CP_ERR_ALIGN;
  VsGrid g;
  if (!vs_grid(W, H, 1, false, P, 1, Vmax, g) || (long long)H * W >= (1LL << 31)) return CP_ERR_RANGE;
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.rect = rect; p.shape = shape; p.pixel = pixel; p.depth = depth;
  p.X = X; p.ok = ok; p.P = P; p.H = H; p.W = W; p.grid = grid; p.tx = g.tx; p.ty = g.ty; p.vchunks = g.vchunks;
  char* at = (char*)scratch;
  p.hdr = (int32_t*)at; at += cp_align16_up((size_t)P * MR_HDR * sizeof(int32_t));
  p.keys = (mr_key_t*)at; at += cp_align16_up((size_t)P * 4 * grid * sizeof(mr_key_t));
  p.sv = (float4*)at;
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(contour_pose_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(contour_vertex_kernel, dim3(g.vert_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(contour_tile_kernel, dim3(g.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(contour_finish_kernel, dim3((unsigned)P), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}

extern "C" int cp_mask_refine_record_doubles(void) { return MR_REC; }
extern "C" int cp_mask_refine_info_doubles(void) { return MR_INFO; }

extern "C" int cp_mask_refine(cp_stream_t stream, const double* pose_in, const double* cam_K, int k_stride, const double* X, const int32_t* pixel,
                              const int32_t* ok, int grid, const int32_t* row, const int32_t* col, const int32_t* mask_ids, int NM, int H, int W,
                              const double* max_dist, const int32_t* status_in, int dof, int max_iters, double step_tol, int min_pairs, int P,
                              double* pose_out, int32_t* status_out, double* info, double* records) {
  if (!pose_in || !X || !pixel || !ok || !row || !col || !max_dist || !pose_out || !status_out || !info) return CP_ERR_INVALID;
  if (vs_view_invalid(cam_K, k_stride, H, W, P) || NM <= 0 || (!mask_ids && NM != P)) return CP_ERR_INVALID;
  if (grid < 1 || grid > MR_GRID_MAX || (dof != 0 && dof != 1) || max_iters < 1 || max_iters > MR_MAX_ITERS || min_pairs < 6) return CP_ERR_INVALID;
  if (!cp_finite_positive(step_tol)) return CP_ERR_INVALID;
  if (cp_misaligned(pose_in, 7) || vs_view_misaligned(cam_K) || cp_misaligned(X, 7) || cp_misaligned(pixel, 3) || cp_misaligned(ok, 3) ||
      cp_misaligned(row, 3) || cp_misaligned(col, 3) || cp_misaligned(mask_ids, 3) || cp_misaligned(max_dist, 7) ||
      cp_misaligned(status_in, 3) || cp_misaligned(pose_out, 7) || cp_misaligned(status_out, 3) || cp_misaligned(info, 7) ||
      cp_misaligned(records, 7))
    return CP_ERR_ALIGN;
  if (cp_pose_alias_invalid(pose_in, pose_out, P)) return CP_ERR_INVALID;
  if ((long long)H * W >= (1LL << 31) || P >= (1 << 24)) return CP_ERR_RANGE;
  MrParams p;
  p.pose_in = pose_in; p.K = cam_K; p.X = X; p.pixel = pixel; p.ok = ok; p.row = row; p.col = col; p.mask_ids = mask_ids; p.max_dist = max_dist;
  p.status_in = status_in; p.pose_out = pose_out; p.status_out = status_out; p.info = info; p.records = records; p.k_stride = k_stride;
  p.P = P; p.grid = grid; p.NM = NM; p.H = H; p.W = W; p.dof = dof; p.max_iters = max_iters; p.min_pairs = min_pairs; p.step_tol = step_tol;
  CP_LAUNCH(mask_refine_kernel, dim3((unsigned)P), dim3(PNP_THREADS), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}
