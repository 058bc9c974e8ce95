// cp_vsd_errors: BOP's Visible Surface Discrepancy of a batch of poses on the device -- a depth rasteriser fused
// with the pixel counting of bop_toolkit_lib/pose_error.py:17-93 (vsd), misc.py:110-163 (depth_im_to_dist_im_fast) and visibility.py
// ('bop19' mode, 'step' cost).  The reference renders the mesh twice per pose through OpenGL (renderer_py.py:185-226, 422-555) and
// then makes several full-frame numpy passes; here no depth image exists unless the caller asks for it.
//
// The render rule, the rasteriser and the scaffold of the four kernels are vsd_raster.h's, shared with rows N10, N12 and N14; a pose
// that the rule does not render (a vertex at Z <= 0) has NaN errors.
//
// Launches (three, + one when meshes are involved):
//   vsd_pose_kernel     per pose: P = K' [R | t] of the estimate and of the ground truth (vs_side_init; K' as render_object takes
//                       it); validity; the caller's overlapping_sphere_projections shortcut (vs_sphere_skip) in double; the pixel
//                       rectangles are initialised.
//   vsd_vertex_kernel   per (pose, side, 256 vertices): screen records (vs_project); the side's pixel rectangle and its "a vertex at
//                       Z <= 0" flag through INTEGER atomic min / max / or (vs_rect_merge: order-independent).
//   vsd_tile_kernel     a workgroup owns a 32 x 32 pixel tile of one pose, a lane 4 pixels of it (both depths in registers): the
//                       walk over the mesh's triangles (vs_depth_tile) once per side.  Then the tile reads the test depth, does
//                       the reference's distance / visibility arithmetic (fp64 square roots and quotients, the fp32 difference
//                       against delta) and reduces INTEGER counts: wave shuffles, LDS, one row of scratch per tile.
//                       Tiles outside the union of the two rectangles leave at once (or write zeros when depth images are asked).
//   vsd_sum_kernel      per pose: the tile rows the rectangles reach, summed (integers), and the quotients.
// Every output is a function of integer counts and per-pixel values: bit-identical from call to call, for a pose alone or in a
// batch, with or without the depth output.  No floating-point atomics, no initialised scratch beyond what vsd_pose_kernel writes.
#include "vsd_raster.h"

namespace {

constexpr int VS_TMAX = 16;                      // taus per call
constexpr int VS_ROW = VS_TMAX + 2;              // ints per tile row: union, inter, cost[T]
using VsH = VsHdr<2>;                            // a pose's header: P, rect and bad of the estimate and the ground truth, ok, then
constexpr int VS_SKIP = VsH::USER;               // the sphere shortcut's verdict;
constexpr int VS_HDR = 40;                       // 4-byte words per pose (the rest is spare)
enum { VS_MODE_VSD = 0, VS_MODE_RENDER = 1, VS_MODE_DEPTH = 2 };

struct VsParams {
  VsMesh mesh;                // (Vmax 0 in DEPTH mode: no vertices)
  const double* est;          // (B, 12)
  const double* gt;
  const double* K;
  const float* depth_test;    // (I, H, W)
  const int32_t* image_id;    // nullptr: image 0
  const double* diameters;    // per mesh (VSD) / per pose (DEPTH)
  const float* in_est;        // DEPTH mode: (B, H, W)
  const float* in_gt;
  float* depth_out;           // (B, nsides, H, W) or nullptr
  double* errors;             // (B, T)
  int32_t* counts;            // (B, T + 2)
  int32_t* hdr;               // (B, VS_HDR)
  float4* sv;                 // (B, 2, Vmax)
  int32_t* rows;              // (B, tiles, VS_ROW)
  double taus[VS_TMAX];
  float delta;
  // (tx and ty stand apart on purpose: vsd_tile_kernel's speed depends on where its walk loops lie -- a loop start on a 64-byte boundary
  // costs it 3 %, every instruction the same -- and with the two in one scalar load the first loop starts on one.  After a change to
  // this struct or to the kernel's prologue, compare tools/vsd_bench.py with the commit before.)
  int k_stride, B, H, W, I, T, normalise, sphere, mode, tx, nsides, vchunks, ty;
};

__global__ __launch_bounds__(VS_THREADS) void vsd_pose_kernel(VsParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.B) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * VS_HDR;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  bool ok = vs_finite(K, 9);
  if (p.mode != VS_MODE_RENDER) {
    const int img = p.image_id ? p.image_id[b] : 0;
    ok = ok && img >= 0 && img < p.I;
  }
  int skip = 0;
  if (p.mode == VS_MODE_DEPTH) {
    for (int s = 0; s < 2; ++s) vs_rect_set(h + VsH::RECT(s), 0, 0, p.W - 1, p.H - 1);
  } else {
    int vfirst, V, ffirst, F, m;
    ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m) && ok;
    const double* __restrict__ e = p.est + 12 * (size_t)b;
    const double* __restrict__ g = p.gt + 12 * (size_t)b;
    ok = ok && vs_finite(e, 12) && vs_finite(g, 12);
    vs_side_init(K, 1.0, e, (float*)h + VsH::P(0), h + VsH::RECT(0));
    vs_side_init(K, 1.0, g, (float*)h + VsH::P(1), h + VsH::RECT(1));
    if (ok && p.sphere && p.mode == VS_MODE_VSD) skip = vs_sphere_skip(e, g, p.diameters[m] / 2.0);
  }
  h[VsH::BAD(0)] = 0; h[VsH::BAD(1)] = 0;
  h[VsH::OK] = ok ? 1 : 0;
  h[VS_SKIP] = skip;
}

__global__ __launch_bounds__(VS_THREADS) void vsd_vertex_kernel(VsParams p) {
#pragma clang fp contract(off)
  int b, s, vc;
  vs_vertex_block(p.vchunks, p.nsides, b, s, vc);
  int32_t* __restrict__ h = p.hdr + (size_t)b * VS_HDR;
  if (!h[VsH::OK] || h[VS_SKIP]) return;                             // (uniform; no barrier in this kernel)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  vs_vertex_chunk((const float*)h + VsH::P(s), p.mesh.verts + 3 * (size_t)vfirst, V, vc, make_float4(-2.f, (float)p.W + 1.f, -2.f, (float)p.H + 1.f),
                  p.sv + ((size_t)b * 2 + s) * p.mesh.Vmax, h + VsH::RECT(s), h + VsH::BAD(s));
}

__global__ __launch_bounds__(VS_THREADS) void vsd_tile_kernel(VsParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];          // e0 (a b c .) e1 (a b c .) e2 (a b c .) plane (A B C .): .w = ymin ymax - -
  __shared__ int s_n;
  __shared__ int s_cnt[VS_THREADS / 64][VS_ROW];
  const VsTile c = vs_tile(p.tx, p.ty, 0, 0);
  const int tid = c.tid, lane = c.lane, wave = c.wave, b = c.b, ox = c.ox, oy = c.oy, lx = c.lx;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * VS_HDR;
  const bool live = h[VsH::OK] && !h[VS_SKIP] && !h[VsH::BAD(0)] && !h[VsH::BAD(1)];
  // the pose's rectangles against this tile
  bool hit[2];
  for (int s = 0; s < 2; ++s) hit[s] = live && s < p.nsides && vs_tile_hit(h + VsH::RECT(s), ox, oy);
  if (!hit[0] && !hit[1] && !p.depth_out) return;                   // (uniform)
  float dep[2][VS_PPL];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) dep[s][k] = 0.f;

  if (p.mode == VS_MODE_DEPTH) {
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) {
      const int x = ox + lx, y = oy + c.y(k);
      if (hit[0] && x < p.W && y < p.H) {
        const size_t at = ((size_t)b * p.H + y) * p.W + x;
        dep[0][k] = p.in_est[at];
        dep[1][k] = p.in_gt[at];
      }
    }
  } else {
    int vfirst, V, ffirst, F, m;
    vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (hit[s])                                                    // (uniform)
        vs_depth_tile(s_tri, &s_n, p.sv + ((size_t)b * 2 + s) * p.mesh.Vmax, p.mesh.faces + 3 * (size_t)ffirst, F, V, c, dep[s]);
  }

  if (p.depth_out) {
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) {
      const int x = ox + lx, y = oy + c.y(k);
      if (x < p.W && y < p.H)
        for (int s = 0; s < p.nsides; ++s)
          p.depth_out[(((size_t)b * p.nsides + s) * p.H + y) * p.W + x] = s == 0 ? dep[0][k] : dep[1][k];
    }
  }
  if (p.mode == VS_MODE_RENDER || (!hit[0] && !hit[1])) return;     // (uniform)

  // ---- the reference's counting on this tile
  int cnt[VS_ROW];
#pragma unroll
  for (int k = 0; k < VS_ROW; ++k) cnt[k] = 0;
  {
#pragma clang fp contract(off)
    const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const int img = p.image_id ? p.image_id[b] : 0;
    const float* __restrict__ test = p.depth_test + (size_t)img * p.H * p.W;
    const double diam = p.diameters[p.mode == VS_MODE_DEPTH ? b : (p.mesh.mesh_id ? p.mesh.mesh_id[b] : 0)];
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) {
      const int x = ox + lx, y = oy + c.y(k);
      const float de = dep[0][k], dg = dep[1][k];
      if (x >= p.W || y >= p.H || (!(de > 0.f) && !(dg > 0.f))) continue;     // dist_model > 0 fails on both sides: no count moves
      const float dt = test[(size_t)y * p.W + x];
      const double px = ((double)x - cx) / fx, py = ((double)y - cy) / fy;
      const double t_test = vs_dist(px, py, dt), t_est = vs_dist(px, py, de), t_gt = vs_dist(px, py, dg);
      const bool vg = vs_visible(t_test, t_gt, p.delta);
      const bool ve = vs_visible(t_test, t_est, p.delta) || (vg && t_est > 0.0);
      cnt[0] += (vg || ve) ? 1 : 0;
      if (vg && ve) {
        cnt[1] += 1;
        double dd = fabs(t_gt - t_est);
        if (p.normalise) dd = dd / diam;
#pragma unroll
        for (int q = 0; q < VS_TMAX; ++q)
          if (q < p.T) cnt[2 + q] += dd >= p.taus[q] ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < VS_ROW; ++k) {
    int v = cnt[k];
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
    if (lane == 0) s_cnt[wave][k] = v;
  }
  __syncthreads();
  if (tid < VS_ROW) {
    int v = 0;
    for (int w = 0; w < VS_THREADS / 64; ++w) v += s_cnt[w][tid];
    p.rows[((size_t)b * p.tx * p.ty + c.t) * VS_ROW + tid] = v;
  }
}

__global__ __launch_bounds__(64) void vsd_sum_kernel(VsParams p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * VS_HDR;
  const bool ok = h[VsH::OK] != 0, skip = h[VS_SKIP] != 0, bad = h[VsH::BAD(0)] || h[VsH::BAD(1)];
  int cnt[VS_ROW];
#pragma unroll
  for (int k = 0; k < VS_ROW; ++k) cnt[k] = 0;
  if (ok && !skip && !bad) {
    // the tiles vsd_tile_kernel counted on: the ones either rectangle reaches (the others were never written)
    const int tiles = p.tx * p.ty;
    for (int t = lane; t < tiles; t += 64) {
      const int ox = (t % p.tx) * VS_TILE, oy = (t / p.tx) * VS_TILE;
      if (!vs_tile_hit(h + VsH::RECT(0), ox, oy) && !vs_tile_hit(h + VsH::RECT(1), ox, oy)) continue;
      const int32_t* __restrict__ r = p.rows + ((size_t)b * tiles + t) * VS_ROW;
#pragma unroll
      for (int k = 0; k < VS_ROW; ++k) cnt[k] += r[k];
    }
  }
#pragma unroll
  for (int k = 0; k < VS_ROW; ++k)
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) cnt[k] += __shfl_xor(cnt[k], w, 64);
  if (lane == 0) {
#pragma clang fp contract(off)
    const int uni = cnt[0], comp = cnt[0] - cnt[1];
    p.counts[(size_t)b * (p.T + 2)] = cnt[0];
    p.counts[(size_t)b * (p.T + 2) + 1] = cnt[1];
#pragma unroll
    for (int q = 0; q < VS_TMAX; ++q) {
      if (q >= p.T) continue;
      p.counts[(size_t)b * (p.T + 2) + 2 + q] = cnt[2 + q];
      double e = 1.0;                                                // union == 0, or the sphere shortcut
      if (!ok || (bad && !skip)) e = __builtin_nan("");
      else if (!skip && uni > 0) e = (double)(cnt[2 + q] + comp) / (double)uni;
      p.errors[(size_t)b * p.T + q] = e;
    }
  }
}

void vs_carve(VsParams& p, void* scratch) {
  char* at = (char*)scratch;
  p.hdr = (int32_t*)at;
  at += cp_align16_up((size_t)p.B * VS_HDR * sizeof(int32_t));
  p.sv = (float4*)at;
  at += (size_t)p.B * 2 * p.mesh.Vmax * sizeof(float4);
  p.rows = (int32_t*)at;
}

int vs_launch(VsParams& p, hipStream_t st) {
  VsGrid g;
  if (!vs_grid(p.W, p.H, 1, false, p.B, p.nsides, p.mesh.Vmax, g) || (long long)p.H * p.W >= (1LL << 31)) return CP_ERR_RANGE;
  p.tx = g.tx; p.ty = g.ty; p.vchunks = g.vchunks;
  CP_LAUNCH(vsd_pose_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  if (p.mode != VS_MODE_DEPTH) CP_LAUNCH(vsd_vertex_kernel, dim3(g.vert_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(vsd_tile_kernel, dim3(g.tile_blocks), dim3(VS_THREADS), 0, st, p);
  if (p.mode != VS_MODE_RENDER) CP_LAUNCH(vsd_sum_kernel, dim3((unsigned)p.B), dim3(64), 0, st, p);
  return cp_check_launch();
}

}  // namespace

extern "C" size_t cp_vsd_errors_scratch_bytes(int B, int Vmax, int H, int W) {
  if (B <= 0 || Vmax < 0 || H <= 0 || W <= 0) return 0;
  const size_t tiles = (size_t)((W + VS_TILE - 1) / VS_TILE) * (size_t)((H + VS_TILE - 1) / VS_TILE);
  return cp_align16_up((size_t)B * VS_HDR * sizeof(int32_t)) + (size_t)B * 2 * Vmax * sizeof(float4) +
         cp_align16_up((size_t)B * tiles * VS_ROW * sizeof(int32_t));
}

extern "C" int cp_vsd_errors(cp_stream_t stream, const double* pose_est, const double* pose_gt, const double* cam_K, int k_stride,
                             const float* verts, const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M,
                             const int32_t* mesh_ids, const float* depth_test, const int32_t* image_ids, int I, int H, int W,
                             double delta, const double* diameters, const double* taus, int T, int normalized_by_diameter,
                             int sphere_check, int B, int Vmax, double* errors, int32_t* counts, float* depth_out, void* scratch) {
  VsParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!pose_est || !pose_gt || !depth_test || !diameters || !taus || !errors || !counts || !scratch) return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, B) || vs_images_invalid(image_ids, I) || T < 1 || T > VS_TMAX ||
      !(delta == delta))
    return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(pose_est, 7) || cp_misaligned(pose_gt, 7) || vs_view_misaligned(cam_K) ||
      cp_misaligned(diameters, 7) || cp_misaligned(errors, 7) || vs_mesh_misaligned(p.mesh) || cp_misaligned(depth_test, 3) ||
      cp_misaligned(image_ids, 3) || cp_misaligned(counts, 3) || cp_misaligned(depth_out, 3))
    return CP_ERR_ALIGN;
  p.est = pose_est; p.gt = pose_gt; p.K = cam_K; p.k_stride = k_stride; p.depth_test = depth_test; p.image_id = image_ids; p.I = I; p.H = H;
  p.W = W; p.delta = (float)delta; p.diameters = diameters; p.T = T; p.normalise = normalized_by_diameter ? 1 : 0;
  p.sphere = sphere_check ? 1 : 0; p.B = B; p.errors = errors; p.counts = counts; p.depth_out = depth_out; p.mode = VS_MODE_VSD; p.nsides = 2;
  for (int k = 0; k < T; ++k) p.taus[k] = taus[k];
  vs_carve(p, scratch);
  return vs_launch(p, (hipStream_t)stream);
}

extern "C" int cp_vsd_from_depth(cp_stream_t stream, const float* depth_est, const float* depth_gt, const double* cam_K, int k_stride,
                                 const float* depth_test, const int32_t* image_ids, int I, int H, int W, double delta,
                                 const double* diameters, const double* taus, int T, int normalized_by_diameter, int B, double* errors,
                                 int32_t* counts, void* scratch) {
  if (!depth_est || !depth_gt || !depth_test || !diameters || !taus || !errors || !counts || !scratch) return CP_ERR_INVALID;
  if (vs_view_invalid(cam_K, k_stride, H, W, B) || vs_images_invalid(image_ids, I) || T < 1 || T > VS_TMAX || !(delta == delta))
    return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || vs_view_misaligned(cam_K) || cp_misaligned(diameters, 7) || cp_misaligned(errors, 7) ||
      cp_misaligned(depth_est, 3) || cp_misaligned(depth_gt, 3) || cp_misaligned(depth_test, 3) || cp_misaligned(image_ids, 3) ||
      cp_misaligned(counts, 3))
    return CP_ERR_ALIGN;
  VsParams p = {};
  p.in_est = depth_est; p.in_gt = depth_gt; p.K = cam_K; p.k_stride = k_stride; p.depth_test = depth_test; p.image_id = image_ids;
  p.I = I; p.H = H; p.W = W; p.delta = (float)delta; p.diameters = diameters; p.T = T; p.normalise = normalized_by_diameter ? 1 : 0;
  p.B = B; p.errors = errors; p.counts = counts; p.mode = VS_MODE_DEPTH; p.nsides = 2;
  for (int k = 0; k < T; ++k) p.taus[k] = taus[k];
  vs_carve(p, scratch);
  return vs_launch(p, (hipStream_t)stream);
}

extern "C" int cp_render_depth(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                               const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                               int H, int W, int B, int Vmax, float* depth_out, void* scratch) {
  VsParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !depth_out || !scratch || vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, B)) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || vs_mesh_misaligned(p.mesh) ||
      cp_misaligned(depth_out, 3))
    return CP_ERR_ALIGN;
  p.est = poses; p.gt = poses; p.K = cam_K; p.k_stride = k_stride; p.H = H; p.W = W; p.B = B; p.depth_out = depth_out;
  p.mode = VS_MODE_RENDER; p.nsides = 1; p.T = 1;
  vs_carve(p, scratch);
  return vs_launch(p, (hipStream_t)stream);
}
