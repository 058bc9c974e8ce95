// cp_gt_info: what bop_toolkit's scripts/calc_gt_info.py:72-175 and scripts/calc_gt_masks.py:94-127 write for a
// ground-truth pose -- px_count_all / _valid / _visib, visib_fract, bbox_obj, bbox_visib, the mask and mask_visib images -- for a
// batch of poses on the device.  The reference renders every pose through OpenGL on a 3W x 3H canvas (the principal point moved by
// (W, H)) and then makes full-frame numpy passes; here the canvas is the frame's pixel grid extended to x in [-W, 2W), y in [-H, 2H),
// rendered tile by tile with vsd_raster.h's rasteriser (the render rule is stated there), and nothing is stored unless asked.
//
// Tile grid.  32 x 32 tiles starting at (-32 ceil(W/32), -32 ceil(H/32)): frame pixel (0, 0) is a tile corner, so an in-frame tile
// runs vs_depth_tile with the arguments cp_render_depth's tile of the (W, H) frame does -- the in-frame depth is the same bits.
// Tile pixels outside the canvas (the grid overshoots it on every side) count nowhere.
//
// Launches (four; three from a caller's canvas):
//   gt_info_pose_kernel    per pose: P = K' [R | t] (vs_side_init), validity, the rectangle and the integer accumulators initialised.
//   gt_info_vertex_kernel  per (pose, 256 vertices): screen records (vs_vertex_chunk, clamped to the canvas) and the pose's pixel rectangle.
//   gt_info_tile_kernel    a workgroup per (pose, canvas tile).  A tile the rectangle misses leaves at once (or writes zeros into the
//                          images asked for, when it lies in the frame).  Otherwise: the depth of its 1024 pixels; in the canvas,
//                          depth > 0 counts into px_count_all and the silhouette's box; IN THE FRAME ONLY the reference's distance
//                          arithmetic (fp64 square roots and quotients without contraction, the fp32 difference against delta)
//                          gives mask, mask_visib, px_count_valid, px_count_visib and the visible box.  Three sums, four minima and
//                          four maxima are reduced as INTEGERS into the pose's accumulators (vs_acc_reduce: order-independent).
//   gt_info_finish_kernel  per pose: the quotient, the two boxes as x, y, w, h (both gated on px_count_visib > 0), ok.
// Every output is a function of integer counts and per-pixel values: bit-identical from call to call, for a pose alone or in a
// batch, with or without the images.  No floating-point atomics, no initialised scratch beyond what gt_info_pose_kernel writes.
#include "vsd_raster.h"

namespace {

// 4-byte words per pose: VsHdr<1> (P rect bad ok) | all valid visib | obj xmin ymin xmax ymax | visib xmin ymin xmax ymax
using GiH = VsHdr<1>;
constexpr int GI_HDR = 32;
constexpr int GI_ACC = GiH::USER, GI_NSUM = 3, GI_NACC = 11;
enum { GI_MODE_RENDER = 0, GI_MODE_DEPTH = 1 };

struct GiParams {
  VsMesh mesh;                // (Vmax 0 in DEPTH mode: no vertices)
  const double* poses;        // (B, 12)
  const double* K;
  const float* depth;         // (I, H, W): the sensor's
  const int32_t* image_id;    // nullptr: image 0
  const float* large;         // DEPTH mode: (B, 3H, 3W)
  int32_t* counts;            // (B, 3)
  double* fract;              // (B)
  int32_t* boxes;             // (B, 2, 4)
  uint8_t* ok;                // (B)
  uint8_t* mask;              // (B, H, W) or nullptr
  uint8_t* mask_visib;
  float* depth_gt;            // (B, H, W) or nullptr
  int32_t* hdr;               // (B, GI_HDR)
  float4* sv;                 // (B, Vmax)
  float delta;
  int k_stride, B, I, H, W, mode, tx, ty, x0, y0, vchunks;      // (H .. vchunks side by side: one scalar load in the tile kernel)
};

__global__ __launch_bounds__(VS_THREADS) void gt_info_pose_kernel(GiParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.B) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * GI_HDR;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  bool ok = vs_finite(K, 9);
  const int img = p.image_id ? p.image_id[b] : 0;
  ok = ok && img >= 0 && img < p.I;
  if (p.mode == GI_MODE_DEPTH) {
    for (int k = 0; k < 12; ++k) h[k] = 0;
    vs_rect_set(h + GiH::RECT(0), -p.W, -p.H, 2 * p.W - 1, 2 * p.H - 1);
  } else {
    int vfirst, V, ffirst, F, m;
    ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m) && ok;
    const double* __restrict__ q = p.poses + 12 * (size_t)b;
    ok = ok && vs_finite(q, 12);
    vs_side_init(K, 1.0, q, (float*)h + GiH::P(0), h + GiH::RECT(0));
  }
  h[GiH::BAD(0)] = 0;
  h[GiH::OK] = ok ? 1 : 0;
  for (int k = 0; k < GI_NACC; ++k) h[GI_ACC + k] = vs_acc_identity<GI_NSUM>(k);
  for (int k = GI_ACC + GI_NACC; k < GI_HDR; ++k) h[k] = 0;
}

__global__ __launch_bounds__(VS_THREADS) void gt_info_vertex_kernel(GiParams p) {
  int b, s, vc;
  vs_vertex_block(p.vchunks, 1, b, s, vc);
  int32_t* __restrict__ h = p.hdr + (size_t)b * GI_HDR;
  if (!h[GiH::OK]) return;                                           // (uniform; no barrier in this kernel)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  const float4 canvas = make_float4(-(float)p.W - 2.f, 2.f * (float)p.W + 1.f, -(float)p.H - 2.f, 2.f * (float)p.H + 1.f);
  vs_vertex_chunk((const float*)h + GiH::P(0), p.mesh.verts + 3 * (size_t)vfirst, V, vc, canvas, p.sv + (size_t)b * p.mesh.Vmax, h + GiH::RECT(0),
                  h + GiH::BAD(0));
}

__global__ __launch_bounds__(VS_THREADS) void gt_info_tile_kernel(GiParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  __shared__ int s_red[VS_THREADS / 64][GI_NACC];
  const VsTile c = vs_tile(p.tx, p.ty, p.x0, p.y0);
  const int b = c.b, ox = c.ox, oy = c.oy;                           // first pixel, frame coordinates (any sign)
  int32_t* __restrict__ h = p.hdr + (size_t)b * GI_HDR;
  const bool live = h[GiH::OK] && !h[GiH::BAD(0)];
  const bool hit = live && vs_tile_hit(h + GiH::RECT(0), ox, oy);
  const bool in_frame = ox >= 0 && ox < p.W && oy >= 0 && oy < p.H;                  // the grid is anchored at frame pixel (0, 0)
  const bool store = in_frame && (p.mask || p.depth_gt);
  if (!hit && !store) return;                                        // (uniform)
  const int x = ox + c.lx;
  float dep[VS_PPL];
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) dep[k] = 0.f;
  if (hit) {
    if (p.mode == GI_MODE_DEPTH) {
#pragma unroll
      for (int k = 0; k < VS_PPL; ++k) {
        const int y = oy + c.y(k);
        if (x >= -p.W && x < 2 * p.W && y >= -p.H && y < 2 * p.H) dep[k] = p.large[((size_t)b * 3 * p.H + (y + p.H)) * 3 * p.W + (x + p.W)];
      }
    } else {
      const VsMesh mesh = p.mesh;                                   // (a copy on purpose: read through p, the kernel takes 6 more VGPRs)
      int vfirst, V, ffirst, F, m;
      vs_mesh_rows(mesh, b, vfirst, V, ffirst, F, m);
      vs_depth_tile(s_tri, &s_n, p.sv + (size_t)b * mesh.Vmax, mesh.faces + 3 * (size_t)ffirst, F, V, c, dep);
    }
  }

  int acc[GI_NACC];
#pragma unroll
  for (int k = 0; k < GI_NACC; ++k) acc[k] = vs_acc_identity<GI_NSUM>(k);
  // ---- the canvas: the truncated silhouette's count and box (no distance arithmetic)
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) {
    const int y = oy + c.y(k);
    if (dep[k] > 0.f && x >= -p.W && x < 2 * p.W && y >= -p.H && y < 2 * p.H) {
      acc[0] += 1;
      acc[3] = min(acc[3], x); acc[4] = min(acc[4], y); acc[5] = max(acc[5], x); acc[6] = max(acc[6], y);
    }
  }
  // ---- the frame: the reference's distances, masks and counts
  if (in_frame) {
#pragma clang fp contract(off)
    const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) {
      const int y = oy + c.y(k);
      if (x >= p.W || y >= p.H) continue;
      const float dg = dep[k];
      bool m = false, vis = false;
      if (dg != 0.f) {                                               // dist_gt == 0 otherwise: neither mask is set, no count moves
        const int img = p.image_id ? p.image_id[b] : 0;              // (hit, hence a checked id)
        const float dt = p.depth[((size_t)img * p.H + y) * p.W + x];
        const double px = ((double)x - cx) / fx, py = ((double)y - cy) / fy;
        const double t_im = vs_dist(px, py, dt), t_gt = vs_dist(px, py, dg);
        m = t_gt > 0.0;
        vis = vs_visible(t_im, t_gt, p.delta);
        if (m && t_im > 0.0) acc[1] += 1;
        if (vis) {
          acc[2] += 1;
          acc[7] = min(acc[7], x); acc[8] = min(acc[8], y); acc[9] = max(acc[9], x); acc[10] = max(acc[10], y);
        }
      }
      const size_t at = ((size_t)b * p.H + y) * p.W + x;
      if (p.mask) { p.mask[at] = m ? 255 : 0; p.mask_visib[at] = vis ? 255 : 0; }
      if (p.depth_gt) p.depth_gt[at] = dg;
    }
  }
  if (!hit) return;                                                  // (uniform) zeros were stored, nothing to count

  vs_acc_reduce<GI_NSUM, GI_NACC>(acc, s_red, h + GI_ACC);
}

__global__ __launch_bounds__(VS_THREADS) void gt_info_finish_kernel(GiParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.B) return;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * GI_HDR;
  const bool live = h[GiH::OK] && !h[GiH::BAD(0)];
  const int32_t* __restrict__ a = h + GI_ACC;
  const int all = live ? a[0] : 0, valid = live ? a[1] : 0, visib = live ? a[2] : 0;
  p.counts[3 * (size_t)b] = all;
  p.counts[3 * (size_t)b + 1] = valid;
  p.counts[3 * (size_t)b + 2] = visib;
  p.fract[b] = all > 0 ? (double)visib / (double)all : 0.0;
  for (int s = 0; s < 2; ++s)                                        // bbox_obj is gated on the VISIBLE count too
    vs_box_xywh(a + GI_NSUM + 4 * s, visib > 0, p.boxes + 8 * (size_t)b + 4 * s);
  p.ok[b] = live ? 1 : 0;
}

void gi_carve(GiParams& p, void* scratch) {
  char* at = (char*)scratch;
  p.hdr = (int32_t*)at;
  at += cp_align16_up((size_t)p.B * GI_HDR * sizeof(int32_t));
  p.sv = (float4*)at;
}

int gi_launch(GiParams& p, hipStream_t st) {
  VsGrid g;
  if ((long long)p.H * p.W >= (1LL << 31) / 9 || !vs_grid(p.W, p.H, 1, true, p.B, 1, p.mesh.Vmax, g)) return CP_ERR_RANGE;
  p.tx = g.tx; p.ty = g.ty; p.x0 = g.x0; p.y0 = g.y0; p.vchunks = g.vchunks;
  CP_LAUNCH(gt_info_pose_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  if (p.mode == GI_MODE_RENDER) CP_LAUNCH(gt_info_vertex_kernel, dim3(g.vert_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(gt_info_tile_kernel, dim3(g.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(gt_info_finish_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}

}  // namespace

extern "C" size_t cp_gt_info_scratch_bytes(int B, int Vmax) {
  if (B <= 0 || Vmax < 0) return 0;
  return cp_align16_up((size_t)B * GI_HDR * sizeof(int32_t)) + cp_align16_up((size_t)B * Vmax * sizeof(float4));
}

extern "C" int cp_gt_info(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                          const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                          const float* depth, const int32_t* image_ids, int I, int H, int W, double delta, int B, int Vmax,
                          int32_t* counts, double* visib_fract, int32_t* boxes, uint8_t* ok, uint8_t* mask, uint8_t* mask_visib,
                          float* depth_gt, void* scratch) {
  GiParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !depth || !counts || !visib_fract || !boxes || !ok || !scratch) return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, B) || vs_images_invalid(image_ids, I) || !(delta == delta) ||
      (mask == nullptr) != (mask_visib == nullptr))
    return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || cp_misaligned(visib_fract, 7) ||
      vs_mesh_misaligned(p.mesh) || cp_misaligned(depth, 3) || cp_misaligned(image_ids, 3) || cp_misaligned(counts, 3) ||
      cp_misaligned(boxes, 3) || cp_misaligned(depth_gt, 3))
    return CP_ERR_ALIGN;
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.depth = depth; p.image_id = image_ids; p.I = I; p.H = H; p.W = W;
  p.delta = (float)delta; p.B = B; p.counts = counts; p.fract = visib_fract; p.boxes = boxes; p.ok = ok; p.mask = mask;
  p.mask_visib = mask_visib;
  p.depth_gt = depth_gt; p.mode = GI_MODE_RENDER;
  gi_carve(p, scratch);
  return gi_launch(p, (hipStream_t)stream);
}

extern "C" int cp_gt_info_from_depth(cp_stream_t stream, const float* depth_gt_large, const double* cam_K, int k_stride,
                                     const float* depth, const int32_t* image_ids, int I, int H, int W, double delta, int B,
                                     int32_t* counts, double* visib_fract, int32_t* boxes, uint8_t* ok, uint8_t* mask,
                                     uint8_t* mask_visib, void* scratch) {
  if (!depth_gt_large || !depth || !counts || !visib_fract || !boxes || !ok || !scratch) return CP_ERR_INVALID;
  if (vs_view_invalid(cam_K, k_stride, H, W, B) || vs_images_invalid(image_ids, I) || !(delta == delta) ||
      (mask == nullptr) != (mask_visib == nullptr))
    return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || vs_view_misaligned(cam_K) || cp_misaligned(visib_fract, 7) || cp_misaligned(depth_gt_large, 3) ||
      cp_misaligned(depth, 3) || cp_misaligned(image_ids, 3) || cp_misaligned(counts, 3) || cp_misaligned(boxes, 3))
    return CP_ERR_ALIGN;
  GiParams p = {};
  p.large = depth_gt_large; p.K = cam_K; p.k_stride = k_stride; p.depth = depth; p.image_id = image_ids; p.I = I; p.H = H; p.W = W;
  p.delta = (float)delta; p.B = B; p.counts = counts; p.fract = visib_fract; p.boxes = boxes; p.ok = ok; p.mask = mask;
  p.mask_visib = mask_visib; p.mode = GI_MODE_DEPTH;
  gi_carve(p, scratch);
  return gi_launch(p, (hipStream_t)stream);
}
