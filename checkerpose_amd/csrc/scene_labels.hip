// cp_render_scene: occluded multi-object training scenes with their labels, for a batch of images on the device.
// One call gives what the composition vis_poses(resolve) -> gt_info(depth = ren_depth, masks) gives -- the composite colour and depth
// of every image, and for every pose the counts, visib_fract and boxes of scene_gt_info.json with the composite as the sensor depth --
// plus a background behind the objects, and the 2 P full-frame mask images as TWO bit planes per image.
//
// The rule (stated in include/checkerpose_hip.h; every term is another row's, bit for bit):
//   slot s of a pose = its rank among the poses of its image in the order given (pose_order within [img_off[i], img_off[i + 1]));
//   a pose that is not rendered keeps its slot.  At most 32 poses per image.
//   composite: cp_vis_poses' with resolve != 0 -- per pose cp_render_rgb's frame (ssaa 1), the front-most pose under the strict
//   m_depth < ren_depth test (of equal depths the earlier pose keeps the pixel); rgb = the winner's colour where ren_depth > 0, the
//   background elsewhere.
//   labels: cp_gt_info's for every pose with the image's ren_depth as the sensor depth -- the same canvas x in [-W, 2W), y in [-H, 2H)
//   on the same tile grid, vs_dist / vs_visible ('bop19': f32(dist_gt) - f32(dist_im) <= delta), the same integer accumulators.
//   bit planes: bit s of full_bits / visib_bits[img, y, x] is set where pose s's mask / mask_visib would be 255.
//   A pose that cp_vis_poses does not render (a non-finite entry, a singular R, any vertex at Z <= 0, a bad mesh or image id, a
//   non-finite surface colour) is skipped: ok = 0, counts 0, fraction 0, boxes -1, its bits 0.
//
// Textures (row N20, cp_render_scene_tex): the owner's colour is its mesh's texel by render_shade.h's rule; the tile launch is then
// scene_tile_kernel<true> (the colour source is uniform per iteration of the pose loop), without textures scene_tile_kernel<false>,
// which holds no texture code: the kernel this file had before textures, with the same registers, LDS and output bits.
//
// Launches (four, whatever the data):
//   scene_pose_kernel     per pose: render_shade.h's header under the pose's IMAGE's K, validity, its slot, the accumulators initialised.
//   scene_vertex_kernel   per (pose, 256 vertices): cp_render_rgb's records; the pixel rectangle clamped to the CANVAS (gt_info's).
//   scene_tile_kernel     a workgroup per (image, 32 x 32 canvas tile), 4 pixels per lane.  Which of the image's poses meet the tile is
//                         decided once, a lane per slot (sl_hits: a 32-bit mask, uniform over the workgroup); the loops below run
//                         over its bits in slot order.
//                         margin tile: per pose depth only (vs_depth_tile): px_count_all and bbox_obj's limits, no distance arithmetic.
//                         in-frame tile: pass A walks the image's poses depth-only -> ren_depth in registers (skipped where ONE pose
//                         meets the tile: the composite there is that pose's own depth); pass B walks them again
//                         WITH the winning face (vs_raster_tile<true>): the two bits, the pose's counts and box limits against
//                         ren_depth, and rr_shade for the ONE pose that owns the pixel -- the first in order whose depth equals
//                         ren_depth -- instead of one per covering pose.  rgb, depth and the two planes are stored once.
//                         (The second raster was kept: holding P per-pose depths per pixel would take 4 KiB of LDS per pose --
//                         128 KiB at 32 poses -- and cost the occupancy the walk lives on; no LDS variant was built or measured.)
//                         Two integer reductions per pose (vs_acc_reduce: wave shuffles, LDS, one integer atomic per value and tile).
//   scene_finish_kernel   per pose: gt_info's quotient and boxes (both gated on px_count_visib > 0), ok, slot.
// No floating-point atomics; no workgroup waits for another; nothing allocates or synchronises; every output is a function of integer
// counts and per-pixel values: bit-identical from call to call, for an image alone or in a batch, with or without backgrounds.
#include "render_shade.h"

namespace {

// 4-byte words per pose: render_shade.h's RR_HDR words | all, obj xmin ymin xmax ymax | valid visib, visib xmin ymin xmax ymax | slot | spare
constexpr int SL_HDR = 64;
constexpr int SL_CANVAS = RR_HDR, SL_NCANVAS = 5;        // 1 sum + a box: counted on the whole canvas
constexpr int SL_FRAME = SL_CANVAS + SL_NCANVAS, SL_NFRAME = 6;      // 2 sums + a box: counted in the frame
constexpr int SL_SLOT = SL_FRAME + SL_NFRAME;
constexpr int SL_MAX_POSES = 32;                         // per image: one bit each

struct SlParams {
  VsMesh mesh;
  const double* poses;        // (P, 12)
  const double* K;            // (9) or (I, 9)
  const float* colors;        // (sumV, 3) or nullptr
  const float* normals;
  const double* surf;         // (P, 3) or nullptr
  const int32_t* image_of_pose;   // (P)
  const int32_t* img_off;     // (I + 1)
  const int32_t* pose_order;  // (P)
  const uint8_t* backgrounds; // (n_bg, H, W, 3) or nullptr
  const int32_t* bg_index;    // (I) or nullptr
  uint8_t* rgb;               // (I, H, W, 3)
  float* depth;               // (I, H, W)
  uint32_t* full_bits;        // (I, H, W)
  uint32_t* visib_bits;       // (I, H, W)
  int32_t* slot;              // (P)
  int32_t* counts;            // (P, 3)
  double* fract;              // (P)
  int32_t* boxes;             // (P, 2, 4)
  uint8_t* ok;                // (P)
  int32_t* hdr;               // (P, SL_HDR)
  RrTables T;
  float delta;
  int bg[3];                  // the quantised bg_color
  int k_stride, P, I, H, W, n_bg, bgr, tx, ty, x0, y0, vchunks;
  RrTex X;                    // the texture tables, all null without textures
};

__global__ __launch_bounds__(VS_THREADS) void scene_pose_kernel(SlParams p) {
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * SL_HDR;
  int img;
  const bool img_ok = rr_scene_pose_head(p, b, h, img);
  for (int k = 0; k < SL_NCANVAS; ++k) h[SL_CANVAS + k] = vs_acc_identity<1>(k);
  for (int k = 0; k < SL_NFRAME; ++k) h[SL_FRAME + k] = vs_acc_identity<2>(k);
  int slot = -1;
  if (img_ok) {
    int j0, j1;
    vs_image_rows(p.img_off, p.P, img, SL_MAX_POSES, j0, j1);
    for (int j = j0; j < j1; ++j)
      if (slot < 0 && p.pose_order[j] == b) slot = j - j0;
  }
  h[SL_SLOT] = slot;
  for (int k = SL_SLOT + 1; k < SL_HDR; ++k) h[k] = 0;
}

__global__ __launch_bounds__(VS_THREADS) void scene_vertex_kernel(SlParams p) {      // the rectangle clamped to the canvas
  rr_vertex_body(p, SL_HDR, make_float4(-(float)p.W - 2.f, 2.f * (float)p.W + 1.f, -(float)p.H - 2.f, 2.f * (float)p.H + 1.f));
}

// bit s: the pose at slot s of image img (rows [j0, j1) of the CSR, at most 32) is rendered and its rectangle meets the tile at (ox, oy).
// Lane s of EVERY wave looks at slot s, so the dependent loads of all slots are in flight together and every wave holds the same mask:
// what the workgroup does with it is uniform.  A tile that no pose meets -- most of the canvas margin -- costs one such look.
__device__ __forceinline__ uint32_t sl_hits(const SlParams& p, int j0, int j1, int img, int ox, int oy) {
  const int j = j0 + (int)(threadIdx.x & 63);
  bool hit = false;
  if (j < j1) {
    const int b = p.pose_order[j];
    if (b >= 0 && b < p.P && p.image_of_pose[b] == img) {
      const int32_t* __restrict__ h = p.hdr + (size_t)b * SL_HDR;
      hit = h[RrH::OK] && !h[RrH::BAD(0)] && vs_tile_hit(h + RrH::RECT(0), ox, oy);
    }
  }
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)__ballot(hit));      // (j1 - j0 <= 32: the upper half is empty)
}

// (held to 3 waves per SIMD: left alone hipcc takes 174 VGPRs, 6 above what 3 waves allow; with the bound it takes 161, still without
// scratch, and a full device measured the call at 1.37 ms against 1.80 ms -- profiles/scene_bench.json)
// (the <true> instantiation needs the texel's words and blend weights on top: held to 3 waves it takes 168 VGPRs and 28 to 40 bytes of
// scratch per lane, so it is allowed 2 waves and takes them without scratch; the <false> one keeps its bound and its 161 VGPRs)
template <bool TEX>
__global__ __launch_bounds__(VS_THREADS) __attribute__((amdgpu_waves_per_eu(TEX ? 2 : 3, 3))) void scene_tile_kernel(SlParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  __shared__ int s_canvas[VS_WAVES][SL_NCANVAS];
  __shared__ int s_frame[VS_WAVES][SL_NFRAME];
  const VsTile c = vs_tile(p.tx, p.ty, p.x0, p.y0);
  const int img = c.b, ox = c.ox, oy = c.oy, lx = c.lx;              // first pixel, frame coordinates (any sign)
  const bool in_frame = ox >= 0 && ox < p.W && oy >= 0 && oy < p.H;  // the grid is anchored at frame pixel (0, 0)
  const int x = ox + lx;
  int j0, j1;
  vs_image_rows(p.img_off, p.P, img, SL_MAX_POSES, j0, j1);

  const uint32_t hits = sl_hits(p, j0, j1, img, ox, oy);

  if (!in_frame) {                                                   // (uniform) the margin: the truncated silhouette's count and box
    for (uint32_t left = hits; left; left &= left - 1) {
      const int b = p.pose_order[j0 + __ffs((int)left) - 1];
      int vfirst, V, ffirst, F, m;
      vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
      float dep[VS_PPL];
      vs_depth_tile(s_tri, &s_n, p.T.sv + (size_t)b * p.mesh.Vmax, p.mesh.faces + 3 * (size_t)ffirst, F, V, c, dep);
      int acc[SL_NCANVAS];
#pragma unroll
      for (int k = 0; k < SL_NCANVAS; ++k) acc[k] = vs_acc_identity<1>(k);
#pragma unroll
      for (int k = 0; k < VS_PPL; ++k) {
        const int y = oy + c.y(k);
        if (dep[k] > 0.f && x >= -p.W && x < 2 * p.W && y >= -p.H && y < 2 * p.H) {
          acc[0] += 1;
          acc[1] = min(acc[1], x); acc[2] = min(acc[2], y); acc[3] = max(acc[3], x); acc[4] = max(acc[4], y);
        }
      }
      vs_acc_reduce<1, SL_NCANVAS>(acc, s_canvas, p.hdr + (size_t)b * SL_HDR + SL_CANVAS);
      __syncthreads();                                               // s_canvas is read before the next pose writes it
    }
    return;
  }

  // ---- pass A: the composite depth (cp_vis_poses' update, on depths alone).  A tile that ONE pose meets has no use for it: the
  // composite there is that pose's own depth, which pass B takes from its walk (the same maximum of 1 / Z, the same division)
  float ren[VS_PPL];
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) ren[k] = 0.f;
  const bool alone = __popc(hits) == 1;                               // (uniform)
  for (uint32_t left = alone ? 0u : hits; left; left &= left - 1) {
    const int b = p.pose_order[j0 + __ffs((int)left) - 1];
    int vfirst, V, ffirst, F, m;
    vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
    float dep[VS_PPL];
    vs_depth_tile(s_tri, &s_n, p.T.sv + (size_t)b * p.mesh.Vmax, p.mesh.faces + 3 * (size_t)ffirst, F, V, c, dep);
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k)
      if (dep[k] != 0.f && (ren[k] == 0.f || dep[k] < ren[k])) ren[k] = dep[k];
  }

  // ---- pass B: every pose against the composite; the colour of the pose that owns the pixel
  const float fx0 = (float)ox + 0.5f, fy0 = (float)oy + 0.5f;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * img;
  const double kfx = K[0], kfy = K[4], kcx = K[2], kcy = K[5];
  uint32_t col[VS_PPL], fbits[VS_PPL], vbits[VS_PPL];                 // col: r | g << 8 | b << 16
  uint32_t owned = 0u;                                                // bit k: pixel k has its colour
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) { col[k] = 0u; fbits[k] = 0u; vbits[k] = 0u; }
  for (uint32_t left = hits; left; left &= left - 1) {
    const uint32_t bit = left & (0u - left);                          // the lowest slot left: poses in their order
    const int b = p.pose_order[j0 + __ffs((int)left) - 1];
    int32_t* __restrict__ h = p.hdr + (size_t)b * SL_HDR;
    int vfirst, V, ffirst, F, m;
    vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
    const int32_t* __restrict__ faces = p.mesh.faces + 3 * (size_t)ffirst;
    const size_t vbase = (size_t)b * p.mesh.Vmax;
    float best[VS_PPL];
    int face[VS_PPL];
    vs_raster_tile<true>(s_tri, &s_n, p.T.sv + vbase, faces, F, V, c, best, face);
    if (alone) {
#pragma unroll
      for (int k = 0; k < VS_PPL; ++k) ren[k] = vs_depth_of(best[k]);
    }
    float surf[3] = {0.5f, 0.5f, 0.5f};
    const float* __restrict__ colors = p.colors;
    if (p.surf) {
      colors = nullptr;
      for (int k = 0; k < 3; ++k) surf[k] = (float)p.surf[3 * (size_t)b + k];
    }
    const RrTexMesh tm = rr_tex_mesh(p.X, m, (size_t)vfirst, TEX && !p.surf);      // (uniform: one mesh per iteration)
    int acc_c[SL_NCANVAS], acc_f[SL_NFRAME];
#pragma unroll
    for (int k = 0; k < SL_NCANVAS; ++k) acc_c[k] = vs_acc_identity<1>(k);
#pragma unroll
    for (int k = 0; k < SL_NFRAME; ++k) acc_f[k] = vs_acc_identity<2>(k);
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) {
#pragma clang fp contract(off)
      const int ly = c.y(k);
      const int y = oy + ly;
      const float dg = vs_depth_of(best[k]);
      if (dg > 0.f && x >= -p.W && x < 2 * p.W && y >= -p.H && y < 2 * p.H) {      // the canvas (the tile may overhang the frame)
        acc_c[0] += 1;
        acc_c[1] = min(acc_c[1], x); acc_c[2] = min(acc_c[2], y); acc_c[3] = max(acc_c[3], x); acc_c[4] = max(acc_c[4], y);
      }
      if (x >= p.W || y >= p.H || dg == 0.f) continue;               // dist_gt == 0: neither mask is set, no count moves
      const double px = ((double)x - kcx) / kfx, py = ((double)y - kcy) / kfy;
      const double t_im = vs_dist(px, py, ren[k]), t_gt = vs_dist(px, py, dg);
      const bool mk = t_gt > 0.0, vis = vs_visible(t_im, t_gt, p.delta);
      if (mk) fbits[k] |= bit;
      if (mk && t_im > 0.0) acc_f[0] += 1;
      if (vis) {
        vbits[k] |= bit;
        acc_f[1] += 1;
        acc_f[2] = min(acc_f[2], x); acc_f[3] = min(acc_f[3], y); acc_f[4] = max(acc_f[4], x); acc_f[5] = max(acc_f[5], y);
      }
      if (dg == ren[k] && !((owned >> k) & 1u)) {                    // the first pose in order at the composite's depth
        owned |= 1u << k;
        int q[3];
        rr_shade<TEX>(p.T, colors, surf, tm, h, faces, vbase, (size_t)vfirst, face[k], fx0, fy0, (float)lx, (float)ly, q);
        col[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
      }
    }
    vs_acc_reduce<1, SL_NCANVAS>(acc_c, s_canvas, h + SL_CANVAS);
    vs_acc_reduce<2, SL_NFRAME>(acc_f, s_frame, h + SL_FRAME);
    __syncthreads();                                                  // both are read before the next pose writes them
  }

  // ---- the image's pixels, stored once
  int bgi = -1;                                                       // the image's row of the backgrounds, -1: bg_color
  if (p.backgrounds) {
    bgi = p.bg_index ? p.bg_index[img] : (p.n_bg == 1 ? 0 : img);
    if (bgi < 0 || bgi >= p.n_bg) bgi = -1;
  }
  const int c0 = p.bgr ? 2 : 0, c2 = p.bgr ? 0 : 2;
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) {
    const int y = oy + c.y(k);
    if (x >= p.W || y >= p.H) continue;
    const size_t at = ((size_t)img * p.H + y) * p.W + x;
    int r = p.bg[0], g = p.bg[1], bl = p.bg[2];
    if ((owned >> k) & 1u) {
      r = (int)(col[k] & 255u); g = (int)((col[k] >> 8) & 255u); bl = (int)((col[k] >> 16) & 255u);
    } else if (bgi >= 0) {
      const uint8_t* __restrict__ s = p.backgrounds + 3 * (((size_t)bgi * p.H + y) * p.W + x);
      r = s[0]; g = s[1]; bl = s[2];
    }
    p.rgb[3 * at + c0] = (uint8_t)r; p.rgb[3 * at + 1] = (uint8_t)g; p.rgb[3 * at + c2] = (uint8_t)bl;
    p.depth[at] = ren[k];
    p.full_bits[at] = fbits[k];
    p.visib_bits[at] = vbits[k];
  }
}

__global__ __launch_bounds__(VS_THREADS) void scene_finish_kernel(SlParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * SL_HDR;
  const bool live = h[RrH::OK] && !h[RrH::BAD(0)];
  const int all = live ? h[SL_CANVAS] : 0, valid = live ? h[SL_FRAME] : 0, visib = live ? h[SL_FRAME + 1] : 0;
  p.counts[3 * (size_t)b] = all;
  p.counts[3 * (size_t)b + 1] = valid;
  p.counts[3 * (size_t)b + 2] = visib;
  p.fract[b] = all > 0 ? (double)visib / (double)all : 0.0;
  vs_box_xywh(h + SL_CANVAS + 1, visib > 0, p.boxes + 8 * (size_t)b);          // bbox_obj is gated on the VISIBLE count too
  vs_box_xywh(h + SL_FRAME + 2, visib > 0, p.boxes + 8 * (size_t)b + 4);
  p.ok[b] = live ? 1 : 0;
  p.slot[b] = h[SL_SLOT];
}

}  // namespace

extern "C" size_t cp_render_scene_scratch_bytes(int P, int Vmax, int I) {
  if (P <= 0 || Vmax < 0 || I <= 0) return 0;
  return rr_scratch_bytes(P, Vmax, SL_HDR);
}

extern "C" int cp_render_scene_tex(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                                   const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                                   const float* colors, const float* normals, const double* surf_colors, const int32_t* image_of_pose,
                                   const int32_t* img_off, const int32_t* pose_order, const int32_t* img_off_host,
                                   const int32_t* pose_order_host, const uint8_t* backgrounds, int n_bg, const int32_t* bg_index,
                                   const double* bg_color, int shading, double ambient_weight, const double* light_pos, double delta,
                                   int bgr, int H, int W, int P, int I, int Vmax, uint8_t* rgb, float* depth, uint32_t* full_bits,
                                   uint32_t* visib_bits, int32_t* slot, int32_t* counts, double* visib_fract, int32_t* boxes, uint8_t* ok,
                                   void* scratch, const float* uv, const uint32_t* texels, const int32_t* tex_off,
                                   const int32_t* tex_dims, int filter) {
  SlParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !image_of_pose || !img_off || !pose_order || !img_off_host || !pose_order_host || !bg_color || !rgb || !depth ||
      !full_bits || !visib_bits || !slot || !counts || !visib_fract || !boxes || !ok || !scratch)
    return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, P) || I <= 0) return CP_ERR_INVALID;
  if ((bgr != 0 && bgr != 1) || !(delta == delta)) return CP_ERR_INVALID;
  if (backgrounds ? (n_bg <= 0 || (!bg_index && n_bg != 1 && n_bg != I)) : (n_bg != 0 || bg_index)) return CP_ERR_INVALID;
  if (const int e = rr_shading_args(shading, normals, ambient_weight, light_pos, uv, texels, tex_off, tex_dims, filter, p.T, p.X)) return e;
  if (!rr_finite3(bg_color)) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || cp_misaligned(surf_colors, 7) ||
      cp_misaligned(visib_fract, 7) || vs_mesh_misaligned(p.mesh) || cp_misaligned(colors, 3) || cp_misaligned(normals, 3) ||
      cp_misaligned(image_of_pose, 3) || cp_misaligned(img_off, 3) || cp_misaligned(pose_order, 3) || cp_misaligned(img_off_host, 3) ||
      cp_misaligned(pose_order_host, 3) || cp_misaligned(bg_index, 3) || cp_misaligned(depth, 3) || cp_misaligned(full_bits, 3) ||
      cp_misaligned(visib_bits, 3) || cp_misaligned(slot, 3) || cp_misaligned(counts, 3) || cp_misaligned(boxes, 3))
    return CP_ERR_ALIGN;
  if (vs_csr_invalid(img_off_host, pose_order_host, I, P)) return CP_ERR_INVALID;
  if (vs_csr_over(img_off_host, I, SL_MAX_POSES)) return CP_ERR_RANGE;                  // one bit per pose of an image
  if (W >= (1 << 24) || H >= (1 << 24) || (long long)I * H * W >= (1LL << 31) / 3 || (long long)H * W >= (1LL << 31) / 9)
    return CP_ERR_RANGE;
  if (backgrounds && (long long)n_bg * H * W >= (1LL << 31) / 3) return CP_ERR_RANGE;
  VsGrid gp, gi;
  if (!vs_grid(W, H, 1, false, P, 1, Vmax, gp) || !vs_grid(W, H, 1, true, I, 1, Vmax, gi)) return CP_ERR_RANGE;      // gp: its pose and vertex blocks
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.colors = colors; p.normals = normals; p.surf = surf_colors;
  p.image_of_pose = image_of_pose; p.img_off = img_off; p.pose_order = pose_order; p.backgrounds = backgrounds; p.n_bg = n_bg;
  p.bg_index = bg_index; p.rgb = rgb; p.depth = depth; p.full_bits = full_bits; p.visib_bits = visib_bits; p.slot = slot; p.counts = counts;
  p.fract = visib_fract; p.boxes = boxes; p.ok = ok; p.P = P; p.I = I; p.H = H; p.W = W; p.bgr = bgr; p.delta = (float)delta;
  for (int k = 0; k < 3; ++k) p.bg[k] = rr_quant_host(bg_color[k]);
  p.tx = gi.tx; p.ty = gi.ty; p.x0 = gi.x0; p.y0 = gi.y0; p.vchunks = gp.vchunks;
  rr_carve(scratch, P, Vmax, SL_HDR, p.hdr, p.T);
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(scene_pose_kernel, dim3(gp.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(scene_vertex_kernel, dim3(gp.vert_blocks), dim3(VS_THREADS), 0, st, p);
  RR_LAUNCH_TILE(scene_tile_kernel, texels != nullptr, dim3(gi.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(scene_finish_kernel, dim3(gp.pose_blocks), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}

extern "C" int cp_render_scene(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                               const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                               const float* colors, const float* normals, const double* surf_colors, const int32_t* image_of_pose,
                               const int32_t* img_off, const int32_t* pose_order, const int32_t* img_off_host,
                               const int32_t* pose_order_host, const uint8_t* backgrounds, int n_bg, const int32_t* bg_index,
                               const double* bg_color, int shading, double ambient_weight, const double* light_pos, double delta, int bgr,
                               int H, int W, int P, int I, int Vmax, uint8_t* rgb, float* depth, uint32_t* full_bits,
                               uint32_t* visib_bits, int32_t* slot, int32_t* counts, double* visib_fract, int32_t* boxes, uint8_t* ok,
                               void* scratch) {
  return cp_render_scene_tex(stream, poses, cam_K, k_stride, verts, v_offsets, faces, f_offsets, M, mesh_ids, colors, normals, surf_colors,
                             image_of_pose, img_off, pose_order, img_off_host, pose_order_host, backgrounds, n_bg, bg_index, bg_color,
                             shading, ambient_weight, light_pos, delta, bgr, H, W, P, I, Vmax, rgb, depth, full_bits, visib_bits, slot,
                             counts, visib_fract, boxes, ok, scratch, nullptr, nullptr, nullptr, nullptr, RR_NEAREST);
}
