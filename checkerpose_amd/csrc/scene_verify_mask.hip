// cp_verify_scene_mask: the poses of an image verified TOGETHER against the network's visible masks on the device.
// Row N28 (pose_verify_mask.hip) scores every pose as if its object stood alone; here the counted poses of one image occlude each
// other -- the front-most composite and the BOP'19 visibility test are row N19's (scene_labels.hip) --, and what the scene predicts to be
// visible of a pose is counted against the pose's visible mask inside the raster tile: depth only, no shading, no frame and no dense mask
// stored.  The reference does not verify; opt-in, the rule is this project's own (tests/scene_verify_stages.py restates it in numpy).
// One more consumer of vsd_raster.h's scaffold.  The choice among candidates is row N26's cp_select_poses, unchanged.
//
// The rule.  All floating-point work after the render is fp64 without contraction.
//   Inputs.  P poses; pose p belongs to image image_ids[p] (0 .. I-1) and reads mask row m = mask_ids[p] (m = p without ids) of TWO sets
//   of NM packed masks of one W x H frame: the full masks F and the visible masks V (cp_coco_pack's layout: pixel x of a row is bit
//   x & 31 of word x >> 5 of its WW = ceil(W / 32) words; bits at columns >= W are never read).
//   Counted poses.  A pose is COUNTED unless: an entry of the pose or of its cam_K is not finite; a vertex is at Z <= 0; its mesh id, its
//   mask id or its image id is out of range; status[p] == 0; its slot (below) is 32 or more.  A pose that is not counted occludes
//   nothing: its sums are 0, its boxes -1s, ok = 0, its five quotients NaN.
//   Slots.  slot[p] = the rank of p among the poses of its image in the order given (the number of q < p with image_ids[q] ==
//   image_ids[p]), whether counted or not; -1 for an image id out of range.  At most 32 poses per image take part.
//   Render.  D_p = the pose's depth render over the frame alone (vs_depth_tile: cp_render_depth's bits).  A MODEL pixel has D_p > 0.
//   Composite.  ren(x) = the smallest positive D_p(x) over the counted poses of the image, 0 where there is none (of equal depths the
//   earlier slot owns the pixel: row N19's strict <; the value is the same either way).
//   Predicted-visible pixel of p.  A model pixel with vs_visible(vs_dist(ren), vs_dist(D_p), delta): row N19's 'bop19' test,
//   f32(dist_p) - f32(dist_ren) <= f32(delta), both distances (vs_dist: integer pixel coordinates, fp64) under pose p's OWN cam_K.
//   delta is in the unit of the meshes and t.  Two identical poses in one image are both fully visible, as in BOP's scene_gt_info.
//   Integer sums per pose, in the frame:  n_model = |model|   n_pvis = |pvis|   n_inter = |model and F|   n_vis_in = |model and V|
//   n_pvis_in = |pvis and V|;  box_model, box_pvis = xmin ymin xmax ymax of the model / predicted-visible pixels, -1 four times when
//   there is none.  READ, not recounted: n_mask = full_area[m], n_vis = vis_area[m] (both 0 for a mask id out of range).
//   Finish (scene_verify_finish_kernel), every quotient ONE fp64 division of integers:
//     iou = n_inter / (n_model + n_mask - n_inter)          cover = n_vis_in / n_vis              (NaN exactly where row N28 gives NaN)
//     iou_vis = n_pvis_in / (n_pvis + n_vis - n_pvis_in)    visib_fract = n_pvis / n_model        n_hidden_seen = n_vis_in - n_pvis_in
//     score = iou_vis
//   iou_vis and score are NaN with ok = 0 when their union is 0 (a fully hidden object under an empty visible mask) or the pose is not
//   counted; visib_fract is NaN when n_model == 0 or the pose is not counted.  How to combine iou and iou_vis stays the caller's choice.
//   Optional planes plane_full, plane_visib (I, H, W) int32: bit s is set where the pose at slot s of the image has a model pixel / a
//   predicted-visible pixel (row N19's layout).
//
// Launches of cp_verify_scene_mask (five, whatever the data):
//   scene_verify_table_kernel   the slot table (I, 32) of pose indices at -1.
//   scene_verify_pose_kernel    per pose: P = K' [R | t] (vs_side_init), validity, the mask row, its slot (a count over the ids before
//                               it), its entry of the table, the accumulators at their identities.
//   scene_verify_vertex_kernel  per (pose, 256 vertices): screen records (vs_vertex_chunk, cp_render_depth's clip) and the rectangle.
//   scene_verify_tile_kernel    a workgroup per (image, 32 x 32 frame tile), 4 pixels per lane.  Which of the image's poses meet the tile
//                               is decided once, a lane per slot (sv_hits: a 32-bit mask, uniform over the workgroup).  Pass A walks the
//                               hits depth-only -> ren in registers (skipped where ONE pose meets the tile: the composite there is that
//                               pose's own depth).  Pass B walks them again depth-only: the visibility test, and bit lx of the ONE word of
//                               the tile row of F and of V (tile origins are multiples of 32; the 32 lanes of a row share the load: a
//                               broadcast).  Five sums and two boxes go through vs_acc_reduce<5, 13>; the two plane words are stored once.
//   scene_verify_finish_kernel  per pose: the counts, the boxes, ok, slot, the five quotients.
// Every output is a function of integer counts and per-pixel values: bit-identical from call to call, for an image alone or in a batch,
// with or without the planes; a pose's outputs do not depend on what stands in other images.  No floating-point atomics, no workgroup
// waits for another, no initialised scratch beyond what the first two kernels write, no frame stored.
#include "vsd_raster.h"

namespace {

// 4-byte words per pose: VsHdr<1> (P rect bad ok) | the five sums | box_model | box_pvis | the mask row (-1: none) | slot | spare
using SvH = VsHdr<1>;
constexpr int SV_HDR = 48;
constexpr int SV_ACC = SvH::USER, SV_NSUM = 5, SV_NACC = 13, SV_MASK = SV_ACC + SV_NACC, SV_SLOT = SV_MASK + 1;
constexpr int SV_COUNTS = 8;                     // n_model n_pvis n_inter n_vis_in n_pvis_in n_mask n_vis n_hidden_seen
constexpr int SV_MAX_POSES = 32;                 // per image: one bit each

struct SvParams {
  VsMesh mesh;
  const double* poses;        // (P, 12)
  const double* K;            // (9) or (P, 9)
  const uint32_t* full;       // (NM, H, WW)
  const int32_t* full_area;   // (NM)
  const uint32_t* vis;        // (NM, H, WW)
  const int32_t* vis_area;    // (NM)
  const int32_t* mask_id;     // (P) or nullptr: mask b
  const int32_t* image_id;    // (P)
  const int32_t* status;      // (P) or nullptr: 0 = not a candidate
  int32_t* counts;            // (P, 8)
  int32_t* boxes;             // (P, 2, 4)
  int32_t* slot;              // (P)
  double* score;              // (P)
  double* iou;
  double* cover;
  double* iou_vis;
  double* fract;
  uint8_t* ok;                // (P)
  uint32_t* plane_full;       // (I, H, W) or nullptr
  uint32_t* plane_visib;      // (I, H, W) or nullptr, with plane_full
  int32_t* hdr;               // (P, SV_HDR)
  float4* sv;                 // (P, Vmax)
  int32_t* tab;               // (I, 32): the pose at each slot, -1: none
  float delta;
  int k_stride, P, I, NM, H, W, WW, tx, ty, vchunks;
};

__global__ __launch_bounds__(VS_THREADS) void scene_verify_table_kernel(SvParams p) {
  const long long i = (long long)blockIdx.x * VS_THREADS + threadIdx.x;
  if (i < (long long)p.I * SV_MAX_POSES) p.tab[i] = -1;
}

__global__ __launch_bounds__(VS_THREADS) void scene_verify_pose_kernel(SvParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * SV_HDR;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  const double* __restrict__ q = p.poses + 12 * (size_t)b;
  bool ok = vs_pose_finite(K, q);
  const int mask = p.mask_id ? p.mask_id[b] : b;
  const bool have = mask >= 0 && mask < p.NM;
  ok = ok && have;
  int vfirst, V, ffirst, F, m;
  ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m) && ok;
  ok = ok && (!p.status || p.status[b] != 0);
  const int img = p.image_id[b];
  int slot = -1;
  if (img >= 0 && img < p.I) {
    slot = 0;
    for (int j = 0; j < b; ++j) slot += p.image_id[j] == img ? 1 : 0;
  }
  const bool seated = slot >= 0 && slot < SV_MAX_POSES;
  if (seated) p.tab[(size_t)img * SV_MAX_POSES + slot] = b;           // (img, slot) names one pose: no two threads write one entry
  ok = ok && seated;
  vs_side_init(K, 1.0, q, (float*)h + SvH::P(0), h + SvH::RECT(0));
  h[SvH::BAD(0)] = 0;
  h[SvH::OK] = ok ? 1 : 0;
  for (int k = 0; k < SV_NACC; ++k) h[SV_ACC + k] = vs_acc_identity<SV_NSUM>(k);
  h[SV_MASK] = have ? mask : -1;
  h[SV_SLOT] = slot;
  for (int k = SV_SLOT + 1; k < SV_HDR; ++k) h[k] = 0;
}

__global__ __launch_bounds__(VS_THREADS) void scene_verify_vertex_kernel(SvParams p) {
  int b, s, vc;
  vs_vertex_block(p.vchunks, 1, b, s, vc);
  int32_t* __restrict__ h = p.hdr + (size_t)b * SV_HDR;
  if (!h[SvH::OK]) return;                                           // (uniform; no barrier in this kernel)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  vs_vertex_chunk((const float*)h + SvH::P(0), p.mesh.verts + 3 * (size_t)vfirst, V, vc, make_float4(-2.f, (float)p.W + 1.f, -2.f, (float)p.H + 1.f),
                  p.sv + (size_t)b * p.mesh.Vmax, h + SvH::RECT(0), h + SvH::BAD(0));
}

// bit s: the pose at slot s of image img is counted and its rectangle meets the tile at (ox, oy).  Lane s of EVERY wave looks at slot s,
// so the dependent loads of all slots are in flight together and every wave holds the same mask: what the workgroup does with it is
// uniform (scene_labels.hip's sl_hits, over the slot table).  A table entry is -1 or a pose index the pose kernel wrote; the range
// test bounds the header read whatever the memory holds.
__device__ __forceinline__ uint32_t sv_hits(const SvParams& p, const int32_t* __restrict__ row, int ox, int oy) {
  const int s = (int)(threadIdx.x & 63);
  bool hit = false;
  if (s < SV_MAX_POSES) {
    const int b = row[s];
    if (b >= 0 && b < p.P) {
      const int32_t* __restrict__ h = p.hdr + (size_t)b * SV_HDR;
      hit = h[SvH::OK] && !h[SvH::BAD(0)] && vs_tile_hit(h + SvH::RECT(0), ox, oy);
    }
  }
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)__ballot(hit));      // (lanes 32 .. 63 never hit: the upper half is empty)
}

__global__ __launch_bounds__(VS_THREADS) void scene_verify_tile_kernel(SvParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  __shared__ int s_red[VS_WAVES][SV_NACC];
  const VsTile c = vs_tile(p.tx, p.ty, 0, 0);
  const int img = c.b, ox = c.ox, oy = c.oy, lx = c.lx;              // first pixel: inside the frame (the grid covers the frame alone)
  const int x = ox + lx, H = p.H, W = p.W;
  const int32_t* __restrict__ row = p.tab + (size_t)img * SV_MAX_POSES;

  const uint32_t hits = sv_hits(p, row, ox, oy);

  // ---- pass A: the composite depth.  A tile that ONE pose meets has no use for it: the composite there is that pose's own depth
  float ren[VS_PPL];
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) ren[k] = 0.f;
  const bool alone = __popc(hits) == 1;                               // (uniform)
  for (uint32_t left = alone ? 0u : hits; left; left &= left - 1) {
    const int b = row[__ffs((int)left) - 1];                          // (a hit: a pose index in range)
    int vfirst, V, ffirst, F, m;
    vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
    float dep[VS_PPL];
    vs_depth_tile(s_tri, &s_n, p.sv + (size_t)b * p.mesh.Vmax, p.mesh.faces + 3 * (size_t)ffirst, F, V, c, dep);
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k)
      if (dep[k] > 0.f && (ren[k] == 0.f || dep[k] < ren[k])) ren[k] = dep[k];
  }

  // ---- pass B: every pose against the composite and against its two mask words
  uint32_t fbits[VS_PPL], vbits[VS_PPL];
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) { fbits[k] = 0u; vbits[k] = 0u; }
  for (uint32_t left = hits; left; left &= left - 1) {
    const uint32_t bit = left & (0u - left);                          // the lowest slot left: poses in their order
    const int b = row[__ffs((int)left) - 1];
    int32_t* __restrict__ h = p.hdr + (size_t)b * SV_HDR;
    int vfirst, V, ffirst, F, m;
    vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
    float dep[VS_PPL];
    vs_depth_tile(s_tri, &s_n, p.sv + (size_t)b * p.mesh.Vmax, p.mesh.faces + 3 * (size_t)ffirst, F, V, c, dep);
    if (alone) {
#pragma unroll
      for (int k = 0; k < VS_PPL; ++k) ren[k] = dep[k];
    }
    const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
    const double kfx = K[0], kfy = K[4], kcx = K[2], kcy = K[5];
    // the tile's word of mask row y is word ox >> 5 of the row: ox is a multiple of 32 and < W, y < H; a counted pose's mask row is
    // in 0 .. NM-1 (the clamp bounds the address whatever the header holds)
    const size_t word0 = ((size_t)min(max(h[SV_MASK], 0), p.NM - 1) * H) * p.WW + (size_t)(ox >> 5);
    const uint32_t* __restrict__ full = p.full + word0;
    const uint32_t* __restrict__ vism = p.vis + word0;
    int acc[SV_NACC];
#pragma unroll
    for (int k = 0; k < SV_NACC; ++k) acc[k] = vs_acc_identity<SV_NSUM>(k);
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) {
#pragma clang fp contract(off)
      const int y = oy + c.y(k);
      if (x >= W || y >= H || !(dep[k] > 0.f)) continue;             // no model pixel: no bit, no count moves
      const double px = ((double)x - kcx) / kfx, py = ((double)y - kcy) / kfy;
      const double t_ren = vs_dist(px, py, ren[k]), t_own = vs_dist(px, py, dep[k]);
      const bool pvis = vs_visible(t_ren, t_own, p.delta);
      // every lane of the row reads the same word: a broadcast
      const uint32_t fbit = (full[(size_t)y * p.WW] >> lx) & 1u, vbit = (vism[(size_t)y * p.WW] >> lx) & 1u;
      fbits[k] |= bit;
      acc[0] += 1;
      acc[2] += (int)fbit;
      acc[3] += (int)vbit;
      acc[5] = min(acc[5], x); acc[6] = min(acc[6], y); acc[7] = max(acc[7], x); acc[8] = max(acc[8], y);
      if (pvis) {
        vbits[k] |= bit;
        acc[1] += 1;
        acc[4] += (int)vbit;
        acc[9] = min(acc[9], x); acc[10] = min(acc[10], y); acc[11] = max(acc[11], x); acc[12] = max(acc[12], y);
      }
    }
    vs_acc_reduce<SV_NSUM, SV_NACC>(acc, s_red, h + SV_ACC);
    __syncthreads();                                                  // s_red is read before the next pose writes it
  }

  // ---- the image's two plane words, stored once (zeros where no pose meets the tile)
  if (p.plane_full) {
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) {
      const int y = oy + c.y(k);
      if (x >= W || y >= H) continue;
      const size_t at = ((size_t)img * H + y) * W + x;
      p.plane_full[at] = fbits[k];
      p.plane_visib[at] = vbits[k];
    }
  }
}

__global__ __launch_bounds__(VS_THREADS) void scene_verify_finish_kernel(SvParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * SV_HDR;
  const bool live = h[SvH::OK] && !h[SvH::BAD(0)];
  const int mask = h[SV_MASK];
  const int n_model = live ? h[SV_ACC] : 0, n_pvis = live ? h[SV_ACC + 1] : 0, n_inter = live ? h[SV_ACC + 2] : 0;
  const int n_vis_in = live ? h[SV_ACC + 3] : 0, n_pvis_in = live ? h[SV_ACC + 4] : 0;
  const int n_mask = mask >= 0 ? p.full_area[mask] : 0, n_vis = mask >= 0 ? p.vis_area[mask] : 0;
  int32_t* __restrict__ n = p.counts + SV_COUNTS * (size_t)b;
  n[0] = n_model; n[1] = n_pvis; n[2] = n_inter; n[3] = n_vis_in; n[4] = n_pvis_in; n[5] = n_mask; n[6] = n_vis; n[7] = n_vis_in - n_pvis_in;
  for (int k = 0; k < 4; ++k) {
    p.boxes[8 * (size_t)b + k] = n_model > 0 ? h[SV_ACC + SV_NSUM + k] : -1;
    p.boxes[8 * (size_t)b + 4 + k] = n_pvis > 0 ? h[SV_ACC + SV_NSUM + 4 + k] : -1;
  }
  const long long uni = (long long)n_model + (long long)n_mask - (long long)n_inter;
  const long long uni_vis = (long long)n_pvis + (long long)n_vis - (long long)n_pvis_in;
  const bool ok = live && uni_vis != 0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double iou_vis = ok ? (double)n_pvis_in / (double)uni_vis : nan;
  p.iou[b] = live && uni != 0 ? (double)n_inter / (double)uni : nan;
  p.cover[b] = live && n_vis != 0 ? (double)n_vis_in / (double)n_vis : nan;
  p.iou_vis[b] = iou_vis;
  p.score[b] = iou_vis;
  p.fract[b] = live && n_model != 0 ? (double)n_pvis / (double)n_model : nan;
  p.ok[b] = ok ? 1 : 0;
  p.slot[b] = h[SV_SLOT];
}

}  // namespace

extern "C" size_t cp_verify_scene_mask_scratch_bytes(int P, int Vmax, int I) {
  if (P <= 0 || Vmax < 0 || I <= 0) return 0;
  return cp_align16_up((size_t)P * SV_HDR * sizeof(int32_t)) + cp_align16_up((size_t)P * Vmax * sizeof(float4)) +
         cp_align16_up((size_t)I * SV_MAX_POSES * sizeof(int32_t));
}

extern "C" int cp_verify_scene_mask(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                                    const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M,
                                    const int32_t* mesh_ids, const int32_t* full_bits, const int32_t* full_area, const int32_t* vis_bits,
                                    const int32_t* vis_area, const int32_t* mask_ids, int NM, int H, int W, const int32_t* image_ids, int I,
                                    const int32_t* status, double delta, int P, int Vmax, int32_t* counts, int32_t* boxes, int32_t* slot,
                                    double* score, double* iou, double* cover, double* iou_vis, double* visib_fract, uint8_t* ok,
                                    int32_t* plane_full, int32_t* plane_visib, void* scratch) {
  SvParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !full_bits || !full_area || !vis_bits || !vis_area || !image_ids || !counts || !boxes || !slot || !score || !iou || !cover ||
      !iou_vis || !visib_fract || !ok || !scratch)
    return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, P) || NM <= 0 || (!mask_ids && NM != P) || I <= 0 ||
      (plane_full != nullptr) != (plane_visib != nullptr) ||          // the planes come together, or not at all
      !(delta >= 0.0) || !(delta <= 3.0e38))                          // finite, not negative, a float32
    return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || cp_misaligned(score, 7) || cp_misaligned(iou, 7) ||
      cp_misaligned(cover, 7) || cp_misaligned(iou_vis, 7) || cp_misaligned(visib_fract, 7) || vs_mesh_misaligned(p.mesh) ||
      cp_misaligned(full_bits, 3) || cp_misaligned(full_area, 3) || cp_misaligned(vis_bits, 3) || cp_misaligned(vis_area, 3) ||
      cp_misaligned(mask_ids, 3) || cp_misaligned(image_ids, 3) || cp_misaligned(status, 3) || cp_misaligned(counts, 3) ||
      cp_misaligned(boxes, 3) || cp_misaligned(slot, 3) || cp_misaligned(plane_full, 3) || cp_misaligned(plane_visib, 3))
    return CP_ERR_ALIGN;
  VsGrid gp, gi;
  if ((long long)H * W > (1LL << 24) || !vs_grid(W, H, 1, false, P, 1, Vmax, gp) || !vs_grid(W, H, 1, false, I, 1, Vmax, gi))
    return CP_ERR_RANGE;                                              // int32 sums, as cp_verify_poses_mask; gp: its pose and vertex blocks
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.full = (const uint32_t*)full_bits; p.full_area = full_area;
  p.vis = (const uint32_t*)vis_bits; p.vis_area = vis_area; p.mask_id = mask_ids; p.image_id = image_ids; p.NM = NM; p.H = H; p.W = W;
  p.WW = (W + 31) / 32; p.status = status; p.P = P; p.I = I; p.delta = (float)delta; p.counts = counts; p.boxes = boxes; p.slot = slot;
  p.score = score; p.iou = iou; p.cover = cover; p.iou_vis = iou_vis; p.fract = visib_fract; p.ok = ok;
  p.plane_full = (uint32_t*)plane_full; p.plane_visib = (uint32_t*)plane_visib;
  p.tx = gi.tx; p.ty = gi.ty; p.vchunks = gp.vchunks;
  const size_t hdr_bytes = cp_align16_up((size_t)P * SV_HDR * sizeof(int32_t)), sv_bytes = cp_align16_up((size_t)P * Vmax * sizeof(float4));
  p.hdr = (int32_t*)scratch;
  p.sv = (float4*)((char*)scratch + hdr_bytes);
  p.tab = (int32_t*)((char*)scratch + hdr_bytes + sv_bytes);
  const unsigned table_blocks = (unsigned)(((long long)I * SV_MAX_POSES + VS_THREADS - 1) / VS_THREADS);      // I < 2^24: fits
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(scene_verify_table_kernel, dim3(table_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(scene_verify_pose_kernel, dim3(gp.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(scene_verify_vertex_kernel, dim3(gp.vert_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(scene_verify_tile_kernel, dim3(gi.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(scene_verify_finish_kernel, dim3(gp.pose_blocks), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}
