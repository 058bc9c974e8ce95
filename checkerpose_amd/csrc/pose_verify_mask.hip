// cp_verify_poses_mask: hypothesis verification of poses against the network's own predicted masks on the
// device -- the RGB-only twin of row N26 (pose_verify.hip), which reads the sensor's depth.  A candidate pose's rendered silhouette is
// compared with a packed mask (coco_eval.PackedMasks bit rows, as row N27's cp_paste_masks leaves them: the full, amodal mask is what a
// render of the object alone should look like) inside the raster tile: no depth frame and no dense mask exists, the outputs are integer
// counts.  The reference does not verify; opt-in, the rule is this project's own (tests/verify_mask_stages.py restates it in numpy).
// One more consumer of vsd_raster.h's scaffold.  The choice among candidates is row N26's cp_select_poses, unchanged.
//
// The rule, per pose p with mask row m = mask_ids[p] (m = p without ids).  D = the pose's depth render over the masks' W x H frame (the
// render rule is vsd_raster.h's, vs_depth_tile: the bits cp_render_depth gives).  A pixel is a MODEL pixel iff D > 0.  F = the full mask
// full_bits[m], V = the optional visible mask vis_bits[m]; pixel x of a row is bit x & 31 of word x >> 5 of its WW = ceil(W / 32) words
// (cp_coco_pack's layout).  The integer sums:
//   n_model = |D > 0|      n_inter = |model and F|      n_vis_in = |model and V| (0 without the visible masks)
// n_mask = full_area[m] and n_vis = vis_area[m] (0 without the visible masks) are READ, not recounted (rows N15 and N27 pin them); both
// are 0 for a mask id outside 0..NM-1.  box = xmin ymin xmax ymax of the model pixels, -1 four times when n_model == 0.
//
// Finish (pose_verify_mask_finish_kernel, fp64 without contraction):
//   union = n_model + n_mask - n_inter (as integers)      iou = n_inter / union      cover = n_vis_in / n_vis      score = iou
// score and iou are NaN with ok = 0 when union == 0, or when the pose is not counted at all (its three sums are then 0, its box -1s): a
// non-finite pose or cam_K, a vertex at Z <= 0, a mesh id out of range, a mask id outside 0..NM-1, an input status of 0 (the solvers'
// identity fallback, which must never win).  cover is NaN when n_vis == 0, without the visible masks, or when the pose is not counted.
// An empty full mask under a non-empty render scores exactly 0 with ok = 1.  cover is reported and NOT folded into the score: nothing in
// the project or the reference fixes a rule for combining the two, that stays the caller's choice.
//
// The optional label map (P, H, W) uint8: model | F << 1 | V << 2 per pixel.  A pose that is not counted still gets its mask bits (for a
// valid mask id; zeros for an invalid one).
//
// Launches of cp_verify_poses_mask (four, pose_verify.hip's shape):
//   pose_verify_mask_pose_kernel    per pose: P = K' [R | t] (vs_side_init), validity, the mask row, the accumulators at their identities.
//   pose_verify_mask_vertex_kernel  per (pose, 256 vertices): screen records (vs_vertex_chunk, cp_render_depth's clip) and the rectangle.
//   pose_verify_mask_tile_kernel    a workgroup per (pose, 32 x 32 frame tile).  Tile origins are multiples of 32, so one tile row of one
//                                   mask is exactly ONE 32-bit word.  A tile the rectangle misses leaves at once (after writing the mask
//                                   bits over its in-frame pixels when labels are asked for).  Otherwise vs_depth_tile, then each lane
//                                   tests D > 0 of its four pixels against bit lx of the row's word (one load per row that the 32 lanes
//                                   of the row share: a broadcast); the three sums and the box go through vs_acc_reduce<3, 7>.
//   pose_verify_mask_finish_kernel  per pose: the counts, the box, ok, iou, cover, score.
// Every output is a function of integer counts: bit-identical from call to call, for a pose alone or in a batch, with or without the
// labels.  No floating-point atomics, no initialised scratch beyond what pose_verify_mask_pose_kernel writes, no frame stored.
#include "vsd_raster.h"

namespace {

// 4-byte words per pose: VsHdr<1> (P rect bad ok) | n_model n_inter n_vis_in | xmin ymin xmax ymax | the mask row (-1: none)
using VmH = VsHdr<1>;
constexpr int VM_HDR = 32;
constexpr int VM_ACC = VmH::USER, VM_NSUM = 3, VM_NACC = 7, VM_MASK = VM_ACC + VM_NACC;
constexpr int VM_COUNTS = 5;                     // n_model n_inter n_vis_in n_mask n_vis
enum { VM_MODEL = 1, VM_FULL = 2, VM_VISIBLE = 4 };

struct VmParams {
  VsMesh mesh;
  const double* poses;        // (P, 12)
  const double* K;
  const uint32_t* full;       // (NM, H, WW)
  const int32_t* full_area;   // (NM)
  const uint32_t* vis;        // (NM, H, WW) or nullptr
  const int32_t* vis_area;    // (NM) or nullptr, with vis
  const int32_t* mask_id;     // (P) or nullptr: mask b
  const int32_t* status;      // (P) or nullptr: 0 = not a candidate
  int32_t* counts;            // (P, 5)
  int32_t* box;               // (P, 4)
  double* score;              // (P)
  double* iou;
  double* cover;
  uint8_t* ok;                // (P)
  uint8_t* labels;            // (P, H, W) or nullptr
  int32_t* hdr;               // (P, VM_HDR)
  float4* sv;                 // (P, Vmax)
  int k_stride, P, NM, H, W, WW, tx, ty, vchunks;
};

__global__ __launch_bounds__(VS_THREADS) void pose_verify_mask_pose_kernel(VmParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * VM_HDR;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  const double* __restrict__ q = p.poses + 12 * (size_t)b;
  bool ok = vs_pose_finite(K, q);
  const int mask = p.mask_id ? p.mask_id[b] : b;
  const bool have = mask >= 0 && mask < p.NM;
  ok = ok && have;
  int vfirst, V, ffirst, F, m;
  ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m) && ok;
  ok = ok && (!p.status || p.status[b] != 0);
  vs_side_init(K, 1.0, q, (float*)h + VmH::P(0), h + VmH::RECT(0));
  h[VmH::BAD(0)] = 0;
  h[VmH::OK] = ok ? 1 : 0;
  for (int k = 0; k < VM_NACC; ++k) h[VM_ACC + k] = vs_acc_identity<VM_NSUM>(k);
  h[VM_MASK] = have ? mask : -1;
  for (int k = VM_MASK + 1; k < VM_HDR; ++k) h[k] = 0;
}

__global__ __launch_bounds__(VS_THREADS) void pose_verify_mask_vertex_kernel(VmParams p) {
  int b, s, vc;
  vs_vertex_block(p.vchunks, 1, b, s, vc);
  int32_t* __restrict__ h = p.hdr + (size_t)b * VM_HDR;
  if (!h[VmH::OK]) return;                                           // (uniform; no barrier in this kernel)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  vs_vertex_chunk((const float*)h + VmH::P(0), p.mesh.verts + 3 * (size_t)vfirst, V, vc, make_float4(-2.f, (float)p.W + 1.f, -2.f, (float)p.H + 1.f),
                  p.sv + (size_t)b * p.mesh.Vmax, h + VmH::RECT(0), h + VmH::BAD(0));
}

__global__ __launch_bounds__(VS_THREADS) void pose_verify_mask_tile_kernel(VmParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  __shared__ int s_red[VS_THREADS / 64][VM_NACC];
  const VsTile c = vs_tile(p.tx, p.ty, 0, 0);
  const int b = c.b, ox = c.ox, oy = c.oy;                           // first pixel: inside the frame (the grid covers the frame alone)
  int32_t* __restrict__ h = p.hdr + (size_t)b * VM_HDR;
  const bool live = h[VmH::OK] && !h[VmH::BAD(0)];
  const bool hit = live && vs_tile_hit(h + VmH::RECT(0), ox, oy);
  const int x = ox + c.lx, H = p.H, W = p.W;
  const int mask = h[VM_MASK];                                       // a checked row, or -1
  // the tile's word of mask row y is word ox >> 5 of the row: ox is a multiple of 32 and < W, y < H, mask < NM
  const size_t word0 = ((size_t)max(mask, 0) * H) * p.WW + (size_t)(ox >> 5);
  const uint32_t* __restrict__ full = mask >= 0 ? p.full + word0 : nullptr;
  const uint32_t* __restrict__ vis = mask >= 0 && p.vis ? p.vis + word0 : nullptr;
  if (!hit) {                                                        // (uniform)
    if (p.labels) {
#pragma unroll
      for (int k = 0; k < VS_PPL; ++k) {
        const int y = oy + c.y(k);
        if (x >= W || y >= H) continue;
        const uint32_t fw = full ? full[(size_t)y * p.WW] : 0u, vw = vis ? vis[(size_t)y * p.WW] : 0u;
        p.labels[((size_t)b * H + y) * W + x] = (uint8_t)((((fw >> c.lx) & 1u) * VM_FULL) | (((vw >> c.lx) & 1u) * VM_VISIBLE));
      }
    }
    return;
  }
  float dep[VS_PPL];
  {
    const VsMesh mesh = p.mesh;                                     // (a copy, as in gt_info_tile_kernel)
    int vfirst, V, ffirst, F, m;
    vs_mesh_rows(mesh, b, vfirst, V, ffirst, F, m);
    vs_depth_tile(s_tri, &s_n, p.sv + (size_t)b * mesh.Vmax, mesh.faces + 3 * (size_t)ffirst, F, V, c, dep);
  }

  int acc[VM_NACC];
#pragma unroll
  for (int k = 0; k < VM_NACC; ++k) acc[k] = vs_acc_identity<VM_NSUM>(k);
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) {
    const int y = oy + c.y(k);
    if (x >= W || y >= H) continue;
    // (hit, hence a checked mask row)  every lane of the row reads the same word: a broadcast
    const uint32_t fw = full[(size_t)y * p.WW], vw = vis ? vis[(size_t)y * p.WW] : 0u;
    const uint32_t fbit = (fw >> c.lx) & 1u, vbit = (vw >> c.lx) & 1u;
    const bool model = dep[k] > 0.f;
    if (model) {
      acc[0] += 1;
      acc[1] += (int)fbit;
      acc[2] += (int)vbit;
      acc[3] = min(acc[3], x); acc[4] = min(acc[4], y);
      acc[5] = max(acc[5], x); acc[6] = max(acc[6], y);
    }
    if (p.labels) p.labels[((size_t)b * H + y) * W + x] = (uint8_t)((model ? VM_MODEL : 0) | (fbit * VM_FULL) | (vbit * VM_VISIBLE));
  }
  vs_acc_reduce<VM_NSUM, VM_NACC>(acc, s_red, h + VM_ACC);
}

__global__ __launch_bounds__(VS_THREADS) void pose_verify_mask_finish_kernel(VmParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * VM_HDR;
  const bool live = h[VmH::OK] && !h[VmH::BAD(0)];
  const int mask = h[VM_MASK];
  const int n_model = live ? h[VM_ACC] : 0, n_inter = live ? h[VM_ACC + 1] : 0, n_vis_in = live ? h[VM_ACC + 2] : 0;
  const int n_mask = mask >= 0 ? p.full_area[mask] : 0;
  const int n_vis = mask >= 0 && p.vis_area ? p.vis_area[mask] : 0;
  int32_t* __restrict__ n = p.counts + VM_COUNTS * (size_t)b;
  n[0] = n_model; n[1] = n_inter; n[2] = n_vis_in; n[3] = n_mask; n[4] = n_vis;
  for (int k = 0; k < 4; ++k) p.box[4 * (size_t)b + k] = n_model > 0 ? h[VM_ACC + VM_NSUM + k] : -1;
  const long long uni = (long long)n_model + (long long)n_mask - (long long)n_inter;
  const bool ok = live && uni != 0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double iou = ok ? (double)n_inter / (double)uni : nan;
  p.iou[b] = iou;
  p.score[b] = iou;
  p.cover[b] = live && n_vis != 0 ? (double)n_vis_in / (double)n_vis : nan;
  p.ok[b] = ok ? 1 : 0;
}

}  // namespace

extern "C" size_t cp_verify_poses_mask_scratch_bytes(int P, int Vmax) {
  if (P <= 0 || Vmax < 0) return 0;
  return cp_align16_up((size_t)P * VM_HDR * sizeof(int32_t)) + cp_align16_up((size_t)P * Vmax * sizeof(float4));
}

extern "C" int cp_verify_poses_mask(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                                    const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M,
                                    const int32_t* mesh_ids, const int32_t* full_bits, const int32_t* full_area, const int32_t* vis_bits,
                                    const int32_t* vis_area, const int32_t* mask_ids, int NM, int H, int W, const int32_t* status, int P,
                                    int Vmax, int32_t* counts, int32_t* box, double* score, double* iou, double* cover, uint8_t* ok,
                                    uint8_t* labels, void* scratch) {
  VmParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !full_bits || !full_area || !counts || !box || !score || !iou || !cover || !ok || !scratch) return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, P) || NM <= 0 || (!mask_ids && NM != P) ||
      (vis_bits != nullptr) != (vis_area != nullptr))                // the visible masks come with their areas, or not at all
    return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || cp_misaligned(score, 7) || cp_misaligned(iou, 7) ||
      cp_misaligned(cover, 7) || vs_mesh_misaligned(p.mesh) || cp_misaligned(full_bits, 3) || cp_misaligned(full_area, 3) ||
      cp_misaligned(vis_bits, 3) || cp_misaligned(vis_area, 3) || cp_misaligned(mask_ids, 3) || cp_misaligned(status, 3) ||
      cp_misaligned(counts, 3) || cp_misaligned(box, 3))
    return CP_ERR_ALIGN;
  VsGrid g;
  if ((long long)H * W > (1LL << 24) || !vs_grid(W, H, 1, false, P, 1, Vmax, g)) return CP_ERR_RANGE;      // int32 sums, as cp_verify_poses
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.full = (const uint32_t*)full_bits; p.full_area = full_area;
  p.vis = (const uint32_t*)vis_bits; p.vis_area = vis_area; p.mask_id = mask_ids; p.NM = NM; p.H = H; p.W = W; p.WW = (W + 31) / 32;
  p.status = status; p.P = P; p.counts = counts; p.box = box; p.score = score; p.iou = iou; p.cover = cover; p.ok = ok; p.labels = labels;
  p.tx = g.tx; p.ty = g.ty; p.vchunks = g.vchunks;
  p.hdr = (int32_t*)scratch;
  p.sv = (float4*)((char*)scratch + cp_align16_up((size_t)P * VM_HDR * sizeof(int32_t)));
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(pose_verify_mask_pose_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(pose_verify_mask_vertex_kernel, dim3(g.vert_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(pose_verify_mask_tile_kernel, dim3(g.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(pose_verify_mask_finish_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}
