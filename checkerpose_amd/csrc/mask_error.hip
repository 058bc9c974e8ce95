// cp_mask_errors / cp_mask_overlap / cp_box_overlap: the four overlap errors that close bop_toolkit_lib/
// pose_error.py -- cou_mask :235-253, cus :256-286, cou_bb :289-297, cou_bb_proj :300-330, with misc.calc_2d_bbox / misc.iou
// (misc.py:202-263) -- for a batch of pairs on the device.  The reference renders the mesh twice per pair through OpenGL and then
// makes full-frame numpy passes; here both silhouettes of a 32 x 32 tile are rasterised by the same workgroup (vsd_raster.h's
// rasteriser, the render rule is stated there), so intersection and union are decided in registers and no image exists unless asked.
//
// Mask rule.  A pixel of a side is set exactly where cp_render_depth's depth is > 0: vs_depth_tile is called as cp_render_depth
// calls it (the frame's tile grid, the same arguments), the 1 / Z plane included -- a covered sample whose fp32 plane value is not
// positive is background there, so it is here.
//
// Launches of cp_mask_errors (four):
//   mask_error_pose_kernel    per pair: P = K' [R | t] of both sides (vs_side_init), validity, the caller's
//                             overlapping_sphere_projections shortcut (vs_sphere_skip), the rectangles and accumulators initialised.
//   mask_error_vertex_kernel  per (pair, side, 256 vertices): screen records, the side's pixel rectangle and its "a vertex at Z <= 0"
//                             flag through integer atomics (vs_vertex_chunk).
//   mask_error_tile_kernel    a workgroup per (pair, frame tile).  A tile outside both rectangles leaves at once (or writes zeros when
//                             the masks are asked).  Otherwise both sides' depths of its 1024 pixels, then four sums (inter, union,
//                             n_est, n_gt), four minima and four maxima (both silhouettes' xmin ymin xmax ymax) reduced as INTEGERS
//                             into the pair's accumulators (vs_acc_reduce).
//   mask_error_finish_kernel  per pair: cus = 1 - inter / (double)union (1.0 when union == 0) and cou_bb_proj = 1 - iou of the two
//                             boxes (x, y, xmax - xmin, ymax - ymin: no + 1, not clipped), integer arithmetic until the one quotient.
// The sphere shortcut belongs to 'cus' alone (eval_calc_errors.py:357-362): a skipped pair scores cus = 1.0 and is rendered only when
// cou_bb_proj is asked as well.  cp_mask_overlap is the counting half on caller-supplied masks: one launch, a workgroup per pair.
// Every output is a function of integer counts: bit-identical from call to call, for a pair alone or in a batch, with or without the
// optional outputs.  No floating-point atomics, no initialised scratch beyond what mask_error_pose_kernel writes.
#include "vsd_raster.h"

namespace {

// 4-byte words per pair: VsHdr<2> (P rect bad of both sides, ok) skip render | inter union n_est n_gt | est box | gt box
using MeH = VsHdr<2>;
constexpr int ME_HDR = 52;
constexpr int ME_SKIP = MeH::USER, ME_RENDER = ME_SKIP + 1, ME_ACC = ME_SKIP + 2, ME_NSUM = 4, ME_NACC = 12;
constexpr int MO_THREADS = 512;

struct MeParams {
  VsMesh mesh;
  const double* est;          // (B, 12)
  const double* gt;
  const double* K;
  const double* diameters;    // per mesh (the sphere shortcut) or nullptr
  double* cus;                // (B) or nullptr
  double* bbp;                // (B) or nullptr
  int32_t* counts;            // (B, 4) or nullptr
  int32_t* boxes;             // (B, 2, 4) or nullptr
  uint8_t* ok;                // (B) or nullptr
  uint8_t* masks;             // (B, 2, H, W) or nullptr
  int32_t* hdr;               // (B, ME_HDR)
  float4* sv;                 // (B, 2, Vmax)
  int k_stride, B, H, W, sphere, tx, ty, vchunks;
};

// 1 - misc.iou of two boxes x, y, w, h; T = long long (exact) or double (the caller's values): one quotient at the end
template <typename T>
__device__ __forceinline__ double me_cou_box(T ax, T ay, T aw, T ah, T bx, T by, T bw, T bh) {
#pragma clang fp contract(off)
  const T ar = ax + aw, ab = ay + ah, br = bx + bw, bb = by + bh;
  const T tlx = bx > ax ? bx : ax, tly = by > ay ? by : ay;              // Python's max(a, b): b only when it is larger
  const T brx = br < ar ? br : ar, bry = bb < ab ? bb : ab;              // min(a, b): b only when it is smaller
  const T wi = brx - tlx, hi = bry - tly;
  double iou = 0.0;
  if (wi > 0 && hi > 0) {
    const T inter = wi * hi, area_a = aw * ah, area_b = bw * bh;
    iou = (double)inter / (double)((area_a + area_b) - inter);
  }
  return 1.0 - iou;
}

// the results of four counts and two silhouettes [xmin ymin xmax ymax] (integers): cou_mask / cus, cou_bb / cou_bb_proj, counts, boxes
__device__ __forceinline__ void me_results(const int32_t* __restrict__ a, double& cou, double& cou_bb, int32_t* __restrict__ counts,
                                           int32_t* __restrict__ boxes) {
#pragma clang fp contract(off)
  const int inter = a[0], uni = a[1], n_est = a[2], n_gt = a[3];
  cou = uni > 0 ? 1.0 - (double)inter / (double)uni : 1.0;
  const int32_t* __restrict__ e = a + 4;
  const int32_t* __restrict__ g = a + 8;
  // the reference's xs.min() of an empty silhouette raises: NaN here
  cou_bb = (n_est > 0 && n_gt > 0) ? me_cou_box<long long>(e[0], e[1], (long long)e[2] - e[0], (long long)e[3] - e[1], g[0], g[1],
                                                           (long long)g[2] - g[0], (long long)g[3] - g[1])
                                   : __builtin_nan("");
  if (counts)
    for (int k = 0; k < 4; ++k) counts[k] = a[k];
  if (boxes)
    for (int s = 0; s < 2; ++s) vs_box_xywh(a + 4 + 4 * s, a[2 + s] > 0, boxes + 4 * s);
}

__global__ __launch_bounds__(VS_THREADS) void mask_error_pose_kernel(MeParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.B) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * ME_HDR;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  int vfirst, V, ffirst, F, m;
  bool ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  const double* __restrict__ e = p.est + 12 * (size_t)b;
  const double* __restrict__ g = p.gt + 12 * (size_t)b;
  ok = ok && vs_pose_finite(K, e) && vs_finite(g, 12);
  vs_side_init(K, 1.0, e, (float*)h + MeH::P(0), h + MeH::RECT(0));
  vs_side_init(K, 1.0, g, (float*)h + MeH::P(1), h + MeH::RECT(1));
  h[MeH::BAD(0)] = 0; h[MeH::BAD(1)] = 0;
  const int skip = (ok && p.sphere) ? vs_sphere_skip(e, g, p.diameters[m] / 2.0) : 0;
  h[MeH::OK] = ok ? 1 : 0;
  h[ME_SKIP] = skip;
  h[ME_RENDER] = (ok && !(skip && !p.bbp)) ? 1 : 0;                   // the shortcut is cus' alone: cou_bb_proj still renders
  for (int k = 0; k < ME_NACC; ++k) h[ME_ACC + k] = vs_acc_identity<ME_NSUM>(k);
  for (int k = ME_ACC + ME_NACC; k < ME_HDR; ++k) h[k] = 0;
}

__global__ __launch_bounds__(VS_THREADS) void mask_error_vertex_kernel(MeParams p) {
  int b, s, vc;
  vs_vertex_block(p.vchunks, 2, b, s, vc);
  int32_t* __restrict__ h = p.hdr + (size_t)b * ME_HDR;
  if (!h[ME_RENDER]) return;                                         // (uniform; no barrier in this kernel)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  vs_vertex_chunk((const float*)h + MeH::P(s), p.mesh.verts + 3 * (size_t)vfirst, V, vc, make_float4(-2.f, (float)p.W + 1.f, -2.f, (float)p.H + 1.f),
                  p.sv + ((size_t)b * 2 + s) * p.mesh.Vmax, h + MeH::RECT(s), h + MeH::BAD(s));
}

__global__ __launch_bounds__(VS_THREADS) void mask_error_tile_kernel(MeParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  __shared__ int s_red[VS_THREADS / 64][ME_NACC];
  const VsTile c = vs_tile(p.tx, p.ty, 0, 0);
  const int b = c.b, ox = c.ox, oy = c.oy;
  int32_t* __restrict__ h = p.hdr + (size_t)b * ME_HDR;
  const bool live = h[ME_RENDER] && !h[MeH::BAD(0)] && !h[MeH::BAD(1)];
  bool hit[2];
  for (int s = 0; s < 2; ++s) hit[s] = live && vs_tile_hit(h + MeH::RECT(s), ox, oy);
  // (uniform) with masks asked no tile leaves early: each one walks its pixels to store them, zeros where nothing is rendered
  if (!hit[0] && !hit[1] && !p.masks) return;
  const int x = ox + c.lx;
  float dep[2][VS_PPL];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) dep[s][k] = 0.f;
  if (hit[0] || hit[1]) {
    int vfirst, V, ffirst, F, m;
    vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (hit[s])                                                    // (uniform)
        vs_depth_tile(s_tri, &s_n, p.sv + ((size_t)b * 2 + s) * p.mesh.Vmax, p.mesh.faces + 3 * (size_t)ffirst, F, V, c, dep[s]);
  }

  int acc[ME_NACC];
#pragma unroll
  for (int k = 0; k < ME_NACC; ++k) acc[k] = vs_acc_identity<ME_NSUM>(k);
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) {
    const int y = oy + c.y(k);
    if (x >= p.W || y >= p.H) continue;
    const bool e = dep[0][k] > 0.f, g = dep[1][k] > 0.f;
    acc[0] += (e && g) ? 1 : 0;
    acc[1] += (e || g) ? 1 : 0;
    if (e) { acc[2] += 1; acc[4] = min(acc[4], x); acc[5] = min(acc[5], y); acc[6] = max(acc[6], x); acc[7] = max(acc[7], y); }
    if (g) { acc[3] += 1; acc[8] = min(acc[8], x); acc[9] = min(acc[9], y); acc[10] = max(acc[10], x); acc[11] = max(acc[11], y); }
    if (p.masks) {
      const size_t at = (((size_t)b * 2) * p.H + y) * p.W + x;
      p.masks[at] = e ? 1 : 0;
      p.masks[at + (size_t)p.H * p.W] = g ? 1 : 0;
    }
  }
  if (!hit[0] && !hit[1]) return;                                    // (uniform) zeros were stored, nothing to count

  vs_acc_reduce<ME_NSUM, ME_NACC>(acc, s_red, h + ME_ACC);
}

__global__ __launch_bounds__(VS_THREADS) void mask_error_finish_kernel(MeParams p) {
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.B) return;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * ME_HDR;
  const bool ok = h[MeH::OK] != 0, skip = h[ME_SKIP] != 0, rendered = h[ME_RENDER] != 0, bad = h[MeH::BAD(0)] || h[MeH::BAD(1)];
  int32_t a[ME_NACC];
  for (int k = 0; k < ME_NACC; ++k) a[k] = (rendered && !bad) ? h[ME_ACC + k] : vs_acc_identity<ME_NSUM>(k);
  double cou, cou_bb;
  me_results(a, cou, cou_bb, p.counts ? p.counts + 4 * (size_t)b : nullptr, p.boxes ? p.boxes + 8 * (size_t)b : nullptr);
  const double nan = __builtin_nan("");
  if (p.cus) p.cus[b] = !ok ? nan : (skip ? 1.0 : (bad ? nan : cou));
  if (p.bbp) p.bbp[b] = (!ok || bad) ? nan : cou_bb;
  if (p.ok) p.ok[b] = (ok && !(rendered && bad)) ? 1 : 0;
}

// ---- cp_mask_overlap: the counting on caller-supplied masks, a workgroup per pair
struct MoParams {
  const uint8_t* est;         // (B, H, W), nonzero = set
  const uint8_t* gt;
  double* cou_mask;           // (B) or nullptr
  double* cou_bb;             // (B) or nullptr
  int32_t* counts;            // (B, 4) or nullptr
  int32_t* boxes;             // (B, 2, 4) or nullptr
  int H, W, B;
};

__global__ __launch_bounds__(MO_THREADS) void mask_overlap_kernel(MoParams p) {
  __shared__ int s_red[MO_THREADS / 64][ME_NACC];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int n = p.H * p.W;                                           // (< 2^31: checked by the caller)
  const uint8_t* __restrict__ me = p.est + (size_t)b * n;
  const uint8_t* __restrict__ mg = p.gt + (size_t)b * n;
  const bool words = (((uintptr_t)me | (uintptr_t)mg) & 3) == 0;      // (uniform) both rows of this pair start on a 4-byte boundary
  int acc[ME_NACC];
#pragma unroll
  for (int k = 0; k < ME_NACC; ++k) acc[k] = vs_acc_identity<ME_NSUM>(k);
  for (int i = 4 * tid; i < n; i += 4 * MO_THREADS) {
    const int cnt = min(4, n - i);
    uint32_t we = 0, wg = 0;
    if (words && cnt == 4) {
      we = *(const uint32_t*)(me + i);
      wg = *(const uint32_t*)(mg + i);
    } else {
      for (int j = 0; j < cnt; ++j) { we |= (uint32_t)me[i + j] << (8 * j); wg |= (uint32_t)mg[i + j] << (8 * j); }
    }
    if (!(we | wg)) continue;
    int y = i / p.W, x = i - y * p.W;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool e = ((we >> (8 * j)) & 255u) != 0, g = ((wg >> (8 * j)) & 255u) != 0;
      acc[0] += (e && g) ? 1 : 0;
      acc[1] += (e || g) ? 1 : 0;
      if (e) { acc[2] += 1; acc[4] = min(acc[4], x); acc[5] = min(acc[5], y); acc[6] = max(acc[6], x); acc[7] = max(acc[7], y); }
      if (g) { acc[3] += 1; acc[8] = min(acc[8], x); acc[9] = min(acc[9], y); acc[10] = max(acc[10], x); acc[11] = max(acc[11], y); }
      if (++x == p.W) { x = 0; ++y; }
    }
  }
  vs_acc_waves<ME_NSUM, ME_NACC>(acc, s_red);
  if (tid == 0) {
    int32_t a[ME_NACC];
    for (int k = 0; k < ME_NACC; ++k) {
      int v = s_red[0][k];
      for (int w = 1; w < MO_THREADS / 64; ++w) v = vs_acc_combine<ME_NSUM>(k, v, s_red[w][k]);
      a[k] = v;
    }
    double cou, cou_bb;
    me_results(a, cou, cou_bb, p.counts ? p.counts + 4 * (size_t)b : nullptr, p.boxes ? p.boxes + 8 * (size_t)b : nullptr);
    if (p.cou_mask) p.cou_mask[b] = cou;
    if (p.cou_bb) p.cou_bb[b] = cou_bb;
  }
}

__global__ __launch_bounds__(VS_THREADS) void box_overlap_kernel(const double* __restrict__ a, const double* __restrict__ c,
                                                                 double* __restrict__ out, int B) {
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= B) return;
  const double* __restrict__ p = a + 4 * (size_t)b;
  const double* __restrict__ q = c + 4 * (size_t)b;
  out[b] = me_cou_box<double>(p[0], p[1], p[2], p[3], q[0], q[1], q[2], q[3]);
}

}  // namespace

extern "C" size_t cp_mask_errors_scratch_bytes(int B, int Vmax) {
  if (B <= 0 || Vmax < 0) return 0;
  return cp_align16_up((size_t)B * ME_HDR * sizeof(int32_t)) + cp_align16_up((size_t)B * 2 * Vmax * sizeof(float4));
}

extern "C" int cp_mask_errors(cp_stream_t stream, const double* pose_est, const double* pose_gt, const double* cam_K, int k_stride,
                              const float* verts, const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M,
                              const int32_t* mesh_ids, const double* diameters, int H, int W, int sphere_check, int B, int Vmax,
                              double* cus, double* cou_bb_proj, int32_t* counts, int32_t* boxes, uint8_t* ok, uint8_t* masks,
                              void* scratch) {
  MeParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!pose_est || !pose_gt || !scratch || (!cus && !cou_bb_proj) || (sphere_check && !diameters)) return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, B)) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(pose_est, 7) || cp_misaligned(pose_gt, 7) || vs_view_misaligned(cam_K) ||
      cp_misaligned(diameters, 7) || cp_misaligned(cus, 7) || cp_misaligned(cou_bb_proj, 7) || vs_mesh_misaligned(p.mesh) ||
      cp_misaligned(counts, 3) || cp_misaligned(boxes, 3))
    return CP_ERR_ALIGN;
  p.est = pose_est; p.gt = pose_gt; p.K = cam_K; p.k_stride = k_stride; p.diameters = diameters; p.H = H; p.W = W;
  p.sphere = sphere_check ? 1 : 0; p.B = B; p.cus = cus; p.bbp = cou_bb_proj; p.counts = counts; p.boxes = boxes; p.ok = ok; p.masks = masks;
  p.hdr = (int32_t*)scratch;
  p.sv = (float4*)((char*)scratch + cp_align16_up((size_t)B * ME_HDR * sizeof(int32_t)));
  VsGrid g;
  if (!vs_grid(W, H, 1, false, B, 2, Vmax, g) || (long long)H * W >= (1LL << 31)) return CP_ERR_RANGE;
  p.tx = g.tx; p.ty = g.ty; p.vchunks = g.vchunks;
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(mask_error_pose_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(mask_error_vertex_kernel, dim3(g.vert_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(mask_error_tile_kernel, dim3(g.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(mask_error_finish_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}

extern "C" int cp_mask_overlap(cp_stream_t stream, const uint8_t* mask_est, const uint8_t* mask_gt, int H, int W, int B,
                               double* cou_mask, double* cou_bb, int32_t* counts, int32_t* boxes) {
  if (!mask_est || !mask_gt || (!cou_mask && !cou_bb && !counts && !boxes)) return CP_ERR_INVALID;
  if (B <= 0 || H <= 0 || W <= 0) return CP_ERR_INVALID;
  if (cp_misaligned(cou_mask, 7) || cp_misaligned(cou_bb, 7) || cp_misaligned(counts, 3) || cp_misaligned(boxes, 3)) return CP_ERR_ALIGN;
  if ((long long)H * W >= (1LL << 31) - 4 * MO_THREADS || B >= (1 << 24)) return CP_ERR_RANGE;
  MoParams p = {};
  p.est = mask_est; p.gt = mask_gt; p.cou_mask = cou_mask; p.cou_bb = cou_bb; p.counts = counts; p.boxes = boxes; p.H = H; p.W = W; p.B = B;
  CP_LAUNCH(mask_overlap_kernel, dim3((unsigned)B), dim3(MO_THREADS), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}

extern "C" int cp_box_overlap(cp_stream_t stream, const double* bb_est, const double* bb_gt, int B, double* out) {
  if (!bb_est || !bb_gt || !out || B <= 0) return CP_ERR_INVALID;
  if (cp_misaligned(bb_est, 7) || cp_misaligned(bb_gt, 7) || cp_misaligned(out, 7)) return CP_ERR_ALIGN;
  CP_LAUNCH(box_overlap_kernel, dim3((unsigned)((B + VS_THREADS - 1) / VS_THREADS)), dim3(VS_THREADS), 0, (hipStream_t)stream, bb_est,
            bb_gt, out, B);
  return cp_check_launch();
}
