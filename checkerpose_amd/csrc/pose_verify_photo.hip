// cp_verify_poses_photo: hypothesis verification of poses against the PHOTOGRAPH on the device -- the colour term
// beside row N26 (pose_verify.hip: the sensor's depth), row N28 (pose_verify_mask.hip: the predicted full mask) and row N31
// (scene_verify_mask.hip: an image's visible masks).  Those three see geometry only: a silhouette, and a depth render, does not change
// when a geometrically symmetric object (a can, a box, a bottle) turns about its axis; the printed label does.  A candidate pose's shaded
// render is correlated with the frame's pixels inside the raster tile: no frame, no render and no dense mask is stored, the outputs are
// integer sums and a zero-mean normalised cross-correlation of the lumas, which a gain and an offset of the brightness leave unchanged.
// The reference does not verify; opt-in, RGB-only, the rule is this project's own (tests/photo_stages.py restates it in numpy).  One more
// consumer of vsd_raster.h's scaffold and render_shade.h's shading.  The choice among candidates is row N26's cp_select_poses, unchanged.
//
// The rule, per pose p with frame i = image_ids[p] (frame 0 without ids) of the uint8 frames (I, H, W, 3).
//   Render.  C = the pose's shaded uint8 render at ssaa = 1, D = its depth: the bits cp_render_rgb_tex gives for the same shading, ambient
//            weight, light, surface colour, vertex colours and texture tables (the rules at the top of render_rgb.hip and render_shade.h).
//   Luma.    Y = (77 R + 150 G + 29 B + 128) >> 8 of the render and of the frame (weights sum to 256: R = G = B = g gives exactly g);
//            `bgr` swaps the two outer weights for the FRAME only (its bytes are then B G R).
//   Pixels.  Omega = {D > 0}, with the visible masks (coco_eval.PackedMasks bit rows: pixel x of a row is bit x & 31 of word x >> 5 of its
//            WW = ceil(W / 32) words) intersected with bit (y, x) of mask row m = mask_ids[p] (m = p without ids): where the object is
//            seen, and no occluder.
//   Sums.    With a = Y_render, b = Y_frame over Omega: n, Sa, Sb, Saa, Sbb, Sab, and n_model = |D > 0|: integers.  Frames are limited
//            to H W <= 2^22: a tile's sums fit int32 (1024 * 255^2 < 2^31), a pose's sums, n * Sab and Sa^2 fit int64
//            (2^22 * 2^22 * 255^2 < 2^63).  A larger frame is refused (CP_ERR_RANGE).
//   Finish.  (photo_finish_kernel, fp64 without contraction.)  Three exact int64 terms, each converted to double once:
//              cov = n Sab - Sa Sb      va = n Saa - Sa^2      vb = n Sbb - Sb^2
//              ncc = cov / sqrt(va * vb)     score = ncc     gain = cov / va     offset = (Sb - gain Sa) / n
//            The form gives identities: equal images give exactly 1.0 (sqrt(fl(v v)) == v under a correctly rounded sqrt), b = 2 a + 3
//            gives exactly 1.0 with gain exactly 2.0.
//   NaN.     ok = 0 and ncc, score, gain, offset are NaN when va == 0 (a flat render), vb == 0 (a flat frame patch), n < min_pixels, or
//            the pose is not counted at all: a non-finite pose or cam_K, a singular R (as cp_render_rgb), a vertex at Z <= 0, a mesh id,
//            image id or mask id out of range, an input status of 0 (the solvers' identity fallback, which must never win).  A pose that
//            is not counted reports zero sums.  min_pixels has no default here or anywhere: values below 2 are refused.
//
// Launches (four, render_rgb.hip's shape, whatever the data and the options):
//   photo_pose_kernel     per pose: rr_pose_record, validity, the image and mask rows, the 64-bit accumulators zeroed (a header of PH_HDR words).
//   photo_vertex_kernel   per (pose, 256 vertices): rr_vertex_body.
//   photo_tile_kernel     a workgroup per (pose, 32 x 32 frame tile); tile origins are multiples of 32, so one tile row of one mask is
//                         exactly ONE 32-bit word.  A tile the rectangle misses leaves at once.  Otherwise vs_raster_tile<true>, rr_shade<TEX>
//                         per covered pixel, the frame's three bytes (the 32 lanes of a row read 96 adjacent bytes), the row's mask word (a
//                         broadcast), seven int32 partial sums per lane, reduced through the wave (shuffles) and LDS (vs_acc_waves); ONE
//                         lane adds the tile's sums into the pose's 64-bit accumulators with integer atomics (order-free).
//                         photo_tile_kernel<false> (no texture tables) holds no texture code.
//   photo_finish_kernel   per pose: the counts, the sums, ok, ncc, score, gain, offset.
// No floating-point atomics; nothing allocates or synchronises; every output is a function of integer sums: bit-identical from call to
// call, for a pose alone or in a batch.
#include "render_shade.h"

namespace {

// 4-byte words per pose: RR_HDR words of a shaded pose (render_shade.h) | the image row (-1: none) | the mask row (-1: none) | seven
// 64-bit sums (8-byte aligned: 50 words in, headers of 64 words): n_model n Sa Sb Saa Sbb Sab
constexpr int PH_HDR = 64;
constexpr int PH_IMG = RR_HDR, PH_MASK = RR_HDR + 1, PH_ACC = RR_HDR + 2, PH_NACC = 7;
static_assert(PH_ACC % 2 == 0 && PH_ACC + 2 * PH_NACC <= PH_HDR, "the 64-bit accumulators are aligned and inside the header");
constexpr long long PH_MAX_PIXELS = 1LL << 22;

struct PhParams {
  VsMesh mesh;
  const double* poses;        // (P, 12)
  const double* K;
  const float* colors;        // (sumV, 3) in [0, 1], or nullptr: surf
  const float* normals;       // (sumV, 3), phong
  const uint8_t* frames;      // (I, H, W, 3)
  const int32_t* image_id;    // (P) or nullptr: image 0
  const uint32_t* vis;        // (NM, H, WW) or nullptr: no mask
  const int32_t* mask_id;     // (P) or nullptr: mask b
  const int32_t* status;      // (P) or nullptr: 0 = not a candidate
  int32_t* counts;            // (P, 2) n_model n
  int64_t* sums;              // (P, 5) Sa Sb Saa Sbb Sab
  double* ncc;                // (P)
  double* score;
  double* gain;
  double* offset;
  uint8_t* ok;                // (P)
  int32_t* hdr;               // (P, PH_HDR)
  RrTables T;                 // the (P, Vmax) tables, the light, the ambient weight, the shading (render_shade.h)
  float surf[3];
  int k_stride, P, I, NM, H, W, WW, bgr, min_pixels, tx, ty, vchunks;
  RrTex X;                    // the texture tables, all null without textures
};

// Y = (77 R + 150 G + 29 B + 128) >> 8
__device__ __forceinline__ int ph_luma(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }

__global__ __launch_bounds__(VS_THREADS) void photo_pose_kernel(PhParams p) {
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * PH_HDR;
  int vfirst, V, ffirst, F, m;
  bool ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  const int img = p.image_id ? p.image_id[b] : 0;
  const bool img_ok = img >= 0 && img < p.I;
  const int mask = p.vis ? (p.mask_id ? p.mask_id[b] : b) : -1;
  const bool mask_ok = !p.vis || (mask >= 0 && mask < p.NM);
  ok = ok && img_ok && mask_ok && (!p.status || p.status[b] != 0);
  rr_pose_record(p.K + (size_t)p.k_stride * b, p.poses + 12 * (size_t)b, 1.0, ok, h);
  h[PH_IMG] = img_ok ? img : -1;
  h[PH_MASK] = p.vis && mask_ok ? mask : -1;
  for (int k = PH_ACC; k < PH_HDR; ++k) h[k] = 0;
}

__global__ __launch_bounds__(VS_THREADS) void photo_vertex_kernel(PhParams p) {
  rr_vertex_body(p, PH_HDR, make_float4(-2.f, (float)p.W + 1.f, -2.f, (float)p.H + 1.f));
}

template <bool TEX>
__global__ __launch_bounds__(VS_THREADS) void photo_tile_kernel(PhParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  __shared__ int s_red[VS_WAVES][PH_NACC];
  const VsTile c = vs_tile(p.tx, p.ty, 0, 0);                         // first pixel: inside the frame (the grid covers the frame alone)
  const int b = c.b, ox = c.ox, oy = c.oy, lx = c.lx, H = p.H, W = p.W;
  int32_t* __restrict__ h = p.hdr + (size_t)b * PH_HDR;
  const bool live = h[RrH::OK] && !h[RrH::BAD(0)];
  if (!(live && vs_tile_hit(h + RrH::RECT(0), ox, oy))) return;       // (uniform)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  const int32_t* __restrict__ faces = p.mesh.faces + 3 * (size_t)ffirst;
  const size_t vbase = (size_t)b * p.mesh.Vmax;
  const RrTexMesh tm = rr_tex_mesh(p.X, m, (size_t)vfirst, TEX);      // (uniform: one mesh per workgroup)
  float best[VS_PPL];
  int face[VS_PPL];
  vs_raster_tile<true>(s_tri, &s_n, p.T.sv + vbase, faces, F, V, c, best, face);

  // (live, hence a checked image row and, with masks, a checked mask row)  the tile's word of mask row y is word ox >> 5 of the row: ox
  // is a multiple of 32 and < W, y < H
  const int img = h[PH_IMG], mask = h[PH_MASK];
  const uint8_t* __restrict__ frame = p.frames + (size_t)img * H * W * 3;
  const uint32_t* __restrict__ vis = mask >= 0 ? p.vis + ((size_t)mask * H) * p.WW + (size_t)(ox >> 5) : nullptr;
  const int c0 = p.bgr ? 2 : 0, c2 = p.bgr ? 0 : 2;
  const float fx0 = (float)ox + 0.5f, fy0 = (float)oy + 0.5f;
  const int x = ox + lx;
  int acc[PH_NACC];
#pragma unroll
  for (int k = 0; k < PH_NACC; ++k) acc[k] = 0;
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) {
    const int ly = c.y(k), y = oy + ly;
    if (x >= W || y >= H) continue;
    const size_t at = ((size_t)y * W + x) * 3;                        // the 32 lanes of a row: 96 adjacent bytes
    const int f0 = frame[at + c0], f1 = frame[at + 1], f2 = frame[at + c2];
    const uint32_t word = vis ? vis[(size_t)y * p.WW] : 0xffffffffu;  // every lane of the row reads the same word: a broadcast
    if (!(vs_depth_of(best[k]) > 0.f)) continue;                      // D > 0
    int col[3];
    rr_shade<TEX>(p.T, p.colors, p.surf, tm, h, faces, vbase, (size_t)vfirst, face[k], fx0, fy0, (float)lx, (float)ly, col);
    acc[0] += 1;
    if ((word >> lx) & 1u) {
      const int ya = ph_luma(col[0], col[1], col[2]), yb = ph_luma(f0, f1, f2);
      acc[1] += 1;
      acc[2] += ya; acc[3] += yb;
      acc[4] += ya * ya; acc[5] += yb * yb; acc[6] += ya * yb;       // a tile's sums fit int32: 1024 * 255^2 < 2^31
    }
  }
  vs_acc_waves<PH_NACC, PH_NACC>(acc, s_red);                         // (all sums; ends with a barrier)
  if (c.tid == 0) {                                                   // ONE lane: integer atomics, any order
    unsigned long long* __restrict__ dst = (unsigned long long*)(h + PH_ACC);
    for (int k = 0; k < PH_NACC; ++k) {
      int v = s_red[0][k];
      for (int w = 1; w < VS_WAVES; ++w) v += s_red[w][k];
      if (v != 0) atomicAdd(dst + k, (unsigned long long)v);
    }
  }
}

__global__ __launch_bounds__(VS_THREADS) void photo_finish_kernel(PhParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * PH_HDR;
  const bool live = h[RrH::OK] && !h[RrH::BAD(0)];
  const long long* __restrict__ s = (const long long*)(h + PH_ACC);
  const long long n_model = live ? s[0] : 0, n = live ? s[1] : 0;
  const long long Sa = live ? s[2] : 0, Sb = live ? s[3] : 0, Saa = live ? s[4] : 0, Sbb = live ? s[5] : 0, Sab = live ? s[6] : 0;
  p.counts[2 * (size_t)b] = (int32_t)n_model;                         // (H W <= 2^22)
  p.counts[2 * (size_t)b + 1] = (int32_t)n;
  int64_t* __restrict__ o = p.sums + 5 * (size_t)b;
  o[0] = Sa; o[1] = Sb; o[2] = Saa; o[3] = Sbb; o[4] = Sab;
  const long long cov = n * Sab - Sa * Sb, va = n * Saa - Sa * Sa, vb = n * Sbb - Sb * Sb;      // exact: < 2^63
  const bool ok = live && n >= (long long)p.min_pixels && va != 0 && vb != 0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double dcov = (double)cov, dva = (double)va, dvb = (double)vb;
  const double ncc = ok ? dcov / sqrt(dva * dvb) : nan;
  const double gain = ok ? dcov / dva : nan;
  p.ncc[b] = ncc;
  p.score[b] = ncc;
  p.gain[b] = gain;
  p.offset[b] = ok ? ((double)Sb - gain * (double)Sa) / (double)n : nan;
  p.ok[b] = ok ? 1 : 0;
}

}  // namespace

extern "C" size_t cp_verify_poses_photo_scratch_bytes(int P, int Vmax) {
  if (P <= 0 || Vmax < 0) return 0;
  return rr_scratch_bytes(P, Vmax, PH_HDR);
}

extern "C" int cp_verify_poses_photo_tex(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                                         const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M,
                                         const int32_t* mesh_ids, const float* colors, const float* normals, const double* surf_color,
                                         const double* light_pos, double ambient_weight, int shading, const uint8_t* frames,
                                         const int32_t* image_ids, int I, int H, int W, int bgr, const int32_t* vis_bits,
                                         const int32_t* mask_ids, int NM, const int32_t* status, int min_pixels, int P, int Vmax,
                                         int32_t* counts, int64_t* sums, double* ncc, double* score, double* gain, double* offset,
                                         uint8_t* ok, void* scratch, const float* uv, const uint32_t* texels, const int32_t* tex_off,
                                         const int32_t* tex_dims, int filter) {
  PhParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !surf_color || !frames || !counts || !sums || !ncc || !score || !gain || !offset || !ok || !scratch) return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, P) || vs_images_invalid(image_ids, I) || min_pixels < 2)
    return CP_ERR_INVALID;
  // the visible masks: none (then no ids and no count), or NM > 0 rows, a row per pose when there are no ids
  if (vis_bits ? (NM <= 0 || (!mask_ids && NM != P)) : (NM != 0 || mask_ids != nullptr)) return CP_ERR_INVALID;
  if (const int e = rr_shading_args(shading, normals, ambient_weight, light_pos, uv, texels, tex_off, tex_dims, filter, p.T, p.X)) return e;
  if (!rr_finite3(surf_color)) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || vs_mesh_misaligned(p.mesh) ||
      cp_misaligned(colors, 3) || cp_misaligned(normals, 3) || cp_misaligned(image_ids, 3) || cp_misaligned(vis_bits, 3) ||
      cp_misaligned(mask_ids, 3) || cp_misaligned(status, 3) || cp_misaligned(counts, 3) || cp_misaligned(sums, 7) || cp_misaligned(ncc, 7) ||
      cp_misaligned(score, 7) || cp_misaligned(gain, 7) || cp_misaligned(offset, 7))
    return CP_ERR_ALIGN;
  VsGrid g;
  if ((long long)H * W > PH_MAX_PIXELS || !vs_grid(W, H, 1, false, P, 1, Vmax, g)) return CP_ERR_RANGE;      // int32 tile sums, int64 products
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.colors = colors; p.normals = normals; p.frames = frames; p.image_id = image_ids;
  p.vis = (const uint32_t*)vis_bits; p.mask_id = mask_ids; p.status = status; p.counts = counts; p.sums = sums; p.ncc = ncc; p.score = score;
  p.gain = gain; p.offset = offset; p.ok = ok; p.P = P; p.I = I; p.NM = NM; p.H = H; p.W = W; p.WW = (W + 31) / 32; p.bgr = bgr ? 1 : 0;
  p.min_pixels = min_pixels;
  for (int k = 0; k < 3; ++k) p.surf[k] = (float)surf_color[k];
  p.tx = g.tx; p.ty = g.ty; p.vchunks = g.vchunks;
  rr_carve(scratch, P, Vmax, PH_HDR, p.hdr, p.T);
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(photo_pose_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(photo_vertex_kernel, dim3(g.vert_blocks), dim3(VS_THREADS), 0, st, p);
  RR_LAUNCH_TILE(photo_tile_kernel, texels != nullptr, dim3(g.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(photo_finish_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}

extern "C" int cp_verify_poses_photo(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                                     const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M,
                                     const int32_t* mesh_ids, const float* colors, const float* normals, const double* surf_color,
                                     const double* light_pos, double ambient_weight, int shading, const uint8_t* frames,
                                     const int32_t* image_ids, int I, int H, int W, int bgr, const int32_t* vis_bits,
                                     const int32_t* mask_ids, int NM, const int32_t* status, int min_pixels, int P, int Vmax,
                                     int32_t* counts, int64_t* sums, double* ncc, double* score, double* gain, double* offset,
                                     uint8_t* ok, void* scratch) {
  return cp_verify_poses_photo_tex(stream, poses, cam_K, k_stride, verts, v_offsets, faces, f_offsets, M, mesh_ids, colors, normals,
                                   surf_color, light_pos, ambient_weight, shading, frames, image_ids, I, H, W, bgr, vis_bits, mask_ids, NM,
                                   status, min_pixels, P, Vmax, counts, sums, ncc, score, gain, offset, ok, scratch, nullptr, nullptr,
                                   nullptr, nullptr, RR_NEAREST);
}
