// cp_render_rgb: shaded uint8 RGB frames of coloured meshes for a batch of poses on the device -- what
// bop_toolkit's scripts/render_train_imgs.py gets from renderer_py.RendererPython(mode='rgb') (renderer_py.py:24-105, 422-518) and, with
// ssaa > 1, from its 4x supersampled render followed by cv2.resize(INTER_AREA).  The reference renders through OpenGL, which does not
// run here: the shading is pinned to the RULE read from its GLSL, not to OpenGL's output.
//
// Shading rule, per sample.  Coverage and the front-most surface are vsd_raster.h's render rule and walk (vs_raster_tile<true>: at
// ssaa = 1 the depth is cp_render_depth's, bit for bit), which also names the winning face.  The varyings v_color,
// v_L = normalize(light - eye_pos) PER VERTEX and v_normal are interpolated perspective-correctly over the winner, with barycentrics
// recomputed from its vertices' screen records.
//   flat    f_normal = normalize(cross(dFdx(eye_pos), dFdy(eye_pos))): the unit face normal turned towards the viewer whatever the winding
//   phong   v_normal = normalize(u_nm * vec4(a_normal, 1.0)).xyz as the shader writes it: a FOUR-vector normalisation before .xyz, so
//           the per-vertex lengths differ and weight the interpolation (kept on purpose); u_nm = inverse(model-view)^T
//   light_w = min(1, ambient_w + max(dot(normalize(v_L), normalize(n)), 0));  colour = light_w * v_color
//   uint8 = round-half-even(255 * colour) on the fp32 value (np.round), clamped to 0..255; background = the quantised bg_color.
// The camera frame is OpenCV's (x right, y down, z forward); the reference's eye frame differs by a half turn about x, under which
// every dot product above is unchanged and the cross product turns with it.
//
// SSAA f in {1, 2, 4}: samples lie on the f-times finer grid under K * f (fx, fy, cx, cy all scaled: exact in binary).  Every sample
// is quantised to uint8 first; f x f samples are then averaged per output pixel as integers: (s + 2) >> 2 for f = 2, round-half-even of
// s / 16 for f = 4 (the project's statement of cv2.INTER_AREA's integer-factor path on 8-bit images; UNPINNED against cv2).
// A workgroup owns a 32 x 32 tile of the SAMPLE grid, i.e. exactly the tile a plain render at (f W, f H) under K * f owns, and runs
// the same arithmetic on it: the two are equal bit for bit.  The samples meet in LDS as integer sums (integer atomics: any order);
// no high-resolution image is ever stored.
//
// Textures (row N20): with the texture tables of cp_render_rgb_tex the colour of a textured mesh's sample is its texel -- the rule at the
// top of render_shade.h --; the tile launch is then rgb_tile_kernel<true> (the mesh, hence the colour source, is uniform over a
// workgroup), and without them rgb_tile_kernel<false>, which holds no texture code: the kernel this file had before textures, with the
// same registers, LDS, output bits and measured time; NOT the same instructions any more: the params struct's layout moved the argument
// loads and hipcc's schedule with them (profiles/raster_args_ab.json).
//
// Launches (four, whatever the data and the options):
//   rgb_pose_kernel     per pose: P = (K f)' [R | t] (vs_side_init), [R | t] and the normal matrix in fp32, validity, accumulators.
//   rgb_vertex_kernel   per (pose, 256 vertices): the screen record and the rectangle (vs_vertex_chunk), the eye position, v_L, for
//                       phong v_normal.
//   rgb_tile_kernel     a workgroup per (pose, 32 x 32 sample tile), 4 samples per lane.  Tiles the rectangle misses store the
//                       background and leave.  Otherwise: the walk, the shading of each covered sample, the stores; with f = 1 the
//                       optional depth, mask (0 / 255) and the box limits (integers: vs_acc_reduce).
//   rgb_finish_kernel   per pose: ok, the box as x, y, w, h (-1 when nothing is covered).
// No floating-point atomics; nothing allocates or synchronises; every output is bit-identical from call to call, for a pose alone or
// in a batch, with or without the optional outputs.
#include "render_shade.h"

namespace {

struct RrParams {
  VsMesh mesh;
  const double* poses;        // (B, 12)
  const double* K;
  const float* colors;        // (sumV, 3) in [0, 1], or nullptr: surf
  const float* normals;       // (sumV, 3), phong
  uint8_t* rgb;               // (B, H, W, 3)
  float* depth;               // (B, H, W) or nullptr
  uint8_t* mask;              // (B, H, W) or nullptr
  int32_t* boxes;             // (B, 4) or nullptr
  uint8_t* ok;                // (B)
  int32_t* hdr;               // (B, RR_HDR)
  RrTables T;                 // the (B, Vmax) tables, the light, the ambient weight, the shading (render_shade.h)
  float surf[3];
  int bg[3];                  // the quantised background
  int k_stride, B, H, W, f, bgr, tx, ty, vchunks;
  RrTex X;                    // the texture tables, all null without textures
};

__global__ __launch_bounds__(VS_THREADS) void rgb_pose_kernel(RrParams p) {
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.B) return;
  int vfirst, V, ffirst, F, m;
  const bool ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  rr_pose_record(p.K + (size_t)p.k_stride * b, p.poses + 12 * (size_t)b, (double)p.f, ok, p.hdr + (size_t)b * RR_HDR);
}

__global__ __launch_bounds__(VS_THREADS) void rgb_vertex_kernel(RrParams p) {
  rr_vertex_body(p, RR_HDR, make_float4(-2.f, (float)(p.f * p.W) + 1.f, -2.f, (float)(p.f * p.H) + 1.f));      // the sample grid
}

template <bool TEX>
__global__ __launch_bounds__(VS_THREADS) void rgb_tile_kernel(RrParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  __shared__ int s_red[VS_THREADS / 64][4];
  const VsTile c = vs_tile(p.tx, p.ty, 0, 0);                         // (of the SAMPLE grid)
  const int tid = c.tid, b = c.b, ox = c.ox, oy = c.oy, lx = c.lx;
  const int f = p.f, ot = VS_TILE / f;                                // output pixels per tile side
  int32_t* __restrict__ h = p.hdr + (size_t)b * RR_HDR;
  const bool live = h[RrH::OK] && !h[RrH::BAD(0)];
  const bool hit = live && vs_tile_hit(h + RrH::RECT(0), ox, oy);
  const int c0 = p.bgr ? 2 : 0, c2 = p.bgr ? 0 : 2;

  if (!hit) {                                                         // (uniform) background only
    for (int i = tid; i < ot * ot; i += VS_THREADS) {
      const int x = ox / f + i % ot, y = oy / f + i / ot;
      if (x < p.W && y < p.H) {
        const size_t at = ((size_t)b * p.H + y) * p.W + x;
        p.rgb[3 * at + c0] = (uint8_t)p.bg[0]; p.rgb[3 * at + 1] = (uint8_t)p.bg[1]; p.rgb[3 * at + c2] = (uint8_t)p.bg[2];
        if (p.depth) p.depth[at] = 0.f;
        if (p.mask) p.mask[at] = 0;
      }
    }
    return;
  }
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  const int32_t* __restrict__ faces = p.mesh.faces + 3 * (size_t)ffirst;
  const size_t vbase = (size_t)b * p.mesh.Vmax;
  const RrTexMesh tm = rr_tex_mesh(p.X, m, (size_t)vfirst, TEX);      // (uniform: one mesh per workgroup)
  float best[VS_PPL];
  int face[VS_PPL];
  vs_raster_tile<true>(s_tri, &s_n, p.T.sv + vbase, faces, F, V, c, best, face);

  // f >= 2: the samples' integer sums (at most 16 x 16 output pixels per tile) take over the triangle records' LDS after the walk
  int (*__restrict__ s_sum)[VS_TILE * VS_TILE / 4] = (int (*)[VS_TILE * VS_TILE / 4])s_tri;
  if (f > 1) {
    __syncthreads();                                                  // every wave has left the walk
    for (int i = tid; i < ot * ot; i += VS_THREADS) { s_sum[0][i] = 0; s_sum[1][i] = 0; s_sum[2][i] = 0; }
    __syncthreads();
  }
  const float fx0 = (float)ox + 0.5f, fy0 = (float)oy + 0.5f;
  int bx0 = INT_MAX, by0 = INT_MAX, bx1 = INT_MIN, by1 = INT_MIN;
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) {
    const int ly = c.y(k);
    const int sx = ox + lx, sy = oy + ly;                             // the sample, on the f W x f H grid
    if (sx >= f * p.W || sy >= f * p.H) continue;
    int col[3] = {p.bg[0], p.bg[1], p.bg[2]};
    const bool cov = best[k] > 0.f;
    if (cov) rr_shade<TEX>(p.T, p.colors, p.surf, tm, h, faces, vbase, (size_t)vfirst, face[k], fx0, fy0, (float)lx, (float)ly, col);
    if (f == 1) {
      const size_t at = ((size_t)b * p.H + sy) * p.W + sx;
      p.rgb[3 * at + c0] = (uint8_t)col[0]; p.rgb[3 * at + 1] = (uint8_t)col[1]; p.rgb[3 * at + c2] = (uint8_t)col[2];
      if (p.depth) p.depth[at] = vs_depth_of(best[k]);
      if (p.mask) p.mask[at] = cov ? 255 : 0;
      if (cov) { bx0 = min(bx0, sx); by0 = min(by0, sy); bx1 = max(bx1, sx); by1 = max(by1, sy); }
    } else {
      const int o = (ly / f) * ot + lx / f;
      atomicAdd(&s_sum[0][o], col[0]); atomicAdd(&s_sum[1][o], col[1]); atomicAdd(&s_sum[2][o], col[2]);
    }
  }
  if (f > 1) {
    __syncthreads();
    for (int i = tid; i < ot * ot; i += VS_THREADS) {
      const int x = ox / f + i % ot, y = oy / f + i / ot;
      if (x >= p.W || y >= p.H) continue;
      int v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int s = s_sum[c][i];
        if (f == 2) {
          v[c] = (s + 2) >> 2;
        } else {                                                      // round-half-even of s / 16
          const int q = s >> 4, r = s & 15;
          v[c] = q + ((r > 8 || (r == 8 && (q & 1))) ? 1 : 0);
        }
      }
      const size_t at = ((size_t)b * p.H + y) * p.W + x;
      p.rgb[3 * at + c0] = (uint8_t)v[0]; p.rgb[3 * at + 1] = (uint8_t)v[1]; p.rgb[3 * at + c2] = (uint8_t)v[2];
    }
    return;
  }
  if (!p.boxes) return;                                               // (uniform)
  const int acc[4] = {bx0, by0, bx1, by1};
  vs_acc_reduce<0, 4>(acc, s_red, h + RR_BOX);
}

__global__ __launch_bounds__(VS_THREADS) void rgb_finish_kernel(RrParams p) {
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.B) return;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * RR_HDR;
  const bool live = h[RrH::OK] && !h[RrH::BAD(0)];
  p.ok[b] = live ? 1 : 0;
  if (p.boxes) vs_box_xywh(h + RR_BOX, live && h[RR_BOX] != INT_MAX, p.boxes + 4 * (size_t)b);
}

}  // namespace

extern "C" size_t cp_render_rgb_scratch_bytes(int B, int Vmax) {
  if (B <= 0 || Vmax < 0) return 0;
  return rr_scratch_bytes(B, Vmax, RR_HDR);
}

extern "C" int cp_render_rgb_tex(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                                 const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                                 const float* colors, const float* normals, const double* surf_color, const double* light_pos,
                                 double ambient_weight, const double* bg_color, int shading, int ssaa, int bgr, int H, int W, int B,
                                 int Vmax, uint8_t* rgb, float* depth, uint8_t* mask, int32_t* boxes, uint8_t* ok, void* scratch,
                                 const float* uv, const uint32_t* texels, const int32_t* tex_off, const int32_t* tex_dims, int filter) {
  RrParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !surf_color || !bg_color || !rgb || !ok || !scratch) return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, B)) return CP_ERR_INVALID;
  if (ssaa != 1 && ssaa != 2 && ssaa != 4) return CP_ERR_INVALID;
  if (ssaa != 1 && (depth || mask || boxes)) return CP_ERR_INVALID;   // depth, mask and boxes belong to the ssaa = 1 sample grid
  if (const int e = rr_shading_args(shading, normals, ambient_weight, light_pos, uv, texels, tex_off, tex_dims, filter, p.T, p.X)) return e;
  if (!rr_finite3(surf_color) || !rr_finite3(bg_color)) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || vs_mesh_misaligned(p.mesh) ||
      cp_misaligned(colors, 3) || cp_misaligned(normals, 3) || cp_misaligned(depth, 3) || cp_misaligned(boxes, 3))
    return CP_ERR_ALIGN;
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.colors = colors; p.normals = normals; p.rgb = rgb; p.depth = depth; p.mask = mask;
  p.boxes = boxes; p.ok = ok; p.B = B; p.H = H; p.W = W; p.f = ssaa; p.bgr = bgr ? 1 : 0;
  for (int k = 0; k < 3; ++k) { p.surf[k] = (float)surf_color[k]; p.bg[k] = rr_quant_host(bg_color[k]); }
  const long long sw = (long long)ssaa * W, sh = (long long)ssaa * H;
  if (sw >= (1LL << 24) || sh >= (1LL << 24) || (long long)H * W >= (1LL << 31) / 3) return CP_ERR_RANGE;
  VsGrid g;
  if (!vs_grid(W, H, ssaa, false, B, 1, Vmax, g)) return CP_ERR_RANGE;
  p.tx = g.tx; p.ty = g.ty; p.vchunks = g.vchunks;
  rr_carve(scratch, B, Vmax, RR_HDR, p.hdr, p.T);
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(rgb_pose_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(rgb_vertex_kernel, dim3(g.vert_blocks), dim3(VS_THREADS), 0, st, p);
  RR_LAUNCH_TILE(rgb_tile_kernel, texels != nullptr, dim3(g.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(rgb_finish_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}

extern "C" int cp_render_rgb(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                             const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                             const float* colors, const float* normals, const double* surf_color, const double* light_pos,
                             double ambient_weight, const double* bg_color, int shading, int ssaa, int bgr, int H, int W, int B, int Vmax,
                             uint8_t* rgb, float* depth, uint8_t* mask, int32_t* boxes, uint8_t* ok, void* scratch) {
  return cp_render_rgb_tex(stream, poses, cam_K, k_stride, verts, v_offsets, faces, f_offsets, M, mesh_ids, colors, normals, surf_color,
                           light_pos, ambient_weight, bg_color, shading, ssaa, bgr, H, W, B, Vmax, rgb, depth, mask, boxes, ok, scratch,
                           nullptr, nullptr, nullptr, nullptr, RR_NEAREST);
}
