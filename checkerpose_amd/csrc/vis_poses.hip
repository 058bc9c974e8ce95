// cp_vis_poses, cp_depth_diff_vis: the poses of an image drawn over the photograph, for a batch of images on the
// device -- what bop_toolkit_lib/visualization.py:90-235 (vis_object_poses, driven by scripts/vis_est_poses.py and vis_gt_poses.py)
// composes in numpy from one OpenGL frame of RGB and one of depth per pose.  Here the per-pose frames live in registers: a workgroup
// owns a 32 x 32 tile of ONE IMAGE and walks the image's poses in order; one composite per image is stored.  Text is out of scope.
//
// The rule, per image, poses in the order given (pose_order within [img_off[i], img_off[i + 1])):
//   m_rgb, m_depth of a pose = cp_render_rgb(ssaa 1, background 0 0 0, depth asked) of that pose alone, bit for bit: vsd_raster.h's
//   walk (vs_raster_tile<true>) on the same tile grid and render_shade.h's rr_shade, with the pose's own surface colour (surf_colors
//   row), the mesh's texture (row N20, cp_vis_poses_tex: render_shade.h's rule; the tile launch is then vis_scene_tile_kernel<true>, the
//   colour source uniform per iteration of the pose loop) or the mesh's colours;
//   ren_rgb = 0, ren_depth = 0;  m = m_depth != 0 and (ren_depth == 0 or m_depth < ren_depth) on the fp32 depths (strict: of two
//   equal depths the earlier pose keeps the pixel);  ren_depth[m] = m_depth;
//   resolve != 0: ren_rgb[m] = m_rgb;   resolve == 0: ren_rgb = min(255, ren_rgb + m_rgb) as integers;
//   box of a pose: over the pixels where ANY channel of m_rgb is > 0 (the reference's obj_mask: a black surface occludes but has no
//   box), as x, y, xmax - xmin, ymax - ymin, or -1 four times;
//   boxes layer: a pixel on the one-pixel outline through the inclusive corners (x, y), (x + w, y + h) of ANY pose's box of the image
//   holds int(c * 255) of box_color;   vis = min(255, (frame + ren_rgb) / 2 + layer) per channel, as integers.
//   A pose that cp_render_rgb does not render (a non-finite entry, a singular R, any vertex at Z <= 0, a bad mesh or image id) is
//   skipped: ok = 0, box -1.
//
// Launches of cp_vis_poses (four, whatever the data and the options):
//   vis_pose_kernel        per pose: render_shade.h's header under the pose's IMAGE's K, validity.
//   vis_vertex_kernel      per (pose, 256 vertices): the records cp_render_rgb makes.
//   vis_scene_tile_kernel  a workgroup per (image, 32 x 32 tile), 4 pixels per lane: the loop over the image's poses (bound: the
//                          image's count, at most P), a pose whose rectangle misses the tile skipped (uniform over the workgroup);
//                          per remaining pose the walk (face chunks: ceil(F / 256)), the shading, the update in registers, the
//                          pose's box limits (integers: vs_acc_reduce).  ren_rgb and ren_depth are stored once.
//   vis_finish_kernel      per pixel: the outline test against the image's boxes (complete only now) and the blend; per pose: ok, box.
//
// cp_depth_diff_vis (visualization.py:206-235 with depth_for_vis :76-88): dd = valid ? ren_depth - depth : 0 in fp32,
// valid = depth > 0 and ren_depth > 0;  red = 255 where valid and dd < delta;  m0 = min dd over ALL pixels;  x = dd - m0 (fp32);
// over x > 0, in fp64:  n = (x - mn) / (mx / s) + 0.2, mn = min x, mx = max (x - mn);  green = blue = (uint8)(255 n); all 0 where not
// valid.  mn comes from the second-smallest DISTINCT dd (subtracting m0 is monotone, and two distinct floats never subtract to 0),
// mx from the largest.  Fewer than three distinct dd: diff_ok = 0 and an all-zero picture (the reference raises or divides 0 by 0).
// stats = min, max, mean of dd over the valid pixels (NaN without any).
// Launches (five): dd_init_kernel; dd_reduce_kernel (per (image, 1024 pixels): min and max through order-preserving integer keys
// and integer atomics, the count, the tile's fp64 partial sum in a fixed order); dd_second_kernel (the smallest dd > m0, same keys);
// dd_stats_kernel (per image: the partials summed in tile order, the constants of the colouring); dd_colour_kernel (per pixel).
// No floating-point atomics anywhere; no workgroup waits for another; nothing allocates or synchronises; every output is
// bit-identical from call to call, for an image alone or in a batch.
#include "render_shade.h"

namespace {

struct VpParams {
  VsMesh mesh;
  const double* poses;        // (P, 12)
  const double* K;            // (9) or (I, 9)
  const float* colors;        // (sumV, 3) or nullptr
  const float* normals;
  const double* surf;         // (P, 3) or nullptr: the mesh's colours (0.5 grey without any)
  const int32_t* image_of_pose;   // (P)
  const int32_t* img_off;     // (I + 1)
  const int32_t* pose_order;  // (P)
  const uint8_t* frames;      // (I, H, W, 3)
  uint8_t* vis;               // (I, H, W, 3)
  uint8_t* ren_rgb;           // (I, H, W, 3)
  float* ren_depth;           // (I, H, W)
  int32_t* boxes;             // (P, 4)
  uint8_t* ok;                // (P)
  int32_t* hdr;               // (P, RR_HDR)
  RrTables T;
  int box_q[3];               // int(c * 255) of box_color
  int k_stride, P, I, H, W, resolve, draw_boxes, tx, ty, vchunks;
  RrTex X;                    // the texture tables, all null without textures
};

__global__ __launch_bounds__(VS_THREADS) void vis_pose_kernel(VpParams p) {
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  int img;
  rr_scene_pose_head(p, b, p.hdr + (size_t)b * RR_HDR, img);
}

__global__ __launch_bounds__(VS_THREADS) void vis_vertex_kernel(VpParams p) {
  rr_vertex_body(p, RR_HDR, make_float4(-2.f, (float)p.W + 1.f, -2.f, (float)p.H + 1.f));
}

template <bool TEX>
__global__ __launch_bounds__(VS_THREADS) void vis_scene_tile_kernel(VpParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  __shared__ int s_red[VS_THREADS / 64][4];
  const VsTile c = vs_tile(p.tx, p.ty, 0, 0);
  const int img = c.b, ox = c.ox, oy = c.oy, lx = c.lx;
  const float fx0 = (float)ox + 0.5f, fy0 = (float)oy + 0.5f;
  uint32_t col[VS_PPL];                                               // r | g << 8 | b << 16
  float dep[VS_PPL];
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) { col[k] = 0u; dep[k] = 0.f; }
  int j0, j1;
  vs_image_rows(p.img_off, p.P, img, j0, j1);
  for (int j = j0; j < j1; ++j) {                                     // (every test below is uniform over the workgroup)
    const int b = p.pose_order[j];
    if (b < 0 || b >= p.P || p.image_of_pose[b] != img) continue;
    int32_t* __restrict__ h = p.hdr + (size_t)b * RR_HDR;
    if (!h[RrH::OK] || h[RrH::BAD(0)] || !vs_tile_hit(h + RrH::RECT(0), ox, oy)) continue;
    int vfirst, V, ffirst, F, m;
    vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
    const int32_t* __restrict__ faces = p.mesh.faces + 3 * (size_t)ffirst;
    const size_t vbase = (size_t)b * p.mesh.Vmax;
    float best[VS_PPL];
    int face[VS_PPL];
    vs_raster_tile<true>(s_tri, &s_n, p.T.sv + vbase, faces, F, V, c, best, face);
    float surf[3] = {0.5f, 0.5f, 0.5f};
    const float* __restrict__ colors = p.colors;
    if (p.surf) {
      colors = nullptr;
      for (int k = 0; k < 3; ++k) surf[k] = (float)p.surf[3 * (size_t)b + k];
    }
    const RrTexMesh tm = rr_tex_mesh(p.X, m, (size_t)vfirst, TEX && !p.surf);      // (uniform: one mesh per iteration)
    int acc[4] = {INT_MAX, INT_MAX, INT_MIN, INT_MIN};
#pragma unroll
    for (int k = 0; k < VS_PPL; ++k) {
      const int ly = c.y(k);
      const int sx = ox + lx, sy = oy + ly;
      if (sx >= p.W || sy >= p.H || !(best[k] > 0.f)) continue;
      int q[3];
      rr_shade<TEX>(p.T, colors, surf, tm, h, faces, vbase, (size_t)vfirst, face[k], fx0, fy0, (float)lx, (float)ly, q);
      const float md = vs_depth_of(best[k]);
      const bool front = md != 0.f && (dep[k] == 0.f || md < dep[k]);
      if (front) dep[k] = md;
      if (p.resolve) {
        if (front) col[k] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
      } else {
        const int r = min(255, (int)(col[k] & 255u) + q[0]), g = min(255, (int)((col[k] >> 8) & 255u) + q[1]);
        const int bl = min(255, (int)((col[k] >> 16) & 255u) + q[2]);
        col[k] = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)bl << 16);
      }
      if (q[0] | q[1] | q[2]) { acc[0] = min(acc[0], sx); acc[1] = min(acc[1], sy); acc[2] = max(acc[2], sx); acc[3] = max(acc[3], sy); }
    }
    vs_acc_reduce<0, 4>(acc, s_red, h + RR_BOX);
    __syncthreads();                                                  // s_red is read before the next pose writes it
  }
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) {
    const int sx = ox + lx, sy = oy + c.y(k);
    if (sx >= p.W || sy >= p.H) continue;
    const size_t at = ((size_t)img * p.H + sy) * p.W + sx;
    p.ren_rgb[3 * at] = (uint8_t)(col[k] & 255u); p.ren_rgb[3 * at + 1] = (uint8_t)((col[k] >> 8) & 255u);
    p.ren_rgb[3 * at + 2] = (uint8_t)((col[k] >> 16) & 255u);
    p.ren_depth[at] = dep[k];
  }
}

__global__ __launch_bounds__(VS_THREADS) void vis_finish_kernel(VpParams p) {
  const size_t g = (size_t)blockIdx.x * VS_THREADS + threadIdx.x;
  if (g < (size_t)p.P) {
    const int32_t* __restrict__ h = p.hdr + g * RR_HDR;
    const bool live = h[RrH::OK] && !h[RrH::BAD(0)];
    p.ok[g] = live ? 1 : 0;
    vs_box_xywh(h + RR_BOX, live && h[RR_BOX] != INT_MAX, p.boxes + 4 * g);
  }
  const size_t hw = (size_t)p.H * p.W;
  if (g >= (size_t)p.I * hw) return;
  const int img = (int)(g / hw);
  const int y = (int)((g % hw) / p.W), x = (int)((g % hw) % p.W);
  bool on = false;
  if (p.draw_boxes) {
    int j0, j1;
    vs_image_rows(p.img_off, p.P, img, j0, j1);
    for (int j = j0; j < j1; ++j) {
      const int b = p.pose_order[j];
      if (b < 0 || b >= p.P || p.image_of_pose[b] != img) continue;
      const int32_t* __restrict__ h = p.hdr + (size_t)b * RR_HDR;
      if (!h[RrH::OK] || h[RrH::BAD(0)] || h[RR_BOX] == INT_MAX) continue;
      const int x0 = h[RR_BOX], y0 = h[RR_BOX + 1], x1 = h[RR_BOX + 2], y1 = h[RR_BOX + 3];
      on = on || (((x == x0 || x == x1) && y >= y0 && y <= y1) || ((y == y0 || y == y1) && x >= x0 && x <= x1));
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int v = (((int)p.frames[3 * g + ch] + (int)p.ren_rgb[3 * g + ch]) >> 1) + (on ? p.box_q[ch] : 0);
    p.vis[3 * g + ch] = (uint8_t)min(255, v);
  }
}

// ---- depth difference ------------------------------------------------------------------------------------------------------------
constexpr int DD_TILE = 4 * VS_THREADS;          // pixels per workgroup of the reductions
// 4-byte words per image: key min over all | key max over all | key min over valid | key max over valid | valid count | second key
constexpr int DD_HDR = 8;
constexpr int DD_ALLMIN = 0, DD_ALLMAX = 1, DD_VMIN = 2, DD_VMAX = 3, DD_COUNT = 4, DD_SECOND = 5;
constexpr int DD_CONST = 4;                      // doubles per image: m0, mn, mx / s, ok

struct DdParams {
  const float* ren;           // (I, H, W)
  const float* depth;         // (ND, H, W)
  const int32_t* image_id;    // (I) or nullptr: image i (ND == I) or image 0 (ND == 1)
  uint8_t* out;               // (I, H, W, 3)
  double* stats;              // (I, 3)
  uint8_t* diff_ok;           // (I)
  uint32_t* hdr;              // (I, DD_HDR)
  double* cst;                // (I, DD_CONST)
  double* part;               // (I, tiles)
  double s;
  float delta;
  int I, ND, H, W, tiles;
};

// fp32 -> a uint32 that orders as the floats do (NaN: above every number), and back
__device__ __forceinline__ uint32_t dd_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dd_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// dd at pixel `at` of image img, +0.0 where not valid (and for a zero difference: one key per value)
__device__ __forceinline__ float dd_at(const DdParams& p, int img, size_t at, bool& valid) {
#pragma clang fp contract(off)
  const size_t hw = (size_t)p.H * p.W;
  int src = p.image_id ? p.image_id[img] : (p.ND == 1 ? 0 : img);
  const bool src_ok = src >= 0 && src < p.ND;
  const float r = p.ren[(size_t)img * hw + at], d = src_ok ? p.depth[(size_t)src * hw + at] : 0.f;
  valid = d > 0.f && r > 0.f;
  const float dd = valid ? r - d : 0.f;
  return dd == 0.f ? 0.f : dd;
}

__global__ __launch_bounds__(VS_THREADS) void dd_init_kernel(DdParams p) {
  const int i = blockIdx.x * VS_THREADS + threadIdx.x;
  if (i >= p.I) return;
  uint32_t* __restrict__ h = p.hdr + (size_t)i * DD_HDR;
  h[DD_ALLMIN] = 0xffffffffu; h[DD_ALLMAX] = 0u; h[DD_VMIN] = 0xffffffffu; h[DD_VMAX] = 0u; h[DD_COUNT] = 0u; h[DD_SECOND] = 0xffffffffu;
  h[6] = 0u; h[7] = 0u;
}

__device__ __forceinline__ uint32_t dd_wave_min(uint32_t v) {
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, w, 64));
  return v;
}
__device__ __forceinline__ uint32_t dd_wave_max(uint32_t v) {
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, w, 64));
  return v;
}

__global__ __launch_bounds__(VS_THREADS) void dd_reduce_kernel(DdParams p) {
#pragma clang fp contract(off)
  __shared__ uint32_t s_k[VS_WAVES][5];
  __shared__ double s_sum[VS_WAVES];
  const int img = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
  const size_t hw = (size_t)p.H * p.W;
  uint32_t amin = 0xffffffffu, amax = 0u, vmin = 0xffffffffu, vmax = 0u, cnt = 0u;
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t at = (size_t)tile * DD_TILE + (size_t)k * VS_THREADS + threadIdx.x;
    if (at >= hw) continue;
    bool valid;
    const float dd = dd_at(p, img, at, valid);
    const uint32_t key = dd_key(dd);
    amin = min(amin, key); amax = max(amax, key);
    if (valid) { vmin = min(vmin, key); vmax = max(vmax, key); cnt += 1u; sum = sum + (double)dd; }
  }
  amin = dd_wave_min(amin); amax = dd_wave_max(amax); vmin = dd_wave_min(vmin); vmax = dd_wave_max(vmax);
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {                                   // a fixed tree: the same sum on every call
    cnt += (uint32_t)__shfl_xor((int)cnt, w, 64);
    sum = sum + __shfl_xor(sum, w, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_k[wave][0] = amin; s_k[wave][1] = amax; s_k[wave][2] = vmin; s_k[wave][3] = vmax; s_k[wave][4] = cnt;
    s_sum[wave] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < VS_WAVES; ++w) {
      amin = min(amin, s_k[w][0]); amax = max(amax, s_k[w][1]); vmin = min(vmin, s_k[w][2]); vmax = max(vmax, s_k[w][3]);
      cnt += s_k[w][4];
      sum = sum + s_sum[w];
    }
    uint32_t* __restrict__ h = p.hdr + (size_t)img * DD_HDR;
    atomicMin(h + DD_ALLMIN, amin); atomicMax(h + DD_ALLMAX, amax);
    if (cnt) { atomicMin(h + DD_VMIN, vmin); atomicMax(h + DD_VMAX, vmax); atomicAdd(h + DD_COUNT, cnt); }
    p.part[(size_t)img * p.tiles + tile] = sum;
  }
}

__global__ __launch_bounds__(VS_THREADS) void dd_second_kernel(DdParams p) {
  __shared__ uint32_t s_k[VS_WAVES];
  const int img = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
  const size_t hw = (size_t)p.H * p.W;
  uint32_t* __restrict__ h = p.hdr + (size_t)img * DD_HDR;
  const uint32_t k0 = h[DD_ALLMIN];
  uint32_t sec = 0xffffffffu;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t at = (size_t)tile * DD_TILE + (size_t)k * VS_THREADS + threadIdx.x;
    if (at >= hw) continue;
    bool valid;
    const uint32_t key = dd_key(dd_at(p, img, at, valid));
    if (key > k0) sec = min(sec, key);
  }
  sec = dd_wave_min(sec);
  if ((threadIdx.x & 63) == 0) s_k[threadIdx.x >> 6] = sec;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < VS_WAVES; ++w) sec = min(sec, s_k[w]);
    if (sec != 0xffffffffu) atomicMin(h + DD_SECOND, sec);
  }
}

__global__ __launch_bounds__(VS_THREADS) void dd_stats_kernel(DdParams p) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * VS_THREADS + threadIdx.x;
  if (i >= p.I) return;
  const uint32_t* __restrict__ h = p.hdr + (size_t)i * DD_HDR;
  const uint32_t cnt = h[DD_COUNT];
  double sum = 0.0;
  for (int t = 0; t < p.tiles; ++t) sum = sum + p.part[(size_t)i * p.tiles + t];      // tile order
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  p.stats[3 * (size_t)i] = cnt ? (double)dd_unkey(h[DD_VMIN]) : nan;
  p.stats[3 * (size_t)i + 1] = cnt ? (double)dd_unkey(h[DD_VMAX]) : nan;
  p.stats[3 * (size_t)i + 2] = cnt ? sum / (double)cnt : nan;
  // three distinct values at least: m0 < second < max
  const bool ok = h[DD_SECOND] != 0xffffffffu && h[DD_SECOND] < h[DD_ALLMAX];
  const float m0 = dd_unkey(h[DD_ALLMIN]);
  double* __restrict__ c = p.cst + (size_t)i * DD_CONST;
  c[0] = (double)m0;
  double mn = 0.0, den = 1.0;
  if (ok) {
    const float xs = dd_unkey(h[DD_SECOND]) - m0, xl = dd_unkey(h[DD_ALLMAX]) - m0;       // fp32, as depth_diff - depth_diff.min()
    mn = (double)xs;
    den = ((double)xl - mn) / p.s;
  }
  c[1] = mn; c[2] = den; c[3] = ok ? 1.0 : 0.0;
  p.diff_ok[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(VS_THREADS) void dd_colour_kernel(DdParams p) {
#pragma clang fp contract(off)
  const int img = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
  const size_t hw = (size_t)p.H * p.W;
  const double* __restrict__ c = p.cst + (size_t)img * DD_CONST;
  const float m0 = (float)c[0];
  const double mn = c[1], den = c[2];
  const bool ok = c[3] != 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t at = (size_t)tile * DD_TILE + (size_t)k * VS_THREADS + threadIdx.x;
    if (at >= hw) continue;
    bool valid;
    const float dd = dd_at(p, img, at, valid);
    int red = 0, gb = 0;
    if (ok && valid) {
      red = dd < p.delta ? 255 : 0;
      const float x = dd - m0;
      if (x > 0.f) {
        const double n = ((double)x - mn) / den + 0.2;
        gb = (int)(255.0 * n) & 255;
      }
    }
    uint8_t* __restrict__ o = p.out + 3 * ((size_t)img * hw + at);
    o[0] = (uint8_t)red; o[1] = (uint8_t)gb; o[2] = (uint8_t)gb;
  }
}

inline long long dd_tiles(int H, int W) { return ((long long)H * W + DD_TILE - 1) / DD_TILE; }

}  // namespace

extern "C" size_t cp_vis_poses_scratch_bytes(int P, int Vmax, int I) {
  if (P <= 0 || Vmax < 0 || I <= 0) return 0;
  return rr_scratch_bytes(P, Vmax, RR_HDR);
}

extern "C" int cp_vis_poses_tex(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                                const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                                const float* colors, const float* normals, const double* surf_colors, const int32_t* image_of_pose,
                                const int32_t* img_off, const int32_t* pose_order, const int32_t* img_off_host,
                                const int32_t* pose_order_host, const uint8_t* frames, int shading, double ambient_weight,
                                const double* light_pos, const double* box_color, int resolve, int draw_boxes, int H, int W, int P, int I,
                                int Vmax, uint8_t* vis, uint8_t* ren_rgb, float* ren_depth, int32_t* boxes, uint8_t* ok, void* scratch,
                                const float* uv, const uint32_t* texels, const int32_t* tex_off, const int32_t* tex_dims, int filter) {
  VpParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !image_of_pose || !img_off || !pose_order || !img_off_host || !pose_order_host || !frames || !box_color || !vis ||
      !ren_rgb || !ren_depth || !boxes || !ok || !scratch)
    return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, P) || I <= 0) return CP_ERR_INVALID;
  if ((resolve != 0 && resolve != 1) || (draw_boxes != 0 && draw_boxes != 1)) return CP_ERR_INVALID;
  if (const int e = rr_shading_args(shading, normals, ambient_weight, light_pos, uv, texels, tex_off, tex_dims, filter, p.T, p.X)) return e;
  if (!rr_finite3(box_color)) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || cp_misaligned(surf_colors, 7) ||
      vs_mesh_misaligned(p.mesh) || cp_misaligned(colors, 3) || cp_misaligned(normals, 3) || cp_misaligned(image_of_pose, 3) ||
      cp_misaligned(img_off, 3) || cp_misaligned(pose_order, 3) || cp_misaligned(img_off_host, 3) || cp_misaligned(pose_order_host, 3) ||
      cp_misaligned(ren_depth, 3) || cp_misaligned(boxes, 3))
    return CP_ERR_ALIGN;
  if (vs_csr_invalid(img_off_host, pose_order_host, I, P)) return CP_ERR_INVALID;
  if (W >= (1 << 24) || H >= (1 << 24) || (long long)I * H * W >= (1LL << 31) / 3) return CP_ERR_RANGE;
  VsGrid gp, gi;
  if (!vs_grid(W, H, 1, false, P, 1, Vmax, gp) || !vs_grid(W, H, 1, false, I, 1, Vmax, gi)) return CP_ERR_RANGE;
  const long long npix = (long long)I * H * W;
  const long long finish_blocks = ((npix > P ? npix : (long long)P) + VS_THREADS - 1) / VS_THREADS;
  if (finish_blocks >= (1LL << 24)) return CP_ERR_RANGE;
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.colors = colors; p.normals = normals; p.surf = surf_colors;
  p.image_of_pose = image_of_pose; p.img_off = img_off; p.pose_order = pose_order; p.frames = frames; p.vis = vis; p.ren_rgb = ren_rgb;
  p.ren_depth = ren_depth; p.boxes = boxes; p.ok = ok; p.P = P; p.I = I; p.H = H; p.W = W; p.resolve = resolve; p.draw_boxes = draw_boxes;
  for (int k = 0; k < 3; ++k) {
    const double q = box_color[k] * 255.0;                            // int(c * 255): truncation, then the uint8 range
    p.box_q[k] = q >= 255.0 ? 255 : (q > 0.0 ? (int)q : 0);
  }
  p.tx = gi.tx; p.ty = gi.ty; p.vchunks = gp.vchunks;
  rr_carve(scratch, P, Vmax, RR_HDR, p.hdr, p.T);
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(vis_pose_kernel, dim3(gp.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(vis_vertex_kernel, dim3(gp.vert_blocks), dim3(VS_THREADS), 0, st, p);
  RR_LAUNCH_TILE(vis_scene_tile_kernel, texels != nullptr, dim3(gi.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(vis_finish_kernel, dim3((unsigned)finish_blocks), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}

extern "C" int cp_vis_poses(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                            const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                            const float* colors, const float* normals, const double* surf_colors, const int32_t* image_of_pose,
                            const int32_t* img_off, const int32_t* pose_order, const int32_t* img_off_host,
                            const int32_t* pose_order_host, const uint8_t* frames, int shading, double ambient_weight,
                            const double* light_pos, const double* box_color, int resolve, int draw_boxes, int H, int W, int P, int I,
                            int Vmax, uint8_t* vis, uint8_t* ren_rgb, float* ren_depth, int32_t* boxes, uint8_t* ok, void* scratch) {
  return cp_vis_poses_tex(stream, poses, cam_K, k_stride, verts, v_offsets, faces, f_offsets, M, mesh_ids, colors, normals, surf_colors,
                          image_of_pose, img_off, pose_order, img_off_host, pose_order_host, frames, shading, ambient_weight, light_pos,
                          box_color, resolve, draw_boxes, H, W, P, I, Vmax, vis, ren_rgb, ren_depth, boxes, ok, scratch, nullptr, nullptr,
                          nullptr, nullptr, RR_NEAREST);
}

extern "C" size_t cp_depth_diff_vis_scratch_bytes(int I, int H, int W) {
  if (I <= 0 || H <= 0 || W <= 0) return 0;
  return cp_align16_up((size_t)I * DD_HDR * sizeof(uint32_t)) + cp_align16_up((size_t)I * DD_CONST * sizeof(double)) +
         cp_align16_up((size_t)I * (size_t)dd_tiles(H, W) * sizeof(double));
}

extern "C" int cp_depth_diff_vis(cp_stream_t stream, const float* ren_depth, const float* depth, const int32_t* image_ids, int n_depth,
                                 double delta, double s, int H, int W, int I, uint8_t* out, double* stats, uint8_t* diff_ok,
                                 void* scratch) {
  if (!ren_depth || !depth || !out || !stats || !diff_ok || !scratch) return CP_ERR_INVALID;
  if (I <= 0 || n_depth <= 0 || H <= 0 || W <= 0) return CP_ERR_INVALID;
  if (!image_ids && n_depth != 1 && n_depth != I) return CP_ERR_INVALID;
  if (!(delta == delta) || !__builtin_isfinite(s) || !(s > 0.0)) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(ren_depth, 3) || cp_misaligned(depth, 3) || cp_misaligned(image_ids, 3) ||
      cp_misaligned(stats, 7))
    return CP_ERR_ALIGN;
  if ((long long)H * W >= (1LL << 31) / 3) return CP_ERR_RANGE;
  const long long tiles = dd_tiles(H, W);
  if (tiles * I >= (1LL << 24)) return CP_ERR_RANGE;
  DdParams p = {};
  p.ren = ren_depth; p.depth = depth; p.image_id = image_ids; p.out = out; p.stats = stats; p.diff_ok = diff_ok; p.s = s;
  p.delta = (float)delta; p.I = I; p.ND = n_depth; p.H = H; p.W = W; p.tiles = (int)tiles;
  char* at = (char*)scratch;
  p.hdr = (uint32_t*)at; at += cp_align16_up((size_t)I * DD_HDR * sizeof(uint32_t));
  p.cst = (double*)at; at += cp_align16_up((size_t)I * DD_CONST * sizeof(double));
  p.part = (double*)at;
  hipStream_t st = (hipStream_t)stream;
  const unsigned per_image = (unsigned)((I + VS_THREADS - 1) / VS_THREADS), per_tile = (unsigned)(tiles * I);
  CP_LAUNCH(dd_init_kernel, dim3(per_image), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(dd_reduce_kernel, dim3(per_tile), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(dd_second_kernel, dim3(per_tile), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(dd_stats_kernel, dim3(per_image), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(dd_colour_kernel, dim3(per_tile), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}
