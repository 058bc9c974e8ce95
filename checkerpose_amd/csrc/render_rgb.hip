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
#include "vsd_raster.h"

namespace {

// 4-byte words per pose: VsHdr<1> (P rect bad ok) | RT[12] | NM[12] = N (3x3) c (3) | box xmin ymin xmax ymax | sign(fx fy) | spare
using RrH = VsHdr<1>;
constexpr int RR_HDR = 48;
constexpr int RR_RT = RrH::USER, RR_NM = RR_RT + 12, RR_BOX = RR_NM + 12, RR_SK = RR_BOX + 4;
enum { RR_FLAT = 0, RR_PHONG = 1 };

struct RrParams {
  const double* poses;        // (B, 12)
  const double* K;
  const float* verts;
  const int32_t* v_off;
  const int32_t* faces;       // (sumF, 3), indices local to the mesh
  const int32_t* f_off;
  const int32_t* mesh_id;
  const float* colors;        // (sumV, 3) in [0, 1], or nullptr: surf
  const float* normals;       // (sumV, 3), phong
  uint8_t* rgb;               // (B, H, W, 3)
  float* depth;               // (B, H, W) or nullptr
  uint8_t* mask;              // (B, H, W) or nullptr
  int32_t* boxes;             // (B, 4) or nullptr
  uint8_t* ok;                // (B)
  int32_t* hdr;               // (B, RR_HDR)
  float4* sv;                 // (B, Vmax) screen records
  float4* eye;                // (B, Vmax)
  float4* vl;                 // (B, Vmax)
  float4* vn;                 // (B, Vmax), phong
  float surf[3], light[3], ambient;
  int bg[3];                  // the quantised background
  int k_stride, M, B, Vmax, H, W, f, shading, bgr, tx, ty, vchunks;
};

// round-half-even(255 v) of an fp32 colour value, clamped to 0..255 (NaN -> 0)
__device__ __forceinline__ int rr_quant(float v) {
#pragma clang fp contract(off)
  const float q = rintf(255.0f * v);
  return q >= 255.f ? 255 : (q > 0.f ? (int)q : 0);
}

__global__ __launch_bounds__(VS_THREADS) void rgb_pose_kernel(RrParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.B) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * RR_HDR;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  int vfirst, V, ffirst, F, m;
  bool ok = vs_mesh_rows(p.mesh_id, p.v_off, p.f_off, p.M, p.Vmax, b, vfirst, V, ffirst, F, m);
  const double* __restrict__ q = p.poses + 12 * (size_t)b;
  ok = ok && vs_pose_finite(K, q);
  vs_side_init(K, (double)p.f, q, (float*)h + RrH::P(0), h + RrH::RECT(0));      // P = (K f)' [R | t]
  float* __restrict__ rt = (float*)(h + RR_RT);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) rt[4 * r + c] = (float)q[3 * r + c];
    rt[4 * r + 3] = (float)q[9 + r];
  }
  // u_nm = inverse([R t; 0 1])^T = [R^-T 0; -(R^-1 t)^T 1]: N = R^-T (cofactors / det), c = R^-1 t = N^T t
  const double c00 = q[4] * q[8] - q[5] * q[7], c01 = q[5] * q[6] - q[3] * q[8], c02 = q[3] * q[7] - q[4] * q[6];
  const double c10 = q[2] * q[7] - q[1] * q[8], c11 = q[0] * q[8] - q[2] * q[6], c12 = q[1] * q[6] - q[0] * q[7];
  const double c20 = q[1] * q[5] - q[2] * q[4], c21 = q[2] * q[3] - q[0] * q[5], c22 = q[0] * q[4] - q[1] * q[3];
  const double det = (q[0] * c00 + q[1] * c01) + q[2] * c02;
  ok = ok && isfinite(det) && det != 0.0;
  const double N[9] = {c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det};
  float* __restrict__ nm = (float*)(h + RR_NM);
  for (int k = 0; k < 9; ++k) nm[k] = (float)N[k];
  for (int c = 0; c < 3; ++c) nm[9 + c] = (float)((N[c] * q[9] + N[3 + c] * q[10]) + N[6 + c] * q[11]);
  h[RrH::BAD(0)] = 0;
  h[RrH::OK] = ok ? 1 : 0;
  vs_rect_set(h + RR_BOX, INT_MAX, INT_MAX, INT_MIN, INT_MIN);
  h[RR_SK] = (K[0] > 0.0) == (K[4] > 0.0) ? 1 : -1;
  h[RR_SK + 1] = 0;
}

__global__ __launch_bounds__(VS_THREADS) void rgb_vertex_kernel(RrParams p) {
#pragma clang fp contract(off)
  int b, s, vc;
  vs_vertex_block(p.vchunks, 1, b, s, vc);
  int32_t* __restrict__ h = p.hdr + (size_t)b * RR_HDR;
  if (!h[RrH::OK]) return;                                           // (uniform; no barrier in this kernel)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh_id, p.v_off, p.f_off, p.M, p.Vmax, b, vfirst, V, ffirst, F, m);
  const float4 grid = make_float4(-2.f, (float)(p.f * p.W) + 1.f, -2.f, (float)(p.f * p.H) + 1.f);      // the sample grid
  // besides the screen record: the eye position, v_L and, for phong, v_normal of the vertex
  const auto shading_records = [&](int i, const float* __restrict__ vt) {
#pragma clang fp contract(off)
    const size_t at = (size_t)b * p.Vmax + i;
    const float* __restrict__ rt = (const float*)(h + RR_RT);
    const float ex = vs_affine(rt, vt[0], vt[1], vt[2]), ey = vs_affine(rt + 4, vt[0], vt[1], vt[2]), ez = vs_affine(rt + 8, vt[0], vt[1], vt[2]);
    p.eye[at] = make_float4(ex, ey, ez, 0.f);
    const float lx = p.light[0] - ex, ly = p.light[1] - ey, lz = p.light[2] - ez;
    const float ll = sqrtf((lx * lx + ly * ly) + lz * lz);
    p.vl[at] = make_float4(lx / ll, ly / ll, lz / ll, 0.f);
    if (p.shading == RR_PHONG) {
      const float* __restrict__ nm = (const float*)(h + RR_NM);
      const float* __restrict__ nr = p.normals + 3 * ((size_t)vfirst + i);
      const float nx = fmaf(nm[2], nr[2], fmaf(nm[1], nr[1], nm[0] * nr[0]));
      const float ny = fmaf(nm[5], nr[2], fmaf(nm[4], nr[1], nm[3] * nr[0]));
      const float nz = fmaf(nm[8], nr[2], fmaf(nm[7], nr[1], nm[6] * nr[0]));
      const float nw = 1.0f - fmaf(nm[11], nr[2], fmaf(nm[10], nr[1], nm[9] * nr[0]));
      const float nl = sqrtf(((nx * nx + ny * ny) + nz * nz) + nw * nw);    // the shader's 4-vector length
      p.vn[at] = make_float4(nx / nl, ny / nl, nz / nl, 0.f);
    }
  };
  vs_vertex_chunk((const float*)h + RrH::P(0), p.verts + 3 * (size_t)vfirst, V, vc, grid, p.sv + (size_t)b * p.Vmax, h + RrH::RECT(0),
                  h + RrH::BAD(0), shading_records);
}

__device__ __forceinline__ float rr_mix(float w0, float w1, float w2, float a, float c, float d) {
#pragma clang fp contract(off)
  return (w0 * a + w1 * c) + w2 * d;
}

// the same interpolation with w0 = 1 - w1 - w2 implied: three equal values give that value EXACTLY (a mesh of one colour, the 0.5
// grey a mesh without colours gets inside a coloured MeshSet), whatever the weights' rounded sum is
__device__ __forceinline__ float rr_mix_col(float w1, float w2, float a, float c, float d) {
#pragma clang fp contract(off)
  return a + (w1 * (c - a) + w2 * (d - a));
}

// the shaded, quantised colour of the sample (qx, qy) (tile-relative indices) on face fidx
__device__ __forceinline__ void rr_shade(const RrParams& p, const int32_t* __restrict__ h, const int32_t* __restrict__ faces, size_t vbase,
                                         size_t cbase, int fidx, float fx0, float fy0, float qx, float qy, int (&out)[3]) {
#pragma clang fp contract(off)
  const int32_t* __restrict__ fi = faces + 3 * (size_t)fidx;
  const int i0 = fi[0], i1 = fi[1], i2 = fi[2];
  const float4 a = p.sv[vbase + i0], c = p.sv[vbase + i1], d = p.sv[vbase + i2];
  const float ax = a.x - fx0, ay = a.y - fy0, cx = c.x - fx0, cy = c.y - fy0, dx = d.x - fx0, dy = d.y - fy0;
  const float area = (cx - ax) * (dy - ay) - (dx - ax) * (cy - ay);   // (the walk's expression: the same bits, never 0 here)
  // edge i is opposite vertex i, differences first; perspective-correct weights w_i = E_i / Z_i / sum_j E_j / Z_j
  const float e0 = (dx - cx) * (qy - cy) - (dy - cy) * (qx - cx);
  const float e1 = (ax - dx) * (qy - dy) - (ay - dy) * (qx - dx);
  const float e2 = (cx - ax) * (qy - ay) - (cy - ay) * (qx - ax);
  const float p0 = e0 * a.w, p1 = e1 * c.w, p2 = e2 * d.w;
  const float ps = (p0 + p1) + p2;
  const float w0 = p0 / ps, w1 = p1 / ps, w2 = p2 / ps;
  const float4 la = p.vl[vbase + i0], lc = p.vl[vbase + i1], ld = p.vl[vbase + i2];
  const float lx = rr_mix(w0, w1, w2, la.x, lc.x, ld.x), ly = rr_mix(w0, w1, w2, la.y, lc.y, ld.y), lz = rr_mix(w0, w1, w2, la.z, lc.z, ld.z);
  float nx, ny, nz;
  if (p.shading == RR_PHONG) {
    const float4 na = p.vn[vbase + i0], nc = p.vn[vbase + i1], nd = p.vn[vbase + i2];
    nx = rr_mix(w0, w1, w2, na.x, nc.x, nd.x); ny = rr_mix(w0, w1, w2, na.y, nc.y, nd.y); nz = rr_mix(w0, w1, w2, na.z, nc.z, nd.z);
  } else {
    const float4 ea = p.eye[vbase + i0], ec = p.eye[vbase + i1], ed = p.eye[vbase + i2];
    const float ux = ec.x - ea.x, uy = ec.y - ea.y, uz = ec.z - ea.z, vx = ed.x - ea.x, vy = ed.y - ea.y, vz = ed.z - ea.z;
    nx = uy * vz - uz * vy; ny = uz * vx - ux * vz; nz = ux * vy - uy * vx;
    // n . eye_a = det[eye_a eye_c eye_d] has the sign of (screen area) * sign(fx fy): towards the viewer means n . eye < 0
    if ((area > 0.f) == (h[RR_SK] > 0)) { nx = -nx; ny = -ny; nz = -nz; }
  }
  const float ll = sqrtf((lx * lx + ly * ly) + lz * lz), nl = sqrtf((nx * nx + ny * ny) + nz * nz);
  const float dt = ((lx * nx + ly * ny) + lz * nz) / (ll * nl);
  float lw = p.ambient + (dt > 0.f ? dt : 0.f);                        // (NaN from a zero-length vector: no diffuse term)
  if (lw > 1.0f) lw = 1.0f;
  float r = p.surf[0], g = p.surf[1], bl = p.surf[2];
  if (p.colors) {
    const float* __restrict__ ca = p.colors + 3 * (cbase + i0);
    const float* __restrict__ cc = p.colors + 3 * (cbase + i1);
    const float* __restrict__ cd = p.colors + 3 * (cbase + i2);
    r = rr_mix_col(w1, w2, ca[0], cc[0], cd[0]); g = rr_mix_col(w1, w2, ca[1], cc[1], cd[1]); bl = rr_mix_col(w1, w2, ca[2], cc[2], cd[2]);
  }
  out[0] = rr_quant(lw * r); out[1] = rr_quant(lw * g); out[2] = rr_quant(lw * bl);
}

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
  vs_mesh_rows(p.mesh_id, p.v_off, p.f_off, p.M, p.Vmax, b, vfirst, V, ffirst, F, m);
  const int32_t* __restrict__ faces = p.faces + 3 * (size_t)ffirst;
  const size_t vbase = (size_t)b * p.Vmax;
  float best[VS_PPL];
  int face[VS_PPL];
  vs_raster_tile<true>(s_tri, &s_n, p.sv + vbase, faces, F, V, c, best, face);

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
    if (cov) rr_shade(p, h, faces, vbase, (size_t)vfirst, face[k], fx0, fy0, (float)lx, (float)ly, col);
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

int rr_quant_host(double v) {
  if (!(v > 0.0)) return 0;
  const float q = __builtin_rintf(255.0f * (float)v);
  return q >= 255.f ? 255 : (int)q;
}

}  // namespace

extern "C" size_t cp_render_rgb_scratch_bytes(int B, int Vmax) {
  if (B <= 0 || Vmax < 0) return 0;
  return cp_align16_up((size_t)B * RR_HDR * sizeof(int32_t)) + 4 * cp_align16_up((size_t)B * Vmax * sizeof(float4));
}

extern "C" int cp_render_rgb(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                             const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                             const float* colors, const float* normals, const double* surf_color, const double* light_pos,
                             double ambient_weight, const double* bg_color, int shading, int ssaa, int bgr, int H, int W, int B, int Vmax,
                             uint8_t* rgb, float* depth, uint8_t* mask, int32_t* boxes, uint8_t* ok, void* scratch) {
  if (!poses || !cam_K || !verts || !v_offsets || !faces || !f_offsets || !surf_color || !light_pos || !bg_color || !rgb || !ok || !scratch)
    return CP_ERR_INVALID;
  if (B <= 0 || M <= 0 || Vmax <= 0 || H <= 0 || W <= 0 || (k_stride != 0 && k_stride != 9)) return CP_ERR_INVALID;
  if (ssaa != 1 && ssaa != 2 && ssaa != 4) return CP_ERR_INVALID;
  if (ssaa != 1 && (depth || mask || boxes)) return CP_ERR_INVALID;   // depth, mask and boxes belong to the ssaa = 1 sample grid
  if (shading != RR_FLAT && shading != RR_PHONG) return CP_ERR_INVALID;
  if (shading == RR_PHONG && !normals) return CP_ERR_INVALID;
  if (!mesh_ids && M != 1) return CP_ERR_INVALID;
  if (!(ambient_weight == ambient_weight) || __builtin_isinf(ambient_weight)) return CP_ERR_INVALID;
  for (int k = 0; k < 3; ++k)
    if (!__builtin_isfinite(surf_color[k]) || !__builtin_isfinite(light_pos[k]) || !__builtin_isfinite(bg_color[k])) return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || cp_misaligned(cam_K, 7) || cp_misaligned(verts, 3) ||
      cp_misaligned(v_offsets, 3) || cp_misaligned(faces, 3) || cp_misaligned(f_offsets, 3) || cp_misaligned(mesh_ids, 3) ||
      cp_misaligned(colors, 3) || cp_misaligned(normals, 3) || cp_misaligned(depth, 3) || cp_misaligned(boxes, 3))
    return CP_ERR_ALIGN;
  RrParams p = {};
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.verts = verts; p.v_off = v_offsets; p.faces = faces; p.f_off = f_offsets;
  p.M = M; p.mesh_id = mesh_ids; p.colors = colors; p.normals = normals; p.rgb = rgb; p.depth = depth; p.mask = mask; p.boxes = boxes;
  p.ok = ok; p.B = B; p.Vmax = Vmax; p.H = H; p.W = W; p.f = ssaa; p.shading = shading; p.bgr = bgr ? 1 : 0;
  p.ambient = (float)ambient_weight;
  for (int k = 0; k < 3; ++k) { p.surf[k] = (float)surf_color[k]; p.light[k] = (float)light_pos[k]; p.bg[k] = rr_quant_host(bg_color[k]); }
  const long long sw = (long long)ssaa * W, sh = (long long)ssaa * H;
  if (sw >= (1LL << 24) || sh >= (1LL << 24) || (long long)H * W >= (1LL << 31) / 3) return CP_ERR_RANGE;
  VsGrid g;
  if (!vs_grid(W, H, ssaa, false, B, 1, Vmax, g)) return CP_ERR_RANGE;
  p.tx = g.tx; p.ty = g.ty; p.vchunks = g.vchunks;
  char* at = (char*)scratch;
  const size_t rec = cp_align16_up((size_t)B * Vmax * sizeof(float4));
  p.hdr = (int32_t*)at; at += cp_align16_up((size_t)B * RR_HDR * sizeof(int32_t));
  p.sv = (float4*)at; at += rec;
  p.eye = (float4*)at; at += rec;
  p.vl = (float4*)at; at += rec;
  p.vn = (float4*)at;
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(rgb_pose_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(rgb_vertex_kernel, dim3(g.vert_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(rgb_tile_kernel, dim3(g.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(rgb_finish_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}
