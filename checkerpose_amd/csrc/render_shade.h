// The shading half that render_rgb.hip (row N14) and vis_poses.hip (row N18) share, on top of vsd_raster.h's scaffold: the pose and
// vertex records of a shaded render, the shading of one covered sample, and the uint8 quantisation.  The shading rule itself is
// stated at the top of render_rgb.hip.  The .hip files keep their kernels, params structs and entry points.
//
//   RrH, RR_HDR, RR_RT .. RR_SK     the header words of a shaded pose: VsHdr<1> | R t | normal matrix | box | sign(fx fy) | spare
//   rr_quant, rr_quant_host         round-half-even(255 v) of an fp32 colour value, clamped to 0..255
//   rr_pose_record                  a pose kernel's body: P = (K scale)' [R | t], [R | t] and the normal matrix in fp32, validity
//   rr_vertex_record                per vertex, beside the screen record: the eye position, v_L and, for phong, v_normal
//   RrTables, rr_shade              the shaded, quantised colour of one sample on one face.  The colour source is an argument: the
//                                   mesh's texture (row N20: rr_texel, in rr_shade<true> only -- the tile kernels' <true> instantiations), its vertex colours
//                                   (interpolated), or one surface colour when `colors` is null
//   RrTex, RrTexMesh, rr_tex_mesh   the texture tables of a MeshSet and one mesh's view of them;  rr_tex_args: their host-side checks
//   rr_vertex_body, rr_scene_pose_head    the three vertex kernels' body; what vis_pose_kernel and scene_pose_kernel start with
//   rr_shading_args, rr_scratch_bytes, rr_carve     (host) the shading, light and texture arguments checked and filled in; the scratch
//                                   of a shaded call -- a header per pose and the four tables -- sized and carved
//
// Texture rule (row N20; bop_toolkit_lib/renderer_py.py:309-352 add_object + the fragment shaders' texture2D(u_texture, v_texcoord), the
// sampler pinned to the OpenGL specification's "Texture Minification / Magnification" rule, NOT to a driver's output).  Per mesh a
// texture T, uint8 (Ht, Wt, 3) with rows in the image FILE's order (row 0 on top), held as one RGBX word per texel (r | g << 8 |
// b << 16), and UVs fp32 (V, 2) = (texture_u, texture_v).  The reference uploads np.flipud(image) / 255: GL's texel row j is the file's
// row Ht - 1 - j; the table stays in file order and the flip is in the index.  Per covered sample, on the winning face:
//   (u, v) interpolated perspective-correctly with v_color's weights and v_color's expression, a + (w1 (c - a) + w2 (d - a));
//   nearest:  i = clamp(floor(u * Wt), 0, Wt - 1),  j = clamp(floor(v * Ht), 0, Ht - 1),  texel = T[Ht - 1 - j, i];
//   linear, clamp-to-edge:  a = u * Wt - 0.5,  i0 = floor(a),  alpha = a - i0,  i1 = i0 + 1, both clamped to [0, Wt - 1]; the same in
//             v gives j0, j1, beta.  In fp32, per channel, on the BYTES as floats (no fused multiply-add), with t_ij = T[Ht - 1 - j, i]:
//               lo = t_i0j0 + alpha * (t_i1j0 - t_i0j0);   hi = t_i0j1 + alpha * (t_i1j1 - t_i0j1);   texel = lo + beta * (hi - lo)
//             (four equal texels give that texel exactly);
//   colour = light_w * (texel / 255), the quotient a correctly rounded fp32 division; then rr_quant.
// Wrap is clamp-to-edge only, there are no mipmaps, one filter per MeshSet.  The clamps are taken on the floats (NaN -> 0), so every
// index lies inside the mesh's texture whatever the UVs hold.  Priority: a surface colour, then the texture, then the vertex colours,
// then 0.5 grey.  UNPINNED: which filter vispy selects, a driver's fixed-point filtering, OpenGL's own output.
#pragma once
#include "vsd_raster.h"

namespace {

// 4-byte words per pose: VsHdr<1> (P rect bad ok) | RT[12] | NM[12] = N (3x3) c (3) | box xmin ymin xmax ymax | sign(fx fy) | spare
using RrH = VsHdr<1>;
constexpr int RR_HDR = 48;
constexpr int RR_RT = RrH::USER, RR_NM = RR_RT + 12, RR_BOX = RR_NM + 12, RR_SK = RR_BOX + 4;
enum { RR_FLAT = 0, RR_PHONG = 1 };
enum { RR_NEAREST = 0, RR_LINEAR = 1 };
constexpr int RR_TEX_SIDE = 16384;               // the largest side of a texture

// round-half-even(255 v) of an fp32 colour value, clamped to 0..255 (NaN -> 0)
__device__ __forceinline__ int rr_quant(float v) {
#pragma clang fp contract(off)
  const float q = rintf(255.0f * v);
  return q >= 255.f ? 255 : (q > 0.f ? (int)q : 0);
}

inline int rr_quant_host(double v) {
  if (!(v > 0.0)) return 0;
  const float q = __builtin_rintf(255.0f * (float)v);
  return q >= 255.f ? 255 : (int)q;
}

// The header h of one pose q (12 doubles) under K (9 doubles) scaled by `scale`; mesh_ok: vs_mesh_rows' verdict (and whatever else
// the caller checked).  Everything but the accumulators' meaning is here: the box starts empty.
__device__ inline void rr_pose_record(const double* __restrict__ K, const double* __restrict__ q, double scale, bool mesh_ok,
                                      int32_t* __restrict__ h) {
#pragma clang fp contract(off)
  bool ok = mesh_ok && vs_pose_finite(K, q);
  vs_side_init(K, scale, q, (float*)h + RrH::P(0), h + RrH::RECT(0));      // P = (K f)' [R | t]
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

// the per-vertex tables of a shaded render, (poses, Vmax) float4 each, and what the shading needs beside them
struct RrTables {
  float4* sv;                 // screen records
  float4* eye;
  float4* vl;
  float4* vn;                 // phong
  float light[3], ambient;
  int shading;
};

// besides the screen record: the eye position, v_L and, for phong, v_normal of vertex vt (its normal: nr) -> row `at` of the tables
__device__ __forceinline__ void rr_vertex_record(const RrTables& T, const int32_t* __restrict__ h, size_t at, const float* __restrict__ vt,
                                                 const float* __restrict__ nr) {
#pragma clang fp contract(off)
  const float* __restrict__ rt = (const float*)(h + RR_RT);
  const float ex = vs_affine(rt, vt[0], vt[1], vt[2]), ey = vs_affine(rt + 4, vt[0], vt[1], vt[2]), ez = vs_affine(rt + 8, vt[0], vt[1], vt[2]);
  T.eye[at] = make_float4(ex, ey, ez, 0.f);
  const float lx = T.light[0] - ex, ly = T.light[1] - ey, lz = T.light[2] - ez;
  const float ll = sqrtf((lx * lx + ly * ly) + lz * lz);
  T.vl[at] = make_float4(lx / ll, ly / ll, lz / ll, 0.f);
  if (T.shading == RR_PHONG) {
    const float* __restrict__ nm = (const float*)(h + RR_NM);
    const float nx = fmaf(nm[2], nr[2], fmaf(nm[1], nr[1], nm[0] * nr[0]));
    const float ny = fmaf(nm[5], nr[2], fmaf(nm[4], nr[1], nm[3] * nr[0]));
    const float nz = fmaf(nm[8], nr[2], fmaf(nm[7], nr[1], nm[6] * nr[0]));
    const float nw = 1.0f - fmaf(nm[11], nr[2], fmaf(nm[10], nr[1], nm[9] * nr[0]));
    const float nl = sqrtf(((nx * nx + ny * ny) + nz * nz) + nw * nw);    // the shader's 4-vector length
    T.vn[at] = make_float4(nx / nl, ny / nl, nz / nl, 0.f);
  }
}

// The body of the three shaded vertex kernels (p: RrParams, VpParams or SlParams), for ALL threads of the workgroup: the screen record
// and the rectangle (vs_vertex_chunk, the sample's pixels clamped to `clip`) and the shading records, under the pose's header of
// hdr_words words.
template <typename Params>
__device__ __forceinline__ void rr_vertex_body(const Params& p, int hdr_words, float4 clip) {
  int b, s, vc;
  vs_vertex_block(p.vchunks, 1, b, s, vc);
  int32_t* __restrict__ h = p.hdr + (size_t)b * hdr_words;
  if (!h[RrH::OK]) return;                                           // (uniform; no barrier in this kernel)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  const auto shading_records = [&](int i, const float* __restrict__ vt) {
    rr_vertex_record(p.T, h, (size_t)b * p.mesh.Vmax + i, vt, p.normals ? p.normals + 3 * ((size_t)vfirst + i) : nullptr);
  };
  vs_vertex_chunk((const float*)h + RrH::P(0), p.mesh.verts + 3 * (size_t)vfirst, V, vc, clip, p.T.sv + (size_t)b * p.mesh.Vmax,
                  h + RrH::RECT(0), h + RrH::BAD(0), shading_records);
}

// What the pose kernels of an image's poses (p: VpParams or SlParams) start with: pose b's mesh rows, its image (img; false: no such
// image), its surface colour finite, and the header h under the IMAGE's K.
template <typename Params>
__device__ __forceinline__ bool rr_scene_pose_head(const Params& p, int b, int32_t* __restrict__ h, int& img) {
  int vfirst, V, ffirst, F, m;
  bool ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  img = p.image_of_pose[b];
  const bool img_ok = img >= 0 && img < p.I;
  ok = ok && img_ok;
  if (p.surf) ok = ok && vs_finite(p.surf + 3 * (size_t)b, 3);
  rr_pose_record(p.K + (size_t)p.k_stride * (img_ok ? img : 0), p.poses + 12 * (size_t)b, 1.0, ok, h);
  return img_ok;
}

// the texture tables of a MeshSet (all null without textures) and one mesh's view of them
struct RrTex {
  const float* uv;            // (sumV, 2), rows as verts
  const uint32_t* texels;     // (sum Wt Ht) RGBX words, file row order
  const int32_t* off;         // (M + 1) texel offsets
  const int32_t* dims;        // (M, 2) = Wt, Ht; 0 0: the mesh has no texture
  int filter;
};
struct RrTexMesh {
  const float* uv;            // the mesh's first row
  const uint32_t* tex;        // the mesh's first texel
  int Wt, Ht, filter;         // Wt == 0: no texture
};

// mesh m's (first vertex row vfirst) view; `use` false (a surface colour overrides the texture) or no tables: Wt == 0
__device__ __forceinline__ RrTexMesh rr_tex_mesh(const RrTex& X, int m, size_t vfirst, bool use) {
  RrTexMesh t = {nullptr, nullptr, 0, 0, X.filter};
  if (!use || !X.texels) return t;
  const int Wt = X.dims[2 * m], Ht = X.dims[2 * m + 1];
  if (Wt <= 0 || Ht <= 0 || Wt > RR_TEX_SIDE || Ht > RR_TEX_SIDE || X.off[m] < 0) return t;
  t.uv = X.uv + 2 * vfirst; t.tex = X.texels + (size_t)X.off[m]; t.Wt = Wt; t.Ht = Ht;
  return t;
}

// the host-side checks of the texture arguments of the three _tex entry points: all four tables or none, a known filter
inline int rr_tex_args(const float* uv, const uint32_t* texels, const int32_t* tex_off, const int32_t* tex_dims, int filter) {
  if (filter != RR_NEAREST && filter != RR_LINEAR) return CP_ERR_INVALID;
  const int given = (uv ? 1 : 0) + (texels ? 1 : 0) + (tex_off ? 1 : 0) + (tex_dims ? 1 : 0);
  if (given != 0 && given != 4) return CP_ERR_INVALID;
  if (cp_misaligned(uv, 3) || cp_misaligned(texels, 3) || cp_misaligned(tex_off, 3) || cp_misaligned(tex_dims, 3)) return CP_ERR_ALIGN;
  return CP_OK;
}

// The host-side checks of a shaded call's shading, light and texture arguments, which they fill into T and X: a known shading, normals
// for phong, a finite ambient weight, rr_tex_args (its own code: the one ALIGN among an entry point's INVALID rules), a finite light.
inline int rr_shading_args(int shading, const float* normals, double ambient_weight, const double* light_pos, const float* uv,
                           const uint32_t* texels, const int32_t* tex_off, const int32_t* tex_dims, int filter, RrTables& T, RrTex& X) {
  if (!light_pos || (shading != RR_FLAT && shading != RR_PHONG) || (shading == RR_PHONG && !normals) || !__builtin_isfinite(ambient_weight))
    return CP_ERR_INVALID;
  if (const int e = rr_tex_args(uv, texels, tex_off, tex_dims, filter)) return e;
  for (int k = 0; k < 3; ++k)
    if (!__builtin_isfinite(light_pos[k])) return CP_ERR_INVALID;
  T.shading = shading; T.ambient = (float)ambient_weight;
  for (int k = 0; k < 3; ++k) T.light[k] = (float)light_pos[k];
  X.uv = uv; X.texels = texels; X.off = tex_off; X.dims = tex_dims; X.filter = filter;
  return CP_OK;
}
// a[0 .. 3) are finite (a colour of an entry point's own)
inline bool rr_finite3(const double* a) { return __builtin_isfinite(a[0]) && __builtin_isfinite(a[1]) && __builtin_isfinite(a[2]); }

// the scratch of a shaded call over n poses: n headers of hdr_words words, then the four (n, Vmax) tables
inline size_t rr_scratch_bytes(int n, int Vmax, int hdr_words) {
  return cp_align16_up((size_t)n * hdr_words * sizeof(int32_t)) + 4 * cp_align16_up((size_t)n * Vmax * sizeof(float4));
}
inline void rr_carve(void* scratch, int n, int Vmax, int hdr_words, int32_t*& hdr, RrTables& T) {
  char* at = (char*)scratch;
  const size_t rec = cp_align16_up((size_t)n * Vmax * sizeof(float4));
  hdr = (int32_t*)at; at += cp_align16_up((size_t)n * hdr_words * sizeof(int32_t));
  T.sv = (float4*)at; at += rec;
  T.eye = (float4*)at; at += rec;
  T.vl = (float4*)at; at += rec;
  T.vn = (float4*)at;
}

// The tile launch of a shaded call: the kernel's <true> instantiation when the call has texture tables, else its <false> one -- the
// code the rows N14 / N18 / N19 always had (no texture code in it: the same registers, LDS and output bits; the params structs' layout
// only moves the argument loads) -- recorded under the plain name the launch lists always showed.
#define RR_LAUNCH_TILE(kernel, textured, ...)                                                          \
  do {                                                                                                 \
    if (textured) { cp_mark_kernel("%s", #kernel "<true>"); hipLaunchKernelGGL(kernel<true>, __VA_ARGS__); } \
    else { cp_mark_kernel("%s", #kernel); hipLaunchKernelGGL(kernel<false>, __VA_ARGS__); }            \
  } while (0)

// an index of a texture axis of n texels from its float position: clamped to [0, n - 1] on the float (NaN -> 0)
__device__ __forceinline__ int rr_tex_index(float f, int n) { return (int)fminf(fmaxf(f, 0.f), (float)(n - 1)); }

// the texel of mesh texture t at (u, v) by the rule at the top of this file, as bytes in float (0..255), per channel
__device__ __forceinline__ void rr_texel(const RrTexMesh& t, float u, float v, float (&rgb)[3]) {
#pragma clang fp contract(off)
  const float su = u * (float)t.Wt, sv = v * (float)t.Ht;
  if (t.filter == RR_NEAREST) {                                        // (uniform)
    const int i = rr_tex_index(floorf(su), t.Wt), j = rr_tex_index(floorf(sv), t.Ht);
    const uint32_t w = t.tex[(size_t)(t.Ht - 1 - j) * t.Wt + i];
    rgb[0] = (float)(w & 255u); rgb[1] = (float)((w >> 8) & 255u); rgb[2] = (float)((w >> 16) & 255u);
    return;
  }
  const float a = su - 0.5f, b = sv - 0.5f;
  const float fa = floorf(a), fb = floorf(b);
  const float alpha = a - fa, beta = b - fb;
  const int i0 = rr_tex_index(fa, t.Wt), i1 = rr_tex_index(fa + 1.0f, t.Wt);
  const int j0 = rr_tex_index(fb, t.Ht), j1 = rr_tex_index(fb + 1.0f, t.Ht);
  const size_t r0 = (size_t)(t.Ht - 1 - j0) * t.Wt, r1 = (size_t)(t.Ht - 1 - j1) * t.Wt;
  const uint32_t w00 = t.tex[r0 + i0], w10 = t.tex[r0 + i1], w01 = t.tex[r1 + i0], w11 = t.tex[r1 + i1];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t00 = (float)((w00 >> (8 * c)) & 255u), t10 = (float)((w10 >> (8 * c)) & 255u);
    const float t01 = (float)((w01 >> (8 * c)) & 255u), t11 = (float)((w11 >> (8 * c)) & 255u);
    const float lo = t00 + alpha * (t10 - t00), hi = t01 + alpha * (t11 - t01);
    rgb[c] = lo + beta * (hi - lo);
  }
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

// the shaded, quantised colour of the sample (qx, qy) (tile-relative indices) on face fidx; the colour is the texture `tm` (TEX and
// tm.Wt > 0: uniform over the caller's workgroup), else `colors` (rows from cbase, interpolated) or, with colors == nullptr, the one
// colour `surf`.  rr_shade<false> is the code the rows N14 / N18 / N19 always had.
template <bool TEX>
__device__ __forceinline__ void rr_shade(const RrTables& T, const float* __restrict__ colors, const float (&surf)[3], const RrTexMesh& tm,
                                         const int32_t* __restrict__ h, const int32_t* __restrict__ faces, size_t vbase, size_t cbase,
                                         int fidx, float fx0, float fy0, float qx, float qy, int (&out)[3]) {
#pragma clang fp contract(off)
  const int32_t* __restrict__ fi = faces + 3 * (size_t)fidx;
  const int i0 = fi[0], i1 = fi[1], i2 = fi[2];
  const float4 a = T.sv[vbase + i0], c = T.sv[vbase + i1], d = T.sv[vbase + i2];
  const float ax = a.x - fx0, ay = a.y - fy0, cx = c.x - fx0, cy = c.y - fy0, dx = d.x - fx0, dy = d.y - fy0;
  const float area = (cx - ax) * (dy - ay) - (dx - ax) * (cy - ay);   // (the walk's expression: the same bits, never 0 here)
  // edge i is opposite vertex i, differences first; perspective-correct weights w_i = E_i / Z_i / sum_j E_j / Z_j
  const float e0 = (dx - cx) * (qy - cy) - (dy - cy) * (qx - cx);
  const float e1 = (ax - dx) * (qy - dy) - (ay - dy) * (qx - dx);
  const float e2 = (cx - ax) * (qy - ay) - (cy - ay) * (qx - ax);
  const float p0 = e0 * a.w, p1 = e1 * c.w, p2 = e2 * d.w;
  const float ps = (p0 + p1) + p2;
  const float w0 = p0 / ps, w1 = p1 / ps, w2 = p2 / ps;
  float tx[3] = {0.f, 0.f, 0.f};
  if (TEX && tm.Wt > 0) {                                              // (the texel first: three values live through the lighting)
    const float* __restrict__ ua = tm.uv + 2 * (size_t)i0;
    const float* __restrict__ uc = tm.uv + 2 * (size_t)i1;
    const float* __restrict__ ud = tm.uv + 2 * (size_t)i2;
    rr_texel(tm, rr_mix_col(w1, w2, ua[0], uc[0], ud[0]), rr_mix_col(w1, w2, ua[1], uc[1], ud[1]), tx);
  }
  const float4 la = T.vl[vbase + i0], lc = T.vl[vbase + i1], ld = T.vl[vbase + i2];
  const float lx = rr_mix(w0, w1, w2, la.x, lc.x, ld.x), ly = rr_mix(w0, w1, w2, la.y, lc.y, ld.y), lz = rr_mix(w0, w1, w2, la.z, lc.z, ld.z);
  float nx, ny, nz;
  if (T.shading == RR_PHONG) {
    const float4 na = T.vn[vbase + i0], nc = T.vn[vbase + i1], nd = T.vn[vbase + i2];
    nx = rr_mix(w0, w1, w2, na.x, nc.x, nd.x); ny = rr_mix(w0, w1, w2, na.y, nc.y, nd.y); nz = rr_mix(w0, w1, w2, na.z, nc.z, nd.z);
  } else {
    const float4 ea = T.eye[vbase + i0], ec = T.eye[vbase + i1], ed = T.eye[vbase + i2];
    const float ux = ec.x - ea.x, uy = ec.y - ea.y, uz = ec.z - ea.z, vx = ed.x - ea.x, vy = ed.y - ea.y, vz = ed.z - ea.z;
    nx = uy * vz - uz * vy; ny = uz * vx - ux * vz; nz = ux * vy - uy * vx;
    // n . eye_a = det[eye_a eye_c eye_d] has the sign of (screen area) * sign(fx fy): towards the viewer means n . eye < 0
    if ((area > 0.f) == (h[RR_SK] > 0)) { nx = -nx; ny = -ny; nz = -nz; }
  }
  const float ll = sqrtf((lx * lx + ly * ly) + lz * lz), nl = sqrtf((nx * nx + ny * ny) + nz * nz);
  const float dt = ((lx * nx + ly * ny) + lz * nz) / (ll * nl);
  float lw = T.ambient + (dt > 0.f ? dt : 0.f);                        // (NaN from a zero-length vector: no diffuse term)
  if (lw > 1.0f) lw = 1.0f;
  float r = surf[0], g = surf[1], bl = surf[2];
  if (TEX && tm.Wt > 0) {
    r = tx[0] / 255.0f; g = tx[1] / 255.0f; bl = tx[2] / 255.0f;
  } else if (colors) {
    const float* __restrict__ ca = colors + 3 * (cbase + i0);
    const float* __restrict__ cc = colors + 3 * (cbase + i1);
    const float* __restrict__ cd = colors + 3 * (cbase + i2);
    r = rr_mix_col(w1, w2, ca[0], cc[0], cd[0]); g = rr_mix_col(w1, w2, ca[1], cc[1], cd[1]); bl = rr_mix_col(w1, w2, ca[2], cc[2], cd[2]);
  }
  out[0] = rr_quant(lw * r); out[1] = rr_quant(lw * g); out[2] = rr_quant(lw * bl);
}

}  // namespace
