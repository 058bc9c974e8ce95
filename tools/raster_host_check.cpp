// The host halves of the raster family's entry points that have no check of their own -- cp_render_depth, cp_vsd_errors,
// cp_vsd_from_depth (csrc/vsd_error.hip), cp_gt_info, cp_gt_info_from_depth (csrc/gt_info.hip), cp_mask_errors (csrc/mask_error.hip) and
// the untextured cp_render_rgb (csrc/render_rgb.hip) -- swept field by field: every pointer that must not be null, every scalar rule, one
// misaligned pointer per alignment class, every size rule, every scratch size, and the order of the error classes (INVALID before ALIGN
// before RANGE) when a call breaks two rules at once.  A stand-alone program, so that it can be built under AddressSanitizer +
// UndefinedBehaviorSanitizer (`make -C checkerpose_amd/csrc raster_host_check`, then run checkerpose_amd/csrc/raster_host_check).
// Every call below is refused before any launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal
// and every size as expected.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../include/checkerpose_hip.h"

static int failures = 0;
#define EXPECT(what, want)                                                                          \
  do {                                                                                              \
    const long long got_ = (long long)(what);                                                       \
    if (got_ != (long long)(want)) { printf("FAIL %s line %d: %lld, expected %lld\n", #what, __LINE__, got_, (long long)(want)); ++failures; } \
  } while (0)
// inside a block that names its arguments `good`, a scratch copy `a` and the entry point `call`
#define NULLED(field) a = good; a.field = nullptr; EXPECT(call(a), CP_ERR_INVALID)
#define WITH(field, value, want) a = good; a.field = value; EXPECT(call(a), want)
#define WITH2(f1, v1, f2, v2, want) a = good; a.f1 = v1; a.f2 = v2; EXPECT(call(a), want)

alignas(16) static unsigned char buf[256];        // stands for every device pointer: never dereferenced by a refused call
static float* const f = (float*)buf;
static int32_t* const i32 = (int32_t*)buf;
static double* const d = (double*)buf;
static uint8_t* const u8 = buf;
static float* const f_odd = (float*)(buf + 2);              // off a 4-byte boundary
static int32_t* const i_odd = (int32_t*)(buf + 2);
static double* const d_odd = (double*)(buf + 4);            // off an 8-byte boundary
static const double vec[3] = {0.3, 0.3, 0.3}, bad_vec[3] = {0.3, NAN, 0.3}, taus[3] = {0.05, 0.1, 0.15};
// square frames at each file's own pixel bound, every side below 2^24 and every tile grid below 2^24 workgroups:
// 46341^2 >= 2^31 > 46340^2;  26755^2 >= 2^31 / 3 > 26754^2;  15447^2 >= 2^31 / 9 > 15446^2
static const int SIDE_31 = 46341, SIDE_31_3 = 26755, SIDE_31_9 = 15447;

struct Depth {      // cp_render_depth
  const double* poses; const double* K; int k_stride; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off;
  int M; const int32_t* mesh_ids; int H, W, B, Vmax; float* depth_out; void* scratch;
};
static void check_render_depth() {
  const auto call = [](const Depth& a) {
    return cp_render_depth(nullptr, a.poses, a.K, a.k_stride, a.verts, a.v_off, a.faces, a.f_off, a.M, a.mesh_ids, a.H, a.W, a.B, a.Vmax,
                           a.depth_out, a.scratch);
  };
  const Depth good = {d, d, 9, f, i32, i32, i32, 2, i32, 40, 48, 5, 12, f, buf};
  Depth a;
  NULLED(poses); NULLED(K); NULLED(verts); NULLED(v_off); NULLED(faces); NULLED(f_off); NULLED(depth_out); NULLED(scratch);
  NULLED(mesh_ids);                                // M == 2
  WITH(B, 0, CP_ERR_INVALID); WITH(M, 0, CP_ERR_INVALID); WITH(Vmax, 0, CP_ERR_INVALID); WITH(H, 0, CP_ERR_INVALID);
  WITH(W, -3, CP_ERR_INVALID); WITH(k_stride, 3, CP_ERR_INVALID);
  WITH(scratch, buf + 8, CP_ERR_ALIGN); WITH(poses, d_odd, CP_ERR_ALIGN); WITH(K, d_odd, CP_ERR_ALIGN); WITH(verts, f_odd, CP_ERR_ALIGN);
  WITH(v_off, i_odd, CP_ERR_ALIGN); WITH(faces, i_odd, CP_ERR_ALIGN); WITH(f_off, i_odd, CP_ERR_ALIGN); WITH(mesh_ids, i_odd, CP_ERR_ALIGN);
  WITH(depth_out, f_odd, CP_ERR_ALIGN);
  WITH2(H, SIDE_31, W, SIDE_31, CP_ERR_RANGE);
  WITH(W, 1 << 29, CP_ERR_RANGE);                  // 2^24 tiles in a row
  WITH2(B, 1 << 20, Vmax, 1 << 13, CP_ERR_RANGE);  // 2^20 poses of 32 vertex chunks each
  WITH2(poses, nullptr, verts, f_odd, CP_ERR_INVALID);
  a = good; a.K = d_odd; a.H = SIDE_31; a.W = SIDE_31; EXPECT(call(a), CP_ERR_ALIGN);
}

struct Vsd {        // cp_vsd_errors
  const double* est; const double* gt; const double* K; int k_stride; const float* verts; const int32_t* v_off; const int32_t* faces;
  const int32_t* f_off; int M; const int32_t* mesh_ids; const float* depth_test; const int32_t* image_ids; int I, H, W; double delta;
  const double* diameters; const double* taus; int T, normalise, sphere, B, Vmax; double* errors; int32_t* counts; float* depth_out;
  void* scratch;
};
static void check_vsd_errors() {
  const auto call = [](const Vsd& a) {
    return cp_vsd_errors(nullptr, a.est, a.gt, a.K, a.k_stride, a.verts, a.v_off, a.faces, a.f_off, a.M, a.mesh_ids, a.depth_test, a.image_ids,
                         a.I, a.H, a.W, a.delta, a.diameters, a.taus, a.T, a.normalise, a.sphere, a.B, a.Vmax, a.errors, a.counts, a.depth_out,
                         a.scratch);
  };
  const Vsd good = {d, d, d, 0, f, i32, i32, i32, 2, i32, f, i32, 2, 40, 48, 15.0, d, taus, 3, 1, 1, 5, 12, d, i32, f, buf};
  Vsd a;
  NULLED(est); NULLED(gt); NULLED(K); NULLED(verts); NULLED(v_off); NULLED(faces); NULLED(f_off); NULLED(depth_test); NULLED(diameters);
  NULLED(taus); NULLED(errors); NULLED(counts); NULLED(scratch);
  NULLED(mesh_ids);                                // M == 2
  NULLED(image_ids);                               // I == 2
  WITH(B, 0, CP_ERR_INVALID); WITH(M, 0, CP_ERR_INVALID); WITH(Vmax, 0, CP_ERR_INVALID); WITH(I, 0, CP_ERR_INVALID);
  WITH(H, 0, CP_ERR_INVALID); WITH(W, -3, CP_ERR_INVALID); WITH(T, 0, CP_ERR_INVALID); WITH(T, 17, CP_ERR_INVALID);
  WITH(k_stride, 3, CP_ERR_INVALID); WITH(delta, NAN, CP_ERR_INVALID);
  WITH(scratch, buf + 8, CP_ERR_ALIGN); WITH(est, d_odd, CP_ERR_ALIGN); WITH(gt, d_odd, CP_ERR_ALIGN); WITH(K, d_odd, CP_ERR_ALIGN);
  WITH(diameters, d_odd, CP_ERR_ALIGN); WITH(errors, d_odd, CP_ERR_ALIGN); WITH(verts, f_odd, CP_ERR_ALIGN); WITH(v_off, i_odd, CP_ERR_ALIGN);
  WITH(faces, i_odd, CP_ERR_ALIGN); WITH(f_off, i_odd, CP_ERR_ALIGN); WITH(mesh_ids, i_odd, CP_ERR_ALIGN);
  WITH(depth_test, f_odd, CP_ERR_ALIGN); WITH(image_ids, i_odd, CP_ERR_ALIGN); WITH(counts, i_odd, CP_ERR_ALIGN);
  WITH(depth_out, f_odd, CP_ERR_ALIGN);
  WITH2(H, SIDE_31, W, SIDE_31, CP_ERR_RANGE);
  WITH2(B, 1 << 20, Vmax, 1 << 13, CP_ERR_RANGE);  // 2^20 pairs of 2 x 32 vertex chunks each
  WITH2(errors, nullptr, K, d_odd, CP_ERR_INVALID);
  a = good; a.counts = i_odd; a.H = SIDE_31; a.W = SIDE_31; EXPECT(call(a), CP_ERR_ALIGN);
  // scratch: B headers of 40 words, (B, 2, Vmax) float4, 18 words per (pose, tile); the first and the last part rounded up to 16 bytes
  EXPECT(cp_vsd_errors_scratch_bytes(5, 12, 40, 48), 800 + 1920 + 1440);
  EXPECT(cp_vsd_errors_scratch_bytes(3, 7, 33, 31), 480 + 672 + 432);
  EXPECT(cp_vsd_errors_scratch_bytes(3, 0, 40, 48), 480 + 864);                  // cp_vsd_from_depth's: no vertices
  EXPECT(cp_vsd_errors_scratch_bytes(0, 12, 40, 48), 0); EXPECT(cp_vsd_errors_scratch_bytes(5, -1, 40, 48), 0);
  EXPECT(cp_vsd_errors_scratch_bytes(5, 12, 0, 48), 0); EXPECT(cp_vsd_errors_scratch_bytes(5, 12, 40, 0), 0);
}

struct VsdDepth {   // cp_vsd_from_depth
  const float* est; const float* gt; const double* K; int k_stride; const float* depth_test; const int32_t* image_ids; int I, H, W;
  double delta; const double* diameters; const double* taus; int T, normalise, B; double* errors; int32_t* counts; void* scratch;
};
static void check_vsd_from_depth() {
  const auto call = [](const VsdDepth& a) {
    return cp_vsd_from_depth(nullptr, a.est, a.gt, a.K, a.k_stride, a.depth_test, a.image_ids, a.I, a.H, a.W, a.delta, a.diameters, a.taus, a.T,
                             a.normalise, a.B, a.errors, a.counts, a.scratch);
  };
  const VsdDepth good = {f, f, d, 9, f, i32, 2, 40, 48, 15.0, d, taus, 3, 1, 5, d, i32, buf};
  VsdDepth a;
  NULLED(est); NULLED(gt); NULLED(K); NULLED(depth_test); NULLED(diameters); NULLED(taus); NULLED(errors); NULLED(counts); NULLED(scratch);
  NULLED(image_ids);                               // I == 2
  WITH(B, 0, CP_ERR_INVALID); WITH(I, 0, CP_ERR_INVALID); WITH(H, 0, CP_ERR_INVALID); WITH(W, -3, CP_ERR_INVALID);
  WITH(T, 0, CP_ERR_INVALID); WITH(T, 17, CP_ERR_INVALID); WITH(k_stride, 3, CP_ERR_INVALID); WITH(delta, NAN, CP_ERR_INVALID);
  WITH(scratch, buf + 8, CP_ERR_ALIGN); WITH(K, d_odd, CP_ERR_ALIGN); WITH(diameters, d_odd, CP_ERR_ALIGN); WITH(errors, d_odd, CP_ERR_ALIGN);
  WITH(est, f_odd, CP_ERR_ALIGN); WITH(gt, f_odd, CP_ERR_ALIGN); WITH(depth_test, f_odd, CP_ERR_ALIGN); WITH(image_ids, i_odd, CP_ERR_ALIGN);
  WITH(counts, i_odd, CP_ERR_ALIGN);
  WITH2(H, SIDE_31, W, SIDE_31, CP_ERR_RANGE);
  WITH(B, 1 << 22, CP_ERR_RANGE);                  // 2^22 pairs of 4 tiles each
  WITH2(counts, nullptr, est, f_odd, CP_ERR_INVALID);
  a = good; a.errors = d_odd; a.H = SIDE_31; a.W = SIDE_31; EXPECT(call(a), CP_ERR_ALIGN);
}

struct Gi {         // cp_gt_info
  const double* poses; const double* K; int k_stride; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off;
  int M; const int32_t* mesh_ids; const float* depth; const int32_t* image_ids; int I, H, W; double delta; int B, Vmax; int32_t* counts;
  double* fract; int32_t* boxes; uint8_t* ok; uint8_t* mask; uint8_t* mask_visib; float* depth_gt; void* scratch;
};
static void check_gt_info() {
  const auto call = [](const Gi& a) {
    return cp_gt_info(nullptr, a.poses, a.K, a.k_stride, a.verts, a.v_off, a.faces, a.f_off, a.M, a.mesh_ids, a.depth, a.image_ids, a.I, a.H,
                      a.W, a.delta, a.B, a.Vmax, a.counts, a.fract, a.boxes, a.ok, a.mask, a.mask_visib, a.depth_gt, a.scratch);
  };
  const Gi good = {d, d, 0, f, i32, i32, i32, 2, i32, f, i32, 2, 40, 48, 15.0, 5, 12, i32, d, i32, u8, u8, u8, f, buf};
  Gi a;
  NULLED(poses); NULLED(K); NULLED(verts); NULLED(v_off); NULLED(faces); NULLED(f_off); NULLED(depth); NULLED(counts); NULLED(fract);
  NULLED(boxes); NULLED(ok); NULLED(scratch);
  NULLED(mesh_ids);                                // M == 2
  NULLED(image_ids);                               // I == 2
  NULLED(mask); NULLED(mask_visib);                // both or neither
  WITH(B, 0, CP_ERR_INVALID); WITH(M, 0, CP_ERR_INVALID); WITH(Vmax, 0, CP_ERR_INVALID); WITH(I, 0, CP_ERR_INVALID);
  WITH(H, 0, CP_ERR_INVALID); WITH(W, -3, CP_ERR_INVALID); WITH(k_stride, 3, CP_ERR_INVALID); WITH(delta, NAN, CP_ERR_INVALID);
  WITH(scratch, buf + 8, CP_ERR_ALIGN); WITH(poses, d_odd, CP_ERR_ALIGN); WITH(K, d_odd, CP_ERR_ALIGN); WITH(fract, d_odd, CP_ERR_ALIGN);
  WITH(verts, f_odd, CP_ERR_ALIGN); WITH(v_off, i_odd, CP_ERR_ALIGN); WITH(faces, i_odd, CP_ERR_ALIGN); WITH(f_off, i_odd, CP_ERR_ALIGN);
  WITH(mesh_ids, i_odd, CP_ERR_ALIGN); WITH(depth, f_odd, CP_ERR_ALIGN); WITH(image_ids, i_odd, CP_ERR_ALIGN);
  WITH(counts, i_odd, CP_ERR_ALIGN); WITH(boxes, i_odd, CP_ERR_ALIGN); WITH(depth_gt, f_odd, CP_ERR_ALIGN);
  WITH2(H, SIDE_31_9, W, SIDE_31_9, CP_ERR_RANGE);
  WITH2(B, 1 << 20, Vmax, 1 << 13, CP_ERR_RANGE);  // 2^20 poses of 32 vertex chunks each
  WITH2(ok, nullptr, fract, d_odd, CP_ERR_INVALID);
  a = good; a.depth = f_odd; a.H = SIDE_31_9; a.W = SIDE_31_9; EXPECT(call(a), CP_ERR_ALIGN);
  // scratch: B headers of 32 words, (B, Vmax) float4, each part rounded up to 16 bytes
  EXPECT(cp_gt_info_scratch_bytes(5, 12), 640 + 960); EXPECT(cp_gt_info_scratch_bytes(3, 7), 384 + 336);
  EXPECT(cp_gt_info_scratch_bytes(3, 0), 384);     // cp_gt_info_from_depth's: no vertices
  EXPECT(cp_gt_info_scratch_bytes(0, 12), 0); EXPECT(cp_gt_info_scratch_bytes(5, -1), 0);
}

struct GiDepth {    // cp_gt_info_from_depth
  const float* large; const double* K; int k_stride; const float* depth; const int32_t* image_ids; int I, H, W; double delta; int B;
  int32_t* counts; double* fract; int32_t* boxes; uint8_t* ok; uint8_t* mask; uint8_t* mask_visib; void* scratch;
};
static void check_gt_info_from_depth() {
  const auto call = [](const GiDepth& a) {
    return cp_gt_info_from_depth(nullptr, a.large, a.K, a.k_stride, a.depth, a.image_ids, a.I, a.H, a.W, a.delta, a.B, a.counts, a.fract,
                                 a.boxes, a.ok, a.mask, a.mask_visib, a.scratch);
  };
  const GiDepth good = {f, d, 9, f, i32, 2, 40, 48, 15.0, 5, i32, d, i32, u8, u8, u8, buf};
  GiDepth a;
  NULLED(large); NULLED(K); NULLED(depth); NULLED(counts); NULLED(fract); NULLED(boxes); NULLED(ok); NULLED(scratch);
  NULLED(image_ids);                               // I == 2
  NULLED(mask); NULLED(mask_visib);                // both or neither
  WITH(B, 0, CP_ERR_INVALID); WITH(I, 0, CP_ERR_INVALID); WITH(H, 0, CP_ERR_INVALID); WITH(W, -3, CP_ERR_INVALID);
  WITH(k_stride, 3, CP_ERR_INVALID); WITH(delta, NAN, CP_ERR_INVALID);
  WITH(scratch, buf + 8, CP_ERR_ALIGN); WITH(K, d_odd, CP_ERR_ALIGN); WITH(fract, d_odd, CP_ERR_ALIGN); WITH(large, f_odd, CP_ERR_ALIGN);
  WITH(depth, f_odd, CP_ERR_ALIGN); WITH(image_ids, i_odd, CP_ERR_ALIGN); WITH(counts, i_odd, CP_ERR_ALIGN); WITH(boxes, i_odd, CP_ERR_ALIGN);
  WITH2(H, SIDE_31_9, W, SIDE_31_9, CP_ERR_RANGE);
  WITH(B, 1 << 20, CP_ERR_RANGE);                  // 2^20 poses of 5 x 5 canvas tiles each
  WITH2(large, nullptr, boxes, i_odd, CP_ERR_INVALID);
  a = good; a.scratch = buf + 8; a.H = SIDE_31_9; a.W = SIDE_31_9; EXPECT(call(a), CP_ERR_ALIGN);
}

struct Me {         // cp_mask_errors
  const double* est; const double* gt; const double* K; int k_stride; const float* verts; const int32_t* v_off; const int32_t* faces;
  const int32_t* f_off; int M; const int32_t* mesh_ids; const double* diameters; int H, W, sphere, B, Vmax; double* cus; double* bbp;
  int32_t* counts; int32_t* boxes; uint8_t* ok; uint8_t* masks; void* scratch;
};
static void check_mask_errors() {
  const auto call = [](const Me& a) {
    return cp_mask_errors(nullptr, a.est, a.gt, a.K, a.k_stride, a.verts, a.v_off, a.faces, a.f_off, a.M, a.mesh_ids, a.diameters, a.H, a.W,
                          a.sphere, a.B, a.Vmax, a.cus, a.bbp, a.counts, a.boxes, a.ok, a.masks, a.scratch);
  };
  const Me good = {d, d, d, 0, f, i32, i32, i32, 2, i32, d, 40, 48, 1, 5, 12, d, d, i32, i32, u8, u8, buf};
  Me a;
  NULLED(est); NULLED(gt); NULLED(K); NULLED(verts); NULLED(v_off); NULLED(faces); NULLED(f_off); NULLED(scratch);
  NULLED(mesh_ids);                                // M == 2
  NULLED(diameters);                               // the sphere shortcut needs them
  WITH2(cus, nullptr, bbp, nullptr, CP_ERR_INVALID);         // nothing asked
  WITH(B, 0, CP_ERR_INVALID); WITH(M, 0, CP_ERR_INVALID); WITH(Vmax, 0, CP_ERR_INVALID); WITH(H, 0, CP_ERR_INVALID);
  WITH(W, -3, CP_ERR_INVALID); WITH(k_stride, 3, CP_ERR_INVALID);
  WITH(scratch, buf + 8, CP_ERR_ALIGN); WITH(est, d_odd, CP_ERR_ALIGN); WITH(gt, d_odd, CP_ERR_ALIGN); WITH(K, d_odd, CP_ERR_ALIGN);
  WITH(diameters, d_odd, CP_ERR_ALIGN); WITH(cus, d_odd, CP_ERR_ALIGN); WITH(bbp, d_odd, CP_ERR_ALIGN); WITH(verts, f_odd, CP_ERR_ALIGN);
  WITH(v_off, i_odd, CP_ERR_ALIGN); WITH(faces, i_odd, CP_ERR_ALIGN); WITH(f_off, i_odd, CP_ERR_ALIGN); WITH(mesh_ids, i_odd, CP_ERR_ALIGN);
  WITH(counts, i_odd, CP_ERR_ALIGN); WITH(boxes, i_odd, CP_ERR_ALIGN);
  WITH2(H, SIDE_31, W, SIDE_31, CP_ERR_RANGE);
  WITH2(B, 1 << 20, Vmax, 1 << 13, CP_ERR_RANGE);  // 2^20 pairs of 2 x 32 vertex chunks each
  WITH2(gt, nullptr, cus, d_odd, CP_ERR_INVALID);
  a = good; a.boxes = i_odd; a.H = SIDE_31; a.W = SIDE_31; EXPECT(call(a), CP_ERR_ALIGN);
  // scratch: B headers of 52 words, (B, 2, Vmax) float4, each part rounded up to 16 bytes
  EXPECT(cp_mask_errors_scratch_bytes(5, 12), 1040 + 1920); EXPECT(cp_mask_errors_scratch_bytes(3, 7), 624 + 672);
  EXPECT(cp_mask_errors_scratch_bytes(0, 12), 0); EXPECT(cp_mask_errors_scratch_bytes(5, -1), 0);
}

struct Rgb {        // cp_render_rgb
  const double* poses; const double* K; int k_stride; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off;
  int M; const int32_t* mesh_ids; const float* colors; const float* normals; const double* surf; const double* light; double ambient;
  const double* bg; int shading, ssaa, bgr, H, W, B, Vmax; uint8_t* rgb; float* depth; uint8_t* mask; int32_t* boxes; uint8_t* ok; void* scratch;
};
static void check_render_rgb() {
  const auto call = [](const Rgb& a) {
    return cp_render_rgb(nullptr, a.poses, a.K, a.k_stride, a.verts, a.v_off, a.faces, a.f_off, a.M, a.mesh_ids, a.colors, a.normals, a.surf,
                         a.light, a.ambient, a.bg, a.shading, a.ssaa, a.bgr, a.H, a.W, a.B, a.Vmax, a.rgb, a.depth, a.mask, a.boxes, a.ok,
                         a.scratch);
  };
  const Rgb good = {d, d, 0, f, i32, i32, i32, 2, i32, f, f, vec, vec, 0.5, vec, 1, 1, 0, 40, 48, 5, 12, u8, f, u8, i32, u8, buf};
  Rgb a;
  NULLED(poses); NULLED(K); NULLED(verts); NULLED(v_off); NULLED(faces); NULLED(f_off); NULLED(surf); NULLED(light); NULLED(bg); NULLED(rgb);
  NULLED(ok); NULLED(scratch);
  NULLED(normals);                                 // phong needs them
  NULLED(mesh_ids);                                // M == 2
  WITH(B, 0, CP_ERR_INVALID); WITH(M, 0, CP_ERR_INVALID); WITH(Vmax, 0, CP_ERR_INVALID); WITH(H, 0, CP_ERR_INVALID);
  WITH(W, -3, CP_ERR_INVALID); WITH(k_stride, 3, CP_ERR_INVALID);
  WITH(ssaa, 0, CP_ERR_INVALID); WITH(ssaa, 3, CP_ERR_INVALID); WITH(ssaa, 8, CP_ERR_INVALID);
  WITH(ssaa, 2, CP_ERR_INVALID);                   // depth, mask and boxes belong to ssaa = 1: each of them alone refuses the call
  a = good; a.ssaa = 2; a.mask = nullptr; a.boxes = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = good; a.ssaa = 4; a.depth = nullptr; a.boxes = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = good; a.ssaa = 2; a.depth = nullptr; a.mask = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  WITH(shading, 2, CP_ERR_INVALID); WITH(shading, -1, CP_ERR_INVALID); WITH(ambient, NAN, CP_ERR_INVALID);
  WITH(ambient, INFINITY, CP_ERR_INVALID); WITH(ambient, -INFINITY, CP_ERR_INVALID);
  WITH(surf, bad_vec, CP_ERR_INVALID); WITH(light, bad_vec, CP_ERR_INVALID); WITH(bg, bad_vec, CP_ERR_INVALID);
  WITH(scratch, buf + 8, CP_ERR_ALIGN); WITH(poses, d_odd, CP_ERR_ALIGN); WITH(K, d_odd, CP_ERR_ALIGN); WITH(verts, f_odd, CP_ERR_ALIGN);
  WITH(v_off, i_odd, CP_ERR_ALIGN); WITH(faces, i_odd, CP_ERR_ALIGN); WITH(f_off, i_odd, CP_ERR_ALIGN); WITH(mesh_ids, i_odd, CP_ERR_ALIGN);
  WITH(colors, f_odd, CP_ERR_ALIGN); WITH(normals, f_odd, CP_ERR_ALIGN); WITH(depth, f_odd, CP_ERR_ALIGN); WITH(boxes, i_odd, CP_ERR_ALIGN);
  WITH2(H, SIDE_31_3, W, SIDE_31_3, CP_ERR_RANGE);
  WITH(W, 1 << 24, CP_ERR_RANGE);                  // a sample row of 2^24
  a = good; a.ssaa = 4; a.H = 1 << 22; a.depth = nullptr; a.mask = nullptr; a.boxes = nullptr; EXPECT(call(a), CP_ERR_RANGE);
  WITH2(B, 1 << 20, Vmax, 1 << 13, CP_ERR_RANGE);  // 2^20 poses of 32 vertex chunks each
  WITH2(rgb, nullptr, colors, f_odd, CP_ERR_INVALID);
  WITH2(light, bad_vec, normals, f_odd, CP_ERR_INVALID);
  a = good; a.normals = f_odd; a.H = SIDE_31_3; a.W = SIDE_31_3; EXPECT(call(a), CP_ERR_ALIGN);
  // scratch: B headers of 48 words, four float4 tables of (B, Vmax), each part rounded up to 16 bytes
  EXPECT(cp_render_rgb_scratch_bytes(5, 12), 960 + 4 * 960); EXPECT(cp_render_rgb_scratch_bytes(3, 7), 576 + 4 * 336);
  EXPECT(cp_render_rgb_scratch_bytes(0, 12), 0); EXPECT(cp_render_rgb_scratch_bytes(5, -1), 0);
}

int main() {
  check_render_depth();
  check_vsd_errors();
  check_vsd_from_depth();
  check_gt_info();
  check_gt_info_from_depth();
  check_mask_errors();
  check_render_rgb();
  printf("raster host check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
