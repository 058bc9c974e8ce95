// The host half of csrc/pose_verify_photo.hip -- cp_verify_poses_photo, cp_verify_poses_photo_tex: argument checks, scratch sizing --
// exercised by a stand-alone program, so that it can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc photo_host_check`, then run checkerpose_amd/csrc/photo_host_check).  Every call below returns before
// any launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal as expected.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../include/checkerpose_hip.h"

static int failures = 0, refusals = 0;
#define EXPECT(what, want)                                                                          \
  do {                                                                                              \
    const long long got_ = (long long)(what);                                                       \
    if (got_ != (long long)(want)) { printf("FAIL %s: %lld, expected %lld\n", #what, got_, (long long)(want)); ++failures; } \
    else if ((long long)(want) < 0) ++refusals;                                                     \
  } while (0)

int main() {
  alignas(16) static unsigned char buf[8192];
  float* f = (float*)buf;
  int32_t* i32 = (int32_t*)buf;
  int64_t* i64 = (int64_t*)buf;
  double* d = (double*)buf;
  uint8_t* u8 = buf;
  void* odd = buf + 2;
  static const double grey[3] = {0.5, 0.5, 0.5}, light[3] = {0.0, 0.0, 0.0};
  static const double bad3[3] = {0.5, NAN, 0.5};

  struct A {
    const double* poses; const double* K; int ks; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off; int M;
    const int32_t* ids; const float* colors; const float* normals; const double* surf; const double* light; double ambient; int shading;
    const uint8_t* frames; const int32_t* image_ids; int I, H, W, bgr; const int32_t* vis; const int32_t* mask_ids; int NM;
    const int32_t* status; int min_pixels, P, Vmax; int32_t* counts; int64_t* sums; double* ncc; double* score; double* gain; double* offset;
    uint8_t* ok; void* scratch; const float* uv; const uint32_t* texels; const int32_t* tex_off; const int32_t* tex_dims; int filter;
  };
  const A okA = {d, d, 0, f, i32, i32, i32, 1, nullptr, nullptr, nullptr, grey, light, 0.5, 0, u8, nullptr, 1, 80, 96, 0, nullptr, nullptr, 0,
                 nullptr, 2, 3, 64, i32, i64, d, d, d, d, u8, buf, nullptr, nullptr, nullptr, nullptr, 0};
  auto call = [](const A& a) {
    return cp_verify_poses_photo_tex(nullptr, a.poses, a.K, a.ks, a.verts, a.v_off, a.faces, a.f_off, a.M, a.ids, a.colors, a.normals, a.surf,
                                     a.light, a.ambient, a.shading, a.frames, a.image_ids, a.I, a.H, a.W, a.bgr, a.vis, a.mask_ids, a.NM,
                                     a.status, a.min_pixels, a.P, a.Vmax, a.counts, a.sums, a.ncc, a.score, a.gain, a.offset, a.ok, a.scratch,
                                     a.uv, a.texels, a.tex_off, a.tex_dims, a.filter);
  };
  auto plain = [](const A& a) {
    return cp_verify_poses_photo(nullptr, a.poses, a.K, a.ks, a.verts, a.v_off, a.faces, a.f_off, a.M, a.ids, a.colors, a.normals, a.surf,
                                 a.light, a.ambient, a.shading, a.frames, a.image_ids, a.I, a.H, a.W, a.bgr, a.vis, a.mask_ids, a.NM, a.status,
                                 a.min_pixels, a.P, a.Vmax, a.counts, a.sums, a.ncc, a.score, a.gain, a.offset, a.ok, a.scratch);
  };
  A a;
  // null pointers (mesh_ids, colors, normals with flat shading, image_ids, the masks, status and the texture tables may be null)
  a = okA; a.poses = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.K = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.surf = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.light = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.frames = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.counts = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.sums = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.ncc = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.score = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.gain = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.offset = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.ok = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.scratch = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.poses = nullptr; EXPECT(plain(a), CP_ERR_INVALID);
  a = okA; a.frames = nullptr; EXPECT(plain(a), CP_ERR_INVALID);
  // the mesh table
  a = okA; a.verts = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.v_off = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.faces = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.f_off = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.M = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.M = 2; EXPECT(call(a), CP_ERR_INVALID);                           // several meshes need ids
  a = okA; a.Vmax = 0; EXPECT(call(a), CP_ERR_INVALID);
  // the view and the images
  a = okA; a.ks = 3; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.H = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.W = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.P = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.P = -4; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.I = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.I = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.I = 2; EXPECT(call(a), CP_ERR_INVALID);                           // several images need ids
  // min_pixels: no default, at least 2
  a = okA; a.min_pixels = 1; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.min_pixels = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.min_pixels = -7; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.min_pixels = 1; EXPECT(plain(a), CP_ERR_INVALID);
  // the visible masks
  a = okA; a.vis = i32; EXPECT(call(a), CP_ERR_INVALID);                       // masks with NM == 0
  a = okA; a.vis = i32; a.NM = -2; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.vis = i32; a.NM = 2; EXPECT(call(a), CP_ERR_INVALID);             // NM != P needs mask ids
  a = okA; a.vis = i32; a.NM = 5; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.NM = 3; EXPECT(call(a), CP_ERR_INVALID);                          // a count without masks
  a = okA; a.mask_ids = i32; EXPECT(call(a), CP_ERR_INVALID);                  // ids without masks
  // the shading, the light, the colours
  a = okA; a.shading = 2; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.shading = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.shading = 1; EXPECT(call(a), CP_ERR_INVALID);                     // phong without normals
  a = okA; a.ambient = NAN; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.ambient = INFINITY; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.light = bad3; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.surf = bad3; EXPECT(call(a), CP_ERR_INVALID);
  // the texture tables: all four or none, a known filter
  a = okA; a.uv = f; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.uv = f; a.texels = (const uint32_t*)buf; a.tex_off = i32; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.texels = (const uint32_t*)buf; a.tex_off = i32; a.tex_dims = i32; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.filter = 2; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.filter = -1; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.uv = (const float*)odd; a.texels = (const uint32_t*)buf; a.tex_off = i32; a.tex_dims = i32; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.uv = f; a.texels = (const uint32_t*)odd; a.tex_off = i32; a.tex_dims = i32; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.uv = f; a.texels = (const uint32_t*)buf; a.tex_off = (const int32_t*)odd; a.tex_dims = i32; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.uv = f; a.texels = (const uint32_t*)buf; a.tex_off = i32; a.tex_dims = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  // alignment
  a = okA; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.poses = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.K = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.verts = (const float*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.v_off = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.faces = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.f_off = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.ids = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.colors = (const float*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.normals = (const float*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.image_ids = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.vis = (const int32_t*)odd; a.NM = 3; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.vis = i32; a.NM = 5; a.mask_ids = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.status = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.counts = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.sums = (int64_t*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.ncc = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.score = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.gain = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.offset = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  // the order of the classes: INVALID before ALIGN before RANGE
  a = okA; a.H = 0; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.H = 2049; a.W = 2048; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_ALIGN);
  // sizes: H W <= 2^22 (a tile's sums are int32, a pose's products int64)
  a = okA; a.H = 2049; a.W = 2048; EXPECT(call(a), CP_ERR_RANGE);              // H * W = 2^22 + 2048
  a = okA; a.H = 2049; a.W = 2048; EXPECT(plain(a), CP_ERR_RANGE);
  a = okA; a.H = 1; a.W = (1 << 22) + 1; EXPECT(call(a), CP_ERR_RANGE);
  a = okA; a.H = 1 << 16; a.W = 1 << 15; EXPECT(call(a), CP_ERR_RANGE);
  a = okA; a.H = 2048; a.W = 2048; a.P = 1 << 12; EXPECT(call(a), CP_ERR_RANGE);      // H * W = 2^22 is allowed; 2^24 tile blocks are not
  a = okA; a.P = 1 << 20; a.Vmax = 1 << 12; EXPECT(call(a), CP_ERR_RANGE);            // 2^24 vertex blocks
  // the scratch: a header of 64 words per pose, then four (P, Vmax) float4 tables
  EXPECT(cp_verify_poses_photo_scratch_bytes(0, 64), 0);
  EXPECT(cp_verify_poses_photo_scratch_bytes(-1, 64), 0);
  EXPECT(cp_verify_poses_photo_scratch_bytes(3, -1), 0);
  EXPECT(cp_verify_poses_photo_scratch_bytes(3, 64), 768 + 4 * 3 * 64 * 16);
  EXPECT(cp_verify_poses_photo_scratch_bytes(1, 0), 256);
  EXPECT(cp_verify_poses_photo_scratch_bytes(5, 3), 1280 + 4 * 240);
  EXPECT(cp_version() >= 245, 1);
  printf("photo host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
