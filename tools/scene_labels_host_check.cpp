// The host half of csrc/scene_labels.hip and of cp_crop_mask_bits (csrc/preprocess.hip) -- argument checks, the CSR checks, the limit of
// 32 poses per image and scratch sizing -- exercised by a stand-alone program, so that it can be built under AddressSanitizer +
// UndefinedBehaviorSanitizer (`make -C checkerpose_amd/csrc scene_host_check`, then run checkerpose_amd/csrc/scene_host_check).
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
    if (got_ != (long long)(want)) { printf("FAIL %s: %lld, expected %lld\n", #what, got_, (long long)(want)); ++failures; } \
  } while (0)

struct Args {
  const double* poses; const double* K; int k_stride; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off;
  int M; const int32_t* mesh_ids; const float* colors; const float* normals; const double* surf; const int32_t* image_of_pose;
  const int32_t* img_off; const int32_t* pose_order; const int32_t* img_off_host; const int32_t* pose_order_host; const uint8_t* backgrounds;
  int n_bg; const int32_t* bg_index; const double* bg_color; int shading; double ambient; const double* light; double delta; int bgr, H, W, P, I,
      Vmax;
  uint8_t* rgb; float* depth; uint32_t* full_bits; uint32_t* visib_bits; int32_t* slot; int32_t* counts; double* fract; int32_t* boxes;
  uint8_t* ok; void* scratch;
};

static int call(const Args& a) {
  return cp_render_scene(nullptr, a.poses, a.K, a.k_stride, a.verts, a.v_off, a.faces, a.f_off, a.M, a.mesh_ids, a.colors, a.normals, a.surf,
                         a.image_of_pose, a.img_off, a.pose_order, a.img_off_host, a.pose_order_host, a.backgrounds, a.n_bg, a.bg_index,
                         a.bg_color, a.shading, a.ambient, a.light, a.delta, a.bgr, a.H, a.W, a.P, a.I, a.Vmax, a.rgb, a.depth, a.full_bits,
                         a.visib_bits, a.slot, a.counts, a.fract, a.boxes, a.ok, a.scratch);
}

int main() {
  alignas(16) static unsigned char buf[256];      // stands for every device pointer: never dereferenced by a refused call
  float* f = (float*)buf;
  int32_t* i32 = (int32_t*)buf;
  uint32_t* u32 = (uint32_t*)buf;
  double* d = (double*)buf;
  uint8_t* u8 = buf;
  const double vec[3] = {0.3, 0.3, 0.3};
  const int P = 5, I = 3;
  const int32_t off[I + 1] = {0, 2, 2, 5}, order[P] = {0, 3, 1, 2, 4};
  const Args good = {d, d, 0, f, i32, i32, i32, 2, i32, f, f, d, i32, i32, i32, off, order, u8, 3, i32, vec, 1, 0.5, vec, 15.0, 0, 40, 48, P, I, 12,
                     u8, f, u32, u32, i32, i32, d, i32, u8, buf};
  Args a;
  // null pointers
#define NULLED(field) a = good; a.field = nullptr; EXPECT(call(a), CP_ERR_INVALID)
  NULLED(poses); NULLED(K); NULLED(verts); NULLED(v_off); NULLED(faces); NULLED(f_off); NULLED(image_of_pose); NULLED(img_off);
  NULLED(pose_order); NULLED(img_off_host); NULLED(pose_order_host); NULLED(bg_color); NULLED(light); NULLED(rgb); NULLED(depth);
  NULLED(full_bits); NULLED(visib_bits); NULLED(slot); NULLED(counts); NULLED(fract); NULLED(boxes); NULLED(ok); NULLED(scratch);
  NULLED(normals);                                 // phong needs them
  NULLED(mesh_ids);                                // M == 2
  NULLED(backgrounds);                             // n_bg and bg_index without backgrounds
  // shapes and enums
#define WITH(field, value, want) a = good; a.field = value; EXPECT(call(a), want)
  WITH(P, 0, CP_ERR_INVALID); WITH(I, 0, CP_ERR_INVALID); WITH(M, 0, CP_ERR_INVALID); WITH(Vmax, 0, CP_ERR_INVALID);
  WITH(H, 0, CP_ERR_INVALID); WITH(W, -3, CP_ERR_INVALID); WITH(k_stride, 3, CP_ERR_INVALID); WITH(shading, 2, CP_ERR_INVALID);
  WITH(shading, -1, CP_ERR_INVALID); WITH(bgr, 2, CP_ERR_INVALID); WITH(ambient, NAN, CP_ERR_INVALID); WITH(ambient, INFINITY, CP_ERR_INVALID);
  WITH(delta, NAN, CP_ERR_INVALID); WITH(n_bg, 0, CP_ERR_INVALID);
  const double bad_vec[3] = {0.3, NAN, 0.3};
  WITH(light, bad_vec, CP_ERR_INVALID); WITH(bg_color, bad_vec, CP_ERR_INVALID);
  // backgrounds: without bg_index there must be one row, or one per image; without backgrounds neither a count nor an index
  a = good; a.bg_index = nullptr; a.n_bg = 2; EXPECT(call(a), CP_ERR_INVALID);
  a = good; a.backgrounds = nullptr; a.bg_index = nullptr; a.n_bg = 1; EXPECT(call(a), CP_ERR_INVALID);
  // alignment
  WITH(scratch, buf + 8, CP_ERR_ALIGN); WITH(poses, (const double*)(buf + 4), CP_ERR_ALIGN); WITH(surf, (const double*)(buf + 4), CP_ERR_ALIGN);
  WITH(fract, (double*)(buf + 4), CP_ERR_ALIGN); WITH(verts, (const float*)(buf + 2), CP_ERR_ALIGN); WITH(depth, (float*)(buf + 2), CP_ERR_ALIGN);
  WITH(full_bits, (uint32_t*)(buf + 2), CP_ERR_ALIGN); WITH(visib_bits, (uint32_t*)(buf + 1), CP_ERR_ALIGN);
  WITH(boxes, (int32_t*)(buf + 1), CP_ERR_ALIGN); WITH(slot, (int32_t*)(buf + 2), CP_ERR_ALIGN); WITH(bg_index, (const int32_t*)(buf + 2), CP_ERR_ALIGN);
  WITH(img_off, (const int32_t*)(buf + 2), CP_ERR_ALIGN);
  // the CSR
  const int32_t off_first[I + 1] = {1, 2, 2, 5}, off_last[I + 1] = {0, 2, 2, 4}, off_back[I + 1] = {0, 3, 2, 5};
  WITH(img_off_host, off_first, CP_ERR_INVALID); WITH(img_off_host, off_last, CP_ERR_INVALID); WITH(img_off_host, off_back, CP_ERR_INVALID);
  const int32_t order_hi[P] = {0, 3, 1, 2, 5}, order_lo[P] = {0, -1, 1, 2, 4};
  WITH(pose_order_host, order_hi, CP_ERR_INVALID); WITH(pose_order_host, order_lo, CP_ERR_INVALID);
  {                                                // 33 poses in one image: a pose per bit, no more
    static int32_t order33[34];
    for (int j = 0; j < 34; ++j) order33[j] = j;
    const int32_t off33[3] = {0, 33, 34}, off32[3] = {0, 32, 34};
    a = good; a.P = 34; a.I = 2; a.n_bg = 2; a.pose_order_host = order33; a.img_off_host = off33; EXPECT(call(a), CP_ERR_RANGE);
    // 32 pass that check: the call goes on to the size checks (a frame side of 2^24 refuses it there, still before any launch)
    a.img_off_host = off32; a.W = 1 << 24; EXPECT(call(a), CP_ERR_RANGE);
    // 33 poses in one image and an entry of pose_order that is no pose: the CSR's INVALID comes before the limit's RANGE
    static int32_t order33_bad[34];
    for (int j = 0; j < 34; ++j) order33_bad[j] = j == 33 ? 34 : j;
    a = good; a.P = 34; a.I = 2; a.n_bg = 2; a.pose_order_host = order33_bad; a.img_off_host = off33; EXPECT(call(a), CP_ERR_INVALID);
  }
  // two rules broken at once: INVALID before ALIGN, ALIGN before the CSR's INVALID, the CSR before RANGE
  a = good; a.rgb = nullptr; a.verts = (const float*)(buf + 2); EXPECT(call(a), CP_ERR_INVALID);
  a = good; a.slot = (int32_t*)(buf + 2); a.W = 1 << 24; EXPECT(call(a), CP_ERR_ALIGN);
  a = good; a.fract = (double*)(buf + 4); a.img_off_host = off_back; EXPECT(call(a), CP_ERR_ALIGN);
  a = good; a.pose_order_host = order_hi; a.W = 1 << 24; EXPECT(call(a), CP_ERR_INVALID);
  // sizes: a frame side of 2^24, a batch of 2^31 / 3 bytes, a canvas of 2^31 / 9 pixels, 2^24 workgroups
  WITH(W, 1 << 24, CP_ERR_RANGE);
  a = good; a.H = 4096; a.W = 4096; a.I = 64; a.n_bg = 1; { static int32_t big_off[65]; for (int i = 0; i < 65; ++i) big_off[i] = i == 0 ? 0 : P; a.img_off_host = big_off; EXPECT(call(a), CP_ERR_RANGE); }
  a = good; a.H = 16384; a.W = 16384; a.I = 1; a.n_bg = 1; { const int32_t one_off[2] = {0, P}; a.img_off_host = one_off; EXPECT(call(a), CP_ERR_RANGE); }
  // scratch: P headers of 64 words, four float4 tables of (P, Vmax)
  EXPECT(cp_render_scene_scratch_bytes(5, 12, 3), 5 * 64 * 4 + 4 * 5 * 12 * 16);
  EXPECT(cp_render_scene_scratch_bytes(3, 7, 1), 3 * 64 * 4 + 4 * 3 * 7 * 16);
  EXPECT(cp_render_scene_scratch_bytes(0, 12, 3), 0); EXPECT(cp_render_scene_scratch_bytes(5, -1, 3), 0); EXPECT(cp_render_scene_scratch_bytes(5, 12, 0), 0);

  // cp_crop_mask_bits
  auto crop = [&](const uint32_t* plane, int n_img, int H, int W, const int32_t* win, const int32_t* idx, const int32_t* bit, uint8_t* out, int B,
                  int size) { return cp_crop_mask_bits(nullptr, plane, n_img, H, W, win, idx, bit, out, B, size); };
  EXPECT(crop(nullptr, 2, 40, 48, i32, i32, i32, u8, 3, 64), CP_ERR_INVALID);
  EXPECT(crop(u32, 2, 40, 48, nullptr, i32, i32, u8, 3, 64), CP_ERR_INVALID);
  EXPECT(crop(u32, 2, 40, 48, i32, i32, nullptr, u8, 3, 64), CP_ERR_INVALID);
  EXPECT(crop(u32, 2, 40, 48, i32, i32, i32, nullptr, 3, 64), CP_ERR_INVALID);
  EXPECT(crop(u32, 2, 40, 48, i32, nullptr, i32, u8, 3, 64), CP_ERR_INVALID);          // 2 images, 3 crops: which image?
  EXPECT(crop(u32, 0, 40, 48, i32, i32, i32, u8, 3, 64), CP_ERR_INVALID);
  EXPECT(crop(u32, 2, 0, 48, i32, i32, i32, u8, 3, 64), CP_ERR_INVALID);
  EXPECT(crop(u32, 2, 40, -1, i32, i32, i32, u8, 3, 64), CP_ERR_INVALID);
  EXPECT(crop(u32, 2, 40, 48, i32, i32, i32, u8, 0, 64), CP_ERR_INVALID);
  EXPECT(crop(u32, 2, 40, 48, i32, i32, i32, u8, 3, 0), CP_ERR_INVALID);
  EXPECT(crop((const uint32_t*)(buf + 2), 2, 40, 48, i32, i32, i32, u8, 3, 64), CP_ERR_ALIGN);
  EXPECT(crop(u32, 2, 40, 48, (const int32_t*)(buf + 1), i32, i32, u8, 3, 64), CP_ERR_ALIGN);
  EXPECT(crop(u32, 2, 40, 48, i32, i32, (const int32_t*)(buf + 2), u8, 3, 64), CP_ERR_ALIGN);
  EXPECT(crop(u32, 1, 65536, 65536, i32, i32, i32, u8, 3, 64), CP_ERR_RANGE);
  printf("scene_labels host check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
