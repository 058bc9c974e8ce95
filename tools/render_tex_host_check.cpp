// The host halves of the three textured entry points (row N20: cp_render_rgb_tex in csrc/render_rgb.hip, cp_vis_poses_tex in
// csrc/vis_poses.hip, cp_render_scene_tex in csrc/scene_labels.hip) -- the plain calls' argument checks, which they share, and the checks
// of the five texture arguments -- exercised by a stand-alone program, so that it can be built under AddressSanitizer +
// UndefinedBehaviorSanitizer (`make -C checkerpose_amd/csrc tex_host_check`, then run checkerpose_amd/csrc/tex_host_check).
// Every call below is refused before any launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal
// as expected.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../include/checkerpose_hip.h"

static int failures = 0;
#define EXPECT(what, want)                                                                          \
  do {                                                                                              \
    const long long got_ = (long long)(what);                                                       \
    if (got_ != (long long)(want)) { printf("FAIL %s (line %d): %lld, expected %lld\n", #what, __LINE__, got_, (long long)(want)); ++failures; } \
  } while (0)

struct Tex { const float* uv; const uint32_t* texels; const int32_t* off; const int32_t* dims; int filter; };

alignas(16) static unsigned char buf[256];        // stands for every device pointer: never dereferenced by a refused call
static float* const f = (float*)buf;
static int32_t* const i32 = (int32_t*)buf;
static uint32_t* const u32 = (uint32_t*)buf;
static double* const d = (double*)buf;
static uint8_t* const u8 = buf;
static const double vec[3] = {0.3, 0.3, 0.3};
static const int32_t off[4] = {0, 2, 2, 5}, order[5] = {0, 3, 1, 2, 4};

// each call with ONE thing of the plain arguments varied: the frame width W, the pose count, the scratch pointer
static int rgb(const Tex& t, int W = 48, int B = 5, void* scratch = buf) {
  return cp_render_rgb_tex(nullptr, d, d, 0, f, i32, i32, i32, 2, i32, f, f, vec, vec, 0.5, vec, 1, 1, 0, 40, W, B, 12, u8, f, u8, i32, u8, scratch,
                           t.uv, t.texels, t.off, t.dims, t.filter);
}
static int vis(const Tex& t, int W = 48, int P = 5, void* scratch = buf) {
  return cp_vis_poses_tex(nullptr, d, d, 0, f, i32, i32, i32, 2, i32, f, f, d, i32, i32, i32, off, order, u8, 1, 0.5, vec, vec, 1, 1, 40, W, P, 3, 12,
                          u8, u8, f, i32, u8, scratch, t.uv, t.texels, t.off, t.dims, t.filter);
}
static int scene(const Tex& t, int W = 48, int P = 5, void* scratch = buf) {
  return cp_render_scene_tex(nullptr, d, d, 0, f, i32, i32, i32, 2, i32, f, f, d, i32, i32, i32, off, order, u8, 3, i32, vec, 1, 0.5, vec, 15.0, 0, 40,
                             W, P, 3, 12, u8, f, u32, u32, i32, i32, d, i32, u8, scratch, t.uv, t.texels, t.off, t.dims, t.filter);
}

template <class Call>
static void check(Call call) {
  const Tex good = {f, u32, i32, i32, 1}, none = {nullptr, nullptr, nullptr, nullptr, 0};
  Tex t;
  // the four tables come together or not at all
  t = good; t.uv = nullptr; EXPECT(call(t, 48, 5, buf), CP_ERR_INVALID);                 // null UVs with texels
  t = good; t.texels = nullptr; EXPECT(call(t, 48, 5, buf), CP_ERR_INVALID);
  t = good; t.off = nullptr; EXPECT(call(t, 48, 5, buf), CP_ERR_INVALID);
  t = good; t.dims = nullptr; EXPECT(call(t, 48, 5, buf), CP_ERR_INVALID);
  t = none; t.uv = f; EXPECT(call(t, 48, 5, buf), CP_ERR_INVALID);
  t = none; t.dims = i32; EXPECT(call(t, 48, 5, buf), CP_ERR_INVALID);
  // the filter, with and without tables
  t = good; t.filter = 2; EXPECT(call(t, 48, 5, buf), CP_ERR_INVALID);
  t = good; t.filter = -1; EXPECT(call(t, 48, 5, buf), CP_ERR_INVALID);
  t = none; t.filter = 7; EXPECT(call(t, 48, 5, buf), CP_ERR_INVALID);
  // alignment
  t = good; t.uv = (const float*)(buf + 2); EXPECT(call(t, 48, 5, buf), CP_ERR_ALIGN);
  t = good; t.texels = (const uint32_t*)(buf + 1); EXPECT(call(t, 48, 5, buf), CP_ERR_ALIGN);
  t = good; t.off = (const int32_t*)(buf + 2); EXPECT(call(t, 48, 5, buf), CP_ERR_ALIGN);
  t = good; t.dims = (const int32_t*)(buf + 3); EXPECT(call(t, 48, 5, buf), CP_ERR_ALIGN);
  // the plain calls' checks hold with and without tables: sizes, the scratch pointer.  Good texture arguments pass theirs: the call
  // goes on to the size checks, where a frame side of 2^24 refuses it, still before any launch
  for (const Tex& x : {good, none}) {
    EXPECT(call(x, 0, 5, buf), CP_ERR_INVALID); EXPECT(call(x, -3, 5, buf), CP_ERR_INVALID); EXPECT(call(x, 48, 0, buf), CP_ERR_INVALID);
    EXPECT(call(x, 48, 5, nullptr), CP_ERR_INVALID); EXPECT(call(x, 48, 5, buf + 8), CP_ERR_ALIGN);
    EXPECT(call(x, 1 << 24, 5, buf), CP_ERR_RANGE);
  }
  t = good; t.filter = 0; EXPECT(call(t, 1 << 24, 5, buf), CP_ERR_RANGE);
}

int main() {
  check(rgb);
  check(vis);
  check(scene);
  // the plain entry points forward with no tables: the same refusals
  EXPECT(cp_render_rgb(nullptr, d, d, 0, f, i32, i32, i32, 2, i32, f, f, vec, vec, 0.5, vec, 1, 1, 0, 40, 1 << 24, 5, 12, u8, f, u8, i32, u8, buf),
         CP_ERR_RANGE);
  EXPECT(cp_render_rgb(nullptr, d, d, 0, f, i32, i32, i32, 2, i32, f, f, vec, vec, 0.5, vec, 1, 3, 0, 40, 48, 5, 12, u8, f, u8, i32, u8, buf),
         CP_ERR_INVALID);
  // scratch sizes do not depend on textures: the plain queries serve both
  EXPECT(cp_render_rgb_scratch_bytes(5, 12), 5 * 48 * 4 + 4 * 5 * 12 * 16);
  EXPECT(cp_vis_poses_scratch_bytes(5, 12, 3), 5 * 48 * 4 + 4 * 5 * 12 * 16);
  EXPECT(cp_render_scene_scratch_bytes(5, 12, 3), 5 * 64 * 4 + 4 * 5 * 12 * 16);
  EXPECT(cp_version() >= 230, 1);
  printf("render_tex host check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
