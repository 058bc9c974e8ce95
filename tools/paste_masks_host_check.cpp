// The host halves of csrc/paste_masks.hip -- cp_paste_masks, cp_paste_rle_count, cp_paste_rle_write -- and of cp_coco_unpack
// (csrc/coco_eval.hip): argument checks, the offsets argument's checks -- exercised by a stand-alone program, so that they can be built
// under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C checkerpose_amd/csrc paste_host_check`, then run
// checkerpose_amd/csrc/paste_host_check).  Every call below returns before any launch: no device is needed, nothing is loaded into
// Python.  Exit status 0 = every refusal as expected.
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
  uint32_t* u32 = (uint32_t*)buf;
  uint8_t* u8 = buf;
  void* odd = buf + 2;

  // ---- the arguments the three paste entry points share
  struct S { const float* seg; long long bs; int Sh, Sw; const int32_t* win; int B, H, W; };
  const S okS = {f, 2 * 64 * 64, 64, 64, i32, 3, 480, 640};
  // cp_paste_masks: bits, area, box; cp_paste_rle_count: n_runs, area, box; cp_paste_rle_write: offsets, counts, total
  struct O { void* a; int32_t* b; int32_t* c; long long total; };
  const O okO = {buf, i32, i32, 16};
  auto call = [](int which, const S& s, const O& o) {
    if (which == 0) return cp_paste_masks(nullptr, s.seg, s.bs, s.Sh, s.Sw, s.win, s.B, s.H, s.W, (uint32_t*)o.a, o.b, o.c);
    if (which == 1) return cp_paste_rle_count(nullptr, s.seg, s.bs, s.Sh, s.Sw, s.win, s.B, s.H, s.W, (int32_t*)o.a, o.b, o.c);
    return cp_paste_rle_write(nullptr, s.seg, s.bs, s.Sh, s.Sw, s.win, s.B, s.H, s.W, (const int64_t*)o.a, o.b, o.total);
  };
  for (int which = 0; which < 3; ++which) {
    S s; O o;
    // null pointers
    s = okS; s.seg = nullptr; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.win = nullptr; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    o = okO; o.a = nullptr; EXPECT(call(which, okS, o), CP_ERR_INVALID);
    o = okO; o.b = nullptr; EXPECT(call(which, okS, o), CP_ERR_INVALID);
    if (which < 2) { o = okO; o.c = nullptr; EXPECT(call(which, okS, o), CP_ERR_INVALID); }
    // the batch and the stride
    s = okS; s.B = 0; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.B = -2; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.bs = -1; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    // the plane: 1..128 cells per side
    s = okS; s.Sh = 0; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.Sh = 129; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.Sw = 0; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.Sw = 129; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.Sw = -64; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    // the frame: 1..4096 pixels per side (the LDS pattern rows and the cell tables are sized by it)
    s = okS; s.H = 0; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.H = 4097; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.W = 0; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.W = 4097; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.H = 1 << 16; s.W = 1 << 15; EXPECT(call(which, s, okO), CP_ERR_INVALID);      // H * W = 2^31: refused by the side limit first
    // alignment
    s = okS; s.seg = (const float*)odd; EXPECT(call(which, s, okO), CP_ERR_ALIGN);
    s = okS; s.seg = (const float*)(buf + 1); EXPECT(call(which, s, okO), CP_ERR_ALIGN);
    s = okS; s.win = (const int32_t*)odd; EXPECT(call(which, s, okO), CP_ERR_ALIGN);
    o = okO; o.a = odd; EXPECT(call(which, okS, o), CP_ERR_ALIGN);
    o = okO; o.b = (int32_t*)odd; EXPECT(call(which, okS, o), CP_ERR_ALIGN);
    if (which < 2) { o = okO; o.c = (int32_t*)odd; EXPECT(call(which, okS, o), CP_ERR_ALIGN); }
    // the order of the classes: INVALID before ALIGN before RANGE
    s = okS; s.H = 0; s.seg = (const float*)odd; EXPECT(call(which, s, okO), CP_ERR_INVALID);
    s = okS; s.B = 1 << 24; s.seg = (const float*)odd; EXPECT(call(which, s, okO), CP_ERR_ALIGN);
    s = okS; s.B = 1 << 24; EXPECT(call(which, s, okO), CP_ERR_RANGE);
  }
  // the offsets argument: 8-byte aligned, total >= 1
  O o = okO; o.a = buf + 4; EXPECT(call(2, okS, o), CP_ERR_ALIGN);
  o = okO; o.total = 0; EXPECT(call(2, okS, o), CP_ERR_INVALID);
  o = okO; o.total = -5; EXPECT(call(2, okS, o), CP_ERR_INVALID);

  // ---- cp_coco_unpack
  EXPECT(cp_coco_unpack(nullptr, nullptr, 2, 31, 33, u8), CP_ERR_INVALID);
  EXPECT(cp_coco_unpack(nullptr, u32, 2, 31, 33, nullptr), CP_ERR_INVALID);
  EXPECT(cp_coco_unpack(nullptr, u32, 0, 31, 33, u8), CP_ERR_INVALID);
  EXPECT(cp_coco_unpack(nullptr, u32, 2, 0, 33, u8), CP_ERR_INVALID);
  EXPECT(cp_coco_unpack(nullptr, u32, 2, 31, -1, u8), CP_ERR_INVALID);
  EXPECT(cp_coco_unpack(nullptr, (const uint32_t*)odd, 2, 31, 33, u8), CP_ERR_ALIGN);
  EXPECT(cp_coco_unpack(nullptr, (const uint32_t*)odd, 2, 0, 33, u8), CP_ERR_INVALID);
  EXPECT(cp_coco_unpack(nullptr, u32, 2, 1 << 16, 1 << 15, u8), CP_ERR_RANGE);                // H * W = 2^31
  EXPECT(cp_coco_unpack(nullptr, u32, 1 << 24, 31, 33, u8), CP_ERR_RANGE);
  EXPECT(cp_coco_unpack(nullptr, u32, 1 << 23, 4096, 4096, u8), CP_ERR_RANGE);                 // 2^39 workgroups
  EXPECT(cp_version() >= 237, 1);
  printf("paste host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
