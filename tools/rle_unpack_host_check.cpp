// The host half of csrc/rle_unpack.hip -- cp_coco_rle_unpack's argument checks and cp_coco_rle_unpack_scratch_bytes -- exercised by a
// stand-alone program, so that it can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc rle_host_check`, then run checkerpose_amd/csrc/rle_host_check).  Every call below returns before any
// launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal as expected.
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

struct A {
  const int32_t* counts; const int64_t* offsets; int N, H, W; long long total;
  int32_t* ends; uint32_t* bits; int32_t* area; int32_t* box; int32_t* status;
};
static int call(const A& a) {
  return cp_coco_rle_unpack(nullptr, a.counts, a.offsets, a.N, a.H, a.W, a.total, a.ends, a.bits, a.area, a.box, a.status);
}

int main() {
  alignas(16) static unsigned char buf[8192];
  int32_t* i32 = (int32_t*)buf;
  const A ok = {i32, (const int64_t*)buf, 3, 480, 640, 100, i32, (uint32_t*)buf, i32, i32, i32};
  A a;
  // null pointers; counts / ends_scratch only while there are counts
  a = ok; a.offsets = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.area = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.box = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.status = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.counts = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.ends = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  // the sizes
  a = ok; a.N = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.N = -3; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.H = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.W = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.W = -640; EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.total = -1; EXPECT(call(a), CP_ERR_INVALID);
  // alignment: four bytes, the offsets eight
  for (int which = 0; which < 7; ++which) {
    a = ok;
    void* odd = buf + 2;
    if (which == 0) a.counts = (const int32_t*)odd;
    if (which == 1) a.offsets = (const int64_t*)(buf + 4);
    if (which == 2) a.ends = (int32_t*)odd;
    if (which == 3) a.bits = (uint32_t*)odd;
    if (which == 4) a.area = (int32_t*)odd;
    if (which == 5) a.box = (int32_t*)odd;
    if (which == 6) a.status = (int32_t*)odd;
    EXPECT(call(a), CP_ERR_ALIGN);
  }
  // the ranges
  a = ok; a.H = 1 << 16; a.W = 1 << 15; EXPECT(call(a), CP_ERR_RANGE);                       // H * W = 2^31
  a = ok; a.H = 1; a.W = (int)((1LL << 31) - 4096); EXPECT(call(a), CP_ERR_RANGE);          // the first H * W refused
  a = ok; a.N = 1 << 24; EXPECT(call(a), CP_ERR_RANGE);
  a = ok; a.total = 1LL << 31; EXPECT(call(a), CP_ERR_RANGE);
  a = ok; a.total = 1LL << 40; EXPECT(call(a), CP_ERR_RANGE);
  a = ok; a.N = (1 << 24) - 1; a.H = 4096; a.W = 4096; EXPECT(call(a), CP_ERR_RANGE);        // 2^34 workgroups in the bits launch
  // the order of the classes: INVALID before ALIGN before RANGE
  a = ok; a.H = 0; a.area = (int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_INVALID);
  a = ok; a.N = 1 << 24; a.area = (int32_t*)(buf + 2); EXPECT(call(a), CP_ERR_ALIGN);
  a = ok; a.total = 1LL << 31; a.counts = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  // the scratch
  EXPECT(cp_coco_rle_unpack_scratch_bytes(0), 0);
  EXPECT(cp_coco_rle_unpack_scratch_bytes(-7), 0);
  EXPECT(cp_coco_rle_unpack_scratch_bytes(1), 4);
  EXPECT(cp_coco_rle_unpack_scratch_bytes(19042), 4 * 19042);
  EXPECT(cp_coco_rle_unpack_scratch_bytes((1LL << 31) - 1), 4 * ((1LL << 31) - 1));
  EXPECT(cp_version() >= 239, 1);
  printf("rle host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
