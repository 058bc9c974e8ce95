// The host half of csrc/warp_affine.hip -- the argument checks of cp_warp_affine_u8 and cp_warp_mask_bits -- exercised by a stand-alone
// program, so that it can be built under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C checkerpose_amd/csrc warp_host_check`,
// then run checkerpose_amd/csrc/warp_host_check).  Every call below is refused before any launch: no device is needed, nothing is
// loaded into Python.  Exit status 0 = every refusal as expected.
#include <stdint.h>
#include <stdio.h>

#include "../include/checkerpose_hip.h"

static int failures = 0;
#define EXPECT(what, want)                                                                          \
  do {                                                                                              \
    const long long got_ = (long long)(what);                                                       \
    if (got_ != (long long)(want)) { printf("FAIL %s: %lld, expected %lld\n", #what, got_, (long long)(want)); ++failures; } \
  } while (0)

int main() {
  alignas(16) static unsigned char buf[256];      // stands for every device pointer: never dereferenced by a refused call
  const uint8_t* u8 = buf;
  uint8_t* out = buf;
  const double* f64 = (const double*)buf;
  const int32_t* i32 = (const int32_t*)buf;
  const uint32_t* u32 = (const uint32_t*)buf;
  auto warp = [&](const uint8_t* images, int n_img, int H, int W, int C, const double* inv, const int32_t* idx, uint8_t* o, int B, int oh, int ow,
                  int interp) { return cp_warp_affine_u8(nullptr, images, n_img, H, W, C, inv, idx, o, B, oh, ow, interp); };
  EXPECT(warp(nullptr, 2, 48, 64, 3, f64, i32, out, 3, 8, 8, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 48, 64, 3, nullptr, i32, out, 3, 8, 8, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 48, 64, 3, f64, i32, nullptr, 3, 8, 8, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 48, 64, 3, f64, nullptr, out, 3, 8, 8, 1), CP_ERR_INVALID);          // 2 images, 3 crops: which image?
  EXPECT(warp(u8, 2, 48, 64, 5, f64, i32, out, 3, 8, 8, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 48, 64, 0, f64, i32, out, 3, 8, 8, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 0, 48, 64, 3, f64, i32, out, 3, 8, 8, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 0, 64, 3, f64, i32, out, 3, 8, 8, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 48, -1, 3, f64, i32, out, 3, 8, 8, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 48, 64, 3, f64, i32, out, 0, 8, 8, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 48, 64, 3, f64, i32, out, 3, 0, 8, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 48, 64, 3, f64, i32, out, 3, 8, -2, 1), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 48, 64, 3, f64, i32, out, 3, 8, 8, 2), CP_ERR_INVALID);
  EXPECT(warp(u8, 2, 48, 64, 3, (const double*)(buf + 4), i32, out, 3, 8, 8, 1), CP_ERR_ALIGN);
  EXPECT(warp(u8, 2, 48, 64, 3, f64, (const int32_t*)(buf + 2), out, 3, 8, 8, 1), CP_ERR_ALIGN);
  EXPECT(warp(buf + 1, 2, 48, 64, 4, f64, i32, out, 3, 8, 8, 1), CP_ERR_ALIGN);          // dword taps
  EXPECT(warp(u8, 2, 48, 64, 4, f64, i32, buf + 2, 3, 8, 8, 1), CP_ERR_ALIGN);           // dword stores
  EXPECT(warp(u8, 1, 65536, 65536, 3, f64, i32, out, 3, 8, 8, 1), CP_ERR_RANGE);
  EXPECT(warp(u8, 1, 48, 64, 3, f64, i32, out, 3, 65536, 65536, 1), CP_ERR_RANGE);
  EXPECT(warp(u8, 1, 48, 64, 3, f64, i32, out, 1 << 20, 4096, 4096, 1), CP_ERR_RANGE);
  auto bits = [&](const uint32_t* plane, int n_img, int H, int W, const double* inv, const int32_t* idx, const int32_t* bit, uint8_t* o, int B, int oh,
                  int ow) { return cp_warp_mask_bits(nullptr, plane, n_img, H, W, inv, idx, bit, o, B, oh, ow); };
  EXPECT(bits(nullptr, 2, 48, 64, f64, i32, i32, out, 3, 8, 8), CP_ERR_INVALID);
  EXPECT(bits(u32, 2, 48, 64, nullptr, i32, i32, out, 3, 8, 8), CP_ERR_INVALID);
  EXPECT(bits(u32, 2, 48, 64, f64, i32, nullptr, out, 3, 8, 8), CP_ERR_INVALID);
  EXPECT(bits(u32, 2, 48, 64, f64, i32, i32, nullptr, 3, 8, 8), CP_ERR_INVALID);
  EXPECT(bits(u32, 2, 48, 64, f64, nullptr, i32, out, 3, 8, 8), CP_ERR_INVALID);
  EXPECT(bits(u32, 2, 48, 64, f64, i32, i32, out, 3, 8, 0), CP_ERR_INVALID);
  EXPECT(bits((const uint32_t*)(buf + 2), 2, 48, 64, f64, i32, i32, out, 3, 8, 8), CP_ERR_ALIGN);
  EXPECT(bits(u32, 2, 48, 64, f64, i32, (const int32_t*)(buf + 1), out, 3, 8, 8), CP_ERR_ALIGN);
  EXPECT(bits(u32, 2, 48, 64, (const double*)(buf + 4), i32, i32, out, 3, 8, 8), CP_ERR_ALIGN);
  EXPECT(bits(u32, 1, 65536, 65536, f64, i32, i32, out, 3, 8, 8), CP_ERR_RANGE);
  printf("warp_affine host check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
