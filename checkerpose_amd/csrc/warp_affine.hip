// Input side on the device, SURVEY.md 8f row N21: the loader's third resize_method, "crop_resize_by_warp_affine"
// (bop_dataset_pytorch.py:39-52, 111-129, 132-145 -> GDR_Net_Augmentation.py:199-240 get_affine_transform -> cv2.warpAffine), for a whole
// batch in ONE launch from full uint8 images that are already in HBM.  It is not a variant of cp_crop_resize_u8 (preprocess.hip): there is
// no half-pixel centre shift, coordinates are quantised to 1/32 pixel, four taps are blended with 15-bit weights, every tap outside the
// frame counts as zero on its own, and the map may rotate.
//
// THE RULE.  cv2 is not available where this project is built and tested, so parity with cv2's own bytes is UNPINNED (as for row N3's
// cv2.resize).  What follows is OpenCV's published imgwarp.cpp arithmetic for 8-bit images (warpAffine -> WarpAffineInvoker -> remap's
// fixed-point bilinear table); the numpy restatement is tests/warp_stages.py.
//   The host (checkerpose_amd/preprocess.py) hands over the INVERSE map A, b of each crop as six doubles a00 a01 b0 a10 a11 b1: output
//   pixel (x, y) samples the source at A . (x, y) + b.  From a forward matrix M (dst = M . src) it is invertAffineTransform's, in float64:
//     D = M00 M11 - M01 M10;  D = D != 0 ? 1 / D : 0;  A = [[M11 D, -M01 D], [-M10 D, M00 D]];  b = -A . (M02, M12), every product
//     rounded on its own.  With inverse_map the given matrix is used as it is.
//   AB_BITS = 10, INTER_BITS = 5.  With rint = round half to even, saturated to int32, in float64, the product and the sum inside X0 / Y0
//   rounded separately (no fma: `fp contract(off)` below):
//     adelta[x] = rint(a00 * x * 1024)        bdelta[x] = rint(a10 * x * 1024)
//     X0[y] = rint((a01 * y + b0) * 1024) + rd        Y0[y] = rint((a11 * y + b1) * 1024) + rd
//     rd = 512 for INTER_NEAREST, 16 for INTER_LINEAR; the sums X0 + adelta, Y0 + bdelta are int32 (the host refuses a map that sends an
//     output corner further than 2^20 pixels from the origin, where they would wrap as they do in OpenCV).
//   INTER_NEAREST: source pixel ((Y0 + bdelta[x]) >> 10, (X0 + adelta[x]) >> 10), zero outside the frame.
//   INTER_LINEAR:  X = (X0 + adelta[x]) >> 5, Y likewise; sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31; weights
//     (32 - fy)(32 - fx) 32, (32 - fy) fx 32, fy (32 - fx) 32, fy fx 32 (sum 2^15) on the taps (sy, sx), (sy, sx + 1), (sy + 1, sx),
//     (sy + 1, sx + 1); a tap outside the frame counts as 0 on its own (BORDER_CONSTANT, value 0); per channel (sum + 16384) >> 15.
//   All shifts are arithmetic.  A row of inv_mats that holds a NaN marks "no box": a zero crop.
//
// One thread per output pixel, all channels; every thread derives its own adelta / bdelta / X0 / Y0 (a dozen fp64 operations against four
// byte gathers that miss L1 at arbitrary positions: L2 / HBM bound).  A C == 4 tap is one dword load, and a C == 4 pixel one dword
// store; consecutive threads write consecutive pixels of a row.  No LDS stage.
//
// cp_warp_mask_bits: the INTER_NEAREST warp of ONE BIT of a uint32 plane (cp_render_scene's full_bits / visib_bits) as the 0 / 255 mask
// that bit stands for -- warp_fixed's coordinates, so the crop equals cp_warp_affine_u8's of the expanded mask image, which is never
// stored (what cp_crop_mask_bits is to cp_crop_resize_u8).
#include "common.h"

// saturate_cast<int>(double): round half to even, clamped to int32
__device__ __forceinline__ int warp_sat_rint(double v) { return (int)fmin(fmax(rint(v), -2147483648.0), 2147483647.0); }

// the fixed-point source coordinates (X0[y] + adelta[x], Y0[y] + bdelta[x]) of output pixel (x, y) under the inverse map m (6 doubles);
// false where m holds a NaN (no box)
__device__ __forceinline__ bool warp_fixed(const double* __restrict__ m, int x, int y, int rd, int& X, int& Y) {
#pragma clang fp contract(off)
  const double a00 = m[0], a01 = m[1], b0 = m[2], a10 = m[3], a11 = m[4], b1 = m[5];
  if (a00 != a00 || a01 != a01 || b0 != b0 || a10 != a10 || a11 != a11 || b1 != b1) return false;
  const double dx = (double)x, dy = (double)y;
  const int adelta = warp_sat_rint(a00 * dx * 1024.0), bdelta = warp_sat_rint(a10 * dx * 1024.0);
  const double px = a01 * dy, py = a11 * dy;
  const int X0 = warp_sat_rint((px + b0) * 1024.0), Y0 = warp_sat_rint((py + b1) * 1024.0);
  X = (int)((uint32_t)X0 + (uint32_t)rd + (uint32_t)adelta);          // int32 sums, wrapping as OpenCV's do
  Y = (int)((uint32_t)Y0 + (uint32_t)rd + (uint32_t)bdelta);
  return true;
}

struct WarpParams {
  const uint8_t* images; const double* inv; const int32_t* img_idx; uint8_t* out;
  int n_img, H, W, B, out_h, out_w, interp;
};

// acc[c] += w * image pixel (sy, sx), nothing for a tap outside the frame or of weight 0
template <int C>
__device__ __forceinline__ void warp_tap(const uint8_t* __restrict__ img, int H, int W, int sy, int sx, int w, int* acc) {
  if (w == 0 || (unsigned)sx >= (unsigned)W || (unsigned)sy >= (unsigned)H) return;
  const size_t o = ((size_t)sy * W + sx) * C;
  if constexpr (C == 4) {
    const uint32_t d = *reinterpret_cast<const uint32_t*>(img + o);
    acc[0] += w * (int)(d & 255u); acc[1] += w * (int)((d >> 8) & 255u); acc[2] += w * (int)((d >> 16) & 255u); acc[3] += w * (int)(d >> 24);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += w * (int)img[o + c];
  }
}

template <int C>
__global__ __launch_bounds__(256) void warp_affine_u8_kernel(const WarpParams p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // over B * out_h * out_w
  const size_t per = (size_t)p.out_h * p.out_w;
  if (i >= (size_t)p.B * per) return;
  const int x = (int)(i % p.out_w);
  const int y = (int)((i / p.out_w) % p.out_h);
  const int b = (int)(i / per);
  const int im = p.img_idx ? p.img_idx[b] : (p.n_img == 1 ? 0 : b);
  int acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0;
  int X, Y;
  if (im >= 0 && im < p.n_img && warp_fixed(p.inv + 6 * (size_t)b, x, y, p.interp == 0 ? 512 : 16, X, Y)) {
    const uint8_t* img = p.images + (size_t)im * p.H * p.W * C;
    if (p.interp == 0) {
      warp_tap<C>(img, p.H, p.W, Y >> 10, X >> 10, 1, acc);
    } else {
      X >>= 5; Y >>= 5;
      const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
      warp_tap<C>(img, p.H, p.W, sy, sx, (32 - fy) * (32 - fx) * 32, acc);
      warp_tap<C>(img, p.H, p.W, sy, sx + 1, (32 - fy) * fx * 32, acc);
      warp_tap<C>(img, p.H, p.W, sy + 1, sx, fy * (32 - fx) * 32, acc);
      warp_tap<C>(img, p.H, p.W, sy + 1, sx + 1, fy * fx * 32, acc);
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = (acc[c] + 16384) >> 15;
    }
  }
  uint8_t* o = p.out + i * C;
  if constexpr (C == 4) {
    *reinterpret_cast<uint32_t*>(o) = (uint32_t)acc[0] | ((uint32_t)acc[1] << 8) | ((uint32_t)acc[2] << 16) | ((uint32_t)acc[3] << 24);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (uint8_t)acc[c];
  }
}

// the checks the two entry points share
static int warp_args(const void* src, int n_img, int H, int W, int C, const double* inv_mats, const int32_t* img_idx, const uint8_t* out,
                     int B, int out_h, int out_w) {
  if (!src || !inv_mats || !out || n_img <= 0 || H <= 0 || W <= 0 || C <= 0 || C > 4 || B <= 0 || out_h <= 0 || out_w <= 0) return CP_ERR_INVALID;
  if (!img_idx && n_img != 1 && n_img != B) return CP_ERR_INVALID;          // which image does crop b come from?
  if (cp_misaligned(inv_mats, 7) || cp_misaligned(img_idx, 3)) return CP_ERR_ALIGN;
  if ((size_t)n_img * H * W * C >= ((size_t)1 << 40) || (size_t)H * W >= ((size_t)1 << 31)) return CP_ERR_RANGE;
  if ((size_t)out_h * out_w >= ((size_t)1 << 31) || ((size_t)B * out_h * out_w + 255) / 256 >= ((size_t)1 << 31)) return CP_ERR_RANGE;
  return CP_OK;
}

extern "C" int cp_warp_affine_u8(cp_stream_t stream, const uint8_t* images, int n_img, int H, int W, int C, const double* inv_mats,
                                 const int32_t* img_idx, uint8_t* out, int B, int out_h, int out_w, int interpolation) {
  if (interpolation != 0 && interpolation != 1) return CP_ERR_INVALID;
  const int rc = warp_args(images, n_img, H, W, C, inv_mats, img_idx, out, B, out_h, out_w);
  if (rc != CP_OK) return rc;
  if (C == 4 && (cp_misaligned(images, 3) || cp_misaligned(out, 3))) return CP_ERR_ALIGN;      // dword taps and stores
  WarpParams p;
  p.images = images; p.inv = inv_mats; p.img_idx = img_idx; p.out = out;
  p.n_img = n_img; p.H = H; p.W = W; p.B = B; p.out_h = out_h; p.out_w = out_w; p.interp = interpolation;
  const dim3 grid((unsigned)(((size_t)B * out_h * out_w + 255) / 256)), block(256);
  switch (C) {
    case 1: CP_LAUNCH(warp_affine_u8_kernel<1>, grid, block, 0, (hipStream_t)stream, p); break;
    case 2: CP_LAUNCH(warp_affine_u8_kernel<2>, grid, block, 0, (hipStream_t)stream, p); break;
    case 3: CP_LAUNCH(warp_affine_u8_kernel<3>, grid, block, 0, (hipStream_t)stream, p); break;
    default: CP_LAUNCH(warp_affine_u8_kernel<4>, grid, block, 0, (hipStream_t)stream, p); break;
  }
  return cp_check_launch();
}

struct WarpBitsParams {
  const uint32_t* plane; const double* inv; const int32_t* img_idx; const int32_t* bit; uint8_t* out;
  int n_img, H, W, B, out_h, out_w;
};

__global__ __launch_bounds__(256) void warp_mask_bits_kernel(const WarpBitsParams p) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // over B * out_h * out_w
  const size_t per = (size_t)p.out_h * p.out_w;
  if (i >= (size_t)p.B * per) return;
  const int x = (int)(i % p.out_w);
  const int y = (int)((i / p.out_w) % p.out_h);
  const int b = (int)(i / per);
  const int im = p.img_idx ? p.img_idx[b] : (p.n_img == 1 ? 0 : b);
  const int bit = p.bit[b];
  uint8_t v = 0;
  int X, Y;
  if (im >= 0 && im < p.n_img && bit >= 0 && bit < 32 && warp_fixed(p.inv + 6 * (size_t)b, x, y, 512, X, Y)) {
    const int sx = X >> 10, sy = Y >> 10;
    if ((unsigned)sx < (unsigned)p.W && (unsigned)sy < (unsigned)p.H)
      v = ((p.plane[((size_t)im * p.H + sy) * p.W + sx] >> bit) & 1u) ? 255 : 0;
  }
  p.out[i] = v;
}

extern "C" int cp_warp_mask_bits(cp_stream_t stream, const uint32_t* plane, int n_img, int H, int W, const double* inv_mats,
                                 const int32_t* img_idx, const int32_t* bit, uint8_t* out, int B, int out_h, int out_w) {
  if (!bit) return CP_ERR_INVALID;
  const int rc = warp_args(plane, n_img, H, W, 4, inv_mats, img_idx, out, B, out_h, out_w);
  if (rc != CP_OK) return rc;
  if (cp_misaligned(plane, 3) || cp_misaligned(bit, 3)) return CP_ERR_ALIGN;
  WarpBitsParams p;
  p.plane = plane; p.inv = inv_mats; p.img_idx = img_idx; p.bit = bit; p.out = out;
  p.n_img = n_img; p.H = H; p.W = W; p.B = B; p.out_h = out_h; p.out_w = out_w;
  CP_LAUNCH(warp_mask_bits_kernel, dim3((unsigned)(((size_t)B * out_h * out_w + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}
