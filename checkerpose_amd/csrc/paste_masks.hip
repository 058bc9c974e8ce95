// cp_paste_* (SURVEY.md 8f row N27): the network's predicted masks -- `seg` (B, 2, Sh, Sw) fp32 logits, channel 0 the visible and
// channel 1 the full mask, at crop resolution -- pasted back into their photograph, straight into the operands of row N15
// (csrc/coco_eval.hip): PackedMasks bit rows (cp_paste_masks) or the column-major RLE (cp_paste_rle_count / cp_paste_rle_write).
// No dense mask exists anywhere.  The reference never pastes a mask; the rule is the project's OWN:
//
// THE RULE.  It is the geometric inverse of the crop of rows N2 / N3 and uses integers only.  For mask b take its window
// (x1, y1, x2, y2, rw, rh) -- exactly what preprocess._windows / roi_window give cp_crop_resize_u8 for the same (already padded) box and
// resize_method --, a seg plane of Sh x Sw logits and a frame of H x W pixels.  Frame pixel (y, x) is set if and only if
//   * rw > 0 and rh > 0;
//   * max(x1, 0) <= x < min(x2, W, x1 + rw), and max(y1, 0) <= y < min(y2, H, y1 + rh): where the crop read a real pixel (the
//     adjoint of crop_nearest_src's domain, preprocess.hip; zero padding excluded);
//   * with rx = x - x1, ry = y - y1, cx = ((2 rx + 1) Sw) / (2 rw) and cy = ((2 ry + 1) Sh) / (2 rh) in INTEGER division, the logit
//     seg[cy, cx] passes cp_sigmoid_gt_half (common.h: z > 1.5 * 2^-24, the pinned fp32 `sigmoid(z) > 0.5`; NaN, -0.0, +0.0 fail).
// Pixel CENTRES, not cv2.INTER_NEAREST's left edges floor(rx Sw / rw) (cp_crop_mask_bits restates those for the forward crop): the
// correspondences' coordinate grid and the INTER_LINEAR crop are centre-aligned, and the mask has to land where the p2d land.
// INTEGERS, not float: torch's "nearest-exact" is the same rule in float and differs wherever (2 rx + 1) Sw / (2 rw) is an integer
// (Sw = 64, rw = 41: index 20 reads cell 31 instead of 32).  (2 rx + 1) Sw < 2^40: 64-bit, 32-bit where rw < 2^22.
//
//   paste_masks_kernel   a 256-thread workgroup per mask.  (1) the Sh x Sw logits are thresholded with coalesced loads and wave
//                        ballots into an LDS bit table (2 * ceil(Sw / 64) words per cell row, <= 2 KB); the cell of every window
//                        column / row goes into two byte tables (a division per column and row, not per pixel).  (2) ALL frame rows
//                        that map to one cell row are identical: the finished output row of WW = ceil(W / 32) words is built once per
//                        cell row in LDS (<= Sh x WW words: 64 KB at the limits), with its popcount and first / last set column.
//                        (3) the H rows stream out as plain coalesced 32-bit vector stores of the pattern row cy(y), zeros outside
//                        the window's rows: every word is written (the buffer arrives uninitialised), bits past W are zero.  Area
//                        and box: the pattern rows' popcounts over the window's rows, reduced by wave shuffles and LDS.
//   paste_rle_kernel     a 512-thread workgroup per mask; work proportional to the WINDOW, no frame-sized bits are stored or read.
//                        pycoco_utils.binary_mask_to_rle ravels column-major (i = x H + y; runs go on across the column boundary; a
//                        leading 0 when pixel 0 is set).  A run START is a pixel unlike its predecessor (or pixel 0).  Outside the
//                        window everything is clear, so starts lie only AT window pixels (unlike their predecessor, which is read
//                        through the same rule) and DIRECTLY AFTER a set pixel that ends its column's stretch of the window when the
//                        pixel after it is no window pixel.  Every thread owns a contiguous stretch of the window's pixels in column-
//                        major order and meets its starts in ascending i; cp_scan_sum_max (coco_rle_kernel's block scan) places
//                        them.  The count launch also sums area and box.  Offsets contract as cp_coco_rle_write.
//
// No atomics, no scratch memory; every output is a function of the mask's own logits and window: bit-identical alone or at any batch
// position.  Equal to cp_coco_pack / cp_coco_rle_* of the dense pasted mask by construction of the rule (tests/paste_stages.py).
#include <limits.h>

#include "common.h"

namespace {

constexpr int PM_THREADS = 256, PM_RLE_THREADS = 512, PM_SMAX = 128, PM_FMAX = 4096;

struct PmGeom { int lx, hx, ly, hy; long long x1, y1, rw, rh; };      // the window's pixels [lx, hx) x [ly, hy): empty as 0, 0, 0, 0

__device__ __forceinline__ PmGeom pm_geom(const int32_t* __restrict__ w, int H, int W) {
  PmGeom g;
  g.x1 = w[0]; g.y1 = w[1]; g.rw = w[4]; g.rh = w[5];
  g.lx = g.hx = g.ly = g.hy = 0;
  if (g.rw > 0 && g.rh > 0) {
    const long long lx = max(g.x1, 0LL), hx = min(min((long long)w[2], (long long)W), g.x1 + g.rw);
    const long long ly = max(g.y1, 0LL), hy = min(min((long long)w[3], (long long)H), g.y1 + g.rh);
    if (hx > lx && hy > ly) { g.lx = (int)lx; g.hx = (int)hx; g.ly = (int)ly; g.hy = (int)hy; }
  }
  return g;
}

// ((2 r + 1) S) / (2 n) for 0 <= r < n, S <= 128: the cell of window offset r, < S
__device__ __forceinline__ int pm_cell(long long r, int S, long long n) {
  if (n < (1LL << 22)) return (int)((uint32_t)((2 * r + 1) * S) / (uint32_t)(2 * n));
  return (int)((unsigned long long)((2 * r + 1) * S) / (unsigned long long)(2 * n));
}

// the thresholded plane as bits: word 2 c + h of cell row y holds cells 64 c + 32 h .. + 31 (SWW = 2 * ceil(Sw / 64) words per row)
template <int T>
__device__ __forceinline__ void pm_threshold(const float* __restrict__ z, int Sh, int Sw, uint32_t* __restrict__ s_bt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, chunks = (Sw + 63) >> 6;
  for (int it = wave; it < Sh * chunks; it += T / 64) {                // (uniform per wave)
    const int y = it / chunks, c = it - y * chunks, x = c * 64 + lane;
    const bool set = x < Sw && cp_sigmoid_gt_half(z[(size_t)y * Sw + x]);
    const unsigned long long bal = __ballot(set);
    if (lane == 0) { s_bt[(y * chunks + c) * 2] = (uint32_t)bal; s_bt[(y * chunks + c) * 2 + 1] = (uint32_t)(bal >> 32); }
  }
}

template <int T>
__device__ __forceinline__ void pm_cell_tables(const PmGeom& g, int Sh, int Sw, uint8_t* __restrict__ s_cx, uint8_t* __restrict__ s_cy) {
  for (int x = g.lx + (int)threadIdx.x; x < g.hx; x += T) s_cx[x] = (uint8_t)pm_cell(x - g.x1, Sw, g.rw);
  for (int y = g.ly + (int)threadIdx.x; y < g.hy; y += T) s_cy[y] = (uint8_t)pm_cell(y - g.y1, Sh, g.rh);
}

// (area, xmin, ymin, xmax, ymax) over the workgroup -> area[n], box[4 n ..]; s: a row per wave
template <int T>
__device__ __forceinline__ void pm_area_box(int cnt, int x0, int y0, int x1, int y1, int (*s)[5], int32_t* __restrict__ area,
                                            int32_t* __restrict__ box, int n) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    cnt += __shfl_xor(cnt, w, 64);
    x0 = min(x0, __shfl_xor(x0, w, 64)); y0 = min(y0, __shfl_xor(y0, w, 64));
    x1 = max(x1, __shfl_xor(x1, w, 64)); y1 = max(y1, __shfl_xor(y1, w, 64));
  }
  if (lane == 0) { s[wave][0] = cnt; s[wave][1] = x0; s[wave][2] = y0; s[wave][3] = x1; s[wave][4] = y1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < T / 64; ++w) {
      cnt += s[w][0]; x0 = min(x0, s[w][1]); y0 = min(y0, s[w][2]); x1 = max(x1, s[w][3]); y1 = max(y1, s[w][4]);
    }
    area[n] = cnt;
    box[4 * n] = cnt ? x0 : -1; box[4 * n + 1] = cnt ? y0 : -1; box[4 * n + 2] = cnt ? x1 : -1; box[4 * n + 3] = cnt ? y1 : -1;
  }
}

// ---- bits
// the LDS carve of paste_masks_kernel, in bytes, every offset a multiple of 16
struct PmCarve { size_t pat, bt, cx, cy, rows, red, total; };
__host__ __device__ inline PmCarve pm_carve(int Sh, int Sw, int H, int W) {
  auto up = [](size_t n) { return (n + 15) & ~(size_t)15; };
  PmCarve c;
  c.pat = 0;
  c.bt = c.pat + up((size_t)Sh * ((W + 31) / 32) * 4);
  c.cx = c.bt + up((size_t)Sh * 2 * ((Sw + 63) / 64) * 4);
  c.cy = c.cx + up((size_t)W);
  c.rows = c.cy + up((size_t)H);
  c.red = c.rows + up((size_t)Sh * 3 * 4);
  c.total = c.red + up((size_t)(PM_THREADS / 64) * 5 * 4);
  return c;
}

__global__ __launch_bounds__(PM_THREADS) void paste_masks_kernel(const float* __restrict__ seg, long long seg_bstride, int Sh, int Sw,
                                                                 const int32_t* __restrict__ windows, int H, int W, int WW,
                                                                 uint32_t* __restrict__ bits, int32_t* __restrict__ area,
                                                                 int32_t* __restrict__ box) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pm_lds[];
  const PmCarve cv = pm_carve(Sh, Sw, H, W);
  uint32_t* __restrict__ s_pat = (uint32_t*)(pm_lds + cv.pat);         // (Sh, WW): the output row of every cell row
  uint32_t* __restrict__ s_bt = (uint32_t*)(pm_lds + cv.bt);
  uint8_t* __restrict__ s_cx = pm_lds + cv.cx;
  uint8_t* __restrict__ s_cy = pm_lds + cv.cy;
  int* __restrict__ s_rows = (int*)(pm_lds + cv.rows);                 // (Sh, 3): popcount, first and last set column of the pattern row
  int (*s_red)[5] = (int (*)[5])(pm_lds + cv.red);
  const int tid = threadIdx.x, n = blockIdx.x, SWW = 2 * ((Sw + 63) >> 6);
  const PmGeom g = pm_geom(windows + 6 * (size_t)n, H, W);
  pm_threshold<PM_THREADS>(seg + (size_t)n * seg_bstride, Sh, Sw, s_bt);
  pm_cell_tables<PM_THREADS>(g, Sh, Sw, s_cx, s_cy);
  __syncthreads();
  for (int i = tid; i < Sh * WW; i += PM_THREADS) {
    const int r = i / WW, w = i - r * WW, x0 = w * 32, lo = max(g.lx, x0), hi = min(g.hx, x0 + 32);
    uint32_t word = 0;
    for (int x = lo; x < hi; ++x) {
      const int c = s_cx[x];
      word |= ((s_bt[r * SWW + (c >> 5)] >> (c & 31)) & 1u) << (x - x0);
    }
    s_pat[i] = word;
  }
  __syncthreads();
  for (int r = tid; r < Sh; r += PM_THREADS) {
    int pop = 0, first = INT_MAX, last = -1;
    for (int w = g.lx >> 5; w < WW && w * 32 < g.hx; ++w) {
      const uint32_t v = s_pat[r * WW + w];
      if (v) { pop += __popc(v); first = min(first, w * 32 + __ffs((int)v) - 1); last = w * 32 + 31 - __clz((int)v); }
    }
    s_rows[3 * r] = pop; s_rows[3 * r + 1] = first; s_rows[3 * r + 2] = last;
  }
  __syncthreads();
  uint32_t* __restrict__ b = bits + (size_t)n * H * WW;
  for (int i = tid; i < H * WW; i += PM_THREADS) {                      // (H * WW <= 2^19)
    const int y = i / WW, w = i - y * WW;
    b[i] = (y >= g.ly && y < g.hy) ? s_pat[(int)s_cy[y] * WW + w] : 0u;
  }
  int cnt = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
  for (int y = g.ly + tid; y < g.hy; y += PM_THREADS) {
    const int r = s_cy[y], pop = s_rows[3 * r];
    if (pop) { cnt += pop; x0 = min(x0, s_rows[3 * r + 1]); x1 = max(x1, s_rows[3 * r + 2]); y0 = min(y0, y); y1 = max(y1, y); }
  }
  pm_area_box<PM_THREADS>(cnt, x0, y0, x1, y1, s_red, area, box, n);
}

// ---- rle
template <bool WRITE>
__global__ __launch_bounds__(PM_RLE_THREADS) void paste_rle_kernel(const float* __restrict__ seg, long long seg_bstride, int Sh, int Sw,
                                                                   const int32_t* __restrict__ windows, int H, int W,
                                                                   const int64_t* __restrict__ off, int32_t* __restrict__ n_runs,
                                                                   int32_t* __restrict__ area, int32_t* __restrict__ box,
                                                                   int32_t* __restrict__ counts, long long total) {
  __shared__ uint32_t s_bt[PM_SMAX * 4];
  __shared__ uint8_t s_cx[PM_FMAX], s_cy[PM_FMAX];
  __shared__ int s_scan[PM_RLE_THREADS / 64][2];
  __shared__ int s_red[PM_RLE_THREADS / 64][5];
  const int tid = threadIdx.x, mi = blockIdx.x, SWW = 2 * ((Sw + 63) >> 6);
  const PmGeom g = pm_geom(windows + 6 * (size_t)mi, H, W);
  pm_threshold<PM_RLE_THREADS>(seg + (size_t)mi * seg_bstride, Sh, Sw, s_bt);
  pm_cell_tables<PM_RLE_THREADS>(g, Sh, Sw, s_cx, s_cy);
  __syncthreads();
  const int n = H * W;                                               // (<= 2^24: checked by the caller)
  const int hh = g.hy - g.ly, nw = (g.hx - g.lx) * hh;               // the window's pixels, column-major: j = (x - lx) hh + (y - ly)
  const int L = (nw + PM_RLE_THREADS - 1) / PM_RLE_THREADS;
  const int j0 = min(tid * L, nw), j1 = min(j0 + L, nw);
  auto cell = [&](int r, int c) -> int { return (int)((s_bt[r * SWW + (c >> 5)] >> (c & 31)) & 1u); };
  auto value = [&](int i) -> int {                                   // any frame pixel i = x H + y
    const int x = i / H, y = i - x * H;
    return (x >= g.lx && x < g.hx && y >= g.ly && y < g.hy) ? cell(s_cy[y], s_cx[x]) : 0;
  };
  const bool first_in = nw > 0 && g.lx == 0 && g.ly == 0;            // pixel 0 is a window pixel
  const int lead = first_in ? cell(s_cy[0], s_cx[0]) : 0;
  // walks this thread's stretch and calls start(i) for every run start it owns, in ascending i
  auto walk = [&](auto&& start, auto&& pixel) {
    if (tid == 0 && !first_in) start(0);                             // pixel 0 outside the window: clear, and a start
    if (j0 >= j1) return;
    int xr = j0 / hh, y = g.ly + (j0 - xr * hh), x = g.lx + xr, c = s_cx[x], prev = 0;
    for (int j = j0; j < j1; ++j) {
      const int i = x * H + y, v = cell(s_cy[y], c);
      if (j == j0 || y == g.ly) prev = i == 0 ? -1 : value(i - 1);
      if (v != prev) start(i);
      if (v) pixel(x, y);
      prev = v;
      if (y == g.hy - 1) {                                           // the last window pixel of its column
        if (v && i + 1 < n && (g.hy < H || g.ly > 0 || x + 1 >= g.hx)) start(i + 1);      // the pixel after it is no window pixel
        y = g.ly; ++x;
        if (x < g.hx) c = s_cx[x];
      } else {
        ++y;
      }
    }
  };
  int cnt = 0, last = -1, ar = 0, bx0 = INT_MAX, by0 = INT_MAX, bx1 = -1, by1 = -1;
  walk([&](int i) { ++cnt; last = i; },
       [&](int x, int y) { ++ar; bx0 = min(bx0, x); bx1 = max(bx1, x); by0 = min(by0, y); by1 = max(by1, y); });
  int ec, el;
  cp_scan_sum_max(cnt, last, ec, el, s_scan);                        // cnt / last are inclusive now
  if (!WRITE) {
    if (tid == PM_RLE_THREADS - 1) n_runs[mi] = cnt + lead;
    pm_area_box<PM_RLE_THREADS>(ar, bx0, by0, bx1, by1, s_red, area, box, mi);
    return;
  }
  const long long base = off[mi], cap = off[mi + 1] - base;
  if (base < 0 || cap < 0 || base + cap > total) return;             // (uniform) offsets that do not fit the buffer: nothing written
  int32_t* __restrict__ out = counts + base;
  int k = ec, prv = el;
  walk([&](int i) {
         if (i == 0) {
           if (lead && cap > 0) out[0] = 0;
         } else {
           const int at = k - 1 + lead;                              // the run that ends here
           if (at < cap) out[at] = i - prv;
         }
         prv = i;
         ++k;
       },
       [](int, int) {});
  if (tid == PM_RLE_THREADS - 1) {
    const int at = cnt - 1 + lead;
    if (at < cap) out[at] = n - last;
  }
}

// the checks every entry point shares (null pointers are the caller's; out_misaligned: its verdict on its own output pointers)
int pm_check(const void* seg, long long seg_bstride, int Sh, int Sw, const void* windows, int B, int H, int W, bool out_misaligned) {
  if (B < 1 || seg_bstride < 0 || Sh < 1 || Sh > PM_SMAX || Sw < 1 || Sw > PM_SMAX || H < 1 || H > PM_FMAX || W < 1 || W > PM_FMAX)
    return CP_ERR_INVALID;
  if (cp_misaligned(seg, 3) || cp_misaligned(windows, 3) || out_misaligned) return CP_ERR_ALIGN;
  if ((long long)H * W >= (1LL << 31) - 512 || B >= (1 << 24)) return CP_ERR_RANGE;
  return CP_OK;
}

}  // namespace

extern "C" int cp_paste_masks(cp_stream_t stream, const float* seg, long long seg_bstride, int Sh, int Sw, const int32_t* windows, int B,
                              int H, int W, uint32_t* bits, int32_t* area, int32_t* box) {
  if (!seg || !windows || !bits || !area || !box) return CP_ERR_INVALID;
  const int rc = pm_check(seg, seg_bstride, Sh, Sw, windows, B, H, W, cp_misaligned(bits, 3) || cp_misaligned(area, 3) || cp_misaligned(box, 3));
  if (rc != CP_OK) return rc;
  static CpDeviceOnce once;
  const int dev = cp_current_device();
  CP_LDS_ATTR_ONCE(once, dev, cp_set_max_lds((const void*)paste_masks_kernel, pm_carve(PM_SMAX, PM_SMAX, PM_FMAX, PM_FMAX).total));
  CP_LAUNCH(paste_masks_kernel, dim3((unsigned)B), dim3(PM_THREADS), pm_carve(Sh, Sw, H, W).total, (hipStream_t)stream, seg, seg_bstride, Sh,
            Sw, windows, H, W, (W + 31) / 32, bits, area, box);
  return cp_check_launch();
}

extern "C" int cp_paste_rle_count(cp_stream_t stream, const float* seg, long long seg_bstride, int Sh, int Sw, const int32_t* windows, int B,
                                  int H, int W, int32_t* n_runs, int32_t* area, int32_t* box) {
  if (!seg || !windows || !n_runs || !area || !box) return CP_ERR_INVALID;
  const int rc = pm_check(seg, seg_bstride, Sh, Sw, windows, B, H, W, cp_misaligned(n_runs, 3) || cp_misaligned(area, 3) || cp_misaligned(box, 3));
  if (rc != CP_OK) return rc;
  CP_LAUNCH(paste_rle_kernel<false>, dim3((unsigned)B), dim3(PM_RLE_THREADS), 0, (hipStream_t)stream, seg, seg_bstride, Sh, Sw, windows, H, W,
            (const int64_t*)nullptr, n_runs, area, box, (int32_t*)nullptr, 0LL);
  return cp_check_launch();
}

extern "C" int cp_paste_rle_write(cp_stream_t stream, const float* seg, long long seg_bstride, int Sh, int Sw, const int32_t* windows, int B,
                                  int H, int W, const int64_t* offsets, int32_t* counts, long long total) {
  if (!seg || !windows || !offsets || !counts) return CP_ERR_INVALID;
  if (total < 1) return CP_ERR_INVALID;
  const int rc = pm_check(seg, seg_bstride, Sh, Sw, windows, B, H, W, cp_misaligned(offsets, 7) || cp_misaligned(counts, 3));
  if (rc != CP_OK) return rc;
  CP_LAUNCH(paste_rle_kernel<true>, dim3((unsigned)B), dim3(PM_RLE_THREADS), 0, (hipStream_t)stream, seg, seg_bstride, Sh, Sw, windows, H, W,
            offsets, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, counts, total);
  return cp_check_launch();
}
