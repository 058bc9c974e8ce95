// Training-frame augmentation on the device, SURVEY.md 8f row N13: the LM loader's background swap (lm_dataset_pytorch.py:523-541
// replace_bg) and the colour chain of GDR_Net_Augmentation.build_augmentations (:161-178) for a whole batch in ONE launch, from
// frames, masks and a background pool that are already in HBM.  Everything random or floating-point is decided on the host and
// arrives as a plan (checkerpose_amd/augment.py: sample_plan); the kernel is integer work on bytes, bit-exact against the numpy
// restatement tests/augment_stages.py.  Parity with imgaug itself is UNPINNED (imgaug / cv2 are not available to compare with).
//
// Per sample, every step yielding uint8 before the next (out-of-frame neighbours of the two blurs: BORDER_REFLECT_101 of the
// step's own input image):
//   1 background   bg_index >= 0: pixel = mask != 0 ? frame : background[bg_index]
//   2 salt+pepper  hash(key, 1, y, x) < sp_thresh: all channels = table[hash(key, 2, y, x) >> 24] (the arcsine-law table of the plan)
//   3 motion blur  25 integer taps summing to 65536 (correlation, row-major 5 x 5): (acc + 32768) >> 16
//   4 dropout      cell (cy, cx) = (min(y * gh / H, gh - 1), min(x * gw / W, gw - 1)) in exact integers (what the project's
//                  INTER_NEAREST rule gives in double); all channels 0 where hash(key, 3, cy, cx) < drop_thresh
//   5 Gaussian     separable 5 taps summing to 4096: the horizontal pass keeps the exact sum, the vertical pass gives
//                  (acc + (1 << 23)) >> 24 (acc <= 255 * 2^24 and acc + 2^23 < 2^32: unsigned 32-bit arithmetic holds what the
//                  statement's 64-bit accumulator holds)
//   6 LUT          one 256-entry table per channel (Add, Invert, Multiply, Multiply, Contrast composed on the host)
//
// hash(key, op, a, b) -- a fixed 32-bit mixer over ABSOLUTE frame coordinates (never tile or launch positions), murmur3's finaliser
// fmix32(h) = { h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16 } applied three times:
//   s = fmix32(key ^ (op * 0x9E3779B9));  t = fmix32(s ^ (a * 0x85EBCA6B + 0x165667B1));  hash = fmix32(t ^ (b * 0xC2B2AE35 + 0x27D4EB2F))
// all in uint32 arithmetic; (a, b) = (y, x) for salt-and-pepper, (cy, cx) for the dropout.
//
// Plan blob (device, one upload per call): 256 bytes of salt-and-pepper values, then per sample 944 bytes = 44 int32 words
// [key, flags, bg_index, img_index, sp_thresh, drop_thresh, gh, gw, rect x1 y1 x2 y2, gauss_w 5, motion_w 25, 2 spare] + the LUT
// uint8 (3, 256).  flags: 1 salt-and-pepper, 2 motion, 4 dropout, 8 Gaussian, 16 LUT is not the identity, 32 rect given.
//
// One workgroup per (sample, 64 x 32 tile).  The tile plus the halo its switched-on blurs need (motion 2 + Gaussian 2) of the image
// after steps 1-2 is staged in LDS as interleaved bytes (a row is a byte stream: the horizontal neighbour is 3 bytes away, so the
// passes never look at channels), REFLECT_101 resolved at load time on absolute coordinates; steps 3-5 run LDS -> LDS with the halo
// shrinking.  A blur's output is only formed INSIDE the frame; where the Gaussian's halo leaves the frame the values are copied from
// their mirror positions first (a convolution's output beyond the border is not the mirror of its output inside for an asymmetric
// kernel, so the mirror is taken of the finished step, as the statement has it).  A stage that is off is skipped by a branch on the
// sample's flags (uniform per workgroup).  LDS: 2 x 8,640 B images + 768 B LUT + cell tables = 18.3 KB, 8 workgroups per CU = the
// 32-wave cap; lanes of a wave read consecutive bytes of a row (four lanes per dword, no bank conflict).  The output leaves as
// dwords when rows are 4-byte aligned (W * 3 % 4 == 0), else as bytes.  Tiles that miss a sample's rect leave at once.
#include "common.h"

namespace {
constexpr int TW = 64, TH = 32, HALO = 4;
constexpr int RW = TW + 2 * HALO;                // 72 pixels per staged row
constexpr int RS = RW * 3;                       // 216 bytes
constexpr int RH = TH + 2 * HALO;                // 40 rows
constexpr int TB = TW * 3;                       // 192 bytes per tile row
constexpr int HEAD_BYTES = 256, REC_WORDS = 44, REC_BYTES = REC_WORDS * 4 + 768;
enum { F_SP = 1, F_MOTION = 2, F_DROP = 4, F_GAUSS = 8, F_LUT = 16, F_RECT = 32 };

struct AugParams {
  const uint8_t* frames; const uint8_t* masks; const uint8_t* bgs; const uint8_t* plan; uint8_t* out;
  int n_img, n_bg, H, W, tiles_x, ntile, vec4;
};

__device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
__device__ __forceinline__ uint32_t aug_seed(uint32_t key, uint32_t op) { return fmix32(key ^ (op * 0x9E3779B9u)); }
__device__ __forceinline__ uint32_t aug_hash(uint32_t seed, int a, int b) {
  const uint32_t t = fmix32(seed ^ ((uint32_t)a * 0x85EBCA6Bu + 0x165667B1u));
  return fmix32(t ^ ((uint32_t)b * 0xC2B2AE35u + 0x27D4EB2Fu));
}
// BORDER_REFLECT_101 for p in [-4, n + 3], n >= 5
__device__ __forceinline__ int r101(int p, int n) {
  p = p < 0 ? -p : p;
  return p >= n ? 2 * n - 2 - p : p;
}
}  // namespace

__global__ __launch_bounds__(256) void augment_frames_kernel(const AugParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t bufA[RH * RS];
  __shared__ __attribute__((aligned(16))) uint8_t bufB[RH * RS];
  __shared__ __attribute__((aligned(16))) uint8_t lut[768];
  __shared__ int16_t celly[RH], cellx[RW];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / p.ntile, t = blockIdx.x - b * p.ntile;
  const int ty = t / p.tiles_x;
  const int x0 = (t - ty * p.tiles_x) * TW, y0 = ty * TH;
  const int H = p.H, W = p.W;
  const uint8_t* recb = p.plan + HEAD_BYTES + (size_t)b * REC_BYTES;
  const int32_t* rec = (const int32_t*)recb;
  const int flags = rec[1];
  const int vw = min(TW, W - x0), vh = min(TH, H - y0);
  if ((flags & F_RECT) && (rec[10] <= rec[8] || rec[11] <= rec[9] || x0 >= rec[10] || x0 + vw <= rec[8] || y0 >= rec[11] || y0 + vh <= rec[9]))
    return;                                                 // an empty rect, or one this tile does not meet
  const int im = rec[3], bgi = rec[2];
  if (im < 0 || im >= p.n_img) return;
  const uint32_t key = (uint32_t)rec[0];
  const size_t fpix = (size_t)H * W;
  const uint8_t* frame = p.frames + (size_t)im * fpix * 3;
  const bool swap = bgi >= 0 && bgi < p.n_bg && p.masks && p.bgs;
  const uint8_t* mask = swap ? p.masks + (size_t)im * fpix : nullptr;
  const uint8_t* bgimg = swap ? p.bgs + (size_t)bgi * fpix * 3 : nullptr;
  const int hg = (flags & F_GAUSS) ? 2 : 0, hl = hg + ((flags & F_MOTION) ? 2 : 0);

  if ((flags & F_LUT) && tid < 192) ((uint32_t*)lut)[tid] = ((const uint32_t*)(recb + REC_WORDS * 4))[tid];

  // ---- steps 1-2 while staging: the tile and the halo the switched-on blurs need, mirrored on absolute coordinates
  {
    const bool sp = flags & F_SP;
    const uint32_t s_hit = aug_seed(key, 1), s_val = aug_seed(key, 2), sp_thresh = (uint32_t)rec[4];
    const int rlo = HALO - hl, rhi = HALO + vh + hl, clo = HALO - hl, chi = HALO + vw + hl;
    for (int i = tid; i < RH * RW; i += 256) {
      const int ry = i / RW, rx = i - ry * RW;
      if (ry < rlo || ry >= rhi || rx < clo || rx >= chi) continue;
      const int y = r101(y0 - HALO + ry, H), x = r101(x0 - HALO + rx, W);
      const size_t pix = (size_t)y * W + x;
      const uint8_t* src = frame + pix * 3;
      if (swap && mask[pix] == 0) src = bgimg + pix * 3;
      uint8_t c0 = src[0], c1 = src[1], c2 = src[2];
      if (sp && aug_hash(s_hit, y, x) < sp_thresh) c0 = c1 = c2 = p.plan[aug_hash(s_val, y, x) >> 24];
      uint8_t* d = bufA + ry * RS + rx * 3;
      d[0] = c0; d[1] = c1; d[2] = c2;
    }
  }
  uint8_t* cur = bufA;
  uint8_t* oth = bufB;
  __syncthreads();

  // what steps 3-4 produce: the part of tile + Gaussian halo that lies inside the frame (rows [rlo, rhi), byte columns [clo, chi))
  const int rlo = max(HALO - hg, HALO - y0), rhi = min(HALO + vh + hg, HALO + H - y0);
  const int plo = max(HALO - hg, HALO - x0), phi = min(HALO + vw + hg, HALO + W - x0);

  if (flags & F_MOTION) {                                   // ---- step 3
    int w[25];
#pragma unroll
    for (int k = 0; k < 25; ++k) w[k] = rec[17 + k];
    const int clo = plo * 3, chi = phi * 3;
    for (int i = tid; i < RH * RS; i += 256) {
      const int ry = i / RS, cb = i - ry * RS;
      if (ry < rlo || ry >= rhi || cb < clo || cb >= chi) continue;
      const uint8_t* s = cur + i;
      int acc = 32768;
#pragma unroll
      for (int dy = 0; dy < 5; ++dy)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) acc += w[dy * 5 + dx] * (int)s[(dy - 2) * RS + (dx - 2) * 3];
      oth[i] = (uint8_t)(acc >> 16);
    }
    uint8_t* x = cur; cur = oth; oth = x;
    __syncthreads();
  }

  if (flags & F_DROP) {                                     // ---- step 4, in place
    const int gh = max(rec[6], 1), gw = max(rec[7], 1);
    if (tid < RH) {
      const int y = min(max(y0 - HALO + tid, 0), H - 1);
      celly[tid] = (int16_t)min((int)(((long long)y * gh) / H), gh - 1);
    } else if (tid >= 64 && tid < 64 + RW) {
      const int x = min(max(x0 - HALO + tid - 64, 0), W - 1);
      cellx[tid - 64] = (int16_t)min((int)(((long long)x * gw) / W), gw - 1);
    }
    __syncthreads();
    const uint32_t s_drop = aug_seed(key, 3), thresh = (uint32_t)rec[5];
    for (int i = tid; i < RH * RW; i += 256) {
      const int ry = i / RW, rx = i - ry * RW;
      if (ry < rlo || ry >= rhi || rx < plo || rx >= phi) continue;
      if (aug_hash(s_drop, celly[ry], cellx[rx]) < thresh) {
        uint8_t* d = cur + ry * RS + rx * 3;
        d[0] = 0; d[1] = 0; d[2] = 0;
      }
    }
    __syncthreads();
  }

  if (flags & F_GAUSS) {                                    // ---- step 5
    if (y0 < 2 || x0 < 2 || y0 + vh + 2 > H || x0 + vw + 2 > W) {      // the halo leaves the frame: mirror the finished step 4 image
      for (int i = tid; i < RH * RW; i += 256) {
        const int ry = i / RW, rx = i - ry * RW;
        if (ry < HALO - 2 || ry >= HALO + vh + 2 || rx < HALO - 2 || rx >= HALO + vw + 2) continue;
        const int y = y0 - HALO + ry, x = x0 - HALO + rx;
        if (y >= 0 && y < H && x >= 0 && x < W) continue;
        const uint8_t* s = cur + (r101(y, H) - (y0 - HALO)) * RS + (r101(x, W) - (x0 - HALO)) * 3;
        uint8_t* d = cur + ry * RS + rx * 3;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
      }
      __syncthreads();
    }
    const uint32_t g0 = (uint32_t)rec[12], g1 = (uint32_t)rec[13], g2 = (uint32_t)rec[14], g3 = (uint32_t)rec[15], g4 = (uint32_t)rec[16];
    if (tid < vw * 3) {                                     // a thread per byte column, five horizontal sums kept in registers
      const uint8_t* s = cur + HALO * 3 + tid;
      uint8_t* d = oth + HALO * 3 + tid;
      uint32_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;
      for (int r = HALO - 2; r < HALO + vh + 2; ++r) {
        const uint8_t* q = s + r * RS;
        const uint32_t h4 = g0 * q[-6] + g1 * q[-3] + g2 * q[0] + g3 * q[3] + g4 * q[6];
        if (r >= HALO + 2) d[(r - 2) * RS] = (uint8_t)((g0 * h0 + g1 * h1 + g2 * h2 + g3 * h3 + g4 * h4 + (1u << 23)) >> 24);
        h0 = h1; h1 = h2; h2 = h3; h3 = h4;
      }
    }
    uint8_t* x = cur; cur = oth; oth = x;
    __syncthreads();
  }

  // ---- step 6 on the way out
  const bool use_lut = flags & F_LUT;
  uint8_t* outp = p.out + ((size_t)b * fpix + (size_t)y0 * W + x0) * 3;
  if (p.vec4) {                                             // rows are 4-byte aligned: vw * 3 is a multiple of 4 too
    const int nd = (vw * 3) >> 2;
    for (int i = tid; i < vh * (TB / 4); i += 256) {
      const int ry = i / (TB / 4), k = i - ry * (TB / 4);
      if (k >= nd) continue;
      uint32_t v = *(const uint32_t*)(cur + (HALO + ry) * RS + HALO * 3 + 4 * k);
      if (use_lut) {
        const int c0 = k % 3, c1 = c0 == 2 ? 0 : c0 + 1, c2 = c1 == 2 ? 0 : c1 + 1;      // byte 4 k + m is channel (k + m) % 3
        v = (uint32_t)lut[c0 * 256 + (v & 255)] | ((uint32_t)lut[c1 * 256 + ((v >> 8) & 255)] << 8) |
            ((uint32_t)lut[c2 * 256 + ((v >> 16) & 255)] << 16) | ((uint32_t)lut[c0 * 256 + (v >> 24)] << 24);
      }
      *(uint32_t*)(outp + (size_t)ry * W * 3 + 4 * k) = v;
    }
  } else {
    const int nb = vw * 3;
    for (int i = tid; i < vh * TB; i += 256) {
      const int ry = i / TB, cb = i - ry * TB;
      if (cb >= nb) continue;
      uint8_t v = cur[(HALO + ry) * RS + HALO * 3 + cb];
      if (use_lut) v = lut[(cb % 3) * 256 + v];
      outp[(size_t)ry * W * 3 + cb] = v;
    }
  }
}

extern "C" size_t cp_augment_plan_bytes(int B) { return B > 0 ? (size_t)HEAD_BYTES + (size_t)B * REC_BYTES : 0; }

extern "C" int cp_augment_frames(cp_stream_t stream, const uint8_t* frames, int n_img, int H, int W, const uint8_t* masks,
                                 const uint8_t* backgrounds, int n_bg, const void* plan, int B, uint8_t* out) {
  if (!frames || !plan || !out || n_img <= 0 || B <= 0 || n_bg < 0 || H < 5 || W < 5) return CP_ERR_INVALID;
  if ((n_bg > 0) != (backgrounds != nullptr)) return CP_ERR_INVALID;
  if (!cp_aligned16(plan)) return CP_ERR_ALIGN;
  if ((size_t)H * W >= ((size_t)1 << 31) || H >= (1 << 15) || W >= (1 << 15)) return CP_ERR_RANGE;      // (cells are stored as int16)
  AugParams p;
  p.frames = frames; p.masks = masks; p.bgs = backgrounds; p.plan = (const uint8_t*)plan; p.out = out;
  p.n_img = n_img; p.n_bg = n_bg; p.H = H; p.W = W;
  p.tiles_x = (W + TW - 1) / TW;
  p.ntile = p.tiles_x * ((H + TH - 1) / TH);
  p.vec4 = ((W * 3) % 4 == 0 && (((uintptr_t)out) & 3u) == 0) ? 1 : 0;
  const size_t blocks = (size_t)B * p.ntile;
  if (blocks >= ((size_t)1 << 31)) return CP_ERR_RANGE;
  CP_LAUNCH(augment_frames_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}
