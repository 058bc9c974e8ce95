// cp_verify_poses / cp_select_poses: hypothesis verification of poses against the sensor's depth image on the
// device -- render the candidate, compare it pixel by pixel with what the sensor saw, keep the candidate the sensor supports.  The
// reference does not verify; opt-in, the rule is this project's own (tests/verify_stages.py restates it in numpy).  One more consumer
// of vsd_raster.h's scaffold: the per-pixel classes are counted inside the tile kernel and reduced as integers, no depth frame exists.
//
// The rule, per pose.  D = the pose's depth render over the W x H frame (the render rule is vsd_raster.h's, vs_depth_tile: the bits
// cp_render_depth gives), S = the sensor depth of the pose's image, tau = the pose's tolerance in the meshes' units, converted to
// fp32 ONCE.  Every frame pixel with D > 0 is a model pixel (n_model) and falls in exactly one class:
//   missing    S is not finite or S <= 0                               (the validity test of rows N24 / N25)
//   match      a = |d| <= tau, d = S - D as ONE fp32 subtraction       (no contraction)
//   occluded   d < -tau: the sensor saw something in front of the model, an occluder
//   through    d >  tau: the sensor saw past where the model's surface should be, a free-space violation
// A matching pixel also adds q = min(63, (int)(64.f * (a / tau))) to sum_q: the fp32 division, then the fp32 product, then truncation
// -- the truncated-linear kernel, quantised so that every sum is an integer.  The six sums: n_model n_missing n_match n_occluded
// n_through sum_q.
//
// Score (pose_verify_finish_kernel, fp64 without contraction):
//   fit = n_match - sum_q / 64.0      den = (n_match + n_through) + occlusion_weight * n_occluded      score = fit / den
// score is NaN with ok = 0 when den == 0, or when the pose is not counted at all (its six sums are then 0): a non-finite pose or cam_K,
// a vertex at Z <= 0, an image id outside 0..I-1, a mesh id out of range, an input status of 0 (the solvers' identity fallback, which
// must never win), or a tau that as fp32 is not positive and finite.  occlusion_weight in [0, 1]: 1 counts every measured model pixel
// that does not support the pose against it; a caller who trusts occluders lowers it.
//
// Selection (pose_select_kernel).  Candidates are laid out candidate-major, (C, B).  Per crop the eligible candidate (ok = 1 and a score
// that is not NaN) with the largest score wins, the smallest candidate index on equal scores; candidate 0 when none is eligible.
//
// Launches of cp_verify_poses (four, gt_info.hip's shape):
//   pose_verify_pose_kernel    per pose: P = K' [R | t] (vs_side_init), validity, tau as fp32, the accumulators at their identities.
//   pose_verify_vertex_kernel  per (pose, 256 vertices): screen records (vs_vertex_chunk, cp_render_depth's clip) and the rectangle.
//   pose_verify_tile_kernel    a workgroup per (pose, 32 x 32 frame tile).  A tile the rectangle misses leaves at once (after writing
//                              zeros over its in-frame pixels when labels are asked for).  Otherwise vs_depth_tile, then each lane
//                              classifies its four pixels against S; the six sums go through vs_acc_reduce<6, 6>.  Optionally the
//                              (P, H, W) uint8 label map: 0 none, 1 match, 2 occluded, 3 through, 4 missing.
//   pose_verify_finish_kernel  per pose: the counts, ok, fit, den, score.
// Every output is a function of integer counts: bit-identical from call to call, for a pose alone or in a batch, with or without the
// labels.  No floating-point atomics, no initialised scratch beyond what pose_verify_pose_kernel writes.
#include "vsd_raster.h"

namespace {

// 4-byte words per pose: VsHdr<1> (P rect bad ok) | n_model n_missing n_match n_occluded n_through sum_q | tau (fp32 bits)
using PvH = VsHdr<1>;
constexpr int PV_HDR = 32;
constexpr int PV_ACC = PvH::USER, PV_NACC = 6, PV_TAU = PV_ACC + PV_NACC;
constexpr int PV_CMAX = 64;                      // candidates per crop (cp_select_poses)
enum { PV_NONE = 0, PV_MATCH = 1, PV_OCCLUDED = 2, PV_THROUGH = 3, PV_MISSING = 4 };

struct PvParams {
  VsMesh mesh;
  const double* poses;        // (P, 12)
  const double* K;
  const float* depth;         // (I, H, W): the sensor's
  const int32_t* image_id;    // nullptr: image 0
  const double* tau;          // (P)
  const int32_t* status;      // (P) or nullptr: 0 = not a candidate
  int32_t* counts;            // (P, 6)
  double* score;              // (P)
  double* fit;
  double* den;
  uint8_t* ok;                // (P)
  uint8_t* labels;            // (P, H, W) or nullptr
  int32_t* hdr;               // (P, PV_HDR)
  float4* sv;                 // (P, Vmax)
  double occlusion_weight;
  int k_stride, P, I, H, W, tx, ty, vchunks;
};

__global__ __launch_bounds__(VS_THREADS) void pose_verify_pose_kernel(PvParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  int32_t* __restrict__ h = p.hdr + (size_t)b * PV_HDR;
  const double* __restrict__ K = p.K + (size_t)p.k_stride * b;
  const double* __restrict__ q = p.poses + 12 * (size_t)b;
  bool ok = vs_pose_finite(K, q);
  const int img = p.image_id ? p.image_id[b] : 0;
  ok = ok && img >= 0 && img < p.I;
  int vfirst, V, ffirst, F, m;
  ok = vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m) && ok;
  ok = ok && (!p.status || p.status[b] != 0);
  const float tau = (float)p.tau[b];                                 // the ONE conversion
  ok = ok && tau > 0.f && isfinite(tau);
  vs_side_init(K, 1.0, q, (float*)h + PvH::P(0), h + PvH::RECT(0));
  h[PvH::BAD(0)] = 0;
  h[PvH::OK] = ok ? 1 : 0;
  for (int k = 0; k < PV_NACC; ++k) h[PV_ACC + k] = vs_acc_identity<PV_NACC>(k);
  h[PV_TAU] = __float_as_int(tau);
  for (int k = PV_TAU + 1; k < PV_HDR; ++k) h[k] = 0;
}

__global__ __launch_bounds__(VS_THREADS) void pose_verify_vertex_kernel(PvParams p) {
  int b, s, vc;
  vs_vertex_block(p.vchunks, 1, b, s, vc);
  int32_t* __restrict__ h = p.hdr + (size_t)b * PV_HDR;
  if (!h[PvH::OK]) return;                                           // (uniform; no barrier in this kernel)
  int vfirst, V, ffirst, F, m;
  vs_mesh_rows(p.mesh, b, vfirst, V, ffirst, F, m);
  vs_vertex_chunk((const float*)h + PvH::P(0), p.mesh.verts + 3 * (size_t)vfirst, V, vc, make_float4(-2.f, (float)p.W + 1.f, -2.f, (float)p.H + 1.f),
                  p.sv + (size_t)b * p.mesh.Vmax, h + PvH::RECT(0), h + PvH::BAD(0));
}

__global__ __launch_bounds__(VS_THREADS) void pose_verify_tile_kernel(PvParams p) {
  __shared__ float4 s_tri[VS_CHUNK][4];
  __shared__ int s_n;
  __shared__ int s_red[VS_THREADS / 64][PV_NACC];
  const VsTile c = vs_tile(p.tx, p.ty, 0, 0);
  const int b = c.b, ox = c.ox, oy = c.oy;                           // first pixel: inside the frame (the grid covers the frame alone)
  int32_t* __restrict__ h = p.hdr + (size_t)b * PV_HDR;
  const bool live = h[PvH::OK] && !h[PvH::BAD(0)];
  const bool hit = live && vs_tile_hit(h + PvH::RECT(0), ox, oy);
  const int x = ox + c.lx, H = p.H, W = p.W;
  if (!hit) {                                                        // (uniform)
    if (p.labels) {
#pragma unroll
      for (int k = 0; k < VS_PPL; ++k) {
        const int y = oy + c.y(k);
        if (x < W && y < H) p.labels[((size_t)b * H + y) * W + x] = PV_NONE;
      }
    }
    return;
  }
  float dep[VS_PPL];
  {
    const VsMesh mesh = p.mesh;                                     // (a copy, as in gt_info_tile_kernel)
    int vfirst, V, ffirst, F, m;
    vs_mesh_rows(mesh, b, vfirst, V, ffirst, F, m);
    vs_depth_tile(s_tri, &s_n, p.sv + (size_t)b * mesh.Vmax, mesh.faces + 3 * (size_t)ffirst, F, V, c, dep);
  }

  int acc[PV_NACC];
#pragma unroll
  for (int k = 0; k < PV_NACC; ++k) acc[k] = 0;
  const float tau = __int_as_float(h[PV_TAU]);
  const int img = p.image_id ? p.image_id[b] : 0;                    // (hit, hence a checked id)
  const float* __restrict__ sensor = p.depth + (size_t)img * H * W;
#pragma unroll
  for (int k = 0; k < VS_PPL; ++k) {
#pragma clang fp contract(off)
    const int y = oy + c.y(k);
    if (x >= W || y >= H) continue;
    int lab = PV_NONE;
    const float D = dep[k];
    if (D > 0.f) {
      const float S = sensor[(size_t)y * W + x];
      acc[0] += 1;
      if (!isfinite(S) || !(S > 0.f)) {
        lab = PV_MISSING; acc[1] += 1;
      } else {
        const float d = S - D;
        const float a = fabsf(d);
        if (a <= tau) {
          const float r = a / tau;
          lab = PV_MATCH; acc[2] += 1;
          acc[5] += min(63, (int)(64.f * r));
        } else if (d < -tau) {
          lab = PV_OCCLUDED; acc[3] += 1;
        } else {
          lab = PV_THROUGH; acc[4] += 1;
        }
      }
    }
    if (p.labels) p.labels[((size_t)b * H + y) * W + x] = (uint8_t)lab;
  }
  vs_acc_reduce<PV_NACC, PV_NACC>(acc, s_red, h + PV_ACC);
}

__global__ __launch_bounds__(VS_THREADS) void pose_verify_finish_kernel(PvParams p) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.P) return;
  const int32_t* __restrict__ h = p.hdr + (size_t)b * PV_HDR;
  const bool live = h[PvH::OK] && !h[PvH::BAD(0)];
  int n[PV_NACC];
  for (int k = 0; k < PV_NACC; ++k) {
    n[k] = live ? h[PV_ACC + k] : 0;
    p.counts[PV_NACC * (size_t)b + k] = n[k];
  }
  const double fit = (double)n[2] - (double)n[5] / 64.0;
  const double weighted = p.occlusion_weight * (double)n[3];
  const double den = ((double)n[2] + (double)n[4]) + weighted;
  const bool ok = live && den != 0.0;
  p.fit[b] = fit;
  p.den[b] = den;
  p.score[b] = ok ? fit / den : __longlong_as_double(0x7ff8000000000000LL);
  p.ok[b] = ok ? 1 : 0;
}

struct PsParams {
  const double* score;        // (C, B)
  const uint8_t* ok;          // (C, B) or nullptr: every score that is not NaN is eligible
  int32_t* choice;            // (B)
  int C, B;
};

__global__ __launch_bounds__(VS_THREADS) void pose_select_kernel(PsParams p) {
  const int b = blockIdx.x * VS_THREADS + threadIdx.x;
  if (b >= p.B) return;
  int best = -1;
  double top = 0.0;
  for (int c = 0; c < p.C; ++c) {
    const size_t at = (size_t)c * p.B + b;
    const double s = p.score[at];
    if ((p.ok && !p.ok[at]) || !(s == s)) continue;
    if (best < 0 || s > top) { best = c; top = s; }                  // (strict: the smallest index among equals)
  }
  p.choice[b] = best < 0 ? 0 : best;
}

}  // namespace

extern "C" size_t cp_verify_poses_scratch_bytes(int P, int Vmax) {
  if (P <= 0 || Vmax < 0) return 0;
  return cp_align16_up((size_t)P * PV_HDR * sizeof(int32_t)) + cp_align16_up((size_t)P * Vmax * sizeof(float4));
}

extern "C" int cp_verify_poses(cp_stream_t stream, const double* poses, const double* cam_K, int k_stride, const float* verts,
                               const int32_t* v_offsets, const int32_t* faces, const int32_t* f_offsets, int M, const int32_t* mesh_ids,
                               const float* depth, const int32_t* image_ids, int I, int H, int W, const double* tau,
                               const int32_t* status, double occlusion_weight, int P, int Vmax, int32_t* counts, double* score,
                               double* fit, double* den, uint8_t* ok, uint8_t* labels, void* scratch) {
  PvParams p = {};
  p.mesh = {verts, v_offsets, faces, f_offsets, mesh_ids, M, Vmax};
  if (!poses || !depth || !tau || !counts || !score || !fit || !den || !ok || !scratch) return CP_ERR_INVALID;
  if (vs_mesh_invalid(p.mesh) || vs_view_invalid(cam_K, k_stride, H, W, P) || vs_images_invalid(image_ids, I) ||
      !(occlusion_weight >= 0.0 && occlusion_weight <= 1.0))
    return CP_ERR_INVALID;
  if (cp_misaligned(scratch, 15) || cp_misaligned(poses, 7) || vs_view_misaligned(cam_K) || cp_misaligned(tau, 7) ||
      cp_misaligned(score, 7) || cp_misaligned(fit, 7) || cp_misaligned(den, 7) || vs_mesh_misaligned(p.mesh) ||
      cp_misaligned(depth, 3) || cp_misaligned(image_ids, 3) || cp_misaligned(status, 3) || cp_misaligned(counts, 3))
    return CP_ERR_ALIGN;
  VsGrid g;
  if ((long long)H * W > (1LL << 24) || !vs_grid(W, H, 1, false, P, 1, Vmax, g)) return CP_ERR_RANGE;      // int32 sums: 63 H W must fit
  p.poses = poses; p.K = cam_K; p.k_stride = k_stride; p.depth = depth; p.image_id = image_ids; p.I = I; p.H = H; p.W = W;
  p.tau = tau; p.status = status; p.occlusion_weight = occlusion_weight; p.P = P; p.counts = counts; p.score = score; p.fit = fit;
  p.den = den; p.ok = ok; p.labels = labels;
  p.tx = g.tx; p.ty = g.ty; p.vchunks = g.vchunks;
  p.hdr = (int32_t*)scratch;
  p.sv = (float4*)((char*)scratch + cp_align16_up((size_t)P * PV_HDR * sizeof(int32_t)));
  hipStream_t st = (hipStream_t)stream;
  CP_LAUNCH(pose_verify_pose_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(pose_verify_vertex_kernel, dim3(g.vert_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(pose_verify_tile_kernel, dim3(g.tile_blocks), dim3(VS_THREADS), 0, st, p);
  CP_LAUNCH(pose_verify_finish_kernel, dim3(g.pose_blocks), dim3(VS_THREADS), 0, st, p);
  return cp_check_launch();
}

extern "C" int cp_select_poses(cp_stream_t stream, const double* score, const uint8_t* ok, int C, int B, int32_t* choice) {
  if (!score || !choice || C < 1 || C > PV_CMAX || B < 1) return CP_ERR_INVALID;
  if (cp_misaligned(score, 7) || cp_misaligned(choice, 3)) return CP_ERR_ALIGN;
  if ((long long)C * B >= (1LL << 31)) return CP_ERR_RANGE;
  PsParams p = {score, ok, choice, C, B};
  CP_LAUNCH(pose_select_kernel, dim3((unsigned)((B + VS_THREADS - 1) / VS_THREADS)), dim3(VS_THREADS), 0, (hipStream_t)stream, p);
  return cp_check_launch();
}
