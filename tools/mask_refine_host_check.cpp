// The host half of csrc/mask_refine.hip -- cp_mask_extents, cp_contour_samples, cp_mask_refine: argument checks, scratch sizing --
// exercised by a stand-alone program, so that it can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc mask_refine_host_check`, then run checkerpose_amd/csrc/mask_refine_host_check).  Every call below
// returns before any launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal as expected.
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
  double* d = (double*)buf;
  void* odd = buf + 2;

  // ---- cp_mask_extents
  EXPECT(cp_mask_extents(nullptr, nullptr, 2, 50, 70, i32, i32), CP_ERR_INVALID);
  EXPECT(cp_mask_extents(nullptr, i32, 2, 50, 70, nullptr, i32), CP_ERR_INVALID);
  EXPECT(cp_mask_extents(nullptr, i32, 2, 50, 70, i32, nullptr), CP_ERR_INVALID);
  EXPECT(cp_mask_extents(nullptr, i32, 0, 50, 70, i32, i32), CP_ERR_INVALID);
  EXPECT(cp_mask_extents(nullptr, i32, 2, 0, 70, i32, i32), CP_ERR_INVALID);
  EXPECT(cp_mask_extents(nullptr, i32, 2, 50, -1, i32, i32), CP_ERR_INVALID);
  EXPECT(cp_mask_extents(nullptr, (const int32_t*)odd, 2, 50, 70, i32, i32), CP_ERR_ALIGN);
  EXPECT(cp_mask_extents(nullptr, i32, 2, 50, 70, (int32_t*)odd, i32), CP_ERR_ALIGN);
  EXPECT(cp_mask_extents(nullptr, i32, 2, 50, 70, i32, (int32_t*)odd), CP_ERR_ALIGN);
  EXPECT(cp_mask_extents(nullptr, i32, 2, 1 << 16, 1 << 15, i32, i32), CP_ERR_RANGE);
  EXPECT(cp_mask_extents(nullptr, i32, 1 << 30, 300, 300, i32, i32), CP_ERR_RANGE);      // 3 * 2^30 blocks

  // ---- cp_contour_samples
  struct A {
    const double* poses; const double* K; int ks; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off; int M;
    const int32_t* ids; int H, W, P, Vmax, grid; int32_t* rect; int32_t* shape; int32_t* pixel; float* depth; double* X; int32_t* ok; void* scratch;
  };
  const A okA = {d, d, 0, f, i32, i32, i32, 1, nullptr, 80, 96, 3, 64, 5, i32, i32, i32, f, d, i32, buf};
  auto call = [](const A& a) {
    return cp_contour_samples(nullptr, a.poses, a.K, a.ks, a.verts, a.v_off, a.faces, a.f_off, a.M, a.ids, a.H, a.W, a.P, a.Vmax, a.grid, a.rect,
                              a.shape, a.pixel, a.depth, a.X, a.ok, a.scratch);
  };
  A a;
  a = okA; a.poses = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.K = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.rect = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.shape = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.pixel = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.depth = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.X = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.ok = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.scratch = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.verts = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.faces = nullptr; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.M = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.M = 2; EXPECT(call(a), CP_ERR_INVALID);                           // several meshes need ids
  a = okA; a.ks = 3; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.H = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.P = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.grid = 0; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.grid = 65; EXPECT(call(a), CP_ERR_INVALID);
  a = okA; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.poses = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.K = (const double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.X = (double*)(buf + 4); EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.rect = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.shape = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.pixel = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.depth = (float*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.ok = (int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.ids = (const int32_t*)odd; EXPECT(call(a), CP_ERR_ALIGN);
  a = okA; a.H = 0; a.scratch = buf + 8; EXPECT(call(a), CP_ERR_INVALID);      // the order of the classes
  a = okA; a.H = 1 << 16; a.W = 1 << 15; EXPECT(call(a), CP_ERR_RANGE);
  a = okA; a.P = 1 << 20; a.Vmax = 1 << 12; EXPECT(call(a), CP_ERR_RANGE);     // 2^24 vertex blocks
  EXPECT(cp_contour_samples_scratch_bytes(0, 64, 5), 0);
  EXPECT(cp_contour_samples_scratch_bytes(3, -1, 5), 0);
  EXPECT(cp_contour_samples_scratch_bytes(3, 64, 0), 0);
  EXPECT(cp_contour_samples_scratch_bytes(3, 64, 65), 0);
  EXPECT(cp_contour_samples_scratch_bytes(3, 64, 5), 288 + 480 + 3 * 64 * 16);
  EXPECT(cp_contour_samples_scratch_bytes(1, 0, 1), 96 + 32);

  // ---- cp_mask_refine
  struct B {
    const double* pose_in; const double* K; int ks; const double* X; const int32_t* pixel; const int32_t* ok; int grid; const int32_t* row;
    const int32_t* col; const int32_t* mask_ids; int NM, H, W; const double* max_dist; const int32_t* status; int dof, max_iters; double step_tol;
    int min_pairs, P; double* pose_out; int32_t* status_out; double* info; double* records;
  };
  const B okB = {d, d, 0, d, i32, i32, 5, i32, i32, nullptr, 3, 80, 96, d, nullptr, 1, 20, 1e-6, 6, 3, d + 64, i32, d, nullptr};
  auto refine = [](const B& b) {
    return cp_mask_refine(nullptr, b.pose_in, b.K, b.ks, b.X, b.pixel, b.ok, b.grid, b.row, b.col, b.mask_ids, b.NM, b.H, b.W, b.max_dist, b.status,
                          b.dof, b.max_iters, b.step_tol, b.min_pairs, b.P, b.pose_out, b.status_out, b.info, b.records);
  };
  B b;
  b = okB; b.pose_in = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.K = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.X = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.pixel = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.ok = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.row = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.col = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.max_dist = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.pose_out = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.status_out = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.info = nullptr; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.ks = 4; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.H = 0; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.P = 0; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.NM = 0; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.NM = 4; EXPECT(refine(b), CP_ERR_INVALID);                        // NM != P needs mask ids
  b = okB; b.grid = 0; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.grid = 65; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.dof = 2; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.dof = -1; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.max_iters = 0; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.max_iters = 65; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.step_tol = 0.0; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.step_tol = INFINITY; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.step_tol = NAN; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.min_pairs = 5; EXPECT(refine(b), CP_ERR_INVALID);
  b = okB; b.pose_in = (const double*)(buf + 4); EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.X = (const double*)(buf + 4); EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.pixel = (const int32_t*)odd; EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.ok = (const int32_t*)odd; EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.row = (const int32_t*)odd; EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.col = (const int32_t*)odd; EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.mask_ids = (const int32_t*)odd; EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.max_dist = (const double*)(buf + 4); EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.status = (const int32_t*)odd; EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.pose_out = (double*)(buf + 516); EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.status_out = (int32_t*)odd; EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.info = (double*)(buf + 4); EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.records = (double*)(buf + 4); EXPECT(refine(b), CP_ERR_ALIGN);
  b = okB; b.pose_out = d + 1; EXPECT(refine(b), CP_ERR_INVALID);              // a partial overlap of the poses
  b = okB; b.H = 1 << 16; b.W = 1 << 15; EXPECT(refine(b), CP_ERR_RANGE);
  b = okB; b.P = 1 << 24; b.NM = 1 << 24; b.pose_out = d; EXPECT(refine(b), CP_ERR_RANGE);
  EXPECT(cp_mask_refine_record_doubles(), 18);
  EXPECT(cp_mask_refine_info_doubles(), 42);
  EXPECT(cp_version() >= 240, 1);
  printf("mask_refine host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
