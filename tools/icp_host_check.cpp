// The host halves of csrc/icp_refine.hip -- cp_surface_samples and cp_icp_refine: argument checks, scratch sizing -- exercised by a
// stand-alone program, so that they can be built under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C checkerpose_amd/csrc icp_host_check`, then run checkerpose_amd/csrc/icp_host_check).  Every call below returns before any
// launch: no device is needed, nothing is loaded into Python.  Exit status 0 = every refusal as expected.
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

  // ---- cp_surface_samples
  struct A {
    const double* poses; const double* K; int ks; const float* verts; const int32_t* v_off; const int32_t* faces; const int32_t* f_off; int M;
    const int32_t* ids; int H, W, P, Vmax, grid; int32_t* rect; int32_t* shape; int32_t* pixel; float* depth; int32_t* face; double* X; double* N;
    int32_t* ok; void* scratch;
  };
  const A okA = {d, d, 0, f, i32, i32, i32, 1, nullptr, 80, 96, 3, 64, 32, i32, i32, i32, f, i32, d, d, i32, buf};
  auto callA = [](const A& a) {
    return cp_surface_samples(nullptr, a.poses, a.K, a.ks, a.verts, a.v_off, a.faces, a.f_off, a.M, a.ids, a.H, a.W, a.P, a.Vmax, a.grid, a.rect,
                              a.shape, a.pixel, a.depth, a.face, a.X, a.N, a.ok, a.scratch);
  };
  A a;
  // null pointers (mesh_ids may be null with one mesh)
  a = okA; a.poses = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.K = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.rect = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.shape = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.pixel = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.depth = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.face = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.X = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.N = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.ok = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.scratch = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  // the mesh table
  a = okA; a.verts = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.v_off = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.faces = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.f_off = nullptr; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.M = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.M = 2; EXPECT(callA(a), CP_ERR_INVALID);                          // several meshes need ids
  a = okA; a.Vmax = 0; EXPECT(callA(a), CP_ERR_INVALID);
  // the view
  a = okA; a.ks = 3; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.H = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.W = -1; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.P = 0; EXPECT(callA(a), CP_ERR_INVALID);
  // the grid
  a = okA; a.grid = 0; EXPECT(callA(a), CP_ERR_INVALID);
  a = okA; a.grid = 65; EXPECT(callA(a), CP_ERR_INVALID);
  // alignment
  a = okA; a.scratch = buf + 8; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.poses = (const double*)(buf + 4); EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.K = (const double*)(buf + 4); EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.verts = (const float*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.ids = (const int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.rect = (int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.shape = (int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.pixel = (int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.depth = (float*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.face = (int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.X = (double*)(buf + 4); EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.N = (double*)(buf + 4); EXPECT(callA(a), CP_ERR_ALIGN);
  a = okA; a.ok = (int32_t*)odd; EXPECT(callA(a), CP_ERR_ALIGN);
  // sizes
  a = okA; a.H = 1 << 16; a.W = 1 << 15; EXPECT(callA(a), CP_ERR_RANGE);       // H * W = 2^31
  a = okA; a.H = 4096; a.W = 4096; a.P = 1 << 12; EXPECT(callA(a), CP_ERR_RANGE);      // 2^26 tile blocks
  EXPECT(cp_surface_samples_scratch_bytes(0, 64), 0);
  EXPECT(cp_surface_samples_scratch_bytes(3, -1), 0);
  EXPECT(cp_surface_samples_scratch_bytes(3, 64), 288 + 3 * 64 * 16);
  EXPECT(cp_surface_samples_scratch_bytes(1, 0), 96);

  // ---- cp_icp_refine
  struct B {
    const double* pose_in; const double* K; int ks; const double* X; const double* N; const int32_t* face; int S; const float* depth;
    const int32_t* img; int I, H, W; const double* md; const double* diam; int M; const int32_t* ids; const int32_t* st_in; int iters;
    double tol; int min_pairs; double inertia; int P; double* pose_out; int32_t* st_out; double* info; double* rec;
  };
  const B okB = {d, d, 0, d, d, i32, 1024, f, nullptr, 1, 80, 96, d, d, 1, nullptr, nullptr, 20, 1e-6, 6, 1e-2, 2, d, i32, d, nullptr};
  auto callB = [](const B& b) {
    return cp_icp_refine(nullptr, b.pose_in, b.K, b.ks, b.X, b.N, b.face, b.S, b.depth, b.img, b.I, b.H, b.W, b.md, b.diam, b.M, b.ids, b.st_in,
                         b.iters, b.tol, b.min_pairs, b.inertia, b.P, b.pose_out, b.st_out, b.info, b.rec);
  };
  B b;
  // null pointers (image_ids, mesh_ids, status_in and records may be null)
  b = okB; b.pose_in = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.K = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.X = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.N = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.face = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.depth = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.md = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.diam = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.pose_out = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.st_out = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.info = nullptr; EXPECT(callB(b), CP_ERR_INVALID);
  // the view, the images, the meshes
  b = okB; b.ks = 8; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.H = 0; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.W = 0; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.P = 0; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.P = -2; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.I = 0; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.I = 2; EXPECT(callB(b), CP_ERR_INVALID);                          // several images need ids
  b = okB; b.M = 0; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.M = 2; EXPECT(callB(b), CP_ERR_INVALID);                          // several meshes need ids
  // the slots, the iteration bound, the tolerances
  b = okB; b.S = 0; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.S = 4097; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.iters = 0; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.iters = 65; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.tol = 0.0; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.tol = NAN; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.tol = INFINITY; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.min_pairs = 5; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.inertia = -1e-3; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.inertia = NAN; EXPECT(callB(b), CP_ERR_INVALID);
  b = okB; b.inertia = INFINITY; EXPECT(callB(b), CP_ERR_INVALID);
  // alignment
  b = okB; b.pose_in = (const double*)(buf + 4); EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.K = (const double*)(buf + 4); EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.X = (const double*)(buf + 4); EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.N = (const double*)(buf + 4); EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.face = (const int32_t*)odd; EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.depth = (const float*)odd; EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.img = (const int32_t*)odd; EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.md = (const double*)(buf + 4); EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.diam = (const double*)(buf + 4); EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.ids = (const int32_t*)odd; EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.st_in = (const int32_t*)odd; EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.pose_out = (double*)(buf + 4); EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.st_out = (int32_t*)odd; EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.info = (double*)(buf + 4); EXPECT(callB(b), CP_ERR_ALIGN);
  b = okB; b.rec = (double*)(buf + 4); EXPECT(callB(b), CP_ERR_ALIGN);
  // pose_out over pose_in: all of it (in place) is allowed, a part of it is not
  b = okB; b.pose_out = d + 12; EXPECT(callB(b), CP_ERR_INVALID);              // P = 2: rows 1..2 over rows 0..1
  b = okB; b.pose_in = d + 23; EXPECT(callB(b), CP_ERR_INVALID);
  // sizes
  b = okB; b.H = 1 << 16; b.W = 1 << 15; EXPECT(callB(b), CP_ERR_RANGE);
  b = okB; b.P = 1 << 24; b.pose_out = d; EXPECT(callB(b), CP_ERR_RANGE);
  EXPECT(cp_icp_refine_record_doubles(), 18);
  EXPECT(cp_icp_refine_info_doubles(), 42);
  EXPECT(cp_version() >= 234, 1);
  printf("icp host check: %d refusal(s) as expected, %d failure(s)\n", refusals, failures);
  return failures ? 1 : 0;
}
