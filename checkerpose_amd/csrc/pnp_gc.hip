// Graph-cut RANSAC pose solver on the device: what the reference's `--use_progressivex` runs comes down to with
// maximum_model_number = 1 (test_network_with_test_data.py:68-99) -- RANSAC from a minimal solver, a locally optimised model whose
// inlier set is a two-label graph cut (unary term from the residual, Potts term over a neighbourhood graph of the MODEL keypoints),
// and a refit over that labelling repeated while it improves.  pyprogressivex is not part of the reference's tree: the rule below is
// this project's own, restated in tests/gc_stages.py; parity with pyprogressivex is UNPINNED.  All arithmetic in fp64 / integers.
//   radius_graph_count_kernel / radius_graph_fill_kernel   the neighbourhood graph of an object as CSR, once per object
//   gc_hypotheses_kernel    one launch per round of 64 hypotheses (a lane each): 4 distinct valid correspondences from the hash32
//                           sequence, solve_four_points (P3P on three, the fourth picks the root), count + MSAC score -> a 14-double
//                           record; between rounds OpenCV's stopping rule (needed_iters, m = 4) on the counts
//   gc_select_lo_kernel     one 256-thread workgroup per crop: winner = first record with the largest score among those with count >= 4;
//                           then at most GC_LO_MAX refits: L_k = label(P_k) (below), Q_k = EPnP over L_k (pnp_core.h's
//                           epnp_block_refit), accepted while score(Q_k) > score(P_k)
//   graphcut_label_kernel   the labelling alone on caller-given capacities (what the tests compare with an exact max-flow)
// The labelling: capacities are integers with Q = 2^16: s->i = Q, i->t = cin_i, i<->j = w per direction on every graph edge between two
// valid points.  The inlier set is the MINIMAL source side of a minimum cut (the nodes reachable from s in the residual graph of a
// maximum flow): the same set for every maximum flow, so it depends on no thread order and can be checked exactly.
// The max flow (gc_maxflow): min(Q, cin_i) is cancelled at each node first, which leaves a node either an excess (Q - cin_i) or a
// capacity to the sink (cin_i - Q).  Then push-relabel in sweeps over the nodes with a global relabel (BFS from the sink over the
// residual arcs: exact distances, GC_INF where the sink cannot be reached) every GC_SWEEPS_PER_RELABEL sweeps; it ends when a fresh
// global relabel finds no node that holds excess and can reach the sink.  Excess that cannot reach the sink stays where it is (no
// second phase): the minimal source side is exactly the set reachable over residual arcs from the nodes that still hold excess --
// arcs into that set carry no flow and arcs out of it are saturated, and returning the excess to s along the flow that brought it
// only frees arcs inside the set.  Net flows per directed CSR slot (flow[rev] = -flow) live in scratch, heights / excesses / sink
// capacities in LDS.  Within a sweep a node pushes to every neighbour below it and is relabelled only when it could push nothing, so
// of an arc's two ends at most one writes its two slots in a sweep; excesses are 64-bit integer atomics.  Heights only steer the
// work: the answer rests on the BFS alone.  GC_MAX_SWEEPS bounds the sweeps (DESIGN.md section 5 has the counts it was chosen from);
// hitting it is reported as status -1, never as an approximate labelling.
#include "pnp_core.h"

namespace {

constexpr int GC_THREADS = 256, GC_MAX_ITERS = 512, GC_NMAX = 4096, GC_LO_MAX = 8, GC_STEP = 30;
constexpr long long GC_MAX_EDGES = 1ll << 21;              // directed edges per object
constexpr int32_t GC_Q = 1 << 16, GC_INF = 0x3fffffff, GC_WMAX = 1 << 28;
// sweeps: the largest count over the committed cases is 48 on an MI355X (case thr_2; the count depends on the threads' timing within
// a sweep) and 40 with the procedure below on one lane (tests/gc_stages.py:count_sweeps; 24 over the hand-built labelling problems);
// 2048 leaves a margin of 42 x.  The tests hold the device's own counts (in the stage records) to a sixteenth of the bound
constexpr int GC_SWEEPS_PER_RELABEL = 8, GC_MAX_SWEEPS = 2048;

// ------------------------------------------------------------------------------------------------ the neighbourhood graph
__device__ __forceinline__ bool rg_near(const float* a, const float* b, double r2) {
#pragma clang fp contract(off)
  const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
  const double d2 = dx * dx + dy * dy + dz * dz;
  return d2 <= r2;
}

// one workgroup per object: degrees into LDS, then the exclusive prefix sums (a serial pass: N <= 4096, once per object)
__global__ __launch_bounds__(GC_THREADS) void radius_graph_count_kernel(const float* __restrict__ pts, int N, double r2,
                                                                        int32_t* __restrict__ offsets, int32_t* __restrict__ totals) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t* const deg = (int32_t*)smem;
  const int m = blockIdx.x, tid = threadIdx.x;
  const float* P = pts + (size_t)m * N * 3;
  for (int i = tid; i < N; i += GC_THREADS) {
    int c = 0;
    for (int j = 0; j < N; ++j) c += (j != i && rg_near(P + 3 * i, P + 3 * j, r2)) ? 1 : 0;
    deg[i] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int32_t* off = offsets + (size_t)m * (N + 1);
    int32_t run = 0;
    for (int i = 0; i < N; ++i) { off[i] = run; run += deg[i]; }
    off[N] = run;
    totals[m] = run;
  }
}

__global__ __launch_bounds__(GC_THREADS) void radius_graph_fill_kernel(const float* __restrict__ pts, int N, double r2,
                                                                       const int32_t* __restrict__ offsets, const long long* __restrict__ base,
                                                                       int32_t* __restrict__ indices, long long n_indices) {
  const int m = blockIdx.x, tid = threadIdx.x;
  const float* P = pts + (size_t)m * N * 3;
  const int32_t* off = offsets + (size_t)m * (N + 1);
  const long long b0 = base[m];
  for (int i = tid; i < N; i += GC_THREADS) {
    long long k = b0 + off[i];
    const long long end = b0 + off[i + 1];
    for (int j = 0; j < N; ++j)                               // columns ascending
      if (j != i && rg_near(P + 3 * i, P + 3 * j, r2)) {
        if (k >= 0 && k < end && k < n_indices) indices[k] = j;
        ++k;
      }
  }
}

// ------------------------------------------------------------------------------------------------ the labelling
struct GcNet { const int32_t* off; const int32_t* idx; int32_t* flow; int N; int32_t w; long long E; };     // off[N + 1], idx / flow [E]
struct GcState { int32_t* cin; int32_t* h; int32_t* sk; long long* ex; uint8_t* lab; };                    // [N] each

__device__ __forceinline__ int gc_lo(const GcNet& g, int v) { const long long a = g.off[v]; return (int)(a < 0 ? 0 : (a > g.E ? g.E : a)); }
__device__ __forceinline__ int gc_hi(const GcNet& g, int v) { const long long a = g.off[v + 1]; return (int)(a < 0 ? 0 : (a > g.E ? g.E : a)); }
// the slot of arc v -> u in v's ascending list, -1 where the list does not hold u (a graph that is not symmetric)
__device__ __forceinline__ int gc_rev(const GcNet& g, int v, int u) {
  int lo = gc_lo(g, v), hi = gc_hi(g, v) - 1;
  if (lo > hi) return -1;
  while (lo < hi) {                                           // at most 22 halvings: E <= 2^21
    const int mid = (lo + hi) >> 1;
    if (g.idx[mid] < u) lo = mid + 1; else hi = mid;
  }
  return g.idx[lo] == u ? lo : -1;
}

// all GC_THREADS threads; s.cin holds the capacities (-1 = not a node).  -> 0, or -1 when GC_MAX_SWEEPS did not suffice; s.lab = the
// minimal source side, *flow_out = the value of the maximum flow (min(Q, cin) included), *sweeps_out = sweeps run.  red / ctl: LDS words
__device__ int gc_maxflow(const GcNet g, const GcState s, int tid, unsigned long long* red, int* ctl, long long* flow_out, int* sweeps_out) {
  const int N = g.N;
  long long part = 0;                                         // this thread's share of: cancelled flow + the sink capacities
  if (tid == 0) red[0] = 0ull;
  for (int i = tid; i < N; i += GC_THREADS) {
    const int32_t c = s.cin[i];
    long long e = 0;
    int32_t k = 0;
    if (c >= 0) {
      if (c < GC_Q) { e = GC_Q - c; part += c; } else { k = c - GC_Q; part += (long long)GC_Q + k; }
    }
    s.ex[i] = e; s.sk[i] = k; s.lab[i] = 0;
    for (int a = gc_lo(g, i), hi = gc_hi(g, i); a < hi; ++a) g.flow[a] = 0;
  }
  __syncthreads();
  int sweeps = 0, rc = -1;
  for (int round = 0; round <= GC_MAX_SWEEPS / GC_SWEEPS_PER_RELABEL; ++round) {
    // global relabel: exact distances to the sink over the residual arcs, level by level (at most N levels)
    for (int i = tid; i < N; i += GC_THREADS) s.h[i] = (s.cin[i] >= 0 && s.sk[i] > 0) ? 1 : GC_INF;
    __syncthreads();
    for (int L = 1; L <= N; ++L) {
      if (tid == 0) ctl[0] = 0;
      __syncthreads();
      for (int v = tid; v < N; v += GC_THREADS) {
        if (s.cin[v] < 0 || s.h[v] != GC_INF) continue;
        for (int a = gc_lo(g, v), hi = gc_hi(g, v); a < hi; ++a) {
          const int u = g.idx[a];
          if ((unsigned)u < (unsigned)N && s.h[u] == L && g.w - g.flow[a] > 0) { s.h[v] = L + 1; ctl[0] = 1; break; }
        }
      }
      __syncthreads();
      const int changed = ctl[0];
      __syncthreads();
      if (!changed) break;
    }
    if (tid == 0) ctl[1] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += GC_THREADS)
      if (s.ex[i] > 0 && s.h[i] < GC_INF) ctl[1] = 1;
    __syncthreads();
    const int active = ctl[1];
    __syncthreads();
    if (!active) { rc = 0; break; }
    if (round == GC_MAX_SWEEPS / GC_SWEEPS_PER_RELABEL) break;
    for (int k = 0; k < GC_SWEEPS_PER_RELABEL; ++k) {
      for (int u = tid; u < N; u += GC_THREADS) {
        const long long e0 = s.ex[u];
        const int hu = s.h[u];
        if (e0 <= 0 || hu >= GC_INF) continue;
        long long rem = e0;
        int hmin = GC_INF;
        if (s.sk[u] > 0) {                                    // the sink, height 0
          const long long d = rem < s.sk[u] ? rem : (long long)s.sk[u];
          s.sk[u] -= (int32_t)d;
          rem -= d;
        }
        for (int a = gc_lo(g, u), hi = gc_hi(g, u); a < hi && rem > 0; ++a) {
          const int v = g.idx[a];
          if ((unsigned)v >= (unsigned)N || s.cin[v] < 0) continue;
          const int32_t r = g.w - g.flow[a];
          if (r <= 0) continue;
          const int hv = s.h[v];
          if (hv < hu) {
            const int ra = gc_rev(g, v, u);
            if (ra < 0) continue;
            const long long d = rem < r ? rem : (long long)r;
            g.flow[a] += (int32_t)d;
            g.flow[ra] -= (int32_t)d;
            atomicAdd((unsigned long long*)&s.ex[v], (unsigned long long)d);
            rem -= d;
          } else if (hv < hmin) hmin = hv;
        }
        if (rem != e0) atomicAdd((unsigned long long*)&s.ex[u], (unsigned long long)(rem - e0));
        else s.h[u] = hmin >= GC_INF ? GC_INF : hmin + 1;
      }
      __syncthreads();
      ++sweeps;
    }
  }
  *sweeps_out = sweeps;
  if (rc != 0) return rc;
  // the minimal source side: reachable over residual arcs from the nodes that still hold excess
  for (int i = tid; i < N; i += GC_THREADS) {
    s.lab[i] = (s.cin[i] >= 0 && s.ex[i] > 0) ? 1 : 0;
    part -= s.sk[i];
  }
  atomicAdd(red, (unsigned long long)part);
  __syncthreads();
  for (int it = 0; it < N; ++it) {
    if (tid == 0) ctl[0] = 0;
    __syncthreads();
    for (int v = tid; v < N; v += GC_THREADS) {
      if (s.cin[v] < 0 || s.lab[v]) continue;
      for (int a = gc_lo(g, v), hi = gc_hi(g, v); a < hi; ++a) {
        const int u = g.idx[a];                               // residual of u -> v = w - flow[u -> v] = w + flow[v -> u]
        if ((unsigned)u < (unsigned)N && s.lab[u] && g.w + g.flow[a] > 0) { s.lab[v] = 1; ctl[0] = 1; break; }
      }
    }
    __syncthreads();
    const int changed = ctl[0];
    __syncthreads();
    if (!changed) break;
  }
  *flow_out = (long long)red[0];
  return 0;
}

__global__ __launch_bounds__(GC_THREADS) void graphcut_label_kernel(const int32_t* __restrict__ cin, const int32_t* __restrict__ off,
                                                                    const int32_t* __restrict__ idx, int N, long long E, int32_t w,
                                                                    uint8_t* __restrict__ labels, long long* __restrict__ flow_value,
                                                                    int32_t* __restrict__ status, int32_t* __restrict__ sweeps, int32_t* __restrict__ flow) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  GcState s;
  s.ex = (long long*)smem; s.cin = (int32_t*)(s.ex + N); s.h = s.cin + N; s.sk = s.h + N; s.lab = (uint8_t*)(s.sk + N);
  __shared__ unsigned long long red[1];
  __shared__ int ctl[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < N; i += GC_THREADS) s.cin[i] = cin[(size_t)b * N + i];
  __syncthreads();
  GcNet g;
  g.off = off; g.idx = idx; g.flow = flow + (size_t)b * (size_t)E; g.N = N; g.w = w; g.E = E;
  long long fv = 0;
  int sw = 0;
  const int rc = gc_maxflow(g, s, tid, red, ctl, &fv, &sw);
  for (int i = tid; i < N; i += GC_THREADS) labels[(size_t)b * N + i] = rc == 0 ? s.lab[i] : 0;
  if (tid == 0) {
    flow_value[b] = rc == 0 ? fv : -1;
    status[b] = rc;
    if (sweeps) sweeps[b] = sw;
  }
}

// ------------------------------------------------------------------------------------------------ the solver
struct GcParams {
  const float* p3d; const float* p2d; const uint8_t* valid; const float* K;
  const int32_t* g_off; const int32_t* g_idx; const long long* g_base; const int32_t* graph_ids;
  double* pose; uint8_t* inliers; int32_t* status;
  double* hyp; double* steps; int32_t* cin_rec; uint8_t* lab_rec; int32_t* flow;
  long long p3d_bs, K_bs, max_edges, n_indices;
  int B, N, M, valid_stride, iters, round, min_inliers;
  int32_t w;
  float thr;
  uint32_t seed;
};

// one launch per round of 64 hypotheses, grid B, one wave per workgroup, a hypothesis per lane
__global__ __launch_bounds__(64) void gc_hypotheses_kernel(const GcParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint16_t* const vidx = (uint16_t*)smem;                    // [N] valid indices, ascending
  __shared__ int wsum[1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint8_t* valid = p.valid + (size_t)b * p.N * p.valid_stride;
  const int vs = p.valid_stride;
  const int nv = block_compact<64>([&](int i) { return valid[(size_t)i * vs] != 0; }, p.N, vidx, wsum, tid);
  const int h = p.round * 64 + tid;
  if (nv < p.min_inliers) return;                            // the identity fallback: no hypotheses
  double* hb = p.hyp + (size_t)b * p.iters * PNP_HYP;
  if (p.round > 0 && hypotheses_run(hb, nv, 4, p.iters, p.round) <= 64 * p.round) return;      // whole workgroup, uniform
  if (h >= p.iters) return;
  const Points P = crop_points(p.p3d + (size_t)b * p.p3d_bs, p.p2d + (size_t)b * p.N * 2, p.K + (size_t)b * p.K_bs);
  const double thr2 = (double)p.thr * (double)p.thr;
  int pos[4];
  double R[9], t[3];
  bool ok = sample_distinct<4>(p.seed, (uint32_t)b, (uint32_t)h, nv, pos);
  if (ok) {
    float pw4[12], uv4[8];
    for (int i = 0; i < 4; ++i) {
      const size_t k = (size_t)vidx[pos[i]];
      for (int c = 0; c < 3; ++c) pw4[3 * i + c] = P.p3d[3 * k + c];
      uv4[2 * i] = P.p2d[2 * k]; uv4[2 * i + 1] = P.p2d[2 * k + 1];
    }
    ok = solve_four_points(pw4, uv4, P.fu, P.fv, P.uc, P.vc, R, t);
  }
  double* rec = hb + (size_t)h * PNP_HYP;
  int cnt = -1;
  if (ok) {
    cnt = 0;
    double score = 0.0;
    for (int i = 0; i < nv; ++i) {
      const double r2 = reproj_sq(P, R, t, (int)vidx[i]);
      if (r2 <= thr2) { ++cnt; score += 1.0 - r2 / thr2; }
    }
    rec[1] = score;
    for (int i = 0; i < 9; ++i) rec[2 + i] = R[i];
    for (int i = 0; i < 3; ++i) rec[11 + i] = t[i];
  }
  rec[0] = (double)cnt;
}

__global__ __launch_bounds__(GC_THREADS) void gc_select_lo_kernel(const GcParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int N = p.N;
  GcState s;
  s.ex = (long long*)smem; s.cin = (int32_t*)(s.ex + N); s.h = s.cin + N; s.sk = s.h + N;
  int32_t* const vidx = s.sk + N;
  int32_t* const iidx = vidx + N;
  s.lab = (uint8_t*)(iidx + N);
  bool* const flag = (bool*)(s.lab + N);
  __shared__ EpnpRefitLds rl;
  __shared__ unsigned long long red[1];
  __shared__ int ctl[2], wsum[GC_THREADS / 64], s_best;
  const int b = blockIdx.x, tid = threadIdx.x;
  const uint8_t* valid = p.valid + (size_t)b * N * p.valid_stride;
  for (int i = tid; i < N; i += GC_THREADS) { flag[i] = valid[(size_t)i * p.valid_stride] != 0; p.inliers[(size_t)b * N + i] = 0; }
  __syncthreads();
  const int nv = block_compact<GC_THREADS>([&](int i) { return flag[i]; }, N, vidx, wsum, tid);
  double* pose = p.pose + (size_t)b * 12;
  auto identity = [&](int st) {                              // the reference's fallback: identity pose, no inliers
    if (tid == 0) {
      write_identity_pose(pose);
      p.status[b] = st;
    }
  };
  if (nv < p.min_inliers) { identity(0); return; }
  Points P = crop_points(p.p3d + (size_t)b * p.p3d_bs, p.p2d + (size_t)b * N * 2, p.K + (size_t)b * p.K_bs);
  P.idx = iidx;
  const double thr2 = (double)p.thr * (double)p.thr;
  const double* hb = p.hyp + (size_t)b * p.iters * PNP_HYP;
  if (tid == 0) {                                            // the largest score among the records with count >= 4, first on ties
    int best = -1;
    double bs = -1.0;
    const int nrun = hypotheses_run(hb, nv, 4, p.iters, GC_MAX_ITERS / 64);
    for (int h = 0; h < nrun; ++h) {
      if ((int)hb[(size_t)h * PNP_HYP] < 4) continue;
      const double sc = hb[(size_t)h * PNP_HYP + 1];
      if (sc > bs) { bs = sc; best = h; }
    }
    s_best = best;
  }
  __syncthreads();
  const int best = s_best;
  if (best < 0) { identity(0); return; }
  double Pk[12], sP = hb[(size_t)best * PNP_HYP + 1];
  for (int i = 0; i < 12; ++i) Pk[i] = hb[(size_t)best * PNP_HYP + 2 + i];
  const int m = p.graph_ids ? p.graph_ids[b] : 0;
  const long long gb = (m >= 0 && m < p.M) ? p.g_base[m] : -1;
  if (gb < 0 || gb > p.n_indices) { identity(-2); return; }   // a graph id or a base outside the graph: refused, nothing is read
  GcNet g;
  g.off = p.g_off + (size_t)m * (N + 1);
  g.idx = p.g_idx + gb;
  g.flow = p.flow + (size_t)b * (size_t)p.max_edges;
  g.N = N; g.w = p.w;
  g.E = p.n_indices - gb < p.max_edges ? p.n_indices - gb : p.max_edges;
  bool have = false;
  for (int k = 0; k <= GC_LO_MAX; ++k) {
    double* rec = p.steps + ((size_t)b * (GC_LO_MAX + 1) + k) * GC_STEP;
    int32_t* crec = p.cin_rec + ((size_t)b * (GC_LO_MAX + 1) + k) * N;
    uint8_t* lrec = p.lab_rec + ((size_t)b * (GC_LO_MAX + 1) + k) * N;
    for (int i = tid; i < N; i += GC_THREADS) {
      int32_t c = -1;
      if (flag[i]) {
        double q = reproj_sq(P, Pk, Pk + 9, i) / thr2;
        if (!(q < 16384.0)) q = 16384.0;                      // the cap, also where the projection is not finite
        c = (int32_t)floor(q * (double)GC_Q + 0.5);
      }
      s.cin[i] = c;
      crec[i] = c;
    }
    if (tid == 0) {
      rec[0] = (double)k;
      for (int i = 0; i < 12; ++i) rec[1 + i] = Pk[i];
      rec[13] = sP;
    }
    __syncthreads();
    long long fv = 0;
    int sw = 0;
    const int rc = gc_maxflow(g, s, tid, red, ctl, &fv, &sw);
    if (tid == 0) rec[29] = (double)sw;
    if (rc != 0) { identity(-1); return; }
    for (int i = tid; i < N; i += GC_THREADS) lrec[i] = s.lab[i];
    const int nl = block_compact<GC_THREADS>([&](int i) { return s.lab[i] != 0; }, N, iidx, wsum, tid);
    if (tid == 0) rec[14] = (double)nl;
    have = nl >= p.min_inliers;
    if (!have || k == GC_LO_MAX) break;
    Points S = P;
    S.n = nl;
    const bool ok = epnp_block_refit(S, rl, tid);
    if (tid == 0) rec[15] = ok ? 1.0 : 0.0;
    if (!ok) break;
    double Qk[12];
    for (int i = 0; i < 12; ++i) Qk[i] = rl.pose[i];
    double acc[1] = {0.0};
    for (int i = tid; i < nv; i += GC_THREADS) {
      const double r2 = reproj_sq(P, Qk, Qk + 9, vidx[i]);
      if (r2 <= thr2) acc[0] += 1.0 - r2 / thr2;
    }
    block_sum<1>(acc, rl.sred, tid);
    const double sQ = acc[0];
    if (tid == 0) {
      for (int i = 0; i < 12; ++i) rec[16 + i] = Qk[i];
      rec[28] = sQ;
    }
    if (!(sQ > sP)) break;
    for (int i = 0; i < 12; ++i) Pk[i] = Qk[i];
    sP = sQ;
  }
  if (!have) { identity(0); return; }
  for (int i = tid; i < N; i += GC_THREADS) p.inliers[(size_t)b * N + i] = s.lab[i];
  if (tid == 0) {
    for (int i = 0; i < 12; ++i) pose[i] = Pk[i];
    p.status[b] = 1;
  }
}

struct GcScratch { size_t hyp, steps, cin, lab, flow, total; };
GcScratch gc_scratch(int B, int N, long long max_edges) {
  GcScratch s;
  s.hyp = 0;
  s.steps = (size_t)B * GC_MAX_ITERS * PNP_HYP * sizeof(double);
  s.cin = s.steps + (size_t)B * (GC_LO_MAX + 1) * GC_STEP * sizeof(double);
  s.lab = s.cin + (size_t)B * (GC_LO_MAX + 1) * N * sizeof(int32_t);
  s.flow = (s.lab + (size_t)B * (GC_LO_MAX + 1) * N + 7) & ~(size_t)7;
  s.total = s.flow + (size_t)B * (size_t)(max_edges > 0 ? max_edges : 1) * sizeof(int32_t);
  return s;
}

}  // namespace

extern "C" int cp_radius_graph_count(cp_stream_t stream, const float* pts, int M, int N, double radius, int32_t* offsets, int32_t* totals) {
  if (!pts || !offsets || !totals) return CP_ERR_INVALID;
  if (M <= 0 || N <= 0 || N > GC_NMAX || !(radius >= 0.0) || !(radius < 1e150)) return CP_ERR_INVALID;
  if (cp_misaligned(pts, 3) || cp_misaligned(offsets, 3) || cp_misaligned(totals, 3)) return CP_ERR_ALIGN;
  CP_LAUNCH(radius_graph_count_kernel, dim3((unsigned)M), dim3(GC_THREADS), (size_t)N * 4, (hipStream_t)stream, pts, N, radius * radius, offsets, totals);
  return cp_check_launch();
}

extern "C" int cp_radius_graph_fill(cp_stream_t stream, const float* pts, int M, int N, double radius, const int32_t* offsets,
                                    const int64_t* base, int32_t* indices, long long n_indices) {
  if (!pts || !offsets || !base || !indices) return CP_ERR_INVALID;
  if (M <= 0 || N <= 0 || N > GC_NMAX || !(radius >= 0.0) || !(radius < 1e150)) return CP_ERR_INVALID;
  if (n_indices < 0 || n_indices > (long long)M * GC_MAX_EDGES) return CP_ERR_INVALID;
  if (cp_misaligned(pts, 3) || cp_misaligned(offsets, 3) || cp_misaligned(indices, 3) || cp_misaligned(base, 7)) return CP_ERR_ALIGN;
  CP_LAUNCH(radius_graph_fill_kernel, dim3((unsigned)M), dim3(GC_THREADS), 0, (hipStream_t)stream, pts, N, radius * radius, offsets,
            (const long long*)base, indices, n_indices);
  return cp_check_launch();
}

extern "C" int cp_graphcut_label(cp_stream_t stream, const int32_t* cin, const int32_t* offsets, const int32_t* indices, int B, int N,
                                 long long n_edges, int32_t w, uint8_t* labels, int64_t* flow_value, int32_t* status, int32_t* sweeps,
                                 void* scratch, size_t scratch_bytes) {
  if (!cin || !offsets || !indices || !labels || !flow_value || !status || !scratch) return CP_ERR_INVALID;
  if (B <= 0 || N <= 0 || N > GC_NMAX || n_edges < 0 || n_edges > GC_MAX_EDGES || w < 0 || w > GC_WMAX) return CP_ERR_INVALID;
  if (scratch_bytes < (size_t)B * (size_t)(n_edges > 0 ? n_edges : 1) * sizeof(int32_t)) return CP_ERR_INVALID;
  if (cp_misaligned(cin, 3) || cp_misaligned(offsets, 3) || cp_misaligned(indices, 3) || cp_misaligned(status, 3) || cp_misaligned(sweeps, 3) ||
      cp_misaligned(scratch, 3) || cp_misaligned(flow_value, 7))
    return CP_ERR_ALIGN;
  static CpDeviceOnce once;
  const int dev = cp_current_device();
  CP_LDS_ATTR_ONCE(once, dev, cp_set_max_lds((const void*)graphcut_label_kernel, (size_t)GC_NMAX * 21 + 16));
  CP_LAUNCH(graphcut_label_kernel, dim3((unsigned)B), dim3(GC_THREADS), (size_t)N * 21 + 16, (hipStream_t)stream, cin, offsets, indices, N,
            n_edges, w, labels, (long long*)flow_value, status, sweeps, (int32_t*)scratch);
  return cp_check_launch();
}

extern "C" size_t cp_pnp_gc_scratch_bytes(int B, int N, long long max_edges) {
  if (B <= 0 || N <= 0 || N > GC_NMAX || max_edges < 0 || max_edges > GC_MAX_EDGES) return 0;
  return gc_scratch(B, N, max_edges).total;
}

extern "C" int cp_pnp_gc(cp_stream_t stream, const float* p3d, long long p3d_bstride, const float* p2d, const uint8_t* valid,
                         int valid_stride, const float* cam_K, long long K_bstride, const int32_t* g_offsets, const int32_t* g_indices,
                         const int64_t* g_base, const int32_t* graph_ids, int M, long long max_edges, long long n_indices, int B, int N,
                         float reproj_threshold, int32_t w, int iterations, int min_inliers, uint32_t seed, double* pose,
                         uint8_t* inliers, int32_t* status, void* scratch) {
  if (!p3d || !p2d || !valid || !cam_K || !g_offsets || !g_indices || !g_base || !pose || !inliers || !status || !scratch) return CP_ERR_INVALID;
  if (B <= 0 || N <= 0 || N > GC_NMAX || valid_stride <= 0 || iterations <= 0 || iterations > GC_MAX_ITERS || !(reproj_threshold > 0.f))
    return CP_ERR_INVALID;
  if (M <= 0 || (M > 1 && !graph_ids) || max_edges < 0 || max_edges > GC_MAX_EDGES || n_indices < 0 || n_indices > (long long)M * GC_MAX_EDGES ||
      w < 0 || w > GC_WMAX || min_inliers < 4)
    return CP_ERR_INVALID;
  if (cp_p3d_stride_invalid(p3d_bstride, N) || cp_K_stride_invalid(K_bstride)) return CP_ERR_INVALID;
  if (cp_misaligned(pose, 7) || cp_misaligned(scratch, 7) || cp_misaligned(g_base, 7) || cp_misaligned(status, 3) || cp_misaligned(g_offsets, 3) ||
      cp_misaligned(g_indices, 3) || cp_misaligned(graph_ids, 3))
    return CP_ERR_ALIGN;
  const GcScratch sc = gc_scratch(B, N, max_edges);
  unsigned char* base = (unsigned char*)scratch;
  GcParams p;
  p.p3d = p3d; p.p2d = p2d; p.valid = valid; p.K = cam_K;
  p.g_off = g_offsets; p.g_idx = g_indices; p.g_base = (const long long*)g_base; p.graph_ids = graph_ids;
  p.pose = pose; p.inliers = inliers; p.status = status;
  p.hyp = (double*)(base + sc.hyp); p.steps = (double*)(base + sc.steps); p.cin_rec = (int32_t*)(base + sc.cin);
  p.lab_rec = base + sc.lab; p.flow = (int32_t*)(base + sc.flow);
  p.p3d_bs = p3d_bstride; p.K_bs = K_bstride; p.max_edges = max_edges; p.n_indices = n_indices;
  p.B = B; p.N = N; p.M = M; p.valid_stride = valid_stride; p.iters = iterations; p.round = 0; p.min_inliers = min_inliers;
  p.w = w; p.thr = reproj_threshold; p.seed = seed;
  static CpDeviceOnce once;
  const int dev = cp_current_device();
  CP_LDS_ATTR_ONCE(once, dev, cp_set_max_lds((const void*)gc_select_lo_kernel, (size_t)GC_NMAX * 30 + 16));
  hipStream_t st = (hipStream_t)stream;
  for (int r = 0; 64 * r < iterations; ++r) {
    p.round = r;
    CP_LAUNCH(gc_hypotheses_kernel, dim3((unsigned)B), dim3(64), (size_t)N * 2 + 16, st, p);
  }
  p.round = 0;
  CP_LAUNCH(gc_select_lo_kernel, dim3((unsigned)B), dim3(GC_THREADS), (size_t)N * 30 + 16, st, p);
  return cp_check_launch();
}
