// wgrad.hip — GEMM problem helpers and the weight-gradient scheduling (wgrad.h): split counts, the grouped and the
// deterministic launch, and the launch on the side stream.  The one file that knows both GEMM problems and the side stream.
#include "wgrad.h"
#include "side_stream.h"
#include <string.h>

// ----------------------------------------------------------------- GEMM helpers
GemmProblem gp(const float* A, int lda, int ta, const float* Bm, int ldb, int tb, float* C, int ldc, int M,
                      int N, int K) {
  GemmProblem p;
  memset(&p, 0, sizeof(p));
  p.A = A; p.lda = lda; p.ta = ta;
  p.Bseg[0] = Bm; p.kseg = K; p.ldb = ldb; p.tb = tb;
  p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  p.alpha = 1.f; p.ksplit = 1;
  return p;
}
int run1(const GemmProblem& p, hipStream_t st) {
  GemmGroup g;
  memset(&g, 0, sizeof(g));
  g.n = 1; g.p[0] = p;
  return ps_launch_gemm(g, st);
}
// weight gradient  dW[N_out, K_in] += dY[rows, N_out]^T . X[rows, K_in]   (atomic, split over rows)
GemmProblem gp_wgrad(const float* dY, int lddy, const float* X, int ldx, float* dW, int n_out, int k_in,
                            int rows) {
  GemmProblem p = gp(dY, lddy, 1, X, ldx, 1, dW, k_in, n_out, k_in, rows);
  p.accumulate = 2;
  return p;
}
static int pick_ksplit(int tiles, int rows) {   // ~2 workgroups per CU, but at least ~512 reduction rows per split
  // Every split adds a 64x64 tile of fp32 atomics onto the same weight-gradient addresses.  Measured: C2 (8,064 rows; step
  // time by blocks per launch: 512 0.380 ms, 256 0.375, 224 0.373, 192 0.372-0.377, 128 0.392) wants ~15 splits of ~540
  // rows; the review transformer (78k rows, 4 tiles) wants its 128 splits of ~610 rows (1.146 ms vs 1.193 with 56).
  static const int target = ps_env_int("PS_WGRAD_BLOCKS", 512);   // tuning experiments
  static const int min_rows = ps_env_int("PS_WGRAD_ROWS", 512);
  const int nt = tiles > 0 ? tiles : 1;
  const int want = target / nt;
  int ks = (rows + min_rows - 1) / min_rows;                 // >= ~512 rows per split ...
  const int fill = (128 + nt - 1) / nt, cap128 = (rows + 127) / 128;
  if (ks < fill) ks = fill < cap128 ? fill : cap128;         // ... unless that leaves fewer than ~128 workgroups (Wo: 4 tiles)
  if (ks > want) ks = want;
  return ks < 1 ? 1 : ks;
}
// scratch of the ordered split reduction: per device, grow-only, allocated outside any stream capture
static float* det_scratch(size_t floats, hipStream_t st) { return ps_det_scratch(0, floats, st); }
// dW[i] += sum_s part[s][i], s ascending: the second pass of a deterministic split reduction
__global__ __launch_bounds__(256) void wgrad_sum_kernel(const float* part, int ks, int64_t n, float* dW) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s0 = 0; s0 < ks; s0 += 8) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(part + (size_t)(s0 + u < ks ? s0 + u : s0) * n + i);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (s0 + u < ks) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
  }
  float4 d = *reinterpret_cast<float4*>(dW + i);
  d.x += acc.x; d.y += acc.y; d.z += acc.z; d.w += acc.w;
  *reinterpret_cast<float4*>(dW + i) = d;
}
static int run_wgrads_det(GemmGroup& g, hipStream_t st) {
  // every member writes ks partial matrices [M][N] (plain stores), then one ordered sum per member
  size_t total = 0;
  for (int i = 0; i < g.n; ++i) {
    PS_REQUIRE(g.p[i].ldc == g.p[i].N && (g.p[i].M * (int64_t)g.p[i].N) % 4 == 0 && !g.p[i].bias,
               "deterministic weight gradient: contiguous, bias-free output expected");
    total += (size_t)g.p[i].ksplit * g.p[i].M * g.p[i].N;
  }
  float* sc = det_scratch(total, st);
  PS_REQUIRE(sc, "deterministic mode: no scratch for the split reduction (allocation failed or stream capture)");
  PS_CHECK_HIP(hipMemsetAsync(sc, 0, total * sizeof(float), st));     // splits without slabs (row lists) leave zeros
  float* dW[4]; float* part[4];
  size_t off = 0;
  for (int i = 0; i < g.n; ++i) {
    GemmProblem& p = g.p[i];
    dW[i] = p.C; part[i] = sc + off;
    p.C = part[i]; p.accumulate = 0; p.split_stride = (int64_t)p.M * p.N;
    off += (size_t)p.ksplit * p.M * p.N;
  }
  TRY(ps_launch_gemm(g, st));
  for (int i = 0; i < g.n; ++i) {
    const int64_t n = (int64_t)g.p[i].M * g.p[i].N;
    hipLaunchKernelGGL(wgrad_sum_kernel, dim3((unsigned)ps_cdiv(n / 4, 256)), dim3(256), 0, st, part[i], g.p[i].ksplit, n, dW[i]);
    PS_LAUNCH_CHECK();
  }
  return PS_OK;
}

// (measured and dropped, round 2: a two-pass split reduction — every split stores its partial tile in scratch, takes a ticket,
// the last arriver of a tile adds the partials up in split order — deterministic and free of fp32 atomics, but 122 us against
// 44 for the grouped launch at C2 and 0.395 against 0.292 ms per step: the device-scope release each of the 600 workgroups
// needs before its ticket writes back its XCD's L2, MI300-class L2s not being coherent with one another)
// Groups with row-list members at the item transformer's d = 128 shapes (the deferred K / V / Q / f_W group of the C2 step, the
// K / V / Q group of the unfused paths): every member its own split count, one flat launch (profiles/kvq_wgrad_notes.md).
//   listed member: the host knows the position count only; the list the step really produces holds about a third of it (C2: ~2,900
//     of 8,064).  One split per 288 positions is three 32-row slabs at that length, all three requested before the first is used
//     (ps_launch_gemm, PF = 3); a full list is nine slabs per split, an empty one none — correct at any length.
//   plain member (Q, f_W: one row per sequence): a split per 64 rows (two slabs; with four the Q workgroups were the launch's longest),
//     not one per 32-row slab; at most the 16 the common count gave.
// The common count of the 3-D grid came from the largest K: 16 splits of six serial slabs for K / V on 128 of 256 CUs, and twelve
// one-slab workgroups with a 16 KB atomic tile each for Q and for f_W.  PS_KVQ_SPLIT=0 / ps_set_kvq_split(0): that form.
// Measured at C2 only, so the rule keeps to outputs of at most 128 x 128 and at most 16,384 positions: the review transformer's 78k
// positions and the d = 256 shard keep the common count.  Never in deterministic mode.
static int& kvq_split_slot() { static int v = ps_env_int("PS_KVQ_SPLIT", 1); return v; }
extern "C" int ps_set_kvq_split(int on) { const int was = kvq_split_slot(); kvq_split_slot() = on; return was; }
static int g_kvq_force[2] = {0, 0};      // ps_wgrad_group_test / the sweep: split counts of the listed and the plain members (0: the rule)
static bool kvq_split_takes(const GemmProblem* ps, int n) {
  if (!kvq_split_slot() || ps_deterministic() || n < 2) return false;
  bool listed = false;
  for (int i = 0; i < n; ++i) {
    if (ps[i].M > 128 || ps[i].N > 128 || ps[i].K > 16384 || !(ps[i].ta == 1 && ps[i].tb == 1)) return false;
    listed = listed || ps[i].ridx;
  }
  return listed;
}
static int kvq_ksplit(const GemmProblem& p) {
  static const int diag_listed = ps_diag_int("PS_KVQ_KS", 0), diag_plain = ps_diag_int("PS_KVQ_KS_PLAIN", 0);   // the sweep
  const int forced = p.ridx ? (g_kvq_force[0] ? g_kvq_force[0] : diag_listed) : (g_kvq_force[1] ? g_kvq_force[1] : diag_plain);
  int ks = forced > 0 ? forced : (p.ridx ? ps_cdiv(p.K, 288) : (p.K / 64 < 16 ? p.K / 64 : 16));
  const int need = p.ridx ? ps_cdiv(ps_cdiv(p.K, 32) * 32, PS_GEMM_KIDX_MAX - 32) : 1;     // one split's rows map through LDS
  if (ks < need) ks = need;
  if (forced <= 0 && ks > 8 && ks % 8 != 0) ks = (ks + 7) / 8 * 8;      // GemmGroup::flat_xcd
  return ks < 1 ? 1 : ks;
}

int run_wgrads(GemmProblem* ps, int n, hipStream_t st) {
  GemmGroup g;
  memset(&g, 0, sizeof(g));
  g.n = n;
  bool same = true, plain = true;
  for (int i = 0; i < n; ++i) {
    same = same && ps[i].M == ps[0].M && ps[i].N == ps[0].N && ps[i].K == ps[0].K;
    plain = plain && !ps[i].ridx;
  }
  if (kvq_split_takes(ps, n)) {
    for (int i = 0; i < n; ++i) { g.p[i] = ps[i]; g.p[i].ksplit = kvq_ksplit(ps[i]); }
    g.flat = 1;
    return ps_launch_gemm(g, st);
  }
  if (n > 1 && n <= 3 && !same && plain) {
    // different shapes in one launch: the flat form (GemmGroup::flat) — every problem keeps the split count it would
    // take alone, no idle workgroups for the tiles the smaller members do not have
    for (int i = 0; i < n; ++i) {
      g.p[i] = ps[i];
      g.p[i].ksplit = pick_ksplit(ps_cdiv(ps[i].M, 64) * ps_cdiv(ps[i].N, 64), ps[i].K);
    }
    g.flat = 1;
    if (ps_deterministic()) return run_wgrads_det(g, st);
    KTimeScope kt("wgrad_group", st);
    return ps_launch_gemm(g, st);
  }
  int tiles = 0, rows = 0;
  for (int i = 0; i < n; ++i) {
    tiles += ps_cdiv(ps[i].M, 64) * ps_cdiv(ps[i].N, 64);
    rows = ps[i].K > rows ? ps[i].K : rows;
  }
  int ks = pick_ksplit(tiles, rows);
  // Big weight gradients (the d = 256 step's W2 / W1: 16 tiles of 128 x 128 over 21,504 reduction rows) take the direct-to-LDS
  // bf16x3 kernel with 128x128 tiles and ~512 workgroups: 104-109 us against 129-131 for the 64x64 tiles at ANY split count
  // (MI355X, profiles/r04_gemm_wgrad_ksplit.txt) — half the operand bytes per flop through LDS, a quarter of the atomic tiles'
  // row segments.  Few tiles (Wo: 4) or few rows (C2: 8,064) cannot fill the chip that way and keep the 64x64 form.
  {
    int t128 = 0;
    for (int i = 0; i < n; ++i) t128 += ps_cdiv(ps[i].M, 128) * ps_cdiv(ps[i].N, 128);
    const int by_rows = ps_cdiv(rows, 512), by_fill = 512 / (t128 > 0 ? t128 : 1);
    const int ks3 = by_rows < by_fill ? by_rows : by_fill;
    if (plain && gemm_x3_on() && !ps_deterministic() && t128 * ks3 >= 384 && rows % 32 == 0) { ks = ks3; g.prefer_x3d = 1; }
  }
  for (int i = 0; i < n; ++i)
    if (ps[i].ridx) {   // a row-list problem maps one split's reduction rows through LDS: at most PS_GEMM_KIDX_MAX of them
      const int need = ps_cdiv(ps_cdiv(ps[i].K, 32) * 32, PS_GEMM_KIDX_MAX - 32);
      if (ks < need) ks = need;
    }
  // a split count that is a multiple of 8 lets the launch place every split's tiles on one XCD (GemmGroup::split_xcd / flat_xcd)
  static const int ks_round8 = ps_diag_int("PS_KS_ROUND8", 1);
  if (ks_round8 && ks > 8 && ks % 8 != 0 && !ps_deterministic()) ks = (ks + 7) / 8 * 8;
  for (int i = 0; i < n; ++i) { g.p[i] = ps[i]; g.p[i].ksplit = ks; }
  if (ps_deterministic() && ks > 1) return run_wgrads_det(g, st);
  return ps_launch_gemm(g, st);
}

int side_run(GemmProblem* ps, int n, hipStream_t main_st) {
  return run_wgrads(ps, n, side_stream_or(main_st));
}
int side_wgrads(GemmProblem* ps, int n, hipStream_t main_st) {
  TRY(side_fork(main_st));
  return side_run(ps, n, main_st);
}

// Test hook (tests/test_gpu_wgrad_listed.py): one weight-gradient group from raw pointers through run_wgrads.  Member i:
// dW[i][n_out, k_in] += dY[i][rows[i], n_out]^T . X[i][rows[i], k_in]; listed[i] != 0: over the *rcount rows ridx[0..] only (rows[i]
// bounds the list).  ks_listed / ks_plain > 0 replace the rule's split counts where the per-member form is taken.
extern "C" int ps_wgrad_group_test(int n, const float* const* dY, const float* const* X, float* const* dW, const int32_t* rows,
                                   const int32_t* listed, const int32_t* ridx, const int32_t* rcount, int n_out, int k_in,
                                   int ks_listed, int ks_plain, ps_stream_t stream) {
  PS_REQUIRE(n >= 1 && n <= 4 && ks_listed >= 0 && ks_plain >= 0, "wgrad group test: %d members", n);
  GemmProblem ps[4];
  for (int i = 0; i < n; ++i) {
    ps[i] = gp_wgrad(dY[i], n_out, X[i], k_in, dW[i], n_out, k_in, rows[i]);
    if (listed[i]) { PS_REQUIRE(ridx && rcount, "wgrad group test: listed member without a list"); ps[i].ridx = ridx; ps[i].rcount = rcount; }
  }
  g_kvq_force[0] = ks_listed; g_kvq_force[1] = ks_plain;
  const int rc = run_wgrads(ps, n, (hipStream_t)stream);
  g_kvq_force[0] = g_kvq_force[1] = 0;
  return rc;
}
