// gemm_kernels.hip — the four GEMM kernel families, each followed by its launch switch (launch_f32, launch_x3, launch_x3d,
// launch_x3w: the plan's (ta, tb, full, idx, ...) -> template instantiation); the epilogues they share: gemm.h; which launch takes
// which: gemm.hip.  One translation unit on purpose: compiled apart, hipcc allocates registers differently in one fp32 kernel and
// commutes the operands of the plain epilogue's v_add_f32 in seven bf16x3 kernels (profiles/gemm_plan_forms.md).
//
// The exact-fp32 MFMA GEMM with fused epilogues (gfx950).
//
// The only dense contractions of the hot path are the transformer's linears
// (reference models/neural.py:86-96 K/V/Q/final_linear, :20-21 w_1/w_2, and
// text_encoder.py:24 f_W) and their two backward products.  They are computed
// with v_mfma_f32_32x32x2_f32 (f32 in / f32 accumulate = a k-ordered fmaf chain,
// so results are exact fp32 like the reference's mm), tiled for 64-wide waves:
//
//   workgroup = 4 waves, tile 64x64 (each wave one 32x32 accumulator = 16 AGPRs);
//   the reduction advances in slabs of 32 (128 for launches of few workgroups: the hot path's K
//   is d = 128, so a whole projection is then ONE global->register->LDS round trip followed by
//   64 back-to-back MFMAs per wave); the next slabs are prefetched into registers while the
//   current one is multiplied — which only holds if nothing touches the loaded registers before
//   the LDS store (see tile_load: a zero-fill select, a scratch-resident segment table or a load
//   under a branch each made the compiler drain vmcnt BEFORE the MFMA block; fixing the three
//   took the step from 0.51 to 0.46 ms); operands sit in LDS as [k][row+1] so every MFMA operand
//   fetch is a conflict-free ds_read_b32 per lane.
//
// One kernel serves forward (A[m][k] . W[n][k]), input-grad (dY[m][n] . W[n][k'])
// and weight-grad (dY[m][n]^T . X[m][k'], split over the row reduction with fp32
// atomics) through (ta, tb) layouts.  Two epilogue instantiations keep the code in
// the instruction cache: PLAIN (bias, scale, store / += / atomic) and FULL (adds
// GELU/tanh or their derivatives, Philox dropout, residual direct / gathered from
// the layer input / fan-in summed over replicas, bias-grad column sums, 2nd output),
// whose body is a rolled loop over an LDS-staged tile so it exists once in the code.
//
// Measured alternatives (MI355X, tools/gemm_bench.py): a 128x128 tile with 2x2 accumulators per wave (half the LDS and
// L2 bytes per flop) is SLOWER on every hot shape — K is only 128-512 deep, so a workgroup's life is 4-16 slabs and the
// larger tile just has fewer workgroups to hide its fill/drain behind (78k x 256 x 128: 92 vs 80 us; 78k x 128 x 128:
// 66 vs 44 us; weight gradients over 78k rows: 65 vs 49 us).  128-deep slabs for every launch cost the review
// transformer 15 % (one workgroup per CU).
#include "gemm.h"
#include <string.h>

// TRANS==0: src[row][k] (k contiguous): one instruction = 8 rows x 128 B
// TRANS==1: src[k][row] (row contiguous): one instruction = 4 k-rows x 256 B

// BK = reduction depth of one slab (32 or 128); NLD = float4 loads per thread per operand per slab.
// The loaded registers must not be touched before the slab is stored to LDS, or the compiler waits for the loads
// BEFORE the MFMAs of the current slab and the prefetch overlaps nothing (it did: a v_cndmask zero-fill per load put
// s_waitcnt vmcnt(0) ahead of the MFMA block).  So rows are clamped instead of masked — rows past the edge are
// duplicates whose products land in output rows/columns the epilogue never stores — and only a ragged reduction
// tail (kmask: K not a multiple of the slab, block-uniform) takes the zero-filling path.
// pr0 / pr1 (TRANS == 0, row list; -1: none): the two physical rows this thread loads from, fetched once per workgroup.
// kmap (TRANS == 1, row list): LDS copy of the physical reduction rows of this workgroup's range, kmap[k - kbase].
template <int TRANS, int BK>
__device__ inline void tile_load(const float* __restrict__ src, int ld, int row0, int nrows, int k0, int kend,
                                 float4 (&reg)[BK / 16], int tid, bool kmask, const float* __restrict__ seg1 = nullptr,
                                 const float* __restrict__ seg2 = nullptr, int kseg = 0, int pr0 = -1, int pr1 = -1,
                                 const int* kmap = nullptr, int kbase = 0) {
  constexpr int NLD = BK / 16;
#pragma unroll
  for (int u = 0; u < NLD; ++u) {
    int r, k;
    if (TRANS == 0) {
      r = pr0 >= 0 ? ((u & 1) ? pr1 : pr0) : min(row0 + (tid >> 3) + 32 * (u & 1), nrows - 1);   // u is compile-time
      k = k0 + 32 * (u >> 1) + 4 * (tid & 7);
    } else {
      r = min(row0 + 4 * (tid & 15), nrows - 4);              // nrows % 4 == 0 (validated)
      k = k0 + (tid >> 4) + 16 * u;
    }
    const bool ok = !kmask || k < kend;
    int kl = ok ? k : k0;
    if (TRANS == 1 && kmap) kl = kmap[kl - kbase];
    const float* base = src;
    if (kseg > 0) {                            // K-concatenated operand (kseg > 0): pick the segment of this k.  Plain
      const int sg = (kl >= kseg) + (kl >= 2 * kseg);   // scalars, no table: a table indexed per lane lives in scratch,
      base = sg == 0 ? src : (sg == 1 ? seg1 : seg2);   // whose loads share vmcnt with the tile loads and serialise them
      kl -= sg * kseg;
    }
    const size_t off = TRANS == 0 ? (size_t)r * ld + kl : (size_t)kl * ld + r;
    reg[u] = *reinterpret_cast<const float4*>(base + off);    // raw: tile_store zero-fills a ragged tail
  }
}

template <int TRANS, int BK>
__device__ inline void tile_store(float (*T)[LDT], const float4 (&reg)[BK / 16], int tid, bool kmask, int k0, int kend) {
  constexpr int NLD = BK / 16;
#pragma unroll
  for (int u = 0; u < NLD; ++u) {
    float4 v = reg[u];
    if (TRANS == 0) {
      const int i = (tid >> 3) + 32 * (u & 1), kk = 32 * (u >> 1) + 4 * (tid & 7);
      if (kmask && k0 + kk >= kend) v = make_float4(0.f, 0.f, 0.f, 0.f);
      T[kk + 0][i] = v.x;
      T[kk + 1][i] = v.y;
      T[kk + 2][i] = v.z;
      T[kk + 3][i] = v.w;
    } else {
      const int kk = (tid >> 4) + 16 * u, i = 4 * (tid & 15);
      if (kmask && k0 + kk >= kend) v = make_float4(0.f, 0.f, 0.f, 0.f);
      T[kk][i + 0] = v.x;
      T[kk][i + 1] = v.y;
      T[kk][i + 2] = v.z;
      T[kk][i + 3] = v.w;
    }
  }
}

// diagnostics (PS_GEMM_STAMP=2 / 3, tools/gemm_f32_stamps.py): s_memtime of the four waves of workgroup (0, 8, 0) at the phase
// boundaries of the fp32 kernel — the step's own dX product over the row list (2) or its K/V projection (3); 5 (GemmGroup::stamp_kvq):
// one listed and one plain workgroup of the deferred K / V / Q / f_W weight gradients, chosen once the decode knows who they are
#if PS_DIAG_ON      // in-kernel phase stamps: diagnostic build only
#define F32_NOW(t_) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory")
#define F32_STAMP(slot)                                                                                              \
  do {                                                                                                               \
    if (stamp_off >= 0 && (threadIdx.x & 63) == 0) {                                                                 \
      unsigned long long t_;                                                                                         \
      F32_NOW(t_);                                                                                                   \
      if ((slot) < 32) g.stamp[stamp_off + 32 * (threadIdx.x >> 6) + (slot)] = t_;                                   \
    }                                                                                                                \
  } while (0)
#else
#define F32_STAMP(slot) do { } while (0)
#endif
template <int TA, int TB, int FULL, int BK, int PF, int IDX = 0>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const GemmGroup g) {
  fork_signal(g.sig, g.sigval);
#if PS_DIAG_ON
  int stamp_off = (g.stamp && !g.stamp_kvq && blockIdx.x == 0 && blockIdx.y == 8 && blockIdx.z == 0) ? 0 : -1;
  unsigned long long stamp_t0 = 0;
  if (g.stamp && g.stamp_kvq) F32_NOW(stamp_t0);
#endif
  F32_STAMP(0);
  constexpr int NLD = BK / 16;
  __shared__ float As[2][BK][LDT];
  __shared__ float Bs[2][BK][LDT];
  __shared__ int kidx[IDX && TA == 1 ? KIDX_MAX : 1];
  __shared__ int rows_s[IDX && TA == 0 ? BM : 1];

  int prob, split, ftile = 0;
  if (g.flat) {
    const int L = blockIdx.x;
    prob = L >= g.flat0[3] ? 3 : (L >= g.flat0[2] ? 2 : (L >= g.flat0[1] ? 1 : 0));
    const int t = L - g.flat0[prob];
    if ((g.flat_xcd >> prob) & 1) {
      const int s8 = t >> 3, grp = s8 / g.flat_tiles[prob];
      split = (t & 7) + 8 * grp;
      ftile = s8 - grp * g.flat_tiles[prob];
    } else {
      split = t / g.flat_tiles[prob];
      ftile = t - split * g.flat_tiles[prob];
    }
  } else if (g.split_xcd) {       // 3-D grid of a split reduction: all tiles of a split on one XCD, as GemmGroup::flat_xcd does it
    const int T = gridDim.x * gridDim.y, ks = g.p[0].ksplit;
    const int Lz = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;       // dispatch order
    prob = Lz / (T * ks);
    const int t = Lz - prob * T * ks, s8 = t >> 3, grp = s8 / T;
    split = (t & 7) + 8 * grp;
    ftile = s8 - grp * T;
  } else {
    prob = blockIdx.z / g.p[0].ksplit;
    split = blockIdx.z - prob * g.p[0].ksplit;
  }
  const GemmProblem& P = g.p[prob];
  const bool listed = IDX && P.ridx != nullptr;                 // block-uniform
  // XCD-aware tile mapping: workgroups are dealt round-robin over the 8 XCDs (each with its own L2),
  // so give every XCD whole ROW tiles: all column tiles that re-read one A row-tile share an L2.
  int tm = blockIdx.y, tn = blockIdx.x;
  if (g.flat) {
    tm = ftile % g.flat_tm[prob];
    tn = ftile / g.flat_tm[prob];
  } else if (g.split_xcd) {
    tm = ftile % (int)gridDim.y;
    tn = ftile / (int)gridDim.y;
  } else {
    const int nx = gridDim.x, ny = gridDim.y;
    const int L = blockIdx.y * nx + blockIdx.x;       // dispatch order (x fastest)
    const int grp = L / (8 * nx), r = L - grp * 8 * nx;
    const int rows_here = min(8, ny - grp * 8);
    tm = grp * 8 + r % rows_here;
    tn = r / rows_here;
  }
  const int m0 = tm * BM, n0 = tn * BN;
#if PS_DIAG_ON
  if (g.stamp && g.stamp_kvq && split == 1 && tm == 0 && tn == 0 && (prob == 0 || prob == 2)) {
    stamp_off = 256 + 64 * prob;
    if ((threadIdx.x & 63) == 0) g.stamp[stamp_off + 32 * (threadIdx.x >> 6)] = stamp_t0;
  }
#endif
  // row list, ta == 0: the tile's 64 list entries are fetched NOW, beside the list length (the list has room for P.M
  // entries, common.h; what lies past the length is never used), and kept in LDS for the operand loads and the epilogue
  // — after the length they were a second dependent round trip here and a third in front of every epilogue row group
  int my_row = 0;
  if (IDX && TA == 0 && listed && threadIdx.x < BM) my_row = P.ridx[min(m0 + (int)threadIdx.x, P.M - 1)];
  const int nlist = listed ? *P.rcount : 0;
  const int M = (listed && TA == 0) ? nlist : P.M, N = P.N, K = (listed && TA == 1) ? nlist : P.K;
  const int nslab = (K + BK - 1) / BK;
  const int per = (nslab + P.ksplit - 1) / P.ksplit;
  const int kbeg = split * per * BK;
  const int kend = min(K, kbeg + per * BK);
  if (m0 >= M || n0 >= N || kbeg >= kend) return;   // block-uniform
  F32_STAMP(1);
  const bool kmask = (kend - kbeg) % BK != 0;       // ragged reduction tail (never on the hot shapes)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, h = lane >> 5;

  int pr0 = -1, pr1 = -1;
  const int* kmap = nullptr;
  if (IDX && TA == 0) {                                         // the two A rows this thread loads, once (plain
    pr0 = min(m0 + (tid >> 3), M - 1);                          // problems of a row-list launch: the natural rows)
    pr1 = min(m0 + (tid >> 3) + 32, M - 1);
    if (listed) {
      if (tid < BM) rows_s[tid] = my_row;
      __syncthreads();
      pr0 = rows_s[pr0 - m0]; pr1 = rows_s[pr1 - m0];
    }
  }
  if (listed && TA == 1) {                                      // physical reduction rows of this split -> LDS
    for (int i = tid; i < kend - kbeg; i += 256) kidx[i] = P.ridx[kbeg + i];
    __syncthreads();
    kmap = kidx;
  }
  const int* const rows_l = (IDX && TA == 0 && listed) ? rows_s : nullptr;
  F32_STAMP(2);

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  // PF slabs are in flight in registers (slot u holds slab  u  mod PF of the current group): with one workgroup per
  // CU — the 8k-row shapes of the step — a single slab of prefetch (1024 MFMA cycles) does not cover a global round trip
  float4 ra[PF][NLD], rb[PF][NLD];
  const int ldb = P.ldb;
  const float* const bs0 = P.Bseg[0];
  const float* const bs1 = P.Bseg[1];
  const float* const bs2 = P.Bseg[2];
  const int bkseg = K > P.kseg ? P.kseg : 0;          // 0: B is one segment

  // every slot load is UNCONDITIONAL (past the end it re-reads the first slab, a cache hit whose result is dropped): a
  // load under a branch makes the number of loads in flight unknown at the join, and the compiler then waits for all
  // of them (vmcnt(0)) where vmcnt(4*(PF-1)) is enough
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const int kl = kbeg + u * BK < kend ? kbeg + u * BK : kbeg;
    tile_load<TA, BK>(P.A, P.lda, m0, M, kl, kend, ra[u], tid, kmask, nullptr, nullptr, 0, pr0, pr1, kmap, kbeg);
    tile_load<TB, BK>(bs0, ldb, n0, N, kl, kend, rb[u], tid, kmask, bs1, bs2, bkseg, -1, -1, TA == 1 ? kmap : nullptr, kbeg);
  }
  F32_STAMP(3);
  tile_store<TA, BK>(As[0], ra[0], tid, kmask, kbeg, kend);
  tile_store<TB, BK>(Bs[0], rb[0], tid, kmask, kbeg, kend);
  __syncthreads();
  F32_STAMP(4);

  int buf = 0;
  for (int kg = kbeg; kg < kend; kg += PF * BK) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int k0 = kg + u * BK;
      if (k0 >= kend) break;                         // block-uniform
      const int kp = k0 + PF * BK < kend ? k0 + PF * BK : kbeg;   // slot u is free (its slab sits in LDS): refill it
      tile_load<TA, BK>(P.A, P.lda, m0, M, kp, kend, ra[u], tid, kmask, nullptr, nullptr, 0, pr0, pr1, kmap, kbeg);            // PF slabs ahead
      tile_load<TB, BK>(bs0, ldb, n0, N, kp, kend, rb[u], tid, kmask, bs1, bs2, bkseg, -1, -1, TA == 1 ? kmap : nullptr, kbeg);
      const float* a_base = &As[buf][h][wm * 32 + l31];
      const float* b_base = &Bs[buf][h][wn * 32 + l31];
#pragma unroll
      for (int q = 0; q < BK / 32; ++q) {
        float av[16], bv[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          av[s] = a_base[(32 * q + 2 * s) * LDT];
          bv[s] = b_base[(32 * q + 2 * s) * LDT];
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
      }
      if (k0 + BK < kend) {
        const int nx = (u + 1) % PF;                 // compile-time after unrolling
        tile_store<TA, BK>(As[buf ^ 1], ra[nx], tid, kmask, k0 + BK, kend);
        tile_store<TB, BK>(Bs[buf ^ 1], rb[nx], tid, kmask, k0 + BK, kend);
      }
      __syncthreads();
      F32_STAMP(5 + (k0 - kbeg) / BK);
      buf ^= 1;
    }
  }

  // ------------------------------------------------------------------ epilogue
  if (!FULL) {
    epi_plain<TA, IDX>(P, acc, m0, n0, split, M, N, listed, wm, wn, l31, h, rows_l);
    F32_STAMP(31);
    return;
  }
  // FULL: stage the 64x64 tile through LDS so that the (large) epilogue body exists ONCE in the
  // instruction stream: thread t owns column t&63 and rows 4*((t>>6)+4i)+q  (i,q < 4); the four q-rows
  // of one i share a Philox call (counter (col, row>>2), word row&3); stores are 256-B coalesced.
  float (*Ct)[LDT] = reinterpret_cast<float (*)[LDT]>(&As[0][0][0]);   // 64x65 floats fit As for BK >= 32
  epi_stage(Ct, acc, wm, wn, l31, h);
  __syncthreads();
  F32_STAMP(30);
  epi_full<TA, IDX>(P, Ct, m0, n0, tm, split, M, N, listed, tid, rows_l);
  F32_STAMP(31);
}

// ---- the plan's (ta, tb, full, idx, bk, pf) -> instantiation.  Plain launches: every layout and epilogue, as 32-deep slabs with two in
// flight or one 128-deep slab, and the weight-gradient layout with 3 / 4 in flight (PS_WGRAD_PF); row lists: the three shapes of the
// step that use them, the K / V projection also as one deep slab, the flat weight-gradient groups with three slabs in flight.
template <int TA, int TB, int FULL>
static void go_plain(const GemmPlan& pl, const GemmGroup& g, hipStream_t st) {
  if (pl.bk == 128) gemm_go(gemm_f32_kernel<TA, TB, FULL, 128, 1>, pl, g, st);
  else gemm_go(gemm_f32_kernel<TA, TB, FULL, 32, 2>, pl, g, st);
}
void launch_f32(const GemmPlan& pl, const GemmGroup& g, hipStream_t st) {
  if (!pl.idx && pl.pf == 4) return gemm_go(gemm_f32_kernel<1, 1, 0, 32, 4>, pl, g, st);
  if (!pl.idx && pl.pf == 3) return gemm_go(gemm_f32_kernel<1, 1, 0, 32, 3>, pl, g, st);
  switch (gemm_key(pl.ta, pl.tb, pl.full, pl.idx)) {
    case gemm_key(0, 0, 0, 0): return go_plain<0, 0, 0>(pl, g, st);
    case gemm_key(0, 0, 1, 0): return go_plain<0, 0, 1>(pl, g, st);
    case gemm_key(0, 1, 0, 0): return go_plain<0, 1, 0>(pl, g, st);
    case gemm_key(0, 1, 1, 0): return go_plain<0, 1, 1>(pl, g, st);
    case gemm_key(1, 0, 0, 0): return go_plain<1, 0, 0>(pl, g, st);
    case gemm_key(1, 0, 1, 0): return go_plain<1, 0, 1>(pl, g, st);
    case gemm_key(1, 1, 0, 0): return go_plain<1, 1, 0>(pl, g, st);
    case gemm_key(1, 1, 1, 0): return go_plain<1, 1, 1>(pl, g, st);
    case gemm_key(0, 1, 1, 1): return gemm_go(gemm_f32_kernel<0, 1, 1, 32, 2, 1>, pl, g, st);
    case gemm_key(1, 1, 0, 1):
      if (pl.pf == 3) return gemm_go(gemm_f32_kernel<1, 1, 0, 32, 3, 1>, pl, g, st);
      return gemm_go(gemm_f32_kernel<1, 1, 0, 32, 2, 1>, pl, g, st);
    case gemm_key(0, 0, 0, 1):
      if (pl.bk == 128) return gemm_go(gemm_f32_kernel<0, 0, 0, 128, 1, 1>, pl, g, st);
      return gemm_go(gemm_f32_kernel<0, 0, 0, 32, 2, 1>, pl, g, st);
  }
}

// ====================================================================== bf16x3 product form
// v_mfma_f32_32x32x2_f32 runs at the fp32 vector rate (4,445 cycles per 32x32x128 product); the same product as SIX
// v_mfma_f32_32x32x16_bf16 over a three-way bf16 split of both operands (x = hi + mid + lo: 3 x 8 = 24 mantissa bits, an
// exact decomposition;  hl + lh + mm + hm + mh + hh, fp32 accumulation) costs 1,457 and is as accurate (max error /
// sum|a b| against fp64: 1.10e-7, the fp32 MFMA's own 1.13e-7 — tools/micro/bf16x3.hip, profiles/r02_mlp_notes.md).
// This kernel is gemm_f32_kernel with that product for the large launches (the d = 256 step's linears over 21,504 rows,
// the review transformer's over 78k): tile (64 MT) x (64 NT), each of the 4 waves owns the 32x32 accumulator (wm, wn) of
// every 64x64 quadrant — so the epilogues above serve unchanged, quadrant by quadrant — 32-deep slabs; fp32 operands
// are fetched one slab ahead into registers, split on their way into LDS (three planes per operand, [row][32 k] bf16,
// 16-byte chunks XOR-swizzled by (row >> 2) & 3 so that ds_read_b128 by its lane groups and ds_write_b128 by 8-lane
// groups are conflict-free), and read back as whole MFMA operands (one ds_read_b128 per plane and 32 rows x 16 k).

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define X3K 32

__device__ __forceinline__ int x3g_off(int row, int chunk) { return row * X3K + ((chunk ^ ((row >> 2) & 3)) << 3); }

// two adjacent reduction elements -> one packed pair per plane.  Non-finite operands: hi carries the Inf / NaN and the residual
// Inf - Inf = NaN follows it, so every output the operand reaches is NON-FINITE, as with the fp32 MFMA — but its class is NaN
// where the fp32 kernel gives +-Inf (the form's own terms Inf * b_hi and Inf * b_mid have opposite signs: no split of b can
// preserve the class); tests/test_gpu_gemm_x3.py pins exactly this
__device__ __forceinline__ void x3g_split2(float x0, float x1, uint32_t& hi, uint32_t& mi, uint32_t& lo) {
  f32x2 v = {x0, x1};
  bf16x2 b = __builtin_convertvector(v, bf16x2);                         // v_cvt_pk_bf16_f32 (round to nearest even)
  hi = __builtin_bit_cast(uint32_t, b);
  v -= f32x2{__uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};   // v_pk_add_f32: exact
  b = __builtin_convertvector(v, bf16x2);
  mi = __builtin_bit_cast(uint32_t, b);
  v -= f32x2{__uint_as_float(mi << 16), __uint_as_float(mi & 0xffff0000u)};
  b = __builtin_convertvector(v, bf16x2);
  lo = __builtin_bit_cast(uint32_t, b);
}
// eight consecutive reduction elements of one tile row -> its 16-byte chunk in each plane
template <int R>
__device__ __forceinline__ void x3g_put8(uint16_t* planes, int row, int chunk, const float (&v)[8]) {
  uint32_t H[4], Mi[4], Lo[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) x3g_split2(v[2 * e], v[2 * e + 1], H[e], Mi[e], Lo[e]);
  uint16_t* dst = planes + x3g_off(row, chunk);
  *reinterpret_cast<uint4*>(dst) = make_uint4(H[0], H[1], H[2], H[3]);
  *reinterpret_cast<uint4*>(dst + R * X3K) = make_uint4(Mi[0], Mi[1], Mi[2], Mi[3]);
  *reinterpret_cast<uint4*>(dst + 2 * R * X3K) = make_uint4(Lo[0], Lo[1], Lo[2], Lo[3]);
}
// One operand slab (R tile rows x 32 reduction elements) global -> registers, R / 8 floats per thread.
//   TRANS == 0 (src[row][k]): thread = (row, 8-element chunk): q = tid + 256 u, row q >> 2, chunk q & 3: two float4
//   TRANS == 1 (src[k][row]): wave w takes reduction elements 8 w .. 8 w + 7, lane l the R / 64 adjacent rows at (R / 64) l
//                             (their 16-byte LDS stores are 2-way conflicts: 16 LDS-array cycles under a 13-cycle store)
//                             (measured alternative for weight gradients: waves 0-1 fetch A, waves 2-3 B, four float4 loads of
//                             4 rows x 4 reduction elements per thread and 8-byte LDS stores — 1024x256x21504: 120 -> 115 us,
//                             256x256x21504: 55 -> 63 us, 128x384x78336: 164 -> 197 us, C2 step unchanged: not kept)
// Rows are clamped (duplicates land in outputs the epilogue never stores), reduction indices past the end too (x3g_store
// zero-fills them); the loads are unconditional and untouched until the store (see tile_load).
template <int TRANS, int R>
__device__ __forceinline__ void x3g_load(const float* __restrict__ src, int ld, int row0, int nrows, int k0, int kend,
                                         bool kmask, float (&reg)[R / 8], int tid, const float* __restrict__ seg1,
                                         const float* __restrict__ seg2, int kseg, int pr0, int pr1, const int* kmap,
                                         int kbase) {
  if (TRANS == 0) {
#pragma unroll
    for (int u = 0; u < R / 64; ++u) {
      const int q = tid + 256 * u, row = q >> 2, c = q & 3;
      const int r = pr0 >= 0 ? (u ? pr1 : pr0) : min(row0 + row, nrows - 1);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        int kl = min(k0 + 8 * c + 4 * j, kend - 4);              // (kend % 4 == 0: validated)
        const float* base = src;
        if (kseg > 0) {
          const int sg = (kl >= kseg) + (kl >= 2 * kseg);
          base = sg == 0 ? src : (sg == 1 ? seg1 : seg2);
          kl -= sg * kseg;
        }
        const float4 t = *reinterpret_cast<const float4*>(base + (size_t)r * ld + kl);
        reg[8 * u + 4 * j + 0] = t.x; reg[8 * u + 4 * j + 1] = t.y; reg[8 * u + 4 * j + 2] = t.z; reg[8 * u + 4 * j + 3] = t.w;
      }
    }
  } else {
    constexpr int RPT = R / 64;
    const int w = tid >> 6;
    const int r = min(row0 + RPT * (tid & 63), nrows - RPT);      // nrows % 4 == 0 (validated)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int kl = min(k0 + 8 * w + j, kend - 1);
      if (kmap) kl = kmap[kl - kbase];
      const float* base = src;
      if (kseg > 0) {
        const int sg = (kl >= kseg) + (kl >= 2 * kseg);
        base = sg == 0 ? src : (sg == 1 ? seg1 : seg2);
        kl -= sg * kseg;
      }
      if (RPT == 2) {
        const float2 t = *reinterpret_cast<const float2*>(base + (size_t)kl * ld + r);
        reg[2 * j] = t.x; reg[2 * j + 1] = t.y;
      } else {
        reg[j] = base[(size_t)kl * ld + r];
      }
    }
  }
}
template <int TRANS, int R, bool KMASK>
__device__ __forceinline__ void x3g_store_impl(uint16_t* planes, const float (&reg)[R / 8], int tid, int k0, int kend) {
  if (TRANS == 0) {
#pragma unroll
    for (int u = 0; u < R / 64; ++u) {
      const int q = tid + 256 * u, row = q >> 2, c = q & 3;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (KMASK && k0 + 8 * c + e >= kend) ? 0.f : reg[8 * u + e];
      x3g_put8<R>(planes, row, c, v);
    }
  } else {
    constexpr int RPT = R / 64;
    const int w = tid >> 6;
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (KMASK && k0 + 8 * w + j >= kend) ? 0.f : reg[RPT * j + u];
      x3g_put8<R>(planes, RPT * (tid & 63) + u, w, v);
    }
  }
}
// (the zero-fill of a ragged last slab as selects in the common path cost ~100 vector instructions per slab: a block-uniform branch)
template <int TRANS, int R>
__device__ __forceinline__ void x3g_store(uint16_t* planes, const float (&reg)[R / 8], int tid, bool kmask, int k0, int kend) {
  if (kmask && k0 + X3K > kend) x3g_store_impl<TRANS, R, true>(planes, reg, tid, k0, kend);
  else x3g_store_impl<TRANS, R, false>(planes, reg, tid, k0, kend);
}

#if PS_DIAG_ON      // in-kernel phase stamps: diagnostic build only
#define GEMM_STAMP(slot)                                                                                             \
  do {                                                                                                               \
    if (g.stamp && blockIdx.x == 0 && blockIdx.y == gridDim.y / 2 && blockIdx.z == 0 && (threadIdx.x & 63) == 0) {   \
      unsigned long long t_;                                                                                         \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                                     \
      if ((slot) < 32) g.stamp[32 * (threadIdx.x >> 6) + (slot)] = t_;                                               \
    }                                                                                                                \
  } while (0)
#else
#define GEMM_STAMP(slot) do { } while (0)
#endif
template <int TA, int TB, int FULL, int MT, int NT, int IDX, int PF = 1>
__global__ __launch_bounds__(256, 2) void gemm_x3_kernel(const GemmGroup g) {
  fork_signal(g.sig, g.sigval);
  GEMM_STAMP(0);
  constexpr int RA = 64 * MT, RB = 64 * NT;
  constexpr int MAIN_BYTES = 3 * (RA + RB) * X3K * 2;
  constexpr int EPI_BYTES = FULL ? MT * NT * 64 * LDT * 4 : 16;
  __shared__ __attribute__((aligned(16))) unsigned char smem[MAIN_BYTES > EPI_BYTES ? MAIN_BYTES : EPI_BYTES];
  __shared__ int kidx[IDX && TA == 1 ? KIDX_MAX : 1];
  uint16_t* const As = reinterpret_cast<uint16_t*>(smem);
  uint16_t* const Bs = As + 3 * RA * X3K;

  int prob, split, ftile = 0;
  if (g.flat) {
    const int L = blockIdx.x;
    prob = L >= g.flat0[3] ? 3 : (L >= g.flat0[2] ? 2 : (L >= g.flat0[1] ? 1 : 0));
    const int t = L - g.flat0[prob];
    if ((g.flat_xcd >> prob) & 1) {
      const int s8 = t >> 3, grp = s8 / g.flat_tiles[prob];
      split = (t & 7) + 8 * grp;
      ftile = s8 - grp * g.flat_tiles[prob];
    } else {
      split = t / g.flat_tiles[prob];
      ftile = t - split * g.flat_tiles[prob];
    }
  } else if (g.split_xcd) {       // 3-D grid of a split reduction: all tiles of a split on one XCD, as GemmGroup::flat_xcd does it
    const int T = gridDim.x * gridDim.y, ks = g.p[0].ksplit;
    const int Lz = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;       // dispatch order
    prob = Lz / (T * ks);
    const int t = Lz - prob * T * ks, s8 = t >> 3, grp = s8 / T;
    split = (t & 7) + 8 * grp;
    ftile = s8 - grp * T;
  } else {
    prob = blockIdx.z / g.p[0].ksplit;
    split = blockIdx.z - prob * g.p[0].ksplit;
  }
  const GemmProblem& P = g.p[prob];
  const bool listed = IDX && P.ridx != nullptr;                 // block-uniform
  const int nlist = listed ? *P.rcount : 0;
  const int M = (listed && TA == 0) ? nlist : P.M, N = P.N, K = (listed && TA == 1) ? nlist : P.K;
  int tm, tn;                                                    // XCD-aware tile mapping as in gemm_f32_kernel
  if (g.flat) {
    tm = ftile % g.flat_tm[prob];
    tn = ftile / g.flat_tm[prob];
  } else if (g.split_xcd) {
    tm = ftile % (int)gridDim.y;
    tn = ftile / (int)gridDim.y;
  } else {
    const int nx = gridDim.x, ny = gridDim.y;
    const int L = blockIdx.y * nx + blockIdx.x;
    const int grp = L / (8 * nx), r = L - grp * 8 * nx;
    const int rows_here = min(8, ny - grp * 8);
    tm = grp * 8 + r % rows_here;
    tn = r / rows_here;
  }
  const int m0 = tm * RA, n0 = tn * RB;
  const int nslab = (K + X3K - 1) / X3K;
  const int per = (nslab + P.ksplit - 1) / P.ksplit;
  const int kbeg = split * per * X3K;
  const int kend = min(K, kbeg + per * X3K);
  if (m0 >= M || n0 >= N || kbeg >= kend) return;   // block-uniform
  const bool kmask = (kend - kbeg) % X3K != 0;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, h = lane >> 5;

  int pr0 = -1, pr1 = -1;
  const int* kmap = nullptr;
  if (IDX && TA == 0) {                                         // the A rows this thread loads, once
    pr0 = min(m0 + (tid >> 2), M - 1);
    pr1 = min(m0 + (tid >> 2) + 64, M - 1);
    if (listed) { pr0 = P.ridx[pr0]; pr1 = P.ridx[pr1]; }
  }
  if (listed && TA == 1) {                                      // physical reduction rows of this split -> LDS
    for (int i = tid; i < kend - kbeg; i += 256) kidx[i] = P.ridx[kbeg + i];
    __syncthreads();
    kmap = kidx;
  }

  f32x16 acc[MT][NT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  // PF slabs in flight in registers (slot u holds slab u mod PF of the current group), every load unconditional — see gemm_f32_kernel
  float ra[PF][RA / 8], rb[PF][RB / 8];
  const int ldb = P.ldb;
  const float* const bs0 = P.Bseg[0];
  const float* const bs1 = P.Bseg[1];
  const float* const bs2 = P.Bseg[2];
  const int bkseg = K > P.kseg ? P.kseg : 0;          // 0: B is one segment
#pragma unroll
  for (int u = 0; u < PF; ++u) {
    const int kl = kbeg + u * X3K < kend ? kbeg + u * X3K : kbeg;
    x3g_load<TA, RA>(P.A, P.lda, m0, M, kl, kend, kmask, ra[u], tid, nullptr, nullptr, 0, pr0, pr1, kmap, kbeg);
    x3g_load<TB, RB>(bs0, ldb, n0, N, kl, kend, kmask, rb[u], tid, bs1, bs2, bkseg, -1, -1, TA == 1 ? kmap : nullptr, kbeg);
  }

  GEMM_STAMP(1);
  // one slab: publish slot `ra_u / rb_u` (slab k0), refill it two slabs ahead, multiply
  auto slab = [&](float (&ra_u)[RA / 8], float (&rb_u)[RB / 8], const int k0) __attribute__((always_inline)) {
    const int si = (k0 - kbeg) / X3K;
    x3g_store<TA, RA>(As, ra_u, tid, kmask, k0, kend);
    x3g_store<TB, RB>(Bs, rb_u, tid, kmask, k0, kend);
    GEMM_STAMP(2 + 4 * si);
    __syncthreads();
    GEMM_STAMP(3 + 4 * si);
    const int kp = k0 + PF * X3K < kend ? k0 + PF * X3K : kbeg;
    x3g_load<TA, RA>(P.A, P.lda, m0, M, kp, kend, kmask, ra_u, tid, nullptr, nullptr, 0, pr0, pr1, kmap, kbeg);
    x3g_load<TB, RB>(bs0, ldb, n0, N, kp, kend, kmask, rb_u, tid, bs1, bs2, bkseg, -1, -1, TA == 1 ? kmap : nullptr, kbeg);
#pragma unroll
    for (int s = 0; s < X3K / 16; ++s) {
      bf16x8 a[MT][3], b[NT][3];
      const int cl = 2 * s + h;
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
          a[mi][p] = *reinterpret_cast<const bf16x8*>(As + p * RA * X3K + x3g_off(64 * mi + 32 * wm + l31, cl));
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
          b[ni][p] = *reinterpret_cast<const bf16x8*>(Bs + p * RB * X3K + x3g_off(64 * ni + 32 * wn + l31, cl));
      }
      // small terms first; the MT x NT accumulators of one term are independent MFMAs
#define X3G_TERM(pa, pb)                                                                                          \
  _Pragma("unroll") for (int mi = 0; mi < MT; ++mi) _Pragma("unroll") for (int ni = 0; ni < NT; ++ni)              \
      acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi][pa], b[ni][pb], acc[mi][ni], 0, 0, 0);
      X3G_TERM(0, 2) X3G_TERM(2, 0) X3G_TERM(1, 1) X3G_TERM(0, 1) X3G_TERM(1, 0) X3G_TERM(0, 0)
#undef X3G_TERM
    }
    GEMM_STAMP(4 + 4 * si);
    __syncthreads();
    GEMM_STAMP(5 + 4 * si);
  };
  // slabs go in pairs with no exit between them — a `break` inside the pair joins paths with different loads in flight
  // and the compiler then waits for ALL of them (vmcnt(0)) at the next store; an odd last slab runs after the loop
  static_assert(PF == 1 || PF == 2, "one or two register slots");
  const int nsl = (kend - kbeg + X3K - 1) / X3K;
  int k0 = kbeg;
  if (PF == 1) {
    for (int it = 0; it < nsl; ++it, k0 += X3K) slab(ra[0], rb[0], k0);
  } else {
    for (int it = 0; it < (nsl >> 1); ++it) {
      slab(ra[0], rb[0], k0);
      slab(ra[PF - 1], rb[PF - 1], k0 + X3K);
      k0 += 2 * X3K;
    }
    if (nsl & 1) slab(ra[0], rb[0], k0);
  }

  GEMM_STAMP(30);
  // ------------------------------------------------------------------ epilogue, one 64x64 quadrant at a time
  if (!FULL) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
        if (m0 + 64 * mi < M && n0 + 64 * ni < N)
          epi_plain<TA, IDX>(P, acc[mi][ni], m0 + 64 * mi, n0 + 64 * ni, split, M, N, listed, wm, wn, l31, h);
    return;
  }
  float (*Ct)[64][LDT] = reinterpret_cast<float (*)[64][LDT]>(smem);       // all quadrants staged, ONE rolled body
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) epi_stage(Ct[mi * NT + ni], acc[mi][ni], wm, wn, l31, h);
  __syncthreads();
#pragma unroll 1
  for (int q = 0; q < MT * NT; ++q) {
    const int mq = m0 + 64 * (q / NT), nq = n0 + 64 * (q % NT);
    if (mq < M && nq < N) epi_full<TA, IDX>(P, Ct[q], mq, nq, MT * tm + q / NT, split, M, N, listed, tid);
  }
  GEMM_STAMP(31);
}

// ---- the plan's (ta, tb, full, idx, tile) -> instantiation
// (one 32-deep slab of operands in flight in registers: two — the PF = 2 instantiation, 36 more registers — measured the same
// in the d = 256 step, 1.41-1.43 ms either way, and 5 % slower alone: the workgroups' own count hides the latency)
template <int TA, int TB, int FULL, int IDX>
static void go_tile(const GemmPlan& pl, const GemmGroup& g, hipStream_t st) {
  if (pl.tile_n == 128) gemm_go(gemm_x3_kernel<TA, TB, FULL, 2, 2, IDX, 1>, pl, g, st);
  else if (pl.tile_m == 128) gemm_go(gemm_x3_kernel<TA, TB, FULL, 2, 1, IDX, 1>, pl, g, st);
  else gemm_go(gemm_x3_kernel<TA, TB, FULL, 1, 1, IDX, 1>, pl, g, st);
}
void launch_x3(const GemmPlan& pl, const GemmGroup& g, hipStream_t st) {
  switch (gemm_key(pl.ta, pl.tb, pl.full, pl.idx)) {
    case gemm_key(0, 0, 0, 0): return go_tile<0, 0, 0, 0>(pl, g, st);
    case gemm_key(0, 0, 1, 0): return go_tile<0, 0, 1, 0>(pl, g, st);
    case gemm_key(0, 1, 0, 0): return go_tile<0, 1, 0, 0>(pl, g, st);
    case gemm_key(0, 1, 1, 0): return go_tile<0, 1, 1, 0>(pl, g, st);
    case gemm_key(1, 1, 0, 0): return go_tile<1, 1, 0, 0>(pl, g, st);
    case gemm_key(0, 1, 1, 1): return go_tile<0, 1, 1, 1>(pl, g, st);
    case gemm_key(1, 1, 0, 1): return go_tile<1, 1, 0, 1>(pl, g, st);
    case gemm_key(0, 0, 0, 1): return go_tile<0, 0, 0, 1>(pl, g, st);
  }
}

// ====================================================================== bf16x3 product form, operands straight into LDS (round 4)
// gemm_x3_kernel above spends as long moving a slab VGPR -> split -> ds_write_b128 as multiplying it, and the two phases ADD
// (profiles/r03_gemm_notes.md: fixed 31 + products 36 + loads / split / LDS stores 41 of the FF1 product's 100 us).  This form has
// no store phase at all:
//   * the fp32 operand slabs go global -> LDS by global_load_lds_dwordx4 (LDS-DMA: no VGPR staging, no ds_write); the LDS image
//     is the DMA's lane-linear one, the bank swizzle sits on the per-lane SOURCE address (k contiguous: 128-byte rows, 16-byte
//     chunk c of row r is stored at chunk c ^ ((r >> 1) & 7), so the ds_read_b128 lane groups of a fragment read hit 16
//     different 16-byte slots; row contiguous: [k][128 rows], a fragment is eight conflict-free ds_read_b32);
//   * a wave reads the fp32 fragments of a WHOLE 32-deep slab into registers (64 VGPRs), then the workgroup's loads of the
//     next slab are issued into the other LDS stage and fly under the slab's products: one barrier per slab, and hipcc's
//     forced vmcnt(0) in front of a ds_read that follows an LDS-DMA (SIInsertWaitcnts cannot tell the stages apart) falls
//     where the loop has to wait anyway;
//   * the three-way split happens on the fragments in registers, between the MFMAs (a wave pays it for the operands of its own
//     64x64 accumulator only): tile 128x128, 4 waves, each wave the (wm, wn) 32x32 block of every 64x64 quadrant as above — so
//     the epilogues serve unchanged — = 0.5 ds_read_b128 per MFMA; 64 KB of LDS per workgroup, two workgroups per CU, the other
//     workgroup's wave on the SIMD multiplies while this one splits.
// Takes what the kernel above takes except a ragged reduction tail and K-concatenated B operands (the caller falls back).
#define X3D_STAGE (2 * X3D_T * X3D_BK * 4)          // bytes of one stage: A slab + B slab

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

// the four 16-byte pieces this thread fetches of one operand's slab (wave w issues instructions 4 w .. 4 w + 3, each 1 KB)
template <int TRANS>
__device__ __forceinline__ void x3d_issue(const float* const (&p)[4], size_t step, unsigned char* stage, int wave) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    __builtin_amdgcn_global_load_lds((glb_ptr_t)(p[j] + step), (lds_ptr_t)(stage + (4 * wave + j) * 1024), 16, 0, 0);
}

// fragment (8 reduction elements of one tile row per lane) of k-step s from a stage image, fp32
template <int TRANS>
__device__ __forceinline__ void x3d_frag(const unsigned char* img, int row, int s, int h, int swz, float (&f)[8]) {
  if (TRANS == 0) {
    const int c = 4 * s + 2 * h;
    const float4 u = *reinterpret_cast<const float4*>(img + row * 128 + ((c ^ swz) << 4));
    const float4 v = *reinterpret_cast<const float4*>(img + row * 128 + (((c + 1) ^ swz) << 4));
    f[0] = u.x; f[1] = u.y; f[2] = u.z; f[3] = u.w; f[4] = v.x; f[5] = v.y; f[6] = v.z; f[7] = v.w;
  } else {
    const float* t = reinterpret_cast<const float*>(img) + (16 * s + 8 * h) * X3D_T + row;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = t[j * X3D_T];
  }
}
// The same split for the kernels that split FRAGMENTS between their MFMAs (gemm_x3d_kernel, gemm_x3w_kernel): the residuals by two
// plain v_sub_f32 instead of one v_pk_add_f32 (inline asm: -O3 re-packs adjacent scalar subtractions) — packed fp32 VALU is the one
// vector instruction class that does not co-issue with bf16 MFMAs (MI355X_MICROARCH.md, cycle constants: +13 cycles each beside an
// MFMA).  Measured both ways in every kernel (profiles/r04_gemm_notes.md): here 2-3 % faster (4096^3 783 -> 765 us, the 21,504-row
// weight gradients 289 -> 279), in gemm_x3_kernel — whose split runs in a phase of its own, away from the MFMAs — 9 % SLOWER
// (193 -> 211 us), so that kernel keeps the packed form.  Same values bit for bit (both subtractions are exact).
__device__ __forceinline__ float x3d_sub(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ void x3d_split2(float x0, float x1, uint32_t& hi, uint32_t& mi, uint32_t& lo) {
  hi = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2{x0, x1}), bf16x2));
  float r0 = x3d_sub(x0, __uint_as_float(hi << 16)), r1 = x3d_sub(x1, __uint_as_float(hi & 0xffff0000u));
  mi = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2{r0, r1}), bf16x2));
  r0 = x3d_sub(r0, __uint_as_float(mi << 16)); r1 = x3d_sub(r1, __uint_as_float(mi & 0xffff0000u));
  lo = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2{r0, r1}), bf16x2));
}
__device__ __forceinline__ void x3d_split8(const float (&f)[8], bf16x8 (&pl)[3]) {
  uint32_t H[4], Mi[4], Lo[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) x3d_split2(f[2 * e], f[2 * e + 1], H[e], Mi[e], Lo[e]);
  pl[0] = __builtin_bit_cast(bf16x8, make_uint4(H[0], H[1], H[2], H[3]));
  pl[1] = __builtin_bit_cast(bf16x8, make_uint4(Mi[0], Mi[1], Mi[2], Mi[3]));
  pl[2] = __builtin_bit_cast(bf16x8, make_uint4(Lo[0], Lo[1], Lo[2], Lo[3]));
}

// DIAG (diagnostic build only, PS_X3D_DIAG; WRONG results): 1 no split (raw bits as planes), 2 no MFMAs, 3 no slab loads in the loop
template <int TA, int TB, int FULL, int IDX, int DIAG = 0>
__global__ __launch_bounds__(256, 2) void gemm_x3d_kernel(const GemmGroup g) {
  fork_signal(g.sig, g.sigval);
  constexpr int MT = 2, NT = 2;
  constexpr int MAIN_BYTES = 2 * X3D_STAGE;
  constexpr int EPI_BYTES = FULL ? MT * NT * 64 * LDT * 4 : 16;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[MAIN_BYTES > EPI_BYTES ? MAIN_BYTES : EPI_BYTES];
  __shared__ int kidx[IDX && TA == 1 ? KIDX_MAX : 1];

  int prob, split, ftile = 0;
  if (g.flat) {
    const int L = blockIdx.x;
    prob = L >= g.flat0[3] ? 3 : (L >= g.flat0[2] ? 2 : (L >= g.flat0[1] ? 1 : 0));
    const int t = L - g.flat0[prob];
    if ((g.flat_xcd >> prob) & 1) {
      const int s8 = t >> 3, grp = s8 / g.flat_tiles[prob];
      split = (t & 7) + 8 * grp;
      ftile = s8 - grp * g.flat_tiles[prob];
    } else {
      split = t / g.flat_tiles[prob];
      ftile = t - split * g.flat_tiles[prob];
    }
  } else if (g.split_xcd) {       // 3-D grid of a split reduction: all tiles of a split on one XCD, as GemmGroup::flat_xcd does it
    const int T = gridDim.x * gridDim.y, ks = g.p[0].ksplit;
    const int Lz = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;       // dispatch order
    prob = Lz / (T * ks);
    const int t = Lz - prob * T * ks, s8 = t >> 3, grp = s8 / T;
    split = (t & 7) + 8 * grp;
    ftile = s8 - grp * T;
  } else {
    prob = blockIdx.z / g.p[0].ksplit;
    split = blockIdx.z - prob * g.p[0].ksplit;
  }
  const GemmProblem& P = g.p[prob];
  const bool listed = IDX && P.ridx != nullptr;                 // block-uniform
  const int nlist = listed ? *P.rcount : 0;
  const int M = (listed && TA == 0) ? nlist : P.M, N = P.N, K = (listed && TA == 1) ? nlist : P.K;
  int tm, tn;                                                    // XCD-aware tile mapping as in gemm_f32_kernel
  if (g.flat) {
    tm = ftile % g.flat_tm[prob];
    tn = ftile / g.flat_tm[prob];
  } else if (g.split_xcd) {
    tm = ftile % (int)gridDim.y;
    tn = ftile / (int)gridDim.y;
  } else {
    const int nx = gridDim.x, ny = gridDim.y;
    const int L = blockIdx.y * nx + blockIdx.x;
    const int grp = L / (8 * nx), r = L - grp * 8 * nx;
    const int rows_here = min(8, ny - grp * 8);
    tm = grp * 8 + r % rows_here;
    tn = r / rows_here;
  }
  const int m0 = tm * X3D_T, n0 = tn * X3D_T;
  const int nslab = (K + X3D_BK - 1) / X3D_BK;
  const int per = (nslab + P.ksplit - 1) / P.ksplit;
  const int kbeg = split * per * X3D_BK;
  const int kend = min(K, kbeg + per * X3D_BK);
  if (m0 >= M || n0 >= N || kbeg >= kend) return;   // block-uniform
  const int nsl = (kend - kbeg + X3D_BK - 1) / X3D_BK;      // listed weight gradients: a ragged last slab repeats the list's last row ...
  const int ktail = kend - kbeg - (nsl - 1) * X3D_BK;       // ... and the fragments of the repeated rows are zeroed (below)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, h = lane >> 5;

  // ---- per-thread sources of the slab loads
  const float* pa[4];
  const float* pb[4];
  size_t stepa, stepb;                                           // floats per slab
  if (listed && TA == 1) {                                       // physical reduction rows of this split -> LDS (padded by the last one)
    for (int i = tid; i < nsl * X3D_BK; i += 256) kidx[i] = P.ridx[min(kbeg + i, kend - 1)];
    __syncthreads();
  }
  if (TA == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 32 * wave + 8 * j + (lane >> 3);
      int row = min(m0 + r, M - 1);
      if (listed) row = P.ridx[row];
      pa[j] = P.A + (size_t)row * P.lda + kbeg + 4 * ((lane & 7) ^ ((r >> 1) & 7));
    }
    stepa = X3D_BK;
  } else {
    const int col = min(m0 + 4 * (lane & 31), M - 4);          // M % 4 == 0 (validated)
#pragma unroll
    for (int j = 0; j < 4; ++j) pa[j] = P.A + (size_t)(listed ? 0 : kbeg + 8 * wave + 2 * j + (lane >> 5)) * P.lda + col;
    stepa = (size_t)X3D_BK * P.lda;
  }
  if (TB == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = 32 * wave + 8 * j + (lane >> 3);
      pb[j] = P.Bseg[0] + (size_t)min(n0 + r, N - 1) * P.ldb + kbeg + 4 * ((lane & 7) ^ ((r >> 1) & 7));
    }
    stepb = X3D_BK;
  } else {
    const int col = min(n0 + 4 * (lane & 31), N - 4);          // N % 4 == 0 (validated)
#pragma unroll
    for (int j = 0; j < 4; ++j) pb[j] = P.Bseg[0] + (size_t)((listed && TA == 1) ? 0 : kbeg + 8 * wave + 2 * j + (lane >> 5)) * P.ldb + col;
    stepb = (size_t)X3D_BK * P.ldb;
  }
  auto issue = [&](int it) __attribute__((always_inline)) {
    unsigned char* const stage = smem + (it & 1) * X3D_STAGE;
    if (listed && TA == 1) {                                     // reduction rows through the list
      const float* qa[4];
      const float* qb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const size_t kr = (size_t)kidx[it * X3D_BK + 8 * wave + 2 * j + (lane >> 5)];
        qa[j] = pa[j] + kr * P.lda;
        qb[j] = pb[j] + kr * P.ldb;
      }
      x3d_issue<TA>(qa, 0, stage, wave);
      x3d_issue<TB>(qb, 0, stage + X3D_STAGE / 2, wave);
    } else {
      x3d_issue<TA>(pa, it * stepa, stage, wave);
      x3d_issue<TB>(pb, it * stepb, stage + X3D_STAGE / 2, wave);
    }
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int swz = (l31 >> 1) & 7;
  issue(0);
  for (int it = 0; it < nsl; ++it) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this thread's pieces of slab `it` have landed
    __syncthreads();                                             // everybody's; and everybody is done with the other stage
    const unsigned char* const sa = smem + (it & 1) * X3D_STAGE;
    const unsigned char* const sb = sa + X3D_STAGE / 2;
    float fa[2][MT][8], fb[2][NT][8];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) x3d_frag<TA>(sa, 64 * mi + 32 * wm + l31, s, h, swz, fa[s][mi]);
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) x3d_frag<TB>(sb, 64 * ni + 32 * wn + l31, s, h, swz, fb[s][ni]);
    }
    if (it + 1 < nsl && DIAG != 3) issue(it + 1);                // block-uniform; flies under the products below
    if (IDX && TA == 1 && it == nsl - 1 && ktail < X3D_BK) {     // ragged tail of a listed reduction: zero A's repeated rows
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (16 * s + 8 * h + j >= ktail) fa[s][mi][j] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 a[MT][3], b[NT][3];
      if (DIAG == 1) {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
          a[mi][0] = a[mi][2] = __builtin_bit_cast(bf16x8, make_float4(fa[s][mi][0], fa[s][mi][1], fa[s][mi][2], fa[s][mi][3]));
          a[mi][1] = __builtin_bit_cast(bf16x8, make_float4(fa[s][mi][4], fa[s][mi][5], fa[s][mi][6], fa[s][mi][7]));
        }
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
          b[ni][0] = b[ni][2] = __builtin_bit_cast(bf16x8, make_float4(fb[s][ni][0], fb[s][ni][1], fb[s][ni][2], fb[s][ni][3]));
          b[ni][1] = __builtin_bit_cast(bf16x8, make_float4(fb[s][ni][4], fb[s][ni][5], fb[s][ni][6], fb[s][ni][7]));
        }
      } else {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) x3d_split8(fa[s][mi], a[mi]);
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) x3d_split8(fb[s][ni], b[ni]);
      }
      if (DIAG == 2) {
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int p = 0; p < 3; ++p) { asm volatile("" ::"v"(a[mi][p])); asm volatile("" ::"v"(b[mi][p])); }
        continue;
      }
#define X3D_TERM(pa_, pb_)                                                                                        \
  _Pragma("unroll") for (int mi = 0; mi < MT; ++mi) _Pragma("unroll") for (int ni = 0; ni < NT; ++ni)              \
      acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi][pa_], b[ni][pb_], acc[mi][ni], 0, 0, 0);
      X3D_TERM(0, 2) X3D_TERM(2, 0) X3D_TERM(1, 1) X3D_TERM(0, 1) X3D_TERM(1, 0) X3D_TERM(0, 0)
#undef X3D_TERM
    }
  }

  // ------------------------------------------------------------------ epilogue, one 64x64 quadrant at a time (as gemm_x3_kernel)
  if (!FULL) {
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int ni = 0; ni < NT; ++ni)
        if (m0 + 64 * mi < M && n0 + 64 * ni < N)
          epi_plain<TA, IDX>(P, acc[mi][ni], m0 + 64 * mi, n0 + 64 * ni, split, M, N, listed, wm, wn, l31, h);
    return;
  }
  __syncthreads();                                               // the last slab's fragments have left LDS in every wave
  float (*Ct)[64][LDT] = reinterpret_cast<float (*)[64][LDT]>(smem);
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NT; ++ni) epi_stage(Ct[mi * NT + ni], acc[mi][ni], wm, wn, l31, h);
  __syncthreads();
#pragma unroll 1
  for (int q = 0; q < MT * NT; ++q) {
    const int mq = m0 + 64 * (q / NT), nq = n0 + 64 * (q % NT);
    if (mq < M && nq < N) epi_full<TA, IDX>(P, Ct[q], mq, nq, MT * tm + q / NT, split, M, N, listed, tid);
  }
}

// ---- the plan's (ta, tb, full, idx) -> instantiation (the set gemm_x3_kernel has)
void launch_x3d(const GemmPlan& pl, const GemmGroup& g, hipStream_t st) {
#if PS_DIAG_ON
  if (pl.diag == 1) return gemm_go(gemm_x3d_kernel<0, 0, 0, 0, 1>, pl, g, st);
  if (pl.diag == 2) return gemm_go(gemm_x3d_kernel<0, 0, 0, 0, 2>, pl, g, st);
  if (pl.diag == 3) return gemm_go(gemm_x3d_kernel<0, 0, 0, 0, 3>, pl, g, st);
#endif
  switch (gemm_key(pl.ta, pl.tb, pl.full, pl.idx)) {
    case gemm_key(0, 0, 0, 0): return gemm_go(gemm_x3d_kernel<0, 0, 0, 0>, pl, g, st);
    case gemm_key(0, 0, 1, 0): return gemm_go(gemm_x3d_kernel<0, 0, 1, 0>, pl, g, st);
    case gemm_key(0, 1, 0, 0): return gemm_go(gemm_x3d_kernel<0, 1, 0, 0>, pl, g, st);
    case gemm_key(0, 1, 1, 0): return gemm_go(gemm_x3d_kernel<0, 1, 1, 0>, pl, g, st);
    case gemm_key(1, 1, 0, 0): return gemm_go(gemm_x3d_kernel<1, 1, 0, 0>, pl, g, st);
    case gemm_key(0, 1, 1, 1): return gemm_go(gemm_x3d_kernel<0, 1, 1, 1>, pl, g, st);
    case gemm_key(1, 1, 0, 1): return gemm_go(gemm_x3d_kernel<1, 1, 0, 1>, pl, g, st);
    case gemm_key(0, 0, 0, 1): return gemm_go(gemm_x3d_kernel<0, 0, 0, 1>, pl, g, st);
  }
}

// ====================================================================== bf16x3 products against PRE-SPLIT weights (round 4)
// In the products of a layer's forward and input gradients the B operand is a WEIGHT: a few hundred KB that every one of the
// launch's hundreds of workgroups used to split again, slab by slab (and, for the dX products, fetch through the row-contiguous
// loader with its strided 4 / 8-byte accesses).  WPlaneScope splits each weight once per entry-point call into bf16 plane
// matrices [3][N][K] in BOTH orientations; this kernel then
//   * brings B's planes global -> LDS by global_load_lds_dwordx4 ([row][32 k] bf16 images, 16-byte chunks XOR-swizzled by
//     (row >> 2) & 3 on the source address: the read pattern of gemm_x3_kernel, SQ_LDS_BANK_CONFLICT 0) and feeds them to the
//     MFMAs as they are: no VALU, no LDS store;
//   * brings A (the activation, fp32) in as gemm_x3d_kernel does and splits its fragments in registers — but the four waves
//     are stacked 4 x 1 over the 128-row tile (wave tile 32 x 128), so every A fragment is split by exactly ONE wave: a quarter
//     of gemm_x3d_kernel's split work per MFMA, an eighth of gemm_x3_kernel's per element (which re-split A for every 64-wide
//     column tile);
//   * tile 128 x 128, 32-deep slabs, two LDS stages of 16 KB (A) + 24 KB (B planes), one barrier per slab, two workgroups per CU.
// K-concatenated B operands (the K/V dX product: [dK | dV] against [Wk ; Wv]) pick the segment per slab (kseg % 32 == 0).
#define X3W_STAGE (X3D_T * X3D_BK * 4 + 3 * X3D_T * X3D_BK * 2)      // 16 KB + 24 KB

template <int FULL, int IDX>
__global__ __launch_bounds__(256, 2) void gemm_x3w_kernel(const GemmGroup g) {
  fork_signal(g.sig, g.sigval);
  constexpr int MAIN_BYTES = 2 * X3W_STAGE;
  constexpr int EPI_BYTES = FULL ? 4 * 64 * LDT * 4 : 16;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[MAIN_BYTES > EPI_BYTES ? MAIN_BYTES : EPI_BYTES];

  const int prob = blockIdx.z;
  const GemmProblem& P = g.p[prob];
  const bool listed = IDX && P.ridx != nullptr;                 // block-uniform
  const int nlist = listed ? *P.rcount : 0;
  const int M = listed ? nlist : P.M, N = P.N, K = P.K;
  int tm, tn;                                                    // XCD-aware tile mapping as in gemm_f32_kernel
  {
    const int nx = gridDim.x, ny = gridDim.y;
    const int L = blockIdx.y * nx + blockIdx.x;
    const int grp = L / (8 * nx), r = L - grp * 8 * nx;
    const int rows_here = min(8, ny - grp * 8);
    tm = grp * 8 + r % rows_here;
    tn = r / rows_here;
  }
  const int m0 = tm * X3D_T, n0 = tn * X3D_T;
  if (m0 >= M || n0 >= N) return;                               // block-uniform
  const int nsl = K / X3D_BK;                                    // (K % 32 == 0: the launcher checked)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;

  // ---- per-thread sources of the slab loads.  A: 16 instructions of 8 rows x 128 B, wave w issues 4 w .. 4 w + 3.
  const float* pa[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = 32 * wave + 8 * j + (lane >> 3);
    int row = min(m0 + r, M - 1);
    if (listed) row = P.ridx[row];
    pa[j] = P.A + (size_t)row * P.lda + 4 * ((lane & 7) ^ ((r >> 1) & 7));
  }
  // B planes: 24 instructions of 16 rows x 64 B (3 planes x 8 row blocks), wave w issues 6 w .. 6 w + 5
  const int kseg = P.kseg;
  size_t pboff[6];                                               // element offset inside a segment's plane set, slab 0
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int q = 6 * wave + j, pl = q >> 3, rb = q & 7;
    const int r = 16 * rb + (lane >> 2);
    const int row = min(n0 + r, N - 1);
    pboff[j] = ((size_t)pl * N + row) * kseg + 8 * ((lane & 3) ^ ((r >> 2) & 3));
  }
  auto issue = [&](int it) __attribute__((always_inline)) {
    unsigned char* const stage = smem + (it & 1) * X3W_STAGE;
    const int k0 = it * X3D_BK;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(pa[j] + k0), (lds_ptr_t)(stage + (4 * wave + j) * 1024), 16, 0, 0);
    const int sg = k0 >= kseg ? (k0 >= 2 * kseg ? 2 : 1) : 0;   // block-uniform
    const uint16_t* const bp = (sg == 0 ? P.bpl[0] : (sg == 1 ? P.bpl[1] : P.bpl[2])) + (k0 - sg * kseg);
#pragma unroll
    for (int j = 0; j < 6; ++j)
      __builtin_amdgcn_global_load_lds((glb_ptr_t)(bp + pboff[j]), (lds_ptr_t)(stage + X3D_T * X3D_BK * 4 + (6 * wave + j) * 1024), 16, 0, 0);
  };

  f32x16 acc[4];                                                 // column block j = 2 ni + wn of the tile, rows 32 wave ..
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int swz = (l31 >> 1) & 7, bsw = (l31 >> 2) & 3;
  issue(0);
  for (int it = 0; it < nsl; ++it) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned char* const sa = smem + (it & 1) * X3W_STAGE;
    const unsigned char* const sb = sa + X3D_T * X3D_BK * 4;
    float fa[2][8];
    bf16x8 b[2][4][3];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      x3d_frag<0>(sa, 32 * wave + l31, s, h, swz, fa[s]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int p = 0; p < 3; ++p)
          b[s][j][p] = *reinterpret_cast<const bf16x8*>(sb + p * (X3D_T * 64) + (32 * j + l31) * 64 + (((2 * s + h) ^ bsw) << 4));
    }
    if (it + 1 < nsl) issue(it + 1);                             // block-uniform; flies under the products below
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 a[3];
      x3d_split8(fa[s], a);
#define X3W_TERM(pa_, pb_)                                                                                        \
  _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                    \
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa_], b[s][j][pb_], acc[j], 0, 0, 0);
      X3W_TERM(0, 2) X3W_TERM(2, 0) X3W_TERM(1, 1) X3W_TERM(0, 1) X3W_TERM(1, 0) X3W_TERM(0, 0)
#undef X3W_TERM
    }
  }

  // ------------------------------------------------------------------ epilogue: this wave holds block (wm, wn) = (wave & 1, j & 1) of
  // the 64x64 quadrants (mi, ni) = (wave >> 1, j >> 1) — the layout the shared epilogues expect
  const int mi = wave >> 1, wm = wave & 1;
  if (!FULL) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (m0 + 64 * mi < M && n0 + 64 * (j >> 1) < N)
        epi_plain<0, IDX>(P, acc[j], m0 + 64 * mi, n0 + 64 * (j >> 1), 0, M, N, listed, wm, j & 1, l31, h);
    return;
  }
  __syncthreads();                                               // the last slab's fragments have left LDS in every wave
  float (*Ct)[64][LDT] = reinterpret_cast<float (*)[64][LDT]>(smem);
#pragma unroll
  for (int j = 0; j < 4; ++j) epi_stage(Ct[mi * 2 + (j >> 1)], acc[j], wm, j & 1, l31, h);
  __syncthreads();
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    const int mq = m0 + 64 * (q >> 1), nq = n0 + 64 * (q & 1);
    if (mq < M && nq < N) epi_full<0, IDX>(P, Ct[q], mq, nq, 2 * tm + (q >> 1), 0, M, N, listed, tid);
  }
}

// ---- the weight planes
struct WPlaneJob { const float* w; int rows, cols; uint16_t* nrm; uint16_t* trn; int first_block; };
struct WPlaneJobs { WPlaneJob j[PS_WPLANES_MAX]; int n; };
// one thread per 8-element chunk of an output plane row: first the rows x cols / 8 chunks of the normal orientation, then the
// cols x rows / 8 chunks of the transposed one (strided reads of a matrix that lives in L2)
__global__ __launch_bounds__(256) void wplanes_kernel(const WPlaneJobs J) {
  int ji = 0;
#pragma unroll
  for (int i = 1; i < PS_WPLANES_MAX; ++i)
    if (i < J.n && (int)blockIdx.x >= J.j[i].first_block) ji = i;
  const WPlaneJob& jb = J.j[ji];
  const int rows = jb.rows, cols = jb.cols;
  const int64_t c = (int64_t)(blockIdx.x - jb.first_block) * 256 + threadIdx.x;
  const int64_t n_nrm = (int64_t)rows * (cols >> 3), n_trn = (int64_t)cols * (rows >> 3);
  if (c >= n_nrm + n_trn) return;
  float v[8];
  uint16_t* dst;
  size_t pstride = (size_t)rows * cols;
  if (c < n_nrm) {
    const int r = (int)(c / (cols >> 3)), kc = (int)(c - (int64_t)r * (cols >> 3));
    const float4 v0 = *reinterpret_cast<const float4*>(jb.w + (size_t)r * cols + 8 * kc);
    const float4 v1 = *reinterpret_cast<const float4*>(jb.w + (size_t)r * cols + 8 * kc + 4);
    v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
    dst = jb.nrm + (size_t)r * cols + 8 * kc;
  } else {
    const int64_t t = c - n_nrm;
    const int cc = (int)(t / (rows >> 3)), rc = (int)(t - (int64_t)cc * (rows >> 3));
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = jb.w[(size_t)(8 * rc + j) * cols + cc];
    dst = jb.trn + (size_t)cc * rows + 8 * rc;
  }
  bf16x8 pl[3];
  x3d_split8(v, pl);
#pragma unroll
  for (int p = 0; p < 3; ++p) *reinterpret_cast<bf16x8*>(dst + p * pstride) = pl[p];
}

struct WPlaneEntry { const float* w; int rows, cols; const uint16_t* nrm; const uint16_t* trn; };
static thread_local WPlaneEntry g_wplanes[PS_WPLANES_MAX];
static thread_local int g_wplanes_n = 0;

WPlaneScope::WPlaneScope(hipStream_t st, const float* const* w, const int* rows, const int* cols, int n) : on(false) {
  g_wplanes_n = 0;
  if (!gemm_x3w_on() || n <= 0) return;
  WPlaneJobs J;
  memset(&J, 0, sizeof(J));
  size_t elems = 0;
  int blocks = 0, k = 0;
  for (int i = 0; i < n && k < PS_WPLANES_MAX; ++i) {
    if (!w[i] || rows[i] % 32 || cols[i] % 32 || ((uintptr_t)w[i] & 15)) continue;
    bool dup = false;
    for (int q = 0; q < k; ++q) dup = dup || J.j[q].w == w[i];
    if (dup) continue;
    J.j[k].w = w[i]; J.j[k].rows = rows[i]; J.j[k].cols = cols[i]; J.j[k].first_block = blocks;
    blocks += ps_cdiv((int64_t)2 * rows[i] * (cols[i] >> 3), 256);
    elems += (size_t)rows[i] * cols[i];
    ++k;
  }
  if (!k) return;
  uint16_t* base = reinterpret_cast<uint16_t*>(ps_det_scratch(2, (elems * 2 * 3 * 2 + 3) / 4 + 64, st));
  if (!base) return;                                             // stream capture or out of memory: the products split B themselves
  size_t off = 0;
  for (int i = 0; i < k; ++i) {
    const size_t e = (size_t)J.j[i].rows * J.j[i].cols;
    J.j[i].nrm = base + off; off += 3 * e;
    J.j[i].trn = base + off; off += 3 * e;
    g_wplanes[i] = WPlaneEntry{J.j[i].w, J.j[i].rows, J.j[i].cols, J.j[i].nrm, J.j[i].trn};
  }
  J.n = k;
  hipLaunchKernelGGL(wplanes_kernel, dim3(blocks), dim3(256), 0, st, J);
  if (hipGetLastError() != hipSuccess) return;
  g_wplanes_n = k;
  on = true;
}
WPlaneScope::~WPlaneScope() { g_wplanes_n = 0; }

// B segments of `p` as plane matrices [3][N][kseg]; false: not (all) registered (which shapes the kernel takes: gemm.hip, x3w_takes)
bool wplanes_find(const GemmProblem& p, const uint16_t* (&bpl)[3]) {
  if (g_wplanes_n == 0) return false;
  const int nseg = ps_cdiv(p.K, p.kseg), ks = nseg > 1 ? p.kseg : p.K;
  for (int sg = 0; sg < nseg; ++sg) {
    const uint16_t* found = nullptr;
    for (int i = 0; i < g_wplanes_n; ++i) {
      const WPlaneEntry& e = g_wplanes[i];
      if (e.w != p.Bseg[sg]) continue;
      if (!p.tb && e.rows == p.N && e.cols == ks && p.ldb == e.cols) found = e.nrm;       // B[n][k] = W[n][k]
      if (p.tb && e.cols == p.N && e.rows == ks && p.ldb == e.cols) found = e.trn;        // B[k][n] = W[k][n]: planes of W^T
    }
    if (!found) return false;
    bpl[sg] = found;
  }
  return true;
}

// ---- the plan's (full, idx) -> instantiation
void launch_x3w(const GemmPlan& pl, const GemmGroup& g, hipStream_t st) {
  if (pl.full && pl.idx) gemm_go(gemm_x3w_kernel<1, 1>, pl, g, st);
  else if (pl.full) gemm_go(gemm_x3w_kernel<1, 0>, pl, g, st);
  else if (pl.idx) gemm_go(gemm_x3w_kernel<0, 1>, pl, g, st);
  else gemm_go(gemm_x3w_kernel<0, 0>, pl, g, st);
}
