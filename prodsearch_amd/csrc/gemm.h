// gemm.h — what the GEMM kernel families (gemm_kernels.hip: the fp32 MFMA and the three bf16x3 forms) and their dispatcher
// (gemm.hip) share: the launch plan, and what the kernels share among themselves: the two epilogues and the tile constants.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------- the launch plan (host only; not a kernel argument)
// gemm.hip's gemm_plan decides one launch completely; gemm_launch applies it to the group and hands both to the family's
// launch_<family>, which is nothing but the switch from the plan's (ta, tb, full, idx) to the template instantiation.
enum GemmFamily { GEMM_F32 = 0, GEMM_X3 = 1, GEMM_X3D = 2, GEMM_X3W = 3 };
struct GemmPlan {
  int family;                         // GemmFamily
  int ta, tb, full, idx;              // the instantiation: layouts, FULL epilogue, row-list (IDX) form
  int bk, pf;                         // fp32: slab depth (32 / 128) and slabs in flight; the bf16x3 forms: 32, 1
  int tile_m, tile_n;                 // output tile of one workgroup (64 / 128)
  int diag;                           // x3d, diagnostic build only (PS_X3D_DIAG): the timing-only variant
  int flat, redirected;               // 1-D grid over the flat tables; the caller asked for the 3-D grid and was sent to the flat one
  dim3 grid;
  int lds_bytes;                      // dynamic LDS (0 but for PS_X3D_LDSPAD)
  int flat0[5], flat_tm[4], flat_tiles[4], flat_xcd;      // flat launches: GemmGroup's tables
  int split_xcd;                      // GemmGroup::split_xcd
  int timed;                          // a PS_KLAUNCH site (the kernel timer can attach to it)
  int repeat;                         // PS_DEBUG_REPEAT (plain fp32 launches, timing experiments)
  const uint16_t* bpl[4][3];          // x3w: the members' weight planes ...
  int kseg[4];                        // ... and their kseg (a single segment's planes are [3][N][K])
};
// the instantiation key of the families' switches
constexpr int gemm_key(int ta, int tb, int full, int idx) { return ta << 3 | tb << 2 | full << 1 | idx; }
template <typename Kern>
static inline void gemm_go(Kern kernel, const GemmPlan& pl, const GemmGroup& g, hipStream_t st) {
  if (pl.timed) PS_KLAUNCH(kernel, pl.grid, dim3(256), pl.lds_bytes, st, g);
  else hipLaunchKernelGGL(kernel, pl.grid, dim3(256), pl.lds_bytes, st, g);
}
// one per family, beside its kernel; every combination the plan can hold has its instantiation there (gemm_plan refuses the others)
void launch_f32(const GemmPlan& pl, const GemmGroup& g, hipStream_t st);
void launch_x3(const GemmPlan& pl, const GemmGroup& g, hipStream_t st);
void launch_x3d(const GemmPlan& pl, const GemmGroup& g, hipStream_t st);
void launch_x3w(const GemmPlan& pl, const GemmGroup& g, hipStream_t st);
// gemm_kernels.hip's registry of weight planes (WPlaneScope): the B segments of `p` as registered plane matrices; false: not (all) registered
bool wplanes_find(const GemmProblem& p, const uint16_t* (&bpl)[3]);

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define BM 64
#define BN 64
#define LDT (BM + 1)

// ---------------------------------------------------------------------- epilogues (shared by both product forms)
// One 64x64 tile whose four 32x32 accumulators sit in the workgroup's four waves (wave (wm, wn), MFMA 32x32 C layout).
template <int TA, int IDX>
__device__ __forceinline__ void epi_plain(const GemmProblem& P, const f32x16& acc, int m0, int n0, int split, int M, int N,
                                          bool listed, int wm, int wn, int l31, int h, const int* rows_s = nullptr) {
  const int col = n0 + wn * 32 + l31;
  const bool col_ok = col < N;
  const float bias = (P.bias && col_ok && split == 0) ? P.bias[col] : 0.f;
  const float alpha = P.alpha;
  float* const C = P.C + (size_t)split * P.split_stride;
  const int ldc = P.ldc, accumulate = P.accumulate;
  if (accumulate == 2) {
    // split reduction (kernel-uniform): sixteen atomics in a straight line.  In the general loop below every row sits under its own
    // test beside the load + store of `accumulate == 1`, and the compiler opened each row's block with s_waitcnt vmcnt(0): a wave
    // waited for the previous row's atomic to be ACKNOWLEDGED before it issued the next — sixteen dependent round trips, 15,000 of
    // the 42,000 cycles a K / V weight-gradient workgroup lived at C2 (profiles/kvq_wgrad_notes.md).  No test here:
    // a row or column past the edge adds 0.f to the last real one.
    const int ccol = min(col, N - 1);
    size_t off[16];
    float v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, rr = min(row, M - 1);
      off[r] = (size_t)((listed && TA == 0) ? (rows_s ? rows_s[rr - m0] : P.ridx[rr]) : rr) * ldc + ccol;
      v[r] = (col_ok && row < M) ? (acc[r] + bias) * alpha : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) atomicAdd(&C[off[r]], v[r]);
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (col_ok && row < M) {
      const float v = (acc[r] + bias) * alpha;
      const size_t off = (size_t)((listed && TA == 0) ? (rows_s ? rows_s[row - m0] : P.ridx[row]) : row) * ldc + col;
      if (accumulate == 0) C[off] = v;
      else if (accumulate == 1) C[off] += v;
      else atomicAdd(&C[off], v);
    }
  }
}

__device__ __forceinline__ void epi_stage(float (*Ct)[LDT], const f32x16& acc, int wm, int wn, int l31, int h) {
#pragma unroll
  for (int r = 0; r < 16; ++r) Ct[wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h][wn * 32 + l31] = acc[r];
}

template <int TA, int IDX>
__device__ __forceinline__ void epi_full(const GemmProblem& P, const float (*Ct)[LDT], int m0, int n0, int tm, int split,
                                         int M, int N, bool listed, int tid, const int* rows_s = nullptr) {
  float* const C = P.C + (size_t)split * P.split_stride;
  const float alpha = P.alpha;
  const int ldc = P.ldc, accumulate = P.accumulate;
  const int ccol = tid & 63, gcol = n0 + ccol;
  if (gcol >= N) return;
  const float cbias = (P.bias && split == 0) ? P.bias[gcol] : 0.f;
  const int act = P.act;
  const DropSpec drop = P.drop;
  const bool dropping = drop.thr != 0u, has_res = P.res.mode != RES_NONE;
  const float add2 = (P.out2 && P.add2) ? P.add2[gcol] : 0.f;
  float csum = 0.f;
  // global operands of the epilogue (activation aux, residual) of ALL 16 rows of this thread, fetched up front by loads that
  // are unconditional inside their (kernel-uniform) switch: a load under a per-row condition makes the compiler wait for
  // everything in flight at the join, and the rolled loop this used to be — one row group fetched ahead under `ok ? load : 0`
  // selects — was sixteen dependent round trips (11 us of the 24 us dX product over the step's row list,
  // tools/gemm_f32_stamps.py).  Rows past M repeat row M - 1, so every address is a real one; their values are never used.
  const bool need_aux = act == ACT_GELU_BWD || act == ACT_TANH_BWD;
  float paux[4][4], pres[4][4];
  int prow[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int lrow = min(m0 + 4 * ((tid >> 6) + 4 * i) + q, M - 1);
      // physical row of the operands (rows_s: the tile's 64 list entries, put in LDS by the prologue)
      prow[i][q] = (listed && TA == 0) ? (rows_s ? rows_s[lrow - m0] : P.ridx[lrow]) : lrow;
      paux[i][q] = 0.f; pres[i][q] = 0.f;
    }
  if (need_aux) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) paux[i][q] = P.act_aux[(size_t)prow[i][q] * ldc + gcol];
  }
  if (has_res) {
    const ResMap& R = P.res;
    if (R.mode == RES_DIRECT) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) pres[i][q] = R.ptr[(size_t)prow[i][q] * R.ld + gcol];
    } else if (R.mode == RES_FANIN && !R.ptr && R.extra) {   // the fan-in sums already sit in extra (+ extra2): one row per sequence
      const float* const e2 = R.extra2 ? R.extra2 : R.extra;
      const float w2 = R.extra2 ? 1.f : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int nin = fdiv(prow[i][q], R.dS), pos = prow[i][q] - nin * R.S;
          const float v1 = R.extra[(size_t)nin * R.extra_ld + gcol], v2 = e2[(size_t)nin * R.extra_ld + gcol];
          pres[i][q] = (R.Sq == R.S || pos == R.qpos) ? v1 + w2 * v2 : 0.f;
        }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) pres[i][q] = res_value(R, prow[i][q], gcol);
    }
  }
  // lean form (bias / scale / residual only — the step's dX products): straight-line, nothing re-read from the argument
  // segment per row (the general body below is so large that the compiler keeps none of P's fields in scalar registers: it
  // fetched three of them again for EVERY row, each a scalar-cache round trip in front of the row's store)
  if (!dropping && act == ACT_NONE && !P.aux_out && !P.out2 && !P.colsum && !P.colsum_part && accumulate == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // (no branch per row: a row past M repeats row M - 1 — same address, same value — because a store under a per-row
        // condition made the compiler wait for the previous row's store to be acknowledged before the next LDS read)
        const int lrow = min(4 * ((tid >> 6) + 4 * i) + q, M - 1 - m0);
        C[(size_t)((IDX && TA == 0) ? prow[i][q] : m0 + lrow) * ldc + gcol] = (Ct[lrow][ccol] + cbias) * alpha + pres[i][q];
      }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lrow = 4 * ((tid >> 6) + 4 * i);
    const int rbase = m0 + lrow;
    if (rbase >= M) break;
    Philox4 rnd = {0u, 0u, 0u, 0u};
    float hm[4] = {1.f, 1.f, 1.f, 1.f};
    if (dropping && drop.half) {
      // half form (common.h): the 8 lanes that hold columns 8g .. 8g+7 share ONE call per row; lane j of the group draws
      // the call of row rbase + (j & 3) and the group exchanges the words (tiles start at multiples of 64 columns, a lane's
      // column is n0 + (tid & 63): groups are aligned)
      const int j = tid & 7, e = gcol & 7, base = (tid & 63) & ~7;
      if ((N & 7) == 0) {                                  // whole groups are active (lanes past N have left)
        const Philox4 mine = drop_call16(drop, (uint32_t)(rbase + (j & 3)), (uint32_t)gcol >> 3, drop_step(drop));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          Philox4 rq;
          rq.x = __shfl(mine.x, base + q, 64); rq.y = __shfl(mine.y, base + q, 64);
          rq.z = __shfl(mine.z, base + q, 64); rq.w = __shfl(mine.w, base + q, 64);
          hm[q] = drop_half(drop, rq, e);
        }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) hm[q] = drop_half(drop, drop_call16(drop, (uint32_t)(rbase + q), (uint32_t)gcol >> 3, drop_step(drop)), e);
      }
    } else if (dropping) rnd = philox4x32_10((uint32_t)gcol, (uint32_t)rbase >> 2, drop.site, drop_step(drop), drop.k0, drop.k1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = rbase + q;
      if (row >= M) break;
      float v = (Ct[lrow + q][ccol] + cbias) * alpha;
      const size_t off = (size_t)((IDX && TA == 0) ? prow[i][q] : row) * ldc + gcol;
      if (P.aux_out) P.aux_out[off] = v;
      if (act == ACT_GELU) v = gelu_tanh_f(v);
      else if (act == ACT_TANH) v = tanh_fast(v);
      else if (act == ACT_GELU_BWD) v *= gelu_tanh_grad(paux[i][q]);
      else if (act == ACT_TANH_BWD) v *= (1.f - paux[i][q] * paux[i][q]);
      if (dropping) {
        const uint32_t wv = q == 0 ? rnd.x : (q == 1 ? rnd.y : (q == 2 ? rnd.z : rnd.w));
        v *= drop.half ? hm[q] : drop_word(drop, wv);
      }
      v += pres[i][q];
      csum += v;
      if (P.out2) P.out2[(size_t)((IDX && TA == 0) ? prow[i][q] : row) * P.ld2 + gcol] = v + add2;
      if (accumulate == 0) C[off] = v;
      else if (accumulate == 1) C[off] += v;
      else atomicAdd(&C[off], v);
    }
  }
  if (P.colsum_part) P.colsum_part[((size_t)(4 * tm + (tid >> 6)) * 3) * N + gcol] = csum;   // one parked row per (tile, row group)
  else if (P.colsum) atomicAdd(&P.colsum[gcol], csum);
}

#define KIDX_MAX PS_GEMM_KIDX_MAX
// slab depth and tile of the direct-to-LDS bf16x3 forms (gemm_x3d_kernel, gemm_x3w_kernel)
#define X3D_BK 32
#define X3D_T 128

