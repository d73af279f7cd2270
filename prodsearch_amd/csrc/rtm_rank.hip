// rtm_rank.hip — the review transformer over the WHOLE catalogue in one pass (include/prodsearch_hip.h,
// ps_rtm_rank_*).  Reference: Trainer.test with test_candi_size < 1 (trainer.py:141-143, 189-226), which feeds ProductRanker.test
// (ps_model.py:205-239) chunks of candidates and runs the whole encoder over every (entry, candidate) sequence.
//
// With ONE encoder layer three things hold:
//   * layer 0 has no LayerNorm in front of its attention (transformer.py:48-51), so a key / value row is linear in its token:
//       K(rev[r] + seg[s] + user_emb[u] + product_emb[i] + pe[pos]) = Wk.(rev[r] + user_emb[u] + product_emb[i]) + (Wk.(seg[s] + pe[pos]) + bk)
//   * every per-review term depends on the review id alone — a review has one author and one item (global_data.review_u_p;
//     prod_search_dataloader.py:78-85 puts exactly those ids at the review's position) — so KR / VR [review_count, d] are
//     projected once per evaluation and what remains per token is a [segment][position] table;
//   * only position 0 is consumed and its residual is the query token, the same for every candidate of an entry: candidates are
//     to an entry what dropout replicas are to a sequence in encoder.hip — K / V / Q once per entry (n_in = B), the tail per pair.
// The softmax over [query | user's reviews | item's reviews] splits like an online softmax: the running (max, sum, weighted V) over
// {query, user's reviews} is taken once per entry, and every pair continues it over the item's reviews.
//   rr_table / rr_segpos   index: T[r] = rev[r] (+ user_emb) (+ product_emb); Z[s][pos] = seg[s] + pe[pos]  -> the fp32-grade GEMM
//   rr_x0 / rr_entry       per entry: the query token's row, then the softmax state over its 1 + n_u keys (one wave per entry)
//   rr_pair                per (entry, item): an item tile's K / V rows sit in LDS while the workgroup's waves walk the entries
//   rr_head                wo . enc + b into the dense score matrix; the selection is rank.hip's (rank.h)
// The same pass over per-entry CANDIDATE LISTS (include/prodsearch_rtm_cand.h, ps_rtm_rank_cand_* /
// ps_rtm_rank_candidates: sampled validation, the rerank of test_candi_size lists) shares the index and the entry side:
//   rr_slot<EPL, false>    per (entry, slot of its list): one wave per pair, the K / V rows straight from KR / VR — no LDS tile,
//                          two entries' lists have no item in common
//   rr_head / rr_cand_target / _ids   scores [B, C] (-inf at dead slots), the target's column, the selected columns -> item ids
// The TIME-ORDERED evaluation (include/prodsearch_rtm_seq.h, ps_rtm_rank_seq*: do_seq_review_test without
// train_review_only) keeps the index and the entry side too; what changes is which review ids a pair reads:
//   rr_slot<EPL, true>     per (entry, slot): the item's time-ordered sequence is searched wave-wide for the entry's time stamp and the
//                          iprev_review_limit reviews just before the cut are the pair's list
// Every key / value walk is rr_walk — the one call of rr_step — over a row source (review ids held one per lane, or a
// workgroup's LDS tile), and the three launch entries are one driver (rr_run) over one column description (RrCols): a further
// column source adds a row source or a slot rule and nothing else.
// fp32 throughout, plain C++; the per-pair tail is the encoder's own (enc_tail_forward).
#include "rtm.h"
#include "../../include/prodsearch_rtm_cand.h"
#include "../../include/prodsearch_rtm_seq.h"
#include "rank.h"
#include "wgrad.h"      // gp / run1
#include <math.h>
#include <string.h>
#include <type_traits>

#define RR_IT_MAX 16                 // items of one workgroup's tile
#define RR_LDS_MAX (128 * 1024)      // bytes of K / V rows a workgroup may hold
#define RR_PASS_PAIRS 32768          // default pairs per pass (ps_rtm_rank_scratch_bytes)

static int rr_check(const PsRtmDesc& D, const PsRtmRankShape& S) {
  PS_REQUIRE(D.n_layers == 1, "rtm rank_all: inter_layers = %d: one encoder layer is built (deeper encoders need every position of layer 0)", D.n_layers);
  PS_REQUIRE(!S.seq_review_test, "rtm rank_all: do_seq_review_test without train_review_only: an item's review list then depends on the entry");
  PS_REQUIRE(!(S.fix_emb && (D.review_encoder == PS_RENC_FS || D.review_encoder == PS_RENC_AVG)),
             "rtm rank_all: fix_emb with the fs / avg review encoders is not built");
  PS_REQUIRE(D.review_encoder >= PS_RENC_PV && D.review_encoder <= PS_RENC_AVG, "rtm rank_all: review encoder %d", D.review_encoder);
  // (R only sizes the [segment][position] tables and caps a sequence: bounded by the positional table's 5000 rows, transformer.py:10-17)
  PS_REQUIRE(D.B > 0 && D.Q > 0 && D.R > 0 && D.R + 1 <= 5000, "rtm rank_all: bad sizes B=%d Q=%d R=%d (R + 1 <= 5000)", D.B, D.Q, D.R);
  PS_REQUIRE(D.d == 64 || D.d == 128 || D.d == 256 || D.d == 512, "rtm rank_all: embedding_size %d (64, 128, 256, 512)", D.d);
  PS_REQUIRE(D.H > 0 && D.H <= 64 && (D.H & (D.H - 1)) == 0 && D.d % D.H == 0, "rtm rank_all: heads %d (a power of two <= 64)", D.H);
  PS_REQUIRE(D.F > 0 && D.F % 4 == 0, "rtm rank_all: ff_size %d", D.F);
  PS_REQUIRE(D.review_count > 1 && D.review_count < ((int64_t)1 << 31) && D.vocab_size > 1, "rtm rank_all: table sizes");
  PS_REQUIRE(S.n_items >= 1 && S.n_items < ((int64_t)1 << 31), "rtm rank_all: %lld items", (long long)S.n_items);
  PS_REQUIRE(S.I >= 1 && S.I <= 64 && S.U >= 1 && S.U <= 64, "rtm rank_all: I=%d U=%d reviews per item / user (1..64)", S.I, S.U);
  PS_REQUIRE((size_t)S.I * 2 * D.d * sizeof(float) <= RR_LDS_MAX, "rtm rank_all: %d reviews of %d floats do not fit a workgroup's LDS", S.I, D.d);
  PS_REQUIRE(S.review_u_p_rows >= 0 && S.review_u_p_rows <= D.review_count, "rtm rank_all: review_u_p rows");
  return PS_OK;
}

static inline int64_t rtake(int64_t& cur, int64_t n) { int64_t o = cur; cur += (n + 63) & ~(int64_t)63; return o; }   // 256-byte steps

// ------------------------------------------------------------------ the projection's layout (floats)
struct RrIndex { int64_t KR, VR, kt, vt, Z, T, total; int T1; };
static RrIndex rr_index_layout(const PsRtmDesc& D) {
  RrIndex x;
  const int64_t d = D.d, RC = D.review_count;
  x.T1 = D.R + 1;
  int64_t cur = 0;
  x.KR = rtake(cur, RC * d); x.VR = rtake(cur, RC * d);
  x.kt = rtake(cur, 2 * (int64_t)x.T1 * d); x.vt = rtake(cur, 2 * (int64_t)x.T1 * d);
  x.Z = rtake(cur, 2 * (int64_t)x.T1 * d);
  x.T = (D.use_user_emb || D.use_item_emb) ? rtake(cur, RC * d) : -1;
  x.total = cur;
  return x;
}

// ------------------------------------------------------------------ one call's scratch (floats from its start)
struct RrWs {
  Ws w;                       // the tail's slice, laid out for enc_tail_forward: n_in = B, fan = tile, S = 1, qpos = 0
  int64_t qmean, qemb, x0, qp, k0, v0, em, es, eacc, entn, S, sel, total;
  int64_t tcol;               // RrCols::tcol: the target's column per entry (int64)
  int64_t ldS, sel_bytes;
  int tile;
  bool fuse;
};
static bool rr_tail_fused(const PsRtmDesc& D) { return ps_fusion_enabled() && mlp_fused_serves(D.d, D.F); }
// The scored columns of a call: the catalogue's items, or the slots of the entries' candidate lists.  One description serves the
// layout, the pass size, the plans and the driver; `name` / `unit` word the messages of the entry it was made for.
struct RrCols {
  int64_t n;                  // columns per entry
  bool list;                  // they are the slots of per-entry lists: dead slots, the selection over columns -> item ids
  bool tcol;                  // the scratch ends with the target's column per entry (int64)
  const char *name, *unit;
};
static RrCols rr_all_cols(const PsRtmRankShape& S) { return RrCols{S.n_items, false, false, "rtm rank_all", "item"}; }
static int rr_cand_cols(int64_t C, RrCols& c) {
  PS_REQUIRE(C >= 1 && C < ((int64_t)1 << 31), "rtm rank_candidates: %lld candidates per entry (at least 1)", (long long)C);
  c = RrCols{C, true, true, "rtm rank_candidates", "candidate"};
  return PS_OK;
}
// the time-ordered entries: the slots of the lists (C of them) or, with no list, the P catalogue rows
static int rr_seq_cols(const PsRtmRankShape& S, int64_t C, bool list, RrCols& c) {
  const int64_t cols = list ? C : S.n_items;
  PS_REQUIRE(!list || cols >= 1, "rtm rank_seq: %lld candidates per entry (at least 1)", (long long)cols);
  PS_REQUIRE(cols >= 1 && cols < ((int64_t)1 << 31), "rtm rank_seq: %lld columns", (long long)cols);
  c = RrCols{cols, list, true, "rtm rank_seq", "slot"};
  return PS_OK;
}
// `tile` of the columns per pass
static int rr_layout(const PsRtmDesc& D, const RrCols& c, int topk, int64_t tile, RrWs& r) {
  PS_REQUIRE(tile >= 1 && tile <= c.n && (int64_t)D.B * tile < ((int64_t)1 << 30), "%s: %lld %ss per pass", c.name, (long long)tile, c.unit);
  memset(&r, 0, sizeof(r));
  const int64_t B = D.B, d = D.d, F = D.F, P = c.n;
  r.tile = (int)tile;
  r.fuse = rr_tail_fused(D);
  r.sel_bytes = rank_select_scratch_bytes((int)B, P, topk);
  PS_REQUIRE(r.sel_bytes >= 0, "%s: topk must be 1..256", c.name);
  int64_t cur = 0;
  r.qmean = rtake(cur, B * d); r.qemb = rtake(cur, B * d); r.x0 = rtake(cur, B * d);
  r.qp = rtake(cur, B * d); r.k0 = rtake(cur, B * d); r.v0 = rtake(cur, B * d);
  r.em = rtake(cur, B * 64); r.es = rtake(cur, B * 64); r.eacc = rtake(cur, B * d); r.entn = rtake(cur, B);
  r.ldS = (P + 3) & ~(int64_t)3;
  r.S = rtake(cur, B * r.ldS);
  r.sel = rtake(cur, (r.sel_bytes + 3) / 4);
  Ws& w = r.w;
  w.R = 1; w.S = 1; w.qpos = 0;
  w.wsplit = r.fuse ? rtake(cur, mlp_x3_floats((int)d, (int)F)) : 0;
  LayerWs& l = w.layer[0];
  const int64_t M = B * tile;
  l.n_in = (int)B; l.fan = (int)tile; l.n_out = (int)M; l.Sq = 1; l.M2 = (int)M;
  l.ctx = rtake(cur, M * d); l.y1 = rtake(cur, M * d); l.ff_stats = rtake(cur, M * 2); l.ln1 = rtake(cur, M * d);
  l.a1 = rtake(cur, M * F); l.h1 = rtake(cur, M * F); l.y2 = rtake(cur, M * d);
  w.Mf = (int)M;
  w.fin_stats = rtake(cur, M * 2); w.enc = rtake(cur, M * d);
  w.total = cur;
  if (c.tcol) r.tcol = rtake(cur, 2 * (int64_t)B);
  r.total = cur;
  return PS_OK;
}

// ------------------------------------------------------------------ kernels
struct RrK {
  int B, d, lph, I, U, T1, tile, IT, P, i0, nv, ldS;
  int64_t RC;
  const int64_t *item_r, *u_r;
  const float *KR, *VR, *kt, *vt;      // kt / vt [2][T1][d]: segment 1 (user's reviews), segment 2 (item's reviews)
  const float *qp, *k0, *v0;
  float *em, *es, *eacc; int32_t* entn;
  float* ctx;
  const int64_t* candi; int C;         // rr_slot_kernel: the lists [B, C] (or null); i0 is the pass's first column
  const int64_t *tl_ptr, *tl_rids, *tl_times, *stamps; int64_t tl_n;   // rr_slot_kernel<EPL, true>: the timeline (CSR + times) and the entries' stamps [B]
};

// T[r] = rev[r] (+ user_emb[author]) (+ product_emb[item]) with the id rule of rtm_embed_kernel: an id outside [0, pad] adds nothing
__global__ __launch_bounds__(256) void rr_table_kernel(const float* rev, const int64_t* up, int64_t up_rows, const float* user_emb,
                                                       const float* item_emb, int64_t Upad, int64_t Ppad, int64_t RC, int d, float* out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (r >= RC) return;
  int64_t uid = -1, iid = -1;
  if (r < up_rows) {
    if (user_emb) { uid = up[2 * r]; if (uid < 0 || uid > Upad) uid = -1; }
    if (item_emb) { iid = up[2 * r + 1]; if (iid < 0 || iid > Ppad) iid = -1; }
  }
  for (int c = lane; c < d; c += 64) {
    float v = rev[r * d + c];
    if (uid >= 0) v += user_emb[uid * d + c];
    if (iid >= 0) v += item_emb[iid * d + c];
    out[r * d + c] = v;
  }
}
// Z[s][pos] = seg[1 + s] + pe[pos]  (s = 0: the user's reviews, 1: the item's), either term dropped with its flag
__global__ __launch_bounds__(256) void rr_segpos_kernel(const float* seg, const float* pe, int T1, int d, float* out) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= 2 * T1) return;
  const int s = row / T1, pos = row - s * T1;
  for (int c = lane; c < d; c += 64) {
    float v = 0.f;
    if (seg) v += seg[(size_t)(1 + s) * d + c];
    if (pe) v += pe[(size_t)pos * d + c];
    out[(size_t)row * d + c] = v;
  }
}
// the query token's row as rtm_embed_kernel builds it: query_emb + seg[0] + user_emb[pad] + product_emb[pad] + pe[0]
__global__ __launch_bounds__(256) void rr_x0_kernel(const float* qemb, const float* seg, const float* urow, const float* irow, const float* pe,
                                                    int B, int d, float* x0) {
  const int lane = threadIdx.x & 63;
  const int e = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (e >= B) return;
  for (int c = lane; c < d; c += 64) {
    float v = qemb[(size_t)e * d + c];
    if (seg) v += seg[c];
    if (urow) v += urow[c];
    if (irow) v += irow[c];
    if (pe) v += pe[c];
    x0[(size_t)e * d + c] = v;
  }
}

// RR_U key / value pairs join a head's running softmax at once (the first `live` of them count): lane owns EPL consecutive columns,
// the 64 / H lanes of a head add their dots.  One rescale per group: the dependent chain of a sequence is a quarter as long as
// key by key, and the group's loads are issued together.
#define RR_U 4
template <int EPL>
__device__ __forceinline__ void rr_step(const float (&q)[EPL], const float (&k)[RR_U][EPL], const float (&v)[RR_U][EPL], int live, int lph,
                                        float& m, float& s, float (&acc)[EPL]) {
  float dot[RR_U];
#pragma unroll
  for (int u = 0; u < RR_U; ++u) {
    dot[u] = 0.f;
#pragma unroll
    for (int i = 0; i < EPL; ++i) dot[u] = __builtin_fmaf(q[i], k[u][i], dot[u]);
  }
  for (int o = lph >> 1; o > 0; o >>= 1)
#pragma unroll
    for (int u = 0; u < RR_U; ++u) dot[u] += __shfl_xor(dot[u], o, 64);
  float mn = m;
#pragma unroll
  for (int u = 0; u < RR_U; ++u) { dot[u] = u < live ? dot[u] : -INFINITY; mn = fmaxf(mn, dot[u]); }
  const float sc = __expf(m - mn);
  float p[RR_U];
#pragma unroll
  for (int u = 0; u < RR_U; ++u) p[u] = __expf(dot[u] - mn);
  s = s * sc + ((p[0] + p[1]) + (p[2] + p[3]));
#pragma unroll
  for (int i = 0; i < EPL; ++i) acc[i] = acc[i] * sc + ((p[0] * v[0][i] + p[1] * v[1][i]) + (p[2] * v[2][i] + p[3] * v[3][i]));
  m = mn;
}
// the leading non-pad ids of a padded list held one per lane (ids outside the table count as the pad)
__device__ __forceinline__ int rr_leading(int id, int pad) {
  const unsigned long long inv = ~__ballot(id != pad);
  return inv ? __builtin_ctzll(inv) : 64;
}

// Where a walk's rows come from: two fixed bases and ONE offset per row, K[off(jj) + column] / V[off(jj) + column].  (Handing
// back a K and a V pointer per row instead costs the slot kernel six VGPRs and a wave of occupancy at d = 128.)
struct RrIdRows {                                    // by review id, held one per lane: rows of KR / VR
  const float *K, *V; int id, d;
  __device__ __forceinline__ size_t off(int jj) const { return (size_t)__shfl(id, jj, 64) * d; }
};
struct RrLdsRows {                                   // a workgroup's LDS tile [I][2][d]: K = the item's rows, V = K + d
  const float *K, *V; int d;
  __device__ __forceinline__ size_t off(int jj) const { return (size_t)(2 * jj) * d; }
};
// THE key / value walk: rows 0 .. n - 1 of `rows`, at positions pos0 .. of the [position] tables kt / vt, join the running softmax
// (m, s, acc) in groups of RR_U, the 2 * RR_U row loads of a group issued together.  Every kernel walks through here, so two of
// them that see the same rows give the same bits.
template <int EPL, class Rows>
__device__ __forceinline__ void rr_walk(const Rows rows, int n, int pos0, const float* kt, const float* vt, int d, size_t col, int lph,
                                        const float (&q)[EPL], float& m, float& s, float (&acc)[EPL]) {
  float k[RR_U][EPL], v[RR_U][EPL];
  for (int j = 0; j < n; j += RR_U) {
#pragma unroll
    for (int u = 0; u < RR_U; ++u) {
      const int jj = j + u < n ? j + u : n - 1;     // (a slot past the list repeats its last row; rr_step drops it)
      const size_t off = rows.off(jj) + col;
      const size_t pos = (size_t)(pos0 + jj) * d + col;
#pragma unroll
      for (int i = 0; i < EPL; ++i) {
        k[u][i] = rows.K[off + i] + kt[pos + i];
        v[u][i] = rows.V[off + i] + vt[pos + i];
      }
    }
    rr_step<EPL>(q, k, v, n - j, lph, m, s, acc);
  }
}
// the pair side of a walk: entry e's state over {query, the user's reviews} continues over `n` rows of an item at positions
// 1 + n_u .. (segment 2), and the normalised context row goes to `out`
template <int EPL, class Rows>
__device__ __forceinline__ void rr_pair_walk(const RrK& a, int e, const Rows rows, int n, int lane, float* out) {
  const int d = a.d, nu = a.entn[e];
  n = n < a.T1 - 1 - nu ? n : a.T1 - 1 - nu;        // the sequence never exceeds 1 + total_review_limit positions
  const size_t col = (size_t)lane * EPL;
  float q[EPL], acc[EPL];
#pragma unroll
  for (int i = 0; i < EPL; ++i) { q[i] = a.qp[(size_t)e * d + col + i]; acc[i] = a.eacc[(size_t)e * d + col + i]; }
  float m = a.em[(size_t)e * 64 + lane], s = a.es[(size_t)e * 64 + lane];
  rr_walk<EPL>(rows, n, 1 + nu, a.kt + (size_t)a.T1 * d, a.vt + (size_t)a.T1 * d, d, col, a.lph, q, m, s, acc);
  const float inv = 1.f / s;
#pragma unroll
  for (int i = 0; i < EPL; ++i) out[col + i] = acc[i] * inv;
}

// once per entry: the softmax state over {query token, the user's reviews at positions 1 .. n_u, segment 1}
template <int EPL>
__global__ __launch_bounds__(256) void rr_entry_kernel(const RrK a) {
  const int lane = threadIdx.x & 63;
  const int e = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (e >= a.B) return;
  const int pad = (int)(a.RC - 1), d = a.d;
  const int id = lane < a.U ? (int)rclamp(a.u_r[(size_t)e * a.U + lane], a.RC - 1) : pad;
  int nu = rr_leading(id, pad);
  nu = nu < a.T1 - 1 ? nu : a.T1 - 1;
  float q[EPL], acc[EPL];
  const size_t col = (size_t)lane * EPL;
  float m = 0.f, s = 1.f;                          // the query token's own key opens the state: weight exp(0) = 1 on v0
#pragma unroll
  for (int i = 0; i < EPL; ++i) {
    q[i] = a.qp[(size_t)e * d + col + i]; acc[i] = a.v0[(size_t)e * d + col + i];
    m = __builtin_fmaf(q[i], a.k0[(size_t)e * d + col + i], m);
  }
  m = group_sum(m, a.lph);
  rr_walk<EPL>(RrIdRows{a.KR, a.VR, id, d}, nu, 1, a.kt, a.vt, d, col, a.lph, q, m, s, acc);
  a.em[(size_t)e * 64 + lane] = m; a.es[(size_t)e * 64 + lane] = s;
#pragma unroll
  for (int i = 0; i < EPL; ++i) a.eacc[(size_t)e * d + col + i] = acc[i];
  if (lane == 0) a.entn[e] = nu;
}

// per (entry, item): the workgroup loads the K / V rows of its IT items once (unconditional, batched loads: a pad slot reads the
// pad review's row, an index past the tile repeats row 0) and its four waves walk the (entry, item) pairs; item t of the pass is
// catalogue row min(i0 + t, P - 1), so a ragged last pass runs at the full pass shape.
template <int EPL>
__global__ __launch_bounds__(256) void rr_pair_kernel(const RrK a) {
  extern __shared__ float kv[];                     // [IT][I][2][d]
  __shared__ int s_n[RR_IT_MAX];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int d = a.d, c4 = d >> 2, pad = (int)(a.RC - 1), total = a.I * c4;
  const int t0 = blockIdx.x * a.IT;
  for (int it = wv; it < a.IT; it += 4) {
    int gi = a.i0 + t0 + it;
    gi = gi < a.P ? gi : a.P - 1;
    const int id = lane < a.I ? (int)rclamp(a.item_r[(size_t)gi * a.I + lane], a.RC - 1) : pad;
    const int n = rr_leading(id, pad);
    if (lane == 0) s_n[it] = n;
    float* dst = kv + (size_t)it * a.I * 2 * d;
    for (int base = 0; base < total; base += 256) {
      float4 kk[4], vv[4]; int jj[4], cc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = base + 64 * u + lane;
        const int ix = idx < total ? idx : 0;
        jj[u] = ix / c4; cc[u] = ix - jj[u] * c4;
        const size_t r = (size_t)__shfl(id, jj[u], 64);
        kk[u] = *reinterpret_cast<const float4*>(a.KR + r * d + 4 * cc[u]);
        vv[u] = *reinterpret_cast<const float4*>(a.VR + r * d + 4 * cc[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (base + 64 * u + lane < total) {
          *reinterpret_cast<float4*>(dst + (size_t)(2 * jj[u]) * d + 4 * cc[u]) = kk[u];
          *reinterpret_cast<float4*>(dst + (size_t)(2 * jj[u] + 1) * d + 4 * cc[u]) = vv[u];
        }
    }
  }
  __syncthreads();
  for (int p = wv; p < a.B * a.IT; p += 4) {
    const int e = p / a.IT, it = p - e * a.IT;
    if (t0 + it >= a.tile) continue;                // (wave-uniform)
    const float* src = kv + (size_t)it * a.I * 2 * d;
    rr_pair_walk<EPL>(a, e, RrLdsRows{src, src + d, d}, s_n[it], lane, a.ctx + ((size_t)e * a.tile + t0 + it) * d);
  }
}

// per (entry, slot): one wave per pair.  The slot's item is the entry's own list's (candi: slot t of the pass is column
// min(i0 + t, C - 1), a dead slot — an id outside [0, P) — is computed on item 0 and rr_head_kernel writes its score as -inf), or
// without a list catalogue row min(i0 + t, P - 1); either way a ragged last pass runs at the full pass shape and every load stays
// unconditional.  Two entries' lists have no item in common, so an LDS tile would amortise nothing: the K / V rows come by review
// id straight from KR / VR, as in rr_entry_kernel.
//   SEQ = false: the pair's list is the item's static [P, I] row; always launched with lists.
//   SEQ = true:  the time-ordered evaluation (do_seq_review_test without train_review_only, prod_search_dataloader.py:60-77,
// 138-147): the list is the I reviews of the item just before a cut in the item's time-ordered sequence, cut = bisect_right(times
// of the sequence, the entry's stamp).  The search is wave-wide: each round the 64 lanes probe 64 evenly spaced elements of the
// open range, one ballot of time <= stamp and its population count leave the stretch between two probes: one round up to 64
// reviews, two up to 4,160, three up to 266,304.  Every load of the search and of the window is unconditional on an index clamped
// into [0, N - 1] (N >= 1); what a lane may use of it is decided afterwards.
// From the list on both are rr_pair_walk, so a pair's bits are those of rr_pair_kernel on the same list.
template <int EPL, bool SEQ>
__global__ __launch_bounds__(256) void rr_slot_kernel(const RrK a) {
  const int lane = threadIdx.x & 63;
  const int p = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (p >= a.B * a.tile) return;                    // (wave-uniform)
  const int e = p / a.tile, t = p - e * a.tile;
  const int pad = (int)(a.RC - 1);
  int64_t gi;
  if (!SEQ || a.candi) {                            // (wave-uniform; the static rows without a list are rr_pair_kernel's)
    int c = a.i0 + t;
    c = c < a.C ? c : a.C - 1;
    gi = a.candi[(size_t)e * a.C + c];
    gi = (gi < 0 || gi >= a.P) ? 0 : gi;
  } else {
    gi = a.i0 + t;
    gi = gi < a.P ? gi : a.P - 1;
  }
  int id;
  if constexpr (SEQ) {
    const int64_t stamp = a.stamps[e], last = a.tl_n - 1;
    int64_t lo = a.tl_ptr[gi], hi = a.tl_ptr[gi + 1];
    lo = lo < 0 ? 0 : (lo > a.tl_n ? a.tl_n : lo);  // (a corrupt ptr cannot send a load outside the arrays)
    hi = hi < lo ? lo : (hi > a.tl_n ? a.tl_n : hi);
    // the cut lies in [b0, b1]: every element before b0 is <= stamp, every element from b1 on is greater
    int64_t b0 = lo, b1 = hi;
    while (b1 > b0) {                               // (wave-uniform: b0 / b1 come from ballots)
      const int64_t len = b1 - b0, step = (len + 63) >> 6;
      const int64_t off = (int64_t)lane * step;
      int64_t ix = b0 + off;
      ix = ix < last ? ix : last;
      const bool le = a.tl_times[ix] <= stamp && off < len;
      const int c = __popcll(__ballot(le));          // the probes are in time order: the first c of them hold
      if (c == 0) { b1 = b0; break; }
      const int64_t nb1 = b0 + (int64_t)c * step;
      b0 = b0 + (int64_t)(c - 1) * step + 1;
      b1 = nb1 < b1 ? nb1 : b1;
    }
    const int64_t cut = b0 - lo;
    const int nraw = (int)(cut < a.I ? cut : a.I);
    int64_t wx = b0 - nraw + lane;
    wx = wx < 0 ? 0 : (wx < last ? wx : last);
    const int rid = (int)rclamp(a.tl_rids[wx], a.RC - 1);
    id = lane < nraw ? rid : pad;
  } else {
    id = lane < a.I ? (int)rclamp(a.item_r[(size_t)gi * a.I + lane], a.RC - 1) : pad;
  }
  rr_pair_walk<EPL>(a, e, RrIdRows{a.KR, a.VR, id, a.d}, rr_leading(id, pad), lane, a.ctx + ((size_t)e * a.tile + t) * a.d);
}

// S[e][c0 + t] = wo . enc[e * tile + t] + b  (rtm_score_kernel's sum order), one wave per pair; with the entries' lists (candi, may
// be null) -inf for a dead slot
__global__ __launch_bounds__(256) void rr_head_kernel(const float* enc, const float* wo_w, const float* wo_b, const int64_t* candi,
                                                      int B, int tile, int nv, int d, int c0, int C, int P, int ldS, float* S) {
  const int lane = threadIdx.x & 63;
  const int n = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (n >= B * tile) return;
  const int e = n / tile, t = n - e * tile;
  if (t >= nv) return;
  float s = 0.f;
  for (int c = lane; c < d; c += 64) s += enc[(size_t)n * d + c] * wo_w[c];
  s = wave_sum(s) + wo_b[0];
  if (candi) {                                      // (uniform)
    const int64_t gi = candi[(size_t)e * C + c0 + t];
    s = (gi < 0 || gi >= P) ? -INFINITY : s;
  }
  if (lane == 0) S[(size_t)e * ldS + c0 + t] = s;
}
// the first live column of every entry's list that holds its target; C (not a column: rank 0) where there is none.  One wave per entry.
__global__ __launch_bounds__(256) void rr_cand_target_kernel(const int64_t* candi, const int64_t* target, int B, int C, int P, int64_t* tcol) {
  const int lane = threadIdx.x & 63;
  const int e = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (e >= B) return;
  const int64_t tg = target[e];
  const bool ok = tg >= 0 && tg < P;
  int best = C;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int c = c0 + lane, cc = c < C ? c : C - 1;
    const int64_t gi = candi[(size_t)e * C + cc];
    best = (ok && c < best && gi == tg) ? c : best;   // (c < best <= C: a lane keeps its first hit)
  }
  for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(best, o, 64); best = other < best ? other : best; }
  if (lane == 0) tcol[e] = best;
}
// the selected columns -> item ids; a dead slot that filled a place (fewer live slots than topk) reads as unfilled
__global__ __launch_bounds__(256) void rr_cand_ids_kernel(const int64_t* candi, int B, int C, int topk, int64_t* top_idx, const float* top_score) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= B * topk) return;
  const int e = n / topk;
  const int64_t c = top_idx[n];
  top_idx[n] = (c < 0 || c >= C || top_score[n] == -INFINITY) ? -1 : candi[(size_t)e * C + c];
}

// ------------------------------------------------------------------ host side
static void rr_tem_tensors(const PsRtmTensors& R, PsTemTensors& T) {
  memset(&T, 0, sizeof(T));
  T.word_emb = R.word_emb; T.fs_w = R.fs_w; T.fs_b = R.fs_b; T.pe = R.pe;
  T.final_ln_g = R.final_ln_g; T.final_ln_b = R.final_ln_b;
  T.layer[0] = R.layer[0];
}
static PsTemDesc rr_enc_desc(const PsRtmDesc& D) {
  PsTemDesc E;
  memset(&E, 0, sizeof(E));
  E.B = D.B; E.Q = 1; E.d = D.d; E.H = D.H; E.F = D.F; E.n_layers = 1;
  E.product_size = 1; E.vocab_size = 2;
  E.model = PS_MODEL_TEM; E.query_encoder = PS_QENC_AVG;
  return E;                                         // (training = 0: no dropout site draws)
}
static int rr_layer_check(const PsRtmTensors& P) {
  const PsLayerTensors& L = P.layer[0];
  PS_REQUIRE(L.wk && L.wv && L.wq && L.wo && L.w1 && L.w2 && L.bk && L.bv && L.bq && L.bo && L.b1 && L.b2 && L.ff_ln_g && L.ff_ln_b &&
             P.final_ln_g && P.final_ln_b && P.wo_w && P.wo_b, "rtm rank_all: null encoder tensors");
  return PS_OK;
}

extern "C" int64_t ps_rtm_rank_index_floats(const PsRtmDesc* desc, const PsRtmRankShape* shape) {
  if (!desc || !shape) { ps_set_error("rtm rank index: null argument"); return -1; }
  if (rr_check(*desc, *shape)) return -1;
  return rr_index_layout(*desc).total;
}

extern "C" int ps_rtm_rank_index(const PsRtmDesc* desc, const PsRtmRankShape* shape, const PsRtmTensors* params,
                                 const float* review_embeddings, const int64_t* review_u_p, float* index_out, ps_stream_t stream) {
  PS_REQUIRE(desc && shape && params && review_embeddings && index_out, "rtm rank index: null argument");
  const PsRtmDesc& D = *desc;
  const PsRtmTensors& P = *params;
  TRY(rr_check(D, *shape));
  TRY(rr_layer_check(P));
  PS_REQUIRE(!D.use_seg_emb || P.seg_emb, "rtm rank index: null segment table");
  PS_REQUIRE(!D.use_pos_emb || P.pe, "rtm rank index: null positional table");
  PS_REQUIRE(!D.use_user_emb || (P.user_emb && review_u_p), "rtm rank index: use_user_emb needs user_emb and review_u_p");
  PS_REQUIRE(!D.use_item_emb || (P.product_emb && review_u_p), "rtm rank index: use_item_emb needs product_emb and review_u_p");
  hipStream_t st = (hipStream_t)stream;
  const RrIndex x = rr_index_layout(D);
  const int d = D.d, RC = (int)D.review_count;
  const float* T = review_embeddings;
  if (x.T >= 0) {     // (neither embedding: the review table is used as it is)
    hipLaunchKernelGGL(rr_table_kernel, dim3(ps_cdiv(RC, 4)), dim3(256), 0, st, review_embeddings, review_u_p, shape->review_u_p_rows,
                       D.use_user_emb ? P.user_emb : nullptr, D.use_item_emb ? P.product_emb : nullptr, D.user_size, D.product_size,
                       D.review_count, d, index_out + x.T);
    PS_LAUNCH_CHECK();
    T = index_out + x.T;
  }
  hipLaunchKernelGGL(rr_segpos_kernel, dim3(ps_cdiv(2 * x.T1, 4)), dim3(256), 0, st, D.use_seg_emb ? P.seg_emb : nullptr,
                     D.use_pos_emb ? P.pe : nullptr, x.T1, d, index_out + x.Z);
  PS_LAUNCH_CHECK();
  const PsLayerTensors& L = P.layer[0];
  TRY(run1(gp(T, d, 0, L.wk, d, 0, index_out + x.KR, d, RC, d, d), st));
  TRY(run1(gp(T, d, 0, L.wv, d, 0, index_out + x.VR, d, RC, d, d), st));
  GemmProblem pk = gp(index_out + x.Z, d, 0, L.wk, d, 0, index_out + x.kt, d, 2 * x.T1, d, d);
  pk.bias = L.bk;
  TRY(run1(pk, st));
  GemmProblem pv = gp(index_out + x.Z, d, 0, L.wv, d, 0, index_out + x.vt, d, 2 * x.T1, d, d);
  pv.bias = L.bv;
  return run1(pv, st);
}

// ---- what a call launches: the launch entries and the plans read the same rules
static int64_t rr_default_tile(const PsRtmDesc& D, int64_t cols) {
  int64_t t = RR_PASS_PAIRS / D.B;
  t = t < 1 ? 1 : t;
  return t < cols ? t : cols;
}
// bytes of scratch with `per_pass` columns per pass (<= 0: the default), -1: refused
static int64_t rr_scratch_bytes(const PsRtmDesc& D, const RrCols& c, int topk, int64_t per_pass) {
  int64_t tile = per_pass > 0 ? per_pass : rr_default_tile(D, c.n);
  if (tile > c.n) tile = c.n;
  RrWs r;
  if (rr_layout(D, c, topk, tile, r)) return -1;
  return r.total * (int64_t)sizeof(float);
}
// items per workgroup: as many as ~48 KB of K / V rows hold (at least one), so several workgroups share a CU
static int rr_items_per_workgroup(int I, int d, int tile) {
  const size_t per = (size_t)I * 2 * d * sizeof(float);
  int it = (int)((48 * 1024) / per);
  it = it < 1 ? 1 : (it > RR_IT_MAX ? RR_IT_MAX : it);
  return it < tile ? it : tile;
}
static int rr_epl(const PsRtmDesc& D) { return D.d / 64; }     // columns per lane: the instantiation of the entry / pair / slot kernels
static int rr_lph(const PsRtmDesc& D) { return 64 / D.H; }     // lanes per head: the width of a logit's cross-lane sum
static size_t rr_pair_lds(int IT, int I, int d) { return (size_t)IT * I * 2 * d * sizeof(float); }   // rr_pair_kernel's dynamic LDS
static bool rr_query_fs_fused(const PsRtmDesc& D) { return D.query_encoder == PS_QENC_FS && ps_fusion_enabled() && D.d <= 128; }
// the pass size comes from the scratch: the most columns whose pairs fit (the layout grows with the tile)
static int rr_pass_layout(const PsRtmDesc& D, const RrCols& c, int topk, int64_t scratch_bytes, RrWs& r) {
  TRY(rr_layout(D, c, topk, 1, r));
  PS_REQUIRE(r.total * (int64_t)sizeof(float) <= scratch_bytes, "%s: scratch %lld < %lld bytes (one %s per pass)", c.name,
             (long long)scratch_bytes, (long long)(r.total * (int64_t)sizeof(float)), c.unit);
  int64_t lo = 1, hi = c.n;
  while ((int64_t)D.B * hi >= ((int64_t)1 << 30)) hi >>= 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    RrWs t;
    if (rr_layout(D, c, topk, mid, t) == PS_OK && t.total * (int64_t)sizeof(float) <= scratch_bytes) lo = mid; else hi = mid - 1;
  }
  return rr_layout(D, c, topk, lo, r);
}
// the fields the three plans share; `per_pass` is the plan's own name for the pass size
template <class Plan>
static int rr_plan(const PsRtmDesc& D, const RrCols& c, int topk, int64_t scratch_bytes, int64_t Plan::*per_pass, Plan* out) {
  RrWs r;
  TRY(rr_pass_layout(D, c, topk, scratch_bytes, r));
  out->*per_pass = r.tile;
  out->passes = (c.n + r.tile - 1) / r.tile;
  out->epl = rr_epl(D);
  out->lph = rr_lph(D);
  out->tail_fused = r.fuse ? 1 : 0;
  out->query_fs_fused = rr_query_fs_fused(D) ? 1 : 0;
  return PS_OK;
}

// the one dispatch on the columns per lane: f(std::integral_constant<int, EPL>) at the descriptor's EPL
template <class F>
static int rr_with_epl(int epl, F&& f) {
  if (epl == 1) return f(std::integral_constant<int, 1>());
  if (epl == 2) return f(std::integral_constant<int, 2>());
  if (epl == 4) return f(std::integral_constant<int, 4>());
  return f(std::integral_constant<int, 8>());
}
// a pass's walk: one wave per (entry, slot) where the columns come from a timeline or from lists, the catalogue's item tiles
// through LDS otherwise.  The kernel timer's label is the launching entry's.
static int rr_launch_walk(const RrK& k, int epl, hipStream_t st) {
  return rr_with_epl(epl, [&](auto E) -> int {
    constexpr int EPL = decltype(E)::value;
    if (k.tl_ptr || k.candi) {
      const dim3 pg(ps_cdiv((int64_t)k.B * k.tile, 4));
      KTimeScope kt(k.tl_ptr ? "rtm_rank_seq" : "rtm_rank_cand", st);
      if (k.tl_ptr) PS_KLAUNCH((rr_slot_kernel<EPL, true>), pg, dim3(256), 0, st, k);
      else PS_KLAUNCH((rr_slot_kernel<EPL, false>), pg, dim3(256), 0, st, k);
      PS_LAUNCH_CHECK();
      return PS_OK;
    }
    const size_t lds = rr_pair_lds(k.IT, k.I, k.d);
    // (a function attribute is per device: set whenever the tile needs more than the default 64 KB, not once per process)
    if (lds > 64 * 1024)
      PS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rr_pair_kernel<EPL>), hipFuncAttributeMaxDynamicSharedMemorySize, RR_LDS_MAX));
    KTimeScope kt("rtm_rank_pair", st);
    PS_KLAUNCH((rr_pair_kernel<EPL>), dim3(ps_cdiv(k.tile, k.IT)), dim3(256), lds, st, k);
    PS_LAUNCH_CHECK();
    return PS_OK;
  });
}

// ---- the entry side, once per call, the same for every launch entry: the shared query encoder (as
// rtm_encode), the query token, K / V / Q of it, the softmax state over {query, the user's reviews}.  Fills the encoder's view of
// the tensors and the kernels' arguments for the passes that follow.
struct RrCall {
  PsTemDesc E;
  PsTemTensors Tt;                                   // the tail's view: no K / V streams in the weight split
  WSplit x3;                                         // ... (all zero without the fused tail)
  RrK k;
  int epl;
};
static int rr_entry_side(const PsRtmDesc& D, const PsRtmRankShape& Sh, const PsRtmTensors& P, const float* index, const int64_t* item_ridxs,
                         const int64_t* query_word_idxs, const int64_t* u_ridxs, const RrWs& r, float* ws, hipStream_t st, RrCall& c) {
  const int B = D.B, d = D.d;
  const RrIndex x = rr_index_layout(D);
  c.E = rr_enc_desc(D);
  const PsTemDesc& E = c.E;
  PsTemTensors T;
  rr_tem_tensors(P, T);
  c.Tt = T;
  PsTemTensors& Tt = c.Tt;
  Tt.layer[0].wk = nullptr; Tt.layer[0].wv = nullptr;
  EmbedArgs e;
  memset(&e, 0, sizeof(e));
  e.B = B; e.Q = D.Q; e.L = 0; e.S = 1; e.d = d; e.P = 1; e.V = D.vocab_size; e.tem = 0;
  e.fs = D.query_encoder == PS_QENC_FS; e.qw = query_word_idxs; e.word_emb = P.word_emb;
  e.drop_fs = make_drop(E, PS_SITE_FS);
  e.qmean_d = ws + r.qmean; e.query_emb = ws + r.qemb;
  PS_REQUIRE(!e.fs || (P.fs_w && P.fs_b), "rtm rank_all: null FS encoder weights");
  const bool fs_fused = rr_query_fs_fused(D);
  if (fs_fused) { e.fs_w = P.fs_w; e.fs_b = P.fs_b; }
  if (r.fuse) { e.split = make_wsplit(E, Tt, ws, r.w); e.split_fwd_only = 1; }
  PS_REQUIRE(!r.fuse || e.split.on, "rtm rank_all: the fused tail's weight split is missing");
  c.x3 = e.split;
  TRY(launch_embed_fwd(e, st));
  if (e.fs && !fs_fused) {
    GemmProblem p = gp(ws + r.qmean, d, 0, P.fs_w, d, 0, ws + r.qemb, d, B, d, d);
    p.bias = P.fs_b; p.act = ACT_TANH;
    TRY(run1(p, st));
  }
  hipLaunchKernelGGL(rr_x0_kernel, dim3(ps_cdiv(B, 4)), dim3(256), 0, st, ws + r.qemb, D.use_seg_emb ? P.seg_emb : nullptr,
                     D.use_user_emb ? P.user_emb + (size_t)D.user_size * d : nullptr,
                     D.use_item_emb ? P.product_emb + (size_t)D.product_size * d : nullptr, D.use_pos_emb ? P.pe : nullptr, B, d, ws + r.x0);
  PS_LAUNCH_CHECK();
  {
    const PsLayerTensors& L = P.layer[0];
    GemmGroup g;
    memset(&g, 0, sizeof(g));
    g.n = 3;
    g.p[0] = gp(ws + r.x0, d, 0, L.wk, d, 0, ws + r.k0, d, B, d, d); g.p[0].bias = L.bk;
    g.p[1] = gp(ws + r.x0, d, 0, L.wv, d, 0, ws + r.v0, d, B, d, d); g.p[1].bias = L.bv;
    g.p[2] = gp(ws + r.x0, d, 0, L.wq, d, 0, ws + r.qp, d, B, d, d); g.p[2].bias = L.bq;
    g.p[2].alpha = 1.f / sqrtf((float)(d / D.H));    // Q pre-divided by sqrt(dh) (neural.py:206)
    TRY(ps_launch_gemm(g, st));
  }
  RrK& k = c.k;
  memset(&k, 0, sizeof(k));
  k.B = B; k.d = d; k.lph = rr_lph(D); k.I = Sh.I; k.U = Sh.U; k.T1 = x.T1; k.tile = r.tile; k.P = (int)Sh.n_items; k.ldS = (int)r.ldS;
  k.RC = D.review_count;
  k.item_r = item_ridxs; k.u_r = u_ridxs;
  k.KR = index + x.KR; k.VR = index + x.VR; k.kt = index + x.kt; k.vt = index + x.vt;
  k.qp = ws + r.qp; k.k0 = ws + r.k0; k.v0 = ws + r.v0;
  k.em = ws + r.em; k.es = ws + r.es; k.eacc = ws + r.eacc; k.entn = reinterpret_cast<int32_t*>(ws + r.entn);
  k.ctx = ws + r.w.layer[0].ctx;
  k.IT = rr_items_per_workgroup(Sh.I, d, r.tile);
  const dim3 eg(ps_cdiv(B, 4));
  c.epl = rr_epl(D);
  return rr_with_epl(c.epl, [&](auto E) -> int {
    hipLaunchKernelGGL(rr_entry_kernel<decltype(E)::value>, eg, dim3(256), 0, st, k);
    PS_LAUNCH_CHECK();
    return PS_OK;
  });
}
static int rr_tensor_check(const PsRtmDesc& D, const PsRtmTensors& P) {
  TRY(rr_layer_check(P));
  PS_REQUIRE(P.word_emb, "rtm rank_all: null word table");
  PS_REQUIRE(!D.use_seg_emb || P.seg_emb, "rtm rank_all: null segment table");
  PS_REQUIRE(!D.use_pos_emb || P.pe, "rtm rank_all: null positional table");
  PS_REQUIRE(!D.use_user_emb || P.user_emb, "rtm rank_all: use_user_emb needs user_emb");
  PS_REQUIRE(!D.use_item_emb || P.product_emb, "rtm rank_all: use_item_emb needs product_emb");
  return PS_OK;
}

// what every launch entry asks of its arguments after its own null checks, under its own name
static int rr_call_check(const char* name, const PsRtmDesc& D, const PsRtmRankShape& Sh, const PsRtmTensors& P, const int32_t* rank,
                         const int64_t* target_prod_idxs, const void* scratch) {
  TRY(rr_check(D, Sh));
  PS_REQUIRE(!rank || target_prod_idxs, "%s: rank needs target_prod_idxs", name);
  PS_REQUIRE((((uintptr_t)scratch) & 255) == 0, "%s: scratch must be 256-byte aligned", name);
  return rr_tensor_check(D, P);
}

// ---- THE driver of the three launch entries: the entry side, then passes over tiles of the columns — the walk (item tiles of
// the catalogue through LDS, or one wave per slot) -> the encoder's per-replica tail (n_in = B, fan = tile) -> head — and the
// selection.  `item_ridxs` [P, I] the static lists (null with a timeline), `candi` [B, cols.n] the entries' lists (null: the
// columns are the catalogue rows), `tl` / `stamps` the time-ordered evaluation's (null otherwise).
struct RrSrc { const int64_t *item_ridxs, *candi; const PsRtmSeqTimeline* tl; const int64_t* stamps; };
static int rr_run(const PsRtmDesc& D, const PsRtmRankShape& Sh, const PsRtmTensors& P, const float* index, const RrSrc& src, const RrCols& cols,
                  const int64_t* query_word_idxs, const int64_t* u_ridxs, const int64_t* target_prod_idxs, int32_t topk, int64_t* top_idx,
                  float* top_score, int32_t* rank, float* scores_out, void* scratch, int64_t scratch_bytes, ps_stream_t stream) {
  const int B = D.B, d = D.d;
  const int64_t N = cols.n;
  RrWs r;
  TRY(rr_pass_layout(D, cols, topk, scratch_bytes, r));
  hipStream_t st = (hipStream_t)stream;
  float* ws = reinterpret_cast<float*>(scratch);
  RrCall c;
  TRY(rr_entry_side(D, Sh, P, index, src.item_ridxs, query_word_idxs, u_ridxs, r, ws, st, c));
  RrK& k = c.k;
  k.candi = src.candi; k.C = cols.list ? (int)N : 0;
  if (src.tl) { k.tl_ptr = src.tl->ptr; k.tl_rids = src.tl->rids; k.tl_times = src.tl->times; k.tl_n = src.tl->n; k.stamps = src.stamps; }
  float* S = ws + r.S;
  for (int64_t c0 = 0; c0 < N; c0 += r.tile) {
    k.i0 = (int)c0;
    k.nv = (int)(c0 + r.tile <= N ? r.tile : N - c0);
    TRY(rr_launch_walk(k, c.epl, st));
    const EncBase eb = {c.E, c.Tt, ws, r.w, st};
    TRY(enc_tail_forward(eb, c.x3, 0, ws + r.x0, r.fuse, nullptr));
    if (!r.fuse) TRY(enc_final_ln_forward(eb));
    hipLaunchKernelGGL(rr_head_kernel, dim3(ps_cdiv((int64_t)B * r.tile, 4)), dim3(256), 0, st, ws + r.w.enc, P.wo_w, P.wo_b, src.candi, B,
                       r.tile, k.nv, d, k.i0, k.C, k.P, k.ldS, S);
    PS_LAUNCH_CHECK();
  }
  if (scores_out)
    PS_CHECK_HIP(hipMemcpy2DAsync(scores_out, (size_t)N * sizeof(float), S, (size_t)r.ldS * sizeof(float), (size_t)N * sizeof(float),
                                  (size_t)B, hipMemcpyDeviceToDevice, st));
  // ---- the selection is rank.hip's: over the catalogue rows, or over [B, C] with the columns as ids — the target's column
  // first, the columns -> item ids after
  if (!cols.list) return rank_select_scores(S, r.ldS, B, N, target_prod_idxs, topk, top_idx, top_score, rank, ws + r.sel, r.sel_bytes, st);
  int64_t* tcol = reinterpret_cast<int64_t*>(ws + r.tcol);
  if (target_prod_idxs) {
    hipLaunchKernelGGL(rr_cand_target_kernel, dim3(ps_cdiv(B, 4)), dim3(256), 0, st, src.candi, target_prod_idxs, B, (int)N, k.P, tcol);
    PS_LAUNCH_CHECK();
  }
  TRY(rank_select_scores(S, r.ldS, B, N, target_prod_idxs ? tcol : nullptr, topk, top_idx, top_score, rank, ws + r.sel, r.sel_bytes, st));
  hipLaunchKernelGGL(rr_cand_ids_kernel, dim3(ps_cdiv((int64_t)B * topk, 256)), dim3(256), 0, st, src.candi, B, (int)N, topk, top_idx,
                     top_score);
  PS_LAUNCH_CHECK();
  return PS_OK;
}

// ------------------------------------------------------------------ the whole catalogue (ps_rtm_rank_scratch_bytes / _plan / _all)
extern "C" int64_t ps_rtm_rank_scratch_bytes(const PsRtmDesc* desc, const PsRtmRankShape* shape, int32_t topk, int64_t items_per_pass) {
  if (!desc || !shape) { ps_set_error("rtm rank scratch: null argument"); return -1; }
  if (rr_check(*desc, *shape)) return -1;
  return rr_scratch_bytes(*desc, rr_all_cols(*shape), topk, items_per_pass);
}

extern "C" int ps_rtm_rank_plan(const PsRtmDesc* desc, const PsRtmRankShape* shape, int32_t topk, int64_t scratch_bytes,
                                PsRtmRankPlan* out) {
  PS_REQUIRE(desc && shape && out, "rtm rank plan: null argument");
  memset(out, 0, sizeof(*out));
  TRY(rr_check(*desc, *shape));
  TRY(rr_plan(*desc, rr_all_cols(*shape), topk, scratch_bytes, &PsRtmRankPlan::items_per_pass, out));
  out->items_per_workgroup = rr_items_per_workgroup(shape->I, desc->d, (int)out->items_per_pass);
  out->lds_bytes = (int32_t)rr_pair_lds(out->items_per_workgroup, shape->I, desc->d);
  return PS_OK;
}

extern "C" int ps_rtm_rank_all(const PsRtmDesc* desc, const PsRtmRankShape* shape, const PsRtmTensors* params, const float* index,
                               const int64_t* item_ridxs, const int64_t* query_word_idxs, const int64_t* u_ridxs,
                               const int64_t* target_prod_idxs, int32_t topk, int64_t* top_idx, float* top_score, int32_t* rank,
                               float* scores_out, void* scratch, int64_t scratch_bytes, ps_stream_t stream) {
  PS_REQUIRE(desc && shape && params && index && item_ridxs && query_word_idxs && u_ridxs && top_idx && top_score && scratch,
             "rtm rank_all: null argument");
  TRY(rr_call_check("rtm rank_all", *desc, *shape, *params, rank, target_prod_idxs, scratch));
  return rr_run(*desc, *shape, *params, index, RrSrc{item_ridxs, nullptr, nullptr, nullptr}, rr_all_cols(*shape), query_word_idxs, u_ridxs,
                target_prod_idxs, topk, top_idx, top_score, rank, scores_out, scratch, scratch_bytes, stream);
}

// ------------------------------------------------------------------ per-entry candidate lists (ps_rtm_rank_cand_*, ps_rtm_rank_candidates)
extern "C" int64_t ps_rtm_rank_cand_scratch_bytes(const PsRtmDesc* desc, const PsRtmRankShape* shape, int64_t C, int32_t topk,
                                                  int64_t cands_per_pass) {
  if (!desc || !shape) { ps_set_error("rtm rank_candidates scratch: null argument"); return -1; }
  RrCols cols;
  if (rr_check(*desc, *shape) || rr_cand_cols(C, cols)) return -1;
  return rr_scratch_bytes(*desc, cols, topk, cands_per_pass);
}

extern "C" int ps_rtm_rank_cand_plan(const PsRtmDesc* desc, const PsRtmRankShape* shape, int64_t C, int32_t topk, int64_t scratch_bytes,
                                     PsRtmRankCandPlan* out) {
  PS_REQUIRE(desc && shape && out, "rtm rank_candidates plan: null argument");
  memset(out, 0, sizeof(*out));
  TRY(rr_check(*desc, *shape));
  RrCols cols;
  TRY(rr_cand_cols(C, cols));
  return rr_plan(*desc, cols, topk, scratch_bytes, &PsRtmRankCandPlan::cands_per_pass, out);
}

extern "C" int ps_rtm_rank_candidates(const PsRtmDesc* desc, const PsRtmRankShape* shape, const PsRtmTensors* params, const float* index,
                                      const int64_t* item_ridxs, const int64_t* query_word_idxs, const int64_t* u_ridxs,
                                      const int64_t* candi_prod_idxs, int64_t C, const int64_t* target_prod_idxs, int32_t topk,
                                      int64_t* top_idx, float* top_score, int32_t* rank, float* scores_out, void* scratch,
                                      int64_t scratch_bytes, ps_stream_t stream) {
  PS_REQUIRE(desc && shape && params && index && item_ridxs && query_word_idxs && u_ridxs && candi_prod_idxs && top_idx && top_score && scratch,
             "rtm rank_candidates: null argument");
  TRY(rr_call_check("rtm rank_candidates", *desc, *shape, *params, rank, target_prod_idxs, scratch));
  RrCols cols;
  TRY(rr_cand_cols(C, cols));
  return rr_run(*desc, *shape, *params, index, RrSrc{item_ridxs, candi_prod_idxs, nullptr, nullptr}, cols, query_word_idxs, u_ridxs,
                target_prod_idxs, topk, top_idx, top_score, rank, scores_out, scratch, scratch_bytes, stream);
}

// ------------------------------------------------------------------ the time-ordered evaluation (ps_rtm_rank_seq*)
// The shape's seq_review_test says what the run is and is not a refusal here: rr_check sees the shape with the field cleared.
// (The host-only entries have no list pointer to look at: C = PS_RTM_SEQ_NO_LIST names the catalogue form there.)
static PsRtmRankShape rr_seq_shape(const PsRtmRankShape& S) { PsRtmRankShape s = S; s.seq_review_test = 0; return s; }

extern "C" int64_t ps_rtm_rank_seq_scratch_bytes(const PsRtmDesc* desc, const PsRtmRankShape* shape, int64_t C, int32_t topk,
                                                 int64_t slots_per_pass) {
  if (!desc || !shape) { ps_set_error("rtm rank_seq scratch: null argument"); return -1; }
  const PsRtmRankShape Sh = rr_seq_shape(*shape);
  RrCols cols;
  if (rr_check(*desc, Sh) || rr_seq_cols(Sh, C, C != PS_RTM_SEQ_NO_LIST, cols)) return -1;
  return rr_scratch_bytes(*desc, cols, topk, slots_per_pass);
}

extern "C" int ps_rtm_rank_seq_plan(const PsRtmDesc* desc, const PsRtmRankShape* shape, int64_t C, int32_t topk, int64_t scratch_bytes,
                                    PsRtmRankSeqPlan* out) {
  PS_REQUIRE(desc && shape && out, "rtm rank_seq plan: null argument");
  memset(out, 0, sizeof(*out));
  const PsRtmRankShape Sh = rr_seq_shape(*shape);
  TRY(rr_check(*desc, Sh));
  RrCols cols;
  TRY(rr_seq_cols(Sh, C, C != PS_RTM_SEQ_NO_LIST, cols));
  return rr_plan(*desc, cols, topk, scratch_bytes, &PsRtmRankSeqPlan::slots_per_pass, out);
}

extern "C" int ps_rtm_rank_seq(const PsRtmDesc* desc, const PsRtmRankShape* shape, const PsRtmTensors* params, const float* index,
                               const PsRtmSeqTimeline* timeline, const int64_t* query_word_idxs, const int64_t* u_ridxs,
                               const int64_t* time_stamps, const int64_t* candi_prod_idxs, int64_t C, const int64_t* target_prod_idxs,
                               int32_t topk, int64_t* top_idx, float* top_score, int32_t* rank, float* scores_out, void* scratch,
                               int64_t scratch_bytes, ps_stream_t stream) {
  PS_REQUIRE(desc && shape && params && index && query_word_idxs && u_ridxs && time_stamps && top_idx && top_score && scratch,
             "rtm rank_seq: null argument");
  PS_REQUIRE(timeline && timeline->ptr && timeline->rids && timeline->times, "rtm rank_seq: null timeline");
  PS_REQUIRE(timeline->n >= 1, "rtm rank_seq: a timeline of %lld reviews (at least 1)", (long long)timeline->n);
  const PsRtmRankShape Sh = rr_seq_shape(*shape);
  TRY(rr_call_check("rtm rank_seq", *desc, Sh, *params, rank, target_prod_idxs, scratch));
  RrCols cols;
  TRY(rr_seq_cols(Sh, C, candi_prod_idxs != nullptr, cols));
  return rr_run(*desc, Sh, *params, index, RrSrc{nullptr, candi_prod_idxs, timeline, time_stamps}, cols, query_word_idxs, u_ridxs,
                target_prod_idxs, topk, top_idx, top_score, rank, scores_out, scratch, scratch_bytes, stream);
}
