// rtm.h — private to the review transformer's files: the workspace layout and the kernel-side view of one call (rtm.hip fills
// both), the constants and device helpers its kernel families share, and the host stages each family's file implements
// (rtm_embed.hip, rtm_score.hip, rtm_index.hip, rtm_embed_bwd.hip).
#pragma once
#include "encoder.h"
#include "rowwise.h"

#define SITE_REV_PV 0x200u
#define SITE_REV_POS 0x201u
#define SITE_REV_NEG 0x202u
#define SITE_TOK_POS 0x203u
#define SITE_TOK_NEG 0x204u

struct RtmWs {
  int Bseq, S, J;
  int64_t qmean, query_emb, valid, vec, cnt, scores, weight, pv_scores, pv_terms, nvalid, dvec, dqe, dqpre, dqmean;
  int64_t loss_blk;         // the 64-bit loss / arrival word of rtm_score_kernel (cleared by the query-encoder launch)
  int64_t glist;            // int32 list of the review-row groups that hold at least one real review (rtm_grouplist_kernel)
  int64_t hist;             // int32 [RTM_HIST_G][V]: per-workgroup word histograms -> exclusive prefixes (rtm_hist_kernel / rtm_hist_scan_kernel)
  int64_t seqcnt;           // int32 [Bseq]: valid positions per sequence (rtm_embed_kernel -> rtm_rowlist_kernel)
  int64_t wrank;
  int64_t wcnt, woff, wcur, wl;   // pvc backward: inverted index word -> review slots (int32 arrays; wl: int2 {slot, word})
  int64_t segpart;          // [ceil(Bseq*S / 64)][3][d] parked segment-embedding gradient partials (rtm_embed_bwd_kernel)
  int64_t raw, yfs, dpre, dmean;                // fs review encoder: [Bseq*R, d] dropped means, projections, their gradients
  int64_t enc_base;         // the shared encoder workspace (Ws) starts here
  int64_t total;
};

struct RtmK {              // kernel-side view of one call
  int B, J, K, R, S, Q, W, WL, d;
  int64_t V, RC;
  int pvc, use_pos, use_seg, pos_weight, train_pv, training, eval;
  FDiv fJ, fS, fK1;
  DropSpec d_pv, d_pos, d_neg, t_pos, t_neg;
  // batch
  const int64_t *pos_r, *neg_r, *pos_seg, *neg_seg, *pos_words, *neg_words_rev, *pos_pvc, *neg_pvc, *neg_word_idxs;
  const int64_t *pos_u, *neg_u, *pos_i, *neg_i;   // per-position user / item ids (use_user_emb / use_item_emb), else null
  int64_t U, PI;                                  // their pad ids (user_size, product_size)
  const float *user_emb, *item_emb; float *g_user_emb, *g_item_emb;
  const uint8_t* pos_masks;
  // fs / avg review encoders (ps_model.py:301-305): the word-mean path of pvc with the BATCH's word masks deciding which
  // words count (text_encoder.py:6-16; pvc uses idx != pad, PVC.py:58) and no token corruption.  fs additionally
  // projects the mean: tanh(f_W . dropout(mean) + b) (text_encoder.py:32-40) — the embed kernels then leave the
  // dropped means in `raw` [B*R + B*K*R, d] (positive rows first), a GEMM writes `yfs`, rtm_fs_finish builds x.
  const uint8_t *wmask_pos, *wmask_neg;
  float *raw; const float* yfs; const float* dmean;   // dmean: backward, grad wrt raw (same layout)
  // tensors
  const float *word_emb, *table, *seg_emb, *pe, *wo_w, *wo_b;
  // workspace
  float *query_emb, *x, *valid, *vec, *cnt, *enc, *scores, *weight, *pv_scores, *pv_terms, *nvalid;
  int32_t *seqcnt, *vrows, *vcount;   // valid-row list of x (GemmProblem::ridx): per-sequence counts, rows, length
  int count_fwd;                      // rtm_embed4_kernel counts them (the counters were cleared by the query-encoder launch)
  int det;                            // deterministic mode (ps_deterministic): no fp32 atomic whose order could differ between runs
  unsigned long long* stamp;          // diagnostics (PS_RTM_STAMP=1, tools/rtm_stamps.py): phase stamps of one workgroup of rtm_embed4_kernel
  float* loss3;
  // backward
  float scale; const float* scale_dev;
  const float *dx; float *denc, *dvec, *dqe;
  float *g_word_emb, *g_table, *g_seg_emb, *g_wo_w, *g_wo_b;
  // pvc backward through an inverted index (word -> review slots) instead of one atomic row per word occurrence
  float* gs;                  // = dx, rewritten in place: row (n, s) becomes the gradient each of its words receives
  int *wcnt, *woff, *wcur;
  int2* wl;                   // the occurrence list: {slot, word}, one 8-byte store per occurrence
  int* wrank;                 // [B*R + B*K*R][WL] rank of a counted word among its word's occurrences, -1: not counted (count_fwd)
  int* hist; int hist_rows;   // LDS-histogram index (rtm_hist_kernel): [RTM_HIST_G][V]; review rows per histogram workgroup
};

// waves of rtm_embed_bwd_kernel: EB_GROUPS four-review groups per wave on each side, EB_QSEQ query slots per wave
#define EB_GROUPS 4
#define EB_QSEQ 16
static inline int rtm_eb_waves(int B, int K, int R, int* npos_w, int* nneg_w) {
  const int np = ps_cdiv((int64_t)B * R, 4 * EB_GROUPS), nn = ps_cdiv((int64_t)B * K * R, 4 * EB_GROUPS);
  if (npos_w) *npos_w = np;
  if (nneg_w) *nneg_w = nn;
  return np + nn + ps_cdiv((int64_t)B * (K + 1), EB_QSEQ);
}
#define RTM_HIST_G 256          // workgroups (= partitions of the review rows) of the LDS-histogram index
#define RTM_HIST_MAXV 38000     // vocabulary sizes whose histogram fits one workgroup's LDS (4 B per word, 160 KB)

// ------------------------------------------------------------------ device helpers more than one family uses
#if defined(__HIPCC__)
__device__ inline int64_t rclamp(int64_t i, int64_t hi) { return i < 0 ? hi : (i > hi ? hi : i); }
// does word slot `off` (= review row * WL + slot) count in its review's mean?
__device__ inline bool word_ok(const RtmK& a, const uint8_t* wm, size_t off, int64_t wi) {
  return (wm ? wm[off] != 0 : wi != a.V - 1) && wi >= 0 && wi < a.V;
}
// sequence n, position s -> batch row, member, review id (s > 0), review row on its side, segment id (, position in the id tensors)
__device__ inline void seq_decode(const RtmK& a, int n, int s, int& b, int& j, int64_t& ridx, int& revrow, int& seg,
                                  size_t* spos = nullptr) {
  b = fdiv(n, a.fJ); j = n - b * a.J;
  const int r = s - 1;
  if (a.eval || j > 0) {
    const int jj = a.eval ? j : j - 1, JN = a.eval ? a.J : a.K;
    const size_t base = ((size_t)b * JN + jj);
    ridx = s > 0 ? a.neg_r[base * a.R + r] : 0;
    seg = (int)a.neg_seg[base * a.S + s];
    revrow = (int)(base * a.R + r);
    if (spos) *spos = base * a.S + s;
  } else {
    ridx = s > 0 ? a.pos_r[(size_t)b * a.R + r] : 0;
    seg = (int)a.pos_seg[(size_t)b * a.S + s];
    revrow = b * a.R + r;
    if (spos) *spos = (size_t)b * a.S + s;
  }
}
#endif

// ------------------------------------------------------------------ host side: the stages of a call, one file per kernel family.
// A stage launches on the stream it is given and never chooses one: forks, joins and the side stream are rtm.hip's business.
// deterministic mode's scratch (ps_det_scratch, slot 1)
static inline int rtm_det_scratch(size_t floats, hipStream_t st, float** out) {
  *out = ps_det_scratch(1, floats, st);
  PS_REQUIRE(*out, "rtm backward: deterministic mode has no scratch (allocation failed or stream capture)");
  return PS_OK;
}

// rtm_embed.hip — the forward input assembly
bool rtm_embed4_taken(const PsRtmDesc& D, bool eval, const RtmWs& r);
// x (and, fs: raw) from the batch: the valid-group list where it applies, then the gather.  rowlist: the encoder walks the valid-row list
int rtm_embed_fwd(const PsRtmDesc& D, const RtmK& k, float* ws, const RtmWs& r, bool eval, bool rowlist, hipStream_t st);
int rtm_fs_finish(const RtmK& k, const RtmWs& r, hipStream_t st);
int rtm_rowlist(const RtmK& k, const RtmWs& r, hipStream_t st);
int rtm_review_table(const PsRtmDesc& D, const float* word_emb, const int64_t* review_words, float* out, hipStream_t st);

// rtm_score.hip — the head
int rtm_head_fwd(const RtmK& k, const RtmWs& r, float* ws, hipStream_t st);      // scores (+ PV terms + loss unless the loss is folded) -> k.loss3
int rtm_score_eval(const RtmK& k, const RtmWs& r, float* scores, hipStream_t st);
// d enc, d wo, the PV loss's d vec and word rows; its first launch carries the fork signal (sig, sigval) if there is one
int rtm_head_bwd(const RtmK& k, const RtmWs& r, const PsRtmBwdPlan& pl, uint32_t* sig, uint32_t sigval, hipStream_t st);

// rtm_index.hip — the inverted word index and the word-gradient reduce over it
bool rtm_hist_index(const PsRtmDesc& D, const RtmWs& r);
int rtm_build_index_hist(const RtmK& k, int V, hipStream_t st);
int rtm_build_index(const RtmK& k, const RtmWs& r, int V, bool count, hipStream_t st);
int rtm_word_reduce(const PsRtmDesc& D, const RtmK& k, const RtmWs& r, hipStream_t st);

// rtm_embed_bwd.hip — backward of the input assembly
int rtm_slot_blocks(const RtmWs& r);
// fs review projection: d pre = d x * tanh' for every review slot and the bias gradient (the two GEMMs behind it are the caller's)
int rtm_fs_bwd(const RtmK& k, const RtmWs& r, float* dpre, float* g_bias, hipStream_t st);
// d x -> segment partials (parked in `fold`), user / item / review rows, d query_emb, the per-word slot rows (k.gs)
int rtm_embed_bwd(const PsRtmDesc& D, const RtmK& k, const RtmWs& r, const PsRtmBwdPlan& pl, float* ws, ColFoldList& fold, hipStream_t st);
