// rtm.hip — the RTM (review_transformer) ranking-loss step: ProductRanker of the reference
// (models/ps_model.py:53-370) with the pv (models/PV.py) and pvc (models/PVC.py) review encoders.
//
// Sequences are n = b*J + j (J = 1+K in training: j = 0 positive, j = 1+k negative k; J = C in
// eval), S = R+1 positions: [query, R reviews].  Unlike TEM every sequence is distinct, so the
// encoder (the shared layer loops of encoder.hip) runs on B*J sequences with no replica
// fan-out; only position 0 is consumed (TransformerEncoder.forward, transformer.py:90-98), so the
// last layer is the one-query-row form.  This file: the workspace layout, the backward plan, the entry points and the
// order of a call's stages with every stream decision between them.  The RTM-specific kernels, one family per file (rtm.h):
//   rtm_embed.hip      rtm_embed: review vectors (pv: row gather; pvc: masked mean of <= WL word rows per review with
//                      Philox token corruption, PVC.py:46-61 — the bandwidth-heavy gather of config 4),
//                      dropout, segment embedding, key mask, positional add -> x[B*J, S, d]
//   rtm_score.hip      rtm_score   wo . enc + bias (transformer.py:95-96)
//                      rtm_pv_fwd  PV word-prediction logits (PV.py:59-66 / PVC.py:83-91), gather + dot per task
//                      rtm_loss    weighted BCE over products (ps_model.py:341-356) + PV loss (:277-280), one block
//                      and their backward
//   rtm_embed_bwd.hip  backward of rtm_embed: fp32-atomic scatter-adds into the dense table gradients, slot rows for
//   rtm_index.hip      the inverted word index and the word-gradient reduce over it
#include "rtm.h"
#include "side_stream.h"
#include "wgrad.h"
#include <string.h>

static inline int64_t rtake(int64_t& cur, int64_t n) { int64_t o = cur; cur += (n + 3) & ~(int64_t)3; return o; }

static int rtm_check(const PsRtmDesc& D) {
  PS_REQUIRE(D.B > 0 && D.K >= 0 && D.R > 0 && D.Q > 0 && D.d > 0, "rtm desc: bad sizes");
  PS_REQUIRE(D.d % 32 == 0 && D.d <= 512 && D.d / 4 <= 64 * 2, "rtm desc: embedding_size %d", D.d);
  PS_REQUIRE(D.R + 1 <= 64, "rtm desc: %d reviews per sequence (S <= 64)", D.R);
  PS_REQUIRE(D.review_encoder >= PS_RENC_PV && D.review_encoder <= PS_RENC_AVG, "rtm desc: review encoder %d", D.review_encoder);
  PS_REQUIRE(D.review_encoder == PS_RENC_PV || D.WL > 0, "rtm desc: word-mean review encoders need WL");
  PS_REQUIRE(D.review_encoder == PS_RENC_PV || D.review_encoder == PS_RENC_PVC || !D.train_pv,
             "rtm desc: the fs / avg review encoders have no PV loss (ps_model.py:264: train_pv only applies to pv / pvc)");
  PS_REQUIRE(D.dropout >= 0.f && D.dropout < 1.f && D.corrupt_rate >= 0.f && D.corrupt_rate < 1.f, "rtm desc: rates");
  return PS_OK;
}

static PsTemDesc enc_desc(const PsRtmDesc& D, int J) {
  PsTemDesc E;
  memset(&E, 0, sizeof(E));
  E.B = D.B * J; E.K = 0; E.L = D.R; E.Q = 1; E.W = 0; E.C = 0;
  E.d = D.d; E.H = D.H; E.F = D.F; E.n_layers = D.n_layers;
  E.product_size = 1; E.vocab_size = 2;
  E.model = PS_MODEL_TEM; E.query_encoder = PS_QENC_AVG;
  E.use_pos_emb = D.use_pos_emb; E.training = D.training; E.dropout = D.dropout; E.seed = D.seed; E.step = D.step;
  return E;
}

static int rtm_make_ws(const PsRtmDesc& D, bool eval, RtmWs& r, Ws& w, PsTemDesc& E) {
  TRY(rtm_check(D));
  const int J = eval ? D.C : D.K + 1;
  PS_REQUIRE(J > 0, "rtm: no sequences per row");
  E = enc_desc(D, J);
  if (eval) E.training = 0;
  r.J = J; r.Bseq = D.B * J; r.S = D.R + 1;
  const int d = D.d;
  int64_t cur = 0;
  r.qmean = rtake(cur, (int64_t)D.B * d);
  r.query_emb = rtake(cur, (int64_t)D.B * d);
  r.valid = rtake(cur, (int64_t)r.Bseq * r.S);
  r.vec = rtake(cur, (int64_t)D.B * D.R * d);
  r.cnt = rtake(cur, (int64_t)r.Bseq * D.R);
  r.scores = rtake(cur, r.Bseq);
  r.weight = rtake(cur, r.Bseq);
  const int64_t npv = (int64_t)D.B * D.R * (D.W > 0 ? D.W : 1) * (D.K + 1);
  r.pv_scores = rtake(cur, npv);
  r.pv_terms = rtake(cur, npv);
  r.nvalid = rtake(cur, 4);
  r.seqcnt = rtake(cur, (int64_t)r.Bseq + 4);
  r.loss_blk = rtake(cur, 4);         // [0..1] the loss word, [2] the valid-group count of rtm_grouplist_kernel
  r.glist = eval ? 0 : rtake(cur, (int64_t)ps_cdiv((int64_t)D.B * D.R, 4) + ps_cdiv((int64_t)D.B * D.K * D.R, 4) + 4);
  r.dvec = rtake(cur, (int64_t)D.B * D.R * d);
  r.dqpre = rtake(cur, (int64_t)D.B * d);
  r.dqmean = rtake(cur, (int64_t)D.B * d);
  r.dqe = rtake(cur, (int64_t)D.B * d);          // dqe and wcnt are adjacent: the backward zeroes both with ONE memset
  r.wcnt = r.woff = r.wcur = r.wl = r.wrank = r.hist = 0;
  r.raw = r.yfs = r.dpre = r.dmean = 0;
  if (!eval && D.review_encoder != PS_RENC_PV) {
    r.wcnt = rtake(cur, D.vocab_size + 1);        // [V] occurrence counts + the segment allocator's running total
    r.woff = rtake(cur, D.vocab_size + 1);
    r.wcur = rtake(cur, D.vocab_size);
    r.wl = rtake(cur, 2 * (int64_t)r.Bseq * D.R * D.WL);
    r.wrank = rtake(cur, (int64_t)r.Bseq * D.R * D.WL);
    if (D.vocab_size <= RTM_HIST_MAXV) r.hist = rtake(cur, (int64_t)RTM_HIST_G * D.vocab_size);
  }
  if (!eval && D.review_encoder == PS_RENC_FS) {     // (behind the index arrays: dqe .. wcnt must stay one contiguous memset)
    const int64_t nr = (int64_t)r.Bseq * D.R * d;
    r.raw = rtake(cur, nr); r.yfs = rtake(cur, nr); r.dpre = rtake(cur, nr); r.dmean = rtake(cur, nr);
  }
  r.segpart = eval ? 0 : rtake(cur, (int64_t)ps_cdiv(rtm_eb_waves(D.B, D.K, D.R, nullptr, nullptr), 4) * 3 * d);
  r.enc_base = cur;
  TRY(make_ws(E, w));
  r.total = cur + w.total;
  return PS_OK;
}

extern "C" int ps_rtm_workspace_floats(const PsRtmDesc* desc, int32_t eval, int64_t* total) {
  PS_REQUIRE(desc && total, "rtm workspace: null argument");
  RtmWs r; Ws w; PsTemDesc E;
  TRY(rtm_make_ws(*desc, eval != 0, r, w, E));
  *total = r.total;
  return PS_OK;
}

// offsets (floats) of the intermediates the parity tests compare stage by stage
extern "C" int ps_rtm_workspace_layout(const PsRtmDesc* desc, int32_t eval, PsRtmWsLayout* out) {
  PS_REQUIRE(desc && out, "rtm workspace layout: null argument");
  RtmWs r; Ws w; PsTemDesc E;
  TRY(rtm_make_ws(*desc, eval != 0, r, w, E));
  memset(out, 0, sizeof(*out));
  out->total_floats = r.total; out->Bseq = r.Bseq; out->S = r.S; out->J = r.J;
  out->query_emb = r.query_emb; out->valid = r.valid; out->vec = r.vec; out->cnt = r.cnt; out->scores = r.scores;
  out->weight = r.weight; out->pv_scores = r.pv_scores;
  out->x = r.enc_base + w.x; out->enc = r.enc_base + w.enc; out->dx = r.enc_base + w.dx;
  return PS_OK;
}

// ------------------------------------------------------------------ host side
static void fill_k(const PsRtmDesc& D, const PsRtmTensors& P, const PsRtmBatch& Bt, float* ws, const RtmWs& r, const Ws& w,
                   bool eval, RtmK& k) {
  memset(&k, 0, sizeof(k));
  k.B = D.B; k.J = r.J; k.K = D.K; k.R = D.R; k.S = r.S; k.Q = D.Q; k.W = D.W > 0 ? D.W : 1; k.WL = D.WL; k.d = D.d;
  k.V = D.vocab_size; k.RC = D.review_count;
  k.det = ps_deterministic() ? 1 : 0;
  static const bool rtm_stamps = ps_diag_int("PS_RTM_STAMP", 0) != 0;
  k.stamp = rtm_stamps ? ps_debug_stamp_ptr() : nullptr;
  // `pvc` = every word-mean review encoder in training (pvc, fs, avg); only pvc corrupts tokens and ignores the word masks
  k.pvc = D.review_encoder != PS_RENC_PV && !eval; k.use_pos = D.use_pos_emb; k.use_seg = D.use_seg_emb;
  const bool masked_mean = !eval && (D.review_encoder == PS_RENC_FS || D.review_encoder == PS_RENC_AVG);
  if (masked_mean) { k.wmask_pos = Bt.pos_prod_rword_masks; k.wmask_neg = Bt.neg_prod_rword_masks; }
  if (!eval && D.review_encoder == PS_RENC_FS) { k.raw = ws + r.raw; k.yfs = ws + r.yfs; }
  k.pos_weight = D.pos_weight; k.train_pv = eval ? 0 : D.train_pv; k.training = eval ? 0 : D.training; k.eval = eval;
  k.fJ = make_fdiv(r.J); k.fS = make_fdiv(r.S); k.fK1 = make_fdiv(D.K + 1);
  PsTemDesc dd;
  memset(&dd, 0, sizeof(dd));
  dd.training = k.training; dd.dropout = D.dropout; dd.seed = D.seed; dd.step = D.step;
  k.d_pv = make_drop(dd, SITE_REV_PV); k.d_pos = make_drop(dd, SITE_REV_POS); k.d_neg = make_drop(dd, SITE_REV_NEG);
  if (D.no_pv_drop) {      // fix_emb: PV.forward's drop_layer has p = 0 (PV.py:36-39) — the site is the identity, forward and backward
    dd.dropout = 0.f;
    k.d_pv = make_drop(dd, SITE_REV_PV);
  }
  dd.dropout = D.review_encoder == PS_RENC_PVC ? D.corrupt_rate : 0.f;
  k.t_pos = make_drop(dd, SITE_TOK_POS); k.t_neg = make_drop(dd, SITE_TOK_NEG);
  k.U = D.user_size; k.PI = D.product_size;
  if (D.use_user_emb) { k.user_emb = P.user_emb; k.pos_u = Bt.pos_user_idxs; k.neg_u = eval ? Bt.candi_seq_user_idxs : Bt.neg_user_idxs; }
  if (D.use_item_emb) { k.item_emb = P.product_emb; k.pos_i = Bt.pos_item_idxs; k.neg_i = eval ? Bt.candi_seq_item_idxs : Bt.neg_item_idxs; }
  if (eval) {
    k.neg_r = Bt.candi_prod_ridxs; k.neg_seg = Bt.candi_seg_idxs; k.table = Bt.review_embeddings;
  } else {
    k.pos_r = Bt.pos_prod_ridxs; k.neg_r = Bt.neg_prod_ridxs; k.pos_seg = Bt.pos_seg_idxs; k.neg_seg = Bt.neg_seg_idxs;
    k.pos_words = Bt.pos_prod_rword_idxs; k.neg_words_rev = Bt.neg_prod_rword_idxs;
    k.pos_pvc = Bt.pos_prod_rword_idxs_pvc; k.neg_pvc = Bt.neg_prod_rword_idxs_pvc;
    k.neg_word_idxs = Bt.neg_word_idxs; k.pos_masks = Bt.pos_prod_rword_masks;
    k.table = P.review_emb;
  }
  k.word_emb = P.word_emb; k.seg_emb = P.seg_emb; k.pe = P.pe; k.wo_w = P.wo_w; k.wo_b = P.wo_b;
  float* we = ws + r.enc_base;
  k.vrows = reinterpret_cast<int32_t*>(we + w.vrows); k.vcount = reinterpret_cast<int32_t*>(we + w.vcount);
  k.query_emb = ws + r.query_emb; k.x = we + w.x; k.valid = ws + r.valid; k.vec = ws + r.vec; k.cnt = ws + r.cnt;
  k.enc = we + w.enc; k.scores = ws + r.scores; k.weight = ws + r.weight; k.pv_scores = ws + r.pv_scores; k.pv_terms = ws + r.pv_terms;
  k.nvalid = ws + r.nvalid;
  k.seqcnt = reinterpret_cast<int32_t*>(ws + r.seqcnt);
  k.dx = we + w.dx; k.denc = we + w.denc; k.dvec = ws + r.dvec; k.dqe = ws + r.dqe;
  if (r.wcnt) {
    k.wcnt = (int*)(ws + r.wcnt); k.woff = (int*)(ws + r.woff); k.wcur = (int*)(ws + r.wcur);
    k.wl = (int2*)(ws + r.wl); k.wrank = (int*)(ws + r.wrank);
    k.hist = r.hist ? (int*)(ws + r.hist) : nullptr;
    k.hist_rows = ps_cdiv((int64_t)r.Bseq * D.R, RTM_HIST_G);
  }
}
// the query encoder's FS dropout site: the forward and the backward draw the same words
static DropSpec rtm_query_drop(const PsRtmDesc& D, const RtmK& k) {
  PsTemDesc dq;
  memset(&dq, 0, sizeof(dq));
  dq.training = k.training; dq.dropout = D.dropout; dq.seed = D.seed; dq.step = D.step;
  return make_drop(dq, PS_SITE_FS);
}

// The inverted index word -> review slots of the pvc / fs / avg backward depends on the batch's indices only.  Its first
// pass (per-word counts, and with them every occurrence's rank inside its word) rides in the training forward when that
// embeds through rtm_embed4_kernel, which holds every word id in registers; the backward then only allocates and fills,
// on the side stream under its first kernels.
static bool rtm_counts_in_forward(const PsRtmDesc& D, const RtmWs& r) {
  static const bool late = ps_diag_int("PS_RTM_LATE_INDEX", 0) != 0;
  return !late && !rtm_hist_index(D, r) && rtm_embed4_taken(D, false, r);
}

// What one training backward runs, decided ONCE from the descriptor (its frozen mask included), the workspace layout and the
// process's switches — like EncPlan for the layer loops (encoder.h).  rtm_backward_impl reads this and nothing else; the
// training forward reads `index` (does its gather count word ranks?); ps_rtm_backward_plan hands it out (host only).
//   review side = what sits behind a review vector: the word table for the word-mean encoders (pvc / fs / avg), the review
//   table for pv.  When it is frozen nothing behind x's review slots takes a gradient (fs: f_W does, straight from d x).
static PsRtmBwdPlan rtm_bwd_plan(const PsRtmDesc& D, const RtmWs& r, bool det) {
  PsRtmBwdPlan p;
  memset(&p, 0, sizeof(p));
  const bool wordmean = D.review_encoder != PS_RENC_PV;
  const bool words = !(D.frozen_mask & PS_RTM_FROZEN_WORD);
  const bool reviews = !wordmean && !(D.frozen_mask & PS_RTM_FROZEN_REVIEW);
  const bool side = wordmean ? words : reviews;
  p.index = !(wordmean && words) ? PS_RTM_INDEX_NONE
            : rtm_hist_index(D, r) ? PS_RTM_INDEX_HIST : (rtm_counts_in_forward(D, r) ? PS_RTM_INDEX_FWD_COUNTS : PS_RTM_INDEX_LATE);
  p.word_reduce = wordmean && words;
  p.slot_rows = p.word_reduce || (det && reviews);
  p.review_scatter = reviews;
  if (D.train_pv) {        // (pv / pvc only: rtm_check)
    p.pv_bwd = (side ? PS_RTM_PV_DVEC : 0) | (words ? PS_RTM_PV_WORDS : 0);
    p.pv_bwd_kernel = side || (words && !det);       // det: the word rows go through rtm_pv_keys_kernel + the sole-owner scatter
  }
  p.fs_draw = D.review_encoder == PS_RENC_FS && words;
  p.query_scatter = words;
  p.user_scatter = D.use_user_emb && !(D.frozen_mask & PS_RTM_FROZEN_USER);
  p.item_scatter = D.use_item_emb && !(D.frozen_mask & PS_RTM_FROZEN_ITEM);
  p.embed_form = !side ? PS_RTM_EB_FROZEN
                 : (wordmean && D.review_encoder != PS_RENC_FS && !p.user_scatter && !p.item_scatter && !D.train_pv) ? PS_RTM_EB_PLAIN
                                                                                                                   : PS_RTM_EB_GENERAL;
  // frozen form: a review-slot wave feeds the segment partials and (by atomics; deterministic mode scatters them beforehand) the
  // user / item rows — with none of them there is nothing for it to do
  p.slot_waves = p.embed_form != PS_RTM_EB_FROZEN || D.use_seg_emb || (!det && (p.user_scatter || p.item_scatter));
  p.side_fork = p.index == PS_RTM_INDEX_HIST || p.index == PS_RTM_INDEX_FWD_COUNTS;
  return p;
}
extern "C" int ps_rtm_backward_plan(const PsRtmDesc* desc, PsRtmBwdPlan* out) {
  PS_REQUIRE(desc && out, "rtm backward plan: null argument");
  RtmWs r; Ws w; PsTemDesc E;
  TRY(rtm_make_ws(*desc, false, r, w, E));
  *out = rtm_bwd_plan(*desc, r, ps_deterministic());
  return PS_OK;
}

static void to_tem_tensors(const PsRtmTensors& R, PsTemTensors& T) {
  memset(&T, 0, sizeof(T));
  T.word_emb = R.word_emb; T.fs_w = R.fs_w; T.fs_b = R.fs_b; T.pe = R.pe;
  T.final_ln_g = R.final_ln_g; T.final_ln_b = R.final_ln_b;
  for (int i = 0; i < PS_MAX_LAYERS; ++i) T.layer[i] = R.layer[i];
}

// the row list costs Bseq^2 / 2 count reads (rtm_rowlist_kernel): built up to 8k sequences, dense products beyond
static bool rtm_rows_listed(const RtmWs& r, const Ws& w) { return r.S <= 64 && w.vrows != 0 && r.Bseq <= 8192; }

static int rtm_encode(const PsRtmDesc& D, const PsRtmTensors& P, const PsRtmBatch& Bt, float* ws, const RtmWs& r,
                      const Ws& w, const PsTemDesc& E, bool eval, RtmK& k, hipStream_t st) {
  const int B = D.B, d = D.d;
  PS_REQUIRE(P.word_emb && P.seg_emb && P.wo_w && P.wo_b && Bt.query_word_idxs, "rtm: null tensors");
  fill_k(D, P, Bt, ws, r, w, eval, k);
  PS_REQUIRE(k.neg_r && k.neg_seg && (eval || (k.pos_r && k.pos_seg)), "rtm: null review index tensors");
  PS_REQUIRE(k.pvc || k.table, "rtm: null review embedding table");
  PS_REQUIRE(!D.use_user_emb || (k.user_emb && k.neg_u && (eval || k.pos_u)), "rtm: use_user_emb needs user_emb and the user index tensors");
  PS_REQUIRE(!D.use_item_emb || (k.item_emb && k.neg_i && (eval || k.pos_i)), "rtm: use_item_emb needs product_emb and the item index tensors");
  if (k.pvc) PS_REQUIRE(k.train_pv ? (k.pos_pvc && k.neg_pvc) : (k.pos_words && k.neg_words_rev), "rtm: null review word tensors");
  if (!eval && (D.review_encoder == PS_RENC_FS || D.review_encoder == PS_RENC_AVG))
    PS_REQUIRE(k.wmask_pos && k.wmask_neg, "rtm: the fs / avg review encoders need the batch's word masks");
  if (k.train_pv) PS_REQUIRE(k.pos_words && k.pos_masks && k.neg_word_idxs, "rtm: null PV-loss tensors");
  // query encoder (shared kernels): masked mean (+FS dropout) then tanh(f_W . + b)
  EmbedArgs e;
  memset(&e, 0, sizeof(e));
  e.B = B; e.Q = D.Q; e.L = 0; e.S = 1; e.d = d; e.P = 1; e.V = D.vocab_size; e.tem = 0;
  e.fs = D.query_encoder == PS_QENC_FS; e.qw = Bt.query_word_idxs; e.word_emb = P.word_emb;
  e.drop_fs = rtm_query_drop(D, k);
  e.qmean_d = ws + r.qmean; e.query_emb = ws + r.query_emb;
  PS_REQUIRE(!e.fs || (P.fs_w && P.fs_b), "rtm: null FS encoder weights");
  const bool fs_fused = e.fs && ps_fusion_enabled() && d <= 128;
  if (fs_fused) { e.fs_w = P.fs_w; e.fs_b = P.fs_b; }
  PsTemTensors T;
  to_tem_tensors(P, T);
  const EncCall c = enc_call({E, T, ws + r.enc_base, w, st}, nullptr, ws + r.valid, rtm_rows_listed(r, w));
  e.split = c.x3;                                       // the fused kernels' bf16x3 weight planes ride in this launch
  // the backward's inverted index (rtm_counts_in_forward): its counters are cleared by this launch, filled by the next
  k.count_fwd = !eval && rtm_bwd_plan(D, r, k.det != 0).index == PS_RTM_INDEX_FWD_COUNTS;      // (none with a frozen word table)
  if (k.count_fwd) { e.zero_i32 = k.wcnt; e.zero_n = (int)D.vocab_size + 1; }
  if (!eval) e.clear_word = reinterpret_cast<uint32_t*>(ws + r.loss_blk);   // rtm_score_kernel's 64-bit loss word
  TRY(launch_embed_fwd(e, st));
  if (e.fs && !fs_fused) {
    GemmProblem p = gp(ws + r.qmean, d, 0, P.fs_w, d, 0, ws + r.query_emb, d, B, d, d);
    p.bias = P.fs_b; p.act = ACT_TANH;
    TRY(run1(p, st));
  }
  PS_REQUIRE(!D.use_pos_emb || P.pe, "rtm: null positional table");
  TRY(rtm_embed_fwd(D, k, ws, r, eval, c.plan.rowlist, st));
  if (k.raw) {   // fs review encoder: y = tanh(f_W . raw + b) for every review slot, then the rest of x
    PS_REQUIRE(P.rev_fs_w && P.rev_fs_b, "rtm: null review-encoder f_W");
    GemmProblem p = gp(ws + r.raw, d, 0, P.rev_fs_w, d, 0, ws + r.yfs, d, r.Bseq * D.R, d, d);
    p.bias = P.rev_fs_b; p.act = ACT_TANH;
    TRY(run1(p, st));
    TRY(rtm_fs_finish(k, r, st));
  }
  if (c.rows_listed) TRY(rtm_rowlist(k, r, st));
  return enc_layers_forward(c, EncFwdOpts());
}

extern "C" int ps_rtm_forward(const PsRtmDesc* desc, const PsRtmTensors* params, const PsRtmBatch* batch, float* ws,
                              float* loss3, ps_stream_t stream) {
  PS_REQUIRE(desc && params && batch && ws && loss3, "rtm forward: null argument");
  RtmWs r; Ws w; PsTemDesc E; RtmK k;
  TRY(rtm_make_ws(*desc, false, r, w, E));
  hipStream_t st = (hipStream_t)stream;
  TRY(rtm_encode(*desc, *params, *batch, ws, r, w, E, false, k, st));
  k.loss3 = loss3;
  return rtm_head_fwd(k, r, ws, st);
}

extern "C" int ps_rtm_score(const PsRtmDesc* desc, const PsRtmTensors* params, const PsRtmBatch* batch, float* ws,
                            float* scores, ps_stream_t stream) {
  PS_REQUIRE(desc && params && batch && ws && scores, "rtm score: null argument");
  PS_REQUIRE(desc->C > 0 && batch->candi_prod_ridxs && batch->candi_seg_idxs && batch->review_embeddings,
             "rtm score: needs candidates and the review-embedding table");
  RtmWs r; Ws w; PsTemDesc E; RtmK k;
  TRY(rtm_make_ws(*desc, true, r, w, E));
  hipStream_t st = (hipStream_t)stream;
  TRY(rtm_encode(*desc, *params, *batch, ws, r, w, E, true, k, st));
  return rtm_score_eval(k, r, scores, st);
}

extern "C" int ps_rtm_review_embeddings(const PsRtmDesc* desc, const PsRtmTensors* params, const int64_t* review_words,
                                        float* scratch, float* out, ps_stream_t stream) {
  PS_REQUIRE(desc && params && review_words && out && params->word_emb && desc->WL > 0, "rtm review table: bad argument");
  const bool fs = desc->review_encoder == PS_RENC_FS;
  PS_REQUIRE(!fs || (scratch && params->rev_fs_w && params->rev_fs_b), "rtm review table: fs needs scratch and f_W");
  hipStream_t st = (hipStream_t)stream;
  TRY(rtm_review_table(*desc, params->word_emb, review_words, fs ? scratch : out, st));
  if (fs) {
    const int d = desc->d;
    // The reference fills the table in slices of 128 reviews up to row ceil((RC-1)/128)*128 (ps_model.py:190-203): unless
    // RC-1 is a multiple of 128 that takes in the padding review, whose empty mean is projected like any other —
    // its row is tanh(bias), not 0 (its positions are masked in every sequence, so only the table itself shows it)
    const int64_t rc = desc->review_count;
    const bool pad_projected = (rc - 1) % 128 != 0;
    const int64_t n = pad_projected ? rc : rc - 1;
    PS_REQUIRE(n < ((int64_t)1 << 31), "rtm review table: too many reviews");
    if (n > 0) {
      GemmProblem p = gp(scratch, d, 0, params->rev_fs_w, d, 0, out, d, (int)n, d, d);
      p.bias = params->rev_fs_b; p.act = ACT_TANH;
      TRY(run1(p, st));
    }
    if (!pad_projected) PS_CHECK_HIP(hipMemsetAsync(out + (size_t)n * d, 0, sizeof(float) * d, st));
  }
  return PS_OK;
}

static int rtm_backward_impl(const PsRtmDesc* desc, const PsRtmTensors* params, const PsRtmBatch* batch, float* ws,
                             const PsRtmTensors* grads, float loss_scale, const float* loss_scale_dev, ps_stream_t stream,
                             EncBwdOut& out) {
  PS_REQUIRE(desc && params && batch && ws && grads, "rtm backward: null argument");
  const PsRtmDesc& D = *desc;
  RtmWs r; Ws w; PsTemDesc E; RtmK k;
  TRY(rtm_make_ws(D, false, r, w, E));
  hipStream_t st = (hipStream_t)stream;
  fill_k(D, *params, *batch, ws, r, w, false, k);
  const PsRtmTensors& G = *grads;
  const PsRtmBwdPlan pl = rtm_bwd_plan(D, r, k.det != 0);
  PS_REQUIRE((!D.use_seg_emb || G.seg_emb) && G.wo_w && G.wo_b, "rtm backward: null gradients");
  // a NULL table gradient means frozen, and the descriptor says the same (the forward and the plan only see the descriptor)
  PS_REQUIRE((G.word_emb == nullptr) == ((D.frozen_mask & PS_RTM_FROZEN_WORD) != 0),
             "rtm backward: the word_emb gradient is %s but frozen_mask = %d", G.word_emb ? "given" : "NULL", D.frozen_mask);
  PS_REQUIRE(k.pvc || (G.review_emb == nullptr) == ((D.frozen_mask & PS_RTM_FROZEN_REVIEW) != 0),
             "rtm backward: the review_emb gradient is %s but frozen_mask = %d", G.review_emb ? "given" : "NULL", D.frozen_mask);
  PS_REQUIRE(!D.use_user_emb || (G.user_emb == nullptr) == ((D.frozen_mask & PS_RTM_FROZEN_USER) != 0),
             "rtm backward: the user_emb gradient is %s but frozen_mask = %d", G.user_emb ? "given" : "NULL", D.frozen_mask);
  PS_REQUIRE(!D.use_item_emb || (G.product_emb == nullptr) == ((D.frozen_mask & PS_RTM_FROZEN_ITEM) != 0),
             "rtm backward: the product_emb gradient is %s but frozen_mask = %d", G.product_emb ? "given" : "NULL", D.frozen_mask);
  k.scale = loss_scale; k.scale_dev = loss_scale_dev;
  k.g_word_emb = G.word_emb; k.g_table = G.review_emb; k.g_seg_emb = G.seg_emb; k.g_wo_w = G.wo_w; k.g_wo_b = G.wo_b;
  if (pl.user_scatter) k.g_user_emb = G.user_emb;
  if (pl.item_scatter) k.g_item_emb = G.product_emb;
  k.count_fwd = pl.index == PS_RTM_INDEX_FWD_COUNTS;
  const int B = D.B, d = D.d, V = (int)D.vocab_size;
  const bool fwd_index = pl.side_fork != 0;     // HIST or FWD_COUNTS — either way: built on the side stream, right here
  // Deterministic mode covers every review encoder (pvc — BASELINE configs[3] —, fs, avg: the word index + ordered reduce; pv:
  // the review rows through the sole-owner row scatter), the user / item embedding rows and the PV loss's word rows.
  // (A frozen word table has no index: any vocabulary size.)
  PS_REQUIRE(!k.det || !pl.word_reduce || pl.index == PS_RTM_INDEX_HIST,
             "rtm backward: deterministic mode needs the LDS-histogram word index (vocabulary <= %d, PS_RTM_HIST != 0)", RTM_HIST_MAXV);

  // ---- the word index: [count +] allocate + fill on the side stream (or here, without one), under the fused kernel and the attention
  if (fwd_index) {
    hipStream_t ss = side_stream_or(st);
    if (ss != st) { side_set_light(false); TRY(side_fork(st)); }
    if (pl.index == PS_RTM_INDEX_HIST) TRY(rtm_build_index_hist(k, V, ss));
    else TRY(rtm_build_index(k, r, V, false, ss));
  }
  // ---- the head; its first launch carries the index's fork
  uint32_t* sig = nullptr; uint32_t sigval = 0;
  static const bool sbwd_carries = ps_diag_int("PS_RTM_SBWD_SIG", 1) != 0;
  if (sbwd_carries) side_take_signal(st, &sig, &sigval);
  TRY(rtm_head_bwd(k, r, pl, sig, sigval, st));
  // ---- the encoder layers
  PsTemTensors T, TG;
  to_tem_tensors(*params, T);
  to_tem_tensors(G, TG);
  ColFoldList fold;
  fold.n = 0;
  // d query_emb (+, when the index is built here, the per-word counters right behind it, rtm_make_ws): one memset
  if (pl.index == PS_RTM_INDEX_LATE) {
    const int64_t zend = r.wcnt + (((int64_t)D.vocab_size + 1 + 3) & ~(int64_t)3);
    PS_CHECK_HIP(hipMemsetAsync(ws + r.dqe, 0, sizeof(float) * (size_t)(zend - r.dqe), st));
  }
  if (pl.slot_rows) k.gs = ws + r.enc_base + w.dx;     // (det + pv encoder: the review rows' gradients are parked in place, scattered by the embed backward)
  EncBwdIn in;
  in.fold = &fold;
  TRY(enc_layers_backward(enc_call({E, T, ws + r.enc_base, w, st}, nullptr, ws + r.valid, rtm_rows_listed(r, w)), TG, in, out));
  PS_REQUIRE(!out.dx_two_partials, "rtm backward: the encoder left d x as two partials, which nothing here adds");
  // ---- fs: through the review projection: d pre = dx * tanh', bias gradient, weight gradient, d raw = d pre . f_W
  if (D.review_encoder == PS_RENC_FS) {
    PS_REQUIRE(G.rev_fs_w && G.rev_fs_b && params->rev_fs_w, "rtm backward: null review-encoder f_W gradient");
    const int NR = r.Bseq * D.R;
    TRY(rtm_fs_bwd(k, r, ws + r.dpre, G.rev_fs_b, st));
    GemmProblem wg[1] = {gp_wgrad(ws + r.dpre, d, ws + r.raw, d, G.rev_fs_w, d, d, NR)};
    TRY(side_wgrads(wg, 1, st));
    if (pl.fs_draw) {                              // (frozen words: d raw has no consumer)
      GemmProblem px = gp(ws + r.dpre, d, 0, params->rev_fs_w, d, 1, ws + r.dmean, d, NR, d, d);
      TRY(run1(px, st));
      k.dmean = ws + r.dmean;
    }
  }
  // ---- the input assembly
  TRY(rtm_embed_bwd(D, k, r, pl, ws, fold, st));
  // ---- the word rows
  if (pl.word_reduce) {
    if (pl.index == PS_RTM_INDEX_LATE) TRY(rtm_build_index(k, r, V, true, st));
    // The word-gradient reduce needs the index (side stream, in order there) and the slot gradients the kernel above left
    // (main stream): with forks free it runs ON the side stream behind a fork — carried by the query scatter below — beside
    // that scatter, and the join that used to precede it (5 us on the main stream with nothing to wait for) is gone.
    // PS_RTM_WR_SIDE=0: joined and launched on the main stream.
    static const bool wr_side_on = ps_diag_int("PS_RTM_WR_SIDE", 1) != 0;
    hipStream_t wst = st;
    if (fwd_index) {
      hipStream_t ss = side_stream_or(st);
      if (wr_side_on && ss != st) { TRY(side_fork(st)); wst = ss; }
      else TRY(side_join(st));                      // the index (and the weight gradients queued behind it) are through
    }
    TRY(rtm_word_reduce(D, k, r, wst));
  }
  // ---- query encoder backward (shared kernels) + scatter to the query word rows
  EmbedBwdArgs e;
  memset(&e, 0, sizeof(e));
  e.B = B; e.Q = D.Q; e.L = 0; e.S = 1; e.d = d; e.P = 1; e.V = D.vocab_size; e.tem = 0;
  e.qw = batch->query_word_idxs; e.drop_fs = rtm_query_drop(D, k); e.g_word_emb = G.word_emb;
  if (D.query_encoder == PS_QENC_FS) {
    PS_REQUIRE(G.fs_w && G.fs_b, "rtm backward: null FS gradients");
    if (ps_fusion_enabled() && d <= 128) {   // whole FS backward inside the scatter launch (EmbedBwdArgs::fsb_*)
      e.fw_x = ws + r.qmean; e.g_fs_w = G.fs_w;
      e.fsb_dqe = ws + r.dqe; e.fsb_lddqe = d; e.fsb_qe = ws + r.query_emb; e.fsb_w = params->fs_w; e.g_fs_b = G.fs_b;
      e.det_dm = ws + r.dqmean;                   // (deterministic mode only: launch_embed_scatter)
    } else {
      TRY(launch_tanh_bwd(ws + r.dqe, d, ws + r.query_emb, ws + r.dqpre, G.fs_b, B, d, st));
      if (pl.query_scatter) {                       // (frozen words: d mean has no consumer)
        GemmProblem p = gp(ws + r.dqpre, d, 0, params->fs_w, d, 1, ws + r.dqmean, d, B, d, d);
        TRY(run1(p, st));
      }
      GemmProblem wg[1] = {gp_wgrad(ws + r.dqpre, d, ws + r.qmean, d, G.fs_w, d, d, B)};
      TRY(side_wgrads(wg, 1, st));
      e.dqmean_d = ws + r.dqmean;
    }
  } else {
    e.dqmean_d = ws + r.dqe;
  }
  e.fold = fold;
  TRY(launch_embed_scatter(e, st));
  TRY(side_join(st));
  return PS_OK;
}

extern "C" int ps_rtm_backward(const PsRtmDesc* desc, const PsRtmTensors* params, const PsRtmBatch* batch, float* ws,
                               const PsRtmTensors* grads, float loss_scale, const float* loss_scale_dev,
                               ps_stream_t stream) {
  EncBwdOut out;
  const int rc = rtm_backward_impl(desc, params, batch, ws, grads, loss_scale, loss_scale_dev, stream, out);
  enc_record_backward(out);
  if (rc != PS_OK) side_abort();    // never leave the side stream waiting behind a failed call (side_stream.h)
  return rc;
}
