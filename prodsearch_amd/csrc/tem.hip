// tem.hip — host orchestration + C ABI of the TEM / QEM ranking-loss step (gfx950).
//
// Forward  = ItemTransformerRanker.forward_dotproduct (item_transformer.py:440-520)
//            / forward_attn with model_name == 'QEM' (:361-438)
// Backward = autograd of the same (trainer.py:77)
// Score    = test_dotproduct (:111-146) / test_attn QEM (:148-195)
//
// The transformer encoder it drives (workspace layout, plan, layer loops) is encoder.hip; this file embeds, scores, stages and
// replays the step around it.
#include "encoder.h"
#include "graph.h"
#include "side_stream.h"
#include "wgrad.h"
#include <string.h>
#include <math.h>
#include <vector>

// -------------------------------------------------------------- encoder forward
struct SamplerArgs { const float* prob; const int32_t* alias; int64_t* items; int64_t* words; };

// The valid-row list is built by one workgroup per sequence that counts the valid positions of ALL earlier sequences
// (B^2 L / 2 index reads in total): fine up to a few thousand sequences, dense products beyond
static bool rows_list_ok(const PsTemDesc& D) { return D.L <= 64 && (int64_t)D.B * D.B * D.L <= ((int64_t)64 << 20); }

// ---- one call object per entry point: the descriptor as the entry's mode reads it, the workspace layout, the stream, whether the
// valid-row list is built; `rc`: make_ws's answer (bad descriptor), to be checked right behind the constructor.  base / enc: the
// encoder's views of the call (encoder.h), made where the entry has the tensors and the workspace.
enum TemMode {
  TEM_TRAIN,                // a training-mode forward / backward: no candidates (C = 0)
  TEM_EVAL,                 // ps_tem_score / ps_tem_encode: C candidates, no dropout drawn
  TEM_DESCRIBED             // as the descriptor says (ps_tem_plan): C > 0 describes an eval call, C == 0 a training-mode one
};
struct TemCall {
  PsTemDesc D; Ws w; hipStream_t st; bool listed; int rc;
  TemCall(const PsTemDesc* desc, TemMode mode, ps_stream_t stream) : D(*desc), st((hipStream_t)stream) {
    if (mode == TEM_TRAIN) D.C = 0;
    if (mode == TEM_EVAL || (mode == TEM_DESCRIBED && D.C > 0)) D.training = 0;
    rc = make_ws(D, w);
    listed = rows_list_ok(D);
  }
  TemCall(const TemCall&) = delete;             // (the views below point into it)
  EncBase base(const PsTemTensors& P, float* ws) const { return {D, P, ws, w, st}; }
  EncCall enc(const PsTemTensors& P, float* ws, const int64_t* ui, hipStream_t on) const { return enc_call({D, P, ws, w, on}, ui, nullptr, listed); }
};

static int encode_forward(const EncCall& c, const PsTemBatch& Bt, const SamplerArgs* samp = nullptr, const ScoreArgs* fold_sc = nullptr) {
  const PsTemDesc& D = c.D; const PsTemTensors& P = c.P; float* ws = c.ws; const Ws& w = c.w; hipStream_t st = c.st;
  const bool tem = D.model == PS_MODEL_TEM;
  const int B = D.B, d = D.d, S = w.S;
  const float* hist = D.sep_prod_emb ? P.hist_product_emb : P.product_emb;
  enc_taken_clear(0, 0);                        // (QEM / AEM / ZAM: no encoder layers; enc_layers_forward fills it otherwise)
  PS_REQUIRE(P.word_emb && P.product_emb && hist, "forward: null embedding table");
  EmbedArgs e;
  memset(&e, 0, sizeof(e));
  e.B = B; e.Q = D.Q; e.L = D.L; e.S = S; e.d = d; e.P = D.product_size; e.V = D.vocab_size;
  e.tem = tem; e.fs = D.query_encoder == PS_QENC_FS; e.use_pos = D.use_pos_emb;
  e.qw = Bt.query_word_idxs; e.ui = Bt.u_item_idxs;
  e.word_emb = P.word_emb; e.hist_tab = hist; e.pe = P.pe;
  e.drop_fs = make_drop(D, PS_SITE_FS);
  e.qmean_d = ws + w.qmean; e.query_emb = ws + w.query_emb; e.x = ws + w.x;
  PS_REQUIRE(e.qw && ((!tem && !ps_model_attn(D.model)) || e.ui), "forward: null batch indices");
  PS_REQUIRE(!tem || !D.use_pos_emb || P.pe, "forward: null positional table");
  if (tem && c.rows_listed) { e.vrows = reinterpret_cast<int32_t*>(ws + w.vrows); e.vcount = reinterpret_cast<int32_t*>(ws + w.vcount); }
  const float* wp_w[PS_WPLANES_MAX]; int wp_r[PS_WPLANES_MAX], wp_c[PS_WPLANES_MAX];
  const int wp_n = wplane_list(D, P, w, wp_w, wp_r, wp_c);
  WPlaneScope wplanes(st, wp_w, wp_r, wp_c, wp_n);             // the big linears multiply against pre-split weight planes (gemm_kernels.hip)
  if (samp) {
    e.samp_prob = samp->prob; e.samp_alias = samp->alias; e.samp_items = samp->items; e.samp_words = samp->words;
    e.samp_nitem = D.B * D.K; e.samp_nword = D.B * D.W * D.K; e.samp_step = (uint32_t)D.step;
    e.samp_k0 = (uint32_t)(D.seed & 0xffffffffu); e.samp_k1 = (uint32_t)(D.seed >> 32);
  }
  PS_REQUIRE(!e.fs || (P.fs_w && P.fs_b), "forward: null FS encoder weights");
  // FS projection as a per-row mat-vec inside the embed launch — while the [d,d] weight a workgroup streams from L2 is
  // small (64 KB at d = 128; at d = 256 the C5 step lost 60 us to it and the GEMM launch is the better deal)
  const bool fs_fused = e.fs && ps_fusion_enabled() && d <= 128;
  if (fs_fused) { e.fs_w = P.fs_w; e.fs_b = P.fs_b; }
  if (fold_sc) { e.fold_words = 1; e.sc = *fold_sc; }
  e.split = c.x3;
  EncFwdOpts o;
  o.fold_sc = fold_sc;
  if (tem && c.plan.front_fused) {               // one launch embeds, projects and attends: layer 0's (enc_layers_forward)
    PS_REQUIRE(fs_fused && e.vrows, "forward: the fused front end needs the FS projection and the row list");
    o.front = &e;
    return enc_layers_forward(c, o);
  }
  // the fused projection + attention launch re-splits the backward's streams
  o.split_bwd_left = e.split.on && D.training && c.plan.attn[0] == ATTN_KVQ;
  e.split_fwd_only = o.split_bwd_left ? 1 : 0;
  TRY(launch_embed_fwd(e, st));
  if (e.fs && !fs_fused) {   // FSEncoder: tanh(f_W . mean + b)  (text_encoder.py:39); also writes row 0 of x (+pe[0])
    GemmProblem p = gp(ws + w.qmean, d, 0, P.fs_w, d, 0, ws + w.query_emb, d, B, d, d);
    p.bias = P.fs_b; p.act = ACT_TANH;
    if (tem) { p.out2 = ws + w.x; p.ld2 = S * d; p.add2 = D.use_pos_emb ? P.pe : nullptr; }
    TRY(run1(p, st));
  }
  if (ps_model_attn(D.model)) return ae_forward(c);
  if (!tem) return PS_OK;
  return enc_layers_forward(c, o);
}

static void fold_finish(const EncBase& c, ScoreArgs& s, const SamplerArgs* samp) {
  const PsTemDesc& D = c.D; float* ws = c.ws; const Ws& w = c.w;
  s.word_blk = ws + w.word_blk; s.item_blk = ws + w.item_blk; s.ticket = reinterpret_cast<uint32_t*>(ws + w.ticket);
  s.word_nblk = ps_cdiv((int64_t)D.B * D.W * (D.K + 1), PS_WORD_TASKS_PER_WG);
  if (samp) {
    s.samp_inline = 1; s.samp_prob = samp->prob; s.samp_alias = samp->alias;
    s.samp_step = (uint32_t)D.step; s.samp_k0 = (uint32_t)(D.seed & 0xffffffffu); s.samp_k1 = (uint32_t)(D.seed >> 32);
  }
}

static void fill_score(const EncBase& c, const PsTemBatch& Bt, ScoreArgs& s) {
  const PsTemDesc& D = c.D; const PsTemTensors& P = c.P; float* ws = c.ws; const Ws& w = c.w;
  memset(&s, 0, sizeof(s));
  s.B = D.B; s.K = D.K; s.W = D.W; s.C = 0; s.R = w.R; s.d = D.d;
  s.P = D.product_size; s.V = D.vocab_size;
  s.bias_product = D.bias_product; s.pos_weight = D.pos_weight;
  s.target = Bt.target_prod_idxs; s.neg_items = Bt.neg_item_idxs; s.pos_words = Bt.pos_iword_idxs;
  s.neg_words = Bt.neg_word_idxs; s.candi = Bt.candi_prod_idxs;
  s.product_emb = P.product_emb; s.word_emb = P.word_emb; s.product_bias = P.product_bias; s.word_bias = P.word_bias;
  s.enc = ws + w.enc;
  s.item_scores = ws + w.item_scores; s.word_scores = ws + w.word_scores; s.loss_parts = ws + w.loss_parts;
  s.item_terms = ws + w.item_terms; s.word_terms = ws + w.word_terms; s.loss_blk = ws + w.loss_blk;
  score_finish(s);
}

// The training forward of ps_tem_forward, ps_tem_forward_sampled and ps_tem_forward_step: [the staging prologue,] embed + encode,
// score, loss.  Folded scoring (EncPlan::fold_score: no gather+score / loss launches, see ScoreArgs, folded form) where the caller
// allows it and the stream is not capturing: graph replay patches the loss kernel's arguments (unfolded form).
static int tem_forward(const EncCall& c, const PsTemBatch& Bt, const SamplerArgs* samp, float* loss3, float* loss_acc, bool may_fold,
                       const StageArgs* stage) {
  if (stage) TRY(launch_stage(*stage, c.st));
  ScoreArgs s;
  fill_score(c, Bt, s);
  s.loss3 = loss3; s.loss_acc = loss_acc;
  if (may_fold && c.plan.fold_score && !stream_capturing(c.st)) {
    fold_finish(c, s, samp);
    return encode_forward(c, Bt, samp, &s);
  }
  TRY(encode_forward(c, Bt, samp));
  TRY(launch_score_fwd(s, c.st));
  return launch_loss(s, c.st);
}

extern "C" int ps_tem_forward(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                              float* workspace, float* loss3, float* loss_acc, ps_stream_t stream) {
  PS_REQUIRE(desc && params && batch && workspace && loss3, "forward: null argument");
  const TemCall t(desc, TEM_TRAIN, stream);
  TRY(t.rc);
  PS_REQUIRE(batch->target_prod_idxs && batch->neg_item_idxs && (t.D.W == 0 || (batch->pos_iword_idxs &&
             batch->neg_word_idxs)), "forward: null batch tensors");
  PS_REQUIRE(params->word_bias && (!t.D.bias_product || params->product_bias), "forward: null bias tensors");
  return tem_forward(t.enc(*params, workspace, batch->u_item_idxs, t.st), *batch, nullptr, loss3, loss_acc, true, nullptr);
}

// forward with the two negative draws folded into its first launch: neg_item_out / neg_word_out receive the draws
// (they are what batch->neg_* would have held) and must stay alive until the backward has run.
extern "C" int ps_tem_forward_sampled(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                                      const float* alias_prob, const int32_t* alias_idx, int64_t* neg_item_out,
                                      int64_t* neg_word_out, float* workspace, float* loss3, float* loss_acc,
                                      ps_stream_t stream) {
  PS_REQUIRE(desc && params && batch && workspace && loss3 && alias_prob && alias_idx && neg_item_out && neg_word_out,
             "forward_sampled: null argument");
  const TemCall t(desc, TEM_TRAIN, stream);
  TRY(t.rc);
  PS_REQUIRE(batch->target_prod_idxs && (t.D.W == 0 || batch->pos_iword_idxs), "forward_sampled: null batch tensors");
  PS_REQUIRE(params->word_bias && (!t.D.bias_product || params->product_bias), "forward_sampled: null bias tensors");
  PsTemBatch Bt = *batch;
  Bt.neg_item_idxs = neg_item_out; Bt.neg_word_idxs = neg_word_out;
  const SamplerArgs samp = {alias_prob, alias_idx, neg_item_out, neg_word_out};
  return tem_forward(t.enc(*params, workspace, Bt.u_item_idxs, t.st), Bt, &samp, loss3, loss_acc, true, nullptr);
}

// Unit-test hook (prodsearch_hip.h): the forward with the embed launch in front (ws_a) and inside the projection + attention
// launch (ws_b), region by region.  Host-side comparison of copies: a test entry, not a step.
extern "C" int ps_set_front_fused(int on);
extern "C" int ps_front_fused_taken(void);
extern "C" int ps_front_fused_test(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch, const float* alias_prob,
                                   const int32_t* alias_idx, float* ws_a, float* ws_b, int64_t* neg_item_a, int64_t* neg_word_a,
                                   int64_t* neg_item_b, int64_t* neg_word_b, float* loss3_a, float* loss3_b, double* diff,
                                   int32_t* taken, ps_stream_t stream) {
  PS_REQUIRE(desc && params && batch && ws_a && ws_b && diff && taken && batch->u_item_idxs, "front_fused_test: null argument");
  PS_REQUIRE(desc->model == PS_MODEL_TEM && desc->n_layers >= 1, "front_fused_test: an item-transformer step with encoder layers");
  const TemCall t(desc, TEM_DESCRIBED, stream);   // (the layout to compare by; the two forwards build their own calls)
  TRY(t.rc);
  const PsTemDesc& D = t.D; const Ws& w = t.w; hipStream_t st = t.st;
  const int old = ps_set_front_fused(0);
  int rc = ps_tem_forward_sampled(desc, params, batch, alias_prob, alias_idx, neg_item_a, neg_word_a, ws_a, loss3_a, nullptr, stream);
  taken[0] = ps_front_fused_taken();
  if (rc == PS_OK) {
    ps_set_front_fused(1);
    rc = ps_tem_forward_sampled(desc, params, batch, alias_prob, alias_idx, neg_item_b, neg_word_b, ws_b, loss3_b, nullptr, stream);
    taken[1] = ps_front_fused_taken();
  }
  ps_set_front_fused(old);
  TRY(rc);
  PS_CHECK_HIP(hipStreamSynchronize(st));
  const int B = D.B, S = w.S, d = D.d, L = D.L;
  const LayerWs& l0 = w.layer[0];
  std::vector<int64_t> ui((size_t)B * L);
  PS_CHECK_HIP(hipMemcpy(ui.data(), batch->u_item_idxs, ui.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  std::vector<uint32_t> ha, hb;
  // words [off, off + n) of both workspaces -> ha / hb
  auto fetch = [&](const void* pa, const void* pb, size_t n) -> int {
    ha.resize(n); hb.resize(n);
    if (n == 0) return PS_OK;
    PS_CHECK_HIP(hipMemcpy(ha.data(), pa, n * 4, hipMemcpyDeviceToHost));
    PS_CHECK_HIP(hipMemcpy(hb.data(), pb, n * 4, hipMemcpyDeviceToHost));
    return PS_OK;
  };
  auto fdiff = [&](size_t i) -> double {          // as floats
    if (ha[i] == hb[i]) return 0.0;
    float x, y;
    memcpy(&x, &ha[i], 4); memcpy(&y, &hb[i], 4);
    const double e = fabs((double)x - (double)y);
    return e == e ? e : INFINITY;
  };
  auto region_f = [&](int64_t off, size_t n, double& out) -> int {
    TRY(fetch(ws_a + off, ws_b + off, n));
    out = 0.0;
    for (size_t i = 0; i < n; ++i) out = fmax(out, fdiff(i));
    return PS_OK;
  };
  auto region_i = [&](const void* pa, const void* pb, size_t n, double& out) -> int {   // as int32 words
    TRY(fetch(pa, pb, n));
    out = 0.0;
    for (size_t i = 0; i < n; ++i) out = fmax(out, fabs((double)(int32_t)ha[i] - (double)(int32_t)hb[i]));
    return PS_OK;
  };
  for (int r = 0; r < PS_FRONT_TEST_REGIONS; ++r) diff[r] = 0.0;
  TRY(region_f(w.x, (size_t)B * S * d, diff[0]));
  TRY(region_f(w.qmean, (size_t)B * d, diff[1]));
  TRY(region_f(w.query_emb, (size_t)B * d, diff[2]));
  for (int kv = 0; kv < 2; ++kv) {                 // K / V rows exist at valid positions only
    TRY(fetch(ws_a + (kv ? l0.vp : l0.kp), ws_b + (kv ? l0.vp : l0.kp), (size_t)l0.n_in * S * d));
    if (l0.n_in != B || w.qpos != 0) continue;     // (other layouts: nothing to say about which rows are written)
    for (int b = 0; b < B; ++b)
      for (int s2 = 0; s2 < S; ++s2) {
        if (s2 > 0 && ui[(size_t)b * L + s2 - 1] == D.product_size) continue;
        for (int c = 0; c < d; ++c) diff[3 + kv] = fmax(diff[3 + kv], fdiff(((size_t)b * S + s2) * d + c));
      }
  }
  TRY(region_f(l0.qp, (size_t)l0.n_in * l0.Sq * d, diff[5]));
  TRY(region_f(l0.attn, (size_t)l0.n_in * D.H * l0.Sq * S, diff[6]));
  if (l0.amask) TRY(region_i(ws_a + l0.amask, ws_b + l0.amask, (size_t)l0.n_in * l0.fan * D.H, diff[7]));
  TRY(region_f(l0.ctx, (size_t)l0.M2 * d, diff[8]));
  TRY(region_f(w.word_scores, (size_t)B * D.W * (D.K + 1), diff[9]));
  TRY(region_f(w.word_terms, (size_t)B * D.W * (D.K + 1), diff[10]));
  TRY(region_i(neg_item_a, neg_item_b, (size_t)2 * B * D.K, diff[11]));
  TRY(region_i(neg_word_a, neg_word_b, (size_t)2 * B * D.W * D.K, diff[12]));
  if (w.vrows) {
    int32_t ca = 0, cb = 0;
    PS_CHECK_HIP(hipMemcpy(&ca, ws_a + w.vcount, 4, hipMemcpyDeviceToHost));
    PS_CHECK_HIP(hipMemcpy(&cb, ws_b + w.vcount, 4, hipMemcpyDeviceToHost));
    diff[14] = fabs((double)ca - (double)cb);
    const int n = ca < cb ? ca : cb;
    PS_REQUIRE(n >= 0 && n <= B * S, "front_fused_test: row count %d / %d out of range", ca, cb);
    TRY(region_i(ws_a + w.vrows, ws_b + w.vrows, (size_t)n, diff[13]));
  }
  return PS_OK;
}

extern "C" int ps_gather_score(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                               float* workspace, ps_stream_t stream) {
  PS_REQUIRE(desc && params && batch && workspace, "gather_score: null argument");
  const TemCall t(desc, TEM_TRAIN, stream);
  TRY(t.rc);
  ScoreArgs s;
  fill_score(t.base(*params, workspace), *batch, s);
  return launch_score_fwd(s, t.st);
}

extern "C" int ps_tem_score(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                            float* workspace, float* scores, ps_stream_t stream) {
  PS_REQUIRE(desc && params && batch && workspace && scores, "score: null argument");
  PS_REQUIRE(desc->C > 0 && batch->candi_prod_idxs, "score: needs C > 0 candidates");
  const TemCall t(desc, TEM_EVAL, stream);
  TRY(t.rc);
  const EncCall c = t.enc(*params, workspace, batch->u_item_idxs, t.st);
  TRY(encode_forward(c, *batch));
  ScoreArgs s;
  fill_score(c, *batch, s);
  s.C = t.D.C; s.item_scores = scores; score_finish(s);
  return launch_score_fwd(s, t.st);
}

// model.eval() sequence representation the dot-product heads consume (item_transformer.py:118-131): one encode per
// (user, query) row, replicas collapse (R = 1).  Feeds ps_rank_all (full-catalogue evaluation).
extern "C" int ps_tem_encode(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                             float* workspace, float* enc_out, ps_stream_t stream) {
  PS_REQUIRE(desc && params && batch && workspace && enc_out, "encode: null argument");
  PS_REQUIRE(desc->C > 0, "encode: build the descriptor in eval mode (C >= 1)");
  const TemCall t(desc, TEM_EVAL, stream);
  TRY(t.rc);
  TRY(encode_forward(t.enc(*params, workspace, batch->u_item_idxs, t.st), *batch));
  PS_CHECK_HIP(hipMemcpyAsync(enc_out, workspace + t.w.enc, sizeof(float) * (size_t)t.D.B * t.D.d, hipMemcpyDeviceToDevice, t.st));
  return PS_OK;
}

extern "C" int ps_tem_plan(const PsTemDesc* desc, const PsTemTensors* params, int32_t has_valid, PsEncPath* out) {
  PS_REQUIRE(desc && out, "plan: null argument");
  const TemCall t(desc, TEM_DESCRIBED, nullptr);
  TRY(t.rc);
  const PsTemDesc& D = t.D;
  // enc_call tests pointers against null and adds offsets to the workspace base, nothing more: stand-ins that are never read
  static float stand_in[4];
  PsTemTensors all;
  memset(&all, 0, sizeof(all));
  if (!params) {
    const float** slot = reinterpret_cast<const float**>(&all);
    for (size_t k = 0; k < sizeof(all) / sizeof(float*); ++k) slot[k] = stand_in;
  }
  const EncPlan pl = enc_call(t.base(params ? *params : all, stand_in), nullptr, has_valid ? stand_in : nullptr, t.listed).plan;
  memset(out, 0, sizeof(*out));
  const bool enc = D.model == PS_MODEL_TEM && D.n_layers > 0;
  out->n_layers = enc ? D.n_layers : 0;
  for (int i = 0; i < out->n_layers; ++i) out->attn[i] = pl.attn[i];
  out->rowlist = pl.rowlist; out->fwd_fuse_last = pl.fwd_fuse_last; out->fold_score = pl.fold_score;
  out->bwd_fuse_last = pl.bwd.fuse_last; out->item_scatter = pl.bwd.item_scatter; out->wg3_main = pl.bwd.wg3_main;
  out->wg3_last = pl.bwd.wg3_last; out->wgrad_early = pl.bwd.wgrad_early; out->q_folded = pl.bwd.q_folded;
  out->listed = pl.bwd.listed; out->presum = pl.bwd.presum; out->dx_fused = pl.bwd.dx_fused;
  return PS_OK;
}

// --------------------------------------------------------------------- backward
static int tem_backward_impl(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                             float* ws, const PsTemTensors* grads, float loss_scale, const float* loss_scale_dev,
                             ps_stream_t stream, EncBwdOut& out) {
  PS_REQUIRE(desc && params && batch && ws && grads, "backward: null argument");
  enc_taken_clear(1, 0);                          // (QEM / AEM / ZAM: no encoder layers; enc_layers_backward fills it otherwise)
  const TemCall t(desc, TEM_TRAIN, stream);
  TRY(t.rc);
  const PsTemDesc& D = t.D; const Ws& w = t.w; hipStream_t st = t.st;
  const PsTemTensors& P = *params;
  const PsTemTensors& G = *grads;
  const EncCall c = t.enc(P, ws, batch->u_item_idxs, st);
  const bool tem = D.model == PS_MODEL_TEM;
  const int B = D.B, d = D.d, S = w.S, NL = tem ? D.n_layers : 0;
  const float* hist = D.sep_prod_emb ? P.hist_product_emb : P.product_emb;
  float* ghist = D.sep_prod_emb ? G.hist_product_emb : G.product_emb;
  // G.word_emb null: the word table is frozen (a pretrained table, nn.Embedding.from_pretrained): no kernel reads or writes a
  // word-row gradient, and the d mean of the query encoder (its only consumer) is not built
  const bool word_grad = G.word_emb != nullptr;
  PS_REQUIRE(G.product_emb && G.word_bias && ghist && hist, "backward: null table gradient");
  PS_REQUIRE(!D.bias_product || G.product_bias, "backward: null product_bias gradient");

  // 1. loss + score backward: d enc, table-row scatter-adds
  ScoreArgs s;
  fill_score(c, *batch, s);
  s.scale = loss_scale; s.scale_dev = loss_scale_dev; s.denc = ws + w.denc;
  s.g_product_emb = G.product_emb; s.g_word_emb = G.word_emb; s.g_product_bias = G.product_bias;
  s.g_word_bias = G.word_bias;
  // TEM with replicas: the encoder backward decides where the score backward runs (enc_layers_backward, score_on_side)
  static const bool score_side_on = ps_diag_int("PS_SCORE_BWD_MAIN", 0) == 0;
  const bool score_deferred = tem && NL > 0 && w.R > 1 && score_side_on;
  if (!score_deferred) TRY(launch_score_bwd(s, st));

  const float* wp_w[PS_WPLANES_MAX]; int wp_r[PS_WPLANES_MAX], wp_c[PS_WPLANES_MAX];
  const int wp_n = wplane_list(D, P, w, wp_w, wp_r, wp_c);
  WPlaneScope wplanes(st, wp_w, wp_r, wp_c, wp_n);             // the dX products read the TRANSPOSED weight planes (gemm_kernels.hip)
  ColFoldList fold;
  fold.n = 0;
  const float* dqe = ws + w.denc;   // grad wrt query_emb rows (QEM: enc IS query_emb)
  int lddqe = d;
  if (tem) {
    EncBwdIn in;
    in.fold = &fold; in.score_on_side = score_deferred ? &s : nullptr;
    in.caller_flushes_tail = true;     // out.wg3_last and out.score_words_last: this function's last launches
    TRY(enc_layers_backward(c, G, in, out));
    dqe = ws + w.dx;      // row 0 of each sequence is the query embedding
    lddqe = S * d;
  } else if (ps_model_attn(D.model)) {
    TRY(ae_backward(c, G));
    dqe = ws + w.ae_dqe;
  }

  // 4. query encoder backward + scatter to the word / history rows
  bool fw_by_gemm = false;
  EmbedBwdArgs e;
  memset(&e, 0, sizeof(e));
  e.B = B; e.Q = D.Q; e.L = D.L; e.S = S; e.d = d; e.P = D.product_size; e.V = D.vocab_size; e.tem = tem;
  e.qw = batch->query_word_idxs; e.ui = batch->u_item_idxs; e.dx = ws + w.dx;
  if (out.dx_two_partials) e.dx2 = ws + w.dxn;   // the attention backward left d x as two partial rows per position
  e.drop_fs = make_drop(D, PS_SITE_FS);
  e.g_hist_tab = ghist; e.g_word_emb = G.word_emb;
  if (D.query_encoder == PS_QENC_FS) {
    PS_REQUIRE(G.fs_w && G.fs_b, "backward: null FS encoder gradient");
    e.fw_x = ws + w.qmean; e.g_fs_w = G.fs_w;   // f_W weight gradient rides in the scatter launch (extra workgroups)
    if (ps_fusion_enabled() && d <= 128) {
      // ... and so does the rest of the FS backward: tanh', d mean = dqpre . f_W (per-row mat-vec), bias gradient
      e.fsb_dqe = dqe; e.fsb_lddqe = lddqe; e.fsb_qe = ws + w.query_emb; e.fsb_w = P.fs_w; e.g_fs_b = G.fs_b;
      if (word_grad) e.det_dm = ws + w.dqmean;    // (deterministic mode only: launch_embed_scatter)
      // round 5: the f_W weight gradient as one more member of the weight-gradient GEMM launched behind this one, instead of 512
      // extra workgroups of the scatter launch looping over the batch (33 of its 40 us at C2: tools/scatter_parts.sh); the row
      // workgroups leave dqpre in the workspace for it and add the bias gradient themselves.  PS_FW_BY_GEMM=0: the riders.
      static const bool fw_gemm_on = ps_env_int("PS_FW_BY_GEMM", 1) != 0;
      if (fw_gemm_on && !ps_deterministic()) { e.fsb_dqpre_out = ws + w.dqpre; fw_by_gemm = true; }
    } else {
      TRY(launch_tanh_bwd(dqe, lddqe, ws + w.query_emb, ws + w.dqpre, G.fs_b, B, d, st));
      if (word_grad) {
        GemmProblem p = gp(ws + w.dqpre, d, 0, P.fs_w, d, 1, ws + w.dqmean, d, B, d, d);   // d mean = dqpre . f_W
        p.no_deep = 1;   // the tail of the main stream, beside the side stream's weight gradients: the 128-deep form's 133 KB of LDS per
                         // workgroup waits for whole CUs there (50 us for 0.13 GFLOP at the C5 shard, r04_c5_step_timeline.txt)
        TRY(run1(p, st));
        e.dqmean_d = ws + w.dqmean;
      }
      e.fw_dy = ws + w.dqpre;
    }
  } else if (word_grad) {
    // AVG encoder: query_emb == post-dropout mean; copy rows to a dense [B,d] buffer
    PS_CHECK_HIP(hipMemcpy2DAsync(ws + w.dqmean, sizeof(float) * d, dqe, sizeof(float) * lddqe, sizeof(float) * d, B,
                                  hipMemcpyDeviceToDevice, st));
    e.dqmean_d = ws + w.dqmean;
  }
  e.fold = fold;
  TRY(launch_embed_scatter(e, st));
  if (fw_by_gemm) {      // g_fs_w[o][i] += sum_b dqpre[b][o] * qmean[b][i]  (text_encoder.py:38)
    PS_REQUIRE(out.wg3_last_n <= 3, "backward: deferred weight-gradient group is full");
    out.wg3_last[out.wg3_last_n++] = gp_wgrad(ws + w.dqpre, d, ws + w.qmean, d, G.fs_w, d, d, B);
  }
  if (out.wg3_last_n) TRY(run_wgrads(out.wg3_last, out.wg3_last_n, st));
  if (out.score_words_last) {      // the word tasks of the score backward (the fused backward has scattered the item rows)
    ScoreArgs t = s;
    t.denc = nullptr; t.items_elsewhere = 1;
    TRY(launch_score_bwd(t, st));
  }
  TRY(side_join(st));
  return PS_OK;
}

extern "C" int ps_tem_backward(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                               float* ws, const PsTemTensors* grads, float loss_scale, const float* loss_scale_dev,
                               ps_stream_t stream) {
  EncBwdOut out;
  const int rc = tem_backward_impl(desc, params, batch, ws, grads, loss_scale, loss_scale_dev, stream, out);
  enc_record_backward(out);
  if (rc != PS_OK) side_abort();    // never leave the side stream waiting behind a failed call
  return rc;
}

// ------------------------------------------------------------------ graph-replayed training step (graph.h)
// Layout of the staging region: [step word | pad] then the six int64 index arrays, 16-byte aligned each.
struct StageLayout { uint32_t* step_word; int64_t* p[6]; int n[6]; };
static StageLayout stage_layout(const PsTemDesc& D, float* ws, const Ws& w) {
  StageLayout L;
  L.step_word = reinterpret_cast<uint32_t*>(ws + w.stage);
  int64_t* base = reinterpret_cast<int64_t*>(ws + w.stage + 4);
  const int n[6] = {D.B * D.Q, D.B * D.L, D.B, D.B * D.W, D.B * D.K, D.B * D.W * D.K};
  int64_t off = 0;
  for (int k = 0; k < 6; ++k) { L.p[k] = base + off; L.n[k] = n[k]; off += (n[k] + 1) & ~1; }
  return L;
}
static PsTemBatch staged_batch(const StageLayout& L) {
  PsTemBatch b;
  memset(&b, 0, sizeof(b));
  b.query_word_idxs = L.p[0]; b.u_item_idxs = L.p[1]; b.target_prod_idxs = L.p[2]; b.pos_iword_idxs = L.p[3];
  b.neg_item_idxs = L.p[4]; b.neg_word_idxs = L.p[5];
  return b;
}

extern "C" int ps_graph_replay_enabled(void) { return ps_graphs_enabled() ? 1 : 0; }

// where ps_tem_forward_step staged the call's index tensors (for an eager ps_tem_backward after a replayed forward)
extern "C" int ps_tem_staged_batch(const PsTemDesc* desc, float* workspace, PsTemBatch* out) {
  PS_REQUIRE(desc && workspace && out, "staged_batch: null argument");
  const TemCall t(desc, TEM_TRAIN, nullptr);
  TRY(t.rc);
  *out = staged_batch(stage_layout(t.D, workspace, t.w));
  return PS_OK;
}

// forward of one training step with the caller-varying inputs routed through the staging prologue, so that the launch
// sequence can be captured once per shape and replayed.  sampler_prob/alias non-null: negatives are drawn in the
// prologue (batch->neg_* ignored), else batch->neg_* are staged like the other index tensors.
extern "C" int ps_tem_forward_step(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                                   const float* sampler_prob, const int32_t* sampler_alias, float* workspace,
                                   float* loss3, float* loss_acc, ps_stream_t stream) {
  PS_REQUIRE(desc && params && batch && workspace && loss3, "forward_step: null argument");
  const TemCall t(desc, TEM_TRAIN, stream);
  TRY(t.rc);
  const PsTemDesc& D = t.D;
  const bool sampled = sampler_prob && sampler_alias;
  const bool hist = D.model == PS_MODEL_TEM || ps_model_attn(D.model);
  PS_REQUIRE(batch->query_word_idxs && batch->target_prod_idxs && (!hist || batch->u_item_idxs) &&
             (D.W == 0 || batch->pos_iword_idxs), "forward_step: null batch tensors");
  PS_REQUIRE(sampled || (batch->neg_item_idxs && (D.W == 0 || batch->neg_word_idxs)), "forward_step: no negatives");
  PS_REQUIRE(params->word_bias && (!D.bias_product || params->product_bias), "forward_step: null bias tensors");
  const StageLayout L = stage_layout(D, workspace, t.w);
  const PsTemBatch Bs = staged_batch(L);
  StageArgs sa;
  memset(&sa, 0, sizeof(sa));
  const int64_t* src[6] = {batch->query_word_idxs, hist ? batch->u_item_idxs : nullptr,
                           batch->target_prod_idxs, D.W > 0 ? batch->pos_iword_idxs : nullptr,
                           sampled ? nullptr : batch->neg_item_idxs, (sampled || D.W == 0) ? nullptr : batch->neg_word_idxs};
  for (int k = 0; k < 6; ++k) { sa.src[k] = src[k]; sa.dst[k] = L.p[k]; sa.n[k] = L.n[k]; }
  sa.step = (uint32_t)D.step; sa.step_word = L.step_word;
  if (sampled) {
    sa.prob = sampler_prob; sa.alias = sampler_alias; sa.nitem = D.B * D.K; sa.nword = D.B * D.W * D.K;
    sa.P = D.product_size; sa.V = D.vocab_size;
    sa.k0 = (uint32_t)(D.seed & 0xffffffffu); sa.k1 = (uint32_t)(D.seed >> 32);
  }
  ps_step_ptr_slot() = L.step_word;               // every DropSpec built below reads the step from the workspace
  PsGraphEntry* e = nullptr;
  if (ps_graphs_enabled()) {
    PsTemDesc Dk = D;
    Dk.step = 0;
    uint64_t key = ps_fnv(PS_FNV0, "fwd", 3);
    key = ps_fnv(key, &Dk, sizeof(Dk)); key = ps_fnv(key, params, sizeof(*params));
    key = ps_fnv(key, &workspace, sizeof(workspace)); key = ps_fnv(key, &loss_acc, sizeof(loss_acc));
    key = ps_fnv(key, &sampler_prob, sizeof(sampler_prob)); key = ps_fnv(key, &sampler_alias, sizeof(sampler_alias));
    for (int k = 0; k < 6; ++k) { const int has = sa.src[k] != nullptr; key = ps_fnv(key, &has, sizeof(has)); }
    e = ps_graph_lookup(key);
  }
  ScoreArgs s;                                    // a replay's loss-kernel arguments
  if (e && e->state == 2) {
    fill_score(t.base(*params, workspace), Bs, s);
    s.loss3 = loss3; s.loss_acc = loss_acc; s.loss_nblk = score_fwd_blocks(s);
  }
  const PsGraphPatch patch[2] = {{stage_kernel_handle(), &sa}, {loss_kernel_handle(), &s}};
  // (never folded, captured or not: may_fold = false)
  const int rc = ps_graph_step(e, t.st, "forward_step", patch, 2, [&](hipStream_t on) {
    return tem_forward(t.enc(*params, workspace, Bs.u_item_idxs, on), Bs, nullptr, loss3, loss_acc, false, &sa);
  });
  ps_step_ptr_slot() = nullptr;
  return rc;
}

// backward of the step ps_tem_forward_step ran last on this workspace (its staged indices and step word are reused);
// zero_ptr/zero_floats: model.zero_grad() of the flat gradient buffer folded in as the first node (or null).
extern "C" int ps_tem_backward_step(const PsTemDesc* desc, const PsTemTensors* params, float* ws,
                                    const PsTemTensors* grads, float loss_scale, float* zero_ptr, int64_t zero_floats,
                                    ps_stream_t stream) {
  PS_REQUIRE(desc && params && ws && grads, "backward_step: null argument");
  const TemCall t(desc, TEM_TRAIN, stream);
  TRY(t.rc);
  const StageLayout L = stage_layout(t.D, ws, t.w);
  const PsTemBatch Bs = staged_batch(L);
  ps_step_ptr_slot() = L.step_word;
  PsGraphEntry* e = nullptr;
  if (ps_graphs_enabled()) {
    PsTemDesc Dk = t.D;
    Dk.step = 0;
    uint64_t key = ps_fnv(PS_FNV0, "bwd", 3);
    key = ps_fnv(key, &Dk, sizeof(Dk)); key = ps_fnv(key, params, sizeof(*params)); key = ps_fnv(key, grads, sizeof(*grads));
    key = ps_fnv(key, &ws, sizeof(ws)); key = ps_fnv(key, &loss_scale, sizeof(loss_scale));
    key = ps_fnv(key, &zero_ptr, sizeof(zero_ptr)); key = ps_fnv(key, &zero_floats, sizeof(zero_floats));
    e = ps_graph_lookup(key);
  }
  const int rc = ps_graph_step(e, t.st, "backward_step", nullptr, 0, [&](hipStream_t on) -> int {
    if (zero_ptr && zero_floats > 0) PS_CHECK_HIP(hipMemsetAsync(zero_ptr, 0, sizeof(float) * (size_t)zero_floats, on));
    return ps_tem_backward(&t.D, params, &Bs, ws, grads, loss_scale, nullptr, on);
  });
  ps_step_ptr_slot() = nullptr;
  if (rc != PS_OK) side_abort();
  return rc;
}

extern "C" float ps_dropout_mult_host(const PsTemDesc* desc, uint32_t site, uint32_t row, uint32_t col) {
  PsTemDesc D = *desc;
  D.training = 1;
  DropSpec s = make_drop(D, site);
  if (s.thr == 0u) return 1.f;
  if (s.half) return drop_half(s, drop_call16(s, row, col >> 3, s.step), (int)(col & 7u));
  Philox4 r = philox4x32_10(col, row >> 2, s.site, s.step, s.k0, s.k1);
  uint32_t sel = row & 3u;
  uint32_t wv = sel == 0 ? r.x : (sel == 1 ? r.y : (sel == 2 ? r.z : r.w));
  return wv >= s.thr ? s.scale : 0.f;
}

// ------------------------------------------------------------ sampling / alias
extern "C" int ps_sample_negatives(const PsTemDesc* desc, const float* alias_prob, const int32_t* alias_idx,
                                   int64_t* neg_item_idxs, int64_t* neg_word_idxs, ps_stream_t stream) {
  PS_REQUIRE(desc && alias_prob && alias_idx && neg_item_idxs && neg_word_idxs, "sample: null argument");
  return launch_sample(*desc, alias_prob, alias_idx, neg_item_idxs, neg_word_idxs, (hipStream_t)stream);
}

// Vose's alias method over `n` outcomes with (unnormalised) weights dist[].
extern "C" int ps_build_alias_host(const double* dist, int64_t n, float* prob, int32_t* alias) {
  PS_REQUIRE(dist && prob && alias && n > 0 && n < (1ll << 31), "alias: bad argument");
  double sum = 0;
  for (int64_t i = 0; i < n; ++i) { PS_REQUIRE(dist[i] >= 0, "alias: negative weight"); sum += dist[i]; }
  PS_REQUIRE(sum > 0, "alias: zero total weight");
  double* q = new double[n];
  int32_t* small = new int32_t[n];
  int32_t* large = new int32_t[n];
  int64_t ns = 0, nl = 0;
  for (int64_t i = 0; i < n; ++i) {
    q[i] = dist[i] / sum * (double)n;
    alias[i] = (int32_t)i;
    if (q[i] < 1.0) small[ns++] = (int32_t)i; else large[nl++] = (int32_t)i;
  }
  while (ns > 0 && nl > 0) {
    int32_t s = small[--ns], l = large[--nl];
    prob[s] = (float)q[s];
    alias[s] = l;
    q[l] = (q[l] + q[s]) - 1.0;
    if (q[l] < 1.0) small[ns++] = l; else large[nl++] = l;
  }
  while (nl > 0) prob[large[--nl]] = 1.f;
  while (ns > 0) prob[small[--ns]] = 1.f;
  delete[] q; delete[] small; delete[] large;
  return PS_OK;
}
