// encoder.hip — the transformer encoder both models share (encoder.h): workspace layout, the per-call context and its plan (enc_call),
// the taken-path record and the layer loops, forward and backward.  The item models (tem.hip) and the review transformer
// (rtm.hip) call it alike.
//
// Structure of the encoder ("replicas"): the reference encodes the SAME (query, history)
// sequence K+1 times (once for the positive, K expanded copies for the negatives).  The copies
// only differ through dropout, which first acts on the softmax output of layer 0, so:
//   * K/V/Q projections and softmax of layer 0 run once per batch row          (n_in  = B)
//   * everything after the first dropout runs per replica                       (n_out = B*R)
//     with R = K+1 when dropout is drawn (training && dropout > 0) and R = 1 otherwise,
//     where all replicas are bit-identical and one is computed;
//   * the LAST layer only produces the one output position that is consumed
//     (x[:, 0] or x[:, -1], item_transformer.py:482-492), so its query/attention/FFN rows
//     are n_out x 1 instead of n_out x S.
#include "encoder.h"
#include "side_stream.h"
#include "wgrad.h"
#include <math.h>
#include <string.h>
#include <utility>

static int check_desc(const PsTemDesc& D) {
  PS_REQUIRE(D.B > 0 && D.K >= 0 && D.Q > 0 && D.W >= 0 && D.d > 0, "desc: bad sizes B=%d K=%d Q=%d W=%d d=%d",
             D.B, D.K, D.Q, D.W, D.d);
  PS_REQUIRE(D.d % 32 == 0 && D.d <= 512, "desc: embedding_size %d must be a multiple of 32 and <= 512", D.d);
  PS_REQUIRE(D.model == PS_MODEL_TEM || D.model == PS_MODEL_QEM || ps_model_attn(D.model), "desc: model %d", D.model);
  if (ps_model_attn(D.model)) {
    const int S = D.L + ae_zoff(D);
    PS_REQUIRE(D.L >= (D.model == PS_MODEL_AEM ? 1 : 0) && S <= 64, "desc: history length %d (AEM: L >= 1, S <= 64)", D.L);
    PS_REQUIRE(D.H > 0 && D.d % D.H == 0 && D.d / D.H <= 64 && D.H * S <= 4096, "desc: heads %d for d %d", D.H, D.d);
  }
  if (D.model == PS_MODEL_TEM) {
    PS_REQUIRE(D.L >= 0 && D.L + 1 <= 64, "desc: history length %d (S <= 64)", D.L);
    PS_REQUIRE(D.n_layers >= 0 && D.n_layers <= PS_MAX_LAYERS, "desc: inter_layers %d", D.n_layers);
    if (D.n_layers > 0) {
      PS_REQUIRE(D.H > 0 && D.d % D.H == 0 && D.d / D.H <= 64, "desc: heads %d for d %d", D.H, D.d);
      PS_REQUIRE(D.F > 0 && D.F % 4 == 0, "desc: ff_size %d", D.F);
    }
  }
  PS_REQUIRE(D.dropout >= 0.f && D.dropout < 1.f, "desc: dropout %f", D.dropout);
  PS_REQUIRE(D.product_size > 0 && D.vocab_size > 1, "desc: table sizes");
  return PS_OK;
}

static inline int64_t take(int64_t& cur, int64_t n) {
  int64_t o = cur;
  cur += (n + 3) & ~(int64_t)3;     // keep every buffer 16-byte aligned
  return o;
}

int make_ws(const PsTemDesc& D, Ws& w) {
  int rc = check_desc(D);
  if (rc) return rc;
  memset(&w, 0, sizeof(w));
  const bool tem = D.model == PS_MODEL_TEM, ae = ps_model_attn(D.model);
  const bool drop = D.training && D.dropout > 0.f;
  const int B = D.B, d = D.d, S = tem ? D.L + 1 : (ae ? D.L + ae_zoff(D) : 1), NL = tem ? D.n_layers : 0;
  w.S = S;
  w.R = (((tem && NL > 0) || ae) && drop && D.C == 0) ? D.K + 1 : 1;
  w.qpos = D.use_item_pos ? S - 1 : 0;
  int64_t cur = 0;
  w.qmean = take(cur, (int64_t)B * d);
  w.query_emb = take(cur, (int64_t)B * d);
  w.x = tem ? take(cur, (int64_t)B * S * d) : 0;
  int64_t maxM2 = 0, maxNS = 0;
  for (int i = 0; i < NL; ++i) {
    LayerWs& l = w.layer[i];
    l.n_in = i == 0 ? B : B * w.R;
    l.n_out = B * w.R;
    l.fan = l.n_out / l.n_in;
    l.Sq = i == NL - 1 ? 1 : S;
    l.M2 = l.n_out * l.Sq;
    const int64_t ns = (int64_t)l.n_in * S;
    l.xn = i == 0 ? w.x : take(cur, ns * d);
    l.pre_stats = i == 0 ? 0 : take(cur, ns * 2);
    l.kp = take(cur, ns * d);
    l.vp = take(cur, ns * d);
    l.qp = take(cur, (int64_t)l.n_in * l.Sq * d);
    l.attn = take(cur, (int64_t)l.n_in * D.H * l.Sq * S);
    l.amask = take(cur, (int64_t)l.n_in * l.fan * D.H);
    l.ctx = take(cur, (int64_t)l.M2 * d);
    l.y1 = take(cur, (int64_t)l.M2 * d);
    l.ff_stats = take(cur, (int64_t)l.M2 * 2);
    l.ln1 = take(cur, (int64_t)l.M2 * d);
    l.a1 = take(cur, (int64_t)l.M2 * D.F);
    l.h1 = take(cur, (int64_t)l.M2 * D.F);
    l.y2 = take(cur, (int64_t)l.M2 * d);
    maxM2 = l.M2 > maxM2 ? l.M2 : maxM2;
    maxNS = ns > maxNS ? ns : maxNS;
  }
  w.Mf = B * w.R;
  w.fin_stats = take(cur, (int64_t)w.Mf * 2);
  if (ae) {      // AEM / ZAM (attn_emb.hip): key rows, K / V / Q, softmax, per-replica ctx and their gradients
    LayerWs& l = w.layer[0];
    const int64_t ns = (int64_t)B * S;
    l.n_in = B; l.n_out = B * w.R; l.fan = w.R; l.Sq = 1; l.M2 = B * w.R;
    w.x = take(cur, ns * d);
    l.kp = take(cur, ns * d);
    l.vp = take(cur, ns * d);
    l.qp = take(cur, (int64_t)B * d);
    l.attn = take(cur, (int64_t)B * D.H * S);
    l.ctx = take(cur, (int64_t)B * w.R * d);
    w.ae_qhalf = take(cur, (int64_t)B * d);
    w.ae_dhalf = take(cur, (int64_t)B * w.R * d);
    w.dctx = take(cur, (int64_t)B * w.R * d);
    w.ae_dqe = take(cur, (int64_t)B * d);
    w.ae_dqp = take(cur, (int64_t)B * d);
    w.ae_dk = take(cur, ns * d);
    w.ae_dv = take(cur, ns * d);
    w.dx = take(cur, ns * d);
    w.ae_part = take(cur, (int64_t)4 * PS_AE_COL_SPLITS * d);
    w.ae_keys = take(cur, (int64_t)2 * B * D.L);     // int32 [2][B*L]: deterministic scatter tasks
  }
  w.enc = (tem || ae) ? take(cur, (int64_t)w.Mf * d) : w.query_emb;
  const int C = D.C > 0 ? D.C : D.K + 1;
  w.item_scores = take(cur, (int64_t)B * C);
  w.word_scores = take(cur, (int64_t)B * (D.W > 0 ? D.W : 1) * (D.K + 1));
  w.loss_parts = take(cur, (int64_t)B * 2);
  w.item_terms = take(cur, (int64_t)B * (D.K + 1));
  w.word_terms = take(cur, (int64_t)B * (D.W > 0 ? D.W : 1) * (D.K + 1));
  w.loss_blk = take(cur, 2 * ((int64_t)B * (D.K + 1) * (1 + D.W) / 4 + 2));     // >= 2 floats per score workgroup
  w.word_blk = take(cur, ps_cdiv((int64_t)B * (D.W > 0 ? D.W : 1) * (D.K + 1), PS_WORD_TASKS_PER_WG) + 4);
  w.item_blk = take(cur, ps_cdiv((int64_t)B * w.R, 32) + 4);
  w.ticket = take(cur, 20);      // 9 x 64-bit words (8 shards + top), 16-byte aligned
  w.wsplit = (tem && NL > 0 && d == 128 && mlp_x3_enabled(D.F)) ? take(cur, mlp_x3_floats(d, D.F)) : 0;
  // backward scratch (sized for the widest layer)
  w.denc = take(cur, (int64_t)w.Mf * d);
  if (tem) {
    const int64_t F = NL > 0 ? D.F : 0;
    w.dy2 = take(cur, (maxM2 > w.Mf ? maxM2 : w.Mf) * d);
    w.do2 = take(cur, maxM2 * d);
    w.da1 = take(cur, maxM2 * F);
    w.dln1 = take(cur, maxM2 * d);
    w.dy1 = take(cur, maxM2 * d);
    w.do_ = take(cur, maxM2 * d);
    w.dctx = take(cur, maxM2 * d);
    w.dq = take(cur, maxNS * d);
    w.dkv = take(cur, maxNS * 3 * d);
    w.dxn = take(cur, maxNS * d);
    w.dx = take(cur, (int64_t)B * S * d);
  }
  w.dqpre = take(cur, (int64_t)B * d);
  w.dqmean = take(cur, (int64_t)B * d);
  w.lnrows = (int)((maxM2 + 31) / 32 > 256 ? (maxM2 + 31) / 32 : 256);
  w.lnpart = take(cur, (int64_t)PS_MAX_COLFOLD * w.lnrows * 3 * d);
  w.stage = take(cur, 4 + 2 * ((int64_t)B * (D.Q + D.L + 1 + D.W + D.K + D.W * D.K) + 8));   // int64 = 2 floats
  w.gcpart = take(cur, (int64_t)4 * ((maxM2 + 31) / 32 + 1) * 3 * (tem && NL > 0 ? D.F : 0));   // >= mlp_bwd_b1_rows()
  w.abpart = take(cur, (int64_t)NL * (NL > 0 ? w.layer[NL - 1].n_in : 0) * 3 * d);
  w.vrows = tem ? take(cur, (int64_t)B * S + 4) : 0;
  w.vcount = tem ? take(cur, 4) : 0;
  w.total = cur;
  return PS_OK;
}

extern "C" int ps_tem_workspace_layout(const PsTemDesc* desc, PsTemWsLayout* out) {
  PS_REQUIRE(desc && out, "workspace_layout: null argument");
  Ws w;
  int rc = make_ws(*desc, w);
  if (rc) return rc;
  memset(out, 0, sizeof(*out));
  out->total_floats = w.total;
  out->R = w.R; out->S = w.S;
  out->qmean = w.qmean; out->query_emb = w.query_emb; out->x = w.x;
  const int NL = desc->model == PS_MODEL_TEM ? desc->n_layers : (ps_model_attn(desc->model) ? 1 : 0);
  if (NL > 0) {
    const LayerWs& l = w.layer[NL - 1];
    out->kp = l.kp; out->vp = l.vp; out->qp = l.qp; out->attn = l.attn; out->ctx = l.ctx;
    out->y1 = l.y1; out->ln1 = l.ln1; out->a1 = l.a1; out->h1 = l.h1; out->y2 = l.y2;
  }
  out->enc = w.enc;
  out->item_scores = w.item_scores; out->word_scores = w.word_scores; out->loss_parts = w.loss_parts;
  out->denc = w.denc; out->dx = w.dx;
  return PS_OK;
}

WSplit make_wsplit(const PsTemDesc& D, const PsTemTensors& P, float* ws, const Ws& w) {
  WSplit s;
  memset(&s, 0, sizeof(s));
  const int NL = D.model == PS_MODEL_TEM ? D.n_layers : 0;
  if (NL < 1 || !w.wsplit || D.d != 128 || !mlp_x3_enabled(D.F) || w.layer[NL - 1].Sq != 1) return s;
  const PsLayerTensors& L = P.layer[NL - 1];
  if (!L.wo || !L.w1 || !L.w2) return s;
  const int d = D.d, F = D.F;
  s.w[0] = L.wo; s.rows[0] = d; s.cols[0] = d;
  s.w[1] = L.w1; s.rows[1] = F; s.cols[1] = d;
  s.w[2] = L.w2; s.rows[2] = d; s.cols[2] = F;
  uint16_t* base = reinterpret_cast<uint16_t*>(ws + w.wsplit);
  const size_t n_wo = (size_t)3 * d * d, n_ff = (size_t)3 * 2 * d * F;
  s.fwd_wo = base; s.fwd_ff = base + n_wo; s.bwd_ff = base + n_wo + n_ff; s.bwd_wo = base + n_wo + 2 * n_ff;
  s.on = 1;
  if (NL == 1 && L.wk && L.wv) {      // one layer: its K / V projections can take the fused projection + attention forward
    s.wkv[0] = L.wk; s.wkv[1] = L.wv;
    s.fwd_kv = base + 2 * (n_wo + n_ff);
    s.bwd_kv = s.fwd_kv + (size_t)3 * 2 * d * d;
  }
  return s;
}

// The encoder weights a WPlaneScope (common.h) should hold for this call: the last layer's six linears when its products are
// big enough for the pre-split-weight kernel (>= 4096 replica rows) and are not taken by the fused d = 128 kernels.
int wplane_list(const PsTemDesc& D, const PsTemTensors& P, const Ws& w, const float** ws_, int* rows, int* cols) {
  const int NL = D.model == PS_MODEL_TEM ? D.n_layers : 0;
  if (NL < 1 || D.d < 256 || D.d % 32 || D.F % 32) return 0;
  int n = 0;
  for (int i = NL - 1; i >= 0 && n + 6 <= PS_WPLANES_MAX; --i) {
    const LayerWs& l = w.layer[i];
    if ((int64_t)l.M2 < 4096 && (int64_t)l.n_in * w.S < 4096) continue;
    const PsLayerTensors& L = P.layer[i];
    const float* ptr[6] = {L.wk, L.wv, L.wq, L.wo, L.w1, L.w2};
    const int r[6] = {D.d, D.d, D.d, D.d, D.F, D.d}, c[6] = {D.d, D.d, D.d, D.d, D.d, D.F};
    for (int k = 0; k < 6; ++k) { ws_[n] = ptr[k]; rows[n] = r[k]; cols[n] = c[k]; ++n; }
  }
  return n;
}

// the shape part of layer i's attention arguments — all that the attn_*_fits predicates read —, dividers filled
static AttnArgs attn_shape(const PsTemDesc& D, const Ws& w, int i, const int64_t* ui, const float* valid) {
  const LayerWs& l = w.layer[i];
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.n_in = l.n_in; a.fan = l.fan; a.H = D.H; a.S = w.S; a.Sq = l.Sq; a.d = D.d; a.dh = D.d / (D.H > 0 ? D.H : 1); a.qpos = w.qpos;
  a.seq_div = l.n_in / D.B; a.L = D.L; a.P = D.product_size; a.ui = ui; a.valid = valid;
  a.qscale = 1.f / sqrtf((float)a.dh);
  attn_finish(a);
  return a;
}

// Layer i's per-replica tail behind its attention (encoder.h): reads l.ctx and the residual rows of xin.
int enc_tail_forward(const EncBase& b, const WSplit& x3, int i, const float* xin, bool fuse, const ScoreArgs* fold_sc) {
  const PsTemDesc& D = b.D; const PsTemTensors& P = b.P; float* ws = b.ws; const Ws& w = b.w; hipStream_t st = b.st;
  const int d = D.d, S = w.S;
  const LayerWs& l = w.layer[i];
  const PsLayerTensors& Lp = P.layer[i];
  if (fuse) {   // Wo + LN + W1 + GELU + W2 + final LN of the last layer in one kernel (mlp_fused.hip)
    MlpFwdArgs m;
    memset(&m, 0, sizeof(m));
    m.M = l.M2; m.F = D.F; m.fan = l.fan; m.S = S; m.qpos = w.qpos;
    m.ctx = ws + l.ctx; m.xin = xin;
    m.wo = Lp.wo; m.bo = Lp.bo; m.g1 = Lp.ff_ln_g; m.be1 = Lp.ff_ln_b; m.w1 = Lp.w1; m.b1 = Lp.b1;
    m.w2 = Lp.w2; m.b2 = Lp.b2; m.gf = P.final_ln_g; m.bef = P.final_ln_b;
    m.drop_ctx = make_drop(D, PS_SITE_CTX(i)); m.drop_ff1 = make_drop(D, PS_SITE_FF1(i));
    m.drop_ff2 = make_drop(D, PS_SITE_FF2(i));
    m.y1 = ws + l.y1; m.ln1 = ws + l.ln1; m.st1 = ws + l.ff_stats; m.a1 = ws + l.a1; m.h1 = ws + l.h1;
    m.y2 = ws + l.y2; m.stf = ws + w.fin_stats; m.enc = ws + w.enc;
    if (fold_sc) { m.fold_score = 1; m.sc = *fold_sc; }
    m.x3 = x3;
    return launch_mlp_fwd_fused(m, st);
  }
  {   // final_linear + dropout + residual (neural.py:228-231, transformer.py:56)
    GemmProblem p = gp(ws + l.ctx, d, 0, Lp.wo, d, 0, ws + l.y1, d, l.M2, d, d);
    p.bias = Lp.bo; p.drop = make_drop(D, PS_SITE_CTX(i));
    p.res.mode = RES_GATHER; p.res.ptr = xin; p.res.ld = d; p.res.Sq = l.Sq; p.res.fan = l.fan; p.res.S = S;
    p.res.qpos = w.qpos; res_finish(p.res);
    TRY(run1(p, st));
  }
  {   // PositionwiseFeedForward (neural.py:30-33)
    LnFwdArgs n = {ws + l.y1, d, ws + l.ln1, d, ws + l.ff_stats, Lp.ff_ln_g, Lp.ff_ln_b, l.M2, d, 1e-6f};
    TRY(launch_ln_fwd(n, st));
    GemmProblem p1 = gp(ws + l.ln1, d, 0, Lp.w1, d, 0, ws + l.h1, D.F, l.M2, D.F, d);
    p1.bias = Lp.b1; p1.aux_out = ws + l.a1; p1.act = ACT_GELU; p1.drop = make_drop(D, PS_SITE_FF1(i));
    TRY(run1(p1, st));
    GemmProblem p2 = gp(ws + l.h1, D.F, 0, Lp.w2, D.F, 0, ws + l.y2, d, l.M2, d, D.F);
    p2.bias = Lp.b2; p2.drop = make_drop(D, PS_SITE_FF2(i));
    p2.res.mode = RES_DIRECT; p2.res.ptr = ws + l.y1; p2.res.ld = d;
    TRY(run1(p2, st));
  }
  return PS_OK;
}

// final LayerNorm (transformer.py:86) on the consumed position only
int enc_final_ln_forward(const EncBase& b) {
  const PsTemDesc& D = b.D; const PsTemTensors& P = b.P; float* ws = b.ws; const Ws& w = b.w; hipStream_t st = b.st;
  const int d = D.d, S = w.S, NL = D.n_layers;
  PS_REQUIRE(P.final_ln_g && P.final_ln_b, "forward: null final LayerNorm");
  LnFwdArgs f;
  if (NL > 0) {
    const LayerWs& l = w.layer[NL - 1];
    f = LnFwdArgs{ws + l.y2, d, ws + w.enc, d, ws + w.fin_stats, P.final_ln_g, P.final_ln_b, w.Mf, d, 1e-6f};
  } else {
    f = LnFwdArgs{ws + w.x + (size_t)w.qpos * d, S * d, ws + w.enc, d, ws + w.fin_stats, P.final_ln_g,
                  P.final_ln_b, D.B, d, 1e-6f};
  }
  TRY(launch_ln_fwd(f, st));
  return PS_OK;
}

// ---- what the plan reads besides its arguments (and ps_deterministic()): the env / diag switches, read once per process, and
// the three values the setters write, which enc_plan reads on every call
struct EncSwitches {
  bool rows_on, bwd_fuse_on, dx_fused_on;      // PS_NO_ROWLIST, PS_NO_FUSE_BWD, PS_KVDX_FUSED
  bool wgrad_early, wg3_main_on, wg3_last;     // PS_WGRAD_LATE, PS_WG3_SIDE (unset: by fork_by_kernel()), PS_WG3_LAST
  // The embed launch inside the projection + attention launch (front_attn_fwd_kernel, attn_sq1.hip): PS_FRONT_FUSED=0 /
  // ps_set_front_fused(0) restores the two launches; PS_KVQ_FUSED=0 implies it (the form is the kvq form's).
  int front_fused;
  int fuse_bwd_min;                            // PS_FUSE_BWD_MIN / ps_set_fuse_bwd_min
  // The item rows' gradient scatter (g_product_emb[idx(b, j)] += ds * enc[(b, j)]) rides in the fused per-replica backward, which
  // holds ds and idx already, and the score backward's launch shrinks to its word tasks (MlpBwdArgs::g_product_emb,
  // ScoreArgs::items_elsewhere), which then are the main stream's last launch instead of the side stream's first (see
  // bwd_fused_last).  PS_ITEM_SCATTER_FUSED=0: the score backward's own item workgroups, on the side stream, as before.
  // Deterministic mode never takes it (its sole-owner scatter walks the item tasks in order).
  int item_scatter_fused;
};
static EncSwitches& enc_switches() {
  static const int wg3_side = ps_diag_int("PS_WG3_SIDE", -1);
  static EncSwitches s = {ps_env_int("PS_NO_ROWLIST", 0) == 0, ps_env_int("PS_NO_FUSE_BWD", 0) == 0, ps_env_int("PS_KVDX_FUSED", 1) != 0,
                          ps_diag_int("PS_WGRAD_LATE", 0) == 0, wg3_side >= 0 ? wg3_side == 0 : fork_by_kernel(), ps_diag_int("PS_WG3_LAST", 1) != 0,
                          ps_env_int("PS_FRONT_FUSED", 1), ps_env_int("PS_FUSE_BWD_MIN", 1024), ps_env_int("PS_ITEM_SCATTER_FUSED", 1)};
  return s;
}
extern "C" int ps_set_front_fused(int on) { return std::exchange(enc_switches().front_fused, on); }
extern "C" int ps_set_fuse_bwd_min(int rows) { return std::exchange(enc_switches().fuse_bwd_min, rows); }
extern "C" int ps_set_item_scatter_fused(int on) { return std::exchange(enc_switches().item_scatter_fused, on); }

// What the last forward [0] / backward [1] launched (encoder.h, enc_taken); item_scatter: the fused kernel scattered the item rows.
// front: the last forward embedded inside layer 0's launch (ps_front_fused_taken; PsEncPath has no field for it)
static struct { PsEncPath path[2]; int front; } g_taken;
PsEncPath& enc_taken(int backward) { return g_taken.path[backward ? 1 : 0]; }
void enc_taken_clear(int backward, int n_layers) {
  PsEncPath& t = enc_taken(backward);
  memset(&t, 0, sizeof(t));
  if (!backward) g_taken.front = 0;
  t.n_layers = n_layers;
}
extern "C" int ps_front_fused_taken(void) { return g_taken.front; }
extern "C" int ps_item_scatter_fused_taken(void) { return g_taken.path[1].item_scatter; }
void enc_record_backward(const EncBwdOut& out) { g_taken.path[1].item_scatter = out.item_scatter_taken ? 1 : 0; }
extern "C" int ps_enc_path_taken(int32_t backward, PsEncPath* out) {
  PS_REQUIRE(out, "enc_path_taken: null argument");
  *out = enc_taken(backward);
  return PS_OK;
}

int enc_layers_forward(const EncCall& c, const EncFwdOpts& o) {
  const PsTemDesc& D = c.D; const PsTemTensors& P = c.P; float* ws = c.ws; const Ws& w = c.w; hipStream_t st = c.st;
  const int d = D.d, S = w.S, NL = D.n_layers;
  const EncPlan& pl = c.plan;
  enc_taken_clear(0, NL);
  PsEncPath& tk = enc_taken(0);
  for (int i = 0; i < NL; ++i) {
    const LayerWs& l = w.layer[i];
    const PsLayerTensors& Lp = P.layer[i];
    PS_REQUIRE(Lp.wk && Lp.wv && Lp.wq && Lp.wo && Lp.w1 && Lp.w2 && Lp.bk && Lp.bv && Lp.bq && Lp.bo && Lp.b1 &&
               Lp.b2 && Lp.ff_ln_g && Lp.ff_ln_b, "forward: layer %d has null tensors", i);
    const float* xin = i == 0 ? ws + w.x : ws + w.layer[i - 1].y2;
    const int ns = l.n_in * S;
    if (i != 0) {   // pre-LayerNorm only when iter != 0 (transformer.py:48-51)
      PS_REQUIRE(Lp.ln_g && Lp.ln_b, "forward: layer %d null pre-LN", i);
      LnFwdArgs a = {xin, d, ws + l.xn, d, ws + l.pre_stats, Lp.ln_g, Lp.ln_b, ns, d, 1e-6f};
      TRY(launch_ln_fwd(a, st));
    }
    const float* xn = ws + l.xn;
    AttnArgs a = attn_shape(D, w, i, c.ui, c.valid);
    a.kp = ws + l.kp; a.vp = ws + l.vp; a.qp = ws + l.qp; a.attn = ws + l.attn; a.ctx = ws + l.ctx;
    a.drop = make_drop(D, PS_SITE_ATTN(i));
    uint32_t* amask = reinterpret_cast<uint32_t*>(ws + l.amask);
    if (pl.attn[i] == ATTN_KVQ) {
      const WSplit& kvs = c.x3;
      KvqArgs q;
      memset(&q, 0, sizeof(q));
      if (o.split_bwd_left) q.split = kvs;           // the backward-only streams, left out of the embed launch (encode_forward)
      q.at = a; q.x = xn; q.kv_stream = kvs.fwd_kv;
      q.bk = Lp.bk; q.bv = Lp.bv; q.wq = Lp.wq; q.bq = Lp.bq;
      q.kp = ws + l.kp; q.vp = ws + l.vp; q.qp = ws + l.qp; q.amask = amask;
      if (pl.front_fused) {                          // ... and the embed launch's work (its caller did not launch it)
        q.wkv[0] = Lp.wk; q.wkv[1] = Lp.wv;
        TRY(launch_front_attn_fwd(q, *o.front, st));
        g_taken.front = 1;
      } else TRY(launch_kvq_attn_fwd(q, st));
      tk.attn[i] = ATTN_KVQ; tk.rowlist = 1;         // (its workgroups project their sequence's valid positions only)
    } else {   // K, V, Q projections (neural.py:192-197), Q pre-divided by sqrt(dh) (:206)
      GemmGroup g;
      memset(&g, 0, sizeof(g));
      g.n = 3;
      g.p[0] = gp(xn, d, 0, Lp.wk, d, 0, ws + l.kp, d, ns, d, d); g.p[0].bias = Lp.bk;
      g.p[1] = gp(xn, d, 0, Lp.wv, d, 0, ws + l.vp, d, ns, d, d); g.p[1].bias = Lp.bv;
      if (l.Sq == S) g.p[2] = gp(xn, d, 0, Lp.wq, d, 0, ws + l.qp, d, ns, d, d);
      else g.p[2] = gp(xn + (size_t)w.qpos * d, S * d, 0, Lp.wq, d, 0, ws + l.qp, d, l.n_in, d, d);
      g.p[2].bias = Lp.bq; g.p[2].alpha = a.qscale;
      // valid rows only (EmbedArgs::vrows): the K / V rows of padded positions are never read (sq1_load zero-fills them)
      if (pl.rowlist) {
        const int32_t* vr = reinterpret_cast<const int32_t*>(ws + w.vrows);
        const int32_t* vc = reinterpret_cast<const int32_t*>(ws + w.vcount);
        g.p[0].ridx = vr; g.p[0].rcount = vc;
        g.p[1].ridx = vr; g.p[1].rcount = vc;
        tk.rowlist = 1;
      }
      TRY(ps_launch_gemm(g, st));
      switch (pl.attn[i]) {
        case ATTN_WF: TRY(launch_attn_fwd_wf(a, amask, st)); tk.attn[i] = ATTN_WF; break;
        case ATTN_W1: TRY(launch_attn_fwd_w1(a, st)); tk.attn[i] = ATTN_W1; break;
        case ATTN_SQ1: TRY(launch_attn_fwd_sq1(a, st)); tk.attn[i] = ATTN_SQ1; break;
        default: TRY(launch_attn_fwd(a, st)); tk.attn[i] = ATTN_GENERIC;
      }
    }
    const bool fuse = pl.fwd_fuse_last && i == NL - 1;
    PS_REQUIRE(!o.fold_sc || fuse || i != NL - 1, "forward: folded scoring without the fused last layer");   // (earlier layers: never fused)
    TRY(enc_tail_forward(c, c.x3, i, xin, fuse, fuse ? o.fold_sc : nullptr));
    if (fuse) { tk.fwd_fuse_last = 1; tk.fold_score = o.fold_sc ? 1 : 0; }
  }
  if (pl.fwd_fuse_last) return PS_OK;
  return enc_final_ln_forward(c);
}

// park the {dgamma, dbeta, colsum} column sums of one LN backward (see ColFoldList) when the caller collects them
static float* park(ColFoldList* fold, float* partial, int nblk, int d, float* g0, float* g1, float* g2) {
  ColFold& f = fold->e[fold->n++];
  f.partial = partial; f.nblk = nblk; f.d = d;
  f.dst[0] = g0; f.dst[1] = g1; f.dst[2] = g2;
  return partial;
}
static void park_colsums(LnBwdArgs& a, float* ws, const Ws& w, ColFoldList* fold) {
  if (!fold || fold->n >= PS_MAX_COLFOLD) return;
  a.partial = park(fold, ws + w.lnpart + (size_t)fold->n * w.lnrows * 3 * a.d, ln_bwd_blocks(a.rows), a.d, a.dgamma, a.dbeta, a.colsum);
}

// `kvs`: make_wsplit's answer for the call (fwd_kv / bwd_kv: one-layer encoders only)
static EncPlan enc_plan(const PsTemDesc& D, const PsTemTensors& P, const Ws& w, const WSplit& kvs, bool rows_listed, const float* valid) {
  const EncSwitches& sw = enc_switches();
  EncPlan pl;
  memset(&pl, 0, sizeof(pl));
  const int NL = D.n_layers, d = D.d, S = w.S;
  if (D.model != PS_MODEL_TEM || NL < 1) return pl;
  AttnArgs a0;                                           // (ends as layer 0's)
  for (int i = NL - 1; i >= 0; --i) {
    a0 = attn_shape(D, w, i, nullptr, valid);
    pl.attn[i] = !attn_sq1_fits(a0) ? ATTN_GENERIC : a0.fan > 1 && attn_wf_fits(a0) ? ATTN_WF : attn_w1_fits(a0) ? ATTN_W1 : ATTN_SQ1;
  }
  const LayerWs& l0 = w.layer[0];
  const LayerWs& ll = w.layer[NL - 1];
  const bool sq1 = pl.attn[0] != ATTN_GENERIC, wf = pl.attn[0] == ATTN_WF, w1 = wf || pl.attn[0] == ATTN_W1;
  const bool qall = l0.Sq == S;
  pl.rowlist = sw.rows_on && rows_listed && NL == 1 && w.qpos == 0 && w.vrows != 0 && l0.n_in == D.B && sq1;
  // One layer, replicas, d = 128: projections + attention of the one consumed position in ONE launch, a workgroup per
  // sequence (kvq_attn_fwd_kernel): the K / V weight fragments were re-split by the embed launch in front (WSplit::fwd_kv)
  // (the streams must exist either way: ps_set_front_fused can restore that launch from one call to the next)
  if (NL == 1 && kvs.on && kvs.fwd_kv && ps_fusion_enabled() && pl.rowlist && wf && kvq_attn_fits(a0) && l0.amask) pl.attn[0] = ATTN_KVQ;
  // ... and the embed launch in front of it as well (front_attn_fwd_kernel): FS query encoder (projected in the launch), positional
  // rows, at most PS_FRONT_MAX_Q query words; the AVG encoder and longer queries keep the two launches
  pl.front_fused = pl.attn[0] == ATTN_KVQ && sw.front_fused != 0 && D.query_encoder == PS_QENC_FS && D.use_pos_emb &&
                   D.Q >= 1 && D.Q <= PS_FRONT_MAX_Q && P.fs_w && P.fs_b && P.pe && kvs.bwd_kv;
  const bool last_fusable = ps_fusion_enabled() && ll.Sq == 1 && mlp_fused_serves(d, D.F) && w.wsplit;
  pl.fwd_fuse_last = last_fusable && P.final_ln_g && P.final_ln_b;
  // Folded scoring (ScoreArgs): TEM training forward with replicas whose last layer takes the wave-specialised fused form
  pl.fold_score = pl.fwd_fuse_last && D.C == 0 && w.R == D.K + 1 && w.R >= 2 && D.W >= 1 && ll.M2 == w.Mf &&
                  mlp_fwd_can_fold_score(w.Mf, D.F, d);
  EncPlan::Bwd& b = pl.bwd;
  // The last layer's whole per-replica backward (final LN, FFN, FF LN, Wo) as one kernel (mlp_fused.hip) when the
  // forward took the fused form too; needs parked column sums (fold) and one parked row per workgroup (Ws::lnrows of them).
  b.fuse_last = last_fusable && sw.bwd_fuse_on && ll.M2 == w.Mf && w.Mf >= sw.fuse_bwd_min && mlp_bwd_fused_blocks(w.Mf) <= w.lnrows;
  b.item_scatter = b.fuse_last && sw.item_scatter_fused != 0 && !ps_deterministic();
  b.wg3_main = b.fuse_last && sw.wg3_main_on && ll.n_in * S <= 2 * ll.M2;   // (review transformer: 78k K/V rows vs 1.5k replica rows -> side)
  b.wg3_last = b.wg3_main && sw.wg3_last && NL == 1;
  b.wgrad_early = sw.wgrad_early;
  // first layer, one query row per sequence, d == 128: dQ.Wq rides in the attention backward's tail (two partial
  // rows per sequence in the free d ln1 buffer) instead of a [n_in,128]x[128,128] GEMM launch of its own
  b.q_folded = sq1 && !qall && ps_fusion_enabled() &&
               (w1 ? (!wf || d == 128) && (size_t)(wf ? 2 : 1) * l0.n_in <= (size_t)l0.M2
                   : d == 128 && attn_sq1_split(a0) == 2 && (size_t)2 * l0.n_in <= (size_t)l0.M2);
  // valid rows only: padded positions have exactly-zero dK / dV rows (their attention weights are 0), never read and never
  // written: the K/V weight gradients (and the dX product) run over the batch's row list instead of all n_in*S rows
  b.listed = pl.rowlist && !qall;
  // ... and, one-layer encoder with replicas: so does the K / V input gradient itself (AttnArgs::kvb_stream) — no dX GEMM launch
  // on the dependent chain; the embed scatter adds the two head groups' partial rows (EmbedBwdArgs::dx2)
  // (FS query encoder only: its fused backward reads d query_emb as the two partials; the AVG branch copies one row of dx)
  b.dx_fused = sw.dx_fused_on && wf && b.q_folded && b.listed && d == 128 && kvs.on && kvs.bwd_kv && !ps_deterministic() &&
               attn_bwd_wf_two_partials(a0) && D.query_encoder == PS_QENC_FS;
  // round 4: where dQ.Wq is NOT folded (d != 128: the C5 shard) the replicas' fan-in is summed by a launch of its own
  // (launch_fanin_sum) so that the dX product can still run over the row list: 133 -> ~50 us at C5
  b.presum = b.listed && !b.q_folded && l0.fan > 1 && (d % 4) == 0;
  return pl;
}

EncCall enc_call(const EncBase& b, const int64_t* ui, const float* valid, bool rows_listed) {
  EncCall c = {b, ui, valid, rows_listed, {}, make_wsplit(b.D, b.P, b.ws, b.w)};
  c.plan = enc_plan(b.D, b.P, b.w, c.x3, rows_listed, valid);
  return c;
}

// What the three sequences of the encoder backward share: the call, the gradients, the caller's options and what it gets back
struct EncBwd : EncCall {
  const PsTemTensors& G; const EncBwdIn& in; EncBwdOut& out;
  bool drop() const { return D.training && D.dropout > 0.f; }
  const float* do2() const { return drop() ? ws + w.do2 : ws + w.dy2; }     // d y2 behind the FF2 dropout
  const float* dout() const { return drop() ? ws + w.do_ : ws + w.dy1; }    // d y1 behind the context dropout
  GemmProblem wgrad_w2(int i) const { return gp_wgrad(do2(), D.d, ws + w.layer[i].h1, D.F, G.layer[i].w2, D.d, D.F, w.layer[i].M2); }
  GemmProblem wgrad_w1(int i) const { return gp_wgrad(ws + w.da1, D.F, ws + w.layer[i].ln1, D.d, G.layer[i].w1, D.F, D.d, w.layer[i].M2); }
  GemmProblem wgrad_wo(int i) const { return gp_wgrad(dout(), D.d, ws + w.layer[i].ctx, D.d, G.layer[i].wo, D.d, D.d, w.layer[i].M2); }
};

// The last layer's per-replica backward as one kernel: final LN, FFN, FF LN, Wo (EncPlan::Bwd::fuse_last).  `score`: d enc from
// the scores inside the kernel, the rest of the score backward placed here.
static int bwd_fused_last(const EncBwd& c, const ScoreArgs* score) {
  const PsTemDesc& D = c.D; const Ws& w = c.w; float* ws = c.ws; hipStream_t st = c.st;
  const int i = D.n_layers - 1, d = D.d, F = D.F, M2 = w.layer[i].M2;
  const LayerWs& l = w.layer[i];
  const PsLayerTensors& Lp = c.P.layer[i];
  const PsLayerTensors& Lg = c.G.layer[i];
  ColFoldList* fold = c.in.fold;
  PS_REQUIRE(fold && fold->n + 3 <= PS_MAX_COLFOLD, "backward: the fused last layer parks three column sums with its caller");
  MlpBwdArgs m;
  memset(&m, 0, sizeof(m));
  m.M = M2; m.F = F;
  m.denc = ws + w.denc; m.y2 = ws + l.y2; m.stf = ws + w.fin_stats; m.gf = c.P.final_ln_g;
  m.y1 = ws + l.y1; m.st1 = ws + l.ff_stats; m.g1 = Lp.ff_ln_g; m.a1 = ws + l.a1;
  m.wo = Lp.wo; m.w1 = Lp.w1; m.w2 = Lp.w2;
  m.drop_ctx = make_drop(D, PS_SITE_CTX(i)); m.drop_ff1 = make_drop(D, PS_SITE_FF1(i));
  m.drop_ff2 = make_drop(D, PS_SITE_FF2(i));
  if (score) {   // d enc from the scores (see MlpBwdArgs::item_scores)
    const ScoreArgs& sa = *score;
    m.item_scores = sa.item_scores; m.target = sa.target; m.neg_items = sa.neg_items; m.product_emb = sa.product_emb;
    m.B = sa.B; m.K = sa.K; m.pos_weight = sa.pos_weight; m.P = sa.P; m.scale = sa.scale; m.scale_dev = sa.scale_dev;
    if (c.plan.bwd.item_scatter && c.in.caller_flushes_tail && sa.part == 0 && sa.enc && sa.g_product_emb) {
      m.enc = sa.enc; m.g_product_emb = sa.g_product_emb;
      m.g_product_bias = sa.bias_product ? sa.g_product_bias : nullptr;
    }
  }
  m.x3 = c.x3;                                       // the fragment streams the forward's embed launch left in the workspace
  m.do2 = const_cast<float*>(c.do2()); m.da1 = ws + w.da1; m.dy1 = ws + w.dy1;
  m.dout = const_cast<float*>(c.dout()); m.dctx = ws + w.dctx;
  const int nwg = mlp_bwd_fused_blocks(M2);
  // parked column sums: {final LN gamma, beta, b2}, {FF LN gamma, beta, bo}, {b1}
  m.part_f = park(fold, ws + w.lnpart + (size_t)fold->n * w.lnrows * 3 * d, nwg, d, c.G.final_ln_g, c.G.final_ln_b, Lg.b2);
  m.part_1 = park(fold, ws + w.lnpart + (size_t)fold->n * w.lnrows * 3 * d, nwg, d, Lg.ff_ln_g, Lg.ff_ln_b, Lg.bo);
  m.part_b1 = park(fold, ws + w.gcpart, mlp_bwd_b1_rows(M2, F), F, Lg.b1, nullptr, nullptr);
  // (measured and dropped: the table scatter of the score backward — it needs nothing of this backward — started beside
  // the fused kernel below, its fork carried by that kernel: starved by 252 workgroups that own their CUs' LDS it took
  // 74 us instead of 29 and slowed the attention backward behind it, 0.278 -> 0.282 ms/step)
  TRY(launch_mlp_bwd_fused(m, st));
  enc_taken(1).bwd_fuse_last = 1;
  TRY(side_fork(st));                           // fork 1: W2, W1, Wo weight gradients under the attention backward
  if (score && m.g_product_emb) {
    // the fused kernel above has added the item rows: what is left of the score backward are its word tasks (2 B workgroups,
    // 14 us alone at C2).  Leading the side stream, as the whole scatter does below, they only moved the W2 / W1 / Wo group
    // into the attention backward and the embedding scatter (42 -> 52-58 us, the side stream still the last to end: a wash);
    // the caller launches them as the main stream's LAST kernel instead, behind its K / V / Q weight gradients — the main
    // stream ended 12 us before the side stream, which now carries the group alone, and the join's value is there when the
    // main stream arrives (C2 0.2133 -> 0.2067 ms/step, profiles/item_scatter_fused_notes.md)
    c.out.score_words_last = true;
    c.out.item_scatter_taken = true;
  } else if (score) {                           // ... led by the table scatter of the score backward (behind them instead: 0.284 -> 0.293 ms/step)
    ScoreArgs t = *score;
    t.denc = nullptr;
    TRY(launch_score_bwd(t, side_stream_or(st)));
  }
  // (a second side stream for W1 / Wo beside W2 measured 0.389 vs 0.368 ms: slower)
  // one launch for the three (the flat group form: every member keeps its own split count; three launches of ~250
  // latency-bound workgroups one after the other took 86 us at C2; review transformer 0.563 -> 0.543 ms/step, C2 0.3156 ->
  // 0.3144).  PS_WGRAD_GROUP_ROWS=0 restores the separate launches.
  static const int wg_group_rows = ps_diag_int("PS_WGRAD_GROUP_ROWS", (1 << 30));
  GemmProblem all3[3] = {c.wgrad_w2(i), c.wgrad_w1(i), c.wgrad_wo(i)};
  if (M2 <= wg_group_rows) return side_run(all3, 3, st);
  for (int q = 0; q < 3; ++q) TRY(side_run(all3 + q, 1, st));
  return PS_OK;
}

// Layer i's FFN, FF LayerNorm and Wo backward as launches of their own: d y2 -> d ctx
static int bwd_ffn(const EncBwd& c, int i) {
  const PsTemDesc& D = c.D; const Ws& w = c.w; float* ws = c.ws; hipStream_t st = c.st;
  const int d = D.d, F = D.F, M2 = w.layer[i].M2;
  const LayerWs& l = w.layer[i];
  const PsLayerTensors& Lp = c.P.layer[i];
  const PsLayerTensors& Lg = c.G.layer[i];
  ColFoldList* fold = c.in.fold;
  GemmProblem p = gp(c.do2(), d, 0, Lp.w2, F, 1, ws + w.da1, F, M2, F, d);      // d h1 = do2 . W2
  p.act = ACT_GELU_BWD; p.act_aux = ws + l.a1; p.drop = make_drop(D, PS_SITE_FF1(i)); p.colsum = Lg.b1;
  if (fold && fold->n < PS_MAX_COLFOLD && i == D.n_layers - 1)      // park the b1 column sums (one buffer: last layer only)
    p.colsum_part = park(fold, ws + w.gcpart, 4 * ps_cdiv(M2, 64), F, Lg.b1, nullptr, nullptr);
  TRY(run1(p, st));
  // dW2 += do2^T . h1 and dW1 += da1^T . ln1 are launched further down, once the dX chain of the MLP is through
  // (beside it they slowed every link: 44 vs 33 us for the GEMM below); they then share the machine with the
  // attention backward and the big dX GEMM instead.  Measured a wash in step time (both orders 0.509 ms): the
  // backward is throughput-bound once both streams are busy.
  GemmProblem wg[1] = {c.wgrad_w2(i)};
  GemmProblem wg1[1] = {c.wgrad_w1(i)};
  GemmProblem q = gp(ws + w.da1, F, 0, Lp.w1, d, 1, ws + w.dln1, d, M2, d, F);  // d ln1 = da1 . W1
  TRY(run1(q, st));
  // fork 1: the two big weight gradients (W2, W1) start as soon as d a1 exists, under the LN backward, the Wo dX
  // GEMM and the attention backward.  (Forked one GEMM later, behind d ctx, the side stream's 112 us of weight
  // gradients ended 13 us after the main chain and the step paid a late join on top.)
  if (c.plan.bwd.wgrad_early) {
    TRY(side_fork(st));
    TRY(side_run(wg, 1, st));
    TRY(side_run(wg1, 1, st));
    enc_taken(1).wgrad_early = 1;
  }
  LnBwdArgs n;
  memset(&n, 0, sizeof(n));
  n.dy = ws + w.dln1; n.lddy = d; n.x = ws + l.y1; n.ldx = d; n.stats = ws + l.ff_stats; n.g = Lp.ff_ln_g;
  n.rows = M2; n.d = d;
  n.res.mode = RES_DIRECT; n.res.ptr = ws + w.dy2; n.res.ld = d;            // residual  output + x
  n.dx = ws + w.dy1; n.lddx = d;
  if (c.drop()) { n.out2 = ws + w.do_; n.drop2 = make_drop(D, PS_SITE_CTX(i)); }
  n.colsum = Lg.bo; n.dgamma = Lg.ff_ln_g; n.dbeta = Lg.ff_ln_b;
  park_colsums(n, ws, w, fold);
  TRY(launch_ln_bwd(n, st));
  GemmProblem pc = gp(c.dout(), d, 0, Lp.wo, d, 1, ws + w.dctx, d, M2, d, d);    // d ctx = do . Wo
  TRY(run1(pc, st));
  if (!c.plan.bwd.wgrad_early) {
    GemmProblem wgo[1] = {c.wgrad_wo(i)};
    TRY(side_fork(st));                         // fork 1 (late form): W2, W1, Wo weight gradients under the attention backward
    TRY(side_run(wg, 1, st));
    TRY(side_run(wg1, 1, st));
    TRY(side_run(wgo, 1, st));
  }
  return PS_OK;
}

// Layer i's attention backward, the K / V / Q weight gradients and the input gradient d xn = dK.Wk + dV.Wv (+ dQ.Wq).
// `fused`: bwd_fused_last ran in front (the side stream holds W2 / W1 / Wo), not bwd_ffn.
static int bwd_attention(const EncBwd& c, int i, bool fused) {
  const PsTemDesc& D = c.D; const Ws& w = c.w; float* ws = c.ws; hipStream_t st = c.st;
  const EncPlan::Bwd& pb = c.plan.bwd;
  const int d = D.d, S = w.S;
  const LayerWs& l = w.layer[i];
  const PsLayerTensors& Lp = c.P.layer[i];
  const PsLayerTensors& Lg = c.G.layer[i];
  const float* xn = ws + l.xn;
  const int ns = l.n_in * S;
  ColFoldList* fold = c.in.fold;
  AttnArgs a = attn_shape(D, w, i, c.ui, c.valid);
  a.kp = ws + l.kp; a.vp = ws + l.vp; a.qp = ws + l.qp; a.attn = ws + l.attn;
  a.drop = make_drop(D, PS_SITE_ATTN(i));
  a.dctx = ws + w.dctx;
  const bool qall = l.Sq == S;
  a.lddkv = qall ? 3 * d : 2 * d;
  a.dkv = ws + w.dkv;
  a.dq = qall ? ws + w.dkv + 2 * d : ws + w.dq;
  a.lddq = qall ? 3 * d : d;
  a.dbq = Lg.bq; a.dbk = Lg.bk; a.dbv = Lg.bv;
  const AttnForm form = c.plan.attn[i];
  const bool wf = form == ATTN_WF || form == ATTN_KVQ;   // one wave per (sequence, four heads), replicas inside
  const bool w1 = wf || form == ATTN_W1;                 // one wave per sequence (no replicas)
  if (form != ATTN_GENERIC && fold && fold->n < PS_MAX_COLFOLD)   // bias gradients: one parked row per sequence instead of n_in same-address atomics per column
    a.bias_part = park(fold, ws + w.abpart + (size_t)i * w.layer[D.n_layers - 1].n_in * 3 * d, l.n_in, d, Lg.bq, Lg.bk, Lg.bv);
  // the first layer's forms (EncPlan::Bwd); listed / presum / dx_fused: one-layer encoders only
  const bool q_folded = i == 0 && pb.q_folded, listed = pb.listed, presum = pb.presum, dx_fused = pb.dx_fused;
  PsEncPath& tk = enc_taken(1);
  if (q_folded) { a.wq = Lp.wq; a.dxq_part = ws + w.dln1; a.fanin_src = ws + w.dy1; tk.q_folded = 1; }
  if (dx_fused) { a.kvb_stream = c.x3.bwd_kv; a.dxp[0] = ws + w.dx; a.dxp[1] = ws + w.dxn; tk.dx_fused = 1; }
  c.out.dx_two_partials = dx_fused;
  const bool pads_unread = listed && (q_folded || l.fan == 1 || presum);
  if (wf) {
    bool key_split = false;
    TRY(launch_attn_bwd_wf(a, reinterpret_cast<const uint32_t*>(ws + l.amask), pads_unread, st, &key_split));
    tk.attn[i] = ATTN_WF; tk.wf_key_split = key_split ? 1 : 0;
  } else if (w1) {
    TRY(launch_attn_bwd_w1(a, pads_unread, st));
    tk.attn[i] = ATTN_W1;
  } else if (form == ATTN_SQ1) {
    TRY(launch_attn_bwd_sq1(a, st));
    tk.attn[i] = ATTN_SQ1;
  } else {
    TRY(launch_attn_bwd(a, st));
    tk.attn[i] = ATTN_GENERIC;
  }
  // weight gradients of Wo, Wk, Wv, Wq: one fork right behind the attention backward, off the dX chain
  GemmProblem wg3[3];
  wg3[0] = gp_wgrad(ws + w.dkv, a.lddkv, xn, d, Lg.wk, d, d, ns);
  wg3[1] = gp_wgrad(ws + w.dkv + d, a.lddkv, xn, d, Lg.wv, d, d, ns);
  if (qall) wg3[2] = gp_wgrad(ws + w.dkv + 2 * d, a.lddkv, xn, d, Lg.wq, d, d, ns);
  else wg3[2] = gp_wgrad(ws + w.dq, d, xn + (size_t)w.qpos * d, S * d, Lg.wq, d, d, l.n_in);
  // first layer, one query row per sequence: dQ.Wq is a [n_in, d] product whose rows join the big dX GEMM below
  // through its fan-in epilogue — computed here, before the weight gradients start competing for the CUs
  // (as a trailing accumulate-GEMM it took 26 us on the critical path under them)
  const bool q_via_res = !qall && i == 0;
  float* dxq = ws + w.dctx;                      // free again: the attention backward has consumed it
  if (q_via_res && !q_folded) {
    GemmProblem xq = gp(ws + w.dq, d, 0, Lp.wq, d, 1, dxq, d, l.n_in, d, d);
    xq.no_deep = 1;   // runs beside the side stream's weight gradients (at C5 the deep form waited 110 us for whole CUs)
    TRY(run1(xq, st));
  }
  // fork 2: they need the attention backward's dK / dV / dQ.  With the fused backward the side stream already
  // holds W2 / W1 / Wo (~90 us, the step's tail): the K/V/Q weight gradients then follow the dX GEMM on the MAIN
  // stream instead — one event less, and the side stream ends before the scatter does.
  // (round 2: W2 / W1 / Wo are ONE launch of ~45 us now, the side stream is free again when the attention backward
  // ends: the K / V / Q weight gradients go back to it, 0.3151 -> 0.3124 ms/step; PS_WG3_SIDE=0: main stream)
  // (later in round 2: with forks signalled by the next kernel the main stream lost its two bubbles and ENDED 30 us before
  // the side stream — score scatter 28 + W2/W1/Wo 45 + these 16 us; back on the main stream: 0.2861 -> 0.2801 ms/step)
  const bool wg3_main = fused && pb.wg3_main;
  const int32_t* vr = reinterpret_cast<const int32_t*>(ws + w.vrows);
  const int32_t* vc = reinterpret_cast<const int32_t*>(ws + w.vcount);
  if (listed) {
    wg3[0].ridx = vr; wg3[0].rcount = vc;
    wg3[1].ridx = vr; wg3[1].rcount = vc;
    tk.listed = 1;
  }
  if (!wg3_main) {
    TRY(side_fork(st));
    TRY(side_run(wg3, 3, st));
  }
  if (pb.wgrad_early && !fused) {
    GemmProblem wgo[1] = {c.wgrad_wo(i)};
    TRY(side_run(wgo, 1, st));
  }
  // d xn = dK.Wk + dV.Wv (+ dQ.Wq)
  float* dxn = i == 0 ? ws + w.dx : ws + w.dxn;
  GemmProblem x = gp(ws + w.dkv, a.lddkv, 0, Lp.wk, d, 1, dxn, d, ns, d, qall ? 3 * d : 2 * d);
  x.kseg = d; x.Bseg[1] = Lp.wv; x.Bseg[2] = Lp.wq;
  if (i == 0) {   // + residual path of `out = dropout(context) + inputs`, summed over the replicas
    x.res.mode = RES_FANIN; x.res.ptr = ws + w.dy1; x.res.ld = d; x.res.Sq = l.Sq; x.res.fan = l.fan;
    x.res.S = S; x.res.qpos = w.qpos; res_finish(x.res);
    if (q_folded) {   // both partial rows already hold the replicas' fan-in sum: nothing left to walk here
      x.res.extra = ws + w.dln1; x.res.extra2 = (w1 && !(wf && attn_bwd_wf_two_partials(a))) ? nullptr : ws + w.dln1 + (size_t)l.n_in * d; x.res.extra_ld = d; x.res.ptr = nullptr;
    }
    else if (q_via_res) { x.res.extra = dxq; x.res.extra_ld = d; }
    if (presum) {   // fan-in summed up front: one row per sequence beside the dQ.Wq row, nothing to walk
      float* fsum = ws + w.dln1;          // (free: the FF LayerNorm backward has consumed d ln1)
      TRY(launch_fanin_sum(ws + w.dy1, d, l.n_in, l.fan, d, fsum, st));
      tk.presum = 1;
      x.res.ptr = nullptr; x.res.extra = dxq; x.res.extra2 = fsum; x.res.extra_ld = d;
    }
  }
  // (the dX product over the row list only when its fan-in residual is already folded: walking 21 replica rows per
  // query row in a third of the workgroups made it slower than the dense form — 144 vs 106 us at C5)
  if (pads_unread) { x.ridx = vr; x.rcount = vc; }
  if (!dx_fused) TRY(run1(x, st));
  if (wg3_main) {
    tk.wg3_main = 1;
    if (pb.wg3_last && c.in.caller_flushes_tail) { for (int q = 0; q < 3; ++q) c.out.wg3_last[q] = wg3[q]; c.out.wg3_last_n = 3; tk.wg3_last = 1; }
    else TRY(run_wgrads(wg3, 3, st));
  }
  if (!qall && !q_via_res) {
    GemmProblem xq = gp(ws + w.dq, d, 0, Lp.wq, d, 1, dxn + (size_t)w.qpos * d, S * d, l.n_in, d, d);
    xq.accumulate = 1;
    TRY(run1(xq, st));
  }
  return PS_OK;
}

int enc_layers_backward(const EncCall& call, const PsTemTensors& G, const EncBwdIn& in, EncBwdOut& out) {
  const PsTemDesc& D = call.D; const PsTemTensors& P = call.P; float* ws = call.ws; const Ws& w = call.w; hipStream_t st = call.st;
  const int B = D.B, d = D.d, S = w.S, NL = D.n_layers;
  PS_REQUIRE(G.final_ln_g && G.final_ln_b, "backward: null final LayerNorm gradient");
  out = EncBwdOut();
  enc_taken_clear(1, NL);
  const EncBwd c = {call, G, in, out};
  const bool fuse_last = c.plan.bwd.fuse_last;
  side_set_light((int64_t)B * S * d <= ((int64_t)2 << 20));   // C2: 1.03 M elements of x; review transformer 10 M; C5 5.5 M
  const ScoreArgs* score_fused = fuse_last && w.R > 1 ? in.score_on_side : nullptr;
  if (in.score_on_side && !score_fused) {
    // not the fused form: d enc is needed first, so the score backward is cut in two — its d enc half leads the main
    // stream, its table scatter (the expensive half: 127 us of scattered atomics at C5) goes to the side stream
    ScoreArgs t = *in.score_on_side;
    t.denc = ws + w.denc;
    const hipStream_t side = side_stream_or(st);
    if (side != st && w.R > 1) {
      t.part = 1;
      TRY(launch_score_bwd(t, st));
      TRY(side_fork(st));
      t.part = 2;
      TRY(launch_score_bwd(t, side));
    } else {
      TRY(launch_score_bwd(t, st));
    }
  }
  if (!fuse_last) {   // 2. final LayerNorm backward (fused form: inside the last layer's kernel)
    LnBwdArgs f;
    memset(&f, 0, sizeof(f));
    f.dy = ws + w.denc; f.lddy = d; f.stats = ws + w.fin_stats; f.g = P.final_ln_g; f.d = d;
    f.dgamma = G.final_ln_g; f.dbeta = G.final_ln_b;
    if (NL > 0) {
      const LayerWs& l = w.layer[NL - 1];
      f.x = ws + l.y2; f.ldx = d; f.rows = w.Mf; f.dx = ws + w.dy2; f.lddx = d;
      f.colsum = G.layer[NL - 1].b2;
      if (c.drop()) { f.out2 = ws + w.do2; f.drop2 = make_drop(D, PS_SITE_FF2(NL - 1)); }
    } else {
      PS_CHECK_HIP(hipMemsetAsync(ws + w.dx, 0, sizeof(float) * (size_t)B * S * d, st));
      f.x = ws + w.x + (size_t)w.qpos * d; f.ldx = S * d; f.rows = B;
      f.dx = ws + w.dx + (size_t)w.qpos * d; f.lddx = S * d;
    }
    park_colsums(f, ws, w, in.fold);
    TRY(launch_ln_bwd(f, st));
  }
  // 3. layers, last to first
  for (int i = NL - 1; i >= 0; --i) {
    const LayerWs& l = w.layer[i];
    const PsLayerTensors& Lp = P.layer[i];
    const PsLayerTensors& Lg = G.layer[i];
    PS_REQUIRE(Lg.wk && Lg.wv && Lg.wq && Lg.wo && Lg.w1 && Lg.w2 && Lg.bk && Lg.bv && Lg.bq && Lg.bo && Lg.b1 &&
               Lg.b2 && Lg.ff_ln_g && Lg.ff_ln_b, "backward: layer %d has null gradients", i);
    const bool fused = fuse_last && i == NL - 1;
    if (fused) TRY(bwd_fused_last(c, score_fused));
    else TRY(bwd_ffn(c, i));
    TRY(bwd_attention(c, i, fused));
    if (i != 0) {   // pre-LayerNorm backward -> grad wrt the previous layer's output
      TRY(side_join(st));   // the next layer reuses the scratch buffers the side-stream GEMMs read
      PS_REQUIRE(Lg.ln_g && Lg.ln_b, "backward: layer %d null pre-LN gradient", i);
      LnBwdArgs n;
      memset(&n, 0, sizeof(n));
      n.dy = ws + w.dxn; n.lddy = d; n.x = ws + w.layer[i - 1].y2; n.ldx = d; n.stats = ws + l.pre_stats; n.g = Lp.ln_g;
      n.rows = l.n_in * S; n.d = d;
      n.res.mode = RES_FANIN; n.res.ptr = ws + w.dy1; n.res.ld = d; n.res.Sq = l.Sq; n.res.fan = l.fan;
      n.res.S = S; n.res.qpos = w.qpos; res_finish(n.res);
      n.dx = ws + w.dy2; n.lddx = d;
      if (c.drop()) { n.out2 = ws + w.do2; n.drop2 = make_drop(D, PS_SITE_FF2(i - 1)); }
      n.colsum = G.layer[i - 1].b2; n.dgamma = Lg.ln_g; n.dbeta = Lg.ln_b;
      park_colsums(n, ws, w, in.fold);
      TRY(launch_ln_bwd(n, st));
    }
  }
  return PS_OK;
}
