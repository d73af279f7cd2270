// encoder.h — the transformer encoder shared by the item models (tem.hip) and the review transformer (rtm.hip), implemented in
// encoder.hip: the workspace layout, the per-call context with its plan (EncCall) and the layer loops (forward / backward).
#pragma once
#include "rowwise.h"

// ------------------------------------------------------------- workspace layout
struct LayerWs {
  int n_in, fan, n_out, Sq, M2;
  int64_t xn, pre_stats, kp, vp, qp, attn, ctx, y1, ff_stats, ln1, a1, h1, y2;
  int64_t amask;            // uint32 [n_in*fan][H]: keep bits of the attention dropout (attn_fwd_wf_kernel -> its backward)
};
struct Ws {
  int R, S, Mf, qpos;
  int64_t qmean, query_emb, x;
  LayerWs layer[PS_MAX_LAYERS];
  int64_t fin_stats, enc;
  int64_t item_scores, word_scores, loss_parts, item_terms, word_terms, loss_blk;
  int64_t word_blk, item_blk, ticket;   // folded scoring (ScoreArgs): word / item loss partials, arrival counter
  int64_t wsplit;           // bf16x3 planes of the last layer's wo / w1 / w2 (WSplit), 0: not allocated
  int64_t denc, dy2, do2, da1, dln1, dy1, do_, dctx, dq, dkv, dxn, dx, dqpre, dqmean;
  int64_t lnpart;           // PS_MAX_COLFOLD x [lnrows][3][d] parked LN-backward column sums
  int lnrows;               // parked rows per entry: 256 (the LayerNorm backward's row groups) or one per 32-row workgroup of the fused backward, whichever is more
  int64_t gcpart;           // [4 * row tiles][3][F] parked column sums of the FF2 dX GEMM (b1 gradient)
  int64_t abpart;           // per layer [n_in][3][d] parked attention bias gradients {bq, bk, bv} (sq1 backward)
  int64_t vrows, vcount;    // int32 [B*S] valid-row list of x and its length (EmbedArgs::vrows), TEM only
  int64_t ae_qhalf, ae_dhalf, ae_dqe, ae_dqp, ae_dk, ae_dv, ae_part, ae_keys;   // AEM / ZAM (attn_emb.hip), 0 otherwise
  int64_t stage;            // graph replay: step word + staged copies of the call's int64 index tensors (stage_layout)
  int64_t total;
};

int make_ws(const PsTemDesc& D, Ws& w);
// the last layer's weights as the fused kernels' bf16x3 planes inside the workspace (on = 0 when the x3 form is not taken)
WSplit make_wsplit(const PsTemDesc& D, const PsTemTensors& P, float* ws, const Ws& w);
// The encoder weights a WPlaneScope (common.h) should hold for this call; returns their number (at most PS_WPLANES_MAX)
int wplane_list(const PsTemDesc& D, const PsTemTensors& P, const Ws& w, const float** ws_, int* rows, int* cols);

// ------------------------------------------------------------- one plan per call
// Which path every step of the encoder takes, decided by enc_plan (host only, no launches) from the shapes, the weights present
// and the switches.  An entry point decides it ONCE, when it builds its EncCall (below); everything under it reads that copy.
enum AttnForm {
  ATTN_GENERIC,             // any Sq (launch_attn_fwd / launch_attn_bwd)
  ATTN_SQ1,                 // one query row: a workgroup per sequence, replicas share K / V in LDS
  ATTN_W1,                  // ... no replicas: a wave per sequence
  ATTN_WF,                  // ... replicas: a wave per (sequence, four heads)
  ATTN_KVQ                  // layer 0 of a one-layer encoder: K / V / Q projections + the wf attention in one forward launch
};
struct EncPlan {
  AttnForm attn[PS_MAX_LAYERS];
  bool rowlist;             // the (one-layer) encoder walks the valid-row list: padded rows of x are read nowhere, need not be written
  bool front_fused;         // ATTN_KVQ whose launch embeds the sequences too (front_attn_fwd_kernel): no embed launch; ps_set_front_fused
  bool fwd_fuse_last;       // last layer's Wo + LN + FFN + final LN as one forward kernel (mlp_fused.hip)
  bool fold_score;          // ... whose epilogue can take item scoring + loss (ScoreArgs, folded form)
  struct Bwd {
    bool fuse_last;         // the last layer's whole per-replica backward as one kernel; needs the caller's ColFoldList
    bool item_scatter;      // ... which may scatter the item rows' gradients too (ps_set_item_scatter_fused; never deterministic)
    bool wg3_main;          // ... and whose K / V / Q weight gradients follow the dX product on the main stream
                            //     (only while the layer's K / V rows are at most twice its replica rows, n_in * S <= 2 * M2: a longer
                            //     product goes to the side stream, as the review transformer's 78k rows against 1.5k do)
    bool wg3_last;          // ... as the caller's last launches, where it flushes them (EncBwdIn::caller_flushes_tail)
    bool wgrad_early;       // unfused form: W2 / W1 weight gradients fork as soon as d a1 exists
    bool q_folded;          // layer 0: dQ.Wq rides in the attention backward's tail
    bool listed;            // one layer: dK / dV, their weight gradients and the dX product walk the valid-row list
    bool presum;            // ... with the replicas' fan-in summed by a launch of its own (dQ.Wq not folded)
    bool dx_fused;          // ... or no dX product at all: the attention backward leaves d x as two partial rows
  } bwd;
};

// ------------------------------------------------------------- one context per entry call
// EncBase: what every encoder function of a call reads.  EncCall: ... plus whose sequences these are, the plan and the weight
// split, each made once, by enc_call.  Built per entry call and never kept: the setters may change between two calls.
// enc_call dereferences neither a tensor nor ws (it reads which tensors are null and adds offsets: ps_tem_plan builds one over
// stand-ins, without a device); enc_plan (encoder.hip) has no other caller.  Besides the call it reads enc_switches() — the env /
// diag switches, read once per process, and the values ps_set_front_fused / ps_set_fuse_bwd_min / ps_set_item_scatter_fused
// write — and ps_deterministic(), each time.
struct EncBase { const PsTemDesc& D; const PsTemTensors& P; float* ws; const Ws& w; hipStream_t st; };
struct EncCall : EncBase {
  const int64_t* ui;        // key-padding mask: `valid` [n_seq, S] floats if given, else u_item_idxs != P (TEM)
  const float* valid;
  bool rows_listed;         // w.vrows / w.vcount hold the list of valid (non-pad) rows of x (EmbedArgs::vrows, or the review transformer's rtm_rowlist_kernel)
  EncPlan plan;
  WSplit x3;
};
EncCall enc_call(const EncBase& b, const int64_t* ui, const float* valid, bool rows_listed);
// What the layer loops really launched (ps_enc_path_taken): one record per direction, cleared where a direction's call starts
// and filled at the launching branches — host bookkeeping, never read by the step itself.
PsEncPath& enc_taken(int backward);
void enc_taken_clear(int backward, int n_layers);

// All encoder layers + the final LayerNorm on the consumed position: reads w.x, writes w.enc.
struct EncFwdOpts {
  const ScoreArgs* fold_sc = nullptr;  // TEM with replicas: item scoring + loss run in the epilogue of the last layer's fused kernel
  bool split_bwd_left = false;         // the embed launch left the backward-only weight streams to the fused projection + attention launch
  const EmbedArgs* front = nullptr;    // EncPlan::front_fused: the embed launch's arguments — NOT launched by the caller; layer 0's launch does its work
};
int enc_layers_forward(const EncCall& c, const EncFwdOpts& o);
// The per-replica tail of layer i behind its attention, as enc_layers_forward runs it: Wo + residual -> FF LayerNorm -> W1 -> GELU
// -> W2 + residual, reading l.ctx [l.M2, d] and the residual row (m / l.fan) * w.S + w.qpos of xin.  `fuse`: the one-kernel form of
// the LAST layer (mlp_fused.hip: needs the streams of x3 filled by an embed launch, d = 128), which also applies the final
// LayerNorm into w.enc; otherwise the caller follows with enc_final_ln_forward.  Callers: the layer loop, and the review
// transformer's full-catalogue ranking (rtm_rank.hip), whose "replicas" are the candidates of an entry and which has no plan.
int enc_tail_forward(const EncBase& b, const WSplit& x3, int i, const float* xin, bool fuse, const ScoreArgs* fold_sc);
int enc_final_ln_forward(const EncBase& b);
// Backward of enc_layers_forward: reads w.denc (grad wrt w.enc), accumulates parameter grads into G, writes w.dx.
struct EncBwdIn {
  // the LayerNorm backwards park their column sums in w.lnpart and append to this list; the caller must hand it to a later
  // launch_embed_scatter (EmbedBwdArgs::fold).  nullptr: plain atomics
  ColFoldList* fold = nullptr;
  // TEM with replicas: the caller has NOT launched the score backward; when the last layer's backward is fused, d enc is derived
  // from the scores inside that kernel and the score backward (table scatter only) is launched on the side stream behind it, off
  // the dependent chain; otherwise it is launched first, as usual
  const ScoreArgs* score_on_side = nullptr;
  bool caller_flushes_tail = false;    // the caller launches EncBwdOut's deferred work behind its embedding scatter
};
struct EncBwdOut {
  bool dx_two_partials = false;        // the attention backward left d x as two partial rows per position (dx and dxn, AttnArgs::dxp)
  // K/V/Q weight gradients of the first layer that the caller launches on the main stream AFTER its embedding scatter
  // (PS_WG3_LAST, item transformer): the scatter (atomics) then shares the machine with the side stream's W2 / W1 / Wo
  // products, and these follow when those are nearly through, instead of slowing each other down product beside product
  GemmProblem wg3_last[4]; int wg3_last_n = 0;   // (the fourth slot: the caller's own f_W weight gradient)
  bool score_words_last = false;       // ... and, when the fused backward has scattered the item rows, the score backward's word tasks behind them
  bool item_scatter_taken = false;     // the fused kernel scattered the item rows
};
void enc_record_backward(const EncBwdOut& out);   // once per backward entry point: what ps_item_scatter_fused_taken() reports (the taken record's item_scatter)
int enc_layers_backward(const EncCall& c, const PsTemTensors& G, const EncBwdIn& in, EncBwdOut& out);

// ZAM / AEM (attn_emb.hip): the attention-embedding step between the query encoder and the scoring.  ae_forward reads
// w.query_emb and writes w.enc [B*R,d]; ae_backward reads w.denc and leaves d query_emb in w.ae_dqe [B,d].
#define PS_AE_COL_SPLITS 128      // row splits of ae_backward's deterministic bias column sums (w.ae_part: [4][splits][d])
bool ps_model_attn(int model);
int ae_zoff(const PsTemDesc& D);
int ae_forward(const EncCall& c);
int ae_backward(const EncCall& c, const PsTemTensors& G);
