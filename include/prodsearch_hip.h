/*
 * prodsearch_hip.h — C ABI of libprodsearch_hip.so (MI355X / gfx950 only).
 *
 * The drop-in boundary of the ProdSearch ranking-loss training step.  The
 * reference (kepingbi/ProdSearch) is pure Python/PyTorch and has NO FFI of its
 * own; each entry point below names the reference interface it replaces
 * (file:line relative to the reference repo).  A maintainer binds them with the
 * ctypes stub shown in INTEGRATION.md (prodsearch_amd/_lib.py is that stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - indices are int64 (the reference's torch.int64 batches, data/batch_data.py:17-22),
 *     parameters/activations are fp32, row-major, nn.Linear weights are [out, in];
 *   - every call is asynchronous on `stream` (a hipStream_t), allocates nothing,
 *     synchronises nothing, and may be captured into a hipGraph;
 *   - return value: 0 = ok, otherwise an error code; ps_last_error() gives text;
 *   - no CPU fallback exists: without a gfx950 device every compute call fails.
 */
#ifndef PRODSEARCH_HIP_H
#define PRODSEARCH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PS_MAX_LAYERS 8
#define PS_OK 0
#define PS_ERR_ARG 1      /* bad descriptor / unsupported shape */
#define PS_ERR_HIP 2      /* a HIP runtime call failed          */

typedef void* ps_stream_t; /* hipStream_t */

enum { PS_MODEL_TEM = 0, PS_MODEL_QEM = 1,
       PS_MODEL_AEM = 2,   /* forward_attn / test_attn, model_name 'AEM': attention over the history only (S = L, L >= 1)     */
       PS_MODEL_ZAM = 3 }; /* 'ZAM': the same with a zero key / value row prepended, always valid (S = L + 1)                  */
/* AEM / ZAM (item_transformer.py:148-195, 361-438): attention_encoder.* (neural.py:86-96) travels in PsTemTensors.layer[0]'s
 * wk..bo (params and grads); its FFN / LayerNorm pointers, pe and the final LayerNorm are not read (NULL).  n_layers and F are
 * ignored; H heads with d / H <= 64 and H * S <= 4096.  The attention dropout is site PS_SITE_ATTN(0), element
 * (row = (b R + j) H + h, col = original key index s, ZAM's zero column s = 0) with R = K + 1 replicas when dropout is drawn. */
enum { PS_QENC_FS = 0, PS_QENC_AVG = 1 };

/* Shape/flag descriptor of one step.  Field <- reference flag (main.py:26-137). */
typedef struct PsTemDesc {
  int32_t B;             /* batch rows                         (--batch_size)            */
  int32_t K;             /* negatives per positive             (--neg_per_pos)           */
  int32_t L;             /* padded history length              (<= --uprev_review_limit) */
  int32_t Q;             /* padded query length                                          */
  int32_t W;             /* PV window                          (--pv_window_size)        */
  int32_t C;             /* candidates per row, eval only      (--candi_batch_size)      */
  int32_t d;             /* --embedding_size                                             */
  int32_t H;             /* --heads                                                      */
  int32_t F;             /* --ff_size                                                    */
  int32_t n_layers;      /* --inter_layers                                               */
  int64_t product_size;  /* P; pad index = P, tables have P+1 rows (item_transformer.py:34,46) */
  int64_t vocab_size;    /* V; pad index = V-1                    (item_transformer.py:35)     */
  int32_t model;         /* PS_MODEL_TEM: forward_dotproduct; PS_MODEL_QEM: forward_attn/QEM; PS_MODEL_AEM / _ZAM: forward_attn */
  int32_t query_encoder; /* PS_QENC_FS / PS_QENC_AVG          (--query_encoder_name)     */
  int32_t use_pos_emb;   /* --use_pos_emb                                                */
  int32_t use_item_pos;  /* --use_item_pos : output position -1 instead of 0             */
  int32_t bias_product;  /* --sim_func bias_product                                      */
  int32_t pos_weight;    /* --pos_weight : weight K on the positive's loss term          */
  int32_t sep_prod_emb;  /* --sep_prod_emb : history rows come from hist_product_emb     */
  int32_t training;      /* nn.Module.training; dropout is drawn only if set and dropout>0 */
  float   dropout;       /* --dropout                                                    */
  uint64_t seed;         /* Philox key of the dropout / sampling streams                 */
  uint64_t step;         /* Philox counter word: distinct per training step              */
} PsTemDesc;

/* One transformer layer's tensors (state_dict keys under
 * transformer_encoder.transformer_inter.{i}. — transformer.py:37-45, neural.py:20-26,86-96). */
typedef struct PsLayerTensors {
  float *wk, *bk;        /* self_attn.linear_keys   [d,d],[d] */
  float *wv, *bv;        /* self_attn.linear_values           */
  float *wq, *bq;        /* self_attn.linear_query            */
  float *wo, *bo;        /* self_attn.final_linear            */
  float *w1, *b1;        /* feed_forward.w_1 [F,d],[F]        */
  float *w2, *b2;        /* feed_forward.w_2 [d,F],[d]        */
  float *ff_ln_g, *ff_ln_b; /* feed_forward.layer_norm        */
  float *ln_g, *ln_b;    /* layer_norm (pre-LN, used only when i != 0: transformer.py:48-51) */
} PsLayerTensors;

/* A full set of model tensors.  The same struct describes parameters, their
 * gradients, and Adam moments (pointers may be NULL where the reference has no
 * gradient: product_bias unless bias_product, layer-0 ln, hist table unless sep).
 * As a gradient struct of ps_tem_backward / ps_tem_backward_step, word_emb NULL means
 * the word table is FROZEN (pretrain_emb_dir: nn.Embedding.from_pretrained, freeze=True):
 * no word-row gradient is read or written; word_bias and the other tables stay required. */
typedef struct PsTemTensors {
  float *product_emb;       /* product_emb.weight      [P+1, d] (item_transformer.py:46) */
  float *hist_product_emb;  /* hist_product_emb.weight [P+1, d] (:48) or NULL            */
  float *word_emb;          /* word_embeddings.weight  [V, d]   (:70)                    */
  float *product_bias;      /* product_bias            [P+1]    (:56)                    */
  float *word_bias;         /* word_bias               [V]      (:57)                    */
  float *fs_w, *fs_b;       /* query_encoder.f_W       [d,d],[d] (text_encoder.py:24)    */
  float *pe;                /* transformer_encoder.pos_emb.pe [5000, d] buffer (transformer.py:10-19) */
  float *final_ln_g, *final_ln_b; /* transformer_encoder.layer_norm (transformer.py:68)  */
  PsLayerTensors layer[PS_MAX_LAYERS];
} PsTemTensors;

/* The reference's ItemPVBatch (data/batch_data.py:3-37) + the two multinomial draws. */
typedef struct PsTemBatch {
  const int64_t *query_word_idxs;   /* [B,Q]   pad V-1 */
  const int64_t *target_prod_idxs;  /* [B]             */
  const int64_t *u_item_idxs;       /* [B,L]   pad P   */
  const int64_t *pos_iword_idxs;    /* [B,W]   pad V-1 */
  const int64_t *neg_item_idxs;     /* [B,K]   draw 1: torch.multinomial(prod_dists) item_transformer.py:447 */
  const int64_t *neg_word_idxs;     /* [B,W*K] draw 2: torch.multinomial(word_dists) item_transformer.py:268 */
  const int64_t *candi_prod_idxs;   /* [B,C]   eval only, pad P (item_pv_dataloader.py:44) */
} PsTemBatch;

/* Float offsets (in units of sizeof(float)) of the intermediates inside the
 * workspace; exported so the parity tests can compare every stage to the oracle.
 * Only the LAST layer's buffers are listed (n_layers == 1 covers everything). */
typedef struct PsTemWsLayout {
  int64_t total_floats;
  int32_t R;             /* encoder replicas per batch row: K+1 if dropout is drawn, else 1 */
  int32_t S;             /* L+1 (AEM: L) */
  int64_t qmean, query_emb, x;                 /* [B,d],[B,d],[B,S,d]                 */
  int64_t kp, vp, qp, attn, ctx;               /* last layer: [n_in*S,d] x2, [n_in,d].. ; K/V rows of MASKED key positions
                                                  are not written when the one-layer sq1 path is in use (row-list projection);
                                                  AEM / ZAM: K, V [B*S,d], scaled Q [B,d], softmax [B,H,S], ctx [B*R,d], and
                                                  x = the gathered key rows [B*S,d] */
  int64_t y1, ln1, a1, h1, y2, enc;            /* last layer replica rows              */
  int64_t item_scores, word_scores, loss_parts;/* [B,1+K],[B,W,1+K],[B,2]             */
  int64_t denc, dx;                            /* backward: [B*R,d], [B,S,d]           */
} PsTemWsLayout;

const char* ps_version(void);
const char* ps_last_error(void);
/* The arithmetic the step computes in, as text for bench.py's `dtype` field: "f32 (...)" naming the bf16x3 product form
 * when it is enabled (ps_gemm_x3_config).  No reference counterpart (the reference is fp32 ATen throughout). */
const char* ps_arith_info(void);
/* Tuning knob (no reference counterpart): the last encoder layer's per-replica backward runs as one fused kernel from
 * this many replica rows upwards (default 1024, env PS_FUSE_BWD_MIN; below it five short launches are as fast).  The
 * parity tests set it to 1 to drive the fused kernel through the small golden cases.  Returns the previous value. */
int ps_set_fuse_bwd_min(int rows);
/* Tuning knob (no reference counterpart): with replicas and the fused per-replica backward, that kernel adds the item rows'
 * gradients (product_emb / product_bias) itself and the score backward's launch is its word tasks only (default 1, env
 * PS_ITEM_SCATTER_FUSED; 0 = the score backward's own item workgroups).  Deterministic mode never takes the form.  Returns
 * the previous value.  ps_item_scatter_fused_taken: 1 when the last backward of this process took it. */
int ps_set_item_scatter_fused(int on);
int ps_item_scatter_fused_taken(void);
/* Tuning knob (no reference counterpart): the one-layer d = 128 forward with replicas (attention form kvq) embeds its
 * sequences inside the projection + attention launch — one launch instead of two (default 1, env PS_FRONT_FUSED; 0 = the embed
 * launch in front, as PS_KVQ_FUSED=0 implies).  FS query encoder, positional rows, at most 16 query words; anything else keeps
 * the two launches.  Returns the previous value.  ps_front_fused_taken: 1 when the last forward of this process took it (the
 * attention form stays 4 with rowlist = 1 in ps_tem_plan and ps_enc_path_taken; PsEncPath has no field for it). */
int ps_set_front_fused(int on);
int ps_front_fused_taken(void);
/* Unit-test hook of that form: ps_tem_forward_sampled twice from the same inputs — the two launches into ws_a, the one launch
 * into ws_b (neg_* / loss3_*: each run's draws and loss) — and the largest absolute difference of what the front end and its
 * riders leave, per region (a value that differs only as a NaN counts as infinity), in this order: x, qmean_d, query_emb,
 * kp, vp (valid positions only), qp, attn, amask, ctx, word_scores, word_terms, neg items, neg words, vrows (the listed part),
 * vcount.  taken[0] / taken[1]: ps_front_fused_taken() after each run.  Synchronises the stream. */
#define PS_FRONT_TEST_REGIONS 15
int ps_front_fused_test(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch, const float* alias_prob,
                        const int32_t* alias_idx, float* ws_a, float* ws_b, int64_t* neg_item_a, int64_t* neg_word_a,
                        int64_t* neg_item_b, int64_t* neg_word_b, float* loss3_a, float* loss3_b, double* diff,
                        int32_t* taken, ps_stream_t stream);
/* Which kernels an item-transformer step launches (no reference counterpart; csrc/encoder.h, EncPlan): one attention form per
 * layer and the forms of the steps around it.  Forward: rowlist (K / V products over the valid-row list), fwd_fuse_last (the
 * last layer's Wo + LN + FFN + final LN as one kernel), fold_score (... with item scoring and the loss in its epilogue).
 * Backward: fuse_last (the last layer's per-replica backward as one kernel), item_scatter (... which scatters the item rows),
 * wg3_main / wg3_last (its K / V / Q weight gradients on the main stream / as the caller's last launches), wgrad_early (unfused
 * form: W2 / W1 weight gradients forked as soon as d a1 exists), q_folded (dQ.Wq in the attention backward's tail), listed
 * (dK / dV consumers walk the valid-row list), presum (the replicas' fan-in summed by its own launch), dx_fused (no dX product:
 * the attention backward leaves d x as two partial rows). */
typedef struct PsEncPath {
  int32_t n_layers;
  int32_t attn[PS_MAX_LAYERS];     /* AttnForm per layer: 0 generic, 1 sq1, 2 w1, 3 wf, 4 kvq */
  int32_t rowlist, fwd_fuse_last, fold_score;
  int32_t bwd_fuse_last, item_scatter, wg3_main, wg3_last, wgrad_early, q_folded, listed, presum, dx_fused;
  int32_t wf_key_split;            /* taken record only: the WF backward launched attn_bwd_wk_kernel */
} PsEncPath;
/* The plan of the call this descriptor describes (C == 0: a training-mode forward / backward, C > 0: an eval scoring call), under
 * the process's switches and setters.  Host only: no HIP call, works without a device — the plan reads the descriptor, the
 * workspace layout, which tensors are null and the switches, and never dereferences a tensor or the workspace.  params NULL:
 * every tensor present.  has_valid: the layer loops get a key-padding mask (the review transformer's callers; 0 here). */
int ps_tem_plan(const PsTemDesc* desc, const PsTemTensors* params, int32_t has_valid, PsEncPath* out);
/* What the last encoder forward (backward = 0: any entry point that encodes, eval calls included) or backward (backward = 1)
 * of this process really launched: every field is set at the branch that launches, none is copied from the plan; the fields of
 * the other direction are 0, and a backward reads the kvq form as wf (3).  Two fields are inferred at their branch rather than
 * seen at a launch: rowlist is set with the kvq launch (whose workgroups project their sequence's valid positions only; the form
 * exists only under the row list), and wg3_last where the three weight-gradient problems are handed to the caller, which
 * launches them behind its embedding scatter.  A non-encoder model leaves n_layers = 0.  Under
 * graph replay the record is that of the capture.  item_scatter equals ps_item_scatter_fused_taken(). */
int ps_enc_path_taken(int32_t backward, PsEncPath* out);
/* Tuning knob: how the backward's side stream crosses the main stream.  Bit 1: a join is a stream write-value / wait-value
 * pair instead of an event pair; bit 0: a fork is a wait-value on the side stream whose value the NEXT kernel launched on the
 * main stream stores as its first workgroup starts (every earlier main-stream kernel has completed by then) — the main stream
 * itself executes nothing for a fork (round 2: -9 us per C2 step against write operations, which in turn were -5..-8 us
 * against events).  Default 3 (env PS_SIDE_MODE), 0 = event pairs only.  The wait is a spinning one-thread kernel: tools that
 * let only one kernel run at a time (counter-collecting profilers) are recognised from their environment and always get
 * events (PS_SIDE_EVENTS=1 forces that).  Returns the previous value. */
int ps_set_side_mode(int mode);
/* The value crossings are used only where a start-up self-test (once per process and device: the side stream parked on a
 * probe word, released by a write-value on another stream, polled with a host-side timeout and, failing that, released from
 * the host) has shown that a wait makes progress beside its producer; otherwise event pairs, which cannot hang.
 * ps_side_values_in_use(): 1 = value waits in use, 0 = event pairs or a single stream.  PS_SIDE_SELFTEST_FAIL=1 makes the
 * probe fail (tests). */
int ps_side_values_in_use(void);
/* Error-path hygiene of the side stream: every ps_*_backward that fails releases a fork of the side stream whose
 * signalling launch never happened, so the caller's next synchronize returns and the error surfaces (it could otherwise
 * wait forever on hipStreamWaitValue32).  ps_side_abort() does the same on demand; ps_debug_fail_fork(n) is the test hook
 * that makes the n-th fork from now on fail after it has parked the side stream (0 = off). */
void ps_side_abort(void);
void ps_debug_fail_fork(int nth);
/* Deterministic mode (env PS_DETERMINISTIC=1, no reference counterpart: the reference's CUDA index_add_ / embedding backward are
 * not deterministic either): the item-transformer training step becomes bitwise reproducible run to run — everything on one
 * stream, weight gradients as per-split partial matrices added up in split order by a second launch, table scatters by
 * sole-owner half-waves that walk the task lists in order.  ~2.6x the default step time (0.78 ms at C2: a
 * popular row's additions are one chain); allocates scratch buffers on first use; process-wide.  The review transformer runs
 * in this mode too.  Returns the previous value; a negative argument only queries. */
int ps_set_deterministic(int on);
/* Product form of the large linears (no reference counterpart).  mode 1: launches with enough tiles to fill the chip take
 * the bf16x3 kernel — every fp32 operand split exactly into three bf16 values, six v_mfma_f32_32x32x16_bf16 per product step,
 * fp32 accumulation: as accurate as the fp32 MFMA (1.1e-7 of sum|a b|) at a third of its cycles; mode 0: the fp32 MFMA
 * everywhere.  force_shape -1: tile chosen by the launch's size; 0 / 1 / 2: 64x64 / 128x64 / 128x128 for every launch that
 * has an instantiation (tests); 3: the direct-to-LDS form (fp32 slabs by global_load_lds, split on the fragments in registers,
 * 128x128 tiles) wherever it applies; 4: weights pre-split once per call into bf16 plane images (ps_gemm_f32_weight; the d >= 256
 * step's forward / dX products), the size rule elsewhere.  3 and 4 are measured alternatives (profiles/r04_gemm_notes.md), not defaults.  Env PS_GEMM_X3 / PS_GEMM_X3_SHAPE set the initial values.  Process-wide. */
int ps_gemm_x3_config(int mode, int force_shape);
/* C = (A . op(W) + bias) * alpha with W declared a WEIGHT — [N][K] (tb 0, nn.Linear, models/neural.py:20-21, 86-96) or [K][N]
 * (tb 1: the input-gradient product of the same linear) with dense rows: W is split once into bf16 plane images for the
 * duration of the call and the product runs on the pre-split-weight kernel (gemm_x3w_kernel) where it applies
 * (ps_gemm_x3_config(1, 4), M >= 4096, N / K multiples of 32), otherwise as ps_gemm_f32 would.  What the d >= 256 step's forward / dX products do. */
int ps_gemm_f32_weight(const float* A, int lda, const float* W, int tb, float* C, int ldc, int M, int N, int K,
                       const float* bias, float alpha, ps_stream_t stream);
/* Which kernel a group of products takes (no reference counterpart; csrc/gemm.hip, gemm_plan — the function every launch goes
 * through; DESIGN.md, "which kernel a product takes").  A member is described by its shape and layouts, full (0: the plain
 * epilogue, 1: an activation, 2: dropout — both need the full one), listed (a row list), accumulate (0 store, 1 +=, 2 atomic),
 * split_stride (> 0: per-split outputs), no_deep and kseg (reduction rows per B segment; 0: one segment).  flat / prefer_x3d: the
 * group's fields of the same name; planes: weight planes are registered for every member (ps_gemm_f32_weight's scope).  The plan:
 * family 0 fp32 / 1 bf16x3 / 2 bf16x3 direct-to-LDS / 3 bf16x3 pre-split weights; the instantiation (ta, tb, full, idx); bk / pf
 * (slab depth, slabs in flight); the tile; flat (1-D grid) and redirected (asked for on the 3-D grid, sent to the flat one); the
 * grid; dynamic LDS bytes; the XCD placement masks.  Host only: no HIP call, works without a device — the group is filled with
 * dummy addresses that are never dereferenced.  A group no launch would accept is refused with the launch's own message. */
typedef struct PsGemmMember {
  int32_t M, N, K, ksplit, ta, tb, full, listed, accumulate, split_stride, no_deep, kseg;
} PsGemmMember;
typedef struct PsGemmPlan {
  int32_t family, ta, tb, full, idx, bk, pf, tile_m, tile_n, flat, redirected, grid_x, grid_y, grid_z, lds_bytes, flat_xcd, split_xcd;
} PsGemmPlan;
int ps_gemm_plan(int32_t n, const PsGemmMember* members, int32_t flat, int32_t prefer_x3d, int32_t planes, PsGemmPlan* out);

/* Workspace the caller allocates once per shape (bytes) and its layout. */
int ps_tem_workspace_layout(const PsTemDesc* desc, PsTemWsLayout* out);

/* loss = model(batch)                      -- ItemTransformerRanker.forward
 *   (models/item_transformer.py:352-359 -> forward_dotproduct :440-520, or forward_attn/QEM :361-438)
 * loss3[0..2] = {ps_loss + item_loss, ps_loss, item_loss} (device floats);
 * loss_acc (optional, device float[2]) += {ps_loss, item_loss}: the running sums the reference keeps in
 * model.ps_loss / model.item_loss with two .item() syncs per step (item_transformer.py:516-517). */
int ps_tem_forward(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                   float* workspace, float* loss3, float* loss_acc, ps_stream_t stream);
/* The same with the two negative draws (ps_sample_negatives) folded into the forward's first launch: batch->neg_* are
 * ignored, neg_item_out [B,K] / neg_word_out [B,W*K] receive the draws and are what the backward must be given. */
int ps_tem_forward_sampled(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                           const float* alias_prob, const int32_t* alias_idx, int64_t* neg_item_out, int64_t* neg_word_out,
                           float* workspace, float* loss3, float* loss_acc, ps_stream_t stream);

/* loss.backward()                          -- trainer.py:77 (autograd of the above).
 * ACCUMULATES loss_scale * dloss/dparam into `grads` (dense, like the reference's
 * nn.Embedding(sparse=False)); the caller zeroes grads (model.zero_grad(), trainer.py:76). */
int ps_tem_backward(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                    float* workspace, const PsTemTensors* grads, float loss_scale,
                    const float* loss_scale_dev /* optional device scalar multiplied in (autograd's grad_output) */,
                    ps_stream_t stream);

/* The embedding-gather+score kernel alone (the launch ps_tem_forward makes after the encoder):
 * B*(1+K) item rows . encoder output + B*W*(1+K) word rows . target item row -> workspace scores.
 * Exposed so bench.py / rocprofv3 can time exactly this launch. */
int ps_gather_score(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                    float* workspace, ps_stream_t stream);

/* scores = model.test(batch) [B,C]         -- test_dotproduct (item_transformer.py:111-146)
 *                                             / test_attn QEM (:148-160,189-195) */
int ps_tem_score(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                 float* workspace, float* scores, ps_stream_t stream);

/* The two torch.multinomial draws of one forward (item_transformer.py:447, :268):
 * uniform items over [0,P) and alias-table words ~ word_dists.  alias tables are
 * built on the host by ps_build_alias_host. */
int ps_sample_negatives(const PsTemDesc* desc, const float* alias_prob, const int32_t* alias_idx,
                        int64_t* neg_item_idxs, int64_t* neg_word_idxs, ps_stream_t stream);
int ps_build_alias_host(const double* dist_host, int64_t n, float* prob_host, int32_t* alias_host);

/* optim.step()                             -- Optimizer.step (models/optimizers.py:205-243):
 * clip_grad_norm_(max_grad_norm) over all listed grads, then dense Adam(eps) with
 * bias correction, optional L2 (weight_decay) and noam schedule.  The tensor
 * table lives on the device (ps_adam_plan_bytes / ps_adam_plan_write_host); its
 * tail is device scratch the two launches of a step hand the gradients' non-zero
 * mask through (the update does not re-read 16-byte groups of zeros), so a plan
 * serves ONE optimizer step at a time and must be writable.
 * state[0] (device, int64) holds the step count and is incremented by the call;
 * (float*)(state+2) is scratch for n_chunks partial sums. */
typedef struct PsAdamHyper {
  float lr;            /* --lr (original_lr when noam)                 */
  float beta1, beta2;  /* --beta1 --beta2                              */
  float eps;           /* 1e-9 (optimizers.py:186-187)                 */
  float weight_decay;  /* --l2_lambda                                  */
  float max_grad_norm; /* --max_grad_norm, 0 = no clip                 */
  int32_t noam;        /* --decay_method noam                          */
  int32_t warmup_steps;/* --warmup_steps                               */
  float grad_scale;    /* multiplies every grad first (1/world for DP) */
  int32_t zero_grads;  /* dense step: leave every gradient it consumed at 0 (the next zero_grad() is then free) */
  int32_t method;      /* --optim (optimizers.py:175-187): 0 adam, 1 sgd, 2 adagrad (eps 1e-10; the plan's `m` is the sum of
                          squares, initialised by the caller with adagrad_accum), 3 adadelta (rho 0.9, eps 1e-6; `m` = square_avg,
                          `v` = acc_delta).  Same clip, same noam schedule; sgd touches neither `m` nor `v`. */
  int32_t pad_;
} PsAdamHyper;

int64_t ps_adam_plan_bytes(int32_t n_tensors, const int64_t* numel_host);
int ps_adam_plan_write_host(int32_t n_tensors, float* const* p, float* const* g, float* const* m,
                            float* const* v, const int64_t* numel_host, void* plan_host);
int32_t ps_adam_plan_chunks_host(const void* plan_host);     /* grid size; state needs 2 int64 + n_chunks floats */
int ps_clip_adam_dense(const void* plan_dev, int32_t n_chunks, const PsAdamHyper* hyper,
                       int64_t* state_dev, float* gnorm_out_dev /* [2]: norm, lr; may be NULL */,
                       ps_stream_t stream);

/* The same step cut in two for the SHARDED data-parallel optimizer (no reference counterpart; the reference is
 * single-process, trainer.py:64-83): after a reduce-scatter every rank owns 1/world of the flat gradient, and
 * clip_grad_norm_ (optimizers.py:241-242) is a norm over ALL gradients, so the ranks' partial sums of squares meet in one
 * scalar all-reduce between the two launches.  ps_adam_sumsq: out_sumsq_dev[0] = sum over the plan of (g*grad_scale)^2
 * (fixed-order reduction) and state[0] += 1.  ps_adam_update_ext: clip + Adam exactly as ps_clip_adam_dense, with the
 * global sum of squares read from total_sumsq_dev. */
int ps_adam_sumsq(const void* plan_dev, int32_t n_chunks, const PsAdamHyper* hyper, int64_t* state_dev,
                  float* out_sumsq_dev, ps_stream_t stream);
int ps_adam_update_ext(const void* plan_dev, int32_t n_chunks, const PsAdamHyper* hyper, int64_t* state_dev,
                       const float* total_sumsq_dev, float* gnorm_out_dev, ps_stream_t stream);

/* Peer-to-peer reduce-scatter, local half (no reference counterpart: trainer.py:64-83 is single-process): recv [world][n] =
 * every rank's copy of this rank's slice of the flat gradient (after an equal-split all-to-all); out[i] = sum over ranks in
 * rank order; the same launch clears `zero_n` floats at `zero` (the flat gradient buffer the all-to-all has consumed).
 * n and zero_n multiples of 4, buffers 16-byte aligned. */
int ps_sum_slices(const float* recv, int32_t world, int64_t n, float* out, float* zero, int64_t zero_n, ps_stream_t stream);

/* model.zero_grad() helper (trainer.py:76): async memset of a float buffer. */
int ps_zero_floats(float* p, int64_t n, ps_stream_t stream);

/* ------------------------------------------------------------------ graph-replayed training step
 * ps_tem_forward_step / ps_tem_backward_step run the same launch sequences as ps_tem_forward / ps_tem_backward, but
 * capture them once per shape (second call) and replay them as HIP graphs afterwards; what varies per call — the
 * caller's index tensors, the Philox step, the loss output — enters through a staging prologue (first node) and the
 * loss node, whose arguments are refreshed before each replay.  Same kernels, same results.  It cuts the host cost of
 * a step (347 -> 285 us), which matters when the host also builds batches; it does not shorten the device timeline, so
 * it is opt-in: PS_GRAPHS=1 (otherwise ps_graph_replay_enabled() is 0 and callers use the eager entry points).
 *   forward_step : batch as for ps_tem_forward; sampler_prob/alias (ps_build_alias_host tables) non-NULL => the two
 *                  negative draws (item_transformer.py:447, :268) happen in the prologue and batch->neg_* are ignored.
 *   backward_step: reuses the staged inputs of the last forward_step on this workspace; zero_ptr/zero_floats fold
 *                  model.zero_grad() of the flat gradient buffer in as the first node (NULL/0: keep accumulating). */
int ps_graph_replay_enabled(void);
int ps_tem_staged_batch(const PsTemDesc* desc, float* workspace, PsTemBatch* out);   /* where forward_step staged the indices */
int ps_tem_forward_step(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch,
                        const float* sampler_prob, const int32_t* sampler_alias, float* workspace, float* loss3,
                        float* loss_acc, ps_stream_t stream);
int ps_tem_backward_step(const PsTemDesc* desc, const PsTemTensors* params, float* workspace, const PsTemTensors* grads,
                         float loss_scale, float* zero_ptr, int64_t zero_floats, ps_stream_t stream);

/* ------------------------------------------------------------------ full-catalogue evaluation
 * Trainer.test / validate over ALL products (trainer.py:125-226 with test_candi_size < 1): encode each (user, query)
 * row once, score it against every row of the table with one fp32 MFMA GEMM per table panel, and select the top-k and
 * the target's rank on the device.  ps_tem_encode = the eval-mode sequence representation of item_transformer.py:118-131
 * (descriptor as for ps_tem_score, C >= 1; candidates are not read). */
int ps_tem_encode(const PsTemDesc* desc, const PsTemTensors* params, const PsTemBatch* batch, float* workspace,
                  float* enc_out /* [B,d] */, ps_stream_t stream);
/* scores[b,p] = q[b]·table[p] (+ bias[p]), p in [0, n_rows).  top_idx/top_score [B,topk]: best first, ties by lower
 * row id (unfilled slots: -1 / -inf when n_rows < topk).  rank[b] (optional, needs target) = 1 + number of rows ranked
 * ahead of target[b] under the same order = position in `argsort(scores)[::-1]` (trainer.py:137,172-180); 0 if the
 * target is not a table row.  topk <= 256.  scratch: ps_rank_scratch_bytes() bytes, 256-byte aligned. */
int64_t ps_rank_scratch_bytes(int32_t B, int64_t n_rows, int32_t d, int32_t topk);
int ps_rank_all(const float* q, int32_t B, int32_t d, const float* table, int64_t n_rows, const float* bias,
                const int64_t* target, int32_t topk, int64_t* top_idx, float* top_score, int32_t* rank,
                void* scratch, int64_t scratch_bytes, ps_stream_t stream);
/* One rank's part of the same ranking over a ROW-SHARDED table (prodsearch_amd/sharded.py; the reference keeps
 * the whole table on one device, item_transformer.py:46): table row i is catalogue id i * id_mul + id_add (world, rank);
 * target[b] is a catalogue id and target_score[b] its score, computed where its row lives (+inf: not a product);
 * ahead[b] = rows of THIS shard ranked ahead of the target under (score desc, id asc), the target's own row excluded;
 * top_idx carries catalogue ids.  The caller adds the shards' counts (rank = 1 + sum) and merges their top-k lists. */
int ps_rank_shard(const float* q, int32_t B, int32_t d, const float* table, int64_t n_rows, const float* bias,
                  const int64_t* target, const float* target_score, int64_t id_mul, int64_t id_add, int32_t topk,
                  int64_t* top_idx, float* top_score, int32_t* ahead, void* scratch, int64_t scratch_bytes, ps_stream_t stream);

/* ------------------------------------------------------------------ row-sparse optimizer path
 * For tables too large to stream every step (BASELINE configs[4]: 50 M x 256).  The gradient tensors
 * stay dense, like nn.Embedding(sparse=False) gives the reference (item_transformer.py:46,70); the
 * optimizer, the zeroing and the data-parallel exchange only visit the rows a step touched.
 * Replaces: the table part of Optimizer.step (optimizers.py:241-243) and model.zero_grad (trainer.py:76).
 * Semantics of untouched rows: p, m, v unchanged (torch.optim.SparseAdam's rule), NOT dense Adam's decay. */
typedef struct PsIdxList { const int64_t* idx; int64_t n; } PsIdxList;   /* device pointer, element count */

/* Sorted unique row ids (!= pad_row) over up to 8 index lists -> rows_out[0..*count).  ws = ps_coalesce_ws_bytes
 * bytes, zeroed once by the caller and left zeroed by every call.  cap >= min(sum n, n_rows).  The one-table form of
 * ps_coalesce_tables (below): the same kernels, launched over one table. */
int64_t ps_coalesce_ws_bytes(int64_t n_rows);
int ps_coalesce_rows(const PsIdxList* lists_host, int32_t n_lists, int64_t n_rows, int64_t pad_row, void* ws_dev,
                     int64_t* rows_out_dev, int64_t cap, int32_t* count_out_dev, ps_stream_t stream);
/* values[u,:] = table[rows[u],:] and the inverse, u < *count_dev (or < cap when count_dev is NULL); d % 4 == 0 */
int ps_gather_rows(const float* table_dev, int32_t d, const int64_t* rows_dev, const int32_t* count_dev, int64_t cap,
                   float* values_out_dev, ps_stream_t stream);
int ps_scatter_rows(float* table_dev, int32_t d, const int64_t* rows_dev, const int32_t* count_dev, int64_t cap,
                    const float* values_dev, ps_stream_t stream);
int ps_zero_rows(float* table_dev, int32_t d, const int64_t* rows_dev, const int32_t* count_dev, int64_t cap,
                 ps_stream_t stream);
/* Device address of a coalesce workspace's status word: 0 ok, 1 an index outside [0, n_rows) was dropped, 2 more
 * unique rows than `cap`.  Callers copy it back when they can afford a sync (the step itself never does). */
const int32_t* ps_coalesce_bad_flag(void* ws_dev, int64_t n_rows);

/* Data-parallel exchange of a table's touched rows with NO host synchronisation (new: the reference is single-process,
 * trainer.py:64-83).  Every rank packs a fixed-capacity message — msg_rows[cap]: its sorted touched ids, then -1;
 * msg_vals[cap,d]: their gradient rows, then zeros — the messages are all-gathered (RCCL), the union of the ids is
 * ps_coalesce_rows over the gathered ids with pad_row = -1, and ps_merge_rows writes, for every union row, the sum of the
 * ranks' rows IN RANK ORDER into the dense gradient: bitwise the same result on every rank.  world <= 32, d % 4 == 0.
 * These are the one-table forms of ps_pack_tables / ps_merge_tables (below), with the id and value sections in buffers
 * of their own: all_rows [world, cap], all_vals [world, cap, d].
 * ps_pack_rows: grad_dev [n_rows, d]; rows_dev holds list_cap entries (the touched list's allocation, 1 <= list_cap <= cap),
 * *count_dev of them live.  msg_rows[u] / msg_vals[u, :] for u < cap: the list's id and its gradient row, or -1 / zeros for
 * a slot past the count, past list_cap or holding an id outside [0, n_rows) — nothing past list_cap is read. */
int ps_pack_rows(const float* grad_dev, int32_t d, int64_t n_rows, const int64_t* rows_dev, const int32_t* count_dev,
                 int64_t list_cap, int64_t cap, int64_t* msg_rows_dev, float* msg_vals_dev, ps_stream_t stream);
int ps_merge_rows(const int64_t* all_rows_dev, const float* all_vals_dev, int32_t world, int64_t cap, int32_t d,
                  float* grad_dev, const int64_t* union_rows_dev, const int32_t* union_count_dev, int64_t union_cap,
                  ps_stream_t stream);

typedef struct PsRowTable {
  float* p; float* g; float* m; float* v;   /* [n_rows, d] parameter, dense gradient, Adam moments */
  const int64_t* rows;                      /* touched rows (device)                                 */
  const int32_t* count;                     /* number of valid entries of rows (device)              */
  int64_t cap;                              /* launch bound: *count <= cap                           */
  int32_t d;
  int32_t pad_;
} PsRowTable;

/* clip_grad_norm_ over (tensors of the dense plan + touched rows of the tables) then Adam on exactly those;
 * touched gradient rows are zeroed in the same pass.  plan = ps_adam_plan_* over the small tensors.
 * state_dev: 2 int64 {step, -} followed by ps_adam_rowsparse_state_floats() floats of scratch. */
int64_t ps_adam_rowsparse_state_floats(int32_t n_chunks, const PsRowTable* tables_host, int32_t n_tables);
int ps_clip_adam_rowsparse(const void* plan_dev, int32_t n_chunks, const PsRowTable* tables_host, int32_t n_tables,
                           const PsAdamHyper* hyper, int64_t* state_dev, float* gnorm_out_dev, ps_stream_t stream);

/* Lazy-EXACT dense Adam on the row-sparse machinery (args.lazy_exact_adam): last_dev[i][r] = optimizer steps row r of table i
 * has had applied; the call replays, for every listed row (tables_host[i].rows / count) or every row (all_rows != 0), the
 * steps last+1 .. state_dev[0] it missed with a ZERO gradient — the dense optimizer's arithmetic for a row without gradient
 * (optimizers.py:186-187, 241-243: the moments decay, the row keeps moving) — and sets last = state_dev[0] (+1 with `advance`:
 * the step in progress is about to update the row).  Called before a forward reads the rows, over the final touched list before
 * ps_clip_adam_rowsparse, and with all_rows before evaluation / checkpointing.  tables_host[i].g is not read. */
int ps_rowsparse_catchup(const PsRowTable* tables_host, int32_t n_tables, int32_t* const* last_dev, const int64_t* n_rows_host,
                         const PsAdamHyper* hyper, const int64_t* state_dev, int32_t advance, int32_t all_rows,
                         ps_stream_t stream);

/* ------------------------------------------------------------------ row-sharded tables (no reference
 * counterpart: item_transformer.py:46,464-469 keeps the whole table on one device).  Row i lives on rank i % world at local
 * row i / world.  Per step: ps_coalesce_rows gives the rank's sorted unique rows; ps_shard_bucket cuts that list into one
 * fixed-capacity request per owner — send_ids[o][0..capp): local rows (id / world) of the ids with id % world == o,
 * ascending, then -1 — and records the slot o * capp + position of every list entry (slot_of); the requests and then the
 * rows (ps_gather_rows accepts the -1 padding: zero rows) travel by equal-split all-to-alls; ps_shard_remap rewrites an
 * index tensor into slots (pad_in -> pad_out), so the receive buffer [world * capp + 1, d] IS the table the step reads.
 * The gradient returns the same way; ps_coalesce_rows (pad -1) + ps_merge_rows over the received requests give the owner's
 * touched rows and their rank-ordered sums.  *bad_dev: 1 = an index missing from the list, 2 = a request overflowed capp. */
int ps_shard_bucket(const int64_t* rows_dev, const int32_t* count_dev, int32_t world, int64_t capp, int64_t* send_ids_dev,
                    int32_t* slot_of_dev, int32_t* bad_dev, ps_stream_t stream);
int ps_shard_remap(const int64_t* idx_dev, int64_t n, int64_t pad_in, const int64_t* rows_dev, const int32_t* count_dev,
                   const int32_t* slot_of_dev, int64_t pad_out, int64_t* out_dev, int32_t* bad_dev, ps_stream_t stream);
/* ps_clip_adam_rowsparse cut in two for sharded tables: tables [0, n_shared) and the dense plan are replicated (their sum of
 * squares counts once), tables [n_shared, n_tables) are this rank's shards (their sums add over the ranks).  sums_dev[0] =
 * replicated part, sums_dev[1] = owned part; the caller all-reduces sums_dev[1] between the calls; the clip norm
 * (optimizers.py:241-242) is sqrt(sums[0] + sums[1]).  state as for ps_clip_adam_rowsparse. */
int ps_rowsparse_sumsq(const void* plan_dev, int32_t n_chunks, const PsRowTable* tables_host, int32_t n_tables, int32_t n_shared,
                       const PsAdamHyper* hyper, int64_t* state_dev, float* sums_dev, ps_stream_t stream);
int ps_rowsparse_update_ext(const void* plan_dev, int32_t n_chunks, const PsRowTable* tables_host, int32_t n_tables,
                            const PsAdamHyper* hyper, int64_t* state_dev, const float* sums_dev, float* gnorm_out_dev,
                            ps_stream_t stream);

/* ------------------------------------------------------------------ RTM (review_transformer)
 * ProductRanker (models/ps_model.py:53-370) with the pv (models/PV.py) / pvc (models/PVC.py) review
 * encoders.  Sequences are [query, R reviews]; K negatives per row (training) or C candidates (eval). */
enum { PS_RENC_PV = 0, PS_RENC_PVC = 1,
       PS_RENC_FS = 2,    /* review vector = tanh(f_W . dropout(masked mean of its words) + b)  (ps_model.py:148-149, 301-305;   */
       PS_RENC_AVG = 3 }; /*                 dropout(masked mean)                                text_encoder.py:19-40, 62-83)  */

typedef struct PsRtmDesc {
  int32_t B, K;          /* batch rows, --neg_per_pos                                             */
  int32_t R;             /* padded reviews per sequence (<= --uprev_review_limit + --iprev_review_limit) */
  int32_t Q;             /* padded query length                                                   */
  int32_t W;             /* PV window (--pv_window_size), words predicted per positive review     */
  int32_t WL;            /* words per review of the pvc encoder (--review_word_limit)             */
  int32_t C;             /* candidates per row, eval only                                         */
  int32_t d, H, F, n_layers;
  int64_t vocab_size;    /* V, pad = V-1                                                          */
  int64_t review_count;  /* pad review = review_count-1 (ps_model.py:70)                          */
  int32_t review_encoder;/* PS_RENC_PV / PVC / FS / AVG (--review_encoder_name)                   */
  int32_t query_encoder; /* PS_QENC_FS / PS_QENC_AVG                                              */
  int32_t use_pos_emb, use_seg_emb, pos_weight;
  int32_t train_pv;      /* forward(batch, train_pv): add the PV word-prediction loss (ps_model.py:265-280) */
  int32_t training;
  float dropout;         /* --dropout                                                             */
  float corrupt_rate;    /* --corrupt_rate: token dropout of the pvc encoder (PVC.py:46-54)       */
  uint64_t seed, step;
  int32_t use_user_emb;  /* --use_user_emb / --use_item_emb: per-position user / item embeddings added  */
  int32_t use_item_emb;  /*   to every sequence (ps_model.py:325-334, :229-234)                         */
  int64_t user_size;     /* pad user = user_size, pad item = product_size (ps_model.py:66-67)           */
  int64_t product_size;
  /* appended (a zero-filled tail is the behaviour before them): */
  int32_t frozen_mask;   /* PS_RTM_FROZEN_*: tables that take no gradient (nn.Embedding.from_pretrained, fix_emb,       */
                         /*   requires_grad False); ps_rtm_backward wants exactly their gradient pointers NULL          */
  int32_t no_pv_drop;    /* fix_emb (PV.py:36-39): PV.forward's own drop_layer has p = 0; dropout_layer still applies   */
} PsRtmDesc;
enum { PS_RTM_FROZEN_WORD = 1,     /* word_embeddings (= pvc's context_embeddings)            */
       PS_RTM_FROZEN_REVIEW = 2,   /* review_encoder.review_embeddings (pv)                   */
       PS_RTM_FROZEN_USER = 4,     /* user_emb (use_user_emb)                                 */
       PS_RTM_FROZEN_ITEM = 8 };   /* product_emb (use_item_emb)                              */

typedef struct PsRtmTensors {
  float *word_emb;       /* word_embeddings.weight [V,d] (= review_encoder.context_embeddings for pvc) */
  float *review_emb;     /* review_encoder.review_embeddings.weight [review_count,d] (pv) or NULL  */
  float *seg_emb;        /* seg_embeddings.weight [4,d]                                            */
  float *fs_w, *fs_b;    /* query_encoder.f_W                                                      */
  float *pe;             /* transformer_encoder.pos_emb.pe                                         */
  float *final_ln_g, *final_ln_b;
  float *wo_w, *wo_b;    /* transformer_encoder.wo [1,d],[1] (transformer.py:69,96)                */
  float *user_emb;       /* user_emb.weight [user_size+1,d]       (use_user_emb) or NULL           */
  float *product_emb;    /* product_emb.weight [product_size+1,d] (use_item_emb) or NULL           */
  float *rev_fs_w, *rev_fs_b; /* review_encoder.f_W [d,d],[d] (fs review encoder) or NULL          */
  PsLayerTensors layer[PS_MAX_LAYERS];
} PsRtmTensors;

/* ProdSearchTrainBatch / ProdSearchTestBatch (data/batch_data.py:137-223, :94-135) + the PV-loss draw */
typedef struct PsRtmBatch {
  const int64_t *query_word_idxs;         /* [B,Q]                                   */
  const int64_t *pos_prod_ridxs;          /* [B,R]                                   */
  const int64_t *pos_seg_idxs;            /* [B,R+1]                                 */
  const int64_t *pos_prod_rword_idxs;     /* [B,R,W] PV target words (train_pv) / [B,R,WL] review words (pvc, !train_pv) */
  const uint8_t *pos_prod_rword_masks;    /* [B,R,W] uint8                           */
  const int64_t *neg_prod_ridxs;          /* [B,K,R]                                 */
  const int64_t *neg_seg_idxs;            /* [B,K,R+1]                               */
  const int64_t *neg_prod_rword_idxs;     /* [B,K,R,WL] pvc, !train_pv               */
  const int64_t *pos_prod_rword_idxs_pvc; /* [B,R,WL]   pvc, train_pv                */
  const int64_t *neg_prod_rword_idxs_pvc; /* [B,K,R,WL] pvc, train_pv                */
  const int64_t *neg_word_idxs;           /* [B*R, W*K] torch.multinomial(word_dists) of PV.py:57 / PVC.py:81 */
  const int64_t *candi_prod_ridxs;        /* [B,C,R]   eval                          */
  const int64_t *candi_seg_idxs;          /* [B,C,R+1] eval                          */
  const float *review_embeddings;         /* [review_count,d] eval table (get_review_embeddings, ps_model.py:186-203) */
  const int64_t *pos_user_idxs;           /* [B,R+1]   use_user_emb (pad user_size)  */
  const int64_t *neg_user_idxs;           /* [B,K,R+1]                               */
  const int64_t *pos_item_idxs;           /* [B,R+1]   use_item_emb (pad product_size) */
  const int64_t *neg_item_idxs;           /* [B,K,R+1]                               */
  const int64_t *candi_seq_user_idxs;     /* [B,C,R+1] eval                          */
  const int64_t *candi_seq_item_idxs;     /* [B,C,R+1] eval                          */
  const uint8_t *neg_prod_rword_masks;    /* [B,K,R,WL] uint8: fs / avg review encoders (with pos_prod_rword_masks [B,R,WL]) */
} PsRtmBatch;

int ps_rtm_workspace_floats(const PsRtmDesc* desc, int32_t eval, int64_t* total);
/* Offsets (in floats) of the intermediates inside the workspace, for stage-by-stage parity tests.  Sequences are
 * n = b*J + j (J = 1+K training: j = 0 positive; J = C eval), S = R+1 positions [query, reviews]. */
typedef struct PsRtmWsLayout {
  int64_t total_floats;
  int32_t Bseq, S, J, pad_;
  int64_t query_emb;   /* [B,d]        FS(query)                                   (ps_model.py:257-258) */
  int64_t valid;       /* [Bseq,S]     1 = unmasked position                        (:316-318)            */
  int64_t x;           /* [Bseq,S,d]   encoder input (review vectors + seg/user/item emb, masked, + pe) (:320-334) */
  int64_t vec;         /* [B*R,d]      review vector the PV loss predicts from (train_pv)  (PV.py:53-54, PVC.py:77-78) */
  int64_t cnt;         /* [Bseq,R]     non-pad words per review (pvc)                */
  int64_t enc;         /* [Bseq,d]     final-LayerNorm output at position 0          (transformer.py:90-95) */
  int64_t scores;      /* [Bseq]       wo . enc + b                                  (transformer.py:96)    */
  int64_t weight;      /* [Bseq]       BCE weight of each sequence                   (ps_model.py:344-345)  */
  int64_t pv_scores;   /* [B*R,W,1+K]  PV-loss logits (train_pv)                     (PV.py:59-63)          */
  int64_t dx;          /* [Bseq,S,d]   gradient w.r.t. x after the backward                                 */
} PsRtmWsLayout;
int ps_rtm_workspace_layout(const PsRtmDesc* desc, int32_t eval, PsRtmWsLayout* out);
/* loss = model(batch, train_pv) -- ProductRanker.forward (ps_model.py:241-358); loss3 = {loss, ps_loss, pv_loss} */
int ps_rtm_forward(const PsRtmDesc* desc, const PsRtmTensors* params, const PsRtmBatch* batch, float* workspace,
                   float* loss3, ps_stream_t stream);
/* loss.backward() (trainer.py:77): accumulates into dense grads.  grads->word_emb / review_emb / user_emb / product_emb NULL:
 * that table is frozen and no kernel reads or writes a gradient row of it; the NULLs must agree with desc->frozen_mask (a table
 * the configuration does not have — review_emb of pvc / fs / avg, user_emb without use_user_emb — is not checked). */
int ps_rtm_backward(const PsRtmDesc* desc, const PsRtmTensors* params, const PsRtmBatch* batch, float* workspace,
                    const PsRtmTensors* grads, float loss_scale, const float* loss_scale_dev, ps_stream_t stream);
/* What ps_rtm_backward runs for this descriptor, decided once (csrc/rtm.hip, rtm_bwd_plan; the backward reads this plan and
 * nothing else).  Host only: no HIP call, works without a device; reads the descriptor, the workspace layout and the process's
 * switches (ps_set_deterministic, PS_RTM_HIST). */
enum { PS_RTM_INDEX_NONE = 0, PS_RTM_INDEX_HIST = 1,    /* LDS-histogram index on the side stream                        */
       PS_RTM_INDEX_FWD_COUNTS = 2,                     /* counts + ranks from the forward's gather, fill on the side stream */
       PS_RTM_INDEX_LATE = 3 };                         /* counted, allocated and filled behind the embed backward       */
enum { PS_RTM_PV_NONE = 0, PS_RTM_PV_DVEC = 1, PS_RTM_PV_WORDS = 2, PS_RTM_PV_BOTH = 3 };
enum { PS_RTM_EB_GENERAL = 0, PS_RTM_EB_PLAIN = 1,      /* rtm_embed_bwd_kernel<NK, 0 / 1>                               */
       PS_RTM_EB_FROZEN = 2 };                          /* <NK, 2>: no review-side table takes a gradient                */
typedef struct PsRtmBwdPlan {
  int32_t index;          /* PS_RTM_INDEX_*: the inverted index word -> review slots (rtm_hist* / rtm_walloc / rtm_windex) */
  int32_t word_reduce;    /* rtm_wreduce* sums the slot rows of every word into word_emb's gradient                        */
  int32_t slot_rows;      /* the review slots of d x are rewritten in place as per-word (pv, deterministic: per-review) rows */
  int32_t review_scatter; /* review rows are added into review_emb's gradient (atomics, or the sole-owner scatter)         */
  int32_t pv_bwd;         /* PS_RTM_PV_*: which gradients of the PV loss exist (d vec -> the review side, the word rows)    */
  int32_t pv_bwd_kernel;  /* rtm_pv_bwd_kernel is launched (deterministic + word rows only: rtm_pv_keys_kernel alone)      */
  int32_t fs_draw;        /* fs: the d raw = d pre . f_W product                                                           */
  int32_t query_scatter;  /* the query words' rows are scattered (and the unfused FS path builds d mean)                   */
  int32_t user_scatter, item_scatter;
  int32_t embed_form;     /* PS_RTM_EB_*                                                                                   */
  int32_t slot_waves;     /* the embed backward launches review-slot waves (0: the query-position waves alone)             */
  int32_t side_fork;      /* the backward forks its side stream for the index at its head                                  */
} PsRtmBwdPlan;
int ps_rtm_backward_plan(const PsRtmDesc* desc, PsRtmBwdPlan* out);
/* scores = model.test(batch) [B,C] -- ProductRanker.test (ps_model.py:205-239) */
int ps_rtm_score(const PsRtmDesc* desc, const PsRtmTensors* params, const PsRtmBatch* batch, float* workspace,
                 float* scores, ps_stream_t stream);
/* model.get_review_embeddings() for the pvc / fs / avg encoders (ps_model.py:186-203): per review the (uncorrupted,
 * undropped) mean of its non-pad words — fs: projected, tanh(f_W . mean + b) — last row 0.
 * scratch: [review_count, d] floats, fs only (else NULL). */
int ps_rtm_review_embeddings(const PsRtmDesc* desc, const PsRtmTensors* params, const int64_t* review_words,
                             float* scratch, float* out, ps_stream_t stream);

/* ------------------------------------------------------------------ RTM: the whole catalogue in one pass
 * What Trainer.test computes for the review transformer with test_candi_size < 1 (trainer.py:141-143, 189-226), without running
 * the encoder over every (entry, candidate) sequence: with ONE encoder layer a key / value row is linear in its token, every
 * per-review term depends on the review id alone (a review has one author and one item), and only position 0 is consumed —
 * so the reviews are projected once per evaluation (ps_rtm_rank_index), K / V / Q and the softmax partial over {query, the
 * user's reviews} once per entry, and per (entry, item) pair there is the softmax partial over the item's reviews, the merge
 * and the position-0 tail.  desc: B = entries per call, R = --uprev_review_limit + --iprev_review_limit (longest sequence;
 * item reviews past it are cut, as the loader cuts), Q, d, H, F, n_layers, review_count, vocab_size, the encoders and the use_*
 * flags; K, W, WL, C, training, dropout are not read.
 * Refused (error return, message naming the flag): n_layers != 1 (deeper encoders need every position of layer 0);
 * seq_review_test (do_seq_review_test and not train_review_only: the item lists then depend on the entry); fs / avg review
 * encoders with fix_emb. */
typedef struct PsRtmRankShape {
  int64_t n_items;           /* P: rows of item_ridxs, catalogue ids 0..P-1                                      */
  int64_t review_u_p_rows;   /* rows of review_u_p (reviews past them get no user / item row)                    */
  int32_t I;                 /* item_ridxs [P, I]: the item's reviews, then the pad id review_count-1            */
  int32_t U;                 /* u_ridxs [B, U]: the user's reviews, then the pad id                              */
  int32_t seq_review_test;   /* the run has do_seq_review_test and not train_review_only: refused                */
  int32_t fix_emb;           /* the run has fix_emb (refused with the fs / avg review encoders)                  */
} PsRtmRankShape;
/* floats of the projection ps_rtm_rank_index writes; -1 with ps_last_error() set: refused / bad sizes */
int64_t ps_rtm_rank_index_floats(const PsRtmDesc* desc, const PsRtmRankShape* shape);
/* Once per evaluation: KR / VR [review_count, d] = Wk / Wv . (review_embeddings[r] (+ user_emb[u_r]) (+ product_emb[i_r])) and the
 * [segment][position] key / value tables Wk / Wv . (seg + pe) + b.  review_embeddings: the table ProductRanker.test indexes;
 * review_u_p [review_u_p_rows, 2] (author, item): read only with use_user_emb / use_item_emb, else NULL.  The result is
 * stale once a weight or a table changes. */
int ps_rtm_rank_index(const PsRtmDesc* desc, const PsRtmRankShape* shape, const PsRtmTensors* params,
                      const float* review_embeddings, const int64_t* review_u_p, float* index_out, ps_stream_t stream);
/* bytes of scratch for ps_rtm_rank_all with `items_per_pass` items scored per pass (<= 0: the default, 32768 pairs);
 * -1: refused / bad sizes.  ps_rtm_rank_all sizes its passes from the scratch it is given: the most items that fit. */
int64_t ps_rtm_rank_scratch_bytes(const PsRtmDesc* desc, const PsRtmRankShape* shape, int32_t topk, int64_t items_per_pass);
/* What ps_rtm_rank_all launches for this descriptor, shape, topk and scratch size, from the rules the launcher itself reads
 * (csrc/rtm_rank.hip: rr_pass_layout, rr_epl, rr_lph, rr_items_per_workgroup, rr_pair_lds, rr_tail_fused, rr_query_fs_fused).  Host only: no
 * HIP call, works without a device; reads the process's switches (PS_NO_FUSE).  Refused as ps_rtm_rank_all refuses. */
typedef struct PsRtmRankPlan {
  int64_t items_per_pass;       /* items scored per pass: the most whose pairs fit the scratch                         */
  int64_t passes;               /* ceil(n_items / items_per_pass)                                                      */
  int32_t epl;                  /* d / 64: columns per lane, the instantiation of rr_entry_kernel / rr_pair_kernel     */
  int32_t lph;                  /* 64 / H: lanes per head, the width of the cross-lane sum of a logit                  */
  int32_t items_per_workgroup;  /* items whose K / V rows one workgroup of rr_pair_kernel holds in LDS                 */
  int32_t lds_bytes;            /* that tile's dynamic LDS; above 64 KB the launcher raises the kernel's limit first   */
  int32_t tail_fused;           /* the per-pair tail is the fused d = 128 kernel (0: GEMMs and row kernels)            */
  int32_t query_fs_fused;       /* the fs query encoder's projection runs inside the embed launch (0: a GEMM, or avg)  */
} PsRtmRankPlan;
int ps_rtm_rank_plan(const PsRtmDesc* desc, const PsRtmRankShape* shape, int32_t topk, int64_t scratch_bytes, PsRtmRankPlan* out);
/* item_ridxs [P, I]; query_word_idxs [B, Q]; u_ridxs [B, U]; target_prod_idxs [B] (NULL: no rank).  top_idx / top_score
 * [B, topk], rank [B]: the semantics of ps_rank_all (score desc, id asc; rank 1-based, 0: the target is not an item;
 * topk <= 256; unfilled slots -1 / -inf).  scores_out (optional) [B, P] dense.  scratch: 256-byte aligned. */
int ps_rtm_rank_all(const PsRtmDesc* desc, const PsRtmRankShape* shape, const PsRtmTensors* params, const float* index,
                    const int64_t* item_ridxs, const int64_t* query_word_idxs, const int64_t* u_ridxs,
                    const int64_t* target_prod_idxs, int32_t topk, int64_t* top_idx, float* top_score, int32_t* rank,
                    float* scores_out, void* scratch, int64_t scratch_bytes, ps_stream_t stream);
/* The same pass over per-entry candidate lists (sampled validation, the rerank of --test_candi_size lists): the entries of
 * include/prodsearch_rtm_cand.h, which take this section's descriptor, shape and index. */

/* Host evaluation of the dropout stream (tests pin oracle/philox.py to it): multiplier
 * (0 or 1/(1-p)) of element (row, col) of dropout site `site` at desc->seed/step/dropout. */
float ps_dropout_mult_host(const PsTemDesc* desc, uint32_t site, uint32_t row, uint32_t col);

/* Measurement hook (bench.py's roofline): while armed, the launch sites of ONE tagged kernel ("gather_score", "mlp_fwd",
 * "mlp_bwd", "rtm_embed") bracket every launch with a HIP event pair recorded on the launch stream, up to max_samples;
 * ps_ktimer_read synchronises, returns the average / minimum duration in microseconds and disarms.  tag NULL: disarm. */
int ps_ktimer_arm(const char* tag, int32_t max_samples);
int ps_ktimer_read(double* avg_us, double* min_us, int32_t* count);

/* Tuning knob (no reference counterpart): weight-gradient groups with row-list members at d = 128 (K / V / Q and the deferred
 * K / V / Q / f_W group) give every member its own split count in one flat launch (default 1, env PS_KVQ_SPLIT; 0 = one common
 * count on the 3-D grid).  Deterministic mode never takes the form.  Returns the previous value. */
int ps_set_kvq_split(int on);
/* Unit-test hook of the grouped weight-gradient launch: member i (n <= 4) adds dY[i][rows[i], n_out]^T . X[i][rows[i], k_in] onto
 * dW[i][n_out, k_in]; listed[i] != 0: over the *rcount rows ridx[0 .. *rcount) only (device memory; rows[i] bounds the list, ridx has
 * room for rows[i] entries).  ks_listed / ks_plain > 0 replace the per-member split counts where that form is taken. */
int ps_wgrad_group_test(int n, const float* const* dY, const float* const* X, float* const* dW, const int32_t* rows,
                        const int32_t* listed, const int32_t* ridx, const int32_t* rcount, int n_out, int k_in,
                        int ks_listed, int ks_plain, ps_stream_t stream);

/* Unit-test hook of the fp32 MFMA GEMM: C[M,N] = alpha * op(A) op(B) (+bias) (+C if accumulate).
 * ta: A stored [K,M];  tb==0: B stored [N,K] (nn.Linear), tb==1: B stored [K,N]. */
int ps_gemm_f32(const float* A, int lda, int ta, const float* Bm, int ldb, int tb,
                float* Cm, int ldc, int M, int N, int K, const float* bias, float alpha,
                int accumulate, ps_stream_t stream);

/* ------------------------------------------------------------------ several tables in one coalesce
 * A model with several row-sparse tables (the review transformer: review / user / item / word) builds all its touched lists
 * in THREE launches instead of three per table (ps_coalesce_rows is this entry with one table).  Each entry is what one
 * ps_coalesce_rows call takes — 1..8 index lists,
 * n_rows, pad_row, the table's own workspace (ps_coalesce_ws_bytes, zeroed once, left zeroed), rows_out / cap / count_out —
 * and gets what that call gives: the sorted unique non-pad ids, bit for bit, and the same status word (ps_coalesce_bad_flag:
 * 1 an id outside [0, n_rows) was dropped, 2 more unique rows than cap), set for that table only.  n_tabs 1..4. */
typedef struct PsCoalesceTable {
  PsIdxList lists[8];
  int32_t n_lists;
  int32_t pad_;
  int64_t n_rows, pad_row;
  void* ws_dev;
  int64_t* rows_out_dev;
  int64_t cap;
  int32_t* count_out_dev;
} PsCoalesceTable;
int ps_coalesce_tables(const PsCoalesceTable* tabs_host, int32_t n_tabs, ps_stream_t stream);

/* ------------------------------------------------------------------ several tables in one row exchange
 * The data-parallel row exchange of ps_pack_rows / ps_coalesce_rows / ps_merge_rows for a model with several row-sparse
 * tables: ONE message per rank, ONE all-gather, one pack launch, one union (three launches) and one merge launch per step.
 * A rank's message is one byte buffer: for tables t = 0 .. n_tabs-1 first the id sections (cap_t int64: the rank's ascending
 * touched ids, then -1), then the value sections (cap_t x d_t fp32: their gradient rows, then zeros).  Every section starts
 * on a 16-byte boundary (the 8 bytes after an id section of odd capacity are written as -1) and the total is a multiple of 16, so slot r of the gathered [world, msg_bytes] buffer is aligned
 * like the message; the bytes are a function of the gradient only.  ps_row_msg_layout is host-only arithmetic: the section
 * offsets and the total from (cap_t, d_t); -1 (and ps_last_error) on a bad argument.  The three entries derive the same
 * layout from their tables and refuse a msg_bytes that differs.  n_tabs 1..4, d % 4 == 0, world 1..32. */
typedef struct PsRowMsgTable {
  int64_t cap;                 /* message capacity in rows: the same on every rank */
  int32_t d;
  int32_t pad_;
  int64_t n_rows;
  float* grad_dev;             /* [n_rows, d] dense gradient: ps_pack_tables reads it, ps_merge_tables writes the union's rows */
  const int64_t* rows_dev;     /* this rank's touched list (ps_coalesce_*): list_cap entries, *count_dev of them live */
  const int32_t* count_dev;
  int64_t list_cap;            /* <= cap */
  void* ws_dev;                /* union: a ps_coalesce_ws_bytes(n_rows) workspace of its own (zeroed once, left zeroed) */
  int64_t* union_rows_dev;     /* union_cap entries: the sorted unique ids over the ranks' sections */
  int64_t union_cap;
  int32_t* union_count_dev;
} PsRowMsgTable;
int64_t ps_row_msg_layout(const int64_t* caps_host, const int32_t* ds_host, int32_t n_tabs, int64_t* ids_off_out,
                          int64_t* vals_off_out);
/* msg_dev[msg_bytes] <- this rank's message.  Slots past *count_dev are written as -1 / zeros whatever the buffer held. */
int ps_pack_tables(const PsRowMsgTable* tabs_host, int32_t n_tabs, void* msg_dev, int64_t msg_bytes, ps_stream_t stream);
/* Per table the sorted unique ids over the `world` id sections of all_dev [world, msg_bytes] -> union_rows / union_count.
 * Workspace, status word (ps_coalesce_bad_flag: 1 an id outside [0, n_rows), 2 more unique ids than union_cap — the call
 * still returns PS_OK, the ids that fit are written, *union_count is the full count) and output are ps_coalesce_rows' own. */
int ps_union_tables(const PsRowMsgTable* tabs_host, int32_t n_tabs, const void* all_dev, int64_t msg_bytes, int32_t world,
                    ps_stream_t stream);
/* grad[union row, :] = sum over ranks 0 .. world-1, in that order, of the rows the ranks sent for it (ps_merge_rows'
 * arithmetic): bitwise the same on every rank.  Rows outside the union are not touched. */
int ps_merge_tables(const PsRowMsgTable* tabs_host, int32_t n_tabs, const void* all_dev, int64_t msg_bytes, int32_t world,
                    ps_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PRODSEARCH_HIP_H */
