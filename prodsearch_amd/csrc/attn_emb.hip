// attn_emb.hip — the attention-embedding models of the Zero Attention Model paper (ZAM / AEM): ItemTransformerRanker.forward_attn
// / test_attn with model_name 'ZAM' or 'AEM' (item_transformer.py:148-195, 361-438), one MultiHeadedAttention
// (neural.py:192-231) whose single query is the encoded search query and whose keys / values are the user's purchase history.
//
//   h_s   = hist_tab[u_item_idxs[b, s]]            (ZAM: a zero row prepended at s = 0, always valid; S = L + 1, else S = L)
//   K, V  = h Wk^T + bk, h Wv^T + bv              once per batch row (all replicas share them)
//   q_s   = (query_emb Wq^T + bq) / sqrt(dh)      once per batch row
//   P     = softmax(masked_fill(q_s . K^T, -1e18)) once per batch row and head
//   ctx_j = dropout_j(P) . V                      per replica j (j = 0 positive, 1 + k negative k; one replica without dropout)
//   out_j = 0.5 (ctx_j Wo^T + bo) + 0.5 query_emb
//
// The attention dropout of replica j, head h, key s (original key index, ZAM's zero column at s = 0) is element
// (row = (b R + j) H + h, col = s) of the Philox site PS_SITE_ATTN(0) — oracle/philox.py's PhiloxDropout with n_layers = 1.
// AEM rows without history: every key is masked, the -1e18 fill gives uniform weights over the L pad positions (their values
// are projections of the pad row), and no score gradient flows (masked_fill blocks it) — both fall out of the code below,
// which never drops masked keys from the softmax.
//
// Launches (forward): history gather, K / V / Q products (fp32-grade GEMMs, gemm.hip), one attention workgroup per batch row,
// the per-replica final_linear product with the 0.5 residual in its epilogue.  Backward: the halved d out and its replica
// fan-in, d ctx = dhalf Wo, the attention backward (one workgroup per batch row), deterministic bias column sums, the weight
// gradients and the d h / d query products, then the history-row scatter into the table.
#include "encoder.h"
#include "wgrad.h"
#include <string.h>

#define AE_THREADS 256
#define AE_AM_FLOATS 4096        // LDS floats of dropout weights per chunk of replicas
#define AE_COL_SPLITS PS_AE_COL_SPLITS   // row splits of the deterministic bias column sums (encoder.h)

bool ps_model_attn(int model) { return model == PS_MODEL_AEM || model == PS_MODEL_ZAM; }
int ae_zoff(const PsTemDesc& D) { return D.model == PS_MODEL_ZAM ? 1 : 0; }

static int ae_jc(int R, int HS) {
  int jc = AE_AM_FLOATS / HS;
  if (jc < 1) jc = 1;
  return jc < R ? jc : R;
}

// x[b*S + s] = hist_tab[u_item_idxs[b, s - zoff]] (s >= zoff), 0 for ZAM's zero column
__global__ __launch_bounds__(AE_THREADS) void ae_gather_kernel(const int64_t* ui, const float* hist, int B, int S, int L, int zoff,
                                                              int d, int64_t P, float* x) {
  const int n4 = d >> 2;
  const int64_t i = (int64_t)blockIdx.x * AE_THREADS + threadIdx.x;
  if (i >= (int64_t)B * S * n4) return;
  const int64_t row = i / n4;
  const int c = (int)(i - row * n4);
  const int b = (int)(row / S), s = (int)(row - (int64_t)b * S);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s >= zoff) {
    int64_t id = ui[(size_t)b * L + s - zoff];
    id = (id < 0 || id > P) ? P : id;
    v = reinterpret_cast<const float4*>(hist + (size_t)id * d)[c];
  }
  reinterpret_cast<float4*>(x)[i] = v;
}

struct AeAttnArgs {
  int B, S, L, zoff, d, H, dh, R, JC;
  int64_t P;
  const int64_t* ui;
  const float *kp, *vp, *qp;      // [B*S,d], [B*S,d], [B,d] (q already scaled by 1/sqrt(dh))
  const float* query_emb;         // [B,d]
  float* attn;                    // [B,H,S] softmax output (pre-dropout)
  float* ctx;                     // [B*R,d]
  float* qhalf;                   // [B,d] 0.5 * query_emb: the residual of final_linear's epilogue
  DropSpec drop;
  // backward
  const float* dctx;              // [B*R,d]
  float *dk, *dv, *dqp;           // [B*S,d], [B*S,d], [B,d] (d of the UNscaled query projection)
  float qscale;                   // 1/sqrt(dh)
  int32_t *keys, *rowidx;         // [B*L] deterministic scatter tasks: table row (-1: none) and row of d h
};

__device__ inline bool ae_valid(const AeAttnArgs& a, int b, int s) {
  return s < a.zoff || a.ui[(size_t)b * a.L + s - a.zoff] != a.P;
}

// one workgroup per batch row: scores, masked softmax, then the replicas' dropout-weighted sums of V
__global__ __launch_bounds__(AE_THREADS) void ae_attn_fwd_kernel(AeAttnArgs a) {
  extern __shared__ float lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int S = a.S, d = a.d, H = a.H, dh = a.dh, HS = H * S;
  float* p = lds;                              // [H][S]
  float* am = p + HS;                          // [JC][H][S]
  int* valid = reinterpret_cast<int*>(am + a.JC * HS);
  for (int s = tid; s < S; s += AE_THREADS) valid[s] = ae_valid(a, b, s) ? 1 : 0;
  for (int c = tid; c < d; c += AE_THREADS) a.qhalf[(size_t)b * d + c] = 0.5f * a.query_emb[(size_t)b * d + c];
  __syncthreads();
  const float* q = a.qp + (size_t)b * d;
  const float* k = a.kp + (size_t)b * S * d;
  const float* v = a.vp + (size_t)b * S * d;
  for (int t = tid; t < HS; t += AE_THREADS) {
    const int h = t / S, s = t - h * S;
    float acc = 0.f;
    for (int e = 0; e < dh; ++e) acc += q[h * dh + e] * k[(size_t)s * d + h * dh + e];
    p[t] = valid[s] ? acc : -1e18f;
  }
  __syncthreads();
  for (int h = tid; h < H; h += AE_THREADS) {
    float* ph = p + h * S;
    float m = ph[0];
    for (int s = 1; s < S; ++s) m = fmaxf(m, ph[s]);
    float sum = 0.f;
    for (int s = 0; s < S; ++s) { const float e = expf(ph[s] - m); ph[s] = e; sum += e; }
    const float inv = 1.f / sum;
    for (int s = 0; s < S; ++s) ph[s] *= inv;
  }
  __syncthreads();
  for (int t = tid; t < HS; t += AE_THREADS) a.attn[(size_t)b * HS + t] = p[t];
  for (int j0 = 0; j0 < a.R; j0 += a.JC) {
    const int jn = a.R - j0 < a.JC ? a.R - j0 : a.JC;
    for (int t = tid; t < jn * HS; t += AE_THREADS) {
      const int jj = t / HS, r = t - jj * HS, h = r / S, s = r - h * S;
      const uint32_t row = (uint32_t)(((int64_t)b * a.R + j0 + jj) * H + h);
      am[t] = p[r] * drop_mult(a.drop, row, (uint32_t)s);
    }
    __syncthreads();
    for (int t = tid; t < jn * d; t += AE_THREADS) {
      const int jj = t / d, c = t - jj * d, h = c / dh;
      const float* w = am + jj * HS + h * S;
      float acc = 0.f;
      for (int s = 0; s < S; ++s) acc += w[s] * v[(size_t)s * d + c];
      a.ctx[((size_t)b * a.R + j0 + jj) * d + c] = acc;
    }
    __syncthreads();
  }
}

// dhalf = 0.5 d out (the final_linear branch's gradient), dqe[b] = sum_j dhalf[b R + j] (the residual branch's, in replica order)
__global__ __launch_bounds__(AE_THREADS) void ae_half_kernel(const float* denc, int B, int R, int d, float* dhalf, float* dqe) {
  const int64_t i = (int64_t)blockIdx.x * AE_THREADS + threadIdx.x;
  if (i >= (int64_t)B * d) return;
  const int b = (int)(i / d), c = (int)(i - (int64_t)b * d);
  float s = 0.f;
  for (int j = 0; j < R; ++j) {
    const size_t o = ((size_t)b * R + j) * d + c;
    const float v = 0.5f * denc[o];
    dhalf[o] = v;
    s += v;
  }
  dqe[i] = s;
}

// one workgroup per batch row: d P through the replicas' masks, softmax backward, d q, d K, d V
__global__ __launch_bounds__(AE_THREADS) void ae_attn_bwd_kernel(AeAttnArgs a) {
  extern __shared__ float lds[];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int S = a.S, d = a.d, H = a.H, dh = a.dh, HS = H * S;
  float* p = lds;                              // [H][S]
  float* dP = p + HS;                          // [H][S]: d P, then d scores
  float* am = dP + HS;                         // [JC][H][S] dropout multipliers
  int* valid = reinterpret_cast<int*>(am + a.JC * HS);
  for (int s = tid; s < S; s += AE_THREADS) valid[s] = ae_valid(a, b, s) ? 1 : 0;
  for (int t = tid; t < HS; t += AE_THREADS) { p[t] = a.attn[(size_t)b * HS + t]; dP[t] = 0.f; }
  if (a.keys)
    for (int l = tid; l < a.L; l += AE_THREADS) {
      const int64_t id = a.ui[(size_t)b * a.L + l];
      a.keys[(size_t)b * a.L + l] = (id >= 0 && id < a.P) ? (int32_t)id : -1;
      a.rowidx[(size_t)b * a.L + l] = b * S + l + a.zoff;
    }
  __syncthreads();
  const float* k = a.kp + (size_t)b * S * d;
  const float* v = a.vp + (size_t)b * S * d;
  const float* dc = a.dctx + (size_t)b * a.R * d;
  float* dv = a.dv + (size_t)b * S * d;
  for (int j0 = 0; j0 < a.R; j0 += a.JC) {
    const int jn = a.R - j0 < a.JC ? a.R - j0 : a.JC;
    for (int t = tid; t < jn * HS; t += AE_THREADS) {
      const int jj = t / HS, r = t - jj * HS, h = r / S, s = r - h * S;
      const uint32_t row = (uint32_t)(((int64_t)b * a.R + j0 + jj) * H + h);
      am[t] = drop_mult(a.drop, row, (uint32_t)s);
    }
    __syncthreads();
    for (int r = tid; r < HS; r += AE_THREADS) {      // d P[h][s] += sum_j m_j (d ctx_j,h . V_s,h)
      const int h = r / S, s = r - h * S;
      const float* vs = v + (size_t)s * d + h * dh;
      float acc = dP[r];
      for (int jj = 0; jj < jn; ++jj) {
        const float m = am[jj * HS + r];
        if (m == 0.f) continue;
        const float* g = dc + (size_t)(j0 + jj) * d + h * dh;
        float dot = 0.f;
        for (int e = 0; e < dh; ++e) dot += g[e] * vs[e];
        acc += m * dot;
      }
      dP[r] = acc;
    }
    for (int t = tid; t < S * d; t += AE_THREADS) {   // d V[s][c] += sum_j P m_j d ctx_j
      const int s = t / d, c = t - s * d, h = c / dh;
      float acc = j0 == 0 ? 0.f : dv[t];
      for (int jj = 0; jj < jn; ++jj) acc += p[h * S + s] * am[jj * HS + h * S + s] * dc[(size_t)(j0 + jj) * d + c];
      dv[t] = acc;
    }
    __syncthreads();
  }
  for (int h = tid; h < H; h += AE_THREADS) {         // softmax backward; masked keys take no score gradient (masked_fill)
    float dot = 0.f;
    for (int s = 0; s < S; ++s) dot += p[h * S + s] * dP[h * S + s];
    for (int s = 0; s < S; ++s) dP[h * S + s] = valid[s] ? p[h * S + s] * (dP[h * S + s] - dot) : 0.f;
  }
  __syncthreads();
  const float* qs = a.qp + (size_t)b * d;
  for (int c = tid; c < d; c += AE_THREADS) {
    const int h = c / dh;
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += dP[h * S + s] * k[(size_t)s * d + c];
    a.dqp[(size_t)b * d + c] = acc * a.qscale;
  }
  float* dk = a.dk + (size_t)b * S * d;
  for (int t = tid; t < S * d; t += AE_THREADS) {
    const int s = t / d, c = t - s * d;
    dk[t] = dP[(c / dh) * S + s] * qs[c];
  }
}

// out[job][c] += sum over rows of X[job][row][c], in a fixed order (two passes: row splits, then the splits in order)
struct AeColJobs {
  const float* X[4]; int rows[4]; float* out[4];
  float* part;                     // [4][AE_COL_SPLITS][d]
  int d, n;
};
__global__ __launch_bounds__(AE_THREADS) void ae_colsum_part_kernel(AeColJobs a) {
  const int job = blockIdx.z, sp = blockIdx.x, c = blockIdx.y * AE_THREADS + threadIdx.x;
  if (c >= a.d) return;
  const int rows = a.rows[job];
  const int r0 = (int)((int64_t)rows * sp / AE_COL_SPLITS), r1 = (int)((int64_t)rows * (sp + 1) / AE_COL_SPLITS);
  const float* X = a.X[job];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int r = r0;
  for (; r + 4 <= r1; r += 4) {
    s0 += X[(size_t)r * a.d + c]; s1 += X[(size_t)(r + 1) * a.d + c];
    s2 += X[(size_t)(r + 2) * a.d + c]; s3 += X[(size_t)(r + 3) * a.d + c];
  }
  for (; r < r1; ++r) s0 += X[(size_t)r * a.d + c];
  a.part[((size_t)job * AE_COL_SPLITS + sp) * a.d + c] = (s0 + s1) + (s2 + s3);
}
__global__ __launch_bounds__(AE_THREADS) void ae_colsum_fin_kernel(AeColJobs a) {
  const int job = blockIdx.y, c = blockIdx.x * AE_THREADS + threadIdx.x;
  if (c >= a.d) return;
  float s = 0.f;
  for (int sp = 0; sp < AE_COL_SPLITS; ++sp) s += a.part[((size_t)job * AE_COL_SPLITS + sp) * a.d + c];
  a.out[job][c] += s;
}

// table[keys] += d h rows (atomics; deterministic mode takes launch_rows_scatter_det)
__global__ __launch_bounds__(AE_THREADS) void ae_scatter_kernel(const int64_t* ui, const float* dh, int B, int S, int L, int zoff,
                                                               int d, int64_t P, float* table) {
  const int64_t i = (int64_t)blockIdx.x * AE_THREADS + threadIdx.x;
  if (i >= (int64_t)B * L * d) return;
  const int64_t e = i / d;
  const int c = (int)(i - e * d);
  const int64_t id = ui[e];
  if (id < 0 || id >= P) return;                     // the pad row's gradient stays zero (padding_idx)
  const int b = (int)(e / L), l = (int)(e - (int64_t)b * L);
  atomicAdd(table + (size_t)id * d + c, dh[((size_t)b * S + l + zoff) * d + c]);
}

static AeAttnArgs ae_args(const PsTemDesc& D, const int64_t* ui, float* ws, const Ws& w) {
  AeAttnArgs a;
  memset(&a, 0, sizeof(a));
  const LayerWs& l = w.layer[0];
  a.B = D.B; a.S = w.S; a.L = D.L; a.zoff = ae_zoff(D); a.d = D.d; a.H = D.H; a.dh = D.d / D.H; a.R = w.R;
  a.JC = ae_jc(w.R, D.H * w.S);
  a.P = D.product_size; a.ui = ui;
  a.kp = ws + l.kp; a.vp = ws + l.vp; a.qp = ws + l.qp;
  a.query_emb = ws + w.query_emb; a.attn = ws + l.attn; a.ctx = ws + l.ctx; a.qhalf = ws + w.ae_qhalf;
  a.drop = make_drop(D, PS_SITE_ATTN(0));
  a.qscale = 1.f / sqrtf((float)a.dh);
  return a;
}

// forward: reads w.query_emb, writes w.enc [B*R, d]
int ae_forward(const EncCall& c) {
  const PsTemDesc& D = c.D; const PsTemTensors& P = c.P; const int64_t* ui = c.ui; float* ws = c.ws; const Ws& w = c.w; hipStream_t st = c.st;
  const PsLayerTensors& A = P.layer[0];
  PS_REQUIRE(ui, "forward: null u_item_idxs");
  PS_REQUIRE(A.wk && A.bk && A.wv && A.bv && A.wq && A.bq && A.wo && A.bo, "forward: null attention_encoder tensors (layer[0])");
  const float* hist = D.sep_prod_emb ? P.hist_product_emb : P.product_emb;
  const int B = D.B, d = D.d, S = w.S;
  const LayerWs& l = w.layer[0];
  const int64_t n4 = (int64_t)B * S * d / 4;
  hipLaunchKernelGGL(ae_gather_kernel, dim3((unsigned)ps_cdiv(n4, AE_THREADS)), dim3(AE_THREADS), 0, st, ui, hist, B, S, D.L,
                     ae_zoff(D), d, D.product_size, ws + w.x);
  PS_LAUNCH_CHECK();
  AeAttnArgs a = ae_args(D, ui, ws, w);
  {   // linear_keys / linear_values over every key row (ZAM's zero row gives the bias), linear_query / sqrt(dh)
    GemmProblem pk = gp(ws + w.x, d, 0, A.wk, d, 0, ws + l.kp, d, B * S, d, d);
    pk.bias = A.bk;
    TRY(run1(pk, st));
    GemmProblem pv = gp(ws + w.x, d, 0, A.wv, d, 0, ws + l.vp, d, B * S, d, d);
    pv.bias = A.bv;
    TRY(run1(pv, st));
    GemmProblem pq = gp(ws + w.query_emb, d, 0, A.wq, d, 0, ws + l.qp, d, B, d, d);
    pq.bias = A.bq; pq.alpha = a.qscale;
    TRY(run1(pq, st));
  }
  const size_t lds = sizeof(float) * ((size_t)(1 + a.JC) * D.H * S + S);
  hipLaunchKernelGGL(ae_attn_fwd_kernel, dim3(B), dim3(AE_THREADS), lds, st, a);
  PS_LAUNCH_CHECK();
  {   // out = 0.5 (ctx Wo^T + bo) + 0.5 query_emb: alpha then the residual row b = m / R of qhalf
    GemmProblem po = gp(ws + l.ctx, d, 0, A.wo, d, 0, ws + w.enc, d, B * w.R, d, d);
    po.bias = A.bo; po.alpha = 0.5f;
    po.res.mode = RES_GATHER; po.res.ptr = ws + w.ae_qhalf; po.res.ld = d;
    po.res.Sq = 1; po.res.fan = w.R; po.res.S = 1; po.res.qpos = 0; res_finish(po.res);
    TRY(run1(po, st));
  }
  return PS_OK;
}

// backward: reads w.denc (d out, [B*R,d]); accumulates the attention_encoder gradients into G.layer[0] and the history rows'
// into the history table; leaves d query_emb in w.ae_dqe [B,d]
int ae_backward(const EncCall& call, const PsTemTensors& G) {
  const PsTemDesc& D = call.D; const PsTemTensors& P = call.P; const int64_t* ui = call.ui; float* ws = call.ws; const Ws& w = call.w; hipStream_t st = call.st;
  const PsLayerTensors& A = P.layer[0];
  const PsLayerTensors& GA = G.layer[0];
  PS_REQUIRE(ui, "backward: null u_item_idxs");
  PS_REQUIRE(GA.wk && GA.bk && GA.wv && GA.bv && GA.wq && GA.bq && GA.wo && GA.bo,
             "backward: null attention_encoder gradients (layer[0])");
  float* ghist = D.sep_prod_emb ? G.hist_product_emb : G.product_emb;
  const int B = D.B, d = D.d, S = w.S, R = w.R;
  const LayerWs& l = w.layer[0];
  float* dhalf = ws + w.ae_dhalf;
  float* dqe = ws + w.ae_dqe;
  hipLaunchKernelGGL(ae_half_kernel, dim3((unsigned)ps_cdiv((int64_t)B * d, AE_THREADS)), dim3(AE_THREADS), 0, st, ws + w.denc,
                     B, R, d, dhalf, dqe);
  PS_LAUNCH_CHECK();
  {   // d ctx = dhalf . Wo ; dWo += dhalf^T ctx
    GemmProblem p = gp(dhalf, d, 0, A.wo, d, 1, ws + w.dctx, d, B * R, d, d);
    TRY(run1(p, st));
    GemmProblem g = gp_wgrad(dhalf, d, ws + l.ctx, d, GA.wo, d, d, B * R);
    TRY(run_wgrads(&g, 1, st));
  }
  AeAttnArgs a = ae_args(D, ui, ws, w);
  a.dctx = ws + w.dctx; a.dk = ws + w.ae_dk; a.dv = ws + w.ae_dv; a.dqp = ws + w.ae_dqp;
  const bool det = ps_deterministic();
  if (det) { a.keys = reinterpret_cast<int32_t*>(ws + w.ae_keys); a.rowidx = a.keys + (size_t)B * D.L; }
  const size_t lds = sizeof(float) * ((size_t)(2 + a.JC) * D.H * S + S);
  hipLaunchKernelGGL(ae_attn_bwd_kernel, dim3(B), dim3(AE_THREADS), lds, st, a);
  PS_LAUNCH_CHECK();
  {   // bias gradients: bo (sum of dhalf over all replica rows = sum of dqe over rows), bq, bk, bv
    AeColJobs c;
    memset(&c, 0, sizeof(c));
    c.X[0] = dqe;          c.rows[0] = B;     c.out[0] = GA.bo;
    c.X[1] = a.dqp;        c.rows[1] = B;     c.out[1] = GA.bq;
    c.X[2] = a.dk;         c.rows[2] = B * S; c.out[2] = GA.bk;
    c.X[3] = a.dv;         c.rows[3] = B * S; c.out[3] = GA.bv;
    c.part = ws + w.ae_part; c.d = d; c.n = 4;
    hipLaunchKernelGGL(ae_colsum_part_kernel, dim3(AE_COL_SPLITS, ps_cdiv(d, AE_THREADS), 4), dim3(AE_THREADS), 0, st, c);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(ae_colsum_fin_kernel, dim3(ps_cdiv(d, AE_THREADS), 4), dim3(AE_THREADS), 0, st, c);
    PS_LAUNCH_CHECK();
  }
  {   // dWk += dK^T h, dWv += dV^T h (one launch), dWq += dQ^T query_emb
    GemmProblem g[2] = {gp_wgrad(a.dk, d, ws + w.x, d, GA.wk, d, d, B * S), gp_wgrad(a.dv, d, ws + w.x, d, GA.wv, d, d, B * S)};
    TRY(run_wgrads(g, 2, st));
    GemmProblem gq = gp_wgrad(a.dqp, d, ws + w.query_emb, d, GA.wq, d, d, B);
    TRY(run_wgrads(&gq, 1, st));
  }
  {   // d h = dK . Wk + dV . Wv ; d query_emb += dQ . Wq
    GemmProblem p1 = gp(a.dk, d, 0, A.wk, d, 1, ws + w.dx, d, B * S, d, d);
    TRY(run1(p1, st));
    GemmProblem p2 = gp(a.dv, d, 0, A.wv, d, 1, ws + w.dx, d, B * S, d, d);
    p2.accumulate = 1;
    TRY(run1(p2, st));
    GemmProblem p3 = gp(a.dqp, d, 0, A.wq, d, 1, dqe, d, B, d, d);
    p3.accumulate = 1;
    TRY(run1(p3, st));
  }
  if (D.L > 0) {
    if (det) {
      TRY(launch_rows_scatter_det(a.keys, B * D.L, ws + w.dx, d, d, ghist, st, nullptr, a.rowidx));
    } else {
      const int64_t n = (int64_t)B * D.L * d;
      hipLaunchKernelGGL(ae_scatter_kernel, dim3((unsigned)ps_cdiv(n, AE_THREADS)), dim3(AE_THREADS), 0, st, ui, ws + w.dx, B, S,
                         D.L, ae_zoff(D), d, D.product_size, ghist);
      PS_LAUNCH_CHECK();
    }
  }
  return PS_OK;
}
