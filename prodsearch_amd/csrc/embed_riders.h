// embed_riders.h — the work that rides in the forward's first launch beside the sequences' workgroups (EmbedArgs, rowwise.h): the
// step's negative draws, the valid-row list, the loss's word tasks and the int32 clear, each written for a block of 256 threads
// (`tid` = the thread's index in it).  Two launches carry them: embed_fwd_kernel (rowwise.hip: one block = one workgroup) and the
// fused front end (attn_sq1.hip: a workgroup of 512 threads runs two blocks side by side).  The weight re-split is wsplit_chunk.
#pragma once
#include "rowwise.h"

__device__ inline int64_t clamp_idx(int64_t i, int64_t hi) { return i < 0 ? hi : (i > hi ? hi : i); }

struct Task {
  const float* row; const float* vec; float bias; float* out;
  float* term; float tw;     // loss term = |tw| * softplus(sign(tw) * score): tw < 0 for the positive
  float lw;                  // weight of the term in the batch loss: item tasks +1; word tasks -(valid / #valid windows)
};
__device__ __forceinline__ Task score_task(const ScoreArgs& a, int t) {
  Task k;
  const int K1 = a.K + 1;
  if (a.C > 0) {                                   // eval: candidates
    int b = fdiv(t, a.fC);
    int64_t idx = clamp_idx(a.candi[t], a.P);
    k.row = a.product_emb + (size_t)idx * a.d;
    k.vec = a.enc + (size_t)b * a.R * a.d;
    k.bias = a.bias_product ? a.product_bias[idx] : 0.f;
    k.out = a.item_scores + t;
    k.term = nullptr; k.tw = 0.f; k.lw = 0.f;
    return k;
  }
  const int nitem = a.B * K1;
  if (t < nitem) {
    int b = fdiv(t, a.fK1), j = t - b * K1;
    int64_t idx = clamp_idx(j == 0 ? a.target[b] : a.neg_items[(size_t)b * a.K + j - 1], a.P);
    k.row = a.product_emb + (size_t)idx * a.d;
    k.vec = a.enc + ((size_t)b * a.R + (a.R > 1 ? j : 0)) * a.d;
    k.bias = a.bias_product ? a.product_bias[idx] : 0.f;
    k.out = a.item_scores + t;
    k.term = a.item_terms + t;
    k.tw = j == 0 ? -(a.pos_weight ? (float)a.K : 1.f) : 1.f;
    k.lw = 1.f;
  } else {
    int u = t - nitem;
    int b = fdiv(u, a.fWK1), r = u - b * (a.W * K1);
    int w = fdiv(r, a.fK1), j = r - w * K1;
    int64_t widx;
    if (j == 0) widx = a.pos_words[(size_t)b * a.W + w];
    else if (a.samp_inline) {                      // the draw sample_kernel makes for this slot (same stream, same table)
      const uint32_t su = (uint32_t)(b * a.W * a.K + w * a.K + j - 1);
      Philox4 rr = philox4x32_10(su, 0u, PS_SITE_SAMPLE_WORD, a.samp_step, a.samp_k0, a.samp_k1);
      const int64_t i = (int64_t)(((uint64_t)rr.x * (uint64_t)a.V) >> 32);
      const float f = (float)(rr.y >> 8) * (1.0f / 16777216.0f);
      widx = f < a.samp_prob[i] ? i : (int64_t)a.samp_alias[i];
    } else widx = a.neg_words[(size_t)b * a.W * a.K + (size_t)w * a.K + j - 1];
    int64_t idx = clamp_idx(widx, a.V - 1);
    int64_t tb = clamp_idx(a.target[b], a.P);
    k.row = a.word_emb + (size_t)idx * a.d;
    k.vec = a.product_emb + (size_t)tb * a.d;
    k.bias = a.word_bias[idx];
    k.out = a.word_scores + u;
    k.term = a.word_terms + u;
    k.tw = j == 0 ? -1.f : 1.f;
    // masked mean over the window (get_vector_mean, item_transformer.py:281): padded slots drop out
    int cnt = 0;
    for (int ww = 0; ww < a.W; ++ww) cnt += a.pos_words[(size_t)b * a.W + ww] != a.V - 1;
    const bool valid = a.pos_words[(size_t)b * a.W + w] != a.V - 1;
    k.lw = valid ? -1.f / (float)cnt : -0.f;
  }
  return k;
}

// Word tasks of the loss (ScoreArgs, folded form): 16 lanes per task (rows of d <= 512 floats in 16-byte chunks), 16 tasks per
// pass, PS_WORD_TASKS_PER_WG tasks per block; one {il} partial per block in word_blk[wg].  `wred`: 16 floats of LDS of the
// block's own.  Every thread of the workgroup must arrive (one __syncthreads); a block past the last one (wg >= word_nblk) writes nothing.
__device__ __forceinline__ void word_tasks_wg(const ScoreArgs& a, int wg, int tid, float* wred) {
  const int grp = tid >> 4, c = tid & 15;
  const int nitem = a.B * (a.K + 1), nword = a.B * a.W * (a.K + 1);
  const int nch = a.d >> 2;
  float cil = 0.f;
  if (wg == 0 && tid < 18) a.ticket[tid] = 0u;         // the fused kernel's 9 arrival / partial-sum words, reset once per step
  for (int pass = 0; pass < PS_WORD_TASKS_PER_WG / 16; ++pass) {
    const int u = wg * PS_WORD_TASKS_PER_WG + pass * 16 + grp;
    float s = 0.f;
    Task k;
    k.out = nullptr;
    if (u < nword) {
      k = score_task(a, nitem + u);
      for (int cc = c; cc < nch; cc += 16) {
        const float4 r = *reinterpret_cast<const float4*>(k.row + 4 * cc);
        const float4 v = *reinterpret_cast<const float4*>(k.vec + 4 * cc);
        s += r.x * v.x + r.y * v.y + r.z * v.z + r.w * v.w;
      }
    }
    s = group_sum(s, 16);
    if (c == 0 && k.out) {
      const float sc = s + k.bias;
      *k.out = sc;
      const float term = fabsf(k.tw) * softplus_f(k.tw < 0.f ? -sc : sc);
      *k.term = term;
      cil -= term * k.lw;
    }
  }
  if (c == 0) wred[grp] = cil;
  __syncthreads();
  if (tid == 0 && wg < a.word_nblk) {
    float q = 0.f;
    for (int g2 = 0; g2 < 16; ++g2) q += wred[g2];
    a.word_blk[wg] = q;
  }
}

// the step's negative draws (EmbedArgs::samp_*): draw t of samp_nitem + samp_nword, the same as sample_kernel's
__device__ __forceinline__ void embed_sample_draw(const EmbedArgs a, int t)    /* (by value: through a reference the draws' int64 stores keep the whole struct in scratch) */ {
  if (t < a.samp_nitem) {
    Philox4 r = philox4x32_10((uint32_t)t, 0u, PS_SITE_SAMPLE_ITEM, a.samp_step, a.samp_k0, a.samp_k1);
    a.samp_items[t] = (int64_t)(((uint64_t)r.x * (uint64_t)a.P) >> 32);
  } else if (t < a.samp_nitem + a.samp_nword) {
    const int u = t - a.samp_nitem;
    Philox4 r = philox4x32_10((uint32_t)u, 0u, PS_SITE_SAMPLE_WORD, a.samp_step, a.samp_k0, a.samp_k1);
    const int64_t i = (int64_t)(((uint64_t)r.x * (uint64_t)a.V) >> 32);
    const float f = (float)(r.y >> 8) * (1.0f / 16777216.0f);
    a.samp_words[u] = f < a.samp_prob[i] ? i : (int64_t)a.samp_alias[i];
  }
}

// EmbedArgs::zero_i32: thread q of the clearing blocks owns four words
__device__ __forceinline__ void embed_zero_words(const EmbedArgs& a, int q) {
  const int i = q * 4;
  if (i + 3 < a.zero_n) *reinterpret_cast<int4*>(a.zero_i32 + i) = make_int4(0, 0, 0, 0);
  else for (int j = i; j < a.zero_n; ++j) a.zero_i32[j] = 0;
}

// Valid-row list (EmbedArgs::vrows), one block per sequence beside the gathering ones: this sequence's rows start behind the
// valid rows of all earlier sequences, counted here (b*L coalesced int64 reads, L2 hits) — no scan kernel, no host round trip,
// nothing added to the gather's own chain.  `vred`: 4 ints of LDS of the block's own; every thread of the workgroup must
// arrive (one __syncthreads); a block past the last sequence (b >= B) writes nothing.
__device__ __forceinline__ void embed_list_rows(const EmbedArgs& a, int b_in, int tid, int* vred) {
  const bool live = b_in < a.B;
  const int b = live ? b_in : 0;
  // (round 5: eight entries per lane and trip, four 16-byte loads in flight (eight measured the same) — as a loop of one 8-byte load per trip, each waited for,
  //  the last sequences' workgroups took 30 serial round trips at C2 and 80 at the C5 shard: the longest workgroups of the launch)
  int cntp = 0;
  {
    const int n = b * a.L;
    const bool al16 = (reinterpret_cast<uintptr_t>(a.ui) & 15) == 0;
    if (al16) {
      const longlong2* u2 = reinterpret_cast<const longlong2*>(a.ui);
      const int n2 = n >> 1;                                  // pairs; an odd last entry is counted below
      for (int i = tid; i < n2; i += 4 * 256) {
        longlong2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const int j = i + 256 * u; v[u] = u2[j < n2 ? j : 0]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int j = i + 256 * u;
          cntp += (j < n2 && v[u].x != a.P) + (j < n2 && v[u].y != a.P);
        }
      }
      if ((n & 1) && tid == 0) cntp += (a.ui[n - 1] != a.P);
    } else {
      for (int i = tid; i < n; i += 256) cntp += (a.ui[i] != a.P);
    }
  }
  const bool mine = tid < a.L && a.ui[(size_t)b * a.L + tid] != a.P;       // L <= 64 (validated): wave 0 holds the row
  const unsigned long long vm = __ballot(mine);
  cntp = (int)wave_sum((float)cntp);                        // < 2^24: exact in fp32
  if ((tid & 63) == 0) vred[tid >> 6] = cntp;
  __syncthreads();
  const int off = vred[0] + vred[1] + vred[2] + vred[3] + b;   // + one query row per earlier sequence
  if (!live) return;
  if (tid == 0) a.vrows[off] = b * a.S;
  if (mine) a.vrows[off + 1 + __popcll(vm & ((1ull << tid) - 1ull))] = b * a.S + 1 + tid;
  if (tid == 0 && b == a.B - 1) *a.vcount = off + 1 + __popcll(vm);
}
