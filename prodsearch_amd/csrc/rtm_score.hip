// rtm_score.hip — the review transformer's head: scores (wo . enc + bias) with the folded ranking loss, the PV word-prediction
// logits, the loss kernel, and their backward (d enc, d wo, the PV loss's d vec and word rows).  Host stages at the end (rtm.h).
#include "rtm.h"

// ------------------------------------------------------------------ scores
// also writes the loss weight of the sequence (ps_model.py:344-345): pos_weight for the positive, and for a
// negative 1 iff it has at least one real review
// `fold_loss` (training without the PV loss): the workgroup adds its four loss terms to ONE 64-bit word with a returning
// agent-scope atomic — fixed point (2^-20 units: integer adds, so the total does not depend on the arrival order) in the
// low 48 bits, the arrival count above them — and the workgroup that sees the count complete holds the total in the
// value it got back: rtm_loss_kernel's result without its launch and without a device-scope fence (which on this part
// writes back the XCD's L2: the first form, partials + __threadfence + ticket, doubled this kernel's 6 us).
__global__ __launch_bounds__(256) void rtm_score_kernel(const RtmK a, float* out, int fold_loss, unsigned long long* ticket) {
  __shared__ float wterm[4];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int n = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  float term = 0.f;
  if (n < a.B * a.J) {
    float s = 0.f;
    for (int e = lane; e < a.d; e += 64) s += a.enc[(size_t)n * a.d + e] * a.wo_w[e];
    s = wave_sum(s) + a.wo_b[0];
    if (lane == 0) out[n] = s;
    if (!a.eval) {
      const int b = fdiv(n, a.fJ), j = n - b * a.J;
      float wgt;
      if (j == 0) wgt = a.pos_weight ? (float)a.K : 1.f;
      else {
        bool any = false;
        for (int r = lane; r < a.R; r += 64) any = any || (a.neg_r[((size_t)b * a.K + j - 1) * a.R + r] != a.RC - 1);
        wgt = __ballot(any) != 0ull ? 1.f : 0.f;
      }
      if (lane == 0) a.weight[n] = wgt;
      term = wgt * softplus_f(j == 0 ? -s : s);
    }
  }
  if (!fold_loss) return;
  if (lane == 0) wterm[wv] = term;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float mine_f = (wterm[0] + wterm[1]) + (wterm[2] + wterm[3]);           // >= 0: weights and softplus are
    // (a partial that is NaN / Inf / beyond the 48-bit field's share — 2^27 / grid per workgroup — is handed over as 0 and
    // poisons the loss through the spare word of the cleared group, set by a returning atomic the arrival add depends on:
    // garbage must not carry into the arrival count)
    uint32_t* spare = reinterpret_cast<uint32_t*>(ticket) + 3;
    long long fx = 0;
    if (mine_f >= 0.f && mine_f * (float)gridDim.x < 134217728.f) fx = (long long)llrintf(mine_f * 1048576.f);
    else fx = (long long)(__hip_atomic_fetch_or(spare, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0u);
    const unsigned long long mine = (unsigned long long)fx + (1ull << 48);
    const unsigned long long old = __hip_atomic_fetch_add(ticket, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((old >> 48) == (unsigned long long)gridDim.x - 1ull) {
      const unsigned long long tot = (old + mine) & ((1ull << 48) - 1ull);
      const bool poison = __hip_atomic_load(spare, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
      const float psl = poison ? __builtin_inff() : (float)((double)tot * (1.0 / 1048576.0)) / (float)a.B;
      a.loss3[0] = psl; a.loss3[1] = psl; a.loss3[2] = 0.f;
      a.nvalid[0] = 0.f;
    }
  }
}

// PV logits: task t = ((b*R + r)*W + w)*(1+K) + j
#define PV_U 4
__global__ __launch_bounds__(256) void rtm_pv_fwd_kernel(const RtmK a, int ntask, int lpr) {
  const int tid = threadIdx.x, c = tid % lpr;
  const int grp = blockIdx.x * (256 / lpr) + tid / lpr;
  const int K1 = a.K + 1, nch = a.d >> 2;
  const float* rows[PV_U]; const float* vecs[PV_U]; int tt[PV_U]; float sgn[PV_U];
#pragma unroll
  for (int u = 0; u < PV_U; ++u) {
    const int t = grp * PV_U + u;
    tt[u] = t; rows[u] = nullptr; vecs[u] = nullptr; sgn[u] = 1.f;
    if (t < ntask) {
      const int tw = fdiv(t, a.fK1), j = t - tw * K1;
      const int rev = tw / a.W, w = tw - rev * a.W;
      int64_t idx = j == 0 ? a.pos_words[(size_t)rev * a.W + w] : a.neg_word_idxs[(size_t)rev * a.W * a.K + (size_t)w * a.K + j - 1];
      idx = rclamp(idx, a.V - 1);
      rows[u] = a.word_emb + (size_t)idx * a.d;
      vecs[u] = a.vec + (size_t)rev * a.d;
      sgn[u] = j == 0 ? -1.f : 1.f;
    }
  }
  float4 r[PV_U], v[PV_U];
#pragma unroll
  for (int u = 0; u < PV_U; ++u) {
    r[u] = make_float4(0.f, 0.f, 0.f, 0.f); v[u] = r[u];
    if (rows[u] && c < nch) {
      r[u] = *reinterpret_cast<const float4*>(rows[u] + 4 * c);
      v[u] = *reinterpret_cast<const float4*>(vecs[u] + 4 * c);
    }
  }
#pragma unroll
  for (int u = 0; u < PV_U; ++u) {
    float s = r[u].x * v[u].x + r[u].y * v[u].y + r[u].z * v[u].z + r[u].w * v[u].w;
    if (rows[u])
      for (int cc = c + lpr; cc < nch; cc += lpr) {
        float4 rr = *reinterpret_cast<const float4*>(rows[u] + 4 * cc);
        float4 vv = *reinterpret_cast<const float4*>(vecs[u] + 4 * cc);
        s += rr.x * vv.x + rr.y * vv.y + rr.z * vv.z + rr.w * vv.w;
      }
    s = group_sum(s, lpr);
    if (c == 0 && rows[u]) {
      a.pv_scores[tt[u]] = s;
      a.pv_terms[tt[u]] = softplus_f(sgn[u] < 0.f ? -s : s);
    }
  }
}

// Loss: ps = mean_b sum_j weight * bce ; pv = sum_rev masked-mean_w(sum_j bce) / #non-pad positive reviews
__global__ __launch_bounds__(256) void rtm_loss_kernel(const RtmK a) {
  __shared__ float s1[256], s2[256], s3[256];
  const int tid = threadIdx.x, K1 = a.K + 1;
  float ps = 0.f, pv = 0.f, nv = 0.f;
  for (int b = tid; b < a.B; b += 256) {
    const float* sc = a.scores + (size_t)b * K1;
    const float* wg = a.weight + (size_t)b * K1;
    ps += wg[0] * softplus_f(-sc[0]);
    for (int k = 0; k < a.K; ++k) ps += wg[1 + k] * softplus_f(sc[1 + k]);
  }
  if (a.train_pv) {
    for (int rev = tid; rev < a.B * a.R; rev += 256) {
      nv += (a.pos_r[rev] != a.RC - 1) ? 1.f : 0.f;
      float sum = 0.f; int cnt = 0;
      for (int w = 0; w < a.W; ++w) {
        if (a.pos_masks[(size_t)rev * a.W + w]) {
          ++cnt;
          const float* t = a.pv_terms + ((size_t)rev * a.W + w) * K1;
          for (int j = 0; j < K1; ++j) sum += t[j];
        }
      }
      pv += sum / (float)(cnt > 0 ? cnt : 1);
    }
  }
  s1[tid] = ps; s2[tid] = pv; s3[tid] = nv;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { s1[tid] += s1[tid + o]; s2[tid] += s2[tid + o]; s3[tid] += s3[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    const float psl = s1[0] / (float)a.B;
    const float pvl = a.train_pv ? s2[0] / s3[0] : 0.f;
    a.loss3[0] = psl + pvl; a.loss3[1] = psl; a.loss3[2] = pvl;
    a.nvalid[0] = s3[0];
  }
}

// ------------------------------------------------------------------ backward kernels
__global__ __launch_bounds__(256) void rtm_score_bwd_kernel(const RtmK a, int zero_dqe, uint32_t* sig, uint32_t sigval) {
  fork_signal(sig, sigval);
  extern __shared__ float acc[];                  // [d] partial of d wo_w, + 1 for d wo_b
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), K1 = a.K + 1;
  if (zero_dqe)                                   // d query_emb collects atomics much later (rtm_embed_bwd_kernel): no memset launch
    for (int e = blockIdx.x * 256 + threadIdx.x; e < a.B * a.d; e += gridDim.x * 256) a.dqe[e] = 0.f;
  for (int e = threadIdx.x; e <= a.d; e += 256) acc[e] = 0.f;
  __syncthreads();
  const float sc = a.scale * (a.scale_dev ? *a.scale_dev : 1.f) / (float)a.B;
  const int nw = gridDim.x * 4;
  for (int n = blockIdx.x * 4 + wv; n < a.B * K1; n += nw) {
    const int b = fdiv(n, a.fK1), j = n - b * K1;
    const float wgt = a.weight[n];
    const float s = a.scores[n];
    const float ds = wgt * (sigmoid_f(s) - (j == 0 ? 1.f : 0.f)) * sc;
    for (int e = lane; e < a.d; e += 64) {
      a.denc[(size_t)n * a.d + e] = ds * a.wo_w[e];
      if (!a.det) atomicAdd(&acc[e], ds * a.enc[(size_t)n * a.d + e]);
    }
    if (lane == 0 && !a.det) atomicAdd(&acc[a.d], ds);
  }
  if (a.det) return;                              // rtm_score_wo_det_kernel adds them up in sequence order
  __syncthreads();
  for (int e = threadIdx.x; e < a.d; e += 256) atomicAdd(&a.g_wo_w[e], acc[e]);
  if (threadIdx.x == 0) atomicAdd(&a.g_wo_b[0], acc[a.d]);
}
// ---- deterministic mode (ps_deterministic): the reductions of the backward whose fp32 additions could meet in a
// different order from run to run, each as a fixed-order sum.  (The word index gets its ranks from rtm_hist_kernel<0, 64, 1>.)
// d wo_w / d wo_b: one workgroup, a thread owns its columns and walks the sequences in order
__global__ __launch_bounds__(256) void rtm_score_wo_det_kernel(const RtmK a) {
  const int K1 = a.K + 1, tid = threadIdx.x;
  const float sc = a.scale * (a.scale_dev ? *a.scale_dev : 1.f) / (float)a.B;
  float acc0 = 0.f, acc1 = 0.f, accb = 0.f;
  const int e0 = tid < a.d ? tid : a.d - 1, e1 = tid + 256 < a.d ? tid + 256 : a.d - 1;
  for (int n0 = 0; n0 < a.B * K1; n0 += 8) {
    float ds[8], x0[8], x1[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int n = n0 + u < a.B * K1 ? n0 + u : n0;
      const int b = fdiv(n, a.fK1), j = n - b * K1;
      ds[u] = a.weight[n] * (sigmoid_f(a.scores[n]) - (j == 0 ? 1.f : 0.f)) * sc;
      x0[u] = a.enc[(size_t)n * a.d + e0];
      x1[u] = a.enc[(size_t)n * a.d + e1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (n0 + u < a.B * K1) { acc0 += ds[u] * x0[u]; acc1 += ds[u] * x1[u]; accb += ds[u]; }
  }
  if (tid < a.d) a.g_wo_w[tid] += acc0;
  if (tid + 256 < a.d) a.g_wo_w[tid + 256] += acc1;
  if (tid == 0) a.g_wo_b[0] += accb;
}

// deterministic mode: the PV loss's word-row tasks (review, window slot, 1 + K words) as scatter keys with their scalar — the
// task's row is  ds * vec[review]  (the same arithmetic as rtm_pv_bwd_kernel below)
__global__ __launch_bounds__(256) void rtm_pv_keys_kernel(const RtmK a, int32_t* keys, float* scale, int32_t* rowidx, int ntask) {
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= ntask) return;
  const int K1 = a.K + 1, per = a.W * K1;
  const int rev = t / per, rem = t - rev * per, w = rem / K1, j = rem - w * K1;
  int cnt = 0;
  for (int w2 = 0; w2 < a.W; ++w2) cnt += a.pos_masks[(size_t)rev * a.W + w2] ? 1 : 0;
  const float sc = a.scale * (a.scale_dev ? *a.scale_dev : 1.f) / ((float)(cnt > 0 ? cnt : 1) * a.nvalid[0]);
  int32_t key = -1; float ds = 0.f;
  if (a.pos_masks[(size_t)rev * a.W + w]) {
    int64_t idx = j == 0 ? a.pos_words[(size_t)rev * a.W + w] : a.neg_word_idxs[(size_t)rev * a.W * a.K + (size_t)w * a.K + j - 1];
    idx = rclamp(idx, a.V - 1);
    const float s = a.pv_scores[((size_t)rev * a.W + w) * K1 + j];
    ds = (sigmoid_f(s) - (j == 0 ? 1.f : 0.f)) * sc;
    key = idx != a.V - 1 ? (int32_t)idx : -1;
  }
  keys[t] = key; scale[t] = ds; rowidx[t] = rev;
}

// PV backward: one wave per positive review; d vec (dense) and word-row scatter-adds
// WR = false: the word table is frozen — no word-row atomics (and in deterministic mode, where rtm_pv_keys_kernel scatters the
// rows, this kernel only ever builds d vec).  DV = false: the review side takes no gradient (pv: a frozen review table; pvc's
// d vec only ever reaches the word rows) — no word row is loaded and d vec is not stored.  <false, false> is never launched.
template <bool WR, bool DV>
__global__ __launch_bounds__(256) void rtm_pv_bwd_kernel(const RtmK a) {
  const int lane = threadIdx.x & 63, half = lane >> 5, c = lane & 31;
  const int rev = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (rev >= a.B * a.R) return;
  const int d = a.d, epl = d >> 5, K1 = a.K + 1;
  int cnt = 0;
  for (int w = 0; w < a.W; ++w) cnt += a.pos_masks[(size_t)rev * a.W + w] ? 1 : 0;
  const float sc = a.scale * (a.scale_dev ? *a.scale_dev : 1.f) / ((float)(cnt > 0 ? cnt : 1) * a.nvalid[0]);
  float dv[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) dv[k] = 0.f;
  const float* vec = a.vec + (size_t)rev * d;
  for (int t = half; t < a.W * K1; t += 2) {
    const int w = t / K1, j = t - w * K1;
    if (!a.pos_masks[(size_t)rev * a.W + w]) continue;
    int64_t idx = j == 0 ? a.pos_words[(size_t)rev * a.W + w] : a.neg_word_idxs[(size_t)rev * a.W * a.K + (size_t)w * a.K + j - 1];
    idx = rclamp(idx, a.V - 1);
    const float s = a.pv_scores[((size_t)rev * a.W + w) * K1 + j];
    const float ds = (sigmoid_f(s) - (j == 0 ? 1.f : 0.f)) * sc;
    const float* wrow = a.word_emb + (size_t)idx * d;
    float* grow = WR ? a.g_word_emb + (size_t)idx * d : nullptr;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k < epl) {
        const int e = c + 32 * k;
        if (WR && idx != a.V - 1 && !a.det) atomicAdd(&grow[e], ds * vec[e]);      // det: rtm_pv_keys_kernel + launch_rows_scatter_det
        if (DV) dv[k] += ds * wrow[e];
      }
  }
  if (!DV) return;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < epl) {
      float v = dv[k] + __shfl_xor(dv[k], 32, 64);
      if (half == 0) a.dvec[(size_t)rev * d + c + 32 * k] = v;
    }
}

// ------------------------------------------------------------------ host side
int rtm_head_fwd(const RtmK& k, const RtmWs& r, float* ws, hipStream_t st) {
  const bool fold_loss = !k.train_pv;               // (the PV loss needs rtm_pv_fwd_kernel's terms: rtm_loss_kernel then)
  PS_REQUIRE(!fold_loss || ps_cdiv(r.Bseq, 4) < 65536, "rtm forward: too many sequences for the folded loss");
  hipLaunchKernelGGL(rtm_score_kernel, dim3(ps_cdiv(r.Bseq, 4)), dim3(256), 0, st, k, k.scores, fold_loss ? 1 : 0,
                     reinterpret_cast<unsigned long long*>(ws + r.loss_blk));
  PS_LAUNCH_CHECK();
  if (fold_loss) return PS_OK;
  if (k.train_pv) {
    const int ntask = k.B * k.R * k.W * (k.K + 1);
    int lpr = 1; while (lpr < k.d / 4 && lpr < 64) lpr <<= 1;
    hipLaunchKernelGGL(rtm_pv_fwd_kernel, dim3(ps_cdiv(ps_cdiv(ntask, PV_U), 256 / lpr)), dim3(256), 0, st, k, ntask, lpr);
    PS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rtm_loss_kernel, dim3(1), dim3(256), 0, st, k);
  PS_LAUNCH_CHECK();
  return PS_OK;
}

int rtm_score_eval(const RtmK& k, const RtmWs& r, float* scores, hipStream_t st) {
  hipLaunchKernelGGL(rtm_score_kernel, dim3(ps_cdiv(r.Bseq, 4)), dim3(256), 0, st, k, scores, 0, nullptr);
  PS_LAUNCH_CHECK();
  return PS_OK;
}

int rtm_head_bwd(const RtmK& k, const RtmWs& r, const PsRtmBwdPlan& pl, uint32_t* sig, uint32_t sigval, hipStream_t st) {
  const int B = k.B, d = k.d;
  int blocks = ps_cdiv(r.Bseq, 4); if (blocks > 256) blocks = 256;
  // (d query_emb is zeroed by this launch unless the late index's memset covers it)
  hipLaunchKernelGGL(rtm_score_bwd_kernel, dim3(blocks), dim3(256), (size_t)(d + 1) * sizeof(float), st, k, pl.index != PS_RTM_INDEX_LATE ? 1 : 0, sig, sigval);
  PS_LAUNCH_CHECK();
  if (k.det) {
    PS_REQUIRE(d <= 512, "rtm backward: deterministic mode supports d <= 512");
    hipLaunchKernelGGL(rtm_score_wo_det_kernel, dim3(1), dim3(256), 0, st, k);
    PS_LAUNCH_CHECK();
  }
  if (pl.pv_bwd_kernel) {
    const dim3 pg(ps_cdiv(B * k.R, 4));
    const bool wr = (pl.pv_bwd & PS_RTM_PV_WORDS) != 0, dv = (pl.pv_bwd & PS_RTM_PV_DVEC) != 0;
    if (wr && dv) hipLaunchKernelGGL((rtm_pv_bwd_kernel<true, true>), pg, dim3(256), 0, st, k);
    else if (dv) hipLaunchKernelGGL((rtm_pv_bwd_kernel<false, true>), pg, dim3(256), 0, st, k);
    else hipLaunchKernelGGL((rtm_pv_bwd_kernel<true, false>), pg, dim3(256), 0, st, k);
    PS_LAUNCH_CHECK();
  }
  if ((pl.pv_bwd & PS_RTM_PV_WORDS) && k.det) {      // the PV loss's word rows: sole-owner scatter of ds * vec[review]
    const int ntask = B * k.R * k.W * (k.K + 1);
    float* scr;
    TRY(rtm_det_scratch((size_t)3 * ntask + 8, st, &scr));
    int32_t* pk = reinterpret_cast<int32_t*>(scr);
    float* psc = scr + ntask;
    int32_t* pri = reinterpret_cast<int32_t*>(scr + 2 * (size_t)ntask);
    hipLaunchKernelGGL(rtm_pv_keys_kernel, dim3(ps_cdiv(ntask, 256)), dim3(256), 0, st, k, pk, psc, pri, ntask);
    PS_LAUNCH_CHECK();
    TRY(launch_rows_scatter_det(pk, ntask, k.vec, d, d, k.g_word_emb, st, psc, pri));
  }
  return PS_OK;
}
