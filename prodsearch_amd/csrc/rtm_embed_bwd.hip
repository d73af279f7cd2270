// rtm_embed_bwd.hip — backward of the review transformer's input assembly (rtm_embed.hip): d x into the segment rows, the user /
// item / review rows, d query_emb and the per-word slot rows the word reduce sums (rtm_index.hip); the fs review projection's
// d pre; deterministic mode's fixed-order sums and scatter keys for them.  Host stages at the end (rtm.h).
#include "rtm.h"

// ---- deterministic mode (ps_deterministic): fixed-order sums in place of the kernels' fp32 atomics
// d query_emb[b] = the query-position gradients of b's J sequences, in sequence order
__global__ __launch_bounds__(256) void rtm_dqe_det_kernel(const RtmK a) {
  const int b = blockIdx.x;
  for (int e = threadIdx.x; e < a.d; e += 256) {
    float acc = 0.f;
    for (int j = 0; j < a.J; ++j) acc += a.dx[(size_t)(b * a.J + j) * a.S * a.d + e];
    a.dqe[(size_t)b * a.d + e] = acc;
  }
}
// column sums of x [rows, d] in two fixed-order levels (the fs projection's bias gradient)
__global__ __launch_bounds__(256) void rtm_colsum_det_kernel(const float* x, int rows, int d, float* part) {
  const int per = (rows + (int)gridDim.x - 1) / (int)gridDim.x;
  const int r0 = blockIdx.x * per, r1 = min(rows, r0 + per);
  for (int e = threadIdx.x; e < d; e += 256) {
    float acc = 0.f;
    for (int r = r0; r < r1; ++r) acc += x[(size_t)r * d + e];
    part[(size_t)blockIdx.x * d + e] = acc;
  }
}
__global__ __launch_bounds__(256) void rtm_colsum_det_fold_kernel(const float* part, int nblk, int d, float* dst) {
  for (int e = threadIdx.x; e < d; e += 256) {
    float acc = 0.f;
    for (int b = 0; b < nblk; ++b) acc += part[(size_t)b * d + e];
    dst[e] += acc;
  }
}

// deterministic mode: the user / item row of every sequence position as a scatter key (-1: no gradient — a padded review
// position, the embedding's padding row, an id out of range), position-major like d x
__global__ __launch_bounds__(256) void rtm_ui_keys_kernel(const RtmK a, int32_t* ukeys, int32_t* ikeys, int32_t* rkeys, int npos) {
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= npos) return;
  const int n = t / a.S, s = t - n * a.S;
  const int b = fdiv(n, a.fJ), j = n - b * a.J;
  const bool pos = j == 0;
  const size_t base = pos ? (size_t)b : (size_t)b * a.K + (j - 1);
  bool ok = true;
  int64_t rid = -1;
  if (s > 0) { rid = (pos ? a.pos_r : a.neg_r)[base * a.R + s - 1]; ok = rid != a.RC - 1; }
  if (rkeys) rkeys[t] = (s > 0 && rid >= 0 && rid < a.RC - 1) ? (int32_t)rid : -1;      // pv encoder: the review's table row
  const size_t spos = base * a.S + s;
  if (ukeys) {
    const int64_t uid = ok ? (pos ? a.pos_u : a.neg_u)[spos] : -1;
    ukeys[t] = (uid >= 0 && uid < a.U) ? (int32_t)uid : -1;
  }
  if (ikeys) {
    const int64_t iid = ok ? (pos ? a.pos_i : a.neg_i)[spos] : -1;
    ikeys[t] = (iid >= 0 && iid < a.PI) ? (int32_t)iid : -1;
  }
}

// Backward of rtm_embed.  Like rtm_embed4_kernel it works on groups of the four review rows 4g .. 4g+3 of one side, which
// share one Philox counter row: a lane evaluates the dropout words of its columns once for the four reviews, and the
// (unconditional, all-real-address) loads of the four rows are in flight together — the wave's dependent chain is one round
// trip per group, EB_GROUPS groups per wave.  (Round 1: one wave per slot in a 38-slot grid-stride walk, one Philox
// evaluation per element: 69 us.)  Lane l owns columns l, l + 64, ...  The query slots (s = 0) ride as extra waves.
// The segment-embedding gradient (3 rows fed by EVERY slot) is summed in registers, combined over the workgroup's waves
// in LDS and PARKED as one [3][d] partial per workgroup (`seg_part`, folded by the step's last launch, ColFoldList)
// instead of 3d same-address atomics per workgroup.
// PL (the pvc encoder without the PV loss, the feature-selection layer and the user / item embeddings — configs[3]): those
// switches are compile-time off, which takes their pointers and flags out of the scalar registers (the general form reloads 34
// spilled scalars per group from VGPR lanes)
// PL = 2, the frozen form: no review-side table takes a gradient (frozen words under pvc / fs / avg, a frozen
// review table under pv).  A review-slot wave then only feeds d x into the segment partials and the trainable user / item rows:
// no Philox word, no cnt / dvec / d raw load, no store to gs, no add to g_table — all compile-time off, as with PL = 1.  When
// neither the segment rows nor user / item rows take a gradient the launcher passes npos_w = nneg_w = 0 and the grid is the
// query-position waves alone.
template <int NK, int PL>      // columns per lane: d <= 64 * NK
__global__ __launch_bounds__(256) void rtm_embed_bwd_kernel(const RtmK a, float* seg_part, int npos_w, int nneg_w, FDiv fR, FDiv fK) {
  __shared__ float segs[4][3][64 * NK];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wave = (int)blockIdx.x * 4 + wv;
  const int d = a.d;
  constexpr bool FZ = PL == 2;
  const bool pvc = PL == 1 ? true : (bool)a.pvc, has_ui = PL != 1 && !a.det && (a.g_user_emb || a.g_item_emb);   // det: rtm_ui_keys_kernel + launch_rows_scatter_det
  const float* const dmean = PL ? nullptr : a.dmean;
  const int64_t rpad = a.RC - 1;
  DropSpec dpos = a.d_pos, dneg = a.d_neg, dpv = a.d_pv;      // the step word is read once, not per element
  dpos.step = drop_step(a.d_pos); dpos.step_ptr = nullptr;
  dneg.step = drop_step(a.d_neg); dneg.step_ptr = nullptr;
  dpv.step = drop_step(a.d_pv); dpv.step_ptr = nullptr;
  float sacc[3][NK];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int k = 0; k < NK; ++k) sacc[q][k] = 0.f;
  int colc[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) colc[k] = lane + 64 * k < d ? lane + 64 * k : d - 1;
  if (wave < npos_w + nneg_w) {
    const bool pos = wave < npos_w;
    const int w0 = pos ? wave : wave - npos_w;
    const int nrev = pos ? a.B * a.R : a.B * a.K * a.R;
    const DropSpec ds = drop_select(pos, dpos, dneg);
    const bool wantdv = !PL && pos && a.train_pv;
    // lane i < 4 * EB_GROUPS decodes review row  4 * EB_GROUPS * w0 + i  (one coalesced read of the review ids / segment ids:
    // group after group through scalar loads the decode alone took 20 us)
    int my_n = 0, my_s = 1, my_seg = 3; int64_t my_rid = rpad; bool my_ok = false;
    {
      const int rr = w0 * 4 * EB_GROUPS + lane;
      if (lane < 4 * EB_GROUPS && rr < nrev) {
        const int base = fdiv(rr, fR), r = rr - base * a.R;
        int b;
        if (pos) { b = base; my_n = b * a.J; }
        else { b = fdiv(base, fK); my_n = b * a.J + 1 + (base - b * a.K); }
        my_s = r + 1;
        my_rid = (pos ? a.pos_r : a.neg_r)[rr];
        my_ok = my_rid != rpad;
        my_seg = (int)(pos ? a.pos_seg : a.neg_seg)[(size_t)base * a.S + r + 1];
      }
    }
    const unsigned long long okm = __ballot(my_ok);
    for (int gi = 0; gi < EB_GROUPS; ++gi) {
      const int gg = w0 * EB_GROUPS + gi;                   // review rows 4gg .. 4gg+3 of this side: one Philox counter row
      if (!((okm >> (4 * gi)) & 0xfull)) continue;
      int nq[4], sq[4], segq[4], rrq[4]; bool okq[4]; int64_t ridq[4]; size_t sposq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int src_lane = 4 * gi + q;
        okq[q] = (okm >> src_lane) & 1ull;
        const int sl = okq[q] ? src_lane : 4 * gi + (__ffsll((long long)((okm >> (4 * gi)) & 0xfull)) - 1);   // a dead row repeats a live one
        rrq[q] = w0 * 4 * EB_GROUPS + sl;
        // (the source lane is the same for the whole wave: v_readlane into scalar registers, not an LDS permute)
        nq[q] = __builtin_amdgcn_readlane(my_n, sl); sq[q] = __builtin_amdgcn_readlane(my_s, sl);
        segq[q] = __builtin_amdgcn_readlane(my_seg, sl);
        ridq[q] = (int64_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)((unsigned long long)my_rid >> 32), sl) << 32) |
                            (unsigned)__builtin_amdgcn_readlane((int)(unsigned long long)my_rid, sl));
        const int base = pos ? fdiv(nq[q], a.fJ) : (fdiv(nq[q], a.fJ) * a.K + (nq[q] - fdiv(nq[q], a.fJ) * a.J - 1));
        sposq[q] = (size_t)base * a.S + sq[q];
      }
      uint32_t dw[NK][4];
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        Philox4 t = {0u, 0u, 0u, 0u};
        if (!FZ && ds.thr) t = philox4x32_10((uint32_t)(lane + 64 * k), (uint32_t)gg, ds.site, ds.step, ds.k0, ds.k1);
        dw[k][0] = t.x; dw[k][1] = t.y; dw[k][2] = t.z; dw[k][3] = t.w;
      }
      // every address is a real one (a dead row repeats the group's first, columns past d clamp), so the loads of the four
      // rows are unconditional and in flight together
      float gk[4][NK], src[4][NK], dvv[4][NK], cntv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float* g = a.dx + ((size_t)nq[q] * a.S + sq[q]) * d;
        // fs: the review vector reached x through tanh(f_W . raw + b); its input gradient d raw was left in a.dmean
        if (FZ) {                                          // (compile-time) d x is all a frozen slot needs
#pragma unroll
          for (int k = 0; k < NK; ++k) { gk[q][k] = g[colc[k]]; src[q][k] = 0.f; dvv[q][k] = 0.f; }
          cntv[q] = 1.f;
          continue;
        }
        const float* gm = dmean ? dmean + ((pos ? (size_t)0 : (size_t)a.B * a.R) + rrq[q]) * d : g;
        const float* dvp = wantdv ? a.dvec + (size_t)rrq[q] * d : g;
#pragma unroll
        for (int k = 0; k < NK; ++k) { gk[q][k] = g[colc[k]]; src[q][k] = gm[colc[k]]; dvv[q][k] = dvp[colc[k]]; }
        cntv[q] = pvc ? a.cnt[(size_t)nq[q] * a.R + sq[q] - 1] : 1.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!okq[q]) continue;                             // wave-uniform
        if (has_ui) {                // user / item embedding rows of this position
          const int64_t uid = a.g_user_emb ? (pos ? a.pos_u : a.neg_u)[sposq[q]] : -1;
          const int64_t iid = a.g_item_emb ? (pos ? a.pos_i : a.neg_i)[sposq[q]] : -1;
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            const int col = lane + 64 * k;
            if (col < d) {
              if (uid >= 0 && uid < a.U) atomicAdd(&a.g_user_emb[(size_t)uid * d + col], gk[q][k]);
              if (iid >= 0 && iid < a.PI) atomicAdd(&a.g_item_emb[(size_t)iid * d + col], gk[q][k]);
            }
          }
        }
        if (a.use_seg && segq[q] < 3) {                    // row 3 is the padding_idx of seg_embeddings: no gradient
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            const float v = lane + 64 * k < d ? gk[q][k] : 0.f;
            if (segq[q] == 0) sacc[0][k] += v;
            else if (segq[q] == 1) sacc[1][k] += v;
            else sacc[2][k] += v;
          }
        }
        if (FZ) continue;                                  // (compile-time) nothing behind the review vector takes a gradient
        // through dropout_layer (and, pv positive with train_pv, the PV drop_layer + the PV-loss gradient)
        float t[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          float v = src[q][k] * (ds.thr ? drop_word(ds, dw[k][q]) : 1.f);
          if (wantdv) {
            v += dvv[q][k];
            if (!pvc) v *= drop_mult(dpv, (uint32_t)rrq[q], (uint32_t)(lane + 64 * k));
          }
          t[k] = v;
        }
        if (!pvc && !a.det) {
          float* grow = a.g_table + (size_t)rclamp(ridq[q], rpad) * d;
#pragma unroll
          for (int k = 0; k < NK; ++k)
            if (lane + 64 * k < d) atomicAdd(&grow[lane + 64 * k], t[k]);
        } else if (!pvc) {
          // deterministic mode: the review row's gradient parked in place of d x (like the pvc rows below); rtm_ui_keys_kernel's
          // review keys + launch_rows_scatter_det add the rows up, one owner per table row, in position order
          float* gw = a.gs + ((size_t)nq[q] * a.S + sq[q]) * d;
#pragma unroll
          for (int k = 0; k < NK; ++k)
            if (lane + 64 * k < d) gw[lane + 64 * k] = t[k];
        } else {
          // mean backward: every non-pad word row of the review gets g / cnt (token corruption bypasses autograd, PVC.py:53)
          // 1.2 M word occurrences x 512 B of fp32 atomics per step ran at 0.7 TB/s; instead the row is rewritten in
          // place as the per-word gradient (rtm_wreduce_kernel sums the rows of a word's occurrences through the index)
          const float inv = 1.f / cntv[q];
          float* gw = a.gs + ((size_t)nq[q] * a.S + sq[q]) * d;
#pragma unroll
          for (int k = 0; k < NK; ++k)
            if (lane + 64 * k < d) gw[lane + 64 * k] = t[k] * inv;
        }
      }
    }
  } else {
    // ---- query positions (s = 0) of EB_QSEQ sequences: segment / user / item rows and d query_emb
    const int n0 = (wave - npos_w - nneg_w) * EB_QSEQ, nseq = a.B * a.J;
    for (int i0 = 0; i0 < EB_QSEQ && n0 + i0 < nseq; i0 += 4) {
      float gk[4][NK]; int bq[4], segq[4]; bool on[4], posq[4]; size_t sposq[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n = n0 + i0 + q;
        on[q] = n < nseq;
        const int nc = on[q] ? n : n0;
        const int b = fdiv(nc, a.fJ), j = nc - b * a.J;
        bq[q] = b; posq[q] = j == 0;
        sposq[q] = (posq[q] ? (size_t)b : (size_t)b * a.K + (j - 1)) * a.S;
        segq[q] = (int)(posq[q] ? a.pos_seg : a.neg_seg)[sposq[q]];
        const float* g = a.dx + (size_t)nc * a.S * d;
#pragma unroll
        for (int k = 0; k < NK; ++k) gk[q][k] = g[colc[k]];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!on[q]) continue;
        if (has_ui) {
          const int64_t uid = a.g_user_emb ? (posq[q] ? a.pos_u : a.neg_u)[sposq[q]] : -1;
          const int64_t iid = a.g_item_emb ? (posq[q] ? a.pos_i : a.neg_i)[sposq[q]] : -1;
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            const int col = lane + 64 * k;
            if (col < d) {
              if (uid >= 0 && uid < a.U) atomicAdd(&a.g_user_emb[(size_t)uid * d + col], gk[q][k]);
              if (iid >= 0 && iid < a.PI) atomicAdd(&a.g_item_emb[(size_t)iid * d + col], gk[q][k]);
            }
          }
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const int col = lane + 64 * k;
          if (col >= d) continue;
          if (a.use_seg && segq[q] < 3) {
            if (segq[q] == 0) sacc[0][k] += gk[q][k];
            else if (segq[q] == 1) sacc[1][k] += gk[q][k];
            else sacc[2][k] += gk[q][k];
          }
          if (!a.det) atomicAdd(&a.dqe[(size_t)bq[q] * d + col], gk[q][k]);      // det: rtm_dqe_det_kernel
        }
      }
    }
  }
  if (!a.use_seg) return;
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (lane + 64 * k < d) segs[wv][q][lane + 64 * k] = sacc[q][k];
  __syncthreads();
  for (int e = threadIdx.x; e < 3 * d; e += 256) {
    const int q = e / d, col = e - q * d;
    seg_part[(size_t)blockIdx.x * 3 * d + e] = (segs[0][q][col] + segs[1][q][col]) + (segs[2][q][col] + segs[3][q][col]);
  }
}

// backward head: d pre[row] = valid ? dx[n][s] * (1 - y^2) : 0 for every review slot; bias gradient = its column sums
__global__ __launch_bounds__(256) void rtm_fs_bwd_kernel(const RtmK a, float* dpre, float* g_bias) {
  extern __shared__ float bsum[];                  // [d]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int d = a.d;
  for (int e = threadIdx.x; e < d; e += 256) bsum[e] = 0.f;
  __syncthreads();
  const int nslots = a.B * a.J * a.S, nw = gridDim.x * 4;
  for (int slot = blockIdx.x * 4 + wv; slot < nslots; slot += nw) {
    const int n = fdiv(slot, a.fS), s = slot - n * a.S;
    if (s == 0) continue;
    int b, j, revrow, seg; int64_t ridx;
    seq_decode(a, n, s, b, j, ridx, revrow, seg);
    const bool ok = ridx != a.RC - 1;
    const size_t rg = j == 0 ? (size_t)revrow : (size_t)a.B * a.R + revrow;
    for (int col = lane; col < d; col += 64) {
      float v = 0.f;
      if (ok) {
        const float y = a.yfs[rg * d + col];
        v = a.dx[((size_t)n * a.S + s) * d + col] * (1.f - y * y);
        if (!a.det) atomicAdd(&bsum[col], v);
      }
      dpre[rg * d + col] = v;
    }
  }
  __syncthreads();
  if (a.det) return;                               // rtm_colsum_det_kernel over dpre
  for (int e = threadIdx.x; e < d; e += 256) atomicAdd(&g_bias[e], bsum[e]);
}

// ------------------------------------------------------------------ host side
// workgroups of the slot-walking kernels (measured, ms/step: 128 0.850, 256 0.764, 384 0.762, 512 0.734, 1024 0.749,
// 2048 0.784, 4096 0.837)
int rtm_slot_blocks(const RtmWs& r) {
  static const int eb_cap = ps_diag_int("PS_RTM_EB", 512);
  int eb = ps_cdiv(r.Bseq * r.S, 4);
  return eb > eb_cap ? eb_cap : eb;
}

int rtm_fs_bwd(const RtmK& k, const RtmWs& r, float* dpre, float* g_bias, hipStream_t st) {
  const int d = k.d;
  hipLaunchKernelGGL(rtm_fs_bwd_kernel, dim3(rtm_slot_blocks(r)), dim3(256), (size_t)d * sizeof(float), st, k, dpre, g_bias);
  PS_LAUNCH_CHECK();
  if (k.det) {
    float* part;
    TRY(rtm_det_scratch((size_t)256 * d, st, &part));
    hipLaunchKernelGGL(rtm_colsum_det_kernel, dim3(256), dim3(256), 0, st, dpre, r.Bseq * k.R, d, part);
    PS_LAUNCH_CHECK();
    hipLaunchKernelGGL(rtm_colsum_det_fold_kernel, dim3(1), dim3(256), 0, st, part, 256, d, g_bias);
    PS_LAUNCH_CHECK();
  }
  return PS_OK;
}

template <int NK>
static void eb_launch(int form, int nwg, hipStream_t st, const RtmK& k, float* sp, int npw, int nnw, FDiv fR, FDiv fK) {
  if (form == PS_RTM_EB_PLAIN) hipLaunchKernelGGL((rtm_embed_bwd_kernel<NK, 1>), dim3(nwg), dim3(256), 0, st, k, sp, npw, nnw, fR, fK);
  else if (form == PS_RTM_EB_FROZEN) hipLaunchKernelGGL((rtm_embed_bwd_kernel<NK, 2>), dim3(nwg), dim3(256), 0, st, k, sp, npw, nnw, fR, fK);
  else hipLaunchKernelGGL((rtm_embed_bwd_kernel<NK, 0>), dim3(nwg), dim3(256), 0, st, k, sp, npw, nnw, fR, fK);
}

int rtm_embed_bwd(const PsRtmDesc& D, const RtmK& k, const RtmWs& r, const PsRtmBwdPlan& pl, float* ws, ColFoldList& fold, hipStream_t st) {
  const int B = D.B, d = D.d, npos = r.Bseq * r.S;
  int npw, nnw;
  int nwg = ps_cdiv(rtm_eb_waves(B, D.K, D.R, &npw, &nnw), 4);
  if (!pl.slot_waves) {                            // frozen form with nothing to feed: the query-position waves alone
    npw = nnw = 0;
    nwg = ps_cdiv(ps_cdiv((int64_t)B * (D.K + 1), EB_QSEQ), 4);
  }
  const FDiv fR = make_fdiv(D.R), fK = make_fdiv(D.K > 0 ? D.K : 1);
  float* sp = ws + r.segpart;
  if (k.det && (k.g_user_emb || k.g_item_emb)) {
    // user / item embedding rows, deterministic mode: a sole-owner scatter of d x by position — BEFORE the kernel below, which
    // rewrites the review positions' rows of d x in place (pvc: RtmK::gs)
    float* scr;
    TRY(rtm_det_scratch((size_t)2 * npos + 8, st, &scr));
    int32_t* keys = reinterpret_cast<int32_t*>(scr);
    int32_t* uk = k.g_user_emb ? keys : nullptr;
    int32_t* ik = k.g_item_emb ? keys + npos : nullptr;
    hipLaunchKernelGGL(rtm_ui_keys_kernel, dim3(ps_cdiv(npos, 256)), dim3(256), 0, st, k, uk, ik, (int32_t*)nullptr, npos);
    PS_LAUNCH_CHECK();
    if (uk) TRY(launch_rows_scatter_det(uk, npos, k.dx, d, d, k.g_user_emb, st));
    if (ik) TRY(launch_rows_scatter_det(ik, npos, k.dx, d, d, k.g_item_emb, st));
  }
  if (d <= 64) eb_launch<1>(pl.embed_form, nwg, st, k, sp, npw, nnw, fR, fK);
  else if (d <= 128) eb_launch<2>(pl.embed_form, nwg, st, k, sp, npw, nnw, fR, fK);
  else if (d <= 256) eb_launch<4>(pl.embed_form, nwg, st, k, sp, npw, nnw, fR, fK);
  else eb_launch<8>(pl.embed_form, nwg, st, k, sp, npw, nnw, fR, fK);
  PS_LAUNCH_CHECK();
  if (k.det && pl.review_scatter) {                // pv encoder: the parked review-row gradients -> review_emb, by review id
    float* scr;
    TRY(rtm_det_scratch((size_t)npos + 8, st, &scr));
    int32_t* rk = reinterpret_cast<int32_t*>(scr);
    hipLaunchKernelGGL(rtm_ui_keys_kernel, dim3(ps_cdiv(npos, 256)), dim3(256), 0, st, k, (int32_t*)nullptr, (int32_t*)nullptr, rk, npos);
    PS_LAUNCH_CHECK();
    TRY(launch_rows_scatter_det(rk, npos, k.gs, d, d, k.g_table, st));
  }
  if (k.det) {
    hipLaunchKernelGGL(rtm_dqe_det_kernel, dim3(B), dim3(256), 0, st, k);
    PS_LAUNCH_CHECK();
  }
  if (D.use_seg_emb) {
    PS_REQUIRE(fold.n < PS_MAX_COLFOLD, "rtm backward: too many parked column sums");
    ColFold& f = fold.e[fold.n++];
    f.partial = sp; f.nblk = nwg; f.d = d;
    f.dst[0] = k.g_seg_emb; f.dst[1] = k.g_seg_emb + d; f.dst[2] = k.g_seg_emb + 2 * (size_t)d;
  }
  return PS_OK;
}
