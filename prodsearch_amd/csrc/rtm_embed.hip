// rtm_embed.hip — the review transformer's forward input assembly: review vectors (pv: row gather; pvc / fs / avg: masked mean
// of the review's word rows), dropout, segment / user / item rows, key mask, positional add -> x[B*J, S, d]; the valid-row and
// valid-group lists; the fs encoder's forward tail; the eval review table.  Host stages at the end (rtm.h).
#include "rtm.h"

// valid-row list of x: wave n places its sequence's valid rows behind those of all earlier sequences (their counts come
// from rtm_embed_kernel: Bseq ints, L2 hits) — one short launch that lets the three K/V GEMMs skip the padded
// positions (73 % of the rows on the synthetic C4 batches)
__global__ __launch_bounds__(256) void rtm_rowlist_kernel(const RtmK a) {
  const int lane = threadIdx.x & 63;
  const int n = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nseq = a.B * a.J;
  if (n >= nseq) return;
  int prev = strided_sum_i32<8>(a.seqcnt, n, lane, 64);      // (up to 24 elements per lane: as a plain loop, 24 serial round trips)
  prev = (int)wave_sum((float)prev);                         // < 2^24: exact in fp32
  const bool okl = lane < a.S && a.valid[(size_t)n * a.S + lane] != 0.f;
  const unsigned long long vm = __ballot(okl);
  if (okl) a.vrows[prev + __popcll(vm & ((1ull << lane) - 1ull))] = n * a.S + lane;
  if (n == nseq - 1 && lane == 0) *a.vcount = prev + __popcll(vm);
}

// ------------------------------------------------------------------ embed forward
// one wave per (sequence, position); lanes: half = lane>>5 picks every other word row, c = lane&31 the float4
// chunk of the row (d <= 128: one chunk per lane; wider rows loop).
__global__ __launch_bounds__(256) void rtm_embed_kernel(const RtmK a) {
  const int lane = threadIdx.x & 63, half = lane >> 5, c = lane & 31;
  const int slot = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (slot >= a.B * a.J * a.S) return;
  const int n = fdiv(slot, a.fS), s = slot - n * a.S;
  const int d = a.d, nch = d >> 2;
  int b, j, revrow, seg; int64_t ridx; size_t spos;
  seq_decode(a, n, s, b, j, ridx, revrow, seg, &spos);
  const bool pos = !a.eval && j == 0;
  const int64_t rpad = a.RC - 1;
  const bool ok = s == 0 || ridx != rpad;
  if (lane == 0) a.valid[(size_t)n * a.S + s] = ok ? 1.f : 0.f;
  if (s == 0 && a.S <= 64) {        // valid positions of this sequence (lane l looks at position l) for the row list
    bool okl = lane == 0;
    if (lane > 0 && lane < a.S) {
      int b2, j2, rr2, sg2; int64_t rid2;
      seq_decode(a, n, lane, b2, j2, rid2, rr2, sg2);
      okl = rid2 != rpad;
    }
    const int cntv = __popcll(__ballot(okl));
    if (lane == 0) a.seqcnt[n] = cntv;
  }
  // per-position user / item embedding rows (ps_model.py:325-334).  The pad id addresses the table's last row,
  // which is READ like any other (nn.Embedding's padding_idx only stops its gradient) and never updated.
  int64_t uid = -1, iid = -1;
  if (a.user_emb) { uid = (pos ? a.pos_u : a.neg_u)[spos]; if (uid < 0 || uid > a.U) uid = -1; }
  if (a.item_emb) { iid = (pos ? a.pos_i : a.neg_i)[spos]; if (iid < 0 || iid > a.PI) iid = -1; }
  for (int cc0 = 0; cc0 < nch; cc0 += 32) {          // wave-uniform trip count: the shuffles below need every lane
    const int cc = cc0 + c;
    const bool act = cc < nch;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f), vcor = v;
    float cnt = 1.f;
    if (s == 0) {
      if (half == 0 && act) v = *reinterpret_cast<const float4*>(a.query_emb + (size_t)b * d + 4 * cc);
    } else if (ok) {
      const int r = s - 1;
      if (!a.pvc) {
        if (half == 0 && act) v = *reinterpret_cast<const float4*>(a.table + (size_t)rclamp(ridx, rpad) * d + 4 * cc);
        vcor = v;
      } else {
        // masked mean of the review's word rows; corrupted and (positive, train_pv) uncorrupted sums
        const int64_t* words;
        if (pos) words = (a.train_pv ? a.pos_pvc : a.pos_words) + ((size_t)b * a.R + r) * a.WL;
        else words = ((a.train_pv || a.eval) ? a.neg_pvc : a.neg_words_rev) + (size_t)revrow * a.WL;
        const uint8_t* wm = pos ? a.wmask_pos : a.wmask_neg;
        const size_t woff = (size_t)revrow * a.WL;
        const DropSpec& ts = pos ? a.t_pos : a.t_neg;
        // one Philox evaluation per (review, word slot): lane l owns slots l and l+64, the loop reads them by shuffle
        const float tm0 = drop_mult(ts, (uint32_t)revrow, (uint32_t)lane);
        const float tm1 = a.WL > 64 ? drop_mult(ts, (uint32_t)revrow, (uint32_t)(lane + 64)) : 1.f;
        // only the positive sequence under train_pv also needs the UNcorrupted sum; everywhere else a word whose
        // token mask is 0 (90 % of them at the reference's corrupt_rate) contributes nothing and is not fetched
        const bool need_unc = pos && a.train_pv;
        int nw = 0;
        if (a.WL <= 128) {
          // lane l holds word slots l and l+64 (two coalesced loads); the slots that survive the token mask are
          // compacted with ballots, so the row loop runs over ~10 % of the review at the reference's corrupt_rate
          const int64_t wa64 = lane < a.WL ? words[lane] : a.V - 1, wb64 = lane + 64 < a.WL ? words[lane + 64] : a.V - 1;
          const bool va = lane < a.WL && word_ok(a, wm, woff + lane, wa64), vb = lane + 64 < a.WL && word_ok(a, wm, woff + lane + 64, wb64);
          const int wa = va ? (int)wa64 : 0, wb = vb ? (int)wb64 : 0;
          unsigned long long ma = __ballot(va && (need_unc || tm0 != 0.f)), mb = __ballot(vb && (need_unc || tm1 != 0.f));
          // (the ballots are taken by the WHOLE wave, outside the half-wave select: inside it only lanes 0-31 would vote
          // and a review would never count more than 32 words)
          const int nvalid = __popcll(__ballot(va)) + __popcll(__ballot(vb));
          nw = half == 0 ? nvalid : 0;                                            // the halves are summed below
          while (ma | mb) {                                               // 8 word rows in flight per wave
            float4 rowv[4]; float mt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              int l0 = -1, s0 = 0, l1 = -1, s1 = 0;
              if (ma) { l0 = __ffsll((long long)ma) - 1; ma &= ma - 1; } else if (mb) { l0 = __ffsll((long long)mb) - 1; mb &= mb - 1; s0 = 1; }
              if (ma) { l1 = __ffsll((long long)ma) - 1; ma &= ma - 1; } else if (mb) { l1 = __ffsll((long long)mb) - 1; mb &= mb - 1; s1 = 1; }
              const int l = half ? l1 : l0, sl = half ? s1 : s0, src = l < 0 ? 0 : l;
              const int wia = __shfl(wa, src, 64), wib = __shfl(wb, src, 64);
              const float ta = __shfl(tm0, src, 64), tb = __shfl(tm1, src, 64);
              rowv[u] = make_float4(0.f, 0.f, 0.f, 0.f); mt[u] = 0.f;
              if (l >= 0) {
                const int wi = sl ? wib : wia;
                if (act) rowv[u] = *reinterpret_cast<const float4*>(a.word_emb + (size_t)wi * d + 4 * cc);
                mt[u] = sl ? tb : ta;
              }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              v.x += rowv[u].x; v.y += rowv[u].y; v.z += rowv[u].z; v.w += rowv[u].w;
              vcor.x += rowv[u].x * mt[u]; vcor.y += rowv[u].y * mt[u]; vcor.z += rowv[u].z * mt[u]; vcor.w += rowv[u].w * mt[u];
            }
          }
        } else
        for (int w0 = 0; w0 < a.WL; w0 += 8) {                 // 8 word rows in flight per wave
          float4 rowv[4]; float mt[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int w = w0 + 2 * u + half;
            int64_t wi = w < a.WL ? words[w] : a.V - 1;
            rowv[u] = make_float4(0.f, 0.f, 0.f, 0.f); mt[u] = 0.f;
            const float tmw = w < 64 ? __shfl(tm0, w & 63, 64) : (w < 128 ? __shfl(tm1, (w - 64) & 63, 64)
                                                                          : drop_mult(ts, (uint32_t)revrow, (uint32_t)w));
            if (w < a.WL && word_ok(a, wm, woff + w, wi)) {
              if (act && (need_unc || tmw != 0.f))
                rowv[u] = *reinterpret_cast<const float4*>(a.word_emb + (size_t)wi * d + 4 * cc);
              mt[u] = tmw;
              ++nw;
            }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            v.x += rowv[u].x; v.y += rowv[u].y; v.z += rowv[u].z; v.w += rowv[u].w;
            vcor.x += rowv[u].x * mt[u]; vcor.y += rowv[u].y * mt[u]; vcor.z += rowv[u].z * mt[u]; vcor.w += rowv[u].w * mt[u];
          }
        }
        nw += __shfl_xor(nw, 32, 64);
        cnt = (float)(nw > 0 ? nw : 1);
      }
    }
    // combine the two half-waves
    v.x += __shfl_xor(v.x, 32, 64); v.y += __shfl_xor(v.y, 32, 64); v.z += __shfl_xor(v.z, 32, 64); v.w += __shfl_xor(v.w, 32, 64);
    vcor.x += __shfl_xor(vcor.x, 32, 64); vcor.y += __shfl_xor(vcor.y, 32, 64);
    vcor.z += __shfl_xor(vcor.z, 32, 64); vcor.w += __shfl_xor(vcor.w, 32, 64);
    if (half != 0 || !act) continue;
    float o[4];
    if (s == 0) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
    else {
      const float inv = 1.f / cnt;
      float unc[4] = {v.x * inv, v.y * inv, v.z * inv, v.w * inv};
      float cor[4] = {vcor.x * inv, vcor.y * inv, vcor.z * inv, vcor.w * inv};
      const int rr = s - 1;
      if (a.pvc && lane == 0 && cc0 == 0) a.cnt[(size_t)n * a.R + rr] = cnt;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t col = (uint32_t)(4 * cc + e);
        float val;
        if (!a.pvc) {
          val = unc[e];
          if (pos && a.train_pv) {                               // PV.forward: drop_layer(review_emb) (PV.py:54)
            val *= drop_mult(a.d_pv, (uint32_t)revrow, col);
            a.vec[(size_t)revrow * d + col] = ok ? val : 0.f;
          }
        } else if (pos && a.train_pv) {
          val = unc[e];                                          // the sequence gets the UNcorrupted mean (PVC.py:76,95)
          a.vec[(size_t)revrow * d + col] = ok ? cor[e] : 0.f;    // the PV loss the corrupted one (PVC.py:78)
        } else {
          val = cor[e];
        }
        val *= drop_mult(pos ? a.d_pos : a.d_neg, (uint32_t)revrow, col);     // dropout_layer (ps_model.py:303-304)
        o[e] = val;
      }
      if (a.raw) {                                   // fs: the projection and the rest of x follow (rtm_fs_finish_kernel)
        const size_t rg = pos ? (size_t)revrow : (size_t)a.B * a.R + revrow;
        *reinterpret_cast<float4*>(a.raw + rg * d + 4 * cc) = ok ? make_float4(o[0], o[1], o[2], o[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        continue;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = 4 * cc + e;
      float val = o[e];
      if (a.use_seg) val += a.seg_emb[(size_t)seg * d + col];
      if (uid >= 0) val += a.user_emb[(size_t)uid * d + col];
      if (iid >= 0) val += a.item_emb[(size_t)iid * d + col];
      val = ok ? val : 0.f;
      if (a.use_pos) val += a.pe[(size_t)s * d + col];
      o[e] = val;
    }
    *reinterpret_cast<float4*>(a.x + ((size_t)n * a.S + s) * d + 4 * cc) = make_float4(o[0], o[1], o[2], o[3]);
  }
  // padded positive reviews still own a (zero) PV vector
  if (!ok && pos && a.train_pv && s > 0 && half == 0)
    for (int cc = c; cc < nch; cc += 32)
      *reinterpret_cast<float4*>(a.vec + (size_t)revrow * d + 4 * cc) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Which groups of four consecutive review rows hold at least one real review?  73 % of the review slots of a C4 batch are
// padding, and a launch over ALL groups spends most of its workgroup slots on waves that only find that out after a
// dependent load.  One thread per group: a group with a real review is appended to the list (wave-aggregated: one atomic
// per wave; the order of the list does not matter — a group's outputs are its own), a group of padding only has its key-mask
// flags and word counts written here and never reaches the gather launch (only used when padded rows of x are not read:
// `pads_unread`).  *gcount is cleared by the query-encoder launch (EmbedArgs::clear_word).
__global__ __launch_bounds__(256) void rtm_grouplist_kernel(const RtmK a, int npos_grp, int nneg_grp, FDiv fR, FDiv fK, int* glist,
                                                            int* gcount) {
  const int g = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const bool in = g < npos_grp + nneg_grp;
  const bool pos = g < npos_grp;
  const int gg = pos ? g : g - npos_grp;
  const int nrev = pos ? a.B * a.R : a.B * a.K * a.R;
  const int64_t rpad = a.RC - 1;
  bool any_ok = false;
  if (in) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int rr = 4 * gg + q;
      if (rr < nrev) any_ok |= (pos ? a.pos_r : a.neg_r)[rr] != rpad;
    }
    if (!any_ok) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rr = 4 * gg + q;
        if (rr >= nrev) continue;
        const int base = fdiv(rr, fR), r = rr - base * a.R;
        int n;
        if (pos) n = base * a.J;
        else { const int b = fdiv(base, fK); n = b * a.J + 1 + (base - b * a.K); }
        a.valid[(size_t)n * a.S + r + 1] = 0.f;
        a.cnt[(size_t)n * a.R + r] = 1.f;
      }
    }
  }
  const unsigned long long m = __ballot(in && any_ok);
  int base = 0;
  if (lane == 0 && m) base = atomicAdd(gcount, __popcll(m));
  base = __shfl(base, 0, 64);
  if (in && any_ok) glist[base + __popcll(m & ((1ull << lane) - 1ull))] = g;
}

// ------------------------------------------------------------------ embed forward, pvc encoder: four reviews per wave
// The per-slot kernel above spends most of its time in Philox: a wave (one review) evaluates the token masks of its word
// slots and the dropout words of its output columns, and every evaluation yields four words of which it uses ONE — the
// other three belong to the three neighbouring review rows (counter (col, row >> 2), word row & 3).  Here a wave owns
// the four review rows  4g .. 4g+3  of one side (positive: row b*R + r; negative: row (b*K + k)*R + r), so each
// evaluation serves four reviews (6x fewer Philox instructions), and the gather runs in four 16-lane groups, one review
// each (rows of d <= 256 floats in 16-byte chunks, c and c + 16, ...), four word rows in flight per group:
//   1. lane l reads word slots l and l + 64 of the four reviews (coalesced) and evaluates their token masks;
//   2. the surviving (word id, multiplier) pairs are compacted into one LDS list per review (ballot + prefix popcount);
//   3. group q walks list q, accumulating the corrupted (and, positive under train_pv, the uncorrupted) sum;
//   4. mean, dropout (the wave's 128 dropout evaluations shared through LDS), segment / user / item rows, key mask,
//      positional row -> x.   Query positions (s = 0) and the per-sequence counts ride as extra waves of the launch.
#define E4_LIST 128
template <int NCHL>
struct E4Lds {
  int wid[4][4][E4_LIST];          // [wave][review][entry]
  float tm[4][4][E4_LIST];
  uint32_t dw[4][64 * NCHL][4];    // [wave][column][review]: dropout words of the output row (d = 64 * NCHL columns)
};
template <int NCHL>     // 16-byte chunks per lane of a 16-lane group: d = 64 * NCHL
__global__ __launch_bounds__(256) void rtm_embed4_kernel(const RtmK a, int npos_grp, int nneg_grp, FDiv fR, FDiv fK, int pads_unread,
                                                         const int* __restrict__ glist, const int* __restrict__ gcount, int nq_wg, int diag_arg) {
  const int diag = PS_DIAG_ON ? diag_arg : 0;      // timing-only variants (WRONG results) exist in the diagnostic build only
  __shared__ E4Lds<NCHL> L;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#if PS_DIAG_ON      // in-kernel phase stamps: diagnostic build only
#define E4_STAMP(slot)                                                                             \
  do {                                                                                             \
    if (a.stamp && (int)blockIdx.x == nq_wg + 8 && lane == 0) {                                    \
      unsigned long long t_;                                                                       \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                   \
      a.stamp[16 * wv + (slot)] = t_;                                                              \
    }                                                                                              \
  } while (0)
#else
#define E4_STAMP(slot) do { } while (0)
#endif
  E4_STAMP(0);
  // PS_RTM_STAMP=1 PS_RTM_DIAG=64 (tools/rtm_wg_times.py): start / end time (s_memrealtime: the 100 MHz counter all CUs share —
  // s_memtime is per CU) and XCC of EVERY workgroup's wave 0, behind the phase slots
  const bool wg_times = a.stamp && diag == 64 && threadIdx.x == 0;
  if (wg_times) {
    unsigned long long t_;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
    a.stamp[64 + 3 * blockIdx.x] = t_;
    a.stamp[64 + 3 * blockIdx.x + 2] = (unsigned long long)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));   // HW_REG_XCC_ID bits 3:0
  }
  struct WgEnd {
    unsigned long long* p; bool on;
    __device__ ~WgEnd() {
      if (on) { unsigned long long t_; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); *p = t_; }
    }
  } wg_end = {wg_times ? a.stamp + 64 + 3 * blockIdx.x + 1 : nullptr, wg_times};
  int g = blockIdx.x * 4 + wv;
  if (glist) {
    // with the valid-group list (rtm_grouplist_kernel) the launch is DENSE in real work: the first nq_wg workgroups are the
    // query waves, the rest take groups from the list; waves past its end leave at once (no workgroup barrier in this kernel)
    if ((int)blockIdx.x < nq_wg) g = npos_grp + nneg_grp + (int)blockIdx.x * 4 + wv;
    else {
      const int gi = ((int)blockIdx.x - nq_wg) * 4 + wv;
      const int gsp = glist[gi];                     // requested WITH the count (the list has room for every group: in bounds)
      if (gi >= *gcount) return;
      g = gsp;
    }
  }
  g = __builtin_amdgcn_readfirstlane(g);            // wave-uniform: everything derived from it lives in scalar registers
  const int d = a.d;
  const int64_t rpad = a.RC - 1;
  if (g >= npos_grp + nneg_grp) {
    // ---- query position of sequence n (one wave): x[n][0], valid[n][0], the sequence's valid-position count
    const int n = g - npos_grp - nneg_grp;
    if (n >= a.B * a.J) return;
    const int b = fdiv(n, a.fJ), j = n - b * a.J;
    const bool pos = j == 0;
    const size_t base = pos ? (size_t)b : (size_t)b * a.K + (j - 1);
    const int64_t* rid = (pos ? a.pos_r : a.neg_r) + base * a.R;
    bool okl = lane == 0;
    if (lane > 0 && lane < a.S) okl = rid[lane - 1] != rpad;
    const int cntv = __popcll(__ballot(okl));
    if (lane == 0) { a.seqcnt[n] = cntv; a.valid[(size_t)n * a.S] = 1.f; }
    const size_t spos = base * a.S;
    const int seg = (int)(pos ? a.pos_seg : a.neg_seg)[spos];
    int64_t uid = -1, iid = -1;
    if (a.user_emb) { uid = (pos ? a.pos_u : a.neg_u)[spos]; if (uid < 0 || uid > a.U) uid = -1; }
    if (a.item_emb) { iid = (pos ? a.pos_i : a.neg_i)[spos]; if (iid < 0 || iid > a.PI) iid = -1; }
    for (int col = lane; col < d; col += 64) {
      float val = a.query_emb[(size_t)b * d + col];
      if (a.use_seg) val += a.seg_emb[(size_t)seg * d + col];
      if (uid >= 0) val += a.user_emb[(size_t)uid * d + col];
      if (iid >= 0) val += a.item_emb[(size_t)iid * d + col];
      if (a.use_pos) val += a.pe[col];
      a.x[(size_t)n * a.S * d + col] = val;
    }
    return;
  }
  const bool pos = g < npos_grp;
  const int gg = pos ? g : g - npos_grp;            // = review row >> 2 on its side: the Philox row counter
  const int nrev = pos ? a.B * a.R : a.B * a.K * a.R;
  const bool need_unc = pos && a.train_pv;
  const int64_t* wsrc = pos ? (a.train_pv ? a.pos_pvc : a.pos_words) : (a.train_pv ? a.neg_pvc : a.neg_words_rev);
  const DropSpec& ts = pos ? a.t_pos : a.t_neg;
  const DropSpec& ds = pos ? a.d_pos : a.d_neg;

  // ---- 1. the four reviews: where they sit
  int nq[4], sq[4], segq[4], nwq[4], nlq[4], rrq[4];
  bool okq[4], liveq[4];
  int64_t uidq[4], iidq[4];
  // lane l reads the id and the segment of review l & 3 (two wave-instructions, one round trip; the values then go to
  // scalar registers by v_readlane).  Review after review through wave-uniform loads — each followed by its own wait — the
  // decode was eight dependent round trips: 6.1 k of a workgroup's 10.7 k cycles (profiles/r03_rtm_embed4_stamps.txt)
  int my_rid_lo, my_rid_hi, my_seg;
  {
    const int rr = 4 * gg + (lane & 3);
    const int rrc = rr < nrev ? rr : 0;
    const int base = fdiv(rrc, fR), r = rrc - base * a.R;
    const int64_t rid = (pos ? a.pos_r : a.neg_r)[rrc];
    my_seg = (int)(pos ? a.pos_seg : a.neg_seg)[(size_t)base * a.S + r + 1];
    my_rid_lo = (int)(unsigned long long)rid; my_rid_hi = (int)((unsigned long long)rid >> 32);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int rr = 4 * gg + q;
    liveq[q] = rr < nrev;
    const int rrc = liveq[q] ? rr : 0;
    rrq[q] = rrc;
    const int base = fdiv(rrc, fR), r = rrc - base * a.R;
    const int bn = fdiv(base, fK);
    const int n = pos ? base * a.J : bn * a.J + 1 + (base - bn * a.K);
    nq[q] = n; sq[q] = r + 1;
    const int64_t ridx = (int64_t)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(my_rid_hi, q) << 32) |
                                   (unsigned)__builtin_amdgcn_readlane(my_rid_lo, q));
    okq[q] = liveq[q] && ridx != rpad;
    const size_t spos = (size_t)base * a.S + r + 1;
    segq[q] = __builtin_amdgcn_readlane(my_seg, q);
    uidq[q] = -1; iidq[q] = -1;
    if (a.user_emb) { uidq[q] = (pos ? a.pos_u : a.neg_u)[spos]; if (uidq[q] < 0 || uidq[q] > a.U) uidq[q] = -1; }
    if (a.item_emb) { iidq[q] = (pos ? a.pos_i : a.neg_i)[spos]; if (iidq[q] < 0 || iidq[q] > a.PI) iidq[q] = -1; }
    nwq[q] = 0; nlq[q] = 0;
  }
  // The word slots of the four reviews depend on the group number only, not on what the review ids turn out to be: they are
  // requested HERE, beside the ids and segments, by unconditional loads (slot clamped to the review's last) — one round trip
  // for both.  Fetched under `ok && lane < WL` selects, each of the eight loads sat behind its own branch, the compiler
  // waited for everything in flight at every join, and the whole block came a round trip after the ids.
  const uint8_t* const wm = pos ? a.wmask_pos : a.wmask_neg;
  const int la = min(lane, a.WL - 1), lb = min(lane + 64, a.WL - 1);
  int64_t waq[4], wbq[4];
  uint8_t mka[4] = {1, 1, 1, 1}, mkb[4] = {1, 1, 1, 1};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t* words = wsrc + (size_t)rrq[q] * a.WL;
    waq[q] = words[la];
    wbq[q] = words[lb];
  }
  if (wm) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { mka[q] = wm[(size_t)rrq[q] * a.WL + la]; mkb[q] = wm[(size_t)rrq[q] * a.WL + lb]; }
  }
  // 73 % of the review slots of a C4 batch are padding: a group without a real review skips the Philox evaluations, the
  // lists and the gather (wave-uniform branch) and only writes its masked rows
  const bool any_ok = okq[0] || okq[1] || okq[2] || okq[3];
  E4_STAMP(1);
  int cwa[4] = {-1, -1, -1, -1}, cwb[4] = {-1, -1, -1, -1};     // the counted words of slots lane / lane + 64 (-1: none)
  if (any_ok) {
    // ---- the word slots and their token masks
    Philox4 t0 = {0u, 0u, 0u, 0u}, t1 = {0u, 0u, 0u, 0u};
    if (ts.thr && !(diag & 8)) {
      t0 = philox4x32_10((uint32_t)lane, (uint32_t)gg, ts.site, drop_step(ts), ts.k0, ts.k1);
      if (a.WL > 64) t1 = philox4x32_10((uint32_t)lane + 64u, (uint32_t)gg, ts.site, drop_step(ts), ts.k0, ts.k1);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // word slots lane and lane + 64 of review q
      const int64_t wa64 = (okq[q] && lane < a.WL) ? waq[q] : a.V - 1;
      const int64_t wb64 = (okq[q] && lane + 64 < a.WL) ? wbq[q] : a.V - 1;
      const bool va = okq[q] && lane < a.WL && (wm ? mka[q] != 0 : wa64 != a.V - 1) && wa64 >= 0 && wa64 < a.V;      // = word_ok
      const bool vb = okq[q] && lane + 64 < a.WL && (wm ? mkb[q] != 0 : wb64 != a.V - 1) && wb64 >= 0 && wb64 < a.V;
      const uint32_t w0 = q == 0 ? t0.x : (q == 1 ? t0.y : (q == 2 ? t0.z : t0.w));
      const uint32_t w1 = q == 0 ? t1.x : (q == 1 ? t1.y : (q == 2 ? t1.z : t1.w));
      const float tm0 = ts.thr ? drop_word(ts, w0) : 1.f, tm1 = ts.thr ? drop_word(ts, w1) : 1.f;
      // ---- 2. compaction: entries of slots < 64 first, then slots >= 64 (ascending slot order, like the per-slot kernel)
      const bool ka = va && (need_unc || tm0 != 0.f), kb = vb && (need_unc || tm1 != 0.f);
      const unsigned long long ma = __ballot(ka), mb = __ballot(kb);
      const unsigned long long lt = (1ull << lane) - 1ull;
      nwq[q] = __popcll(__ballot(va)) + __popcll(__ballot(vb));
      nlq[q] = __popcll(ma) + __popcll(mb);
      cwa[q] = va ? (int)wa64 : -1; cwb[q] = vb ? (int)wb64 : -1;
      if (ka) { const int p = __popcll(ma & lt); L.wid[wv][q][p] = (int)wa64; L.tm[wv][q][p] = tm0; }
      if (kb) { const int p = __popcll(ma) + __popcll(mb & lt); L.wid[wv][q][p] = (int)wb64; L.tm[wv][q][p] = tm1; }
    }
  }
  // dropout words of the output row: lane evaluates columns lane, lane + 64, ... for the four reviews at once
  if (ds.thr && any_ok && !(diag & 2))
    for (int col = lane; col < d; col += 64) {
      const Philox4 r = philox4x32_10((uint32_t)col, (uint32_t)gg, ds.site, drop_step(ds), ds.k0, ds.k1);
      L.dw[wv][col][0] = r.x; L.dw[wv][col][1] = r.y; L.dw[wv][col][2] = r.z; L.dw[wv][col][3] = r.w;
    }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the lists are read back by other lanes of this wave only
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  E4_STAMP(2);
  // ---- 3. gather: group q = lane >> 4 walks list q
  const int q = lane >> 4, c = lane & 15;
  const int myn = q == 0 ? nlq[0] : (q == 1 ? nlq[1] : (q == 2 ? nlq[2] : nlq[3]));
  const int maxn = (diag & 1) ? 0 : max(max(nlq[0], nlq[1]), max(nlq[2], nlq[3]));       // diag: timing experiments only
  float4 v[NCHL], vc[NCHL];
#pragma unroll
  for (int k = 0; k < NCHL; ++k) { v[k] = make_float4(0.f, 0.f, 0.f, 0.f); vc[k] = v[k]; }
  const int* wl = L.wid[wv][q];
  const float* tl = L.tm[wv][q];
  constexpr int E4_U = 2;          // word rows REALLY in flight per 16-lane group now that their loads are unconditional (d = 128: 95 registers, five waves per SIMD; 3 measured the same, 4 costs a wave)
  for (int i0 = 0; i0 < maxn; i0 += E4_U) {
    float4 rowv[E4_U][NCHL]; float mt[E4_U], mo[E4_U];
#pragma unroll
    for (int u = 0; u < E4_U; ++u) {
      const bool on = i0 + u < myn;
      const int wi = on ? wl[i0 + u] : 0;
      mt[u] = on ? tl[i0 + u] : 0.f;
      mo[u] = on ? 1.f : 0.f;
      const float* row = a.word_emb + (size_t)wi * d + 4 * c;
      // (unconditional: an entry past this list reads row 0 and is weighted 0 — under `on ? load : 0` every one of the
      // E4_U x NCHL loads was its own branch and the compiler waited for all loads in flight at each join)
#pragma unroll
      for (int k = 0; k < NCHL; ++k) rowv[u][k] = *reinterpret_cast<const float4*>(row + 64 * k);
    }
#pragma unroll
    for (int u = 0; u < E4_U; ++u)
#pragma unroll
      for (int k = 0; k < NCHL; ++k) {
        v[k].x += rowv[u][k].x * mo[u]; v[k].y += rowv[u][k].y * mo[u]; v[k].z += rowv[u][k].z * mo[u]; v[k].w += rowv[u][k].w * mo[u];
        vc[k].x += rowv[u][k].x * mt[u]; vc[k].y += rowv[u][k].y * mt[u];
        vc[k].z += rowv[u][k].z * mt[u]; vc[k].w += rowv[u][k].w * mt[u];
      }
  }

  E4_STAMP(3);
  // ---- first pass of the backward's inverted index (RtmK::count_fwd): every counted word takes its RANK among the
  // occurrences of that word (a returning atomic on the word's counter, in flight under the rest of the kernel (issued in front of the gather instead they cost 4 us: measured)); the fill
  // then places the occurrence at  segment start + rank  without another atomic
  int rka[4] = {-1, -1, -1, -1}, rkb[4] = {-1, -1, -1, -1};
  if (a.count_fwd && any_ok) {
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      rka[qq] = cwa[qq] >= 0 ? atomicAdd(&a.wcnt[cwa[qq]], 1) : -1;
      rkb[qq] = cwb[qq] >= 0 ? atomicAdd(&a.wcnt[cwb[qq]], 1) : -1;
    }
  }
  // ---- 4. this group's review: mean, dropout, segment / user / item rows, mask, positional row
  const bool live = q == 0 ? liveq[0] : (q == 1 ? liveq[1] : (q == 2 ? liveq[2] : liveq[3]));
  if (live) {
  const bool ok = q == 0 ? okq[0] : (q == 1 ? okq[1] : (q == 2 ? okq[2] : okq[3]));
  const int n = q == 0 ? nq[0] : (q == 1 ? nq[1] : (q == 2 ? nq[2] : nq[3]));
  const int s = q == 0 ? sq[0] : (q == 1 ? sq[1] : (q == 2 ? sq[2] : sq[3]));
  const int seg = q == 0 ? segq[0] : (q == 1 ? segq[1] : (q == 2 ? segq[2] : segq[3]));
  const int nw = q == 0 ? nwq[0] : (q == 1 ? nwq[1] : (q == 2 ? nwq[2] : nwq[3]));
  const int64_t uid = q == 0 ? uidq[0] : (q == 1 ? uidq[1] : (q == 2 ? uidq[2] : uidq[3]));
  const int64_t iid = q == 0 ? iidq[0] : (q == 1 ? iidq[1] : (q == 2 ? iidq[2] : iidq[3]));
  const int rr = 4 * gg + q;
  const float cntf = (float)(nw > 0 ? nw : 1), inv = 1.f / cntf;
  if (c == 0) { a.valid[(size_t)n * a.S + s] = ok ? 1.f : 0.f; a.cnt[(size_t)n * a.R + s - 1] = cntf; }
  const bool skip_row = (!ok && pads_unread && !need_unc) || (diag & 4);
  // segment / positional (/ user / item) rows of this position, all chunks at once (each behind its own per-element test
  // before: a round trip per element)
  float4 addv[NCHL], pev[NCHL];       // addv: segment + user + item rows (summed in that order, as the per-element form did)
#pragma unroll
  for (int k = 0; k < NCHL; ++k) { addv[k] = make_float4(0.f, 0.f, 0.f, 0.f); pev[k] = addv[k]; }
  if (!skip_row && !a.raw) {
    if (a.use_seg) {
#pragma unroll
      for (int k = 0; k < NCHL; ++k) addv[k] = *reinterpret_cast<const float4*>(a.seg_emb + (size_t)seg * d + 4 * c + 64 * k);
    }
    if (a.use_pos) {
#pragma unroll
      for (int k = 0; k < NCHL; ++k) pev[k] = *reinterpret_cast<const float4*>(a.pe + (size_t)s * d + 4 * c + 64 * k);
    }
  }
#pragma unroll
  for (int k = 0; k < NCHL; ++k) {
    if (skip_row) break;
    const int col0 = 4 * c + 64 * k;
    const float sg4[4] = {addv[k].x, addv[k].y, addv[k].z, addv[k].w}, pe4[4] = {pev[k].x, pev[k].y, pev[k].z, pev[k].w};
    const float unc[4] = {v[k].x * inv, v[k].y * inv, v[k].z * inv, v[k].w * inv};
    const float cor[4] = {vc[k].x * inv, vc[k].y * inv, vc[k].z * inv, vc[k].w * inv};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = col0 + e;
      float val = need_unc ? unc[e] : cor[e];        // the sequence gets the UNcorrupted mean under train_pv (PVC.py:76,95)
      if (ds.thr && ok) val *= drop_word(ds, L.dw[wv][col][q]);                   // dropout_layer (ps_model.py:303-304)
      if (a.raw) { o[e] = ok ? val : 0.f; continue; }                             // fs: rtm_fs_finish_kernel does the rest
      if (a.use_seg) val += sg4[e];
      if (uid >= 0) val += a.user_emb[(size_t)uid * d + col];       // (user / item rows: not in configs[3]; per element as before)
      if (iid >= 0) val += a.item_emb[(size_t)iid * d + col];
      val = ok ? val : 0.f;
      if (a.use_pos) val += pe4[e];
      o[e] = val;
    }
    if (a.raw) {
      const size_t rg = pos ? (size_t)rr : (size_t)a.B * a.R + rr;
      *reinterpret_cast<float4*>(a.raw + rg * d + col0) = make_float4(o[0], o[1], o[2], o[3]);
      continue;
    }
    *reinterpret_cast<float4*>(a.x + ((size_t)n * a.S + s) * d + col0) = make_float4(o[0], o[1], o[2], o[3]);
    if (need_unc)                                   // the PV loss predicts from the corrupted mean (PVC.py:78)
      *reinterpret_cast<float4*>(a.vec + (size_t)rr * d + col0) =
          ok ? make_float4(cor[0], cor[1], cor[2], cor[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  }
  if (a.count_fwd && any_ok) {
#pragma unroll
    for (int qq = 0; qq < 4; ++qq)
      if (okq[qq]) {
        int* rk = a.wrank + ((size_t)(pos ? 0 : a.B * a.R) + rrq[qq]) * a.WL;
        if (lane < a.WL) rk[lane] = rka[qq];
        if (lane + 64 < a.WL) rk[lane + 64] = rkb[qq];
      }
  }
  E4_STAMP(4);
#undef E4_STAMP
}

// uncorrupted pvc review table for eval: out[i] = mean of the review's word rows, last row 0 (ps_model.py:186-203)
__global__ __launch_bounds__(256) void rtm_review_table_kernel(const float* word_emb, const int64_t* review_words, float* out,
                                                               int64_t RC, int WL, int d, int64_t V) {
  const int lane = threadIdx.x & 63;
  const int64_t rev = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (rev >= RC) return;
  for (int e = lane; e < d; e += 64) {
    float s = 0.f; int cnt = 0;
    if (rev < RC - 1)
      for (int w = 0; w < WL; ++w) {
        const int64_t wi = review_words[rev * WL + w];
        if (wi != V - 1 && wi >= 0 && wi < V) { s += word_emb[(size_t)wi * d + e]; ++cnt; }
      }
    out[rev * d + e] = s / (float)(cnt > 0 ? cnt : 1);
  }
}

// ------------------------------------------------------------------ fs review encoder (text_encoder.py:32-40)
// forward tail: x[n][s] = (valid ? tanh-projection + segment / user / item rows : 0) + pe[s]; one wave per review slot
__global__ __launch_bounds__(256) void rtm_fs_finish_kernel(const RtmK a) {
  const int lane = threadIdx.x & 63;
  const int slot = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (slot >= a.B * a.J * a.S) return;
  const int n = fdiv(slot, a.fS), s = slot - n * a.S;
  if (s == 0) return;                                   // query rows were written by the embed kernel
  int b, j, revrow, seg; int64_t ridx; size_t spos;
  seq_decode(a, n, s, b, j, ridx, revrow, seg, &spos);
  const bool pos = j == 0, ok = ridx != a.RC - 1;
  const size_t rg = pos ? (size_t)revrow : (size_t)a.B * a.R + revrow;
  int64_t uid = -1, iid = -1;
  if (a.user_emb) { uid = (pos ? a.pos_u : a.neg_u)[spos]; if (uid < 0 || uid > a.U) uid = -1; }
  if (a.item_emb) { iid = (pos ? a.pos_i : a.neg_i)[spos]; if (iid < 0 || iid > a.PI) iid = -1; }
  const int d = a.d;
  for (int col = lane; col < d; col += 64) {
    float val = 0.f;
    if (ok) {
      val = a.yfs[rg * d + col];
      if (a.use_seg) val += a.seg_emb[(size_t)seg * d + col];
      if (uid >= 0) val += a.user_emb[(size_t)uid * d + col];
      if (iid >= 0) val += a.item_emb[(size_t)iid * d + col];
    }
    if (a.use_pos) val += a.pe[(size_t)s * d + col];
    a.x[((size_t)n * a.S + s) * d + col] = val;
  }
}

// ------------------------------------------------------------------ host side
bool rtm_embed4_taken(const PsRtmDesc& D, bool eval, const RtmWs& r) {
  static const bool e4_on = ps_diag_int("PS_RTM_EMBED4", 1) != 0;
  return e4_on && D.review_encoder != PS_RENC_PV && !eval && D.WL <= 128 && (D.d == 64 || D.d == 128 || D.d == 256) && r.S <= 64;
}

int rtm_embed_fwd(const PsRtmDesc& D, const RtmK& k, float* ws, const RtmWs& r, bool eval, bool rowlist, hipStream_t st) {
  const int B = D.B, d = D.d;
  {
    KTimeScope kt("rtm_embed", st);
    if (rtm_embed4_taken(D, eval, r)) {
      const int npos = ps_cdiv((int64_t)B * D.R, 4), nneg = ps_cdiv((int64_t)B * D.K * D.R, 4);
      const dim3 grid(ps_cdiv(npos + nneg + r.Bseq, 4));
      // x rows of padded positions: with the valid-row list nothing downstream reads them (the projections, the attention and
      // the backward all walk the list), so they are not written either (18 us of the launch at C4, 73 % padding)
      static const bool keep_pads = ps_diag_int("PS_RTM_WRITE_PADS", 0) != 0;
      const int pads_unread = rowlist && !k.raw && !keep_pads ? 1 : 0;
      const FDiv fR = make_fdiv(D.R), fK = make_fdiv(D.K > 0 ? D.K : 1);
      // the valid-group list (rtm_grouplist_kernel): only when padded rows of x are not read and the counter is cleared by
      // the query-encoder launch (training).  PS_RTM_GROUPLIST=0: every group gets a wave, as in round 2.
      static const int e4_diag = ps_diag_int("PS_RTM_DIAG", 0);      // timing experiments (wrong results)
      static const bool list_on = ps_env_int("PS_RTM_GROUPLIST", 1) != 0;
      const int* glist = nullptr; const int* gcount = nullptr;
      const int nq_wg = ps_cdiv(r.Bseq, 4);
      dim3 egrid = grid;
      if (list_on && pads_unread && !eval && r.glist && !k.train_pv) {
        int* gl = reinterpret_cast<int*>(ws + r.glist);
        int* gc = reinterpret_cast<int*>(ws + r.loss_blk) + 2;
        hipLaunchKernelGGL(rtm_grouplist_kernel, dim3(ps_cdiv(npos + nneg, 256)), dim3(256), 0, st, k, npos, nneg, fR, fK, gl, gc);
        PS_LAUNCH_CHECK();
        glist = gl; gcount = gc;
        egrid = dim3(nq_wg + ps_cdiv(npos + nneg, 4));
      }
      if (d == 64) PS_KLAUNCH(rtm_embed4_kernel<1>, egrid, dim3(256), 0, st, k, npos, nneg, fR, fK, pads_unread, glist, gcount, nq_wg, e4_diag);
      else if (d == 128) PS_KLAUNCH(rtm_embed4_kernel<2>, egrid, dim3(256), 0, st, k, npos, nneg, fR, fK, pads_unread, glist, gcount, nq_wg, e4_diag);
      else PS_KLAUNCH(rtm_embed4_kernel<4>, egrid, dim3(256), 0, st, k, npos, nneg, fR, fK, pads_unread, glist, gcount, nq_wg, e4_diag);
    } else {
      PS_KLAUNCH(rtm_embed_kernel, dim3(ps_cdiv(r.Bseq * r.S, 4)), dim3(256), 0, st, k);
    }
  }
  PS_LAUNCH_CHECK();
  return PS_OK;
}

int rtm_fs_finish(const RtmK& k, const RtmWs& r, hipStream_t st) {
  hipLaunchKernelGGL(rtm_fs_finish_kernel, dim3(ps_cdiv(r.Bseq * r.S, 4)), dim3(256), 0, st, k);
  PS_LAUNCH_CHECK();
  return PS_OK;
}

int rtm_rowlist(const RtmK& k, const RtmWs& r, hipStream_t st) {
  hipLaunchKernelGGL(rtm_rowlist_kernel, dim3(ps_cdiv(r.Bseq, 4)), dim3(256), 0, st, k);
  PS_LAUNCH_CHECK();
  return PS_OK;
}

int rtm_review_table(const PsRtmDesc& D, const float* word_emb, const int64_t* review_words, float* out, hipStream_t st) {
  hipLaunchKernelGGL(rtm_review_table_kernel, dim3(ps_cdiv(D.review_count, 4)), dim3(256), 0, st,
                     word_emb, review_words, out, D.review_count, D.WL, D.d, D.vocab_size);
  PS_LAUNCH_CHECK();
  return PS_OK;
}
