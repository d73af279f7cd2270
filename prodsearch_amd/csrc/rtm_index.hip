// rtm_index.hip — the inverted index word -> review slots of the word-mean review encoders' backward (pvc / fs / avg) and the
// word-gradient reduce over it: the atomic-cursor index (its count pass also rides in rtm_embed4_kernel, rtm_embed.hip), the
// LDS-histogram index, the run-length reduce and deterministic mode's ordered reduce.  Host stages at the end (rtm.h).
#include "rtm.h"

// segment of every word in the occurrence list, cursor reset.  wreduce needs a word's occurrences CONTIGUOUS, not the
// segments in word order, so instead of a scan (one workgroup, 27 us for 32k words) every wave sums its 64 counts and
// bumps one running total (`tot`, zeroed with the counts) by the sum; the total ends as the list length.
__global__ __launch_bounds__(256) void rtm_walloc_kernel(const int* cnt, int* off, int* cur, int* tot, int V) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = w < V ? cnt[w] : 0;
  int incl = c;                                            // inclusive prefix over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  const int total = __shfl(incl, 63, 64);
  int base = 0;
  if (lane == 63 && total > 0) base = atomicAdd(tot, total);
  base = __shfl(base, 63, 64);
  if (w < V) { off[w] = base + incl - c; cur[w] = 0; }
}

// ---- the inverted index word -> review slots: count, allocate (rtm_walloc_kernel), fill.
// The index depends on the batch's indices only, not on any gradient (rtm_index_in_forward).  Round 1 walked the slots one
// wave per slot, 38 slots in a row per wave: each step of that walk is a chain of dependent reads (review id -> word ids ->
// atomic), 56 us to count and 70 us to fill.  (Aggregating a workgroup's words in an LDS hash table first was measured and
// is slower: a chunk's words are mostly distinct, the popular ones are not what costs.)  Now
//   * the count rides in rtm_embed4_kernel, which has every word id in registers anyway (RtmK::count_fwd);
//   * the fill (and the count, when it does not ride) flattens a chunk of slots: the workgroup lists its real reviews, then
//     its threads stride over (review, word slot) pairs, four independent reads / atomics in flight per lane.
#define WI_CHUNK_MAX 256
template <int FILL>     // 0: count, 1: fill (a returning atomic on the word's cursor per occurrence), 2: fill from the ranks
__global__ __launch_bounds__(256) void rtm_windex_kernel(const RtmK a, int chunk, FDiv fWL) {
  __shared__ int l_rev[WI_CHUNK_MAX], l_slot[WI_CHUNK_MAX];     // rev: review row on its side, ~row for a positive
  __shared__ int l_n;
  const int tid = threadIdx.x, lane = tid & 63;
  const int nslots = a.B * a.J * a.S;
  const int64_t rpad = a.RC - 1;
  if (tid == 0) l_n = 0;
  __syncthreads();
  {
    const int slot = (int)blockIdx.x * chunk + tid;
    bool real = false; int enc = 0;
    if (tid < chunk && slot < nslots) {
      const int n = fdiv(slot, a.fS), s = slot - n * a.S;
      if (s > 0) {
        int b, j, seg, rev; int64_t ridx;
        seq_decode(a, n, s, b, j, ridx, rev, seg);
        real = ridx != rpad;
        enc = j == 0 ? ~rev : rev;
      }
    }
    const unsigned long long m = __ballot(real);
    int base = 0;
    if (lane == 0 && m) base = atomicAdd(&l_n, __popcll(m));
    base = __shfl(base, 0, 64);
    if (real) { const int at = base + __popcll(m & ((1ull << lane) - 1ull)); l_rev[at] = enc; l_slot[at] = slot; }
  }
  __syncthreads();
  const int total = l_n * a.WL;
  for (int i0 = tid; i0 < total; i0 += 4 * 256) {
    int64_t wi[4]; int sl[4], rk[4]; bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + 256 * u;
      const bool in = i < total;
      const int r = in ? fdiv(i, fWL) : 0, w = i - r * a.WL;
      const int enc = l_rev[r];
      const bool pos = enc < 0;
      const int rev = pos ? ~enc : enc;
      const int64_t* words = (pos ? (a.train_pv ? a.pos_pvc : a.pos_words) : (a.train_pv ? a.neg_pvc : a.neg_words_rev));
      const uint8_t* wm = pos ? a.wmask_pos : a.wmask_neg;
      const size_t off = (size_t)rev * a.WL + (in ? w : 0);
      wi[u] = in ? words[off] : -1;
      if (FILL >= 2) {
        const size_t grow = (size_t)(pos ? 0 : a.B * a.R) + rev;
        rk[u] = in ? a.wrank[grow * a.WL + w] : -1;
        ok[u] = rk[u] >= 0;
      } else {
        ok[u] = in && word_ok(a, wm, off, wi[u]);
      }
      sl[u] = l_slot[r];
    }
    if (FILL == 0) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u]) atomicAdd(&a.wcnt[wi[u]], 1);
    } else {
      int at[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        at[u] = !ok[u] ? 0 : a.woff[wi[u]] + (FILL >= 2 ? rk[u] : atomicAdd(&a.wcur[wi[u]], 1));
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (ok[u]) a.wl[at[u]] = make_int2(sl[u], (int)wi[u]);
    }
  }
}

// ---- the index WITHOUT global atomics (round 3).  Timing-only variants of rtm_embed4_kernel showed its per-occurrence returning
// atomics (1.16 M scattered 4-byte atomics: the memory-side rate for one dword per lane in 64 different lines) cost 45 of its
// 97 us, and kernels of such atomics slow whatever runs beside them.  Counting sort by word with the histogram in LDS instead:
//   rtm_hist_kernel      RTM_HIST_G workgroups, each owns a contiguous range of review rows and the WHOLE vocabulary as an LDS
//                        histogram (4 B x V <= 160 KB): an occurrence's rank inside its partition is a returning LDS atomic;
//                        ranks -> wrank (-1: not counted), the partition's histogram -> hist[g][.]
//   rtm_hist_scan_kernel per word: exclusive prefix of the partitions' counts, the word's total, and (folded in: the wave-sum +
//                        one bump of the running total that rtm_walloc_kernel does) the word's segment start; hist[g][w] becomes
//                        the list position of partition g's first occurrence of w
//   rtm_hist_fill_kernel the partitions again, their row of positions in LDS: position + rank, one 8-byte store per occurrence
// All of it on the side stream at the start of the backward; the forward's gather carries no atomics at all.
// (First form, measured: 128 partitions, a one-thread-per-word scan (26 us: 128 dependent strided reads per thread) and the fill
// as rtm_windex_kernel reading hist[g][w] per occurrence (59 us: a random 4-byte read in a 16 MB table each) — the gather fell
// 97 -> 52 us but the step ROSE 0.449 -> 0.462 ms.)
__device__ inline int hist_list_rows(const RtmK& a, int base, int row1, int* l_rev, int* l_n) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int64_t rpad = a.RC - 1;
  if (tid == 0) *l_n = 0;
  __syncthreads();
  const int grow = base + tid;
  bool real = false;
  if (grow < row1) {
    const bool pos = grow < a.B * a.R;
    real = (pos ? a.pos_r[grow] : a.neg_r[grow - a.B * a.R]) != rpad;
  }
  const unsigned long long m = __ballot(real);
  int at0 = 0;
  if (lane == 0 && m) at0 = atomicAdd(l_n, __popcll(m));     // (one wave when the order matters: DET)
  at0 = __shfl(at0, 0, 64);
  if (real) l_rev[at0 + __popcll(m & ((1ull << lane) - 1ull))] = grow;
  __syncthreads();
  return *l_n;
}
// FILL 0: histogram + ranks, 1: fill the list from the ranks and the partition's positions.
// NT threads.  DET (deterministic mode, NT = 64): ONE wave walks the partition in task order and hands out the ranks without
// atomics — per batch of 64 occurrences a lane counts the lower lanes holding its word, every lane reads the word's counter,
// the last lane of each word adds the word's batch count — so a word's occurrences sit in its segment in task order.
template <int FILL, int NT, int DET>
__global__ __launch_bounds__(NT) void rtm_hist_kernel(const RtmK a) {
  extern __shared__ int hist_lds[];                 // [V]: FILL 0 the partition's counts, FILL 1 its list positions
  __shared__ int l_rev[NT];                         // this partition's real reviews: global review row
  __shared__ int l_n;
  static_assert(!DET || NT == 64, "the deterministic ranks are one wave's");
  const int tid = threadIdx.x;
  const int g = blockIdx.x, NP = a.B * a.R, NR = NP + a.B * a.K * a.R;
  for (int i = tid; i < a.V; i += NT) hist_lds[i] = FILL ? a.hist[(size_t)g * a.V + i] : 0;
  const int row0 = g * a.hist_rows, row1 = min(row0 + a.hist_rows, NR);
  for (int base = row0; base < row1; base += NT) {             // lists of up to NT rows at a time
    const int total = hist_list_rows(a, base, row1, l_rev, &l_n) * a.WL;
    for (int ib = 0; ib < total; ib += 4 * NT) {               // (workgroup-uniform trip count: DET shuffles below)
      int64_t wi[4]; size_t ro[4]; bool ok[4]; int rk[4], sl[4]; const uint8_t* wmo[4] = {nullptr, nullptr, nullptr, nullptr};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = ib + NT * u + tid;
        const bool in = i < total;
        const int ic = in ? i : 0;                             // (a slot past the end repeats slot 0: every load below is
        const int r = ic / a.WL, w = ic - r * a.WL;            // unconditional — under `in ? load : -1` each was its own branch
        const int gr = l_rev[r];                               // and the four, or eight, round trips of a pass ran one by one)
        const bool pos = gr < NP;
        const int rev = pos ? gr : gr - NP;
        const int64_t* words = (pos ? (a.train_pv ? a.pos_pvc : a.pos_words) : (a.train_pv ? a.neg_pvc : a.neg_words_rev));
        const size_t off = (size_t)rev * a.WL + w;
        wi[u] = words[off];
        if (!in) wi[u] = -1;
        ro[u] = (size_t)gr * a.WL + w;
        if (FILL) {
          rk[u] = a.wrank[ro[u]];
          if (!in) rk[u] = -1;
          ok[u] = rk[u] >= 0;
          // the slot of review row `rev` (the inverse of seq_decode: sequence n = b*J + j, position r + 1)
          const int seq = rev / a.R, r_in = rev - seq * a.R;
          int n;
          if (pos) n = seq * a.J;
          else { const int b = seq / a.K; n = b * a.J + (seq - b * a.K) + 1; }
          sl[u] = n * a.S + r_in + 1;
        } else {
          wmo[u] = (pos ? a.wmask_pos : a.wmask_neg) + off;
          ok[u] = in;
        }
      }
      if (!FILL) {                                             // word_ok, the mask bytes (if the batch has any) in one request
        uint8_t mk[4] = {1, 1, 1, 1};
        if (a.wmask_pos && a.wmask_neg) {
#pragma unroll
          for (int u = 0; u < 4; ++u) mk[u] = *wmo[u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          ok[u] = ok[u] && ((a.wmask_pos && a.wmask_neg) ? mk[u] != 0 : wi[u] != a.V - 1) && wi[u] >= 0 && wi[u] < a.V;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = ib + NT * u + tid;
        if (FILL) {
          if (ok[u]) a.wl[hist_lds[wi[u]] + rk[u]] = make_int2(sl[u], (int)wi[u]);
        } else if (DET) {
          const int w = ok[u] ? (int)wi[u] : -1;
          int before = 0, same = 0;
          for (int l = 0; l < 64; ++l) {
            const int o = __shfl(w, l, 64);
            same += o == w ? 1 : 0;
            before += (o == w && l < tid) ? 1 : 0;
          }
          const int at = ok[u] ? hist_lds[w] : 0;              // every lane reads before any lane writes (one wave, in order)
          asm volatile("" ::: "memory");
          if (ok[u] && before == same - 1) hist_lds[w] = at + same;
          asm volatile("" ::: "memory");
          if (i < total) a.wrank[ro[u]] = ok[u] ? at + before : -1;
        } else if (i < total) {
          a.wrank[ro[u]] = ok[u] ? atomicAdd(&hist_lds[wi[u]], 1) : -1;
        }
      }
    }
    __syncthreads();
  }
  if (!FILL)
    for (int i = tid; i < a.V; i += NT) a.hist[(size_t)g * a.V + i] = hist_lds[i];
}
// 64 words x 8 groups of RTM_HIST_G/8 partitions per workgroup: every lane has its group's counts in registers at once
// (independent loads), the groups meet in LDS, wave 0 allocates the 64 segments (wave prefix + ONE bump of the running total)
__global__ __launch_bounds__(512) void rtm_hist_scan_kernel(int* hist, int* wcnt, int* woff, int* tot, int V) {
  __shared__ int l_tot[8][64];
  __shared__ int l_base[64];
  constexpr int PG = RTM_HIST_G / 8;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = blockIdx.x * 64 + lane;
  const bool in = w < V;
  int c[PG];
#pragma unroll
  for (int g = 0; g < PG; ++g) c[g] = in ? hist[(size_t)(wv * PG + g) * V + w] : 0;
  int run = 0;
#pragma unroll
  for (int g = 0; g < PG; ++g) { const int t = c[g]; c[g] = run; run += t; }
  l_tot[wv][lane] = run;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) { const int t = l_tot[q][lane]; before += q < wv ? t : 0; total += t; }
  if (wv == 0) {
    int incl = total;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    const int all = __shfl(incl, 63, 64);
    int base = 0;
    if (lane == 63 && all > 0) base = atomicAdd(tot, all);
    base = __shfl(base, 63, 64) + incl - total;
    l_base[lane] = base;
    if (in) { woff[w] = base; wcnt[w] = total; }
  }
  __syncthreads();
  const int start = l_base[lane] + before;
  if (in) {
#pragma unroll
    for (int g = 0; g < PG; ++g) hist[(size_t)(wv * PG + g) * V + w] = start + c[g];
  }
}

// segmented sum over the word-sorted occurrence list: a wave owns 64 consecutive entries, adds the slot rows of a
// run of equal words in registers and issues ONE atomic row per run (runs spanning waves meet in the atomics)
__global__ __launch_bounds__(256) void rtm_wreduce_kernel(const RtmK a) {
  const int lane = threadIdx.x & 63;
  const int wave0 = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6)), nwave = (gridDim.x * blockDim.x) >> 6;
  const int T = a.wcnt[a.V];                         // the allocator's total (rtm_walloc_kernel)
  const int d = a.d;                                 // lane l owns columns l, l+64, ... (< d <= 512)
  // (the list length is only known on the device: a capped grid strides over it instead of one workgroup per 256 POSSIBLE
  // occurrences, 30,000 launches of which 25,000 found nothing to do)
  for (int base = wave0 * 64; base < T; base += nwave * 64) {
  const int e = base + lane;
  const int2 mine = e < T ? a.wl[e] : make_int2(-1, -1);
  const int my_slot = mine.x, my_word = mine.y;
  const int n = min(64, T - base);
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  int cur = __builtin_amdgcn_readlane(my_word, 0);
  if (d <= 128) {
    // d <= 128 (two columns per lane): 8 slot rows are requested before the first is added — one by one the loop is a
    // chain of 64 dependent L2 round trips per wave (149 us for the 594 MB of a C4 step)
    const int c0 = lane < d ? lane : d - 1, c1 = lane + 64 < d ? lane + 64 : d - 1;
    constexpr int WR_U = 16;                         // rows in flight (unconditional loads: a dead entry repeats row 0)
    for (int i0 = 0; i0 < n; i0 += WR_U) {
      float r0[WR_U], r1[WR_U];
#pragma unroll
      for (int u = 0; u < WR_U; ++u) {
        const int sl = __builtin_amdgcn_readlane(my_slot, (i0 + u) & 63);
        const bool live = i0 + u < n;
        const float* row = a.gs + (size_t)(live ? sl : 0) * d;
        r0[u] = row[c0];
        r1[u] = row[c1];
      }
#pragma unroll
      for (int u = 0; u < WR_U; ++u) {
        if (i0 + u < n) {                            // wave-uniform
          const int w = __builtin_amdgcn_readlane(my_word, (i0 + u) & 63);
          if (w != cur) {
            float* grow = a.g_word_emb + (size_t)cur * d;
            if (lane < d) { atomicAdd(&grow[lane], acc[0]); acc[0] = 0.f; }
            if (lane + 64 < d) { atomicAdd(&grow[lane + 64], acc[1]); acc[1] = 0.f; }
            cur = w;
          }
          acc[0] += r0[u]; acc[1] += r1[u];
        }
      }
    }
  } else
  for (int i = 0; i < n; ++i) {
    const int w = __shfl(my_word, i, 64), sl = __shfl(my_slot, i, 64);
    if (w != cur) {
      float* grow = a.g_word_emb + (size_t)cur * d;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (lane + 64 * k < d) { atomicAdd(&grow[lane + 64 * k], acc[k]); acc[k] = 0.f; }
      cur = w;
    }
    const float* row = a.gs + (size_t)sl * d;
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (lane + 64 * k < d) acc[k] += row[lane + 64 * k];
  }
  float* grow = a.g_word_emb + (size_t)cur * d;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (lane + 64 * k < d) atomicAdd(&grow[lane + 64 * k], acc[k]);
  }
}

// deterministic mode (ps_deterministic; the ranks come from rtm_hist_kernel<0, 64, 1>).
// The word-gradient reduce: a word's occurrences in list order (= task order, see the ranks) by ONE wave, plain add into the
// word's row (its sole writer in this launch).  Words with more than WR_DET_LIM occurrences (Zipf heads: tens of thousands) go
// to a list — its order does not matter — and get a 16-wave workgroup each: wave k sums the k-th sixteenth of the segment, the
// sixteen partials are added in wave order.
#define WR_DET_LIM 4096
template <int NK>
__device__ inline void wr_det_sum(const RtmK& a, int off, int n, int lane, float (&acc)[NK]) {
  constexpr int U = NK <= 2 ? 16 : 4;
  const int d = a.d;
  int col[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) { acc[k] = 0.f; col[k] = lane + 64 * k < d ? lane + 64 * k : d - 1; }
  for (int i0 = 0; i0 < n; i0 += U) {
    float r[U][NK];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int sl = a.wl[off + (i0 + u < n ? i0 + u : i0)].x;
      const float* row = a.gs + (size_t)sl * d;
#pragma unroll
      for (int k = 0; k < NK; ++k) r[u][k] = row[col[k]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i0 + u < n) {
#pragma unroll
        for (int k = 0; k < NK; ++k) acc[k] += r[u][k];
      }
  }
}
template <int NK>
__global__ __launch_bounds__(256) void rtm_wreduce_det_kernel(const RtmK a, int* heavy, int* nheavy) {
  const int lane = threadIdx.x & 63;
  const int wave0 = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwave = (gridDim.x * blockDim.x) >> 6;
  for (int w = wave0; w < (int)a.V; w += nwave) {
    const int n = a.wcnt[w];
    if (n == 0) continue;
    if (n > WR_DET_LIM) { if (lane == 0) heavy[atomicAdd(nheavy, 1)] = w; continue; }
    float acc[NK];
    wr_det_sum<NK>(a, a.woff[w], n, lane, acc);
    float* grow = a.g_word_emb + (size_t)w * a.d;
#pragma unroll
    for (int k = 0; k < NK; ++k)
      if (lane + 64 * k < a.d) grow[lane + 64 * k] += acc[k];
  }
}
template <int NK>
__global__ __launch_bounds__(1024) void rtm_wreduce_heavy_det_kernel(const RtmK a, const int* heavy, const int* nheavy) {
  __shared__ float part[16][64 * NK];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int h = blockIdx.x; h < *nheavy; h += gridDim.x) {
    const int w = heavy[h], n = a.wcnt[w], per = (n + 15) / 16;
    const int i0 = wv * per, cnt = max(0, min(n, i0 + per) - i0);
    float acc[NK];
    wr_det_sum<NK>(a, a.woff[w] + i0, cnt, lane, acc);
#pragma unroll
    for (int k = 0; k < NK; ++k) part[wv][lane + 64 * k] = acc[k];
    __syncthreads();
    for (int e = threadIdx.x; e < a.d; e += 1024) {
      float t = 0.f;
      for (int q = 0; q < 16; ++q) t += part[q][e];
      a.g_word_emb[(size_t)w * a.d + e] += t;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ host side
// (Round 3, measured and dropped: the whole index built on the side stream BESIDE the forward, so that the forward carries no
// atomics.  Kernels of scattered global atomics poison whatever runs next to them: the gather launch stayed at 97 us without its
// atomics, a 3 us list kernel took 44 us, the step went 0.454 -> 0.507 ms.  Timing-only variants of rtm_embed4_kernel show the
// rank atomics cost 45 of its 97 us — the fix is fewer global atomics, not a different place for them.)
// the LDS-histogram index (rtm_hist_kernel): the backward builds the whole index on its side stream without global atomics and
// the forward carries none.  PS_RTM_HIST=0: the round-2 form (ranks by global atomics in the forward's gather).
bool rtm_hist_index(const PsRtmDesc& D, const RtmWs& r) {
  static const bool on = ps_env_int("PS_RTM_HIST", 1) != 0;
  static const bool late = ps_diag_int("PS_RTM_LATE_INDEX", 0) != 0;
  return on && !late && D.review_encoder != PS_RENC_PV && r.hist != 0 && D.vocab_size <= RTM_HIST_MAXV && r.S == D.R + 1 &&
         ps_cdiv((int64_t)r.Bseq * D.R, RTM_HIST_G) <= (1 << 20);
}
int rtm_build_index_hist(const RtmK& k, int V, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    const int lim = RTM_HIST_MAXV * (int)sizeof(int);
    PS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rtm_hist_kernel<0, 1024, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, lim));
    PS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rtm_hist_kernel<0, 64, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, lim));
    PS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(rtm_hist_kernel<1, 1024, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, lim));
    attr = true;
  }
  PS_CHECK_HIP(hipMemsetAsync(k.wcnt + V, 0, sizeof(int), st));       // the allocator's running total
  if (k.det) hipLaunchKernelGGL((rtm_hist_kernel<0, 64, 1>), dim3(RTM_HIST_G), dim3(64), (size_t)V * sizeof(int), st, k);
  else hipLaunchKernelGGL((rtm_hist_kernel<0, 1024, 0>), dim3(RTM_HIST_G), dim3(1024), (size_t)V * sizeof(int), st, k);
  PS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rtm_hist_scan_kernel, dim3(ps_cdiv(V, 64)), dim3(512), 0, st, k.hist, k.wcnt, k.woff, k.wcnt + V, V);
  PS_LAUNCH_CHECK();
  hipLaunchKernelGGL((rtm_hist_kernel<1, 1024, 0>), dim3(RTM_HIST_G), dim3(1024), (size_t)V * sizeof(int), st, k);
  PS_LAUNCH_CHECK();
  return PS_OK;
}
// count (unless a kernel that reads the words anyway did), allocate, fill
int rtm_build_index(const RtmK& k, const RtmWs& r, int V, bool count, hipStream_t st) {
  static const int env_chunk = ps_diag_int("PS_RTM_IDX_CHUNK", 64);
  const int nslots = r.Bseq * r.S;
  const int chunk = env_chunk < 1 ? 1 : (env_chunk > WI_CHUNK_MAX ? WI_CHUNK_MAX : env_chunk), nwg = ps_cdiv(nslots, chunk);
  const FDiv fWL = make_fdiv(k.WL > 0 ? k.WL : 1);
  if (count) {
    hipLaunchKernelGGL(rtm_windex_kernel<0>, dim3(nwg), dim3(256), 0, st, k, chunk, fWL);
    PS_LAUNCH_CHECK();
  }
  // the allocator's running total starts at 0 on EVERY build: a second backward over the same forward (retain_graph) must
  // lay the list out from the start again, not behind the first one (the counts themselves are the forward's and stay)
  if (!count) PS_CHECK_HIP(hipMemsetAsync(k.wcnt + V, 0, sizeof(int), st));
  hipLaunchKernelGGL(rtm_walloc_kernel, dim3(ps_cdiv(V, 256)), dim3(256), 0, st, k.wcnt, k.woff, k.wcur, k.wcnt + V, V);
  PS_LAUNCH_CHECK();
  if (k.count_fwd) hipLaunchKernelGGL(rtm_windex_kernel<2>, dim3(nwg), dim3(256), 0, st, k, chunk, fWL);
  else hipLaunchKernelGGL(rtm_windex_kernel<1>, dim3(nwg), dim3(256), 0, st, k, chunk, fWL);
  PS_LAUNCH_CHECK();
  return PS_OK;
}

template <int NK>
static void wr_det_launch(const RtmK& k, int lw, int* heavy, int* nheavy, hipStream_t st) {
  hipLaunchKernelGGL(rtm_wreduce_det_kernel<NK>, dim3(lw), dim3(256), 0, st, k, heavy, nheavy);
  hipLaunchKernelGGL(rtm_wreduce_heavy_det_kernel<NK>, dim3(512), dim3(1024), 0, st, k, heavy, nheavy);
}
// the slot rows rtm_embed_bwd_kernel left (k.gs) summed per word through the index into g_word_emb
int rtm_word_reduce(const PsRtmDesc& D, const RtmK& k, const RtmWs& r, hipStream_t st) {
  const int d = D.d;
  const int64_t max_occ = (int64_t)r.Bseq * D.R * D.WL;
  static const int wr_cap = ps_diag_int("PS_RTM_WR_WGS", 4096);
  int64_t wr = (max_occ + 255) / 256;
  if (wr > wr_cap) wr = wr_cap;
  // (measured and dropped: the columns split over the XCDs — workgroup i takes d/8 columns of every entry, so that an XCD's
  // L2 holds 1/8 of each gathered row and serves the 56 re-reads itself: 206 us against 66, each 4-lane entry stream keeps
  // too few bytes in flight; this form reads 594 MB from the Infinity Cache at 8.9 TB/s)
  if (k.det) {
    const int V = (int)D.vocab_size;
    float* scr;
    TRY(rtm_det_scratch((size_t)V + 8, st, &scr));
    int* heavy = reinterpret_cast<int*>(scr);
    int* nheavy = heavy + V;
    PS_CHECK_HIP(hipMemsetAsync(nheavy, 0, sizeof(int), st));
    const int lw = ps_cdiv(V, 4) < 2048 ? ps_cdiv(V, 4) : 2048;
    if (d <= 128) wr_det_launch<2>(k, lw, heavy, nheavy, st);
    else if (d <= 256) wr_det_launch<4>(k, lw, heavy, nheavy, st);
    else wr_det_launch<8>(k, lw, heavy, nheavy, st);
  } else {
    // (round 5, measured and dropped: a wave OWNING words — one atomic row per word — that walks their occurrences in passes over the
    // slot space for L2 residency, and 32 lanes x 16 bytes per slot row: 57-100 and 79 us against 55.5, profiles/r05_c4_wreduce_notes.md)
    hipLaunchKernelGGL(rtm_wreduce_kernel, dim3((unsigned)wr), dim3(256), 0, st, k);
  }
  PS_LAUNCH_CHECK();
  return PS_OK;
}
