// gemm.hip — the GEMM dispatcher: every dense product of every model goes through ps_launch_gemm, which plans the launch once
// (gemm_plan: validate, then decide the kernel family, its instantiation, the grid and the flat tables — host only, no HIP call)
// and launches the plan (gemm_launch: one switch over the family).  The kernels and their instantiation switches: gemm_kernels.hip
// (the exact-fp32 MFMA and the three bf16x3 forms); the plan and what the kernels share: gemm.h.  The rules as a table: DESIGN.md,
// "which kernel a product takes"; ps_gemm_plan (include/prodsearch_hip.h) shows the plan of a described group without a device.
#include "gemm.h"
#include "side_stream.h"
#include <stdlib.h>
#include <string.h>

static bool needs_full(const GemmProblem& p) {
  return p.act != ACT_NONE || p.drop.thr != 0u || p.res.mode != RES_NONE || p.aux_out || p.out2 || p.colsum;
}

static int validate(const GemmProblem& p) {
  PS_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "gemm: empty problem %d %d %d", p.M, p.N, p.K);
  PS_REQUIRE(p.lda % 4 == 0 && p.ldb % 4 == 0, "gemm: lda/ldb must be multiples of 4 (%d,%d)", p.lda, p.ldb);
  PS_REQUIRE(((uintptr_t)p.A & 15) == 0, "gemm: A not 16-byte aligned");
  if (p.ta) PS_REQUIRE(p.M % 4 == 0, "gemm: ta needs M %% 4 == 0 (%d)", p.M);
  else PS_REQUIRE(p.K % 4 == 0, "gemm: K %% 4 != 0 (%d)", p.K);
  if (p.tb) PS_REQUIRE(p.N % 4 == 0, "gemm: tb needs N %% 4 == 0 (%d)", p.N);
  else PS_REQUIRE(p.K % 4 == 0, "gemm: K %% 4 != 0 (%d)", p.K);
  int nseg = (p.K + p.kseg - 1) / p.kseg;
  PS_REQUIRE(p.kseg > 0 && nseg <= 3, "gemm: bad segments kseg=%d K=%d", p.kseg, p.K);
  if (nseg > 1) PS_REQUIRE(p.kseg % 4 == 0, "gemm: kseg %% 4 != 0 (%d)", p.kseg);
  for (int s = 0; s < nseg; ++s)
    PS_REQUIRE(p.Bseg[s] && ((uintptr_t)p.Bseg[s] & 15) == 0, "gemm: B segment %d null/unaligned", s);
  PS_REQUIRE(p.ksplit >= 1, "gemm: ksplit");
  if (p.ksplit > 1) PS_REQUIRE((p.accumulate == 2 || (p.accumulate == 0 && p.split_stride > 0)) && !needs_full(p),
                               "gemm: split reduction needs a plain atomic epilogue (or per-split outputs)");
  return PS_OK;
}

// ---- the launch-shape knobs (diagnostic build only: ps_diag_int folds to the default in the shipped library), read once
struct GemmKnobs {
  int wgrad_pf;          // PS_WGRAD_PF: slabs in flight of the plain fp32 weight-gradient form.  Two 32-deep slabs measured on MI355X:
                         // 1 -> 2 takes the 8064x128x512 product from 24.4 to 20.5 us and 4096^3 from 104 to 112 TFLOP/s; 3 and 4 give
                         // nothing more; a 128-deep slab is a whole reduction already
  int t22, t21, t11;     // PS_GEMM_X3_T22 / T21 / T11: workgroups from which the size rule takes the 128x128 / 128x64 / 64x64 tile
  int tall;              // PS_GEMM_X3_TALL: 1 forward / dX products over >= 32768 rows take bf16x3, 2 their weight gradients too
  int flat_d;            // PS_X3_FLAT_D: flat weight-gradient groups take gemm_x3d_kernel's 128x128 tiles
  int x3d_diag, x3d_ldspad;   // PS_X3D_DIAG (timing-only variants, WRONG results) / PS_X3D_LDSPAD (dynamic LDS bytes: 96 KB total = one workgroup per CU)
  int flat_x3;           // PS_GEMM_X3_FLAT: plain flat groups take the bf16x3 forms
  int flat_shape;        // PS_X3_FLAT_SHAPE: 1: 128x64, 2: 128x128 tiles of gemm_x3_kernel for them
  int flat_xcd;          // PS_FLAT_XCD: GemmGroup::flat_xcd
  int flat_all;          // PS_WGRAD_FLAT_ALL: plain split reductions on the 3-D grid go flat
  int x3w_min_rows;      // PS_GEMM_X3W_MIN_ROWS: rows that are worth the pre-split-weight form's 128-row tile
  int kv_deep;           // PS_KV_DEEP: the listed K / V projection as one 128-deep slab
  int deep_max;          // PS_GEMM_DEEP_MAX: workgroups up to which a plain fp32 launch takes 128-deep slabs
  int repeat;            // PS_DEBUG_REPEAT: timing experiments only
  int split_xcd;         // PS_SPLIT_XCD: GemmGroup::split_xcd
};
static const GemmKnobs& gemm_knobs() {
  static const GemmKnobs k = {ps_diag_int("PS_WGRAD_PF", 2),       ps_diag_int("PS_GEMM_X3_T22", 4096), ps_diag_int("PS_GEMM_X3_T21", 384),
                              ps_diag_int("PS_GEMM_X3_T11", 512),  ps_diag_int("PS_GEMM_X3_TALL", 1),    ps_diag_int("PS_X3_FLAT_D", 0),
                              ps_diag_int("PS_X3D_DIAG", 0),       ps_diag_int("PS_X3D_LDSPAD", 0),     ps_diag_int("PS_GEMM_X3_FLAT", 1),
                              ps_diag_int("PS_X3_FLAT_SHAPE", 0),  ps_diag_int("PS_FLAT_XCD", 1),       ps_diag_int("PS_WGRAD_FLAT_ALL", 1),
                              ps_diag_int("PS_GEMM_X3W_MIN_ROWS", 4096), ps_diag_int("PS_KV_DEEP", 1),  ps_diag_int("PS_GEMM_DEEP_MAX", 64),
                              ps_diag_int("PS_DEBUG_REPEAT", 1),   ps_diag_int("PS_SPLIT_XCD", 1)};
  return k;
}

// ---- bf16x3 form: which launches take it, and with which tile
// PS_GEMM_X3: 0 = never, 1 (default) = wide products with enough tiles to fill the chip.  shape 2 = 128x128, 1 = 128x64,
// 0 = 64x64 tiles; -1 = the fp32 kernel (small / latency-bound launches, where the deep-slab forms matter more).
// Measured at the d = 256 shard step (21,504 rows): 128x64 wins on every forward / dX product (128x128: 2 workgroups per
// CU, 1.53 vs 1.41 ms per step), the weight gradients take 64x64 with the split counts wgrad.hip picks.
static int g_x3_mode = -2, g_x3_force = -1;           // -2: not read yet
extern "C" int ps_gemm_x3_config(int mode, int force_shape) {   // tests / experiments: mode 0|1, force_shape -1 (rule) | 0 | 1 | 2
  PS_REQUIRE((mode == 0 || mode == 1) && force_shape >= -1 && force_shape <= 4, "gemm x3 config %d %d", mode, force_shape);
  g_x3_mode = mode; g_x3_force = force_shape;
  return PS_OK;
}
static bool x3_on() {
  if (g_x3_mode == -2) { g_x3_mode = ps_env_int("PS_GEMM_X3", 1) ? 1 : 0; g_x3_force = ps_env_int("PS_GEMM_X3_SHAPE", -1); }
  return g_x3_mode != 0;
}
bool gemm_x3_on() { return x3_on(); }
// the pre-split-weight form is OFF unless asked for (ps_gemm_x3_config(1, 4) / PS_GEMM_X3_SHAPE=4): measured on MI355X it ties
// the 128x64 kernel on the d = 256 step's products (profiles/r04_gemm_notes.md) — kept as a tested alternative, not the default
bool gemm_x3w_on() { x3_on(); return g_x3_mode != 0 && g_x3_force == 4; }
static bool x3_rule_free() { return g_x3_force < 0 || g_x3_force == 4; }      // no tile forced: prefer_x3d counts

static int x3_shape(const GemmGroup& g, const GemmKnobs& kn, int maxM, int maxN) {
  if (!x3_on()) return -1;
  if (g_x3_force >= 0 && g_x3_force != 4) return g_x3_force > 3 ? 3 : g_x3_force;   // (4: pre-split weights where registered, the rule elsewhere)
  const int z = g.n * g.p[0].ksplit;
  int kmin = g.p[0].K;
  for (int i = 1; i < g.n; ++i) kmin = g.p[i].K < kmin ? g.p[i].K : kmin;
  // Products of a wide model (every weight dimension >= 256: the d = 256 configuration) — at d = 128 a reduction is 4 slabs
  // deep and the fp32 kernel's deep-slab forms win at C2's 8k rows (0.289 -> 0.293 ms per step with this form forced); the
  // review transformer's 78k-row launches lose with 128x64 tiles and with their weight gradients included (0.540 -> 0.550) ...
  int nmin = g.p[0].N, mmin = g.p[0].M;
  for (int i = 1; i < g.n; ++i) { nmin = g.p[i].N < nmin ? g.p[i].N : nmin; mmin = g.p[i].M < mmin ? g.p[i].M : mmin; }
  // ... and the forward / dX products over very many rows (the review transformer's 78k sequence positions), with 64x64 tiles:
  // 0.544 -> 0.534 ms per step there (its weight gradients gain nothing: PS_GEMM_X3_TALL=2 adds them)
  if (kn.tall >= 1 && !g.p[0].ta && maxM >= 32768) return 0;
  if (kn.tall >= 2 && g.p[0].ta && kmin >= 32768) return 0;
  if (kmin < 256 || nmin < 256 || kmin / g.p[0].ksplit < 256 || (g.p[0].ta && mmin < 256)) return -1;
  if ((long)ps_cdiv(maxM, 128) * ps_cdiv(maxN, 128) * z >= kn.t22) return 2;
  if ((long)ps_cdiv(maxM, 128) * ps_cdiv(maxN, 64) * z >= kn.t21) return 1;
  if ((long)ps_cdiv(maxM, 64) * ps_cdiv(maxN, 64) * z >= kn.t11) return 0;
  return -1;
}
// the (ta, tb, full, row list) combinations gemm_x3_kernel and gemm_x3d_kernel are instantiated for (launch_x3, launch_x3d): the
// others fall back to the fp32 kernel
static bool x3_has(int ta, int tb, bool full, bool listed) {
  if (!listed) return ta == 0 || (tb == 1 && !full);
  return (ta == 0 && tb == 1 && full) || (ta == 1 && tb == 1 && !full) || (ta == 0 && tb == 0 && !full);
}
// the direct-to-LDS form (gemm_x3d_kernel) takes single-segment operands and whole 32-deep slabs (a listed weight gradient pads
// its reduction list itself)
static bool x3d_takes(const GemmGroup& g) {
  for (int i = 0; i < g.n; ++i) {
    const GemmProblem& p = g.p[i];
    if (p.K > p.kseg) return false;
    if (p.K % X3D_BK != 0 && !(p.ridx && p.ta)) return false;
    if (((uintptr_t)p.Bseg[0] & 15) || ((uintptr_t)p.A & 15)) return false;
  }
  return true;
}
// the shapes gemm_x3w_kernel takes (its B planes: wplanes_find)
static bool x3w_takes(const GemmProblem& p) {
  return !(p.ta || p.K % X3D_BK || p.kseg % X3D_BK || ((uintptr_t)p.A & 15) || p.lda % 4);
}

static void plan_tile(GemmPlan* pl, int family, int tm, int tn, int maxM, int maxN, int z) {
  pl->family = family; pl->tile_m = tm; pl->tile_n = tn; pl->bk = 32; pl->pf = 1;
  pl->grid = dim3(ps_cdiv(maxN, tn), ps_cdiv(maxM, tm), z);
}
// false: not taken (the next form is tried).  No grid.y test here or in plan_x3: gemm_plan has required ceil(maxM / 64) <= 65535
// of every 3-D launch, and these tiles are at least 64 rows tall
static bool plan_x3d(const GemmGroup& g, const GemmKnobs& kn, bool full, bool listed, int maxM, int maxN, int z, GemmPlan* pl) {
  if (!x3d_takes(g)) return false;
  const bool diag = !listed && pl->ta == 0 && pl->tb == 0 && !full && (kn.x3d_diag || kn.x3d_ldspad);
  if (!diag && !x3_has(pl->ta, pl->tb, full, listed)) return false;
  plan_tile(pl, GEMM_X3D, X3D_T, X3D_T, maxM, maxN, z);
  if (diag) { pl->diag = kn.x3d_diag >= 1 && kn.x3d_diag <= 3 ? kn.x3d_diag : 0; pl->lds_bytes = kn.x3d_ldspad; }
  return true;
}
static bool plan_x3(const GemmGroup& g, const GemmKnobs& kn, int shape, bool full, bool listed, int maxM, int maxN, int z, GemmPlan* pl) {
  if (shape == 3) {
    if (plan_x3d(g, kn, full, listed, maxM, maxN, z, pl)) return true;
    shape = 1;                                                   // what the rule picked before this form existed
  }
  if (!x3_has(pl->ta, pl->tb, full, listed)) return false;
  plan_tile(pl, GEMM_X3, shape >= 1 ? 128 : 64, shape == 2 ? 128 : 64, maxM, maxN, z);
  return true;
}

// The whole decision of one launch.  `planes`: -1 look the members' weights up in the registry (WPlaneScope), 0 / 1 take it as
// given that they are not / are all registered (ps_gemm_plan: a description has no weights)
static int gemm_plan(const GemmGroup& g, GemmPlan* pl, int planes = -1) {
  memset(pl, 0, sizeof(*pl));
  PS_REQUIRE(g.n >= 1 && g.n <= 4, "gemm: group size %d", g.n);
  const GemmKnobs& kn = gemm_knobs();
  // ---- every member once: what any launch needs, then what the grid the caller chose needs
  int maxM = 0, maxN = 0;
  bool full = false, listed = false;
  for (int i = 0; i < g.n; ++i) {
    const GemmProblem& p = g.p[i];
    TRY(validate(p));
    if (g.flat) {
      PS_REQUIRE(p.ta == 1 && p.tb == 1 && !needs_full(p) && p.ksplit >= 1 &&
                 (p.accumulate == 2 || (p.accumulate == 0 && p.split_stride > 0)),
                 "gemm: the flat group form takes weight-gradient problems");
      if (p.ridx) {
        const int per = ps_cdiv(ps_cdiv(p.K, 32), p.ksplit);
        PS_REQUIRE(p.rcount && p.kseg >= p.K && !p.bias && per * 32 <= KIDX_MAX,
                   "gemm: flat row-list weight gradient: one segment, no bias, %d rows per split <= %d", per * 32, KIDX_MAX);
      }
    } else {
      PS_REQUIRE(p.ta == g.p[0].ta && p.tb == g.p[0].tb && p.ksplit == g.p[0].ksplit,
                 "gemm: group members must share layout and ksplit");
    }
    maxM = p.M > maxM ? p.M : maxM;
    maxN = p.N > maxN ? p.N : maxN;
    full = full || needs_full(p);
    listed = listed || p.ridx;
  }
  const int ta = g.p[0].ta, tb = g.p[0].tb, ks = g.p[0].ksplit, z = g.n * ks;
  pl->ta = ta; pl->tb = tb; pl->full = full; pl->idx = listed; pl->repeat = 1;
  pl->flat = g.flat ? 1 : 0;
  bool prefer_d = g.prefer_x3d != 0;
  if (!g.flat) {
    PS_REQUIRE(ps_cdiv(maxM, BM) <= 65535 && z <= 65535, "gemm: grid too large");
    for (int i = 0; i < g.n; ++i) {
      const GemmProblem& p = g.p[i];
      if (!p.ridx) continue;
      PS_REQUIRE(p.rcount && p.drop.thr == 0u && !p.colsum && !p.aux_out && p.kseg >= p.K * (p.ta ? 1 : 0),
                 "gemm: row-list problems take no dropout / column sums / pre-activation output");
      if (p.ta) {
        const int per = ps_cdiv(ps_cdiv(p.K, 32), p.ksplit);
        PS_REQUIRE(p.tb == 1 && per * 32 <= KIDX_MAX, "gemm: row-list weight gradient: %d rows per split > %d", per * 32, KIDX_MAX);
      }
    }
    // Plain split reductions (weight gradients) whose form is a bf16x3 kernel that also has a FLAT (1-D grid) launch go through it: the
    // flat decode puts all tiles of a reduction split on one XCD (GemmGroup::flat_xcd), where the 3-D grid spreads them over all
    // eight — the C5 shard's W2 / W1 gradients fetched 2 x 129 = 258 MB per launch for 110 MB of operands, its Wo gradient 2 x 68 = 135
    // MB for 44 (PMC, profiles/r04_c5_pmc_traffic.txt).  Such a group meets everything the flat form requires of its members.
    bool plain = kn.flat_all && !listed && !full && ta == 1 && tb == 1 && ks >= 8 && ks % 8 == 0 && x3_on();
    for (int i = 0; i < g.n && plain; ++i)
      plain = g.p[i].accumulate == 2 || (g.p[i].accumulate == 0 && g.p[i].split_stride > 0);
    if (plain) {
      const bool d = prefer_d && x3_rule_free() && x3d_takes(g);
      if (d || x3_shape(g, kn, maxM, maxN) == 0) { pl->flat = 1; pl->redirected = 1; prefer_d = d; }
    }
  }

  if (pl->flat) {
    // the bf16x3 forms (the same flat tables): C2's W2 / W1 / Wo weight gradients 0.2905 -> 0.2845 ms per step with 64x64 tiles
    // (round 2); 128x128 tiles of the direct-to-LDS form where the caller sized the splits for them (prefer_x3d) or shape 3 is
    // forced.  Groups with listed members: the fp32 kernel
    const bool x3 = kn.flat_x3 && x3_on() && !listed;
    const bool x3d = x3 && (g_x3_force == 3 || kn.flat_d != 0 || prefer_d) && x3d_takes(g);
    const int fs = (x3 && !x3d) ? kn.flat_shape : 0;
    const int TM = x3d ? X3D_T : (fs >= 1 ? 128 : BM), TN = x3d ? X3D_T : (fs == 2 ? 128 : BM);
    int total = 0;
    for (int i = 0; i < 4; ++i) {
      pl->flat0[i] = total;
      if (i >= g.n) { pl->flat_tm[i] = 1; pl->flat_tiles[i] = 1; continue; }
      pl->flat_tm[i] = ps_cdiv(g.p[i].M, TM);
      pl->flat_tiles[i] = pl->flat_tm[i] * ps_cdiv(g.p[i].N, TN);
      total += pl->flat_tiles[i] * g.p[i].ksplit;
    }
    pl->flat0[4] = total;
    for (int i = g.n; i < 4; ++i) pl->flat0[i] = total + 1;      // never selected
    for (int i = 0; i < g.n && kn.flat_xcd; ++i)
      if (g.p[i].ksplit % 8 == 0 && pl->flat0[i] % 8 == 0) pl->flat_xcd |= 1 << i;
    if (!listed && pl->flat_xcd != (1 << g.n) - 1) pl->flat_xcd = 0;
    pl->family = x3d ? GEMM_X3D : (x3 ? GEMM_X3 : GEMM_F32);
    pl->tile_m = TM; pl->tile_n = TN; pl->bk = 32;
    // listed groups: their workgroups run 2-3 slabs at the list lengths the step produces, so ALL of a short reduction's operand
    // slabs are requested before the first is consumed (PF = 3; longer lists refill the slots as any PF does)
    pl->pf = listed ? 3 : (x3 ? 1 : (kn.wgrad_pf == 3 || kn.wgrad_pf == 4 ? kn.wgrad_pf : 2));
    pl->timed = listed || x3;
    pl->grid = dim3(total, 1, 1);
    return PS_OK;
  }

  pl->split_xcd = kn.split_xcd && ta == 1 && ks >= 8 && ks % 8 == 0;   // splits placed by XCD when their count allows
  // products against pre-split weights (WPlaneScope): every member's B found, enough rows to be worth a 128-row tile
  if (gemm_x3w_on() && !ta && ks == 1 && maxM >= kn.x3w_min_rows) {
    bool all = planes != 0;
    for (int i = 0; i < g.n && all; ++i) all = x3w_takes(g.p[i]) && (planes > 0 || wplanes_find(g.p[i], pl->bpl[i]));
    if (all) {
      for (int i = 0; i < g.n; ++i)      // one segment: its planes are [3][N][K]
        pl->kseg[i] = ps_cdiv(g.p[i].K, g.p[i].kseg) == 1 ? g.p[i].K : g.p[i].kseg;
      plan_tile(pl, GEMM_X3W, X3D_T, X3D_T, maxM, maxN, g.n);
      return PS_OK;
    }
  }
  if (prefer_d && x3_on() && x3_rule_free() && plan_x3d(g, kn, full, listed, maxM, maxN, z, pl)) return PS_OK;
  const int x3 = x3_shape(g, kn, maxM, maxN);
  if (x3 >= 0 && plan_x3(g, kn, x3, full, listed, maxM, maxN, z, pl)) return PS_OK;

  plan_tile(pl, GEMM_F32, BM, BN, maxM, maxN, z);
  const size_t wgs = (size_t)pl->grid.x * pl->grid.y * pl->grid.z;
  if (listed) {   // row-list instantiations exist for the three shapes of the step that use them (32-deep slabs)
    // (the K/V dX product as 128-deep slabs measured slower, 0.363 vs 0.355 ms/step: its 133 KB of LDS per workgroup
    // crowds out the weight gradients running beside it)
    PS_REQUIRE((ta == 0 && tb == 1 && full) || (ta == 1 && tb == 1 && !full) || (ta == 0 && tb == 0 && !full),
               "gemm: no row-list instantiation for ta=%d tb=%d full=%d", ta, tb, (int)full);
    // small launches whose whole reduction is one 128-deep slab (the K/V projection at C2: ~240 live workgroups):
    // one global round trip instead of four shallow slabs (0.3615 -> 0.3564 ms/step); big grids keep 4 workgroups per CU
    const bool deep = ta == 0 && tb == 0 && kn.kv_deep && g.p[0].K <= 128 && wgs <= 1024;
    pl->bk = deep ? 128 : 32; pl->pf = deep ? 1 : 2;
    return PS_OK;
  }
  // few workgroups (latency-bound chain): one deep slab per round trip; many: shallow slabs, 4 wgs per CU
  const bool deep = wgs <= (size_t)kn.deep_max && !g.p[0].no_deep;
  pl->bk = deep ? 128 : 32;
  pl->pf = deep ? 1 : ((kn.wgrad_pf == 3 || kn.wgrad_pf == 4) && !full && ta == 1 && tb == 1 ? kn.wgrad_pf : 2);
  pl->repeat = kn.repeat;
  return PS_OK;
}

// the plan's values into the kernel argument, then the family's switch
static int gemm_launch(const GemmPlan& pl, GemmGroup& g, hipStream_t stream) {
  g.flat = pl.flat;
  g.split_xcd = pl.split_xcd;
  if (pl.flat) {
    memcpy(g.flat0, pl.flat0, sizeof(g.flat0));
    memcpy(g.flat_tm, pl.flat_tm, sizeof(g.flat_tm));
    memcpy(g.flat_tiles, pl.flat_tiles, sizeof(g.flat_tiles));
    g.flat_xcd = pl.flat_xcd;
  }
  switch (pl.family) {
    case GEMM_X3W:
      for (int i = 0; i < g.n; ++i) { memcpy(g.p[i].bpl, pl.bpl[i], sizeof(g.p[i].bpl)); g.p[i].kseg = pl.kseg[i]; }
      launch_x3w(pl, g, stream);
      break;
    case GEMM_X3D: launch_x3d(pl, g, stream); break;
    case GEMM_X3: launch_x3(pl, g, stream); break;
    default:
      for (int r = 0; r < pl.repeat; ++r) launch_f32(pl, g, stream);
  }
  PS_LAUNCH_CHECK();
  return PS_OK;
}

int ps_launch_gemm(const GemmGroup& g0, hipStream_t stream) {
  GemmGroup g = g0;
  g.sig = nullptr; g.sigval = 0;
  static const int stamps = ps_diag_int("PS_GEMM_STAMP", 0);
  const bool stamp_this = stamps == 1 || (stamps == 2 && g0.p[0].ridx && g0.p[0].res.mode == RES_FANIN) ||
                          (stamps == 3 && g0.p[0].ridx && !g0.p[0].ta && g0.p[0].res.mode == RES_NONE) ||
                          (stamps == 4 && g0.n == 3 && g0.p[0].ta && !g0.p[0].ridx) ||    // 4: the grouped FF / Wo weight gradients
                          (stamps == 5 && g0.n == 4 && g0.p[0].ta && g0.p[0].ridx);       // 5: the deferred K / V / Q / f_W weight gradients
  g.stamp = stamp_this ? ps_debug_stamp_ptr() : nullptr;
  g.stamp_kvq = stamps == 5;
  const bool took = side_take_signal(stream, &g.sig, &g.sigval);      // a pending fork of the side stream rides on this launch
  GemmPlan pl;
  int rc = gemm_plan(g, &pl);
  if (rc == PS_OK) rc = gemm_launch(pl, g, stream);
  if (took && rc != PS_OK) side_repend_signal(stream, g.sigval);
  return rc;
}

// ---- the plan of a described group (include/prodsearch_hip.h): host only
extern "C" int ps_gemm_plan(int32_t n, const PsGemmMember* m, int32_t flat, int32_t prefer_x3d, int32_t planes, PsGemmPlan* out) {
  PS_REQUIRE(m && out && n >= 0 && n <= 8, "ps_gemm_plan: null argument or more than 8 members");
  alignas(16) static char dummy[16];                 // every address of the group: non-null, 16-byte aligned, never dereferenced
  GemmGroup g;
  memset(&g, 0, sizeof(g));
  g.n = n; g.flat = flat; g.prefer_x3d = prefer_x3d;
  for (int i = 0; i < n && i < 4; ++i) {
    GemmProblem& p = g.p[i];
    const PsGemmMember& d = m[i];
    p.M = d.M; p.N = d.N; p.K = d.K; p.ksplit = d.ksplit; p.ta = d.ta; p.tb = d.tb;
    p.kseg = d.kseg > 0 ? d.kseg : d.K;
    p.A = (const float*)dummy; p.C = (float*)dummy;
    p.Bseg[0] = p.Bseg[1] = p.Bseg[2] = (const float*)dummy;
    p.lda = ((d.ta ? d.M : d.K) + 3) / 4 * 4; p.ldb = ((d.tb ? d.N : p.kseg) + 3) / 4 * 4; p.ldc = d.N;
    p.alpha = 1.f;
    if (d.full == 1) p.act = ACT_GELU;
    if (d.full == 2) { p.drop.thr = 1u << 31; p.drop.scale = 2.f; }
    if (d.listed) { p.ridx = (const int32_t*)dummy; p.rcount = (const int32_t*)dummy; }
    p.accumulate = d.accumulate; p.split_stride = d.split_stride; p.no_deep = d.no_deep;
  }
  GemmPlan pl;
  TRY(gemm_plan(g, &pl, planes ? 1 : 0));
  *out = PsGemmPlan{pl.family, pl.ta, pl.tb, pl.full, pl.idx, pl.bk, pl.pf, pl.tile_m, pl.tile_n, pl.flat, pl.redirected,
                    (int32_t)pl.grid.x, (int32_t)pl.grid.y, (int32_t)pl.grid.z, pl.lds_bytes, pl.flat_xcd, pl.split_xcd};
  return PS_OK;
}

static int gemm_f32_impl(const float* A, int lda, int ta, const float* Bm, int ldb, int tb, float* Cm, int ldc,
                         int M, int N, int K, const float* bias, float alpha, int accumulate, ps_stream_t stream);
extern "C" int ps_gemm_f32(const float* A, int lda, int ta, const float* Bm, int ldb, int tb, float* Cm, int ldc,
                           int M, int N, int K, const float* bias, float alpha, int accumulate,
                           ps_stream_t stream) {
  return gemm_f32_impl(A, lda, ta, Bm, ldb, tb, Cm, ldc, M, N, K, bias, alpha, accumulate, stream);
}
// the same product with B declared a WEIGHT ([N][K] for tb == 0, [K][N] for tb == 1, dense rows): split once into bf16 planes
// for the duration of the call (WPlaneScope), multiplied by gemm_x3w_kernel where that kernel applies — the path the
// training step's forward and dX products of a d >= 256 model take; tests and tools/gemm_x3_bench.py
extern "C" int ps_gemm_f32_weight(const float* A, int lda, const float* W, int tb, float* Cm, int ldc, int M, int N, int K,
                                  const float* bias, float alpha, ps_stream_t stream) {
  const float* ws[1] = {W};
  const int rows[1] = {tb ? K : N}, cols[1] = {tb ? N : K};
  WPlaneScope scope((hipStream_t)stream, ws, rows, cols, 1);
  return gemm_f32_impl(A, lda, 0, W, tb ? N : K, tb, Cm, ldc, M, N, K, bias, alpha, 0, stream);
}
static int gemm_f32_impl(const float* A, int lda, int ta, const float* Bm, int ldb, int tb, float* Cm, int ldc,
                         int M, int N, int K, const float* bias, float alpha, int accumulate, ps_stream_t stream) {
  GemmGroup g = {};
  g.n = 1;
  GemmProblem& p = g.p[0];
  p.A = A; p.lda = lda; p.ta = ta;
  p.Bseg[0] = Bm; p.kseg = K; p.ldb = ldb; p.tb = tb;
  p.C = Cm; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  p.bias = bias; p.alpha = alpha; p.act = ACT_NONE;
  p.accumulate = accumulate == 2 ? 2 : accumulate;
  static const int ks = ps_diag_int("PS_GEMM_KSPLIT", 4);   // timing experiments
  p.ksplit = accumulate == 2 ? ks : 1;
  return ps_launch_gemm(g, (hipStream_t)stream);
}
