"""Which encoder path (csrc/encoder.h: EncPlan) each oracle-compared item-transformer case takes: one table, written by hand,
shared by the plan test that needs no GPU (test_enc_plan_cpu.py: ps_tem_plan equals the table) and the GPU tests, which assert
what the step really launched (ps_enc_path_taken) against the same rows.

The expected values are NOT generated from enc_plan.  They follow the limits the kernels document (csrc/rowwise.h,
csrc/attn_sq1.hip, csrc/mlp_fused.hip):
  * sq1 forms: one query row (the last layer), S = L + 1 <= 64, K / V of one sequence within the 128 KB LDS limit (about 3 S d floats: d = 256
    reaches it between S = 25 and S = 64, d = 512 from S = 20) — otherwise the generic form;
  * wf (a wave per sequence and four heads, replicas inside): 8 heads, 4..24 replicas, d = 128 with S <= 32 or d = 256 with
    S <= 24; kvq (projections + wf attention in one launch): wf at d = 128, one layer, the row list, query position 0;
  * w1 (a wave per sequence): no replicas, d = 64 / 128;
  * every fused form (last layer forward FF, folded scoring FS, fused backward BF, folded dQ.Wq QF at replicas, fused dX DX) is
    d = 128 only; FF needs F in {256, 512, 1024}; BF needs PS_FUSE_BWD_MIN (1024) replica rows; the K / V / Q weight gradients
    stay on the main stream (M, and deferred behind the scatter: ML) while the K / V rows are at most twice the replica rows;
  * the row list (RL; backward LI) is a one-layer, query-position-0, sq1-form matter; PR (the replicas' fan-in summed by its own
    launch) is LI with replicas where dQ.Wq is not folded.
One rule above is written down nowhere but beside enc_plan itself (csrc/encoder.h, EncPlan::Bwd::wg3_main): the "at most twice
the replica rows" bound of M / ML.  The PARTIAL_TILE_ROWS follow it — a choice of stream, not of kernel — and are the only rows
whose expectation rests on the code under test.
A row that disagrees with enc_plan is a finding about enc_plan or about one of the *_fits predicates, not a reason to edit it."""
import ctypes as C
import os

GEN, SQ1, W1, WF, KVQ = 0, 1, 2, 3, 4
FORM_NAMES = ('GEN', 'SQ1', 'W1', 'WF', 'KVQ')

# flag letter -> PsEncPath field
FLAGS = {'RL': 'rowlist', 'FF': 'fwd_fuse_last', 'FS': 'fold_score', 'BF': 'bwd_fuse_last', 'IS': 'item_scatter',
         'M': 'wg3_main', 'ML': 'wg3_last', 'QF': 'q_folded', 'LI': 'listed', 'PR': 'presum', 'DX': 'dx_fused'}
FWD_FIELDS = ('rowlist', 'fwd_fuse_last', 'fold_score')
BWD_FIELDS = ('bwd_fuse_last', 'item_scatter', 'wg3_main', 'wg3_last', 'q_folded', 'listed', 'presum', 'dx_fused')
PS_FUSE_BWD_MIN = 1024

FUSED_D128 = 'RL FF FS QF LI DX'            # one layer at d = 128 with 4..24 replicas and S <= 32
C2_FLAGS = 'RL FF FS BF IS M ML QF LI DX'   # ... from 1,024 replica rows upwards


def row(name, B, K, L, d, attn, flags, H=8, F=None, Q=4, W=1, dropout=0.1, zero_hist=0.2, layers=1, fuse_bwd_min=None,
        Pn=700, V=900, **over):
    """``over``: default_args overrides beyond the shape (query_encoder_name, use_item_pos).  ``fuse_bwd_min``: the value of
    ps_set_fuse_bwd_min the case runs under (None: the process default, 1024)."""
    flags = flags.split()
    assert all(f in FLAGS for f in flags), flags
    return dict(name=name, B=B, K=K, L=L, Q=Q, W=W, d=d, H=H, F=2 * d if F is None else F, dropout=dropout,
                zero_hist=zero_hist, layers=layers, attn=tuple(attn), flags=frozenset(flags), fuse_bwd_min=fuse_bwd_min,
                Pn=Pn, V=V, over=over)


# ---- cases the suite had before this table (tests/test_gpu_shapes.py, tests/test_gpu_tem_options.py), annotated
EDGE_ROWS = [      # test_edge_shapes_match_oracle, in its parameter order
    row('e_1_1_1', 1, 1, 1, 32, [SQ1], 'RL LI', H=1, Q=1, zero_hist=0.0, dropout=0.0),
    row('e_3_2_20', 3, 2, 20, 32, [SQ1], 'RL LI', H=4, Q=8, zero_hist=1.0, dropout=0.0),
    row('e_5_33_7', 5, 33, 7, 64, [W1], 'RL QF LI', Q=3, W=2, zero_hist=0.3, dropout=0.0),
    row('e_130_3_12', 130, 3, 12, 96, [SQ1], 'RL LI PR', Q=5, zero_hist=0.1),
    row('e_2_5_20', 2, 5, 20, 128, [KVQ], FUSED_D128, Q=8, W=3, zero_hist=0.0),
    row('e_50_20_9', 50, 20, 9, 128, [KVQ], C2_FLAGS),
    row('e_400_20_9', 400, 20, 9, 128, [KVQ], C2_FLAGS),
    row('e_6_23_29', 6, 23, 29, 128, [KVQ], FUSED_D128),                          # S = 30, 24 replicas
    row('e_9_3_31', 9, 3, 31, 128, [KVQ], FUSED_D128, zero_hist=0.1),             # S = 32, 4 replicas
    row('e_7_2_12', 7, 2, 12, 128, [SQ1], 'RL FF FS QF LI', zero_hist=0.1),       # 3 replicas: below the wf form
    row('e_6_4_40', 6, 4, 40, 128, [SQ1], 'RL FF FS QF LI', zero_hist=0.1),       # S = 41: above it
    row('e_6_4_40_nodrop', 6, 4, 40, 128, [W1], 'RL FF QF LI', zero_hist=0.1, dropout=0.0),
    row('e_6_4_40_d64', 6, 4, 40, 64, [W1], 'RL QF LI', H=4, zero_hist=0.1, dropout=0.0),
]
WIDE_ROWS = {      # test_wide_embeddings_match_oracle (d, B, K, dropout) -> row; its two large cases are not annotated
    (256, 24, 6, 0.0): row('w_d256_nodrop', 24, 6, 20, 256, [SQ1], 'RL LI', F=1024, Q=8, dropout=0.0, Pn=3000, V=2000),
    (256, 16, 5, 0.1): row('w_d256', 16, 5, 20, 256, [WF], 'RL LI PR', F=1024, Q=8, Pn=3000, V=2000),
    (512, 9, 4, 0.0): row('w_d512_nodrop', 9, 4, 20, 512, [GEN], '', F=1024, Q=8, dropout=0.0, Pn=3000, V=2000),
}
OPTION_ROWS = {    # test_option_matches_oracle
    # the consumed position is S - 1: no row list (so no kvq form, no listed consumers, no fused dX)
    'item_pos': row('o_item_pos', 50, 20, 9, 128, [WF], 'FF FS BF IS M ML QF', F=256, use_item_pos=True),
    # the AVG encoder's backward copies one row of d x: the fused dX form is the FS encoder's
    'avg': row('o_avg', 50, 20, 9, 128, [KVQ], 'RL FF FS BF IS M ML QF LI', F=256, query_encoder_name='avg'),
    # layer 0 attends from every position (generic), the last layer has B * R sequences without replicas of their own (w1);
    # K / V rows = B * R * S = 10 x the replica rows: the K / V / Q weight gradients go to the side stream (no M)
    'two_layers': row('o_two_layers', 50, 20, 9, 128, [GEN, W1], 'FF FS BF IS', F=256, layers=2),
}
# test_fused_backward_partial_tiles: ps_set_fuse_bwd_min(1) on three tiny batches at d = 128.  The fused backward and its item
# scatter are taken; M / ML are not: these batches have more K / V rows than twice their replica rows (147 vs 70, 42 vs 24,
# 198 vs 132 — the rule above, `n_in * S <= 2 * M2` in enc_plan), unlike e_50_20_9 (500 vs 2,100).
PARTIAL_TILE_ROWS = {
    (7, 4, 20): row('p_7_4_20', 7, 4, 20, 128, [KVQ], FUSED_D128 + ' BF IS', Q=8, zero_hist=0.0, fuse_bwd_min=1),
    (2, 5, 20): row('p_2_5_20', 2, 5, 20, 128, [KVQ], FUSED_D128 + ' BF IS', Q=8, W=3, zero_hist=0.0, fuse_bwd_min=1),
    (33, 1, 5): row('p_33_1_5', 33, 1, 5, 128, [SQ1], 'RL FF FS QF LI BF IS', Q=3, zero_hist=0.5, fuse_bwd_min=1),   # 2 replicas
}

# ---- cells of the plan no earlier case reached (tests/test_gpu_enc_paths.py)
NEW_ROWS = [
    row('f128', 6, 4, 20, 128, [WF], 'RL QF LI', F=128),                     # F outside {256, 512, 1024}: nothing fused, no kvq
    row('h4', 6, 4, 20, 128, [SQ1], 'RL FF FS LI PR', H=4),                  # 4 heads: one head group, dQ.Wq not folded
    row('h16', 6, 4, 20, 128, [SQ1], 'RL FF FS QF LI', H=16),                # dh = 8
    row('h16_nodrop', 6, 4, 20, 128, [SQ1], 'RL FF LI', H=16, dropout=0.0),  # ... above the w1 form's 8 heads
    row('fan25', 6, 24, 9, 128, [SQ1], 'RL FF FS QF LI'),                    # 25 replicas: one past the wf form
    row('s2', 6, 4, 1, 128, [KVQ], FUSED_D128),
    row('s24', 6, 4, 23, 128, [KVQ], FUSED_D128),                            # the <16,6> | <16,8> instances of the wf kernels
    row('s25', 6, 4, 24, 128, [KVQ], FUSED_D128),
    row('s33', 6, 4, 32, 128, [SQ1], 'RL FF FS QF LI'),                      # one past the wf form's 32 positions
    row('s64', 6, 4, 63, 128, [SQ1], 'RL FF FS QF LI'),                      # the largest legal S
    row('s64_nodrop', 6, 4, 63, 128, [W1], 'RL FF QF LI', dropout=0.0),
    row('d64_drop', 6, 4, 20, 64, [SQ1], 'RL LI PR', F=128),
    row('d256_s24', 6, 4, 23, 256, [WF], 'RL LI PR', F=1024),
    row('d256_s25', 6, 4, 24, 256, [SQ1], 'RL LI PR', F=1024),
    row('d256_fan3', 6, 2, 20, 256, [SQ1], 'RL LI PR', F=1024),
    row('d256_s64', 6, 4, 63, 256, [GEN], '', F=1024),                       # K / V of 64 positions at d = 256 exceed the LDS limit
    row('d512_drop', 6, 4, 20, 512, [GEN], '', F=1024),
    row('l3', 6, 4, 9, 128, [GEN, GEN, W1], 'FF FS', layers=3),              # a middle layer: n_in = B * R, Sq = S, its own pre-LN
    row('l2_d256', 6, 4, 9, 256, [GEN, SQ1], '', F=1024, layers=2),
    row('l2_d512', 6, 4, 20, 512, [GEN, GEN], '', F=1024, layers=2),         # the generic form as the last of several layers (S = 21, as d512_drop)
    row('mf1008', 48, 20, 9, 128, [KVQ], FUSED_D128, fuse_bwd_min=PS_FUSE_BWD_MIN),
    row('mf1029', 49, 20, 9, 128, [KVQ], C2_FLAGS, fuse_bwd_min=PS_FUSE_BWD_MIN),
    # ---- tests/tem_table_rows.py's shapes that no row above has
    row('avg_d96', 50, 20, 9, 96, [SQ1], 'RL LI PR', F=192, query_encoder_name='avg'),        # d = 96: nothing fused, no wf
    row('avg_d64_nodrop', 6, 4, 20, 64, [W1], 'RL QF LI', H=4, F=128, dropout=0.0, query_encoder_name='avg'),
    row('heavy_nodrop', 50, 20, 9, 128, [W1], 'RL FF QF LI', dropout=0.0),                    # e_50_20_9 without replicas
]
for _q in (33, 64, 65, 70):      # queries of up to Q words at 30 replica rows: the plan does not read Q
    NEW_ROWS.append(row('q%d_fs' % _q, 6, 4, 9, 128, [KVQ], FUSED_D128, Q=_q))
    NEW_ROWS.append(row('q%d_avg' % _q, 6, 4, 9, 128, [KVQ], 'RL FF FS QF LI', Q=_q, query_encoder_name='avg'))

ALL_ROWS = EDGE_ROWS + list(WIDE_ROWS.values()) + list(OPTION_ROWS.values()) + list(PARTIAL_TILE_ROWS.values()) + NEW_ROWS
assert len({r['name'] for r in ALL_ROWS}) == len(ALL_ROWS)


# The switches and setters' environment forms the plan reads.  The table holds the DEFAULT plan; a run of these files under one of
# them (tools/env_matrix.sh) keeps its oracle comparisons and leaves the path assertions to test_enc_plan_cpu.py, which pins every
# supported switch's effect on the plan.
PLAN_SWITCHES = ('PS_NO_FUSE', 'PS_NO_FUSE_BWD', 'PS_NO_ROWLIST', 'PS_NO_FOLD_SCORE', 'PS_KVQ_FUSED', 'PS_KVDX_FUSED', 'PS_ATTN_WF',
                 'PS_ATTN_W1', 'PS_ATTN_WK', 'PS_DETERMINISTIC', 'PS_FUSE_BWD_MIN', 'PS_ITEM_SCATTER_FUSED', 'PS_GRAPHS',
                 'PS_DIAG_LIB')


def default_switches():
    return not any(k in os.environ for k in PLAN_SWITCHES)


def model_kwargs(r):
    """default_args overrides of a row (the module API's arguments)."""
    kw = dict(model_name='item_transformer', embedding_size=r['d'], heads=r['H'], ff_size=r['F'], inter_layers=r['layers'],
              neg_per_pos=r['K'], dropout=r['dropout'], uprev_review_limit=r['L'], pv_window_size=r['W'])
    kw.update(r['over'])
    return kw


def oracle_call(r):
    """Arguments of test_gpu_tem_options.check_against_oracle for a row."""
    kw = model_kwargs(r)
    for k in ('model_name', 'neg_per_pos', 'uprev_review_limit', 'pv_window_size'):
        kw.pop(k)
    return dict(B=r['B'], K=r['K'], L=r['L'], Q=r['Q'], W=r['W'], zero_hist=r['zero_hist'], P_=r['Pn'], V=r['V'], **kw)


def desc_of(r, _lib):
    """The training-step descriptor ItemTransformerRanker._plan_for builds for a row's batch."""
    d = _lib.PsTemDesc()
    d.B, d.K, d.L, d.Q, d.W, d.C = r['B'], r['K'], r['L'], r['Q'], r['W'], 0
    d.d, d.H, d.F, d.n_layers = r['d'], r['H'], r['F'], r['layers']
    d.product_size, d.vocab_size = r['Pn'], r['V']
    d.model = _lib.PS_MODEL_TEM
    d.query_encoder = _lib.PS_QENC_AVG if r['over'].get('query_encoder_name') == 'avg' else _lib.PS_QENC_FS
    d.use_pos_emb, d.use_item_pos = 1, int(bool(r['over'].get('use_item_pos', False)))
    d.training, d.dropout = 1, r['dropout']
    d.seed, d.step = 666, 0
    return d


def path_dict(p):
    """A PsEncPath as a plain dict; attn cut to n_layers."""
    out = {n: int(getattr(p, n)) for n, _ in p._fields_ if n != 'attn'}
    out['attn'] = tuple(int(p.attn[i]) for i in range(p.n_layers))
    return out


def from_json(p):
    return dict(p, attn=tuple(p['attn']))


def expected_plan(r):
    """What ps_tem_plan returns for a row under default switches."""
    e = {f: int(l in r['flags']) for l, f in FLAGS.items()}
    e.update(n_layers=r['layers'], attn=r['attn'], wgrad_early=1, wf_key_split=0)
    return e


def expected_taken(r, backward, wk_on=True):
    """What ps_enc_path_taken reports after a row's forward / backward: the direction's own fields, the other's zero.
    Backward: the kvq form reads as wf; wgrad_early belongs to the unfused FFN backward, which every layer but a fused last one
    runs; the key-split kernel is the wf backward's at 32 columns per head (d = 256) without the folded dQ.Wq (``wk_on``: the
    process's PS_ATTN_WK)."""
    e = {f: 0 for f in FLAGS.values()}
    e.update(n_layers=r['layers'], wgrad_early=0, wf_key_split=0)
    fl = r['flags']
    if not backward:
        e['attn'] = r['attn']
        for l, f in FLAGS.items():
            if f in FWD_FIELDS:
                e[f] = int(l in fl)
        return e
    e['attn'] = tuple(WF if a == KVQ else a for a in r['attn'])
    for l, f in FLAGS.items():
        if f in BWD_FIELDS:
            e[f] = int(l in fl)
    e['wgrad_early'] = int(r['layers'] > 1 or 'BF' not in fl)
    e['wf_key_split'] = int(wk_on and WF in e['attn'] and r['d'] // r['H'] == 32 and 'QF' not in fl)
    return e


def plan_of(lib, _lib, desc):
    p = _lib.PsEncPath()
    _lib.check(lib.ps_tem_plan(desc, None, 0, C.byref(p)), 'ps_tem_plan')
    return path_dict(p)


def taken(lib, _lib, backward):
    p = _lib.PsEncPath()
    _lib.check(lib.ps_enc_path_taken(backward, C.byref(p)), 'ps_enc_path_taken')
    return path_dict(p)


def diff(got, want):
    return {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}


def assert_taken(lib, r, backward):
    """The step that just ran its forward (backward = 0) or backward (1) took the row's path.  The table holds the paths of the
    default switches: in a process started under one of PLAN_SWITCHES the comparison is dropped, and said so on stdout; with a
    default environment it always runs, and deterministic mode left on by somebody is a failure, not a reason to look away."""
    from prodsearch_amd import _lib
    if not default_switches():
        print('path assertion dropped for %s: the process runs under %s'
              % (r['name'], ' '.join(k for k in PLAN_SWITCHES if k in os.environ)))
        return
    assert not lib.ps_set_deterministic(-1), "deterministic mode is on in a default-environment run (leaked by an earlier test?)"
    got, want = taken(lib, _lib, backward), expected_taken(r, backward)
    assert got == want, (r['name'], 'backward' if backward else 'forward', '(got, expected)', diff(got, want))
    if backward:
        assert int(lib.ps_item_scatter_fused_taken()) == want['item_scatter'], r['name']


def taken_checker(r):
    """``expect=`` of check_against_oracle: called with the direction that just ran."""
    from prodsearch_amd import _lib
    lib = _lib.load()
    return lambda backward: assert_taken(lib, r, backward)
