"""The row-wise comparison of tests/tem_table_rows.py, checked with neither the product's kernels nor a GPU: for every case
and every table it trains, the decomposition into occurrences closes, the rows with a scale are the rows the batch addresses,
the fp32 oracle (one thread) stays at or below the recorded yardstick and passes the comparison at the case's bound, a float64
reference with ONE occurrence dropped or doubled (the heaviest row's, a single-occurrence row's) is rejected with the row and
its count named, the bound is below half of the change such an occurrence makes, the case's preconditions hold (its edit did
what it says, Q is really filled), and the host-only plan names the encoder path the case claims."""
import functools

import pytest
import torch

import enc_paths as ep
import tem_table_rows as T

CASE_NAMES = list(T.CASES)


@functools.lru_cache(maxsize=None)
def _fp32(name):
    return T.fp32_step(name, 1)['grads']


def _tables(name):
    return list(T.reference(name)[2].items())


def test_every_case_has_a_yardstick_for_every_table_it_trains():
    assert sorted(T.YARDSTICK) == sorted(T.CASES)
    for name in CASE_NAMES:
        assert sorted(T.YARDSTICK[name]) == sorted(T.trained_tables(T.problem(name))), name
    assert set(T.DET_CASES) <= set(T.CASES)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_rows_decompose_into_occurrences(name):
    """sum c reproduces every row to 1e-12 of its scale; rows without a scale are exactly zero in the reference; the rows
    with a scale, and the reference's non-zero rows, are the rows the index tensors address; the pad rows are zero."""
    p, r64, decs = T.reference(name)
    assert T.PROD in decs and T.WORD in decs and T.WBIAS in decs
    assert (T.HIST in decs) == bool(p.a.sep_prod_emb) and (T.PBIAS in decs) == (p.a.sim_func == 'bias_product')
    for table, dec in decs.items():
        live = dec.scale > 0
        assert float((dec.closure[live] / dec.scale[live]).max()) <= 1e-12, table
        assert float(dec.ref[~live].abs().max()) == 0.0, table
        addr = T.addressed(p, table)
        assert torch.equal(torch.nonzero(live).flatten(), addr), table
        assert torch.equal(torch.nonzero(dec.ref.ne(0).any(1)).flatten(), addr), table
        assert int(dec.count.sum()) == dec.occ_row.numel() > 0
    assert float(decs[T.PROD].scale[p.P_]) == 0.0 and float(decs[T.WORD].scale[p.V - 1]) == 0.0
    for table in (t for t in T.TABLES if t not in decs):
        assert r64['grads'].get(table) is None, table


@pytest.mark.parametrize('name', CASE_NAMES)
def test_fp32_oracle_passes_and_stays_within_the_recorded_yardstick(name):
    p, r64, decs = T.reference(name)
    got = _fp32(name)
    for table, dec in decs.items():
        measured = float(T.row_errors(got[table], dec).max())
        print('figures: %s %s yardstick measured %.3e recorded %.3e bound %.3e' % (
            name, table, measured, T.YARDSTICK[name][table], T.bound(name, table)))
        assert measured <= T.YARDSTICK[name][table], table
        assert T.compare(got[table], dec, T.bound(name, table), T.addressed(p, table), what='%s %s' % (name, table)) == measured


@pytest.mark.parametrize('name', CASE_NAMES)
def test_one_dropped_or_doubled_occurrence_is_rejected(name):
    p, r64, decs = T.reference(name)
    got = _fp32(name)
    for table, dec in decs.items():
        addr, limit = T.addressed(p, table), T.bound(name, table)
        muts = T.mutations(dec)
        assert len(muts) == 4
        # a row with a single occurrence exists in every table; a history table of its own under replicas has K + 1 per slot
        least = p.K + 1 if (table == T.HIST and p.a.dropout > 0) else 1
        assert int(dec.count[muts[2][1]]) == least, table
        if least == 1:
            assert muts[2][3] == pytest.approx(1.0, rel=1e-9)
        assert int(dec.count[muts[0][1]]) == int(dec.count.max())
        for label, r, ref, change in muts:
            print('figures: %s %s %s: err_row %.3e, %.1f x the bound %.3e' % (name, table, label, change, change / limit, limit))
            assert limit < 0.5 * change, (table, label, change)
            assert float(T.row_errors(dec.ref, dec, ref)[r]) == pytest.approx(change, rel=1e-9)
            with pytest.raises(AssertionError, match=r'row %d \(%d occurrences\)' % (r, int(dec.count[r]))):
                T.compare(got[table], dec, limit, addr, ref=ref, what='%s %s' % (name, table))


@pytest.mark.parametrize('name', CASE_NAMES)
def test_case_preconditions(name):
    p, r64, decs = T.reference(name)
    check = T.CASES[name]['check']
    if check is not None:
        check(p)
    row = T.CASES[name]['row']
    if row is not None:              # the case has the shape of the row whose path it claims
        r = T._ROW[row]
        assert (p.B, p.K, p.L, p.W, p.a.embedding_size, p.a.heads, p.a.ff_size, float(p.a.dropout)) == \
               (r['B'], r['K'], r['L'], r['W'], r['d'], r['H'], r['F'], float(r['dropout'])), name
        assert p.batch.query_word_idxs.shape[1] == r['Q'] and p.a.inter_layers == r['layers']
        assert p.a.query_encoder_name == r['over'].get('query_encoder_name', 'fs')
    else:
        assert p.qem
    assert not bool(p.nw.eq(p.V - 1).any())          # the sampled words' distribution gives the pad no weight


def test_what_each_case_is_there_for():
    P = T.problem
    ui = lambda n: P(n).batch.u_item_idxs
    assert not bool(ui('d32_nohist').ne(P('d32_nohist').P_).any()) and T.reference('d32_nohist')[2][T.PROD].count.max() <= 3
    p = P('d32_smallest')
    assert (p.B, p.K, p.L, p.batch.query_word_idxs.shape[1]) == (1, 1, 1, 1)
    p = P('tiles_w3')                # W 3 with a masked window slot under which sampled words lie
    assert p.W == 3 and bool(p.batch.pos_iword_idxs.eq(p.V - 1).any())
    for n in ('tiles_w3', 'tiles_r2'):
        assert T.CASES[n]['fuse_bwd_min'] == 1 and (P(n).B * (P(n).K + 1)) % 32 != 0
    assert P('tiles_r2').K + 1 == 2
    assert P('fan34_d64').K + 1 == 34 and P('fan34_d64').W == 2 and P('fan34_d64').a.embedding_size == 64
    assert P('d96').B == 130 and P('d96').a.embedding_size == 96
    assert P('avg_d96').a.embedding_size == 96 and P('avg_d96').a.dropout > 0 and P('avg_d96').a.query_encoder_name == 'avg'
    assert P('avg_d64_nodrop').a.embedding_size == 64 and P('avg_d64_nodrop').a.dropout == 0
    assert P('sep').a.sep_prod_emb and P('bias').a.sim_func == 'bias_product' and P('bias').a.pos_weight
    assert P('frozen').frozen and P('frozen').sd[T.WORD].shape == P('c2s').sd[T.WORD].shape
    assert not torch.equal(P('frozen').sd[T.WORD], P('c2s').sd[T.WORD])
    for name in CASE_NAMES:
        assert P(name).B <= 130 and P(name).B * (P(name).K + 1) <= 1050, name
    # the heavy rows: thousands of additions with replicas
    dec = T.reference('heavy')[2]
    assert int(dec[T.PROD].count.argmax()) == T.HEAVY_ITEM and int(dec[T.PROD].count.max()) > 1500
    assert int(dec[T.WORD].count.argmax()) == T.HEAVY_WORD


@pytest.mark.parametrize('name', [n for n in CASE_NAMES if T.CASES[n]['row'] is not None])
def test_host_plan_names_the_path(name):
    from prodsearch_amd import _lib
    from prodsearch_amd import build as pbuild
    if not ep.default_switches():
        pytest.skip("the table holds the plan under default switches")
    pbuild.build()
    lib = _lib.load()
    fbm = T.CASES[name]['fuse_bwd_min']
    old = lib.ps_set_fuse_bwd_min(fbm) if fbm is not None else None
    prev = lib.ps_set_deterministic(0)
    try:
        got = ep.plan_of(lib, _lib, T.plan_desc(name))
    finally:
        lib.ps_set_deterministic(prev)
        if old is not None:
            lib.ps_set_fuse_bwd_min(old)
    want = ep.expected_plan(T._ROW[T.CASES[name]['row']])
    assert got == want, (name, '(got, expected)', ep.diff(got, want))


def test_a_row_without_a_reference_must_be_zero_and_the_touched_set_exact():
    p, r64, decs = T.reference('d32_nohist')
    for table, dec in decs.items():
        addr, limit = T.addressed(p, table), T.bound('d32_nohist', table)
        got = dec.ref.clone()
        free = int(torch.nonzero(dec.scale.eq(0)).flatten()[0])
        got[free, 0] = 1e-30
        with pytest.raises(AssertionError, match='row %d has no reference' % free):
            T.compare(got, dec, limit, addr)
        got = dec.ref.clone()
        got[int(addr[0])] = 0
        with pytest.raises(AssertionError, match='addressed rows without a gradient'):
            T.compare(got, dec, limit, addr)
        assert T.compare(dec.ref, dec, limit, addr) == 0.0
