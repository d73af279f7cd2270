"""The item models' table gradients row by row against the float64 oracle (tests/tem_table_rows.py): the score backward's
item and word tasks, the history and query-word scatters, the item scatter inside the fused per-replica backward and the
deterministic forms (csrc/rowwise.hip, csrc/mlp_fused.hip), at the shapes that reach each of their branches — queries of up to
70 words, a query without words, d = 32 .. 512, 2 .. 34 replicas, partial tiles, masked window slots, a separate history
table, the product bias, rows with thousands of additions, a frozen word table.

One forward and one backward of the module per case, built as test_gpu_tem_options.check_against_oracle builds it; the
oracle's Philox masks are the product's (seed 666, training step 1).  The loss to 1e-4, the encoder path the step took
(tests/enc_paths.py, so no case passes through another form), and ``compare`` on every table and bias vector the case
trains: rows without a reference exactly zero, the non-zero rows exactly the addressed ones, every err_row within
max(8 x the fp32 oracle's own, 2^-22)."""
import pytest
import torch

import enc_paths as ep
import tem_table_rows as T
from golden_util import rel_err

pytestmark = pytest.mark.gpu


def _step(name, det=False, item_scatter=1):
    """The case's step on the GPU under its switches: (module, loss, {table: gradient or None}).  The path is asserted
    here: the row's own in a default run; with the item scatter switched off the same but for that field; in deterministic
    mode only that the fused backward did not scatter (the table holds the default plan)."""
    from prodsearch_amd import ItemTransformerRanker, _lib
    p, case = T.problem(name), T.CASES[name]
    row = T._ROW[case['row']] if case['row'] is not None else None
    lib = _lib.load()
    old_min = lib.ps_set_fuse_bwd_min(case['fuse_bwd_min']) if case['fuse_bwd_min'] is not None else None
    old_is = lib.ps_set_item_scatter_fused(0) if item_scatter == 0 else None
    old_det = lib.ps_set_deterministic(1 if det else 0)
    try:
        m = ItemTransformerRanker(p.a, 'cuda', p.V, p.P_, getattr(p, 'words', None), word_dists=p.wd)
        frozen = getattr(p, 'frozen', False)
        m.load_state_dict({k: v for k, v in p.sd.items() if not (frozen and k == T.WORD)}, strict=False)
        if frozen:
            assert torch.equal(m.word_embeddings.weight.detach().cpu(), p.sd[T.WORD])
        m.train()
        assert m._seed == 666
        loss = m(p.batch.to('cuda'), neg_item_idxs=p.ni.cuda(), neg_word_idxs=p.nw.cuda())
        assert m._fwd_step == 1
        plain = row is not None and not det and item_scatter == 1
        if plain:
            ep.assert_taken(lib, row, 0)
        m.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        if plain:
            ep.assert_taken(lib, row, 1)
        elif row is not None and not det and ep.default_switches():
            want = dict(ep.expected_taken(row, 1), item_scatter=0)
            got = ep.taken(lib, _lib, 1)
            assert got == want, (name, '(got, expected)', ep.diff(got, want))
        if det or item_scatter == 0:
            assert int(lib.ps_item_scatter_fused_taken()) == 0
        params = dict(m.named_parameters())
        grads = {t: (None if params[t].grad is None else params[t].grad.detach().cpu().clone()) for t in T.TABLES if t in params}
        return m, loss.detach().cpu(), grads
    finally:
        lib.ps_set_deterministic(old_det)
        if old_is is not None:
            lib.ps_set_item_scatter_fused(old_is)
        if old_min is not None:
            lib.ps_set_fuse_bwd_min(old_min)


def _check(name, loss, grads, label=''):
    p, r64, decs = T.reference(name)
    frozen = getattr(p, 'frozen', False)
    tables = [t for t in decs if not (frozen and t == T.WORD)]
    errs = {t: float(T.row_errors(grads[t], decs[t]).max()) for t in tables if grads.get(t) is not None}
    print('figures: %s%s loss %.2e | %s' % (name, label, rel_err(loss, r64['loss']), ' | '.join(
        '%s worst err_row %.3e bound %.3e' % (t, errs.get(t, float('nan')), T.bound(name, t)) for t in tables)))
    for t in errs:                       # where the order of a sum shows: the row with the most additions
        h = int(decs[t].count.argmax())
        print('figures: %s%s %s heaviest row %d (%d occurrences) err_row %.3e' % (
            name, label, t, h, int(decs[t].count[h]), float(T.row_errors(grads[t], decs[t])[h])))
    assert rel_err(loss, r64['loss']) < 1e-4
    for t in T.TABLES:
        if t in grads and t not in tables:               # a table the case does not train (or the frozen word table)
            assert grads[t] is None, t
    for t in tables:
        assert grads.get(t) is not None, t
        T.compare(grads[t], decs[t], T.bound(name, t), T.addressed(p, t), what='%s%s %s' % (name, label, t))


@pytest.mark.parametrize('name', list(T.CASES))
def test_table_rows_match_the_float64_oracle(name):
    m, loss, grads = _step(name)
    if name == 'c2s' and ep.default_switches():
        from prodsearch_amd import _lib
        assert int(_lib.load().ps_item_scatter_fused_taken()) == 1
    _check(name, loss, grads)


def test_c2s_item_rows_from_the_score_backward():
    """The fused backward's item scatter switched off: the item rows come from the score backward's item workgroups."""
    m, loss, grads = _step('c2s', item_scatter=0)
    _check('c2s', loss, grads, ' (item scatter not fused)')


@pytest.mark.parametrize('name', list(T.DET_CASES))
def test_table_rows_match_in_deterministic_mode(name):
    """The sole-owner forms (score_bwd_det_kernel, embed_scatter_det_kernel, rows_scatter_det_kernel): the same data, the
    same bounds."""
    m, loss, grads = _step(name, det=True)
    _check(name, loss, grads, ' (deterministic)')
