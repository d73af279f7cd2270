"""The row-wise comparison of tests/rtm_word_rows.py, checked with neither the product's kernels nor a GPU: for every case
the decomposition into occurrences is exact, the comparison accepts the fp32 oracle's word gradient at the case's bound and
rejects a float64 reference with ONE occurrence dropped or doubled (the heaviest word's, a singleton's), the bound is below half
of the change such an occurrence makes, and the recorded yardstick is not below what this run measures.  The host-only
backward plan names the index form every case claims to reach."""
import pytest
import torch

import rtm_word_rows as W
import saturated as S

CASE_NAMES = list(W.CASES)


_R32 = {}


def _fp32(name):
    """The fp32 oracle's word gradient, with one thread: a row of thousands of terms then adds up in the same order every run."""
    if name not in _R32:
        p = W.problem(name)
        old = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            _R32[name] = S.rtm_oracle_step(p, p.sd, False)['grads']['word_embeddings.weight']
        finally:
            torch.set_num_threads(old)
    return _R32[name]


@pytest.mark.parametrize('name', CASE_NAMES)
def test_rows_decompose_into_occurrences(name):
    """sum c reproduces every row no query (and no PV loss) reaches; the non-zero rows of the float64 reference are the
    words the batch addresses; the pad word's row is zero."""
    p, r64, dec = W.reference(name)
    ref = dec.ref
    addr = W.addressed_words(p)
    assert torch.equal(torch.nonzero(ref.ne(0).any(1)).flatten(), addr)
    assert float(ref[p.V - 1].abs().max()) == 0.0 and float(dec.scale[p.V - 1]) == 0.0
    other = [p.batch.query_word_idxs.reshape(-1)]
    if p.train_pv:       # the PV loss reaches its target and sampled words and, through the review vector, the positives' words
        other += [p.batch.pos_prod_rword_idxs.reshape(-1), p.neg_words.reshape(-1), p.batch.pos_prod_rword_idxs_pvc.reshape(-1)]
    pure = torch.ones(p.V, dtype=torch.bool)
    pure[torch.cat(other)] = False
    pure &= dec.count > 0
    assert int(pure.sum()) > 0
    assert float((dec.rest[pure] / dec.occ_scale[pure]).max()) < 1e-12
    assert torch.equal(torch.nonzero(dec.scale > 0).flatten(), addr)


@pytest.mark.parametrize('name', CASE_NAMES)
def test_fp32_oracle_passes_and_stays_within_the_recorded_yardstick(name):
    p, r64, dec = W.reference(name)
    got = _fp32(name)
    measured = float(W.row_errors(got, dec).max())
    print('figures: %s yardstick measured %.3e recorded %.3e bound %.3e' % (name, measured, W.YARDSTICK[name], W.bound(name)))
    assert measured <= W.YARDSTICK[name]
    assert W.compare(got, dec, W.bound(name), W.addressed_words(p), what=name) == measured


@pytest.mark.parametrize('name', CASE_NAMES)
def test_one_dropped_or_doubled_occurrence_is_rejected(name):
    p, r64, dec = W.reference(name)
    got, addr = _fp32(name), W.addressed_words(p)
    muts = W.mutations(p, dec)
    assert len(muts) == 4
    if name not in W.SHAPE_CASES:                 # (the existing shapes keep their words: the d = 128 one has no singleton)
        assert int(dec.count[muts[2][1]]) == 1 and muts[2][3] == pytest.approx(1.0, rel=1e-9)
    for label, r, ref, change in muts:
        print('figures: %s %s: err_w %.3e, bound %.3e' % (name, label, change, W.bound(name)))
        assert W.bound(name) < 0.5 * change, (label, change)
        assert float(W.row_errors(dec.ref, dec, ref)[r]) == pytest.approx(change, rel=1e-9)
        with pytest.raises(AssertionError, match='word %d ' % int(dec.rows[r])):
            W.compare(got, dec, W.bound(name), addr, ref=ref, what=name)


def test_heavy_word_is_above_the_ordered_reduce_limit():
    for name in ('heavy_d64', 'heavy_d256', 'heavy_d512'):
        p, r64, dec = W.reference(name)
        idx, ok, real = W.slot_words(p)
        live = ok & real[:, None]
        assert int(dec.count[W.HEAVY_WORD]) == int((idx.eq(W.HEAVY_WORD) & live).sum()) > W.WR_DET_LIM
        assert int((idx.eq(W.HEAVY_WORD) & live).sum(1).max()) > 1            # repeated inside a review


def test_second_list_case_has_more_than_1024_rows_per_partition():
    kw = W.CASES['hist_two_lists'][0]
    rows = kw['B'] * (kw['K'] + 1) * (kw['u_lim'] + kw['i_lim'])
    assert -(-rows // W.RTM_HIST_G) > 1024


def test_mask_cases_count_by_the_mask():
    for name in ('masks_avg', 'masks_fs'):
        p = W.problem(name)
        idx, ok, real = W.slot_words(p)
        words = idx.ne(p.V - 1) & real[:, None]
        share = float((words & ~ok).sum()) / float(words.sum())
        assert 0.25 < share < 0.42 and not bool((ok & ~idx.ne(p.V - 1)).any())


def test_near_empty_cases():
    for name, n in (('one_review', None), ('one_review_wl1', 1)):
        p, r64, dec = W.reference(name)
        real = torch.cat([p.batch.pos_prod_ridxs.reshape(-1), p.batch.neg_prod_ridxs.reshape(-1)]).ne(p.RC - 1)
        assert int(real.sum()) == 1
        assert n is None or int(dec.count.sum()) == n


@pytest.mark.parametrize('name', CASE_NAMES)
def test_host_plan_names_the_index_form(name):
    from prodsearch_amd import _lib
    lib = _lib.load()
    prev = lib.ps_set_deterministic(0)
    try:
        pl = W.backward_plan(W.plan_desc(W.problem(name)))
    finally:
        lib.ps_set_deterministic(prev)
    assert (pl.index, pl.side_fork) == W.expected_plan(name)


def test_full_size_sample_rows():
    """tests/test_gpu_fullsize_rtm.py's 128 rows: summed from the slot gradients alone (the table constant), the fp32 oracle
    within its recorded yardstick, one occurrence of the most frequent sampled word more than twice the bound."""
    p = W.fullsize_problem()
    rows = W.fullsize_sample(p)
    assert rows.numel() == 128 and not bool(torch.isin(rows, p.batch.query_word_idxs).any())
    dec = W.decompose(p, W.slot_grads_with_the_table_constant(p, p.sd, True), rows=rows)
    got = W.fp32_rows(p, W.slot_grads_with_the_table_constant(p, p.sd, False), dec)
    limit = max(8.0 * W.YARDSTICK_FULLSIZE, W.FLOOR)
    measured = W.compare(got, dec, limit, what='full size')
    print('figures: full size yardstick measured %.3e recorded %.3e, counts %d .. %d' % (
        measured, W.YARDSTICK_FULLSIZE, int(dec.count.min()), int(dec.count.max())))
    assert measured <= W.YARDSTICK_FULLSIZE
    for label, r, ref, change in W.mutations(p, dec):
        assert limit < 0.5 * change, (label, change)
        with pytest.raises(AssertionError, match='word %d ' % int(dec.rows[r])):
            W.compare(got, dec, limit, ref=ref, what='full size')


def test_a_row_without_a_reference_must_be_zero_and_the_touched_set_exact():
    p, r64, dec = W.reference('one_review')
    addr = W.addressed_words(p)
    got = dec.ref.clone()
    free = int(torch.nonzero(dec.scale.eq(0)).flatten()[0])
    got[free, 0] = 1e-30
    with pytest.raises(AssertionError, match='word %d has no reference' % free):
        W.compare(got, dec, W.bound('one_review'), addr)
    got = dec.ref.clone()
    got[int(addr[0])] = 0
    with pytest.raises(AssertionError, match='addressed words without a row'):
        W.compare(got, dec, W.bound('one_review'), addr)
