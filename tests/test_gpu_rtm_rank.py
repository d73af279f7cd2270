"""``evaluate.rank_all_rtm`` on an MI355X: the review transformer over the whole catalogue in one pass against
``oracle.rtm.rtm_test`` over candidate chunks assembled from the same entries and catalogue (tests/rtm_rank_util.py), and against
the GPU's own ``model.test()`` on those chunks.  Bounds: the suite's eval bound, rel_err < 1e-4 over the whole score matrix,
and per entry against the float64 oracle 8 x what fp32 costs the same case on the host (rtm_rank_util.YARDSTICK / bound).
Every case asserts from ``ps_rtm_rank_plan`` the branch of csrc/rtm_rank.hip it was written for before it compares anything.

Measured maxima (profiles/rtm_rank_all.md): the factorisation alone costs 5e-7 .. 9e-7 in fp32 on the CPU
(tests/test_rtm_rank_cpu.py); the figures of this file are printed by every case before it asserts; the per-entry figures
measured on an MI355X, 3e-7 .. 5.2e-6 under bounds of 2.7e-6 .. 3.5e-5, are DESIGN.md §8b.1's table."""
import functools

import numpy as np
import pytest
import torch

import rtm_rank_util as U
from golden_util import rel_err

pytestmark = pytest.mark.gpu

CASES = U.CASES          # tests/rtm_rank_util.py: shared with the host-side checks of the same cases (tests/test_rtm_rank_cpu.py)
K = 10


def restore_x3(lib):
    import os
    lib.ps_gemm_x3_config(0 if os.environ.get('PS_GEMM_X3') == '0' else 1, int(os.environ.get('PS_GEMM_X3_SHAPE', '-1')))


@functools.lru_cache(maxsize=None)
def run(name, perm_seed=None):
    """One case, computed once: the oracle's scores (fp32 and float64), the plan of the call and the GPU's (dense, top-k, rank)."""
    from prodsearch_amd import _lib, evaluate
    c, ipp, scale = U.case_of(name)
    m, sd = U.build_model(c, 'cuda', scale=scale)
    ref = U.oracle_scores(c, sd)[0]
    ref64 = U.oracle_scores(c, sd, f64=True)[0]
    plan = U.plan_of(_lib.load(), m, c, K, ipp)
    item_r = c.item_r
    perm = None
    if perm_seed is not None:
        perm = torch.from_numpy(U.synth.rng_for(perm_seed).permutation(c.P))
        item_r = c.item_r[perm]
    up = c.review_u_p.cuda() if (c.a.use_user_emb or c.a.use_item_emb) else None
    index = m.catalogue_index(item_r.cuda(), up)
    rb = U.rank_batch(c, 'cuda')
    top_idx, top_score, rank, scores = evaluate.rank_all_rtm(m, index, rb, K, items_per_pass=ipp, return_scores=True)
    torch.cuda.synchronize()
    return dict(c=c, m=m, sd=sd, ref=ref, ref64=ref64, plan=plan, index=index, rb=rb, ipp=ipp, perm=perm, top_idx=top_idx.cpu(),
                top_score=top_score.cpu(), rank=rank.cpu(), scores=scores.cpu())


def check_entries(name, scores, ref64, what='rank_all_rtm'):
    """The per-entry bound: max_i |got - ref64| / max_i |ref64| of every entry within 8 x the case's host yardstick (U.bound)."""
    err = U.entry_err(scores, ref64)
    print('%s: %s vs the float64 rtm_test, worst entry %.3g (yardstick %.3g, bound %.3g)'
          % (name, what, err.max(), U.YARDSTICK[name], U.bound(name)))
    assert (err < U.bound(name)).all(), (name, what, err.tolist(), U.bound(name))


def check_order(ref, top_idx, rank, target, k, what):
    """``top_idx`` against the oracle's order wherever the oracle's gap to the neighbouring score exceeds 2 * tol * max|score|
    (inside such a band positions may swap); at most a quarter of the positions may lie in a band.  ``rank`` the same way."""
    order, band = U.banded(ref)
    P = ref.shape[1]
    assert band.mean() <= 0.25, (what, band.mean())
    kk = min(k, P)
    free = ~band[:, :kk]
    assert np.array_equal(top_idx.numpy()[:, :kk][free], order[:, :kk][free]), what
    n_banded = 0
    for b, t in enumerate(target.tolist()):
        if not 0 <= t < P:
            assert int(rank[b]) == 0, (what, b)
            continue
        pos = int(np.flatnonzero(order[b] == t)[0])
        if band[b, pos]:
            n_banded += 1
            lo, hi = pos, pos
            while lo > 0 and band[b, lo - 1]:
                lo -= 1
            while hi < P - 1 and band[b, hi + 1]:
                hi += 1
            assert lo + 1 <= int(rank[b]) <= hi + 1, (what, b)
        else:
            assert int(rank[b]) == pos + 1, (what, b, int(rank[b]), pos + 1)
    return float(band.mean()), n_banded


@pytest.mark.parametrize('name', sorted(CASES))
def test_scores_topk_rank_against_the_oracle(name):
    """Every case first shows, from ``ps_rtm_rank_plan``, the branch it was written for (U.PLAN) — a constant that moves
    (RR_IT_MAX, the 48 KB rule, the fused tail's shapes) then fails the case instead of quietly taking its coverage away.
    Then the scores: the suite's eval bound over the whole matrix against the fp32 oracle, and per entry 8 x the case's host
    yardstick against the float64 oracle (measured worst entries: DESIGN.md §8b)."""
    r = run(name)
    c = r['c']
    print('%s: plan %s' % (name, r['plan']))
    for f, v in U.PLAN[name].items():
        assert r['plan'][f] == v, (name, f, r['plan'][f], v)
    err = rel_err(r['scores'], r['ref'])
    print('%s: rank_all_rtm vs rtm_test rel_err %.3g' % (name, err))
    assert err < U.TOL
    check_entries(name, r['scores'], r['ref64'])
    frac, nb = check_order(r['ref'], r['top_idx'], r['rank'], c.target, K, name)
    print('%s: %.3f of the positions in a band, %d targets in one' % (name, frac, nb))
    assert int(r['rank'][-1]) == 0                                   # the target outside [0, P)
    # the selection itself, exactly: (score desc, id asc) over the GPU's own dense scores
    s = r['scores'].double().numpy()
    mine = np.lexsort((np.arange(c.P)[None, :].repeat(c.B, 0), -s), axis=1)[:, :K]
    assert np.array_equal(r['top_idx'].numpy(), mine)
    assert np.array_equal(r['top_score'].numpy(), np.take_along_axis(r['scores'].numpy(), mine, 1))


def test_sharp_case_is_sharp_and_full_lists_are_full():
    """What two cases rest on, shown on the float64 side: at ``scale=8`` some pair's softmax over at least four keys puts
    more than 0.99 of its weight on one key (the online rescale sees weights far from uniform), and ``lds_full`` has an entry
    and an item with 64 live ids (rr_leading's full ballot)."""
    h = U.host_case('sharp')
    assert float(h.wmax[h.keys >= 4].max()) > 0.99
    c = run('lds_full')['c']
    assert U.leading(c.u_r.numpy(), c.RC - 1)[1] == 64 and U.leading(c.item_r.numpy(), c.RC - 1)[1] == 64


def test_big_table_index_through_both_gemms():
    """The index projection KR / VR of a review table with M >= 32768 rows goes to the bf16x3 GEMM (csrc/gemm.hip, x3_shape);
    with the form switched off the fp32 kernel computes it.  Both indexes meet both bounds, and their buffers differ in some
    bit — the evidence that the rule sent the default build to the other kernel."""
    from prodsearch_amd import _lib, evaluate
    lib = _lib.load()
    name = 'big_table'
    r = run(name)
    c, m = r['c'], r['m']
    assert c.RC >= 32768
    built = {}
    try:
        for mode in (1, 0):
            lib.ps_gemm_x3_config(mode, -1)
            m.__dict__['_cat_index'] = None                            # the cached index: built under whatever ran before
            index = m.catalogue_index(c.item_r.cuda())
            scores = evaluate.rank_all_rtm(m, index, r['rb'], K, return_scores=True)[3].cpu()
            torch.cuda.synchronize()
            built[mode] = index.index.clone()
            err = rel_err(scores, r['ref'])
            print('%s: index under ps_gemm_x3_config(%d, -1): rel_err %.3g' % (name, mode, err))
            assert err < U.TOL
            check_entries(name, scores, r['ref64'], 'x3 mode %d' % mode)
    finally:
        restore_x3(lib)
        m.__dict__['_cat_index'] = None
    assert built[0].shape == built[1].shape and not torch.equal(built[0], built[1])
    d = (built[0] - built[1]).abs().max() / built[0].abs().max()
    print('%s: the two indexes differ by %.3g of the largest element' % (name, float(d)))
    assert float(d) < U.TOL


def test_ids_outside_the_review_table_count_as_the_pad():
    """``model._idx`` checks dtype and device, not range, so ids outside [0, review_count) reach the kernels; rclamp /
    rr_leading read them as the pad id: a list ends at a -1 or a review_count + 7 exactly as it ends at the pad.  Same bits."""
    from prodsearch_amd import evaluate, rtm_data
    r = run('base')
    c, m = r['c'], r['m']
    pad = c.RC - 1
    nu, ni = U.leading(c.u_r.numpy(), pad), U.leading(c.item_r.numpy(), pad)
    e, i, j = int(np.flatnonzero(nu >= 3)[0]), int(np.flatnonzero(ni >= 4)[0]), int(np.flatnonzero(ni >= 4)[1])
    got = {}
    for what, bad in (('outside', (-1, c.RC + 7)), ('pad', (pad, pad))):
        u_r, item_r = c.u_r.clone(), c.item_r.clone()
        u_r[e, 1], item_r[i, 2], item_r[j, 1] = bad[0], bad[1], bad[0]       # mid-list: live ids follow
        index = m.catalogue_index(item_r.cuda())
        rb = rtm_data.ProdSearchRankBatch(list(range(c.B)), [int(u) for u in c.users], c.target, c.qw, u_r).to('cuda')
        got[what] = [t.cpu() for t in evaluate.rank_all_rtm(m, index, rb, K, return_scores=True)]
    for a, b in zip(got['outside'], got['pad']):
        assert torch.equal(a, b)
    s = got['pad'][3]
    assert not torch.equal(s[e], r['scores'][e]) and not torch.equal(s[:, i], r['scores'][:, i])   # ... and the cut was felt
    keep = [x for x in range(c.P) if x not in (i, j)]
    others = [x for x in range(c.B) if x != e]
    assert torch.equal(s[others][:, keep], r['scores'][others][:, keep])


@pytest.mark.parametrize('name', ['base', 'pv_user_item', 'pretrained_fix_emb', 'passes', 'long', 'cap', 'cap_user'])
def test_scores_against_the_gpus_own_test(name):
    """``model.test()`` — the existing, parity-checked path — on the same chunks.  ``cap`` / ``cap_user``: the chunks are cut
    by ``assemble_chunk(limit=)``.  ``lds_full`` is not here: ``model.test()`` refuses its 129-position sequences
    (ps_rtm_score serves at most 64 positions, csrc/rtm.hip rtm_check)."""
    r = run(name)
    c, m = r['c'], r['m']
    assert type(m).__name__ == ('PretrainedProductRanker' if name == 'pretrained_fix_emb' else 'ProductRanker')
    got = torch.empty(c.B, c.P)
    with torch.no_grad():
        m.get_review_embeddings()
        for ids, b in U.chunks(c, 16):
            got[:, ids] = m.test(b.to('cuda')).cpu()
    err = rel_err(r['scores'], got)
    print('%s: rank_all_rtm vs model.test() rel_err %.3g' % (name, err))
    assert err < U.TOL


@pytest.mark.parametrize('name', ['base', 'passes'])
def test_duplicate_items_and_moved_items_get_the_same_bits(name):
    from prodsearch_amd import evaluate
    r = run(name)
    s = r['scores']
    assert torch.equal(s[:, 2], s[:, 3])                             # items 2 and 3 share one review list
    ti = evaluate.rank_all_rtm(r['m'], r['index'], r['rb'], r['c'].P, items_per_pass=r['ipp'])[0].cpu().numpy()
    for b in range(ti.shape[0]):                                      # ... and are ordered by id: the whole catalogue is listed
        assert np.flatnonzero(ti[b] == 3)[0] == np.flatnonzero(ti[b] == 2)[0] + 1
    q = run(name, perm_seed=3)                                        # the catalogue's rows permuted: other tiles, other passes
    assert torch.equal(q['scores'], s[:, q['perm']])


@pytest.mark.parametrize('k', [1, 37, 50])
def test_selection_edges(k):
    from prodsearch_amd import evaluate
    r = run('base')
    c = r['c']
    ti, ts, rk = evaluate.rank_all_rtm(r['m'], r['index'], r['rb'], k)
    ti, ts, rk = ti.cpu(), ts.cpu(), rk.cpu()
    kk = min(k, c.P)
    s = r['scores'].double().numpy()
    mine = np.lexsort((np.arange(c.P)[None, :].repeat(c.B, 0), -s), axis=1)[:, :kk]
    assert np.array_equal(ti.numpy()[:, :kk], mine)
    assert np.array_equal(ts.numpy()[:, :kk], np.take_along_axis(r['scores'].numpy(), mine, 1))
    assert (ti[:, kk:] == -1).all() and torch.isneginf(ts[:, kk:]).all()      # unfilled slots as in ps_rank_all
    assert torch.equal(rk, r['rank'])


def test_stale_index_is_refused_and_a_rebuilt_one_matches():
    from prodsearch_amd import evaluate, rtm_data
    from prodsearch_amd.optimizers import build_optim
    c = U.make_case()
    m, _ = U.build_model(c, 'cuda')
    index = m.catalogue_index(c.item_r.cuda())
    rb = U.rank_batch(c, 'cuda')
    evaluate.rank_all_rtm(m, index, rb, K)
    assert m.catalogue_index(index.item_ridxs) is index              # cached while nothing changed
    optim = build_optim(c.a, m, None)
    m.train()
    tb = rtm_data.make_rtm_batch(21, 4, 2, c.RC, c.V, c.rw, Q=5, u_lim=c.U, i_lim=c.I, W=1, train_pv=False, encoder='pvc').to('cuda')
    loss = m(tb, train_pv=False)
    m.zero_grad()
    loss.backward()
    optim.step()
    m.eval()
    with pytest.raises(RuntimeError, match='stale'):
        evaluate.rank_all_rtm(m, index, rb, K)
    old_table = m.review_embeddings                                   # (pvc: computed from the word table, which has moved)
    again = m.catalogue_index(index.item_ridxs)
    assert again is not index and m.review_embeddings is not old_table      # the review table was rebuilt with the index
    scores = evaluate.rank_all_rtm(m, again, rb, K, return_scores=True)[3].cpu()
    err = rel_err(scores, U.oracle_scores(c, U.state_of(m))[0])
    print('after one optimizer step: rel_err %.3g' % err)
    assert err < U.TOL


def test_trainer_takes_the_pass_behind_its_flag(tmp_path):
    """``args.rtm_rank_all``: Trainer.test gives the MRR / P@1 and the ranklist ids of the default chunked path.  Entries whose
    target sits in a band of the default path's own scores (gap <= 2 * tol * max|score|) may differ in rank; printed."""
    import os
    from prodsearch_amd import default_args, synth, trainer, corpus, pyrandom
    data_path, inp = synth.write_corpus(str(tmp_path / 'c'), 33, n_users=50, n_products=40, n_words=150)
    args = default_args(model_name='review_transformer', review_encoder_name='pvc', embedding_size=64, ff_size=128, heads=8,
                        inter_layers=1, uprev_review_limit=4, iprev_review_limit=6, review_word_limit=16, subsampling_rate=1e-1,
                        candi_batch_size=16, test_candi_size=-1, valid_candi_size=-1, valid_batch_size=12, data_dir=data_path,
                        input_train_dir=inp, save_dir=str(tmp_path / 'r'), device='cuda', dropout=0.0)
    os.makedirs(args.save_dir)
    args.start_epoch = 0
    torch.manual_seed(1); pyrandom.seed(1); np.random.seed(1)
    gd = corpus.GlobalProdSearchData(args, data_path, inp)
    train_pd = corpus.ProdSearchData(args, inp, 'train', gd)
    test_pd = corpus.ProdSearchData(args, inp, 'test', gd)
    model, _ = trainer.create_model(args, gd, train_pd)
    tr = trainer.Trainer(args, model, None)
    ds = corpus.ProdSearchDataset(args, gd, test_pd)
    P = gd.product_size
    rank0, ids0, sc0, users0, queries0 = tr._scores_candidates(args, ds, P, topk=P)
    args.rtm_rank_all = True
    rank1, ids1, sc1, users1, queries1 = tr._scores_rank_all_rtm(args, gd, ds, P)
    assert users0 == users1 and queries0 == queries1
    sc0, ids0, ids1 = sc0.cpu().numpy(), ids0.cpu().numpy(), ids1.cpu().numpy()
    close = np.abs(np.diff(sc0, axis=1)) <= 2 * U.TOL * np.abs(sc0).max()
    band = np.zeros_like(sc0, dtype=bool)
    band[:, :-1] |= close
    band[:, 1:] |= close
    assert np.array_equal(ids1[~band], ids0[~band])
    r0, r1 = rank0.cpu().numpy(), rank1.cpu().numpy()
    flagged = np.array([band[b, r - 1] for b, r in enumerate(r0)])
    print('%d of %d entries have their target in a band' % (int(flagged.sum()), len(r0)))
    assert np.array_equal(r0[~flagged], r1[~flagged])
    # ... and through Trainer.test, the flag off and on
    args.rtm_rank_all = False
    m0 = tr.test(args, gd, test_pd, 'chunked.ranklist')
    args.rtm_rank_all = True
    m1 = tr.test(args, gd, test_pd, 'one_pass.ranklist')
    v1 = tr.validate(args, gd, ds)
    from prodsearch_amd import evaluate
    assert m0 == evaluate.calc_metrics(rank0, 100)
    assert m1 == evaluate.calc_metrics(rank1, 100) and v1 == m1       # what Trainer.test / validate return under the flag
    r1_sub = np.where(flagged, r0, r1)                                # ... equal to the default path's but for the flagged entries
    assert evaluate.calc_metrics(torch.from_numpy(r1_sub), 100) == m0
    if not flagged.any():
        assert m0 == m1
    l0 = open(os.path.join(args.save_dir, 'chunked.ranklist')).read().splitlines()
    l1 = open(os.path.join(args.save_dir, 'one_pass.ranklist')).read().splitlines()
    assert len(l0) == len(l1) == len(r0) * min(100, P)
    keep = ~band[:, :min(100, P)].reshape(-1)
    pick = lambda ls: [ln.split(' ')[:4] for ln, k in zip(ls, keep) if k]
    assert pick(l0) == pick(l1)
