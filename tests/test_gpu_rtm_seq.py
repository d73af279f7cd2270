"""``evaluate.rank_seq_rtm`` on an MI355X: the review transformer's one-pass evaluation in the time-ordered
setting (``do_seq_review_test`` without ``train_review_only``), in both forms — over every entry's own candidate list and over
the whole catalogue — against ``oracle.rtm.rtm_test`` entry by entry on the catalogue that entry's stamp cuts
(tests/rtm_seq_util.py: ``cat_of``, numpy's ``searchsorted``), against the GPU's own ``model.test()`` on the same chunks, and
bit for bit against ``evaluate.rank_all_rtm`` of a static-mode twin of the model over ``catalogue_index(cat_of(stamp[e]))``,
which reduces everything after the window lookup to code the static rankers' files already pin.  Bounds: the suite's eval bound,
rel_err < 1e-4, and per entry against the float64 oracle 8 x what fp32 costs the case on the host (S.YARDSTICK / S.bound).
Every case asserts from ``ps_rtm_rank_seq_plan`` the fields it was written for before it compares anything, and every figure is
printed before it is asserted.

Measured on an MI355X (DESIGN.md §8b.3's table): worst entry 2.9e-7 .. 5.4e-6 under bounds of 2.5e-6 .. 6.2e-5; every pair of
every case, in both forms, bit-equal to the static twin's ``rank_all_rtm``."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

import rtm_cand_util as K
import rtm_rank_util as U
import rtm_seq_util as S
from golden_util import rel_err

pytestmark = pytest.mark.gpu

KTOP = 10
# model.test() refuses heads1_d128's head width (the chunked encoder serves d / heads <= 64), as tests/test_gpu_rtm_rank.py found
NO_MODEL_TEST = ('heads1_d128',)


def cat_semantics(scores, target, P, k):
    """The catalogue rule of ``ps_rtm_rank_all`` on a dense [B, P] matrix: ids by (score desc, id asc); rank = 1 + the items
    ahead of the target — a greater score, or an equal one at a lower id — 0 where the target is not a product."""
    s = np.asarray(scores, dtype=np.float32)
    order = np.lexsort((np.arange(P)[None, :].repeat(len(s), 0), -s), axis=1)
    top_idx = order[:, :k].astype(np.int64)
    top_score = np.take_along_axis(s, top_idx, 1)
    rank = np.zeros(len(s), np.int64)
    for b, t in enumerate(np.asarray(target).tolist()):
        if 0 <= t < P:
            rank[b] = 1 + int(np.flatnonzero(order[b] == t)[0])
    return top_idx, top_score, rank


@functools.lru_cache(maxsize=None)
def run(name):
    """One case, computed once: the plans of its two calls, the GPU's (dense, top-k, rank) in both forms, and the static twin's
    ``rank_all_rtm`` scores, row e from ``catalogue_index(cat_of(stamp[e]))``.  The host oracles are ``S.host_case``'s."""
    from prodsearch_amd import _lib, evaluate
    h = S.host_case(name)
    c, tl, lists = h.c, h.tl, h.lists
    W, pad = S.window_of(c), c.RC - 1
    m, sd = U.build_model(c, 'cuda', scale=h.scale)
    lib = _lib.load()
    plans = dict(list=S.plan_of(lib, m, c, S.C_LIST, KTOP, h.spp_list), cat=S.plan_of(lib, m, c, None, KTOP, h.spp_cat))
    up = c.review_u_p.cuda() if (c.a.use_user_emb or c.a.use_item_emb) else None
    index = m.timeline_index(torch.from_numpy(tl.ptr).cuda(), torch.from_numpy(tl.rids).cuda(), torch.from_numpy(tl.times).cuda(), up)
    rb_list, rb_cat = S.rank_batch(c, tl, lists, 'cuda'), S.rank_batch(c, tl, None, 'cuda')
    out = dict(h=h, c=c, m=m, sd=sd, tl=tl, lists=lists, plans=plans, index=index, rb_list=rb_list, rb_cat=rb_cat)
    for form, rb, spp in (('list', rb_list, h.spp_list), ('cat', rb_cat, h.spp_cat)):
        ti, ts, rk, sc = evaluate.rank_seq_rtm(m, index, rb, KTOP, slots_per_pass=spp, return_scores=True)
        out[form] = dict(top_idx=ti.cpu(), top_score=ts.cpu(), rank=rk.cpu(), scores=sc.cpu())
    # the static twin: the same weights, a model of the static mode, one catalogue index per entry
    cs = copy.copy(c)
    cs.a = h.static_a
    ms, _ = U.build_model(cs, 'cuda', scale=h.scale)
    static = torch.empty(c.B, c.P)
    for e in range(c.B):
        cat = torch.from_numpy(S.cat_of(tl, int(tl.stamps[e]), W, pad)).cuda()
        static[e] = evaluate.rank_all_rtm(ms, ms.catalogue_index(cat, up), U.rank_batch(c, 'cuda'), KTOP, return_scores=True)[3][e].cpu()
    torch.cuda.synchronize()
    out['static'] = static
    return out


@pytest.mark.parametrize('name', sorted(S.CASES))
def test_scores_topk_rank_against_the_oracle_and_the_static_pass(name):
    """(a) dense scores against the fp32 oracle at TOL, dead slots -inf; (b) per entry against the float64 oracle within
    min(8 x yardstick, TOL); (d) every score bit-equal to the static twin's ``rank_all_rtm`` over ``cat_of(stamp[e])``, in both
    forms; (e) top-k and rank exactly the stated semantics on the GPU's own scores, and the oracle's order outside bands."""
    r = run(name)
    h, c, lists = r['h'], r['c'], r['lists']
    want = S.plan_passes(name, c)
    for form in ('list', 'cat'):
        print('%s / %s: plan %s' % (name, form, r['plans'][form]))
        for f, v in S.PLAN[name].items():
            assert r['plans'][form][f] == v, (name, form, f, r['plans'][form][f], v)
        assert (r['plans'][form]['slots_per_pass'], r['plans'][form]['passes']) == want[form]
    # ---- the catalogue form
    s = r['cat']['scores']
    assert s.shape == (c.B, c.P) and torch.isfinite(s).all()
    err = rel_err(s, h.ref32)
    e = U.entry_err(s, h.ref64)
    print('%s / cat: vs rtm_test rel_err %.3g; vs the float64 rtm_test worst entry %.3g (yardstick %.3g, bound %.3g)'
          % (name, err, e.max(), S.YARDSTICK[name][0], S.bound(name, 'cat')))
    assert err < S.TOL
    assert (e < S.bound(name, 'cat')).all(), (name, e.tolist())
    n_diff = int((s != r['static']).sum())
    print('%s / cat: %d of %d pairs differ in some bit from the static twin' % (name, n_diff, s.numel()))
    assert torch.equal(s, r['static'])
    ti, ts, rk = cat_semantics(s.numpy(), c.target.numpy(), c.P, KTOP)
    assert np.array_equal(r['cat']['top_idx'].numpy(), ti) and np.array_equal(r['cat']['top_score'].numpy(), ts)
    assert np.array_equal(r['cat']['rank'].numpy().astype(np.int64), rk)
    order, band, frac = S.cat_bands(h.ref32)
    assert frac <= S.BAND_CAP
    n_banded = 0
    for b in range(1, c.B):                                                  # (entry 0: one exact tie, checked below)
        free = ~band[b, :KTOP]
        assert np.array_equal(ti[b][free], order[b, :KTOP][free]), (name, b)
        t = int(c.target[b])
        if not 0 <= t < c.P:
            assert rk[b] == 0
            continue
        pos = int(np.flatnonzero(order[b] == t)[0])
        if band[b, pos]:
            n_banded += 1
        else:
            assert rk[b] == pos + 1, (name, b, rk[b], pos + 1)
    print('%s / cat: %.3f of the positions in a band (entry 0 apart), %d targets in one' % (name, frac, n_banded))
    # ---- the list form
    live = torch.from_numpy(K.live_of(lists, c.P))
    s = r['list']['scores']
    ref32, ref64 = K.take(h.ref32, lists, c.P), K.take(h.ref64, lists, c.P)
    assert torch.isneginf(s[~live]).all() and torch.isfinite(s[live]).all()
    err = rel_err(s[live], ref32[live])
    e = K.list_err(s, ref64, lists, c.P)
    print('%s / list: vs rtm_test rel_err %.3g over %d live slots; vs the float64 rtm_test worst entry %.3g (yardstick %.3g, bound %.3g)'
          % (name, err, int(live.sum()), e.max(), S.YARDSTICK[name][1], S.bound(name, 'list')))
    assert err < S.TOL
    assert (e < S.bound(name, 'list')).all(), (name, e.tolist())
    same = K.take(r['static'], lists, c.P)
    print('%s / list: %d of %d live slots differ in some bit from the static twin' % (name, int((same[live] != s[live]).sum()), int(live.sum())))
    assert torch.equal(same[live], s[live])
    ti, ts, rk = K.semantics(s.numpy(), lists, c.target.numpy(), c.P, KTOP)
    assert np.array_equal(r['list']['top_idx'].numpy(), ti) and np.array_equal(r['list']['top_score'].numpy(), ts)
    assert np.array_equal(r['list']['rank'].numpy().astype(np.int64), rk)
    from test_gpu_rtm_cand import check_order
    frac, nb = check_order(ref32, lists, c.P, r['list']['top_idx'], r['list']['rank'], c.target, KTOP, name)
    print('%s / list: %.3f of the listed positions in a band, %d targets in one' % (name, frac, nb))


@pytest.mark.parametrize('name', sorted(n for n in S.CASES if n not in NO_MODEL_TEST))
def test_scores_against_the_gpus_own_test(name):
    """(c) ``model.test()`` — the existing, parity-checked chunked path — on every entry's own chunk: the whole catalogue as the
    entry's stamp cuts it, and the entry's list."""
    r = run(name)
    c, m, tl, lists = r['c'], r['m'], r['tl'], r['lists']
    W, pad = S.window_of(c), c.RC - 1
    live = K.live_of(lists, c.P)
    got_cat, got_list = torch.empty(c.B, c.P), torch.full((c.B, S.C_LIST), float('-inf'))
    with torch.no_grad():
        m.get_review_embeddings()
        for e in range(c.B):
            item_r = S.cat_of(tl, int(tl.stamps[e]), W, pad)
            got_cat[e] = m.test(S.entry_chunk(c, e, item_r, np.arange(c.P)).to('cuda'))[0].cpu()
            cols = np.where(live[e], lists[e], -1)
            got_list[e] = m.test(S.entry_chunk(c, e, item_r, cols).to('cuda'))[0].cpu()
    lv = torch.from_numpy(live)
    e_cat, e_list = rel_err(r['cat']['scores'], got_cat), rel_err(r['list']['scores'][lv], got_list[lv])
    print('%s: rank_seq_rtm vs model.test() rel_err %.3g (catalogue), %.3g (lists)' % (name, e_cat, e_list))
    assert e_cat < S.TOL and e_list < S.TOL


@pytest.mark.parametrize('name', ['base', 'd512', 'cap'])
def test_special_rows_and_slots(name):
    """(f) the INT64_MIN entry scores every item alike and lists them by id; the tie entry takes the whole run; the long items'
    windows; the pad id in mid-window; a dead slot in the middle of a list; targets absent or outside [0, P)."""
    from prodsearch_amd import evaluate
    r = run(name)
    c, tl, lists, m, index = r['c'], r['tl'], r['lists'], r['m'], r['index']
    W, pad = S.window_of(c), c.RC - 1
    cat, lst = r['cat'], r['list']
    s = cat['scores']
    # entry 0: no item has a review at INT64_MIN — one score, bit for bit, the catalogue listed by id, the target's rank its id + 1
    assert (s[0] == s[0, 0]).all() and cat['top_idx'][0].tolist() == list(range(KTOP))
    assert int(cat['rank'][0]) == int(c.target[0]) + 1
    assert (lst['scores'][0, :4] == s[0, 0]).all() and lst['top_idx'][0].tolist() == [0, 1, 2, 3] + [-1] * (KTOP - 4)
    # entry 2, item 2: bisect_right takes the run of equal times; with bisect_left the pair would score otherwise
    up = c.review_u_p.cuda() if (c.a.use_user_emb or c.a.use_item_emb) else None
    cs = copy.copy(c)
    cs.a = r['h'].static_a
    ms, _ = U.build_model(cs, 'cuda', scale=r['h'].scale)
    left = torch.from_numpy(S.cat_of(tl, int(tl.stamps[2]), W, pad, 'cut_left')).cuda()
    s_left = evaluate.rank_all_rtm(ms, ms.catalogue_index(left, up), U.rank_batch(c, 'cuda'), KTOP, return_scores=True)[3][2].cpu()
    print('%s: entry 2 / item 2 scores %.6f with the run, %.6f without' % (name, float(s[2, 2]), float(s_left[2])))
    assert s[2, 2] == r['static'][2, 2] != s_left[2] and lst['scores'][2, 0] == s[2, 2]
    # the long items (two and three search rounds, the 64 / 65 boundary): each pair on its own, both forms
    for e in range(1, c.B):
        for i in (2, 3, 4, 5, 6):
            assert s[e, i] == r['static'][e, i], (e, i)
    for col, i in ((0, 3), (1, 5), (3, 6), (6, 2), (8, 4)):
        assert lists[1, col] == i and lst['scores'][1, col] == s[1, i]
    # entry 1 sees the last W of item 5, the pad id among them: the reviews after it do not count
    row = S.cat_of(tl, S.I64_MAX, W, pad)
    n = int(U.leading(row, pad)[S.PAD_ITEM])
    assert 0 < n < W and (row[S.PAD_ITEM, n + 1:] != pad).all()
    cut = row.copy()
    cut[S.PAD_ITEM, n:] = pad
    s_cut = evaluate.rank_all_rtm(ms, ms.catalogue_index(torch.from_numpy(cut).cuda(), up), U.rank_batch(c, 'cuda'), KTOP,
                                  return_scores=True)[3][1].cpu()
    assert s[1, S.PAD_ITEM] == s_cut[S.PAD_ITEM]
    # entry 1's list: its target at columns 2 and 7, a dead id at 4, -1 at 5; topk above the live count leaves -1 / -inf
    k = S.C_LIST + 8
    ti, ts, rk = (t.cpu() for t in evaluate.rank_seq_rtm(m, index, r['rb_list'], k, slots_per_pass=r['h'].spp_list))
    e_ti, e_ts, e_rk = K.semantics(lst['scores'].numpy(), lists, c.target.numpy(), c.P, k)
    assert np.array_equal(ti.numpy(), e_ti) and np.array_equal(ts.numpy(), e_ts) and np.array_equal(rk.numpy().astype(np.int64), e_rk)
    n_live = int(K.live_of(lists, c.P)[1].sum())
    assert n_live == S.C_LIST - 2 and (ti[1, n_live:] == -1).all() and torch.isneginf(ts[1, n_live:]).all()
    assert c.P + 3 not in ti[1].tolist() and lst['scores'][1, 2] == lst['scores'][1, 7]
    sl = lst['scores'][1]
    assert int(rk[1]) == 1 + int(((sl > sl[2]) | ((sl == sl[2]) & (torch.arange(S.C_LIST) < 2))).sum())
    # a target outside [0, P): rank 0 in both forms; one inside the catalogue but not in the list: 0 in the list form alone
    assert int(rk[-1]) == 0 and int(cat['rank'][-1]) == 0
    absent = next(i for i in range(c.P) if i not in lists[3].tolist())
    tg = c.target.clone()
    tg[3] = absent
    rk2 = evaluate.rank_seq_rtm(m, index, S.rank_batch(c, tl, lists, 'cuda', target=tg), KTOP, slots_per_pass=r['h'].spp_list)[2].cpu()
    rk3 = evaluate.rank_seq_rtm(m, index, S.rank_batch(c, tl, None, 'cuda', target=tg), KTOP, slots_per_pass=r['h'].spp_cat)[2].cpu()
    assert int(rk2[3]) == 0 and torch.equal(rk2[:3], lst['rank'][:3])
    assert int(rk3[3]) == 1 + int(((s[3] > s[3, absent]) | ((s[3] == s[3, absent]) & (torch.arange(c.P) < absent))).sum())


def test_passes_do_not_change_a_bit():
    """(g) the lists in passes of 5 + 5 + 2 and the catalogue in 8 x 4 + 5 (the last ragged, run at the full pass shape)
    against the single pass."""
    one, many = run('base'), run('passes')
    assert one['plans']['list']['passes'] == 1 and many['plans']['list']['passes'] == 3
    assert one['plans']['cat']['passes'] == 1 and many['plans']['cat']['passes'] == 5
    assert np.array_equal(one['lists'], many['lists']) and np.array_equal(one['tl'].rids, many['tl'].rids)
    for form in ('list', 'cat'):
        for f in ('scores', 'top_idx', 'top_score', 'rank'):
            assert torch.equal(one[form][f], many[form][f]), (form, f)


def test_index_is_cached_checked_and_refused_when_stale():
    """(h) the same inputs give the cached index; a weight edited in place makes it stale; an unsorted item is refused on the
    device with its number; a static-mode model is served as well."""
    from prodsearch_amd import evaluate
    c, static_a, _ = S.case_of('base')
    tl = S.make_timeline(c)
    m, _ = U.build_model(c, 'cuda')
    dev = [torch.from_numpy(x).cuda() for x in (tl.ptr, tl.rids, tl.times)]
    index = m.timeline_index(*dev)
    assert m.timeline_index(*dev) is index and not index.stale()
    rb = S.rank_batch(c, tl, None, 'cuda')
    before = evaluate.rank_seq_rtm(m, index, rb, KTOP, return_scores=True)[3].cpu()
    with torch.no_grad():
        m._named_hot_params()[0][1].mul_(1.0)
    with pytest.raises(RuntimeError, match='stale'):
        evaluate.rank_seq_rtm(m, index, rb, KTOP)
    again = m.timeline_index(*dev)
    assert again is not index
    assert torch.equal(before, evaluate.rank_seq_rtm(m, again, rb, KTOP, return_scores=True)[3].cpu())
    times = tl.times.copy()
    at = int(tl.ptr[3]) + 2000
    times[at - 1], times[at] = S.T_MAX + 5, S.T_MAX + 4
    with pytest.raises(RuntimeError, match='item 3 '):
        m.timeline_index(dev[0], dev[1], torch.from_numpy(times).cuda())
    cs = copy.copy(c)
    cs.a = static_a
    ms, _ = U.build_model(cs, 'cuda')
    assert torch.equal(before, evaluate.rank_seq_rtm(ms, ms.timeline_index(*dev), rb, KTOP, return_scores=True)[3].cpu())
    with pytest.raises(RuntimeError, match='another model'):
        evaluate.rank_seq_rtm(ms, again, rb, KTOP)


def _bands_of(sc):
    close = np.abs(np.diff(sc, axis=1)) <= 2 * U.TOL * np.abs(sc[np.isfinite(sc)]).max()
    band = np.zeros_like(sc, dtype=bool)
    band[:, :-1] |= close
    band[:, 1:] |= close
    return band


def test_trainer_takes_the_time_ordered_pass_behind_its_flag(tmp_path):
    """(i) ``args.rtm_rank_all`` in the time-ordered mode, against the default chunked path: validation on ``valid_candi_size =
    7`` sampled products in chunks of 3, and a test over all products with its ranklist.  Ids, ranks, metrics and ranklist lines
    are equal outside bands of the default path's own scores; printed."""
    from prodsearch_amd import default_args, synth, trainer, corpus, pyrandom, evaluate
    data_path, inp = synth.write_corpus(str(tmp_path / 'c'), 33, n_users=50, n_products=40, n_words=150)
    args = default_args(model_name='review_transformer', review_encoder_name='pvc', embedding_size=64, ff_size=128, heads=8,
                        inter_layers=1, uprev_review_limit=4, iprev_review_limit=6, review_word_limit=16, subsampling_rate=1e-1,
                        candi_batch_size=3, test_candi_size=-1, valid_candi_size=7, valid_batch_size=12, data_dir=data_path,
                        input_train_dir=inp, save_dir=str(tmp_path / 'r'), device='cuda', dropout=0.0, use_user_emb=True,
                        use_item_emb=True, do_seq_review_test=True, train_review_only=False)
    os.makedirs(args.save_dir)
    args.start_epoch = 0
    torch.manual_seed(1); pyrandom.seed(1); np.random.seed(1)
    gd = corpus.GlobalProdSearchData(args, data_path, inp)
    train_pd = corpus.ProdSearchData(args, inp, 'train', gd)
    valid_pd = corpus.ProdSearchData(args, inp, 'valid', gd)
    test_pd = corpus.ProdSearchData(args, inp, 'test', gd)
    model, _ = trainer.create_model(args, gd, train_pd)
    tr = trainer.Trainer(args, model, None)
    P = gd.product_size
    # ---- sampled validation: the dataset draws the lists once; both paths read the same dataset
    ds = corpus.ProdSearchDataset(args, gd, valid_pd)
    rank0, ids0, sc0, users0, queries0 = tr._scores_candidates(args, ds, 7, topk=7)
    args.rtm_rank_all = True
    rank1, ids1, sc1, users1, queries1 = tr._scores_rank_seq_rtm(args, gd, ds, 7, True)
    assert users0 == users1 and queries0 == queries1 and len(users0) * 3 == len(ds)
    sc0, ids0, ids1 = sc0.cpu().numpy(), ids0.cpu().numpy(), ids1.cpu().numpy()
    band = _bands_of(sc0)
    assert ids0.shape == ids1.shape and np.array_equal(ids1[~band], ids0[~band])
    err = rel_err(sc1.cpu()[torch.from_numpy(~band)], torch.from_numpy(sc0)[torch.from_numpy(~band)])
    print('validation: one-pass vs chunked top scores rel_err %.3g' % err)
    assert err < U.TOL
    r0, r1 = rank0.cpu().numpy(), rank1.cpu().numpy()
    assert (r0 > 0).all()
    flagged = np.array([band[b, r - 1] for b, r in enumerate(r0)])
    print('validation: %d of %d entries have their target in a band' % (int(flagged.sum()), len(r0)))
    assert np.array_equal(r0[~flagged], r1[~flagged])
    args.rtm_rank_all = False
    v0 = tr.validate(args, gd, ds)
    args.rtm_rank_all = True
    v1 = tr.validate(args, gd, ds)
    assert v0 == evaluate.calc_metrics(rank0, 100) and v1 == evaluate.calc_metrics(rank1, 100)
    assert evaluate.calc_metrics(torch.from_numpy(np.where(flagged, r0, r1)), 100) == v0
    if not flagged.any():
        assert v0 == v1
    # ---- the test over all products, with its ranklist
    ds_t = corpus.ProdSearchDataset(args, gd, test_pd)
    args.rtm_rank_all = False
    t_rank0, t_ids0, t_sc0, t_users0, t_queries0 = tr._scores_candidates(args, ds_t, P, topk=P)
    args.rtm_rank_all = True
    t_rank1, t_ids1, t_sc1, t_users1, t_queries1 = tr._scores_rank_seq_rtm(args, gd, ds_t, P, False)
    assert t_users0 == t_users1 and t_queries0 == t_queries1
    t_sc0, t_ids0, t_ids1 = t_sc0.cpu().numpy(), t_ids0.cpu().numpy(), t_ids1.cpu().numpy()
    t_band = _bands_of(t_sc0)
    assert np.array_equal(t_ids1[~t_band], t_ids0[~t_band])
    t_r0, t_r1 = t_rank0.cpu().numpy(), t_rank1.cpu().numpy()
    t_flag = np.array([t_band[b, r - 1] for b, r in enumerate(t_r0)])
    print('test: %d of %d entries have their target in a band; %.3f of the positions banded'
          % (int(t_flag.sum()), len(t_r0), float(t_band.mean())))
    assert np.array_equal(t_r0[~t_flag], t_r1[~t_flag])
    args.rtm_rank_all = False
    m0 = tr.test(args, gd, test_pd, 'chunked.ranklist')
    args.rtm_rank_all = True
    m1 = tr.test(args, gd, test_pd, 'one_pass.ranklist')
    assert m0 == evaluate.calc_metrics(t_rank0, 100) and m1 == evaluate.calc_metrics(t_rank1, 100)
    assert evaluate.calc_metrics(torch.from_numpy(np.where(t_flag, t_r0, t_r1)), 100) == m0
    if not t_flag.any():
        assert m0 == m1
    l0 = open(os.path.join(args.save_dir, 'chunked.ranklist')).read().splitlines()
    l1 = open(os.path.join(args.save_dir, 'one_pass.ranklist')).read().splitlines()
    assert len(l0) == len(l1) == len(t_r0) * min(100, P)
    keep = ~t_band[:, :min(100, P)].reshape(-1)
    pick = lambda ls: [ln.split(' ')[:4] for ln, k in zip(ls, keep) if k]
    assert pick(l0) == pick(l1)
    # the static rankers' routes still refuse the mode
    with pytest.raises(NotImplementedError, match='do_seq_review_test'):
        tr._scores_rank_all_rtm(args, gd, ds_t, 10)
