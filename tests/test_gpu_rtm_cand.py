"""``evaluate.rank_candidates_rtm`` on an MI355X: the review transformer over every entry's own candidate
list in one pass, against ``oracle.rtm.rtm_test`` over the chunk assembled from the same entries, catalogue and lists
(tests/rtm_cand_util.py), against the GPU's own ``model.test()`` on that chunk, and bit for bit against
``evaluate.rank_all_rtm`` at the listed (entry, item) pairs.  Bounds: the suite's eval bound, rel_err < 1e-4, over the live
slots, and per entry against the float64 oracle 8 x what fp32 costs the case's listed pairs on the host (K.YARDSTICK / K.bound).
Every case asserts from ``ps_rtm_rank_cand_plan`` the fields it was written for before it compares anything, and every figure
is printed before it is asserted.

Measured on an MI355X (DESIGN.md §8b.2's table): worst entry 1.6e-7 .. 5.0e-6 under bounds of 2.4e-6 .. 2.5e-5; every live
slot of every case bit-equal to ``rank_all_rtm``'s score of the same pair."""
import functools
import os

import numpy as np
import pytest
import torch

import rtm_cand_util as K
import rtm_rank_util as U
from golden_util import rel_err

pytestmark = pytest.mark.gpu

KTOP = 10
# model.test() refuses two of the cases: lds_full's 129-position sequences (ps_rtm_score serves at most 64) and heads1_d128's
# head width (the chunked encoder serves d / heads <= 64, csrc/encoder.hip's descriptor check) — as tests/test_gpu_rtm_rank.py found
NO_MODEL_TEST = ('lds_full', 'heads1_d128')


def oracle_lists(c, sd, cands, f64=False):
    """[B, C] scores of ``oracle.rtm.rtm_test`` over ``assemble_chunk(..., cands, limit=c.T)``; -inf at dead slots."""
    from oracle import rtm as ortm
    P = {k: (v.double() if f64 and v.dtype.is_floating_point else v) for k, v in sd.items()}
    rev = ortm.rtm_review_embeddings(P, c.a, c.rw, c.V)
    s = ortm.rtm_test(P, c.a, K.chunk_of(c, cands), rev, c.V, c.RC)
    return s.masked_fill(~torch.from_numpy(K.live_of(cands, c.P)), float('-inf'))


@functools.lru_cache(maxsize=None)
def run(name):
    """One case, computed once: the oracle's scores of the lists (fp32 and float64), the plan of the call, the GPU's (dense,
    top-k, rank), and ``rank_all_rtm``'s dense catalogue scores from the same index."""
    from prodsearch_amd import _lib, evaluate
    kw = K.CASES[name]
    c, _, scale = U.case_of(kw['data'])
    cands = K.make_cands(c, kw.get('C', 12), kw.get('seed', 101))
    cpp = kw.get('cpp')
    m, sd = U.build_model(c, 'cuda', scale=scale)
    ref, ref64 = oracle_lists(c, sd, cands), oracle_lists(c, sd, cands, f64=True)
    plan = K.plan_of(_lib.load(), m, c, cands.shape[1], KTOP, cpp)
    up = c.review_u_p.cuda() if (c.a.use_user_emb or c.a.use_item_emb) else None
    index = m.catalogue_index(c.item_r.cuda(), up)
    rb = K.rank_batch(c, cands, 'cuda')
    top_idx, top_score, rank, scores = evaluate.rank_candidates_rtm(m, index, rb, KTOP, cands_per_pass=cpp, return_scores=True)
    full = evaluate.rank_all_rtm(m, index, rb, KTOP, return_scores=True)[3]
    torch.cuda.synchronize()
    return dict(c=c, m=m, sd=sd, cands=cands, cpp=cpp, ref=ref, ref64=ref64, plan=plan, index=index, rb=rb, top_idx=top_idx.cpu(),
                top_score=top_score.cpu(), rank=rank.cpu(), scores=scores.cpu(), full=full.cpu())


def check_order(ref, cands, P, top_idx, rank, target, k, what):
    """``top_idx`` against the oracle's order of every list wherever the oracle's gap to the neighbouring score exceeds
    2 * tol * max|score| (inside such a band positions may swap); at most a quarter of the positions may lie in a band.
    ``rank`` the same way, by the FIRST live column that holds the target."""
    orders, bands, frac = K.list_bands(ref, cands, P)
    assert frac <= K.BAND_CAP, (what, frac)
    n_banded = 0
    for b, t in enumerate(target.tolist()):
        cols, band = orders[b], bands[b]
        kk = min(k, len(cols))
        free = ~band[:kk]
        assert np.array_equal(top_idx[b, :kk].numpy()[free], cands[b, cols[:kk]][free]), (what, b)
        hit = [col for col in range(cands.shape[1]) if cands[b, col] == t and 0 <= t < P]
        if not hit:
            assert int(rank[b]) == 0, (what, b)
            continue
        pos = int(np.flatnonzero(cols == hit[0])[0])
        if band[pos]:
            n_banded += 1
            lo, hi = pos, pos
            while lo > 0 and band[lo - 1]:
                lo -= 1
            while hi < len(cols) - 1 and band[hi + 1]:
                hi += 1
            assert lo + 1 <= int(rank[b]) <= hi + 1, (what, b)
        else:
            assert int(rank[b]) == pos + 1, (what, b, int(rank[b]), pos + 1)
    return frac, n_banded


@pytest.mark.parametrize('name', sorted(K.CASES))
def test_scores_topk_rank_against_the_oracle_and_the_catalogue_pass(name):
    """(a) the dense scores against the fp32 oracle at TOL, dead slots -inf; (b) per entry against the float64 oracle within
    min(8 x yardstick, TOL); (d) every live slot bit-equal to ``rank_all_rtm``'s score of the same (entry, item); (e) top-k and
    rank exactly the stated semantics on the GPU's own scores, and the oracle's order outside bands."""
    r = run(name)
    c, cands = r['c'], r['cands']
    print('%s: plan %s' % (name, r['plan']))
    for f, v in K.PLAN[name].items():
        assert r['plan'][f] == v, (name, f, r['plan'][f], v)
    live = torch.from_numpy(K.live_of(cands, c.P))
    s = r['scores']
    assert torch.isneginf(s[~live]).all() and torch.isfinite(s[live]).all()
    err = rel_err(s[live], r['ref'][live])
    print('%s: rank_candidates_rtm vs rtm_test rel_err %.3g over %d live slots' % (name, err, int(live.sum())))
    assert err < K.TOL
    e = K.list_err(s, r['ref64'], cands, c.P)
    print('%s: vs the float64 rtm_test, worst entry %.3g (yardstick %.3g, bound %.3g)' % (name, e.max(), K.YARDSTICK[name], K.bound(name)))
    assert (e < K.bound(name)).all(), (name, e.tolist(), K.bound(name))
    same = K.take(r['full'], cands, c.P)
    n_diff = int((same[live] != s[live]).sum())
    print('%s: %d of %d live slots differ in some bit from rank_all_rtm' % (name, n_diff, int(live.sum())))
    assert torch.equal(same[live], s[live])
    ti, ts, rk = K.semantics(s.numpy(), cands, c.target.numpy(), c.P, KTOP)
    assert np.array_equal(r['top_idx'].numpy(), ti)
    assert np.array_equal(r['top_score'].numpy(), ts)
    assert np.array_equal(r['rank'].numpy().astype(np.int64), rk)
    frac, nb = check_order(r['ref'], cands, c.P, r['top_idx'], r['rank'], c.target, KTOP, name)
    print('%s: %.3f of the listed positions in a band, %d targets in one' % (name, frac, nb))


@pytest.mark.parametrize('name', sorted(n for n in K.CASES if n not in NO_MODEL_TEST))
def test_scores_against_the_gpus_own_test(name):
    """(c) ``model.test()`` — the existing, parity-checked path — on the same chunk."""
    r = run(name)
    c, m, cands = r['c'], r['m'], r['cands']
    with torch.no_grad():
        m.get_review_embeddings()
        got = m.test(K.chunk_of(c, cands).to('cuda')).cpu()
    live = torch.from_numpy(K.live_of(cands, c.P))
    err = rel_err(r['scores'][live], got[live])
    print('%s: rank_candidates_rtm vs model.test() rel_err %.3g' % (name, err))
    assert err < K.TOL


@pytest.mark.parametrize('name', ['base', 'passes', 'lds_full'])
def test_special_slots(name):
    """(f) the shared-list pair is bit-equal and in column order; the duplicated target ranks by its first column; the slot past
    the catalogue and the -1 slot are absent from ``top_idx``; an absent or out-of-range target gives rank 0; ``topk`` above the
    live count leaves -1 / -inf."""
    from prodsearch_amd import evaluate
    r = run(name)
    c, cands, s = r['c'], r['cands'], r['scores']
    C = cands.shape[1]
    assert s[0, 2] == s[0, 3]
    k = C + 8
    ti, ts, rk = (t.cpu() for t in evaluate.rank_candidates_rtm(r['m'], r['index'], r['rb'], k, cands_per_pass=r['cpp']))
    e_ti, e_ts, e_rk = K.semantics(s.numpy(), cands, c.target.numpy(), c.P, k)
    assert np.array_equal(ti.numpy(), e_ti) and np.array_equal(ts.numpy(), e_ts) and np.array_equal(rk.numpy().astype(np.int64), e_rk)
    assert torch.equal(rk, r['rank'])
    # entry 0 lists item 2 at column 2 and item 3 at column 3 (and nowhere before): 3 follows 2 at once
    row = ti[0].tolist()
    assert row.index(3) == row.index(2) + 1
    # entry 1: its target at columns 2 and 7, a dead id at 4, -1 at 5
    n_live = int(K.live_of(cands, c.P)[1].sum())
    assert n_live == C - 2 and (ti[1, n_live:] == -1).all() and torch.isneginf(ts[1, n_live:]).all()
    assert c.P + 3 not in ti[1].tolist() and (ti[1, :n_live] >= 0).all()
    t1 = int(c.target[1])
    assert (ti[1] == t1).sum() == int((cands[1] == t1).sum()) >= 2          # duplicates are slots of their own
    assert s[1, 2] == s[1, 7]
    ahead = int(((s[1] > s[1, 2]) | ((s[1] == s[1, 2]) & (torch.arange(C) < 2))).sum())
    assert int(rk[1]) == 1 + ahead
    assert int(rk[-1]) == 0                                                  # a target outside [0, P)
    # a target inside the catalogue but not in the list: rank 0 as well
    absent = next(i for i in range(c.P) if i not in cands[2].tolist())
    tg = c.target.clone()
    tg[2] = absent
    from prodsearch_amd import rtm_data
    rb = rtm_data.ProdSearchRankBatch(list(range(c.B)), [int(u) for u in c.users], tg, c.qw, c.u_r, torch.from_numpy(cands)).to('cuda')
    rk2 = evaluate.rank_candidates_rtm(r['m'], r['index'], rb, KTOP, cands_per_pass=r['cpp'])[2].cpu()
    assert int(rk2[2]) == 0 and torch.equal(rk2[[0, 1]], r['rank'][[0, 1]])


def test_passes_do_not_change_a_bit():
    """(g) C = 12 in passes of 5 (the last ragged, run at the full pass shape) against the single pass."""
    one, many = run('base'), run('passes')
    assert one['plan']['passes'] == 1 and many['plan']['passes'] == 3
    assert np.array_equal(one['cands'], many['cands'])
    for f in ('scores', 'top_idx', 'top_score', 'rank'):
        assert torch.equal(one[f], many[f]), f


def test_stale_index_is_refused_and_a_rebuilt_one_serves():
    """(h) a weight edited in place after the index was built."""
    from prodsearch_amd import evaluate
    c = U.make_case()
    cands = K.make_cands(c)
    m, _ = U.build_model(c, 'cuda')
    index = m.catalogue_index(c.item_r.cuda())
    rb = K.rank_batch(c, cands, 'cuda')
    before = evaluate.rank_candidates_rtm(m, index, rb, KTOP, return_scores=True)[3].cpu()
    with torch.no_grad():
        m._named_hot_params()[0][1].mul_(1.0)
    with pytest.raises(RuntimeError, match='stale'):
        evaluate.rank_candidates_rtm(m, index, rb, KTOP)
    again = m.catalogue_index(index.item_ridxs)
    assert again is not index
    after = evaluate.rank_candidates_rtm(m, again, rb, KTOP, return_scores=True)[3].cpu()
    assert torch.equal(before, after)


def _bands_of(sc):
    close = np.abs(np.diff(sc, axis=1)) <= 2 * U.TOL * np.abs(sc[np.isfinite(sc)]).max()
    band = np.zeros_like(sc, dtype=bool)
    band[:, :-1] |= close
    band[:, 1:] |= close
    return band


def test_trainer_takes_the_list_pass_behind_its_flag(tmp_path):
    """(i) ``args.rtm_rank_all`` with candidate lists: validation on ``valid_candi_size = 7`` sampled products in chunks of 3
    and the rerank of ``test_candi_size = 7`` ranklist candidates give the default chunked path's users, queries, ids and ranks;
    entries whose target sits in a band of the default path's own scores may differ in rank; printed."""
    from prodsearch_amd import default_args, synth, trainer, corpus, pyrandom, evaluate
    data_path, inp = synth.write_corpus(str(tmp_path / 'c'), 33, n_users=50, n_products=40, n_words=150)
    args = default_args(model_name='review_transformer', review_encoder_name='pvc', embedding_size=64, ff_size=128, heads=8,
                        inter_layers=1, uprev_review_limit=4, iprev_review_limit=6, review_word_limit=16, subsampling_rate=1e-1,
                        candi_batch_size=3, test_candi_size=7, valid_candi_size=7, valid_batch_size=12, data_dir=data_path,
                        input_train_dir=inp, save_dir=str(tmp_path / 'r'), device='cuda', dropout=0.0)
    os.makedirs(args.save_dir)
    args.start_epoch = 0
    torch.manual_seed(1); pyrandom.seed(1); np.random.seed(1)
    gd = corpus.GlobalProdSearchData(args, data_path, inp)
    train_pd = corpus.ProdSearchData(args, inp, 'train', gd)
    valid_pd = corpus.ProdSearchData(args, inp, 'valid', gd)
    model, _ = trainer.create_model(args, gd, train_pd)
    tr = trainer.Trainer(args, model, None)
    P = gd.product_size
    # ---- validation lists: the dataset draws them once; both paths read the same dataset
    ds = corpus.ProdSearchDataset(args, gd, valid_pd)
    rank0, ids0, sc0, users0, queries0 = tr._scores_candidates(args, ds, 7, topk=7)
    args.rtm_rank_all = True
    rank1, ids1, sc1, users1, queries1 = tr._scores_rank_cand_rtm(args, gd, ds, 7)
    assert users0 == users1 and queries0 == queries1 and len(users0) * 3 == len(ds)
    sc0, ids0, ids1 = sc0.cpu().numpy(), ids0.cpu().numpy(), ids1.cpu().numpy()
    band = _bands_of(sc0)
    assert ids0.shape == ids1.shape and np.array_equal(ids1[~band], ids0[~band])
    r0, r1 = rank0.cpu().numpy(), rank1.cpu().numpy()
    assert (r0 > 0).all()                                                   # validation lists hold their target
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
    # ---- the rerank: a ranklist of 7 candidates per (user, query), the target among them for two entries of three
    probe = corpus.ProdSearchData(args, inp, 'test', gd)                    # (no ranklist file yet: uq_pids is None)
    assert probe.uq_pids is None
    rng = synth.rng_for(7)
    seen, lines = set(), []
    for _, user, prod, _ in probe.review_info:
        for q in probe.product_query_idx[prod]:
            if (user, q) in seen:
                continue
            seen.add((user, q))
            cand = [int(x) for x in rng.choice(P, size=7, replace=False)]
            if len(seen) % 3 and prod not in cand:
                cand[int(rng.integers(0, 7))] = int(prod)
            lines += ['%s_%d Q0 %s %d 0.0 x\n' % (gd.user_ids[user], q, gd.product_ids[p], j + 1) for j, p in enumerate(cand)]
    with open(os.path.join(inp, 'test.bias_product.ranklist'), 'w') as f:
        f.writelines(lines)

    def test_with(flag, fname):
        """(the dataset shuffles the ranklist's lists in place with the python generator: a fresh read and seed per run)"""
        pyrandom.seed(5)
        pd = corpus.ProdSearchData(args, inp, 'test', gd)
        assert pd.uq_pids is not None
        args.rtm_rank_all = flag
        return tr.test(args, gd, pd, fname), pd

    (m0, pd0), (m1, _) = test_with(False, 'chunked.ranklist'), test_with(True, 'one_pass.ranklist')
    pyrandom.seed(5)
    ds_t = corpus.ProdSearchDataset(args, gd, corpus.ProdSearchData(args, inp, 'test', gd))
    args.rtm_rank_all = False
    t_rank0, _, t_sc0, _, _ = tr._scores_candidates(args, ds_t, 7, topk=7)
    args.rtm_rank_all = True
    t_rank1 = tr._scores_rank_cand_rtm(args, gd, ds_t, 7)[0]
    assert m0 == evaluate.calc_metrics(t_rank0, 100) and m1 == evaluate.calc_metrics(t_rank1, 100)
    t_sc0, t_r0, t_r1 = t_sc0.cpu().numpy(), t_rank0.cpu().numpy(), t_rank1.cpu().numpy()
    assert (t_r0 == 0).any() and (t_r0 > 0).any()                           # lists with and without their target
    t_band = _bands_of(t_sc0)
    t_flag = np.array([r > 0 and t_band[b, r - 1] for b, r in enumerate(t_r0)])
    print('rerank: %d of %d entries have their target in a band' % (int(t_flag.sum()), len(t_r0)))
    assert np.array_equal(t_r0[~t_flag], t_r1[~t_flag])
    assert evaluate.calc_metrics(torch.from_numpy(np.where(t_flag, t_r0, t_r1)), 100) == m0
    l0 = open(os.path.join(args.save_dir, 'chunked.ranklist')).read().splitlines()
    l1 = open(os.path.join(args.save_dir, 'one_pass.ranklist')).read().splitlines()
    assert len(l0) == len(l1) == len(t_r0) * 7
    keep = ~t_band.reshape(-1)
    pick = lambda ls: [ln.split(' ')[:4] for ln, k in zip(ls, keep) if k]
    assert pick(l0) == pick(l1)
