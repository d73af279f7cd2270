"""GPU checks of the review transformer's row-sparse optimizer path (``args.row_sparse_adam`` on ``ProductRanker``):
``ps_coalesce_tables`` against numpy and ``ps_coalesce_rows`` bit for bit, training parity with the oracle's row-sparse
``ClipAdam(touched=)`` on the dropout-free (and one Philox-masked) fixtures, the lazy rule for rows a step did not address,
``zero_grad`` handling, a table frozen between steps, and a trainer run with a checkpoint that continues bit for bit."""
import copy
import os

import numpy as np
import pytest
import torch

from golden_util import rel_err
from golden_util_rtm import RtmGolden

pytestmark = pytest.mark.gpu

USER_SIZE, PRODUCT_SIZE = 40, 50                # tests/golden/make_golden_rtm.py
REVIEW, USER, ITEM, WORD = ('review_encoder.review_embeddings.weight', 'user_emb.weight', 'product_emb.weight',
                            'word_embeddings.weight')


# ------------------------------------------------------------------------------------------------ ps_coalesce_tables
N_ROWS = (70, 1001, 16385, 131072)              # one bitmap block = 256 words x 64 rows = 16,384 rows: 16,385 is on two
SIZES = ((500,), (64, 320, 1280), (384, 7680, 7680), (0, 17, 900))


def _lists(seed, n_rows, sizes, mode):
    """mode 'live': random ids, 20 % pad, ids 0 / 63 / 64 / n_rows - 2 present; 'empty': only empty lists; 'pad': all pad."""
    rng = np.random.default_rng(seed)
    pad = n_rows - 1
    out = []
    for s in sizes:
        if mode == 'empty':
            out.append(np.zeros(0, np.int64))
            continue
        x = rng.integers(0, n_rows, size=s)
        x[rng.random(s) < 0.2] = pad
        if mode == 'pad':
            x[:] = pad
        out.append(x.astype(np.int64))
    if mode == 'live':
        big = max(range(len(out)), key=lambda i: out[i].size)
        out[big][:4] = [0, n_rows - 2, 63, 64]                  # word boundaries, last real row
    return out


def _want(lists, pad):
    u = np.unique(np.concatenate(lists)) if lists else np.zeros(0, np.int64)
    return u[u != pad]


class _Tables(object):
    """Device state of one ``ps_coalesce_tables`` problem: per table its workspace, rows_out (pre-filled with -7), count."""

    def __init__(self, n_rows_all):
        from prodsearch_amd import _lib
        self.lib = _lib.load()
        self.n_rows = n_rows_all
        self.ws = [torch.zeros(self.lib.ps_coalesce_ws_bytes(n), dtype=torch.uint8, device='cuda') for n in n_rows_all]

    def run(self, lists_all, caps=None, expect_rc=0):
        from prodsearch_amd import _lib
        ts_all = [[torch.as_tensor(x, dtype=torch.int64, device='cuda') for x in ls] for ls in lists_all]
        tabs = (_lib.PsCoalesceTable * len(ts_all))()
        self.rows, self.count = [], []
        for k, (t, ts, n) in enumerate(zip(tabs, ts_all, self.n_rows)):
            total = sum(x.numel() for x in ts)
            cap = max(1, min(total, n)) if caps is None else caps[k]
            self.rows.append(torch.full((max(1, cap),), -7, dtype=torch.int64, device='cuda'))
            self.count.append(torch.full((1,), -7, dtype=torch.int32, device='cuda'))
            for i, x in enumerate(ts):
                t.lists[i].idx, t.lists[i].n = x.data_ptr(), x.numel()
            t.n_lists, t.n_rows, t.pad_row = len(ts), n, n - 1
            t.ws_dev, t.rows_out_dev, t.cap, t.count_out_dev = self.ws[k].data_ptr(), self.rows[k].data_ptr(), cap, \
                self.count[k].data_ptr()
        rc = self.lib.ps_coalesce_tables(tabs, len(ts_all), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (rc != 0) == (expect_rc != 0), self.lib.ps_last_error()
        return [r[:int(c[0])].cpu().numpy() for r, c in zip(self.rows, self.count)] if rc == 0 else None

    def flag(self, k, clear=False):
        addr = self.lib.ps_coalesce_bad_flag(self.ws[k].data_ptr(), self.n_rows[k])
        off = addr - self.ws[k].data_ptr()
        v = int(self.ws[k][off:off + 4].view(torch.int32)[0])
        if clear:
            self.ws[k][off:off + 4].zero_()
        return v

    def bitmap_sum(self, k):
        return int(self.ws[k][:8 * ((self.n_rows[k] + 63) // 64)].to(torch.int32).sum())


def _single(lists, n_rows):
    """``ps_coalesce_rows`` on the same lists, on a workspace of its own."""
    from prodsearch_amd import _lib
    lib = _lib.load()
    ts = [torch.as_tensor(x, dtype=torch.int64, device='cuda') for x in lists]
    cap = max(1, min(sum(t.numel() for t in ts), n_rows))
    ws = torch.zeros(lib.ps_coalesce_ws_bytes(n_rows), dtype=torch.uint8, device='cuda')
    rows = torch.full((cap,), -7, dtype=torch.int64, device='cuda')
    count = torch.zeros(1, dtype=torch.int32, device='cuda')
    arr = (_lib.PsIdxList * len(ts))()
    for i, t in enumerate(ts):
        arr[i].idx, arr[i].n = t.data_ptr(), t.numel()
    _lib.check(lib.ps_coalesce_rows(arr, len(ts), n_rows, n_rows - 1, ws.data_ptr(), rows.data_ptr(), cap, count.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), 'ps_coalesce_rows')
    torch.cuda.synchronize()
    return rows[:int(count[0])].cpu().numpy()


@pytest.mark.parametrize('modes', [('live', 'live', 'live', 'live'), ('empty', 'live', 'pad', 'live'),
                                   ('live', 'pad', 'empty', 'live'), ('live', 'live', 'live', 'empty')])
def test_coalesce_tables_equals_numpy_and_the_single_table_call(modes):
    lists_all = [_lists(11 + k, n, s, mode) for k, (n, s, mode) in enumerate(zip(N_ROWS, SIZES, modes))]
    T = _Tables(N_ROWS)
    got = T.run(lists_all)
    for k, (ls, n) in enumerate(zip(lists_all, N_ROWS)):
        want = _want(ls, n - 1)
        assert np.array_equal(got[k], want), (k, modes[k])                      # bit-exact index work
        assert np.array_equal(got[k], _single(ls, n)), (k, modes[k])            # ... and ps_coalesce_rows' own answer
        assert (want.size == 0) == (modes[k] != 'live')
        if modes[k] == 'live':
            assert {0, 63, 64, n - 2} <= set(want.tolist())
        assert T.flag(k) == 0 and T.bitmap_sum(k) == 0                          # bitmap left clean
        assert int(T.rows[k][got[k].size:].ne(-7).sum()) == 0                   # nothing written past the count
    got2 = T.run([ls[::-1] for ls in lists_all])                                # same workspaces, the lists reversed
    for k in range(4):
        assert np.array_equal(got2[k], got[k]), k
        assert T.flag(k) == 0 and T.bitmap_sum(k) == 0


@pytest.mark.parametrize('n_tabs', [1, 2, 3])
def test_coalesce_tables_with_fewer_tables(n_tabs):
    order = (2, 0, 3)[:n_tabs]                                                  # the two-block table first
    lists_all = [_lists(31 + k, N_ROWS[k], SIZES[k], 'live') for k in order]
    got = _Tables([N_ROWS[k] for k in order]).run(lists_all)
    for g, ls, k in zip(got, lists_all, order):
        assert np.array_equal(g, _want(ls, N_ROWS[k] - 1)), k


def test_coalesce_tables_status_word_is_per_table():
    lists_all = [_lists(51 + k, n, s, 'live') for k, (n, s) in enumerate(zip(N_ROWS, SIZES))]
    T = _Tables(N_ROWS)
    clean = T.run(lists_all)
    bad = [list(ls) for ls in lists_all]
    bad[1][1] = bad[1][1].copy()
    bad[1][1][5:9] = [N_ROWS[1], 10_000_000, -2, N_ROWS[1] + 63]                # outside [0, n_rows): dropped, flagged
    got = T.run(bad)
    assert [T.flag(k) for k in range(4)] == [0, 1, 0, 0]
    for k in range(4):
        want = _want(bad[k], N_ROWS[k] - 1)
        assert np.array_equal(got[k], want[(want >= 0) & (want < N_ROWS[k])]), k   # the stray ids dropped, nothing else
        if k != 1:
            assert np.array_equal(got[k], clean[k]), k
        assert T.bitmap_sum(k) == 0
    assert T.flag(1, clear=True) == 1 and T.flag(1) == 0
    # a capacity one short of min(total, n_rows), in a call of its own, is refused on the host before anything is launched
    # (the number of unique rows can never exceed that minimum, so the kernels' own overflow word — 2 — cannot be reached
    # through a call the entry accepts): error code, message, buffers untouched
    total1 = sum(x.size for x in lists_all[1])
    caps = [max(1, min(sum(x.size for x in ls), n)) for ls, n in zip(lists_all, N_ROWS)]
    caps[1] = min(total1, N_ROWS[1]) - 1
    assert T.run(lists_all, caps=caps, expect_rc=1) is None
    assert b'table 1: rows_out capacity' in T.lib.ps_last_error()
    assert all(int(c[0]) == -7 for c in T.count) and all(T.flag(k) == 0 and T.bitmap_sum(k) == 0 for k in range(4))


# --------------------------------------------------------------------------------------------------- training parity
def _args(g, **over):
    a = copy.copy(g.args)
    a.row_sparse_adam = True
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _model(g, a):
    from prodsearch_amd.ps_model import ProductRanker
    torch.manual_seed(0)
    m = ProductRanker(a, 'cuda', g.V, g.RC, PRODUCT_SIZE, USER_SIZE, g.review_words, None, word_dists=g.word_dists)
    m.load_state_dict(g.params(), strict=False)
    m.train()
    return m


def _neg(g, step):
    nw = g.neg_words(step % g.steps)
    return nw


def _touched_np(g, batch, nw):
    """numpy's sorted unique non-pad ids of the lists DESIGN.md 5b names, per sparse table of the fixture's configuration."""
    a = g.args
    uniq = lambda ls, pad: np.setdiff1d(np.unique(np.concatenate([np.asarray(x).ravel() for x in ls])), [pad])
    out = {}
    if a.review_encoder_name == 'pv':
        out[REVIEW] = uniq([batch.pos_prod_ridxs, batch.neg_prod_ridxs], g.RC - 1)
        words = [batch.query_word_idxs] + ([batch.pos_prod_rword_idxs, nw] if g.train_pv else [])
        out[WORD] = uniq(words, g.V - 1)
    if getattr(a, 'use_user_emb', False):
        out[USER] = uniq([batch.pos_user_idxs, batch.neg_user_idxs], USER_SIZE)
    if getattr(a, 'use_item_emb', False):
        out[ITEM] = uniq([batch.pos_item_idxs, batch.neg_item_idxs], PRODUCT_SIZE)
    return out


def _oracle_pad(g):
    return {WORD: g.V - 1, 'seg_embeddings.weight': 3, REVIEW: g.RC - 1, USER: USER_SIZE, ITEM: PRODUCT_SIZE}


def _oracle_forward(g, P, batch, nw, step):
    from oracle import rtm as ortm
    gen = g.dropout(step)                        # the product's Philox masks at forward #(step + 1)
    drop = gen if (gen is not None and g.args.dropout > 0) else None
    tok = gen.tok if (gen is not None and gen.corrupt_rate > 0) else None
    return ortm.rtm_forward(P, g.args, batch, nw, g.V, g.RC, training=True, train_pv=g.train_pv, drop=drop, tok_drop=tok)[0]


def _cuda(t):
    return None if t is None else t.cuda()


def _check_params(m, P, init, touched_ever, a, step):
    """The bounds of tests/test_gpu_rowsparse.py::test_rowsparse_training_matches_oracle, unchanged."""
    sd = m.state_dict()
    for n in P:
        got, ref = sd[n].cpu(), P[n].detach()
        if n.endswith('linear_keys.bias'):
            assert float((got - ref).abs().max()) <= 2.01 * a.lr * (step + 1), (step, n)
            continue
        if n in touched_ever:                               # rows the optimizer moved = touched rows, exactly
            assert torch.equal((got != init[n]).any(1), (ref != init[n]).any(1)), (step, n)
            never = torch.ones(got.shape[0], dtype=torch.bool)
            never[torch.as_tensor(touched_ever[n], dtype=torch.int64)] = False
            assert torch.equal(got[never], init[n][never]), (step, n)      # a row no step addressed stands still, bit for bit
        assert float((got - ref).abs().max()) < 2e-3 * float(ref.abs().max()) + 0.02 * a.lr * (step + 1), (step, n)
        assert rel_err(got - init[n], ref - init[n]) < 1e-1, (step, n)


@pytest.mark.parametrize('case', ['rtm_pv', 'rtm_pv_user', 'rtm_pv_ui', 'rtm_pvc_item', 'rtm_pv_notrain'])
def test_rtm_rowsparse_training_matches_oracle(case):
    """trainer.py:74-79 order with args.row_sparse_adam: touched lists bit-exact, touched gradient rows zeroed by the step,
    the rows that moved = the touched rows, parameters / loss / clip norm within the item models' bounds of the oracle's
    row-sparse ClipAdam driven by the oracle's own gradients.  (rtm_pvc_item draws dropout and token corruption: the oracle
    runs on the product's own Philox masks, as tests/test_gpu_parity_rtm.py does.)  Once per fixture a dense twin takes the
    same step: a table row with a nonzero dense gradient that is missing from the touched list is a forgotten index list."""
    from oracle import optim as ooptim
    from oracle.tem import grads_of
    from prodsearch_amd import build_optim
    g = RtmGolden(case)
    a = _args(g)
    m = _model(g, a)
    optim = build_optim(a, m, None)
    assert optim.row_sparse and m._row_sparse()
    P = {k: v.clone().requires_grad_(True) for k, v in g.params().items()}
    init = {k: v.detach().clone() for k, v in P.items()}
    opt = ooptim.ClipAdam(a.lr, a.max_grad_norm, a.beta1, a.beta2, 1e-9, a.l2_lambda, a.decay_method, a.warmup_steps)
    batch = g.batch()
    b = batch.to('cuda')
    touched_ever = {}
    for step in range(max(3, g.steps)):
        nw = _neg(g, step)
        loss = m(b, train_pv=g.train_pv, neg_word_idxs=_cuda(nw))
        m.zero_grad()
        loss.backward()
        touched = _touched_np(g, batch, nw)
        got_t = m.touched_rows()
        assert sorted(got_t) == sorted(touched)
        for n in touched:
            assert np.array_equal(got_t[n].cpu().numpy(), touched[n]), (step, n)      # bit-exact index work
            touched_ever[n] = np.union1d(touched_ever.get(n, np.zeros(0, np.int64)), touched[n])
        if step == 0:
            dense = _model(g, _args(g, row_sparse_adam=False))
            dl = dense(b, train_pv=g.train_pv, neg_word_idxs=_cuda(nw))
            dense.zero_grad()
            dl.backward()
            torch.cuda.synchronize()
            assert float(dl.detach()) == pytest.approx(float(loss.detach()), rel=1e-5)
            for n, p in dense.named_parameters():
                if n in touched:
                    hot = torch.nonzero(p.grad.ne(0).any(1)).flatten().cpu().numpy()
                    assert hot.size > 0 and np.isin(hot, touched[n]).all(), (n, np.setdiff1d(hot, touched[n]))
            for n, p in m.named_parameters():                   # the same gradients as the dense twin's
                if p.grad is not None and not n.endswith('linear_keys.bias'):
                    assert rel_err(p.grad.cpu(), dict(dense.named_parameters())[n].grad.cpu()) < 2e-4, n
            del dense
        optim.step()
        in_rows = {id(p) for p, _ in optim._plan['rows']}
        assert {n for n, p in m.named_parameters() if id(p) in in_rows} == set(touched)
        for n, p in m.named_parameters():                       # touched gradient rows come back zeroed
            if n in touched:
                assert float(p.grad.abs().max()) == 0, (step, n)
        oloss = _oracle_forward(g, P, batch, nw, step)
        assert rel_err(loss.detach().cpu(), oloss.detach()) < 2e-4, step
        grads = grads_of(oloss, P, _oracle_pad(g))
        with torch.no_grad():
            opt.step(P, grads, touched=touched)
        assert abs(optim.last_grad_norm - opt.last_total_norm) < 1e-3 * opt.last_total_norm
        _check_params(m, P, init, touched_ever, a, step)
    m.check_index_errors()


# ------------------------------------------------------------------------------------------------------ the lazy rule
def _neighbours(t, pad):
    """Every live id moved to a neighbour id (never onto the pad row, never off the table)."""
    t = t.clone()
    live = t.ne(pad)
    up = live & (t + 1).lt(pad)
    t[up] += 1
    t[live & ~up] -= 1
    return t


def test_rows_a_step_does_not_address_keep_their_moments():
    from oracle import optim as ooptim
    from oracle.tem import grads_of
    from prodsearch_amd import build_optim
    g = RtmGolden('rtm_pv_ui')
    a = _args(g)
    m = _model(g, a)
    optim = build_optim(a, m, None)
    b1 = g.batch()
    b2 = copy.copy(b1)
    for names, pad in ((('pos_prod_ridxs', 'neg_prod_ridxs'), g.RC - 1), (('pos_user_idxs', 'neg_user_idxs'), USER_SIZE),
                       (('pos_item_idxs', 'neg_item_idxs'), PRODUCT_SIZE)):
        for n in names:
            setattr(b2, n, _neighbours(getattr(b1, n), pad))
    P = {k: v.clone().requires_grad_(True) for k, v in g.params().items()}
    init = {k: v.detach().clone() for k, v in P.items()}
    opt = ooptim.ClipAdam(a.lr, a.max_grad_norm, a.beta1, a.beta2, 1e-9, a.l2_lambda, a.decay_method, a.warmup_steps)
    names = [n for n, p in m.named_parameters() if p.requires_grad]              # the checkpoint's parameter order
    touched, states, ostates = [], [], []
    for step, batch in enumerate((b1, b2)):
        nw = _neg(g, step)
        loss = m(batch.to('cuda'), train_pv=g.train_pv, neg_word_idxs=_cuda(nw))
        m.zero_grad()
        loss.backward()
        touched.append(_touched_np(g, batch, nw))
        got_t = m.touched_rows()
        for n in touched[-1]:
            assert np.array_equal(got_t[n].cpu().numpy(), touched[-1][n]), (step, n)
        optim.step()
        sd = optim.state_dict()['state']
        states.append({n: (sd[names.index(n)]['exp_avg'].cpu(), sd[names.index(n)]['exp_avg_sq'].cpu()) for n in touched[-1]})
        oloss = _oracle_forward(g, P, batch, nw, step)
        with torch.no_grad():
            opt.step(P, grads_of(oloss, P, _oracle_pad(g)), touched=touched[-1])
        ostates.append({n: (opt.state[n]['m'].clone(), opt.state[n]['v'].clone()) for n in touched[-1]})
    for n in (REVIEW, USER, ITEM):
        t1, t2 = touched[0][n], touched[1][n]
        only1 = np.setdiff1d(t1, t2)
        assert only1.size > 0, n                                    # the neighbour move leaves step-1-only rows
        outside = np.setdiff1d(np.arange(init[n].shape[0]), np.union1d(t1, t2))
        assert outside.size > 0, n
        for which in (0, 1):
            got1, got2 = states[0][n][which], states[1][n][which]
            assert float(got2[outside].abs().max()) == 0, n          # never addressed: the moments are exactly zero
            assert float(got1[only1].abs().max()) > 0, n
            assert torch.equal(got2[only1], got1[only1]), n          # addressed in step 1 only: step 1's moments, bit for bit
            # the oracle's row-sparse rule says the same
            o1, o2 = ostates[0][n][which], ostates[1][n][which]
            assert float(o2[outside].abs().max()) == 0 and torch.equal(o2[only1], o1[only1]), n
            assert torch.equal(got2.ne(0).any(1), o2.ne(0).any(1)), n    # the same rows carry moments
        sdm = m.state_dict()
        assert torch.equal(sdm[n].cpu()[outside], init[n][outside]), n
    ever = {n: np.union1d(touched[0][n], touched[1][n]) for n in touched[0]}
    _check_params(m, P, init, ever, a, 1)


# -------------------------------------------------------------------------------------------------------- zero_grad
def test_rtm_rowsparse_zero_grad_without_step_cleans_touched_rows():
    g = RtmGolden('rtm_pv_ui')
    m = _model(g, _args(g))
    b = g.batch().to('cuda')
    nw = _cuda(_neg(g, 0))
    grads = []
    for _ in range(2):                                      # two backwards, zero_grad between, no optimizer
        loss = m(b, train_pv=g.train_pv, neg_word_idxs=nw)
        m.zero_grad()
        loss.backward()
        grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    assert {REVIEW, USER, ITEM, WORD} <= set(grads[0])
    for n in grads[0]:
        assert float(grads[0][n].abs().max()) > 0, n
        if not n.endswith('linear_keys.bias'):
            assert rel_err(grads[1][n], grads[0][n]) < 1e-5, n  # not accumulated
    loss = m(b, train_pv=g.train_pv, neg_word_idxs=nw)
    with pytest.raises(NotImplementedError, match='accumulation'):
        loss.backward()                                     # accumulation over dirty rows is refused


# --------------------------------------------------------------------------------------- a table frozen between steps
def test_a_table_frozen_between_steps_leaves_the_sparse_set():
    from oracle import optim as ooptim
    from oracle.tem import grads_of
    from prodsearch_amd import build_optim
    g = RtmGolden('rtm_pv_ui')
    a = _args(g)
    m = _model(g, a)
    optim = build_optim(a, m, None)
    P = {k: v.clone().requires_grad_(True) for k, v in g.params().items()}
    init = {k: v.detach().clone() for k, v in P.items()}
    opt = ooptim.ClipAdam(a.lr, a.max_grad_norm, a.beta1, a.beta2, 1e-9, a.l2_lambda, a.decay_method, a.warmup_steps)
    batch = g.batch()
    b = batch.to('cuda')
    ever = {}
    for step in range(2):
        if step == 1:
            m.user_emb.weight.requires_grad_(False)
            P[USER].requires_grad_(False)
            user_before = m.user_emb.weight.detach().clone()
        nw = _neg(g, step)
        loss = m(b, train_pv=g.train_pv, neg_word_idxs=_cuda(nw))
        m.zero_grad()
        loss.backward()
        touched = _touched_np(g, batch, nw)
        if step == 1:
            del touched[USER]
            assert m.user_emb.weight.grad is None and getattr(m.user_emb.weight, '_ps_rows', None) is None
            assert set(m._sparse_paths()) == {('review_emb',), ('product_emb',), ('word_emb',)}
        got_t = m.touched_rows()
        assert sorted(got_t) == sorted(touched)
        for n in touched:
            assert np.array_equal(got_t[n].cpu().numpy(), touched[n]), (step, n)
            ever[n] = np.union1d(ever.get(n, np.zeros(0, np.int64)), touched[n])
        optim.step()
        assert len(optim._plan['rows']) == len(touched)
        oloss = _oracle_forward(g, P, batch, nw, step)
        assert rel_err(loss.detach().cpu(), oloss.detach()) < 2e-4, step
        with torch.no_grad():
            opt.step(P, grads_of(oloss, P, _oracle_pad(g)), touched=touched)
        assert abs(optim.last_grad_norm - opt.last_total_norm) < 1e-3 * opt.last_total_norm
        _check_params(m, P, init, ever, a, step)
    assert torch.equal(m.user_emb.weight.detach(), user_before)      # the frozen table stood still


# -------------------------------------------------------------------------------------------------- trainer smoke test
def test_trainer_runs_row_sparse_and_its_checkpoint_continues_bit_for_bit(tmp_path):
    from prodsearch_amd import _lib, default_args, synth, trainer, corpus, pyrandom
    from prodsearch_amd.rtm_loader import ProdSearchDataLoader
    data_path, inp = synth.write_corpus(str(tmp_path / 'corpus'), 31, n_users=50, n_products=40, n_words=150)
    save = str(tmp_path / 'run')
    args = default_args(model_name='review_transformer', review_encoder_name='pv', embedding_size=64, ff_size=128, heads=4,
                        inter_layers=1, batch_size=16, neg_per_pos=3, uprev_review_limit=3, iprev_review_limit=4,
                        review_word_limit=12, subsampling_rate=1e-2, lr=0.01, max_train_epoch=1, steps_per_checkpoint=5,
                        has_valid=True, valid_candi_size=8, candi_batch_size=8, test_candi_size=-1, valid_batch_size=6,
                        data_dir=data_path, input_train_dir=inp, save_dir=save, device='cuda', dropout=0.0,
                        train_pv_epoch=1, pv_window_size=4, use_user_emb=True, use_item_emb=True, row_sparse_adam=True)
    os.makedirs(save)
    args.start_epoch = 0
    torch.manual_seed(1); pyrandom.seed(1); np.random.seed(1)
    gd = corpus.GlobalProdSearchData(args, data_path, inp)
    train_pd = corpus.ProdSearchData(args, inp, 'train', gd)
    valid_pd = corpus.ProdSearchData(args, inp, 'valid', gd)
    model, optim = trainer.create_model(args, gd, train_pd)
    tr = trainer.Trainer(args, model, optim)
    tr.train(args, gd, train_pd, valid_pd)
    rows = [p for p, _ in optim._plan['rows']]
    for tab in (model.review_encoder.review_embeddings.weight, model.user_emb.weight, model.product_emb.weight):
        assert any(tab is p for p in rows)
    model.check_index_errors()
    mrr, _ = tr.validate(args, gd, corpus.ProdSearchDataset(args, gd, valid_pd))
    assert np.isfinite(mrr) and 0.0 <= mrr <= 1.0
    # the epoch's checkpoint, reloaded with its optimizer state, takes the next step exactly as the running model does
    path = os.path.join(save, 'model_epoch_1.ckpt')
    args2 = copy.copy(args)
    args2.train_from = path
    model2, optim2 = trainer.create_model(args2, gd, train_pd, path)
    train_pd.initialize_epoch()
    loader = ProdSearchDataLoader(args, corpus.ProdSearchDataset(args, gd, train_pd), prepare_pv=False,
                                  batch_size=args.batch_size, shuffle=False, device='cuda', prefetch=0)
    batch = next(b for b in loader if b is not None)
    lib = _lib.load()
    old = lib.ps_set_deterministic(1)            # the default step's fp32 atomics differ from run to run by themselves
    try:
        for mo, op in ((model, optim), (model2, optim2)):
            mo.train()
            loss = mo(batch, train_pv=False)
            mo.zero_grad()
            loss.backward()
            op.step()
        torch.cuda.synchronize()
    finally:
        lib.ps_set_deterministic(old)
    assert optim._step == optim2._step
    sd1, sd2 = model.state_dict(), model2.state_dict()
    for n in sd1:
        assert torch.equal(sd1[n], sd2[n]), n
    o1, o2 = optim.state_dict()['state'], optim2.state_dict()['state']
    assert sorted(o1) == sorted(o2)
    for i in o1:
        assert torch.equal(o1[i]['exp_avg'], o2[i]['exp_avg']) and torch.equal(o1[i]['exp_avg_sq'], o2[i]['exp_avg_sq']), i
