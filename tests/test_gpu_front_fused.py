"""The d = 128 forward front end as one launch (csrc/attn_sq1.hip, front_attn_fwd_kernel: embed + K / V / Q + attention) against
the two launches it replaces (embed_fwd_kernel, kvq_attn_fwd_kernel), through ps_front_fused_test: the same inputs into two
workspaces, the largest absolute difference per region.  The form does the same arithmetic in the same order — same split, same
products, same sums — so EVERY region must come out exactly 0: x, qmean_d, query_emb, the K / V rows of valid positions, qp, the
softmax, the keep bits, the context rows, the word tasks' scores and terms, the sampled ids, the valid-row list and its length.

What takes the form: kvq_attn_fits (d = 128, 8 heads, S <= 32, 4..24 replicas, one layer, query position 0, the row list) with
the FS query encoder, positional rows and 1 <= Q <= 16 (PS_FRONT_MAX_Q: one query word per lane group of the sequence's
workgroup).  The AVG encoder and longer queries keep the two launches; so does everything that does not take the kvq form.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

REGIONS = ('x', 'qmean_d', 'query_emb', 'kp', 'vp', 'qp', 'attn', 'amask', 'ctx', 'word_scores', 'word_terms', 'neg_items',
           'neg_words', 'vrows', 'vcount')


def _case(B=6, K=4, L=20, Q=4, W=1, zero_hist=0.2, taken=1, **over):
    return dict(B=B, K=K, L=L, Q=Q, W=W, zero_hist=zero_hist, taken=taken, over=over)


TAKEN = {
    's2': _case(L=1),                                   # S = 2
    's25': _case(L=24),                                 # kernel instance <8>
    's32': _case(L=31, B=5),
    's24_fan24': _case(L=23, K=23, B=3),                # instance <6> at its last position count, 24 replicas
    'fan4': _case(K=3, B=7),                            # 4 replicas
    'b1': _case(B=1),                                   # one sequence: an odd rider block count of every kind
    'b33': _case(B=33, K=20, L=9),                      # several rider workgroups of every kind
    'hist_all_pad': _case(zero_hist=1.0),               # one valid position per sequence
    'query_all_pad': _case(Q=4, pad_query=True),        # count 0
    'q1': _case(Q=1),
    'q8': _case(Q=8),
    'q16': _case(Q=16),                                 # the bound
    'w3': _case(W=3, Q=8, K=5, B=2, zero_hist=0.0),     # e_2_5_20
}
NOT_TAKEN = {
    'q17': _case(Q=17, taken=0),                        # one past the bound: the two launches
    'avg': _case(taken=0, query_encoder_name='avg'),    # the AVG encoder keeps the two launches
    'nodrop': _case(taken=0, dropout=0.0),              # no replicas
    's33': _case(L=32, taken=0),
    'item_pos': _case(taken=0, use_item_pos=True),
    'two_layers': _case(L=9, taken=0, inter_layers=2),
}


def _model_and_batch(c):
    from prodsearch_amd import ItemTransformerRanker, default_args, synth
    P_, V = 700, 900
    kw = dict(model_name='item_transformer', embedding_size=128, heads=8, ff_size=256, inter_layers=1, neg_per_pos=c['K'],
              dropout=0.1, uprev_review_limit=c['L'], pv_window_size=c['W'])
    over = dict(c['over'])
    pad_query = over.pop('pad_query', False)
    kw.update(over)
    a = default_args(**kw)
    wd = synth.make_word_dists(V)
    sd = synth.make_state_dict(synth.tem_param_shapes(a, V, P_), 7, {'product_emb.weight': P_, 'hist_product_emb.weight': P_})
    m = ItemTransformerRanker(a, 'cuda', V, P_, None, word_dists=wd)
    m.load_state_dict(sd, strict=False)
    m.train()
    batch = synth.make_tem_batch(11, c['B'], P_, V, Q=c['Q'], L=c['L'], W=c['W'], C=9, word_dists=wd, zero_hist_frac=c['zero_hist'])
    if pad_query:
        batch.query_word_idxs[:] = V - 1
    return m, batch.to('cuda')


def _both_ways(m, batch):
    """ps_front_fused_test on the model's own descriptor and tensors; returns ({region: diff}, taken pair, loss pair)."""
    from prodsearch_amd import _lib
    lib = _lib.load()
    ps, _ = m._structs()
    plan = m._plan_for(batch, eval_mode=False)
    m._fwd_step += 1
    plan.desc.step = m._fwd_step
    d = plan.desc
    dev = plan.ws.device
    negs = [torch.empty(d.B, n, device=dev, dtype=torch.int64) for n in (d.K, d.W * d.K, d.K, d.W * d.K)]
    m._fill_batch(plan, batch, False, negs[0], negs[1])
    ws_b = torch.zeros_like(plan.ws)
    plan.ws.zero_()
    loss = torch.zeros(2, 3, device=dev)
    prob, alias = m._alias_tables()
    diff = (C.c_double * len(REGIONS))()
    taken = (C.c_int32 * 2)()
    _lib.check(lib.ps_front_fused_test(d, ps, plan.batch, prob.data_ptr(), alias.data_ptr(), plan.ws.data_ptr(), ws_b.data_ptr(),
                                       negs[0].data_ptr(), negs[1].data_ptr(), negs[2].data_ptr(), negs[3].data_ptr(),
                                       loss[0].data_ptr(), loss[1].data_ptr(), diff, taken, m._stream()), 'ps_front_fused_test')
    torch.cuda.synchronize()
    return dict(zip(REGIONS, diff)), (taken[0], taken[1]), loss.cpu()


@pytest.mark.parametrize('name', list(TAKEN) + list(NOT_TAKEN))
def test_regions_are_bitwise_equal(name):
    c = TAKEN.get(name) or NOT_TAKEN[name]
    m, batch = _model_and_batch(c)
    diff, taken, loss = _both_ways(m, batch)
    print('figures:', name, 'taken', taken, ' '.join('%s %.3g' % kv for kv in diff.items()),
          'loss %.9g %.9g' % (float(loss[0, 0]), float(loss[1, 0])))
    assert taken == (0, c['taken']), (name, taken)
    assert all(v == 0.0 for v in diff.values()), (name, {k: v for k, v in diff.items() if v != 0.0})
    assert torch.isfinite(loss).all()
    assert torch.equal(loss[0], loss[1]), (name, loss)       # the loss of the whole forward: bitwise


@pytest.mark.parametrize('name', ['b33', 'nodrop', 's33', 'item_pos', 'two_layers'])
def test_module_loss_is_bitwise_equal_with_the_switch_on_and_off(name):
    """The module API's forward, same process, the switch on and off: the same loss, bit for bit (the word tasks kept their mapping
    to word_blk partials), and the same gradients' path behind it."""
    from prodsearch_amd import _lib, synth
    lib = _lib.load()
    c = TAKEN.get(name) or NOT_TAKEN[name]
    losses, grads = [], []
    for on in (1, 0):
        old = lib.ps_set_front_fused(on)
        try:
            m, batch = _model_and_batch(c)
            wd = synth.make_word_dists(900)
            ni, nw = synth.sample_negatives(12, c['B'], c['K'], c['W'], 700, wd)
            loss = m(batch, neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
            assert int(lib.ps_front_fused_taken()) == (c['taken'] if on else 0), name
            m.zero_grad()
            loss.backward()
            torch.cuda.synchronize()
            losses.append(loss.detach().cpu())
            grads.append(dict(m.named_parameters())['query_encoder.f_W.weight'].grad.cpu())
        finally:
            lib.ps_set_front_fused(old)
    assert torch.equal(losses[0], losses[1]), (name, losses)
    # (the backward reads x, qmean_d, query_emb, kp / vp, attn, amask, ctx: bitwise the same inputs; its atomics reassociate)
    assert float((grads[0] - grads[1]).abs().max()) <= 5e-4 * float(grads[1].abs().max()), name


@pytest.mark.parametrize('row', ['e_2_5_20', 'e_50_20_9'])
def test_fused_front_end_matches_oracle(row):
    import enc_paths
    from prodsearch_amd import _lib
    from test_gpu_tem_options import check_against_oracle
    lib = _lib.load()
    r = next(x for x in enc_paths.EDGE_ROWS if x['name'] == row)
    base = enc_paths.taken_checker(r)

    def expect(backward):
        base(backward)
        if not backward and enc_paths.default_switches() and 'PS_FRONT_FUSED' not in __import__('os').environ:
            assert int(lib.ps_front_fused_taken()) == 1, row
    check_against_oracle(expect=expect, **enc_paths.oracle_call(r))
