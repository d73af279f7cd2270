"""The reference's model options (main.py: query encoder, sim_func, pos_weight, sep_prod_emb, use_item_pos, use_pos_emb,
layers, QEM) on the paths that ship: d = 128 / d = 256 with dropout replicas, where the fused per-replica MLP, the projection +
attention launch, the wave-per-replica attention backward, the fused K/V input gradient and the folded scoring run.  The golden
fixtures cover these options only at d <= 64 without replicas, where none of those forms is taken.

Every case against the oracle (replicated, with the product's Philox masks): loss, every parameter gradient, touched rows, the
query words' rows of word_embeddings on their own, eval scores."""
import pytest
import torch

from golden_util import rel_err

pytestmark = pytest.mark.gpu


def check_against_oracle(B, K, L, Q, W=1, zero_hist=0.2, P_=700, V=900, expect=None, **over):
    """One training forward + backward through the module API and one eval call, against oracle.tem.  ``over``: default_args
    overrides on top of d = 128, 8 heads, ff 256, one layer, dropout 0.1.  ``expect``: called with 0 behind the training forward
    and with 1 behind the backward (enc_paths.taken_checker: the encoder path the step took)."""
    from oracle import tem as otem, philox
    from prodsearch_amd import ItemTransformerRanker, default_args, synth
    kw = dict(model_name='item_transformer', embedding_size=128, heads=8, ff_size=256, inter_layers=1, neg_per_pos=K,
              dropout=0.1, uprev_review_limit=L, pv_window_size=W)
    kw.update(over)
    a = default_args(**kw)
    qem = a.model_name == 'QEM'
    wd = synth.make_word_dists(V)
    sd = synth.make_state_dict(synth.tem_param_shapes(a, V, P_), 7, {'product_emb.weight': P_, 'hist_product_emb.weight': P_})
    m = ItemTransformerRanker(a, 'cuda', V, P_, None, word_dists=wd)
    m.load_state_dict(sd, strict=False)
    m.train()
    batch = synth.make_tem_batch(11, B, P_, V, Q=Q, L=L, W=W, C=9, word_dists=wd, zero_hist_frac=zero_hist)
    ni, nw = synth.sample_negatives(12, B, K, W, P_, wd)
    loss = m(batch.to('cuda'), neg_item_idxs=ni.cuda(), neg_word_idxs=nw.cuda())
    if expect:
        expect(0)
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    if expect:
        expect(1)

    Pm = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    drop = None
    if a.dropout > 0:
        drop = philox.PhiloxDropout(a.dropout, m._seed, m._fwd_step, B, K, a.heads, L + 1, a.inter_layers,
                                    L if a.use_item_pos else 0)
    if qem:
        oloss, _, _ = otem.qem_forward(Pm, a, batch, ni, nw, V, P_, training=True, drop=drop)
    else:
        oloss, _, _ = otem.tem_forward(Pm, a, batch, ni, nw, V, P_, training=True, replicate=drop is not None, drop=drop)
    print('figures: loss rel_err %.2e' % rel_err(loss.detach().cpu(), oloss.detach()))
    assert rel_err(loss.detach().cpu(), oloss.detach()) < 1e-4
    grads = otem.grads_of(oloss, Pm, otem.tem_pad_rows(a, V, P_))
    worst = (0.0, None)
    for n, p in m.named_parameters():
        ref = grads.get(n)
        assert (p.grad is None) == (ref is None), n
        if ref is None or n.endswith('linear_keys.bias'):       # (its gradient is rounding noise: softmax is shift-invariant)
            continue
        got = p.grad.cpu()
        err = rel_err(got, ref)
        assert err < 5e-4, (n, err)
        if err >= worst[0]:
            worst = (float(err), n)
        if ref.dim() == 2 and ref.shape[0] > 256:
            assert torch.equal(got.ne(0).any(1), ref.ne(0).any(1)), n
    print('figures: worst gradient rel_err %.2e (%s)' % worst)
    # the query words' rows alone: their gradient shares word_embeddings with item_to_words', and a wrong query part can hide
    # under the whole table's largest entry
    qrows = torch.unique(batch.query_word_idxs)
    qrows = qrows[qrows != V - 1]
    got_q, ref_q = dict(m.named_parameters())['word_embeddings.weight'].grad.cpu()[qrows], grads['word_embeddings.weight'][qrows]
    assert rel_err(got_q, ref_q) < 5e-4, ('word_embeddings (query rows)', rel_err(got_q, ref_q))

    m.eval()
    with torch.no_grad():
        s = m.test(batch.to('cuda')).cpu()
        ref_s = otem.qem_test(sd, a, batch, V, P_) if qem else otem.tem_test(sd, a, batch, V, P_)
    assert rel_err(s, ref_s) < 1e-4


# B = 50, K = 20, L = 9: 1,050 replica rows, the fused forms' shape
C2S = dict(B=50, K=20, L=9, Q=4)
CASES = {
    'avg': dict(C2S, query_encoder_name='avg'),                    # the fused K/V input gradient + the AVG encoder's backward
    'avg_nopos': dict(C2S, query_encoder_name='avg', use_pos_emb=False),
    'avg_f512': dict(B=64, K=20, L=20, Q=6, ff_size=512, query_encoder_name='avg'),   # the benched MLP width
    'avg_zero_hist': dict(C2S, zero_hist=0.5, query_encoder_name='avg'),
    'avg_nodrop': dict(C2S, dropout=0.0, query_encoder_name='avg'),  # no replicas: the single-wave forms
    'item_pos': dict(C2S, use_item_pos=True),                      # the consumed position is S-1
    'bias_product': dict(C2S, sim_func='bias_product'),
    'pos_weight': dict(C2S, pos_weight=True),
    'sep_prod_emb': dict(C2S, sep_prod_emb=True),
    'all_opts': dict(C2S, W=3, sim_func='bias_product', pos_weight=True, sep_prod_emb=True, use_item_pos=True),
    'two_layers': dict(C2S, inter_layers=2),                       # fused last layer (folded scoring) behind an unfused first one
    'qem': dict(C2S, model_name='QEM'),
    'd256_avg': dict(B=70, K=20, L=20, Q=8, embedding_size=256, ff_size=1024, query_encoder_name='avg'),
    'd256_item_pos': dict(B=70, K=20, L=20, Q=8, embedding_size=256, ff_size=1024, use_item_pos=True),
}


@pytest.mark.parametrize('case', list(CASES))
def test_option_matches_oracle(case):
    import enc_paths
    row = enc_paths.OPTION_ROWS.get(case)          # the encoder path of the annotated cases
    check_against_oracle(expect=enc_paths.taken_checker(row) if row else None, **CASES[case])


def test_avg_deterministic_matches_oracle():
    """The 'avg' case in deterministic mode, which leaves the K/V input gradient to the dX product: a control that points at the
    fused form when the default case disagrees."""
    from prodsearch_amd import _lib
    lib = _lib.load()
    old = lib.ps_set_deterministic(1)
    try:
        check_against_oracle(**CASES['avg'])
    finally:
        lib.ps_set_deterministic(old)


def test_batch_past_the_row_list_limit():
    """A batch past the valid-row list's limit (B * B * L > 64 M, tem.hip rows_list_ok): the K / V weight gradients run over all
    B * S rows.  With replicas (S <= 2 (K + 1)) the K / V / Q weight gradients are deferred behind the scatter and the FS f_W
    gradient joins them — four members; 48,768 reduction rows give the bf16x3 split form 96 splits (4 x 96 >= 384 workgroups).
    The grouped launch used to hand that group to its flat form, which holds three ('gemm: group size 4' mid-backward)."""
    check_against_oracle(B=8128, K=3, L=5, Q=4, P_=3000, V=2000)
