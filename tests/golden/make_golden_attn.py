#!/usr/bin/env python3
"""Generate the ZAM / AEM golden fixtures ``tests/golden/attn_*.npz`` from the REFERENCE itself.

Runs only where the reference checkout is available; the fixtures it writes are data (inputs + the reference's outputs)
and are what travels.  The reference is imported unmodified.  The harness hooks act on torch only:

1. ``Tensor.masked_fill`` accepts uint8 masks (make_golden.py);
2. ``1 - bool_tensor`` returns ``(~t).to(uint8)``, the legacy semantics the reference relies on when it builds the
   attention mask (``mask=1-pos_item_seq_mask``, item_transformer.py:401 for AEM, whose mask stays bool; torch >= 2 raises);
3. ``torch.multinomial`` returns pre-drawn negatives (make_golden.py);
4. dropout calls multiply by the product's Philox masks (oracle/philox.py) in call order: FS (text_encoder.py:34), the
   attention of the positive (neural.py:226, call (0, 0)), the attention of the negatives (call (1, 0)).

Recorded per case: inputs, the reference's state_dict keys / shapes, loss, every gradient (step 0), the parameters after
the first and the last ``Optimizer.step``, and ``test_attn`` scores on the initial weights.

Usage:  python tests/golden/make_golden_attn.py [case ...]
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg   # noqa: E402  (hooks 1 and 3, the dropout hook of 4, the reference imports)
import numpy as np          # noqa: E402
import torch                # noqa: E402

from oracle.philox import PhiloxDropout      # noqa: E402
from prodsearch_amd import synth             # noqa: E402
from prodsearch_amd.config import default_args   # noqa: E402

# 2. legacy `1 - bool` (uint8 result)
_orig_rsub = torch.Tensor.__rsub__


def _rsub(self, other):
    if self.dtype == torch.bool and isinstance(other, int) and other == 1:
        return (~self).to(torch.uint8)
    return _orig_rsub(self, other)


torch.Tensor.__rsub__ = _rsub


class _AttnCallOrder(object):
    """Routes the forward's dropout calls (FS, attention positive, attention negatives) to the Philox masks."""

    def __init__(self, gen):
        self.gen, self.n = gen, 0

    def __call__(self, x, kind, call):
        k = self.n
        self.n += 1
        if k == 0:
            return self.gen(x, 'fs', 0)
        assert k in (1, 2), k
        return self.gen(x, 'attn', (k - 1, 0))


CASES = {
    'attn_zam': dict(args=dict(model_name='ZAM', embedding_size=32, heads=4, neg_per_pos=5, dropout=0.0, lr=0.002),
                     P=300, V=400, B=16, Q=6, L=8, W=1, C=20, steps=2),
    'attn_aem': dict(args=dict(model_name='AEM', embedding_size=32, heads=4, neg_per_pos=5, dropout=0.0, lr=0.002),
                     P=300, V=400, B=16, Q=6, L=8, W=1, C=20, steps=2),
    'attn_zam_drop': dict(args=dict(model_name='ZAM', embedding_size=32, heads=4, neg_per_pos=4, dropout=0.2, lr=0.002,
                                    seed=666),
                          P=300, V=400, B=12, Q=6, L=9, W=1, C=20, steps=2),
    'attn_aem_drop': dict(args=dict(model_name='AEM', embedding_size=64, heads=2, neg_per_pos=4, dropout=0.2, lr=0.002,
                                    seed=7),
                          P=300, V=400, B=12, Q=6, L=9, W=1, C=20, steps=2),
    # half of the rows without any history: every key masked, uniform weights over the pad rows
    'attn_aem_empty': dict(args=dict(model_name='AEM', embedding_size=32, heads=4, neg_per_pos=5, dropout=0.1, lr=0.002,
                                     seed=11),
                           P=300, V=400, B=16, Q=6, L=6, W=1, C=20, steps=2, zero_hist_frac=0.5),
    'attn_zam_opts': dict(args=dict(model_name='ZAM', embedding_size=64, heads=8, neg_per_pos=6, dropout=0.0, lr=0.002,
                                    query_encoder_name='avg', sim_func='bias_product', pos_weight=True, sep_prod_emb=True,
                                    pv_window_size=3),
                          P=300, V=400, B=12, Q=5, L=7, W=3, C=20, steps=2),
}


def run_case(name, spec):
    args = default_args(**spec['args'])
    args.device = 'cpu'
    P_, V_, B, Q, L, W, C = (spec[k] for k in ('P', 'V', 'B', 'Q', 'L', 'W', 'C'))
    K = args.neg_per_pos
    wd = synth.make_word_dists(V_, seed=101)
    torch.manual_seed(0)
    model = mg.ItemTransformerRanker(args, 'cpu', V_, P_, None, word_dists=wd)
    ref_sd = model.state_dict()
    shapes = synth.tem_param_shapes(args, V_, P_)
    ref_shapes = {k: tuple(v.shape) for k, v in ref_sd.items()}
    assert ref_shapes == shapes, (set(ref_shapes) ^ set(shapes))
    wseed = 1000 + sum(map(ord, name))
    pad_rows = {'product_emb.weight': P_, 'hist_product_emb.weight': P_}
    sd = synth.make_state_dict(shapes, wseed, pad_rows)
    model.load_state_dict(sd, strict=True)
    optim = mg.build_optim(args, model, None)

    bt = synth.make_tem_batch(2000 + wseed, B, P_, V_, Q=Q, L=L, W=W, C=C, word_dists=wd,
                              zero_hist_frac=spec.get('zero_hist_frac', 0.05))
    rb = mg.RefBatch(bt.query_word_idxs, bt.target_prod_idxs, bt.u_item_idxs, bt.pos_iword_idxs,
                     bt.query_idxs, bt.user_idxs, bt.candi_prod_idxs, to_tensor=False)
    out = {}
    meta = dict(case=name, args=spec['args'], P=P_, V=V_, B=B, Q=Q, L=L, W=W, C=C, K=K,
                steps=spec['steps'], weight_seed=wseed, word_dists_seed=101,
                weight_checksum={k: synth.checksum(v) for k, v in sd.items()},
                sd_keys=[[k, list(v.shape)] for k, v in ref_sd.items()],
                torch=torch.__version__, numpy=np.__version__)
    for k in ('query_word_idxs', 'target_prod_idxs', 'u_item_idxs', 'pos_iword_idxs', 'candi_prod_idxs'):
        out['in_' + k] = getattr(bt, k).numpy()
    out['in_word_dists'] = wd
    meta['empty_rows'] = int((bt.u_item_idxs == P_).all(dim=1).sum())

    model.eval()
    with torch.no_grad():
        out['test_scores'] = model.test(rb).numpy()
    model.train()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    for step in range(spec['steps']):
        ni, nw = synth.sample_negatives(3000 + wseed + step, B, K, W, P_, wd)
        out['in_neg_item_idxs_%d' % step] = ni.numpy()
        out['in_neg_word_idxs_%d' % step] = nw.numpy()
        mg._draw_queue[:] = [ni, nw]
        order = None
        if args.dropout > 0:
            S_ = L + (1 if args.model_name == 'ZAM' else 0)
            order = _AttnCallOrder(PhiloxDropout(args.dropout, args.seed, step + 1, B, K, args.heads, S_, 1, 0))
            mg._drop['gen'], mg._drop['n'] = order, 0
        del mg._bce_tap[:]
        model.clear_loss()
        loss = model(rb, train_pv=False)                 # trainer.py:74
        assert not mg._draw_queue
        if order is not None:
            assert order.n == 3, order.n
            mg._drop['gen'] = None
        model.zero_grad()                                 # trainer.py:76
        loss.backward()                                   # trainer.py:77
        out['loss_%d' % step] = np.float32(loss.item())
        out['ps_loss_%d' % step] = np.float32(model.ps_loss)
        out['item_loss_%d' % step] = np.float32(model.item_loss)
        if step == 0:
            out['prod_scores'] = mg._bce_tap[0].numpy()       # [B,1+K]
            none_grads = []
            for n, p in model.named_parameters():
                if p.grad is None:
                    none_grads.append(n)
                else:
                    mg.pack_rows(out, 'grad_' + n, p.grad)
            meta['none_grads'] = none_grads
        optim.step()                                      # trainer.py:78
        out['lr_%d' % step] = np.float64(optim.learning_rate)
        if step in (0, spec['steps'] - 1):
            for n, p in model.named_parameters():
                mg.pack_rows(out, 'param%d_%s' % (step, n), p.data, base=init[n])

    out['meta'] = np.asarray(json.dumps(meta))
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-16s loss0=%.6f empty_rows=%d ->  %s (%.1f KB)' % (name, out['loss_0'], meta['empty_rows'], path,
                                                              os.path.getsize(path) / 1024))


if __name__ == '__main__':
    todo = sys.argv[1:] or list(CASES)
    for c in todo:
        run_case(c, CASES[c])
