#!/usr/bin/env python3
"""Generate the pretrained-word-table fixtures ``tests/golden/frozen_*.npz`` (and the shared synthetic
``tests/golden/pretrain_emb/word_emb.txt.gz``) from the REFERENCE itself.

Runs only where the reference checkout is available; what it writes is data.  The reference is imported unmodified, with
the torch hooks of make_golden.py / make_golden_attn.py (uint8 masks, legacy ``1 - bool``, pre-drawn negatives, the
product's Philox dropout masks).  Each case builds the reference model with ``args.pretrain_emb_dir`` pointing at the
synthetic file (``nn.Embedding.from_pretrained``: a frozen word table), loads every OTHER tensor from the deterministic
weight generator, and records: the loaded word table, the state_dict keys / shapes, loss and every gradient of step 0,
the global gradient norm of every step (before clipping), and the parameters after the first and the last of three
``Optimizer.step``s.  ``max_grad_norm`` is chosen so that the clip is active, and so that counting a word-table gradient
in its norm would change the parameters (tests/test_pretrained_cpu.py checks both).

Usage:  python tests/golden/make_golden_pretrained.py [case ...]
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_attn as mga   # noqa: E402  (its hooks, and make_golden's)
import numpy as np               # noqa: E402
import torch                     # noqa: E402

import pretrain_util             # noqa: E402
from oracle.philox import PhiloxDropout          # noqa: E402
from prodsearch_amd import synth                 # noqa: E402
from prodsearch_amd.config import default_args   # noqa: E402

mg = mga.mg
EMB_DIR = os.path.join(HERE, 'pretrain_emb')
V_, D_ = 400, 32

_common = dict(embedding_size=D_, heads=4, ff_size=64, inter_layers=1, neg_per_pos=5, lr=0.002, max_grad_norm=0.05)
CASES = {
    'frozen_tem_fs_drop': dict(args=dict(_common, model_name='item_transformer', dropout=0.1, seed=666),
                               P=300, B=16, Q=6, L=8, W=1, C=20),
    'frozen_tem_avg': dict(args=dict(_common, model_name='item_transformer', dropout=0.0, query_encoder_name='avg'),
                           P=300, B=16, Q=6, L=8, W=1, C=20),
    # (QEM's word-gradient share is the same at every step: a clip active at all three steps would hide it under Adam's
    # scale invariance; at 2.0 the clip is active at step 0 only, and counting the word gradient changes that)
    'frozen_qem': dict(args=dict(_common, model_name='QEM', dropout=0.0, max_grad_norm=2.0), P=300, B=16, Q=6, L=8, W=1, C=20),
    'frozen_zam': dict(args=dict(_common, model_name='ZAM', dropout=0.0), P=300, B=16, Q=6, L=8, W=1, C=20),
    'frozen_aem_drop': dict(args=dict(_common, model_name='AEM', dropout=0.1, seed=7), P=300, B=16, Q=6, L=8, W=1, C=20),
}
STEPS = 3


def write_fixture_file():
    os.makedirs(EMB_DIR, exist_ok=True)
    pretrain_util.write_word_emb(os.path.join(EMB_DIR, 'word_emb.txt.gz'), pretrain_util.vocab_words(V_), D_, seed=5)


def run_case(name, spec):
    args = default_args(**spec['args'])
    args.device = 'cpu'
    args.pretrain_emb_dir = EMB_DIR
    P_, B, Q, L, W, C = (spec[k] for k in ('P', 'B', 'Q', 'L', 'W', 'C'))
    K = args.neg_per_pos
    attn = args.model_name in ('ZAM', 'AEM')
    words = pretrain_util.vocab_words(V_)
    wd = synth.make_word_dists(V_, seed=101)
    torch.manual_seed(0)
    model = mg.ItemTransformerRanker(args, 'cpu', V_, P_, words, word_dists=wd)
    assert not model.word_embeddings.weight.requires_grad
    ref_sd = model.state_dict()
    table = model.word_embeddings.weight.detach().clone()
    shapes = synth.tem_param_shapes(args, V_, P_)
    wseed = 1000 + sum(map(ord, name))
    sd = synth.make_state_dict(shapes, wseed, {'product_emb.weight': P_, 'hist_product_emb.weight': P_})
    del sd['word_embeddings.weight']                  # the pretrained table stays
    model.load_state_dict(sd, strict=False)
    optim = mg.build_optim(args, model, None)

    bt = synth.make_tem_batch(2000 + wseed, B, P_, V_, Q=Q, L=L, W=W, C=C, word_dists=wd)
    rb = mg.RefBatch(bt.query_word_idxs, bt.target_prod_idxs, bt.u_item_idxs, bt.pos_iword_idxs,
                     bt.query_idxs, bt.user_idxs, bt.candi_prod_idxs, to_tensor=False)
    out = {'word_table': table.numpy()}
    meta = dict(case=name, args=spec['args'], P=P_, V=V_, B=B, Q=Q, L=L, W=W, C=C, K=K, steps=STEPS, weight_seed=wseed,
                word_dists_seed=101, weight_checksum={k: synth.checksum(v) for k, v in sd.items()},
                sd_keys=[[k, list(v.shape)] for k, v in ref_sd.items()],
                optim_params=[n for n, p in model.named_parameters() if p.requires_grad],
                torch=torch.__version__, numpy=np.__version__)
    for k in ('query_word_idxs', 'target_prod_idxs', 'u_item_idxs', 'pos_iword_idxs', 'candi_prod_idxs'):
        out['in_' + k] = getattr(bt, k).numpy()
    out['in_word_dists'] = wd
    model.train()
    init = {k: v.clone() for k, v in model.state_dict().items()}
    for step in range(STEPS):
        ni, nw = synth.sample_negatives(3000 + wseed + step, B, K, W, P_, wd)
        out['in_neg_item_idxs_%d' % step] = ni.numpy()
        out['in_neg_word_idxs_%d' % step] = nw.numpy()
        mg._draw_queue[:] = [ni, nw]
        if args.dropout > 0:
            if attn:
                S_ = L + (1 if args.model_name == 'ZAM' else 0)
                gen = mga._AttnCallOrder(PhiloxDropout(args.dropout, args.seed, step + 1, B, K, args.heads, S_, 1, 0))
            else:
                S_ = L + 1
                gen = PhiloxDropout(args.dropout, args.seed, step + 1, B, K, args.heads, S_, args.inter_layers,
                                    (S_ - 1) if args.use_item_pos else 0)
                mg._drop['layers'] = args.inter_layers
            mg._drop['gen'], mg._drop['n'] = gen, 0
        del mg._bce_tap[:]
        model.clear_loss()
        loss = model(rb, train_pv=False)                 # trainer.py:74
        assert not mg._draw_queue
        mg._drop['gen'] = None
        model.zero_grad()                                 # trainer.py:76
        loss.backward()                                   # trainer.py:77
        assert model.word_embeddings.weight.grad is None
        out['loss_%d' % step] = np.float32(loss.item())
        gs = [p.grad for p in model.parameters() if p.grad is not None]
        out['gnorm_%d' % step] = np.float64(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in gs])))
        if step == 0:
            none_grads = []
            for n, p in model.named_parameters():
                if p.grad is None:
                    none_grads.append(n)
                else:
                    mg.pack_rows(out, 'grad_' + n, p.grad)
            meta['none_grads'] = none_grads
        optim.step()                                      # trainer.py:78
        if step in (0, STEPS - 1):
            for n, p in model.named_parameters():
                mg.pack_rows(out, 'param%d_%s' % (step, n), p.data, base=init[n])
    assert torch.equal(model.word_embeddings.weight.detach(), table)
    out['meta'] = np.asarray(json.dumps(meta))
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **out)
    print('%-20s loss0=%.6f gnorm0=%.4f ->  %s (%.1f KB)' % (name, out['loss_0'], out['gnorm_0'], path,
                                                           os.path.getsize(path) / 1024))


if __name__ == '__main__':
    write_fixture_file()
    todo = sys.argv[1:] or list(CASES)
    for c in todo:
        run_case(c, CASES[c])
