#!/usr/bin/env python3
"""Training step with a frozen word table (pretrain_emb_dir) against the trainable one, same process, alternating.

At the C2 shape (B = 384, K = 20, L = 20, d = 128, 8 heads, dropout 0.1, V = 32,387; TEM with one layer, ff 512), for TEM
and ZAM: 20 module-API training steps (forward, backward, optimizer) between two synchronisations, after warm-up, in
alternating rounds.  The frozen models are the trainable ones with ``word_embeddings.weight.requires_grad_(False)`` before
``build_optim`` — exactly what ``nn.Embedding.from_pretrained`` leaves (the table's values do not change the step's work).
Prints one JSON line per model and round, then the medians.

    python tools/bench_frozen_words.py [--steps 20] [--warmup 5] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from prodsearch_amd import AttentionEmbeddingRanker, ItemTransformerRanker, build_optim, default_args, synth

B, K, L, Q, d, H, V, P = 384, 20, 20, 8, 128, 8, 32387, 18357


def product_step(name, frozen):
    if name == 'TEM':
        a = default_args(model_name='item_transformer', embedding_size=d, heads=H, ff_size=512, inter_layers=1,
                         neg_per_pos=K, dropout=0.1, uprev_review_limit=L)
        cls = ItemTransformerRanker
    else:
        a = default_args(model_name=name, embedding_size=d, heads=H, neg_per_pos=K, dropout=0.1, uprev_review_limit=L)
        cls = AttentionEmbeddingRanker
    wd = synth.make_word_dists(V)
    torch.manual_seed(0)
    m = cls(a, 'cuda', V, P, None, word_dists=wd)
    if frozen:
        m.word_embeddings.weight.requires_grad_(False)
    opt = build_optim(a, m, None)
    batch = synth.make_tem_batch(1, B, P, V, Q=Q, L=L, W=1, word_dists=wd).to('cuda')
    m.train()

    def step():
        loss = m(batch)                    # negatives drawn on the device
        m.zero_grad()
        loss.backward()
        opt.step()
    return step


def timed(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', default='TEM,ZAM')
    o = ap.parse_args()
    names = ['%s_%s' % (n, mode) for n in o.only.split(',') for mode in ('trainable', 'frozen')]
    steps = {n: product_step(n.split('_')[0], n.endswith('frozen')) for n in names}
    for n in names:
        timed(steps[n], o.warmup)
    res = {n: [] for n in names}
    for r in range(o.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            ms = timed(steps[n], o.steps)
            res[n].append(ms)
            print(json.dumps(dict(model=n, round=r, ms_per_step=round(ms, 4))), flush=True)
    print('# median of %d rounds, %d steps each, B=%d K=%d L=%d d=%d H=%d V=%d dropout 0.1' % (o.rounds, o.steps, B, K, L, d, H, V))
    for n in names:
        print('%-16s %8.4f ms/step  (min %.4f, max %.4f)' % (n, statistics.median(res[n]), min(res[n]), max(res[n])))


if __name__ == '__main__':
    main()
