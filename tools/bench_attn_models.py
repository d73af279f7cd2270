#!/usr/bin/env python3
"""ZAM / AEM training step against the item transformer and an eager-torch restatement, same process, alternating.

20 module-API training steps (forward, backward, optimizer) between two synchronisations, after warm-up, at the C2 shape
(B = 384, K = 20, L = 20, d = 128, 8 heads, dropout 0.1; the item transformer with one layer, ff 512).  The eager baseline is
the ZAM step written in plain torch ops on the GPU (the reference's forward_attn structure: the attention runs once for the
positives and once on B*K expanded copies for the negatives), with torch.optim.Adam.  Prints one JSON line per model and
round, then the medians.

    python tools/bench_attn_models.py [--steps 20] [--warmup 5] [--rounds 3]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from prodsearch_amd import AttentionEmbeddingRanker, ItemTransformerRanker, build_optim, default_args, synth

B, K, L, Q, d, H, V, P = 384, 20, 20, 8, 128, 8, 32387, 18357


def product_step(name):
    if name == 'TEM':
        a = default_args(model_name='item_transformer', embedding_size=d, heads=H, ff_size=512, inter_layers=1,
                         neg_per_pos=K, dropout=0.1, uprev_review_limit=L)
        cls = ItemTransformerRanker
    else:
        a = default_args(model_name=name, embedding_size=d, heads=H, neg_per_pos=K, dropout=0.1, uprev_review_limit=L)
        cls = AttentionEmbeddingRanker
    wd = synth.make_word_dists(V)
    m = cls(a, 'cuda', V, P, None, word_dists=wd)
    opt = build_optim(a, m, None)
    batch = synth.make_tem_batch(1, B, P, V, Q=Q, L=L, W=1, word_dists=wd).to('cuda')
    m.train()

    def step():
        loss = m(batch)                    # negatives drawn on the device
        m.zero_grad()
        loss.backward()
        opt.step()
    return step


def eager_zam_step():
    dev = 'cuda'
    g = torch.Generator().manual_seed(0)
    p = {
        'product_emb': torch.randn(P + 1, d, generator=g), 'word_emb': torch.randn(V, d, generator=g),
        'word_bias': torch.zeros(V), 'fs_w': torch.randn(d, d, generator=g) * 0.1, 'fs_b': torch.zeros(d),
    }
    for n in ('wk', 'wv', 'wq', 'wo'):
        p[n] = torch.randn(d, d, generator=g) / math.sqrt(d)
    for n in ('bk', 'bv', 'bq', 'bo'):
        p[n] = torch.zeros(d)
    p['product_emb'][P] = 0
    p = {k: v.to(dev).requires_grad_(True) for k, v in p.items()}
    opt = torch.optim.Adam(list(p.values()), lr=0.0005)
    wd = torch.as_tensor(synth.make_word_dists(V), dtype=torch.float32, device=dev)
    bt = synth.make_tem_batch(1, B, P, V, Q=Q, L=L, W=1, word_dists=synth.make_word_dists(V)).to(dev)
    prod_dists = torch.ones(P, device=dev)
    dh = d // H

    def mha(kv, q, pad):
        N, S, _ = kv.shape
        k = F.linear(kv, p['wk'], p['bk']).view(N, S, H, dh).transpose(1, 2)
        v = F.linear(kv, p['wv'], p['bv']).view(N, S, H, dh).transpose(1, 2)
        qq = F.linear(q, p['wq'], p['bq']).view(N, 1, H, dh).transpose(1, 2) / math.sqrt(dh)
        sc = torch.matmul(qq, k.transpose(2, 3)).masked_fill(pad[:, None, None, :], -1e18)
        at = F.dropout(torch.softmax(sc, -1), 0.1, True)
        ctx = torch.matmul(at, v).transpose(1, 2).reshape(N, 1, d)
        return F.linear(ctx, p['wo'], p['bo'])[:, 0]

    def step():
        qw, ui, tgt, pw = bt.query_word_idxs, bt.u_item_idxs, bt.target_prod_idxs, bt.pos_iword_idxs
        ni = torch.multinomial(prod_dists, B * K, replacement=True).view(B, K)
        qm = qw.ne(V - 1)
        mean = (p['word_emb'][qw] * qm.unsqueeze(-1)).sum(1) / qm.sum(1, keepdim=True).clamp(min=1)
        q = torch.tanh(F.linear(F.dropout(mean, 0.1, True), p['fs_w'], p['fs_b']))
        h = torch.cat([torch.zeros(B, 1, d, device=dev), p['product_emb'][ui]], 1)
        pad = torch.cat([torch.zeros(B, 1, dtype=torch.bool, device=dev), ui.eq(P)], 1)
        pos = 0.5 * mha(h, q.unsqueeze(1), pad) + 0.5 * q
        neg = 0.5 * mha(h.unsqueeze(1).expand(-1, K, -1, -1).reshape(B * K, L + 1, d),
                        q.unsqueeze(1).expand(-1, K, -1).reshape(B * K, 1, d),
                        pad.unsqueeze(1).expand(-1, K, -1).reshape(B * K, L + 1)) + 0.5 * q.repeat_interleave(K, 0)
        ps = (pos * p['product_emb'][tgt]).sum(-1)
        ns = (neg.view(B, K, d) * p['product_emb'][ni]).sum(-1)
        sc = torch.cat([ps[:, None], ns], 1)
        tg = torch.cat([torch.ones(B, 1, device=dev), torch.zeros(B, K, device=dev)], 1)
        loss = F.binary_cross_entropy_with_logits(sc, tg, reduction='none').sum(-1).mean()
        nw = torch.multinomial(wd, B * K, replacement=True).view(B, K)
        it = p['product_emb'][tgt]
        wsc = torch.cat([(p['word_emb'][pw[:, 0]] * it).sum(-1, keepdim=True) + p['word_bias'][pw[:, 0]][:, None],
                         (p['word_emb'][nw] * it[:, None]).sum(-1) + p['word_bias'][nw]], 1)
        loss = loss + F.binary_cross_entropy_with_logits(wsc, tg, reduction='none').sum(-1).mean()
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(p.values()), 5.0)
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
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default='TEM,ZAM,AEM,eager_ZAM')
    o = ap.parse_args()
    names = o.only.split(',')
    steps = {n: (eager_zam_step() if n == 'eager_ZAM' else product_step(n)) for n in names}
    for n in names:
        timed(steps[n], o.warmup)
    res = {n: [] for n in names}
    for r in range(o.rounds):
        for n in names:
            ms = timed(steps[n], o.steps)
            res[n].append(ms)
            print(json.dumps(dict(model=n, round=r, ms_per_step=round(ms, 4), tuples_per_s=round(B * (K + 1) / ms * 1e3))))
    print('# median of %d rounds, %d steps each, B=%d K=%d L=%d d=%d H=%d dropout 0.1' % (o.rounds, o.steps, B, K, L, d, H))
    for n in names:
        ms = statistics.median(res[n])
        print('%-10s %8.4f ms/step  %6.2f M tuples/s' % (n, ms, B * (K + 1) / ms / 1e3))


if __name__ == '__main__':
    main()
