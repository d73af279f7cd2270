#!/usr/bin/env python3
"""Review-transformer training step with the trainable pv encoder: dense clip + Adam against ``args.row_sparse_adam``, same
process, alternating.

At the C4 shape (BASELINE configs[3]: B = 256, K = 5, 20 + 30 reviews, d = 128, 8 heads, ff 512, one layer, dropout 0.1,
V = 32,387, 296 k reviews; 100 k users and 60 k products where the per-position tables are on) four steps are timed:

    pv_dense        review + word tables trainable, the dense optimizer (what the flag gave before it was wired: ignored)
    pv_rows         the same model with row_sparse_adam: tables zeroed / clipped / updated by their touched rows
    pv_ui_dense     + use_user_emb + use_item_emb, dense
    pv_ui_rows      + use_user_emb + use_item_emb, row-sparse (four tables, one ps_coalesce_tables call)

20 module-API training steps (forward, backward, optimizer) between two synchronisations, after warm-up, in alternating
rounds — boxes of one pool differ by several per cent, so only figures of one process are compared.  Prints one JSON line per
model and round, then the medians with each model's min-to-max spread, and the touched-row counts of the last step.

    python tools/bench_rtm_rowsparse.py [--steps 20] [--warmup 5] [--rounds 5] [--only pv_dense,pv_rows,...] [--train-pv]

``--only pv_ui_dense --rounds 1`` (or ``pv_ui_rows``) under ``rocprofv3 --kernel-trace --stats`` (a run of its own) lists what
``adam_update_kernel`` / ``adam_sumsq_kernel`` cost dense and what the three coalesce launches and ``rs_*`` cost row-sparse.
In a job script every GPU step gets its own ``timeout`` and the steps are chained with ``&&``.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from prodsearch_amd import ProductRanker, build_optim, default_args, rtm_data, synth

B, K, U, I, WL, d, H, V, RC = 256, 5, 20, 30, 100, 128, 8, 32387, 296000
USERS, PRODUCTS = 100000, 60000
MODELS = ('pv_dense', 'pv_rows', 'pv_ui_dense', 'pv_ui_rows')


def product_step(name, train_pv):
    ui, rows = '_ui_' in name, name.endswith('_rows')
    a = default_args(model_name='review_transformer', review_encoder_name='pv', embedding_size=d, heads=H, ff_size=512,
                     inter_layers=1, neg_per_pos=K, dropout=0.1, lr=0.0005, review_word_limit=WL, uprev_review_limit=U,
                     iprev_review_limit=I, use_user_emb=ui, use_item_emb=ui, row_sparse_adam=rows)
    wd = synth.make_word_dists(V)
    rng = synth.rng_for(5)
    rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, WL)))
    lens = torch.from_numpy(rng.integers(WL // 4, WL + 1, size=RC))
    rw[torch.arange(WL)[None, :] >= lens[:, None]] = V - 1
    rw[-1] = V - 1
    torch.manual_seed(1234)
    m = ProductRanker(a, 'cuda', V, RC, PRODUCTS, USERS, rw, None, word_dists=wd)
    opt = build_optim(a, m, None)
    batches = [rtm_data.make_rtm_batch(100 + s, B, K, RC, V, rw, Q=8, u_lim=U, i_lim=I, W=1, train_pv=train_pv, encoder='pv',
                                       word_dists=wd, user_size=USERS if ui else None,
                                       product_size=PRODUCTS if ui else None).to('cuda') for s in range(4)]
    m.train()
    count = [0]

    def step():
        loss = m(batches[count[0] % len(batches)], train_pv=train_pv)
        count[0] += 1
        m.zero_grad()
        loss.backward()
        opt.step()
    return m, step


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
    ap.add_argument('--only', default=','.join(MODELS))
    ap.add_argument('--train-pv', action='store_true', help='add the PV word-prediction loss (window 1, draws on the device)')
    o = ap.parse_args()
    names = o.only.split(',')
    assert all(n in MODELS for n in names), names
    if not torch.cuda.is_available():
        raise SystemExit("bench_rtm_rowsparse: no GPU (a timing needs one)")
    built = {n: product_step(n, o.train_pv) for n in names}
    for n in names:
        timed(built[n][1], o.warmup)
    res = {n: [] for n in names}
    for r in range(o.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            ms = timed(built[n][1], o.steps)
            res[n].append(ms)
            print(json.dumps(dict(model=n, round=r, ms_per_step=round(ms, 4))), flush=True)
    print('# median of %d rounds, %d steps each, pv encoder trainable, train_pv=%d, B=%d K=%d R=%d+%d d=%d H=%d V=%d reviews=%d '
          'users=%d products=%d dropout 0.1' % (o.rounds, o.steps, int(o.train_pv), B, K, U, I, d, H, V, RC, USERS, PRODUCTS))
    for n in names:
        print('%-12s %8.4f ms/step  (min %.4f, max %.4f, spread %.4f)'
              % (n, statistics.median(res[n]), min(res[n]), max(res[n]), max(res[n]) - min(res[n])))
    for n in names:
        m = built[n][0]
        if m._row_sparse():
            m.check_index_errors()
            print('# touched %-12s %s' % (n, ' '.join('%s=%d/%d' % (k, v.numel(), dict(m.named_parameters())[k].shape[0])
                                                        for k, v in m.touched_rows().items())))


if __name__ == '__main__':
    main()
