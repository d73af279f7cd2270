#!/usr/bin/env python3
"""Review-transformer training step on frozen tables against the trainable one, same process, alternating.

At the C4 shape (BASELINE configs[3]: B = 256, K = 5, 20 + 30 reviews of 100 words, d = 128, 8 heads, ff 512, one layer,
dropout 0.1, corrupt_rate 0.9, V = 32,387, 296 k reviews) four steps are timed:

    pvc_trainable   the baseline (bench.py --workload c4)
    pvc_frozen      pvc with the word table frozen (pretrain_emb_dir's context_emb)
    pv_frozen       pv with the word table and the review table frozen (pretrain_emb_dir: word_emb + doc_emb)
    fix_emb         an argument of pvc with fix_emb and both tables frozen: the pv encoder, its PV drop site off

20 module-API training steps (forward, backward, optimizer) between two synchronisations, after warm-up, in alternating
rounds — boxes of one pool differ by several per cent, so only figures of one process are compared.  The frozen models are
the trainable ones with ``requires_grad_(False)`` on their tables before ``build_optim`` — exactly what
``nn.Embedding.from_pretrained`` leaves (a table's values do not change the step's work).  Prints one JSON line per model and
round, then the medians and each model's backward plan (``ps_rtm_backward_plan``).

    python tools/bench_frozen_rtm.py [--steps 20] [--warmup 5] [--rounds 5] [--only pvc_trainable,pvc_frozen,...]

``--only pvc_frozen --rounds 1`` under ``rocprofv3 --kernel-trace --stats`` (a run of its own) lists the launches that remain.
In a job script every GPU step gets its own ``timeout`` and the steps are chained with ``&&``.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from prodsearch_amd import PretrainedProductRanker, ProductRanker, _lib, build_optim, default_args, rtm_data, synth

B, K, U, I, WL, d, H, V, RC = 256, 5, 20, 30, 100, 128, 8, 32387, 296000
MODELS = ('pvc_trainable', 'pvc_frozen', 'pv_frozen', 'fix_emb')


def product_step(name):
    fix = name == 'fix_emb'
    enc = 'pv' if name == 'pv_frozen' else 'pvc'
    a = default_args(model_name='review_transformer', review_encoder_name=enc, embedding_size=d, heads=H, ff_size=512,
                     inter_layers=1, neg_per_pos=K, dropout=0.1, corrupt_rate=0.9, lr=0.0005, review_word_limit=WL,
                     uprev_review_limit=U, iprev_review_limit=I, fix_emb=fix)
    wd = synth.make_word_dists(V)
    rng = synth.rng_for(5)
    rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, WL)))
    lens = torch.from_numpy(rng.integers(WL // 4, WL + 1, size=RC))
    rw[torch.arange(WL)[None, :] >= lens[:, None]] = V - 1
    rw[-1] = V - 1
    torch.manual_seed(1234)
    m = (PretrainedProductRanker if fix else ProductRanker)(a, 'cuda', V, RC, 1000, 1000, rw, None, word_dists=wd)
    if name != 'pvc_trainable':
        m.word_embeddings.weight.requires_grad_(False)
    if name == 'pv_frozen':
        m.review_encoder.review_embeddings.weight.requires_grad_(False)
    opt = build_optim(a, m, None)
    batch_enc = 'pv' if fix else enc
    batches = [rtm_data.make_rtm_batch(100 + s, B, K, RC, V, rw, Q=8, u_lim=U, i_lim=I, W=1, train_pv=False, encoder=batch_enc,
                                       word_dists=wd).to('cuda') for s in range(4)]
    m.train()
    count = [0]

    def step():
        loss = m(batches[count[0] % len(batches)], train_pv=False)
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


def plan_line(m):
    plan = [p for k, p in m._plans.items() if k[0] != 'eval'][-1]
    out = _lib.PsRtmBwdPlan()
    _lib.check(_lib.load().ps_rtm_backward_plan(C.byref(plan.desc), C.byref(out)), 'ps_rtm_backward_plan')
    return ' '.join('%s=%d' % (n, getattr(out, n)) for n, _ in out._fields_)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', default=','.join(MODELS))
    o = ap.parse_args()
    names = o.only.split(',')
    assert all(n in MODELS for n in names), names
    if not torch.cuda.is_available():
        raise SystemExit("bench_frozen_rtm: no GPU (a timing needs one)")
    built = {n: product_step(n) for n in names}
    for n in names:
        timed(built[n][1], o.warmup)
    res = {n: [] for n in names}
    for r in range(o.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            ms = timed(built[n][1], o.steps)
            res[n].append(ms)
            print(json.dumps(dict(model=n, round=r, ms_per_step=round(ms, 4))), flush=True)
    print('# median of %d rounds, %d steps each, B=%d K=%d R=%d+%d WL=%d d=%d H=%d V=%d dropout 0.1 corrupt 0.9'
          % (o.rounds, o.steps, B, K, U, I, WL, d, H, V))
    for n in names:
        print('%-14s %8.4f ms/step  (min %.4f, max %.4f)' % (n, statistics.median(res[n]), min(res[n]), max(res[n])))
    for n in names:
        print('# plan %-14s %s' % (n, plan_line(built[n][0])))


if __name__ == '__main__':
    main()
