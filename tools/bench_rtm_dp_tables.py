#!/usr/bin/env python3
"""Data-parallel review-transformer step, two ranks: the dense exchange against the one-message row exchange
(``make_exchange(mode='tables')``), same pair of processes, alternating.

A two-rank gloo DRY RUN on one GPU (both ranks on cuda:0; gloo stages every collective through the host, so the figures say
what the exchange costs on this path and little about xGMI — no N > 1 RCCL number exists).  Shape: C4 with the pv encoder
and the per-position user / item tables (BASELINE configs[3]: B = 256 per rank, K = 5, 20 + 30 reviews, d = 128, 8 heads,
ff 512, one layer, dropout 0.1, V = 32,387, 296 k reviews, 100 k users, 60 k products).  Two models per rank:

    dense    row_sparse_adam off, the default dense exchange (``ShardedAdamExchange``)
    tables   row_sparse_adam on, ``TablesGradExchange``: four tables in one message, one all-gather

``--steps`` training steps (forward, backward, exchange, optimizer) between two synchronisations, after warm-up, in
alternating rounds; rank 0 prints one JSON line per model and round, the medians, the message's bytes per rank against the
flat gradient's, and the durations of ``ps_pack_tables``, the union's three launches and ``ps_merge_tables`` from event
pairs bound to the dispatches (``ps_ktimer_arm``; a pass of ``--steps`` steps per kernel).

    python tools/bench_rtm_dp_tables.py [--steps 20] [--warmup 5] [--rounds 5]

Started without RANK / WORLD_SIZE it starts its two ranks itself and waits for them with a timeout.
"""
import argparse
import ctypes as C
import datetime
import json
import os
import socket
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, K, U, I, WL, d, H, V, RC, Q = 256, 5, 20, 30, 100, 128, 8, 32387, 296000, 8
USERS, PRODUCTS = 100000, 60000
KERNELS = ('pack_tables', 'union_mark', 'union_count', 'union_emit', 'merge_tables')


def launch(argv):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
        env.pop('PS_DP_EXCHANGE', None)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    rc = 0
    for p in procs:
        try:
            rc |= p.wait(timeout=540)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise SystemExit("bench_rtm_dp_tables: a rank did not finish in time; both were killed")
    raise SystemExit(rc)


def build(rows, rank):
    import torch
    from prodsearch_amd import ProductRanker, build_optim, default_args, dist as pdist, rtm_data, synth
    a = default_args(model_name='review_transformer', review_encoder_name='pv', embedding_size=d, heads=H, ff_size=512,
                     inter_layers=1, neg_per_pos=K, dropout=0.1, lr=0.0005, review_word_limit=WL, uprev_review_limit=U,
                     iprev_review_limit=I, use_user_emb=True, use_item_emb=True, row_sparse_adam=rows, batch_size=B,
                     max_query_len=Q)
    wd = synth.make_word_dists(V)
    rng = synth.rng_for(5)
    rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, WL)))
    rw[-1] = V - 1
    torch.manual_seed(1234)
    m = ProductRanker(a, 'cuda', V, RC, PRODUCTS, USERS, rw, None, word_dists=wd)
    m._seed = pdist.rank_seed(m._seed, rank)
    opt = build_optim(a, m, None)
    exchange = pdist.make_exchange(m, opt, mode='tables' if rows else None)
    batches = [rtm_data.make_rtm_batch(100 + 10 * rank + s, B, K, RC, V, rw, Q=Q, u_lim=U, i_lim=I, W=1, train_pv=False,
                                       encoder='pv', word_dists=wd, user_size=USERS, product_size=PRODUCTS).to('cuda')
               for s in range(4)]
    m.train()
    count = [0]

    def step():
        loss = m(batches[count[0] % len(batches)], train_pv=False)
        count[0] += 1
        m.zero_grad()
        loss.backward()
        exchange()
        opt.step()
    return m, exchange, step


def timed(step, steps):
    import torch
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
    o = ap.parse_args()
    if 'RANK' not in os.environ:
        launch(sys.argv[1:])
    import torch
    import torch.distributed as td
    from prodsearch_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_rtm_dp_tables: no GPU (a timing needs one)")
    rank = int(os.environ['RANK'])
    torch.cuda.set_device(0)
    td.init_process_group(backend='gloo', rank=rank, world_size=int(os.environ['WORLD_SIZE']),
                          timeout=datetime.timedelta(seconds=120))
    say = (lambda *a: print(*a, flush=True)) if rank == 0 else (lambda *a: None)
    names = ('dense', 'tables')
    built = {'dense': build(False, rank), 'tables': build(True, rank)}
    for n in names:
        timed(built[n][2], o.warmup)
    res = {n: [] for n in names}
    for r in range(o.rounds):
        for n in (names if r % 2 == 0 else names[::-1]):       # (the same order on every rank: the steps hold collectives)
            ms = timed(built[n][2], o.steps)
            res[n].append(ms)
            say(json.dumps(dict(model=n, round=r, ms_per_step=round(ms, 4))))
    say('# two ranks, gloo, one GPU: median of %d rounds, %d steps each; B=%d per rank K=%d R=%d+%d d=%d V=%d reviews=%d '
        'users=%d products=%d dropout 0.1, no PV loss' % (o.rounds, o.steps, B, K, U, I, d, V, RC, USERS, PRODUCTS))
    for n in names:
        say('%-7s %8.4f ms/step  (min %.4f, max %.4f)' % (n, statistics.median(res[n]), min(res[n]), max(res[n])))
    m, exchange, step = built['tables']
    flat = built['dense'][0]._grad_flat.numel() * 4
    say('# message %d bytes per rank (capacities %s rows), flat gradient %d bytes: %.1f %%'
        % (exchange.message_bytes(), exchange._caps, flat, 100.0 * exchange.message_bytes() / flat))
    m.check_index_errors()
    say('# union ' + ' '.join('%s=%d/%d' % (k, v.numel(), dict(m.named_parameters())[k].shape[0])
                              for k, v in m.touched_rows().items()))
    lib = _lib.load()
    for tag in KERNELS:
        _lib.check(lib.ps_ktimer_arm(tag.encode(), o.steps), 'ps_ktimer_arm')
        for _ in range(o.steps):
            step()
        avg, mn, n = C.c_double(), C.c_double(), C.c_int32()
        _lib.check(lib.ps_ktimer_read(C.byref(avg), C.byref(mn), C.byref(n)), 'ps_ktimer_read')
        say('# kernel %-13s avg %.2f us, min %.2f us over %d launches' % (tag, avg.value, mn.value, n.value))
    td.barrier()
    td.destroy_process_group()


if __name__ == '__main__':
    main()
