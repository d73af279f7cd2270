"""One rank of the one-message row exchange's tests (tests/test_gpu_dp_tables.py): started as a FRESH process per rank
(nothing touches the GPU before the rendezvous), gloo over 127.0.0.1, every rank on cuda:0, the process group created with
a timeout of 120 s so that a rank that dies cannot leave its peers waiting for long.  Runs the trainer's call order
(trainer.py:74-78) on its slice of the global batch and writes parameters, the last loss, rank 0's touched lists and the
collectives each exchange entered to <out>.rank<r>.npz."""
import argparse
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))

V, RC, K, U, I, Q, W, PRODUCTS, USERS = 3000, 2500, 3, 6, 8, 6, 2, 50, 60        # dp_worker.run_rtm's sizes


class CollectiveCounter(object):
    """Counts the collectives entered through torch.distributed's all_reduce / all_gather_into_tensor / all_gather."""

    def __init__(self):
        import torch.distributed as td
        self.counts = dict(all_reduce=0, all_gather=0)
        for name, key in (('all_reduce', 'all_reduce'), ('all_gather_into_tensor', 'all_gather'), ('all_gather', 'all_gather')):
            setattr(td, name, self._wrap(getattr(td, name), key))

    def _wrap(self, fn, key):
        def counted(*a, **k):
            self.counts[key] += 1
            return fn(*a, **k)
        return counted

    def take(self):
        out = (self.counts['all_reduce'], self.counts['all_gather'])
        self.counts = dict(all_reduce=0, all_gather=0)
        return out


def run_rtm(Bg, pv_steps, rank, world, exchange_factory, ragged=0, counter=None):
    """Review transformer, pv encoder with user and item tables (four row-sparse tables), dropout and corruption 0.
    ``pv_steps``: one entry per step, whether it is a PV step.  ``ragged``: the LAST rank's batch is that many rows short."""
    import copy
    import numpy as np
    import torch
    from prodsearch_amd import ProductRanker, build_optim, default_args, synth, rtm_data
    per = Bg // world
    a = default_args(model_name='review_transformer', review_encoder_name='pv', embedding_size=128, heads=8, ff_size=512,
                     inter_layers=1, neg_per_pos=K, dropout=0.0, corrupt_rate=0.0, lr=0.002, review_word_limit=40,
                     uprev_review_limit=U, iprev_review_limit=I, use_user_emb=True, use_item_emb=True, row_sparse_adam=True,
                     pv_window_size=W, batch_size=per, max_query_len=Q)
    wd = synth.make_word_dists(V)
    rng = synth.rng_for(17)
    rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, 40)))
    rw[-1] = V - 1
    torch.manual_seed(4321)
    m = ProductRanker(a, 'cuda', V, RC, PRODUCTS, USERS, rw, None, word_dists=wd)
    optim = build_optim(a, m, None)
    exchange = exchange_factory(m, optim)
    lo, hi = rank * per, (rank + 1) * per - (ragged if rank == world - 1 else 0)
    batches = {}
    for pv in sorted(set(pv_steps)):
        batch = rtm_data.make_rtm_batch(91 + int(pv), Bg, K, RC, V, rw, Q=Q, u_lim=U, i_lim=I, W=W, train_pv=pv, encoder='pv',
                                        word_dists=wd, user_size=USERS, product_size=PRODUCTS)
        b = copy.copy(batch)
        for k, v in vars(batch).items():
            if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == Bg:
                setattr(b, k, v[lo:hi].contiguous())
        batches[pv] = b.to('cuda')
    m.train()
    collectives = []
    for pv in pv_steps:
        loss = m(batches[pv], train_pv=pv)
        m.zero_grad()
        loss.backward()
        if counter is not None:
            counter.take()
        exchange()
        if counter is not None:
            collectives.append(counter.take())
        optim.step()
    torch.cuda.synchronize()
    m.check_index_errors()
    out = {'__loss': np.float32(float(loss.detach()))}
    if collectives:
        out['__collectives'] = np.array(collectives, dtype=np.int64)
    for name, rows in m.touched_rows().items():
        out['__touched__' + name] = rows.cpu().numpy()
    for n, p in m.named_parameters():
        out[n] = p.detach().cpu().numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='rtm')
    ap.add_argument('--xmode', default='tables')                # 'tables' or 'default' (what make_exchange gives without a mode)
    ap.add_argument('--global-batch', type=int, default=64)
    ap.add_argument('--pv-steps', default='0,0')                # one 0 / 1 per step: a PV step or not
    ap.add_argument('--ragged', type=int, default=0)
    ap.add_argument('--out', required=True)
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.distributed as td
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    torch.cuda.set_device(0)
    td.init_process_group(backend='gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    counter = CollectiveCounter()
    from prodsearch_amd import dist as pdist
    mode = 'tables' if a.xmode == 'tables' else None
    factory = lambda m, o: pdist.make_exchange(m, o, mode=mode)
    pv_steps = [bool(int(x)) for x in a.pv_steps.split(',')]
    if a.model == 'rtm':
        out = run_rtm(a.global_batch, pv_steps, rank, world, factory, ragged=a.ragged, counter=counter)
    else:
        import dp_worker
        out = dp_worker.run('sparse', a.global_batch, len(pv_steps), rank, world, factory)
    np.savez(a.out + '.rank%d.npz' % rank, **out)
    td.barrier()
    td.destroy_process_group()


if __name__ == '__main__':
    main()
