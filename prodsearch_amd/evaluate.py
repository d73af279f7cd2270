"""Full-catalogue evaluation on the device: what ``Trainer.test`` / ``validate`` compute with
``test_candi_size < 1`` (trainer.py:125-226) — every product scored for every (user, query) row, top-``cutoff``
ranklist, MRR and P@1 — without re-encoding the sequence per candidate chunk and without moving the score matrix to the
host.  ``rank_all`` = ``ps_tem_encode`` (one encode per row) + ``ps_rank_all`` (fp32 MFMA GEMM per table panel, radix-select
top-k, rank of the target)."""
import numpy as np
import torch

from . import _lib


def _rank_all_sharded(model, batch, topk):
    """``rank_all`` over a row-sharded item table (``args.shard_tables``, sharded.py): a COLLECTIVE — every rank calls it with a
    batch of the same size.  Each rank encodes its own rows (the history rows come from their owners), the encodings, targets and
    target scores are all-gathered, every rank ranks ALL rows against its shard (``ps_rank_shard``: top-k with catalogue ids and
    the number of its rows ahead of each target), the counts are summed and the W top-k lists merged by (score desc, id asc) —
    the order ``ps_rank_all`` uses on one table."""
    import torch.distributed as dist
    lib = _lib.load()
    sh = model._shard
    W, r = sh.world, sh.rank
    if model.args.sim_func == 'bias_product':
        raise NotImplementedError("rank_all over a sharded table with sim_func='bias_product'")
    was_training = model.training
    model.eval()
    try:
        enc = model.encode(batch)
    finally:
        model.train(was_training)
    B, d = enc.shape
    dev = enc.device
    st = torch.cuda.current_stream(dev).cuda_stream
    P = model.product_size
    target = batch.target_prod_idxs.contiguous()
    # the target's score through the SAME product kernel that scores the shards: q . T^T over the fetched target rows, diagonal
    trows = sh.table_buf[model.__dict__['_shard_eval_target_slots']].contiguous()
    tt = torch.empty(B, B, device=dev, dtype=torch.float32)
    _lib.check(lib.ps_gemm_f32(enc.data_ptr(), d, 0, trows.data_ptr(), d, 0, tt.data_ptr(), B, B, B, d, None, 1.0, 0, st),
               'ps_gemm_f32')
    ok = (target >= 0) & (target < P)
    tscore = torch.where(ok, tt.diagonal(), torch.full_like(tt.diagonal(), float('inf'))).contiguous()
    if W > 1:
        encs = torch.empty(W * B, d, device=dev, dtype=torch.float32)
        tgts = torch.empty(W * B, device=dev, dtype=torch.int64)
        tscs = torch.empty(W * B, device=dev, dtype=torch.float32)
        dist.all_gather_into_tensor(encs, enc.contiguous(), group=sh.group)
        dist.all_gather_into_tensor(tgts, target, group=sh.group)
        dist.all_gather_into_tensor(tscs, tscore, group=sh.group)
    else:
        encs, tgts, tscs = enc.contiguous(), target, tscore
    n_mine = (P - r + W - 1) // W                              # catalogue rows i < P with i % W == r
    k = int(topk)
    NB = W * B
    nbytes = lib.ps_rank_scratch_bytes(NB, n_mine, d, k)
    if nbytes < 0:
        raise RuntimeError("rank_all: unsupported sizes (topk must be 1..256)")
    scratch = model.__dict__.get('_rank_scratch')
    if scratch is None or scratch.numel() < nbytes:
        scratch = model.__dict__['_rank_scratch'] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    top_idx = torch.empty(NB, k, dtype=torch.int64, device=dev)
    top_score = torch.empty(NB, k, dtype=torch.float32, device=dev)
    ahead = torch.zeros(NB, dtype=torch.int32, device=dev)
    _lib.check(lib.ps_rank_shard(encs.data_ptr(), NB, d, sh.weight.data_ptr(), n_mine, None, tgts.data_ptr(), tscs.data_ptr(),
                                 W, r, k, top_idx.data_ptr(), top_score.data_ptr(), ahead.data_ptr(), scratch.data_ptr(),
                                 scratch.numel(), st), 'ps_rank_shard')
    if W > 1:
        all_idx = torch.empty(W, NB, k, dtype=torch.int64, device=dev)
        all_sc = torch.empty(W, NB, k, dtype=torch.float32, device=dev)
        dist.all_gather_into_tensor(all_idx.view(W * NB, k), top_idx, group=sh.group)
        dist.all_gather_into_tensor(all_sc.view(W * NB, k), top_score, group=sh.group)
        dist.all_reduce(ahead, group=sh.group)
        mine = slice(r * B, (r + 1) * B)
        ci = all_idx[:, mine].permute(1, 0, 2).reshape(B, W * k)
        cs = all_sc[:, mine].permute(1, 0, 2).reshape(B, W * k)
        key = torch.where(ci >= 0, ci, torch.full_like(ci, P + 1))          # unfilled slots last among equal (-inf) scores
        o1 = torch.argsort(key, dim=1, stable=True)
        ci, cs = torch.gather(ci, 1, o1), torch.gather(cs, 1, o1)
        o2 = torch.argsort(cs, dim=1, descending=True, stable=True)
        top_idx, top_score = torch.gather(ci, 1, o2)[:, :k].contiguous(), torch.gather(cs, 1, o2)[:, :k].contiguous()
        ahead = ahead[mine]
    rank = torch.where(ok, 1 + ahead, torch.zeros_like(ahead)).to(torch.int32)
    return top_idx, top_score, rank


def rank_all(model, batch, topk=100):
    """-> (top_idx [B,k] int64, top_score [B,k] fp32, rank [B] int32; 1-based, 0 = target not a product), on device."""
    if getattr(model, '_shard', None) is not None:
        return _rank_all_sharded(model, batch, topk)
    lib = _lib.load()
    was_training = model.training
    model.eval()
    try:
        enc = model.encode(batch)
    finally:
        model.train(was_training)
    B, d = enc.shape
    P = model.product_size
    table = model.product_emb.weight                       # rows 0..P-1; the pad row P is not a candidate
    bias = model.product_bias if model.args.sim_func == 'bias_product' else None
    target = batch.target_prod_idxs
    if not (torch.is_tensor(target) and target.is_cuda and target.dtype == torch.int64):
        raise RuntimeError("batch.target_prod_idxs must be an int64 tensor on the model's device")
    k = int(topk)
    nbytes = lib.ps_rank_scratch_bytes(B, P, d, k)
    if nbytes < 0:
        raise RuntimeError("rank_all: unsupported sizes (topk must be 1..256)")
    scratch = getattr(model, '_rank_scratch', None)
    if scratch is None or scratch.numel() < nbytes:
        scratch = model.__dict__['_rank_scratch'] = torch.empty(nbytes, dtype=torch.uint8, device=enc.device)
    top_idx = torch.empty(B, k, dtype=torch.int64, device=enc.device)
    top_score = torch.empty(B, k, dtype=torch.float32, device=enc.device)
    rank = torch.empty(B, dtype=torch.int32, device=enc.device)
    _lib.check(lib.ps_rank_all(enc.data_ptr(), B, d, table.data_ptr(), P, _lib.ptr(bias), target.contiguous().data_ptr(), k,
                               top_idx.data_ptr(), top_score.data_ptr(), rank.data_ptr(), scratch.data_ptr(),
                               scratch.numel(), torch.cuda.current_stream(enc.device).cuda_stream), 'ps_rank_all')
    return top_idx, top_score, rank


def _rank_rtm(fn, model, index, batch, topk, return_scores, attr, extra, shapes, nbytes, launch, width, timeline=False):
    """The common work of ``rank_all_rtm`` / ``rank_candidates_rtm`` / ``rank_seq_rtm`` (``fn`` in the messages): refusal, the
    index's owner and staleness, the batch's fields, the descriptor, a scratch of exactly the entry's size cached on the model
    under ``attr``, the outputs.  What differs comes from the caller: ``extra`` — its further batch fields as (name, dims,
    required), [B, ...] each — and ``shapes``, the shape refusal's wording; ``nbytes(lib, desc, sh, k, *x)`` the entry's
    ``*_scratch_bytes``, ``width(*x)`` the columns of the dense scores and ``launch(lib, head, qw, ur, target, tail, *x)``
    the entry itself, with ``x`` the extra fields' tensors (None for an absent optional one), ``head`` = (desc, shape,
    tensors, index) and ``tail`` = (topk, top_idx, top_score, rank, scores, scratch, its bytes, stream)."""
    kind = 'timeline' if timeline else 'catalogue'
    msg = model._rank_all_refusal(time_ordered=timeline)
    if msg is not None:
        raise NotImplementedError(msg)
    if index.model is not model:
        raise RuntimeError("%s: the %s index belongs to another model" % (fn, kind))
    if index.stale():
        raise RuntimeError("%s: stale %s index — a weight, a table or the %s changed since "
                           "model.%s_index() built it; build it again" % (fn, kind, kind, kind))
    for name, _, required in extra:
        if required and getattr(batch, name, None) is None:
            raise RuntimeError("%s: the batch carries no %s" % (fn, name))
    lib = _lib.load()
    qw = model._idx(batch.query_word_idxs, 'query_word_idxs')
    ur = model._idx(batch.u_ridxs, 'u_ridxs')
    target = model._idx(batch.target_prod_idxs, 'target_prod_idxs')
    x = [model._idx(getattr(batch, name, None), name) for name, _, _ in extra]
    B, Q = qw.shape
    if ur.dim() != 2 or ur.shape[0] != B or target.shape != (B,) or \
            any(t is not None and (t.dim() != dims or t.shape[0] != B) for t, (_, dims, _) in zip(x, extra)):
        raise RuntimeError("%s: %s" % (fn, shapes))
    ps, _ = model._structs()
    desc, sh = model._rank_all_desc(B, Q, ur.shape[1], index.shape3)
    k = int(topk)
    dev = qw.device
    n = nbytes(lib, desc, sh, k, *x)
    if n < 0:
        raise RuntimeError("%s: %s" % (fn, lib.ps_last_error().decode('utf-8', 'replace')))
    # exactly n bytes: the C entry sizes its passes from the scratch it is given, so the buffer is part of the result's shape
    scratch = model.__dict__.get(attr)
    if scratch is None or scratch.numel() != n or scratch.device != dev:
        scratch = model.__dict__[attr] = torch.empty(n, dtype=torch.uint8, device=dev)
    top_idx = torch.empty(B, k, dtype=torch.int64, device=dev)
    top_score = torch.empty(B, k, dtype=torch.float32, device=dev)
    rank = torch.empty(B, dtype=torch.int32, device=dev)
    scores = torch.empty(B, width(*x), dtype=torch.float32, device=dev) if return_scores else None
    head = (desc, sh, ps, index.index.data_ptr())
    tail = (k, top_idx.data_ptr(), top_score.data_ptr(), rank.data_ptr(), _lib.ptr(scores), scratch.data_ptr(), scratch.numel(),
            torch.cuda.current_stream(dev).cuda_stream)
    launch(lib, head, qw.data_ptr(), ur.data_ptr(), target.data_ptr(), tail, *x)
    return (top_idx, top_score, rank, scores) if return_scores else (top_idx, top_score, rank)


def rank_all_rtm(model, index, batch, topk=100, items_per_pass=None, return_scores=False):
    """The review transformer over the whole catalogue (``ps_rtm_rank_all``): what ``Trainer.test`` gets from
    ``model.test`` over chunks of all products plus the host-side ranking, without encoding every (entry, candidate) sequence.
    ``index`` = ``model.catalogue_index(item_ridxs, review_u_p)``; ``batch`` an entries-only batch (``ProdSearchRankBatch``:
    ``query_word_idxs`` [B,Q], ``u_ridxs`` [B,U], ``target_prod_idxs`` [B], on the device).  ``items_per_pass``: bound the
    workspace (default: 32768 pairs per pass).  -> (top_idx [B,k] int64, top_score [B,k], rank [B] int32) as ``rank_all``
    (+ the dense scores [B,P] with ``return_scores``)."""
    return _rank_rtm(
        'rank_all_rtm', model, index, batch, topk, return_scores, '_rtm_rank_scratch',
        (), "u_ridxs must be [B, U] and target_prod_idxs [B]",
        lambda lib, desc, sh, k: lib.ps_rtm_rank_scratch_bytes(desc, sh, k, int(items_per_pass or 0)),
        lambda lib, head, qw, ur, target, tail: _lib.check(
            lib.ps_rtm_rank_all(*head, index.item_ridxs.data_ptr(), qw, ur, target, *tail), 'ps_rtm_rank_all'),
        lambda: index.shape3[0])


def rank_candidates_rtm(model, index, batch, topk=100, cands_per_pass=None, return_scores=False):
    """The review transformer over every entry's OWN candidate list (``ps_rtm_rank_candidates``): what
    ``Trainer._scores_candidates`` gets from ``model.test`` over chunks of the lists plus its ranking chain — validation on
    ``valid_candi_size`` sampled products, the rerank of ``test_candi_size`` lists.  ``index`` as for ``rank_all_rtm``;
    ``batch`` a ``ProdSearchRankBatch`` with ``candi_prod_idxs`` [B, C] (item ids; a slot outside [0, P), the -1 padding of a
    ragged list, is dead).  -> (top_idx [B,k] ITEM ids of the live slots by (score desc, column asc), -1 where unfilled;
    top_score [B,k]; rank [B] int32: 1 + the live slots ahead of the first column holding the target, 0 = not in the list)
    (+ the dense scores [B,C], -inf at dead slots, with ``return_scores``)."""
    return _rank_rtm(
        'rank_candidates_rtm', model, index, batch, topk, return_scores, '_rtm_rank_cand_scratch',
        (('candi_prod_idxs', 2, True),), "u_ridxs must be [B, U], target_prod_idxs [B] and candi_prod_idxs [B, C]",
        lambda lib, desc, sh, k, cand: lib.ps_rtm_rank_cand_scratch_bytes(desc, sh, cand.shape[1], k, int(cands_per_pass or 0)),
        lambda lib, head, qw, ur, target, tail, cand: _lib.check(
            lib.ps_rtm_rank_candidates(*head, index.item_ridxs.data_ptr(), qw, ur, cand.data_ptr(), cand.shape[1], target, *tail),
            'ps_rtm_rank_candidates'),
        lambda cand: cand.shape[1])


def rank_seq_rtm(model, index, batch, topk=100, slots_per_pass=None, return_scores=False):
    """The review transformer's one-pass evaluation in the TIME-ORDERED setting (``ps_rtm_rank_seq``, DESIGN.md §8b.3:
    ``do_seq_review_test`` without ``train_review_only``): a pair reads the ``iprev_review_limit`` reviews of its item written
    up to the entry's time stamp.  ``index`` = ``model.timeline_index(*loader.timeline(), review_u_p)``; ``batch`` a
    ``ProdSearchRankBatch`` with ``time_stamps`` [B] (``ProdSearchDataLoader.seq_rank_batches`` / ``seq_candidate_batches``).
    With ``candi_prod_idxs`` [B, C] the result is ``rank_candidates_rtm``'s over the lists, without them ``rank_all_rtm``'s
    over the catalogue (+ the dense scores [B, C] / [B, P] with ``return_scores``)."""
    def launch(lib, head, qw, ur, target, tail, stamps, cand):
        tl = _lib.PsRtmSeqTimeline(index.ptr.data_ptr(), index.rids.data_ptr(), index.times.data_ptr(), index.rids.numel())
        _lib.check(lib.ps_rtm_rank_seq(*head, tl, qw, ur, stamps.data_ptr(), _lib.ptr(cand), 0 if cand is None else cand.shape[1],
                                       target, *tail), 'ps_rtm_rank_seq')
    return _rank_rtm(
        'rank_seq_rtm', model, index, batch, topk, return_scores, '_rtm_rank_seq_scratch',
        (('time_stamps', 1, True), ('candi_prod_idxs', 2, False)),
        "u_ridxs must be [B, U], target_prod_idxs and time_stamps [B], candi_prod_idxs [B, C]",
        lambda lib, desc, sh, k, stamps, cand: lib.ps_rtm_rank_seq_scratch_bytes(
            desc, sh, _lib.PS_RTM_SEQ_NO_LIST if cand is None else cand.shape[1], k, int(slots_per_pass or 0)),
        launch, lambda stamps, cand: index.shape3[0] if cand is None else cand.shape[1], timeline=True)


def calc_metrics(rank, cutoff=100):
    """``Trainer.calc_metrics`` (trainer.py:172-187) from the 1-based ranks of ``rank_all``."""
    r = torch.as_tensor(rank).detach().cpu().numpy().astype(np.int64)
    hit = (r > 0) & ((cutoff < 0) | (r <= cutoff))
    mrr = float(np.where(hit, 1.0 / np.maximum(r, 1), 0.0).sum() / len(r))
    return mrr, float((r == 1).sum() / len(r))


def ranklist_lines(user_ids, query_idxs, product_ids, top_idx, top_score, tag="ReviewTransformer"):
    """Lines of the TREC-style ranklist ``Trainer.test`` writes (trainer.py:160-170)."""
    ti = torch.as_tensor(top_idx).cpu().numpy()
    ts = torch.as_tensor(top_score).cpu().numpy()
    for i in range(ti.shape[0]):
        for r in range(ti.shape[1]):
            if ti[i, r] < 0:
                break
            yield "%s_%d Q0 %s %d %f %s\n" % (user_ids[i], query_idxs[i], product_ids[int(ti[i, r])], r + 1,
                                              float(ts[i, r]), tag)


def evaluate(model, batches, topk=100, cutoff=100):
    """MRR / P@1 over an iterable of eval batches (``Trainer.test`` without the host-side argsort)."""
    ranks = [rank_all(model, b, topk)[2] for b in batches]
    return calc_metrics(torch.cat(ranks), cutoff)
