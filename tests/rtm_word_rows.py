"""Rows of ``word_embeddings.weight.grad`` of the review transformer, one by one, against the float64 oracle
(tests/test_rtm_word_rows_cpu.py, tests/test_gpu_rtm_word_index.py, tests/test_gpu_rtm_shapes.py, tests/test_gpu_fullsize_rtm.py).
No GPU is needed here.

The word-mean review encoders (pvc, fs, avg) turn the gradient of every review slot into rows of the word table through an
inverted index word -> slots (csrc/rtm_index.hip).  One lost, doubled or misfiled occurrence changes ONE row, and a max-norm
over the whole table does not see a rare word's row beside a frequent word's.  So every row is judged on its own scale.

Per-occurrence contributions.  The oracle keeps the word mean of every review slot with its graph (oracle.rtm: ``mean_pos``,
``mean_neg``); with g_s = d loss / d mean of slot s from the float64 oracle's autograd and n_s the number of words the mean
of s counts (pvc: its non-pad words; fs / avg: the words the batch's mask keeps; at least 1), one occurrence of word w in
slot s adds c = g_s / n_s to row w.  For fs, g_s is taken BEHIND f_W and the tanh (the mean is their input), so the same
decomposition holds for all three encoders and the looser scale the median of the touched rows would give is not needed.
What is left of a row, rest_w = ref_w - sum c, is the query encoder's share and, with train_pv, the PV loss's.

Row metric.  err_w = |got_w - ref_w|_inf / S_w with S_w = sum over the occurrences of |c|_inf + |rest_w|_inf: the scale adds
magnitudes, so a row whose terms cancel is not judged against its small result.  Rows with S_w = 0 must be exactly zero,
and the rows that are not zero must be exactly the words the batch addresses (``addressed_words``).

Bound.  Nothing fixed in advance: YARDSTICK records, per case, the fp32 oracle's worst err_w against the float64 oracle —
the same rounding in another summation order — measured on the CPU, with a tenth on top for another host's order
(tests/test_rtm_word_rows_cpu.py asserts that no run measures more); a product's gradient has to stay within 8 x that (the GPU adds in runs of 64 and through atomics: the same
order of error, with spread), and within 2^-22 where the fp32 oracle happens to be exact.

What the bound can see (asserted for every case on the CPU): ``mutations`` drops or doubles ONE occurrence in the float64
reference — of the case's most frequent word (the occurrence whose |c|_inf is nearest the mean of that word's, S_w / count:
a loss of average size) and of a word that occurs once and is in no query — and the change each makes to err_w is more than
twice the bound.  What no check of values can see is an occurrence far below the word's average: at d = 256 the heavy-word
case scores its negatives near -4, their slots' gradients are 50 times smaller than the positives', and the median
occurrence of the heavy word is a seventh of the mean one.  Such occurrences are covered by the exact checks only."""
import functools
import os
import types

import numpy as np
import torch

import saturated as S

FLOOR = 2.0 ** -22
ZIPF_S = 1.05
HEAVY_WORD, HEAVY_SHARE = 7, 0.7
WR_DET_LIM = 4096             # csrc/rtm_index.hip: words above it take rtm_wreduce_heavy_det_kernel in deterministic mode
RTM_HIST_MAXV, RTM_HIST_G = 38000, 256      # csrc/rtm.h


def _cut(rng, rw, V, lo):
    WL = rw.shape[1]
    lens = torch.from_numpy(rng.integers(lo, WL + 1, size=rw.shape[0]))
    rw[torch.arange(WL)[None, :] >= lens[:, None]] = V - 1
    return rw


def zipf_words(rng, V, RC, WL, s=ZIPF_S):
    """Review words with Zipf frequencies (exponent 1.05): a head word with hundreds of occurrences in a batch — repeated
    inside reviews — beside thousands of words that occur once."""
    p = 1.0 / np.arange(1, V) ** s
    return _cut(rng, torch.from_numpy(rng.choice(V - 1, size=(RC, WL), p=p / p.sum())), V, 1)


def flat_zipf_words(rng, V, RC, WL):
    """Exponent 0.6: with 100,000 occurrences over 2,000 words the head word of exponent 1.05 has 15,000 of them, and one
    of 15,000 moves err_w by 6.6e-5 on average, four times the bound with nothing to spare for the smaller ones; here it has
    about 2,000."""
    return zipf_words(rng, V, RC, WL, 0.6)


def heavy_words(rng, V, RC, WL):
    """Uniform words with HEAVY_SHARE of all word slots set to HEAVY_WORD, reviews of 3 WL / 4 .. WL words."""
    rw = torch.from_numpy(rng.integers(0, V - 1, size=(RC, WL)))
    rw[torch.from_numpy(rng.random((RC, WL)) < HEAVY_SHARE)] = HEAVY_WORD
    return _cut(rng, rw, V, 3 * WL // 4)


def _rewrite_words(batch, rw):
    """The batch's review words and masks from its review ids (make_rtm_batch's own rule, train_pv False)."""
    V = int(rw.max()) + 1
    for side in ('pos', 'neg'):
        w = rw[getattr(batch, side + '_prod_ridxs')]
        setattr(batch, side + '_prod_rword_idxs', w.contiguous())
        setattr(batch, side + '_prod_rword_masks', w.ne(V - 1).to(torch.uint8).contiguous())


def clear_a_third_of_the_masks(batch, rw):
    """The word masks of a third of the REAL words (mask 1) cleared: the mean and the index must follow the mask, not the
    pad id.  (A review of one word can lose it: its mean is then 0 / max(0, 1).)"""
    from prodsearch_amd import synth
    rng = synth.rng_for(31)
    for f in ('pos_prod_rword_masks', 'neg_prod_rword_masks'):
        m = getattr(batch, f)
        m[torch.from_numpy(rng.random(tuple(m.shape)) < 1.0 / 3.0) & m.bool()] = 0


def one_real_review(batch, rw):
    """Every review slot the pad review but one (positive row 2, position 0; its review: the longest of the table)."""
    pad = rw.shape[0] - 1
    V = int(rw.max()) + 1
    keep = int(rw.ne(V - 1).sum(1).argmax())
    batch.pos_prod_ridxs.fill_(pad)
    batch.neg_prod_ridxs.fill_(pad)
    batch.pos_prod_ridxs[2, 0] = keep
    batch.pos_seg_idxs[:, 1:] = 3
    batch.neg_seg_idxs[:, :, 1:] = 3
    batch.pos_seg_idxs[2, 1] = 2
    _rewrite_words(batch, rw)


def plant_a_singleton(batch, rw):
    """Word V - 2 exactly once in the batch (100,000 occurrences over 2,000 words leave no word with one): every occurrence
    of it becomes word 0, then the first word of the last real negative review becomes it."""
    V = int(rw.max()) + 1
    for f in ('query_word_idxs', 'pos_prod_rword_idxs', 'neg_prod_rword_idxs'):
        t = getattr(batch, f)
        t[t.eq(V - 2)] = 0
    nw = batch.neg_prod_rword_idxs.view(-1, rw.shape[1])
    real = torch.nonzero(batch.neg_prod_ridxs.reshape(-1).ne(rw.shape[0] - 1) & nw[:, 0].ne(V - 1)).flatten()
    nw[int(real[-1]), 0] = V - 2


_BATCH = dict(B=6, K=2, u_lim=5, i_lim=6, WL=40)          # R = 11
_BIGV = dict(_BATCH, V=RTM_HIST_MAXV + 1, words=zipf_words, encoder='pvc')
_HEAVY = dict(B=8, K=3, u_lim=5, i_lim=6, WL=40, V=1500, words=heavy_words, encoder='pvc')
# name -> (arguments of saturated.rtm_problem, index form, side_fork) — the form ps_rtm_backward_plan names with no switch set
CASES = {
    # above RTM_HIST_MAXV the workspace has no histogram block; the ranks come out of rtm_embed4_kernel (d = 64 / 128 / 256)
    'fc_d64': (dict(_BIGV, d=64, heads=4), 'FWD_COUNTS', 1),
    'fc_d256': (dict(_BIGV, d=256, heads=8), 'FWD_COUNTS', 1),
    'fc_d64_pv': (dict(_BIGV, d=64, heads=4, train_pv=True), 'FWD_COUNTS', 1),      # the index reads pos_prod_rword_idxs_pvc
    'fc_d256_pv': (dict(_BIGV, d=256, heads=8, train_pv=True), 'FWD_COUNTS', 1),
    # ... and where that kernel is not taken the index is counted, allocated and filled behind the embed backward
    'late_d32': (dict(_BIGV, d=32, heads=4), 'LATE', 0),
    'late_d512': (dict(_BIGV, d=512, heads=8), 'LATE', 0),
    # the LDS histogram at its largest: 152,000 B of dynamic LDS
    'hist_limit': (dict(_BIGV, d=64, heads=4, V=RTM_HIST_MAXV), 'HIST', 1),
    # B (K + 1) R = 264,600 review rows: 1,034 per partition, a second list of rtm_hist_kernel<.., 1024, 0>
    'hist_two_lists': (dict(B=700, K=5, u_lim=30, i_lim=33, WL=3, d=32, heads=4, V=2000, RC=5000, words=flat_zipf_words,
                            encoder='pvc', edit=plant_a_singleton), 'HIST', 1),
    # one word with more than WR_DET_LIM occurrences, repeated inside every review; NK = 2 / 4 / 8 of the ordered reduce
    'heavy_d64': (dict(_HEAVY, d=64, heads=4), 'HIST', 1),
    'heavy_d256': (dict(_HEAVY, d=256, heads=8), 'HIST', 1),
    'heavy_d512': (dict(_HEAVY, d=512, heads=8), 'HIST', 1),
    'masks_avg': (dict(_BATCH, d=64, heads=4, encoder='avg', edit=clear_a_third_of_the_masks), 'HIST', 1),
    'masks_fs': (dict(_BATCH, d=64, heads=4, encoder='fs', edit=clear_a_third_of_the_masks), 'HIST', 1),
    'one_review': (dict(_BATCH, d=64, heads=4, encoder='pvc', edit=one_real_review), 'HIST', 1),
    'one_review_wl1': (dict(_BATCH, d=64, heads=4, encoder='pvc', edit=one_real_review, WL=1), 'HIST', 1),
    'wl1': (dict(_BATCH, d=64, heads=4, encoder='pvc', WL=1), 'HIST', 1),
}
# tests/test_gpu_rtm_shapes.py's word-mean shapes (saturated.rtm_problem's own vocabulary and words)
SHAPE_CASES = {
    'shape_d256_pvc': dict(d=256, heads=8, B=6, K=2, u_lim=5, i_lim=6, WL=40, encoder='pvc'),
    'shape_d512_pvc': dict(d=512, heads=8, B=3, K=2, u_lim=4, i_lim=3, WL=70, encoder='pvc'),
    'shape_d256_avg': dict(d=256, heads=8, B=5, K=3, u_lim=3, i_lim=4, WL=30, encoder='avg'),
    'shape_d64_pvc': dict(d=64, heads=4, B=7, K=1, u_lim=7, i_lim=6, WL=100, encoder='pvc'),
    'shape_d128_pvc': dict(d=128, heads=8, B=9, K=4, u_lim=9, i_lim=4, WL=128, encoder='pvc'),
}
for _n, _kw in SHAPE_CASES.items():
    CASES[_n] = (_kw, 'HIST', 1)

# The fp32 oracle's worst err_w against the float64 oracle, measured on the CPU with 1, 4 and all threads (they differ only
# where a row has thousands of terms).  Recorded: 1.1 x the largest of the three, rounded up to two digits — another host's
# fp32 kernels add in another order (saturated.py's d = 256 case moved by 6 % between two hosts), and a yardstick recorded to
# the last digit of one host would fail tests/test_rtm_word_rows_cpu.py on the next; that test measures with one thread,
# which repeats.  The GPU bound of a case is max(8 x the recorded value, FLOOR).
#                  recorded     measured: 1 thread / 4 / all
YARDSTICK = {
    'fc_d64': 1.2e-6,            # 1.04e-6 all three
    'fc_d256': 1.9e-6,           # 1.64e-6
    'fc_d64_pv': 2.0e-6,         # 1.79e-6
    'fc_d256_pv': 1.1e-5,        # 9.27e-6
    'late_d32': 1.2e-6,          # 1.03e-6
    'late_d512': 3.6e-6,         # 3.20e-6 / 2.28e-6 / 2.28e-6
    'hist_limit': 1.2e-6,        # 1.01e-6
    'hist_two_lists': 1.4e-6,    # 1.27e-6
    'heavy_d64': 5.5e-6,         # 4.31e-6 / 3.01e-6 / 4.96e-6 (4,872 occurrences of one word)
    'heavy_d256': 4.1e-6,        # 3.64e-6 / 1.91e-6 / 2.60e-6
    'heavy_d512': 8.8e-6,        # 7.92e-6 / 6.53e-6 / 6.53e-6
    'masks_avg': 1.6e-6,         # 1.43e-6
    'masks_fs': 4.4e-6,          # 3.96e-6
    'one_review': 5.1e-7,        # 4.60e-7
    'one_review_wl1': 3.9e-7,    # 3.49e-7
    'wl1': 1.8e-6,               # 1.61e-6
    'shape_d256_pvc': 2.3e-6,    # 2.01e-6
    'shape_d512_pvc': 5.0e-6,    # 3.82e-6 / 4.52e-6 / 3.37e-6
    'shape_d256_avg': 2.1e-6,    # 1.82e-6
    'shape_d64_pvc': 1.1e-6,     # 9.82e-7
    'shape_d128_pvc': 9.7e-7,    # 8.77e-7
}
# tests/test_gpu_fullsize_rtm.py's pvc case, on its 128 sampled rows (fullsize_sample, fp32_rows): measured 3.999e-7 at 1 / 4 / all threads
YARDSTICK_FULLSIZE = 4.4e-7


def bound(name):
    return max(8.0 * YARDSTICK[name], FLOOR)


def hist_switch_off():
    return os.environ.get('PS_RTM_HIST', '1') == '0'


def expected_plan(name):
    """(index form, side_fork) of a case, as the _lib constants; under PS_RTM_HIST=0 a HIST case takes the form the switch
    selects: the forward's counts where rtm_embed4_kernel embeds (d = 64 / 128 / 256, WL <= 128), the late index elsewhere."""
    from prodsearch_amd import _lib
    kw, form, fork = CASES[name]
    if form == 'HIST' and hist_switch_off():
        form = 'FWD_COUNTS' if (kw['d'] in (64, 128, 256) and kw['WL'] <= 128) else 'LATE'
        fork = 1 if form == 'FWD_COUNTS' else 0
    return getattr(_lib, 'PS_RTM_INDEX_' + form), fork


@functools.lru_cache(maxsize=None)
def problem(name):
    return S.rtm_problem(**CASES[name][0])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(problem, float64 oracle step, its decomposition) of a case; computed once per process and shared — nobody writes
    to it."""
    p = problem(name)
    r64 = S.rtm_oracle_step(p, p.sd, True)
    return p, r64, decompose(p, r64)


def plan_desc(p):
    """The descriptor ProductRanker._desc builds for the problem's training step (host only)."""
    from prodsearch_amd import _lib
    a, d = p.a, _lib.PsRtmDesc()
    R = p.batch.pos_prod_ridxs.shape[1]
    d.B, d.K, d.R, d.Q, d.W, d.C = p.B, p.K, R, p.batch.query_word_idxs.shape[1], 1, 0
    d.WL = slot_words(p)[0].shape[1]
    d.d, d.H, d.F, d.n_layers = a.embedding_size, a.heads, a.ff_size, a.inter_layers
    d.vocab_size, d.review_count = p.V, p.RC
    d.review_encoder = dict(pv=_lib.PS_RENC_PV, pvc=_lib.PS_RENC_PVC, fs=_lib.PS_RENC_FS, avg=_lib.PS_RENC_AVG)[a.review_encoder_name]
    d.query_encoder = _lib.PS_QENC_FS if a.query_encoder_name == 'fs' else _lib.PS_QENC_AVG
    d.use_pos_emb, d.use_seg_emb, d.pos_weight = int(a.use_pos_emb), int(a.use_seg_emb), int(a.pos_weight)
    d.train_pv, d.training = int(p.train_pv), 1
    d.dropout, d.corrupt_rate = float(a.dropout), float(a.corrupt_rate)
    d.user_size, d.product_size = 60, 50
    return d


def backward_plan(desc):
    import ctypes as C
    from prodsearch_amd import _lib
    out = _lib.PsRtmBwdPlan()
    _lib.check(_lib.load().ps_rtm_backward_plan(C.byref(desc), C.byref(out)), 'ps_rtm_backward_plan')
    return out


# ------------------------------------------------------------------------------------------------------ the decomposition
def slot_words(p):
    """(word ids [NS, WL], counted [NS, WL] bool, real [NS] bool) of the review slots the encoder averages: the positives'
    B R slots, then the negatives' B K R, as oracle.rtm's ``mean_pos`` / ``mean_neg`` order them.  counted: the word is in
    its slot's mean; real: the slot holds a review (the product indexes real reviews only; a pad review has no counted
    word anyway)."""
    b, enc = p.batch, p.a.review_encoder_name
    if enc == 'pvc' and p.train_pv:
        pw, nw = b.pos_prod_rword_idxs_pvc, b.neg_prod_rword_idxs_pvc
    else:
        pw, nw = b.pos_prod_rword_idxs, b.neg_prod_rword_idxs
    WL = pw.shape[-1]
    idx = torch.cat([pw.reshape(-1, WL), nw.reshape(-1, WL)], 0)
    if enc == 'pvc':
        ok = idx.ne(p.V - 1)
    else:
        ok = torch.cat([b.pos_prod_rword_masks.reshape(-1, WL), b.neg_prod_rword_masks.reshape(-1, WL)], 0).bool()
    real = torch.cat([b.pos_prod_ridxs.reshape(-1), b.neg_prod_ridxs.reshape(-1)]).ne(p.RC - 1)
    return idx, ok, real


def addressed_words(p):
    """The words the batch addresses, from its index tensors alone: query words, counted words of real reviews and, with
    train_pv, the PV loss's target and sampled words of real reviews — minus the pad word."""
    b = p.batch
    idx, ok, real = slot_words(p)
    parts = [b.query_word_idxs.reshape(-1), idx[ok & real[:, None]]]
    if p.train_pv:
        preal = b.pos_prod_ridxs.reshape(-1).ne(p.RC - 1)
        W = b.pos_prod_rword_idxs.shape[-1]
        tgt, tm = b.pos_prod_rword_idxs.reshape(-1, W), b.pos_prod_rword_masks.reshape(-1, W).bool()
        parts += [tgt[tm & preal[:, None]], p.neg_words[preal & tm.any(1)].reshape(-1)]
    w = torch.unique(torch.cat(parts))
    return w[w.ne(p.V - 1)]


def decompose(p, r64, rows=None):
    """The float64 reference of the word table, row by row.  ``rows``: only these word ids (a sorted int64 tensor of words
    that are in no query and no PV loss: their reference rows are sum c, built here without a table-sized gradient);
    None: every row, from the oracle's gradient of the table.  Returns a namespace:
      rows [n] word ids, ref [n, d] float64, scale [n] S_w, count [n] occurrences, occ_row / occ_slot [N] (row position
      and slot of every occurrence, grouped by nothing), c [NS, d] per-slot contribution, rest [n] |rest_w|_inf."""
    idx, ok, real = slot_words(p)
    g = torch.cat([t.double() for t in r64['slot_grads']], 0)
    counted = ok.sum(1).clamp(min=1)
    c = g / counted[:, None].double()
    live = ok & real[:, None]
    slot = torch.arange(idx.shape[0])[:, None].expand_as(idx)[live]
    word = idx[live]
    if rows is None:
        n = p.V
        occ_row = word
        rows_t = torch.arange(n)
    else:
        rows_t = rows
        pos = torch.searchsorted(rows_t, word).clamp(max=rows_t.numel() - 1)
        hit = rows_t[pos].eq(word)
        slot, occ_row, n = slot[hit], pos[hit], rows_t.numel()
    d = c.shape[1]
    cn = c.abs().amax(1)
    summed = torch.zeros(n, d, dtype=torch.float64).index_add_(0, occ_row, c[slot])
    occ_scale = torch.zeros(n, dtype=torch.float64).index_add_(0, occ_row, cn[slot])
    count = torch.zeros(n, dtype=torch.int64).index_add_(0, occ_row, torch.ones_like(occ_row))
    ref = r64['grads']['word_embeddings.weight'].double() if rows is None else summed
    rest = (ref - summed).abs().amax(1)
    return types.SimpleNamespace(rows=rows_t, ref=ref, scale=occ_scale + rest, count=count, occ_row=occ_row, occ_slot=slot,
                                 c=c, cn=cn, rest=rest, occ_scale=occ_scale)


def row_errors(got, dec, ref=None):
    """err_w of every row of ``dec`` (0 where S_w = 0: those rows are compared exactly, ``compare``)."""
    ref = dec.ref if ref is None else ref
    diff = (got.double() - ref).abs().amax(1)
    return torch.where(dec.scale > 0, diff / dec.scale.clamp(min=1e-300), torch.zeros_like(diff))


def compare(got, dec, limit, addressed=None, ref=None, what=''):
    """Assert the three properties of a word-table gradient ``got`` (the rows ``dec.rows`` of it, float32 or float64):
    rows with S_w = 0 exactly zero; with ``addressed`` (full table only) the non-zero rows exactly those; every err_w at or
    below ``limit``.  A failure names the word, its occurrence count and ``what`` (the index form).  Returns the worst err_w."""
    got = got.detach().cpu()
    if got.shape[0] != dec.rows.numel():
        got = got[dec.rows]
    dead = dec.scale.eq(0)
    bad = torch.nonzero(got[dead].ne(0).any(1)).flatten()
    assert bad.numel() == 0, '%s: word %d has no reference gradient, its row is not zero' % (what, int(dec.rows[dead][bad[0]]))
    if addressed is not None:
        nz = torch.nonzero(got.ne(0).any(1)).flatten()
        extra, missing = np.setdiff1d(nz.numpy(), addressed.numpy()), np.setdiff1d(addressed.numpy(), nz.numpy())
        assert extra.size == 0 and missing.size == 0, \
            '%s: rows written for words the batch does not address %s, addressed words without a row %s' \
            % (what, extra[:8].tolist(), missing[:8].tolist())
    err = row_errors(got, dec, ref)
    w = int(err.argmax())
    assert float(err[w]) <= limit, '%s: word %d (%d occurrences) err_w %.3e > %.3e' \
        % (what, int(dec.rows[w]), int(dec.count[w]), float(err[w]), limit)
    return float(err[w])


def heaviest_and_singleton(p, dec):
    """Row positions of the most frequent word and of the first of the rarest words that are in no query (nor, with
    train_pv, in the PV loss or a positive's review, which the PV loss reaches: such a row is its occurrences alone).  Every case of this module has a word that occurs once
    (tests/test_rtm_word_rows_cpu.py asserts it); tests/test_gpu_rtm_shapes.py's d = 128 shape, whose 25,000 occurrences
    fall on 1,499 words, has none, and its rarest word stands in."""
    heavy = int(dec.count.argmax())
    pure = (dec.count > 0) & (dec.rest <= 1e-9 * dec.occ_scale)
    assert bool(pure.any()), 'no word outside the queries'
    least = int(dec.count[pure].min())
    return heavy, int(torch.nonzero(pure & dec.count.eq(least)).flatten()[0])


def mutations(p, dec):
    """[(label, row position, mutated float64 reference, err_w the mutation makes in that row)]: one occurrence dropped
    and one doubled, for the heaviest word (the occurrence whose |c|_inf is nearest the mean of the word's) and for a
    singleton.  The scale S_w stays the case's."""
    out = []
    for label, r in zip(('heaviest', 'singleton'), heaviest_and_singleton(p, dec)):
        slots = dec.occ_slot[dec.occ_row.eq(r)]
        s = int(slots[(dec.cn[slots] - dec.cn[slots].mean()).abs().argmin()])
        for kind, sign in (('dropped', -1.0), ('doubled', 1.0)):
            ref = dec.ref.clone()
            ref[r] += sign * dec.c[s]
            out.append(('%s word %d (%d occurrences), one %s' % (label, int(dec.rows[r]), int(dec.count[r]), kind), r, ref,
                        float(dec.cn[s] / dec.scale[r])))
    return out


# ------------------------------------------------------------------------------------------------------ full size
FULL = dict(V=32387, RC=60000, B=256, K=5, WL=100, u_lim=20, i_lim=30, d=128)


def fullsize_problem(seed=11):
    """tests/test_gpu_fullsize_rtm.py's inputs (its ``_setup('pvc')``), built without a device."""
    from prodsearch_amd import ProductRanker, default_args, synth, rtm_data
    f = types.SimpleNamespace(**FULL)
    a = default_args(model_name='review_transformer', review_encoder_name='pvc', embedding_size=f.d, heads=8, ff_size=512,
                     inter_layers=1, neg_per_pos=f.K, dropout=0.0, corrupt_rate=0.0, lr=0.0005, review_word_limit=f.WL,
                     uprev_review_limit=f.u_lim, iprev_review_limit=f.i_lim)
    wd = synth.make_word_dists(f.V)
    rng = synth.rng_for(seed)
    rw = torch.from_numpy(rng.integers(0, f.V - 1, size=(f.RC, f.WL)))
    lens = torch.from_numpy(rng.integers(f.WL // 4, f.WL + 1, size=f.RC))
    rw[torch.arange(f.WL)[None, :] >= lens[:, None]] = f.V - 1
    rw[-1] = f.V - 1
    state = torch.get_rng_state()
    try:
        torch.manual_seed(0)
        m = ProductRanker(a, 'cpu', f.V, f.RC, 1000, 1000, rw, None, word_dists=wd)
    finally:
        torch.set_rng_state(state)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    batch = rtm_data.make_rtm_batch(100 + seed, f.B, f.K, f.RC, f.V, rw, Q=8, u_lim=f.u_lim, i_lim=f.i_lim, W=1,
                                    train_pv=False, encoder='pvc', word_dists=wd)
    return types.SimpleNamespace(a=a, sd=sd, batch=batch, V=f.V, RC=f.RC, B=f.B, K=f.K, train_pv=False, neg_words=None)


def slot_grads_with_the_table_constant(p, sd, f64):
    """{'loss', 'slot_grads'} of oracle.rtm with every parameter held constant and the slots' word means as leaves
    (pvc): no table-sized tensor is saved for the backward."""
    from oracle import rtm as ortm

    def run():
        P = {k: (v.double() if (f64 and v.dtype.is_floating_point) else v) for k, v in sd.items()}
        keep = {'leaf_means': True}
        loss, _, _ = ortm.rtm_forward(P, p.a, p.batch, None, p.V, p.RC, training=True, train_pv=False, keep=keep)
        return dict(loss=loss.detach(), slot_grads=torch.autograd.grad(loss, [keep['mean_pos'], keep['mean_neg']]))
    return S.oracle_f64(run) if f64 else run()


def fp32_rows(p, r32, dec):
    """The rows ``dec.rows`` of the fp32 oracle's word gradient, as its autograd adds them: c = g_s / n_s in fp32, one
    fp32 add per occurrence."""
    idx, ok, real = slot_words(p)
    g = torch.cat(list(r32['slot_grads']), 0)
    c = g / ok.sum(1).clamp(min=1)[:, None].to(g.dtype)
    return torch.zeros(dec.rows.numel(), g.shape[1], dtype=g.dtype).index_add_(0, dec.occ_row, c[dec.occ_slot])


def fullsize_sample(p):
    """tests/test_gpu_fullsize_rtm.py: the 64 most frequent words of the batch's real reviews and its 64 rarest (the
    batch's 1.3 million uniformly drawn occurrences leave no word with exactly one), none of them a query word — their
    rows are sums of occurrences alone —, as a sorted tensor."""
    idx, ok, real = slot_words(p)
    cnt = torch.bincount(idx[ok & real[:, None]], minlength=p.V)
    cnt[p.batch.query_word_idxs.reshape(-1)] = 0
    cnt[p.V - 1] = 0
    top = torch.topk(cnt, 64).indices
    rare = torch.topk(torch.where(cnt > 0, cnt, torch.full_like(cnt, 1 << 40)), 64, largest=False).indices
    assert int(cnt[rare].max()) < int(cnt[top].min()) and int(cnt[rare].min()) > 0
    return torch.sort(torch.cat([top, rare])).values
