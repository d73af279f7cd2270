"""Rows of the item models' table gradients (``product_emb``, ``hist_product_emb``, ``word_embeddings``, ``product_bias``,
``word_bias`` of the item transformer and QEM), one by one, against the float64 oracle
(tests/test_tem_table_rows_cpu.py, tests/test_gpu_tem_table_rows.py).  No GPU is needed here.

The step ends in scatters into these tables: the score backward's item and word tasks (csrc/rowwise.hip: score_bwd_kernel),
the history and query-word rows (embed_scatter_kernel, two forms), the item scatter inside the fused per-replica backward
(csrc/mlp_fused.hip) and the sole-owner deterministic forms.  One lost, doubled or misfiled occurrence changes ONE row, and
the suite's max-norm over a whole table (5e-4 of its largest entry) is larger than the whole gradient of many rows.  So every
row is judged on its own scale, in the manner of tests/rtm_word_rows.py.

Per-occurrence contributions.  With ``keep`` the oracle records every tensor it gathers from a table (oracle.tem); the
gradient of the loss with respect to such a tensor, from the float64 oracle's autograd, holds one row per occurrence: the
contribution c that occurrence adds to the table row its index names (``parts``):
  product_emb       the target row (ranking score), each negative, the target row again (PV loss), and each history slot
                    per replica — (b, l) of the positives' sequence and, when the oracle replicates (dropout), (b, k, l) of
                    the negatives' input.  Per replica on purpose: the positive and the K negative replicas push a history
                    row in opposite directions, and a scale built from their sum would judge the row against a cancelled
                    value.  With sep_prod_emb the history slots go to hist_product_emb instead;
  word_embeddings   query words, PV target words, PV sampled words;
  the bias vectors  the same lists with scalar c.
Occurrences whose index is the pad row are dropped, and so is a sampled word under a masked window slot (its target word is
the pad): its gradient is exactly zero and the product skips it too.  The decomposition closes: the table's own gradient
equals the sum of c to 1e-12 of the row's scale, on every row (asserted for every case).

Row metric.  err_row = |got_row - ref_row|_inf / S_row with S_row = sum over the row's occurrences of |c|_inf.  Rows with
S_row = 0 must be exactly zero, the rows that are not zero must be exactly the rows the batch addresses (``addressed``: from
the index tensors alone), and every err_row stays at or below the case's bound.

Bound.  Nothing fixed in advance: YARDSTICK records, per case and table, the fp32 oracle's worst err_row against the float64
oracle, measured on the CPU with 1, 4 and all threads, as 1.1 x the largest rounded up to two digits
(tests/test_tem_table_rows_cpu.py asserts that a one-thread run measures no more; ``python tests/tem_table_rows.py``
measures again).  The product has to stay within 8 x that — sums formed in runs and through fp32 atomics — and within 2^-22
where the fp32 oracle happens to be exact.

What the bound can see (asserted for every case and table on the CPU): ``mutations`` drops or doubles ONE occurrence in the
float64 reference — of the row with the most occurrences (the occurrence whose |c|_inf is nearest that row's mean: a loss of
average size) and of a row with a single one — and the change each makes to err_row is more than twice the bound.  A history
table of its own (sep_prod_emb) has no row with a single occurrence when the oracle replicates — every slot is K + 1
occurrences — and its rarest row stands in.  What no check of values can see is an occurrence far below its row's average:
a negative replica's share of a history slot whose softmax weight is near zero, a negative scored near -10.  Such
occurrences are covered by the exact non-zero-row check only, and by that only in rows with a single occurrence."""
import atexit
import functools
import os
import shutil
import tempfile
import types

import numpy as np
import torch

import enc_paths
import saturated as S

FLOOR = 2.0 ** -22
PROD, HIST, WORD, PBIAS, WBIAS = 'product_emb.weight', 'hist_product_emb.weight', 'word_embeddings.weight', 'product_bias', 'word_bias'
TABLES = (PROD, HIST, WORD, PBIAS, WBIAS)
HEAVY_ITEM, HEAVY_WORD = 17, 5


# ------------------------------------------------------------------------------------------------------ edits
def refill_queries(p):
    """Queries of 1 .. Q words (make_tem_batch fills 6 at the most): row 0 has Q, its first word again at Q / 2 and Q - 1;
    row 1 has one word; row 2 none — all pad, no occurrence, nothing may be written for it."""
    from prodsearch_amd import synth
    qw = p.batch.query_word_idxs
    B, Q = qw.shape
    rng = synth.rng_for(41)
    lens = rng.integers(1, Q + 1, size=B)
    lens[0], lens[1], lens[2] = Q, 1, 0
    words = torch.from_numpy(rng.choice(p.V, size=(B, Q), p=p.wd))
    qw[:] = torch.where(torch.arange(Q)[None, :] < torch.from_numpy(lens)[:, None], words, torch.full_like(words, p.V - 1))
    qw[0, Q // 2] = qw[0, Q - 1] = qw[0, 0]
    p.qlens = lens


def check_refilled(p):
    qw, pad = p.batch.query_word_idxs, p.V - 1
    Q = qw.shape[1]
    n = qw.ne(pad).sum(1)
    assert n.tolist() == list(p.qlens) and int(n[0]) == Q and int(n[1]) == 1 and int(n[2]) == 0
    assert int(qw[0, 0]) == int(qw[0, Q // 2]) == int(qw[0, Q - 1])
    assert bool((qw.ne(pad) == (torch.arange(Q)[None, :] < n[:, None])).all())             # words first, pad behind
    if Q > 64:
        assert int((n > 64).sum()) >= 1 and int(((n > 32) & (n <= 64)).sum()) >= 1


def make_heavy(p):
    """One item in 60 % of the non-pad history slots, the target of every fourth row, three of row 2's negatives and the
    first negative of every fifth row; one word the PV target of every third row, a sampled word of every second row and
    half of the query words."""
    from prodsearch_amd import synth
    b, rng = p.batch, synth.rng_for(43)
    ui, qw = b.u_item_idxs, b.query_word_idxs
    ui[torch.from_numpy(rng.random(tuple(ui.shape)) < 0.6) & ui.ne(p.P_)] = HEAVY_ITEM
    b.target_prod_idxs[::4] = HEAVY_ITEM
    p.ni[2, :3] = HEAVY_ITEM
    p.ni[::5, 0] = HEAVY_ITEM
    b.pos_iword_idxs[::3, 0] = HEAVY_WORD
    p.nw[::2, 0] = HEAVY_WORD
    qw[torch.from_numpy(rng.random(tuple(qw.shape)) < 0.5) & qw.ne(p.V - 1)] = HEAVY_WORD


def check_heavy(p):
    b = p.batch
    ui, qw, live = b.u_item_idxs, b.query_word_idxs, b.u_item_idxs.ne(p.P_)
    share = float((ui.eq(HEAVY_ITEM) & live).sum()) / float(live.sum())
    assert 0.5 < share < 0.7, share
    assert bool(b.target_prod_idxs[::4].eq(HEAVY_ITEM).all()) and int(p.ni[2].eq(HEAVY_ITEM).sum()) >= 3
    assert bool(p.ni[::5, 0].eq(HEAVY_ITEM).all())
    assert bool(b.pos_iword_idxs[::3, 0].eq(HEAVY_WORD).all()) and bool(p.nw[::2, 0].eq(HEAVY_WORD).all())
    qshare = float(qw.eq(HEAVY_WORD).sum()) / float(qw.ne(p.V - 1).sum())
    assert 0.35 < qshare < 0.65, qshare


_TMP = []


def _tmp_dir():
    if not _TMP:
        _TMP.append(tempfile.mkdtemp(prefix='tem_table_rows_'))
        atexit.register(shutil.rmtree, _TMP[0], True)
    return _TMP[0]


def freeze_words(p):
    """A pretrained word table (tests/pretrain_util.py, as test_gpu_pretrained._setup at this size): the module then takes
    word_embeddings from the file and freezes it.  The oracle's table is the file's, trainable there — the other gradients
    do not depend on that — and the GPU test asserts that the module's has no gradient."""
    import pretrain_util
    from prodsearch_amd.pretrained import word_table
    emb = os.path.join(_tmp_dir(), 'emb_%d_%d' % (p.V, p.a.embedding_size))
    p.words = pretrain_util.vocab_words(p.V)
    if not os.path.exists(os.path.join(emb, 'word_emb.txt.gz')):
        os.makedirs(emb, exist_ok=True)
        pretrain_util.write_word_emb(os.path.join(emb, 'word_emb.txt.gz'), p.words, p.a.embedding_size, seed=11, n_extra=50,
                                     tie_share=0.02)
    p.a.pretrain_emb_dir = emb
    p.sd[WORD] = torch.from_numpy(word_table(emb, p.words, p.V, p.a.embedding_size)).clone()
    p.frozen = True


# ------------------------------------------------------------------------------------------------------ cases
C2S = dict(B=50, K=20, L=9, Q=4)
_QB = dict(B=6, K=4, L=9, ff_size=256)
_ROW = {r['name']: r for r in enc_paths.ALL_ROWS}


def _case(row=None, call=None, fuse_bwd_min=None, check=None, **over):
    """``row``: the enc_paths row whose path the case takes (None: QEM has no encoder); ``call``: saturated.problem's
    arguments where they are not the row's own; ``over``: arguments on top of either."""
    kw = dict(enc_paths.oracle_call(_ROW[row])) if call is None else dict(call)
    kw.update(over)
    if fuse_bwd_min is None and row is not None:
        fuse_bwd_min = _ROW[row]['fuse_bwd_min']
    return dict(row=row, call=kw, fuse_bwd_min=fuse_bwd_min, check=check)


CASES = {
    # the fused backward's item scatter; under ps_set_item_scatter_fused(0) the score backward's item workgroups
    'c2s': _case('e_50_20_9'),
    # a partial last tile of 32 replica rows; W 3 with masked window slots; 2 replicas
    'tiles_w3': _case('p_2_5_20'),
    'tiles_r2': _case('p_33_1_5'),
    'nodrop': _case('e_6_4_40_nodrop'),                 # R = 1: d enc through LDS, no item workgroups
    'fan34_d64': _case('e_5_33_7'),                     # K + 1 = 34 is past the 16 row groups; W 2; EPL 2
    'd96': _case('e_130_3_12'),                         # score_bwd_kernel<16> with masked columns; epl = 3 default: arms
    'd32_nohist': _case('e_3_2_20'),                    # no history occurrence at all
    'd32_smallest': _case('e_1_1_1'),                   # the smallest legal shape
    'd256': _case('w_d256'),                            # EPL 8; presum fan-in
    'd512': _case('d512_drop'),                         # EPL 16; epl = 16 default: arms
    'qem': _case(None, S.QEM_CALL),                     # no encoder, R = 1
    # query-word tasks from dqmean_d: the epl == 4 drop_mult arm, the generic arm, the row_fetch_add(inv) arm
    'avg': _case('o_avg'),
    'avg_d96': _case('avg_d96'),
    'avg_d64_nodrop': _case('avg_d64_nodrop'),
    'sep': _case('e_50_20_9', sep_prod_emb=True),       # a separate history table
    'bias': _case('e_50_20_9', sim_func='bias_product', pos_weight=True),
    'heavy': _case('e_50_20_9', edit=make_heavy, check=check_heavy),          # rows with thousands of additions
    'heavy_nodrop': _case('heavy_nodrop', edit=make_heavy, check=check_heavy),
    'frozen': _case('e_50_20_9', edit=freeze_words),    # the WG = false forms
}
for _q in (33, 64, 65, 70):      # the Q <= 64 ballot and the Q > 64 loop; q += 8; q0 += 32 with the half-wave shift
    CASES['q%d_fs' % _q] = _case('q%d_fs' % _q, edit=refill_queries, check=check_refilled)
    CASES['q%d_avg' % _q] = _case('q%d_avg' % _q, edit=refill_queries, check=check_refilled)
DET_CASES = ('c2s', 'nodrop', 'avg', 'q70_fs', 'q70_avg', 'heavy', 'd256')

# The fp32 oracle's worst err_row against the float64 oracle, per table, measured on the CPU with 1, 4 and all threads.
# Recorded: 1.1 x the largest of the three, rounded up to two digits — another host's fp32 kernels add in another order.
# tests/test_tem_table_rows_cpu.py measures with one thread, which repeats.  The GPU bound is max(8 x recorded, FLOOR).
# (The three thread counts agree at these sizes.  The tenth does not cover every host: a CPU with other vector units measured
# up to 2.4 x the recorded value in five cases — 3.3e-6 for q33_avg's product_emb — as it does in three of
# tests/rtm_word_rows.py's; the GPU's own figures, DESIGN.md 7c, are at most 1.9 x the values recorded here, d512's.)
#   case: {table: recorded}            measured: 1 thread / 4 / all
YARDSTICK = {
    'c2s': {
        'product_emb.weight':       6.4e-06,    # 5.80e-06 / 5.80e-06 / 5.80e-06
        'word_embeddings.weight':   4.1e-06,    # 3.71e-06 / 3.71e-06 / 3.71e-06
        'word_bias':                4.2e-06,    # 3.75e-06 / 3.75e-06 / 3.75e-06
    },
    'tiles_w3': {
        'product_emb.weight':       3.0e-06,    # 2.69e-06 / 2.69e-06 / 2.69e-06
        'word_embeddings.weight':   1.8e-06,    # 1.56e-06 / 1.56e-06 / 1.56e-06
        'word_bias':                1.8e-06,    # 1.58e-06 / 1.58e-06 / 1.58e-06
    },
    'tiles_r2': {
        'product_emb.weight':       3.2e-06,    # 2.87e-06 / 2.87e-06 / 2.87e-06
        'word_embeddings.weight':   4.9e-06,    # 4.36e-06 / 4.36e-06 / 4.36e-06
        'word_bias':                2.3e-06,    # 2.04e-06 / 2.04e-06 / 2.04e-06
    },
    'nodrop': {
        'product_emb.weight':       3.7e-06,    # 3.34e-06 / 3.34e-06 / 3.34e-06
        'word_embeddings.weight':   1.1e-06,    # 9.92e-07 / 9.92e-07 / 9.92e-07
        'word_bias':                9.4e-07,    # 8.50e-07 / 8.50e-07 / 8.50e-07
    },
    'fan34_d64': {
        'product_emb.weight':       3.5e-06,    # 3.15e-06 / 3.15e-06 / 3.15e-06
        'word_embeddings.weight':   1.9e-06,    # 1.65e-06 / 1.65e-06 / 1.65e-06
        'word_bias':                1.9e-06,    # 1.67e-06 / 1.67e-06 / 1.67e-06
    },
    'd96': {
        'product_emb.weight':       5.5e-06,    # 4.95e-06 / 4.95e-06 / 4.95e-06
        'word_embeddings.weight':   1.7e-06,    # 1.49e-06 / 1.49e-06 / 1.49e-06
        'word_bias':                1.6e-06,    # 1.40e-06 / 1.40e-06 / 1.40e-06
    },
    'd32_nohist': {
        'product_emb.weight':       7.0e-07,    # 6.29e-07 / 6.29e-07 / 6.29e-07
        'word_embeddings.weight':   1.1e-06,    # 9.70e-07 / 9.70e-07 / 9.70e-07
        'word_bias':                8.0e-07,    # 7.21e-07 / 7.21e-07 / 7.21e-07
    },
    'd32_smallest': {
        'product_emb.weight':       3.2e-07,    # 2.90e-07 / 2.90e-07 / 2.90e-07
        'word_embeddings.weight':   1.1e-06,    # 9.24e-07 / 9.24e-07 / 9.24e-07
        'word_bias':                7.2e-07,    # 6.54e-07 / 6.54e-07 / 6.54e-07
    },
    'd256': {
        'product_emb.weight':       7.7e-06,    # 6.95e-06 / 6.95e-06 / 6.95e-06
        'word_embeddings.weight':   3.6e-06,    # 3.19e-06 / 3.19e-06 / 3.19e-06
        'word_bias':                3.5e-06,    # 3.18e-06 / 3.18e-06 / 3.18e-06
    },
    'd512': {
        'product_emb.weight':       1.1e-05,    # 9.63e-06 / 9.63e-06 / 9.63e-06
        'word_embeddings.weight':   1.8e-05,    # 1.59e-05 / 1.59e-05 / 1.59e-05
        'word_bias':                1.8e-05,    # 1.59e-05 / 1.59e-05 / 1.59e-05
    },
    'qem': {
        'product_emb.weight':       9.5e-07,    # 8.58e-07 / 8.58e-07 / 8.58e-07
        'word_embeddings.weight':   4.1e-06,    # 3.71e-06 / 3.71e-06 / 3.71e-06
        'word_bias':                4.2e-06,    # 3.75e-06 / 3.75e-06 / 3.75e-06
    },
    'avg': {
        'product_emb.weight':       4.6e-06,    # 4.18e-06 / 4.18e-06 / 4.18e-06
        'word_embeddings.weight':   4.1e-06,    # 3.71e-06 / 3.71e-06 / 3.71e-06
        'word_bias':                4.2e-06,    # 3.75e-06 / 3.75e-06 / 3.75e-06
    },
    'avg_d96': {
        'product_emb.weight':       4.3e-06,    # 3.91e-06 / 3.91e-06 / 3.91e-06
        'word_embeddings.weight':   2.2e-06,    # 1.91e-06 / 1.91e-06 / 1.91e-06
        'word_bias':                2.1e-06,    # 1.87e-06 / 1.87e-06 / 1.87e-06
    },
    'avg_d64_nodrop': {
        'product_emb.weight':       1.2e-06,    # 1.06e-06 / 1.06e-06 / 1.06e-06
        'word_embeddings.weight':   6.6e-07,    # 5.95e-07 / 5.95e-07 / 5.95e-07
        'word_bias':                6.6e-07,    # 5.92e-07 / 5.92e-07 / 5.92e-07
    },
    'sep': {
        'product_emb.weight':       7.1e-06,    # 6.44e-06 / 6.44e-06 / 6.44e-06
        'hist_product_emb.weight':  3.0e-07,    # 2.67e-07 / 2.67e-07 / 2.67e-07
        'word_embeddings.weight':   2.5e-06,    # 2.23e-06 / 2.23e-06 / 2.23e-06
        'word_bias':                2.5e-06,    # 2.26e-06 / 2.26e-06 / 2.26e-06
    },
    'bias': {
        'product_emb.weight':       6.5e-06,    # 5.85e-06 / 5.85e-06 / 5.85e-06
        'word_embeddings.weight':   4.1e-06,    # 3.71e-06 / 3.71e-06 / 3.71e-06
        'product_bias':             1.1e-05,    # 9.53e-06 / 9.53e-06 / 9.53e-06
        'word_bias':                4.2e-06,    # 3.75e-06 / 3.75e-06 / 3.75e-06
    },
    'heavy': {
        'product_emb.weight':       4.6e-06,    # 4.16e-06 / 4.16e-06 / 4.16e-06
        'word_embeddings.weight':   4.1e-06,    # 3.71e-06 / 3.71e-06 / 3.71e-06
        'word_bias':                4.2e-06,    # 3.75e-06 / 3.75e-06 / 3.75e-06
    },
    'heavy_nodrop': {
        'product_emb.weight':       5.1e-06,    # 4.57e-06 / 4.57e-06 / 4.57e-06
        'word_embeddings.weight':   4.1e-06,    # 3.71e-06 / 3.71e-06 / 3.71e-06
        'word_bias':                4.2e-06,    # 3.75e-06 / 3.75e-06 / 3.75e-06
    },
    'frozen': {
        'product_emb.weight':       4.4e-06,    # 3.96e-06 / 3.96e-06 / 3.96e-06
        'word_embeddings.weight':   2.6e-06,    # 2.31e-06 / 2.31e-06 / 2.31e-06
        'word_bias':                2.6e-06,    # 2.35e-06 / 2.35e-06 / 2.35e-06
    },
    'q33_fs': {
        'product_emb.weight':       4.1e-06,    # 3.71e-06 / 3.71e-06 / 3.71e-06
        'word_embeddings.weight':   1.3e-06,    # 1.18e-06 / 1.18e-06 / 1.18e-06
        'word_bias':                1.8e-06,    # 1.56e-06 / 1.56e-06 / 1.56e-06
    },
    'q33_avg': {
        'product_emb.weight':       1.4e-06,    # 1.27e-06 / 1.27e-06 / 1.27e-06
        'word_embeddings.weight':   1.3e-06,    # 1.18e-06 / 1.18e-06 / 1.18e-06
        'word_bias':                1.8e-06,    # 1.56e-06 / 1.56e-06 / 1.56e-06
    },
    'q64_fs': {
        'product_emb.weight':       2.8e-06,    # 2.53e-06 / 2.53e-06 / 2.53e-06
        'word_embeddings.weight':   8.9e-07,    # 8.03e-07 / 8.03e-07 / 8.03e-07
        'word_bias':                5.5e-07,    # 4.92e-07 / 4.92e-07 / 4.92e-07
    },
    'q64_avg': {
        'product_emb.weight':       2.3e-06,    # 2.09e-06 / 2.09e-06 / 2.09e-06
        'word_embeddings.weight':   5.4e-07,    # 4.85e-07 / 4.85e-07 / 4.85e-07
        'word_bias':                5.5e-07,    # 4.92e-07 / 4.92e-07 / 4.92e-07
    },
    'q65_fs': {
        'product_emb.weight':       3.5e-06,    # 3.15e-06 / 3.15e-06 / 3.15e-06
        'word_embeddings.weight':   4.0e-06,    # 3.63e-06 / 3.63e-06 / 3.63e-06
        'word_bias':                4.1e-06,    # 3.66e-06 / 3.66e-06 / 3.66e-06
    },
    'q65_avg': {
        'product_emb.weight':       2.7e-06,    # 2.40e-06 / 2.40e-06 / 2.40e-06
        'word_embeddings.weight':   4.0e-06,    # 3.63e-06 / 3.63e-06 / 3.63e-06
        'word_bias':                4.1e-06,    # 3.66e-06 / 3.66e-06 / 3.66e-06
    },
    'q70_fs': {
        'product_emb.weight':       3.5e-06,    # 3.12e-06 / 3.12e-06 / 3.12e-06
        'word_embeddings.weight':   2.8e-06,    # 2.46e-06 / 2.46e-06 / 2.46e-06
        'word_bias':                3.7e-05,    # 3.34e-05 / 3.34e-05 / 3.34e-05
    },
    'q70_avg': {
        'product_emb.weight':       3.2e-06,    # 2.90e-06 / 2.90e-06 / 2.90e-06
        'word_embeddings.weight':   2.8e-06,    # 2.46e-06 / 2.46e-06 / 2.46e-06
        'word_bias':                3.7e-05,    # 3.34e-05 / 3.34e-05 / 3.34e-05
    },
}


def bound(name, table):
    return max(8.0 * YARDSTICK[name][table], FLOOR)


@functools.lru_cache(maxsize=None)
def problem(name):
    return S.problem(**CASES[name]['call'])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(problem, float64 oracle step, {table: its decomposition}) of a case; computed once per process and shared — nobody
    writes to it."""
    p = problem(name)
    r64 = S.oracle_step(p, p.sd, True, want_eval=False, want_occ=True)
    return p, r64, decompose(p, r64)


def fp32_step(name, threads=1):
    """The fp32 oracle's step, with ``threads`` threads (one: a row of thousands of terms adds up in the same order every
    run)."""
    p = problem(name)
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        return S.oracle_step(p, p.sd, False, want_eval=False)
    finally:
        torch.set_num_threads(old)


def plan_desc(name):
    """The training-step descriptor ItemTransformerRanker._plan_for builds for the case's problem (the fields the plan
    reads), from the problem itself and not from the row the case claims."""
    from prodsearch_amd import _lib
    p, a = problem(name), problem(name).a
    d = enc_paths.desc_of(_ROW[CASES[name]['row']], _lib)
    d.B, d.K, d.L, d.Q, d.W = p.B, p.K, p.L, p.batch.query_word_idxs.shape[1], p.W
    d.d, d.H, d.F, d.n_layers = a.embedding_size, a.heads, a.ff_size, a.inter_layers
    d.product_size, d.vocab_size = p.P_, p.V
    d.query_encoder = _lib.PS_QENC_FS if a.query_encoder_name == 'fs' else _lib.PS_QENC_AVG
    d.use_pos_emb, d.use_item_pos = int(a.use_pos_emb), int(a.use_item_pos)
    d.bias_product, d.pos_weight, d.sep_prod_emb = int(a.sim_func == 'bias_product'), int(a.pos_weight), int(a.sep_prod_emb)
    d.dropout = float(a.dropout)
    return d


# ------------------------------------------------------------------------------------------------------ the decomposition
def parts(p):
    """[(table, key of the oracle's gathered tensor, index of every row of it [N], live [N], rows(g) -> [N, width])]: the
    occurrence lists.  live: the occurrence counts (not the pad row, not under a masked window slot)."""
    b, a = p.batch, p.a
    B, K, L, W = p.B, p.K, p.L, p.W
    tgt, ui, qw, pw = b.target_prod_idxs, b.u_item_idxs, b.query_word_idxs, b.pos_iword_idxs
    ni, nw = p.ni.reshape(-1), p.nw.reshape(-1)
    ppad, wpad = p.P_, p.V - 1
    slot = pw.ne(wpad)[:, :, None].expand(B, W, K).reshape(-1)        # neg_word_idxs is [B, W K]: slot w holds K draws
    flat = lambda g: g.reshape(-1, g.shape[-1])
    col = lambda g: g.reshape(-1, 1)
    hist = HIST if a.sep_prod_emb else PROD
    out = [(PROD, 'target_emb', tgt, tgt.ne(ppad), flat), (PROD, 'neg_emb', ni, ni.ne(ppad), flat),
           (PROD, 'pv_prod', tgt, tgt.ne(ppad), flat)]
    if not p.qem:
        h = ui.reshape(-1)
        out.append((hist, 'pos_seq', h, h.ne(ppad), lambda g: flat(g[:, 1:])))
        if a.dropout > 0:                # the oracle replicates: B K copies of the history, each with a gradient of its own
            hk = ui[:, None, :].expand(B, K, L).reshape(-1)
            out.append((hist, 'neg_seq', hk, hk.ne(ppad), lambda g: flat(g.view(B, K, L + 1, -1)[:, :, 1:])))
    q, w = qw.reshape(-1), pw.reshape(-1)
    out += [(WORD, 'query_word_emb', q, q.ne(wpad), flat), (WORD, 'pv_wpos', w, w.ne(wpad), flat),
            (WORD, 'pv_wneg', nw, nw.ne(wpad) & slot, flat)]
    if a.sim_func == 'bias_product':
        out += [(PBIAS, 'target_bias', tgt, tgt.ne(ppad), col), (PBIAS, 'neg_bias', ni, ni.ne(ppad), col)]
    out += [(WBIAS, 'pv_bpos', w, w.ne(wpad), col), (WBIAS, 'pv_bneg', nw, nw.ne(wpad) & slot, col)]
    return out


def trained_tables(p):
    return [t for t in TABLES if any(x[0] == t for x in parts(p))]


def addressed(p, table):
    """The rows of ``table`` the batch addresses, from its index tensors alone, sorted."""
    return torch.unique(torch.cat([idx[live] for t, _, idx, live, _ in parts(p) if t == table]))


def decompose(p, r64):
    """{table: namespace} of the float64 reference, row by row: rows [n], ref [n, width] (a bias vector: width 1),
    scale [n] S_row, count [n], occ_row [N] and c [N, width] (row and contribution of every occurrence), cn [N] = |c|_inf,
    closure [n] = |ref - sum c|_inf."""
    out = {}
    for table in trained_tables(p):
        idx, c = [], []
        for t, key, i, live, rows in parts(p):
            if t != table:
                continue
            g = rows(r64['occ'][key].double())
            assert g.shape[0] == i.numel(), (table, key)
            idx.append(i[live])
            c.append(g[live])
        idx, c = torch.cat(idx), torch.cat(c)
        ref = r64['grads'][table].double()
        n = ref.shape[0]
        ref = ref.reshape(n, -1)
        cn = c.abs().amax(1)
        summed = torch.zeros_like(ref).index_add_(0, idx, c)
        scale = torch.zeros(n, dtype=torch.float64).index_add_(0, idx, cn)
        count = torch.zeros(n, dtype=torch.int64).index_add_(0, idx, torch.ones_like(idx))
        out[table] = types.SimpleNamespace(rows=torch.arange(n), ref=ref, scale=scale, count=count, occ_row=idx, c=c, cn=cn,
                                           closure=(ref - summed).abs().amax(1))
    return out


def row_errors(got, dec, ref=None):
    """err_row of every row of ``dec`` (0 where S_row = 0: those rows are compared exactly, ``compare``)."""
    ref = dec.ref if ref is None else ref
    diff = (got.detach().cpu().double().reshape(ref.shape) - ref).abs().amax(1)
    return torch.where(dec.scale > 0, diff / dec.scale.clamp(min=1e-300), torch.zeros_like(diff))


def compare(got, dec, limit, addr, ref=None, what=''):
    """Assert the three properties of a table gradient ``got`` (float32 or float64; a bias vector or a table): rows with
    S_row = 0 exactly zero; the non-zero rows exactly ``addr``; every err_row at or below ``limit``.  A failure names the
    row, its occurrence count and ``what`` (case, table, form).  Returns the worst err_row."""
    got = got.detach().cpu().reshape(dec.ref.shape)
    dead = dec.scale.eq(0)
    bad = torch.nonzero(got[dead].ne(0).any(1)).flatten()
    assert bad.numel() == 0, '%s: row %d has no reference gradient and is not zero' % (what, int(dec.rows[dead][bad[0]]))
    nz = torch.nonzero(got.ne(0).any(1)).flatten()
    extra, missing = np.setdiff1d(nz.numpy(), addr.numpy()), np.setdiff1d(addr.numpy(), nz.numpy())
    assert extra.size == 0 and missing.size == 0, '%s: rows written that the batch does not address %s, addressed rows ' \
        'without a gradient %s' % (what, extra[:8].tolist(), missing[:8].tolist())
    err = row_errors(got, dec, ref)
    r = int(err.argmax())
    assert float(err[r]) <= limit, '%s: row %d (%d occurrences) err_row %.3e > %.3e' \
        % (what, r, int(dec.count[r]), float(err[r]), limit)
    return float(err[r])


def heaviest_and_rarest(dec):
    """Rows with the most occurrences and with the fewest (the first of them); the fewest is 1 but for a history table of
    its own under replicas."""
    live = dec.count > 0
    least = int(dec.count[live].min())
    return int(dec.count.argmax()), int(torch.nonzero(dec.count.eq(least)).flatten()[0])


def mutations(dec):
    """[(label, row, mutated float64 reference, err_row the mutation makes in that row)]: one occurrence dropped and one
    doubled, for the heaviest row (the occurrence whose |c|_inf is nearest the mean of the row's) and for the rarest.  The
    scale S_row stays the case's."""
    out = []
    for label, r in zip(('heaviest', 'single'), heaviest_and_rarest(dec)):
        occ = torch.nonzero(dec.occ_row.eq(r)).flatten()
        o = int(occ[(dec.cn[occ] - dec.cn[occ].mean()).abs().argmin()])
        for kind, sign in (('dropped', -1.0), ('doubled', 1.0)):
            ref = dec.ref.clone()
            ref[r] += sign * dec.c[o]
            out.append(('%s row %d (%d occurrences), one %s' % (label, r, int(dec.count[r]), kind), r, ref,
                        float(dec.cn[o] / dec.scale[r])))
    return out


def measure(name, threads):
    """{table: the fp32 oracle's worst err_row} of a case."""
    p, r64, decs = reference(name)
    g = fp32_step(name, threads)['grads']
    return {t: float(row_errors(g[t], dec).max()) for t, dec in decs.items()}


def _round_up(x):
    e = int(np.floor(np.log10(x))) - 1
    return float('%.1e' % (np.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e))


if __name__ == '__main__':       # measure the yardsticks again: 1, 4 and all threads
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
    for _name in (sys.argv[1:] or list(CASES)):
        _m = [measure(_name, _t) for _t in (1, 4, torch.get_num_threads())]
        print("    %r: {" % _name)
        for _t in _m[0]:
            _v = [m[_t] for m in _m]
            print("        %-27s %.1e,    # %.2e / %.2e / %.2e" % (repr(_t) + ':', _round_up(1.1 * max(_v)), _v[0], _v[1], _v[2]))
        print("    },")
