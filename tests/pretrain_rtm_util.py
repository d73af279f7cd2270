"""Synthetic pretrained files of the review transformer (formats: prodsearch_amd/pretrained.py).

``write_dir`` fills a ``pretrain_emb_dir``: ``word_emb.txt.gz`` and ``context_emb.txt.gz`` through
``pretrain_util.write_word_emb`` (shuffled rows, extra keys, a distinctive pad row, rounding-midpoint decimals; different
seeds, so a model that opens the wrong one of the two gets another table) and ``doc_emb.txt.gz`` (one row per review in file
order — the keys are not used —, a share of midpoint decimals as well).  ``write_up_dir`` fills a ``pretrain_up_emb_dir``:
``user_emb.txt`` / ``product_emb.txt``, plain text, a count line, a width line, space-separated rows.
"""
import gzip
import os

import numpy as np

import pretrain_util


def _values(rng, n, width, tie_share):
    vals = rng.standard_normal((n, width)) * 0.5
    rows = []
    for r in range(n):
        row = []
        for j in range(width):
            if rng.random() < tie_share:
                f = np.float32(vals[r, j])
                f = np.uint32(int(f.view(np.uint32)) & ~1).view(np.float32)          # even significand
                row.append(pretrain_util._tie_string(f))
            else:
                row.append(repr(float(vals[r, j])))
        rows.append(row)
    return rows


def write_doc_emb(path, n_reviews, d, seed=0, tie_share=0.15, width=None):
    """``doc_emb.txt.gz``: ``n_reviews`` rows (the model's review_count - 1), keys ``r<i>`` in a shuffled order (ignored)."""
    rng = np.random.default_rng(seed)
    width = d if width is None else width
    keys = ['r%d' % i for i in range(n_reviews)]
    rng.shuffle(keys)
    rows = _values(rng, n_reviews, width, tie_share)
    with open(path, 'wb') as raw:
        with gzip.GzipFile(fileobj=raw, mode='wb', mtime=0) as gz:
            gz.write(('%d\n%d\n' % (n_reviews, width)).encode())
            gz.write(''.join('%s\t%s\n' % (k, ' '.join(r)) for k, r in zip(keys, rows)).encode())


def write_user_item_emb(path, n_rows, d, seed=0, tie_share=0.15, width=None):
    """``user_emb.txt`` / ``product_emb.txt``: ``n_rows`` rows (user_size / product_size), not gzip."""
    rng = np.random.default_rng(seed)
    width = d if width is None else width
    rows = _values(rng, n_rows, width, tie_share)
    with open(path, 'w') as f:
        f.write('%d\n%d\n' % (n_rows, width))
        f.write(''.join(' '.join(r) + '\n' for r in rows))


def write_dir(path, words, review_count, d, seed=0, tie_share=0.15):
    os.makedirs(path, exist_ok=True)
    pretrain_util.write_word_emb(os.path.join(path, 'word_emb.txt.gz'), words, d, seed=seed + 1, tie_share=tie_share)
    pretrain_util.write_word_emb(os.path.join(path, 'context_emb.txt.gz'), words, d, seed=seed + 2, tie_share=tie_share)
    write_doc_emb(os.path.join(path, 'doc_emb.txt.gz'), review_count - 1, d, seed=seed + 3, tie_share=tie_share)
    return path


def write_up_dir(path, user_size, product_size, d, seed=0, tie_share=0.15):
    os.makedirs(path, exist_ok=True)
    write_user_item_emb(os.path.join(path, 'user_emb.txt'), user_size, d, seed=seed + 4, tie_share=tie_share)
    write_user_item_emb(os.path.join(path, 'product_emb.txt'), product_size, d, seed=seed + 5, tie_share=tie_share)
    return path
