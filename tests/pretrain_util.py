"""Synthetic ``word_emb.txt.gz`` files for the pretrained-word-table tests (format: prodsearch_amd/pretrained.py).

``write_word_emb`` makes a file that is not a trivial image of the vocabulary:
  * the rows are in a shuffled order, and ``n_extra`` keys that are not vocabulary words are mixed in;
  * file row ``len(words)`` — the table's pad row — is an extra key with distinctive values;
  * a share of the values are decimals just above a float32 rounding midpoint, so close to it that the double they
    parse to IS the midpoint: double -> float32 (ties to even) rounds them DOWN where a direct decimal -> float32 parse
    rounds them up.  Only a double-then-float32 parser reproduces the reference's table bit for bit.
"""
import gzip
from decimal import Decimal, getcontext

import numpy as np

getcontext().prec = 60


def _tie_string(f32):
    """A decimal string that parses (as a double) to the midpoint between ``f32`` and the next float32 away from zero,
    though its exact value lies above that midpoint; ``f32`` must have an even significand."""
    f = np.float32(f32)
    g = np.nextafter(f, np.float32(np.inf) if f > 0 else np.float32(-np.inf), dtype=np.float32)
    m = (float(f) + float(g)) / 2.0                      # exact in double
    up = np.nextafter(m, np.inf if f > 0 else -np.inf)
    s = Decimal(m) + (Decimal(float(up)) - Decimal(m)) / 4
    return format(s, 'f')


def vocab_words(V, prefix='w'):
    """The vocabulary the models take (``vocab_size = len(words) + 1``); words[0] has no row in the file."""
    return ['<unk>'] + ['%s%d' % (prefix, i) for i in range(1, V - 1)]


def write_word_emb(path, words, d, seed=0, n_extra=37, tie_share=0.15, n_rows=None, width=None):
    """Write ``path`` (a .txt.gz) for ``words``; returns (keys in file order, float64 values as written).
    ``n_rows`` < len(words) + 1 writes a short file; ``width`` overrides the written width."""
    rng = np.random.default_rng(seed)
    width = d if width is None else width
    keys = list(words[1:]) + ['xk%d' % i for i in range(n_extra)]
    rng.shuffle(keys)
    pad_key = 'xk_pad_row'
    keys.insert(len(words), pad_key)                    # file row len(words): the pad row of the table
    if n_rows is not None:
        keys = keys[:n_rows]
    vals = rng.standard_normal((len(keys), width)) * 0.5
    lines = []
    for r, k in enumerate(keys):
        if k == pad_key:
            row = ['%.6f' % (3.25 + 0.125 * j) for j in range(width)]
        else:
            row = []
            for j in range(width):
                if rng.random() < tie_share:
                    f = np.float32(vals[r, j])
                    bits = int(f.view(np.uint32))
                    f = np.uint32(bits & ~1).view(np.float32)          # even significand
                    row.append(_tie_string(f))
                else:
                    row.append(repr(float(vals[r, j])))
        lines.append('%s\t%s\n' % (k, ' '.join(row)))
    with open(path, 'wb') as raw:
        with gzip.GzipFile(fileobj=raw, mode='wb', mtime=0) as gz:
            gz.write(('%d\n%d\n' % (len(keys), width)).encode())
            gz.write(''.join(lines).encode())
    return keys
