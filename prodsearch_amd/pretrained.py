"""Pretrained tables (``--pretrain_emb_dir`` / ``--pretrain_up_emb_dir``; reference ``others/util.py:4-34``,
``models/item_transformer.py:38-43, 59-67``, ``models/ps_model.py:81-119``, ``models/PV.py:27-38``).

File ``<pretrain_emb_dir>/word_emb.txt.gz``, gzip text:

    <count>
    <width>
    <key>\t<v_0> <v_1> ... <v_{width-1}>
    ...

A row line is split as ``line.strip(' ').split('\t')``: field 0 is the key, field 1 holds the whitespace-separated values.
The key -> row map follows line order.  Values are parsed as Python floats (double) and THEN rounded to float32, as
``torch.FloatTensor(list_of_floats)`` does; a direct decimal -> float32 parse can differ in the last bit.

The item models' table is ``rows[[0] + [row(w) for w in words[1:]] + [len(words)]]``: row 0 is file row 0 whatever
``words[0]`` is, and the pad row ``V - 1`` is file row ``len(words)`` (not zero: ``nn.Embedding.from_pretrained`` leaves it).
The table is then frozen (``from_pretrained``'s default ``freeze=True``).

The review transformer reads the same format from ``context_emb.txt.gz`` (pvc) or ``word_emb.txt.gz`` (``word_table``'s
``fname``) and its ``pv`` review table from ``doc_emb.txt.gz`` (``review_table``: the rows in FILE order, keys ignored, plus one
appended zero row — the padding review).  ``pretrain_up_emb_dir`` holds ``user_emb.txt`` / ``product_emb.txt``
(``user_item_table``): plain text, a count line, a width line, then one row of space-separated values per line; one zero row —
the padding id — is appended.  All three parse doubles and round to float32.
"""
import gzip
import os

import numpy as np

WORD_EMB_FILE = 'word_emb.txt.gz'
CONTEXT_EMB_FILE = 'context_emb.txt.gz'
DOC_EMB_FILE = 'doc_emb.txt.gz'
USER_EMB_FILE = 'user_emb.txt'
PRODUCT_EMB_FILE = 'product_emb.txt'


def load_pretrain_embeddings(fname):
    """``(key -> row number, float32 [n_rows, width] array)`` of one embedding file (format above)."""
    keys = {}
    fields = []
    with gzip.open(fname, 'rt') as fin:
        int(fin.readline().strip())                   # count line (not trusted: the rows are what is read)
        int(fin.readline().strip())                   # width line (checked against the model by word_table)
        for line_no, line in enumerate(fin):
            arr = line.strip(' ').split('\t')
            if len(arr) < 2:
                raise ValueError("%s: row line %d has no tab-separated value field" % (fname, line_no + 1))
            keys[arr[0]] = line_no
            fields.append(arr[1].split())
    if not fields:
        raise ValueError("%s: no embedding rows" % fname)
    width = len(fields[0])
    for i, f in enumerate(fields):
        if len(f) != width:
            raise ValueError("%s: row %d has %d values, row 0 has %d" % (fname, i, len(f), width))
    flat = np.fromiter((float(x) for f in fields for x in f), dtype=np.float64, count=len(fields) * width)
    return keys, flat.reshape(len(fields), width).astype(np.float32)


def word_table(pretrain_emb_dir, vocab_words, vocab_size, embedding_size, fname=WORD_EMB_FILE):
    """The frozen word table [vocab_size, embedding_size] (float32 numpy) from ``pretrain_emb_dir``/``fname``."""
    fname = os.path.join(pretrain_emb_dir, fname)
    if vocab_words is None:
        raise ValueError("pretrain_emb_dir: the vocabulary words (vocab_words) are needed to map %s onto the table" % fname)
    words = list(vocab_words)
    if len(words) + 1 != vocab_size:
        raise ValueError("pretrain_emb_dir: vocab_size %d != len(vocab_words) + 1 = %d" % (vocab_size, len(words) + 1))
    keys, rows = load_pretrain_embeddings(fname)
    if rows.shape[1] != embedding_size:
        raise ValueError("%s: embeddings are %d wide, the model's embedding_size is %d" % (fname, rows.shape[1], embedding_size))
    idx = [0]
    for w in words[1:]:
        if w not in keys:
            raise KeyError("%s has no row for the vocabulary word %r" % (fname, w))
        idx.append(keys[w])
    idx.append(vocab_size - 1)
    if max(idx) >= rows.shape[0]:
        raise IndexError("%s: %d rows, but the table needs row %d (the pad row is file row len(vocab_words) = %d)"
                         % (fname, rows.shape[0], max(idx), vocab_size - 1))
    return np.ascontiguousarray(rows[np.asarray(idx, dtype=np.int64)])


def review_table(pretrain_emb_dir, review_count, embedding_size):
    """The ``pv`` encoder's frozen review table [review_count, embedding_size] from ``doc_emb.txt.gz`` (PV.py:27-31): the
    file's rows in file order plus one zero row.  The reference takes whatever the file holds and fails later, with an
    index error on the first review id past it; here ``review_count`` must be the file's rows + 1."""
    fname = os.path.join(pretrain_emb_dir, DOC_EMB_FILE)
    _, rows = load_pretrain_embeddings(fname)
    if rows.shape[1] != embedding_size:
        raise ValueError("%s: embeddings are %d wide, the model's embedding_size is %d" % (fname, rows.shape[1], embedding_size))
    if rows.shape[0] + 1 != review_count:
        raise ValueError("%s: %d rows, but review_count %d needs %d (one row per review; the padding row is appended)"
                         % (fname, rows.shape[0], review_count, review_count - 1))
    return np.ascontiguousarray(np.concatenate([rows, np.zeros((1, embedding_size), np.float32)]))


def load_user_item_embeddings(fname):
    """float32 [n_rows, width] array of a ``user_emb.txt`` / ``product_emb.txt`` file (others/util.py:22-34)."""
    fields = []
    with open(fname, 'r') as fin:
        int(fin.readline().strip())                   # count line (not trusted)
        int(fin.readline().strip())                   # width line (checked against the model by user_item_table)
        for line in fin:
            fields.append(line.strip().split(' '))
    if not fields:
        raise ValueError("%s: no embedding rows" % fname)
    width = len(fields[0])
    for i, f in enumerate(fields):
        if len(f) != width:
            raise ValueError("%s: row %d has %d values, row 0 has %d" % (fname, i, len(f), width))
    flat = np.fromiter((float(x) for f in fields for x in f), dtype=np.float64, count=len(fields) * width)
    return flat.reshape(len(fields), width).astype(np.float32)


def user_item_table(path, rows, embedding_size):
    """A frozen ``user_emb`` / ``product_emb`` table [rows, embedding_size] from the file ``path`` (ps_model.py:89-108): the
    file's rows plus one zero row — ``rows`` is ``user_size + 1`` / ``product_size + 1``, its last row the padding id."""
    tab = load_user_item_embeddings(path)
    if tab.shape[1] != embedding_size:
        raise ValueError("%s: embeddings are %d wide, the model's embedding_size is %d" % (path, tab.shape[1], embedding_size))
    if tab.shape[0] + 1 != rows:
        raise ValueError("%s: %d rows, but the table needs %d (one per id; the padding row is appended)"
                         % (path, tab.shape[0], rows - 1))
    return np.ascontiguousarray(np.concatenate([tab, np.zeros((1, embedding_size), np.float32)]))
