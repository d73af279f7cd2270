"""PretrainedProductRanker — the review transformer on pretrained, frozen paragraph vectors.

``ProductRanker`` with the three arguments the reference trains its ``pv`` / ``pvc`` runs with (``models/ps_model.py:73,
81-128, 163-182, 280-298``, ``models/PV.py:27-38``, ``others/util.py:4-34``; formats in :mod:`prodsearch_amd.pretrained`):

``pretrain_emb_dir`` (taken only if the path exists)
    * word table from ``context_emb.txt.gz`` when the ARGUMENT ``review_encoder_name`` is ``pvc`` (chosen before ``fix_emb``
      renames the encoder), else ``word_emb.txt.gz``; ``nn.Embedding.from_pretrained``: frozen, the pad row keeps the file's
      values, ``initialize_parameters`` leaves it alone; for ``pvc`` ``context_embeddings`` stays an alias of it;
    * ``pv``: ``review_encoder.review_embeddings`` from ``doc_emb.txt.gz`` (file order + one zero row), frozen, not
      re-initialised; ``review_count`` must be the file's rows + 1;
    * ``fs`` / ``avg``: the word table is frozen, ``review_encoder.f_W`` still trains.
``pretrain_up_emb_dir`` (taken only if the path exists; read only with ``use_user_emb`` / ``use_item_emb``)
    ``user_emb.txt`` / ``product_emb.txt`` + one zero row, frozen.
``fix_emb`` (``pv`` / ``pvc`` only; refused with ``fs`` / ``avg``, where the reference's forward ignores the flag and its
``test()`` reads a table computed before initialisation)
    an argument of ``pvc`` becomes the ``pv`` encoder (its ``state_dict`` keys, its table from ``doc_emb.txt.gz``);
    ``review_embeddings.weight.requires_grad = False`` with or without a directory; ``PV.forward``'s own ``drop_layer`` has
    p = 0 (the model's ``dropout_layer`` still applies); ``model.review_embeddings`` is the parameter from construction on and
    ``clear_review_embbeddings()`` is a no-op; the word table is NOT frozen by ``fix_emb`` alone.

A frozen table is outside the optimizer's parameter list and the clip norm (``optimizers.py:170``), has ``.grad is None``, a
NULL pointer in the C ABI's gradient struct and its bit in ``PsRtmDesc.frozen_mask``: the HIP backward then launches neither
the inverted word index nor the word-gradient reduce, and the embed backward runs its frozen form.  That
plumbing is ``ProductRanker``'s (it follows ``requires_grad``); this class only builds the tables.
"""
import os

import torch
import torch.nn as nn

from . import pretrained
from .ps_model import ProductRanker


class PretrainedProductRanker(ProductRanker):
    def _resolve_pretrained(self, args):
        self.fix_emb = bool(getattr(args, 'fix_emb', False))
        if self.fix_emb and args.review_encoder_name not in ('pv', 'pvc'):
            raise NotImplementedError("fix_emb is built for the pv / pvc review encoders only (review_encoder_name %r)"
                                      % args.review_encoder_name)
        self.pretrain_emb_dir = self.pretrain_up_emb_dir = None          # ps_model.py:81-86: a missing path is ignored
        if os.path.exists(getattr(args, 'pretrain_emb_dir', '') or ''):
            self.pretrain_emb_dir = args.pretrain_emb_dir
        if os.path.exists(getattr(args, 'pretrain_up_emb_dir', '') or ''):
            self.pretrain_up_emb_dir = args.pretrain_up_emb_dir

    def _pretrained_table(self, which):
        d = self.embedding_size
        if which in ('user', 'product'):
            if self.pretrain_up_emb_dir is None:
                return None
            fname, rows, pad = (pretrained.USER_EMB_FILE, self.user_pad_idx + 1, self.user_pad_idx) if which == 'user' else \
                (pretrained.PRODUCT_EMB_FILE, self.prod_pad_idx + 1, self.prod_pad_idx)
            tab = pretrained.user_item_table(os.path.join(self.pretrain_up_emb_dir, fname), rows, d)
            return nn.Embedding.from_pretrained(torch.from_numpy(tab), padding_idx=pad)
        if self.pretrain_emb_dir is None:
            return None
        if which == 'word':
            fname = pretrained.CONTEXT_EMB_FILE if self.args.review_encoder_name == 'pvc' else pretrained.WORD_EMB_FILE
            tab = pretrained.word_table(self.pretrain_emb_dir, self.vocab_words, self.vocab_size, d, fname)
            return nn.Embedding.from_pretrained(torch.from_numpy(tab), padding_idx=self.word_pad_idx)
        tab = pretrained.review_table(self.pretrain_emb_dir, self.review_count, d)
        return nn.Embedding.from_pretrained(torch.from_numpy(tab))       # (PV.py:31: no padding_idx; the table is frozen)
