"""ProductRanker — drop-in boundary of the RTM (review_transformer) ranking-loss step.

Mirrors the reference's ``nn.Module`` contract (``models/ps_model.py:53-370``; call sites
``main.py:144-146``, ``trainer.py:74-79,190-201,225``):

    model = ProductRanker(args, device, vocab_size, review_count, product_size, user_size,
                          review_words, vocab_words, word_dists)
    loss = model(batch, train_pv)           # 0-dim fp32 tensor with a grad_fn
    model.zero_grad(); loss.backward(); optim.step()
    model.get_review_embeddings(); scores = model.test(batch); model.clear_review_embbeddings()

Same ``state_dict`` keys as the reference (incl. the aliases ``review_encoder.word_embeddings.weight``
and, for pvc, ``review_encoder.context_embeddings.weight``).  Supported review encoders: ``pv``, ``pvc`` (the reference
default), ``fs`` and ``avg`` (``ps_model.py:148-151``, ``:301-305``; ``models/text_encoder.py``), with or without the
per-position user / item embeddings (``use_user_emb`` / ``use_item_emb``).  ``pretrain_emb_dir`` / ``pretrain_up_emb_dir`` /
``fix_emb`` are :class:`prodsearch_amd.rtm_pretrained.PretrainedProductRanker`'s (this class refuses them, in the hook
``_resolve_pretrained``); what both share is here: a hot table whose ``requires_grad`` is False has no slice of the flat
gradient buffer, a NULL pointer in the gradient struct and its bit in ``PsRtmDesc.frozen_mask``.  All numerics run in
``libprodsearch_hip.so`` (``ps_rtm_*`` entry points); the torch modules are parameter holders.
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .hot_module import HotPathModule, _Holder, _Plan, encoder_layer_params
from .item_transformer import _FSEncoder, _TransformerEncoder, _init_like_reference


class _ReviewEncoder(_Holder):
    """Holder with the reference's attribute names (PV.py:18-34, PVC.py:18-30)."""
    def __init__(self, word_embeddings, name, review_count, d, review_embeddings=None):
        super().__init__()
        self.word_embeddings = word_embeddings
        if name == 'pv':
            self.review_embeddings = review_embeddings if review_embeddings is not None else \
                nn.Embedding(review_count, d, padding_idx=review_count - 1)
        else:
            self.context_embeddings = word_embeddings


class _CatalogueIndex(object):
    """What ``ProductRanker.catalogue_index`` returns: the projection, the catalogue it serves and what it was built from."""
    __slots__ = ('model', 'index', 'item_ridxs', 'review_u_p', 'shape3', 'stamp', 'table')

    def stale(self):
        """A weight, a table, the catalogue or the review-embedding table it was projected from has changed (the table it
        was built from is held here, so clearing the model's copy does not by itself make the projection stale)."""
        return self.model._rank_all_stamp(self.item_ridxs, self.review_u_p, self.table) != self.stamp


class _TimelineIndex(object):
    """What ``ProductRanker.timeline_index`` returns: the projection (the one ``catalogue_index`` builds: it holds no review
    list) and the time-ordered CSR it serves — ``ptr`` [P + 1], ``rids`` / ``times`` [N] on the device."""
    __slots__ = ('model', 'index', 'ptr', 'rids', 'times', 'review_u_p', 'shape3', 'stamp', 'table')

    def stale(self):
        """``_CatalogueIndex.stale`` with the timeline's three arrays in the catalogue's place."""
        return self.model._rank_all_stamp(self.ptr, self.rids, self.times, self.review_u_p, self.table) != self.stamp


class ProductRanker(HotPathModule):
    def __init__(self, args, device, vocab_size, review_count, product_size, user_size,
                 review_words, vocab_words, word_dists=None):
        super(ProductRanker, self).__init__()
        if args.review_encoder_name not in ('pv', 'pvc', 'fs', 'avg'):
            raise NotImplementedError("review_encoder_name %r: pv / pvc / fs / avg are built" % args.review_encoder_name)
        self._resolve_pretrained(args)
        self.args = args
        self.device = device
        self.train_review_only = args.train_review_only
        self.embedding_size = d = args.embedding_size
        self.vocab_words = vocab_words
        self.vocab_size, self.review_count = vocab_size, review_count
        self.word_dists = None if word_dists is None else torch.as_tensor(word_dists, dtype=torch.float64)
        self.prod_pad_idx, self.user_pad_idx = product_size, user_size
        self.word_pad_idx = vocab_size - 1
        self.seg_pad_idx = 3
        self.review_pad_idx = review_count - 1
        # (fix_emb turns an argument of pvc into the pv encoder, ps_model.py:125-128; the word FILE is chosen on the argument)
        self.review_encoder_name = 'pv' if (self.fix_emb and args.review_encoder_name == 'pvc') else args.review_encoder_name
        if not torch.is_tensor(review_words) and not getattr(args, 'do_subsample_mask', False) and \
                len({len(x) for x in review_words}) > 1:
            # ps_model.py:75-78: ragged review texts are cut / padded to review_word_limit (others/util.py:pad)
            lim = int(args.review_word_limit)
            review_words = [list(x[:lim]) + [self.word_pad_idx] * (lim - len(x)) for x in review_words]
        rw = torch.as_tensor(np.asarray(review_words), dtype=torch.int64) if not torch.is_tensor(review_words) \
            else review_words.to(torch.int64)
        if rw.dim() != 2:
            raise ValueError("review_words must be a padded [review_count, review_word_limit] table "
                             "(the reference pads it with others/util.py:pad)")
        self.review_words = rw.to(device)                       # plain attribute, as in the reference (:79)

        # registration order follows ps_model.py:88-126 so state_dicts line up key for key
        self.use_user_emb, self.use_item_emb = bool(args.use_user_emb), bool(args.use_item_emb)
        if self.use_user_emb:
            self.user_emb = self._pretrained_table('user') or nn.Embedding(user_size + 1, d, padding_idx=self.user_pad_idx)
        if self.use_item_emb:
            self.product_emb = self._pretrained_table('product') or \
                nn.Embedding(product_size + 1, d, padding_idx=self.prod_pad_idx)
        self.word_embeddings = self._pretrained_table('word') or nn.Embedding(vocab_size, d, padding_idx=self.word_pad_idx)
        self.transformer_encoder = _TransformerEncoder(d, args.ff_size, args.inter_layers)
        if self.review_encoder_name == 'fs':
            self.review_encoder = _FSEncoder(d)              # review_encoder.f_W (ps_model.py:148-149)
        elif self.review_encoder_name == 'avg':
            self.review_encoder = _Holder()                  # AVGEncoder has no parameters (:150-151)
        else:
            self.review_encoder = _ReviewEncoder(self.word_embeddings, self.review_encoder_name, review_count, d,
                                                 self._pretrained_table('review') if self.review_encoder_name == 'pv' else None)
            if self.fix_emb:                                 # PV.py:36-38 (pv only: fs / avg with fix_emb are refused)
                self.review_encoder.review_embeddings.weight.requires_grad = False
        self.query_encoder = _FSEncoder(d) if args.query_encoder_name == 'fs' else _Holder()
        self.seg_embeddings = nn.Embedding(4, d, padding_idx=self.seg_pad_idx)
        self.review_embeddings = None
        if self.fix_emb:
            self.get_review_embeddings()                     # ps_model.py:163-168: the parameter itself, from construction on
        self.initialize_parameters()
        self.to(device)
        self._reset_cache()
        self._fwd_step = 0
        self._seed = int(getattr(args, 'seed', 666))

    # ------------------------------------------------------- pretrained tables (hooks)
    def _resolve_pretrained(self, args):
        """Sets ``pretrain_emb_dir`` / ``pretrain_up_emb_dir`` (None: not taken) and ``fix_emb``.  This class builds none of
        them and refuses; :class:`prodsearch_amd.rtm_pretrained.PretrainedProductRanker` overrides the hook."""
        if getattr(args, 'fix_emb', False):
            raise NotImplementedError("fix_emb is outside the built path of ProductRanker: use PretrainedProductRanker "
                                      "(trainer.create_model dispatches to it)")
        # (a directory that does not exist is ignored, as the reference ignores it: ps_model.py:81-86)
        if any(os.path.exists(getattr(args, k, '') or '') for k in ('pretrain_emb_dir', 'pretrain_up_emb_dir')):
            raise NotImplementedError("pretrain_emb_dir / pretrain_up_emb_dir are outside the built path of ProductRanker: "
                                      "use PretrainedProductRanker (trainer.create_model dispatches to it)")
        self.pretrain_emb_dir = self.pretrain_up_emb_dir = None
        self.fix_emb = False

    def _pretrained_table(self, which):
        """A frozen ``nn.Embedding`` for 'user' / 'product' / 'word' / 'review' from the pretrained files, or None."""
        return None

    # ---------------------------------------------------------------- reference API
    def initialize_parameters(self, logger=None):
        """ps_model.py:360-370 (+ PV.py:82-90); a pretrained table keeps its values."""
        if self.pretrain_emb_dir is None:
            nn.init.normal_(self.word_embeddings.weight)
        nn.init.normal_(self.seg_embeddings.weight)
        if self.review_encoder_name == 'pv' and self.pretrain_emb_dir is None:
            nn.init.normal_(self.review_encoder.review_embeddings.weight)
        elif self.review_encoder_name == 'fs':
            _init_like_reference(self.review_encoder)
        if self.args.query_encoder_name == 'fs':
            _init_like_reference(self.query_encoder)
        _init_like_reference(self.transformer_encoder)

    def clear_review_embbeddings(self):           # (sic) reference spelling, ps_model.py:177
        if not self.fix_emb:                      # fix_emb: the table is the frozen parameter and stays (:179)
            self.review_embeddings = None

    def get_review_embeddings(self, batch_size=128):
        """ps_model.py:186-203: the table ``test`` indexes (pv: the parameter itself; pvc: one launch
        computing the uncorrupted mean of every review's words, last row 0)."""
        if self.review_embeddings is not None:
            return
        if self.review_encoder_name == 'pv':
            self.review_embeddings = self.review_encoder.review_embeddings.weight
            return
        lib = _lib.load()
        ps, _ = self._structs()
        d = self._desc(1, 0, 1, eval_mode=True, C=1)
        rw = self.review_words if self.review_words.is_cuda else self.review_words.to(self._dev())
        self.review_words = rw.contiguous()
        d.WL = rw.shape[1]
        out = torch.empty(self.review_count, self.embedding_size, device=self._dev(), dtype=torch.float32)
        scratch = torch.empty_like(out) if self.review_encoder_name == 'fs' else None
        _lib.check(lib.ps_rtm_review_embeddings(d, ps, self.review_words.data_ptr(), _lib.ptr(scratch), out.data_ptr(),
                                                self._stream()), 'ps_rtm_review_embeddings')
        self.review_embeddings = out
        self.__dict__['_rev_emb_stamp'] = self._rank_all_stamp()      # (catalogue_index: is this table still the weights'?)

    # ------------------------------------------------------- the whole catalogue in one pass (evaluate.rank_all_rtm)
    def _rank_all_refusal(self, time_ordered=False):
        """Why ``catalogue_index`` / ``rank_all_rtm`` cannot serve this configuration (the message names the flag), or None.
        ``PretrainedProductRanker`` is served: it inherits ``test``, which reads the same ``review_embeddings`` table.
        ``time_ordered``: asked by ``timeline_index`` / ``rank_seq_rtm``, which serve the time-ordered mode as well."""
        a = self.args
        if a.inter_layers != 1:
            return ("rank_all_rtm: inter_layers = %d — one encoder layer is built (deeper encoders need every position of "
                    "layer 0)" % a.inter_layers)
        if not time_ordered and getattr(a, 'do_seq_review_test', False) and not a.train_review_only:
            return ("rank_all_rtm: do_seq_review_test without train_review_only — an item's review list then depends on "
                    "the entry")
        if self.fix_emb and self.review_encoder_name in ('fs', 'avg'):
            return "rank_all_rtm: fix_emb with the fs / avg review encoders is not built"
        return None

    def _rank_all_stamp(self, *extra):
        """What something derived from the weights was built from: storage and torch version of every hot parameter
        (``load_state_dict``, ``.to``, in-place edits) and of ``extra``, and the number of optimizer steps this process has
        taken (``optimizers.STEPS_TAKEN``: the step kernels write the parameters through raw pointers, which the version
        counters do not see; a step on another model counts too — a needless rebuild, never a stale result)."""
        from .optimizers import STEPS_TAKEN
        ts = [p for _, p in self._named_hot_params()] + [t for t in extra if t is not None]
        return tuple((t.data_ptr(), t._version) for t in ts), STEPS_TAKEN[0]

    def _rank_all_desc(self, B, Q, shape_U, index_shape=None):
        a = self.args
        d = self._desc(B, 0, int(a.uprev_review_limit) + int(a.iprev_review_limit), True, 1, Q)
        sh = _lib.PsRtmRankShape()
        if index_shape is not None:
            sh.n_items, sh.review_u_p_rows, sh.I = index_shape
        sh.U = shape_U
        sh.seq_review_test = int(bool(getattr(a, 'do_seq_review_test', False)) and not a.train_review_only)
        sh.fix_emb = int(self.fix_emb)
        return d, sh

    def catalogue_index(self, item_ridxs, review_u_p=None):
        """The per-evaluation projection of ``evaluate.rank_all_rtm`` (``ps_rtm_rank_index``): every review's key / value
        rows and the [segment][position] tables.  ``item_ridxs`` [P, I] int64 on the device: each product's reviews, then the
        review pad id (``ProdSearchDataLoader.catalogue_reviews``).  ``review_u_p`` [n_reviews, 2] (author, item) is read only
        with ``use_user_emb`` / ``use_item_emb``.  Builds ``review_embeddings`` if needed.  Cached: the same inputs and
        unchanged weights give the same object back; an index whose sources changed is refused by ``rank_all_rtm``.  A cached
        pvc / fs / avg review table that the weights have moved away from is rebuilt first."""
        msg = self._rank_all_refusal()
        if msg is not None:
            raise NotImplementedError(msg)
        item_ridxs = self._idx(item_ridxs, 'item_ridxs')
        if item_ridxs.dim() != 2:
            raise RuntimeError("item_ridxs must be [P, I]")
        review_u_p = self._rank_review_u_p(review_u_p, 'catalogue_index')
        self._rank_review_table()
        stamp = self._rank_all_stamp(item_ridxs, review_u_p, self.review_embeddings)
        cached = self.__dict__.get('_cat_index')
        if cached is not None and cached.stamp == stamp:
            return cached
        shape3 = (item_ridxs.shape[0], 0 if review_u_p is None else review_u_p.shape[0], item_ridxs.shape[1])
        out = self._rank_project(shape3, review_u_p)
        idx = _CatalogueIndex()
        idx.model, idx.index, idx.item_ridxs, idx.review_u_p, idx.shape3, idx.stamp = self, out, item_ridxs, review_u_p, shape3, stamp
        idx.table = self.review_embeddings
        self.__dict__['_cat_index'] = idx
        return idx

    def _rank_review_u_p(self, review_u_p, who):
        """``review_u_p`` [n_reviews, 2] on the device where ``use_user_emb`` / ``use_item_emb`` read it, else None."""
        if not (self.use_user_emb or self.use_item_emb):
            return None
        if review_u_p is None:
            raise RuntimeError("use_user_emb / use_item_emb: %s needs review_u_p" % who)
        review_u_p = torch.as_tensor(np.asarray(review_u_p), dtype=torch.int64).reshape(-1, 2) \
            if not torch.is_tensor(review_u_p) else review_u_p
        return self._idx(review_u_p.to(self._dev()), 'review_u_p')

    def _rank_review_table(self):
        """The review table the projection reads: a pvc / fs / avg table computed from weights that have changed since (an
        optimizer step without clear_review_embbeddings()) is computed again; pv / fix_emb: the parameter itself."""
        if self.review_embeddings is not None and self.review_encoder_name != 'pv' and \
                self.__dict__.get('_rev_emb_stamp') != self._rank_all_stamp():
            self.review_embeddings = None
        if self.review_embeddings is None:
            self.get_review_embeddings()

    def _rank_project(self, shape3, review_u_p, clear_seq=False):
        """``ps_rtm_rank_index`` over the current review table -> the projection, a flat fp32 tensor."""
        lib = _lib.load()
        ps, _ = self._structs()
        d, sh = self._rank_all_desc(1, 1, 1, shape3)
        if clear_seq:
            sh.seq_review_test = 0
        n = lib.ps_rtm_rank_index_floats(d, sh)
        if n < 0:
            raise RuntimeError("ps_rtm_rank_index_floats: %s" % lib.ps_last_error().decode('utf-8', 'replace'))
        out = torch.empty(n, device=self._dev(), dtype=torch.float32)
        tab = self.review_embeddings.detach().contiguous()
        _lib.check(lib.ps_rtm_rank_index(d, sh, ps, tab.data_ptr(), _lib.ptr(review_u_p), out.data_ptr(), self._stream()),
                   'ps_rtm_rank_index')
        return out

    @staticmethod
    def _timeline_check(ptr, rids, times):
        """``timeline_index``'s check, torch ops on the tensors' own device: ``ptr`` rises from 0 to N and ``times`` never falls
        inside an item; a RuntimeError names the first item that breaks either."""
        N = rids.numel()
        bad = torch.nonzero(ptr[1:] < ptr[:-1]).flatten()
        if int(ptr[0]) != 0 or int(ptr[-1]) != N or bad.numel():
            raise RuntimeError("timeline_index: ptr must rise from 0 to N = %d (ptr[0] = %d, ptr[-1] = %d%s)"
                               % (N, int(ptr[0]), int(ptr[-1]), ", falls after item %d" % int(bad[0]) if bad.numel() else ""))
        if N < 2:
            return
        inner = torch.ones(N - 1, dtype=torch.bool, device=ptr.device)         # a fall across two items' border is none
        border = ptr[1:-1]
        border = border[(border > 0) & (border < N)]
        inner[border - 1] = False
        at = torch.nonzero((times[1:] < times[:-1]) & inner).flatten()
        if at.numel():
            item = int(torch.searchsorted(ptr, at[:1] + 1, right=True)[0]) - 1
            raise RuntimeError("timeline_index: the times of item %d are not in order (element %d of the timeline)"
                               % (item, int(at[0]) + 1))

    def timeline_index(self, ptr, rids, times, review_u_p=None):
        """The index of ``evaluate.rank_seq_rtm``, the time-ordered evaluation (``do_seq_review_test`` without
        ``train_review_only``): the projection of ``catalogue_index`` plus the items' time-ordered review sequences as a CSR —
        ``ptr`` [P + 1], ``rids`` [N] review ids per item in time order, ``times`` [N] their time stamps, int64 on the device
        (``ProdSearchDataLoader.timeline``).  A pair reads the ``iprev_review_limit`` reviews of its item that sit just before
        ``bisect_right(times of the item, the entry's stamp)``.  Checked once, on the device: ``ptr`` starts at 0, never
        decreases and ends at N, and ``times`` never decreases inside an item — the reference's binary search returns
        *something* on an unsorted sequence; here that is a RuntimeError naming the item.  Works on a model built with or
        without ``do_seq_review_test``; cached and refused when stale like a catalogue index."""
        msg = self._rank_all_refusal(time_ordered=True)
        if msg is not None:
            raise NotImplementedError(msg)
        ptr, rids, times = self._idx(ptr, 'ptr'), self._idx(rids, 'rids'), self._idx(times, 'times')
        if ptr.dim() != 1 or ptr.numel() < 2 or rids.dim() != 1 or times.shape != rids.shape or rids.numel() < 1:
            raise RuntimeError("timeline_index: ptr must be [P + 1], rids and times [N] with N >= 1")
        ptr, rids, times = ptr.contiguous(), rids.contiguous(), times.contiguous()
        review_u_p = self._rank_review_u_p(review_u_p, 'timeline_index')
        self._rank_review_table()
        stamp = self._rank_all_stamp(ptr, rids, times, review_u_p, self.review_embeddings)
        cached = self.__dict__.get('_seq_index')
        if cached is not None and cached.stamp == stamp:
            return cached
        self._timeline_check(ptr, rids, times)
        P = ptr.numel() - 1
        shape3 = (P, 0 if review_u_p is None else review_u_p.shape[0], int(self.args.iprev_review_limit))
        # seq_review_test cleared: ps_rtm_rank_index refuses the time-ordered mode for the static rankers' sake (their [P, I]
        # catalogue does not exist in it), but the projection holds no review list and is the same in both modes
        out = self._rank_project(shape3, review_u_p, clear_seq=True)
        idx = _TimelineIndex()
        idx.model, idx.index, idx.ptr, idx.rids, idx.times = self, out, ptr, rids, times
        idx.review_u_p, idx.shape3, idx.stamp, idx.table = review_u_p, shape3, stamp, self.review_embeddings
        self.__dict__['_seq_index'] = idx
        return idx

    def forward(self, batch_data, train_pv=True, neg_word_idxs=None):
        return self._loss_forward(*self._run_forward(batch_data, bool(train_pv), neg_word_idxs))

    def test(self, batch_data):
        return self._run_score(batch_data)

    # -------------------------------------------------------------------- plumbing
    _TENSORS = _lib.PsRtmTensors

    def _reset_cache(self):
        self._plans = {}
        self._params_struct = self._grads_struct = None
        self._grad_flat = self._grad_views = None
        self._alias = None

    def _named_hot_params(self):
        a, te = self.args, self.transformer_encoder
        out = [(('word_emb',), self.word_embeddings.weight), (('seg_emb',), self.seg_embeddings.weight),
               (('final_ln_g',), te.layer_norm.weight), (('final_ln_b',), te.layer_norm.bias),
               (('wo_w',), te.wo.weight), (('wo_b',), te.wo.bias)]
        if self.review_encoder_name == 'pv':
            out.append((('review_emb',), self.review_encoder.review_embeddings.weight))
        if self.review_encoder_name == 'fs':
            out += [(('rev_fs_w',), self.review_encoder.f_W.weight), (('rev_fs_b',), self.review_encoder.f_W.bias)]
        if self.use_user_emb:
            out.append((('user_emb',), self.user_emb.weight))
        if self.use_item_emb:
            out.append((('product_emb',), self.product_emb.weight))
        if a.query_encoder_name == 'fs':
            out += [(('fs_w',), self.query_encoder.f_W.weight), (('fs_b',), self.query_encoder.f_W.bias)]
        out += encoder_layer_params(te)
        return out

    _TABLE_BITS = (('word_emb', _lib.PS_RTM_FROZEN_WORD), ('review_emb', _lib.PS_RTM_FROZEN_REVIEW),
                   ('user_emb', _lib.PS_RTM_FROZEN_USER), ('product_emb', _lib.PS_RTM_FROZEN_ITEM))

    def _hot_tables(self):
        """The tables a caller (or ``from_pretrained`` / ``fix_emb``) may freeze: C-ABI field name -> parameter."""
        out = {'word_emb': self.word_embeddings.weight}
        if self.review_encoder_name == 'pv':
            out['review_emb'] = self.review_encoder.review_embeddings.weight
        if self.use_user_emb:
            out['user_emb'] = self.user_emb.weight
        if self.use_item_emb:
            out['product_emb'] = self.product_emb.weight
        return out

    def _frozen_mask(self):
        tabs = self._hot_tables()
        return sum(bit for name, bit in self._TABLE_BITS if name in tabs and not tabs[name].requires_grad)

    def _has_grad(self, path):
        if len(path) == 1 and path[0] in ('word_emb', 'review_emb', 'user_emb', 'product_emb'):
            return self._hot_tables()[path[0]].requires_grad      # frozen: NULL gradient, no slice of the flat buffer
        if path == ('seg_emb',):
            return bool(self.args.use_seg_emb)
        if path[0] == 'layer' and path[2] in ('ln_g', 'ln_b'):
            return path[1] != 0
        return True

    def _grad_key(self):
        return self._frozen_mask()      # one mask over at most four parameters per call

    def _fill_extra(self, ps):
        ps.pe = self.transformer_encoder.pos_emb.pe.data_ptr()

    def _regrade_refusal(self):
        if self.__dict__.get('_param_flat') is not None:
            return ("requires_grad of an embedding table changed after the first step: not supported with a "
                    "data-parallel exchange")
        return None

    def _regraded(self):
        """The cached descriptors carry the frozen mask and are dropped with the old gradient layout.  A flip BETWEEN a
        forward and its backward is not supported: the backward then holds the forward's descriptor with the old mask beside
        the rebuilt gradient struct, and ``ps_rtm_backward`` refuses the pair (its frozen_mask message) before launching
        anything."""
        self._plans = {}
        for p in self._hot_tables().values():        # touched lists belong to the old gradient layout
            if getattr(p, '_ps_rows', None) is not None:
                del p._ps_rows

    # ------------------------------------------------------------ row-sparse optimizer support
    def _row_sparse(self):
        """``args.row_sparse_adam``: the trainable tables below are zeroed, clipped and updated by the rows a step touched
        (untouched rows keep p, m, v: DESIGN.md §5b).  With ``args.lazy_exact_adam`` — the dense optimizer's results, which
        this model has no replay for — the model stays on the dense path, which IS that result."""
        a = self.args
        return bool(getattr(a, 'row_sparse_adam', False)) and not bool(getattr(a, 'lazy_exact_adam', False))

    def _sparse_paths(self):
        """The trainable id-addressed tables: review (pv) / user / item, and the word table under the pv encoder only — the
        word-mean encoders address ~16 word slots per vocabulary row a step, which is not sparse."""
        if not self._row_sparse():
            return ()
        tabs = self._hot_tables()
        names = ('review_emb', 'user_emb', 'product_emb') + (('word_emb',) if self.review_encoder_name == 'pv' else ())
        return tuple((n,) for n in names if n in tabs and tabs[n].requires_grad)

    def _index_lists(self, path, plan):
        ls = plan.lists
        if path == ('review_emb',):
            return [ls['pos_prod_ridxs'], ls['neg_prod_ridxs']], self.review_pad_idx
        if path == ('user_emb',):
            return [ls['pos_user_idxs'], ls['neg_user_idxs']], self.user_pad_idx
        if path == ('product_emb',):
            return [ls['pos_item_idxs'], ls['neg_item_idxs']], self.prod_pad_idx
        words = [ls['query_word_idxs']]
        if plan.desc.train_pv:                       # the PV loss: each positive review's window words and their draws
            words += [ls['pos_prod_rword_idxs'], ls['neg_word_idxs']]
        return words, self.word_pad_idx

    def _index_cap_bound(self, path):
        """Largest index count a batch of ``args.batch_size`` entries can address in ``path``'s table, whatever the batch:
        the sequence width is padded per batch (<= R = uprev_review_limit + iprev_review_limit), every entry brings
        ``neg_per_pos`` negative sequences, and the user / item ids have one more position than the reviews.  The word
        table (row-sparse under pv only) sees the queries and, in a PV step, ``pv_window_size`` words per positive review
        with ``neg_per_pos`` draws each.  ``args.max_query_len`` is the corpus-wide padded query length; left at None the
        word table's bound is its row count — safe, the message is merely larger.  The data-parallel row exchange sizes its
        fixed-capacity messages with the maximum of this over the ranks (dist.TablesGradExchange)."""
        a = self.args
        B, K = int(a.batch_size), int(a.neg_per_pos)
        R = int(a.uprev_review_limit) + int(a.iprev_review_limit)
        if path == ('review_emb',):
            return B * (1 + K) * R
        if path in (('user_emb',), ('product_emb',)):
            return B * (1 + K) * (R + 1)
        Qmax = getattr(a, 'max_query_len', None)
        if Qmax is None:
            return int(self.word_embeddings.weight.shape[0])
        return B * int(Qmax) + B * R * max(1, int(a.pv_window_size)) * (1 + K)

    def _desc(self, B, K, R, eval_mode, C=0, Q=1, W=1, WL=0, train_pv=False):
        a = self.args
        d = _lib.PsRtmDesc()
        d.B, d.K, d.R, d.Q, d.W, d.WL, d.C = B, K, R, Q, W, WL, C
        d.d, d.H, d.F, d.n_layers = a.embedding_size, a.heads, a.ff_size, a.inter_layers
        d.vocab_size, d.review_count = self.vocab_size, self.review_count
        d.review_encoder = dict(pv=_lib.PS_RENC_PV, pvc=_lib.PS_RENC_PVC, fs=_lib.PS_RENC_FS, avg=_lib.PS_RENC_AVG)[self.review_encoder_name]
        d.query_encoder = _lib.PS_QENC_FS if a.query_encoder_name == 'fs' else _lib.PS_QENC_AVG
        d.use_pos_emb, d.use_seg_emb, d.pos_weight = int(a.use_pos_emb), int(a.use_seg_emb), int(a.pos_weight)
        d.train_pv = int(train_pv)
        d.training = int(bool(self.training) and not eval_mode)
        d.dropout, d.corrupt_rate = float(a.dropout), float(a.corrupt_rate)
        d.seed, d.step = self._seed, 0
        d.use_user_emb, d.use_item_emb = int(self.use_user_emb), int(self.use_item_emb)
        d.user_size, d.product_size = self.user_pad_idx, self.prod_pad_idx
        d.frozen_mask = 0 if eval_mode else self._frozen_mask()
        d.no_pv_drop = int(self.fix_emb)
        return d

    def _seq_ids(self, bt, batch, names, shape, keep):
        """Per-position user / item ids (ps_model.py:325-334, :233-238): [.., R+1] int64, position 0 = pad."""
        want = []
        if self.use_user_emb:
            want += [n for n in names if 'user' in n]
        if self.use_item_emb:
            want += [n for n in names if 'item' in n]
        for n in names:
            setattr(bt, n, None)
        taken = {}
        for n in want:
            t = self._idx(getattr(batch, n, None), n)
            if t is None:
                raise RuntimeError("use_user_emb / use_item_emb: the batch lacks %s" % n)
            exp = shape[n]
            if tuple(t.shape) != exp:
                raise RuntimeError("batch.%s has shape %s, expected %s" % (n, tuple(t.shape), exp))
            setattr(bt, n, t.data_ptr())
            keep.append(t)
            taken[n] = t
        return taken

    @staticmethod
    def _idx(t, name, dtype=torch.int64):
        if t is None:
            return None
        if not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda:
            raise RuntimeError("batch.%s must be a %s tensor on the model's device" % (name, dtype))
        return t if t.is_contiguous() else t.contiguous()

    def _plan(self, key, desc, eval_mode):
        plan = self._plans.get(key)
        if plan is None:
            lib = _lib.load()
            import ctypes as C
            tot = C.c_int64(0)
            _lib.check(lib.ps_rtm_workspace_floats(desc, int(eval_mode), C.byref(tot)), 'ps_rtm_workspace_floats')
            lay = _lib.PsRtmWsLayout()
            _lib.check(lib.ps_rtm_workspace_layout(desc, int(eval_mode), lay), 'ps_rtm_workspace_layout')
            plan = _Plan()
            plan.key, plan.desc, plan.layout, plan.batch = key, desc, lay, _lib.PsRtmBatch()
            plan.ws = torch.empty(tot.value, device=self._dev(), dtype=torch.float32)
            plan.neg_words = plan.keep = None
            self._plans[key] = plan
        return plan

    def _sample_pv_words(self, plan, n_rev, W, K):
        """``torch.multinomial(word_dists, B*R*W*K)`` (PV.py:57 / PVC.py:81) on the device."""
        lib = _lib.load()
        if plan.neg_words is None:
            plan.neg_words = torch.empty(n_rev, W * K, device=self._dev(), dtype=torch.int64)
            plan.dummy_items = torch.empty(1, device=self._dev(), dtype=torch.int64)
        sd = _lib.PsTemDesc()
        sd.B, sd.K, sd.W = n_rev, K, W
        sd.product_size, sd.vocab_size = 1, self.vocab_size
        sd.seed, sd.step = self._seed, self._fwd_step
        prob, alias = self._alias_tables()
        # item draws are not needed here: ask for zero of them by sampling only the word stream (B*W*K words)
        items = torch.empty(n_rev * K, device=self._dev(), dtype=torch.int64)
        _lib.check(lib.ps_sample_negatives(sd, prob.data_ptr(), alias.data_ptr(), items.data_ptr(),
                                           plan.neg_words.data_ptr(), self._stream()), 'ps_sample_negatives')
        return plan.neg_words

    _POS_SEQ = (('pos_prod_ridxs', 1, 'review'), ('pos_seg_idxs', 1, 'seg'), ('pos_user_idxs', 1, 'user'),
                ('pos_item_idxs', 1, 'item'), ('pos_prod_rword_idxs', 1, 'word3'), ('pos_prod_rword_masks', 1, 'mask3'),
                ('pos_prod_rword_idxs_pvc', 1, 'word3'))
    _NEG_SEQ = (('neg_prod_ridxs', 2, 'review'), ('neg_seg_idxs', 2, 'seg'), ('neg_user_idxs', 2, 'user'),
                ('neg_item_idxs', 2, 'item'), ('neg_prod_rword_idxs', 2, 'word3'), ('neg_prod_rword_masks', 2, 'mask3'),
                ('neg_prod_rword_idxs_pvc', 2, 'word3'))

    def _same_width(self, batch):
        """The reference pads the positive and the negative sequences of a batch separately (prod_search_dataloader.py:
        283-300), so their review counts can differ; the kernels run every sequence of a step at one width.  The
        shorter side is padded here with the pad ids — masked positions, no effect on the loss or any gradient."""
        rp, rn = batch.pos_prod_ridxs.shape[1], batch.neg_prod_ridxs.shape[2]
        if rp == rn:
            return batch
        pads = dict(review=self.review_pad_idx, seg=self.seg_pad_idx, user=self.user_pad_idx, item=self.prod_pad_idx,
                    word3=self.word_pad_idx, mask3=0)
        grow, by = (self._POS_SEQ, rn - rp) if rp < rn else (self._NEG_SEQ, rp - rn)

        class _Padded(object):
            pass
        out = _Padded()
        out.__dict__.update(batch.__dict__)
        for name, dim, kind in grow:
            t = getattr(batch, name, None)
            if t is None:
                continue
            spec = [0, 0] * (t.dim() - 1 - dim) + [0, by]      # F.pad lists the last dimension first
            setattr(out, name, torch.nn.functional.pad(t, spec, value=pads[kind]))
        return out

    def _run_forward(self, batch, train_pv, neg_word_idxs=None):
        lib = _lib.load()
        ps, _ = self._structs()
        b = self._same_width(batch)
        qw = self._idx(b.query_word_idxs, 'query_word_idxs')
        pr = self._idx(b.pos_prod_ridxs, 'pos_prod_ridxs')
        nr = self._idx(b.neg_prod_ridxs, 'neg_prod_ridxs')
        B, Q = qw.shape
        R, K = pr.shape[1], nr.shape[1]
        if tuple(nr.shape) != (B, K, R):
            raise RuntimeError("neg_prod_ridxs has shape %s, expected %s" % (tuple(nr.shape), (B, K, R)))
        pvc = self.review_encoder_name in ('pvc', 'fs', 'avg')      # the word-mean encoders: review vectors from review words
        if self.review_encoder_name in ('fs', 'avg'):
            train_pv = False                                         # "pv" not in the name: no PV loss (ps_model.py:264)
        pw = self._idx(b.pos_prod_rword_idxs, 'pos_prod_rword_idxs')
        W = pw.shape[2] if train_pv else max(1, self.args.pv_window_size)
        WL = 0
        if pvc:
            src = b.pos_prod_rword_idxs_pvc if train_pv else b.pos_prod_rword_idxs
            if src is None:
                raise RuntimeError("pvc encoder: the batch lacks the review word indices")
            WL = src.shape[2]
        key = (B, K, R, Q, W, WL, bool(train_pv), bool(self.training))
        desc = self._desc(B, K, R, False, 0, Q, W, WL, train_pv)
        plan = self._plan(key, desc, False)
        self._fwd_step += 1
        plan.desc.step = self._fwd_step
        bt = plan.batch
        keep = [qw, pr, nr, pw]
        bt.query_word_idxs, bt.pos_prod_ridxs, bt.neg_prod_ridxs = qw.data_ptr(), pr.data_ptr(), nr.data_ptr()
        bt.pos_prod_rword_idxs = pw.data_ptr()
        for name, dtype in (('pos_seg_idxs', torch.int64), ('neg_seg_idxs', torch.int64),
                            ('pos_prod_rword_masks', torch.uint8), ('neg_prod_rword_masks', torch.uint8),
                            ('neg_prod_rword_idxs', torch.int64),
                            ('pos_prod_rword_idxs_pvc', torch.int64), ('neg_prod_rword_idxs_pvc', torch.int64)):
            t = self._idx(getattr(b, name, None), name, dtype)
            lead = {'pos_seg_idxs': (B, R + 1), 'neg_seg_idxs': (B, K, R + 1)}.get(
                name, (B, K, R) if name.startswith('neg') else (B, R))
            if t is not None and tuple(t.shape[:len(lead)]) != lead:
                raise RuntimeError("batch.%s has shape %s, expected %s + word axis" % (name, tuple(t.shape), lead))
            setattr(bt, name, None if t is None else t.data_ptr())
            keep.append(t)
        if train_pv:
            if neg_word_idxs is None:
                neg_word_idxs = self._sample_pv_words(plan, B * R, W, K)
            nw = self._idx(neg_word_idxs, 'neg_word_idxs')
            if nw.numel() != B * R * W * K:
                raise RuntimeError("neg_word_idxs must hold B*R*W*K = %d draws" % (B * R * W * K))
            bt.neg_word_idxs = nw.data_ptr()
            keep.append(nw)
        seq = self._seq_ids(bt, b, ('pos_user_idxs', 'neg_user_idxs', 'pos_item_idxs', 'neg_item_idxs'),
                            dict(pos_user_idxs=(B, R + 1), pos_item_idxs=(B, R + 1),
                                 neg_user_idxs=(B, K, R + 1), neg_item_idxs=(B, K, R + 1)), keep)
        plan.keep = keep
        # what the kernels read, by name: the row-sparse optimizer's touched lists are built from these (_index_lists)
        plan.lists = dict(seq, query_word_idxs=qw, pos_prod_ridxs=pr, neg_prod_ridxs=nr, pos_prod_rword_idxs=pw,
                          neg_word_idxs=nw if train_pv else None)
        loss3 = torch.empty(3, device=self._dev(), dtype=torch.float32)
        _lib.check(lib.ps_rtm_forward(plan.desc, ps, bt, plan.ws.data_ptr(), loss3.data_ptr(), self._stream()),
                   'ps_rtm_forward')
        return plan, loss3

    def _run_backward(self, plan, grad_out):
        lib = _lib.load()
        ps, gs = self._structs()
        st = self._stream()
        if self._assign_grads():
            if not self.__dict__.get('_grad_clean', False):     # (clean: the last optimizer step left the buffer at 0)
                self._zero_for_backward()
        else:
            self._refuse_dirty_accumulation()
        self.__dict__['_grad_clean'] = False
        if self._row_sparse():
            self._coalesce_touched(plan)        # the lists need the step's indices only: three launches at the head
        go = None if grad_out is None else grad_out.contiguous().float()          # None: d loss / d loss = 1
        _lib.check(lib.ps_rtm_backward(plan.desc, ps, plan.batch, plan.ws.data_ptr(), gs, 1.0,
                                       None if go is None else go.data_ptr(), st), 'ps_rtm_backward')

    def _run_score(self, batch):
        lib = _lib.load()
        ps, _ = self._structs()
        if self.review_embeddings is None:
            self.get_review_embeddings()
        qw = self._idx(batch.query_word_idxs, 'query_word_idxs')
        cr = self._idx(batch.candi_prod_ridxs, 'candi_prod_ridxs')
        cs = self._idx(batch.candi_seg_idxs, 'candi_seg_idxs')
        B, C, R = cr.shape
        key = ('eval', B, C, R, qw.shape[1])
        desc = self._desc(B, 0, R, True, C, qw.shape[1], 1, int(self.review_words.shape[1]))
        plan = self._plan(key, desc, True)
        bt = plan.batch
        tab = self.review_embeddings.detach().contiguous()
        bt.query_word_idxs, bt.candi_prod_ridxs, bt.candi_seg_idxs = qw.data_ptr(), cr.data_ptr(), cs.data_ptr()
        bt.review_embeddings = tab.data_ptr()
        keep = [qw, cr, cs, tab]
        self._seq_ids(bt, batch, ('candi_seq_user_idxs', 'candi_seq_item_idxs'),
                      dict(candi_seq_user_idxs=(B, C, R + 1), candi_seq_item_idxs=(B, C, R + 1)), keep)
        plan.keep = keep
        scores = torch.empty(B, C, device=self._dev(), dtype=torch.float32)
        _lib.check(lib.ps_rtm_score(plan.desc, ps, bt, plan.ws.data_ptr(), scores.data_ptr(), self._stream()),
                   'ps_rtm_score')
        return scores
