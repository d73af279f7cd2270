"""HotPathModule — the host plumbing that connects an ``nn.Module`` of parameter holders to the C ABI, once.

``ItemTransformerRanker`` (and ``AttentionEmbeddingRanker``) and ``ProductRanker`` (and ``PretrainedProductRanker``) derive
from it.  What it owns is the protocol ``dist.py``, ``optimizers.py``, ``sharded.py`` and ``bench.py`` read:

  * ``_structs()`` -> (parameter struct, gradient struct): raw pointers of every hot tensor, and ONE flat fp32 gradient
    buffer ``_grad_flat`` with a view per graded parameter (``_grad_views``), laid out by :func:`flat_layout`;
  * ``_regrade()``: the rebuild of that layout when a table's ``requires_grad`` flips between steps;
  * the loss tensor whose plain ``backward()`` is one C-ABI call (``_loss_forward``), ``_assign_grads`` and the dense
    ``_zero_for_backward``, the per-shape ``_Plan`` cache, the alias tables of the word sampler;
  * the row-sparse optimizer's host side (``args.row_sparse_adam``): the touched-row lists of a step's index tensors
    (``_coalesce_touched`` -> ``p._ps_rows``, which ``Optimizer._build_plan`` looks for), ``touched_rows``,
    ``check_index_errors``, the zeroing of rows a backward left dirty and the refusal to accumulate over them.  A model names
    its tables and lists in ``_row_sparse`` / ``_sparse_paths`` / ``_index_lists``.

A model supplies the hooks listed under "hooks" below.  This module imports neither model and runs no device code on import.
"""
import torch
import torch.nn as nn

from . import _lib


class _Holder(nn.Module):
    def forward(self, *a, **k):     # pragma: no cover - never on the hot path
        raise RuntimeError("parameter holder: the hot path runs in libprodsearch_hip.so")


# -------------------------------------------------------------------- autograd
def _check_same_forward(model, step):
    """Each batch shape owns ONE workspace (activations, sampled negatives, batch pointers) that the next forward
    overwrites, so only the most recent forward can be differentiated — unlike autograd, which would keep both graphs
    alive.  Anything else must fail loudly rather than return the other forward's gradients."""
    if model._fwd_step != step:
        raise RuntimeError("backward() of a loss whose forward is no longer the model's latest one (forward #%d, now #%d): "
                           "the HIP workspace holds one forward at a time; call backward() before the next forward()"
                           % (step, model._fwd_step))


class _RankLossFn(torch.autograd.Function):
    """One node: forward launched the HIP forward; backward launches the HIP backward,
    which writes the dense ``.grad`` of every reachable parameter directly."""

    @staticmethod
    def forward(ctx, anchor, model, plan, loss3):
        ctx.model, ctx.plan, ctx.step = model, plan, model._fwd_step
        return loss3[0]

    @staticmethod
    def backward(ctx, grad_out):
        _check_same_forward(ctx.model, ctx.step)
        ctx.model._run_backward(ctx.plan, grad_out)
        return None, None, None, None


class _LossTensor(torch.Tensor):
    """The 0-dim loss ``forward`` returns.  It is an ordinary autograd tensor (``grad_fn`` = the node above), but the
    trainer's plain ``loss.backward()`` (trainer.py:77) — no ``gradient``, no ``inputs``, no ``create_graph`` — is
    d loss/d loss = 1 through a single node, so it calls the HIP backward directly: no autograd-engine round trip on
    the host and no ``ones_like`` fill kernel on the device.  Anything else (scaled losses, retained graphs) takes the
    normal autograd path."""

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        fast = self.__dict__.pop('_ps_fast', None)
        if fast is not None and gradient is None and not create_graph and inputs is None and not retain_graph:
            model, plan, step = fast
            _check_same_forward(model, step)         # the workspace must still hold this forward's activations
            model._run_backward(plan, None)
            return None
        return super().backward(gradient, retain_graph, create_graph, inputs)


class _Plan(object):
    """Per-shape cached call state: descriptor, batch struct, workspace (+ what each model parks beside them)."""
    __slots__ = ('desc', 'batch', 'ws', 'layout', 'key', 'neg_items', 'neg_words', 'dummy_items', 'keep', 'staged',
                 'coalesced_at', 'lists')
    __getitem__ = lambda self, slot: getattr(self, slot)     # the review model's plans were dicts: plan['desc'] still reads


# ---------------------------------------------------------------------- layout
def encoder_layer_params(te):
    """(C-ABI field path, parameter) of every layer of a ``_TransformerEncoder`` holder: 16 per layer, ``PsLayerTensors``."""
    out = []
    for i, l in enumerate(te.transformer_inter):
        sa, ff = l.self_attn, l.feed_forward
        out += [(('layer', i, 'wk'), sa.linear_keys.weight), (('layer', i, 'bk'), sa.linear_keys.bias),
                (('layer', i, 'wv'), sa.linear_values.weight), (('layer', i, 'bv'), sa.linear_values.bias),
                (('layer', i, 'wq'), sa.linear_query.weight), (('layer', i, 'bq'), sa.linear_query.bias),
                (('layer', i, 'wo'), sa.final_linear.weight), (('layer', i, 'bo'), sa.final_linear.bias),
                (('layer', i, 'w1'), ff.w_1.weight), (('layer', i, 'b1'), ff.w_1.bias),
                (('layer', i, 'w2'), ff.w_2.weight), (('layer', i, 'b2'), ff.w_2.bias),
                (('layer', i, 'ff_ln_g'), ff.layer_norm.weight), (('layer', i, 'ff_ln_b'), ff.layer_norm.bias),
                (('layer', i, 'ln_g'), l.layer_norm.weight), (('layer', i, 'ln_b'), l.layer_norm.bias)]
    return out


def slice_floats(numel):
    """Floats one tensor occupies in the flat buffer: its length rounded up to 16 bytes."""
    return (numel + 3) // 4 * 4


def flat_layout(numels, pad_to=4):
    """The flat gradient (and parameter) buffer's rule: slices in the given order, each 16-byte aligned, the total padded
    to a multiple of ``pad_to`` (``dist.flatten_parameters``: 4 * world).  Returns (offsets, total), in floats."""
    offsets, cur = [], 0
    for n in numels:
        offsets.append(cur)
        cur += slice_floats(n)
    return offsets, (cur + pad_to - 1) // pad_to * pad_to


# ------------------------------------------------------------------------ base
class HotPathModule(nn.Module):
    # ---------------------------------------------------------------------- hooks
    _TENSORS = None                 # the C-ABI tensor struct (_lib.PsTemTensors / _lib.PsRtmTensors)

    def _named_hot_params(self):
        """[(C-ABI field path, parameter)] of every tensor the kernels read."""
        raise NotImplementedError

    def _has_grad(self, path):
        """Does the step write a gradient for ``path``?  (False: ``.grad`` stays None, NULL in the gradient struct.)"""
        return True

    def _grad_key(self):
        """The value whose change since the structs were built makes ``_structs`` re-plan the gradients (``_regrade``)."""
        return None

    def _grad_order(self, path, p):
        """Sort key of a graded parameter in the flat buffer (the sort is stable): by size, the row-sparse tables behind
        everything dense."""
        return (path in self._sparse_paths(), p.numel())

    def _row_sparse(self):
        """``args.row_sparse_adam`` as this model takes it: table gradients stay dense tensors, but zeroing / clip / Adam
        only visit the rows a step touched."""
        return False

    def _sparse_paths(self):
        """Paths of the tables handled by their touched-row lists (empty unless ``_row_sparse()``)."""
        return ()

    def _index_lists(self, path, plan):
        """([index tensors of the step that address ``path``'s rows], that table's pad row)."""
        raise NotImplementedError

    def _fill_extra(self, ps):
        """Fields of the parameter struct that are not parameters."""

    def _structs_built(self, graded):
        """``graded`` = [(path, parameter, gradient view)] in buffer order: derive what the model keeps beside the structs."""

    def _regrade_refusal(self):
        """The message with which ``_regrade`` refuses in the model's current mode, or None."""
        return None

    def _reset_cache(self):
        """Drop every cached pointer (the storage may have moved)."""
        raise NotImplementedError

    # -------------------------------------------------------------- reference API
    def load_cp(self, pt, strict=True):
        self.load_state_dict(pt['model'], strict=strict)

    # ------------------------------------------------------------------- plumbing
    def _dev(self):
        p = self.word_embeddings.weight
        if not p.is_cuda:
            raise RuntimeError("%s needs its parameters on a gfx950 device (no CPU fallback): model.to('cuda')"
                               % type(self).__name__)
        return p.device

    def _stream(self):
        return torch.cuda.current_stream(self._dev()).cuda_stream

    def _anchor(self):
        a = getattr(self, '_anchor_t', None)
        if a is None or a.device != self._dev():
            a = torch.zeros((), device=self._dev(), requires_grad=True)
            self._anchor_t = a
        return a

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._reset_cache()          # storage may have moved: drop cached pointers
        return r

    @staticmethod
    def _set_field(struct, path, value):
        if path[0] == 'layer':
            setattr(struct.layer[path[1]], path[2], value)
        else:
            setattr(struct, path[0], value)

    def _graded(self, hot):
        """The graded (path, parameter) pairs of ``hot`` in flat-buffer order."""
        return sorted(((path, p) for path, p in hot if self._has_grad(path)), key=lambda t: self._grad_order(*t))

    def _grad_layout(self):
        """([(path, offset, numel)] per graded parameter, total floats) of the flat gradient buffer.  Allocates nothing and
        needs no device."""
        graded = self._graded(self._named_hot_params())
        offs, total = flat_layout([p.numel() for _, p in graded], int(self.__dict__.get('_flat_pad_to', 4)))
        return [(path, o, p.numel()) for (path, p), o in zip(graded, offs)], total

    def _structs(self):
        if self._params_struct is not None:
            if self.__dict__.get('_grad_key_at') == self._grad_key():
                return self._params_struct, self._grads_struct
            self._regrade()
        dev = self._dev()
        hot = self._named_hot_params()
        ps, gs = self._TENSORS(), self._TENSORS()
        for path, p in hot:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("parameters must be contiguous fp32")
            self._set_field(ps, path, p.data_ptr())
        self._fill_extra(ps)
        # one flat gradient buffer; dist.flatten_parameters asks for a total that is a multiple of 4 * world
        graded = self._graded(hot)
        offs, total = flat_layout([p.numel() for _, p in graded], int(self.__dict__.get('_flat_pad_to', 4)))
        self._grad_flat = torch.zeros(total, device=dev, dtype=torch.float32)
        self._grad_views = []
        for (path, p), o in zip(graded, offs):
            v = self._grad_flat[o:o + p.numel()].view_as(p)
            self._grad_views.append((p, v))
            self._set_field(gs, path, v.data_ptr())
        built = [(path, p, v) for (path, p), (_, v) in zip(graded, self._grad_views)]
        # row-sparse mode: the flat buffer is [dense tensors | row-sparse tables]; only the first part is ever memset,
        # table rows are re-zeroed by the optimizer (or zero_grad) through their touched list
        sparse = self._sparse_paths()
        self._n_dense_grad = sum(slice_floats(p.numel()) for path, p, _ in built if path not in sparse)
        self._sparse_tabs = [t for t in built if t[0] in sparse]
        self._structs_built(built)
        self._params_struct, self._grads_struct = ps, gs
        self.__dict__['_grad_key_at'] = self._grad_key()
        return ps, gs

    def _regrade(self):
        """``_grad_key()`` changed since the structs were built (a table's ``requires_grad`` flipped): the gradient struct,
        the flat gradient buffer and its views are rebuilt by the caller (_structs), so a frozen table never receives a
        gradient and a trainable one never loses it.  The gradients of the previous layout are dropped (``.grad = None``, as
        after ``zero_grad()``); the optimizer re-plans on the new ``.grad`` tensors, keeping its moments.  The modes that
        cannot follow (``_regrade_refusal``) refuse; what a model caches on the old layout it drops in ``_regraded``."""
        msg = self._regrade_refusal()
        if msg is not None:
            raise RuntimeError(msg)
        for p, v in self._grad_views or ():
            if p.grad is not None:
                if p.grad is not v and p.grad.data_ptr() != v.data_ptr():
                    raise RuntimeError("a foreign .grad tensor is attached to a hot-path parameter; "
                                       "call model.zero_grad() before backward")
                p.grad = None
        self.__dict__['_grad_clean'] = False
        self._params_struct = self._grads_struct = None
        self._grad_flat = self._grad_views = None
        self._regraded()

    def _regraded(self):
        """What ``_regrade`` drops beyond the structs and the flat buffer."""

    def _alias_tables(self):
        if self._alias is None:
            if self.word_dists is None:
                raise RuntimeError("word_dists is required to sample negative words "
                                   "(or pass neg_word_idxs= explicitly)")
            lib = _lib.load()
            wd = self.word_dists.contiguous()
            n = wd.numel()
            prob = torch.empty(n, dtype=torch.float32)
            alias = torch.empty(n, dtype=torch.int32)
            _lib.check(lib.ps_build_alias_host(wd.data_ptr(), n, prob.data_ptr(), alias.data_ptr()),
                       'ps_build_alias_host')
            self._alias = (prob.to(self._dev()), alias.to(self._dev()))
        return self._alias

    def _loss_forward(self, plan, loss3):
        """The tail of ``forward``: the loss as a tensor whose plain ``backward()`` calls the HIP backward directly."""
        if not torch.is_grad_enabled():
            return loss3[0]
        out = _RankLossFn.apply(self._anchor(), self, plan, loss3).as_subclass(_LossTensor)
        out._ps_fast = (self, plan, self._fwd_step)
        return out

    def _assign_grads(self):
        """Give every reachable parameter its dense ``.grad`` view; returns True if the flat
        buffer must be zeroed first (i.e. zero_grad() ran, trainer.py:76)."""
        fresh = self._grad_views[0][0].grad is None
        for p, v in self._grad_views:
            if p.grad is None:
                p.grad = v
            elif p.grad.data_ptr() != v.data_ptr():
                raise RuntimeError("a foreign .grad tensor is attached to a hot-path parameter; "
                                   "call model.zero_grad() before backward")
        return fresh

    def _zero_for_backward(self):
        lib = _lib.load()
        st = self._stream()
        if not self._row_sparse():
            _lib.check(lib.ps_zero_floats(self._grad_flat.data_ptr(), self._grad_flat.numel(), st), 'ps_zero_floats')
            return
        _lib.check(lib.ps_zero_floats(self._grad_flat.data_ptr(), self._n_dense_grad, st), 'ps_zero_floats')
        for path, p, gview in self._sparse_tabs:
            info = getattr(p, '_ps_rows', None)
            if info is not None and info['dirty']:       # touched by a backward no optimizer step consumed
                rows, count, cap = self._rows_view(info)
                _lib.check(lib.ps_zero_rows(gview.data_ptr(), p.shape[1], rows.data_ptr(), count.data_ptr(), cap, st),
                           'ps_zero_rows')
                info['dirty'] = False

    # ------------------------------------------------------------ row-sparse optimizer support
    def _refuse_dirty_accumulation(self):
        """A second backward onto gradients the first one left (no ``zero_grad()``, no ``optim.step()`` between): its touched
        lists would replace the first one's, whose rows nobody could find again."""
        if self._row_sparse() and any(getattr(p, '_ps_rows', {}).get('dirty') for _, p, _ in self._sparse_tabs):
            raise NotImplementedError("row_sparse_adam: gradient accumulation over several backwards is not "
                                      "supported; call model.zero_grad() (trainer.py:76) or optim.step() first")

    def _coalesce_touched(self, plan):
        """The sorted unique non-pad row ids of the step's index lists, per row-sparse table (``p._ps_rows``): one
        ``ps_coalesce_tables`` call for every ``_lib.PS_MAX_COALESCE_TABLES`` tables that have lists."""
        lib = _lib.load()
        dev, st = self._dev(), self._stream()
        work = []
        for path, p, gview in self._sparse_tabs:
            lists, pad = self._index_lists(path, plan)
            info = getattr(p, '_ps_rows', None)
            total = sum(t.numel() for t in lists)
            cap = max(1, min(total, p.shape[0]))
            if info is None or info['rows'].numel() < cap or info['grad_ptr'] != gview.data_ptr():
                info = dict(rows=torch.empty(cap, device=dev, dtype=torch.int64),
                            count=torch.zeros(1, device=dev, dtype=torch.int32),
                            ws=torch.zeros(lib.ps_coalesce_ws_bytes(p.shape[0]), device=dev, dtype=torch.uint8),
                            grad_ptr=gview.data_ptr(), dirty=False)
                p._ps_rows = info
            info['cap'] = cap
            info['active'] = None          # a data-parallel exchange installs the ranks' union here (dist.SparseGradExchange)
            if not lists:
                info['count'].zero_()
                continue
            work.append((p, info, lists, pad))
        for k in range(0, len(work), _lib.PS_MAX_COALESCE_TABLES):
            chunk = work[k:k + _lib.PS_MAX_COALESCE_TABLES]
            tabs = (_lib.PsCoalesceTable * len(chunk))()
            for t, (p, info, lists, pad) in zip(tabs, chunk):
                for i, x in enumerate(lists):
                    t.lists[i].idx, t.lists[i].n = x.data_ptr(), x.numel()
                t.n_lists, t.n_rows, t.pad_row = len(lists), p.shape[0], pad
                t.ws_dev, t.rows_out_dev, t.cap = info['ws'].data_ptr(), info['rows'].data_ptr(), info['rows'].numel()
                t.count_out_dev = info['count'].data_ptr()
            _lib.check(lib.ps_coalesce_tables(tabs, len(chunk), st), 'ps_coalesce_tables')
        for _, info, _, _ in work:
            info['dirty'] = True

    @staticmethod
    def _rows_view(info):
        """(rows, count, cap) the optimizer and zero_grad walk: the ranks' union after an exchange, else this rank's."""
        return info.get('active') or (info['rows'], info['count'], info['cap'])

    def touched_rows(self):
        """{state_dict key: sorted unique row ids} of the last backward (row-sparse mode; host sync)."""
        self.check_index_errors()
        out = {}
        for name, p in self.named_parameters():
            info = getattr(p, '_ps_rows', None)
            if info is not None:
                rows, count, _ = self._rows_view(info)
                out[name] = rows[:int(count[0])].clone()
        return out

    def check_index_errors(self):
        """Row-sparse mode: raise if a step's index lists held a row outside its table or overflowed a touched list
        (the kernels drop such rows and set a status word; reading it is a host sync, so the step itself never does —
        the trainer calls this where it reads the loss)."""
        if not self._row_sparse():
            return
        lib = _lib.load()
        for name, p in self.named_parameters():
            info = getattr(p, '_ps_rows', None)
            if info is None:
                continue
            for ws in (info['ws'], (info.get('xchg') or {}).get('ws')):
                if ws is None:
                    continue
                addr = lib.ps_coalesce_bad_flag(ws.data_ptr(), p.shape[0])
                off = addr - ws.data_ptr()
                flag = int(ws[off:off + 4].view(torch.int32)[0])
                if flag:
                    ws[off:off + 4].zero_()
                    raise RuntimeError("row-sparse step: %s" % ("an index outside [0, %d) addressed %s" % (p.shape[0], name)
                                       if flag == 1 else "touched-row list of %s overflowed its capacity" % name))

    # --------------------------------------------------------------- test support
    def workspace_view(self, plan, name, shape):
        """View of one intermediate inside the workspace (parity tests compare every stage)."""
        off = getattr(plan.layout, name)
        n = 1
        for s in shape:
            n *= s
        return plan.ws[off:off + n].view(*shape)
