"""HotPathModule — the host plumbing that connects an ``nn.Module`` of parameter holders to the C ABI, once.

``ItemTransformerRanker`` (and ``AttentionEmbeddingRanker``) and ``ProductRanker`` (and ``PretrainedProductRanker``) derive
from it.  What it owns is the protocol ``dist.py``, ``optimizers.py``, ``sharded.py`` and ``bench.py`` read:

  * ``_structs()`` -> (parameter struct, gradient struct): raw pointers of every hot tensor, and ONE flat fp32 gradient
    buffer ``_grad_flat`` with a view per graded parameter (``_grad_views``), laid out by :func:`flat_layout`;
  * ``_regrade()``: the rebuild of that layout when a table's ``requires_grad`` flips between steps;
  * the loss tensor whose plain ``backward()`` is one C-ABI call (``_loss_forward``), ``_assign_grads`` and the dense
    ``_zero_for_backward``, the per-shape ``_Plan`` cache, the alias tables of the word sampler.

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
                 'coalesced_at')
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
        """Sort key of a graded parameter in the flat buffer (the sort is stable)."""
        return p.numel()

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
        self._structs_built([(path, p, v) for (path, p), (_, v) in zip(graded, self._grad_views)])
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
        _lib.check(_lib.load().ps_zero_floats(self._grad_flat.data_ptr(), self._grad_flat.numel(), self._stream()),
                   'ps_zero_floats')

    # --------------------------------------------------------------- test support
    def workspace_view(self, plan, name, shape):
        """View of one intermediate inside the workspace (parity tests compare every stage)."""
        off = getattr(plan.layout, name)
        n = 1
        for s in shape:
            n *= s
        return plan.ws[off:off + n].view(*shape)
