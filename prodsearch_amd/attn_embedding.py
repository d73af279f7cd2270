"""AttentionEmbeddingRanker — the ZAM / AEM heads of the reference's ``ItemTransformerRanker`` on the HIP step.

``model_name`` 'ZAM' (Zero Attention Model) or 'AEM' (Attention Embedding Model): ``forward_attn`` / ``test_attn``
(``models/item_transformer.py:148-195, 361-438``).  The encoded search query attends over the user's purchase history
with ONE ``MultiHeadedAttention`` (``attention_encoder``, neural.py:192-231); the sequence representation is
``0.5 * attention + 0.5 * query``; scoring, the weighted BCE and ``item_to_words`` are the QEM head's.  ZAM prepends a zero
key / value row that is always attended to.

Same constructor signature, ``state_dict`` keys / order / shapes and initialisation as the reference (``attention_encoder``
keeps ``nn.Linear``'s default initialisation: the reference's ``initialize_parameters`` does not touch it), and the same
module API as :class:`ItemTransformerRanker`, whose plumbing this class reuses: the step is one C-ABI call per direction
(model ids ``PS_MODEL_ZAM`` / ``PS_MODEL_AEM``, kernels in ``csrc/attn_emb.hip``), ``attention_encoder.*`` travelling in
``PsTemTensors.layer[0]``.  ``ItemTransformerRanker`` itself still refuses these model names.
"""
from . import _lib
from .item_transformer import ItemTransformerRanker


class AttentionEmbeddingRanker(ItemTransformerRanker):
    MODEL_NAMES = ('ZAM', 'AEM')

    def _check_model_name(self, args):
        if args.model_name not in self.MODEL_NAMES:
            raise NotImplementedError("AttentionEmbeddingRanker: model_name %r (ZAM / AEM only)" % args.model_name)
        if getattr(args, 'shard_tables', False):
            raise NotImplementedError("shard_tables is not supported for the ZAM / AEM models")

    def _model_id(self):
        return _lib.PS_MODEL_ZAM if self.args.model_name == 'ZAM' else _lib.PS_MODEL_AEM

    def _uses_history(self):
        return True

    def _named_hot_params(self):
        ae = self.attention_encoder
        return super()._named_hot_params() + [
            (('layer', 0, 'wk'), ae.linear_keys.weight), (('layer', 0, 'bk'), ae.linear_keys.bias),
            (('layer', 0, 'wv'), ae.linear_values.weight), (('layer', 0, 'bv'), ae.linear_values.bias),
            (('layer', 0, 'wq'), ae.linear_query.weight), (('layer', 0, 'bq'), ae.linear_query.bias),
            (('layer', 0, 'wo'), ae.final_linear.weight), (('layer', 0, 'bo'), ae.final_linear.bias)]
