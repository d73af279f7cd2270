"""Test-side oracle of the ZAM / AEM step (CPU, plain PyTorch fp32) and the loader of their golden fixtures.

``attn_forward`` restates ``ItemTransformerRanker.forward_attn`` with ``model_name`` 'ZAM' / 'AEM'
(models/item_transformer.py:361-438) on top of oracle.tem's ``query_encode`` / ``mha`` / ``bce_rank_loss`` /
``item_to_words``: the history rows (ZAM: a zero row prepended, always valid) are keys and values, the encoded query is
the one query, and the sequence representation is ``0.5 * attention + 0.5 * query``.  The negatives' attention runs on
B*K expanded copies exactly like the reference (their dropout masks differ).  Pinned by tests/golden/attn_*.npz.
"""
import os

import torch

from golden_util import GOLDEN_DIR, Golden
from oracle import tem as otem
from oracle.tem import no_dropout

ATTN_CASES = sorted(f[:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith('attn_') and f.endswith('.npz'))
PRE = 'attention_encoder.'


def history(P, args, ui, product_size):
    """Key / value rows [B,S,d] and the padded-key mask [B,S] (True = masked) of item_transformer.py:378-396."""
    hist_tab = P['hist_product_emb.weight'] if args.sep_prod_emb else P['product_emb.weight']
    emb = hist_tab[ui]
    pad = ui.eq(product_size)
    if args.model_name == 'ZAM':
        B, _, d = emb.shape
        emb = torch.cat([torch.zeros(B, 1, d, dtype=emb.dtype), emb], dim=1)
        pad = torch.cat([torch.zeros(B, 1, dtype=torch.bool), pad], dim=1)
    return emb, pad


def encode(P, args, q, hemb, hpad, drop=no_dropout, call=(0, 0), keep=None):
    top = otem.mha(P, PRE, hemb, q.unsqueeze(1), hpad, args.heads, drop, call, keep)
    return 0.5 * top[:, 0, :] + 0.5 * q                                              # :400-401, :406-407


def attn_forward(P, args, batch, neg_item_idxs, neg_word_idxs, vocab_size, product_size,
                 training=True, drop=None, keep=None):
    """Returns (loss, ps_loss, item_loss)."""
    drop = drop if (drop is not None and training) else no_dropout
    word_pad = vocab_size - 1
    tgt, ui = batch.target_prod_idxs, batch.u_item_idxs
    B, K = neg_item_idxs.shape
    q, qmean, _ = otem.query_encode(P, args, batch.query_word_idxs, word_pad, drop)
    hemb, hpad = history(P, args, ui, product_size)
    S, d = hemb.shape[1], hemb.shape[2]
    pos_out = encode(P, args, q, hemb, hpad, drop, (0, 0), keep)
    neg_out = encode(P, args, q.unsqueeze(1).expand(-1, K, -1).reshape(B * K, d),
                     hemb.unsqueeze(1).expand(-1, K, -1, -1).reshape(B * K, S, d),
                     hpad.unsqueeze(1).expand(-1, K, -1).reshape(B * K, S), drop, (1, 0)).view(B, K, d)
    target_emb = P['product_emb.weight'][tgt]
    neg_emb = P['product_emb.weight'][neg_item_idxs]
    pos_scores = (pos_out * target_emb).sum(-1)
    neg_scores = (neg_out * neg_emb).sum(-1)
    if args.sim_func == 'bias_product':
        pos_scores = pos_scores + P['product_bias'][tgt]
        neg_scores = neg_scores + P['product_bias'][neg_item_idxs]
    ps_loss = otem.bce_rank_loss(pos_scores, neg_scores, K if args.pos_weight else 1)
    item_loss = otem.item_to_words(P, tgt, batch.pos_iword_idxs, neg_word_idxs, word_pad, keep)
    if keep is not None:
        keep.update(query_mean=qmean, query_emb=q, enc=pos_out, neg_enc=neg_out, pos_scores=pos_scores,
                    neg_scores=neg_scores)
    return ps_loss + item_loss, ps_loss, item_loss


def attn_encode(P, args, batch, vocab_size, product_size):
    """Eval-mode sequence representation [B,d] (test_attn, item_transformer.py:148-187)."""
    q, _, _ = otem.query_encode(P, args, batch.query_word_idxs, vocab_size - 1, no_dropout)
    hemb, hpad = history(P, args, batch.u_item_idxs, product_size)
    return encode(P, args, q, hemb, hpad)


def attn_test(P, args, batch, vocab_size, product_size):
    """``test_attn`` scores [B,C] (item_transformer.py:148-195)."""
    out = attn_encode(P, args, batch, vocab_size, product_size)
    candi = batch.candi_prod_idxs
    scores = (out.unsqueeze(1) * P['product_emb.weight'][candi]).sum(-1)
    if args.sim_func == 'bias_product':
        scores = scores + P['product_bias'][candi]
    return scores


def philox_drop(args, seed, step, B, K, L):
    """The product's attention-model dropout masks: FS site, attention site of layer 0 with one query position."""
    from oracle.philox import PhiloxDropout
    S = L + (1 if args.model_name == 'ZAM' else 0)
    return PhiloxDropout(args.dropout, seed, step, B, K, args.heads, S, 1, 0)


class AttnGolden(Golden):
    def dropout(self, step):
        L = self.z['in_u_item_idxs'].shape[1]
        return philox_drop(self.args, self.args.seed, step + 1, self.B, self.K, L)
