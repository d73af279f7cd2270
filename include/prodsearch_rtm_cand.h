/* prodsearch_rtm_cand.h — the review transformer over per-entry candidate lists in one pass: the entries
 * beside prodsearch_hip.h's ps_rtm_rank_all, in csrc/rtm_rank.hip.  They take its descriptor, shape, tensors and catalogue index. */
#ifndef PRODSEARCH_RTM_CAND_H
#define PRODSEARCH_RTM_CAND_H
#include "prodsearch_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ RTM: per-entry candidate lists in one pass
 * The same factorisation for the evaluations that score a LIST per entry — validation on --valid_candi_size sampled products,
 * the rerank of --test_candi_size / uq_pids lists (trainer.py:189-226) — which nothing in it forbids: it never depended on which
 * items are scored.  desc, shape, params, index, item_ridxs: those of ps_rtm_rank_all, the same catalogue index; candi_prod_idxs
 * [B, C] int64 item ids, a slot outside [0, P) (the -1 padding of a ragged list) is dead: scored -inf, never ranked or listed.
 * Two entries' lists share no item, so rr_slot_kernel reads the K / V rows by review id from the index, one wave per pair, and
 * holds no LDS tile.  Refusals: those of ps_rtm_rank_all, with its messages; C >= 1; B * cands_per_pass < 2^30. */
/* bytes of scratch with `cands_per_pass` columns of the lists scored per pass (<= 0: the default, 32768 pairs); -1: refused /
 * bad sizes.  ps_rtm_rank_candidates sizes its passes from the scratch it is given: the most columns that fit. */
int64_t ps_rtm_rank_cand_scratch_bytes(const PsRtmDesc* desc, const PsRtmRankShape* shape, int64_t C, int32_t topk,
                                       int64_t cands_per_pass);
/* What ps_rtm_rank_candidates launches, from the rules the launcher itself reads (csrc/rtm_rank.hip: rr_pass_layout, rr_epl,
 * rr_lph, rr_tail_fused, rr_query_fs_fused).  Host only: no HIP call. */
typedef struct PsRtmRankCandPlan {
  int64_t cands_per_pass;       /* columns of the lists scored per pass: the most whose pairs fit the scratch          */
  int64_t passes;               /* ceil(C / cands_per_pass); a ragged last pass runs at the full pass shape            */
  int32_t epl;                  /* d / 64: the instantiation of rr_entry_kernel / rr_slot_kernel                       */
  int32_t lph;                  /* 64 / H: lanes per head                                                              */
  int32_t tail_fused;           /* the per-pair tail is the fused d = 128 kernel                                       */
  int32_t query_fs_fused;       /* the fs query encoder's projection runs inside the embed launch                      */
} PsRtmRankCandPlan;
int ps_rtm_rank_cand_plan(const PsRtmDesc* desc, const PsRtmRankShape* shape, int64_t C, int32_t topk, int64_t scratch_bytes,
                          PsRtmRankCandPlan* out);
/* rank [B] (optional, needs target_prod_idxs): 1 + the live slots ahead of the FIRST column that holds the target — a slot is
 * ahead with a greater score, or an equal one in a lower column — 0: no live slot holds it.  top_idx [B, topk]: ITEM ids of the
 * live slots by (score desc, column asc), duplicates of an id being slots of their own; unfilled places -1 / -inf.
 * scores_out (optional) [B, C] dense, -inf at dead slots.  A slot's bits do not depend on the pass it lands in, and equal
 * those ps_rtm_rank_all gives the same (entry, item).  scratch: 256-byte aligned. */
int ps_rtm_rank_candidates(const PsRtmDesc* desc, const PsRtmRankShape* shape, const PsRtmTensors* params, const float* index,
                           const int64_t* item_ridxs, const int64_t* query_word_idxs, const int64_t* u_ridxs,
                           const int64_t* candi_prod_idxs, int64_t C, const int64_t* target_prod_idxs, int32_t topk,
                           int64_t* top_idx, float* top_score, int32_t* rank, float* scores_out, void* scratch,
                           int64_t scratch_bytes, ps_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PRODSEARCH_RTM_CAND_H */
