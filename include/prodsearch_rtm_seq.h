/* prodsearch_rtm_seq.h — the review transformer's one-pass evaluation in the TIME-ORDERED setting: the entries
 * beside prodsearch_hip.h's ps_rtm_rank_all and prodsearch_rtm_cand.h's ps_rtm_rank_candidates, in csrc/rtm_rank.hip.  They take
 * the same descriptor, shape, tensors and projection (ps_rtm_rank_index, which holds no review list). */
#ifndef PRODSEARCH_RTM_SEQ_H
#define PRODSEARCH_RTM_SEQ_H
#include "prodsearch_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ RTM: the time-ordered evaluation in one pass
 * --do_seq_review_test with --train_review_only False: every review written before the entry's purchase is available, so an
 * item's review list depends on the entry (prod_search_dataloader.py:60-77, 138-147; prod_search_dataset.py:133-151).  A pair
 * (entry e, item i) reads the shape->I (iprev_review_limit) reviews of item i that sit just before a cut in the item's
 * time-ordered sequence, cut = the number of its times <= time_stamps[e] (bisect_right).  The key / value rows still depend on
 * the review id alone, so the projection and the entry side are ps_rtm_rank_all's; rr_slot_kernel puts a wave-wide search and a
 * window lookup in front of the same walk.   A pair's bits equal those ps_rtm_rank_all / ps_rtm_rank_candidates give
 * the same list in a static catalogue.
 * The entries accept either value of shape->seq_review_test: the field says what the run is, and these entries serve both.
 * Refusals: the others of ps_rtm_rank_all, with its messages; C >= 1 with a list; B * slots_per_pass < 2^30; a null timeline. */
typedef struct PsRtmSeqTimeline {   /* device pointers */
  const int64_t* ptr;    /* [P + 1] the items' ranges in rids / times: non-decreasing, ptr[0] = 0, ptr[P] = N */
  const int64_t* rids;   /* [N] review ids, per item in time order */
  const int64_t* times;  /* [N] non-decreasing within an item */
  int64_t n;             /* N >= 1 */
} PsRtmSeqTimeline;

/* `C` of the two host-only entries where there is no list: the columns are the P catalogue rows */
#define PS_RTM_SEQ_NO_LIST (-1)

/* bytes of scratch with `slots_per_pass` columns scored per pass (<= 0: the default, 32768 pairs); -1: refused / bad sizes.
 * ps_rtm_rank_seq sizes its passes from the scratch it is given: the most columns that fit. */
int64_t ps_rtm_rank_seq_scratch_bytes(const PsRtmDesc* desc, const PsRtmRankShape* shape, int64_t C, int32_t topk,
                                      int64_t slots_per_pass);
/* What ps_rtm_rank_seq launches, from the rules the launcher itself reads (csrc/rtm_rank.hip: rr_pass_layout, rr_epl, rr_lph,    
 * rr_tail_fused, rr_query_fs_fused).  Host only: no HIP call. */
typedef struct PsRtmRankSeqPlan {
  int64_t slots_per_pass;       /* columns scored per pass: the most whose pairs fit the scratch                         */
  int64_t passes;               /* ceil(columns / slots_per_pass); a ragged last pass runs at the full pass shape        */
  int32_t epl;                  /* d / 64: the instantiation of rr_entry_kernel / rr_slot_kernel                         */
  int32_t lph;                  /* 64 / H: lanes per head                                                                */
  int32_t tail_fused;           /* the per-pair tail is the fused d = 128 kernel                                         */
  int32_t query_fs_fused;       /* the fs query encoder's projection runs inside the embed launch                        */
} PsRtmRankSeqPlan;
int ps_rtm_rank_seq_plan(const PsRtmDesc* desc, const PsRtmRankShape* shape, int64_t C, int32_t topk, int64_t scratch_bytes,
                         PsRtmRankSeqPlan* out);
/* time_stamps [B] int64: the entries' stamps.  candi_prod_idxs [B, C] as ps_rtm_rank_candidates takes them, or NULL: C is then
 * ignored and the columns are the P = shape->n_items catalogue rows.  With a list the outputs are exactly
 * ps_rtm_rank_candidates' (item ids of the live slots by score desc, column asc; rank from the target's first live column;
 * scores_out [B, C], -inf at dead slots); without one they are ps_rtm_rank_all's (ties to the lower id, rank 0: the target is
 * not a product; scores_out [B, P]).  A slot's bits do not depend on the pass it lands in.  The timeline is trusted to be
 * sorted (ProductRanker.timeline_index checks it once); a ptr outside [0, N] is clamped, never followed.  scratch: 256-byte
 * aligned. */
int ps_rtm_rank_seq(const PsRtmDesc* desc, const PsRtmRankShape* shape, const PsRtmTensors* params, const float* index,
                    const PsRtmSeqTimeline* timeline, const int64_t* query_word_idxs, const int64_t* u_ridxs,
                    const int64_t* time_stamps, const int64_t* candi_prod_idxs, int64_t C, const int64_t* target_prod_idxs,
                    int32_t topk, int64_t* top_idx, float* top_score, int32_t* rank, float* scores_out, void* scratch,
                    int64_t scratch_bytes, ps_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PRODSEARCH_RTM_SEQ_H */
