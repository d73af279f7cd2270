// rank.h — the selection levels of rank.hip for callers inside the library that computed a dense score matrix themselves
// (rtm_rank.hip): top-k by (score desc, id asc) and the target's 1-based rank, the semantics of ps_rank_all.
#pragma once
#include "common.h"

// bytes of scratch for B rows of n_rows scores; -1: unsupported sizes (topk must be 1..256)
int64_t rank_select_scratch_bytes(int B, int64_t n_rows, int topk);
// S [B, ld] (ld >= n_rows): top_idx / top_score [B, topk] (unfilled slots -1 / -inf), rank [B] (optional, needs target;
// 0: the target is not a column).  scratch: 256-byte aligned.
int rank_select_scores(const float* S, int64_t ld, int B, int64_t n_rows, const int64_t* target, int topk, int64_t* top_idx,
                       float* top_score, int32_t* rank, void* scratch, int64_t scratch_bytes, hipStream_t st);
