// wgrad.h — GEMM problem helpers and the weight-gradient launches of the backward passes; implemented in wgrad.hip.
#pragma once
#include "common.h"

GemmProblem gp(const float* A, int lda, int ta, const float* Bm, int ldb, int tb, float* C, int ldc, int M, int N, int K);
int run1(const GemmProblem& p, hipStream_t st);
GemmProblem gp_wgrad(const float* dY, int lddy, const float* X, int ldx, float* dW, int n_out, int k_in, int rows);
// one launch for a group of weight gradients (at most four) on `st`: picks the split counts and the kernel form (deterministic mode:
// per-split partials and an ordered sum)
int run_wgrads(GemmProblem* ps, int n, hipStream_t st);
// the same launch on the side stream behind its last fork (side_stream.h); on main_st where there is no side stream
int side_run(GemmProblem* ps, int n, hipStream_t main_st);
int side_wgrads(GemmProblem* ps, int n, hipStream_t main_st);   // side_fork + side_run
