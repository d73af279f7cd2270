// side_stream.h — the side stream and its crossings with the caller's ("main") stream; implemented in side_stream.hip.
//
// Work that is off the dependent chain of a backward (weight gradients, table scatters, index builds) runs on ONE
// low-priority side stream per device, beside the main stream.  The contract:
//   * fork (side_fork): everything enqueued on main_st so far is complete before anything enqueued on the side stream
//     afterwards starts.  Each fork costs the main stream a stream operation, so callers batch what they fork.
//   * join (side_join): everything enqueued on the side stream so far is complete before anything enqueued on main_st
//     afterwards starts.  A join without a fork since the last join does nothing.  An entry point joins before it returns.
//   * no side stream — deterministic mode, PS_NO_SIDE=1, a step being captured into a graph, a side stream the start-up
//     self-test could not release: side_stream_or returns main_st, forks and joins do nothing, and the work runs in
//     launch order on the main stream.
// One host thread drives a device's side stream at a time (include/prodsearch_hip.h, "Threading").
#pragma once
#include "common.h"

int side_fork(hipStream_t main_st);
int side_join(hipStream_t main_st);
hipStream_t side_stream_or(hipStream_t main_st);   // the side stream, or main_st when there is none
// short steps cross with stream write / wait-value operations, long ones with event pairs: chosen per backward, before its first fork
void side_set_light(bool light);
bool fork_by_kernel();                             // forks are signalled by the next main-stream kernel (below); PS_FORK_BY_KERNEL=0: by a stream write

// A value fork without a stream operation on the main stream: the side stream waits for a sequence value, and the NEXT
// kernel launched on the main stream stores it as its first workgroup starts (common.h, fork_signal) — every earlier
// main-stream kernel has completed by then (in-order stream), which is all a fork promises.  Who may take the pending
// signal: a launcher on that stream whose kernel calls fork_signal, right before a launch that no check can still stop;
// side_repend_signal hands it back when the launch did not happen after all.  An unclaimed signal is flushed with a stream
// write by the join.  The write-value operation this replaces cost the main stream ~5 us between two
// dependent kernels, twice per backward.
bool side_take_signal(hipStream_t st, uint32_t** flag, uint32_t* val);
void side_repend_signal(hipStream_t st, uint32_t val);

// Error paths: a failed entry point must not leave the side stream parked on a value nobody will store (a kernel-carried
// fork whose carrying launch never happened).  side_abort releases it, so that the caller's next synchronize returns and
// the error surfaces; every entry point that forks calls it when it fails.
void side_abort();
