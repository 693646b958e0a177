// ksg_explain.hip — FitError reports for many pods in one pass (ksg_explain_batch):
// the reference's FailedPredicateMap (generic_scheduler.go:30-44, 100-128) of every pod of a
// list against the cluster as it stands. Nothing is committed, scored or drawn.
//
// Node-stationary tiling: a workgroup owns KSG_EXPLAIN_TILE nodes, one 64-node bitmap
// word per wave (so the word index is wave-uniform, as node_fail_l expects), and a lane
// keeps its node's capacities and requested totals in registers while the workgroup walks
// a chunk of KSG_EXPLAIN_CHUNK pods: grid = node tiles x pod chunks, node state read once
// per (tile, chunk). Per pod every wave resolves the pod itself (pod_resolve<false>:
// wave-uniform loads of one pod record, the ServiceAffinity peer lookup and trap as the
// scan kernels apply them) and then runs node_fail<false> for its lane's node. All state
// is read-only for the kernel's lifetime: plain loads, no cross-block waits, and no
// atomics but the histogram adds.
//
// Outputs: (a) optionally codes[p * n_nodes + n], 64 contiguous bytes per wave;
// (b) hist[p][KSG_EXPLAIN_SLOTS], slot c = nodes whose code is c: per wave one
// ballot/popcount per distinct code present (usually one to three), summed per block in
// the LDS and flushed with one global atomic add per non-zero slot into a zeroed buffer;
// (c) err[p] = 1 for a pod whose ServiceAffinity peer sits on an unknown host
// (predicates.go:293-296): its codes and histogram row stay zero.
#include <hip/hip_runtime.h>

#include "ksg_device.h"
#include "ksg_launch.h"

__global__ __launch_bounds__(KSG_EXPLAIN_TILE) void ksg_explain_kernel(KsgDev d, const ksg_pod* __restrict__ pods,
                                                                      const ksg_pod_ext* __restrict__ exts,
                                                                      const uint32_t* __restrict__ ids, uint32_t n_pods,
                                                                      uint8_t* __restrict__ codes,
                                                                      uint32_t* __restrict__ hist,
                                                                      uint8_t* __restrict__ err) {
  ksg_explain_pass(d, KsgExplainPlain{}, pods, exts, ids, n_pods, codes, hist, err);
}

// codes: optional (nullptr: no per-node bytes); hist zeroed by the caller; grid.y covers n_pods
hipError_t ksg_launch_explain(const KsgDev& d, const ksg_pod* pods, const ksg_pod_ext* exts, const uint32_t* ids,
                              uint32_t n_pods, uint8_t* codes, uint32_t* hist, uint8_t* err, hipStream_t st) {
  if (n_pods == 0 || d.nw == 0) return hipSuccess;
  const dim3 grid((d.nw + KSG_EXPLAIN_WAVES - 1) / KSG_EXPLAIN_WAVES, (n_pods + KSG_EXPLAIN_CHUNK - 1) / KSG_EXPLAIN_CHUNK);
  hipLaunchKernelGGL(ksg_explain_kernel, grid, dim3(KSG_EXPLAIN_TILE), 0, st, d, pods, exts, ids, n_pods, codes, hist,
                     err);
  return hipGetLastError();
}
