// ksg_explain_without.hip — FitError reports with committed pods taken away
// (ksg_explain_without): ksg_explain.hip's pass, but pod p is explained against the state
// WITHOUT the pods absent[first_absent[p] .. n_absent) of an ordered list of committed pods.
// Nothing is removed: the host (ksg_without.cpp) describes the list in three read-only
// tables and the kernel corrects what a touched node's lane sees.
//
//   node deltas   touched[nw]: nodes that carry a listed pod. Per node a CSR row of its listed
//                 pods sorted by list index: nd_idx[e], and nd_sum[k][e] = the wrapping sum of
//                 resource k (cpu, memory, then the extended resources) over the row's entries
//                 e.. . The correction of pod p on the node is nd_sum[.][e] at the first entry
//                 with nd_idx[e] >= first_absent[p] (none: nothing on the node is taken away).
//   conflict bits per node a CSR row (cf_key ascending) of the conflict keys whose holders on
//                 that node are ALL listed, with cf_min = the smallest list index among them:
//                 the key's bit reads as clear for pod p iff first_absent[p] <= cf_min. A key
//                 with a holder outside the list has no entry (its bit stays).
//   peers         peer[p]: the pod's ServiceAffinity peer as of its position (-1 none, -2 a
//                 host outside the node list, else the node rank), instead of d.svc_peer.
//
// Nothing of the pass is restated here. The kernel is ksg_explain_pass (ksg_device.h) and the
// predicates are node_fail_l's; this file only supplies what is taken away, as the two views
// those templates ask for: KsgAbsent for the pass (the touched bit, the peer, the choice of
// the walk) and KsgAbsentAt (ksg_device.h) for node_fail_l (a touched node at a position: cleared conflict
// bits and corrected totals, so a cleared disk bit lets the port, resource and later checks
// report). A lane whose node is not touched, and every lane of a pod with first_absent ==
// n_absent, runs node_fail<false> as it is. The lookups are binary searches on the lane's own
// short rows; the divergence is confined to touched lanes.
#include <hip/hip_runtime.h>

#include "ksg_device.h"
#include "ksg_launch.h"

// ksg_explain_pass's view: the peer as of the pod's position instead of d.svc_peer (the
// spreading terms, which no predicate reads, stay 0), and the hooked walk for a touched lane
// of a pod that has anything taken away
struct KsgAbsent {
  const KsgWithout& w;
  __device__ __forceinline__ void resolve(const KsgDev& d, const ksg_pod* pods, const uint32_t* ids, uint32_t p,
                                          PodCtx& c) const {
    pod_fields(pods[p], ids, c);
    pod_affinity(d, pods[p], w.peer && c.svc >= 0 ? w.peer[p] : -1, c);
  }
  __device__ __forceinline__ bool touched(uint32_t wi, uint64_t bit) const { return (w.touched[wi] & bit) != 0; }
  __device__ __forceinline__ int fail(const KsgDev& d, const PodCtx& c, uint32_t p, bool touched, uint32_t n, uint32_t wi,
                                      uint64_t bit, int64_t capc, int64_t capm, int64_t usedc, int64_t usedm) const {
    const uint32_t fa = w.first_absent[p];  // wave-uniform
    if (!(touched && fa < w.n_absent)) return node_fail<false>(d, c, n, wi, bit, capc, capm, usedc, usedm);
    return node_fail_l<false>(d, c, PtrLists{c.ports, c.pds, c.sel}, n, wi, bit, capc, capm, usedc, usedm,
                              KsgAbsentAt{w, n, fa, w.cf_off[n], w.cf_off[n + 1]});
  }
};

__global__ __launch_bounds__(KSG_EXPLAIN_TILE) void ksg_explain_without_kernel(
    KsgDev d, KsgWithout w, const ksg_pod* __restrict__ pods, const ksg_pod_ext* __restrict__ exts,
    const uint32_t* __restrict__ ids, uint32_t n_pods, uint8_t* __restrict__ codes, uint32_t* __restrict__ hist,
    uint8_t* __restrict__ err) {
  ksg_explain_pass(d, KsgAbsent{w}, pods, exts, ids, n_pods, codes, hist, err);
}

// codes: optional (nullptr: no per-node bytes); hist zeroed by the caller; grid.y covers n_pods;
// w.first_absent and w.peer are indexed from `pods`
hipError_t ksg_launch_explain_without(const KsgDev& d, const KsgWithout& w, const ksg_pod* pods, const ksg_pod_ext* exts,
                                      const uint32_t* ids, uint32_t n_pods, uint8_t* codes, uint32_t* hist, uint8_t* err,
                                      hipStream_t st) {
  if (n_pods == 0 || d.nw == 0) return hipSuccess;
  const dim3 grid((d.nw + KSG_EXPLAIN_WAVES - 1) / KSG_EXPLAIN_WAVES, (n_pods + KSG_EXPLAIN_CHUNK - 1) / KSG_EXPLAIN_CHUNK);
  hipLaunchKernelGGL(ksg_explain_without_kernel, grid, dim3(KSG_EXPLAIN_TILE), 0, st, d, w, pods, exts, ids, n_pods, codes,
                     hist, err);
  return hipGetLastError();
}
