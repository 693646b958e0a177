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

#define KSG_EXPLAIN_WAVES (KSG_EXPLAIN_TILE / 64)
static_assert(KSG_EXPLAIN_TILE % 64 == 0, "one bitmap word per wave");
static_assert((KSG_EXPLAIN_SLOTS & (KSG_EXPLAIN_SLOTS - 1)) == 0 && KSG_FAIL_SCALAR < KSG_EXPLAIN_SLOTS,
              "histogram slots: a power of two past the last fail code");

__global__ __launch_bounds__(KSG_EXPLAIN_TILE) void ksg_explain_kernel(KsgDev d, const ksg_pod* __restrict__ pods,
                                                                      const ksg_pod_ext* __restrict__ exts,
                                                                      const uint32_t* __restrict__ ids, uint32_t n_pods,
                                                                      uint8_t* __restrict__ codes,
                                                                      uint32_t* __restrict__ hist,
                                                                      uint8_t* __restrict__ err) {
  __shared__ uint32_t s_hist[KSG_EXPLAIN_CHUNK * KSG_EXPLAIN_SLOTS];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wi = blockIdx.x * KSG_EXPLAIN_WAVES + (tid >> 6);  // wave-uniform
  const uint32_t n = wi * 64 + lane;
  const uint64_t bit = 1ULL << lane;
  const bool valid = wi < d.nw && n < d.n_nodes;  // the last word's tail neither stores nor counts
  const uint32_t p0 = blockIdx.y * KSG_EXPLAIN_CHUNK;
  const uint32_t p1 = min(p0 + (uint32_t)KSG_EXPLAIN_CHUNK, n_pods);
  for (uint32_t i = tid; i < KSG_EXPLAIN_CHUNK * KSG_EXPLAIN_SLOTS; i += KSG_EXPLAIN_TILE) s_hist[i] = 0;
  int64_t capc = 0, capm = 0, usedc = 0, usedm = 0;
  if (valid) {
    capc = d.cap_cpu[n];
    capm = d.cap_mem[n];
    usedc = d.used_cpu[n];
    usedm = d.used_mem[n];
  }
  __syncthreads();
  if (wi < d.nw) {  // (a whole wave past the last word only joins the barriers)
    const uint64_t live = __ballot(valid);
    for (uint32_t p = p0; p < p1; ++p) {
      PodCtx c;
      pod_resolve<false>(d, pods[p], ids, c);
      if (exts) c.ext = exts + p;
      if (blockIdx.x == 0 && tid == 0) err[p] = c.error ? 1 : 0;
      if (c.error) {  // wave-uniform: the rows stay zero
        if (codes && valid) codes[(size_t)p * d.n_nodes + n] = 0;
        continue;
      }
      // (node_fail's extended-resource loads are indexed by n: only for a lane with a node)
      const int code = valid ? (node_fail<false>(d, c, n, wi, bit, capc, capm, usedc, usedm) & (KSG_EXPLAIN_SLOTS - 1)) : 0;
      if (codes && valid) codes[(size_t)p * d.n_nodes + n] = (uint8_t)code;
      uint64_t rem = live;
      while (rem) {  // one ballot per distinct code present
        const int cc = __builtin_amdgcn_readlane(code, (int)__builtin_ctzll(rem));
        const uint64_t m = __ballot(valid && code == cc);
        if (lane == 0) atomicAdd(&s_hist[(p - p0) * KSG_EXPLAIN_SLOTS + cc], (uint32_t)__popcll(m));
        rem &= ~m;
      }
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < (p1 - p0) * KSG_EXPLAIN_SLOTS; i += KSG_EXPLAIN_TILE)
    if (s_hist[i]) atomicAdd(hist + (size_t)p0 * KSG_EXPLAIN_SLOTS + i, s_hist[i]);
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
