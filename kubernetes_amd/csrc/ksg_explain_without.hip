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
// The tiling, the histogram and the stores are ksg_explain_kernel's. A lane whose node is not
// touched, and every lane of a pod with first_absent == n_absent, runs node_fail<false> as it
// is; a touched lane runs node_fail_without, the same predicates in the same fixed order, so a
// cleared disk bit lets the port, resource and later checks report. The lookups are binary
// searches on the lane's own short rows; the divergence is confined to touched lanes.
#include <hip/hip_runtime.h>

#include "ksg_device.h"
#include "ksg_launch.h"

#define KSG_EXPLAIN_WAVES (KSG_EXPLAIN_TILE / 64)
static_assert(KSG_EXPLAIN_TILE % 64 == 0, "one bitmap word per wave");
static_assert((KSG_EXPLAIN_SLOTS & (KSG_EXPLAIN_SLOTS - 1)) == 0 && KSG_FAIL_SCALAR < KSG_EXPLAIN_SLOTS,
              "histogram slots: a power of two past the last fail code");

// pod_resolve<false> with the ServiceAffinity peer given by the caller (the peer as of the
// pod's position) instead of d.svc_peer; the spreading terms, which no predicate reads, stay 0
__device__ __forceinline__ void pod_resolve_peer(const KsgDev& d, const ksg_pod& p, const uint32_t* ids, int32_t peer,
                                                 PodCtx& c) {
  c.req_cpu = p.milli_cpu;
  c.req_mem = p.memory;
  c.zero_req = (p.milli_cpu == 0 && p.memory == 0);  // predicates.go:129-132
  c.host = p.host;
  c.svc = p.service;
  c.ports = ids + p.ports_off;
  c.n_ports = p.n_ports;
  c.pds = ids + p.pds_off;
  c.n_pds = p.n_pds;
  c.sel = ids + p.sel_off;
  c.n_sel = p.n_sel;
  c.error = 0;
  c.spread_max = 0;
  c.svc_total = 0;
  c.ext = nullptr;
  c.ids = ids;
  if (c.svc < 0) peer = -1;
#pragma unroll
  for (uint32_t j = 0; j < KSG_MAX_AFF; ++j) c.req_aff[j] = -1;
  if (d.preds & KSG_PRED_SERVICEAFFINITY) {  // predicates.go:257-324, as pod_resolve applies it
    bool all_given = true;
#pragma unroll
    for (uint32_t j = 0; j < KSG_MAX_AFF; ++j) {
      if (j < d.n_aff) {
        c.req_aff[j] = p.aff_pair[j];
        if (p.aff_pair[j] == -1) all_given = false;
      }
    }
    if (!all_given && peer != -1) {
      if (peer == -2) {
        c.error = 1;
      } else {
#pragma unroll
        for (uint32_t j = 0; j < KSG_MAX_AFF; ++j)
          if (j < d.n_aff && c.req_aff[j] == -1) c.req_aff[j] = d.aff_pair[(size_t)j * d.n_nodes + peer];
      }
    }
    aff_apply_trap(d, c.req_aff);
  }
}

// first position in [lo, hi) of the ascending array a whose value is >= v (hi: none)
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* __restrict__ a, uint32_t lo, uint32_t hi, uint32_t v) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// does conflict key `key`, set in the keymap for node n, read as clear at position fa
__device__ __forceinline__ bool key_cleared(const KsgWithout& w, uint32_t c0, uint32_t c1, uint32_t key, uint32_t fa) {
  const uint32_t e = lower_bound_u32(w.cf_key, c0, c1, key);
  return e < c1 && w.cf_key[e] == key && fa <= w.cf_min[e];
}

// node_fail_l for a touched node at position fa: the same predicates in the same order, with
// the pod's disk and port bits masked by the conflict table and the requested totals
// corrected by the node's suffix sums
__device__ __forceinline__ int node_fail_without(const KsgDev& d, const PodCtx& c, const KsgWithout& w, uint32_t fa,
                                                 uint32_t n, uint32_t wi, uint64_t bit, int64_t capc, int64_t capm,
                                                 int64_t usedc, int64_t usedm) {
  const uint32_t P = d.preds;
  if ((P & KSG_PRED_HOSTNAME) && c.host != -1 && (int32_t)n != c.host) return KSG_FAIL_HOSTNAME;
  if (d.has_static_fit && !(d.static_fit[wi] & bit)) return KSG_FAIL_LABELSPRESENCE;
  if (P & KSG_PRED_MATCHNODESELECTOR) {
    for (uint32_t i = 0; i < c.n_sel; ++i)
      if (!(d.pairmap[(size_t)c.sel[i] * d.nw + wi] & bit)) return KSG_FAIL_MATCHNODESELECTOR;
  }
  const uint32_t c0 = w.cf_off[n], c1 = w.cf_off[n + 1];
  if (P & KSG_PRED_NODISKCONFLICT) {
    for (uint32_t i = 0; i < c.n_pds; ++i)
      if ((d.keymap[(size_t)c.pds[i] * d.nw + wi] & bit) && !key_cleared(w, c0, c1, c.pds[i], fa))
        return KSG_FAIL_NODISKCONFLICT;
  }
  if (P & KSG_PRED_PODFITSPORTS) {
    for (uint32_t i = 0; i < c.n_ports; ++i)
      if ((d.keymap[(size_t)c.ports[i] * d.nw + wi] & bit) && !key_cleared(w, c0, c1, c.ports[i], fa))
        return KSG_FAIL_PODFITSPORTS;
  }
  // the node's listed pods at or past the position: entries e.. of its row (e == e1: none)
  const uint32_t e1 = w.nd_off[n + 1];
  const uint32_t e = lower_bound_u32(w.nd_idx, w.nd_off[n], e1, fa);
  if ((P & KSG_PRED_PODFITSRESOURCES) && !c.zero_req) {
    if (e < e1) {  // remove_pod_impl's wrapping subtraction, all of the suffix at once
      usedc = (int64_t)((uint64_t)usedc - w.nd_sum[e]);
      usedm = (int64_t)((uint64_t)usedm - w.nd_sum[(size_t)w.nd_n + e]);
    }
    const bool fc = capc == 0 || (int64_t)((uint64_t)capc - (uint64_t)usedc) >= c.req_cpu;
    const bool fm = capm == 0 || (int64_t)((uint64_t)capm - (uint64_t)usedm) >= c.req_mem;
    if (!(fc && fm)) return KSG_FAIL_PODFITSRESOURCES;
  }
  if (P & KSG_PRED_SERVICEAFFINITY) {
#pragma unroll
    for (uint32_t j = 0; j < KSG_MAX_AFF; ++j)
      if (j < d.n_aff && c.req_aff[j] >= 0 && !(d.pairmap[(size_t)c.req_aff[j] * d.nw + wi] & bit))
        return KSG_FAIL_SERVICEAFFINITY;
  }
  if (d.ext_filters && c.ext) {
    if (d.ext_filters & KSG_EXT_TAINTS)
      for (uint32_t i = 0; i < c.ext->n_hard; ++i)
        if (d.taintmap[(size_t)c.ids[c.ext->hard_off + i] * d.nw + wi] & bit) return KSG_FAIL_TAINTS;
    if (d.ext_filters & KSG_EXT_SCALAR)
      for (uint32_t r = 0; r < d.n_scalar; ++r) {
        const int64_t req = c.ext->scalar[r];
        if (req > 0) {
          const int64_t cap = d.scalar_cap[(size_t)r * d.n_nodes + n];
          uint64_t used = (uint64_t)d.scalar_used[(size_t)r * d.n_nodes + n];
          if (e < e1) used -= w.nd_sum[(size_t)(2 + r) * w.nd_n + e];
          if (cap < (int64_t)(used + (uint64_t)req)) return KSG_FAIL_SCALAR;
        }
      }
  }
  return KSG_FAIL_NONE;
}

__global__ __launch_bounds__(KSG_EXPLAIN_TILE) void ksg_explain_without_kernel(
    KsgDev d, KsgWithout w, const ksg_pod* __restrict__ pods, const ksg_pod_ext* __restrict__ exts,
    const uint32_t* __restrict__ ids, uint32_t n_pods, uint8_t* __restrict__ codes, uint32_t* __restrict__ hist,
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
  bool touched = false;
  if (valid) {
    capc = d.cap_cpu[n];
    capm = d.cap_mem[n];
    usedc = d.used_cpu[n];
    usedm = d.used_mem[n];
    touched = (w.touched[wi] & bit) != 0;
  }
  __syncthreads();
  if (wi < d.nw) {  // (a whole wave past the last word only joins the barriers)
    const uint64_t live = __ballot(valid);
    for (uint32_t p = p0; p < p1; ++p) {
      PodCtx c;
      pod_resolve_peer(d, pods[p], ids, w.peer ? w.peer[p] : -1, c);
      if (exts) c.ext = exts + p;
      if (blockIdx.x == 0 && tid == 0) err[p] = c.error ? 1 : 0;
      if (c.error) {  // wave-uniform: the rows stay zero
        if (codes && valid) codes[(size_t)p * d.n_nodes + n] = 0;
        continue;
      }
      const uint32_t fa = w.first_absent[p];  // wave-uniform
      int code = 0;
      if (valid) {
        if (touched && fa < w.n_absent) code = node_fail_without(d, c, w, fa, n, wi, bit, capc, capm, usedc, usedm);
        else code = node_fail<false>(d, c, n, wi, bit, capc, capm, usedc, usedm);
        code &= KSG_EXPLAIN_SLOTS - 1;
      }
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
