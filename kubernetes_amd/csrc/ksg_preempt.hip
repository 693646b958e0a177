// ksg_preempt.hip — victims per node and the node to preempt on (ksg_preempt_batch;
// include/kschedgpu.h has the definition). Pod p may evict the pods absent[first_absent[p] ..
// n_absent) of an ordered list of committed pods, most important first. Nothing is removed: the
// host (ksg_preempt.cpp) describes the list in ksg_explain_without's read-only tables (KsgWithout:
// the touched nodes, per node a CSR row of its listed pods with the wrapping suffix sums of their
// requests, the conflict keys only listed pods hold) plus the conflict keys of every row entry
// (KsgPreemptKeys).
//
// Pass 1 keeps ksg_explain_pass's tiling: a workgroup owns KSG_EXPLAIN_TILE nodes, one 64-node
// word per wave, a lane owns one node and walks a chunk of KSG_EXPLAIN_CHUNK pods. A lane whose
// node carries no listed pod, and every lane of a pod with first_absent == n_absent, runs
// node_fail<false>: a candidate without victims, or none. A touched lane runs node_fail_l with
// the KsgAbsentAt view (the node with every pod the pod may evict taken away); on 0 it walks its
// own row from the position on (preempt_walk) and puts the entries back one by one, most
// important first, while the pod still fits: of the predicates only NoDiskConflict,
// PodFitsPorts, PodFitsResources and the extended resources can change, so the walk keeps
// running totals of what it put back and tests an entry's keys against the pod's lists. An
// entry that cannot come back is a victim. The divergence is confined to touched lanes and the
// trip count is the longest row of the wave.
//
// A candidate's key is (top << 32) | ~victims, top = the smallest list index among its victims
// (n_absent: none); the best node has the largest key, then the highest rank. Each wave reduces
// (candidates, candidates without a victim, best key and node) with ballots and shuffles, lane 0
// stores them in the wave's own LDS slot, and after the chunk one thread per pod folds the
// workgroup's waves into a KsgPreemptPart per (pod, node tile): no float, no atomics.
//
// Pass 2, one wave per pod, folds the tile partials the same way, writes the pod's results and
// walks the best node's row once more (every lane the same walk, lane 0 stores) for the first
// max_victims victim indices.
#include <hip/hip_runtime.h>

#include "ksg_device.h"
#include "ksg_launch.h"

namespace {

// is `key` in the pod's GCE-PD or host-port list, under the predicates that are on
__device__ __forceinline__ bool pod_lists_key(const KsgDev& d, const PodCtx& c, uint32_t key) {
  if (d.preds & KSG_PRED_NODISKCONFLICT)
    for (uint32_t i = 0; i < c.n_pds; ++i)
      if (c.pds[i] == key) return true;
  if (d.preds & KSG_PRED_PODFITSPORTS)
    for (uint32_t i = 0; i < c.n_ports; ++i)
      if (c.ports[i] == key) return true;
  return false;
}

// The reprieve walk of pod c on touched node n, which it fits with the entries [e, e1) of the
// node's row taken away: the number of victims, in `top` the smallest list index among them
// (unchanged without one), and in out[0 .. min(victims, max_out)) their list indices in list
// order (out may be nullptr with max_out == 0). usedc / usedm are the node's committed totals
// as they stand; the tests are node_fail_l's, term for term (wrapping totals, cap == 0, the
// zero-request pod, an extended resource only where the pod requests it).
__device__ __forceinline__ uint32_t preempt_walk(const KsgDev& d, const KsgWithout& w, const KsgPreemptKeys& ek,
                                                 const PodCtx& c, uint32_t n, uint32_t e, uint32_t e1, int64_t capc,
                                                 int64_t capm, int64_t usedc, int64_t usedm, uint32_t& top,
                                                 uint32_t* out, uint32_t max_out) {
  const size_t E = w.nd_n;
  const bool res = (d.preds & KSG_PRED_PODFITSRESOURCES) && !c.zero_req;
  const bool sca = (d.ext_filters & KSG_EXT_SCALAR) && c.ext;
  const bool keys = ((d.preds & KSG_PRED_NODISKCONFLICT) && c.n_pds) || ((d.preds & KSG_PRED_PODFITSPORTS) && c.n_ports);
  // the totals with the whole suffix away, plus what has been put back (wrapping)
  uint64_t tc = (uint64_t)usedc - w.nd_sum[e], tm = (uint64_t)usedm - w.nd_sum[E + e];
  uint64_t ts[KSG_MAX_SCALAR], cs[KSG_MAX_SCALAR];
#pragma unroll
  for (uint32_t r = 0; r < KSG_MAX_SCALAR; ++r) {
    ts[r] = cs[r] = 0;
    if (sca && r < d.n_scalar && c.ext->scalar[r] > 0) {
      cs[r] = w.nd_sum[(2 + r) * E + e];
      ts[r] = (uint64_t)d.scalar_used[(size_t)r * d.n_nodes + n] - cs[r];
    }
  }
  uint64_t cc = w.nd_sum[e], cm = w.nd_sum[E + e];  // the suffix sums at the current entry
  uint32_t victims = 0;
  for (uint32_t j = e; j < e1; ++j) {
    const bool more = j + 1 < e1;
    // the entry's own requests: its suffix sum less the next entry's (the last: its own)
    const uint64_t nc = more ? w.nd_sum[j + 1] : 0, nm = more ? w.nd_sum[E + j + 1] : 0;
    const uint64_t qc = cc - nc, qm = cm - nm;
    cc = nc;
    cm = nm;
    bool ok = true;
    if (keys) {
      const uint32_t k1 = ek.ek_off[j + 1];
      for (uint32_t k = ek.ek_off[j]; k < k1 && ok; ++k) ok = !pod_lists_key(d, c, ek.ek_key[k]);
    }
    if (res) {
      const uint64_t uc = tc + qc, um = tm + qm;
      const bool fc = capc == 0 || (int64_t)((uint64_t)capc - uc) >= c.req_cpu;
      const bool fm = capm == 0 || (int64_t)((uint64_t)capm - um) >= c.req_mem;
      ok = ok && fc && fm;
    }
    uint64_t qs[KSG_MAX_SCALAR];
#pragma unroll
    for (uint32_t r = 0; r < KSG_MAX_SCALAR; ++r) {
      qs[r] = 0;
      if (sca && r < d.n_scalar && c.ext->scalar[r] > 0) {
        const uint64_t ns = more ? w.nd_sum[(2 + r) * E + j + 1] : 0;
        qs[r] = cs[r] - ns;
        cs[r] = ns;
        const int64_t cap = d.scalar_cap[(size_t)r * d.n_nodes + n];
        if (cap < (int64_t)(ts[r] + qs[r] + (uint64_t)c.ext->scalar[r])) ok = false;
      }
    }
    if (ok) {  // reprieved: it stays on the node for the entries after it
      tc += qc;
      tm += qm;
#pragma unroll
      for (uint32_t r = 0; r < KSG_MAX_SCALAR; ++r) ts[r] += qs[r];
    } else {
      const uint32_t idx = w.nd_idx[j];
      if (victims == 0) top = idx;  // (a row's indices ascend)
      if (victims < max_out) out[victims] = idx;
      ++victims;
    }
  }
  return victims;
}

// `a` beats `b`: the larger key, then the higher node (node1 == 0: no candidate, key 0)
__device__ __forceinline__ bool part_beats(uint64_t ka, uint32_t na, uint64_t kb, uint32_t nb) {
  return ka > kb || (ka == kb && na > nb);
}

// the best (key, node1) of the wave's lanes, in every lane
__device__ __forceinline__ void wave_best(uint64_t& key, uint32_t& node1) {
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) {
    const uint64_t ko = ((uint64_t)__shfl_xor((uint32_t)(key >> 32), sh) << 32) | __shfl_xor((uint32_t)key, sh);
    const uint32_t no = __shfl_xor(node1, sh);
    if (part_beats(ko, no, key, node1)) key = ko, node1 = no;
  }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int sh = 32; sh >= 1; sh >>= 1) v += __shfl_xor(v, sh);
  return v;
}

// a pod's context for this query: no ServiceAffinity predicate (the host refuses the context),
// so no peer and no error
__device__ __forceinline__ void preempt_pod(const KsgDev& d, const ksg_pod* pods, const ksg_pod_ext* exts,
                                            const uint32_t* ids, uint32_t p, PodCtx& c) {
  pod_fields(pods[p], ids, c);
  pod_affinity(d, pods[p], -1, c);
  if (exts) c.ext = exts + p;
}

}  // namespace

__global__ __launch_bounds__(KSG_EXPLAIN_TILE) void ksg_preempt_pass_kernel(
    KsgDev d, KsgWithout w, KsgPreemptKeys ek, const ksg_pod* __restrict__ pods, const ksg_pod_ext* __restrict__ exts,
    const uint32_t* __restrict__ ids, uint32_t n_pods, uint32_t* __restrict__ node_victims,
    KsgPreemptPart* __restrict__ part) {
  __shared__ uint64_t s_key[KSG_EXPLAIN_CHUNK][KSG_EXPLAIN_WAVES];
  __shared__ uint32_t s_node[KSG_EXPLAIN_CHUNK][KSG_EXPLAIN_WAVES];
  __shared__ uint32_t s_cand[KSG_EXPLAIN_CHUNK][KSG_EXPLAIN_WAVES];
  __shared__ uint32_t s_free[KSG_EXPLAIN_CHUNK][KSG_EXPLAIN_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t wi = blockIdx.x * KSG_EXPLAIN_WAVES + wv;  // wave-uniform
  const uint32_t n = wi * 64 + lane;
  const uint64_t bit = 1ULL << lane;
  const bool valid = wi < d.nw && n < d.n_nodes;  // the last word's tail neither stores nor counts
  const uint32_t p0 = blockIdx.y * KSG_EXPLAIN_CHUNK;
  const uint32_t p1 = min(p0 + (uint32_t)KSG_EXPLAIN_CHUNK, n_pods);
  for (uint32_t i = tid; i < KSG_EXPLAIN_CHUNK * KSG_EXPLAIN_WAVES; i += KSG_EXPLAIN_TILE) {
    (&s_key[0][0])[i] = 0;  // (a whole wave past the last word leaves its slots at "no candidate")
    (&s_node[0][0])[i] = 0;
    (&s_cand[0][0])[i] = 0;
    (&s_free[0][0])[i] = 0;
  }
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
  if (wi < d.nw) {
    const uint64_t free_key = ((uint64_t)w.n_absent << 32) | 0xffffffffu;  // no victim
    for (uint32_t p = p0; p < p1; ++p) {
      PodCtx c;
      preempt_pod(d, pods, exts, ids, p, c);
      const uint32_t fa = w.first_absent[p];  // wave-uniform
      uint32_t nv = KSG_PREEMPT_NOFIT, top = w.n_absent;
      if (valid) {
        if (!(touched && fa < w.n_absent)) {
          if (node_fail<false>(d, c, n, wi, bit, capc, capm, usedc, usedm) == KSG_FAIL_NONE) nv = 0;
        } else {
          const KsgAbsentAt at{w, n, fa, w.cf_off[n], w.cf_off[n + 1]};
          if (node_fail_l<false>(d, c, PtrLists{c.ports, c.pds, c.sel}, n, wi, bit, capc, capm, usedc, usedm, at) ==
              KSG_FAIL_NONE) {
            at.seek();
            nv = at.e < at.e1 ? preempt_walk(d, w, ek, c, n, at.e, at.e1, capc, capm, usedc, usedm, top, nullptr, 0) : 0;
          }
        }
        if (node_victims) node_victims[(size_t)p * d.n_nodes + n] = nv;
      }
      const uint64_t m_free = __ballot(valid && nv == 0);
      const uint64_t m_cand = __ballot(valid && nv != KSG_PREEMPT_NOFIT);
      uint64_t key = 0;
      uint32_t node1 = 0;
      if (m_free) {  // a node that needs no eviction beats every node that does: the highest such lane
        key = free_key;
        node1 = wi * 64 + (63 - (uint32_t)__builtin_clzll(m_free)) + 1;
      } else if (m_cand) {
        if (valid && nv != KSG_PREEMPT_NOFIT) key = ((uint64_t)top << 32) | (uint32_t)~nv, node1 = n + 1;
        wave_best(key, node1);
      }
      if (lane == 0) {
        s_key[p - p0][wv] = key;
        s_node[p - p0][wv] = node1;
        s_cand[p - p0][wv] = (uint32_t)__popcll(m_cand);
        s_free[p - p0][wv] = (uint32_t)__popcll(m_free);
      }
    }
  }
  __syncthreads();
  if (tid < p1 - p0) {
    KsgPreemptPart r{0, 0, 0, 0, 0};
#pragma unroll
    for (uint32_t v = 0; v < KSG_EXPLAIN_WAVES; ++v) {
      if (part_beats(s_key[tid][v], s_node[tid][v], r.key, r.node1)) r.key = s_key[tid][v], r.node1 = s_node[tid][v];
      r.cand += s_cand[tid][v];
      r.free_ += s_free[tid][v];
    }
    part[(size_t)(p0 + tid) * gridDim.x + blockIdx.x] = r;
  }
}

// one wave per pod (blockIdx.x): fold the pod's n_tiles partials, write its results, and walk
// the best node's row again for the first max_victims victim indices (the rest: 0xffffffff)
__global__ __launch_bounds__(64) void ksg_preempt_pick_kernel(
    KsgDev d, KsgWithout w, KsgPreemptKeys ek, const ksg_pod* __restrict__ pods, const ksg_pod_ext* __restrict__ exts,
    const uint32_t* __restrict__ ids, const KsgPreemptPart* __restrict__ part, uint32_t n_tiles, uint32_t max_victims,
    int32_t* __restrict__ best_node, uint32_t* __restrict__ n_victims, uint32_t* __restrict__ victims,
    uint32_t* __restrict__ cand_count, uint32_t* __restrict__ free_count) {
  const uint32_t p = blockIdx.x, lane = threadIdx.x;
  uint64_t key = 0;
  uint32_t node1 = 0, cand = 0, fre = 0;
  for (uint32_t t = lane; t < n_tiles; t += 64) {
    const KsgPreemptPart r = part[(size_t)p * n_tiles + t];
    if (part_beats(r.key, r.node1, key, node1)) key = r.key, node1 = r.node1;
    cand += r.cand;
    fre += r.free_;
  }
  wave_best(key, node1);
  cand = wave_sum(cand);
  fre = wave_sum(fre);
  const uint32_t nv = node1 ? ~(uint32_t)key : 0;
  if (lane == 0) {
    best_node[p] = (int32_t)node1 - 1;
    n_victims[p] = nv;
    cand_count[p] = cand;
    free_count[p] = fre;
  }
  if (max_victims == 0) return;
  uint32_t* const out = victims + (size_t)p * max_victims;
  uint32_t wrote = 0;
  if (nv) {  // (wave-uniform: a touched node at a position below n_absent, which the pod fits)
    PodCtx c;
    preempt_pod(d, pods, exts, ids, p, c);
    const uint32_t n = node1 - 1, fa = w.first_absent[p];
    const uint32_t e1 = w.nd_off[n + 1], e = lower_bound_u32(w.nd_idx, w.nd_off[n], e1, fa);
    uint32_t top = 0;
    // every lane walks alike; only lane 0 is given somewhere to store
    preempt_walk(d, w, ek, c, n, e, e1, d.cap_cpu[n], d.cap_mem[n], d.used_cpu[n], d.used_mem[n], top, out,
                 lane == 0 ? max_victims : 0);
    wrote = min(nv, max_victims);
  }
  for (uint32_t i = wrote + lane; i < max_victims; i += 64) out[i] = 0xffffffffu;
}

uint32_t ksg_preempt_tiles(const KsgDev& d) { return (d.nw + KSG_EXPLAIN_WAVES - 1) / KSG_EXPLAIN_WAVES; }

// node_victims: optional, uint32[n_pods][n_nodes]; part: KsgPreemptPart[n_pods][ksg_preempt_tiles(d)];
// victims: uint32[n_pods][max_victims] (unread when max_victims == 0); every per-pod array,
// w.first_absent included, is indexed from `pods`
hipError_t ksg_launch_preempt(const KsgDev& d, const KsgWithout& w, const KsgPreemptKeys& ek, const ksg_pod* pods,
                              const ksg_pod_ext* exts, const uint32_t* ids, uint32_t n_pods, uint32_t max_victims,
                              uint32_t* node_victims, KsgPreemptPart* part, int32_t* best_node, uint32_t* n_victims,
                              uint32_t* victims, uint32_t* cand_count, uint32_t* free_count, hipStream_t st) {
  if (n_pods == 0 || d.nw == 0) return hipSuccess;
  const uint32_t T = ksg_preempt_tiles(d);
  const dim3 grid(T, (n_pods + KSG_EXPLAIN_CHUNK - 1) / KSG_EXPLAIN_CHUNK);
  hipLaunchKernelGGL(ksg_preempt_pass_kernel, grid, dim3(KSG_EXPLAIN_TILE), 0, st, d, w, ek, pods, exts, ids, n_pods,
                     node_victims, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(ksg_preempt_pick_kernel, dim3(n_pods), dim3(64), 0, st, d, w, ek, pods, exts, ids, part, T, max_victims,
                     best_node, n_victims, victims, cand_count, free_count);
  return hipGetLastError();
}
