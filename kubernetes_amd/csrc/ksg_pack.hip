// ksg_pack.hip — first-fit pod sets (ksg_pack_batch; include/kschedgpu.h has the definition).
// Set s owns the pods set_off[s] .. set_off[s + 1) of the call. Each of them, in order, goes to
// the highest-rank node it fits on the committed state plus the set's own earlier pods; nothing
// is written to the node state, and no set sees another.
//
// One workgroup of KSG_PACK_STRIP threads per set: the pods of a set are a true dependence
// chain, the grid's parallelism is across sets. For a pod the workgroup scans the nodes from the
// highest rank down in strips of KSG_PACK_WAVES 64-node bitmap words, one word per wave (so the
// word index is wave-uniform, as node_fail_l expects) and one node per lane. Strip k holds the
// words nw - 1 - k * KSG_PACK_WAVES - wave, wave 0 the highest; the first strip therefore holds
// the last, possibly partial, word and between KSG_PACK_STRIP - 63 and KSG_PACK_STRIP nodes.
// Each wave ballots its fitting lanes into its own LDS slot (two banks of slots, alternating, so
// one barrier per strip is enough); after the barrier every thread reads the slots and takes the
// highest set lane of the highest wave, or goes on to the next strip. Most pods end in the first
// strip, whose capacities and committed totals a lane keeps in registers for the whole set; a
// pod that fits nowhere costs the full scan. The excluded node and the nodes whose target bit
// is clear are lanes that never fit.
//
// The set's own placements live in the LDS, as the chains of the set's pods on each node:
//   - s_hnode / s_hhead: an open-addressed table of the nodes the set has touched and, per
//     node, the last pod of the set placed there. In place of the bitmap of touched nodes the
//     issue sketched: a set touches at most KSG_PACK_MAX_SET nodes whatever the cluster's size,
//     so 2 * KSG_PACK_MAX_SET slots (12 KiB) serve every node count with no capacity refusal
//     and no device scratch, where a bitmap costs n_nodes / 8 bytes per workgroup. A miss is the
//     first probe for almost every node, and a set that has placed nothing probes nothing: an
//     untouched lane runs the plain node_fail walk.
//   - s_cum[2][pod]: the wrapping sums of cpu and memory over the chain up to and including the
//     pod. A touched lane's view (KsgPackAt, in the style of KsgAbsentAt) adds the head's sums
//     to the node's committed totals: O(1) whatever the chain's length.
//   - s_klast / s_kprev: the chain thinned to the pods that hold a conflict key or request an
//     extended resource. Only a pod that lists keys under a predicate that is on, or requests an
//     extended resource under KSG_EXT_SCALAR, walks it: the entry's ports and PDs are tested
//     against the pod's lists in the one conflict-key id space (pod_lists_key, as
//     ksg_preempt.hip's), its extended-resource requests join the view's sums. Only fit / no fit
//     is needed, so the key test runs before node_fail_l.
// One thread records a placement, between two barriers.
//
// Known limits: one set is one workgroup's serial work (KSG_PACK_MAX_SET pods at most). And the
// thinned chain is walked whole, by every touched lane of its node, for every later pod that lists
// keys or requests an extended resource, reading pods[], ids[] and exts[] from global memory: a
// set of m key-holding pods piled onto a few nodes costs O(m^2) such reads inside its workgroup.
// tools/pack_bench.py's serial case (config-2 pods, few of them with ports) does not isolate
// this; it is unmeasured. The grid's x extent bounds the sets of a call (the host checks).
#include <hip/hip_runtime.h>

#include "ksg_device.h"
#include "ksg_launch.h"

#define KSG_PACK_WAVES (KSG_PACK_STRIP / 64)
#define KSG_PACK_SLOTS (2 * KSG_PACK_MAX_SET)
#define KSG_PACK_SLOT_BITS 11
#define KSG_PACK_NONE 0xffffu
static_assert(KSG_PACK_STRIP % 64 == 0, "one bitmap word per wave");
static_assert(KSG_PACK_SLOTS == 1 << KSG_PACK_SLOT_BITS, "the table's hash takes the product's top bits");
static_assert(KSG_PACK_MAX_SET < KSG_PACK_NONE, "a pod's index in its set fits uint16");

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

// node_fail_l's view of a node the set has touched: nothing is taken away, the requests of the
// set's earlier pods on the node are added (ksg_add_pod's wrapping sums)
struct KsgPackAt {
  uint64_t cpu, mem, sc[KSG_MAX_SCALAR];
  __device__ __forceinline__ bool key_cleared(uint32_t) const { return false; }
  __device__ __forceinline__ int64_t used(uint32_t k, int64_t v) const {
    uint64_t a = k == 0 ? cpu : mem;
#pragma unroll
    for (uint32_t r = 0; r < KSG_MAX_SCALAR; ++r) a = k == 2 + r ? sc[r] : a;  // (selects: sc stays in registers)
    return (int64_t)((uint64_t)v + a);
  }
};

__device__ __forceinline__ uint32_t pack_hash(uint32_t n) { return (n * 0x9E3779B1u) >> (32 - KSG_PACK_SLOT_BITS); }

}  // namespace

__global__ __launch_bounds__(KSG_PACK_STRIP) void ksg_pack_kernel(KsgDev d, KsgPack k, const ksg_pod* __restrict__ pods,
                                                                   const ksg_pod_ext* __restrict__ exts,
                                                                   const uint32_t* __restrict__ ids,
                                                                   int32_t* __restrict__ out_nodes,
                                                                   uint32_t* __restrict__ placed) {
  __shared__ uint32_t s_hnode[KSG_PACK_SLOTS];  // a touched node's rank (KSG_PACK_NO_NODE: free slot)
  __shared__ uint16_t s_hhead[KSG_PACK_SLOTS];  // ... the last pod of the set placed on it
  __shared__ uint64_t s_cum[2][KSG_PACK_MAX_SET];
  __shared__ uint16_t s_klast[KSG_PACK_MAX_SET];  // the last chain entry at or before the pod that holds keys
  __shared__ uint16_t s_kprev[KSG_PACK_MAX_SET];  // ... or extended resources, and the one before that
  __shared__ uint64_t s_bal[2][KSG_PACK_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint64_t bit = 1ULL << lane;
  const uint32_t set = blockIdx.x;
  const uint32_t base = k.set_off[set], m = k.set_off[set + 1] - base;
  const uint32_t excl = k.exclude ? k.exclude[set] : KSG_PACK_NO_NODE;
  for (uint32_t i = tid; i < KSG_PACK_SLOTS; i += KSG_PACK_STRIP) s_hnode[i] = KSG_PACK_NO_NODE;
  const uint32_t n_strips = (d.nw + KSG_PACK_WAVES - 1) / KSG_PACK_WAVES;
  // the lane's node of strip `s` may take pods at all: a node of the list that is neither the
  // excluded one nor masked out (wi wraps past 2^31 for a wave below word 0)
  const auto open = [&](uint32_t wi, uint32_t n) {
    return wi < d.nw && n < d.n_nodes && n != excl && (!k.targets || (k.targets[wi] & bit));
  };
  // the first strip's node state stays in registers
  const uint32_t wi0 = d.nw - 1 - wv, n0 = wi0 * 64 + lane;
  const bool open0 = open(wi0, n0);
  int64_t capc0 = 0, capm0 = 0, usedc0 = 0, usedm0 = 0;
  if (open0) {
    capc0 = d.cap_cpu[n0];
    capm0 = d.cap_mem[n0];
    usedc0 = d.used_cpu[n0];
    usedm0 = d.used_mem[n0];
  }
  __syncthreads();
  const bool sca_on = (d.ext_filters & KSG_EXT_SCALAR) && exts;
  uint32_t it = 0, n_placed = 0;
  for (uint32_t j = 0; j < m; ++j) {
    const uint32_t p = base + j;
    PodCtx c;  // (no ServiceAffinity predicate: the host refuses the context; so no peer and no error)
    pod_fields(pods[p], ids, c);
    pod_affinity(d, pods[p], -1, c);
    if (exts) c.ext = exts + p;
    // does this pod have to look at the chain's keys and extended resources (wave-uniform)
    bool walk = ((d.preds & KSG_PRED_NODISKCONFLICT) && c.n_pds) || ((d.preds & KSG_PRED_PODFITSPORTS) && c.n_ports);
    const bool keys = walk;
    bool sca = false;
    if (sca_on)
      for (uint32_t r = 0; r < d.n_scalar; ++r) sca = sca || c.ext->scalar[r] > 0;
    walk = walk || sca;
    int32_t found = -1;
    for (uint32_t s = 0; s < n_strips && found < 0; ++s) {
      const uint32_t wi = d.nw - 1 - s * KSG_PACK_WAVES - wv;  // wave-uniform
      const uint32_t n = wi * 64 + lane;
      const bool ok = s == 0 ? open0 : open(wi, n);
      bool fit = false;
      if (ok) {
        int64_t capc = capc0, capm = capm0, usedc = usedc0, usedm = usedm0;
        if (s) {
          capc = d.cap_cpu[n];
          capm = d.cap_mem[n];
          usedc = d.used_cpu[n];
          usedm = d.used_mem[n];
        }
        uint32_t head = KSG_PACK_NONE;
        if (n_placed)
          for (uint32_t h = pack_hash(n); s_hnode[h] != KSG_PACK_NO_NODE; h = (h + 1) & (KSG_PACK_SLOTS - 1))
            if (s_hnode[h] == n) {
              head = s_hhead[h];
              break;
            }
        if (head == KSG_PACK_NONE) {
          fit = node_fail<false>(d, c, n, wi, bit, capc, capm, usedc, usedm) == KSG_FAIL_NONE;
        } else {
          KsgPackAt at;
          at.cpu = s_cum[0][head];
          at.mem = s_cum[1][head];
#pragma unroll
          for (uint32_t r = 0; r < KSG_MAX_SCALAR; ++r) at.sc[r] = 0;
          bool clash = false;
          if (walk)
            for (uint32_t q = s_klast[head]; q != KSG_PACK_NONE && !clash; q = s_kprev[q]) {
              const ksg_pod& e = pods[base + q];
              if (keys) {
                for (uint32_t i = 0; i < e.n_ports && !clash; ++i) clash = pod_lists_key(d, c, ids[e.ports_off + i]);
                for (uint32_t i = 0; i < e.n_pds && !clash; ++i) clash = pod_lists_key(d, c, ids[e.pds_off + i]);
              }
              if (sca) {
#pragma unroll
                for (uint32_t r = 0; r < KSG_MAX_SCALAR; ++r)
                  if (r < d.n_scalar) at.sc[r] += (uint64_t)exts[base + q].scalar[r];
              }
            }
          fit = !clash && node_fail_l<false>(d, c, PtrLists{c.ports, c.pds, c.sel}, n, wi, bit, capc, capm, usedc,
                                             usedm, at) == KSG_FAIL_NONE;
        }
      }
      const uint64_t b = __ballot(fit);
      if (lane == 0) s_bal[it & 1][wv] = b;
      __syncthreads();
#pragma unroll
      for (uint32_t v = 0; v < KSG_PACK_WAVES; ++v) {
        const uint64_t bv = s_bal[it & 1][v];
        if (found < 0 && bv)
          found = (int32_t)((d.nw - 1 - s * KSG_PACK_WAVES - v) * 64 + (63 - (uint32_t)__builtin_clzll(bv)));
      }
      ++it;
    }
    if (found >= 0) {  // (workgroup-uniform) the pod now counts on the node for the set's later pods
      if (tid == 0) {
        const uint32_t t = (uint32_t)found;
        uint32_t h = pack_hash(t);
        while (s_hnode[h] != KSG_PACK_NO_NODE && s_hnode[h] != t) h = (h + 1) & (KSG_PACK_SLOTS - 1);
        const uint32_t prev = s_hnode[h] == t ? s_hhead[h] : KSG_PACK_NONE;
        s_hnode[h] = t;
        s_hhead[h] = (uint16_t)j;
        s_cum[0][j] = (prev == KSG_PACK_NONE ? 0 : s_cum[0][prev]) + (uint64_t)c.req_cpu;
        s_cum[1][j] = (prev == KSG_PACK_NONE ? 0 : s_cum[1][prev]) + (uint64_t)c.req_mem;
        bool holds = c.n_ports + c.n_pds != 0;
        if (exts)
          for (uint32_t r = 0; r < d.n_scalar; ++r) holds = holds || c.ext->scalar[r] != 0;
        const uint16_t kl = prev == KSG_PACK_NONE ? (uint16_t)KSG_PACK_NONE : s_klast[prev];
        s_kprev[j] = kl;
        s_klast[j] = holds ? (uint16_t)j : kl;
      }
      ++n_placed;
      __syncthreads();
    }
    if (tid == 0) out_nodes[p] = found < 0 ? KSG_OUT_NOFIT : found;
  }
  if (tid == 0) placed[set] = n_placed;
}

// k's arrays, pods, exts (optional) and ids are device memory; out_nodes: int32[set_off[n_sets]],
// placed: uint32[n_sets]
hipError_t ksg_launch_pack(const KsgDev& d, const KsgPack& k, const ksg_pod* pods, const ksg_pod_ext* exts,
                           const uint32_t* ids, uint32_t n_sets, int32_t* out_nodes, uint32_t* placed, hipStream_t st) {
  if (n_sets == 0 || d.nw == 0) return hipSuccess;
  hipLaunchKernelGGL(ksg_pack_kernel, dim3(n_sets), dim3(KSG_PACK_STRIP), 0, st, d, k, pods, exts, ids, out_nodes,
                     placed);
  return hipGetLastError();
}
