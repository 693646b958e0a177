// ksg_prioritize.hip — ranked hosts for many pods in one pass (ksg_prioritize_batch):
// prioritizeNodes and the head of the sorted HostPriorityList that selectHost reads
// (generic_scheduler.go:84-96, 136-177; types.go:42-47) for every pod of a list against the
// cluster as it stands. Nothing is committed or drawn. The scoring twin of ksg_explain.hip.
//
// Tiling as there: a workgroup owns KSG_EXPLAIN_TILE nodes, one 64-node bitmap word per wave,
// a lane keeps its node's capacities and requested totals in registers while the workgroup
// walks a chunk of KSG_EXPLAIN_CHUNK pods; grid = node tiles x pod chunks. Every wave
// resolves the pod itself (pod_resolve<false>) and runs node_fail<false> for its lane's node.
// All cluster state is read-only for the call: plain loads, no cross-block waits.
//
// Three kernels on one stream:
//  1. reduce (only with ServiceAntiAffinity, or the TaintToleration score with records): the
//     terms normalised over the pod's filtered nodes, as ksg_scan_kernel's phase 1 takes them
//     for one pod: dnorm[p][anti_dom_off[a] + dom] += svc_cnt of the fitting nodes (summed
//     per wave and distinct domain first), dnorm[p][D] = max soft_taints of the fitting nodes.
//     int32 add and max: the result does not depend on arrival order.
//  2. score: node_fail again (no fit buffer is kept), then node_score + anti_term +
//     w_taint * taint_score combined as scan_pod combines them, always in wrapping int64.
//     Optional scores row, 512 contiguous bytes per wave. Per (pod, tile) one KsgPrioPart and
//     the tile's best `top` entries under the key (score, node rank): each wave takes `top`
//     rounds of arg-max over its 64 nodes (rank rises with the lane, so among equal scores
//     the highest set lane of the ballot wins), leaves them in the LDS, and one wave of the
//     workgroup (they take turns) picks the tile's best from the KSG_PRIO_WAVES lists laid
//     out so that the same rule holds. The LDS lists are double-buffered by pod parity: one
//     barrier per pod.
//  3. merge: one wave per pod over its tile partials: fit_count = sum of the tile fit
//     counts, the max of the tile maxima, tie_count = sum of the counts of the tiles at it,
//     and `top` rounds of "largest key below the previous one" over the tiles' entries (node
//     ranks are distinct, so keys are). The empty-HostPriorityList trap applies here; a pod
//     with a peer error fits nowhere, so its row comes out as 0 / 0 / 0 and -1 / 0.
// No output is written with an atomic, and none depends on workgroup order.
#include <hip/hip_runtime.h>

#include "ksg_device.h"
#include "ksg_launch.h"

static_assert(KSG_EXPLAIN_TILE % 64 == 0, "one bitmap word per wave");
static_assert(KSG_PRIO_WAVES * KSG_PRIO_MAX_TOP == 64, "the tile's candidate lists fill one wave");
static_assert(KSG_SCORE_NOFIT == KSG_SCORE_NONE, "the public sentinel is the kernels'");

// which normalised terms the config has (wave-uniform, fixed for the call)
__host__ __device__ __forceinline__ bool prio_anti(const KsgDev& d) {
  return d.n_anti > 0 && d.n_domains_total > 0 && !d.equal_fallback;
}
__host__ __device__ __forceinline__ bool prio_taint(const KsgDev& d, bool have_ext) {
  return d.w_taint != 0 && have_ext && !d.equal_fallback;
}
bool ksg_prio_needs_reduce(const KsgDev& d, bool have_ext) { return prio_anti(d) || prio_taint(d, have_ext); }

// the lane's node for this block, its validity and register-held state
struct PrioLane {
  uint32_t wi, n;
  uint64_t bit;
  bool valid;
  int64_t capc, capm, usedc, usedm;
};
__device__ __forceinline__ PrioLane prio_lane(const KsgDev& d, uint32_t tid) {
  PrioLane L;
  L.wi = blockIdx.x * KSG_PRIO_WAVES + (tid >> 6);  // wave-uniform
  L.n = L.wi * 64 + (tid & 63);
  L.bit = 1ULL << (tid & 63);
  L.valid = L.wi < d.nw && L.n < d.n_nodes;  // (a lane past the last node fits nothing)
  L.capc = L.capm = L.usedc = L.usedm = 0;
  if (L.valid) {
    L.capc = d.cap_cpu[L.n];
    L.capm = d.cap_mem[L.n];
    L.usedc = d.used_cpu[L.n];
    L.usedm = d.used_mem[L.n];
  }
  return L;
}

__global__ __launch_bounds__(KSG_EXPLAIN_TILE) void ksg_prio_reduce_kernel(KsgDev d, const ksg_pod* __restrict__ pods,
                                                                          const ksg_pod_ext* __restrict__ exts,
                                                                          const uint32_t* __restrict__ ids,
                                                                          uint32_t n_pods, int32_t* __restrict__ dnorm) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const PrioLane L = prio_lane(d, tid);
  if (L.wi >= d.nw) return;  // (no barrier in this kernel)
  const uint32_t p0 = blockIdx.y * KSG_EXPLAIN_CHUNK;
  const uint32_t p1 = min(p0 + (uint32_t)KSG_EXPLAIN_CHUNK, n_pods);
  const bool anti = prio_anti(d), taint = prio_taint(d, exts != nullptr);
  const uint32_t D = d.n_domains_total;
  for (uint32_t p = p0; p < p1; ++p) {
    PodCtx c;
    pod_resolve<false>(d, pods[p], ids, c);
    if (exts) c.ext = exts + p;
    // (anti_term reads no count while the service has no pod at all)
    const bool need = anti && c.svc >= 0 && c.svc_total > 0;
    const bool tt = taint && c.ext->n_soft != 0;
    if (c.error || !(need || tt)) continue;  // wave-uniform
    const bool fit = L.valid && node_fail<false>(d, c, L.n, L.wi, L.bit, L.capc, L.capm, L.usedc, L.usedm) == KSG_FAIL_NONE;
    int32_t* row = dnorm + (size_t)p * (D + 1);
    if (need) {
      const int32_t cnt = fit ? d.svc_cnt[(size_t)c.svc * d.n_nodes + L.n] : 0;
      if (__ballot(cnt != 0)) {
        for (uint32_t a = 0; a < d.n_anti; ++a) {
          const int32_t dom = cnt != 0 ? d.anti_domain[(size_t)a * d.n_nodes + L.n] : -1;
          uint64_t rem = __ballot(dom >= 0);
          while (rem) {  // one add per distinct domain present in the wave
            const int32_t dd = __builtin_amdgcn_readlane(dom, (int)__builtin_ctzll(rem));
            const bool mine = dom == dd;
            const uint32_t s = wave_sum_u32(mine ? (uint32_t)cnt : 0u);
            if (lane == 0) atomicAdd(&row[d.anti_dom_off[a] + dd], (int32_t)s);
            rem &= ~__ballot(mine);
          }
        }
      }
    }
    if (tt) {
      const int32_t s = wave_max_i32(fit ? soft_taints(d, c, L.wi, L.bit) : 0);
      if (lane == 0 && s > 0) atomicMax(&row[D], s);
    }
  }
}

__global__ __launch_bounds__(KSG_EXPLAIN_TILE) void ksg_prio_score_kernel(
    KsgDev d, const ksg_pod* __restrict__ pods, const ksg_pod_ext* __restrict__ exts, const uint32_t* __restrict__ ids,
    uint32_t n_pods, uint32_t top, const int32_t* __restrict__ dnorm, int64_t* __restrict__ scores,
    KsgPrioPart* __restrict__ part, int64_t* __restrict__ cand_score, int32_t* __restrict__ cand_node,
    uint8_t* __restrict__ err) {
  // per wave and pod parity: its best entries, how many, and its max / count at max / fit count
  __shared__ int64_t s_sc[2][KSG_PRIO_WAVES][KSG_PRIO_MAX_TOP];
  __shared__ int32_t s_nd[2][KSG_PRIO_WAVES][KSG_PRIO_MAX_TOP];
  __shared__ int64_t s_wmax[2][KSG_PRIO_WAVES];
  __shared__ uint32_t s_wcnt[2][KSG_PRIO_WAVES], s_wfit[2][KSG_PRIO_WAVES], s_wnc[2][KSG_PRIO_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PrioLane L = prio_lane(d, tid);
  const uint32_t p0 = blockIdx.y * KSG_EXPLAIN_CHUNK;
  const uint32_t p1 = min(p0 + (uint32_t)KSG_EXPLAIN_CHUNK, n_pods);
  const bool anti = prio_anti(d), taint = prio_taint(d, exts != nullptr);
  const uint32_t D = d.n_domains_total;
  const uint32_t tiles = gridDim.x;
  for (uint32_t p = p0; p < p1; ++p) {  // (block-uniform bounds: every wave meets every barrier)
    const uint32_t buf = p & 1;
    PodCtx c;
    pod_resolve<false>(d, pods[p], ids, c);
    if (exts) c.ext = exts + p;
    if (blockIdx.x == 0 && tid == 0) err[p] = c.error ? 1 : 0;
    bool fit = false;
    int64_t sc = KSG_SCORE_NONE;
    if (L.valid && !c.error &&
        node_fail<false>(d, c, L.n, L.wi, L.bit, L.capc, L.capm, L.usedc, L.usedm) == KSG_FAIL_NONE) {
      fit = true;
      const bool need_cnt = (d.w_spread != 0 || anti) && c.svc >= 0;
      const int32_t cnt = need_cnt ? d.svc_cnt[(size_t)c.svc * d.n_nodes + L.n] : 0;
      sc = node_score(d, c, L.n, L.capc, L.capm, L.usedc, L.usedm, cnt);
      const int32_t* row = dnorm + (size_t)p * (D + 1);  // (only read with anti or taint)
      if (anti) sc = wsum(sc, anti_term(d, c, L.n, row));
      if (taint) sc = wsum(sc, wmul((int64_t)d.w_taint, taint_score(soft_taints(d, c, L.wi, L.bit), row[D])));
    }
    if (scores && L.valid) scores[(size_t)p * d.n_nodes + L.n] = sc;
    // this wave's 64 nodes
    const uint64_t fb = __ballot(fit);
    const int64_t wm = wave_max_i64(fit ? sc : KSG_SCORE_NONE);
    const uint64_t tb = __ballot(fit && sc == wm);
    if (lane == 0) {
      s_wmax[buf][wave] = wm;
      s_wcnt[buf][wave] = (uint32_t)__popcll(tb);
      s_wfit[buf][wave] = (uint32_t)__popcll(fb);
    }
    uint64_t alive = fb;
    uint32_t nc = 0;
    for (; nc < top && alive; ++nc) {
      const bool a = (alive >> lane) & 1;
      const int64_t m = nc == 0 ? wm : wave_max_i64(a ? sc : KSG_SCORE_NONE);
      const uint64_t b = __ballot(a && sc == m);  // (non-empty: the max is some live lane's)
      const uint32_t w = 63u - (uint32_t)__builtin_clzll(b);
      if (lane == w) {
        s_sc[buf][wave][nc] = sc;
        s_nd[buf][wave][nc] = (int32_t)L.n;
      }
      alive &= ~(1ULL << w);
    }
    if (lane == 0) s_wnc[buf][wave] = nc;
    __syncthreads();
    if (wave == (p % KSG_PRIO_WAVES)) {  // the tile: this wave's turn
      const size_t slot = (size_t)p * tiles + blockIdx.x;
      uint32_t tf = 0, tc = 0;
      int64_t tm = KSG_SCORE_NONE;
#pragma unroll
      for (uint32_t w = 0; w < KSG_PRIO_WAVES; ++w) {
        if (!s_wfit[buf][w]) continue;
        const int64_t m = s_wmax[buf][w];
        if (tf == 0 || m > tm) {
          tm = m;
          tc = s_wcnt[buf][w];
        } else if (m == tm) {
          tc += s_wcnt[buf][w];
        }
        tf += s_wfit[buf][w];
      }
      if (lane == 0) {
        KsgPrioPart pp;
        pp.max = tm;
        pp.cnt = tc;
        pp.fit = tf;
        part[slot] = pp;
      }
      // lane = wave's list * MAX_TOP + (MAX_TOP - 1 - entry): among equal scores the higher list
      // holds the higher ranks and within a list the earlier entry does, so the highest lane wins
      const uint32_t lw = lane / KSG_PRIO_MAX_TOP, lj = KSG_PRIO_MAX_TOP - 1 - (lane % KSG_PRIO_MAX_TOP);
      bool live = lj < s_wnc[buf][lw];
      const int64_t csc = live ? s_sc[buf][lw][lj] : KSG_SCORE_NONE;
      const int32_t cnd = live ? s_nd[buf][lw][lj] : -1;
      uint32_t j = 0;
      for (; j < top; ++j) {
        const int64_t m = wave_max_i64(live ? csc : KSG_SCORE_NONE);
        const uint64_t b = __ballot(live && csc == m);
        if (!b) break;
        if (lane == 63u - (uint32_t)__builtin_clzll(b)) {
          cand_score[slot * top + j] = csc;
          cand_node[slot * top + j] = cnd;
          live = false;
        }
      }
      if (lane >= j && lane < top) {  // past the tile's fitting nodes
        cand_score[slot * top + lane] = 0;
        cand_node[slot * top + lane] = -1;
      }
    }
  }
}

__global__ __launch_bounds__(64) void ksg_prio_merge_kernel(KsgDev d, uint32_t n_pods, uint32_t top, uint32_t tiles,
                                                           const KsgPrioPart* __restrict__ part,
                                                           const int64_t* __restrict__ cand_score,
                                                           const int32_t* __restrict__ cand_node,
                                                           int64_t* __restrict__ max_score,
                                                           uint32_t* __restrict__ tie_count,
                                                           uint32_t* __restrict__ fit_count,
                                                           int32_t* __restrict__ top_nodes,
                                                           int64_t* __restrict__ top_scores) {
  const uint32_t p = blockIdx.x, lane = threadIdx.x;
  if (p >= n_pods) return;
  const KsgPrioPart* pp = part + (size_t)p * tiles;
  uint32_t f = 0;
  int64_t m = KSG_SCORE_NONE;
  bool any = false;
  for (uint32_t t = lane; t < tiles; t += 64)
    if (pp[t].fit) {
      f += pp[t].fit;
      m = (!any || pp[t].max > m) ? pp[t].max : m;
      any = true;
    }
  const uint32_t F = wave_sum_u32(f);
  const int64_t M = wave_max_i64(any ? m : KSG_SCORE_NONE);
  uint32_t k = 0;
  for (uint32_t t = lane; t < tiles; t += 64)
    if (pp[t].fit && pp[t].max == M) k += pp[t].cnt;
  uint32_t K = wave_sum_u32(k);
  if (F == 0 || d.empty_priorities) K = 0;  // nothing fits / all weights 0: empty HostPriorityList
  if (lane == 0) {
    max_score[p] = K ? M : 0;
    tie_count[p] = K;
    fit_count[p] = F;
  }
  const uint32_t Lst = K ? min(top, F) : 0;
  const uint32_t nc = tiles * top;
  const int64_t* cs = cand_score + (size_t)p * nc;
  const int32_t* cn = cand_node + (size_t)p * nc;
  bool have_prev = false;
  int64_t ps = 0;
  int32_t pn = 0;
  uint32_t j = 0;
  for (; j < Lst; ++j) {
    bool has = false;
    int64_t bs = KSG_SCORE_NONE;
    int32_t bn = -1;
    for (uint32_t i = lane; i < nc; i += 64) {
      const int32_t nd = cn[i];
      if (nd < 0) continue;
      const int64_t s = cs[i];
      if (have_prev && !(s < ps || (s == ps && nd < pn))) continue;  // already listed
      if (!has || s > bs || (s == bs && nd > bn)) {
        has = true;
        bs = s;
        bn = nd;
      }
    }
    const int64_t ws = wave_max_i64(has ? bs : KSG_SCORE_NONE);
    const bool at = has && bs == ws;
    if (!__ballot(at)) break;
    const int32_t wn = wave_max_i32(at ? bn : -1);
    if (lane == 0) {
      top_scores[(size_t)p * top + j] = ws;
      top_nodes[(size_t)p * top + j] = wn;
    }
    have_prev = true;
    ps = ws;
    pn = wn;
  }
  if (lane >= j && lane < top) {
    top_scores[(size_t)p * top + lane] = 0;
    top_nodes[(size_t)p * top + lane] = -1;
  }
}

static dim3 prio_grid(const KsgDev& d, uint32_t n_pods) {
  return dim3((d.nw + KSG_PRIO_WAVES - 1) / KSG_PRIO_WAVES, (n_pods + KSG_EXPLAIN_CHUNK - 1) / KSG_EXPLAIN_CHUNK);
}

// dnorm zeroed by the caller; grid.y covers n_pods
hipError_t ksg_launch_prio_reduce(const KsgDev& d, const ksg_pod* pods, const ksg_pod_ext* exts, const uint32_t* ids,
                                  uint32_t n_pods, int32_t* dnorm, hipStream_t st) {
  if (n_pods == 0 || d.nw == 0) return hipSuccess;
  hipLaunchKernelGGL(ksg_prio_reduce_kernel, prio_grid(d, n_pods), dim3(KSG_EXPLAIN_TILE), 0, st, d, pods, exts, ids,
                     n_pods, dnorm);
  return hipGetLastError();
}

// part / cand_*: [n_pods][node tiles] and [n_pods][node tiles][top]; scores: optional
hipError_t ksg_launch_prio_score(const KsgDev& d, const ksg_pod* pods, const ksg_pod_ext* exts, const uint32_t* ids,
                                 uint32_t n_pods, uint32_t top, const int32_t* dnorm, int64_t* scores,
                                 KsgPrioPart* part, int64_t* cand_score, int32_t* cand_node, uint8_t* err,
                                 hipStream_t st) {
  if (n_pods == 0 || d.nw == 0) return hipSuccess;
  hipLaunchKernelGGL(ksg_prio_score_kernel, prio_grid(d, n_pods), dim3(KSG_EXPLAIN_TILE), 0, st, d, pods, exts, ids,
                     n_pods, top, dnorm, scores, part, cand_score, cand_node, err);
  return hipGetLastError();
}

hipError_t ksg_launch_prio_merge(const KsgDev& d, uint32_t n_pods, uint32_t top, const KsgPrioPart* part,
                                 const int64_t* cand_score, const int32_t* cand_node, int64_t* max_score,
                                 uint32_t* tie_count, uint32_t* fit_count, int32_t* top_nodes, int64_t* top_scores,
                                 hipStream_t st) {
  if (n_pods == 0 || d.nw == 0) return hipSuccess;
  hipLaunchKernelGGL(ksg_prio_merge_kernel, dim3(n_pods), dim3(64), 0, st, d, n_pods, top, prio_grid(d, 1).x, part,
                     cand_score, cand_node, max_score, tie_count, fit_count, top_nodes, top_scores);
  return hipGetLastError();
}
