// ksg_headroom.hip — how many copies of a pod each node can take (ksg_headroom_batch): for
// every pod of a list and every node, the number of copies AssumePod could add to that node one
// after another before the node's predicates refuse the next, capped at `limit`, and the
// constraint that stops it. The predicates of this reference are per-node monotone in the
// number of copies, so the count has a closed form per (pod, node) (node_room, ksg_device.h;
// DESIGN.md has the proof). Nothing is committed, scored or drawn.
//
// The tiling is ksg_explain_kernel's: a workgroup owns KSG_HEADROOM_TILE nodes, one 64-node
// bitmap word per wave, and a lane keeps its node's capacities and requested totals in
// registers while the workgroup walks a chunk of KSG_HEADROOM_CHUNK pods. Per pod every wave
// resolves the pod (pod_resolve<false>), runs node_fail<false> for its lane's node, and only a
// lane whose node fits goes on to node_room and its quotients. All state is read-only for the
// kernel's lifetime: plain loads, no cross-block waits, and no atomics but the result adds.
//
// Outputs: (a) optionally counts[p * n_nodes + n], 64 contiguous uint32 per wave; (b) per pod
// the sum of the counts (uint64), their maximum, the nodes with a non-zero count, and
// hist[p][KSG_HEADROOM_SLOTS], slot b = nodes whose binding is b. Per wave: the sum as two
// 16-bit halves through the DPP add scan, the maximum through the DPP max scan, one
// ballot/popcount per distinct binding present; a wave no node of which fits only counts its
// nodes into slot KSG_ROOM_NONE. Summed per block in the LDS and flushed once per pod per
// block into buffers the caller zeroed; (c) err[p] = KSG_HEADROOM_ERR_*: the rows stay zero.
#include <hip/hip_runtime.h>

#include "ksg_device.h"
#include "ksg_launch.h"

#define KSG_HEADROOM_WAVES (KSG_HEADROOM_TILE / 64)
static_assert(KSG_HEADROOM_TILE % 64 == 0, "one bitmap word per wave");
static_assert((KSG_HEADROOM_SLOTS & (KSG_HEADROOM_SLOTS - 1)) == 0 &&
                  KSG_ROOM_SCALAR0 + KSG_MAX_SCALAR <= KSG_HEADROOM_SLOTS,
              "histogram slots: a power of two past the last binding");

template <int DIV>
__global__ __launch_bounds__(KSG_HEADROOM_TILE) void ksg_headroom_kernel(
    KsgDev d, const ksg_pod* __restrict__ pods, const ksg_pod_ext* __restrict__ exts, const uint32_t* __restrict__ ids,
    uint32_t n_pods, uint32_t limit, uint32_t* __restrict__ counts, unsigned long long* __restrict__ total,
    uint32_t* __restrict__ max_count, uint32_t* __restrict__ fit_count, uint32_t* __restrict__ hist,
    uint8_t* __restrict__ err) {
  __shared__ unsigned long long s_tot[KSG_HEADROOM_CHUNK];
  __shared__ uint32_t s_max[KSG_HEADROOM_CHUNK], s_fit[KSG_HEADROOM_CHUNK];
  __shared__ uint32_t s_hist[KSG_HEADROOM_CHUNK * KSG_HEADROOM_SLOTS];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wi = blockIdx.x * KSG_HEADROOM_WAVES + (tid >> 6);  // wave-uniform
  const uint32_t n = wi * 64 + lane;
  const uint64_t bit = 1ULL << lane;
  const bool valid = wi < d.nw && n < d.n_nodes;  // the last word's tail neither stores nor counts
  const uint32_t p0 = blockIdx.y * KSG_HEADROOM_CHUNK;
  const uint32_t p1 = min(p0 + (uint32_t)KSG_HEADROOM_CHUNK, n_pods);
  for (uint32_t i = tid; i < KSG_HEADROOM_CHUNK * KSG_HEADROOM_SLOTS; i += KSG_HEADROOM_TILE) s_hist[i] = 0;
  for (uint32_t i = tid; i < KSG_HEADROOM_CHUNK; i += KSG_HEADROOM_TILE) s_tot[i] = 0, s_max[i] = 0, s_fit[i] = 0;
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
      // a negative request makes the count non-monotone in the copies: an error row
      bool neg = c.req_cpu < 0 || c.req_mem < 0;
      if (exts)
        for (uint32_t r = 0; r < d.n_scalar; ++r) neg |= exts[p].scalar[r] < 0;
      const int e = c.error ? KSG_HEADROOM_ERR_PEER : neg ? KSG_HEADROOM_ERR_NEGATIVE : 0;
      if (blockIdx.x == 0 && tid == 0) err[p] = (uint8_t)e;
      if (e) {  // wave-uniform: the rows stay zero
        if (counts && valid) counts[(size_t)p * d.n_nodes + n] = 0;
        continue;
      }
      uint32_t cnt = 0;
      int bind = KSG_ROOM_NONE;
      // (node_fail's extended-resource loads are indexed by n: only for a lane with a node)
      if (valid && node_fail<false>(d, c, n, wi, bit, capc, capm, usedc, usedm) == KSG_FAIL_NONE)
        cnt = node_room<false, DIV>(d, c, n, capc, capm, usedc, usedm, limit, bind);
      if (counts && valid) counts[(size_t)p * d.n_nodes + n] = cnt;
      const uint64_t fitm = __ballot(cnt != 0);
      const uint32_t row = (p - p0) * KSG_HEADROOM_SLOTS;
      if (lane == 0 && (live & ~fitm)) atomicAdd(&s_hist[row + KSG_ROOM_NONE], (uint32_t)__popcll(live & ~fitm));
      if (!fitm) continue;  // wave-uniform
      const uint64_t sum = (uint64_t)wave_total_add(cnt & 0xffffu) + ((uint64_t)wave_total_add(cnt >> 16) << 16);
      const uint32_t mx = (uint32_t)wave_total_max((int32_t)(cnt ^ 0x80000000u)) ^ 0x80000000u;  // unsigned order
      uint64_t rem = fitm;
      while (rem) {  // one ballot per distinct binding present
        const int bb = __builtin_amdgcn_readlane(bind, (int)__builtin_ctzll(rem));
        const uint64_t m = __ballot(cnt != 0 && bind == bb);
        if (lane == 0) atomicAdd(&s_hist[row + bb], (uint32_t)__popcll(m));
        rem &= ~m;
      }
      if (lane == 0) {
        atomicAdd(&s_tot[p - p0], (unsigned long long)sum);
        atomicMax(&s_max[p - p0], mx);
        atomicAdd(&s_fit[p - p0], (uint32_t)__popcll(fitm));
      }
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < (p1 - p0) * KSG_HEADROOM_SLOTS; i += KSG_HEADROOM_TILE)
    if (s_hist[i]) atomicAdd(hist + (size_t)p0 * KSG_HEADROOM_SLOTS + i, s_hist[i]);
  for (uint32_t i = tid; i < p1 - p0; i += KSG_HEADROOM_TILE)
    if (s_fit[i]) {
      atomicAdd(total + p0 + i, s_tot[i]);
      atomicMax(max_count + p0 + i, s_max[i]);
      atomicAdd(fit_count + p0 + i, s_fit[i]);
    }
}

// counts: optional (nullptr: no per-node values); total, max_count, fit_count, hist and err
// zeroed by the caller; grid.y covers n_pods; div: udiv_capped's variant (ksg_device.h)
hipError_t ksg_launch_headroom(const KsgDev& d, const ksg_pod* pods, const ksg_pod_ext* exts, const uint32_t* ids,
                               uint32_t n_pods, uint32_t limit, int div, uint32_t* counts, uint64_t* total,
                               uint32_t* max_count, uint32_t* fit_count, uint32_t* hist, uint8_t* err, hipStream_t st) {
  if (n_pods == 0 || d.nw == 0) return hipSuccess;
  const dim3 grid((d.nw + KSG_HEADROOM_WAVES - 1) / KSG_HEADROOM_WAVES,
                  (n_pods + KSG_HEADROOM_CHUNK - 1) / KSG_HEADROOM_CHUNK);
  auto* tot = reinterpret_cast<unsigned long long*>(total);
  auto k = div == 0 ? ksg_headroom_kernel<0> : div == 2 ? ksg_headroom_kernel<2> : ksg_headroom_kernel<1>;
  hipLaunchKernelGGL(k, grid, dim3(KSG_HEADROOM_TILE), 0, st, d, pods, exts, ids, n_pods, limit, counts, tot, max_count,
                     fit_count, hist, err);
  return hipGetLastError();
}
