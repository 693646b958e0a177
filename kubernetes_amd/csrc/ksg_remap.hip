// ksg_remap.hip — ksg_update_cluster's device path: the mutable pod state of the old node
// list renamed into the arrays of the new one, without a pod crossing the ABI.
//
// The host (ksg_update_cluster, ksg_runtime.cpp) uploads src[new n_nodes]: the old rank of the node that now has
// rank n, or -1 for a node nothing survives into (new, or a host that joined the list; the
// joined hosts' pods are patched in afterwards). It has validated every entry against the old
// node count, so no kernel here reads outside an old row. Three kernels, no waits, no spins, no
// atomics; every output word has exactly one writer.
//
//   rows:  new[row][n] = src[n] >= 0 ? old[row][src[n]] : 0 for the per-node rows (used_cpu,
//          used_mem, scalar_used[r]: int64; svc_cnt[s]: int32). Grid (node tiles, rows), a
//          thread per node: the stores are coalesced, the loads as good as (both lists are in
//          name order in practice, so survivors keep their relative order), but nothing relies
//          on that order.
//   bits:  the bitmap rows (keymap[k], svc_bits[s]). One wave per (row, new word): lane j owns
//          node 64 w + j, fetches its old bit, and the new word is the wave's 64-bit ballot,
//          stored by lane 0. Lanes at or past n_nodes vote 0, so the tail bits are zero.
//   svc:   one workgroup per service: svc_max = max(new svc_cnt row, outside_max[s]) with the
//          host's largest count on a host outside the new list, svc_total copied, svc_peer from
//          the host (it knows the members' order of addition).
#include <hip/hip_runtime.h>

#include "ksg_launch.h"

namespace {

constexpr uint32_t kRemapBlock = 256;

template <typename T>
__global__ void __launch_bounds__(kRemapBlock)
ksg_remap_rows_kernel(const T* __restrict__ old_rows, T* __restrict__ new_rows, const int32_t* __restrict__ src,
                      uint32_t old_n, uint32_t new_n, uint32_t rows) {
  const uint32_t n = blockIdx.x * kRemapBlock + threadIdx.x;
  if (n >= new_n) return;
  const int32_t s = src[n];
  for (uint32_t r = blockIdx.y; r < rows; r += gridDim.y)
    new_rows[(size_t)r * new_n + n] = s >= 0 ? old_rows[(size_t)r * old_n + (uint32_t)s] : T(0);
}

__global__ void __launch_bounds__(kRemapBlock)
ksg_remap_bits_kernel(const uint64_t* __restrict__ old_rows, uint64_t* __restrict__ new_rows,
                      const int32_t* __restrict__ src, uint32_t old_nw, uint32_t new_nw, uint32_t new_n, uint64_t waves) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wave = (uint64_t)blockIdx.x * (kRemapBlock / 64) + (threadIdx.x >> 6);
  if (wave >= waves) return;  // (wave-uniform: the ballot below sees whole waves)
  const uint64_t row = wave / new_nw;
  const uint32_t w = (uint32_t)(wave % new_nw);
  const uint32_t n = w * 64u + lane;
  bool bit = false;
  if (n < new_n) {
    const int32_t s = src[n];
    if (s >= 0) bit = (old_rows[row * old_nw + ((uint32_t)s >> 6)] >> ((uint32_t)s & 63u)) & 1ull;
  }
  const unsigned long long word = __ballot(bit);
  if (lane == 0) new_rows[row * new_nw + w] = word;
}

__global__ void __launch_bounds__(kRemapBlock)
ksg_remap_svc_kernel(const int32_t* __restrict__ new_cnt, uint32_t new_n, const int32_t* __restrict__ outside_max,
                     const int32_t* __restrict__ peer, const int32_t* __restrict__ old_total,
                     int32_t* __restrict__ svc_max, int32_t* __restrict__ svc_total, int32_t* __restrict__ svc_peer) {
  __shared__ int32_t part[kRemapBlock / 64];
  const uint32_t s = blockIdx.x;
  const int32_t* row = new_cnt + (size_t)s * new_n;
  int32_t m = 0;
  for (uint32_t n = threadIdx.x; n < new_n; n += kRemapBlock) m = max(m, row[n]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t i = 1; i < kRemapBlock / 64; ++i) m = max(m, part[i]);
    svc_max[s] = max(m, outside_max[s]);
    svc_total[s] = old_total[s];
    svc_peer[s] = peer[s];
  }
}

template <typename T>
hipError_t launch_rows(const T* old_rows, T* new_rows, const int32_t* src, uint32_t old_n, uint32_t new_n, uint32_t rows,
                       hipStream_t st) {
  if (new_n == 0 || rows == 0) return hipSuccess;
  const dim3 grid((new_n + kRemapBlock - 1) / kRemapBlock, rows < 65535u ? rows : 65535u);
  hipLaunchKernelGGL(ksg_remap_rows_kernel<T>, grid, dim3(kRemapBlock), 0, st, old_rows, new_rows, src, old_n, new_n, rows);
  return hipGetLastError();
}

}  // namespace

hipError_t ksg_launch_remap_rows64(const int64_t* old_rows, int64_t* new_rows, const int32_t* src, uint32_t old_n,
                                   uint32_t new_n, uint32_t rows, hipStream_t st) {
  return launch_rows(old_rows, new_rows, src, old_n, new_n, rows, st);
}

hipError_t ksg_launch_remap_rows32(const int32_t* old_rows, int32_t* new_rows, const int32_t* src, uint32_t old_n,
                                   uint32_t new_n, uint32_t rows, hipStream_t st) {
  return launch_rows(old_rows, new_rows, src, old_n, new_n, rows, st);
}

hipError_t ksg_launch_remap_bits(const uint64_t* old_rows, uint64_t* new_rows, const int32_t* src, uint32_t old_nw,
                                 uint32_t new_nw, uint32_t new_n, uint32_t rows, hipStream_t st) {
  const uint64_t waves = (uint64_t)rows * new_nw;
  if (waves == 0) return hipSuccess;
  const uint64_t blocks = (waves + kRemapBlock / 64 - 1) / (kRemapBlock / 64);
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ksg_remap_bits_kernel, dim3((uint32_t)blocks), dim3(kRemapBlock), 0, st, old_rows, new_rows, src,
                     old_nw, new_nw, new_n, waves);
  return hipGetLastError();
}

hipError_t ksg_launch_remap_svc(const int32_t* new_cnt, uint32_t new_n, uint32_t n_services, const int32_t* outside_max,
                                const int32_t* peer, const int32_t* old_total, int32_t* svc_max, int32_t* svc_total,
                                int32_t* svc_peer, hipStream_t st) {
  if (n_services == 0) return hipSuccess;
  hipLaunchKernelGGL(ksg_remap_svc_kernel, dim3(n_services), dim3(kRemapBlock), 0, st, new_cnt, new_n, outside_max, peer,
                     old_total, svc_max, svc_total, svc_peer);
  return hipGetLastError();
}
