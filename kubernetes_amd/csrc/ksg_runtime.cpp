// ksg_runtime.cpp — host runtime of libkschedgpu.so: the C ABI in
// include/kschedgpu.h except the batch entry points, the device-state mirror, the
// RCCL exchange, the per-pod path (begin / commit / evaluate) with its resident
// server, kubelet admission, the pods' extension records and ksg_explain_batch. The batch driver
// (ksg_schedule_batch and its variants) is ksg_batch.cpp, the node list (ksg_set_cluster,
// ksg_update_cluster, the static terms, the node extensions) ksg_cluster.cpp; ksg_host.h holds
// what the files share (struct ksg_ctx, the scratch-buffer types, the helpers declared there).
//
// Reference behaviour mirrored here:
//   genericScheduler.Schedule / selectHost     pkg/scheduler/generic_scheduler.go:54-96
//   MapPodsToMachines (pods keyed by Status.Host)  pkg/scheduler/predicates.go:354-375
//   SimpleModeler.AssumePod / listPods        plugin/pkg/scheduler/modeler.go:77-139
//   ServiceSpread maxCount over all hosts     pkg/scheduler/spreading.go:72-80
//
// The library keeps a host mirror of the mutable per-node state (requested
// totals, conflict-key reference counts, per-service pod counts and peers) so
// ksg_remove_pod can undo exactly; the device copy is authoritative for
// scheduling and is patched from the mirror. All scheduling decisions run in
// the HIP kernels (ksg_kernels.hip); there is no CPU evaluation path.
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "ksg_host.h"
#include "ksg_shard.h"

int fail(ksg_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

// File-local helpers, and the ones ksg_host.h declares for the other host files: none of them
// is exported from the library.
#pragma GCC visibility push(hidden)

// ksg_explain_batch: device staging for the per-node codes of one chunk of pods
constexpr size_t kExplainStageBytes = (size_t)64 << 20;

int pick_R(uint32_t shard_nodes) {
  const uint32_t r = (shard_nodes + KSG_NT - 1) / KSG_NT;
  int R = 1;
  while ((uint32_t)R < r) R <<= 1;
  return R;
}

// ---- patches: host-mirror deltas applied on the device in order ----------
void patch32(ksg_ctx* c, const void* addr, int32_t v) {
  c->patches.push_back(KsgPatch{(uint64_t)(uintptr_t)addr, (uint64_t)(uint32_t)v, 0, 0});
}
void patch64(ksg_ctx* c, const void* addr, int64_t v) {
  c->patches.push_back(KsgPatch{(uint64_t)(uintptr_t)addr, (uint64_t)v, 1, 0});
}
void patch_or(ksg_ctx* c, const void* addr, uint64_t v) {
  c->patches.push_back(KsgPatch{(uint64_t)(uintptr_t)addr, v, 2, 0});
}
void patch_andnot(ksg_ctx* c, const void* addr, uint64_t v) {
  c->patches.push_back(KsgPatch{(uint64_t)(uintptr_t)addr, v, 3, 0});
}

int srv_flush_patches(ksg_ctx* c);

int flush_patches(ksg_ctx* c) {
  if (c->patches.empty()) return KSG_OK;
  if (c->srv_running) return srv_flush_patches(c);
  int rc = c->d_patch.grow(c, c->patches.size());
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_patch, c->patches.data(), c->patches.size() * sizeof(KsgPatch),
                           hipMemcpyHostToDevice, c->st));
  HIPCHK(c, ksg_launch_patch(c->d_patch, (uint32_t)c->patches.size(), c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));  // host vector is reused
  c->patches.clear();
  return KSG_OK;
}

int32_t peer_code(ksg_ctx* c, uint32_t s) {
  if (c->mir.svc_members[s].empty()) return -1;
  const uint32_t h = c->mir.svc_members[s].begin()->second;
  return h < c->cl.N ? (int32_t)h : -2;
}

int32_t recompute_max(ksg_ctx* c, uint32_t s) {
  int32_t m = 0;
  const int32_t* row = c->mir.svc_cnt.data() + (size_t)s * c->cl.N;
  for (uint32_t n = 0; n < c->cl.N; ++n) m = std::max(m, row[n]);
  for (auto& kv : c->mir.svc_ext[s]) m = std::max(m, kv.second);
  return m;
}

// Mirror update for one pod placed on host h. emit=false when the device has
// already applied the same delta (batch commit).
int mirror_add(ksg_ctx* c, uint32_t h, const ksg_pod* p, const uint32_t* ids, bool emit) {
  if (c->pods.count(p->uid)) return fail(c, KSG_ERR_ARG, "duplicate pod uid %llu", (unsigned long long)p->uid);
  PodRec r;
  r.host = h;
  r.cpu = p->milli_cpu;
  r.mem = p->memory;
  r.seq = ++c->seq;
  for (uint32_t i = 0; i < p->n_ports; ++i) r.keys.push_back(ids[p->ports_off + i]);
  for (uint32_t i = 0; i < p->n_pds; ++i) r.keys.push_back(ids[p->pds_off + i]);
  for (uint32_t i = 0; i < p->n_svcs; ++i) r.svcs.push_back(ids[p->svcs_off + i]);
  for (uint32_t k : r.keys)
    if (k >= c->cfg.max_conflict_keys)
      return fail(c, KSG_ERR_CAPACITY, "conflict key %u >= max_conflict_keys %u", k, c->cfg.max_conflict_keys);
  for (uint32_t s : r.svcs)
    if (s >= c->cl.S) return fail(c, KSG_ERR_ARG, "service %u >= n_services %u", s, c->cl.S);
  for (uint32_t q = 0; q < KSG_MAX_SCALAR; ++q) r.scalar[q] = 0;
  if (c->ext_on && c->ext.n_scalar) {  // extension: the pod's extended resource requests
    auto it = c->ext_scalar.find(p->uid);
    if (it != c->ext_scalar.end())
      for (uint32_t q = 0; q < c->ext.n_scalar; ++q) r.scalar[q] = it->second[q];
    if (h < c->cl.N)
      for (uint32_t q = 0; q < c->ext.n_scalar; ++q) {
        if (!r.scalar[q]) continue;
        int64_t& u = c->mir.sc_used[(size_t)q * c->cl.N + h];
        u = (int64_t)((uint64_t)u + (uint64_t)r.scalar[q]);
        if (emit) patch64(c, c->cl.dev.scalar_used + (size_t)q * c->cl.N + h, u);
      }
  }
  if (h < c->cl.N) {
    c->mir.used_c[h] = (int64_t)((uint64_t)c->mir.used_c[h] + (uint64_t)r.cpu);
    c->mir.used_m[h] = (int64_t)((uint64_t)c->mir.used_m[h] + (uint64_t)r.mem);
    c->used_hi = std::max(c->used_hi, std::max(c->mir.used_c[h], c->mir.used_m[h]));
    if (c->mu_neg || c->mir.used_c[h] < 0 || c->mir.used_m[h] < 0) c->mu_dirty = true;
    else c->mu_max = std::max(c->mu_max, std::max(c->mir.used_c[h], c->mir.used_m[h]));
    if (emit) {
      patch64(c, c->cl.dev.used_cpu + h, c->mir.used_c[h]);
      patch64(c, c->cl.dev.used_mem + h, c->mir.used_m[h]);
    }
    for (uint32_t k : r.keys) {
      const uint32_t ref = ++c->mir.key_ref[((uint64_t)k << 32) | h];
      if (ref == 1 && emit) patch_or(c, c->cl.dev.keymap + (size_t)k * c->cl.nw + (h >> 6), 1ULL << (h & 63));
    }
  }
  for (uint32_t s : r.svcs) {
    int32_t v;
    if (h < c->cl.N) {
      v = ++c->mir.svc_cnt[(size_t)s * c->cl.N + h];
      if (emit) patch32(c, c->cl.dev.svc_cnt + (size_t)s * c->cl.N + h, v);
      if (emit && v == 1) patch_or(c, c->cl.dev.svc_bits + (size_t)s * c->cl.nw + (h >> 6), 1ULL << (h & 63));
    } else {
      v = ++c->mir.svc_ext[s][h];
    }
    if (v > c->mir.svc_max[s]) {
      c->mir.svc_max[s] = v;
      if (emit) patch32(c, c->cl.dev.svc_max + s, v);
    }
    ++c->mir.svc_total[s];
    if (emit) patch32(c, c->cl.dev.svc_total + s, c->mir.svc_total[s]);
    c->mir.svc_members[s][r.seq] = h;
    const int32_t pc = peer_code(c, s);
    if (pc != c->mir.svc_peer[s]) {
      c->mir.svc_peer[s] = pc;
      if (emit) patch32(c, c->cl.dev.svc_peer + s, pc);
    }
  }
  c->pods.emplace(p->uid, std::move(r));
  return KSG_OK;
}

void reset_mirror(ksg_ctx* c) {
  c->mir = NodeMirror(c->cl.N, c->cl.S, c->ext.n_scalar);
  c->mu_dirty = true;
  c->used_hi = 0;
  c->ext_scalar.clear();
  c->pods.clear();
  c->seq = 0;
  c->patches.clear();
  c->pending = false;
  c->pend_srv = false;
  c->upd_q.clear();
  c->q_added.clear();
  c->q_removed.clear();
}

int check_pod(ksg_ctx* c, const ksg_pod* p, const uint32_t* ids, size_t n_ids) {
  auto in = [&](uint32_t off, uint32_t n) { return (size_t)off + n <= n_ids; };
  if (!in(p->ports_off, p->n_ports) || !in(p->pds_off, p->n_pds) || !in(p->sel_off, p->n_sel) ||
      !in(p->svcs_off, p->n_svcs))
    return fail(c, KSG_ERR_ARG, "pod id list out of range");
  if (p->host < -2 || p->host >= (int32_t)c->cl.N) return fail(c, KSG_ERR_ARG, "pod host %d out of range", p->host);
  if (p->service < -1 || p->service >= (int32_t)c->cl.S) return fail(c, KSG_ERR_ARG, "pod service out of range");
  for (uint32_t i = 0; i < p->n_ports; ++i)
    if (ids[p->ports_off + i] >= c->cfg.max_conflict_keys) return fail(c, KSG_ERR_CAPACITY, "port key out of range");
  for (uint32_t i = 0; i < p->n_pds; ++i)
    if (ids[p->pds_off + i] >= c->cfg.max_conflict_keys) return fail(c, KSG_ERR_CAPACITY, "pd key out of range");
  for (uint32_t i = 0; i < p->n_sel; ++i)
    if (ids[p->sel_off + i] >= c->cl.n_pairs) return fail(c, KSG_ERR_ARG, "selector pair out of range");
  for (uint32_t i = 0; i < p->n_svcs; ++i)
    if (ids[p->svcs_off + i] >= c->cl.S) return fail(c, KSG_ERR_ARG, "service id out of range");
  for (uint32_t j = 0; j < c->cfg.n_aff_labels; ++j)
    if (p->aff_pair[j] >= (int32_t)c->cl.n_pairs || p->aff_pair[j] < KSG_AFF_INVALID)
      return fail(c, KSG_ERR_ARG, "affinity pair out of range");
  return KSG_OK;
}

int upload_pods(ksg_ctx* c, const ksg_pod* pods, uint32_t n, const uint32_t* ids, size_t n_ids) {
  int rc = c->d_pods.grow(c, n);
  if (rc) return rc;
  rc = c->d_ids.grow(c, std::max<size_t>(n_ids, 1));
  if (rc) return rc;
  // every caller synchronises the stream before it returns, so the staging
  // buffer is free again at the next call
  const size_t pb = (size_t)n * sizeof(ksg_pod), ib = n_ids * sizeof(uint32_t);
  if ((rc = c->h_up.grow(c, pb + ib))) return rc;
  memcpy(c->h_up, pods, pb);
  if (n_ids) memcpy(c->h_up + pb, ids, ib);
  HIPCHK(c, hipMemcpyAsync(c->d_pods, c->h_up, pb, hipMemcpyHostToDevice, c->st));
  if (n_ids) HIPCHK(c, hipMemcpyAsync(c->d_ids, c->h_up + pb, ib, hipMemcpyHostToDevice, c->st));
  return KSG_OK;
}

// the single-pod APIs: pod + ids staged contiguously, one copy into d_one;
// one_pod / one_ids point into it until the next single-pod upload
int upload_one(ksg_ctx* c, const ksg_pod* pod, const uint32_t* ids, size_t n_ids) {
  const size_t pb = (sizeof(ksg_pod) + 15) & ~(size_t)15, ib = std::max<size_t>(n_ids, 1) * sizeof(uint32_t);
  // (extensions: the pod's ksg_pod_ext after the ids, all-zero for the plain entry points)
  const size_t eo = (pb + ib + 15) & ~(size_t)15, eb = c->ext_on ? sizeof(ksg_pod_ext) : 0;
  int rc = c->d_one.grow(c, eo + eb);
  if (rc) return rc;
  if ((rc = c->h_up.grow(c, eo + eb))) return rc;
  memcpy(c->h_up, pod, sizeof(ksg_pod));
  if (n_ids) memcpy(c->h_up + pb, ids, n_ids * sizeof(uint32_t));
  if (eb) {
    if (c->cur_ext) memcpy(c->h_up + eo, c->cur_ext, eb);
    else memset(c->h_up + eo, 0, eb);
  }
  HIPCHK(c, hipMemcpyAsync(c->d_one, c->h_up, eb ? eo + eb : pb + (n_ids ? n_ids * sizeof(uint32_t) : 0),
                           hipMemcpyHostToDevice, c->st));
  c->one_pod = reinterpret_cast<const ksg_pod*>(c->d_one.p);
  c->one_ids = reinterpret_cast<const uint32_t*>(c->d_one + pb);
  c->d_one_ext = eb ? reinterpret_cast<ksg_pod_ext*>(c->d_one + eo) : nullptr;
  return KSG_OK;
}

int ensure_map(ksg_ctx* c) {
  if (c->h_map) return KSG_OK;
  HIPCHK(c, hipHostMalloc((void**)&c->h_map, 64, hipHostMallocCoherent));
  void* dp = nullptr;
  HIPCHK(c, hipHostGetDevicePointer(&dp, c->h_map, 0));
  c->d_map = static_cast<uint8_t*>(dp);
  return KSG_OK;
}

size_t pod_ids_extent(const ksg_pod* p) {
  size_t e = 0;
  e = std::max<size_t>(e, (size_t)p->ports_off + p->n_ports);
  e = std::max<size_t>(e, (size_t)p->pds_off + p->n_pds);
  e = std::max<size_t>(e, (size_t)p->sel_off + p->n_sel);
  e = std::max<size_t>(e, (size_t)p->svcs_off + p->n_svcs);
  return e;
}
// ... and the extension record's taint lists (the single-pod _ext entry points)
size_t call_ids_extent(const ksg_ctx* c, const ksg_pod* p) {
  size_t e = pod_ids_extent(p);
  if (c->cur_ext) {
    e = std::max<size_t>(e, (size_t)c->cur_ext->hard_off + c->cur_ext->n_hard);
    e = std::max<size_t>(e, (size_t)c->cur_ext->soft_off + c->cur_ext->n_soft);
  }
  return e;
}

// the shard records decide reads: all-gathered (exchange path) or this rank's own
uint8_t* rec_buf(ksg_ctx* c) { return c->xchg ? c->cl.d_rec_recv.p : c->cl.d_rec_send.p; }

bool anti_on(const ksg_ctx* c) { return c->cfg.n_anti > 0 && c->cl.dev.n_domains_total > 0; }

// ---- cross-rank exchange: RCCL over xGMI, or the caller's host transport ----
// recv[g * bytes, (g + 1) * bytes) = rank g's send, on c->st
int allgather(ksg_ctx* c, const void* dsend, void* drecv, size_t bytes) {
  if (c->comm) {
    NCCLCHK(c, ncclAllGather(dsend, drecv, bytes, ncclUint8, c->comm, c->st));
    return KSG_OK;
  }
  if (!c->xfn) return fail(c, KSG_ERR_STATE, "sharded context has neither an RCCL communicator nor ksg_set_allgather");
  int rc;
  if ((rc = c->h_xsend.grow(c, bytes)) || (rc = c->h_xrecv.grow(c, bytes * c->world))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_xsend, dsend, bytes, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  if ((rc = c->xfn(c->xuser, c->h_xsend, c->h_xrecv, (uint64_t)bytes)) != 0)
    return fail(c, KSG_ERR_RCCL, "allgather callback returned %d", rc);
  HIPCHK(c, hipMemcpyAsync(drecv, c->h_xrecv, bytes * c->world, hipMemcpyHostToDevice, c->st));
  return KSG_OK;
}

// drecv[i] = sum (wrapping, as ncclSum on int32) or max over the ranks of their dsend[i]
int allreduce_i32(ksg_ctx* c, Reduce op, const int32_t* dsend, int32_t* drecv, uint32_t n) {
  if (c->comm) {
    NCCLCHK(c, ncclAllReduce(dsend, drecv, n, ncclInt32, op == Reduce::Sum ? ncclSum : ncclMax, c->comm, c->st));
    return KSG_OK;
  }
  if (!c->xfn) return fail(c, KSG_ERR_STATE, "sharded context has neither an RCCL communicator nor ksg_set_allgather");
  const size_t bytes = (size_t)n * 4;
  int rc;
  if ((rc = c->h_xsend.grow(c, bytes)) || (rc = c->h_xrecv.grow(c, bytes * (c->world + 1)))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_xsend, dsend, bytes, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  if ((rc = c->xfn(c->xuser, c->h_xsend, c->h_xrecv, (uint64_t)bytes)) != 0)
    return fail(c, KSG_ERR_RCCL, "allgather callback returned %d", rc);
  int32_t* all = reinterpret_cast<int32_t*>(c->h_xrecv.p);
  int32_t* res = all + (size_t)n * c->world;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t acc = (uint32_t)all[i];
    for (int g = 1; g < c->world; ++g) {
      const int32_t v = all[(size_t)g * n + i];
      acc = op == Reduce::Sum ? acc + (uint32_t)v : (uint32_t)std::max((int32_t)acc, v);
    }
    res[i] = (int32_t)acc;
  }
  HIPCHK(c, hipMemcpyAsync(drecv, res, bytes, hipMemcpyHostToDevice, c->st));
  return KSG_OK;
}

// one pod through scan [+ the normalised terms' all-reduces] + record all-gather (device
// only). On a sharded context ServiceAntiAffinity's domain counts and the extension
// TaintTolerationPriority's max are over every shard's filtered nodes: a first pass writes
// this shard's part (dpart: the counts, then the max), the all-reduces combine them (sum,
// max) and the full pass reads the result (dglobal). dext: the pod's extension record.
int scan_exchange(ksg_ctx* c, const ksg_pod* dpod, const uint32_t* dids, int mode, uint8_t* fail_out,
                  int64_t* score_out, const ksg_pod_ext* dext) {
  const bool anti = anti_on(c);
  const bool tt = dext != nullptr && c->ext.w_taint_toleration != 0;
  if ((anti || tt) && c->xchg) {
    HIPCHK(c, ksg_launch_scan(c->cl.R, anti, c->cl.dev, dpod, dids, mode, 1, nullptr, nullptr, c->cl.d_rec_send,
                              c->cl.d_dpart, nullptr, c->st, dext));
    const uint32_t D = c->cl.dev.n_domains_total;
    int rc = anti ? allreduce_i32(c, Reduce::Sum, c->cl.d_dpart, c->cl.d_dglobal, D) : KSG_OK;
    if (!rc && tt) rc = allreduce_i32(c, Reduce::Max, c->cl.d_dpart + D, c->cl.d_dglobal + D, 1);
    if (rc) return rc;
    HIPCHK(c, ksg_launch_scan(c->cl.R, anti, c->cl.dev, dpod, dids, mode, 2, fail_out, score_out, c->cl.d_rec_send,
                              nullptr, c->cl.d_dglobal, c->st, dext));
  } else {
    HIPCHK(c, ksg_launch_scan(c->cl.R, anti, c->cl.dev, dpod, dids, mode, 0, fail_out, score_out, c->cl.d_rec_send,
                              nullptr, nullptr, c->st, dext));
  }
  if (mode == KSG_MODE_BEGIN) {
    if (c->xchg) {
      int rc = allgather(c, c->cl.d_rec_send, c->cl.d_rec_recv, c->cl.rec_bytes);
      if (rc) return rc;
    }  // (one rank: decide reads the record where the scan wrote it, rec_buf)
  }
  return KSG_OK;
}

// |combined score| bound of a weight set: 10 * sum |w| over the score-10
// priorities + |w_equal| (+ the extensions'), exact in 128 bits
unsigned __int128 score_bound(const ksg_config& cf, int64_t w_taint, int64_t w_bal) {
  auto mag = [](int64_t w) -> unsigned __int128 { return w < 0 ? (unsigned __int128)(0 - (uint64_t)w) : (unsigned __int128)w; };
  unsigned __int128 b = 10 * (mag(cf.w_least_requested) + mag(cf.w_service_spreading) + mag(w_taint) + mag(w_bal)) +
                        mag(cf.w_equal);
  for (uint32_t a = 0; a < cf.n_anti; ++a) b += 10 * mag(cf.w_anti[a]);
  for (uint32_t q = 0; q < cf.n_label_pref; ++q) b += 10 * mag(cf.w_pref[q]);
  return b;
}

int cluster_ok(ksg_ctx* c) {
  if (!c->have_cluster) return fail(c, KSG_ERR_STATE, "ksg_set_cluster not called");
  if (c->diverged)
    return fail(c, KSG_ERR_STATE, "device state diverged from the host mirror (a batch failed after its device work "
                "started, or the drop-in server rejected a commit): call ksg_set_cluster");
  return KSG_OK;
}

void drop_deferred(ksg_ctx* c) {
  c->dfr_pods.clear();
  c->dfr_ids.clear();
  c->dfr_out.clear();
  c->dfr_uids.clear();
  c->dfr_sum = 0;
  c->dfr_req = 0;
  c->dfr_neg = false;
}

int flush_deferred(ksg_ctx* c) {
  int rc = KSG_OK;
  for (size_t i = 0; i < c->dfr_out.size() && rc == KSG_OK; ++i)
    if (c->dfr_out[i] >= 0) rc = mirror_add(c, (uint32_t)c->dfr_out[i], &c->dfr_pods[i], c->dfr_ids.data(), false);
  drop_deferred(c);
  return rc;
}

// Waits for the stream's work so far. The batch path's host thread has nothing
// left to do at this point, so it polls an event instead of sleeping in
// hipStreamSynchronize, whose wake-up lands on the per-batch critical path.
int wait_device(ksg_ctx* c) {
  if (!c->spin_wait || !c->ev_wait) {
    HIPCHK(c, hipStreamSynchronize(c->st));
    return KSG_OK;
  }
  HIPCHK(c, hipEventRecord(c->ev_wait, c->st));
  hipError_t e;
  while ((e = hipEventQuery(c->ev_wait)) == hipErrorNotReady) {
  }
  if (e != hipSuccess) return fail(c, KSG_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(e));
  return KSG_OK;
}

// ---- the resident drop-in server (ksg_serve.hip) ------------------------------
// the grid server: plain configurations (no ServiceAntiAffinity, no extensions)
// past srv_grid_min nodes, one scan workgroup per 256 nodes (<= 255)
// nodes per thread of the grid server's scan workgroups
uint32_t srv_npt(const ksg_ctx* c) { return c->cl.hi - c->cl.lo > c->srv_npt4_min ? 4u : 1u; }

bool srv_grid(const ksg_ctx* c) {
  const uint32_t n = c->cl.hi - c->cl.lo, per = KSG_GSRV_NT * srv_npt(c);
  // (extensions: the filters and BalancedAllocation are per node; TaintToleration normalises over
  // the filtered set: the scan workgroups exchange their maxima through device memory)
  // (ServiceAntiAffinity: the domain counts likewise, up to KSG_GSRV_MAXD domains, without extensions)
  return c->srv_grid_on && !(anti_on(c) && (c->ext_on || c->cl.dev.n_domains_total > KSG_GSRV_MAXD)) &&
         !(c->ext_on && !c->srv_grid_ext) &&
         n > c->srv_grid_min &&
         (n + per - 1) / per <= KSG_GSRV_MAXW;
}

bool srv_eligible(const ksg_ctx* c) {
  return c->srv_enabled && c->world == 1 && !c->xchg && (c->cl.R <= KSG_SRV_MAX_R || srv_grid(c)) && !c->cl.dev.wide &&
         c->cl.N > 0;
}

int srv_alloc(ksg_ctx* c) {
  if (!c->srv_box) {
    HIPCHK(c, hipHostMalloc((void**)&c->srv_box, sizeof(KsgSrvBox), hipHostMallocCoherent | hipHostMallocMapped));
    memset(c->srv_box, 0, sizeof(KsgSrvBox));
    void* dp = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&dp, c->srv_box, 0));
    c->srv_dbox = static_cast<KsgSrvBox*>(dp);
  }
  return KSG_OK;
}

// (Re)launches the server on the stream, offering every request after the last
// one answered. A COMMIT is posted without waiting for its answer, so the host's
// srv_served may lag the server's: the response block names the last request the
// server answered, and a server answers a request only once it will complete it
// (the one-workgroup server applies a COMMIT's delta after answering it, before
// it reads the next request or returns). Relaunching at srv_served alone would
// offer an answered COMMIT again and apply its delta twice.
int srv_launch(ksg_ctx* c) {
  if (int rc = srv_alloc(c)) return rc;
  const uint32_t r0 = __atomic_load_n(&c->srv_box->resp[0], __ATOMIC_ACQUIRE);
  if ((int32_t)(r0 - c->srv_served) > 0) c->srv_served = r0;
  const uint32_t start_seq = c->srv_served;
  const size_t nf = ((size_t)(c->cl.hi - c->cl.lo) + 3 & ~(size_t)3) + 64;  // (the grid server stores 4 codes at a time)
  if (c->srv_fail_cap < nf) {
    if (c->srv_fail) (void)hipHostFree(c->srv_fail);
    c->srv_fail = nullptr;
    c->srv_fail_cap = 0;
    HIPCHK(c, hipHostMalloc((void**)&c->srv_fail, nf, hipHostMallocCoherent | hipHostMallocMapped));
    void* dp = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&dp, c->srv_fail, 0));
    c->srv_dfail = static_cast<uint8_t*>(dp);
    c->srv_fail_cap = nf;
  }
  KsgSrvArgs a{c->srv_dbox, c->srv_dfail, start_seq, (uint64_t)c->srv_idle_us * 100,
               (c->srv_stamps ? 1u : 0u) | (c->srv_debug ? 2u : 0u),
               nullptr, 0, ++c->srv_epoch, 0};
  if (srv_grid(c)) {
    const uint32_t n = c->cl.hi - c->cl.lo;
    const size_t need = sizeof(KsgSrvGrid);
    if (c->srv_grid_cap < need) {
      if (c->srv_grid) (void)hipFree(c->srv_grid);
      c->srv_grid = nullptr;
      c->srv_grid_cap = 0;
      HIPCHK(c, hipMalloc((void**)&c->srv_grid, need));
      HIPCHK(c, hipMemsetAsync(c->srv_grid, 0, need, c->st));
      c->srv_grid_cap = need;
    }
    a.grid = c->srv_grid;
    const uint32_t npt = srv_npt(c);
    a.n_workers = (n + KSG_GSRV_NT * npt - 1) / (KSG_GSRV_NT * npt);
    // past 64 scan workgroups their polls of the host block crowd the link: each sleeps ~0.2 us
    // more between polls (measured: 50,000 nodes 73 -> 38 us per pod; no gain at 15,000)
    a.grid_opts = c->srv_grid_opts >= 0 ? (uint32_t)c->srv_grid_opts : a.n_workers > 64 ? 0x10u : 0u;
    HIPCHK(c, ksg_launch_serve_grid((int)npt, c->ext_on, c->cl.dev, a, c->st));
  } else {
    HIPCHK(c, ksg_launch_serve(c->cl.R, anti_on(c), c->ext_on, c->cl.dev, a, c->st));
  }
  c->srv_running = true;
  ++c->srv_launches;
  return KSG_OK;
}

// Waits until request `seq` is answered: its response, or (a grid server's
// BEGIN, parts > 0) that many parts. A server that returned (idle) before it saw
// the request is relaunched to serve it.
int srv_wait(ksg_ctx* c, uint32_t seq, uint32_t parts) {
  const uint32_t* rs = c->srv_box->resp;
  auto done = [&]() {
    if (!parts) return (int32_t)(__atomic_load_n(&rs[0], __ATOMIC_ACQUIRE) - seq) >= 0;  // (answered in order)
    for (uint32_t q = 0; q < parts; ++q)
      if (__atomic_load_n(&c->srv_box->part[q].seq, __ATOMIC_ACQUIRE) != seq ||
          __atomic_load_n(&c->srv_box->part[q].stamp[3], __ATOMIC_ACQUIRE) != seq)  // (both ends of the store)
        return false;
    return true;
  };
  auto t0 = std::chrono::steady_clock::now();
  uint32_t spins = 0, relaunches = 0;
  while (!done()) {
    if ((++spins & 255) != 0) continue;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < 20.0) continue;
    const hipError_t q = hipStreamQuery(c->st);
    if (q == hipSuccess) {  // the server returned without serving `seq`
      if (done()) break;
      if (++relaunches > 3) return fail(c, KSG_ERR_HIP, "drop-in server exits without serving request %u", seq);
      c->srv_running = false;
      if (c->srv_trace) fprintf(stderr, "srv relaunch start %u (waiting %u)\n", c->srv_served, seq);
      if (int rc = srv_launch(c)) return rc;  // (every request after the last answered one is offered again)
      t0 = std::chrono::steady_clock::now();
    } else if (q != hipErrorNotReady) {
      c->srv_running = false;
      std::string marks;
      if (c->srv_debug)  // where each workgroup was (seq:stage), leader first
        for (int i = 0; i < 12; ++i) {
          const uint32_t m = __atomic_load_n(&c->srv_box->dbg[i], __ATOMIC_RELAXED);
          marks += " " + std::to_string(m >> 8) + ":" + std::to_string(m & 255);
        }
      return fail(c, KSG_ERR_HIP, "drop-in server: %s (request %u%s)", hipGetErrorString(q), seq, marks.c_str());
    } else if (us > 5e6) {
      return fail(c, KSG_ERR_HIP, "drop-in server did not answer request %u in 5 s", seq);
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  if ((int32_t)(seq - c->srv_served) > 0) c->srv_served = seq;  // (and every request before it)
  return KSG_OK;
}

// The control block is free once the server has read the last COMMIT (posted
// without waiting for its answer): before the host writes a control request.
int srv_settle(ksg_ctx* c) {
  if (!c->srv_unacked) return KSG_OK;
  const uint32_t u = c->srv_unacked;
  c->srv_unacked = 0;
  if ((int32_t)(c->srv_served - u) < 0)
    if (int rc = srv_wait(c, u, 0)) return rc;
  // resp[KSG_SRV_RESP_REJECTED]: the last request the server rejected, written before its
  // response (later BEGIN answers overwrite resp[0..3], not this word). The host mirror
  // already holds the commit's pod and the device does not: the context is diverged.
  if (__atomic_load_n(&c->srv_box->resp[KSG_SRV_RESP_REJECTED], __ATOMIC_ACQUIRE) == u) {
    c->diverged = true;
    return fail(c, KSG_ERR_STATE, "drop-in server rejected commit request %u (ksg_set_cluster resyncs)", u);
  }
  return KSG_OK;
}

// Posts request ++srv_seq (header dwords hdr[0..KSG_SRV_HDR_DW); the payload
// chunks were written by the caller): a BEGIN into `req`, a control request into
// `creq` once the last COMMIT there was read. A BEGIN carries the last control
// request before it (ARG).
int srv_post(ksg_ctx* c, const uint32_t* hdr_in, uint32_t* seq_out) {
  if (!c->srv_running) {
    if (int rc = srv_launch(c)) return rc;
  }
  const bool ctl = hdr_in[KSG_SRVH_KIND] != KSG_SRV_BEGIN;
  if (ctl) {
    if (int rc = srv_settle(c)) return rc;
  }
  uint32_t hdr[KSG_SRV_HDR_DW];
  memcpy(hdr, hdr_in, sizeof hdr);
  if (!ctl) hdr[KSG_SRVH_ARG] = c->srv_last_ctl;
  if (c->cl.dbg_corrupt) {
    const uint32_t bit = hdr[KSG_SRVH_KIND] == KSG_SRV_COMMIT ? 1u : hdr[KSG_SRVH_KIND] == KSG_SRV_BEGIN ? 2u : 0u;
    if (c->cl.dbg_corrupt & bit) {
      hdr[KSG_SRVH_IDS_AT] = KSG_SRV_PAY_DW + 1;  // (past the payload: req_bad)
      c->cl.dbg_corrupt &= ~bit;
    }
  }
  const uint32_t seq = ++c->srv_seq;
  if (ctl) c->srv_last_ctl = seq;
  if (c->srv_trace)
    fprintf(stderr, "srv post %u kind %u arg %u served %u\n", seq, hdr[KSG_SRVH_KIND], hdr[KSG_SRVH_ARG], c->srv_served);
  uint32_t* req = ctl ? c->srv_box->creq : c->srv_box->req;
  for (uint32_t i = 0; i < KSG_SRV_HDR_DW; ++i) req[4 * (i / KSG_SRV_CHUNK_DW) + i % KSG_SRV_CHUNK_DW] = hdr[i];
  std::atomic_thread_fence(std::memory_order_release);  // data, then tags (x86: stores stay in order)
  for (uint32_t q = 0; q < KSG_SRV_CHUNKS; ++q) __atomic_store_n(&req[4 * q + 3], seq, __ATOMIC_RELEASE);
  *seq_out = seq;
  return KSG_OK;
}

// Posts a request and waits for its response {seq, a, b, c}.
int srv_call(ksg_ctx* c, const uint32_t* hdr, uint32_t* resp4) {
  uint32_t seq = 0;
  if (int rc = srv_post(c, hdr, &seq)) return rc;
  if (int rc = srv_wait(c, seq, 0)) return rc;
  const uint32_t* rs = c->srv_box->resp;
  for (int i = 0; i < 4; ++i) resp4[i] = __atomic_load_n(&rs[i], __ATOMIC_RELAXED);
  if (c->srv_stamps && hdr[KSG_SRVH_KIND] == KSG_SRV_BEGIN && __atomic_load_n(&rs[10], __ATOMIC_RELAXED) == seq) {
    for (int i = 0; i < 6; ++i) c->srv_stage[i] += (int32_t)__atomic_load_n(&rs[4 + i], __ATOMIC_RELAXED);
    ++c->srv_stamped;
  }
  return KSG_OK;
}

// A BEGIN on either server: {k | ~0u (no peer) | KSG_SRV_BADREQ, max} and the
// tie words into srv_tw. The grid server's parts are merged here.
int srv_begin(ksg_ctx* c, const uint32_t* hdr, uint32_t* resp4) {
  const uint32_t n = c->cl.hi - c->cl.lo, nwd = (n + 63) / 64;
  if (!srv_grid(c)) {
    if (int rc = srv_call(c, hdr, resp4)) return rc;
    if (resp4[1] != KSG_SRV_BADREQ && resp4[1] != ~0u && resp4[1] > 0)
      c->srv_tw.assign(c->srv_box->ties, c->srv_box->ties + nwd);
    return KSG_OK;
  }
  const uint32_t npt = srv_npt(c), G = (n + KSG_GSRV_NT * npt - 1) / (KSG_GSRV_NT * npt), NWG = 4 * npt;
  uint32_t seq = 0;
  if (int rc = srv_post(c, hdr, &seq)) return rc;
  if (int rc = srv_wait(c, seq, G)) return rc;
  const KsgSrvPart* pt = c->srv_box->part;
  int32_t M = KSG_S32_NONE;
  uint32_t err = 0;
  for (uint32_t q = 0; q < G; ++q) {
    M = std::max(M, pt[q].max);
    err |= pt[q].err;
  }
  uint32_t k = 0;
  c->srv_tw.assign((size_t)G * NWG, 0);
  if (M != KSG_S32_NONE)
    for (uint32_t q = 0; q < G; ++q)
      if (pt[q].max == M) {
        k += pt[q].cnt;
        const uint64_t* tw = npt == 1 ? pt[q].tie : c->srv_box->part_tie + (size_t)q * KSG_GSRV_TIEW;
        for (uint32_t r = 0; r < NWG; ++r) c->srv_tw[(size_t)q * NWG + r] = tw[r];
      }
  c->srv_tw.resize(nwd);
  if (c->srv_stamps) {  // worker 0: masks + loads, eval + publish (100-MHz ticks)
    c->srv_stage[0] += (int32_t)(pt[0].stamp[1] - pt[0].stamp[0]);
    c->srv_stage[1] += (int32_t)(pt[0].stamp[2] - pt[0].stamp[1]);  // (stamp[3]: the sequence number)
    ++c->srv_stamped;
  }
  resp4[0] = seq;
  resp4[1] = (err & 2) ? KSG_SRV_BADREQ : err ? ~0u : k;
  if (c->srv_trace) fprintf(stderr, "srv begin %u max %d k %u err %u\n", seq, M, k, err);
  const int64_t m64 = M;
  resp4[2] = (uint32_t)(uint64_t)m64;
  resp4[3] = (uint32_t)((uint64_t)m64 >> 32);
  return KSG_OK;
}

// the t-th set bit (ascending) of the tie words -> node offset, -1 if none
int64_t srv_pick(const std::vector<uint64_t>& tw, uint64_t t) {
  uint64_t acc = 0;
  for (size_t i = 0; i < tw.size(); ++i) {
    const uint64_t pc = (uint64_t)__builtin_popcountll(tw[i]);
    if (t < acc + pc) {
      uint64_t w = tw[i];
      for (uint64_t j = acc; j < t; ++j) w &= w - 1;  // drop the lower set bits
      return (int64_t)(i * 64 + (uint64_t)__builtin_ctzll(w));
    }
    acc += pc;
  }
  return -1;
}

// Ends the resident server so other work can use the stream.
int srv_stop(ksg_ctx* c) {
  if (!c->srv_running) return KSG_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = srv_settle(c)) return rc;  // (the last commit is applied first)
  if (hipStreamQuery(c->st) != hipSuccess) {
    uint32_t hdr[KSG_SRV_HDR_DW] = {KSG_SRV_EXIT};
    uint32_t r[4];
    if (int rc = srv_call(c, hdr, r)) return rc;
  }
  c->srv_running = false;
  // (a pending begin served by the server stays pending: its commit picks the node from
  // srv_tw on the host and posts the COMMIT to a relaunched server)
  HIPCHK(c, hipStreamSynchronize(c->st));
  return KSG_OK;
}

// int64 combined scores (the exact kernels; the window path and the resident servers are
// int32): once a |score| could reach KSG_SCORE_BOUND by the weights, or a LeastRequested
// term can leave the [0, 10] that bound assumes
void set_wide(ksg_ctx* c) {
  c->cl.dev.wide = score_bound(c->cfg, c->ext.w_taint_toleration, c->ext.w_balanced) + c->cl.static_mag >=
                    (unsigned __int128)KSG_SCORE_BOUND ||
                (c->cl.lr_wild && c->cfg.w_least_requested != 0);
}

// Pods about to be filtered, scored or committed. A negative request, or a requested total that could pass 2^63 - 1 and wrap
// negative, takes calculateScore out of [0, 10]: the context turns to the int64 kernels
// (the servers leave the stream and decline it from here on) until ksg_set_cluster.
int note_requests(ksg_ctx* c, const ksg_pod* pods, uint32_t n) {
  if (c->cl.lr_wild || c->cfg.w_least_requested == 0) return KSG_OK;
  bool wild = c->used_hi < 0;
  unsigned __int128 sum = 0;
  for (uint32_t i = 0; i < n; ++i) {
    wild |= pods[i].milli_cpu < 0 || pods[i].memory < 0;
    if (!wild) sum += (uint64_t)std::max(pods[i].milli_cpu, pods[i].memory);
  }
  wild = wild || (unsigned __int128)(uint64_t)std::max<int64_t>(c->used_hi, 0) + c->dfr_req + sum >
                     (unsigned __int128)INT64_MAX;
  if (!wild) return KSG_OK;
  c->cl.lr_wild = true;
  if (!c->cl.dev.wide) {
    if (int rc = srv_stop(c)) return rc;
    set_wide(c);
  }
  return KSG_OK;
}

int srv_flush_patches(ksg_ctx* c) {
  if (int rc = srv_alloc(c)) return rc;
  size_t at = 0;
  while (at < c->patches.size()) {
    const uint32_t n = (uint32_t)std::min<size_t>(c->patches.size() - at, KSG_SRV_PATCHES);
    memcpy(c->srv_box->patch, c->patches.data() + at, (size_t)n * sizeof(KsgPatch));
    uint32_t hdr[KSG_SRV_HDR_DW] = {KSG_SRV_PATCH};
    hdr[KSG_SRVH_NPATCH] = n;
    uint32_t r[4];
    if (int rc = srv_call(c, hdr, r)) return rc;
    at += n;
  }
  c->patches.clear();
  return KSG_OK;
}

// The pod, its ids [0, n_ids) and (extensions) its record as the request
// payload; false if it does not fit the block + ext area.
bool srv_put_pod(ksg_ctx* c, const ksg_pod* pod, const uint32_t* ids, size_t n_ids, const ksg_pod_ext* ext,
                 uint32_t* hdr, bool ctl = false) {
  const uint32_t pod_dw = (uint32_t)(sizeof(ksg_pod) / 4), ext_dw = (uint32_t)(sizeof(ksg_pod_ext) / 4);
  const uint32_t ids_at = pod_dw;
  const uint32_t ext_at = (ids_at + (uint32_t)n_ids + 1) & ~1u;  // 8-byte aligned
  const uint64_t paydw = ext ? (uint64_t)ext_at + ext_dw : (uint64_t)ids_at + n_ids;
  if (paydw > KSG_SRV_PAY_DW) return false;
  uint32_t* req = ctl ? c->srv_box->creq : c->srv_box->req;
  uint32_t* xa = ctl ? c->srv_box->cext : c->srv_box->ext;
  auto put = [&](uint32_t i, uint32_t v) {  // payload dword i
    if (i < KSG_SRV_INLINE_DW) {
      const uint32_t j = KSG_SRV_HDR_DW + i;
      req[4 * (j / KSG_SRV_CHUNK_DW) + j % KSG_SRV_CHUNK_DW] = v;
    } else {
      xa[i - KSG_SRV_INLINE_DW] = v;
    }
  };
  const uint32_t* pw = reinterpret_cast<const uint32_t*>(pod);
  for (uint32_t i = 0; i < pod_dw; ++i) put(i, pw[i]);
  for (uint32_t i = 0; i < n_ids; ++i) put(ids_at + i, ids[i]);
  if (ext) {
    const uint32_t* ew = reinterpret_cast<const uint32_t*>(ext);
    for (uint32_t i = 0; i < ext_dw; ++i) put(ext_at + i, ew[i]);
  }
  hdr[KSG_SRVH_PAYDW] = (uint32_t)paydw;
  hdr[KSG_SRVH_IDS_AT] = ids_at;
  hdr[KSG_SRVH_EXT_AT] = ext_at;
  if (ext) hdr[KSG_SRVH_FLAGS] |= KSG_SRVF_EXT;
  return true;
}

// ---- the read-only batch queries' frame (ksg_host.h) --------------------------
int query_enter(ksg_ctx* c, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids, uint32_t n_ids, double* last_ms) {
  if (c->pending) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
  if (ext && !c->ext_on) return fail(c, KSG_ERR_STATE, "extensions are off");
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  if (int rc0 = flush_deferred(c)) return rc0;  // (the mirror now holds the last batch)
  if (int rs = cluster_ok(c)) return rs;
  HIPCHK(c, hipSetDevice(c->device));
  *last_ms = 0.0;
  if (n == 0) return kQueryDone;
  if (c->cl.N == 0) return KSG_NONODES;
  if (n_ids && !ids) return fail(c, KSG_ERR_ARG, "ids missing");
  return KSG_OK;
}

int query_validate(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                   uint32_t n_ids, const std::function<int(uint32_t)>& also) {
  int rc;
  for (uint32_t i = 0; i < n; ++i) {
    if ((rc = check_pod(c, pods + i, ids, n_ids))) return rc;
    if (ext && ((rc = check_ext_range(c, ext + i, n_ids)) || (rc = check_taint_ids(c, ext + i, ids)))) return rc;
    if (also && (rc = also(i))) return rc;
  }
  return KSG_OK;
}

int query_upload(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                 uint32_t n_ids, bool zero_records, const ksg_pod_ext** dext) {
  int rc;
  *dext = nullptr;
  if ((rc = flush_patches(c))) return rc;
  if ((rc = upload_pods(c, pods, n, ids, n_ids))) return rc;
  if (!(ext || (zero_records && c->ext_on))) return KSG_OK;
  if ((rc = c->d_pext.grow(c, n))) return rc;
  if (ext) HIPCHK(c, hipMemcpyAsync(c->d_pext, ext, (size_t)n * sizeof(ksg_pod_ext), hipMemcpyHostToDevice, c->st));
  else HIPCHK(c, hipMemsetAsync(c->d_pext, 0, (size_t)n * sizeof(ksg_pod_ext), c->st));
  *dext = c->d_pext;
  return KSG_OK;
}

uint32_t query_per(size_t budget, size_t bytes_per_pod, uint32_t chunk, uint32_t n) {
  uint32_t per = 1u << 20;  // (the grid's y extent stays far below 65,535)
  if (bytes_per_pod) per = (uint32_t)std::min<size_t>(per, std::max<size_t>(budget / bytes_per_pod, 1));
  if (per > chunk) per -= per % chunk;
  return std::min(per, n);
}

int query_chunks(ksg_ctx* c, uint32_t n, uint32_t per, double* last_ms, const std::function<int(uint32_t, uint32_t)>& launch,
                 const std::function<int(uint32_t, uint32_t, bool)>& copies) {
  int rc;
  if (!c->ev_x0) {
    HIPCHK(c, hipEventCreate(&c->ev_x0));
    HIPCHK(c, hipEventCreate(&c->ev_x1));
  }
  for (uint32_t a = 0; a < n; a += per) {
    const uint32_t m = std::min(per, n - a);
    HIPCHK(c, hipEventRecord(c->ev_x0, c->st));
    if ((rc = launch(a, m))) return rc;
    HIPCHK(c, hipEventRecord(c->ev_x1, c->st));
    if ((rc = copies(a, m, a + per >= n))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));  // (the staging buffers are reused by the next chunk)
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_x0, c->ev_x1));
    *last_ms += ms;
  }
  return KSG_OK;
}

#pragma GCC visibility pop

extern "C" {

int ksg_shard_range(uint32_t n_nodes, int rank, int world, uint32_t* lo, uint32_t* hi) {
  if (world < 1 || rank < 0 || rank >= world || !lo || !hi) return KSG_ERR_ARG;
  uint32_t a, b;
  ksg_shard_words((n_nodes + 63) / 64, (uint32_t)rank, (uint32_t)world, &a, &b);
  *lo = std::min(a * 64, n_nodes);
  *hi = std::min(b * 64, n_nodes);
  return KSG_OK;
}

int ksg_merge_records(const void* records, uint32_t rec_bytes, uint32_t world, uint32_t n_nodes,
                      int empty_priorities, uint64_t* rng_state, uint64_t tie_index, int32_t* out_node,
                      int64_t* max_score, uint64_t* tie_count) {
  if (!records || world < 1 || rec_bytes < sizeof(KsgRecordHdr) || !out_node) return KSG_ERR_ARG;
  const uint8_t* rec = static_cast<const uint8_t*>(records);
  const KsgMerged m = ksg_merge_summary(rec, rec_bytes, world, empty_priorities);
  if (max_score) *max_score = m.max_score;
  if (tie_count) *tie_count = m.tie_count;
  *out_node = -1;
  if (m.error) return KSG_ERR_NOPEER;
  if (m.tie_count == 0) return KSG_NOFIT;
  const uint64_t ix = rng_state ? (ksg_splitmix_next(rng_state) >> 1) % m.tie_count : tie_index % m.tie_count;
  uint64_t lix = 0, kg = 0;
  const int32_t g = ksg_merge_owner(rec, rec_bytes, world, m.max_score, ix, &lix, &kg);
  if (g < 0) return KSG_ERR_ARG;
  uint32_t a, b;
  ksg_shard_words((n_nodes + 63) / 64, (uint32_t)g, world, &a, &b);
  const uint32_t nwords = (rec_bytes - (uint32_t)sizeof(KsgRecordHdr)) / 8;
  const uint64_t* words = reinterpret_cast<const uint64_t*>(rec + (size_t)g * rec_bytes + sizeof(KsgRecordHdr));
  // the lix-th tie from the top = the (kg-1-lix)-th set bit from the bottom
  uint64_t target = kg - 1 - lix;
  for (uint32_t w = 0; w < std::min(nwords, b - a); ++w) {
    uint64_t x = words[w];
    const uint32_t cnt = (uint32_t)__builtin_popcountll(x);
    if (target >= cnt) {
      target -= cnt;
      continue;
    }
    for (; target; --target) x &= x - 1;
    *out_node = (int32_t)((a + w) * 64 + (uint32_t)__builtin_ctzll(x));
    return *out_node < (int32_t)n_nodes ? KSG_OK : KSG_ERR_ARG;
  }
  return KSG_ERR_ARG;  // record's count and bitmap disagree
}

int ksg_nccl_unique_id(void* out128) {
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return KSG_ERR_RCCL;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  memcpy(out128, &id, sizeof id);
  return KSG_OK;
}

static int create_impl(const ksg_config* cfg, int device, int rank, int world, const void* nccl_id,
                       ksg_ctx** out) {
  if (!cfg || !out || world < 1 || rank < 0 || rank >= world) return KSG_ERR_ARG;
  if (cfg->n_anti > KSG_MAX_ANTI || cfg->n_label_pref > KSG_MAX_LABEL_PREF ||
      cfg->n_presence > KSG_MAX_PRESENCE || cfg->n_aff_labels > KSG_MAX_AFF ||
      cfg->n_aff_groups > KSG_MAX_AFF_GROUPS)
    return KSG_ERR_ARG;
  for (uint32_t g = 0; g < cfg->n_aff_groups; ++g)
    if (cfg->aff_group_mask[g] >> cfg->n_aff_labels) return KSG_ERR_ARG;  // a label the config lacks
  for (uint32_t q = 0; q < cfg->n_presence; ++q)
    if (cfg->presence_n_keys[q] > KSG_MAX_PRESENCE_KEYS) return KSG_ERR_ARG;
  ksg_ctx* c = new ksg_ctx();
  c->cfg = *cfg;
  if (c->cfg.max_conflict_keys == 0) c->cfg.max_conflict_keys = 1024;
  if (c->cfg.max_domains == 0) c->cfg.max_domains = 4096;
  c->device = device;
  c->rank = rank;
  c->world = world;
  auto bail = [&](int rc) {
    if (rc != KSG_OK) {
      fprintf(stderr, "ksg_create: %s\n", c->err.c_str());
      delete c;
    }
    return rc;
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return bail(fail(c, KSG_ERR_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e)));
  if ((e = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev0, kTimingEvent)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev1, kTimingEvent)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_wait, hipEventDisableTiming)) != hipSuccess)
    return bail(fail(c, KSG_ERR_HIP, "stream/event: %s", hipGetErrorString(e)));
  c->spin_wait = env_flag("KSG_SPIN_WAIT", true);
  c->srv_enabled = env_flag("KSG_SERVE", true);
  c->srv_stamps = env_flag("KSG_SERVE_STAMPS", false);
  c->srv_debug = env_flag("KSG_SERVE_DEBUG", false);
  c->srv_trace = env_flag("KSG_SERVE_TRACE", false);
  if (const char* go = getenv("KSG_SERVE_GRID_OPTS")) c->srv_grid_opts = (int64_t)strtoul(go, nullptr, 0);
  c->srv_idle_us = (uint64_t)env_int("KSG_SERVE_IDLE_US", (int64_t)c->srv_idle_us, 1, INT64_MAX);
  c->srv_grid_on = env_flag("KSG_SERVE_GRID", true);
  c->srv_grid_min = (uint32_t)env_int("KSG_SERVE_GRID_MIN", c->srv_grid_min, 0, INT32_MAX);
  c->srv_npt4_min = (uint32_t)env_int("KSG_SERVE_GRID_NPT4_MIN", c->srv_npt4_min, 0, INT32_MAX);
  c->srv_grid_ext = env_flag("KSG_SERVE_GRID_EXT", true);
  if (const char* rm = getenv("KSG_ROUND_MARGIN")) c->round_margin = std::min(std::max(atof(rm), 0.5), 4.0);
  // ksg_headroom_batch: the staging budget of the per-node counts (a test knob: a chunk
  // boundary at a small shape) and the quotient's variant (measurements)
  c->headroom_stage = (size_t)env_int("KSG_HEADROOM_STAGE_BYTES", (int64_t)c->headroom_stage, 4, (int64_t)1 << 40);
  c->headroom_div = (int)env_int("KSG_HEADROOM_DIV", c->headroom_div, 0, 2);
  // ksg_explain_without: the staging budget of the per-node codes (the same test knob)
  c->without_stage = (size_t)env_int("KSG_EXPLAIN_WITHOUT_STAGE_BYTES", (int64_t)c->without_stage, 1, (int64_t)1 << 40);
  // ksg_preempt_batch: the staging budget of the tile partials and per-node counts (the same test knob)
  c->preempt_stage = (size_t)env_int("KSG_PREEMPT_STAGE_BYTES", (int64_t)c->preempt_stage, 1, (int64_t)1 << 40);
  // The exchange path (shard scan, all-gather of per-shard records, replicated
  // resolve) runs for world > 1, and for a 1-rank RCCL communicator when the caller
  // passes an nccl_id with world == 1 (RCCL itself exercised on a single GPU).
  c->xchg = world > 1 || nccl_id != nullptr;
  if (c->xchg) {
    if (world > KSG_MAX_WORLD) return bail(fail(c, KSG_ERR_ARG, "world %d > %d", world, KSG_MAX_WORLD));
    if (nccl_id) {  // else: the caller installs a host transport with ksg_set_allgather
      ncclUniqueId id;
      memcpy(&id, nccl_id, sizeof id);
      ncclResult_t r = ncclCommInitRank(&c->comm, world, id, rank);
      if (r != ncclSuccess) return bail(fail(c, KSG_ERR_RCCL, "ncclCommInitRank: %s", ncclGetErrorString(r)));
    }
  }
  int rc;
  c->window = (uint32_t)env_int("KSG_WINDOW", c->window, INT32_MIN, INT32_MAX);
  c->ev_stride = (uint32_t)env_int("KSG_KERNEL_EVENTS", c->ev_stride, 0, INT32_MAX);
  if ((rc = dalloc(c, c->d_rng, 1)) || (rc = dalloc(c, c->d_summary, 4)) || (rc = dalloc(c, c->d_run, 1)))
    return bail(rc);
  if ((e = hipHostMalloc((void**)&c->h_run, sizeof(KsgWinRun), hipHostMallocDefault)) != hipSuccess)
    return bail(fail(c, KSG_ERR_HIP, "hipHostMalloc: %s", hipGetErrorString(e)));
  c->win_fused = env_flag("KSG_FUSED", true);
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 16) cus = 0;
    c->fused_grid = (uint32_t)cus;
    c->fused_grid = (uint32_t)env_int("KSG_FUSED_GRID", c->fused_grid, 9, 4096);
    if (c->fused_grid == 0) c->win_fused = false;
    c->fused_max_words = (uint32_t)env_int("KSG_FUSED_MAX_WORDS", c->fused_max_words, 0, INT32_MAX);
  }
  if ((e = hipMalloc((void**)&c->d_fctl, kFctlBytes)) != hipSuccess ||
      (e = hipHostMalloc((void**)&c->h_fctl, kFctlBytes, hipHostMallocDefault)) != hipSuccess)
    return bail(fail(c, KSG_ERR_HIP, "fused window control: %s", hipGetErrorString(e)));
  memset(c->h_fctl, 0, kFctlBytes);
  *out = c;
  return KSG_OK;
}

int ksg_create(const ksg_config* cfg, int device, ksg_ctx** out) {
  return create_impl(cfg, device, 0, 1, nullptr, out);
}

int ksg_create_sharded(const ksg_config* cfg, int device, int rank, int world, const void* nccl_id,
                       ksg_ctx** out) {
  return create_impl(cfg, device, rank, world, nccl_id, out);
}

int ksg_destroy(ksg_ctx* c) {
  if (!c) return KSG_OK;
  if (c->cl.dev.dbgbuf) {  // debug stamps (KSG_DEBUG & 8): cycles/64 per resolver section
    int32_t h[32];
    (void)hipMemcpy(h, c->cl.dev.dbgbuf, sizeof h, hipMemcpyDeviceToHost);
    fprintf(stderr, "ksg stamps (x64 cycles, committer wave): ring-wait %d head %d recheck-last-slot %d "
            "wait-checkers %d select %d commit %d | drop-path pods %d unpredicted commits %d\n",
            h[0], h[1], h[2], h[3], h[4], h[5], h[7], h[8]);
    fprintf(stderr, "ksg ring-wait split: first 4 pods of each window %d, later pods %d\n", h[10], h[11]);
    fprintf(stderr, "ksg producers (sum over waves): slot-wait %d loads %d draw-wait %d stage %d\n", h[12], h[13],
            h[14], h[15]);
    fprintf(stderr, "ksg stamps raw:");
    for (int q = 0; q < 32; ++q) fprintf(stderr, " %d", h[q]);
    fprintf(stderr, "\n");
  }
  {
    KSG_LOCK(c);  // waits for a call in flight on another thread
    (void)hipSetDevice(c->device);
    (void)srv_stop(c);
  }
  if (c->srv_stamped && srv_grid(c)) {
    const double n = (double)c->srv_stamped;
    fprintf(stderr, "ksg grid serve stamps (10-ns ticks per begin, %llu begins, scan workgroup 0): request seen -> "
            "masks + loads done %.1f, -> eval + part stored %.1f\n",
            (unsigned long long)c->srv_stamped, c->srv_stage[0] / n, c->srv_stage[1] / n);
  } else if (c->srv_stamped) {
    const double n = (double)c->srv_stamped;
    fprintf(stderr, "ksg serve stamps (s_memtime cycles per begin, %llu begins): to-LDS %.0f check %.0f resolve %.0f "
            "scan %.0f reduce %.0f fail-codes %.0f\n", (unsigned long long)c->srv_stamped, c->srv_stage[0] / n,
            c->srv_stage[1] / n, c->srv_stage[2] / n, c->srv_stage[3] / n, c->srv_stage[4] / n, c->srv_stage[5] / n);
  }
  (void)hipSetDevice(c->device);
  if (c->st) (void)hipStreamSynchronize(c->st);
  if (c->comm) ncclCommDestroy(c->comm);
  if (c->h_run) (void)hipHostFree(c->h_run);
  if (c->h_fctl) (void)hipHostFree(c->h_fctl);
  if (c->d_fctl) (void)hipFree(c->d_fctl);
  if (c->h_map) (void)hipHostFree(c->h_map);
  if (c->srv_box) (void)hipHostFree(c->srv_box);
  if (c->srv_grid) (void)hipFree(c->srv_grid);
  if (c->srv_fail) (void)hipHostFree(c->srv_fail);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev_wait) (void)hipEventDestroy(c->ev_wait);
  if (c->ev_x0) (void)hipEventDestroy(c->ev_x0);
  if (c->ev_x1) (void)hipEventDestroy(c->ev_x1);
  for (auto& e : c->wev)
    if (e) (void)hipEventDestroy(e);
  if (c->st) (void)hipStreamDestroy(c->st);
  // (the node list's parts, c->cl, and the scratch buffers free themselves: the device is set and
  // the stream was synchronised above)
  delete c;
  return KSG_OK;
}

const char* ksg_last_error(ksg_ctx* c) { return c ? c->err.c_str() : "null context"; }

static int add_pod_impl(ksg_ctx* c, uint32_t host_id, const ksg_pod* pod, const uint32_t* ids) {
  if (int rc0 = flush_deferred(c)) return rc0;
  if (int rs = cluster_ok(c)) return rs;
  int rc = check_pod(c, pod, ids, pod_ids_extent(pod));
  if (rc) return rc;
  if (host_id < c->cl.N && (rc = note_requests(c, pod, 1))) return rc;
  rc = mirror_add(c, host_id, pod, ids, true);
  if (rc) return rc;
  if (c->patches.size() > 4096) return flush_patches(c);
  return KSG_OK;
}

int remove_pod_impl(ksg_ctx* c, uint64_t uid) {
  if (c->diverged) return cluster_ok(c);
  if (int rc0 = flush_deferred(c)) return rc0;
  auto it = c->pods.find(uid);
  if (it == c->pods.end()) return fail(c, KSG_ERR_ARG, "unknown pod uid %llu", (unsigned long long)uid);
  PodRec r = std::move(it->second);
  c->pods.erase(it);
  const uint32_t h = r.host;
  if (c->ext_on) c->ext_scalar.erase(uid);
  if (h < c->cl.N) {
    c->mir.used_c[h] = (int64_t)((uint64_t)c->mir.used_c[h] - (uint64_t)r.cpu);
    c->mir.used_m[h] = (int64_t)((uint64_t)c->mir.used_m[h] - (uint64_t)r.mem);
    c->mu_dirty = true;
    patch64(c, c->cl.dev.used_cpu + h, c->mir.used_c[h]);
    patch64(c, c->cl.dev.used_mem + h, c->mir.used_m[h]);
    if (c->ext_on)
      for (uint32_t q = 0; q < c->ext.n_scalar; ++q) {
        if (!r.scalar[q]) continue;
        int64_t& u = c->mir.sc_used[(size_t)q * c->cl.N + h];
        u = (int64_t)((uint64_t)u - (uint64_t)r.scalar[q]);
        patch64(c, c->cl.dev.scalar_used + (size_t)q * c->cl.N + h, u);
      }
    for (uint32_t k : r.keys) {
      auto kit = c->mir.key_ref.find(((uint64_t)k << 32) | h);
      if (kit != c->mir.key_ref.end() && --kit->second == 0) {
        c->mir.key_ref.erase(kit);
        patch_andnot(c, c->cl.dev.keymap + (size_t)k * c->cl.nw + (h >> 6), 1ULL << (h & 63));
      }
    }
  }
  for (uint32_t s : r.svcs) {
    int32_t before;
    if (h < c->cl.N) {
      int32_t& v = c->mir.svc_cnt[(size_t)s * c->cl.N + h];
      before = v--;
      patch32(c, c->cl.dev.svc_cnt + (size_t)s * c->cl.N + h, v);
      if (v == 0) patch_andnot(c, c->cl.dev.svc_bits + (size_t)s * c->cl.nw + (h >> 6), 1ULL << (h & 63));
    } else {
      auto& m = c->mir.svc_ext[s];
      before = m[h]--;
      if (m[h] == 0) m.erase(h);
    }
    if (before == c->mir.svc_max[s]) {
      c->mir.svc_max[s] = recompute_max(c, s);
      patch32(c, c->cl.dev.svc_max + s, c->mir.svc_max[s]);
    }
    --c->mir.svc_total[s];
    patch32(c, c->cl.dev.svc_total + s, c->mir.svc_total[s]);
    c->mir.svc_members[s].erase(r.seq);
    const int32_t pc = peer_code(c, s);
    if (pc != c->mir.svc_peer[s]) {
      c->mir.svc_peer[s] = pc;
      patch32(c, c->cl.dev.svc_peer + s, pc);
    }
  }
  if (c->patches.size() > 4096) return flush_patches(c);
  return KSG_OK;
}

// apply the updates queued while a schedule_begin was pending (c->mu held)
static int apply_queued(ksg_ctx* c) {
  std::vector<ksg_ctx::Queued> q;
  q.swap(c->upd_q);
  c->q_added.clear();
  c->q_removed.clear();
  for (auto& u : q) {
    const int rc = u.add ? add_pod_impl(c, u.host, &u.pod, u.ids.data()) : remove_pod_impl(c, u.uid);
    if (rc) return rc;
  }
  return KSG_OK;
}

int ksg_add_pod(ksg_ctx* c, uint32_t host_id, const ksg_pod* pod, const uint32_t* ids) {
  if (!c || !pod) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (c->ext_on && !c->cur_ext) c->ext_scalar.erase(pod->uid);  // (plain entry point: no extension requests)
  HIPCHK(c, hipSetDevice(c->device));  // reflector threads: patches flush on this context's device
  if (!c->pending) return add_pod_impl(c, host_id, pod, ids);
  if (int rs = cluster_ok(c)) return rs;
  const size_t ext = pod_ids_extent(pod);
  int rc = check_pod(c, pod, ids, ext);
  if (rc) return rc;
  const bool live = c->pods.count(pod->uid) && !c->q_removed.count(pod->uid);
  if (live || c->q_added.count(pod->uid) || pod->uid == c->pend.uid)
    return fail(c, KSG_ERR_ARG, "duplicate pod uid %llu", (unsigned long long)pod->uid);
  c->upd_q.push_back({true, host_id, *pod, std::vector<uint32_t>(ids, ids + ext), pod->uid});
  c->q_added.insert(pod->uid);
  c->q_removed.erase(pod->uid);
  return KSG_OK;
}

int ksg_remove_pod(ksg_ctx* c, uint64_t uid) {
  if (!c) return KSG_ERR_ARG;
  KSG_LOCK(c);
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->pending) return remove_pod_impl(c, uid);
  const bool live = (c->pods.count(uid) && !c->q_removed.count(uid)) || c->q_added.count(uid);
  if (!live) return fail(c, KSG_ERR_ARG, "unknown pod uid %llu", (unsigned long long)uid);
  c->upd_q.push_back({false, 0, ksg_pod{}, {}, uid});
  c->q_added.erase(uid);
  c->q_removed.insert(uid);
  return KSG_OK;
}

int ksg_schedule_begin(ksg_ctx* c, const ksg_pod* pod, const uint32_t* ids, int64_t* max_score,
                       uint32_t* tie_count, uint8_t* fail_codes) {
  if (!c || !pod) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (int rc0 = flush_deferred(c)) return rc0;
  if (int rs = cluster_ok(c)) return rs;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pending) {  // the previous begin was abandoned: its queued updates apply now
    c->pending = false;
    c->pend_srv = false;
    if (int rq = apply_queued(c)) return rq;
  }
  if (c->cl.N == 0) return KSG_NONODES;
  if (c->ext_on && !c->cur_ext) c->ext_scalar.erase(pod->uid);  // (plain entry point: no extension requests)
  const size_t ext = call_ids_extent(c, pod);
  int rc = check_pod(c, pod, ids, ext);
  if (rc) return rc;
  if ((rc = note_requests(c, pod, 1))) return rc;
  if (srv_eligible(c)) {  // the resident server: one request, no launch / copy / stream sync
    uint32_t hdr[KSG_SRV_HDR_DW] = {KSG_SRV_BEGIN};
    if ((rc = srv_alloc(c))) return rc;
    // (an all-zero record for the plain entry point of an extensions context)
    static const ksg_pod_ext zero_ext{};
    const ksg_pod_ext* xr = c->ext_on ? (c->cur_ext ? c->cur_ext : &zero_ext) : nullptr;
    // ServiceAffinity (predicates.go:257-324): the labels the pod's nodeSelector does not give come
    // from its service's first peer's node; resolved here from the host mirror (svc_peer, kept equal
    // to the device's) so the scan workgroups skip that dependent chain (pod_resolve then finds
    // every requirement given; an unlabelled peer leaves -1, which it resolves to the same -1)
    ksg_pod rp;
    const ksg_pod* sp = pod;
    if (!c->cl.h_aff_pair.empty() && pod->service >= 0 && (uint32_t)pod->service < c->cl.S) {
      const int32_t peer = c->mir.svc_peer[pod->service];
      bool given = true;
      for (uint32_t j = 0; j < c->cfg.n_aff_labels && j < KSG_MAX_AFF; ++j) given = given && pod->aff_pair[j] != -1;
      if (!given && peer >= 0 && (uint32_t)peer < c->cl.N) {
        rp = *pod;
        for (uint32_t j = 0; j < c->cfg.n_aff_labels && j < KSG_MAX_AFF; ++j)
          if (rp.aff_pair[j] == -1) rp.aff_pair[j] = c->cl.h_aff_pair[(size_t)j * c->cl.N + (uint32_t)peer];
        sp = &rp;
      }
    }
    if (srv_put_pod(c, sp, ids, ext, xr, hdr)) {
      if ((rc = flush_patches(c)) || (!c->srv_running && (rc = srv_flush_patches(c)))) return rc;
      if (fail_codes) hdr[KSG_SRVH_FLAGS] |= KSG_SRVF_WANT_FAIL;
      uint32_t r[4];
      if ((rc = srv_begin(c, hdr, r))) return rc;
      // (the last COMMIT was served before this BEGIN: a rejected one diverged the context)
      if ((rc = srv_settle(c))) return rc;
      if (r[1] == KSG_SRV_BADREQ) return fail(c, KSG_ERR_STATE, "drop-in server rejected begin request");
      if (r[1] == ~0u) return fail(c, KSG_ERR_NOPEER, "service affinity peer is not on a known node");
      if (fail_codes) memcpy(fail_codes, c->srv_fail, (size_t)(c->cl.hi - c->cl.lo));
      const int64_t m = (int64_t)((uint64_t)r[2] | ((uint64_t)r[3] << 32));
      if (max_score) *max_score = r[1] > 0 ? m : 0;
      if (tie_count) *tie_count = r[1];
      if (r[1] == 0) return KSG_NOFIT;
      c->pending = true;
      c->pending_k = r[1];
      c->pend = *pod;
      c->pend_ids.assign(ids, ids + ext);
      c->pend_srv = true;
      memcpy(c->srv_bhdr, hdr, sizeof hdr);
      c->srv_pext_on = xr != nullptr;
      if (xr) c->srv_pext = *xr;
      return KSG_OK;
    }
  }
  if ((rc = srv_stop(c))) return rc;
  if ((rc = flush_patches(c))) return rc;
  if ((rc = ensure_map(c)) || (rc = upload_one(c, pod, ids, ext))) return rc;
  if ((rc = scan_exchange(c, c->one_pod, c->one_ids, KSG_MODE_BEGIN, fail_codes ? c->cl.d_fail : nullptr, nullptr,
                          c->ext_on ? c->d_one_ext : nullptr)))
    return rc;
  HIPCHK(c, ksg_launch_decide(c->cl.dev, c->one_pod, c->one_ids, rec_buf(c), c->cl.rec_bytes, c->world,
                              c->cl.d_shard_wlo, 0, 0, c->d_rng, nullptr, 0, reinterpret_cast<int64_t*>(c->d_map),
                              c->st));
  int64_t summ[3];
  const size_t nf = fail_codes ? (size_t)(c->cl.hi - c->cl.lo) : 0;
  if (nf) {
    if ((rc = c->h_dn.grow(c, nf))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->h_dn, c->cl.d_fail, nf, hipMemcpyDeviceToHost, c->st));
  }
  HIPCHK(c, hipStreamSynchronize(c->st));
  memcpy(summ, c->h_map, sizeof summ);
  if (nf) memcpy(fail_codes, c->h_dn, nf);
  if (summ[2]) return fail(c, KSG_ERR_NOPEER, "service affinity peer is not on a known node");
  if (max_score) *max_score = summ[1] > 0 ? summ[0] : 0;
  if (tie_count) *tie_count = (uint32_t)summ[1];
  if (summ[1] == 0) return KSG_NOFIT;
  c->pending = true;
  c->pending_k = (uint64_t)summ[1];
  c->pend = *pod;
  c->pend_ids.assign(ids, ids + ext);
  return KSG_OK;
}

// the device half of a commit: decide the tie_index-th tie and apply AssumePod's delta
static int commit_on_device(ksg_ctx* c, uint32_t tie_index, int32_t* node) {
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pend_srv) {  // served by the resident server
    c->pend_srv = false;
    // the tie_index-th tie from the top (generic_scheduler.go:88-95) from the begin's tie words
    const int64_t off = srv_pick(c->srv_tw, c->pending_k - 1 - tie_index);
    if (off < 0 || off >= (int64_t)(c->cl.hi - c->cl.lo)) return fail(c, KSG_ERR_STATE, "commit selected no node");
    *node = (int32_t)(c->cl.lo + (uint32_t)off);
    // AssumePod's delta: one control request carrying the pod, not waited for (the next
    // BEGIN's scan waits on the device until it is applied)
    uint32_t hdr[KSG_SRV_HDR_DW] = {KSG_SRV_COMMIT};
    if (int rc = srv_settle(c)) return rc;  // (the control block is free)
    if (!srv_put_pod(c, &c->pend, c->pend_ids.data(), c->pend_ids.size(), c->srv_pext_on ? &c->srv_pext : nullptr,
                     hdr, true))
      return fail(c, KSG_ERR_STATE, "pending pod does not fit the request block");
    hdr[KSG_SRVH_ARG] = (uint32_t)*node;
    if (c->srv_trace) fprintf(stderr, "srv commit node %d\n", *node);
    uint32_t seq = 0;
    if (int rc = srv_post(c, hdr, &seq)) return rc;
    c->srv_unacked = seq;
    return KSG_OK;
  }
  int rc = ensure_map(c);
  if (rc) return rc;
  if ((rc = srv_stop(c))) return rc;
  // the pending pod is still in d_one (begin's upload; nothing re-uploads before the commit)
  HIPCHK(c, ksg_launch_decide(c->cl.dev, c->one_pod, c->one_ids, rec_buf(c), c->cl.rec_bytes, c->world,
                              c->cl.d_shard_wlo, 2, tie_index, c->d_rng, reinterpret_cast<int32_t*>(c->d_map + 32), 0,
                              c->d_summary, c->st, c->ext_on ? c->d_one_ext : nullptr));
  HIPCHK(c, hipStreamSynchronize(c->st));
  memcpy(node, c->h_map + 32, 4);
  if (*node < 0) return fail(c, KSG_ERR_STATE, "commit selected no node (%d)", *node);
  return KSG_OK;
}

int ksg_schedule_commit(ksg_ctx* c, uint32_t tie_index, int32_t* out_node) {
  if (!c) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (!c->pending) return fail(c, KSG_ERR_STATE, "no schedule_begin pending");
  if (tie_index >= c->pending_k) return fail(c, KSG_ERR_ARG, "tie_index %u >= tie_count %llu", tie_index,
                                             (unsigned long long)c->pending_k);
  int32_t node = -1;
  int rc = commit_on_device(c, tie_index, &node);
  c->pending = false;
  if (rc == KSG_OK) rc = mirror_add(c, (uint32_t)node, &c->pend, c->pend_ids.data(), false);
  c->pend.uid = ~0ULL;
  // the updates queued while the begin was pending apply now, whatever the outcome
  const int rq = apply_queued(c);
  if (rc) return rc;
  if (rq) return rq;
  if (out_node) *out_node = node;
  return KSG_OK;
}

int ksg_evaluate(ksg_ctx* c, const ksg_pod* pod, const uint32_t* ids, uint8_t* fail_out, int64_t* score_out) {
  if (!c || !pod) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (c->pending) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  if (int rc0 = flush_deferred(c)) return rc0;
  if (int rs = cluster_ok(c)) return rs;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->cl.N == 0) return KSG_NONODES;
  const size_t ext = call_ids_extent(c, pod);
  int rc = check_pod(c, pod, ids, ext);
  if (rc) return rc;
  if ((rc = note_requests(c, pod, 1))) return rc;
  if ((rc = flush_patches(c))) return rc;
  if ((rc = upload_one(c, pod, ids, ext))) return rc;
  // errors surface through the BEGIN record, so run BEGIN first for the flag
  if ((rc = scan_exchange(c, c->one_pod, c->one_ids, KSG_MODE_BEGIN, nullptr, nullptr, c->ext_on ? c->d_one_ext : nullptr)))
    return rc;
  HIPCHK(c, ksg_launch_decide(c->cl.dev, c->one_pod, c->one_ids, rec_buf(c), c->cl.rec_bytes, c->world,
                              c->cl.d_shard_wlo, 0, 0, c->d_rng, nullptr, 0, c->d_summary, c->st));
  if ((rc = scan_exchange(c, c->one_pod, c->one_ids, KSG_MODE_EVAL, c->cl.d_fail, c->cl.d_score, c->ext_on ? c->d_one_ext : nullptr)))
    return rc;
  int64_t summ[3];
  HIPCHK(c, hipMemcpyAsync(summ, c->d_summary, sizeof summ, hipMemcpyDeviceToHost, c->st));
  const size_t ns = c->cl.hi - c->cl.lo;
  if (fail_out && ns) HIPCHK(c, hipMemcpyAsync(fail_out, c->cl.d_fail, ns, hipMemcpyDeviceToHost, c->st));
  if (score_out && ns) HIPCHK(c, hipMemcpyAsync(score_out, c->cl.d_score, ns * 8, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  if (summ[2]) return fail(c, KSG_ERR_NOPEER, "service affinity peer is not on a known node");
  return KSG_OK;
}

int ksg_set_allgather(ksg_ctx* c, ksg_allgather_fn fn, void* user) {
  if (!c) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (c->comm) return fail(c, KSG_ERR_STATE, "context already exchanges over RCCL");
  c->xfn = fn;
  c->xuser = user;
  return KSG_OK;
}

int ksg_serve_stats(ksg_ctx* c, uint64_t* out4) {
  if (!c || !out4) return KSG_ERR_ARG;
  KSG_LOCK(c);
  out4[0] = c->srv_launches;
  out4[1] = c->srv_seq;
  out4[2] = c->srv_running ? 1 : 0;
  out4[3] = srv_eligible(c) ? (srv_grid(c) ? 2 : 1) : 0;
  return KSG_OK;
}

int ksg_debug_counters(ksg_ctx* c, int32_t* out, uint32_t n_words) {
  if (!c || (!out && n_words)) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  if (!c->cl.dev.dbgbuf) return fail(c, KSG_ERR_STATE, "debug counters need KSG_DEBUG=8 at ksg_create");
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->st));
  int32_t words[KSG_DEBUG_COUNTER_WORDS];
  HIPCHK(c, hipMemcpy(words, c->cl.dev.dbgbuf, sizeof(words), hipMemcpyDeviceToHost));
  for (uint32_t k = 0; k < n_words; ++k) out[k] = k < KSG_DEBUG_COUNTER_WORDS ? words[k] : 0;
  return KSG_OK;
}

int ksg_shard(ksg_ctx* c, uint32_t* lo, uint32_t* hi) {
  if (!c) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (lo) *lo = c->cl.lo;
  if (hi) *hi = c->cl.hi;
  return KSG_OK;
}

int ksg_read_requested(ksg_ctx* c, int64_t* milli_cpu, int64_t* memory) {
  if (!c || !c->have_cluster) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  HIPCHK(c, hipSetDevice(c->device));
  int rc = flush_patches(c);
  if (rc) return rc;
  if (c->cl.N) {
    if (milli_cpu) HIPCHK(c, hipMemcpyAsync(milli_cpu, c->cl.dev.used_cpu, c->cl.N * 8, hipMemcpyDeviceToHost, c->st));
    if (memory) HIPCHK(c, hipMemcpyAsync(memory, c->cl.dev.used_mem, c->cl.N * 8, hipMemcpyDeviceToHost, c->st));
  }
  HIPCHK(c, hipStreamSynchronize(c->st));
  return KSG_OK;
}

// The rest of the mutable per-node state, as the device holds it: like ksg_read_requested,
// and on purpose without flush_deferred (the host mirror's opinion is not what is read).
int ksg_read_state(ksg_ctx* c, uint64_t* keymap, int32_t* svc_cnt, uint64_t* svc_bits, int32_t* svc_max,
                   int32_t* svc_total, int32_t* svc_peer) {
  if (!c || !c->have_cluster) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  HIPCHK(c, hipSetDevice(c->device));
  int rc = flush_patches(c);
  if (rc) return rc;
  const size_t K = c->cfg.max_conflict_keys, S = c->cl.S, N = c->cl.N, nw = c->cl.nw;
  auto out = [&](void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->st) : hipSuccess;
  };
  HIPCHK(c, out(keymap, c->cl.dev.keymap, K * nw * 8));
  HIPCHK(c, out(svc_cnt, c->cl.dev.svc_cnt, S * N * 4));
  HIPCHK(c, out(svc_bits, c->cl.dev.svc_bits, S * nw * 8));
  HIPCHK(c, out(svc_max, c->cl.dev.svc_max, S * 4));
  HIPCHK(c, out(svc_total, c->cl.dev.svc_total, S * 4));
  HIPCHK(c, out(svc_peer, c->cl.dev.svc_peer, S * 4));
  HIPCHK(c, hipStreamSynchronize(c->st));
  return KSG_OK;
}

// ---- kubelet admission (ksg_admit.hip) ------------------------------------
static int admit_impl(ksg_ctx* c, int mode, const ksg_admission_set* sets, uint32_t n_sets, const ksg_pod* pods,
                      uint32_t n_pods, const uint32_t* ids, uint32_t n_ids, const uint32_t* pairs, uint32_t n_pairs,
                      uint8_t* out) {
  if (!c || (n_sets && !sets) || (n_pods && (!pods || !out))) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  for (uint32_t s = 0; s < n_sets; ++s) {
    if ((uint64_t)sets[s].pod_off + sets[s].n_pods > n_pods)
      return fail(c, KSG_ERR_ARG, "admission set %u: pods out of range", s);
    if ((mode & KSG_ADMIT_MODE_SELECTOR) && (uint64_t)sets[s].label_off + sets[s].n_labels > n_pairs)
      return fail(c, KSG_ERR_ARG, "admission set %u: labels out of range", s);
  }
  if (mode & KSG_ADMIT_MODE_SELECTOR) {
    if ((n_ids && !ids) || (n_pairs && !pairs)) return fail(c, KSG_ERR_ARG, "admission: ids / pairs == NULL");
    for (uint32_t i = 0; i < n_pods; ++i)
      if ((uint64_t)pods[i].sel_off + pods[i].n_sel > n_ids)
        return fail(c, KSG_ERR_ARG, "pod %u: nodeSelector ids out of range", i);
  }
  // each pod in at most one set (one kernel lane per set writes its pods' results)
  std::vector<uint8_t> in_set(n_pods, 0);
  for (uint32_t s = 0; s < n_sets; ++s)
    for (uint32_t k = 0; k < sets[s].n_pods; ++k)
      if (in_set[sets[s].pod_off + k]++)
        return fail(c, KSG_ERR_ARG, "admission sets %u and an earlier one share pod %u", s, sets[s].pod_off + k);
  for (uint32_t i = 0; i < n_pods; ++i) out[i] = KSG_ADMIT_OK;  // pods in no set
  if (n_sets == 0 || n_pods == 0) return KSG_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const bool sel = (mode & KSG_ADMIT_MODE_SELECTOR) != 0;
  const size_t b_sets = (size_t)n_sets * sizeof(ksg_admission_set), b_pods = (size_t)n_pods * sizeof(ksg_pod);
  const size_t b_ids = sel ? (size_t)n_ids * 4 : 0, b_pairs = sel ? (size_t)n_pairs * 4 : 0;
  const size_t o_pods = (b_sets + 15) & ~(size_t)15, o_ids = o_pods + ((b_pods + 15) & ~(size_t)15);
  const size_t o_pairs = o_ids + ((b_ids + 15) & ~(size_t)15), o_out = o_pairs + ((b_pairs + 15) & ~(size_t)15);
  const size_t total = o_out + n_pods;
  int rc;
  if ((rc = c->d_admit.grow(c, total))) return rc;
  if ((rc = c->h_up.grow(c, o_out))) return rc;
  memcpy(c->h_up, sets, b_sets);
  memcpy(c->h_up + o_pods, pods, b_pods);
  if (b_ids) memcpy(c->h_up + o_ids, ids, b_ids);
  if (b_pairs) memcpy(c->h_up + o_pairs, pairs, b_pairs);
  HIPCHK(c, hipMemcpyAsync(c->d_admit, c->h_up, o_out, hipMemcpyHostToDevice, c->st));
  HIPCHK(c, ksg_launch_admit(reinterpret_cast<const ksg_admission_set*>(c->d_admit.p), n_sets,
                             reinterpret_cast<const ksg_pod*>(c->d_admit + o_pods),
                             reinterpret_cast<const uint32_t*>(c->d_admit + o_ids),
                             reinterpret_cast<const uint32_t*>(c->d_admit + o_pairs), mode, c->d_admit + o_out, c->st));
  if ((rc = c->h_dn.grow(c, n_pods))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_dn, c->d_admit + o_out, n_pods, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  // pods outside every set keep KSG_ADMIT_OK; the kernel wrote the others
  for (uint32_t i = 0; i < n_pods; ++i)
    if (in_set[i]) out[i] = c->h_dn[i];
  return KSG_OK;
}

// ---- extensions (include/kschedgpu.h; parity unpinned) ----------------------
int ksg_set_extensions(ksg_ctx* c, const ksg_ext_config* e) {
  if (!c || !e) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (c->have_cluster) return fail(c, KSG_ERR_STATE, "ksg_set_extensions: call before ksg_set_cluster");
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  if ((e->filters & ~(KSG_EXT_TAINTS | KSG_EXT_SCALAR)) || e->n_scalar > KSG_MAX_SCALAR)
    return fail(c, KSG_ERR_ARG, "extensions: bad filters / n_scalar");
  c->ext = *e;
  c->ext_on = e->filters || e->w_taint_toleration || e->w_balanced || e->n_scalar;
  return KSG_OK;
}

// validate a pod's extension record against the call's id array and record its
// extended-resource requests by uid (the host mirror's AssumePod/remove)
int check_ext_range(ksg_ctx* c, const ksg_pod_ext* e, size_t n_ids) {
  if ((size_t)e->hard_off + e->n_hard > n_ids || (size_t)e->soft_off + e->n_soft > n_ids)
    return fail(c, KSG_ERR_ARG, "extension taint list out of range");
  return KSG_OK;
}
int note_ext(ksg_ctx* c, const ksg_pod* p, const ksg_pod_ext* e, size_t n_ids) {
  if (int rc = check_ext_range(c, e, n_ids)) return rc;
  std::array<int64_t, KSG_MAX_SCALAR> sc{};
  bool any = false;
  for (uint32_t q = 0; q < c->ext.n_scalar; ++q) {
    sc[q] = e->scalar[q];
    any |= sc[q] != 0;
  }
  if (any) c->ext_scalar[p->uid] = sc;
  else c->ext_scalar.erase(p->uid);
  return KSG_OK;
}
// a taint list is a set: TaintTolerationPriority counts each untolerated taint of the node once,
// and the window path counts a soft list as a bit mask while the exact kernels count its entries,
// so a repeated id would make the answer depend on the path
static bool has_repeat(const uint32_t* v, uint32_t n) {
  if (n <= 64) {
    for (uint32_t i = 1; i < n; ++i)
      for (uint32_t j = 0; j < i; ++j)
        if (v[i] == v[j]) return true;
    return false;
  }
  std::vector<uint32_t> s(v, v + n);
  std::sort(s.begin(), s.end());
  return std::adjacent_find(s.begin(), s.end()) != s.end();
}
int check_taint_ids(ksg_ctx* c, const ksg_pod_ext* e, const uint32_t* ids) {
  for (uint32_t i = 0; i < e->n_hard; ++i)
    if (ids[e->hard_off + i] >= c->ext.max_taints) return fail(c, KSG_ERR_CAPACITY, "taint id out of range");
  for (uint32_t i = 0; i < e->n_soft; ++i)
    if (ids[e->soft_off + i] >= c->ext.max_taints) return fail(c, KSG_ERR_CAPACITY, "taint id out of range");
  if ((e->n_hard && has_repeat(ids + e->hard_off, e->n_hard)) || (e->n_soft && has_repeat(ids + e->soft_off, e->n_soft)))
    return fail(c, KSG_ERR_ARG, "a taint id repeats in the pod's hard or soft list (each list is a set)");
  return KSG_OK;
}

int ksg_add_pod_ext(ksg_ctx* c, uint32_t host_id, const ksg_pod* pod, const ksg_pod_ext* ext, const uint32_t* ids) {
  if (!c || !pod) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (ext && !c->ext_on) return fail(c, KSG_ERR_STATE, "extensions are off");
  if (c->ext_on) {
    const ksg_pod_ext z{};
    const ksg_pod_ext* e = ext ? ext : &z;
    const size_t n_ids = std::max(pod_ids_extent(pod), std::max<size_t>((size_t)e->hard_off + e->n_hard,
                                                                         (size_t)e->soft_off + e->n_soft));
    if (int rc = note_ext(c, pod, e, n_ids)) return rc;
  }
  c->cur_ext = ext;
  const int rc = ksg_add_pod(c, host_id, pod, ids);
  c->cur_ext = nullptr;
  return rc;
}

int ksg_schedule_begin_ext(ksg_ctx* c, const ksg_pod* pod, const ksg_pod_ext* ext, const uint32_t* ids,
                           int64_t* max_score, uint32_t* tie_count, uint8_t* fail_codes) {
  if (!c || !pod) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (ext && !c->ext_on) return fail(c, KSG_ERR_STATE, "extensions are off");
  c->cur_ext = ext;
  int rc = KSG_OK;
  if (ext) {
    const size_t n_ids = call_ids_extent(c, pod);
    if (!(rc = check_ext_range(c, ext, n_ids)) && !(rc = check_taint_ids(c, ext, ids))) rc = note_ext(c, pod, ext, n_ids);
  }
  if (!rc) rc = ksg_schedule_begin(c, pod, ids, max_score, tie_count, fail_codes);
  c->cur_ext = nullptr;
  return rc;
}

int ksg_evaluate_ext(ksg_ctx* c, const ksg_pod* pod, const ksg_pod_ext* ext, const uint32_t* ids, uint8_t* fail_out,
                     int64_t* score_out) {
  if (!c || !pod) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (ext && !c->ext_on) return fail(c, KSG_ERR_STATE, "extensions are off");
  c->cur_ext = ext;
  int rc = ext ? check_taint_ids(c, ext, ids) : KSG_OK;
  if (!rc) rc = ksg_evaluate(c, pod, ids, fail_out, score_out);
  c->cur_ext = nullptr;
  return rc;
}

// The read-only batch queries, each on the frame ksg_host.h describes (query_enter ...
// query_chunks). None looks at a uid or calls note_requests: no query turns the context to the
// int64 kernels, and later batches take the path they would have taken. A sharded context
// covers the whole (replicated) cluster alone.

// FitError reports for many pods: one grid-wide pass (ksg_explain.hip) per chunk.
int ksg_explain_batch(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                      uint32_t n_ids, uint8_t* codes, uint32_t* hist, uint8_t* err) {
  if (!c || (n && (!pods || !hist || !err))) return KSG_ERR_ARG;
  KSG_LOCK(c);
  int rc;
  if ((rc = query_enter(c, ext, n, ids, n_ids, &c->last_explain_ms))) return rc == kQueryDone ? KSG_OK : rc;
  if ((rc = query_validate(c, pods, ext, n, ids, n_ids))) return rc;
  const ksg_pod_ext* dext;
  if ((rc = query_upload(c, pods, ext, n, ids, n_ids, false, &dext))) return rc;
  // hist and err for the whole call; the per-node codes in a bounded staging buffer, a chunk
  // of pods at a time
  const size_t hb = (size_t)n * KSG_EXPLAIN_SLOTS * sizeof(uint32_t);
  if ((rc = c->d_xhist.grow(c, hb + n))) return rc;
  uint32_t* d_hist = reinterpret_cast<uint32_t*>(c->d_xhist.p);
  uint8_t* d_err = c->d_xhist + hb;
  HIPCHK(c, hipMemsetAsync(c->d_xhist, 0, hb + n, c->st));
  const uint32_t per = query_per(kExplainStageBytes, codes ? c->cl.N : 0, KSG_EXPLAIN_CHUNK, n);
  if (codes && (rc = c->d_xcodes.grow(c, (size_t)per * c->cl.N))) return rc;
  const auto launch = [&](uint32_t a, uint32_t m) {
    HIPCHK(c, ksg_launch_explain(c->cl.dev, c->d_pods + a, dext ? dext + a : nullptr, c->d_ids, m,
                                 codes ? c->d_xcodes : nullptr, d_hist + (size_t)a * KSG_EXPLAIN_SLOTS, d_err + a, c->st));
    return KSG_OK;
  };
  const auto copies = [&](uint32_t a, uint32_t m, bool last) {
    if (codes)
      HIPCHK(c, hipMemcpyAsync(codes + (size_t)a * c->cl.N, c->d_xcodes, (size_t)m * c->cl.N, hipMemcpyDeviceToHost, c->st));
    if (last) {  // straight into the caller's arrays
      HIPCHK(c, hipMemcpyAsync(hist, d_hist, hb, hipMemcpyDeviceToHost, c->st));
      HIPCHK(c, hipMemcpyAsync(err, d_err, n, hipMemcpyDeviceToHost, c->st));
    }
    return KSG_OK;
  };
  return query_chunks(c, n, per, &c->last_explain_ms, std::cref(launch), std::cref(copies));
}

int ksg_last_explain_ms(ksg_ctx* c, double* ms) {
  if (!c || !ms) return KSG_ERR_ARG;
  KSG_LOCK(c);
  *ms = c->last_explain_ms;
  return KSG_OK;
}

// Ranked hosts for many pods: the grid-wide reduce / score / merge passes of ksg_prioritize.hip
// per chunk. Scores are always wrapping int64.
int ksg_prioritize_batch(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                         uint32_t n_ids, uint32_t top, int64_t* max_score, uint32_t* tie_count, uint32_t* fit_count,
                         int32_t* top_nodes, int64_t* top_scores, int64_t* scores, uint8_t* err) {
  if (!c || (n && (!pods || !max_score || !tie_count || !fit_count || !err))) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (top > KSG_PRIO_MAX_TOP) return fail(c, KSG_ERR_ARG, "top %u > KSG_PRIO_MAX_TOP", top);
  if (n && top && (!top_nodes || !top_scores)) return fail(c, KSG_ERR_ARG, "top > 0 needs top_nodes and top_scores");
  int rc;
  if ((rc = query_enter(c, ext, n, ids, n_ids, &c->last_prioritize_ms))) return rc == kQueryDone ? KSG_OK : rc;
  if ((rc = query_validate(c, pods, ext, n, ids, n_ids))) return rc;
  const ksg_pod_ext* dext;  // (no records: all-zero ones, which is what ksg_evaluate scores a plain pod with)
  if ((rc = query_upload(c, pods, ext, n, ids, n_ids, true, &dext))) return rc;
  // the per-pod results of the whole call: int64 max[n], int64 top_scores[n][top], uint32 ties[n],
  // uint32 fit[n], int32 top_nodes[n][top], uint8 err[n]
  const size_t o_ts = (size_t)n * 8, o_tie = o_ts + (size_t)n * top * 8, o_fit = o_tie + (size_t)n * 4;
  const size_t o_tn = o_fit + (size_t)n * 4, o_err = o_tn + (size_t)n * top * 4, ob = o_err + n;
  if ((rc = c->d_pout.grow(c, ob)) || (rc = c->h_dn.grow(c, ob))) return rc;
  uint8_t* const po = c->d_pout;
  // pods per launch: the normalised terms, tile partials and candidates of a chunk, and its
  // per-node scores where asked for, each within the staging budget
  const size_t T = (c->cl.nw + KSG_PRIO_WAVES - 1) / KSG_PRIO_WAVES, D1 = (size_t)c->cl.dev.n_domains_total + 1;
  const size_t bpp = D1 * 4 + T * (sizeof(KsgPrioPart) + (size_t)top * 12);
  const uint32_t per = query_per(kExplainStageBytes, scores ? std::max(bpp, (size_t)c->cl.N * 8) : bpp, KSG_EXPLAIN_CHUNK, n);
  const size_t o_part = ((size_t)per * D1 * 4 + 15) & ~(size_t)15, o_cs = o_part + (size_t)per * T * sizeof(KsgPrioPart);
  const size_t o_cn = o_cs + (size_t)per * T * top * 8;
  if ((rc = c->d_ppart.grow(c, o_cn + (size_t)per * T * top * 4))) return rc;
  if (scores && (rc = c->d_pscores.grow(c, (size_t)per * c->cl.N))) return rc;
  int32_t* const dnorm = reinterpret_cast<int32_t*>(c->d_ppart.p);
  KsgPrioPart* const part = reinterpret_cast<KsgPrioPart*>(c->d_ppart + o_part);
  int64_t* const cs = reinterpret_cast<int64_t*>(c->d_ppart + o_cs);
  int32_t* const cn = reinterpret_cast<int32_t*>(c->d_ppart + o_cn);
  const bool reduce = ksg_prio_needs_reduce(c->cl.dev, ext != nullptr);
  const auto launch = [&](uint32_t a, uint32_t m) {
    const ksg_pod_ext* xa = dext ? dext + a : nullptr;
    HIPCHK(c, hipMemsetAsync(dnorm, 0, (size_t)m * D1 * 4, c->st));
    if (reduce) HIPCHK(c, ksg_launch_prio_reduce(c->cl.dev, c->d_pods + a, xa, c->d_ids, m, dnorm, c->st));
    HIPCHK(c, ksg_launch_prio_score(c->cl.dev, c->d_pods + a, xa, c->d_ids, m, top, dnorm,
                                    scores ? c->d_pscores.p : nullptr, part, cs, cn, po + o_err + a, c->st));
    HIPCHK(c, ksg_launch_prio_merge(c->cl.dev, m, top, part, cs, cn, reinterpret_cast<int64_t*>(po) + a,
                                    reinterpret_cast<uint32_t*>(po + o_tie) + a, reinterpret_cast<uint32_t*>(po + o_fit) + a,
                                    reinterpret_cast<int32_t*>(po + o_tn) + (size_t)a * top,
                                    reinterpret_cast<int64_t*>(po + o_ts) + (size_t)a * top, c->st));
    return KSG_OK;
  };
  const auto copies = [&](uint32_t a, uint32_t m, bool last) {
    if (scores)
      HIPCHK(c, hipMemcpyAsync(scores + (size_t)a * c->cl.N, c->d_pscores, (size_t)m * c->cl.N * 8, hipMemcpyDeviceToHost, c->st));
    if (last) HIPCHK(c, hipMemcpyAsync(c->h_dn, po, ob, hipMemcpyDeviceToHost, c->st));
    return KSG_OK;
  };
  rc = query_chunks(c, n, per, &c->last_prioritize_ms, std::cref(launch), std::cref(copies));
  if (rc) return rc;
  memcpy(max_score, c->h_dn, (size_t)n * 8);
  memcpy(tie_count, c->h_dn + o_tie, (size_t)n * 4);
  memcpy(fit_count, c->h_dn + o_fit, (size_t)n * 4);
  if (top) {
    memcpy(top_scores, c->h_dn + o_ts, (size_t)n * top * 8);
    memcpy(top_nodes, c->h_dn + o_tn, (size_t)n * top * 4);
  }
  memcpy(err, c->h_dn + o_err, n);
  return KSG_OK;
}

int ksg_last_prioritize_ms(ksg_ctx* c, double* ms) {
  if (!c || !ms) return KSG_ERR_ARG;
  KSG_LOCK(c);
  *ms = c->last_prioritize_ms;
  return KSG_OK;
}

// How many copies of each pod every node can take: one grid-wide pass (ksg_headroom.hip) per
// chunk.
int ksg_headroom_batch(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                       uint32_t n_ids, uint32_t limit, uint64_t* total, uint32_t* fit_count, uint32_t* max_count,
                       uint32_t* bind_hist, uint32_t* counts, uint8_t* err) {
  if (!c || (n && (!pods || !total || !fit_count || !max_count || !bind_hist || !err))) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (limit == 0) return fail(c, KSG_ERR_ARG, "limit 0");
  int rc;
  if ((rc = query_enter(c, ext, n, ids, n_ids, &c->last_headroom_ms))) return rc == kQueryDone ? KSG_OK : rc;
  if ((rc = query_validate(c, pods, ext, n, ids, n_ids))) return rc;
  const ksg_pod_ext* dext;
  if ((rc = query_upload(c, pods, ext, n, ids, n_ids, false, &dext))) return rc;
  // the per-pod results of the whole call: uint64 total[n], uint32 max[n], uint32 fit[n],
  // uint32 hist[n][KSG_HEADROOM_SLOTS], uint8 err[n]; the per-node counts in a bounded staging
  // buffer, a chunk of pods at a time
  const size_t o_max = (size_t)n * 8, o_fit = o_max + (size_t)n * 4, o_hist = o_fit + (size_t)n * 4;
  const size_t hb = (size_t)n * KSG_HEADROOM_SLOTS * sizeof(uint32_t), o_err = o_hist + hb, ob = o_err + n;
  if ((rc = c->d_hout.grow(c, ob)) || (rc = c->h_dn.grow(c, ob))) return rc;
  uint8_t* const ho = c->d_hout;
  HIPCHK(c, hipMemsetAsync(ho, 0, ob, c->st));
  const uint32_t per = query_per(c->headroom_stage, counts ? (size_t)c->cl.N * sizeof(uint32_t) : 0, KSG_HEADROOM_CHUNK, n);
  if (counts && (rc = c->d_hcounts.grow(c, (size_t)per * c->cl.N))) return rc;
  const auto launch = [&](uint32_t a, uint32_t m) {
    HIPCHK(c, ksg_launch_headroom(c->cl.dev, c->d_pods + a, dext ? dext + a : nullptr, c->d_ids, m, limit, c->headroom_div,
                                  counts ? c->d_hcounts.p : nullptr, reinterpret_cast<uint64_t*>(ho) + a,
                                  reinterpret_cast<uint32_t*>(ho + o_max) + a, reinterpret_cast<uint32_t*>(ho + o_fit) + a,
                                  reinterpret_cast<uint32_t*>(ho + o_hist) + (size_t)a * KSG_HEADROOM_SLOTS,
                                  ho + o_err + a, c->st));
    return KSG_OK;
  };
  const auto copies = [&](uint32_t a, uint32_t m, bool last) {
    if (counts)
      HIPCHK(c, hipMemcpyAsync(counts + (size_t)a * c->cl.N, c->d_hcounts, (size_t)m * c->cl.N * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, c->st));
    if (last) HIPCHK(c, hipMemcpyAsync(c->h_dn, ho, ob, hipMemcpyDeviceToHost, c->st));
    return KSG_OK;
  };
  rc = query_chunks(c, n, per, &c->last_headroom_ms, std::cref(launch), std::cref(copies));
  if (rc) return rc;
  memcpy(total, c->h_dn, (size_t)n * 8);
  memcpy(max_count, c->h_dn + o_max, (size_t)n * 4);
  memcpy(fit_count, c->h_dn + o_fit, (size_t)n * 4);
  memcpy(bind_hist, c->h_dn + o_hist, hb);
  memcpy(err, c->h_dn + o_err, n);
  return KSG_OK;
}

int ksg_last_headroom_ms(ksg_ctx* c, double* ms) {
  if (!c || !ms) return KSG_ERR_ARG;
  KSG_LOCK(c);
  *ms = c->last_headroom_ms;
  return KSG_OK;
}

int ksg_check_pods_exceeding_capacity(ksg_ctx* c, const ksg_admission_set* sets, uint32_t n_sets,
                                      const ksg_pod* pods, uint32_t n_pods, uint8_t* fits) {
  const int rc = admit_impl(c, KSG_ADMIT_MODE_CAPACITY, sets, n_sets, pods, n_pods, nullptr, 0, nullptr, 0, fits);
  if (rc == KSG_OK)
    for (uint32_t i = 0; i < n_pods; ++i) fits[i] = fits[i] == KSG_ADMIT_OK;
  return rc;
}

int ksg_pod_matches_node_labels(ksg_ctx* c, const ksg_admission_set* sets, uint32_t n_sets, const ksg_pod* pods,
                                uint32_t n_pods, const uint32_t* ids, uint32_t n_ids, const uint32_t* pairs,
                                uint32_t n_pairs, uint8_t* matches) {
  const int rc = admit_impl(c, KSG_ADMIT_MODE_SELECTOR, sets, n_sets, pods, n_pods, ids, n_ids, pairs, n_pairs,
                            matches);
  if (rc == KSG_OK)
    for (uint32_t i = 0; i < n_pods; ++i) matches[i] = matches[i] == KSG_ADMIT_OK;
  return rc;
}

int ksg_admit_pods(ksg_ctx* c, const ksg_admission_set* sets, uint32_t n_sets, const ksg_pod* pods, uint32_t n_pods,
                   const uint32_t* ids, uint32_t n_ids, const uint32_t* pairs, uint32_t n_pairs, uint8_t* codes) {
  return admit_impl(c, KSG_ADMIT_MODE_SELECTOR | KSG_ADMIT_MODE_CAPACITY, sets, n_sets, pods, n_pods, ids, n_ids,
                    pairs, n_pairs, codes);
}

}  // extern "C"
