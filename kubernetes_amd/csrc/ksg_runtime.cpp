// ksg_runtime.cpp — host runtime of libkschedgpu.so: the context's lifetime (ksg_create*,
// ksg_destroy), the device-state mirror with its patches, ksg_add_pod / ksg_remove_pod, the
// RCCL exchange, the read-backs, kubelet admission, the pods' extension records, and the
// helpers ksg_host.h declares for the other host files. Those are: the per-pod path (begin /
// commit / evaluate) with the resident server's client, ksg_dropin.cpp; the read-only queries'
// frame and the three oldest queries, ksg_query.cpp (the newer ones: ksg_without.cpp,
// ksg_preempt.cpp, ksg_pack.cpp); the batch driver, ksg_batch.cpp; the node list, ksg_cluster.cpp.
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

int flush_patches(ksg_ctx* c) {
  if (c->patches.empty()) return KSG_OK;
  if (c->srv.running) return srv_flush_patches(c);
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
  c->pb.clear();
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

size_t pod_ids_extent(const ksg_pod* p) {
  size_t e = 0;
  e = std::max<size_t>(e, (size_t)p->ports_off + p->n_ports);
  e = std::max<size_t>(e, (size_t)p->pds_off + p->n_pds);
  e = std::max<size_t>(e, (size_t)p->sel_off + p->n_sel);
  e = std::max<size_t>(e, (size_t)p->svcs_off + p->n_svcs);
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
  auto bail = [&](int rc) {  // (the half-built context frees what it holds: the owners of ksg_host.h)
    if (rc != KSG_OK) {
      fprintf(stderr, "ksg_create: %s\n", c->err.c_str());
      delete c;
    }
    return rc;
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return bail(fail(c, KSG_ERR_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e)));
  if ((e = hipStreamCreateWithFlags(&c->st.s, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev0.e, kTimingEvent)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev1.e, kTimingEvent)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&c->ev_wait.e, hipEventDisableTiming)) != hipSuccess)
    return bail(fail(c, KSG_ERR_HIP, "stream/event: %s", hipGetErrorString(e)));
  c->spin_wait = env_flag("KSG_SPIN_WAIT", true);
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
      ncclResult_t r = ncclCommInitRank(&c->comm.c, world, id, rank);
      if (r != ncclSuccess) return bail(fail(c, KSG_ERR_RCCL, "ncclCommInitRank: %s", ncclGetErrorString(r)));
    }
  }
  int rc;
  c->window = (uint32_t)env_int("KSG_WINDOW", c->window, INT32_MIN, INT32_MAX);
  c->ev_stride = (uint32_t)env_int("KSG_KERNEL_EVENTS", c->ev_stride, 0, INT32_MAX);
  if ((rc = dalloc(c, c->d_rng, 1)) || (rc = dalloc(c, c->d_summary, 4)) || (rc = dalloc(c, c->d_run, 1)) ||
      (rc = c->h_run.alloc(c, 1)))
    return bail(rc);
  c->win_fused = env_flag("KSG_FUSED", true);
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 16) cus = 0;
    c->fused_grid = (uint32_t)cus;
    c->fused_grid = (uint32_t)env_int("KSG_FUSED_GRID", c->fused_grid, 9, 4096);
    if (c->fused_grid == 0) c->win_fused = false;
    c->fused_max_words = (uint32_t)env_int("KSG_FUSED_MAX_WORDS", c->fused_max_words, 0, INT32_MAX);
  }
  if ((rc = c->d_fctl.grow(c, kFctlBytes)) || (rc = c->h_fctl.alloc(c, kFctlBytes)))
    return bail(fail(c, rc, "fused window control: %s", std::string(c->err).c_str()));
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
  srv_print_stamps(c);
  (void)hipSetDevice(c->device);
  if (c->st) (void)hipStreamSynchronize(c->st);
  // (the members free and destroy themselves, the stream last: the device is set and the
  // stream's work is done)
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
int apply_queued(ksg_ctx* c) {
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
  if (!c->pb.on) return add_pod_impl(c, host_id, pod, ids);
  if (int rs = cluster_ok(c)) return rs;
  const size_t ext = pod_ids_extent(pod);
  int rc = check_pod(c, pod, ids, ext);
  if (rc) return rc;
  const bool live = c->pods.count(pod->uid) && !c->q_removed.count(pod->uid);
  if (live || c->q_added.count(pod->uid) || pod->uid == c->pb.pod.uid)
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
  if (!c->pb.on) return remove_pod_impl(c, uid);
  const bool live = (c->pods.count(uid) && !c->q_removed.count(uid)) || c->q_added.count(uid);
  if (!live) return fail(c, KSG_ERR_ARG, "unknown pod uid %llu", (unsigned long long)uid);
  c->upd_q.push_back({false, 0, ksg_pod{}, {}, uid});
  c->q_added.erase(uid);
  c->q_removed.insert(uid);
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
