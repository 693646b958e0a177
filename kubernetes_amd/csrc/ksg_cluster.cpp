// ksg_cluster.cpp — the node list: ksg_set_cluster and ksg_update_cluster with the builder they
// share (build_cluster fills the context's Cluster, ksg_host.h), the static terms folded into a
// list afterwards (ksg_set_static_terms, ksg_add_static_config) and the node extensions
// (ksg_set_node_ext, ksg_read_ext_used). The helpers it calls are ksg_runtime.cpp's (srv_stop: ksg_dropin.cpp's),
// declared in ksg_host.h.
#include <cmath>
#include <cstring>

#include "ksg_host.h"
#include "ksg_shard.h"

constexpr uint32_t kMaxNodesPerShard = KSG_R_MAX * KSG_NT;

extern "C" {

// ksg_set_cluster's and ksg_update_cluster's checks of the node arrays (n_pairs >= 1)
static int check_nodes(ksg_ctx* c, const ksg_node* nodes, uint32_t n_nodes, const uint32_t* node_pairs,
                       uint32_t n_node_pairs, uint32_t n_pairs) {
  if (n_nodes && !nodes) return fail(c, KSG_ERR_ARG, "nodes == NULL");
  for (uint32_t i = 0; i < n_nodes; ++i) {
    if ((size_t)nodes[i].label_off + nodes[i].n_labels > n_node_pairs)
      return fail(c, KSG_ERR_ARG, "node %u label range out of bounds", i);
    for (uint32_t k = 0; k < nodes[i].n_labels; ++k)
      if (node_pairs[nodes[i].label_off + k] >= n_pairs || node_pairs[nodes[i].label_off + k] == 0)
        return fail(c, KSG_ERR_ARG, "node %u has invalid pair id", i);
  }
  return KSG_OK;
}

// Everything a node list determines, built into the context in fresh allocations: the shard
// geometry, the static tables, zeroed pod-state arrays (svc_peer -1), the scratch sized for the
// shard. The caller has put the previous list's parts away, so c->cl is an empty Cluster; the host
// mirror is not touched.
static int build_cluster(ksg_ctx* c, const ksg_node* nodes, uint32_t n_nodes, const uint32_t* node_pairs,
                         uint32_t n_node_pairs, const uint32_t* pair_keys, uint32_t n_pairs, uint32_t n_services) {
  c->cl.N = n_nodes;
  c->cl.nw = (n_nodes + 63) / 64;
  c->cl.n_pairs = n_pairs;
  c->cl.S = n_services;
  // shard by 64-node words
  c->cl.shard_wlo_h.resize(c->world);
  c->cl.nwords_max = 0;
  uint32_t max_shard_nodes = 0;
  for (int g = 0; g < c->world; ++g) {
    uint32_t a, b;
    ksg_shard_words(c->cl.nw, (uint32_t)g, (uint32_t)c->world, &a, &b);
    c->cl.shard_wlo_h[g] = a;
    c->cl.nwords_max = std::max(c->cl.nwords_max, b - a);
    max_shard_nodes = std::max(max_shard_nodes, std::min(b * 64, n_nodes) - std::min(a * 64, n_nodes));
    if (g == c->rank) {
      c->cl.wlo = a;
      c->cl.nwords = b - a;
      c->cl.lo = std::min(a * 64, n_nodes);
      c->cl.hi = std::min(b * 64, n_nodes);
    }
  }
  if (max_shard_nodes > kMaxNodesPerShard)
    return fail(c, KSG_ERR_CAPACITY, "shard of %u nodes exceeds %u (use more GPUs)", max_shard_nodes,
                kMaxNodesPerShard);
  c->cl.R = pick_R(std::max<uint32_t>(max_shard_nodes, 1));

  // anti-affinity domains: dense index of each pair whose key is the label
  std::vector<int32_t> dom_of_pair((size_t)std::max<uint32_t>(c->cfg.n_anti, 1) * n_pairs, -1);
  c->cl.D = 0;
  KsgDev& d = c->cl.dev;
  d = KsgDev{};
  for (uint32_t a = 0; a < c->cfg.n_anti; ++a) {
    d.anti_dom_off[a] = c->cl.D;
    uint32_t nd = 0;
    for (uint32_t p = 1; p < n_pairs; ++p)
      if ((pair_keys[p] & ~KSG_PAIR_INVALID) == c->cfg.anti_key[a]) dom_of_pair[(size_t)a * n_pairs + p] = (int32_t)nd++;
    c->cl.D += nd;
  }
  if (c->cl.D > c->cfg.max_domains)
    return fail(c, KSG_ERR_CAPACITY, "%u anti-affinity domains > max_domains %u", c->cl.D, c->cfg.max_domains);
  c->cl.lds = (size_t)c->cl.D * sizeof(int32_t);

  auto* owner = &c->cl.allocs.v;
  int rc;
  int64_t *cap_c, *cap_m;
  double *inv_c, *inv_m;
  uint64_t *sfit, *keymap, *pairmap;
  int64_t* sscore;
  int32_t *anti_dom, *aff_pair;
  int64_t* gscore = nullptr;  // (int32 or int64 scores: sized for int64)
  const size_t NN = std::max<uint32_t>(n_nodes, 1);
  if ((rc = dalloc(c, &cap_c, NN, owner)) || (rc = dalloc(c, &cap_m, NN, owner)) ||
      (rc = dalloc(c, &inv_c, NN, owner)) || (rc = dalloc(c, &inv_m, NN, owner)) ||
      (rc = dalloc(c, &d.used_cpu, NN, owner)) || (rc = dalloc(c, &d.used_mem, NN, owner)) ||
      (rc = dalloc(c, &sfit, std::max<uint32_t>(c->cl.nw, 1), owner)) ||
      (rc = dalloc(c, &sscore, NN, owner)) ||
      (rc = dalloc(c, &keymap, (size_t)c->cfg.max_conflict_keys * std::max<uint32_t>(c->cl.nw, 1), owner)) ||
      (rc = dalloc(c, &pairmap, (size_t)n_pairs * std::max<uint32_t>(c->cl.nw, 1), owner)) ||
      (rc = dalloc(c, &d.svc_cnt, (size_t)std::max<uint32_t>(n_services, 1) * NN, owner)) ||
      (rc = dalloc(c, &d.svc_bits, (size_t)std::max<uint32_t>(n_services, 1) * std::max<uint32_t>(c->cl.nw, 1), owner)) ||
      (rc = dalloc(c, &d.svc_max, std::max<uint32_t>(n_services, 1), owner)) ||
      (rc = dalloc(c, &d.svc_total, std::max<uint32_t>(n_services, 1), owner)) ||
      (rc = dalloc(c, &d.svc_peer, std::max<uint32_t>(n_services, 1), owner)) ||
      (rc = dalloc(c, &anti_dom, (size_t)std::max<uint32_t>(c->cfg.n_anti, 1) * NN, owner)) ||
      (rc = dalloc(c, &aff_pair, (size_t)std::max<uint32_t>(c->cfg.n_aff_labels, 1) * NN, owner)) ||
      (c->cl.R > KSG_R_LDS / 2 && (rc = dalloc(c, &gscore, (size_t)c->cl.R * KSG_NT, owner))))
    return rc;
  if (n_services) HIPCHK(c, hipMemsetAsync(d.svc_peer, 0xff, n_services * sizeof(int32_t), c->st));

  // upload nodes + static tables
  std::vector<int64_t> hc(NN, 0), hm(NN, 0);
  c->cl.max_cap = 0;
  c->cl.min_cap = 0;
  for (uint32_t i = 0; i < n_nodes; ++i) {
    hc[i] = nodes[i].cap_milli_cpu;
    hm[i] = nodes[i].cap_memory;
    c->cl.max_cap = std::max<int64_t>(c->cl.max_cap, std::max<int64_t>(std::llabs(hc[i]), std::llabs(hm[i])));
    c->cl.min_cap = std::min<int64_t>(c->cl.min_cap, std::min<int64_t>(hc[i], hm[i]));
  }
  HIPCHK(c, hipMemcpyAsync(cap_c, hc.data(), NN * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipMemcpyAsync(cap_m, hm.data(), NN * 8, hipMemcpyHostToDevice, c->st));
  // correctly rounded on host and device alike (lr_inv10, ksg_device.h)
  std::vector<double> ic(NN, 0.0), im(NN, 0.0);
  for (uint32_t i = 0; i < n_nodes; ++i) {
    ic[i] = hc[i] > 0 ? 10.0 / (double)hc[i] : 0.0;
    im[i] = hm[i] > 0 ? 10.0 / (double)hm[i] : 0.0;
  }
  HIPCHK(c, hipMemcpyAsync(inv_c, ic.data(), NN * 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipMemcpyAsync(inv_m, im.data(), NN * 8, hipMemcpyHostToDevice, c->st));
  ksg_node* dn = nullptr;
  uint32_t *dnp = nullptr, *dpk = nullptr;
  int32_t* ddom = nullptr;
  std::vector<void*> tmp;
  // (the node labels stay with the cluster: ksg_add_static_config reads them)
  if ((rc = dalloc(c, &dn, NN, owner)) || (rc = dalloc(c, &dnp, std::max<uint32_t>(n_node_pairs, 1), owner)) ||
      (rc = dalloc(c, &dpk, n_pairs, owner)) || (rc = dalloc(c, &ddom, dom_of_pair.size(), &tmp)))
    return rc;
  c->cl.d_lbl_nodes = dn;
  c->cl.d_lbl_pairs = dnp;
  c->cl.d_lbl_keys = dpk;
  if (n_nodes) HIPCHK(c, hipMemcpyAsync(dn, nodes, n_nodes * sizeof(ksg_node), hipMemcpyHostToDevice, c->st));
  if (n_node_pairs)
    HIPCHK(c, hipMemcpyAsync(dnp, node_pairs, n_node_pairs * 4, hipMemcpyHostToDevice, c->st));
  std::vector<uint32_t> pk(n_pairs, 0xffffffffu);
  if (pair_keys)
    for (uint32_t p = 1; p < n_pairs; ++p) pk[p] = pair_keys[p];
  HIPCHK(c, hipMemcpyAsync(dpk, pk.data(), n_pairs * 4, hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipMemcpyAsync(ddom, dom_of_pair.data(), dom_of_pair.size() * 4, hipMemcpyHostToDevice, c->st));
  KsgStaticCfg sc{};
  sc.n_presence = c->cfg.n_presence;
  memcpy(sc.presence_n_keys, c->cfg.presence_n_keys, sizeof sc.presence_n_keys);
  memcpy(sc.presence_keys, c->cfg.presence_keys, sizeof sc.presence_keys);
  memcpy(sc.presence_flag, c->cfg.presence_flag, sizeof sc.presence_flag);
  sc.n_pref = c->cfg.n_label_pref;
  memcpy(sc.pref_key, c->cfg.pref_key, sizeof sc.pref_key);
  memcpy(sc.pref_presence, c->cfg.pref_presence, sizeof sc.pref_presence);
  memcpy(sc.w_pref, c->cfg.w_pref, sizeof sc.w_pref);
  sc.w_equal = c->cfg.w_equal;
  sc.n_anti = c->cfg.n_anti;
  memcpy(sc.anti_key, c->cfg.anti_key, sizeof sc.anti_key);
  sc.n_aff = c->cfg.n_aff_labels;
  memcpy(sc.aff_key, c->cfg.aff_key, sizeof sc.aff_key);
  HIPCHK(c, ksg_launch_static(sc, n_nodes, dn, dnp, dpk, ddom, n_pairs, c->cl.nw, sfit, sscore, anti_dom, aff_pair,
                              (unsigned long long*)pairmap, c->st));
  // (ServiceAffinity: a host copy of each node's pair per affinity label, so the drop-in server's
  // BEGIN carries a pod's requirements already resolved from its service's first peer)
  c->cl.h_aff_pair.clear();
  if ((c->cfg.predicates & KSG_PRED_SERVICEAFFINITY) && c->cfg.n_aff_labels > 0 && c->world == 1) {
    c->cl.h_aff_pair.resize((size_t)c->cfg.n_aff_labels * NN);
    HIPCHK(c, hipMemcpyAsync(c->cl.h_aff_pair.data(), aff_pair, c->cl.h_aff_pair.size() * sizeof(int32_t),
                             hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
  }
  // ServiceAntiAffinity re-rank (one anti priority, one rank, few domains, an
  // LDS count per service): the nodes of each domain row, row D = unlabelled
  c->cl.d_zmap = nullptr;
  uint32_t rr_dz = 0;
  if (c->cfg.n_anti == 1 && c->cfg.w_anti[0] != 0 && c->cl.D > 0 && c->cl.D + 1 <= KSG_RR_MAXZ && c->world == 1 &&
      n_services <= KSG_RR_MAXSVC && !(env_int("KSG_DEBUG", 0, INT32_MIN, INT32_MAX) & 2048)) {
    rr_dz = c->cl.D + 1;
    if ((rc = dalloc(c, &c->cl.d_zmap, (size_t)rr_dz * std::max<uint32_t>(c->cl.nw, 1), owner))) return rc;
    HIPCHK(c, ksg_launch_zonemap(n_nodes, anti_dom, c->cl.D, c->cl.nw, c->cl.d_zmap, c->st));
  }
  HIPCHK(c, hipStreamSynchronize(c->st));
  for (void* p : tmp) (void)hipFree(p);

  d.n_nodes = n_nodes;
  d.nw = c->cl.nw;
  d.lo = c->cl.lo;
  d.hi = c->cl.hi;
  d.wlo = c->cl.wlo;
  d.nwords = c->cl.nwords;
  d.n_pairs = n_pairs;
  d.n_services = n_services;
  d.max_keys = c->cfg.max_conflict_keys;
  d.n_domains_total = c->cl.D;
  d.rr_dz = rr_dz;
  d.preds = c->cfg.predicates;
  d.n_aff = (c->cfg.predicates & KSG_PRED_SERVICEAFFINITY) ? c->cfg.n_aff_labels : 0;
  // ServiceAffinity predicates (label groups); none given: one over every label
  d.n_aff_groups = c->cfg.n_aff_groups;
  for (uint32_t g = 0; g < d.n_aff_groups; ++g) d.aff_group_mask[g] = c->cfg.aff_group_mask[g];
  if (d.n_aff_groups == 0 && d.n_aff > 0) {
    d.n_aff_groups = 1;
    d.aff_group_mask[0] = (1u << d.n_aff) - 1u;
  }
  // (extension priorities count as priority configs)
  const bool ext_prio = c->ext_on && (c->ext.w_taint_toleration || c->ext.w_balanced);
  d.equal_fallback = c->cfg.n_priority_configs == 0 && !ext_prio;
  // prioritizeNodes skips weight-0 configs; if every config has weight 0 the
  // HostPriorityList is empty and Schedule returns *FitError.
  bool any_weight = c->cfg.w_least_requested || c->cfg.w_service_spreading || c->cfg.w_equal || ext_prio;
  for (uint32_t a = 0; a < c->cfg.n_anti; ++a) any_weight |= c->cfg.w_anti[a] != 0;
  for (uint32_t q = 0; q < c->cfg.n_label_pref; ++q) any_weight |= c->cfg.w_pref[q] != 0;
  d.empty_priorities = (!d.equal_fallback && !any_weight) ? 1 : 0;
  c->cl.static_mag = 0;  // (ksg_set_static_terms' terms end with the node list they were built for)
  // int64 combined scores (exact kernels) once a |score| could reach KSG_SCORE_BOUND, or with a
  // capacity whose LeastRequested term leaves [0, 10]: negative, or past 2^63 / 10 (the x10 wraps)
  c->cl.lr_wild = c->cl.min_cap < 0 || c->cl.max_cap > INT64_MAX / 10;
  set_wide(c);
  d.w_lr = c->cfg.w_least_requested;
  d.w_spread = c->cfg.w_service_spreading;
  d.n_anti = 0;
  for (uint32_t a = 0; a < c->cfg.n_anti; ++a) {
    d.w_anti[a] = c->cfg.w_anti[a];
    if (c->cfg.w_anti[a]) d.n_anti = a + 1;
  }
  if (d.n_anti == 0) d.n_domains_total = 0;
  bool any_pref = false;
  for (uint32_t q = 0; q < c->cfg.n_label_pref; ++q) any_pref |= c->cfg.w_pref[q] != 0;
  d.has_static_score = (c->cfg.w_equal != 0 || any_pref) ? 1 : 0;
  d.dbg = (int)env_int("KSG_DEBUG", 0, INT32_MIN, INT32_MAX);
  // KSG_DEBUG bit 22 / 23: the next COMMIT / BEGIN posted to the resident server carries an
  // out-of-range payload layout (tests/test_gpu_serve.py: the server must reject it, not fault)
  c->cl.dbg_corrupt = ((uint32_t)d.dbg >> 22) & 3u;
  c->cl.win_d1 = env_flag("KSG_WIN_D1", true);
  if (d.dbg & (8 | 32 | 64)) {  // (32: the plain resolver's inconsistency record, ksg_plain.hip; 64: phase-A stamps)
    (void)hipMalloc((void**)&c->cl.dbgbuf.p, KSG_DEBUG_COUNTER_WORDS * sizeof(int32_t));
    (void)hipMemset(c->cl.dbgbuf.p, 0, KSG_DEBUG_COUNTER_WORDS * sizeof(int32_t));
    d.dbgbuf = c->cl.dbgbuf.p;
  }
  d.has_static_fit = ((c->cfg.predicates & KSG_PRED_LABELSPRESENCE) && c->cfg.n_presence > 0) ? 1 : 0;
  d.cap_cpu = cap_c;
  d.cap_mem = cap_m;
  d.inv10_cpu = inv_c;
  d.inv10_mem = inv_m;
  d.static_fit = sfit;
  d.static_score = sscore;
  d.keymap = keymap;
  d.pairmap = pairmap;
  d.anti_domain = anti_dom;
  d.aff_pair = aff_pair;
  d.score_scratch = gscore;
  if (c->ext_on) {  // extensions: extended resources (allocatable, requested) and taint bitmaps
    int64_t *scap = nullptr, *sused = nullptr;
    uint64_t* tmap = nullptr;
    const size_t nsr = std::max<uint32_t>(c->ext.n_scalar, 1);
    if ((rc = dalloc(c, &scap, nsr * NN, owner)) || (rc = dalloc(c, &sused, nsr * NN, owner)) ||
        (rc = dalloc(c, &tmap, (size_t)std::max<uint32_t>(c->ext.max_taints, 1) * std::max<uint32_t>(c->cl.nw, 1), owner)))
      return rc;
    d.ext_filters = c->ext.filters;
    d.w_taint = c->ext.w_taint_toleration;
    d.w_bal = c->ext.w_balanced;
    d.n_scalar = c->ext.n_scalar;
    d.scalar_cap = scap;
    d.scalar_used = sused;
    d.taintmap = tmap;
    d.ntaint = nullptr;
    if (c->ext.max_taints <= 64) {  // (the window path's TaintToleration term: one mask per node)
      uint64_t* ntm = nullptr;
      if ((rc = dalloc(c, &ntm, NN, owner))) return rc;
      d.ntaint = ntm;
    }
  }
  c->cl.lds = (size_t)d.n_domains_total * sizeof(int32_t);

  // scratch sized for the shard
  c->cl.rec_bytes = (uint32_t)(sizeof(KsgRecordHdr) + (size_t)std::max<uint32_t>(c->cl.nwords_max, 1) * 8);
  if ((rc = dalloc(c, c->cl.d_rec_send, c->cl.rec_bytes)) ||
      (rc = dalloc(c, c->cl.d_rec_recv, (size_t)c->cl.rec_bytes * c->world)) ||
      (rc = dalloc(c, c->cl.d_fail, NN)) || (rc = dalloc(c, c->cl.d_score, NN)) ||
      (rc = dalloc(c, c->cl.d_dpart, (size_t)c->cl.dev.n_domains_total + 1)) ||  // (+ the TaintToleration max)
      (rc = dalloc(c, c->cl.d_dglobal, (size_t)c->cl.dev.n_domains_total + 1)) ||
      (rc = dalloc(c, c->cl.d_shard_wlo, c->world)))
    return rc;
  HIPCHK(c, hipMemcpyAsync(c->cl.d_shard_wlo, c->cl.shard_wlo_h.data(), c->world * 4, hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  return KSG_OK;
}

int ksg_set_cluster(ksg_ctx* c, const ksg_node* nodes, uint32_t n_nodes, const uint32_t* node_pairs,
                    uint32_t n_node_pairs, const uint32_t* pair_keys, uint32_t n_pairs, uint32_t n_services) {
  if (!c) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->st));
  if (n_pairs == 0) n_pairs = 1;  // pair 0 always exists (empty)
  if (int rc = check_nodes(c, nodes, n_nodes, node_pairs, n_node_pairs, n_pairs)) return rc;
  c->cl = Cluster{};  // (the previous list's parts are freed here; a failure below leaves what was built to the next call)
  c->have_cluster = false;
  drop_deferred(c);
  c->diverged = false;
  c->ppw_est = 0.0;
  if (int rc = build_cluster(c, nodes, n_nodes, node_pairs, n_node_pairs, pair_keys, n_pairs, n_services)) return rc;
  reset_mirror(c);
  c->have_cluster = true;
  return KSG_OK;
}

int ksg_set_static_terms(ksg_ctx* c, const uint64_t* fit_words, const int64_t* score, int score_weighted) {
  if (!c || (!fit_words && !score)) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (int rs = cluster_ok(c)) return rs;
  if (c->pb.on) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
  // (a node failing the extra fit words reports KSG_FAIL_LABELSPRESENCE: the config must name it)
  if (fit_words && !(c->cfg.predicates & KSG_PRED_LABELSPRESENCE))
    return fail(c, KSG_ERR_ARG, "ksg_set_static_terms: fit words need KSG_PRED_LABELSPRESENCE in the config");
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t N = c->cl.N, nw = (N + 63) / 64;
  if (N == 0) return KSG_OK;
  // a combined score stays int32 on the fast paths only while every |score| < 2^30
  unsigned __int128 mag = 0;
  if (score)
    for (uint32_t n = 0; n < N; ++n) {
      const unsigned __int128 m = score[n] < 0 ? (unsigned __int128)(0 - (uint64_t)score[n]) : (unsigned __int128)score[n];
      mag = std::max(mag, m);
    }
  uint8_t* tmp = nullptr;
  const size_t fb = fit_words ? (size_t)nw * 8 : 0, sb = score ? (size_t)N * 8 : 0;
  HIPCHK(c, hipMalloc((void**)&tmp, fb + sb));
  if (fit_words) HIPCHK(c, hipMemcpyAsync(tmp, fit_words, fb, hipMemcpyHostToDevice, c->st));
  if (score) HIPCHK(c, hipMemcpyAsync(tmp + fb, score, sb, hipMemcpyHostToDevice, c->st));
  KsgDev& d = c->cl.dev;
  HIPCHK(c, ksg_launch_static_fold(const_cast<uint64_t*>(d.static_fit), const_cast<int64_t*>(d.static_score),
                                   fit_words ? reinterpret_cast<const uint64_t*>(tmp) : nullptr,
                                   score ? reinterpret_cast<const int64_t*>(tmp + fb) : nullptr, nw, N,
                                   d.has_static_fit, d.has_static_score, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  (void)hipFree(tmp);
  if (fit_words) d.has_static_fit = 1;
  if (score) {
    d.has_static_score = 1;
    c->cl.static_mag += mag;
    if (score_weighted) d.empty_priorities = 0;
  }
  set_wide(c);
  return KSG_OK;
}

int ksg_add_static_config(ksg_ctx* c, const ksg_config* extra) {
  if (!c || !extra) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (int rs = cluster_ok(c)) return rs;
  if (c->pb.on) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
  if (extra->n_presence > KSG_MAX_PRESENCE || extra->n_label_pref > KSG_MAX_LABEL_PREF)
    return fail(c, KSG_ERR_ARG, "ksg_add_static_config: more terms than the config's slots");
  for (uint32_t q = 0; q < extra->n_presence; ++q)
    if (extra->presence_n_keys[q] > KSG_MAX_PRESENCE_KEYS)
      return fail(c, KSG_ERR_ARG, "ksg_add_static_config: presence predicate %u has too many keys", q);
  // (a node failing the extra predicates reports KSG_FAIL_LABELSPRESENCE: the config must name it)
  if (extra->n_presence && !(c->cfg.predicates & KSG_PRED_LABELSPRESENCE))
    return fail(c, KSG_ERR_ARG, "ksg_add_static_config: LabelsPresence terms need KSG_PRED_LABELSPRESENCE in the config");
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t N = c->cl.N, nw = (N + 63) / 64;
  if (N == 0 || (extra->n_presence == 0 && extra->n_label_pref == 0)) return KSG_OK;
  KsgStaticCfg sc{};  // (the terms only: no EqualPriority, anti-affinity domains or affinity pairs)
  sc.n_presence = extra->n_presence;
  memcpy(sc.presence_n_keys, extra->presence_n_keys, sizeof sc.presence_n_keys);
  memcpy(sc.presence_keys, extra->presence_keys, sizeof sc.presence_keys);
  memcpy(sc.presence_flag, extra->presence_flag, sizeof sc.presence_flag);
  sc.n_pref = extra->n_label_pref;
  memcpy(sc.pref_key, extra->pref_key, sizeof sc.pref_key);
  memcpy(sc.pref_presence, extra->pref_presence, sizeof sc.pref_presence);
  memcpy(sc.w_pref, extra->w_pref, sizeof sc.w_pref);
  // |the pass's score| <= 10 x sum |w| (Go-int weights: a wrapped sum is still bounded by it)
  unsigned __int128 mag = 0;
  bool weighted = false;
  for (uint32_t q = 0; q < extra->n_label_pref; ++q) {
    const int64_t w = extra->w_pref[q];
    mag += (unsigned __int128)(w < 0 ? 0 - (uint64_t)w : (uint64_t)w) * 10u;
    weighted |= w != 0;
  }
  const bool do_fit = extra->n_presence > 0, do_score = extra->n_label_pref > 0;
  const size_t fb = (size_t)nw * 8;
  // the scratch pair, freed on every path out (an error return included)
  struct Scratch {
    uint8_t* p = nullptr;
    ~Scratch() {
      if (p) (void)hipFree(p);
    }
  } tmp;
  HIPCHK(c, hipMalloc((void**)&tmp.p, fb + (size_t)N * 8));
  uint64_t* xfit = reinterpret_cast<uint64_t*>(tmp.p);
  int64_t* xscore = reinterpret_cast<int64_t*>(tmp.p + fb);
  KsgDev& d = c->cl.dev;
  HIPCHK(c, ksg_launch_static_terms(sc, N, c->cl.d_lbl_nodes, c->cl.d_lbl_pairs, c->cl.d_lbl_keys, c->cl.n_pairs, nw, xfit, xscore,
                                    c->st));
  HIPCHK(c, ksg_launch_static_fold(const_cast<uint64_t*>(d.static_fit), const_cast<int64_t*>(d.static_score),
                                   do_fit ? xfit : nullptr, do_score ? xscore : nullptr, nw, N, d.has_static_fit,
                                   d.has_static_score, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  if (do_fit) d.has_static_fit = 1;
  if (do_score) {
    d.has_static_score = 1;
    c->cl.static_mag += mag;
    if (weighted) d.empty_priorities = 0;
  }
  set_wide(c);
  return KSG_OK;
}

// ---- the node extensions (ksg_set_extensions is ksg_runtime.cpp's) --------------------------
static int node_ext_upload(ksg_ctx* c, uint32_t n_nodes, const int64_t* scalar_cap, const uint32_t* taint_off,
                           const uint32_t* taint_n, const uint32_t* taint_ids, uint32_t n_taint_ids);

int ksg_set_node_ext(ksg_ctx* c, uint32_t n_nodes, const int64_t* scalar_cap, const uint32_t* taint_off,
                     const uint32_t* taint_n, const uint32_t* taint_ids, uint32_t n_taint_ids) {
  if (!c) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (c->pb.on) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  if (!c->ext_on) return fail(c, KSG_ERR_STATE, "ksg_set_node_ext: extensions are off");
  if (!c->have_cluster || n_nodes != c->cl.N) return fail(c, KSG_ERR_ARG, "ksg_set_node_ext: node count != cluster");
  if (int rc0 = flush_deferred(c)) return rc0;
  if (!c->pods.empty()) return fail(c, KSG_ERR_STATE, "ksg_set_node_ext: call before adding pods");
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = node_ext_upload(c, n_nodes, scalar_cap, taint_off, taint_n, taint_ids, n_taint_ids)) return rc;
  c->mir.sc_used.assign((size_t)c->ext.n_scalar * c->cl.N, 0);
  return KSG_OK;
}

// ksg_set_node_ext's arrays into the device tables of the context's node list (n_nodes == N):
// scalar_cap, taintmap, ntaint; scalar_used zeroed
static int node_ext_upload(ksg_ctx* c, uint32_t n_nodes, const int64_t* scalar_cap, const uint32_t* taint_off,
                           const uint32_t* taint_n, const uint32_t* taint_ids, uint32_t n_taint_ids) {
  const size_t NN = std::max<uint32_t>(c->cl.N, 1);
  if (c->ext.n_scalar && n_nodes) {
    if (!scalar_cap) return fail(c, KSG_ERR_ARG, "ksg_set_node_ext: scalar_cap missing");
    HIPCHK(c, hipMemcpyAsync(const_cast<int64_t*>(c->cl.dev.scalar_cap), scalar_cap, (size_t)c->ext.n_scalar * n_nodes * 8,
                             hipMemcpyHostToDevice, c->st));
  }
  std::vector<uint64_t> tm((size_t)std::max<uint32_t>(c->ext.max_taints, 1) * std::max<uint32_t>(c->cl.nw, 1), 0);
  if (taint_off && taint_n)
    for (uint32_t n = 0; n < n_nodes; ++n)
      for (uint32_t i = 0; i < taint_n[n]; ++i) {
        if ((size_t)taint_off[n] + i >= n_taint_ids || !taint_ids) return fail(c, KSG_ERR_ARG, "taint list out of range");
        const uint32_t t = taint_ids[taint_off[n] + i];
        if (t >= c->ext.max_taints) return fail(c, KSG_ERR_CAPACITY, "taint id %u >= max_taints", t);
        tm[(size_t)t * c->cl.nw + (n >> 6)] |= 1ULL << (n & 63);
      }
  HIPCHK(c, hipMemcpyAsync(const_cast<uint64_t*>(c->cl.dev.taintmap), tm.data(), tm.size() * 8, hipMemcpyHostToDevice,
                           c->st));
  if (c->cl.dev.ntaint) {  // the same taints as one mask per node (taint ids < 64)
    std::vector<uint64_t> ntm(std::max<uint32_t>(n_nodes, 1), 0);
    if (taint_off && taint_n)
      for (uint32_t n = 0; n < n_nodes; ++n)
        for (uint32_t i = 0; i < taint_n[n]; ++i) ntm[n] |= 1ULL << (taint_ids[taint_off[n] + i] & 63);
    HIPCHK(c, hipMemcpyAsync(const_cast<uint64_t*>(c->cl.dev.ntaint), ntm.data(), ntm.size() * 8, hipMemcpyHostToDevice,
                             c->st));
  }
  HIPCHK(c, hipMemsetAsync(c->cl.dev.scalar_used, 0, (size_t)std::max<uint32_t>(c->ext.n_scalar, 1) * NN * 8, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  return KSG_OK;
}

int ksg_read_ext_used(ksg_ctx* c, int64_t* used) {
  if (!c || !used || !c->have_cluster) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (!c->ext_on) return fail(c, KSG_ERR_STATE, "ksg_read_ext_used: extensions are off");
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = flush_patches(c)) return rc;
  const size_t nb = (size_t)c->ext.n_scalar * c->cl.N * 8;
  if (nb) HIPCHK(c, hipMemcpyAsync(used, c->cl.dev.scalar_used, nb, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipStreamSynchronize(c->st));
  return KSG_OK;
}

// ---- ksg_update_cluster: a new node list under the same pods (ksg_remap.hip) ------------
// ksg_update_cluster swaps the old list's Cluster out of the context, builds the new list's
// beside it (the gather reads the old arrays and writes the new ones), and either drops the old
// one or, on any failure, swaps it back: a refused call leaves the context as it was. Whatever
// the local object holds at the end is freed with it.
static double us_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

// The device half, with the new list's arrays in c->cl.dev and the old list's in old.dev: the
// gather by src, the svc kernel, then the joined hosts' pods as patches (nm has their values).
static int remap_device(ksg_ctx* c, const Cluster& old, const std::vector<int32_t>& src,
                        const std::vector<int32_t>& outside_max, const NodeMirror& nm) {
  const uint32_t N = c->cl.N, S = c->cl.S, K = c->cfg.max_conflict_keys;
  struct Scratch {
    int32_t* p = nullptr;
    ~Scratch() {
      if (p) (void)hipFree(p);
    }
  } tmp;
  const size_t words = (size_t)N + 2 * (size_t)S;
  HIPCHK(c, hipMalloc((void**)&tmp.p, std::max<size_t>(words, 1) * sizeof(int32_t)));
  int32_t *d_src = tmp.p, *d_omax = tmp.p + N, *d_peer = d_omax + S;
  if (N) HIPCHK(c, hipMemcpyAsync(d_src, src.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->st));
  if (S) {
    HIPCHK(c, hipMemcpyAsync(d_omax, outside_max.data(), (size_t)S * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(d_peer, nm.svc_peer.data(), (size_t)S * 4, hipMemcpyHostToDevice, c->st));
  }
  const KsgDev &o = old.dev, &d = c->cl.dev;
  HIPCHK(c, hipEventRecord(c->ev0, c->st));
  HIPCHK(c, ksg_launch_remap_rows64(o.used_cpu, d.used_cpu, d_src, old.N, N, 1, c->st));
  HIPCHK(c, ksg_launch_remap_rows64(o.used_mem, d.used_mem, d_src, old.N, N, 1, c->st));
  if (c->ext_on && c->ext.n_scalar)
    HIPCHK(c, ksg_launch_remap_rows64(o.scalar_used, d.scalar_used, d_src, old.N, N, c->ext.n_scalar, c->st));
  HIPCHK(c, ksg_launch_remap_rows32(o.svc_cnt, d.svc_cnt, d_src, old.N, N, S, c->st));
  HIPCHK(c, ksg_launch_remap_bits(o.keymap, d.keymap, d_src, old.nw, c->cl.nw, N, K, c->st));
  HIPCHK(c, ksg_launch_remap_bits(o.svc_bits, d.svc_bits, d_src, old.nw, c->cl.nw, N, S, c->st));
  HIPCHK(c, ksg_launch_remap_svc(d.svc_cnt, N, S, d_omax, d_peer, o.svc_total, d.svc_max, d.svc_total, d.svc_peer, c->st));
  HIPCHK(c, hipEventRecord(c->ev1, c->st));
  if (int rc = flush_patches(c)) return rc;  // (the joined hosts' pods; synchronises when there are any)
  HIPCHK(c, hipStreamSynchronize(c->st));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->last_update_ms = ms;
  return KSG_OK;
}

static int update_cluster_impl(ksg_ctx* c, const ksg_node* nodes, uint32_t n_nodes, const uint32_t* node_pairs,
                               uint32_t n_node_pairs, const uint32_t* pair_keys, uint32_t n_pairs,
                               const uint32_t* old_to_new, const uint32_t* outside_old, const uint32_t* outside_new,
                               uint32_t n_outside, const ksg_node_ext_arrays* ext) {
  const auto t0 = std::chrono::steady_clock::now();
  if (int rs = cluster_ok(c)) return rs;
  if (c->pb.on) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
  if (ext && !c->ext_on) return fail(c, KSG_ERR_STATE, "ksg_update_cluster: ext given, extensions are off");
  if (!ext && c->ext_on) return fail(c, KSG_ERR_ARG, "ksg_update_cluster: extensions are on, ext == NULL");
  // (what the arguments alone decide comes first: such a refusal does not even stop the server)
  if (n_pairs == 0) n_pairs = 1;  // pair 0 always exists (empty)
  if (int rc = check_nodes(c, nodes, n_nodes, node_pairs, n_node_pairs, n_pairs)) return rc;
  const uint32_t oldN = c->cl.N, S = c->cl.S;
  if (n_nodes > (uint32_t)INT32_MAX) return fail(c, KSG_ERR_CAPACITY, "ksg_update_cluster: %u nodes", n_nodes);
  if (oldN && !old_to_new) return fail(c, KSG_ERR_ARG, "ksg_update_cluster: old_to_new == NULL with %u old nodes", oldN);
  if (n_outside && (!outside_old || !outside_new))
    return fail(c, KSG_ERR_ARG, "ksg_update_cluster: outside arrays missing");
  // the renaming: injective over the old ranks and the listed outside hosts
  std::unordered_map<uint32_t, uint32_t> omap;
  std::unordered_set<uint32_t> taken;
  omap.reserve(n_outside);
  taken.reserve((size_t)oldN + n_outside);
  for (uint32_t r = 0; r < oldN; ++r)
    if (!taken.insert(old_to_new[r]).second)
      return fail(c, KSG_ERR_ARG, "ksg_update_cluster: new host id %u given twice", old_to_new[r]);
  for (uint32_t j = 0; j < n_outside; ++j) {
    if (outside_old[j] < oldN)
      return fail(c, KSG_ERR_ARG, "ksg_update_cluster: outside_old[%u] = %u is a rank of the old list", j, outside_old[j]);
    if (!omap.emplace(outside_old[j], outside_new[j]).second)
      return fail(c, KSG_ERR_ARG, "ksg_update_cluster: outside host %u listed twice", outside_old[j]);
    if (!taken.insert(outside_new[j]).second)
      return fail(c, KSG_ERR_ARG, "ksg_update_cluster: new host id %u given twice", outside_new[j]);
  }
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  HIPCHK(c, hipSetDevice(c->device));
  // the mirror is complete and the device equals it
  if (int rc = flush_deferred(c)) return rc;
  if (int rc = flush_patches(c)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->st));
  for (const auto& kv : c->pods)
    if (kv.second.host >= oldN && !omap.count(kv.second.host))
      return fail(c, KSG_ERR_ARG, "ksg_update_cluster: pod %llu is on outside host %u, which is not listed",
                  (unsigned long long)kv.first, kv.second.host);
  // src: the old rank behind each new rank (every entry < oldN, so no kernel reads outside a row)
  std::vector<int32_t> src(n_nodes, -1);
  for (uint32_t r = 0; r < oldN; ++r)
    if (old_to_new[r] < n_nodes) src[old_to_new[r]] = (int32_t)r;
  auto renamed = [&](uint32_t h) { return h < oldN ? old_to_new[h] : omap.find(h)->second; };
  const double us_valid = us_since(t0);

  // ---- the new list's tables beside the old one's ----
  const auto t1 = std::chrono::steady_clock::now();
  Cluster old;
  std::swap(c->cl, old);
  auto refuse = [&](int rc) {
    std::swap(c->cl, old);  // (the new list's parts leave with `old`)
    c->patches.clear();
    return rc;
  };
  if (int rc = build_cluster(c, nodes, n_nodes, node_pairs, n_node_pairs, pair_keys, n_pairs, S)) return refuse(rc);
  if (ext)
    if (int rc = node_ext_upload(c, n_nodes, ext->scalar_cap, ext->taint_off, ext->taint_n, ext->taint_ids, ext->n_taint_ids))
      return refuse(rc);

  // ---- the new mirror: survivors' rows by src, then one walk over the pods ----
  const auto t2 = std::chrono::steady_clock::now();
  const uint32_t N = n_nodes, nsc = c->ext_on ? c->ext.n_scalar : 0;
  NodeMirror nm(N, S, c->ext.n_scalar);
  nm.svc_total = c->mir.svc_total;  // (the totals do not depend on the node list)
  std::vector<int32_t> outside_max(S, 0);
  std::vector<std::pair<PodRec*, uint32_t>> moved;  // pods whose host id changes
  for (uint32_t n = 0; n < N; ++n)
    if (src[n] >= 0) {
      nm.used_c[n] = c->mir.used_c[src[n]];
      nm.used_m[n] = c->mir.used_m[src[n]];
    }
  for (uint32_t q = 0; q < nsc; ++q)
    for (uint32_t n = 0; n < N; ++n)
      if (src[n] >= 0) nm.sc_used[(size_t)q * N + n] = c->mir.sc_used[(size_t)q * oldN + src[n]];
  for (uint32_t s = 0; s < S; ++s) {
    const int32_t* from = c->mir.svc_cnt.data() + (size_t)s * oldN;
    int32_t* to = nm.svc_cnt.data() + (size_t)s * N;
    int32_t m = 0;
    for (uint32_t n = 0; n < N; ++n)
      if (src[n] >= 0) m = std::max(m, to[n] = from[src[n]]);
    nm.svc_max[s] = m;
  }
  nm.key_ref.reserve(c->mir.key_ref.size());
  for (const auto& kv : c->mir.key_ref) {
    const uint32_t t = old_to_new[(uint32_t)kv.first];
    if (t < N) nm.key_ref[(kv.first & 0xffffffff00000000ull) | t] = kv.second;
  }
  const KsgDev& d = c->cl.dev;
  bool joined_wild = false;         // a joined host's pod would have set lr_wild in the fresh context
  int64_t joined_hi = c->used_hi;   // ... and the largest total it would have seen (used_hi only grows)
  for (auto& kv : c->pods) {
    PodRec& r = kv.second;
    const uint32_t t = renamed(r.host);
    if (t != r.host) moved.emplace_back(&r, t);
    if (t >= N) {  // outside the new list: counted by svc_max alone
      for (uint32_t s : r.svcs) outside_max[s] = std::max(outside_max[s], ++nm.svc_ext[s][t]);
      continue;
    }
    if (r.host < oldN) continue;  // (a survivor: its rows were gathered)
    // a host that joined the list: its pods onto the node, as mirror_add would (values for the patches).
    // On an outside host note_requests never saw them (ksg_add_pod checks node hosts only); the fresh
    // context re-adds them on a node, so a negative request or a total that could wrap turns it wide.
    joined_wild = joined_wild || r.cpu < 0 || r.mem < 0 ||
                  (unsigned __int128)(uint64_t)std::max<int64_t>(joined_hi, 0) + (uint64_t)std::max<int64_t>(std::max(r.cpu, r.mem), 0) >
                      (unsigned __int128)INT64_MAX;
    nm.used_c[t] = (int64_t)((uint64_t)nm.used_c[t] + (uint64_t)r.cpu);
    nm.used_m[t] = (int64_t)((uint64_t)nm.used_m[t] + (uint64_t)r.mem);
    joined_hi = std::max(joined_hi, std::max(nm.used_c[t], nm.used_m[t]));
    patch64(c, d.used_cpu + t, nm.used_c[t]);
    patch64(c, d.used_mem + t, nm.used_m[t]);
    for (uint32_t q = 0; q < nsc; ++q) {
      if (!r.scalar[q]) continue;
      int64_t& u = nm.sc_used[(size_t)q * N + t];
      u = (int64_t)((uint64_t)u + (uint64_t)r.scalar[q]);
      patch64(c, d.scalar_used + (size_t)q * N + t, u);
    }
    for (uint32_t k : r.keys)
      if (++nm.key_ref[((uint64_t)k << 32) | t] == 1) patch_or(c, d.keymap + (size_t)k * c->cl.nw + (t >> 6), 1ULL << (t & 63));
    for (uint32_t s : r.svcs) {
      const int32_t v = ++nm.svc_cnt[(size_t)s * N + t];
      patch32(c, d.svc_cnt + (size_t)s * N + t, v);
      if (v == 1) patch_or(c, d.svc_bits + (size_t)s * c->cl.nw + (t >> 6), 1ULL << (t & 63));
      nm.svc_max[s] = std::max(nm.svc_max[s], v);
    }
  }
  for (uint32_t s = 0; s < S; ++s) {
    for (const auto& m : c->mir.svc_members[s]) nm.svc_members[s].emplace_hint(nm.svc_members[s].end(), m.first, renamed(m.second));
    if (!nm.svc_members[s].empty()) {
      const uint32_t h = nm.svc_members[s].begin()->second;
      nm.svc_peer[s] = h < N ? (int32_t)h : -2;
    }
    nm.svc_max[s] = std::max(nm.svc_max[s], outside_max[s]);
  }
  // (the svc kernel sees the gathered counts only: the joined hosts' maxima go with their patches)
  if (!c->patches.empty())
    for (uint32_t s = 0; s < S; ++s) patch32(c, d.svc_max + s, nm.svc_max[s]);
  double us_mirror = us_since(t2);

  // ---- the device work; then the new list is in force ----
  const auto t3 = std::chrono::steady_clock::now();
  if (int rc = remap_device(c, old, src, outside_max, nm)) return refuse(rc);
  const double us_dev = std::chrono::duration<double, std::micro>(t2 - t1).count() + us_since(t3);
  const auto t4 = std::chrono::steady_clock::now();
  for (auto& mv : moved) mv.first->host = mv.second;
  c->mir = std::move(nm);
  // the score path: never narrower than the fresh context's (the sticky causes stay, the
  // capacities' were recomputed by build_cluster, the used-total bounds are recomputed on use)
  c->cl.lr_wild = c->cl.lr_wild || old.lr_wild || joined_wild;
  c->used_hi = std::max(c->used_hi, joined_hi);
  for (uint32_t n = 0; n < N; ++n) c->used_hi = std::max(c->used_hi, std::max(c->mir.used_c[n], c->mir.used_m[n]));
  c->mu_dirty = true;
  set_wide(c);
  c->ppw_est = 0.0;
  us_mirror += us_since(t4);
  c->last_update_us[0] = us_valid;
  c->last_update_us[1] = us_dev;
  c->last_update_us[2] = us_mirror;
  return KSG_OK;
}

int ksg_update_cluster(ksg_ctx* c, const ksg_node* nodes, uint32_t n_nodes, const uint32_t* node_pairs,
                       uint32_t n_node_pairs, const uint32_t* pair_keys, uint32_t n_pairs, const uint32_t* old_to_new,
                       const uint32_t* outside_old, const uint32_t* outside_new, uint32_t n_outside,
                       const ksg_node_ext_arrays* ext) {
  if (!c) return KSG_ERR_ARG;
  KSG_LOCK(c);
  const int rc = update_cluster_impl(c, nodes, n_nodes, node_pairs, n_node_pairs, pair_keys, n_pairs, old_to_new,
                                     outside_old, outside_new, n_outside, ext);
  // a HIP error at any point: the device may not be what the mirror says (as after a failed batch)
  if (rc == KSG_ERR_HIP && c->have_cluster) c->diverged = true;
  return rc;
}

int ksg_last_update_ms(ksg_ctx* c, double* ms) {
  if (!c || !ms) return KSG_ERR_ARG;
  KSG_LOCK(c);
  *ms = c->last_update_ms;
  return KSG_OK;
}

int ksg_last_update_host_us(ksg_ctx* c, double* us3) {
  if (!c || !us3) return KSG_ERR_ARG;
  KSG_LOCK(c);
  for (int i = 0; i < 3; ++i) us3[i] = c->last_update_us[i];
  return KSG_OK;
}

}  // extern "C"
