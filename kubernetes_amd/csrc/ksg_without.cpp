// ksg_without.cpp — ksg_explain_without: FitError reports against the state with a suffix of
// an ordered list of committed pods taken away (ksg_explain_without.hip). Nothing is removed:
// per call the host mirror (c->pods, key_ref, svc_members) yields three read-only tables,
//
//   node deltas   per node the listed pods on it, sorted by list index, with the wrapping
//                 suffix sums of their cpu, memory and extended-resource requests;
//   conflict bits the (node, key) pairs whose holders are all listed, with the smallest list
//                 index among them (a pair with a holder outside the list keeps its bit);
//   peers         per explained pod its ServiceAffinity peer as of its position,
//
// uploaded in one copy. The protocol, the validation, the uploads and the chunk loop are the
// read-only batch queries' frame (query_enter ... query_chunks, ksg_host.h). The tables are
// built by without_tables, which ksg_preempt_batch (ksg_preempt.cpp) calls too, with a fourth
// table (the conflict keys of every row entry) in place of the peers.
#include <cstring>

#include "ksg_host.h"

namespace {

struct Listed {  // a listed pod on a node of the node list
  uint32_t node, idx;
  const PodRec* r;
};
struct Conflict {
  uint32_t node, key, min_idx, held;  // held: occurrences among the listed pods (mirror_add's count)
};

// A service's peer as a function of the position: its members in commit order up to the
// first one outside the list, keeping of the listed ones those whose list index is below
// every earlier one's (a member is the peer at position fa iff it is the first with
// idx < fa; a member outside the list counts as idx = -1 and ends the walk).
struct PeerChain {
  std::vector<std::pair<uint32_t, int32_t>> listed;  // (list index, peer code), indices descending
  int32_t tail = -1;                                 // the first member outside the list (-1: none)
  int32_t at(uint32_t fa) const {
    for (const auto& m : listed)
      if (m.first < fa) return m.second;
    return tail;
  }
};

inline size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

}  // namespace

#pragma GCC visibility push(hidden)

int without_position(ksg_ctx* c, const uint32_t* first_absent, uint32_t i, uint32_t n_absent) {
  if (first_absent && first_absent[i] > n_absent)
    return fail(c, KSG_ERR_ARG, "first_absent[%u] = %u > n_absent %u", i, first_absent[i], n_absent);
  return KSG_OK;
}

int without_tables(ksg_ctx* c, const ksg_pod* pods, uint32_t n, const uint64_t* absent_uids, uint32_t n_absent,
                   const uint32_t* first_absent, bool peers, bool entry_keys, WithoutTables* tabs) {
  int rc;
  // the list: committed uids, each once (an invalid one leaves the device untouched)
  const uint32_t N = c->cl.N, ns = c->ext_on ? c->ext.n_scalar : 0;
  std::vector<Listed> on;
  std::unordered_map<uint64_t, uint32_t> idx_of_seq;  // a listed pod's commit sequence number -> list index
  idx_of_seq.reserve(n_absent);
  on.reserve(n_absent);
  for (uint32_t j = 0; j < n_absent; ++j) {
    const auto it = c->pods.find(absent_uids[j]);
    if (it == c->pods.end())
      return fail(c, KSG_ERR_ARG, "absent_uids[%u]: unknown pod uid %llu", j, (unsigned long long)absent_uids[j]);
    if (!idx_of_seq.emplace(it->second.seq, j).second)
      return fail(c, KSG_ERR_ARG, "absent_uids[%u]: uid %llu listed twice", j, (unsigned long long)absent_uids[j]);
    if (it->second.host < N) on.push_back(Listed{it->second.host, j, &it->second});
  }
  std::sort(on.begin(), on.end(),
            [](const Listed& a, const Listed& b) { return a.node != b.node ? a.node < b.node : a.idx < b.idx; });
  // conflict keys only listed pods hold: the listed occurrences equal the mirror's count
  std::unordered_map<uint64_t, Conflict> held;
  size_t K = 0;  // the row entries' keys, all told
  for (const Listed& l : on) {
    K += l.r->keys.size();
    for (uint32_t k : l.r->keys) {
      auto ins = held.emplace(((uint64_t)k << 32) | l.node, Conflict{l.node, k, l.idx, 0});
      ins.first->second.min_idx = std::min(ins.first->second.min_idx, l.idx);
      ++ins.first->second.held;
    }
  }
  std::vector<Conflict> cf;
  for (const auto& kv : held) {
    const auto kit = c->mir.key_ref.find(kv.first);
    if (kit != c->mir.key_ref.end() && kit->second == kv.second.held) cf.push_back(kv.second);
  }
  std::sort(cf.begin(), cf.end(),
            [](const Conflict& a, const Conflict& b) { return a.node != b.node ? a.node < b.node : a.key < b.key; });
  const bool aff = peers && (c->cl.dev.preds & KSG_PRED_SERVICEAFFINITY) != 0;  // (else no peer is looked up)
  // one buffer: nd_sum uint64[2 + ns][E], touched uint64[nw], then the uint32 arrays nd_off[N + 1],
  // nd_idx[E], cf_off[N + 1], cf_key[F], cf_min[F], first_absent[n], peer int32[n], and with
  // entry_keys ek_off[E + 1], ek_key[K]
  const size_t E = on.size(), F = cf.size();
  const size_t o_touch = (2 + (size_t)ns) * E * 8, o_ndoff = o_touch + (size_t)c->cl.nw * 8;
  const size_t o_ndidx = o_ndoff + ((size_t)N + 1) * 4, o_cfoff = o_ndidx + E * 4, o_cfkey = o_cfoff + ((size_t)N + 1) * 4;
  const size_t o_cfmin = o_cfkey + F * 4, o_fa = o_cfmin + F * 4, o_peer = o_fa + (size_t)n * 4;
  const size_t o_ekoff = o_peer + (size_t)n * 4, o_ekkey = o_ekoff + (entry_keys ? (E + 1) * 4 : 0);
  const size_t tb = align8(o_ekkey + (entry_keys ? K * 4 : 0));
  if ((rc = c->h_wtab.grow(c, tb)) || (rc = c->d_wtab.grow(c, tb))) return rc;
  uint8_t* const h = c->h_wtab;
  memset(h, 0, o_ndidx);  // (the sums are written below; touched and nd_off start from zero)
  uint64_t* const sum = reinterpret_cast<uint64_t*>(h);
  uint64_t* const touched = reinterpret_cast<uint64_t*>(h + o_touch);
  uint32_t* const nd_off = reinterpret_cast<uint32_t*>(h + o_ndoff);
  uint32_t* const nd_idx = reinterpret_cast<uint32_t*>(h + o_ndidx);
  uint32_t* const cf_off = reinterpret_cast<uint32_t*>(h + o_cfoff);
  uint32_t* const cf_key = reinterpret_cast<uint32_t*>(h + o_cfkey);
  uint32_t* const cf_min = reinterpret_cast<uint32_t*>(h + o_cfmin);
  uint32_t* const fa = reinterpret_cast<uint32_t*>(h + o_fa);
  int32_t* const peer = reinterpret_cast<int32_t*>(h + o_peer);
  for (size_t e = 0; e < E; ++e) {
    nd_idx[e] = on[e].idx;
    ++nd_off[on[e].node + 1];
    touched[on[e].node >> 6] |= 1ULL << (on[e].node & 63);
  }
  for (uint32_t x = 0; x < N; ++x) nd_off[x + 1] += nd_off[x];
  for (size_t e = E; e-- > 0;) {  // suffix sums within a node's row, wrapping like remove_pod_impl's subtraction
    const bool last = e + 1 == E || on[e + 1].node != on[e].node;
    const PodRec& r = *on[e].r;
    sum[e] = (uint64_t)r.cpu + (last ? 0 : sum[e + 1]);
    sum[E + e] = (uint64_t)r.mem + (last ? 0 : sum[E + e + 1]);
    for (uint32_t q = 0; q < ns; ++q) sum[(2 + q) * E + e] = (uint64_t)r.scalar[q] + (last ? 0 : sum[(2 + q) * E + e + 1]);
  }
  memset(cf_off, 0, ((size_t)N + 1) * 4);
  for (size_t f = 0; f < F; ++f) {
    cf_key[f] = cf[f].key;
    cf_min[f] = cf[f].min_idx;
    ++cf_off[cf[f].node + 1];
  }
  for (uint32_t x = 0; x < N; ++x) cf_off[x + 1] += cf_off[x];
  if (entry_keys) {  // each row entry's own conflict keys (PodRec::keys)
    uint32_t* const ek_off = reinterpret_cast<uint32_t*>(h + o_ekoff);
    uint32_t* const ek_key = reinterpret_cast<uint32_t*>(h + o_ekkey);
    uint32_t k = 0;
    for (size_t e = 0; e < E; ++e) {
      ek_off[e] = k;
      for (uint32_t key : on[e].r->keys) ek_key[k++] = key;
    }
    ek_off[E] = k;
  }
  // the positions, and the peers as of each pod's position (one walk per service)
  std::unordered_map<int32_t, PeerChain> chains;
  for (uint32_t i = 0; i < n; ++i) {
    fa[i] = first_absent ? first_absent[i] : 0;
    peer[i] = -1;
    const int32_t s = pods[i].service;
    if (!aff || s < 0) continue;
    auto ins = chains.emplace(s, PeerChain{});
    PeerChain& pc = ins.first->second;
    if (ins.second) {
      uint32_t lowest = UINT32_MAX;
      for (const auto& m : c->mir.svc_members[s]) {  // seq order: commit order
        const int32_t code = m.second < N ? (int32_t)m.second : -2;
        const auto it = idx_of_seq.find(m.first);
        if (it == idx_of_seq.end()) {
          pc.tail = code;
          break;
        }
        if (it->second < lowest) {
          lowest = it->second;
          pc.listed.emplace_back(it->second, code);
        }
      }
    }
    peer[i] = pc.at(fa[i]);
  }
  uint8_t* const t = c->d_wtab;
  KsgWithout& w = tabs->w;
  w = KsgWithout{};
  w.nd_sum = reinterpret_cast<const uint64_t*>(t);
  w.touched = reinterpret_cast<const uint64_t*>(t + o_touch);
  w.nd_off = reinterpret_cast<const uint32_t*>(t + o_ndoff);
  w.nd_idx = reinterpret_cast<const uint32_t*>(t + o_ndidx);
  w.cf_off = reinterpret_cast<const uint32_t*>(t + o_cfoff);
  w.cf_key = reinterpret_cast<const uint32_t*>(t + o_cfkey);
  w.cf_min = reinterpret_cast<const uint32_t*>(t + o_cfmin);
  w.first_absent = reinterpret_cast<const uint32_t*>(t + o_fa);
  w.peer = aff ? reinterpret_cast<const int32_t*>(t + o_peer) : nullptr;
  w.nd_n = (uint32_t)E;
  w.n_absent = n_absent;
  tabs->ek = KsgPreemptKeys{};
  if (entry_keys) {
    tabs->ek.ek_off = reinterpret_cast<const uint32_t*>(t + o_ekoff);
    tabs->ek.ek_key = reinterpret_cast<const uint32_t*>(t + o_ekkey);
  }
  tabs->bytes = tb;
  return KSG_OK;
}

#pragma GCC visibility pop

extern "C" {

int ksg_explain_without(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                        uint32_t n_ids, const uint64_t* absent_uids, uint32_t n_absent, const uint32_t* first_absent,
                        uint8_t* codes, uint32_t* hist, uint8_t* err) {
  if (!c || (n && (!pods || !hist || !err))) return KSG_ERR_ARG;
  KSG_LOCK(c);
  int rc;
  if ((rc = query_enter(c, ext, n, ids, n_ids, &c->last_without_ms))) return rc == kQueryDone ? KSG_OK : rc;
  if (n_absent && (!absent_uids || !first_absent)) return fail(c, KSG_ERR_ARG, "absent list or positions missing");
  const auto position = [&](uint32_t i) { return without_position(c, first_absent, i, n_absent); };
  if ((rc = query_validate(c, pods, ext, n, ids, n_ids, std::cref(position)))) return rc;
  WithoutTables tabs;
  if ((rc = without_tables(c, pods, n, absent_uids, n_absent, first_absent, true, false, &tabs))) return rc;
  const uint32_t N = c->cl.N;
  const ksg_pod_ext* dext;
  if ((rc = query_upload(c, pods, ext, n, ids, n_ids, false, &dext))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_wtab, c->h_wtab, tabs.bytes, hipMemcpyHostToDevice, c->st));
  const uint32_t* const d_fa = tabs.w.first_absent;
  const int32_t* const d_peer = tabs.w.peer;
  KsgWithout w = tabs.w;
  // hist and err for the whole call; the per-node codes in a bounded staging buffer, a chunk
  // of pods at a time
  const size_t hb = (size_t)n * KSG_EXPLAIN_SLOTS * sizeof(uint32_t);
  if ((rc = c->d_whist.grow(c, hb + n))) return rc;
  uint32_t* d_hist = reinterpret_cast<uint32_t*>(c->d_whist.p);
  uint8_t* d_err = c->d_whist + hb;
  HIPCHK(c, hipMemsetAsync(c->d_whist, 0, hb + n, c->st));
  const uint32_t per = query_per(c->without_stage, codes ? N : 0, KSG_EXPLAIN_CHUNK, n);
  if (codes && (rc = c->d_wcodes.grow(c, (size_t)per * N))) return rc;
  const auto launch = [&](uint32_t a, uint32_t m) {
    w.first_absent = d_fa + a;  // (offset like the pods)
    w.peer = d_peer ? d_peer + a : nullptr;
    HIPCHK(c, ksg_launch_explain_without(c->cl.dev, w, c->d_pods + a, dext ? dext + a : nullptr, c->d_ids, m,
                                         codes ? c->d_wcodes.p : nullptr, d_hist + (size_t)a * KSG_EXPLAIN_SLOTS,
                                         d_err + a, c->st));
    return KSG_OK;
  };
  const auto copies = [&](uint32_t a, uint32_t m, bool last) {
    if (codes)
      HIPCHK(c, hipMemcpyAsync(codes + (size_t)a * N, c->d_wcodes, (size_t)m * N, hipMemcpyDeviceToHost, c->st));
    if (last) {  // straight into the caller's arrays
      HIPCHK(c, hipMemcpyAsync(hist, d_hist, hb, hipMemcpyDeviceToHost, c->st));
      HIPCHK(c, hipMemcpyAsync(err, d_err, n, hipMemcpyDeviceToHost, c->st));
    }
    return KSG_OK;
  };
  return query_chunks(c, n, per, &c->last_without_ms, std::cref(launch), std::cref(copies));
}

int ksg_last_explain_without_ms(ksg_ctx* c, double* ms) {
  if (!c || !ms) return KSG_ERR_ARG;
  KSG_LOCK(c);
  *ms = c->last_without_ms;
  return KSG_OK;
}

}  // extern "C"
