// ksg_pack.cpp — ksg_pack_batch: first-fit pod sets (ksg_pack.hip; include/kschedgpu.h has the
// definition). Every set is packed pod by pod against the committed state plus what the set
// itself has placed so far, one workgroup per set; nothing is written to the node state. The
// protocol, the validation and the uploads are the read-only batch queries' frame (query_enter
// ... query_chunks, ksg_host.h); the unit of the frame's one chunk is the set. The call's tables
// (the sets' offsets into the pods, their excluded nodes, the target words) travel in h_wtab /
// d_wtab, which it shares with ksg_explain_without and ksg_preempt_batch. There is no per-node
// output and no limit on the node count: the kernel keeps a set's placements in a table sized by
// KSG_PACK_MAX_SET.
#include <cstring>

#include "ksg_host.h"

extern "C" {

int ksg_pack_batch(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                   uint32_t n_ids, const uint32_t* set_size, const uint32_t* set_exclude, uint32_t n_sets,
                   const uint64_t* target_words, int32_t* out_nodes, uint32_t* placed) {
  if (!c || (n && (!pods || !out_nodes)) || (n_sets && !placed)) return KSG_ERR_ARG;
  KSG_LOCK(c);
  int rc;
  if ((rc = query_enter(c, ext, n_sets, ids, n_ids, &c->last_pack_ms))) {
    if (rc == kQueryDone) return n ? fail(c, KSG_ERR_ARG, "ksg_pack_batch: %u pods in no set", n) : KSG_OK;
    return rc;
  }
  // the set's first member can become the predicate's peer, which is not a per-node question
  if (c->cfg.predicates & KSG_PRED_SERVICEAFFINITY)
    return fail(c, KSG_ERR_STATE,
                "ksg_pack_batch: the configuration has a ServiceAffinity predicate, whose peer is not a per-node "
                "question (a set's first pod can become the peer of the rest)");
  if (n_sets > 0x7fffffffu) return fail(c, KSG_ERR_ARG, "%u sets > 2^31 - 1 (one launch, one workgroup a set)", n_sets);
  if (!set_size) return fail(c, KSG_ERR_ARG, "set_size missing");
  const uint32_t N = c->cl.N, nw = c->cl.nw;
  uint64_t sum = 0;
  for (uint32_t s = 0; s < n_sets; ++s) {
    if (set_size[s] > KSG_PACK_MAX_SET)
      return fail(c, KSG_ERR_ARG, "set %u has %u pods > KSG_PACK_MAX_SET", s, set_size[s]);
    sum += set_size[s];
    if (set_exclude && set_exclude[s] >= N && set_exclude[s] != KSG_PACK_NO_NODE)
      return fail(c, KSG_ERR_ARG, "set %u excludes node %u of %u", s, set_exclude[s], N);
  }
  if (sum != n) return fail(c, KSG_ERR_ARG, "the sets hold %llu pods, the call %u", (unsigned long long)sum, n);
  if (n == 0) {  // (sets of size 0 only)
    memset(placed, 0, (size_t)n_sets * sizeof(uint32_t));
    return KSG_OK;
  }
  if ((rc = query_validate(c, pods, ext, n, ids, n_ids))) return rc;
  // the tables: uint64 targets[nw] (where given), uint32 set_off[n_sets + 1], uint32 exclude[n_sets] (where given)
  const size_t o_off = target_words ? (size_t)nw * 8 : 0, o_ex = o_off + ((size_t)n_sets + 1) * 4;
  const size_t tb = o_ex + (set_exclude ? (size_t)n_sets * 4 : 0);
  if ((rc = c->h_wtab.grow(c, tb)) || (rc = c->d_wtab.grow(c, tb))) return rc;
  if (target_words) memcpy(c->h_wtab, target_words, (size_t)nw * 8);
  uint32_t* const off = reinterpret_cast<uint32_t*>(c->h_wtab + o_off);
  off[0] = 0;
  for (uint32_t s = 0; s < n_sets; ++s) off[s + 1] = off[s] + set_size[s];
  if (set_exclude) memcpy(c->h_wtab + o_ex, set_exclude, (size_t)n_sets * 4);
  const ksg_pod_ext* dext;
  if ((rc = query_upload(c, pods, ext, n, ids, n_ids, false, &dext))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_wtab, c->h_wtab, tb, hipMemcpyHostToDevice, c->st));
  uint8_t* const dt = c->d_wtab;
  const KsgPack k{reinterpret_cast<const uint32_t*>(dt + o_off),
                  set_exclude ? reinterpret_cast<const uint32_t*>(dt + o_ex) : nullptr,
                  target_words ? reinterpret_cast<const uint64_t*>(dt) : nullptr};
  // the results of the whole call: int32 out_nodes[n], then uint32 placed[n_sets] (one buffer, one copy out)
  const size_t o_pl = (size_t)n * 4, ob = o_pl + (size_t)n_sets * 4;
  if ((rc = c->d_kout.grow(c, ob)) || (rc = c->h_dn.grow(c, ob))) return rc;
  uint8_t* const ko = c->d_kout;
  const auto launch = [&](uint32_t, uint32_t sets) {
    HIPCHK(c, ksg_launch_pack(c->cl.dev, k, c->d_pods, dext, c->d_ids, sets, reinterpret_cast<int32_t*>(ko),
                              reinterpret_cast<uint32_t*>(ko + o_pl), c->st));
    return KSG_OK;
  };
  const auto copies = [&](uint32_t, uint32_t, bool) {
    HIPCHK(c, hipMemcpyAsync(c->h_dn, ko, ob, hipMemcpyDeviceToHost, c->st));
    return KSG_OK;
  };
  if ((rc = query_chunks(c, n_sets, n_sets, &c->last_pack_ms, std::cref(launch), std::cref(copies)))) return rc;
  memcpy(out_nodes, c->h_dn, o_pl);
  memcpy(placed, c->h_dn + o_pl, (size_t)n_sets * 4);
  return KSG_OK;
}

int ksg_last_pack_ms(ksg_ctx* c, double* ms) {
  if (!c || !ms) return KSG_ERR_ARG;
  KSG_LOCK(c);
  *ms = c->last_pack_ms;
  return KSG_OK;
}

}  // extern "C"
