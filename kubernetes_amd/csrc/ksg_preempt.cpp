// ksg_preempt.cpp — ksg_preempt_batch: per pending pod and node the committed pods that would
// have to leave (the reprieve walk of selectVictimsOnNode), and the node to preempt on
// (ksg_preempt.hip; include/kschedgpu.h has the definition). Nothing is removed: the call reads
// ksg_explain_without's tables of the ordered list (without_tables, ksg_without.cpp) with the
// conflict keys of every row entry in place of the peers. The protocol, the validation, the
// uploads and the chunk loop are the read-only batch queries' frame (query_enter ...
// query_chunks, ksg_host.h).
#include <cstring>

#include "ksg_host.h"

extern "C" {

int ksg_preempt_batch(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                      uint32_t n_ids, const uint64_t* absent_uids, uint32_t n_absent, const uint32_t* first_absent,
                      uint32_t max_victims, int32_t* best_node, uint32_t* n_victims, uint32_t* victims,
                      uint32_t* cand_count, uint32_t* free_count, uint32_t* node_victims) {
  if (!c || (n && (!pods || !best_node || !n_victims || !cand_count || !free_count))) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (max_victims > KSG_PREEMPT_MAX_VICTIMS)
    return fail(c, KSG_ERR_ARG, "max_victims %u > KSG_PREEMPT_MAX_VICTIMS", max_victims);
  if (n && max_victims && !victims) return fail(c, KSG_ERR_ARG, "max_victims > 0 needs victims");
  int rc;
  if ((rc = query_enter(c, ext, n, ids, n_ids, &c->last_preempt_ms))) return rc == kQueryDone ? KSG_OK : rc;
  // the peer of a ServiceAffinity predicate depends on pods on other nodes: not a per-node question
  if (c->cfg.predicates & KSG_PRED_SERVICEAFFINITY)
    return fail(c, KSG_ERR_STATE,
                "ksg_preempt_batch: the configuration has a ServiceAffinity predicate, whose peer is not a per-node "
                "question (ksg_explain_without answers feasibility there)");
  if (n_absent && (!absent_uids || !first_absent)) return fail(c, KSG_ERR_ARG, "absent list or positions missing");
  const auto position = [&](uint32_t i) { return without_position(c, first_absent, i, n_absent); };
  if ((rc = query_validate(c, pods, ext, n, ids, n_ids, std::cref(position)))) return rc;
  WithoutTables tabs;
  if ((rc = without_tables(c, pods, n, absent_uids, n_absent, first_absent, false, true, &tabs))) return rc;
  const uint32_t N = c->cl.N;
  const ksg_pod_ext* dext;
  if ((rc = query_upload(c, pods, ext, n, ids, n_ids, false, &dext))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_wtab, c->h_wtab, tabs.bytes, hipMemcpyHostToDevice, c->st));
  const uint32_t* const d_fa = tabs.w.first_absent;
  KsgWithout w = tabs.w;
  // the per-pod results of the whole call: int32 best[n], uint32 victims[n], cand[n], free[n], then
  // the victim lists uint32[n][max_victims]; the tile partials and, where asked for, the per-node
  // counts of a chunk of pods in bounded staging buffers
  const size_t o_nv = (size_t)n * 4, o_cand = o_nv * 2, o_free = o_nv * 3, o_vic = o_nv * 4;
  const size_t ob = o_vic + (size_t)n * max_victims * 4;
  if ((rc = c->d_vout.grow(c, ob)) || (rc = c->h_dn.grow(c, ob))) return rc;
  uint8_t* const vo = c->d_vout;
  const size_t T = ksg_preempt_tiles(c->cl.dev);
  const size_t bpp = T * sizeof(KsgPreemptPart) + (node_victims ? (size_t)N * sizeof(uint32_t) : 0);
  const uint32_t per = query_per(c->preempt_stage, bpp, KSG_EXPLAIN_CHUNK, n);
  if ((rc = c->d_vpart.grow(c, (size_t)per * T * sizeof(KsgPreemptPart)))) return rc;
  if (node_victims && (rc = c->d_vnode.grow(c, (size_t)per * N))) return rc;
  const auto launch = [&](uint32_t a, uint32_t m) {
    w.first_absent = d_fa + a;  // (offset like the pods)
    HIPCHK(c, ksg_launch_preempt(c->cl.dev, w, tabs.ek, c->d_pods + a, dext ? dext + a : nullptr, c->d_ids, m, max_victims,
                                 node_victims ? c->d_vnode.p : nullptr, reinterpret_cast<KsgPreemptPart*>(c->d_vpart.p),
                                 reinterpret_cast<int32_t*>(vo) + a, reinterpret_cast<uint32_t*>(vo + o_nv) + a,
                                 reinterpret_cast<uint32_t*>(vo + o_vic) + (size_t)a * max_victims,
                                 reinterpret_cast<uint32_t*>(vo + o_cand) + a, reinterpret_cast<uint32_t*>(vo + o_free) + a,
                                 c->st));
    return KSG_OK;
  };
  const auto copies = [&](uint32_t a, uint32_t m, bool last) {
    if (node_victims)
      HIPCHK(c, hipMemcpyAsync(node_victims + (size_t)a * N, c->d_vnode, (size_t)m * N * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, c->st));
    if (last) HIPCHK(c, hipMemcpyAsync(c->h_dn, vo, ob, hipMemcpyDeviceToHost, c->st));
    return KSG_OK;
  };
  if ((rc = query_chunks(c, n, per, &c->last_preempt_ms, std::cref(launch), std::cref(copies)))) return rc;
  memcpy(best_node, c->h_dn, o_nv);
  memcpy(n_victims, c->h_dn + o_nv, o_nv);
  memcpy(cand_count, c->h_dn + o_cand, o_nv);
  memcpy(free_count, c->h_dn + o_free, o_nv);
  if (max_victims) memcpy(victims, c->h_dn + o_vic, (size_t)n * max_victims * 4);
  return KSG_OK;
}

int ksg_last_preempt_ms(ksg_ctx* c, double* ms) {
  if (!c || !ms) return KSG_ERR_ARG;
  KSG_LOCK(c);
  *ms = c->last_preempt_ms;
  return KSG_OK;
}

}  // extern "C"
