// ksg_query.cpp — the frame of the read-only batch queries (query_enter ... query_chunks, described
// in ksg_host.h) and the three oldest queries on it: ksg_explain_batch, ksg_prioritize_batch and
// ksg_headroom_batch. The newer ones call the frame from files of their own (ksg_without.cpp,
// ksg_preempt.cpp, ksg_pack.cpp).
#include <cstdio>
#include <cstring>

#include "ksg_host.h"

#pragma GCC visibility push(hidden)

// ksg_explain_batch: device staging for the per-node codes of one chunk of pods
constexpr size_t kExplainStageBytes = (size_t)64 << 20;

// ---- the read-only batch queries' frame (ksg_host.h) --------------------------
int query_enter(ksg_ctx* c, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids, uint32_t n_ids, double* last_ms) {
  if (c->pb.on) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
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
    HIPCHK(c, hipEventCreate(&c->ev_x0.e));
    HIPCHK(c, hipEventCreate(&c->ev_x1.e));
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

}  // extern "C"
