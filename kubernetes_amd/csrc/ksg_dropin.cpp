// ksg_dropin.cpp — the per-pod (drop-in) path of the C ABI: ksg_schedule_begin /
// ksg_schedule_commit / ksg_evaluate with their _ext variants, and the host client of the
// resident server (ksg_serve.hip) that answers begin and commit as requests in mapped host
// memory where the context is eligible (srv_eligible), instead of launches, copies and stream
// syncs. The client's state is c->srv (struct SrvClient), the pod between begin and commit
// c->pb (struct PendingBegin), both in ksg_host.h. The other host files call srv_stop before
// they use the stream, flush_patches calls srv_flush_patches while a server runs, and
// ksg_destroy srv_print_stamps; everything else here is this file's own.
#include <atomic>
#include <cstdio>
#include <cstring>

#include "ksg_host.h"

#pragma GCC visibility push(hidden)

// the single-pod APIs: pod + ids staged contiguously, one copy into d_one;
// one_pod / one_ids point into it until the next single-pod upload
static int upload_one(ksg_ctx* c, const ksg_pod* pod, const uint32_t* ids, size_t n_ids) {
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

static int ensure_map(ksg_ctx* c) {
  return c->h_map ? KSG_OK : c->h_map.alloc(c, 64);
}

// ... and the extension record's taint lists (the single-pod _ext entry points)
static size_t call_ids_extent(const ksg_ctx* c, const ksg_pod* p) {
  size_t e = pod_ids_extent(p);
  if (c->cur_ext) {
    e = std::max<size_t>(e, (size_t)c->cur_ext->hard_off + c->cur_ext->n_hard);
    e = std::max<size_t>(e, (size_t)c->cur_ext->soft_off + c->cur_ext->n_soft);
  }
  return e;
}

// ---- the resident drop-in server (ksg_serve.hip) ------------------------------
SrvClient::SrvClient() {
  enabled = env_flag("KSG_SERVE", true);
  stamps = env_flag("KSG_SERVE_STAMPS", false);
  debug = env_flag("KSG_SERVE_DEBUG", false);
  trace = env_flag("KSG_SERVE_TRACE", false);
  if (const char* go = getenv("KSG_SERVE_GRID_OPTS")) grid_opts = (int64_t)strtoul(go, nullptr, 0);
  idle_us = (uint64_t)env_int("KSG_SERVE_IDLE_US", (int64_t)idle_us, 1, INT64_MAX);
  grid_on = env_flag("KSG_SERVE_GRID", true);
  grid_min = (uint32_t)env_int("KSG_SERVE_GRID_MIN", grid_min, 0, INT32_MAX);
  npt4_min = (uint32_t)env_int("KSG_SERVE_GRID_NPT4_MIN", npt4_min, 0, INT32_MAX);
  grid_ext = env_flag("KSG_SERVE_GRID_EXT", true);
}

// nodes per thread of the grid server's scan workgroups (KSG_GSRV_NT threads each)
static uint32_t srv_npt(const ksg_ctx* c) { return c->cl.hi - c->cl.lo > c->srv.npt4_min ? 4u : 1u; }

static bool srv_grid(const ksg_ctx* c) {
  const uint32_t n = c->cl.hi - c->cl.lo, per = KSG_GSRV_NT * srv_npt(c);
  // (extensions: the filters and BalancedAllocation are per node; TaintToleration normalises over
  // the filtered set: the scan workgroups exchange their maxima through device memory)
  // (ServiceAntiAffinity: the domain counts likewise, up to KSG_GSRV_MAXD domains, without extensions)
  return c->srv.grid_on && !(anti_on(c) && (c->ext_on || c->cl.dev.n_domains_total > KSG_GSRV_MAXD)) &&
         !(c->ext_on && !c->srv.grid_ext) &&
         n > c->srv.grid_min &&
         (n + per - 1) / per <= KSG_GSRV_MAXW;
}

static bool srv_eligible(const ksg_ctx* c) {
  return c->srv.enabled && c->world == 1 && !c->xchg && (c->cl.R <= KSG_SRV_MAX_R || srv_grid(c)) && !c->cl.dev.wide &&
         c->cl.N > 0;
}

static int srv_alloc(ksg_ctx* c) {
  if (c->srv.box) return KSG_OK;
  if (int rc = c->srv.box.alloc(c, 1)) return rc;
  memset(c->srv.box, 0, sizeof(KsgSrvBox));
  return KSG_OK;
}

// (Re)launches the server on the stream, offering every request after the last
// one answered. A COMMIT is posted without waiting for its answer, so the host's
// c->srv.served may lag the server's: the response block names the last request the
// server answered, and a server answers a request only once it will complete it
// (the one-workgroup server applies a COMMIT's delta after answering it, before
// it reads the next request or returns). Relaunching at c->srv.served alone would
// offer an answered COMMIT again and apply its delta twice.
static int srv_launch(ksg_ctx* c) {
  if (int rc = srv_alloc(c)) return rc;
  const uint32_t r0 = __atomic_load_n(&c->srv.box->resp[0], __ATOMIC_ACQUIRE);
  if ((int32_t)(r0 - c->srv.served) > 0) c->srv.served = r0;
  const uint32_t start_seq = c->srv.served;
  const size_t nf = ((size_t)(c->cl.hi - c->cl.lo) + 3 & ~(size_t)3) + 64;  // (the grid server stores 4 codes at a time)
  if (c->srv.fail.cap < nf)
    if (int rc = c->srv.fail.alloc(c, nf)) return rc;
  KsgSrvArgs a{c->srv.box.dp, c->srv.fail.dp, start_seq, (uint64_t)c->srv.idle_us * 100,
               (c->srv.stamps ? 1u : 0u) | (c->srv.debug ? 2u : 0u),
               nullptr, 0, ++c->srv.epoch, 0};
  if (srv_grid(c)) {
    const uint32_t n = c->cl.hi - c->cl.lo;
    if (!c->srv.grid)  // (zeroed on the stream, ahead of the launch)
      if (int rc = dalloc(c, c->srv.grid, 1)) return rc;
    a.grid = c->srv.grid;
    const uint32_t npt = srv_npt(c);
    a.n_workers = (n + KSG_GSRV_NT * npt - 1) / (KSG_GSRV_NT * npt);
    // past 64 scan workgroups their polls of the host block crowd the link: each sleeps ~0.2 us
    // more between polls (measured: 50,000 nodes 73 -> 38 us per pod; no gain at 15,000)
    a.grid_opts = c->srv.grid_opts >= 0 ? (uint32_t)c->srv.grid_opts : a.n_workers > 64 ? 0x10u : 0u;
    HIPCHK(c, ksg_launch_serve_grid((int)npt, c->ext_on, c->cl.dev, a, c->st));
  } else {
    HIPCHK(c, ksg_launch_serve(c->cl.R, anti_on(c), c->ext_on, c->cl.dev, a, c->st));
  }
  c->srv.running = true;
  ++c->srv.launches;
  return KSG_OK;
}

// Waits until request `seq` is answered: its response, or (a grid server's
// BEGIN, parts > 0) that many parts. A server that returned (idle) before it saw
// the request is relaunched to serve it.
static int srv_wait(ksg_ctx* c, uint32_t seq, uint32_t parts) {
  const uint32_t* rs = c->srv.box->resp;
  auto done = [&]() {
    if (!parts) return (int32_t)(__atomic_load_n(&rs[0], __ATOMIC_ACQUIRE) - seq) >= 0;  // (answered in order)
    for (uint32_t q = 0; q < parts; ++q)
      if (__atomic_load_n(&c->srv.box->part[q].seq, __ATOMIC_ACQUIRE) != seq ||
          __atomic_load_n(&c->srv.box->part[q].stamp[3], __ATOMIC_ACQUIRE) != seq)  // (both ends of the store)
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
      c->srv.running = false;
      if (c->srv.trace) fprintf(stderr, "srv relaunch start %u (waiting %u)\n", c->srv.served, seq);
      if (int rc = srv_launch(c)) return rc;  // (every request after the last answered one is offered again)
      t0 = std::chrono::steady_clock::now();
    } else if (q != hipErrorNotReady) {
      c->srv.running = false;
      std::string marks;
      if (c->srv.debug)  // where each workgroup was (seq:stage), leader first
        for (int i = 0; i < 12; ++i) {
          const uint32_t m = __atomic_load_n(&c->srv.box->dbg[i], __ATOMIC_RELAXED);
          marks += " " + std::to_string(m >> 8) + ":" + std::to_string(m & 255);
        }
      return fail(c, KSG_ERR_HIP, "drop-in server: %s (request %u%s)", hipGetErrorString(q), seq, marks.c_str());
    } else if (us > 5e6) {
      return fail(c, KSG_ERR_HIP, "drop-in server did not answer request %u in 5 s", seq);
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  if ((int32_t)(seq - c->srv.served) > 0) c->srv.served = seq;  // (and every request before it)
  return KSG_OK;
}

// The control block is free once the server has read the last COMMIT (posted
// without waiting for its answer): before the host writes a control request.
static int srv_settle(ksg_ctx* c) {
  if (!c->srv.unacked) return KSG_OK;
  const uint32_t u = c->srv.unacked;
  c->srv.unacked = 0;
  if ((int32_t)(c->srv.served - u) < 0)
    if (int rc = srv_wait(c, u, 0)) return rc;
  // resp[KSG_SRV_RESP_REJECTED]: the last request the server rejected, written before its
  // response (later BEGIN answers overwrite resp[0..3], not this word). The host mirror
  // already holds the commit's pod and the device does not: the context is diverged.
  if (__atomic_load_n(&c->srv.box->resp[KSG_SRV_RESP_REJECTED], __ATOMIC_ACQUIRE) == u) {
    c->diverged = true;
    return fail(c, KSG_ERR_STATE, "drop-in server rejected commit request %u (ksg_set_cluster resyncs)", u);
  }
  return KSG_OK;
}

// Posts request ++c->srv.seq (header dwords hdr[0..KSG_SRV_HDR_DW); the payload
// chunks were written by the caller): a BEGIN into `req`, a control request into
// `creq` once the last COMMIT there was read. A BEGIN carries the last control
// request before it (ARG).
static int srv_post(ksg_ctx* c, const uint32_t* hdr_in, uint32_t* seq_out) {
  if (!c->srv.running) {
    if (int rc = srv_launch(c)) return rc;
  }
  const bool ctl = hdr_in[KSG_SRVH_KIND] != KSG_SRV_BEGIN;
  if (ctl) {
    if (int rc = srv_settle(c)) return rc;
  }
  uint32_t hdr[KSG_SRV_HDR_DW];
  memcpy(hdr, hdr_in, sizeof hdr);
  if (!ctl) hdr[KSG_SRVH_ARG] = c->srv.last_ctl;
  if (c->cl.dbg_corrupt) {
    const uint32_t bit = hdr[KSG_SRVH_KIND] == KSG_SRV_COMMIT ? 1u : hdr[KSG_SRVH_KIND] == KSG_SRV_BEGIN ? 2u : 0u;
    if (c->cl.dbg_corrupt & bit) {
      hdr[KSG_SRVH_IDS_AT] = KSG_SRV_PAY_DW + 1;  // (past the payload: req_bad)
      c->cl.dbg_corrupt &= ~bit;
    }
  }
  const uint32_t seq = ++c->srv.seq;
  if (ctl) c->srv.last_ctl = seq;
  if (c->srv.trace)
    fprintf(stderr, "srv post %u kind %u arg %u served %u\n", seq, hdr[KSG_SRVH_KIND], hdr[KSG_SRVH_ARG], c->srv.served);
  uint32_t* req = ctl ? c->srv.box->creq : c->srv.box->req;
  for (uint32_t i = 0; i < KSG_SRV_HDR_DW; ++i) req[4 * (i / KSG_SRV_CHUNK_DW) + i % KSG_SRV_CHUNK_DW] = hdr[i];
  std::atomic_thread_fence(std::memory_order_release);  // data, then tags (x86: stores stay in order)
  for (uint32_t q = 0; q < KSG_SRV_CHUNKS; ++q) __atomic_store_n(&req[4 * q + 3], seq, __ATOMIC_RELEASE);
  *seq_out = seq;
  return KSG_OK;
}

// Posts a request and waits for its response {seq, a, b, c}.
static int srv_call(ksg_ctx* c, const uint32_t* hdr, uint32_t* resp4) {
  uint32_t seq = 0;
  if (int rc = srv_post(c, hdr, &seq)) return rc;
  if (int rc = srv_wait(c, seq, 0)) return rc;
  const uint32_t* rs = c->srv.box->resp;
  for (int i = 0; i < 4; ++i) resp4[i] = __atomic_load_n(&rs[i], __ATOMIC_RELAXED);
  if (c->srv.stamps && hdr[KSG_SRVH_KIND] == KSG_SRV_BEGIN && __atomic_load_n(&rs[10], __ATOMIC_RELAXED) == seq) {
    for (int i = 0; i < 6; ++i) c->srv.stage[i] += (int32_t)__atomic_load_n(&rs[4 + i], __ATOMIC_RELAXED);
    ++c->srv.stamped;
  }
  return KSG_OK;
}

// A BEGIN on either server: {k | ~0u (no peer) | KSG_SRV_BADREQ, max} and the
// tie words into c->pb.tw. The grid server's parts are merged here.
static int srv_begin(ksg_ctx* c, const uint32_t* hdr, uint32_t* resp4) {
  const uint32_t n = c->cl.hi - c->cl.lo, nwd = (n + 63) / 64;
  if (!srv_grid(c)) {
    if (int rc = srv_call(c, hdr, resp4)) return rc;
    if (resp4[1] != KSG_SRV_BADREQ && resp4[1] != ~0u && resp4[1] > 0)
      c->pb.tw.assign(c->srv.box->ties, c->srv.box->ties + nwd);
    return KSG_OK;
  }
  const uint32_t npt = srv_npt(c), G = (n + KSG_GSRV_NT * npt - 1) / (KSG_GSRV_NT * npt), NWG = 4 * npt;
  uint32_t seq = 0;
  if (int rc = srv_post(c, hdr, &seq)) return rc;
  if (int rc = srv_wait(c, seq, G)) return rc;
  const KsgSrvPart* pt = c->srv.box->part;
  int32_t M = KSG_S32_NONE;
  uint32_t err = 0;
  for (uint32_t q = 0; q < G; ++q) {
    M = std::max(M, pt[q].max);
    err |= pt[q].err;
  }
  uint32_t k = 0;
  c->pb.tw.assign((size_t)G * NWG, 0);
  if (M != KSG_S32_NONE)
    for (uint32_t q = 0; q < G; ++q)
      if (pt[q].max == M) {
        k += pt[q].cnt;
        const uint64_t* tw = npt == 1 ? pt[q].tie : c->srv.box->part_tie + (size_t)q * KSG_GSRV_TIEW;
        for (uint32_t r = 0; r < NWG; ++r) c->pb.tw[(size_t)q * NWG + r] = tw[r];
      }
  c->pb.tw.resize(nwd);
  if (c->srv.stamps) {  // worker 0: masks + loads, eval + publish (100-MHz ticks)
    c->srv.stage[0] += (int32_t)(pt[0].stamp[1] - pt[0].stamp[0]);
    c->srv.stage[1] += (int32_t)(pt[0].stamp[2] - pt[0].stamp[1]);  // (stamp[3]: the sequence number)
    ++c->srv.stamped;
  }
  resp4[0] = seq;
  resp4[1] = (err & 2) ? KSG_SRV_BADREQ : err ? ~0u : k;
  if (c->srv.trace) fprintf(stderr, "srv begin %u max %d k %u err %u\n", seq, M, k, err);
  const int64_t m64 = M;
  resp4[2] = (uint32_t)(uint64_t)m64;
  resp4[3] = (uint32_t)((uint64_t)m64 >> 32);
  return KSG_OK;
}

// What srv_call / srv_begin summed under KSG_SERVE_STAMPS=1, per begin (ksg_destroy prints it).
void srv_print_stamps(ksg_ctx* c) {
  if (!c->srv.stamped) return;
  const double n = (double)c->srv.stamped;
  const double* t = c->srv.stage;
  if (srv_grid(c))
    fprintf(stderr, "ksg grid serve stamps (10-ns ticks per begin, %llu begins, scan workgroup 0): request seen -> "
            "masks + loads done %.1f, -> eval + part stored %.1f\n", (unsigned long long)c->srv.stamped, t[0] / n, t[1] / n);
  else
    fprintf(stderr, "ksg serve stamps (s_memtime cycles per begin, %llu begins): to-LDS %.0f check %.0f resolve %.0f "
            "scan %.0f reduce %.0f fail-codes %.0f\n", (unsigned long long)c->srv.stamped, t[0] / n, t[1] / n, t[2] / n,
            t[3] / n, t[4] / n, t[5] / n);
}

// the t-th set bit (ascending) of the tie words -> node offset, -1 if none
static int64_t srv_pick(const std::vector<uint64_t>& tw, uint64_t t) {
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
  if (!c->srv.running) return KSG_OK;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = srv_settle(c)) return rc;  // (the last commit is applied first)
  if (hipStreamQuery(c->st) != hipSuccess) {
    uint32_t hdr[KSG_SRV_HDR_DW] = {KSG_SRV_EXIT};
    uint32_t r[4];
    if (int rc = srv_call(c, hdr, r)) return rc;
  }
  c->srv.running = false;
  // (a pending begin served by the server stays pending: its commit picks the node from
  // c->pb.tw on the host and posts the COMMIT to a relaunched server)
  HIPCHK(c, hipStreamSynchronize(c->st));
  return KSG_OK;
}

int srv_flush_patches(ksg_ctx* c) {
  if (int rc = srv_alloc(c)) return rc;
  size_t at = 0;
  while (at < c->patches.size()) {
    const uint32_t n = (uint32_t)std::min<size_t>(c->patches.size() - at, KSG_SRV_PATCHES);
    memcpy(c->srv.box->patch, c->patches.data() + at, (size_t)n * sizeof(KsgPatch));
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
static bool srv_put_pod(ksg_ctx* c, const ksg_pod* pod, const uint32_t* ids, size_t n_ids, const ksg_pod_ext* ext,
                 uint32_t* hdr, bool ctl = false) {
  const uint32_t pod_dw = (uint32_t)(sizeof(ksg_pod) / 4), ext_dw = (uint32_t)(sizeof(ksg_pod_ext) / 4);
  const uint32_t ids_at = pod_dw;
  const uint32_t ext_at = (ids_at + (uint32_t)n_ids + 1) & ~1u;  // 8-byte aligned
  const uint64_t paydw = ext ? (uint64_t)ext_at + ext_dw : (uint64_t)ids_at + n_ids;
  if (paydw > KSG_SRV_PAY_DW) return false;
  uint32_t* req = ctl ? c->srv.box->creq : c->srv.box->req;
  uint32_t* xa = ctl ? c->srv.box->cext : c->srv.box->ext;
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

#pragma GCC visibility pop

extern "C" {

// A begin's answer: max score m over k ties, to the caller's outputs; with k > 0 the pod is now
// pending (served: by the resident server, xr being the extension record its commit carries).
static int begin_answer(ksg_ctx* c, const ksg_pod* pod, const uint32_t* ids, size_t n_ids, int64_t m, uint64_t k,
                        bool served, const ksg_pod_ext* xr, int64_t* max_score, uint32_t* tie_count) {
  if (max_score) *max_score = k > 0 ? m : 0;
  if (tie_count) *tie_count = (uint32_t)k;
  if (k == 0) return KSG_NOFIT;
  c->pb.on = true;
  c->pb.k = k;
  c->pb.pod = *pod;
  c->pb.ids.assign(ids, ids + n_ids);
  c->pb.served = served;
  c->pb.ext_on = xr != nullptr;
  if (xr) c->pb.ext = *xr;
  return KSG_OK;
}

// The begin on the resident server: one request, no launch / copy / stream sync. *served = false,
// nothing done, where the context is not eligible or the pod does not fit the request block.
static int begin_served(ksg_ctx* c, const ksg_pod* pod, const uint32_t* ids, size_t ext, int64_t* max_score,
                        uint32_t* tie_count, uint8_t* fail_codes, bool* served) {
  *served = false;
  if (!srv_eligible(c)) return KSG_OK;
  int rc;
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
  if (!srv_put_pod(c, sp, ids, ext, xr, hdr)) return KSG_OK;
  *served = true;
  if ((rc = flush_patches(c)) || (!c->srv.running && (rc = srv_flush_patches(c)))) return rc;
  if (fail_codes) hdr[KSG_SRVH_FLAGS] |= KSG_SRVF_WANT_FAIL;
  uint32_t r[4];
  if ((rc = srv_begin(c, hdr, r))) return rc;
  // (the last COMMIT was served before this BEGIN: a rejected one diverged the context)
  if ((rc = srv_settle(c))) return rc;
  if (r[1] == KSG_SRV_BADREQ) return fail(c, KSG_ERR_STATE, "drop-in server rejected begin request");
  if (r[1] == ~0u) return fail(c, KSG_ERR_NOPEER, "service affinity peer is not on a known node");
  if (fail_codes) memcpy(fail_codes, c->srv.fail, (size_t)(c->cl.hi - c->cl.lo));
  const int64_t m = (int64_t)((uint64_t)r[2] | ((uint64_t)r[3] << 32));
  return begin_answer(c, pod, ids, ext, m, r[1], true, xr, max_score, tie_count);
}

// The begin as launches: scan [+ exchange], decide, one stream synchronise.
static int begin_launched(ksg_ctx* c, const ksg_pod* pod, const uint32_t* ids, size_t ext, int64_t* max_score,
                          uint32_t* tie_count, uint8_t* fail_codes) {
  int rc;
  if ((rc = srv_stop(c))) return rc;
  if ((rc = flush_patches(c))) return rc;
  if ((rc = ensure_map(c)) || (rc = upload_one(c, pod, ids, ext))) return rc;
  if ((rc = scan_exchange(c, c->one_pod, c->one_ids, KSG_MODE_BEGIN, fail_codes ? c->cl.d_fail : nullptr, nullptr,
                          c->ext_on ? c->d_one_ext : nullptr)))
    return rc;
  HIPCHK(c, ksg_launch_decide(c->cl.dev, c->one_pod, c->one_ids, rec_buf(c), c->cl.rec_bytes, c->world,
                              c->cl.d_shard_wlo, 0, 0, c->d_rng, nullptr, 0, reinterpret_cast<int64_t*>(c->h_map.dp),
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
  return begin_answer(c, pod, ids, ext, summ[0], (uint64_t)summ[1], false, nullptr, max_score, tie_count);
}

int ksg_schedule_begin(ksg_ctx* c, const ksg_pod* pod, const uint32_t* ids, int64_t* max_score,
                       uint32_t* tie_count, uint8_t* fail_codes) {
  if (!c || !pod) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (int rc0 = flush_deferred(c)) return rc0;
  if (int rs = cluster_ok(c)) return rs;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->pb.on) {  // the previous begin was abandoned: its queued updates apply now
    c->pb.clear();
    if (int rq = apply_queued(c)) return rq;
  }
  if (c->cl.N == 0) return KSG_NONODES;
  if (c->ext_on && !c->cur_ext) c->ext_scalar.erase(pod->uid);  // (plain entry point: no extension requests)
  const size_t ext = call_ids_extent(c, pod);
  int rc = check_pod(c, pod, ids, ext);
  if (rc) return rc;
  if ((rc = note_requests(c, pod, 1))) return rc;
  bool served;
  rc = begin_served(c, pod, ids, ext, max_score, tie_count, fail_codes, &served);
  if (rc || served) return rc;
  return begin_launched(c, pod, ids, ext, max_score, tie_count, fail_codes);
}

// The device half of a commit, decide the tie_index-th tie and apply AssumePod's delta, of a
// begin the resident server served: the node from the begin's tie words, the delta as a request.
static int commit_served(ksg_ctx* c, uint32_t tie_index, int32_t* node) {
  // the tie_index-th tie from the top (generic_scheduler.go:88-95)
  const int64_t off = srv_pick(c->pb.tw, c->pb.k - 1 - tie_index);
  if (off < 0 || off >= (int64_t)(c->cl.hi - c->cl.lo)) return fail(c, KSG_ERR_STATE, "commit selected no node");
  *node = (int32_t)(c->cl.lo + (uint32_t)off);
  // AssumePod's delta: one control request carrying the pod, not waited for (the next
  // BEGIN's scan waits on the device until it is applied)
  uint32_t hdr[KSG_SRV_HDR_DW] = {KSG_SRV_COMMIT};
  if (int rc = srv_settle(c)) return rc;  // (the control block is free)
  if (!srv_put_pod(c, &c->pb.pod, c->pb.ids.data(), c->pb.ids.size(), c->pb.ext_on ? &c->pb.ext : nullptr, hdr, true))
    return fail(c, KSG_ERR_STATE, "pending pod does not fit the request block");
  hdr[KSG_SRVH_ARG] = (uint32_t)*node;
  if (c->srv.trace) fprintf(stderr, "srv commit node %d\n", *node);
  uint32_t seq = 0;
  if (int rc = srv_post(c, hdr, &seq)) return rc;
  c->srv.unacked = seq;
  return KSG_OK;
}

// ... and of a launched begin: one decide launch and a stream synchronise.
static int commit_launched(ksg_ctx* c, uint32_t tie_index, int32_t* node) {
  int rc = ensure_map(c);
  if (rc) return rc;
  if ((rc = srv_stop(c))) return rc;
  // the pending pod is still in d_one (begin's upload; nothing re-uploads before the commit)
  HIPCHK(c, ksg_launch_decide(c->cl.dev, c->one_pod, c->one_ids, rec_buf(c), c->cl.rec_bytes, c->world,
                              c->cl.d_shard_wlo, 2, tie_index, c->d_rng, reinterpret_cast<int32_t*>(c->h_map.dp + 32), 0,
                              c->d_summary, c->st, c->ext_on ? c->d_one_ext : nullptr));
  HIPCHK(c, hipStreamSynchronize(c->st));
  memcpy(node, c->h_map + 32, 4);
  if (*node < 0) return fail(c, KSG_ERR_STATE, "commit selected no node (%d)", *node);
  return KSG_OK;
}

static int commit_on_device(ksg_ctx* c, uint32_t tie_index, int32_t* node) {
  HIPCHK(c, hipSetDevice(c->device));
  return c->pb.served ? commit_served(c, tie_index, node) : commit_launched(c, tie_index, node);
}

int ksg_schedule_commit(ksg_ctx* c, uint32_t tie_index, int32_t* out_node) {
  if (!c) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (!c->pb.on) return fail(c, KSG_ERR_STATE, "no schedule_begin pending");
  if (tie_index >= c->pb.k) return fail(c, KSG_ERR_ARG, "tie_index %u >= tie_count %llu", tie_index,
                                        (unsigned long long)c->pb.k);
  int32_t node = -1;
  int rc = commit_on_device(c, tie_index, &node);
  if (rc == KSG_OK) rc = mirror_add(c, (uint32_t)node, &c->pb.pod, c->pb.ids.data(), false);
  c->pb.clear();
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
  if (c->pb.on) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
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

int ksg_serve_stats(ksg_ctx* c, uint64_t* out4) {
  if (!c || !out4) return KSG_ERR_ARG;
  KSG_LOCK(c);
  out4[0] = c->srv.launches;
  out4[1] = c->srv.seq;
  out4[2] = c->srv.running ? 1 : 0;
  out4[3] = srv_eligible(c) ? (srv_grid(c) ? 2 : 1) : 0;
  return KSG_OK;
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

}  // extern "C"
