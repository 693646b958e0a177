// ksg_batch.cpp — the batch driver of libkschedgpu.so: ksg_schedule_batch and its variants
// (_draws, _ext), ksg_batch_unwind, ksg_set_window and the per-batch diagnostics. One batch is
// a sequence of phases over two small structs (WinPlan: what the window path's rounds only
// read; BatchRun: what the phases share and the deferred replay takes over on success):
//
//   batch_stage      validate, flush, upload the pods                   (host phases 0)
//   batch_begin      generator state, ev0, the extension records        (1)
//   use_window ?     win_plan -> rounds of win_enqueue_round / win_collect_round  (2, 3, 5)
//              :     exact_pods
//   overlap_work     the previous batch's mirror replay, under the device's work  (4, 7)
//   batch_publish    the deferred replay and the totals                 (7)
//
// The context, the scratch buffers and the helpers shared with the rest of the runtime
// (ksg_runtime.cpp; srv_stop is ksg_dropin.cpp's) are in ksg_host.h.
#include <cmath>
#include <cstring>

#include "ksg_host.h"
#include "ksg_shard.h"

namespace {

// The window path needs scores that commits can only lower (see ksg_window.hip):
// non-negative LeastRequested / ServiceSpreading weights and int64 totals far
// from wrapping (ServiceAntiAffinity is handled by its count pass and stops).
// The resolver walks the whole node set on every rank (state is replicated).
KsgDev full_geometry(const ksg_ctx* c) {
  KsgDev f = c->cl.dev;
  f.lo = 0;
  f.hi = c->cl.N;
  f.wlo = 0;
  f.nwords = c->cl.nw;
  return f;
}

// a pod's share of the window path's request budget: lr_win (ksg_device.h) is exact for
// 0 <= capacity, requested totals <= KSG_WIN_LR_BOUND (2^49)
// (each operand clamped first: two requests of 2^62 overflow the signed add)
int64_t win_request(const ksg_pod& p) {
  const int64_t lim = KSG_WIN_LR_BOUND;
  return std::min<int64_t>(std::min<int64_t>(p.milli_cpu, lim) + std::min<int64_t>(p.memory, lim), lim);
}

bool use_window(ksg_ctx* c, const ksg_pod* pods, uint32_t n) {
  if (c->window == 0 || c->cl.nw > 32 * 64 || ksg_win_max_window(full_geometry(c)) < 8) return false;
  // extensions: PodToleratesNodeTaints is static per (pod, node); extended
  // resources only shrink under commits and the resolver re-checks them on the
  // window's committed nodes like cpu / memory. With TaintToleration /
  // BalancedAllocation scores the resolver re-scores the committed nodes (a
  // BalancedAllocation score can RISE: ksg_plain.hip's risers and joiners); the
  // TaintToleration term needs the node taints as one mask (max_taints <= 64).
  // ServiceAntiAffinity, negative requests and requests past 2^16 take the exact
  // kernels.
  if (c->ext_on) {
    // ServiceAntiAffinity with the extensions: the window path only for the static filters —
    // PodToleratesNodeTaints, and extended resources no pod of the batch requests (a zero request
    // fits whatever the node's usage) — with both extension scores off: the anti-affinity
    // resolvers re-check nothing extension-specific on the window's committed nodes
    const bool anti = anti_on(c);
    if (anti && (c->ext.w_taint_toleration != 0 || c->ext.w_balanced != 0)) return false;
    if (c->ext.w_taint_toleration != 0 && !c->cl.dev.ntaint) return false;
    if (c->cur_ext)
      for (uint32_t i = 0; i < n; ++i)
        for (uint32_t r = 0; r < c->ext.n_scalar; ++r) {
          const int64_t v = c->cur_ext[i].scalar[r];
          if (anti && v != 0) return false;
          if (v < 0 || v > KSG_WIN_XREQ_BOUND) return false;
        }
  }
  // int64 combined scores
  if (c->cl.dev.wide) return false;
  // monotonicity under commits needs non-negative pod-dependent weights
  if (c->cfg.w_least_requested < 0 || c->cfg.w_service_spreading < 0) return false;
  const int64_t lim = KSG_WIN_LR_BOUND;
  if (c->cl.max_cap > lim || c->cl.min_cap < 0) return false;
  if (c->mu_dirty) {
    c->mu_max = 0;
    c->mu_neg = false;
    for (uint32_t i = 0; i < c->cl.N; ++i) {
      c->mu_neg |= c->mir.used_c[i] < 0 || c->mir.used_m[i] < 0;
      c->mu_max = std::max<int64_t>(c->mu_max, std::max<int64_t>(c->mir.used_c[i], c->mir.used_m[i]));
    }
    c->mu_dirty = false;
  }
  if (c->mu_neg) return false;
  const int64_t mu = c->mu_max;
  // commits not yet in the mirror (non-negative: checked by the caller) only add
  int64_t sum = c->dfr_sum;
  for (uint32_t i = 0; i < n; ++i) {
    if (pods[i].milli_cpu < 0 || pods[i].memory < 0) return false;
    sum += win_request(pods[i]);
    if (sum > lim) return false;
  }
  return mu + sum <= lim;
}

// ---- what the phases of one batch share -------------------------------------------
struct BatchRun {
  const ksg_pod* pods;
  const uint32_t* ids;
  uint32_t n, n_ids;
  // the placements and the generator state come back through pinned staging
  // (a pageable copy-out blocks the host until the stream drains); the window
  // path enqueues them with each round, which usually ends the batch, so the
  // host waits for the device once per batch
  size_t dn_rng = 0;  // h_dn: int32[n] placements, then (8-aligned) the generator state
  bool tail_queued = false;
  // this batch's deferred-replay inputs (pods, ids, every uid: the few pods that find no
  // node are taken out again after the wait), stashed here: they become the context's
  // deferred replay only when the batch succeeds; a failure after the device work started
  // leaves the context diverged until ksg_set_cluster
  bool stashed = false, dup_any = false;
  std::vector<ksg_pod> st_pods;
  std::vector<uint32_t> st_ids;
  std::unordered_set<uint64_t> st_uids;
  std::chrono::steady_clock::time_point t_last;  // host time per phase (ksg_last_batch_host_us)
};

void hphase(ksg_ctx* c, BatchRun& run, int k) {
  const auto t = std::chrono::steady_clock::now();
  c->last_hus[k] += std::chrono::duration<double, std::micro>(t - run.t_last).count();
  run.t_last = t;
}

int enqueue_tail(ksg_ctx* c, const BatchRun& run) {
  HIPCHK(c, hipEventRecord(c->ev1, c->st));
  HIPCHK(c, hipMemcpyAsync(c->h_dn, c->d_out, (size_t)run.n * 4, hipMemcpyDeviceToHost, c->st));
  HIPCHK(c, hipMemcpyAsync(c->h_dn + run.dn_rng, c->d_rng, 8, hipMemcpyDeviceToHost, c->st));
  return KSG_OK;
}

// Host work that overlaps the device: the previous batch's mirror replay, then
// this batch's deferred-replay inputs
int overlap_work(ksg_ctx* c, BatchRun& run) {
  if (run.stashed) return KSG_OK;
  int rc = flush_deferred(c);
  if (rc) return rc;
  hphase(c, run, 4);
  run.st_pods.assign(run.pods, run.pods + run.n);
  run.st_ids.assign(run.ids, run.ids + run.n_ids);
  run.st_uids.swap(c->dfr_uids);  // (empty after the flush: keeps its buckets)
  run.st_uids.reserve(2 * (size_t)run.n);
  for (uint32_t i = 0; i < run.n; ++i) run.dup_any |= !run.st_uids.insert(run.pods[i].uid).second;
  run.stashed = true;
  hphase(c, run, 7);
  return KSG_OK;
}

// the copies out, the overlapped host work and the wait that end a round or the batch
int finish_device(ksg_ctx* c, BatchRun& run, int wait_phase) {
  int rc;
  if ((rc = enqueue_tail(c, run))) return rc;
  hphase(c, run, 3);
  if ((rc = overlap_work(c, run))) return rc;  // the host mirror catches up while the device works
  if ((rc = wait_device(c))) return rc;
  hphase(c, run, wait_phase);
  return KSG_OK;
}

// keeps a half-done batch from being trusted: armed before the batch's first device
// operation, disarmed only on success
struct DivergeGuard {
  ksg_ctx* c;
  bool armed = false;
  ~DivergeGuard() {
    if (armed) {
      drop_deferred(c);
      c->diverged = true;
    }
  }
};

// validate the pods, bring the device state up to date, upload the batch
int batch_stage(ksg_ctx* c, BatchRun& run) {
  int rc;
  for (uint32_t i = 0; i < run.n; ++i) {
    if ((rc = check_pod(c, run.pods + i, run.ids, run.n_ids))) return rc;
    if (c->pods.count(run.pods[i].uid) || c->dfr_uids.count(run.pods[i].uid))
      return fail(c, KSG_ERR_ARG, "pod %u: duplicate uid", i);
  }
  hphase(c, run, 0);
  if ((rc = note_requests(c, run.pods, run.n))) return rc;
  if (c->dfr_neg && (rc = flush_deferred(c))) return rc;
  if ((rc = flush_patches(c))) return rc;
  if ((rc = upload_pods(c, run.pods, run.n, run.ids, run.n_ids))) return rc;
  if ((rc = c->d_out.grow(c, run.n))) return rc;
  run.dn_rng = ((size_t)run.n * 4 + 7) & ~(size_t)7;
  return c->h_dn.grow(c, run.dn_rng + 8);
}

// the batch's first device work: the generator state, ev0, and with extensions each pod's
// record (all-zero for the plain entry point) -> *dext
int batch_begin(ksg_ctx* c, BatchRun& run, const uint64_t* rng_state, const ksg_pod_ext** dext) {
  HIPCHK(c, hipMemcpyAsync(c->d_rng, rng_state, 8, hipMemcpyHostToDevice, c->st));
  HIPCHK(c, hipEventRecord(c->ev0, c->st));
  c->last_stats[0] = c->last_stats[1] = c->last_stats[2] = c->last_stats[3] = 0;
  c->last_kms[0] = c->last_kms[1] = c->last_kms[2] = c->last_t0ms = 0;
  c->last_wsum = 0;
  hphase(c, run, 1);
  *dext = nullptr;
  if (!c->ext_on) return KSG_OK;
  const size_t bytes = (size_t)run.n * sizeof(ksg_pod_ext);
  if (int rc = c->d_pext.grow(c, run.n)) return rc;
  if (c->cur_ext) {
    HIPCHK(c, hipMemcpyAsync(c->d_pext, c->cur_ext, bytes, hipMemcpyHostToDevice, c->st));
  } else {
    HIPCHK(c, hipMemsetAsync(c->d_pext, 0, bytes, c->st));
  }
  *dext = c->d_pext;
  return KSG_OK;
}

// The exact path for pods [first, first + count): one batch kernel on one rank; on a sharded
// context per pod scan + record exchange + decide. The whole batch when the window path is
// off, one pod when the window path met a pod whose id lists exceed the window record.
int exact_pods(ksg_ctx* c, uint32_t first, uint32_t count, const ksg_pod_ext* dext) {
  if (!c->xchg) {
    HIPCHK(c, ksg_launch_batch(c->cl.R, anti_on(c), c->cl.dev, c->d_pods + first, c->d_ids, count, c->d_rng,
                               c->d_out + first, c->st, dext ? dext + first : nullptr));
    return KSG_OK;
  }
  for (uint32_t i = first; i < first + count; ++i) {
    if (int rc = scan_exchange(c, c->d_pods + i, c->d_ids, KSG_MODE_BEGIN, nullptr, nullptr, dext ? dext + i : nullptr))
      return rc;
    HIPCHK(c, ksg_launch_decide(c->cl.dev, c->d_pods + i, c->d_ids, rec_buf(c), c->cl.rec_bytes, c->world,
                                c->cl.d_shard_wlo, 1, 0, c->d_rng, c->d_out, i, c->d_summary, c->st,
                                dext ? dext + i : nullptr));
  }
  return KSG_OK;
}

// ---- the window path ----------------------------------------------------------------
// Phase A scores the window on this rank's shard; with world > 1 the per-word results are
// all-gathered once per window (not per pod) and every rank runs the same resolver over the
// whole replicated node state, so every rank commits the same pods to the same nodes.
struct WinPlan {
  KsgDev full;    // the resolver's geometry: the whole node set
  uint32_t W;     // window capacity of this batch's launches
  KsgWinXchg x;   // the exchange block's layout and the per-window arrays
  bool anti;      // ServiceAntiAffinity: count pass, the anti resolvers
  bool rr;        // ... its re-rank
  bool esc;       // extension scores on the plain resolver
  bool etm;       // ... TaintToleration among them: its count pass
  bool d1;        // phase A's single-commit drop bitmaps
  bool plain;     // the plain resolver (reads T0 images)
  bool fused;     // one launch per window (KsgFused)
  uint32_t fgroups;
  size_t fit_off, dcnt_n;
  uint64_t* wbits;
  int32_t* wmax;
  const ksg_pod_ext* dext;
};

// Lays out the exchange block, grows the window buffers and enqueues their first zeroing
// (the resolvers re-zero them for the next window). The one place that knows the block's
// layout. One rank's block (x.blk bytes, 256-aligned; a row is x.ostride 64-node words, R =
// W x ostride), and who reads what:
//
//   offset             type       flag   written by                read by
//   0                  u64[R]     all    phase A (wbits)           T0 images / resolver
//   8 R                i32[R]     all    phase A (wmax)            T0 images / resolver
//   fit_off = a8(12R)  u64[R]     one of:
//     x.fit_off                   anti   score pass: fit bitmaps   the anti resolvers
//     x.efit_off                  esc    phase A: fit bitmaps      plain resolver, extension scores
//     x.d1_off                    d1     phase A: drop bitmaps     plain resolver's committer (x_fast)
//   x.b_off = fit_off + 8 R  u64[R]  rr  score pass: nodes at their row's best   re-rank resolver
//
// anti, esc and d1 exclude each other (use_window keeps extension scores off an anti context;
// d1 needs a context without either), so the three offsets alias one region.
int win_plan(ksg_ctx* c, uint32_t n, const ksg_pod_ext* dext, WinPlan* pl) {
  int rc;
  pl->dext = dext;
  pl->full = full_geometry(c);
  uint32_t W = std::min(c->window, ksg_win_max_window(pl->full));
  // Phase A scores all W pods of a window whatever the resolver gets through.
  // Where windows stop early (ServiceAntiAffinity: every ~13 pods on config 4)
  // the capacity follows the pods per window measured on earlier batches: 3x
  // that, in pod groups of 8, at least 16. (A sharded context keeps W: every
  // rank must size its launches alike, and its estimate restarts each batch.)
  if (!c->xchg && c->ppw_est > 0.0) {
    const uint32_t want = ((uint32_t)std::ceil(3.0 * c->ppw_est) + 7u) & ~7u;
    W = std::min(W, std::max<uint32_t>(want, 16u));
  }
  pl->W = W;
  KsgWinXchg& x = pl->x;
  x = KsgWinXchg{};
  x.exts = dext;  // (extensions: the filters, and the scores when esc)
  x.ostride = std::max<uint32_t>(c->cl.nwords_max, 1);
  x.wcap = W;
  x.world = (uint32_t)c->world;
  for (int g = 0; g < c->world; ++g) {
    uint32_t a, b;
    ksg_shard_words(c->cl.nw, (uint32_t)g, (uint32_t)c->world, &a, &b);
    x.wlo[g] = a;
    x.nw[g] = b - a;
  }
  const bool anti = pl->anti = anti_on(c);
  const bool rr = pl->rr = anti && c->cl.dev.rr_dz != 0 && c->cl.d_zmap;  // ServiceAntiAffinity re-rank
  const size_t fit_off = pl->fit_off = ((size_t)W * x.ostride * 12 + 7) & ~(size_t)7;
  // (the domain counts are zeroed once here, then by each resolver for the next window)
  x.fit_off = anti ? (uint32_t)fit_off : 0u;
  x.b_off = rr ? (uint32_t)(fit_off + (size_t)W * x.ostride * 8) : 0u;
  // extension scores on the plain resolver: the pods' fit bitmaps at the same offset
  const bool esc = pl->esc = c->ext_on && (c->ext.w_taint_toleration != 0 || c->ext.w_balanced != 0);
  pl->etm = esc && c->ext.w_taint_toleration != 0;  // (the TaintToleration count pass)
  x.esc = esc ? 1u : 0u;
  x.efit_off = esc ? (uint32_t)fit_off : 0u;
  // the plain resolver without extensions up to 16,384 nodes (its ring holds the bitmaps):
  // phase A's single-commit drop bitmaps at the same offset
  const bool d1 = pl->d1 = !anti && !dext && c->cl.win_d1 && c->cl.nw <= 4 * 64;
  x.d1 = d1 ? 1u : 0u;
  x.d1_off = d1 ? (uint32_t)fit_off : 0u;
  x.blk = ((rr                  ? fit_off + (size_t)W * x.ostride * 16
            : anti || esc || d1 ? fit_off + (size_t)W * x.ostride * 8
                                : (size_t)W * x.ostride * 12) +
           255) & ~(size_t)255;
  if (esc) {
    if ((rc = c->d_etmax.grow(c, W)) || (rc = c->d_ethist.grow(c, (size_t)W * KSG_TBINS)) ||
        (rc = c->d_epsoft.grow(c, W)))
      return rc;
    // (zero once here; each resolver zeroes them again for the next window's count pass)
    HIPCHK(c, hipMemsetAsync(c->d_etmax, 0, (size_t)W * sizeof(int32_t), c->st));
    HIPCHK(c, hipMemsetAsync(c->d_ethist, 0, (size_t)W * KSG_TBINS * sizeof(int32_t), c->st));
    x.tmax = c->d_etmax;
    x.thist = c->d_ethist;
    x.psoft = c->d_epsoft;
  }
  const size_t dcnt_n = pl->dcnt_n = (size_t)W * std::max<uint32_t>(c->cl.D, 1);
  if (anti) {
    if ((rc = c->d_dcnt.grow(c, dcnt_n))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_dcnt, 0, dcnt_n * sizeof(int32_t), c->st));
    x.dcnt = c->d_dcnt;
    x.dcnt_n = (uint32_t)dcnt_n;
  }
  if (rr) {  // (the resolver resets the row bests to KSG_S32_NONE and the B counts to 0 for the next window)
    const size_t dmb_n = (size_t)W * c->cl.dev.rr_dz;  // [W][dz] row bests, then [W][dz] B nodes per row
    if ((rc = c->d_dmb.grow(c, 2 * dmb_n))) return rc;
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->d_dmb.p, (int)0x80000000, dmb_n, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_dmb + dmb_n, 0, dmb_n * sizeof(int32_t), c->st));
    x.rr = 1;
    x.dz = c->cl.dev.rr_dz;
    x.dmb = c->d_dmb;
    x.zmap = c->cl.d_zmap;
  }
  if ((rc = c->d_winsum.grow(c, W))) return rc;
  if ((rc = c->d_xsend.grow(c, x.blk))) return rc;
  if (c->xchg && (rc = c->d_xrecv.grow(c, x.blk * c->world))) return rc;
  x.buf = c->xchg ? c->d_xrecv.p : c->d_xsend.p;
  pl->plain = !anti;  // the plain resolver reads T0 images
  if (pl->plain) {
    x.img_stride = ksg_win_t0_stride(pl->full);
    if ((rc = c->d_t0img.grow(c, (size_t)W * x.img_stride))) return rc;
    x.img = c->d_t0img;
  }
  // one launch per window (KsgFused): one rank, no ServiceAntiAffinity, no extensions
  pl->fgroups = pl->plain && !c->xchg && !dext && c->win_fused && pl->full.nwords <= c->fused_max_words &&
                        ksg_win_fused_ok(pl->full)
                    ? ksg_win_fused_groups(pl->full, W) : 0u;
  pl->fused = pl->fgroups > 0 && pl->fgroups <= kFctlGroups;
  pl->wbits = reinterpret_cast<uint64_t*>(c->d_xsend.p);
  pl->wmax = reinterpret_cast<int32_t*>(c->d_xsend + (size_t)W * x.ostride * 8);
  return KSG_OK;
}

// Windows per round: from the pods per window the previous rounds resolved
// (windows stop early on service / exhaustion / slot events, e.g. every ~13
// pods with ServiceAntiAffinity), 10% over; launches past the batch's end
// return at once. Fewer rounds = fewer host synchronisations per batch.
uint32_t round_k(const ksg_ctx* c, uint32_t W, double ppw_est, uint32_t left) {
  const double ppw = ppw_est > 0.0 ? std::min<double>(std::max(ppw_est, 1.0), (double)W) : 0.8 * W;
  const double k = std::ceil((double)left / ppw * c->round_margin) + 1.0;
  return (uint32_t)std::min(k, 8192.0);
}

// One round on the stream: the run record (from pod `pos` of n) up, K window launches in
// their form (fused; else [anti count pass] [TaintToleration count pass] score pass, T0
// images, resolver, with the sharded collectives between them), events around the sampled
// launches (k with (k + ev_off) % es == 0), the run record back.
int win_enqueue_round(ksg_ctx* c, const WinPlan& pl, uint32_t pos, uint32_t n, uint32_t K, uint32_t es,
                      uint32_t ev_off) {
  int rc;
  const KsgWinXchg& x = pl.x;
  const uint32_t W = pl.W;
  KsgWinRun* const fruns = reinterpret_cast<KsgWinRun*>(c->d_fctl.p);
  uint32_t* const fcnt = reinterpret_cast<uint32_t*>(c->d_fctl + kFctlRuns);
  *c->h_run = KsgWinRun{pos, n, 0, 0, {0, 0, 0, 0}};
  if (pl.fused) {  // slot 0 and both counter sets (the launches zero the next set as they go)
    *reinterpret_cast<KsgWinRun*>(c->h_fctl.p) = *c->h_run;
    HIPCHK(c, hipMemcpyAsync(c->d_fctl, c->h_fctl, kFctlRuns + (size_t)2 * pl.fgroups * 8 * sizeof(uint32_t),
                             hipMemcpyHostToDevice, c->st));
  } else {
    HIPCHK(c, hipMemcpyAsync(c->d_run, c->h_run, sizeof(KsgWinRun), hipMemcpyHostToDevice, c->st));
  }
  HIPCHK(c, hipEventRecord(c->wev[0], c->st));
  for (uint32_t k = 0; k < K; ++k) {
    // HIP events on this stream around the sampled launches (per-kernel device time)
    const bool evk = es && (k + ev_off) % es == 0;
    // (launch k: events 3k before phase A, 3k+1 after it, 3k+2 before the resolver, 3k+3 =
    // the next launch's 3(k+1) after it; the fused launch: 3k before it, 3k+3 after it)
    if (evk && k > 0) HIPCHK(c, hipEventRecord(c->wev[3 * k], c->st));
    if (pl.fused) {
      // the counter rows: fgroups per set, set k & 1 (the host zeroed both for launch 0; each
      // launch's block 0 zeroes the other set for the next launch)
      KsgFused f{c->d_pods, c->d_ids, fruns + ((k + 1) & 1), fcnt, k & 1u, pl.fgroups};
      HIPCHK(c, ksg_launch_win_fused(pl.full, W, fruns + (k & 1), c->d_winsum, x, c->d_rng, c->d_out, f,
                                     c->fused_grid, c->st));
      if (evk) HIPCHK(c, hipEventRecord(c->wev[3 * k + 3], c->st));
      continue;
    }
    if (pl.anti) {
      // ServiceAntiAffinity: the pods' per-domain counts over their filtered nodes first
      // (into d_dcnt, zero: the previous resolver cleared it)
      HIPCHK(c, ksg_launch_win_eval(c->cl.dev, 1, c->d_pods, c->d_ids, c->d_run, W, c->d_winsum, pl.wbits, pl.wmax,
                                    x.ostride, c->d_dcnt, nullptr, x.dmb, nullptr, x.dz, c->st, pl.dext));
      if (c->xchg && (rc = allreduce_i32(c, Reduce::Sum, c->d_dcnt, c->d_dcnt, (uint32_t)pl.dcnt_n))) return rc;
    }
    if (pl.etm) {  // TaintToleration: each pod's max soft-taint count over its filtered nodes first
      HIPCHK(c, ksg_launch_win_eval(c->cl.dev, 3, c->d_pods, c->d_ids, c->d_run, W, c->d_winsum, pl.wbits, pl.wmax,
                                    x.ostride, nullptr, nullptr, nullptr, nullptr, 0, c->st, pl.dext, x.tmax,
                                    x.psoft, x.thist));
      // sharded: over every shard's filtered nodes (the max, and the histogram of soft
      // counts whose bin at the max the resolver's normalisation stop reads)
      if (c->xchg && ((rc = allreduce_i32(c, Reduce::Max, x.tmax, x.tmax, W)) ||
                      (rc = allreduce_i32(c, Reduce::Sum, x.thist, x.thist, W * KSG_TBINS))))
        return rc;
    }
    HIPCHK(c, ksg_launch_win_eval(c->cl.dev, pl.anti ? 2 : 0, c->d_pods, c->d_ids, c->d_run, W, c->d_winsum, pl.wbits,
                                  pl.wmax, x.ostride, c->d_dcnt,
                                  (pl.anti || pl.esc || pl.d1) ? reinterpret_cast<uint64_t*>(c->d_xsend + pl.fit_off)
                                                               : nullptr,
                                  x.dmb, pl.rr ? reinterpret_cast<uint64_t*>(c->d_xsend + x.b_off) : nullptr, x.dz,
                                  c->st, pl.dext, x.tmax, x.psoft));
    if (evk) HIPCHK(c, hipEventRecord(c->wev[3 * k + 1], c->st));
    if (c->xchg && (rc = allgather(c, c->d_xsend, c->d_xrecv, x.blk))) return rc;
    if (pl.plain) HIPCHK(c, ksg_launch_win_t0(pl.full, W, c->d_run, x, c->st));
    if (evk) HIPCHK(c, hipEventRecord(c->wev[3 * k + 2], c->st));
    HIPCHK(c, ksg_launch_win_resolve(pl.full, W, c->d_run, c->d_winsum, x, c->d_rng, c->d_out, c->st));
    if (evk) HIPCHK(c, hipEventRecord(c->wev[3 * k + 3], c->st));
  }
  HIPCHK(c, hipMemcpyAsync(c->h_run, pl.fused ? fruns + (K & 1) : c->d_run.p, sizeof(KsgWinRun),
                           hipMemcpyDeviceToHost, c->st));
  return KSG_OK;
}

// After the round's wait: the run record -> *r, the pods-per-window estimate, the sampled
// event times scaled to the round's K launches, the stats, and the resolver's halts as errors.
int win_collect_round(ksg_ctx* c, const WinPlan& pl, uint32_t n, uint32_t K, uint32_t es, uint32_t ev_off,
                      uint32_t pos, double* ppw_est, KsgWinRun* out) {
  const KsgWinRun r = *out = *c->h_run;
  if (r.windows > 0 && r.pos > pos) {  // pods per window, smoothed over rounds and batches
    const double ppw = (double)(r.pos - pos) / (double)r.windows;
    *ppw_est = *ppw_est > 0.0 ? 0.5 * *ppw_est + 0.5 * ppw : ppw;
    if (!c->xchg) c->ppw_est = *ppw_est;
  }
  // the sampled launches (every one of the round's launches is a sampling
  // candidate, including the ones after the batch was done, which return at
  // once, so the mean matches a kernel trace of the run), scaled to all K
  double ea = 0.0, eb = 0.0, et = 0.0;
  uint32_t nt = 0;
  for (uint32_t k = es ? (es - ev_off) % es : 0u; es && k < K; k += es) {
    float a = 0.f, t0 = 0.f, b = 0.f;
    if (pl.fused) {  // (one kernel: its whole time is the resolver's, phase A runs inside it)
      HIPCHK(c, hipEventElapsedTime(&b, c->wev[3 * k], c->wev[3 * k + 3]));
    } else {
      HIPCHK(c, hipEventElapsedTime(&a, c->wev[3 * k], c->wev[3 * k + 1]));
      HIPCHK(c, hipEventElapsedTime(&t0, c->wev[3 * k + 1], c->wev[3 * k + 2]));
      HIPCHK(c, hipEventElapsedTime(&b, c->wev[3 * k + 2], c->wev[3 * k + 3]));
    }
    ea += a;
    et += t0;
    eb += b;
    ++nt;
  }
  if (nt) {
    c->last_kms[0] += ea * K / nt;
    c->last_kms[1] += eb * K / nt;
    c->last_t0ms += et * K / nt;
  }
  c->last_kms[2] += K;
  c->last_wsum += (double)pl.W * K;
  c->last_stats[0] += r.windows;
  for (int q = 1; q <= 3; ++q) c->last_stats[q] += r.stops[q];
  if (c->dbg_fail_next) {
    c->dbg_fail_next = false;
    return fail(c, KSG_ERR_STATE, "window resolver: injected failure (KSG_DEBUG & 16384) at pod %u", r.pos);
  }
  if (r.halt == KSG_HALT_HANG) return fail(c, KSG_ERR_STATE, "window resolver: ring wait timed out at pod %u", r.pos);
  if (r.halt == KSG_HALT_BAD)
    return fail(c, KSG_ERR_STATE,
                "window resolver: selection outside T0 at pod %u (inconsistent prefixes or drop positions: a bug, "
                "or stale verdicts under the KSG_DEBUG timing switches)", r.pos);
  if (r.halt == KSG_HALT_BADCOUNT || r.pos < pos || r.pos > n)
    return fail(c, KSG_ERR_STATE, "window resolver: bad progress (halt %u, pos %u -> %u)", r.halt, pos, r.pos);
  return KSG_OK;
}

// Windows are chained on the device: each kernel reads the window's start
// from d_run (written by the previous resolver), so the host enqueues a
// round of windows and synchronises once per round, not once per window.
// A sharded context issues one collective per launch, so every rank must
// enqueue the same number of launches: its estimate starts fresh each batch
// and follows only this batch's progress, which every rank resolves alike.
int win_rounds(ksg_ctx* c, const WinPlan& pl, BatchRun& run) {
  int rc;
  const uint32_t n = run.n;
  double ppw_est = c->xchg ? 0.0 : c->ppw_est;
  uint32_t pos = 0, K = round_k(c, pl.W, ppw_est, n);
  hphase(c, run, 2);
  while (pos < n) {
    if (c->wev.size() < 3 * (size_t)K + 1) {
      const size_t old = c->wev.size();
      c->wev.resize(3 * (size_t)K + 1);
      for (size_t i = old; i < c->wev.size(); ++i) HIPCHK(c, hipEventCreateWithFlags(&c->wev[i].e, kTimingEvent));
    }
    // the sampled launches rotate from round to round (launches k with
    // (k + ev_off) % es == 0), so every position in a round, the no-op
    // launches after the batch's end included, is timed equally often
    const uint32_t es = std::min(c->ev_stride, K);  // (a short round still times one launch)
    const uint32_t ev_off = es ? c->ev_phase++ % es : 0u;
    if ((rc = win_enqueue_round(c, pl, pos, n, K, es, ev_off))) return rc;
    if ((rc = finish_device(c, run, 5))) return rc;
    KsgWinRun r;
    if ((rc = win_collect_round(c, pl, n, K, es, ev_off, pos, &ppw_est, &r))) return rc;
    pos = r.pos;
    run.tail_queued = pos >= n && r.halt != KSG_HALT_OVERSIZE;  // (the copies saw the finished batch)
    if (r.halt == KSG_HALT_OVERSIZE) {
      // a pod whose id lists exceed the window record: the exact per-pod path
      if ((rc = exact_pods(c, pos, 1, pl.dext))) return rc;
      pos += 1;
      ++c->last_stats[3];
    }
    // next round (rare: stops shortened this round's windows): the rest at W/2 pods per window
    K = round_k(c, pl.W, ppw_est, n - std::min(pos, n));
    hphase(c, run, 2);
  }
  return KSG_OK;
}

// The device applied every commit; the host mirror replays them later (flush_deferred),
// overlapped with the next batch's device work: the stashed inputs become the context's
// deferred replay, with what use_window and note_requests need to know of it before then.
int batch_publish(ksg_ctx* c, BatchRun& run, int32_t* out_nodes) {
  const ksg_pod* pods = run.pods;
  const uint32_t n = run.n;
  if (c->ext_on && !c->cur_ext)  // (plain entry point: the pods carry no extension requests)
    for (uint32_t i = 0; i < n; ++i) c->ext_scalar.erase(pods[i].uid);
  c->dfr_pods.swap(run.st_pods);
  c->dfr_ids.swap(run.st_ids);
  c->dfr_uids.swap(run.st_uids);
  c->dfr_out.assign(out_nodes, out_nodes + n);
  for (uint32_t i = 0; i < n; ++i)  // the uids of the pods that found no node are free again
    if (out_nodes[i] < 0 && !run.dup_any) c->dfr_uids.erase(pods[i].uid);
  if (run.dup_any) {  // a uid repeats within the batch: an error iff two placed pods share it
    for (uint32_t i = 0; i < n; ++i) c->dfr_uids.erase(pods[i].uid);
    for (uint32_t i = 0; i < n; ++i)
      if (out_nodes[i] >= 0 && !c->dfr_uids.insert(pods[i].uid).second)  // (mirror_add reports it at the replay)
        return fail(c, KSG_ERR_ARG, "pod %u: duplicate uid within the batch", i);
  }
  for (uint32_t i = 0; i < n; ++i) {
    if (out_nodes[i] < 0) continue;
    // (this batch's commits reach the mirror, and used_hi, at the next flush_deferred)
    c->dfr_req += (uint64_t)std::max<int64_t>(std::max(pods[i].milli_cpu, pods[i].memory), 0);
    if (pods[i].milli_cpu < 0 || pods[i].memory < 0) c->dfr_neg = true;
    else c->dfr_sum = std::min<int64_t>(c->dfr_sum + win_request(pods[i]), KSG_WIN_LR_BOUND + 1);
  }
  hphase(c, run, 7);
  double* t = c->totals;  // (layout: ksg_batch_totals in kschedgpu.h)
  t[0] += 1;
  t[1] += c->last_ms;
  for (int q = 0; q < 3; ++q) t[2 + q] += c->last_kms[q];
  t[17] += c->last_wsum;
  t[18] += c->last_t0ms;
  for (int q = 0; q < 4; ++q) t[5 + q] += c->last_stats[q];
  for (int q = 0; q < 8; ++q) t[9 + q] += c->last_hus[q];
  return KSG_OK;
}

}  // namespace

extern "C" {

int ksg_schedule_batch(ksg_ctx* c, const ksg_pod* pods, uint32_t n, const uint32_t* ids, uint32_t n_ids,
                       uint64_t* rng_state, int32_t* out_nodes) {
  if (!c || (n && (!pods || !out_nodes)) || !rng_state) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (c->pb.on) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
  if (int rs_ = srv_stop(c)) return rs_;  // (the resident server leaves the stream)
  if (int rs = cluster_ok(c)) return rs;
  HIPCHK(c, hipSetDevice(c->device));
  c->last_ms = 0.0;
  if (n == 0) return KSG_OK;
  if (c->cl.N == 0) {
    for (uint32_t i = 0; i < n; ++i) out_nodes[i] = KSG_OUT_NONODES;
    return KSG_OK;
  }
  for (double& v : c->last_hus) v = 0.0;
  BatchRun run{pods, ids, n, n_ids};
  run.t_last = std::chrono::steady_clock::now();
  int rc;
  if ((rc = batch_stage(c, run))) return rc;
  DivergeGuard guard{c};
  if (c->cl.dev.dbg & 16384) c->dbg_fail_next = true;  // KSG_DEBUG & 16384: fail the batch after its device work
  guard.armed = true;  // device work from here on
  const ksg_pod_ext* dext = nullptr;
  if ((rc = batch_begin(c, run, rng_state, &dext))) return rc;
  if (use_window(c, pods, n)) {
    WinPlan plan;
    if ((rc = win_plan(c, n, dext, &plan)) || (rc = win_rounds(c, plan, run))) return rc;
  } else if ((rc = exact_pods(c, 0, n, dext))) {
    return rc;
  }
  if (!run.tail_queued && (rc = finish_device(c, run, 6))) return rc;
  memcpy(out_nodes, c->h_dn, (size_t)n * 4);
  memcpy(rng_state, c->h_dn + run.dn_rng, 8);
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->last_ms = ms;
  if (!run.stashed)  // (overlap_work ran on every path that reaches here)
    return fail(c, KSG_ERR_STATE, "internal: batch replay inputs missing");
  guard.armed = false;
  return batch_publish(c, run, out_nodes);
}

int ksg_schedule_batch_draws(ksg_ctx* c, const ksg_pod* pods, uint32_t n, const uint32_t* ids, uint32_t n_ids,
                             const uint64_t* draws, uint32_t n_draws, uint32_t* draws_used, int32_t* out_nodes) {
  if (!c || (n && (!pods || !out_nodes || !draws)) || !draws_used) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (n_draws < n) return fail(c, KSG_ERR_ARG, "%u draws for %u pods: one per pod that may find a node", n_draws, n);
  for (uint32_t k = 0; k < n; ++k)
    if (draws[k] > (uint64_t)INT64_MAX) return fail(c, KSG_ERR_ARG, "draw %u is not a rand.Int() value", k);
  *draws_used = 0;
  if (c->pb.on) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
  if (n == 0) return ksg_schedule_batch(c, pods, 0, ids, n_ids, &c->draw_tmp, out_nodes);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rs_ = srv_stop(c)) return rs_;
  if (int rc = c->d_draws.grow(c, n)) return rc;
  HIPCHK(c, hipMemcpy(c->d_draws, draws, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice));
  c->cl.dev.draws = c->d_draws;  // (the generator state is now the index of the next value)
  uint64_t state = 0;
  const int rc = ksg_schedule_batch(c, pods, n, ids, n_ids, &state, out_nodes);
  c->cl.dev.draws = nullptr;
  if (rc == KSG_OK) *draws_used = (uint32_t)state;
  return rc;
}

// A rejected Bind in batch mode (scheduler.go:107-112: no AssumePod for pod k, its rand.Int()
// already drawn at generic_scheduler.go:94, pod k + 1 scheduled against the state without it).
// The batch committed pods 0..n-1 in order, so undoing the commits of pods n-1 down to k leaves
// exactly the state after pods 0..k-1; pods k+1..n-1 are then re-batched by the caller with the
// draws they had consumed put back (a splitmix64 state is stepped back over them instead).
int ksg_batch_unwind(ksg_ctx* c, const ksg_pod* pods, const int32_t* out_nodes, uint32_t n, uint32_t k,
                     uint64_t* rng_state, uint32_t* draws_kept) {
  if (!c || !pods || !out_nodes || !draws_kept || k >= n) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (c->pb.on) return fail(c, KSG_ERR_STATE, "schedule_begin pending");
  if (out_nodes[k] < 0) return fail(c, KSG_ERR_ARG, "pod %u found no node: there was no Bind to reject", k);
  if (int rs = cluster_ok(c)) return rs;
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc0 = flush_deferred(c)) return rc0;  // (the batch's commits into the host mirror)
  // (validate every uid before removing any: a failed call changes nothing)
  for (uint32_t i = k; i < n; ++i)
    if (out_nodes[i] >= 0 && !c->pods.count(pods[i].uid))
      return fail(c, KSG_ERR_ARG, "pod %u (uid %llu) is not a committed pod of this context", i,
                  (unsigned long long)pods[i].uid);
  uint32_t kept = 0, back = 0;
  for (uint32_t i = 0; i <= k; ++i) kept += out_nodes[i] >= 0 ? 1u : 0u;
  for (uint32_t i = n; i-- > k;) {  // newest first
    if (out_nodes[i] < 0) continue;
    if (i > k) ++back;
    if (int rc = remove_pod_impl(c, pods[i].uid)) return rc;
  }
  if (rng_state) *rng_state -= (uint64_t)back * ksg_rng_step(nullptr);
  *draws_kept = kept;
  return flush_patches(c);
}

int ksg_schedule_batch_ext(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                           uint32_t n_ids, uint64_t* rng_state, int32_t* out_nodes) {
  if (!c || (n && (!pods || !out_nodes)) || !rng_state) return KSG_ERR_ARG;
  KSG_LOCK(c);
  if (ext && !c->ext_on) return fail(c, KSG_ERR_STATE, "extensions are off");
  // validate the whole batch first; each placed pod's extended-resource requests
  // are recorded (for the host mirror's deferred replay) only once the batch
  // succeeded, and the pods that found no node leave no entry
  if (c->ext_on && ext)
    for (uint32_t i = 0; i < n; ++i) {
      if (int rc = check_ext_range(c, ext + i, n_ids)) return rc;
      if (int rc = check_taint_ids(c, ext + i, ids)) return rc;
    }
  c->cur_ext = ext;
  const int rc = ksg_schedule_batch(c, pods, n, ids, n_ids, rng_state, out_nodes);
  c->cur_ext = nullptr;
  if (rc == KSG_OK && c->ext_on && ext)
    for (uint32_t i = 0; i < n; ++i) {
      if (out_nodes[i] >= 0) (void)note_ext(c, pods + i, ext + i, n_ids);
      else c->ext_scalar.erase(pods[i].uid);
    }
  return rc;
}

int ksg_set_window(ksg_ctx* c, uint32_t window) {
  if (!c) return KSG_ERR_ARG;
  KSG_LOCK(c);
  c->window = window;
  c->ppw_est = 0.0;
  return KSG_OK;
}

int ksg_last_batch_stats(ksg_ctx* c, uint32_t* stats4) {
  if (!c || !stats4) return KSG_ERR_ARG;
  KSG_LOCK(c);
  for (int i = 0; i < 4; ++i) stats4[i] = c->last_stats[i];
  return KSG_OK;
}

int ksg_last_batch_kernel_ms(ksg_ctx* c, double* out3) {
  if (!c || !out3) return KSG_ERR_ARG;
  KSG_LOCK(c);
  for (int i = 0; i < 3; ++i) out3[i] = c->last_kms[i];
  return KSG_OK;
}

int ksg_batch_totals(ksg_ctx* c, double* out24) {
  if (!c || !out24) return KSG_ERR_ARG;
  KSG_LOCK(c);
  for (int k = 0; k < 24; ++k) out24[k] = c->totals[k];
  return KSG_OK;
}

int ksg_last_batch_host_us(ksg_ctx* c, double* out8) {
  if (!c || !out8) return KSG_ERR_ARG;
  KSG_LOCK(c);
  for (int k = 0; k < 8; ++k) out8[k] = c->last_hus[k];
  return KSG_OK;
}

int ksg_last_batch_ms(ksg_ctx* c, double* ms) {
  if (!c || !ms) return KSG_ERR_ARG;
  KSG_LOCK(c);
  *ms = c->last_ms;
  return KSG_OK;
}

}  // extern "C"
