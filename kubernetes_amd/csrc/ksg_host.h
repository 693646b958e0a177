// ksg_host.h — what the host translation units share: the error macros, the environment
// switches' parsers, the owning types (device and pinned memory, stream, event, communicator;
// none can be copied), the context (struct ksg_ctx) and its named parts (struct Cluster and struct
// NodeMirror: what a node list determines; struct SrvClient: the resident server's host state;
// struct PendingBegin: the pod between begin and commit), and the functions one host file
// defines and another calls: ksg_runtime.cpp's helpers, the little ksg_dropin.cpp shows of the
// server's client, ksg_query.cpp's frame of the read-only batch queries (query_enter ...
// query_chunks) and ksg_without.cpp's table builder.
#ifndef KSG_HOST_H_
#define KSG_HOST_H_

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "ksg_internal.h"
#include "ksg_launch.h"

// The helpers below are shared between the host files only: they stay out of the library's
// dynamic symbol table (the C ABI of include/kschedgpu.h is all it exports).
#pragma GCC visibility push(hidden)

int fail(ksg_ctx* c, int code, const char* fmt, ...);

#define HIPCHK(c, x)                                                                 \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess)                                                            \
      return fail((c), KSG_ERR_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #x,          \
                  hipGetErrorString(e_));                                            \
  } while (0)

#define NCCLCHK(c, x)                                                                \
  do {                                                                               \
    ncclResult_t r_ = (x);                                                           \
    if (r_ != ncclSuccess)                                                           \
      return fail((c), KSG_ERR_RCCL, "%s:%d %s: %s", __FILE__, __LINE__, #x,         \
                  ncclGetErrorString(r_));                                           \
  } while (0)

// ---- environment switches ---------------------------------------------------
// KSG_X=0 turns a default-on switch off, KSG_X=<non-zero> a default-off switch on
inline bool env_flag(const char* name, bool dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) != 0 : dflt;
}
// the variable's integer value clamped to [lo, hi]; unset: dflt as it stands
inline int64_t env_int(const char* name, int64_t dflt, int64_t lo, int64_t hi) {
  const char* v = getenv(name);
  return v ? std::min<int64_t>(std::max<int64_t>(atoll(v), lo), hi) : dflt;
}

// ---- scratch memory -----------------------------------------------------------
// Device scratch of `cap` elements that frees itself with the context. grow() keeps the
// contents only while the buffer is large enough: max(need, 2 x cap, 64) elements, freed
// before the new allocation, so a warm context allocates nothing per batch.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  // (move-only: the moved-from buffer is left empty)
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      std::swap(p, o.p);
      std::swap(cap, o.cap);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  int grow(ksg_ctx* c, size_t need) {
    if (need <= cap && p) return KSG_OK;
    const size_t nc = std::max<size_t>(need, std::max<size_t>(cap * 2, 64));
    if (p) (void)hipFree(p);
    p = nullptr;
    HIPCHK(c, hipMalloc((void**)&p, nc * sizeof(T)));
    cap = nc;
    return KSG_OK;
  }
};

// Pinned host memory of `cap` elements, allocated with `flags`, that frees itself with the
// context; dp is its device address where the device writes it (any flags but the default:
// the coherent and the mapped allocations). alloc() replaces it with exactly `count` elements,
// contents dropped; grow() is the staging policy: max(need, 2 x cap, 4096) (geometric: a
// pinned (re)allocation costs ~0.2 ms, hipHostFree synchronises). Stays where it is declared.
template <typename T>
struct Pinned {
  T* p = nullptr;
  T* dp = nullptr;
  size_t cap = 0;
  const unsigned flags;
  explicit Pinned(unsigned flags_ = hipHostMallocDefault) : flags(flags_) {}
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  ~Pinned() {
    if (p) (void)hipHostFree(p);
  }
  operator T*() const { return p; }
  T* operator->() const { return p; }
  int alloc(ksg_ctx* c, size_t count) {
    if (p) (void)hipHostFree(p);
    p = dp = nullptr;
    cap = 0;
    HIPCHK(c, hipHostMalloc((void**)&p, count * sizeof(T), flags));
    cap = count;
    if (flags != hipHostMallocDefault && hipHostGetDevicePointer((void**)&dp, p, 0) != hipSuccess) {
      (void)hipHostFree(p);
      p = dp = nullptr;
      cap = 0;
      return fail(c, KSG_ERR_HIP, "hipHostGetDevicePointer failed");
    }
    return KSG_OK;
  }
  int grow(ksg_ctx* c, size_t need) {
    return cap >= need ? KSG_OK : alloc(c, std::max<size_t>(need, std::max<size_t>(cap * 2, 4096)));
  }
};
using HostBuf = Pinned<uint8_t>;  // the staging buffers, in bytes

// A HIP stream, a HIP event and the RCCL communicator, each destroyed with its owner while
// the owner's device is current. The stream and the communicator stay where they are
// declared; an event moves (the window path keeps a growing vector of them).
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  operator hipEvent_t() const { return e; }
};
struct Comm {
  ncclComm_t c = nullptr;
  Comm() = default;
  Comm(const Comm&) = delete;
  Comm& operator=(const Comm&) = delete;
  ~Comm() {
    if (c) (void)ncclCommDestroy(c);
  }
  operator ncclComm_t() const { return c; }
};
static_assert(!std::is_copy_constructible<HostBuf>::value && !std::is_copy_constructible<Stream>::value &&
                  !std::is_copy_constructible<Event>::value && !std::is_copy_constructible<Comm>::value,
              "the owners of pinned memory, streams, events and the communicator are not copied");

// The fixed-size device arrays of one node list (dalloc adds them), freed with their owner.
// Move-only; a moved-from owner holds none.
struct DevAllocs {
  std::vector<void*> v;
  DevAllocs() = default;
  DevAllocs(DevAllocs&& o) noexcept { v.swap(o.v); }
  DevAllocs& operator=(DevAllocs&& o) noexcept {
    if (this != &o) {
      release();
      v.swap(o.v);
    }
    return *this;
  }
  ~DevAllocs() { release(); }
  void release() {
    for (void* q : v) (void)hipFree(q);
    v.clear();
  }
};

struct PodRec {
  uint32_t host;
  int64_t cpu, mem;
  int64_t scalar[KSG_MAX_SCALAR];  // extension: extended resource requests
  std::vector<uint32_t> keys;  // ports + PDs
  std::vector<uint32_t> svcs;
  uint64_t seq;
};

// the fused window launch's control block: two KsgWinRun slots, then the pod groups'
// counters uint32[2][kFctlGroups][8] (a window of up to 4 x kFctlGroups pods)
constexpr uint32_t kFctlGroups = 1024;
constexpr size_t kFctlRuns = 2 * sizeof(KsgWinRun);
constexpr size_t kFctlBytes = kFctlRuns + (size_t)2 * kFctlGroups * 8 * sizeof(uint32_t);

// Timing-only events: no system-scope fence when they complete. A default
// hipEventRecord writes back and invalidates the caches, which costs the
// stream time between the window kernels and evicts the node state the next
// kernel reads from L2 (KSG_EVENT_FENCE=1 restores the default for A/B).
inline const unsigned kTimingEvent = env_flag("KSG_EVENT_FENCE", false) ? hipEventDefault : hipEventDisableSystemFence;

// Everything a node list determines: what build_cluster and node_ext_upload (ksg_cluster.cpp)
// write, and nothing else. The context holds one (c->cl): ksg_set_cluster starts from an empty
// one; ksg_update_cluster swaps the old one out, builds the new one beside it and swaps back on
// any failure. It owns its device memory (allocs and the DevBufs); the pointers in dev, d_zmap
// and d_lbl_* are views into allocs. Destroy one only while its device is current.
struct Cluster {
  uint32_t N = 0, nw = 0, n_pairs = 0, S = 0, D = 0;
  uint32_t lo = 0, hi = 0, wlo = 0, nwords = 0, nwords_max = 0;
  std::vector<uint32_t> shard_wlo_h;
  int R = 1;
  size_t lds = 0;
  KsgDev dev{};
  DevAllocs allocs;
  DevBuf<uint32_t> d_shard_wlo;
  DevBuf<int32_t> dbgbuf;  // dev.dbgbuf's owner (KSG_DEBUG & (8 | 32 | 64))
  // scratch sized for the shard
  DevBuf<uint8_t> d_fail;
  DevBuf<int64_t> d_score;
  DevBuf<uint8_t> d_rec_send, d_rec_recv;
  uint32_t rec_bytes = 0;
  DevBuf<int32_t> d_dpart, d_dglobal;
  uint32_t dbg_corrupt = 0;         // KSG_DEBUG bits 22 / 23: corrupt the next COMMIT / BEGIN request's layout
  bool win_d1 = true;               // phase A's single-commit drop bitmaps (KSG_WIN_D1=0: off; ksg_plain.hip)
  uint64_t* d_zmap = nullptr;       // [D+1][nw] re-rank: nodes of each domain row
  std::vector<int32_t> h_aff_pair;  // [affinity label][node] (ServiceAffinity, one rank)
  int64_t max_cap = 0, min_cap = 0;
  // calculateScore (priorities.go:27-37) stays in [0, 10] only while capacities lie in
  // [0, 2^63 / 10] and requested totals are non-negative; score_bound() assumes that range.
  // lr_wild: this node list, or a pod seen since ksg_set_cluster, can take a LeastRequested
  // term out of it (a negative capacity or one whose x10 wraps, a negative request, a total
  // that wraps): the int64 score kernels serve the context from then on (KsgDev.wide)
  bool lr_wild = false;
  unsigned __int128 static_mag = 0;  // max |score| of the terms ksg_set_static_terms added
  // the node labels on the device (ksg_add_static_config evaluates more static terms from them)
  const ksg_node* d_lbl_nodes = nullptr;
  const uint32_t* d_lbl_pairs = nullptr;
  const uint32_t* d_lbl_keys = nullptr;
};
static_assert(!std::is_copy_constructible<Cluster>::value && std::is_nothrow_move_constructible<Cluster>::value,
              "Cluster is move-only");

// The per-node half of the host mirror: what the committed pods add up to on each node and in
// each service. As constructed: no pods on N nodes and S services.
struct NodeMirror {
  std::vector<int64_t> used_c, used_m;
  std::vector<int64_t> sc_used;                    // [n_scalar][N] host mirror of scalar_used
  std::unordered_map<uint64_t, uint32_t> key_ref;  // (key << 32) | node
  std::vector<int32_t> svc_cnt;                    // S*N
  std::vector<std::unordered_map<uint32_t, int32_t>> svc_ext;
  std::vector<int32_t> svc_max, svc_total, svc_peer;
  std::vector<std::map<uint64_t, uint32_t>> svc_members;  // seq -> host
  NodeMirror() = default;
  NodeMirror(uint32_t N, uint32_t S, uint32_t n_scalar)
      : used_c(N, 0), used_m(N, 0), sc_used((size_t)n_scalar * N, 0), svc_cnt((size_t)S * N, 0), svc_ext(S),
        svc_max(S, 0), svc_total(S, 0), svc_peer(S, -1), svc_members(S) {}
};

// The host's side of the resident drop-in server (ksg_serve.hip; the client is ksg_dropin.cpp):
// begin / commit as requests in mapped host memory instead of launches, copies and stream
// syncs. The context holds one (c->srv), which owns the request block, the fail codes and the
// grid server's device state. As constructed: the KSG_SERVE* switches read, nothing allocated,
// no server running.
struct SrvClient {
  bool enabled = true;       // KSG_SERVE=0: the launch-per-call path
  bool running = false;      // a server kernel may be resident on the context's stream
  Pinned<KsgSrvBox> box{hipHostMallocCoherent | hipHostMallocMapped};  // the request / response block
  Pinned<uint8_t> fail{hipHostMallocCoherent | hipHostMallocMapped};   // fail codes of the shard's nodes
  DevBuf<KsgSrvGrid> grid;   // the grid server's device state
  uint32_t seq = 0;          // last request posted
  uint64_t idle_us = 20000;  // KSG_SERVE_IDLE_US: the server returns after this long without a request
  uint32_t unacked = 0;      // a COMMIT posted without waiting for its answer (0: none)
  uint32_t served = 0;       // every request up to this one was served
  uint32_t last_ctl = 0;     // the last control request posted
  uint64_t launches = 0;
  bool grid_on = true;       // KSG_SERVE_GRID=0: the one-workgroup server at every size
  uint32_t npt4_min = 16384;  // KSG_SERVE_GRID_NPT4_MIN: past this many nodes 4 nodes per thread
  // KSG_SERVE_GRID_MIN: shards above this many nodes take the grid server
  // (it beats the one-workgroup server at 500 nodes already: 7.2 vs 10.9 us)
  uint32_t grid_min = 0;
  bool grid_ext = true;      // KSG_SERVE_GRID_EXT=0: extension contexts on the one-workgroup server
  uint32_t epoch = 0;
  int64_t grid_opts = -1;    // KSG_SERVE_GRID_OPTS (KsgSrvArgs.grid_opts; -1: by size)
  bool stamps = false;       // KSG_SERVE_STAMPS=1: sum the server's per-stage cycles of each begin
  bool debug = false;        // KSG_SERVE_DEBUG=1: the grid server's stage markers, reported on a fault
  bool trace = false;        // KSG_SERVE_TRACE=1: every post, wait and relaunch to stderr
  double stage[6] = {};      // (printed by srv_print_stamps)
  uint64_t stamped = 0;
  SrvClient();
};

// The pod between ksg_schedule_begin and its commit (c->pb). clear() ends it: at the commit,
// when the next begin abandons it, and when ksg_set_cluster resets the mirror.
struct PendingBegin {
  bool on = false;
  uint64_t k = 0;  // its tie count
  ksg_pod pod{};
  std::vector<uint32_t> ids;
  bool served = false;       // by the resident server: the commit picks the node on the host, from
  std::vector<uint64_t> tw;  // ... the begin's tie words (node lo + 64 i + b)
  bool ext_on = false;       // ... and carries the begin's extension record
  ksg_pod_ext ext{};
  PendingBegin() = default;
  PendingBegin(const PendingBegin&) = delete;
  PendingBegin& operator=(const PendingBegin&) = delete;
  void clear() {
    on = served = ext_on = false;
    k = 0;
    pod.uid = ~0ULL;
    ids.clear();
    tw.clear();
  }
};
static_assert(!std::is_copy_constructible<SrvClient>::value && !std::is_copy_constructible<PendingBegin>::value,
              "the server's client and the pending begin stay in their context");

#pragma GCC visibility pop

struct ksg_ctx {
  ksg_config cfg{};
  int device = 0, rank = 0, world = 1;
  // Declared before everything that is freed, so destroyed after it: members go in reverse
  // order, and hipFree / hipHostFree of memory the stream's work used come before the stream's end.
  Stream st;
  Comm comm;
  bool xchg = false;  // exchange path: world > 1, or a 1-rank RCCL communicator
  double ppw_est = 0.0;  // pods resolved per window (window path round sizing)
  // windows per round = margin x (pods left) / ppw_est + 1 (KSG_ROUND_MARGIN): the
  // launches past the batch's end cost ~8 us each, a second round a host round trip
  double round_margin = 1.0;
  // pinned staging for the per-call uploads / small read-backs (a pageable
  // hipMemcpyAsync is a staged, effectively synchronous copy)
  HostBuf h_up, h_dn;
  // host-staged exchange (ksg_set_allgather) for sharded contexts without RCCL
  ksg_allgather_fn xfn = nullptr;
  void* xuser = nullptr;
  HostBuf h_xsend, h_xrecv;
  Event ev0, ev1;
  // the batch path's waits spin on this event (KSG_SPIN_WAIT=0: hipStreamSynchronize)
  Event ev_wait;
  bool spin_wait = true;
  double last_ms = 0.0;
  std::string err;

  // cluster
  bool have_cluster = false;
  // a batch failed after its device work was enqueued: the device may hold some
  // of its commits and the host mirror none, so every call fails until
  // ksg_set_cluster uploads the cluster again
  bool diverged = false;
  Cluster cl;  // the node list's parts

  // scratch
  DevBuf<ksg_pod> d_pods;
  DevBuf<uint32_t> d_ids;
  DevBuf<int32_t> d_out;
  DevBuf<uint64_t> d_rng;
  DevBuf<int64_t> d_summary;
  // the per-pod path (begin / commit / evaluate): the pod and its id list in
  // one device buffer (one copy in), and the decide kernel's summary and chosen
  // node written straight into pinned host memory (no copy out)
  DevBuf<uint8_t> d_one;
  const ksg_pod* one_pod = nullptr;
  const uint32_t* one_ids = nullptr;
  Pinned<uint8_t> h_map{hipHostMallocCoherent};  // [0, 32) summary int64[3], [32, 36) node (the device writes h_map.dp)
  DevBuf<KsgPatch> d_patch;
  DevBuf<uint64_t> d_draws;  // ksg_schedule_batch_draws: the caller's rand.Int() values
  uint64_t draw_tmp = 0;
  DevBuf<uint8_t> d_admit;  // kubelet admission: sets, pods, ids, pairs, codes (one buffer)
  // ksg_explain_batch: the per-node codes of one chunk of pods (bounded: kExplainStageBytes),
  // the histograms uint32[n][KSG_EXPLAIN_SLOTS] then the error flags uint8[n] of the whole call
  DevBuf<uint8_t> d_xcodes, d_xhist;
  Event ev_x0, ev_x1;  // around its kernel launches
  double last_explain_ms = 0.0;
  // ksg_prioritize_batch, per chunk of pods (each bounded by kExplainStageBytes): the per-node
  // scores; the normalised terms int32[per][D + 1], the tile partials and their candidates
  // (one buffer); and for the whole call the per-pod results (one buffer, one copy out)
  DevBuf<int64_t> d_pscores;
  DevBuf<uint8_t> d_ppart, d_pout;
  double last_prioritize_ms = 0.0;
  // ksg_headroom_batch: the per-node counts of one chunk of pods (bounded: headroom_stage
  // bytes, KSG_HEADROOM_STAGE_BYTES), and for the whole call uint64 total[n], uint32 max[n],
  // uint32 fit[n], uint32 hist[n][KSG_HEADROOM_SLOTS], uint8 err[n] (one buffer, one copy out)
  DevBuf<uint32_t> d_hcounts;
  DevBuf<uint8_t> d_hout;
  size_t headroom_stage = (size_t)64 << 20;
  int headroom_div = 1;  // udiv_capped's variant (KSG_HEADROOM_DIV)
  double last_headroom_ms = 0.0;
  // ksg_explain_without (ksg_without.cpp): the per-node codes of one chunk of pods (bounded:
  // without_stage bytes, KSG_EXPLAIN_WITHOUT_STAGE_BYTES), the histograms then the error flags of
  // the whole call, and the call's tables (KsgWithout's arrays, one buffer, one copy in)
  DevBuf<uint8_t> d_wcodes, d_whist, d_wtab;
  HostBuf h_wtab;
  size_t without_stage = (size_t)64 << 20;
  double last_without_ms = 0.0;
  // ksg_preempt_batch (ksg_preempt.cpp): per chunk of pods the tile partials (KsgPreemptPart) and,
  // where asked for, the per-node victim counts (together bounded: preempt_stage bytes,
  // KSG_PREEMPT_STAGE_BYTES), and for the whole call int32 best[n], uint32 victims[n], cand[n],
  // free[n], then the victim lists uint32[n][max_victims] (one buffer, one copy out). Its tables
  // share d_wtab / h_wtab with ksg_explain_without.
  DevBuf<uint8_t> d_vpart, d_vout;
  DevBuf<uint32_t> d_vnode;
  size_t preempt_stage = (size_t)64 << 20;
  double last_preempt_ms = 0.0;
  // ksg_pack_batch (ksg_pack.cpp): for the whole call int32 out_nodes[n], then uint32
  // placed[n_sets] (one buffer, one copy out). Its tables share d_wtab / h_wtab too.
  DevBuf<uint8_t> d_kout;
  double last_pack_ms = 0.0;
  std::vector<KsgPatch> patches;
  // ksg_update_cluster: its remap kernels' device ms (ev0 .. ev1), and the call's host us:
  // validation, device (build, gather, patches, the wait), host mirror
  double last_update_ms = 0.0;
  double last_update_us[3] = {0, 0, 0};

  // host mirror
  NodeMirror mir;
  // max over nodes of used_c / used_m for use_window: raised by each mirror add,
  // recomputed after anything else changes them (a removal, a negative total)
  int64_t mu_max = 0;
  bool mu_neg = false, mu_dirty = true;
  std::unordered_map<uint64_t, PodRec> pods;
  uint64_t seq = 0;

  // window (speculative) path
  uint32_t window = 128;        // 0 = exact one-pod-at-a-time kernel
  // HIP events around every ev_stride-th window launch (phase A and resolver;
  // KSG_KERNEL_EVENTS=N: every N-th, 0: none). An event between two dependent
  // launches lengthens the gap between them, so a sample of the windows is timed
  // and the per-launch mean scaled to all launches (ksg_last_batch_kernel_ms).
  uint32_t ev_stride = 4;
  uint32_t ev_phase = 0;  // which launches of a round are timed; advances every round
  DevBuf<KsgWinSum> d_winsum;
  DevBuf<uint8_t> d_xsend;   // phase A block of this shard (KsgWinXchg layout)
  DevBuf<uint8_t> d_xrecv;   // all-gathered blocks of every shard (world > 1)
  DevBuf<uint8_t> d_t0img;   // the plain resolver's T0 images, one per window pod
  DevBuf<int32_t> d_dcnt;    // [W][D] per-pod anti-affinity domain counts (phase A pre-pass)
  DevBuf<int32_t> d_dmb;     // [W][D+1] re-rank: best score without the anti term per domain row
  DevBuf<int32_t> d_etmax;    // [W] extension scores: TaintToleration max per window pod (count pass)
  DevBuf<int32_t> d_ethist;   // [W][KSG_TBINS] ... the histogram of its soft-taint counts
  DevBuf<uint64_t> d_epsoft;  // [W] ... the pods' untolerated soft taints as masks
  DevBuf<KsgWinRun> d_run;         // progress of the window chain (device)
  Pinned<KsgWinRun> h_run;         // pinned host copy
  uint32_t last_stats[4] = {0, 0, 0, 0};  // windows, stops (service scalar), stops (ties exhausted)
  std::vector<Event> wev;          // event pairs around the chained window kernels
  double last_kms[3] = {0, 0, 0};  // phase A ms, phase B ms, launches (window path)
  double last_t0ms = 0;            // ... and between them: the exchange (sharded) and the T0 images
  double last_wsum = 0;            // window capacity W summed over the launches
  bool dbg_fail_next = false;      // KSG_DEBUG & 16384: the next window batch fails after its device work
  // the fused window launch (KsgFused, ksg_plain.hip): one launch per window on one rank without
  // ServiceAntiAffinity or extensions (KSG_FUSED=0: phase A, T0 images and resolver apart)
  bool win_fused = true;
  uint32_t fused_grid = 0;          // its blocks: one per CU (KSG_FUSED_GRID overrides)
  // ... up to this many 64-node words per shard (KSG_FUSED_MAX_WORDS; 65,536 nodes): past them the
  // scoring blocks, one per CU under the resolver's LDS, are too few waves to hide phase A's load
  // latency (config 5, 100k nodes, same box: 255k fused against 385k apart; 45k nodes: 492k fused
  // against 465k, profiles/r6_fused_threshold.json)
  uint32_t fused_max_words = 1024;
  DevBuf<uint8_t> d_fctl;           // KsgWinRun[2], then the counters uint32[2][groups][8]
  HostBuf h_fctl;                   // pinned: the round's first slot and zeroed counters
  double last_hus[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // host us per phase of the last batch (ksg_last_batch_host_us)
  double totals[24] = {};  // ksg_batch_totals: the per-batch diagnostics summed over batches

  // Commits of the last ksg_schedule_batch not yet replayed into the host
  // mirror: replayed while the next batch runs on the device, or before any
  // call that reads the mirror (flush_deferred).
  std::vector<ksg_pod> dfr_pods;
  std::vector<uint32_t> dfr_ids;
  std::vector<int32_t> dfr_out;
  std::unordered_set<uint64_t> dfr_uids;
  int64_t dfr_sum = 0;   // sum of the deferred pods' requests (cpu + memory), capped
  bool dfr_neg = false;  // a deferred pod has a negative request
  int64_t used_hi = 0;                // the largest committed total the mirror has held
  unsigned __int128 dfr_req = 0;      // requests of batches whose commits are not in the mirror yet

  // extensions (ksg_set_extensions; exact kernels, one rank, parity unpinned)
  bool ext_on = false;
  ksg_ext_config ext{};
  std::unordered_map<uint64_t, std::array<int64_t, KSG_MAX_SCALAR>> ext_scalar;  // uid -> requests
  const ksg_pod_ext* cur_ext = nullptr;  // the _ext entry point's records for this call
  DevBuf<ksg_pod_ext> d_pext;            // device copy (batch / explain)
  ksg_pod_ext* d_one_ext = nullptr;      // the single pod's record (inside d_one)

  SrvClient srv;    // the resident drop-in server's client (ksg_dropin.cpp)
  PendingBegin pb;  // the begin that awaits its commit

  // Every entry point holds `mu`, so reflector threads may call ksg_add_pod /
  // ksg_remove_pod while the scheduling thread schedules. Updates that arrive
  // between ksg_schedule_begin and its commit are queued (validated first) and
  // applied, in arrival order, when the pending pod is committed or abandoned:
  // between pods, never inside one (SURVEY.md 8(b) "Threading").
  std::recursive_mutex mu;
  struct Queued {
    bool add;
    uint32_t host;
    ksg_pod pod;
    std::vector<uint32_t> ids;
    uint64_t uid;
  };
  std::vector<Queued> upd_q;
  std::unordered_set<uint64_t> q_added, q_removed;
};

#define KSG_LOCK(c) std::lock_guard<std::recursive_mutex> ksg_lock_((c)->mu)

// ---- ksg_runtime.cpp's helpers the other host files call --------------------------
#pragma GCC visibility push(hidden)

enum class Reduce { Sum, Max };

int check_pod(ksg_ctx* c, const ksg_pod* p, const uint32_t* ids, size_t n_ids);
int note_requests(ksg_ctx* c, const ksg_pod* pods, uint32_t n);
int flush_deferred(ksg_ctx* c);
void drop_deferred(ksg_ctx* c);
int flush_patches(ksg_ctx* c);
int upload_pods(ksg_ctx* c, const ksg_pod* pods, uint32_t n, const uint32_t* ids, size_t n_ids);
int wait_device(ksg_ctx* c);
int cluster_ok(ksg_ctx* c);
int mirror_add(ksg_ctx* c, uint32_t h, const ksg_pod* p, const uint32_t* ids, bool emit);
size_t pod_ids_extent(const ksg_pod* p);
int scan_exchange(ksg_ctx* c, const ksg_pod* dpod, const uint32_t* dids, int mode, uint8_t* fail_out,
                  int64_t* score_out, const ksg_pod_ext* dext);
int allgather(ksg_ctx* c, const void* dsend, void* drecv, size_t bytes);
int allreduce_i32(ksg_ctx* c, Reduce op, const int32_t* dsend, int32_t* drecv, uint32_t n);
bool anti_on(const ksg_ctx* c);
uint8_t* rec_buf(ksg_ctx* c);
// ... and the ones the node list (ksg_cluster.cpp) is built with
int pick_R(uint32_t shard_nodes);
void patch32(ksg_ctx* c, const void* addr, int32_t v);
void patch64(ksg_ctx* c, const void* addr, int64_t v);
void patch_or(ksg_ctx* c, const void* addr, uint64_t v);
void patch_andnot(ksg_ctx* c, const void* addr, uint64_t v);
void set_wide(ksg_ctx* c);
void reset_mirror(ksg_ctx* c);
// a zeroed device array of max(count, 1) elements, added to `owner` where one is given
template <typename T>
int dalloc(ksg_ctx* c, T** p, size_t count, std::vector<void*>* owner) {
  void* q = nullptr;
  HIPCHK(c, hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
  HIPCHK(c, hipMemsetAsync(q, 0, std::max<size_t>(count, 1) * sizeof(T), c->st));
  *p = static_cast<T*>(q);
  if (owner) owner->push_back(q);
  return KSG_OK;
}
// ... a fixed-size zeroed scratch buffer; the one it replaces is freed first
template <typename T>
int dalloc(ksg_ctx* c, DevBuf<T>& b, size_t count) {
  b.release();
  int rc = dalloc(c, &b.p, count, nullptr);
  if (rc == KSG_OK) b.cap = std::max<size_t>(count, 1);
  return rc;
}

// ---- the resident server's client (ksg_dropin.cpp), as far as the other files see it ------
// Ends the resident server so other work can use the context's stream (every entry point that
// enqueues on it calls this first); the next served begin launches it again.
int srv_stop(ksg_ctx* c);
int srv_flush_patches(ksg_ctx* c);  // flush_patches while a server is running: through its request block
void srv_print_stamps(ksg_ctx* c);  // ksg_destroy: what KSG_SERVE_STAMPS=1 gathered, to stderr

// ---- the read-only batch queries' frame (ksg_query.cpp) ---------------------------
// ksg_explain_batch, ksg_prioritize_batch, ksg_headroom_batch (ksg_query.cpp),
// ksg_explain_without (ksg_without.cpp), ksg_preempt_batch (ksg_preempt.cpp) and ksg_pack_batch
// (ksg_pack.cpp, whose unit is the pod set) answer for n pods against the device state as it
// stands, in one or more launches over chunks of pods. Each is: its null-pointer check, the
// lock, its own argument checks, then these steps in this order, with what only it does
// (buffers, zeroing, tables, where the results land) in between. Every step returns a KSG_*
// code the entry point passes on.
//
// enter: ksg_evaluate's protocol (no pending begin, no records while extensions are off, the
// server leaves the stream, the mirror and the cluster are current, the device is set), then
// *last_ms = 0, then n == 0 -> kQueryDone (nothing to do: the entry point returns KSG_OK),
// no nodes -> KSG_NONODES, ids missing. Any other non-zero code the entry point returns as it is.
constexpr int kQueryDone = 1 << 20;  // (no KSG_* code)
int query_enter(ksg_ctx* c, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids, uint32_t n_ids, double* last_ms);
// validate: ksg_schedule_batch's checks pod by pod; also(i), where given, after pod i's own
// checks and before pod i + 1's. No uid is looked at and note_requests is NOT called.
int query_validate(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                   uint32_t n_ids, const std::function<int(uint32_t)>& also = {});
// upload: the patches, the pods and their ids, and the extension records into d_pext. *dext is
// nullptr without records (the kernels then skip the extension filters, as an all-zero record
// passes them), unless zero_records asks for all-zero ones whenever the extensions are on.
int query_upload(ksg_ctx* c, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n, const uint32_t* ids,
                 uint32_t n_ids, bool zero_records, const ksg_pod_ext** dext);
// pods per launch: as many as `budget` bytes of staging hold at bytes_per_pod each (0: no
// staging, no bound), at most 2^20, whole pod chunks of the kernel past one chunk, at least 1
// and at most n.
uint32_t query_per(size_t budget, size_t bytes_per_pod, uint32_t chunk, uint32_t n);
// the chunk loop: for each chunk [a, a + m) of `per` pods launch(a, m) between the events
// ev_x0 / ev_x1 (created here on first use), then copies(a, m, last) outside them, which
// enqueues the chunk's per-node rows and with the last chunk the per-pod results, then one
// stream synchronise; the elapsed times add up in *last_ms. (Callers pass their lambdas as
// std::cref: a std::function holding a reference allocates nothing.)
int query_chunks(ksg_ctx* c, uint32_t n, uint32_t per, double* last_ms, const std::function<int(uint32_t, uint32_t)>& launch,
                 const std::function<int(uint32_t, uint32_t, bool)>& copies);
// ---- ksg_without.cpp's table builder, shared with ksg_preempt.cpp -------------------------
// The tables of an ordered list of committed pods (KsgWithout, ksg_internal.h), built in
// c->h_wtab with their device addresses in c->d_wtab (both grown here): the caller copies
// `bytes` across on the stream after its uploads. w.first_absent and w.peer point at pod 0's
// entries (a chunk offsets them). peers: look up each pod's ServiceAffinity peer as of its
// position (w.peer stays nullptr without the predicate); entry_keys: also the conflict keys of
// every row entry (ek). KSG_ERR_ARG, nothing built, for an unknown uid or a uid listed twice.
struct WithoutTables {
  KsgWithout w{};
  KsgPreemptKeys ek{};
  size_t bytes = 0;
};
int without_tables(ksg_ctx* c, const ksg_pod* pods, uint32_t n, const uint64_t* absent_uids, uint32_t n_absent,
                   const uint32_t* first_absent, bool peers, bool entry_keys, WithoutTables* tabs);
// query_validate's per-pod extra of both callers: first_absent[i] <= n_absent
int without_position(ksg_ctx* c, const uint32_t* first_absent, uint32_t i, uint32_t n_absent);
extern "C" {  // (defined among the entry points, inside ksg_runtime.cpp's extern "C" block)
int remove_pod_impl(ksg_ctx* c, uint64_t uid);
int apply_queued(ksg_ctx* c);
int note_ext(ksg_ctx* c, const ksg_pod* p, const ksg_pod_ext* e, size_t n_ids);
int check_ext_range(ksg_ctx* c, const ksg_pod_ext* e, size_t n_ids);
int check_taint_ids(ksg_ctx* c, const ksg_pod_ext* e, const uint32_t* ids);
}

#pragma GCC visibility pop

#endif  // KSG_HOST_H_
