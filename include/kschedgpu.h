/*
 * kschedgpu.h — C ABI of libkschedgpu.so, the MI355X-native Filter/Score pass of
 * the kube-scheduler generic scheduler (smarterclayton/kubernetes v0.13.0-dev).
 *
 * What this ABI replaces (reference file:line, all under /root/reference):
 *   algorithm.Scheduler.Schedule(pod, minionLister)      pkg/scheduler/scheduler.go:25-27
 *     implemented by genericScheduler.Schedule           pkg/scheduler/generic_scheduler.go:54-80
 *       findNodesThatFit                                 pkg/scheduler/generic_scheduler.go:100-128
 *       prioritizeNodes                                  pkg/scheduler/generic_scheduler.go:136-165
 *       selectHost / getBestHosts                        pkg/scheduler/generic_scheduler.go:84-96,167-177
 *   SystemModeler.AssumePod (the commit)                 plugin/pkg/scheduler/scheduler.go:42-47,115-118
 *   NewGenericScheduler(predicates, prioritizers, ...)   pkg/scheduler/generic_scheduler.go:197-204
 *     built by ConfigFactory.CreateFromKeys              plugin/pkg/scheduler/factory/factory.go:107-172
 *
 * Conventions
 *   - Strings never cross this ABI. The caller (the Go cgo shim, or the Python
 *     mirror in kubernetes_amd/) interns node names, label (key,value) pairs,
 *     label keys, host ports, GCE PD names and services to dense ids.
 *   - Node "rank" = index of the node in byte-wise ascending name order. The
 *     reference's tie order (score desc, host name desc; types.go:42-47) is
 *     therefore "rank desc".
 *   - All input arrays are caller-owned and copied before return. Output
 *     buffers are caller-allocated.
 *   - Return codes: KSG_OK (0); KSG_NOFIT (1) = *FitError; KSG_NONODES (2) =
 *     "no minions available to schedule pods"; negative = internal error, see
 *     ksg_last_error(). There is NO CPU fallback inside this library: every
 *     predicate/priority evaluation runs in HIP kernels on the GPU.
 *   - One scheduling thread per context (the reference calls Schedule from one
 *     goroutine, plugin/pkg/scheduler/scheduler.go:86-88). Every entry point
 *     holds the context's mutex, so other threads (the reflectors feeding the
 *     scheduled-pod store, factory.go:126-145) may call ksg_add_pod /
 *     ksg_remove_pod at any time: between pods they apply at once (a batch in
 *     flight finishes first); between ksg_schedule_begin and its commit they
 *     are validated, queued and applied in arrival order right after the
 *     commit (or when the begin is abandoned by the next begin).
 */
#ifndef KSCHEDGPU_H_
#define KSCHEDGPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSG_ABI_VERSION 3

/* ---- return codes ---------------------------------------------------- */
#define KSG_OK 0
#define KSG_NOFIT 1          /* generic_scheduler.go:72-77  *FitError              */
#define KSG_NONODES 2        /* generic_scheduler.go:59-61  no minions available   */
#define KSG_ERR_ARG (-1)
#define KSG_ERR_HIP (-2)
#define KSG_ERR_CAPACITY (-3)
#define KSG_ERR_STATE (-4)
#define KSG_ERR_NOPEER (-5)  /* predicates.go:293-296: service peer's host is not a known node */
#define KSG_ERR_RCCL (-6)

/* out_nodes[] codes of ksg_schedule_batch (>= 0 is a node rank) */
#define KSG_OUT_NOFIT (-1)
#define KSG_OUT_ERROR (-2)
#define KSG_OUT_NONODES (-3)

/* ---- predicates (FitPredicate registry names, factory/plugins.go:63-117) */
#define KSG_PRED_PODFITSPORTS      (1u << 0) /* predicates.go:326-350 */
#define KSG_PRED_PODFITSRESOURCES  (1u << 1) /* predicates.go:94-145  */
#define KSG_PRED_NODISKCONFLICT    (1u << 2) /* predicates.go:52-83   */
#define KSG_PRED_MATCHNODESELECTOR (1u << 3) /* predicates.go:161-179 */
#define KSG_PRED_HOSTNAME          (1u << 4) /* predicates.go:181-186 */
#define KSG_PRED_SERVICEAFFINITY   (1u << 5) /* predicates.go:231-324 (policy) */
#define KSG_PRED_LABELSPRESENCE    (1u << 6) /* predicates.go:188-229 (policy) */

/* fail codes written per node by ksg_schedule_begin/ksg_evaluate:
 * 0 = fits, otherwise the first failing predicate in this fixed order. */
#define KSG_FAIL_NONE 0
#define KSG_FAIL_HOSTNAME 1
#define KSG_FAIL_LABELSPRESENCE 2
#define KSG_FAIL_MATCHNODESELECTOR 3
#define KSG_FAIL_NODISKCONFLICT 4
#define KSG_FAIL_PODFITSPORTS 5
#define KSG_FAIL_PODFITSRESOURCES 6
#define KSG_FAIL_SERVICEAFFINITY 7

#define KSG_MAX_ANTI 64          /* ServiceAntiAffinity priorities (policy)      */
#define KSG_MAX_LABEL_PREF 32    /* LabelPreference priorities (policy)          */
#define KSG_MAX_PRESENCE 16      /* LabelsPresence predicates (policy)           */
#define KSG_MAX_PRESENCE_KEYS 16 /* labels per LabelsPresence predicate          */
#define KSG_MAX_AFF 16          /* ServiceAffinity labels (union of predicates) */
#define KSG_MAX_AFF_GROUPS 32   /* ServiceAffinity predicates (label groups)    */

/* Label pair flag in ksg_set_cluster's pair_keys[p]: the pair's key fails
 * IsQualifiedName or its value fails IsValidLabelValue (pkg/util/validation.go),
 * so a selector built from it by SelectorFromSet is the empty selector that
 * matches every node (pkg/labels/selector.go:654-668). The key id is
 * pair_keys[p] & ~KSG_PAIR_INVALID. */
#define KSG_PAIR_INVALID 0x80000000u
/* ksg_pod.aff_pair[j]: the pod's nodeSelector gives ServiceAffinity label j
 * an invalid value (or label j's key is invalid). */
#define KSG_AFF_INVALID (-2)

/* Scheduler configuration: the compiled form of map[string]FitPredicate +
 * []PriorityConfig that NewGenericScheduler receives (factory.go:149).
 * Any Policy the reference accepts fits: weights are int64 and the list caps
 * above are well past what a Policy names in practice (the reference registers
 * any number, plugins.go:81-183); factory.compile reports a Policy beyond them. */
typedef struct ksg_config {
  uint32_t predicates;          /* KSG_PRED_* bitmask                                   */
  uint32_t n_priority_configs;  /* len(priorityConfigs); 0 => EqualPriority fallback
                                   (generic_scheduler.go:141-143)                       */
  /* Priority weights are Go ints (plugin/pkg/scheduler/api/types.go:46: int64 on
   * the reference's platform) and combined scores wrap like Go's int
   * (generic_scheduler.go:145-159). While 10 * sum|w| + |w_equal| < 2^30 the
   * window path runs with int32 scores (any number of ServiceAntiAffinity
   * priorities, any shard size up to 131,072 nodes); otherwise every batch takes
   * the exact kernels with int64 (wrapping) combined scores. That bound takes
   * every priority's score to lie in [0, 10]; calculateScore (priorities.go:27-37)
   * leaves the range with a negative capacity, a capacity past 2^63 / 10 (its x10
   * wraps) or a negative requested total, so a node list or a pod that can produce
   * one of these also puts the context on the int64 kernels, until the next
   * ksg_set_cluster. */
  int64_t w_least_requested;    /* LeastRequestedPriority weight, 0 = absent/skipped    */
  int64_t w_service_spreading;  /* ServiceSpreadingPriority weight                       */
  int64_t w_equal;              /* EqualPriority weight (DefaultProvider: 0, skipped)    */
  uint32_t n_anti;              /* ServiceAntiAffinity priorities                        */
  uint32_t anti_key[KSG_MAX_ANTI];   /* label-key id of each                           */
  int64_t w_anti[KSG_MAX_ANTI];
  uint32_t n_label_pref;        /* LabelPreference priorities                            */
  uint32_t pref_key[KSG_MAX_LABEL_PREF];
  uint32_t pref_presence[KSG_MAX_LABEL_PREF];
  int64_t w_pref[KSG_MAX_LABEL_PREF];
  uint32_t n_presence;          /* LabelsPresence predicates                             */
  uint32_t presence_n_keys[KSG_MAX_PRESENCE];
  uint32_t presence_keys[KSG_MAX_PRESENCE][KSG_MAX_PRESENCE_KEYS];
  uint32_t presence_flag[KSG_MAX_PRESENCE];
  uint32_t n_aff_labels;        /* ServiceAffinity: label-key ids (union over predicates) */
  uint32_t aff_key[KSG_MAX_AFF];
  uint32_t max_conflict_keys;   /* capacity for interned host-port + GCE-PD ids          */
  uint32_t max_domains;         /* capacity for anti-affinity label values (pair ids)    */
  /* ServiceAffinity predicates: bit j of aff_group_mask[g] = aff label j belongs
   * to predicate g. Each predicate builds its own selector, so SelectorFromSet's
   * invalid-value trap empties one predicate's selector, not the others'
   * (predicates.go:311-315). n_aff_groups == 0: one predicate over every label. */
  uint32_t n_aff_groups;
  uint32_t aff_group_mask[KSG_MAX_AFF_GROUPS];
} ksg_config;

/* One node, rank-ordered. Capacity is node.Spec.Capacity converted with
 * Quantity.MilliValue (cpu) / Value (memory) (resource_helpers.go:29-42). */
typedef struct ksg_node {
  int64_t cap_milli_cpu;
  int64_t cap_memory;
  uint32_t label_off;   /* offset into node_pairs[] of this node's label pair ids */
  uint32_t n_labels;
} ksg_node;

/* One pod (pending or existing). Variable-length lists are (offset, count)
 * into a caller-supplied uint32 id array passed alongside. */
typedef struct ksg_pod {
  uint64_t uid;         /* caller-unique id (namespace/name) for ksg_remove_pod     */
  int64_t milli_cpu;    /* getResourceRequest: sum of container Limits cpu (milli)  */
  int64_t memory;       /* ... and memory (bytes) (predicates.go:94-102)            */
  int32_t host;         /* Spec.Host: -1 empty, -2 names no node, else node rank    */
  int32_t service;      /* services[0] of GetPodServices, -1 none                   */
  uint32_t ports_off, n_ports;  /* conflict-key ids of HostPorts != 0               */
  uint32_t pds_off, n_pds;      /* conflict-key ids of GCE PD names                 */
  uint32_t sel_off, n_sel;      /* nodeSelector pair ids; 0 = pair no node has;
                                   n_sel == 0 => selector matches everything        */
  uint32_t svcs_off, n_svcs;    /* every service whose selector matches the pod     */
  int32_t aff_pair[KSG_MAX_AFF];/* ServiceAffinity: pair id of the pod's own
                                   nodeSelector value for aff label j; -1 = the pod
                                   does not specify it; 0 = value no node has;
                                   KSG_AFF_INVALID = an invalid value            */
} ksg_pod;

typedef struct ksg_ctx ksg_ctx;

/* Create a context on HIP device `device`. Single-GPU form. */
int ksg_create(const ksg_config* cfg, int device, ksg_ctx** out);

/* Node-sharded form: `world` (<= 16) processes, one per GPU, each owning the
 * node ranks of its run of 64-node words (ksg_shard_range). Node state is
 * replicated; filter/score evaluation is sharded. Window path: the shards'
 * per-word results for a window of pods are all-gathered once per window and
 * every rank resolves the window identically. Per-pod path (begin/commit,
 * ServiceAntiAffinity): the shard records are all-gathered per pod. `nccl_id`
 * is the 128-byte ncclUniqueId from rank 0 (RCCL over xGMI), or NULL to use a
 * host transport installed with ksg_set_allgather. world == 1 with an nccl_id
 * runs the same exchange path over a 1-rank RCCL communicator. */
int ksg_create_sharded(const ksg_config* cfg, int device, int rank, int world,
                       const void* nccl_id, ksg_ctx** out);
/* Host transport for a sharded context created with nccl_id == NULL: the
 * library calls fn(user, send, recv, bytes) with host buffers and fn must
 * all-gather `bytes` from every rank into recv, rank-major (world * bytes),
 * returning 0 on success. Every rank must make the same sequence of calls.
 * This is how a caller that owns its own transport (or a test that runs
 * several ranks on one GPU, where RCCL refuses duplicate devices) drives the
 * same sharded kernels; with an RCCL communicator the exchange stays on the
 * device stream. */
typedef int (*ksg_allgather_fn)(void* user, const void* send, void* recv, uint64_t bytes);
int ksg_set_allgather(ksg_ctx* ctx, ksg_allgather_fn fn, void* user);
/* Fill a fresh ncclUniqueId (128 bytes) for ksg_create_sharded on rank 0. */
int ksg_nccl_unique_id(void* out128);

int ksg_destroy(ksg_ctx* ctx);
const char* ksg_last_error(ksg_ctx* ctx);

/* Replace the node set (MinionLister.List()). Resets all pod state
 * (ksg_update_cluster, below, replaces it and keeps the pods).
 * pair_keys[p] = label-key id of label pair p, | KSG_PAIR_INVALID for a pair
 * SelectorFromSet would reject (pair 0 is reserved: "no node has it").
 * node_pairs holds each node's label pair ids. */
int ksg_set_cluster(ksg_ctx* ctx, const ksg_node* nodes, uint32_t n_nodes,
                    const uint32_t* node_pairs, uint32_t n_node_pairs,
                    const uint32_t* pair_keys, uint32_t n_pairs,
                    uint32_t n_services);

/* Existing / assumed pods (SimpleModeler.AssumePod + scheduled-pod store).
 * host_id < n_nodes is a node rank (Status.Host); host_id >= n_nodes is a host
 * that is not in the node list (still counted by ServiceSpreading's maxCount,
 * spreading.go:73-80). */
int ksg_add_pod(ksg_ctx* ctx, uint32_t host_id, const ksg_pod* pod, const uint32_t* ids);
int ksg_remove_pod(ksg_ctx* ctx, uint64_t uid);

/* Static node terms beyond the config's fixed slots (more LabelsPresence
 * predicates or keys than KSG_MAX_PRESENCE x KSG_MAX_PRESENCE_KEYS, more
 * LabelPreference priorities than KSG_MAX_LABEL_PREF): the caller evaluates
 * them per node from the node labels and folds them in after ksg_set_cluster
 * (they end with that node list: call again after the next one).
 * fit_words (optional): ceil(n_nodes / 64) words in node-rank order, bit n%64
 * of word n/64 set iff node n passes every extra LabelsPresence predicate
 * (CheckNodeLabelPresence, predicates.go:194-229); a node that fails gets
 * KSG_FAIL_LABELSPRESENCE. score (optional): n_nodes Go-int sums of weight x
 * CalculateNodeLabelPriority (priorities.go:98-134) over the extra priorities,
 * added to every node's combined score with Go's wrap; score_weighted != 0
 * when any of them has a nonzero weight (the HostPriorityList is then not
 * empty). The config's predicates must include KSG_PRED_LABELSPRESENCE and its
 * n_priority_configs count the extra priorities. No reference counterpart (the
 * reference's registry takes any number of them: plugins.go:81-117, 145-183). */
int ksg_set_static_terms(ksg_ctx* ctx, const uint64_t* fit_words, const int64_t* score, int score_weighted);
/* The same static terms evaluated on the device from the node labels of the last
 * ksg_set_cluster, one slot pass per call: `extra`'s LabelsPresence slots
 * (n_presence, presence_n_keys, presence_keys, presence_flag) and LabelPreference
 * slots (n_label_pref, pref_key, pref_presence, w_pref) are evaluated per node
 * (ksg_static_kernel) and folded in like ksg_set_static_terms' arrays; every other
 * field of `extra` is ignored. Call it as often as the policy needs (each pass
 * holds up to KSG_MAX_PRESENCE predicates of KSG_MAX_PRESENCE_KEYS keys and
 * KSG_MAX_LABEL_PREF priorities); the terms end with the node list. */
int ksg_add_static_config(ksg_ctx* ctx, const ksg_config* extra);

/* Split Schedule: begin evaluates every node and reports the best combined
 * score and the number of nodes tied at it (0 => KSG_NOFIT). The caller draws
 * r = rand.Int() iff tie_count > 0 and calls commit(r % tie_count), which picks
 * the tie_index-th tie in descending name order (generic_scheduler.go:88-95)
 * and applies AssumePod's delta. fail_codes (optional, n_nodes bytes) gets the
 * per-node KSG_FAIL_* code to rebuild FailedPredicateMap.
 * On one rank (int32 scores; plain shards up to 261,120 nodes, others up to
 * 16,384) both calls are served by a resident kernel polling mapped host memory
 * (ksg_serve.hip): no kernel launch, copy or stream synchronisation per call.
 * begin returns the pod's tie words with its answer, and commit picks the node
 * from them on the host and returns at once: AssumePod's delta is applied on
 * the device before any later call reads device state (a rejected commit is
 * reported by the next call). The server returns after KSG_SERVE_IDLE_US
 * (default 20,000) without a request and is relaunched by the next one; any
 * other entry point that needs the device stops it first. KSG_SERVE=0 in the
 * environment at ksg_create: kernels launched per call. */
int ksg_schedule_begin(ksg_ctx* ctx, const ksg_pod* pod, const uint32_t* ids,
                       int64_t* max_score, uint32_t* tie_count, uint8_t* fail_codes);
int ksg_schedule_commit(ksg_ctx* ctx, uint32_t tie_index, int32_t* out_node);

/* Schedule n pods in order, committing each before the next, entirely on the
 * device. Tie-break source: splitmix64 with state *rng_state; one Int63 draw
 * (next() >> 1) per successful schedule only (generic_scheduler.go:94).
 * out_nodes[i] = node rank or KSG_OUT_*. *rng_state is advanced. */
int ksg_schedule_batch(ksg_ctx* ctx, const ksg_pod* pods, uint32_t n,
                       const uint32_t* ids, uint32_t n_ids,
                       uint64_t* rng_state, int32_t* out_nodes);

/* ksg_schedule_batch with the caller's own random source: draws[k] is the
 * k-th rand.Int() value the caller's generator would return (e.g. a Go
 * *rand.Rand's next n Int()s, n_draws >= n). Pod i that finds a node uses the
 * next unused value, exactly as n sequential Schedule calls would
 * (generic_scheduler.go:94); *draws_used = how many were used (the caller keeps
 * the rest for its next call). The sequential path's stream is reproduced:
 * no splitmix64. Every rank of a sharded context passes the same values. */
int ksg_schedule_batch_draws(ksg_ctx* ctx, const ksg_pod* pods, uint32_t n, const uint32_t* ids,
                             uint32_t n_ids, const uint64_t* draws, uint32_t n_draws, uint32_t* draws_used,
                             int32_t* out_nodes);

/* Bind rejected in batch mode. The reference binds each pod before it schedules
 * the next: a rejected Bind means no AssumePod for that pod, but its rand.Int()
 * was already drawn (plugin/pkg/scheduler/scheduler.go:93-118,
 * pkg/scheduler/generic_scheduler.go:94). A batch committed every placement on
 * the device, so when the caller binds pods[0..n) of the last batch in order and
 * pod k's Bind (out_nodes[k] >= 0) is rejected, this call undoes the commits of
 * pods k..n-1 (newest first), leaving the state of pods 0..k-1 committed.
 * *draws_kept = the draws pods 0..k consumed (pod k's stays consumed): with
 * ksg_schedule_batch_draws the caller puts draws[*draws_kept .. draws_used) back
 * at the front of its FIFO; rng_state (optional, ksg_schedule_batch's splitmix64
 * state) is stepped back over the draws of pods k+1..n-1. The caller then
 * re-batches pods k+1..n-1. pods / out_nodes are the last batch's arrays; every
 * rank of a sharded context makes the same call. KSG_ERR_ARG (nothing changed)
 * when k >= n, pod k found no node, or a placed pod's uid is not committed.
 * The pods are removed by uid and out_nodes is read only for its sign, so the call
 * also works after a ksg_update_cluster has renumbered the nodes. */
int ksg_batch_unwind(ksg_ctx* ctx, const ksg_pod* pods, const int32_t* out_nodes, uint32_t n, uint32_t k,
                     uint64_t* rng_state, uint32_t* draws_kept);

/* Introspection (HostPriorityList): per-node fail code and combined score for
 * a pod, without committing. score_out[i] is meaningful where fail_out[i]==0. */
int ksg_evaluate(ksg_ctx* ctx, const ksg_pod* pod, const uint32_t* ids,
                 uint8_t* fail_out, int64_t* score_out);

/* Batch execution strategy. window > 0 (default 128, env KSG_WINDOW): pods
 * are filtered/scored a window at a time against one snapshot on all CUs and
 * then resolved in order by one workgroup (exact; see ksg_window.hip);
 * ServiceAntiAffinity adds a per-window domain-count pass. window = 0: the
 * persistent one-pod-at-a-time kernel. Both give identical results; a batch
 * takes the window path only where it is exact (non-negative LeastRequested /
 * ServiceSpreading weights, capacities and requested totals within 2^49, at
 * most 2048 node words). */
int ksg_set_window(ksg_ctx* ctx, uint32_t window);
/* Window statistics of the last ksg_schedule_batch: stats4[0] = windows
 * (snapshots), [1] = windows ended because a service scalar changed, [2] =
 * windows ended because every snapshot tie of a pod got worse, [3] = windows
 * ended by the per-node window cache filling up or an oversized pod. */
int ksg_last_batch_stats(ksg_ctx* ctx, uint32_t* stats4);

/* Device time (ms) of the last ksg_schedule_batch's kernels, from HIP events
 * recorded on the stream the kernels ran on. */
int ksg_last_batch_ms(ksg_ctx* ctx, double* ms);

/* Window path of the last ksg_schedule_batch: out3[0] = device ms in the
 * snapshot-scoring kernel(s) (ksg_win_score_kernel, its count passes and, on a
 * sharded context, the count passes' all-reduces; not the all-gather or the
 * T0-image kernel: ksg_batch_totals [18]), out3[1] = device ms in the
 * resolver (ksg_win_plain_kernel, or with ServiceAntiAffinity
 * ksg_win_resolve2_kernel / ksg_win_resolve_kernel; the fused window launch of
 * one plain rank scores the window inside the resolver's launch, so its whole
 * time is here and out3[0] is 0), out3[2] = resolver launches (windows are
 * chained on the device, so a round may end with launches that find the batch
 * done and return at once); from HIP events recorded on the context's stream
 * around every 4th launch of a round, the sampled positions rotating from round
 * to round (KSG_KERNEL_EVENTS=N in the environment at context creation: every
 * N-th, 0: none), the sampled launches' mean scaled to all launches: an event
 * between two dependent launches lengthens the gap between them. */
int ksg_last_batch_kernel_ms(ksg_ctx* ctx, double* out3);

/* Host time (microseconds, steady clock) of the last ksg_schedule_batch by
 * phase: out8[0] validation (pod checks, duplicate uids), [1] upload (pending
 * patches, pod copy-in), [2] window setup and round sizing, [3] enqueueing the
 * launches and copies, [4] the host-mirror replay of the previous batch
 * (overlapped with the device), [5] waiting for the device at the end of each
 * window round (the placements' copy-out rides with it), [6] waiting for a
 * separate copy-out (exact path, or a round that did not finish the batch),
 * [7] the deferred-replay bookkeeping. No reference counterpart (diagnostics). */
int ksg_last_batch_host_us(ksg_ctx* ctx, double* out8);

/* The per-batch diagnostics above summed over every successful
 * ksg_schedule_batch since the context was created, so a caller can read them
 * once around a run instead of after each batch: out24[0] batches, [1] device
 * ms (ksg_last_batch_ms), [2..4] ksg_last_batch_kernel_ms, [5..8]
 * ksg_last_batch_stats, [9..16] ksg_last_batch_host_us, [17] the window
 * capacity (pods phase A scores per launch) summed over the window-path
 * launches, [18] device ms between phase A and the resolver (the sharded
 * all-gather and the T0-image kernel, ksg_win_t0_kernel; the count passes'
 * all-reduces are in [2]; sampled like ksg_last_batch_kernel_ms), [19..23] zero. */
int ksg_batch_totals(ksg_ctx* ctx, double* out24);

/* Diagnostics: the window resolver's per-stage clock counters (s_memtime
 * cycles / 64, summed over every window since the context was created) for a
 * context created with KSG_DEBUG=8 in the environment (layout: DESIGN.md
 * section 4, "resolver stages"). The library holds KSG_DEBUG_COUNTER_WORDS
 * words; it copies min(n_words, KSG_DEBUG_COUNTER_WORDS) of them into out and
 * zero-fills the rest of out (ABI version 3: version 2's form took no length
 * and wrote 64 words into a buffer its parameter name said held 32).
 * KSG_ERR_STATE when not enabled. */
#define KSG_DEBUG_COUNTER_WORDS 64
int ksg_debug_counters(ksg_ctx* ctx, int32_t* out, uint32_t n_words);

/* Diagnostics of the resident begin/commit server: out4[0] kernel launches,
 * [1] requests served (begin, commit, patch, exit), [2] 1 while resident,
 * [3] 1 when this context uses the one-workgroup server, 2 the grid server
 * (one scan workgroup per 256 nodes; every plain shard by default,
 * KSG_SERVE_GRID=0 / KSG_SERVE_GRID_MIN), 0 none. No reference counterpart. */
int ksg_serve_stats(ksg_ctx* ctx, uint64_t* out4);

/* ---- node sharding (multi-GPU) ------------------------------
 * Nodes are split into contiguous runs of 64-node words in name-rank order.
 * Per pod every shard produces one record: this header followed by the shard's
 * tie bitmap (uint64 words, bit j of word w = node 64*(shard_first_word+w)+j
 * scores max_score). The winner rule over all records is the reference's
 * selectHost (generic_scheduler.go:84-96): global max, k = sum of the shards'
 * counts at the max, ix = Int63() % k, ix-th tie counted from the highest name
 * rank. ksg_schedule_batch/begin/commit apply it on the device after an RCCL
 * all-gather; these two host functions expose the same rule (same code) for a
 * caller that exchanges records over its own transport. */
typedef struct ksg_shard_record {
  int64_t max_score;  /* INT64_MIN if nothing fits in the shard */
  uint64_t tie_count; /* nodes of the shard at max_score */
  int32_t error;      /* nonzero: the pod errors (ServiceAffinity peer not a node) */
  int32_t pad;
  uint64_t pad2;
} ksg_shard_record;

/* Node range [lo, hi) of shard `rank` of `world` over n_nodes rank-ordered nodes. */
int ksg_shard_range(uint32_t n_nodes, int rank, int world, uint32_t* lo, uint32_t* hi);

/* Merge `world` records of rec_bytes each (header + ceil-words tie bitmap).
 * rng_state != NULL: draw Int63 from the splitmix64 stream only if k > 0 (as the
 * batch path); else use tie_index % k (as ksg_schedule_commit). Returns KSG_OK
 * with *out_node = global node rank, KSG_NOFIT (no draw), or KSG_ERR_NOPEER.
 * empty_priorities: the config has priority configs but all weights are 0. */
int ksg_merge_records(const void* records, uint32_t rec_bytes, uint32_t world, uint32_t n_nodes,
                      int empty_priorities, uint64_t* rng_state, uint64_t tie_index, int32_t* out_node,
                      int64_t* max_score, uint64_t* tie_count);

/* Node shard owned by this context: [lo, hi). */
int ksg_shard(ksg_ctx* ctx, uint32_t* lo, uint32_t* hi);

/* Copy the committed per-node requested totals (sum of limits of all pods on
 * the node) back to the host, for state checks. */
int ksg_read_requested(ksg_ctx* ctx, int64_t* milli_cpu, int64_t* memory);

/* Copy the rest of the committed per-node pod state back to the host, for state
 * checks (diagnostics, like ksg_read_requested; with it and ksg_read_ext_used this
 * is every word a commit, ksg_add_pod, ksg_remove_pod or ksg_batch_unwind changes).
 * The state is a function of the ordered list of live pods and their hosts:
 *   keymap[k * nw + n / 64] bit n % 64   some live pod on node n lists conflict key k
 *                                        among its host ports or GCE PDs
 *   svc_cnt[s * n_nodes + n]             live pods on node n whose service list holds s
 *   svc_bits[s * nw + n / 64] bit n % 64 svc_cnt[s][n] > 0
 *   svc_total[s]                         live pods of service s, on any host
 *   svc_max[s]                           the largest count of service s on one host, hosts
 *                                        outside the node list included (spreading.go:72-80)
 *   svc_peer[s]                          -1: no live pod of s; else the host of the one
 *                                        added earliest (predicates.go:293), -2 if that
 *                                        host is not a node
 * with nw = ceil(n_nodes / 64), k < max_conflict_keys, s < n_services. Bits at or above
 * n_nodes in a last word are zero. Every field is specified; none is left to the
 * implementation. Any pointer may be NULL. The call reads what the device holds: pending
 * patches of ksg_add_pod / ksg_remove_pod are applied first, as any kernel would see them,
 * but the host's replay of the last batch is not consulted. KSG_ERR_ARG before the first
 * ksg_set_cluster. On a sharded context, as with ksg_read_requested, the node state is
 * replicated and every rank returns all of it. */
int ksg_read_state(ksg_ctx* ctx, uint64_t* keymap /* max_conflict_keys x ceil(n_nodes/64) */,
                   int32_t* svc_cnt /* n_services x n_nodes */, uint64_t* svc_bits /* n_services x ceil(n_nodes/64) */,
                   int32_t* svc_max, int32_t* svc_total, int32_t* svc_peer /* n_services each */);

/* ---- kubelet admission -------------------------------
 * The node agent re-checks its own pods with the scheduler's predicates
 * (handleNotFittingPods, pkg/kubelet/kubelet.go:1716-1771):
 *   checkNodeSelectorMatching -> PodMatchesNodeLabels          predicates.go:161-167
 *   checkCapacityExceeded     -> CheckPodsExceedingCapacity on
 *                                the pods sorted by creation    predicates.go:104-124
 * These entry points check many nodes' admission sets in one device pass. They
 * use only the context's device and stream (no ksg_set_cluster needed) and do
 * not touch its scheduling state. The caller orders each set's pods (creation
 * order for the capacity check) and interns node label pairs and nodeSelector
 * pairs in one id space (0 = a pair no node has). */
typedef struct ksg_admission_set {
  int64_t cap_milli_cpu;  /* CapacityFromMachineInfo (kubelet/util.go:48-58): NumCores*1000 */
  int64_t cap_memory;     /* ... MemoryCapacity (bytes); 0 = unlimited, as in the reference */
  uint32_t pod_off, n_pods;     /* this set's pods: pods[pod_off, pod_off + n_pods)   */
  uint32_t label_off, n_labels; /* the node's label pair ids: pairs[label_off, ...)   */
} ksg_admission_set;

#define KSG_ADMIT_OK 0
#define KSG_ADMIT_NODESELECTOR 1  /* "nodeSelectorMismatching" (kubelet.go:1757-1763) */
#define KSG_ADMIT_CAPACITY 2      /* "capacityExceeded" (kubelet.go:1765-1770)        */

/* CheckPodsExceedingCapacity per set, greedy in the given order: fits[i] = 1
 * (fitting) or 0 (notFitting); only fitting pods accumulate. */
int ksg_check_pods_exceeding_capacity(ksg_ctx* ctx, const ksg_admission_set* sets, uint32_t n_sets,
                                      const ksg_pod* pods, uint32_t n_pods, uint8_t* fits);
/* PodMatchesNodeLabels: matches[i] = 1 iff every nodeSelector pair of pod i
 * (ids[sel_off, sel_off + n_sel)) is one of its set's node label pairs. */
int ksg_pod_matches_node_labels(ksg_ctx* ctx, const ksg_admission_set* sets, uint32_t n_sets,
                                const ksg_pod* pods, uint32_t n_pods, const uint32_t* ids, uint32_t n_ids,
                                const uint32_t* pairs, uint32_t n_pairs, uint8_t* matches);
/* Both, in the kubelet's order: codes[i] = KSG_ADMIT_NODESELECTOR for a pod
 * whose selector does not match, else the capacity check over the matching pods
 * only (KSG_ADMIT_CAPACITY or KSG_ADMIT_OK). */
int ksg_admit_pods(ksg_ctx* ctx, const ksg_admission_set* sets, uint32_t n_sets, const ksg_pod* pods,
                   uint32_t n_pods, const uint32_t* ids, uint32_t n_ids, const uint32_t* pairs, uint32_t n_pairs,
                   uint8_t* codes);

/* ---- extensions beyond this reference vintage ----
 * BASELINE.json's configs name node taints / pod tolerations, extended (scalar)
 * resources and BalancedResourceAllocation. smarterclayton/kubernetes v0.13 has
 * none of them, so their semantics follow the published later kube-scheduler
 * (v1.10: algorithm/predicates PodToleratesNodeTaints and PodFitsResources'
 * ScalarResources, priorities TaintTolerationPriority + NormalizeReduce and
 * BalancedResourceAllocation) and PARITY IS UNPINNED (no reference to run or
 * table to check against; the C restatement oracle/ksg_oracle.c is the checker).
 * Off unless ksg_set_extensions enables them. On a node-sharded context the node
 * state is replicated as usual and TaintTolerationPriority's NormalizeReduce max
 * (over every shard's filtered nodes) is all-reduced (max) before the scores, per
 * window on the window path and per pod on the per-pod path. Batches take the
 * speculative-window path (otherwise the exact one-pod-at-a-time kernels) unless
 *   - a pod's extended-resource request is outside [0, 2^16], or
 *   - the config has a ServiceAntiAffinity priority and either extension score
 *     is on or a pod of the batch requests an extended resource (with both
 *     scores off and no requests the filters are static per (pod, node) and the
 *     anti-affinity window path takes them, round 6), or
 *   - TaintToleration scores (w_taint_toleration != 0) with max_taints > 64 (the
 *     window path counts a node's taints as one 64-bit mask),
 * on top of the window path's general conditions (ksg_set_window). The reference's
 * own predicates and priorities are unchanged. */
#define KSG_EXT_TAINTS (1u << 0) /* PodToleratesNodeTaints: NoSchedule / NoExecute taints */
#define KSG_EXT_SCALAR (1u << 1) /* extended resources: allocatable >= used + request    */
#define KSG_FAIL_TAINTS 8        /* fail codes after the reference's seven             */
#define KSG_FAIL_SCALAR 9
#define KSG_MAX_SCALAR 4         /* extended resource kinds (e.g. GPU counts)          */

typedef struct ksg_ext_config {
  uint32_t filters;            /* KSG_EXT_* bitmask                                     */
  int32_t w_taint_toleration;  /* TaintTolerationPriority weight (0 = off)              */
  int32_t w_balanced;          /* BalancedResourceAllocation weight (0 = off)           */
  uint32_t n_scalar;           /* extended resource kinds in use (<= KSG_MAX_SCALAR)    */
  uint32_t max_taints;         /* interned taint ids are < max_taints                   */
} ksg_ext_config;

/* Per pod, alongside its ksg_pod. The caller interns each distinct node taint
 * (key, value, effect) and lists the ones the pod's tolerations do NOT tolerate
 * (Toleration.ToleratesTaint: effect empty or equal, key empty or equal,
 * operator Exists or value equal): hard = effect NoSchedule or NoExecute,
 * soft = effect PreferNoSchedule against the tolerations whose effect is empty
 * or PreferNoSchedule. Lists are (offset, count) into the call's id array; each
 * list is a set (a taint id repeated in one list is rejected with KSG_ERR_ARG:
 * TaintTolerationPriority counts each untolerated taint of a node once). */
typedef struct ksg_pod_ext {
  int64_t scalar[KSG_MAX_SCALAR]; /* extended resource requests (0: not requested)   */
  uint32_t hard_off, n_hard;
  uint32_t soft_off, n_soft;
} ksg_pod_ext;

/* Enable extensions; call before ksg_set_cluster (every rank of a sharded
 * context alike; KSG_ERR_ARG for n_scalar > KSG_MAX_SCALAR). */
int ksg_set_extensions(ksg_ctx* ctx, const ksg_ext_config* ext);
/* Per node, after ksg_set_cluster: scalar_cap[r * n_nodes + n] = allocatable of
 * resource r (0: none), node n's taint ids taint_ids[taint_off[n], + taint_n[n]).
 * Resets the extended-resource usage (re-add pods with ksg_add_pod_ext). */
int ksg_set_node_ext(ksg_ctx* ctx, uint32_t n_nodes, const int64_t* scalar_cap, const uint32_t* taint_off,
                     const uint32_t* taint_n, const uint32_t* taint_ids, uint32_t n_taint_ids);
/* The pod-taking entry points with each pod's extension record (ext[i] goes
 * with pods[i]); the plain forms use an all-zero record. */
int ksg_add_pod_ext(ksg_ctx* ctx, uint32_t host_id, const ksg_pod* pod, const ksg_pod_ext* ext,
                    const uint32_t* ids);
int ksg_schedule_batch_ext(ksg_ctx* ctx, const ksg_pod* pods, const ksg_pod_ext* ext, uint32_t n,
                           const uint32_t* ids, uint32_t n_ids, uint64_t* rng_state, int32_t* out_nodes);
int ksg_schedule_begin_ext(ksg_ctx* ctx, const ksg_pod* pod, const ksg_pod_ext* ext, const uint32_t* ids,
                           int64_t* max_score, uint32_t* tie_count, uint8_t* fail_codes);
int ksg_evaluate_ext(ksg_ctx* ctx, const ksg_pod* pod, const ksg_pod_ext* ext, const uint32_t* ids,
                     uint8_t* fail_out, int64_t* score_out);
/* Copy the committed extended-resource usage back to the host, for state checks:
 * used[r * n_nodes + n] = the requests of resource r of every pod on node n
 * (the extended-resource counterpart of ksg_read_requested). */
int ksg_read_ext_used(ksg_ctx* ctx, int64_t* used);

/* ---- A changed node list that keeps the pods ----
 * ksg_set_cluster resets all pod state; ksg_update_cluster replaces the node list (a node
 * joined, left, was cordoned, changed its labels or capacity) and keeps every live pod under
 * its uid. The first seven arguments are ksg_set_cluster's, for the new list; n_services and
 * the config stay as they are (a changed service list needs ksg_set_cluster).
 *
 * Hosts are renamed. old_to_new[r], for each of the old n_nodes ranks (NULL iff there were
 * none), is the host id the pods of old node r now have: below the new n_nodes the node's new
 * rank, at or above it a host outside the list (the node left; its pods count as
 * ksg_add_pod(host_id >= n_nodes) counts them). (outside_old[j], outside_new[j]), j < n_outside,
 * renames a host id that was outside the old list; a new id below n_nodes means that host joined
 * the list and its pods now count on that node. Every outside host that holds a live pod must be
 * listed (listed hosts without pods are harmless), and the whole renaming must be injective. New
 * nodes nothing maps to start empty. ext: ksg_set_node_ext's arrays for the new list, NULL iff
 * the context has no extensions.
 *
 * After KSG_OK every later call's result, and every word ksg_read_requested, ksg_read_state and
 * ksg_read_ext_used return, is what a fresh context gives after ksg_set_cluster with the new
 * arrays and the same n_services, ksg_set_node_ext with `ext`, and ksg_add_pod / ksg_add_pod_ext
 * of every live pod in its original order of addition (commit order for scheduled pods) on its
 * renamed host. So a service's peer is still its earliest-added live member (-2 when that host
 * left the list), svc_max still counts hosts outside the list, and a conflict bit stays while
 * any holder is on the node.
 *
 * Uids stay committed: ksg_remove_pod and the absent_uids lists of ksg_explain_without /
 * ksg_preempt_batch keep working, and so does ksg_batch_unwind of the last batch (it removes by
 * uid and reads out_nodes only for its sign, so the ranks in it may be the old list's). The
 * window setting and the extension config stay. What ends is what ksg_set_cluster ends, except
 * the pods: the static terms (call ksg_set_static_terms / ksg_add_static_config again), the
 * window path's pods-per-window estimate, the resident server (stopped first; the next begin
 * relaunches it). The context never takes a narrower score path than the fresh context would.
 *
 * Nothing is changed and the old node list stays in force for KSG_ERR_STATE (no
 * ksg_set_cluster yet, a ksg_schedule_begin pending, a diverged context, ext given without
 * extensions), KSG_ERR_ARG (ext NULL with extensions on, any of ksg_set_cluster's node / pair
 * checks, old_to_new NULL with old nodes, a live pod on an outside host that is not listed,
 * outside_old[j] below the old n_nodes or repeated, a repeated new id, a taint list out of
 * range) and KSG_ERR_CAPACITY (shard size, max_domains, max_taints); the one visible trace of
 * a call refused after its arguments passed is that the resident server was stopped (the next
 * begin relaunches it). KSG_ERR_HIP marks the context diverged, as a failed batch does. On a sharded context every rank makes the same call
 * (node state is replicated, the shard ranges are recomputed, nothing is exchanged). The pod
 * state moves on the device (ksg_remap.hip): no pod crosses the ABI. */
typedef struct ksg_node_ext_arrays { /* ksg_set_node_ext's arguments, for the new node list */
  const int64_t* scalar_cap;         /* n_scalar x n_nodes */
  const uint32_t* taint_off;
  const uint32_t* taint_n;
  const uint32_t* taint_ids;
  uint32_t n_taint_ids;
} ksg_node_ext_arrays;
int ksg_update_cluster(ksg_ctx* ctx, const ksg_node* nodes, uint32_t n_nodes, const uint32_t* node_pairs,
                       uint32_t n_node_pairs, const uint32_t* pair_keys, uint32_t n_pairs,
                       const uint32_t* old_to_new, const uint32_t* outside_old, const uint32_t* outside_new,
                       uint32_t n_outside, const ksg_node_ext_arrays* ext);
/* Device time of the last ksg_update_cluster's remap kernels (HIP events), ms. */
int ksg_last_update_ms(ksg_ctx* ctx, double* ms);
/* Host time of the last ksg_update_cluster, microseconds: us3[0] validation, us3[1] the device
 * work (the new list's tables, the remap kernels, the joined hosts' patches, the wait), us3[2]
 * the host mirror. */
int ksg_last_update_host_us(ksg_ctx* ctx, double* us3);

/* ---- FitError reports for many pods (the batch path's FailedPredicateMap) ----
 * One device pass evaluates the predicates of n pods against every node, as
 * ksg_evaluate does for one (generic_scheduler.go:30-44, 100-128), without scores:
 *   codes (optional, n * n_nodes bytes): codes[i * n_nodes + node] = the KSG_FAIL_*
 *     code of pod i on that node (0: fits). NULL: no per-node bytes are produced or
 *     copied at all (the backlog question "which pods fit somewhere now": hist[i][0]).
 *   hist (n * KSG_EXPLAIN_SLOTS): hist[i][c] = nodes whose code for pod i is c
 *     (slot 0 = nodes the pod fits); a row sums to n_nodes.
 *   err (n): 1 for a pod whose ServiceAffinity peer is on a host that is not a known
 *     node (predicates.go:293-296; ksg_evaluate's KSG_ERR_NOPEER). Its rows of codes
 *     and hist are zero; the other pods of the call are unaffected.
 * ext (optional, extension contexts): ext[i] goes with pods[i]; NULL = all-zero records.
 * The report is against the state AT THE TIME OF THE CALL: after a batch that is the
 * state with the whole batch committed, the state a retry of the pod would meet. It
 * equals what the sequential reference reported for pod i whenever no pod after i in
 * the batch was placed; otherwise it may differ on the nodes that later pods took
 * (this call does not go back to the state "as of pod i": ksg_explain_without, below, does).
 * Every node of the cluster is covered on every rank of a sharded context (node state
 * is replicated), with no exchange: ranks need not make the call together.
 * uid is ignored: a pod whose uid is committed, or the same pod twice, is legal.
 * n == 0: KSG_OK, nothing written. hist or err NULL with n > 0: KSG_ERR_ARG.
 * KSG_ERR_STATE while a ksg_schedule_begin is pending; KSG_NONODES for an empty node
 * list (nothing written). Pods and id extents are validated as by ksg_schedule_batch.
 * The call changes nothing a later call can observe: not the committed totals, the
 * generator state, the uid bookkeeping, the extended-resource usage or the results of
 * any later batch. Unlike ksg_evaluate it does not look at the pods' requests to decide
 * between the int32 and the int64 score kernels (it computes no score), so it leaves
 * the path later batches take as it was. The pods are processed in chunks whose
 * per-node codes fit a fixed device staging budget (64 MiB). */
#define KSG_EXPLAIN_SLOTS 16   /* histogram slots per pod; codes KSG_FAIL_* 0..9 used */
int ksg_explain_batch(ksg_ctx* ctx, const ksg_pod* pods, const ksg_pod_ext* ext /* NULL: all-zero records */,
                      uint32_t n, const uint32_t* ids, uint32_t n_ids,
                      uint8_t* codes /* optional, n * n_nodes */, uint32_t* hist /* n * KSG_EXPLAIN_SLOTS */,
                      uint8_t* err /* n */);
/* Device time (ms) of the last ksg_explain_batch's kernel launches, from HIP events
 * on the context's stream (the copies out are not in it). Diagnostics. */
int ksg_last_explain_ms(ksg_ctx* ctx, double* ms);

/* ---- FitError reports with committed pods taken away ----
 * ksg_explain_batch against an earlier or a hypothetical state: absent_uids is an ordered
 * list of n_absent committed pods and first_absent[i] pod i's position in it. Row i of
 * codes, hist and err is bit for bit what ksg_explain_batch would write for pod i if
 * ksg_remove_pod had first been called for every uid of
 * absent_uids[first_absent[i] .. n_absent). The order of those removals does not matter:
 * the requested cpu, memory and extended-resource totals subtract with the reference's
 * wrapping arithmetic, as ksg_remove_pod does; a host-port / GCE-PD conflict bit stays
 * while any holder remains on the node; the ServiceAffinity peer is the first remaining
 * member of the pod's service in commit order. A listed pod on a host outside the node
 * list changes only the peer. A peer that becomes an unknown host gives err[i] = 1 and
 * zero rows, as ksg_explain_batch reports it; a peer that stops being one clears the error.
 * Two uses:
 *   - the state AS OF POD i of the last batch, which is what the sequential reference
 *     reported for it (generic_scheduler.go:30-44, 100-128): the list is the batch's
 *     placed pods in order, first_absent[i] the number placed before pod i;
 *   - preemption feasibility, "on which nodes would this pod fit if every lower-priority
 *     pod were evicted": the list is the removable pods sorted by descending priority,
 *     first_absent[i] the first entry below pod i's priority. The library knows no
 *     priorities; the caller's ordering carries them.
 * n_absent == 0, or every first_absent[i] == n_absent: the output is ksg_explain_batch's.
 * Nothing is removed. The call changes nothing a later call can observe: not the
 * committed totals, the generator state, the uid bookkeeping, the extended-resource usage
 * or the results of any later batch, and like ksg_explain_batch it does not look at the
 * pods' requests to decide between the int32 and the int64 score kernels (it computes no
 * score), so it leaves the path later batches take as it was.
 * Protocol and validation are ksg_explain_batch's: ext, uid, n == 0 (KSG_OK, nothing
 * written), hist or err NULL, KSG_ERR_STATE while a ksg_schedule_begin is pending or for
 * ext without extensions, KSG_NONODES for an empty node list, every node covered on every
 * rank of a sharded context with no exchange. The last batch's commits are in the list's
 * reach as soon as ksg_schedule_batch has returned. Also KSG_ERR_ARG, with nothing
 * written: an absent_uids entry that is not a committed uid, the same uid twice,
 * first_absent[i] > n_absent, absent_uids or first_absent NULL with n_absent > 0.
 * The pods are processed in chunks whose per-node codes fit a device staging budget
 * (64 MiB; the environment variable KSG_EXPLAIN_WITHOUT_STAGE_BYTES, read by ksg_create,
 * overrides it). */
int ksg_explain_without(ksg_ctx* ctx, const ksg_pod* pods, const ksg_pod_ext* ext /* NULL: all-zero */,
                        uint32_t n, const uint32_t* ids, uint32_t n_ids,
                        const uint64_t* absent_uids /* n_absent; may be NULL iff n_absent == 0 */,
                        uint32_t n_absent, const uint32_t* first_absent /* n; may be NULL iff n_absent == 0 */,
                        uint8_t* codes /* optional, n * n_nodes */, uint32_t* hist /* n * KSG_EXPLAIN_SLOTS */,
                        uint8_t* err /* n */);
/* Device time (ms) of the last ksg_explain_without's kernel launches, from HIP events on
 * the context's stream (the table upload and the copies out are not in it). Diagnostics. */
int ksg_last_explain_without_ms(ksg_ctx* ctx, double* ms);

/* ---- Preemption: victims per node and the node to preempt on ----
 * The second half of preemption, after ksg_explain_without's "on which nodes would this pod
 * fit if every lower-priority pod were evicted": which of those pods really have to leave,
 * per node, and on which node the eviction hurts least. The model is the later
 * kube-scheduler's selectVictimsOnNode plus pickOneNodeForPreemption (v1.10, without
 * PodDisruptionBudgets); parity is unpinned, and the definition below, in terms of
 * ksg_evaluate, is the specification. The inputs are ksg_explain_without's: n pending pods,
 * an ordered list absent_uids of n_absent committed pods that the caller sorted by descending
 * priority, and per pod i the position first_absent[i] of the first entry below its own
 * priority. The library knows no priorities; the order carries them.
 * For pod i and node x:
 *   - Candidates. C(i,x) is the listed pods at positions >= first_absent[i] whose host is
 *     node x, in list order. Listed pods on hosts outside the node list play no part.
 *   - Base state. S0 is the current state with every pod of C(i,x) removed from node x. If
 *     pod i's fail code on node x in S0 (what ksg_evaluate would report) is not 0, node x is
 *     not a candidate for pod i.
 *   - Reprieve. Otherwise C(i,x) is walked in list order, most important first, with R = {}:
 *     pod c is reprieved (R += c) iff pod i's fail code on node x is still 0 with R + {c} put
 *     back on the node; else c is a victim. V(i,x) = C(i,x) \ R, in list order.
 *   - Only NoDiskConflict, PodFitsPorts, PodFitsResources and the extended resources change
 *     when a pod is put back, exactly as ksg_evaluate tests them: wrapping totals, a capacity
 *     of 0 fits everything, a pod that requests neither cpu nor memory skips
 *     PodFitsResources, an extended resource counts only where the pod requests it. A
 *     candidate that holds a host port or GCE PD the pod lists is therefore always a victim,
 *     and a holder outside C(i,x) makes the node fail in S0. HostName, LabelsPresence and the
 *     other static terms, MatchNodeSelector and the taints do not depend on the pods on the
 *     node; a negative request of a candidate makes the greedy order matter.
 * The node for pod i is the best candidate in this order (ties the project's way, rank
 * descending):
 *   1. the largest top(i,x), the smallest list index in V(i,x), or n_absent when V is empty:
 *      the most important victim is as unimportant as possible, and a node that needs no
 *      eviction beats every node that does;
 *   2. the fewest victims;
 *   3. the highest node rank.
 * v1.10's "smallest sum of victim priorities" criterion needs magnitudes the ordering does
 * not carry and is left out, as are PodDisruptionBudgets.
 * ServiceAffinity: the predicate's peer depends on pods on other nodes, and evicting the
 * peer itself is not a per-node question. A context whose configuration has a
 * ServiceAffinity predicate gets KSG_ERR_STATE (ksg_last_error says why), nothing written;
 * ksg_explain_without stays the tool there.
 * Outputs per pod i: best_node[i] (-1: no candidate), n_victims[i] = |V| on it (the true
 * count even past max_victims), victims[i][..] the first max_victims list indices of V in
 * list order, padded with 0xffffffff, cand_count[i] the candidate nodes and free_count[i]
 * those with an empty V; optionally node_victims[i][x] = |V(i,x)|, KSG_PREEMPT_NOFIT where
 * node x is not a candidate. Invariants: cand_count[i] is ksg_explain_without's hist[i][0]
 * for the same inputs and free_count[i] is ksg_explain_batch's hist[i][0]; with
 * n_absent == 0 or first_absent[i] == n_absent, best_node[i] is the highest-rank fitting
 * node and n_victims[i] is 0.
 * Nothing is removed. The call changes nothing a later call can observe: not the committed
 * totals, the generator state, the uid bookkeeping, the extended-resource usage or the
 * results and the path of any later batch.
 * Protocol and validation are ksg_explain_without's: ext, uid is ignored, n == 0 (KSG_OK,
 * nothing written), KSG_ERR_STATE while a ksg_schedule_begin is pending or for ext without
 * extensions, KSG_NONODES for an empty node list, every node covered on every rank of a
 * sharded context with no exchange. KSG_ERR_ARG, with nothing written: an absent_uids entry
 * that is not a committed uid, the same uid twice, first_absent[i] > n_absent, absent_uids
 * or first_absent NULL with n_absent > 0, best_node, n_victims, cand_count or free_count
 * NULL with n > 0, victims NULL with max_victims > 0, max_victims > KSG_PREEMPT_MAX_VICTIMS.
 * The pods are processed in chunks whose per-node counts and per-tile partial results fit
 * a device staging budget (64 MiB; the environment variable KSG_PREEMPT_STAGE_BYTES, read by
 * ksg_create, overrides it). */
#define KSG_PREEMPT_MAX_VICTIMS 256
#define KSG_PREEMPT_NOFIT 0xffffffffu
int ksg_preempt_batch(ksg_ctx* ctx, const ksg_pod* pods, const ksg_pod_ext* ext /* NULL: all-zero */,
                      uint32_t n, const uint32_t* ids, uint32_t n_ids,
                      const uint64_t* absent_uids /* n_absent; may be NULL iff n_absent == 0 */,
                      uint32_t n_absent, const uint32_t* first_absent /* n; may be NULL iff n_absent == 0 */,
                      uint32_t max_victims /* 0..KSG_PREEMPT_MAX_VICTIMS */,
                      int32_t* best_node /* n; -1: no candidate */,
                      uint32_t* n_victims /* n */,
                      uint32_t* victims /* n * max_victims; NULL iff max_victims == 0 */,
                      uint32_t* cand_count /* n */, uint32_t* free_count /* n */,
                      uint32_t* node_victims /* optional, n * n_nodes */);
/* Device time (ms) of the last ksg_preempt_batch's kernel launches, from HIP events on the
 * context's stream (the table upload and the copies out are not in it). Diagnostics. */
int ksg_last_preempt_ms(ksg_ctx* ctx, double* ms);

/* ---- Ranked hosts for many pods (prioritizeNodes + the sorted HostPriorityList) ----
 * One device pass filters and scores n pods against every node, as ksg_evaluate does
 * for one (generic_scheduler.go:84-96, 136-177), and returns per pod i, against the
 * state AT THE TIME OF THE CALL (as ksg_explain_batch words it):
 *   fit_count[i]: the nodes with fail code 0 (ksg_explain_batch's hist[i][0]).
 *   max_score[i], tie_count[i]: what ksg_schedule_begin would return for the pod now:
 *     the best combined score (Go int: wrapping) and the fitting nodes at it. 0, 0 when
 *     nothing fits, and 0, 0 when the config has priority configs whose weights are all 0
 *     (the empty HostPriorityList; fit_count may still be non-zero). Without priority
 *     configs (EqualPriority fallback) every fitting node scores 1.
 *   top_nodes[i * top + j], top_scores[i * top + j]: entry j of the HostPriorityList in
 *     the reference's order, score descending then node rank descending (types.go:42-47).
 *     L = min(top, fit_count[i]) entries are listed (L = 0 for the empty list above);
 *     the first min(top, tie_count[i]) are the nodes ksg_schedule_commit(tie_index = j)
 *     would pick. Entries j >= L are -1 / 0.
 *   scores (optional, n * n_nodes): scores[i * n_nodes + node] = the combined score
 *     where the pod fits, KSG_SCORE_NOFIT elsewhere: bit-identical to ksg_evaluate's
 *     score_out row of that pod. NULL: no per-node values are produced or copied.
 *   err (n): 1 for a pod whose ServiceAffinity peer is on a host that is not a known
 *     node (predicates.go:293-296). Its max_score, tie_count and fit_count are 0, its top
 *     entries -1 / 0 and its scores row all KSG_SCORE_NOFIT; the other pods are unaffected.
 * Scores are always computed as wrapping int64 (the int32 kernels are proven equal to
 * that while a context is narrow), so unlike ksg_evaluate the call does not look at the
 * pods' requests to choose between the int32 and the int64 kernels and leaves the path
 * later batches take as it was.
 * ext (optional, extension contexts): ext[i] goes with pods[i]; NULL = all-zero records.
 * Every node of the cluster is covered on every rank of a sharded context (node state is
 * replicated; ServiceAntiAffinity's domain counts and TaintToleration's max are taken
 * over all nodes), with no exchange: ranks need not make the call together.
 * uid is ignored. n == 0: KSG_OK, nothing written. KSG_ERR_ARG for max_score, tie_count,
 * fit_count or err NULL with n > 0, for top > KSG_PRIO_MAX_TOP, and for top > 0 with
 * top_nodes or top_scores NULL (both may be NULL iff top == 0). KSG_ERR_STATE while a
 * ksg_schedule_begin is pending, or for ext on a context without extensions; KSG_NONODES
 * for an empty node list. On any of these nothing is written. Pods and id extents are
 * validated as by ksg_schedule_batch, extension records as by ksg_schedule_batch_ext.
 * The call changes nothing a later call can observe: not the committed totals, the
 * generator state, the uid bookkeeping, the extended-resource usage or the results or
 * path of any later batch. The pods are processed in chunks whose per-node scores and
 * per-tile partial results each fit a fixed device staging budget (64 MiB). */
#define KSG_PRIO_MAX_TOP 16
#define KSG_SCORE_NOFIT (-0x7fffffffffffffffLL - 1)  /* what ksg_evaluate's score_out holds where a node does not fit */
int ksg_prioritize_batch(ksg_ctx* ctx, const ksg_pod* pods, const ksg_pod_ext* ext /* NULL: all-zero records */,
                         uint32_t n, const uint32_t* ids, uint32_t n_ids, uint32_t top /* 0..KSG_PRIO_MAX_TOP */,
                         int64_t* max_score /* n */, uint32_t* tie_count /* n */, uint32_t* fit_count /* n */,
                         int32_t* top_nodes /* n * top; may be NULL iff top == 0 */,
                         int64_t* top_scores /* n * top; may be NULL iff top == 0 */,
                         int64_t* scores /* optional, n * n_nodes */, uint8_t* err /* n */);
/* Device time (ms) of the last ksg_prioritize_batch's kernel launches, from HIP events
 * on the context's stream (the copies out are not in it). Diagnostics. */
int ksg_last_prioritize_ms(ksg_ctx* ctx, double* ms);

/* ---- Headroom for many pods: how many copies of a pod each node can take ----
 * The gang-admission and capacity-planning question ("do 64 replicas of this pod fit now",
 * "how many more can the cluster hold, and what runs out first"), answered in one device
 * pass without committing anything. For pod i and node n, against the state AT THE TIME OF
 * THE CALL, the count is the largest k <= limit such that for every j < k the node's fail
 * code for the pod (what ksg_evaluate reports) is 0 once j copies of the pod (distinct uids,
 * otherwise identical) have been added to node n by ksg_add_pod. Copies on other nodes are
 * not part of the definition. The count is > 0 exactly where ksg_explain_batch's code is 0.
 * The predicates of this reference are per-node monotone in the number of copies, so the
 * count is min(limit, the bounds that apply), with, in the fail-code order:
 *   disk    NoDiskConflict is on and the pod has a GCE PD: 1 (the second copy conflicts).
 *   ports   PodFitsPorts is on and the pod has a host port: 1.
 *   cpu     PodFitsResources is on, the pod is not the zero-request pod, the node's
 *           cap_milli_cpu != 0 and milli_cpu > 0: floor((cap - used) / milli_cpu), with the
 *           reference's wrapping subtraction; exact for every int64 capacity and total.
 *   memory  the same with cap_memory and memory.
 *   scalar r (r < n_scalar)  KSG_EXT_SCALAR is on, a record is given and scalar[r] > 0:
 *           floor(((uint64)cap - (uint64)used) / scalar[r]); exact wherever used + scalar[r]
 *           does not overflow int64. Where it does, the count and binding of that (node,
 *           resource) are unspecified (the node still counts as fitting).
 * HostName, LabelsPresence and the static terms, MatchNodeSelector, ServiceAffinity and the
 * taints do not change with copies on the node. Outputs, per pod i:
 *   total[i]      sum of the counts over the nodes. total[i] >= r answers "does a gang of r
 *                 fit", exactly whenever the nodes are independent. They are not in ONE case:
 *                 a ServiceAffinity predicate while the pod's service has no peer yet. The
 *                 first copy placed becomes the peer, and copies on other nodes must then
 *                 share its affinity labels, so there total[i] is an upper bound.
 *   fit_count[i]  nodes with count > 0.   max_count[i]  the largest count.
 *   bind_hist (n * KSG_HEADROOM_SLOTS): bind_hist[i][b] = nodes whose binding is b; a row
 *     sums to n_nodes. The binding of a node is KSG_ROOM_NONE if its count is 0, else the
 *     first constraint in the order above whose bound equals the count (for count < limit:
 *     the refinement of the fail code the node reports once it holds that many copies), or
 *     KSG_ROOM_LIMIT if none does (then count == limit and nothing binds below it).
 *   counts (optional, n * n_nodes): counts[i * n_nodes + node]. NULL: no per-node values are
 *     produced or copied.
 *   err (n): KSG_HEADROOM_ERR_PEER for a pod whose ServiceAffinity peer is on a host that is
 *     not a known node (as ksg_explain_batch reports it), KSG_HEADROOM_ERR_NEGATIVE for a
 *     pod with a negative milli_cpu, memory or scalar[r < n_scalar] (legal elsewhere, but the
 *     count is then not monotone; PEER is reported first). An error row has total, fit_count,
 *     max_count, its bind_hist row and its counts row all zero; the other pods are unaffected.
 * ext (optional, extension contexts): ext[i] goes with pods[i]; NULL skips the extension
 * filters, as an all-zero record passes them.
 * Every node of the cluster is covered on every rank of a sharded context (node state is
 * replicated), with no exchange: ranks need not make the call together.
 * uid is ignored: a pod whose uid is committed, or the same pod twice, is legal.
 * n == 0: KSG_OK, nothing written. KSG_ERR_ARG for total, fit_count, max_count, bind_hist or
 * err NULL with n > 0, and for limit == 0. KSG_ERR_STATE while a ksg_schedule_begin is
 * pending, or for ext on a context without extensions; KSG_NONODES for an empty node list.
 * On any of these nothing is written. Pods and id extents are validated as by
 * ksg_schedule_batch, extension records as by ksg_schedule_batch_ext.
 * The call changes nothing a later call can observe: not the committed totals, the
 * generator state, the uid bookkeeping, the extended-resource usage or the results or path
 * of any later batch (it computes no score and does not look at the pods' requests to choose
 * between the int32 and the int64 kernels). The pods are processed in chunks whose per-node
 * counts fit a fixed device staging budget (64 MiB; KSG_HEADROOM_STAGE_BYTES in the
 * environment at ksg_create overrides it: a test knob). */
#define KSG_HEADROOM_SLOTS 16
#define KSG_ROOM_NONE 0
#define KSG_ROOM_LIMIT 1
#define KSG_ROOM_DISK 2
#define KSG_ROOM_PORTS 3
#define KSG_ROOM_CPU 4
#define KSG_ROOM_MEMORY 5
#define KSG_ROOM_SCALAR0 6      /* + r, r < KSG_MAX_SCALAR */
#define KSG_HEADROOM_ERR_PEER 1
#define KSG_HEADROOM_ERR_NEGATIVE 2
int ksg_headroom_batch(ksg_ctx* ctx, const ksg_pod* pods, const ksg_pod_ext* ext /* NULL: all-zero */,
                       uint32_t n, const uint32_t* ids, uint32_t n_ids, uint32_t limit /* >= 1 */,
                       uint64_t* total /* n: sum of counts */, uint32_t* fit_count /* n: nodes with count > 0 */,
                       uint32_t* max_count /* n */, uint32_t* bind_hist /* n * KSG_HEADROOM_SLOTS */,
                       uint32_t* counts /* optional, n * n_nodes */, uint8_t* err /* n */);
/* Device time (ms) of the last ksg_headroom_batch's kernel launches, from HIP events
 * on the context's stream (the copies out are not in it). Diagnostics. */
int ksg_last_headroom_ms(ksg_ctx* ctx, double* ms);

/* ---- First-fit pod sets: does a set of different pods fit together ----
 * The drain, scale-down and gang-admission question ("if node x goes, do its pods all find
 * room elsewhere", "do this driver and its workers fit now"), where a pod's placement changes
 * what the next pod of the set sees: ksg_headroom_batch's total answers it for copies of one
 * template only, and ksg_explain_batch judges every pod against the same state. Every set is
 * packed on the device, independently and in parallel, without committing anything. The
 * definition, in terms of ksg_explain_batch and ksg_add_pod, is the specification:
 *   - Sets are independent: no set sees another set's placements. Set s owns the next
 *     set_size[s] pods of the call; the sizes sum to n.
 *   - For set s, start from the state AT THE TIME OF THE CALL. Its pods are p_0 .. p_{m-1}, in
 *     the given order. For j = 0 .. m-1:
 *     1. F is the nodes where ksg_explain_batch would report code 0 for p_j, with ext passed
 *        the same way (ext == NULL skips the extension filters there too), less
 *        set_exclude[s] and every node whose target_words bit is clear. Bits at or past
 *        n_nodes are ignored.
 *     2. If F is empty, out_nodes of p_j is KSG_OUT_NOFIT and the set goes on with p_{j+1}.
 *     3. Otherwise t = the highest rank in F and out_nodes of p_j is t. Before p_{j+1} is
 *        looked at, p_j counts as added to node t by ksg_add_pod / ksg_add_pod_ext under a
 *        fresh uid.
 *   - What counts as added: the pod's cpu, memory and extended-resource requests join the
 *     node's totals with the reference's wrapping arithmetic (so a negative request makes
 *     room), and every host port and GCE PD id it lists is held on t from then on, in the one
 *     conflict-key id space: a key one pod lists as a port blocks a later pod that lists it as
 *     a PD, as the keymap does.
 *   - placed[s] is the number of pods of the set that found a node. The set fits iff
 *     placed[s] == set_size[s]. A set of size 0 is legal: placed[s] is 0.
 * First fit by descending rank is deterministic and cheap; it is a feasibility heuristic, as
 * the cluster autoscaler's drain simulation is. A full placed[s] PROVES that a packing exists;
 * a short one does NOT prove that none does. The caller's order is the heuristic's lever:
 * largest pods first. Scores play no part, so HostName, LabelsPresence and the static terms,
 * MatchNodeSelector and the taints are per (pod, node) constants; only NoDiskConflict,
 * PodFitsPorts, PodFitsResources and the extended resources see the set's earlier pods.
 * Invariants: with every set of size 1, no exclusion and no mask, out_nodes is
 * ksg_preempt_batch's best_node with n_absent == 0; one set of k copies of a pod without ports
 * or PDs and with non-negative requests fills the nodes, highest rank first, with
 * ksg_headroom_batch's counts.
 * ServiceAffinity: a set's first member can become the predicate's peer for the rest, which is
 * not a per-node question (ksg_preempt_batch's reason). A context whose configuration has a
 * ServiceAffinity predicate gets KSG_ERR_STATE (ksg_last_error says why), nothing written.
 * Protocol and validation are the read-only queries'. ext[i] goes with pods[i], and uid is
 * ignored. KSG_ERR_STATE while a ksg_schedule_begin is pending, or for ext on a context without
 * extensions. KSG_NONODES for an empty node list (n_sets > 0). Every node is covered on every
 * rank of a sharded context, with no exchange. n_sets == 0: KSG_OK, nothing written; n must
 * then be 0. KSG_ERR_ARG, with nothing written: set_size NULL with n_sets > 0, sizes that do not
 * sum to n, a size above KSG_PACK_MAX_SET, more than 2^31 - 1 sets (all sets go in one launch,
 * one workgroup each), a set_exclude entry that is neither below n_nodes nor KSG_PACK_NO_NODE,
 * out_nodes NULL with n > 0, placed NULL with n_sets > 0.
 * The call changes nothing a later call can observe: not the committed totals, the keymap,
 * the service tables, the generator state, the uid bookkeeping, the extended-resource usage or
 * the results and the path of any later batch (like its siblings it does not look at the
 * requests to decide between the int32 and the int64 score kernels).
 * One workgroup packs one set, its pods one after another: the sets of a call run in parallel,
 * one large set is serial work. All sets go in one launch, and no node count is too large: a
 * set's own placements live in a table sized by KSG_PACK_MAX_SET, not by the cluster. A pod that
 * lists host ports or GCE PDs, or requests an extended resource, also reads the records of the
 * set's earlier such pods on every node the set has touched: quadratic in the pods of one set
 * that pile onto a node, inside that one workgroup (unmeasured beyond the serial case). */
#define KSG_PACK_NO_NODE 0xffffffffu
#define KSG_PACK_MAX_SET 1024   /* pods per set */
int ksg_pack_batch(ksg_ctx* ctx, const ksg_pod* pods, const ksg_pod_ext* ext /* NULL: all-zero */,
                   uint32_t n, const uint32_t* ids, uint32_t n_ids,
                   const uint32_t* set_size    /* n_sets; sums to n: set s owns the next set_size[s] pods */,
                   const uint32_t* set_exclude /* n_sets node ranks or KSG_PACK_NO_NODE; NULL: none excluded */,
                   uint32_t n_sets,
                   const uint64_t* target_words /* optional, ceil(n_nodes/64): bit set = node may take pods */,
                   int32_t* out_nodes /* n: node rank or KSG_OUT_NOFIT */,
                   uint32_t* placed   /* n_sets: pods of the set that found a node */);
/* Device time (ms) of the last ksg_pack_batch's kernel launch, from HIP events on the
 * context's stream (the table upload and the copies out are not in it). Diagnostics. */
int ksg_last_pack_ms(ksg_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* KSCHEDGPU_H_ */
