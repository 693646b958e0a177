// ksg_launch.h — the host launchers the .hip files define and the host runtime calls.
// Included by both sides, so each declaration meets its definition in one translation unit;
// default arguments live here only.
#ifndef KSG_LAUNCH_H_
#define KSG_LAUNCH_H_

#include <hip/hip_runtime.h>

#include "ksg_internal.h"

// ksg_kernels.hip
hipError_t ksg_launch_batch(int R, bool anti, const KsgDev& d, const ksg_pod* pods,
                            const uint32_t* ids, uint32_t n, uint64_t* rng, int32_t* out,
                            hipStream_t st, const ksg_pod_ext* ext = nullptr);
hipError_t ksg_launch_scan(int R, bool anti, const KsgDev& d, const ksg_pod* pods,
                           const uint32_t* ids, int mode, int phase, uint8_t* fail_out,
                           int64_t* score_out, uint8_t* record, int32_t* dpart,
                           const int32_t* dglobal, hipStream_t st, const ksg_pod_ext* ext = nullptr);
hipError_t ksg_launch_decide(const KsgDev& d, const ksg_pod* pods, const uint32_t* ids,
                             const uint8_t* records, uint32_t rec_bytes, uint32_t world,
                             const uint32_t* shard_wlo, int mode, uint64_t tie_index,
                             uint64_t* rng, int32_t* out, uint32_t out_idx, int64_t* summary,
                             hipStream_t st, const ksg_pod_ext* ext = nullptr);
hipError_t ksg_launch_static(const KsgStaticCfg& sc, uint32_t n_nodes, const ksg_node* nodes,
                             const uint32_t* node_pairs, const uint32_t* pair_keys,
                             const int32_t* dom_of_pair, uint32_t n_pairs, uint32_t nw,
                             uint64_t* static_fit, int64_t* static_score, int32_t* anti_domain,
                             int32_t* aff_pair, unsigned long long* pairmap, hipStream_t st);
hipError_t ksg_launch_static_terms(const KsgStaticCfg& sc, uint32_t n_nodes, const ksg_node* nodes,
                                   const uint32_t* node_pairs, const uint32_t* pair_keys, uint32_t n_pairs, uint32_t nw,
                                   uint64_t* fit, int64_t* score, hipStream_t st);
hipError_t ksg_launch_static_fold(uint64_t* static_fit, int64_t* static_score, const uint64_t* xfit,
                                  const int64_t* xscore, uint32_t nw, uint32_t n, int own_fit, int own_score,
                                  hipStream_t st);
hipError_t ksg_launch_zonemap(uint32_t n_nodes, const int32_t* anti_domain, uint32_t d0, uint32_t nw,
                              uint64_t* zmap, hipStream_t st);
hipError_t ksg_launch_patch(const KsgPatch* patches, uint32_t n, hipStream_t st);

// ksg_window.hip
hipError_t ksg_launch_win_eval(const KsgDev& d, int mode, const ksg_pod* batch, const uint32_t* ids,
                               const KsgWinRun* run, uint32_t wcap, KsgWinSum* sums, uint64_t* wbits, int32_t* wmax,
                               uint32_t ostride, int32_t* dcnt, uint64_t* wfit, int32_t* dmb, uint64_t* wbz,
                               uint32_t dz, hipStream_t st, const ksg_pod_ext* exts = nullptr,
                               int32_t* tmax = nullptr, uint64_t* psoft = nullptr, int32_t* thist = nullptr);
uint32_t ksg_win_max_window(const KsgDev& d);
hipError_t ksg_launch_win_resolve(const KsgDev& d, uint32_t wcap, KsgWinRun* run, const KsgWinSum* sums,
                                  const KsgWinXchg& x, uint64_t* rng, int32_t* out, hipStream_t st);

// ksg_plain.hip
uint32_t ksg_win_t0_stride(const KsgDev& d);
hipError_t ksg_launch_win_t0(const KsgDev& d, uint32_t wcap, const KsgWinRun* run, const KsgWinXchg& x,
                             hipStream_t st);
bool ksg_win_fused_ok(const KsgDev& d);
uint32_t ksg_win_fused_groups(const KsgDev& d, uint32_t wcap);
hipError_t ksg_launch_win_fused(const KsgDev& d, uint32_t wcap, KsgWinRun* run, const KsgWinSum* sums,
                                const KsgWinXchg& x, uint64_t* rng, int32_t* out, const KsgFused& f, uint32_t grid,
                                hipStream_t st);

// ksg_serve.hip, ksg_admit.hip, ksg_explain.hip
hipError_t ksg_launch_serve(int R, bool anti, bool ext, const KsgDev& d, const KsgSrvArgs& a, hipStream_t st);
hipError_t ksg_launch_serve_grid(int npt, bool ext, const KsgDev& d, const KsgSrvArgs& a, hipStream_t st);
hipError_t ksg_launch_admit(const ksg_admission_set* sets, uint32_t n_sets, const ksg_pod* pods,
                            const uint32_t* ids, const uint32_t* pairs, int mode, uint8_t* out, hipStream_t st);
hipError_t ksg_launch_explain(const KsgDev& d, const ksg_pod* pods, const ksg_pod_ext* exts, const uint32_t* ids,
                              uint32_t n_pods, uint8_t* codes, uint32_t* hist, uint8_t* err, hipStream_t st);

// ksg_explain_without.hip (w.first_absent and w.peer are indexed from `pods`, like the outputs)
hipError_t ksg_launch_explain_without(const KsgDev& d, const KsgWithout& w, const ksg_pod* pods, const ksg_pod_ext* exts,
                                      const uint32_t* ids, uint32_t n_pods, uint8_t* codes, uint32_t* hist, uint8_t* err,
                                      hipStream_t st);

// ksg_preempt.hip (every per-pod array, w.first_absent included, is indexed from `pods`; part =
// KsgPreemptPart[n_pods][ksg_preempt_tiles(d)]; w.peer is not read)
uint32_t ksg_preempt_tiles(const KsgDev& d);
hipError_t ksg_launch_preempt(const KsgDev& d, const KsgWithout& w, const KsgPreemptKeys& ek, const ksg_pod* pods,
                              const ksg_pod_ext* exts, const uint32_t* ids, uint32_t n_pods, uint32_t max_victims,
                              uint32_t* node_victims, KsgPreemptPart* part, int32_t* best_node, uint32_t* n_victims,
                              uint32_t* victims, uint32_t* cand_count, uint32_t* free_count, hipStream_t st);

// ksg_pack.hip (one workgroup per set; out_nodes = int32[k.set_off[n_sets]], placed = uint32[n_sets])
hipError_t ksg_launch_pack(const KsgDev& d, const KsgPack& k, const ksg_pod* pods, const ksg_pod_ext* exts,
                           const uint32_t* ids, uint32_t n_sets, int32_t* out_nodes, uint32_t* placed, hipStream_t st);

// ksg_headroom.hip (the per-pod arrays are indexed from `pods`; div: udiv_capped's variant)
hipError_t ksg_launch_headroom(const KsgDev& d, const ksg_pod* pods, const ksg_pod_ext* exts, const uint32_t* ids,
                               uint32_t n_pods, uint32_t limit, int div, uint32_t* counts, uint64_t* total,
                               uint32_t* max_count, uint32_t* fit_count, uint32_t* hist, uint8_t* err, hipStream_t st);

// ksg_prioritize.hip (all per-pod arrays are indexed from `pods`; dnorm = int32[n_pods][D + 1]:
// a pod's ServiceAntiAffinity domain counts, then its TaintToleration max)
bool ksg_prio_needs_reduce(const KsgDev& d, bool have_ext);
hipError_t ksg_launch_prio_reduce(const KsgDev& d, const ksg_pod* pods, const ksg_pod_ext* exts, const uint32_t* ids,
                                  uint32_t n_pods, int32_t* dnorm, hipStream_t st);
hipError_t ksg_launch_prio_score(const KsgDev& d, const ksg_pod* pods, const ksg_pod_ext* exts, const uint32_t* ids,
                                 uint32_t n_pods, uint32_t top, const int32_t* dnorm, int64_t* scores,
                                 KsgPrioPart* part, int64_t* cand_score, int32_t* cand_node, uint8_t* err,
                                 hipStream_t st);
hipError_t ksg_launch_prio_merge(const KsgDev& d, uint32_t n_pods, uint32_t top, const KsgPrioPart* part,
                                 const int64_t* cand_score, const int32_t* cand_node, int64_t* max_score,
                                 uint32_t* tie_count, uint32_t* fit_count, int32_t* top_nodes, int64_t* top_scores,
                                 hipStream_t st);

// ksg_remap.hip (ksg_update_cluster): src[new_n] = the old rank behind each new rank or -1, every
// entry below old_n (the host checks); rows are [rows][old_n] -> [rows][new_n], bitmap rows
// [rows][old_nw] -> [rows][new_nw]. Nothing is launched for an empty grid.
hipError_t ksg_launch_remap_rows64(const int64_t* old_rows, int64_t* new_rows, const int32_t* src, uint32_t old_n,
                                   uint32_t new_n, uint32_t rows, hipStream_t st);
hipError_t ksg_launch_remap_rows32(const int32_t* old_rows, int32_t* new_rows, const int32_t* src, uint32_t old_n,
                                   uint32_t new_n, uint32_t rows, hipStream_t st);
hipError_t ksg_launch_remap_bits(const uint64_t* old_rows, uint64_t* new_rows, const int32_t* src, uint32_t old_nw,
                                 uint32_t new_nw, uint32_t new_n, uint32_t rows, hipStream_t st);
hipError_t ksg_launch_remap_svc(const int32_t* new_cnt, uint32_t new_n, uint32_t n_services, const int32_t* outside_max,
                                const int32_t* peer, const int32_t* old_total, int32_t* svc_max, int32_t* svc_total,
                                int32_t* svc_peer, hipStream_t st);

#endif  // KSG_LAUNCH_H_
