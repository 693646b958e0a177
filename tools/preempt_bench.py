"""ksg_preempt_batch against ksg_explain_without (the feasibility half it extends) and against
the only other route to the same answer, mutating the live state through the ABI.

A config-2 cluster (default 5,000 nodes) is filled in `--batch`-pod (1,000) batches until a
batch leaves pods without a node; the next `--batch` pods of the stream are the pending pods.
The list is EVERY committed pod under a synthetic priority (a hash of the uid, 0..7), sorted by
descending priority (stable); a pending pod has a synthetic priority 1..8 and its position is the
first entry below it. Over the pending pods:

  a  ksg_explain_without(codes = NULL)          (feasibility only: the expectation to report against)
  b  ksg_preempt_batch without node_victims
  c  ksg_preempt_batch with node_victims
  d  the mutate-and-evaluate route on `--walk` (3) of the pods: ksg_remove_pod for every pod the
     pending pod may evict, ksg_evaluate, then ksg_add_pod + ksg_evaluate per removed pod (and
     ksg_remove_pod again for a victim), through the Python wrappers; scaled to per pod. Its
     per-node victim counts must equal c's rows.

Wall ms (host clock around calls that end in a stream synchronise) and kernel ms (HIP events,
ksg_last_explain_without_ms / ksg_last_preempt_ms), each the median of `--runs` (20) after
`--warmup` (5), the three forms alternating run by run. The result goes to `--out`
(profiles/preempt_batch.json) and, as one JSON line, to stdout. Needs the GPU.

    python tools/preempt_bench.py [--nodes 5000] [--batch 1000] [--out profiles/preempt_batch.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _prio(uids, salt):
    """a synthetic priority 0..7 per uid (splitmix64's finaliser)"""
    z = (np.asarray(uids, np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return ((z ^ (z >> np.uint64(31))) % np.uint64(8)).astype(np.int64)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--max-fill", type=int, default=400000)
    ap.add_argument("--max-victims", type=int, default=16)
    ap.add_argument("--walk", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preempt_batch.json"))
    a = ap.parse_args()

    from kubernetes_amd import abi, ingest, podstream, workload
    from kubernetes_amd.engine import DeviceScheduler, PodBatch
    from tools.srcsha import kernel_src_sha

    w = workload.build("config2", n_nodes=a.nodes, n_pods=a.max_fill, pod_stream=True)
    it = ingest.Interner()
    for k in w.config.label_keys():
        it.key_id(k)
    view = ingest.ClusterView(w.nodes, w.services, it)
    stream = podstream.ingest_stream(view, w.stream, aff_labels=w.config.affinity_labels())
    dev = DeviceScheduler(w.config.compile(it.key_id), device=0)
    dev.set_cluster(view.arrays)
    lib, ctx = dev._lib, dev._ctx
    N = a.nodes
    ids = np.ascontiguousarray(stream.ids, dtype=np.uint32)

    # fill until a batch leaves pods unplaced
    state, filled, hosts = workload.TIEBREAK_SEED, 0, []
    while True:
        if filled + 2 * a.batch > len(stream):
            raise SystemExit(f"the cluster is not full after {filled} pods: raise --max-fill")
        out, state = dev.batch(PodBatch(stream.pods[filled:filled + a.batch], stream.ids), state)
        hosts.append(out.copy())
        filled += a.batch
        if (out < 0).any():
            break
    host_of = np.concatenate(hosts)
    placed = np.flatnonzero(host_of >= 0)  # indices into the stream
    uids = stream.pods["uid"][placed].astype(np.uint64)
    order = np.argsort(-_prio(uids, 1), kind="stable")
    listed, listed_idx = np.ascontiguousarray(uids[order]), placed[order]
    lprio = _prio(listed, 1)
    pend = np.ascontiguousarray(stream.pods[filled:filled + a.batch], dtype=abi.POD_DTYPE)
    n = len(pend)
    mine = _prio(pend["uid"], 2) + 1
    pos = np.array([(lprio >= p).sum() for p in mine], np.uint32)  # the first entry below the pod's priority
    na, mv = len(listed), a.max_victims

    hist, err = np.zeros((n, abi.EXPLAIN_SLOTS), np.uint32), np.zeros(n, np.uint8)
    outs = {x: (np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros((n, mv), np.uint32), np.zeros(n, np.uint32),
                np.zeros(n, np.uint32)) for x in "bc"}
    per_node = np.zeros((n, N), np.uint32)
    kms = C.c_double(0)

    def call(which):
        t = time.perf_counter()
        if which == "a":
            rc = lib.ksg_explain_without(ctx, abi.ptr(pend), None, n, abi.ptr(ids), len(ids), abi.ptr(listed), na,
                                         abi.ptr(pos), None, abi.ptr(hist), abi.ptr(err))
        else:
            b, v, vl, cnd, fr = outs[which]
            rc = lib.ksg_preempt_batch(ctx, abi.ptr(pend), None, n, abi.ptr(ids), len(ids), abi.ptr(listed), na, abi.ptr(pos),
                                       mv, abi.ptr(b), abi.ptr(v), abi.ptr(vl), abi.ptr(cnd), abi.ptr(fr),
                                       abi.ptr(per_node) if which == "c" else None)
        dt = time.perf_counter() - t
        if rc != abi.KSG_OK:
            raise SystemExit(f"call {which}: {rc} {lib.ksg_last_error(ctx)}")
        (lib.ksg_last_explain_without_ms if which == "a" else lib.ksg_last_preempt_ms)(ctx, C.byref(kms))
        return dt * 1e3, kms.value

    # alternate the three forms run by run, so that drift on a shared host hits them alike
    for _ in range(a.warmup):
        for x in "abc":
            call(x)
    runs = {x: [] for x in "abc"}
    for _ in range(a.runs):
        for x in "abc":
            runs[x].append(call(x))

    # d: the mutate-and-evaluate route for a few pods that have something to evict
    fill_batch = PodBatch(stream.pods[:filled], stream.ids)
    pend_batch = PodBatch(pend, stream.ids)
    walked = [int(i) for i in np.flatnonzero((outs["c"][3] > 0) & (pos < na))[: a.walk]]
    walk_ms, walk_ok, walk_calls = [], True, 0
    for i in walked:
        cands = list(range(int(pos[i]), na))
        t = time.perf_counter()
        for j in cands:
            dev.remove_pod(int(listed[j]))
        ok = dev.evaluate(pend_batch, i)[1] == 0
        row = np.where(ok, 0, abi.PREEMPT_NOFIT).astype(np.uint32)
        gone = []
        for j in cands:
            host = int(host_of[listed_idx[j]])
            dev.add_pod(host, fill_batch, int(listed_idx[j]))
            if not ok[host]:
                continue
            if dev.evaluate(pend_batch, i)[1][host] != 0:
                dev.remove_pod(int(listed[j]))
                gone.append(j)
                row[host] += 1
        walk_ms.append((time.perf_counter() - t) * 1e3)
        walk_calls += 2 * len(cands) + 1 + int(ok[host_of[listed_idx[cands]]].sum()) + len(gone)
        for j in gone:  # (untimed: back to the state the device calls saw)
            dev.add_pod(int(host_of[listed_idx[j]]), fill_batch, int(listed_idx[j]))
        walk_ok = walk_ok and bool(np.array_equal(row, per_node[i]))
    dev.close()

    m = statistics.median
    wall = {x: m([r[0] for r in runs[x]]) for x in "abc"}
    kern = {x: m([r[1] for r in runs[x]]) for x in "abc"}
    same = all(np.array_equal(p, q) for p, q in zip(outs["b"], outs["c"]))
    cand_is_hist = bool(np.array_equal(outs["c"][3], hist[:, 0]))
    per_pod_walk = m(walk_ms) if walk_ms else None
    res = {
        "workload": "config2", "nodes": N, "pods_filled": int(filled), "listed": int(na), "pending": n,
        "max_victims": mv, "warmup": a.warmup, "runs": a.runs, "kernel_src_sha": kernel_src_sha(),
        "pending_that_fit_as_things_stand": int((outs["c"][4] > 0).sum()),
        "pending_with_a_preemption": int(((outs["c"][4] == 0) & (outs["c"][3] > 0)).sum()),
        "pending_without_candidate": int((outs["c"][3] == 0).sum()),
        "mean_victims_on_the_chosen_node": float(outs["c"][1][(outs["c"][4] == 0) & (outs["c"][3] > 0)].mean())
        if ((outs["c"][4] == 0) & (outs["c"][3] > 0)).any() else 0.0,
        "a_explain_without_ms": wall["a"], "a_kernel_ms": kern["a"],
        "b_preempt_ms": wall["b"], "b_kernel_ms": kern["b"],
        "c_preempt_per_node_ms": wall["c"], "c_kernel_ms": kern["c"],
        "kernel_ratio_b_over_a": kern["b"] / kern["a"] if kern["a"] > 0 else None,
        "kernel_ratio_c_over_a": kern["c"] / kern["a"] if kern["a"] > 0 else None,
        "d_walked_pods": walked, "d_mutate_route_ms_per_pod": per_pod_walk, "d_abi_calls": walk_calls,
        "d_mutate_route_ms_scaled_to_pending": per_pod_walk * n if per_pod_walk is not None else None,
        "wall_speedup_c_over_d_scaled": per_pod_walk * n / wall["c"] if per_pod_walk is not None else None,
        "b_identical_to_c": bool(same), "cand_count_is_explain_without_hist0": cand_is_hist,
        "d_rows_identical_to_c": walk_ok,
        "spread_ms": {x: [min(r[0] for r in runs[x]), max(r[0] for r in runs[x])] for x in "abc"},
        "spread_kernel_ms": {x: [min(r[1] for r in runs[x]), max(r[1] for r in runs[x])] for x in "abc"},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return 0 if same and cand_is_hist and walk_ok else 1


if __name__ == "__main__":
    sys.exit(main())
