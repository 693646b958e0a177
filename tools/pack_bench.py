"""ksg_pack_batch against one predicate pass over the same pods (ksg_explain_batch without
codes) and against the only other route to the same answer, mutating a context through the ABI.

A config-2 cluster (default 5,000 nodes) is filled in `--batch`-pod (1,000) batches until a batch
leaves pods without a node; the pods after it in the stream are the pending pods. Three cases:

  a  drain every node: one set per node, the node's own committed pods in commit order, that
     node excluded
  b  `--gangs` (1,000) gangs of 8 consecutive pending pods
  c  one set of KSG_PACK_MAX_SET pending pods: one workgroup's serial work, the worst case

Per case: ksg_pack_batch's wall ms (host clock around the call, which ends in a stream
synchronise) and kernel ms (HIP events, ksg_last_pack_ms), and ksg_explain_batch(codes = NULL)
over the same pods likewise, each the median of `--runs` (10) after `--warmup` (3), the two calls
alternating run by run. Then the route without the call, on `--walk` (3) sets of the case (the
first, the middle and the last) on a second context loaded the same way: per pod
ksg_explain_batch of the one pod with codes, ksg_add_pod on the highest open node with code 0,
and after the set ksg_remove_pod of all of them, through the Python wrappers; its rows must equal
the call's, and its time per set is scaled to the case's sets.

The result goes to `--out` (profiles/pack_batch.json) and, as one JSON line, to stdout. Needs the
GPU.

    python tools/pack_bench.py [--nodes 5000] [--batch 1000] [--out profiles/pack_batch.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--max-fill", type=int, default=400000)
    ap.add_argument("--gangs", type=int, default=1000)
    ap.add_argument("--walk", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_batch.json"))
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
    cfg = w.config.compile(it.key_id)
    N = a.nodes

    def filled_context():
        """a context filled until a batch leaves pods unplaced -> (context, pods filled, their hosts)"""
        dev = DeviceScheduler(cfg, device=0)
        dev.set_cluster(view.arrays)
        state, filled, hosts = workload.TIEBREAK_SEED, 0, []
        while True:
            if filled + a.batch + max(8 * a.gangs, abi.PACK_MAX_SET) > len(stream):
                raise SystemExit(f"the cluster is not full after {filled} pods: raise --max-fill")
            out, state = dev.batch(PodBatch(stream.pods[filled:filled + a.batch], stream.ids), state)
            hosts.append(out.copy())
            filled += a.batch
            if (out < 0).any():
                return dev, filled, np.concatenate(hosts)

    dev, filled, host_of = filled_context()
    placed = np.flatnonzero(host_of >= 0)
    by_node = placed[np.argsort(host_of[placed], kind="stable")]  # grouped by node, commit order within
    sizes_a = np.bincount(host_of[placed], minlength=N).astype(np.uint32)
    if sizes_a.max() > abi.PACK_MAX_SET:
        raise SystemExit("a node holds more pods than KSG_PACK_MAX_SET")
    pend = stream.pods[filled:]
    cases = {
        "a": (PodBatch(np.ascontiguousarray(stream.pods[by_node]), stream.ids), sizes_a, np.arange(N, dtype=np.uint32)),
        "b": (PodBatch(np.ascontiguousarray(pend[: 8 * a.gangs]), stream.ids), np.full(a.gangs, 8, np.uint32), None),
        "c": (PodBatch(np.ascontiguousarray(pend[: abi.PACK_MAX_SET]), stream.ids),
              np.array([abi.PACK_MAX_SET], np.uint32), None),
    }

    res = {"workload": "config2", "nodes": N, "pods_filled": int(filled), "pods_committed": int(len(placed)),
           "warmup": a.warmup, "runs": a.runs, "kernel_src_sha": kernel_src_sha(), "strip": None, "cases": {}}
    res["strip"] = int(open(os.path.join(ROOT, "kubernetes_amd", "csrc", "ksg_internal.h")).read()
                       .split("#define KSG_PACK_STRIP ")[1].split()[0])
    rows = {}
    m = statistics.median
    for name, (batch, sizes, excl) in cases.items():
        def pack():
            t = time.perf_counter()
            out = dev.pack(batch, sizes, exclude=excl)
            return (time.perf_counter() - t) * 1e3, dev.last_pack_ms(), out

        def explain():
            t = time.perf_counter()
            dev.explain(batch, want_codes=False)
            return (time.perf_counter() - t) * 1e3, dev.last_explain_ms()

        for _ in range(a.warmup):
            pack(), explain()
        pr, er = [], []
        for _ in range(a.runs):
            pr.append(pack())
            er.append(explain())
        out, placed_sets = pr[-1][2]
        rows[name] = (out, placed_sets)
        res["cases"][name] = {
            "sets": int(len(sizes)), "pods": int(len(batch)), "largest_set": int(sizes.max()),
            "sets_that_fit": int((placed_sets == sizes).sum()), "pods_placed": int((out >= 0).sum()),
            "pack_ms": m([r[0] for r in pr]), "pack_kernel_ms": m([r[1] for r in pr]),
            "explain_ms": m([r[0] for r in er]), "explain_kernel_ms": m([r[1] for r in er]),
            "kernel_ratio_pack_over_explain": m([r[1] for r in pr]) / m([r[1] for r in er]),
            "spread_pack_kernel_ms": [min(r[1] for r in pr), max(r[1] for r in pr)],
            "spread_explain_kernel_ms": [min(r[1] for r in er), max(r[1] for r in er)],
        }
    dev.close()

    # the route without the call, on a second context
    twin, filled2, host2 = filled_context()
    assert filled2 == filled and np.array_equal(host2, host_of)
    all_ok = True
    for name, (batch, sizes, excl) in cases.items():
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        ns = len(sizes)
        walked = sorted({0, ns // 2, ns - 1})[: a.walk]
        ms, calls, ok = [], 0, True
        for s in walked:
            uid, added = 7 * 10 ** 9, []
            got = np.full(int(sizes[s]), abi.KSG_OUT_NOFIT, np.int32)
            t = time.perf_counter()
            for j in range(int(sizes[s])):
                one = batch.one(int(off[s]) + j)
                fit = twin.explain(one)[0][0] == 0
                if excl is not None:
                    fit[int(excl[s])] = False
                f = np.flatnonzero(fit)
                calls += 1
                if len(f):
                    one.pods["uid"] = uid + j
                    twin.add_pod(int(f[-1]), one, 0)
                    added.append(uid + j)
                    got[j] = f[-1]
                    calls += 1
            for u in added:
                twin.remove_pod(u)
            calls += len(added)
            ms.append((time.perf_counter() - t) * 1e3)
            ok = ok and bool(np.array_equal(got, rows[name][0][off[s]: off[s + 1]]))
        c = res["cases"][name]
        c["mutate_route_sets_walked"] = [int(s) for s in walked]
        c["mutate_route_pods_walked"] = int(sum(int(sizes[s]) for s in walked))
        c["mutate_route_abi_calls"] = calls
        c["mutate_route_ms_per_set"] = statistics.mean(ms)
        c["mutate_route_ms_scaled_to_the_case"] = statistics.mean(ms) * ns
        c["wall_speedup_over_mutate_route"] = statistics.mean(ms) * ns / c["pack_ms"]
        c["mutate_route_rows_identical"] = ok
        all_ok = all_ok and ok
    twin.close()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
