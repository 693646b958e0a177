"""ksg_headroom_batch against its floor and against the only route without it.

Per workload (configs 2 and 4, default 5,000 nodes) the cluster is filled with `--fill` pods
(default 2 per node, bench.py's shape) and the next `--pods` (1,000) pods of the stream are the
templates asked about, with `--limit` (64) copies per node at most:

  headroom_counts_ms    wall time of one ksg_headroom_batch with the per-node counts
  headroom_nocounts_ms  ... with counts == NULL (totals, maxima, histograms, error flags only)
  explain_nocodes_ms    one ksg_explain_batch(codes == NULL) over the same pods and state: it
                        reads the same node state and divides nothing, so it is the floor
  kernel_*_ms           device time of a call's kernel launches (HIP events,
                        ksg_last_headroom_ms / ksg_last_explain_ms)
  loop_ms_per_pod       the route of the library without the call, on `--loop-pods` (3) of the
                        pods that fit somewhere: rounds of ksg_evaluate plus one ksg_add_pod per node that still
                        fits, until nothing fits or `--limit` rounds, then one ksg_remove_pod per
                        copy (driven through ctypes, as every call here); loop_ms_scaled is that
                        per pod times `--pods`
  div                   the same call under each variant of the 64-bit quotient
                        (KSG_HEADROOM_DIV 0 compiler expansion, 1 f64 reciprocal and correction,
                        2 a 32-bit divide where both operands fit, else 1), one context each on
                        the same state, the variants alternating inside every timed round; also
                        at `--div-limit` (2^20), which no count reaches, so that no quotient is
                        cut short by the limit (kernel_nocounts_div_limit_ms)

each the median of `--runs` (20) after `--warmup` (5), host clock around calls that end in a
stream synchronise. The result goes to `--out` (profiles/headroom_batch.json) and, as one
JSON line, to stdout. Needs the GPU: there is no other implementation to fall back on.

    python tools/headroom_bench.py [--nodes 5000] [--pods 1000] [--out profiles/headroom_batch.json]
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

DIV_NAMES = {0: "compiler", 1: "reciprocal", 2: "narrow_or_reciprocal"}


def run_workload(name: str, a) -> dict:
    from kubernetes_amd import abi, ingest, podstream, workload
    from kubernetes_amd.engine import DeviceScheduler, PodBatch

    n, N = a.pods, a.nodes
    fill = a.fill if a.fill else 2 * N
    w = workload.build(name, n_nodes=N, n_pods=fill + n, pod_stream=True)
    it = ingest.Interner()
    for k in w.config.label_keys():
        it.key_id(k)
    view = ingest.ClusterView(w.nodes, w.services, it)
    stream = podstream.ingest_stream(view, w.stream, aff_labels=w.config.affinity_labels())
    cfg = w.config.compile(it.key_id)
    pods = np.ascontiguousarray(stream.pods[fill:fill + n], dtype=abi.POD_DTYPE)
    ids = np.ascontiguousarray(stream.ids, dtype=np.uint32)

    devs = {}
    for div in DIV_NAMES:  # one context per quotient variant, the same fill on each
        os.environ["KSG_HEADROOM_DIV"] = str(div)
        d = DeviceScheduler(cfg, device=0)
        d.set_cluster(view.arrays)
        placed, _ = d.batch(PodBatch(stream.pods[:fill], stream.ids), workload.TIEBREAK_SEED)
        devs[div] = d
    os.environ.pop("KSG_HEADROOM_DIV", None)
    lib = devs[1]._lib
    out = {div: dict(total=np.zeros(n, np.uint64), fit=np.zeros(n, np.uint32), mx=np.zeros(n, np.uint32),
                     hist=np.zeros((n, abi.HEADROOM_SLOTS), np.uint32), counts=np.zeros((n, N), np.uint32),
                     err=np.zeros(n, np.uint8)) for div in DIV_NAMES}
    nocounts = dict(total=np.zeros(n, np.uint64), fit=np.zeros(n, np.uint32), mx=np.zeros(n, np.uint32),
                    hist=np.zeros((n, abi.HEADROOM_SLOTS), np.uint32), err=np.zeros(n, np.uint8))
    wide = {div: {k: v.copy() for k, v in nocounts.items()} for div in DIV_NAMES}  # (the --div-limit legs')
    xhist, xerr = np.zeros((n, abi.EXPLAIN_SLOTS), np.uint32), np.zeros(n, np.uint8)
    kms = C.c_double(0)

    def headroom(div: int, with_counts: bool, limit: int = a.limit):
        o, ctx = (out[div] if with_counts else nocounts if limit == a.limit else wide[div]), devs[div]._ctx
        t = time.perf_counter()
        rc = lib.ksg_headroom_batch(ctx, abi.ptr(pods), None, n, abi.ptr(ids), len(ids), limit, abi.ptr(o["total"]),
                                    abi.ptr(o["fit"]), abi.ptr(o["mx"]), abi.ptr(o["hist"]),
                                    abi.ptr(o["counts"]) if with_counts else None, abi.ptr(o["err"]))
        dt = time.perf_counter() - t
        if rc != abi.KSG_OK:
            raise SystemExit(f"ksg_headroom_batch: {rc} {lib.ksg_last_error(ctx)}")
        lib.ksg_last_headroom_ms(ctx, C.byref(kms))
        return dt * 1e3, kms.value

    def explain():
        ctx = devs[1]._ctx
        t = time.perf_counter()
        rc = lib.ksg_explain_batch(ctx, abi.ptr(pods), None, n, abi.ptr(ids), len(ids), None, abi.ptr(xhist), abi.ptr(xerr))
        dt = time.perf_counter() - t
        if rc != abi.KSG_OK:
            raise SystemExit(f"ksg_explain_batch: {rc} {lib.ksg_last_error(ctx)}")
        lib.ksg_last_explain_ms(ctx, C.byref(kms))
        return dt * 1e3, kms.value

    # the legs alternate inside every round, so that drift of the shared host lands on all alike
    legs = {("counts", d): (lambda d=d: headroom(d, True)) for d in DIV_NAMES}
    legs.update({("nocounts", d): (lambda d=d: headroom(d, False)) for d in DIV_NAMES})
    legs.update({("nocounts_div_limit", d): (lambda d=d: headroom(d, False, a.div_limit)) for d in DIV_NAMES})
    legs[("explain", 1)] = explain
    samples = {k: [] for k in legs}
    for r in range(a.warmup + a.runs):
        for k, fn in legs.items():
            s = fn()
            if r >= a.warmup:
                samples[k].append(s)
    m = statistics.median
    wall = {k: m([s[0] for s in v]) for k, v in samples.items()}
    kern = {k: m([s[1] for s in v]) for k, v in samples.items()}
    spread = {k: [min(s[0] for s in v), max(s[0] for s in v)] for k, v in samples.items()}
    same = all(all(np.array_equal(out[1][f], out[d][f]) for f in out[1]) for d in DIV_NAMES)
    same = same and all(np.array_equal(out[1][f], nocounts[f]) for f in nocounts)
    same = same and all(all(np.array_equal(wide[1][f], wide[d][f]) for f in wide[1]) for d in DIV_NAMES)
    same = same and bool(np.array_equal(out[1]["fit"], xhist[:, 0]) and np.array_equal(wide[1]["fit"], xhist[:, 0]))

    # the route without the call, on a handful of the pods (they are committed and removed again)
    ctx = devs[1]._ctx
    fails, scores = np.zeros(N, np.uint8), np.zeros(N, np.int64)
    loop_ms, loop_same, uid = [], True, 1 << 40
    fitting = np.nonzero(out[1]["fit"] > 0)[0]  # (a pod that fits nowhere costs the loop one evaluate)
    for i in fitting[np.linspace(0, len(fitting) - 1, min(a.loop_pods, len(fitting))).astype(int)].tolist():
        pod = pods[i:i + 1].copy()
        pp = abi.ptr(pod)
        cnt, live, added = np.zeros(N, np.uint32), np.ones(N, bool), []
        t = time.perf_counter()
        for _ in range(a.limit):
            rc = lib.ksg_evaluate(ctx, pp, abi.ptr(ids), abi.ptr(fails), abi.ptr(scores))
            if rc != abi.KSG_OK:
                raise SystemExit(f"ksg_evaluate: {rc} {lib.ksg_last_error(ctx)}")
            live &= fails == 0
            nodes = np.nonzero(live)[0]
            if not len(nodes):
                break
            for node in nodes.tolist():
                pod["uid"] = uid
                if lib.ksg_add_pod(ctx, node, pp, abi.ptr(ids)) != abi.KSG_OK:
                    raise SystemExit(f"ksg_add_pod: {lib.ksg_last_error(ctx)}")
                added.append(uid)
                uid += 1
            cnt += live
        for u in added:
            if lib.ksg_remove_pod(ctx, u) != abi.KSG_OK:
                raise SystemExit(f"ksg_remove_pod: {lib.ksg_last_error(ctx)}")
        loop_ms.append((time.perf_counter() - t) * 1e3)
        loop_same = loop_same and bool(np.array_equal(cnt, out[1]["counts"][i]))
    headroom(1, True)  # (the removals restored the state: the call again, against the other context's result)
    restored = all(np.array_equal(out[1][f], out[0][f]) for f in out[1])
    for d in devs.values():
        d.close()

    o = out[1]
    per_pod = statistics.mean(loop_ms) if loop_ms else None
    return {
        "workload": name, "nodes": N, "pods_filled": int(fill), "pods_placed_by_fill": int((placed >= 0).sum()),
        "pods_asked": n, "limit": a.limit,
        "headroom_counts_ms": wall["counts", 1], "headroom_nocounts_ms": wall["nocounts", 1],
        "kernel_counts_ms": kern["counts", 1], "kernel_nocounts_ms": kern["nocounts", 1],
        "explain_nocodes_ms": wall["explain", 1], "kernel_explain_nocodes_ms": kern["explain", 1],
        "kernel_nocounts_over_explain": kern["nocounts", 1] / kern["explain", 1] if kern["explain", 1] > 0 else None,
        "copy_and_host_counts_ms": wall["counts", 1] - kern["counts", 1],
        "div": {DIV_NAMES[d]: {"kernel_counts_ms": kern["counts", d], "kernel_nocounts_ms": kern["nocounts", d],
                               "headroom_nocounts_ms": wall["nocounts", d],
                               "kernel_nocounts_div_limit_ms": kern["nocounts_div_limit", d]} for d in DIV_NAMES},
        "div_limit": a.div_limit, "max_count_div_limit": int(wide[1]["mx"].max()),
        "loop_pods": int(a.loop_pods), "loop_ms_per_pod": per_pod, "loop_ms_each": loop_ms,
        "loop_ms_scaled": per_pod * n if per_pod is not None else None,
        "loop_over_headroom_counts": per_pod * n / wall["counts", 1] if per_pod is not None else None,
        "spread_ms": {f"{k[0]}_{DIV_NAMES[k[1]]}": v for k, v in spread.items()},
        "mean_fitting_nodes": float(o["fit"].mean()), "mean_total": float(o["total"].mean()),
        "max_count": int(o["mx"].max()), "pods_with_no_node": int((o["fit"] == 0).sum()),
        "bind_hist_sum": {str(b): int(o["hist"][:, b].sum()) for b in range(abi.HEADROOM_SLOTS) if o["hist"][:, b].any()},
        "variants_identical": bool(same), "identical_to_loop": bool(loop_same), "state_restored_after_loop": bool(restored),
    }


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=1000)
    ap.add_argument("--fill", type=int, default=0, help="pods committed first (default: 2 per node)")
    ap.add_argument("--limit", type=int, default=64)
    ap.add_argument("--div-limit", type=int, default=1 << 20, help="a limit no count reaches: every quotient is formed in full")
    ap.add_argument("--loop-pods", type=int, default=3)
    ap.add_argument("--workloads", default="config2,config4")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "headroom_batch.json"))
    a = ap.parse_args()

    from tools.srcsha import kernel_src_sha

    res = {"kernel_src_sha": kernel_src_sha(), "warmup": a.warmup, "runs": a.runs,
           "results": [run_workload(w, a) for w in a.workloads.split(",")]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    ok = all(r["variants_identical"] and r["identical_to_loop"] and r["state_restored_after_loop"] for r in res["results"])
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
