"""ksg_prioritize_batch against its only alternative, a loop of ksg_evaluate calls.

For config 2 and config 4 a cluster (default 5,000 nodes) takes a fill batch (`--fill` pods);
the next `--pods` (default 1,000) pods of the stream are then ranked, on one context and in
one process, in three forms that alternate:

  top      one ksg_prioritize_batch, top = 3, scores == NULL
  scores   one ksg_prioritize_batch, top = 3, with the per-node scores
  loop     one ksg_evaluate per pod over the same pods (fail codes and scores)

After `--warmup` rounds of all three, `--runs` rounds are timed: the host clock around each
call (they end in a stream synchronise) and, for the batched forms, the device time of the
call's kernels (HIP events, ksg_last_prioritize_ms), reported apart. Each figure is given as
median and [min, max] over the rounds. The batched call passes when it beats the loop by more
than the loop's own run-to-run spread (its max - min here); no ratio is fixed in advance. The
scores of the batched call are compared with the loop's rows, bit for bit. The result goes to
`--out` (profiles/prioritize_batch.json), tagged with the source hash, and as one JSON line to
stdout. Needs the GPU: there is no other implementation to fall back on.

    python tools/prioritize_bench.py [--nodes 5000] [--pods 1000] [--out profiles/prioritize_batch.json]
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

TOP = 3


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def run(name: str, a) -> dict:
    from kubernetes_amd import abi, ingest, podstream, workload
    from kubernetes_amd.engine import DeviceScheduler, PodBatch

    w = workload.build(name, n_nodes=a.nodes, n_pods=a.fill + a.pods, pod_stream=True)
    it = ingest.Interner()
    for k in w.config.label_keys():
        it.key_id(k)
    view = ingest.ClusterView(w.nodes, w.services, it)
    stream = podstream.ingest_stream(view, w.stream, aff_labels=w.config.affinity_labels())
    dev = DeviceScheduler(w.config.compile(it.key_id), device=0)
    dev.set_cluster(view.arrays)
    lib, ctx = dev._lib, dev._ctx
    out, _ = dev.batch(PodBatch(stream.pods[:a.fill], stream.ids), workload.TIEBREAK_SEED)

    n, N = a.pods, a.nodes
    pods = np.ascontiguousarray(stream.pods[a.fill:a.fill + n], dtype=abi.POD_DTYPE)
    ids = np.ascontiguousarray(stream.ids, dtype=np.uint32)
    mx, ties, fit = np.zeros(n, np.int64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    tn, ts = np.zeros((n, TOP), np.int32), np.zeros((n, TOP), np.int64)
    err = np.zeros(n, np.uint8)
    scores = np.zeros((n, N), np.int64)
    loop_scores = np.zeros((n, N), np.int64)
    fails = np.zeros((n, N), np.uint8)
    kms = C.c_double(0)

    def prioritize(with_scores: bool):
        t = time.perf_counter()
        rc = lib.ksg_prioritize_batch(ctx, abi.ptr(pods), None, n, abi.ptr(ids), len(ids), TOP, abi.ptr(mx),
                                      abi.ptr(ties), abi.ptr(fit), abi.ptr(tn), abi.ptr(ts),
                                      abi.ptr(scores) if with_scores else None, abi.ptr(err))
        dt = time.perf_counter() - t
        if rc != abi.KSG_OK:
            raise SystemExit(f"ksg_prioritize_batch: {rc} {lib.ksg_last_error(ctx)}")
        lib.ksg_last_prioritize_ms(ctx, C.byref(kms))
        return dt * 1e3, kms.value

    def evaluate_loop():
        base, step = pods.ctypes.data, pods.dtype.itemsize
        t = time.perf_counter()
        for i in range(n):
            rc = lib.ksg_evaluate(ctx, C.c_void_p(base + i * step), abi.ptr(ids), C.c_void_p(fails.ctypes.data + i * N),
                                  C.c_void_p(loop_scores.ctypes.data + i * N * 8))
            if rc != abi.KSG_OK:
                raise SystemExit(f"ksg_evaluate: {rc} {lib.ksg_last_error(ctx)}")
        return (time.perf_counter() - t) * 1e3

    top_t, sc_t, loop_t = [], [], []
    for r in range(a.warmup + a.runs):  # the forms alternate
        x, y, z = prioritize(False), prioritize(True), evaluate_loop()
        if r >= a.warmup:
            top_t.append(x)
            sc_t.append(y)
            loop_t.append(z)
    fitm = fails == 0
    identical = bool(np.array_equal(scores, loop_scores) and np.array_equal(fit, fitm.sum(axis=1)) and not err.any())
    dev.close()

    loop = stat(loop_t)
    res = {
        "nodes": N, "pods_filled": a.fill, "pods_placed_by_fill": int((out >= 0).sum()), "pods_ranked": n, "top": TOP,
        "top_wall_ms": stat([x[0] for x in top_t]), "top_device_ms": stat([x[1] for x in top_t]),
        "scores_wall_ms": stat([x[0] for x in sc_t]), "scores_device_ms": stat([x[1] for x in sc_t]),
        "evaluate_loop_wall_ms": loop,
        "loop_spread_ms": loop["max"] - loop["min"],
        "identical_to_evaluate_loop": identical,
        "mean_fitting_nodes": float(fit.mean()), "pods_with_no_node": int((fit == 0).sum()),
        "mean_ties": float(ties.mean()),
    }
    for form in ("top", "scores"):
        m = res[form + "_wall_ms"]["median"]
        res[form + "_speedup"] = loop["median"] / m
        res[form + "_passes"] = bool(loop["median"] - m > res["loop_spread_ms"])
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=1000)
    ap.add_argument("--fill", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--workloads", default="config2,config4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prioritize_batch.json"))
    a = ap.parse_args()

    from tools.srcsha import kernel_src_sha

    res = {"kernel_src_sha": kernel_src_sha(), "warmup": a.warmup, "runs": a.runs,
           "method": "forms alternate per round; host clock around each call, device ms from HIP events apart"}
    for name in a.workloads.split(","):
        res[name] = run(name, a)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    ok = all(res[k]["identical_to_evaluate_loop"] and res[k]["top_passes"] and res[k]["scores_passes"]
             for k in a.workloads.split(","))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
