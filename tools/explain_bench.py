"""ksg_explain_batch against its only alternative, a loop of ksg_evaluate calls.

A config-2 cluster (default 5,000 nodes) is filled batch by batch until pods start to find
no node; the first `--pods` (default 1,000) pods that found none are then explained:

  explain_codes_ms    wall time of one ksg_explain_batch with the per-node codes
  explain_nocodes_ms  ... with codes == NULL (histograms and error flags only)
  evaluate_loop_ms    wall time of one ksg_evaluate per pod over the same pods
  kernel_*_ms         device time of the call's kernel launches (HIP events, ksg_last_explain_ms)

each the median of `--runs` (20) after `--warmup` (5), host clock around calls that end in a
stream synchronise. The byte model of the kernel is n x N output bytes (with codes) plus the
node state (4 x int64 per node) once per (node tile, pod chunk), plus the histograms; the
achieved rate is that over the kernel time, against the HBM peak. The result goes to `--out`
(profiles/explain_batch.json) and, as one JSON line, to stdout. Needs the GPU: there is no
other implementation to fall back on.

    python tools/explain_bench.py [--nodes 5000] [--pods 1000] [--out profiles/explain_batch.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, as bench.py


def kernel_tiling():
    """(nodes per workgroup, pods per workgroup) of ksg_explain_kernel, from ksg_internal.h."""
    src = open(os.path.join(ROOT, "kubernetes_amd", "csrc", "ksg_internal.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in ("KSG_EXPLAIN_TILE", "KSG_EXPLAIN_CHUNK"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--pods", type=int, default=1000)
    ap.add_argument("--fill-batch", type=int, default=5000)
    ap.add_argument("--max-fill", type=int, default=400000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_batch.json"))
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

    # fill until `pods` pods have found no node
    rng, unplaced, filled = workload.TIEBREAK_SEED, [], 0
    while sum(len(u) for u in unplaced) < a.pods and filled < len(stream):
        sub = PodBatch(stream.pods[filled:filled + a.fill_batch], stream.ids)
        out, rng = dev.batch(sub, rng)
        unplaced.append(filled + np.nonzero(out == abi.KSG_OUT_NOFIT)[0])
        filled += len(sub)
    idx = np.concatenate(unplaced)[:a.pods]
    if len(idx) < a.pods:
        raise SystemExit(f"only {len(idx)} pods found no node after {filled} pods: raise --max-fill")
    n, N = len(idx), a.nodes
    pods = np.ascontiguousarray(stream.pods[idx], dtype=abi.POD_DTYPE)
    ids = np.ascontiguousarray(stream.ids, dtype=np.uint32)
    codes = np.zeros((n, N), np.uint8)
    hist = np.zeros((n, abi.EXPLAIN_SLOTS), np.uint32)
    hist2 = np.zeros_like(hist)
    err = np.zeros(n, np.uint8)
    fails = np.zeros((n, N), np.uint8)
    scores = np.zeros(N, np.int64)
    kms = C.c_double(0)

    def explain(with_codes: bool):
        t = time.perf_counter()
        rc = lib.ksg_explain_batch(ctx, abi.ptr(pods), None, n, abi.ptr(ids), len(ids),
                                   abi.ptr(codes) if with_codes else None, abi.ptr(hist if with_codes else hist2),
                                   abi.ptr(err))
        dt = time.perf_counter() - t
        if rc != abi.KSG_OK:
            raise SystemExit(f"ksg_explain_batch: {rc} {lib.ksg_last_error(ctx)}")
        lib.ksg_last_explain_ms(ctx, C.byref(kms))
        return dt * 1e3, kms.value

    def evaluate_loop():
        base, step = pods.ctypes.data, pods.dtype.itemsize
        t = time.perf_counter()
        for i in range(n):
            rc = lib.ksg_evaluate(ctx, C.c_void_p(base + i * step), abi.ptr(ids), C.c_void_p(fails.ctypes.data + i * N),
                                  abi.ptr(scores))
            if rc != abi.KSG_OK:
                raise SystemExit(f"ksg_evaluate: {rc} {lib.ksg_last_error(ctx)}")
        return (time.perf_counter() - t) * 1e3

    def med(fn):
        for _ in range(a.warmup):
            fn()
        return [fn() for _ in range(a.runs)]

    with_codes = med(lambda: explain(True))
    no_codes = med(lambda: explain(False))
    loop = med(evaluate_loop)
    identical = bool(np.array_equal(codes, fails) and np.array_equal(hist, hist2) and not err.any())
    dev.close()

    tile, chunk = kernel_tiling()
    state = -(-N // tile) * -(-n // chunk) * tile * 32
    model_codes = n * N + state + n * abi.EXPLAIN_SLOTS * 4
    model_nocodes = state + n * abi.EXPLAIN_SLOTS * 4
    m = statistics.median
    t_codes, k_codes = m([x[0] for x in with_codes]), m([x[1] for x in with_codes])
    t_nocodes, k_nocodes = m([x[0] for x in no_codes]), m([x[1] for x in no_codes])
    t_loop = m(loop)
    res = {
        "workload": "config2", "nodes": N, "pods_filled": int(filled), "pods_explained": n,
        "warmup": a.warmup, "runs": a.runs, "kernel_src_sha": kernel_src_sha(),
        "explain_codes_ms": t_codes, "explain_nocodes_ms": t_nocodes, "evaluate_loop_ms": t_loop,
        "speedup_codes": t_loop / t_codes, "speedup_nocodes": t_loop / t_nocodes,
        "kernel_codes_ms": k_codes, "kernel_nocodes_ms": k_nocodes,
        "copy_and_host_ms": t_codes - k_codes,
        "model_bytes_codes": model_codes, "model_bytes_nocodes": model_nocodes,
        "achieved_GBps_codes": model_codes / (k_codes * 1e-3) / 1e9 if k_codes > 0 else None,
        "hbm_peak_GBps": HBM_PEAK / 1e9,
        "frac_of_hbm_peak_codes": model_codes / (k_codes * 1e-3) / HBM_PEAK if k_codes > 0 else None,
        "mean_fitting_nodes": float(hist[:, 0].mean()), "pods_with_no_node": int((hist[:, 0] == 0).sum()),
        "identical_to_evaluate_loop": identical,
        "spread_ms": {"explain_codes": [min(x[0] for x in with_codes), max(x[0] for x in with_codes)],
                      "evaluate_loop": [min(loop), max(loop)]},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return 0 if identical and t_codes < t_loop else 1


if __name__ == "__main__":
    sys.exit(main())
