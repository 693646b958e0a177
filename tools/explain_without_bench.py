"""ksg_explain_without against ksg_explain_batch (its floor) and against the only other route
to the same rows, the batch run pod by pod through ksg_schedule_begin(fail_codes) /
ksg_schedule_commit.

A config-2 cluster (default 5,000 nodes) is filled in `--batch`-pod (1,000) batches until a
batch leaves pods without a node; the next batch that both places pods and leaves pods
unplaced is the measured one. Over its NOFIT pods:

  a  ksg_explain_batch                         (the state after the batch: the parent's kernel)
  b  ksg_explain_without, n_absent = 0         (the same rows through the new kernel)
  c  ksg_explain_without, the batch's placed pods listed, first_absent = placed before the pod
  d  the whole batch pod by pod: ksg_schedule_begin(fail_codes) / ksg_schedule_commit from the
     state before the batch (the placed pods are removed again, untimed, after every run)
  e  the host time c spends building and uploading its tables. It is not timed inside the
     library: it is DERIVED as (wall_c - kernel_c) - (wall_b - kernel_b), the host-and-copy time
     of c beyond that of b, whose tables are empty but for the per-node offsets.

Wall ms (host clock around calls that end in a stream synchronise) and kernel ms (HIP events,
ksg_last_explain_ms / ksg_last_explain_without_ms), each the median of `--runs` (20) after
`--warmup` (5). c's rows must equal d's, and b's must equal a's. The result goes to `--out`
(profiles/explain_without.json) and, as one JSON line, to stdout. Needs the GPU.

    python tools/explain_without_bench.py [--nodes 5000] [--batch 1000] [--out profiles/explain_without.json]
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--max-fill", type=int, default=400000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain_without.json"))
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

    def seq_run(pods, seed, fails):
        """d: the batch pod by pod; -> (wall ms, placements). fails[i] = pod i's codes (NOFIT rows are read)."""
        rng = workload._SM(seed)
        out = np.full(len(pods), -1, np.int32)
        base, step = pods.ctypes.data, pods.dtype.itemsize
        m, k, node = C.c_int64(0), C.c_uint32(0), C.c_int32(-1)
        t = time.perf_counter()
        for i in range(len(pods)):
            rc = lib.ksg_schedule_begin(ctx, C.c_void_p(base + i * step), abi.ptr(ids), C.byref(m), C.byref(k),
                                        C.c_void_p(fails.ctypes.data + i * N))
            if rc == abi.KSG_OK:
                if lib.ksg_schedule_commit(ctx, (rng.next() >> 1) % k.value, C.byref(node)) != abi.KSG_OK:
                    raise SystemExit(f"ksg_schedule_commit: {lib.ksg_last_error(ctx)}")
                out[i] = node.value
            elif rc != abi.KSG_NOFIT:
                raise SystemExit(f"ksg_schedule_begin: {rc} {lib.ksg_last_error(ctx)}")
        return (time.perf_counter() - t) * 1e3, out

    # fill until a batch leaves pods unplaced, then take the next batch with both kinds of pod
    state, filled, full = workload.TIEBREAK_SEED, 0, False
    while True:
        if filled + a.batch > len(stream):
            raise SystemExit(f"no mixed batch after {filled} pods: raise --max-fill")
        pods = np.ascontiguousarray(stream.pods[filled:filled + a.batch], dtype=abi.POD_DTYPE)
        if full:
            fails = np.zeros((len(pods), N), np.uint8)
            _, probe_out = seq_run(pods, state, fails)
            for u in pods["uid"][probe_out >= 0]:
                dev.remove_pod(int(u))
            if (probe_out >= 0).any() and (probe_out < 0).any():
                break
        out, state = dev.batch(PodBatch(pods, stream.ids), state)
        full = full or bool((out < 0).any())
        filled += len(pods)

    def med(fn):
        for _ in range(a.warmup):
            fn()
        return [fn() for _ in range(a.runs)]

    def timed_seq():
        ms, o = seq_run(pods, state, fails)
        for u in pods["uid"][o >= 0]:  # (untimed: back to the state before the batch)
            dev.remove_pod(int(u))
        return ms

    seq = med(timed_seq)
    seq_rows = fails[probe_out < 0].copy()
    out, _ = dev.batch(PodBatch(pods, stream.ids), state)
    same_placements = bool(np.array_equal(out, probe_out))
    nofit = np.ascontiguousarray(pods[out < 0])
    n = len(nofit)
    placed = np.ascontiguousarray(pods["uid"][out >= 0], dtype=np.uint64)
    before = np.concatenate([[0], np.cumsum(out >= 0)])[np.nonzero(out < 0)[0]].astype(np.uint32)
    bufs = {x: (np.zeros((n, N), np.uint8), np.zeros((n, abi.EXPLAIN_SLOTS), np.uint32), np.zeros(n, np.uint8))
            for x in "abc"}
    kms = C.c_double(0)

    def explain(which):
        codes, hist, err = bufs[which]
        t = time.perf_counter()
        if which == "a":
            rc = lib.ksg_explain_batch(ctx, abi.ptr(nofit), None, n, abi.ptr(ids), len(ids), abi.ptr(codes), abi.ptr(hist),
                                       abi.ptr(err))
        elif which == "b":
            rc = lib.ksg_explain_without(ctx, abi.ptr(nofit), None, n, abi.ptr(ids), len(ids), None, 0, None,
                                         abi.ptr(codes), abi.ptr(hist), abi.ptr(err))
        else:
            rc = lib.ksg_explain_without(ctx, abi.ptr(nofit), None, n, abi.ptr(ids), len(ids), abi.ptr(placed), len(placed),
                                         abi.ptr(before), abi.ptr(codes), abi.ptr(hist), abi.ptr(err))
        dt = time.perf_counter() - t
        if rc != abi.KSG_OK:
            raise SystemExit(f"explain {which}: {rc} {lib.ksg_last_error(ctx)}")
        (lib.ksg_last_explain_ms if which == "a" else lib.ksg_last_explain_without_ms)(ctx, C.byref(kms))
        return dt * 1e3, kms.value

    # alternate the three forms run by run, so that drift on a shared host hits them alike
    for _ in range(a.warmup):
        for x in "abc":
            explain(x)
    runs = {x: [] for x in "abc"}
    for _ in range(a.runs):
        for x in "abc":
            runs[x].append(explain(x))
    dev.close()

    m = statistics.median
    wall = {x: m([r[0] for r in runs[x]]) for x in "abc"}
    kern = {x: m([r[1] for r in runs[x]]) for x in "abc"}
    b_is_a = all(np.array_equal(p, q) for p, q in zip(bufs["a"], bufs["b"]))
    c_is_seq = bool(np.array_equal(bufs["c"][0], seq_rows) and not bufs["c"][2].any())
    differing = int((bufs["c"][0] != bufs["a"][0]).any(axis=1).sum())
    t_seq = m(seq)
    res = {
        "workload": "config2", "nodes": N, "pods_filled": int(filled), "batch": len(pods), "batch_placed": int(len(placed)),
        "batch_nofit": n, "nofit_pods_whose_map_differs_from_after_batch": differing,
        "warmup": a.warmup, "runs": a.runs, "kernel_src_sha": kernel_src_sha(),
        "a_explain_batch_ms": wall["a"], "a_kernel_ms": kern["a"],
        "b_without_empty_ms": wall["b"], "b_kernel_ms": kern["b"],
        "c_without_listed_ms": wall["c"], "c_kernel_ms": kern["c"],
        "d_begin_commit_loop_ms": t_seq,
        "e_tables_build_upload_ms_derived": (wall["c"] - kern["c"]) - (wall["b"] - kern["b"]),
        "kernel_ratio_b_over_a": kern["b"] / kern["a"] if kern["a"] > 0 else None,
        "kernel_ratio_c_over_a": kern["c"] / kern["a"] if kern["a"] > 0 else None,
        "wall_speedup_c_over_d": t_seq / wall["c"],
        "b_identical_to_a": bool(b_is_a), "c_identical_to_begin_commit_rows": c_is_seq,
        "batch_placements_identical_to_begin_commit": same_placements,
        "spread_ms": {x: [min(r[0] for r in runs[x]), max(r[0] for r in runs[x])] for x in "abc"} | {"d": [min(seq), max(seq)]},
        "spread_kernel_ms": {x: [min(r[1] for r in runs[x]), max(r[1] for r in runs[x])] for x in "abc"},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return 0 if b_is_a and c_is_seq and same_placements else 1


if __name__ == "__main__":
    sys.exit(main())
