"""ksg_update_cluster against the only other route to the same state: ksg_set_cluster and one
ksg_add_pod per live pod.

A config-2 cluster (default 5,000 nodes out of a universe of 5,050: every 101st node is held
out) is filled in `--batch`-pod (1,000) batches until a batch leaves pods without a node. The
change: 50 nodes leave, the 50 held-out nodes join (their names lie between the others'), 50
survivors change capacity.

  a  ksg_update_cluster: wall ms, ksg_last_update_ms (the remap kernels, HIP events) and the
     host split of ksg_last_update_host_us (validation, device, host mirror). The context is taken
     back to the old list by the inverse update between runs (untimed).
  b  on a second context: ksg_set_cluster with the new arrays plus one ksg_add_pod per live pod on
     its renamed host, in commit order, through the Python wrappers. The pods are ingested
     beforehand; ingest is not charged to it.

Each is the median of `--runs` (20) after `--warmup` (5). `identical` is true only if the nine
state arrays and the placements of one following `--batch`-pod batch are equal after a and after
b. The compulsory bytes of the three kernels (each array once), divided by the device ms, are
reported as a fraction of the 8 TB/s HBM peak. The result goes to `--out` (profiles/update_cluster.json) and,
as one JSON line, to stdout. Needs the GPU.

    python tools/update_cluster_bench.py [--nodes 5000] [--batch 1000] [--out profiles/update_cluster.json]
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8e12  # bytes / s (DESIGN.md's rooflines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=1000)
    ap.add_argument("--max-fill", type=int, default=400000)
    ap.add_argument("--change", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--runs-b", type=int, default=None, help="runs of route b (default: --runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_cluster.json"))
    a = ap.parse_args()

    from kubernetes_amd import ingest, podstream, workload
    from kubernetes_amd.api import Quantity
    from kubernetes_amd.engine import DeviceScheduler, PodBatch
    from tools.srcsha import kernel_src_sha

    ch = a.change
    stride = (a.nodes + ch) // ch
    w = workload.build("config2", n_nodes=a.nodes + ch, n_pods=a.max_fill, pod_stream=True)
    held = set(range(stride // 2, a.nodes + ch, stride))
    assert len(held) == ch
    old_nodes = [n for i, n in enumerate(w.nodes) if i not in held]
    leave = set(range(stride // 5, len(old_nodes), len(old_nodes) // ch)[:ch])
    recap = set(range(stride // 3, len(old_nodes), len(old_nodes) // ch)[:ch]) - leave
    new_nodes = []
    for i, n in enumerate(old_nodes):
        if i in leave:
            continue
        if i in recap:
            n = copy.deepcopy(n)
            n.spec.capacity["cpu"] = Quantity.from_milli(n.spec.capacity.cpu().milli_value() + 1000)
        new_nodes.append(n)
    new_nodes += [w.nodes[i] for i in sorted(held)]
    it = ingest.Interner()
    for k in w.config.label_keys():
        it.key_id(k)
    old = ingest.ClusterView(old_nodes, w.services, it)
    new = ingest.ClusterView(new_nodes, w.services, it)
    stream = podstream.ingest_stream(old, w.stream, aff_labels=w.config.affinity_labels())
    cfg = w.config.compile(it.key_id)
    fwd, back = new.host_map(old), old.host_map(new)

    dev = DeviceScheduler(cfg, device=0)
    dev.set_cluster(old.arrays)
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
    placed = np.flatnonzero(host_of >= 0)
    new_host = fwd[0][host_of[placed]]
    fill_batch = PodBatch(stream.pods[:filled], stream.ids)

    def route_a():
        t = time.perf_counter()
        dev.update_cluster(new.arrays, fwd[0], fwd[1])
        dt = (time.perf_counter() - t) * 1e3
        return dt, dev.last_update_ms(), dev.last_update_host_us()

    devb = DeviceScheduler(cfg, device=0)

    def route_b():
        t = time.perf_counter()
        devb.set_cluster(new.arrays)
        for i, h in zip(placed, new_host):
            devb.add_pod(int(h), fill_batch, int(i))
        devb.read_requested()  # (the patches reach the device: the state is usable, as after a)
        return (time.perf_counter() - t) * 1e3

    ra = []
    for r in range(a.warmup + a.runs):
        if r:
            dev.update_cluster(old.arrays, back[0], back[1])  # untimed: back to the old list
        x = route_a()
        if r >= a.warmup:
            ra.append(x)
    nb = a.runs if a.runs_b is None else a.runs_b
    rb = []
    for r in range(a.warmup + nb):
        x = route_b()
        if r >= a.warmup:
            rb.append(x)

    def arrays(d):  # the nine state arrays (no extensions here: scalar_used is empty)
        st = dict(d.read_state())
        st["used_cpu"], st["used_mem"] = d.read_requested()
        return st

    sa, sb = arrays(dev), arrays(devb)
    diff = next((k for k in sorted(sa) if not np.array_equal(sa[k], sb[k])), None)
    nxt = PodBatch(stream.pods[filled:filled + a.batch], stream.ids)
    ga, gb = dev.batch(nxt, 777), devb.batch(nxt, 777)
    identical = diff is None and bool(np.array_equal(ga[0], gb[0])) and ga[1] == gb[1]
    dev.close()
    devb.close()

    m = statistics.median
    No, Nn, S, K = len(old.names), len(new.names), len(w.services), int(cfg.max_conflict_keys)
    nwo, nwn = (No + 63) // 64, (Nn + 63) // 64
    # compulsory bytes: every old row read and every new row written once (used_cpu, used_mem,
    # svc_cnt, keymap, svc_bits), the new svc_cnt rows read again by the svc kernel, its S-word
    # tables, and src once per gather launch (the waves' repeated reads of src hit the caches)
    byts = (2 * 8 * (No + Nn) + S * 4 * (No + Nn) + (K + S) * 8 * (nwo + nwn)
            + S * (Nn * 4 + 5 * 4) + 6 * 4 * Nn)
    kms = m([x[1] for x in ra])
    wall_a, wall_b = m([x[0] for x in ra]), m(rb)
    res = {
        "workload": "config2", "nodes_old": No, "nodes_new": Nn, "left": len(leave), "joined": ch,
        "capacity_changed": len(recap), "pods_filled": int(filled), "live_pods": int(len(placed)),
        "services": S, "conflict_keys": K, "warmup": a.warmup, "runs": a.runs, "runs_b": nb,
        "kernel_src_sha": kernel_src_sha(),
        "a_update_cluster_ms": wall_a, "a_kernel_ms": kms,
        "a_validate_ms": m([x[2]["validate"] for x in ra]) / 1e3, "a_device_ms": m([x[2]["device"] for x in ra]) / 1e3,
        "a_mirror_ms": m([x[2]["mirror"] for x in ra]) / 1e3, "a_abi_calls": 1,
        "b_set_cluster_add_pods_ms": wall_b, "b_abi_calls": int(len(placed)) + 1,
        "wall_ratio_b_over_a": wall_b / wall_a, "identical": identical, "first_difference": diff,
        "kernel_bytes": int(byts), "kernel_gbps": byts / (kms * 1e-3) / 1e9 if kms > 0 else None,
        "kernel_frac_of_hbm_peak": byts / (kms * 1e-3) / HBM_PEAK if kms > 0 else None,
        "spread_a_ms": [min(x[0] for x in ra), max(x[0] for x in ra)], "spread_b_ms": [min(rb), max(rb)],
        "spread_a_kernel_ms": [min(x[1] for x in ra), max(x[1] for x in ra)],
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return 0 if identical and wall_a < wall_b else 1


if __name__ == "__main__":
    sys.exit(main())
