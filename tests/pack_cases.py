"""Inputs and the reference of the ksg_pack_batch tests (tests/test_pack_inputs.py on the CPU,
tests/test_gpu_pack.py on the device).

A scenario is an engine state (`load`), probe pods grouped into sets (`sizes`), per set an
excluded node or NO_NODE (`exclude`, or None) and a target mask (`targets`, uint64 words, or None).

The reference (`reference`) is the header's definition executed literally on any engine with
add_pod / remove_pod / evaluate, the C restatement or a device context: per set and pod, evaluate
for the codes, take the highest-rank node with code 0 that is neither excluded nor masked, add_pod
the pod there under a fresh uid; after the set, remove_pod all of them. The engine is left in the
scenario's loaded state.

Random scenarios: tests/explain_cases.py's clusters (xcase(policy, nn) for config2, presence and
hosts; xext(nn) for the extensions) after their fill. From 128 nodes on they are made fuller by
blocker pods on most of the top ranks (added with add_pod, which checks no predicate), so that a
set fills the few open nodes of the first strip, piles onto nodes it has touched and spills below;
below 128 nodes the fill leaves no room at all, and every other pod it placed is removed again. A
few probe pods are made larger than any node. The probe pods are drawn
from the case's probe and fill pods and grouped into sets of sizes 0, 1 and 8 to 16; every third
set excludes the node that the first of its pods to fit somewhere would take as things stand; the `mask` variant clears the
bits of the nodes every third pod would take, and of every eleventh node.

The handmade scenarios (HANDMADE) each name what they show; `want` writes their rows out.

Everything is built once and shared by the tests (read-only)."""
from __future__ import annotations

import functools
import os
import re

import numpy as np

from kubernetes_amd import abi, ingest, workload
from kubernetes_amd.api import (GCEPersistentDiskVolumeSource, ObjectMeta, Pod, PodSpec, PodStatus, Volume, make_node,
                                resource_container)
from kubernetes_amd.engine import PodBatch
from tests import explain_cases as X
from tests import without_cases as W

NOFIT = abi.KSG_OUT_NOFIT
NO_NODE = abi.PACK_NO_NODE
MAX_SET = abi.PACK_MAX_SET
FRESH_UID = 5 * 10 ** 6  # the reference's uids for the pods it adds


def kernel_strip() -> int:
    """Nodes per strip of ksg_pack_kernel's scan (one per lane), from ksg_internal.h."""
    src = open(os.path.join(X.ROOT, "kubernetes_amd", "csrc", "ksg_internal.h")).read()
    return int(re.search(r"#define KSG_PACK_STRIP (\d+)", src).group(1))


STRIP = kernel_strip()


def first_strip_lo(nn: int) -> int:
    """The lowest rank of the scan's first strip: it holds the top STRIP / 64 bitmap words, the
    last, possibly partial, word included (ksg_pack.hip's header)."""
    nw = (nn + 63) // 64
    return 64 * max(nw - STRIP // 64, 0)


# (policy or "ext" / "ext-null", node count, variant) of the random scenarios; ServiceAffinity
# configurations (config4) are refused. Both sides of a 64-node word and of a strip, three strips,
# and 1000 nodes once.
RANDOM = (("config2", 63, ""), ("presence", 64, ""), ("hosts", 65, ""), ("config2", STRIP - 1, ""),
          ("presence", STRIP, ""), ("config2", STRIP + 1, ""), ("hosts", 2 * STRIP + 1, ""),
          ("config2", 2 * STRIP + 1, "mask"), ("ext", STRIP + 1, ""), ("ext-null", 65, ""), ("config2", 1000, ""))
SET_SIZES = (0, 1, 8, 12, 1, 16, 0, 9, 3, 10, 1, 14)


class Scenario:
    def __init__(self, name, cfg, load, probe: PodBatch, sizes, exclude, targets, n_nodes: int):
        self.name, self.cfg, self.load, self.probe, self.nn = name, cfg, load, probe, n_nodes
        self.sizes = np.asarray(sizes, np.uint32)
        self.exclude = None if exclude is None else np.asarray(exclude, np.uint32)
        self.targets = None if targets is None else np.asarray(targets, np.uint64)
        assert int(self.sizes.sum()) == len(probe) and (self.sizes <= MAX_SET).all()
        for a in (self.sizes, self.exclude, self.targets):
            if a is not None:
                a.setflags(write=False)

    def open_nodes(self, s: int) -> np.ndarray:
        """bool[N]: the nodes set s may use at all."""
        ok = np.ones(self.nn, bool)
        if self.targets is not None:
            n = np.arange(self.nn)
            ok &= ((self.targets[n >> 6] >> (n & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
        if self.exclude is not None and self.exclude[s] != NO_NODE:
            ok[int(self.exclude[s])] = False
        return ok


class Result:
    """out_nodes and placed as ksg_pack_batch returns them, plus what the reference saw on the way."""

    def __init__(self, sc, out, raw_best, base_best):
        self.out = np.asarray(out, np.int32)
        self.raw_best = np.asarray(raw_best, np.int32)    # the highest node with code 0 as the pod saw the state
        self.base_best = np.asarray(base_best, np.int32)  # ... and as the state stands, among the set's open nodes
        off = np.concatenate([[0], np.cumsum(sc.sizes)]).astype(np.int64)
        self.off = off
        self.placed = np.array([(self.out[off[s]: off[s + 1]] >= 0).sum() for s in range(len(sc.sizes))], np.uint32)
        self.sizes, self.lo = sc.sizes, first_strip_lo(sc.nn)
        for a in (self.out, self.raw_best, self.base_best, self.placed):
            a.setflags(write=False)

    def kinds(self):
        """(sets of at least one pod placed whole, sets with an unplaced pod, pods on a node an
        earlier pod of their set took, pods whose node is not the one the state as it stands would
        give them, pods whose highest fitting node was the excluded or a masked one, pods that end
        below the scan's first strip)"""
        full = int(((self.placed == self.sizes) & (self.sizes > 0)).sum())
        short = int((self.placed < self.sizes).sum())
        again = 0
        for s in range(len(self.sizes)):
            seen = set()
            for o in self.out[self.off[s]: self.off[s + 1]]:
                if o >= 0:
                    again += int(o) in seen
                    seen.add(int(o))
        moved = int(((self.base_best >= 0) & (self.out != self.base_best)).sum())
        barred = int(((self.raw_best >= 0) & (self.out != self.raw_best)).sum())
        below = int(((self.out >= 0) & (self.out < self.lo)).sum())
        return full, short, again, moved, barred, below


def _codes(eng, probe, i):
    err, codes = W._evaluate(eng, probe, i)
    assert not err
    return np.asarray(codes)


def reference(sc: Scenario, eng) -> Result:
    """The definition on `eng` (a fresh engine; left in the scenario's loaded state)."""
    sc.load(eng)
    n = len(sc.probe)
    out, raw = np.full(n, NOFIT, np.int32), np.full(n, -1, np.int32)
    base = np.full(n, -1, np.int32)
    uid, at = FRESH_UID, 0
    for s, m in enumerate(sc.sizes.tolist()):
        ok = sc.open_nodes(s)
        for i in range(at, at + m):
            f = np.flatnonzero((_codes(eng, sc.probe, i) == 0) & ok)
            base[i] = f[-1] if len(f) else -1
        added = []
        for i in range(at, at + m):
            fit = _codes(eng, sc.probe, i) == 0
            raw[i] = np.flatnonzero(fit)[-1] if fit.any() else -1
            f = np.flatnonzero(fit & ok)
            if not len(f):
                continue
            out[i] = f[-1]
            one = sc.probe.one(i)
            one.pods["uid"] = uid
            eng.add_pod(int(f[-1]), one, 0)
            added.append(uid)
            uid += 1
        for u in added:
            eng.remove_pod(u)
        at += m
    return Result(sc, out, raw, base)


_REF = {}


def oracle_reference(sc: Scenario) -> Result:
    """`reference` on the C restatement, computed once per scenario."""
    if sc.name not in _REF:
        from oracle.pyoracle import OracleScheduler

        orc = OracleScheduler(sc.cfg)
        try:
            _REF[sc.name] = reference(sc, orc)
        finally:
            orc.close()
    return _REF[sc.name]


# ---- random scenarios ------------------------------------------------------------------------
N_BLOCK_UID = 800000


def _block_ranks(nn: int) -> np.ndarray:
    """The ranks the blockers fill: from a little below the first strip up (at least the top two
    thirds of a cluster of up to a strip), all but every eighth node."""
    if nn < 128:  # (the fill alone leaves a small cluster tight)
        return np.zeros(0, np.int64)
    lo = min(max(first_strip_lo(nn) - 40, 0), nn // 3)
    r = np.arange(lo, nn)
    return r[r % 8 != 0]


@functools.lru_cache(maxsize=None)
def random_scenario(policy: str, nn: int, variant: str = "") -> Scenario:
    from oracle.pyoracle import OracleScheduler

    ext = policy in ("ext", "ext-null")
    case = X.xext(nn) if ext else X.xcase(policy, nn)
    fe = case.fill.ext if ext else None
    pe = case.probe.ext if ext else None
    pool = np.concatenate([case.probe.pods, case.fill.pods[:67]])
    pool_ext = np.concatenate([pe, fe[:67]]) if ext else None
    rng = workload._SM(131 * nn + len(policy) + 7 * len(variant))
    idx = [rng.below(len(pool)) for _ in range(sum(SET_SIZES))]
    probe = PodBatch(pool[idx].copy(), case.probe.ids, pool_ext[idx].copy() if policy == "ext" else None)
    probe.pods["milli_cpu"][6::13] *= 40  # (a few pods no node can take: the set goes on without them)
    ranks = _block_ranks(nn)
    thin = nn < 128 and not ext
    blockers = PodBatch(np.repeat(case.fill.pods[:1], len(ranks)), case.fill.ids,
                        np.zeros(len(ranks), abi.POD_EXT_DTYPE) if ext else None)
    for f in ("n_ports", "n_pds", "n_sel", "n_svcs"):
        blockers.pods[f] = 0
    blockers.pods["service"], blockers.pods["host"], blockers.pods["milli_cpu"] = -1, -1, 10 ** 9
    blockers.pods["uid"] = N_BLOCK_UID + np.arange(len(ranks))

    def load(eng):
        out, _ = case.load(eng)
        if thin:  # (the fill leaves a small cluster with no room at all: every other placed pod goes again)
            for u in case.fill.pods["uid"][out[: len(case.fill)] >= 0][::2]:
                eng.remove_pod(int(u))
        for j, r in enumerate(ranks):
            eng.add_pod(int(r), blockers, j)

    # the nodes the pods would take as things stand decide what is excluded and masked
    orc = OracleScheduler(case.cfg)
    try:
        load(orc)
        best = []
        for i in range(len(probe)):
            f = np.flatnonzero(_codes(orc, probe, i) == 0)
            best.append(int(f[-1]) if len(f) else -1)
    finally:
        orc.close()
    off = np.concatenate([[0], np.cumsum(SET_SIZES)])
    exclude = [NO_NODE] * len(SET_SIZES)
    for s in range(2, len(SET_SIZES), 3):
        took = [b for b in best[off[s]: off[s + 1]] if b >= 0]  # (the set's first pod that fits somewhere)
        if took:
            exclude[s] = took[0]
    targets = None
    if variant == "mask":
        targets = np.full((nn + 63) // 64, ~np.uint64(0), np.uint64)
        for r in [b for b in best[::3] if b >= 0] + list(range(5, nn, 11)):
            targets[r >> 6] &= ~(np.uint64(1) << np.uint64(r & 63))
    name = f"random-{policy}-{nn}" + (f"-{variant}" if variant else "")
    return Scenario(name, case.cfg, load, probe, SET_SIZES, exclude, targets, nn)


# ---- handmade scenarios ----------------------------------------------------------------------
MI = 1 << 20
GI = 1 << 30
HUGE = (1 << 63) - 100


def _p(name, host="", cpu=0, mem=0, ports=(), pd=None):
    vols = [Volume(name="data", gce_persistent_disk=GCEPersistentDiskVolumeSource(pd_name=pd))] if pd else []
    return Pod(metadata=ObjectMeta(name=name, namespace="ns"),
               spec=PodSpec(containers=[resource_container(cpu, mem, ports)], volumes=vols),
               status=PodStatus(host=host))


def _made(name, nodes, committed, sets, exclude=None, masked=(), patch=None, gpus=None, ext_null=False, want=None):
    """committed: pods with status.host, added in order with add_pod (which checks no predicate);
    sets: lists of probe pods; exclude: per set a node name or None; masked: node names whose
    target bit is clear; patch(committed batch, probe batch): edits the records after ingest;
    gpus: (capacity per node, {pod name: request}) turns the extended-resource filter on, and
    ext_null passes the probe pods without their records; want: per set the node names of its
    pods (None: no node)."""
    it = ingest.Interner()
    config = workload.config_default()
    for k in config.label_keys():
        it.key_id(k)
    view = ingest.ClusterView(nodes, [], it)
    probes = [p for s in sets for p in s]
    cb = ingest.ingest_pods(view, committed, uids=list(range(1, len(committed) + 1)))
    pb = ingest.ingest_pods(view, probes, uids=[10 ** 6 + i for i in range(len(probes))])
    if patch:
        patch(cb, pb)
    ext = None
    if gpus is not None:
        from kubernetes_amd.extensions import ExtConfig, ExtInterner

        caps, req = gpus
        ecfg = ExtConfig(taints=False, scalar_resources=("example.com/gpu",))
        inter = ExtInterner(ecfg)
        node_arrays = inter.node_arrays([[] for _ in nodes], {"example.com/gpu": caps})
        crec, cids = inter.pod_records(cb.ids, [[] for _ in committed],
                                       [{"example.com/gpu": req.get(p.metadata.name, 0)} for p in committed])
        prec, pids = inter.pod_records(pb.ids, [[] for _ in probes],
                                       [{"example.com/gpu": req.get(p.metadata.name, 0)} for p in probes])
        cb, pb = PodBatch(cb.pods, cids, crec), PodBatch(pb.pods, pids, None if ext_null else prec)
        ext = (ecfg.compile(1), node_arrays)
    hosts = [view.host_id(p.status.host) for p in committed]
    cfg = config.compile(it.key_id)

    def load(eng):
        if ext:
            eng.set_extensions(ext[0])
        eng.set_cluster(view.arrays)
        if ext:
            eng.set_node_ext(*ext[1])
        for i, h in enumerate(hosts):
            eng.add_pod(h, cb, i)

    names = view.names
    ex = None if exclude is None else [NO_NODE if e is None else names.index(e) for e in exclude]
    targets = None
    if masked:
        targets = np.full((len(names) + 63) // 64, ~np.uint64(0), np.uint64)
        for m in masked:
            r = names.index(m)
            targets[r >> 6] &= ~(np.uint64(1) << np.uint64(r & 63))
    sc = Scenario(name, cfg, load, pb, [len(s) for s in sets], ex, targets, len(nodes))
    sc.names, sc.want = names, want
    return sc


def _three(cpu=1000, mem=8 * GI):
    return [make_node(f"n{i}", cpu, mem) for i in (1, 2, 3)]


def _fill_then_spill():
    """copies of one pod fill the top node to its capacity; the next copy lands one rank down"""
    return _made("fill-then-spill", _three(), [], [[_p(f"c{j}", cpu=400, mem=MI) for j in range(5)]],
                 want=[["n3", "n3", "n2", "n2", "n1"]])


def _port_twice():
    return _made("port-twice", _three(), [], [[_p("a", cpu=100, mem=MI, ports=(8080,)), _p("b", cpu=100, mem=MI, ports=(8080,))]],
                 want=[["n3", "n2"]])


def _pd_twice():
    return _made("pd-twice", _three(), [], [[_p("a", cpu=100, mem=MI, pd="pd-x"), _p("b", cpu=100, mem=MI, pd="pd-x")]],
                 want=[["n3", "n2"]])


def _port_vs_pd():
    """one key id listed as a port by the first pod and as a PD by the second (its PD list is
    pointed at the first pod's port entry): the id space is one, so the second moves down; the
    third, with a port of its own, stays on top"""
    def patch(cb, pb):
        pb.pods["pds_off"][1], pb.pods["n_pds"][1] = pb.pods["ports_off"][0], 1

    return _made("port-vs-pd", _three(), [],
                 [[_p("a", cpu=100, mem=MI, ports=(8080,)), _p("b", cpu=100, mem=MI), _p("c", cpu=100, mem=MI, ports=(9090,))]],
                 patch=patch, want=[["n3", "n2", "n3"]])


def _exclude_top():
    return _made("exclude-top", _three(), [], [[_p("a", cpu=100, mem=MI)], [_p("b", cpu=100, mem=MI)]],
                 exclude=["n3", None], want=[["n2"], ["n3"]])


def _mask():
    return _made("mask", _three(), [], [[_p("a", cpu=100, mem=MI), _p("b", cpu=950, mem=MI)]], masked=("n3",),
                 want=[["n2", "n1"]])


def _nofit_in_middle():
    return _made("nofit-in-middle", _three(), [], [[_p("a", cpu=100, mem=MI), _p("big", cpu=5000, mem=MI), _p("c", cpu=100, mem=MI)]],
                 want=[["n3", None, "n3"]])


def _negative_request():
    """a pod with a negative cpu request, placed first, makes room on its node for the next pod;
    the second set, the big pod alone, shows that it has none as things stand"""
    def patch(cb, pb):
        pb.pods["milli_cpu"][0] = -500

    return _made("negative-request", _three(), [_p("held", "n3", 900, MI)],
                 [[_p("neg", cpu=0, mem=MI), _p("big", cpu=500, mem=MI)], [_p("big2", cpu=500, mem=MI)]], patch=patch,
                 want=[["n3", "n3"], ["n2"]])


def _wrap():
    """requests that wrap the int64 total, as tests/without_cases.py's `wrap`: n2 holds 200 and
    HUGE, so its total reads -2^63 + 100 and no request >= 0 fits; a request of -2^63 + 900 does
    and wraps the total to 1000 = the capacity: then a request of 0 (with memory) fits and one
    of 1 does not"""
    def patch(cb, pb):
        cb.pods["milli_cpu"][1] = HUGE
        pb.pods["milli_cpu"][0] = -(1 << 63) + 900

    nodes = [make_node(f"n{i}", 1000, 8 * GI) for i in (1, 2)]
    return _made("wrap", nodes, [_p("small", "n2", 200, MI), _p("huge", "n2", 100, MI)],
                 [[_p("a", cpu=1, mem=MI), _p("b", cpu=0, mem=MI), _p("c", cpu=1, mem=MI)], [_p("b2", cpu=0, mem=MI)]],
                 patch=patch, want=[["n2", "n2", "n1"], ["n1"]])


def _cap_zero():
    """a cpu capacity of 0 fits every cpu request: only memory fills the top node"""
    nodes = [make_node("n1", 8000, 8 * GI), make_node("n2", 8000, 8 * GI), make_node("n3", 0, 1000 * MI)]
    return _made("cap-zero", nodes, [], [[_p(f"c{j}", cpu=5000, mem=400 * MI) for j in range(4)]],
                 want=[["n3", "n3", "n2", "n1"]])


def _zero_request():
    """a pod that requests neither cpu nor memory skips PodFitsResources on a full node, and adds nothing"""
    return _made("zero-request", _three(), [_p("full", "n3", 1000, MI)],
                 [[_p("z1"), _p("z2"), _p("p", cpu=100, mem=MI), _p("z3")]], want=[["n3", "n3", "n2", "n3"]])


def _ext(name, ext_null):
    """the set's earlier pods exhaust an extended resource (2 GPUs a pod; n3 has 2, n2 has 4);
    with ext == NULL the same pods ignore it"""
    want = [["n3"] * 4] if ext_null else [["n3", "n2", "n2", None]]
    return _made(name, _three(), [], [[_p(f"g{j}", cpu=100, mem=MI) for j in range(4)]],
                 gpus=([0, 4, 2], {f"g{j}": 2 for j in range(4)}), ext_null=ext_null, want=want)


def _last_strip():
    """2 * STRIP + 1 nodes of which only rank 0 fits: the scan's last strip holds one word"""
    nn = 2 * STRIP + 1
    nodes = [make_node(f"n{i:04d}", 1000 if i == 0 else 100, 8 * GI) for i in range(nn)]
    return _made("last-strip", nodes, [], [[_p(f"c{j}", cpu=400, mem=MI) for j in range(3)]],
                 want=[["n0000", "n0000", None]])


def _same_set_twice():
    """the set listed twice gives two identical rows: set 1 does not see set 0"""
    sets = [[_p(f"c{j}", cpu=400, mem=MI, ports=(8080,) if j == 0 else ()) for j in range(4)] for _ in range(2)]
    return _made("same-set-twice", _three(), [], sets, want=[["n3", "n3", "n2", "n2"]] * 2)


LONG_PER_NODE = 300


def _long_set():
    """KSG_PACK_MAX_SET small pods that spill over several nodes, LONG_PER_NODE to a node"""
    nodes = [make_node(f"n{i}", 100 * LONG_PER_NODE, 64 * GI) for i in (1, 2, 3, 4)]
    names = ["n4", "n3", "n2", "n1"]
    return _made("long-set", nodes, [], [[_p(f"s{j}", cpu=100, mem=MI) for j in range(MAX_SET)]],
                 want=[[names[j // LONG_PER_NODE] for j in range(MAX_SET)]])


HANDMADE = {"fill-then-spill": _fill_then_spill, "port-twice": _port_twice, "pd-twice": _pd_twice,
            "port-vs-pd": _port_vs_pd, "exclude-top": _exclude_top, "mask": _mask, "nofit-in-middle": _nofit_in_middle,
            "negative-request": _negative_request, "wrap": _wrap, "cap-zero": _cap_zero, "zero-request": _zero_request,
            "ext-scalar": lambda: _ext("ext-scalar", False), "ext-null": lambda: _ext("ext-null", True),
            "last-strip": _last_strip, "same-set-twice": _same_set_twice, "long-set": _long_set}


@functools.lru_cache(maxsize=None)
def handmade(name: str) -> Scenario:
    return HANDMADE[name]()


def want_rows(sc: Scenario):
    """(out_nodes, placed) as the scenario's `want` writes them out."""
    out = [NOFIT if w is None else sc.names.index(w) for row in sc.want for w in row]
    placed = [sum(w is not None for w in row) for row in sc.want]
    return np.array(out, np.int32), np.array(placed, np.uint32)
