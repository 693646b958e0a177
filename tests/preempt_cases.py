"""Inputs and the reference of the ksg_preempt_batch tests (tests/test_preempt_inputs.py on the
CPU, tests/test_gpu_preempt.py on the device).

The scenarios are tests/without_cases.py's (an engine state, an ordered list of committed uids,
probe pods and a position per probe pod), the random and extension ones and four of its handmade
ones as they are, plus handmade ones of this file, each named for the edge it pins.

The reference (`reference`) works on any engine with add_pod / remove_pod / evaluate, the C
restatement or a device context. Per probe pod: remove every listed pod at or past its position
(those on a node of the node list), evaluate once (a non-zero code: the node is no candidate),
then walk the removed pods in list order, add_pod each back on its host and evaluate; it stays if
its host's code is still 0, else it is removed again and recorded as a victim of that host.
Without ServiceAffinity the nodes are independent, so one walk serves all of them. `Result` then
applies the choice among the nodes in numpy.

Where a pod was committed (host, record) is recorded while the scenario loads, by an engine proxy
that watches add_pod and batch.

About the choice among nodes: top(i,x) is a list index, and a listed pod is on one host, so two
nodes that both need an eviction never tie on it. The second criterion (fewest victims) therefore
cannot decide between them; the handmade `top-beats-count` scenario shows that the first criterion
wins against the count, and `rank-tie` the only tie there is, between nodes that need no eviction.

Everything is built once and shared by the tests (read-only)."""
from __future__ import annotations

import functools

import numpy as np

from kubernetes_amd import abi, ingest, workload
from kubernetes_amd.api import (GCEPersistentDiskVolumeSource, ObjectMeta, Pod, PodSpec, PodStatus, Volume, make_node,
                                resource_container)
from kubernetes_amd.engine import PodBatch
from tests import explain_cases as X
from tests import without_cases as W

NOFIT = abi.PREEMPT_NOFIT
PAD = 0xFFFFFFFF
MAX_VICTIMS = 16
# (policy, node count) of the random scenarios; ServiceAffinity configurations (config4) are refused
RANDOM = (("config2", 65), ("presence", 63), ("config2", X.TILE + 1))
REUSED = ("two-holders", "outside-holder", "wrap", "outside-host")


class _Recorder:
    """An engine proxy that notes where every pod is committed: uid -> (host, batch, index)."""

    def __init__(self, eng):
        self.eng, self.where = eng, {}

    def __getattr__(self, name):
        return getattr(self.eng, name)

    def add_pod(self, host, batch, i=0):
        self.where[int(batch.pods["uid"][i])] = (int(host), batch, int(i))
        return self.eng.add_pod(host, batch, i)

    def batch(self, batch, seed):
        out, state = self.eng.batch(batch, seed)
        for i in np.flatnonzero(out[: len(batch)] >= 0):
            self.where[int(batch.pods["uid"][i])] = (int(out[i]), batch, int(i))
        return out, state


class Result:
    """What ksg_preempt_batch returns, plus the full victim lists per (pod, node)."""

    def __init__(self, node_victims, lists, rows, n_absent, max_victims):
        n, nn = node_victims.shape
        self.node_victims, self.lists = node_victims, lists
        self.rows = rows  # |C(i,x)| on the candidate nodes
        self.best = np.full(n, -1, np.int32)
        self.n_victims = np.zeros(n, np.uint32)
        self.victims = np.full((n, max_victims), PAD, np.uint32)
        cand = node_victims != NOFIT
        self.cand = cand.sum(axis=1).astype(np.uint32)
        self.free = (node_victims == 0).sum(axis=1).astype(np.uint32)
        for i in range(n):
            if not cand[i].any():
                continue
            # the largest top, then the fewest victims, then the highest rank
            top = np.array([lists[i][x][0] if lists[i][x] else n_absent for x in range(nn)], np.int64)
            key = np.where(cand[i], (top << 32) | (0xFFFFFFFF - node_victims[i].astype(np.int64)), -1)
            x = int(np.flatnonzero(key == key.max())[-1])
            self.best[i], self.n_victims[i] = x, node_victims[i, x]
            v = lists[i][x][:max_victims]
            self.victims[i, : len(v)] = v
        for a in (self.node_victims, self.rows, self.best, self.n_victims, self.victims, self.cand, self.free):
            a.setflags(write=False)

    def kinds(self):
        """(cells with victims and reprieved pods both, non-candidate cells, pods whose best node
        needs an eviction, pods that fit a node with none, pods without a candidate)"""
        nv = self.node_victims
        mixed = (nv != NOFIT) & (nv > 0) & (self.rows > nv)
        return (int(mixed.sum()), int((nv == NOFIT).sum()), int((self.n_victims > 0).sum()), int((self.free > 0).sum()),
                int((self.cand == 0).sum()))

    def outputs(self):
        return self.best, self.n_victims, self.victims, self.cand, self.free, self.node_victims


def reference(sc, eng, max_victims: int = MAX_VICTIMS) -> Result:
    """The walk described above on `eng` (a fresh engine; left in the scenario's loaded state)."""
    rec = _Recorder(eng)
    sc.load(rec)
    nn, na, n = sc.nn, len(sc.absent), len(sc.probe)
    where = [rec.where[int(u)] for u in sc.absent]
    node_victims = np.full((n, nn), NOFIT, np.uint32)
    lists = [[[] for _ in range(nn)] for _ in range(n)]
    rows = np.zeros((n, nn), np.uint32)
    for i in range(n):
        cands = [j for j in range(int(sc.positions[i]), na) if where[j][0] < nn]
        for j in cands:
            eng.remove_pod(int(sc.absent[j]))
        err, codes = W._evaluate(eng, sc.probe, i)
        assert not err
        ok = np.array(codes) == 0
        node_victims[i, ok] = 0
        gone = []
        for j in cands:
            host = where[j][0]
            eng.add_pod(*where[j])
            if not ok[host]:
                continue  # (no candidate: its pods only go back)
            rows[i, host] += 1
            err, codes = W._evaluate(eng, sc.probe, i)
            assert not err
            if codes[host] != 0:
                eng.remove_pod(int(sc.absent[j]))
                gone.append(j)
                lists[i][host].append(j)
                node_victims[i, host] += 1
        for j in gone:
            eng.add_pod(*where[j])
    return Result(node_victims, lists, rows, na, max_victims)


_REF = {}


def oracle_reference(sc, max_victims: int = MAX_VICTIMS) -> Result:
    """`reference` on the C restatement, computed once per (scenario, max_victims)."""
    if (sc.name, max_victims) not in _REF:
        from oracle.pyoracle import OracleScheduler

        orc = OracleScheduler(sc.cfg)
        try:
            _REF[sc.name, max_victims] = reference(sc, orc, max_victims)
        finally:
            orc.close()
    return _REF[sc.name, max_victims]


# ---- handmade scenarios ----------------------------------------------------------------------
MI = 1 << 20
GI = 1 << 30


def _p(name, host="", cpu=0, mem=0, ports=(), pd=None):
    vols = [Volume(name="data", gce_persistent_disk=GCEPersistentDiskVolumeSource(pd_name=pd))] if pd else []
    return Pod(metadata=ObjectMeta(name=name, namespace="ns"),
               spec=PodSpec(containers=[resource_container(cpu, mem, ports)], volumes=vols),
               status=PodStatus(host=host))


def _made(name, nodes, committed, listed, probes, positions=None, patch=None, gpus=None, want=None):
    """committed: pods with status.host, added in order with add_pod (which checks no predicate);
    listed: their names in list order; every probe at position 0 unless `positions` says otherwise;
    patch(batch): edits the committed records after ingest; gpus: (capacity per node, {pod name:
    request}) turns the extended-resource filter on; want: {(probe, node name): [victim names]}
    for the test that writes the lists out (nodes not named: no candidate)."""
    it = ingest.Interner()
    config = workload.config_default()
    for k in config.label_keys():
        it.key_id(k)
    view = ingest.ClusterView(nodes, [], it)
    cb = ingest.ingest_pods(view, committed, uids=list(range(1, len(committed) + 1)))
    pb = ingest.ingest_pods(view, probes, uids=[10 ** 6 + i for i in range(len(probes))])
    if patch:
        patch(cb)
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
        cb, pb = PodBatch(cb.pods, cids, crec), PodBatch(pb.pods, pids, prec)
        ext = (ecfg.compile(1), node_arrays)
    hosts = [view.host_id(p.status.host) for p in committed]
    uid = {p.metadata.name: i + 1 for i, p in enumerate(committed)}
    cfg = config.compile(it.key_id)

    def load(eng):
        if ext:
            eng.set_extensions(ext[0])
        eng.set_cluster(view.arrays)
        if ext:
            eng.set_node_ext(*ext[1])
        for i, h in enumerate(hosts):
            eng.add_pod(h, cb, i)

    sc = W.Scenario(name, cfg, load, [uid[x] for x in listed], pb,
                    [0] * len(probes) if positions is None else positions, len(nodes))
    sc.names = [n.metadata.name for n in nodes]
    sc.listed = list(listed)
    sc.want = want
    return sc


def _memory_only():
    """cpu never binds: of a (400Mi), b (300Mi), c (100Mi) on a 1000Mi node a pod of 500Mi lets a
    and c stay and evicts b."""
    nodes = [make_node("n1", 8000, 1000 * MI), make_node("n2", 8000, 100 * MI)]
    committed = [_p("a", "n1", 100, 400 * MI), _p("b", "n1", 100, 300 * MI), _p("c", "n1", 100, 100 * MI)]
    return _made("memory-only", nodes, committed, ["a", "b", "c"], [_p("p", cpu=100, mem=500 * MI)],
                 want={(0, "n1"): ["b"]})


def _ext_only():
    """only the extended resource binds: 4 GPUs, a (2), b (1), c (2), a pod of 2: a stays."""
    nodes = [make_node("n1", 8000, 8 * GI), make_node("n2", 8000, 8 * GI)]
    committed = [_p("a", "n1", 100, MI), _p("b", "n1", 100, MI), _p("c", "n1", 100, MI)]
    return _made("ext-only", nodes, committed, ["a", "b", "c"], [_p("p", cpu=100, mem=MI)],
                 gpus=([4, 0], {"a": 2, "b": 1, "c": 2, "p": 2}), want={(0, "n1"): ["b", "c"]})


def _zero_request():
    """a pod that requests neither cpu nor memory skips PodFitsResources: on a full node every
    candidate is reprieved; a second probe with a request evicts them all."""
    nodes = [make_node("n1", 1000, 1000 * MI)]
    committed = [_p("a", "n1", 500, 500 * MI), _p("b", "n1", 500, 500 * MI)]
    return _made("zero-request", nodes, committed, ["a", "b"], [_p("zero"), _p("full", cpu=1000, mem=MI)],
                 want={(0, "n1"): [], (1, "n1"): ["a", "b"]})


def _cap_zero():
    """a cpu capacity of 0 fits every cpu request: only memory decides (a leaves, b stays)."""
    nodes = [make_node("n1", 0, 1000 * MI)]
    committed = [_p("a", "n1", 5000, 600 * MI), _p("b", "n1", 5000, 300 * MI)]
    return _made("cap-zero", nodes, committed, ["a", "b"], [_p("p", cpu=9000, mem=500 * MI)], want={(0, "n1"): ["a"]})


def _negative_request():
    """the greedy order matters: x (600) before neg (-200) is a victim on n1 (600 + 500 > 1000);
    after neg on n2 it stays (-200 + 600 + 500 <= 1000)."""
    nodes = [make_node("n1", 1000, 8 * GI), make_node("n2", 1000, 8 * GI)]
    committed = [_p("x1", "n1", 600, MI), _p("neg1", "n1", 0, MI), _p("neg2", "n2", 0, MI), _p("x2", "n2", 600, MI)]

    def patch(cb):
        cb.pods["milli_cpu"][1] = -200
        cb.pods["milli_cpu"][2] = -200

    return _made("negative-request", nodes, committed, ["x1", "neg1", "neg2", "x2"], [_p("p", cpu=500, mem=MI)],
                 patch=patch, want={(0, "n1"): ["x1"], (0, "n2"): []})


def _top_beats_count():
    """n1 needs one victim, the most important pod of the list; n2 needs two lesser ones: n2."""
    nodes = [make_node("n1", 1000, 8 * GI), make_node("n2", 1000, 8 * GI), make_node("n3", 100, 8 * GI)]
    committed = [_p("vip", "n1", 1000, MI), _p("l1", "n2", 500, MI), _p("l2", "n2", 500, MI)]
    return _made("top-beats-count", nodes, committed, ["vip", "l1", "l2"], [_p("p", cpu=900, mem=MI)],
                 want={(0, "n1"): ["vip"], (0, "n2"): ["l1", "l2"]})


def _rank_tie():
    """n1 and n3 take the pod as they are, n2 after an eviction: the highest rank of the two, n3;
    a second, larger probe must evict somewhere and has one candidate."""
    nodes = [make_node("n1", 1000, 8 * GI), make_node("n2", 1000, 8 * GI), make_node("n3", 1000, 8 * GI)]
    committed = [_p("a", "n2", 800, MI), _p("b", "n1", 100, MI), _p("c", "n3", 100, MI)]
    return _made("rank-tie", nodes, committed, ["a", "b", "c"], [_p("p", cpu=500, mem=MI), _p("q", cpu=950, mem=MI)],
                 positions=[0, 0], want={(0, "n1"): [], (0, "n2"): ["a"], (0, "n3"): [], (1, "n1"): ["b"],
                                         (1, "n2"): ["a"], (1, "n3"): ["c"]})


LONG = 20


def _long_row():
    """a row of LONG pods of 100 on a node of 2000: a pod of 1850 lets the first stay and evicts
    the other LONG - 1, more than MAX_VICTIMS."""
    nodes = [make_node("n1", 2000, 8 * GI), make_node("n2", 1000, 8 * GI)]
    committed = [_p(f"s{j}", "n1", 100, MI) for j in range(LONG)]
    listed = [f"s{j}" for j in range(LONG)]
    return _made("long-row", nodes, committed, listed, [_p("p", cpu=1850, mem=MI)], want={(0, "n1"): listed[1:]})


HANDMADE = {"memory-only": _memory_only, "ext-only": _ext_only, "zero-request": _zero_request, "cap-zero": _cap_zero,
            "negative-request": _negative_request, "top-beats-count": _top_beats_count, "rank-tie": _rank_tie,
            "long-row": _long_row}


@functools.lru_cache(maxsize=None)
def handmade(name: str):
    """One of this file's scenarios, or one of tests/without_cases.py's that take no ServiceAffinity."""
    return HANDMADE[name]() if name in HANDMADE else W.handmade(name)


ALL_HANDMADE = tuple(sorted(HANDMADE)) + REUSED
