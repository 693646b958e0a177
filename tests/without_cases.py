"""Inputs and references of the ksg_explain_without tests (tests/test_without_inputs.py on the
CPU, tests/test_gpu_without.py on the device).

Two kinds of input:

  batch cases   tests/explain_cases.py's fill and probe pods of XCase(policy, nn) submitted as ONE
                batch. The reference rows of the pods that find no node are the sequential
                scheduler's: pod by pod begin(want_fail=True) / commit((next() >> 1) % k) on the C
                restatement, splitmix64 seed 1234.
  scenarios     an engine state (`load`), an ordered list of committed uids (`absent`), probe pods
                and a position per probe pod. The reference on any engine with add_pod /
                remove_pod / evaluate: remove the list's tail progressively, in descending
                position order, and evaluate the pods of each position (`scenario_reference`).
                The handmade ones (HANDMADE) pin the edges: two holders of one port, a holder
                outside the list, ServiceAffinity peers that leave, appear or sit on an unknown
                host, a total that wrapped, a listed pod on a host outside the node list.

Everything is built once and shared by the tests (read-only)."""
from __future__ import annotations

import functools

import numpy as np

from kubernetes_amd import abi, ingest, workload
from kubernetes_amd.api import (GCEPersistentDiskVolumeSource, ObjectMeta, Pod, PodSpec, PodStatus, Volume, make_node,
                                resource_container)
from kubernetes_amd.engine import PodBatch
from tests import explain_cases as X

SEED = 1234
BATCH_POLICIES = ("config2", "config4", "invalid_selectors", "presence", "hosts")


# ---- batch cases ---------------------------------------------------------------------------
class BatchCase:
    """XCase(policy, nn)'s fill and probe pods as one batch, and its sequential reference."""

    def __init__(self, policy: str, nn: int):
        from oracle.pyoracle import OracleScheduler

        self.case = case = X.xcase(policy, nn)
        self.policy, self.nn, self.cfg = policy, nn, case.cfg
        self.batch = PodBatch(np.concatenate([case.fill.pods, case.probe.pods]), case.fill.ids)
        n = len(self.batch)
        orc = OracleScheduler(case.cfg)
        try:
            orc.set_cluster(case.view.arrays)
            rng = workload._SM(SEED)
            out = np.full(n, -1, np.int32)
            rows = {}
            for i in range(n):
                rc, _, k, fails = orc.begin(self.batch, i, want_fail=True)
                if rc == abi.KSG_OK:
                    out[i] = orc.commit((rng.next() >> 1) % k)
                else:
                    assert rc == abi.KSG_NOFIT, rc
                    rows[i] = fails.copy()
            self.state = rng.s
        finally:
            orc.close()
        self.out = out
        self.nofit = np.array(sorted(rows), np.int64)
        self.rows = np.stack([rows[i] for i in self.nofit]) if len(rows) else np.zeros((0, nn), np.uint8)
        self.placed_uids = self.batch.pods["uid"][out >= 0].astype(np.uint64)
        before = np.concatenate([[0], np.cumsum(out >= 0)])  # placed before pod i
        self.positions = before[self.nofit].astype(np.uint32)
        self.sub = PodBatch(self.batch.pods[self.nofit], self.batch.ids)
        for a in (self.out, self.rows, self.placed_uids, self.positions):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def batch_case(policy: str, nn: int) -> BatchCase:
    return BatchCase(policy, nn)


# ---- scenarios -----------------------------------------------------------------------------
class Scenario:
    def __init__(self, name, cfg, load, absent, probe: PodBatch, positions, n_nodes: int):
        self.name, self.cfg, self.load, self.probe, self.nn = name, cfg, load, probe, n_nodes
        self.absent = np.asarray(absent, np.uint64)
        self.positions = np.asarray(positions, np.uint32)
        assert len(self.positions) == len(probe) and (self.positions <= len(self.absent)).all()


def _evaluate(eng, batch, i):
    """(err, fail codes) on the oracle (a return code) or the device (a KsgError)."""
    try:
        rc, fails, _ = eng.evaluate(batch, i)
    except Exception as e:
        if getattr(e, "code", None) != abi.KSG_ERR_NOPEER:
            raise
        rc, fails = abi.KSG_ERR_NOPEER, None
    if rc == abi.KSG_ERR_NOPEER:
        return 1, None
    assert rc == abi.KSG_OK, rc
    return 0, fails


def scenario_reference(sc: Scenario, eng):
    """(codes uint8[n, N], err uint8[n]) by really removing the list's tail on `eng` (a fresh
    engine, left with the pods removed): descending position order, the pods of each position
    evaluated one by one."""
    sc.load(eng)
    n = len(sc.probe)
    codes, err = np.zeros((n, sc.nn), np.uint8), np.zeros(n, np.uint8)
    left = len(sc.absent)
    for pos in sorted(set(sc.positions.tolist()), reverse=True):
        while left > pos:
            left -= 1
            eng.remove_pod(int(sc.absent[left]))
        for i in np.nonzero(sc.positions == pos)[0]:
            err[i], fails = _evaluate(eng, sc.probe, int(i))
            if fails is not None:
                codes[i] = fails
    return codes, err


_REF = {}


def oracle_reference(sc: Scenario):
    """scenario_reference on the C restatement, computed once per scenario and left unchanged."""
    if sc.name not in _REF:
        from oracle.pyoracle import OracleScheduler

        orc = OracleScheduler(sc.cfg)
        try:
            codes, err = scenario_reference(sc, orc)
        finally:
            orc.close()
        codes.setflags(write=False)
        err.setflags(write=False)
        _REF[sc.name] = (codes, err)
    return _REF[sc.name]


def _spread(k: int, n: int, n_absent: int, salt: int):
    """k probe indices (cycling over n) with positions 0, n_absent and random ones between."""
    rng = workload._SM(salt)
    pos = [0, n_absent] + [rng.below(n_absent + 1) for _ in range(max(k - 2, 0))]
    return [i % n for i in range(k)], pos[:k]


@functools.lru_cache(maxsize=None)
def random_scenario(policy: str, nn: int, k: int) -> Scenario:
    """A random list over the fill's placed pods (about two thirds of them, shuffled), k probe
    pods at positions 0, n_absent and random ones."""
    case = X.xcase(policy, nn)
    placed = case.fill.pods["uid"][batch_fill_out(policy, nn) >= 0]
    rng = workload._SM(31 * nn + k)
    order = sorted(range(len(placed)), key=lambda _: rng.next())
    absent = placed[order[: max(2 * len(placed) // 3, 1)]]
    idx, pos = _spread(k, len(case.probe), len(absent), 7 * nn + k)
    probe = PodBatch(case.probe.pods[idx], case.probe.ids)
    return Scenario(f"random-{policy}-{nn}-{k}", case.cfg, case.load, absent, probe, pos, nn)


@functools.lru_cache(maxsize=None)
def batch_fill_out(policy: str, nn: int) -> np.ndarray:
    from oracle.pyoracle import OracleScheduler

    orc = OracleScheduler(X.xcase(policy, nn).cfg)
    try:
        out, _ = X.xcase(policy, nn).load(orc)
        return out.copy()
    finally:
        orc.close()


N_BLOCKERS = 6
BLOCKER_UID = 900000


@functools.lru_cache(maxsize=None)
def ext_scenario(nn: int, plain_probe: bool = False) -> Scenario:
    """tests/explain_cases.py's extension cluster: the listed pods carry extended-resource
    requests; every probe pod at position 0 and at n_absent, then at random positions. The fill
    leaves the tainted nodes the probe pods stumble over (code 8) with room to spare, so
    N_BLOCKERS of them also get a listed pod that asks for far more cpu than any node has (added
    with add_pod, which checks no predicate): PodFitsResources hides the taint until it leaves."""
    from oracle.pyoracle import OracleScheduler

    c = X.xext(nn)
    orc = OracleScheduler(c.cfg)
    try:
        out, _ = c.load(orc)
        out = out.copy()
        after = np.stack([orc.evaluate(c.probe, i)[1].copy() for i in range(len(c.probe))])
    finally:
        orc.close()
    tainted = np.argsort(-(after == abi.FAIL_TAINTS).sum(axis=0), kind="stable")[:N_BLOCKERS]
    blockers = PodBatch(c.fill.pods[:N_BLOCKERS].copy(), c.fill.ids, np.zeros(N_BLOCKERS, abi.POD_EXT_DTYPE))
    for f in ("n_ports", "n_pds", "n_sel", "n_svcs"):
        blockers.pods[f] = 0
    blockers.pods["service"], blockers.pods["host"], blockers.pods["milli_cpu"] = -1, -1, 10 ** 9
    blockers.pods["uid"] = BLOCKER_UID + np.arange(N_BLOCKERS)

    def load(eng):
        got, _ = c.load(eng)
        assert np.array_equal(got, out)
        for j, node in enumerate(tainted):
            eng.add_pod(int(node), blockers, j)

    placed = np.concatenate([c.fill.pods["uid"][out >= 0], blockers.pods["uid"]])
    rng = workload._SM(5 * nn)
    order = sorted(range(len(placed)), key=lambda _: rng.next())
    absent = placed[order]
    src = c.probe_plain if plain_probe else c.probe
    m = len(src)
    idx = list(range(m)) * 3
    pos = [0] * m + [len(absent)] * m + [rng.below(len(absent) + 1) for _ in range(m)]
    probe = PodBatch(src.pods[idx], src.ids, None if src.ext is None else src.ext[idx])
    return Scenario(f"ext-{nn}-{int(plain_probe)}", c.cfg, load, absent, probe, pos, nn)


# ---- handmade scenarios ----------------------------------------------------------------------
GI = 1 << 30
WEB = {"app": "web"}


def _hpod(name, host="", cpu=None, ports=(), pd=None, selector=None, labels=None):
    vols = [Volume(name="data", gce_persistent_disk=GCEPersistentDiskVolumeSource(pd_name=pd))] if pd else []
    return Pod(metadata=ObjectMeta(name=name, namespace="ns", labels=dict(labels) if labels else None),
               spec=PodSpec(containers=[resource_container(cpu, None if cpu is None else 64 << 20, ports)], volumes=vols,
                            node_selector=selector),
               status=PodStatus(host=host))


def _handmade(name, config, nodes, services, committed, listed, probes, positions=None, patch=None):
    """committed: pods with status.host, added in order with add_pod (which checks no predicate);
    listed: names of committed pods, the ordered list; every probe at every position unless
    `positions` pairs them up; patch(batch): edits the committed pods' records after ingest."""
    it = ingest.Interner()
    for k in config.label_keys():
        it.key_id(k)
    view = ingest.ClusterView(nodes, services, it)
    aff = config.affinity_labels()
    cb = ingest.ingest_pods(view, committed, uids=list(range(1, len(committed) + 1)), aff_labels=aff)
    if patch:
        patch(cb)
    hosts = [view.host_id(p.status.host) for p in committed]
    uid = {p.metadata.name: i + 1 for i, p in enumerate(committed)}
    pb = ingest.ingest_pods(view, probes, uids=[10 ** 6 + i for i in range(len(probes))], aff_labels=aff)
    if positions is None:
        idx = [i for i in range(len(probes)) for _ in range(len(listed) + 1)]
        positions = [p for _ in range(len(probes)) for p in range(len(listed) + 1)]
    else:
        idx = list(range(len(probes)))
    cfg = config.compile(it.key_id)

    def load(eng):
        eng.set_cluster(view.arrays)
        for i, h in enumerate(hosts):
            eng.add_pod(h, cb, i)

    sc = Scenario(name, cfg, load, [uid[x] for x in listed], PodBatch(pb.pods[idx], pb.ids), positions, len(nodes))
    sc.names = [n.metadata.name for n in nodes]
    sc.per_probe = len(listed) + 1
    return sc


def _two_holders(outside: bool) -> Scenario:
    nodes = [make_node(f"n{i}", 1000, 8 * GI) for i in (1, 2, 3)]
    committed = [_hpod("f0", "n2", 100), _hpod("big1", "n1", 700), _hpod("f2", "n3", 100),
                 _hpod("h3", "n1", 100, ports=(8080,)), _hpod("f4", "n2", 100), _hpod("d5", "n1", 100, pd="pd-x"),
                 _hpod("f6", "n3", 100), _hpod("h7", "n1", 100, ports=(8080,))]
    listed = [p.metadata.name for p in committed]  # list index == commit index: h3 at 3, h7 at 7
    if outside:
        committed = committed + [_hpod("out", "n1", 0, ports=(8080,))]
    probes = [_hpod("port-and-pd", cpu=400, ports=(8080,), pd="pd-x"), _hpod("port-only", cpu=100, ports=(8080,))]
    return _handmade("outside-holder" if outside else "two-holders", workload.config_default(), nodes, [], committed,
                     listed, probes)


def _peer_config():
    from tests.test_affinity_trap import _cfg

    return _cfg(("region",))


def _peer_nodes():
    return [make_node("n1", 4000, 8 * GI, labels={"region": "r1"}), make_node("n2", 4000, 8 * GI, labels={"region": "r2"}),
            make_node("n3", 4000, 8 * GI, labels={"region": "r1"})]


def _peer_probes():
    return [_hpod("needs-peer", labels=WEB), _hpod("own-region", selector={"region": "r1"}, labels=WEB),
            _hpod("no-service", labels={"app": "other"})]


def _svc():
    from tests.test_affinity_trap import SVC

    return SVC


def _peers() -> Scenario:
    committed = [_hpod("m0", "n1", labels=WEB), _hpod("m1", "n2", labels=WEB), _hpod("m2", "n3", labels=WEB)]
    return _handmade("peers", _peer_config(), _peer_nodes(), _svc(), committed, ["m2", "m1", "m0"], _peer_probes())


def _peer_unknown() -> Scenario:
    committed = [_hpod("m0", "n1", labels=WEB), _hpod("g", "gone-host", labels=WEB), _hpod("m2", "n3", labels=WEB)]
    return _handmade("peer-unknown", _peer_config(), _peer_nodes(), _svc(), committed, ["m0"], _peer_probes())


def _peer_unknown_converse() -> Scenario:
    committed = [_hpod("g", "gone-host", labels=WEB), _hpod("m1", "n2", labels=WEB)]
    return _handmade("peer-unknown-converse", _peer_config(), _peer_nodes(), _svc(), committed, ["g"], _peer_probes())


HUGE = (1 << 63) - 100  # with the 200 already on the node the int64 total wraps


def _wrap() -> Scenario:
    nodes = [make_node(f"n{i}", 1000, 8 * GI) for i in (1, 2)]
    committed = [_hpod("small", "n1", 200), _hpod("huge", "n1", 100), _hpod("late", "n1", 300)]

    def patch(cb):
        cb.pods["milli_cpu"][1] = HUGE

    return _handmade("wrap", workload.config_default(), nodes, [], committed, ["late", "huge"], [_hpod("p", cpu=500)],
                     patch=patch)


def _outside_host() -> Scenario:
    nodes = [make_node(f"n{i}", 1000, 8 * GI) for i in (1, 2)]
    committed = [_hpod("o", "gone-host", 900, ports=(8080,), pd="pd-x"), _hpod("a", "n1", 300, ports=(8080,))]
    return _handmade("outside-host", workload.config_default(), nodes, [], committed, ["o", "a"],
                     [_hpod("p", cpu=800, ports=(8080,), pd="pd-x")])


HANDMADE = {"two-holders": lambda: _two_holders(False), "outside-holder": lambda: _two_holders(True), "peers": _peers,
            "peer-unknown": _peer_unknown, "peer-unknown-converse": _peer_unknown_converse, "wrap": _wrap,
            "outside-host": _outside_host}


@functools.lru_cache(maxsize=None)
def handmade(name: str) -> Scenario:
    return HANDMADE[name]()
