"""ksg_explain_batch on the GPU: FitError reports (per-node fail codes, per-pod histograms,
peer-error flags) for many pods in one pass, against the C restatement's per-pod evaluate
and the device's own ksg_evaluate. The inputs are tests/explain_cases.py's, which
tests/test_explain_inputs.py shows to reach every fail code; shapes stay within
1,000 nodes x 300 pods.

The report is against the state at the time of the call (include/kschedgpu.h): every test
here explains after a fill batch, with nothing scheduled in between."""
import copy
import ctypes as C
import os
import socket

import numpy as np
import pytest

from kubernetes_amd import abi
from kubernetes_amd.engine import DeviceScheduler, KsgError, PodBatch
from tests import explain_cases as X

pytestmark = pytest.mark.gpu


def _bincount(codes):
    return np.stack([np.bincount(r, minlength=abi.EXPLAIN_SLOTS) for r in codes]).astype(np.uint32)


def _raw_explain(dev, batch, n=None, n_ids=None, codes=None, hist=None, err=None):
    """The C entry point itself, for its return code."""
    pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
    ids = np.ascontiguousarray(batch.ids if len(batch.ids) else np.zeros(1, np.uint32), dtype=np.uint32)
    return dev._lib.ksg_explain_batch(dev._ctx, abi.ptr(pods), None, len(batch) if n is None else n, abi.ptr(ids),
                                      len(batch.ids) if n_ids is None else n_ids, abi.ptr(codes), abi.ptr(hist),
                                      abi.ptr(err))


_DEVICE = {}


def _device_result(policy, nn):
    """One context per (policy, node count), shared by the parity and histogram tests: the fill,
    explain over the probe pods with and without codes, every prefix of POD_COUNTS, and the
    device's own per-pod evaluate."""
    if (policy, nn) in _DEVICE:
        return _DEVICE[policy, nn]
    case = X.xcase(policy, nn)
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        case.load(dev)
        codes, hist, err = dev.explain(case.probe)
        nocodes = dev.explain(case.probe, want_codes=False)
        prefixes = {k: dev.explain(PodBatch(case.probe.pods[:k], case.probe.ids)) for k in X.POD_COUNTS}
        evals = np.stack([dev.evaluate(case.probe, i)[1].copy() for i in range(len(case.probe))])
        again = dev.explain(case.probe)  # (after the evaluates: nothing moved)
    finally:
        dev.close()
    _DEVICE[policy, nn] = dict(codes=codes, hist=hist, err=err, nocodes=nocodes, prefixes=prefixes, evals=evals,
                               again=again)
    return _DEVICE[policy, nn]


@pytest.mark.parametrize("nn", X.NODE_COUNTS)
@pytest.mark.parametrize("policy", X.POLICIES)
def test_parity_with_oracle_and_device_evaluate(policy, nn):
    want = X.oracle_codes_cached(policy, nn)
    r = _device_result(policy, nn)
    assert r["codes"].shape == want.shape == (X.N_PROBE, nn)
    bad = np.argwhere(r["codes"] != want)
    assert bad.size == 0, f"first mismatches (pod, node) {bad[:6].tolist()}"
    assert np.array_equal(r["evals"], r["codes"])  # the device's own per-pod path
    assert not r["err"].any()
    for k, (c, h, e) in r["prefixes"].items():  # 1, chunk - 1, chunk, chunk + 1 pods
        assert c.shape == (k, nn)
        assert np.array_equal(c, want[:k]) and np.array_equal(h, r["hist"][:k]) and not e.any(), k
    assert all(np.array_equal(a, b) for a, b in zip(r["again"], (r["codes"], r["hist"], r["err"])))


@pytest.mark.parametrize("nn", X.NODE_COUNTS)
@pytest.mark.parametrize("policy", X.POLICIES)
def test_histogram(policy, nn):
    want = X.oracle_codes_cached(policy, nn)
    r = _device_result(policy, nn)
    assert r["hist"].shape == (X.N_PROBE, abi.EXPLAIN_SLOTS) and r["hist"].dtype == np.uint32
    assert np.array_equal(r["hist"], _bincount(r["codes"]))
    assert (r["hist"].sum(axis=1) == nn).all()
    assert np.array_equal(r["hist"][:, 0], (want == 0).sum(axis=1))
    c0, h0, e0 = r["nocodes"]  # codes == NULL
    assert c0 is None and np.array_equal(h0, r["hist"]) and np.array_equal(e0, r["err"])


@pytest.mark.parametrize("nn", (X.TILE + 1, 1000))
def test_extensions(nn):
    """Taints and extended resources (codes 8, 9): the `ext` form and the ext == NULL form
    (all-zero records) on an extension context, against the C restatement's evaluate."""
    c = X.xext(nn)
    want, want_plain = X.oracle_codes(c), X.oracle_codes(c, c.probe_plain)
    assert {abi.FAIL_TAINTS, abi.FAIL_SCALAR} <= set(np.unique(want).tolist())
    dev = DeviceScheduler(c.cfg, device=0)
    try:
        c.load(dev)
        codes, hist, err = dev.explain(c.probe)
        pc, ph, pe = dev.explain(c.probe_plain)
        evals = np.stack([dev.evaluate(c.probe, i)[1].copy() for i in range(len(c.probe))])
    finally:
        dev.close()
    assert np.array_equal(codes, want) and np.array_equal(evals, want)
    assert np.array_equal(pc, want_plain)
    assert np.array_equal(hist, _bincount(want)) and np.array_equal(ph, _bincount(want_plain))
    assert not err.any() and not pe.any()


def test_peer_error():
    """A ServiceAffinity pod whose first service peer sits on a host outside the node list
    (predicates.go:293-296): err = 1 and zero rows for it, the other pods unaffected."""
    from kubernetes_amd import ingest
    from oracle.pyoracle import OracleScheduler
    from tests.test_affinity_trap import NODES3, SVC, _cfg, _pod

    config = _cfg(("region",))
    it = ingest.Interner()
    for k in config.label_keys():
        it.key_id(k)
    view = ingest.ClusterView(NODES3, SVC, it)
    aff = config.affinity_labels()
    existing = [_pod("peer", status_host="gone-host")]
    eb = ingest.ingest_pods(view, existing, aff_labels=aff)
    probe = ingest.ingest_pods(view, [_pod("needs-peer"), _pod("own-region", node_selector={"region": "r1"}),
                                      _pod("no-service", labels={"app": "other"}), _pod("needs-peer-too")],
                               uids=[10 ** 6 + i for i in range(4)], aff_labels=aff)
    cfg = config.compile(it.key_id)
    dev, orc = DeviceScheduler(cfg, device=0), OracleScheduler(cfg)
    try:
        for eng in (dev, orc):
            eng.set_cluster(view.arrays)
            eng.add_pod(view.host_id("gone-host"), eb, 0)
        codes, hist, err = dev.explain(probe)
        assert err.tolist() == [1, 0, 0, 1]
        assert not codes[[0, 3]].any() and not hist[[0, 3]].any()
        assert orc.evaluate(probe, 0)[0] == abi.KSG_ERR_NOPEER
        with pytest.raises(KsgError) as ei:
            dev.evaluate(probe, 0)
        assert ei.value.code == abi.KSG_ERR_NOPEER
        for i in (1, 2):
            rc, want, _ = orc.evaluate(probe, i)
            assert rc == abi.KSG_OK and np.array_equal(codes[i], want)
            assert np.array_equal(hist[i], _bincount(want[None])[0])
        assert codes[1].tolist() == [0, abi.FAIL_SERVICEAFFINITY, 0] and not codes[2].any()
    finally:
        dev.close()
        orc.close()


@pytest.mark.parametrize("window", [128, 0])
@pytest.mark.parametrize("ext", [False, True], ids=["plain", "extensions"])
def test_no_side_effects(ext, window):
    """A batch run in chunks with explains of unrelated pods (and of pods already committed,
    and of pods about to be scheduled) in between: placements, the final generator state and
    the committed totals equal the C restatement's uninterrupted run."""
    from oracle.pyoracle import OracleScheduler
    from tests.ext_cases import ExtCase
    from tests.helpers import Case

    nn, n_run, n_other, chunk = 700, 600, 100, 150
    c = ExtCase("config2", nn, n_run + n_other, w_taint=0, w_bal=0) if ext else Case("config2", nn, n_run + n_other)
    b = c.batch

    def sub(lo, hi):
        return PodBatch(b.pods[lo:hi], b.ids, None if b.ext is None else b.ext[lo:hi])

    orc, dev = OracleScheduler(c.cfg), DeviceScheduler(c.cfg, device=0)
    try:
        for eng in (orc, dev):
            c.load(eng) if ext else eng.set_cluster(c.view.arrays)
        dev.set_window(window)
        want, want_state = orc.batch(sub(0, n_run), 4321)
        got, state, windows = [], 4321, 0
        for lo in range(0, n_run, chunk):
            o, state = dev.batch(sub(lo, lo + chunk), state)
            got.append(o)
            windows += dev.last_batch_windows()
            dev.explain(sub(n_run, n_run + n_other))               # unrelated pods
            dev.explain(sub(0, lo + chunk), want_codes=False)      # committed uids
            dev.explain(sub(lo + chunk, min(lo + 2 * chunk, n_run + n_other)))  # the next chunk's pods
        got = np.concatenate(got)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"first mismatches at {bad[:8]}: {got[bad[:8]]} vs {want[bad[:8]]}"
        assert state == want_state
        for a, w_ in zip(dev.read_requested(), orc.read_requested()):
            assert np.array_equal(a, w_)
        if ext:
            assert np.array_equal(dev.read_ext_used(), orc.read_ext_used())
        assert (windows > 0) == (window > 0)  # the explains did not move the batches off their path
    finally:
        dev.close()
        orc.close()


# ---- a node-sharded context explains the whole cluster on every rank -----------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard_worker(rank, world, port, policy, nn, q):
    import torch.distributed as dist

    from kubernetes_amd.engine import gloo_allgather

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        case = X.xcase(policy, nn)
        dev = DeviceScheduler(case.cfg, device=0, rank=rank, world=world, allgather=gloo_allgather())
        case.load(dev)  # (the fill batch is collective)
        codes, hist, err = dev.explain(case.probe)  # (no exchange: each rank on its own)
        lo, hi = dev.shard()
        dev.close()
        q.put((rank, codes, hist, err, lo, hi, None))
    except Exception as e:  # report instead of hanging the parent
        import traceback

        q.put((rank, None, None, None, None, None, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_sharded_ranks_explain_the_whole_cluster():
    import torch.multiprocessing as mp

    policy, nn, world = "config4", 1000, 2
    single = _device_result(policy, nn)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_shard_worker, args=(r, world, port, policy, nn, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=110))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    res.sort(key=lambda r: r[0])
    assert [r[6] for r in res] == [None] * world, [r[6] for r in res]
    assert res[0][4] == 0 and res[0][5] == res[1][4] and 0 < res[1][4] < nn and res[1][5] == nn  # two real shards
    for rank, codes, hist, err, lo, hi, _ in res:
        assert codes.shape == (X.N_PROBE, nn)
        assert np.array_equal(codes, single["codes"]) and np.array_equal(hist, single["hist"])
        assert np.array_equal(err, single["err"])
    assert np.array_equal(single["codes"], X.oracle_codes_cached(policy, nn))


def test_arguments():
    case = X.xcase("config2", 65)
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        case.load(dev)
        nn, probe = case.nn, case.probe
        # n == 0: KSG_OK, nothing written (with or without output buffers)
        codes, hist, err = (np.full(nn, 0xAB, np.uint8), np.full(abi.EXPLAIN_SLOTS, 0xABABABAB, np.uint32),
                            np.full(1, 0xAB, np.uint8))
        assert _raw_explain(dev, probe, n=0, codes=codes, hist=hist, err=err) == abi.KSG_OK
        assert (codes == 0xAB).all() and (hist == 0xABABABAB).all() and (err == 0xAB).all()
        assert _raw_explain(dev, probe, n=0) == abi.KSG_OK
        c0, h0, e0 = dev.explain(PodBatch(probe.pods[:0], probe.ids))
        assert c0.shape == (0, nn) and h0.shape == (0, abi.EXPLAIN_SLOTS) and e0.shape == (0,)
        # hist / err are required once there is a pod
        h1, e1 = np.zeros(abi.EXPLAIN_SLOTS, np.uint32), np.zeros(1, np.uint8)
        assert _raw_explain(dev, probe, n=1, hist=None, err=e1) == abi.KSG_ERR_ARG
        assert _raw_explain(dev, probe, n=1, hist=h1, err=None) == abi.KSG_ERR_ARG
        assert _raw_explain(dev, probe, n=1, hist=h1, err=e1) == abi.KSG_OK and h1.sum() == nn
        # an id list that ends before a pod's lists
        k = int(np.argmax(probe.pods["n_ports"] > 0))
        assert probe.pods["n_ports"][k] > 0
        short = int(probe.pods["ports_off"][k])
        hk, ek = np.zeros((k + 1, abi.EXPLAIN_SLOTS), np.uint32), np.zeros(k + 1, np.uint8)
        assert _raw_explain(dev, probe, n=k + 1, n_ids=short, hist=hk, err=ek) == abi.KSG_ERR_ARG
        assert not hk.any()
        # the same pod twice, and a committed uid, are legal (uid is ignored)
        twice = PodBatch(np.concatenate([probe.pods[:1], probe.pods[:1], case.fill.pods[:1]]), probe.ids)
        c2, _, _ = dev.explain(twice)
        assert np.array_equal(c2[0], c2[1])
        # a pending begin: KSG_ERR_STATE, and the begin is still committable afterwards
        fit = int(np.argmax(dev.explain(probe, want_codes=False)[1][:, 0] > 0))
        rc, _, ties, _ = dev.begin(probe, fit)
        assert rc == abi.KSG_OK and ties > 0
        with pytest.raises(KsgError) as ei:
            dev.explain(probe)
        assert ei.value.code == abi.KSG_ERR_STATE
        node = dev.commit(0)
        after = dev.explain(probe)[0]  # (the resident server, if it served the begin, left the stream)
        assert np.array_equal(after[fit], dev.evaluate(probe, fit)[1])
        assert 0 <= node < nn
        # no nodes
        a = case.view.arrays
        dev.set_cluster(type(a)(a.nodes[:0], a.node_pairs[:0], a.pair_keys, a.n_services))
        h1[:] = 7
        assert _raw_explain(dev, probe, n=1, hist=h1, err=e1) == abi.KSG_NONODES and (h1 == 7).all()
    finally:
        dev.close()


def test_scheduler_level():
    """GPUScheduler.schedule_batch(explain=True) on a nearly full cluster: every unplaced pod's
    FitError carries the map that Schedule(pod) raises right afterwards (a NOFIT commits
    nothing, so the state is the same), from one explain call."""
    from kubernetes_amd.api import PodStatus
    from kubernetes_amd.scheduler import (FakeMinionLister, FakePodLister, FakeServiceLister, FitError, GPUScheduler,
                                          SplitMix64Rand)
    from tests.test_oracle_crosscheck import _workload

    w = _workload("config2", 20, 80, tight=True)
    minions = FakeMinionLister(w.nodes)
    plain = GPUScheduler(w.config, FakePodLister([]), FakeServiceLister(w.services), SplitMix64Rand(3))
    try:
        two = plain.schedule_batch(w.pods, minions, 91)  # explain=False: the two-tuple, as before
    finally:
        plain.close()
    assert len(two) == 2
    lister = FakePodLister([])
    gpu = GPUScheduler(w.config, lister, FakeServiceLister(w.services), SplitMix64Rand(3))
    calls = []
    real = gpu.engine.explain
    gpu.engine.explain = lambda *a, **k: calls.append(1) or real(*a, **k)
    gpu.engine.evaluate = None  # (the report does not go pod by pod)
    try:
        hosts, state, errors = gpu.schedule_batch(w.pods, minions, 91, explain=True)
        assert (hosts, state) == two and len(calls) == 1
        assert len(errors) == len(w.pods) and any(h is None for h in hosts) and any(h is not None for h in hosts)
        for p, h in zip(w.pods, hosts):  # AssumePod reported back by the lister
            if h is not None:
                q = copy.copy(p)
                q.status = PodStatus(host=h)
                lister.pods.append(q)
        nn = len(w.nodes)
        for p, h, e in zip(w.pods, hosts, errors):
            if h is not None:
                assert e is None
                continue
            assert isinstance(e, FitError) and e.pod is p
            with pytest.raises(FitError) as ei:
                gpu.schedule(p, minions)
            assert e.failed_predicates == ei.value.failed_predicates
            assert str(e) == str(ei.value)
            fitting = nn - len(ei.value.failed_predicates)
            assert sum(e.counts.values()) == nn - fitting
            for name, cnt in e.counts.items():
                assert cnt == sum(1 for s in e.failed_predicates.values() if name in s)
        assert FitError(w.pods[0], {}).counts is None  # the positional form stays
    finally:
        gpu.close()
