"""ksg_prioritize_batch on the GPU: per pod what ksg_schedule_begin would return now, the nodes
it fits, the head of its HostPriorityList and (optionally) its per-node combined scores, for
many pods in one pass, against the C restatement's per-pod evaluate (tests/prioritize_cases.py)
and the device's own ksg_evaluate, ksg_explain_batch and begin / commit. Every comparison is
integer and bit-exact. tests/test_prioritize_inputs.py shows the inputs reach every regime.

The result is against the state at the time of the call (include/kschedgpu.h): every test here
asks after a fill, with nothing scheduled in between unless the test is about that."""
import os

import numpy as np
import pytest

from kubernetes_amd import abi
from kubernetes_amd.engine import DeviceScheduler, KsgError, PodBatch
from tests import explain_cases as X
from tests import prioritize_cases as P
from tests.test_gpu_explain import _free_port

pytestmark = pytest.mark.gpu

KEYS = ("max", "ties", "fit", "top_nodes", "top_scores", "scores", "err")
PER_POD = ("max", "ties", "fit", "top_nodes", "top_scores", "err")
TOPS = (0, 1, abi.PRIO_MAX_TOP)


def _res(t) -> dict:
    return dict(zip(KEYS, t))


def _same(got: dict, want: dict, keys=KEYS, rows=slice(None)):
    for k in keys:
        g, w = got[k], want[k][rows]
        assert g.dtype == w.dtype and g.shape == w.shape, (k, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{k}: first mismatches {bad[:6].tolist()}: {g[g != w][:6]} vs {w[g != w][:6]}"


def _retop(want: dict, top: int) -> dict:
    """The reference at another list length, from one with a longer (or equal) list."""
    w = dict(want)
    w["top_nodes"], w["top_scores"] = want["top_nodes"][:, :top], want["top_scores"][:, :top]
    return w


def _eval_rows(dev, probe):
    """The device's own per-pod path: score_out rows, NOFIT rows for a peer error."""
    rows = []
    for i in range(len(probe)):
        try:
            rows.append(dev.evaluate(probe, i)[2].copy())
        except KsgError as e:
            assert e.code == abi.KSG_ERR_NOPEER
            rows.append(np.full(dev.n_nodes, abi.SCORE_NOFIT, np.int64))
    return np.stack(rows)


_DEVICE = {}


def _device_result(policy, nn):
    """One context per (policy, node count): the fill, then every form the parity test compares."""
    if (policy, nn) in _DEVICE:
        return _DEVICE[policy, nn]
    case = X.xcase(policy, nn)
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        case.load(dev)
        r = dict(full=_res(dev.prioritize(case.probe, top=P.TOP, want_scores=True)),
                 noscores=_res(dev.prioritize(case.probe, top=P.TOP)),
                 prefixes={k: _res(dev.prioritize(PodBatch(case.probe.pods[:k], case.probe.ids), top=P.TOP,
                                                  want_scores=True)) for k in X.POD_COUNTS},
                 tops={t: _res(dev.prioritize(case.probe, top=t, want_scores=True)) for t in TOPS},
                 hist0=dev.explain(case.probe, want_codes=False)[1][:, 0].copy(),
                 evals=_eval_rows(dev, case.probe))
        r["again"] = _res(dev.prioritize(case.probe, top=P.TOP, want_scores=True))  # (after the evaluates)
        r["ms"] = dev.last_prioritize_ms()
    finally:
        dev.close()
    _DEVICE[policy, nn] = r
    return r


@pytest.mark.parametrize("nn", X.NODE_COUNTS)
@pytest.mark.parametrize("policy", X.POLICIES)
def test_parity_with_oracle_and_device(policy, nn):
    want = P.xreference(policy, nn)
    want16 = P.xreference(policy, nn, abi.PRIO_MAX_TOP)
    r = _device_result(policy, nn)
    assert r["full"]["scores"].shape == (X.N_PROBE, nn) and r["full"]["top_nodes"].shape == (X.N_PROBE, P.TOP)
    _same(r["full"], want)
    assert np.array_equal(r["full"]["scores"], r["evals"])  # ksg_evaluate's score_out rows, bit for bit
    assert np.array_equal(r["full"]["fit"], r["hist0"])     # ksg_explain_batch's hist[:, 0]
    for k, got in r["prefixes"].items():  # 1, chunk - 1, chunk, chunk + 1 pods
        _same(got, want, rows=slice(0, k))
    for t, got in r["tops"].items():
        _same(got, _retop(want16, t))
    assert r["noscores"]["scores"] is None
    _same(r["noscores"], want, keys=PER_POD)
    _same(r["again"], r["full"])
    assert r["ms"] > 0.0


@pytest.mark.parametrize("name", ("config2", "config4"))
def test_normalised_terms_and_extensions(name):
    """TaintToleration (normalised by the max over the filtered nodes), BalancedResourceAllocation,
    taints and extended resources as filters, with ServiceAntiAffinity's domain counts under
    config4: the `ext` form and the ext == NULL form (all-zero records) on one context."""
    c = P.pext(name)
    want, want_plain = P.pext_reference(name, False), P.pext_reference(name, True)
    dev = DeviceScheduler(c.cfg, device=0)
    try:
        c.load(dev)
        got = _res(dev.prioritize(c.probe, top=P.TOP, want_scores=True))
        got_plain = _res(dev.prioritize(c.probe_plain, top=P.TOP, want_scores=True))
        evals, evals_plain = _eval_rows(dev, c.probe), _eval_rows(dev, c.probe_plain)
    finally:
        dev.close()
    _same(got, want)
    _same(got_plain, want_plain)
    assert np.array_equal(got["scores"], evals) and np.array_equal(got_plain["scores"], evals_plain)
    assert (want["scores"] != want_plain["scores"]).any()


def _edge_policies():
    from tests import numeric_edges as NE

    return sorted(NE.policies())


@pytest.mark.parametrize("policy", _edge_policies())
@pytest.mark.parametrize("kind", ("tame", "wild"))
def test_wide_scores(kind, policy):
    """Weights up to 2^62 and LeastRequested terms outside [0, 10]: rows, max and ties equal the
    C restatement's wrapped int64 values."""
    from oracle.pyoracle import OracleScheduler
    from tests import numeric_edges as NE

    case = NE.edge_case(kind, policy)
    orc = OracleScheduler(case.cfg)
    try:
        case.load(orc)
        rows = []
        for i in range(len(case.batch)):
            rc, fails, scores = orc.evaluate(case.batch, i)
            rows.append((rc, fails.copy(), scores.copy()))
    finally:
        orc.close()
    want = P.reference(rows, P.TOP)
    assert (want["fit"] > 0).any()
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        case.load(dev)
        got = _res(dev.prioritize(case.batch, top=P.TOP, want_scores=True))
        _same(got, want)
    finally:
        dev.close()


def test_wild_requests_leave_the_window_path_on():
    """The call scores in wrapping int64 whatever the pods ask, so it does not move a context to
    the int64 kernels: after pods with negative requests went through it, a tame batch still
    runs in windows. (numeric_edges.edge_case's tame clusters hold capacities past the window
    path's 2^49 bound and never run in windows, so this uses gate_case's window-eligible one.)
    The same pods through ksg_evaluate do move it: that call looks at the requests."""
    from oracle.pyoracle import OracleScheduler
    from tests import numeric_edges as NE

    case = NE.gate_case("requests_non_negative")
    assert NE.GATE_CASES["requests_non_negative"]
    wild = PodBatch(case.batch.pods[:5].copy(), case.batch.ids)
    wild.pods["milli_cpu"][:] = [-1, -(1 << 40), 3, -7, 1 << 61]
    wild.pods["memory"][:] = [2, 5, -(1 << 62), -7, 1 << 61]
    orc = case.load(OracleScheduler(case.cfg))
    try:
        rows = []
        for i in range(len(wild)):
            rc, fails, scores = orc.evaluate(wild, i)
            rows.append((rc, fails.copy(), scores.copy()))
    finally:
        orc.close()
    want = P.reference(rows, P.TOP)
    assert (want["fit"] > 0).any()
    dev = case.load(DeviceScheduler(case.cfg, device=0))
    try:
        dev.set_window(64)
        _same(_res(dev.prioritize(wild, top=P.TOP, want_scores=True)), want)
        dev.batch(case.batch, 31)
        assert dev.last_batch_windows() > 0
    finally:
        dev.close()
    dev = case.load(DeviceScheduler(case.cfg, device=0))
    try:
        dev.set_window(64)
        dev.evaluate(wild, 0)
        dev.batch(case.batch, 31)
        assert dev.last_batch_windows() == 0
    finally:
        dev.close()


def test_empty_priorities_and_equal_fallback():
    """Priority configs whose weights are all 0: the HostPriorityList is empty (0 ties, no top
    entries) although nodes fit, and the scores row is still ksg_evaluate's. No priority configs
    at all: EqualPriority scores every fitting node 1. begin agrees on (rc, max, ties)."""
    from kubernetes_amd import factory, ingest
    from oracle.pyoracle import OracleScheduler

    case = X.xcase("config2", 65)
    preds = ["PodFitsResources", "PodFitsPorts", "NoDiskConflict", "MatchNodeSelector", "HostName"]
    for prios, empty in ((["EqualPriority"], True), ([], False)):
        sc = factory.create_from_keys(preds, prios)
        sc.max_conflict_keys = 4096
        assert not sc.label_keys()  # (so the case's interned cluster serves this policy too)
        cfg = sc.compile(ingest.Interner().key_id)
        orc = OracleScheduler(cfg)
        try:
            case.load(orc)
            rows = []
            for i in range(len(case.probe)):
                rc, fails, scores = orc.evaluate(case.probe, i)
                rows.append((rc, fails.copy(), scores.copy()))
        finally:
            orc.close()
        want = P.reference(rows, P.TOP, empty_priorities=empty)
        assert (want["fit"] > 0).any() and (want["fit"] < P.TOP).any() and (want["fit"] < case.nn).any()
        dev = DeviceScheduler(cfg, device=0)
        try:
            case.load(dev)
            got = _res(dev.prioritize(case.probe, top=P.TOP, want_scores=True))
            _same(got, want)
            assert np.array_equal(got["scores"], _eval_rows(dev, case.probe))
            if empty:
                assert not got["ties"].any() and not got["max"].any() and (got["top_nodes"] == -1).all()
            else:
                fits = got["fit"] > 0
                assert (got["max"][fits] == 1).all() and np.array_equal(got["ties"], got["fit"])
                assert set(np.unique(got["scores"]).tolist()) <= {1, abi.SCORE_NOFIT}
            # begin for the same pod, last (a begin that finds a node stays pending)
            for i in np.argsort(got["ties"], kind="stable"):
                rc, m, k, _ = dev.begin(case.probe, int(i))
                assert (m, k) == (int(got["max"][i]), int(got["ties"][i])), i
                assert rc == (abi.KSG_OK if k else abi.KSG_NOFIT)
                if rc == abi.KSG_OK:
                    assert dev.commit(0) == got["top_nodes"][i, 0]
                    break
        finally:
            dev.close()


def test_commit_order():
    """begin + commit(tie_index = j) picks top_nodes[i][j] for j < ties."""
    case = X.xcase("config2", X.TILE + 1)
    want = P.xreference("config2", X.TILE + 1)
    i = int(np.argmax(want["ties"] >= 3))
    assert want["ties"][i] >= 3
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        case.load(dev)
        got = _res(dev.prioritize(case.probe, top=P.TOP))
        rc, m, k, _ = dev.begin(case.probe, i)
        assert (rc, m, k) == (abi.KSG_OK, int(got["max"][i]), int(got["ties"][i]))
        assert dev.commit(2) == got["top_nodes"][i, 2] == want["top_nodes"][i, 2]
    finally:
        dev.close()


def test_peer_error():
    """A ServiceAffinity pod whose first service peer sits on a host outside the node list
    (predicates.go:293-296): err = 1 and an empty row for it, the other pods unaffected."""
    from kubernetes_amd import ingest
    from oracle.pyoracle import OracleScheduler
    from tests.test_affinity_trap import NODES3, SVC, _cfg, _pod

    config = _cfg(("region",))
    it = ingest.Interner()
    for k in config.label_keys():
        it.key_id(k)
    view = ingest.ClusterView(NODES3, SVC, it)
    aff = config.affinity_labels()
    eb = ingest.ingest_pods(view, [_pod("peer", status_host="gone-host")], aff_labels=aff)
    probe = ingest.ingest_pods(view, [_pod("needs-peer"), _pod("own-region", node_selector={"region": "r1"}),
                                      _pod("no-service", labels={"app": "other"}), _pod("needs-peer-too")],
                               uids=[10 ** 6 + i for i in range(4)], aff_labels=aff)
    cfg = config.compile(it.key_id)
    dev, orc = DeviceScheduler(cfg, device=0), OracleScheduler(cfg)
    try:
        for eng in (dev, orc):
            eng.set_cluster(view.arrays)
            eng.add_pod(view.host_id("gone-host"), eb, 0)
        rows = []
        for i in range(4):
            rc, fails, scores = orc.evaluate(probe, i)
            rows.append((rc, fails.copy(), scores.copy()))
        assert [r[0] for r in rows] == [abi.KSG_ERR_NOPEER, abi.KSG_OK, abi.KSG_OK, abi.KSG_ERR_NOPEER]
        want = P.reference(rows, 2)
        got = _res(dev.prioritize(probe, top=2, want_scores=True))
        assert got["err"].tolist() == [1, 0, 0, 1]
        _same(got, want)
        for i in (0, 3):
            assert (got["max"][i], got["ties"][i], got["fit"][i]) == (0, 0, 0)
            assert (got["top_nodes"][i] == -1).all() and not got["top_scores"][i].any()
            assert (got["scores"][i] == abi.SCORE_NOFIT).all()
        assert got["fit"][1] > 0 and got["fit"][2] > 0
    finally:
        dev.close()
        orc.close()


@pytest.mark.parametrize("window", [128, 0])
@pytest.mark.parametrize("ext", [False, True], ids=["plain", "extensions"])
def test_no_side_effects(ext, window):
    """A batch run in chunks with prioritize calls over unrelated pods, committed uids and the next
    chunk's pods in between: placements, the final generator state, the committed totals and the
    extended-resource usage equal the C restatement's uninterrupted run, on the same path."""
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
            dev.prioritize(sub(n_run, n_run + n_other), top=4, want_scores=True)   # unrelated pods
            dev.prioritize(sub(0, lo + chunk), top=4)                              # committed uids
            dev.prioritize(sub(lo + chunk, min(lo + 2 * chunk, n_run + n_other)), top=4, want_scores=True)  # the next chunk's
        got = np.concatenate(got)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"first mismatches at {bad[:8]}: {got[bad[:8]]} vs {want[bad[:8]]}"
        assert state == want_state
        for a, w_ in zip(dev.read_requested(), orc.read_requested()):
            assert np.array_equal(a, w_)
        if ext:
            assert np.array_equal(dev.read_ext_used(), orc.read_ext_used())
        assert (windows > 0) == (window > 0)  # the calls did not move the batches off their path
    finally:
        dev.close()
        orc.close()


# ---- a node-sharded context ranks the whole cluster on every rank ---------------------
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
        # no exchange: each rank on its own, a different number of times (a collective call would hang)
        for _ in range(rank + 1):
            res = dev.prioritize(case.probe, top=P.TOP, want_scores=True)
        lo, hi = dev.shard()
        dev.close()
        q.put((rank, res, lo, hi, None))
    except Exception as e:  # report instead of hanging the parent
        import traceback

        q.put((rank, None, None, None, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_sharded_ranks_cover_the_whole_cluster():
    import torch.multiprocessing as mp

    policy, nn, world = "config4", X.TILE + 1, 2
    single = _device_result(policy, nn)["full"]
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
    assert [r[4] for r in res] == [None] * world, [r[4] for r in res]
    assert res[0][2] == 0 and res[0][3] == res[1][2] and 0 < res[1][2] < nn and res[1][3] == nn  # two real shards
    for rank, got, lo, hi, _ in res:
        _same(_res(got), single)
    _same(single, P.xreference(policy, nn))


def _raw(dev, batch, n=None, n_ids=None, top=0, ext=None, **out):
    """The C entry point itself, for its return code. out: max, ties, fit, tn, ts, scores, err."""
    pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
    ids = np.ascontiguousarray(batch.ids if len(batch.ids) else np.zeros(1, np.uint32), dtype=np.uint32)
    return dev._lib.ksg_prioritize_batch(dev._ctx, abi.ptr(pods), abi.ptr(ext), len(batch) if n is None else n,
                                         abi.ptr(ids), len(batch.ids) if n_ids is None else n_ids, top,
                                         *(abi.ptr(out.get(k)) for k in ("max", "ties", "fit", "tn", "ts", "scores", "err")))


def test_arguments():
    case = X.xcase("config2", 65)
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        case.load(dev)
        nn, probe = case.nn, case.probe

        def bufs(n=1, top=2):
            return dict(max=np.full(n, 0x5A5A, np.int64), ties=np.full(n, 0x5A5A, np.uint32),
                        fit=np.full(n, 0x5A5A, np.uint32), tn=np.full(n * top, 0x5A5A, np.int32),
                        ts=np.full(n * top, 0x5A5A, np.int64), scores=np.full(n * nn, 0x5A5A, np.int64),
                        err=np.full(n, 0x5A, np.uint8))

        def untouched(o):
            return all((a == (0x5A if a.dtype == np.uint8 else 0x5A5A)).all() for a in o.values())

        # n == 0: KSG_OK, nothing written (with or without output buffers)
        o = bufs()
        assert _raw(dev, probe, n=0, top=2, **o) == abi.KSG_OK and untouched(o)
        assert _raw(dev, probe, n=0) == abi.KSG_OK
        e = dev.prioritize(PodBatch(probe.pods[:0], probe.ids), top=3, want_scores=True)
        assert e[3].shape == (0, 3) and e[5].shape == (0, nn) and e[6].shape == (0,)
        # the per-pod arrays are required once there is a pod
        for missing in ("max", "ties", "fit", "err"):
            o = bufs()
            o[missing] = None
            assert _raw(dev, probe, n=1, top=2, **o) == abi.KSG_ERR_ARG, missing
            assert untouched({k: v for k, v in o.items() if v is not None})
        # top: at most KSG_PRIO_MAX_TOP; the top arrays may be NULL iff top == 0
        o = bufs(top=abi.PRIO_MAX_TOP + 1)
        assert _raw(dev, probe, n=1, top=abi.PRIO_MAX_TOP + 1, **o) == abi.KSG_ERR_ARG and untouched(o)
        for missing in ("tn", "ts"):
            o = bufs()
            o[missing] = None
            assert _raw(dev, probe, n=1, top=2, **o) == abi.KSG_ERR_ARG, missing
            assert untouched({k: v for k, v in o.items() if v is not None})
        o = bufs()
        o["tn"] = o["ts"] = o["scores"] = None
        assert _raw(dev, probe, n=1, top=0, **o) == abi.KSG_OK and o["err"][0] == 0 and o["fit"][0] <= nn
        o = bufs()
        assert _raw(dev, probe, n=1, top=2, **o) == abi.KSG_OK and not untouched(o)
        # ext on a context without extensions
        o = bufs()
        ext = np.zeros(1, abi.POD_EXT_DTYPE)
        assert _raw(dev, probe, n=1, top=2, ext=ext, **o) == abi.KSG_ERR_STATE and untouched(o)
        # an id list that ends before a pod's lists
        k = int(np.argmax(probe.pods["n_ports"] > 0))
        assert probe.pods["n_ports"][k] > 0
        o = bufs(n=k + 1)
        assert _raw(dev, probe, n=k + 1, n_ids=int(probe.pods["ports_off"][k]), top=2, **o) == abi.KSG_ERR_ARG
        assert untouched(o)
        # the same pod twice, and a committed uid, are legal (uid is ignored)
        twice = PodBatch(np.concatenate([probe.pods[:1], probe.pods[:1], case.fill.pods[:1]]), probe.ids)
        t = _res(dev.prioritize(twice, top=2, want_scores=True))
        assert all(np.array_equal(t[key][0], t[key][1]) for key in KEYS)
        # a pending begin: KSG_ERR_STATE, and the begin is still committable afterwards
        first = _res(dev.prioritize(probe, top=2))
        fit = int(np.argmax(first["fit"] > 0))
        rc, _, ties, _ = dev.begin(probe, fit)
        assert rc == abi.KSG_OK and ties == first["ties"][fit] > 0
        o = bufs()
        assert _raw(dev, probe, n=1, top=2, **o) == abi.KSG_ERR_STATE and untouched(o)
        with pytest.raises(KsgError) as ei:
            dev.prioritize(probe)
        assert ei.value.code == abi.KSG_ERR_STATE
        assert dev.commit(0) == first["top_nodes"][fit, 0]
        after = _res(dev.prioritize(probe, top=2, want_scores=True))  # (the resident server left the stream)
        assert np.array_equal(after["scores"][fit], dev.evaluate(probe, fit)[2])
        # no nodes
        a = case.view.arrays
        dev.set_cluster(type(a)(a.nodes[:0], a.node_pairs[:0], a.pair_keys, a.n_services))
        o = bufs()
        o["scores"] = None
        assert _raw(dev, probe, n=1, top=2, **o) == abi.KSG_NONODES
        assert untouched({k: v for k, v in o.items() if v is not None})
    finally:
        dev.close()


@pytest.mark.parametrize("policy", ("default", "config4"))
def test_scheduler_level(policy):
    """GPUScheduler.prioritize on an object-level cluster against the reference model's
    findNodesThatFit + prioritizeNodes, sorted as selectHost sorts; a schedule_batch afterwards
    gives what it gives without the call."""
    from kubernetes_amd import workload
    from kubernetes_amd.scheduler import FakeMinionLister, FakePodLister, FakeServiceLister, GPUScheduler, SplitMix64Rand
    from oracle import ref_model as R

    rng = workload._SM(4242)
    nodes = workload.make_nodes(60, rng)
    pods = workload.make_pods(90, rng, n_apps=5, port_frac=0.3, pd_frac=0.0, sel_frac=0.25)
    services = workload.make_services(5)
    config = workload.config4() if policy == "config4" else workload.config_default()
    for n in nodes:
        n.spec.capacity["cpu"] = n.spec.capacity["cpu"].__class__.from_milli(1500)
    existing, probe, later = pods[:40], pods[40:70], pods[70:]
    names = sorted(n.metadata.name for n in nodes)
    import copy

    from kubernetes_amd.api import PodStatus

    placed = []
    for i, p in enumerate(existing):
        q = copy.copy(p)
        q.status = PodStatus(host=names[(i * 7) % len(names)])
        placed.append(q)
    minions = FakeMinionLister(nodes)
    top = 5

    # the reference model
    lister = R.PodLister(list(placed))
    preds, prios = R.from_config(config, nodes, lister, R.ServiceLister(services))
    want = []
    for p in probe:
        filtered, _ = R.find_nodes_that_fit(p, lister, preds, list(nodes))
        plist = R.prioritize_nodes(p, lister, prios, filtered)
        srt = sorted(plist, key=lambda hs: (hs[1], hs[0].encode()), reverse=True)
        want.append(srt[:top])
    assert any(len(w) == top for w in want) and any(w and R.get_best_hosts(w) != [w[0][0]] for w in want)

    def run(with_call):
        gpu = GPUScheduler(config, FakePodLister(list(placed)), FakeServiceLister(services), SplitMix64Rand(3))
        try:
            got = gpu.prioritize(probe, minions, top=top) if with_call else None
            return got, gpu.schedule_batch(later, minions, 77)
        finally:
            gpu.close()

    got, after = run(True)
    _, plain = run(False)
    assert got == want
    assert after == plain
    gpu = GPUScheduler(config, FakePodLister([]), FakeServiceLister(services), SplitMix64Rand(3))
    try:
        none = gpu.prioritize(probe[:2], FakeMinionLister([]), top=top)
        assert len(none) == 2 and all(type(e).__name__ == "NoMinionsError" for e in none)
    finally:
        gpu.close()
