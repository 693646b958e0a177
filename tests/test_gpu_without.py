"""ksg_explain_without on the GPU: FitError reports against the state with a suffix of an
ordered list of committed pods taken away. The inputs and references are
tests/without_cases.py's, which tests/test_without_inputs.py shows not to be vacuous: the
sequential scheduler's begin(want_fail) rows of a batch's NOFIT pods (the state as of pod i),
and scenarios whose reference really removes the list's tail, on the C restatement and on a
twin device context. Shapes stay within 1,000 nodes x 233 pods."""
import copy
import os
import socket

import numpy as np
import pytest

from kubernetes_amd import abi
from kubernetes_amd.engine import DeviceScheduler, KsgError, PodBatch
from tests import explain_cases as X
from tests import without_cases as W

pytestmark = pytest.mark.gpu

NODE_COUNTS = (63, 64, 65, X.TILE + 1, 1000)


def _bincount(codes):
    if len(codes) == 0:
        return np.zeros((0, abi.EXPLAIN_SLOTS), np.uint32)
    return np.stack([np.bincount(r, minlength=abi.EXPLAIN_SLOTS) for r in codes]).astype(np.uint32)


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def _check_rows(got, want_codes, want_err, nn):
    codes, hist, err = got
    assert codes.shape == want_codes.shape
    bad = np.argwhere(codes != want_codes)
    assert bad.size == 0, f"first mismatches (pod, node) {bad[:6].tolist()}: {codes[tuple(bad[0])]} vs {want_codes[tuple(bad[0])]}"
    assert np.array_equal(err, want_err)
    assert np.array_equal(hist, _bincount(codes) * (1 - err[:, None].astype(np.uint32)))
    assert (hist.sum(axis=1) == nn * (1 - err.astype(np.int64))).all()  # a row sums to nn (an error row to 0)


# ---- the state as of pod i of a batch ---------------------------------------------------------
_ASOF = {}


def _asof_result(policy, nn):
    """One context per (policy, node count): the one-batch input through ksg_schedule_batch, then
    ksg_explain_without over its NOFIT pods in every form the parity test compares."""
    if (policy, nn) in _ASOF:
        return _ASOF[policy, nn]
    bc = W.batch_case(policy, nn)
    dev = DeviceScheduler(bc.cfg, device=0)
    try:
        dev.set_cluster(bc.case.view.arrays)
        out, state = dev.batch(bc.batch, W.SEED)
        na = len(bc.placed_uids)
        r = dict(out=out.copy(), state=state,
                 asof=dev.explain_without(bc.sub, bc.placed_uids, bc.positions),
                 nocodes=dev.explain_without(bc.sub, bc.placed_uids, bc.positions, want_codes=False),
                 plain=dev.explain(bc.sub),
                 at_end=dev.explain_without(bc.sub, bc.placed_uids, np.full(len(bc.sub), na, np.uint32)),
                 no_list=dev.explain_without(bc.sub, [], np.zeros(len(bc.sub), np.uint32)),
                 again=dev.explain_without(bc.sub, bc.placed_uids, bc.positions),
                 ms=dev.last_explain_without_ms())
    finally:
        dev.close()
    _ASOF[policy, nn] = r
    return r


@pytest.mark.parametrize("nn", NODE_COUNTS)
@pytest.mark.parametrize("policy", W.BATCH_POLICIES)
def test_as_of_parity(policy, nn):
    bc = W.batch_case(policy, nn)
    r = _asof_result(policy, nn)
    assert np.array_equal(r["out"], bc.out) and r["state"] == bc.state
    _check_rows(r["asof"], bc.rows, np.zeros(len(bc.sub), np.uint8), nn)
    c0, h0, e0 = r["nocodes"]  # codes == NULL
    assert c0 is None and np.array_equal(h0, r["asof"][1]) and np.array_equal(e0, r["asof"][2])
    assert _same(r["at_end"], r["plain"]) and _same(r["no_list"], r["plain"])  # nothing taken away: ksg_explain_batch
    assert _same(r["again"], r["asof"])
    assert r["ms"] > 0 or len(bc.sub) == 0


def test_as_of_differs_from_explain_batch():
    """The rows ksg_explain_batch gives after the batch are NOT the sequential ones on these
    inputs (tests/test_without_inputs.py): the parity above is not ksg_explain_batch's."""
    bc = W.batch_case("config4", 65)
    r = _asof_result("config4", 65)
    assert (r["plain"][0] != bc.rows).any() and not (r["asof"][0] != bc.rows).any()


def test_as_of_against_device_begin_commit():
    """The device's own ksg_schedule_begin(fail_codes) / ksg_schedule_commit pod by pod, on a
    second context with the same draws."""
    from kubernetes_amd import workload

    policy, nn = "config4", X.TILE + 1
    bc = W.batch_case(policy, nn)
    r = _asof_result(policy, nn)
    dev = DeviceScheduler(bc.cfg, device=0)
    try:
        dev.set_cluster(bc.case.view.arrays)
        rng = workload._SM(W.SEED)
        rows, out = [], []
        for i in range(len(bc.batch)):
            rc, _, k, fails = dev.begin(bc.batch, i, want_fail=True)
            if rc == abi.KSG_OK:
                out.append(dev.commit((rng.next() >> 1) % k))
            else:
                assert rc == abi.KSG_NOFIT
                out.append(-1)
                rows.append(fails.copy())
    finally:
        dev.close()
    assert np.array_equal(out, bc.out)
    assert np.array_equal(np.stack(rows), r["asof"][0])


# ---- general suffixes: scenarios against a twin oracle and a twin device context ------------------
def _run_scenario(sc, want_codes=True):
    dev, twin = DeviceScheduler(sc.cfg, device=0), DeviceScheduler(sc.cfg, device=0)
    try:
        sc.load(dev)
        got = dev.explain_without(sc.probe, sc.absent, sc.positions)
        nocodes = dev.explain_without(sc.probe, sc.absent, sc.positions, want_codes=False)
        tcodes, terr = W.scenario_reference(sc, twin)  # ksg_remove_pod + ksg_evaluate
    finally:
        dev.close()
        twin.close()
    wcodes, werr = W.oracle_reference(sc)
    _check_rows(got, wcodes, werr, sc.nn)
    assert np.array_equal(tcodes, wcodes) and np.array_equal(terr, werr)
    assert nocodes[0] is None and np.array_equal(nocodes[1], got[1]) and np.array_equal(nocodes[2], got[2])
    return got


@pytest.mark.parametrize("k", X.POD_COUNTS)
@pytest.mark.parametrize("policy,nn", [("config2", 65), ("config4", X.TILE + 1), ("presence", 63)])
def test_random_suffixes(policy, nn, k):
    sc = W.random_scenario(policy, nn, k)
    codes, _, _ = _run_scenario(sc)
    assert len(codes) == k


def test_positions_move_the_rows():
    """The same pods at position 0 and at n_absent: the latter is ksg_explain_batch's report,
    the former differs from it on these inputs."""
    sc = W.random_scenario("config4", X.TILE + 1, 1)
    probe = X.xcase("config4", X.TILE + 1).probe
    m, na = len(probe), len(sc.absent)
    dev = DeviceScheduler(sc.cfg, device=0)
    try:
        sc.load(dev)
        twice = PodBatch(np.concatenate([probe.pods, probe.pods]), probe.ids)
        codes, _, _ = dev.explain_without(twice, sc.absent, [0] * m + [na] * m)
        plain = dev.explain(probe)[0]
    finally:
        dev.close()
    assert np.array_equal(codes[m:], plain) and (codes[:m] != plain).any()


@pytest.mark.parametrize("name", sorted(W.HANDMADE))
def test_handmade(name):
    _run_scenario(W.handmade(name))


@pytest.mark.parametrize("plain_probe", [False, True], ids=["ext", "ext-null"])
def test_extensions(plain_probe):
    """Listed pods carry extended-resource requests; codes 8 and 9 appear and move with the
    position (the `ext` form), and the ext == NULL form skips the extension filters."""
    nn = X.TILE + 1
    sc = W.ext_scenario(nn, plain_probe)
    codes, _, err = _run_scenario(sc)
    assert not err.any()
    m = len(sc.probe) // 3
    first, last = codes[:m], codes[m:2 * m]  # every probe pod at position 0, then at n_absent
    assert (first != last).any()
    if plain_probe:
        assert not np.isin(codes, (abi.FAIL_TAINTS, abi.FAIL_SCALAR)).any()
    else:
        for code in (abi.FAIL_TAINTS, abi.FAIL_SCALAR):
            assert (codes == code).any()
            assert ((first == code) != (last == code)).any(), code  # the code moves with the position


def test_chunking(monkeypatch):
    """A staging budget of CHUNK pods' codes (then of 5 pods'): three or more launches at 65
    nodes, first_absent and the peer override offset per chunk; rows identical to one chunk's."""
    policy, nn = "config4", 65
    bc = W.batch_case(policy, nn)
    one = _asof_result(policy, nn)["asof"]
    assert len(bc.sub) >= 3 * X.CHUNK
    for stage in (nn * X.CHUNK, nn * 5):
        monkeypatch.setenv("KSG_EXPLAIN_WITHOUT_STAGE_BYTES", str(stage))
        dev = DeviceScheduler(bc.cfg, device=0)
        try:
            dev.set_cluster(bc.case.view.arrays)
            out, _ = dev.batch(bc.batch, W.SEED)
            got = dev.explain_without(bc.sub, bc.placed_uids, bc.positions)
            nocodes = dev.explain_without(bc.sub, bc.placed_uids, bc.positions, want_codes=False)
        finally:
            dev.close()
        assert np.array_equal(out, bc.out)
        assert _same(got, one), stage
        assert np.array_equal(nocodes[1], one[1])
    sc = W.handmade("peers")  # the peer override across chunks of one pod
    monkeypatch.setenv("KSG_EXPLAIN_WITHOUT_STAGE_BYTES", "1")
    _run_scenario(sc)


@pytest.mark.parametrize("window", [128, 0])
@pytest.mark.parametrize("ext", [False, True], ids=["plain", "extensions"])
def test_no_side_effects(ext, window):
    """A batch run in chunks with explain_without calls in between that list committed pods:
    placements, the final generator state and the committed totals equal the C restatement's
    uninterrupted run, and a ksg_batch_unwind right after an explain_without still undoes."""
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
        got, state, windows, placed = [], 4321, 0, []
        other = sub(n_run, n_run + n_other)
        for lo in range(0, n_run, chunk):
            o, state = dev.batch(sub(lo, lo + chunk), state)
            got.append(o)
            windows += dev.last_batch_windows()
            placed += b.pods["uid"][lo:lo + chunk][o >= 0].tolist()
            pos = np.arange(n_other) * len(placed) // n_other
            dev.explain_without(other, placed, pos)                                  # every committed pod listed
            newest = placed[::-1][:50]
            dev.explain_without(other, newest, pos % (len(newest) + 1), want_codes=False)  # the last 50, newest first
            dev.explain_without(sub(0, lo + chunk), placed, np.zeros(lo + chunk, np.uint32), want_codes=False)
        got = np.concatenate(got)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"first mismatches at {bad[:8]}: {got[bad[:8]]} vs {want[bad[:8]]}"
        assert state == want_state
        for a, w_ in zip(dev.read_requested(), orc.read_requested()):
            assert np.array_equal(a, w_)
        if ext:
            assert np.array_equal(dev.read_ext_used(), orc.read_ext_used())
        assert (windows > 0) == (window > 0)  # the calls did not move the batches off their path
        # one more batch, an explain_without over it, then pod k's Bind is rejected
        last = sub(n_run, n_run + n_other)
        o, st = dev.batch(last, state)
        w1, s1 = orc.batch(last, state)
        assert np.array_equal(o, w1) and (o >= 0).sum() >= 2
        k = int(np.flatnonzero(o >= 0)[(o >= 0).sum() // 2])
        uids = b.pods["uid"][n_run:n_run + n_other][o >= 0]
        dev.explain_without(last, uids, np.zeros(n_other, np.uint32))
        kept, _ = dev.batch_unwind(last, o, k, rng_state=st)
        assert kept == int(np.count_nonzero(o[: k + 1] >= 0))
        for i in np.flatnonzero(o[k:] >= 0) + k:  # the oracle undoes the same commits
            orc.remove_pod(int(last.pods["uid"][i]))
        for a, w_ in zip(dev.read_requested(), orc.read_requested()):
            assert np.array_equal(a, w_)
        with pytest.raises(KsgError):  # an unwound uid is no longer committed
            dev.explain_without(last, uids, np.zeros(n_other, np.uint32))
    finally:
        dev.close()
        orc.close()


# ---- arguments ------------------------------------------------------------------------------
def _raw(dev, batch, uids, fa, n=None, n_absent=None, codes=None, hist=None, err=None, ext=None):
    """The C entry point itself, for its return code."""
    pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
    ids = np.ascontiguousarray(batch.ids if len(batch.ids) else np.zeros(1, np.uint32), dtype=np.uint32)
    u = None if uids is None else np.ascontiguousarray(uids, np.uint64)
    f = None if fa is None else np.ascontiguousarray(fa, np.uint32)
    return dev._lib.ksg_explain_without(dev._ctx, abi.ptr(pods), abi.ptr(ext), len(batch) if n is None else n,
                                        abi.ptr(ids), len(batch.ids), abi.ptr(u),
                                        (0 if u is None else len(u)) if n_absent is None else n_absent, abi.ptr(f),
                                        abi.ptr(codes), abi.ptr(hist), abi.ptr(err))


def test_arguments():
    case = X.xcase("config2", 65)
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        out, _ = case.load(dev)
        nn, probe = case.nn, PodBatch(case.probe.pods[:4], case.probe.ids)
        uids = case.fill.pods["uid"][out >= 0][:6].astype(np.uint64)
        free_uid = int(case.fill.pods["uid"][out < 0][0]) if (out < 0).any() else 10 ** 9
        fa = np.array([0, 3, 6, 6], np.uint32)

        def bufs():
            return (np.full((4, nn), 0xAB, np.uint8), np.full((4, abi.EXPLAIN_SLOTS), 0xABABABAB, np.uint32),
                    np.full(4, 0xAB, np.uint8))

        def untouched(b):
            return (b[0] == 0xAB).all() and (b[1] == 0xABABABAB).all() and (b[2] == 0xAB).all()

        def call(u, f, **kw):
            b = bufs()
            rc = _raw(dev, probe, u, f, codes=b[0], hist=b[1], err=b[2], **kw)
            return rc, b

        rc, b = call(uids, fa)
        assert rc == abi.KSG_OK and _same(b, dev.explain_without(probe, uids, fa))
        # n == 0: KSG_OK, nothing written
        rc, b = call(uids, fa, n=0)
        assert rc == abi.KSG_OK and untouched(b)
        assert _raw(dev, probe, None, None, n=0) == abi.KSG_OK
        c0, h0, e0 = dev.explain_without(PodBatch(probe.pods[:0], probe.ids), uids, [])
        assert c0.shape == (0, nn) and h0.shape == (0, abi.EXPLAIN_SLOTS) and e0.shape == (0,)
        # hist / err are required once there is a pod
        b = bufs()
        assert _raw(dev, probe, uids, fa, hist=None, err=b[2]) == abi.KSG_ERR_ARG
        assert _raw(dev, probe, uids, fa, hist=b[1], err=None) == abi.KSG_ERR_ARG
        # the new KSG_ERR_ARG cases, nothing written
        bad = [(np.concatenate([uids[:3], [free_uid], uids[3:]]).astype(np.uint64), fa),  # not a committed uid
               (np.array([10 ** 12], np.uint64), np.zeros(4, np.uint32)),
               (np.concatenate([uids, uids[:1]]), fa),                                   # the same uid twice
               (uids, np.array([0, 3, 7, 6], np.uint32))]                                # first_absent > n_absent
        for u, f in bad:
            rc, b = call(u, f)
            assert rc == abi.KSG_ERR_ARG and untouched(b)
        rc, b = call(None, fa, n_absent=6)  # NULL list with n_absent > 0
        assert rc == abi.KSG_ERR_ARG and untouched(b)
        rc, b = call(uids, None)            # NULL first_absent with n_absent > 0
        assert rc == abi.KSG_ERR_ARG and untouched(b)
        rc, b = call(None, None)            # n_absent == 0: both may be NULL
        assert rc == abi.KSG_OK and _same(b, dev.explain(probe))
        # ext on a context without extensions
        rc, b = call(uids, fa, ext=np.zeros(4, abi.POD_EXT_DTYPE))
        assert rc == abi.KSG_ERR_STATE and untouched(b)
        # a pending begin: KSG_ERR_STATE, and the begin is still committable afterwards
        fit = int(np.argmax(dev.explain(case.probe, want_codes=False)[1][:, 0] > 0))
        rc, _, ties, _ = dev.begin(case.probe, fit)
        assert rc == abi.KSG_OK and ties > 0
        rc, b = call(uids, fa)
        assert rc == abi.KSG_ERR_STATE and untouched(b)
        node = dev.commit(0)
        assert 0 <= node < nn
        rc, b = call(uids, fa)
        assert rc == abi.KSG_OK
        # no nodes
        a = case.view.arrays
        dev.set_cluster(type(a)(a.nodes[:0], a.node_pairs[:0], a.pair_keys, a.n_services))
        rc, b = call(None, None)
        assert rc == abi.KSG_NONODES and untouched(b)
    finally:
        dev.close()


# ---- a node-sharded context answers for the whole cluster on every rank ---------------------------
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
        bc = W.batch_case(policy, nn)
        dev = DeviceScheduler(bc.cfg, device=0, rank=rank, world=world, allgather=gloo_allgather())
        dev.set_cluster(bc.case.view.arrays)
        out, _ = dev.batch(bc.batch, W.SEED)  # (collective)
        res = dev.explain_without(bc.sub, bc.placed_uids, bc.positions)  # (no exchange: each rank on its own)
        lo, hi = dev.shard()
        dev.close()
        q.put((rank, out.copy(), res, lo, hi, None))
    except Exception as e:  # report instead of hanging the parent
        import traceback

        q.put((rank, None, None, None, None, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_sharded_ranks_answer_for_the_whole_cluster():
    import torch.multiprocessing as mp

    policy, nn, world = "config4", 1000, 2
    bc = W.batch_case(policy, nn)
    single = _asof_result(policy, nn)
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
    assert [r[5] for r in res] == [None] * world, [r[5] for r in res]
    assert res[0][3] == 0 and res[0][4] == res[1][3] and 0 < res[1][3] < nn and res[1][4] == nn  # two real shards
    for rank, out, got, lo, hi, _ in res:
        assert np.array_equal(out, bc.out)
        assert _same(got, single["asof"])
    assert np.array_equal(single["asof"][0], bc.rows)


# ---- GPUScheduler.schedule_batch(explain="as_of") ------------------------------------------------
def test_scheduler_level():
    """Every error of schedule_batch(explain="as_of") equals the one a second GPUScheduler raises
    when the same pods go through schedule() one at a time with the same random source; one
    explain_without call, no evaluate; explain=True still reports against the state after the batch."""
    from kubernetes_amd.api import PodStatus
    from kubernetes_amd.scheduler import (FakeMinionLister, FakePodLister, FakeServiceLister, FitError, GPUScheduler,
                                          SplitMix64Rand)
    from tests.test_oracle_crosscheck import _workload

    w = _workload("config2", 20, 80, tight=True)
    minions = FakeMinionLister(w.nodes)
    seed = 91

    def fresh():
        lister = FakePodLister([])
        return lister, GPUScheduler(w.config, lister, FakeServiceLister(w.services), SplitMix64Rand(seed))

    # the sequential run: schedule() pod by pod, AssumePod reported back by the lister
    lister, seq = fresh()
    want_hosts, want_errors = [], []
    try:
        for p in w.pods:
            try:
                h = seq.schedule(p, minions)
                q = copy.copy(p)
                q.status = PodStatus(host=h)
                lister.pods.append(q)
                want_hosts.append(h)
                want_errors.append(None)
            except FitError as e:
                want_hosts.append(None)
                want_errors.append(e)
        end_state = seq.random.state
    finally:
        seq.close()
    # the parent's behaviour: explain=True reports against the state after the batch, the map
    # Schedule(pod) raises right afterwards (tests/test_gpu_explain.py::test_scheduler_level)
    lister_t, plain = fresh()
    try:
        hosts_t, state_t, errors_t = plain.schedule_batch(w.pods, minions, seed, explain=True)
        for p, h in zip(w.pods, hosts_t):
            if h is not None:
                q = copy.copy(p)
                q.status = PodStatus(host=h)
                lister_t.pods.append(q)
        for p, h, e in zip(w.pods, hosts_t, errors_t):
            if h is None:
                with pytest.raises(FitError) as ei:
                    plain.schedule(p, minions)
                assert e.failed_predicates == ei.value.failed_predicates
    finally:
        plain.close()
    _, gpu = fresh()
    calls, plain_calls = [], []
    real = gpu.engine.explain_without
    gpu.engine.explain_without = lambda *a, **k: calls.append(1) or real(*a, **k)
    real_plain = gpu.engine.explain
    gpu.engine.explain = lambda *a, **k: plain_calls.append(1) or real_plain(*a, **k)
    gpu.engine.evaluate = None  # (the report does not go pod by pod)
    try:
        hosts, state, errors = gpu.schedule_batch(w.pods, minions, seed, explain="as_of")
        assert len(calls) == 1 and not plain_calls
        with pytest.raises(ValueError):
            gpu.schedule_batch(w.pods, minions, seed, explain="as-of")
    finally:
        gpu.close()
    assert hosts == want_hosts == hosts_t and state == end_state == state_t
    assert any(h is None for h in hosts) and any(h is not None for h in hosts)
    for p, h, e, we in zip(w.pods, hosts, errors, want_errors):
        if h is not None:
            assert e is None
            continue
        assert isinstance(e, FitError) and e.pod is p
        assert e.failed_predicates == we.failed_predicates and str(e) == str(we)
        assert sum(e.counts.values()) == len(e.failed_predicates)
        for name, cnt in e.counts.items():
            assert cnt == sum(1 for s in e.failed_predicates.values() if name in s)
