"""ksg_preempt_batch on the GPU: per pending pod and node the committed pods that would have to
leave, and the node to preempt on. The inputs and the reference are tests/preempt_cases.py's,
which tests/test_preempt_inputs.py shows not to be vacuous: the reference really removes the
candidates, evaluates, and adds them back one by one, on the C restatement and on a twin device
context. Shapes stay within 1,000 nodes x 233 pods.

ksg_preempt_batch refuses a configuration with a ServiceAffinity predicate (KSG_ERR_STATE), so the
(config4, TILE + 1) random scenario checks the refusal; (config2, TILE + 1) covers more than one
node tile instead."""
import os
import socket

import numpy as np
import pytest

from kubernetes_amd import abi
from kubernetes_amd.engine import DeviceScheduler, KsgError, PodBatch
from tests import explain_cases as X
from tests import preempt_cases as P
from tests import without_cases as W

pytestmark = pytest.mark.gpu

NAMES = ("best_node", "n_victims", "victims", "cand_count", "free_count", "node_victims")


def _assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        if g is None or w is None:
            assert g is None and w is None, name
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what} {name}: first mismatches at {bad[:6].tolist()}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"


def _run(sc, max_victims=P.MAX_VICTIMS):
    """The call with and without node_victims on a fresh context, against the oracle reference."""
    dev = DeviceScheduler(sc.cfg, device=0)
    try:
        sc.load(dev)
        got = dev.preempt(sc.probe, sc.absent, sc.positions, max_victims=max_victims, want_per_node=True)
        ms = dev.last_preempt_ms()
        lean = dev.preempt(sc.probe, sc.absent, sc.positions, max_victims=max_victims)
        again = dev.preempt(sc.probe, sc.absent, sc.positions, max_victims=max_victims, want_per_node=True)
    finally:
        dev.close()
    want = P.oracle_reference(sc, max_victims).outputs()
    _assert_same(got, want, sc.name)
    _assert_same(lean[:5], want[:5], sc.name)
    assert lean[5] is None
    _assert_same(again, got, sc.name)
    assert ms > 0
    return got


# ---- parity with the reference ----------------------------------------------------------------
@pytest.mark.parametrize("name", P.ALL_HANDMADE)
def test_handmade(name):
    _run(P.handmade(name))


@pytest.mark.parametrize("k", X.POD_COUNTS)
@pytest.mark.parametrize("policy,nn", [("config2", 65), ("config4", X.TILE + 1), ("presence", 63), ("config2", X.TILE + 1)])
def test_random_scenarios(policy, nn, k):
    sc = W.random_scenario(policy, nn, k)
    if policy == "config4":  # ServiceAffinity: refused, nothing computed
        dev = DeviceScheduler(sc.cfg, device=0)
        try:
            sc.load(dev)
            with pytest.raises(KsgError) as ei:
                dev.preempt(sc.probe, sc.absent, sc.positions)
            assert ei.value.code == abi.KSG_ERR_STATE and "ServiceAffinity" in str(ei.value)
        finally:
            dev.close()
        return
    got = _run(sc)
    assert len(got[0]) == k


@pytest.mark.parametrize("plain_probe", [False, True], ids=["ext", "ext-null"])
def test_extensions(plain_probe):
    """Listed pods carry extended-resource requests and sit on tainted nodes; the ext == NULL
    form skips the extension filters."""
    sc = W.ext_scenario(X.TILE + 1, plain_probe)
    got = _run(sc)
    nv = got[5]
    assert ((nv != P.NOFIT) & (nv > 0)).any()


def test_reference_on_the_device_itself():
    """The same walk with ksg_remove_pod / ksg_evaluate / ksg_add_pod on a second context."""
    sc = W.random_scenario("config2", 65, X.CHUNK)
    twin = DeviceScheduler(sc.cfg, device=0)
    try:
        ref = P.reference(sc, twin)
        # the twin is back in the loaded state: the call on it gives the same answer
        after = twin.preempt(sc.probe, sc.absent, sc.positions, want_per_node=True)
    finally:
        twin.close()
    want = P.oracle_reference(sc).outputs()
    _assert_same(ref.outputs(), want, "twin walk")
    _assert_same(after, want, "twin call")


# ---- invariants ----------------------------------------------------------------------------------
@pytest.mark.parametrize("policy,nn", [("config2", X.TILE + 1), ("presence", 63)])
def test_counts_are_the_explain_calls(policy, nn):
    """cand_count is ksg_explain_without's hist[:, 0] and free_count ksg_explain_batch's, on the
    same context; the candidates are the nodes with code 0."""
    sc = W.random_scenario(policy, nn, X.CHUNK + 1)
    dev = DeviceScheduler(sc.cfg, device=0)
    try:
        sc.load(dev)
        _, _, _, cand, free, nv = dev.preempt(sc.probe, sc.absent, sc.positions, want_per_node=True)
        codes, hist_w, _ = dev.explain_without(sc.probe, sc.absent, sc.positions)
        _, hist_x, _ = dev.explain(sc.probe, want_codes=False)
    finally:
        dev.close()
    assert np.array_equal(cand, hist_w[:, 0]) and np.array_equal(free, hist_x[:, 0])
    assert np.array_equal(nv != P.NOFIT, codes == 0)


def test_positions_at_the_end_evict_nothing():
    """first_absent == n_absent for every pod, and an empty list: the highest-rank fitting node,
    no victim."""
    sc = W.random_scenario("config2", X.TILE + 1, X.CHUNK + 1)
    n, na = len(sc.probe), len(sc.absent)
    dev = DeviceScheduler(sc.cfg, device=0)
    try:
        sc.load(dev)
        end = dev.preempt(sc.probe, sc.absent, np.full(n, na, np.uint32), want_per_node=True)
        empty = dev.preempt(sc.probe, [], np.zeros(n, np.uint32), want_per_node=True)
        codes, _, _ = dev.explain(sc.probe)
    finally:
        dev.close()
    fits = codes == 0
    want_best = np.array([np.flatnonzero(r)[-1] if r.any() else -1 for r in fits], np.int32)
    assert (want_best >= 0).any() and (want_best < 0).any()
    for got in (end, empty):
        best, nv, victims, cand, free, per_node = got
        assert np.array_equal(best, want_best) and not nv.any() and (victims == P.PAD).all()
        assert np.array_equal(cand, fits.sum(axis=1)) and np.array_equal(free, cand)
        assert np.array_equal(per_node, np.where(fits, 0, P.NOFIT).astype(np.uint32))


@pytest.mark.parametrize("max_victims", [0, 1, abi.PREEMPT_MAX_VICTIMS])
def test_truncation(max_victims):
    """The long row against max_victims 0, 1 and the cap: n_victims stays the true count."""
    sc = P.handmade("long-row")
    best, nv, victims, _, _, _ = _run(sc, max_victims)
    assert nv[0] == P.LONG - 1 and victims.shape == (1, max_victims)
    assert victims[0].tolist() == (list(range(1, P.LONG)) + [P.PAD] * max_victims)[:max_victims]


def test_chunking(monkeypatch):
    """A staging budget of CHUNK pods (then of 5 pods): four or more launches, first_absent, the
    partials and the outputs offset per chunk; the result is the unchunked one."""
    base = W.random_scenario("config2", 65, X.CHUNK + 1)
    reps = 3
    idx = list(range(len(base.probe))) * reps
    sc = W.Scenario("chunked", base.cfg, base.load, base.absent, PodBatch(base.probe.pods[idx], base.probe.ids),
                    np.tile(base.positions, reps), base.nn)
    want = tuple(np.concatenate([a] * reps) for a in P.oracle_reference(base).outputs())
    tiles = -(-((base.nn + 63) // 64) // (X.TILE // 64))
    for per_node in (True, False):
        bpp = tiles * 24 + (base.nn * 4 if per_node else 0)
        for stage in (None, bpp * X.CHUNK, bpp * 5):
            if stage is None:
                monkeypatch.delenv("KSG_PREEMPT_STAGE_BYTES", raising=False)
            else:
                monkeypatch.setenv("KSG_PREEMPT_STAGE_BYTES", str(stage))
            dev = DeviceScheduler(sc.cfg, device=0)
            try:
                sc.load(dev)
                got = dev.preempt(sc.probe, sc.absent, sc.positions, want_per_node=per_node)
            finally:
                dev.close()
            _assert_same(got[:5], want[:5], f"stage {stage}")
            if per_node:
                _assert_same(got[5:], want[5:], f"stage {stage}")


# ---- no side effects -------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [128, 0])
@pytest.mark.parametrize("ext", [False, True], ids=["plain", "extensions"])
def test_no_side_effects(ext, window):
    """A batch run in chunks with preempt calls in between that list committed pods: placements,
    the final generator state, the committed totals and the pod state equal a second context's
    that makes no such call."""
    from tests.ext_cases import ExtCase
    from tests.helpers import Case

    nn, n_run, n_other, chunk = 300, 300, 40, 100
    c = ExtCase("config2", nn, n_run + n_other, w_taint=0, w_bal=0) if ext else Case("config2", nn, n_run + n_other)
    b = c.batch

    def sub(lo, hi):
        return PodBatch(b.pods[lo:hi], b.ids, None if b.ext is None else b.ext[lo:hi])

    plain, dev = DeviceScheduler(c.cfg, device=0), DeviceScheduler(c.cfg, device=0)
    try:
        for eng in (plain, dev):
            c.load(eng) if ext else eng.set_cluster(c.view.arrays)
            eng.set_window(window)
        other = sub(n_run, n_run + n_other)
        state_p = state_d = 4321
        placed, windows = [], 0
        for lo in range(0, n_run, chunk):
            o_p, state_p = plain.batch(sub(lo, lo + chunk), state_p)
            o_d, state_d = dev.batch(sub(lo, lo + chunk), state_d)
            windows += dev.last_batch_windows()
            assert np.array_equal(o_p, o_d) and state_p == state_d
            placed += b.pods["uid"][lo:lo + chunk][o_d >= 0].tolist()
            pos = np.arange(n_other) * len(placed) // n_other
            dev.preempt(other, placed, pos, want_per_node=True)     # every committed pod listed
            newest = placed[::-1][:50]
            dev.preempt(other, newest, pos % (len(newest) + 1))     # the last 50, newest first
            dev.preempt(sub(0, lo + chunk), placed, np.zeros(lo + chunk, np.uint32), max_victims=0)
        for a, w_ in zip(dev.read_requested(), plain.read_requested()):
            assert np.array_equal(a, w_)
        st_d, st_p = dev.read_state(), plain.read_state()
        assert sorted(st_d) == sorted(st_p) and all(np.array_equal(st_d[k], st_p[k]) for k in st_d)
        if ext:
            assert np.array_equal(dev.read_ext_used(), plain.read_ext_used())
        assert (windows > 0) == (window > 0)  # the calls did not move the batches off their path
        # a following batch with the same seed
        o_p, s_p = plain.batch(other, state_p)
        o_d, s_d = dev.batch(other, state_d)
        assert np.array_equal(o_p, o_d) and s_p == s_d and (o_d >= 0).any()
        # every listed uid is still committed: removing one works exactly once
        dev.remove_pod(int(placed[0]))
        with pytest.raises(KsgError):
            dev.preempt(other, placed, np.zeros(n_other, np.uint32))
    finally:
        dev.close()
        plain.close()


# ---- arguments ------------------------------------------------------------------------------------
SENT = 0xABABABAB


def _raw(dev, batch, uids, fa, n=None, n_absent=None, max_victims=4, ext=None, skip=(), nn=None):
    """The C entry point itself on sentinel-filled outputs. -> (rc, outputs untouched?)"""
    pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
    ids = np.ascontiguousarray(batch.ids if len(batch.ids) else np.zeros(1, np.uint32), dtype=np.uint32)
    u = None if uids is None else np.ascontiguousarray(uids, np.uint64)
    f = None if fa is None else np.ascontiguousarray(fa, np.uint32)
    m = len(batch)
    bufs = {"best": np.full(m, -77, np.int32), "nv": np.full(m, SENT, np.uint32),
            "victims": np.full((m, max(max_victims, 1)), SENT, np.uint32), "cand": np.full(m, SENT, np.uint32),
            "free": np.full(m, SENT, np.uint32), "per_node": np.full((m, max(nn or dev.n_nodes, 1)), SENT, np.uint32)}
    arg = {k: (None if k in skip else abi.ptr(v)) for k, v in bufs.items()}
    rc = dev._lib.ksg_preempt_batch(dev._ctx, abi.ptr(pods), abi.ptr(ext), m if n is None else n, abi.ptr(ids),
                                    len(batch.ids), abi.ptr(u), (0 if u is None else len(u)) if n_absent is None else n_absent,
                                    abi.ptr(f), max_victims, arg["best"], arg["nv"], arg["victims"], arg["cand"],
                                    arg["free"], arg["per_node"])
    untouched = (bufs["best"] == -77).all() and all((bufs[k] == SENT).all() for k in bufs if k != "best")
    return rc, untouched


def test_arguments():
    case = X.xcase("config2", 65)
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        out, _ = case.load(dev)
        probe = PodBatch(case.probe.pods[:4], case.probe.ids)
        uids = case.fill.pods["uid"][out >= 0][:6].astype(np.uint64)
        free_uid = int(case.fill.pods["uid"][out < 0][0]) if (out < 0).any() else 10 ** 9
        fa = np.array([0, 3, 6, 6], np.uint32)
        rc, untouched = _raw(dev, probe, uids, fa)
        assert rc == abi.KSG_OK and not untouched
        # n == 0: KSG_OK, nothing written
        assert _raw(dev, probe, uids, fa, n=0) == (abi.KSG_OK, True)
        res = dev.preempt(PodBatch(probe.pods[:0], probe.ids), uids, [], want_per_node=True)
        assert [a.shape for a in res] == [(0,), (0,), (0, P.MAX_VICTIMS), (0,), (0,), (0, case.nn)]
        # a required array is missing
        for k in ("best", "nv", "cand", "free", "victims"):
            assert _raw(dev, probe, uids, fa, skip=(k,)) == (abi.KSG_ERR_ARG, True), k
        assert _raw(dev, probe, uids, fa, skip=("victims",), max_victims=0)[0] == abi.KSG_OK  # NULL iff 0
        assert _raw(dev, probe, uids, fa, skip=("per_node",))[0] == abi.KSG_OK                # optional
        # max_victims over the cap
        assert _raw(dev, probe, uids, fa, max_victims=abi.PREEMPT_MAX_VICTIMS + 1) == (abi.KSG_ERR_ARG, True)
        assert _raw(dev, probe, uids, fa, max_victims=abi.PREEMPT_MAX_VICTIMS)[0] == abi.KSG_OK
        # the list
        bad = [(np.concatenate([uids[:3], [free_uid], uids[3:]]).astype(np.uint64), fa),  # not a committed uid
               (np.array([10 ** 12], np.uint64), np.zeros(4, np.uint32)),
               (np.concatenate([uids, uids[:1]]), fa),                                   # the same uid twice
               (uids, np.array([0, 3, 7, 6], np.uint32))]                                # first_absent > n_absent
        for u, f in bad:
            assert _raw(dev, probe, u, f) == (abi.KSG_ERR_ARG, True)
        assert _raw(dev, probe, None, fa, n_absent=6) == (abi.KSG_ERR_ARG, True)  # NULL list with n_absent > 0
        assert _raw(dev, probe, uids, None) == (abi.KSG_ERR_ARG, True)            # NULL first_absent with n_absent > 0
        assert _raw(dev, probe, None, None)[0] == abi.KSG_OK                       # n_absent == 0: both may be NULL
        # ext on a context without extensions
        assert _raw(dev, probe, uids, fa, ext=np.zeros(4, abi.POD_EXT_DTYPE)) == (abi.KSG_ERR_STATE, True)
        # a pending begin: KSG_ERR_STATE, and the begin is still committable afterwards
        fit = int(np.argmax(dev.explain(case.probe, want_codes=False)[1][:, 0] > 0))
        rc, _, ties, _ = dev.begin(case.probe, fit)
        assert rc == abi.KSG_OK and ties > 0
        assert _raw(dev, probe, uids, fa) == (abi.KSG_ERR_STATE, True)
        assert 0 <= dev.commit(0) < case.nn
        assert _raw(dev, probe, uids, fa)[0] == abi.KSG_OK
        # no nodes
        a = case.view.arrays
        dev.set_cluster(type(a)(a.nodes[:0], a.node_pairs[:0], a.pair_keys, a.n_services))
        assert _raw(dev, probe, None, None, nn=case.nn) == (abi.KSG_NONODES, True)
    finally:
        dev.close()


def test_service_affinity_is_refused():
    """tests/test_affinity_trap.py's configuration: KSG_ERR_STATE, a reason, nothing written;
    ksg_explain_without still answers there."""
    sc = W.handmade("peers")
    assert sc.cfg.predicates & abi.PRED_SERVICEAFFINITY
    dev = DeviceScheduler(sc.cfg, device=0)
    try:
        sc.load(dev)
        assert _raw(dev, sc.probe, sc.absent, sc.positions) == (abi.KSG_ERR_STATE, True)
        with pytest.raises(KsgError) as ei:
            dev.preempt(sc.probe, sc.absent, sc.positions)
        assert ei.value.code == abi.KSG_ERR_STATE and "ServiceAffinity" in str(ei.value)
        codes, _, _ = dev.explain_without(sc.probe, sc.absent, sc.positions)
        assert codes.shape == (len(sc.probe), sc.nn)
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
        sc = W.random_scenario(policy, nn, X.CHUNK + 1)
        dev = DeviceScheduler(sc.cfg, device=0, rank=rank, world=world, allgather=gloo_allgather())
        out, _ = sc.load(dev)  # (set_cluster and the fill batch: collective)
        res = dev.preempt(sc.probe, sc.absent, sc.positions, want_per_node=True)  # (no exchange: each rank on its own)
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

    policy, nn, world = "config2", 1000, 2
    sc = W.random_scenario(policy, nn, X.CHUNK + 1)
    single = _run(sc)
    nv = single[5]
    assert ((nv != P.NOFIT) & (nv > 0)).any() and (nv == P.NOFIT).any()
    fill_out = W.batch_fill_out(policy, nn)
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
        assert np.array_equal(out, fill_out)
        _assert_same(got, single, f"rank {rank}")


# ---- GPUScheduler.preempt ---------------------------------------------------------------------------
def test_scheduler_level():
    """The three kinds of result on a small cluster, and nothing committed or removed."""
    from kubernetes_amd import workload
    from kubernetes_amd.api import make_node
    from kubernetes_amd.scheduler import FakeMinionLister, FakePodLister, FitError, GPUScheduler, NoMinionsError

    def pod(name, host="", cpu=0, prio=0):
        return W._hpod(name, host, cpu, labels={"prio": str(prio)})

    nodes = [make_node("n1", 1000, 8 * W.GI), make_node("n2", 1000, 8 * W.GI)]
    running = [pod("high", "n2", 900, prio=10), pod("low-a", "n1", 450, prio=1), pod("low-b", "n1", 450, prio=2)]
    pending = [pod("small", cpu=50, prio=5), pod("mid", cpu=500, prio=5), pod("huge", cpu=5000, prio=5),
               pod("boss", cpu=1000, prio=20), pod("meek", cpu=500, prio=0)]
    gpu = GPUScheduler(workload.config_default(), FakePodLister(running))
    try:
        minions = FakeMinionLister(nodes)
        prio = lambda p: int(p.metadata.labels["prio"])
        res = gpu.preempt(pending, minions, prio)
        before = [a.copy() for a in gpu.engine.read_requested()]
        assert res[0] is None                                                    # fits as things stand
        assert res[1] == {"host": "n1", "victims": ["ns/low-a"], "n_victims": 1}  # low-b (2) goes back first and stays
        assert isinstance(res[2], FitError) and res[2].pod is pending[2]          # too large for any node
        assert res[2].failed_predicates == {"n1": {"PodFitsResources"}, "n2": {"PodFitsResources"}}
        assert res[2].counts == {"PodFitsResources": 2}
        # both nodes are candidates; n2's victim (high, index 0) is more important than n1's (low-b, index 1)
        assert res[3] == {"host": "n1", "victims": ["ns/low-b", "ns/low-a"], "n_victims": 2}
        assert isinstance(res[4], FitError)  # may evict nobody: the error is against the state as it stands
        assert res[4].failed_predicates == {"n1": {"PodFitsResources"}, "n2": {"PodFitsResources"}}
        assert gpu.preempt(pending, minions, prio, max_victims=1)[3] == {"host": "n1", "victims": ["ns/low-b"], "n_victims": 2}
        # nothing was committed or removed: the totals stand, and the answer repeats
        for a, w_ in zip(gpu.engine.read_requested(), before):
            assert np.array_equal(a, w_)
        assert before[0].tolist() == [900, 900]
        again = gpu.preempt(pending, minions, prio)
        assert again[:2] == res[:2] and again[3] == res[3]
        assert gpu.preempt([], minions, prio) == []
        none = gpu.preempt(pending, FakeMinionLister([]), prio)
        assert len(none) == len(pending) and all(isinstance(e, NoMinionsError) for e in none)
    finally:
        gpu.close()
