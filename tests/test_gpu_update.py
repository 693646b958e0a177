"""ksg_update_cluster on the device: a new node list under the same pods.

The specification (include/kschedgpu.h): after the call, every word ksg_read_requested,
ksg_read_state and ksg_read_ext_used return and every later call's result are what a fresh context
gives after ksg_set_cluster with the new arrays, ksg_set_node_ext, and ksg_add_pod of every live
pod in its original order on its renamed host. The expected state is tests/state_model.StateModel
over the renamed live list, the expected behaviour a fresh oracle.pyoracle.OracleScheduler built
that way; neither knows the call. The cases (tests/update_cases.py) are keyed by host names."""
import os
import socket

import numpy as np
import pytest

from kubernetes_amd import abi, workload
from kubernetes_amd.engine import DeviceScheduler, KsgError
from oracle.pyoracle import OracleScheduler
from tests import update_cases as uc
from tests.state_model import diff_states, engine_state

pytestmark = pytest.mark.gpu


def _audit(dev, case, live, step, what):
    d = diff_states(engine_state(dev, case.n_scalar), case.model(live, step).arrays())
    assert d is None, (case.name, case.policy, what, d)


def _update(dev, case, step):
    o2n, out = case.maps(step)
    dev.update_cluster(case.arrays[step + 1], o2n, out, node_ext=case.node_ext(step + 1))
    assert dev.n_nodes == case.n_nodes(step + 1)
    assert dev.last_update_ms() >= 0.0


def _remove(dev, orc, live, uid):
    dev.remove_pod(uid)
    orc.remove_pod(uid)
    live[:] = [l for l in live if l.rec.uid != uid]


def _after(dev, case, live, step, lo):
    """Everything the specification promises after the update to list `step`, in lockstep with the
    fresh oracle; the state is audited after every operation. Pool pods [lo, lo + AFTER] are used."""
    orc = case.rebuild(OracleScheduler(case.cfg), live, step)
    try:
        n = case.n_nodes(step)
        b = case.slice(step, lo, lo + uc.AFTER)
        got, rng_g = dev.batch(b, 4242)
        want, rng_w = orc.batch(b, 4242)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (case.name, step, "batch", bad[:8], got[bad[:8]], want[bad[:8]])
        assert rng_g == rng_w
        placed = [i for i, x in enumerate(got) if x >= 0]
        for i in placed:
            live.append(case.pool_live(step, lo + i, int(got[i])))
        _audit(dev, case, live, step, "batch after the update")
        i = lo + uc.AFTER
        try:
            g = dev.begin(case.pool[step], i)[:3]
        except KsgError as e:
            g = (e.code, 0, 0)
        try:
            w = orc.begin(case.pool[step], i)[:3]
        except RuntimeError as e:
            assert "rc=-5" in str(e)
            w = (abi.KSG_ERR_NOPEER, 0, 0)
        assert g == w, (case.name, step, "begin")
        if g[0] == abi.KSG_OK:
            node = dev.commit(g[2] // 2)
            assert node == orc.commit(g[2] // 2)
            live.append(case.pool_live(step, i, node))
        _audit(dev, case, live, step, "begin / commit after the update")
        # a pod committed before the update (the first holder of a shared key: the bit stays) and one after
        first = uc.HAND_UID + case.second_holder
        if any(l.rec.uid == first for l in live):
            _remove(dev, orc, live, first)
        if placed:
            _remove(dev, orc, live, uc.POOL_UID + lo + placed[-1])
        _audit(dev, case, live, step, "remove_pod after the update")
        if n == 0:
            return
        q = case.slice(step, lo + uc.AFTER + 1, lo + uc.AFTER + 9)
        codes, _, err = dev.explain(q)
        for j in range(len(q)):
            rc, fails, _ = orc.evaluate(q, j)
            assert (rc == abi.KSG_ERR_NOPEER) == bool(err[j]), (case.name, step, "explain err", j)
            if rc == abi.KSG_OK:
                assert np.array_equal(codes[j], fails), (case.name, step, "explain", j)
        dev.prioritize(q, top=4)
        dev.headroom(q, 8)
        gone = np.asarray([l.rec.uid for l in live[:6]], np.uint64)
        dev.explain_without(q, gone, np.zeros(len(q), np.uint32))
        _audit(dev, case, live, step, "read-only queries after the update")
    finally:
        orc.close()


def _run(case, window, make_dev=None):
    dev = make_dev(case.cfg) if make_dev else DeviceScheduler(case.cfg, device=0)
    try:
        dev.set_window(window)
        case.load(dev)
        live, _ = case.fill(dev)
        _audit(dev, case, live, 0, "fill")
        for step in range(case.steps):
            _update(dev, case, step)
            _audit(dev, case, live, step + 1, f"update {step}")
            _after(dev, case, live, step + 1, uc.FILL + 1 + step * (uc.AFTER + 10))
    finally:
        dev.close()


@pytest.mark.parametrize("serve", [None, "0"])
@pytest.mark.parametrize("window", [0, 128])
@pytest.mark.parametrize("name", uc.CASES)
def test_update_default_policy(name, window, serve, monkeypatch):
    """State and behaviour, every case (churn runs on into its inverse: two updates in a row,
    back to the model at the original list; empty_out_in goes through an empty list)."""
    if serve is not None:
        monkeypatch.setenv("KSG_SERVE", serve)
    _run(uc.UpdateCase(name), window)


@pytest.mark.parametrize("debug", [0, 2048])
@pytest.mark.parametrize("name", uc.CASES)
def test_update_config4(name, debug, monkeypatch):
    """ServiceAffinity + ServiceAntiAffinity: the domains and the re-rank map are recomputed
    (KSG_DEBUG 2048: without the re-rank map)."""
    if debug:
        monkeypatch.setenv("KSG_DEBUG", str(debug))
    _run(uc.UpdateCase(name, "config4"), 128)


@pytest.mark.parametrize("name", ["shrink", "churn"])
def test_update_config4_exact_path(name):
    _run(uc.UpdateCase(name, "config4"), 0)


@pytest.mark.parametrize("name", uc.CASES)
def test_update_service_affinity(name):
    """A peer whose host left the list: KSG_ERR_NOPEER from begin, as for the oracle."""
    _run(uc.UpdateCase(name, "affinity"), 128)


@pytest.mark.parametrize("window", [0, 128])
@pytest.mark.parametrize("name", ["shrink", "grow", "churn"])
def test_update_every_extension(name, window):
    """scalar_used moves with the nodes, the new list's taints and allocatables apply."""
    _run(uc.UpdateCase(name, ext=True), window)


def test_unwind_across_the_update():
    """Batch, update, ksg_batch_unwind of that batch at a middle placed pod (its out_nodes hold
    the old list's ranks), re-batch: state and placements equal the model's and the oracle's."""
    case = uc.UpdateCase("shrink")
    dev = DeviceScheduler(case.cfg, device=0)
    orc0, orc1 = OracleScheduler(case.cfg), OracleScheduler(case.cfg)
    try:
        dev.set_window(128)
        hand = case.hand_live()
        for s in (case.load(dev), case.load(orc0)):
            for l in hand:
                s.add_pod(case.host_id(0, l.host), case.hand, l.idx)
        b0 = case.slice(0, 0, uc.FILL)
        out, rng = dev.batch(b0, workload.TIEBREAK_SEED)
        placed = [i for i, x in enumerate(out) if x >= 0]
        k = placed[len(placed) // 2]
        want0, rng_k = orc0.batch(case.slice(0, 0, k + 1), workload.TIEBREAK_SEED)
        assert np.array_equal(out[:k + 1], want0)
        live = hand + [case.pool_live(0, i, int(out[i])) for i in placed]
        _update(dev, case, 0)
        _audit(dev, case, live, 1, "update")
        kept, rng_back = dev.batch_unwind(b0, out, k, rng_state=rng)
        assert kept == len([i for i in placed if i <= k]) and rng_back == rng_k
        live = [l for l in live if l.kind == "hand" or l.idx < k]
        _audit(dev, case, live, 1, "unwind")
        case.rebuild(orc1, live, 1)
        b1 = case.slice(1, k + 1, uc.FILL)
        got, rng_g = dev.batch(b1, rng_back)
        want, rng_w = orc1.batch(b1, rng_k)
        assert np.array_equal(got, want) and rng_g == rng_w
        live += [case.pool_live(1, k + 1 + i, int(x)) for i, x in enumerate(got) if x >= 0]
        _audit(dev, case, live, 1, "re-batch")
    finally:
        dev.close()
        orc0.close()
        orc1.close()


# ---- refusals: nothing changes, the old list stays in force ------------------------------------
def _raw(dev, arrays, o2n, oo, on, ext=None, null_map=False):
    nodes = np.ascontiguousarray(arrays.nodes, dtype=abi.NODE_DTYPE)
    np_ = np.ascontiguousarray(arrays.node_pairs if len(arrays.node_pairs) else np.zeros(1), np.uint32)
    pk = np.ascontiguousarray(arrays.pair_keys, np.uint32)
    o2n, oo, on = (np.ascontiguousarray(a, np.uint32) for a in (o2n, oo, on))
    return dev._lib.ksg_update_cluster(dev._ctx, abi.ptr(nodes), len(nodes), abi.ptr(np_), len(arrays.node_pairs),
                                       abi.ptr(pk), len(pk), None if null_map else abi.ptr(o2n),
                                       abi.ptr(oo) if len(oo) else None, abi.ptr(on) if len(on) else None, len(oo),
                                       None if ext is None else ext)


def _ext_struct(arrs, keep):
    cap, toff, tn, ti = arrs
    cap = np.ascontiguousarray(cap, np.int64).reshape(-1)
    toff, tn = np.ascontiguousarray(toff, np.uint32), np.ascontiguousarray(tn, np.uint32)
    ti = np.ascontiguousarray(ti if len(ti) else np.zeros(1), np.uint32)
    keep += [cap, toff, tn, ti]
    import ctypes as C
    e = abi.KsgNodeExtArrays(cap.ctypes.data, toff.ctypes.data, tn.ctypes.data, ti.ctypes.data, len(arrs[3]))
    keep.append(e)
    return C.byref(e)


def _still_old(dev, case, live, before, what, step=0):
    d = diff_states(engine_state(dev, case.n_scalar), before)
    assert d is None, (what, d)
    assert dev.n_nodes == case.n_nodes(step)


def _old_list_in_force(dev, case, live, step=0, lo=uc.FILL + 1):
    """A following small batch (pool pods [lo, lo + 20)) is exactly the oracle's on the OLD list,
    list `step` (its pods join `live`)."""
    orc = case.rebuild(OracleScheduler(case.cfg), live, step)
    try:
        b = case.slice(step, lo, lo + 20)
        got, want = dev.batch(b, 99), orc.batch(b, 99)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
        live += [case.pool_live(step, lo + i, int(x)) for i, x in enumerate(got[0]) if x >= 0]
        _audit(dev, case, live, step, "batch on the old list")
    finally:
        orc.close()


def test_refused_calls_change_nothing():
    import copy

    case = uc.UpdateCase("shrink")
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        new = case.arrays[1]
        o2n, out = case.maps(0)  # (before any pod: GHOST gets its number below)
        assert _raw(dev, new, o2n, [], []) == abi.KSG_ERR_STATE  # before the first ksg_set_cluster
        dev.set_window(128)
        case.load(dev)
        live, _ = case.fill(dev)
        o2n, out = case.maps(0)
        oo, on = [a for a, _ in out], [b for _, b in out]
        assert oo, "the case has a pod on an outside host"
        before = engine_state(dev, 0)
        bad = copy.copy(new)
        bad.node_pairs = new.node_pairs.copy()
        bad.node_pairs[0] = 10 ** 6
        bad2 = copy.copy(new)
        bad2.nodes = new.nodes.copy()
        bad2.nodes[3]["n_labels"] = 10 ** 6
        twice = o2n.copy()
        twice[1] = twice[0]
        huge = copy.copy(new)  # one node more than a shard holds (KSG_R_MAX x KSG_NT = 131,072), no labels
        huge.nodes = np.zeros(128 * 1024 + 1, abi.NODE_DTYPE)
        keep = []
        calls = {
            "invalid pair id": (abi.KSG_ERR_ARG, lambda: _raw(dev, bad, o2n, oo, on)),
            "label range": (abi.KSG_ERR_ARG, lambda: _raw(dev, bad2, o2n, oo, on)),
            "old_to_new NULL": (abi.KSG_ERR_ARG, lambda: _raw(dev, new, o2n, oo, on, null_map=True)),
            "outside host not listed": (abi.KSG_ERR_ARG, lambda: _raw(dev, new, o2n, [], [])),
            "outside_old below n_nodes": (abi.KSG_ERR_ARG, lambda: _raw(dev, new, o2n, oo + [5], on + [10 ** 6])),
            "outside_old repeated": (abi.KSG_ERR_ARG, lambda: _raw(dev, new, o2n, oo + oo[:1], on + [10 ** 6])),
            "new id repeated": (abi.KSG_ERR_ARG, lambda: _raw(dev, new, twice, oo, on)),
            "new id repeated (outside)": (abi.KSG_ERR_ARG, lambda: _raw(dev, new, o2n, oo + [10 ** 6], on + [int(o2n[0])])),
            "shard size": (abi.KSG_ERR_CAPACITY, lambda: _raw(dev, huge, o2n, oo, on)),
            "ext without extensions": (abi.KSG_ERR_STATE, lambda: _raw(
                dev, new, o2n, oo, on, ext=_ext_struct((np.zeros(1), np.zeros(65), np.zeros(65), np.zeros(1)), keep))),
        }
        for what, (code, call) in calls.items():
            assert call() == code, what
            _still_old(dev, case, live, before, what)
        rc, ties = uc.begin_rc(dev, case.pool[0], uc.FILL + 30)
        assert rc == abi.KSG_OK
        assert _raw(dev, new, o2n, oo, on) == abi.KSG_ERR_STATE  # a ksg_schedule_begin is pending
        live.append(case.pool_live(0, uc.FILL + 30, dev.commit(0)))
        _audit(dev, case, live, 0, "commit after the refused update")
        _old_list_in_force(dev, case, live)
    finally:
        dev.close()


def test_refused_updated_refused_reset_in_one_context():
    """One context's node list through every way it changes hands, in a row: a refusal after the
    new list's parts were being built ("shard size": the old parts come back), the same update with
    good arguments (the old parts go), a second such refusal on the new list, then ksg_set_cluster
    of the original list with the pods added again. After each step the device state is the
    model's and a 20-pod batch the oracle's."""
    import copy

    case = uc.UpdateCase("shrink")
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        dev.set_window(128)
        case.load(dev)
        live, _ = case.fill(dev)
        o2n, out = case.maps(0)
        oo, on = [a for a, _ in out], [b for _, b in out]
        huge = copy.copy(case.arrays[1])  # one node more than a shard holds, no labels
        huge.nodes = np.zeros(128 * 1024 + 1, abi.NODE_DTYPE)
        before = engine_state(dev, 0)
        assert _raw(dev, huge, o2n, oo, on) == abi.KSG_ERR_CAPACITY
        _still_old(dev, case, live, before, "shard size, list 0")
        _old_list_in_force(dev, case, live)
        _update(dev, case, 0)
        _audit(dev, case, live, 1, "update")
        _old_list_in_force(dev, case, live, 1, uc.FILL + 21)
        # the way back to list 0, by names, with the oversized node array again
        back = np.asarray([case.host_id(0, nm) for nm in case.names[1]], np.uint32)
        outside = [nm for nm in list(case.it.ext_hosts) if nm not in case.ranks[1]]
        assert any(l.host in outside for l in live), "a pod is on a host outside list 1"
        before = engine_state(dev, 0)
        assert _raw(dev, huge, back, [case.host_id(1, nm) for nm in outside],
                    [case.host_id(0, nm) for nm in outside]) == abi.KSG_ERR_CAPACITY
        _still_old(dev, case, live, before, "shard size, list 1", 1)
        _old_list_in_force(dev, case, live, 1, uc.FILL + 41)
        case.rebuild(dev, live, 0)
        _audit(dev, case, live, 0, "set_cluster of list 0 and the pods again")
        _old_list_in_force(dev, case, live, 0, uc.FILL + 61)
    finally:
        dev.close()


def test_refused_on_a_diverged_context(monkeypatch):
    case = uc.UpdateCase("churn")
    monkeypatch.setenv("KSG_DEBUG", "16384")  # the next window batch fails after its device work
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        dev.set_window(128)
        case.load(dev)
        monkeypatch.delenv("KSG_DEBUG")
        with pytest.raises(KsgError, match="injected"):
            dev.batch(case.slice(0, 0, 50), 5)
        o2n, out = case.maps(0)
        with pytest.raises(KsgError, match="ksg_set_cluster") as ei:
            dev.update_cluster(case.arrays[1], o2n, out)
        assert ei.value.code == abi.KSG_ERR_STATE
    finally:
        dev.close()


def test_refused_extension_arguments():
    case = uc.UpdateCase("shrink", ext=True)
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        dev.set_window(0)
        case.load(dev)
        live, _ = case.fill(dev)
        o2n, out = case.maps(0)
        oo, on = [a for a, _ in out], [b for _, b in out]
        before = engine_state(dev, case.n_scalar)
        cap, toff, tn, ti = case.node_ext(1)
        assert len(ti) > 0
        keep = []
        far = toff.copy()
        far[np.nonzero(tn)[0][0]] = len(ti) + 7
        big = ti.copy()
        big[0] = int(case.ext.kcfg.max_taints)
        for what, code, ext in (("ext NULL", abi.KSG_ERR_ARG, None),
                                ("taint list out of range", abi.KSG_ERR_ARG, _ext_struct((cap, far, tn, ti), keep)),
                                ("taint id past max_taints", abi.KSG_ERR_CAPACITY, _ext_struct((cap, toff, tn, big), keep))):
            assert _raw(dev, case.arrays[1], o2n, oo, on, ext=ext) == code, what
            _still_old(dev, case, live, before, what)
        _old_list_in_force(dev, case, live)
        _update(dev, case, 0)  # and the same arguments with a good `ext` go through
        _audit(dev, case, live, 1, "update")
    finally:
        dev.close()


def test_refused_capacity_max_domains():
    """config4 with max_domains = the zones there are: a new list with one more zone value is
    refused (KSG_ERR_CAPACITY) and the old list stays in force."""
    import copy

    from kubernetes_amd import ingest

    case = uc.UpdateCase("shrink", "config4", max_domains=8)
    dev = DeviceScheduler(case.cfg, device=0)
    try:
        dev.set_window(128)
        case.load(dev)
        live, _ = case.fill(dev)
        before = engine_state(dev, 0)
        nodes = [copy.deepcopy(n) for n in case.views[1].nodes]
        nodes[4].metadata.labels["zone"] = "z99"
        wide = ingest.ClusterView(nodes, case.services, case.it)
        o2n, out = case.maps(0)
        with pytest.raises(KsgError, match="max_domains") as ei:
            dev.update_cluster(wide.arrays, o2n, out)
        assert ei.value.code == abi.KSG_ERR_CAPACITY
        _still_old(dev, case, live, before, "max_domains")
        _old_list_in_force(dev, case, live)
    finally:
        dev.close()


# ---- the score path: never narrower than the fresh context's ------------------------------------
def test_joining_host_with_a_negative_request_takes_the_fresh_contexts_path():
    """A pod with a negative request on an outside host does not widen the context (ksg_add_pod
    looks at node hosts only). When that host joins the list, the fresh context of the
    specification re-adds the pod on a node and turns to the int64 kernels (no windows); the
    updated context must do the same, with the same placements. No node total is negative here, so
    only the request itself can be the cause."""
    case = uc.UpdateCase("churn", join_negative=True)
    dev, fresh = DeviceScheduler(case.cfg, device=0), DeviceScheduler(case.cfg, device=0)
    orc = OracleScheduler(case.cfg)
    try:
        dev.set_window(128)
        fresh.set_window(128)
        case.load(dev)
        live, _ = case.fill(dev)
        assert dev.last_batch_stats()["windows"] > 0  # (int32 window path so far)
        _update(dev, case, 0)
        _audit(dev, case, live, 1, "update")
        case.rebuild(fresh, live, 1)
        case.rebuild(orc, live, 1)
        b = case.slice(1, uc.FILL + 1, uc.FILL + 1 + uc.AFTER)
        got, want, ref = dev.batch(b, 4242), fresh.batch(b, 4242), orc.batch(b, 4242)
        assert np.array_equal(got[0], ref[0]) and got[1] == ref[1]
        assert np.array_equal(want[0], ref[0]) and want[1] == ref[1]
        assert fresh.last_batch_stats()["windows"] == 0  # the fresh context is on the int64 kernels ...
        assert dev.last_batch_stats()["windows"] == 0    # ... and so is the updated one
    finally:
        dev.close()
        fresh.close()
        orc.close()


# ---- static terms past the config's slots -------------------------------------------------------
def test_static_terms_end_with_the_update_and_apply_again():
    """A policy past the config's LabelsPresence / LabelPreference slots (ksg_add_static_config
    passes). After the update the extra terms are gone: the context evaluates like the restatement
    with the config's slots alone. After the passes are applied again, the batch equals the
    object-level reference's (oracle/ref_model, which takes any number of terms) on the new list."""
    import copy

    from kubernetes_amd import ingest
    from kubernetes_amd.api import PodStatus
    from kubernetes_amd.engine import PodBatch
    from kubernetes_amd.scheduler import SplitMix64Rand
    from oracle import ref_model as R
    from tests.test_oracle_crosscheck import _workload

    w = _workload("policy_many_labels", 130, 230, False, 0)
    it = ingest.Interner()
    for k in w.config.label_keys():
        it.key_id(k)
    lists = [list(w.nodes), list(w.nodes)[0:130:2]]
    views = [ingest.ClusterView(l, w.services, it) for l in lists]
    cfg = w.config.compile(it.key_id)
    aff = w.config.affinity_labels()
    pool = [ingest.ingest_pods(v, w.pods, uids=list(range(1, len(w.pods) + 1)), aff_labels=aff) for v in views]
    cut = lambda b, lo, hi: PodBatch(b.pods[lo:hi].copy(), b.ids)
    lister, rnd = R.PodLister([]), SplitMix64Rand(91)

    def ref_run(nodes, pods):
        preds, prios = R.from_config(w.config, nodes, lister, R.ServiceLister(w.services))
        ref = R.GenericScheduler(preds, prios, lister, rnd)
        out = []
        for p in pods:
            try:
                h = ref.schedule(p, nodes)
            except (R.FitError, KeyError):
                out.append(None)
                continue
            out.append(h)
            q = copy.copy(p)
            q.status = PodStatus(host=h)
            lister.pods.append(q)
        return out

    def passes(dev):
        n = 0
        for extra in w.config.static_passes(it.key_id):
            dev.add_static_config(extra)
            n += 1
        return n

    named = lambda out, v: [v.names[x] if x >= 0 else None for x in out]
    dev = DeviceScheduler(cfg, device=0)
    orc = OracleScheduler(cfg)
    try:
        dev.set_window(128)
        dev.set_cluster(views[0].arrays)
        assert passes(dev) >= 1
        want0 = ref_run(lists[0], w.pods[:100])
        got0, st0 = dev.batch(cut(pool[0], 0, 100), 91)
        assert named(got0, views[0]) == want0 and st0 == rnd.state and any(want0)
        dev.update_cluster(views[1].arrays, *views[1].host_map(views[0]))
        # the static terms ended with the old list: the config's own slots are all that is left
        orc.set_cluster(views[1].arrays)
        for i, h in enumerate(want0):
            if h is not None:
                orc.add_pod(views[1].host_id(h), pool[1], i)
        probe = range(200, 208)
        bare = []
        for i in probe:
            (_, fg, sg), (_, fo, so) = dev.evaluate(pool[1], i), orc.evaluate(pool[1], i)
            assert np.array_equal(fg, fo) and np.array_equal(sg[fg == 0], so[fo == 0]), i
            bare.append((fg.copy(), sg.copy()))
        assert passes(dev) >= 1
        again = [dev.evaluate(pool[1], i)[1:] for i in probe]
        assert any(not (np.array_equal(f0, f1) and np.array_equal(s0[f0 == 0], s1[f1 == 0]))
                   for (f0, s0), (f1, s1) in zip(bare, again)), "the extra terms change no probe pod's row"
        want1 = ref_run(lists[1], w.pods[100:200])
        got1, st1 = dev.batch(cut(pool[1], 100, 200), st0)
        assert named(got1, views[1]) == want1 and st1 == rnd.state and any(want1)
    finally:
        dev.close()
        orc.close()


# ---- sharded contexts ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shrink", "grow"])
def test_update_rccl_one_rank(name):
    """The exchange path over a 1-rank RCCL communicator (tests/test_gpu_sharded.py::_rccl_ctx)."""
    _run(uc.UpdateCase(name), 128,
         make_dev=lambda cfg: DeviceScheduler(cfg, device=0, rank=0, world=1, nccl_id=DeviceScheduler.nccl_unique_id()))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, q):
    import torch.distributed as dist

    from kubernetes_amd.engine import gloo_allgather

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        case = uc.UpdateCase("shrink")
        dev = DeviceScheduler(case.cfg, device=0, rank=rank, world=world, allgather=gloo_allgather())
        dev.set_window(128)
        case.load(dev)
        live, _ = case.fill(dev, with_begin=False)
        fill_hosts = [(l.kind, l.idx, l.host) for l in live]
        _update(dev, case, 0)
        d = diff_states(engine_state(dev, 0), case.model(live, 1).arrays())
        got, rng = dev.batch(case.slice(1, uc.FILL + 1, uc.FILL + 1 + uc.AFTER), 4242)
        lo, hi = dev.shard()
        dev.close()
        q.put((rank, fill_hosts, d, got.tolist(), rng, (lo, hi), None))
    except Exception as e:  # report instead of hanging the parent
        import traceback

        q.put((rank, None, None, None, None, None, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_update_two_ranks_gloo():
    """130 -> 65 nodes, window 128, two ranks over gloo: both make the update (replicated node
    state, recomputed shard ranges) and their placements equal the oracle's."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(2):
            res.append(q.get(timeout=110))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    res.sort(key=lambda r: r[0])
    for r in res:
        assert r[6] is None, r[6]
    case = uc.UpdateCase("shrink")
    orc0 = case.load(OracleScheduler(case.cfg))
    live, _ = case.fill(orc0, with_begin=False)
    orc0.close()
    orc = case.rebuild(OracleScheduler(case.cfg), live, 1)
    want, rng = orc.batch(case.slice(1, uc.FILL + 1, uc.FILL + 1 + uc.AFTER), 4242)
    orc.close()
    from kubernetes_amd.engine import shard_range

    for r in res:  # the new list's shard ranges
        assert tuple(r[5]) == tuple(shard_range(case.n_nodes(1), r[0], 2)), r[5]
    assert res[0][5][0] == 0 and res[1][5][1] == case.n_nodes(1) and res[0][5][1] == res[1][5][0]
    for r in res:
        assert r[1] == [(l.kind, l.idx, l.host) for l in live]
        assert r[2] is None, r[2]
        assert r[3] == want.tolist() and r[4] == rng


# ---- the scheduler: GPUScheduler(incremental_nodes=True) -----------------------------------------
def _scheduler_run(w, incremental, modeler):
    """w.pods through schedule() with three node-list changes in between (a node leaves, it
    rejoins, a node is relabelled), against oracle.ref_model with the same random source.
    -> (hosts, the scheduler's PodMirror stats or None)."""
    import copy

    from kubernetes_amd.api import PodStatus
    from kubernetes_amd.modeler import SimpleModeler, StoreToPodLister
    from kubernetes_amd.scheduler import (FakeMinionLister, FakePodLister, FakeServiceLister, FitError, GPUScheduler,
                                          SchedulingError, SplitMix64Rand)
    from oracle import ref_model as R

    nodes = list(w.nodes)
    relabelled = copy.deepcopy(nodes[5])
    relabelled.metadata.labels["zone"] = "z-moved"
    lists = {len(w.pods) // 4: nodes[:2] + nodes[3:], len(w.pods) // 2: list(nodes),
             3 * len(w.pods) // 4: nodes[:5] + [relabelled] + nodes[6:]}
    rnd_ref, rnd_gpu = SplitMix64Rand(77), SplitMix64Rand(77)
    if modeler:
        sched_store = StoreToPodLister()
        for p in w.existing:
            sched_store.store.add(p)
        m = SimpleModeler(StoreToPodLister(), sched_store)
        lister_ref = lister_gpu = m.pod_lister()
        report = lambda q: m.assume_pod(q)
    else:
        lister_ref, lister_gpu = R.PodLister(list(w.existing)), FakePodLister(list(w.existing))

        def report(q):
            lister_ref.pods.append(q)
            lister_gpu.pods.append(q)

    def new_ref():
        preds, prios = R.from_config(w.config, nodes, lister_ref, R.ServiceLister(w.services))
        return R.GenericScheduler(preds, prios, lister_ref, rnd_ref)

    ref = new_ref()
    gpu = GPUScheduler(w.config, lister_gpu, FakeServiceLister(w.services), rnd_gpu, incremental_nodes=incremental)
    hosts = []
    try:
        for i, p in enumerate(w.pods):
            if i in lists:
                nodes = lists[i]
                ref = new_ref()
            minions = FakeMinionLister(nodes)
            try:
                want = ref.schedule(p, nodes)
            except R.FitError as e:
                with pytest.raises(FitError) as ei:
                    gpu.schedule(p, minions)
                assert set(ei.value.failed_predicates) == set(e.failed_predicates)
                hosts.append(None)
                continue
            except KeyError:  # ServiceAffinity's peer is on a host that is not a node
                with pytest.raises(SchedulingError):
                    gpu.schedule(p, minions)
                hosts.append("error")
                continue
            assert gpu.schedule(p, minions) == want, i
            hosts.append(want)
            q = copy.copy(p)
            q.spec = copy.copy(p.spec)
            q.spec.host = want
            q.status = PodStatus(host=want)
            report(q)
        assert rnd_gpu.state == rnd_ref.state
        return hosts, (dict(gpu._events.stats) if gpu._events is not None else None)
    finally:
        gpu.close()


@pytest.mark.parametrize("name,nn,npods,tight,existing", [("config2", 60, 120, False, 10), ("config4", 48, 100, True, 12),
                                                         ("policy_many_labels", 90, 100, False, 8)])
def test_scheduler_incremental_nodes(name, nn, npods, tight, existing):
    """Same hosts and FitError maps as the reference model across a leave, a join and a relabel;
    on the modeler path one reload (the first list) and three rehosts; the flag off gives the
    same hosts. policy_many_labels: the static passes are applied again after each update."""
    from tests.test_oracle_crosscheck import _workload

    for modeler in (True, False):
        on, st_on = _scheduler_run(_workload(name, nn, npods, tight, existing), True, modeler)
        off, st_off = _scheduler_run(_workload(name, nn, npods, tight, existing), False, modeler)
        assert on == off and any(h not in (None, "error") for h in on)
        if modeler:
            assert st_on["reloads"] == 1 and st_on["rehosts"] == 3
            assert st_off["reloads"] == 4 and st_off["rehosts"] == 0
