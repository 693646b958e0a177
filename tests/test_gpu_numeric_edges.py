"""The device's restatements of calculateScore and of the float32 spreading terms at
their numeric edges (tests/numeric_edges.py), against an independent plain-Python
reference and against the C oracle. Everything compared is an integer and every
comparison is exact.

  A  per-node fail codes and scores (ksg_evaluate) and (rc, max score, tie count, fail
     codes) of ksg_schedule_begin on 130-node clusters at the edges of lr_calc, lr_win and
     lr_fast, under four policies, through the scan kernel, the block server and the grid
     server
  B  batches whose commits carry a node's LeastRequested term across a tenth inside a
     window (the resolvers' re-checks, lr_win_nb), on the fused launch and apart, on the
     ServiceAntiAffinity resolvers and under two wave skews
  C  both sides of each bound of the use_window gate; ServiceSpreading and
     ServiceAntiAffinity for every maxCount 1..300; the servers' 1024-entry table edge

The file's 54 cases take about 2 s together on an MI355X (the longest, 0.4 s), so the
ladders run every maxCount step.
"""
import functools

import numpy as np
import pytest

from kubernetes_amd import abi
from kubernetes_amd.engine import DeviceScheduler
from oracle.pyoracle import OracleScheduler
from tests import numeric_edges as ne

pytestmark = pytest.mark.gpu

# how ksg_schedule_begin is served (the environment is read by ksg_create)
MODES = {
    "scan": {"KSG_SERVE": "0"},           # the servers off: the scan kernel
    "block": {"KSG_SERVE_GRID": "0"},     # the one-workgroup resident server
    "grid": {"KSG_SERVE_GRID_MIN": "48"},  # the grid server from 49 nodes on
}


def _device(monkeypatch, mode, cfg):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    return DeviceScheduler(cfg, device=0)


@functools.lru_cache(maxsize=None)
def _edge_expected(kind, policy):
    """The reference's (fail codes, scores, begin) per pending pod, computed once."""
    case = ne.edge_case(kind, policy)
    ref = case.reference()
    return [(ref.evaluate(cpu, mem, 0), ref.begin(cpu, mem, 0)) for cpu, mem in case.requests]


def _same_scores(got_fails, got_scores, fails, scores, where):
    assert got_fails.tolist() == fails, where
    bad = [(n, int(got_scores[n]), s) for n, s in enumerate(scores) if s is not None and int(got_scores[n]) != s]
    assert not bad, (where, bad[:4])


def _same_begin(got, want, where):
    rc, m, k, fails = got
    assert (rc, m if rc == abi.KSG_OK else 0, k) == tuple(want[:3]), (where, (rc, m, k), want[:3])
    assert fails.tolist() == want[3], where


# ---- A ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("policy", ["config1", "default", "big", "huge"])
@pytest.mark.parametrize("kind", ["tame", "wild"])
def test_edge_scores_match_reference_and_oracle(kind, policy, mode, monkeypatch):
    """tame: every LeastRequested term in [0, 10]: the three int32-score policies are served
    by the resident servers (asserted), and the reciprocal's teeth, the 2^49 switch of
    lr_fast and lr_calc's two paths are all reached there. wild: negative capacities,
    capacities past 2^63 / 10, negative totals and requests: combined scores leave int32
    under every policy, so the int64 kernels have to serve the context and the servers
    decline it (asserted). huge: int64 scores by its weights; the servers never take it."""
    case = ne.edge_case(kind, policy)
    expected = _edge_expected(kind, policy)
    dev = case.load(_device(monkeypatch, mode, case.cfg))
    orc = case.load(OracleScheduler(case.cfg))
    served = mode != "scan" and policy != "huge" and kind == "tame"
    st = dev.serve_stats()
    assert st["eligible"] == served and (not served or st["grid"] == (mode == "grid")), st
    if mode == "scan":  # (ksg_evaluate first: it is refused while a begin is pending)
        for i, ((fails, scores), _) in enumerate(expected):
            where = (kind, policy, "evaluate", i, case.requests[i])
            rc, gf, gs = dev.evaluate(case.batch, i)
            ro, of, os_ = orc.evaluate(case.batch, i)
            assert rc == abi.KSG_OK
            _same_scores(of, os_, fails, scores, where + ("oracle",))
            _same_scores(gf, gs, fails, scores, where)
    for i, (_, begin) in enumerate(expected):  # (each begin abandons the one before)
        where = (kind, policy, mode, i, case.requests[i])
        _same_begin(orc.begin(case.batch, i, want_fail=True), begin, where + ("oracle",))
        _same_begin(dev.begin(case.batch, i, want_fail=True), begin, where)
    st = dev.serve_stats()
    assert st["eligible"] == served and (not served or st["requests"] >= len(expected)), st
    if kind == "tame":
        # a negative request on the tame cluster: the term leaves [0, 10] for this pod, on a
        # context the servers were serving a moment ago
        ref = case.reference()
        one = case.batch.one(0)
        for cpu, mem in ne.WILD_REQUESTS[len(ne.TAME_REQUESTS):]:
            one.pods["milli_cpu"][0], one.pods["memory"][0] = cpu, mem
            want = ref.begin(cpu, mem, 0)
            _same_begin(orc.begin(one, 0, want_fail=True), want, (kind, policy, mode, cpu, mem, "oracle"))
            _same_begin(dev.begin(one, 0, want_fail=True), want, (kind, policy, mode, cpu, mem))
        assert not dev.serve_stats()["eligible"]
    dev.close()


# ---- B ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _walk_expected(nn, policy):
    case = ne.walk_case(nn, policy)
    orc = case.load(OracleScheduler(case.cfg))
    want, st = orc.batch(case.batch, 4949)
    wc, wm = orc.read_requested()
    return want.copy(), st, wc.copy(), wm.copy()


def _walk(nn, policy, window):
    case = ne.walk_case(nn, policy)
    want, sw, wc, wm = _walk_expected(nn, policy)
    dev = case.load(DeviceScheduler(case.cfg, device=0))
    dev.set_window(window)
    got, sg = dev.batch(case.batch, 4949)
    windows = dev.last_batch_stats()["windows"]
    gc, gm = dev.read_requested()
    dev.close()
    bad = np.nonzero(got != want)[0]
    where = (nn, policy, window)
    assert bad.size == 0, f"{where}: first mismatches at {bad[:6]}: {got[bad[:6]]} vs {want[bad[:6]]}"
    assert sg == sw, where
    assert np.array_equal(gc, wc) and np.array_equal(gm, wm), where
    assert windows > 0, where  # (a gate that fell back to the exact kernel would hide the window path)


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("policy", ["config1", "default"])
@pytest.mark.parametrize("nn", [64, 130])
def test_commits_across_a_tenth_inside_a_window(nn, policy, fused, monkeypatch):
    monkeypatch.setenv("KSG_FUSED", fused)
    for window in (5, 64, 128):
        _walk(nn, policy, window)


@pytest.mark.parametrize("resolver", ["rerank", "ldsslot"])
def test_commits_across_a_tenth_anti_affinity_resolvers(resolver, monkeypatch):
    """Config 4's policy at 130 nodes: the register-slot re-rank resolver, and with
    KSG_DEBUG & 4096 the LDS-slot one."""
    if resolver == "ldsslot":
        monkeypatch.setenv("KSG_DEBUG", "4096")
    for window in (5, 64, 128):
        _walk(130, "config4", window)


@pytest.mark.parametrize("skew", [4, 1], ids=["checker-late", "committer-late"])
def test_commits_across_a_tenth_under_skew(skew, monkeypatch):
    monkeypatch.setenv("KSG_DEBUG", str(skew << 16))  # (tests/test_gpu_fuzz.py _SKEWS)
    _walk(64, "default", 64)


# ---- C: the gate -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ne.GATE_CASES))
def test_use_window_gate_both_sides(name):
    """On the bound the window path runs, one past it the exact kernel; both equal the
    oracle. A negative request or capacity cannot reach the window path at all."""
    case = ne.gate_case(name)
    orc = case.load(OracleScheduler(case.cfg))
    want, sw = orc.batch(case.batch, 31)
    dev = case.load(DeviceScheduler(case.cfg, device=0))
    dev.set_window(64)
    got, sg = dev.batch(case.batch, 31)
    windows = dev.last_batch_stats()["windows"]
    gc, gm = dev.read_requested()
    wc, wm = orc.read_requested()
    dev.close()
    assert np.array_equal(got, want) and sg == sw, (name, got, want)
    assert np.array_equal(gc, wc) and np.array_equal(gm, wm), name
    assert (windows > 0) == ne.GATE_CASES[name], (name, windows)


# ---- C: spreading and anti-affinity ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ladder_expected(policy):
    case = ne.ladder_case(policy, ne.LADDER_POOL)
    ref = ne.RefCluster(case.policy, case.cap_c, case.cap_m, case.labels)
    out = []
    for host, k, compare in ne.ladder_steps():
        for _ in range(k):
            ref.add_pod(host, 0, 0, (0,))
        if compare:
            out.append((ref.evaluate(*case.request, 0), ref.begin(*case.request, 0)))
    return out


def _compare_step(dev, orc, case, mode, want, where):
    (fails, scores), begin = want
    if mode == "evaluate":
        rc, gf, gs = dev.evaluate(case.batch, 0)
        assert rc == abi.KSG_OK
        _same_scores(gf, gs, fails, scores, where)
        _, of, os_ = orc.evaluate(case.batch, 0)
        _same_scores(of, os_, fails, scores, where + ("oracle",))
    else:
        _same_begin(dev.begin(case.batch, 0, want_fail=True), begin, where)
        _same_begin(orc.begin(case.batch, 0, want_fail=True), begin, where + ("oracle",))


@pytest.mark.parametrize("mode", ["evaluate", "block", "grid"])
@pytest.mark.parametrize("policy", ["default", "anti"])
def test_spreading_ladder_every_max_count(policy, mode, monkeypatch):
    """One service on 64 nodes; maxCount takes every value 1..300 (none thinned out): node j
    filled to j pods for j = 1..63, then pods on a host outside the node list. After each
    step the per-node scores (ksg_evaluate) or the begin result (both servers) against
    the reference: frac10_f32 with every divisor, the servers' table at every length.
    policy anti adds one ServiceAntiAffinity priority on zone (anti_term's
    frac10_f32(n - c_z, n) with the service's total as divisor)."""
    case = ne.ladder_case(policy, ne.LADDER_POOL)
    expected = _ladder_expected(policy)
    dev = _device(monkeypatch, "scan" if mode == "evaluate" else mode, case.cfg)
    orc = OracleScheduler(case.cfg)
    dev.set_cluster(case.arrays)
    orc.set_cluster(case.arrays)
    e = s = 0
    for host, k, compare in ne.ladder_steps():
        for _ in range(k):
            dev.add_pod(host, case.pool, e)
            orc.add_pod(host, case.pool, e)
            e += 1
        if compare:
            _compare_step(dev, orc, case, mode, expected[s], (policy, mode, s))
            s += 1
    assert s == len(expected) == ne.LADDER_TOP
    if mode != "evaluate":
        st = dev.serve_stats()
        assert st["eligible"] and st["grid"] == (mode == "grid") and st["requests"] >= s, st
    dev.close()


@pytest.mark.parametrize("mode", ["evaluate", "block", "grid"])
def test_spreading_table_edge(mode, monkeypatch):
    """The servers' per-pod table s_tab[count] has 1024 entries: one node's count at its last
    entry (maxCount 1023), just past it (1024, 1030: the direct form), and with maxCount
    1100 from a host outside the node list; the other nodes hold 0..6 pods, inside it."""
    case = ne.ladder_case("default", ne.TABLE_POOL)
    ref = ne.RefCluster(case.policy, case.cap_c, case.cap_m, case.labels)
    dev = _device(monkeypatch, "scan" if mode == "evaluate" else mode, case.cfg)
    orc = OracleScheduler(case.cfg)
    dev.set_cluster(case.arrays)
    orc.set_cluster(case.arrays)
    e, maxima = 0, []
    steps = [(j, j % 7) for j in range(ne.LADDER_NODES)] + list(ne.TABLE_STEPS)
    for s, (host, k) in enumerate(steps):
        for _ in range(k):
            dev.add_pod(host, case.pool, e)
            orc.add_pod(host, case.pool, e)
            ref.add_pod(host, 0, 0, (0,))
            e += 1
        if s >= ne.LADDER_NODES:
            maxima.append(max(ref.cnt[0].values()))
            want = (ref.evaluate(*case.request, 0), ref.begin(*case.request, 0))
            _compare_step(dev, orc, case, mode, want, ("table", mode, s))
    assert maxima == [1023, 1024, 1030, 1100]
    if mode != "evaluate":
        st = dev.serve_stats()
        assert st["eligible"] and st["grid"] == (mode == "grid"), st
    dev.close()
