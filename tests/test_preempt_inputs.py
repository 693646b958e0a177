"""The inputs of the ksg_preempt_batch tests are not vacuous, on the CPU with the C restatement
only: what tests/preempt_cases.py's reference yields for the scenarios tests/test_gpu_preempt.py
compares the device against."""
import numpy as np
import pytest

from kubernetes_amd import abi
from tests import explain_cases as X
from tests import preempt_cases as P
from tests import without_cases as W

# (cells with victims and reprieved pods both, non-candidate cells, pods whose best node needs an
# eviction, pods that fit a node as things stand, pods without a candidate) of
# random_scenario(policy, nn, k) under the reference
KINDS = {("config2", 65, 31): (66, 1567, 17, 8, 6), ("config2", 65, 32): (72, 1552, 19, 9, 4),
         ("config2", 65, 33): (62, 1601, 14, 9, 10), ("presence", 63, 31): (42, 1626, 25, 4, 2),
         ("presence", 63, 32): (59, 1732, 24, 4, 4), ("presence", 63, 33): (58, 1739, 24, 4, 5),
         ("config2", 257, 31): (16, 5806, 12, 19, 0), ("config2", 257, 32): (24, 5945, 13, 19, 0),
         ("config2", 257, 33): (35, 6285, 13, 20, 0)}


def test_the_symbols_are_bound():
    lib = abi.load_library()
    assert lib.ksg_preempt_batch is not None and lib.ksg_last_preempt_ms is not None
    assert abi.PREEMPT_MAX_VICTIMS == 256 and abi.PREEMPT_NOFIT == 0xFFFFFFFF


@pytest.mark.parametrize("policy,nn,k", sorted(KINDS))
def test_random_scenarios_are_not_vacuous(policy, nn, k):
    assert nn in (63, 65, X.TILE + 1) and k in X.POD_COUNTS
    sc = W.random_scenario(policy, nn, k)
    r = P.oracle_reference(sc)
    mixed, nocand_cells, evict, free, _ = kinds = r.kinds()
    assert mixed > 0 and nocand_cells > 0 and evict > 0 and free > 0
    assert kinds == KINDS[policy, nn, k]
    # a pod at position n_absent may evict nothing
    at_end = sc.positions == len(sc.absent)
    assert at_end.any() and not r.n_victims[at_end].any()
    assert np.isin(r.node_victims[at_end], (0, P.NOFIT)).all()


@pytest.mark.parametrize("policy,nn,k", sorted(KINDS))
def test_candidates_are_explain_withouts_fitting_nodes(policy, nn, k):
    """The reference's cand_count is the zero-code count of without_cases.scenario_reference, and
    its free_count the zero-code count at position n_absent (the state as it stands)."""
    from oracle.pyoracle import OracleScheduler

    sc = W.random_scenario(policy, nn, k)
    r = P.oracle_reference(sc)
    codes, err = W.oracle_reference(sc)
    assert not err.any()
    assert np.array_equal(r.cand, (codes == 0).sum(axis=1))
    assert np.array_equal(r.node_victims != P.NOFIT, codes == 0)
    orc = OracleScheduler(sc.cfg)
    try:
        sc.load(orc)
        now = np.stack([orc.evaluate(sc.probe, i)[1].copy() for i in range(len(sc.probe))])
    finally:
        orc.close()
    assert np.array_equal(r.free, (now == 0).sum(axis=1))


@pytest.mark.parametrize("name", sorted(P.HANDMADE))
def test_handmade_victim_lists(name):
    """The handmade scenarios give the victim lists they are named for."""
    sc = P.handmade(name)
    r = P.oracle_reference(sc)
    named = {}
    for (i, node), want in sc.want.items():
        x = sc.names.index(node)
        named.setdefault(i, set()).add(x)
        assert [sc.listed[j] for j in r.lists[i][x]] == want, (i, node)
        assert r.node_victims[i, x] == len(want)
    for i in range(len(sc.probe)):  # every other node is no candidate
        others = [x for x in range(sc.nn) if x not in named.get(i, ())]
        assert (r.node_victims[i, others] == P.NOFIT).all()


def test_handmade_choices():
    """The choice among the nodes, written out."""
    def best(name):
        sc = P.handmade(name)
        r = P.oracle_reference(sc)
        return [(None if b < 0 else sc.names[b], int(k)) for b, k in zip(r.best, r.n_victims)]

    assert best("memory-only") == [("n1", 1)]
    assert best("ext-only") == [("n1", 2)]
    assert best("zero-request") == [("n1", 0), ("n1", 2)]
    assert best("cap-zero") == [("n1", 1)]
    assert best("negative-request") == [("n2", 0)]      # x2 stays behind neg2; on n1 x1 came first
    assert best("top-beats-count") == [("n2", 2)]       # two lesser victims before the most important one
    assert best("rank-tie") == [("n3", 0), ("n3", 1)]   # n1 and n3 tie without a victim; then c is the least important
    assert best("long-row") == [("n1", P.LONG - 1)]
    r = P.oracle_reference(P.handmade("long-row"))
    assert r.n_victims[0] > P.MAX_VICTIMS and r.victims[0].tolist() == list(range(1, P.MAX_VICTIMS + 1))
    r = P.oracle_reference(P.handmade("rank-tie"))
    assert r.free.tolist() == [2, 0] and r.cand.tolist() == [3, 3]


def test_reused_handmade_scenarios_conflict_keys():
    """without_cases' port and disk scenarios: a holder among the candidates is a victim, a holder
    outside them makes the node fail."""
    two, out = P.handmade("two-holders"), P.handmade("outside-holder")
    r2, ro = P.oracle_reference(two), P.oracle_reference(out)
    n1 = two.names.index("n1")
    per = two.per_probe  # probe 1 (port-only) at position 0: rows per, per + 1, ...
    # every listed pod may go: both holders of port 8080 (list indices 3 and 7) are victims of n1
    assert [j for j in r2.lists[per][n1] if j in (3, 7)] == [3, 7]
    # position 4: h3 stays on the node, outside C: n1 is no candidate
    assert r2.node_victims[per + 4, n1] == P.NOFIT
    # a holder outside the list: n1 is never a candidate for the port pods
    assert (ro.node_victims[:, n1] == P.NOFIT).all()
    for name in ("wrap", "outside-host"):
        r = P.oracle_reference(P.handmade(name))
        assert (r.cand > 0).all()
