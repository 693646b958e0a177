"""The inputs of the ksg_explain_without tests, on the CPU with the C restatement only
(tests/without_cases.py): the one-batch inputs really have pods whose FailedPredicateMap as of
the pod differs from the map after the batch (so the device parity test cannot pass by calling
ksg_explain_batch), removing the placed pods from the tail reproduces the sequential rows, and
the handmade scenarios reach the edges they are named for."""
import numpy as np
import pytest

from kubernetes_amd import abi
from oracle.pyoracle import OracleScheduler
from tests import without_cases as W

# pods with a differing map, NOFIT pods, differing (pod, node) cells: the sequential rows against
# the after-batch evaluate, XCase(policy, nn) as one 233-pod batch, seed 1234
DIFFERING = {("config2", 63): (12, 121, 17), ("config2", 65): (22, 122, 41), ("config2", 257): (8, 40, 17),
             ("config4", 63): (63, 132, 260), ("config4", 65): (41, 129, 158), ("config4", 257): (39, 52, 152),
             ("presence", 63): (25, 147, 29), ("presence", 65): (27, 137, 42), ("presence", 257): (10, 45, 24)}


def _after_batch(bc):
    """(placements of orc.batch, its final state, the NOFIT pods' evaluate rows after the batch, the oracle)"""
    orc = OracleScheduler(bc.cfg)
    orc.set_cluster(bc.case.view.arrays)
    out, state = orc.batch(bc.batch, W.SEED)
    rows = np.stack([orc.evaluate(bc.batch, int(i))[1].copy() for i in bc.nofit])
    return out.copy(), state, rows, orc


@pytest.mark.parametrize("policy,nn", sorted(DIFFERING))
def test_batch_inputs_are_not_vacuous(policy, nn):
    bc = W.batch_case(policy, nn)
    out, state, after, orc = _after_batch(bc)
    try:
        assert np.array_equal(out, bc.out) and state == bc.state  # the sequential run is the batch
        diff = after != bc.rows
        later = np.array([(bc.out[i + 1:] >= 0).any() for i in bc.nofit])
        assert (diff.any(axis=1) & later).any()
        assert not diff[~later].any()  # no later placement: the two states are the same
        assert (int(diff.any(axis=1).sum()), len(bc.nofit), int(diff.sum())) == DIFFERING[policy, nn]
    finally:
        orc.close()


@pytest.mark.parametrize("nn", (65, 257))
@pytest.mark.parametrize("policy", W.BATCH_POLICIES)
def test_removing_the_tail_reproduces_the_sequential_rows(policy, nn):
    bc = W.batch_case(policy, nn)
    sc = W.Scenario(f"asof-{policy}-{nn}", bc.cfg, None, bc.placed_uids, bc.sub, bc.positions, nn)

    def load(orc):
        orc.set_cluster(bc.case.view.arrays)
        out, _ = orc.batch(bc.batch, W.SEED)
        assert np.array_equal(out, bc.out)

    sc.load = load
    orc = OracleScheduler(bc.cfg)
    try:
        codes, err = W.scenario_reference(sc, orc)
    finally:
        orc.close()
    assert not err.any()
    bad = np.argwhere(codes != bc.rows)
    assert bad.size == 0, f"first mismatches (NOFIT pod, node) {bad[:6].tolist()}"


def _rows(name):
    sc = W.handmade(name)
    codes, err = W.oracle_reference(sc)
    k = sc.per_probe
    return sc, codes.reshape(-1, k, sc.nn), err.reshape(-1, k)  # [probe][position][node]


def test_two_holders():
    """h3 and h7 hold port 8080 on n1 at list indices 3 and 7: the bit is clear iff position <= 3."""
    D, P, R = abi.FAIL_NODISKCONFLICT, abi.FAIL_PODFITSPORTS, abi.FAIL_PODFITSRESOURCES
    sc, codes, err = _rows("two-holders")
    assert not err.any() and sc.per_probe == 9
    n1 = sc.names.index("n1")
    # port + PD, 400m: free, then big1's 700m, then a port holder, then d5's disk
    assert codes[0, :, n1].tolist() == [0, 0, R, R, P, P, D, D, D]
    assert codes[1, :, n1].tolist() == [0, 0, 0, 0, P, P, P, P, P]  # the port alone
    assert not codes[:, :, [sc.names.index("n2"), sc.names.index("n3")]].any()
    sc2, codes2, err2 = _rows("outside-holder")
    assert not err2.any()
    assert codes2[0, :, n1].tolist() == [P, P, P, P, P, P, D, D, D]  # a holder outside the list: always set
    assert codes2[1, :, n1].tolist() == [P] * 9


def test_peers():
    A = abi.FAIL_SERVICEAFFINITY
    sc, codes, err = _rows("peers")  # members m0@n1(r1), m1@n2(r2), m2@n3(r1); the list is m2, m1, m0
    assert not err.any()
    # needs-peer at positions 0..3: no member left, m2 (r1), m1 (r2: the first member is absent), m0 (r1)
    assert codes[0].tolist() == [[0, 0, 0], [0, A, 0], [A, 0, A], [0, A, 0]]
    assert codes[1].tolist() == [[0, A, 0]] * 4 and not codes[2].any()  # its own selector; no service


def test_peer_on_an_unknown_host():
    sc, codes, err = _rows("peer-unknown")  # m0@n1, g@gone-host, m2@n3; the list is m0
    assert err.tolist() == [[1, 0], [0, 0], [0, 0]]  # m0 away: the peer is g; the unmodified state has none
    assert not codes[0, 0].any() and codes[0, 1].tolist() == [0, abi.FAIL_SERVICEAFFINITY, 0]
    sc, codes, err = _rows("peer-unknown-converse")  # g@gone-host, m1@n2; the list is g
    assert err.tolist() == [[0, 1], [0, 0], [0, 0]]  # g away clears the error the unmodified state has
    assert codes[0, 0].tolist() == [abi.FAIL_SERVICEAFFINITY, 0, abi.FAIL_SERVICEAFFINITY]
    orc = OracleScheduler(sc.cfg)
    try:
        sc.load(orc)
        assert orc.evaluate(sc.probe, sc.per_probe - 1)[0] == abi.KSG_ERR_NOPEER
    finally:
        orc.close()


def test_wrap_and_outside_host():
    R = abi.FAIL_PODFITSRESOURCES
    sc, codes, err = _rows("wrap")  # n1: 200m + (2^63 - 100)m + 300m wrapped; the list is late, huge
    orc = OracleScheduler(sc.cfg)
    try:
        sc.load(orc)
        assert orc.read_requested()[0][0] < 0  # the total did wrap
    finally:
        orc.close()
    assert codes[0, :, 0].tolist() == [0, 0, R] and not err.any()  # 200m, 500m: fits; wrapped: does not
    sc, codes, err = _rows("outside-host")  # o on a host outside the node list, a@n1 (300m, port 8080)
    assert codes[0].tolist() == [[0, 0], [0, 0], [abi.FAIL_PODFITSPORTS, 0]] and not err.any()
