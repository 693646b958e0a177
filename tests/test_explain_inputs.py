"""The inputs of tests/test_gpu_explain.py are not vacuous (CPU; the C restatement alone):
after the fill batch the probe pods of tests/explain_cases.py together meet every fail code
1-7 (8 and 9 in the extension cases), some pod fits no node at all, and some pod fits some
nodes and fails on others. A parity test over inputs where every pod fits everywhere would
pass with a kernel that writes zeros."""
import numpy as np
import pytest

from kubernetes_amd import abi
from tests import explain_cases as X


def _hist(codes):
    return np.stack([np.bincount(r, minlength=abi.EXPLAIN_SLOTS) for r in codes])


def test_tiling_constants_are_read_from_the_kernel_header():
    assert X.TILE % 64 == 0 and X.TILE > 64 and X.CHUNK > 1
    assert len(set(X.NODE_COUNTS)) == len(X.NODE_COUNTS) and len(set(X.POD_COUNTS)) == len(X.POD_COUNTS)
    assert X.N_PROBE >= max(X.POD_COUNTS)


@pytest.mark.parametrize("nn", X.NODE_COUNTS)
def test_reference_policies_cover_fail_codes_1_to_7(nn):
    seen, none_fits, mixed = set(), False, False
    by_policy = {}
    for policy in X.POLICIES:
        codes = X.oracle_codes_cached(policy, nn)
        assert codes.shape == (X.N_PROBE, nn)
        h = _hist(codes)
        by_policy[policy] = set(np.unique(codes).tolist())
        seen |= by_policy[policy]
        none_fits |= bool((h[:, 0] == 0).any())
        mixed |= bool(((h[:, 0] > 0) & (h[:, 0] < nn)).any())
    assert seen >= set(range(0, 8)), (nn, by_policy)
    assert max(seen) <= abi.FAIL_SERVICEAFFINITY
    assert none_fits and mixed
    # each policy's own code comes from its own case
    assert abi.FAIL_SERVICEAFFINITY in by_policy["config4"] | by_policy["invalid_selectors"]
    assert abi.FAIL_LABELSPRESENCE in by_policy["presence"]
    assert abi.FAIL_HOSTNAME in by_policy["hosts"]
    # the fill left state-dependent failures behind (not only static ones)
    assert {abi.FAIL_PODFITSRESOURCES, abi.FAIL_PODFITSPORTS, abi.FAIL_NODISKCONFLICT} <= by_policy["config2"]


def test_hosts_case_pins_to_a_rank_and_to_no_node():
    c = X.xcase("hosts", 257)
    hosts = c.probe.pods["host"]
    assert (hosts >= 0).any() and (hosts == -2).any() and (hosts == -1).any()
    codes = X.oracle_codes_cached("hosts", 257)
    assert (codes[hosts == -2] == abi.FAIL_HOSTNAME).all()  # fits nowhere
    for row, h in zip(codes[hosts >= 0], hosts[hosts >= 0]):
        assert (np.delete(row, h) == abi.FAIL_HOSTNAME).all()


@pytest.mark.parametrize("nn", (X.TILE + 1, 1000))
def test_extension_case_covers_codes_8_and_9(nn):
    c = X.xext(nn)
    codes = X.oracle_codes(c)
    seen = set(np.unique(codes).tolist())
    assert {abi.FAIL_NONE, abi.FAIL_TAINTS, abi.FAIL_SCALAR} <= seen, seen
    plain = X.oracle_codes(c, c.probe_plain)  # ext == NULL: the extension filters see an all-zero record
    assert not ({abi.FAIL_TAINTS, abi.FAIL_SCALAR} & set(np.unique(plain).tolist()))
    assert (plain != codes).any()
