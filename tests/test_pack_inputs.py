"""The inputs of the ksg_pack_batch tests are not vacuous, on the CPU with the C restatement only:
what tests/pack_cases.py's reference yields for the scenarios tests/test_gpu_pack.py compares the
device against."""
import numpy as np
import pytest

from kubernetes_amd import abi
from tests import pack_cases as K

# (sets of at least one pod placed whole, sets with an unplaced pod, pods on a node an earlier pod of
# their set took, pods whose node is not the one the state as it stands would give them, pods
# whose highest fitting node was the excluded or a masked one, pods that end below the scan's
# first strip) of random_scenario(policy, nn, variant) under the reference. The last kind cannot
# occur where the whole cluster is one strip (nn <= STRIP): there it is pinned at 0.
KINDS = {("config2", 63, ""): (4, 6, 15, 34, 22, 0), ("presence", 64, ""): (4, 6, 5, 30, 14, 0),
         ("hosts", 65, ""): (4, 6, 3, 26, 10, 0), ("config2", 255, ""): (3, 7, 5, 29, 12, 0),
         ("presence", 256, ""): (3, 7, 8, 21, 11, 0), ("config2", 257, ""): (2, 8, 1, 16, 7, 4),
         ("hosts", 513, ""): (2, 8, 5, 19, 9, 11), ("config2", 513, "mask"): (2, 8, 3, 19, 42, 14),
         ("ext", 257, ""): (6, 4, 20, 7, 11, 15), ("ext-null", 65, ""): (8, 2, 50, 17, 35, 0),
         ("config2", 1000, ""): (4, 6, 22, 37, 25, 4)}


def test_the_symbols_are_bound():
    lib = abi.load_library()
    assert lib.ksg_pack_batch is not None and lib.ksg_last_pack_ms is not None
    assert abi.PACK_NO_NODE == 0xFFFFFFFF and abi.PACK_MAX_SET == 1024
    assert K.STRIP % 64 == 0 and K.STRIP == 256  # (the node counts below stand on both sides of it)


def test_the_table_covers_the_scenarios_and_node_counts():
    assert sorted(KINDS) == sorted(K.RANDOM)
    assert {nn for _, nn, _ in K.RANDOM} == {63, 64, 65, K.STRIP - 1, K.STRIP, K.STRIP + 1, 2 * K.STRIP + 1, 1000}
    assert {p for p, _, _ in K.RANDOM} == {"config2", "presence", "hosts", "ext", "ext-null"}
    assert sum(1 for _, _, v in K.RANDOM if v == "mask") == 1
    assert {0, 1} <= set(K.SET_SIZES) and sum(1 for m in K.SET_SIZES if m >= 8) >= 3


@pytest.mark.parametrize("policy,nn,variant", sorted(KINDS))
def test_random_scenarios_are_not_vacuous(policy, nn, variant):
    sc = K.random_scenario(policy, nn, variant)
    r = K.oracle_reference(sc)
    full, short, again, moved, barred, below = kinds = r.kinds()
    assert full > 0 and short > 0 and again > 0 and moved > 0 and barred > 0
    assert (below > 0) == (nn > K.STRIP)  # (no node lies below the first strip of a one-strip cluster)
    assert kinds == KINDS[policy, nn, variant]
    # about a third of the sets exclude a node; the mask variant masks some
    n_ex = int((sc.exclude != K.NO_NODE).sum())
    assert 2 <= n_ex <= len(sc.sizes) // 2
    assert (sc.targets is not None) == (variant == "mask")
    # the rows are the definition's: a placed pod's node was open to its set, an unplaced pod had no open node
    at = 0
    for s, m in enumerate(sc.sizes.tolist()):
        ok = sc.open_nodes(s)
        for i in range(at, at + m):
            if r.out[i] >= 0:
                assert ok[r.out[i]] and (r.raw_best[i] == r.out[i] or not ok[r.raw_best[i]])
            else:
                assert r.out[i] == K.NOFIT
        at += m


@pytest.mark.parametrize("name", sorted(K.HANDMADE))
def test_handmade_rows(name):
    """The handmade scenarios give the rows they are named for, written out."""
    sc = K.handmade(name)
    r = K.oracle_reference(sc)
    out, placed = K.want_rows(sc)
    assert r.out.tolist() == out.tolist()
    assert r.placed.tolist() == placed.tolist()


def test_handmade_rows_say_what_their_names_say():
    def rows(name):
        sc = K.handmade(name)
        r = K.oracle_reference(sc)
        return [[None if o < 0 else sc.names[o] for o in r.out[r.off[s]: r.off[s + 1]]] for s in range(len(sc.sizes))]

    assert rows("fill-then-spill") == [["n3", "n3", "n2", "n2", "n1"]]
    assert rows("port-twice") == rows("pd-twice") == [["n3", "n2"]]
    assert rows("port-vs-pd") == [["n3", "n2", "n3"]]
    assert rows("exclude-top") == [["n2"], ["n3"]]
    assert rows("mask") == [["n2", "n1"]]
    assert rows("nofit-in-middle") == [["n3", None, "n3"]]
    assert K.oracle_reference(K.handmade("nofit-in-middle")).placed.tolist() == [2]
    assert rows("negative-request") == [["n3", "n3"], ["n2"]]  # the big pod alone has no room on n3
    assert rows("wrap") == [["n2", "n2", "n1"], ["n1"]]
    assert rows("cap-zero") == [["n3", "n3", "n2", "n1"]]
    assert rows("zero-request") == [["n3", "n3", "n2", "n3"]]
    assert rows("ext-scalar") == [["n3", "n2", "n2", None]]
    assert rows("ext-null") == [["n3"] * 4]
    assert rows("last-strip") == [["n0000", "n0000", None]]
    two = rows("same-set-twice")
    assert two[0] == two[1] == ["n3", "n3", "n2", "n2"]
    long = K.oracle_reference(K.handmade("long-set"))
    assert long.placed.tolist() == [K.MAX_SET]
    assert np.bincount(long.out, minlength=4).tolist() == [K.MAX_SET - 3 * K.LONG_PER_NODE] + [K.LONG_PER_NODE] * 3
    assert K.handmade("last-strip").nn == 2 * K.STRIP + 1 and K.first_strip_lo(2 * K.STRIP + 1) > 0
