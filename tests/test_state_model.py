"""The plain state model (tests/state_model.py) against the C restatement's read_state(), bit for
bit after every operation of every sequence tests/test_gpu_state.py runs on the device, and the
sequences' own coverage, so that the device test cannot pass vacuously. No GPU needed: the
placements come from the restatement."""
import numpy as np
import pytest

from tests import state_model as sm
from tests.state_model import SEQUENCES, StateModel, make_sequence, run_sequence


@pytest.mark.parametrize("spec", SEQUENCES, ids=lambda s: "-".join(str(x) for x in s))
def test_model_matches_oracle_and_sequence_covers(spec):
    seq = make_sequence(*spec)
    assert 30 <= len(seq.ops) <= 45, len(seq.ops)
    for op in seq.ops:
        if op[0] == "batch":
            assert 30 <= op[2] - op[1] <= 120
    cov = run_sequence(seq)
    # each of these is a condition on the generator
    assert 2 * cov["batch_placed"] >= cov["batch_pods"] > 0, cov
    assert cov["max_undone"] >= 5, cov
    assert cov["peer_moved"] >= 1, cov
    assert cov["max_lowered"] >= 1, cov
    assert cov["shared_left"] >= 1, cov
    assert cov["offlist_audits"] >= 1, cov
    assert cov["nofit_after_mid"] >= 1, cov
    kinds = {op[0] for op in seq.ops} | {op[:2] for op in seq.ops if op[0] in ("unwind", "fail", "query")}
    for need in ("add", "remove", "batch", "rebatch", "begin_commit", "begin_abandon", "set_cluster", "remove_all",
                 ("unwind", "first"), ("unwind", "mid"), ("unwind", "last"), ("fail", "batch_live_uid"),
                 ("fail", "unwind_k_ge_n"), ("fail", "unwind_nofit"), ("fail", "remove_unknown"),
                 ("query", "explain"), ("query", "prioritize"), ("query", "headroom"), ("query", "explain_without")):
        assert need in kinds, need
    assert {op[3] for op in seq.ops if op[0] == "batch"} == {"seed", "draws"}


def test_second_unwind_in_some_sequences():
    n = [sum(op[0] == "unwind" for op in make_sequence(*s).ops) for s in SEQUENCES[:4]]
    assert 4 in n and 3 in n, n


def test_model_on_a_hand_worked_example():
    """Five pods on three nodes and one host outside the list, every array written out by hand."""
    m = StateModel(n_nodes=3, n_services=2, n_keys=4, n_scalar=1)
    P = sm.PodRec
    m.add(P(1, 5, 100, 10, [0], [0], (1,)))          # off-list: counts only for total, max, peer
    m.add(P(2, 5, 100, 10, [], [0, 1], (0,)))
    m.add(P(3, 2, 300, 30, [1, 1, 3], [0], (2,)))    # a key listed twice
    m.add(P(4, 2, -50, 5, [1], [1], (4,)))
    m.add(P(5, 0, (1 << 63) - 1, 1, [], [], (0,)))
    a = m.arrays()
    assert a["used_cpu"].tolist() == [(1 << 63) - 1, 0, 250] and a["used_mem"].tolist() == [1, 0, 35]
    assert a["scalar_used"].tolist() == [[0, 0, 6]]
    assert a["keymap"].tolist() == [[0], [4], [0], [4]]
    assert a["svc_cnt"].tolist() == [[0, 0, 1], [0, 0, 1]] and a["svc_bits"].tolist() == [[4], [4]]
    assert a["svc_total"].tolist() == [3, 2] and a["svc_max"].tolist() == [2, 1]
    assert a["svc_peer"].tolist() == [-2, -2]
    m.add(P(6, 0, 1, 0, [], [], (0,)))               # int64 wrap, as Go's
    assert m.arrays()["used_cpu"][0] == -(1 << 63)
    m.remove(1)
    m.remove(2)
    a = m.arrays()
    assert a["svc_peer"].tolist() == [2, 2] and a["svc_max"].tolist() == [1, 1] and a["svc_total"].tolist() == [1, 1]
    m.remove(4)
    assert m.arrays()["keymap"].tolist() == [[0], [4], [0], [4]]  # pod 3 still holds key 1 on node 2
    m.remove(3)
    a = m.arrays()
    assert not a["keymap"].any() and a["svc_peer"].tolist() == [-1, -1] and not a["svc_cnt"].any()


class _NoOffListMax(StateModel):
    """Broken on purpose: svc_max over the node hosts only."""

    def host_counts(self, s):
        return {h: v for h, v in super().host_counts(s).items() if h < self.N}


class _NewestPeer(StateModel):
    """Broken on purpose: the newest member as the peer."""

    def arrays(self):
        a = super().arrays()
        for p in self.live:
            for s in p.svcs:
                a["svc_peer"][s] = p.host if p.host < self.N else -2
        return a


@pytest.mark.parametrize("broken,array", [(_NoOffListMax, "svc_max"), (_NewestPeer, "svc_peer")])
def test_a_broken_model_is_caught_at_the_first_operation_that_touches_the_field(broken, array):
    seq = make_sequence(*SEQUENCES[0])
    with pytest.raises(AssertionError) as e:
        run_sequence(seq, model_cls=broken)
    msg = str(e.value)
    assert "oracle vs model: " + array in msg, msg
    idx = int(msg.split(" op ")[1].split(" ")[0])
    # the first operation after which the two models differ at all (the sequence opens with adds)
    good, bad = StateModel(seq.n_nodes, seq.arrays.n_services, sm.MAX_KEYS), broken(seq.n_nodes, seq.arrays.n_services,
                                                                                  sm.MAX_KEYS)
    for first, op in enumerate(seq.ops):
        assert op[0] == "add", "the models never differed over the opening adds"
        for m in (good, bad):
            m.add(sm.pod_rec(seq.pool, op[1], op[2]))
        if sm.diff_states(bad.arrays(), good.arrays()):
            break
    assert idx == first, (idx, first, msg)
