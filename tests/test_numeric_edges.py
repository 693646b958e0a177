"""CPU-only checks of tests/numeric_edges.py: the reference against the C oracle on
every generated case, the builders' own conditions (the reciprocal's teeth, the
capacity set, what the factory compiled), and the reference's arithmetic by hand."""
import numpy as np
import pytest

from kubernetes_amd import abi
from oracle.pyoracle import OracleScheduler
from tests import numeric_edges as ne

EDGE = [(k, p) for k in ("tame", "wild") for p in ("config1", "default", "big", "huge")]


def test_reference_arithmetic_by_hand():
    assert ne.calculate_score(0, 0) == 0 and ne.calculate_score(5, 4) == 0
    assert ne.calculate_score(0, 7) == 10 and ne.calculate_score(7, 7) == 0 and ne.calculate_score(3, 7) == 5
    # the issue's example: cap -1, requested -2^41 -> (2^41 - 1) * 10 / -1
    assert ne.calculate_score(-(1 << 41), -1) == -((1 << 41) - 1) * 10
    # (cap - requested) * 10 wraps: cap 2^63 - 1, requested 0 -> (2^63 - 1) * 10 mod 2^64 = -10
    assert ne.calculate_score(0, (1 << 63) - 1) == go_trunc(-10, (1 << 63) - 1) == 0
    assert ne.calculate_score(0, 1 << 62) == go_trunc(ne.i64((1 << 62) * 10), 1 << 62) == -2
    assert ne.go_div(-(1 << 63), -1) == -(1 << 63) and ne.go_div(-7, 2) == -3 and ne.go_div(7, -2) == -3
    assert ne.frac10(3, 3) == 10 and ne.frac10(0, 5) == 0 and ne.frac10(1, 3) == 3
    # the true float32 form equals floor(10 a / b) for every pair up to 2048 ...
    for b in range(1, 2049, 7):
        for a in range(0, b + 1):
            assert ne.frac10(a, b) == 10 * a // b, (a, b)
    # ... while a reciprocal multiply does not (e.g. maxCount 25, 41, 47)
    for b in (25, 41, 47):
        r = np.float32(1) / np.float32(b)
        assert any(int(np.float32(10) * (np.float32(a) * r)) != 10 * a // b for a in range(b + 1)), b


def go_trunc(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def test_capacity_set_and_slots():
    tame, wild = ne.edge_case("tame", "config1"), ne.edge_case("wild", "config1")
    caps_t, caps_w = set(tame.cap_c) | set(tame.cap_m), set(wild.cap_c) | set(wild.cap_m)
    assert len(tame.cap_c) == len(wild.cap_c) == 130
    want_tame = {0, 1, 3, 7, 9, 10, 11, (1 << 49) - 1, 1 << 49, (1 << 49) + 1, ne.LR_FAST_CAP, ne.LR_FAST_CAP + 1,
                 (1 << 63) // 10, ne.PRIME_49}
    assert want_tame <= caps_t and max(caps_t) <= ne.TENTH_MAX and min(caps_t) == 0
    assert {(1 << 63) // 10 + 1, 1 << 62, (1 << 63) - 1, -1, -5, -(1 << 40), 0, 1 << 49} <= caps_w
    assert sum(1 for c in caps_t if c % 10 == 0 and 11 < c <= 1 << 49) >= 32
    assert all(p % q for p in (ne.PRIME_49,) for q in range(3, 10 ** 6, 2))  # (the prime: no factor below 10^6 ...)
    assert pow(2, ne.PRIME_49 - 1, ne.PRIME_49) == 1                          # (... and a Fermat witness)
    # nothing negative is committed or asked for in the tame cluster
    assert all(c >= 0 and m >= 0 for _, c, m, _ in tame.existing_plain) and all(min(r) >= 0 for r in tame.requests)
    # every slot of a kind is on some node
    for case in (tame, wild):
        ref = case.reference()
        have = set(zip(ref.cap_c, ref.used_c)) | set(zip(ref.cap_m, ref.used_m))
        assert set(ne._slots(case.kind)) <= have
    # requested = cap, requested = cap + 1, a zero request on a full node, negative requests, 2^62
    ref = tame.reference()
    totals = {(cap, ne.i64(used + r)) for cap, used in zip(ref.cap_c, ref.used_c) for r, _ in tame.requests}
    assert any(c == t and c > 11 for c, t in totals) and any(t == c + 1 and c > 11 for c, t in totals)
    assert (0, 0) in tame.requests and any(u >= c > 0 for c, u in zip(ref.cap_c, ref.used_c))
    assert any(min(r) < 0 for r in wild.requests) and (1 << 62, 1 << 62) in tame.requests


def test_reciprocal_teeth():
    """The reciprocal form is wrong without its fix-up on >= 32 of the points the tame
    cluster scores at (capacity <= 2^49), and the upward correction applies on >= 8."""
    for cap, u in ne.TEETH:
        assert cap % 10 == 0 and cap < 1 << 49 and (10 * u) % cap == 0 and ne.reciprocal_wrong(u, cap), (cap, u)
    pts = ne.lr_points(ne.edge_case("tame", "config1"))
    wrong = [p for p in pts if ne.reciprocal_wrong(p[1], p[0])]
    up = [p for p in pts if ne.reciprocal_needs_up(p[1], p[0])]
    assert len(wrong) >= 32, len(wrong)
    assert len(up) >= 8, len(up)
    # u on ceil(k cap / 10) + {-1, 0, +1} for every k, for each large tame capacity
    for cap in ne.TAME_BIG_CAPS:
        if cap > 1 << 49:
            continue
        us = {u for c, u in pts if c == cap}
        for k in range(1, 10):
            t = -((-k * cap) // 10)
            assert {t - 1, t, t + 1} <= us, (cap, k)


@pytest.mark.parametrize("name", ["config1", "default", "big", "huge", "anti"])
def test_policy_numbers_match_the_compiled_config(name):
    policy, _ = ne.policies()[name]
    cfg = ne.edge_case("tame", name).cfg if name != "anti" else ne.ladder_case("anti", 8).cfg
    assert (cfg.w_least_requested, cfg.w_service_spreading, cfg.w_equal) == (policy.w_lr, policy.w_spread, policy.w_equal)
    assert [cfg.w_anti[a] for a in range(cfg.n_anti)] == [w for _, w in policy.antis]
    assert [(cfg.w_pref[q], bool(cfg.pref_presence[q])) for q in range(cfg.n_label_pref)] == \
        [(w, pres) for _, pres, w in policy.prefs]
    assert bool(cfg.predicates & abi.PRED_PODFITSRESOURCES) and not cfg.predicates & abi.PRED_SERVICEAFFINITY


def _check_pod(ref, orc, batch, i, cpu, mem, where):
    svc = int(batch.pods["service"][i])
    p = batch.pods[i]
    assert svc == 0 and p["n_svcs"] == 1 and batch.ids[p["svcs_off"]] == 0 and p["host"] == -1
    assert p["n_ports"] == p["n_pds"] == p["n_sel"] == 0 and (int(p["milli_cpu"]), int(p["memory"])) == (cpu, mem)
    fails, scores = ref.evaluate(cpu, mem, svc)
    rc, ofails, oscores = orc.evaluate(batch, i)
    assert ofails.tolist() == fails, (where, i)
    for n, s in enumerate(scores):
        if s is not None:
            assert int(oscores[n]) == s, (where, i, n, ref.cap_c[n], ref.used_c[n], ref.cap_m[n], ref.used_m[n])
    want = ref.begin(cpu, mem, svc)
    rc, m, k, bf = orc.begin(batch, i, want_fail=True)
    assert (rc, m if rc == abi.KSG_OK else 0, k, bf.tolist()) == (want[0], want[1], want[2], want[3]), (where, i)


@pytest.mark.parametrize("kind,policy", EDGE)
def test_reference_equals_oracle_on_edge_cases(kind, policy):
    case = ne.edge_case(kind, policy)
    ref, orc = case.reference(), case.load(OracleScheduler(case.cfg))
    oc, om = orc.read_requested()
    assert oc.tolist() == ref.used_c and om.tolist() == ref.used_m
    for i, (cpu, mem) in enumerate(case.requests):
        _check_pod(ref, orc, case.batch, i, cpu, mem, (kind, policy))
    if kind == "wild":  # the point of the wild cluster: combined scores outside int32
        scores = [s for cpu, mem in case.requests for s in ref.evaluate(cpu, mem, 0)[1] if s is not None]
        if policy != "huge":
            assert min(scores) < -(1 << 31) and max(scores) >= 1 << 31


@pytest.mark.parametrize("policy", ["default", "anti"])
def test_reference_equals_oracle_on_the_ladder(policy):
    case = ne.ladder_case(policy, ne.LADDER_POOL)
    ref = ne.RefCluster(case.policy, case.cap_c, case.cap_m, case.labels)
    orc = OracleScheduler(case.cfg)
    orc.set_cluster(case.arrays)
    e, seen = 0, set()
    for host, k, compare in ne.ladder_steps():
        for _ in range(k):
            orc.add_pod(host, case.pool, e)
            ref.add_pod(host, 0, 0, (0,))
            e += 1
        if compare:
            seen.add(max(ref.cnt[0].values()))
            _check_pod(ref, orc, case.batch, 0, *case.request, (policy, e))
    assert e == ne.LADDER_POOL and seen == set(range(1, ne.LADDER_TOP + 1))


def test_reference_equals_oracle_at_the_table_edge():
    case = ne.ladder_case("default", ne.TABLE_POOL)
    ref = ne.RefCluster(case.policy, case.cap_c, case.cap_m, case.labels)
    orc = OracleScheduler(case.cfg)
    orc.set_cluster(case.arrays)
    e, maxima = 0, []
    steps = [(j, j % 7) for j in range(ne.LADDER_NODES)] + list(ne.TABLE_STEPS)
    for s, (host, k) in enumerate(steps):
        for _ in range(k):
            orc.add_pod(host, case.pool, e)
            ref.add_pod(host, 0, 0, (0,))
            e += 1
        if s >= ne.LADDER_NODES:
            maxima.append(max(ref.cnt[0].values()))
            _check_pod(ref, orc, case.batch, 0, *case.request, ("table", s))
    assert maxima == [1023, 1024, 1030, 1100] and ref.cnt[0][ne.TABLE_NODE] == 1030


@pytest.mark.parametrize("nn,policy", [(64, "config1"), (64, "default"), (130, "config1"), (130, "default"),
                                       (130, "config4")])
def test_walk_cases_cross_tenths_and_fill_nodes(nn, policy):
    """Part B's inputs do what they are for, per the oracle: most pods find a node, nodes
    take several commits (so their terms cross the tenth they sit above) and some fill up."""
    case = ne.walk_case(nn, policy)
    orc = case.load(OracleScheduler(case.cfg))
    c0, m0 = (a.copy() for a in orc.read_requested())
    out, _ = orc.batch(case.batch, 99)
    assert len(out) == 300 and (out >= 0).sum() > 150
    c1, m1 = orc.read_requested()
    crossed = 0  # (node, resource) whose LeastRequested tenth changed under the batch's commits
    for res, u0, u1 in (("cap_milli_cpu", c0, c1), ("cap_memory", m0, m1)):
        for n in range(nn):
            cap = int(case.arrays.nodes[res][n])
            crossed += (10 * (cap - int(u0[n]))) // cap != (10 * (cap - int(u1[n]))) // cap
    assert crossed >= nn // 2, crossed
    one = case.batch.one(0)
    one.pods["milli_cpu"][0], one.pods["memory"][0] = 3, 3
    _, fails, _ = orc.evaluate(one, 0)
    assert (fails == abi.FAIL_PODFITSRESOURCES).sum() >= 2


@pytest.mark.parametrize("name", list(ne.GATE_CASES))
def test_gate_cases_sit_on_their_bound(name):
    case = ne.gate_case(name)
    caps = np.concatenate([case.arrays.nodes["cap_milli_cpu"], case.arrays.nodes["cap_memory"]])
    used = np.concatenate([case.existing.pods["milli_cpu"], case.existing.pods["memory"]])
    reqs = np.concatenate([case.batch.pods["milli_cpu"], case.batch.pods["memory"]])
    total = int(used.max()) + sum(int(r) for r in reqs)
    inside = int(caps.max()) <= 1 << 49 and int(caps.min()) >= 0 and int(reqs.min()) >= 0 and total <= 1 << 49
    assert inside == ne.GATE_CASES[name]
    if name == "cap_at_bound":
        assert int(caps.max()) == 1 << 49
    if name == "cap_past_bound":
        assert int(caps.max()) == (1 << 49) + 1
    if name == "sum_at_bound":
        assert total == 1 << 49
    if name == "sum_past_bound":
        assert total == (1 << 49) + 1 and int(caps.max()) == 1 << 49
    if name == "one_negative_request":
        assert (reqs < 0).sum() == 1
    if name == "one_negative_capacity":
        assert (caps < 0).sum() == 1
    if name == "one_request_pair_2_62":
        assert (reqs == 1 << 62).sum() == 2 and int(reqs.min()) >= 0
    orc = case.load(OracleScheduler(case.cfg))
    out, _ = orc.batch(case.batch, 5)
    assert (out >= 0).sum() >= 30
