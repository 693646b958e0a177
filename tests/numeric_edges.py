"""Numeric-edge cases for LeastRequested and the float32 spreading terms, and an
independent reference for them.

Two halves:

  the reference   calculateScore (priorities.go:27-37), the two float32 spreading
                  terms (spreading.go:79-83, 156-160) and the weighted sum
                  (generic_scheduler.go:145-159) restated in plain Python integers and
                  numpy.float32. It calls neither the C oracle nor the package; a test
                  that finds the two restatements apart has found a bug in one of them.
  the builders    clusters and pods at the edges of the device's restatements of those
                  terms (lr_calc / lr_win / lr_win_nb / lr_fast, frac10_f32 / frac10_i32 /
                  the servers' per-pod table, the use_window gate and the int32 / int64
                  score split), as ClusterArrays / PodBatch for an engine together with
                  the same inputs as plain numbers for the reference.

No GPU is used here; tests/test_numeric_edges.py checks the builders and the reference
against the oracle on the CPU, tests/test_gpu_numeric_edges.py runs them on the device.
"""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

# =============================================================================
# the reference (plain Python; nothing below this line up to the builders
# imports the package or the oracle)
# =============================================================================
RC_OK, RC_NOFIT = 0, 1
FAIL_NONE, FAIL_RESOURCES = 0, 6  # include/kschedgpu.h KSG_FAIL_*

_MASK = (1 << 64) - 1


def i64(x: int) -> int:
    """Reduce to int64 two's complement (Go's int on amd64)."""
    x &= _MASK
    return x - (1 << 64) if x >> 63 else x


def go_div(a: int, b: int) -> int:
    """Go's int64 `/`: truncation toward zero; MinInt64 / -1 wraps."""
    if b == -1:
        return i64(-a)
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def calculate_score(requested: int, capacity: int) -> int:
    """priorities.go:27-37 in Go int64 arithmetic."""
    if capacity == 0:
        return 0
    if requested > capacity:
        return 0
    diff = i64(capacity - requested)
    return go_div(i64(diff * 10), capacity)


def frac10(num: int, den: int) -> int:
    """int(10 * (float32(num) / float32(den))): one IEEE divide, one IEEE multiply, truncate."""
    q = np.float32(num) / np.float32(den)
    return int(np.float32(10) * q)


@dataclass(frozen=True)
class Policy:
    """The weights of a policy as plain numbers (what the reference scores with)."""

    name: str
    w_lr: int = 0
    w_spread: int = 0
    w_equal: int = 0
    prefs: Tuple[Tuple[str, bool, int], ...] = ()  # (label, presence, weight)
    antis: Tuple[Tuple[str, int], ...] = ()        # (label, weight)
    fit_resources: bool = True


class RefCluster:
    """Nodes (capacities, labels), committed totals and per-host service counts; filter
    and score of one pod per node. Pods here carry no ports, disks, selectors or host,
    so PodFitsResources (predicates.go:104-145 in its closed form over the committed
    totals) is the only predicate that can fail."""

    def __init__(self, policy: Policy, cap_c: List[int], cap_m: List[int], labels: List[Dict[str, str]]):
        self.p = policy
        self.cap_c, self.cap_m, self.labels = list(cap_c), list(cap_m), labels
        self.n = len(cap_c)
        self.used_c = [0] * self.n
        self.used_m = [0] * self.n
        self.cnt: Dict[int, Dict[int, int]] = {}  # service -> host id (>= n: not a node) -> pods

    def add_pod(self, host: int, cpu: int, mem: int, svcs=()):
        if host < self.n:
            self.used_c[host] = i64(self.used_c[host] + cpu)
            self.used_m[host] = i64(self.used_m[host] + mem)
        for s in svcs:
            h = self.cnt.setdefault(s, {})
            h[host] = h.get(host, 0) + 1

    def fails(self, cpu: int, mem: int) -> List[int]:
        out = []
        for n in range(self.n):
            f = FAIL_NONE
            if self.p.fit_resources and not (cpu == 0 and mem == 0):
                fc = self.cap_c[n] == 0 or i64(self.cap_c[n] - self.used_c[n]) >= cpu
                fm = self.cap_m[n] == 0 or i64(self.cap_m[n] - self.used_m[n]) >= mem
                if not (fc and fm):
                    f = FAIL_RESOURCES
            out.append(f)
        return out

    def least_requested(self, n: int, cpu: int, mem: int) -> int:
        cs = calculate_score(i64(self.used_c[n] + cpu), self.cap_c[n])
        ms = calculate_score(i64(self.used_m[n] + mem), self.cap_m[n])
        return go_div(i64(cs + ms), 2)

    def evaluate(self, cpu: int, mem: int, svc: int):
        """-> (fail code per node, combined score per node; None where the node fails)."""
        p = self.p
        fails = self.fails(cpu, mem)
        counts = self.cnt.get(svc, {}) if svc >= 0 else {}
        maxc = max(counts.values(), default=0)
        tot = sum(counts.values())
        dom: Dict[Tuple[str, str], int] = {}
        for label, w in p.antis:  # the service's pods on fitting labelled nodes, per label value
            if w == 0:
                continue
            for n in range(self.n):
                if fails[n] == FAIL_NONE and label in self.labels[n]:
                    k = (label, self.labels[n][label])
                    dom[k] = dom.get(k, 0) + counts.get(n, 0)
        scores: List[Optional[int]] = []
        for n in range(self.n):
            if fails[n] != FAIL_NONE:
                scores.append(None)
                continue
            s = 0
            if p.w_lr:
                s = i64(s + i64(p.w_lr * self.least_requested(n, cpu, mem)))
            if p.w_spread:
                sp = frac10(maxc - counts.get(n, 0), maxc) if maxc > 0 else 10
                s = i64(s + i64(p.w_spread * sp))
            for label, w in p.antis:
                if w == 0:
                    continue
                v = 0  # an unlabelled node scores 0 (spreading.go:164-166)
                if label in self.labels[n]:
                    v = frac10(tot - dom[(label, self.labels[n][label])], tot) if tot > 0 else 10
                s = i64(s + i64(w * v))
            for label, presence, w in p.prefs:
                if w:
                    s = i64(s + i64(w * (10 if (label in self.labels[n]) == presence else 0)))
            scores.append(i64(s + p.w_equal))
        return fails, scores

    def begin(self, cpu: int, mem: int, svc: int):
        """-> (rc, max score, tie count, fail codes) of Schedule's first half."""
        fails, scores = self.evaluate(cpu, mem, svc)
        fit = [s for s in scores if s is not None]
        if not fit:
            return RC_NOFIT, 0, 0, fails
        m = max(fit)
        return RC_OK, m, fit.count(m), fails


# the naive f64-reciprocal form of calculateScore's quotient (what lr_win / lr_win_nb
# compute before their integer fix-up) and whether the fix-up has to raise it
def reciprocal_naive(u: int, cap: int) -> int:
    return int(float(u) * (10.0 / cap))


def reciprocal_wrong(u: int, cap: int) -> bool:
    return reciprocal_naive(u, cap) != (10 * u) // cap


def reciprocal_needs_up(u: int, cap: int) -> bool:
    return (reciprocal_naive(u, cap) + 1) * cap <= 10 * u


# =============================================================================
# the builders
# =============================================================================
LR_FAST_CAP = ((1 << 63) - 1) // 16     # ksg_device.h: lr_calc's fast path ends here
WIN_LR_BOUND = 1 << 49                  # ksg_internal.h KSG_WIN_LR_BOUND
TENTH_MAX = (1 << 63) // 10             # above it (cap - requested) * 10 can wrap
PRIME_49 = (1 << 49) - 81               # the largest prime below 2^49
BIG_W = (1 << 30) // 10 // 4 - 1        # tests/families.py: weights just under the int32 bound
R0 = 4                                  # the base request the slots are laid out for

# (capacity = 10 m < 2^49, u = k m exactly on a tenth) where the f64 reciprocal form
# truncates to k - 1: found once by a seeded search over such capacities (about 1.2 % of
# them), fixed here. lr_win / lr_win_nb are wrong on every one without their fix-up.
TEETH = (
    (198740704849290, 19874070484929), (233240630979120, 46648126195824), (438999366876640, 87799873375328),
    (331197941251950, 132479176500780), (166397851171600, 49919355351480), (369272832733720, 36927283273372),
    (384081866557090, 153632746622836), (130907350966100, 26181470193220), (24838293551420, 9935317420568),
    (544224028151780, 435379222521424), (21284444595990, 2128444459599), (493723281456380, 98744656291276),
    (351490428542060, 175745214271030), (515668811435760, 51566881143576), (486329649221050, 389063719376840),
    (60037988599030, 24015195439612), (346635777448200, 173317888724100), (303120421801310, 121248168720524),
    (32567954013290, 9770386203987), (540294512786390, 432235610229112), (64350295579600, 12870059115920),
    (506544698191670, 354581288734169), (107620600567240, 10762060056724), (313072145457500, 250457716366000),
    (307672064233480, 123068825693392), (158859669011280, 63543867604512), (289795445007270, 28979544500727),
    (156640144910760, 31328028982152), (459439581072690, 91887916214538), (118266974608390, 94613579686712),
    (19612496141020, 15689996912816), (73721224060350, 58976979248280), (516001149172700, 309600689503620),
    (29956513350280, 20969559345196), (318727923075510, 223109546152857), (343573882989230, 34357388298923),
    (41682586066780, 25009551640068), (285775950134130, 228620760107304), (333311854331910, 233318298032337),
    (70068547533150, 7006854753315),
    # (from the issue that asked for these tests)
    (130143110685220, 91100177479654), (136402956370490, 81841773822294), (330969015178110, 132387606071244),
    (147673448168190, 88604068900914), (132447878036740, 13244787803674),
)

SMALL_CAPS = (0, 1, 3, 7, 9, 10, 11)
# capacities whose LeastRequested term stays in [0, 10] for non-negative totals
TAME_BIG_CAPS = (WIN_LR_BOUND - 1, WIN_LR_BOUND, WIN_LR_BOUND + 1, LR_FAST_CAP, LR_FAST_CAP + 1, TENTH_MAX,
                 PRIME_49, 10 ** 6, 10 << 45, WIN_LR_BOUND - WIN_LR_BOUND % 10)
# ... and those where it does not: the x10 wraps, or the capacity is negative
WILD_BIG_CAPS = (TENTH_MAX + 1, 1 << 62, (1 << 63) - 1)
NEG_CAPS = (-1, -5, -(1 << 40))

# requests (cpu, memory) of the pending pods. Around R0: a slot laid out for u lands on
# u + 1, u, u - 1; then a zero request (fits a full node), one-sided zero requests (the
# other side's total is the committed one), and 2^62.
TAME_REQUESTS = ((R0, R0), (R0 - 1, R0 - 1), (R0 + 1, R0 + 1), (0, 0), (R0, 0), (0, R0),
                 (1 << 62, 1 << 62), (1 << 62, 0))
# ... and negative ones
WILD_REQUESTS = TAME_REQUESTS + ((-1, -1), (-(1 << 41), R0), (R0, -(1 << 41)), (-(1 << 62), -(1 << 62)),
                                 (-(1 << 41), -(1 << 41)))


def _tenth_slots(cap: int, clamp: bool) -> List[Tuple[int, int]]:
    """(capacity, committed total) so that with a request of R0 the free amount
    u = cap - committed - R0 is ceil(k cap / 10), k = 0..10 (requests R0 -/+ 1 give the
    neighbours). clamp: no negative committed total (k = 10 then starts R0 short)."""
    out = []
    for k in range(11):
        u = -((-k * cap) // 10)
        used = cap - u - R0
        out.append((cap, max(used, 0) if clamp else used))
    return out


def _slots(kind: str) -> List[Tuple[int, int]]:
    tame = kind == "tame"
    s: List[Tuple[int, int]] = []
    for cap in SMALL_CAPS if tame else (0, 1, 10):
        s += [(cap, used) for used in range(cap + 2)]  # every total up to requested = cap + 1
    for cap in TAME_BIG_CAPS if tame else (WIN_LR_BOUND, LR_FAST_CAP + 1, TENTH_MAX, 10 ** 6):
        s += _tenth_slots(cap, tame)
    for cap in (WIN_LR_BOUND, LR_FAST_CAP, TENTH_MAX) if tame else WILD_BIG_CAPS:
        s += [(cap, cap), (cap, cap + 1 if cap + 1 < 1 << 63 else cap - 1)]  # a full node, and one past full
    if tame:
        s += [(cap, cap - u - R0) for cap, u in TEETH]
    else:
        for cap in WILD_BIG_CAPS:
            s += _tenth_slots(cap, False)
        # negative capacities: requested <= cap scores ((cap - requested) * 10) / cap <= 0,
        # far below -2^31 for totals like -2^41 (the int32 narrowing the exact kernels had)
        for cap in NEG_CAPS:
            for total in (cap, cap - 1, cap - 2, cap - 7, 10 * cap, -(1 << 41), -(1 << 41) - 3, -(1 << 62),
                          -(1 << 63) + 5, cap + 1, 0):
                s.append((cap, i64(total - R0)))
    return s


@dataclass
class EdgeCase:
    """One cluster at the edges for one policy: engine inputs and the same as plain numbers."""

    kind: str
    policy: Policy
    cfg: object                 # abi.KsgConfig
    arrays: object              # engine.ClusterArrays
    existing: object            # engine.PodBatch: the pods already on the nodes
    existing_hosts: List[int]
    batch: object               # engine.PodBatch: the pending pods
    cap_c: List[int] = field(default_factory=list)
    cap_m: List[int] = field(default_factory=list)
    labels: List[Dict[str, str]] = field(default_factory=list)
    existing_plain: List[Tuple[int, int, int, Tuple[int, ...]]] = field(default_factory=list)  # host, cpu, mem, svcs
    requests: List[Tuple[int, int]] = field(default_factory=list)

    def load(self, engine):
        engine.set_cluster(self.arrays)
        for i, h in enumerate(self.existing_hosts):
            engine.add_pod(h, self.existing, i)
        return engine

    def reference(self) -> RefCluster:
        ref = RefCluster(self.policy, self.cap_c, self.cap_m, self.labels)
        for h, c, m, svcs in self.existing_plain:
            ref.add_pod(h, c, m, svcs)
        return ref


N_EDGE_NODES = 130  # two full 64-node words and a partial one


def policies() -> Dict[str, Tuple[Policy, object]]:
    """name -> (the weights as plain numbers, the factory's SchedulerConfig)."""
    from kubernetes_amd import factory, workload
    from tests import families

    default_preds = [{"name": n} for n in ("PodFitsPorts", "PodFitsResources", "NoDiskConflict", "MatchNodeSelector",
                                           "HostName")]
    anti = factory.create_from_config({
        "predicates": default_preds,
        "priorities": [{"name": "LeastRequestedPriority", "weight": 1}, {"name": "ServiceSpreadingPriority", "weight": 1},
                       {"name": "NumericEdgeZoneSpread", "weight": 1,
                        "argument": {"serviceAntiAffinity": {"label": "zone"}}}]})
    return {
        "config1": (Policy("config1", w_lr=1), workload.config1()),
        "default": (Policy("default", w_lr=1, w_spread=1), workload.config_default()),
        "big": (Policy("big", w_lr=BIG_W, w_spread=BIG_W, prefs=(("rack", True, BIG_W),)),
                families.build("big_weights", 1, 1).config),
        "huge": (Policy("huge", w_lr=(3 << 40) + 7, w_spread=5 << 39, prefs=(("rack", True, (1 << 62) + 12345),),
                        antis=(("zone", -(3 << 40)),)),
                 families.build("huge_weights", 1, 1).config),
        "anti": (Policy("anti", w_lr=1, w_spread=1, antis=(("zone", 1),)), anti),
    }


def _nodes(n: int, seed: int):
    """workload.make_nodes with the rack label off every third node and the zone label off
    every fifth (LabelPreference 0, ServiceAntiAffinity's unlabelled 0)."""
    from kubernetes_amd import workload

    nodes = workload.make_nodes(n, workload._SM(seed))
    for i, nd in enumerate(nodes):
        if i % 3 == 0:
            del nd.metadata.labels["rack"]
        if i % 5 == 0:
            del nd.metadata.labels["zone"]
    return nodes


def _ingest(nodes, n_existing: int, n_pending: int, config, n_apps: int = 1, seed: int = 5):
    """-> (compiled config, ClusterArrays, existing PodBatch, pending PodBatch, view); pods of
    services a0..a{n_apps-1} without ports, disks or selectors."""
    from kubernetes_amd import ingest, workload

    rng = workload._SM(seed)
    pods = workload.make_pods(n_existing + n_pending, rng, n_apps=n_apps, port_frac=0.0, pd_frac=0.0, sel_frac=0.0)
    it = ingest.Interner()
    for k in config.label_keys():
        it.key_id(k)
    view = ingest.ClusterView(nodes, workload.make_services(n_apps), it)
    aff = config.affinity_labels()
    existing = ingest.ingest_pods(view, pods[:n_existing], uids=list(range(1, n_existing + 1)), aff_labels=aff)
    batch = ingest.ingest_pods(view, pods[n_existing:], uids=list(range(10 ** 6, 10 ** 6 + n_pending)), aff_labels=aff)
    config.max_conflict_keys = 64
    return config.compile(it.key_id), view.arrays, existing, batch, view


@functools.lru_cache(maxsize=None)
def edge_case(kind: str, policy_name: str) -> EdgeCase:
    """kind "tame": every LeastRequested term stays in [0, 10] (capacities 0 .. 2^63/10,
    non-negative totals; the reciprocal's teeth, the 2^49 and LR_FAST_CAP switches, the
    wrapping divide above LR_FAST_CAP). kind "wild": negative capacities, capacities
    past 2^63/10, negative committed totals and requests, whose terms leave that range."""
    policy, config = policies()[policy_name]
    slots = _slots(kind)
    assert len(slots) <= 2 * N_EDGE_NODES, len(slots)
    # a slot whose node cannot take R0 hides the node's other resource for that pod: pair
    # those with each other (cpu, memory), then the rest; what is left over repeats slots
    tight = [s for s in slots if s[0] != 0 and i64(s[0] - s[1]) < R0 + 1]
    roomy = [s for s in slots if not (s[0] != 0 and i64(s[0] - s[1]) < R0 + 1)]
    order = tight + roomy
    pairs = [(order[i], order[i + 1] if i + 1 < len(order) else order[0]) for i in range(0, len(order), 2)]
    fill = [s for s in roomy if s[0] > 11]
    while len(pairs) < N_EDGE_NODES:  # (the same slots again, cpu and memory swapped)
        j = len(pairs)
        pairs.append((fill[(2 * j + 1) % len(fill)], fill[(2 * j) % len(fill)]))
    n = N_EDGE_NODES
    extra = [i % 4 for i in range(n)]  # zero-request pods of the service: counts 1..4 per node
    requests = list(TAME_REQUESTS if kind == "tame" else WILD_REQUESTS)
    cfg, arrays, existing, batch, _ = _ingest(_nodes(n, 77), n + sum(extra), len(requests), config)
    case = EdgeCase(kind, policy, cfg, arrays, existing, [], batch, requests=requests)
    e = 0
    for i, ((cap_c, used_c), (cap_m, used_m)) in enumerate(pairs):
        arrays.nodes["cap_milli_cpu"][i] = cap_c
        arrays.nodes["cap_memory"][i] = cap_m
        case.cap_c.append(cap_c)
        case.cap_m.append(cap_m)
        for cpu, mem in [(used_c, used_m)] + [(0, 0)] * extra[i]:
            existing.pods["milli_cpu"][e] = cpu
            existing.pods["memory"][e] = mem
            case.existing_hosts.append(i)
            case.existing_plain.append((i, cpu, mem, (0,)))
            e += 1
    for j, (cpu, mem) in enumerate(requests):
        batch.pods["milli_cpu"][j] = cpu
        batch.pods["memory"][j] = mem
    case.labels = [dict(nd.metadata.labels) for nd in _nodes(n, 77)]
    return case


def lr_points(case: EdgeCase):
    """Every (capacity, free amount u) a fitting node's LeastRequested term is computed at,
    over all pending pods and both resources, with 0 < capacity <= 2^49 and 0 <= u."""
    ref = case.reference()
    pts = set()
    for cpu, mem in case.requests:
        fails = ref.fails(cpu, mem)
        for n in range(ref.n):
            if fails[n] != FAIL_NONE:
                continue
            for cap, total in ((ref.cap_c[n], i64(ref.used_c[n] + cpu)), (ref.cap_m[n], i64(ref.used_m[n] + mem))):
                if 0 < cap <= WIN_LR_BOUND and 0 <= total <= cap:
                    pts.add((cap, cap - total))
    return pts


# ---- part B: commits that walk a node's term across a tenth ------------------------
@dataclass
class WalkCase:
    cfg: object
    arrays: object
    existing: object
    existing_hosts: List[int]
    batch: object

    def load(self, engine):
        engine.set_cluster(self.arrays)
        for i, h in enumerate(self.existing_hosts):
            engine.add_pod(h, self.existing, i)
        return engine


@functools.lru_cache(maxsize=None)
def walk_case(n_nodes: int, policy_name: str, n_pods: int = 300) -> WalkCase:
    """Every node's free cpu and memory sit one or two units above a tenth (the fifth or the
    sixth) of a capacity in [2^20, 2^48]; the pods ask for 1..3 units of each, so successive commits on a node carry
    its LeastRequested term over the boundary (the resolvers' re-checks, lr_win_nb). Every
    ninth node has 2..4 units left in all: a commit or two and PodFitsResources fails there.
    The largest committed total plus every request of the batch stays below 2^49."""
    from kubernetes_amd import workload

    config = workload.config4() if policy_name == "config4" else policies()[policy_name][1]
    rnd = random.Random(4900 + n_nodes)
    n_apps = 3
    cfg, arrays, existing, batch, _ = _ingest(workload.make_nodes(n_nodes, workload._SM(78)), n_nodes, n_pods, config,
                                              n_apps=n_apps, seed=9)
    hosts = []
    for i in range(n_nodes):
        used = []
        for res in ("cap_milli_cpu", "cap_memory"):
            cap = rnd.randrange(1 << 20, 1 << 48)
            if i % 9 == 4:
                u = rnd.randrange(2, 5)  # nearly full
            else:
                k = rnd.choice((5, 6))  # (two levels only: every node is near the top score, and is chosen)
                u = -((-k * cap) // 10) + rnd.randrange(1, 3)
            arrays.nodes[res][i] = cap
            used.append(cap - u)
        existing.pods["milli_cpu"][i], existing.pods["memory"][i] = used
        hosts.append(i)
    for j in range(n_pods):
        batch.pods["milli_cpu"][j] = rnd.randrange(1, 4)
        batch.pods["memory"][j] = rnd.randrange(1, 4)
    top = max(int(existing.pods["milli_cpu"].max()), int(existing.pods["memory"].max()))
    assert top + int(batch.pods["milli_cpu"].sum() + batch.pods["memory"].sum()) <= WIN_LR_BOUND
    return WalkCase(cfg, arrays, existing, hosts, batch)


# ---- part C: the use_window gate ------------------------------------------------
GATE_CASES = {
    # name: (what is set, which side of the bound, whether the window path may run)
    "cap_at_bound": True, "cap_past_bound": False,
    "sum_at_bound": True, "sum_past_bound": False,
    "requests_non_negative": True, "one_negative_request": False,
    "capacities_non_negative": True, "one_negative_capacity": False,
    # (one pod asking 2^62 of each: cpu + memory overflows a signed add before any clamp)
    "one_request_pair_2_62": False,
}


def gate_case(name: str) -> WalkCase:
    """A 64-node, 40-pod resources-only batch on one side of one of use_window's bounds
    (ksg_runtime.cpp): the largest capacity, the largest committed total plus the batch's
    requests, a negative request, a negative capacity, a request pair whose sum overflows."""
    from kubernetes_amd import workload

    n_nodes, n_pods = 64, 40
    cfg, arrays, existing, batch, _ = _ingest(workload.make_nodes(n_nodes, workload._SM(79)), n_nodes, n_pods,
                                              policies()["config1"][1], seed=10)
    rnd = random.Random(64)
    for i in range(n_nodes):
        for res, req in (("cap_milli_cpu", "milli_cpu"), ("cap_memory", "memory")):
            cap = rnd.randrange(1 << 20, 1 << 30)
            arrays.nodes[res][i] = cap
            existing.pods[req][i] = cap - rnd.randrange(5, 60)
    for j in range(n_pods):
        batch.pods["milli_cpu"][j] = rnd.randrange(1, 4)
        batch.pods["memory"][j] = rnd.randrange(1, 4)
    total = int(batch.pods["milli_cpu"].sum() + batch.pods["memory"].sum())
    if name in ("cap_at_bound", "cap_past_bound"):
        arrays.nodes["cap_milli_cpu"][7] = WIN_LR_BOUND + (name == "cap_past_bound")
    elif name in ("sum_at_bound", "sum_past_bound"):
        arrays.nodes["cap_memory"][9] = WIN_LR_BOUND
        existing.pods["memory"][9] = WIN_LR_BOUND - total + (name == "sum_past_bound")
    elif name == "one_negative_request":
        batch.pods["milli_cpu"][17] = -1
    elif name == "one_negative_capacity":
        arrays.nodes["cap_memory"][11] = -1
    elif name == "one_request_pair_2_62":
        batch.pods["milli_cpu"][17] = batch.pods["memory"][17] = 1 << 62
    else:
        assert name in ("requests_non_negative", "capacities_non_negative"), name
    return WalkCase(cfg, arrays, existing, list(range(n_nodes)), batch)


# ---- part C: the spreading / anti-affinity ladder ---------------------------------
# maxCount steps of the ladder: every value 1..300. (If the ladder has to be thinned,
# 25, 41, 47, 63, 64, 65, 127, 128, 255 and 256 stay: at 25, 41 and 47 a reciprocal-multiply
# divide differs from the IEEE one, the others sit at the table's and the words' edges.)
LADDER_TOP = 300
LADDER_NODES = 64


@dataclass
class LadderCase:
    policy: Policy
    cfg: object
    arrays: object
    pool: object        # PodBatch: zero-request pods of the service, added one by one
    batch: object       # PodBatch: the one pending pod
    cap_c: List[int]
    cap_m: List[int]
    labels: List[Dict[str, str]]
    request: Tuple[int, int]


@functools.lru_cache(maxsize=None)
def ladder_case(policy_name: str, n_pool: int) -> LadderCase:
    """64 ordinary nodes, one service, a pool of zero-request pods of it to place (on nodes,
    or on a host id past the node list: a pod whose host is not a node still counts for
    maxCount and the service's total), and one pending pod of the service."""
    policy, config = policies()[policy_name]
    nodes = _nodes(LADDER_NODES, 80)
    cfg, arrays, pool, batch, _ = _ingest(nodes, n_pool, 1, config, seed=11)
    pool.pods["milli_cpu"][:] = 0
    pool.pods["memory"][:] = 0
    return LadderCase(policy, cfg, arrays, pool, batch, [int(v) for v in arrays.nodes["cap_milli_cpu"]],
                      [int(v) for v in arrays.nodes["cap_memory"]], [dict(nd.metadata.labels) for nd in nodes],
                      (int(batch.pods["milli_cpu"][0]), int(batch.pods["memory"][0])))


def ladder_steps():
    """The ladder as (host id, pods to add there, compare after?) steps: node j filled to
    j pods, j = 1..63 (maxCount = j, counts 0..j present), then pods on a host outside the
    node list one by one up to LADDER_TOP (the first 63 of them change nothing)."""
    steps = [(j, j, True) for j in range(1, LADDER_NODES)]
    steps.append((LADDER_NODES, LADDER_NODES - 1, False))
    steps += [(LADDER_NODES, 1, True) for _ in range(LADDER_NODES, LADDER_TOP + 1)]
    return steps


LADDER_POOL = sum(k for _, k, _ in ladder_steps())

# the servers' per-pod table holds KSG_NT = 1024 entries (ksg_serve.hip): (host, pods to
# add) steps, compared after each: one node's count at the table's last entry, just past
# it, then maxCount raised past it through an outside host
TABLE_NODE = 35  # (35 % 7 == 0: it starts empty)
TABLE_STEPS = ((TABLE_NODE, 1023), (TABLE_NODE, 1), (TABLE_NODE, 6), (LADDER_NODES, 1100))
TABLE_POOL = sum(k for _, k in TABLE_STEPS) + sum(j % 7 for j in range(LADDER_NODES))
