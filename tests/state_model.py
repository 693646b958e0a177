"""A plain model of the mutable per-node pod state, and operation sequences to audit it with.

The state the HIP library keeps in HBM (used_cpu / used_mem / scalar_used, the host-port / GCE-PD
bitmaps, the per-service counts, bitmaps, maxima, totals and peers: include/kschedgpu.h,
ksg_read_state) is a pure function of the ordered list of live pods and their hosts. `StateModel`
holds that list and computes every array from scratch with Python integers; nothing is updated
incrementally, which is what makes it a reference for the three writers of the device state (the
kernels' commit code, the host mirror's patches, ksg_batch_unwind).

`make_sequence` builds a seeded sequence of operations (add / remove / batch / batch_draws /
begin+commit / batch_unwind and re-batch / read-only queries / calls that must fail / set_cluster /
remove everything) and `run_sequence` applies it in lockstep to the model, to the C restatement
and, when given one, to an engine (DeviceScheduler), comparing every array after every operation.
tests/test_state_model.py runs the sequences on the CPU and asserts their coverage;
tests/test_gpu_state.py runs the same ones against the device under every state writer.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from kubernetes_amd import abi, ingest, workload
from kubernetes_amd.api import ContainerPort
from kubernetes_amd.engine import PodBatch
from oracle.pyoracle import OracleScheduler
from tests import families
from tests.ext_cases import ExtCase

_M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15  # splitmix64's step: one draw per placed pod (ksg_schedule_batch)
FAT_CPU = 10 ** 7           # milli-cpu no node has: a pod that finds no node under PodFitsResources
MAX_KEYS = 64
POOL = 640                  # pods per sequence; the last RESERVED are for add_pod / begin / hand-made pods
RESERVED = 96


def _wrap(x: int) -> int:
    """Go's int64 wrap."""
    return ((x + (1 << 63)) & _M64) - (1 << 63)


@dataclass
class PodRec:
    uid: int
    host: int
    cpu: int
    mem: int
    keys: list      # conflict-key ids, ports then PDs, repeats kept
    svcs: list      # every service that selects the pod
    scalar: tuple   # extended-resource requests


def pod_rec(batch: PodBatch, i: int, host: int, n_scalar: int = 0) -> PodRec:
    p, ids = batch.pods[i], batch.ids
    keys = [int(x) for x in ids[int(p["ports_off"]): int(p["ports_off"]) + int(p["n_ports"])]]
    keys += [int(x) for x in ids[int(p["pds_off"]): int(p["pds_off"]) + int(p["n_pds"])]]
    svcs = [int(x) for x in ids[int(p["svcs_off"]): int(p["svcs_off"]) + int(p["n_svcs"])]]
    sc = tuple(int(x) for x in batch.ext[i]["scalar"][:n_scalar]) if batch.ext is not None else (0,) * n_scalar
    return PodRec(int(p["uid"]), int(host), int(p["milli_cpu"]), int(p["memory"]), keys, svcs, sc)


class StateModel:
    """The ordered list of live pods; arrays() recomputes the whole state from it."""

    def __init__(self, n_nodes: int, n_services: int, n_keys: int, n_scalar: int = 0):
        self.N, self.S, self.K, self.R = n_nodes, n_services, n_keys, n_scalar
        self.live: list = []  # PodRec, in order of addition

    def add(self, rec: PodRec):
        assert all(p.uid != rec.uid for p in self.live), rec.uid
        self.live.append(rec)

    def remove(self, uid: int):
        self.live = [p for p in self.live if p.uid != uid]

    def has(self, uid: int) -> bool:
        return any(p.uid == uid for p in self.live)

    def host_counts(self, s: int) -> dict:
        """host -> live pods of service s on it, hosts outside the node list included."""
        c: dict = {}
        for p in self.live:
            if s in p.svcs:
                c[p.host] = c.get(p.host, 0) + p.svcs.count(s)
        return c

    def arrays(self) -> dict:
        N, S, K, R = self.N, self.S, self.K, self.R
        nw = (N + 63) // 64
        cpu, mem = [0] * N, [0] * N
        sc = [[0] * N for _ in range(R)]
        keymap = [[0] * nw for _ in range(K)]
        cnt = [[0] * N for _ in range(S)]
        bits = [[0] * nw for _ in range(S)]
        total, peer = [0] * S, [-1] * S
        for p in self.live:
            on_node = p.host < N
            if on_node:
                cpu[p.host] = _wrap(cpu[p.host] + p.cpu)
                mem[p.host] = _wrap(mem[p.host] + p.mem)
                for r in range(R):
                    sc[r][p.host] = _wrap(sc[r][p.host] + p.scalar[r])
                for k in p.keys:
                    keymap[k][p.host >> 6] |= 1 << (p.host & 63)
            for s in p.svcs:
                total[s] += 1
                if on_node:
                    cnt[s][p.host] += 1
                    bits[s][p.host >> 6] |= 1 << (p.host & 63)
                if peer[s] == -1:  # the earliest-added live member
                    peer[s] = p.host if on_node else -2
        mx = [max(self.host_counts(s).values(), default=0) for s in range(S)]  # spreading.go:72-80
        return {
            "used_cpu": np.array(cpu, np.int64).reshape(N), "used_mem": np.array(mem, np.int64).reshape(N),
            "scalar_used": np.array(sc, np.int64).reshape(R, N),
            "keymap": np.array(keymap, np.uint64).reshape(K, nw), "svc_cnt": np.array(cnt, np.int32).reshape(S, N),
            "svc_bits": np.array(bits, np.uint64).reshape(S, nw), "svc_max": np.array(mx, np.int32).reshape(S),
            "svc_total": np.array(total, np.int32).reshape(S), "svc_peer": np.array(peer, np.int32).reshape(S),
        }


# ---- reading an engine's state ----------------------------------------------------------------
FIELDS = ("used_cpu", "used_mem", "scalar_used", "keymap", "svc_cnt", "svc_bits", "svc_max", "svc_total", "svc_peer")
_BITMAPS = ("keymap", "svc_bits")
_PER_NODE = ("used_cpu", "used_mem")


def engine_state(sched, n_scalar: int) -> dict:
    st = dict(sched.read_state())
    st["used_cpu"], st["used_mem"] = sched.read_requested()
    st["scalar_used"] = sched.read_ext_used() if n_scalar else np.zeros((0, sched.n_nodes), np.int64)
    return st


def first_diff(name: str, got, want):
    """None when equal, else a description of the first differing (row, node)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{name}: {got.dtype}{got.shape} vs {want.dtype}{want.shape}"
    if np.array_equal(got, want):
        return None
    if name in _BITMAPS:  # name the node, not the word
        g = np.unpackbits(np.ascontiguousarray(got).view(np.uint8), bitorder="little").reshape(got.shape[0], -1)
        w = np.unpackbits(np.ascontiguousarray(want).view(np.uint8), bitorder="little").reshape(want.shape[0], -1)
        r, n = (int(x) for x in np.argwhere(g != w)[0])
        return f"{name}[row {r}, node {n}]: bit {int(g[r, n])}, want {int(w[r, n])}"
    ix = tuple(int(x) for x in np.argwhere(got != want)[0])
    where = f"node {ix[0]}" if name in _PER_NODE else f"row {ix[0]}" + (f", node {ix[1]}" if len(ix) > 1 else "")
    return f"{name}[{where}]: {int(got[ix])}, want {int(want[ix])}"


def diff_states(got: dict, want: dict):
    for f in FIELDS:
        d = first_diff(f, got[f], want[f])
        if d:
            return d
    return None


# ---- sequences ----------------------------------------------------------------------------------
POLICIES = {"plain": workload.config_default, "config4": workload.config4}
SOURCES = {"multi": "multi_service", "ns": "namespaces", "hosts": "existing_hosts", "ext": "namespaces"}


class _PoolCase:
    """The shape of tests.helpers.Case over a family's pods under one of POLICIES."""

    def __init__(self, source: str, policy: str, nn: int, seed: int):
        w = families.build(SOURCES[source], nn, POOL, seed)
        existing = list(w.existing)[:9]  # the family's pods with a Status.Host: the pool's last ones
        pods = list(w.pods)[:POOL - len(existing)] + existing
        assert len(pods) == POOL
        for i, p in enumerate(pods):  # the dense pools of test_gpu_fuzz._case: three ports, five PDs
            c = p.spec.containers[0]
            if not c.ports and i % 4 == 0:
                c.ports = [ContainerPort(container_port=80, host_port=9000 + i % 3)]
            for cp in c.ports:
                cp.host_port = 9000 + (cp.host_port % 3)
            for v in p.spec.volumes:
                if v.gce_persistent_disk is not None:
                    v.gce_persistent_disk.pd_name = f"pd-{int(v.gce_persistent_disk.pd_name.split('-')[1]) % 5}"
        cfg = POLICIES[policy]()
        cfg.max_conflict_keys = MAX_KEYS
        self.api_pods = pods
        self.it = ingest.Interner()
        for k in cfg.label_keys():
            self.it.key_id(k)
        self.view = ingest.ClusterView(w.nodes, w.services, self.it)
        self.aff = cfg.affinity_labels()
        self.batch = ingest.ingest_pods(self.view, pods, uids=list(range(1000, 1000 + POOL)), aff_labels=self.aff)
        self.cfg = cfg.compile(self.it.key_id)
        # pool index -> host id of the pods that came with a Status.Host ("" and gone nodes are
        # hosts outside the node list: ids at or above n_nodes)
        self.preset = {POOL - len(existing) + j: self.view.host_id(p.status.host) for j, p in enumerate(existing)}


@dataclass
class Sequence:
    name: str
    cfg: object
    arrays: object
    pool: PodBatch
    n_scalar: int
    ext: object            # ExtCase or None
    ops: list
    coverage: dict = field(default_factory=dict)

    @property
    def n_nodes(self):
        return self.arrays.n_nodes

    def load(self, sched, first: bool):
        if self.ext is not None:
            if first:
                sched.set_extensions(self.ext.kcfg)
            sched.set_cluster(self.arrays)
            sched.set_node_ext(*self.ext.node_arrays)
        else:
            sched.set_cluster(self.arrays)


def _slice(b: PodBatch, lo: int, hi: int) -> PodBatch:
    return PodBatch(b.pods[lo:hi].copy(), b.ids, None if b.ext is None else b.ext[lo:hi].copy())


def _hand_made(pool: PodBatch, first: int):
    """Pods the ingest never produces, written into pool[first ..]: a key listed twice, a port and
    a PD together, and two pods sharing one key (they meet on a node only through add_pod).
    -> (ids, {role: pool index})."""
    extra = [0, 0, 1, 3, 2, 2]
    base = len(pool.ids)
    ids = np.concatenate([pool.ids, np.asarray(extra, np.uint32)])
    # (pool index, ports (offset, count), PDs (offset, count)); pods 3 and 7 meet the kernels'
    # commit code in the first batch, the others go through add_pod and begin / commit
    for j, (i, po, pn, do, dn) in enumerate(((first, 0, 2, 0, 0), (first + 1, 2, 1, 3, 1), (first + 2, 4, 1, 0, 0),
                                             (first + 3, 5, 1, 0, 0), (3, 0, 2, 0, 0), (7, 2, 1, 3, 1))):
        p = pool.pods[i]
        p["ports_off"], p["n_ports"] = base + po, pn
        p["pds_off"], p["n_pds"] = base + do, dn
        p["n_sel"] = 0
        if j in (2, 3):  # in no service, so that no removal chosen by service takes one of the pair early
            p["n_svcs"], p["service"] = 0, -1
    return ids, {"twice": first, "port_pd": first + 1, "share_a": first + 2, "share_b": first + 3}


def make_sequence(source: str, policy: str, nn: int, seed: int) -> Sequence:
    """One seeded operation sequence (about 40 operations) over `nn` nodes."""
    rng = workload._SM(77000 + seed)
    case = _PoolCase(source, policy, nn, seed)
    ext = None
    if source == "ext":
        ext = ExtCase(nn=nn, npods=POOL, seed=seed, case=case)
        pool = PodBatch(ext.batch.pods.copy(), ext.batch.ids, ext.batch.ext.copy())
    else:
        pool = PodBatch(case.batch.pods.copy(), case.batch.ids, None)
    n_scalar = int(ext.kcfg.n_scalar) if ext is not None else 0
    res0 = POOL - RESERVED
    ids, hand = _hand_made(pool, res0)
    pool = PodBatch(pool.pods, ids, pool.ext)
    free = list(range(res0 + 4, POOL))  # reserved pods not yet used

    def svcs_of(i):
        p = pool.pods[i]
        return [int(x) for x in pool.ids[int(p["svcs_off"]): int(p["svcs_off"]) + int(p["n_svcs"])]]

    def take(pred=lambda i: True):
        for i in free:
            if pred(i):
                free.remove(i)
                return i
        raise AssertionError("reserved pods exhausted")

    # the service with the most reserved members carries the stack and the peer moves
    tally: dict = {}
    for i in free:
        for s in svcs_of(i)[:1]:
            tally[s] = tally.get(s, 0) + 1
    s0 = max(sorted(tally), key=lambda s: tally[s])
    in_s0 = lambda i: s0 in svcs_of(i)
    node = lambda: int(rng.below(nn))
    off = [nn + 1 + int(rng.below(3)), nn + 7]  # hosts outside the node list

    ops = []
    # the family's own existing pods on their Status.Host: two distinct hosts, off-list ones first
    seen_hosts = set()
    for i, h in sorted(case.preset.items(), key=lambda kv: (kv[1] < nn, kv[0])):
        if len(seen_hosts) < 2 and h not in seen_hosts:
            seen_hosts.add(h)
            ops.append(("add", i, h))
    free = [i for i in free if i not in case.preset]
    h_shared, h_last = node(), nn - 1  # nn - 1: the single node of a last word at 65 and 4,097
    ops.append(("add", take(in_s0), node()))                 # the service's oldest member, on a node
    for _ in range(4):                                       # its maximum, held by an off-list host alone
        ops.append(("add", take(in_s0), off[0]))
    ops.append(("add", take(in_s0), h_last))
    ops.append(("add", hand["share_a"], h_shared))           # two pods sharing a key on one node
    ops.append(("add", hand["share_b"], h_shared))
    ops.append(("add", hand["twice"], h_last))               # a key listed twice

    cursor = 0

    def batch_op(kind):
        nonlocal cursor
        n = 30 + int(rng.below(91))
        lo, hi = cursor, cursor + n
        cursor = hi
        assert hi <= res0
        for j in (lo + (2 * n) // 3, lo + (3 * n) // 4, hi - 1):  # pods that find no node, late in the batch
            pool.pods[j]["milli_cpu"] = FAT_CPU
        return ("batch", lo, hi, kind)

    kinds = ["seed", "draws", "seed", "draws"] if rng.below(2) else ["draws", "seed", "draws", "seed"]
    queries = ["explain", "prioritize", "headroom", "explain_without"]
    q0 = int(rng.below(4))
    queries = queries[q0:] + queries[:q0]
    second = seed % 2 == 0  # a second unwind, on the re-batch

    ops.append(batch_op(kinds[0]))
    ops.append(("query", queries[0]))
    ops.append(("remove", "peer"))
    ops.append(("fail", "batch_live_uid"))
    ops.append(("remove", "max"))
    ops.append(batch_op(kinds[1]))
    ops.append(("unwind", "first"))
    ops.append(("rebatch",))
    ops.append(("query", queries[1]))
    ops.append(("begin_commit", take()))
    ops.append(("begin_abandon", take()))
    ops.append(("begin_commit", hand["port_pd"]))
    ops.append(("remove", "shared"))
    ops.append(batch_op(kinds[2]))
    ops.append(("fail", "unwind_k_ge_n"))
    ops.append(("fail", "unwind_nofit"))
    ops.append(("unwind", "mid"))
    ops.append(("rebatch",))
    if second:
        ops.append(("unwind", "last"))
        ops.append(("rebatch",))
    ops.append(("query", queries[2]))
    ops.append(("remove", "peer"))
    ops.append(("fail", "remove_unknown"))
    ops.append(("set_cluster",))
    ops.append(("add", take(in_s0), off[0]))
    ops.append(("add", take(in_s0), node()))
    ops.append(batch_op(kinds[3]))
    ops.append(("query", queries[3]))
    ops.append(("unwind", "last" if not second else "mid"))
    ops.append(("rebatch",))
    ops.append(("remove", "any"))
    ops.append(("begin_commit", take()))
    ops.append(("remove_all",))
    name = f"{source}-{policy}-{nn}-s{seed}"
    return Sequence(name, case.cfg, case.view.arrays, pool, n_scalar, ext, ops)


# (source, policy, nodes, seed). 65 and 130 cross word edges; 4,097 is 65 words with a single node
# in the last one, for one plain and one config 4 sequence. "ext": every extension on.
SEQUENCES = [("multi", "plain", 65, 1), ("ns", "plain", 130, 2), ("hosts", "plain", 700, 3), ("multi", "plain", 4097, 4),
             ("multi", "config4", 65, 5), ("ns", "config4", 130, 6), ("hosts", "config4", 700, 7),
             ("multi", "config4", 4097, 8), ("ext", "plain", 65, 9), ("ext", "plain", 130, 10), ("ext", "plain", 700, 11)]


# ---- the runner ---------------------------------------------------------------------------------
class _Fail(AssertionError):
    pass


def run_sequence(seq: Sequence, engine=None, model_cls=StateModel, check_oracle: bool = True) -> dict:
    """Apply seq.ops to the model, the C restatement and `engine` (a fresh DeviceScheduler, or
    None) in lockstep; after every operation every array of each must equal the model's.
    -> coverage counters of the sequence. Raises AssertionError naming the operation index, the
    operation, the array and the first differing (row, node)."""
    N, R = seq.n_nodes, seq.n_scalar
    S = int(seq.arrays.n_services)
    pool = seq.pool
    orc = OracleScheduler(seq.cfg)
    seq.load(orc, True)
    if engine is not None:
        seq.load(engine, True)
    model = model_cls(N, S, MAX_KEYS, R)
    rng_state = 0xC0FFEE + N
    draws = np.random.default_rng(N + len(seq.ops)).integers(0, 1 << 63, size=4 * POOL, dtype=np.uint64)
    dcur = 0
    last = None  # the last batch: dict(batch, out, kind, rng_before / d0)
    cov = {"batch_pods": 0, "batch_placed": 0, "max_undone": 0, "peer_moved": 0, "max_lowered": 0,
           "shared_left": 0, "offlist_audits": 0, "windows": 0, "audits": 0, "nofit_after_mid": 0}
    where = ["", None]

    def fail(msg):
        raise _Fail(f"{seq.name} op {where[0]} {where[1]}: {msg}")

    def audit():
        want = model.arrays()
        cov["audits"] += 1
        if any(p.host >= N for p in model.live):
            cov["offlist_audits"] += 1
        if check_oracle:
            d = diff_states(engine_state(orc, R), want)
            if d:
                fail(f"oracle vs model: {d}")
        if engine is not None:
            d = diff_states(engine_state(engine, R), want)
            if d:
                fail(f"device vs model: {d}")
        return want

    def both(fn):
        a = fn(orc)
        if engine is not None:
            fn(engine)
        return a

    def begin(s, b, i):
        """(rc, max, ties); a ServiceAffinity peer on an unknown host is (KSG_ERR_NOPEER, 0, 0)."""
        try:
            return tuple(s.begin(b, i)[:3])
        except Exception as e:  # KsgError on the device, RuntimeError from the restatement
            if getattr(e, "code", None) == abi.KSG_ERR_NOPEER or str(e).endswith(f"rc={abi.KSG_ERR_NOPEER}"):
                return (abi.KSG_ERR_NOPEER, 0, 0)
            raise

    def orc_draws_batch(b, dr):
        out = np.empty(len(b), np.int32)
        used = 0
        for i in range(len(b)):
            rc, _, k = begin(orc, b, i)
            if rc == abi.KSG_OK:
                out[i] = orc.commit(int(dr[used]) % k)
                used += 1
            else:
                out[i] = -2 if rc == abi.KSG_ERR_NOPEER else -1  # (KSG_OUT_ERROR, KSG_OUT_NOFIT)
        return out, used

    def do_batch(b):
        nonlocal rng_state, dcur, last
        kind = b["kind"]
        if kind == "draws" and b["batch"].ext is not None:
            # ksg_schedule_batch_draws is a plain entry point: on a context with extensions its
            # pods carry all-zero extension records, for the restatement and the model alike
            b["batch"] = PodBatch(b["batch"].pods, b["batch"].ids, None)
        sub = b["batch"]
        if kind == "seed":
            want, st = orc.batch(sub, rng_state)
            if engine is not None:
                got, sg = engine.batch(sub, rng_state)
                if not np.array_equal(got, want):
                    i = int(np.flatnonzero(got != want)[0])
                    fail(f"placement of pod {i}: {int(got[i])}, oracle {int(want[i])}")
                if sg != st:
                    fail(f"rng state {sg:#x}, oracle {st:#x}")
            b["rng_before"], rng_state = rng_state, st
        else:
            want, used = orc_draws_batch(sub, draws[dcur:])
            if engine is not None:
                got, ug = engine.batch_draws(sub, draws[dcur:])
                if not np.array_equal(got, want):
                    i = int(np.flatnonzero(got != want)[0])
                    fail(f"placement of pod {i}: {int(got[i])}, oracle {int(want[i])}")
                if ug != used:
                    fail(f"draws used {ug}, oracle {used}")
            b["d0"], dcur = dcur, dcur + used
        if engine is not None:
            cov["windows"] += engine.last_batch_stats()["windows"]
        b["out"] = np.asarray(want).copy()
        for i in np.flatnonzero(b["out"] >= 0):
            model.add(pod_rec(sub, int(i), int(b["out"][i]), R))
        cov["batch_pods"] += len(sub)
        cov["batch_placed"] += int((b["out"] >= 0).sum())
        last = b

    def note_removal(before, after, rec):
        if rec.host < N and any((int(after["keymap"][k, rec.host >> 6]) >> (rec.host & 63)) & 1 for k in rec.keys):
            cov["shared_left"] += 1  # another holder keeps the key's bit
        if np.any(before["svc_peer"] != after["svc_peer"]):
            moved = (before["svc_peer"] != after["svc_peer"]) & (after["svc_peer"] != -1)
            cov["peer_moved"] += int(moved.any())
        if np.any(after["svc_max"] < before["svc_max"]):
            cov["max_lowered"] += 1

    def pick_removal(how):
        live = model.live
        order = list(range(S))
        if how == "peer":
            for s in order:
                mem = [p for p in live if s in p.svcs]
                if len(mem) >= 2 and (mem[0].host if mem[0].host < N else -2) != (mem[1].host if mem[1].host < N else -2):
                    return mem[0]
        if how == "max":
            best = None
            for s in order:
                c = model.host_counts(s)
                if not c:
                    continue
                m = max(c.values())
                holders = [h for h, v in c.items() if v == m]
                if len(holders) == 1 and m >= 2:
                    cand = (holders[0] >= N, m, s, holders[0])  # prefer a maximum held by an off-list host
                    if best is None or cand > best:
                        best = cand
            if best is not None:
                _, _, s, h = best
                return [p for p in live if p.host == h and s in p.svcs][-1]
        if how == "shared":
            seen: dict = {}
            for p in live:
                if p.host < N:
                    for k in set(p.keys):
                        if (k, p.host) in seen:
                            return p
                        seen[(k, p.host)] = p
        assert live, "nothing to remove"
        return live[len(live) // 2]

    for idx, op in enumerate(seq.ops):
        where[0], where[1] = idx, op
        kind = op[0]
        if kind == "add":
            _, i, host = op
            both(lambda s: s.add_pod(host, pool, i))
            model.add(pod_rec(pool, i, host, R))
        elif kind == "remove":
            before = model.arrays()
            rec = pick_removal(op[1])
            both(lambda s: s.remove_pod(rec.uid))
            model.remove(rec.uid)
            note_removal(before, model.arrays(), rec)
        elif kind == "batch":
            do_batch({"batch": _slice(pool, op[1], op[2]), "kind": op[3]})
        elif kind == "unwind":
            out, sub = last["out"], last["batch"]
            placed = np.flatnonzero(out >= 0)
            assert len(placed) >= 3, "the batch placed too few pods to unwind"
            if op[1] == "first":
                k = int(placed[0])
            elif op[1] == "last":
                k = int(placed[-1])
            else:  # a placed pod in the middle with pods that found no node after it
                k = int(placed[len(placed) // 2])
                cov["nofit_after_mid"] += int((out[k + 1:] < 0).any())
            undo = [int(i) for i in placed if i >= k]
            kept_w = int((out[: k + 1] >= 0).sum())
            back = len(undo) - 1
            for i in reversed(undo):
                orc.remove_pod(int(sub.pods[i]["uid"]))
                model.remove(int(sub.pods[i]["uid"]))
            cov["max_undone"] = max(cov["max_undone"], len(undo))
            if last["kind"] == "seed":
                st_w = (rng_state - back * GAMMA) & _M64
                if engine is not None:
                    kept, st = engine.batch_unwind(sub, out, k, rng_state=rng_state)
                    if (kept, st) != (kept_w, st_w):
                        fail(f"unwind kept {kept} state {st:#x}, want {kept_w} {st_w:#x}")
                rng_state = st_w
            else:
                if engine is not None:
                    kept, _ = engine.batch_unwind(sub, out, k)
                    if kept != kept_w:
                        fail(f"unwind kept {kept}, want {kept_w}")
                dcur = last["d0"] + kept_w
            last = dict(last, k=k)
        elif kind == "rebatch":
            k, sub = last["k"], last["batch"]
            if k + 1 < len(sub):
                do_batch({"batch": _slice(sub, k + 1, len(sub)), "kind": last["kind"]})
        elif kind in ("begin_commit", "begin_abandon"):
            i = op[1]
            want = begin(orc, pool, i)
            if engine is not None:
                got = begin(engine, pool, i)
                if got != want:
                    fail(f"begin (rc, max, ties) {got}, oracle {want}")
            if kind == "begin_commit" and want[0] == abi.KSG_OK:
                r = int(draws[dcur])
                dcur += 1
                nw_ = orc.commit(r % want[2])
                if engine is not None:
                    ng = engine.commit(r % want[2])
                    if ng != nw_:
                        fail(f"commit node {ng}, oracle {nw_}")
                model.add(pod_rec(pool, i, nw_, R))
        elif kind == "query":
            if engine is not None:
                q = _slice(pool, POOL - 8, POOL)
                if op[1] == "explain":
                    engine.explain(q)
                elif op[1] == "prioritize":
                    engine.prioritize(q, top=4)
                elif op[1] == "headroom":
                    engine.headroom(q, 8)
                else:
                    uids = [int(last["batch"].pods[i]["uid"]) for i in np.flatnonzero(last["out"] >= 0)
                            if model.has(int(last["batch"].pods[i]["uid"]))]
                    engine.explain_without(q, uids, [min(j, len(uids)) for j in range(len(q))])
        elif kind == "fail":
            if engine is not None:
                try:
                    if op[1] == "batch_live_uid":
                        b = _slice(pool, POOL - RESERVED - 8, POOL - RESERVED - 3)
                        b.pods[2]["uid"] = model.live[len(model.live) // 2].uid
                        engine.batch(b, 99)
                    elif op[1] == "unwind_k_ge_n":
                        engine.batch_unwind(last["batch"], last["out"], len(last["batch"]))
                    elif op[1] == "unwind_nofit":
                        engine.batch_unwind(last["batch"], last["out"], int(np.flatnonzero(last["out"] < 0)[0]))
                    else:
                        engine.remove_pod(0xDEAD0000)
                except Exception as e:  # KsgError / ctypes: the call is refused
                    if isinstance(e, _Fail):
                        raise
                else:
                    fail("the call succeeded; it must fail and change nothing")
            if op[1] == "remove_unknown":
                try:
                    orc.remove_pod(0xDEAD0000)
                except KeyError:
                    pass
                else:
                    fail("oracle removed an unknown uid")
        elif kind == "set_cluster":
            seq.load(orc, False)
            if engine is not None:
                seq.load(engine, False)
            model = model_cls(N, S, MAX_KEYS, R)
            last = None
        elif kind == "remove_all":
            order = list(model.live)
            perm = np.random.default_rng(len(order)).permutation(len(order))
            for j, pi in enumerate(perm):
                rec = order[int(pi)]
                both(lambda s: s.remove_pod(rec.uid))
                model.remove(rec.uid)
                if j % 8 == 0:
                    audit()
        else:
            raise ValueError(op)
        st = audit()
        if kind == "set_cluster" or kind == "remove_all":
            if any(st[f].any() for f in FIELDS if f != "svc_peer") or (st["svc_peer"] != -1).any():
                fail("the model is not empty")
    orc.close()
    seq.coverage = cov
    return cov
