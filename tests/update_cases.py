"""Cases for ksg_update_cluster (a new node list under the same pods): helpers without a GPU.

A case is a chain of node lists over one universe of nodes and one shared Interner, a pool of
pending pods from tests.families ("namespaces": two namespaces, five services each), and a set of
pods placed by hand so that the case provably contains what it is there for (`facts`).
Everything is keyed by host NAME: a pod's host id under a node list, the renaming between two
lists (`maps`) and the expected state (`model`) all come from names, independently of the
library and of ClusterView.host_map. tests/test_update_inputs.py asserts the facts on the CPU;
tests/test_gpu_update.py runs the cases against the device.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass

import numpy as np

from kubernetes_amd import abi, ingest, workload
from kubernetes_amd.api import Quantity
from kubernetes_amd.engine import ClusterArrays, PodBatch
from tests import families
from tests.ext_cases import ExtCase
from tests.state_model import StateModel, pod_rec

POOL = 320          # pending pods per case
POOL_UID = 5000
HAND_UID = 100
FILL = 100          # pods of the batch before the update; pod FILL goes through begin / commit
AFTER = 100         # pods of the batch after it; pod FILL + 1 + AFTER through begin / commit
MAX_KEYS = 256
SEED = 5

CASES = ("shift_front", "drop_last", "shrink", "grow", "churn", "permute", "empty_out_in")
GHOST = "ghost-host-a"   # a host outside every node list

# what each case is there for (asserted by tests/test_update_inputs.py on the models)
EXPECT = {
    "shift_front": {"bit_moves_word", "new_empty_node", "second_holder", "outside_stays"},
    "drop_last": {"last_word_leaves", "leaver_max_alone", "leaver_peer", "second_holder", "outside_stays"},
    "shrink": {"bit_moves_word", "last_word_single", "leaver_max_alone", "leaver_peer", "second_holder", "negative",
               "outside_stays"},
    "grow": {"bit_moves_word", "new_empty_node", "second_holder", "outside_stays"},
    "churn": {"bit_moves_word", "leaver_max_alone", "leaver_peer", "joined_outside", "second_holder", "negative",
              "new_empty_node", "changed_capacity", "changed_label", "outside_stays"},
    "permute": {"bit_moves_word", "second_holder", "negative", "outside_stays"},
    "empty_out_in": {"leaver_max_alone", "leaver_peer", "second_holder", "outside_stays"},
}


@dataclass
class Live:
    """A live pod: the model's record (host filled in per node list), the host's name, and where
    its ABI record is (batch kind "hand" or "pool", index)."""
    rec: object
    host: str
    kind: str
    idx: int


def _policy(policy):
    if policy == "default":
        return workload.config_default()
    if policy == "config4":
        return workload.config4()
    if policy == "affinity":  # the family's own: ServiceAffinity{region} + LeastRequested + spreading
        return families.build("namespaces", 4, 4, SEED).config
    raise ValueError(policy)


class UpdateCase:
    def __init__(self, name: str, policy: str = "default", ext: bool = False, max_domains=None,
                 join_negative: bool = False):
        """join_negative (churn): the only pod with a negative request sits on an outside host that
        joins the list, beside a larger positive one, so no node total is ever negative."""
        self.name, self.policy, self.join_negative = name, policy, join_negative
        nu = 720 if name == "churn" else 130
        w = families.build("namespaces", nu, POOL, SEED)
        U = w.nodes
        self.services = w.services
        self.config = _policy(policy)
        self.config.max_conflict_keys = MAX_KEYS
        if max_domains is not None:
            self.config.max_domains = max_domains
        self.it = ingest.Interner()
        for k in self.config.label_keys():
            self.it.key_id(k)
        self.aff = self.config.affinity_labels()
        self.api_pods = list(w.pods)[:POOL]
        self.outside_join = []   # names of outside hosts that join the list at step 1
        self.perm = None
        self.changed_cap, self.changed_label = [], []
        lists = self._node_lists(name, U)
        self.views = [ingest.ClusterView(l, self.services, self.it) for l in lists]
        self.arrays = [v.arrays for v in self.views]
        self.names = [list(v.names) for v in self.views]
        if name == "permute":  # the same nodes, reordered by the caller's arrays (no view sorts like this)
            a0 = self.arrays[0]
            n = len(a0.nodes)
            self.perm = np.asarray([(i * 37 + 11) % n for i in range(n)])  # new rank i holds old rank perm[i]
            names = [a0.names[j] for j in self.perm]
            self.arrays.append(ClusterArrays(nodes=a0.nodes[self.perm].copy(), node_pairs=a0.node_pairs,
                                             pair_keys=a0.pair_keys, n_services=a0.n_services, names=names))
            self.names.append(names)
            self.views.append(self.views[0])
        self.ranks = [{nm: i for i, nm in enumerate(ns)} for ns in self.names]
        self.cfg = self.config.compile(self.it.key_id)
        uids = list(range(POOL_UID, POOL_UID + POOL))
        self.pool = [ingest.ingest_pods(v, self.api_pods, uids=uids, aff_labels=self.aff) for v in self.views]
        # ---- extensions: taints and extended resources by node of the universe ----
        self.ext = None
        self.n_scalar = 0
        if ext:
            shim = type("Shim", (), {})()
            shim.cfg, shim.view, shim.batch = self.cfg, self.views[0], self.pool[0]
            self.ext = ExtCase(nn=nu, npods=POOL, seed=SEED, case=shim)
            _, self._taints, self._scalar, tols, scal = workload.extension_data(nu, POOL, SEED)
            self._uidx = {n.metadata.name: i for i, n in enumerate(U)}
            self.n_scalar = int(self.ext.kcfg.n_scalar)
            for s in range(len(self.pool)):
                rec, ids = self.ext.inter.pod_records(self.pool[s].ids, tols, scal)
                self.pool[s] = PodBatch(self.pool[s].pods, ids, rec)
        self._hand()

    # ---- the node lists ---------------------------------------------------------------------
    def _node_lists(self, name, U):
        if name == "shift_front":
            return [U[1:66], U[0:66]]
        if name == "drop_last":
            return [U[0:65], U[0:64]]
        if name == "shrink":
            return [U[0:130], U[0:130:2]]
        if name == "grow":
            return [U[0:130:2], U[0:130]]
        if name == "permute":
            return [U[0:130]]
        if name == "empty_out_in":
            return [U[0:65], [], U[0:65]]
        if name == "churn":  # and its inverse as a third list
            old = U[0:700]
            leave = {7 + 35 * i for i in range(20)}
            new = [n for i, n in enumerate(old) if i not in leave]
            for j, i in enumerate(range(3, 700, 35)):  # 20 capacities, 20 labels on survivors
                n = copy.deepcopy(old[i])
                n.spec.capacity["cpu"] = Quantity.from_milli(6000 + 500 * (j % 5))
                new[new.index(old[i])] = n
                self.changed_cap.append(n.metadata.name)
            for j, i in enumerate(range(5, 700, 35)):
                n = copy.deepcopy(old[i])
                n.metadata.labels["zone"] = f"z{(int(n.metadata.labels['zone'][1:]) + 1) % 8}"
                n.metadata.labels["fresh"] = f"f{j % 2}"
                new[new.index(old[i])] = n
                self.changed_label.append(n.metadata.name)
            new += U[700:720]
            self.outside_join = [n.metadata.name for n in U[700:705]]
            return [old, new, old]
        raise ValueError(name)

    @property
    def steps(self):
        return len(self.arrays) - 1

    def n_nodes(self, step):
        return len(self.names[step])

    def host_id(self, step, host: str) -> int:
        """The host's id under list `step`, from its name (outside hosts: N + the interner's number)."""
        r = self.ranks[step].get(host)
        if r is not None:
            return r
        e = self.it.ext_hosts
        if host not in e:
            e[host] = len(e)
        return len(self.names[step]) + e[host]

    def maps(self, step):
        """(old_to_new, outside pairs) of the update from list `step` to `step + 1`, by names."""
        o2n = [self.host_id(step + 1, nm) for nm in self.names[step]]
        out = [(self.host_id(step, nm), self.host_id(step + 1, nm)) for nm in list(self.it.ext_hosts)
               if nm not in self.ranks[step]]
        return np.asarray(o2n, np.uint32), out

    def node_ext(self, step):
        """set_node_ext's arrays for list `step` (None without extensions)."""
        if self.ext is None:
            return None
        ix = [self._uidx[nm] for nm in self.names[step]]
        sc = {k: [v[i] for i in ix] for k, v in self._scalar.items()}
        return self.ext.inter.node_arrays([self._taints[i] for i in ix], sc)

    # ---- the pods placed by hand ------------------------------------------------------------
    def _hand(self):
        old, new = self.ranks[0], self.ranks[1]
        surv = [nm for nm in self.names[0] if nm in new]
        leav = [nm for nm in self.names[0] if nm not in new]
        plain = [nm for nm in surv if nm not in self.changed_cap and nm not in self.changed_label]
        mover = next((nm for nm in surv if old[nm] >> 6 != new[nm] >> 6), None)
        n1 = len(self.names[1])
        last = self.names[1][-1] if n1 % 64 == 1 and self.names[1][-1] in old else None
        self.roles = {"mover": mover, "last": last, "L0": leav[0] if leav else None,
                      "L1": leav[-1] if leav else None, "J0": self.outside_join[0] if self.outside_join else None,
                      "S0": plain[0] if plain else None, "S1": plain[len(plain) // 2] if plain else None}
        key = [self.it.conflict_id("port", 30000 + j) for j in range(4)]
        negative = "negative" in EXPECT[self.name] and not self.join_negative
        spec = []  # (host name, cpu, mem, keys, svcs, scalar0)
        r = self.roles
        if r["mover"]:
            spec.append((r["mover"], 300, 1 << 20, [key[0]], [0], 1))
        if r["last"]:
            spec.append((r["last"], 200, 2 << 20, [key[1]], [0], 0))
        if r["L0"]:
            spec += [(r["L0"], 100, 1 << 20, [], [1], 1)] * 16
        if r["S0"]:
            spec.append((r["S0"], 100, 1 << 20, [], [1], 0))
        if r["L1"]:
            spec.append((r["L1"], 150, 1 << 20, [], [2, 3], 0))
        if r["S1"]:
            spec.append((r["S1"], 150, 1 << 20, [], [2], 0))
        if r["J0"]:
            spec += [(r["J0"], 250, 3 << 20, [key[2]], [4], 1)] * 2 + [(r["J0"], 250, 3 << 20, [], [4], 0)] * 14
            spec += [(nm, 120, 1 << 20, [], [0], 0) for nm in self.outside_join[1:]]
            if self.join_negative:
                spec += [(self.outside_join[1], 1000, 8 << 20, [], [], 0), (self.outside_join[1], -300, -(1 << 20), [], [], 0)]
        anchor = r["S0"] or self.names[0][0]
        self.second_holder = len(spec)
        spec += [(anchor, 50, 1 << 20, [key[3]], [], 0)] * 2
        if negative:
            spec.append((r["S1"], -70000, -(50 << 30), [], [], 0))
        spec.append((GHOST, 100, 1 << 20, [key[0]], [0], 0))
        pods = np.zeros(len(spec), abi.POD_DTYPE)
        ids = []
        for i, (host, cpu, mem, keys, svcs, _) in enumerate(spec):
            p = pods[i]
            p["uid"], p["milli_cpu"], p["memory"], p["host"] = HAND_UID + i, cpu, mem, -1
            p["service"] = svcs[0] if svcs else -1
            p["ports_off"], p["n_ports"] = len(ids), len(keys)
            ids += keys
            p["pds_off"], p["sel_off"] = len(ids), len(ids)
            p["svcs_off"], p["n_svcs"] = len(ids), len(svcs)
            ids += svcs
            p["aff_pair"] = -1
        ext = None
        if self.ext is not None:
            ext = np.zeros(len(spec), abi.POD_EXT_DTYPE)
            for i, s in enumerate(spec):
                ext[i]["scalar"][0] = s[5]
        self.hand = PodBatch(pods, np.asarray(ids + [0], np.uint32), ext)
        self.hand_hosts = [s[0] for s in spec]

    # ---- live pods and the model ---------------------------------------------------------------
    def hand_live(self):
        return [Live(pod_rec(self.hand, i, 0, self.n_scalar), h, "hand", i) for i, h in enumerate(self.hand_hosts)]

    def pool_live(self, step, i, node):
        return Live(pod_rec(self.pool[step], i, 0, self.n_scalar), self.names[step][node], "pool", i)

    def batch_of(self, live: Live, step):
        return self.hand if live.kind == "hand" else self.pool[step]

    def model(self, live, step) -> StateModel:
        m = StateModel(self.n_nodes(step), len(self.services), MAX_KEYS, self.n_scalar)
        for l in live:
            rec = copy.copy(l.rec)
            rec.host = self.host_id(step, l.host)
            m.add(rec)
        return m

    def slice(self, step, lo, hi) -> PodBatch:
        b = self.pool[step]
        return PodBatch(b.pods[lo:hi].copy(), b.ids, None if b.ext is None else b.ext[lo:hi].copy())

    def load(self, sched, step=0, first=True):
        """set_cluster (+ the extensions) for list `step`."""
        if self.ext is not None:
            if first:
                sched.set_extensions(self.ext.kcfg)
            sched.set_cluster(self.arrays[step])
            sched.set_node_ext(*self.node_ext(step))
        else:
            sched.set_cluster(self.arrays[step])
        return sched

    def rebuild(self, sched, live, step):
        """The specification's fresh context: the new list, then every live pod in order."""
        self.load(sched, step)
        for l in live:
            sched.add_pod(self.host_id(step, l.host), self.batch_of(l, step), l.idx)
        return sched

    def fill(self, sched, live=None, step=0, with_begin=True):
        """The state before the update on `sched` (an engine or the oracle): the hand-placed pods,
        one batch of FILL pods, one begin / commit. -> (live list, generator state)."""
        live = [] if live is None else live
        for l in self.hand_live():
            sched.add_pod(self.host_id(step, l.host), self.hand, l.idx)
            live.append(l)
        out, rng = sched.batch(self.slice(step, 0, FILL), workload.TIEBREAK_SEED)
        for i, n in enumerate(out):
            if n >= 0:
                live.append(self.pool_live(step, i, int(n)))
        rc, ties = begin_rc(sched, self.pool[step], FILL) if with_begin else (None, 0)
        if rc == abi.KSG_OK:
            live.append(self.pool_live(step, FILL, sched.commit(ties // 2)))
        return live, rng


def begin_rc(sched, batch, i):
    """begin on an engine or the oracle -> (rc, tie count); a refused begin (KSG_ERR_NOPEER: the
    pod's ServiceAffinity peer is on a host outside the list) comes back as its code."""
    try:
        rc, _, ties, _ = sched.begin(batch, i)
        return rc, ties
    except RuntimeError as e:  # KsgError carries the code, the oracle's wrapper names it
        code = getattr(e, "code", None)
        if code is None and "rc=-5" in str(e):
            code = abi.KSG_ERR_NOPEER
        if code != abi.KSG_ERR_NOPEER:
            raise
        return code, 0


def facts(case: UpdateCase, live, step=0) -> set:
    """What the models before and after the update from `step` show, by the names of EXPECT."""
    a, b = case.model(live, step).arrays(), case.model(live, step + 1).arrays()
    r, old, new = case.roles, case.ranks[step], case.ranks[step + 1]
    nb = case.n_nodes(step + 1)
    key = [case.it.conflict_id("port", 30000 + j) for j in range(4)]
    f = set()
    bit = lambda st, k, n: bool((int(st["keymap"][k][n >> 6]) >> (n & 63)) & 1)
    if r["mover"] and bit(a, key[0], old[r["mover"]]) and bit(b, key[0], new[r["mover"]]) and \
            old[r["mover"]] >> 6 != new[r["mover"]] >> 6:
        f.add("bit_moves_word")
    if r["last"] and nb % 64 == 1 and new[r["last"]] == nb - 1 and bit(b, key[1], nb - 1):
        f.add("last_word_single")
    na = case.n_nodes(step)
    if na % 64 == 1 and case.names[step][-1] not in new and int(a["svc_cnt"][:, na - 1].sum()) > 0:
        f.add("last_word_leaves")
    if r["L0"] and r["L0"] not in new:
        cnt = a["svc_cnt"][1]
        if cnt[old[r["L0"]]] == a["svc_max"][1] and (cnt == cnt.max()).sum() == 1 and b["svc_max"][1] == a["svc_max"][1] \
                and (nb == 0 or b["svc_cnt"][1].max() < b["svc_max"][1]):
            f.add("leaver_max_alone")
    if r["L1"] and r["L1"] not in new and a["svc_peer"][2] == old[r["L1"]] and a["svc_peer"][3] == old[r["L1"]] and \
            b["svc_peer"][2] == -2 and b["svc_peer"][3] == -2:
        f.add("leaver_peer")
    if r["J0"] and r["J0"] in new and r["J0"] not in old:
        j = new[r["J0"]]
        two = [l for l in live if l.host == r["J0"] and key[2] in l.rec.keys]
        if len(two) == 2 and bit(b, key[2], j) and b["svc_cnt"][4][j] == 16 == b["svc_max"][4] and \
                a["svc_cnt"][4].max(initial=0) < 16 and a["svc_max"][4] == 16 and b["used_cpu"][j] == 16 * 250:
            f.add("joined_outside")
    anchor = r["S0"] or case.names[step][0]
    holders = [l for l in live if key[3] in l.rec.keys and l.host == anchor]
    if len(holders) == 2 and (anchor not in new or bit(b, key[3], new[anchor])):
        f.add("second_holder")
    if any(l.rec.cpu < 0 for l in live) and (a["used_cpu"] < 0).any() and (b["used_cpu"] < 0).any():
        f.add("negative")
    neg = [l for l in live if l.rec.cpu < 0 or l.rec.mem < 0]
    if neg and all(l.host in case.outside_join and l.host not in old and l.host in new for l in neg) and \
            not any((st[k] < 0).any() for st in (a, b) for k in ("used_cpu", "used_mem")):
        f.add("joined_negative")
    fresh = [nm for nm in case.names[step + 1] if nm not in old and nm not in case.outside_join]
    if fresh and all(b["used_cpu"][new[nm]] == 0 and b["svc_cnt"][:, new[nm]].sum() == 0 for nm in fresh):
        f.add("new_empty_node")
    if case.changed_cap and step == 0:
        v0, v1 = case.arrays[0].nodes, case.arrays[1].nodes
        if all(v0[old[nm]]["cap_milli_cpu"] != v1[new[nm]]["cap_milli_cpu"] for nm in case.changed_cap):
            f.add("changed_capacity")
    if case.changed_label and step == 0:
        lab = lambda arr, n: tuple(arr.node_pairs[int(arr.nodes[n]["label_off"]):
                                                  int(arr.nodes[n]["label_off"]) + int(arr.nodes[n]["n_labels"])])
        if all(lab(case.arrays[0], old[nm]) != lab(case.arrays[1], new[nm]) for nm in case.changed_label):
            f.add("changed_label")
    if any(l.host == GHOST for l in live) and a["svc_total"][0] > a["svc_cnt"][0].sum():
        f.add("outside_stays")
    return f
