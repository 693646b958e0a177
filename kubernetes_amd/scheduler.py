"""The drop-in `algorithm.Scheduler` backed by the HIP Filter/Score pass.

Reference interface (pkg/scheduler):
  type Scheduler interface { Schedule(api.Pod, MinionLister) (string, error) }   scheduler.go:25-27
  NewGenericScheduler(predicates, prioritizers, pods PodLister, random)           generic_scheduler.go:197-204
  FitError{Pod, FailedPredicates}                                                  generic_scheduler.go:30-44
  MinionLister / PodLister / ServiceLister and their fakes                         listers.go:27-93

`GPUScheduler.schedule(pod, minion_lister)` keeps the reference's contract:
  * no nodes -> NoMinionsError("no minions available to schedule pods");
  * nothing fits (or the priority list is empty) -> FitError with a
    FailedPredicateMap (one failing predicate name per node);
  * otherwise exactly one `random.int()` draw and the ix-th host, ix = r % ties,
    in (score desc, name desc) order.
The pods the scheduler sees are exactly what `pod_lister.list()` returns at each
call (as MapPodsToMachines re-lists them, predicates.go:354-375). With a plain
lister the device state is reconciled against it by namespace/name before each
pod; with SimpleModeler's lister (kubernetes_amd.modeler) it is kept equal to
the modeler's stores by their change events (PodMirror), so a Schedule call costs
O(events + assumed pods) on the host instead of O(all pods).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import abi
from .api import Node, Pod, Service
from .engine import DeviceScheduler, PodBatch
from .factory import SchedulerConfig
from .ingest import ClusterView, Interner, PodBatchBuilder
from .labels import everything, selector_from_set
from .modeler import ModelerPodLister, PodMirror


class FitError(Exception):
    """*FitError (generic_scheduler.go:30-44). `counts` (optional; no reference counterpart):
    predicate name -> number of nodes it failed on, as the batch path's report gives them."""

    def __init__(self, pod: Pod, failed_predicates: Dict[str, set], counts: Optional[Dict[str, int]] = None):
        self.pod = pod
        self.failed_predicates = failed_predicates
        self.counts = counts
        out = f"failed to find fit for pod: {pod.metadata.namespace}/{pod.metadata.name}"
        for node in sorted(failed_predicates):
            out += f"Node {node}: {','.join(sorted(failed_predicates[node]))}"
        super().__init__(out)


class NoMinionsError(Exception):
    def __init__(self):
        super().__init__("no minions available to schedule pods")


class SchedulingError(Exception):
    """Non-fit errors from a predicate (e.g. ServiceAffinity's peer lookup)."""


# ---- listers (listers.go:27-93) ----------------------------------------------
class FakeMinionLister:
    def __init__(self, nodes: Sequence[Node]):
        self.nodes = list(nodes)

    def list(self) -> List[Node]:
        return list(self.nodes)


class FakePodLister:
    def __init__(self, pods: Sequence[Pod]):
        self.pods = list(pods)

    def list(self, selector=None) -> List[Pod]:
        sel = selector or everything()
        return [p for p in self.pods if sel.matches(p.metadata.labels)]


class FakeServiceLister:
    def __init__(self, services: Sequence[Service]):
        self.services = list(services)

    def list(self) -> List[Service]:
        return list(self.services)

    def get_pod_services(self, pod: Pod) -> List[Service]:
        out = [s for s in self.services
               if s.metadata.namespace == pod.metadata.namespace
               and selector_from_set(s.spec.selector).matches(pod.metadata.labels)]
        if not out:
            raise LookupError(f"Could not find service for pod {pod.metadata.name} in namespace "
                              f"{pod.metadata.namespace} with labels: {pod.metadata.labels}")
        return out


class SplitMix64Rand:
    """Injected deterministic source: Int() = splitmix64 >> 1.
    Go's `*rand.Rand` stream cannot be reproduced without the Go stdlib; the
    caller's own source can be passed instead (anything with .int())."""

    MASK = (1 << 64) - 1

    def __init__(self, seed: int = 0):
        self.state = seed & self.MASK

    def next(self) -> int:
        self.state = (self.state + 0x9E3779B97F4A7C15) & self.MASK
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & self.MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & self.MASK
        return z ^ (z >> 31)

    def int(self) -> int:
        return self.next() >> 1


class GPUScheduler:
    """algorithm.Scheduler on the MI355X (NewGenericScheduler's drop-in)."""

    def __init__(self, config: SchedulerConfig, pod_lister, service_lister=None, random=None,
                 device: int = 0, incremental_nodes: bool = False):
        self.config = config
        # a changed node list under an unchanged service list keeps the device's pods
        # (DeviceScheduler.update_cluster) instead of resetting and re-adding every one
        self.incremental_nodes = incremental_nodes
        self.pod_lister = pod_lister
        self.service_lister = service_lister or FakeServiceLister([])
        self.random = random if random is not None else SplitMix64Rand(0)
        self.interner = Interner()
        for k in config.label_keys():
            self.interner.key_id(k)
        self.aff_labels = config.affinity_labels()
        self.engine = DeviceScheduler(config.compile(self.interner.key_id), device=device)
        self.fail_names = config.fail_code_names()
        self.view: Optional[ClusterView] = None
        self._node_sig = None
        self._svc_sig = None
        self._mirror: Dict[str, tuple] = {}  # listed pod's distinct key -> (uid, host_id, id(pod))
        self._assumed: List[tuple] = []  # (pod key, uid, host_id) committed since the last re-list
        self._next_uid = 1
        # the modeler's PodLister (factory.go: f.PodLister = modeler.PodLister()):
        # mirror its stores by events instead of re-listing every pod per Schedule
        self._events: Optional[PodMirror] = None
        if isinstance(pod_lister, ModelerPodLister):
            self._events = PodMirror(pod_lister.modeler, self.engine, self._ingest_one, self._uid,
                                     host_of=lambda p: self.view.host_id(p.status.host))

    def close(self):
        self.engine.close()

    # ---- state reconciliation ----------------------------------------------
    def _uid(self) -> int:
        u = self._next_uid
        self._next_uid += 1
        return u

    def _ingest_one(self, pod: Pod, uid: int):
        b = PodBatchBuilder(self.view, self.aff_labels)
        b.add(pod, uid)
        return self.view.host_id(pod.status.host), b.build()

    def _sync(self, nodes: Sequence[Node]):
        services = self.service_lister.list()
        # list equality: identity first per element, so an unchanged list is ~10 us at
        # 5k nodes (an equal-valued replacement object counts as unchanged)
        nsig = list(nodes)
        ssig = list(services)
        if self.incremental_nodes and self.view is not None and ssig == self._svc_sig and nsig != self._node_sig:
            old = self.view
            view = ClusterView(nodes, services, self.interner)
            old_to_new, outside = view.host_map(old)
            self.engine.update_cluster(view.arrays, old_to_new, outside)
            self.view = view
            for extra in self.config.static_passes(self.interner.key_id):
                self.engine.add_static_config(extra)
            self._node_sig = nsig
            ren = dict(outside)

            def fn(h, n_old=len(old.names)):
                return int(old_to_new[h]) if h < n_old else ren.get(h, h)

            self._mirror = {k: (uid, fn(h), pid) for k, (uid, h, pid) in self._mirror.items()}
            self._assumed = [(k, uid, fn(h)) for k, uid, h in self._assumed]
            if self._events is not None:
                self._events.rehost(fn)
        if nsig != self._node_sig or ssig != self._svc_sig or self.view is None:
            self.view = ClusterView(nodes, services, self.interner)
            self.engine.set_cluster(self.view.arrays)
            # LabelsPresence / LabelPreference past the config's slots: slot passes on the device
            for extra in self.config.static_passes(self.interner.key_id):
                self.engine.add_static_config(extra)
            self._node_sig, self._svc_sig = nsig, ssig
            self._mirror = {}
            self._assumed = []
            if self._events is not None:
                self._events.reload()
                return
        if self._events is not None:
            self._events.sync()
            return
        pods = self.pod_lister.list(everything())
        want = {}
        for p in pods:  # unnamed / duplicate keys (fake listers) stay distinct pods
            k = p.key()
            if k in want:
                j = 1
                while f"{k}#{j}" in want:
                    j += 1
                k = f"{k}#{j}"
            want[k] = p
        # pods this scheduler committed since the last call: kept iff the lister now
        # reports them (under their key, or a #j variant of it) on the same host
        assumed, self._assumed = self._assumed, []
        for akey, uid, host in assumed:
            k, j, match = akey, 0, None
            while k in want:
                if k not in self._mirror and self.view.host_id(want[k].status.host) == host:
                    match = k
                    break
                j += 1
                k = f"{akey}#{j}"
            if match is None:
                self.engine.remove_pod(uid)
            else:
                self._mirror[match] = (uid, host, id(want[match]))
        for key in [k for k, (uid, host, pid) in self._mirror.items()
                    if k not in want or id(want[k]) != pid or self.view.host_id(want[k].status.host) != host]:
            self.engine.remove_pod(self._mirror.pop(key)[0])
        add = [(k, p) for k, p in want.items() if k not in self._mirror]
        if add:
            b = PodBatchBuilder(self.view, self.aff_labels)
            uids = []
            for _, p in add:
                uid = self._uid()
                uids.append(uid)
                b.add(p, uid)
            batch = b.build()
            for i, (k, p) in enumerate(add):
                h = self.view.host_id(p.status.host)
                self.engine.add_pod(h, batch, i)
                self._mirror[k] = (uids[i], h, id(p))

    # ---- Schedule -------------------------------------------------------------
    def schedule(self, pod: Pod, minion_lister) -> str:
        nodes = minion_lister.list()
        if len(nodes) == 0:
            raise NoMinionsError()
        self._sync(nodes)
        uid = self._uid()
        b = PodBatchBuilder(self.view, self.aff_labels)
        b.add(pod, uid)
        batch = b.build()
        try:
            rc, _, k, fails = self.engine.begin(batch, 0, want_fail=True)
        except Exception as e:  # ServiceAffinity peer on an unknown node, etc.
            if getattr(e, "code", None) == abi.KSG_ERR_NOPEER:
                raise SchedulingError(str(e)) from e
            raise
        if rc == abi.KSG_NONODES:
            raise NoMinionsError()
        if rc == abi.KSG_NOFIT:
            failed = {}
            for n, code in enumerate(fails):
                if code:
                    failed[self.view.names[n]] = {self.fail_names[int(code)]}
            raise FitError(pod, failed)
        r = self.random.int()
        node = self.engine.commit(r % k)
        # the device now assumes the pod on `node` (AssumePod); the next _sync keeps it
        # iff the pod lister reports it there too.
        host = self.view.names[node]
        if self._events is not None:  # adopted when AssumePod reports it, else dropped
            self._events.committed(pod, uid, node)
        else:
            self._assumed.append((pod.key(), uid, node))
        return host

    # ---- batch path (persistent kernel) -------------------------------------
    def schedule_batch(self, pods: Sequence[Pod], minion_lister, rng_state: int, explain=False):
        """Schedule pods in order without host round-trips; each success is assumed
        (committed) before the next pod. -> (hosts or None per pod, rng_state).
        explain=True: -> (hosts, rng_state, errors), errors[i] None for a placed pod, else the
        error Schedule would return for it: a FitError (with `counts`) built from one
        ksg_explain_batch over the batch's unschedulable pods, or a SchedulingError for a
        ServiceAffinity peer on an unknown host (NoMinionsError without nodes). The report is
        against the state after the whole batch: the state a retry of the pod would meet.
        explain="as_of": the same triple, each error against the state as of its pod, with the
        batch's later placements taken away again: the FitError pod-by-pod schedule() calls
        would have raised, from one ksg_explain_without over the batch's unschedulable pods."""
        if explain not in (False, True, "as_of"):
            raise ValueError(f"explain={explain!r}: False, True or 'as_of'")
        nodes = minion_lister.list()
        if len(nodes) == 0:
            if explain:
                return [None] * len(pods), rng_state, [NoMinionsError() for _ in pods]
            return [None] * len(pods), rng_state
        self._sync(nodes)
        b = PodBatchBuilder(self.view, self.aff_labels)
        uids = []
        for p in pods:
            uids.append(self._uid())
            b.add(p, uids[-1])
        batch = b.build()
        out, rng_state = self.engine.batch(batch, rng_state)
        hosts = []
        for i, p in enumerate(pods):
            if out[i] >= 0:
                hosts.append(self.view.names[out[i]])
                if self._events is not None:
                    self._events.committed(p, uids[i], int(out[i]))
                else:
                    self._assumed.append((p.key(), uids[i], int(out[i])))
            else:
                hosts.append(None)
        if explain:
            placed = None
            if explain == "as_of":  # the placed uids in order; a pod's position: the number placed before it
                placed = [uids[i] for i in range(len(pods)) if out[i] >= 0]
            return hosts, rng_state, self._explain(pods, batch, [i for i, h in enumerate(hosts) if h is None], out, placed)
        return hosts, rng_state

    def _explain(self, pods: Sequence[Pod], batch: PodBatch, idx: List[int], out=None, placed=None) -> list:
        """errors[i] for the pods `idx` of a batch that found no node: one device pass
        (`placed`: against the state as of each pod, the later of these uids taken away)."""
        errors: list = [None] * len(pods)
        if not idx:
            return errors
        sub = PodBatch(batch.pods[idx], batch.ids, None if batch.ext is None else batch.ext[idx])
        if placed is None:
            codes, hist, err = self.engine.explain(sub)
        else:
            before, k = [], 0  # placed before pod i
            for o in out:
                before.append(k)
                k += o >= 0
            codes, hist, err = self.engine.explain_without(sub, placed, [before[i] for i in idx])
        names = self.view.names
        for j, i in enumerate(idx):
            if err[j]:
                errors[i] = SchedulingError("service affinity peer is not on a known node")
                continue
            row = codes[j]
            failed = {names[n]: {self.fail_names[int(row[n])]} for n in row.nonzero()[0]}
            counts = {self.fail_names[c]: int(hist[j, c]) for c in range(1, hist.shape[1]) if hist[j, c]}
            errors[i] = FitError(pods[i], failed, counts)
        return errors

    # ---- dry run: the sorted HostPriorityList's head ---------------------------------
    def prioritize(self, pods: Sequence[Pod], minion_lister, top: int = 3) -> list:
        """Where would each pod go now, and how close is the runner-up: per pod the first `top`
        entries (host name, score) of the HostPriorityList selectHost would read, in its order
        (score descending, then host descending; generic_scheduler.go:84-96, types.go:42-47),
        from one ksg_prioritize_batch. Nothing is committed or drawn, and no pod is assumed. An
        empty list: nothing fits, or the priority list is empty (Schedule's FitError). A
        SchedulingError instead of a list: the pod's ServiceAffinity peer is on an unknown host;
        NoMinionsError entries without nodes."""
        nodes = minion_lister.list()
        if len(nodes) == 0:
            return [NoMinionsError() for _ in pods]
        self._sync(nodes)
        if not pods:
            return []
        b = PodBatchBuilder(self.view, self.aff_labels)
        for p in pods:
            b.add(p, 0)  # (the call ignores uids)
        _, _, _, tn, ts, _, err = self.engine.prioritize(b.build(), top=top)
        names = self.view.names
        out: list = []
        for i in range(len(pods)):
            if err[i]:
                out.append(SchedulingError("service affinity peer is not on a known node"))
            else:
                out.append([(names[int(n)], int(s)) for n, s in zip(tn[i], ts[i]) if n >= 0])
        return out

    # ---- dry run: how many copies of a pod fit ----------------------------------------
    ROOM_NAMES = {abi.ROOM_LIMIT: "limit", abi.ROOM_DISK: "disk", abi.ROOM_PORTS: "ports", abi.ROOM_CPU: "cpu",
                  abi.ROOM_MEMORY: "memory", **{abi.ROOM_SCALAR0 + r: f"scalar{r}" for r in range(abi.MAX_SCALAR)}}

    def headroom(self, pods: Sequence[Pod], minion_lister, limit: int = 1 << 16, per_node: bool = False) -> list:
        """How many copies of each pod (a template) fit now: per pod a record from one
        ksg_headroom_batch, {"total": the copies the nodes take together (each node filled on its
        own, at most `limit` per node), "nodes": the nodes that take at least one, "largest": the
        most one node takes, "binding": {constraint name: nodes it stops}, names "limit", "disk",
        "ports", "cpu", "memory", "scalar<r>"}, and with per_node=True "per_node": {host name:
        count} for the nodes that take at least one. total >= r says a gang of r fits, except
        under a ServiceAffinity predicate while the pod's service has no peer, where it is an
        upper bound. Nothing is committed or drawn, and no pod is assumed. A SchedulingError
        instead of a record: the pod's ServiceAffinity peer is on an unknown host; a ValueError:
        the pod has a negative request; NoMinionsError entries without nodes."""
        nodes = minion_lister.list()
        if len(nodes) == 0:
            return [NoMinionsError() for _ in pods]
        self._sync(nodes)
        if not pods:
            return []
        b = PodBatchBuilder(self.view, self.aff_labels)
        for p in pods:
            b.add(p, 0)  # (the call ignores uids)
        total, fit, mx, hist, counts, err = self.engine.headroom(b.build(), limit, want_counts=per_node)
        names = self.view.names
        out: list = []
        for i in range(len(pods)):
            if err[i] == abi.HEADROOM_ERR_PEER:
                out.append(SchedulingError("service affinity peer is not on a known node"))
                continue
            if err[i]:
                out.append(ValueError("negative resource request"))
                continue
            rec = {"total": int(total[i]), "nodes": int(fit[i]), "largest": int(mx[i]),
                   "binding": {self.ROOM_NAMES[s]: int(hist[i, s]) for s in range(1, hist.shape[1]) if hist[i, s]}}
            if per_node:
                rec["per_node"] = {names[int(n)]: int(counts[i, n]) for n in counts[i].nonzero()[0]}
            out.append(rec)
        return out

    # ---- dry run: preemption ------------------------------------------------------------
    def _committed(self) -> list:
        """(pod, uid) of every listed pod the device holds (after a _sync), in uid order."""
        out = []
        if self._events is not None:
            m = self._events.modeler
            stores = {PodMirror.SCHED: m.scheduled_pods.store, PodMirror.ASSUMED: m.assumed_pods.store}
            for (src, key), uid in self._events.on_device.items():
                p, ok = stores[src].get_by_key(key)
                if ok:
                    out.append((p, uid))
        else:
            by_id = {id(p): p for p in self.pod_lister.list(everything())}
            out = [(by_id[pid], uid) for uid, _, pid in self._mirror.values() if pid in by_id]
        out.sort(key=lambda t: t[1])
        return out

    def preempt(self, pods: Sequence[Pod], minion_lister, priority_of, max_victims: int = 16) -> list:
        """Which pods would have to leave for each pending pod, from one ksg_preempt_batch:
        the committed pods are sorted by priority_of(pod) descending (stable), and a pending pod
        may evict those strictly below its own priority. Per pending pod: None when a node takes
        it as things stand (schedule it, evict nothing); {"host": name, "victims": [namespace/name,
        ...] (most important first, at most max_victims), "n_victims": their true number} for the
        node where the eviction hurts least (the least important most-important victim, then the
        fewest victims, then the highest host); a FitError against the state with every pod it
        may evict taken away when even that leaves no node. Nothing is committed or removed.
        NoMinionsError entries without nodes. Not available under a ServiceAffinity predicate
        (KsgError)."""
        nodes = minion_lister.list()
        if len(nodes) == 0:
            return [NoMinionsError() for _ in pods]
        self._sync(nodes)
        if not pods:
            return []
        listed = sorted(self._committed(), key=lambda t: -priority_of(t[0]))  # (stable)
        prios = [priority_of(p) for p, _ in listed]
        uids = [u for _, u in listed]
        b = PodBatchBuilder(self.view, self.aff_labels)
        for p in pods:
            b.add(p, 0)  # (the call ignores uids)
        batch = b.build()
        pos = []
        for p in pods:  # the first entry below the pod's own priority
            mine = priority_of(p)
            pos.append(sum(1 for q in prios if q >= mine))
        best, nv, victims, cand, free, _ = self.engine.preempt(batch, uids, pos, max_victims=max_victims)
        names = self.view.names
        out: list = [None] * len(pods)
        nofit = [i for i in range(len(pods)) if cand[i] == 0]
        for i in range(len(pods)):
            if free[i] > 0 or cand[i] == 0:
                continue
            out[i] = {"host": names[int(best[i])],
                      "victims": [listed[int(j)][0].key() for j in victims[i] if j != 0xFFFFFFFF],
                      "n_victims": int(nv[i])}
        if nofit:
            sub = PodBatch(batch.pods[nofit], batch.ids, None if batch.ext is None else batch.ext[nofit])
            codes, hist, _ = self.engine.explain_without(sub, uids, [pos[i] for i in nofit])
            for j, i in enumerate(nofit):
                row = codes[j]
                failed = {names[n]: {self.fail_names[int(row[n])]} for n in row.nonzero()[0]}
                counts = {self.fail_names[c]: int(hist[j, c]) for c in range(1, hist.shape[1]) if hist[j, c]}
                out[i] = FitError(pods[i], failed, counts)
        return out

    # ---- dry run: do pod sets fit together ------------------------------------------------
    def drainable(self, node_names: Sequence[str], minion_lister, movable=None) -> list:
        """If node x goes, do its pods all find room elsewhere: one answer per name of
        `node_names`, from one ksg_pack_batch. A node's set is the committed pods the device
        holds on it, in uid order, without those `movable(pod)` says stay (DaemonSet-like pods),
        as pending pods that are no longer pinned to a host. Each is placed first-fit on the
        highest host that takes it given the set's earlier pods; the node itself is excluded,
        and so is every other named node, so the answers for several nodes do not lean on each
        other's room. Per node {"fits": every pod found a host, "moves": {namespace/name: host
        name or None}}. First fit is a heuristic: fits=True proves that the node can be drained
        now, fits=False does not prove that it cannot. Nothing is committed, drawn or assumed.
        A KeyError for a name that is no node; NoMinionsError entries without nodes. Not
        available under a ServiceAffinity predicate (KsgError)."""
        nodes = minion_lister.list()
        if len(nodes) == 0:
            return [NoMinionsError() for _ in node_names]
        self._sync(nodes)
        if not node_names:
            return []
        names = self.view.names
        rank = {n: i for i, n in enumerate(names)}
        ranks = [rank[n] for n in node_names]
        on = {r: [] for r in ranks}
        for p, _ in self._committed():
            r = rank.get(p.status.host)
            if r in on and (movable is None or movable(p)):
                on[r].append(p)
        b = PodBatchBuilder(self.view, self.aff_labels)
        sets = [on[r] for r in ranks]
        for pods in sets:
            for p in pods:
                b.add(Pod(metadata=p.metadata, spec=dataclasses.replace(p.spec, host="")), 0)  # (uids are ignored)
        targets = np.full((len(names) + 63) // 64, ~np.uint64(0), np.uint64)
        for r in ranks:
            targets[r >> 6] &= ~(np.uint64(1) << np.uint64(r & 63))
        out, placed = self.engine.pack(b.build(), [len(s) for s in sets], exclude=ranks, targets=targets)
        res, at = [], 0
        for s, pods in enumerate(sets):
            moves = {p.key(): (names[int(out[at + j])] if out[at + j] >= 0 else None) for j, p in enumerate(pods)}
            res.append({"fits": int(placed[s]) == len(pods), "moves": moves})
            at += len(pods)
        return res

    def fits_together(self, gangs: Sequence[Sequence[Pod]], minion_lister) -> list:
        """Does each gang of pending pods (a driver and its workers, a pod group with a port or a
        PD per member) fit as a whole now: per gang {"fits": bool, "hosts": [host name or None per
        pod]}, from one ksg_pack_batch. The pods of a gang are placed in the given order, first
        fit on the highest host, each seeing the requests, host ports and GCE PDs of the gang's
        earlier pods; gangs do not see each other. First fit is a heuristic: fits=True proves that
        the gang fits, fits=False does not prove that it cannot (largest pods first helps).
        Nothing is committed, drawn or assumed. NoMinionsError entries without nodes. Not
        available under a ServiceAffinity predicate (KsgError)."""
        nodes = minion_lister.list()
        if len(nodes) == 0:
            return [NoMinionsError() for _ in gangs]
        self._sync(nodes)
        if not gangs:
            return []
        b = PodBatchBuilder(self.view, self.aff_labels)
        for g in gangs:
            for p in g:
                b.add(p, 0)  # (the call ignores uids)
        out, placed = self.engine.pack(b.build(), [len(g) for g in gangs])
        names = self.view.names
        res, at = [], 0
        for s, g in enumerate(gangs):
            hosts = [names[int(o)] if o >= 0 else None for o in out[at: at + len(g)]]
            res.append({"fits": int(placed[s]) == len(g), "hosts": hosts})
            at += len(g)
        return res


def new_gpu_scheduler(config: SchedulerConfig, pod_lister, service_lister=None, random=None,
                      device: int = 0) -> GPUScheduler:
    """Counterpart of NewGenericScheduler at factory.go:149."""
    return GPUScheduler(config, pod_lister, service_lister, random, device)
