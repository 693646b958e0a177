"""Inputs of the ksg_explain_batch tests (tests/test_explain_inputs.py on the CPU,
tests/test_gpu_explain.py on the device): small clusters tightened so that a fill batch
leaves resource, port and disk failures behind, one case per policy that has a fail code
of its own, and the probe pods that are then explained.

  config2            the default provider (HostName, MatchNodeSelector, NoDiskConflict,
                     PodFitsPorts, PodFitsResources)
  config4            + ServiceAffinity{region} and ServiceAntiAffinity{zone}
  invalid_selectors  tests/families.py: two ServiceAffinity predicates under SelectorFromSet's trap
  presence           + a LabelsPresence predicate over a label a third of the nodes lack
  hosts              config2's policy, probe pods pinned to a node rank / to a host that names no node

Every case is built once per (policy, node count) and shared by the tests (read-only)."""
from __future__ import annotations

import functools
import re
import os

import numpy as np

from kubernetes_amd import factory, ingest, workload
from kubernetes_amd.api import GCEPersistentDiskVolumeSource, Quantity, Volume
from kubernetes_amd.engine import PodBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICIES = ("config2", "config4", "invalid_selectors", "presence", "hosts")
N_FILL = 200


def kernel_tiling():
    """(nodes per workgroup, pods per workgroup) of ksg_explain_kernel, from ksg_internal.h."""
    src = open(os.path.join(ROOT, "kubernetes_amd", "csrc", "ksg_internal.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in ("KSG_EXPLAIN_TILE", "KSG_EXPLAIN_CHUNK"))


TILE, CHUNK = kernel_tiling()
# each side of a 64-node word and of the kernel's node tile, and a multi-tile count that is a multiple of neither
NODE_COUNTS = (63, 64, 65, TILE - 1, TILE, TILE + 1, 1000)
POD_COUNTS = (1, CHUNK - 1, CHUNK, CHUNK + 1)
N_PROBE = CHUNK + 1


def _presence_config():
    preds = [{"name": n} for n in ("PodFitsPorts", "PodFitsResources", "NoDiskConflict", "MatchNodeSelector", "HostName")]
    preds.append({"name": "explain-needs-ssd", "argument": {"labelsPresence": {"labels": ["ssd"], "presence": True}}})
    return factory.create_from_config({"predicates": preds,
                                       "priorities": [{"name": "LeastRequestedPriority", "weight": 1},
                                                      {"name": "ServiceSpreadingPriority", "weight": 1}]})


class XCase:
    """cfg, view, `fill` (committed first) and `probe` (explained) as PodBatches."""

    def __init__(self, policy: str, nn: int, n_fill: int = N_FILL, n_probe: int = N_PROBE):
        self.policy, self.nn = policy, nn
        rng = workload._SM(977 * nn + len(policy))
        npods = n_fill + n_probe
        if policy == "invalid_selectors":
            from tests.families import build

            w = build("invalid_selectors", nn, npods)
            nodes, pods, services, cfg = w.nodes, w.pods, w.services, w.config
        else:
            nodes = workload.make_nodes(nn, rng)
            pods = workload.make_pods(npods, rng, n_apps=8, port_frac=0.3, pd_frac=0.0, sel_frac=0.25)
            services = workload.make_services(8)
            cfg = {"config4": workload.config4, "presence": _presence_config}.get(policy, workload.config_default)()
            cfg.max_conflict_keys = 4096
            for i, p in enumerate(pods):  # GCE PDs from a small pool: the fill leaves conflicts behind
                if i % 4 == 0:
                    p.spec.volumes = [Volume(name="data", gce_persistent_disk=GCEPersistentDiskVolumeSource(
                        pd_name=f"pd-{rng.below(6)}"))]
        # tight capacities (tests/families.py::_tighten, tighter): most pods fill a node alone
        for n in nodes:
            n.spec.capacity["cpu"] = Quantity.from_milli(400 + 200 * rng.below(4))
        if policy == "presence":
            for i, n in enumerate(nodes):
                if i % 3:
                    n.metadata.labels["ssd"] = "true"
        if policy == "hosts":
            names = [n.metadata.name for n in nodes]
            for i, p in enumerate(pods[n_fill:]):
                if i % 3 == 0:
                    p.spec.host = names[(i * 37) % nn]
                elif i % 3 == 1:
                    p.spec.host = "no-such-node"
        it = ingest.Interner()
        for k in cfg.label_keys():
            it.key_id(k)
        self.view = ingest.ClusterView(nodes, services, it)
        self.cfg = cfg.compile(it.key_id)
        b = ingest.ingest_pods(self.view, pods, uids=list(range(1, npods + 1)), aff_labels=cfg.affinity_labels())
        self.fill = PodBatch(b.pods[:n_fill], b.ids)
        self.probe = PodBatch(b.pods[n_fill:], b.ids)

    def load(self, sched, seed: int = 1234):
        """set_cluster + the fill batch. -> (placements, rng state)"""
        sched.set_cluster(self.view.arrays)
        return sched.batch(self.fill, seed)


@functools.lru_cache(maxsize=None)
def xcase(policy: str, nn: int) -> XCase:
    return XCase(policy, nn)


class XExtCase:
    """tests/ext_cases.py's config2 cluster with taints and extended resources (codes 8, 9)."""

    def __init__(self, nn: int, n_fill: int = N_FILL, n_probe: int = N_PROBE):
        from tests.ext_cases import ExtCase

        self.c = ExtCase("config2", nn, n_fill + n_probe, w_taint=0, w_bal=0)
        b = self.c.batch
        self.cfg, self.nn = self.c.cfg, nn
        self.fill = PodBatch(b.pods[:n_fill], b.ids, b.ext[:n_fill])
        self.probe = PodBatch(b.pods[n_fill:], b.ids, b.ext[n_fill:])
        self.probe_plain = PodBatch(b.pods[n_fill:], b.ids, None)  # the ext == NULL form

    def load(self, sched, seed: int = 1234):
        self.c.load(sched)
        return sched.batch(self.fill, seed)


@functools.lru_cache(maxsize=None)
def xext(nn: int) -> XExtCase:
    return XExtCase(nn)


def oracle_codes(case, probe=None) -> np.ndarray:
    """uint8[n, N]: OracleScheduler.evaluate's fail codes of every probe pod after the fill."""
    from oracle.pyoracle import OracleScheduler

    probe = case.probe if probe is None else probe
    orc = OracleScheduler(case.cfg)
    try:
        case.load(orc)
        return np.stack([orc.evaluate(probe, i)[1].copy() for i in range(len(probe))])
    finally:
        orc.close()


_ORACLE = {}


def oracle_codes_cached(policy: str, nn: int) -> np.ndarray:
    """The reference codes of xcase(policy, nn), computed once and left unchanged."""
    if (policy, nn) not in _ORACLE:
        a = oracle_codes(xcase(policy, nn))
        a.setflags(write=False)
        _ORACLE[policy, nn] = a
    return _ORACLE[policy, nn]
