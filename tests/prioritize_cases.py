"""The reference of the ksg_prioritize_batch tests (tests/test_prioritize_inputs.py on the CPU,
tests/test_gpu_prioritize.py on the device), derived from the C restatement's per-pod evaluate:
for a pod's row (rc, fails, scores), fit = fails == 0, max and ties come from scores[fit], and
the HostPriorityList is the fitting nodes sorted by (-score, -rank) (types.go:42-47).

The clusters are tests/explain_cases.py's (a fill batch, then probe pods) and tests/ext_cases.py's
with the scoring extensions on. Every reference is computed once and left unchanged."""
from __future__ import annotations

import functools

import numpy as np

from kubernetes_amd import abi
from kubernetes_amd.engine import PodBatch
from tests import explain_cases as X

TOP = 8
EXT_NODES = X.TILE + 1
EXT_FILL = X.N_FILL
EXT_PODS = X.N_FILL + X.N_PROBE
FILL_SEED = 1234


def reference(rows, top: int, empty_priorities: bool = False) -> dict:
    """rows: [(rc, fails, scores)] per pod -> the arrays ksg_prioritize_batch returns for them.
    A row with rc == KSG_ERR_NOPEER is an error row (err 1, zeros, -1 / 0, all NOFIT)."""
    n = len(rows)
    nn = len(rows[0][1]) if n else 0
    r = dict(max=np.zeros(n, np.int64), ties=np.zeros(n, np.uint32), fit=np.zeros(n, np.uint32),
             top_nodes=np.full((n, top), -1, np.int32), top_scores=np.zeros((n, top), np.int64),
             scores=np.full((n, nn), abi.SCORE_NOFIT, np.int64), err=np.zeros(n, np.uint8))
    for i, (rc, fails, scores) in enumerate(rows):
        if rc == abi.KSG_ERR_NOPEER:
            r["err"][i] = 1
            continue
        assert rc == abi.KSG_OK, rc
        fit = fails == 0
        r["fit"][i] = fit.sum()
        r["scores"][i, fit] = scores[fit]
        if not fit.any() or empty_priorities:
            continue
        idx = np.nonzero(fit)[0]
        r["max"][i] = scores[idx].max()
        r["ties"][i] = (scores[idx] == r["max"][i]).sum()
        order = idx[np.lexsort((idx, scores[idx]))][::-1][:top]  # score descending, then rank descending
        r["top_nodes"][i, : len(order)] = order
        r["top_scores"][i, : len(order)] = scores[order]
    for a in r.values():
        a.setflags(write=False)
    return r


def oracle_rows(case, probe=None, loader=None):
    """OracleScheduler.evaluate of every probe pod after the case's fill (copies)."""
    from oracle.pyoracle import OracleScheduler

    probe = case.probe if probe is None else probe
    orc = OracleScheduler(case.cfg)
    try:
        (loader or case.load)(orc)
        rows = []
        for i in range(len(probe)):
            rc, fails, scores = orc.evaluate(probe, i)
            rows.append((rc, fails.copy(), scores.copy()))
        return rows
    finally:
        orc.close()


@functools.lru_cache(maxsize=None)
def xreference(policy: str, nn: int, top: int = TOP) -> dict:
    """The reference of explain_cases.xcase(policy, nn)'s probe pods."""
    return reference(oracle_rows(X.xcase(policy, nn)), top)


class PExtCase:
    """tests/ext_cases.py's cluster with TaintToleration and BalancedResourceAllocation scored:
    the first EXT_FILL pods are the fill, the rest the probe pods (with records, and the
    ext == NULL form of the same pods)."""

    def __init__(self, name: str):
        from tests.ext_cases import ExtCase

        self.c = ExtCase(name, EXT_NODES, EXT_PODS, w_taint=1, w_bal=1)
        b = self.c.batch
        self.cfg, self.nn = self.c.cfg, EXT_NODES
        self.fill = PodBatch(b.pods[:EXT_FILL], b.ids, b.ext[:EXT_FILL])
        self.probe = PodBatch(b.pods[EXT_FILL:], b.ids, b.ext[EXT_FILL:])
        self.probe_plain = PodBatch(b.pods[EXT_FILL:], b.ids, None)

    def load(self, sched, seed: int = FILL_SEED):
        self.c.load(sched)
        return sched.batch(self.fill, seed)


@functools.lru_cache(maxsize=None)
def pext(name: str) -> PExtCase:
    return PExtCase(name)


@functools.lru_cache(maxsize=None)
def pext_reference(name: str, plain: bool, top: int = TOP) -> dict:
    c = pext(name)
    return reference(oracle_rows(c, c.probe_plain if plain else c.probe), top)
