"""workload.make_pods + ingest.ingest_pods without the api objects: the same seeded pod stream,
drawn and interned with numpy, for runs whose pod count makes the per-object path the
bottleneck of their set-up (bench.py). The result is the PodBatch ingest_pods builds from
make_pods' list, array for array, and the interner ends in the same state
(tests/test_podstream.py).

splitmix64's k-th output is a function of seed + k * gamma, so a block of draws is one
vector expression; a pod consumes 6 to 9 of them (11 with dense selectors) depending on its
own draws, so the block is read as "a pod starting at draw k would take len[k] draws" and
the pods' starts are that map's orbit from the block's first draw.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import abi
from .api import ObjectMeta, Pod, PodSpec
from .engine import PodBatch
from .ingest import ClusterView, pair_is_valid
from .labels import selector_from_set

MI = 1 << 20
_MASK = (1 << 64) - 1
_GAMMA = 0x9E3779B97F4A7C15
_MEMS = np.array((128, 256, 512, 1024, 2048), np.int64) * MI
_MAX_DRAWS = 11  # cpu, memory, port?, port, pd?, pd, selector?, zone, dense value, dense key, app


@dataclass
class PodStream:
    """make_pods(n, rng, dense_sel=dense_sel) for a generator in this state; resources_only is
    config 1's strip (no ports, PDs or selectors on the pods; the draws are the same)."""
    state: int
    n: int
    dense_sel: int = 0
    resources_only: bool = False
    n_apps: int = 100
    port_frac: float = 0.10
    pd_frac: float = 0.05
    sel_frac: float = 0.20


def _draws(state: int, m: int) -> np.ndarray:
    """The generator's next m outputs from this state."""
    z = np.uint64(state) + np.arange(1, m + 1, dtype=np.uint64) * np.uint64(_GAMMA)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_pods(st: PodStream, chunk: int = 1 << 17) -> dict:
    """Every pod's fields as arrays (cpu milli, memory bytes, has_port / port, has_pd / pd,
    has_sel / zone / dense key / dense value, app), plus the generator state after the last pod."""
    P, D, S = int(st.port_frac * 1000), int(st.pd_frac * 1000), int(st.sel_frac * 1000)
    dense = 1 if st.dense_sel else 0
    cols = {k: [] for k in ("cpu", "mem", "has_port", "port", "has_pd", "pd", "has_sel", "zone", "dkey", "dval", "app")}
    state, done = st.state & _MASK, 0
    while done < st.n:
        c = min(chunk, st.n - done)
        K = _MAX_DRAWS * c
        r = _draws(state, K + _MAX_DRAWS)
        m1000 = (r % np.uint64(1000)).astype(np.int64)
        k = np.arange(K, dtype=np.int64)
        pf = m1000[k + 2] < P
        pos_pd = k + 3 + pf
        df = m1000[pos_pd] < D
        pos_sel = pos_pd + 1 + df
        sf = m1000[pos_sel] < S
        pos_app = pos_sel + 1 + sf * (1 + 2 * dense)
        ln = (pos_app + 1 - k).tolist()
        starts = [0] * c
        at = 0
        for i in range(c):
            starts[i] = at
            at += ln[at]
        s = np.asarray(starts, np.int64)
        ps, pp, pa = pos_sel[s], pos_pd[s], pos_app[s]
        cols["cpu"].append(100 * (1 + (r[s] % np.uint64(10)).astype(np.int64)))
        cols["mem"].append(_MEMS[(r[s + 1] % np.uint64(5)).astype(np.int64)])
        cols["has_port"].append(pf[s])
        cols["port"].append(8000 + (r[s + 3] % np.uint64(16)).astype(np.int64))
        cols["has_pd"].append(df[s])
        cols["pd"].append((r[pp + 1] % np.uint64(2000)).astype(np.int64))
        cols["has_sel"].append(sf[s])
        cols["zone"].append((r[ps + 1] % np.uint64(8)).astype(np.int64))
        # (make_pods' `sel[key] = value` draws the value, the right-hand side, first)
        cols["dval"].append((r[ps + 2] % np.uint64(8)).astype(np.int64))
        cols["dkey"].append((r[ps + 3] % np.uint64(max(st.dense_sel, 1))).astype(np.int64))
        cols["app"].append((r[pa] % np.uint64(st.n_apps)).astype(np.int64))
        state = (state + at * _GAMMA) & _MASK
        done += c
    out = {k_: (np.concatenate(v) if v else np.zeros(0, np.int64)) for k_, v in cols.items()}
    for k_ in ("has_port", "has_pd", "has_sel"):
        out[k_] = out[k_].astype(bool)
    out["state"] = state
    return out


def ingest_stream(view: ClusterView, st: PodStream, aff_labels=(), chunk: int = 1 << 17) -> PodBatch:
    """ingest_pods(view, make_pods(...), aff_labels=aff_labels) of the stream's pods (uids 1..n)."""
    it = view.interner
    d = draw_pods(st, chunk)
    n = st.n
    has_port, has_pd, has_sel = d["has_port"], d["has_pd"], d["has_sel"]
    if st.resources_only:
        has_port = has_pd = has_sel = np.zeros(n, bool)

    # host ports and PD names share one id space, numbered by first appearance (a pod's ports
    # before its PDs): code 0..15 the ports, 16.. the PDs
    code_port = np.where(has_port, d["port"] - 8000, -1)
    code_pd = np.where(has_pd, 16 + d["pd"], -1)
    ev = np.stack([code_port, code_pd], axis=1).ravel()
    ev = ev[ev >= 0]
    uniq, first = np.unique(ev, return_index=True)
    conflict = np.zeros(16 + 2000, np.int64)
    for code in uniq[np.argsort(first)].tolist():
        conflict[code] = (it.conflict_id("port", 8000 + code) if code < 16
                          else it.conflict_id("pd", f"pd-{code - 16}"))

    # nodeSelector -> pair ids and the ServiceAffinity pairs, once per distinct selector
    sel_code = np.where(has_sel, d["zone"] + 8 * ((1 + d["dkey"] * 8 + d["dval"]) if st.dense_sel else 0), -1)
    n_codes = 8 * (1 + 8 * st.dense_sel)
    sel_n = np.zeros(n_codes, np.int64)
    sel_ids = np.zeros((n_codes, 2), np.int64)
    aff_tab = np.full((n_codes, abi.MAX_AFF), -1, np.int64)
    for code in np.unique(sel_code[sel_code >= 0]).tolist():
        ns = {"zone": f"z{code % 8}"}
        if st.dense_sel:
            ns[f"k{(code // 8 - 1) // 8}"] = f"v{(code // 8 - 1) % 8}"
        ids = [it.pair_id(k_, v_, create=False) for k_, v_ in selector_from_set(ns).requirements]
        sel_n[code] = len(ids)
        sel_ids[code, :len(ids)] = ids
        for j, l in enumerate(aff_labels):
            if l in ns:
                aff_tab[code, j] = it.pair_id(l, ns[l], create=False) if pair_is_valid(l, ns[l]) else abi.AFF_INVALID

    # the services selecting a pod, once per app label
    svcs = [view.pod_services(Pod(metadata=ObjectMeta(name="p", namespace="default", labels={"app": f"a{a}"}),
                                  spec=PodSpec(containers=[]))) for a in range(st.n_apps)]
    width = max([len(s_) for s_ in svcs] + [1])
    svc_n = np.array([len(s_) for s_ in svcs], np.int64)
    svc_tab = np.full((st.n_apps, width), -1, np.int64)
    for a, s_ in enumerate(svcs):
        svc_tab[a, :len(s_)] = s_

    n_ports, n_pds = has_port.astype(np.int64), has_pd.astype(np.int64)
    sc = np.maximum(sel_code, 0)
    n_sel = np.where(has_sel, sel_n[sc], 0)
    n_svcs = svc_n[d["app"]]
    per_pod = n_ports + n_pds + n_sel + n_svcs
    base = np.cumsum(per_pod) - per_pod
    ids = np.zeros(int(per_pod.sum()), np.uint32)
    ids[base[has_port]] = conflict[code_port[has_port]]
    pds_off = base + n_ports
    ids[pds_off[has_pd]] = conflict[code_pd[has_pd]]
    sel_off = pds_off + n_pds
    for j in range(2):
        m = n_sel > j
        ids[sel_off[m] + j] = sel_ids[sc[m], j]
    svcs_off = sel_off + n_sel
    for j in range(width):
        m = n_svcs > j
        ids[svcs_off[m] + j] = svc_tab[d["app"][m], j]

    arr = np.zeros(n, dtype=abi.POD_DTYPE)
    arr["uid"] = np.arange(1, n + 1, dtype=np.uint64)
    arr["milli_cpu"] = d["cpu"]
    arr["memory"] = d["mem"]
    arr["host"] = -1
    arr["service"] = np.where(n_svcs > 0, svc_tab[d["app"], 0], -1)
    arr["ports_off"], arr["n_ports"] = base, n_ports
    arr["pds_off"], arr["n_pds"] = pds_off, n_pds
    arr["sel_off"], arr["n_sel"] = sel_off, n_sel
    arr["svcs_off"], arr["n_svcs"] = svcs_off, n_svcs
    arr["aff_pair"] = np.where(has_sel[:, None], aff_tab[sc], -1)
    return PodBatch(arr, ids)
