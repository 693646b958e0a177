"""Thin object wrapper over one libkschedgpu.so context.

`DeviceScheduler` owns a `ksg_ctx` (device memory, HIP stream, optional RCCL
communicator) and speaks in the interned numpy arrays of kubernetes_amd.ingest.
Every method maps 1:1 onto a C-ABI entry point of include/kschedgpu.h; any
non-OK return that is not a scheduling outcome raises KsgError. There is no
host-side evaluation here — the HIP kernels are the only implementation.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

from typing import Optional

import numpy as np

from . import abi


class KsgError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"ksg error {code}: {msg}")
        self.code = code


@dataclass
class ClusterArrays:
    """Interned node set: rank-ordered nodes, their label pair ids, pair->key."""

    nodes: np.ndarray  # NODE_DTYPE[N]
    node_pairs: np.ndarray  # uint32
    pair_keys: np.ndarray  # uint32[n_pairs] (entry 0 unused)
    n_services: int
    names: list = field(default_factory=list)  # node names in rank order (optional)

    @property
    def n_nodes(self) -> int:
        return int(self.nodes.shape[0])


@dataclass
class PodBatch:
    """Interned pods (POD_DTYPE) with their shared id list."""

    pods: np.ndarray
    ids: np.ndarray  # uint32
    # extensions (include/kschedgpu.h ksg_pod_ext, POD_EXT_DTYPE[n]; None: none)
    ext: Optional[np.ndarray] = None

    def __len__(self):
        return int(self.pods.shape[0])

    def one(self, i: int) -> "PodBatch":
        return PodBatch(self.pods[i : i + 1].copy(), self.ids,
                        None if self.ext is None else self.ext[i : i + 1].copy())



def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


class DeviceScheduler:
    """One scheduling context on one GPU (or one shard of a node-sharded set)."""

    def __init__(self, cfg: abi.KsgConfig, device: int = 0, rank: int = 0, world: int = 1,
                 nccl_id: bytes | None = None, allgather=None):
        """world > 1: exchange over RCCL (`nccl_id` from rank 0's nccl_unique_id()),
        or over the caller's transport `allgather(send: bytes) -> bytes` (the
        rank-major concatenation of every rank's `send`; ksg_set_allgather).
        world == 1 with an `nccl_id`: the exchange path over a 1-rank RCCL
        communicator (RCCL exercised on one GPU)."""
        self._lib = abi.load_library()
        self._ctx = C.c_void_p()
        self._xfn = None
        if world == 1 and nccl_id is None:
            rc = self._lib.ksg_create(C.byref(cfg), device, C.byref(self._ctx))
        else:
            if (nccl_id is None) == (allgather is None):
                raise ValueError("a sharded context needs exactly one of nccl_id / allgather")
            idbuf = C.create_string_buffer(nccl_id, 128) if nccl_id is not None else None
            rc = self._lib.ksg_create_sharded(C.byref(cfg), device, rank, world, idbuf, C.byref(self._ctx))
        if rc != abi.KSG_OK:
            raise KsgError(rc, "ksg_create failed (see stderr)")
        self.cfg = cfg
        self.n_nodes = 0
        self.n_services = 0
        self.n_scalar = 0
        self.world = world
        self.rank = rank
        if world > 1 and allgather is not None:
            self._install_allgather(allgather)

    def _install_allgather(self, allgather):
        world = self.world

        def cb(_user, send, recv, nbytes):
            try:
                got = allgather(C.string_at(send, nbytes))
                if len(got) != world * nbytes:
                    return -1
                C.memmove(recv, got, world * nbytes)
                return 0
            except Exception:  # an exception must not unwind through C
                import traceback

                traceback.print_exc()
                return -1

        self._xfn = abi.ALLGATHER_FN(cb)  # kept alive with the context
        rc = self._lib.ksg_set_allgather(self._ctx, self._xfn, None)
        if rc != abi.KSG_OK:
            self._err(rc)

    @staticmethod
    def nccl_unique_id() -> bytes:
        lib = abi.load_library()
        buf = C.create_string_buffer(128)
        rc = lib.ksg_nccl_unique_id(buf)
        if rc != abi.KSG_OK:
            raise KsgError(rc, "ncclGetUniqueId failed")
        return buf.raw

    def close(self):
        if self._ctx:
            self._lib.ksg_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, rc: int):
        msg = self._lib.ksg_last_error(self._ctx)
        raise KsgError(rc, msg.decode() if msg else "")

    # ---- cluster / pod state ---------------------------------------------
    def set_cluster(self, cl: ClusterArrays):
        nodes = np.ascontiguousarray(cl.nodes, dtype=abi.NODE_DTYPE)
        np_ = _u32(cl.node_pairs if len(cl.node_pairs) else np.zeros(1, np.uint32))
        pk = _u32(cl.pair_keys if len(cl.pair_keys) else np.zeros(1, np.uint32))
        rc = self._lib.ksg_set_cluster(self._ctx, abi.ptr(nodes), len(nodes), abi.ptr(np_), len(cl.node_pairs),
                                       abi.ptr(pk), len(pk), int(cl.n_services))
        if rc != abi.KSG_OK:
            self._err(rc)
        self.n_nodes = len(nodes)
        self.n_services = int(cl.n_services)

    def update_cluster(self, cl: ClusterArrays, old_to_new, outside=(), node_ext=None):
        """ksg_update_cluster: `cl` replaces the node list and every live pod stays, on its renamed
        host. old_to_new[r] = the host id of old node r's pods now (>= len(cl.nodes): the node left);
        outside = (old id, new id) pairs of the hosts outside the old list (ClusterView.host_map
        builds both); node_ext = set_node_ext's (scalar_cap, taint_off, taint_n, taint_ids) for the
        new list, required exactly when the context has extensions. The service count must not have
        changed; the static terms end (set_static_terms / add_static_config again)."""
        nodes = np.ascontiguousarray(cl.nodes, dtype=abi.NODE_DTYPE)
        np_ = _u32(cl.node_pairs if len(cl.node_pairs) else np.zeros(1, np.uint32))
        pk = _u32(cl.pair_keys if len(cl.pair_keys) else np.zeros(1, np.uint32))
        o2n = _u32(old_to_new)
        if len(o2n) != self.n_nodes:
            raise ValueError(f"old_to_new has {len(o2n)} entries for {self.n_nodes} old nodes")
        if int(cl.n_services) != self.n_services:
            raise ValueError("update_cluster keeps the service list: a changed one needs set_cluster")
        out = np.asarray(list(outside), dtype=np.uint32).reshape(-1, 2)
        oo, on = _u32(out[:, 0]), _u32(out[:, 1])
        ext = None
        if node_ext is not None:
            scalar_cap, taint_off, taint_n, taint_ids = node_ext
            cap = np.ascontiguousarray(scalar_cap, np.int64).reshape(-1)
            cap = cap if len(cap) else np.zeros(1, np.int64)
            ti = _u32(taint_ids if len(taint_ids) else np.zeros(1, np.uint32))
            toff, tn = _u32(taint_off), _u32(taint_n)  # (held: a converted copy must outlive the call)
            ext = abi.KsgNodeExtArrays(cap.ctypes.data, toff.ctypes.data if len(toff) else None,
                                       tn.ctypes.data if len(tn) else None, ti.ctypes.data, len(taint_ids))
        rc = self._lib.ksg_update_cluster(self._ctx, abi.ptr(nodes), len(nodes), abi.ptr(np_), len(cl.node_pairs),
                                          abi.ptr(pk), len(pk), abi.ptr(o2n) if len(o2n) else None,
                                          abi.ptr(oo) if len(oo) else None, abi.ptr(on) if len(on) else None, len(oo),
                                          C.byref(ext) if ext is not None else None)
        if rc != abi.KSG_OK:
            self._err(rc)
        self.n_nodes = len(nodes)

    def last_update_ms(self) -> float:
        """Device ms of the last update_cluster's remap kernels."""
        ms = C.c_double(0.0)
        self._lib.ksg_last_update_ms(self._ctx, C.byref(ms))
        return ms.value

    def last_update_host_us(self) -> dict:
        """Host microseconds of the last update_cluster by phase."""
        out = np.zeros(3, np.float64)
        self._lib.ksg_last_update_host_us(self._ctx, abi.ptr(out))
        return {"validate": float(out[0]), "device": float(out[1]), "mirror": float(out[2])}

    # ---- extensions (include/kschedgpu.h; parity unpinned) ---------------------
    def set_extensions(self, ext: abi.KsgExtConfig):
        rc = self._lib.ksg_set_extensions(self._ctx, C.byref(ext))
        if rc != abi.KSG_OK:
            self._err(rc)
        self.n_scalar = int(ext.n_scalar)

    def set_node_ext(self, scalar_cap: np.ndarray, taint_off: np.ndarray, taint_n: np.ndarray,
                     taint_ids: np.ndarray):
        """scalar_cap int64[n_scalar, N]; node n's taints taint_ids[taint_off[n]:+taint_n[n]]."""
        cap = np.ascontiguousarray(scalar_cap, np.int64).reshape(-1)
        cap = cap if len(cap) else np.zeros(1, np.int64)
        ti = _u32(taint_ids if len(taint_ids) else np.zeros(1, np.uint32))
        toff, tn = _u32(taint_off), _u32(taint_n)  # (held: a converted copy must outlive the call)
        rc = self._lib.ksg_set_node_ext(self._ctx, self.n_nodes, abi.ptr(cap), abi.ptr(toff), abi.ptr(tn), abi.ptr(ti),
                                        len(taint_ids))
        if rc != abi.KSG_OK:
            self._err(rc)

    def add_pod(self, host_id: int, batch: PodBatch, i: int = 0):
        pod = np.ascontiguousarray(batch.pods[i : i + 1])
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        if batch.ext is not None:
            ext = np.ascontiguousarray(batch.ext[i : i + 1], dtype=abi.POD_EXT_DTYPE)
            rc = self._lib.ksg_add_pod_ext(self._ctx, int(host_id), abi.ptr(pod), abi.ptr(ext), abi.ptr(ids))
        else:
            rc = self._lib.ksg_add_pod(self._ctx, int(host_id), abi.ptr(pod), abi.ptr(ids))
        if rc != abi.KSG_OK:
            self._err(rc)

    def remove_pod(self, uid: int):
        rc = self._lib.ksg_remove_pod(self._ctx, int(uid))
        if rc != abi.KSG_OK:
            self._err(rc)

    # ---- scheduling ---------------------------------------------------------
    def begin(self, batch: PodBatch, i: int = 0, want_fail: bool = False):
        """-> (rc, max_score, tie_count, fail_codes|None); rc in {OK, NOFIT, NONODES}."""
        pod = np.ascontiguousarray(batch.pods[i : i + 1])
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        m = C.c_int64(0)
        k = C.c_uint32(0)
        lo, hi = self.shard()
        fails = np.zeros(max(hi - lo, 1), np.uint8) if want_fail else None
        if batch.ext is not None:
            ext = np.ascontiguousarray(batch.ext[i : i + 1], dtype=abi.POD_EXT_DTYPE)
            rc = self._lib.ksg_schedule_begin_ext(self._ctx, abi.ptr(pod), abi.ptr(ext), abi.ptr(ids), C.byref(m),
                                                  C.byref(k), abi.ptr(fails))
        else:
            rc = self._lib.ksg_schedule_begin(self._ctx, abi.ptr(pod), abi.ptr(ids), C.byref(m), C.byref(k),
                                              abi.ptr(fails))
        if rc not in (abi.KSG_OK, abi.KSG_NOFIT, abi.KSG_NONODES):
            self._err(rc)
        return rc, m.value, k.value, (fails[: hi - lo] if fails is not None else None)

    def commit(self, tie_index: int) -> int:
        out = C.c_int32(-1)
        rc = self._lib.ksg_schedule_commit(self._ctx, int(tie_index), C.byref(out))
        if rc != abi.KSG_OK:
            self._err(rc)
        return out.value

    def batch(self, batch: PodBatch, rng_state: int):
        """Schedule every pod of the batch in order on the device. -> (out, rng_state)."""
        n = len(batch)
        pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        out = np.empty(max(n, 1), np.int32)
        st = C.c_uint64(rng_state)
        if batch.ext is not None:
            ext = np.ascontiguousarray(batch.ext, dtype=abi.POD_EXT_DTYPE)
            rc = self._lib.ksg_schedule_batch_ext(self._ctx, abi.ptr(pods), abi.ptr(ext), n, abi.ptr(ids),
                                                  len(batch.ids), C.byref(st), abi.ptr(out))
        else:
            rc = self._lib.ksg_schedule_batch(self._ctx, abi.ptr(pods), n, abi.ptr(ids), len(batch.ids),
                                              C.byref(st), abi.ptr(out))
        if rc != abi.KSG_OK:
            self._err(rc)
        return out[:n], st.value

    def batch_draws(self, batch: PodBatch, draws):
        """ksg_schedule_batch_draws: the batch with the caller's rand.Int() values
        (draws[k] for the k-th pod that finds a node). -> (out, draws used)."""
        n = len(batch)
        pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        out = np.empty(max(n, 1), np.int32)
        dr = np.ascontiguousarray(draws if len(draws) else np.zeros(1), dtype=np.uint64)
        used = C.c_uint32(0)
        rc = self._lib.ksg_schedule_batch_draws(self._ctx, abi.ptr(pods), n, abi.ptr(ids), len(batch.ids), abi.ptr(dr),
                                                len(draws), C.byref(used), abi.ptr(out))
        if rc != abi.KSG_OK:
            self._err(rc)
        return out[:n], int(used.value)

    def batch_unwind(self, batch: PodBatch, out, k: int, rng_state=None):
        """ksg_batch_unwind: pod k's Bind was rejected (scheduler.go:107-112). Undoes the
        commits of pods k..n-1 of the last batch; -> (draws pods 0..k consumed, the
        rng_state stepped back over pods k+1..n-1's draws, or None)."""
        n = len(batch)
        pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
        o = np.ascontiguousarray(out, dtype=np.int32)
        kept = C.c_uint32(0)
        st = C.c_uint64(0 if rng_state is None else int(rng_state))
        rc = self._lib.ksg_batch_unwind(self._ctx, abi.ptr(pods), abi.ptr(o), n, int(k),
                                        None if rng_state is None else C.byref(st), C.byref(kept))
        if rc != abi.KSG_OK:
            self._err(rc)
        return int(kept.value), (None if rng_state is None else st.value)

    def evaluate(self, batch: PodBatch, i: int = 0):
        """Per-node (fail code, combined score) of the shard, no commit."""
        pod = np.ascontiguousarray(batch.pods[i : i + 1])
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        lo, hi = self.shard()
        fails = np.zeros(max(hi - lo, 1), np.uint8)
        scores = np.zeros(max(hi - lo, 1), np.int64)
        if batch.ext is not None:
            ext = np.ascontiguousarray(batch.ext[i : i + 1], dtype=abi.POD_EXT_DTYPE)
            rc = self._lib.ksg_evaluate_ext(self._ctx, abi.ptr(pod), abi.ptr(ext), abi.ptr(ids), abi.ptr(fails),
                                            abi.ptr(scores))
        else:
            rc = self._lib.ksg_evaluate(self._ctx, abi.ptr(pod), abi.ptr(ids), abi.ptr(fails), abi.ptr(scores))
        if rc not in (abi.KSG_OK, abi.KSG_NONODES):
            self._err(rc)
        return rc, fails[: hi - lo], scores[: hi - lo]

    def explain(self, batch: PodBatch, want_codes: bool = True):
        """ksg_explain_batch: the predicates of every pod of `batch` against every node of the
        cluster as it stands, in one device pass, committing nothing.
        -> (codes uint8[n, N] | None, hist uint32[n, EXPLAIN_SLOTS], err uint8[n]): the per-node
        fail codes (want_codes), per pod the number of nodes with each code (slot 0: the nodes it
        fits), and 1 where the pod's ServiceAffinity peer is on an unknown host (rows zero)."""
        n = len(batch)
        pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        ext = None if batch.ext is None else np.ascontiguousarray(batch.ext, dtype=abi.POD_EXT_DTYPE)
        codes = np.zeros((n, self.n_nodes), np.uint8) if want_codes else None
        hist = np.zeros((n, abi.EXPLAIN_SLOTS), np.uint32)
        err = np.zeros(n, np.uint8)
        rc = self._lib.ksg_explain_batch(self._ctx, abi.ptr(pods), abi.ptr(ext), n, abi.ptr(ids), len(batch.ids),
                                         abi.ptr(codes) if want_codes and codes.size else None, abi.ptr(hist),
                                         abi.ptr(err))
        if rc not in (abi.KSG_OK, abi.KSG_NONODES):
            self._err(rc)
        return codes, hist, err

    def last_explain_ms(self) -> float:
        """Device ms of the last explain()'s kernel launches (HIP events)."""
        ms = C.c_double(0)
        self._lib.ksg_last_explain_ms(self._ctx, C.byref(ms))
        return ms.value

    def explain_without(self, batch: PodBatch, absent_uids, first_absent, want_codes: bool = True):
        """ksg_explain_without: explain() against the state with committed pods taken away.
        `absent_uids` is an ordered list of committed uids and `first_absent[i]` pod i's position
        in it: pod i is explained as if every pod of absent_uids[first_absent[i]:] had been
        removed first (nothing is). The batch's placed uids in order with the number placed before
        pod i give the state as of pod i; removable pods sorted by descending priority with the
        first entry below pod i's priority give preemption feasibility.
        -> (codes | None, hist, err) as explain()."""
        n = len(batch)
        pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        ext = None if batch.ext is None else np.ascontiguousarray(batch.ext, dtype=abi.POD_EXT_DTYPE)
        uids = np.ascontiguousarray(absent_uids, dtype=np.uint64)
        fa = _u32(first_absent)
        if len(fa) != n:
            raise ValueError(f"first_absent has {len(fa)} entries for {n} pods")
        codes = np.zeros((n, self.n_nodes), np.uint8) if want_codes else None
        hist = np.zeros((n, abi.EXPLAIN_SLOTS), np.uint32)
        err = np.zeros(n, np.uint8)
        rc = self._lib.ksg_explain_without(self._ctx, abi.ptr(pods), abi.ptr(ext), n, abi.ptr(ids), len(batch.ids),
                                           abi.ptr(uids) if len(uids) else None, len(uids),
                                           abi.ptr(fa) if n else None,
                                           abi.ptr(codes) if want_codes and codes.size else None, abi.ptr(hist),
                                           abi.ptr(err))
        if rc not in (abi.KSG_OK, abi.KSG_NONODES):
            self._err(rc)
        return codes, hist, err

    def last_explain_without_ms(self) -> float:
        """Device ms of the last explain_without()'s kernel launches (HIP events)."""
        ms = C.c_double(0)
        self._lib.ksg_last_explain_without_ms(self._ctx, C.byref(ms))
        return ms.value

    def preempt(self, batch: PodBatch, absent_uids, first_absent, max_victims: int = 16, want_per_node: bool = False):
        """ksg_preempt_batch: which committed pods would have to leave for each pod of `batch`,
        per node, and the node to preempt on. `absent_uids` lists the removable committed pods by
        descending priority and `first_absent[i]` is the first entry below pod i's priority, as
        explain_without() takes them; nothing is removed. On a node the pod fits with all of its
        removable pods away, they are put back one by one, most important first, while the pod
        still fits; the rest are the node's victims. The chosen node has the least important
        most-important victim (none at all first), then the fewest victims, then the highest rank.
        -> (best_node int32[n] (-1: no candidate), n_victims uint32[n], victims uint32[n,
        max_victims] (list indices in list order, 0xffffffff padding), cand_count uint32[n],
        free_count uint32[n] (candidates that need no eviction), node_victims uint32[n, N] | None
        (want_per_node; abi.PREEMPT_NOFIT where the node is no candidate)). A configuration with
        a ServiceAffinity predicate raises KsgError (KSG_ERR_STATE)."""
        n = len(batch)
        pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        ext = None if batch.ext is None else np.ascontiguousarray(batch.ext, dtype=abi.POD_EXT_DTYPE)
        uids = np.ascontiguousarray(absent_uids, dtype=np.uint64)
        fa = _u32(first_absent)
        if len(fa) != n:
            raise ValueError(f"first_absent has {len(fa)} entries for {n} pods")
        best = np.full(n, -1, np.int32)
        nv = np.zeros(n, np.uint32)
        victims = np.full((n, max_victims), 0xFFFFFFFF, np.uint32)
        cand = np.zeros(n, np.uint32)
        free = np.zeros(n, np.uint32)
        per_node = np.full((n, self.n_nodes), abi.PREEMPT_NOFIT, np.uint32) if want_per_node else None
        rc = self._lib.ksg_preempt_batch(self._ctx, abi.ptr(pods), abi.ptr(ext), n, abi.ptr(ids), len(batch.ids),
                                         abi.ptr(uids) if len(uids) else None, len(uids), abi.ptr(fa) if n else None,
                                         int(max_victims), abi.ptr(best), abi.ptr(nv),
                                         abi.ptr(victims) if max_victims else None, abi.ptr(cand), abi.ptr(free),
                                         abi.ptr(per_node) if want_per_node and per_node.size else None)
        if rc not in (abi.KSG_OK, abi.KSG_NONODES):
            self._err(rc)
        return best, nv, victims, cand, free, per_node

    def last_preempt_ms(self) -> float:
        """Device ms of the last preempt()'s kernel launches (HIP events)."""
        ms = C.c_double(0)
        self._lib.ksg_last_preempt_ms(self._ctx, C.byref(ms))
        return ms.value

    def pack(self, batch: PodBatch, set_size, exclude=None, targets=None):
        """ksg_pack_batch: do the pods of each set fit together. Set s owns the next set_size[s]
        pods of `batch`; each pod in turn goes to the highest-rank node it fits on the committed
        state plus the set's own earlier pods (their requests, host ports and GCE PDs), less
        exclude[s] (a node rank, or abi.PACK_NO_NODE) and the nodes whose bit in `targets`
        (uint64[ceil(N / 64)]) is clear. Sets do not see each other and nothing is committed.
        First fit is a heuristic: a set that is placed whole fits, one that is not may still have
        a packing in another order (largest pods first helps).
        -> (out_nodes int32[n] (abi.KSG_OUT_NOFIT: no node), placed uint32[n_sets]). A
        configuration with a ServiceAffinity predicate raises KsgError (KSG_ERR_STATE)."""
        n = len(batch)
        pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        ext = None if batch.ext is None else np.ascontiguousarray(batch.ext, dtype=abi.POD_EXT_DTYPE)
        sizes = _u32(set_size)
        ns = len(sizes)
        ex = None if exclude is None else _u32(exclude)
        if ex is not None and len(ex) != ns:
            raise ValueError(f"exclude has {len(ex)} entries for {ns} sets")
        tw = None if targets is None else np.ascontiguousarray(targets, dtype=np.uint64)
        if tw is not None and len(tw) != (self.n_nodes + 63) // 64:
            raise ValueError(f"targets has {len(tw)} words for {self.n_nodes} nodes")
        out = np.full(n, abi.KSG_OUT_NOFIT, np.int32)
        placed = np.zeros(ns, np.uint32)
        rc = self._lib.ksg_pack_batch(self._ctx, abi.ptr(pods) if n else None, abi.ptr(ext), n, abi.ptr(ids),
                                      len(batch.ids), abi.ptr(sizes) if ns else None,
                                      abi.ptr(ex) if ex is not None and ns else None, ns,
                                      abi.ptr(tw) if tw is not None and len(tw) else None,
                                      abi.ptr(out) if n else None, abi.ptr(placed) if ns else None)
        if rc not in (abi.KSG_OK, abi.KSG_NONODES):
            self._err(rc)
        return out, placed

    def last_pack_ms(self) -> float:
        """Device ms of the last pack()'s kernel launch (HIP events)."""
        ms = C.c_double(0)
        self._lib.ksg_last_pack_ms(self._ctx, C.byref(ms))
        return ms.value

    def prioritize(self, batch: PodBatch, top: int = 0, want_scores: bool = False):
        """ksg_prioritize_batch: filter and score every pod of `batch` against every node of the
        cluster as it stands, in one device pass, committing nothing.
        -> (max_score int64[n], tie_count uint32[n], fit_count uint32[n], top_nodes int32[n, top],
        top_scores int64[n, top], scores int64[n, N] | None, err uint8[n]): what begin() would
        return for each pod now, the nodes it fits, the head of its HostPriorityList (score
        descending, then node rank descending; -1 / 0 past min(top, fit_count)), the per-node
        combined scores (want_scores; abi.SCORE_NOFIT where the pod does not fit), and 1 where
        the pod's ServiceAffinity peer is on an unknown host (its row: 0, 0, 0, -1 / 0, NOFIT)."""
        n = len(batch)
        pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        ext = None if batch.ext is None else np.ascontiguousarray(batch.ext, dtype=abi.POD_EXT_DTYPE)
        mx = np.zeros(n, np.int64)
        ties = np.zeros(n, np.uint32)
        fit = np.zeros(n, np.uint32)
        tn = np.full((n, top), -1, np.int32)
        ts = np.zeros((n, top), np.int64)
        scores = np.full((n, self.n_nodes), abi.SCORE_NOFIT, np.int64) if want_scores else None
        err = np.zeros(n, np.uint8)
        rc = self._lib.ksg_prioritize_batch(self._ctx, abi.ptr(pods), abi.ptr(ext), n, abi.ptr(ids), len(batch.ids),
                                            int(top), abi.ptr(mx), abi.ptr(ties), abi.ptr(fit),
                                            abi.ptr(tn) if tn.size else None, abi.ptr(ts) if ts.size else None,
                                            abi.ptr(scores) if want_scores and scores.size else None, abi.ptr(err))
        if rc not in (abi.KSG_OK, abi.KSG_NONODES):
            self._err(rc)
        return mx, ties, fit, tn, ts, scores, err

    def last_prioritize_ms(self) -> float:
        """Device ms of the last prioritize()'s kernel launches (HIP events)."""
        ms = C.c_double(0)
        self._lib.ksg_last_prioritize_ms(self._ctx, C.byref(ms))
        return ms.value

    def headroom(self, batch: PodBatch, limit: int, want_counts: bool = True):
        """ksg_headroom_batch: how many copies of every pod of `batch` each node of the cluster
        as it stands can take (placed one after another on that node, capped at `limit`), in one
        device pass, committing nothing.
        -> (total uint64[n], fit_count uint32[n], max_count uint32[n], bind_hist uint32[n,
        HEADROOM_SLOTS], counts uint32[n, N] | None, err uint8[n]): per pod the sum of the counts,
        the nodes with a non-zero count, the largest count, the nodes per binding constraint
        (abi.ROOM_*), the per-node counts (want_counts), and abi.HEADROOM_ERR_* for a pod whose
        ServiceAffinity peer is on an unknown host or that has a negative request (rows zero)."""
        n = len(batch)
        pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        ext = None if batch.ext is None else np.ascontiguousarray(batch.ext, dtype=abi.POD_EXT_DTYPE)
        total = np.zeros(n, np.uint64)
        fit = np.zeros(n, np.uint32)
        mx = np.zeros(n, np.uint32)
        hist = np.zeros((n, abi.HEADROOM_SLOTS), np.uint32)
        counts = np.zeros((n, self.n_nodes), np.uint32) if want_counts else None
        err = np.zeros(n, np.uint8)
        rc = self._lib.ksg_headroom_batch(self._ctx, abi.ptr(pods), abi.ptr(ext), n, abi.ptr(ids), len(batch.ids),
                                          int(limit), abi.ptr(total), abi.ptr(fit), abi.ptr(mx), abi.ptr(hist),
                                          abi.ptr(counts) if want_counts and counts.size else None, abi.ptr(err))
        if rc not in (abi.KSG_OK, abi.KSG_NONODES):
            self._err(rc)
        return total, fit, mx, hist, counts, err

    def last_headroom_ms(self) -> float:
        """Device ms of the last headroom()'s kernel launches (HIP events)."""
        ms = C.c_double(0)
        self._lib.ksg_last_headroom_ms(self._ctx, C.byref(ms))
        return ms.value

    def set_window(self, window: int):
        """Pods per speculative window (0 = exact one-pod-at-a-time kernel)."""
        rc = self._lib.ksg_set_window(self._ctx, int(window))
        if rc != abi.KSG_OK:
            self._err(rc)

    def last_batch_stats(self) -> dict:
        st = np.zeros(4, np.uint32)
        self._lib.ksg_last_batch_stats(self._ctx, abi.ptr(st))
        return {"windows": int(st[0]), "stops_service": int(st[1]), "stops_exhausted": int(st[2]),
                "stops_cache": int(st[3])}

    def last_batch_windows(self) -> int:
        return self.last_batch_stats()["windows"]

    def last_batch_kernel_ms(self) -> dict:
        """Window path: device ms of the snapshot kernel, of the resolver, windows."""
        o = np.zeros(3, np.float64)
        self._lib.ksg_last_batch_kernel_ms(self._ctx, abi.ptr(o))
        return {"eval_ms": float(o[0]), "resolve_ms": float(o[1]), "launches": int(o[2])}

    HOST_PHASES = ("validate", "upload", "setup", "enqueue", "mirror_replay", "round_wait", "final_wait",
                   "bookkeeping")

    def last_batch_host_us(self) -> dict:
        """Host microseconds of the last batch by phase (ksg_last_batch_host_us)."""
        o = np.zeros(8, np.float64)
        self._lib.ksg_last_batch_host_us(self._ctx, abi.ptr(o))
        return {k: float(v) for k, v in zip(self.HOST_PHASES, o)}

    def batch_totals(self) -> dict:
        """The per-batch diagnostics summed over every batch so far (ksg_batch_totals)."""
        o = np.zeros(24, np.float64)
        self._lib.ksg_batch_totals(self._ctx, abi.ptr(o))
        return {"batches": int(o[0]), "device_ms": float(o[1]), "eval_ms": float(o[2]),
                "resolve_ms": float(o[3]), "launches": int(o[4]), "windows": int(o[5]),
                "stops_service": int(o[6]), "stops_exhausted": int(o[7]), "stops_cache": int(o[8]),
                "host_us": {k: float(v) for k, v in zip(self.HOST_PHASES, o[9:17])},
                "wcap_sum": float(o[17]), "t0_ms": float(o[18])}

    def set_static_terms(self, fit_words, score, weighted: bool):
        """ksg_set_static_terms: static node terms past the config's slots (after
        set_cluster; fit_words uint64[ceil(N/64)] or None, score int64[N] or None)."""
        fw = None if fit_words is None else np.ascontiguousarray(fit_words, np.uint64)
        sc = None if score is None else np.ascontiguousarray(score, np.int64)
        rc = self._lib.ksg_set_static_terms(self._ctx, None if fw is None else abi.ptr(fw),
                                            None if sc is None else abi.ptr(sc), 1 if weighted else 0)
        if rc != abi.KSG_OK:
            self._err(rc)

    def add_static_config(self, extra: abi.KsgConfig):
        """ksg_add_static_config: one slot pass of LabelsPresence / LabelPreference terms
        past the config's slots, evaluated on the device from the node labels."""
        rc = self._lib.ksg_add_static_config(self._ctx, C.byref(extra))
        if rc != abi.KSG_OK:
            self._err(rc)

    def serve_stats(self) -> dict:
        """The resident begin/commit server (ksg_serve_stats)."""
        o = np.zeros(4, np.uint64)
        self._lib.ksg_serve_stats(self._ctx, abi.ptr(o))
        return {"launches": int(o[0]), "requests": int(o[1]), "running": bool(o[2]), "eligible": bool(o[3]),
                "grid": int(o[3]) == 2}

    def debug_counters(self) -> np.ndarray:
        """KSG_DEBUG=8 contexts: the window resolver's per-stage cycle counters
        (cycles / 64, summed over every window so far)."""
        o = np.zeros(abi.KSG_DEBUG_COUNTER_WORDS, np.int32)
        rc = self._lib.ksg_debug_counters(self._ctx, abi.ptr(o), len(o))
        if rc != abi.KSG_OK:
            self._err(rc)
        return o

    def last_batch_ms(self) -> float:
        ms = C.c_double(0)
        self._lib.ksg_last_batch_ms(self._ctx, C.byref(ms))
        return ms.value

    def shard(self):
        lo = C.c_uint32(0)
        hi = C.c_uint32(0)
        self._lib.ksg_shard(self._ctx, C.byref(lo), C.byref(hi))
        return lo.value, hi.value

    def admit(self, sets: np.ndarray, batch: PodBatch, pairs, mode: int = 3) -> np.ndarray:
        """Kubelet admission over many nodes' sets (ksg_admit.hip). mode 1:
        ksg_check_pods_exceeding_capacity (1 = fitting), 2: ksg_pod_matches_node_labels
        (1 = matches), 3: ksg_admit_pods (KSG_ADMIT_* codes)."""
        sets = np.ascontiguousarray(sets, dtype=abi.ADMISSION_SET_DTYPE)
        pods = np.ascontiguousarray(batch.pods, dtype=abi.POD_DTYPE)
        ids = _u32(batch.ids if len(batch.ids) else np.zeros(1, np.uint32))
        prs = _u32(pairs if len(pairs) else np.zeros(1, np.uint32))
        out = np.zeros(max(len(pods), 1), np.uint8)
        if mode == 1:
            rc = self._lib.ksg_check_pods_exceeding_capacity(self._ctx, abi.ptr(sets), len(sets), abi.ptr(pods),
                                                             len(pods), abi.ptr(out))
        elif mode == 2:
            rc = self._lib.ksg_pod_matches_node_labels(self._ctx, abi.ptr(sets), len(sets), abi.ptr(pods), len(pods),
                                                       abi.ptr(ids), len(batch.ids), abi.ptr(prs), len(pairs),
                                                       abi.ptr(out))
        else:
            rc = self._lib.ksg_admit_pods(self._ctx, abi.ptr(sets), len(sets), abi.ptr(pods), len(pods), abi.ptr(ids),
                                          len(batch.ids), abi.ptr(prs), len(pairs), abi.ptr(out))
        if rc != abi.KSG_OK:
            self._err(rc)
        return out[: len(pods)]

    def read_ext_used(self) -> np.ndarray:
        """Committed extended-resource usage, int64[n_scalar, n_nodes] (ksg_read_ext_used)."""
        u = np.zeros(max(self.n_scalar * self.n_nodes, 1), np.int64)
        rc = self._lib.ksg_read_ext_used(self._ctx, abi.ptr(u))
        if rc != abi.KSG_OK:
            self._err(rc)
        return u[: self.n_scalar * self.n_nodes].reshape(self.n_scalar, self.n_nodes)

    def read_requested(self):
        c = np.zeros(max(self.n_nodes, 1), np.int64)
        m = np.zeros(max(self.n_nodes, 1), np.int64)
        rc = self._lib.ksg_read_requested(self._ctx, abi.ptr(c), abi.ptr(m))
        if rc != abi.KSG_OK:
            self._err(rc)
        return c[: self.n_nodes], m[: self.n_nodes]

    def read_state(self) -> dict:
        """The rest of the committed per-node pod state as the device holds it (ksg_read_state):
        keymap uint64[max_conflict_keys, nw], svc_cnt int32[S, N], svc_bits uint64[S, nw],
        svc_max / svc_total / svc_peer int32[S], with nw = ceil(N / 64)."""
        return _read_state(lambda *a: self._lib.ksg_read_state(self._ctx, *a), self._err,
                           int(self.cfg.max_conflict_keys), self.n_services, self.n_nodes)


def _read_state(call, err, n_keys: int, n_services: int, n_nodes: int) -> dict:
    nw = (n_nodes + 63) // 64
    shapes = (("keymap", np.uint64, (n_keys, nw)), ("svc_cnt", np.int32, (n_services, n_nodes)),
              ("svc_bits", np.uint64, (n_services, nw)), ("svc_max", np.int32, (n_services,)),
              ("svc_total", np.int32, (n_services,)), ("svc_peer", np.int32, (n_services,)))
    bufs = [np.zeros(max(int(np.prod(s)), 1), t) for _, t, s in shapes]
    rc = call(*[abi.ptr(b) for b in bufs])
    if rc != abi.KSG_OK:
        err(rc)
    return {name: b[: int(np.prod(s))].reshape(s) for (name, _, s), b in zip(shapes, bufs)}


def gloo_allgather(group=None):
    """allgather callable for DeviceScheduler over a torch.distributed process
    group (host transport; e.g. gloo ranks sharing one GPU in tests)."""
    import torch
    import torch.distributed as dist

    def ag(send: bytes) -> bytes:
        t = torch.frombuffer(bytearray(send), dtype=torch.uint8)
        outs = [torch.empty_like(t) for _ in range(dist.get_world_size(group))]
        dist.all_gather(outs, t, group=group)
        return b"".join(o.numpy().tobytes() for o in outs)

    return ag


# ---- node sharding (host side of the multi-GPU exchange; include/kschedgpu.h) ----
REC_HDR_BYTES = C.sizeof(abi.KsgShardRecord)


def shard_range(n_nodes: int, rank: int, world: int):
    """ksg_shard_range: node range [lo, hi) of `rank`'s shard."""
    lib = abi.load_library()
    lo, hi = C.c_uint32(0), C.c_uint32(0)
    rc = lib.ksg_shard_range(int(n_nodes), int(rank), int(world), C.byref(lo), C.byref(hi))
    if rc != abi.KSG_OK:
        raise KsgError(rc, "ksg_shard_range")
    return lo.value, hi.value


def merge_records(records: np.ndarray, n_nodes: int, empty_priorities: bool = False,
                  rng_state: int | None = None, tie_index: int = 0):
    """ksg_merge_records over a uint8[world, rec_bytes] array of shard records.
    -> (rc, node, max_score, tie_count, rng_state)."""
    lib = abi.load_library()
    rec = np.ascontiguousarray(records, dtype=np.uint8)
    world, rec_bytes = rec.shape
    node = C.c_int32(-1)
    m = C.c_int64(0)
    k = C.c_uint64(0)
    st = C.c_uint64(rng_state or 0)
    rc = lib.ksg_merge_records(abi.ptr(rec), rec_bytes, world, int(n_nodes), 1 if empty_priorities else 0,
                               C.byref(st) if rng_state is not None else None, int(tie_index), C.byref(node),
                               C.byref(m), C.byref(k))
    if rc not in (abi.KSG_OK, abi.KSG_NOFIT, abi.KSG_ERR_NOPEER):
        raise KsgError(rc, "ksg_merge_records")
    return rc, node.value, m.value, k.value, (st.value if rng_state is not None else None)


def make_shard_record(fails: np.ndarray, scores: np.ndarray, lo: int, word_lo: int, nwords_max: int,
                      error: bool = False) -> np.ndarray:
    """Pack one shard's record (header + tie bitmap) from its per-node fail codes and scores
    (the layout ksg_scan_kernel writes; used by callers that evaluate shards themselves)."""
    out = np.zeros(REC_HDR_BYTES + 8 * nwords_max, np.uint8)
    hdr = abi.KsgShardRecord.from_buffer(out)
    fit = fails == 0
    hdr.error = 1 if error else 0
    if fit.any() and not error:
        m = int(scores[fit].max())
        ties = np.nonzero(fit & (scores == m))[0] + lo
        hdr.max_score = m
        hdr.tie_count = len(ties)
        words = out[REC_HDR_BYTES:].view(np.uint64)
        rel = ties - word_lo * 64
        np.bitwise_or.at(words, rel // 64, (np.uint64(1) << (rel % 64).astype(np.uint64)))
    else:
        hdr.max_score = -(1 << 63)
        hdr.tie_count = 0
    return out
