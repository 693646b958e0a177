"""ksg_update_cluster without a GPU: the binding against the header, ClusterView.host_map on
hand-written name lists, and for every case of tests/update_cases.py the facts it is there for,
asserted on the StateModels before and after the renaming (the fill runs on the C restatement,
so a case cannot silently lose what it covers)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kubernetes_amd import abi, ingest
from kubernetes_amd.api import Node, NodeSpec, ObjectMeta, Quantity, ResourceList
from kubernetes_amd.modeler import PodMirror, SimpleModeler, StoreToPodLister
from oracle.pyoracle import OracleScheduler
from tests import update_cases as uc
from tests.state_model import diff_states, engine_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "kschedgpu.h"
#ifdef PROTO
int (*p_upd)(ksg_ctx*, const ksg_node*, uint32_t, const uint32_t*, uint32_t, const uint32_t*, uint32_t,
             const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, const ksg_node_ext_arrays*) = ksg_update_cluster;
int (*p_ms)(ksg_ctx*, double*) = ksg_last_update_ms;
int (*p_us)(ksg_ctx*, double*) = ksg_last_update_host_us;
_Static_assert(KSG_ABI_VERSION == 3, "the call is additive");
#else
#define P(f) printf(#f " %zu\n", offsetof(ksg_node_ext_arrays, f));
int main(void) {
  printf("size %zu\n", sizeof(ksg_node_ext_arrays));
  P(scalar_cap) P(taint_off) P(taint_n) P(taint_ids) P(n_taint_ids)
  return 0;
}
#endif
"""


def test_binding_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "layout"
    gcc = ["gcc", "-std=c11", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o"]
    subprocess.run(gcc + [str(tmp_path / "proto.o"), "-c", "-DPROTO"], check=True)  # the prototypes as declared
    subprocess.run(gcc + [str(exe)], check=True)
    got = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(abi.KsgNodeExtArrays)
    for name, _ in abi.KsgNodeExtArrays._fields_:
        assert int(got[name]) == getattr(abi.KsgNodeExtArrays, name).offset, name
    for s in ("ksg_update_cluster", "ksg_last_update_ms", "ksg_last_update_host_us"):
        assert s in abi.EXPORTS
    lib = abi.load_library()
    vp = C.c_void_p
    assert lib.ksg_update_cluster.argtypes == [vp, vp, abi.U32, vp, abi.U32, vp, abi.U32, vp, vp, vp, abi.U32,
                                               C.POINTER(abi.KsgNodeExtArrays)]
    assert lib.ksg_update_cluster.restype is C.c_int
    assert lib.ksg_last_update_ms.argtypes == [vp, C.POINTER(C.c_double)]


def _nodes(names):
    return [Node(metadata=ObjectMeta(name=n, labels={"zone": "z0"}),
                 spec=NodeSpec(capacity=ResourceList(cpu=Quantity.from_milli(1000), memory=Quantity.from_int(1 << 30))))
            for n in names]


def test_host_map_on_hand_written_lists():
    it = ingest.Interner()
    old = ingest.ClusterView(_nodes(["b", "d", "f"]), [], it)
    assert old.host_id("ghost") == 3 and old.host_id("c") == 4  # outside hosts 0 and 1
    new = ingest.ClusterView(_nodes(["a", "b", "c", "f"]), [], it)
    o2n, out = new.host_map(old)
    # b -> 1, d left (outside host 2 of the interner: 4 + 2), f -> 3
    assert o2n.dtype == np.uint32 and o2n.tolist() == [1, 6, 3]
    # ghost stays outside (3 + 0 -> 4 + 0), c joined at rank 2 (3 + 1 -> 2); d is old_to_new's
    assert sorted(out) == [(3, 4), (4, 2)]
    ids = o2n.tolist() + [b for _, b in out]
    assert len(set(ids)) == len(ids)
    # back again: d rejoins from outside, a and c leave
    o2n2, out2 = old.host_map(new)
    assert o2n2.tolist() == [3 + it.ext_hosts["a"], 0, 3 + it.ext_hosts["c"], 2]
    assert sorted(out2) == sorted([(4 + 0, 3 + 0), (4 + it.ext_hosts["d"], 1)])
    # nothing to nothing, and views of different interners
    e0, e1 = ingest.ClusterView([], [], it), ingest.ClusterView([], [], it)
    o, p = e1.host_map(e0)
    assert len(o) == 0 and all(a == b for a, b in p)
    with pytest.raises(ValueError):
        new.host_map(ingest.ClusterView(_nodes(["a"]), [], ingest.Interner()))


def test_host_map_equals_the_cases_name_maps():
    for name in ("shrink", "churn", "empty_out_in"):
        case = uc.UpdateCase(name)
        for l in case.hand_live():
            case.host_id(0, l.host)  # (the outside hosts get their numbers in the order the fill meets them)
        for step in range(case.steps):
            want_o2n, want_out = case.maps(step)
            o2n, out = case.views[step + 1].host_map(case.views[step])
            assert o2n.tolist() == want_o2n.tolist(), (name, step)
            assert sorted(out) == sorted(want_out), (name, step)


def test_pod_mirror_rehost_keeps_the_device_pods():
    class Sink:
        def add_pod(self, *a):
            raise AssertionError("rehost must not add")

        def remove_pod(self, *a):
            raise AssertionError("rehost must not remove")

    m = SimpleModeler(StoreToPodLister(), StoreToPodLister())
    mir = PodMirror(m, Sink(), lambda p, u: (0, None), lambda: 1)
    mir.on_device[(0, "ns/a")] = 7
    mir.pending["ns/b"] = (8, 3)
    mir.pending["ns/c"] = (9, 70)
    mir.rehost(lambda h: {3: 5, 70: 2}[h])
    assert mir.pending == {"ns/b": (8, 5), "ns/c": (9, 2)} and mir.on_device == {(0, "ns/a"): 7}
    assert mir.stats["rehosts"] == 1 and mir.stats["reloads"] == 0


@pytest.fixture(scope="module")
def filled():
    """name -> (case, live list of the fill on the C restatement)."""
    out = {}
    for name in uc.CASES:
        case = uc.UpdateCase(name)
        orc = case.load(OracleScheduler(case.cfg))
        live, _ = case.fill(orc)
        assert diff_states(engine_state(orc, 0), case.model(live, 0).arrays()) is None, name
        orc.close()
        out[name] = (case, live)
    return out


@pytest.mark.parametrize("name", uc.CASES)
def test_case_contains_what_it_is_there_for(filled, name):
    case, live = filled[name]
    got = uc.facts(case, live, 0)
    assert uc.EXPECT[name] <= got, (name, sorted(uc.EXPECT[name] - got))
    sizes = {"shift_front": (65, 66), "drop_last": (65, 64), "shrink": (130, 65), "grow": (65, 130),
             "churn": (700, 700), "permute": (130, 130), "empty_out_in": (65, 0)}[name]
    assert (case.n_nodes(0), case.n_nodes(1)) == sizes
    assert len(live) <= 600
    # the renaming is injective and lists every outside host that holds a pod
    o2n, out = case.maps(0)
    ids = o2n.tolist() + [b for _, b in out]
    assert len(set(ids)) == len(ids)
    listed = {a for a, _ in out}
    for l in live:
        h = case.host_id(0, l.host)
        assert h < case.n_nodes(0) or h in listed


def test_negative_pod_on_a_joining_host():
    """The variant for the score path: the only negative request is on an outside host that joins,
    and no node total is negative before or after (only the request itself can widen the context)."""
    case = uc.UpdateCase("churn", join_negative=True)
    orc = case.load(OracleScheduler(case.cfg))
    live, _ = case.fill(orc)
    orc.close()
    got = uc.facts(case, live, 0)
    assert "joined_negative" in got and "negative" not in got and "joined_outside" in got


def test_churn_and_permute_shapes(filled):
    case, _ = filled["churn"]
    old, new = set(case.names[0]), set(case.names[1])
    assert len(old - new) == 20 and len(new - old) == 20 and len(case.outside_join) == 5
    assert len(case.changed_cap) == 20 and len(case.changed_label) == 20 and case.names[2] == case.names[0]
    case, _ = filled["permute"]
    o2n, _ = case.maps(0)
    assert sorted(o2n.tolist()) == list(range(130)) and (np.diff(o2n.astype(np.int64)) < 0).any()  # not monotone
    assert [case.names[0][j] for j in case.perm] == case.names[1]


def test_rebuilt_oracle_equals_the_renamed_model(filled):
    """The specification's reference is self-consistent: the restatement rebuilt on the new list
    holds the renamed model's state (every case, every step)."""
    for name, (case, live) in filled.items():
        for step in range(1, case.steps + 1):
            orc = case.rebuild(OracleScheduler(case.cfg), live, step)
            assert diff_states(engine_state(orc, 0), case.model(live, step).arrays()) is None, (name, step)
            orc.close()
