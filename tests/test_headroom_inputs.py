"""ksg_headroom_batch on the CPU (the C restatement alone): the header and the binding declare
the call; the closed form of include/kschedgpu.h equals the sequential rule it is defined by,
on every input tests/test_gpu_headroom.py then holds the kernel to; and those inputs are not
vacuous (a parity test over counts that are all 0 or all the limit would pass with a kernel
that divides nothing)."""
import os
import re

import numpy as np
import pytest

from kubernetes_amd import abi
from kubernetes_amd.engine import PodBatch
from tests import explain_cases as X
from tests import headroom_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "kschedgpu.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int ksg_headroom_batch(ksg_ctx* ctx, const ksg_pod* pods, const ksg_pod_ext* ext , uint32_t n, "
            "const uint32_t* ids, uint32_t n_ids, uint32_t limit , uint64_t* total , uint32_t* fit_count , "
            "uint32_t* max_count , uint32_t* bind_hist , uint32_t* counts , uint8_t* err );") in flat
    assert "int ksg_last_headroom_ms(ksg_ctx* ctx, double* ms);" in flat
    want = {"KSG_HEADROOM_SLOTS": abi.HEADROOM_SLOTS, "KSG_ROOM_NONE": abi.ROOM_NONE, "KSG_ROOM_LIMIT": abi.ROOM_LIMIT,
            "KSG_ROOM_DISK": abi.ROOM_DISK, "KSG_ROOM_PORTS": abi.ROOM_PORTS, "KSG_ROOM_CPU": abi.ROOM_CPU,
            "KSG_ROOM_MEMORY": abi.ROOM_MEMORY, "KSG_ROOM_SCALAR0": abi.ROOM_SCALAR0,
            "KSG_HEADROOM_ERR_PEER": abi.HEADROOM_ERR_PEER, "KSG_HEADROOM_ERR_NEGATIVE": abi.HEADROOM_ERR_NEGATIVE,
            "KSG_ABI_VERSION": 3}
    for name, value in want.items():
        m = re.search(r"#define %s (\d+)" % name, hdr)
        assert m and int(m.group(1)) == value, name
    assert (abi.HEADROOM_SLOTS, abi.ROOM_NONE, abi.ROOM_LIMIT, abi.ROOM_DISK, abi.ROOM_PORTS, abi.ROOM_CPU,
            abi.ROOM_MEMORY, abi.ROOM_SCALAR0, abi.HEADROOM_ERR_PEER, abi.HEADROOM_ERR_NEGATIVE) == (16, 0, 1, 2, 3, 4, 5, 6, 1, 2)
    assert abi.ROOM_SCALAR0 + abi.MAX_SCALAR <= abi.HEADROOM_SLOTS
    assert {"ksg_headroom_batch", "ksg_last_headroom_ms"} <= set(abi.EXPORTS)
    lib = abi.load_library()
    assert lib.ksg_headroom_batch.argtypes is not None and len(lib.ksg_headroom_batch.argtypes) == 13
    assert len(lib.ksg_last_headroom_ms.argtypes) == 2


@pytest.mark.parametrize("policy", X.POLICIES + ("ext",))
def test_closed_form_equals_sequential_rule(policy):
    nn = X.TILE + 1
    r = H.reference(policy, nn)
    assert r["counts"].shape == r["seq"].shape == (X.N_PROBE, nn)
    bad = np.argwhere(r["counts"] != r["seq"])
    assert bad.size == 0, f"first mismatches (pod, node) {bad[:6].tolist()}"
    H.check_stop_codes(r["counts"], r["bind"], r["stop"], H.LIMIT)
    if policy == "ext":  # the ext == NULL form skips the extension filters
        rp = H.reference(policy, nn, plain=True)
        assert np.array_equal(rp["counts"], rp["seq"]) and (rp["counts"] != r["counts"]).any()
        H.check_stop_codes(rp["counts"], rp["bind"], rp["stop"], H.LIMIT)
        assert not (rp["bind"] >= abi.ROOM_SCALAR0).any()


def test_fill_gives_every_probed_service_a_peer():
    """What makes the rounds reference valid for the ServiceAffinity policies: the nodes are
    independent once the pod's service has a peer (its node supplies the affinity labels)."""
    for policy in ("config4", "invalid_selectors"):
        case = H.hcase(policy, X.TILE + 1)
        r = H.reference(policy, X.TILE + 1)
        from oracle.pyoracle import OracleScheduler

        orc = OracleScheduler(case.cfg)
        try:
            case.load(orc)
            per_node, stop = H.sequential_per_node(orc, PodBatch(case.probe.pods[:4], case.probe.ids), H.LIMIT)
        finally:
            orc.close()
        assert np.array_equal(per_node, r["seq"][:4])


def test_no_peer_case():
    """config4 with no pod in the cluster: the first copy of a ServiceAffinity pod becomes its
    service's peer on that very node, so the per-node count is the closed form's all the same."""
    r = H.reference("nopeer", 65)
    assert np.array_equal(r["counts"], r["seq"])
    H.check_stop_codes(r["counts"], r["bind"], r["stop"], H.LIMIT)
    assert (r["counts"] > 1).any()


def test_inputs_are_not_vacuous():
    seen = set()
    for policy in X.POLICIES + ("ext", "nopeer"):
        nn = 65 if policy == "nopeer" else X.TILE + 1
        r = H.reference(policy, nn)
        c = r["counts"]
        if policy in X.POLICIES:
            assert (c == 0).any() and (c == 1).any() and ((c > 1) & (c < H.LIMIT)).any() and (c == H.LIMIT).any(), policy
        seen |= set(np.unique(r["bind"]).tolist())
    want = {abi.ROOM_NONE, abi.ROOM_LIMIT, abi.ROOM_DISK, abi.ROOM_PORTS, abi.ROOM_CPU, abi.ROOM_MEMORY, abi.ROOM_SCALAR0}
    assert want <= seen, sorted(want - seen)


def test_big_number_boundary():
    """Numerators near 2^62 over a divisor of 2^31 + 7 with limit 2^32 - 1: the quotient in
    Python integers, the boundary confirmed by the restatement with two adds."""
    from oracle.pyoracle import OracleScheduler

    case = H.hcase("big", 65)
    r = H.reference("big", 65, H.BIG_LIMIT)
    req = (1 << 31) + 7
    assert int(case.probe.pods["memory"][0]) == req
    orc = OracleScheduler(case.cfg)
    try:
        case.load(orc)
        usedm = orc.read_requested()[1].copy()
        for k, node in enumerate(H.BIG_NODES):
            avail = int(case.arrays.nodes["cap_memory"][node]) - int(usedm[node])
            q = avail // req
            assert avail > 1 << 53 and 1 << 30 < q < H.BIG_LIMIT
            assert int(r["counts"][0, node]) == q and int(r["bind"][0, node]) == abi.ROOM_MEMORY
            pod, _, ids = H._one(case.probe, 0)
            pod["uid"], pod["memory"] = H.UID0 + 2 * k, (q - 1) * req
            H._raw_add(orc, node, pod, None, ids)  # q - 1 copies' worth
            assert orc.evaluate(case.probe, 0)[1][node] == 0  # copy q still fits
            pod["uid"], pod["memory"] = H.UID0 + 2 * k + 1, req
            H._raw_add(orc, node, pod, None, ids)
            assert orc.evaluate(case.probe, 0)[1][node] == abi.FAIL_PODFITSRESOURCES  # copy q + 1 does not
    finally:
        orc.close()
    # the other nodes hold ordinary memories: small counts, several values
    others = np.delete(r["counts"][0], H.BIG_NODES)
    assert others.max() < 64 and len(np.unique(others)) > 2
