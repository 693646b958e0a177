"""The device's whole pod state against the plain model (tests/state_model.py) after every call.

Three writers update the mutable per-node state in HBM: the commit code of every kernel family,
the host mirror's patches (ksg_add_pod / ksg_remove_pod) and ksg_batch_unwind. Each sequence of
tests/state_model.py runs once per writer variant below; after every operation
ksg_read_state, ksg_read_requested and (extensions) ksg_read_ext_used must equal the model
computed from scratch from the list of live pods, as exact integers, and the placements, the
generator state / draws used and begin's (rc, max, ties) must equal the C restatement's. A
mismatch names the operation index, the operation, the array and the first differing (row, node).
tests/test_state_model.py asserts on the CPU what the sequences cover.

Variants (each set by the switch the rest of the suite uses for it):
  window 0 / 5 / 128            the exact one-pod kernel, the plain window resolvers
  KSG_FUSED=0 / 1               phase A launched apart / inside the resolver's launch
  KSG_SERVE=0 / default         begin/commit by launched kernels / by the resident server
  config 4, KSG_DEBUG 0 / 2048 / 4096   ServiceAntiAffinity: the re-rank resolver, no re-rank,
                                the re-rank in the LDS-slot resolver
  ext                           every extension on (taints, extended resources, both scores):
                                the XS resolvers and scalar_used, at windows 0 and 128
"""
import pytest

from kubernetes_amd.engine import DeviceScheduler
from tests.state_model import SEQUENCES, make_sequence, run_sequence

pytestmark = pytest.mark.gpu

_PLAIN = [s for s in SEQUENCES if s[0] != "ext" and s[1] == "plain"]
_C4 = [s for s in SEQUENCES if s[1] == "config4"]
_EXT = [s for s in SEQUENCES if s[0] == "ext"]
_SMALL = lambda seqs: [s for s in seqs if s[2] < 4097]
_BIG = lambda seqs: [s for s in seqs if s[2] == 4097]

# (variant name, window, environment)
_PLAIN_VARIANTS = [("w0", 0, {}), ("w5", 5, {}), ("w128", 128, {}), ("fused0", 128, {"KSG_FUSED": "0"}),
                   ("fused1", 128, {"KSG_FUSED": "1"}), ("serve0", 128, {"KSG_SERVE": "0"})]
_C4_VARIANTS = [("rerank", 128, {}), ("norerank", 128, {"KSG_DEBUG": "2048"}), ("ldsslot", 128, {"KSG_DEBUG": "4096"})]
_EXT_VARIANTS = [("xs128", 128, {}), ("xs0", 0, {})]

CASES = ([(v, s) for v in _PLAIN_VARIANTS for s in _SMALL(_PLAIN)] + [(_PLAIN_VARIANTS[2], s) for s in _BIG(_PLAIN)]
         + [(v, s) for v in _C4_VARIANTS for s in _SMALL(_C4)] + [(_C4_VARIANTS[0], s) for s in _BIG(_C4)]
         + [(v, s) for v in _EXT_VARIANTS for s in _EXT])

_cache = {}


def _sequence(spec):
    """One generated sequence per spec, shared by its variants (run_sequence does not change it)."""
    if spec not in _cache:
        _cache[spec] = make_sequence(*spec)
    return _cache[spec]


@pytest.mark.parametrize("variant,spec", CASES, ids=lambda x: x[0] if isinstance(x[1], int) else "-".join(map(str, x)))
def test_device_state_equals_model_after_every_call(variant, spec, monkeypatch):
    name, window, env = variant
    for k in ("KSG_FUSED", "KSG_SERVE", "KSG_DEBUG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (KSG_FUSED / KSG_SERVE: read by ksg_create; KSG_DEBUG: by ksg_set_cluster)
    seq = _sequence(spec)
    dev = DeviceScheduler(seq.cfg, device=0)
    try:
        dev.set_window(window)
        cov = run_sequence(seq, engine=dev)
        srv = dev.serve_stats()
        print(f"{name} {seq.name}: {cov} server {srv['launches']}/{srv['requests']}")
        assert cov["audits"] >= len(seq.ops)
        if "KSG_SERVE" in env:
            assert srv["launches"] == 0, srv
        elif spec[0] != "ext" and spec[1] == "plain":
            assert srv["requests"] > 0, srv  # (begin / commit went through the resident server)
        if window:
            # (the variant must have run its resolver: some batch took the window path)
            assert cov["windows"] > 0, cov
    finally:
        dev.close()
