"""kubernetes_amd/podstream.py (CPU): the vectorised pod stream is make_pods + ingest_pods, array
for array, with the interner and the generator left in the same state; chunks of every size meet
the same pods (a pod's draws may straddle two blocks of draws)."""
import numpy as np
import pytest

from kubernetes_amd import ingest, podstream, workload

N_PODS = 4000  # (~400 ports, ~200 PDs, ~800 selectors; config5: 32 dense selector keys x 8 values)


def _view(w):
    it = ingest.Interner()
    for k in w.config.label_keys():
        it.key_id(k)
    return ingest.ClusterView(w.nodes, w.services, it), it


@pytest.mark.parametrize("name,nodes", [("config1", 200), ("config2", 300), ("config4", 300), ("config5", 400)])
@pytest.mark.parametrize("chunk", [1 << 17, 777, 1])
def test_stream_is_the_object_path(name, nodes, chunk):
    n = N_PODS if chunk > 1 else 300
    w = workload.build(name, n_nodes=nodes, n_pods=n)
    view, it = _view(w)
    want = ingest.ingest_pods(view, w.pods, aff_labels=w.config.affinity_labels())
    ws = workload.build(name, n_nodes=nodes, n_pods=n, pod_stream=True)
    assert ws.pods == [] and ws.stream.n == n
    view_s, it_s = _view(ws)
    got = podstream.ingest_stream(view_s, ws.stream, aff_labels=ws.config.affinity_labels(), chunk=chunk)
    assert got.pods.dtype == want.pods.dtype and got.ids.dtype == want.ids.dtype
    assert got.pods.tobytes() == want.pods.tobytes()
    assert np.array_equal(got.ids, want.ids)
    assert it_s.conflict == it.conflict and list(it_s.conflict) == list(it.conflict)
    assert it_s.pairs == it.pairs and it_s.pair_key == it.pair_key and it_s.label_keys == it.label_keys


def test_stream_leaves_the_generator_where_make_pods_does():
    rng = workload._SM(workload.WORKLOAD_SEED)
    st = podstream.PodStream(rng.s, 2500, dense_sel=32)
    workload.make_pods(2500, rng, dense_sel=32)
    assert podstream.draw_pods(st, chunk=300)["state"] == rng.s
