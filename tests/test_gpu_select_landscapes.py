"""k_select against the lock-step oracle reference on dictated score landscapes (landscapes.py), in the four select
configurations -- register-resident in one part, split in two parts with the in-launch merge, streamed
(k_select<false, 0>: a wave segment above 4096 nodes) in one part and in two -- and the three schedule modes: serial
(exact lists of k_j = j + 1 entries, so every list's last entry is consumed and a wrong threshold tie moves a
placement), pipelined with stale lists, pipelined with k_fixup.  Every case is bit-exact in placements and scores and
leaves exact records and rows.  The hot-node landscape makes speculative rounds fail on purpose; the DeviceShare and
NUMA queues at 66,061 nodes reach k_select<true, 0> and, in one part, the serial batches' streamed select."""
import numpy as np
import pytest

import landscapes as L
from koordinator_amd import Evaluator, synth
from oracle.binding import Oracle
from test_landscapes_host import assert_band_consumed
from test_node_scores_host import lockstep_scores, offsets_of

pytestmark = pytest.mark.gpu
T0 = synth.T0
MODES = {"serial": False, "stale-slots": True, "fixup": "fixup"}


def assert_placed(got, want):
    (c1, s1), (c0, s0) = got, want
    bad = np.flatnonzero((c1 != c0) | (s1 != s0))
    assert len(bad) == 0, (len(bad), [(int(p), int(p) % 64, int(c1[p]), int(c0[p]), int(s1[p]), int(s0[p])) for p in bad[:5]])


def assert_state_exact(ev):
    assert ev.check_records(T0) == 0
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)


def run_case(monkeypatch, config, name, mode, fix_merge=None):
    n, env, parts = L.CONFIGS[config]
    if env is not None:
        monkeypatch.setenv("KOORDEVAL_SELECT_PARTS", env)
    if fix_merge is not None:
        monkeypatch.setenv("KOORDEVAL_FIX_MERGE", fix_merge)
    g = L.select_boundaries(n, parts)
    assert g["streamed"] == config.startswith("stream")  # the dispatch's arithmetic: a segment above 4096 streams
    if g["streamed"]:
        assert g["seg"] > L.RESIDENT_SEG and all(p["seg"] > L.RESIDENT_SEG for p in g["parts"])
    c = L.landscape_reference(name, n, parts)
    if name.startswith("band-"):
        assert_band_consumed(c, n, parts, name[5:])
    ev = Evaluator(synth.config(n))
    synth.load_into(ev, c["cl"])
    if c["tables"] is not None:
        ev.node_scores_load(c["tables"])
    if c["sets"] is not None:
        ev.node_sets_load(c["sets"])
    ev.set_pipeline(MODES[mode])
    got = ev.schedule(c["pods"], T0, node_sets=c["sids"], node_scores=c["ids"])
    assert (ev.kernel_stats()["pipelined_batches"] > 0) == (mode != "serial")
    assert_placed(got, c["want"])
    assert (got[0] >= 0).all()
    assert_state_exact(ev)
    ev.close()


def _landscapes(config):
    return [x for x in L.LANDSCAPES if x != "band-part" or L.CONFIGS[config][2] > 1]


CASES = [(c, x) for c in L.CONFIGS for x in _landscapes(c)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("config,name", CASES, ids=[f"{c}-{x}" for c, x in CASES])
def test_landscape(gpu, monkeypatch, config, name, mode):
    run_case(monkeypatch, config, name, mode)


@pytest.mark.parametrize("name", _landscapes("split"))
def test_landscape_split_merge_in_select(gpu, monkeypatch, name):
    """The split select's last part merges the parts itself (KOORDEVAL_FIX_MERGE=0) instead of k_fixlist."""
    run_case(monkeypatch, "split", name, "stale-slots", fix_merge="0")


# ---- hot nodes: speculative rounds that fail -----------------------------------------------------------------------------
def _hot():
    def make():
        n, n_pods = 600, 256
        cl = synth.make_cluster(n, synth.BASE_SEED + 5)
        pods = synth.make_pods(n_pods, synth.BASE_SEED + 6)
        tables, ids = L.hot_nodes(n, n_pods)
        o = Oracle(synth.config(n), n)
        synth.load_into(o, cl)
        want = lockstep_scores(o, pods, offsets_of(tables, ids, n))
        in_batch, prev_batch, placed = L.repeat_counts(want[0], 64)
        assert 5 * in_batch >= placed and prev_batch >= 20
        return dict(n=n, cl=cl, pods=pods, tables=tables, ids=ids, want=want)
    return L.cached("hot", make)


def run_hot(cfg, mode):
    c = _hot()
    ev = Evaluator(cfg)
    synth.load_into(ev, c["cl"])
    ev.node_scores_load(c["tables"])
    ev.set_pipeline(MODES[mode])
    got = ev.schedule(c["pods"], T0, node_scores=c["ids"])
    ks = ev.kernel_stats()
    assert_placed(got, c["want"])
    if mode != "fixup":  # (the stale-list run and the serial batches use the speculative replay)
        assert ks["spec_failed_rounds"] > 0
    assert (ks["pipelined_batches"] > 0) == (mode != "serial")
    assert_state_exact(ev)
    ev.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("batch", [7, 64])
def test_hot_nodes(gpu, batch, mode):
    run_hot(synth.config(600, pod_batch=batch), mode)


def test_hot_nodes_without_t_helpers(gpu, monkeypatch):
    monkeypatch.setenv("KOORDEVAL_T_HELPERS", "0")
    run_hot(synth.config(600), "stale-slots")


# ---- the streamed select of DeviceShare and NUMA-policy batches (no offset tables) -----------------------------------
N_STREAM = L.CONFIGS["stream"][0]


def _big_cluster():
    return L.cached("big", lambda: synth.make_cluster(N_STREAM, synth.BASE_SEED + 9411))


def test_deviceshare_streamed_select(gpu):
    """A DeviceShare batch always selects in one part (the dispatch splits plain batches only): over 66,061 nodes a
    wave's segment is 4,608 nodes and k_select<true, 0> runs.  (The queue's plain batches split in two resident
    parts.)  Device caches on 1,500 scattered nodes; the others pass DeviceShare with score 0."""
    assert L.select_boundaries(N_STREAM, 1)["streamed"]  # parts = 1 whatever the batch size: a DeviceShare batch
    cl = _big_cluster()
    inner = 1 + np.random.default_rng(synth.BASE_SEED + 9412).choice(N_STREAM - 2, 1498, replace=False)
    with_cache = np.sort(np.concatenate([[0, N_STREAM - 1], inner]))
    devs = synth.make_devices(1500, synth.BASE_SEED + 9413, no_cache_fraction=0.0)
    pods = synth.make_ds_pods(120, synth.BASE_SEED + 9414)
    cfg = synth.config(N_STREAM)
    ev, o = Evaluator(cfg), Oracle(cfg, N_STREAM)
    for h in (ev, o):
        synth.load_into(h, cl)
        for i, d in zip(with_cache, devs):
            h.set_devices(int(i), d)
    got, want = ev.schedule(pods, T0), o.schedule(pods, T0)
    assert_placed(got, want)
    assert np.array_equal(ev.last_device_allocations, o.last_device_allocations)
    assert (ev.last_device_allocations != 0).sum() >= 20 and (got[0] >= 0).sum() >= 100
    assert_state_exact(ev)
    ev.close()


def test_numa_policy_streamed_select(gpu, monkeypatch):
    """A context with NUMA topology policies schedules in serial batches with lists of 64 entries.  Left alone the
    dispatch splits them in two register-resident parts at 66,061 nodes; in one part (KOORDEVAL_SELECT_PARTS=1, as the
    "stream" configuration) their select streams."""
    env = L.CONFIGS["stream"][1]
    monkeypatch.setenv("KOORDEVAL_SELECT_PARTS", env)
    for bp in (64, 32):  # the queue's batches: 96 pods
        parts = L.select_parts(N_STREAM, bp, env, list_len=64)
        assert parts == 1 and L.select_boundaries(N_STREAM, parts)["streamed"]
    assert not L.select_boundaries(N_STREAM, L.select_parts(N_STREAM, 64, None, list_len=64))["streamed"]
    cl = _big_cluster()
    nodes = cl.nodes.copy()  # (make_numa writes the policy labels: the shared cluster keeps none)
    numa_cl = synth.Cluster(cl.n_nodes, nodes, cl.nm, cl.has_nm, cl.pm_offsets, cl.pod_metrics, cl.agg_offsets,
                            cl.aggregated, cl.asg_nodes, cl.asg_pods, cl.asg_ts)
    head = synth.Cluster(2000, nodes[:2000], *[None] * 9)  # a view: zones and policies on the first 2,000 nodes
    zones = synth.make_numa(head, synth.BASE_SEED + 9416, zone_counts=(1, 2, 4))
    pods = synth.make_numa_pods(96, synth.BASE_SEED + 9417, policy_fraction=0.5)
    cfg = synth.config(N_STREAM)
    ev, o = Evaluator(cfg), Oracle(cfg, N_STREAM)
    for h in (ev, o):
        synth.load_into(h, numa_cl)
        synth.load_numa(h, zones)
    got, want = ev.schedule(pods, T0), o.schedule(pods, T0)
    assert_placed(got, want)
    assert np.array_equal(ev.last_numa_allocations, o.last_numa_allocations)
    assert (got[0] >= 0).sum() >= 80 and (ev.last_numa_allocations != 0).any(1).sum() >= 10
    assert_state_exact(ev)
    ev.close()
