"""Per-pod node eligibility sets (ABI v14), host side: the table and id entry points' argument checks, the Python
packer, the refusals a call with set ids meets before it needs the device, and the two oracle-based references the
GPU tests (test_gpu_node_sets.py) rely on -- a cluster gathered by an arbitrary node index list evaluates as the
full cluster's columns, and a Reserve applied by hand on the oracle equals the one its schedule() applies."""
import numpy as np
import pytest

from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from koordinator_amd.evaluator import pack_node_sets, unpack_node_sets
from oracle.binding import Oracle

EVAL_KEYS = ("status", "reason", "la", "numa", "total")


# ---- helpers shared with the GPU tests --------------------------------------------------------------------------
def gather_cluster(cl, idx):
    """The sub-cluster of nodes `idx` (any order, no repeats) of a synth.Cluster: node k of it is node idx[k]."""
    idx = np.asarray(idx, np.int64)
    pm = [cl.pod_metrics[cl.pm_offsets[i]:cl.pm_offsets[i + 1]] for i in idx]
    ag = [cl.aggregated[cl.agg_offsets[i]:cl.agg_offsets[i + 1]] for i in idx]
    pm_off = np.zeros(len(idx) + 1, cl.pm_offsets.dtype)
    ag_off = np.zeros(len(idx) + 1, cl.agg_offsets.dtype)
    pm_off[1:] = np.cumsum([len(x) for x in pm])
    ag_off[1:] = np.cumsum([len(x) for x in ag])
    back = np.full(cl.n_nodes, -1, np.int64)
    back[idx] = np.arange(len(idx))
    keep = back[cl.asg_nodes] >= 0
    cat = lambda parts, like: np.concatenate(parts) if len(parts) else like[:0].copy()  # noqa: E731
    return synth.Cluster(len(idx), cl.nodes[idx].copy(), cl.nm[idx].copy(), cl.has_nm[idx].copy(), pm_off,
                         cat(pm, cl.pod_metrics), ag_off, cat(ag, cl.aggregated),
                         back[cl.asg_nodes[keep]].astype(np.int32), cl.asg_pods[keep].copy(), cl.asg_ts[keep].copy(),
                         cl.now)


def sub_oracle(cfg_of, cl, idx, devices=None, tables=None):
    """An oracle over the sub-cluster of nodes `idx` (cfg_of(n) -> its config), with the nodes' device cache entries
    and node resource tables gathered the same way."""
    sub = gather_cluster(cl, idx)
    o = Oracle(cfg_of(len(idx)), len(idx))
    synth.load_into(o, sub)
    if devices is not None:
        synth.load_devices(o, [devices[int(i)] for i in idx])
    if tables is not None:
        synth.load_node_resources(o, [tables[int(i)] for i in idx])
    return o


def manual_reserve(o, node, pod):
    """What the oracle's schedule() Reserve does to `node` for a plain pod: the LoadAware assign cache entry and
    NodeInfo.Requested += the pod's cpu / memory requests."""
    o.assign_bulk([node], pod.reshape(1), [synth.T0])
    req = o.node_info_requested(node)[0]
    o.set_requested(node, int(req[0]) + int(pod["requests"][abi.RES_CPU]), int(req[1]) + int(pod["requests"][abi.RES_MEMORY]))


def masked_argmax(total, eligible):
    """selectHost over the eligible nodes: (node, total) of the highest total, lowest index on ties; (-1, -1)."""
    t = np.where(eligible, total.astype(np.int64), -1)
    n = int(np.argmax(t))
    return (n, int(t[n])) if t[n] >= 0 else (-1, -1)


def code_of(fn, *a, **k):
    with pytest.raises(KoordEvalError) as e:
        fn(*a, **k)
    return e.value.code


def ctx(n=8):
    cl = synth.make_cluster(n, synth.BASE_SEED + 9001)
    ev = Evaluator(synth.config(n))
    synth.load_into(ev, cl)
    return ev


# ---- the table ---------------------------------------------------------------------------------------------------
def test_abi_version_is_14(lib):
    assert abi.ABI_VERSION == 14 and lib.ke_abi_version() == 14
    assert abi.REASON_NODE_SET == 96 and abi.MAX_NODE_SETS == 4096


def test_load_refusals():
    ev = ctx()
    w = np.zeros(abi.MAX_NODE_SETS + 1, np.uint64)
    assert ev.lib.ke_node_sets_load(ev.h, abi.MAX_NODE_SETS + 1, 1, abi.ptr(w)) == abi.ERR_INVALID
    assert ev.lib.ke_node_sets_load(ev.h, abi.MAX_NODE_SETS, 1, abi.ptr(w)) == abi.OK
    assert ev.lib.ke_node_sets_load(ev.h, -1, 1, abi.ptr(w)) == abi.ERR_INVALID
    assert ev.lib.ke_node_sets_load(ev.h, 1, -1, abi.ptr(w)) == abi.ERR_INVALID
    assert ev.lib.ke_node_sets_load(ev.h, 2, 1, None) == abi.ERR_INVALID
    assert ev.lib.ke_node_sets_load(ev.h, 0, 0, None) == abi.OK  # drops the table
    assert ev.lib.ke_node_sets_load(None, 1, 1, abi.ptr(w)) == abi.ERR_INVALID
    # a refused load leaves the table as it was: ids of the earlier table stay invalid
    assert code_of(ev.pod_node_sets, [1]) == abi.ERR_INVALID


def test_id_staging():
    ev = ctx()
    ev.node_sets_load([[0, 1], [2]], n_nodes=8)
    assert code_of(ev.pod_node_sets, [0, 3]) == abi.ERR_INVALID  # above n_sets
    assert code_of(ev.pod_node_sets, [-1]) == abi.ERR_INVALID
    ev.pod_node_sets([0, 1, 2])
    ev.pod_node_sets([])
    # a following call with a different n_pods is refused, and the ids are gone afterwards
    pods = synth.make_ds_pods(3, synth.BASE_SEED + 9002, device_fraction=1.0)
    ev.pod_node_sets([1, 1])
    assert code_of(ev.schedule, pods, synth.T0) == abi.ERR_INVALID
    # (with the ids still staged this DeviceShare queue of 2 would be KE_ERR_UNSUPPORTED)
    try:
        ev.schedule(pods[:2], synth.T0)
    except KoordEvalError as e:
        assert e.code == abi.ERR_NO_DEVICE
    # the same through ke_eval and ke_schedule_submit
    ev.pod_node_sets([1, 1])
    assert code_of(ev.eval, pods, synth.T0) == abi.ERR_INVALID
    ev.pod_node_sets([1, 1])
    assert code_of(ev.submit, pods, synth.T0) == abi.ERR_INVALID
    # ids staged against a table replaced by a smaller one since
    ev.pod_node_sets([2, 0, 0])
    ev.node_sets_load([[0]], n_nodes=8)
    assert code_of(ev.schedule, pods, synth.T0) == abi.ERR_INVALID


def test_node_set_bits_refusals():
    ev = ctx()
    ev.node_sets_load([[0, 1], [2]], n_nodes=8)
    assert code_of(ev.node_set_bits, 0, [1]) == abi.ERR_INVALID           # n_sets differs
    assert code_of(ev.node_set_bits, 0, [1, 0, 1]) == abi.ERR_INVALID
    assert code_of(ev.node_set_bits, 64, [1, 0]) == abi.ERR_NOT_FOUND     # beyond 64 * words_per_set
    assert code_of(ev.node_set_bits, -1, [1, 0]) == abi.ERR_NOT_FOUND
    ev.node_set_bits(63, [1, 0])
    ev.node_sets_load([])
    assert code_of(ev.node_set_bits, 0, [1, 0]) == abi.ERR_INVALID
    assert code_of(ev.node_set_bits, 0, []) == abi.ERR_NOT_FOUND


@pytest.mark.parametrize("n", [1, 64, 65, 333])
def test_packer_round_trip(n):
    rng = np.random.default_rng(synth.BASE_SEED + n)
    m = rng.random((5, n)) < 0.4
    m[0], m[1] = True, False
    n_sets, wps, words = pack_node_sets(m)
    assert (n_sets, wps) == (5, (n + 63) // 64) and words.shape == (5, wps) and words.dtype == np.uint64
    for s in range(5):
        for i in range(n):  # bit i & 63 of word i >> 6 <-> node i
            assert bool((int(words[s, i >> 6]) >> (i & 63)) & 1) == bool(m[s, i])
        tail = int(words[s, -1]) >> (((n - 1) & 63) + 1) if n % 64 else 0
        assert tail == 0
    assert np.array_equal(unpack_node_sets(words, n), m)
    # index lists pack to the same words
    n2, w2, words2 = pack_node_sets([np.nonzero(r)[0] for r in m], n_nodes=n)
    assert (n2, w2) == (n_sets, wps) and np.array_equal(words2, words)
    with pytest.raises(ValueError):
        pack_node_sets([[n]], n_nodes=n)


# ---- the refusals of a call with a non-zero id (before it needs the device) ---------------------------------------
def _plain(n, seed=9010):
    return synth.make_pods(n, synth.BASE_SEED + seed)


def _refused(ev, pods, ids, **kw):
    for call in (ev.schedule, ev.submit):
        ev.pod_node_sets(ids)
        with pytest.raises(KoordEvalError) as e:
            call(pods, synth.T0, **kw)
        assert e.value.code == abi.ERR_UNSUPPORTED, str(e.value)
        assert "node sets" in str(e.value)
    return str(e.value)


def test_schedule_refusals_name_the_condition():
    ev = ctx()
    ev.node_sets_load([[0, 1, 2]], n_nodes=8)
    ds = synth.make_ds_pods(4, synth.BASE_SEED + 9011, device_fraction=1.0)
    assert "DeviceShare" in _refused(ev, ds, [0, 1, 0, 0])
    numa = _plain(3)
    numa["numa_topology_policy"][1] = abi.NUMA_POLICY_SINGLE_NUMA_NODE
    assert "NUMA" in _refused(ev, numa, [1, 0, 0])
    quota = _plain(3)
    quota["quota"][2] = 1
    assert "ElasticQuota" in _refused(ev, quota, [1, 0, 0])
    for mode in (abi.RSV_MATCHED, abi.RSV_IGNORED, abi.RSV_AFFINITY):
        rsv = _plain(2)
        rsv["reservation_matched"][0] = mode
        assert "reservation" in _refused(ev, rsv, [0, 1])
    cpuset = synth.make_cpuset_pods(6, synth.BASE_SEED + 9012, cpuset_fraction=1.0)
    assert "cpuset" in _refused(ev, cpuset, [1] * 6)
    # every id 0: no refusal of the node sets' (the call gets as far as it does without them)
    for pods in (ds, numa):
        ev.pod_node_sets([0] * len(pods))
        try:
            ev.schedule(pods, synth.T0)
        except KoordEvalError as e:
            assert "node sets" not in str(e)


def test_refusals_of_context_state():
    ev = ctx()
    ev.node_sets_load([[0, 1, 2]], n_nodes=8)
    cl = synth.make_cluster(8, synth.BASE_SEED + 9001)
    synth.load_numa(ev, synth.make_numa(cl, synth.BASE_SEED + 9013, policy_weights=(0.0, 0.4, 0.3, 0.3), no_zone_fraction=0.0))
    assert "NUMA" in _refused(ev, _plain(2), [1, 1])
    ev = Evaluator(synth.config(8, global_node_offset=8))
    synth.load_into(ev, cl)
    ev.node_sets_load([[0, 1, 2]], n_nodes=8)
    assert "sharded" in _refused(ev, _plain(2), [1, 1])
    ev.pod_node_sets([1, 1])
    assert code_of(ev.eval, _plain(2), synth.T0) == abi.ERR_UNSUPPORTED


# ---- the references of the GPU tests -----------------------------------------------------------------------------
def test_gathered_sub_cluster_evaluates_as_the_columns():
    n = 333
    cl = synth.make_cluster(n, synth.BASE_SEED + 9020)
    pods = synth.make_pods(40, synth.BASE_SEED + 9021)
    full = Oracle(synth.config(n), n)
    synth.load_into(full, cl)
    want = full.eval(pods, synth.T0)
    rng = np.random.default_rng(synth.BASE_SEED + 9022)
    cls = rng.integers(0, 3, n)
    for c in range(3):
        idx = np.nonzero(cls == c)[0]
        got = sub_oracle(synth.config, cl, idx).eval(pods, synth.T0)
        for k in EVAL_KEYS:
            assert np.array_equal(got[k], want[k][:, idx]), (c, k)
    idx = rng.permutation(n)[:50]  # any order
    got = sub_oracle(synth.config, cl, idx).eval(pods, synth.T0)
    for k in EVAL_KEYS:
        assert np.array_equal(got[k], want[k][:, idx]), k


def test_gathered_sub_cluster_with_devices_and_resources():
    n = 96
    cl = synth.make_cluster(n, synth.BASE_SEED + 9030)
    devs = synth.make_devices(n, synth.BASE_SEED + 9031)
    tables = synth.make_node_resources(cl, synth.BASE_SEED + 9032)
    cfg_of = lambda m: synth.ext_config(synth.config(m))  # noqa: E731
    full = Oracle(cfg_of(n), n)
    synth.load_into(full, cl)
    synth.load_devices(full, devs)
    synth.load_node_resources(full, tables)
    pods = synth.add_pod_xres(synth.make_pods(20, synth.BASE_SEED + 9033), synth.BASE_SEED + 9034)
    want = full.eval(pods, synth.T0)
    idx = np.arange(1, n, 3)
    got = sub_oracle(cfg_of, cl, idx, devices=devs, tables=tables).eval(pods, synth.T0)
    for k in EVAL_KEYS:  # (plain pods: no DeviceShare normalisation over the node set)
        assert np.array_equal(got[k], want[k][:, idx]), k


def test_manual_reserve_equals_the_oracles():
    n = 150
    cl = synth.make_cluster(n, synth.BASE_SEED + 9040)
    pods = synth.make_pods(60, synth.BASE_SEED + 9041)
    probe = synth.make_pods(40, synth.BASE_SEED + 9042)
    a, b = Oracle(synth.config(n), n), Oracle(synth.config(n), n)
    synth.load_into(a, cl)
    synth.load_into(b, cl)
    everywhere = np.ones(n, bool)
    for p in range(len(pods)):
        node, total = masked_argmax(b.eval(pods[p:p + 1], synth.T0)["total"][0], everywhere)
        c, s = a.schedule(pods[p:p + 1], synth.T0)
        assert (int(c[0]), int(s[0]) if c[0] >= 0 else -1) == (node, total), p
        if node >= 0:
            manual_reserve(b, node, pods[p])
    ea, eb = a.eval(probe, synth.T0), b.eval(probe, synth.T0)
    for k in EVAL_KEYS + ("best",):
        assert np.array_equal(ea[k], eb[k]), k
