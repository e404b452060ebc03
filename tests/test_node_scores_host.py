"""Per-pod node score offsets (ke_node_scores_load / ke_node_scores_set / ke_pod_node_scores, ABI v14, additive),
host side: the entry points' argument checks and the key-range cap, id staging and consumption, the refusals a call
with table ids meets before it needs the device, and two pins of the lock-step reference the GPU tests
(test_gpu_node_scores.py) use -- on the oracle alone: a constant offset shifts every score and moves no placement,
and a node set written as offsets places exactly as the node set."""
import numpy as np
import pytest

from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from oracle.binding import Oracle
from test_node_sets_host import code_of, ctx, manual_reserve, masked_argmax

T0 = synth.T0
CAP = 722  # synth.config: LoadAware, NodeNUMAResource, DeviceShare at weight 1 -> 1022 - 100 * 3


# ---- the reference shared with the GPU tests ---------------------------------------------------------------------
def offsets_of(tables, ids, n):
    """int64 [pod, node] offsets of the pods' tables (id 0: none); `tables` a [n_tables, <= n] matrix."""
    t = np.zeros((len(tables) + 1, n), np.int64)
    if len(tables):
        t[1:, :np.shape(tables)[1]] = tables
    return t[np.asarray(ids)]


def lockstep_scores(o, pods, off, elig=None):
    """One pod at a time on the oracle: its eval's total plus the offset where the total is >= 0, the masked argmax
    over the pod's set (lowest index on ties), then the Reserve by hand."""
    chosen, score = np.full(len(pods), -1, np.int32), np.full(len(pods), -1, np.int32)
    everywhere = np.ones(off.shape[1], bool)
    for p in range(len(pods)):
        t = o.eval(pods[p:p + 1], T0)["total"][0].astype(np.int64)
        t = np.where(t >= 0, t + off[p], -1)
        chosen[p], score[p] = masked_argmax(t, everywhere if elig is None else elig[p])
        if chosen[p] >= 0:
            manual_reserve(o, int(chosen[p]), pods[p])
    return chosen, score


# ---- 1: the ABI ------------------------------------------------------------------------------------------------------
def test_abi_is_additive(lib):
    assert abi.ABI_VERSION == 14 and lib.ke_abi_version() == 14
    for name in ("ke_node_scores_load", "ke_node_scores_set", "ke_pod_node_scores"):
        assert hasattr(lib, name), name
    assert abi.MAX_NODE_SCORE_TABLES == 1024


# ---- 2: load refusals ------------------------------------------------------------------------------------------------
def test_load_refusals():
    ev = ctx()
    v = np.zeros((abi.MAX_NODE_SCORE_TABLES + 1, 8), np.uint16)
    load = ev.lib.ke_node_scores_load
    assert load(ev.h, abi.MAX_NODE_SCORE_TABLES + 1, 8, abi.ptr(v)) == abi.ERR_INVALID
    assert load(ev.h, abi.MAX_NODE_SCORE_TABLES, 8, abi.ptr(v)) == abi.OK
    assert load(ev.h, -1, 8, abi.ptr(v)) == abi.ERR_INVALID
    assert load(ev.h, 1, -1, abi.ptr(v)) == abi.ERR_INVALID
    assert load(ev.h, 2, 8, None) == abi.ERR_INVALID
    assert load(None, 1, 8, abi.ptr(v)) == abi.ERR_INVALID
    assert load(ev.h, 0, 0, None) == abi.OK  # drops the table
    assert code_of(ev.pod_node_scores, [1]) == abi.ERR_INVALID


def test_load_cap_names_722_and_keeps_the_earlier_table():
    ev = ctx()
    t = np.zeros((2, 8), np.int64)
    t[1, 5] = CAP
    ev.node_scores_load(t)  # 722 loads
    t[0, 3] = CAP + 1
    with pytest.raises(KoordEvalError) as e:
        ev.node_scores_load(t)
    assert e.value.code == abi.ERR_UNSUPPORTED and str(CAP) in str(e.value), str(e.value)
    # the refused load left the earlier table (2 rows) valid: id 2 stages, id 3 does not
    ev.pod_node_scores([2, 0])
    assert code_of(ev.pod_node_scores, [3]) == abi.ERR_INVALID
    # other refused loads leave it too
    assert ev.lib.ke_node_scores_load(ev.h, 3, 8, None) == abi.ERR_INVALID
    ev.pod_node_scores([2])
    ev.pod_node_scores([])


# ---- 3: id staging and consumption -----------------------------------------------------------------------------------
def test_id_staging():
    ev = ctx()
    ev.node_scores_load(np.arange(16).reshape(2, 8))
    assert code_of(ev.pod_node_scores, [0, 3]) == abi.ERR_INVALID  # above n_tables
    assert code_of(ev.pod_node_scores, [-1]) == abi.ERR_INVALID
    ev.pod_node_scores([0, 1, 2])
    ev.pod_node_scores([])
    # a following call with a different n_pods is refused, and the ids are gone afterwards
    pods = synth.make_ds_pods(3, synth.BASE_SEED + 9302, device_fraction=1.0)
    ev.pod_node_scores([1, 1])
    assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID
    # (with the ids still staged this DeviceShare queue of 2 would be KE_ERR_UNSUPPORTED)
    try:
        ev.schedule(pods[:2], T0)
    except KoordEvalError as e:
        assert e.code == abi.ERR_NO_DEVICE
    # the same through ke_eval and ke_schedule_submit
    ev.pod_node_scores([1, 1])
    assert code_of(ev.eval, pods, T0) == abi.ERR_INVALID
    try:
        ev.eval(pods[:2], T0)
    except KoordEvalError as e:
        assert e.code == abi.ERR_NO_DEVICE
    ev.pod_node_scores([1, 1])
    assert code_of(ev.submit, pods, T0) == abi.ERR_INVALID
    # the keyword stages them too
    assert code_of(ev.schedule, pods, T0, node_scores=[1, 1]) == abi.ERR_INVALID
    assert code_of(ev.eval, pods, T0, node_scores=[1, 1]) == abi.ERR_INVALID
    assert code_of(ev.submit, pods, T0, node_scores=[1, 1]) == abi.ERR_INVALID
    # ids staged against a table replaced by a smaller one since
    ev.pod_node_scores([2, 0, 0])
    ev.node_scores_load(np.zeros((1, 8), np.int64))
    assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID
    # set ids and table ids of one call: both are consumed by a refused call
    ev.node_sets_load([[0, 1]], n_nodes=8)
    ev.pod_node_sets([1, 1])
    ev.pod_node_scores([1, 1, 1, 1])
    assert code_of(ev.schedule, pods[:2], T0) == abi.ERR_INVALID
    try:
        ev.schedule(pods[:2], T0)
    except KoordEvalError as e:
        assert e.code == abi.ERR_NO_DEVICE


# ---- 4: ke_node_scores_set ---------------------------------------------------------------------------------------------
def test_node_scores_set_refusals():
    ev = ctx()
    ev.node_scores_load(np.zeros((2, 6), np.int64))
    assert code_of(ev.node_scores_set, 0, [1]) == abi.ERR_INVALID            # n_tables differs
    assert code_of(ev.node_scores_set, 0, [1, 0, 1]) == abi.ERR_INVALID
    assert code_of(ev.node_scores_set, 6, [1, 0]) == abi.ERR_NOT_FOUND       # beyond the table's n_nodes
    assert code_of(ev.node_scores_set, -1, [1, 0]) == abi.ERR_NOT_FOUND
    with pytest.raises(KoordEvalError) as e:
        ev.node_scores_set(2, [0, CAP + 1])
    assert e.value.code == abi.ERR_UNSUPPORTED and str(CAP) in str(e.value)
    ev.node_scores_set(5, [CAP, 0])
    assert ev.lib.ke_node_scores_set(ev.h, 0, 2, None) == abi.ERR_INVALID
    ev.node_scores_load([])
    assert code_of(ev.node_scores_set, 0, [1, 0]) == abi.ERR_INVALID         # after the table was dropped
    assert code_of(ev.node_scores_set, 0, []) == abi.ERR_NOT_FOUND


# ---- 5: the refusals of a call with a non-zero id (before it needs the device) -----------------------------------------
def _plain(n, seed=9310):
    return synth.make_pods(n, synth.BASE_SEED + seed)


def _refused(ev, pods, ids, **kw):
    for call in (ev.schedule, ev.submit):
        ev.pod_node_scores(ids)
        with pytest.raises(KoordEvalError) as e:
            call(pods, T0, **kw)
        assert e.value.code == abi.ERR_UNSUPPORTED, str(e.value)
        assert "node scores" in str(e.value)
    return str(e.value)


def test_schedule_refusals_name_the_condition():
    ev = ctx()
    ev.node_scores_load(np.full((1, 8), 7))
    ds = synth.make_ds_pods(4, synth.BASE_SEED + 9311, device_fraction=1.0)
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
    cpuset = synth.make_cpuset_pods(6, synth.BASE_SEED + 9312, cpuset_fraction=1.0)
    assert "cpuset" in _refused(ev, cpuset, [1] * 6)
    # a non-zero set id next to a non-zero table id: the node sets' message stays
    ev.node_sets_load([[0, 1, 2]], n_nodes=8)
    for call in (ev.schedule, ev.submit):
        ev.pod_node_sets([0, 1, 0, 0])
        ev.pod_node_scores([1, 0, 0, 0])
        with pytest.raises(KoordEvalError) as e:
            call(ds, T0)
        assert e.value.code == abi.ERR_UNSUPPORTED and "node sets" in str(e.value) and "DeviceShare" in str(e.value)
    # set ids all 0 next to a non-zero table id: the node scores'
    ev.pod_node_sets([0, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, [1, 0, 0, 0])

    # every id 0: no refusal of the node scores' (the call gets as far as it does without them)
    for pods in (ds, numa):
        ev.pod_node_scores([0] * len(pods))
        try:
            ev.schedule(pods, T0)
        except KoordEvalError as e:
            assert "node scores" not in str(e)

def test_refusals_of_context_state():
    ev = ctx()
    ev.node_scores_load(np.full((1, 8), 7))
    cl = synth.make_cluster(8, synth.BASE_SEED + 9001)
    synth.load_numa(ev, synth.make_numa(cl, synth.BASE_SEED + 9313, policy_weights=(0.0, 0.4, 0.3, 0.3), no_zone_fraction=0.0))
    assert "NUMA" in _refused(ev, _plain(2), [1, 1])
    ev = Evaluator(synth.config(8, global_node_offset=8))
    synth.load_into(ev, cl)
    ev.node_scores_load(np.full((1, 8), 7))
    assert "sharded" in _refused(ev, _plain(2), [1, 1])
    ev.pod_node_scores([1, 1])
    with pytest.raises(KoordEvalError) as e:
        ev.eval(_plain(2), T0)
    assert e.value.code == abi.ERR_UNSUPPORTED and "node scores" in str(e.value)


# ---- 6: the reference, pinned on the oracle alone ----------------------------------------------------------------------
_REF = {}


def _ref():
    if not _REF:
        n = 150
        cl = synth.make_cluster(n, synth.BASE_SEED + 9321)
        pods = synth.make_pods(600, synth.BASE_SEED + 9322)
        _REF.update(n=n, cl=cl, pods=pods)
    return _REF


def _oracle(r):
    o = Oracle(synth.config(r["n"]), r["n"])
    synth.load_into(o, r["cl"])
    return o


def test_reference_constant_shift():
    r = _ref()
    n, pods = r["n"], r["pods"]
    rng = np.random.default_rng(synth.BASE_SEED + 9324)
    c = np.array([0, 5, 100, CAP, 37], np.int64)
    tables = np.repeat(c[:, None], n, axis=1)
    ids = rng.integers(0, len(c) + 1, len(pods))
    shift = np.concatenate([[0], c])[ids]
    c0, s0 = _oracle(r).schedule(pods, T0)
    c1, s1 = lockstep_scores(_oracle(r), pods, offsets_of(tables, ids, n))
    assert np.array_equal(c1, c0)
    assert np.array_equal(s1, np.where(c0 >= 0, s0 + shift, -1))
    assert (c0 >= 0).sum() > 300 and int(s1.max()) > 511


def test_reference_sets_expressed_as_offsets():
    r = _ref()
    n, pods = r["n"], r["pods"][:400]
    rng = np.random.default_rng(synth.BASE_SEED + 9324)
    sets = rng.random((4, n)) < 0.4
    ids = rng.integers(0, 5, len(pods))
    elig = np.concatenate([np.ones((1, n), bool), sets])[ids]
    zero = np.zeros((len(pods), n), np.int64)
    c0, s0 = lockstep_scores(_oracle(r), pods, zero, elig)  # the node sets' reference
    assert (c0 < 0).sum() == 0
    # table t = 400 on set t, 0 elsewhere: inside the set the offset outweighs every plugin total (<= 300), so as
    # long as the set holds a feasible node the placements are the node sets', the score + 400 (id 0: no offset)
    c1, s1 = lockstep_scores(_oracle(r), pods, offsets_of(np.where(sets, 400, 0), ids, n))
    assert np.array_equal(c1, c0)
    assert np.array_equal(s1, s0 + np.where(ids > 0, 400, 0))
