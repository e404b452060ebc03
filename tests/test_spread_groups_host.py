"""Spread groups (ke_spread_groups_load / ke_spread_group_add / ke_spread_groups_get / ke_pod_spread_groups, ABI v14,
additive), host side: the entry points' argument checks and staging rules, the refusals a call with group ids meets
before it needs the device, and the lock-step reference of the GPU tests (test_gpu_spread_groups.py) pinned on the
oracle alone -- its inputs must make a site that ignores the cap, or reads a stale count, move a placement."""
import numpy as np
import pytest

from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from landscapes import HOT_NODES
from spread_groups import Lockstep, eligibility, fresh_oracle, make_input, offsets, reference, reference_without_groups
from test_node_sets_host import code_of, ctx

T0 = synth.T0


# ---- the entry points ------------------------------------------------------------------------------------------------
def test_abi_version_and_limits(lib):
    assert abi.ABI_VERSION == 14 and lib.ke_abi_version() == 14
    assert abi.MAX_SPREAD_GROUPS == 1024
    assert abi.STRUCTS[-1] is abi.PodDiagnosis  # no new struct: the entry points take plain arrays
    for name in ("ke_spread_groups_load", "ke_spread_group_add", "ke_spread_groups_get", "ke_pod_spread_groups",
                 "ke_debug_spread_groups_check"):
        assert hasattr(lib, name), name


def test_load_refusals():
    ev = ctx()
    caps = np.ones(abi.MAX_SPREAD_GROUPS + 1, np.uint16)
    load = ev.lib.ke_spread_groups_load
    assert load(ev.h, abi.MAX_SPREAD_GROUPS + 1, 8, None, abi.ptr(caps)) == abi.ERR_INVALID
    assert load(ev.h, abi.MAX_SPREAD_GROUPS, 8, None, abi.ptr(caps)) == abi.OK  # counts NULL: all zero
    assert not ev.spread_groups_get(abi.MAX_SPREAD_GROUPS, 8).any()
    assert load(ev.h, -1, 8, None, abi.ptr(caps)) == abi.ERR_INVALID
    assert load(ev.h, 1, -1, None, abi.ptr(caps)) == abi.ERR_INVALID
    assert load(ev.h, 2, 8, None, None) == abi.ERR_INVALID
    assert load(None, 1, 8, None, abi.ptr(caps)) == abi.ERR_INVALID
    caps[1] = 0  # every cap is >= 1
    assert load(ev.h, 2, 8, None, abi.ptr(caps)) == abi.ERR_INVALID
    # a refused load leaves the table as it was
    ev.pod_spread_groups([abi.MAX_SPREAD_GROUPS])
    assert load(ev.h, 0, 0, None, None) == abi.OK  # drops the table
    assert code_of(ev.pod_spread_groups, [1]) == abi.ERR_INVALID
    assert code_of(ev.spread_groups_get, 1, 8) == abi.ERR_NOT_FOUND
    assert ev.debug_spread_groups_check() == 0  # (nothing on a device to differ)


def test_counts_round_trip_and_add():
    ev = ctx()
    rng = np.random.default_rng(synth.BASE_SEED + 9660)
    counts = rng.integers(0, 5, (3, 8)).astype(np.uint16)
    ev.spread_groups_load(counts, [1, 2, 65535])
    for g in range(3):
        assert np.array_equal(ev.spread_groups_get(g + 1, 8), counts[g])
        got = ev.spread_groups_get(g + 1, 11)  # nodes at or beyond the table's n_nodes: count 0
        assert np.array_equal(got[:8], counts[g]) and not got[8:].any()
        assert np.array_equal(ev.spread_groups_get(g + 1, 3), counts[g][:3])
    # a narrower table: the nodes beyond it have count 0
    ev.spread_groups_load(counts[:, :5], [1, 2, 3])
    assert np.array_equal(ev.spread_groups_get(2, 8), np.concatenate([counts[1, :5], [0, 0, 0]]))
    # add: informer events and undos; clamps at 0, refuses to pass 65535
    ev.spread_groups_load(counts, [1, 2, 3])
    ev.spread_group_add(2, 4, 3)
    ev.spread_group_add(2, 4, -1)
    assert ev.spread_groups_get(2, 8)[4] == counts[1, 4] + 2
    ev.spread_group_add(2, 4, -100)
    assert ev.spread_groups_get(2, 8)[4] == 0
    ev.spread_group_add(1, 0, 65535 - int(counts[0, 0]))
    assert ev.spread_groups_get(1, 8)[0] == 65535
    assert code_of(ev.spread_group_add, 1, 0, 1) == abi.ERR_INVALID
    assert ev.spread_groups_get(1, 8)[0] == 65535
    assert code_of(ev.spread_group_add, 0, 0, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_group_add, 4, 0, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_group_add, 1, -1, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_group_add, 1, 1 << 20, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_groups_get, 0, 8) == abi.ERR_NOT_FOUND
    # the other rows are untouched
    assert np.array_equal(ev.spread_groups_get(3, 8), counts[2])
    with pytest.raises(ValueError):
        ev.spread_groups_load(counts, [1, 2])  # one row of counts per cap
    with pytest.raises(ValueError):
        ev.spread_groups_load(counts, [1, 2, 70000])


def test_id_staging():
    ev = ctx()
    ev.spread_groups_load(None, [1, 2], n_nodes=8)
    assert code_of(ev.pod_spread_groups, [0, 3]) == abi.ERR_INVALID  # above n_groups
    assert code_of(ev.pod_spread_groups, [-1]) == abi.ERR_INVALID
    ev.pod_spread_groups([0, 1, 2])
    ev.pod_spread_groups([])
    # a following call with a different n_pods is refused, and the ids are gone afterwards: consumed on failure
    pods = synth.make_ds_pods(3, synth.BASE_SEED + 9661, device_fraction=1.0)
    ev.pod_spread_groups([1, 1])
    assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID
    # (with the ids still staged this DeviceShare queue of 2 would be KE_ERR_UNSUPPORTED)
    try:
        ev.schedule(pods[:2], T0)
    except KoordEvalError as e:
        assert e.code == abi.ERR_NO_DEVICE
    # the same through ke_eval, ke_diagnose and ke_schedule_submit
    for call in (ev.eval, ev.diagnose, ev.submit):
        ev.pod_spread_groups([1, 1])
        assert code_of(call, pods, T0) == abi.ERR_INVALID
        try:
            call(pods[:2], T0)
        except KoordEvalError as e:
            assert e.code == abi.ERR_NO_DEVICE, call
    # the keyword stages them too
    assert code_of(ev.schedule, pods, T0, spread_groups=[1, 1]) == abi.ERR_INVALID
    # ids staged against a table replaced by a smaller one since
    ev.pod_spread_groups([2, 0, 0])
    ev.spread_groups_load(None, [4], n_nodes=8)
    assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID
    # group ids, set ids and table ids may be staged together; all are consumed by the one call
    ev.node_sets_load([[0, 1]], n_nodes=8)
    ev.node_scores_load([[1] * 8])
    ev.pod_spread_groups([1, 1])
    ev.pod_node_sets([1, 1, 1])
    ev.pod_node_scores([1, 1, 1])
    assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID  # (the group ids' n_pods)
    try:
        ev.schedule(pods, T0)
    except KoordEvalError as e:
        assert e.code == abi.ERR_NO_DEVICE


# ---- the refusals of a call with a non-zero id (before it needs the device) -------------------------------------------
def _plain(n, seed=9662):
    return synth.make_pods(n, synth.BASE_SEED + seed)


def _refused(ev, pods, ids, word="spread groups: ", **kw):
    for call in (ev.schedule, ev.submit):
        ev.pod_spread_groups(ids)
        for k, v in kw.items():
            getattr(ev, "pod_" + k)(v)
        with pytest.raises(KoordEvalError) as e:
            call(pods, T0)
        assert e.value.code == abi.ERR_UNSUPPORTED, str(e.value)
        assert word in str(e.value), str(e.value)
    return str(e.value)


def test_schedule_refusals_name_the_condition():
    ev = ctx()
    ev.spread_groups_load(None, [1], n_nodes=8)
    ds = synth.make_ds_pods(4, synth.BASE_SEED + 9663, device_fraction=1.0)
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
    cpuset = synth.make_cpuset_pods(6, synth.BASE_SEED + 9664, cpuset_fraction=1.0)
    assert "cpuset" in _refused(ev, cpuset, [1] * 6)
    # with a non-zero set / table id in the call the earlier message stays
    ev.node_sets_load([[0, 1, 2]], n_nodes=8)
    ev.node_scores_load([[1] * 8])
    assert "DeviceShare" in _refused(ev, ds, [0, 1, 0, 0], word="node sets: ", node_sets=[1, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, [0, 1, 0, 0], word="node scores: ", node_scores=[1, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, [0, 1, 0, 0], node_sets=[0] * 4, node_scores=[0] * 4)
    # every id 0: refused by nothing new (the call gets as far as it does without them)
    for pods in (ds, numa):
        ev.pod_spread_groups([0] * len(pods))
        try:
            ev.schedule(pods, T0)
        except KoordEvalError as e:
            assert "spread groups" not in str(e)


def test_refusals_of_context_state():
    ev = ctx()
    ev.spread_groups_load(None, [1], n_nodes=8)
    cl = synth.make_cluster(8, synth.BASE_SEED + 9001)
    synth.load_numa(ev, synth.make_numa(cl, synth.BASE_SEED + 9665, policy_weights=(0.0, 0.4, 0.3, 0.3), no_zone_fraction=0.0))
    assert "NUMA" in _refused(ev, _plain(2), [1, 1])
    ev = Evaluator(synth.config(8, global_node_offset=8))
    synth.load_into(ev, cl)
    ev.spread_groups_load(None, [1], n_nodes=8)
    assert "sharded" in _refused(ev, _plain(2), [1, 1])
    for call in (ev.eval, ev.diagnose):
        ev.pod_spread_groups([1, 1])
        assert code_of(call, _plain(2), T0) == abi.ERR_UNSUPPORTED


# ---- the reference of the GPU tests, on the oracle alone -----------------------------------------------------------------
def test_reference_without_groups_is_the_oracles_schedule():
    c = make_input("A")
    ls = Lockstep(fresh_oracle(c), c["counts"], c["caps"])
    got = ls.run(c["pods"], np.zeros(len(c["pods"]), np.int32), eligibility(c), offsets(c))
    want = fresh_oracle(c).schedule(c["pods"], T0)
    assert np.array_equal(got[0], want[0])
    placed = want[0] >= 0
    assert placed.any() and np.array_equal(got[1][placed], want[1][placed])
    assert np.array_equal(ls.counts[1:], c["counts"])  # id 0 counts nothing


@pytest.mark.parametrize("name,own_batch,unplaced", [("A", 20, 0), ("B", 80, 0), ("C", 150, 40)])
def test_reference_depends_on_the_counts(name, own_batch, unplaced):
    r = reference(name)
    chosen = r["want"][0]
    print(name, "grouped", int((r["gids"] > 0).sum()), "best capped", r["best_capped"], "own batch", r["own_batch"],
          "unplaced", r["unplaced"])
    assert r["own_batch"] >= own_batch
    assert r["unplaced"] >= unplaced if unplaced else r["unplaced"] == 0
    assert r["best_capped"] >= r["own_batch"] > 0
    # the result respects every cap, and the counts are the seeds plus the placements
    add = np.zeros_like(r["counts"], dtype=np.int64)
    for p in np.nonzero((chosen >= 0) & (r["gids"] > 0))[0]:
        add[r["gids"][p] - 1, chosen[p]] += 1
    assert np.array_equal(r["counts_after"], r["counts"] + add)
    grew = add > 0
    assert (r["counts_after"][grew] <= np.broadcast_to(r["caps"][:, None], add.shape)[grew]).all()
    if name == "A":
        assert int((r["gids"] > 0).sum()) == 187


def test_reference_d_moves_most_placements():
    r = reference("D")
    free = reference_without_groups("D")
    differ = int((free[0] != r["want"][0]).sum())
    print("D own batch", r["own_batch"], "unplaced", r["unplaced"], "differ", differ)
    assert differ >= 150 and r["unplaced"] == 0 and r["own_batch"] > 0
    el = eligibility(r)
    placed = r["want"][0] >= 0
    assert el[np.nonzero(placed)[0], r["want"][0][placed]].all()
    assert not r["counts"].any() and (r["sids"] > 0).any()
    # without groups the offsets crowd the pods onto the hot nodes
    assert np.isin(free[0], HOT_NODES).sum() > np.isin(r["want"][0], HOT_NODES).sum()
