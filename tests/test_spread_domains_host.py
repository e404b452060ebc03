"""Spread domains (ke_spread_domains_load / ke_spread_domain_add / ke_spread_domain_node_set / ke_spread_domains_get /
ke_pod_spread_domains, ABI v14, additive), host side: the entry points' argument checks and staging rules, the
refusals a call with spread domain ids meets before it needs the device, and the lock-step reference of the GPU tests
(test_gpu_spread_domains.py) pinned on the oracle alone -- its inputs must make a site that ignores the skew, or reads
the counts of an earlier batch, move a placement."""
import numpy as np
import pytest

from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from spread_domains import (Lockstep, eligibility, fresh_oracle, full_mask, group_ids, make_input, offsets, open_domains,
                            reference, reference_without_domains)
from test_node_sets_host import code_of, ctx

T0 = synth.T0
NONE = abi.DOMAIN_NONE
I32 = lambda *v: np.array(v, np.int32)  # noqa: E731
U64 = lambda *v: np.array(v, np.uint64)  # noqa: E731


def _load(ev, n_maps, n_nodes, maps, n_groups, gmap, dom, skew, mind=None, counts=None):
    p = lambda a: None if a is None else abi.ptr(a)  # noqa: E731
    lib = (ev or ctx()).lib
    return lib.ke_spread_domains_load(ev.h if ev is not None else None, n_maps, n_nodes, p(maps), n_groups, p(gmap),
                                      p(dom), p(skew), p(mind), p(counts))


# ---- the entry points ------------------------------------------------------------------------------------------------
def test_abi_version_and_limits(lib):
    assert abi.ABI_VERSION == 14 and lib.ke_abi_version() == 14
    assert (abi.MAX_SPREAD_DOMAIN_GROUPS, abi.MAX_SPREAD_DOMAINS, abi.MAX_SPREAD_DOMAIN_MAPS) == (1024, 64, 8)
    assert abi.DOMAIN_NONE == 0xFFFF
    assert abi.STRUCTS[-1] is abi.PodDiagnosis  # no new struct: the entry points take plain arrays
    for name in ("ke_spread_domains_load", "ke_spread_domain_add", "ke_spread_domain_node_set", "ke_spread_domains_get",
                 "ke_pod_spread_domains", "ke_debug_spread_domains_check"):
        assert hasattr(lib, name), name


def test_load_refusals():
    ev = ctx()
    G = abi.MAX_SPREAD_DOMAIN_GROUPS
    maps = np.zeros((9, 8), np.uint16)
    gmap, dom, skew = np.ones(G + 1, np.int32), np.ones(G + 1, np.uint64), np.ones(G + 1, np.int32)
    assert _load(ev, 1, 8, maps, G + 1, gmap, dom, skew) == abi.ERR_INVALID
    assert _load(ev, 1, 8, maps, G, gmap, dom, skew) == abi.OK  # min_domains, counts NULL: all zero
    assert not ev.spread_domains_get(G).any()
    good = np.arange(64, dtype=np.uint32)
    assert _load(ev, 2, 8, maps, 1, I32(2), U64(3), I32(1), I32(0), good) == abi.OK
    assert np.array_equal(ev.spread_domains_get(1), good)
    bad = [
        _load(ev, 9, 8, maps, 1, gmap, dom, skew),            # more than MAX_SPREAD_DOMAIN_MAPS maps
        _load(ev, 0, 8, maps, 1, gmap, dom, skew),            # a group needs a map
        _load(ev, -1, 8, maps, 1, gmap, dom, skew),
        _load(ev, 1, -1, maps, 1, gmap, dom, skew),
        _load(ev, 1, 8, maps, -1, gmap, dom, skew),
        _load(ev, 1, 8, None, 1, gmap, dom, skew),
        _load(ev, 1, 8, maps, 1, None, dom, skew),
        _load(ev, 1, 8, maps, 1, gmap, None, skew),
        _load(ev, 1, 8, maps, 1, gmap, dom, None),
        _load(None, 1, 8, maps, 1, gmap, dom, skew),
        _load(ev, 1, 8, maps, 1, I32(2), dom, skew),           # map outside 1..n_maps
        _load(ev, 1, 8, maps, 1, I32(0), dom, skew),
        _load(ev, 1, 8, maps, 1, gmap, U64(0), skew),          # popcount(domains) >= 1
        _load(ev, 1, 8, maps, 1, gmap, dom, I32(0)),           # max_skew >= 1
        _load(ev, 1, 8, maps, 1, gmap, dom, skew, I32(-1)),    # min_domains >= 0
        _load(ev, 1, 8, maps, 1, gmap, dom, skew, None, np.full(64, 1 << 31, np.uint32)),
    ]
    assert bad == [abi.ERR_INVALID] * len(bad), bad
    m = maps.copy()
    m[0, 3] = 64  # a domain id >= 64 other than NONE
    assert _load(ev, 1, 8, m, 1, gmap, dom, skew) == abi.ERR_INVALID
    m[0, 3] = NONE
    # a refused load leaves the table as it was
    assert np.array_equal(ev.spread_domains_get(1), good)
    ev.pod_spread_domains([1])
    assert code_of(ev.pod_spread_domains, [2]) == abi.ERR_INVALID
    ev.spread_domain_node_set(2, 0, 5)
    assert _load(ev, 1, 8, m, 2, I32(1, 1), U64(1, 2), I32(1, 2)) == abi.OK
    assert not ev.spread_domains_get(2).any()
    assert _load(ev, 0, 0, None, 0, None, None, None) == abi.OK  # drops the table
    assert code_of(ev.pod_spread_domains, [1]) == abi.ERR_INVALID
    assert code_of(ev.spread_domains_get, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_domain_node_set, 1, 0, 0) == abi.ERR_NOT_FOUND
    assert ev.debug_spread_domains_check() == 0  # (nothing on a device to differ)


def test_counts_round_trip_add_and_node_set():
    ev = ctx()
    rng = np.random.default_rng(synth.BASE_SEED + 9780)
    counts = rng.integers(0, 5, (3, 64)).astype(np.uint32)
    maps = rng.integers(0, 64, (2, 8))
    ev.spread_domains_load(maps, [1, 2, 2], [full_mask(64), 1, 1 << 63], [1, 2, 3], [0, 0, 70], counts)
    for g in range(3):
        assert np.array_equal(ev.spread_domains_get(g + 1), counts[g])
    # add: informer events and undos; clamps at 0, refuses to pass 2^31-1
    ev.spread_domain_add(2, 4, 3)
    ev.spread_domain_add(2, 4, -1)
    assert ev.spread_domains_get(2)[4] == counts[1, 4] + 2
    ev.spread_domain_add(2, 4, -100)
    assert ev.spread_domains_get(2)[4] == 0
    top = (1 << 31) - 1
    ev.spread_domain_add(1, 63, top - int(counts[0, 63]))
    assert ev.spread_domains_get(1)[63] == top
    assert code_of(ev.spread_domain_add, 1, 63, 1) == abi.ERR_INVALID
    assert ev.spread_domains_get(1)[63] == top
    assert code_of(ev.spread_domain_add, 0, 0, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_domain_add, 4, 0, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_domain_add, 1, -1, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_domain_add, 1, 64, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_domains_get, 0) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_domains_get, 4) == abi.ERR_NOT_FOUND
    assert ev.lib.ke_spread_domains_get(ev.h, 1, None) == abi.ERR_INVALID
    assert np.array_equal(ev.spread_domains_get(3), counts[2])  # the other rows are untouched
    # node_set: 0..63 or NONE, a map of the table, a node of the context
    ev.spread_domain_node_set(1, 7, 63)
    ev.spread_domain_node_set(2, 0, NONE)
    assert code_of(ev.spread_domain_node_set, 1, 0, 64) == abi.ERR_INVALID
    assert code_of(ev.spread_domain_node_set, 1, 0, -1) == abi.ERR_INVALID
    assert code_of(ev.spread_domain_node_set, 0, 0, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_domain_node_set, 3, 0, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_domain_node_set, 1, -1, 1) == abi.ERR_NOT_FOUND
    assert code_of(ev.spread_domain_node_set, 1, 1 << 20, 1) == abi.ERR_NOT_FOUND
    assert ev.debug_spread_domains_check() == 0
    with pytest.raises(ValueError):
        ev.spread_domains_load(maps, [1, 2], [1, 1], [1, 1], counts=counts)  # counts is [n_groups, 64]
    with pytest.raises(ValueError):
        ev.spread_domains_load(maps, [1, 2], [1], [1, 1])
    ev.spread_domains_load(maps, [], [], [])  # no groups: drops the table
    assert code_of(ev.spread_domains_get, 1) == abi.ERR_NOT_FOUND


def test_id_staging():
    ev = ctx()
    ev.spread_domains_load(np.zeros((1, 8)), [1, 1], [1, 1], [1, 2])
    assert code_of(ev.pod_spread_domains, [0, 3]) == abi.ERR_INVALID  # above n_groups
    assert code_of(ev.pod_spread_domains, [-1]) == abi.ERR_INVALID
    assert ev.lib.ke_pod_spread_domains(ev.h, 2, None) == abi.ERR_INVALID
    ev.pod_spread_domains([0, 1, 2])
    ev.pod_spread_domains([])
    # a following call with a different n_pods is refused, and the ids are gone afterwards: consumed on failure
    pods = synth.make_ds_pods(3, synth.BASE_SEED + 9781, device_fraction=1.0)
    ev.pod_spread_domains([1, 1])
    assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID
    # (with the ids still staged this DeviceShare queue of 2 would be KE_ERR_UNSUPPORTED)
    try:
        ev.schedule(pods[:2], T0)
    except KoordEvalError as e:
        assert e.code == abi.ERR_NO_DEVICE
    # the same through ke_eval, ke_diagnose and ke_schedule_submit
    for call in (ev.eval, ev.diagnose, ev.submit):
        ev.pod_spread_domains([1, 1])
        assert code_of(call, pods, T0) == abi.ERR_INVALID
        try:
            call(pods[:2], T0)
        except KoordEvalError as e:
            assert e.code == abi.ERR_NO_DEVICE, call
    # the keyword stages them too
    for call in (ev.schedule, ev.submit, ev.eval, ev.diagnose):
        assert code_of(call, pods, T0, spread_domains=[1, 1]) == abi.ERR_INVALID
    # ids staged against a table replaced by a smaller one since
    ev.pod_spread_domains([2, 0, 0])
    ev.spread_domains_load(np.zeros((1, 8)), [1], [1], [4])
    assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID
    # domain ids, group ids, set ids and table ids may be staged together; all are consumed by the one call
    ev.node_sets_load([[0, 1]], n_nodes=8)
    ev.node_scores_load([[1] * 8])
    ev.spread_groups_load(None, [1], n_nodes=8)
    ev.pod_spread_domains([1, 1])
    ev.pod_spread_groups([1, 1, 1])
    ev.pod_node_sets([1, 1, 1])
    ev.pod_node_scores([1, 1, 1])
    assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID  # (the domain ids' n_pods)
    try:
        ev.schedule(pods, T0)
    except KoordEvalError as e:
        assert e.code == abi.ERR_NO_DEVICE


# ---- the refusals of a call with a non-zero id (before it needs the device) -------------------------------------------
def _plain(n, seed=9782):
    return synth.make_pods(n, synth.BASE_SEED + seed)


def _refused(ev, pods, ids, word="spread domains: ", **kw):
    for call in (ev.schedule, ev.submit):
        ev.pod_spread_domains(ids)
        for k, v in kw.items():
            getattr(ev, "pod_" + k)(v)
        with pytest.raises(KoordEvalError) as e:
            call(pods, T0)
        assert e.value.code == abi.ERR_UNSUPPORTED, str(e.value)
        assert word in str(e.value), str(e.value)
    return str(e.value)


def test_schedule_refusals_name_the_condition():
    ev = ctx()
    ev.spread_domains_load(np.zeros((1, 8)), [1], [1], [1])
    ds = synth.make_ds_pods(4, synth.BASE_SEED + 9783, device_fraction=1.0)
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
    cpuset = synth.make_cpuset_pods(6, synth.BASE_SEED + 9784, cpuset_fraction=1.0)
    assert "cpuset" in _refused(ev, cpuset, [1] * 6)
    # with a non-zero id of an earlier feature in the call that feature's message stays
    ev.node_sets_load([[0, 1, 2]], n_nodes=8)
    ev.node_scores_load([[1] * 8])
    ev.spread_groups_load(None, [1], n_nodes=8)
    assert "DeviceShare" in _refused(ev, ds, [0, 1, 0, 0], word="node sets: ", node_sets=[1, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, [0, 1, 0, 0], word="node scores: ", node_scores=[1, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, [0, 1, 0, 0], word="spread groups: ", spread_groups=[1, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, [0, 1, 0, 0], node_sets=[0] * 4, node_scores=[0] * 4, spread_groups=[0] * 4)
    # every id 0: refused by nothing new (the call gets as far as it does without them)
    for pods in (ds, numa):
        ev.pod_spread_domains([0] * len(pods))
        try:
            ev.schedule(pods, T0)
        except KoordEvalError as e:
            assert "spread domains" not in str(e)


def test_refusals_of_context_state():
    ev = ctx()
    ev.spread_domains_load(np.zeros((1, 8)), [1], [1], [1])
    cl = synth.make_cluster(8, synth.BASE_SEED + 9001)
    synth.load_numa(ev, synth.make_numa(cl, synth.BASE_SEED + 9785, policy_weights=(0.0, 0.4, 0.3, 0.3), no_zone_fraction=0.0))
    assert "NUMA" in _refused(ev, _plain(2), [1, 1])
    ev = Evaluator(synth.config(8, global_node_offset=8))
    synth.load_into(ev, cl)
    ev.spread_domains_load(np.zeros((1, 8)), [1], [1], [1])
    assert "sharded" in _refused(ev, _plain(2), [1, 1])
    for call in (ev.eval, ev.diagnose):
        ev.pod_spread_domains([1, 1])
        assert code_of(call, _plain(2), T0) == abi.ERR_UNSUPPORTED


# ---- the reference of the GPU tests, on the oracle alone -----------------------------------------------------------------
def test_open_domains_is_upstreams_filter():
    cnt = np.zeros(64, np.int64)
    cnt[:4] = [3, 1, 2, 7]
    assert open_domains(0b0111, 1, 0, cnt).nonzero()[0].tolist() == [1]        # min 1: 3+1-1 and 2+1-1 exceed 1
    assert open_domains(0b0111, 2, 0, cnt).nonzero()[0].tolist() == [1, 2]
    assert open_domains(0b1101, 1, 0, cnt).nonzero()[0].tolist() == [2]        # the minimum ranges over `domains` only
    assert open_domains(0b0111, 1, 4, cnt).nonzero()[0].tolist() == []         # fewer than minDomains: min = 0
    assert open_domains(0b0111, 4, 4, cnt).nonzero()[0].tolist() == [0, 1, 2]
    assert open_domains(0b1000, 1, 0, cnt).nonzero()[0].tolist() == [3]        # one domain: its own count is the min


def test_reference_without_ids_is_the_oracles_schedule():
    c = make_input("E")
    ls = Lockstep(fresh_oracle(c), c)
    zero = np.zeros(len(c["pods"]), np.int32)
    got = ls.run(c["pods"], zero, zero, eligibility(c), offsets(c))
    want = fresh_oracle(c).schedule(c["pods"], T0)
    assert np.array_equal(got[0], want[0])
    placed = want[0] >= 0
    assert placed.any() and np.array_equal(got[1][placed], want[1][placed])
    assert np.array_equal(ls.dcounts[1:], c["dcounts"])  # id 0 counts nothing


@pytest.mark.parametrize("name,unplaced", [("E", 0), ("F", 40), ("G", 40), ("H", 0)])
def test_reference_depends_on_the_counts(name, unplaced):
    r = reference(name)
    chosen = r["want"][0]
    print(name, "grouped", int((r["dids"] > 0).sum()), "best filtered", r["best_filtered"], "moved", r["moved"],
          "newly eligible", r["newly"], "unplaced", r["unplaced"])
    assert r["moved"] >= 50 and r["newly"] >= 15
    assert r["unplaced"] >= unplaced if unplaced else r["unplaced"] == 0
    assert r["best_filtered"] >= r["moved"]
    # the counts are the seeds plus the placements, and every placement satisfied the skew bound when it was made
    add = np.zeros_like(r["dcounts"], dtype=np.int64)
    for p in np.nonzero((chosen >= 0) & (r["dids"] > 0))[0]:
        g = r["dids"][p]
        d = r["maps"][r["gmap"][g - 1] - 1, chosen[p]]
        assert d < 64 and (r["dom"][g - 1] >> int(d)) & 1
        add[g - 1, d] += 1
    assert np.array_equal(r["dcounts_after"], r["dcounts"] + add)
    assert r["skew_ok"]
    if name == "H":  # the single-domain group is always open
        assert (chosen[r["dids"] == 1] >= 0).all() and not r["dcounts"].any()
    if name == "G":  # minDomains above the domains there are: at most maxSkew pods a domain
        assert r["dcounts_after"][1].max() <= max(1, r["dcounts"][1].max())


def test_reference_e_with_groups_sets_and_offsets_moves_most_placements():
    r = reference("E", extras=True)
    free = reference_without_domains("E", extras=True)
    differ = int((free[0] != r["want"][0]).sum())
    print("E+ moved", r["moved"], "newly", r["newly"], "unplaced", r["unplaced"], "differ", differ)
    assert differ >= 150 and r["moved"] >= 50 and r["newly"] >= 15
    el = eligibility(r)
    placed = r["want"][0] >= 0
    assert el[np.nonzero(placed)[0], r["want"][0][placed]].all()
    assert not r["counts"].any() and (r["sids"] > 0).any() and (group_ids(r) > 0).all()
    assert (r["counts_after"] <= r["caps"][:, None]).all() and r["counts_after"].any()
