"""Spread terms (ke_pod_spread_terms, ABI v14, additive), host side: the entry point's argument checks and staging
rules, the both-staged refusal, the refusals a call with lists meets before it needs the device (the key range among
them, on both sides of the cap), and the lock-step reference of the GPU tests (test_gpu_spread_terms.py) pinned on the
oracle alone -- its inputs must make a site that drops a filter term, reads a stale count, takes the bonus from other
counts or skips a member move a placement."""
import numpy as np
import pytest

import spread_groups
from koordinator_amd import KoordEvalError, abi, synth
from spread_terms import (AFFINITY, ANTI, FEWER, MORE, Lockstep, affinity_only_reference, apply_terms, domain_ids,
                          eligibility, fresh_oracle, from_groups, make_input, offsets, reference)
from test_node_sets_host import code_of, ctx

T0 = synth.T0


def _ctx(groups=2):
    ev = ctx()
    ev.spread_groups_load(None, [1] * groups, n_nodes=8)
    return ev


def _plain(n, seed=9862):
    return synth.make_pods(n, synth.BASE_SEED + seed)


# ---- the entry point ---------------------------------------------------------------------------------------------------
def test_abi_version_and_limits(lib):
    assert abi.ABI_VERSION == 14 and lib.ke_abi_version() == 14
    assert (abi.MAX_POD_TERMS, abi.MAX_POD_MEMBERS) == (4, 4)
    assert (abi.TERM_ANTI, abi.TERM_AFFINITY, abi.TERM_PREFER_FEWER, abi.TERM_PREFER_MORE) == (1, 2, 3, 4)
    assert abi.STRUCTS[-1] is abi.PodDiagnosis  # no new struct: the entry point takes plain arrays
    assert hasattr(lib, "ke_pod_spread_terms")


def test_argument_checks():
    ev = _ctx(3)
    ok = ev.pod_spread_terms
    ok([[(1, ANTI, 1), (2, AFFINITY, 65535), (3, FEWER, 1, 1), (3, MORE, 2, 100)], []], [[1, 2, 3], []])
    ok([], [])
    ok([[]], [[1, 2, 3]])  # (members alone; three of three groups)
    bad = lambda t, m: code_of(ok, t, m) == abi.ERR_INVALID
    assert bad([[(0, ANTI, 1)]], [[]]) and bad([[(4, ANTI, 1)]], [[]])  # a term's group outside 1..n_groups
    assert bad([[]], [[0]]) and bad([[]], [[4]])  # a member outside
    assert bad([[(1, 0, 1)]], [[]]) and bad([[(1, 5, 1)]], [[]])  # an unknown kind
    assert bad([[(1, ANTI, 0)]], [[]]) and bad([[(1, ANTI, 65536)]], [[]])  # param
    assert bad([[(1, ANTI, 1, 1)]], [[]]) and bad([[(1, AFFINITY, 1, 5)]], [[]])  # a filter term's weight is 0
    assert bad([[(1, FEWER, 1, 0)]], [[]]) and bad([[(1, MORE, 1, 101)]], [[]])  # a score term's is 1..100
    assert bad([[(1, ANTI, 1)] * 5], [[]])  # more than 4 terms
    assert bad([[]], [[1, 2, 1]])  # a repeated member
    ev4 = _ctx(5)
    assert code_of(ev4.pod_spread_terms, [[]], [[1, 2, 3, 4, 5]]) == abi.ERR_INVALID  # more than 4 members
    ev4.pod_spread_terms([[]], [[1, 2, 3, 4]])
    # the raw arrays: offsets that do not ascend, or do not start at 0; missing arrays
    f = ev.lib.ke_pod_spread_terms
    i32 = lambda *v: np.asarray(v, np.int32)
    t, z = i32(1, ANTI, 1, 0), i32(0, 0, 0)
    assert f(ev.h, 2, abi.ptr(i32(0, 1, 0)), abi.ptr(t), abi.ptr(z), None) == abi.ERR_INVALID
    assert f(ev.h, 2, abi.ptr(i32(1, 1, 1)), abi.ptr(t), abi.ptr(z), None) == abi.ERR_INVALID
    assert f(ev.h, 2, abi.ptr(z), None, abi.ptr(i32(0, 1, 0)), abi.ptr(i32(1))) == abi.ERR_INVALID
    assert f(ev.h, 2, abi.ptr(i32(0, 1, 1)), None, abi.ptr(z), None) == abi.ERR_INVALID
    assert f(ev.h, 2, None, None, abi.ptr(z), None) == abi.ERR_INVALID
    assert f(ev.h, -1, abi.ptr(z), None, abi.ptr(z), None) == abi.ERR_INVALID
    assert f(None, 2, abi.ptr(z), None, abi.ptr(z), None) == abi.ERR_INVALID
    assert f(ev.h, 2, abi.ptr(i32(0, 1, 1)), abi.ptr(t), abi.ptr(z), None) == abi.OK
    # no table loaded: every group is outside
    none = ctx()
    assert code_of(none.pod_spread_terms, [[(1, ANTI, 1)]], [[]]) == abi.ERR_INVALID
    none.pod_spread_terms([[]], [[]])
    with pytest.raises(ValueError):
        ok([[]], [])  # one list of each kind per pod


def _no_device(call, *a, **kw):
    """The call gets as far as the device (this context has none): nothing refused it before."""
    with pytest.raises(KoordEvalError) as e:
        call(*a, **kw)
    assert e.value.code == abi.ERR_NO_DEVICE, str(e.value)


def test_staging_and_consumption():
    ev = _ctx()
    pods = _plain(3)
    lists = ([[(1, ANTI, 1)], []], [[1], [2]])
    # a following call with a different n_pods is refused, and the lists are gone afterwards: consumed on failure
    for call in (ev.schedule, ev.eval, ev.diagnose, ev.submit):
        ev.pod_spread_terms(*lists)
        assert code_of(call, pods, T0) == abi.ERR_INVALID, call
        _no_device(call, pods[:2], T0)  # (still staged, a DeviceShare queue below would be refused: see the refusals)
    assert code_of(ev.schedule, pods, T0, spread_terms=lists) == abi.ERR_INVALID  # the keyword stages them too
    ds = synth.make_ds_pods(2, synth.BASE_SEED + 9861, device_fraction=1.0)
    ev.pod_spread_terms(*lists)
    assert code_of(ev.schedule, ds, T0) == abi.ERR_UNSUPPORTED
    _no_device(ev.schedule, ds, T0)  # consumed by the refused call
    # lists staged against a table replaced by a smaller one since: a term's group, a member
    for lists2 in (([[(2, ANTI, 1)], [], []], [[], [], []]), ([[], [], []], [[], [2], []])):
        ev.spread_groups_load(None, [1, 1], n_nodes=8)
        ev.pod_spread_terms(*lists2)
        ev.spread_groups_load(None, [1], n_nodes=8)
        assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID
    ev.spread_groups_load(None, [1, 1], n_nodes=8)
    # together with set ids, table ids and spread domain ids: all consumed by the one call
    ev.node_sets_load([[0, 1]], n_nodes=8)
    ev.node_scores_load([[1] * 8])
    ev.spread_domains_load(np.zeros((1, 8), np.uint16), [1], [1], [1])
    ev.pod_spread_terms(*lists)
    ev.pod_node_sets([1, 1, 1])
    ev.pod_node_scores([1, 1, 1])
    ev.pod_spread_domains([1, 1, 1])
    assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID  # (the lists' n_pods)
    _no_device(ev.schedule, pods, T0)


def test_both_staged_is_invalid():
    ev = _ctx()
    pods = _plain(2)
    for call in (ev.schedule, ev.submit, ev.eval, ev.diagnose):
        ev.pod_spread_groups([0, 0])  # (also with every id 0 and every list empty: both are staged)
        ev.pod_spread_terms([[], []], [[], []])
        with pytest.raises(KoordEvalError) as e:
            call(pods, T0)
        assert e.value.code == abi.ERR_INVALID and "both" in str(e.value)
        _no_device(call, pods, T0)  # both consumed


# ---- the refusals of a call with a non-empty list (before it needs the device) -------------------------------------------
def _refused(ev, pods, lists, word="spread terms: ", **kw):
    for call in (ev.schedule, ev.submit):
        ev.pod_spread_terms(*lists)
        for k, v in kw.items():
            getattr(ev, "pod_" + k)(v)
        with pytest.raises(KoordEvalError) as e:
            call(pods, T0)
        assert e.value.code == abi.ERR_UNSUPPORTED, str(e.value)
        assert str(e.value).split(": ", 1)[1].startswith(word), str(e.value)
    return str(e.value)


def _lists(n, which=1):
    """n pods, pod `which` alone with a list (members only: a list without a term is a list)."""
    return [[] for _ in range(n)], [[1] if p == which else [] for p in range(n)]


def test_schedule_refusals_name_the_condition():
    ev = _ctx()
    ds = synth.make_ds_pods(4, synth.BASE_SEED + 9863, device_fraction=1.0)
    assert "DeviceShare" in _refused(ev, ds, _lists(4))
    numa = _plain(3)
    numa["numa_topology_policy"][1] = abi.NUMA_POLICY_SINGLE_NUMA_NODE
    assert "NUMA" in _refused(ev, numa, _lists(3, 0))
    quota = _plain(3)
    quota["quota"][2] = 1
    assert "ElasticQuota" in _refused(ev, quota, _lists(3, 0))
    for mode in (abi.RSV_MATCHED, abi.RSV_IGNORED, abi.RSV_AFFINITY):
        rsv = _plain(2)
        rsv["reservation_matched"][0] = mode
        assert "reservation" in _refused(ev, rsv, _lists(2))
    cpuset = synth.make_cpuset_pods(6, synth.BASE_SEED + 9864, cpuset_fraction=1.0)
    assert "cpuset" in _refused(ev, cpuset, _lists(6))
    # with a non-zero set / table / domain id in the call the earlier message stays
    ev.node_sets_load([[0, 1, 2]], n_nodes=8)
    ev.node_scores_load([[1] * 8])
    ev.spread_domains_load(np.zeros((1, 8), np.uint16), [1], [1], [1])
    assert "DeviceShare" in _refused(ev, ds, _lists(4), word="node sets: ", node_sets=[1, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, _lists(4), word="node scores: ", node_scores=[1, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, _lists(4), word="spread domains: ", spread_domains=[1, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, _lists(4), node_sets=[0] * 4, node_scores=[0] * 4, spread_domains=[0] * 4)
    # every list empty: refused by nothing new (the call gets as far as it does without them)
    for pods in (ds, numa):
        ev.pod_spread_terms([[]] * len(pods), [[]] * len(pods))
        try:
            ev.schedule(pods, T0)
        except KoordEvalError as e:
            assert "spread terms" not in str(e)


def test_refusals_of_context_state():
    from koordinator_amd import Evaluator
    ev = _ctx()
    cl = synth.make_cluster(8, synth.BASE_SEED + 9001)
    synth.load_numa(ev, synth.make_numa(cl, synth.BASE_SEED + 9865, policy_weights=(0.0, 0.4, 0.3, 0.3), no_zone_fraction=0.0))
    assert "NUMA" in _refused(ev, _plain(2), _lists(2))
    ev = Evaluator(synth.config(8, global_node_offset=8))
    synth.load_into(ev, cl)
    ev.spread_groups_load(None, [1], n_nodes=8)
    assert "sharded" in _refused(ev, _plain(2), _lists(2))
    for call in (ev.eval, ev.diagnose):
        ev.pod_spread_terms(*_lists(2))
        assert code_of(call, _plain(2), T0) == abi.ERR_UNSUPPORTED


def test_key_range_refusal_on_both_sides_of_the_cap():
    ev = _ctx()
    pods = _plain(2)
    cfg = synth.config(8)
    cap = 1022 - 100 * (cfg.weight_loadaware + cfg.weight_numa + cfg.weight_deviceshare)
    assert cap == 722
    at = [(1, FEWER, 7, 100), (2, MORE, 22, 1)]  # 700 + 22
    over = [(1, FEWER, 7, 100), (2, MORE, 23, 1)]
    for call in (ev.schedule, ev.submit, ev.eval):
        _no_device(call, pods, T0, spread_terms=([[], at], [[], []]))
        with pytest.raises(KoordEvalError) as e:
            call(pods, T0, spread_terms=([[], over], [[], []]))
        assert e.value.code == abi.ERR_UNSUPPORTED
        msg = str(e.value).split(": ", 1)[1]
        assert msg.startswith("spread terms: ") and "723" in msg and "cap 722" in msg, msg
        _no_device(call, pods, T0)  # consumed
    # filter terms do not count
    _no_device(ev.schedule, pods, T0, spread_terms=([[(1, ANTI, 65535), (2, AFFINITY, 65535)] + at, []], [[], []]))
    # the largest entry of the loaded score tables counts when the call carries a non-zero table id
    ev.node_scores_load([[0, 3, 0, 0, 0, 0, 0, 0], [1] * 8])
    _no_device(ev.schedule, pods, T0, spread_terms=([[], at], [[], []]), node_scores=[0, 0])
    with pytest.raises(KoordEvalError) as e:
        ev.schedule(pods, T0, spread_terms=([[], at], [[], []]), node_scores=[2, 0])
    assert e.value.code == abi.ERR_UNSUPPORTED and "cap 719" in str(e.value) and "spread terms: " in str(e.value)
    _no_device(ev.schedule, pods, T0, spread_terms=([[], [(1, FEWER, 7, 100), (2, MORE, 19, 1)]], [[], []]), node_scores=[2, 0])


# ---- the reference of the GPU tests, on the oracle alone -----------------------------------------------------------------
def test_apply_terms():
    counts = np.array([[0, 0, 0, 0], [0, 1, 2, 5]], np.int64)
    ok, bonus = apply_terms([(1, ANTI, 2, 0), (1, FEWER, 3, 10), (1, MORE, 2, 7)], counts)
    assert ok.tolist() == [True, True, False, False]
    assert bonus.tolist() == [30 + 0, 20 + 7, 10 + 14, 0 + 14]
    ok, bonus = apply_terms([(1, AFFINITY, 2, 0)], counts)
    assert ok.tolist() == [False, False, True, True] and not bonus.any()


def test_reference_without_lists_is_the_oracles_schedule():
    c = make_input("T")
    ls = Lockstep(fresh_oracle(c), c)
    P = len(c["pods"])
    got = ls.run(c["pods"], [[]] * P, [[]] * P, eligibility(c), offsets(c))
    want = fresh_oracle(c).schedule(c["pods"], T0)
    assert np.array_equal(got[0], want[0])
    placed = want[0] >= 0
    assert placed.any() and np.array_equal(got[1][placed], want[1][placed])
    assert np.array_equal(ls.counts[1:], c["counts"])  # no member counts nothing


# the committed inputs' statistics: (a) own_batch, (b) opened, (c) best_filtered, (d) moved, (e) two_members, max score
STATS = {"T": (66, 21, 97, 226, 68, 231), "U": (68, 17, 103, 214, 84, 227), "V": (107, 21, 132, 234, 71, 216),
         "W": (57, 16, 98, 218, 75, 234), "X": (62, 10, 109, 174, 81, 762)}


@pytest.mark.parametrize("name", sorted(STATS))
def test_reference_depends_on_every_site(name):
    r = reference(name)
    got = (r["own_batch"], r["opened"], r["best_filtered"], r["moved"], r["two_members"], r["max_score"])
    print(name, "own batch", got[0], "opened", got[1], "best filtered", got[2], "moved", got[3], "two members", got[4],
          "max score", got[5], "unplaced", r["unplaced"])
    assert min(got[:5]) >= 8
    assert got == STATS[name]
    assert r["unplaced"] == 0
    chosen = r["want"][0]
    # the counts are the seeds plus every member of every placement, and every placement respects its filter terms
    # against the counts of its moment (replayed here without the oracle)
    cnt = np.concatenate([np.zeros((1, r["n"]), np.int64), r["counts"].astype(np.int64)])
    for p in range(len(chosen)):
        ok, _ = apply_terms(r["terms"][p], cnt)
        assert ok[chosen[p]], p
        for m in r["members"][p]:
            cnt[m, chosen[p]] += 1
    assert np.array_equal(r["counts_after"], cnt[1:])
    kinds = {t[1] for tl in r["terms"] for t in tl}
    assert kinds == {ANTI, AFFINITY, FEWER, MORE}
    assert any(t[1] == ANTI and t[0] not in ml for tl, ml in zip(r["terms"], r["members"]) for t in tl)
    if name == "X":
        el = eligibility(r)
        assert el[np.arange(len(chosen)), chosen].all() and (domain_ids(r) > 0).any() and offsets(r).any()
        assert (r["dcounts_after"].astype(np.int64) - r["dom"]["dcounts"]).sum() == (domain_ids(r) > 0).sum()


def test_affinity_only_pods_without_seeds_stay_unplaced():
    r = affinity_only_reference()
    assert r["unplaced"] == len(r["pods"]) and not r["counts_after"].any()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_groups_are_the_special_case(name):
    g = spread_groups.reference(name)
    terms, members = from_groups(g["gids"], g["caps"])
    c = dict(n=g["n"], cl=g["cl"], pods=g["pods"], counts=g["counts"], dom=None)
    ls = Lockstep(fresh_oracle(c), c)
    got = ls.run(g["pods"], terms, members, spread_groups.eligibility(g), spread_groups.offsets(g))
    assert np.array_equal(got[0], g["want"][0]) and np.array_equal(got[1], g["want"][1])
    assert np.array_equal(ls.counts[1:], g["counts_after"])
