"""Spread domain terms (ke_pod_spread_domain_terms, ABI v14, additive), host side: the entry point's argument checks
and staging rules, the two both-staged refusals, the refusals a call with lists meets before it needs the device (the
key range among them, summed over both list kinds), and the lock-step reference of the GPU tests
(test_gpu_spread_domain_terms.py) pinned on the oracle alone -- its inputs must make a site that drops a filter term,
reads counts of another moment, takes the bonus from other counts or skips a member move a placement."""
import numpy as np
import pytest

import spread_domains
from koordinator_amd import KoordEvalError, abi, synth
from spread_domain_terms import (AFFINITY, ANTI, FEWER, MORE, SKEW, Y_CAP, Lockstep, affinity_only_reference, eligibility,
                                 fresh_oracle, id_equivalent_reference, make_input, node_terms, offsets, plan, reference)
from spread_domains import D, NONE
from test_node_sets_host import code_of, ctx

T0 = synth.T0


def _ctx(groups=2):
    ev = ctx()
    ev.spread_domains_load(np.zeros((1, 8), np.uint16), [1] * groups, [1] * groups, [1] * groups)
    return ev


def _plain(n, seed=9962):
    return synth.make_pods(n, synth.BASE_SEED + seed)


# ---- the entry point ---------------------------------------------------------------------------------------------------
def test_abi_version_and_the_new_kind(lib):
    assert abi.ABI_VERSION == 14 and lib.ke_abi_version() == 14
    assert abi.TERM_SKEW == 5
    assert abi.STRUCTS[-1] is abi.PodDiagnosis  # no new struct: the entry point takes plain arrays
    assert hasattr(lib, "ke_pod_spread_domain_terms")


def test_argument_checks():
    ev = _ctx(3)
    ok = ev.pod_spread_domain_terms
    ok([[(1, SKEW), (2, AFFINITY, 65535), (3, FEWER, 1, 1), (3, MORE, 2, 100)], [(2, ANTI, 1)]], [[1, 2, 3], []])
    ok([], [])
    ok([[]], [[1, 2, 3]])  # (members alone; three of three groups)
    bad = lambda t, m: code_of(ok, t, m) == abi.ERR_INVALID
    assert bad([[(0, ANTI, 1)]], [[]]) and bad([[(4, ANTI, 1)]], [[]])  # a term's group outside 1..n_groups
    assert bad([[(0, SKEW)]], [[]]) and bad([[(4, SKEW)]], [[]])
    assert bad([[]], [[0]]) and bad([[]], [[4]])  # a member outside
    assert bad([[(1, 0, 1)]], [[]]) and bad([[(1, 6, 1)]], [[]])  # an unknown kind
    assert bad([[(1, SKEW, 1)]], [[]]) and bad([[(1, SKEW, 0, 1)]], [[]])  # SKEW takes neither
    assert bad([[(1, ANTI, 0)]], [[]]) and bad([[(1, ANTI, 65536)]], [[]])  # param
    assert bad([[(1, ANTI, 1, 1)]], [[]]) and bad([[(1, AFFINITY, 1, 5)]], [[]])  # a filter term's weight is 0
    assert bad([[(1, FEWER, 1, 0)]], [[]]) and bad([[(1, MORE, 1, 101)]], [[]])  # a score term's is 1..100
    assert bad([[(1, SKEW)] * 5], [[]])  # more than 4 terms
    assert bad([[]], [[1, 2, 1]])  # a repeated member
    ev5 = _ctx(5)
    assert code_of(ev5.pod_spread_domain_terms, [[]], [[1, 2, 3, 4, 5]]) == abi.ERR_INVALID  # more than 4 members
    ev5.pod_spread_domain_terms([[]], [[1, 2, 3, 4]])
    # the raw arrays: offsets that do not ascend, or do not start at 0; missing arrays
    f = ev.lib.ke_pod_spread_domain_terms
    i32 = lambda *v: np.asarray(v, np.int32)
    t, z = i32(1, SKEW, 0, 0), i32(0, 0, 0)
    assert f(ev.h, 2, abi.ptr(i32(0, 1, 0)), abi.ptr(t), abi.ptr(z), None) == abi.ERR_INVALID
    assert f(ev.h, 2, abi.ptr(i32(1, 1, 1)), abi.ptr(t), abi.ptr(z), None) == abi.ERR_INVALID
    assert f(ev.h, 2, abi.ptr(z), None, abi.ptr(i32(0, 1, 0)), abi.ptr(i32(1))) == abi.ERR_INVALID
    assert f(ev.h, 2, abi.ptr(i32(0, 1, 1)), None, abi.ptr(z), None) == abi.ERR_INVALID
    assert f(ev.h, 2, None, None, abi.ptr(z), None) == abi.ERR_INVALID
    assert f(ev.h, -1, abi.ptr(z), None, abi.ptr(z), None) == abi.ERR_INVALID
    assert f(None, 2, abi.ptr(z), None, abi.ptr(z), None) == abi.ERR_INVALID
    assert f(ev.h, 2, abi.ptr(i32(0, 1, 1)), abi.ptr(t), abi.ptr(z), None) == abi.OK
    # no table loaded: every group is outside (the spread groups' table is another one)
    none = ctx()
    none.spread_groups_load(None, [1, 1], n_nodes=8)
    assert code_of(none.pod_spread_domain_terms, [[(1, SKEW)]], [[]]) == abi.ERR_INVALID
    none.pod_spread_domain_terms([[]], [[]])
    # ke_pod_spread_terms does not take the new kind
    assert code_of(none.pod_spread_terms, [[(1, SKEW, 1)]], [[]]) == abi.ERR_INVALID
    with pytest.raises(ValueError):
        ok([[]], [])  # one list of each kind per pod
    with pytest.raises(ValueError):
        ok([[(1,)]], [[]])  # a term is (group, kind[, param[, weight]])
    with pytest.raises(ValueError):
        none.pod_spread_terms([[(1, ANTI)]], [[]])  # ... and a spread term still has its param


def _no_device(call, *a, **kw):
    """The call gets as far as the device (this context has none): nothing refused it before."""
    with pytest.raises(KoordEvalError) as e:
        call(*a, **kw)
    assert e.value.code == abi.ERR_NO_DEVICE, str(e.value)


def test_staging_and_consumption():
    ev = _ctx()
    pods = _plain(3)
    lists = ([[(1, SKEW)], []], [[1], [2]])
    # a following call with a different n_pods is refused, and the lists are gone afterwards: consumed on failure
    for call in (ev.schedule, ev.eval, ev.diagnose, ev.submit):
        ev.pod_spread_domain_terms(*lists)
        assert code_of(call, pods, T0) == abi.ERR_INVALID, call
        _no_device(call, pods[:2], T0)
    assert code_of(ev.schedule, pods, T0, spread_domain_terms=lists) == abi.ERR_INVALID  # the keyword stages them too
    ds = synth.make_ds_pods(2, synth.BASE_SEED + 9961, device_fraction=1.0)
    ev.pod_spread_domain_terms(*lists)
    assert code_of(ev.schedule, ds, T0) == abi.ERR_UNSUPPORTED
    _no_device(ev.schedule, ds, T0)  # consumed by the refused call
    # lists staged against a table replaced by a smaller one since: a term's group, a member
    for lists2 in (([[(2, ANTI, 1)], [], []], [[], [], []]), ([[], [], []], [[], [2], []])):
        ev.spread_domains_load(np.zeros((1, 8), np.uint16), [1, 1], [1, 1], [1, 1])
        ev.pod_spread_domain_terms(*lists2)
        ev.spread_domains_load(np.zeros((1, 8), np.uint16), [1], [1], [1])
        assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID
    ev.spread_domains_load(np.zeros((1, 8), np.uint16), [1, 1], [1, 1], [1, 1])
    # together with set ids, table ids and §4t lists: all consumed by the one call
    ev.node_sets_load([[0, 1]], n_nodes=8)
    ev.node_scores_load([[1] * 8])
    ev.spread_groups_load(None, [1], n_nodes=8)
    ev.pod_spread_domain_terms(*lists)
    ev.pod_node_sets([1, 1, 1])
    ev.pod_node_scores([1, 1, 1])
    ev.pod_spread_terms([[(1, ANTI, 1)], [], []], [[1], [], []])
    assert code_of(ev.schedule, pods, T0) == abi.ERR_INVALID  # (the domain lists' n_pods)
    _no_device(ev.schedule, pods, T0)
    three = ([[(1, SKEW)], [], [(2, FEWER, 2, 3)]], [[1], [2], []])
    _no_device(ev.schedule, pods, T0, spread_domain_terms=three, node_sets=[1, 1, 1], node_scores=[1, 1, 1],
               spread_terms=([[(1, ANTI, 1)], [], []], [[1], [], []]))  # allowed together


def test_staged_with_group_ids_or_domain_ids_is_invalid():
    ev = _ctx()
    ev.spread_groups_load(None, [1], n_nodes=8)
    pods = _plain(2)
    for call in (ev.schedule, ev.submit, ev.eval, ev.diagnose):
        for stage, form in ((ev.pod_spread_groups, "ANTI"), (ev.pod_spread_domains, "KE_TERM_SKEW")):
            stage([0, 0])  # (also with every id 0 and every list empty: both are staged)
            ev.pod_spread_domain_terms([[], []], [[], []])
            with pytest.raises(KoordEvalError) as e:
                call(pods, T0)
            assert e.value.code == abi.ERR_INVALID and "both" in str(e.value) and form in str(e.value)  # names the list form
            _no_device(call, pods, T0)  # both consumed


# ---- the refusals of a call with a non-empty list (before it needs the device) -------------------------------------------
def _refused(ev, pods, lists, word="spread domain terms: ", **kw):
    for call in (ev.schedule, ev.submit):
        ev.pod_spread_domain_terms(*lists)
        for k, v in kw.items():
            getattr(ev, "pod_" + k)(*v) if k == "spread_terms" else getattr(ev, "pod_" + k)(v)
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
    ds = synth.make_ds_pods(4, synth.BASE_SEED + 9963, device_fraction=1.0)
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
    cpuset = synth.make_cpuset_pods(6, synth.BASE_SEED + 9964, cpuset_fraction=1.0)
    assert "cpuset" in _refused(ev, cpuset, _lists(6))
    # with a non-zero set / table id or a non-empty §4t list in the call the earlier message stays
    ev.node_sets_load([[0, 1, 2]], n_nodes=8)
    ev.node_scores_load([[1] * 8])
    ev.spread_groups_load(None, [1], n_nodes=8)
    assert "DeviceShare" in _refused(ev, ds, _lists(4), word="node sets: ", node_sets=[1, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, _lists(4), word="node scores: ", node_scores=[1, 0, 0, 0])
    assert "DeviceShare" in _refused(ev, ds, _lists(4), word="spread terms: ", spread_terms=_lists(4, 2))
    assert "DeviceShare" in _refused(ev, ds, _lists(4), node_sets=[0] * 4, node_scores=[0] * 4,
                                     spread_terms=([[]] * 4, [[]] * 4))
    # every list empty: refused by nothing new (the call gets as far as it does without them)
    for pods in (ds, numa):
        ev.pod_spread_domain_terms([[]] * len(pods), [[]] * len(pods))
        try:
            ev.schedule(pods, T0)
        except KoordEvalError as e:
            assert "spread domain terms" not in str(e)


def test_refusals_of_context_state():
    from koordinator_amd import Evaluator
    ev = _ctx()
    cl = synth.make_cluster(8, synth.BASE_SEED + 9001)
    synth.load_numa(ev, synth.make_numa(cl, synth.BASE_SEED + 9965, policy_weights=(0.0, 0.4, 0.3, 0.3), no_zone_fraction=0.0))
    assert "NUMA" in _refused(ev, _plain(2), _lists(2))
    ev = Evaluator(synth.config(8, global_node_offset=8))
    synth.load_into(ev, cl)
    ev.spread_domains_load(np.zeros((1, 8), np.uint16), [1], [1], [1])
    assert "sharded" in _refused(ev, _plain(2), _lists(2))
    for call in (ev.eval, ev.diagnose):
        ev.pod_spread_domain_terms(*_lists(2))
        assert code_of(call, _plain(2), T0) == abi.ERR_UNSUPPORTED


def test_key_range_refusal_sums_both_list_kinds():
    ev = _ctx()
    ev.spread_groups_load(None, [1, 1], n_nodes=8)
    pods = _plain(2)
    cfg = synth.config(8)
    cap = 1022 - 100 * (cfg.weight_loadaware + cfg.weight_numa + cfg.weight_deviceshare)
    assert cap == 722
    at = [(1, FEWER, 7, 100), (2, MORE, 22, 1)]  # 700 + 22
    over = [(1, FEWER, 7, 100), (2, MORE, 23, 1)]
    for call in (ev.schedule, ev.submit, ev.eval):
        _no_device(call, pods, T0, spread_domain_terms=([[], at], [[], []]))
        with pytest.raises(KoordEvalError) as e:
            call(pods, T0, spread_domain_terms=([[], over], [[], []]))
        assert e.value.code == abi.ERR_UNSUPPORTED
        msg = str(e.value).split(": ", 1)[1]
        assert msg.startswith("spread domain terms: ") and "723" in msg and "cap 722" in msg, msg
        _no_device(call, pods, T0)  # consumed
    # filter terms do not count, SKEW among them
    _no_device(ev.schedule, pods, T0, spread_domain_terms=([[(1, ANTI, 65535), (2, SKEW)] + at, []], [[], []]))
    # one pod's §4t score terms and its domain score terms count together; two pods' do not
    half = [(1, FEWER, 7, 50)]  # 350
    _no_device(ev.schedule, pods, T0, spread_terms=([half, []], [[], []]), spread_domain_terms=([[(1, MORE, 372, 1)], half], [[], []]))
    with pytest.raises(KoordEvalError) as e:
        ev.schedule(pods, T0, spread_terms=([half, []], [[], []]), spread_domain_terms=([[(1, MORE, 373, 1)], half], [[], []]))
    assert e.value.code == abi.ERR_UNSUPPORTED and "spread domain terms: " in str(e.value) and "723" in str(e.value)
    _no_device(ev.schedule, pods, T0, spread_terms=([half, []], [[], []]), spread_domain_terms=([[], [(1, MORE, 373, 1)]], [[], []]))
    # the largest entry of the loaded score tables counts when the call carries a non-zero table id
    ev.node_scores_load([[0, 3, 0, 0, 0, 0, 0, 0], [1] * 8])
    _no_device(ev.schedule, pods, T0, spread_domain_terms=([[], at], [[], []]), node_scores=[0, 0])
    with pytest.raises(KoordEvalError) as e:
        ev.schedule(pods, T0, spread_domain_terms=([[], at], [[], []]), node_scores=[2, 0])
    assert e.value.code == abi.ERR_UNSUPPORTED and "cap 719" in str(e.value)


# ---- the reference of the GPU tests, on the oracle alone -----------------------------------------------------------------
def test_apply_per_kind_and_the_none_column():
    c = dict(n=5, maps=np.array([[0, 1, 2, 1, NONE]], np.uint16), gmap=[1], dom=[0b111], skew=[1], mind=[0],
             dcounts=np.zeros((1, D), np.uint32), x=None)
    c["dcounts"][0, :3] = [0, 1, 5]
    ls = Lockstep(None, c)
    ok, bonus = ls.apply([(1, ANTI, 2, 0), (1, FEWER, 3, 10), (1, MORE, 2, 7)])
    assert ok.tolist() == [True, True, False, True, True]  # ANTI: a node without the key passes
    assert bonus.tolist() == [30 + 0, 20 + 7, 0 + 14, 20 + 7, 0]  # ... and takes no bonus
    ok, bonus = ls.apply([(1, AFFINITY, 1, 0)])
    assert ok.tolist() == [False, True, True, True, False] and not bonus.any()
    ok, _ = ls.apply([(1, SKEW, 0, 0)])
    assert ok.tolist() == [True, False, False, False, False]  # count + 1 - min <= 1: the emptiest domain alone
    assert ls.apply([])[0].all()


def test_reference_without_lists_is_the_oracles_schedule():
    c = make_input("P")
    ls = Lockstep(fresh_oracle(c), c)
    P = len(c["pods"])
    got = ls.run(c["pods"], [[]] * P, [[]] * P, eligibility(c), offsets(c))
    want = fresh_oracle(c).schedule(c["pods"], T0)
    assert np.array_equal(got[0], want[0])
    placed = want[0] >= 0
    assert placed.any() and np.array_equal(got[1][placed], want[1][placed])
    assert np.array_equal(ls.dcounts[1:], c["dcounts"])  # no member counts nothing


# the committed inputs' statistics: own_window, best_filtered, newly, score_moved, same_node, cell_hits, unplaced,
# max score, batches at 64, the longest
STATS = {"P": (80, 123, 26, 194, 58, 199, 25, 236, 145, 5), "Q": (47, 142, 7, 229, 56, 38, 1, 257, 45, 14),
         "R": (0, 256, 0, 230, 92, 262, 0, 236, 4, 64), "Y": (72, 126, 23, 156, 62, 201, 26, 805, 145, 5)}


@pytest.mark.parametrize("name", sorted(STATS))
def test_reference_depends_on_every_site(name):
    r = reference(name)
    got = (r["own_window"], r["best_filtered"], r["newly"], r["score_moved"], r["same_node"], r["cell_hits"], r["unplaced"],
           r["max_score"], r["batches"], r["longest"])
    print(name, dict(zip(("own_window", "best_filtered", "newly", "score_moved", "same_node", "cell_hits", "unplaced",
                          "max_score", "batches", "longest"), got)), "increments", r["increments"])
    assert got == STATS[name]
    if name == "R":  # read-only and write-only: no cut at batch 64, and the batch's own placements still matter
        assert (r["batches"], r["longest"], r["own_window"]) == (4, 64, 0)
        assert r["same_node"] >= 50 and r["cell_hits"] >= 100 and r["score_moved"] >= 100
    else:
        assert min(r["own_window"], r["best_filtered"], r["score_moved"]) >= 40
        assert r["batches"] > 40
    if name in ("P", "Y"):
        assert r["newly"] >= 16
    chosen = r["want"][0]
    # the counts are the seeds plus every member of every placement, and every placement respects its filter terms
    # against the counts of its moment (replayed here without the oracle)
    ls = Lockstep(None, r)
    for p in range(len(chosen)):
        if chosen[p] < 0:
            continue
        assert ls.apply(r["dterms"][p])[0][chosen[p]], p
        for m in r["dmembers"][p]:
            d = ls.maps[ls.gmap[m], chosen[p]]
            if d < D:
                ls.dcounts[m, d] += 1
    assert np.array_equal(r["dcounts_after"], ls.dcounts[1:])
    assert r["increments"] == int((r["dcounts_after"].astype(np.int64) - r["dcounts"]).sum())
    kinds = {t[1] for tl in r["dterms"] for t in tl}
    assert kinds == ({ANTI, AFFINITY, FEWER, MORE} if name == "R" else {SKEW, ANTI, AFFINITY, FEWER, MORE})
    assert (r["maps"] == NONE).any() and len({int(m) for m in r["gmap"]}) >= 2  # members in different maps
    assert any(len(ml) == 2 and r["gmap"][ml[0] - 1] != r["gmap"][ml[1] - 1] for ml in r["dmembers"])
    if name == "Y":
        el = eligibility(r)
        placed = chosen >= 0
        assert el[np.arange(len(chosen))[placed], chosen[placed]].all() and offsets(r).any()
        assert any(node_terms(r)[0]) and (r["counts_after"] != r["x"]["counts"]).any()
        both = [sum(t[2] * t[3] for t in a if t[1] in (FEWER, MORE)) + sum(t[2] * t[3] for t in b if t[1] in (FEWER, MORE))
                for a, b in zip(r["dterms"], node_terms(r)[0])]
        assert max(both) <= Y_CAP and max(both) > Y_CAP - 8


def test_plan_restated():
    assert plan([[(1,)], [(1,)], [(2,)]], [[1], [], [2]], 64) == [1, 2]
    assert plan([[]] * 5, [[]] * 5, 2) == [2, 2, 1]
    r = make_input("R")
    assert plan(r["dterms"], r["dmembers"], 64) == [64] * 4 and plan(r["dterms"], r["dmembers"], 7) == [7] * 36 + [4]


def test_affinity_only_pods_without_seeds_stay_unplaced():
    r = affinity_only_reference()
    assert r["unplaced"] == len(r["pods"]) and not r["dcounts_after"].any()


@pytest.mark.parametrize("name", ["E", "F", "G", "H"])
def test_domain_ids_are_the_special_case(name):
    c, got, after = id_equivalent_reference(name)
    ref = spread_domains.reference(name)
    assert np.array_equal(got[0], ref["want"][0]) and np.array_equal(got[1], ref["want"][1])
    assert np.array_equal(after, ref["dcounts_after"])
    assert plan(c["dterms"], c["dmembers"], 64) == spread_domains.plan(c["dids"], 64)
