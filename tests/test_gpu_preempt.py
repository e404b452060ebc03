"""ke_preempt on the device: every ke_preemption field, the victim list and the candidate bitmap equal, exactly, the
plain-Python restatement of elasticquota/preempt.go in preempt_ref.py -- over the node / preemptor / resident-count
boundaries of the mapping (one wave per node, lane = resident, 8 preemptors a group), quota trees, node sets, deleted
slots, a profile without NodeResourcesFit's Filter, a saturated queue, table changes between calls, and without side
effects.  tests/test_preempt_host.py asserts on the reference alone that each input is worth running."""
import numpy as np
import pytest

import preempt_ref as R
from koordinator_amd import Evaluator, abi, synth
from koordinator_amd.evaluator import unpack_node_sets
from oracle.binding import Oracle

pytestmark = pytest.mark.gpu
T0 = synth.T0


def evaluator(sc, residents=True):
    ev = Evaluator(sc.cfg)
    sc.load(ev)
    if sc.sets is not None:
        ev.node_sets_load(sc.sets)
    if residents:
        ev.resident_pods_load(sc.residents)
        ev.pdbs_load(sc.pdbs)
    return ev


def run(ev, sc, pods=None, priorities=None, cap=abi.MAX_RESIDENT_PODS, **kw):
    pods = sc.pods if pods is None else pods
    return ev.preempt(pods, sc.priorities if priorities is None else priorities, T0, args=sc.args(), victims_cap=cap,
                      candidates=True, node_sets=sc.ids if pods is sc.pods else None, **kw)


def check(sc, what, cap=abi.MAX_RESIDENT_PODS, **kw):
    ev = evaluator(sc)
    o, twin = sc.oracles()
    want = R.preempt_ref(sc.input(o, twin))
    got = run(ev, sc, cap=cap, **kw)
    R.assert_same(got, want, cap, what)
    populated = sc.n - len(sc.deleted)
    assert (sum(got[k] for k in R.COUNTS) == populated).all()
    return ev, got, want


# ---- 1 shapes: the wave / block / group boundaries, words_per_pod exact and larger -------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 333])
def test_shapes(gpu, n):
    sc = R.scenario(n, n, 9, sets=n >= 63)
    ev = evaluator(sc)
    o, twin = sc.oracles()
    want_all = R.preempt_ref(sc.input(o, twin))
    for P in (1, 8, 9):
        want = {k: (v[:P] if k != "detail" else v) for k, v in want_all.items()}
        for extra in (0, 3):
            if sc.ids is not None:
                ev.pod_node_sets(sc.ids[:P])
            got = ev.preempt(sc.pods[:P], sc.priorities[:P], T0, args=sc.args(), candidates=True, extra_words=extra)
            R.assert_same(got, want, abi.MAX_RESIDENT_PODS, f"n={n} P={P} extra={extra}")
            wpp = (n + 63) // 64
            w = got["candidate_words"]
            assert w.shape == (P, wpp + extra) and (w[:, wpp:] == 0).all()
            assert (unpack_node_sets(w[:, :wpp], wpp * 64)[:, n:] == 0).all()  # the tail bits


# ---- 2 residents per node: the lane boundary of the mapping (two entries a lane) --------------------------------------
def test_resident_counts(gpu):
    sc = R.scenario(100, 20, 9, counts=R.LANE_COUNTS, quota=True)
    _, got, want = check(sc, "resident counts")
    assert want["n_candidates"].sum() > 0


# ---- 2b Requested below the listed pods' requests: every removal ends at 0 (RemovePod does not go negative) ----------
def test_requested_below_the_listed_requests(gpu):
    sc = R.scenario(120, 95, 9, understated=True)
    _, got, want = check(sc, "understated")
    assert (want["n_victims"] > 0).any()


# ---- 3 victims_cap 1 and smaller than n_victims ------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 2])
def test_victims_cap(gpu, cap):
    sc = R.scenario(100, 20, 9, counts=R.LANE_COUNTS, quota=True)
    _, got, want = check(sc, f"cap {cap}", cap=cap)
    assert (want["n_victims"] > cap).any()  # (the list is cut: n_victims still counts them all)


# ---- 4 quota tree (half the leaves at their used limit), a preemptor of quota 0, default-quota preemption on / off -----
@pytest.mark.parametrize("disable", [0, 1])
def test_quota(gpu, disable):
    sc = R.scenario(333, 1, 9, quota=True, sets=True, disable_default=disable, quota0=True)
    _, got, want = check(sc, f"quota disable={disable}")
    assert want["n_error"].sum() > 0 and want["n_candidates"].sum() > 0


# ---- 5 deleted node slots, capacity above the populated range ----------------------------------------------------------
def test_deleted_nodes(gpu):
    gone = [0, 63, 64, 130, 199]
    sc = R.scenario(200, 40, 9, deleted=gone, capacity=320, sets=True)
    ev, got, want = check(sc, "deleted")
    assert not got["candidates"][:, gone].any()
    # ke_node_delete drops the node's list, and the next call sees the table without it
    assert len(ev.resident_pods_get(7)) == len(sc.residents[7]) > 0
    ev.delete_node(7)
    assert len(ev.resident_pods_get(7)) == 0
    sc.deleted = tuple(gone) + (7,)
    o, twin = sc.oracles()
    R.assert_same(run(ev, sc), R.preempt_ref(sc.input(o, twin)), abi.MAX_RESIDENT_PODS, "one more deleted")


# ---- 6 a profile without NodeResourcesFit's Filter ---------------------------------------------------------------------
def test_without_fit_filter(gpu):
    sc = R.scenario(150, 50, 9, fit=False, quota=True)
    _, got, want = check(sc, "no fit filter")
    assert want["n_candidates"].sum() > 0


# ---- 7 the pick: each criterion decides one pod's pick ------------------------------------------------------------------
def test_pick_criteria(gpu):
    sc = R.pick_scenario()
    _, got, want = check(sc, "pick")
    assert got["node"].tolist() == [1, 3, 5, 7, 9, 10]


# ---- 8 after a saturated queue: pods that fit nowhere, LoadAware-failing nodes in n_unfit ------------------------------
def test_after_a_saturated_queue(gpu):
    sc = R.scenario(40, 60, 9)
    sc.cl.nodes = synth.make_cluster(40, R.S + 100 * 60 + 1).nodes  # (the plain cluster's own NodeInfo: the queue fills it)
    sc.tables = synth.make_node_resources(sc.cl, R.S + 62)
    queue = R.plain_pods(1500, R.S + 61)
    ev = evaluator(sc)
    o, twin = sc.oracles()
    c1, c0 = ev.schedule(queue, T0)[0], o.schedule(queue, T0)[0]
    assert np.array_equal(c1, c0) and (c0 < 0).sum() > 100
    R.replay(twin, o, queue, c0)
    pending = queue[c0 < 0][:9]
    pri = np.full(9, 10000, np.int32)
    want = R.preempt_ref(sc.input(o, twin, pods=pending, priorities=pri))
    got = run(ev, sc, pods=pending, priorities=pri)
    R.assert_same(got, want, abi.MAX_RESIDENT_PODS, "saturated")
    assert want["n_unfit"].sum() > 0 and want["n_candidates"].sum() > 0


# ---- 9 table changes between two calls ----------------------------------------------------------------------------------
def test_table_changes(gpu):
    sc = R.scenario(130, 70, 9, quota=True)
    ev, got, want = check(sc, "before")
    p = int(np.argmax(want["n_victims"]))
    node, uid = int(want["node"][p]), want["victims"][p][0]
    ev.resident_pod_remove(node, uid)
    gone = [r for r in sc.residents[node] if int(r["uid"]) == uid][0]
    sc.residents[node] = [r for r in sc.residents[node] if int(r["uid"]) != uid]
    extra = R.resident(77, 1, T0, 500, synth.GI, quota=int(sc.pods["quota"][p]))
    ev.resident_pod_add(node, extra)
    sc.residents[node].append(extra)
    o, twin = sc.oracles()
    want2 = R.preempt_ref(sc.input(o, twin))
    R.assert_same(run(ev, sc), want2, abi.MAX_RESIDENT_PODS, "after remove / add")
    assert uid not in want2["victims"][p] and gone is not None
    # a load that shrinks the table
    sc.residents = [lst[:3] for lst in sc.residents[:60]] + [[] for _ in range(sc.n - 60)]
    ev.resident_pods_load(sc.residents[:60])
    want3 = R.preempt_ref(sc.input(o, twin))
    R.assert_same(run(ev, sc), want3, abi.MAX_RESIDENT_PODS, "after a smaller load")


# ---- 10 no side effects -------------------------------------------------------------------------------------------------
def test_no_side_effects(gpu):
    sc = R.scenario(300, 80, 9, quota=True)
    ev = evaluator(sc)
    ev.diagnose(sc.pods, T0)  # (the first call uploads the rows)
    rows0 = ev.debug_rows(T0)[0].copy()
    assert rows0["flags"].any()
    quota0 = [ev.quota_state(q) for q in range(len(sc.quota_arr))]
    res0 = [ev.resident_pods_get(i) for i in range(sc.n)]
    run(ev, sc)
    run(ev, sc, cap=1)
    assert np.array_equal(ev.debug_rows(T0)[0], rows0)
    for q, st in enumerate(quota0):
        now = ev.quota_state(q)
        assert all(np.array_equal(st[k], now[k]) for k in st)
    assert all(np.array_equal(a, ev.resident_pods_get(i)) for i, a in enumerate(res0))
    assert ev.check_records(T0) == 0


def test_between_submit_and_wait(gpu):
    """A ke_preempt between ke_schedule_submit and ke_schedule_wait completes the call in flight, sees its Reserves,
    and leaves its placements equal to the oracle's."""
    n = 200
    cl = synth.make_cluster(n, R.S + 9001)
    cfg = synth.config(n)
    ev, o = Evaluator(cfg), Oracle(cfg, n)
    twin = R.twin_of(cfg, n)
    for h in (ev, o, twin):
        synth.load_into(h, cl)
    residents = R.make_residents(cl, R.S + 9002)
    ev.resident_pods_load(residents)
    ev.pdbs_load([1] * 6)
    queue = synth.make_pods(150, R.S + 9003)
    probe, pri = R.plain_pods(9, R.S + 9004), np.full(9, 6000, np.int32)
    t = ev.submit(queue, T0)
    mid = ev.preempt(probe, pri, T0, candidates=True)
    got = ev.wait(t)
    want = o.schedule(queue, T0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    R.replay(twin, o, queue, want[0])
    inp = R.Input(o, twin, False, probe, pri, residents, [1] * 6)
    R.assert_same(mid, R.preempt_ref(inp), abi.MAX_RESIDENT_PODS, "in flight")
    assert ev.check_records(T0) == 0


# ---- 11 end to end, once: evict the reported victims, then ke_schedule places the preemptor on the picked node ----------
def test_end_to_end(gpu):
    sc = R.scenario(60, 90, 9)
    ev, got, want = check(sc, "e2e before")
    o, _ = sc.oracles()
    room = sc.cl.nodes["allowed_pods"] > sc.cl.nodes["pod_count"]  # (the eviction below frees Requested, not a pod slot)
    fit_driven = [p for p in range(9) if got["node"][p] >= 0 and got["n_victims"][p] > 0 and room[got["node"][p]]
                  and not any(d["fits_as_is"] for d in want["detail"][p]["nodes"].values())]
    assert fit_driven
    p = fit_driven[0]
    node = int(got["node"][p])
    victims = [r for r in sc.residents[node] if int(r["uid"]) in set(got["victims"][p][:got["n_victims"][p]].tolist())]
    assert len(victims) == got["n_victims"][p]
    cpu = int(sc.cl.nodes["requested"][node, 0]) - sum(int(v["requests"][0]) for v in victims)
    mem = int(sc.cl.nodes["requested"][node, 1]) - sum(int(v["requests"][1]) for v in victims)
    for h in (ev, o):  # the eviction: what NodeInfo.RemovePod leaves of Requested
        h.set_requested(node, cpu, mem)
    for v in victims:
        ev.resident_pod_remove(node, int(v["uid"]))
    c1, c0 = ev.schedule(sc.pods[p:p + 1], T0)[0], o.schedule(sc.pods[p:p + 1], T0)[0]
    assert c1[0] == c0[0] == node
