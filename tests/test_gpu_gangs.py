"""Gang runs on the device: ke_schedule / ke_schedule_submit with ke_pod_gangs, bit-exact with the
core.go reference of gang_ref.py over the oracle -- placements, scores, statuses, the nodes rolled-back members had --
and after every call the replay records consistent, the device rows equal to the host's, the quota figures equal to the
oracle's and ke_debug_gangs' counters equal to the reference's.  test_gang_host.py pins on the CPU what each input
contains."""
import numpy as np
import pytest

import gang_ref as G
from koordinator_amd import Evaluator, abi, synth

pytestmark = pytest.mark.gpu
T0 = synth.T0


def evaluator(I):
    ev = Evaluator(I.cfg)
    I.load_ev(ev)
    return ev


def assert_result(ev, got, want, what=""):
    (c, s), (st, tr) = got, ev.last_gang_status()
    for k, v in (("chosen", c), ("score", s), ("status", st), ("tried", tr)):
        assert np.array_equal(v, want[k]), (what, k, np.argwhere(v != want[k])[:5].ravel().tolist())
    d = ev.debug_gangs()
    assert {k: d[k] for k in want["counts"]} == want["counts"], (what, d)
    return d


def assert_state(ev, I, o):
    assert ev.check_records(T0) == 0
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)
    if I.quota is not None:
        for i in range(len(I.quota[1])):
            a, b = ev.quota_state(i), o.quota_state(i)
            for k in ("limit", "used", "np_used"):
                assert np.array_equal(a[k], b[k]), (i, k, a[k], b[k])
    # the placements' mirror on the host objects: NodeInfo.Requested of every node as the oracle's
    for i in range(0, I.n, max(1, I.n // 16)):
        assert ev.node_info_requested(i)[0] == o.node_info_requested(i)[0], i


def run_input(name):
    I, want, o = G.reference(name)
    ev = evaluator(I)
    d = assert_result(ev, ev.schedule(I.pods, T0, gangs=I.runs, **I.kw()), want, name)
    assert d["cuts"] == G.plan_cut(I.P, I.B, I.runs)[1]
    assert_state(ev, I, o)
    # a rolled-back member reads as unplaced: no allocation, and its Unreserve is a no-op
    al = ev.last_allocations()
    assert np.array_equal(al["node"], want["chosen"])
    for p in np.nonzero(want["status"] == G.ROLLED_BACK)[0][:2]:
        ev.unreserve(I.pods[p], int(p))
    assert_state(ev, I, o)
    return I, ev, want


@pytest.mark.parametrize("name", [n for n in G.BUILDERS if n.startswith("layout-")])
def test_run_layouts(gpu, name):
    """Clusters of 1, 63, 64, 65 and 300 nodes at batch sizes 7 and 64; runs of 1, 2, B - 1 and B members at batch
    position 0, in mid-batch, where they force the cut, and at the call's end."""
    run_input(name)


@pytest.mark.parametrize("name", ["two-runs-sat-rb", "two-runs-rb-sat", "same-node", "thresholds", "capacity"])
def test_run_rules(gpu, name):
    """Two runs in one batch in both orders (FitPlus profile); several inverse Reserves on one slot beside a plain pod's
    Reserve; thresholds, assumed members, need = 0, non-strict and waiting runs; the global changed-node bitmap."""
    run_input(name)


@pytest.mark.parametrize("name", ["quota-64", "quota-7"])
def test_quota_refusal_rolls_back_and_returns_the_used(gpu, name):
    I, ev, want = run_input(name)
    assert want["chosen"][6] >= 0 and ev.quota_state(1)["used"][0] == 8000


def test_node_sets_and_score_tables_on_members(gpu):
    run_input("sets-scores")


def test_mixed_call_keeps_plain_stretches_pipelined(gpu):
    I, ev, want = run_input("mixed")
    assert ev.kernel_stats()["pipelined_batches"] == 10  # five plain batches on either side of the serial gang batch


def test_two_submits_in_flight_keep_their_own_statuses(gpu):
    I, want, o = G.reference("slices")
    ev = evaluator(I)
    runs = [[(r[0] - a,) + r[1:] for r in I.runs if a <= r[0] < a + 40] for a in (0, 40)]
    t0 = ev.submit(I.pods[:40], T0, gangs=runs[0])
    t1 = ev.submit(I.pods[40:], T0, gangs=runs[1])
    assert_result(ev, ev.wait(t0), want[0], "first slice")
    assert_result(ev, ev.wait(t1), want[1], "second slice")
    assert_state(ev, I, o)


def test_gang_submit_then_plain_submit_in_flight(gpu):
    """A gang slice and a plain slice behind it, both in flight: the plain ticket answers 0 / -1 and zero counters,
    whichever ticket is collected first, and the gang ticket keeps its statuses and counters."""
    I, want, o = G.reference("slices")
    runs = [(r[0],) + r[1:] for r in I.runs if r[0] < 40]
    for order in ((0, 1), (1, 0)):
        ev = evaluator(I)
        t = [ev.submit(I.pods[:40], T0, gangs=runs), ev.submit(I.pods[40:], T0)]
        for k in order:
            c, s = ev.wait(t[k])
            st, tr = ev.last_gang_status()
            if k == 0:
                assert_result(ev, (c, s), want[0], "gang slice")
            else:
                assert not st.any() and (tr == -1).all()
                assert ev.debug_gangs() == dict(runs=0, rolled_back=0, inverse_reserves=0, cuts=0)
                assert (c >= 0).sum() > 30
        assert ev.check_records(T0) == 0


@pytest.mark.parametrize("name", ["layout-300-64", "thresholds", "two-runs-rb-sat"])
def test_twin_one_call_per_run_with_unreserves(gpu, name):
    """Today's path on a second context -- one ke_schedule per run and per plain stretch, ke_unreserve per placed member
    of a failed run -- ends with the same placements and the same rows."""
    I, ev, want = run_input(name)
    twin = evaluator(I)
    chosen = np.full(I.P, -1, np.int32)
    edges = sorted({0, I.P} | {r[0] for r in I.runs} | {r[0] + r[1] for r in I.runs})
    run_at = {r[0]: r for r in I.runs}
    for a, b in zip(edges[:-1], edges[1:]):
        c, _ = twin.schedule(I.pods[a:b], T0)
        r = run_at.get(a)
        if r is not None:
            need, failed = max(r[2] - r[3], 0), np.nonzero(c < 0)[0]
            if len(failed) and int((c[:failed[0]] >= 0).sum()) < need:  # the run failed before it was satisfied
                drop = range(len(c)) if r[4] == G.STRICT else range(int(failed[0]) + 1, len(c))
                for q in drop:
                    if c[q] >= 0:
                        twin.unreserve(I.pods[a + q], q)
                        c[q] = -1
        chosen[a:b] = c
    assert np.array_equal(chosen, want["chosen"])
    twin.schedule(I.pods[:0], T0)  # (an empty call refreshes the rows of the nodes the last Unreserves left dirty)
    (dev, host), (tdev, thost) = ev.debug_rows(T0), twin.debug_rows(T0)
    assert np.array_equal(dev, tdev) and np.array_equal(host, thost)
    assert twin.check_records(T0) == 0
