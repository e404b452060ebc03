"""Gang runs with DeviceShare members on the device (ke_set_gang_devices; DESIGN.md §4w, "DeviceShare members"):
ke_schedule / ke_schedule_submit with ke_pod_gangs, bit-exact with the reference of gang_ds_ref.py over the oracle --
placements, scores, statuses, the nodes rolled-back members had, the minors every pod holds -- and after every call the
replay records consistent, the device rows equal to the host's, the host's device cache equal to the oracle's, and the
device's DeviceShare SoA answering probe pods as the oracle's state does.  test_gang_devices_host.py pins on the CPU what
each input contains."""
import numpy as np
import pytest

import gang_ds_ref as D
import gang_ref as G
from koordinator_amd import Evaluator, abi, synth

pytestmark = pytest.mark.gpu
T0 = synth.T0


def evaluator(I, on=True):
    ev = Evaluator(I.cfg)
    I.load_ev(ev)
    ev.set_gang_devices(on)
    return ev


PROBES = D.probe_pods()  # one pod of each kind: together they read every device of a node


def assert_result(ev, got, want, what=""):
    (c, s), (st, tr) = got, ev.last_gang_status()
    for k, v in (("chosen", c), ("score", s), ("status", st), ("tried", tr),
                 ("minors", np.asarray(ev.last_device_allocations, np.uint64))):
        assert np.array_equal(v, want[k]), (what, k, np.argwhere(v != want[k])[:5].ravel().tolist())
    d = ev.debug_gangs()
    assert {k: d[k] for k in want["counts"]} == want["counts"], (what, d)
    return d


def assert_state(ev, I, o):
    assert ev.check_records(T0) == 0
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)
    assert D.device_used(ev, I.n) == D.device_used(o, I.n)  # the host mirror: a rolled-back member was never applied
    # the device's DeviceShare SoA, used-key bits included, word for word against the host's derivation from that mirror
    assert ev.devices_check() == 0
    for i in range(0, I.n, max(1, I.n // 16)):
        assert ev.node_info_requested(i)[0] == o.node_info_requested(i)[0], i
    # ... and as probe pods see it (the nodes are not dirty: nothing is re-derived from the host for this)
    a, b = ev.eval(PROBES, T0), o.eval(PROBES, T0)
    for k in ("status", "reason", "la", "ds", "total", "best"):
        assert np.array_equal(a[k], b[k]), ("probe", k)


def run_input(name):
    I, want, o = D.reference(name)
    ev = evaluator(I)
    d = assert_result(ev, ev.schedule(I.pods, T0, gangs=I.runs), want, name)
    assert d["cuts"] == G.plan_cut(I.P, I.B, I.runs)[1]
    assert_state(ev, I, o)
    # a rolled-back member reads as unplaced: no node, no minors, and its Unreserve is a no-op
    al = ev.last_allocations()
    assert np.array_equal(al["node"], want["chosen"]) and np.array_equal(al["device_minors"], want["minors"])
    for p in np.nonzero(want["status"] == G.ROLLED_BACK)[0][:2]:
        ev.unreserve(I.pods[p], int(p))
    assert_state(ev, I, o)
    inv = sum(1 for _, _, m in want["rollbacks"] if m)
    assert ev.debug_gang_devices()["device_inverses"] == inv, (name, ev.debug_gang_devices())
    return I, ev, want


def test_the_switch_is_off_by_default(gpu):
    I, want, o = D.reference("kind-whole-1")
    ev = Evaluator(I.cfg)
    I.load_ev(ev)
    with pytest.raises(Exception, match="gangs: a DeviceShare member"):
        ev.schedule(I.pods, T0, gangs=I.runs)


@pytest.mark.parametrize("name", [n for n in D.BUILDERS if n.startswith("layout-")])
def test_run_layouts(gpu, name):
    """Clusters of 1, 63, 64, 65 and 300 nodes at batch sizes 7 and 64; runs of 1, 2, B - 1 and B whole-GPU members at
    batch position 0, in mid-batch, where they force the cut rule, and at the call's end."""
    run_input(name)


@pytest.mark.parametrize("name", [n for n in D.BUILDERS if n.startswith("kind-")])
def test_member_kinds(gpu, name):
    """Whole GPUs (1, 2, 8), shared GPUs in both memory forms, GPU + RDMA: a strict run that is rolled back and pods behind
    it that need the freed devices."""
    run_input(name)


@pytest.mark.parametrize("name", ["same-node", "zero-keys", "thresholds", "partition-topology"])
def test_run_rules(gpu, name):
    """Several inverses on one node beside a non-member's allocation on the same minor; used keys present with value 0
    before the run (dropped, as the host path drops them); thresholds, assumed members, need = 0, non-strict and waiting
    runs; partition tables, honor policies and topology scopes beside default nodes."""
    run_input(name)


@pytest.mark.parametrize("name", ["cut-in-run-64", "cut-in-run-7"])
def test_cut_inside_an_open_run(gpu, name):
    """The batch is cut inside an open run, the run goes on in the relaunch from its stored state, and its rollback reaches
    members an earlier launch placed: their nodes are adopted as changed slots."""
    I, ev, want = run_input(name)
    assert want["rollbacks"] and min(p for p, _, _ in want["rollbacks"]) + 2 <= np.nonzero(want["status"] == G.FAILED)[0][0]
    d = ev.debug_gang_devices()
    assert d["cuts_in_run"] > 0 and d["adopted"] > 0 and d["restored"] > 0, d
    assert ev.ds_cuts() >= d["cuts_in_run"]


@pytest.mark.parametrize("name", ["short-list-16-7", "short-list-16-8"])
def test_plain_pod_behind_adopted_nodes_needs_the_longer_list(gpu, name):
    """The launch that begins at the run's failing last member adopts the nodes earlier launches filled; they were the
    plain pod's best snapshot candidates and fall behind an unchanged node, which only the extra list entries of the
    relaunch's select still hold."""
    I, ev, want = run_input(name)
    d = ev.debug_gang_devices()
    assert d["adopted"] >= 2 and d["restored"] > 0, d


def test_mixed_call_keeps_plain_stretches_pipelined(gpu):
    I, ev, want = run_input("mixed")
    assert ev.kernel_stats()["pipelined_batches"] == 10  # five plain batches on either side of the DeviceShare gang batch


def test_mixed_call_as_two_submits_in_flight(gpu):
    """The mixed queue cut in two behind its gang batch, both halves in flight: pipelined plain stretches of two calls
    around the serial DeviceShare gang batch of the first."""
    I, want, o = D.reference("mixed")
    ev = evaluator(I)
    cut = 64 * 7
    t0 = ev.submit(I.pods[:cut], T0, gangs=I.runs)
    t1 = ev.submit(I.pods[cut:], T0)
    for t, (a, b) in ((t0, (0, cut)), (t1, (cut, I.P))):
        part = {k: want[k][a:b] for k in ("chosen", "score", "status", "tried", "minors")}
        part["counts"] = want["counts"] if a == 0 else dict(runs=0, rolled_back=0, inverse_reserves=0)
        assert_result(ev, ev.wait(t), part, f"pods {a}..{b}")
        assert ev.kernel_stats()["pipelined_batches"] >= 4  # the plain stretches of either call stay pipelined
    assert_state(ev, I, o)


def test_two_submits_in_flight(gpu):
    I, want, o = D.reference("slices")
    ev = evaluator(I)
    runs = [[(r[0] - a,) + r[1:] for r in I.runs if a <= r[0] < a + 40] for a in (0, 40)]
    t0 = ev.submit(I.pods[:40], T0, gangs=runs[0])
    t1 = ev.submit(I.pods[40:], T0, gangs=runs[1])
    assert_result(ev, ev.wait(t0), want[0], "first slice")
    assert_result(ev, ev.wait(t1), want[1], "second slice")
    assert_state(ev, I, o)


@pytest.mark.parametrize("name", ["kind-shared-bytes", "zero-keys", "partition-topology", "cut-in-run-64"])
def test_twin_one_call_per_run_with_unreserves(gpu, name):
    """The path without the switch on a second context -- one ke_schedule per run and per plain stretch, ke_unreserve per
    placed member of a failed run -- ends with the same placements, minors, device cache, SoA answers and rows."""
    I, ev, want = run_input(name)
    twin = evaluator(I, on=False)
    chosen, minors = np.full(I.P, -1, np.int32), np.zeros(I.P, np.uint64)
    edges = sorted({0, I.P} | {r[0] for r in I.runs} | {r[0] + r[1] for r in I.runs})
    run_at = {r[0]: r for r in I.runs}
    for a, b in zip(edges[:-1], edges[1:]):
        c, _ = twin.schedule(I.pods[a:b], T0)
        m = np.asarray(twin.last_device_allocations, np.uint64).copy()
        r = run_at.get(a)
        if r is not None:
            need, failed = max(r[2] - r[3], 0), np.nonzero(c < 0)[0]
            if len(failed) and int((c[:failed[0]] >= 0).sum()) < need:  # the run failed before it was satisfied
                drop = range(len(c)) if r[4] == G.STRICT else range(int(failed[0]) + 1, len(c))
                for q in drop:
                    if c[q] >= 0:
                        twin.unreserve(I.pods[a + q], q)
                        c[q], m[q] = -1, 0
        chosen[a:b], minors[a:b] = c, m
    assert np.array_equal(chosen, want["chosen"]) and np.array_equal(minors, want["minors"])
    assert D.device_used(twin, I.n) == D.device_used(ev, I.n)
    twin.schedule(I.pods[:0], T0)  # (an empty call refreshes the rows of the nodes the last Unreserves left dirty)
    assert twin.devices_check() == 0
    (dev, host), (tdev, thost) = ev.debug_rows(T0), twin.debug_rows(T0)
    assert np.array_equal(dev, tdev) and np.array_equal(host, thost)
    assert twin.check_records(T0) == 0
    a, b = twin.eval(PROBES, T0), ev.eval(PROBES, T0)
    for k in ("status", "reason", "ds", "total", "best"):
        assert np.array_equal(a[k], b[k]), k
