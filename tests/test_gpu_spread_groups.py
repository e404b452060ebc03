"""Spread groups on the device: ke_schedule / submit-ahead against the lock-step reference of
spread_groups.py (pinned on the CPU in test_spread_groups_host.py: its inputs make a site that ignores the cap, or
reads a stale count, move a placement), the counts afterwards on the host and on the device, ke_spread_group_add
between calls, a queue with grouped and plain batches, ke_eval / ke_diagnose with group ids and a refusal.  Every
comparison is exact."""
import numpy as np
import pytest

from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from spread_groups import (Lockstep, eligibility, fresh_oracle, load, make_input, offsets, plain_alloc, reference,
                           slice_kw)
from test_gpu_diagnose import assert_same, reduce_eval
from test_node_sets_host import EVAL_KEYS, sub_oracle

pytestmark = pytest.mark.gpu
T0 = synth.T0


def context(c, batch, pipelined=True):
    ev = Evaluator(synth.config(c["n"], pod_batch=batch))
    synth.load_into(ev, c["cl"])
    kw = load(ev, c)
    ev.set_pipeline(pipelined)
    return ev, kw


def assert_placed(got, want):
    (c1, s1), (c0, s0) = got, want
    assert np.array_equal(c1, c0), np.argwhere(c1 != c0)[:5].ravel().tolist()
    assert np.array_equal(s1, s0), np.argwhere(s1 != s0)[:5].ravel().tolist()


def assert_counts(ev, counts, n):
    """The host copy (ke_spread_groups_get) equals `counts`, the device copy equals the host copy, the records hold."""
    for g in range(len(counts)):
        got = ev.spread_groups_get(g + 1, n)
        assert np.array_equal(got, counts[g]), (g + 1, np.nonzero(got != counts[g])[0][:5].tolist())
    assert ev.debug_spread_groups_check() == 0
    assert ev.check_records(T0) == 0


# ---- ke_schedule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [True, False], ids=["pipelined", "serial"])
@pytest.mark.parametrize("batch", [1, 7, 64])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_schedule_lockstep(gpu, name, batch, pipelined):
    r = reference(name)
    ev, kw = context(r, batch, pipelined)
    got = ev.schedule(r["pods"], T0, **kw)
    assert_placed(got, r["want"])
    assert_counts(ev, r["counts_after"], r["n"])


@pytest.mark.parametrize("batch", [7, 64])
def test_schedule_with_sets_and_offsets(gpu, batch):
    r = reference("D")
    ev, kw = context(r, batch)
    assert set(kw) == {"spread_groups", "node_sets", "node_scores"}
    got = ev.schedule(r["pods"], T0, **kw)
    assert_placed(got, r["want"])
    assert_counts(ev, r["counts_after"], r["n"])


def test_two_calls_on_one_context(gpu):
    r = reference("A")
    ev, kw = context(r, 64)
    a = ev.schedule(r["pods"][:100], T0, **slice_kw(kw, 0, 100))
    mid = np.stack([ev.spread_groups_get(g + 1, r["n"]) for g in range(len(r["caps"]))])
    assert (mid != r["counts"]).any() and (mid != r["counts_after"]).any()
    b = ev.schedule(r["pods"][100:], T0, **slice_kw(kw, 100, None))  # sees the first call's increments
    assert_placed((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), r["want"])
    assert_counts(ev, r["counts_after"], r["n"])


def test_submit_ahead(gpu):
    r = reference("A")
    ev, kw = context(r, 64)
    chosen, score, prev = [], [], None
    for a in range(0, len(r["pods"]), 64):  # four slices, one call kept in flight
        t = ev.submit(r["pods"][a:a + 64], T0, **slice_kw(kw, a, a + 64))
        if prev is not None:
            c, s = ev.wait(prev)
            chosen.append(c), score.append(s)
        prev = t
    c, s = ev.wait(prev)
    chosen.append(c), score.append(s)
    assert len(chosen) == 4
    assert_placed((np.concatenate(chosen), np.concatenate(score)), r["want"])
    assert_counts(ev, r["counts_after"], r["n"])


def test_group_add_between_calls(gpu):
    c = make_input("A")
    ev, kw = context(c, 64)
    ls = Lockstep(fresh_oracle(c), c["counts"], c["caps"])
    elig, off = eligibility(c), offsets(c)
    pods, gids = c["pods"], c["gids"]
    got = ev.schedule(pods, T0, **kw)
    want = ls.run(pods, gids, elig, off)
    assert_placed(got, want)
    # undo three placements of grouped pods: the Unreserve and the caller's -1
    undo = np.nonzero((want[0] >= 0) & (gids > 0))[0][[3, 40, 90]]
    for p in undo:
        node, g = int(want[0][p]), int(gids[p])
        ev.unreserve(pods[p], int(p))
        ev.spread_group_add(g, node, -1)
        ls.o.release(pods[p], plain_alloc(node))
        ls.counts[g, node] -= 1
    assert_counts(ev, ls.counts[1:], c["n"])
    # an informer's pod add on another node, then the three pods again
    ev.spread_group_add(1, 5, 1)
    ls.counts[1, 5] += 1
    again = ev.schedule(pods[undo], T0, spread_groups=gids[undo])
    assert_placed(again, ls.run(pods[undo], gids[undo], elig[undo], off[undo]))
    assert (again[0] >= 0).all()
    assert_counts(ev, ls.counts[1:], c["n"])
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)


def test_mixed_queue_keeps_plain_batches_pipelined(gpu):
    c = make_input("A")
    gids = c["gids"].copy()
    gids[:128] = 0  # two plain batches, then grouped ones
    assert (gids[128:192] > 0).any() and (gids[192:] > 0).any()
    ls = Lockstep(fresh_oracle(c), c["counts"], c["caps"])
    want = ls.run(c["pods"], gids, eligibility(c), offsets(c))
    ev, _ = context(c, 64)
    got = ev.schedule(c["pods"], T0, spread_groups=gids)
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, want)
    assert_counts(ev, ls.counts[1:], c["n"])
    # every id 0 on the same context: the call it is without ids
    more = synth.make_pods(128, synth.BASE_SEED + 9671, key_base=9_600_000_000)
    got = ev.schedule(more, T0, spread_groups=np.zeros(len(more), np.int32))
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, ls.run(more, np.zeros(len(more), np.int32), np.ones((len(more), c["n"]), bool),
                              np.zeros((len(more), c["n"]), np.int64)))
    assert_counts(ev, ls.counts[1:], c["n"])


# ---- ke_eval / ke_diagnose ---------------------------------------------------------------------------------------------
def _ds_context():
    n = 96
    cl = synth.make_cluster(n, synth.BASE_SEED + 9681)
    devs = synth.make_devices(n, synth.BASE_SEED + 9682)
    pods = synth.make_ds_pods(36, synth.BASE_SEED + 9683, device_fraction=0.8)
    ev = Evaluator(synth.config(n))
    synth.load_into(ev, cl)
    synth.load_devices(ev, devs)
    rng = np.random.default_rng(synth.BASE_SEED + 9684)
    counts = rng.integers(0, 3, (3, n)).astype(np.uint16)
    caps = np.array([1, 2, 2], np.uint16)
    gids = 1 + np.arange(len(pods)) % 3  # one group per pod class
    ev.spread_groups_load(counts, caps)
    return n, cl, devs, pods, ev, counts, caps, gids


def test_eval_filters_capped_nodes_and_normalises_over_the_rest(gpu):
    n, cl, devs, pods, ev, counts, caps, gids = _ds_context()
    got = ev.eval(pods, T0, spread_groups=gids)
    assert (got["ds"] > 0).any()
    for g in range(3):
        idx, grp = np.nonzero(counts[g] < caps[g])[0], np.nonzero(gids == g + 1)[0]
        assert 0 < len(idx) < n
        want = sub_oracle(synth.config, cl, idx, devices=devs).eval(pods[grp], T0)
        for k in EVAL_KEYS + ("ds",):  # (DeviceShare's normalisation runs over the uncapped nodes)
            assert np.array_equal(got[k][np.ix_(grp, idx)], want[k]), (g, k)
        wb = np.where(want["best"] >= 0, idx[np.maximum(want["best"], 0)], -1)
        assert np.array_equal(got["best"][grp], wb), g
        out = np.setdiff1d(np.arange(n), idx)
        assert (got["status"][np.ix_(grp, out)] == abi.CODE_UNSCHEDULABLE_AND_UNRESOLVABLE).all()
        assert (got["reason"][np.ix_(grp, out)] == abi.REASON_NODE_SET).all()
        for k in ("la", "numa", "ds"):
            assert (got[k][np.ix_(grp, out)] == 0).all(), k
        assert (got["total"][np.ix_(grp, out)] == -1).all()
    # ke_eval changes nothing, and the ids were consumed: the next call is the plain one
    for g in range(3):
        assert np.array_equal(ev.spread_groups_get(g + 1, n), counts[g])
    assert ev.debug_spread_groups_check() == 0
    plain = ev.eval(pods, T0)
    assert not (plain["reason"] == abi.REASON_NODE_SET).any()
    # groups together with a node set: a pair outside either reports the same way
    sets = np.random.default_rng(synth.BASE_SEED + 9685).random((1, n)) < 0.5
    ev.node_sets_load(sets)
    both = ev.eval(pods, T0, node_sets=np.ones(len(pods), np.int32), spread_groups=gids)
    open_ = sets[0][None, :] & (counts[gids - 1] < caps[gids - 1][:, None])
    assert np.array_equal(both["reason"] == abi.REASON_NODE_SET, ~open_)
    assert (both["total"][~open_] == -1).all() and (both["total"][open_] >= 0).any()


def test_diagnose_counts_capped_pairs_under_node_set(gpu):
    n, cl, devs, pods, ev, counts, caps, gids = _ds_context()
    capped = counts[gids - 1] >= caps[gids - 1][:, None]
    got = ev.diagnose(pods, T0, spread_groups=gids, bitmaps=True)
    assert np.array_equal(got["reason_nodes"][:, abi.REASON_NODE_SET], capped.sum(1))
    assert (got["plugins"][capped.any(1)] & abi.PLUGIN_NODE_SET).all()
    dev = ev.eval(pods, T0, spread_groups=gids)
    assert_same(got, reduce_eval(dev["status"], dev["reason"]), "vs ke_eval")
    assert np.array_equal(got["unresolvable"] & capped, capped)
    for g in range(3):  # ke_diagnose changes nothing
        assert np.array_equal(ev.spread_groups_get(g + 1, n), counts[g])
    assert ev.debug_spread_groups_check() == 0


# ---- a refusal -----------------------------------------------------------------------------------------------------------
def test_refused_deviceshare_pod_leaves_the_context_untouched(gpu):
    n = 120
    cl = synth.make_cluster(n, synth.BASE_SEED + 9691)
    devs = synth.make_devices(n, synth.BASE_SEED + 9692)
    ev, fresh = Evaluator(synth.config(n)), Evaluator(synth.config(n))
    for h in (ev, fresh):
        synth.load_into(h, cl)
        synth.load_devices(h, devs)
    ev.spread_groups_load(None, [1, 1])
    pods = synth.make_ds_pods(8, synth.BASE_SEED + 9693, device_fraction=1.0)
    with pytest.raises(KoordEvalError) as e:
        ev.schedule(pods, T0, spread_groups=[1] * 8)
    assert e.value.code == abi.ERR_UNSUPPORTED and "spread groups: " in str(e.value) and "DeviceShare" in str(e.value)
    assert not ev.spread_groups_get(1, n).any() and ev.debug_spread_groups_check() == 0
    plain = synth.make_pods(200, synth.BASE_SEED + 9694)
    got, want = ev.schedule(plain, T0), fresh.schedule(plain, T0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] >= 0).any()
