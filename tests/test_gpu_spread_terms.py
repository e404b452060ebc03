"""Spread terms on the device: ke_schedule / submit-ahead against the lock-step reference of
spread_terms.py (pinned on the CPU in test_spread_terms_host.py: its inputs make a site that drops a filter term, reads
a stale count, takes the bonus from other counts or skips a member move a placement), the counts afterwards on the host
and on the device, ke_spread_group_add undos between calls, a queue with listed and plain batches, the §4r
equivalence, ke_eval / ke_diagnose with lists, scores on both sides of 511, saturation and a refusal.  Every comparison
is exact."""
import numpy as np
import pytest

import spread_groups
from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from landscapes import flat_cluster, ls_pods
from spread_terms import (AFFINITY, ANTI, FEWER, MORE, Lockstep, apply_terms, eligibility, fresh_oracle,
                          from_groups, load, make_input, offsets, plain_alloc, reference, slice_kw)
from test_gpu_diagnose import assert_same, reduce_eval
from test_node_sets_host import masked_argmax, sub_oracle

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
@pytest.mark.parametrize("name", ["T", "U", "V", "W"])
def test_schedule_lockstep(gpu, name, batch, pipelined):
    r = reference(name)
    ev, kw = context(r, batch, pipelined)
    got = ev.schedule(r["pods"], T0, **kw)
    assert_placed(got, r["want"])
    assert_counts(ev, r["counts_after"], r["n"])


@pytest.mark.parametrize("batch", [7, 64])
def test_schedule_with_sets_offsets_and_domains(gpu, batch):
    r = reference("X")
    ev, kw = context(r, batch)
    assert set(kw) == {"spread_terms", "spread_domains", "node_sets", "node_scores"}
    got = ev.schedule(r["pods"], T0, **kw)
    assert_placed(got, r["want"])
    assert_counts(ev, r["counts_after"], r["n"])
    for g in range(len(r["dcounts_after"])):
        assert np.array_equal(ev.spread_domains_get(g + 1), r["dcounts_after"][g]), g + 1
    assert ev.debug_spread_domains_check() == 0


def test_two_calls_on_one_context(gpu):
    r = reference("T")
    ev, kw = context(r, 64)
    a = ev.schedule(r["pods"][:100], T0, **slice_kw(kw, 0, 100))
    mid = np.stack([ev.spread_groups_get(g + 1, r["n"]) for g in range(r["G"])])
    assert (mid != r["counts"]).any() and (mid != r["counts_after"]).any()
    b = ev.schedule(r["pods"][100:], T0, **slice_kw(kw, 100, None))  # sees the first call's increments
    assert_placed((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), r["want"])
    assert_counts(ev, r["counts_after"], r["n"])


def test_submit_ahead(gpu):
    r = reference("U")
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


def test_group_add_undos_between_calls(gpu):
    c = make_input("T")
    ev, kw = context(c, 64)
    ls = Lockstep(fresh_oracle(c), c)
    elig, off = eligibility(c), offsets(c)
    pods, terms, members = c["pods"], c["terms"], c["members"]
    got = ev.schedule(pods, T0, **kw)
    want = ls.run(pods, terms, members, elig, off)
    assert_placed(got, want)
    # undo three placements, one of a pod with two members: the Unreserve and the caller's -1 per member
    two = [p for p in range(len(pods)) if len(members[p]) == 2][5]
    undo = np.array([3, two, 200])
    for p in undo:
        node = int(want[0][p])
        ev.unreserve(pods[p], int(p))
        ls.o.release(pods[p], plain_alloc(node))
        for m in members[p]:
            ev.spread_group_add(m, node, -1)
            ls.counts[m, node] -= 1
    assert_counts(ev, ls.counts[1:], c["n"])
    # an informer's pod add on another node, then the three pods again
    ev.spread_group_add(1, 5, 1)
    ls.counts[1, 5] += 1
    sub = ([terms[p] for p in undo], [members[p] for p in undo])
    again = ev.schedule(pods[undo], T0, spread_terms=sub)
    assert_placed(again, ls.run(pods[undo], sub[0], sub[1], elig[undo], off[undo]))
    assert_counts(ev, ls.counts[1:], c["n"])
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)


def test_mixed_queue_keeps_plain_batches_pipelined(gpu):
    c = make_input("T")
    P = len(c["pods"])
    terms = [[] if p < 128 else c["terms"][p] for p in range(P)]  # two plain batches, then listed ones
    members = [[] if p < 128 else c["members"][p] for p in range(P)]
    ls = Lockstep(fresh_oracle(c), c)
    want = ls.run(c["pods"], terms, members, eligibility(c), offsets(c))
    ev, _ = context(c, 64)
    got = ev.schedule(c["pods"], T0, spread_terms=(terms, members))
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, want)
    assert_counts(ev, ls.counts[1:], c["n"])
    # every list empty on the same context: the call it is without lists
    more = synth.make_pods(128, synth.BASE_SEED + 9871, key_base=9_800_000_000)
    got = ev.schedule(more, T0, spread_terms=([[]] * len(more), [[]] * len(more)))
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, ls.run(more, [[]] * len(more), [[]] * len(more), np.ones((len(more), c["n"]), bool),
                              np.zeros((len(more), c["n"]), np.int64)))
    assert_counts(ev, ls.counts[1:], c["n"])


@pytest.mark.parametrize("name", ["A", "D"])
def test_groups_are_the_special_case(gpu, name):
    g = spread_groups.reference(name)
    ev = Evaluator(synth.config(g["n"], pod_batch=64))
    synth.load_into(ev, g["cl"])
    kw = spread_groups.load(ev, g)
    del kw["spread_groups"]
    got = ev.schedule(g["pods"], T0, spread_terms=from_groups(g["gids"], g["caps"]), **kw)
    assert_placed(got, g["want"])
    assert_counts(ev, g["counts_after"], g["n"])


# ---- ke_eval / ke_diagnose ---------------------------------------------------------------------------------------------
CLASSES = ([(1, ANTI, 1, 0), (2, FEWER, 3, 10)], [(2, AFFINITY, 1, 0), (3, MORE, 2, 7)],
           [(3, ANTI, 2, 0), (1, AFFINITY, 1, 0), (1, MORE, 2, 5), (2, FEWER, 2, 9)])


def _ds_context():
    n = 96
    cl = synth.make_cluster(n, synth.BASE_SEED + 9881)
    devs = synth.make_devices(n, synth.BASE_SEED + 9882)
    pods = synth.make_ds_pods(36, synth.BASE_SEED + 9883, device_fraction=0.8)
    ev = Evaluator(synth.config(n))
    synth.load_into(ev, cl)
    synth.load_devices(ev, devs)
    rng = np.random.default_rng(synth.BASE_SEED + 9884)
    counts = rng.integers(0, 3, (3, n)).astype(np.uint16)
    cls = np.arange(len(pods)) % 3  # one term list per pod class
    ev.spread_groups_load(counts, [1, 1, 1])
    lists = ([CLASSES[k] for k in cls], [[1 + int(k)] for k in cls])
    return n, cl, devs, pods, ev, counts, cls, lists


def test_eval_applies_filter_terms_and_adds_the_bonus_behind_the_normalisation(gpu):
    n, cl, devs, pods, ev, counts, cls, lists = _ds_context()
    got = ev.eval(pods, T0, spread_terms=lists)
    assert (got["ds"] > 0).any()
    full = np.concatenate([np.zeros((1, n), np.int64), counts.astype(np.int64)])
    for k in range(3):
        ok, bonus = apply_terms(CLASSES[k], full)
        idx, grp = np.nonzero(ok)[0], np.nonzero(cls == k)[0]
        assert 0 < len(idx) < n and bonus[idx].any()
        want = sub_oracle(synth.config, cl, idx, devices=devs).eval(pods[grp], T0)
        for key in ("status", "reason", "la", "numa", "ds"):  # (DeviceShare's normalisation runs over the open nodes)
            assert np.array_equal(got[key][np.ix_(grp, idx)], want[key]), (k, key)
        wt = np.where(want["total"] >= 0, want["total"] + bonus[idx][None, :], -1)
        assert np.array_equal(got["total"][np.ix_(grp, idx)], wt), k
        assert (want["total"] >= 0).any()
        wb = np.array([masked_argmax(t, np.ones(len(idx), bool))[0] for t in wt])
        assert np.array_equal(got["best"][grp], np.where(wb >= 0, idx[np.maximum(wb, 0)], -1)), k
        out = np.setdiff1d(np.arange(n), idx)
        assert (got["status"][np.ix_(grp, out)] == abi.CODE_UNSCHEDULABLE_AND_UNRESOLVABLE).all()
        assert (got["reason"][np.ix_(grp, out)] == abi.REASON_NODE_SET).all()
        for key in ("la", "numa", "ds"):
            assert (got[key][np.ix_(grp, out)] == 0).all(), key
        assert (got["total"][np.ix_(grp, out)] == -1).all()
    # ke_eval changes nothing, and the lists were consumed: the next call is the plain one
    for g in range(3):
        assert np.array_equal(ev.spread_groups_get(g + 1, n), counts[g])
    assert ev.debug_spread_groups_check() == 0
    plain = ev.eval(pods, T0)
    assert not (plain["reason"] == abi.REASON_NODE_SET).any()
    # lists together with a node set: a pair outside either reports the same way
    sets = np.random.default_rng(synth.BASE_SEED + 9885).random((1, n)) < 0.5
    ev.node_sets_load(sets)
    both = ev.eval(pods, T0, node_sets=np.ones(len(pods), np.int32), spread_terms=lists)
    open_ = sets[0][None, :] & np.stack([apply_terms(CLASSES[k], full)[0] for k in cls])
    assert np.array_equal(both["reason"] == abi.REASON_NODE_SET, ~open_)
    assert (both["total"][~open_] == -1).all() and (both["total"][open_] >= 0).any()


def test_diagnose_counts_filtered_pairs_under_node_set(gpu):
    n, cl, devs, pods, ev, counts, cls, lists = _ds_context()
    full = np.concatenate([np.zeros((1, n), np.int64), counts.astype(np.int64)])
    closed = ~np.stack([apply_terms(CLASSES[k], full)[0] for k in cls])
    got = ev.diagnose(pods, T0, spread_terms=lists, bitmaps=True)
    assert np.array_equal(got["reason_nodes"][:, abi.REASON_NODE_SET], closed.sum(1))
    assert (got["plugins"][closed.any(1)] & abi.PLUGIN_NODE_SET).all()
    dev = ev.eval(pods, T0, spread_terms=lists)
    assert_same(got, reduce_eval(dev["status"], dev["reason"]), "vs ke_eval")
    assert np.array_equal(got["unresolvable"] & closed, closed)
    # the score kinds alone filter nothing
    soft = ([[t for t in tl if t[1] in (FEWER, MORE)] for tl in lists[0]], lists[1])
    assert not ev.diagnose(pods, T0, spread_terms=soft)["reason_nodes"][:, abi.REASON_NODE_SET].any()
    for g in range(3):  # ke_diagnose changes nothing
        assert np.array_equal(ev.spread_groups_get(g + 1, n), counts[g])
    assert ev.debug_spread_groups_check() == 0


# ---- the edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [7, 64])
def test_scores_on_both_sides_of_511_in_one_select(gpu, batch):
    n, P = 333, 128
    cl = flat_cluster(n)
    pods = ls_pods(P, synth.BASE_SEED + 9891)
    rng = np.random.default_rng(synth.BASE_SEED + 9892)
    counts = rng.integers(0, 8, (1, n)).astype(np.uint16)
    counts[0, rng.random(n) < 0.9] = 7  # few nodes above the rest: they fill up, and the pods move down the levels
    c = dict(n=n, cl=cl, pods=pods, G=1, counts=counts, terms=[[(1, FEWER, 7, 100)]] * P, members=[[1]] * P, dom=None)
    ls = Lockstep(fresh_oracle(c), c)
    want = ls.run(pods, c["terms"], c["members"], eligibility(c), offsets(c))
    assert want[1].max() > 700 and (want[1] > 511).sum() >= 8 and (want[1] < 511).sum() >= 8 and (want[0] >= 0).all()
    ev, kw = context(c, batch)
    assert_placed(ev.schedule(pods, T0, **kw), want)
    assert_counts(ev, ls.counts[1:], n)


def test_member_counts_saturate_on_host_and_device(gpu):
    n = 130
    cl = flat_cluster(n)  # (every pod below fits node 17 four times over)
    pods = ls_pods(4, synth.BASE_SEED + 9897)
    counts = np.zeros((2, n), np.uint16)
    counts[0, 17] = 65534
    ev = Evaluator(synth.config(n, pod_batch=64))
    synth.load_into(ev, cl)
    ev.spread_groups_load(counts, [1, 1])
    only17 = np.zeros((1, n), bool)
    only17[0, 17] = True
    ev.node_sets_load(only17)
    got = ev.schedule(pods[:3], T0, node_sets=[1, 1, 1], spread_terms=([[], [], []], [[1, 2], [1], [2, 1]]))
    assert (got[0] == 17).all()
    want = np.zeros((2, n), np.uint16)
    want[0, 17], want[1, 17] = 65535, 2
    assert_counts(ev, want, n)
    # and stays there over a second call
    got = ev.schedule(pods[3:], T0, node_sets=[1], spread_terms=([[(1, AFFINITY, 65535)]], [[1]]))
    assert got[0][0] == 17
    assert_counts(ev, want, n)


# ---- a refusal -----------------------------------------------------------------------------------------------------------
def test_refused_deviceshare_pod_leaves_the_context_untouched(gpu):
    n = 120
    cl = synth.make_cluster(n, synth.BASE_SEED + 9893)
    devs = synth.make_devices(n, synth.BASE_SEED + 9894)
    ev, fresh = Evaluator(synth.config(n)), Evaluator(synth.config(n))
    for h in (ev, fresh):
        synth.load_into(h, cl)
        synth.load_devices(h, devs)
    ev.spread_groups_load(None, [1, 1])
    pods = synth.make_ds_pods(8, synth.BASE_SEED + 9895, device_fraction=1.0)
    with pytest.raises(KoordEvalError) as e:
        ev.schedule(pods, T0, spread_terms=([[(1, ANTI, 1)]] * 8, [[1, 2]] * 8))
    assert e.value.code == abi.ERR_UNSUPPORTED and "spread terms: " in str(e.value) and "DeviceShare" in str(e.value)
    assert not ev.spread_groups_get(1, n).any() and not ev.spread_groups_get(2, n).any()
    assert ev.debug_spread_groups_check() == 0
    plain = synth.make_pods(200, synth.BASE_SEED + 9896)
    got, want = ev.schedule(plain, T0), fresh.schedule(plain, T0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] >= 0).any()
