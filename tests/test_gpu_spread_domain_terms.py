"""Spread domain terms on the device: ke_schedule / submit-ahead against the lock-step reference of
spread_domain_terms.py (pinned on the CPU in test_spread_domain_terms_host.py: its inputs make a site that drops a
filter term, reads the counts of another batch, takes the bonus from other counts or skips a member move a placement),
the counts afterwards on the host and on the device, the batch count against the plan restated, ke_spread_domain_add
undos and a ke_spread_domain_node_set relabel between calls, a queue with plain and listed halves, the §4s
equivalence, ke_eval / ke_diagnose with lists, a node without the topology key under each kind, scores on both sides of
511 and a refusal.  Every comparison is exact."""
import numpy as np
import pytest

import spread_domains
from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from landscapes import flat_cluster, ls_pods
from spread_domain_terms import (AFFINITY, ANTI, FEWER, MORE, SKEW, Lockstep, eligibility, fresh_oracle, from_domain_ids,
                                 load, make_input, node_terms, offsets, plan, reference, slice_kw)
from spread_domains import D, NONE, full_mask
from spread_groups import plain_alloc
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


def assert_counts(ev, dcounts, counts=None, n=0):
    """The host copy (ke_spread_domains_get) equals `dcounts`, the device copy equals the host copy, the records
    hold; `counts`: the same for the spread groups' table (§4t lists)."""
    for g in range(len(dcounts)):
        got = ev.spread_domains_get(g + 1)
        assert np.array_equal(got, dcounts[g]), (g + 1, np.nonzero(got != dcounts[g])[0][:5].tolist())
    assert ev.debug_spread_domains_check() == 0
    for g in range(0 if counts is None else len(counts)):
        assert np.array_equal(ev.spread_groups_get(g + 1, n), counts[g]), g + 1
    assert ev.debug_spread_groups_check() == 0
    assert ev.check_records(T0) == 0


# ---- ke_schedule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipelined", [True, False], ids=["pipelined", "serial"])
@pytest.mark.parametrize("batch", [1, 7, 64])
@pytest.mark.parametrize("name", ["P", "Q", "R", "Y"])
def test_schedule_lockstep(gpu, name, batch, pipelined):
    r = reference(name)
    ev, kw = context(r, batch, pipelined)
    if name == "Y":
        assert set(kw) == {"spread_domain_terms", "spread_terms", "node_sets", "node_scores"}
    got = ev.schedule(r["pods"], T0, **kw)
    assert_placed(got, r["want"])
    assert_counts(ev, r["dcounts_after"], r["counts_after"] if name == "Y" else None, r["n"])
    # the plan restated: the call ran its batches (R: uncut ones)
    want = plan(r["dterms"], r["dmembers"], batch)
    assert len(ev.stats()[1]) == len(want)
    assert batch == 1 or max(want) > 1
    assert name != "R" or want == [batch] * (256 // batch) + ([256 % batch] if 256 % batch else [])


def test_two_calls_on_one_context(gpu):
    r = reference("P")
    ev, kw = context(r, 64)
    a = ev.schedule(r["pods"][:100], T0, **slice_kw(kw, 0, 100))
    mid = np.stack([ev.spread_domains_get(g + 1) for g in range(len(r["gmap"]))])
    assert (mid != r["dcounts"]).any() and (mid != r["dcounts_after"]).any()
    b = ev.schedule(r["pods"][100:], T0, **slice_kw(kw, 100, None))  # sees the first call's increments
    assert_placed((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), r["want"])
    assert_counts(ev, r["dcounts_after"])


@pytest.mark.parametrize("name", ["Q", "R"])
def test_submit_ahead(gpu, name):
    r = reference(name)
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
    assert_counts(ev, r["dcounts_after"])


def test_mixed_queue_keeps_plain_batches_pipelined(gpu):
    c = make_input("P")
    P = len(c["pods"])
    terms = [[] if p < 128 else c["dterms"][p] for p in range(P)]  # two plain batches, then listed ones
    members = [[] if p < 128 else c["dmembers"][p] for p in range(P)]
    ls = Lockstep(fresh_oracle(c), c)
    want = ls.run(c["pods"], terms, members, eligibility(c), offsets(c))
    ev, _ = context(c, 64)
    got = ev.schedule(c["pods"], T0, spread_domain_terms=(terms, members))
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert len(ev.stats()[1]) == len(plan(terms, members, 64)) > 4
    assert_placed(got, want)
    assert_counts(ev, ls.dcounts[1:])
    # every list empty on the same context: the call it is without lists
    more = synth.make_pods(128, synth.BASE_SEED + 9971, key_base=9_900_000_000)
    got = ev.schedule(more, T0, spread_domain_terms=([[]] * len(more), [[]] * len(more)))
    assert ev.kernel_stats()["pipelined_batches"] > 0 and len(ev.stats()[1]) == 2
    assert_placed(got, ls.run(more, [[]] * len(more), [[]] * len(more), np.ones((len(more), c["n"]), bool),
                              np.zeros((len(more), c["n"]), np.int64)))
    assert_counts(ev, ls.dcounts[1:])


def test_domain_add_undos_and_a_relabel_between_calls(gpu):
    c = make_input("P")
    ev, kw = context(c, 64)
    ls = Lockstep(fresh_oracle(c), c)
    elig, off = eligibility(c), offsets(c)
    pods, terms, members = c["pods"], c["dterms"], c["dmembers"]
    got = ev.schedule(pods[:192], T0, **slice_kw(kw, 0, 192))
    want = ls.run(pods[:192], terms[:192], members[:192], elig[:192], off[:192])
    assert_placed(got, want)
    # undo three placements, one of a pod with two members: the Unreserve and the caller's -1 per member
    placed = [p for p in range(192) if want[0][p] >= 0]
    two = [p for p in placed if len(members[p]) == 2][5]
    undo = np.array([placed[3], two, placed[-1]])
    for p in undo:
        node = int(want[0][p])
        ev.unreserve(pods[p], int(p))
        ls.o.release(pods[p], plain_alloc(node))
        for m in members[p]:
            dom = int(ls.maps[ls.gmap[m], node])
            if dom < D:
                ev.spread_domain_add(m, dom, -1)
                ls.dcounts[m, dom] -= 1
    assert_counts(ev, ls.dcounts[1:])
    # the informer relabels nodes the first call used: some lose the key, some move to the next zone / rack
    moved = np.unique(want[0][want[0] >= 0])[:12]
    for k, node in enumerate(moved):
        for m, width in ((1, 3), (2, 7)):
            dom = NONE if k % 3 == 0 else (int(c["maps"][m - 1, node]) + 1) % width
            ev.spread_domain_node_set(m, int(node), dom)
            ls.maps[m, node] = dom
    assert ev.debug_spread_domains_check() == 0
    # the three pods again, then the rest of the queue
    sub = ([terms[p] for p in undo], [members[p] for p in undo])
    again = ev.schedule(pods[undo], T0, spread_domain_terms=sub)
    assert_placed(again, ls.run(pods[undo], sub[0], sub[1], elig[undo], off[undo]))
    rest = ev.schedule(pods[192:], T0, **slice_kw(kw, 192, None))
    assert_placed(rest, ls.run(pods[192:], terms[192:], members[192:], elig[192:], off[192:]))
    assert (rest[0] >= 0).any()
    assert_counts(ev, ls.dcounts[1:])
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)


@pytest.mark.parametrize("name", ["E", "G"])
def test_domain_ids_are_the_special_case(gpu, name):
    g = spread_domains.reference(name)
    c = from_domain_ids(g)
    ev = Evaluator(synth.config(g["n"], pod_batch=64))
    synth.load_into(ev, g["cl"])
    kw = load(ev, c)
    got = ev.schedule(g["pods"], T0, **kw)
    assert_placed(got, g["want"])
    assert_counts(ev, g["dcounts_after"])
    assert len(ev.stats()[1]) == len(spread_domains.plan(g["dids"], 64))


# ---- ke_eval / ke_diagnose ---------------------------------------------------------------------------------------------
CLASSES = ([(1, ANTI, 3, 0), (2, FEWER, 3, 10)], [(2, AFFINITY, 1, 0), (3, MORE, 2, 7)],
           [(3, SKEW, 0, 0), (1, AFFINITY, 1, 0), (1, MORE, 2, 5), (2, FEWER, 2, 9)])


def _ds_context():
    n = 96
    cl = synth.make_cluster(n, synth.BASE_SEED + 9981)
    devs = synth.make_devices(n, synth.BASE_SEED + 9982)
    pods = synth.make_ds_pods(36, synth.BASE_SEED + 9983, device_fraction=0.8)
    ev = Evaluator(synth.config(n))
    synth.load_into(ev, cl)
    synth.load_devices(ev, devs)
    rng = np.random.default_rng(synth.BASE_SEED + 9984)
    maps = np.stack([rng.integers(0, 3, n), rng.integers(0, 7, n)])
    maps[:, rng.random(n) < 0.1] = NONE
    c = dict(n=n, maps=maps.astype(np.uint16), gmap=np.array([1, 2, 2], np.int32), dom=[full_mask(3), full_mask(7), full_mask(7)],
             skew=np.array([1, 1, 1], np.int32), mind=np.zeros(3, np.int32), dcounts=np.zeros((3, D), np.uint32), x=None)
    c["dcounts"][0, :3] = rng.integers(0, 4, 3)
    c["dcounts"][1:, :7] = rng.integers(0, 3, (2, 7))
    ev.spread_domains_load(c["maps"], c["gmap"], c["dom"], c["skew"], c["mind"], c["dcounts"])
    cls = np.arange(len(pods)) % 3  # one term list per pod class
    lists = ([CLASSES[k] for k in cls], [[1 + int(k)] for k in cls])
    return n, cl, devs, pods, ev, Lockstep(None, c), cls, lists, c


def test_eval_applies_filter_terms_and_adds_the_bonus_behind_the_normalisation(gpu):
    n, cl, devs, pods, ev, ls, cls, lists, c = _ds_context()
    got = ev.eval(pods, T0, spread_domain_terms=lists)
    assert (got["ds"] > 0).any()
    for k in range(3):
        ok, bonus = ls.apply(CLASSES[k])
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
    assert_counts(ev, c["dcounts"])
    plain = ev.eval(pods, T0)
    assert not (plain["reason"] == abi.REASON_NODE_SET).any()
    # lists together with a node set: a pair outside either reports the same way
    sets = np.random.default_rng(synth.BASE_SEED + 9985).random((1, n)) < 0.5
    ev.node_sets_load(sets)
    both = ev.eval(pods, T0, node_sets=np.ones(len(pods), np.int32), spread_domain_terms=lists)
    open_ = sets[0][None, :] & np.stack([ls.apply(CLASSES[k])[0] for k in cls])
    assert np.array_equal(both["reason"] == abi.REASON_NODE_SET, ~open_)
    assert (both["total"][~open_] == -1).all() and (both["total"][open_] >= 0).any()


def test_diagnose_counts_filtered_pairs_under_node_set(gpu):
    n, cl, devs, pods, ev, ls, cls, lists, c = _ds_context()
    closed = ~np.stack([ls.apply(CLASSES[k])[0] for k in cls])
    got = ev.diagnose(pods, T0, spread_domain_terms=lists, bitmaps=True)
    assert np.array_equal(got["reason_nodes"][:, abi.REASON_NODE_SET], closed.sum(1))
    assert (got["plugins"][closed.any(1)] & abi.PLUGIN_NODE_SET).all()
    dev = ev.eval(pods, T0, spread_domain_terms=lists)
    assert_same(got, reduce_eval(dev["status"], dev["reason"]), "vs ke_eval")
    assert np.array_equal(got["unresolvable"] & closed, closed)
    # the score kinds alone filter nothing
    soft = ([[t for t in tl if t[1] in (FEWER, MORE)] for tl in lists[0]], lists[1])
    assert not ev.diagnose(pods, T0, spread_domain_terms=soft)["reason_nodes"][:, abi.REASON_NODE_SET].any()
    assert_counts(ev, c["dcounts"])  # ke_diagnose changes nothing


# ---- the edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [SKEW, ANTI, AFFINITY, FEWER, MORE])
def test_a_node_without_the_topology_key_under_each_kind(gpu, kind):
    """Node 17 is far the best node of a flat cluster's first pods (a score table) and has no zone: SKEW and AFFINITY
    close it, ANTI leaves it open whatever the counts, the score kinds leave it open and add nothing there."""
    n, P = 130, 6
    cl = flat_cluster(n)
    pods = ls_pods(P, synth.BASE_SEED + 9986)
    maps = (np.arange(n) % 3)[None].astype(np.int64)
    maps[0, 17] = NONE
    dc = np.zeros((1, D), np.uint32)
    dc[0, :3] = [3, 3, 4]
    c = dict(n=n, cl=cl, pods=pods, maps=maps.astype(np.uint16), gmap=np.array([1], np.int32), dom=[full_mask(3)],
             skew=np.array([2], np.int32), mind=np.zeros(1, np.int32), dcounts=dc, x=None)
    term = {SKEW: (1, SKEW, 0, 0), ANTI: (1, ANTI, 1, 0), AFFINITY: (1, AFFINITY, 1, 0), FEWER: (1, FEWER, 9, 5),
            MORE: (1, MORE, 9, 5)}[kind]
    terms, members = [[term]] * P, [[1]] * P
    table = np.zeros((1, n), np.int64)
    table[0, 17] = 120  # (above any bonus here: 9 * 5)
    off = np.repeat(table, P, 0)
    ls = Lockstep(fresh_oracle(c), c)
    want = ls.run(pods, terms, members, np.ones((P, n), bool), off)
    on17 = int((want[0] == 17).sum())
    if kind in (SKEW, AFFINITY):
        assert on17 == 0 and (want[0] >= 0).all()
    elif kind == ANTI:  # every zone is at its limit: the keyless node alone is open
        assert (want[0][want[0] >= 0] == 17).all() and on17 >= 1
    else:  # (the exact scores below: the offset alone, no bonus)
        assert on17 >= 1
    for batch in (1, 64):
        ev = Evaluator(synth.config(n, pod_batch=batch))
        synth.load_into(ev, cl)
        ev.spread_domains_load(c["maps"], c["gmap"], c["dom"], c["skew"], c["mind"], c["dcounts"])
        ev.node_scores_load(table)
        got = ev.schedule(pods, T0, spread_domain_terms=(terms, members), node_scores=np.ones(P, np.int32))
        assert_placed(got, want)
        assert_counts(ev, ls.dcounts[1:])  # a placement on node 17 counts for no domain
    e = ev.eval(pods[:1], T0, spread_domain_terms=([[term]], [[]]))
    assert (e["reason"][0, 17] == abi.REASON_NODE_SET) == (kind in (SKEW, AFFINITY))


@pytest.mark.parametrize("batch", [7, 64])
def test_scores_on_both_sides_of_511_in_one_select(gpu, batch):
    n, P = 333, 128
    cl = flat_cluster(n)
    pods = ls_pods(P, synth.BASE_SEED + 9991)
    rng = np.random.default_rng(synth.BASE_SEED + 9992)
    maps = rng.choice(64, n, p=np.r_[np.full(8, 0.0125), np.full(56, 0.9 / 56)])[None]  # eight small domains
    dc = np.full((1, D), 7, np.uint32)
    dc[0, :8] = rng.integers(0, 7, 8)  # ... above the rest: they fill up, and the pods move down the levels
    c = dict(n=n, cl=cl, pods=pods, maps=maps.astype(np.uint16), gmap=np.array([1], np.int32), dom=[full_mask(64)],
             skew=np.array([1], np.int32), mind=np.zeros(1, np.int32), dcounts=dc, x=None,
             dterms=[[(1, FEWER, 7, 100)]] * P, dmembers=[[1]] * P)
    ls = Lockstep(fresh_oracle(c), c)
    want = ls.run(pods, c["dterms"], c["dmembers"], eligibility(c), offsets(c))
    print("scores", int(want[1].max()), int((want[1] > 511).sum()), int((want[1] < 511).sum()))
    assert want[1].max() > 700 and (want[1] > 511).sum() >= 8 and (want[1] < 511).sum() >= 8 and (want[0] >= 0).all()
    ev, kw = context(c, batch)
    assert_placed(ev.schedule(pods, T0, **kw), want)
    assert_counts(ev, ls.dcounts[1:])


# ---- a refusal -----------------------------------------------------------------------------------------------------------
def test_refused_deviceshare_pod_leaves_the_context_untouched(gpu):
    n = 120
    cl = synth.make_cluster(n, synth.BASE_SEED + 9993)
    devs = synth.make_devices(n, synth.BASE_SEED + 9994)
    ev, fresh = Evaluator(synth.config(n)), Evaluator(synth.config(n))
    for h in (ev, fresh):
        synth.load_into(h, cl)
        synth.load_devices(h, devs)
    ev.spread_domains_load(np.arange(n)[None] % 3, [1, 1], [7, 7], [1, 2])
    pods = synth.make_ds_pods(8, synth.BASE_SEED + 9995, device_fraction=1.0)
    with pytest.raises(KoordEvalError) as e:
        ev.schedule(pods, T0, spread_domain_terms=([[(1, ANTI, 1)]] * 8, [[1, 2]] * 8))
    assert e.value.code == abi.ERR_UNSUPPORTED and "spread domain terms: " in str(e.value) and "DeviceShare" in str(e.value)
    assert not ev.spread_domains_get(1).any() and not ev.spread_domains_get(2).any()
    assert ev.debug_spread_domains_check() == 0
    plain = synth.make_pods(200, synth.BASE_SEED + 9996)
    got, want = ev.schedule(plain, T0), fresh.schedule(plain, T0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] >= 0).any()
