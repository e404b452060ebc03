"""Spread domains on the device: ke_schedule / submit-ahead against the lock-step reference of
spread_domains.py (pinned on the CPU in test_spread_domains_host.py: its inputs make a site that ignores the skew, or
reads the counts of an earlier batch, move a placement), the counts afterwards on the host and on the device,
ke_spread_domain_add and ke_spread_domain_node_set between calls, a queue with plain and grouped halves, ke_eval /
ke_diagnose with domain ids and a refusal.  Every comparison is exact."""
import numpy as np
import pytest

from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from spread_domains import (Lockstep, eligibility, fresh_oracle, full_mask, group_ids, load, make_input, offsets, plan,
                            reference, reference_without_domains, slice_kw)
from spread_groups import plain_alloc
from test_gpu_diagnose import assert_same, reduce_eval

pytestmark = pytest.mark.gpu
T0 = synth.T0
NONE = abi.DOMAIN_NONE


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
    hold; `counts`: the same for the §4r table."""
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
@pytest.mark.parametrize("name", ["E", "F", "G", "H"])
def test_schedule_lockstep(gpu, name, batch, pipelined):
    r = reference(name)
    ev, kw = context(r, batch, pipelined)
    got = ev.schedule(r["pods"], T0, **kw)
    assert_placed(got, r["want"])
    assert_counts(ev, r["dcounts_after"])
    # the plan restated: batches of several pods with a grouped one among them ran
    want = plan(r["dids"], batch)
    assert len(ev.stats()[1]) == len(want)
    assert batch == 1 or max(want) > 1


@pytest.mark.parametrize("batch", [7, 64])
def test_schedule_with_groups_sets_and_offsets(gpu, batch):
    r = reference("E", extras=True)
    ev, kw = context(r, batch)
    assert set(kw) == {"spread_domains", "spread_groups", "node_sets", "node_scores"}
    got = ev.schedule(r["pods"], T0, **kw)
    assert_placed(got, r["want"])
    assert_counts(ev, r["dcounts_after"], r["counts_after"], r["n"])
    # most placements move against the same run without domain ids
    ev, kw = context(r, batch)
    kw.pop("spread_domains")
    free = ev.schedule(r["pods"], T0, **kw)
    assert_placed(free, reference_without_domains("E", extras=True))
    assert int((free[0] != got[0]).sum()) >= 150
    assert_counts(ev, r["dcounts"])


def test_two_calls_on_one_context(gpu):
    r = reference("E")
    ev, kw = context(r, 64)
    a = ev.schedule(r["pods"][:100], T0, **slice_kw(kw, 0, 100))
    mid = np.stack([ev.spread_domains_get(g + 1) for g in range(len(r["gmap"]))])
    assert (mid != r["dcounts"]).any() and (mid != r["dcounts_after"]).any()
    b = ev.schedule(r["pods"][100:], T0, **slice_kw(kw, 100, None))  # sees the first call's increments
    assert_placed((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), r["want"])
    assert_counts(ev, r["dcounts_after"])


@pytest.mark.parametrize("name", ["E", "F"])
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
    c = make_input("E")
    dids = c["dids"].copy()
    dids[:128] = 0  # two plain batches, then grouped ones
    dids[128:] = np.where(dids[128:] > 0, dids[128:], 1)
    ls = Lockstep(fresh_oracle(c), c)
    want = ls.run(c["pods"], dids, group_ids(c), eligibility(c), offsets(c))
    ev, _ = context(c, 64)
    got = ev.schedule(c["pods"], T0, spread_domains=dids)
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert len(ev.stats()[1]) == len(plan(dids, 64)) > 4
    assert_placed(got, want)
    assert_counts(ev, ls.dcounts[1:])
    # every id 0 on the same context: the call it is without ids
    more = synth.make_pods(128, synth.BASE_SEED + 9761, key_base=9_700_000_000)
    zero = np.zeros(len(more), np.int32)
    got = ev.schedule(more, T0, spread_domains=zero)
    assert ev.kernel_stats()["pipelined_batches"] > 0 and len(ev.stats()[1]) == 2
    assert_placed(got, ls.run(more, zero, zero, np.ones((len(more), c["n"]), bool), np.zeros((len(more), c["n"]), np.int64)))
    assert_counts(ev, ls.dcounts[1:])


def test_domain_add_undo_and_reschedule(gpu):
    c = make_input("E")
    ev, kw = context(c, 64)
    ls = Lockstep(fresh_oracle(c), c)
    elig, off, zero = eligibility(c), offsets(c), group_ids(c)
    pods, dids = c["pods"], c["dids"]
    got = ev.schedule(pods, T0, **kw)
    want = ls.run(pods, dids, zero, elig, off)
    assert_placed(got, want)
    # undo three placements of grouped pods: the Unreserve and the caller's -1
    undo = np.nonzero((want[0] >= 0) & (dids > 0))[0][[3, 40, 90]]
    for p in undo:
        node, g = int(want[0][p]), int(dids[p])
        dom = int(ls.maps[ls.gmap[g], node])
        ev.unreserve(pods[p], int(p))
        ev.spread_domain_add(g, dom, -1)
        ls.o.release(pods[p], plain_alloc(node))
        ls.dcounts[g, dom] -= 1
    assert_counts(ev, ls.dcounts[1:])
    # an informer's pod add in another domain, then the three pods again
    ev.spread_domain_add(1, 2, 1)
    ls.dcounts[1, 2] += 1
    again = ev.schedule(pods[undo], T0, spread_domains=dids[undo])
    assert_placed(again, ls.run(pods[undo], dids[undo], zero[undo], elig[undo], off[undo]))
    assert (again[0] >= 0).all()
    assert_counts(ev, ls.dcounts[1:])
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)


def test_node_set_between_calls(gpu):
    c = dict(make_input("H"))
    ev, kw = context(c, 64)
    ls = Lockstep(fresh_oracle(c), c)
    elig, off, zero = eligibility(c), offsets(c), group_ids(c)
    a = ev.schedule(c["pods"][:128], T0, **slice_kw(kw, 0, 128))
    assert_placed(a, ls.run(c["pods"][:128], c["dids"][:128], zero[:128], elig[:128], off[:128]))
    # the informer relabels nodes: the first call's best nodes lose the key or move to another block, and a node
    # without the key gets one
    moved = np.unique(a[0][a[0] >= 0])[:12]
    none = np.nonzero(c["maps"][1] == NONE)[0][:3]
    for k, node in enumerate(moved):
        dom = NONE if k % 3 == 0 else (int(c["maps"][1, node]) + 1) % 4
        ev.spread_domain_node_set(2, int(node), dom)
        ls.maps[2, node] = dom
    for node in none:
        ev.spread_domain_node_set(2, int(node), 3)
        ev.spread_domain_node_set(1, int(node), 0)
        ls.maps[2, node], ls.maps[1, node] = 3, 0
    assert ev.debug_spread_domains_check() == 0
    b = ev.schedule(c["pods"][128:], T0, **slice_kw(kw, 128, None))
    assert_placed(b, ls.run(c["pods"][128:], c["dids"][128:], zero[128:], elig[128:], off[128:]))
    assert (b[0] >= 0).any()
    assert_counts(ev, ls.dcounts[1:])


def test_single_bit_and_all_64_bit_domains(gpu):
    n = 200
    cl = synth.make_cluster(n, synth.BASE_SEED + 9762)
    pods = synth.make_pods(96, synth.BASE_SEED + 9763)
    rng = np.random.default_rng(synth.BASE_SEED + 9764)
    maps = np.stack([rng.integers(0, 64, n), rng.integers(0, 4, n)])
    # group 1: every domain of the 64-domain map, maxSkew 2; group 2: domain 63 alone (the pod's node affinity admits
    # no other); group 3: bit 2 of the 4-domain map
    c = dict(n=n, cl=cl, pods=pods, maps=maps.astype(np.uint16), gmap=np.array([1, 1, 2], np.int32),
             dom=[full_mask(64), 1 << 63, 1 << 2], skew=np.array([2, 1, 1], np.int32), mind=np.zeros(3, np.int32),
             dids=rng.integers(1, 4, len(pods)).astype(np.int32), dcounts=rng.integers(0, 2, (3, 64)).astype(np.uint32),
             caps=None, counts=None, gids=None, sets=None, sids=None, table=None, tids=None)
    ls = Lockstep(fresh_oracle(c), c)
    want = ls.run(pods, c["dids"], group_ids(c), eligibility(c), offsets(c))
    for g, only in ((2, 63), (3, 2)):  # the single-domain groups' pods all went to their domain
        sel = (c["dids"] == g) & (want[0] >= 0)
        assert sel.any() and (maps[c["gmap"][g - 1] - 1][want[0][sel]] == only).all()
    ev, kw = context(c, 64)
    assert_placed(ev.schedule(pods, T0, **kw), want)
    assert_counts(ev, ls.dcounts[1:])


# ---- ke_eval / ke_diagnose ---------------------------------------------------------------------------------------------
def _open_pairs(r, ls, P):
    return np.stack([ls.domain_ok(int(r["dids"][p])) for p in range(P)])


@pytest.mark.parametrize("name", ["E", "F"])
def test_eval_and_diagnose_filter_closed_domains(gpu, name):
    r = reference(name)
    P = 64
    ev, kw = context(r, 64)
    ls = Lockstep(fresh_oracle(r), r)
    open_ = _open_pairs(r, ls, P)
    assert (~open_).any() and open_.any()
    pods, ids = r["pods"][:P], r["dids"][:P]
    plain = ev.eval(pods, T0)
    got = ev.eval(pods, T0, spread_domains=ids)
    # a closed pair reports as one outside the pod's node set; an open pair as it does without ids
    assert (got["status"][~open_] == abi.CODE_UNSCHEDULABLE_AND_UNRESOLVABLE).all()
    assert (got["reason"][~open_] == abi.REASON_NODE_SET).all()
    assert (got["total"][~open_] == -1).all()
    for k in ("la", "numa", "ds"):
        assert (got[k][~open_] == 0).all(), k
    for k in ("status", "reason", "la", "numa", "ds", "total"):
        assert np.array_equal(got[k][open_], plain[k][open_]), k
    assert not (plain["reason"] == abi.REASON_NODE_SET).any()
    wb = np.array([np.argmax(np.where(open_[p], plain["total"][p], -1)) if (open_[p] & (plain["total"][p] >= 0)).any() else -1
                   for p in range(P)])
    assert np.array_equal(got["best"], wb)
    # ke_diagnose: the same pairs tallied under the node set reason
    dg = ev.diagnose(pods, T0, spread_domains=ids, bitmaps=True)
    assert np.array_equal(dg["reason_nodes"][:, abi.REASON_NODE_SET], (~open_).sum(1))
    assert (dg["plugins"][(~open_).any(1)] & abi.PLUGIN_NODE_SET).all()
    assert_same(dg, reduce_eval(got["status"], got["reason"]), "vs ke_eval")
    assert np.array_equal(dg["unresolvable"] & ~open_, ~open_)
    # neither changed anything, and the ids were consumed
    assert_counts(ev, r["dcounts"])
    again = ev.eval(pods, T0)
    assert np.array_equal(again["total"], plain["total"])
    # together with a node set: a pair outside either reports the same way
    sets = np.random.default_rng(synth.BASE_SEED + 9765).random((1, r["n"])) < 0.5
    ev.node_sets_load(sets)
    both = ev.eval(pods, T0, node_sets=np.ones(P, np.int32), spread_domains=ids)
    assert np.array_equal(both["reason"] == abi.REASON_NODE_SET, ~(open_ & sets[0][None, :]))


# ---- a refusal -----------------------------------------------------------------------------------------------------------
def test_refused_deviceshare_pod_leaves_the_context_untouched(gpu):
    n = 120
    cl = synth.make_cluster(n, synth.BASE_SEED + 9766)
    devs = synth.make_devices(n, synth.BASE_SEED + 9767)
    ev, fresh = Evaluator(synth.config(n)), Evaluator(synth.config(n))
    for h in (ev, fresh):
        synth.load_into(h, cl)
        synth.load_devices(h, devs)
    ev.spread_domains_load(np.arange(n)[None] % 3, [1, 1], [7, 7], [1, 2])
    pods = synth.make_ds_pods(8, synth.BASE_SEED + 9768, device_fraction=1.0)
    with pytest.raises(KoordEvalError) as e:
        ev.schedule(pods, T0, spread_domains=[1] * 8)
    assert e.value.code == abi.ERR_UNSUPPORTED and "spread domains: " in str(e.value) and "DeviceShare" in str(e.value)
    assert not ev.spread_domains_get(1).any() and ev.debug_spread_domains_check() == 0
    plain = synth.make_pods(200, synth.BASE_SEED + 9769)
    got, want = ev.schedule(plain, T0), fresh.schedule(plain, T0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] >= 0).any()
