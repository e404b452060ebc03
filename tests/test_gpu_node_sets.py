"""Per-pod node eligibility sets (ABI v14) on the device: ke_eval's ineligible pairs and its DeviceShare
normalisation over the eligible nodes, ke_schedule / submit-ahead against oracle references that never see an
ineligible node (one oracle per sub-cluster for disjoint sets; for overlapping sets a lock-step oracle: masked argmax
of its eval, then the Reserve by hand -- both pinned on the CPU in test_node_sets_host.py), table maintenance and the
refusals."""
import numpy as np
import pytest

from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from oracle.binding import Oracle
from test_node_sets_host import EVAL_KEYS, manual_reserve, masked_argmax, sub_oracle

pytestmark = pytest.mark.gpu
T0 = synth.T0


def both(cfg, cl, n=None):
    n = n or cl.n_nodes
    ev, o = Evaluator(cfg), Oracle(cfg, n)
    synth.load_into(ev, cl)
    synth.load_into(o, cl)
    return ev, o


def eligibility(sets, ids):
    """bool [pod, node] of the pods' sets (id 0: every node); `sets` a bool [n_sets, N] matrix."""
    return np.concatenate([np.ones((1, sets.shape[1]), bool), sets])[np.asarray(ids)]


def lockstep(o, pods, elig):
    """One pod at a time on the oracle: the masked argmax of its eval (lowest index on ties), then the Reserve."""
    chosen, score = np.full(len(pods), -1, np.int32), np.full(len(pods), -1, np.int32)
    for p in range(len(pods)):
        chosen[p], score[p] = masked_argmax(o.eval(pods[p:p + 1], T0)["total"][0], elig[p])
        if chosen[p] >= 0:
            manual_reserve(o, int(chosen[p]), pods[p])
    return chosen, score


def assert_placed(got, want):
    (c1, s1), (c0, s0) = got, want
    assert np.array_equal(c1, c0), np.argwhere(c1 != c0)[:5].ravel().tolist()
    assert np.array_equal(s1, s0), np.argwhere(s1 != s0)[:5].ravel().tolist()


# ---- 1, 2: ke_eval ---------------------------------------------------------------------------------------------------
def test_eval_parity_plain(gpu):
    n = 333  # two eval blocks, a partial last table word
    cl = synth.make_cluster(n, synth.BASE_SEED + 9201)
    pods = synth.make_pods(40, synth.BASE_SEED + 9202)
    ev, o = both(synth.config(n), cl)
    rng = np.random.default_rng(synth.BASE_SEED + 9203)
    sets = rng.random((3, n)) < 0.45
    ids = rng.integers(0, 4, len(pods))
    ids[:4] = [0, 1, 2, 3]
    ev.node_sets_load(sets)
    got, want = ev.eval(pods, T0, node_sets=ids), o.eval(pods, T0)
    el = eligibility(sets, ids)
    assert (~el).any() and el.any()
    for k in EVAL_KEYS + ("ds",):
        assert np.array_equal(got[k][el], want[k][el]), k
    assert (got["status"][~el] == abi.CODE_UNSCHEDULABLE_AND_UNRESOLVABLE).all()
    assert (got["reason"][~el] == abi.REASON_NODE_SET).all()
    for k in ("la", "numa", "ds"):
        assert (got[k][~el] == 0).all(), k
    assert (got["total"][~el] == -1).all()
    best = [masked_argmax(want["total"][p], el[p])[0] for p in range(len(pods))]
    assert got["best"].tolist() == best
    # the ids were consumed: the next call is the plain one
    again = ev.eval(pods, T0)
    for k in EVAL_KEYS + ("best",):
        assert np.array_equal(again[k], want[k]), k


def test_eval_parity_deviceshare_normalises_over_the_set(gpu):
    n = 96
    cl = synth.make_cluster(n, synth.BASE_SEED + 9211)
    devs = synth.make_devices(n, synth.BASE_SEED + 9212)
    pods = synth.make_ds_pods(36, synth.BASE_SEED + 9213, device_fraction=0.8)
    ev = Evaluator(synth.config(n))
    synth.load_into(ev, cl)
    synth.load_devices(ev, devs)
    rng = np.random.default_rng(synth.BASE_SEED + 9214)
    sets = rng.random((3, n)) < 0.4
    ids = 1 + np.arange(len(pods)) % 3  # one set per pod group
    ev.node_sets_load(sets)
    got = ev.eval(pods, T0, node_sets=ids)
    assert (got["ds"] > 0).any()
    for s in range(3):
        idx, grp = np.nonzero(sets[s])[0], np.nonzero(ids == s + 1)[0]
        want = sub_oracle(synth.config, cl, idx, devices=devs).eval(pods[grp], T0)
        for k in EVAL_KEYS + ("ds",):
            assert np.array_equal(got[k][np.ix_(grp, idx)], want[k]), (s, k)
        wb = np.where(want["best"] >= 0, idx[np.maximum(want["best"], 0)], -1)
        assert np.array_equal(got["best"][grp], wb), s
        out = np.setdiff1d(np.arange(n), idx)
        assert (got["reason"][np.ix_(grp, out)] == abi.REASON_NODE_SET).all()
        assert (got["total"][np.ix_(grp, out)] == -1).all()


def test_eval_empty_slots_under_node_sets(gpu):
    """A pin of ke_eval at empty node slots in a call with node sets: the set gate comes ahead of the slot's own
    validity test, so an empty slot outside the pod's set reports KE_REASON_NODE_SET and one inside it (or any with
    id 0) KE_CODE_ERROR; ke_diagnose counts an empty slot as absent whatever the set says."""
    n, cap = 200, 320
    cl = synth.make_cluster(n, synth.BASE_SEED + 9221)
    ev, o = both(synth.config(cap), cl, n)
    gone = [0, 63, 64, 130, 199]
    for h in (ev, o):
        for i in gone:
            h.delete_node(i)
    assert ev.num_nodes == n
    present = np.ones(n, bool)
    present[gone] = False
    sets = np.random.default_rng(synth.BASE_SEED + 9222).random((3, n)) < 0.5
    sets[0, gone] = [True, False, True, False, True]   # every deleted node inside at least one set
    sets[1, gone] = [False, True, False, True, False]  # ... and outside at least one
    assert sets[:, gone].any(0).all() and not sets[:, gone].all(0).any()
    pods = synth.make_pods(8, synth.BASE_SEED + 9223)
    ids = np.array([0, 1, 2, 3, 0, 1, 2, 3])
    ev.node_sets_load(sets)
    el = eligibility(sets, ids)
    got, want = ev.eval(pods, T0, node_sets=ids), o.eval(pods, T0)
    # every pair outside the pod's set, the deleted columns included
    assert (~el[:, gone]).any() and el[:, gone].any()
    assert (got["status"][~el] == abi.CODE_UNSCHEDULABLE_AND_UNRESOLVABLE).all()
    assert (got["reason"][~el] == abi.REASON_NODE_SET).all()
    # a deleted column inside the set (or id 0): the empty slot itself
    empty = el & ~present
    assert (got["status"][empty] == abi.CODE_ERROR).all()
    assert (got["reason"][empty] == abi.REASON_NONE).all()
    for k in ("la", "numa", "ds"):
        assert (got[k][:, gone] == 0).all() and (got[k][~el] == 0).all(), k
    assert (got["total"][:, gone] == -1).all() and (got["total"][~el] == -1).all()
    # the populated columns: the oracle
    live = el & present
    for k in EVAL_KEYS + ("ds",):
        assert np.array_equal(got[k][live], want[k][live]), k
    d = ev.diagnose(pods, T0, node_sets=ids)
    assert (d["n_absent"] == len(gone)).all() and (d["n_nodes"] == n - len(gone)).all()
    assert np.array_equal(d["reason_nodes"][:, abi.REASON_NODE_SET], (~el & present).sum(1))


# ---- 3, 4: ke_schedule, disjoint sets: one oracle per sub-cluster ----------------------------------------------------
def _partition(n, n_pods, seed):
    rng = np.random.default_rng(synth.BASE_SEED + seed)
    cls = rng.integers(2, 4, n)       # classes 2 and 3 interleaved over the node indices
    cls[[7, 53, 88, 131]] = 1         # class 1: 4 nodes
    return cls, rng.integers(1, 4, n_pods)  # the pods' classes interleave in the queue


def _partition_reference(cfg_of, cl, pods, cls, pc, tables=None):
    chosen, score = np.full(len(pods), -1, np.int32), np.full(len(pods), -1, np.int32)
    unplaced = {}
    for c in (1, 2, 3):
        idx, grp = np.nonzero(cls == c)[0], np.nonzero(pc == c)[0]
        ch, sc = sub_oracle(cfg_of, cl, idx, tables=tables).schedule(pods[grp], T0)
        chosen[grp] = np.where(ch >= 0, idx[np.maximum(ch, 0)], -1)
        score[grp] = sc
        unplaced[c] = int((ch < 0).sum())
    return chosen, score, unplaced


def test_schedule_partition_pipelined(gpu):
    n = 150
    cl = synth.make_cluster(n, synth.BASE_SEED + 9101)
    pods = synth.make_pods(2500, synth.BASE_SEED + 9102)
    cls, pc = _partition(n, len(pods), 9103)
    c0, s0, unplaced = _partition_reference(synth.config, cl, pods, cls, pc)
    # the 4-node class saturates, the others do not: an unmasked site would send a class-1 pod elsewhere
    assert unplaced[1] >= 100 and unplaced[2] == 0 and unplaced[3] == 0, unplaced
    ev = Evaluator(synth.config(n, pod_batch=64))
    synth.load_into(ev, cl)
    ev.node_sets_load(np.stack([cls == c for c in (1, 2, 3)]))
    got = ev.schedule(pods, T0, node_sets=pc)
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, (c0, s0))
    assert ev.check_records(T0) == 0
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)


def test_schedule_partition_ext_resources(gpu):
    n = 150
    cfg_of = lambda m: synth.ext_config(synth.config(m, pod_batch=64))  # noqa: E731
    cl = synth.make_cluster(n, synth.BASE_SEED + 9111)
    tables = synth.make_node_resources(cl, synth.BASE_SEED + 9112)
    pods = synth.add_pod_xres(synth.make_pods(600, synth.BASE_SEED + 9113), synth.BASE_SEED + 9114)
    cls, pc = _partition(n, len(pods), 9115)
    c0, s0, unplaced = _partition_reference(cfg_of, cl, pods, cls, pc, tables=tables)
    assert unplaced[1] > 0 and unplaced[2] == 0 and unplaced[3] == 0, unplaced
    ev = Evaluator(cfg_of(n))
    synth.load_into(ev, cl)
    synth.load_node_resources(ev, tables)
    ev.node_sets_load(np.stack([cls == c for c in (1, 2, 3)]))
    got = ev.schedule(pods, T0, node_sets=pc)
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, (c0, s0))
    assert ev.check_records(T0) == 0


# ---- 5, 6: overlapping sets, the lock-step oracle -------------------------------------------------------------------
_OVERLAP = {}


def _overlap():
    if not _OVERLAP:
        n = 150
        cl = synth.make_cluster(n, synth.BASE_SEED + 9121)
        pods = synth.make_pods(600, synth.BASE_SEED + 9122)
        rng = np.random.default_rng(synth.BASE_SEED + 9123)
        sets = rng.random((4, n)) < 0.4
        ids = rng.integers(0, 5, len(pods))
        o = Oracle(synth.config(n), n)
        synth.load_into(o, cl)
        want = lockstep(o, pods, eligibility(sets, ids))
        assert (want[0] >= 0).sum() > 300
        _OVERLAP.update(n=n, cl=cl, pods=pods, sets=sets, ids=ids, want=want)
    return _OVERLAP


def _overlap_ctx(batch):
    r = _overlap()
    ev = Evaluator(synth.config(r["n"], pod_batch=batch))
    synth.load_into(ev, r["cl"])
    ev.node_sets_load(r["sets"])
    return r, ev


@pytest.mark.parametrize("pipelined", [True, False], ids=["pipelined", "serial"])
@pytest.mark.parametrize("batch", [1, 7, 64])
def test_schedule_overlapping_sets_lockstep(gpu, batch, pipelined):
    r, ev = _overlap_ctx(batch)
    ev.set_pipeline(pipelined)
    got = ev.schedule(r["pods"], T0, node_sets=r["ids"])
    assert_placed(got, r["want"])
    el = eligibility(r["sets"], r["ids"])
    placed = got[0] >= 0
    assert el[np.nonzero(placed)[0], got[0][placed]].all()
    assert ev.check_records(T0) == 0


def test_submit_ahead_with_sets(gpu):
    r, ev = _overlap_ctx(64)
    pods, ids = r["pods"], r["ids"]
    cuts = list(range(0, len(pods), 100))
    chosen, score, prev = [], [], None
    for a in cuts:  # one call kept in flight
        t = ev.submit(pods[a:a + 100], T0, node_sets=ids[a:a + 100])
        if prev is not None:
            c, s = ev.wait(prev)
            chosen.append(c), score.append(s)
        prev = t
    c, s = ev.wait(prev)
    chosen.append(c), score.append(s)
    got = (np.concatenate(chosen), np.concatenate(score))
    assert_placed(got, r["want"])
    _, one = _overlap_ctx(64)
    single = one.schedule(pods, T0, node_sets=ids)
    assert np.array_equal(got[0], single[0]) and np.array_equal(got[1], single[1])
    assert ev.check_records(T0) == 0


# ---- 7: table maintenance --------------------------------------------------------------------------------------------
def test_table_maintenance(gpu):
    n = 150
    cl = synth.make_cluster(n, synth.BASE_SEED + 9131)
    ev, o = both(synth.config(n), cl)
    sets = np.zeros((3, n), bool)
    sets[0, 10:30] = True
    sets[1, ::3] = True       # set 3 stays empty
    ev.node_sets_load(sets)
    q = [synth.make_pods(40, synth.BASE_SEED + 9132 + i, key_base=9_100_000_000 + 1000 * i) for i in range(6)]
    ids = np.array([1, 2] * 20)
    got = ev.schedule(q[0], T0, node_sets=ids)
    assert_placed(got, lockstep(o, q[0], eligibility(sets, ids)))
    # a node flipped out of set 1 (and into set 3): the next call no longer places set 1's pods there
    x = int(np.bincount(got[0][(ids == 1) & (got[0] >= 0)]).argmax())
    sets[0, x], sets[2, x] = False, True
    ev.node_set_bits(x, sets[:, x])
    got = ev.schedule(q[1], T0, node_sets=ids)
    assert not (got[0][ids == 1] == x).any()
    assert_placed(got, lockstep(o, q[1], eligibility(sets, ids)))
    ids3 = np.array([3, 0] * 20)
    got = ev.schedule(q[2], T0, node_sets=ids3)
    assert set(got[0][ids3 == 3].tolist()) <= {x, -1}
    assert_placed(got, lockstep(o, q[2], eligibility(sets, ids3)))
    # an empty set: every pod -1 and no state change
    sets[2, x] = False
    ev.node_set_bits(x, sets[:, x])
    before = ev.debug_rows(T0)[0].copy()
    c, _ = ev.schedule(q[3], T0, node_sets=np.full(40, 3))
    assert (c == -1).all()
    assert np.array_equal(ev.debug_rows(T0)[0], before)
    assert ev.check_records(T0) == 0
    # a table of one word per set: nodes at or beyond 64 are ineligible
    ev.node_sets_load(np.ones((1, 64), bool))
    short = np.zeros((1, n), bool)
    short[0, :64] = True
    got = ev.schedule(q[4], T0, node_sets=np.ones(40, np.int32))
    assert (got[0] < 64).all()
    assert_placed(got, lockstep(o, q[4], eligibility(short, np.ones(40, np.int32))))
    # n_sets = 0: the no-set behaviour
    ev.node_sets_load([])
    with pytest.raises(KoordEvalError):
        ev.pod_node_sets([1] * 40)
    c1, s1 = ev.schedule(q[5], T0)
    c0, s0 = o.schedule(q[5], T0)
    assert np.array_equal(c1, c0) and np.array_equal(s1, s0)
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)


# ---- 8: refusals -----------------------------------------------------------------------------------------------------
def _refused_then_clean(ev, fresh, pods, ids):
    ev.pod_node_sets(ids)
    with pytest.raises(KoordEvalError) as e:
        ev.schedule(pods, T0)
    assert e.value.code == abi.ERR_UNSUPPORTED and "node sets" in str(e.value)
    plain = synth.make_pods(200, synth.BASE_SEED + 9149)
    got, want = ev.schedule(plain, T0), fresh.schedule(plain, T0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert (got[0] >= 0).any()


def _pair(n, seed, devices=False, shard=False):
    cl = synth.make_cluster(n, synth.BASE_SEED + seed)
    devs = synth.make_devices(n, synth.BASE_SEED + seed + 1) if devices else None
    out = []
    for _ in range(2):
        ev = Evaluator(synth.config(n))
        if shard:
            ev.shard_init(0, 2)  # both shards in this context
        synth.load_into(ev, cl)
        if devs is not None:
            synth.load_devices(ev, devs)
        ev.node_sets_load(np.ones((1, n), bool))
        out.append(ev)
    return out


def test_refused_deviceshare_pod(gpu):
    ev, fresh = _pair(120, 9141, devices=True)
    pods = synth.make_ds_pods(8, synth.BASE_SEED + 9143, device_fraction=1.0)
    _refused_then_clean(ev, fresh, pods, [1] * 8)


def test_refused_numa_policy_pod(gpu):
    ev, fresh = _pair(120, 9144)
    pods = synth.make_pods(8, synth.BASE_SEED + 9145)
    pods["numa_topology_policy"][3] = abi.NUMA_POLICY_SINGLE_NUMA_NODE
    _refused_then_clean(ev, fresh, pods, [0, 0, 1, 0, 0, 0, 0, 0])


def test_refused_sharded_context(gpu):
    ev, fresh = _pair(120, 9146, shard=True)
    pods = synth.make_pods(8, synth.BASE_SEED + 9147)
    _refused_then_clean(ev, fresh, pods, [1] * 8)
    ev.pod_node_sets([1] * 8)
    with pytest.raises(KoordEvalError) as e:
        ev.eval(pods, T0)
    assert e.value.code == abi.ERR_UNSUPPORTED
