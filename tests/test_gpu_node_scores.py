"""Per-pod node score offsets on the device: ke_eval's total and best with the offset (DeviceShare pods and node sets
too), ke_schedule / submit-ahead bit-exact with the lock-step oracle reference (its eval's total plus the offset
where feasible, the masked argmax, the Reserve by hand -- pinned on the CPU in test_node_scores_host.py), keys on both
sides of bit 31, the ext-resource instantiations, table maintenance and the refusals."""
import numpy as np
import pytest

from koordinator_amd import Evaluator, KoordEvalError, abi, synth
from oracle.binding import Oracle
from test_node_scores_host import lockstep_scores, offsets_of
from test_node_sets_host import EVAL_KEYS, masked_argmax, sub_oracle

pytestmark = pytest.mark.gpu
T0 = synth.T0
CAP = 722  # synth.config's weights 1/1/1


def both(cfg, cl):
    ev, o = Evaluator(cfg), Oracle(cfg, cl.n_nodes)
    synth.load_into(ev, cl)
    synth.load_into(o, cl)
    return ev, o


def with_offset(total, off):
    return np.where(total >= 0, total.astype(np.int64) + off, -1)


def assert_placed(got, want):
    (c1, s1), (c0, s0) = got, want
    assert np.array_equal(c1, c0), np.argwhere(c1 != c0)[:5].ravel().tolist()
    assert np.array_equal(s1, s0), np.argwhere(s1 != s0)[:5].ravel().tolist()


# ---- 1, 2: ke_eval ---------------------------------------------------------------------------------------------------
def test_eval_plain(gpu):
    n = 333  # two eval blocks, a partial last 64-node segment
    cl = synth.make_cluster(n, synth.BASE_SEED + 9331)
    pods = synth.make_pods(40, synth.BASE_SEED + 9332)
    ev, o = both(synth.config(n), cl)
    rng = np.random.default_rng(synth.BASE_SEED + 9333)
    tables = rng.integers(0, 201, (3, n))
    ids = rng.integers(0, 4, len(pods))
    ids[:4] = [0, 1, 2, 3]
    ev.node_scores_load(tables)
    got, want = ev.eval(pods, T0, node_scores=ids), o.eval(pods, T0)
    off = offsets_of(tables, ids, n)
    total = with_offset(want["total"], off)
    assert (want["total"] >= 0).any() and (want["total"] < 0).any() and (total != want["total"]).any()
    assert np.array_equal(got["total"], total)
    for k in ("status", "reason", "la", "numa"):
        assert np.array_equal(got[k], want[k]), k
    everywhere = np.ones(n, bool)
    assert got["best"].tolist() == [masked_argmax(total[p], everywhere)[0] for p in range(len(pods))]
    # the ids were consumed: the next call is the plain one
    again = ev.eval(pods, T0)
    for k in EVAL_KEYS + ("best",):
        assert np.array_equal(again[k], want[k]), k


def test_eval_deviceshare_and_node_sets(gpu):
    n = 96
    cl = synth.make_cluster(n, synth.BASE_SEED + 9341)
    devs = synth.make_devices(n, synth.BASE_SEED + 9342)
    pods = synth.make_ds_pods(36, synth.BASE_SEED + 9343, device_fraction=0.8)
    ev, o = both(synth.config(n), cl)
    synth.load_devices(ev, devs)
    synth.load_devices(o, devs)
    rng = np.random.default_rng(synth.BASE_SEED + 9344)
    tables = rng.integers(0, 201, (3, n))
    tids = rng.integers(0, 4, len(pods))
    tids[:4] = [0, 1, 2, 3]
    off = offsets_of(tables, tids, n)
    ev.node_scores_load(tables)
    got, want = ev.eval(pods, T0, node_scores=tids), o.eval(pods, T0)
    assert (want["ds"] > 0).any()
    for k in ("status", "reason", "la", "numa", "ds"):  # the offset comes after DeviceShare's normalisation
        assert np.array_equal(got[k], want[k]), k
    total = with_offset(want["total"], off)
    assert np.array_equal(got["total"], total)
    assert got["best"].tolist() == [masked_argmax(total[p], np.ones(n, bool))[0] for p in range(len(pods))]
    # node sets in the same call: per set an oracle over its sub-cluster (DeviceShare normalises over the set)
    sets = rng.random((3, n)) < 0.4
    sids = 1 + np.arange(len(pods)) % 3
    ev.node_sets_load(sets)
    got = ev.eval(pods, T0, node_sets=sids, node_scores=tids)
    for s in range(3):
        idx, grp = np.nonzero(sets[s])[0], np.nonzero(sids == s + 1)[0]
        want = sub_oracle(synth.config, cl, idx, devices=devs).eval(pods[grp], T0)
        for k in ("status", "reason", "la", "numa", "ds"):
            assert np.array_equal(got[k][np.ix_(grp, idx)], want[k]), (s, k)
        total = with_offset(want["total"], off[np.ix_(grp, idx)])
        assert np.array_equal(got["total"][np.ix_(grp, idx)], total), s
        wb = [masked_argmax(t, np.ones(len(idx), bool))[0] for t in total]
        assert got["best"][grp].tolist() == [int(idx[b]) if b >= 0 else -1 for b in wb], s
        out = np.setdiff1d(np.arange(n), idx)
        assert (got["reason"][np.ix_(grp, out)] == abi.REASON_NODE_SET).all()
        assert (got["total"][np.ix_(grp, out)] == -1).all()


def test_eval_numa_policy_pairs(gpu):
    """A context with NUMA topology policy nodes: the pairs whose evaluation is finished by the NUMA fallback kernels,
    after the first pass, take the offset too."""
    n = 400
    cl = synth.make_cluster(n, synth.BASE_SEED + 9381, amplified_fraction=0.3)
    zones = synth.make_numa(cl, synth.BASE_SEED + 9382, zone_counts=(1, 2, 4, 8), status_fraction=0.4)
    pods = synth.make_numa_pods(48, synth.BASE_SEED + 9383, policy_fraction=0.6)
    ev, o = both(synth.config(n), cl)
    synth.load_numa(ev, zones)
    synth.load_numa(o, zones)
    rng = np.random.default_rng(synth.BASE_SEED + 9384)
    tables = rng.integers(0, 201, (3, n))
    ids = rng.integers(0, 4, len(pods))
    ev.node_scores_load(tables)
    got, want = ev.eval(pods, T0, node_scores=ids), o.eval(pods, T0)
    assert ev.numa_deferred() > 0
    for k in ("status", "reason", "la", "numa"):
        assert np.array_equal(got[k], want[k]), k
    total = with_offset(want["total"], offsets_of(tables, ids, n))
    assert np.array_equal(got["total"], total)
    assert got["best"].tolist() == [masked_argmax(total[p], np.ones(n, bool))[0] for p in range(len(pods))]


# ---- 3 - 5, 7: ke_schedule against the lock-step reference ------------------------------------------------------------
_REF = {}


def _base():
    if "n" not in _REF:
        n = 150
        cl = synth.make_cluster(n, synth.BASE_SEED + 9321)
        pods = synth.make_pods(600, synth.BASE_SEED + 9322)
        o = Oracle(synth.config(n), n)
        synth.load_into(o, cl)
        _REF.update(n=n, cl=cl, pods=pods, plain=o.schedule(pods, T0))
    return _REF


def _case(name):
    """The tables, ids (and sets) of a named case with its reference, computed once."""
    r = _base()
    if name not in _REF:
        n, pods = r["n"], r["pods"]
        rng = np.random.default_rng(synth.BASE_SEED + 9323)
        ids = rng.integers(0, 5, len(pods))
        sets = sids = elig = None
        if name == "wide":
            tables = rng.integers(0, 201, (4, n))
        elif name == "ties":
            tables = rng.integers(0, 4, (4, n))
        elif name == "cap":
            tables = np.where(rng.random((4, n)) < 0.3, CAP, 0)
        else:  # "sets": 4 random sets next to 4 tables, independent ids
            tables = rng.integers(0, 201, (4, n))
            sets = rng.random((4, n)) < 0.4
            sids = rng.integers(0, 5, len(pods))
            elig = np.concatenate([np.ones((1, n), bool), sets])[sids]
        o = Oracle(synth.config(n), n)
        synth.load_into(o, r["cl"])
        want = lockstep_scores(o, pods, offsets_of(tables, ids, n), elig)
        _REF[name] = dict(tables=tables, ids=ids, sets=sets, sids=sids, elig=elig, want=want)
    return r, _REF[name]


def _ctx(r, c, batch):
    ev = Evaluator(synth.config(r["n"], pod_batch=batch))
    synth.load_into(ev, r["cl"])
    ev.node_scores_load(c["tables"])
    if c["sets"] is not None:
        ev.node_sets_load(c["sets"])
    return ev


@pytest.mark.parametrize("pipelined", [True, False], ids=["pipelined", "serial"])
@pytest.mark.parametrize("batch", [1, 7, 64])
@pytest.mark.parametrize("values", ["wide", "ties"])
def test_schedule_lockstep(gpu, values, batch, pipelined):
    r, c = _case(values)
    # the offsets move most placements: a site that drops them cannot pass
    assert int((c["want"][0] != r["plain"][0]).sum()) >= 300
    ev = _ctx(r, c, batch)
    ev.set_pipeline(pipelined)
    got = ev.schedule(r["pods"], T0, node_scores=c["ids"])
    assert_placed(got, c["want"])
    assert ev.check_records(T0) == 0
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)


def test_schedule_cap_edge(gpu):
    r, c = _case("cap")
    s = c["want"][1]
    # keys on both sides of bit 31 (score + 1 >= 512) and of the u16 half-range in one select
    assert int((s >= 511).sum()) >= 100 and int(((s >= 0) & (s < 511)).sum()) >= 100, (int((s >= 511).sum()), int(s.max()))
    ev = _ctx(r, c, 64)
    got = ev.schedule(r["pods"], T0, node_scores=c["ids"])
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, c["want"])
    assert ev.check_records(T0) == 0


@pytest.mark.parametrize("batch", [7, 64])
def test_schedule_sets_and_scores(gpu, batch):
    r, c = _case("sets")
    ev = _ctx(r, c, batch)
    got = ev.schedule(r["pods"], T0, node_sets=c["sids"], node_scores=c["ids"])
    assert_placed(got, c["want"])
    placed = got[0] >= 0
    assert placed.sum() > 300 and c["elig"][np.nonzero(placed)[0], got[0][placed]].all()
    assert ev.check_records(T0) == 0


def test_submit_ahead_with_scores(gpu):
    r, c = _case("wide")
    pods, ids = r["pods"], c["ids"]
    ev = _ctx(r, c, 64)
    chosen, score, prev = [], [], None
    for a in range(0, len(pods), 100):  # one call kept in flight
        t = ev.submit(pods[a:a + 100], T0, node_scores=ids[a:a + 100])
        if prev is not None:
            ch, sc = ev.wait(prev)
            chosen.append(ch), score.append(sc)
        prev = t
    ch, sc = ev.wait(prev)
    chosen.append(ch), score.append(sc)
    got = (np.concatenate(chosen), np.concatenate(score))
    assert_placed(got, c["want"])
    single = _ctx(r, c, 64).schedule(pods, T0, node_scores=ids)
    assert np.array_equal(got[0], single[0]) and np.array_equal(got[1], single[1])
    assert ev.check_records(T0) == 0


# ---- 6: ext resources (the EXT instantiations): a constant offset shifts the score and moves no placement -------------
def test_schedule_ext_resources_constant_shift(gpu):
    n = 150
    cfg = synth.ext_config(synth.config(n, pod_batch=64))
    cap = 1022 - 100 * (cfg.weight_loadaware + cfg.weight_numa + cfg.weight_deviceshare + cfg.ext.weight_fitplus +
                        cfg.ext.weight_sra + cfg.fit.weight)
    assert 0 < cap < CAP
    cl = synth.make_cluster(n, synth.BASE_SEED + 9351)
    tables = synth.make_node_resources(cl, synth.BASE_SEED + 9352)
    pods = synth.add_pod_xres(synth.make_pods(600, synth.BASE_SEED + 9353), synth.BASE_SEED + 9354)
    ev, o = both(cfg, cl)
    synth.load_node_resources(ev, tables)
    synth.load_node_resources(o, tables)
    c = np.array([0, 5, 100, cap, 37], np.int64)
    ids = np.random.default_rng(synth.BASE_SEED + 9355).integers(0, len(c) + 1, len(pods))
    shift = np.concatenate([[0], c])[ids]
    with pytest.raises(KoordEvalError) as e:  # this context's cap, not synth.config's
        ev.node_scores_load(np.full((1, n), cap + 1))
    assert e.value.code == abi.ERR_UNSUPPORTED and str(cap) in str(e.value)
    ev.node_scores_load(np.repeat(c[:, None], n, axis=1))
    c0, s0 = o.schedule(pods, T0)
    assert (c0 >= 0).sum() > 300
    got = ev.schedule(pods, T0, node_scores=ids)
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, (c0, np.where(c0 >= 0, s0 + shift, -1).astype(np.int32)))
    assert ev.check_records(T0) == 0


# ---- 8: table maintenance --------------------------------------------------------------------------------------------
def test_table_maintenance(gpu):
    n = 150
    cl = synth.make_cluster(n, synth.BASE_SEED + 9361)
    ev, o = both(synth.config(n), cl)
    rng = np.random.default_rng(synth.BASE_SEED + 9362)
    tables = rng.integers(0, 101, (2, n))
    ev.node_scores_load(tables)
    q = [synth.make_pods(40, synth.BASE_SEED + 9363 + i, key_base=9_300_000_000 + 1000 * i) for i in range(5)]
    ids = np.array([1, 2] * 20)
    got = ev.schedule(q[0], T0, node_scores=ids)
    assert_placed(got, lockstep_scores(o, q[0], offsets_of(tables, ids, n)))
    # one node's column raised to the cap in table 1: the next call places table 1's pods there first
    x = int(np.argmin(tables[0]))
    tables[0, x] = CAP
    ev.node_scores_set(x, tables[:, x])
    got = ev.schedule(q[1], T0, node_scores=ids)
    want = lockstep_scores(o, q[1], offsets_of(tables, ids, n))
    first = int(np.nonzero(ids == 1)[0][0])
    assert want[0][first] == x and got[0][first] == x
    assert_placed(got, want)
    # lowered back, another node patched in the same round
    y = (x + 71) % n
    tables[0, x], tables[1, y] = 0, 100
    ev.node_scores_set(x, tables[:, x])
    ev.node_scores_set(y, tables[:, y])
    got = ev.schedule(q[2], T0, node_scores=ids)
    assert_placed(got, lockstep_scores(o, q[2], offsets_of(tables, ids, n)))
    assert ev.check_records(T0) == 0
    # a table over the first 64 nodes only: nodes at or beyond 64 get offset 0
    short = rng.integers(50, 201, (1, 64))
    ev.node_scores_load(short, n_nodes=64)
    ones = np.ones(40, np.int32)
    got = ev.schedule(q[3], T0, node_scores=ones)
    want = lockstep_scores(o, q[3], offsets_of(short, ones, n))
    assert_placed(got, want)
    # n_tables = 0: the ids are refused, a plain call is the oracle's
    ev.node_scores_load([])
    with pytest.raises(KoordEvalError) as e:
        ev.pod_node_scores([1] * 40)
    assert e.value.code == abi.ERR_INVALID
    c1, s1 = ev.schedule(q[4], T0)
    c0, s0 = o.schedule(q[4], T0)
    assert np.array_equal(c1, c0) and np.array_equal(s1, s0)
    dev, host = ev.debug_rows(T0)
    assert np.array_equal(dev, host)


# ---- 9: refusals -----------------------------------------------------------------------------------------------------
def _refused_then_clean(ev, fresh, pods, ids):
    ev.pod_node_scores(ids)
    with pytest.raises(KoordEvalError) as e:
        ev.schedule(pods, T0)
    assert e.value.code == abi.ERR_UNSUPPORTED and "node scores" in str(e.value)
    plain = synth.make_pods(200, synth.BASE_SEED + 9379)
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
        ev.node_scores_load(np.full((1, n), 50))
        out.append(ev)
    return out


def test_refused_deviceshare_pod(gpu):
    ev, fresh = _pair(120, 9371, devices=True)
    pods = synth.make_ds_pods(8, synth.BASE_SEED + 9373, device_fraction=1.0)
    _refused_then_clean(ev, fresh, pods, [1] * 8)


def test_refused_numa_policy_pod(gpu):
    ev, fresh = _pair(120, 9374)
    pods = synth.make_pods(8, synth.BASE_SEED + 9375)
    pods["numa_topology_policy"][3] = abi.NUMA_POLICY_SINGLE_NUMA_NODE
    _refused_then_clean(ev, fresh, pods, [0, 0, 1, 0, 0, 0, 0, 0])


def test_refused_sharded_context(gpu):
    ev, fresh = _pair(120, 9376, shard=True)
    pods = synth.make_pods(8, synth.BASE_SEED + 9377)
    _refused_then_clean(ev, fresh, pods, [1] * 8)
    ev.pod_node_scores([1] * 8)
    with pytest.raises(KoordEvalError) as e:
        ev.eval(pods, T0)
    assert e.value.code == abi.ERR_UNSUPPORTED and "node scores" in str(e.value)
